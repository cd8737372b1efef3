"""The arithmetic of memo_ec_check_batch (memo_amd/csrc/check_plan.h: the
scratch layout, the strides of the MAC launch and the offsets of a launch
span), walked by a stand-alone C++ program built with the host sanitizers
(tests/check_plan_check.cc: its own main, nothing loaded into Python), so
every offset the check's kernels are handed is judged on the CPU before a
GPU sees one.

The program runs every shape of the device tests (SHAPES of
tests/test_check_reference.py) and the same shapes with n = 1, each with
launch spans cut at a tile limit of 3 and at the 31-bit grid limit."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_check_reference import SHAPES
from test_ragged_plan import compiler

SRC = os.path.join(ROOT, "tests", "check_plan_check.cc")
HDR = os.path.join(ROOT, "memo_amd", "csrc", "check_plan.h")


def lines(shapes):
    return "".join("%d %d %d %d %d\n" % s for s in shapes)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("check_plan") / "check_plan_check")
    subprocess.check_call(compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                        SRC, "-o", exe])
    return exe


def run(program, shapes):
    r = subprocess.run([program], input=lines(shapes), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok %d" % len(shapes), r.stdout[-2000:]


def test_every_device_test_shape(program):
    run(program, SHAPES)


def test_one_block_of_every_shape(program):
    run(program, [(k, m, x, S, 1) for (k, m, x, S, n) in SHAPES])


def test_span_and_region_edges(program):
    """The span test's own shape, many small blocks (a span of one block each
    under the limit of 3, one span at the grid limit), regions whose sizes
    are exact multiples of 256, and the smallest and widest codes."""
    run(program, [(10, 4, 4, 4160, 5), (16, 4, 3, 64, 130), (16, 4, 4, 64, 256), (2, 1, 1, 64, 128),
                  (64, 16, 1, 128, 7), (1, 1, 1, 64, 1)])


def test_header_has_no_gpu_include():
    txt = open(HDR).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>"]


def test_program_notices_a_wrong_spare_base(program, tmp_path):
    """The check has teeth: over a header whose spares start one shard late,
    (k + 1) * S instead of k * S, the same program must fail."""
    hdr = open(HDR).read()
    broken = hdr.replace("s.spares = (uint64_t)k * S;", "s.spares = (uint64_t)(k + 1) * S;")
    assert broken != hdr
    d = tmp_path / "memo_amd" / "csrc"
    d.mkdir(parents=True)
    (d / "check_plan.h").write_text(broken)
    t = tmp_path / "tests"
    t.mkdir()
    shutil.copy(SRC, t / "check_plan_check.cc")
    exe = str(tmp_path / "broken")
    subprocess.check_call([compiler()[0], "-std=c++17", "-O1", str(t / "check_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe], input=lines(SHAPES[:1]), capture_output=True, text=True)
    assert r.returncode != 0, r.stdout[-2000:]
    assert "FAILED" in r.stdout

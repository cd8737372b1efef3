"""The arithmetic of memo_ec_correct_batch (memo_amd/csrc/correct_plan.h: the
scratch behind the check's, the list entries, the work items and every offset
a work item reads or writes), walked by a stand-alone C++ program built with
the host sanitizers (tests/correct_plan_check.cc: its own main, nothing loaded
into Python), so every offset the correction's kernels use is judged on the
CPU before a GPU sees one.

The program runs every shape of the device tests (correct_cases.GPU_SHAPES)
and the same shapes with n = 1."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from correct_cases import GPU_SHAPES
from test_ragged_plan import compiler

SRC = os.path.join(ROOT, "tests", "correct_plan_check.cc")
HDR = os.path.join(ROOT, "memo_amd", "csrc", "correct_plan.h")
# S == 0 and x == 1 never reach the correction's kernels
WALKED = sorted({s for s in GPU_SHAPES if s[3] > 0})


def lines(shapes):
    return "".join("%d %d %d %d %d\n" % s for s in shapes)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("correct_plan") / "correct_plan_check")
    subprocess.check_call(compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                        SRC, "-o", exe])
    return exe


def run(program, shapes):
    r = subprocess.run([program], input=lines(shapes), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok %d" % len(shapes), r.stdout[-2000:]


def test_every_device_test_shape(program):
    run(program, WALKED)


def test_one_block_of_every_shape(program):
    run(program, sorted({(k, m, x, S, 1) for (k, m, x, S, n) in WALKED}))


def test_region_and_tile_edges(program):
    """Lists whose sizes are exact multiples of 256 bytes, a shard of exactly
    one tile, one byte column more, and the widest code."""
    run(program, [(3, 2, 2, 64, 32), (3, 2, 2, 64, 33), (10, 4, 2, 4096, 3), (10, 4, 2, 4096 + 64, 3),
                  (64, 16, 16, 128, 7), (1, 2, 2, 64, 1), (16, 4, 4, 8192, 2)])


def test_header_includes_no_gpu_header():
    txt = open(HDR).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>", '"check_plan.h"']


def build_broken(tmp_path, old, new):
    hdr = open(HDR).read()
    broken = hdr.replace(old, new)
    assert broken != hdr
    d = tmp_path / "memo_amd" / "csrc"
    d.mkdir(parents=True)
    (d / "correct_plan.h").write_text(broken)
    shutil.copy(os.path.join(ROOT, "memo_amd", "csrc", "check_plan.h"), d / "check_plan.h")
    t = tmp_path / "tests"
    t.mkdir()
    shutil.copy(SRC, t / "correct_plan_check.cc")
    exe = str(tmp_path / "broken")
    subprocess.check_call([compiler()[0], "-std=c++17", "-O1", str(t / "correct_plan_check.cc"), "-o", exe])
    return exe


def test_program_notices_a_target_among_the_inputs(program, tmp_path):
    """The check has teeth: over a header whose inputs are the basis as it
    stands (a basis target reads the wrong shard it is about to replace), the
    same program must fail."""
    exe = build_broken(tmp_path, "return (q < k && j == q) ? k : j;", "return (q < k && j == q) ? j : j;")
    r = subprocess.run([exe], input=lines(WALKED[:1]), capture_output=True, text=True)
    assert r.returncode != 0, r.stdout[-2000:]
    assert "FAILED" in r.stdout


def test_program_notices_a_short_tile_count(program, tmp_path):
    """... and over a header that rounds the tiles of a shard down."""
    exe = build_broken(tmp_path, "return (S + kTileBytes - 1) / kTileBytes;", "return S / kTileBytes + (S < kTileBytes);")
    r = subprocess.run([exe], input=lines([(10, 4, 2, 4160, 3)]), capture_output=True, text=True)
    assert r.returncode != 0, r.stdout[-2000:]
    assert "FAILED" in r.stdout

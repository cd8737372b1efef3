"""The arithmetic of memo_ec_correct_pair_batch
(memo_amd/csrc/correct_pair_plan.h: the scratch behind the single
correction's, the pair entries, the k input positions of a pair of targets,
the rows their coefficients come from and every offset a work item reads or
writes), walked by a stand-alone C++ program built with the host sanitizers
(tests/correct_pair_plan_check.cc: its own main, nothing loaded into Python),
so every offset the pair correction's kernels use is judged on the CPU before
a GPU sees one.

The program runs every shape of the device tests
(correct_pair_cases.GPU_SHAPES), the same shapes with n = 1, and -- offsets
only -- blocks past 2^32 bytes into `have` and shards past 2^31 bytes, which
no device test of this call reaches."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from correct_pair_cases import GPU_SHAPES
from test_ragged_plan import compiler

SRC = os.path.join(ROOT, "tests", "correct_pair_plan_check.cc")
CSRC = os.path.join(ROOT, "memo_amd", "csrc")
HDR = os.path.join(CSRC, "correct_pair_plan.h")
# x <= 2 and S == 0 never reach the pair correction's kernels
WALKED = sorted({s for s in GPU_SHAPES if s[3] > 0 and s[2] >= 3})


def lines(shapes):
    return "".join(" ".join(str(v) for v in s) + "\n" for s in shapes)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("correct_pair_plan") / "correct_pair_plan_check")
    subprocess.check_call(compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                        SRC, "-o", exe])
    return exe


def run(program, shapes):
    r = subprocess.run([program], input=lines(shapes), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok %d" % len(shapes), r.stdout[-2000:]


def test_every_device_test_shape(program):
    assert len(WALKED) > 30
    run(program, WALKED)


def test_one_block_of_every_shape(program):
    run(program, sorted({(k, m, x, S, 1) for (k, m, x, S, n) in WALKED}))


def test_region_and_tile_edges(program):
    """Lists whose sizes are exact multiples of 256 bytes, a shard of exactly
    one tile, one byte column more, the narrowest and the widest code."""
    run(program, [(3, 3, 3, 64, 32), (3, 3, 3, 64, 33), (10, 4, 4, 4096, 3), (10, 4, 4, 4096 + 64, 3),
                  (64, 16, 16, 128, 7), (1, 3, 3, 64, 1), (16, 4, 4, 8192, 2), (2, 16, 16, 64, 2)])


def test_offsets_past_32_bits(program):
    """Block b with b * (k + x) * S past 2^32, and shards past 2^31 bytes: every
    input, target and row offset against a 128-bit product."""
    run(program, [("big", 10, 4, 4, 4096, 1 << 17),            # b * 14 * 4096 = 7.5 GiB
                  ("big", 10, 4, 4, 64, (1 << 32) + 5),        # the block number itself past 2^32
                  ("big", 4, 4, 4, (1 << 31) + 64, 3),         # S past 2^31
                  ("big", 64, 16, 16, (1 << 32) - 64, 1 << 10),
                  ("big", 10, 4, 3, 1 << 20, (1 << 30) // 13)])


def test_header_includes_the_single_plan_only():
    txt = open(HDR).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>", '"correct_plan.h"']


def build_broken(tmp_path, old, new):
    hdr = open(HDR).read()
    assert hdr.count(old) == 1
    d = tmp_path / "memo_amd" / "csrc"
    d.mkdir(parents=True)
    (d / "correct_pair_plan.h").write_text(hdr.replace(old, new))
    for name in ("check_plan.h", "correct_plan.h"):
        shutil.copy(os.path.join(CSRC, name), d / name)
    t = tmp_path / "tests"
    t.mkdir()
    shutil.copy(SRC, t / "correct_pair_plan_check.cc")
    exe = str(tmp_path / "broken")
    subprocess.check_call([compiler()[0], "-std=c++17", "-O1", str(t / "correct_pair_plan_check.cc"), "-o", exe])
    return exe


def test_program_notices_a_target_among_the_inputs(program, tmp_path):
    """The check has teeth: over a header in which a basis target is read as
    its own input, the same program must fail."""
    exe = build_broken(tmp_path, "if (j == qa) return k + clean_row(0, qa, qb, k);", "if (j == qa) return j;")
    r = subprocess.run([exe], input=lines(WALKED[:1]), capture_output=True, text=True)
    assert r.returncode != 0, r.stdout[-2000:]
    assert "FAILED" in r.stdout


def test_program_notices_one_clean_row_used_twice(program, tmp_path):
    """... and over a header in which the second clean row equals the first
    (two basis targets would read one spare twice, and the 2 x 2 system of
    their coefficients would be singular)."""
    exe = build_broken(tmp_path, "  if (i == 0) return r;\n  ++r;\n", "  if (i == 0) return r;\n")
    r = subprocess.run([exe], input=lines(WALKED[:1]), capture_output=True, text=True)
    assert r.returncode != 0, r.stdout[-2000:]
    assert "FAILED" in r.stdout

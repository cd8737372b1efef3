"""The GPU-free staging layout of host-memory calls (memo_amd/csrc/
ragged_plan.h: stage::Plan and the shared wave rule), checked by a stand-alone
C++ program built with the host sanitizers (tests/stage_plan_check.cc: its own
main, nothing loaded into Python).

For the size lists A-E, F1, F2 and the edge lists, codes (10,4) and (3,2),
pinned and pageable callers and pipeline batches of 4 KiB and 64 KiB (and the
single wave of a zero-copy call) the program lays out the waves the entry
points build and checks that every extent lies inside the slot sizes
reported, that no two extents of a wave overlap, that shard extents are
16-byte aligned, that a pinned caller's host slot holds no payload and that
the slot is no larger than (k + r) * tmax (encode, rebuild; plus the staged
index bytes) or (k + m) * tmax + 4 * nmax (verify) plus alignment padding.
A list of equal sizes cut through the shared wave rule without a size array
gives exactly max(1, pipe / (per * S)) blocks per wave."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
import ragged_cases as RC
from test_ragged_plan import compiler

SRC = os.path.join(ROOT, "tests", "stage_plan_check.cc")
HDR = os.path.join(ROOT, "memo_amd", "csrc", "ragged_plan.h")

EDGE = [("empty", []), ("zeros", [0, 0, 0]), ("lead0", [0, 0, 64, 0, 4096, 0]),
        ("edge", [4096, 64, 64, 3968, 0, 64]), ("big", [4096 * 5 + 64, 64, 4096 * 2])]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_plan") / "stage_plan_check")
    subprocess.check_call(compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                        SRC, "-o", exe])
    return exe


def run(program, lists):
    text = "".join("%s %s\n" % (name, " ".join(map(str, sz))) for name, sz in lists)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok %d" % len(lists), r.stdout[-2000:]


def test_lists_A_to_F(program):
    run(program, [(n, RC.LISTS[n]) for n in ("A", "B", "C", "D", "D1", "E", "F1", "F2")])


def test_edge_lists(program):
    run(program, EDGE)


def test_program_notices_a_wrong_offset(program, tmp_path):
    """The check has teeth: the same program over a header that advances the
    slot offset by half an extent must fail."""
    hdr = open(HDR).read()
    broken = hdr.replace("at += e.bytes;", "at += e.bytes / 2;")
    assert broken != hdr
    d = tmp_path / "memo_amd" / "csrc"
    d.mkdir(parents=True)
    (d / "ragged_plan.h").write_text(broken)
    t = tmp_path / "tests"
    t.mkdir()
    shutil.copy(SRC, t / "stage_plan_check.cc")
    exe = str(tmp_path / "broken")
    subprocess.check_call([compiler()[0], "-std=c++17", "-O1", str(t / "stage_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe], input="B 4096 4096 4096\n", capture_output=True, text=True)
    assert r.returncode != 0

"""The capped tiles of the ragged rebuild (memo_amd/csrc/ragged_plan.h:
rows_cap, rows_index_counts, build_rows_index, cut_rows_spans), checked by a
stand-alone C++ program built with the host sanitizers
(tests/ragged_rebuild_plan_check.cc: its own main, nothing loaded into
Python).

For each size list and caps 1, 2, 9, 24, 38 and 64 the program compares the
tile descriptors with a brute-force walk over the columns: the tiles
partition the columns in order, none has more than 256 columns or more than
cap blocks, a short tile other than the last ends on a block boundary with
exactly cap blocks, a host restatement of the kernel's lane search finds
every column's block and size, and span cuts by tile limit cover every block
once."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
import ragged_cases as RC
from test_ragged_plan import compiler

SRC = os.path.join(ROOT, "tests", "ragged_rebuild_plan_check.cc")
G = [64, 0, 0, 128, 0, 64, 0, 4160, 0, 0, 64]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ragged_rebuild_plan") / "ragged_rebuild_plan_check")
    subprocess.check_call(compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                        SRC, "-o", exe])
    return exe


def run(program, lists):
    text = "".join("%s %s\n" % (name, " ".join(map(str, sz))) for name, sz in lists)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok %d" % len(lists), r.stdout[-2000:]


def test_shared_lists(program):
    run(program, [(n, sz) for n, sz in RC.LISTS.items()] + [("G", G)])


def test_lists_around_each_cap(program):
    """c blocks of 64 bytes and one of two tiles, c one below, at and one
    above each cap the program runs."""
    run(program, [("H%d" % c, [64] * c + [8192]) for cap in (1, 2, 9, 24, 38, 64)
                  for c in (cap - 1, cap, cap + 1)])


def test_edge_lists(program):
    run(program, [("empty", []), ("zeros", [0, 0, 0]), ("lead0", [0, 0, 64, 0, 4096, 0]),
                  ("edge", [4096, 64, 64, 3968, 0, 64]), ("big", [4096 * 5 + 64, 64, 4096 * 2]),
                  ("tail", [4096 * 3 + 192] + [64] * 70 + [4096 - 64, 128])])


def test_program_notices_a_wrong_cap(program, tmp_path):
    """The check has teeth: over a header whose tiles ignore the cap the
    same program must fail."""
    hdr = open(os.path.join(ROOT, "memo_amd", "csrc", "ragged_plan.h")).read()
    broken = hdr.replace("if (q + cap <= nq && coff[q + cap] < end) end = coff[q + cap];", "")
    assert broken != hdr
    d = tmp_path / "memo_amd" / "csrc"
    d.mkdir(parents=True)
    (d / "ragged_plan.h").write_text(broken)
    t = tmp_path / "tests"
    t.mkdir()
    shutil.copy(SRC, t / "ragged_rebuild_plan_check.cc")
    exe = str(tmp_path / "broken")
    subprocess.check_call([compiler()[0], "-std=c++17", "-O1", str(t / "ragged_rebuild_plan_check.cc"),
                           "-o", exe])
    r = subprocess.run([exe], input="A %s\n" % " ".join(["64"] * 65), capture_output=True, text=True)
    assert r.returncode != 0

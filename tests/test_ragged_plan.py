"""The GPU-free planning of ragged batches (memo_amd/csrc/ragged_plan.h),
checked by a stand-alone C++ program built with the host sanitizers
(tests/ragged_plan_check.cc: its own main, nothing loaded into Python).

For the size lists A-E the program compares the per-tile descriptors, and a
host restatement of the kernels' lane search, with a brute-force walk over
the columns; cuts launch spans under tile limits 1, 2, 3 and pipeline waves
under 4 KiB and 64 KiB and checks that they cover every block once, cut only
on block boundaries, respect the limit unless a single block exceeds it and
are never cut early; and feeds prefix_sums each class of invalid size."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
import ragged_cases as RC

SRC = os.path.join(ROOT, "tests", "ragged_plan_check.cc")


def compiler():
    """The host compiler and the flags that link the sanitizer runtimes into
    the program itself (clang does by default), so it runs the same whatever
    else the process environment loads."""
    for name in ("g++", "clang++", "c++"):
        cxx = shutil.which(name)
        if cxx:
            return [cxx] + (["-static-libasan", "-static-libubsan"] if name == "g++" else [])
    raise AssertionError("no host C++ compiler")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ragged_plan") / "ragged_plan_check")
    subprocess.check_call(compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                        SRC, "-o", exe])
    return exe


def run(program, lists):
    text = "".join("%s %s\n" % (name, " ".join(map(str, sz))) for name, sz in lists)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok %d" % len(lists), r.stdout[-2000:]


def test_lists_A_to_E(program):
    run(program, [(n, RC.LISTS[n]) for n in ("A", "B", "C", "D", "D1", "E")])


def test_edge_lists(program):
    """Empty and all-zero batches, zero sizes first and between straddling
    blocks, a block ending exactly on a tile edge followed by small ones."""
    run(program, [("empty", []), ("zeros", [0, 0, 0]), ("lead0", [0, 0, 64, 0, 4096, 0]),
                  ("edge", [4096, 64, 64, 3968, 0, 64]), ("uniform", RC.F1), ("uniform2", RC.F2),
                  ("big", [4096 * 5 + 64, 64, 4096 * 2])])


def test_program_notices_a_wrong_index(program, tmp_path):
    """The check has teeth: the same program over a header whose tile walk
    is off by one must fail."""
    hdr = open(os.path.join(ROOT, "memo_amd", "csrc", "ragged_plan.h")).read()
    broken = hdr.replace("while (coff[q + 1] <= c) ++q;", "while (coff[q + 1] < c) ++q;")
    assert broken != hdr
    d = tmp_path / "memo_amd" / "csrc"
    d.mkdir(parents=True)
    (d / "ragged_plan.h").write_text(broken)
    t = tmp_path / "tests"
    t.mkdir()
    shutil.copy(SRC, t / "ragged_plan_check.cc")
    exe = str(tmp_path / "broken")
    subprocess.check_call([compiler()[0], "-std=c++17", "-O1", str(t / "ragged_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe], input="B 4096 4096 4096\n", capture_output=True, text=True)
    assert r.returncode != 0

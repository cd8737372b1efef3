"""The GF(2^8) algebra of memo_ec_check_pair_batch
(memo_amd/csrc/check_pair_logic.h: span membership and the rank of an x x 3
matrix, the text check_pair_kernel compiles) run on the CPU by a stand-alone
C++ program built with the host sanitizers (tests/check_pair_logic_check.cc:
its own main and table multiply, nothing loaded into Python), and held to the
host reference on the blocks of tests/test_check_pair_reference.py, the
(64,16,16) limit included."""
import os
import subprocess

import numpy as np
import pytest

import check_pair_cases as C
from conftest import ROOT
from test_check_pair_reference import AMBIGUOUS, SHAPES
from test_ragged_plan import compiler

SRC = os.path.join(ROOT, "tests", "check_pair_logic_check.cc")
HDR = os.path.join(ROOT, "memo_amd", "csrc", "check_pair_logic.h")
LIMIT = (64, 16, 16, 64)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("check_pair_logic") / "check_pair_logic_check")
    subprocess.check_call(compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                        SRC, "-o", exe])
    return exe


def judge(program, k, m, x, idx, have):
    """Feed every block the check leaves unlocated to the program; its
    answers must be the reference's: the one explaining pair of positions, or
    none.  Returns (located, unlocated)."""
    from memo_amd import check_pair_ref as P, check_ref as R
    text, want = [], []
    for b in range(idx.shape[0]):
        word = R.check_block(k, m, idx[b], have[b], x)
        if not P.qualifies(word, x, have.shape[2]):
            continue
        d, syn = P.syndromes(k, m, idx[b], have[b], x)
        s = np.unique(syn[:, syn.any(axis=0)].T, axis=0)
        text.append("%d %d %d\n%s\n%s\n" % (k, x, len(s), " ".join(map(str, d.reshape(-1))),
                                          " ".join(map(str, s.reshape(-1)))))
        pairs = P.explaining_pairs(k, m, idx[b], have[b], x)
        want.append("%d %d" % pairs[0] if len(pairs) == 1 else "none")
    r = subprocess.run([program], input="".join(text), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "ok %d" % len(want), r.stdout[-2000:]
    assert out[:-1] == want
    return sum(w != "none" for w in want), want.count("none")


@pytest.mark.parametrize("shape", SHAPES + [(10, 4, 3, 448), LIMIT],
                         ids=lambda s: "rs%d_%d_x%d_S%d" % s)
def test_program_agrees_with_the_reference(program, shape):
    k, m, x, S = shape
    idx, have, _ = C.batch(shape)
    located, unlocated = judge(program, k, m, x, idx, have)
    assert located >= (9 if x >= 4 else 6) and unlocated >= 1  # the pairs; the three wrong shards


def test_x3_ambiguous_blocks(program):
    k, m, x, S, n, seed = AMBIGUOUS
    idx, have, _ = C.same_offset_blocks(k, m, x, S, n, seed)
    located, unlocated = judge(program, k, m, x, idx, have)
    assert located >= 1 and unlocated >= 1


def test_header_includes_are_standard_only():
    txt = open(HDR).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes == ["<cstdint>"]
    assert "hip" not in " ".join(includes)

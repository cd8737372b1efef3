"""The check family swept by position on the MI355X: memo_ec_check_batch,
memo_ec_check_pair_batch and memo_ec_correct_batch on batches in which every
byte offset, lane, wave and stride round of a shard, every position of the
code, every pair of positions and every grid round decides some block's word.

tests/test_gpu_check.py, test_gpu_correct.py and test_gpu_check_pair.py put
the wrong bytes at byte 0, at byte S - 1 and at a random offset or two, and
choose the wrong positions with a seeded rng; no batch of theirs has more than
4099 blocks.  So a dropped dword, lane, wave or stride round of
check_locate_kernel's candidate set (two 32-bit halves ANDed over 64 lanes, 4
waves and a stride loop) or of one of check_pair_kernel's three walks, a
position >= 32 or >= 64, a pair late in nth_pair, a second grid round of the
three kernels with a capped grid, and a work-item range of gf_correct_kernel
that begins or ends inside a list entry are caught there only by luck, or not
at all.  Here every one of them decides a word, as
tests/test_gpu_verify_sweep.py does for the parity verify.

The batches are the families of tests/check_sweep_cases.py: every expected
word is stated by construction, and tests/test_check_sweep_cases.py holds
every one of them bit for bit to the host references (check_ref,
check_pair_ref, correct_ref) without a GPU.  There is no tolerance.  Every
buffer of every call sits between guards (tests/guarded.py).

  A  memo_ec_check_batch       A1 every byte  A2 a disqualifying byte in every
                               lane  A3 every position of (64,16,16)  A4 all 64
                               words of a round  A5 the second grid round
  B  memo_ec_check_pair_batch  B1 every pair  B2 the limit shape's pairs  B3-B5
                               walks 1-3 in every lane  B6 the rounds
  C  memo_ec_correct_batch     C1 ranges cut inside entries  C2 located and
                               unlocated interleaved  C3 the list kernel's
                               second round  C4 sweep, mend, check again"""
import numpy as np
import pytest

import check_sweep_cases as W
import correct_cases as CC
from correct_cases import CORRECTED, single_batch
from guarded import Guarded
from test_gpu_bounds import Cases
from test_gpu_check import run_check
from test_gpu_check_pair import run_pair
from test_gpu_correct import inout, run_correct

pytestmark = pytest.mark.gpu


def ids(shape):
    return "rs%d_%d_x%d_S%d" % tuple(shape)


def check_family(codec, label, f):
    k, m, x, S = f.shape
    n, idx, have, want = W.full(f)
    cases = Cases()
    run_check(codec, cases, label, k, m, x, S, n, idx, have, want)
    cases.done()


def pair_family(codec, label, f):
    k, m, x, S = f.shape
    n, idx, have, want = W.full(f)
    cases = Cases()
    run_pair(codec, cases, label, k, m, x, S, n, idx, have, want)
    cases.done()


def correct_family(codec, label, f):
    k, m, x, S = f.shape
    n, idx, have, want = W.full(f)
    mended = W.after(f)
    cases = Cases()
    run_correct(codec, cases, label, k, m, x, S, n, idx, have, want,
                mended if f.sel is None else mended[f.sel])
    cases.done()


# ------------------------------------------------------ A: memo_ec_check_batch
@pytest.mark.parametrize("part", W.A1_PARTS, ids=lambda p: "rs%d_%d_x%d_S%d_from%d" % (p[0] + (p[1],)))
def test_a1_every_byte_position(codec, part):
    """Block i is wrong at byte lo + i alone: every lane, dword and byte of
    gf_check_kernel's compare and every lane, wave and stride round of the
    locate pass decides one word.  S = 1088 is 272 dwords (256 lanes and a
    second stride round of 16); S = 4160, a quarter of its offsets a call,
    crosses a MAC tile edge.  The same buffers through the pair check give the
    same words: nothing qualifies."""
    (k, m, x, S), lo, hi = part
    f = W.every_byte(*part)
    n = hi - lo
    g = Guarded("device")
    hidx = g.input("have_idx", f.idx)
    hv = g.input("have", f.have.reshape(n, -1))
    g.output("check", 4 * n)
    g.output("pair", 4 * n)
    codec.check(k, m, hidx, hv, g.words("check"), x=x, S=S, n=n)
    codec.check_pair(k, m, hidx, hv, g.words("pair"), x=x, S=S, n=n)
    codec.synchronize()
    cases = Cases()
    cases.check("bytes %d..%d" % (lo, hi - 1), g, check=f.want, pair=f.want)
    cases.done()


def test_a2_disqualifying_byte_in_every_lane(codec):
    """(4,3,3,1088): in (a)-(c) the single byte of the second wrong basis
    shard empties the candidate set wherever it lies (x = 3), so a reduction
    that drops one lane's, wave's or stride round's set locates the first;
    (d) is located.  Wrong blocks odd, clean blocks even."""
    check_family(codec, "a-d", W.disqualifying_byte())


def test_a3_every_position_of_the_limit_shape(codec):
    """(64,16,16,64), n = 80, position b of block b wrong: every bit of the
    candidate set's lo / hi halves and both atomicAnd words, on the KMAX = 64
    body."""
    check_family(codec, "limit", W.every_limit_position())


def test_a4_all_64_words_of_a_round_flagged(codec):
    check_family(codec, "n=130", W.every_word_flagged())


def test_a5_second_grid_round(codec):
    """n = 2048 * 64 + 64 + 3 (42 MB): wrong blocks in the first and last word
    of round one's first and last workgroups and of round two's two, and an
    unlocated block inside round two; every other word is 0."""
    check_family(codec, "two rounds", W.check_second_round())


# ------------------------------------------------- B: memo_ec_check_pair_batch
@pytest.mark.parametrize("shape", W.B1_SHAPES, ids=ids)
def test_b1_every_pair_of_positions(codec, shape):
    """All C(k + x, 2) pairs, each at one offset (rank 1: the search over
    nth_pair) and at two (rank 2: the column test)."""
    pair_family(codec, "every pair", W.every_pair(shape))


def test_b2_limit_shape_pairs(codec):
    """(64,16,16,64): the column test's lanes sit in two waves, the rank-1
    search strides over 3160 pairs; named positions >= 64 and the pair 63/64."""
    pair_family(codec, "limit pairs", W.limit_pairs())


def test_b3_walk_1_in_every_lane(codec):
    """(10,4,4,1088): the only syndrome of block b is at byte b."""
    pair_family(codec, "walk 1", W.walk1())


@pytest.mark.parametrize("shape", W.B4_SHAPES, ids=ids)
def test_b4_walk_2_in_every_lane(codec, shape):
    """x = 3: a rank-1 block two pairs explain (the control: unlocated), and
    the same with the one syndrome off the line in dword w, for every w: it
    names the pair only when walk 2 finds that byte."""
    pair_family(codec, "walk 2", W.walk2(shape))


@pytest.mark.parametrize("shape", W.B5_SHAPES, ids=ids)
def test_b5_walk_3_in_every_lane(codec, shape):
    """Two whole shards wrong (the control names them), and a third wrong at
    one byte of dword w, for every w: rank 3, the check's word, unless walk 3
    misses that byte."""
    pair_family(codec, "walk 3", W.walk3(shape))


def test_b6_all_64_words_of_a_round_qualify(codec):
    pair_family(codec, "n=130", W.every_word_a_pair())


def test_b6_second_grid_round(codec):
    """(4,4,4,64), n = 2048 * 64 + 64 + 3 (67 MB): pair, single and
    three-wrong blocks at the boundaries of both rounds."""
    pair_family(codec, "two rounds", W.pair_second_round())


# ---------------------------------------------------- C: memo_ec_correct_batch
def test_c1_ranges_cut_inside_entries(codec):
    """(3,2,2,8256), n = 700, every block located: 3 tiles an entry (the last
    one 64 bytes), 2100 work items over 2048 workgroups, 2 each, so the ranges
    begin at tile 0, 2, 1, ... of successive entries and the images kept
    through `cur` are rebuilt mid-entry."""
    k, m, x, S, n = CC.SWEEP_RANGES
    idx, clean, have, words = single_batch(CC.SWEEP_RANGES)
    assert (words >> 24 == 1).all()
    cases = Cases()
    run_correct(codec, cases, "ranges", k, m, x, S, n, idx, have, words, clean)
    cases.done()


def test_c2_located_and_unlocated_interleaved(codec):
    """(10,4,3,4160), n = 24: only the located blocks' target shards change."""
    correct_family(codec, "interleaved", W.interleaved())


def test_c3_list_kernel_second_round(codec):
    """(3,2,2,64), n = 1024 * 256 + 256 + 3 (84 MB): located blocks at the
    boundaries of correct_list_kernel's two rounds, a wave of 64 located words
    and a wave with lane 63 alone; also the check's third grid round."""
    correct_family(codec, "two rounds", W.list_second_round())


@pytest.mark.parametrize("part", W.A1_QUARTERS, ids=lambda p: "rs%d_%d_x%d_S%d_from%d" % (p[0] + (p[1],)))
def test_c4_sweep_then_mend(codec, part):
    """A1's RS(10,4) batches mended: every block comes back clean with bit 24
    set, and a check of the mended buffer on the same stream, with no
    synchronize between, reads 0 everywhere."""
    (k, m, x, S), lo, hi = part
    f = W.every_byte(*part)
    n = hi - lo
    g = Guarded("device")
    hidx = g.input("have_idx", f.idx)
    hv = inout(g, "have", f.have.reshape(n, -1))
    g.output("mend", 4 * n)
    g.output("again", 4 * n)
    codec.correct(k, m, hidx, hv, g.words("mend"), x=x, S=S, n=n)
    codec.check(k, m, hidx, hv, g.words("again"), x=x, S=S, n=n)
    codec.synchronize()
    cases = Cases()
    cases.check("bytes %d..%d" % (lo, hi - 1), g, have=f.clean.reshape(n, -1),
                mend=f.want | np.uint32(CORRECTED), again=np.zeros(n, np.uint32))
    cases.done()

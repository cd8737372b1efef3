"""The families of tests/check_sweep_cases.py held to the host references
with no GPU, so every case tests/test_gpu_check_sweep.py puts on the device
is proven first: each family's words, stated by construction, equal
check_ref.check_reference, check_pair_ref.check_pair_reference or
correct_ref.correct_reference bit for bit on the family's distinct blocks;
blocks left untouched read 0; and the conditions the families rest on hold
(two wrong shards at x = 3 are never located, the x = 3 rank-1 pairs are
named and left unlocated at least once each, the ambiguous factor was found,
a third wrong byte never yields a pair).  For the three batches with a second
grid round the distinct blocks are judged, and the index arithmetic that puts
them at the round boundaries; the caps are read from the sources' text."""
import os
import re

import numpy as np
import pytest

import check_sweep_cases as W
import correct_cases as CC
from conftest import ROOT
from correct_cases import CORRECTED, single_batch
from test_check_restated import UNLOCATED


def shard(words):
    return (np.asarray(words, np.uint32) >> 16) & 0xFF


def second(words):
    return np.asarray(words, np.uint32) >> 25


def untouched_read_zero(f):
    quiet = np.array([len(t) == 0 for t in f.truth])
    assert not f.want[quiet].any() and f.want[~quiet].all()
    assert np.array_equal(f.have[quiet], f.clean[quiet])
    assert f.sel is None or quiet[0]  # the block a long batch repeats is clean


def held_to_check(f):
    assert np.array_equal(f.want, W.check_words(f))
    untouched_read_zero(f)


def held_to_pair(f):
    assert np.array_equal(f.want, W.pair_words(f))
    untouched_read_zero(f)


def named(f, b):
    """Does word b name exactly the planted pair of block b?"""
    lo, hi = sorted(int(f.idx[b, q]) for q in f.truth[b])
    w = int(f.want[b])
    return len(f.truth[b]) == 2 and (w >> 16) & 0xFF == lo and w >> 25 == hi + 1 and not w & CORRECTED


def neighbours_differ(f, positions=True):
    """Neighbouring blocks have different index sets and, unless told
    otherwise, different wrong positions."""
    assert (f.idx[1:] != f.idx[:-1]).any(axis=1).all()
    assert not positions or all(a != b for a, b in zip(f.truth, f.truth[1:]))


# ------------------------------------------------------------------------- A
@pytest.mark.parametrize("part", W.A1_PARTS, ids=lambda p: "rs%d_%d_x%d_S%d_from%d" % (p[0] + (p[1],)))
def test_a1_every_byte(part):
    shape, lo, hi = part
    k, m, x, S = shape
    f = W.every_byte(*part)
    assert [int(np.flatnonzero((f.have[i] ^ f.clean[i]).any(axis=0))[0]) for i in range(hi - lo)] \
        == list(range(lo, hi))
    assert all(np.count_nonzero(f.have[i] ^ f.clean[i]) == 1 for i in range(hi - lo))
    held_to_check(f)
    held_to_pair(f)  # nothing qualifies: the pair check's words are the check's
    neighbours_differ(f)
    assert (shard(f.want) != UNLOCATED).all() and not second(f.want).any()


def test_a1_parts_cover_every_byte():
    for shape in {p[0] for p in W.A1_PARTS}:
        spans = sorted((lo, hi) for s, lo, hi in W.A1_PARTS if s == shape)
        assert spans[0][0] == 0 and spans[-1][1] == shape[3]
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert W.A1_WHOLE[0][3] // 4 == 272            # 256 lanes and a second stride round of 16
    assert W.A1_QUARTERS[0][0][3] > 4096           # past a MAC tile edge


def test_a2_disqualifying_byte():
    f = W.disqualifying_byte()
    k, m, x, S = f.shape
    cases = W.a2_cases()
    held_to_check(f)
    assert all(len(f.truth[b]) == 0 for b in range(0, len(f.truth), 2))
    two = [2 * c + 1 for c, (fam, _) in enumerate(cases) if fam != "d"]
    one = [2 * c + 1 for c, (fam, _) in enumerate(cases) if fam == "d"]
    assert len(two) == 814 and len(one) == k
    assert (f.want[two] == ((1 << x) - 1) | (UNLOCATED << 16)).all()   # every one unlocated, every row lit
    assert [int(s) for s in shard(f.want[one])] == [int(f.idx[b, j]) for j, b in enumerate(one)]
    # the one byte of j2 lies in dword w, for every w
    for fam in "abc":
        ws = set()
        for c, (g, w) in enumerate(cases):
            if g == fam:
                b = 2 * c + 1
                j2 = f.truth[b][1]
                at = np.flatnonzero(f.have[b, j2] ^ f.clean[b, j2])
                assert at.size == 1 and at[0] // 4 == w
                ws.add(w)
        assert ws == set(range(S // 4)) - ({0} if fam == "a" else {S // 4 - 1} if fam == "b" else set())


def test_a3_every_limit_position():
    f = W.every_limit_position()
    k, m, x, S = f.shape
    assert f.truth == tuple((b,) for b in range(k + x)) and k == 64
    held_to_check(f)
    neighbours_differ(f)
    assert [int(s) for s in shard(f.want)] == [int(f.idx[b, b]) for b in range(k + x)]


def test_a4_every_word_flagged():
    f = W.every_word_flagged()
    assert f.idx.shape[0] == 130 and f.want.all()
    held_to_check(f)
    neighbours_differ(f)


def source(*path):
    with open(os.path.join(ROOT, "memo_amd", "csrc", *path)) as fh:
        return fh.read()


def launch_cap(name):
    """(words a workgroup, cap) of a launch function's grid, from its text."""
    body = source("ec_kernels.hip").split("hipError_t %s(" % name, 1)[1].split("\n}\n", 1)[0]
    m = re.search(r"grid = \(a\.n \+ (\d+)\) / (\d+);.*\n\s*if \(grid > (\d+)\) grid = (\d+);", body)
    assert m and int(m.group(1)) + 1 == int(m.group(2)) and m.group(3) == m.group(4), body
    return int(m.group(2)), int(m.group(3))


def test_round_caps_are_the_sources():
    assert launch_cap("launch_check_locate") == (W.LOCATE_WORDS, W.LOCATE_GRID)
    assert launch_cap("launch_check_pair") == (W.LOCATE_WORDS, W.LOCATE_GRID)
    plan = source("correct_plan.h")
    assert re.search(r"kListGridCap = %d;" % W.LIST_GRID, plan)
    assert "const uint64_t wgs = (n + %d) / %d;" % (W.LIST_WORDS - 1, W.LIST_WORDS) in plan
    assert re.search(r"correct_list_kernel, dim3\(correct::list_grid_for\(a\.n\)\), dim3\(%d\)" % W.LIST_WORDS,
                     source("ec_kernels.hip"))


def where(b, grid, words):
    """(round, workgroup, word of the workgroup) of block b."""
    return b // (grid * words), (b // words) % grid, b % words


def boundaries_hold(f, grid, words):
    n = f.sel.size
    assert n == grid * words + words + 3
    _, places = W.round_places(grid, words)
    assert [where(b, grid, words) for b in places] == [
        (0, 0, 0), (0, 0, words - 1), (0, grid - 1, 0), (0, grid - 1, words - 1),
        (1, 0, 0), (1, 0, words - 1), (1, 1, 0), (1, 1, 2)]
    assert f.sel.min() == 0 and f.sel.max() == f.idx.shape[0] - 1 and (f.sel[places] != 0).all()
    return n, places


def test_a5_check_second_round():
    f = W.check_second_round()
    held_to_check(f)
    n, places = boundaries_hold(f, W.LOCATE_GRID, W.LOCATE_WORDS)
    assert n * f.have[0].size < 45 << 20
    inside = W.LOCATE_GRID * W.LOCATE_WORDS + 10
    assert np.flatnonzero(f.sel).tolist() == sorted(places + [inside])
    assert shard(f.want)[f.sel[inside]] == UNLOCATED and where(inside, W.LOCATE_GRID, W.LOCATE_WORDS)[0] == 1
    assert (shard(f.want[f.sel[places]]) != UNLOCATED).all()
    assert {f.truth[int(p)][0] for p in f.sel[places]} == set(range(5))  # every position of the code
    assert len({f.idx[int(p)].tobytes() for p in f.sel[places]}) >= 4    # on index sets of their own


# ------------------------------------------------------------------------- B
@pytest.mark.parametrize("shape", W.B1_SHAPES, ids=lambda s: "rs%d_%d_x%d_S%d" % s)
def test_b1_every_pair(shape):
    k, m, x, S = shape
    f = W.every_pair(shape)
    n = f.idx.shape[0]
    assert n == (k + x) * (k + x - 1) and len(set(f.truth)) == n // 2
    held_to_pair(f)
    same, apart = range(0, n, 2), range(1, n, 2)
    for b in same:
        err = f.have[b] ^ f.clean[b]
        assert np.count_nonzero(err) == 2 and np.flatnonzero(err.any(axis=0)).size == 1
    for b in apart:
        err = f.have[b] ^ f.clean[b]
        assert np.count_nonzero(err) == 2 and np.flatnonzero(err.any(axis=0)).size == 2
    assert all(named(f, b) for b in apart)
    if x >= 4:
        assert all(named(f, b) for b in same)
    else:  # rank 1 at x = 3: named, or two pairs explain it
        hit = [named(f, b) for b in same]
        assert any(hit) and not all(hit)
        assert all(h or (shard(f.want[b]) == UNLOCATED and second(f.want[b]) == 0) for b, h in zip(same, hit))


def test_b2_limit_pairs():
    f = W.limit_pairs()
    assert len(W.B2_PAIRS) < 50 and f.idx.shape[0] == 2 * len(W.B2_PAIRS)
    held_to_pair(f)
    assert all(named(f, b) for b in range(f.idx.shape[0]))
    assert any(q >= 64 for t in f.truth for q in t) and (63, 64) in f.truth
    assert (0, 1) in f.truth and (64, 79) in f.truth  # the first pair of nth_pair and its tail


def test_b3_walk1():
    f = W.walk1()
    k, m, x, S = f.shape
    assert f.idx.shape[0] == S
    for b in range(S):
        err = f.have[b] ^ f.clean[b]
        assert np.flatnonzero(err.any(axis=0)).tolist() == [b] and np.count_nonzero(err) == 2
    held_to_pair(f)
    assert all(named(f, b) for b in range(S))


@pytest.mark.parametrize("shape", W.B4_SHAPES, ids=lambda s: "rs%d_%d_x%d_S%d" % s)
def test_b4_walk2(shape):
    from memo_amd import check_pair_ref as P
    k, m, x, S = shape
    row, blk, e, c = W.ambiguous_factor(shape)   # asserts that the search found a factor
    assert 1 <= c <= 255 and e.all()
    f = W.walk2(shape)
    assert f.idx.shape[0] == 1 + S // 4
    pairs = P.explaining_pairs(k, m, f.idx[0], f.have[0], x)
    assert (0, 1) in pairs and len(pairs) >= 2
    held_to_pair(f)
    assert shard(f.want[0]) == UNLOCATED and second(f.want[0]) == 0   # the control stays ambiguous
    assert all(named(f, b) for b in range(1, f.idx.shape[0]))
    for w in range(S // 4):
        extra = np.flatnonzero((f.have[1 + w] ^ f.have[0]).any(axis=0))
        assert extra.tolist() == [4 * w + w % 4]


@pytest.mark.parametrize("shape", W.B5_SHAPES, ids=lambda s: "rs%d_%d_x%d_S%d" % s)
def test_b5_walk3(shape):
    k, m, x, S = shape
    f = W.walk3(shape)
    assert f.idx.shape[0] == 1 + S // 4
    held_to_pair(f)
    assert named(f, 0)                                                 # the control names its pair
    assert (shard(f.want[1:]) == UNLOCATED).all() and not second(f.want[1:]).any()
    assert np.array_equal(f.want[1:], W.check_words(f)[1:])            # the check's words
    for w in range(S // 4):
        qc = f.truth[1 + w][2]
        assert np.flatnonzero(f.have[1 + w, qc] ^ f.clean[1 + w, qc]).tolist() == [4 * w + w % 4]


def test_b6_every_word_a_pair():
    f = W.every_word_a_pair()
    assert f.idx.shape[0] == 130
    held_to_pair(f)
    assert all(named(f, b) for b in range(130))
    neighbours_differ(f, positions=False)  # a pair's "same" and "apart" blocks are neighbours


def test_b6_pair_second_round():
    f = W.pair_second_round()
    held_to_pair(f)
    n, places = boundaries_hold(f, W.LOCATE_GRID, W.LOCATE_WORDS)
    assert n * f.have[0].size < 70 << 20
    kinds = [len(f.truth[f.sel[b]]) for b in places]
    assert sorted(set(kinds)) == [1, 2, 3]
    for b in places + [W.LOCATE_GRID * W.LOCATE_WORDS + 10]:
        p = int(f.sel[b])
        t = f.truth[p]
        if len(t) == 2:
            assert named(f, p)
        elif len(t) == 3:
            assert shard(f.want[p]) == UNLOCATED and second(f.want[p]) == 0
        else:
            assert shard(f.want[p]) == f.idx[p, t[0]] and second(f.want[p]) == 0


# ------------------------------------------------------------------------- C
def test_c1_ranges_cut_inside_entries():
    """The item ranges of correct_plan.h's wg_items for C1, restated: 2100
    items over 2048 workgroups, 2 each, beginning at every tile of an entry."""
    k, m, x, S, n = CC.SWEEP_RANGES
    plan = source("correct_plan.h")
    assert "kTileBytes = 4096;" in plan and "kGridCap = 2048;" in plan
    tpb = -(-S // 4096)
    assert tpb == 3 and S - 2 * 4096 == 64
    total = n * tpb
    grid = min(total, 2048)
    per = -(-total // grid)
    assert (total, grid, per) == (2100, 2048, 2)
    starts = {(w * per) % tpb for w in range(grid) if w * per < total}
    ends = {min((w + 1) * per, total) % tpb for w in range(grid) if w * per < total}
    assert starts == {0, 1, 2} and ends == {0, 1, 2}
    assert CC.SWEEP_RANGES in CC.GPU_SHAPES
    idx, clean, have, words = single_batch(CC.SWEEP_RANGES)
    # the one shard each block has overwritten: positions 0..4 in turn, and
    # the word names that shard
    changed = [np.flatnonzero((have[b] ^ clean[b]).any(axis=1)).tolist() for b in range(n)]
    assert changed == [[b % (k + x)] for b in range(n)]
    assert [int(s) for s in shard(words)] == [int(idx[b, b % (k + x)]) for b in range(n)]
    assert (words >> 24 == 1).all()
    # every block against the reference: the mended bytes are the clean ones
    from memo_amd import correct_ref as C
    got, mended = C.correct_reference(k, m, idx, have.reshape(n, -1), x=x, S=S)
    assert np.array_equal(got, words) and np.array_equal(mended, clean)


def test_c2_interleaved():
    f = W.interleaved()
    k, m, x, S = f.shape
    words, mended = W.correct_words(f)
    assert np.array_equal(words, f.want) and np.array_equal(mended, W.after(f))
    untouched_read_zero(f)
    kinds = [len(t) for t in f.truth]
    assert kinds.count(1) == k + x and kinds.count(2) >= 4 and kinds.count(0) >= 4
    # no two neighbours of a kind, but the last two (13 located blocks of 24)
    assert all(a != b for a, b in zip(kinds[:-1], kinds[1:-1])) and kinds[-2:] == [1, 1]
    for b, t in enumerate(f.truth):
        changed = np.flatnonzero((W.after(f)[b] ^ f.have[b]).any(axis=1)).tolist()
        assert changed == (list(t) if len(t) == 1 else [])   # the target shard alone
        if len(t) == 2:
            assert f.want[b] == ((1 << x) - 1) | (UNLOCATED << 16)


def test_c3_list_second_round():
    f = W.list_second_round()
    words, mended = W.correct_words(f)
    assert np.array_equal(words, f.want) and np.array_equal(mended, W.after(f))
    assert np.array_equal(W.after(f), f.clean)
    untouched_read_zero(f)
    n, places = boundaries_hold(f, W.LIST_GRID, W.LIST_WORDS)
    assert n * f.have[0].size < 90 << 20
    located = np.flatnonzero(f.sel)
    wave = list(range(W.C3_WAVE, W.C3_WAVE + 64))
    assert located.tolist() == sorted(places + wave + [W.C3_LANE63])
    assert W.C3_WAVE % 64 == 0 and W.C3_LANE63 % 64 == 63
    assert not f.sel[W.C3_LANE63 - 63:W.C3_LANE63].any()          # lane 63 alone in its wave
    assert (f.sel[wave][1:] != f.sel[wave][:-1]).all()            # neighbours differ
    assert -(-n // W.LOCATE_WORDS) > 2 * W.LOCATE_GRID            # the check's third grid round
    assert (f.want[1:] >> 24 == 1).all()


@pytest.mark.parametrize("part", W.A1_QUARTERS, ids=lambda p: "rs%d_%d_x%d_S%d_from%d" % (p[0] + (p[1],)))
def test_c4_sweep_then_mend_words(part):
    """C4 mends A1's RS(10,4) batches: every word of every block is the
    check's with bit 24, every block comes back clean (so a re-check reads
    0)."""
    f = W.every_byte(*part)
    words, mended = W.correct_words(f)
    assert np.array_equal(words, f.want | np.uint32(CORRECTED)) and np.array_equal(mended, f.clean)

"""memo_amd.check_pair_ref, the host reference of memo_ec_check_pair_batch,
held to ground truth that comes from construction (tests/check_pair_cases.py:
which shards were made wrong), not from its own search.  No GPU."""
import functools

import numpy as np
import pytest

import check_pair_cases as C
from conftest import SEED
from test_check_restated import INVALID, UNLOCATED, random_sets, shards_of, take

# (k, m, x, S): x >= 4, where two wrong shards are always found
SHAPES = [(4, 4, 4, 64), (10, 4, 4, 448), (16, 4, 4, 64), (20, 6, 4, 256), (7, 5, 5, 128)]
IDS = ["rs%d_%d_x%d_S%d" % s for s in SHAPES]


def refs():
    from memo_amd import check_pair_ref as P, check_ref as R
    return P, R


@functools.lru_cache(maxsize=None)
def words(shape):
    P, R = refs()
    k, m, x, S = shape
    idx, have, truth = C.batch(shape)
    got = P.check_pair_reference(k, m, idx, have.reshape(C.N, -1))
    chk = R.check_reference(k, m, idx, have.reshape(C.N, -1))
    assert got.dtype == np.uint32 and got.shape == (C.N,)
    return got, chk


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_planted_errors_are_found(shape):
    """Basis + basis, basis + spare, spare + spare; one byte each at the same
    offset (rank 1), at offsets 0 and S - 1, and whole shards: the word names
    exactly the two changed shards, the smaller index in bits 16..23."""
    P, _ = refs()
    k, m, x, S = shape
    idx, have, truth = C.batch(shape)
    got, chk = words(shape)
    for b in range(3, 12):
        a, c = (int(idx[b, q]) for q in truth[b])
        assert chk[b] != 0 and chk[b] >> 16 == UNLOCATED, (C.kind(b), hex(int(chk[b])))
        want = (int(chk[b]) & 0xFFFF) | (min(a, c) << 16) | ((max(a, c) + 1) << 25)
        assert got[b] == want, (C.kind(b), hex(int(got[b])), hex(want))
        assert P.split_verdict_pair(got[b]) == (int(chk[b]) & 0xFFFF, min(a, c), max(a, c))
        assert not (int(got[b]) >> 24) & 1


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_words_the_check_settles_are_the_checks(shape):
    """Clean, located and three-error blocks: the check's word, bit for bit."""
    P, _ = refs()
    k, m, x, S = shape
    idx, have, truth = C.batch(shape)
    got, chk = words(shape)
    assert got[0] == chk[0] == 0
    for b in (1, 2):
        assert got[b] == chk[b] and chk[b] >> 16 == int(idx[b, truth[b][0]]), (b, hex(int(chk[b])))
        assert P.split_verdict_pair(got[b])[2] is None
    assert got[12] == chk[12] and chk[12] >> 16 == UNLOCATED, (hex(int(got[12])), hex(int(chk[12])))
    assert chk[12] & 0xFFFF


def test_invalid_sets_and_other_settled_words_are_untouched():
    """test_check_reference's invalid-set batch with x = 3: every word that is
    0, INVALID or located is the check's."""
    P, R = refs()
    k, m, x, S, n = 10, 4, 3, 448, 24
    rng = np.random.default_rng(SEED + 16)
    full = shards_of(C.oracle(), k, m, S, rng, n)
    idx = random_sets(rng, k, m, x, n)
    have = take(full, idx)
    idx[2, 7] = idx[2, 3]
    idx[6, k + 1] = idx[6, 4]
    idx[14, 5] = k + m
    idx[18, k] = 255
    have[5, 2, 17] ^= 0x40
    have[13, k + 1, S - 1] ^= 0x01
    got = P.check_pair_reference(k, m, idx, have)
    chk = R.check_reference(k, m, idx, have)
    assert np.array_equal(got, chk)
    assert np.count_nonzero(chk == INVALID) == 4 and chk[5] >> 16 == idx[5, 2]


@pytest.mark.parametrize("x", [1, 2])
def test_x_below_three_is_the_check(x):
    """Corrupted batches with x <= 2: the check's words."""
    P, R = refs()
    k, m, S = 10, 4, 64
    idx, have, truth = C.batch((k, m, 4, S))
    idx, have = idx[:, :k + x], have[:, :k + x]
    got = P.check_pair_reference(k, m, idx, have)
    assert np.array_equal(got, R.check_reference(k, m, idx, have))
    assert np.count_nonzero(got) >= 6 and not (got >> 24).any()


def test_s_zero_and_empty_calls():
    P, _ = refs()
    idx = np.tile(np.arange(14, dtype=np.uint8), (4, 1))
    assert P.check_pair_reference(10, 4, idx, np.zeros((4, 0), np.uint8), S=0).tolist() == [0] * 4
    assert P.check_pair_reference(10, 4, idx[:, :10], np.zeros((4, 640), np.uint8), x=0).tolist() == [0] * 4
    assert P.check_pair_reference(10, 4, idx[:0], np.zeros((0, 0), np.uint8)).tolist() == []
    with pytest.raises(ValueError):
        P.check_pair_reference(10, 4, idx.reshape(-1), np.zeros(4 * 14 * 64, np.uint8))  # flat, no x


# RS(10,4), x = 3, one flipped byte at the same offset of two shards (rank 1)
AMBIGUOUS = (10, 4, 3, 64, 36, 0x33)


def test_x3_same_offset_blocks_are_located_or_have_two_pairs():
    """x = 3: a block whose syndromes are all proportional is located when one
    pair explains it and stays unlocated when two do.  Both occur here."""
    P, R = refs()
    k, m, x, S, n, seed = AMBIGUOUS
    idx, have, truth = C.same_offset_blocks(k, m, x, S, n, seed)
    got = P.check_pair_reference(k, m, idx, have)
    chk = R.check_reference(k, m, idx, have)
    located = ambiguous = 0
    for b in range(n):
        pairs = P.explaining_pairs(k, m, idx[b], have[b], x)
        planted = tuple(sorted(truth[b]))
        assert chk[b] != 0 and chk[b] >> 16 == UNLOCATED, (b, hex(int(chk[b])))
        assert planted in pairs, (b, planted, pairs)  # what was planted always explains
        if len(pairs) == 1:
            a, c = sorted(int(idx[b, q]) for q in planted)
            assert got[b] == (int(chk[b]) & 0xFFFF) | (a << 16) | ((c + 1) << 25), (b, hex(int(got[b])))
            located += 1
        else:
            assert got[b] == chk[b], (b, hex(int(got[b])))
            ambiguous += 1
    assert located >= 1 and ambiguous >= 1, (located, ambiguous)


def test_x3_rank_two_is_located():
    """x = 3, the two errors at different offsets: the syndromes span two
    dimensions and the pair is unique."""
    P, _ = refs()
    shape = (10, 4, 3, 448)
    k, m, x, S = shape
    idx, have, truth = C.batch(shape)
    got, chk = words(shape)
    for b in (4, 5, 7, 8, 10, 11):  # "ends" and "whole"
        a, c = sorted(int(idx[b, q]) for q in truth[b])
        assert got[b] == (int(chk[b]) & 0xFFFF) | (a << 16) | ((c + 1) << 25), (C.kind(b), hex(int(got[b])))
    assert got[12] == chk[12]


def test_split_verdict_pair_of_the_binding_agrees():
    from memo_amd import ec
    P, _ = refs()
    for v in (0x000F00FF, 0x00070203, (0xF | (3 << 16) | (80 << 25)), 0x00FF0003):
        assert ec.split_verdict_pair(v) == P.split_verdict_pair(v)
    arr = np.array([0xF | (0xFF << 16), 0xF | (3 << 16) | (14 << 25)], dtype=np.uint32)
    mask, shard, second = ec.split_verdict_pair(arr)
    assert mask.tolist() == [0xF, 0xF] and shard.tolist() == [0xFF, 3] and second.tolist() == [-1, 13]

"""memo_amd.check_ref: the package's host reference of the k + x shard check
(own GF tables, own generator and Gauss-Jordan) against the oracle-based
restatement of tests/test_check_restated.py, on per-block random index sets
(parity in the basis, data among the spares, unsorted) of the shapes the
device tests of the call use.  No GPU."""
import numpy as np
import pytest

from conftest import SEED
from test_check_restated import INVALID, UNLOCATED, expected_check, random_sets, shards_of, take

# (k, m, x, S, n)
SHAPES = [
    (3, 2, 2, 64, 130),
    (10, 4, 2, 448, 37),
    (10, 4, 4, 448, 37),
    (16, 4, 3, 4160, 5),
    (5, 3, 3, 192, 20),
    (7, 5, 5, 128, 12),
    (20, 6, 4, 256, 9),
    (4, 1, 1, 64, 70),       # x = 1: detect only
    (64, 16, 16, 64, 3),     # the limits
    (10, 4, 4, 104896, 2),   # the 1 MiB block
]
IDS = ["rs%d_%d_x%d_S%d_n%d" % s for s in SHAPES]


def test_tables_generator_and_rows_match_the_oracle_and_the_library(O):
    from memo_amd import check_ref as R, ec
    rng = np.random.default_rng(SEED)
    for a, b in rng.integers(0, 256, size=(2000, 2)):
        assert R.MUL[a, b] == O.gf_mul(int(a), int(b))
    for a in range(256):
        assert R.MUL[a, 0] == 0 and R.MUL[0, a] == 0 and R.MUL[a, 1] == a
    for a in range(1, 256):
        assert R.gf_inv(a) == O.gf_inv(a)
    for (k, m) in [(3, 2), (4, 1), (10, 4), (16, 4), (20, 6), (64, 16)]:
        g = R.generator(k, m)
        assert np.array_equal(g, O.cauchy(k, m))
        assert np.array_equal(g, ec.generator(k, m))
        for x in {1, m}:
            row = random_sets(rng, k, m, x, 1)[0]
            assert np.array_equal(R.decode_rows(k, m, row[:k], row[k:]),
                                  O.decode_matrix(k, m, row[:k], row[k:]))
    assert (R.VERDICT_UNLOCATED, R.VERDICT_INVALID) == (UNLOCATED, INVALID)
    assert R.VERDICT_UNLOCATED == ec.VERDICT_UNLOCATED


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_reference_equals_the_restated_definition(O, shape):
    """Clean blocks, one wrong spare, one wrong basis shard (first and last
    byte), two wrong basis shards (same byte, different bytes): the two
    implementations agree on every word, the corruptions built for a shard
    name it, and the clean blocks read 0."""
    from memo_amd import check_ref as R
    k, m, x, S, n = shape
    rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + x * 101 + S * 31 + n))
    full = shards_of(O, k, m, S, rng, n)
    idx = random_sets(rng, k, m, x, n)
    have = take(full, idx)
    want = {}
    for c, b in enumerate(range(1, n, 2)):
        kind = c % 5
        if kind == 0:                       # a spare
            pos = k + c % x
            have[b, pos, int(rng.integers(0, S))] ^= 1 << int(rng.integers(0, 8))
        elif kind in (1, 2):                # a basis shard, first / last byte
            pos = c % k
            have[b, pos, 0 if kind == 1 else S - 1] ^= int(rng.integers(1, 256))
        else:                               # two basis shards
            t1 = int(rng.integers(0, k))
            t2 = (t1 + 1 + int(rng.integers(0, k - 1))) % k
            p1 = int(rng.integers(0, S))
            p2 = p1 if kind == 3 else (p1 + 1 + int(rng.integers(0, S - 1))) % S
            have[b, t1, p1] ^= int(rng.integers(1, 256))
            have[b, t2, p2] ^= int(rng.integers(1, 256))
            if x >= 3 or (x == 2 and kind == 4):
                want[b] = None              # never located
            continue
        shard = int(idx[b, pos]) if x >= 2 else UNLOCATED
        want[b] = (((1 << x) - 1) if pos < k else 1 << (pos - k), shard)
    got = R.check_reference(k, m, idx, have.reshape(n, -1))
    assert got.dtype == np.uint32 and got.shape == (n,)
    assert np.array_equal(got, expected_check(O, k, m, S, idx, have, x))
    assert not (got >> 24).any()
    for b in range(n):
        if b % 2 == 0:
            assert got[b] == 0, (b, hex(int(got[b])))
    for b, w in want.items():
        mask, shard = R.split_verdict(got[b])
        if w is None:
            assert mask != 0 and shard == UNLOCATED, (b, hex(int(got[b])))
        else:
            assert (mask, shard) == w, (b, hex(int(got[b])))


@pytest.mark.parametrize("km", [(3, 2), (10, 4), (7, 5), (4, 1)], ids=lambda p: "rs%d_%d" % p)
def test_identity_set_is_the_parity_verify(O, km):
    """have_idx = 0..k+m-1 and x = m: the words tests/test_gpu_verify.py
    expects of memo_ec_verify_batch."""
    import test_gpu_verify as V
    from memo_amd import check_ref as R
    k, m = km
    S, n = 128, 16
    rng = np.random.default_rng(SEED ^ (k * 131 + m))
    full = shards_of(O, k, m, S, rng, n)
    for b in range(1, n, 2):
        full[b, b % (k + m), int(rng.integers(0, S))] ^= int(rng.integers(1, 256))
        if b % 3 == 0:
            full[b, (b + 1) % (k + m), int(rng.integers(0, S))] ^= int(rng.integers(1, 256))
    ident = np.tile(np.arange(k + m, dtype=np.uint8), (n, 1))
    got = R.check_reference(k, m, ident, full)
    assert np.array_equal(got, V.expected(O, k, m, S, full[:, :k], full[:, k:], set(range(n))))
    assert np.count_nonzero(got) >= n // 2 - 1


def test_invalid_sets_one_per_block_between_valid_ones(O):
    from memo_amd import check_ref as R
    k, m, x, S, n = 10, 4, 3, 448, 24
    rng = np.random.default_rng(SEED + 16)
    full = shards_of(O, k, m, S, rng, n)
    idx = random_sets(rng, k, m, x, n)
    have = take(full, idx)
    idx[2, 7] = idx[2, 3]            # duplicate inside the basis
    idx[6, k + 1] = idx[6, 4]        # spare equal to a basis shard
    idx[10, k + 2] = idx[10, k]      # spare equal to another spare
    idx[14, 5] = k + m               # first index past the code
    idx[18, k] = 255
    have[5, 2, 17] ^= 0x40
    have[13, k + 1, S - 1] ^= 0x01
    want = np.zeros(n, dtype=np.uint32)
    want[[2, 6, 10, 14, 18]] = INVALID
    want[5] = 0x7 | (int(idx[5, 2]) << 16)
    want[13] = 0x2 | (int(idx[13, k + 1]) << 16)
    got = R.check_reference(k, m, idx, have)
    assert np.array_equal(got, want)
    assert np.array_equal(got, expected_check(O, k, m, S, idx, have, x))


def test_arguments():
    from memo_amd import check_ref as R
    idx = np.tile(np.arange(14, dtype=np.uint8), (4, 1))
    have = np.zeros((4, 14 * 64), dtype=np.uint8)
    assert R.check_reference(10, 4, idx, have).tolist() == [0, 0, 0, 0]       # zeros are a codeword
    assert R.check_reference(10, 4, idx[:, :10], have[:, :640], x=0).tolist() == [0] * 4
    assert R.check_reference(10, 4, idx[:0], have[:0]).tolist() == []
    assert R.check_reference(10, 4, idx.reshape(-1), have.reshape(-1), x=4, S=64).tolist() == [0] * 4
    with pytest.raises(ValueError):
        R.check_reference(10, 4, np.zeros((4, 15), np.uint8), np.zeros((4, 15 * 64), np.uint8))  # x > m
    with pytest.raises(ValueError):
        R.check_reference(10, 4, idx[:, :9], have)                                                # x < 0
    with pytest.raises(ValueError):
        R.check_reference(65, 4, idx, have, x=4)
    with pytest.raises(ValueError):
        R.check_reference(10, 4, idx.reshape(-1), have.reshape(-1))                               # flat, no x
    with pytest.raises(ValueError):
        R.check_reference(10, 4, idx, have[:, :-1])
    with pytest.raises(ValueError):
        R.invert(np.array([[1, 1], [1, 1]], dtype=np.uint8))

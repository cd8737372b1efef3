"""The verdict of a check of any k + x shards in hand (DESIGN.md section 8,
"Next" item 5) stated in numpy, and the two facts about the code it rests
on.  No GPU, no library call: the oracle alone.

A block's k + x shards in hand are named by have_idx: entries 0..k-1 its
basis, entries k..k+x-1 its spares.  With D (x x k) the decode rows of the
spares over the basis (oracle.decode_matrix) and s_r = spare r XOR
sum_t D[r][t] * basis_t:
  every s_r zero                -> 0
  x == 1                        -> mask, 0xFF
  one row r differs             -> have_idx[k + r]
  all x rows differ (x >= 2)    -> have_idx[t] for the basis position t with
                                   s_r[p] * D[0][t] == D[r][t] * s_0[p] at
                                   every byte p and row r, else 0xFF
  any other mask                -> 0xFF
  invalid index set             -> 0xFFFFFFFF (index >= k + m, or one that
                                   repeats)
`expected_check` is that definition, importable, for the device tests of the
call to judge by.  The rule is the parity verify's with D in place of g_ij
(tests/test_gpu_verify.py's `expected` is the identity-set case), which needs
every D entry nonzero and D[r'][t] / D[r][t] injective in t: both are checked
here, exhaustively for RS(3,2) and on seeded random sets for RS(10,4) and
RS(16,4)."""
import itertools

import numpy as np

from conftest import SEED

UNLOCATED = 0xFF
INVALID = 0xFFFFFFFF

_MUL = None


def mul_table(O):
    """256 x 256 GF(2^8) products from oracle.gf_mul."""
    global _MUL
    if _MUL is None:
        _MUL = np.array([[O.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)
    return _MUL


def valid_set(k, m, row):
    row = [int(v) for v in row]
    return all(v < k + m for v in row) and len(set(row)) == len(row)


def decode_rows(O, k, m, row, x):
    """D (x x k): spare r = sum_t D[r][t] * basis_t."""
    return O.decode_matrix(k, m, row[:k], row[k:k + x])


def syndromes(O, k, m, row, shards, x):
    """(D, s): s (x x S) = the spares XOR their values recomputed from the basis."""
    MUL = mul_table(O)
    D = decode_rows(O, k, m, row, x)
    s = shards[k:k + x].copy()
    for r in range(x):
        for t in range(k):
            s[r] ^= MUL[D[r, t], shards[t]]
    return D, s


def expected_check(O, k, m, S, have_idx, have, x):
    """The verdict words by the definition.  have_idx: n x (k + x); have:
    n x (k + x) x S."""
    have_idx = np.asarray(have_idx).reshape(-1, k + x)
    n = have_idx.shape[0]
    have = np.asarray(have).reshape(n, k + x, S)
    MUL = mul_table(O)
    out = np.zeros(n, dtype=np.uint32)
    for b in range(n):
        row = have_idx[b]
        if not valid_set(k, m, row):
            out[b] = INVALID
            continue
        D, syn = syndromes(O, k, m, row, have[b], x)
        rows = syn.any(axis=1)
        mask = sum(1 << r for r in range(x) if rows[r])
        if mask == 0:
            continue
        shard = UNLOCATED
        if x >= 2 and bin(mask).count("1") == 1:
            shard = int(row[k + int(np.flatnonzero(rows)[0])])
        elif x >= 2 and mask == (1 << x) - 1:
            s = syn[:, syn.any(axis=0)]  # consistent bytes constrain nothing
            fits = [t for t in range(k)
                    if all(np.array_equal(MUL[s[r], D[0, t]], MUL[D[r, t], s[0]]) for r in range(x))]
            assert len(fits) <= 1  # D[1][t] / D[0][t] is injective in t
            if fits:
                shard = int(row[fits[0]])
        out[b] = mask | (shard << 16)
    return out


def shards_of(O, k, m, S, rng, n):
    """n clean blocks: all k + m shards, n x (k + m) x S."""
    data = rng.integers(0, 256, size=(n, k, S), dtype=np.uint8)
    parity = O.encode(k, m, S, data.reshape(n, k * S)).reshape(n, m, S)
    return np.concatenate([data, parity], axis=1)


def take(full, have_idx):
    """have (n x (k + x) x S) of the index rows."""
    return np.stack([full[b][have_idx[b]] for b in range(full.shape[0])])


def random_sets(rng, k, m, x, n):
    return np.stack([rng.permutation(k + m)[:k + x] for _ in range(n)]).astype(np.uint8)


def test_identity_set_is_the_parity_verify(O):
    """have_idx = 0..k+m-1, x = m: the words of tests/test_gpu_verify.py's
    `expected`, on blocks with a wrong data shard, a wrong parity shard, two
    wrong shards and none."""
    import test_gpu_verify as V
    for (k, m) in [(3, 2), (10, 4), (7, 5)]:
        S, n = 64, 12
        rng = np.random.default_rng(SEED ^ (k * 131 + m))
        full = shards_of(O, k, m, S, rng, n)
        for b in range(1, n):
            kind = b % 4
            if kind == 0:
                continue
            idx = int(rng.integers(0, k)) if kind != 2 else k + int(rng.integers(0, m))
            full[b, idx, int(rng.integers(0, S))] ^= int(rng.integers(1, 256))
            if kind == 3:
                full[b, (idx + 1) % k, int(rng.integers(0, S))] ^= int(rng.integers(1, 256))
        ident = np.tile(np.arange(k + m, dtype=np.uint8), (n, 1))
        got = expected_check(O, k, m, S, ident, full, m)
        want = V.expected(O, k, m, S, full[:, :k], full[:, k:], set(range(n)))
        assert np.array_equal(got, want)
        assert (got != 0).sum() >= n // 2


def check_rows_property(O, k, m, row, x):
    MUL = mul_table(O)
    D = decode_rows(O, k, m, row, x)
    assert D.all(), (k, m, list(row))
    inv = np.array([0] + [O.gf_inv(a) for a in range(1, 256)], dtype=np.uint8)
    for r, r2 in itertools.combinations(range(x), 2):
        ratio = MUL[D[r2], inv[D[r]]]
        assert len(set(ratio.tolist())) == k, (k, m, list(row), r, r2)


def test_decode_rows_are_nonzero_and_ratios_injective(O):
    k, m = 3, 2
    sets = 0
    for x in (1, 2):
        for row in itertools.permutations(range(k + m), k + x):
            check_rows_property(O, k, m, np.array(row, dtype=np.uint8), x)
            sets += 1
    assert sets == 120 + 120  # 5!/1! + 5!/0!
    for (k, m) in [(10, 4), (16, 4)]:
        rng = np.random.default_rng(SEED ^ (k << 8 | m))
        for i in range(200):
            x = 2 + i % (m - 1)
            check_rows_property(O, k, m, random_sets(rng, k, m, x, 1)[0], x)


def test_one_wrong_byte_is_located_as_that_shard(O):
    """Any one shard in hand, basis or spare, x >= 2."""
    for (k, m, xs) in [(3, 2, [2]), (10, 4, [2, 3, 4]), (16, 4, [2, 4])]:
        for x in xs:
            S, n = 64, k + x
            rng = np.random.default_rng(SEED ^ (k * 977 + m * 31 + x))
            full = shards_of(O, k, m, S, rng, n)
            idx = random_sets(rng, k, m, x, n)
            have = take(full, idx)
            for b in range(n):  # block b: position b of its row is wrong
                have[b, b, int(rng.integers(0, S))] ^= int(rng.integers(1, 256))
            got = expected_check(O, k, m, S, idx, have, x)
            for b in range(n):
                mask = (1 << x) - 1 if b < k else 1 << (b - k)
                assert got[b] == mask | (int(idx[b, b]) << 16), (k, m, x, b, hex(int(got[b])))


def test_two_wrong_basis_shards(O):
    """x >= 3: never located (three rows over-determine t: any three columns
    of D are independent over three rows).  Errors at different bytes light
    every row; at the same byte they can cancel in at most one row (any 2 x 2
    minor of D is nonzero), which leaves a mask that is neither one row nor
    all.  x == 2: two syndromes fix one ratio and some t may own it, so the
    definition alone judges the same-byte case (as for the verify with
    m == 2)."""
    for (k, m, x) in [(10, 4, 3), (10, 4, 4), (16, 4, 3), (7, 5, 5), (10, 4, 2), (3, 2, 2)]:
        S, n = 64, 24
        rng = np.random.default_rng(SEED ^ (k * 7919 + m * 13 + x))
        full = shards_of(O, k, m, S, rng, n)
        idx = random_sets(rng, k, m, x, n)
        have = take(full, idx)
        for b in range(n):
            t1 = int(rng.integers(0, k))
            t2 = (t1 + 1 + int(rng.integers(0, k - 1))) % k
            p1 = int(rng.integers(0, S))
            p2 = p1 if b % 2 else (p1 + 1 + int(rng.integers(0, S - 1))) % S
            have[b, t1, p1] ^= int(rng.integers(1, 256))
            have[b, t2, p2] ^= int(rng.integers(1, 256))
        got = expected_check(O, k, m, S, idx, have, x)
        for b in range(n):
            if x >= 3:
                assert got[b] >> 16 == UNLOCATED, (k, m, x, b, hex(int(got[b])))
                lit = bin(int(got[b]) & 0xFFFF).count("1")
                assert lit == x if b % 2 == 0 else lit >= x - 1, (k, m, x, b, hex(int(got[b])))
            elif b % 2 == 0:  # different bytes: each byte names another shard
                assert got[b] == 0x3 | (UNLOCATED << 16), (k, m, x, b, hex(int(got[b])))
            else:
                assert got[b] & 0xFFFF, (k, m, x, b)


def test_invalid_sets_are_marked(O):
    k, m, x, S = 3, 2, 2, 64
    rng = np.random.default_rng(SEED)
    full = shards_of(O, k, m, S, rng, 5)
    idx = np.array([[0, 1, 2, 3, 4], [0, 0, 2, 3, 4], [0, 1, 2, 2, 4], [0, 1, 2, 4, 4], [0, 1, 2, 3, 5]],
                   dtype=np.uint8)
    have = take(full, np.minimum(idx, k + m - 1))
    assert expected_check(O, k, m, S, idx, have, x).tolist() == [0] + [INVALID] * 4

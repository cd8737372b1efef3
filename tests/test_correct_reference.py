"""memo_amd.correct_ref: the host reference of memo_ec_correct_batch, on the
shapes the device tests of the check use.  One shard of a block overwritten
with random bytes comes back as the original, in every position in turn; what
cannot be located is left byte for byte; the mended shard is what the numpy
oracle rebuilds from k of the other shards; and where two wrong shards pass
for one, the bytes written are those of the call's two formulas and the block
checks clean afterwards.  No GPU, no library call."""
import numpy as np
import pytest

from conftest import SEED
from correct_cases import CORRECTED, MISLOCATED, mislocated_blocks, overwrite, single_word
from test_check_reference import IDS, SHAPES
from test_check_restated import INVALID, UNLOCATED, random_sets, shards_of, take


def positions_batch(O, shape):
    """k + x blocks of the shape's code and shard size, block c with position
    c overwritten: every position in turn, basis and spares."""
    k, m, x, S, n = shape
    kx = k + x
    pos = list(range(kx))
    rng = np.random.default_rng(SEED ^ (k * 65537 + x * 257 + S))
    full = shards_of(O, k, m, S, rng, len(pos))
    idx = random_sets(rng, k, m, x, len(pos))
    clean = take(full, idx)
    have = clean.copy()
    for b, p in enumerate(pos):
        overwrite(have, b, p, rng)
    return k, m, x, S, idx, full, clean, have, pos


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_overwritten_shard_comes_back(O, shape):
    from memo_amd import check_ref as R, correct_ref as C
    k, m, x, S, idx, full, clean, have, pos = positions_batch(O, shape)
    n = len(pos)
    before = have.copy()
    words, after = C.correct_reference(k, m, idx, have.reshape(n, -1))
    assert np.array_equal(have, before)                       # the argument is not written
    assert words.dtype == np.uint32 and words.shape == (n,) and after.shape == (n, k + x, S)
    checked = R.check_reference(k, m, idx, have)
    if x == 1:                                                # detect only: the call is the check
        assert np.array_equal(words, checked) and np.array_equal(after, have)
        assert all(int(w) == 1 | (UNLOCATED << 16) for w in words)
        return
    assert np.array_equal(after, clean)
    assert np.array_equal(words, checked | np.uint32(CORRECTED))
    assert [int(w) for w in words] == [single_word(idx, b, p, k, x) for b, p in enumerate(pos)]
    assert not R.check_reference(k, m, idx, after).any()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_the_mended_shard_is_the_oracles_rebuild(O, shape):
    """Independent of check_ref's tables and inversion: the numpy oracle's
    decode of the located index from k of the other shards in hand."""
    from memo_amd import correct_ref as C
    from oracle import rs_numpy as N
    k, m, x, S, idx, full, clean, have, pos = positions_batch(O, shape)
    _, after = C.correct_reference(k, m, idx, have)
    for b, q in enumerate(pos):
        others = [t for t in range(k + x) if t != q][:k]
        rows = N.decode_matrix(k, m, [int(v) for v in idx[b, others]], [int(idx[b, q])])
        want = N.mac(rows, np.ascontiguousarray(have[b, others]))
        assert np.array_equal(after[b, q], want.reshape(-1)), (b, q)


def test_what_is_not_located_comes_back_unchanged(O):
    from memo_amd import check_ref as R, correct_ref as C
    k, m, x, S, n = 10, 4, 3, 448, 24
    rng = np.random.default_rng(SEED + 16)
    full = shards_of(O, k, m, S, rng, n)
    idx = random_sets(rng, k, m, x, n)
    clean = take(full, idx)
    have = clean.copy()
    idx[2, 7] = idx[2, 3]            # invalid sets, as the check's tests have them
    idx[14, 5] = k + m
    idx[18, k] = 255
    have[2, 1, 5] ^= 1               # an invalid block's bytes are not looked at
    have[5, 2, 17] ^= 0x40           # located: a basis shard
    have[9, 0, 3] ^= 0x11            # two wrong basis shards, different bytes: unlocated with x = 3
    have[9, 4, 200] ^= 0x22
    have[11, k, 0] ^= 1              # two wrong spares: a mask that is neither one row nor all
    have[11, k + 2, 1] ^= 1
    words, after = C.correct_reference(k, m, idx, have)
    checked = R.check_reference(k, m, idx, have)
    assert [b for b in range(n) if words[b] != checked[b]] == [5]
    assert words[5] == (0x7 | (int(idx[5, 2]) << 16) | CORRECTED)
    assert all(words[b] == INVALID for b in (2, 14, 18))
    assert (int(words[9]) >> 16) == UNLOCATED and (int(words[11]) >> 16) == UNLOCATED
    changed = [b for b in range(n) if not np.array_equal(after[b], have[b])]
    assert changed == [5] and np.array_equal(after[5], clean[5])
    # x == 1, S == 0, x == 0, n == 0: the call is the check
    w1, a1 = C.correct_reference(k, m, idx[:, :k + 1], have[:, :k + 1])
    assert np.array_equal(w1, R.check_reference(k, m, idx[:, :k + 1], have[:, :k + 1]))
    assert np.array_equal(a1, have[:, :k + 1]) and not ((w1 != INVALID) & ((w1 >> 24) & 1 == 1)).any()
    w0, a0 = C.correct_reference(k, m, idx, np.zeros((n, k + x, 0), np.uint8), S=0)
    assert sorted(set(w0.tolist())) == [0, INVALID] and a0.shape == (n, k + x, 0)
    wz, _ = C.correct_reference(k, m, idx[:, :k], have[:, :k], x=0)
    assert not wz.any()
    we, ae = C.correct_reference(k, m, idx[:0], have[:0])
    assert we.shape == (0,) and ae.size == 0


def test_binding_agrees_on_the_bit():
    from memo_amd import correct_ref as C, ec
    assert C.VERDICT_CORRECTED == CORRECTED == 1 << 24
    assert ec.verdict_corrected(0x01050003) is True and ec.verdict_corrected(0x00050003) is False
    assert ec.verdict_corrected(0xFFFFFFFF) is False
    assert ec.verdict_corrected(np.array([0, 0x01050003, 0xFFFFFFFF, 0x00FF0001], np.uint32)).tolist() == \
        [False, True, False, False]


@pytest.mark.parametrize("code", MISLOCATED, ids=lambda c: "rs%d_%d_x%d_S%d" % c)
def test_two_wrong_shards_that_pass_for_one(O, code):
    """Errors e and c * e in basis shards 0 and 1, x = 2.  The syndromes are
    s_r = (D[r][0] + c D[r][1]) e: one c per row makes that row vanish (the
    other row's spare is blamed), and one c per further basis shard t makes
    s_1 / s_0 = D[1][t] / D[0][t] (shard t is blamed): 2 + (k - 2) = k values
    of c.  The reference then overwrites a shard that was right, with the
    bytes of the call's two formulas, and the block checks clean."""
    from memo_amd import check_ref as R, correct_ref as C
    k, m, x, S = code
    idx, have, cs = mislocated_blocks(k, m, x, S)
    assert len(cs) == k and len(set(cs)) == k      # 3 for RS(3,2), 10 for RS(10,4)
    words, after = C.correct_reference(k, m, idx, have)
    masks = {int(w) & 0xFFFF for w in words}
    assert masks == {0x1, 0x2, 0x3}                # single-row and all-row masks among them
    assert all((int(w) >> 24) == 1 for w in words)
    MUL = R.MUL
    for b in range(len(cs)):
        row = idx[b]
        shard = (int(words[b]) >> 16) & 0xFF
        q = [int(v) for v in row].index(shard)
        assert q >= 2                              # a third shard, not one of the two wrong ones
        d = R.decode_rows(k, m, row[:k], row[k:])
        want = np.zeros(S, np.uint8)
        if q >= k:
            for t in range(k):
                want ^= MUL[d[q - k, t], have[b, t]]
        else:
            want ^= have[b, k]
            for t in range(k):
                if t != q:
                    want ^= MUL[d[0, t], have[b, t]]
            want = MUL[R.gf_inv(int(d[0, q])), want]
        assert np.array_equal(after[b, q], want)
        assert not np.array_equal(after[b, q], have[b, q])    # a shard that was right is gone
        untouched = [t for t in range(k + x) if t != q]
        assert np.array_equal(after[b, untouched], have[b, untouched])
    assert not R.check_reference(k, m, idx, after).any()

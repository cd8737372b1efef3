"""memo_amd/correct_pair_ref.py, the host reference of
memo_ec_correct_pair_batch, held to what was planted and to the CPU oracle.
No GPU, no library call.

The batches are tests/correct_pair_cases.py's: clean / one basis / one spare /
nine pair blocks (bb, bs, ss x same, ends, whole) / three wrong, and what was
planted is known from the construction."""
import itertools

import numpy as np
import pytest

import correct_pair_cases as CP
from check_pair_cases import same_offset_blocks
from conftest import SEED
from correct_pair_cases import CORRECTED, INVALID

SHAPES = CP.REF_SHAPES
IDS = ["rs%d_%d_x%d_S%d" % s for s in SHAPES]


@pytest.fixture(scope="module")
def O():
    return CP.PC.oracle()


def has_pair(w):
    return int(w) != INVALID and (int(w) >> 25) != 0


def test_input_positions_as_the_definition_reads():
    from memo_amd.correct_pair_ref import input_positions
    k, x = 10, 4
    assert input_positions(k, x, 11, 13) == list(range(10))                      # two spares: the basis
    assert input_positions(k, x, 3, 12) == [0, 1, 2, 10, 4, 5, 6, 7, 8, 9]       # r = 2: spare 0
    assert input_positions(k, x, 3, 10) == [0, 1, 2, 11, 4, 5, 6, 7, 8, 9]       # r = 0: spare 1
    assert input_positions(k, x, 2, 7) == [0, 1, 10, 3, 4, 5, 6, 11, 8, 9]       # spare 0 in q1, spare 1 in q2
    for k, x in [(4, 4), (10, 3), (7, 5), (1, 3), (64, 16)]:
        for qa, qb in itertools.combinations(range(k + x), 2):
            pos = input_positions(k, x, qa, qb)
            assert len(pos) == k == len(set(pos)) and qa not in pos and qb not in pos and max(pos) < k + x
            assert all(p == j for j, p in enumerate(pos) if j not in (qa, qb))
            subs = [p for j, p in enumerate(pos) if j in (qa, qb)]
            free = [k + r for r in range(x) if k + r not in (qa, qb)]
            assert subs == free[:len(subs)]
    with pytest.raises(ValueError):
        input_positions(10, 4, 5, 5)
    with pytest.raises(ValueError):
        input_positions(10, 4, 5, 14)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_batch_against_what_was_planted(shape):
    from memo_amd import check_pair_ref, check_ref, correct_ref
    k, m, x, S = shape
    idx, clean, have, truth = CP.batch(shape)
    words, after = CP.batch_reference(shape)
    pair_words = check_pair_ref.check_pair_reference(k, m, idx, have, x=x, S=S)
    single_words, single_after = correct_ref.correct_reference(k, m, idx, have, x=x, S=S)
    recheck = check_ref.check_reference(k, m, idx, after, x=x, S=S)
    # clean
    assert words[0] == 0 and np.array_equal(after[0], have[0])
    # single blocks: correct_reference's
    for b in (1, 2):
        assert words[b] == single_words[b] and (int(words[b]) >> 24) == 1
        assert np.array_equal(after[b], single_after[b]) and np.array_equal(after[b], clean[b])
    # pair blocks
    named = 0
    for b in range(3, 12):
        if has_pair(pair_words[b]):
            named += 1
            assert words[b] == pair_words[b] | CORRECTED, CP.PC.kind(b)
            assert np.array_equal(after[b], clean[b]), CP.PC.kind(b)
            lo, hi = sorted(int(idx[b, q]) for q in truth[b])
            assert (int(words[b]) >> 16) & 0xFF == lo and ((int(words[b]) >> 25) & 0x7F) - 1 == hi
            assert recheck[b] == 0
        else:  # x = 3, every syndrome proportional: two explaining pairs, or the check took it for one shard
            assert x == 3 and CP.PC.kind(b).endswith("same")
            if (int(words[b]) >> 24) & 1:
                assert words[b] == single_words[b] and np.array_equal(after[b], single_after[b])
            else:
                assert words[b] == pair_words[b] and np.array_equal(after[b], have[b])
    assert named == 9 if x >= 4 else named >= 6
    # three wrong: rank 3, no pair
    assert words[12] == pair_words[12] and not has_pair(words[12]) and np.array_equal(after[12], have[12])
    # every corrected block re-checks clean
    for b in range(CP.N):
        if int(words[b]) != INVALID and (int(words[b]) >> 24) & 1:
            assert recheck[b] == 0, b


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_written_shards_are_the_oracles_rebuild(O, shape):
    """The two written shards are the CPU oracle's rebuild (e = 2) from the
    stated input positions -- and from any other k of the non-target
    positions, since exactly two shards were wrong."""
    from memo_amd.correct_pair_ref import input_positions, pair_positions
    k, m, x, S = shape
    idx, clean, have, truth = CP.batch(shape)
    words, after = CP.batch_reference(shape)
    rng = np.random.default_rng(SEED + k + x)
    seen = 0
    for b in range(3, 12):
        qs = pair_positions(idx[b], words[b], k, x)
        if qs is None:
            continue
        seen += 1
        qa, qb = qs
        assert qs == tuple(sorted(truth[b]))
        others = [q for q in range(k + x) if q not in qs]
        picks = [input_positions(k, x, qa, qb)] + [sorted(rng.choice(others, size=k, replace=False).tolist())
                                                  for _ in range(3)]
        lost = np.array([[idx[b, qa], idx[b, qb]]], dtype=np.uint8)
        for pos in picks:
            surv_idx = np.array([idx[b, pos]], dtype=np.uint8)
            out = O.rebuild(k, m, S, surv_idx, have[b, pos].reshape(1, k * S), lost).reshape(2, S)
            assert np.array_equal(out[0], after[b, qa]) and np.array_equal(out[1], after[b, qb]), (b, pos)
    assert seen >= 6


def test_invalid_sets_keep_word_and_bytes():
    from memo_amd import correct_pair_ref as R
    k, m, x, S = 10, 4, 4, 64
    idx, clean, have, truth = CP.batch((k, m, x, 448))
    idx, have = idx.copy(), np.ascontiguousarray(have[:, :, :S])
    idx[5, 3] = idx[5, 0]
    idx[8, k] = k + m
    words, after = R.correct_pair_reference(k, m, idx, have, x=x, S=S)
    assert words[5] == INVALID and words[8] == INVALID
    assert np.array_equal(after[[5, 8]], have[[5, 8]])


def test_x3_two_explaining_pairs_stay_as_they_are():
    """x = 3, one flipped byte at the same offset of two shards: where two
    pairs explain the block the word is check_pair_reference's (unlocated)
    and no byte changes."""
    from memo_amd import check_pair_ref as P
    from memo_amd import correct_pair_ref as R
    k, m, x, S, n = 10, 4, 3, 64, 24
    idx, have, truth = same_offset_blocks(k, m, x, S, n, 11)
    words, after = R.correct_pair_reference(k, m, idx, have, x=x, S=S)
    pw = P.check_pair_reference(k, m, idx, have, x=x, S=S)
    kept = 0
    for b in range(n):
        if not has_pair(pw[b]) and not (int(words[b]) >> 24) & 1:
            assert len(P.explaining_pairs(k, m, idx[b], have[b], x)) != 1
            assert words[b] == pw[b] and np.array_equal(after[b], have[b])
            kept += 1
        elif has_pair(pw[b]):
            assert words[b] == pw[b] | CORRECTED
    assert kept >= 1


@pytest.mark.parametrize("x", [1, 2])
def test_x_up_to_2_is_correct_reference(x):
    from memo_amd import correct_pair_ref as R
    from memo_amd import correct_ref as C
    k, m, S = 10, 4, 64
    idx, clean, have, truth = CP.batch((k, m, 4, 448))
    idx, have = np.ascontiguousarray(idx[:, :k + x]), np.ascontiguousarray(have[:, :k + x, :S])
    w, a = R.correct_pair_reference(k, m, idx, have, x=x, S=S)
    cw, ca = C.correct_reference(k, m, idx, have, x=x, S=S)
    assert np.array_equal(w, cw) and np.array_equal(a, ca) and not any(has_pair(v) for v in w)


def test_S_0_and_empty_calls_are_the_check():
    from memo_amd import check_ref
    from memo_amd import correct_pair_ref as R
    k, m, x = 10, 4, 4
    idx = CP.batch((k, m, x, 448))[0].copy()
    idx[4, 1] = idx[4, 0]
    w, a = R.correct_pair_reference(k, m, idx, np.zeros((CP.N, 0), np.uint8), x=x, S=0)
    assert np.array_equal(w, check_ref.check_reference(k, m, idx, np.zeros((CP.N, 0), np.uint8), x=x, S=0))
    assert w[4] == INVALID and not w[:4].any() and a.size == 0
    w, a = R.correct_pair_reference(k, m, np.zeros((0, k + x), np.uint8), np.zeros((0, 0), np.uint8))
    assert w.size == 0
    w, a = R.correct_pair_reference(k, m, idx[:, :k], np.zeros((CP.N, k * 64), np.uint8), x=0, S=64)
    assert not w.any()


def test_three_wrong_shards_that_pass_for_two():
    """A mislocation block: at x = 3 the errors in positions a, b, c add up,
    byte for byte, to alpha H_d XOR beta H_e.  The reference names {d, e},
    overwrites two shards that were right, and the block re-checks clean and
    differs from the original."""
    from memo_amd import check_ref
    from memo_amd import correct_pair_ref as R
    k, m, x, S = CP.MISLOCATION
    idx, clean, have, (d, e), wrong = CP.mislocation_block(k, m, x, S)
    assert all(not np.array_equal(have[0, q], clean[0, q]) for q in wrong)
    assert np.array_equal(have[0, d], clean[0, d]) and np.array_equal(have[0, e], clean[0, e])
    words, after = R.correct_pair_reference(k, m, idx, have, x=x, S=S)
    assert R.pair_positions(idx[0], words[0], k, x) == (d, e) and (int(words[0]) >> 24) & 1
    changed = [q for q in range(k + x) if not np.array_equal(after[0, q], have[0, q])]
    assert changed == [d, e]
    assert check_ref.check_reference(k, m, idx, after, x=x, S=S)[0] == 0
    assert not np.array_equal(after, clean)

"""Shared by the tests of memo_ec_correct_pair_batch: the shapes the device
tests run (so tests/test_correct_pair_plan.py walks every one of them on the
CPU first) and the batches built for them, on top of tests/check_pair_cases.py.
Ground truth comes from the construction: which positions were changed and
what the clean bytes were.  No test lives here."""
import functools
import itertools

import numpy as np

import check_pair_cases as PC
from conftest import SEED
from correct_cases import clean_batch, overwrite
from test_check_restated import random_sets, shards_of, take

CORRECTED = 1 << 24
INVALID = 0xFFFFFFFF
N = PC.N

# (k, m, x, S) of the 13-block batches: the reference test's and the device's
REF_SHAPES = [(4, 4, 4, 64), (10, 4, 4, 448), (10, 4, 3, 448), (16, 4, 4, 64), (20, 6, 4, 256), (7, 5, 5, 128)]
BATCHES = [(4, 4, 4, 64), (10, 4, 3, 448), (10, 4, 4, 4160), (10, 4, 3, 4160), (16, 4, 4, 64), (16, 4, 4, 4160),
           (20, 6, 4, 256), (7, 5, 5, 128)]

CLEAN = (10, 4, 4, 448, 70)
BRINGUP = (4, 4, 4, 64)
EVERY_PAIR = [(4, 4, 4, 64), (10, 4, 4, 448)]
WIDE = (64, 16, 16, 64)
WIDE_PAIRS = [(30, 31), (31, 32), (32, 33), (0, 63), (62, 63), (63, 64), (64, 65), (31, 64), (63, 79), (78, 79),
              (0, 79), (64, 79)]
# The compiled shard chunks (KC, R = 2) and the codes that reach each: k == KC,
# and under KC = 4 the chunk loop at k = 5, 33 and 64.
KCS = [2, 3, 4, 6, 10, 12, 14, 16]
KC_CODES = {KC: [KC] for KC in KCS}
KC_CODES[4] = [4, 5, 33, 64]
KC_M, KC_S = 4, 192
EDGES = [(5, 3, 3, 64), (5, 3, 3, 4160), (10, 4, 4, 64), (10, 4, 4, 4160)]
# 3 tiles an entry, 2100 work items over 2048 workgroups: item ranges begin and
# end inside entries
RANGES = (3, 3, 3, 8256, 700)
# the list kernel's second grid round: 1024 workgroups x 256 words, and 259 more
LIST = (4, 4, 4, 64, 1024 * 256 + 259)
MIXED = (10, 4, 4, 448, 64)
WAVES = (10, 4, 4, 32768, 9)     # pipe_bytes = 1 MiB: two blocks a wave, five waves
SPLIT = (10, 4, 4, 4160, 5)
BACK = (10, 4, 4, 448, N)
SINGLES = (10, 4, 4, 448, 14)
LOW_X = [(10, 4, 2, 448, 12), (10, 4, 1, 448, 12)]
IDENTITY = [(4, 4), (10, 4), (7, 5)]
MISLOCATION = (10, 4, 3, 64)


def every_pair(k, x):
    return list(itertools.combinations(range(k + x), 2))


def edge_pairs(k, x):
    """The targets first and last of basis and of spares."""
    return [(0, k - 1), (0, k), (k - 1, k + x - 1), (k, k + x - 1), (0, k + x - 1), (k - 1, k)]


def kc_pairs(k, x):
    """One pair of each kind with both clean-row choices, at the ends."""
    return [(0, k - 1), (k // 2, k), (0, k + 1), (k - 1, k + x - 1), (k, k + 1), (k + 1, k + x - 1)]


# (k, m, x, S, n) of every device test, for the CPU walk of correct_pair_plan.h
GPU_SHAPES = ([CLEAN, SINGLES, RANGES, LIST, MIXED, WAVES, SPLIT, BACK, BRINGUP + (1,)]
              + [s + (N,) for s in BATCHES]
              + [s + (len(every_pair(s[0], s[2])),) for s in EVERY_PAIR]
              + [WIDE + (len(WIDE_PAIRS),)]
              + [(k, KC_M, KC_M, KC_S, len(kc_pairs(k, KC_M))) for KC in KCS for k in KC_CODES[KC]]
              + [s + (len(edge_pairs(s[0], s[2])) + 2,) for s in EDGES]
              + [(k, m, m, 128, 16) for (k, m) in IDENTITY]
              + [MISLOCATION + (1,)])


# ------------------------------------------------------------------ the 13-block batch
@functools.lru_cache(maxsize=None)
def batch(shape):
    """(idx, clean, have, truth) of `shape` = (k, m, x, S): check_pair_cases'
    batch -- clean / one basis / one spare / nine pair blocks (bb, bs, ss x
    same, ends, whole) / three wrong -- and the clean blocks it was made
    from, rebuilt from the batch's own seed."""
    k, m, x, S = shape
    idx, have, truth = PC.batch(shape)
    rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + x * 101 + S * 31 + 2))
    assert np.array_equal(random_sets(rng, k, m, x, N), idx)
    clean = take(shards_of(PC.oracle(), k, m, S, rng, N), idx)
    for b in range(N):
        differs = tuple(q for q in range(k + x) if not np.array_equal(clean[b, q], have[b, q]))
        assert differs == tuple(sorted(truth[b])), b
    clean.setflags(write=False)
    return idx, clean, have, truth


@functools.lru_cache(maxsize=None)
def batch_reference(shape):
    """(words, after) of batch(shape) by memo_amd.correct_pair_ref, read-only."""
    from memo_amd import correct_pair_ref as CP
    k, m, x, S = shape
    idx, _, have, _ = batch(shape)
    words, after = CP.correct_pair_reference(k, m, idx, have, x=x, S=S)
    words.setflags(write=False)
    after.setflags(write=False)
    return words, after


# ------------------------------------------------------------- planted pairs, analytic
def pair_word(idx, b, qa, qb, k, x):
    """The corrected word of block b with whole shards qa < qb alone wrong: a
    wrong basis shard lights every row (every entry of D is nonzero and the
    shard's bytes are random), a wrong spare its own."""
    mask = (1 << x) - 1 if qa < k else (1 << (qa - k)) | (1 << (qb - k))
    lo, hi = sorted((int(idx[b, qa]), int(idx[b, qb])))
    return mask | (lo << 16) | ((hi + 1) << 25) | CORRECTED


@functools.lru_cache(maxsize=None)
def pair_batch(shape, targets, seed=0):
    """(idx, clean, have, words): the shape's clean blocks, and the same with
    both shards of `targets` ((block, qa, qb) triples) overwritten with random
    bytes.  Whole random shards have syndromes of rank 2, so the pair is
    unique for every x >= 3."""
    k, m, x, S, n = shape
    idx, clean = clean_batch(k, m, x, S, n, SEED ^ (k * 7919 + x * 131 + S + n + seed + 5))
    rng = np.random.default_rng(SEED + 25 + seed)
    have = clean.copy()
    words = np.zeros(n, np.uint32)
    for b, qa, qb in targets:
        assert qa < qb < k + x
        overwrite(have, b, qa, rng)
        overwrite(have, b, qb, rng)
        words[b] = pair_word(idx, b, qa, qb, k, x)
    for a in (idx, clean, have, words):
        a.setflags(write=False)
    return idx, clean, have, words


def one_per_pair(k, m, x, S, pairs, seed=0):
    """One block per pair, in order."""
    return pair_batch((k, m, x, S, len(pairs)), tuple((b, qa, qb) for b, (qa, qb) in enumerate(pairs)), seed)


# ------------------------------------------------------------------ the mislocation block
@functools.lru_cache(maxsize=None)
def mislocation_block(k, m, x, S):
    """x = 3: a block whose three wrong shards pass for two others.  Per byte
    the error syndrome is alpha H_d XOR beta H_e (alpha, beta random nonzero:
    rank 2 over the shard), expressed in the three OTHER columns a, b, c of
    H = [D | I_3] -- any three columns are a basis -- and planted there as
    errors in positions a, b, c.  (idx, clean, have, (d, e), (a, b, c))."""
    from memo_amd import check_ref as R
    assert x == 3
    rng = np.random.default_rng(SEED + 99 + k)
    idx, clean = clean_batch(k, m, x, S, 1, SEED + 98 + k)
    D = R.decode_rows(k, m, idx[0, :k], idx[0, k:])
    H = np.concatenate([D, np.eye(x, dtype=np.uint8)], axis=1)
    d, e, a, b, c = 1, k + 1, 0, k - 1, k + 2
    alpha = rng.integers(1, 256, size=S, dtype=np.uint8)
    beta = rng.integers(1, 256, size=S, dtype=np.uint8)
    syn = R.MUL[H[:, d][:, None], alpha[None, :]] ^ R.MUL[H[:, e][:, None], beta[None, :]]   # 3 x S
    coef = R.matmul(R.invert(H[:, [a, b, c]]), syn)                                         # 3 x S
    have = clean.copy()
    for pos, err in zip((a, b, c), coef):
        have[0, pos] ^= err
    # a wrong basis shard t adds D[:, t] * err to the syndromes, a wrong spare r adds e_r * err
    for arr in (idx, clean, have):
        arr.setflags(write=False)
    return idx, clean, have, (d, e), (a, b, c)

"""Shared by the tests of memo_ec_correct_batch: the shapes the device tests
run (so tests/test_correct_plan.py walks every one of them on the CPU first),
the batches built for them and the search for mislocation blocks.  No test
lives here."""
import functools

import numpy as np

from conftest import SEED
from test_check_reference import SHAPES
from test_check_restated import random_sets, shards_of, take

CORRECTED = 1 << 24

# The compiled shard chunks (KC, R = 1) and the codes that reach each: k == KC,
# and under KC = 4 the chunk loop at k = 5, 33 and 64.
KCS = [2, 3, 4, 6, 10, 12, 14, 16]
KC_CODES = {KC: [KC] for KC in KCS}
KC_CODES[4] = [4, 5, 33, 64]
KC_M, KC_S, KC_N = 4, 192, 6     # every KC code: m = 4, x in (2, 4)

BRINGUP = (3, 2, 2, 64, 5)
WAVES = (10, 4, 2, 32768, 9)     # pipe_bytes = 1 MiB: two blocks a wave, five waves
EDGES = [(5, 3, 3, 4160, 6), (5, 3, 3, 64, 6), (10, 4, 2, 4160, 6), (10, 4, 2, 64, 6)]
LIST = (3, 2, 2, 64, 4099)
SPLIT = (10, 4, 4, 4160, 5)
MISLOCATED = [(3, 2, 2, 64), (10, 4, 2, 64)]   # (k, m, x, S)
# tests/test_gpu_check_sweep.py: 3 tiles an entry (the last 64 bytes), 2100 work
# items over 2048 workgroups, so item ranges begin and end inside entries
SWEEP_RANGES = (3, 2, 2, 8256, 700)

# (k, m, x, S, n) of every device test, for the CPU walk of correct_plan.h
NOTHING = [(10, 4, 3, 448, 24), (16, 4, 2, 8256, 3)]   # invalid sets; a clean batch of several tiles a block
GPU_SHAPES = (list(SHAPES) + [BRINGUP, WAVES, LIST, SPLIT, SWEEP_RANGES] + EDGES + NOTHING
              + [(k, KC_M, x, KC_S, KC_N) for KC in KCS for k in KC_CODES[KC] for x in (2, KC_M)]
              + [(k, m, x, S, k) for (k, m, x, S) in MISLOCATED]   # k such blocks each (see there)
              + [(k, m, m, 128, 16) for (k, m) in [(3, 2), (10, 4), (7, 5)]])


def oracle():
    from oracle import oracle as O
    O.build()
    return O


def clean_batch(k, m, x, S, n, seed):
    """(idx, have): n clean blocks on random index sets."""
    rng = np.random.default_rng(seed)
    idx = random_sets(rng, k, m, x, n)
    have = take(shards_of(oracle(), k, m, S, rng, n), idx)
    return idx, have


def overwrite(have, b, pos, rng):
    """Shard `pos` of block b overwritten with random bytes (never the
    original ones)."""
    old = have[b, pos].copy()
    have[b, pos] = rng.integers(0, 256, size=old.size, dtype=np.uint8)
    have[b, pos, 0] = old[0] ^ 0x5A


def single_word(idx, b, pos, k, x):
    """The corrected word of block b with position pos alone wrong (x >= 2):
    a wrong spare r lights row r, a wrong basis shard every row (every entry
    of D is nonzero)."""
    mask = (1 << x) - 1 if pos < k else 1 << (pos - k)
    return mask | (int(idx[b, pos]) << 16) | CORRECTED


@functools.lru_cache(maxsize=None)
def single_batch(shape, targets=None, seed=0):
    """(idx, clean, have, words): the shape's clean blocks, and the same with
    one shard overwritten in the blocks named by targets ((block, position)
    pairs; default: every block, its position cycling through all k + x)."""
    k, m, x, S, n = shape
    idx, clean = clean_batch(k, m, x, S, n, SEED ^ (k * 7919 + x * 131 + S + n + seed))
    if targets is None:
        targets = tuple((b, b % (k + x)) for b in range(n))
    rng = np.random.default_rng(SEED + 24 + seed)
    have = clean.copy()
    words = np.zeros(n, np.uint32)
    for b, pos in targets:
        overwrite(have, b, pos, rng)
        words[b] = single_word(idx, b, pos, k, x) if x >= 2 else 1 | (0xFF << 16)
    for a in (idx, clean, have, words):
        a.setflags(write=False)
    return idx, clean, have, words


@functools.lru_cache(maxsize=None)
def mislocated_blocks(k, m, x, S):
    """Blocks with two wrong basis shards that the check takes for a third
    shard: errors e and c * e (e one random nonzero byte pattern) in basis
    positions 0 and 1 of a fixed seeded block, for every c in 1..255 whose
    word locates a shard other than those two.  (idx, have, c values); the
    search runs memo_amd.check_ref only."""
    from memo_amd import check_ref as R
    rng = np.random.default_rng(SEED + 77 + k)
    idx1 = random_sets(rng, k, m, x, 1)
    base = take(shards_of(oracle(), k, m, S, rng, 1), idx1)[0]
    e = rng.integers(1, 256, size=S, dtype=np.uint8)
    rows, blocks, cs = [], [], []
    for c in range(1, 256):
        blk = base.copy()
        blk[0] ^= e
        blk[1] ^= R.MUL[c, e]
        w = R.check_block(k, m, idx1[0], blk, x)
        shard = (w >> 16) & 0xFF
        if w not in (0, R.VERDICT_INVALID) and shard != R.VERDICT_UNLOCATED \
                and shard not in (int(idx1[0, 0]), int(idx1[0, 1])):
            rows.append(idx1[0])
            blocks.append(blk)
            cs.append(c)
    idx, have = np.array(rows, np.uint8).reshape(-1, k + x), np.array(blocks, np.uint8).reshape(-1, k + x, S)
    idx.setflags(write=False)
    have.setflags(write=False)
    return idx, have, tuple(cs)

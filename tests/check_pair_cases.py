"""Blocks with planted wrong shards for the tests of memo_ec_check_pair_batch
(the reference, the stand-alone logic program and the device call share
them).  Ground truth comes from the construction: which positions were
changed, never from a search.

A batch of `shape` = (k, m, x, S) holds, on random per-block index sets,
  block 0            clean
  block 1            one wrong basis shard (one byte)
  block 2            one wrong spare (one byte)
  blocks 3..11       two wrong shards: basis + basis, basis + spare, spare +
                     spare, each with one flipped byte per shard at the same
                     offset ("same": every syndrome proportional, rank 1), one
                     flipped byte per shard at offsets 0 and S - 1 ("ends"),
                     and every byte of both shards randomised ("whole")
  block 12           three wrong shards, one flipped byte each at three
                     distinct offsets (the syndromes are multiples of three
                     independent columns: rank 3)
`truth[b]` is the tuple of changed positions."""
import functools

import numpy as np

from conftest import SEED
from test_check_restated import random_sets, shards_of, take

WHERE = ("bb", "bs", "ss")
HOW = ("same", "ends", "whole")
N = 13


def oracle():
    from oracle import oracle as O
    O.build()
    return O


def positions(where, k, x, rng):
    """Two distinct positions: basis + basis, basis + spare or spare + spare."""
    if where == "bb":
        a, b = rng.choice(k, size=2, replace=False)
    elif where == "bs":
        a, b = rng.integers(0, k), k + rng.integers(0, x)
    else:
        a, b = k + rng.choice(x, size=2, replace=False)
    return int(a), int(b)


def plant(block, pos, how, S, rng):
    """Make the shards at `pos` of one block ((k + x) x S) wrong."""
    if how == "whole":
        for q in pos:
            block[q] ^= rng.integers(1, 256, size=S, dtype=np.uint8)  # every byte changes
        return
    if how == "same":
        offs = [int(rng.integers(0, S))] * len(pos)
    elif how == "ends":
        offs = [0, S - 1]
    else:  # "apart": distinct offsets, the first and the last among them
        offs = [0, S - 1, S // 2][:len(pos)]
    for q, p in zip(pos, offs):
        block[q, p] ^= int(rng.integers(1, 256))


@functools.lru_cache(maxsize=None)
def batch(shape):
    """(idx, have, truth) of `shape`, read-only."""
    k, m, x, S = shape
    rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + x * 101 + S * 31 + 2))
    idx = random_sets(rng, k, m, x, N)
    have = take(shards_of(oracle(), k, m, S, rng, N), idx)
    truth = [()] * N
    truth[1] = (int(rng.integers(0, k)),)
    truth[2] = (k + int(rng.integers(0, x)),)
    plant(have[1], truth[1], "same", S, rng)
    plant(have[2], truth[2], "same", S, rng)
    b = 3
    for where in WHERE:
        for how in HOW:
            truth[b] = positions(where, k, x, rng)
            plant(have[b], truth[b], how, S, rng)
            b += 1
    three = rng.choice(k + x, size=3, replace=False)
    truth[12] = tuple(int(q) for q in three)
    plant(have[12], truth[12], "apart", S, rng)
    idx.setflags(write=False)
    have.setflags(write=False)
    return idx, have, truth


def kind(b):
    """What block b of a batch holds, for messages."""
    if b < 3:
        return ("clean", "one basis", "one spare")[b]
    if b == 12:
        return "three"
    return "%s/%s" % (WHERE[(b - 3) // 3], HOW[(b - 3) % 3])


@functools.lru_cache(maxsize=None)
def same_offset_blocks(k, m, x, S, n, seed):
    """n blocks with one flipped byte at the same offset of two shards each
    (rank 1): with x = 3 some are located and some have two explaining
    pairs.  (idx, have, truth), read-only."""
    rng = np.random.default_rng(SEED ^ seed)
    idx = random_sets(rng, k, m, x, n)
    have = take(shards_of(oracle(), k, m, S, rng, n), idx)
    truth = []
    for b in range(n):
        pos = positions(WHERE[b % 3], k, x, rng)
        plant(have[b], pos, "same", S, rng)
        truth.append(pos)
    idx.setflags(write=False)
    have.setflags(write=False)
    return idx, have, truth


def pair_reference(k, m, x, S, idx, have):
    """check_pair_reference evaluated on the batch's distinct blocks only."""
    from memo_amd import check_pair_ref as P
    idx = np.ascontiguousarray(idx, dtype=np.uint8).reshape(-1, k + x)
    n = idx.shape[0]
    have = np.ascontiguousarray(have, dtype=np.uint8).reshape(n, k + x, S)
    first, which = {}, np.empty(n, np.int64)
    for b in range(n):
        which[b] = first.setdefault((idx[b].tobytes(), have[b].tobytes()), b)
    words = {b: P.check_pair_block(k, m, idx[b], have[b], x) if x else 0 for b in sorted(set(first.values()))}
    return np.array([words[int(which[b])] for b in range(n)], dtype=np.uint32)

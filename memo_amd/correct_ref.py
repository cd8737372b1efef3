"""Host reference of memo_ec_correct_batch: the k + x shard check of
memo_amd/check_ref.py, and the wrong shard of every located block rewritten.

Pure numpy, built on check_ref (decode_rows, MUL, gf_inv, check_block); it
needs neither the GPU nor libmemo_ec.so.  It is the written-to-be-read form of
the call and the yardstick the device implementation is held to.

A block is located when its word is neither 0 nor VERDICT_INVALID, its shard
field is not VERDICT_UNLOCATED and S > 0.  With q the position of that shard
in the block's row of have_idx and D (x x k) the decode rows of the spares
over the basis, the shard in position q becomes

  q >= k (spare r = q - k)   sum_t D[r][t] * basis_t
  q <  k (a basis shard)     inv(D[0][q]) * (spare_0 XOR
                               sum_{t != q} D[0][t] * basis_t)

-- a one-row multiply-accumulate over k shards that never reads position q --
and bit 24 (VERDICT_CORRECTED) of the word is set; bits 0..23 stay the
check's.  Nothing else changes: clean, unlocated and invalid blocks, and every
block when x == 1, come back byte for byte.  A located shard is the code's
best explanation, not a proof (x = 2: two wrong shards can pass for one, and
the shard overwritten may have been right)."""
import numpy as np

from . import check_ref as R

VERDICT_CORRECTED = 1 << 24


def located_position(row, word, k, x):
    """Position q of the shard a word locates in its block's index row, or
    None when the word locates nothing."""
    word = int(word) & 0xFFFFFFFF
    if word == 0 or word == R.VERDICT_INVALID:
        return None
    shard = (word >> 16) & 0xFF
    if shard == R.VERDICT_UNLOCATED:
        return None
    hits = [t for t in range(k + x) if int(row[t]) == shard]
    return hits[0] if len(hits) == 1 else None


def mended_shard(k, m, row, shards, x, q):
    """The new bytes of position q by the two formulas: row = the block's
    k + x indices, shards ((k + x) x S uint8) in that order.  Position q is
    not read."""
    d = R.decode_rows(k, m, row[:k], row[k:k + x])
    out = np.zeros(shards.shape[1], dtype=np.uint8)
    if q >= k:
        for t in range(k):
            out ^= R.MUL[d[q - k, t], shards[t]]
        return out
    out ^= shards[k]
    for t in range(k):
        if t != q:
            out ^= R.MUL[d[0, t], shards[t]]
    return R.MUL[R.gf_inv(int(d[0, q])), out]


def correct_reference(k, m, have_idx, have, x=None, S=None):
    """(verdict, have_after) of n blocks: have_idx n x (k + x) shard indices,
    have n x (k + x) x S bytes in that order (any shape with those sizes), as
    check_ref.check_reference takes them.  verdict: n uint32 words; have_after:
    a new n x (k + x) x S array."""
    have_idx = np.asarray(have_idx, dtype=np.uint8)
    if x is None:
        if have_idx.ndim != 2:
            raise ValueError("x is needed unless have_idx is n x (k + x)")
        x = have_idx.shape[1] - k
    verdict = R.check_reference(k, m, have_idx, have, x=x, S=S)  # judges the arguments too
    have_idx = have_idx.reshape(-1, k + x)
    n = have_idx.shape[0]
    have = np.asarray(have, dtype=np.uint8)
    if S is None:
        S = have.size // (n * (k + x)) if n and x else 0
    if x == 0 or n == 0:
        return verdict, have.copy()
    after = have.reshape(n, k + x, S).copy()
    if S == 0 or x < 2:
        return verdict, after
    for b in range(n):
        q = located_position(have_idx[b], verdict[b], k, x)
        if q is None:
            continue
        after[b, q] = mended_shard(k, m, have_idx[b], after[b], x, q)
        verdict[b] |= VERDICT_CORRECTED
    return verdict, after

"""Host reference of memo_ec_check_pair_batch: the k + x shard check
(memo_amd/check_ref.py), and for a block it leaves unlocated the two wrong
shards, when exactly one pair of shards explains every mismatch.

Pure numpy on check_ref's tables; it needs neither the GPU nor libmemo_ec.so,
and is written as the definition reads, not to be fast.

With check_ref's notation -- D (x x k) the decode rows of the spares over the
basis, s[p] the syndrome vector at byte p -- let H = [D | I_x] be the
x x (k + x) matrix with one column per POSITION q of have_idx: column q < k is
D[:, q], column k + r the unit vector e_r.  A set E of positions explains the
block when s[p] lies in span{H_q : q in E} at every byte p.  check_ref's shard
field is "some one position explains"; here

  the word is check_ref's, bit for bit, unless x >= 3, S > 0, that word is
  nonzero, is not VERDICT_INVALID, its shard field is VERDICT_UNLOCATED, and
  EXACTLY ONE pair of positions {a, b} explains the block.  Then
    bits 0..15   the check's mask
    bits 16..23  the smaller of the two shard INDICES (values of have_idx)
    bit 24       zero
    bits 25..31  the larger index plus 1 (1..80)

In every other word bits 25..31 are zero; VERDICT_INVALID stays all ones.

The code is MDS, so any min(x, .) columns of H are independent.  With x >= 4
at most one pair explains an unlocated block (two disjoint pairs would force
every syndrome to zero, two pairs sharing q would make q alone explain it), so
two wrong shards are always named.  With x = 3 the pair is unique when the
syndromes span two dimensions; when they are all proportional, two pairs can
explain the same block, and the word stays unlocated.  With x <= 2 every pair
explains everything: the words are check_ref's.  A located pair is the code's
best explanation, not a proof: three wrong shards can pass for two."""
import itertools

import numpy as np

from . import check_ref as R

VERDICT_UNLOCATED = R.VERDICT_UNLOCATED
VERDICT_INVALID = R.VERDICT_INVALID


def syndromes(k, m, row, shards, x):
    """(D, syn): the decode rows (x x k) and the syndromes (x x S) of one
    block with a valid index set."""
    d = R.decode_rows(k, m, row[:k], row[k:k + x])
    syn = shards[k:k + x].copy()
    for r in range(x):
        for t in range(k):
            syn[r] ^= R.MUL[d[r, t], shards[t]]
    return d, syn


def explains(cols, syn):
    """Is every column of syn (x x ns) in the span of the independent columns
    cols (x x e)?  rank [cols | s] == e for every s, by one row reduction of
    [cols | syn] on pivots in cols: what is left of a syndrome in the rows
    without a pivot must be zero."""
    x, e = cols.shape
    w = np.concatenate([cols, syn], axis=1).astype(np.uint8)
    used = []
    for c in range(e):
        piv = next((r for r in range(x) if r not in used and w[r, c]), None)
        if piv is None:
            raise ValueError("dependent columns")
        w[piv] = R.MUL[R.gf_inv(int(w[piv, c])), w[piv]]
        f = w[:, c].copy()
        f[piv] = 0
        w ^= R.MUL[f[:, None], w[piv][None, :]]
        used.append(piv)
    rest = [r for r in range(x) if r not in used]
    return not w[rest, e:].any()


def explaining_pairs(k, m, row, shards, x):
    """Every pair of positions (a < b) that explains the block."""
    d, syn = syndromes(k, m, row, shards, x)
    h = np.concatenate([d, np.eye(x, dtype=np.uint8)], axis=1)
    s = np.unique(syn[:, syn.any(axis=0)].T, axis=0).T  # the distinct nonzero syndrome vectors
    return [(a, b) for a, b in itertools.combinations(range(k + x), 2) if explains(h[:, [a, b]], s)]


def qualifies(word, x, S):
    """Does the check's word leave room for a pair?"""
    word = int(word)
    return (x >= 3 and S > 0 and word != 0 and word != VERDICT_INVALID
            and (word >> 16) & 0xFF == VERDICT_UNLOCATED)


def pair_word(mask, idx_a, idx_b):
    lo, hi = min(int(idx_a), int(idx_b)), max(int(idx_a), int(idx_b))
    return (mask & 0xFFFF) | (lo << 16) | ((hi + 1) << 25)


def check_pair_block(k, m, row, shards, x):
    """The verdict word of one block: row = its k + x indices, shards
    ((k + x) x S uint8) in that order."""
    word = R.check_block(k, m, row, shards, x)
    if not qualifies(word, x, shards.shape[1]):
        return word
    pairs = explaining_pairs(k, m, row, shards, x)
    if len(pairs) != 1:
        return word
    a, b = pairs[0]
    return pair_word(word, row[a], row[b])


def check_pair_reference(k, m, have_idx, have, x=None, S=None):
    """verdict (n uint32 words) of n blocks; arguments as for
    check_ref.check_reference."""
    have_idx = np.asarray(have_idx, dtype=np.uint8)
    if x is None:
        if have_idx.ndim != 2:
            raise ValueError("x is needed unless have_idx is n x (k + x)")
        x = have_idx.shape[1] - k
    if not (1 <= k <= R.MAX_K and 0 <= m <= R.MAX_M) or not 0 <= x <= m:
        raise ValueError("need 1 <= k <= %d, 0 <= x <= m <= %d" % (R.MAX_K, R.MAX_M))
    have_idx = have_idx.reshape(-1, k + x)
    n = have_idx.shape[0]
    out = np.zeros(n, dtype=np.uint32)
    if x == 0 or n == 0:
        return out
    have = np.asarray(have, dtype=np.uint8)
    if S is None:
        if have.size % (n * (k + x)):
            raise ValueError("have does not hold n x (k + x) shards of one size")
        S = have.size // (n * (k + x))
    have = have.reshape(n, k + x, S)
    for b in range(n):
        out[b] = check_pair_block(k, m, have_idx[b], have[b], x)
    return out


def split_verdict_pair(v):
    """(mask, shard, second) of a verdict word that is neither 0 nor
    VERDICT_INVALID: second is the larger shard index of a located pair (shard
    is then the smaller), None when the word names no pair."""
    v = int(v) & 0xFFFFFFFF
    hi = (v >> 25) & 0x7F
    return v & 0xFFFF, (v >> 16) & 0xFF, hi - 1 if hi else None

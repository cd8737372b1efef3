"""Host reference of memo_ec_correct_pair_batch: the pair check of
memo_amd/check_pair_ref.py, the single correction of memo_amd/correct_ref.py
for the blocks the check locates, and both named shards of every pair block
rewritten.

Pure numpy on check_ref's tables; it needs neither the GPU nor libmemo_ec.so,
and is written as the definition reads, not to be fast.

A block's word is check_pair_ref's.  When it names one shard, the block is
correct_ref's: that shard rewritten, bit 24 set.  When it names a pair, the
shards in the positions qa < qb of the two named indices become the rebuild of
those two shards from the k positions input_positions(k, x, qa, qb) -- any k
positions determine the block (the code is MDS), and this fixed choice only
matters when more than two shards are wrong -- and bit 24 (VERDICT_CORRECTED)
of the pair word is set.  Every other block comes back byte for byte.

A named pair is the code's best explanation, not a proof: three wrong shards
can pass for two, and both shards overwritten may have been right."""
import numpy as np

from . import check_pair_ref as P
from . import check_ref as R
from . import correct_ref as C

VERDICT_CORRECTED = C.VERDICT_CORRECTED


def input_positions(k, x, qa, qb):
    """The k positions the rebuild of the targets qa < qb reads, by input
    slot: basis position j is slot j; the slot of each basis target is filled
    by a spare position that is no target, the lowest such spares in
    ascending order."""
    if not 0 <= qa < qb < k + x:
        raise ValueError("need 0 <= qa < qb < k + x")
    free = (k + r for r in range(x) if k + r not in (qa, qb))
    return [next(free) if j in (qa, qb) else j for j in range(k)]


def pair_positions(row, word, k, x):
    """Positions (qa < qb) of the two shards a word names in its block's index
    row, or None when the word names no pair."""
    word = int(word) & 0xFFFFFFFF
    if word == R.VERDICT_INVALID or (word >> 25) == 0:
        return None
    lo, hi = (word >> 16) & 0xFF, ((word >> 25) & 0x7F) - 1
    qs = sorted(t for t in range(k + x) if int(row[t]) in (lo, hi))
    return tuple(qs) if len(qs) == 2 else None


def rebuilt_pair(k, m, row, shards, pos, qa, qb):
    """The shards of positions qa and qb (2 x S) rebuilt from the k positions
    `pos`: shard row[q] = sum_t D[.][t] * shard row[pos[t]], D the decode rows
    of the two lost indices over the k surviving ones."""
    d = R.decode_rows(k, m, [int(row[p]) for p in pos], [int(row[qa]), int(row[qb])])
    out = np.zeros((2, shards.shape[1]), dtype=np.uint8)
    for i in range(2):
        for t in range(k):
            out[i] ^= R.MUL[d[i, t], shards[pos[t]]]
    return out


def correct_pair_reference(k, m, have_idx, have, x=None, S=None):
    """(verdict, have_after) of n blocks; arguments as for
    correct_ref.correct_reference."""
    have_idx = np.asarray(have_idx, dtype=np.uint8)
    if x is None:
        if have_idx.ndim != 2:
            raise ValueError("x is needed unless have_idx is n x (k + x)")
        x = have_idx.shape[1] - k
    verdict, after = C.correct_reference(k, m, have_idx, have, x=x, S=S)  # judges the arguments too
    have_idx = have_idx.reshape(-1, k + x)
    n = have_idx.shape[0]
    if x < 3 or n == 0 or after.ndim != 3 or after.shape[2] == 0:
        return verdict, after
    before = np.asarray(have, dtype=np.uint8).reshape(after.shape)
    for b in range(n):
        if not P.qualifies(verdict[b], x, after.shape[2]):
            continue  # clean, invalid, or a single the lines above mended
        word = P.check_pair_block(k, m, have_idx[b], before[b], x)
        qs = pair_positions(have_idx[b], word, k, x)
        if qs is None:
            continue
        qa, qb = qs
        after[b, [qa, qb]] = rebuilt_pair(k, m, have_idx[b], before[b], input_positions(k, x, qa, qb), qa, qb)
        verdict[b] = word | VERDICT_CORRECTED
    return verdict, after

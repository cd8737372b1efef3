"""Host reference of the k + x shard check ("Next" item
5): do the shards in hand of a block agree, and if not, which one is wrong.

Pure numpy over GF(2^8) (polynomial 0x11D, generator 2) and the systematic
Cauchy generator of DESIGN.md section 2; it needs neither the GPU nor
libmemo_ec.so.  It is the slow, written-to-be-read form of the verdict: for
tools and tests that must judge a set of shards without a device, and the
yardstick a device implementation of the call is held to.

A block's shards in hand are named by a row of have_idx: entries 0..k-1 are
its basis, entries k..k+x-1 its spares (1 <= x <= m), in any order.  With D
(x x k) the decode rows of the spares over the basis and
s_r = spare r XOR sum_t D[r][t] * basis_t, the verdict word is

  0                          every s_r is zero everywhere
  mask | shard << 16         bit r of mask (bits 0..15): s_r is nonzero
                             somewhere; shard (bits 16..23): the shard INDEX
                             (a value of have_idx) that explains every
                             mismatch --
                               have_idx[k + r] when row r alone differs,
                               have_idx[t] when all x rows differ and
                               s_r[p] * D[0][t] == D[r][t] * s_0[p] at every
                               byte p and row r,
                               VERDICT_UNLOCATED when no such t exists, for
                               any other mask, and always for x == 1
  VERDICT_INVALID            the index set is invalid: an index >= k + m, or
                             one that repeats

The code is MDS, so every entry of D is nonzero and D[r][t] / D[0][t] is
injective in t: at most one t fits.  With have_idx = 0..k+m-1 and x = m the
words are those of memo_ec_verify_batch.  A located shard is the code's best
explanation, not a proof (x = 2: two wrong shards can pass for one)."""
import numpy as np

VERDICT_UNLOCATED = 0xFF
VERDICT_INVALID = 0xFFFFFFFF
MAX_K, MAX_M = 64, 16

_EXP = np.zeros(512, dtype=np.uint8)
_LOG = np.zeros(256, dtype=np.int64)
_v = 1
for _i in range(255):
    _EXP[_i] = _EXP[_i + 255] = _v
    _LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= 0x11D
del _v, _i
# MUL[a, b] = a * b
_a = np.arange(256)
MUL = _EXP[(_LOG[_a][:, None] + _LOG[_a][None, :]) % 255].astype(np.uint8)
MUL[0, :] = 0
MUL[:, 0] = 0
del _a


def gf_inv(a):
    if a == 0:
        raise ZeroDivisionError("0 has no inverse in GF(2^8)")
    return int(_EXP[255 - _LOG[a]])


def generator(k, m):
    """(k + m) x k: identity over the rows 1 / (i XOR j), i >= k."""
    if not (1 <= k <= MAX_K and 0 <= m <= MAX_M):
        raise ValueError("bad (k, m)")
    g = np.zeros((k + m, k), dtype=np.uint8)
    g[:k] = np.eye(k, dtype=np.uint8)
    for i in range(k, k + m):
        for j in range(k):
            g[i, j] = gf_inv(i ^ j)
    return g


def matmul(a, b):
    """a (p x q) * b (q x r) over GF(2^8)."""
    out = np.zeros((a.shape[0], b.shape[1]), dtype=np.uint8)
    for t in range(a.shape[1]):
        out ^= MUL[a[:, t][:, None], b[t][None, :]]
    return out


def invert(a):
    """Inverse of a square matrix by Gauss-Jordan; ValueError when singular."""
    n = a.shape[0]
    w = np.concatenate([a.astype(np.uint8), np.eye(n, dtype=np.uint8)], axis=1)
    for c in range(n):
        piv = next((r for r in range(c, n) if w[r, c]), None)
        if piv is None:
            raise ValueError("singular")
        if piv != c:
            w[[c, piv]] = w[[piv, c]]
        w[c] = MUL[gf_inv(int(w[c, c])), w[c]]
        for r in range(n):
            if r != c and w[r, c]:
                w[r] ^= MUL[w[r, c], w[c]]
    return w[:, n:].copy()


def decode_rows(k, m, basis, spares):
    """D (len(spares) x k): shard spares[r] = sum_t D[r][t] * shard basis[t]."""
    g = generator(k, m)
    return matmul(g[np.asarray(spares, dtype=np.int64)], invert(g[np.asarray(basis, dtype=np.int64)]))


def valid_index_set(k, m, row):
    row = [int(v) for v in row]
    return all(0 <= v < k + m for v in row) and len(set(row)) == len(row)


def check_block(k, m, row, shards, x):
    """The verdict word of one block: row = its k + x indices, shards
    ((k + x) x S uint8) in that order."""
    if not valid_index_set(k, m, row):
        return VERDICT_INVALID
    d = decode_rows(k, m, row[:k], row[k:k + x])
    syn = shards[k:k + x].copy()
    for r in range(x):
        for t in range(k):
            syn[r] ^= MUL[d[r, t], shards[t]]
    lit = syn.any(axis=1)
    mask = sum(1 << r for r in range(x) if lit[r])
    if mask == 0:
        return 0
    shard = VERDICT_UNLOCATED
    if x >= 2 and bin(mask).count("1") == 1:
        shard = int(row[k + int(np.flatnonzero(lit)[0])])
    elif x >= 2 and mask == (1 << x) - 1:
        s = syn[:, syn.any(axis=0)]  # consistent bytes constrain nothing
        fits = [t for t in range(k)
                if all(np.array_equal(MUL[s[r], d[0, t]], MUL[d[r, t], s[0]]) for r in range(1, x))]
        if len(fits) == 1:
            shard = int(row[fits[0]])
    return mask | (shard << 16)


def check_reference(k, m, have_idx, have, x=None, S=None):
    """verdict (n uint32 words) of n blocks: have_idx n x (k + x) shard
    indices, have n x (k + x) x S bytes in that order (any shape with those
    sizes).  x defaults to have_idx's row length - k, S to what have holds.
    x == 0 or n == 0 gives zeros."""
    have_idx = np.asarray(have_idx, dtype=np.uint8)
    if x is None:
        if have_idx.ndim != 2:
            raise ValueError("x is needed unless have_idx is n x (k + x)")
        x = have_idx.shape[1] - k
    if not (1 <= k <= MAX_K and 0 <= m <= MAX_M) or not 0 <= x <= m:
        raise ValueError("need 1 <= k <= %d, 0 <= x <= m <= %d" % (MAX_K, MAX_M))
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
        out[b] = check_block(k, m, have_idx[b], have[b], x)
    return out


def split_verdict(v):
    """(mask, shard) of a verdict word that is neither 0 nor VERDICT_INVALID."""
    v = int(v) & 0xFFFFFFFF
    return v & 0xFFFF, (v >> 16) & 0xFF

"""The families of tests/test_gpu_check_sweep.py: batches for
memo_ec_check_batch, memo_ec_check_pair_batch and memo_ec_correct_batch in
which every byte position, lane, wave, stride round, position of the code,
pair of positions and grid round decides some block's word.  No test lives
here; tests/test_check_sweep_cases.py holds every family to the host
references without a GPU, tests/test_gpu_check_sweep.py runs them on the
device.

Every expected word comes from the construction -- which positions were
changed, and by what bytes -- never from a search:
  one wrong position q      correct_cases.single_word without bit 24
  two wrong positions       check_pair_ref.pair_word of the planted pair
  what stays unlocated      mask | UNLOCATED << 16
The mask of a block with more than one wrong position is formed from the
planted error bytes alone (error_mask: the syndromes are linear in them).  The
one exception is named where it is made: with x = 3 a pair of errors at one
offset is named or left unlocated as the reference says.

A family is built once (functools.lru_cache) and its arrays are read-only;
of A1's parts only the last one asked for is kept (they are the large ones).
The three batches too long to keep distinct blocks for (a second grid round)
are a pool of distinct blocks and `sel`, the pool index of every block of the
batch: a reference judges the pool, full() makes the batch."""
import collections
import functools
import itertools

import numpy as np

from conftest import SEED
from correct_cases import CORRECTED, oracle, overwrite, single_word
from test_check_restated import UNLOCATED, random_sets, shards_of, take

# shape: (k, m, x, S).  idx, clean, have, want: one entry per distinct block
# (clean: the shards before anything was planted; want: the words of the call
# the family is for).  truth[b]: the positions changed in block b.  sel: None,
# or the pool index of every block of the batch.
Family = collections.namedtuple("Family", "shape idx clean have want truth sel")

# launch_check_locate and launch_check_pair (memo_amd/csrc/ec_kernels.hip): one
# workgroup per 64 verdict words, at most 2048.  correct::list_grid_for
# (memo_amd/csrc/correct_plan.h): one per 256 words, at most kListGridCap =
# 1024.  The numbers are those of the sources' text, as
# tests/test_gpu_verify_sweep.py follows launch_verify_locate's;
# tests/test_check_sweep_cases.py reads them there again.
LOCATE_GRID, LOCATE_WORDS = 2048, 64
LIST_GRID, LIST_WORDS = 1024, 256


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def family(shape, idx, clean, have, want, truth, sel=None):
    frozen(idx, clean, have, want)
    if sel is not None:
        frozen(sel)
    return Family(shape, idx, clean, have, want, tuple(tuple(t) for t in truth), sel)


def full(f, what=None):
    """(n, idx, have, want) of the whole batch; `what` in place of f.want."""
    want = f.want if what is None else what
    if f.sel is None:
        return f.idx.shape[0], f.idx, f.have, want
    return f.sel.size, f.idx[f.sel], f.have[f.sel], want[f.sel]


def base(shape, n, tag):
    """(rng, idx, clean): n clean blocks on random index sets (parity shards
    in the basis, data among the spares, every block its own set)."""
    k, m, x, S = shape
    rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + x * 101 + S * 31 + tag * 7919))
    idx = random_sets(rng, k, m, x, n)
    clean = take(shards_of(oracle(), k, m, S, rng, n), idx)
    return rng, idx, clean


def nonzero(rng):
    return int(rng.integers(1, 256))


def check_word(idx, b, pos, k, x):
    """The check's word of block b with position pos alone wrong (x >= 2)."""
    return single_word(idx, b, pos, k, x) & ~CORRECTED


def unlocated(mask):
    return mask | (UNLOCATED << 16)


def error_mask(shape, row, err, truth):
    """The mask of a block from its planted errors alone: err ((k + x) x S) =
    have XOR clean, nonzero in the positions `truth` only.  With H = [D | I_x]
    the syndromes are sum_q H_q * err[q]; bit r is set when row r of that is
    nonzero somewhere."""
    from memo_amd import check_ref as R
    k, m, x, S = shape
    assert not np.delete(err, list(truth), axis=0).any()
    h = np.concatenate([R.decode_rows(k, m, row[:k], row[k:k + x]), np.eye(x, dtype=np.uint8)], axis=1)
    syn = np.zeros((x, S), np.uint8)
    for q in truth:
        syn ^= R.MUL[h[:, q][:, None], err[q][None, :]]
    return sum(1 << r for r in range(x) if syn[r].any())


def block_mask(shape, idx, clean, have, b, truth):
    return error_mask(shape, idx[b], have[b] ^ clean[b], truth)


def pair_word(mask, idx, b, qa, qb):
    from memo_amd import check_pair_ref as P
    return P.pair_word(mask, idx[b, qa], idx[b, qb])


# ------------------------------------------------------------------ references
def check_words(f):
    """check_ref's words of the family's distinct blocks (equal blocks are
    judged once, as test_gpu_check.reference does)."""
    from memo_amd import check_ref as R
    k, m, x, S = f.shape
    n = f.idx.shape[0]
    first, which = {}, np.empty(n, np.int64)
    for b in range(n):
        which[b] = first.setdefault((f.idx[b].tobytes(), f.have[b].tobytes()), len(first))
    pick = np.array([int(np.flatnonzero(which == u)[0]) for u in range(len(first))])
    return R.check_reference(k, m, f.idx[pick], f.have[pick], x=x, S=S)[which]


def pair_words(f):
    """check_pair_ref's words of the family's distinct blocks."""
    import check_pair_cases as C
    k, m, x, S = f.shape
    return C.pair_reference(k, m, x, S, f.idx, f.have)


def correct_words(f):
    """(words, after) of correct_ref on the family's distinct blocks."""
    from memo_amd import correct_ref as C
    k, m, x, S = f.shape
    return C.correct_reference(k, m, f.idx, f.have.reshape(f.idx.shape[0], -1), x=x, S=S)


# --------------------------------------------------- A: memo_ec_check_batch
# A1: (shape, first offset, end offset).  RS(10,4) x 4160 B is run a quarter
# of its offsets a call (61 MB each; all 4160 blocks at once would be 242 MB).
A1_WHOLE = ((4, 3, 3, 1088), 0, 1088)
A1_QUARTERS = tuple(((10, 4, 4, 4160), q * 1040, (q + 1) * 1040) for q in range(4))
A1_PARTS = (A1_WHOLE,) + A1_QUARTERS


@functools.lru_cache(maxsize=1)  # one part at a time: an RS(10,4) quarter holds 2 x 61 MB
def every_byte(shape, lo, hi):
    """A1: block i is wrong at byte p = lo + i alone, in position
    p % (k + x), bit 1 << (p % 8)."""
    k, m, x, S = shape
    n = hi - lo
    _, idx, clean = base(shape, n, 0xA1 + lo)
    have, want, truth = clean.copy(), np.zeros(n, np.uint32), []
    for i in range(n):
        p = lo + i
        pos = p % (k + x)
        have[i, pos, p] ^= 1 << (p % 8)
        want[i] = check_word(idx, i, pos, k, x)
        truth.append((pos,))
    return family(shape, idx, clean, have, want, truth)


A2_SHAPE = (4, 3, 3, 1088)


def a2_cases():
    W = A2_SHAPE[3] // 4
    k = A2_SHAPE[0]
    return ([("a", w) for w in range(1, W)] + [("b", w) for w in range(W - 1)] +
            [("c", w) for w in range(W)] + [("d", j) for j in range(k)])


@functools.lru_cache(maxsize=None)
def disqualifying_byte():
    """A2: the four families of test_gpu_verify_sweep.test_disqualifying_byte_
    in_every_lane over basis positions j1, j2 of random index sets; wrong
    blocks odd, clean blocks even.  x = 3: two wrong shards never pass for
    one, so (a)-(c) are unlocated with every row lit, (d) is located at j1."""
    shape = A2_SHAPE
    k, m, x, S = shape
    W = S // 4
    cases = a2_cases()
    n = 2 * len(cases) + 1
    rng, idx, clean = base(shape, n, 0xA2)
    have, want, truth = clean.copy(), np.zeros(n, np.uint32), [()] * n
    for c, (fam, w) in enumerate(cases):
        b = 2 * c + 1
        if fam == "d":
            j1 = w
            have[b, j1, 4 * np.arange(W) + np.arange(W) % 4] ^= rng.integers(1, 256, W, dtype=np.uint8)
            want[b] = check_word(idx, b, j1, k, x)
            truth[b] = (j1,)
            continue
        j1 = w % k
        j2 = (j1 + 1 + (w // k) % (k - 1)) % k
        assert j1 != j2
        if fam == "a":
            have[b, j1, w % 4] ^= nonzero(rng)
        elif fam == "b":
            have[b, j1, 4 * (W - 1) + w % 4] ^= nonzero(rng)
        else:
            have[b, j1] ^= rng.integers(1, 256, S, dtype=np.uint8)
        have[b, j2, 4 * w + w % 4] ^= nonzero(rng)
        want[b] = unlocated((1 << x) - 1)
        truth[b] = (j1, j2)
    return family(shape, idx, clean, have, want, truth)


LIMIT = (64, 16, 16, 64)


@functools.lru_cache(maxsize=None)
def every_limit_position():
    """A3: (64,16,16,64), n = 80: block b has position b wrong at one byte."""
    shape = LIMIT
    k, m, x, S = shape
    n = k + x
    _, idx, clean = base(shape, n, 0xA3)
    have, want = clean.copy(), np.zeros(n, np.uint32)
    for b in range(n):
        have[b, b, (7 * b + 3) % S] ^= 1 << (b % 8)
        want[b] = check_word(idx, b, b, k, x)
    return family(shape, idx, clean, have, want, [(b,) for b in range(n)])


@functools.lru_cache(maxsize=None)
def every_word_flagged():
    """A4: (10,4,4,448), n = 130, every block wrong, position b % 14."""
    shape = (10, 4, 4, 448)
    k, m, x, S = shape
    n = 130
    _, idx, clean = base(shape, n, 0xA4)
    have, want = clean.copy(), np.zeros(n, np.uint32)
    for b in range(n):
        have[b, b % (k + x), (37 * b) % S] ^= 1 << (b % 8)
        want[b] = check_word(idx, b, b % (k + x), k, x)
    return family(shape, idx, clean, have, want, [(b % (k + x),) for b in range(n)])


def round_places(grid, words):
    """(n, places) of a batch of grid * words + words + 3 blocks: the first
    and last block of round one's first and last workgroups, and of round
    two's two workgroups (the second a partial one of three blocks)."""
    first2 = grid * words
    n = first2 + words + 3
    return n, [0, words - 1, first2 - words, first2 - 1, first2, first2 + words - 1, first2 + words, n - 1]


@functools.lru_cache(maxsize=None)
def check_second_round():
    """A5: (3,2,2,64), n = 2048 * 64 + 64 + 3: one clean block repeated, a
    block with one wrong byte (each its own position and index set) at the
    eight round_places, and one with two wrong basis shards at different
    bytes (x = 2: each byte alone names another shard, so unlocated) inside
    round two."""
    shape = (3, 2, 2, 64)
    k, m, x, S = shape
    n, places = round_places(LOCATE_GRID, LOCATE_WORDS)
    _, idx, clean = base(shape, 10, 0xA5)
    have, want, truth = clean.copy(), np.zeros(10, np.uint32), [()] * 10
    for i in range(8):
        pos = i % (k + x)
        have[1 + i, pos, (11 * i + 3) % S] ^= 1 << (i % 8)
        want[1 + i] = check_word(idx, 1 + i, pos, k, x)
        truth[1 + i] = (pos,)
    have[9, 0, 5] ^= 0x21
    have[9, 2, 40] ^= 0x84
    want[9] = unlocated(0x3)
    truth[9] = (0, 2)
    sel = np.zeros(n, np.int32)
    sel[places] = 1 + np.arange(8)
    sel[LOCATE_GRID * LOCATE_WORDS + 10] = 9
    return family(shape, idx, clean, have, want, truth, sel)


# ---------------------------------------------- B: memo_ec_check_pair_batch
def plant_pair(have, b, qa, qb, pa, pb, rng):
    have[b, qa, pa] ^= nonzero(rng)
    have[b, qb, pb] ^= nonzero(rng)


def pair_offsets(b, S, how):
    """"same": one offset, rank 1; "apart": two offsets, rank 2."""
    pa = (7 * b) % S
    return pa, pa if how == "same" else (7 * b + S // 2 + 1) % S


def pair_blocks(shape, pairs, tag):
    """Block 2 i is pair i "same", block 2 i + 1 pair i "apart".  x >= 4, and
    x = 3 "apart": the planted pair is named.  x = 3 "same": the word is the
    reference's, which is that or the check's unlocated word (two pairs can
    explain a rank-1 block)."""
    from memo_amd import check_pair_ref as P
    k, m, x, S = shape
    n = 2 * len(pairs)
    rng, idx, clean = base(shape, n, tag)
    have, want, truth = clean.copy(), np.zeros(n, np.uint32), []
    for b in range(n):
        qa, qb = pairs[b // 2]
        how = ("same", "apart")[b % 2]
        plant_pair(have, b, qa, qb, *pair_offsets(b, S, how), rng)
        mask = block_mask(shape, idx, clean, have, b, (qa, qb))
        want[b] = pair_word(mask, idx, b, qa, qb)
        if x == 3 and how == "same":
            ref = P.check_pair_block(k, m, idx[b], have[b], x)
            assert ref in (int(want[b]), unlocated(mask)), (b, hex(ref))
            want[b] = ref
        truth.append((qa, qb))
    return family(shape, idx, clean, have, want, truth)


B1_SHAPES = [(4, 4, 4, 64), (10, 4, 4, 448), (10, 4, 3, 448)]


@functools.lru_cache(maxsize=None)
def every_pair(shape):
    """B1: all C(k + x, 2) pairs of positions, each "same" and "apart"."""
    k, m, x, S = shape
    return pair_blocks(shape, list(itertools.combinations(range(k + x), 2)), 0xB1)


B2_PAIRS = [(a, b) for a in (0, 31, 32, 63, 64, 79) for b in (1, 33, 62, 63, 64, 65, 78, 79) if a < b]


@functools.lru_cache(maxsize=None)
def limit_pairs():
    """B2: (64,16,16,64), the pairs around positions 31/32, 63/64 and 79."""
    return pair_blocks(LIMIT, B2_PAIRS, 0xB2)


@functools.lru_cache(maxsize=None)
def walk1():
    """B3: (10,4,4,1088), n = 1088: block b has two shards wrong at byte b and
    nowhere else (rank 1; x = 4 names the pair)."""
    shape = (10, 4, 4, 1088)
    k, m, x, S = shape
    kx, n = k + x, S
    rng, idx, clean = base(shape, n, 0xB3)
    have, want, truth = clean.copy(), np.zeros(n, np.uint32), []
    for b in range(n):
        qa = b % kx
        qb = (qa + 1 + (b // kx) % (kx - 1)) % kx
        plant_pair(have, b, qa, qb, b, b, rng)
        want[b] = pair_word(block_mask(shape, idx, clean, have, b, (qa, qb)), idx, b, qa, qb)
        truth.append((qa, qb))
    return family(shape, idx, clean, have, want, truth)


B4_SHAPES = [(4, 3, 3, 1088), (10, 4, 3, 1088)]


@functools.lru_cache(maxsize=None)
def ambiguous_factor(shape):
    """(idx row, clean block, e, c) for B4: errors e (nonzero everywhere) in
    position 0 and c * e in position 1 of a seeded block give syndromes that
    are all multiples of v = H_0 + c * H_1; c is the first factor for which a
    second pair's columns span v too (check_pair_ref.explains), so the block
    stays unlocated.  The search asserts that it found one."""
    from memo_amd import check_pair_ref as P, check_ref as R
    k, m, x, S = shape
    assert x == 3
    rng, idx, clean = base(shape, 1, 0xB4)
    row = idx[0]
    h = np.concatenate([R.decode_rows(k, m, row[:k], row[k:k + x]), np.eye(x, dtype=np.uint8)], axis=1)
    e = rng.integers(1, 256, S, dtype=np.uint8)
    for c in range(1, 256):
        v = (h[:, 0] ^ R.MUL[c, h[:, 1]])[:, None]
        pairs = [pq for pq in itertools.combinations(range(k + x), 2) if P.explains(h[:, list(pq)], v)]
        assert (0, 1) in pairs
        if len(pairs) >= 2:
            return row, clean[0], e, c
    assert False, "no factor c makes positions (0, 1) ambiguous for %r" % (shape,)


@functools.lru_cache(maxsize=None)
def walk2(shape):
    """B4: block 0 is the rank-1 block of ambiguous_factor (unlocated: the
    control); block 1 + w is the same plus one more byte flipped in position 1
    at offset 4 w + w % 4, the only syndrome off the line: rank 2, which names
    positions {0, 1}."""
    from memo_amd import check_ref as R
    k, m, x, S = shape
    row, blk, e, c = ambiguous_factor(shape)
    W = S // 4
    n = 1 + W
    rng = np.random.default_rng(SEED + 0xB4 + k)
    idx = np.tile(row, (n, 1))
    clean = np.tile(blk, (n, 1, 1))
    have = clean.copy()
    have[:, 0] ^= e
    have[:, 1] ^= R.MUL[c, e]
    want = np.zeros(n, np.uint32)
    want[0] = unlocated(block_mask(shape, idx, clean, have, 0, (0, 1)))
    for w in range(W):
        have[1 + w, 1, 4 * w + w % 4] ^= nonzero(rng)
        want[1 + w] = pair_word(block_mask(shape, idx, clean, have, 1 + w, (0, 1)), idx, 1 + w, 0, 1)
    return family(shape, idx, clean, have, want, [(0, 1)] * n)


B5_SHAPES = [(4, 3, 3, 1088), (10, 4, 4, 1088)]


@functools.lru_cache(maxsize=None)
def walk3(shape):
    """B5: every block has two whole shards wrong; block 0 nothing else (the
    control: the pair is named), block 1 + w a third shard wrong at byte
    4 w + w % 4: three independent columns, rank 3, the check's word."""
    k, m, x, S = shape
    W = S // 4
    n = 1 + W
    rng, idx, clean = base(shape, n, 0xB5)
    have, want, truth = clean.copy(), np.zeros(n, np.uint32), []
    for b in range(n):
        qa, qb, qc = (int(q) for q in rng.permutation(k + x)[:3])
        have[b, qa] ^= rng.integers(1, 256, S, dtype=np.uint8)
        have[b, qb] ^= rng.integers(1, 256, S, dtype=np.uint8)
        if b == 0:
            want[b] = pair_word(block_mask(shape, idx, clean, have, b, (qa, qb)), idx, b, qa, qb)
            truth.append((qa, qb))
            continue
        w = b - 1
        have[b, qc, 4 * w + w % 4] ^= nonzero(rng)
        want[b] = unlocated(block_mask(shape, idx, clean, have, b, (qa, qb, qc)))
        truth.append((qa, qb, qc))
    return family(shape, idx, clean, have, want, truth)


B6_SHAPE = (4, 4, 4, 64)


@functools.lru_cache(maxsize=None)
def every_word_a_pair():
    """B6: (4,4,4,64), n = 130, every block a pair block: the 28 pairs in
    turn, "same" and "apart" alternating."""
    k, m, x, S = B6_SHAPE
    pairs = list(itertools.combinations(range(k + x), 2))
    return pair_blocks(B6_SHAPE, [pairs[i % len(pairs)] for i in range(65)], 0xB6)


def plant_three(have, b, pos, S, rng):
    for q, p in zip(pos, (0, S - 1, S // 2)):
        have[b, q, p] ^= nonzero(rng)


@functools.lru_cache(maxsize=None)
def pair_second_round():
    """B6: (4,4,4,64), n = 2048 * 64 + 64 + 3: one clean block repeated; pair
    ("apart"), single and three-wrong blocks at the eight round_places and a
    pair block inside round two."""
    shape = B6_SHAPE
    k, m, x, S = shape
    n, places = round_places(LOCATE_GRID, LOCATE_WORDS)
    kinds = ["pair", "single", "three", "pair", "pair", "three", "single", "pair", "pair"]
    rng, idx, clean = base(shape, 1 + len(kinds), 0xB7)
    have, want, truth = clean.copy(), np.zeros(1 + len(kinds), np.uint32), [()]
    for i, kind in enumerate(kinds):
        b = 1 + i
        pos = tuple(int(q) for q in rng.permutation(k + x)[:{"single": 1, "pair": 2, "three": 3}[kind]])
        if kind == "single":
            have[b, pos[0], (11 * i + 3) % S] ^= 1 << (i % 8)
            want[b] = check_word(idx, b, pos[0], k, x)
        elif kind == "pair":
            plant_pair(have, b, pos[0], pos[1], *pair_offsets(b, S, "apart"), rng)
            want[b] = pair_word(block_mask(shape, idx, clean, have, b, pos), idx, b, *pos)
        else:
            plant_three(have, b, pos, S, rng)
            want[b] = unlocated(block_mask(shape, idx, clean, have, b, pos))
        truth.append(pos)
    sel = np.zeros(n, np.int32)
    sel[places] = 1 + np.arange(8)
    sel[LOCATE_GRID * LOCATE_WORDS + 10] = 9
    return family(shape, idx, clean, have, want, truth, sel)


# ------------------------------------------------ C: memo_ec_correct_batch
# C1: correct_cases.single_batch(correct_cases.SWEEP_RANGES), every block
# located; 3 tiles an entry, 2100 work items over 2048 workgroups.

C2_SHAPE = (10, 4, 3, 4160)


@functools.lru_cache(maxsize=None)
def interleaved():
    """C2: (10,4,3,4160), n = 24.  Even blocks and block 23: one shard
    overwritten, positions 0..12 in turn; the other odd blocks clean and, in
    turn, two basis shards wrong at one byte each (x = 3: unlocated).  want:
    the corrected words; the mended batch is `clean` in the located blocks and
    `have` elsewhere (after())."""
    shape = C2_SHAPE
    k, m, x, S = shape
    n = 24
    rng, idx, clean = base(shape, n, 0xC2)
    have, want, truth = clean.copy(), np.zeros(n, np.uint32), [()] * n
    for b in range(n):
        if b % 2 == 0 or b == n - 1:
            pos = b // 2 if b % 2 == 0 else k + x - 1
            overwrite(have, b, pos, rng)
            want[b] = single_word(idx, b, pos, k, x)
            truth[b] = (pos,)
        elif (b // 2) % 2:
            j1, j2 = b % k, (b + 3) % k
            have[b, j1, (97 * b) % S] ^= nonzero(rng)
            have[b, j2, (97 * b + 2081) % S] ^= nonzero(rng)
            want[b] = unlocated((1 << x) - 1)
            truth[b] = (j1, j2)
    assert sorted(t[0] for t in truth if len(t) == 1) == list(range(k + x))
    return family(shape, idx, clean, have, want, truth)


def after(f):
    """The batch after the call: blocks with one wrong position are `clean`
    again, every other block is as it was."""
    out = f.have.copy()
    for b, t in enumerate(f.truth):
        if len(t) == 1:
            out[b] = f.clean[b]
    return out


C3_WAVE = 2 * LIST_WORDS            # all 64 words of this wave located
C3_LANE63 = 5 * LIST_WORDS + 64 + 63  # the one located word of its wave


@functools.lru_cache(maxsize=None)
def list_second_round():
    """C3: (3,2,2,64), n = 1024 * 256 + 256 + 3: one clean block repeated;
    located blocks (15 kinds in turn, each its own position and index set) at
    the eight round_places of the list kernel, in all 64 words of the wave at
    C3_WAVE and in lane 63 alone of the wave that ends at C3_LANE63."""
    shape = (3, 2, 2, 64)
    k, m, x, S = shape
    n, places = round_places(LIST_GRID, LIST_WORDS)
    rng, idx, clean = base(shape, 16, 0xC3)
    have, want, truth = clean.copy(), np.zeros(16, np.uint32), [()]
    for b in range(1, 16):
        pos = b % (k + x)
        overwrite(have, b, pos, rng)
        want[b] = single_word(idx, b, pos, k, x)
        truth.append((pos,))
    located = places + list(range(C3_WAVE, C3_WAVE + 64)) + [C3_LANE63]
    sel = np.zeros(n, np.int32)
    sel[located] = 1 + np.arange(len(located)) % 15
    return family(shape, idx, clean, have, want, truth, sel)

"""Buffers and shards past 4 GiB at the cost of seconds: the shapes, the
periodic templates, the reduced references and the comparison behind
tests/test_gpu_wide_offsets.py (the device) and tests/test_wide_cases.py (the
proof, without a GPU, that these cases can fail).

A CPU oracle over 8 GiB is too slow, so the content is periodic and so is
what every call must produce from it:

  many blocks   block b holds template b % 7 of 7 distinct random blocks, and
                its index set, erasure pattern and output are template
                b % 7's ("blocks" layout);
  huge shards   byte i of shard j is tmpl[j][i % P], P = 7 * 4096 ("cols"
                layout; the code works column by column).

The oracle runs on the 7 templates (or on P-byte shards) only; the device
result is compared with the templates over the WHOLE buffer, in slices, with
plain torch operations that work on either device.  Strides and wrap distances
are powers of two, and neither 2^31 nor 2^32 is a multiple of 7 * 4096 or of a
block stride here (test_wide_cases.py), so a read or write displaced by 2^31
or 2^32 meets another template phase and shows in an output byte or in a
guard.

A verdict call that reads data and parity displaced the same way still says
"clean", so the verdict cases plant wrong bytes at high offsets (plant_groups)
and hold the whole verdict array to the numpy references (memo_amd/check_ref,
correct_ref, check_pair_ref) run on a REDUCED block: the tiles that hold a
planted byte plus one clean tile, under the block's own index set.  The
reduction is exact: every rule of a verdict word is an AND (or an OR) over
byte positions, and a position whose syndromes are all zero keeps every
candidate and lights no row.

Nothing here needs a GPU or libmemo_ec.so to import."""
import numpy as np

from guarded import FILL, GUARD, pattern
from memo_amd import check_pair_ref as PR
from memo_amd import check_ref as R
from memo_amd import correct_ref as CR

PERIOD = 7
TILE = 4096
CORRECTED = CR.VERDICT_CORRECTED
SLICE = 1 << 28       # bytes compared at once: no boolean temporary is larger
WORD_FILL = 0xA5A5A5A5

# (k, m, S, n): the three shapes, and the same with every boundary 2^16 times lower
SHAPE_A = dict(k=4, m=2, S=(1 << 20) + 4160, n=2045, tile=TILE, period=None, bounds=(1 << 31, 1 << 32))
SHAPE_B = dict(k=2, S=(1 << 31) + 3 * 4096 + 64, n=1, tile=TILE, period=PERIOD * TILE,
               bounds=(1 << 31, 1 << 32))
SHAPE_C = dict(k=4, m=2, S=64, n=(1 << 25) + 13, tile=TILE, period=None, bounds=(1 << 31, 1 << 32))
SMALL_A = dict(k=4, m=2, S=18, n=2045, tile=4, period=None, bounds=(1 << 15, 1 << 16))
SMALL_B = dict(k=2, S=(1 << 15) + 3 * 4 + 2, n=1, tile=4, period=PERIOD * 4, bounds=(1 << 15, 1 << 16))


def reduced_b(x, small=False):
    """Shape B for check_pair at k + x shards in hand, cut to the smallest
    shard whose last shard still straddles the upper boundary ((k + x) * S just
    past it, a partial last tile): shard offsets above the lower boundary are
    then no longer met inside one shard."""
    base = SMALL_B if small else SHAPE_B
    tile, hi = base["tile"], base["bounds"][1]
    S = -(-hi // (base["k"] + x) // tile) * tile + base["S"] % tile
    assert (base["k"] + x - 1) * S < hi < (base["k"] + x) * S and S < base["bounds"][0]
    return dict(base, S=S)


SMALL_C = dict(k=4, m=2, S=2, n=(1 << 16) + 13, tile=4, period=None, bounds=(1 << 15, 1 << 16))


# ------------------------------------------------------------------ layouts

class Layout:
    """What a buffer of `total` bytes must hold: a periodic template plus a
    few flipped bytes (flips: flat offset -> XOR value).
      blocks  tmpl (T, W): byte o is tmpl[(o // W) % T][o % W]
      cols    tmpl (rows, P), shards of S bytes: byte o is tmpl[o // S][(o % S) % P]"""

    def __init__(self, mode, tmpl, total, S=None, flips=None):
        assert mode in ("blocks", "cols")
        self.mode, self.total, self.S = mode, int(total), S
        self.tmpl = np.ascontiguousarray(tmpl, dtype=np.uint8)
        assert self.tmpl.ndim == 2
        assert mode == "blocks" or self.total == self.tmpl.shape[0] * S
        self.flips = dict(flips or {})
        self._dev = {}

    def base(self, o):
        """The template's byte at flat offset o."""
        if self.mode == "blocks":
            T, W = self.tmpl.shape
            return int(self.tmpl[(o // W) % T, o % W])
        return int(self.tmpl[o // self.S, (o % self.S) % self.tmpl.shape[1]])

    def flipped(self, flips):
        return Layout(self.mode, self.tmpl, self.total, self.S, flips)

    def on(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev = {key: torch.from_numpy(self.tmpl).to(device)}
        return self._dev[key]

    def drop(self):
        self._dev = {}

    def _pieces(self, buf):
        """(view of buf, matching template view, flat offset of the view's
        first byte, row length) per piece; the views broadcast against each
        other and no piece's comparison exceeds SLICE bytes."""
        t = self.on(buf.device)
        assert buf.numel() == self.total and buf.dim() == 1
        if self.mode == "blocks":
            T, W = self.tmpl.shape
            groups = self.total // (T * W)
            step = max(1, SLICE // (T * W))
            for g0 in range(0, groups, step):
                g1 = min(groups, g0 + step)
                yield buf[g0 * T * W:g1 * T * W].view(g1 - g0, T * W), t.view(1, T * W), g0 * T * W, T * W
            o = groups * T * W
            if o < self.total:
                yield buf[o:].view(1, -1), t.view(1, T * W)[:, :self.total - o], o, self.total - o
        else:
            rows, P = self.tmpl.shape
            S = self.S
            q = S // P
            step = max(1, SLICE // P)
            for j in range(rows):
                for g0 in range(0, q, step):
                    g1 = min(q, g0 + step)
                    yield (buf[j * S + g0 * P:j * S + g1 * P].view(g1 - g0, P), t[j].view(1, P),
                           j * S + g0 * P, P)
                if q * P < S:
                    yield buf[j * S + q * P:(j + 1) * S].view(1, -1), t[j, :S - q * P].view(1, -1), j * S + q * P, S - q * P


def fill(buf, lay):
    """buf (flat uint8 torch tensor) <- the layout's bytes, flips included."""
    for view, t, _, _ in lay._pieces(buf):
        view.copy_(t.expand_as(view))
    for o, v in lay.flips.items():
        buf[o] = lay.base(o) ^ v
    return buf


def mismatches(buf, lay, cap=32):
    """Flat offsets, ascending, at which buf differs from the bare template
    (the first `cap` per slice): the whole buffer is compared."""
    out = []
    for view, t, o, L in lay._pieces(buf):
        ne = view != t
        if bool(ne.any()):
            for r in ne.any(dim=1).nonzero().reshape(-1)[:cap].tolist():
                out += [o + r * L + c for c in ne[r].nonzero().reshape(-1)[:cap].tolist()]
        del ne
    return sorted(out)


def problems(name, buf, lay):
    """What is wrong with buf against the layout, as messages (none: it holds
    the template everywhere and exactly the flips)."""
    bad = mismatches(buf, lay)
    want = sorted(lay.flips)
    msgs = []
    if bad != want:
        extra = [o for o in bad if o not in lay.flips][:4]
        missing = [o for o in want if o not in bad][:4]
        msgs.append("%s: %d byte(s) off the template, want %d; unexpected at %s, flips not seen at %s"
                    % (name, len(bad), len(want), extra, missing))
    for o in want:
        got, exp = int(buf[o]), lay.base(o) ^ lay.flips[o]
        if got != exp:
            msgs.append("%s: byte %d is 0x%02X, want 0x%02X" % (name, o, got, exp))
    return msgs


def word_problems(name, words, want):
    """words (int32 or uint32, torch or numpy, any device) against want
    (block -> word): every other word must be 0; the whole array is looked at."""
    import torch
    if isinstance(words, np.ndarray):
        words = torch.from_numpy(words.view(np.int32))
    nz = words.nonzero().reshape(-1).cpu().numpy()
    got = {int(b): int(words[int(b)]) & 0xFFFFFFFF for b in nz[:64]}
    want = {int(b): int(w) for b, w in want.items() if w}
    msgs = []
    if len(nz) != len(want) or got != want:
        diff = sorted(set(got.items()) ^ set(want.items()))[:8]
        msgs.append("%s: %d nonzero word(s), want %d; differing (block, word): %s"
                    % (name, len(nz), len(want), [(b, hex(w)) for b, w in diff]))
    return msgs


class Guard:
    """One output (or in-place) buffer between two patterned guards of GUARD
    bytes, on `device`; payload: the flat uint8 view handed to the call."""

    def __init__(self, nbytes, device, preset=FILL):
        import torch
        self.n = int(nbytes)
        self.raw = torch.empty(self.n + 2 * GUARD, dtype=torch.uint8, device=device)
        self.pat = torch.from_numpy(pattern(GUARD)).to(device)
        self.raw[:GUARD] = self.pat
        self.raw[GUARD + self.n:] = self.pat
        self.payload = self.raw[GUARD:GUARD + self.n]
        if preset is not None:
            self.payload.fill_(preset)

    def words(self):
        import torch
        return self.payload.view(torch.int32)

    def problems(self, name):
        import torch
        return ["%s: guard %s the payload written" % (name, side)
                for side, g in (("before", self.raw[:GUARD]), ("after", self.raw[GUARD + self.n:]))
                if not torch.equal(g, self.pat)]


# ---------------------------------------------------------------- templates

def gf_encode(k, m, data):
    """parity (..., m, L) of data (..., k, L): the systematic Cauchy code of
    check_ref.generator, by table lookups."""
    g = R.generator(k, m)
    par = np.zeros(data.shape[:-2] + (m, data.shape[-1]), dtype=np.uint8)
    for i in range(m):
        for j in range(k):
            par[..., i, :] ^= R.MUL[g[k + i, j]][data[..., j, :]]
    return par


def shard_templates(k, m, width, count, seed):
    """(count, k + m, width): random data shards over their parity."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, size=(count, k, width), dtype=np.uint8)
    return np.concatenate([data, gf_encode(k, m, data)], axis=1)


def index_templates(k, m, cols, count, seed, shuffled=True):
    """(count, cols): per template, cols distinct shard indices in a shuffled
    order (or 0..cols-1)."""
    rng = np.random.default_rng(seed ^ 0x1D)
    if not shuffled:
        return np.tile(np.arange(cols, dtype=np.uint8), (count, 1))
    return np.stack([rng.permutation(k + m)[:cols].astype(np.uint8) for _ in range(count)])


def periodic(tmpl, n):
    """rows 0..n-1 of a (T, ...) template cycling: row b is tmpl[b % T]."""
    return tmpl[np.arange(n) % tmpl.shape[0]]


class Code:
    """One geometry with its templates.  shards: (T, k + m, width), T = 7 and
    width = S for a many-block shape, T = 1 and width = period for huge shards."""

    def __init__(self, shape, m=None, seed=1):
        self.k, self.S, self.n = shape["k"], shape["S"], shape["n"]
        self.m = shape.get("m") if m is None else m
        self.tile, self.period, self.bounds = shape["tile"], shape["period"], shape["bounds"]
        self.T = PERIOD if self.period is None else 1
        assert self.period is None or self.n == 1
        self.width = self.S if self.period is None else self.period
        self.seed = seed
        self.shards = shard_templates(self.k, self.m, self.width, self.T, seed)

    def layout(self, rows_t):
        """The layout of a buffer whose block b holds the shards rows_t[b % T]
        (a (T, rows) array of shard indices) back to back."""
        rows = rows_t.shape[1]
        picked = np.stack([self.shards[t][rows_t[t]] for t in range(self.T)])  # (T, rows, width)
        if self.period is None:
            return Layout("blocks", picked.reshape(self.T, rows * self.S), self.n * rows * self.S)
        return Layout("cols", picked[0], rows * self.S, S=self.S)

    def index_layout(self, rows_t):
        return Layout("blocks", rows_t, self.n * rows_t.shape[1])


class MacCase:
    """encode, rebuild, rebuild_uniform or gather: in_idx / out_idx (T, rows)
    name the shards of each template the input and the output hold."""

    def __init__(self, shape, in_idx, out_idx, m=None, seed=1):
        self.code = Code(shape, m, seed)
        self.in_idx, self.out_idx = in_idx, out_idx
        self.inp = self.code.layout(in_idx)
        self.out = self.code.layout(out_idx)


def encode_case(shape, seed=1):
    k, m = shape["k"], shape["m"]
    T = PERIOD if shape["period"] is None else 1
    return MacCase(shape, np.tile(np.arange(k, dtype=np.uint8), (T, 1)),
                   np.tile(np.arange(k, k + m, dtype=np.uint8), (T, 1)), seed=seed)


def rebuild_case(shape, e=2, seed=2, uniform=False):
    """Erasure patterns cycling with the templates: k survivors in a shuffled
    order, e lost shards among the rest."""
    k, m = shape["k"], shape["m"]
    T = PERIOD if shape["period"] is None else 1
    perm = index_templates(k, m, k + e, T, seed)
    if uniform:
        perm = np.tile(perm[:1], (T, 1))
    return MacCase(shape, perm[:, :k].copy(), perm[:, k:].copy(), seed=seed)


# ------------------------------------------------------------ verdict cases

class VerdictCase:
    """verify, check, correct or check_pair over one shape.  bufs: name ->
    (rows per block, position of the buffer's first shard in the block's row
    of k + x, clean layout).  groups: the plants of one call each, as lists of
    (buffer, flat offset, XOR value)."""

    def __init__(self, kind, shape, x, m=None, seed=3, n=None):
        assert kind in ("verify", "check", "correct", "pair")
        shape = dict(shape, n=shape["n"] if n is None else n)
        self.kind, self.x = kind, x
        c = self.code = Code(shape, m, seed)
        self.k, self.m, self.S, self.n = c.k, c.m, c.S, c.n
        kx = self.kx = c.k + x
        if kind == "verify":
            assert x == c.m
            self.idx_t = index_templates(c.k, c.m, kx, c.T, seed, shuffled=False)
            self.bufs = {"data": (c.k, 0, c.layout(self.idx_t[:, :c.k])),
                         "parity": (c.m, c.k, c.layout(self.idx_t[:, c.k:]))}
        else:
            self.idx_t = index_templates(c.k, c.m, kx, c.T, seed)
            self.bufs = {"have": (kx, 0, c.layout(self.idx_t))}
        self.groups = plant_groups(self)

    # where a flat offset of a buffer lies
    def where(self, buf, off):
        rows, pos0, _ = self.bufs[buf]
        b, r = divmod(off, rows * self.S)
        return b, pos0 + r // self.S, r % self.S

    def block(self, b, cols):
        """Columns `cols` of clean block b, (k + x, len(cols)), in have order."""
        c = self.code
        t = b % c.T
        return c.shards[t][self.idx_t[t]][:, np.asarray(cols) % c.width]

    def reduced_cols(self, positions):
        """The byte columns of the reduced block: the tiles that hold a
        planted byte, and one clean tile (the whole block if it has no
        more than that)."""
        tile, S = self.code.tile, self.S
        tiles = sorted({i // tile for i in positions})
        ntiles = -(-S // tile)
        clean = next((t for t in range(ntiles) if t not in tiles), None)
        if clean is not None:
            tiles = sorted(tiles + [clean])
        return np.concatenate([np.arange(t * tile, min((t + 1) * tile, S)) for t in tiles])

    def judge(self, b, flips, cols=None):
        """(word, flips left in the block afterwards) of block b with the
        flips [(position, byte, xor)], by the numpy reference of this kind over
        the columns `cols` (default: the reduced block)."""
        if cols is None:
            cols = self.reduced_cols([i for _, i, _ in flips])
        at = {int(c): n for n, c in enumerate(cols)}
        blk = self.block(b, cols).copy()
        for q, i, v in flips:
            blk[q, at[i]] ^= v
        row = self.idx_t[b % self.code.T]
        if self.kind == "pair":
            return int(PR.check_pair_block(self.k, self.m, row, blk, self.x)), flips
        if self.kind == "correct":
            words, after = CR.correct_reference(self.k, self.m, row[None], blk[None], x=self.x)
            if not int(words[0]) & CORRECTED:
                assert np.array_equal(after[0], blk)
                return int(words[0]), flips
            # a mended block is the clean one: every plant here is a single wrong shard
            assert np.array_equal(after[0], self.block(b, cols)), "the reference did not restore block %d" % b
            return int(words[0]), []
        return int(R.check_block(self.k, self.m, row, blk, self.x)), flips

    def by_block(self, group):
        out = {}
        for buf, off, v in group:
            b, q, i = self.where(buf, off)
            out.setdefault(b, []).append((q, i, v))
        return out

    def expected(self, group, full=False):
        """(block -> word, buffer -> flips left after the call) of one call."""
        words, left = {}, {name: {} for name in self.bufs}
        for b, flips in self.by_block(group).items():
            w, rest = self.judge(b, flips, np.arange(self.S) if full else None)
            words[b] = w
            for buf, off, v in group:
                bb, q, i = self.where(buf, off)
                if bb == b and (q, i, v) in rest:
                    left[buf][off] = v
        return words, left

    def planted(self, group):
        out = {name: {} for name in self.bufs}
        for buf, off, v in group:
            out[buf][off] = v
        return out


def plant_places(case):
    """The places the issue names, as (label, buffer, flat offset): the first
    block; the byte at 2^31 and at 2^32 of every input buffer that reaches it
    (so the block or shard that straddles it); the first and the last byte of
    the last (partial) tile of the last shard of the last block."""
    S, tile = case.S, case.code.tile
    lo, hi = case.code.bounds
    names = list(case.bufs)
    first, last = names[0], names[-1]
    rows0 = case.bufs[first][0]
    places = [("first", first, (1 % rows0) * S + min(5, S - 1))]
    for name in names:
        total = case.bufs[name][2].total
        places += [(label, name, at) for label, at in (("lo", lo), ("hi", hi)) if at < total]
    total = case.bufs[last][2].total
    part = S % tile or min(tile, S)
    places += [("last", last, total - part), ("last", last, total - 1)]
    return places


def plant_groups(case):
    """The calls of a verdict case.  Many blocks: one call with every plant,
    and one with each plant at or past the upper boundary moved down by it
    into an otherwise clean batch (the high block's word must then be 0).
    One block: a clean call first (at x = 1 every wrong block reads
    mask | 0xFF << 16, whatever was read, so only a word of 0 shows what a
    displaced read does), then one call per place (a second wrong shard would
    only make the block unlocated); moved down, a plant is just another low
    plant of the same block, which "first" already is.  check_pair: every plant has a
    partner in the same block, in the last shard's last tile (in shard 0 when
    the plant itself lies in the last shard)."""
    places = plant_places(case)
    hi = case.code.bounds[1]
    S = case.S

    def with_partner(buf, off, v):
        flips = [(buf, off, v)]
        if case.kind == "pair":
            rows, _, _ = case.bufs[buf]
            b, r = divmod(off, rows * S)
            q = r // S
            partner = b * rows * S + ((rows - 1) * S + S - 3 if q != rows - 1 else min(7, S - 1))
            if partner not in [o for _, o, _ in flips]:
                flips.append((buf, partner, 0x5A))
        return flips

    def merged(parts):
        seen, out = set(), []
        for p in parts:
            for f in p:
                if (f[0], f[1]) not in seen:
                    seen.add((f[0], f[1]))
                    out.append(f)
        return out

    by_label = {}
    for n, (label, buf, off) in enumerate(places):
        by_label.setdefault(label + buf, []).append((buf, off, 0x10 << (n % 3)))
    if case.n == 1 and case.kind == "pair":
        # each call walks the block four times with one workgroup, so the last
        # tile's two bytes get no call of their own: they are the partner
        last = by_label.pop("last" + places[-1][1])
        groups = [[]]
        for (plant,) in by_label.values():
            in_last = case.where(plant[0], plant[1])[1] == case.kx - 1
            groups.append(with_partner(*plant) if in_last else [plant] + last)
        return groups
    if case.n == 1:
        groups = [[]]
        for plants in by_label.values():
            parts = [with_partner(*plants[0])] + [[p] for p in plants[1:]]
            groups.append(merged(parts))
        return groups
    main = merged([with_partner(*p) for plants in by_label.values() for p in plants[:1]] +
                  [[p] for plants in by_label.values() for p in plants[1:]])
    twin = merged([with_partner(buf, off - hi, v) for plants in by_label.values()
                   for buf, off, v in plants[:1] if off >= hi])
    return [main, twin] if twin else [main]


# ------------------------------------------- numpy models of whole calls

def narrow_read(a, bits):
    """What a reader sees whose byte offsets into `a` are cut to `bits` bits."""
    return a[np.arange(a.size, dtype=np.int64) % (1 << bits)]


def narrow_write(res, bits, preset):
    """A buffer preset to `preset` after a writer stored res[o] at o mod 2^bits."""
    out = np.full(res.size, preset, dtype=res.dtype)
    out[np.arange(res.size, dtype=np.int64) % (1 << bits)] = res
    return out


def model_mac(case, inp):
    """The output buffer of a MacCase from the whole input buffer `inp`
    (numpy): every block's output shards from its input shards, by decode rows
    over GF(2^8)."""
    c = case.code
    k, S, n = c.k, c.S, c.n
    ri, ro = case.in_idx.shape[1], case.out_idx.shape[1]
    src = inp.reshape(n, ri, S)
    out = np.zeros((n, ro, S), dtype=np.uint8)
    for t in range(c.T):
        d = R.decode_rows(k, c.m, case.in_idx[t][:k], case.out_idx[t])
        sel = np.arange(t, n, c.T)
        for r in range(ro):
            for j in range(k):
                out[sel, r] ^= R.MUL[d[r, j]][src[sel, j]]
    return out.reshape(-1)


def model_verdict(case, bufs):
    """(words, buffers after the call) of a VerdictCase over whole numpy
    buffers (name -> flat array), the reference of its kind run once per
    distinct block."""
    n, S, kx = case.n, case.S, case.kx
    parts = [bufs[name].reshape(n, rows * S) for name, (rows, _, _) in case.bufs.items()]
    have = np.concatenate(parts, axis=1)
    idx = periodic(case.idx_t, n)
    uniq, inv = np.unique(np.concatenate([idx, have], axis=1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    words = np.zeros(len(uniq), dtype=np.uint32)
    after = uniq[:, kx:].copy()
    for u, rowbytes in enumerate(uniq):
        row, blk = rowbytes[:kx], rowbytes[kx:].reshape(kx, S)
        if case.kind == "pair":
            words[u] = PR.check_pair_block(case.k, case.m, row, blk, case.x)
        elif case.kind == "correct":
            w, a = CR.correct_reference(case.k, case.m, row[None], blk[None], x=case.x)
            words[u], after[u] = w[0], a.reshape(-1)
        else:
            words[u] = R.check_block(case.k, case.m, row, blk, case.x)
    have_after = after[inv]
    out, at = {}, 0
    for name, (rows, _, _) in case.bufs.items():
        out[name] = have_after[:, at:at + rows * S].reshape(-1)
        at += rows * S
    return words[inv], out

"""Every entry point with buffers and shards past 4 GiB (tests/wide_cases.py:
the shapes, the periodic templates and the comparison; tests/test_wide_cases.py:
the proof that these cases reject narrowed offsets).

Each call runs on device memory over a buffer that passes 2^31 and 2^32 bytes
(shape A: 2045 blocks of RS(4,2) with S = 1 MiB + 4160; shape C: 2^25 + 13
blocks with S = 64, 64 to a tile) or over shards of more than 2^31 bytes
(shape B: one block, S = 2^31 + 3 * 4096 + 64).  Its whole output is compared
on the device with the templates the oracle was run on, its inputs with what
was put in, its guards with their pattern; the verdict calls carry planted
wrong bytes in the first block, at 2^31 and 2^32 of every input buffer and in
the last partial tile, and their whole verdict array is held to the numpy
references."""
import gc
import hashlib

import numpy as np
import pytest

import wide_cases as W
from conftest import REBUILD_PATHS, SEED

pytestmark = pytest.mark.gpu

GIB = 1 << 30


def need(gib):
    """Skip only when the device has less free memory than the test needs."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < gib * GIB:
        pytest.skip("needs %d GiB of free device memory, %.1f GiB are free" % (gib, free / GIB))
    assert gib <= 32


@pytest.fixture(autouse=True)
def freed():
    yield
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def dev_fill(lay):
    import torch
    return W.fill(torch.empty(lay.total, dtype=torch.uint8, device="cuda"), lay)


def ready():
    """The buffers are written on torch's stream and the codec runs on its
    own: everything torch has enqueued is done before a call starts."""
    import torch
    torch.cuda.synchronize()


def finish(msgs, *lays):
    for lay in lays:
        lay.drop()
    assert not msgs, "\n".join(msgs)


_CASES = {}


def cached(key, make):
    """A case's templates are made once (the oracle's part) and never written."""
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ------------------------------------------------------ encode and rebuild

@pytest.mark.parametrize("shape", ["A", "C"])
def test_encode(codec, shape):
    """parity passes 2^32 bytes, data 2^33."""
    need(14)
    case = cached(("encode", shape), lambda: W.encode_case(getattr(W, "SHAPE_" + shape)))
    c = case.code
    d = dev_fill(case.inp)
    g = W.Guard(case.out.total, "cuda")
    ready()
    codec.encode(c.k, c.m, d, g.payload, S=c.S, n=c.n)
    codec.synchronize()
    assert case.out.total > 1 << 32 and case.inp.total > 1 << 33
    finish(W.problems("parity", g.payload, case.out) + g.problems("parity") +
           W.problems("data", d, case.inp), case.inp, case.out)


def rebuild_checked(codec, case, uniform=False):
    c = case.code
    e = case.out_idx.shape[1]
    surv = dev_fill(case.inp)
    g = W.Guard(case.out.total, "cuda")
    if uniform:
        ready()
        codec.rebuild_uniform(c.k, c.m, case.in_idx[0], surv, case.out_idx[0], g.payload, S=c.S, n=c.n)
        lays = ()
    else:
        lays = (c.index_layout(case.in_idx), c.index_layout(case.out_idx))
        si, li = dev_fill(lays[0]).view(c.n, c.k), dev_fill(lays[1]).view(c.n, e)
        ready()
        codec.rebuild(c.k, c.m, si, surv, li, g.payload, S=c.S, n=c.n)
    codec.synchronize()
    assert case.out.total > 1 << 32 and case.inp.total > 1 << 33
    msgs = W.problems("out", g.payload, case.out) + g.problems("out") + W.problems("surv", surv, case.inp)
    if not uniform:
        msgs += W.problems("surv_idx", si.view(-1), lays[0]) + W.problems("lost_idx", li.view(-1), lays[1])
    finish(msgs, case.inp, case.out, *lays)


def test_rebuild_many_blocks(codec, rebuild_path):
    """Shape A, e = 2, erasure patterns cycling with the templates, on every
    device rebuild path: surv passes 2^33 bytes, out 2^32."""
    need(14)
    rebuild_checked(codec, cached(("rebuild", "A"), lambda: W.rebuild_case(W.SHAPE_A)))


@pytest.mark.parametrize("path", ["rows", "fused"])
def test_rebuild_tiny_blocks(codec, path):
    """Shape C: 64 blocks to a tile, block and index numbers past 2^25."""
    need(14)
    v, t, cf = REBUILD_PATHS[path]
    with codec.options(rebuild_path=v, image_min_tiles=t, image_min_coefs=cf):
        rebuild_checked(codec, cached(("rebuild", "C"), lambda: W.rebuild_case(W.SHAPE_C)))


def test_rebuild_uniform(codec):
    need(14)
    rebuild_checked(codec, cached(("uniform", "A"), lambda: W.rebuild_case(W.SHAPE_A, uniform=True)), True)


# ------------------------------------------------------------ verdict calls

def pair_n(x):
    """Blocks of RS(4,4) with 4 + x shards: `have` just passes 2^32, and 5 more."""
    return -(-(1 << 32) // ((4 + x) * W.SHAPE_A["S"])) + 5


VERDICT = {
    "verify_A": lambda: W.VerdictCase("verify", W.SHAPE_A, 2),
    "verify_B": lambda: W.VerdictCase("verify", W.SHAPE_B, 2, m=2),
    "verify_C": lambda: W.VerdictCase("verify", W.SHAPE_C, 2),
    "check_A_x1": lambda: W.VerdictCase("check", W.SHAPE_A, 1),
    "check_A_x2": lambda: W.VerdictCase("check", W.SHAPE_A, 2),
    "check_B_x1": lambda: W.VerdictCase("check", W.SHAPE_B, 1, m=1),
    "check_B_x2": lambda: W.VerdictCase("check", W.SHAPE_B, 2, m=2),
    "check_C": lambda: W.VerdictCase("check", W.SHAPE_C, 2),
    "correct_A": lambda: W.VerdictCase("correct", W.SHAPE_A, 2),
    "correct_B": lambda: W.VerdictCase("correct", W.SHAPE_B, 2, m=2),
    "correct_C": lambda: W.VerdictCase("correct", W.SHAPE_C, 2),
    "pair_A_x3": lambda: W.VerdictCase("pair", W.SHAPE_A, 3, m=4, n=pair_n(3)),
    "pair_A_x4": lambda: W.VerdictCase("pair", W.SHAPE_A, 4, m=4, n=pair_n(4)),
    "pair_B_x3": lambda: W.VerdictCase("pair", W.reduced_b(3), 3, m=4),
    "pair_B_x4": lambda: W.VerdictCase("pair", W.reduced_b(4), 4, m=4),
}
# One-block cases: one test per call (a located block is walked by a single
# workgroup).  Their templates are a few KiB, so they are made at collection.
ONE_BLOCK = [(name, g) for name in VERDICT if "_B" in name
             for g in range(len(cached(name, VERDICT[name]).groups))]


def verdict_checked(codec, case, groups):
    """The calls `groups` of a verdict case over one set of device buffers:
    the whole verdict array, every input (for correct: the mended `have`) and
    the guards of what the call writes."""
    import torch
    k, m, x, S, n = case.k, case.m, case.x, case.S, case.n
    lays = {name: lay for name, (_, _, lay) in case.bufs.items()}
    held = {name: (W.Guard(lay.total, "cuda", preset=None) if case.kind == "correct" else None)
            for name, lay in lays.items()}
    bufs = {name: W.fill(held[name].payload, lay) if held[name] else dev_fill(lay) for name, lay in lays.items()}
    idx_lay = case.code.index_layout(case.idx_t)
    idx = dev_fill(idx_lay)
    v = W.Guard(4 * n, "cuda")
    msgs = []
    for group in groups:
        planted = case.planted(group)
        for name, flips in planted.items():
            for o, xor in flips.items():
                bufs[name][o] = lays[name].base(o) ^ xor
        v.payload.fill_(W.FILL)
        ready()
        if case.kind == "verify":
            codec.verify(k, m, bufs["data"], bufs["parity"], verdict=v.words(), S=S, n=n)
        else:
            call = {"check": codec.check, "correct": codec.correct, "pair": codec.check_pair}[case.kind]
            call(k, m, idx.view(n, k + x), bufs["have"], verdict=v.words(), x=x, S=S, n=n)
        codec.synchronize()
        want, left = case.expected(group)
        tag = "%s %s: " % (case.kind, [(b, o) for b, o, _ in group])
        found = W.word_problems("verdict", v.words(), want) + v.problems("verdict")
        for name, lay in lays.items():
            found += W.problems(name, bufs[name], lay.flipped(left[name]))
            if held[name]:
                found += held[name].problems(name)
            for o in planted[name]:
                bufs[name][o] = lay.base(o)
        found += W.problems("have_idx", idx, idx_lay)
        msgs += [tag + f for f in found]
    del bufs, held, idx, v
    torch.cuda.synchronize()
    finish(msgs, idx_lay, *lays.values())


@pytest.mark.parametrize("name", [name for name in VERDICT if "_B" not in name])
def test_verdicts_many_blocks(codec, name):
    """Shapes A and C: every input buffer passes 2^32 bytes (`have` at x = 2:
    12.9 GB); two calls, the second with the high plants moved down by 2^32."""
    need(16)
    case = cached(name, VERDICT[name])
    assert all(lay.total > 1 << 32 for _, _, lay in case.bufs.values())
    verdict_checked(codec, case, case.groups)


@pytest.mark.parametrize("name,g", ONE_BLOCK, ids=["%s_call%d" % c for c in ONE_BLOCK])
def test_verdicts_one_huge_block(codec, name, g):
    """Shape B: every column offset of a shard passes 2^31, shard 2 starts
    past 2^32; call 0 is clean, the others carry one place's plants each.
    check_pair walks a block it names a pair in four times with one workgroup
    (46.6 s at this S), so its shards are cut to the smallest whose last one
    still straddles 2^32 (wide_cases.reduced_b)."""
    need(16)
    case = cached(name, VERDICT[name])
    assert (case.S > 1 << 31 or case.kind == "pair") and all(lay.total > 1 << 32 for _, _, lay in case.bufs.values())
    verdict_checked(codec, case, [case.groups[g]])


# ---------------------------------------------------------- gather and fill

def test_gather_shards(codec):
    """Shape A: data passes 2^33, parity and the gathered shards 2^32; index
    rows cycling with the templates."""
    need(24)
    case = cached(("rebuild", "A"), lambda: W.rebuild_case(W.SHAPE_A))
    enc = cached(("encode", "A"), lambda: W.encode_case(W.SHAPE_A))
    c = case.code
    data_lay = c.layout(enc.in_idx)
    par_lay = c.layout(enc.out_idx)
    idx_lay = c.index_layout(case.in_idx)
    d, p, idx = dev_fill(data_lay), dev_fill(par_lay), dev_fill(idx_lay)
    g = W.Guard(case.inp.total, "cuda")
    ready()
    codec.gather_shards(c.k, c.m, c.S, c.n, d, p, idx.view(c.n, c.k), g.payload)
    codec.synchronize()
    finish(W.problems("out", g.payload, case.inp) + g.problems("out") + W.problems("data", d, data_lay) +
           W.problems("parity", p, par_lay) + W.problems("idx", idx, idx_lay),
           data_lay, par_lay, idx_lay, case.inp)


def test_fill_blocks(codec, O):
    """Shape A's 8.6 GB buffer: the content depends on the block number, so
    seven blocks are compared one by one with the oracle's: the first, those
    that hold byte 2^31, 2^32 and 2^33, their successors' neighbour and the last."""
    need(10)
    k, S, n = W.SHAPE_A["k"], W.SHAPE_A["S"], W.SHAPE_A["n"]
    B, first = k * S - 3, 1 << 33
    g = W.Guard(n * k * S, "cuda")
    ready()
    codec.fill_blocks(SEED, first, n, B, k, S, g.payload)
    codec.synchronize()
    picked = [0, (1 << 31) // (k * S), (1 << 32) // (k * S), (1 << 32) // (k * S) + 1, (1 << 33) // (k * S),
              n - 2, n - 1]
    msgs = g.problems("out")
    out = g.payload.view(n, k * S)
    for b in picked:
        want = O.fill_blocks(SEED, first + b, 1, B, k, S)
        if not np.array_equal(out[b].cpu().numpy(), want[0]):
            msgs.append("block %d differs from the oracle's" % b)
    finish(msgs)


# ------------------------------------------------------------------ SHA-256

def test_sha256(codec):
    """4100 messages at a stride of 1 MiB + 16 (4.3 GB: message 4096 starts
    past 2^32), lengths cycling over 7 values around 1 MiB with every padding
    case, a 64-byte prefix cycling over 3: hashlib on the 21 variants, digest
    rows of all 4100."""
    import torch
    need(6)
    n, stride = 4100, (1 << 20) + 16
    lens = np.array([(1 << 20) - 9, (1 << 20) - 8, (1 << 20) - 1, 1 << 20, stride, (1 << 20) + 7, 1000003], np.int64)
    assert [int(v) % 64 for v in lens[:4]] == [55, 56, 63, 0] and n * stride > 1 << 32
    rng = np.random.default_rng(SEED ^ 0x5A)
    msg_lay = W.Layout("blocks", rng.integers(0, 256, (W.PERIOD, stride), dtype=np.uint8), n * stride)
    pre_lay = W.Layout("blocks", rng.integers(0, 256, (3, 64), dtype=np.uint8), n * 64)
    want = np.stack([np.frombuffer(hashlib.sha256(
        pre_lay.tmpl[i % 3].tobytes() + msg_lay.tmpl[i % 7, :lens[i % 7]].tobytes()).digest(), np.uint8)
        for i in range(21)])
    dig_lay = W.Layout("blocks", want, n * 32)
    msg, pre = dev_fill(msg_lay), dev_fill(pre_lay)
    ml = torch.from_numpy(lens[np.arange(n) % 7]).cuda()
    g = W.Guard(n * 32, "cuda")
    ready()
    codec.sha256(msg.view(n, stride), g.payload.view(n, 32), prefix=pre.view(n, 64), msg_len=ml)
    codec.synchronize()
    finish(W.problems("digest", g.payload, dig_lay) + g.problems("digest") + W.problems("msg", msg, msg_lay) +
           W.problems("prefix", pre, pre_lay), msg_lay, pre_lay, dig_lay)


# ------------------------------------------------------------------- ragged

RAGGED_SIZES = [64, 4096, (2 << 20) + 64, (1 << 20) + 4160, 8320, 640, 12352]


class Ragged:
    """A ragged batch whose sizes cycle through RAGGED_SIZES with k * T past
    2^32: block b is template b % 7 (its own size, data and erasure pattern),
    so seven blocks in a row form one period of k * sum(sizes) bytes."""

    def __init__(self, k=4, m=2, e=2, seed=11):
        self.k, self.m, self.e = k, m, e
        per = sum(RAGGED_SIZES)
        groups = -(-(1 << 32) // (k * per))
        self.sizes = np.array((RAGGED_SIZES * (groups + 1))[:groups * 7 + 3], dtype=np.uint64)
        self.n, self.T = len(self.sizes), int(self.sizes.sum())
        assert k * self.T > 1 << 32 > k * (groups - 1) * per
        self.shards = [W.shard_templates(k, m, S, 1, seed + t)[0] for t, S in enumerate(RAGGED_SIZES)]
        self.perm = W.index_templates(k, m, k + e, 7, seed)
        self.coff = np.concatenate([[0], np.cumsum(RAGGED_SIZES)])

    def layout(self, rows_t):
        """rows_t (7, rows): the shards of each template a buffer holds."""
        row = np.concatenate([self.shards[t][rows_t[t]].reshape(-1) for t in range(7)])
        return W.Layout("blocks", row[None], rows_t.shape[1] * self.T)

    def where(self, rows, off):
        """(block, shard, byte) of flat offset `off` of a buffer of `rows` shards per block."""
        per = rows * int(self.coff[-1])
        g, r = divmod(off, per)
        t = int(np.searchsorted(rows * self.coff, r, side="right")) - 1
        j, i = divmod(r - rows * int(self.coff[t]), RAGGED_SIZES[t])
        return 7 * g + t, j, i


def test_ragged_encode_verify(codec):
    """encode_ragged, then verify_ragged clean and with wrong bytes in the
    first block, at 2^31 and 2^32 of data, at 2^31 of parity and in the last
    byte of both: data passes 2^32 bytes, parity 2^31."""
    need(10)
    rg = cached("ragged", Ragged)
    k, m, n = rg.k, rg.m, rg.n
    ident = np.tile(np.arange(k + m, dtype=np.uint8), (7, 1))
    data_lay, par_lay = rg.layout(ident[:, :k]), rg.layout(ident[:, k:])
    d = dev_fill(data_lay)
    g = W.Guard(par_lay.total, "cuda")
    ready()
    codec.encode_ragged(k, m, rg.sizes, d, g.payload)
    codec.synchronize()
    msgs = W.problems("parity", g.payload, par_lay) + g.problems("parity") + W.problems("data", d, data_lay)
    v = W.Guard(4 * n, "cuda")
    plants = [("data", RAGGED_SIZES[0] + 5, 0x10), ("data", 1 << 31, 0x20), ("data", 1 << 32, 0x40),
              ("data", k * rg.T - 1, 0x10), ("parity", 1 << 31, 0x20), ("parity", m * rg.T - 1, 0x40)]
    bufs, lays = {"data": d, "parity": g.payload}, {"data": data_lay, "parity": par_lay}
    for group in ([], plants):
        blocks, flips = {}, {"data": {}, "parity": {}}
        for name, off, xor in group:
            b, j, i = rg.where(k if name == "data" else m, off)
            blocks.setdefault(b, []).append((j + (0 if name == "data" else k), i, xor))
            bufs[name][off] = lays[name].base(off) ^ xor
            flips[name][off] = xor
        want = {}
        for b, fl in blocks.items():
            blk = rg.shards[b % 7].copy()
            for q, i, xor in fl:
                blk[q, i] ^= xor
            want[b] = int(W.R.check_block(k, m, ident[0], blk, m))
        v.payload.fill_(W.FILL)
        ready()
        codec.verify_ragged(k, m, rg.sizes, d, g.payload, verdict=v.words())
        codec.synchronize()
        assert all(want.values()) and bool(want) == bool(group)
        msgs += W.word_problems("verdict", v.words(), want) + v.problems("verdict")
        msgs += W.problems("data", d, data_lay.flipped(flips["data"]))
        msgs += W.problems("parity", g.payload, par_lay.flipped(flips["parity"])) + g.problems("parity")
    finish(msgs, data_lay, par_lay)


@pytest.mark.parametrize("uniform", [0, 1])
def test_ragged_rebuild(codec, uniform):
    """rebuild_ragged, e = 2, per-block patterns cycling with the templates
    (or one for all): surv passes 2^32 bytes, out 2^31."""
    need(10)
    rg = cached("ragged", Ragged)
    k, m, e, n = rg.k, rg.m, rg.e, rg.n
    perm = np.tile(rg.perm[:1], (7, 1)) if uniform else rg.perm
    surv_lay, out_lay = rg.layout(perm[:, :k]), rg.layout(perm[:, k:])
    surv = dev_fill(surv_lay)
    g = W.Guard(out_lay.total, "cuda")
    if uniform:
        ready()
        codec.rebuild_ragged(k, m, rg.sizes, perm[0, :k], surv, perm[0, k:], g.payload, uniform=True)
    else:
        si = dev_fill(W.Layout("blocks", perm[:, :k], n * k)).view(n, k)
        li = dev_fill(W.Layout("blocks", perm[:, k:], n * e)).view(n, e)
        ready()
        codec.rebuild_ragged(k, m, rg.sizes, si, surv, li, g.payload)
    codec.synchronize()
    finish(W.problems("out", g.payload, out_lay) + g.problems("out") + W.problems("surv", surv, surv_lay),
           surv_lay, out_lay)


def test_ragged_huge_block_between_small_ones(codec):
    """RS(2,2), sizes 64, 2^31 + 4160, 64: encode_ragged and verify_ragged
    (clean, then a wrong byte at 2^32 of data, inside the huge block's second
    shard, which sends verify_locate_ragged_kernel over the whole block)."""
    need(10)
    k = m = 2
    S = (1 << 31) + 4160
    sizes = [64, S, 64]
    code = W.Code(dict(W.SHAPE_B, S=S), m=m, seed=13)
    small = [W.shard_templates(k, m, 64, 1, 14 + t)[0] for t in range(2)]
    ident = np.arange(k + m, dtype=np.uint8)[None]
    huge = {"data": code.layout(ident[:, :k]), "parity": code.layout(ident[:, k:])}
    import torch

    def build(name, rows, lo):
        buf = torch.empty(rows * (S + 128), dtype=torch.uint8, device="cuda")
        buf[:rows * 64] = torch.from_numpy(small[0][lo:lo + rows].reshape(-1)).cuda()
        W.fill(buf[rows * 64:rows * (64 + S)], huge[name])
        buf[rows * (64 + S):] = torch.from_numpy(small[1][lo:lo + rows].reshape(-1)).cuda()
        return buf

    def held(name, buf, rows, lo, flips=None):
        msgs = W.problems(name + " of the huge block", buf[rows * 64:rows * (64 + S)],
                          huge[name].flipped(flips or {}))
        for t, part in ((0, buf[:rows * 64]), (1, buf[rows * (64 + S):])):
            if not np.array_equal(part.cpu().numpy(), small[t][lo:lo + rows].reshape(-1)):
                msgs.append("%s of small block %d differs" % (name, 2 * t))
        return msgs

    d = build("data", k, 0)
    g = W.Guard(m * (S + 128), "cuda")
    ready()
    codec.encode_ragged(k, m, sizes, d, g.payload)
    codec.synchronize()
    msgs = held("parity", g.payload, m, k) + g.problems("parity") + held("data", d, k, 0)
    v = W.Guard(4 * 3, "cuda")
    at = (1 << 32) - k * 64                     # byte 2^32 of data, inside the huge block
    assert S < at < 2 * S
    col = at - S
    for flips in ({}, {at: 0x20}):
        for o, xor in flips.items():
            d[k * 64 + o] = huge["data"].base(o) ^ xor
        want = {}
        if flips:
            blk = code.shards[0][:, [col % code.width, (col + 1) % code.width]].copy()
            blk[1, 0] ^= 0x20
            want = {1: int(W.R.check_block(k, m, ident[0], blk, m))}
            assert want[1] == 0b11 | 1 << 16
        v.payload.fill_(W.FILL)
        ready()
        codec.verify_ragged(k, m, sizes, d, g.payload, verdict=v.words())
        codec.synchronize()
        msgs += W.word_problems("verdict", v.words(), want) + v.problems("verdict")
        msgs += held("data", d, k, 0, flips) + held("parity", g.payload, m, k) + g.problems("parity")
    finish(msgs, *huge.values())


# ----------------------------------------------------------- mixed segments

def test_segments(codec, O):
    """encode_segments and rebuild_segments, one call each: a shape-A segment
    (4.3 GB of parity, 8.6 GB of survivors) followed by three RS(10,4) blocks
    of 4 KiB, whose tiles are numbered behind the first segment's."""
    need(16)
    enc = cached(("encode", "A"), lambda: W.encode_case(W.SHAPE_A))
    reb = cached(("rebuild", "A"), lambda: W.rebuild_case(W.SHAPE_A))
    c = enc.code
    k2, m2, n2, B2 = 10, 4, 3, 4096
    S2 = O.shard_size(B2, k2)
    data2 = O.fill_blocks(SEED, 5, n2, B2, k2, S2)
    par2 = O.encode(k2, m2, S2, data2)
    import torch
    d1 = dev_fill(enc.inp)
    g1 = W.Guard(enc.out.total, "cuda")
    d2 = torch.from_numpy(data2).cuda()
    g2 = W.Guard(n2 * m2 * S2, "cuda")
    ready()
    codec.encode_segments([(c.k, c.m, c.S, c.n, d1, g1.payload), (k2, m2, S2, n2, d2, g2.payload)])
    codec.synchronize()
    msgs = W.problems("seg0.parity", g1.payload, enc.out) + g1.problems("seg0.parity") + g2.problems("seg1.parity")
    msgs += W.problems("seg0.data", d1, enc.inp)
    if not np.array_equal(g2.payload.cpu().numpy(), par2.reshape(-1)):
        msgs.append("seg1.parity differs from the oracle's")
    del d1, g1
    torch.cuda.empty_cache()
    s2, l2 = O.erasures(SEED, 5, n2, k2, m2, 2)
    lays = (reb.code.index_layout(reb.in_idx), reb.code.index_layout(reb.out_idx))
    surv1 = dev_fill(reb.inp)
    o1 = W.Guard(reb.out.total, "cuda")
    o2 = W.Guard(n2 * 2 * S2, "cuda")
    segs = [dict(k=c.k, m=c.m, S=c.S, n=c.n, surv=surv1, out=o1.payload,
                 surv_idx=dev_fill(lays[0]).view(c.n, c.k), lost_idx=dev_fill(lays[1]).view(c.n, 2)),
            dict(k=k2, m=m2, S=S2, n=n2, surv=torch.from_numpy(O.gather(k2, m2, S2, data2, par2, s2)).cuda(),
                 out=o2.payload, surv_idx=torch.from_numpy(s2).cuda(), lost_idx=torch.from_numpy(l2).cuda())]
    ready()
    codec.rebuild_segments(segs)
    codec.synchronize()
    msgs += W.problems("seg0.out", o1.payload, reb.out) + o1.problems("seg0.out") + o2.problems("seg1.out")
    msgs += W.problems("seg0.surv", surv1, reb.inp)
    if not np.array_equal(o2.payload.cpu().numpy(), O.gather(k2, m2, S2, data2, par2, l2).reshape(-1)):
        msgs.append("seg1.out differs from the oracle's")
    finish(msgs, enc.inp, enc.out, reb.inp, reb.out, *lays)


# -------------------------------------------------------------- host memory

def host_n(rows):
    """Blocks of shape A's S so that a buffer of `rows` shards a block just passes 2^32."""
    return -(-(1 << 32) // (rows * W.SHAPE_A["S"]))


def host_buffer(lay, pinned):
    import torch
    t = torch.empty(lay.total, dtype=torch.uint8, pin_memory=pinned)
    W.fill(t, lay)
    return t if pinned else t.numpy()


def as_tensor(a):
    import torch
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(a)


@pytest.mark.parametrize("memory", ["pageable", "pinned"])
def test_host_encode_verify(codec, memory):
    """encode and verify from host buffers through the staging engine at the
    default pipe_bytes: the caller's data buffer just passes 2^32 bytes (the
    last block straddles it); parity and the words are compared on the host,
    slice by slice."""
    pinned = memory == "pinned"
    case = cached("host_verify", lambda: W.VerdictCase("verify", W.SHAPE_A, 2, n=host_n(4), seed=5))
    k, m, S, n = case.k, case.m, case.S, case.n
    lays = {name: lay for name, (_, _, lay) in case.bufs.items()}
    assert lays["data"].total > 1 << 32 > lays["data"].total - k * S
    data = host_buffer(lays["data"], pinned)
    import torch
    parity = torch.full((lays["parity"].total,), W.FILL, dtype=torch.uint8, pin_memory=pinned)
    parity = parity if pinned else parity.numpy()
    codec.encode(k, m, data, parity, S=S, n=n)
    msgs = W.problems("parity", as_tensor(parity), lays["parity"]) + W.problems("data", as_tensor(data), lays["data"])
    bufs = {"data": data, "parity": parity}
    words = torch.empty(n, dtype=torch.int32, pin_memory=True) if pinned else np.empty(n, np.uint32)
    for group in case.groups[:1] if pinned else case.groups:
        planted = case.planted(group)
        for name, flips in planted.items():
            for o, xor in flips.items():
                bufs[name][o] = lays[name].base(o) ^ xor
        words[:] = 0x25A5A5A5
        codec.verify(k, m, data, parity, verdict=words, S=S, n=n)
        want, left = case.expected(group)
        msgs += W.word_problems("verdict", words, want)
        for name, lay in lays.items():
            msgs += W.problems(name, as_tensor(bufs[name]), lay.flipped(left[name]))
            for o in planted[name]:
                bufs[name][o] = lay.base(o)
    finish(msgs, *lays.values())


def test_host_check(codec):
    """check from pageable host buffers: `have` (k + 2 shards a block) just
    passes 2^32 bytes; every plant, then the high plants moved down by 2^32."""
    case = cached("host_check", lambda: W.VerdictCase("check", W.SHAPE_A, 2, n=host_n(6), seed=6))
    k, m, x, S, n = case.k, case.m, case.x, case.S, case.n
    lay = case.bufs["have"][2]
    assert lay.total > 1 << 32 > lay.total - (k + x) * S
    have = host_buffer(lay, False)
    idx = W.periodic(case.idx_t, n).copy()
    words = np.empty(n, np.uint32)
    msgs = []
    for group in case.groups:
        planted = case.planted(group)["have"]
        for o, xor in planted.items():
            have[o] = lay.base(o) ^ xor
        words[:] = W.WORD_FILL
        codec.check(k, m, idx, have, verdict=words, x=x, S=S, n=n)
        want, left = case.expected(group)
        msgs += W.word_problems("verdict", words, want) + W.problems("have", as_tensor(have), lay.flipped(left["have"]))
        for o in planted:
            have[o] = lay.base(o)
    assert np.array_equal(idx, W.periodic(case.idx_t, n))
    finish(msgs, lay)

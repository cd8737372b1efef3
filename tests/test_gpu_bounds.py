"""Guard bands and tile edges of every kernel entry point.

Every buffer of every call below sits between two 8 KiB guards
(tests/guarded.py): after the call the guards must hold their pattern, the
inputs what was put in, and the outputs (preset to 0xA5) the CPU oracle's
bytes.  A store past a buffer's end, which in a plain torch tensor lands in
the caching allocator's slack or a neighbour, fails here.

Shapes: C = S / 16 columns, a tile is 256 columns.
  S = 64    C = 4    64 blocks per flat tile
  S = 192   C = 12   256 % 12 != 0: flat tiles cut blocks mid-way
  S = 4032  C = 252  one partial tile per block, four lanes clamped
  S = 4096  C = 256  exactly one tile per block
  S = 4160  C = 260  a second tile of 4 columns / a flat tile across two blocks
  S = 8256  C = 516  two whole tiles plus 4 columns
with n in {1, 2, 3} and one n with n * C % 256 != 0 (67 for S = 64, else 5);
one code per straight-line shard chunk and row bound of the MAC (CODES; the
three largest at S in {64, 4160}).  A test loops over the shapes of one code
and reports every failing shape, not the first.

The pointer contract (include/memo_ec.h, "Alignment") is pinned down at the
end: misaligned device and pinned shard pointers and misaligned verdict
arrays are refused with MEMO_EC_EINVAL before anything is enqueued -- no test
lets one reach a kernel -- while pageable buffers work at any byte address.
decode_rows is the one device call that documents byte alignment for its
output; it is run at rows offsets 0..3."""
import functools
import hashlib

import numpy as np
import pytest

from conftest import REBUILD_PATHS, SEED
from guarded import FILL, Guarded
from test_gpu_parity import DECODE_KERNELS
from test_gpu_verify import expected as verdict_by_definition

pytestmark = pytest.mark.gpu

CODES = [(2, 1), (3, 2), (4, 2), (10, 4), (12, 4), (14, 2), (16, 4), (5, 3), (6, 3), (6, 6), (7, 5),
         (16, 16), (20, 8), (33, 12), (64, 16)]
LARGEST = {(20, 8), (33, 12), (64, 16)}
CODE_IDS = ["rs%d_%d" % c for c in CODES]
SIZES = [64, 192, 4032, 4096, 4160, 8256]
MIN_PIPE = 1 << 20
EINVAL = -1


def blocks_of(S):
    return [1, 2, 3, 67 if S == 64 else 5]


def shapes(k, m):
    """(S, n) of a code, in the module docstring's order."""
    sizes = [64, 4160] if (k, m) in LARGEST else SIZES
    out = [(S, n) for S in sizes for n in blocks_of(S)]
    for S, n in out:
        assert n <= 3 or S == 4096 or (n * (S // 16)) % 256 != 0  # (C = 256: every n is whole tiles)
    return out


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def ref(k, m, S, nmax):
    """(data nmax x k*S, parity nmax x m*S) by the oracle, computed once and
    read only; blocks are independent, so a case of n blocks takes [:n]."""
    from oracle import oracle as O
    data = O.fill_blocks(SEED, 1000 * k + S, nmax, k * S, k, S)
    return frozen(data, O.encode(k, m, S, data, threads=4))


def ref_for(k, m, S):
    return ref(k, m, S, max(blocks_of(S)))


@functools.lru_cache(maxsize=None)
def patterns(k, m, e, nmax):
    """Per-block patterns (survivors in random order; block 0 and every
    third block lose the last parity shard first) and one shared pattern
    whose first lost shard is a parity shard."""
    rng = np.random.default_rng(SEED ^ (k * 4099 + m * 131 + e))
    s = np.zeros((nmax, k), np.uint8)
    l = np.zeros((nmax, e), np.uint8)
    for b in range(nmax + 1):
        perm = rng.permutation(k + m)
        if b % 3 == 0 or b == nmax:
            at = int(np.flatnonzero(perm == k + m - 1)[0])
            perm[at], perm[k] = perm[k], perm[at]  # the last parity shard: lost, and first
        else:
            perm[k:] = rng.permutation(perm[k:])
        if b < nmax:
            s[b], l[b] = perm[:k], perm[k:k + e]
        else:
            su, lu = perm[:k].astype(np.uint8), perm[k:k + e].astype(np.uint8)
    assert (l[:, 0] >= k).any() and lu[0] == k + m - 1
    return frozen(s, l, su, lu)


@functools.lru_cache(maxsize=None)
def rebuild_ref(k, m, S, e, nmax, uniform=False):
    """(surv_idx, lost_idx, survivors, the lost shards) of nmax blocks."""
    from oracle import oracle as O
    data, par = ref(k, m, S, nmax)
    s, l, su, lu = patterns(k, m, e, nmax)
    if uniform:
        s, l = np.tile(su, (nmax, 1)), np.tile(lu, (nmax, 1))
    return frozen(s, l, O.gather(k, m, S, data, par, s), O.gather(k, m, S, data, par, l))


class Cases:
    """Runs the cases of one test and fails at the end with all that failed."""

    def __init__(self):
        self.failed = []

    def check(self, label, g, **want):
        from memo_amd import ec
        # every buffer is in the memory it was asked for, as the binding reads
        # it: a pinned view taken for pageable would quietly be bounce-copied
        kind = {"device": ec.DEVICE, "pinned": ec.HOST_PINNED, "pageable": ec.HOST}
        for b in g.bufs.values():
            assert ec._ptr(b.view())[1] == kind[b.memory], (label, b.name)
        try:
            g.check(**want)
        except AssertionError as exc:
            self.failed.append("%s:\n%s" % (label, exc))

    def done(self):
        assert not self.failed, "%d case(s) failed\n%s" % (len(self.failed), "\n".join(self.failed[:24]))


def sync(codec, memory):
    if memory == "device":
        codec.synchronize()


def idx_memory(memory):
    """Index arrays live where the shards do on the device; every host call
    takes them pageable."""
    return "device" if memory == "device" else "pageable"


# ------------------------------------------------------------------ the calls
def run_encode(codec, cases, label, k, m, S, n, data, par, memory="device", shift=0):
    g = Guarded(memory)
    d = g.input("data", data[:n], shift=shift)
    p = g.output("parity", (n, m * S), shift=shift)
    codec.encode(k, m, d, p)
    sync(codec, memory)
    cases.check(label, g, parity=par[:n])


def run_rebuild(codec, cases, label, k, m, S, n, r, memory="device", shift=0, uniform=False):
    s, l, surv, want = r
    e = l.shape[1]
    g = Guarded(memory)
    sv = g.input("surv", surv[:n], shift=shift)
    out = g.output("out", (n, e * S), shift=shift)
    if uniform:
        codec.rebuild_uniform(k, m, s[0], sv, l[0], out)
    else:
        si = g.input("surv_idx", s[:n], memory=idx_memory(memory), shift=shift and 1)
        li = g.input("lost_idx", l[:n], memory=idx_memory(memory), shift=shift and 1)
        codec.rebuild(k, m, si, sv, li, out)
    sync(codec, memory)
    cases.check(label, g, out=want[:n])


def run_verify(codec, cases, label, k, m, S, n, data, par, want, memory="device", shift=0):
    g = Guarded(memory)
    d = g.input("data", data, shift=shift)
    p = g.input("parity", par, shift=shift)
    g.output("verdict", 4 * n)  # 0xA5A5A5A5 words
    codec.verify(k, m, d, p, g.words("verdict"), S=S, n=n)
    sync(codec, memory)  # a mismatch is a result, not an error
    cases.check(label, g, verdict=want)


# (k, m, S, n, e, uniform): three codes at different S, one of them with a
# shared pattern, and a fourth segment with nothing lost
SEGMENT_MIX = [(10, 4, 4160, 5, 4, False), (5, 3, 192, 5, 3, True), (3, 2, 64, 67, 2, False),
               (16, 4, 4032, 3, 0, False)]


def run_rebuild_segments(codec, cases, label, mix, memory="device", shift=0, nmax=None):
    g = Guarded(memory)
    segs, want = [], {}
    for i, (k, m, S, n, e, uni) in enumerate(mix):
        name = "seg%d_rs%d_%d" % (i, k, m)
        top = nmax or max(blocks_of(S))
        if e == 0:
            # nothing to rebuild: the segment's out is not written at all
            data, _ = ref(k, m, S, top)
            s, l = patterns(k, m, 1, top)[:2]
            lost = g.input(name + ".lost_idx", l[:n], memory=idx_memory(memory))
            segs.append(dict(k=k, m=m, surv=g.input(name + ".surv", data[:n], shift=shift),
                             surv_idx=g.input(name + ".surv_idx", s[:n], memory=idx_memory(memory)),
                             lost_idx=lost[:, :0],  # n x 0
                             out=g.output(name + ".out", 64, shift=shift), S=S, n=n))
            continue
        s, l, surv, w = rebuild_ref(k, m, S, e, top, uni)
        seg = dict(k=k, m=m, surv=g.input(name + ".surv", surv[:n], shift=shift),
                   out=g.output(name + ".out", (n, e * S), shift=shift))
        if uni:
            seg.update(surv_idx=s[0], lost_idx=l[0], uniform=True)
        else:
            seg.update(surv_idx=g.input(name + ".surv_idx", s[:n], memory=idx_memory(memory)),
                       lost_idx=g.input(name + ".lost_idx", l[:n], memory=idx_memory(memory)))
        segs.append(seg)
        want[name + ".out"] = w[:n]
    codec.rebuild_segments(segs)
    sync(codec, memory)
    cases.check(label, g, **want)


def run_encode_segments(codec, cases, label, mix):
    g = Guarded("device")
    segs, want = [], {}
    for i, (k, m, S, n, _, _) in enumerate(mix):
        name = "seg%d_rs%d_%d" % (i, k, m)
        data, par = ref_for(k, m, S)
        segs.append((k, m, S, n, g.input(name + ".data", data[:n]), g.output(name + ".parity", (n, m * S))))
        want[name + ".parity"] = par[:n]
    codec.encode_segments(segs)
    codec.synchronize()
    cases.check(label, g, **want)


# ------------------------------------------------ device entry points, by code
@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_encode_device(codec, O, k, m):
    cases = Cases()
    for S, n in shapes(k, m):
        data, par = ref_for(k, m, S)
        run_encode(codec, cases, "encode S=%d n=%d" % (S, n), k, m, S, n, data, par)
    cases.done()


@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_rebuild_device(codec, O, rebuild_path, k, m):
    cases = Cases()
    for S, n in shapes(k, m):
        for e in sorted({1, m}):
            r = rebuild_ref(k, m, S, e, max(blocks_of(S)))
            run_rebuild(codec, cases, "rebuild[%s] S=%d n=%d e=%d" % (rebuild_path, S, n, e), k, m, S, n, r)
    cases.done()


@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_rebuild_uniform_device(codec, O, k, m):
    cases = Cases()
    for S, n in shapes(k, m):
        for e in sorted({1, m}):
            r = rebuild_ref(k, m, S, e, max(blocks_of(S)), True)
            run_rebuild(codec, cases, "uniform S=%d n=%d e=%d" % (S, n, e), k, m, S, n, r, uniform=True)
    cases.done()


@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_verify_device(codec, O, k, m):
    """A clean batch reads all zero (the words were 0xA5A5A5A5); a batch
    whose only corruption is its very last parity byte flags its last block,
    by the definition test_gpu_verify.expected restates; data and parity
    come back unchanged."""
    cases = Cases()
    for S, n in shapes(k, m):
        data, par = ref_for(k, m, S)
        data, par = data[:n], par[:n]
        run_verify(codec, cases, "verify clean S=%d n=%d" % (S, n), k, m, S, n, data, par,
                   np.zeros(n, np.uint32))
        bad = par.copy()
        bad[n - 1, m * S - 1] ^= 0x80
        want = verdict_by_definition(O, k, m, S, data.reshape(n, k, S), bad.reshape(n, m, S), {n - 1})
        assert want[n - 1] != 0 and not want[:n - 1].any()
        run_verify(codec, cases, "verify last byte S=%d n=%d" % (S, n), k, m, S, n, data, bad, want)
    cases.done()


@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_stream_probe_copy(codec, O, k, m):
    """COPY mode: out shard i of block b = XOR of the block's k input
    shards, every byte XOR i (include/memo_ec.h)."""
    cases = Cases()
    for S, n in shapes(k, m):
        data, _ = ref_for(k, m, S)
        acc = np.bitwise_xor.reduce(data[:n].reshape(n, k, S), axis=1)
        want = np.stack([acc ^ np.uint8(i) for i in range(m)], axis=1)
        g = Guarded("device")
        codec.stream_probe(k, m, g.input("in", data[:n]), g.output("out", (n, m * S)))
        codec.synchronize()
        cases.check("probe S=%d n=%d" % (S, n), g, out=want)
    cases.done()


@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_fill_blocks(codec, O, k, m):
    """Blocks of B bytes in k * S: the zero padding up to k * S is inside
    the payload, and nothing beyond it is written."""
    cases = Cases()
    for S, n in shapes(k, m):
        for B in (0, 1, k * S - 1, k * S):
            g = Guarded("device")
            codec.fill_blocks(SEED, 5, n, B, k, S, g.output("out", (n, k * S)))
            codec.synchronize()
            want = O.fill_blocks(SEED, 5, n, B, k, S)
            assert not want[:, B:].any() and (B < 64 or want[:, :B].any())
            cases.check("fill S=%d n=%d B=%d" % (S, n, B), g, out=want)
    cases.done()


@pytest.mark.parametrize("k,m", CODES, ids=CODE_IDS)
def test_gather_shards(codec, O, k, m):
    cases = Cases()
    rng = np.random.default_rng(k * 100 + m)
    for S, n in shapes(k, m):
        data, par = ref_for(k, m, S)
        for cnt in sorted({1, k}):
            idx = rng.integers(0, k + m, (n, cnt)).astype(np.uint8)
            idx[n - 1, cnt - 1] = k + m - 1  # the last slot takes the last parity shard
            g = Guarded("device")
            codec.gather_shards(k, m, S, n, g.input("data", data[:n]), g.input("parity", par[:n]),
                                g.input("idx", idx), g.output("out", (n, cnt * S)))
            codec.synchronize()
            cases.check("gather S=%d n=%d cnt=%d" % (S, n, cnt), g,
                        out=O.gather(k, m, S, data[:n], par[:n], idx))
    cases.done()


def test_rebuild_segments_mix(codec, O, rebuild_path):
    cases = Cases()
    run_rebuild_segments(codec, cases, "rebuild_segments[%s]" % rebuild_path, SEGMENT_MIX)
    cases.done()


def test_encode_segments_mix(codec, O):
    cases = Cases()
    run_encode_segments(codec, cases, "encode_segments", SEGMENT_MIX)
    cases.done()


# ------------------------------------------------------------- decode rows
@functools.lru_cache(maxsize=None)
def decode_ref(k, m, e, nmax=700):
    from oracle import oracle as O
    s, l = patterns(k, m, e, nmax)[:2]
    rows = np.stack([O.decode_matrix(k, m, s[b], l[b]) for b in range(nmax)])  # every block
    return frozen(s, l, rows.reshape(nmax, e * k))


@pytest.mark.parametrize("kernel", list(DECODE_KERNELS))
@pytest.mark.parametrize("k,m,e", [(16, 4, 4), (5, 3, 3)], ids=["rs16_4_e4", "rs5_3_e3"])
def test_decode_rows_at_every_byte_offset(codec, O, k, m, e, kernel):
    """The rows pointer 0..3 bytes into its payload: offsets 1..3 take the
    kernels' byte stores (they branch on rows & 3), with e * k a multiple of
    4 (every block's rows then share the pointer's misalignment) and not."""
    assert (e * k % 4 == 0) == (k == 16)
    s, l, rows = decode_ref(k, m, e)
    cases = Cases()
    with codec.options(**DECODE_KERNELS[kernel]):
        for n in (1, 255, 256, 257, 700):
            for off in range(4):
                g = Guarded("device")
                buf = g.output("rows", n * e * k + 4)
                codec.decode_rows(k, m, g.input("surv_idx", s[:n]), g.input("lost_idx", l[:n]),
                                  buf[off:off + n * e * k])
                codec.synchronize()
                want = np.full(n * e * k + 4, FILL, np.uint8)
                want[off:off + n * e * k] = rows[:n].reshape(-1)
                cases.check("decode_rows[%s] n=%d offset=%d" % (kernel, n, off), g, rows=want)
    cases.done()


# ------------------------------------------------------------------ SHA-256
@pytest.mark.parametrize("n", [1, 255, 257])
def test_sha256_digest_guarded(codec, n):
    """Messages of 0, 55, 56 and 64 bytes (no padding block, the last length
    that fits one, the first that needs two, a whole chunk) in rows of 64;
    with and without a 7-byte prefix (prefixes and messages may sit at any
    byte address)."""
    rng = np.random.default_rng(n)
    msg = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    lens = np.array([(0, 55, 56, 64)[i % 4] for i in range(n)], np.int64)
    pre = rng.integers(0, 256, (n, 7), dtype=np.uint8)
    cases = Cases()
    for with_prefix in (False, True):
        import torch
        g = Guarded("device")
        ml = g.input("msg_len", lens).view(torch.int64)
        codec.sha256(g.input("msg", msg), g.output("digest", (n, 32)), msg_len=ml,
                     prefix=g.input("prefix", pre) if with_prefix else None)
        codec.synchronize()
        want = np.stack([np.frombuffer(hashlib.sha256(
            (pre[i].tobytes() if with_prefix else b"") + msg[i, :lens[i]].tobytes()).digest(), np.uint8)
            for i in range(n)])
        cases.check("sha256 n=%d prefix=%s" % (n, with_prefix), g, digest=want)
    cases.done()


# ------------------------------------------------------------ host memory
HOST_CODES = [(10, 4), (5, 3)]
HOST_SIZES = [64, 4160]
# three pipeline waves at the smallest batch, the last of one block; and the
# defaults, where calls of these sizes run zero-copy in one shot
HOST_SETTINGS = {"pipeline": dict(zero_copy_bytes=0, pipe_bytes=MIN_PIPE), "one_shot": {}}


def three_waves(per_block):
    """The smallest n whose blocks of per_block bytes take three waves of
    MIN_PIPE bytes: two full ones and one block."""
    nb = MIN_PIPE // per_block
    assert nb > 1
    return 2 * nb + 1


@pytest.mark.parametrize("setting", list(HOST_SETTINGS))
@pytest.mark.parametrize("memory", ["pinned", "pageable"])
@pytest.mark.parametrize("k,m", HOST_CODES, ids=["rs10_4", "rs5_3"])
def test_host_memory_calls(codec, O, k, m, memory, setting):
    """encode, rebuild, rebuild_segments and verify from host memory.  On
    the pinned path the kernels or the DMA write straight into the caller's
    payload, on the pageable path the bounce copies do."""
    cases = Cases()
    for S in HOST_SIZES:
        n = three_waves(k * S)            # encode, rebuild: a wave holds pipe_bytes / (k * S) blocks
        nv = three_waves((k + m) * S)     # verify: pipe_bytes / ((k + m) * S)
        if setting == "one_shot":
            assert n * ((k + m) * S + k + m) + 64 <= codec.get_option("zero_copy_bytes")
        data, par = ref(k, m, S, n)
        r = rebuild_ref(k, m, S, m, n)
        ru = rebuild_ref(k, m, S, 1, n, True)
        tag = "%s %s S=%d" % (memory, setting, S)
        with codec.options(**HOST_SETTINGS[setting]):
            run_encode(codec, cases, "encode %s n=%d" % (tag, n), k, m, S, n, data, par, memory)
            run_rebuild(codec, cases, "rebuild %s n=%d" % (tag, n), k, m, S, n, r, memory)
            run_rebuild(codec, cases, "uniform %s n=%d" % (tag, n), k, m, S, n, ru, memory, uniform=True)
            run_rebuild_segments(codec, cases, "rebuild_segments %s" % tag,
                                 [(k, m, S, n, m, False), (k, m, S, 3, 1, True), (k, m, S, 2, 0, False)],
                                 memory, nmax=n)
            bad = par[:nv].copy()
            bad[nv - 1, m * S - 1] ^= 0x01
            want = verdict_by_definition(O, k, m, S, data[:nv].reshape(nv, k, S), bad.reshape(nv, m, S),
                                         {nv - 1})
            run_verify(codec, cases, "verify clean %s n=%d" % (tag, nv), k, m, S, nv, data[:nv], par[:nv],
                       np.zeros(nv, np.uint32), memory)
            run_verify(codec, cases, "verify last byte %s n=%d" % (tag, nv), k, m, S, nv, data[:nv], bad,
                       want, memory)
    cases.done()


# -------------------------------------------------------------- tile order
def rows_paths():
    """The two-kernel rebuild as the defaults choose its tables and with
    tables always built in LDS (conftest.REBUILD_PATHS)."""
    for name in ("rows", "lds"):
        v, t, cf = REBUILD_PATHS[name]
        yield name, dict(rebuild_path=v, image_min_tiles=t, image_min_coefs=cf)


def test_tile_order_every_tile_count(codec, O):
    """The XCD-contiguous order on small grids: RS(10,4) at S = 4096 is one
    tile per block, so n = 1..24 gives every tile count up to 24 -- every
    remainder mod 8, and counts below 8, where a tile's XCD share is 0."""
    k, m, S, e = 10, 4, 4096, 4
    data, par = ref(k, m, S, 24)
    r = rebuild_ref(k, m, S, e, 24)
    cases = Cases()
    with codec.options(xcd_min_tiles=1):
        for n in range(1, 25):
            run_encode(codec, cases, "xcd encode n=%d" % n, k, m, S, n, data, par)
            for name, opts in rows_paths():
                with codec.options(**opts):
                    run_rebuild(codec, cases, "xcd rebuild[%s] n=%d" % (name, n), k, m, S, n, r)
    cases.done()


def test_tile_order_flat_tiles(codec, O):
    """RS(3,2) at S = 64 (64 blocks per tile), n = 64 t + 3: 1..10 tiles,
    the last one of three blocks."""
    k, m, S, e = 3, 2, 64, 2
    top = 64 * 9 + 3
    data, par = ref(k, m, S, top)
    r = rebuild_ref(k, m, S, e, top)
    cases = Cases()
    with codec.options(xcd_min_tiles=1):
        for t in range(10):
            n = 64 * t + 3
            run_encode(codec, cases, "xcd encode n=%d" % n, k, m, S, n, data, par)
            for name, opts in rows_paths():
                with codec.options(**opts):
                    run_rebuild(codec, cases, "xcd rebuild[%s] n=%d" % (name, n), k, m, S, n, r)
    cases.done()


def test_tile_order_segment_mixes(codec, O, rebuild_path):
    """Several segments in one launch, each remapped over its own tiles."""
    cases = Cases()
    with codec.options(xcd_min_tiles=1):
        run_rebuild_segments(codec, cases, "xcd rebuild_segments[%s]" % rebuild_path, SEGMENT_MIX)
        run_encode_segments(codec, cases, "xcd encode_segments", SEGMENT_MIX)
    cases.done()


# --------------------------------------------------------- launch splitting
@pytest.mark.parametrize("tiles", [2, 3, 7])
@pytest.mark.parametrize("k,m", [(10, 4), (16, 4)], ids=["rs10_4", "rs16_4"])
def test_split_launches(codec, O, k, m, tiles):
    """max_launch_tiles = 2, 3: every launch is one block (S = 64 counts 2
    tiles per block, S = 4160 counts 3); 7: spans of 3 and 2 blocks, so
    n = 5 ends on a shorter span.  Each span's pointers start at its first
    block."""
    n = 5
    cases = Cases()
    for S in (64, 4160):
        per = (S // 16 + 255) // 256 + 1  # max_blocks_per_launch (memo_ec.cpp)
        assert max(1, tiles // per) == {2: 1, 3: 1, 7: 3 if S == 64 else 2}[tiles]
        data, par = ref_for(k, m, S)
        with codec.options(max_launch_tiles=tiles):
            run_encode(codec, cases, "split encode S=%d" % S, k, m, S, n, data, par)
            for e in (1, m):
                ru = rebuild_ref(k, m, S, e, max(blocks_of(S)), True)
                run_rebuild(codec, cases, "split uniform S=%d e=%d" % (S, e), k, m, S, n, ru, uniform=True)
                r = rebuild_ref(k, m, S, e, max(blocks_of(S)))
                for name, (v, t, cf) in REBUILD_PATHS.items():
                    with codec.options(rebuild_path=v, image_min_tiles=t, image_min_coefs=cf):
                        run_rebuild(codec, cases, "split rebuild[%s] S=%d e=%d" % (name, S, e), k, m, S, n, r)
    cases.done()


# ------------------------------------------------- the pointer contract
K, M, S0, N0 = 10, 4, 4160, 3
SPARE = 16  # room behind each payload, so a refused call's range lies inside it


def contract_buffers(memory):
    """Guarded buffers of one RS(10,4) x 4160 x 3 call of every kind, each
    with SPARE bytes behind it, and their addresses."""
    import torch
    data, par = ref_for(K, M, S0)
    s, l, surv, _ = rebuild_ref(K, M, S0, M, max(blocks_of(S0)))
    g = Guarded(memory)
    pad = np.zeros(SPARE, np.uint8)
    bufs = {"data": g.input("data", np.concatenate([data[:N0].reshape(-1), pad])),
            "parity": g.input("parity", np.concatenate([par[:N0].reshape(-1), pad])),
            "surv": g.input("surv", np.concatenate([surv[:N0].reshape(-1), pad])),
            "surv_idx": g.input("surv_idx", s[:N0], memory=idx_memory(memory)),
            "lost_idx": g.input("lost_idx", l[:N0], memory=idx_memory(memory)),
            "out": g.output("out", N0 * K * S0 + SPARE),  # large enough for a fill / gather of k shards
            "verdict": g.output("verdict", 4 * N0 + SPARE)}
    ptr = {name: (b.data_ptr() if isinstance(b, torch.Tensor) else b.ctypes.data) for name, b in bufs.items()}
    for name in ("data", "parity", "surv", "out", "verdict"):
        assert ptr[name] % 64 == 0
    return g, ptr, (s, l)


def contract_calls(codec, p, where, patt):
    """name -> (pointers that must be aligned, fn(**overrides) -> status) for
    every call that takes `where` memory; fn calls the C ABI directly."""
    from memo_amd import ec
    L, ctx = ec._lib(), codec._ctx
    s, l = patt
    su = np.ascontiguousarray(s[0])
    lu = np.ascontiguousarray(l[0])

    def with_(over):
        q = dict(p)
        q.update(over)
        return q

    def encode(**o):
        q = with_(o)
        return L.memo_ec_encode_batch(ctx, K, M, S0, N0, q["data"], q["parity"], where)

    def verify(**o):
        q = with_(o)
        return L.memo_ec_verify_batch(ctx, K, M, S0, N0, q["data"], q["parity"], q["verdict"], where)

    def rebuild(**o):
        q = with_(o)
        return L.memo_ec_rebuild_batch(ctx, K, M, S0, N0, q["surv_idx"], q["surv"], q["lost_idx"], M, q["out"],
                                       where)

    def uniform(**o):
        q = with_(o)
        return L.memo_ec_rebuild_uniform(ctx, K, M, S0, N0, su.ctypes.data, q["surv"], lu.ctypes.data, M,
                                         q["out"], where)

    def rebuild_segments(**o):
        q = with_(o)
        arr = (ec.RebuildSegment * 2)(
            ec.RebuildSegment(K, M, S0, 1, p["surv_idx"], p["surv"], p["lost_idx"], M, 0, p["out"]),
            ec.RebuildSegment(K, M, S0, 2, q["surv_idx"] + K, q["surv"] + K * S0, q["lost_idx"] + M, M, 0,
                              q["out"] + M * S0))
        return L.memo_ec_rebuild_segments(ctx, 2, arr, where)

    calls = {"encode_batch": (("data", "parity"), encode),
             "verify_batch": (("data", "parity", "verdict"), verify),
             "rebuild_batch": (("surv", "out"), rebuild),
             "rebuild_uniform": (("surv", "out"), uniform),
             "rebuild_segments": (("surv", "out"), rebuild_segments)}
    if where != ec.DEVICE:
        return calls

    def encode_segments(**o):
        q = with_(o)
        arr = (ec.Segment * 2)(ec.Segment(K, M, S0, 1, p["data"], p["parity"]),
                               ec.Segment(K, M, S0, 2, q["data"] + K * S0, q["parity"] + M * S0))
        return L.memo_ec_encode_segments(ctx, 2, arr)

    def probe(**o):
        q = with_(o)
        return L.memo_ec_stream_probe(ctx, K, M, S0, N0, q["data"], q["out"], 0)

    def fill(**o):
        q = with_(o)
        return L.memo_ec_fill_blocks(ctx, SEED, 0, N0, K * S0, K, S0, q["out"])

    def gather(**o):
        q = with_(o)
        return L.memo_ec_gather_shards(ctx, K, M, S0, N0, q["data"], q["parity"], q["surv_idx"], K, q["out"])

    calls.update({"encode_segments": (("data", "parity"), encode_segments),
                  "stream_probe": (("data", "out"), probe),
                  "fill_blocks": (("out",), fill),
                  "gather_shards": (("data", "parity", "out"), gather)})
    return calls


@pytest.mark.parametrize("memory", ["device", "pinned"])
def test_misaligned_shard_pointers_are_refused(codec, O, memory):
    """Every call, with each shard pointer moved by 1 and by 8 bytes (and a
    verdict array by 1 and 2): MEMO_EC_EINVAL before anything is enqueued --
    synchronize reports nothing and every output still holds its preset.
    The aligned calls are not made here: nothing reaches a kernel."""
    from memo_amd import ec
    where = ec.DEVICE if memory == "device" else ec.HOST_PINNED
    g, p, patt = contract_buffers(memory)
    tried = 0
    for name, (pointers, fn) in contract_calls(codec, p, where, patt).items():
        for which in pointers:
            for off in ((1, 2) if which == "verdict" else (1, 8)):
                assert fn(**{which: p[which] + off}) == EINVAL, (name, which, off)
                tried += 1
    assert tried == (38 if memory == "device" else 22)
    codec.synchronize()  # returns 0: nothing was deferred
    g.check()            # inputs intact, both outputs all preset, guards whole


def test_misaligned_verdict_is_refused_in_pageable_memory(codec, O):
    from memo_amd import ec
    g, p, patt = contract_buffers("pageable")
    _, verify = contract_calls(codec, p, ec.HOST, patt)["verify_batch"]
    for off in (1, 2, 3):
        assert verify(verdict=p["verdict"] + off) == EINVAL
    g.check()


def test_sha256_word_pointers_are_refused(codec):
    """The digest is stored in 4-byte words and msg_len read in 8-byte ones:
    a digest off a 4-byte or a msg_len off an 8-byte boundary is refused."""
    from memo_amd import ec
    L, ctx, n = ec._lib(), codec._ctx, 3
    g = Guarded("device")
    msg = g.input("msg", np.zeros((n, 64), np.uint8)).data_ptr()
    lens = g.input("msg_len", np.full(n + 1, 64, np.int64)).data_ptr()
    dig = g.output("digest", n * 32 + SPARE).data_ptr()
    for d, ml in [(dig + 1, lens), (dig + 2, lens), (dig, lens + 1), (dig, lens + 4), (dig + 2, None)]:
        assert L.memo_ec_sha256_batch(ctx, n, None, 0, 0, msg, 64, ml, 64, d) == EINVAL, (d - dig, ml)
    codec.synchronize()
    g.check()


def test_segments_with_nothing_to_do_are_still_skipped(codec, O):
    """A segment with e = 0 (rebuild) or m = 0 (encode) is skipped with its
    pointers unread, as before the contract was enforced; nothing is
    written.  (A misaligned pointer in the second of two live segments is
    refused: contract_calls.)"""
    from memo_amd import ec
    L, ctx = ec._lib(), codec._ctx
    g, p, patt = contract_buffers("device")
    arr = (ec.RebuildSegment * 1)(ec.RebuildSegment(K, M, S0, N0, p["surv_idx"], p["surv"] + 1, p["lost_idx"], 0,
                                                    0, p["out"] + 1))
    assert L.memo_ec_rebuild_segments(ctx, 1, arr, ec.DEVICE) == 0
    enc = (ec.Segment * 1)(ec.Segment(K, 0, S0, N0, p["data"] + 1, p["parity"] + 1))
    assert L.memo_ec_encode_segments(ctx, 1, enc) == 0
    codec.synchronize()
    g.check()


@pytest.mark.parametrize("setting", list(HOST_SETTINGS))
@pytest.mark.parametrize("shift", [1, 17])
def test_pageable_buffers_at_any_byte_address(codec, O, shift, setting):
    """Pageable data, parity, surv and out 1 and 17 bytes past a 64-byte
    boundary (index arrays 1 byte), zero-copy in one shot and through three
    pipeline waves: the library copies them, so they are the oracle's bytes
    and the guards are whole.  The verdict array stays 4-byte aligned."""
    k, m, S = K, M, S0
    n, nv = three_waves(k * S), three_waves((k + m) * S)
    data, par = ref(k, m, S, n)
    r = rebuild_ref(k, m, S, m, n)
    cases = Cases()
    with codec.options(**HOST_SETTINGS[setting]):
        run_encode(codec, cases, "encode shift=%d" % shift, k, m, S, n, data, par, "pageable", shift)
        run_rebuild(codec, cases, "rebuild shift=%d" % shift, k, m, S, n, r, "pageable", shift)
        run_rebuild_segments(codec, cases, "rebuild_segments shift=%d" % shift,
                             [(k, m, S, n, m, False), (k, m, S, 3, 1, True)], "pageable", shift, nmax=n)
        bad = par[:nv].copy()
        bad[nv - 1, m * S - 1] ^= 0x40
        want = verdict_by_definition(O, k, m, S, data[:nv].reshape(nv, k, S), bad.reshape(nv, m, S), {nv - 1})
        run_verify(codec, cases, "verify shift=%d" % shift, k, m, S, nv, data[:nv], bad, want, "pageable",
                   shift)
    cases.done()

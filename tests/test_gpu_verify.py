"""Parity verify on the MI355X (memo_ec_verify_batch: gf_verify_kernel +
verify_locate_kernel) against a numpy restatement of the verdict's definition.

verdict[b] = 0 when the k data and m stored parity shards of block b agree;
otherwise mask (bit i: stored parity i differs from the recomputed one) in
bits 0..15 and, in bits 16..23, the single shard that explains every
mismatch or 0xFF.  With s_i = stored parity i XOR recomputed parity i and
g_ij = 1 / ((k + i) ^ j):
  m == 1                      -> 0xFF
  one row i mismatches        -> k + i
  all m rows mismatch (m >= 2) -> the j < k with s_i[p] * g_0j == g_ij * s_0[p]
                                 at every byte p and row i, else 0xFF
  any other mask              -> 0xFF
`expected` below is that definition over oracle.encode and oracle.gf_mul;
every case also asserts the located shard it built the corruption for, and
that every block it did not touch reads 0 (a tile of the flat mapping spans
several blocks: a mismatch must land in its own block's word).

Where the definition, not the construction, is the judge: with m == 2 two
wrong shards can satisfy the single-shard relation (two syndromes fix one
ratio, and some j may own it), so those cases assert the restated definition
only; with m >= 3 three rows over-determine j and two wrong data shards can
never pass for one (any 3 x 3 Cauchy submatrix is nonsingular).
"""
import numpy as np
import pytest

from conftest import SEED

pytestmark = pytest.mark.gpu

UNLOCATED = 0xFF

# (k, m, S, n)
SHAPES = [
    (3, 2, 64, 130),      # 64 blocks per tile, partial last tile
    (10, 4, 448, 37),     # 4 KiB blocks, tile edges inside blocks
    (16, 4, 4160, 5),     # 260 chunks: a tile across two blocks
    (5, 3, 192, 20),      # chunk loop, k not specialised
    (7, 5, 128, 12),      # R = 6 > m: padded rows must not be compared
    (20, 6, 256, 9),      # chunk loop + R = 6
    (4, 1, 64, 70),       # m = 1: detect only
    (64, 16, 64, 3),      # the limits
    (10, 4, 104896, 2),   # the 1 MiB block
]
IDS = ["rs%d_%d_S%d_n%d" % s for s in SHAPES]

_MUL = None
_CLEAN = {}


def mul_table(O):
    """256 x 256 GF(2^8) products from oracle.gf_mul."""
    global _MUL
    if _MUL is None:
        _MUL = np.array([[O.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)
    return _MUL


def clean(O, shape):
    """(data n x k x S, parity n x m x S) of a shape, computed once and never
    written (cases corrupt copies)."""
    if shape not in _CLEAN:
        k, m, S, n = shape
        rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + S * 31 + n))
        data = rng.integers(0, 256, size=(n, k, S), dtype=np.uint8)
        parity = O.encode(k, m, S, data.reshape(n, k * S)).reshape(n, m, S)
        data.setflags(write=False)
        parity.setflags(write=False)
        _CLEAN[shape] = (data, parity)
    return _CLEAN[shape]


def expected(O, k, m, S, data, parity, touched):
    """The verdict words by the definition; blocks outside `touched` hold the
    clean bytes and read 0."""
    n = data.shape[0]
    MUL = mul_table(O)
    G = O.cauchy(k, m)[k:]  # g_ij, m x k
    out = np.zeros(n, dtype=np.uint32)
    for b in sorted(touched):
        want = O.encode(k, m, S, data[b].reshape(1, k * S)).reshape(m, S)
        syn = want ^ parity[b]
        rows = syn.any(axis=1)
        mask = sum(1 << i for i in range(m) if rows[i])
        if mask == 0:
            continue
        shard = UNLOCATED
        if m >= 2 and bin(mask).count("1") == 1:
            shard = k + int(np.flatnonzero(rows)[0])
        elif m >= 2 and mask == (1 << m) - 1:
            s = syn[:, syn.any(axis=0)]  # consistent bytes constrain nothing
            fits = [j for j in range(k)
                    if all(np.array_equal(MUL[s[i], G[0, j]], MUL[G[i, j], s[0]]) for i in range(m))]
            assert len(fits) <= 1  # g_1j / g_0j is injective in j
            if fits:
                shard = fits[0]
        out[b] = mask | (shard << 16)
    return out


def run_device(codec, k, m, data, parity):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    p = torch.from_numpy(np.ascontiguousarray(parity)).cuda()
    v = codec.verify(k, m, d, p)
    codec.synchronize()  # a mismatch is a result, not an error
    assert v.dtype == torch.int32 and v.numel() == data.shape[0]
    return v.cpu().numpy().view(np.uint32)


def victims(n):
    """The corrupted blocks of a case: every other block, so each has clean
    neighbours on both sides where the batch allows."""
    return list(range(1, n, 2))


def check(O, codec, shape, data, parity, touched, by_construction):
    """Run the device verify and compare: the restated definition for every
    block, (mask, shard) by construction for the corrupted ones, 0 around."""
    from memo_amd import ec
    k, m, S, n = shape
    got = run_device(codec, k, m, data, parity)
    want = expected(O, k, m, S, data, parity, touched)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "blocks %s: got %s want %s" % (
        bad[:8], [hex(x) for x in got[bad[:8]]], [hex(x) for x in want[bad[:8]]])
    assert not (got >> 24).any()
    mask, shard = ec.split_verdict(got)
    for b, (cm, cs) in by_construction.items():
        assert (int(mask[b]), int(shard[b])) == (cm, cs), (b, hex(int(got[b])))
    for b in range(n):
        if b not in touched:
            assert got[b] == 0, (b, hex(int(got[b])))


def copies(O, shape):
    data, parity = clean(O, shape)
    return data.copy(), parity.copy()


def single(k, m, idx):
    """(mask, shard) a single wrong shard idx must give."""
    if idx >= k:
        return 1 << (idx - k), (idx if m >= 2 else UNLOCATED)
    return (1 << m) - 1, (idx if m >= 2 else UNLOCATED)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_clean_is_zero(codec, O, shape):
    data, parity = copies(O, shape)
    check(O, codec, shape, data, parity, set(), {})


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_flipped_bit_locates_every_shard(codec, O, shape):
    """One flipped bit in one shard of each corrupted block; rounds move the
    shard along so every index 0..k+m-1 is hit; the byte cycles through 0,
    S-1 and a seeded interior one."""
    k, m, S, n = shape
    vs = victims(n)
    rng = np.random.default_rng(SEED + 1)
    rounds = -(-(k + m) // len(vs))
    hit = set()
    for t in range(rounds):
        data, parity = copies(O, shape)
        want = {}
        for c, b in enumerate(vs):
            idx = (t * len(vs) + c) % (k + m)
            pos = [0, S - 1, int(rng.integers(1, S - 1))][(t + c) % 3]
            bit = 1 << int(rng.integers(0, 8))
            if idx < k:
                data[b, idx, pos] ^= bit
            else:
                parity[b, idx - k, pos] ^= bit
            want[b] = single(k, m, idx)
            hit.add(idx)
        check(O, codec, shape, data, parity, set(vs), want)
    assert hit == set(range(k + m))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_whole_data_shard_replaced(codec, O, shape):
    k, m, S, n = shape
    rng = np.random.default_rng(SEED + 2)
    data, parity = copies(O, shape)
    want = {}
    for b in victims(n):
        j = int(rng.integers(0, k))
        data[b, j] = rng.integers(0, 256, size=S, dtype=np.uint8)
        want[b] = single(k, m, j)
    check(O, codec, shape, data, parity, set(want), want)


def two_shards(rng, k):
    j1 = int(rng.integers(0, k))
    j2 = (j1 + 1 + int(rng.integers(0, k - 1))) % k
    return j1, j2


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_data_shards_same_byte(codec, O, shape):
    """Unlocated by construction for m >= 3 (and m == 1); for m == 2 the
    restated definition decides (see the module docstring)."""
    k, m, S, n = shape
    rng = np.random.default_rng(SEED + 3)
    data, parity = copies(O, shape)
    want = {}
    for b in victims(n):
        j1, j2 = two_shards(rng, k)
        pos = int(rng.integers(0, S))
        data[b, j1, pos] ^= int(rng.integers(1, 256))
        data[b, j2, pos] ^= int(rng.integers(1, 256))
        if m == 1:
            continue  # the two errors may cancel in the one syndrome
        if m >= 3:
            want[b] = ((1 << m) - 1, UNLOCATED)
    check(O, codec, shape, data, parity, set(victims(n)), want)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_data_shards_different_bytes(codec, O, shape):
    """Each byte alone looks like a single-shard error, of a different shard."""
    k, m, S, n = shape
    rng = np.random.default_rng(SEED + 4)
    data, parity = copies(O, shape)
    want = {}
    for b in victims(n):
        j1, j2 = two_shards(rng, k)
        p1 = int(rng.integers(0, S))
        p2 = (p1 + 1 + int(rng.integers(0, S - 1))) % S
        data[b, j1, p1] ^= int(rng.integers(1, 256))
        data[b, j2, p2] ^= int(rng.integers(1, 256))
        want[b] = ((1 << m) - 1, UNLOCATED)
    check(O, codec, shape, data, parity, set(want), want)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] >= 3],
                         ids=[i for s, i in zip(SHAPES, IDS) if s[1] >= 3])
def test_data_shard_plus_parity_row(codec, O, shape):
    """Rows 0 and 1 agree on the data shard j, a later row does not."""
    k, m, S, n = shape
    rng = np.random.default_rng(SEED + 5)
    data, parity = copies(O, shape)
    want = {}
    for c, b in enumerate(victims(n)):
        j = int(rng.integers(0, k))
        i = 2 + int(rng.integers(0, m - 2))
        pos = int(rng.integers(0, S))
        data[b, j, pos] ^= int(rng.integers(1, 256))
        # the same byte in odd cases, another byte in even ones
        q = pos if c % 2 else (pos + 1 + int(rng.integers(0, S - 1))) % S
        parity[b, i, q] ^= int(rng.integers(1, 256))
        want[b] = ((1 << m) - 1, UNLOCATED)
    check(O, codec, shape, data, parity, set(want), want)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] >= 2],
                         ids=[i for s, i in zip(SHAPES, IDS) if s[1] >= 2])
def test_two_parity_rows(codec, O, shape):
    """The mask shows exactly the two rows.  They are wrong at different
    bytes, so that with m == 2 (mask = every row) no data shard fits either:
    a byte with one zero and one nonzero syndrome rules every j out."""
    k, m, S, n = shape
    rng = np.random.default_rng(SEED + 6)
    data, parity = copies(O, shape)
    want = {}
    for b in victims(n):
        i1 = int(rng.integers(0, m))
        i2 = (i1 + 1 + int(rng.integers(0, m - 1))) % m
        p1 = int(rng.integers(0, S))
        p2 = (p1 + 1 + int(rng.integers(0, S - 1))) % S
        parity[b, i1, p1] ^= int(rng.integers(1, 256))
        parity[b, i2, p2] ^= int(rng.integers(1, 256))
        want[b] = ((1 << i1) | (1 << i2), UNLOCATED)
    check(O, codec, shape, data, parity, set(want), want)


def test_first_and_last_byte_of_the_batch(codec, O):
    shape = (10, 4, 448, 37)
    k, m, S, n = shape
    data, parity = copies(O, shape)
    data[0, 0, 0] ^= 0x01
    parity[n - 1, m - 1, S - 1] ^= 0x80
    check(O, codec, shape, data, parity, {0, n - 1},
          {0: single(k, m, 0), n - 1: single(k, m, k + m - 1)})


@pytest.mark.parametrize("where", ["pageable", "pinned"])
def test_host_memory_several_pipeline_waves(codec, O, where):
    """64 blocks of RS(10,4) x 4160 (58 240 B each) with pipe_bytes = 1 MiB:
    18 blocks per wave, four waves, a corrupted block in each; the verdict
    words come back at their blocks' offsets."""
    import torch
    from memo_amd import ec
    shape = (10, 4, 4160, 64)
    k, m, S, n = shape
    data, parity = copies(O, shape)
    per_wave = (1 << 20) // ((k + m) * S)
    assert per_wave == 18 and -(-n // per_wave) == 4
    want = {}
    for w, (off, idx) in enumerate([(0, 3), (17, 12), (5, 0), (9, 13)]):
        b = w * per_wave + off
        if idx < k:
            data[b, idx, (w * 977) % S] ^= 0x10
        else:
            parity[b, idx - k, S - 1 - w] ^= 0x10
        want[b] = single(k, m, idx)
    d2, p2 = data.reshape(n, k * S), parity.reshape(n, m * S)
    with codec.options(pipe_bytes=1 << 20):
        if where == "pinned":
            v = codec.verify(k, m, torch.from_numpy(d2).pin_memory(), torch.from_numpy(p2).pin_memory(),
                             torch.full((n,), -1, dtype=torch.int32).pin_memory())
            got = v.numpy().view(np.uint32)
        else:
            got = codec.verify(k, m, d2, p2, np.full(n, 0xFFFFFFFF, dtype=np.uint32))
    assert np.array_equal(got, expected(O, k, m, S, data, parity, set(want)))
    mask, shard = ec.split_verdict(got)
    for b in range(n):
        assert (int(mask[b]), int(shard[b])) == want.get(b, (0, 0)), b


def test_device_call_on_caller_stream(codec, O):
    import torch
    shape = (10, 4, 448, 37)
    k, m, S, n = shape
    data, parity = copies(O, shape)
    data[7, 4, 100] ^= 0x40
    parity[20, 2, 5] ^= 0x02
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            d = torch.from_numpy(data).cuda()
            p = torch.from_numpy(parity).cuda()
            v = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            codec.set_stream(st)
            assert codec.verify(k, m, d, p, v) is v
        st.synchronize()
    finally:
        codec.set_stream(None)
    got = v.cpu().numpy().view(np.uint32)
    want = np.zeros(n, dtype=np.uint32)
    want[7] = 0xF | (4 << 16)
    want[20] = 0x4 | (12 << 16)
    assert np.array_equal(got, want)
    assert np.array_equal(got, expected(O, k, m, S, data, parity, {7, 20}))


def test_split_at_max_launch_tiles(codec, O):
    """max_launch_tiles = 30 with 260-chunk shards (3 tiles counted per
    block) cuts 64 blocks into launches of 10: each launch's words start at
    its first block's offset.  A corrupted block in the first, a middle and
    the last (4-block) launch, and on both sides of a cut."""
    shape = (10, 4, 4160, 64)
    k, m, S, n = shape
    data, parity = copies(O, shape)
    want = {}
    for b, idx in [(3, 2), (9, 11), (10, 0), (35, 13), (59, 7), (60, 10), (63, 9)]:
        if idx < k:
            data[b, idx, (b * 131) % S] ^= 0x04
        else:
            parity[b, idx - k, (b * 131) % S] ^= 0x04
        want[b] = single(k, m, idx)
    with codec.options(max_launch_tiles=30):
        check(O, codec, shape, data, parity, set(want), want)


def test_default_verdict_is_not_wiped_by_the_callers_stream(codec, O):
    """verify(verdict=None) on device tensors while torch's current stream is
    busy: the buffer the binding makes must not be written on that stream (a
    fill there would land after the verify on the ctx stream and leave every
    block reading clean)."""
    import torch
    shape = (10, 4, 448, 37)
    k, m, S, n = shape
    data, parity = copies(O, shape)
    data[5, 1, 9] ^= 0x20
    parity[30, 3, 400] ^= 0x01
    d = torch.from_numpy(data).cuda()
    p = torch.from_numpy(parity).cuda()
    busy = torch.zeros(1 << 28, dtype=torch.uint8, device="cuda")
    # the code's tables cached first: their one synchronous upload would wait
    # for torch's stream and hide the race
    codec.verify(k, m, d, p)
    codec.synchronize()
    torch.cuda.synchronize()
    for _ in range(200):  # tens of ms queued on torch's current stream
        busy.add_(1)
    v = codec.verify(k, m, d, p)
    codec.synchronize()
    torch.cuda.synchronize()
    got = v.cpu().numpy().view(np.uint32)
    want = np.zeros(n, dtype=np.uint32)
    want[5] = 0xF | (1 << 16)
    want[30] = 0x8 | (13 << 16)
    assert np.array_equal(got, want)
    # m == 0: the library writes nothing, the binding hands back zeros
    z = codec.verify(k, 0, d, p[:, :0].contiguous(), S=S, n=n)
    codec.synchronize()
    torch.cuda.synchronize()
    assert z.cpu().tolist() == [0] * n


def test_argument_errors(codec):
    import torch
    from memo_amd import ec
    L = ec._lib()
    d = torch.zeros(4 * 65 * 64, dtype=torch.uint8, device="cuda")
    v = torch.zeros(4, dtype=torch.int32, device="cuda")
    ctx, dp, vp = codec._ctx, d.data_ptr(), v.data_ptr()
    assert L.memo_ec_verify_batch(ctx, 10, 4, 96, 1, dp, dp, vp, ec.DEVICE) == -1   # S % 64
    assert L.memo_ec_verify_batch(ctx, 10, 4, 64, 1, dp, dp, None, ec.DEVICE) == -1  # null verdict
    assert L.memo_ec_verify_batch(ctx, 65, 4, 64, 1, dp, dp, vp, ec.DEVICE) == -6   # k = 65
    assert L.memo_ec_verify_batch(ctx, 10, 4, 64, 1, dp, dp, vp, 7) == -1           # where
    assert L.memo_ec_verify_batch(None, 10, 4, 64, 1, dp, dp, vp, ec.DEVICE) == -1
    # m == 0 or n == 0: nothing is written, not even with a null verdict
    v.fill_(5)
    assert L.memo_ec_verify_batch(ctx, 10, 0, 64, 4, dp, dp, vp, ec.DEVICE) == 0
    assert L.memo_ec_verify_batch(ctx, 10, 4, 64, 0, dp, dp, None, ec.DEVICE) == 0
    codec.synchronize()
    assert v.cpu().tolist() == [5, 5, 5, 5]
    with pytest.raises(TypeError):  # the words are int32 / uint32
        codec.verify(10, 4, torch.zeros((4, 640), dtype=torch.uint8, device="cuda"),
                     torch.zeros((4, 256), dtype=torch.uint8, device="cuda"),
                     torch.zeros(4, dtype=torch.int64, device="cuda"))

"""Ragged encode and verify on the MI355X (memo_ec_encode_ragged /
memo_ec_verify_ragged: gf_mac_ragged_kernel, gf_verify_ragged_kernel,
verify_locate_ragged_kernel).

A ragged batch packs blocks of their own shard sizes back to back: data
shard j of block b at k * off[b] + j * S[b], parity shard i at
m * off[b] + i * S[b].  The judge of an encode is the oracle's encoding of
each block on its own, bit for bit; of a verify, the numpy restatement of
the verdict's definition in tests/test_gpu_verify.py, block by block.  Every
buffer is guarded (tests/guarded.py).

Size lists (shard bytes; a tile is 4096): tests/ragged_cases.py.
  A  65 x 64: 64 blocks in tile 0 (the most a tile holds), one alone in tile 1
  B  3 x 4096: every tile exactly one block (the wave-uniform path only)
  C  straddles, a three-tile block, zero sizes inside and last, partial tail
  D  one 64-byte block; D1 one block of a tile and a bit
  E  200 seeded sizes 0..8320
  F1 / F2  uniform: the layout of memo_ec_encode_batch
"""
import numpy as np
import pytest

from conftest import SEED
from guarded import MEMORIES, Guarded
import ragged_cases as RC
import test_gpu_verify as V

pytestmark = pytest.mark.gpu

# RS(5,3) and RS(20,8) take the chunk loop, RS(6,6) has R > 4
CODES = [(3, 2), (10, 4), (16, 4), (5, 3), (20, 8), (6, 6)]
CASES = [(name, k, m) for name in RC.LISTS for (k, m) in CODES] + \
        [(name, 64, 16) for name in ("A", "C", "D")]
CASE_IDS = ["%s_rs%d_%d" % c for c in CASES]

_CLEAN = {}


def clean(O, name, k, m):
    """(sizes, data k*T, parity m*T) of a list and code: seeded data and the
    oracle's parity of each block on its own; computed once, never written."""
    key = (name, k, m)
    if key not in _CLEAN:
        sizes = RC.LISTS[name]
        off = RC.offsets(sizes)
        T = off[-1]
        rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + T))
        data = rng.integers(0, 256, size=k * T, dtype=np.uint8)
        parity = np.zeros(m * T, dtype=np.uint8)
        for b, S in enumerate(sizes):
            if S:
                d = data[k * off[b]:k * off[b] + k * S].reshape(1, k * S)
                parity[m * off[b]:m * off[b] + m * S] = O.encode(k, m, S, d).reshape(-1)
        data.setflags(write=False)
        parity.setflags(write=False)
        _CLEAN[key] = (sizes, data, parity)
    return _CLEAN[key]


def encode_checked(codec, O, name, k, m, memory="device", sync=True):
    sizes, data, parity = clean(O, name, k, m)
    g = Guarded(memory)
    d = g.input("data", data)
    p = g.output("parity", parity.size)
    assert codec.encode_ragged(k, m, sizes, d, p) is p
    if sync:
        codec.synchronize()
        g.check(parity=parity)
    return g, parity


def expected_words(O, k, m, sizes, data, parity, touched):
    """The verdict words by the definition (test_gpu_verify.expected), each
    touched block judged on its own; every other word 0."""
    off = RC.offsets(sizes)
    out = np.zeros(len(sizes), dtype=np.uint32)
    for b in sorted(touched):
        S = sizes[b]
        d = data[k * off[b]:k * off[b] + k * S].reshape(1, k, S)
        p = parity[m * off[b]:m * off[b] + m * S].reshape(1, m, S)
        out[b] = V.expected(O, k, m, S, d, p, {0})[0]
    return out


def verify_checked(codec, O, k, m, sizes, data, parity, touched, memory="device", sync=True):
    """verify_ragged over guarded buffers (the words preset to 0xA5A5A5A5);
    returns the words after comparing them with the definition."""
    n = len(sizes)
    g = Guarded(memory)
    d = g.input("data", data)
    p = g.input("parity", parity)
    g.output("verdict", 4 * n)
    v = g.words("verdict")
    assert codec.verify_ragged(k, m, sizes, d, p, v) is v
    want = expected_words(O, k, m, sizes, data, parity, touched)
    if not sync:
        return g, want
    codec.synchronize()
    g.check(verdict=want)
    return want


def flip(sizes, k, m, data, parity, b, idx, pos):
    """XOR one bit into byte pos of shard idx (data < k <= parity) of block b."""
    off = RC.offsets(sizes)
    S = sizes[b]
    assert 0 <= pos < S
    if idx < k:
        data[k * off[b] + idx * S + pos] ^= 0x10
    else:
        parity[m * off[b] + (idx - k) * S + pos] ^= 0x10


# ------------------------------------------------------------------ encode

@pytest.mark.parametrize("memory", MEMORIES)
@pytest.mark.parametrize("name,k,m", CASES, ids=CASE_IDS)
def test_encode_matches_the_oracle_block_by_block(codec, O, name, k, m, memory):
    encode_checked(codec, O, name, k, m, memory)


@pytest.mark.parametrize("memory", MEMORIES)
def test_zero_size_blocks_write_nothing(codec, O, memory):
    """A batch of zero sizes only (T == 0) writes nothing at all; zero sizes
    around one real block leave everything but its parity alone."""
    k, m = 10, 4
    g = Guarded(memory)
    d = g.input("data", np.arange(640, dtype=np.uint8))
    p = g.output("parity", 256)
    g.output("verdict", 12)
    codec.encode_ragged(k, m, [0, 0, 0], d, p)
    codec.verify_ragged(k, m, [0, 0, 0], d, p, g.words("verdict"))
    codec.synchronize()
    g.check()
    want = O.encode(k, m, 64, np.arange(640, dtype=np.uint8).reshape(1, 640)).reshape(-1)
    codec.encode_ragged(k, m, [0, 64, 0], d, p)
    codec.verify_ragged(k, m, [0, 64, 0], d, p, g.words("verdict"))
    codec.synchronize()
    g.check(parity=want, verdict=np.zeros(3, np.uint32))


@pytest.mark.parametrize("name", ["F1", "F2"])
@pytest.mark.parametrize("k,m", CODES, ids=["rs%d_%d" % c for c in CODES])
def test_uniform_sizes_equal_the_uniform_call(codec, O, name, k, m):
    """On equal sizes the ragged call writes byte for byte what Codec.encode
    writes from the same data buffer."""
    import torch
    sizes, data, parity = clean(O, name, k, m)
    n, S = len(sizes), sizes[0]
    g = Guarded()
    d = g.input("data", data)
    p1 = g.output("ragged", parity.size)
    p2 = g.output("uniform", parity.size)
    codec.encode_ragged(k, m, sizes, d, p1)
    codec.encode(k, m, d.view(n, k * S), p2.view(n, m * S))
    codec.synchronize()
    assert torch.equal(p1, p2)
    g.check(ragged=parity, uniform=parity)


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("name", ["C", "E"])
def test_launch_split_on_block_boundaries(codec, O, name, limit):
    """max_launch_tiles 1 and 2: spans cut on block boundaries, a block of
    more tiles than the limit in a launch of its own."""
    k, m = 10, 4
    with codec.options(max_launch_tiles=limit):
        encode_checked(codec, O, name, k, m)
        sizes, data, parity = clean(O, name, k, m)
        data, parity = data.copy(), parity.copy()
        victims = [b for b in (0, 3, len(sizes) // 2, len(sizes) - 2) if sizes[b]]
        for b in victims:
            flip(sizes, k, m, data, parity, b, b % (k + m), sizes[b] - 1)
        want = verify_checked(codec, O, k, m, sizes, data, parity, set(victims))
        assert np.count_nonzero(want) == len(set(victims))


def test_xcd_tile_order(codec, O):
    k, m = 10, 4
    with codec.options(xcd_min_tiles=1):
        encode_checked(codec, O, "E", k, m)
        sizes, data, parity = clean(O, "E", k, m)
        verify_checked(codec, O, k, m, sizes, data, parity, set())


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_host_pipeline_waves_cut_by_bytes(codec, O, memory):
    """E from host memory with zero-copy off and the smallest pipe_bytes the
    option takes (1 MiB; k * T is about 8 MiB: several waves, cut on block
    boundaries): encode, then a verify with a corrupted block in the first,
    a middle and the last wave."""
    k, m = 10, 4
    sizes, data, parity = clean(O, "E", k, m)
    assert k * sum(sizes) > 4 << 20
    with codec.options(zero_copy_bytes=0, pipe_bytes=1 << 20):
        encode_checked(codec, O, "E", k, m, memory)
        data, parity = data.copy(), parity.copy()
        victims = [b for b in (1, 99, 100, 198) if sizes[b]]
        assert len(victims) >= 3
        for b in victims:
            flip(sizes, k, m, data, parity, b, (3 * b) % (k + m), 0)
        want = verify_checked(codec, O, k, m, sizes, data, parity, set(victims), memory)
        assert np.count_nonzero(want) == len(victims)


def test_back_to_back_calls_need_no_synchronize(codec, O):
    """Two different ragged encodes (C, then A), then their verifies, on one
    ctx with no synchronize in between: each call's block index must outlive
    the call that follows it."""
    k, m = 10, 4
    gc, pc = encode_checked(codec, O, "C", k, m, sync=False)
    ga, pa = encode_checked(codec, O, "A", k, m, sync=False)
    sc, dc, _ = clean(O, "C", k, m)
    sa, da, _ = clean(O, "A", k, m)
    dcx, pcx = dc.copy(), pc.copy()
    flip(sc, k, m, dcx, pcx, 3, 2, 8255)
    dax, pax = da.copy(), pa.copy()
    flip(sa, k, m, dax, pax, 64, 11, 0)
    gvc, wc = verify_checked(codec, O, k, m, sc, dcx, pcx, {3}, sync=False)
    gva, wa = verify_checked(codec, O, k, m, sa, dax, pax, {64}, sync=False)
    codec.synchronize()
    gc.check(parity=pc)
    ga.check(parity=pa)
    gvc.check(verdict=wc)
    gva.check(verdict=wa)
    assert wc[3] == 0xF | (2 << 16) and wa[64] == 0x2 | (11 << 16)


# ------------------------------------------------------------------ verify

@pytest.mark.parametrize("name,k,m", CASES, ids=CASE_IDS)
def test_verify_clean_is_all_zero(codec, O, name, k, m):
    sizes, data, parity = clean(O, name, k, m)
    want = verify_checked(codec, O, k, m, sizes, data, parity, set())
    assert not want.any()


# blocks on both sides of a tile boundary: A's tile 0 ends behind block 63;
# C has tile edges between blocks 1 | 2, inside 2 (before 3) and inside 3
# (before 4 and 6)
FLIP_BLOCKS = {"A": [0, 63, 64], "C": [0, 1, 2, 3, 4, 6]}


@pytest.mark.parametrize("k,m", [(10, 4), (16, 4), (3, 2)], ids=["rs10_4", "rs16_4", "rs3_2"])
@pytest.mark.parametrize("name", ["A", "C"])
def test_verify_single_flips(codec, O, name, k, m):
    """One flipped byte per call: the first and the last byte of a data shard
    and of a parity shard, in blocks on both sides of a tile boundary.  The
    block's word is the definition's, every other word 0."""
    from memo_amd import ec
    sizes, data0, parity0 = clean(O, name, k, m)
    for b in FLIP_BLOCKS[name]:
        S = sizes[b]
        for idx in (b % k, k + b % m):
            for pos in (0, S - 1):
                data, parity = data0.copy(), parity0.copy()
                flip(sizes, k, m, data, parity, b, idx, pos)
                want = verify_checked(codec, O, k, m, sizes, data, parity, {b})
                assert ec.split_verdict(int(want[b])) == V.single(k, m, idx), (b, idx, pos)
                assert np.count_nonzero(want) == 1


@pytest.mark.parametrize("k,m", [(10, 4), (3, 2)], ids=["rs10_4", "rs3_2"])
def test_verify_two_flips_in_one_tile(codec, O, k, m):
    """Blocks 3 and 4 of A share tile 0 (and a wave): exactly those two are
    flagged, each with its own shard."""
    from memo_amd import ec
    sizes, data, parity = clean(O, "A", k, m)
    data, parity = data.copy(), parity.copy()
    flip(sizes, k, m, data, parity, 3, 1, 63)
    flip(sizes, k, m, data, parity, 4, k + 1, 0)
    want = verify_checked(codec, O, k, m, sizes, data, parity, {3, 4})
    assert np.flatnonzero(want).tolist() == [3, 4]
    assert ec.split_verdict(int(want[3])) == V.single(k, m, 1)
    assert ec.split_verdict(int(want[4])) == V.single(k, m, k + 1)


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_verify_host_memory(codec, O, memory):
    k, m = 10, 4
    sizes, data, parity = clean(O, "C", k, m)
    data, parity = data.copy(), parity.copy()
    flip(sizes, k, m, data, parity, 2, 7, 4159)
    flip(sizes, k, m, data, parity, 6, 12, 0)
    want = verify_checked(codec, O, k, m, sizes, data, parity, {2, 6}, memory)
    assert np.flatnonzero(want).tolist() == [2, 6]


@pytest.mark.parametrize("name", ["F1", "F2"])
def test_verify_uniform_sizes_equal_the_uniform_call(codec, O, name):
    k, m = 10, 4
    sizes, data, parity = clean(O, name, k, m)
    n, S = len(sizes), sizes[0]
    data, parity = data.copy(), parity.copy()
    victims = {0: 3, n // 2: 12, n - 1: 9}
    for b, idx in victims.items():
        flip(sizes, k, m, data, parity, b, idx, (b * 37) % S)
    want = verify_checked(codec, O, k, m, sizes, data, parity, set(victims))
    got = V.run_device(codec, k, m, data.reshape(n, k, S), parity.reshape(n, m, S))
    assert np.array_equal(got, want)
    assert np.count_nonzero(got) == 3


def test_argument_errors_and_empty_calls(codec):
    import ctypes
    import torch
    from memo_amd import ec
    L = ec._lib()
    d = torch.zeros(14 * 4096, dtype=torch.uint8, device="cuda")
    v = torch.full((4,), 5, dtype=torch.int32, device="cuda")
    ctx, dp, vp = codec._ctx, d.data_ptr(), v.data_ptr()
    ok = (ctypes.c_size_t * 2)(64, 128)
    enc, ver = L.memo_ec_encode_ragged, L.memo_ec_verify_ragged
    assert enc(ctx, 10, 4, 2, (ctypes.c_size_t * 2)(64, 96), dp, dp, ec.DEVICE) == -1   # S % 64
    assert enc(ctx, 10, 4, 2, (ctypes.c_size_t * 2)(64, 1 << 32), dp, dp, ec.DEVICE) == -1
    assert enc(ctx, 10, 4, 2, None, dp, dp, ec.DEVICE) == -1                            # NULL sizes
    assert enc(ctx, 10, 4, 2, ok, dp, dp, 7) == -1                                      # where
    assert enc(ctx, 10, 4, 2, ok, dp + 8, dp, ec.DEVICE) == -1                          # alignment
    assert enc(ctx, 10, 4, 2, ok, None, dp, ec.DEVICE) == -1
    assert ver(ctx, 10, 4, 2, ok, dp, dp, None, ec.DEVICE) == -1                        # NULL verdict
    assert ver(ctx, 10, 4, 2, ok, dp, dp, vp + 2, ec.DEVICE) == -1
    # n == 0, T == 0 or m == 0: nothing is written, whatever the buffers
    assert ver(ctx, 10, 4, 0, None, None, None, None, ec.DEVICE) == 0
    assert ver(ctx, 10, 4, 2, (ctypes.c_size_t * 2)(0, 0), dp, dp, vp, ec.DEVICE) == 0
    assert ver(ctx, 10, 0, 2, ok, dp, dp, vp, ec.DEVICE) == 0
    assert enc(ctx, 10, 0, 2, ok, dp, None, ec.DEVICE) == 0
    codec.synchronize()
    assert v.cpu().tolist() == [5, 5, 5, 5]
    assert not d.any().item()

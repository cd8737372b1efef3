"""memo_ec_correct_batch on the MI355X: the check of any k + x shards in hand
and, on the device, the wrong shard of every located block rewritten.  Words
are held bit for bit, bytes byte for byte: to the original shards where one
shard of a block was overwritten, to memo_amd/correct_ref.py otherwise.  There
is no tolerance.

Every buffer of every call sits between guards (tests/guarded.py): the index
rows, the shards -- read and written here, so their payload is judged against
the bytes expected after the call and everything the call must leave alone is
held to what was put in -- and the verdict words, in device, pinned and
pageable memory.

The first tests run the call's two new kernels on the narrowest inputs that
reach them, one more at a time:
  test_1a  one clean block      correct_list_kernel finds nothing,
                                gf_correct_kernel reads a count of 0
  test_1b  one wrong spare      + one list entry, row q - k as it is
  test_1c  one wrong basis      + the scaled row 0 and spare 0 standing in
  test_1d  the bring-up batch   clean, spare, basis, two wrong shards, invalid
Every shape here is walked on the CPU first (tests/test_correct_plan.py)."""
import functools

import numpy as np
import pytest

import correct_cases as CC
from conftest import SEED
from correct_cases import CORRECTED, clean_batch, mislocated_blocks, oracle, single_batch, single_word
from guarded import Guarded
from test_check_reference import IDS, SHAPES
from test_check_restated import INVALID, UNLOCATED, random_sets, shards_of, take
from test_gpu_bounds import Cases, rebuild_ref, sync
from test_gpu_check import recipe, reference

pytestmark = pytest.mark.gpu

ESINGULAR = -4


def inout(g, name, data):
    """A guarded buffer the call reads and writes: preset to `data`, judged
    like an output (unnamed in check(): it must still hold `data`)."""
    data = np.ascontiguousarray(data, np.uint8)
    return g._add(name, "output", data, None, 0, data.shape)


def run_correct(codec, cases, label, k, m, x, S, n, idx, have, words, after, memory="device", idx_shift=0):
    g = Guarded(memory)
    hi = g.input("have_idx", np.ascontiguousarray(idx, np.uint8).reshape(n, k + x), shift=idx_shift)
    hv = inout(g, "have", np.asarray(have).reshape(n, (k + x) * S)) if S else None
    g.output("verdict", 4 * n)  # 0xA5A5A5A5 words: the call must write every one
    codec.correct(k, m, hi, hv, g.words("verdict"), x=x, S=S, n=n)
    sync(codec, memory)  # a correction is a result, not an error
    want = {"verdict": np.asarray(words, np.uint32)}
    if S:
        want["have"] = np.asarray(after, np.uint8).reshape(n, (k + x) * S)
    cases.check(label, g, **want)


def by_reference(k, m, x, S, idx, have):
    """(words, after) by memo_amd.correct_ref, the words' low 24 bits held to
    both host statements of the check (test_gpu_check.reference)."""
    from memo_amd import correct_ref as C
    n = np.asarray(idx).reshape(-1, k + x).shape[0]
    words, after = C.correct_reference(k, m, idx, np.asarray(have).reshape(n, -1), x=x, S=S)
    chk = reference(k, m, x, S, idx, have)
    located = (chk != 0) & (chk != INVALID) & (((chk >> 16) & 0xFF) != UNLOCATED) & (x >= 2) & (S > 0)
    assert np.array_equal(words, np.where(located, chk | np.uint32(CORRECTED), chk))
    return words, after


def run_single(codec, cases, label, shape, targets=None, memory="device", idx_shift=0, seed=0):
    """One overwritten shard in each target block: the original bytes come
    back and the words are the analytic ones."""
    k, m, x, S, n = shape
    idx, clean, have, words = single_batch(shape, targets, seed)
    run_correct(codec, cases, label, k, m, x, S, n, idx, have, words, clean, memory, idx_shift)


# ------------------------------------------------------------------ 1: bring-up
@functools.lru_cache(maxsize=None)
def bringup():
    """RS(3,2), x = 2, S = 64, n = 5: clean, a wrong spare, a wrong basis
    shard, two wrong shards (different bytes: unlocated), an invalid set."""
    k, m, x, S, n = CC.BRINGUP
    idx, clean = clean_batch(k, m, x, S, n, SEED + 101)
    idx, have = idx.copy(), clean.copy()
    rng = np.random.default_rng(SEED + 102)
    CC.overwrite(have, 1, k + 1, rng)
    CC.overwrite(have, 2, 1, rng)
    have[3, 0, 5] ^= 0x21
    have[3, 2, 40] ^= 0x7
    idx[4, 2] = idx[4, 0]
    have[4, 1, 9] ^= 0xFF           # an invalid block's bytes are never judged or written
    words, after = by_reference(k, m, x, S, idx, have)
    assert words[0] == 0 and words[1] == single_word(idx, 1, k + 1, k, x) and words[2] == single_word(idx, 2, 1, k, x)
    assert (int(words[3]) >> 16) == UNLOCATED and words[4] == INVALID
    assert np.array_equal(after[:3], clean[:3]) and np.array_equal(after[3:], have[3:])
    return idx, have, words, after


def test_1a_one_clean_block(codec):
    k, m, x, S, _ = CC.BRINGUP
    idx, have, words, after = bringup()
    cases = Cases()
    run_correct(codec, cases, "clean", k, m, x, S, 1, idx[:1], have[:1], words[:1], after[:1])
    cases.done()


def test_1b_one_wrong_spare(codec):
    k, m, x, S, _ = CC.BRINGUP
    idx, have, words, after = bringup()
    cases = Cases()
    run_correct(codec, cases, "spare", k, m, x, S, 1, idx[1:2], have[1:2], words[1:2], after[1:2])
    cases.done()


def test_1c_one_wrong_basis_shard(codec):
    k, m, x, S, _ = CC.BRINGUP
    idx, have, words, after = bringup()
    cases = Cases()
    run_correct(codec, cases, "basis", k, m, x, S, 1, idx[2:3], have[2:3], words[2:3], after[2:3])
    cases.done()


def test_1d_bringup_batch(codec):
    k, m, x, S, n = CC.BRINGUP
    idx, have, words, after = bringup()
    cases = Cases()
    run_correct(codec, cases, "bring-up", k, m, x, S, n, idx, have, words, after)
    cases.done()


# ------------------------------------------------ 2: every shape, every memory
@functools.lru_cache(maxsize=None)
def expected(shape):
    """The check tests' batch of `shape` (clean blocks, one wrong spare, one
    wrong basis shard, two wrong basis shards) and what the call makes of it:
    (idx, have, words, after).  Blocks with one wrong shard are held to the
    original bytes, rebuilt here from the batch's own seed."""
    k, m, x, S, n = shape
    idx, have, _ = recipe(shape)
    words, after = by_reference(k, m, x, S, idx, have)
    rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + x * 101 + S * 31 + n))
    full = shards_of(oracle(), k, m, S, rng, n)
    assert np.array_equal(random_sets(rng, k, m, x, n), idx)
    clean = take(full, idx)
    for c, b in enumerate(range(1, n, 2)):
        if c % 5 in (0, 1, 2) and x >= 2:
            assert np.array_equal(after[b], clean[b]) and (int(words[b]) >> 24) == 1, b
    for b in range(0, n, 2):
        assert words[b] == 0 and np.array_equal(after[b], have[b])
    for a in (words, after):
        a.setflags(write=False)
    return idx, have, words, after


@pytest.mark.parametrize("memory", ["device", "pinned", "pageable"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_2_shapes_in_every_memory(codec, shape, memory):
    k, m, x, S, n = shape
    idx, have, words, after = expected(shape)
    cases = Cases()
    run_correct(codec, cases, memory, k, m, x, S, n, idx, have, words, after, memory=memory,
                idx_shift=1 if memory == "pageable" else 0)
    cases.done()


# ------------------------------------------------------ 3: several pipeline waves
@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_3_host_memory_several_pipeline_waves(codec, memory):
    """RS(10,4), x = 2, S = 32 KiB, n = 9 with a 1 MiB pipeline batch: two
    blocks per wave, five waves over the three slots.  A corrected block in
    every wave, always the wave's last one, both blocks of the first wave,
    and the single block of the last."""
    k, m, x, S, n = CC.WAVES
    targets = ((0, k), (1, 0), (3, k + 1), (5, k - 1), (7, 4), (8, k))
    cases = Cases()
    with codec.options(pipe_bytes=1 << 20):
        run_single(codec, cases, memory, CC.WAVES, targets, memory=memory,
                   idx_shift=1 if memory == "pageable" else 0)
    cases.done()


# ------------------------------------------------------------------ 4: tile edges
@pytest.mark.parametrize("shape", CC.EDGES, ids=["rs%d_%d_x%d_S%d_n%d" % s for s in CC.EDGES])
def test_4_tile_edges(codec, shape):
    """S = 4160: a full tile and a 64-byte tail (4 active lanes); S = 64: 4
    active lanes in all.  The target in the first and last position of the
    basis and of the spares; two clean blocks behind them."""
    k, m, x, S, n = shape
    cases = Cases()
    run_single(codec, cases, "edges", shape, ((0, 0), (1, k - 1), (2, k), (3, k + x - 1)))
    cases.done()


# ---------------------------------------------------------------- 5: list and grid
def test_5_every_block_located(codec):
    """n = 4099, S = 64, RS(3,2): 4099 located blocks, one tile each -- more
    than the correction's grid cap, and 17 list-building workgroups.  The
    words are analytic: a wrong spare r gives 1 << r, a wrong basis shard
    every row."""
    k, m, x, S, n = CC.LIST
    idx, clean, have, words = single_batch(CC.LIST)
    for b in (0, 1, 2, 3, 4, n - 1):
        pos = b % (k + x)
        assert int(words[b]) & 0xFFFF == (0x3 if pos < k else 1 << (pos - k))
    cases = Cases()
    run_correct(codec, cases, "all", k, m, x, S, n, idx, have, words, clean)
    cases.done()


def test_5_one_block_in_64_located(codec):
    k, m, x, S, n = CC.LIST
    targets = tuple((b, (b // 64) % (k + x)) for b in range(63, n, 64))
    assert len(targets) == 64
    cases = Cases()
    run_single(codec, cases, "1 in 64", CC.LIST, targets, seed=1)
    cases.done()


# ------------------------------------------------------------ 6: every compiled KC
@pytest.mark.parametrize("KC", CC.KCS, ids=["kc%d" % KC for KC in CC.KCS])
def test_6_every_compiled_chunk(codec, KC):
    """gf_correct_kernel<KC> with k == KC, and under KC = 4 the chunk loop at
    k = 5 (a tail of one shard), 33 and 64; x = 2 and x = m.  Targets: first
    and last of basis and spares and a middle basis shard; one clean block."""
    from memo_amd import ec
    cases = Cases()
    for k in CC.KC_CODES[KC]:
        assert ec.mac_kchunk(k, 1) == KC
        for x in (2, CC.KC_M):
            shape = (k, CC.KC_M, x, CC.KC_S, CC.KC_N)
            targets = ((0, 0), (1, k - 1), (2, k), (3, k + x - 1), (4, k // 2))
            run_single(codec, cases, "k=%d x=%d" % (k, x), shape, targets)
    cases.done()


# --------------------------------------------------------------- 7: nothing to mend
def test_7_nothing_to_mend(codec):
    """x == 1, S == 0, invalid sets and clean batches: the words are
    Codec.check's and `have` is byte-identical."""
    import torch
    cases = Cases()

    def both(label, k, m, x, S, n, idx, have, analytic):
        hi = torch.from_numpy(np.array(idx, np.uint8)).cuda()
        hv = torch.from_numpy(np.array(have, np.uint8).reshape(n, -1)).cuda() if S else None
        chk = codec.check(k, m, hi, hv, x=x, S=S, n=n)
        codec.synchronize()
        chk = chk.cpu().numpy().view(np.uint32)
        assert np.array_equal(chk, analytic), label
        run_correct(codec, cases, label, k, m, x, S, n, idx, have, chk, have)

    # x == 1: detect only
    shape = SHAPES[7]
    k, m, x, S, n = shape
    assert x == 1
    idx, have, want = recipe(shape)
    assert want[1::2].all()
    both("x=1", k, m, x, S, n, idx, have, want)
    # invalid sets between clean blocks, with bytes and with S == 0
    k, m, x, S, n = 10, 4, 3, 448, 24
    idx, have = clean_batch(k, m, x, S, n, SEED + 71)
    idx = idx.copy()
    idx[2, 7] = idx[2, 3]
    idx[14, 5] = k + m
    idx[23, k] = 255
    analytic = np.zeros(n, np.uint32)
    analytic[[2, 14, 23]] = INVALID
    both("invalid sets", k, m, x, S, n, idx, have, analytic)
    both("S=0", k, m, x, 0, n, idx, None, analytic)
    # clean batches: small blocks and several tiles per block
    for shape in [(10, 4, 4, 448, 37), (16, 4, 2, 8256, 3)]:
        k, m, x, S, n = shape
        idx, have = clean_batch(k, m, x, S, n, SEED + 72)
        both("clean S=%d" % S, k, m, x, S, n, idx, have, np.zeros(n, np.uint32))
    cases.done()


# ------------------------------------------------- 8: the identity set is verify's
@pytest.mark.parametrize("km", [(3, 2), (10, 4), (7, 5)], ids=lambda p: "rs%d_%d" % p)
def test_8_identity_set_corrects_what_verify_locates(codec, km):
    import torch
    k, m = km
    S, n = 128, 16
    rng = np.random.default_rng(SEED ^ (k * 137 + m))
    clean = shards_of(oracle(), k, m, S, rng, n)
    full = clean.copy()
    for b in range(1, n, 2):
        CC.overwrite(full, b, (3 * b) % (k + m), rng)
    ident = np.tile(np.arange(k + m, dtype=np.uint8), (n, 1))
    d = torch.from_numpy(np.ascontiguousarray(full[:, :k]).reshape(n, k * S)).cuda()
    p = torch.from_numpy(np.ascontiguousarray(full[:, k:]).reshape(n, m * S)).cuda()
    v = codec.verify(k, m, d, p)
    codec.synchronize()
    v = v.cpu().numpy().view(np.uint32)
    assert not v[0::2].any() and v[1::2].all() and not (v >> 24).any()
    assert [int(w) >> 16 for w in v[1::2]] == [(3 * b) % (k + m) for b in range(1, n, 2)]
    words = np.where(v != 0, v | np.uint32(CORRECTED), v)
    cases = Cases()
    run_correct(codec, cases, "identity", k, m, m, S, n, ident, full, words, clean)
    cases.done()


# ------------------------------------------------------------- 9: launch splitting
def test_9_split_at_max_launch_tiles(codec):
    k, m, x, S, n = CC.SPLIT
    cases = Cases()
    with codec.options(max_launch_tiles=3):  # the check: one block per launch
        run_single(codec, cases, "tiles=3", CC.SPLIT, ((1, 0), (3, k + 1), (4, k - 1)))
    cases.done()


# ----------------------------------------------- 10: back to back on one scratch
def test_10_two_corrects_and_a_singular_rebuild_without_a_synchronize(codec):
    """correct, a rebuild with a bad survivor set, correct of the same
    buffers, one synchronize: the second correct finds the mended blocks
    clean, and the rebuild's ESINGULAR is still reported afterwards."""
    import torch
    from memo_amd import ec
    shape = (10, 4, 4, 448, 37)
    k, m, x, S, n = shape
    idx, clean, have, words = single_batch(shape, tuple((b, (5 * b) % (k + x)) for b in range(1, n, 3)))
    rk, rm, rS, rn = 10, 4, 448, 5
    s, l, surv, _ = rebuild_ref(rk, rm, rS, 2, rn)
    s = s.copy()
    s[1, 3] = s[1, 0]
    r_out = torch.empty((rn, 2 * rS), dtype=torch.uint8, device="cuda")
    r_s, r_surv, r_l = (torch.from_numpy(a.copy()).cuda() for a in (s, surv, l))
    g = Guarded("device")
    hi = g.input("have_idx", idx)
    hv = inout(g, "have", have.reshape(n, -1))
    g.output("first", 4 * n)
    g.output("second", 4 * n)
    codec.synchronize()
    codec.correct(k, m, hi, hv, g.words("first"), x=x, S=S, n=n)
    codec.rebuild(rk, rm, r_s, r_surv, r_l, r_out)
    codec.correct(k, m, hi, hv, g.words("second"), x=x, S=S, n=n)
    with pytest.raises(ec.MemoECError) as err:
        codec.synchronize()
    assert err.value.code == ESINGULAR
    cases = Cases()
    cases.check("back to back", g, have=clean.reshape(n, -1), first=words, second=np.zeros(n, np.uint32))
    codec.synchronize()  # reported once
    cases.done()


# ------------------------------------------------------------------ 11: mislocation
@pytest.mark.parametrize("code", CC.MISLOCATED, ids=lambda c: "rs%d_%d_x%d_S%d" % c)
def test_11_two_wrong_shards_that_pass_for_one(codec, code):
    """The blocks of tests/test_correct_reference.py's mislocation test: the
    device overwrites the same (right) shard with the same bytes."""
    k, m, x, S = code
    idx, have, cs = mislocated_blocks(k, m, x, S)
    n = len(cs)
    assert n == k
    words, after = by_reference(k, m, x, S, idx, have)
    assert all((int(w) >> 24) == 1 for w in words) and not np.array_equal(after, have)
    cases = Cases()
    run_correct(codec, cases, "mislocated", k, m, x, S, n, idx, have, words, after)
    cases.done()

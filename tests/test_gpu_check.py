"""memo_ec_check_batch on the MI355X: any k + x shards in hand, judged on the
GPU, every verdict word held bit for bit to both host statements of it --
the oracle-based definition (tests/test_check_restated.py: expected_check)
and the package's reference (memo_amd/check_ref.py: check_reference).  There
is no tolerance.

Every buffer of every call sits between guards (tests/guarded.py): the index
rows, the shards and the verdict words, in device, pinned and pageable
memory, so a stray store shows as a failed assertion.

The first three tests run the call's new kernels one more at a time, each on
the narrowest input that reaches it:
  test_1  S = 0                   check_prepare_kernel alone
  test_2  one clean block         + the decode rows and gf_check_kernel (the
                                  locate pass finds no flagged word)
  test_3  one flipped byte        + the work of check_locate_kernel

A reference is computed once per batch (both statements, which must agree)
and only for the batch's distinct blocks: the verdict is a function of one
block's index row and bytes, so equal blocks have equal words."""
import functools

import numpy as np
import pytest

import mac_bodies as B
from conftest import SEED
from guarded import Guarded
from test_check_reference import IDS, SHAPES
from test_check_restated import INVALID, UNLOCATED, expected_check, random_sets, shards_of, take
from test_gpu_bounds import Cases, rebuild_ref, sync

pytestmark = pytest.mark.gpu

ESINGULAR = -4


def oracle():
    from oracle import oracle as O
    O.build()
    return O


def reference(k, m, x, S, idx, have):
    """The n verdict words by both host statements (asserted equal), each
    evaluated on the batch's distinct blocks only."""
    from memo_amd import check_ref as R
    O = oracle()
    idx = np.ascontiguousarray(idx, dtype=np.uint8).reshape(-1, k + x)
    n = idx.shape[0]
    have = np.ascontiguousarray(have, dtype=np.uint8).reshape(n, k + x, S)
    first, which = {}, np.empty(n, np.int64)
    for b in range(n):
        which[b] = first.setdefault((idx[b].tobytes(), have[b].tobytes()), len(first))
    rows = sorted(first.values())
    pick = np.array([int(np.flatnonzero(which == u)[0]) for u in rows])
    a = expected_check(O, k, m, S, idx[pick], have[pick], x)
    r = R.check_reference(k, m, idx[pick], have[pick], x=x, S=S)
    assert a.dtype == r.dtype == np.uint32 and np.array_equal(a, r), (a, r)
    return a[which]


def run_check(codec, cases, label, k, m, x, S, n, idx, have, want, memory="device", idx_shift=0):
    g = Guarded(memory)
    hi = g.input("have_idx", np.ascontiguousarray(idx, np.uint8).reshape(n, k + x), shift=idx_shift)
    hv = g.input("have", np.ascontiguousarray(have, np.uint8).reshape(n, (k + x) * S)) if S else None
    g.output("verdict", 4 * n)  # 0xA5A5A5A5 words: the call must write every one
    codec.check(k, m, hi, hv, g.words("verdict"), x=x, S=S, n=n)
    sync(codec, memory)  # a mismatch and an invalid set are results, not errors
    cases.check(label, g, verdict=np.asarray(want, np.uint32))


@functools.lru_cache(maxsize=None)
def invalid_batch():
    """The batch of test_check_reference.test_invalid_sets_one_per_block_
    between_valid_ones: RS(10,4), x = 3, S = 448, n = 24, five invalid sets of
    five kinds between valid ones, two corrupted blocks.  (idx, have)."""
    k, m, x, S, n = 10, 4, 3, 448, 24
    rng = np.random.default_rng(SEED + 16)
    full = shards_of(oracle(), k, m, S, rng, n)
    idx = random_sets(rng, k, m, x, n)
    have = take(full, idx)
    idx[2, 7] = idx[2, 3]            # duplicate inside the basis
    idx[6, k + 1] = idx[6, 4]        # spare equal to a basis shard
    idx[10, k + 2] = idx[10, k]      # spare equal to another spare
    idx[14, 5] = k + m               # first index past the code
    idx[18, k] = 255
    have[5, 2, 17] ^= 0x40
    have[13, k + 1, S - 1] ^= 0x01
    idx.setflags(write=False)
    have.setflags(write=False)
    return idx, have


INVALID_AT = [2, 6, 10, 14, 18]


# ---------------------------------------------------- 1-3: one kernel more each
def test_1_index_sets_alone(codec):
    """S = 0: check_prepare_kernel alone.  Words 0 / INVALID, `have` NULL."""
    k, m, x, n = 10, 4, 3, 24
    idx, _ = invalid_batch()
    want = np.zeros(n, np.uint32)
    want[INVALID_AT] = INVALID
    assert np.array_equal(want, reference(k, m, x, 0, idx, np.zeros((n, k + x, 0), np.uint8)))
    cases = Cases()
    run_check(codec, cases, "S=0", k, m, x, 0, n, idx, None, want)
    cases.done()


@functools.lru_cache(maxsize=None)
def one_block():
    k, m, x, S = 3, 2, 2, 64
    rng = np.random.default_rng(SEED + 3)
    full = shards_of(oracle(), k, m, S, rng, 1)
    idx = np.array([[4, 0, 2, 1, 3]], np.uint8)  # a parity shard in the basis, a data shard spare
    have = take(full, idx)
    idx.setflags(write=False)
    have.setflags(write=False)
    return idx, have


def test_2_one_clean_block(codec):
    k, m, x, S = 3, 2, 2, 64
    idx, have = one_block()
    want = reference(k, m, x, S, idx, have)
    assert want.tolist() == [0]
    cases = Cases()
    run_check(codec, cases, "clean", k, m, x, S, 1, idx, have, want)
    cases.done()


def test_3_one_flipped_byte(codec):
    """The same block with one spare byte flipped, then one basis byte."""
    k, m, x, S = 3, 2, 2, 64
    idx, clean = one_block()
    cases = Cases()
    for pos, byte, word in [(k + 1, 37, 0x2 | (int(idx[0, k + 1]) << 16)), (1, 63, 0x3 | (int(idx[0, 1]) << 16))]:
        have = clean.copy()
        have[0, pos, byte] ^= 0x20
        want = reference(k, m, x, S, idx, have)
        assert want.tolist() == [word], (hex(int(want[0])), hex(word))
        run_check(codec, cases, "position %d" % pos, k, m, x, S, 1, idx, have, want)
    cases.done()


# ------------------------------------------------- 4: every shape, every memory
@functools.lru_cache(maxsize=None)
def recipe(shape):
    """The batch of test_check_reference.test_reference_equals_the_restated_
    definition for `shape`: clean blocks, one wrong spare, one wrong basis
    shard (first and last byte), two wrong basis shards.  (idx, have, want)."""
    O = oracle()
    k, m, x, S, n = shape
    rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + x * 101 + S * 31 + n))
    full = shards_of(O, k, m, S, rng, n)
    idx = random_sets(rng, k, m, x, n)
    have = take(full, idx)
    for c, b in enumerate(range(1, n, 2)):
        kind = c % 5
        if kind == 0:
            have[b, k + c % x, int(rng.integers(0, S))] ^= 1 << int(rng.integers(0, 8))
        elif kind in (1, 2):
            have[b, c % k, 0 if kind == 1 else S - 1] ^= int(rng.integers(1, 256))
        else:
            t1 = int(rng.integers(0, k))
            t2 = (t1 + 1 + int(rng.integers(0, k - 1))) % k
            p1 = int(rng.integers(0, S))
            p2 = p1 if kind == 3 else (p1 + 1 + int(rng.integers(0, S - 1))) % S
            have[b, t1, p1] ^= int(rng.integers(1, 256))
            have[b, t2, p2] ^= int(rng.integers(1, 256))
    want = reference(k, m, x, S, idx, have)
    assert not want[0::2].any() and (n == 1 or want[1::2].all())
    for a in (idx, have, want):
        a.setflags(write=False)
    return idx, have, want


@pytest.mark.parametrize("memory", ["device", "pinned", "pageable"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_4_shapes_in_every_memory(codec, shape, memory):
    k, m, x, S, n = shape
    idx, have, want = recipe(shape)
    cases = Cases()
    run_check(codec, cases, memory, k, m, x, S, n, idx, have, want, memory=memory,
              idx_shift=1 if memory == "pageable" else 0)
    cases.done()


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_4_host_memory_several_pipeline_waves(codec, memory):
    """RS(10,4), x = 2, S = 32 KiB, n = 9 with a 1 MiB pipeline batch: two
    blocks per wave, five waves over the three slots, each with its own part
    of the scratch; every second block corrupted."""
    shape = (10, 4, 2, 32768, 9)
    k, m, x, S, n = shape
    idx, have, want = recipe(shape)
    cases = Cases()
    with codec.options(pipe_bytes=1 << 20):
        run_check(codec, cases, memory, k, m, x, S, n, idx, have, want, memory=memory,
                  idx_shift=1 if memory == "pageable" else 0)
    cases.done()


# ------------------------------------------------------------- 5: tile edges
def test_5_tile_edges(codec):
    """S = 4160 (a 256-column tile and a 4-column one, or a flat tile across
    two blocks), RS(16,4), x = 3: single flipped bytes on either side of the
    tile edge and at the shard's ends, in a basis shard and in a spare."""
    k, m, x, S = 16, 4, 3, 4160
    offsets = [0, 4095, 4096, 4159]
    n = 2 * len(offsets) + 2
    rng = np.random.default_rng(SEED + 5)
    idx = random_sets(rng, k, m, x, n)
    have = take(shards_of(oracle(), k, m, S, rng, n), idx)
    words = {}
    for i, p in enumerate(offsets):
        have[1 + i, 7, p] ^= 0x80
        words[1 + i] = 0x7 | (int(idx[1 + i, 7]) << 16)
        have[5 + i, k + 2, p] ^= 0x01
        words[5 + i] = 0x4 | (int(idx[5 + i, k + 2]) << 16)
    want = reference(k, m, x, S, idx, have)
    assert want[0] == 0 and want[n - 1] == 0 and all(want[b] == w for b, w in words.items())
    cases = Cases()
    run_check(codec, cases, "S=4160", k, m, x, S, n, idx, have, want)
    cases.done()


def test_5_alternating_blocks_inside_one_flat_tile(codec):
    """S = 64, n = 130: 64 blocks per tile, clean and corrupted alternating,
    so neighbouring lanes OR into different words."""
    k, m, x, S, n = 16, 4, 3, 64, 130
    rng = np.random.default_rng(SEED + 55)
    idx = random_sets(rng, k, m, x, n)
    have = take(shards_of(oracle(), k, m, S, rng, n), idx)
    for b in range(1, n, 2):
        pos = (b // 2) % (k + x)
        have[b, pos, (7 * b) % S] ^= 1 + b % 255
    want = reference(k, m, x, S, idx, have)
    assert not want[0::2].any() and want[1::2].all()
    assert all(int(want[b]) >> 16 == int(idx[b, (b // 2) % (k + x)]) for b in range(1, n, 2))
    cases = Cases()
    run_check(codec, cases, "S=64 n=130", k, m, x, S, n, idx, have, want)
    cases.done()


# ------------------------------------------------------------ 6: invalid sets
def test_6_invalid_sets_are_results(codec):
    from memo_amd import ec
    k, m, x, S, n = 10, 4, 3, 448, 24
    idx, have = invalid_batch()
    want = reference(k, m, x, S, idx, have)
    assert (want[INVALID_AT] == INVALID).all() and np.count_nonzero(want == INVALID) == 5
    assert want[5] == 0x7 | (int(idx[5, 2]) << 16) and want[13] == 0x2 | (int(idx[13, k + 1]) << 16)
    cases = Cases()
    codec.synchronize()
    run_check(codec, cases, "invalid sets", k, m, x, S, n, idx, have, want)  # its synchronize() raises nothing
    # a rebuild with a bad survivor set, then a check: the rebuild's error is
    # still pending afterwards, and the check's words are right
    import torch
    s, l, surv, _ = rebuild_ref(k, m, S, 2, 5)
    s = s.copy()
    s[1, 3] = s[1, 0]
    out = torch.empty((5, 2 * S), dtype=torch.uint8, device="cuda")
    codec.rebuild(k, m, torch.from_numpy(s).cuda(), torch.from_numpy(surv.copy()).cuda(),
                  torch.from_numpy(l.copy()).cuda(), out)
    g = Guarded("device")
    hi = g.input("have_idx", idx)
    hv = g.input("have", have.reshape(n, -1))
    g.output("verdict", 4 * n)
    codec.check(k, m, hi, hv, g.words("verdict"), x=x, S=S, n=n)
    with pytest.raises(ec.MemoECError) as err:
        codec.synchronize()
    assert err.value.code == ESINGULAR
    cases.check("after a singular rebuild", g, verdict=want)
    codec.synchronize()  # reported once
    cases.done()


# ------------------------------------------------- 7: the identity set is verify
@pytest.mark.parametrize("km", [(3, 2), (10, 4), (7, 5)], ids=lambda p: "rs%d_%d" % p)
def test_7_identity_set_equals_verify(codec, km):
    import torch
    k, m = km
    S, n = 128, 16
    rng = np.random.default_rng(SEED ^ (k * 131 + m))
    full = shards_of(oracle(), k, m, S, rng, n)
    for b in range(1, n, 2):
        full[b, b % (k + m), int(rng.integers(0, S))] ^= int(rng.integers(1, 256))
        if b % 3 == 0:
            full[b, (b + 1) % (k + m), int(rng.integers(0, S))] ^= int(rng.integers(1, 256))
    ident = np.tile(np.arange(k + m, dtype=np.uint8), (n, 1))
    want = reference(k, m, m, S, ident, full)
    d = torch.from_numpy(np.ascontiguousarray(full[:, :k]).reshape(n, k * S)).cuda()
    p = torch.from_numpy(np.ascontiguousarray(full[:, k:]).reshape(n, m * S)).cuda()
    v = codec.verify(k, m, d, p)
    codec.synchronize()
    assert np.array_equal(v.cpu().numpy().view(np.uint32), want)
    cases = Cases()
    run_check(codec, cases, "identity", k, m, m, S, n, ident, full, want)
    cases.done()


# ------------------------------------------------------------ 8: several spans
def test_8_split_at_max_launch_tiles(codec):
    shape = (10, 4, 4, 4160, 5)
    k, m, x, S, n = shape
    idx, have, want = recipe(shape)
    assert want[1] and want[3] and not want[4]
    cases = Cases()
    with codec.options(max_launch_tiles=3):  # one block per launch
        run_check(codec, cases, "tiles=3", k, m, x, S, n, idx, have, want)
    cases.done()


# --------------------------------------------- 9: back to back on one scratch
def test_9_two_checks_and_a_rebuild_without_a_synchronize(codec):
    """check, rebuild (decode rows + MAC: the path that uses the scratch),
    check of another geometry, one synchronize at the end: the three share
    the ctx's scratch and are ordered by the stream alone."""
    sa, sb = (10, 4, 4, 448, 37), (16, 4, 3, 4160, 5)
    ia, ha, wa = recipe(sa)
    ib, hb, wb = recipe(sb)
    rk, rm, rS, re, rn = 10, 4, 4160, 4, 5
    s, l, surv, lost = rebuild_ref(rk, rm, rS, re, rn)
    g = Guarded("device")
    a_idx, a_have = g.input("a.have_idx", ia), g.input("a.have", ha.reshape(sa[4], -1))
    b_idx, b_have = g.input("b.have_idx", ib), g.input("b.have", hb.reshape(sb[4], -1))
    g.output("a.verdict", 4 * sa[4])
    g.output("b.verdict", 4 * sb[4])
    r_s, r_l, r_surv = g.input("r.surv_idx", s), g.input("r.lost_idx", l), g.input("r.surv", surv)
    r_out = g.output("r.out", (rn, re * rS))
    with codec.options(rebuild_path=0, image_min_tiles=0):
        codec.check(sa[0], sa[1], a_idx, a_have, g.words("a.verdict"), x=sa[2], S=sa[3], n=sa[4])
        codec.rebuild(rk, rm, r_s, r_surv, r_l, r_out)
        codec.check(sb[0], sb[1], b_idx, b_have, g.words("b.verdict"), x=sb[2], S=sb[3], n=sb[4])
        codec.synchronize()
    cases = Cases()
    cases.check("back to back", g, **{"a.verdict": wa, "b.verdict": wb, "r.out": lost})
    cases.done()


# ------------------------------------------------------ 10: every compiled body
KCS = sorted({KC for KC, _ in B.COMPILED})
COMMON = [(64, 1), (64, 130), (4160, 3)]   # (S, n)


def body_batch(k, m, x, S, n):
    """n blocks made of three distinct clean ones (their own index sets,
    repeated in turn) and one corrupted block: the last byte of the last
    spare where the code's number is even (the row next to the padding), the
    last byte of the last basis shard where it is odd (the chunk loop's tail
    shard)."""
    rng = np.random.default_rng(SEED ^ (k * 8191 + x * 127 + S))
    idx3 = random_sets(rng, k, m, x, 3)
    have3 = take(shards_of(oracle(), k, m, S, rng, 3), idx3)
    sel = np.arange(n) % 3
    idx, have = idx3[sel].copy(), have3[sel].copy()
    b = n // 2
    pos = k + x - 1 if (k + x) % 2 == 0 else k - 1
    have[b, pos, S - 1] ^= 0x10
    return idx, have, b, pos


@pytest.mark.parametrize("KC", KCS, ids=["kc%d" % KC for KC in KCS])
def test_10_every_compiled_body(codec, KC):
    """gf_check_kernel<KC, R> for every R, through the codes of
    mac_bodies.codes() with r as x and m = max(x, 1): every body dense and
    with its largest padding, the chunk loop at every k % 4.  R <= 4 takes
    the early spare loads, k <= 16 check_locate_kernel<16>, k > 16 <64>."""
    cases = Cases()
    for k, x in B.codes_of(KC):
        m = max(x, 1)
        shapes = list(COMMON)
        edge = B.edge_sizes("rows", k, x)
        if edge:
            shapes += [(S, 5) for S in edge]
        for S, n in shapes:
            label = "k=%d x=%d S=%d n=%d" % (k, x, S, n)
            idx, have, b, pos = body_batch(k, m, x, S, n)
            want = reference(k, m, x, S, idx, have)
            if x >= 2:
                mask = (1 << x) - 1 if pos < k else 1 << (pos - k)
                assert want[b] == mask | (int(idx[b, pos]) << 16), label
            else:
                assert want[b] == 1 | (UNLOCATED << 16), label
            assert np.count_nonzero(want) == 1, label
            run_check(codec, cases, label, k, m, x, S, n, idx, have, want)
    cases.done()

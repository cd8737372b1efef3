"""memo_ec_check_pair_batch on the MI355X: the check of k + x shards in hand,
and the two wrong shards of the blocks it leaves unlocated.  Every verdict
word is held bit for bit to the host reference (memo_amd/check_pair_ref.py:
check_pair_reference), which tests/test_check_pair_reference.py holds to what
was planted.  There is no tolerance.

Every buffer of every call sits between guards (tests/guarded.py): the index
rows, the shards and the verdict words, in device, pinned and pageable memory.

The first three tests bring the new launch up one thing at a time:
  test_1  a clean batch            check_pair_kernel finds no word to take
  test_2  one wrong shard          a located word: still nothing to take
  test_3  two wrong basis shards   RS(4,4), x = 4, S = 64, one block
The batches are those of tests/check_pair_cases.py: per shape a clean block,
two with one wrong shard, nine with two (basis + basis, basis + spare, spare +
spare; one byte each at the same offset -- rank 1 --, at bytes 0 and S - 1,
whole shards) and one with three.  A reference is computed once per batch."""
import functools

import numpy as np
import pytest

import check_pair_cases as C
from conftest import SEED
from guarded import Guarded
from test_check_pair_reference import AMBIGUOUS
from test_check_restated import INVALID, UNLOCATED
from test_gpu_bounds import Cases, rebuild_ref, sync

pytestmark = pytest.mark.gpu

ESINGULAR = -4


@functools.lru_cache(maxsize=None)
def wanted(shape, pick=None):
    """(idx, have, want) of C.batch(shape), or of its blocks `pick`."""
    k, m, x, S = shape
    idx, have, _ = C.batch(shape)
    if pick is not None:
        idx, have = idx[list(pick)], have[list(pick)]
    want = C.pair_reference(k, m, x, S, idx, have)
    want.setflags(write=False)
    return idx, have, want


def pairs_in(want):
    return int(np.count_nonzero((want != INVALID) & ((want >> 25) != 0)))


def run_pair(codec, cases, label, k, m, x, S, n, idx, have, want, memory="device", idx_shift=0):
    g = Guarded(memory)
    hi = g.input("have_idx", np.ascontiguousarray(idx, np.uint8).reshape(n, k + x), shift=idx_shift)
    hv = g.input("have", np.ascontiguousarray(have, np.uint8).reshape(n, (k + x) * S)) if S else None
    g.output("verdict", 4 * n)  # 0xA5A5A5A5 words: the call must write every one
    codec.check_pair(k, m, hi, hv, g.words("verdict"), x=x, S=S, n=n)
    sync(codec, memory)  # a pair, a mismatch and an invalid set are results, not errors
    cases.check(label, g, verdict=np.asarray(want, np.uint32))


def plain_check(codec, k, m, x, S, n, idx, have):
    """Codec.check's words of the same device buffers."""
    import torch
    hi = torch.from_numpy(np.ascontiguousarray(idx, np.uint8).reshape(n, k + x)).cuda()
    hv = torch.from_numpy(np.ascontiguousarray(have, np.uint8).reshape(n, (k + x) * S)).cuda()
    v = codec.check(k, m, hi, hv, x=x, S=S, n=n)
    codec.synchronize()
    return v.cpu().numpy().view(np.uint32)


# ---------------------------------------------------- 1-3: one new thing each
def test_1_clean_batch(codec):
    k, m, x, S, n = 10, 4, 4, 448, 70
    idx, have, _ = wanted((k, m, x, S), pick=(0,))
    idx, have = np.repeat(idx, n, axis=0), np.repeat(have, n, axis=0)
    want = np.zeros(n, np.uint32)
    assert np.array_equal(plain_check(codec, k, m, x, S, n, idx, have), want)
    cases = Cases()
    run_pair(codec, cases, "clean", k, m, x, S, n, idx, have, want)
    cases.done()


def test_2_one_block_one_wrong_shard(codec):
    k, m, x, S = 10, 4, 4, 448
    cases = Cases()
    for b in (1, 2):
        idx, have, want = wanted((k, m, x, S), pick=(b,))
        assert want[0] != 0 and want[0] >> 24 == 0 and (want[0] >> 16) & 0xFF != UNLOCATED
        assert np.array_equal(plain_check(codec, k, m, x, S, 1, idx, have), want)
        run_pair(codec, cases, C.kind(b), k, m, x, S, 1, idx, have, want)
    cases.done()


def test_3_one_block_two_wrong_basis_shards(codec):
    k, m, x, S = 4, 4, 4, 64
    cases = Cases()
    for b in (4, 3, 5):  # ends (rank 2), same offset (rank 1), whole shards
        idx, have, want = wanted((k, m, x, S), pick=(b,))
        assert pairs_in(want) == 1
        run_pair(codec, cases, C.kind(b), k, m, x, S, 1, idx, have, want)
    cases.done()


# ------------------------------------------------ 4: every shape, every memory
# S = 4160: a tile edge and more dwords than lanes; the "ends" blocks have their
# errors at byte 0 of one shard and byte S - 1 of the other, so different waves
# see v1 and v2.  (20,6,4): the KMAX = 64 body.
SHAPES = [(4, 4, 4, 64), (10, 4, 3, 448), (10, 4, 4, 4160), (10, 4, 3, 4160), (16, 4, 4, 64),
          (16, 4, 4, 4160), (20, 6, 4, 256), (7, 5, 5, 128)]
IDS = ["rs%d_%d_x%d_S%d" % s for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_4_shapes_on_the_device(codec, shape):
    k, m, x, S = shape
    idx, have, want = wanted(shape)
    assert pairs_in(want) >= (9 if x >= 4 else 6) and want[0] == 0
    assert want[12] != 0 and want[12] >> 16 == UNLOCATED  # three wrong shards
    cases = Cases()
    run_pair(codec, cases, "device", k, m, x, S, C.N, idx, have, want)
    cases.done()


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
@pytest.mark.parametrize("shape", [(10, 4, 4, 448), (20, 6, 4, 256)], ids=["rs10_4_x4_S448", "rs20_6_x4_S256"])
def test_4_host_memory(codec, shape, memory):
    k, m, x, S = shape
    idx, have, want = wanted(shape)
    cases = Cases()
    run_pair(codec, cases, memory, k, m, x, S, C.N, idx, have, want, memory=memory,
             idx_shift=1 if memory == "pageable" else 0)  # have_idx at an odd address
    cases.done()


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_4_host_memory_more_waves_than_pipeline_slots(codec, memory):
    """S = 32 KiB, 13 blocks, a 1 MiB pipeline batch: two blocks per wave,
    seven waves over the three slots."""
    shape = (10, 4, 4, 32768)
    k, m, x, S = shape
    idx, have, want = wanted(shape)
    assert pairs_in(want) == 9
    cases = Cases()
    with codec.options(pipe_bytes=1 << 20):
        run_pair(codec, cases, memory, k, m, x, S, C.N, idx, have, want, memory=memory,
                 idx_shift=1 if memory == "pageable" else 0)
    cases.done()


def test_4_the_limit_shape(codec):
    """RS(64,16), x = 16, S = 64, n = 3: 3160 pairs in the rank-1 search."""
    shape = (64, 16, 16, 64)
    k, m, x, S = shape
    idx, have, want = wanted(shape, pick=(3, 8, 12))  # bb/same (rank 1), bs/whole, three
    assert pairs_in(want) == 2 and want[2] >> 16 == UNLOCATED
    cases = Cases()
    run_pair(codec, cases, "limit", k, m, x, S, 3, idx, have, want)
    cases.done()


# --------------------------------------------- 5: one round, alternating blocks
def test_5_alternating_blocks_inside_one_round(codec):
    """S = 64, n = 70: clean, single and pair blocks in turn inside one
    64-word round of a workgroup, and a second round of six."""
    shape = (16, 4, 4, 64)
    k, m, x, S = shape
    idx13, have13, want13 = wanted(shape)
    n = 70
    sel = np.array([0 if b % 3 == 0 else 1 + (b // 3) % 2 if b % 3 == 1 else 3 + (b // 3) % 9 for b in range(n)])
    idx, have, want = idx13[sel], have13[sel], want13[sel]
    assert pairs_in(want) == len([b for b in range(n) if b % 3 == 2])
    cases = Cases()
    run_pair(codec, cases, "S=64 n=70", k, m, x, S, n, idx, have, want)
    cases.done()


# ------------------------------------------------------- 6: x = 3, two pairs
def test_6_x3_same_offset_blocks(codec):
    """The blocks of test_check_pair_reference's x = 3 test: some located,
    some left unlocated because two pairs explain them."""
    k, m, x, S, n, seed = AMBIGUOUS
    idx, have, _ = C.same_offset_blocks(k, m, x, S, n, seed)
    want = C.pair_reference(k, m, x, S, idx, have)
    assert 1 <= pairs_in(want) < n
    cases = Cases()
    run_pair(codec, cases, "x=3 rank 1", k, m, x, S, n, idx, have, want)
    cases.done()


# ------------------------------------------------------------ 7: invalid sets
@functools.lru_cache(maxsize=None)
def invalid_batch():
    shape = (10, 4, 4, 448)
    k, m, x, S = shape
    idx, have, _ = C.batch(shape)
    idx, have = idx.copy(), have.copy()
    idx[2, 7] = idx[2, 3]          # a repeat, between a single and a pair block
    idx[6, k + 1] = idx[6, 4]      # a pair block's own set made invalid
    idx[9, 0] = k + m              # an index past the code
    want = C.pair_reference(k, m, x, S, idx, have)
    assert (want[[2, 6, 9]] == INVALID).all() and pairs_in(want) == 7
    return idx, have, want


def test_7_invalid_sets_between_pair_blocks(codec):
    from memo_amd import ec
    import torch
    k, m, x, S = 10, 4, 4, 448
    idx, have, want = invalid_batch()
    cases = Cases()
    codec.synchronize()
    run_pair(codec, cases, "invalid sets", k, m, x, S, C.N, idx, have, want)  # its synchronize() raises nothing
    # a rebuild with a bad survivor set, then the pair check: the rebuild's
    # error is still pending afterwards, and the words are right
    s, l, surv, _ = rebuild_ref(k, m, S, 2, 5)
    s = s.copy()
    s[1, 3] = s[1, 0]
    out = torch.empty((5, 2 * S), dtype=torch.uint8, device="cuda")
    codec.rebuild(k, m, torch.from_numpy(s).cuda(), torch.from_numpy(surv.copy()).cuda(),
                  torch.from_numpy(l.copy()).cuda(), out)
    g = Guarded("device")
    hi = g.input("have_idx", idx)
    hv = g.input("have", have.reshape(C.N, -1))
    g.output("verdict", 4 * C.N)
    codec.check_pair(k, m, hi, hv, g.words("verdict"), x=x, S=S, n=C.N)
    with pytest.raises(ec.MemoECError) as err:
        codec.synchronize()
    assert err.value.code == ESINGULAR
    cases.check("after a singular rebuild", g, verdict=want)
    codec.synchronize()  # reported once
    cases.done()


# ------------------------------------------------------------ 8: several spans
def test_8_split_at_max_launch_tiles(codec):
    shape = (10, 4, 4, 4160)
    k, m, x, S = shape
    idx, have, want = wanted(shape)
    cases = Cases()
    with codec.options(max_launch_tiles=3):  # one block per MAC launch
        run_pair(codec, cases, "tiles=3", k, m, x, S, C.N, idx, have, want)
    cases.done()


# --------------------------------------------- 9: back to back on one scratch
def test_9_pair_check_plain_check_and_rebuild_without_a_synchronize(codec):
    """A pair check, a plain check of the same buffers, a rebuild and a pair
    check of another geometry, one synchronize at the end: they share the
    ctx's scratch and are ordered by the stream alone."""
    from memo_amd import check_ref as R
    sa, sb = (10, 4, 4, 448), (20, 6, 4, 256)
    ia, ha, wa = wanted(sa)
    ib, hb, wb = wanted(sb)
    plain = R.check_reference(sa[0], sa[1], ia, ha.reshape(C.N, -1))
    assert not np.array_equal(plain, wa)
    rk, rm, rS, re, rn = 10, 4, 4160, 4, 5
    s, l, surv, lost = rebuild_ref(rk, rm, rS, re, rn)
    g = Guarded("device")
    a_idx, a_have = g.input("a.have_idx", ia), g.input("a.have", ha.reshape(C.N, -1))
    b_idx, b_have = g.input("b.have_idx", ib), g.input("b.have", hb.reshape(C.N, -1))
    g.output("a.pair", 4 * C.N)
    g.output("a.plain", 4 * C.N)
    g.output("b.pair", 4 * C.N)
    r_s, r_l, r_surv = g.input("r.surv_idx", s), g.input("r.lost_idx", l), g.input("r.surv", surv)
    r_out = g.output("r.out", (rn, re * rS))
    with codec.options(rebuild_path=0, image_min_tiles=0):
        codec.check_pair(sa[0], sa[1], a_idx, a_have, g.words("a.pair"), x=sa[2], S=sa[3], n=C.N)
        codec.check(sa[0], sa[1], a_idx, a_have, g.words("a.plain"), x=sa[2], S=sa[3], n=C.N)
        codec.rebuild(rk, rm, r_s, r_surv, r_l, r_out)
        codec.check_pair(sb[0], sb[1], b_idx, b_have, g.words("b.pair"), x=sb[2], S=sb[3], n=C.N)
        codec.synchronize()
    cases = Cases()
    cases.check("back to back", g, **{"a.pair": wa, "a.plain": plain, "b.pair": wb, "r.out": lost})
    cases.done()


# ------------------------------------------------------- 10: x <= 2, and S = 0
@pytest.mark.parametrize("x", [1, 2])
def test_10_x_below_three_is_the_check(codec, x):
    from memo_amd import check_ref as R
    k, m, S = 10, 4, 448
    idx, have, _ = C.batch((k, m, 4, S))
    idx = np.ascontiguousarray(idx[:, :k + x])
    have = np.ascontiguousarray(have[:, :k + x])
    want = R.check_reference(k, m, idx, have.reshape(C.N, -1))
    assert np.count_nonzero(want) >= 6
    assert np.array_equal(plain_check(codec, k, m, x, S, C.N, idx, have), want)
    cases = Cases()
    run_pair(codec, cases, "x=%d" % x, k, m, x, S, C.N, idx, have, want)
    cases.done()


def test_10_index_sets_alone(codec):
    """S = 0: only the sets are judged; `have` NULL."""
    k, m, x = 10, 4, 4
    idx, _, _ = invalid_batch()
    want = np.zeros(C.N, np.uint32)
    want[[2, 6, 9]] = INVALID
    cases = Cases()
    run_pair(codec, cases, "S=0", k, m, x, 0, C.N, idx, None, want)
    cases.done()

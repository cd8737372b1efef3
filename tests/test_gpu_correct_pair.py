"""memo_ec_correct_pair_batch on the MI355X: the pair check of any k + x shards
in hand and, on the device, every block with one or two wrong shards mended.
Words are held bit for bit and every byte of `have` byte for byte to
memo_amd/correct_pair_ref.py -- and, where whole shards were overwritten, to
the original bytes and the analytic word as well.  There is no tolerance.

Every buffer of every call sits between guards (tests/guarded.py): the index
rows, the shards -- read and written here, so their payload is judged against
the bytes expected after the call, and everything the call must leave alone
is held to what was put in -- and the verdict words, in device, pinned and
pageable memory.

The first tests run the call's two new kernels on the narrowest inputs that
reach them, one new thing each:
  test_1a  a clean batch         both new kernels launch and find nothing
  test_1b  single blocks only    the result is Codec.correct's
  test_1c  one pair block each   ss, bs with clean row 1 (r = 0), bs with
                                 clean row 0, bb
Every shape here is walked on the CPU first (tests/test_correct_pair_plan.py)."""
import functools

import numpy as np
import pytest

import correct_pair_cases as CP
from conftest import SEED
from correct_cases import clean_batch, overwrite, single_batch
from correct_pair_cases import CORRECTED, INVALID
from guarded import Guarded
from test_gpu_bounds import Cases, rebuild_ref, sync
from test_gpu_correct import inout

pytestmark = pytest.mark.gpu

ESINGULAR = -4
UNLOCATED = 0xFF


def reference(k, m, x, S, idx, have):
    from memo_amd import correct_pair_ref as R
    n = np.asarray(idx).reshape(-1, k + x).shape[0]
    return R.correct_pair_reference(k, m, idx, np.asarray(have).reshape(n, -1), x=x, S=S)


def held_to_reference(k, m, x, S, idx, have, words, after, blocks):
    """The analytic expectation of `blocks` is the reference's."""
    blocks = list(blocks)
    w, a = reference(k, m, x, S, np.asarray(idx)[blocks], np.asarray(have)[blocks])
    assert np.array_equal(w, np.asarray(words)[blocks])
    assert np.array_equal(a, np.asarray(after).reshape(-1, k + x, S)[blocks])


def run_pair(codec, cases, label, k, m, x, S, n, idx, have, words, after, memory="device", idx_shift=0):
    g = Guarded(memory)
    hi = g.input("have_idx", np.ascontiguousarray(idx, np.uint8).reshape(n, k + x), shift=idx_shift)
    hv = inout(g, "have", np.asarray(have).reshape(n, (k + x) * S)) if S else None
    g.output("verdict", 4 * n)  # 0xA5A5A5A5 words: the call must write every one
    codec.correct_pair(k, m, hi, hv, g.words("verdict"), x=x, S=S, n=n)
    sync(codec, memory)  # a correction is a result, not an error
    want = {"verdict": np.asarray(words, np.uint32)}
    if S:
        want["have"] = np.asarray(after, np.uint8).reshape(n, (k + x) * S)
    cases.check(label, g, **want)


def run_planted(codec, cases, label, shape, targets, memory="device", idx_shift=0, seed=0, sample=None):
    """Whole shards overwritten in the target blocks: the original bytes come
    back and the words are the analytic ones, which the reference confirms on
    `sample` (default: every block)."""
    k, m, x, S, n = shape
    idx, clean, have, words = CP.pair_batch(shape, tuple(targets), seed)
    held_to_reference(k, m, x, S, idx, have, words, clean, range(n) if sample is None else sample)
    run_pair(codec, cases, label, k, m, x, S, n, idx, have, words, clean, memory, idx_shift)


# ------------------------------------------------------------------ 1: bring-up
def test_1a_clean_batch(codec):
    k, m, x, S, n = CP.CLEAN
    idx, have = clean_batch(k, m, x, S, n, SEED + 201)
    cases = Cases()
    run_pair(codec, cases, "clean", k, m, x, S, n, idx, have, np.zeros(n, np.uint32), have)
    cases.done()


def test_1b_single_blocks_only(codec):
    """One wrong shard in every other block: the bytes and words of
    Codec.correct, which are the reference's."""
    import torch
    shape = CP.SINGLES
    k, m, x, S, n = shape
    idx, clean, have, words = single_batch(shape, tuple((b, (3 * b) % (k + x)) for b in range(0, n, 2)))
    held_to_reference(k, m, x, S, idx, have, words, clean, range(n))
    hi = torch.from_numpy(np.array(idx)).cuda()
    hv = torch.from_numpy(np.array(have).reshape(n, -1)).cuda()
    v = codec.correct(k, m, hi, hv, x=x, S=S, n=n)
    codec.synchronize()
    assert np.array_equal(v.cpu().numpy().view(np.uint32), words)
    assert np.array_equal(hv.cpu().numpy().reshape(clean.shape), clean)
    cases = Cases()
    run_pair(codec, cases, "singles", k, m, x, S, n, idx, have, words, clean)
    cases.done()


@pytest.mark.parametrize("pair", [(5, 7), (1, 4), (2, 6), (0, 3)], ids=["ss", "bs_r0", "bs_r2", "bb"])
def test_1c_one_pair_block(codec, pair):
    k, m, x, S = CP.BRINGUP
    cases = Cases()
    run_planted(codec, cases, "pair %d,%d" % pair, (k, m, x, S, 1), [(0,) + pair], seed=pair[0])
    cases.done()


# ------------------------------------------------ 2: the 13-block batches, every memory
@pytest.mark.parametrize("memory", ["device", "pinned", "pageable"])
@pytest.mark.parametrize("shape", CP.BATCHES, ids=["rs%d_%d_x%d_S%d" % s for s in CP.BATCHES])
def test_2_batches_in_every_memory(codec, shape, memory):
    """clean / one basis / one spare / nine pair blocks / three wrong."""
    k, m, x, S = shape
    idx, clean, have, truth = CP.batch(shape)
    words, after = CP.batch_reference(shape)
    for b in (1, 2) + tuple(range(3, 12)):
        if (int(words[b]) >> 24) & 1:
            assert np.array_equal(after[b], clean[b]), b
    assert (int(words[5]) >> 25) and (int(words[8]) >> 25) and (int(words[11]) >> 25)  # "whole": always a pair
    cases = Cases()
    run_pair(codec, cases, memory, k, m, x, S, CP.N, idx, have, words, after, memory=memory,
             idx_shift=0 if memory == "device" else 1)
    cases.done()


# ------------------------------------------------------------ 3: every pair of positions
@pytest.mark.parametrize("shape", CP.EVERY_PAIR, ids=["rs%d_%d_x%d_S%d" % s for s in CP.EVERY_PAIR])
def test_3_every_pair_of_positions(codec, shape):
    k, m, x, S = shape
    pairs = CP.every_pair(k, x)
    cases = Cases()
    run_planted(codec, cases, "every pair", shape + (len(pairs),), [(b,) + p for b, p in enumerate(pairs)])
    cases.done()


def test_3_widest_code(codec):
    """RS(64,16), x = 16: 80 positions, pairs around 31/32, 63/64 and 79."""
    k, m, x, S = CP.WIDE
    cases = Cases()
    run_planted(codec, cases, "wide", CP.WIDE + (len(CP.WIDE_PAIRS),),
                [(b,) + p for b, p in enumerate(CP.WIDE_PAIRS)], sample=(0, 3, 5, 11))
    cases.done()


# ------------------------------------------------------------ 4: every compiled KC
@pytest.mark.parametrize("KC", CP.KCS, ids=["kc%d" % KC for KC in CP.KCS])
def test_4_every_compiled_chunk(codec, KC):
    """gf_correct_pair_kernel<KC> with k == KC, and under KC = 4 the chunk loop
    at k = 5 (a tail of one shard), 33 and 64."""
    from memo_amd import ec
    cases = Cases()
    for k in CP.KC_CODES[KC]:
        assert ec.mac_kchunk(k, 2) == KC
        pairs = CP.kc_pairs(k, CP.KC_M)
        run_planted(codec, cases, "k=%d" % k, (k, CP.KC_M, CP.KC_M, CP.KC_S, len(pairs)),
                    [(b,) + p for b, p in enumerate(pairs)], sample=(0, 1, 2, 4) if k > 16 else None)
    cases.done()


# ------------------------------------------------------------------ 5: tile edges
@pytest.mark.parametrize("shape", CP.EDGES, ids=["rs%d_%d_x%d_S%d" % s for s in CP.EDGES])
def test_5_tile_edges(codec, shape):
    """S = 4160: a full tile and a 64-byte tail (4 active lanes); S = 64: 4
    active lanes in all.  The targets first and last of basis and of spares;
    two clean blocks behind them."""
    k, m, x, S = shape
    pairs = CP.edge_pairs(k, x)
    cases = Cases()
    run_planted(codec, cases, "edges", shape + (len(pairs) + 2,), [(b,) + p for b, p in enumerate(pairs)])
    cases.done()


# ---------------------------------------------------------------- 6: ranges and list
def test_6_item_ranges_inside_entries(codec):
    """RS(3,3), x = 3, S = 8256: 700 pair blocks of 3 tiles, 2100 items over
    2048 workgroups."""
    k, m, x, S, n = CP.RANGES
    pairs = CP.every_pair(k, x)
    cases = Cases()
    run_planted(codec, cases, "ranges", CP.RANGES, [(b,) + pairs[b % len(pairs)] for b in range(n)],
                sample=range(0, n, 47))
    cases.done()


@functools.lru_cache(maxsize=None)
def list_batch():
    """n = 1024 * 256 + 259 blocks of RS(4,4), x = 4, S = 64, tiled from 256
    clean ones: the list kernel's grid takes a second round.  Pair blocks at
    the boundaries of both rounds, a whole wave of 64, and waves whose lane 63
    alone holds one (in both rounds)."""
    k, m, x, S, n = CP.LIST
    idx0, clean0 = clean_batch(k, m, x, S, 256, SEED + 301)
    reps = -(-n // 256)
    idx = np.tile(idx0, (reps, 1))[:n]
    clean = np.tile(clean0, (reps, 1, 1))[:n]
    r2 = 1024 * 256
    blocks = sorted({0, 255, 256, r2 - 1, r2, r2 + 255, r2 + 256, n - 1, 2048 + 63, r2 + 64 + 63}
                    | set(range(1024, 1088)))
    pairs = CP.every_pair(k, x)
    rng = np.random.default_rng(SEED + 302)
    have = clean.copy()
    words = np.zeros(n, np.uint32)
    for i, b in enumerate(blocks):
        qa, qb = pairs[i % len(pairs)]
        overwrite(have, b, qa, rng)
        overwrite(have, b, qb, rng)
        words[b] = CP.pair_word(idx, b, qa, qb, k, x)
    held_to_reference(k, m, x, S, idx, have, words, clean, blocks + [1, 257, r2 + 1])
    return idx, clean, have, words


def test_6_list_kernel_second_round(codec):
    k, m, x, S, n = CP.LIST
    idx, clean, have, words = list_batch()
    cases = Cases()
    run_pair(codec, cases, "list", k, m, x, S, n, idx, have, words, clean)
    cases.done()


# ------------------------------------------------------------------ 7: mixed words
@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Pair, single, clean, unlocated (three whole shards) and invalid blocks
    alternating inside one 64-word round."""
    k, m, x, S, n = CP.MIXED
    idx, clean = clean_batch(k, m, x, S, n, SEED + 401)
    idx, have = idx.copy(), clean.copy()
    rng = np.random.default_rng(SEED + 402)
    pairs = CP.every_pair(k, x)
    for b in range(n):
        kind = b % 5
        if kind == 0:
            for q in pairs[(7 * b) % len(pairs)]:
                overwrite(have, b, q, rng)
        elif kind == 1:
            overwrite(have, b, (3 * b) % (k + x), rng)
        elif kind == 3:
            for q in rng.choice(k + x, size=3, replace=False):
                overwrite(have, b, int(q), rng)
        elif kind == 4:
            idx[b, (b + 1) % (k + x)] = idx[b, b % (k + x)]
            have[b, 2, 9] ^= 0xFF  # an invalid block's bytes are never judged or written
    words, after = reference(k, m, x, S, idx, have)
    for b in range(n):
        kind = b % 5
        w = int(words[b])
        if kind == 0:
            assert (w >> 25) and (w >> 24) & 1 and np.array_equal(after[b], clean[b])
        elif kind == 1:
            assert (w >> 24) == 1 and np.array_equal(after[b], clean[b])
        elif kind == 2:
            assert w == 0
        elif kind == 3:
            assert (w >> 16) == UNLOCATED and np.array_equal(after[b], have[b])
        else:
            assert w == INVALID and np.array_equal(after[b], have[b])
    return idx, have, words, after


@pytest.mark.parametrize("memory", ["device", "pageable"])
def test_7_mixed_words_in_one_round(codec, memory):
    k, m, x, S, n = CP.MIXED
    idx, have, words, after = mixed_batch()
    cases = Cases()
    run_pair(codec, cases, "mixed", k, m, x, S, n, idx, have, words, after, memory=memory,
             idx_shift=0 if memory == "device" else 1)
    cases.done()


# ------------------------------------------------------ 8: several pipeline waves
@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_8_host_memory_several_pipeline_waves(codec, memory):
    """RS(10,4), x = 4, S = 32 KiB, n = 9 with a 1 MiB pipeline batch: two
    blocks per wave, five waves over the three slots; a pair block last in
    each wave, and a single block first in two of them."""
    k, m, x, S, n = CP.WAVES
    idx, clean, have, words = CP.pair_batch(CP.WAVES, ((1, 0, k), (3, 2, 5), (5, k, k + 3), (7, k - 1, k + x - 1),
                                                       (8, 4, k + 1)))
    have, words = have.copy(), words.copy()
    rng = np.random.default_rng(SEED + 501)
    for b, q in ((0, k + 1), (4, 3)):
        overwrite(have, b, q, rng)
        words[b] = ((1 << x) - 1 if q < k else 1 << (q - k)) | (int(idx[b, q]) << 16) | CORRECTED
    held_to_reference(k, m, x, S, idx, have, words, clean, (0, 1, 4))
    cases = Cases()
    with codec.options(pipe_bytes=1 << 20):
        run_pair(codec, cases, memory, k, m, x, S, n, idx, have, words, clean, memory=memory,
                 idx_shift=1 if memory == "pageable" else 0)
    cases.done()


# ------------------------------------------------------------- 9: launch splitting
def test_9_split_at_max_launch_tiles(codec):
    k, m, x, S, n = CP.SPLIT
    cases = Cases()
    with codec.options(max_launch_tiles=3):  # the check: one block per launch
        run_planted(codec, cases, "tiles=3", CP.SPLIT, ((1, 0, k + 1), (3, k, k + 2), (4, 2, k - 1)))
    cases.done()


# ----------------------------------------------- 10: back to back on one scratch
def test_10_back_to_back_without_a_synchronize(codec):
    """correct_pair, a check of the same buffers, a rebuild with a bad survivor
    set, correct_pair again, one synchronize: the check and the second
    correct_pair find the mended blocks clean, and the rebuild's ESINGULAR is
    still reported afterwards."""
    import torch
    from memo_amd import check_ref, ec
    k, m, x, S, n = CP.BACK
    idx, clean, have, truth = CP.batch((k, m, x, S))
    words, after = CP.batch_reference((k, m, x, S))
    second = check_ref.check_reference(k, m, idx, after, x=x, S=S)
    third, after3 = reference(k, m, x, S, idx, after)
    assert not second[:12].any() and second[12] and np.array_equal(third, second) and np.array_equal(after3, after)
    rk, rm, rS, rn = 10, 4, 448, 5
    s, l, surv, _ = rebuild_ref(rk, rm, rS, 2, rn)
    s = s.copy()
    s[1, 3] = s[1, 0]
    r_out = torch.empty((rn, 2 * rS), dtype=torch.uint8, device="cuda")
    r_s, r_surv, r_l = (torch.from_numpy(a.copy()).cuda() for a in (s, surv, l))
    g = Guarded("device")
    hi = g.input("have_idx", idx)
    hv = inout(g, "have", have.reshape(n, -1))
    for name in ("first", "second", "third"):
        g.output(name, 4 * n)
    codec.synchronize()
    codec.correct_pair(k, m, hi, hv, g.words("first"), x=x, S=S, n=n)
    codec.check(k, m, hi, hv, g.words("second"), x=x, S=S, n=n)
    codec.rebuild(rk, rm, r_s, r_surv, r_l, r_out)
    codec.correct_pair(k, m, hi, hv, g.words("third"), x=x, S=S, n=n)
    with pytest.raises(ec.MemoECError) as err:
        codec.synchronize()
    assert err.value.code == ESINGULAR
    cases = Cases()
    cases.check("back to back", g, have=after.reshape(n, -1), first=words, second=second, third=third)
    codec.synchronize()  # reported once
    cases.done()


# ------------------------------------------------------------------ 11: equalities
def device_call(codec, fn, k, m, x, S, n, idx, have):
    import torch
    hi = torch.from_numpy(np.array(idx, np.uint8)).cuda()
    hv = torch.from_numpy(np.array(have, np.uint8).reshape(n, -1)).cuda() if S else None
    v = fn(k, m, hi, hv, x=x, S=S, n=n)
    codec.synchronize()
    return v.cpu().numpy().view(np.uint32), (hv.cpu().numpy() if S else None)


@pytest.mark.parametrize("shape", CP.LOW_X, ids=["x2", "x1"])
def test_11_x_up_to_2_is_correct(codec, shape):
    k, m, x, S, n = shape
    idx, clean, have, _ = single_batch(shape, tuple((b, (5 * b) % (k + x)) for b in range(1, n - 2, 2)))
    have = have.copy()
    rng = np.random.default_rng(SEED + 601)
    overwrite(have, n - 1, 0, rng)
    overwrite(have, n - 1, k, rng)  # two wrong shards: no pair can be named with x <= 2
    words, after = device_call(codec, codec.correct, k, m, x, S, n, idx, have)
    rw, ra = reference(k, m, x, S, idx, have)
    assert np.array_equal(rw, words) and np.array_equal(ra.reshape(n, -1), after)
    cases = Cases()
    run_pair(codec, cases, "x=%d" % x, k, m, x, S, n, idx, have, words, after)
    cases.done()


def test_11_S_0_is_the_check(codec):
    k, m, x, n = 10, 4, 4, 24
    idx, _ = clean_batch(k, m, x, 64, n, SEED + 602)
    idx = idx.copy()
    idx[2, 7] = idx[2, 3]
    idx[23, k] = 255
    words, _ = device_call(codec, codec.check, k, m, x, 0, n, idx, None)
    assert [int(w) for w in words[[0, 2, 23]]] == [0, INVALID, INVALID]
    cases = Cases()
    run_pair(codec, cases, "S=0", k, m, x, 0, n, idx, None, words, None)
    cases.done()


@pytest.mark.parametrize("km", CP.IDENTITY, ids=lambda p: "rs%d_%d" % p)
def test_11_identity_set_and_verify(codec, km):
    """have_idx = 0..k+m-1, x = m: a single block's word is verify's with bit
    24, a pair block's mask is verify's (which leaves it unlocated)."""
    import torch
    k, m = km
    S, n = 128, 16
    from test_check_restated import shards_of
    rng = np.random.default_rng(SEED ^ (k * 139 + m))
    clean = shards_of(CP.PC.oracle(), k, m, S, rng, n)
    full = clean.copy()
    pairs = CP.every_pair(k, m)
    for b in range(1, n):
        if b % 3 == 1:
            overwrite(full, b, (3 * b) % (k + m), rng)
        elif b % 3 == 2:
            for q in pairs[(11 * b) % len(pairs)]:
                overwrite(full, b, q, rng)
    ident = np.tile(np.arange(k + m, dtype=np.uint8), (n, 1))
    d = torch.from_numpy(np.ascontiguousarray(full[:, :k]).reshape(n, k * S)).cuda()
    p = torch.from_numpy(np.ascontiguousarray(full[:, k:]).reshape(n, m * S)).cuda()
    v = codec.verify(k, m, d, p)
    codec.synchronize()
    v = v.cpu().numpy().view(np.uint32)
    words, after = reference(k, m, m, S, ident, full)
    for b in range(n):
        if b % 3 == 0:
            assert v[b] == 0 and words[b] == 0
        elif b % 3 == 1:
            assert words[b] == v[b] | CORRECTED and (int(v[b]) >> 16) != UNLOCATED
        else:
            assert (int(v[b]) >> 16) == UNLOCATED and (int(words[b]) & 0xFFFF) == (int(v[b]) & 0xFFFF)
            assert (int(words[b]) >> 25) and (int(words[b]) >> 24) & 1
    assert np.array_equal(after, clean)
    cases = Cases()
    run_pair(codec, cases, "identity", k, m, m, S, n, ident, full, words, clean)
    cases.done()


# ------------------------------------------------------------------ 12: mislocation
def test_12_three_wrong_shards_that_pass_for_two(codec):
    """The block of tests/test_correct_pair_reference.py's mislocation test:
    the device overwrites the same two (right) shards with the same bytes."""
    k, m, x, S = CP.MISLOCATION
    idx, clean, have, (d, e), wrong = CP.mislocation_block(k, m, x, S)
    words, after = reference(k, m, x, S, idx, have)
    lo, hi = sorted((int(idx[0, d]), int(idx[0, e])))
    assert (int(words[0]) >> 16) & 0xFF == lo and (int(words[0]) >> 25) - 1 == hi and (int(words[0]) >> 24) & 1
    assert not np.array_equal(after, clean) and not np.array_equal(after, have)
    cases = Cases()
    run_pair(codec, cases, "mislocated", k, m, x, S, 1, idx, have, words, after)
    cases.done()

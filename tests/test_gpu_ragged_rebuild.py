"""Ragged rebuild on the MI355X (memo_ec_rebuild_ragged: the decode kernels
and gf_mac_ragged_rows_kernel for per-block patterns, gf_mac_ragged_kernel
over a pattern's table image for a shared one).

A ragged batch packs blocks of their own shard sizes back to back: survivor
t of block b at k * off[b] + t * S[b], rebuilt shard r at e * off[b] +
r * S[b].  The judge is the oracle's rebuild of each block on its own
(O.rebuild, one block per call), bit for bit.  Every buffer is guarded
(tests/guarded.py).

Size lists (shard bytes; a tile is 4096): tests/ragged_cases.py, plus
  G      zero-size blocks inside tiles, so a tile's table sets are not the
         rows of consecutive caller blocks
  H(c)   c blocks of 64 bytes and one of two tiles, c = cap - 1, cap, cap + 1,
         where cap is the number of table sets a tile may build for the
         code: the first tile is short of, at and past the cap (at cap = 64,
         the most blocks 256 columns hold, Hp's 65th block opens tile 1)
cap() restates the planner's bound (memo_ec.cpp ragged_rows_cap) over the
constants read from the sources.  It only chooses inputs and judges nothing.
"""
import numpy as np
import pytest

from conftest import SEED
from guarded import FILL, Guarded
import mac_bodies as MB
import ragged_cases as RC

pytestmark = pytest.mark.gpu

ESINGULAR, EINVAL = -4, -1
G = [64, 0, 0, 128, 0, 64, 0, 4160, 0, 0, 64]

# (k, m) -> the e each runs
CODES = {(3, 2): (1, 2), (10, 4): (1, 4), (16, 4): (2, 4), (5, 3): (3,), (20, 8): (5, 8), (6, 6): (6,)}
HS = {"Hm": -1, "H0": 0, "Hp": 1}


def cap(k, e):
    c = MB.constants()
    per = MB.body(k, e)[1] * MB.kpad(k, e)
    return max(1, min(64, MB.LANES * c["MAC_COEF_REGS"] // per, c["kLdsBudget"] // ((per + 1) * 20)))


def sizes_of(name, k, e):
    if name == "G":
        return G
    if name in HS:
        return [64] * (cap(k, e) + HS[name]) + [8192]
    return RC.LISTS[name]


CASES = [(name, k, m, e) for (k, m), es in CODES.items() for e in es
         for name in list(RC.LISTS) + ["G"] + list(HS)] + \
        [(name, 64, 16, 16) for name in ["A", "C", "D"] + list(HS)]
CASE_IDS = ["%s_rs%d_%d_e%d" % c for c in CASES]

_CLEAN = {}


def patterns(rng, n, k, m, e):
    """A different seeded pattern per block: e lost shards and k survivors in
    shuffled order, data and parity shards on both sides."""
    sidx = np.zeros((n, k), dtype=np.uint8)
    lidx = np.zeros((n, e), dtype=np.uint8)
    for b in range(n):
        p = rng.permutation(k + m)
        lidx[b] = p[:e]
        sidx[b] = p[e:e + k]
    return sidx, lidx


def judge(O, k, m, sizes, sidx, surv, lidx, faulty=()):
    """O.rebuild of each block on its own; a faulty block's bytes are zero."""
    e = lidx.shape[1]
    off = RC.offsets(sizes)
    want = np.zeros(e * off[-1], dtype=np.uint8)
    for b, S in enumerate(sizes):
        if S and b not in faulty:
            s = surv[k * off[b]:k * off[b] + k * S].reshape(1, k * S)
            want[e * off[b]:e * off[b] + e * S] = O.rebuild(k, m, S, sidx[b:b + 1], s, lidx[b:b + 1]).reshape(-1)
    return want


def clean(O, name, k, m, e):
    """(sizes, sidx, lidx, surv k*T, want e*T) of a list and code: seeded
    survivors and patterns, the oracle's rebuild of each block; computed
    once, never written."""
    key = (name, k, m, e)
    if key not in _CLEAN:
        sizes = sizes_of(name, k, e)
        T = sum(sizes)
        rng = np.random.default_rng(SEED ^ (k * 1000003 + m * 10007 + e * 101 + T))
        sidx, lidx = patterns(rng, len(sizes), k, m, e)
        surv = rng.integers(0, 256, size=k * T, dtype=np.uint8)
        want = judge(O, k, m, sizes, sidx, surv, lidx)
        for a in (sidx, lidx, surv, want):
            a.setflags(write=False)
        _CLEAN[key] = (sizes, sidx, lidx, surv, want)
    return _CLEAN[key]


def run(codec, sizes, k, m, sidx, surv, lidx, memory="device", uniform=False, nbytes=None):
    """One rebuild_ragged over guarded buffers; the indices live where the
    shards do (host sequences for a shared pattern)."""
    e = len(lidx) if uniform else lidx.shape[1]
    g = Guarded(memory)
    s = g.input("surv", surv)
    o = g.output("out", e * sum(sizes) if nbytes is None else nbytes)
    if uniform:
        si, li = sidx, lidx
    else:
        si = g.input("surv_idx", sidx, shift=3)   # any byte alignment
        li = g.input("lost_idx", lidx, shift=1)
    assert codec.rebuild_ragged(k, m, sizes, si, s, li, o, uniform=uniform) is o
    return g


def checked(codec, O, name, k, m, e, memory="device"):
    sizes, sidx, lidx, surv, want = clean(O, name, k, m, e)
    g = run(codec, sizes, k, m, sidx, surv, lidx, memory)
    codec.synchronize()
    g.check(out=want)


def sync_code(codec):
    from memo_amd import ec
    try:
        codec.synchronize()
    except ec.MemoECError as ex:
        return ex.code
    return 0


# ------------------------------------------------------- per-block patterns

@pytest.mark.parametrize("name,k,m,e", CASES, ids=CASE_IDS)
def test_rebuild_matches_the_oracle_block_by_block(codec, O, name, k, m, e):
    checked(codec, O, name, k, m, e)


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
@pytest.mark.parametrize("name", ["C", "E", "G"])
@pytest.mark.parametrize("k,m,e", [(10, 4, 4), (16, 4, 2), (5, 3, 3)])
def test_rebuild_from_host_memory(codec, O, name, k, m, e, memory):
    checked(codec, O, name, k, m, e, memory)


@pytest.mark.parametrize("name", ["F1", "F2"])
@pytest.mark.parametrize("k,m,e", [(k, m, e) for (k, m), es in CODES.items() for e in es])
def test_uniform_sizes_equal_rebuild_batch(codec, O, name, k, m, e):
    """On equal sizes the call writes byte for byte what Codec.rebuild writes
    from the same buffers."""
    import torch
    sizes, sidx, lidx, surv, want = clean(O, name, k, m, e)
    n, S = len(sizes), sizes[0]
    g = Guarded()
    s = g.input("surv", surv)
    si, li = g.input("surv_idx", sidx), g.input("lost_idx", lidx)
    o1 = g.output("ragged", want.size)
    o2 = g.output("batch", want.size)
    codec.rebuild_ragged(k, m, sizes, si, s, li, o1)
    codec.rebuild(k, m, si, s.view(n, k * S), li, o2.view(n, e * S))
    codec.synchronize()
    assert torch.equal(o1, o2)
    g.check(ragged=want, batch=want)


# ----------------------------------------------------------- shared pattern

def shared(O, name, k, m, e):
    sizes, _, _, surv, _ = clean(O, name, k, m, e)
    rng = np.random.default_rng(SEED + 17 * k + e)
    p = rng.permutation(k + m)
    lu, su = p[:e].astype(np.uint8), p[e:e + k].astype(np.uint8)
    n = len(sizes)
    want = judge(O, k, m, sizes, np.tile(su, (n, 1)), surv, np.tile(lu, (n, 1)))
    return sizes, su, lu, surv, want


@pytest.mark.parametrize("name", ["C", "E", "F2"])
@pytest.mark.parametrize("k,m,e", [(10, 4, 1), (10, 4, 4), (16, 4, 2), (16, 4, 4)])
def test_shared_pattern(codec, O, name, k, m, e):
    import torch
    sizes, su, lu, surv, want = shared(O, name, k, m, e)
    g = run(codec, sizes, k, m, su, surv, lu, uniform=True)
    if name == "F2":  # byte-identical to rebuild_uniform on the same buffers
        n, S = len(sizes), sizes[0]
        o2 = g.output("uniform", want.size)
        codec.rebuild_uniform(k, m, su, g.bufs["surv"].view().view(n, k * S), lu, o2.view(n, e * S))
        codec.synchronize()
        assert torch.equal(g.bufs["out"].view(), o2)
        g.check(out=want, uniform=want)
    else:
        codec.synchronize()
        g.check(out=want)


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_shared_pattern_from_host_memory(codec, O, memory):
    sizes, su, lu, surv, want = shared(O, "C", 10, 4, 4)
    g = run(codec, sizes, 10, 4, su, surv, lu, memory, uniform=True)
    g.check(out=want)


# ------------------------------------------------- launch spans and waves

@pytest.mark.parametrize("limit", [1, 3])
@pytest.mark.parametrize("name", ["C", "E", "H0"])
def test_launch_split_on_block_boundaries(codec, O, name, limit):
    """max_launch_tiles 1 and 3: spans cut on block boundaries by the capped
    tile count, a block of more tiles than the limit in a launch of its own."""
    with codec.options(max_launch_tiles=limit):
        checked(codec, O, name, 10, 4, 4)
        checked(codec, O, name, 16, 4, 4)


@pytest.mark.parametrize("name", ["E", "H0", "A"])
def test_xcd_tile_order(codec, O, name):
    with codec.options(xcd_min_tiles=1):
        checked(codec, O, name, 10, 4, 4)


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
def test_host_pipeline_waves_cut_by_bytes(codec, O, memory):
    """E from host memory with zero-copy off and the smallest pipe_bytes the
    option takes (1 MiB; (k + e) * T is about 11 MiB: many waves, cut on
    block boundaries, each with its slice of the pattern bytes)."""
    k, m, e = 10, 4, 4
    sizes = clean(O, "E", k, m, e)[0]
    assert (k + e) * sum(sizes) > 3 << 20
    with codec.options(zero_copy_bytes=0, pipe_bytes=1 << 20):
        checked(codec, O, "E", k, m, e, memory)
        sz, su, lu, surv, want = shared(O, "E", k, m, e)
        g = run(codec, sz, k, m, su, surv, lu, memory, uniform=True)
        g.check(out=want)


def test_back_to_back_calls_need_no_synchronize(codec, O):
    """Two calls with different size lists on one ctx, no synchronize in
    between: the first call's index and decode rows must outlive the second
    call's staging."""
    k, m, e = 10, 4, 4
    sc, ic, lc, vc, wc = clean(O, "C", k, m, e)
    sa, ia, la, va, wa = clean(O, "A", k, m, e)
    gc = run(codec, sc, k, m, ic, vc, lc)
    ga = run(codec, sa, k, m, ia, va, la)
    codec.synchronize()
    gc.check(out=wc)
    ga.check(out=wa)


# ------------------------------------------------------------------- faults

def faulted(O, name, k, m, e):
    """The clean case with one block given a duplicate survivor index,
    another an index >= k + m and (C) a zero-size block a bad pattern."""
    sizes, sidx, lidx, surv, _ = clean(O, name, k, m, e)
    sidx, lidx = sidx.copy(), lidx.copy()
    real = [b for b, S in enumerate(sizes) if S]
    dup, big = real[1], real[len(real) // 2 + 1]
    assert dup != big
    sidx[dup, k - 1] = sidx[dup, 0]
    sidx[big, 2] = k + m
    faulty = {dup, big}
    if name == "C":
        zero = sizes.index(0)
        sidx[zero, :] = 0
        faulty.add(zero)
    return sizes, sidx, lidx, surv, judge(O, k, m, sizes, sidx, surv, lidx, faulty), faulty


@pytest.mark.parametrize("name", ["C", "E"])
def test_faulty_blocks_on_the_device(codec, O, name):
    k, m, e = 10, 4, 4
    sizes, sidx, lidx, surv, want, faulty = faulted(O, name, k, m, e)
    g = run(codec, sizes, k, m, sidx, surv, lidx)
    assert sync_code(codec) == ESINGULAR
    assert sync_code(codec) == 0
    g.check(out=want)
    off = RC.offsets(sizes)
    for b in faulty:
        assert not want[e * off[b]:e * off[b + 1]].any()


def test_a_bad_zero_size_block_alone_is_reported(codec, O):
    k, m, e = 10, 4, 4
    sizes, sidx, lidx, surv, want = clean(O, "C", k, m, e)
    sidx = sidx.copy()
    sidx[sizes.index(0), 1] = sidx[sizes.index(0), 0]
    g = run(codec, sizes, k, m, sidx, surv, lidx)
    assert sync_code(codec) == ESINGULAR
    assert sync_code(codec) == 0
    g.check(out=want)


@pytest.mark.parametrize("memory", ["pinned", "pageable"])
@pytest.mark.parametrize("name", ["C", "E"])
def test_faulty_blocks_from_host_memory(codec, O, name, memory):
    from memo_amd import ec
    k, m, e = 10, 4, 4
    sizes, sidx, lidx, surv, want, _ = faulted(O, name, k, m, e)
    g = Guarded(memory)
    s, o = g.input("surv", surv), g.output("out", want.size)
    si, li = g.input("surv_idx", sidx), g.input("lost_idx", lidx)
    with pytest.raises(ec.MemoECError) as ex:
        codec.rebuild_ragged(k, m, sizes, si, s, li, o)
    assert ex.value.code == ESINGULAR
    assert sync_code(codec) == 0
    g.check(out=want)


def test_a_bad_shared_pattern_is_refused(codec, O):
    from memo_amd import ec
    k, m, e = 10, 4, 4
    sizes, su, lu, surv, want = shared(O, "C", k, m, e)
    for bad in (np.r_[su[:-1], su[0]], np.r_[su[:-1], k + m]):
        g = Guarded()
        s, o = g.input("surv", surv), g.output("out", want.size)
        with pytest.raises(ec.MemoECError) as ex:
            codec.rebuild_ragged(k, m, sizes, bad.astype(np.uint8), s, lu, o, uniform=True)
        assert ex.value.code == ESINGULAR
        assert sync_code(codec) == 0
        g.check()  # out still reads 0xA5
    g = run(codec, sizes, k, m, su, surv, lu, uniform=True)  # nothing refused was cached
    codec.synchronize()
    g.check(out=want)


# ----------------------------------------------------- refusals and no-ops

def test_misaligned_device_buffers_are_refused(codec, O):
    from memo_amd import ec
    k, m, e = 10, 4, 4
    sizes, sidx, lidx, surv, want = clean(O, "C", k, m, e)
    for which in ("surv", "out"):
        g = Guarded()
        s = g.input("surv", surv, shift=8 if which == "surv" else 0)
        o = g.output("out", want.size, shift=8 if which == "out" else 0)
        si, li = g.input("surv_idx", sidx), g.input("lost_idx", lidx)
        with pytest.raises(ec.MemoECError) as ex:
            codec.rebuild_ragged(k, m, sizes, si, s, li, o)
        assert ex.value.code == EINVAL
        assert sync_code(codec) == 0
        g.check()


def test_empty_calls_write_nothing(codec, O):
    import torch
    k, m = 10, 4
    sizes, sidx, lidx, surv, want = clean(O, "C", k, m, 4)
    g = Guarded()
    s, o = g.input("surv", surv), g.output("out", want.size)
    si, li = g.input("surv_idx", sidx), g.input("lost_idx", lidx)
    n = len(sizes)
    none = torch.empty((n, 0), dtype=torch.uint8, device="cuda")
    codec.rebuild_ragged(k, m, sizes, si, s, none, o)                       # e == 0
    codec.rebuild_ragged(k, m, [], si[:0], s, li[:0], o)                    # n == 0
    codec.rebuild_ragged(k, m, [0] * n, si, s, li, o)                       # T == 0
    codec.rebuild_ragged(k, m, [0] * n, sidx[0], s, lidx[0], o, uniform=True)
    assert sync_code(codec) == 0
    g.check()
    assert (g.bufs["out"].snapshot()[g.bufs["out"].lo:][:want.size] == FILL).all()

"""The three rebuild entry points are one implementation: the same survivors
through memo_ec_rebuild_batch (codec.rebuild), a one-segment
memo_ec_rebuild_segments and, for a shared pattern, memo_ec_rebuild_uniform
give the same bytes, and those are the CPU oracle's shards -- from device,
pageable and pinned memory, zero-copy and through the copy pipeline (one
wave, more waves than slots), and with the launch split.

Geometries are the smallest at which each branch of the launch plan can go
wrong (plan_segment / rows_images in memo_ec.cpp):
  RS(4,2)   S = 64    n = 3   e = 2     many blocks per tile, flat mapping
  RS(10,4)  S = 4160  n = 37  e = 1, 4  260 chunks: a tile straddles two blocks
  RS(16,4)  S = 8192  n = 9   e = 4     two whole tiles per shard (table images)
  RS(5,3)   S = 128   n = 11  e = 3     k off the straight-line bodies: chunk loop

A call of these n cannot take four pipeline waves: a wave holds at least one
block (RS(4,2), n = 3: three waves at most) and MEMO_EC_OPT_PIPE_BYTES takes
no less than 1 MiB, above the survivors of every geometry here.  The
many-waves setting therefore runs each geometry twice at pipe_bytes = 1 MiB:
with its own n, and with the smallest n that takes four waves (same k, m, S
and e: 3 x floor(1 MiB / (k x S)) + 1 blocks, 3.0-3.3 MB of survivors)."""
import functools

import numpy as np
import pytest

from conftest import SEED

pytestmark = pytest.mark.gpu

GEOMETRIES = [(4, 2, 64, 3, 2), (10, 4, 4160, 37, 1), (10, 4, 4160, 37, 4), (16, 4, 8192, 9, 4),
              (5, 3, 128, 11, 3)]
MIN_PIPE = 1 << 20  # the smallest MEMO_EC_OPT_PIPE_BYTES
MEMORIES = ["device", "pageable", "pinned"]


def four_wave_blocks(k, S):
    return 3 * (MIN_PIPE // (k * S)) + 1


@functools.lru_cache(maxsize=None)
def case(k, m, S, n, e):
    """Survivors, patterns and the oracle's lost shards of n blocks, with
    per-block patterns ("block") and with one pattern for all ("shared").
    Computed once per geometry and shared by the rebuild paths; read only."""
    from oracle import oracle as O
    assert O.shard_size(k * S, k) == S
    rng = np.random.default_rng(1000 * k + 10 * e + n % 7)
    data = O.fill_blocks(SEED, 7 * k + e, n, k * S, k, S)
    par = O.encode(k, m, S, data, threads=4)
    # random survivor orders; lost shards that are data or parity
    s = np.stack([rng.permutation(k + m)[:k] for _ in range(n)]).astype(np.uint8)
    l = np.stack([np.setdiff1d(np.arange(k + m), x)[rng.permutation(m)[:e]] for x in s]).astype(np.uint8)
    perm = rng.permutation(k + m)
    su, lu = perm[:k].astype(np.uint8), perm[k:k + e].astype(np.uint8)
    ts, tl = np.tile(su, (n, 1)), np.tile(lu, (n, 1))
    out = {"block": dict(s=s, l=l, surv=O.gather(k, m, S, data, par, s), want=O.gather(k, m, S, data, par, l)),
           "shared": dict(s=ts, l=tl, su=su, lu=lu, surv=O.gather(k, m, S, data, par, ts),
                          want=O.gather(k, m, S, data, par, tl))}
    for c in out.values():
        for v in c.values():
            v.setflags(write=False)
    return out


def place(x, memory):
    """x (numpy) in `memory`; a fresh buffer each time."""
    import torch
    if memory == "pageable":
        return x.copy()
    t = torch.from_numpy(x.copy())
    return t.cuda() if memory == "device" else t.pin_memory()


def run_entries(codec, k, m, S, n, e, c, memory):
    """Every entry point that takes case c, each into an output of its own
    (preset to 0xA5, so an unwritten byte shows) -> {entry: bytes}."""
    surv = place(c["surv"], memory)
    # per-block indices: where the shards are (host: pageable is what every host call takes)
    s, l = (place(c["s"], "device"), place(c["l"], "device")) if memory == "device" else (c["s"], c["l"])
    outs = {}

    def out(name):
        outs[name] = place(np.full((n, e * S), 0xA5, np.uint8), memory)
        return outs[name]

    codec.rebuild(k, m, s, surv, l, out("rebuild"))
    codec.rebuild_segments([dict(k=k, m=m, surv_idx=s, surv=surv, lost_idx=l, out=out("segments"))])
    if "su" in c:
        codec.rebuild_uniform(k, m, c["su"], surv, c["lu"], out("uniform"))
        codec.rebuild_segments([dict(k=k, m=m, surv_idx=c["su"], surv=surv, lost_idx=c["lu"],
                                     out=out("segments_uniform"), uniform=True)])
        # the pattern's tables are cached by now: the cache hit gives the same bytes
        codec.rebuild_uniform(k, m, c["su"], surv, c["lu"], out("uniform_again"))
    if memory == "device":
        codec.synchronize()
        return {name: o.cpu().numpy() for name, o in outs.items()}
    return {name: np.asarray(o) for name, o in outs.items()}


def check(codec, k, m, S, n, e, opts):
    for kind, c in case(k, m, S, n, e).items():
        for memory in MEMORIES:
            with codec.options(**opts):
                got = run_entries(codec, k, m, S, n, e, c, memory)
            assert len(got) == (5 if kind == "shared" else 2)
            for name, o in got.items():
                assert np.array_equal(o, c["want"]), (name, kind, memory, opts)
                assert np.array_equal(o, got["rebuild"]), (name, kind, memory, opts)


@pytest.mark.parametrize("k,m,S,n,e", GEOMETRIES)
def test_entries_agree_zero_copy_on_and_off(codec, O, rebuild_path, k, m, S, n, e):
    """Zero-copy off, at its default, and on either side of its bound
    (survivors + outputs + per-block indices + 64 bytes: the last call that
    runs zero-copy and the first that takes the pipeline)."""
    total = n * ((k + e) * S + k + e)
    default = codec.get_option("zero_copy_bytes")
    assert default >= total + 64  # every geometry runs zero-copy by default
    for zc in (0, default, total + 64, total + 63):
        check(codec, k, m, S, n, e, dict(zero_copy_bytes=zc))


@pytest.mark.parametrize("k,m,S,n,e", GEOMETRIES)
def test_entries_agree_one_wave(codec, O, rebuild_path, k, m, S, n, e):
    """The copy pipeline with a batch the call's survivors fill exactly (or,
    below the smallest batch, fit): one wave."""
    pipe = max(MIN_PIPE, n * k * S)
    check(codec, k, m, S, n, e, dict(zero_copy_bytes=0, pipe_bytes=pipe))


@pytest.mark.parametrize("k,m,S,n,e", GEOMETRIES)
def test_entries_agree_many_waves(codec, O, rebuild_path, k, m, S, n, e):
    """The copy pipeline at its smallest batch: the geometry's own n, and the
    smallest n that takes four waves -- more waves than slots, the last one
    a single block (module docstring)."""
    per = MIN_PIPE // (k * S)
    n4 = four_wave_blocks(k, S)
    assert -(-n4 // per) == 4
    for blocks in (n, n4):
        check(codec, k, m, S, blocks, e, dict(zero_copy_bytes=0, pipe_bytes=MIN_PIPE))


@pytest.mark.parametrize("k,m,S,n,e", GEOMETRIES)
def test_entries_agree_split_launches(codec, O, rebuild_path, k, m, S, n, e):
    """max_launch_tiles = 30: RS(10,4) x 37 blocks splits into four spans of
    at most 10 blocks (device, zero-copy and pipeline calls alike); the
    other geometries fit one span and must not change."""
    step = max(1, 30 // ((S // 16 + 255) // 256 + 1))  # max_blocks_per_launch (memo_ec.cpp)
    assert (n > step) == (k == 10)
    check(codec, k, m, S, n, e, dict(max_launch_tiles=30))
    check(codec, k, m, S, n, e, dict(max_launch_tiles=30, zero_copy_bytes=0))

"""Ragged rebuild (memo_ec_rebuild_ragged) against memo_ec_rebuild_batch and
against the bucket-and-pad way the plugin takes without it, RS(10,4), e = 2,
per-block random patterns from ec.erasures.  Legs are alternated in one
process; each figure is the median of --rounds rounds of --reps calls, with
every round's value and the leg's own spread ((max - min) / median).

  (a) uniform batches, device-resident, 4096 x 1 MiB and 64 Ki x 4 KiB:
      rebuild against rebuild_ragged over the same buffers (the same layout
      when every size is equal), timed with device events around the call:
      for the ragged leg that is the index upload, the decode and the MAC.
      rebuild_path names what the uniform leg ran (fused / rows / images).
  (b) the seeded mixed batch of tools/ragged_probe.py: 2048 blocks, sizes
      log-uniform in [4 KiB, 1 MiB].  One ragged call against the plugin's
      way: blocks grouped by power-of-two shard size, every survivor padded
      to its bucket's largest, ONE rebuild_segments call (the padding is
      filled outside the timed region).  Device-resident (device events) and
      from pinned host memory (wall clock; the calls are synchronous).
      GiB/s counts the exact survivor bytes k * sum(S[b]) for both legs;
      padding_factor = padded bytes / exact bytes.

One JSON document (--out, default profiles/ragged_rebuild_probe.json), one
line per configuration on stdout.
  python tools/ragged_rebuild_probe.py [--rounds 5] [--reps 10] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from memo_amd import ec  # noqa: E402

SEED = 0x6D656D6F
K, M, E = 10, 4, 2


def spread(xs):
    return (max(xs) - min(xs)) / float(np.median(xs))


def summary(ms):
    return {name: {"ms": round(float(np.median(x)), 4), "rounds": [round(y, 4) for y in x],
                   "spread": round(spread(x), 4)} for name, x in ms.items()}


def bucket_of(S):
    b = 0
    while S > 64:
        S >>= 1
        b += 1
    return b


def timed_events(st, fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    with torch.cuda.stream(st):
        for e0, e1 in ev:
            e0.record(st)
            fn()
            e1.record(st)
        st.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))


def timed_wall(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # host-memory calls return when the shards are there
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def part_a(c, st, rounds, reps):
    out = []
    for B, n in [(1 << 20, 4096), (4096, 64 << 10)]:
        S = ec.shard_size(B, K)
        sizes = np.full(n, S, dtype=np.uint64)
        s, l = ec.erasures(SEED, 0, n, K, M, E)
        with torch.cuda.stream(st):
            surv = torch.randint(0, 256, (n * K * S,), dtype=torch.uint8, device="cuda")
            sd, ld = torch.from_numpy(s).cuda(), torch.from_numpy(l).cuda()
            o_u = torch.empty(n * E * S, dtype=torch.uint8, device="cuda")
            o_r = torch.empty(n * E * S, dtype=torch.uint8, device="cuda")
        st.synchronize()
        legs = {"rebuild_batch": lambda: c.rebuild(K, M, sd, surv, ld, o_u, S=S, n=n),
                "rebuild_ragged": lambda: c.rebuild_ragged(K, M, sizes, sd, surv, ld, o_r)}
        with torch.cuda.stream(st):
            for fn in legs.values():
                fn()
            st.synchronize()
        c.synchronize()
        same = bool(torch.equal(o_u, o_r))
        ms = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                ms[name].append(timed_events(st, fn, reps))
        host = []
        for _ in range(reps):
            st.synchronize()
            t0 = time.perf_counter()
            legs["rebuild_ragged"]()
            host.append((time.perf_counter() - t0) * 1e3)
        st.synchronize()
        res = summary(ms)
        mu, mr = res["rebuild_batch"]["ms"], res["rebuild_ragged"]["ms"]
        row = {"part": "a", "block_bytes": B, "blocks": n, "S": S, "out_equal": same, "legs": res,
               "rebuild_path": c.rebuild_path(n, K, S, E),
               "ragged_over_batch": round(mr / mu, 4),
               "inside_batch_spread": bool(abs(mr - mu) / mu <= res["rebuild_batch"]["spread"]),
               "ragged_host_ms": round(float(np.median(host)), 4),
               "survivor_GiBs": {name: round(n * K * S / res[name]["ms"] * 1e3 / 2 ** 30, 1) for name in legs}}
        out.append(row)
        print(json.dumps(row), flush=True)
        del surv, o_u, o_r
        torch.cuda.empty_cache()
    return out


def part_b(c, st, rounds, reps):
    rng = np.random.default_rng(SEED)
    n = 2048
    Bs = np.exp(rng.uniform(np.log(4096), np.log(1 << 20), size=n)).astype(np.int64)
    sizes = np.array([ec.shard_size(int(B), K) for B in Bs], dtype=np.uint64)
    off = ec.ragged_offsets(sizes)
    T = int(off[-1])
    s, l = ec.erasures(SEED, 0, n, K, M, E)
    buckets = {}
    for b, S in enumerate(sizes):
        buckets.setdefault(bucket_of(int(S)), []).append(b)
    groups = [(int(max(sizes[i] for i in ids)), ids) for _, ids in sorted(buckets.items())]
    padded = sum(Smax * len(ids) for Smax, ids in groups)
    out = []
    for memory in ("device", "pinned"):
        def alloc(nbytes):
            if memory == "device":
                return torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            return torch.empty(nbytes, dtype=torch.uint8).pin_memory()

        def put(a):
            t = alloc(a.size)
            t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
            return t.view(a.shape)
        src = torch.from_numpy(np.random.default_rng(SEED + 1).integers(0, 256, size=K * T, dtype=np.uint8))
        surv = alloc(K * T)
        surv.copy_(src)
        outb = alloc(E * T)
        sd, ld = put(s), put(l)
        segs = []
        for Smax, ids in groups:  # the bucket's blocks padded to its largest shard (untimed)
            d = torch.zeros((len(ids), K, Smax), dtype=torch.uint8)
            for x, b in enumerate(ids):
                S, o = int(sizes[b]), int(off[b])
                d[x, :, :S] = src[K * o:K * o + K * S].view(K, S)
            dd = alloc(d.numel())
            dd.copy_(d.view(-1))
            segs.append(dict(k=K, m=M, S=Smax, n=len(ids), surv=dd, out=alloc(len(ids) * E * Smax),
                             surv_idx=put(s[ids]), lost_idx=put(l[ids])))
        torch.cuda.synchronize()

        def leg_ragged():
            c.rebuild_ragged(K, M, sizes, sd, surv, ld, outb)

        def leg_bucketed():
            c.rebuild_segments(segs)

        legs = {"bucketed": leg_bucketed, "ragged": leg_ragged}
        timed = (lambda fn: timed_events(st, fn, reps)) if memory == "device" else (lambda fn: timed_wall(fn, reps))
        with torch.cuda.stream(st):
            for fn in legs.values():
                fn()
        c.synchronize()
        torch.cuda.synchronize()
        # the two ways agree: each block's shards are the head of its padded slot's
        same = True
        for g, (Smax, ids) in enumerate(groups):
            pg = segs[g]["out"].view(len(ids), E, Smax)
            for x in (0, len(ids) - 1):
                S, o = int(sizes[ids[x]]), int(off[ids[x]])
                same = same and bool(torch.equal(pg[x, :, :S].reshape(-1).cpu(), outb[E * o:E * o + E * S].cpu()))
        ms = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                with torch.cuda.stream(st):
                    ms[name].append(timed(fn))
        res = summary(ms)
        mb, mr = res["bucketed"]["ms"], res["ragged"]["ms"]
        row = {"part": "b", "memory": memory, "blocks": n, "exact_shard_bytes": T, "buckets": len(groups),
               "padding_factor": round(padded / T, 4), "out_equal": same, "legs": res,
               "ragged_over_bucketed": round(mr / mb, 4),
               "inside_bucketed_spread": bool(abs(mr - mb) / mb <= res["bucketed"]["spread"]),
               "survivor_GiBs": {name: round(K * T / res[name]["ms"] * 1e3 / 2 ** 30, 2) for name in legs}}
        out.append(row)
        print(json.dumps(row), flush=True)
        del surv, outb, segs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_rebuild_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_rebuild_probe: no GPU")
    ec.check_build()
    c = ec.Codec(0)
    st = torch.cuda.Stream()
    c.set_stream(st)
    results = part_a(c, st, a.rounds, a.reps) + part_b(c, st, a.rounds, a.reps)
    c.close()
    doc = {"tool": "tools/ragged_rebuild_probe.py", "device": torch.cuda.get_device_name(0),
           "build_id": ec.build_id(), "code": "RS(%d,%d) e=%d" % (K, M, E), "rounds": a.rounds, "reps": a.reps,
           "timing": "median of reps per round, legs alternated, median over rounds; device events "
                     "(device-resident) or wall clock (pinned host memory)",
           "all_equal": all(r["out_equal"] for r in results), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not doc["all_equal"]:
        sys.exit("ragged_rebuild_probe: the legs disagree")


if __name__ == "__main__":
    main()

"""Ragged encode (memo_ec_encode_ragged) against the uniform call and against
the bucket-and-pad way a caller without it has to take, RS(10,4).  Legs are
alternated in one process; the median of --rounds rounds is reported with
every round's value and the leg's own spread ((max - min) / median).

  (a) uniform batches, device-resident, 4096 x 1 MiB and 1 Mi x 4 KiB:
      encode_batch against encode_ragged over the same buffers (the same
      layout when every size is equal).  Timed with device events around the
      call: for the ragged leg that is the index upload plus the kernel.
      host_ms is the wall time the ragged call takes to return on an idle
      stream (the host-side index build and the enqueue); index_bytes what it
      uploads.  The kernels' own times come from a kernel trace of --quick.
  (b) a mixed batch: 2048 blocks, sizes log-uniform in [4 KiB, 1 MiB], fixed
      seed.  One ragged call against the plugin's bucketed way (blocks grouped
      by power-of-two shard size, every shard padded to its bucket's largest,
      one encode_batch per bucket; the padded buffers are filled outside the
      timed region), device-resident (device events) and from pinned host
      memory (wall clock; the calls are synchronous).  GiB/s counts the exact
      data bytes k * sum(S[b]) for both legs; padding_factor = padded bytes /
      exact bytes.

One JSON document (--out, default profiles/ragged_probe.json), one line per
configuration on stdout.
  python tools/ragged_probe.py [--rounds 5] [--reps 10] [--quick] [--out PATH]
--quick: part (a) only, 2 rounds, 3 reps (for a kernel trace)."""
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
K, M = 10, 4


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


def part_a(c, st, a, rounds, reps):
    out = []
    for B, n in [(1 << 20, 4096), (4096, 1 << 20)]:
        S = ec.shard_size(B, K)
        sizes = np.full(n, S, dtype=np.uint64)
        with torch.cuda.stream(st):
            data = torch.empty(n * K * S, dtype=torch.uint8, device="cuda")
            p_u = torch.empty(n * M * S, dtype=torch.uint8, device="cuda")
            p_r = torch.empty(n * M * S, dtype=torch.uint8, device="cuda")
            c.fill_blocks(SEED, 0, n, B, K, S, data)
        st.synchronize()
        legs = {"encode_batch": lambda: c.encode(K, M, data, p_u, S=S, n=n),
                "encode_ragged": lambda: c.encode_ragged(K, M, sizes, data, p_r)}

        def timed(fn):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(reps)]
            with torch.cuda.stream(st):
                for e0, e1 in ev:
                    e0.record(st)
                    fn()
                    e1.record(st)
                st.synchronize()
            return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

        with torch.cuda.stream(st):
            for fn in legs.values():
                fn()
            st.synchronize()
        same = bool(torch.equal(p_u, p_r))
        ms = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                ms[name].append(timed(fn))
        host = []
        for _ in range(reps):
            st.synchronize()
            t0 = time.perf_counter()
            legs["encode_ragged"]()
            host.append((time.perf_counter() - t0) * 1e3)
        st.synchronize()
        cols = S // 16
        tiles = -(-n * cols // 256)
        first = np.arange(tiles, dtype=np.int64) * 256  # a tile's first and last column
        last = np.minimum(first + 255, n * cols - 1)
        res = summary(ms)
        mu, mr = res["encode_batch"]["ms"], res["encode_ragged"]["ms"]
        row = {"part": "a", "block_bytes": B, "blocks": n, "S": S, "parity_equal": same, "legs": res,
               "ragged_over_batch": round(mr / mu, 4),
               "inside_batch_spread": bool(abs(mr - mu) / mu <= res["encode_batch"]["spread"]),
               "ragged_host_ms": round(float(np.median(host)), 4),
               "index_bytes": int(8 * (n + 1) + 4 * n + 16 * tiles),
               "tiles": int(tiles),
               "tiles_inside_one_block": int(np.count_nonzero(first // cols == last // cols)),
               "data_GiBs": {name: round(n * K * S / res[name]["ms"] * 1e3 / 2 ** 30, 1) for name in legs}}
        out.append(row)
        print(json.dumps({x: row[x] for x in row}), flush=True)
        del data, p_u, p_r
        torch.cuda.empty_cache()
    return out


def part_b(c, st, a, rounds, reps):
    rng = np.random.default_rng(SEED)
    n = 2048
    Bs = np.exp(rng.uniform(np.log(4096), np.log(1 << 20), size=n)).astype(np.int64)
    sizes = np.array([ec.shard_size(int(B), K) for B in Bs], dtype=np.uint64)
    off = ec.ragged_offsets(sizes)
    T = int(off[-1])
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
        src = torch.from_numpy(np.random.default_rng(SEED + 1).integers(0, 256, size=K * T, dtype=np.uint8))
        data = alloc(K * T)
        data.copy_(src)
        parity = alloc(M * T)
        gbufs = []
        for Smax, ids in groups:  # the bucket's blocks padded to its largest shard (untimed)
            d = torch.zeros((len(ids), K, Smax), dtype=torch.uint8)
            for x, b in enumerate(ids):
                S, o = int(sizes[b]), int(off[b])
                d[x, :, :S] = src[K * o:K * o + K * S].view(K, S)
            dd = alloc(d.numel())
            dd.copy_(d.view(-1))
            gbufs.append((Smax, len(ids), dd, alloc(len(ids) * M * Smax)))
        torch.cuda.synchronize()

        def leg_ragged():
            c.encode_ragged(K, M, sizes, data, parity)

        def leg_bucketed():
            for Smax, cnt, d, p in gbufs:
                c.encode(K, M, d, p, S=Smax, n=cnt)

        legs = {"bucketed": leg_bucketed, "ragged": leg_ragged}

        def timed(fn):
            if memory == "device":
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(reps)]
                with torch.cuda.stream(st):
                    for e0, e1 in ev:
                        e0.record(st)
                        fn()
                        e1.record(st)
                    st.synchronize()
                return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()  # host-memory calls return when the parity is there
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts))

        for fn in legs.values():
            fn()
        c.synchronize()
        torch.cuda.synchronize()
        # the two ways agree: each block's parity is the head of its padded slot's
        same = True
        for g, (Smax, ids) in enumerate(groups):
            pg = gbufs[g][3].view(len(ids), M, Smax)
            for x in (0, len(ids) - 1):
                S, o = int(sizes[ids[x]]), int(off[ids[x]])
                same = same and bool(torch.equal(pg[x, :, :S].reshape(-1).cpu(), parity[M * o:M * o + M * S].cpu()))
        ms = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                ms[name].append(timed(fn))
        res = summary(ms)
        mb, mr = res["bucketed"]["ms"], res["ragged"]["ms"]
        row = {"part": "b", "memory": memory, "blocks": n, "exact_shard_bytes": T, "buckets": len(groups),
               "padding_factor": round(padded / T, 4), "parity_equal": same, "legs": res,
               "ragged_over_bucketed": round(mr / mb, 4),
               # the plugin default's condition: not slower than the bucketed
               # way by more than the bucketed leg's own spread
               "ragged_within_bucketed_spread": bool(mr <= mb * (1 + res["bucketed"]["spread"])),
               "payload_GiBs": {name: round(K * T / res[name]["ms"] * 1e3 / 2 ** 30, 2) for name in legs}}
        out.append(row)
        print(json.dumps(row), flush=True)
        del data, parity, gbufs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_probe: no GPU")
    ec.check_build()
    rounds, reps = (2, 3) if a.quick else (a.rounds, a.reps)
    c = ec.Codec(0)
    st = torch.cuda.Stream()
    c.set_stream(st)
    results = part_a(c, st, a, rounds, reps)
    if not a.quick:
        results += part_b(c, st, a, rounds, max(3, reps // 2))
    c.close()
    doc = {"tool": "tools/ragged_probe.py", "device": torch.cuda.get_device_name(0),
           "build_id": ec.build_id(), "code": "RS(%d,%d)" % (K, M), "rounds": rounds, "reps": reps,
           "timing": "median of reps per round, legs alternated, median over rounds; device events "
                     "(device-resident) or wall clock (pinned host memory)",
           "index": "built on the host, one upload per call",
           "all_equal": all(r["parity_equal"] for r in results), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not doc["all_equal"]:
        sys.exit("ragged_probe: the legs disagree")


if __name__ == "__main__":
    main()

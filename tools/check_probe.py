"""The check of k + x shards in hand (memo_ec_check_batch) against what a
caller without it has to do, device-resident, at bench.py's two sizes
(4096 x 1 MiB and 1 M x 4 KiB) for RS(10,4) and RS(16,4), with x = 2 and
x = m spares, per-block random index sets.  Legs, alternated in one process
and timed with device events, on clean data and on data with 1 % of the
blocks corrupted in one shard:
  check         (a) Codec.check: check_prepare_kernel, the decode rows,
                    gf_check_kernel, check_locate_kernel
  rebuild_cmp   (b) rebuild of the x spares from the basis into a scratch
                    buffer (decode rows + gf_mac_kernel with tables built in
                    LDS: rebuild_path = 0, image_min_tiles = 0), then a
                    compare with the spares in hand per block in torch
  rebuild       (c) that rebuild alone: the yardstick -- the same bytes
                    moved, but it stores the x * S bytes the check only reads
  rebuild_images    the rebuild as the defaults run it (image_min_tiles = 1:
                    per-block table images through HBM where a shard holds a
                    whole tile and the tables are costly; the same kernels as
                    (c) elsewhere): the check's distance to it is the case
                    for an image variant of the check
  read          (d) stream_probe READ with kin = k + x, r = 1: the read rate
                    of the same (k + x) * S bytes per block
Every verdict word of (a) is checked: 0 for a clean block, and for a
corrupted one the word its single flipped byte gives by construction (a
spare: its row's bit and its index; a basis shard: all x bits and its
index); (b)'s flagged blocks are the same blocks.  One JSON document (--out,
default profiles/check_probe.json) and one line per configuration on stdout.
  python tools/check_probe.py [--rounds 5] [--reps 20] [--quick] [--code K,M] [--clean-only] [--out PATH]
--quick: RS(10,4) only (or --code's), 2 rounds; with --clean-only under
`rocprofv3 --kernel-trace --stats` it gives each kernel's share of a clean
check."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from memo_amd import ec  # noqa: E402

SEED = 0x6D656D6F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--clean-only", action="store_true", help="skip the corrupted state")
    ap.add_argument("--code", default=None, metavar="K,M", help="this code alone, e.g. 16,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("check_probe: no GPU")
    ec.check_build()
    codes = [(10, 4)] if a.quick else [(10, 4), (16, 4)]
    if a.code:
        codes = [tuple(int(v) for v in a.code.split(","))]
    rounds = 2 if a.quick else a.rounds
    sizes = [(1 << 20, 4096), (4096, 1 << 20)]
    c = ec.Codec(0)
    c.set_option("rebuild_path", 0)      # legs (b), (c): decode rows + MAC ...
    c.set_option("image_min_tiles", 0)   # ... with tables built in LDS, as the check builds them
    st = torch.cuda.Stream()
    c.set_stream(st)
    results = []
    for k, m in codes:
        for B, n in sizes:
            S = ec.shard_size(B, k)
            with torch.cuda.stream(st):
                data = torch.empty((n, k * S), dtype=torch.uint8, device="cuda")
                parity = torch.empty((n, m * S), dtype=torch.uint8, device="cuda")
                c.fill_blocks(SEED, 0, n, B, k, S, data)
                c.encode(k, m, data, parity)
            st.synchronize()
            for x in (2, m):
                kx = k + x
                rng = np.random.default_rng(SEED ^ (k << 8) ^ (x << 4) ^ n)
                idx_h = rng.permuted(np.tile(np.arange(k + m, dtype=np.uint8), (n, 1)), axis=1)[:, :kx]
                idx_h = np.ascontiguousarray(idx_h)
                with torch.cuda.stream(st):
                    idx = torch.from_numpy(idx_h).cuda()
                    basis_idx = idx[:, :k].contiguous()
                    spare_idx = idx[:, k:].contiguous()
                    have = torch.empty((n, kx * S), dtype=torch.uint8, device="cuda")
                    c.gather_shards(k, m, S, n, data, parity, idx, have)
                    surv = torch.empty((n, k * S), dtype=torch.uint8, device="cuda")
                    spares = torch.empty((n, x * S), dtype=torch.uint8, device="cuda")
                    scratch = torch.empty((n, x * S), dtype=torch.uint8, device="cuda")
                    rout = torch.empty((n, S), dtype=torch.uint8, device="cuda")
                    verdict = torch.empty(n, dtype=torch.int32, device="cuda")
                st.synchronize()

                def leg_check():
                    c.check(k, m, idx, have, verdict, x=x, S=S, n=n)

                def leg_rebuild_cmp():
                    c.rebuild(k, m, basis_idx, surv, spare_idx, scratch)
                    return (scratch != spares).view(n, -1).any(dim=1)

                def leg_rebuild():
                    c.rebuild(k, m, basis_idx, surv, spare_idx, scratch)

                def leg_rebuild_images():
                    c.set_option("image_min_tiles", 1)
                    c.rebuild(k, m, basis_idx, surv, spare_idx, scratch)
                    c.set_option("image_min_tiles", 0)

                def leg_read():
                    c.stream_probe(kx, 1, have, rout, mode="read")

                legs = {"check": leg_check, "rebuild_cmp": leg_rebuild_cmp, "rebuild": leg_rebuild,
                        "rebuild_images": leg_rebuild_images, "read": leg_read}

                def timed(fn):
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                          for _ in range(a.reps)]
                    with torch.cuda.stream(st):
                        for e0, e1 in ev:
                            e0.record(st)
                            fn()
                            e1.record(st)
                        st.synchronize()
                    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

                for state in ("clean",) if a.clean_only else ("clean", "corrupt_1pct"):
                    want = np.zeros(n, dtype=np.uint32)
                    if state != "clean":
                        # one flipped byte in one of the k + x shards in hand of 1 % of the blocks
                        cnt = max(1, n // 100)
                        blocks = np.sort(rng.choice(n, size=cnt, replace=False))
                        pos = rng.integers(0, kx, size=cnt)
                        byte = rng.integers(0, S, size=cnt)
                        with torch.cuda.stream(st):
                            have[torch.from_numpy(blocks).cuda(), torch.from_numpy(pos * S + byte).cuda()] ^= 0x5A
                        mask = np.where(pos < k, (1 << x) - 1, 1 << np.maximum(pos - k, 0))
                        want[blocks] = mask | (idx_h[blocks, pos].astype(np.uint32) << 16)
                    with torch.cuda.stream(st):
                        surv.copy_(have[:, :k * S])  # the caller's survivors and spares: the same bytes
                        spares.copy_(have[:, k * S:])
                        # correctness first: every word of (a), and (b)'s flagged blocks
                        leg_check()
                        flagged_b = leg_rebuild_cmp()
                        st.synchronize()
                    v = verdict.cpu().numpy().view(np.uint32)
                    ok = bool(np.array_equal(v, want)) and \
                        bool(np.array_equal(flagged_b.cpu().numpy(), want != 0))
                    c.synchronize()  # no deferred error from the rebuilds
                    with torch.cuda.stream(st):  # warm-up of every leg
                        for fn in legs.values():
                            fn()
                        st.synchronize()
                    ms = {name: [] for name in legs}
                    for _ in range(rounds):
                        for name, fn in legs.items():
                            ms[name].append(timed(fn))
                    med = {name: float(np.median(t)) for name, t in ms.items()}
                    bytes_read = n * kx * S
                    row = {"code": "RS(%d,%d)" % (k, m), "x": x, "block_bytes": B, "blocks": n, "S": S,
                           "state": state, "verdicts_exact": ok,
                           "corrupted_blocks": int(np.count_nonzero(want)),
                           "ms": {name: round(t, 4) for name, t in med.items()},
                           "ms_rounds": {name: [round(y, 4) for y in t] for name, t in ms.items()},
                           # the (k + x) * S bytes of every block over the leg's time (the check and
                           # the read load all of them; the rebuild loads k * S and stores x * S)
                           "shard_GBs": {name: round(bytes_read / med[name] / 1e6, 1)
                                         for name in ("check", "rebuild", "read")},
                           "check_over_rebuild_cmp": round(med["check"] / med["rebuild_cmp"], 4),
                           "check_over_rebuild": round(med["check"] / med["rebuild"], 4),
                           "check_over_rebuild_images": round(med["check"] / med["rebuild_images"], 4),
                           "check_over_read": round(med["check"] / med["read"], 4)}
                    results.append(row)
                    print(json.dumps({f: row[f] for f in row if f != "ms_rounds"}), flush=True)
                del idx, basis_idx, spare_idx, have, surv, spares, scratch, rout, verdict
                torch.cuda.empty_cache()
            del data, parity
            torch.cuda.empty_cache()
    c.close()
    doc = {"tool": "tools/check_probe.py", "device": torch.cuda.get_device_name(0),
           "build_id": ec.build_id(), "rounds": rounds, "reps": a.reps,
           "timing": "device events around each call, median of reps, median over alternated rounds",
           "rebuild_legs": "rebuild_path=0, image_min_tiles=0 (decode rows + gf_mac_kernel, tables built in LDS)",
           "all_exact": all(r["verdicts_exact"] for r in results), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not doc["all_exact"]:
        sys.exit("check_probe: a verdict word is not the expected one")


if __name__ == "__main__":
    main()

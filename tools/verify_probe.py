"""Parity verify (memo_ec_verify_batch) against what a caller without it has
to do, device-resident, at bench.py's two sizes (4096 x 1 MiB and
1 M x 4 KiB) for RS(10,4) and RS(16,4).  Legs, alternated in one process and
timed with device events, on clean data and on data with 1 % of the blocks
corrupted in one shard:
  verify        (a) Codec.verify: gf_verify_kernel + verify_locate_kernel
  encode_cmp    (b) encode into a scratch parity, then compare it with the
                    stored parity per block in torch (the parent's way)
  encode        (c) the encode alone
  read          (d) stream_probe READ with kin = k + m, r = 1: the read rate
                    of the same (k + m) * S bytes per block
(a)'s answer is checked against (b)'s on the same inputs: the same blocks
flagged, and every located shard the one that was corrupted.  One JSON
document (--out, default profiles/verify_probe.json) and one line per
configuration on stdout.
  python tools/verify_probe.py [--rounds 5] [--reps 20] [--quick] [--clean-only] [--out PATH]
--quick: RS(10,4) only, 2 rounds; with --clean-only under
`rocprofv3 --kernel-trace --stats` it gives the locate pass's cost on a clean
batch (verify_locate_kernel's own line)."""
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


def corrupt(data, parity, k, m, S, n, rng):
    """One flipped byte in one shard of 1 % of the blocks; returns (blocks,
    shard per block)."""
    cnt = max(1, n // 100)
    blocks = np.sort(rng.choice(n, size=cnt, replace=False))
    shards = rng.integers(0, k + m, size=cnt)
    pos = rng.integers(0, S, size=cnt)
    dmask = shards < k
    bd = torch.from_numpy(blocks[dmask]).cuda()
    od = torch.from_numpy(shards[dmask] * S + pos[dmask]).cuda()
    bp = torch.from_numpy(blocks[~dmask]).cuda()
    op = torch.from_numpy((shards[~dmask] - k) * S + pos[~dmask]).cuda()
    data[bd, od] ^= 0x5A
    parity[bp, op] ^= 0x5A
    return blocks, shards


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--clean-only", action="store_true", help="skip the corrupted state")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("verify_probe: no GPU")
    ec.check_build()
    codes = [(10, 4)] if a.quick else [(10, 4), (16, 4)]
    rounds = 2 if a.quick else a.rounds
    sizes = [(1 << 20, 4096), (4096, 1 << 20)]
    c = ec.Codec(0)
    st = torch.cuda.Stream()
    c.set_stream(st)
    results = []
    for k, m in codes:
        for B, n in sizes:
            S = ec.shard_size(B, k)
            with torch.cuda.stream(st):
                data = torch.empty((n, k * S), dtype=torch.uint8, device="cuda")
                parity = torch.empty((n, m * S), dtype=torch.uint8, device="cuda")
                scratch = torch.empty((n, m * S), dtype=torch.uint8, device="cuda")
                allsh = torch.empty((n, (k + m) * S), dtype=torch.uint8, device="cuda")
                rout = torch.empty((n, S), dtype=torch.uint8, device="cuda")
                verdict = torch.empty(n, dtype=torch.int32, device="cuda")
                c.fill_blocks(SEED, 0, n, B, k, S, data)
                c.encode(k, m, data, parity)
                allsh[:, :k * S] = data  # the same bytes as one (k + m)-shard input
                allsh[:, k * S:] = parity
            st.synchronize()

            def leg_verify():
                c.verify(k, m, data, parity, verdict)

            def leg_encode_cmp():
                c.encode(k, m, data, scratch)
                return (scratch != parity).view(n, -1).any(dim=1)

            def leg_encode():
                c.encode(k, m, data, scratch)

            def leg_read():
                c.stream_probe(k + m, 1, allsh, rout, mode="read")

            legs = {"verify": leg_verify, "encode_cmp": leg_encode_cmp, "encode": leg_encode,
                    "read": leg_read}

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
                rng = np.random.default_rng(SEED ^ (k << 8) ^ n)
                blocks = shards = None
                if state != "clean":
                    with torch.cuda.stream(st):
                        blocks, shards = corrupt(data, parity, k, m, S, n, rng)
                    st.synchronize()
                # correctness first: (a) against (b) on these inputs
                with torch.cuda.stream(st):
                    leg_verify()
                    flagged_b = leg_encode_cmp()
                    st.synchronize()
                v = verdict.cpu().numpy().view(np.uint32)
                fb = flagged_b.cpu().numpy()
                ok = bool(np.array_equal(v != 0, fb))
                if blocks is None:
                    ok = ok and not fb.any()
                else:
                    mask, shard = ec.split_verdict(v)
                    ok = ok and np.array_equal(np.flatnonzero(fb), blocks) and \
                        np.array_equal(shard[blocks], shards.astype(np.uint32))
                with torch.cuda.stream(st):  # warm-up of every leg
                    for fn in legs.values():
                        fn()
                    st.synchronize()
                ms = {name: [] for name in legs}
                for _ in range(rounds):
                    for name, fn in legs.items():
                        ms[name].append(timed(fn))
                med = {name: float(np.median(x)) for name, x in ms.items()}
                bytes_read = n * (k + m) * S
                row = {"code": "RS(%d,%d)" % (k, m), "block_bytes": B, "blocks": n, "S": S, "state": state,
                       "matches_encode_compare": ok,
                       "corrupted_blocks": 0 if blocks is None else int(len(blocks)),
                       "ms": {name: round(x, 4) for name, x in med.items()},
                       "ms_rounds": {name: [round(y, 4) for y in x] for name, x in ms.items()},
                       # the (k + m) * S bytes of every block over the leg's time (verify and
                       # read load all of them; the encode loads k * S and stores m * S)
                       "shard_GBs": {name: round(bytes_read / med[name] / 1e6, 1)
                                     for name in ("verify", "encode", "read")},
                       "verify_over_encode_cmp": round(med["verify"] / med["encode_cmp"], 4),
                       "verify_over_encode": round(med["verify"] / med["encode"], 4),
                       "verify_over_read": round(med["verify"] / med["read"], 4)}
                results.append(row)
                print(json.dumps({x: row[x] for x in row if x != "ms_rounds"}), flush=True)
            del data, parity, scratch, allsh, rout, verdict
            torch.cuda.empty_cache()
    c.close()
    doc = {"tool": "tools/verify_probe.py", "device": torch.cuda.get_device_name(0),
           "build_id": ec.build_id(), "rounds": rounds, "reps": a.reps,
           "timing": "device events around each call, median of reps, median over alternated rounds",
           "all_match": all(r["matches_encode_compare"] for r in results), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not doc["all_match"]:
        sys.exit("verify_probe: verify disagrees with encode + compare")


if __name__ == "__main__":
    main()

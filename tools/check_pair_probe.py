"""What memo_ec_check_pair_batch costs over memo_ec_check_batch,
device-resident, RS(10,4) with x = 4 spares and per-block random index sets,
at bench.py's two sizes (4096 x 1 MiB and 1 M x 4 KiB).  Two legs, alternated
in one process and timed with device events:
  check       Codec.check: the yardstick, in the same run
  check_pair  Codec.check_pair: the same launches and check_pair_kernel
on three states of the data:
  clean          every word 0: the extra launch reads n verdict words
  corrupt_1pct   one flipped byte in one shard of 1 % of the blocks: located
                 by the check, so the extra launch still only reads the words
  pair_1pct      one flipped byte in each of two shards (different offsets)
                 of 1 % of the blocks: the cold path of the new kernel.  The
                 check leaves these unlocated; its time is given for
                 information (no bound is set on the pair leg here)
Every verdict word of both legs is checked against what the flipped bytes
give by construction.  One JSON document (--out, default
profiles/check_pair_probe.json) and one line per configuration on stdout.
  python tools/check_pair_probe.py [--rounds 5] [--reps 20] [--quick] [--out PATH]
--quick: 2 rounds of 5 calls."""
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
UNLOCATED = ec.VERDICT_UNLOCATED


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_pair_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("check_pair_probe: no GPU")
    ec.check_build()
    rounds, reps = (2, 5) if a.quick else (a.rounds, a.reps)
    k, m, x = 10, 4, 4
    kx = k + x
    sizes = [(1 << 20, 4096), (4096, 1 << 20)]
    c = ec.Codec(0)
    st = torch.cuda.Stream()
    c.set_stream(st)
    results = []
    for B, n in sizes:
        S = ec.shard_size(B, k)
        rng = np.random.default_rng(SEED ^ (k << 8) ^ (x << 4) ^ n)
        idx_h = rng.permuted(np.tile(np.arange(k + m, dtype=np.uint8), (n, 1)), axis=1)[:, :kx]
        idx_h = np.ascontiguousarray(idx_h)
        with torch.cuda.stream(st):
            data = torch.empty((n, k * S), dtype=torch.uint8, device="cuda")
            parity = torch.empty((n, m * S), dtype=torch.uint8, device="cuda")
            c.fill_blocks(SEED, 0, n, B, k, S, data)
            c.encode(k, m, data, parity)
            idx = torch.from_numpy(idx_h).cuda()
            have = torch.empty((n, kx * S), dtype=torch.uint8, device="cuda")
            c.gather_shards(k, m, S, n, data, parity, idx, have)
            verdict = torch.empty(n, dtype=torch.int32, device="cuda")
        st.synchronize()
        del data, parity
        torch.cuda.empty_cache()

        def leg_check():
            c.check(k, m, idx, have, verdict, x=x, S=S, n=n)

        def leg_pair():
            c.check_pair(k, m, idx, have, verdict, x=x, S=S, n=n)

        legs = {"check": leg_check, "check_pair": leg_pair}

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

        def flip(blocks, pos, byte):
            with torch.cuda.stream(st):
                have[torch.from_numpy(blocks).cuda(), torch.from_numpy(pos * S + byte).cuda()] ^= 0x5A

        cnt = max(1, n // 100)
        for state in ("clean", "corrupt_1pct", "pair_1pct"):
            want = {name: np.zeros(n, dtype=np.uint32) for name in legs}
            undo = []
            if state != "clean":
                blocks = np.sort(rng.choice(n, size=cnt, replace=False))
                pos = rng.integers(0, kx, size=cnt)
                byte = rng.integers(0, S, size=cnt)
                flip(blocks, pos, byte)
                undo.append((blocks, pos, byte))
                mask = np.where(pos < k, (1 << x) - 1, 1 << np.maximum(pos - k, 0)).astype(np.uint32)
                word = mask | (idx_h[blocks, pos].astype(np.uint32) << 16)
                if state == "pair_1pct":
                    # a second shard of the same blocks, at another offset: the syndromes
                    # of the two bytes are multiples of two columns (rank 2)
                    pos2 = (pos + 1 + rng.integers(0, kx - 1, size=cnt)) % kx
                    byte2 = (byte + 1 + rng.integers(0, S - 1, size=cnt)) % S
                    flip(blocks, pos2, byte2)
                    undo.append((blocks, pos2, byte2))
                    mask |= np.where(pos2 < k, (1 << x) - 1, 1 << np.maximum(pos2 - k, 0)).astype(np.uint32)
                    ia, ib = idx_h[blocks, pos].astype(np.uint32), idx_h[blocks, pos2].astype(np.uint32)
                    want["check"][blocks] = mask | (UNLOCATED << 16)
                    want["check_pair"][blocks] = mask | (np.minimum(ia, ib) << 16) | ((np.maximum(ia, ib) + 1) << 25)
                else:
                    want["check"][blocks] = want["check_pair"][blocks] = word
            ok = {}
            for name, fn in legs.items():  # correctness first, which is the warm-up too
                with torch.cuda.stream(st):
                    verdict.fill_(0x5A5A5A5A)
                    fn()
                    st.synchronize()
                ok[name] = bool(np.array_equal(verdict.cpu().numpy().view(np.uint32), want[name]))
            c.synchronize()
            ms = {name: [] for name in legs}
            for _ in range(rounds):
                for name, fn in legs.items():
                    ms[name].append(timed(fn))
            med = {name: float(np.median(t)) for name, t in ms.items()}
            row = {"code": "RS(%d,%d)" % (k, m), "x": x, "block_bytes": B, "blocks": n, "S": S,
                   "state": state, "verdicts_exact": ok,
                   "flagged_blocks": int(np.count_nonzero(want["check"])),
                   "pair_blocks": int(np.count_nonzero(want["check_pair"] >> 25)),
                   "ms": {name: round(t, 4) for name, t in med.items()},
                   "ms_rounds": {name: [round(y, 4) for y in t] for name, t in ms.items()},
                   "check_pair_over_check": round(med["check_pair"] / med["check"], 4)}
            results.append(row)
            print(json.dumps({f: row[f] for f in row if f != "ms_rounds"}), flush=True)
            for blocks, pos, byte in undo:  # put the bytes back: each state starts clean
                flip(blocks, pos, byte)
            st.synchronize()
        del idx, have, verdict
        torch.cuda.empty_cache()
    c.close()
    doc = {"tool": "tools/check_pair_probe.py", "device": torch.cuda.get_device_name(0),
           "build_id": ec.build_id(), "rounds": rounds, "reps": reps,
           "timing": "device events around each call, median of reps, median over alternated rounds",
           "all_exact": all(all(r["verdicts_exact"].values()) for r in results), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not doc["all_exact"]:
        sys.exit("check_pair_probe: a verdict word is not the expected one")


if __name__ == "__main__":
    main()

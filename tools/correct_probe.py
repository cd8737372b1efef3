"""The check-and-mend call (memo_ec_correct_batch) against the check alone and
against what a caller without it has to do, device-resident, at the points of
tools/check_probe.py: 4096 x 1 MiB and 1 M x 4 KiB, RS(10,4) and RS(16,4),
x = 2 and x = m spares, per-block random index sets, on clean data and with
1 % of the blocks corrupted in one shard.  Legs, alternated in one process
and timed with device events:
  correct       (a) Codec.correct: the check's kernels, correct_list_kernel,
                    gf_correct_kernel
  check         (b) Codec.check alone
  caller        (c) what a caller does today: Codec.check, the verdicts to
                    the host, the flagged blocks' k other shards gathered,
                    Codec.rebuild with e = 1, the result scattered back
  read              stream_probe READ with kin = k + x, r = 1: the read rate
                    of the run, for the cost of the mended blocks' bytes
The corrupted shards are put back before every timed call (outside the
events).  Every verdict word of (a) and every byte of `have` after (a) and
after (c) is checked.  Reported per point: a / b; on corrupted data a - b
against the time the mended blocks' (k + 1) * S bytes take at the read rate,
and a / c.  One JSON document (--out, default profiles/correct_probe.json)
and one line per configuration on stdout.
  python tools/correct_probe.py [--rounds 5] [--reps 20] [--quick] [--code K,M] [--clean-only] [--out PATH]
--quick: RS(10,4) only (or --code's), 2 rounds; with --clean-only under
`rocprofv3 --kernel-trace --stats` it gives each kernel's share of a clean
call."""
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
CORRECTED = 1 << 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--clean-only", action="store_true", help="skip the corrupted state")
    ap.add_argument("--code", default=None, metavar="K,M", help="this code alone, e.g. 16,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("correct_probe: no GPU")
    ec.check_build()
    codes = [(10, 4)] if a.quick else [(10, 4), (16, 4)]
    if a.code:
        codes = [tuple(int(v) for v in a.code.split(","))]
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
                    clean = torch.empty((n, kx * S), dtype=torch.uint8, device="cuda")
                    c.gather_shards(k, m, S, n, data, parity, idx, clean)
                    have = clean.clone()
                    rout = torch.empty((n, S), dtype=torch.uint8, device="cuda")
                    verdict = torch.empty(n, dtype=torch.int32, device="cuda")
                st.synchronize()
                have3 = have.view(n, kx, S)
                state_v = {}  # the corrupted state: set per state below

                def restore():
                    if state_v.get("blocks") is not None:
                        have[state_v["blocks"], state_v["off"]] = state_v["bad"]

                def leg_correct():
                    c.correct(k, m, idx, have, verdict, x=x, S=S, n=n)

                def leg_check():
                    c.check(k, m, idx, have, verdict, x=x, S=S, n=n)

                def leg_caller():
                    c.check(k, m, idx, have, verdict, x=x, S=S, n=n)
                    v = verdict.cpu().numpy().view(np.uint32)  # waits for the check
                    fl = np.flatnonzero((v != 0) & (v != ec.VERDICT_INVALID) & (((v >> 16) & 0xFF) != 0xFF))
                    if fl.size == 0:
                        return
                    shard = ((v[fl] >> 16) & 0xFF).astype(np.uint8)
                    q = np.argmax(idx_h[fl] == shard[:, None], axis=1)
                    others = np.arange(k)[None, :] + (np.arange(k)[None, :] >= q[:, None])  # k positions, not q
                    flt = torch.from_numpy(fl).cuda()
                    surv = have3[flt[:, None], torch.from_numpy(others).cuda()].reshape(fl.size, k * S)
                    surv_idx = torch.from_numpy(np.take_along_axis(idx_h[fl], others, axis=1)).cuda()
                    lost_idx = torch.from_numpy(shard.reshape(-1, 1)).cuda()
                    out = torch.empty((fl.size, S), dtype=torch.uint8, device="cuda")
                    c.rebuild(k, m, surv_idx, surv, lost_idx, out)
                    have3[flt, torch.from_numpy(q).cuda()] = out

                def leg_read():
                    c.stream_probe(kx, 1, have, rout, mode="read")

                legs = {"correct": leg_correct, "check": leg_check, "caller": leg_caller, "read": leg_read}

                def timed(fn):
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                          for _ in range(a.reps)]
                    with torch.cuda.stream(st):
                        for e0, e1 in ev:
                            restore()
                            e0.record(st)
                            fn()
                            e1.record(st)
                        st.synchronize()
                    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

                for state in ("clean",) if a.clean_only else ("clean", "corrupt_1pct"):
                    want = np.zeros(n, dtype=np.uint32)
                    state_v.clear()
                    if state != "clean":
                        # one flipped byte in one of the k + x shards in hand of 1 % of the blocks
                        cnt = max(1, n // 100)
                        blocks = np.sort(rng.choice(n, size=cnt, replace=False))
                        pos = rng.integers(0, kx, size=cnt)
                        byte = rng.integers(0, S, size=cnt)
                        mask = np.where(pos < k, (1 << x) - 1, 1 << np.maximum(pos - k, 0))
                        want[blocks] = mask | (idx_h[blocks, pos].astype(np.uint32) << 16) | CORRECTED
                        with torch.cuda.stream(st):
                            state_v["blocks"] = torch.from_numpy(blocks).cuda()
                            state_v["off"] = torch.from_numpy(pos * S + byte).cuda()
                            state_v["bad"] = clean[state_v["blocks"], state_v["off"]] ^ 0x5A
                    with torch.cuda.stream(st):
                        # correctness first: every word and byte of (a), every byte of (c)
                        restore()
                        leg_correct()
                        st.synchronize()
                        ok = bool(np.array_equal(verdict.cpu().numpy().view(np.uint32), want)) and \
                            bool(torch.equal(have, clean))
                        restore()
                        leg_caller()
                        st.synchronize()
                        ok = ok and bool(torch.equal(have, clean))
                    c.synchronize()  # no deferred error from the rebuilds
                    with torch.cuda.stream(st):  # warm-up of every leg
                        for fn in legs.values():
                            restore()
                            fn()
                        st.synchronize()
                    ms = {name: [] for name in legs}
                    for _ in range(rounds):
                        for name, fn in legs.items():
                            ms[name].append(timed(fn))
                    med = {name: float(np.median(t)) for name, t in ms.items()}
                    mended = int(np.count_nonzero(want))
                    read_rate = n * kx * S / med["read"] / 1e6   # GB/s
                    row = {"code": "RS(%d,%d)" % (k, m), "x": x, "block_bytes": B, "blocks": n, "S": S,
                           "state": state, "words_and_bytes_exact": ok, "corrupted_blocks": mended,
                           "ms": {name: round(t, 4) for name, t in med.items()},
                           "ms_rounds": {name: [round(y, 4) for y in t] for name, t in ms.items()},
                           "read_GBs": round(read_rate, 1),
                           "correct_over_check": round(med["correct"] / med["check"], 4),
                           "correct_minus_check_ms": round(med["correct"] - med["check"], 4),
                           # the mended blocks' (k + 1) * S bytes (k loaded, 1 stored) at the read rate
                           "mended_bytes_at_read_rate_ms": round(mended * (k + 1) * S / read_rate / 1e6, 4),
                           "correct_over_caller": round(med["correct"] / med["caller"], 4)}
                    results.append(row)
                    print(json.dumps({f: row[f] for f in row if f != "ms_rounds"}), flush=True)
                state_v.clear()
                del idx, clean, have, have3, rout, verdict
                torch.cuda.empty_cache()
            del data, parity
            torch.cuda.empty_cache()
    c.close()
    doc = {"tool": "tools/correct_probe.py", "device": torch.cuda.get_device_name(0),
           "build_id": ec.build_id(), "rounds": rounds, "reps": a.reps,
           "timing": "device events around each call, the corrupted shards put back before it; "
                     "median of reps, median over alternated rounds",
           "all_exact": all(r["words_and_bytes_exact"] for r in results), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not doc["all_exact"]:
        sys.exit("correct_probe: a verdict word or a mended byte is not the expected one")


if __name__ == "__main__":
    main()

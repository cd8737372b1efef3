"""The check-and-mend call for one or two wrong shards
(memo_ec_correct_pair_batch) against the pair check alone and against what a
caller without it has to do, device-resident, at the points of
tools/check_probe.py: 4096 x 1 MiB and 1 M x 4 KiB, RS(10,4) and RS(16,4),
x = 4 spares, per-block random index sets, on clean data, with 1 % of the
blocks corrupted in one shard and with 1 % corrupted in two.  Legs, alternated
in one process and timed with device events:
  correct_pair  (a) Codec.correct_pair: the check's kernels, the single
                    correction's two, check_pair_kernel,
                    correct_pair_list_kernel, gf_correct_pair_kernel
  check_pair    (b) Codec.check_pair alone
  caller        (c) what a caller does without (a): Codec.check_pair, the
                    words to the host, the named blocks' k input shards
                    gathered with torch, Codec.rebuild with e = 1 (singles)
                    and e = 2 (pairs), the results scattered back
  correct, check    Codec.correct and Codec.check: the single correction's
                    own cost in the same run, to hold a - b against
  read              stream_probe READ with kin = k + x, r = 1: the read rate
                    of the run, for the cost of the mended blocks' bytes
The corrupted shards are put back before every timed call (outside the
events).  Every verdict word of (a) and every byte of `have` after (a) and
after (c) is checked.  Reported per point: a / b; on corrupted data a - b
against the time the mended blocks' bytes ((k + 1) * S a single, (k + 2) * S a
pair) take at the read rate, and a / c.  One JSON document (--out, default
profiles/correct_pair_probe.json) and one line per configuration on stdout.
  python tools/correct_pair_probe.py [--rounds 5] [--reps 20] [--quick] [--code K,M] [--clean-only] [--out PATH]
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
from memo_amd import correct_pair_ref, ec  # noqa: E402

SEED = 0x6D656D6F
CORRECTED = 1 << 24
STATES = ("clean", "one_1pct", "two_1pct")


def input_positions(k, x, qa, qb):
    """correct_pair_ref.input_positions for arrays of targets qa < qb: (cnt x k)."""
    cnt = qa.size
    pos = np.tile(np.arange(k), (cnt, 1))
    sp = np.tile(np.arange(k, k + x), (cnt, 1))
    taken = (sp == qa[:, None]) | (sp == qb[:, None])
    free = np.take_along_axis(sp, np.argsort(taken, axis=1, kind="stable"), axis=1)  # free spares first, ascending
    ia, ib = np.flatnonzero(qa < k), np.flatnonzero(qb < k)
    pos[ia, qa[ia]] = free[ia, 0]
    pos[ib, qb[ib]] = free[ib, 1]
    return pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--clean-only", action="store_true", help="skip the corrupted states")
    ap.add_argument("--code", default=None, metavar="K,M", help="this code alone, e.g. 16,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_pair_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("correct_pair_probe: no GPU")
    ec.check_build()
    for kk, xx in ((10, 4), (16, 4)):  # the vectorised input positions are the reference's, for every pair
        qq = np.array([(p, q) for p in range(kk + xx) for q in range(p + 1, kk + xx)])
        got = input_positions(kk, xx, qq[:, 0], qq[:, 1])
        assert all(got[i].tolist() == correct_pair_ref.input_positions(kk, xx, int(p), int(q))
                   for i, (p, q) in enumerate(qq))
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
            x = 4
            kx = k + x
            rng = np.random.default_rng(SEED ^ (k << 8) ^ (x << 4) ^ n)  # check_probe's index sets
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
            del data, parity
            torch.cuda.empty_cache()
            have3 = have.view(n, kx, S)
            state_v = {}  # the corrupted state: set per state below

            def restore():
                if state_v.get("blocks") is not None:
                    have[state_v["blocks"], state_v["off"]] = state_v["bad"]

            def rebuild_into(fl, pos, lost_pos):
                """Blocks fl: the shards in lost_pos (cnt x e) rebuilt from those in pos (cnt x k)."""
                e = lost_pos.shape[1]
                flt = torch.from_numpy(fl).cuda()
                surv = have3[flt[:, None], torch.from_numpy(pos).cuda()].reshape(fl.size, k * S)
                surv_idx = torch.from_numpy(np.take_along_axis(idx_h[fl], pos, axis=1)).cuda()
                lost_idx = torch.from_numpy(np.take_along_axis(idx_h[fl], lost_pos, axis=1)).cuda()
                out = torch.empty((fl.size, e * S), dtype=torch.uint8, device="cuda")
                c.rebuild(k, m, surv_idx, surv, lost_idx, out)
                have3[flt[:, None], torch.from_numpy(lost_pos).cuda()] = out.view(fl.size, e, S)

            def leg_caller():
                c.check_pair(k, m, idx, have, verdict, x=x, S=S, n=n)
                v = verdict.cpu().numpy().view(np.uint32)  # waits for the check
                live = (v != 0) & (v != ec.VERDICT_INVALID)
                pair = live & ((v >> 25) != 0)
                one = live & ~pair & (((v >> 16) & 0xFF) != 0xFF)
                fl = np.flatnonzero(one)
                if fl.size:
                    shard = ((v[fl] >> 16) & 0xFF).astype(np.uint8)
                    q = np.argmax(idx_h[fl] == shard[:, None], axis=1)
                    others = np.arange(k)[None, :] + (np.arange(k)[None, :] >= q[:, None])  # k positions, not q
                    rebuild_into(fl, others, q.reshape(-1, 1))
                fl = np.flatnonzero(pair)
                if fl.size:
                    lo = ((v[fl] >> 16) & 0xFF).astype(np.uint8)
                    hi = (((v[fl] >> 25) & 0x7F) - 1).astype(np.uint8)
                    q1 = np.argmax(idx_h[fl] == lo[:, None], axis=1)
                    q2 = np.argmax(idx_h[fl] == hi[:, None], axis=1)
                    qa, qb = np.minimum(q1, q2), np.maximum(q1, q2)
                    rebuild_into(fl, input_positions(k, x, qa, qb), np.stack([qa, qb], axis=1))

            legs = {"correct_pair": lambda: c.correct_pair(k, m, idx, have, verdict, x=x, S=S, n=n),
                    "check_pair": lambda: c.check_pair(k, m, idx, have, verdict, x=x, S=S, n=n),
                    "caller": leg_caller,
                    "correct": lambda: c.correct(k, m, idx, have, verdict, x=x, S=S, n=n),
                    "check": lambda: c.check(k, m, idx, have, verdict, x=x, S=S, n=n),
                    "read": lambda: c.stream_probe(kx, 1, have, rout, mode="read")}

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

            for state in STATES[:1] if a.clean_only else STATES:
                want = np.zeros(n, dtype=np.uint32)
                state_v.clear()
                singles = pairs = 0
                if state != "clean":
                    cnt = max(1, n // 100)
                    blocks = np.sort(rng.choice(n, size=cnt, replace=False))
                    if state == "one_1pct":  # one flipped byte in one of the k + x shards in hand
                        pos = rng.integers(0, kx, size=cnt)
                        byte = rng.integers(0, S, size=cnt)
                        mask = np.where(pos < k, (1 << x) - 1, 1 << np.maximum(pos - k, 0))
                        want[blocks] = mask | (idx_h[blocks, pos].astype(np.uint32) << 16) | CORRECTED
                        bl, off = blocks, pos * S + byte
                        singles = cnt
                    else:  # one flipped byte in each of two shards, at different offsets
                        qa = rng.integers(0, kx - 1, size=cnt)
                        qb = rng.integers(0, kx - 1, size=cnt)
                        qb = np.where(qb >= qa, qb + 1, qb)
                        qa, qb = np.minimum(qa, qb), np.maximum(qa, qb)
                        ba, bb = rng.integers(0, S // 2, size=cnt), rng.integers(S // 2, S, size=cnt)
                        ra, rb = np.maximum(qa - k, 0), np.maximum(qb - k, 0)
                        mask = np.where(qa < k, (1 << x) - 1, (1 << ra) | (1 << rb))
                        ia, ib = idx_h[blocks, qa].astype(np.uint32), idx_h[blocks, qb].astype(np.uint32)
                        want[blocks] = (mask | (np.minimum(ia, ib) << 16) | ((np.maximum(ia, ib) + 1) << 25)
                                        | CORRECTED).astype(np.uint32)
                        bl = np.concatenate([blocks, blocks])
                        off = np.concatenate([qa * S + ba, qb * S + bb])
                        pairs = cnt
                    with torch.cuda.stream(st):
                        state_v["blocks"] = torch.from_numpy(bl).cuda()
                        state_v["off"] = torch.from_numpy(off).cuda()
                        state_v["bad"] = clean[state_v["blocks"], state_v["off"]] ^ 0x5A
                with torch.cuda.stream(st):
                    # correctness first: every word and byte of (a), every byte of (c)
                    restore()
                    legs["correct_pair"]()
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
                with torch.cuda.stream(st):  # ... and after the timed legs
                    restore()
                    legs["correct_pair"]()
                    st.synchronize()
                    ok = ok and bool(np.array_equal(verdict.cpu().numpy().view(np.uint32), want)) and \
                        bool(torch.equal(have, clean))
                med = {name: float(np.median(t)) for name, t in ms.items()}
                read_rate = n * kx * S / med["read"] / 1e6   # GB/s
                mended_bytes = (singles * (k + 1) + pairs * (k + 2)) * S
                row = {"code": "RS(%d,%d)" % (k, m), "x": x, "block_bytes": B, "blocks": n, "S": S,
                       "state": state, "words_and_bytes_exact": ok, "single_blocks": singles, "pair_blocks": pairs,
                       "ms": {name: round(t, 4) for name, t in med.items()},
                       "ms_rounds": {name: [round(y, 4) for y in t] for name, t in ms.items()},
                       "read_GBs": round(read_rate, 1),
                       "a_over_b": round(med["correct_pair"] / med["check_pair"], 4),
                       "a_minus_b_ms": round(med["correct_pair"] - med["check_pair"], 4),
                       "a_minus_b_ms_rounds": [round(p - q, 4) for p, q in zip(ms["correct_pair"], ms["check_pair"])],
                       "correct_minus_check_ms": round(med["correct"] - med["check"], 4),
                       "correct_minus_check_ms_rounds": [round(p - q, 4) for p, q in zip(ms["correct"], ms["check"])],
                       "mended_bytes_at_read_rate_ms": round(mended_bytes / read_rate / 1e6, 4),
                       "a_over_c": round(med["correct_pair"] / med["caller"], 4)}
                results.append(row)
                print(json.dumps({f: row[f] for f in row if not f.endswith("_rounds")}), flush=True)
            state_v.clear()
            del idx, clean, have, have3, rout, verdict
            torch.cuda.empty_cache()
    c.close()
    doc = {"tool": "tools/correct_pair_probe.py", "device": torch.cuda.get_device_name(0),
           "build_id": ec.build_id(), "rounds": rounds, "reps": a.reps,
           "timing": "device events around each call, the corrupted shards put back before it; "
                     "median of reps, median over alternated rounds",
           "all_exact": all(r["words_and_bytes_exact"] for r in results), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not doc["all_exact"]:
        sys.exit("correct_pair_probe: a verdict word or a mended byte is not the expected one")


if __name__ == "__main__":
    main()

"""What gs4d_compact_records costs: 10^6 and 10^7 96-byte records at keep fractions 0.05, 0.5 and 0.95, the kept records uniformly
scattered over a synthetic, uploaded statistics table.

Device time: the call is asynchronous and its three kernels run back to back on one frame lane, so a window is `calls` calls between two
gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the fractions taking turns to lead a round.  (The
launch gaps between the kernels are inside that figure; `rocprofv3 --kernel-trace --stats -- python tools/compact_cost.py` gives the kernels alone
and says which of them dominates.)  Against it, in the same run:
  (a) the host round trip that was the only way before: read_record_stats, a numpy mask, rec[mask], Context.buffer — once per fraction and size;
  (b) the bytes the pass moves, 32 n + (2 * 96 + 4) kept (the table is read twice), over the 6.3 TB/s copy ceiling DESIGN.md uses.
Prints one JSON line.  Usage: python tools/compact_cost.py [calls] [rounds] [largest n]."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
gs4d = importlib.import_module("4dgaussiansplatrendering_amd")

STRIDE = 96
FRACTIONS = (0.05, 0.5, 0.95)
COPY_CEILING = 6.3e12                                     # bytes / s: DESIGN.md's HBM copy ceiling


def table(n, frac, seed):
    st = np.zeros(n, gs4d.Context.RECORD_STAT)
    keep = np.random.default_rng(seed).uniform(size=n) < frac
    st["pixels"][keep] = 7
    st["wmax"][keep] = 0.25
    st["wsum"][keep] = 7 << 22
    return st, int(keep.sum())


def window(ctx, call, calls):
    ctx.finish()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    ctx.finish()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(n, calls, rounds):
    ctx = gs4d.Context(64, 64)
    rec = np.arange(n * (STRIDE // 4), dtype=np.float32).reshape(n, STRIDE // 4)
    src = ctx.buffer(rec)
    dst, idx, count = ctx.buffer(nbytes=n * STRIDE), ctx.buffer(nbytes=n * 4), ctx.buffer(nbytes=8)
    cases = {}
    for k, frac in enumerate(FRACTIONS):
        st, kept = table(n, frac, 1000 + k)
        cases[frac] = (ctx.buffer(st), kept)
    rule = dict(min_pixels=1, min_wmax=1.0 / 255.0)
    calls_of = {f: (lambda sb=cases[f][0]: ctx.compact_records(sb, n, src=src, stride=STRIDE, dst=dst, kept_index=idx, count=count, **rule)) for f in FRACTIONS}
    for f in FRACTIONS:                                    # warm-up, and the counts are the tables'
        for _ in range(5):
            calls_of[f]()
        assert ctx.read_compact_count(count) == (cases[f][1], cases[f][1])
    ms = {f: [] for f in FRACTIONS}
    for r in range(rounds):
        for k in range(len(FRACTIONS)):
            f = FRACTIONS[(k + r) % len(FRACTIONS)]
            ms[f].append(window(ctx, calls_of[f], calls))
    out = {}
    for f in FRACTIONS:
        sb, kept = cases[f]
        # (a) the host round trip, once more than is kept: the first one pays for page faults of fresh host memory
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            st = ctx.read_record_stats(sb, n)
            mask = (st["pixels"] >= 1) & (st["wmax"] >= np.float32(1.0 / 255.0))
            pruned = rec[mask]
            nb = ctx.buffer(pruned)
            ctx.finish()
            host.append((time.perf_counter() - t0) * 1e3)
            assert pruned.shape[0] == kept
            ctx.delete(nb)
        dev = float(np.median(ms[f]))
        budget = (32 * n + (2 * STRIDE + 4) * kept) / COPY_CEILING * 1e3
        out[str(f)] = {"kept": kept, "ms_device_call": dev, "ms_host_round_trip": float(np.median(host)), "host_over_device": float(np.median(host)) / dev,
                       "ms_byte_budget": budget, "fraction_of_ceiling": budget / dev, "spread_pct": 100.0 * (max(ms[f]) - min(ms[f])) / dev, "windows": ms[f]}
    ctx.close()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    res = {str(n): measure(n, calls, rounds) for n in (1_000_000, 10_000_000) if n <= largest}
    print(json.dumps({"tool": "compact_cost", "stride": STRIDE, "calls": calls, "rounds": rounds, "records": res}))


if __name__ == "__main__":
    main()

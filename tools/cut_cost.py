"""What gs4d_stat_cut costs: 10^6 and 10^7 statistics rows, each of the three fields, on a synthetic, uploaded table of the kind a
draw leaves (a third of the rows zero, the rest counts, float32 weights and their sums), the budget a quarter of the rows.

Device time as tools/compact_cost.py takes it: the call is asynchronous and its kernels (a histogram and a pick per digit) run back to back on one
frame lane, so a window is `calls` calls between two gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the
fields taking turns to lead a round.  (The launch gaps between the kernels are inside that figure; `rocprofv3 --kernel-trace --stats -- python
tools/cut_cost.py` gives the kernels alone.)  Against it, in the same run:
  (a) the host route that was the only way before: read_record_stats of the whole table and np.partition of the field, once per field and size;
  (b) the bytes the passes move, passes x 16 n (a row's field sits in one 32-byte sector of its 16-byte row), over the 6.3 TB/s copy ceiling
      DESIGN.md uses.
Prints one JSON line.  Usage: python tools/cut_cost.py [calls] [rounds] [largest n]."""
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

FIELDS = ("pixels", "wmax", "wsum")
PASSES = {"pixels": 4, "wmax": 4, "wsum": 8}              # 8-bit digits (CUT_DIGIT_BITS)
COPY_CEILING = 6.3e12                                     # bytes / s: DESIGN.md's HBM copy ceiling


def table(n, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros(n, gs4d.Context.RECORD_STAT)
    shown = rng.uniform(size=n) < 2.0 / 3.0
    m = int(shown.sum())
    w = (1.0 - rng.uniform(0.0, 1.0, m)).astype(np.float32)
    px = rng.integers(1, 4000, m)
    st["pixels"][shown] = px
    st["wmax"][shown] = w
    st["wsum"][shown] = px.astype(np.uint64) * np.rint(w.astype(np.float64) * 0.3 * (1 << 24)).astype(np.uint64)
    return st


def host_cut(st, field, k):
    """the numpy route: (value, above, equal)"""
    f = st[field].view(np.uint32) if field == "wmax" else st[field]
    v = np.partition(f, f.size - k)[f.size - k]
    return int(v), int((f > v).sum()), int((f == v).sum())


def window(ctx, call, calls):
    ctx.finish()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    ctx.finish()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(n, calls, rounds):
    ctx = gs4d.Context(64, 64)
    st = table(n, 2000 + n % 977)
    sb, k = ctx.buffer(st), n // 4
    outs = {f: ctx.buffer(nbytes=16) for f in FIELDS}
    calls_of = {f: (lambda f=f: ctx.stat_cut(sb, n, k, f, out=outs[f])) for f in FIELDS}
    for f in FIELDS:                                       # warm-up, and the results are the table's
        for _ in range(5):
            calls_of[f]()
        assert ctx.read_stat_cut(outs[f]) == host_cut(st, f, k), f
    ms = {f: [] for f in FIELDS}
    for r in range(rounds):
        for j in range(len(FIELDS)):
            f = FIELDS[(j + r) % len(FIELDS)]
            ms[f].append(window(ctx, calls_of[f], calls))
    out = {}
    for f in FIELDS:
        host = []                                          # (a) once more than is kept: the first one pays for page faults of fresh host memory
        for _ in range(3):
            t0 = time.perf_counter()
            got = host_cut(ctx.read_record_stats(sb, n), f, k)
            host.append((time.perf_counter() - t0) * 1e3)
            assert got == ctx.read_stat_cut(outs[f])
        dev = float(np.median(ms[f]))
        budget = PASSES[f] * 16 * n / COPY_CEILING * 1e3
        out[f] = {"passes": PASSES[f], "ms_device_call": dev, "ms_host_route": float(np.median(host)), "host_over_device": float(np.median(host)) / dev,
                  "ms_byte_budget": budget, "fraction_of_ceiling": budget / dev, "spread_pct": 100.0 * (max(ms[f]) - min(ms[f])) / dev, "windows": ms[f]}
    ctx.close()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    res = {str(n): measure(n, calls, rounds) for n in (1_000_000, 10_000_000) if n <= largest}
    print(json.dumps({"tool": "cut_cost", "calls": calls, "rounds": rounds, "budget": "n / 4", "rows": res}))


if __name__ == "__main__":
    main()

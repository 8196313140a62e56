#!/usr/bin/env python3
"""Host cost of a record-set call: CALLS back-to-back gs4d_slice_records calls at n = 1024 followed by one gs4d_finish, then the same for
gs4d_count_neighbours with a source table and a rule (the longest operand list with a settled and a scanned table).  The clock is the host's,
around the calls and the finish, so a figure is the larger of what the host needs to check and queue a call and what the device needs to run it.
Prints one JSON line; profiles/r10_operand_host_cost.md has the method and the figures.

    python tools/operand_host_cost.py [--calls 10000] [--label NAME]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10_000)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
    import scenes
    n = 1024
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    ctx = gs4d.Context(64, 64)
    lib, h = gs4d._lib, ctx._h
    src, dst = ctx.buffer(rec), ctx.buffer(nbytes=n * 96)
    source, stats = ctx.record_stats(n), ctx.record_stats(n)
    sl, nq, rule = gs4d.slice_query(0.0), gs4d.neighbour_query(0.5, cap=1), gs4d._keep_rule(min_pixels=0)
    slq, nqq, rp = C.byref(sl), C.byref(nq), gs4d._ptr(rule)

    def timed(call):
        for _ in range(a.calls // 10):              # warm-up: code objects, the lane's scratch
            assert call() == 0, lib.gs4d_last_error(h)
        ctx.finish()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            rc = call()
        ctx.finish()
        t1 = time.perf_counter()
        assert rc == 0
        return (t1 - t0) / a.calls * 1e6

    out = {"label": a.label, "calls": a.calls, "n": n,
           "slice_records_us_per_call": round(timed(lambda: lib.gs4d_slice_records(h, src, n, slq, dst, 0)), 3),
           "count_neighbours_us_per_call": round(timed(lambda: lib.gs4d_count_neighbours(h, src, n, nqq, source, rp, stats)), 3)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What gs4d_measure_records costs: 10^6 and 10^7 96-byte records of the 4D variant of the benchmark's cube set (scenes.cube_params_4d),
measured whole (no table) and through a table that selects 0 %, 1 %, 50 % and 100 % of them, the selected records spread evenly over the set.

Device time of the call: it is asynchronous and its three kernels run back to back with the next call's on one frame lane, so a window is `calls`
calls between two gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the cases taking turns to lead a
round.  Such a window is CACHE-WARM: the same buffers are read call after call, and a 160 MB table, or the pieces of 10^6 records, fit the 256 MB
last-level cache.  So every case is also timed COLD (`cold_ms`): one call between two gs4d_finish, after a device copy of 2 x 384 MB of other memory
(gs4d_transform_records of a scratch set) has gone through the cache; median of `cold repeats` such calls.  That host clock also holds what issuing
one call and waiting for it costs, which `cold_floor_ms` (the same call on 256 records) reports.

What the figure is a share of (`ms_useful_bytes`): the HBM time, at the 6.3 TB/s copy ceiling DESIGN.md uses, of the 16 n bytes of the table (none
without one) plus the record pieces of the selected records — five 16-byte pieces in the box kernel, two in the cell kernel (the alpha piece is
not read: no GS4D_MS_SKIP_HIDDEN here), and the table a second time: 32 n + 112 s bytes with a table, 112 n without.  The pieces of a record lie in
both 64-byte halves of its 96 bytes, so the hardware moves most of 96 bytes per selected record and kernel whatever is done.

And the route the call replaces, on the same machine: gs4d_buffer_read of the records and the table, gs4d_host_measure_records.
shadow_builds must not move.
Prints one JSON line.  Usage: python tools/measure_cost.py [calls] [rounds] [largest n] [host repeats] [cold repeats]."""
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
gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
import scenes  # noqa: E402
from centres_cost import COPY_CEILING, FLUSH_RECORDS, cold, records_of, turns, window  # noqa: E402

T = 25.0
SHARES = {"table_0": 0, "table_1": 1, "table_50": 50, "table_100": 100}      # per cent selected


def table_for(n, per_cent):
    """a RECORD_STAT table whose rule {1, 0, 0} selects per_cent of the rows, evenly spread"""
    st = np.zeros(n, gs4d.RECORD_STAT)
    if per_cent:
        st["pixels"][(np.arange(n, dtype=np.int64) * per_cent) % 100 < per_cent] = 1
    return st


def measure(n, calls, rounds, host_repeats, cold_repeats):
    print(f"measure_cost: {n} records", file=sys.stderr, flush=True)
    rec = records_of("symmetric4d", n)
    ctx = gs4d.Context(64, 48)
    data = ctx.buffer(rec)
    out = ctx.buffer(nbytes=96)
    tables = {name: table_for(n, pc) for name, pc in SHARES.items()}
    bufs = {name: ctx.buffer(t) for name, t in tables.items()}
    scratch, scratch_out = ctx.buffer(nbytes=96 * FLUSH_RECORDS), ctx.buffer(nbytes=96 * FLUSH_RECORDS)
    identity = ctx.buffer(gs4d.affine4())

    def flush():
        ctx.transform_records(scratch, FLUSH_RECORDS, identity, 1, scratch_out)

    do = {"whole": lambda: ctx.measure_records(data, n, t=T, out=out)}
    for name in SHARES:
        do[name] = lambda name=name: ctx.measure_records(data, n, t=T, stats=bufs[name], out=out, min_pixels=1)
    selected = {}
    for name, call in do.items():                                                        # warm-up, the bits, and how many each case measures
        call()
        got = ctx.read(out, np.uint8, 96).tobytes()
        want = gs4d.measure_records_host(rec, t=T, stats=tables.get(name), **({"min_pixels": 1} if name in tables else {}))
        assert got == bytes(want), f"{name}: the device and the host definition differ"
        selected[name] = int(want.count)
    res = turns(do, rounds, lambda call: window(ctx, call, calls))
    for name in do:
        useful = 112 * n if name == "whole" else 32 * n + 112 * selected[name]
        b = useful / COPY_CEILING * 1e3
        res[name].update(selected=selected[name], selected_pct=100.0 * selected[name] / n, ms_useful_bytes=b, fraction_of_ceiling=b / res[name]["ms"])
        if cold_repeats:
            res[name]["cold_ms"], res[name]["cold_runs"] = cold(ctx, flush, do[name], cold_repeats)
    if cold_repeats:
        res["cold_floor_ms"], _ = cold(ctx, flush, lambda: ctx.measure_records(data, 256, t=T, out=out), cold_repeats)
    res["shadow_builds"] = ctx.shadow_builds(data)
    assert res["shadow_builds"] == 0
    if host_repeats:
        parts = {"buffer_read": [], "measure_records_host": [], "total": []}
        for _ in range(host_repeats):
            ctx.finish()
            t0 = time.perf_counter()
            back = ctx.read(data, np.float32, n * 24)
            table = ctx.read(bufs["table_50"], gs4d.RECORD_STAT, n)
            t1 = time.perf_counter()
            m = gs4d.measure_records_host(back, t=T, stats=table, min_pixels=1)
            t2 = time.perf_counter()
            for key, v in zip(parts, (t1 - t0, t2 - t1, t2 - t0)):
                parts[key].append(v * 1e3)
        assert int(m.count) == selected["table_50"]
        res["host_route_table_50"] = {key: {"ms": float(np.median(v)), "runs": v} for key, v in parts.items()}
        res["host_route_over_call"] = res["host_route_table_50"]["total"]["ms"] / res["table_50"]["ms"]
    ctx.close()
    return res


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    host_repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    cold_repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 9
    res = {str(n): measure(n, calls, rounds, host_repeats, cold_repeats) for n in (1_000_000, 10_000_000) if n <= largest}
    print(json.dumps({"tool": "measure_cost", "calls": calls, "rounds": rounds, "cold_repeats": cold_repeats, "records": res}))


if __name__ == "__main__":
    main()

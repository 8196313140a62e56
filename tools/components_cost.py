"""What gs4d_label_components and gs4d_count_labels cost: 10^6 and 10^7 96-byte records of the benchmark's cube set (bench.py,
scenes.cube_params: static 3D splats, uniform in [-200, 200]^3), the radii of tools/neighbours_cost.py (a mean of about 1, 8 and 64 neighbours),
every record a member.  Per radius, on the same buffers:

  neighbours_uncapped   (a) the yardstick: gs4d_count_neighbours with the same radius and no cap — the link kernel does that call's walk plus the unions
  labels                gs4d_label_components without a table (grid phases, init, link, flatten)
  labels_sizes          ... with a table and no cap (a memset, the size and the row kernels more)
  count_labels          gs4d_count_labels of those labels with a 1 % seed table

and what the labels are (`components`, `largest`, `singletons_pct`).  Device time as in neighbours_cost.py: windows of `calls` back-to-back calls
between two gs4d_finish, medians of `rounds` windows, the cases taking turns to lead.

(b) The routes the calls replace, on the same machine.  Select connected: the host loop of grow_selection calls from one seed, each step with
the blocking read-back of a count that notices the fixed point (`grow_loop`: at most `grow steps` steps are run; ms per step, the steps done and
whether the fixed point was reached — a thin object takes as many steps as it is long).  Floater clumps: gs4d_buffer_read of the records,
label_components_host — the double loop, on a sample of `host sample` records, scaled by (n / sample)^2 — and gs4d_buffer_subdata of the table.

Every window ends in gs4d_finish, which raises on a device fault or a device-side check (a union-find trip bound among them): the tool then ends
with that error and starts nothing more.  Run it under a time limit (`timeout -k 10 900 python tools/components_cost.py ...`).  shadow_builds
must not move.  Prints one JSON line.  Usage: python tools/components_cost.py [calls] [rounds] [largest n] [host sample] [grow steps]."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
import scenes  # noqa: E402
from neighbours_cost import MEANS, W, H, one_pct_table, radius_for, turns, window  # noqa: E402


def measure(n, calls, rounds, host_sample, grow_steps):
    print(f"components_cost: {n} records", file=sys.stderr, flush=True)
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    ctx = gs4d.Context(W, H)
    data, seeds, stats = ctx.buffer(rec), ctx.buffer(one_pct_table(n)), ctx.record_stats(n)
    labels = ctx.buffer(nbytes=4 * n)
    out = {}
    for mean in MEANS:
        r = radius_for(n, mean)
        do = {
            "neighbours_uncapped": lambda: ctx.count_neighbours(stats, n, data, r),
            "labels": lambda: ctx.label_components(n, data, r, labels=labels),
            "labels_sizes": lambda: ctx.label_components(n, data, r, labels=labels, stats=stats),
            "count_labels": lambda: ctx.count_labels(stats, n, labels, seeds, min_pixels=1),
        }
        for name in do:                                         # warm-up; "labels" comes before "count_labels"
            do[name]()
        ctx.finish()
        lab = ctx.read(labels, np.uint32, n)
        size = np.bincount(lab[lab != gs4d.ID_NONE].astype(np.int64))
        size = size[size > 0]
        res = turns(do, rounds, lambda f: window(ctx, f, calls))
        res["radius"] = r
        res["components"], res["largest"], res["singletons_pct"] = int(size.size), int(size.max()), 100.0 * float((size == 1).sum()) / n
        res["labels_over_neighbours"] = res["labels"]["ms"] / res["neighbours_uncapped"]["ms"]
        if grow_steps:
            res["grow_loop"] = grow_loop(ctx, data, n, r, int(lab[n // 2]), lab, grow_steps)
        out[f"mean{mean}"] = res
    assert ctx.shadow_builds(data) == 0
    if host_sample:
        out["host_route_mean8"] = host_route(ctx, data, stats, n, host_sample)
        out["host_route_over_call"] = out["host_route_mean8"]["total_ms_scaled"] / out["mean8"]["labels_sizes"]["ms"]
    ctx.close()
    return out


def grow_loop(ctx, data, n, r, seed, lab, max_steps):
    """the route select_connected replaces: grow_selection from one seed until the count stops growing, a blocking read-back per step"""
    table = np.zeros(n, gs4d.RECORD_STAT)
    table["pixels"][seed] = 1
    source = ctx.buffer(table)
    ctx.finish()
    t0 = time.perf_counter()
    have, steps, fixed = 1, 0, False
    while steps < max_steps:
        grown = ctx.grow_selection(n, data, source, r)
        count = ctx.compact_records(grown, n, min_pixels=1)
        now = ctx.read_compact_count(count)[0]
        ctx.delete(count)
        ctx.delete(source)
        source, steps = grown, steps + 1
        if now == have:
            fixed = True
            break
        have = now
    ms = (time.perf_counter() - t0) * 1e3
    ctx.delete(source)
    return {"steps": steps, "reached_fixed_point": fixed, "selected": int(have), "component": int((lab == lab[seed]).sum()), "ms": ms, "ms_per_step": ms / steps}


def host_route(ctx, data, stats, n, sample):
    """read back, the host definition on `sample` records scaled to n, upload; ms"""
    ctx.finish()
    t0 = time.perf_counter()
    back = ctx.read(data, np.float32, n * 24)
    t1 = time.perf_counter()
    m = min(sample, n)
    gs4d.label_components_host(back.reshape(-1, 24)[:m], radius_for(n, 8))
    t2 = time.perf_counter()
    ctx.subdata(stats, np.zeros(n, gs4d.RECORD_STAT))
    ctx.finish()
    t3 = time.perf_counter()
    host_scaled = (t2 - t1) * 1e3 * (n / m) ** 2
    return {"buffer_read_ms": (t1 - t0) * 1e3, "host_sample": m, "host_ms_sample": (t2 - t1) * 1e3, "host_ms_scaled": host_scaled,
            "buffer_subdata_ms": (t3 - t2) * 1e3, "total_ms_scaled": (t1 - t0 + t3 - t2) * 1e3 + host_scaled}


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    host_sample = int(sys.argv[4]) if len(sys.argv) > 4 else 20000
    grow_steps = int(sys.argv[5]) if len(sys.argv) > 5 else 32
    res = {str(n): measure(n, calls, rounds, host_sample, grow_steps) for n in (1_000_000, 10_000_000) if n <= largest}
    print(json.dumps({"tool": "components_cost", "calls": calls, "rounds": rounds, "records": res}))


if __name__ == "__main__":
    main()

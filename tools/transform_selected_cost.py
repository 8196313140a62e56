"""What gs4d_transform_selected costs: 10^6 and 10^7 records with 1 %, 50 % and 100 % of them selected — scattered over the set, and
as one contiguous run; scattered also at 5, 12.5 and 25 %, the densities around which a wave changes its store path — moved in place under a rigid
map about a pivot, against its two yardsticks on the same machine: gs4d_transform_records of the full set into a second buffer (the same 192 bytes
per record at 100 %), and the host route (read the records back, gs4d_host_transform_records, upload them again; 10^6 records, three times).

Device time of the call: it is asynchronous and its kernel runs back to back on one frame lane, so a window is `calls` calls between two gs4d_finish,
and the time of a call is the window over `calls`; medians of `rounds` windows, the shapes taking turns to lead a round.  The byte budget of a call is
16 n for the table plus 192 per selected record over the 6.3 TB/s copy ceiling DESIGN.md uses (a scattered selection moves whole 128-byte lines for
96-byte records, which the budget does not count).  One shape is also run with the pivot taken from a measurement on the device.
Run it once per build of the library, each in a process of its own, to compare the shipped staged store with `make lib XFSEL_PLAIN=1`; `label` says
which one the line is for.  Prints one JSON line.  Usage: python tools/transform_selected_cost.py [label] [calls] [rounds] [largest n]."""
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

COPY_CEILING = 6.3e12                                     # bytes / s: DESIGN.md's HBM copy ceiling
SIZES = (1_000_000, 10_000_000)
SELECTIONS = (("scattered", 0.01), ("run", 0.01), ("scattered", 0.05), ("scattered", 0.125), ("scattered", 0.25), ("scattered", 0.5), ("run", 0.5), ("all", 1.0))
RIGID = dict(q_wxyz=(0.9393727, 0.1496044, 0.2992088, -0.0748022), translate=(0.5, -0.25, 0.125))      # 0.7 rad about (1, 2, -0.5)
PIVOT = (1.0, -2.0, 3.0)


def window(ctx, call, calls):
    ctx.finish()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    ctx.finish()
    return (time.perf_counter() - t0) * 1e3 / calls


def records(n):
    pos4, q4, sc4, life, fade, vel, rgba4 = scenes.cube_params_4d(n)
    return gs4d.build_records_4d(pos4, q4, sc4, life, fade, vel, rgba4)


def table(n, pattern, fraction, seed=0x5853):
    """a RECORD_STAT table whose rows pass min_pixels = 1 for `fraction` of the n records"""
    st = np.zeros(n, gs4d.RECORD_STAT)
    if pattern == "scattered":
        st["pixels"] = np.random.default_rng(seed).random(n) < fraction
    else:
        k = int(round(n * fraction))
        st["pixels"][n // 3:n // 3 + k] = 1
    return st


def measure_calls(calls, rounds, largest):
    sizes = [n for n in SIZES if n <= largest]
    ctx = gs4d.Context(64, 64)
    rec = records(max(sizes))
    data, dst = ctx.buffer(rec), ctx.buffer(nbytes=96 * max(sizes))
    xf = gs4d.affine4(**RIGID)
    xfb = ctx.buffer(xf)
    x = gs4d.selection_xf(xf, pivot=PIVOT)
    do, selected = {}, {}
    for n in sizes:
        for pattern, fraction in SELECTIONS:
            name = f"{n}:{pattern}:{fraction:g}"
            if pattern == "all":
                do[name], selected[name] = (lambda n=n: ctx.transform_selected(data, n, x)), n
                continue
            st = table(n, pattern, fraction)
            sb = ctx.buffer(st)
            do[name], selected[name] = (lambda n=n, sb=sb: ctx.transform_selected(data, n, x, stats=sb, min_pixels=1)), int((st["pixels"] > 0).sum())
            if (pattern, fraction) == ("scattered", 0.5):
                mb = ctx.measure_records(data, n, t=25.0, stats=sb, min_pixels=1)
                xm = gs4d.selection_xf(xf, measure=True)
                do[name + ":measured_pivot"] = lambda n=n, sb=sb, mb=mb, xm=xm: ctx.transform_selected(data, n, xm, stats=sb, measure=mb, min_pixels=1)
                selected[name + ":measured_pivot"] = selected[name]
        do[f"{n}:transform_records"], selected[f"{n}:transform_records"] = (lambda n=n: ctx.transform_records(data, n, xfb, 1, dst=dst)), n
    for call in do.values():
        call()
    names = list(do)
    ms = {name: [] for name in names}
    for r in range(rounds):
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            ms[name].append(window(ctx, do[name], calls))
    res = {}
    for name in names:
        n = int(name.split(":")[0])
        v = ms[name]
        table_bytes = 0 if name.endswith(":all:1") or name.endswith("transform_records") else 16 * n
        budget = (table_bytes + 192 * selected[name]) / COPY_CEILING * 1e3
        med = float(np.median(v))
        res[name] = {"selected": selected[name], "ms": med, "spread_pct": 100.0 * (max(v) - min(v)) / med, "windows": v, "ms_byte_budget": budget,
                     "fraction_of_ceiling": budget / med}
    # the host route at 10^6: read back, transform on the host, upload
    n = min(sizes)
    host = []
    for _ in range(3):
        ctx.finish()
        t0 = time.perf_counter()
        back = ctx.read(data, np.float32, n * 24)
        ctx.subdata(data, gs4d.transform_records_host(back, xf))
        ctx.finish()
        host.append((time.perf_counter() - t0) * 1e3)
    res[f"{n}:host_route"] = {"ms": float(np.median(host)), "windows": host}
    ctx.close()
    return res


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "shipped"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    largest = int(sys.argv[4]) if len(sys.argv) > 4 else 10_000_000
    print(json.dumps({"tool": "transform_selected_cost", "build": label, "calls": calls, "rounds": rounds, "records": measure_calls(calls, rounds, largest)}))


if __name__ == "__main__":
    main()

"""What gs4d_shade_sh_t and gs4d_collapse_sh cost: 10^6 and 10^7 96-byte records of the benchmark's cube set (bench.py,
scenes.cube_params) with random coefficients and minimal rows — degree 3 at degree_t 0, 1, 2 and degrees 0 .. 2 at degree_t 2 — and, in the same
run, gs4d_shade_sh at the same degree on a 3DGS table and gs4d_copy_rows of a table of the same row bytes (the floor: the row read once and written
once, so half of it is what reading the rows must cost).

Device time of a call: it is asynchronous and its kernels run back to back on one frame lane, so a window is `calls` calls between two gs4d_finish,
and the time of a call is the window over `calls`; medians of `rounds` windows, the entries taking turns to lead a round, every entry warmed up
first.  The byte budget of a shade is n * (row + 64 + 32) — the row, the record's two 32-byte sectors read, its one sector written — over the 6.3
TB/s copy ceiling DESIGN.md uses; the issue's byte ratio to gs4d_shade_sh, (row + 32 + 12) / (row of the 3DGS table + 32 + 12), is printed beside
the measured one.
Tables and records above 10^6 rows are uploaded as repeats of a block of 10^6, so the host never holds more than that.
Prints one JSON line.  Usage: python tools/shade_sh_t_cost.py [calls] [rounds] [largest n]."""
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
BLOCK = 1_000_000
CASES = ((3, 0), (3, 1), (3, 2), (0, 2), (1, 2), (2, 2))  # (degree, degree_t)
T, INV_PERIOD = 0.3, 0.25


def window(ctx, call, calls):
    ctx.finish()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    ctx.finish()
    return (time.perf_counter() - t0) * 1e3 / calls


def turns(do, rounds, run):
    """medians of `rounds` windows of every entry of `do`, the entries taking turns to lead"""
    names = list(do)
    ms = {name: [] for name in names}
    for r in range(rounds):
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            ms[name].append(run(do[name]))
    return {name: {"ms": float(np.median(v)), "spread_pct": 100.0 * (max(v) - min(v)) / float(np.median(v)), "windows": v} for name, v in ms.items()}


def repeated(ctx, block, n):
    """a buffer of n rows: `block` (at most BLOCK rows) over and over"""
    row = block.nbytes // block.shape[0]
    buf = ctx.buffer(nbytes=n * row)
    for first in range(0, n, block.shape[0]):
        count = min(block.shape[0], n - first)
        ctx.subdata(buf, block[:count], offset=first * row)
    return buf


def random_rows(rows, nbytes, seed):
    out = np.zeros((rows, nbytes // 4), np.float32)
    out[:] = np.random.default_rng(seed).random(out.shape, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)
    return out


def measure(n, calls, rounds):
    pos, q, scale, rgba = scenes.cube_params(min(n, BLOCK))
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    cam = scenes.CAM_CUBE[0]
    ctx = gs4d.Context(64, 64)
    data = repeated(ctx, rec, n)                                                         # never drawn: no shadow, records only
    out = {}
    for degree, degree_t in CASES:
        row_t, row = gs4d.sh_row_bytes_t(degree, degree_t), gs4d.sh_row_bytes(degree)
        sh_t = repeated(ctx, random_rows(min(n, BLOCK), row_t, 0x5368 + 4 * degree + degree_t), n)
        sh = repeated(ctx, random_rows(min(n, BLOCK), row, 0x5369 + degree), n)
        copy_dst, rows_dst = ctx.buffer(nbytes=n * row_t), ctx.buffer(nbytes=n * row)
        do = {
            "shade_sh_t": lambda: ctx.shade_sh_t(data, n, sh_t, degree, degree_t, T, INV_PERIOD, cam),
            "collapse_sh": lambda: ctx.collapse_sh(data, n, sh_t, degree, degree_t, T, INV_PERIOD, dst=rows_dst),
            "shade_sh": lambda: ctx.shade_sh(data, n, sh, degree, T, cam),
            "copy_rows": lambda: ctx.copy_rows(sh_t, n, row_t, dst=copy_dst),
        }
        for call in do.values():
            call()
        res = turns(do, rounds, lambda call: window(ctx, call, calls))
        shade_t, shade, copy = res["shade_sh_t"]["ms"], res["shade_sh"]["ms"], res["copy_rows"]["ms"]
        budget = n * (row_t + 64 + 32) / COPY_CEILING * 1e3
        res.update(row_bytes=row_t, row_bytes_3dgs=row, ms_byte_budget=budget, fraction_of_ceiling=budget / shade_t,
                   over_shade_sh=shade_t / shade, byte_ratio_to_shade_sh=(row_t + 32 + 12) / (row + 32 + 12),
                   over_copy_rows=shade_t / copy, collapse_over_copy_rows=res["collapse_sh"]["ms"] / copy)
        out[f"degree {degree}, degree_t {degree_t}"] = res
        for b in (sh_t, sh, copy_dst, rows_dst):
            ctx.delete(b)
    ctx.close()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    res = {str(n): measure(n, calls, rounds) for n in (1_000_000, 10_000_000) if n <= largest}
    print(json.dumps({"tool": "shade_sh_t_cost", "calls": calls, "rounds": rounds, "records": res}))


if __name__ == "__main__":
    main()

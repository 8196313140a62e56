"""What gs4d_merge_rows costs beside gs4d_merge_records of the same set in the same run.

Calls: 10^6 and 10^7 records of the benchmark's cube set (scenes.cube_params: BASELINE.json configs[1] / configs[2]) under cell grids whose edge gives
a mean of about 2, 8 and 64 members per group; gs4d_merge_records writes the merged records and member_group, and gs4d_merge_rows merges a table of
3, 12, 27 and 48 words per row (SH degree 0 .. 3 at the minimal strides 16, 48, 112, 192) under that member_group, weighted by the records.  Both
calls run the same key kernel, sort and run starts and a scattered gather behind them — 96 bytes per member for the records, the row for the table —
so every entry is printed beside the record merge of its set, and beside the bytes the call must move, n * (roundup16(4 * width) + weight bytes) +
groups * stride (weight bytes: the mass word the key kernel leaves per record, or the 96-byte record in a ROWS_MASS_RECOMPUTE build).  Each call is
also timed with an output that holds no row, which skips the reduction kernel alone: the difference is the reduction's share.  Device time of a
call: it is asynchronous and its kernels run back to back with the next on one frame lane, so a window is `calls` calls between two gs4d_finish, and
the time of a call is the window over `calls`; medians of `rounds` windows after a warm-up call of every entry, the entries of one n taking turns to
lead a round.  Prints one JSON line.  Usage: python tools/merge_rows_cost.py [calls] [rounds] [largest n] [weight bytes]."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
import scenes  # noqa: E402
from merge_cost import MEMBERS, SIZES, grid_for, turns, window  # noqa: E402

WIDTHS = (3, 12, 27, 48)


def measure(calls, rounds, largest, weight_bytes):
    res = {}
    for n in [s for s in SIZES if s <= largest]:
        pos, q, scale, rgba = scenes.cube_params(n)
        rec = gs4d.build_records_3d(pos, q, scale, rgba)
        del pos, q, scale, rgba
        ctx = gs4d.Context(64, 64)
        src = ctx.buffer(rec)
        del rec
        count, none = ctx.buffer(nbytes=16), ctx.buffer(nbytes=16)
        block = np.random.default_rng(7).normal(0.0, 1.0, (1 << 16, 48)).astype(np.float32)
        tables = {}
        for width in WIDTHS:
            stride = (4 * width + 15) // 16 * 16
            t = np.zeros((1 << 16, stride // 4), np.float32)
            t[:, :width] = block[:, :width]
            tables[width] = (ctx.buffer(np.ascontiguousarray(np.resize(t, (n, stride // 4)))), stride)
        do, facts = {}, {}
        for m in MEMBERS:
            grid, cells = grid_for(n, m)
            labels = ctx.cell_labels(src, n, grid)
            member_group = ctx.buffer(nbytes=4 * n)
            ctx.merge_records(src, n, labels, dst=none, member_group=member_group, count=count)
            g = int(ctx.read_merge_count(count)["groups"])
            dst = ctx.buffer(nbytes=96 * max(1, g))                # (a buffer of exactly the merged set, as tools/merge_cost.py times it)
            do[f"{n}:m{m}:merge_records"] = lambda labels=labels, dst=dst: ctx.merge_records(src, n, labels, dst=dst, count=count)
            do[f"{n}:m{m}:merge_records:no_reduction"] = lambda labels=labels: ctx.merge_records(src, n, labels, dst=none, count=count)
            for width in WIDTHS:
                table, stride = tables[width]
                out = ctx.buffer(nbytes=max(16, g * stride))
                name = f"{n}:m{m}:merge_rows:w{width}"
                do[name] = lambda mg=member_group, table=table, stride=stride, width=width, out=out: ctx.merge_rows(mg, n, table, stride, width, data=src, dst=out, count=count)
                # (dst_first 1 with a dst of 16 bytes: no row lies below the capacity, the reduction is not launched)
                do[name + ":no_reduction"] = lambda mg=member_group, table=table, stride=stride, width=width: ctx.merge_rows(mg, n, table, stride, width, data=src, dst=none, dst_first=1, count=count)
                facts[name] = {"groups": g, "stride": stride, "must_move_bytes": n * ((4 * width + 15) // 16 * 16 + weight_bytes) + g * stride}
        for call in do.values():
            call()
        out = turns(do, rounds, lambda call: window(ctx, call, calls))
        for m in MEMBERS:
            merge = out[f"{n}:m{m}:merge_records"]["ms"]
            merge_red = merge - out[f"{n}:m{m}:merge_records:no_reduction"]["ms"]
            out[f"{n}:m{m}:merge_records"]["reduction_ms"] = merge_red
            for width in WIDTHS:
                name = f"{n}:m{m}:merge_rows:w{width}"
                e = out[name]
                e.update(facts[name])
                e["reduction_ms"] = e["ms"] - out[name + ":no_reduction"]["ms"]
                e["over_merge_records"] = e["ms"] / merge
                e["reduction_over_merge_records_reduction"] = e["reduction_ms"] / merge_red if merge_red > 0 else None
                e["reduction_gb_per_s"] = e["must_move_bytes"] / (e["reduction_ms"] * 1e6) if e["reduction_ms"] > 0 else None
        res.update(out)
        ctx.close()
    return res


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    weight_bytes = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    print(json.dumps({"tool": "merge_rows_cost", "calls": calls, "rounds": rounds, "weight_bytes": weight_bytes, "records": measure(calls, rounds, largest, weight_bytes)}))


if __name__ == "__main__":
    main()

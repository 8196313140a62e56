"""What gs4d_cell_labels + gs4d_merge_records cost, and what the coarser sets buy.

Calls: 10^6 and 10^7 records of the benchmark's cube set (scenes.cube_params: BASELINE.json configs[1] / configs[2]) merged over cell grids whose
edge gives a mean of about 2, 8 and 64 members per group, beside gs4d_cell_labels alone and beside gs4d_spatial_order + gs4d_gather_records of the
same set — that pair runs the library's sort of n keys and the same scattered reads of 96-byte records, and writes n records where a merge writes
n / members: it is the yardstick for whether the reduction kernel, and not the sort, dominates a merge.  Device time of a call: it is asynchronous
and its kernels run back to back with the next on one frame lane, so a window is `calls` calls between two gs4d_finish, and the time of a call is the
window over `calls`; medians of `rounds` windows, the entries of one n taking turns to lead a round.
Frames: the 1080p frame (clear, keygen, sort, draw at the benchmark camera) of the full set and of every merged set, `frames` frames per window.
Pictures: the mean absolute difference per pixel and colour channel (L1, colours in 0 .. 1) between the picture of every merged set and the picture of
the full set, at the benchmark camera and from 4 x its distance.  No test holds these to a threshold: there is no reference for them.
Prints one JSON line.  Usage: python tools/merge_cost.py [calls] [rounds] [largest n] [frames]."""
import importlib
import itertools
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

W, H = 1920, 1080
SIZES = (1_000_000, 10_000_000)
MEMBERS = (2, 8, 64)                                      # members per group the cell edges aim at
SIDE = 400.0                                              # the cube is [-200, 200]^3


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


def grid_for(n, members):
    """the grid of cubic cells over the cube that holds about `members` records per cell"""
    cells = max(1, int(round((n / members) ** (1.0 / 3.0))))
    return gs4d.cell_grid((-SIDE / 2,) * 3, SIDE / cells, (cells,) * 3), cells


def picture(ctx, data, n, keys, idx, cam):
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=gs4d.look_at(cam[0], cam[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
    frame(ctx, data, n, keys, idx, cam)
    return ctx.read_pixels()[:, :, :3].astype(np.float64)


def frame(ctx, data, n, keys, idx, cam):
    ctx.clear()
    ctx.keygen(data, 0.0, cam[0], keys, idx, n)
    ctx.sort_pairs(keys, idx, n)
    ctx.bind(1, idx)
    ctx.bind(2, data)
    ctx.draw_instanced(n)


def measure(calls, rounds, largest, frames):
    res = {}
    near = scenes.CAM_CUBE
    far = (tuple(4.0 * v for v in near[0]), near[1])
    for n in [s for s in SIZES if s <= largest]:
        pos, q, scale, rgba = scenes.cube_params(n)
        rec = gs4d.build_records_3d(pos, q, scale, rgba)
        del pos, q, scale, rgba
        ctx = gs4d.Context(W, H)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_mode(gs4d.MODE_4D_SORTED)
        src = ctx.buffer(rec)
        del rec
        keys, idx = ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
        order, gathered = ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=96 * n)
        count = ctx.buffer(nbytes=16)
        full = {cam: picture(ctx, src, n, keys, idx, c) for cam, c in (("near", near), ("far", far))}
        sets, do = {}, {}
        for m in MEMBERS:
            grid, cells = grid_for(n, m)
            labels = ctx.cell_labels(src, n, grid)
            # twice: a call that can write nothing counts the groups, then the set goes into a buffer of exactly that many records (a draw
            # packs the whole buffer into its shadow, so the merged set gets a buffer of its own size)
            small = ctx.buffer(nbytes=16)
            ctx.merge_records(src, n, labels, dst=small, count=count)
            g = int(ctx.read_merge_count(count)["groups"])
            ctx.delete(small)
            dst, _ = ctx.merge_records(src, n, labels, dst=ctx.buffer(nbytes=96 * max(1, g)), count=count)
            c = ctx.read_merge_count(count)
            assert int(c["written"]) == g
            sets[m] = (dst, g)
            res[f"{n}:set:m{m}"] = {"cells_per_axis": cells, "groups": int(c["groups"]), "members": int(c["members"]), "left_out": int(c["left_out"]),
                                    "l1_near": float(np.abs(picture(ctx, dst, g, keys, idx, near) - full["near"]).mean()),
                                    "l1_far": float(np.abs(picture(ctx, dst, g, keys, idx, far) - full["far"]).mean())}
            do[f"{n}:merge:m{m}"] = lambda labels=labels, dst=dst: ctx.merge_records(src, n, labels, dst=dst, count=count)
            if m == MEMBERS[0]:
                do[f"{n}:cell_labels"] = lambda grid=grid, labels=labels: ctx.cell_labels(src, n, grid, labels)

        def order_and_gather():
            ctx.spatial_order(src, n, order_index=order)
            ctx.gather_records(order, n, src, n, dst=gathered)
        do[f"{n}:spatial_order+gather_records"] = order_and_gather
        for call in do.values():
            call()
        out = turns(do, rounds, lambda call: window(ctx, call, calls))
        base = out[f"{n}:spatial_order+gather_records"]["ms"]
        for name in do:
            out[name]["over_order_and_gather"] = out[name]["ms"] / base
        res.update(out)
        # frames: the full set and every merged set, at the benchmark camera
        ctx.set_uniforms(time=0.0, min_opacity=0.0, view=gs4d.look_at(near[0], near[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
        # (key and index buffers in rotation, as the benchmark has them: frame f + 1 makes its keys while frame f is in flight)
        pairs = itertools.cycle([(keys, idx)] + [(ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)) for _ in range(3)])
        draws = {f"{n}:frame:full": lambda: frame(ctx, src, n, *next(pairs), near)}
        for m, (dst, g) in sets.items():
            draws[f"{n}:frame:m{m}"] = lambda dst=dst, g=g: frame(ctx, dst, g, *next(pairs), near)
        for call in draws.values():
            for _ in range(5):
                call()
        res.update(turns(draws, rounds, lambda call: window(ctx, call, frames)))
        ctx.close()
    return res


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    frames = int(sys.argv[4]) if len(sys.argv) > 4 else 60
    print(json.dumps({"tool": "merge_cost", "calls": calls, "rounds": rounds, "frames": frames, "records": measure(calls, rounds, largest, frames)}))


if __name__ == "__main__":
    main()

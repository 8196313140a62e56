"""What gs4d_lod_cut costs, and what the frames drawn from its cuts cost.

Forests: 10^6 and 10^7 leaves of the benchmark's cube set (scenes.cube_params: BASELINE.json configs[1] / configs[2]) under cell grids of about 8
members per group, each level's cells twice the edge of the level below, until one cell is left — what Context.build_lod does, with the level
buffers kept so that every fixed level can be drawn too.
Calls: the cut at the benchmark camera at ratios that draw about 100 %, 30 %, 10 % and 1 % of the leaf count (found by bisection on the device), dst
and cut_index given; beside it, in the same run, gs4d_count_centres (a box test) + gs4d_compact_records over the same N nodes: the yardstick — that
pair reads 32 bytes of every record and reads and writes a 16-byte row where a node under a parent that is not refined costs the cut about 6 bytes.
Device time of a call: it is asynchronous and its kernels run back to back with the next on one frame lane, so a window is `calls` calls between two
gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the entries of one n taking turns to lead a round.
Frames: the 1080p frame (clear, keygen, sort, draw at the benchmark camera) of the full set, of every fixed level and of every cut (from a buffer of
exactly `drawn` records), and the per-frame loop lod_cut -> keygen -> sort -> draw, in which the cut rewrites dst and the draw repacks it (four dst
buffers in rotation, one per frame in flight).
Prints one JSON line.  Usage: python tools/lod_cost.py [calls] [rounds] [largest n] [frames]."""
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
SHARES = (1.0, 0.3, 0.1, 0.01)                            # of the leaf count, drawn
MEMBERS = 8
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


def frame(ctx, data, n, keys, idx, cam):
    ctx.clear()
    ctx.keygen(data, 0.0, cam[0], keys, idx, n)
    ctx.sort_pairs(keys, idx, n)
    ctx.bind(1, idx)
    ctx.bind(2, data)
    ctx.draw_instanced(n)


def build(ctx, src, n):
    """(forest, [(buffer, records) of every level]): build_lod's steps with the level buffers kept"""
    cells = max(2, int(round((n / MEMBERS) ** (1.0 / 3.0))))
    levels, links = [(src, n)], []
    count = ctx.buffer(nbytes=16)
    while len(levels) < 16:
        prev, pn = levels[-1]
        labels = ctx.cell_labels(prev, pn, gs4d.cell_grid((-SIDE / 2,) * 3, SIDE / cells, (cells,) * 3))
        small = ctx.buffer(nbytes=16)
        ctx.merge_records(prev, pn, labels, dst=small, count=count)
        g = int(ctx.read_merge_count(count)["groups"])
        ctx.delete(small)
        dst, member_group = ctx.buffer(nbytes=96 * max(1, g)), ctx.buffer(nbytes=4 * pn)
        ctx.merge_records(prev, pn, labels, dst=dst, member_group=member_group, count=count)
        ctx.delete(labels)
        levels.append((dst, g))
        links.append(member_group)
        if cells == 1:
            break
        cells = max(1, cells // 2)
    first = [0]
    for _, m in levels:
        first.append(first[-1] + m)
    nodes, parent = ctx.buffer(nbytes=96 * first[-1]), ctx.buffer(nbytes=4 * first[-1])
    for k, (buf, m) in enumerate(levels):
        if k == 0:
            ctx.lod_append(buf, m, nodes, parent, 0)
        else:
            ctx.lod_append(buf, m, nodes, parent, first[k], member_group=links[k - 1], child_first=first[k - 1], c=levels[k - 1][1])
    ctx.finish()
    for b in links + [count]:
        ctx.delete(b)
    return gs4d.LodForest(nodes, parent, first), levels


def ratio_for(ctx, forest, eye, share, count):
    """the ratio whose cut draws about `share` of the leaf count: the drawn count falls as the ratio grows; 40 halvings of a bracket in log space"""
    if share >= 1.0:
        return 0.0
    lo, hi, want = 1e-6, 1e3, share * forest.level_first[1]
    for _ in range(40):
        mid = float(np.sqrt(lo * hi))
        ctx.lod_cut(forest, eye, 0.0, mid, count=count)
        if int(ctx.read_lod_count(count)["drawn"]) > want:
            lo = mid
        else:
            hi = mid
    return hi


def measure(calls, rounds, largest, frames):
    res = {}
    cam = scenes.CAM_CUBE
    for n in [s for s in SIZES if s <= largest]:
        pos, q, scale, rgba = scenes.cube_params(n)
        rec = gs4d.build_records_3d(pos, q, scale, rgba)
        del pos, q, scale, rgba
        ctx = gs4d.Context(W, H)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_mode(gs4d.MODE_4D_SORTED)
        ctx.set_uniforms(time=0.0, min_opacity=0.0, view=gs4d.look_at(cam[0], cam[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
        src = ctx.buffer(rec)
        del rec
        forest, levels = build(ctx, src, n)
        N = forest.n
        res[f"{n}:forest"] = {"nodes": N, "level_first": forest.level_first}
        count = ctx.buffer(nbytes=16)
        index = ctx.buffer(nbytes=4 * N)
        scratch_dst = ctx.buffer(nbytes=96 * n)              # every cut fits: it draws at most one node per leaf
        do, cuts = {}, {}
        for share in SHARES:
            ratio = ratio_for(ctx, forest, cam[0], share, count)
            ctx.lod_cut(forest, cam[0], 0.0, ratio, count=count)
            c = ctx.read_lod_count(count)
            drawn = int(c["drawn"])
            exact = ctx.buffer(nbytes=96 * max(1, drawn))
            ctx.lod_cut(forest, cam[0], 0.0, ratio, dst=exact, count=count)
            cuts[share] = (ratio, exact, drawn)
            res[f"{n}:cut:{share}"] = {"ratio": ratio, "drawn": drawn, "tested": int(c["tested"]), "drawn_leaves": int(c["drawn_leaves"])}
            do[f"{n}:lod_cut:{share}"] = lambda ratio=ratio: ctx.lod_cut(forest, cam[0], 0.0, ratio, dst=scratch_dst, cut_index=index, count=count)
        stats = ctx.buffer(np.zeros(N, gs4d.RECORD_STAT))
        ccount = ctx.buffer(nbytes=8)

        def centres_and_compact():
            ctx.count_centres(stats, N, forest.nodes, box=((-SIDE / 8,) * 3, (SIDE / 8,) * 3), t=0.0)
            ctx.compact_records(stats, N, src=forest.nodes, dst=scratch_dst, kept_index=index, count=ccount)
        do[f"{n}:count_centres+compact_records"] = centres_and_compact
        for call in do.values():
            call()
        out = turns(do, rounds, lambda call: window(ctx, call, calls))
        base = out[f"{n}:count_centres+compact_records"]["ms"]
        for name in do:
            out[name]["over_centres_and_compact"] = out[name]["ms"] / base
        res.update(out)
        res[f"{n}:count_centres+compact_records"]["kept"] = int(ctx.read_compact_count(ccount)[0])
        # frames (key and index buffers in rotation, as the benchmark has them: frame f + 1 makes its keys while frame f is in flight)
        pairs = itertools.cycle([(ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)) for _ in range(4)])
        draws = {f"{n}:frame:level{k}": (lambda buf=buf, m=m: frame(ctx, buf, m, *next(pairs), cam)) for k, (buf, m) in enumerate(levels) if m}
        for share, (ratio, exact, drawn) in cuts.items():
            if drawn:
                draws[f"{n}:frame:cut:{share}"] = lambda exact=exact, drawn=drawn: frame(ctx, exact, drawn, *next(pairs), cam)

                # (a dst and a count per frame in flight, like the key buffers: a cut into the buffer the previous frame still draws from would wait for it)
                ring = itertools.cycle([(exact, count)] + [(ctx.buffer(nbytes=96 * drawn), ctx.buffer(nbytes=16)) for _ in range(3)])

                def loop(ratio=ratio, drawn=drawn, ring=ring):
                    dst, cnt = next(ring)
                    ctx.lod_cut(forest, cam[0], 0.0, ratio, dst=dst, count=cnt)
                    frame(ctx, dst, drawn, *next(pairs), cam)
                draws[f"{n}:cut+frame:{share}"] = loop
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
    print(json.dumps({"tool": "lod_cost", "calls": calls, "rounds": rounds, "frames": frames, "records": measure(calls, rounds, largest, frames)}))


if __name__ == "__main__":
    main()

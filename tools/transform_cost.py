"""What gs4d_transform_records costs: 10^6 and 10^7 records under one transform, and 10^5 records under 10 (instances).

Device time of the call: it is asynchronous and its kernel runs back to back on one frame lane, so a window is `calls` calls between two gs4d_finish,
and the time of a call is the window over `calls`; medians of `rounds` windows, the shapes taking turns to lead a round.  The byte budget of a call is
m * n * 192 (96 read, 96 written; the 80 bytes of a transform are read once per workgroup and stay in cache) over the 6.3 TB/s copy ceiling DESIGN.md
uses.
Layout: which SoA layout the draw after a call settles on (gs4d_get_stats [3] bits 32-39: bytes per record the projection read) for a transformed
static 3D set and a transformed 4D set, against the same sets uploaded as they are.
Run it once per build of the library, each in a process of its own, to compare the shipped per-thread load with `make lib TRANSFORM_STAGED_LOAD=1`; `label` says which
one the line is for.  Prints one JSON line.  Usage: python tools/transform_cost.py [label] [calls] [rounds] [largest m * n]."""
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
SHAPES = ((1_000_000, 1), (10_000_000, 1), (100_000, 10))
RIGID = dict(q_wxyz=(0.9393727, 0.1496044, 0.2992088, -0.0748022), translate=(12.0, -7.5, 20.0))      # 0.7 rad about (1, 2, -0.5)


def window(ctx, call, calls):
    ctx.finish()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    ctx.finish()
    return (time.perf_counter() - t0) * 1e3 / calls


def sets(n):
    """(a static 3D set, a 4D set) of n records in front of scenes.CAM_CUBE"""
    pos, q, scale, rgba = scenes.cube_params(n)
    pos4, q4, sc4, life, fade, vel, rgba4 = scenes.cube_params_4d(n)
    return gs4d.build_records_3d(pos, q, scale, rgba), gs4d.build_records_4d(pos4, q4, sc4, life, fade, vel, rgba4)


def measure_calls(calls, rounds, largest):
    shapes = [s for s in SHAPES if s[0] * s[1] <= largest]
    ctx = gs4d.Context(64, 64)
    rec = sets(max(n for n, _ in shapes))[1]
    src = ctx.buffer(rec)
    dst = ctx.buffer(nbytes=96 * max(n * m for n, m in shapes))
    do = {}
    for n, m in shapes:
        xf = ctx.buffer(np.stack([gs4d.affine4(RIGID["q_wxyz"], translate=(float(j), 0.0, 0.0)) for j in range(m)]))
        do[f"{n}x{m}"] = lambda n=n, m=m, xf=xf: ctx.transform_records(src, n, xf, m, dst=dst)
    for call in do.values():
        call()
    names = list(do)
    ms = {name: [] for name in names}
    for r in range(rounds):
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            ms[name].append(window(ctx, do[name], calls))
    res = {}
    for (n, m), name in zip(shapes, names):
        v, budget = ms[name], n * m * 192 / COPY_CEILING * 1e3
        med = float(np.median(v))
        res[name] = {"ms": med, "spread_pct": 100.0 * (max(v) - min(v)) / med, "windows": v, "ms_byte_budget": budget, "fraction_of_ceiling": budget / med}
    ctx.close()
    return res


def layout_after(n=100_000):
    """bytes per record the projection of the next draw read: the sets as uploaded, and transformed by a rigid map on the device"""
    W, H = 640, 360
    cam = scenes.CAM_CUBE
    out = {}
    for name, rec, t in zip(("static_3d", "4d"), sets(n), (0.0, 25.0)):
        ctx = gs4d.Context(W, H)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_uniforms(time=t, min_opacity=0.0, view=gs4d.look_at(cam[0], cam[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
        keys, idx = ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
        src = ctx.buffer(rec)
        for what, data in (("uploaded", src), ("transformed", ctx.transform_records(src, n, gs4d.affine4(**RIGID)))):
            ctx.clear()
            ctx.keygen(data, t, cam[0], keys, idx, n)
            ctx.sort_pairs(keys, idx, n)
            ctx.set_mode(gs4d.MODE_4D_SORTED)
            ctx.bind(1, idx)
            ctx.bind(2, data)
            ctx.draw_instanced(n)
            ctx.finish()
            out[f"{name}_{what}"] = ctx.stats()["record_read_bytes"]
        ctx.close()
    return out


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "shipped"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    largest = int(sys.argv[4]) if len(sys.argv) > 4 else 10_000_000
    print(json.dumps({"tool": "transform_cost", "build": label, "calls": calls, "rounds": rounds, "records": measure_calls(calls, rounds, largest),
                      "record_read_bytes_of_the_next_draw": layout_after()}))


if __name__ == "__main__":
    main()

"""What record statistics (gs4d_set_record_stats) cost a frame: the C2 set (configs[1]: 10^6 static 3D splats) and configs[3]'s 10^6
4D splats at t = 25, 1080p, the reference's frame loop (clear -> keygen -> sort -> draw), statistics off and on.  Rotating windows of one
context each, medians.  Lanes accumulate concurrently; GS4D_LANES=1 gives the one-lane figures.  Prints one JSON line.  Usage: python tools/stats_cost.py [steps] [rounds]."""
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

W, H, N = 1920, 1080, 1_000_000
MODES = ("off", "on")


def frame(ctx, b, n, t):
    cam = scenes.CAM_CUBE
    ctx.clear()
    ctx.set_uniforms(time=t, min_opacity=0.0, view=gs4d.look_at(cam[0], cam[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
    ctx.keygen(b[0], t, cam[0], b[1], b[2], n)
    ctx.sort_pairs(b[1], b[2], n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, b[2])
    ctx.bind(2, b[0])
    ctx.draw_instanced(n)


def make(rec, mode):
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    n = rec.shape[0]
    b = (ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n))
    sb = None
    if mode == "on":
        sb = ctx.record_stats(n)
        ctx.set_record_stats(sb, n)
    return ctx, b, sb


def window(ctx, b, n, t, steps):
    ctx.finish()
    t0 = time.perf_counter()
    for _ in range(steps):
        frame(ctx, b, n, t)
    ctx.finish()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(rec, t, steps, rounds):
    n = rec.shape[0]
    ctxs = {m: make(rec, m) for m in MODES}
    for ctx, b, _ in ctxs.values():
        for _ in range(60):
            frame(ctx, b, n, t)
    ms = {m: [] for m in MODES}
    for r in range(rounds):
        for k in range(len(MODES)):
            m = MODES[(k + r) % len(MODES)]                          # each mode leads a round in turn
            ctx, b, _ = ctxs[m]
            ms[m].append(window(ctx, b, n, t, steps))
    ctx, _, sb = ctxs["on"]
    st = ctx.read_record_stats(sb, n)
    frames = 60 + steps * rounds
    for ctx, _, _ in ctxs.values():
        ctx.close()
    med = {m: float(np.median(ms[m])) for m in MODES}
    return {"ms_off": med["off"], "ms_on": med["on"], "on_over_off": med["on"] / med["off"], "spread_off_pct": 100.0 * (max(ms["off"]) - min(ms["off"])) / med["off"],
            "records_that_count": float((st["pixels"] > 0).mean()), "fragments_per_frame": float(st["pixels"].sum()) / frames, "windows": ms}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    pos, q, scale, rgba = scenes.cube_params(N)
    c2 = measure(gs4d.build_records_3d(pos, q, scale, rgba), 0.0, steps, rounds)
    del pos, q, scale, rgba
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(N)
    c4 = measure(gs4d.build_records_4d(pos4, q, scale, life, fade, vel, rgba), 25.0, steps, rounds)
    print(json.dumps({"tool": "stats_cost", "W": W, "H": H, "splats": N, "steps": steps, "rounds": rounds, "lanes_env": os.environ.get("GS4D_LANES"), "c2": c2, "c4_t25": c4}))


if __name__ == "__main__":
    main()

"""What gs4d_shade_sh costs: 10^6 and 10^7 96-byte records of the benchmark's cube set (bench.py, scenes.cube_params) with random
coefficients, degrees 0 .. 3, minimal rows.

Device time of the call: it is asynchronous and its kernels run back to back on one frame lane, so a window is `calls` calls between two
gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the degrees taking turns to lead a round — once on a
buffer without a shadow (records only) and once on a buffer whose shadow is current (records + the shadow's colour plane).  The byte budget of a
call is n * (12 (degree + 1)^2 rounded up to 16) + 64 n read and 32 n written, plus 32 n when the shadow is patched (whole 32-byte sectors), over
the 6.3 TB/s copy ceiling DESIGN.md uses.
Frame loop: the benchmark's 1080p frame (bench.Scene) at 10^6 records, frames in flight on every lane — clear, shade (degree 3), keygen, sort, draw
against the same loop without the shade call, the two taking turns in one context, `frames` frames per window, medians of `rounds`; and the same
loop with the colours written by the only route there was before: the restatement of tests/shade_cases.py on the host, then gs4d_buffer_subdata
(which makes the next draw repack).  shadow_builds of the shaded loop must stay 1.
Prints one JSON line.  Usage: python tools/shade_cost.py [calls] [rounds] [largest n] [frames] [host frames]."""
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
import bench  # noqa: E402
import scenes  # noqa: E402
import shade_cases  # noqa: E402

COPY_CEILING = 6.3e12                                     # bytes / s: DESIGN.md's HBM copy ceiling


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


def budget_ms(n, degree, patched):
    return (n * shade_cases.row_bytes(degree) + 64 * n + 32 * n + (32 * n if patched else 0)) / COPY_CEILING * 1e3


def records_of(n):
    pos, q, scale, rgba = scenes.cube_params(n)
    return gs4d.build_records_3d(pos, q, scale, rgba)


def random_coefficients(n, degree):
    return np.random.default_rng(0x5348 + degree).random((n, 3 * shade_cases.coeffs(degree)), dtype=np.float32) * np.float32(2.0) - np.float32(1.0)


def new_scene(rec):
    cam = scenes.CAM_CUBE
    return bench.Scene(gs4d, rec, cam, gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, bench.W, bench.H, scenes.ZNEAR, scenes.ZFAR), 0)


def measure_calls(n, calls, rounds):
    rec = records_of(n)
    cam = scenes.CAM_CUBE[0]
    sc = new_scene(rec)
    ctx = sc.ctx
    tables = {d: ctx.buffer(shade_cases.table(random_coefficients(n, d), shade_cases.row_bytes(d), pad_nan=False)) for d in range(4)}      # minimal rows
    plain = ctx.buffer(rec)                                                              # never drawn: no shadow
    out = {}
    sc.frame()                                                                           # sc.data has a current shadow from here on
    ctx.finish()
    for patched, data in ((False, plain), (True, sc.data)):
        do = {str(d): (lambda d=d: ctx.shade_sh(data, n, tables[d], d, 0.0, cam)) for d in range(4)}
        for call in do.values():
            call()
        res = turns(do, rounds, lambda call: window(ctx, call, calls))
        for d in range(4):
            b = budget_ms(n, d, patched)
            res[str(d)].update(ms_byte_budget=b, fraction_of_ceiling=b / res[str(d)]["ms"])
        out["shadow_patched" if patched else "records_only"] = res
    out["shadow_builds"] = ctx.shadow_builds(sc.data)
    sc.close()
    return out


def measure_frames(n, frames, rounds, host_frames):
    rec = records_of(n)
    cam = scenes.CAM_CUBE[0]
    sc = new_scene(rec)
    ctx = sc.ctx
    coeff = random_coefficients(n, 3)
    sh = ctx.buffer(coeff)

    def shaded_frame(t=0.0):
        keys, idx = sc.keybufs[sc.k % len(sc.keybufs)]
        sc.k += 1
        ctx.clear()
        ctx.set_uniforms(time=t)
        ctx.shade_sh(sc.data, n, sh, 3, t, cam)
        ctx.keygen(sc.data, t, cam, keys, idx, n)
        ctx.sort_pairs(keys, idx, n)
        ctx.bind(1, idx)
        ctx.draw_instanced(n)

    def host_frame(t=0.0):
        ctx.subdata(sc.data, shade_cases.shaded_records(rec, coeff, 3, t, cam))
        sc.frame(t)

    for f in (sc.frame, shaded_frame):                     # warm-up: the library learns the tile-list capacities
        window(ctx, f, frames)
    builds0 = ctx.shadow_builds(sc.data)
    res = turns({"frame": sc.frame, "frame_with_shade": shaded_frame}, rounds, lambda f: window(ctx, f, frames))
    builds = ctx.shadow_builds(sc.data)
    host = [window(ctx, host_frame, host_frames) for _ in range(3)]
    res["frame_with_host_colours"] = {"ms": float(np.median(host)), "windows": host, "frames_per_window": host_frames}
    res["shade_adds_ms"] = res["frame_with_shade"]["ms"] - res["frame"]["ms"]
    res["host_route_over_shade_route"] = res["frame_with_host_colours"]["ms"] / res["frame_with_shade"]["ms"]
    res["shadow_builds_before_the_loop"], res["shadow_builds_after_the_shaded_loop"] = builds0, builds
    res["shadow_builds_after_the_host_loop"] = ctx.shadow_builds(sc.data)
    st = ctx.stats()
    res["aborted_discarded"], res["reruns"] = st["aborted_discarded"], st["reruns"]
    assert builds0 == builds == 1, (builds0, builds)
    sc.close()
    return res


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    frames = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    host_frames = int(sys.argv[5]) if len(sys.argv) > 5 else 5
    res = {str(n): measure_calls(n, calls, rounds) for n in (1_000_000, 10_000_000) if n <= largest}
    loop = measure_frames(1_000_000, frames, rounds, host_frames)
    print(json.dumps({"tool": "shade_cost", "calls": calls, "rounds": rounds, "frames": frames, "records": res, "frame_loop_1e6": loop}))


if __name__ == "__main__":
    main()

"""What gs4d_build_records costs: 10^6 and 10^7 records of each form from the clean parameter sets of tests/build_cases.py.

Device time of the call: it is asynchronous and its kernel runs back to back on one frame lane, so a window is `calls` calls between two gs4d_finish,
and the time of a call is the window over `calls`; medians of `rounds` windows, the forms taking turns to lead a round.  The byte budget of a call is
n * (56 / 72 / 80 read for 3D / 4D_VEL / 4D_2Q + 96 written) over the 6.3 TB/s copy ceiling DESIGN.md uses.
Frame loop: the benchmark's 1080p frame (bench.Scene) at 10^6 records of the benchmark's cube set, frames in flight on every lane — clear, build (3D),
keygen, sort, draw against the same loop without the build, the two taking turns in one context, `frames` frames per window, medians of `rounds`.  A build
every frame also makes every draw repack the SoA shadow: a third loop that only declares the records changed (gs4d_buffer_invalidate, which without a
caller stream also blocks the host until the frames that read the buffer are done — an upper bound of the repack's share) takes turns with the two.  And
the same frames with the records built by the only route there was before: build_records_3d on the CPU, then gs4d_buffer_subdata.
Run it once per build of the library to compare the staged write with `make lib BUILD_PLAIN=1`; `label` says which one the line is for.
Prints one JSON line.  Usage: python tools/build_cost.py [label] [calls] [rounds] [largest n] [frames] [host frames]."""
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
import build_cases  # noqa: E402
import scenes  # noqa: E402

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


def budget_ms(n, form):
    return n * (build_cases.READ_BYTES[form] + 96) / COPY_CEILING * 1e3


def measure_calls(n, calls, rounds):
    ctx = gs4d.Context(64, 64)
    dst = ctx.buffer(nbytes=96 * n)
    do = {}
    for form in build_cases.FORMS:
        bufs = {k: ctx.buffer(a) for k, a in build_cases.clean(gs4d, form, n).items()}
        do[form] = lambda form=form, bufs=bufs: ctx.build_records(build_cases.form_id(gs4d, form), n, dst=dst, **bufs)
    for call in do.values():
        call()
    res = turns(do, rounds, lambda call: window(ctx, call, calls))
    for form in build_cases.FORMS:
        b = budget_ms(n, form)
        res[form].update(ms_byte_budget=b, fraction_of_ceiling=b / res[form]["ms"])
    ctx.close()
    return res


def measure_frames(n, frames, rounds, host_frames):
    pos, q, scale, rgba = scenes.cube_params(n)
    cam = scenes.CAM_CUBE
    sc = bench.Scene(gs4d, gs4d.build_records_3d(pos, q, scale, rgba), cam, gs4d.look_at(cam[0], cam[1]),
                     gs4d.perspective(scenes.FOV, bench.W, bench.H, scenes.ZNEAR, scenes.ZFAR), 0)
    ctx = sc.ctx
    bufs = {"pos": ctx.buffer(pos), "rot": ctx.buffer(q), "scale": ctx.buffer(scale), "rgba": ctx.buffer(rgba)}

    def rest_of_frame(t):
        keys, idx = sc.keybufs[sc.k % len(sc.keybufs)]
        sc.k += 1
        ctx.keygen(sc.data, t, cam[0], keys, idx, n)
        ctx.sort_pairs(keys, idx, n)
        ctx.bind(1, idx)
        ctx.draw_instanced(n)

    def built_frame(t=0.0):
        ctx.clear()
        ctx.set_uniforms(time=t)
        ctx.build_records(gs4d.PARAMS_3D, n, dst=sc.data, **bufs)
        rest_of_frame(t)

    def repacked_frame(t=0.0):
        ctx.clear()
        ctx.set_uniforms(time=t)
        ctx.invalidate(sc.data)
        rest_of_frame(t)

    def host_frame(t=0.0):
        ctx.subdata(sc.data, gs4d.build_records_3d(pos, q, scale, rgba))
        sc.frame(t)

    for f in (sc.frame, built_frame, repacked_frame):      # warm-up: the library learns the tile-list capacities
        window(ctx, f, frames)
    builds0 = ctx.shadow_builds(sc.data)
    res = turns({"frame": sc.frame, "frame_with_build": built_frame, "frame_with_repack_only": repacked_frame}, rounds, lambda f: window(ctx, f, frames))
    res["shadow_builds_per_frame_in_the_three_loops"] = (ctx.shadow_builds(sc.data) - builds0) / float(rounds * frames)
    host = [window(ctx, host_frame, host_frames) for _ in range(3)]
    res["frame_with_host_records"] = {"ms": float(np.median(host)), "windows": host, "frames_per_window": host_frames}
    res["build_adds_ms"] = res["frame_with_build"]["ms"] - res["frame"]["ms"]
    res["repack_adds_ms_upper_bound"] = res["frame_with_repack_only"]["ms"] - res["frame"]["ms"]
    res["host_route_over_build_route"] = res["frame_with_host_records"]["ms"] / res["frame_with_build"]["ms"]
    st = ctx.stats()
    res["aborted_discarded"], res["reruns"] = st["aborted_discarded"], st["reruns"]
    sc.close()
    return res


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "staged"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    largest = int(sys.argv[4]) if len(sys.argv) > 4 else 10_000_000
    frames = int(sys.argv[5]) if len(sys.argv) > 5 else 100
    host_frames = int(sys.argv[6]) if len(sys.argv) > 6 else 5
    res = {str(n): measure_calls(n, calls, rounds) for n in (1_000_000, 10_000_000) if n <= largest}
    loop = measure_frames(1_000_000, frames, rounds, host_frames) if frames > 0 else None
    print(json.dumps({"tool": "build_cost", "build": label, "calls": calls, "rounds": rounds, "frames": frames, "records": res, "frame_loop_1e6": loop}))


if __name__ == "__main__":
    main()

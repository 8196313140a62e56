"""What gs4d_spatial_order and gs4d_gather_records cost and what the order is worth: 10^6 and 10^7 96-byte records of the benchmark's
cube set (bench.py, scenes.cube_params), in the benchmark's random order.

Device time of the calls: they are asynchronous and their kernels run back to back on one frame lane, so a window is `calls` calls between two
gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the two calls taking turns to lead a round.  The
gather's byte budget is 4 m + 2 * stride * m (the index, the records read, the records written) over the 6.3 TB/s copy ceiling DESIGN.md uses.
Frame time: the benchmark's 1080p frame (bench.Scene) of the random-order set against the device-reordered set in ONE context, the two taking
turns, `frames` frames per window, medians of `rounds`; and the frames after which the one-off reorder (order + gather) has paid for itself.
The tool asserts that the reordered set is byte-identical to the upload bench.py --spatial-order makes (bench.morton_order on the host): the
frame time of the reordered set is that experiment's by construction.
Prints one JSON line.  Usage: python tools/reorder_cost.py [calls] [rounds] [largest n] [frames]."""
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

STRIDE = 96
COPY_CEILING = 6.3e12                                     # bytes / s: DESIGN.md's HBM copy ceiling


def window(ctx, call, calls):
    ctx.finish()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    ctx.finish()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(n, calls, rounds, frames):
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    cam = scenes.CAM_CUBE
    sc = bench.Scene(gs4d, rec, cam, gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, bench.W, bench.H, scenes.ZNEAR, scenes.ZFAR), 0)
    ctx = sc.ctx
    src = sc.data
    oi, dst = ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=STRIDE * n)
    do = {"spatial_order": lambda: ctx.spatial_order(src, n, stride=STRIDE, order_index=oi), "gather_records": lambda: ctx.gather_records(oi, n, src, n, stride=STRIDE, dst=dst)}
    for name in do:                                        # warm-up (the lane's scratch is allocated in the first call)
        for _ in range(3):
            do[name]()
    # the device's permutation and the device's reordered set against the host's (bench.py --spatial-order)
    host_order = bench.morton_order(pos)
    assert np.array_equal(ctx.read(oi, np.uint32, n), host_order.astype(np.uint32)), "order_index differs from bench.morton_order"
    assert np.array_equal(ctx.read(dst, np.uint32, n * (STRIDE // 4)), np.ascontiguousarray(rec[host_order]).view(np.uint32).reshape(-1)), "dst differs from the host-permuted upload"
    names = list(do)
    ms = {name: [] for name in names}
    for r in range(rounds):
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            ms[name].append(window(ctx, do[name], calls))
    out = {}
    for name in names:
        med = float(np.median(ms[name]))
        out[name] = {"ms_device_call": med, "spread_pct": 100.0 * (max(ms[name]) - min(ms[name])) / med, "windows": ms[name]}
    budget = (4 * n + 2 * STRIDE * n) / COPY_CEILING * 1e3
    out["gather_records"].update(ms_byte_budget=budget, fraction_of_ceiling=budget / out["gather_records"]["ms_device_call"])
    # the frame, the two sets taking turns in one context
    sets = {"random_order": src, "device_reordered": dst}

    def frames_of(data):
        sc.data = data
        ctx.bind(2, data)
        return window(ctx, sc.frame, frames)

    for data in sets.values():                             # warm-up: the library learns the tile-list capacities of each set
        frames_of(data)
    fms = {name: [] for name in sets}
    order = list(sets)
    for r in range(rounds):
        for k in range(len(order)):
            name = order[(k + r) % len(order)]
            fms[name].append(frames_of(sets[name]))
    frame = {name: {"ms_frame": float(np.median(v)), "spread_pct": 100.0 * (max(v) - min(v)) / float(np.median(v)), "windows": v} for name, v in fms.items()}
    gain = frame["random_order"]["ms_frame"] - frame["device_reordered"]["ms_frame"]
    one_off = out["spatial_order"]["ms_device_call"] + out["gather_records"]["ms_device_call"]
    out["frame"] = dict(frame, gain_ms=gain, gain_pct=100.0 * gain / frame["random_order"]["ms_frame"], ms_one_off_reorder=one_off,
                        frames_to_pay_back=(one_off / gain if gain > 0 else None), aborted_discarded=ctx.stats()["aborted_discarded"])
    sc.close()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    frames = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    res = {str(n): measure(n, calls, rounds, frames) for n in (1_000_000, 10_000_000) if n <= largest}
    print(json.dumps({"tool": "reorder_cost", "stride": STRIDE, "calls": calls, "rounds": rounds, "frames": frames, "records": res}))


if __name__ == "__main__":
    main()

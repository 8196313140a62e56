"""What gs4d_slice_records costs, and what a baked slice buys a paused frame.

Calls: 10^6 and 10^7 records of BASELINE.json configs[3]'s 4D set (scenes.cube_params_4d) sliced at t = 25, beside gs4d_transform_records with one
transform at the same n — the two move the same 192 bytes per record (96 read, 96 written), so they should be close.  Device time of a call: it is
asynchronous and its kernel runs back to back with the next on one frame lane, so a window is `calls` calls between two gs4d_finish, and the time of
a call is the window over `calls`; medians of `rounds` windows, the entries taking turns to lead a round.  The byte budget is 192 n over the 6.3 TB/s
copy ceiling DESIGN.md uses.
Frames: the benchmark's 1080p frame (bench.Scene: clear, keygen, sort, draw; frames in flight on every lane) of the 10^6 records of that set paused at
t in {0, 12.5, 25}, against the same loop over Context.freeze(t) of it — the slice without its dead records, drawn at the same time — `frames` frames
per window, medians of `rounds`, the two taking turns; with the bytes per record the projection read (gs4d_get_stats [3] bits 32-39) and the record
counts of both.
Prints one JSON line.  Usage: python tools/slice_cost.py [calls] [rounds] [largest n] [frames]."""
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

COPY_CEILING = 6.3e12                                     # bytes / s: DESIGN.md's HBM copy ceiling
SIZES = (1_000_000, 10_000_000)
PAUSED_AT = (0.0, 12.5, 25.0)
T_CALLS = 25.0


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


def records_of(n):
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)
    return gs4d.build_records_4d(pos4, q, scale, life, fade, vel, rgba)


def measure_calls(calls, rounds, largest):
    sizes = [n for n in SIZES if n <= largest]
    ctx = gs4d.Context(64, 64)
    src = ctx.buffer(records_of(max(sizes)))
    dst = ctx.buffer(nbytes=96 * max(sizes))
    xf = ctx.buffer(gs4d.affine4(translate=(1.0, 0.0, 0.0)).reshape(1, 20))
    do = {}
    for n in sizes:
        do[f"{n}:slice_records"] = lambda n=n: ctx.slice_records(src, n, T_CALLS, dst=dst)
        do[f"{n}:transform_records"] = lambda n=n: ctx.transform_records(src, n, xf, 1, dst=dst)
    for call in do.values():
        call()
    res = turns(do, rounds, lambda call: window(ctx, call, calls))
    for name in do:
        b = int(name.split(":")[0]) * 192 / COPY_CEILING * 1e3
        res[name].update(ms_byte_budget=b, fraction_of_ceiling=b / res[name]["ms"])
    for n in sizes:
        res[f"{n}:slice_over_transform"] = res[f"{n}:slice_records"]["ms"] / res[f"{n}:transform_records"]["ms"]
    ctx.close()
    return res


def measure_frames(n, frames, rounds):
    rec = records_of(n)
    cam = scenes.CAM_CUBE
    view, proj = gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, bench.W, bench.H, scenes.ZNEAR, scenes.ZFAR)
    out = {}
    for t in PAUSED_AT:
        paused = bench.Scene(gs4d, rec, cam, view, proj, 0)
        dst, kept_index, count = paused.ctx.freeze(paused.data, n, t)
        kept, _ = paused.ctx.read_compact_count(count)
        frozen_rec = paused.ctx.read(dst, np.float32, kept * 24).reshape(kept, 24)
        frozen = bench.Scene(gs4d, frozen_rec, cam, view, proj, 0)
        do = {"paused_4d": (paused, lambda: paused.frame(t)), "frozen": (frozen, lambda: frozen.frame(t))}
        for sc, f in do.values():                          # warm-up: the library learns the tile-list capacities
            window(sc.ctx, f, frames)
        res = turns(do, rounds, lambda e: window(e[0].ctx, e[1], frames))
        res["paused_4d"].update(records=n, record_read_bytes=paused.ctx.stats()["record_read_bytes"])
        res["frozen"].update(records=kept, record_read_bytes=frozen.ctx.stats()["record_read_bytes"])
        res["frozen_over_paused"] = res["frozen"]["ms"] / res["paused_4d"]["ms"]
        out[str(t)] = res
        paused.close()
        frozen.close()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    frames = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    print(json.dumps({"tool": "slice_cost", "calls": calls, "rounds": rounds, "records": measure_calls(calls, rounds, largest),
                      "paused_frames": measure_frames(1_000_000, frames, rounds), "frames_per_window": frames}))


if __name__ == "__main__":
    main()

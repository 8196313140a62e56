"""What gs4d_edit_colours costs: 10^6 and 10^7 96-byte records of the benchmark's cube set (bench.py, scenes.cube_params), an rgba
LERP by a table that selects 0 %, 1 %, 50 % and 100 % of them (a seeded random mask: the selected records are scattered).

Device time of the call: it is asynchronous and its kernel runs back to back with the next on one frame lane, so a window is `calls` calls between
two gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the fractions taking turns to lead a round — once on
a buffer without a shadow (records only: the colour is read from the records) and once on a buffer whose shadow is current (the colour is read from
the shadow's plane 1, and written to the records and to the plane).  The byte budget of a call is 16 n for the table and, per selected record, 16
read + 16 written, + 16 written when the shadow is patched, over the 6.3 TB/s copy ceiling DESIGN.md uses (useful bytes: the 16-byte store into a
96-byte record touches part of a line whatever is done).
Frame loop: the benchmark's 1080p frame (bench.Scene) at 10^6 records — clear, keygen, sort, draw — against the same loop with an edit of 50 % of
the records in front of every frame's keygen and in front of every 8th frame's, taking turns in one context, `frames` frames per window, medians of
`rounds`; once with the library's frame lanes (frames in flight on every lane: an edit waits on the device for the frames that still read the
records, so an edit in EVERY frame gives up the overlap of consecutive frames) and once with one lane (no overlap to give up: what is left is the
kernel and whatever the edit makes the next draw do).  And the same effect by the only route there was before: the restatement of
tests/edit_cases.py on the host, then gs4d_buffer_subdata (which makes the next draw repack), with and without the host's arithmetic.
shadow_builds of the edited loops must stay 1.
Prints one JSON line.  Usage: python tools/edit_cost.py [calls] [rounds] [largest n] [frames] [host frames]."""
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
import edit_cases  # noqa: E402
import scenes  # noqa: E402

COPY_CEILING = 6.3e12                                     # bytes / s: DESIGN.md's HBM copy ceiling
FRACTIONS = (0.0, 0.01, 0.5, 1.0)
TINT = dict(op="lerp", value=(1.0, 0.1, 0.9, 0.35), channels=15, amount=0.75)


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


def budget_ms(n, selected, patched):
    return (16 * n + selected * (32 + (16 if patched else 0))) / COPY_CEILING * 1e3


def records_of(n):
    pos, q, scale, rgba = scenes.cube_params(n)
    return gs4d.build_records_3d(pos, q, scale, rgba)


def table_of(n, fraction):
    """a record_stats table whose rows pass {pixels >= 1} for a seeded random `fraction` of the records"""
    mask = np.random.default_rng(0x4544).random(n) < fraction if 0.0 < fraction < 1.0 else np.full(n, fraction >= 1.0)
    st = np.zeros(n, gs4d.RECORD_STAT)
    st["pixels"] = mask
    return st, mask


def new_scene(rec, lanes=None):
    cam = scenes.CAM_CUBE
    return bench.Scene(gs4d, rec, cam, gs4d.look_at(cam[0], cam[1]), gs4d.perspective(scenes.FOV, bench.W, bench.H, scenes.ZNEAR, scenes.ZFAR), 0, lanes=lanes)


def edit(ctx, data, n, stats):
    ctx.edit_colours(data, n, TINT["op"], TINT["value"], TINT["channels"], TINT["amount"], stats=stats, min_pixels=1)


def measure_calls(n, calls, rounds):
    rec = records_of(n)
    sc = new_scene(rec)
    ctx = sc.ctx
    tables, selected = {}, {}
    for f in FRACTIONS:
        st, mask = table_of(n, f)
        tables[f], selected[f] = ctx.buffer(st), int(mask.sum())
    plain = ctx.buffer(rec)                                                              # never drawn: no shadow
    out = {}
    sc.frame()                                                                           # sc.data has a current shadow from here on
    ctx.finish()
    for patched, data in ((False, plain), (True, sc.data)):
        do = {str(f): (lambda f=f: edit(ctx, data, n, tables[f])) for f in FRACTIONS}
        for call in do.values():
            call()
        res = turns(do, rounds, lambda call: window(ctx, call, calls))
        for f in FRACTIONS:
            b = budget_ms(n, selected[f], patched)
            res[str(f)].update(selected=selected[f], ms_byte_budget=b, fraction_of_ceiling=b / res[str(f)]["ms"])
        out["shadow_patched" if patched else "records_only"] = res
    out["shadow_builds"] = ctx.shadow_builds(sc.data)
    assert out["shadow_builds"] == 1, out["shadow_builds"]
    sc.close()
    return out


def measure_frames(n, frames, rounds, host_frames, lanes=None):
    rec = records_of(n)
    cam = scenes.CAM_CUBE[0]
    sc = new_scene(rec, lanes)
    ctx = sc.ctx
    st, _ = table_of(n, 0.5)
    stats = ctx.buffer(st)
    table = np.ascontiguousarray(st).view(edit_cases.STAT)

    def edited_frame(every):
        def frame(t=0.0):
            keys, idx = sc.keybufs[sc.k % len(sc.keybufs)]
            sc.k += 1
            ctx.clear()
            ctx.set_uniforms(time=t)
            if sc.k % every == 0:
                edit(ctx, sc.data, n, stats)
            ctx.keygen(sc.data, t, cam, keys, idx, n)
            ctx.sort_pairs(keys, idx, n)
            ctx.bind(1, idx)
            ctx.draw_instanced(n)
        return frame

    do = {"frame": sc.frame, "edit_every_frame": edited_frame(1), "edit_every_8th_frame": edited_frame(8)}
    for f in do.values():                                  # warm-up: the library learns the tile-list capacities
        window(ctx, f, frames)
    builds0 = ctx.shadow_builds(sc.data)
    res = turns(do, rounds, lambda f: window(ctx, f, frames))
    builds = ctx.shadow_builds(sc.data)
    for name in ("edit_every_frame", "edit_every_8th_frame"):
        res[name]["adds_ms_per_frame"] = res[name]["ms"] - res["frame"]["ms"]
        res[name]["adds_pct"] = 100.0 * res[name]["adds_ms_per_frame"] / res["frame"]["ms"]
    res["lanes"] = ctx.stats()["lanes"]
    res["shadow_builds_before_the_loop"], res["shadow_builds_after_the_edited_loops"] = builds0, builds
    assert builds0 == builds == 1, (builds0, builds)
    if host_frames:
        host_rec = [rec]

        def host_frame(t=0.0):
            host_rec[0] = edit_cases.edit(host_rec[0], TINT["op"], TINT["channels"], TINT["value"], TINT["amount"], stats=table)
            ctx.subdata(sc.data, host_rec[0])
            sc.frame(t)

        def upload_frame(t=0.0):
            ctx.subdata(sc.data, rec)                      # the upload and the repack alone, without the host's arithmetic
            sc.frame(t)

        host = [window(ctx, host_frame, host_frames) for _ in range(3)]
        upload = [window(ctx, upload_frame, host_frames) for _ in range(3)]
        res["frame_with_host_edit"] = {"ms": float(np.median(host)), "windows": host, "frames_per_window": host_frames}
        res["frame_with_upload_only"] = {"ms": float(np.median(upload)), "windows": upload, "frames_per_window": host_frames}
        res["upload_route_over_edit_every_frame"] = res["frame_with_upload_only"]["ms"] / res["edit_every_frame"]["ms"]
        res["shadow_builds_after_the_host_loops"] = ctx.shadow_builds(sc.data)
    s = ctx.stats()
    res["aborted_discarded"], res["reruns"] = s["aborted_discarded"], s["reruns"]
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
    one_lane = measure_frames(1_000_000, frames, rounds, 0, lanes=1)
    print(json.dumps({"tool": "edit_cost", "calls": calls, "rounds": rounds, "frames": frames, "records": res, "frame_loop_1e6": loop,
                      "frame_loop_1e6_one_lane": one_lane}))


if __name__ == "__main__":
    main()

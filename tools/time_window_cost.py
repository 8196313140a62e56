"""What the time windows cost and what they save: gs4d_record_time_spans and gs4d_compact_time_window on the 10^6 4D splats of
BASELINE.json configs[3], and the 1080p frame at t = 25 — key generation, depth sort, draw — of the full set against the set compacted to the
one-frame window [25, 25].

Device time as tools/compact_cost.py takes it: the calls are asynchronous, so a window is `calls` calls (or frames) between two gs4d_finish and
the figure is the window over `calls`; medians of `rounds` windows, the full and the compacted frames taking turns.  Prints one JSON line.
Usage: python tools/time_window_cost.py [calls] [rounds] [n]."""
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

W, H, T = 1920, 1080, 25.0
WINDOWS = ((25.0, 25.0), (24.0, 26.0), (20.0, 30.0))


def window(ctx, call, calls):
    ctx.finish()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    ctx.finish()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)
    rec = gs4d.build_records_4d(pos4, q, scale, life, fade, vel, rgba)
    cam = scenes.CAM_CUBE
    view, proj = gs4d.look_at(*cam), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.set_uniforms(time=T, min_opacity=0.0, view=view, proj=proj)
    data = ctx.buffer(rec)
    spans = ctx.record_time_spans(data, n)
    dst, idx, count = ctx.buffer(nbytes=n * 96), ctx.buffer(nbytes=n * 4), ctx.buffer(nbytes=8)
    out = {"n": n, "calls": calls, "rounds": rounds, "lanes": ctx.stats()["lanes"]}
    out["record_time_spans_ms"] = float(np.median([window(ctx, lambda: ctx.record_time_spans(data, n, 0.0, spans), calls) for _ in range(rounds)]))
    for w in WINDOWS:
        call = lambda: ctx.compact_time_window(spans, n, *w, src=data, dst=dst, kept_index=idx, count=count)
        ms = float(np.median([window(ctx, call, calls) for _ in range(rounds)]))
        kept, _ = ctx.read_compact_count(count)
        out[f"compact_time_window_{w[0]:g}_{w[1]:g}"] = {"ms": ms, "kept": kept, "kept_share": kept / n}
    # the frame at t = 25: the full set against the set of the one-frame window
    cdata, kidx, kept = ctx.time_window(data, n, T, T, spans=spans)
    keybufs = [(ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)) for _ in range(4)]
    state = {"k": 0}

    def frame(buf, count_):
        keys, index = keybufs[state["k"] % 4]
        state["k"] += 1
        ctx.clear()
        ctx.keygen(buf, T, cam[0], keys, index, count_)
        ctx.sort_pairs(keys, index, count_)
        ctx.set_mode(gs4d.MODE_4D_SORTED)
        ctx.bind(1, index)
        ctx.bind(2, buf)
        ctx.draw_instanced(count_)

    sets = {"full": (data, n), "compacted": (cdata, kept)}
    images, ms = {}, {k: [] for k in sets}
    for name, (buf, m) in sets.items():
        for _ in range(24):
            frame(buf, m)
        images[name] = ctx.read_pixels()
    for r in range(rounds):
        for name in (list(sets) if r % 2 == 0 else list(sets)[::-1]):
            buf, m = sets[name]
            for _ in range(8):                               # the staged lists settle on this set again
                frame(buf, m)
            ms[name].append(window(ctx, lambda: frame(buf, m), calls))
    out["frame_t25"] = {"kept": kept, "kept_share": kept / n, "full_ms": float(np.median(ms["full"])), "compacted_ms": float(np.median(ms["compacted"])),
                        "images_bit_equal": bool(np.array_equal(images["full"].view(np.uint32), images["compacted"].view(np.uint32)))}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What gs4d_count_centres costs: 10^6 and 10^7 96-byte records of the benchmark's cube set (bench.py, scenes.cube_params: static 3D
splats, the 64-byte shadow layout) and of its 4D variant (scenes.cube_params_4d: a symmetric sig, the 72-byte layout), a box-only query and a
screen + mask query that select about 0 %, 50 % and 100 % of them (the table says how many: `selected`).

Device time of the call: it is asynchronous and its kernel runs back to back with the next on one frame lane, so a window is `calls` calls between
two gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the cases taking turns to lead a round.  Such a
window is CACHE-WARM: the same buffers are read call after call, and 10^6 records (96 MB), or at 10^7 a 160 MB plane or table, fit the 256 MB
last-level cache.  So every case is also timed COLD (`cold_ms`): one call between two gs4d_finish, after a device copy of 2 x 384 MB of other
memory (gs4d_transform_records of a scratch set) has gone through the cache; median of `cold repeats` such calls.  That host clock also holds what
issuing one call and waiting for it costs, which `cold_floor_ms` (the same call on 256 records) reports.  Both are measured once on a
buffer without a shadow (the kernel reads the 16-byte pieces 0 and 5 of every 96-byte record) and once on a buffer whose shadow is current (it reads
plane 0 and the sig[3] plane; plane 0 alone for static 3D splats).  The useful bytes of a call are those fields (32 n, 16 n for the static layout)
and, per selected record, a 16-byte row read and written, over the 6.3 TB/s copy ceiling DESIGN.md uses; from the records the two pieces of a record
lie in different 64-byte halves of its 96 bytes, so the hardware moves most of the 96 n bytes whatever is done.
And the route the call replaces, on the same machine: gs4d_buffer_read of the records, count_centres_host, gs4d_buffer_subdata of the table.
shadow_builds must not move.
Prints one JSON line.  Usage: python tools/centres_cost.py [calls] [rounds] [largest n] [host repeats] [cold repeats]."""
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
CAM = ((0.0, 0.0, 600.0), (0.0, 0.0, -1.0))               # the whole cube ([-200, 200]^3) is on the 1080p screen
FAR = 1e9
FLUSH_RECORDS = 4_000_000                                 # 384 MB read and 384 MB written: more than the 256 MB last-level cache, twice


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


def records_of(kind, n):
    if kind == "static3d":
        pos, q, scale, rgba = scenes.cube_params(n)
        return gs4d.build_records_3d(pos, q, scale, rgba)
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)
    rec = gs4d.build_records_4d(pos4, q, scale, life, fade, vel, rgba)
    sig = rec[:, 8:].reshape(-1, 4, 4)
    iu = np.triu_indices(4, 1)
    sig[:, iu[0], iu[1]] = sig[:, iu[1], iu[0]]           # bit-symmetric: the 72-byte layout
    return rec


def queries(view, proj):
    """name -> (CentreQuery, mask array or None): a box that holds nothing, half the cube, all of it; the whole screen under a lasso of zeros, a
    one-pixel checkerboard, ones"""
    out = {}
    for name, (lo, hi) in (("box_0", ((FAR, FAR, FAR), (2 * FAR, 2 * FAR, 2 * FAR))), ("box_50", ((-FAR, -FAR, -FAR), (0.0, FAR, FAR))),
                           ("box_100", ((-FAR, -FAR, -FAR), (FAR, FAR, FAR)))):
        out[name] = (gs4d.centre_query(box=(lo, hi), t=25.0), None)
    r, c = np.mgrid[0:bench.H, 0:bench.W]
    for name, m in (("screen_mask_0", np.zeros((bench.H, bench.W), np.uint8)), ("screen_mask_50", ((r + c) & 1).astype(np.uint8)),
                    ("screen_mask_100", np.ones((bench.H, bench.W), np.uint8))):
        out[name] = (gs4d.centre_query(screen=(view, proj), rect=(0, 0, bench.W, bench.H), t=25.0), m)
    return out


def cold(ctx, flush, call, repeats):
    """ms of one call between two gs4d_finish with the cache flushed in front of it: (median, runs)"""
    runs = []
    for _ in range(repeats):
        flush()
        ctx.finish()
        t0 = time.perf_counter()
        call()
        ctx.finish()
        runs.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(runs)), runs


def measure(kind, n, calls, rounds, host_repeats, cold_repeats):
    print(f"centres_cost: {kind}, {n} records", file=sys.stderr, flush=True)
    rec = records_of(kind, n)
    view, proj = gs4d.look_at(*CAM), gs4d.perspective(scenes.FOV, bench.W, bench.H, scenes.ZNEAR, scenes.ZFAR)
    sc = bench.Scene(gs4d, rec, CAM, view, proj, 0)
    ctx = sc.ctx
    qs = queries(view, proj)
    masks = {name: ctx.buffer(m) for name, (_, m) in qs.items() if m is not None}
    plain = ctx.buffer(rec)                                                              # never drawn: no shadow
    stats = ctx.record_stats(n)
    scratch, scratch_out = ctx.buffer(nbytes=96 * FLUSH_RECORDS), ctx.buffer(nbytes=96 * FLUSH_RECORDS)
    identity = ctx.buffer(gs4d.affine4())

    def flush():
        ctx.transform_records(scratch, FLUSH_RECORDS, identity, 1, scratch_out)

    sc.frame(25.0)                                                                       # sc.data has a current shadow from here on
    ctx.finish()
    layout = ctx.stats()["record_read_bytes"]
    field_bytes = {64: 16, 72: 32, 96: 32}[layout]
    out = {"shadow_layout_bytes": layout}
    selected = {}
    for shadow, data in ((False, plain), (True, sc.data)):
        do = {name: (lambda name=name: ctx.count_centres(stats, n, data, mask=masks.get(name), query=qs[name][0])) for name in qs}
        for name, call in do.items():                                                    # warm-up, and how many each query selects
            ctx.subdata(stats, np.zeros(n, gs4d.RECORD_STAT))
            call()
            got = int((ctx.read_record_stats(stats, n)["pixels"] == 1).sum())
            assert selected.setdefault(name, got) == got, "the shadow and the records select different sets"
        res = turns(do, rounds, lambda call: window(ctx, call, calls))
        for name in qs:
            useful = (field_bytes if shadow else 32) * n + 32 * selected[name]
            b = useful / COPY_CEILING * 1e3
            res[name].update(selected=selected[name], selected_pct=100.0 * selected[name] / n, ms_useful_bytes=b, fraction_of_ceiling=b / res[name]["ms"])
            if cold_repeats:
                res[name]["cold_ms"], res[name]["cold_runs"] = cold(ctx, flush, do[name], cold_repeats)
        if cold_repeats:
            res["cold_floor_ms"], _ = cold(ctx, flush, lambda: ctx.count_centres(stats, 256, data, query=qs["box_100"][0]), cold_repeats)
        out["shadow_current" if shadow else "records_only"] = res
    out["shadow_over_records"] = {name: out["shadow_current"][name]["ms"] / out["records_only"][name]["ms"] for name in qs}
    if cold_repeats:
        out["cold_shadow_over_records"] = {name: out["shadow_current"][name]["cold_ms"] / out["records_only"][name]["cold_ms"] for name in qs}
    out["shadow_builds"] = [ctx.shadow_builds(plain), ctx.shadow_builds(sc.data)]
    assert out["shadow_builds"] == [0, 1], out["shadow_builds"]
    if host_repeats:
        q, m = qs["screen_mask_50"]
        parts = {"buffer_read": [], "count_centres_host": [], "buffer_subdata": [], "total": []}
        for _ in range(host_repeats):
            ctx.finish()
            t0 = time.perf_counter()
            back = ctx.read(plain, np.float32, n * 24)
            t1 = time.perf_counter()
            table = gs4d.count_centres_host(back, q, bench.W, bench.H, mask=m)
            t2 = time.perf_counter()
            ctx.subdata(stats, table)
            ctx.finish()
            t3 = time.perf_counter()
            for key, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                parts[key].append(v * 1e3)
        assert int((table["pixels"] == 1).sum()) == selected["screen_mask_50"]
        out["host_route_screen_mask_50"] = {key: {"ms": float(np.median(v)), "runs": v} for key, v in parts.items()}
        out["host_route_over_call"] = out["host_route_screen_mask_50"]["total"]["ms"] / out["records_only"]["screen_mask_50"]["ms"]
    sc.close()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    host_repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    cold_repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 9
    res = {kind: {str(n): measure(kind, n, calls, rounds, host_repeats, cold_repeats) for n in (1_000_000, 10_000_000) if n <= largest} for kind in ("static3d", "symmetric4d")}
    print(json.dumps({"tool": "centres_cost", "calls": calls, "rounds": rounds, "cold_repeats": cold_repeats, "records": res}))


if __name__ == "__main__":
    main()

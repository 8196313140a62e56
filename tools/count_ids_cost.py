"""What gs4d_count_ids costs on a full 1920 x 1080 image: (a) a frame one splat covers — every lane of every wave shows the same
record, the worst case for the table's atomics — and (b) a frame of 46 046 small splats, where neighbouring lanes differ.

Prints, per frame, a hash of the table one call leaves (the same for every build of the kernel) and the time of a call from windows of `calls`
calls between two gs4d_finish (the launch gaps are inside that figure; `rocprofv3 --kernel-trace --stats -- python tools/count_ids_cost.py`
gives k_count_ids alone).  Run it on the shipped build and on one without the in-wave aggregation (`make lib COUNT_IDS_PLAIN=1`; a plain `make lib` afterwards
rebuilds the shipped kernel) to see what the aggregation buys.  Usage: python tools/count_ids_cost.py [calls] [directory that holds the package to load]."""
import ctypes
import hashlib
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
sys.path.insert(0, sys.argv[2] if len(sys.argv) > 2 else ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
import stats_cases as sc
print("library:", gs4d.LIB_PATH, flush=True)
W, H = 1920, 1080
scenes = {
    "one_splat": sc.records(gs4d, W, H, [W / 2.0], [H / 2.0], [0.0], [4000.0], [[0.9, 0.4, 0.1, 0.9]]),
    "small_splats": sc.records(gs4d, W, H, *sc.disjoint("small", W, H)),
}
for name, rec in scenes.items():
    n = rec.shape[0]
    ctx = gs4d.Context(W, H)
    ctx.set_id_outputs(True)
    db = ctx.buffer(rec)
    view, proj = sc.mats(gs4d, W, H)
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
    ctx.set_mode(gs4d.MODE_4D_DIRECT)
    ctx.bind(1, db)
    ctx.clear()
    ctx.draw_instanced(n)
    ctx.finish()
    rid = ctx.read_ids()[0]
    shown = rid != 0xFFFFFFFF
    t = ctx.record_stats(n)
    ctx.count_ids(t, n)
    tab = ctx.read(t, np.uint8, 16 * n)
    print(f"{name}: {n} records, {int(shown.sum())} pixels shown, {np.unique(rid[shown]).size} records shown, table sha1 {hashlib.sha1(tab.tobytes()).hexdigest()[:16]}", flush=True)
    g = gs4d.IdRegion(0, 0, W, H, 0, 0xFFFFFFFF, 0, 0)
    call = lambda: gs4d._lib.gs4d_count_ids(ctx._h, ctypes.byref(g), 0, t, ctypes.c_size_t(n))
    for _ in range(5):
        assert call() == 0
    ctx.finish()
    for rnd in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        ctx.finish()
        dt = time.perf_counter() - t0
        print(f"{name}: round {rnd}: {reps} calls back to back, {1e6 * dt / reps:.1f} us per call (host clock, ends in a finish)", flush=True)
    ctx.close()

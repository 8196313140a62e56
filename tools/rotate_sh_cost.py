"""What gs4d_rotate_sh costs beside gs4d_copy_rows and gs4d_shade_sh.

Calls: 10^6 and 10^7 rows at degrees 0..3, every degree at its minimal stride (16 / 48 / 112 / 192 bytes), rotated
  each_m1           GS4D_SH_EACH with one map;
  index_m16, index_m64, index_m1024   GS4D_POSE_INDEX with 16, 64 and 1024 maps;
  blend4_m64        GS4D_POSE_BLEND4, four slots of normalised weights over 64 maps;
  blend4_one_m16    the bind rows of index_m16 as GS4D_POSE_BLEND4 rows with one slot of weight 1: the same bits as index_m16 through the blend — what
                    a build with the matrices of a small table in LDS was compared against;
beside gs4d_copy_rows of the same rows (it moves the same 2 * stride bytes per row: the floor the call should approach) and gs4d_shade_sh at the
same degree over the same table (what the frame pays anyway).  The bind rows are coherent: runs of 4096 rows name the same maps, as the splats of a
joint or an object lie together.  Device time of a call: it is asynchronous and its kernel runs back to back with the next on one frame lane, so a
window is `calls` calls between two gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the entries of one
(n, degree) taking turns to lead a round.
Prints one JSON line.  Usage: python tools/rotate_sh_cost.py [calls] [rounds] [largest n]."""
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
SIZES = (1_000_000, 10_000_000)
DEGREES = (0, 1, 2, 3)
RUN = 4096                                                # rows in a row that are bound alike
BIND_BYTES = {"each_m1": 0, "index_m16": 4, "index_m64": 4, "index_m1024": 4, "blend4_m64": 32, "blend4_one_m16": 32, "copy_rows": 0}


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


def table_of(m, rng):
    """m similarities: unit quaternions, scales around 1 and shifts of a few units"""
    q = rng.standard_normal((m, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.stack([gs4d.affine4(q[k], float(rng.uniform(0.5, 2.0)), rng.uniform(-5.0, 5.0, 3)) for k in range(m)])


def joints_of(n, m, k, rng):
    runs = rng.integers(m, size=((n + RUN - 1) // RUN, k)).astype(np.uint32)
    return np.repeat(runs, RUN, axis=0)[:n]


def measure_calls(calls, rounds, largest):
    sizes = [n for n in SIZES if n <= largest]
    rng = np.random.default_rng(0x5348524F)
    ctx = gs4d.Context(64, 64)
    nmax = max(sizes)
    records = ctx.buffer(records_of(nmax))
    coeff = (rng.random((nmax, 48), dtype=np.float32) - np.float32(0.5))
    tables = {m: ctx.buffer(table_of(m, rng)) for m in (1, 16, 64, 1024)}
    j16, j64, j1024 = joints_of(nmax, 16, 1, rng), joints_of(nmax, 64, 4, rng), joints_of(nmax, 1024, 1, rng)
    w = rng.uniform(0.05, 1.0, (nmax, 4)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    binds = {"index_m16": ctx.buffer(np.ascontiguousarray(j16[:, 0])), "index_m64": ctx.buffer(np.ascontiguousarray(j64[:, 0])),
             "index_m1024": ctx.buffer(np.ascontiguousarray(j1024[:, 0])), "blend4_m64": ctx.buffer(gs4d.bind_rows(j64, w)),
             "blend4_one_m16": ctx.buffer(gs4d.bind_rows(j16, np.ones((nmax, 1), np.float32)))}
    del w, j1024
    res = {}
    for degree in DEGREES:
        stride = gs4d.sh_row_bytes(degree)
        src = ctx.buffer(np.ascontiguousarray(coeff[:, :stride // 4]))
        dst = ctx.buffer(nbytes=stride * nmax)
        for n in sizes:
            def rotate(m=1, bind=None, form=None, n=n):
                return lambda: ctx.rotate_sh(src, n, tables[m], degree, m=m, bind=bind, form=form, stride=stride, dst=dst)
            do = {"copy_rows": lambda n=n: ctx.copy_rows(src, n, stride, dst=dst),
                  "shade_sh": lambda n=n: ctx.shade_sh(records, n, src, degree, 25.0, (31.0, -12.5, 140.0), sh_stride=stride),
                  "each_m1": rotate(),
                  "index_m16": rotate(16, binds["index_m16"], gs4d.POSE_INDEX),
                  "index_m64": rotate(64, binds["index_m64"], gs4d.POSE_INDEX),
                  "index_m1024": rotate(1024, binds["index_m1024"], gs4d.POSE_INDEX),
                  "blend4_m64": rotate(64, binds["blend4_m64"], gs4d.POSE_BLEND4),
                  "blend4_one_m16": rotate(16, binds["blend4_one_m16"], gs4d.POSE_BLEND4)}
            for call in do.values():
                call()
            out = turns(do, rounds, lambda call: window(ctx, call, calls))
            floor = out["copy_rows"]["ms"]
            for name in do:
                if name in BIND_BYTES:
                    b = n * (2 * stride + BIND_BYTES[name]) / COPY_CEILING * 1e3
                    out[name].update(ms_byte_budget=b, fraction_of_ceiling=b / out[name]["ms"])
                out[name].update(over_copy_rows=out[name]["ms"] / floor, over_shade_sh=out[name]["ms"] / out["shade_sh"]["ms"])
            out["index_over_one_slot_blend4"] = out["index_m16"]["ms"] / out["blend4_one_m16"]["ms"]
            res[f"{n}:degree{degree}"] = out
        ctx.delete(src)
        ctx.delete(dst)
    ctx.close()
    return res


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    print(json.dumps({"tool": "rotate_sh_cost", "calls": calls, "rounds": rounds, "rows": measure_calls(calls, rounds, largest)}))


if __name__ == "__main__":
    main()

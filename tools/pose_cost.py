"""What gs4d_pose_records costs beside gs4d_transform_records.

Calls: 10^6 and 10^7 records of BASELINE.json configs[3]'s 4D set (scenes.cube_params_4d) posed with the INDEX and the BLEND4 form from tables of
m in {1, 64, 1024} rigid rows, the bind rows coherent (runs of 4096 records that name the same rows, as the splats of a joint or an object lie
together) or random, beside gs4d_transform_records with one transform at the same n — that call moves 192 bytes per record (96 read, 96 written), a
pose call 196 (INDEX) or 224 (BLEND4) plus whatever of the table does not come from a cache, so from the bytes alone a pose call should cost
196 / 192 or 224 / 192 of it.  Device time of a call: it is asynchronous and its kernel runs back to back with the next on one frame lane, so a window
is `calls` calls between two gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the entries of one n taking
turns to lead a round.  The two table-gather builds (make lib and make lib POSE_GLOBAL_TABLE=1) are two runs of this tool; the JSON line names
neither, so keep the outputs apart.
Prints one JSON line.  Usage: python tools/pose_cost.py [calls] [rounds] [largest n]."""
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
TABLES = (1, 64, 1024)
RUN = 4096                                                # records in a row that are bound alike in the coherent tables
BYTES = {"index": 196, "blend4": 224, "transform_records": 192}


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
    """m rigid rows: unit quaternions and shifts of a few units"""
    q = rng.standard_normal((m, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.stack([gs4d.affine4(q[k], 1.0, rng.uniform(-5.0, 5.0, 3)) for k in range(m)])


def joints_of(n, m, k, coherent, rng):
    """uint32 [n, k]: rows of the table, per run of RUN records or per record"""
    if not coherent:
        return rng.integers(m, size=(n, k)).astype(np.uint32)
    runs = rng.integers(m, size=((n + RUN - 1) // RUN, k)).astype(np.uint32)
    return np.repeat(runs, RUN, axis=0)[:n]


def measure_calls(calls, rounds, largest):
    sizes = [n for n in SIZES if n <= largest]
    rng = np.random.default_rng(0x504F5345)
    ctx = gs4d.Context(64, 64)
    nmax = max(sizes)
    src = ctx.buffer(records_of(nmax))
    dst = ctx.buffer(nbytes=96 * nmax)
    one = ctx.buffer(gs4d.affine4(translate=(1.0, 0.0, 0.0)).reshape(1, 20))
    tables = {m: ctx.buffer(table_of(m, rng)) for m in TABLES}
    binds = {}
    for m in TABLES:
        for how in ("coherent", "random"):
            if m == 1 and how == "random":
                continue                                   # (one row: every bind table is the same)
            j = joints_of(nmax, m, 4, how == "coherent", rng)
            w = rng.uniform(0.05, 1.0, (nmax, 4)).astype(np.float32)
            w /= w.sum(1, keepdims=True)
            binds["index", m, how] = ctx.buffer(np.ascontiguousarray(j[:, 0]))
            binds["blend4", m, how] = ctx.buffer(gs4d.bind_rows(j, w))
    res = {}
    for n in sizes:
        do = {f"{n}:transform_records": lambda n=n: ctx.transform_records(src, n, one, 1, dst=dst)}
        for (fname, m, how), bind in binds.items():
            form = gs4d.POSE_INDEX if fname == "index" else gs4d.POSE_BLEND4
            do[f"{n}:{fname}:m{m}:{how}"] = lambda n=n, m=m, bind=bind, form=form: ctx.pose_records(src, n, tables[m], bind, form, m, dst=dst)
        for call in do.values():
            call()
        out = turns(do, rounds, lambda call: window(ctx, call, calls))
        base = out[f"{n}:transform_records"]["ms"]
        for name in do:
            b = n * BYTES[name.split(":")[1]] / COPY_CEILING * 1e3
            out[name].update(ms_byte_budget=b, fraction_of_ceiling=b / out[name]["ms"], over_transform_records=out[name]["ms"] / base,
                             byte_ratio=BYTES[name.split(":")[1]] / 192.0)
        res.update(out)
    ctx.close()
    return res


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    print(json.dumps({"tool": "pose_cost", "calls": calls, "rounds": rounds, "records": measure_calls(calls, rounds, largest)}))


if __name__ == "__main__":
    main()

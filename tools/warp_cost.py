"""What gs4d_warp_records costs beside gs4d_transform_records and gs4d_pose_records.

Calls: 10^6 and 10^7 records of BASELINE.json configs[3]'s 4D set (scenes.cube_params_4d) warped through lattices of 8^3 and 17^3 nodes (static)
and 17^3 x 8 nodes (a time axis) laid over the set's bounding box, with the records in the order they were uploaded in and after reorder_spatial —
the order in which neighbouring lanes share nodes — beside gs4d_transform_records with one transform and gs4d_pose_records INDEX with m = 64 at the
same n.  gs4d_transform_records moves 192 bytes per record (96 read, 96 written); a warp call moves the same plus whatever of the lattice does not
come from a cache (8 or 16 nodes of 16 bytes are gathered per record), so from the bytes alone it should cost what gs4d_transform_records costs.
Device time of a call: it is asynchronous and its kernel runs back to back with the next on one frame lane, so a window is `calls` calls between two
gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the entries of one n taking turns to lead a round.  The
two node-gather builds (make lib and make lib WARP_GLOBAL_LATTICE=1) are two runs of this tool; the JSON line names neither, so keep the outputs
apart.
Prints one JSON line.  Usage: python tools/warp_cost.py [calls] [rounds] [largest n]."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
from pose_cost import COPY_CEILING, joints_of, records_of, table_of, turns, window  # noqa: E402  (the same windows, medians and turn-taking)

SIZES = (1_000_000, 10_000_000)
LATTICES = {"8x8x8": (8, 8, 8, 1), "17x17x17": (17, 17, 17, 1), "17x17x17x8": (17, 17, 17, 8)}
POSE_ROWS = 64
BYTES = {"warp": 192, "pose_index": 196, "transform_records": 192}


def lattice_over(rec, dims, rng):
    """(Lattice, nodes): the lattice over the bounding box of the centres, every record inside, with a smooth field of a few percent of the box"""
    p = rec[:, :4].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    hi = np.where(hi - lo > 1e-6, hi, lo + 1.0)
    lat = gs4d.lattice(lo, hi, dims)
    q = (gs4d.lattice_points(lat).astype(np.float64) - lo) / (hi - lo)
    nodes = 0.03 * (hi - lo) * np.sin(5.0 * q[..., ::-1] + rng.uniform(0.0, 6.0, 4))
    return lat, np.ascontiguousarray(nodes, np.float32)


def measure_calls(calls, rounds, largest):
    sizes = [n for n in SIZES if n <= largest]
    rng = np.random.default_rng(0x57415250)
    ctx = gs4d.Context(64, 64)
    nmax = max(sizes)
    rec = records_of(nmax)
    res = {}
    one = ctx.buffer(gs4d.affine4(translate=(1.0, 0.0, 0.0)).reshape(1, 20))
    table = ctx.buffer(table_of(POSE_ROWS, rng))
    bind = ctx.buffer(np.ascontiguousarray(joints_of(nmax, POSE_ROWS, 1, True, rng)[:, 0]))
    dst = ctx.buffer(nbytes=96 * nmax)
    for n in sizes:
        # the first n records in the order they come in, and the same n records in spatial order
        src = {"uploaded": ctx.buffer(rec[:n])}
        src["spatial"] = ctx.reorder_spatial(src["uploaded"], n)[0]
        do = {f"{n}:transform_records": lambda n=n, s=src["uploaded"]: ctx.transform_records(s, n, one, 1, dst=dst),
              f"{n}:pose_index:m{POSE_ROWS}": lambda n=n, s=src["uploaded"]: ctx.pose_records(s, n, table, bind, gs4d.POSE_INDEX, POSE_ROWS, dst=dst)}
        for lname, dims in LATTICES.items():
            lat, values = lattice_over(rec[:n], dims, rng)
            nodes = ctx.buffer(values)
            for order, s in src.items():
                do[f"{n}:warp:{lname}:{order}"] = lambda n=n, s=s, nodes=nodes, lat=lat: ctx.warp_records(s, n, nodes, lat, dst=dst)
        for call in do.values():
            call()
        out = turns(do, rounds, lambda call: window(ctx, call, calls))
        base = out[f"{n}:transform_records"]["ms"]
        for name in do:
            kind = name.split(":")[1]
            b = n * BYTES[kind] / COPY_CEILING * 1e3
            out[name].update(ms_byte_budget=b, fraction_of_ceiling=b / out[name]["ms"], over_transform_records=out[name]["ms"] / base, byte_ratio=BYTES[kind] / 192.0)
        res.update(out)
        ctx.finish()
        for s in src.values():
            ctx.delete(s)
    ctx.close()
    return res


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    print(json.dumps({"tool": "warp_cost", "calls": calls, "rounds": rounds, "records": measure_calls(calls, rounds, largest)}))


if __name__ == "__main__":
    main()

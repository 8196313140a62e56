"""What gs4d_decompose_records costs beside gs4d_transform_records.

Calls: 10^6 and 10^7 records of BASELINE.json configs[3]'s 4D set (scenes.cube_params_4d) taken out as GS4D_PARAMS_3D and as GS4D_PARAMS_4D_VEL, with
every destination of the form (the eigen-solve runs), with only rot and scale, and with the destinations that need no solve (the instance without
it), beside gs4d_transform_records with one transform at the same n in the same run.  A record is 96 bytes read; the rows written are 56 (3D) or 72
(4D_VEL) bytes with every destination, 28 with rot and scale alone, 28 / 44 without them: 124 to 168 bytes per record against the 192 of
gs4d_transform_records, so from the bytes alone every entry should cost less than that call.  The solve is some 12 rotations of two square roots and
two divisions each, correctly rounded: whether that puts the call above its memory time is what this tool measures.
Device time of a call: it is asynchronous and its kernel runs back to back with the next on one frame lane, so a window is `calls` calls between two
gs4d_finish, and the time of a call is the window over `calls`; medians of `rounds` windows, the entries of one n taking turns to lead a round.
Prints one JSON line.  Usage: python tools/decompose_cost.py [calls] [rounds] [largest n]."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
from pose_cost import COPY_CEILING, records_of, turns, window  # noqa: E402  (the same windows, medians and turn-taking)

SIZES = (1_000_000, 10_000_000)
FORMS = {"3d": gs4d.PARAMS_3D, "4d_vel": gs4d.PARAMS_4D_VEL}
# the destinations of an entry: every one of the form, the two the solve makes, and the rest
WANTED = {"all": None, "rot_scale": ("rot", "scale"), "no_solve": ("pos", "rgba", "dir", "tvar")}


def measure_calls(calls, rounds, largest):
    sizes = [n for n in SIZES if n <= largest]
    ctx = gs4d.Context(64, 64)
    nmax = max(sizes)
    src = ctx.buffer(records_of(nmax))
    dst = ctx.buffer(nbytes=96 * nmax)
    one = ctx.buffer(gs4d.affine4(translate=(1.0, 0.0, 0.0)).reshape(1, 20))
    res = {}
    for n in sizes:
        do = {f"{n}:transform_records": lambda n=n: ctx.transform_records(src, n, one, 1, dst=dst)}
        bytes_of = {f"{n}:transform_records": 192}
        held = []
        for fname, form in FORMS.items():
            rows = gs4d.PARAM_ROWS[form]
            for wname, only in WANTED.items():
                names = [k for k in rows if only is None or k in only]
                bufs = {k: ctx.buffer(nbytes=4 * rows[k] * n) for k in names}
                held += list(bufs.values())
                name = f"{n}:decompose:{fname}:{wname}"
                do[name] = lambda n=n, form=form, bufs=bufs: ctx.decompose_records(src, n, form, **bufs)
                bytes_of[name] = 96 + 4 * sum(rows[k] for k in names)
        for call in do.values():
            call()
        out = turns(do, rounds, lambda call: window(ctx, call, calls))
        base = out[f"{n}:transform_records"]["ms"]
        for name in do:
            b = n * bytes_of[name] / COPY_CEILING * 1e3
            out[name].update(bytes_per_record=bytes_of[name], ms_byte_budget=b, fraction_of_ceiling=b / out[name]["ms"],
                             over_transform_records=out[name]["ms"] / base, byte_ratio=bytes_of[name] / 192.0)
        res.update(out)
        ctx.finish()
        for b in held:
            ctx.delete(b)
    ctx.close()
    return res


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    largest = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
    print(json.dumps({"tool": "decompose_cost", "calls": calls, "rounds": rounds, "records": measure_calls(calls, rounds, largest)}))


if __name__ == "__main__":
    main()

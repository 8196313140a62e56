"""GPU: every buffer argument of every call on record sets and tables, made bad one fault at a time (csrc/operands.h).

One 64 x 64 context, n = 300 records.  Each case is one good call with ALL its buffer arguments given; for each argument in turn the call is made
with the name 0 (where the argument is required), a destroyed name, the name 9999, a buffer one element short (where the call asks the argument for
a size: dst and kept_index of the compactions hold what they hold) and the name of another argument of the same call.  Every such call returns
GS4D_E_INVALID; gs4d_last_error starts with "<fn>: ", names the argument, and differs from the message the refusal before it left — between two
faults the same call is refused for its record count, so a stale message cannot pass; after gs4d_finish every buffer the call writes still holds
what it held; and the good call then returns 0.  gs4d_build_records has two cases: no form takes all seven parameters.
"""
import ctypes as C

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu
N, W, H = 300, 64, 64
SENTINEL = 0xA5
TOO_MANY = 1 << 32            # a record count every call refuses before it looks at a buffer


class Arg:
    """one buffer argument: its name, what the good call's buffer holds, whether the call needs it, whether the call writes it, and the bytes of one
    element (None: the call asks it for no size)"""
    def __init__(self, name, content, required=True, written=False, element=None):
        self.name, self.content, self.required, self.written, self.element = name, np.ascontiguousarray(content).view(np.uint8).reshape(-1), required, written, element


def out(nbytes):
    return np.full(nbytes, SENTINEL, np.uint8)


def cases(gs4d, ctx):
    """[(id, fn, [Arg], call(names, n) -> rc)]: the call takes a dict argument name -> buffer name and the record count"""
    lib, h = gs4d._lib, ctx._h
    pos, q, scale, rgba = scenes.cube_params(N)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    f32 = lambda a, cols: np.ascontiguousarray(a, np.float32).reshape(N, -1)[:, :cols].copy()
    stats = np.zeros(N, gs4d.RECORD_STAT)
    rule, p = gs4d._keep_rule(min_pixels=0), gs4d._ptr
    spans = np.zeros((N, 2), np.float32)
    view, proj = gs4d.look_at(scenes.CAM_CUBE[0], scenes.CAM_CUBE[1]), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    m_buf = ctx.measure_records(ctx.buffer(rec), N)
    measure = ctx.read(m_buf, np.uint8, C.sizeof(gs4d.Measure))
    table = lambda name, written=False, required=True: Arg(name, stats, required, written, 16)
    compact = lambda tab: [Arg(tab, stats if tab == "stats" else spans, element=16 if tab == "stats" else 8), Arg("src", rec, False, element=96),
                           Arg("dst", out(N * 96), False, True), Arg("kept_index", out(N * 4), False, True), Arg("count", out(8), True, True, 1)]
    edit = gs4d.colour_edit("copy")
    xs = gs4d.selection_xf(gs4d.affine4(), measure=True)
    sl = gs4d.slice_query(0.0)
    region = gs4d.IdRegion(0, 0, 8, 8, 0, 0xFFFFFFFF, 0, 0)
    cq = gs4d.centre_query(screen=(view, proj), rect=(0, 0, 8, 8))
    mq, nq, kq, rq = gs4d.measure_query(), gs4d.neighbour_query(0.1), gs4d.component_query(0.1), gs4d.nearest_query(0.1, 3)
    stride = gs4d.hit_stride_for(3)
    cam = np.zeros(3, np.float32)

    def build(form, rot_r, dir_, tvar):
        def call(a, n):
            sp = gs4d.SplatParams(form, 0, a["pos"], a["rot"], a.get("rot_r", 0), a["scale"], a["rgba"], a.get("dir", 0), a.get("tvar", 0), 0)
            return lib.gs4d_build_records(h, C.byref(sp), n, a["dst"])
        args = [Arg("pos", np.zeros((N, 4), np.float32), element=16), Arg("rot", f32(q, 4), element=16)]
        args += [Arg("rot_r", f32(q, 4), element=16)] if rot_r else []
        args += [Arg("scale", np.ones((N, 4 if rot_r else 3), np.float32), element=16 if rot_r else 12), Arg("rgba", f32(rgba, 4), element=16)]
        args += [Arg("dir", np.zeros((N, 3), np.float32), element=12)] if dir_ else []
        args += [Arg("tvar", np.ones(N, np.float32), element=4)] if tvar else []
        return args + [Arg("dst", out(N * 96), True, True, 96)], call

    vel_args, vel_call = build(gs4d.PARAMS_4D_VEL, False, True, True)
    twoq_args, twoq_call = build(gs4d.PARAMS_4D_2Q, True, False, False)
    grid_args = lambda first: [Arg("data", rec, element=96), table("source", required=False)] + first + [table("stats", True, not first)]
    return [
        ("compact_records", "compact_records", compact("stats"),
         lambda a, n: lib.gs4d_compact_records(h, a["stats"], n, p(rule), a["src"], 96, a["dst"], a["kept_index"], a["count"])),
        ("stat_cut", "stat_cut", [table("stats"), Arg("out", out(16), True, True, 1)],
         lambda a, n: lib.gs4d_stat_cut(h, a["stats"], n, gs4d.STAT_WSUM, 10, a["out"])),
        ("record_time_spans", "record_time_spans", [Arg("data", rec, element=96), Arg("spans", out(N * 8), True, True, 8)],
         lambda a, n: lib.gs4d_record_time_spans(h, a["data"], n, 0.0, a["spans"])),
        ("compact_time_window", "compact_time_window", compact("spans"),
         lambda a, n: lib.gs4d_compact_time_window(h, a["spans"], n, 0.0, 1.0, a["src"], 96, a["dst"], a["kept_index"], a["count"])),
        ("spatial_order", "spatial_order", [Arg("src", rec, element=96), Arg("order_index", out(N * 4), True, True, 4)],
         lambda a, n: lib.gs4d_spatial_order(h, a["src"], n, 96, 0, a["order_index"])),
        ("gather_records", "gather_records", [Arg("index", np.arange(N, dtype=np.uint32)[::-1], element=4), Arg("src", rec, element=96), Arg("dst", out(N * 96), True, True, 96)],
         lambda a, n: lib.gs4d_gather_records(h, a["index"], n, a["src"], min(n, N), 96, a["dst"])),
        ("shade_sh", "shade_sh", [Arg("data", rec, True, True, 96), Arg("sh", np.zeros((N, 12), np.float32), element=48)],
         lambda a, n: lib.gs4d_shade_sh(h, a["data"], n, a["sh"], 48, 1, 0.0, p(cam))),
        ("edit_colours", "edit_colours", [Arg("data", rec, True, True, 96), table("stats", required=False), Arg("from", rec, False, element=96)],
         lambda a, n: lib.gs4d_edit_colours(h, a["data"], n, p(edit), a["stats"], p(rule), a["from"])),
        ("build_records-vel", "build_records", vel_args, vel_call),
        ("build_records-2q", "build_records", twoq_args, twoq_call),
        ("transform_records", "transform_records", [Arg("src", rec, element=96), Arg("xf", np.stack([gs4d.affine4(), gs4d.affine4(scale=2.0)]), element=80),
                                                    Arg("dst", out((3 + 2 * N) * 96), True, True, 96)],
         lambda a, n: lib.gs4d_transform_records(h, a["src"], n, a["xf"], 2, a["dst"], 3)),
        ("slice_records", "slice_records", [Arg("src", rec, element=96), Arg("dst", out((3 + N) * 96), True, True, 96)],
         lambda a, n: lib.gs4d_slice_records(h, a["src"], n, C.byref(sl), a["dst"], 3)),
        ("transform_selected", "transform_selected", [Arg("data", rec, True, True, 96), table("stats", required=False), Arg("measure", measure, False, element=1)],
         lambda a, n: lib.gs4d_transform_selected(h, a["data"], n, C.byref(xs), a["stats"], p(rule), a["measure"])),
        ("count_ids", "count_ids", [Arg("mask", np.ones(64, np.uint8), False, element=1), table("stats", True)],
         lambda a, n: lib.gs4d_count_ids(h, C.byref(region), a["mask"], a["stats"], n)),
        ("count_centres", "count_centres", [Arg("data", rec, element=96), Arg("mask", np.ones(64, np.uint8), False, element=1), table("stats", True)],
         lambda a, n: lib.gs4d_count_centres(h, a["data"], n, C.byref(cq), a["mask"], a["stats"])),
        ("measure_records", "measure_records", [Arg("data", rec, element=96), table("stats", required=False), Arg("out", out(96), True, True, 1)],
         lambda a, n: lib.gs4d_measure_records(h, a["data"], n, C.byref(mq), a["stats"], p(rule), a["out"])),
        ("count_neighbours", "count_neighbours", grid_args([]),
         lambda a, n: lib.gs4d_count_neighbours(h, a["data"], n, C.byref(nq), a["source"], p(rule), a["stats"])),
        ("label_components", "label_components", grid_args([Arg("labels", out(N * 4), True, True, 4)]),
         lambda a, n: lib.gs4d_label_components(h, a["data"], n, C.byref(kq), a["source"], p(rule), a["labels"], a["stats"])),
        ("count_labels", "count_labels", [Arg("labels", np.arange(N, dtype=np.uint32), element=4), table("seeds"), table("stats", True)],
         lambda a, n: lib.gs4d_count_labels(h, a["labels"], n, a["seeds"], p(rule), a["stats"])),
        ("nearest_neighbours", "nearest_neighbours", grid_args([Arg("hits", out(N * stride), True, True, stride)]),
         lambda a, n: lib.gs4d_nearest_neighbours(h, a["data"], n, C.byref(rq), a["source"], p(rule), a["hits"], stride, a["stats"])),
    ]


CASE_IDS = ["compact_records", "stat_cut", "record_time_spans", "compact_time_window", "spatial_order", "gather_records", "shade_sh", "edit_colours",
            "build_records-vel", "build_records-2q", "transform_records", "slice_records", "transform_selected", "count_ids", "count_centres",
            "measure_records", "count_neighbours", "label_components", "count_labels", "nearest_neighbours"]


@pytest.fixture(scope="module")
def world(gs4d):
    ctx = gs4d.Context(W, H)
    ctx.set_id_outputs(True)          # gs4d_count_ids reads the ID planes of the current frame
    ctx.clear()
    table = {c[0]: c for c in cases(gs4d, ctx)}
    assert list(table) == CASE_IDS
    yield gs4d, ctx, table
    ctx.close()


@pytest.mark.parametrize("case", CASE_IDS)
def test_every_argument_made_bad_one_fault_at_a_time(world, case):
    gs4d, ctx, table = world
    lib, h = gs4d._lib, ctx._h
    _, fn, args, call = table[case]
    good = {a.name: ctx.buffer(a.content) for a in args}
    short = {a.name: ctx.buffer(a.content[:a.content.size - a.element]) for a in args if a.element is not None}
    message = lambda: lib.gs4d_last_error(h).decode()
    previous = [message()]

    def refused(names, n, argument=None):
        rc = call(names, n)
        msg = message()
        print(f"{case}: {argument or 'n'} -> {msg}")
        assert rc == -1, (argument, rc, msg)
        assert msg.startswith(fn + ": "), (argument, msg)
        assert msg != previous[0], (argument, msg)
        if argument is not None:
            assert argument in msg[len(fn) + 2:], (argument, msg)
        previous[0] = msg
        assert lib.gs4d_finish(h) == 0
        for a in args:
            if a.written:
                assert np.array_equal(ctx.read(good[a.name], np.uint8, a.content.size), a.content), (argument, a.name)

    dead = ctx.buffer(nbytes=16)
    ctx.delete(dead)                    # (a destroyed name stays dead until the next buffer is created: none is, below)
    faults = 0
    for i, a in enumerate(args):
        other = args[(i + 1) % len(args)].name
        for bad in ([0] if a.required else []) + [dead, 9999] + ([short[a.name]] if a.name in short else []) + [good[other]]:
            refused(good, TOO_MANY)                                   # the call's own refusal in between: the next message must replace it
            refused(dict(good, **{a.name: bad}), N, a.name)
            faults += 1
    assert faults >= len(args) * 3
    assert call(good, N) == 0, message()
    assert lib.gs4d_finish(h) == 0, message()
    for b in list(good.values()) + list(short.values()):
        ctx.delete(b)

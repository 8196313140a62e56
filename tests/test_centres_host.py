"""CPU: gs4d_host_count_centres — the definition of gs4d_count_centres (include/gs4d.h) — against the numpy restatement of
tests/centre_cases.py, table byte for byte; the cases say something (none is vacuous); calls combine as set arithmetic; and for a symmetric set the
window position of the restatement is, bit for bit, the centre the CPU checker's projection gives the draws."""
import numpy as np
import pytest

import centre_cases as cc
import hostile_cases


def host(gs4d, rec, q, table, mask=None, width=cc.W, height=cc.H):
    return gs4d.count_centres_host(rec, cc.struct(q), width, height, mask=mask, stats=table).view(cc.STAT)


def check(gs4d, rec, q, mask, what, kinds=("zero", "random")):
    """the host definition against the restatement on a zeroed and on a random table; returns who takes part"""
    n = rec.shape[0]
    part = None
    for kind in kinds:
        table = cc.table(kind, n)
        want, part = cc.restate(rec, q, table, mask)
        got = host(gs4d, rec, q, table, mask)
        assert got.tobytes() == want.tobytes(), f"{what}, {kind} table: {int((got != want).sum())} rows differ from the restatement"
        # what the restatement itself must do: rows that do not take part keep their bits, ADD adds, REMOVE zeroes
        assert want[~part].tobytes() == table[~part].tobytes(), what
        if q["op"] == cc.ADD:
            assert np.array_equal(want["pixels"][part], table["pixels"][part] + np.uint32(1)), what
            assert np.array_equal(want["wsum"][part], table["wsum"][part] + np.uint64(1 << 24)), what
            assert (want["wmax"][part] >= cc.ONE_BITS).all() and np.array_equal(want["wmax"][part], np.maximum(table["wmax"][part], cc.ONE_BITS)), what
        else:
            assert not want[part].view(np.uint8).any(), what
    return part


def test_the_binding_has_the_call(gs4d):
    assert {"gs4d_count_centres", "gs4d_host_count_centres"} <= set(gs4d.EXPORTS)
    import ctypes
    assert ctypes.sizeof(gs4d.CentreQuery) == 256
    q = gs4d.centre_query(box=((-1, -2, -3), (1, 2, 3)), sphere=((0.5, 0.25, 0.125), 2.0), frame=np.arange(12), screen=cc.mats(), rect=(1, 2, 3, 4),
                          depth=(0.5, 9.0), t=1.5, skip_hidden=True, skip_dead=True, remove=True)
    assert (q.tests, q.op, q.t, q.reserved) == (cc.ALL_BITS, cc.REMOVE, 1.5, 0)
    assert list(q.box_lo) == [-1, -2, -3] and list(q.box_hi) == [1, 2, 3] and list(q.sphere) == [0.5, 0.25, 0.125, 2.0] and list(q.frame) == list(range(12))
    assert (q.x, q.y, q.w, q.h, q.depth_min, q.depth_max) == (1, 2, 3, 4, 0.5, 9.0)
    assert np.array_equal(np.array(q.view[:], np.float32), cc.mats()[0].ravel()) and np.array_equal(np.array(q.proj[:], np.float32), cc.mats()[1].ravel())
    assert list(gs4d.centre_query(frame=np.arange(12).reshape(4, 3).T).frame) == list(range(12))      # a [3, 4] array: rows of the matrix
    plain = gs4d.centre_query()
    assert (plain.tests, plain.op, plain.t) == (0, cc.ADD, 0.0)
    with pytest.raises(TypeError):
        gs4d.centre_query(screen=cc.mats())
    with pytest.raises(TypeError):
        gs4d.centre_query(rect=(0, 0, 1, 1))


@pytest.mark.parametrize("kind", cc.KINDS)
def test_the_host_definition_equals_the_restatement(gs4d, kind):
    """every subset of the six test bits, both ops, every size.  Non-vacuity, by the restatement alone: at every size of a tile or more, a subset
    with a test bit other than FRAME (which has no effect alone) takes some records and leaves some; the two subsets without one take every
    record, as the definition says."""
    for n in cc.SIZES:
        rec = cc.records(kind, n)
        mask = cc.mask_for(cc.RECT)
        for tests in cc.subsets():
            for op in (cc.ADD, cc.REMOVE):
                q = cc.query(tests, op)
                part = check(gs4d, rec, q, mask if tests & cc.SCREEN else None, f"{kind}, n = {n}, tests = {tests}, op = {op}")
                if tests & ~cc.FRAME == 0:
                    assert part.all(), (kind, n, tests)
                elif n >= cc.TILE - 1:
                    assert 0 < int(part.sum()) < n, f"{kind}, n = {n}, tests = {tests}: a vacuous case ({int(part.sum())} of {n} take part)"
            if tests & cc.SCREEN and n >= cc.TILE - 1:                   # ... and the mask itself leaves records out that the rectangle takes
                q = cc.query(tests)
                assert int(cc.takes_part(rec, q, mask).sum()) < int(cc.takes_part(rec, q, None).sum()), (kind, n, tests)
                check(gs4d, rec, q, None, f"{kind}, n = {n}, tests = {tests}, no mask", kinds=("random",))


def test_frame_alone_has_no_effect_and_frame_moves_the_volume(gs4d):
    """through the host definition: FRAME changes who a BOX or SPHERE takes, FRAME without either changes nothing — also not the screen test"""
    rec = cc.records("symmetric", 1000)
    zero = cc.table("zero", 1000)
    took = lambda tests: host(gs4d, rec, cc.query(tests), zero, cc.mask_for(cc.RECT) if tests & cc.SCREEN else None)["pixels"] == 1
    for tests in (cc.BOX, cc.SPHERE, cc.BOX | cc.SPHERE):
        a, b = took(tests), took(tests | cc.FRAME)
        assert np.array_equal(a, check(gs4d, rec, cc.query(tests), None, f"tests = {tests}"))
        assert np.array_equal(b, check(gs4d, rec, cc.query(tests | cc.FRAME), None, f"tests = {tests | cc.FRAME}"))
        assert (a != b).sum() > 10, "the frame changed nothing"
    for tests in (0, cc.SCREEN, cc.SKIP_HIDDEN, cc.SCREEN | cc.SKIP_DEAD):
        assert np.array_equal(took(tests), took(tests | cc.FRAME)), tests
    assert took(cc.FRAME).all() and 0 < took(cc.SCREEN | cc.FRAME).sum() < 1000


@pytest.mark.parametrize("rect", cc.EDGE_RECTS, ids=lambda r: "x%d_y%d_w%d_h%d" % r)
def test_a_rectangle_that_touches_the_image_edges(gs4d, rect):
    x, y, w, h = rect
    assert x == 0 or y == 0 or x + w == cc.W or y + h == cc.H
    for kind in cc.KINDS:
        rec = cc.records(kind, 1000)
        for tests in (cc.SCREEN, cc.ALL_BITS):
            for mask in (None, cc.mask_for(rect)):
                part = check(gs4d, rec, cc.query(tests, rect=rect), mask, f"{kind}, rect = {rect}, tests = {tests}")
                assert 0 < int(part.sum()) < 1000, (kind, rect, tests, int(part.sum()))


def test_the_rectangle_bounds_are_half_open_in_window_coordinates(gs4d):
    """records placed so that wx falls exactly on x, just below x + w and exactly on x + w: in, in, out"""
    rec = np.array(cc.records("static3d", 64), copy=True)
    q = cc.query(cc.SCREEN, rect=(32, 24, 8, 8), depth=(0.0, cc.INF))
    rec[:, 0:3] = 0.0                                           # on the camera's axis: the centre of the image, wx = 32, wy = 24 exactly
    wx, wy, _, _ = cc.window(rec, q)
    assert (wx == 32.0).all() and (wy == 24.0).all()
    assert check(gs4d, rec, q, None, "on the lower bounds").all()
    assert not check(gs4d, rec, cc.query(cc.SCREEN, rect=(24, 16, 8, 8), depth=(0.0, cc.INF)), None, "on the upper bounds").any()
    assert not check(gs4d, rec, cc.query(cc.SCREEN, rect=(24, 24, 8, 8), depth=(0.0, cc.INF)), None, "on the upper x bound").any()
    # the depth range is closed: -pc.z of these records is exactly 150
    _, _, depth, _ = cc.window(rec, q)
    assert (depth == 150.0).all()
    assert check(gs4d, rec, cc.query(cc.SCREEN, rect=(32, 24, 8, 8), depth=(150.0, 150.0)), None, "the closed depth range").all()
    assert not check(gs4d, rec, cc.query(cc.SCREEN, rect=(32, 24, 8, 8), depth=(150.00002, 200.0)), None, "above the depth").any()


def test_hostile_record_sets(gs4d):
    """the records of tests/hostile_cases.py, with each case's own time and camera: whatever they select, the definition and the restatement agree"""
    total = 0
    for case in hostile_cases.all_cases():
        for k, q in enumerate(cc.hostile_queries(case)):
            mask = cc.mask_for(q["rect"]) if (q["tests"] & cc.SCREEN and k % 2 == 0) else None
            total += int(check(gs4d, case.rec, q, mask, f"{case.name}, query {k}", kinds=("random",)).sum())
    assert total > 1000, "the hostile sets select next to nothing"


def test_non_finite_operands_are_data(gs4d):
    for kind in cc.KINDS:
        rec = cc.records(kind, cc.TILE + 1)
        for name, q in cc.nonfinite_queries():
            mask = cc.mask_for(q["rect"]) if q["tests"] & cc.SCREEN else None
            check(gs4d, rec, q, mask, f"{kind}, {name}", kinds=("random",))
    # what the definition says they select
    rec = cc.records("symmetric", 1000)
    part = lambda name: cc.takes_part(rec, dict(cc.nonfinite_queries())[name])
    assert not part("t_nan_no_skip").any() and not part("box_lo_nan").any() and not part("radius_nan").any() and not part("box_inverted").any()
    assert np.array_equal(part("radius_negative"), cc.takes_part(rec, cc.query(cc.SPHERE)))
    assert part("radius_3e38").all() and np.array_equal(part("radius_pinf"), rec[:, 7] > 0)
    assert not part("zero_matrices").any() and not part("depth_min_pinf").any() and not part("depth_max_ninf").any()


def test_a_query_the_device_call_would_refuse_changes_nothing(gs4d):
    rec = cc.records("symmetric", 300)
    table = cc.table("random", 300)
    mask = cc.mask_for(cc.RECT)

    def unchanged(q, mask=None, **fields):
        s = cc.struct(q)
        for k, v in fields.items():
            setattr(s, k, v)
        got = gs4d.count_centres_host(rec, s, cc.W, cc.H, mask=mask, stats=table)
        return got.tobytes() == table.tobytes()

    assert not unchanged(cc.query(cc.ALL_BITS), mask)           # the premise: the valid query changes rows
    assert unchanged(cc.query(cc.ALL_BITS), tests=64) and unchanged(cc.query(cc.ALL_BITS), tests=0x80000000 | cc.BOX)
    assert unchanged(cc.query(cc.BOX), op=2) and unchanged(cc.query(cc.BOX), reserved=1)
    assert unchanged(cc.query(cc.BOX), mask)                    # a mask without SCREEN
    for rect in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (60, 0, 5, 8), (0, 44, 8, 5), (0, 0, 65, 8), (0, 0, 8, 49)):
        assert unchanged(cc.query(cc.SCREEN, rect=rect)), rect
    assert not unchanged(cc.query(cc.BOX, rect=(-5, -5, 0, 0)))     # without SCREEN the rectangle is not looked at


def test_three_calls_combine_as_sets(gs4d):
    """on a zeroed table each ADD adds at most one to pixels: rule {1,0,0,0} is the union, {3,0,0,0} the intersection; REMOVE subtracts"""
    for kind in cc.KINDS:
        rec = cc.records(kind, 1000)
        mask = cc.mask_for(cc.RECT)
        calls = [(cc.query(cc.BOX | cc.FRAME), None), (cc.query(cc.SPHERE | cc.SKIP_HIDDEN), None), (cc.query(cc.SCREEN), mask)]
        sets = [cc.takes_part(rec, q, m) for q, m in calls]
        table = cc.table("zero", 1000)
        for q, m in calls:
            table = host(gs4d, rec, q, table, m)
        union, inter = sets[0] | sets[1] | sets[2], sets[0] & sets[1] & sets[2]
        assert np.array_equal(table["pixels"] >= 1, union) and np.array_equal(table["pixels"] >= 3, inter)
        assert np.array_equal(table["pixels"], sets[0].astype(np.uint32) + sets[1] + sets[2])
        assert np.array_equal(table["wsum"], table["pixels"].astype(np.uint64) << np.uint64(24)) and np.array_equal(table["wmax"] != 0, union)
        assert 0 < inter.sum() < union.sum() < 1000 and all(inter.sum() < s.sum() < union.sum() for s in sets)
        cut = cc.query(cc.SKIP_DEAD | cc.BOX, cc.REMOVE, box_lo=(-100.0, -100.0, -100.0), box_hi=(0.0, 100.0, 100.0))
        gone = cc.takes_part(rec, cut)
        table = host(gs4d, rec, cut, table)
        assert np.array_equal(table["pixels"] >= 1, union & ~gone) and 0 < (union & gone).sum() < union.sum()
        assert not table[gone].view(np.uint8).any()


def test_the_window_position_is_the_draws_centre(gs4d, oracle):
    """for a symmetric set, wx and wy of the restatement are the cx and cy the CPU checker projects, bit for bit, wherever it calls the record valid"""
    view, proj = cc.mats()
    valid_total = 0
    for kind, t in (("symmetric", cc.T), ("symmetric", cc.T + 0.75), ("static3d", cc.T)):
        rec = cc.records(kind, 1000)
        pj = oracle.preprocess(oracle.MODE_4D_DIRECT, rec, view, proj, cc.W, cc.H, t=t, min_opacity=0.0)
        wx, wy, depth, psw = cc.window(rec, cc.query(cc.SCREEN, t=t))
        valid = pj["valid"] != 0
        valid_total += int(valid.sum())
        assert np.array_equal(wx[valid].view(np.uint32), pj["cx"][valid].view(np.uint32)), kind
        assert np.array_equal(wy[valid].view(np.uint32), pj["cy"][valid].view(np.uint32)), kind
        assert (psw[valid] > 0).all()
    assert valid_total > 1500

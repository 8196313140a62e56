"""CPU: gs4d_host_measure_records — the definition of gs4d_measure_records (include/gs4d.h) — against the numpy restatement of the
header's text (tests/measure_cases.py), byte for byte; the centroid of gs4d_host_measure_centre; the camera of gs4d_host_frame_box."""
import numpy as np

import measure_cases as mc
import scenes

f32, f64 = np.float32, np.float64


def check(rec, t, flags, stats, rule, invert, what):
    got = mc.host(rec, t, flags, stats, rule, invert)
    want, p = mc.restate(rec, t, flags, stats, rule, invert)
    assert got.tobytes() == want.tobytes(), f"{what}:\n{got}\n{want}"
    return want[0], p


class Premises:
    """what the case matrix must have exercised somewhere, so that no case is vacuous"""

    def __init__(self):
        self.count = self.unplaced = self.skipped = self.var_le_0 = self.end_left_out = self.e_zero = 0

    def add(self, m, p):
        on = p["measured"]
        self.count += int(m["count"])
        self.unplaced += int(m["unplaced"])
        self.skipped += int(m["skipped"])
        with np.errstate(all="ignore"):
            self.var_le_0 += int((p["var"][on] <= 0).sum())
        self.end_left_out += int((~np.isfinite(p["e0"][on])).sum() + (~np.isfinite(p["e1"][on])).sum())
        self.e_zero += int(sum(m["count"] > 0 and m["hi"][a] == m["lo"][a] for a in range(3)))

    def hold(self):
        assert self.count and self.unplaced and self.skipped and self.var_le_0 and self.end_left_out and self.e_zero, vars(self)


def test_the_host_definition_equals_the_restatement_byte_for_byte():
    seen = Premises()
    per_kind = {k: Premises() for k in mc.KINDS}
    for kind, n, t, flags, form in mc.matrix(sizes=(1, 65, 257, 1000)):
        rec = mc.records(kind, n)
        stats, rule, invert = mc.selection(n, form)
        m, p = check(rec, t, flags, stats, rule, invert, f"{kind}, n = {n}, t = {t}, flags = {flags}, {form}")
        seen.add(m, p)
        per_kind[kind].add(m, p)
        if form != "all" and n > 1:
            assert 0 < int(p["selected"].sum()) < n
    seen.hold()
    for kind in ("static3d", "symmetric"):                      # both skips bite in the sets of the issue, not only in the hand-made one
        assert per_kind[kind].count and per_kind[kind].skipped, kind
    dead = mc.parts(mc.records("symmetric", 1000), mc.T, mc.SKIP_DEAD)["skipped"].sum()
    assert 0 < dead < 1000, "no part of the 4D set is dead at T"


def test_hostile_record_sets():
    seen = Premises()
    for case in mc.hostile_sets():
        for flags in mc.FLAGS:
            for form in mc.FORMS:
                stats, rule, invert = mc.selection(case.n, form)
                seen.add(*check(case.rec, case.t, flags, stats, rule, invert, f"{case.name}, flags = {flags}, {form}"))
    assert seen.count and seen.unplaced and seen.skipped, vars(seen)


def test_non_finite_times_are_data():
    rec = mc.records("symmetric", 257)
    for t in (mc.NAN, mc.INF, -mc.INF, 3e38):
        for flags in mc.FLAGS:
            check(rec, t, flags, None, mc.RULE, False, f"t = {t}, flags = {flags}")


def test_a_box_end_has_the_bits_of_minus_zero_below_and_plus_zero_above_in_either_order():
    """+0 and -0 on x (sig3.x = -0 and dt = +0: k * sig3 = -0, so the centre keeps the sign of the position)"""
    rec = np.zeros((2, 24), f32)
    rec[:, 8], rec[:, 13], rec[:, 18], rec[:, 23], rec[:, 7], rec[:, 20] = 1.0, 1.0, 1.0, 1.0, 1.0, -0.0
    rec[0, 0], rec[1, 0] = 0.0, -0.0
    for order in (rec, rec[::-1].copy()):
        m, p = check(order, 0.0, 0, None, mc.RULE, False, "zeros")
        assert sorted(np.ascontiguousarray(p["m"][:, 0]).view(np.uint32).tolist()) == [0, 0x80000000], "the set does not hold both zeros"
        assert m["lo"][:1].view(np.uint32)[0] == 0x80000000 and m["hi"][:1].view(np.uint32)[0] == 0
        assert m["count"] == 2 and m["cell_sum"][0] == 0


def test_an_empty_selection_gives_the_empty_measurement():
    rec = mc.records("symmetric", 65)
    none = mc.one_selected(65, 3)
    empty = np.zeros(1, mc.MEASURE)
    empty["lo"], empty["hi"], empty["ext_lo"], empty["ext_hi"] = mc.INF, -mc.INF, mc.INF, -mc.INF
    for got in (mc.host(rec[:0], 1.0, 3), mc.host(rec, mc.T, 0, none[0], (1 << 31, 0, 0), False),
                mc.host(rec, mc.T, 0, np.zeros(65, mc.ec.STAT), (0, 0, 0), True)):
        assert got.tobytes() == empty.tobytes(), got
    # everything selected is skipped or unplaced: the counters move, the boxes stay empty
    hidden = np.array(rec, copy=True)
    hidden[:, 7] = 0.0
    got = mc.host(hidden, mc.T, mc.SKIP_HIDDEN)[0]
    assert (got["count"], got["unplaced"], got["skipped"]) == (0, 0, 65) and got["lo"][0] == mc.INF and got["ext_hi"][2] == -mc.INF and not got["cell_sum"].any()
    # a query the device call would refuse
    g = mc._gs4d()
    q = mc.struct(mc.T, 4)
    assert bytes(g.measure_records_host(rec, query=q)) == empty.tobytes()
    q = mc.struct(mc.T, 0)
    q.reserved[1] = 1
    assert bytes(g.measure_records_host(rec, query=q)) == empty.tobytes()


def test_the_centre_is_the_mean_of_the_centres_to_within_the_cells():
    g = mc._gs4d()
    for kind, n, t in (("static3d", 1000, mc.T), ("symmetric", 1000, mc.T), ("symmetric", 257, mc.T - 0.25), ("static3d", 1, 0.0)):
        rec = mc.records(kind, n)
        m = g.measure_records_host(rec, t=t)
        d = m.as_dict()
        p = mc.parts(rec, t, 0)
        assert d["count"] == n == int(p["measured"].sum()) and d["centre"] is not None
        mean = p["m"].astype(f64).mean(0)
        ext = d["hi"].astype(f64) - d["lo"].astype(f64)
        assert (np.abs(d["centre"].astype(f64) - mean) <= ext * 2.0 ** -19).all(), (kind, n, d["centre"], mean)
        assert n == 1 or (ext > 1.0).all()
    empty = g.measure_records_host(mc.records("symmetric", 65)[:0])
    assert empty.as_dict()["centre"] is None
    out = np.ones(3, f32)
    assert g._lib.gs4d_host_measure_centre(None, out.ctypes.data) == 0 and not out.any()


def test_frame_box_shows_the_whole_box_with_its_centre_in_the_middle():
    g = mc._gs4d()
    u = scenes.uniform(9 * 40, 2, seed=0x4D55).reshape(40, 9)
    for k, row in enumerate(u):
        c, half, o = (row[0:3] - 0.5) * 40.0, row[3:6] * 10.0 + 0.05, row[6:9] - 0.5
        o[2] -= 0.75 if o[2] <= 0 else -0.75                     # (never close to the zero vector, never along the up vector alone)
        lo, hi = (c - half).astype(f32), (c + half).astype(f32)
        fov, (w, h) = (30.0, 45.0, 70.0)[k % 3], ((64, 48), (48, 64), (200, 200))[k % 3 if k < 20 else (k + 1) % 3]
        eye = g.frame_box(lo, hi, o, fov, w, h)
        view, proj = g.look_at(eye, o), g.perspective(fov, w, h, scenes.ZNEAR, scenes.ZFAR)
        vp = proj.reshape(4, 4).T.astype(f64) @ view.reshape(4, 4).T.astype(f64)
        corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[l][2], 1.0] for i in (0, 1) for j in (0, 1) for l in (0, 1)], f64)
        clip = corners @ vp.T
        assert (clip[:, 3] > 0).all()
        px, py = (clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * w, (clip[:, 1] / clip[:, 3] * 0.5 + 0.5) * h
        assert (px > 0).all() and (px < w).all() and (py > 0).all() and (py < h).all(), (k, px, py)
        mid = np.append((lo.astype(f64) + hi.astype(f64)) * 0.5, 1.0) @ vp.T
        assert abs((mid[0] / mid[3] * 0.5 + 0.5) * w - w / 2) < 1e-3 and abs((mid[1] / mid[3] * 0.5 + 0.5) * h - h / 2) < 1e-3, k
    # a degenerate box is seen from the distance of a sphere of radius 1
    one = g.frame_box((1, 2, 3), (1, 2, 3), (0, 0, -2), 90.0, 64, 64)
    assert np.allclose(one, (1.0, 2.0, 3.0 + 2.0 ** 0.5), atol=1e-6)

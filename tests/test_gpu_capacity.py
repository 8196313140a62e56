"""GPU: every instantiation of the unordered path's compositor — list capacity x record form x outputs x depth test.

k_composite_v2<PREMULT_C, PER, OUT, ZTEST> (csrc/composite2.hip) is 96 kernels: PER = list capacity / 64 in {1, 2, 3, 4, 6, 8, 12, 16}, chosen by the
host from the longest tile list of earlier draws (csrc/gs4d_api.hip, resolve_lane).  tests/capacity_cases.py builds, for every rung, one image
whose longest list lands on it, and tests/test_capacity_host.py proves on the CPU that the list's order shows (removing or swapping one entry
moves a pixel by more than ten times the bar used here).  Each cell below draws that image as 4D records (MODE_4D_SORTED, view-z keys, ties)
or as 3D-Full quads (index keys, premultiplied colour) with one output set and with or without a depth test, and

* proves the rung with the counters that exist: longest_list equals the L of the CPU, the draw stayed on the unordered path; above 256 the
  first frame is re-run exactly once (the growth) and the repeated frame not at all; below 256 the context is warmed until the capacity has
  shrunk, and a PROBE frame whose longest list is just over the rung, but under 256, is re-run once — a capacity still at 256 would hold
  it.  (A list-only miss counts as a re-run, not as a staged miss: tests/test_gpu_staged_misses.py case d pins that, so reruns is the
  counter asserted here and staged_misses must stay.)  A list of 1060 leaves the unordered path (tile_sort_passes >= 2);
* compares every frame (both frames, the probe frame too) with the CPU checker: colour within 1e-4; aux by colour substitution within the
  bars of tests/test_gpu_aux.py, colour bit-equal to the colour cell; IDs against the numpy restatement under check_parity's rules, colour
  and aux bit-equal to the cells below; with the depth test, the checker with the hidden records' alpha zeroed per plane value and merged
  per pixel, and the GPU twin bit for bit (tests/ztest_cases.py).

Beside the matrix, at the 1024 rung's image: depth slabs (4, 32), the ordered path as cross-check (bit-equal), a tile shard, one lane, and
an image whose sides are not multiples of 8 with the long tile clipped in the corner.

That the matrix reaches all 96 instantiations is shown by the kernel-name table of a kernel-trace run of this file,
profiles/capacity_kernel_names.txt (profiles/README.md).
"""
import numpy as np
import pytest

import capacity_cases as cc
import id_cases
import staged_cases as sc
import ztest_cases as zc
from test_gpu_aux import substituted
from test_gpu_ids import check_parity
from test_gpu_render import TOL

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
OUTPUTS = ["colour", "aux", "ids"]
FORMS = ["4d", "quads"]
KNOBS = ("GS4D_DRAW_PATH", "GS4D_SLABS", "GS4D_LANES", "GS4D_STAGED", "GS4D_STAGED_BOX", "GS4D_SORT_RANK", "GS4D_SORT_SHAPE", "GS4D_SORT_RB")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Dev:
    """one context with the records or quads of a prepared frame uploaded; frame() is Clear -> (key loop -> sort) -> Draw"""

    def __init__(self, gs4d, p, outputs, data=None, shard=None):
        self.gs4d, self.p, self.outputs = gs4d, p, outputs
        c = self.ctx = gs4d.Context(p.w, p.h)
        c.set_clear_color(gs4d.CLEAR_COLOR)
        c.set_aux_outputs(outputs == "aux")
        c.set_id_outputs(outputs == "ids")
        if shard:
            c.set_tile_shard(*shard)
        self.db = c.buffer(p.data if data is None else data)
        if p.form == "4d":
            self.kb, self.ib = c.buffer(nbytes=4 * p.n), c.buffer(nbytes=4 * p.n)

    def frame(self):
        g, c, p = self.gs4d, self.ctx, self.p
        c.clear()
        if p.form == "4d":
            c.set_uniforms(time=0.0, min_opacity=0.0, view=p.view, proj=p.proj)
            c.keygen(self.db, 0.0, cc.CAM[0], self.kb, self.ib, p.n, key_mode=g.KEY_VIEW_Z)
            c.sort_pairs(self.kb, self.ib, p.n)
            c.set_mode(g.MODE_4D_SORTED)
            c.bind(1, self.ib)
            c.bind(2, self.db)
            c.draw_instanced(p.n)
        else:
            c.set_mode(g.MODE_3D_FULL)
            c.set_uniforms(view=p.view, proj=p.proj)
            c.draw_quads(self.db, p.n)

    def read(self):
        c = self.ctx
        out = {"rgba": c.read_pixels()}
        if self.outputs in ("aux", "ids"):
            out["aux"] = c.read_aux()
        if self.outputs == "ids":
            out["ids"] = c.read_ids()
        out["pj"] = c.debug_projected(self.p.n)
        if self.p.form == "4d":
            out["perm"] = c.read(self.ib, np.uint32, self.p.n)
        out["stats"] = c.stats()
        return out


def plane_for(p):
    """the depth-test plane of a frame: 8x8 tiles of {three thresholds in gaps of the record depths, +inf, 0}, cut by a diagonal and stripes"""
    zs = zc.pick_thresholds(p.depth[p.eproj["valid"] != 0], min_rel_gap=1e-6)
    values = [zs[0], zs[1], zs[2], INF, np.float32(0.0)]
    return zc.per_pixel_plane(p.w, p.h, values, seed=11), values


_RUNS = {}


def run(gs4d, oracle, monkeypatch, case, form, outputs, zt, env=(), shard=None, dims=None):
    """The frames of one cell, with the counters that prove its rung; memoised (the cells above compare with the cells below)."""
    key = (case, form, outputs, zt, env, shard, dims)
    if key in _RUNS:
        return _RUNS[key]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GS4D_NB", str(sc.NB))
    for k, v in env:
        monkeypatch.setenv(k, str(v))
    geo = {} if dims is None else {"w": dims[0], "h": dims[1], "long_tile": dims[2]}
    p = cc.prepared(gs4d, oracle, case, form, **geo)
    dev = Dev(gs4d, p, outputs, shard=shard)
    Z = values = None
    if zt:
        Z, values = plane_for(p)
        dev.ctx.set_depth_test(dev.ctx.depth_plane(Z))
    rung, _, k_probe = cc.CASES[case]
    plain = bool(env) and dict(env).get("GS4D_LANES") is None or shard is not None         # slabs / ordered path / shard: pictures only
    frames = []

    def shot(label, pp):
        dev.frame()
        got = dev.read()
        frames.append((label, pp, got))
        return got["stats"]

    if plain:
        shot("first", p)
        shot("again", p)
    elif dims is not None:
        s = shot("first", p)
        assert s["longest_list"] == p.L and s["tile_sort_passes"] == 0 and s["reruns"] == (1 if p.L > sc.LIST_HINT0 else 0), (s, p.L)
    elif case == "over":
        s = shot("first", p)
        assert s["reruns"] >= 1 and s["tile_sort_passes"] >= 2 and s["longest_list"] == p.L, (s, p.L)
    elif k_probe:
        lanes = dev.ctx.stats()["lanes"]
        for _ in range(2 * lanes + 8):                                 # as tests/test_gpu_staged_misses.py warms up: the capacity shrinks after 8 short draws
            dev.frame()
        dev.ctx.finish()
        s0 = dev.ctx.stats()
        assert s0["reruns"] == 0 and s0["staged_misses"] == 0 and s0["tile_sort_passes"] == 0, s0
        s1 = shot("shrunk", p)
        assert s1["longest_list"] == p.L and s1["unordered_draws"] == s0["unordered_draws"] + 1 and s1["reruns"] == 0 and s1["tile_sort_passes"] == 0, (s0, s1)
        q = cc.prepared(gs4d, oracle, case, form, probe=True)
        assert rung < q.L < sc.LIST_HINT0 and sc.crossed(p.load, q.load) == {"list"}
        dev.ctx.subdata(dev.db, q.data)
        s2 = shot("probe", q)
        # over the shrunk capacity, under 256: re-run once with a larger one (a capacity still at 256 would not re-run); nothing else missed
        assert s2["longest_list"] == q.L and s2["reruns"] == s1["reruns"] + 1 and s2["staged_misses"] == s1["staged_misses"] and s2["tile_sort_passes"] == 0, (s1, s2)
    else:
        s1 = shot("first", p)
        grow = 0 if rung == sc.LIST_HINT0 else 1
        assert s1["longest_list"] == p.L and s1["unordered_draws"] >= 1 and s1["reruns"] == grow and s1["tile_sort_passes"] == 0, (s1, p.L)
        if grow:
            s2 = shot("again", p)
            assert s2["longest_list"] == p.L and s2["unordered_draws"] == s1["unordered_draws"] + 1 and s2["reruns"] == grow and s2["tile_sort_passes"] == 0, (s1, s2)
    dev.ctx.close()
    _RUNS[key] = res = {"frames": frames, "Z": Z, "values": values, "form": form, "outputs": outputs, "env": env, "shard": shard}
    return res


_TWINS = {}


def twins(gs4d, pp, values, env, shard, monkeypatch):
    """per plane value, the frame without the test in which every hidden record has alpha 0 (ID outputs: all planes at once)"""
    key = (id(pp), env, shard)
    if key not in _TWINS:
        for k, v in env:
            monkeypatch.setenv(k, str(v))
        out = {}
        for z in values:
            dev = Dev(gs4d, pp, "ids", data=cc.hide(pp.data, pp.form, ~(pp.depth < z)), shard=shard)
            dev.frame()
            out[z] = dev.read()
            dev.ctx.close()
        _TWINS[key] = out
    return _TWINS[key]


def per_value(Z, values, make):
    """make(hidden-per-record or None) -> array or dict of arrays; merged per pixel by the plane's value"""
    if Z is None:
        return make(None)
    out = None
    for z in values:
        one = make(z)
        if out is None:
            out = {k: v.copy() for k, v in one.items()} if isinstance(one, dict) else one.copy()
        m = Z == z
        if isinstance(one, dict):
            for k in one:
                out[k][m] = one[k][m]
        else:
            out[m] = one[m]
    return out


def check(gs4d, oracle, monkeypatch, res, mine=None):
    """every frame of a cell against the CPU references (mine: the pixel rows of a shard, else all)"""
    Z, values, outputs = res["Z"], res["values"], res["outputs"]
    sel = (lambda a: a) if mine is None else (lambda a: a[mine])
    for label, pp, got in res["frames"]:
        w, h = pp.w, pp.h
        if pp.form == "4d":
            assert np.array_equal(got["perm"], pp.order), label
        valid = pp.eproj["valid"] != 0
        assert np.array_equal(got["pj"][:, 14] != 0, valid)

        def hidden_proj(proj, z):
            q = proj.copy()
            if z is not None:
                q["alpha"][~(pp.depth < z)] = 0.0
            return q

        want = per_value(Z, values, lambda z: oracle.composite(hidden_proj(pp.eproj, z), pp.order, pp.frag_mode, w, h, oracle.clear_image(w, h)))
        err = float(np.abs(sel(got["rgba"]).astype(np.float64) - sel(want)).max())
        print(f"{label}: colour linf {err:.3g}")
        assert err <= TOL, (label, err)
        assert np.abs(want - oracle.CLEAR).max() > 0.05
        if outputs in ("aux", "ids") or Z is not None:
            d = got["pj"][:, 15].copy()
            np.testing.assert_allclose(d[valid], pp.depth[valid], rtol=1e-6)
        if outputs in ("aux", "ids"):
            # depth and opacity by colour substitution; the weights do not depend on the colour: quads composite in the 4D fragment mode
            def aux_ref(z):
                q, s = substituted(hidden_proj(pp.eproj, z), d)
                e = oracle.composite(q, pp.order, oracle.MODE_4D, w, h, np.zeros((h, w, 4), np.float32))
                return np.stack([s * e[..., 0].astype(np.float64), e[..., 1].astype(np.float64)], -1)
            e = per_value(Z, values, aux_ref)
            s = float(d.max())
            assert np.abs(sel(got["aux"][..., 0]) - sel(e[..., 0])).max() <= 1e-4 * s, label
            assert np.abs(sel(got["aux"][..., 1]) - sel(e[..., 1])).max() <= 1e-4, label
            assert got["aux"][..., 1].max() > 0.3
        if outputs == "ids":
            dproj = id_cases.from_device(got["pj"])
            r = per_value(Z, values, lambda z: id_cases.restate(hidden_proj(dproj, z), pp.order, w, h, premult=(pp.form == "quads")))
            if mine is None:
                check_parity(got["ids"], r)
            else:
                check_parity([x[mine] for x in got["ids"]], {k: v[mine] for k, v in r.items()})
        if Z is not None:
            tw = twins(gs4d, pp, values, res["env"], res["shard"], monkeypatch)
            for k in ("rgba", "aux", "ids"):
                if k in got:
                    planes = (lambda x: x) if k == "ids" else (lambda x: (x,))
                    for j, a in enumerate(planes(got[k])):
                        t = per_value(Z, values, lambda z: planes(tw[z][k])[j])
                        assert np.array_equal(bits(a), bits(t)), (label, k, j)


def same_planes(a, b, keys, where=None):
    sel = (lambda x: x) if where is None else (lambda x: x[where])
    for (la, _, ga), (lb, _, gb) in zip(a["frames"], b["frames"]):
        for k in keys:
            xs, ys = (ga[k], gb[k]) if k == "ids" else ((ga[k],), (gb[k],))
            for x, y in zip(xs, ys):
                assert np.array_equal(bits(sel(x)), bits(sel(y))), (la, lb, k)


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zt", [False, True], ids=["ztest_off", "ztest_on"])
@pytest.mark.parametrize("outputs", OUTPUTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(cc.CASES))
def test_cell(gs4d, oracle, monkeypatch, case, form, outputs, zt):
    res = run(gs4d, oracle, monkeypatch, case, form, outputs, zt)
    check(gs4d, oracle, monkeypatch, res)
    if outputs in ("aux", "ids"):
        same_planes(res, run(gs4d, oracle, monkeypatch, case, form, "colour", zt), ["rgba"])
    if outputs == "ids":
        same_planes(res, run(gs4d, oracle, monkeypatch, case, form, "aux", zt), ["rgba", "aux"])
        if zt and case not in ("c128", "c1024"):                       # (the sweeps below compare with those two; the others are done with)
            for k in [k for k in _RUNS if k[:2] == (case, form)]:
                del _RUNS[k]
            _TWINS.clear()


# ---- sweeps at the 1024 rung's image ------------------------------------------------------------------------------------------------------
PLANES = {"colour": ["rgba"], "aux": ["rgba", "aux"], "ids": ["rgba", "aux", "ids"]}


@pytest.mark.parametrize("zt", [False, True], ids=["ztest_off", "ztest_on"])
@pytest.mark.parametrize("outputs", OUTPUTS)
@pytest.mark.parametrize("slabs", [4, 32])
def test_depth_slabs(gs4d, oracle, monkeypatch, slabs, outputs, zt):
    """GS4D_SLABS: sub-lists by key range, far slab first, early exit — same picture as the cell without slabs, bit for bit (as
    tests/test_gpu_paths.py::test_depth_slabs claims against the ordered path)"""
    res = run(gs4d, oracle, monkeypatch, "c1024", "4d", outputs, zt, env=(("GS4D_SLABS", slabs),))
    for _, _, got in res["frames"]:
        assert got["stats"]["unordered_draws"] >= 1 and got["stats"]["tile_sort_passes"] == 0, got["stats"]
    check(gs4d, oracle, monkeypatch, res)
    same_planes(res, run(gs4d, oracle, monkeypatch, "c1024", "4d", outputs, zt), PLANES[outputs])


@pytest.mark.parametrize("zt", [False, True], ids=["ztest_off", "ztest_on"])
@pytest.mark.parametrize("outputs", OUTPUTS)
@pytest.mark.parametrize("form", FORMS)
def test_ordered_path_gives_the_same_bits(gs4d, oracle, monkeypatch, form, outputs, zt):
    res = run(gs4d, oracle, monkeypatch, "c1024", form, outputs, zt, env=(("GS4D_DRAW_PATH", "ordered"),))
    for _, _, got in res["frames"]:
        assert got["stats"]["unordered_draws"] == 0 and got["stats"]["tile_sort_passes"] >= 2, got["stats"]
    check(gs4d, oracle, monkeypatch, res)
    same_planes(res, run(gs4d, oracle, monkeypatch, "c1024", form, outputs, zt), PLANES[outputs])


@pytest.mark.parametrize("zt", [False, True], ids=["ztest_off", "ztest_on"])
def test_tile_shard(gs4d, oracle, monkeypatch, zt):
    """set_tile_shard(1, 2): the odd tile rows only — the long tile's row among them"""
    assert cc.LONG[1] % 2 == 1 and cc.SHORT[65][1] % 2 == 1
    for rank in (1,):
        res = run(gs4d, oracle, monkeypatch, "c1024", "4d", "ids", zt, shard=(rank, 2))
        mine = (np.arange(cc.H) // 8) % 2 == rank
        check(gs4d, oracle, monkeypatch, res, mine=mine)
        same_planes(res, run(gs4d, oracle, monkeypatch, "c1024", "4d", "ids", zt), ["rgba", "aux", "ids"], where=mine)
        for _, _, got in res["frames"]:
            assert not got["aux"][~mine].any() and (got["ids"][0][~mine] == id_cases.ID_NONE).all()
            assert got["stats"]["longest_list"] == cc.CASES["c1024"][1] and got["stats"]["tile_sort_passes"] == 0, got["stats"]


@pytest.mark.parametrize("case", ["c128", "c1024"])
def test_one_lane(gs4d, oracle, monkeypatch, case):
    res = run(gs4d, oracle, monkeypatch, case, "4d", "ids", True, env=(("GS4D_LANES", 1),))
    check(gs4d, oracle, monkeypatch, res)
    same_planes(res, run(gs4d, oracle, monkeypatch, case, "4d", "ids", True), ["rgba", "aux", "ids"])


@pytest.mark.parametrize("form", FORMS)
def test_long_tile_clipped_in_the_corner(gs4d, oracle, monkeypatch, form):
    """636 x 356: the last tile column and row are 4 pixels wide; the long tile is the corner one"""
    w, h = 636, 356
    res = run(gs4d, oracle, monkeypatch, "c1024", form, "ids", False, dims=(w, h, (79, 44)))
    p = res["frames"][0][1]
    assert p.load.tiles[44 * 80 + 79] == p.L > sc.LIST_HINT0, p.L
    check(gs4d, oracle, monkeypatch, res)

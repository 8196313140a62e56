"""GPU: hostile records (tests/hostile_cases.py) are data, not device faults.

Every case at 256 x 192, keys by gs4d_keygen's kernel or by the draw, tile lists chosen by the library or instance-ordered, the compact record
shadow or the full one; representatives at 1 and 8 frame lanes and with aux and ID outputs.  Against the CPU checker (whose own side of the
contract tests/test_hostile_host.py pins): no call reports an error, keys bit-equal (NaN where NaN), the permutation is the stable sort of
the GPU's own key bit patterns, the image is finite and within test_gpu_render's TOL of the checker's — with and without the dead records.
"""
import functools

import numpy as np
import pytest

import hostile_cases as hc
import scenes
from test_gpu_render import linf, TOL
from test_hostile_host import checker_frame, same_keys

pytestmark = pytest.mark.gpu

SETTINGS = [(fuse, path, full) for fuse in (1, 0) for path in ("auto", "ordered") for full in (0, 1)]
REPRESENTATIVES = ["utm_slab_20000", "several_at_once", "whole_screen_1e3", "nan_inf_colour"]      # one per family
_CTX = {}


def _context(gs4d, monkeypatch, fuse, path, full, lanes=None):
    """One context per setting for the whole module; dropped when a test on it fails."""
    key = (fuse, path, full, lanes)
    for k in ("GS4D_DRAW_PATH", "GS4D_SOA_FULL", "GS4D_LANES", "GS4D_FUSE_KEYGEN", "GS4D_SORT_RANK", "GS4D_SORT_SHAPE", "GS4D_SORT_RB"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GS4D_FUSE_KEYGEN", str(fuse))          # (set for every test, not only the first: GS4D_SOA_FULL is read when records are repacked)
    if path == "ordered":
        monkeypatch.setenv("GS4D_DRAW_PATH", "ordered")
    if full:
        monkeypatch.setenv("GS4D_SOA_FULL", "1")
    if lanes is not None:
        monkeypatch.setenv("GS4D_LANES", str(lanes))
    if key not in _CTX:
        _CTX[key] = gs4d.Context(hc.W, hc.H)
    return key, _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx in _CTX.values():
        ctx.close()
    _CTX.clear()


@functools.lru_cache(maxsize=None)
def _expected(name):
    import oracle_lib
    c = hc.get(name)
    ekeys, eperm, _, eimg = checker_frame(oracle_lib, c.rec, c)
    rec2, remap = hc.without_dead(c)
    order2 = remap[eperm][~c.dead[eperm]].astype(np.uint32)
    _, _, _, eimg2 = checker_frame(oracle_lib, rec2, c, order=order2)
    return ekeys, eperm, eimg, eimg2


def gpu_frame(ctx, gs4d, c, outputs=False):
    """Scenes.h:312-339 through the C ABI, every step once; any error a call reports raises."""
    n = c.n
    db, kb, ib = ctx.buffer(c.rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
    try:
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_id_outputs(outputs)
        ctx.clear()
        ctx.set_uniforms(time=c.t, min_opacity=c.min_opacity, view=c.view, proj=c.proj)
        ctx.keygen(db, c.t, c.cam[0], kb, ib, n)
        ctx.sort_pairs(kb, ib, n)
        ctx.set_mode(gs4d.MODE_4D_SORTED)
        ctx.bind(1, ib)
        ctx.bind(2, db)
        ctx.draw_instanced(n)
        ctx.finish()
        out = {"img": ctx.read_pixels(), "sorted_keys": ctx.read(kb, np.uint32, n), "perm": ctx.read(ib, np.uint32, n), "stats": ctx.stats()}
        if outputs:
            out["aux"], out["ids"] = ctx.read_aux(), ctx.read_ids()
    finally:
        for b in (db, kb, ib):
            ctx.delete(b)
    return out


def check_frame(c, got):
    ekeys, eperm, eimg, eimg2 = _expected(c.name)
    n = c.n
    perm, sk = got["perm"], got["sorted_keys"]
    assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32)), "not a permutation"
    bits = np.empty(n, np.uint32)
    bits[perm] = sk                                              # the key the GPU gave each record
    assert same_keys(bits.view(np.float32), ekeys)
    assert np.array_equal(perm, np.argsort(bits, kind="stable").astype(np.uint32)), "not the stable sort of the GPU's own keys"
    if not np.isnan(ekeys).any():
        assert not c.nan_key
        assert np.array_equal(perm, eperm)
    img = got["img"]
    assert np.isfinite(img).all()
    err, err2 = linf(img, eimg), linf(img, eimg2)
    print(f"{c.name}: Linf {err:.3e} (without the dead records {err2:.3e})")
    assert err <= TOL and err2 <= TOL
    if c.whole_screen:
        clear = np.array(hc._gs4d().CLEAR_COLOR, np.float32)
        assert float(np.abs(img - clear).max(axis=2).min()) > 0.05
    if "ids" in got:
        rec_id, draw_id, weight = got["ids"]
        assert np.isfinite(got["aux"]).all() and np.isfinite(weight).all()
        named = rec_id[rec_id != 0xFFFFFFFF]
        assert named.size and (named < n).all()
        assert not c.dead[named].any(), "a pixel names a dead record"


def _run(gs4d, monkeypatch, c, fuse, path, full, lanes=None, outputs=False):
    key, ctx = _context(gs4d, monkeypatch, fuse, path, full, lanes)
    try:
        got = gpu_frame(ctx, gs4d, c, outputs)
        check_frame(c, got)
    except BaseException:
        _CTX.pop(key).close()
        raise
    return got


@pytest.mark.parametrize("fuse,path,full", SETTINGS)
@pytest.mark.parametrize("name", hc.names())
def test_hostile_case(gs4d, monkeypatch, name, fuse, path, full):
    _run(gs4d, monkeypatch, hc.get(name), fuse, path, full)


@pytest.mark.parametrize("lanes", [1, 8])
@pytest.mark.parametrize("name", REPRESENTATIVES)
def test_hostile_case_by_lanes(gs4d, monkeypatch, name, lanes):
    c = hc.get(name)
    for _ in range(2 if lanes == 1 else 9):                     # every lane draws the frame once, the first a second time
        got = _run(gs4d, monkeypatch, c, 1, "auto", 0, lanes=lanes)
    assert got["stats"]["lanes"] == lanes


@pytest.mark.parametrize("path", ["auto", "ordered"])
@pytest.mark.parametrize("name", REPRESENTATIVES)
def test_hostile_case_with_aux_and_id_outputs(gs4d, monkeypatch, name, path):
    _run(gs4d, monkeypatch, hc.get(name), 1, path, 0, outputs=True)
    _run(gs4d, monkeypatch, hc.get(name), 1, path, 0, outputs=False)      # and the context goes back to plain frames


def test_benign_shape_keeps_its_three_pass_sort(gs4d, monkeypatch):
    """bench.py's workload — 10^6 static splats in the cube, seen from outside: the proven span stays within 24 bits, three 8-bit passes."""
    for k in ("GS4D_DRAW_PATH", "GS4D_SOA_FULL", "GS4D_LANES", "GS4D_FUSE_KEYGEN", "GS4D_SORT_RANK", "GS4D_SORT_SHAPE", "GS4D_SORT_RB"):
        monkeypatch.delenv(k, raising=False)
    n, W, H = 1000000, 640, 360
    pos, q, scale, rgba = scenes.cube_params(n)
    rec = gs4d.build_records_3d(pos, q, scale, rgba)
    cam = scenes.CAM_CUBE
    ctx = gs4d.Context(W, H)
    db, kb, ib = ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.clear()
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=gs4d.look_at(cam[0], cam[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
    ctx.keygen(db, 0.0, cam[0], kb, ib, n)
    ctx.sort_pairs(kb, ib, n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.draw_instanced(n)
    ctx.finish()
    st = ctx.stats()
    sk, perm = ctx.read(kb, np.uint32, n), ctx.read(ib, np.uint32, n)
    ctx.close()
    assert st["depth_sort_passes"] == 3, st
    d = rec[:, 0:3] - np.array(cam[0], np.float32)
    keys = (np.float32(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])).view(np.uint32)
    assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32)) and np.array_equal(sk, keys[perm])

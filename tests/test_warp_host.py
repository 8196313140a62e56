"""CPU: the host side of gs4d_warp_records (include/gs4d.h) — gs4d_host_warp_records against the header's text restated in numpy float32
(tests/warp_cases.py), the consequences the header states, copied records, lattice() and lattice_points(), the per-record text that the kernel and the
host function share (csrc/warp_record.h) compiled stand-alone with g++ against the host function, and the ABI."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import transform_cases as tc
import warp_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
u32 = np.uint32
IDENTITY = tc.transforms()["identity"]


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", wc.SETS)
def test_the_host_function_is_the_headers_text(gs4d, which):
    """over the calls of the GPU record test; by_the_text alone says how many records of them are warped, copied and clamped"""
    warped = copied = clamped = 0
    for what, rec, nodes, lat in wc.calls(gs4d, which):
        got = gs4d.warp_records_host(rec, nodes, lat)
        assert got.shape == rec.shape and got.dtype == f32
        want, w, c, k = wc.by_the_text(rec, nodes, lat)
        wc.assert_records(got, want, rec, w, what)
        warped, copied, clamped = warped + int(w.sum()), copied + int(c.sum()), clamped + int(k.sum())
    assert warped > 1000 and copied > 1000 and clamped > 1000, (warped, copied, clamped)


def test_the_cases_hold_what_they_promise(gs4d):
    rec = tc.records(gs4d, "4d_vel", 769)
    lat = wc.lattice_for(gs4d, rec, (3, 2, 4, 5))
    inside = np.ones(769, bool)
    for a in range(4):
        u = wc.u_of(rec[:, a], lat, a)
        inside &= (u >= 0) & (u <= lat.dims[a] - 1)
    assert 0.3 < inside.mean() < 0.7, "the box does not take roughly half the centres"
    sp = wc.special_centres(gs4d, lat)
    for a in range(4):
        u = wc.u_of(sp[4 * a:4 * a + 4, a], lat, a)
        assert u[0] == 0 and u[1] < 0 and u[2] == lat.dims[a] - 1 and u[3] > lat.dims[a] - 1, (a, u)      # on a face, in front, u == top, behind
    assert sp.shape[0] > 16                                                          # and centres on nodes
    hostile = wc.nodes_for(gs4d, lat, "hostile", 3)
    assert np.isnan(hostile).any() and np.isposinf(hostile).any() and np.isneginf(hostile).any() and (hostile == f32(1e30)).any()
    assert (wc.bits(hostile) == 0x80000000).any()
    assert wc.LDS_NODES in (0, wc.EDGE) and (wc.EDGE, 1, 1, 1) in wc.DIMS and (wc.EDGE + 1, 1, 1, 1) in wc.DIMS
    assert not np.isfinite(wc.records_for(gs4d, "hostile", 769, lat)[:, :4]).all()      # NaN and Inf centres come by


def test_copied_records_are_byte_equal(gs4d):
    n = 257
    rec = tc.records(gs4d, "hostile", n)                                              # NaN payloads and signed zeros must survive a copy
    assert np.isnan(rec).any()
    lat = gs4d.lattice((1e9, 1e9, 1e9, 1e9), (2e9, 2e9, 2e9, 2e9), (2, 2, 2, 2))      # nobody is inside
    nodes = wc.nodes_for(gs4d, lat, "hostile")
    assert np.array_equal(gs4d.warp_records_host(rec, nodes, lat).view(np.uint8), rec.view(np.uint8))
    nan_box = gs4d.lattice((np.nan,) * 4, (1.0,) * 4, (2, 2, 2, 2), "xyzt")          # a NaN u is never inside, with or without the clamp
    assert np.array_equal(gs4d.warp_records_host(rec, nodes, nan_box).view(np.uint8), rec.view(np.uint8))


# ---- the consequences the header states -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", wc.SETS)
def test_a_zero_lattice_leaves_sigma_with_the_bits_of_the_identity_row(gs4d, which):
    rec = tc.records(gs4d, which, 769)
    want = gs4d.transform_records_host(rec, IDENTITY)
    for dims in wc.DIMS:
        lat = wc.lattice_for(gs4d, rec, dims, 0xF)
        got = gs4d.warp_records_host(rec, np.zeros((wc.count_of(dims), 4), f32), lat)
        warped = wc.by_the_text(rec, np.zeros((wc.count_of(dims), 4), f32), lat)[1]
        assert warped.sum() > 700
        assert np.array_equal(got.view(u32)[warped, 8:], want.view(u32)[warped, 8:]), f"{which}, dims {dims}"      # the same code on the same machine
        with np.errstate(all="ignore"):
            assert wc.same_bits(got[warped, :8], np.concatenate([rec[:, :4] + f32(0.0), rec[:, 4:8]], 1)[warped]).all()


@pytest.mark.parametrize("which", ("3d", "4d_vel", "4d_2q"))
def test_two_equal_nodes_on_an_axis_are_one_node(gs4d, which):
    rec = tc.records(gs4d, which, 769)
    assert np.isfinite(rec).all()
    for what, nodes, lat, nodes2, lat2 in wc.equal_node_pairs(gs4d, rec):
        want, got = gs4d.warp_records_host(rec, nodes, lat), gs4d.warp_records_host(rec, nodes2, lat2)
        assert wc.by_the_text(rec, nodes, lat)[1].sum() > 100
        assert np.isfinite(want).all() and np.array_equal(got.view(u32), want.view(u32)), f"{which}, {what}"


def test_an_exact_case(gs4d):
    """lo = 0, inv = 1, node displacements that are an integer-valued affine function of the node index, centres and covariances of small dyadic
    values: every operation of the text is exact, so G is the affine function's matrix, Sigma' has the bits of transform_records_host with
    L = I + G, and the means are exact"""
    rng = np.random.default_rng(0x5745)
    dims = (4, 3, 5, 3)
    lat = gs4d.lattice((0, 0, 0, 0), [d - 1 for d in dims], dims)
    assert list(lat.inv) == [1.0] * 4
    M, c = rng.integers(-2, 3, (4, 4)).astype(np.float64), rng.integers(-3, 4, 4).astype(np.float64)
    idx = gs4d.lattice_points(lat).astype(np.float64)
    nodes = (idx @ M.T + c).astype(f32)
    n = 600
    rec = np.zeros((n, 24), f32)
    rec[:, :4] = rng.integers(0, 8 * (np.array(dims) - 1) + 1, (n, 4)) / 8.0          # multiples of 1/8 from face to face, u == top included
    rec[:, 4:8] = rng.uniform(0, 1, (n, 4))
    rec[:, 8:] = rng.integers(-8, 9, (n, 16)) / 4.0
    got = gs4d.warp_records_host(rec, nodes, lat)
    L = np.eye(4) + M
    want = gs4d.transform_records_host(rec, tc.row(L, c))
    assert np.array_equal(got.view(u32)[:, 8:], want.view(u32)[:, 8:])
    mean = rec[:, :4].astype(np.float64) @ L.T + c
    assert np.array_equal(got[:, :4].astype(np.float64), mean) and np.array_equal(got.view(u32)[:, 4:8], rec.view(u32)[:, 4:8])
    text, warped = wc.by_the_text(rec, nodes, lat)[:2]
    assert warped.all() and np.array_equal(text.view(u32), got.view(u32))
    assert (rec[:, 0] == dims[0] - 1).any()


def test_a_single_node_is_a_translation(gs4d):
    d = np.array([1.5, -2.0, 0.25, 3.0], f32)
    lat = gs4d.lattice((5, 5, 5, 5), (5, 5, 5, 5), (1, 1, 1, 1), "xyzt")
    for which in wc.SETS:
        rec = tc.records(gs4d, which, 300)
        got = gs4d.warp_records_host(rec, d, lat)                                       # no axis takes part: every record is inside, a NaN centre too
        with np.errstate(all="ignore"):
            assert wc.same_bits(got[:, :4], rec[:, :4] + d).all(), which
        assert np.array_equal(got.view(u32)[:, 4:8], rec.view(u32)[:, 4:8])
        assert np.array_equal(got.view(u32)[:, 8:], gs4d.transform_records_host(rec, IDENTITY).view(u32)[:, 8:]), which


# ---- lattice() and lattice_points() ---------------------------------------------------------------------------------------------------------------
def test_lattice_and_lattice_points_round_trip(gs4d):
    lo, hi, dims = (-2.0, 1.0, 0.5, 10.0), (6.0, 2.0, 0.5, 14.0), (5, 3, 1, 9)
    lat = gs4d.lattice(lo, hi, dims, "tx")
    assert ctypes.sizeof(lat) == 64 and list(lat.dims) == list(dims) and lat.clamp == 9 and list(lat.pad) == [0, 0, 0]
    assert list(lat.lo) == list(lo) and list(lat.inv) == [0.5, 2.0, 0.0, 2.0]
    pts = gs4d.lattice_points(lat)
    assert pts.shape == (9, 1, 3, 5, 4) and pts.dtype == f32
    assert pts[0, 0, 0, 0].tolist() == list(lo) and pts[8, 0, 2, 4].tolist() == list(hi)
    assert pts[3, 0, 1, 2].tolist() == [2.0, 1.5, 0.5, 11.5]                          # [t, z, y, x]: the order of the nodes in memory
    # a field is f(points) - points: a lattice of an affine f warps a centre to f(centre)
    f = lambda p: p * np.array([2.0, 1.0, 1.0, 0.5], f32) + np.array([1.0, 0.0, -3.0, 2.0], f32)
    rec = np.zeros((1, 24), f32)
    rec[0, :4], rec[0, 8::5] = (1.0, 1.25, 7.0, 13.0), 1.0
    out = gs4d.warp_records_host(rec, f(pts) - pts, lat)
    assert out[0, :4].tolist() == f(rec[0, :4]).tolist() and out[0, 8::5].tolist() == [4.0, 1.0, 1.0, 0.25]
    assert gs4d.lattice(lo, hi, dims).clamp == 0 and gs4d.lattice(lo, hi, dims, "xyzt").clamp == 15
    with pytest.raises(ValueError):
        gs4d.lattice(lo, hi, dims, "w")
    with pytest.raises(ValueError):
        gs4d.lattice(lo, hi, (2, 2, 2))
    with pytest.raises(ValueError):
        gs4d.warp_records_host(rec, np.zeros((7, 4), f32), lat)                         # not the lattice's node count


def test_lattices_the_device_would_refuse_write_nothing(gs4d):
    rec = tc.records(gs4d, "3d", 4)
    for what, lat in wc.refused_lattices(gs4d).items():
        assert not gs4d.warp_records_host(rec, np.ones((1, 4), f32), lat).any(), what
    out = np.zeros_like(rec)
    gs4d._lib.gs4d_host_warp_records(4, rec.ctypes.data, np.ones(4, f32).ctypes.data, None, out.ctypes.data)
    assert not out.any()


# ---- the kernel's text on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=("plain", "asan_ubsan"))
def check_program(request, tmp_path_factory):
    """the stand-alone program, built plainly and as an executable instrumented with AddressSanitizer + UndefinedBehaviorSanitizer + the
    float-to-integer conversion check (nothing is preloaded)"""
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("warp_record_check") / "warp_record_check"
    san = ["-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *san, os.path.join(ROOT, "tests", "warp_record_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return str(exe)


def hostile_boxes(gs4d, rec, dims, clamp):
    """the lattice over the set, and the same with lo and inv that are no numbers to lay a lattice with: the text must still read nodes only"""
    yield "the box of the set", wc.lattice_for(gs4d, rec, dims, clamp)
    for name, lo, inv in (("inv inf", 0.0, np.inf), ("inv -inf", 0.0, -np.inf), ("inv nan", 0.0, np.nan), ("lo nan", np.nan, 1.0), ("lo -inf", -np.inf, 1.0),
                          ("inv 1e38", 1.0, 1e38), ("inv -1e-45", 0.0, -1e-45), ("inv 0", 3.0, 0.0), ("inv -0", 3.0, -0.0)):
        lat = wc.lattice_for(gs4d, rec, dims, clamp)
        lat.lo[:], lat.inv[:] = [lo] * 4, [inv] * 4
        yield name, lat


def test_the_kernels_text_gives_the_host_functions_bits_on_the_cpu(gs4d, check_program, tmp_path):
    """the hostile set and the clean ones through hostile lattices under every clamp mask: the instrumented build ends a run that reads outside the
    node array or converts a NaN, a negative or a too-large value"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    paths = [tmp_path / f for f in ("records.bin", "nodes.bin", "lattice.bin", "out.bin")]
    runs = 0
    for which in wc.SETS:
        n = 257 if which != "hostile" else tc.hostile_block().shape[0] + 40
        base = tc.records(gs4d, which, n)
        for dims in wc.DIMS if which == "hostile" else ((3, 2, 4, 5), (1, 3, 1, 2)):
            for cname, clamp in wc.CLAMPS.items():
                proper = wc.lattice_for(gs4d, base, dims, clamp)
                rec = wc.records_for(gs4d, which, n, proper)
                every_box = which == "hostile" and dims in ((2, 2, 2, 2), (3, 2, 4, 5), (1, 3, 1, 2), (wc.EDGE + 1, 1, 1, 1))
                for bname, lat in hostile_boxes(gs4d, base, dims, clamp) if every_box else (("the box of the set", proper),):
                    what = f"{which}, dims {dims}, clamp {cname}, {bname}"
                    nodes = wc.nodes_for(gs4d, proper, "hostile", runs)
                    rec.tofile(paths[0])
                    nodes.tofile(paths[1])
                    open(paths[2], "wb").write(bytes(lat))
                    r = subprocess.run([check_program, str(n), *map(str, paths)], capture_output=True, text=True, timeout=120, env=env)
                    assert r.returncode == 0, what + "\n" + r.stderr[-3000:]
                    got = np.fromfile(paths[3], f32).reshape(n, 24)
                    want, warped = gs4d.warp_records_host(rec, nodes, lat), wc.by_the_text(rec, nodes, lat)[1]
                    # the NaN rule of gs4d.h: the library's host code and this program come from two compilers
                    wc.assert_records(got, want, rec, warped, what)
                    runs += 1
    assert runs > 100


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_the_constants_and_the_abi(gs4d):
    assert ctypes.sizeof(gs4d.Lattice) == 64
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert "GS4D_API int gs4d_warp_records(gs4d_ctx* ctx, gs4d_buf src, size_t n, gs4d_buf nodes, const gs4d_lattice* lat, gs4d_buf dst, size_t dst_first);" in hdr
    assert "GS4D_API void gs4d_host_warp_records(size_t n, const float* records24, const float* nodes4, const gs4d_lattice* lat, float* out24);" in hdr
    assert "} gs4d_lattice;         /* 64 bytes */" in hdr
    assert f"constexpr uint32_t WARP_TILE = {wc.TILE};" in wc.INTERNAL and wc.TILE == 256
    assert f"constexpr uint32_t WARP_LDS_NODES = {wc.LDS_NODES};" in wc.INTERNAL      # the threshold the GPU tests are laid around
    assert {"gs4d_warp_records", "gs4d_host_warp_records"} <= set(gs4d.EXPORTS)
    lat = gs4d.lattice((0,) * 4, (1,) * 4, (1, 1, 1, 1))
    assert gs4d._lib.gs4d_warp_records(None, 1, 1, 2, ctypes.byref(lat), 3, 0) == -1   # GS4D_E_INVALID: no context

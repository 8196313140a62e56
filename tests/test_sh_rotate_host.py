"""CPU: the host side of gs4d_rotate_sh (include/gs4d.h) — gs4d_host_sh_rotation and gs4d_host_rotate_sh against an independent float64
definition (tests/sh_rotate_cases.py: least squares over the basis of gs4d_shade_sh, nothing of the header's recurrences), the form and row rules the
header states, the per-row text that the kernel and the host function share (csrc/sh_rotate_record.h) and the call's checks
(csrc/sh_rotate_operands.h) compiled stand-alone with g++, and the ABI."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_cases as pc
import sh_rotate_cases as rc
import shade_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
f64 = np.float64
u32 = np.uint32
U = 2.0 ** -24                                                # the unit roundoff of float32


def rotation_of(d):
    """R from D_1 = P R P^T"""
    return rc.PERM.T @ np.asarray(d[:9], f64).reshape(3, 3) @ rc.PERM


def blend_rows(gs4d):
    """(xf [4, 20], bind_rows [n, 8]): rows blended from two, three and four rotations about one axis, at most 0.4 rad apart — well-conditioned
    skinning blends — under normalised and unnormalised weights"""
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    xf = np.stack([gs4d.affine4(np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * axis]).astype(f32), translate=(a, 0.0, 1.0)) for a in (0.9, 1.0, 1.15, 1.3)])
    j = np.array([[0, 1, rc.ID_NONE, rc.ID_NONE], [3, rc.ID_NONE, 1, 2], [0, 1, 2, 3], [2, 9, 0, rc.ID_NONE], [1, 1, 1, 1], [3, 2, 1, 0]], u32)
    w = np.array([[0.5, 0.5, 7, 7], [0.2, np.nan, 0.3, 0.5], [0.25, 0.25, 0.25, 0.25], [1.5, 3, 0.75, np.inf], [0.1, 0.2, 0.3, 0.4], [0.7, 0.1, 0.1, 0.1]], f32)
    return xf.astype(f32), gs4d.bind_rows(j, w)


# ---- the frame ----------------------------------------------------------------------------------------------------------------------------------
def test_the_frame_is_orthonormal_and_a_similaritys_rotation(gs4d):
    """Each e_c is a vector times one rounded reciprocal of a rounded root of a three-term rounded sum: its length is 1 within 4 U.  A dot product of
    two such vectors carries three rounded products, two rounded sums and what the two projections left, each a few U: 16 U bounds every entry of
    R^T R - I, and the same count bounds the distance from the rotation of a similarity, whose entries gs4d_host_affine4 rounded once more."""
    worst = far = 0.0
    for name, l in rc.maps(gs4d).items():
        ok, d = gs4d.sh_rotation(l)
        assert ok and d[83] == 0, name
        R = rotation_of(d)
        worst = max(worst, float(np.abs(R.T @ R - np.eye(3)).max()))
        far = max(far, float(np.abs(R - rc.frame64(l)).max()))
        if name.startswith(("rotation", "similarity")):
            k = int(name.split("_")[1]) if name.startswith("rotation") else 10 + [f"{s:g}" for s in rc.SCALES].index(name.split("_")[1])
            far = max(far, float(np.abs(R - rc.quat_matrix(rc.quaternion(k))).max()))
    print(f"R^T R - I: {worst:.3g}; R - the rotation: {far:.3g}")
    assert worst <= 16 * U and far <= 16 * U
    mirror = rotation_of(gs4d.sh_rotation(rc.maps(gs4d)["mirror"])[1])
    assert np.linalg.det(mirror) < -0.99, "a mirror must stay a mirror"
    # velocity, time terms and the offset take no part
    assert np.array_equal(gs4d.sh_rotation(rc.maps(gs4d)["moving"])[1].view(u32), gs4d.sh_rotation(rc.maps(gs4d)["rotation_0"])[1].view(u32))


def test_maps_that_do_not_rotate(gs4d):
    decided = 0
    for name, (l, rotates) in rc.hostile_maps(gs4d).items():
        ok, d = gs4d.sh_rotation(l)
        if rotates is not None:
            assert ok == rotates, name
            decided += 1
        assert ok or not d.any(), f"{name}: d was written"
    assert decided >= 8


# ---- the defining identity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", (1, 2, 3))
def test_the_defining_identity(gs4d, degree):
    worst = 0.0
    n = 120
    for k, (name, l) in enumerate(rc.maps(gs4d).items()):
        t = rc.table(n, degree, rc.strides(degree)[k % 3], seed=0x5350 + k)
        out = gs4d.rotate_sh_host(t, l.reshape(1, 20), degree)
        worst = max(worst, rc.identity_ratio(t, out, rc.frame64(l), degree, seed=0x5353 + 16 * k + degree))
    # blended maps: the frame their columns span
    xf, rows = blend_rows(gs4d)
    a, mapped = rc.chosen_maps(xf, rows.view(np.uint8).reshape(-1), rc.BLEND4, 32, rows.shape[0])
    assert mapped.all()
    for i in range(rows.shape[0]):
        t = rc.table(n, degree, sc.row_bytes(degree), seed=0x5360 + i)
        out = gs4d.rotate_sh_host(t, xf, degree, np.repeat(rows[i:i + 1], n, 0))
        assert not np.array_equal(out, t)
        worst = max(worst, rc.identity_ratio(t, out, rc.frame64(a[i]), degree, seed=0x5370 + 16 * i + degree))
    print(f"degree {degree}: the identity holds to {worst:.3g} sum |c_k|")
    assert rc.IDENTITY_BAR <= 1e-5
    assert worst <= rc.IDENTITY_BAR


def test_the_matrices_are_those_of_the_least_squares_definition(gs4d):
    worst = 0.0
    for name, l in rc.maps(gs4d).items():
        ok, d = gs4d.sh_rotation(l)
        assert ok
        want = rc.d84(rc.band_matrices64(rc.frame64(l)))
        worst = max(worst, float(np.abs(d.astype(f64) - want).max()))
    print(f"d[84] is the least-squares D to {worst:.3g}")
    assert rc.MATRIX_BAR <= 1e-5
    assert worst <= rc.MATRIX_BAR


def test_a_transposed_or_mis_signed_matrix_would_show(gs4d):
    """the identity check has teeth: the library's own d[84] applied as it is passes the bar; transposed, or with the sign of one column turned, it
    misses the bar by orders of magnitude"""
    l = rc.maps(gs4d)["rotation_1"]
    ok, d = gs4d.sh_rotation(l)
    assert ok
    R = rc.frame64(l)
    D = np.zeros((16, 16))
    D[0, 0] = 1.0
    for L in (1, 2, 3):
        w = 2 * L + 1
        D[L * L:(L + 1) ** 2, L * L:(L + 1) ** 2] = d[rc.AT[L]:rc.AT[L] + w * w].astype(f64).reshape(w, w)
    c = rc.table(50, 3, 192)[:, :48].astype(f64).reshape(50, 16, 3)
    for wrong in (D.T, D * np.where(np.arange(16) == 5, -1.0, 1.0)[None, :]):
        out = np.einsum("ij,njc->nic", wrong, c).reshape(50, 48)
        assert rc.identity_ratio(c.reshape(50, 48), out, R, 3, seed=1) > 1000 * rc.IDENTITY_BAR
    assert rc.identity_ratio(c.reshape(50, 48), np.einsum("ij,njc->nic", D, c).reshape(50, 48), R, 3, seed=1) <= rc.IDENTITY_BAR


# ---- forms and rows -----------------------------------------------------------------------------------------------------------------------------
def calls(gs4d, degree):
    """(what, table, xf, bind bytes or None, form, bind_stride) over sizes, strides, table sizes and forms"""
    call = 0
    for n in (1, 129, 300):
        for m in (0, 1, 3, 17):
            for form in (rc.EACH, rc.INDEX, rc.BLEND4):
                if form == rc.EACH and (m > 3 or n > 129):
                    continue
                stride = rc.strides(degree)[call % 3]
                bs = 0 if form == rc.EACH else pc.STRIDES[form][call % 2]
                t = rc.table(n, degree, stride, seed=0x5350 + call, hostile=bool(call % 2))
                xf = rc.map_table(gs4d, m, call)
                bind = None if form == rc.EACH else pc.bind_bytes(gs4d, form, n, m, bs, seed=call)
                call += 1
                yield f"degree {degree}, n = {n}, m = {m}, form {form}, stride {stride}, bind_stride {bs}", t, xf, bind, form, bs


def source_rows(t, xf, form):
    return np.tile(t, (xf.shape[0], 1)) if form == rc.EACH else t


@pytest.mark.parametrize("degree", rc.DEGREES)
def test_rows_that_are_copied_and_words_that_are_kept(gs4d, degree):
    turned = copied = 0
    for what, t, xf, bind, form, bs in calls(gs4d, degree):
        got = gs4d.rotate_sh_host(t, xf, degree, bind, form if bind is not None else None, bs or None)
        rot = rc.rotated_mask(gs4d, xf, t.shape[0], bind, form, bs)
        assert got.shape[0] == rot.shape[0], what
        rc.assert_rows(got, got, source_rows(t, xf, form), rot, degree, what)
        if degree:
            moved = (got.view(u32) != source_rows(t, xf, form).view(u32)).any(1)
            assert not (moved & ~rot).any(), what
            turned, copied = turned + int(moved.sum()), copied + int((~rot).sum())
        else:
            assert np.array_equal(got.view(u32), source_rows(t, xf, form).view(u32)), what
    assert degree == 0 or (turned > 300 and copied > 300)


@pytest.mark.parametrize("degree", (1, 2, 3))
def test_each_with_one_map_is_index_zero_and_a_weight_one_slot_is_the_index_form(gs4d, degree):
    n = 150
    t = rc.table(n, degree, rc.strides(degree)[1], hostile=True)
    for name, l in list(rc.maps(gs4d).items()) + [(k, v[0]) for k, v in rc.hostile_maps(gs4d).items()]:
        each = gs4d.rotate_sh_host(t, l.reshape(1, 20), degree)
        index = gs4d.rotate_sh_host(t, l.reshape(1, 20), degree, np.zeros(n, u32))
        assert np.array_equal(each.view(np.uint8), index.view(np.uint8)), name      # byte-equal: the same code on the same machine
    xf = rc.map_table(gs4d, 9, 2)
    idx, rows = pc.weight_one_binds(gs4d, n, 9)
    assert np.array_equal(gs4d.rotate_sh_host(t, xf, degree, rows).view(np.uint8), gs4d.rotate_sh_host(t, xf, degree, idx).view(np.uint8))


@pytest.mark.parametrize("degree", (1, 2, 3))
def test_rows_that_name_no_map_or_a_map_that_does_not_rotate_are_byte_equal(gs4d, degree):
    n = 77
    t = rc.table(n, degree, rc.strides(degree)[1], hostile=True)
    assert np.isnan(t[:, :rc.used_words(degree)]).any() and np.isnan(t[:, rc.used_words(degree):]).any()
    xf = rc.map_table(gs4d, 3)
    same = lambda out: np.array_equal(out.view(np.uint8), t.view(np.uint8))
    assert same(gs4d.rotate_sh_host(t, xf, degree, np.full(n, rc.ID_NONE, u32)))
    assert same(gs4d.rotate_sh_host(t, xf, degree, np.full(n, 3, u32)))
    assert same(gs4d.rotate_sh_host(t, xf[:0], degree, np.zeros(n, u32)))                                  # m == 0 with a bind table: every row copied
    assert same(gs4d.rotate_sh_host(t, xf, degree, gs4d.bind_rows(np.full((n, 4), 4, u32), np.full((n, 4), np.nan, f32))))
    assert same(gs4d.rotate_sh_host(t, xf, degree, pc.packed(np.full(n, rc.ID_NONE, u32), 12), rc.INDEX, 12))
    for name, (l, rotates) in rc.hostile_maps(gs4d).items():
        if rotates is False:
            assert same(gs4d.rotate_sh_host(t, l.reshape(1, 20), degree)), name
            assert same(gs4d.rotate_sh_host(t, np.stack([l, l]), degree, np.arange(n, dtype=u32) % 2)), name
    assert gs4d.rotate_sh_host(t, xf[:0], degree).shape[0] == 0                                             # m == 0 with EACH: no rows


@pytest.mark.parametrize("degree", (1, 2, 3))
def test_the_identity_map_and_its_power_of_two_scales(gs4d, degree):
    """gs4d.h: every finite row comes back with its values and, for every word that is not a zero, its bits; a -0 need not keep its sign"""
    t = rc.table(200, degree, rc.strides(degree)[1], hostile=True)
    K3 = rc.used_words(degree)
    finite = np.isfinite(t[:, :K3]).all(1)
    assert finite.sum() > 100 and (t[finite, :K3].view(u32) == 0x80000000).any(), "no -0 coefficient among the finite rows"
    for scale in (1.0, 4.0, 2.0 ** -20):
        out = gs4d.rotate_sh_host(t, gs4d.affine4(scale=scale).reshape(1, 20), degree)
        a, b = t[finite], out[finite]
        assert np.array_equal(a[:, :K3], b[:, :K3]), scale                                                  # the values (-0 == +0)
        nz = a[:, :K3] != 0
        assert np.array_equal(a[:, :K3].view(u32)[nz], b[:, :K3].view(u32)[nz]), scale                      # the bits of everything but a zero
        assert np.array_equal(a[:, K3:].view(u32), b[:, K3:].view(u32))


def test_two_quarter_turns_about_z_are_the_half_turn(gs4d):
    quarter, half = gs4d.affine4(), gs4d.affine4()
    quarter[0:3], quarter[4:7] = (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0)             # x -> y, y -> -x
    half[0:3], half[4:7] = (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0)
    t = rc.table(300, 3, 208)
    assert (t[:, :48] != 0).all()
    once = gs4d.rotate_sh_host(t, quarter.reshape(1, 20), 3)
    twice = gs4d.rotate_sh_host(once, quarter.reshape(1, 20), 3)
    want = gs4d.rotate_sh_host(t, half.reshape(1, 20), 3)
    assert not np.array_equal(once.view(u32), t.view(u32))
    assert np.array_equal(twice.view(u32), want.view(u32))
    four = gs4d.rotate_sh_host(gs4d.rotate_sh_host(twice, quarter.reshape(1, 20), 3), quarter.reshape(1, 20), 3)
    assert np.array_equal(four.view(u32), t.view(u32)), "four quarter turns are not the identity"


def test_calls_the_device_would_refuse_write_nothing(gs4d):
    t, xf = rc.table(4, 1, 64), rc.map_table(gs4d, 2)
    lib, out = gs4d._lib, np.zeros((8, 16), f32)
    bind = np.zeros(4 * 64, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(n=4, stride=64, degree=1, m=2, bind=None, form=rc.EACH, bs=0)
    bad = [dict(degree=-1), dict(degree=4), dict(stride=8), dict(stride=24), dict(stride=1040), dict(stride=32), dict(stride=0), dict(form=3), dict(form=0xFFFFFFFF),
           dict(bind=bind), dict(form=rc.INDEX, bs=4), dict(form=rc.BLEND4, bs=32), dict(form=rc.INDEX, bind=bind, bs=0), dict(form=rc.INDEX, bind=bind, bs=6),
           dict(form=rc.BLEND4, bind=bind, bs=16), dict(form=rc.BLEND4, bind=bind, bs=40), dict(n=1 << 32), dict(m=1 << 32), dict(n=1 << 16, m=1 << 16)]
    for kw in bad:
        a = dict(good, **kw)
        lib.gs4d_host_rotate_sh(a["n"], p(t), a["stride"], a["degree"], p(xf), a["m"], None if a["bind"] is None else p(a["bind"]), a["form"], a["bs"], p(out))
        assert not out.any(), kw
    lib.gs4d_host_rotate_sh(4, p(t), 64, 1, p(xf), 2, None, rc.EACH, 0, p(out))
    assert out.view(u32).any()
    with pytest.raises(ValueError):
        gs4d.rotate_sh_host(t, xf, 1, np.zeros(3, u32))                       # fewer bind rows than table rows
    with pytest.raises(ValueError):
        gs4d.sh_rotation(np.zeros(12, f32))


# ---- the kernel's text on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=("plain", "asan_ubsan"))
def check_program(request, tmp_path_factory):
    """the stand-alone program, built plainly and as an executable instrumented with AddressSanitizer + UndefinedBehaviorSanitizer (nothing is preloaded)"""
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("sh_rotate_check") / "sh_rotate_check"
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *san, os.path.join(ROOT, "tests", "sh_rotate_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return str(exe)


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_the_kernels_text_gives_the_host_functions_bits_on_the_cpu(gs4d, check_program, tmp_path):
    paths = [tmp_path / f for f in ("rows.bin", "xf.bin", "bind.bin", "out.bin")]
    for degree in rc.DEGREES:
        for what, t, xf, bind, form, bs in calls(gs4d, degree):
            n, m = t.shape[0], xf.shape[0]
            if n == 300 and degree in (0, 1):                                 # (every form, table size and stride still comes by at the other sizes)
                continue
            t.tofile(paths[0])
            xf.tofile(paths[1])
            (bind if bind is not None else np.zeros(0, np.uint8)).tofile(paths[2])
            r = subprocess.run([check_program, "rows", str(n), str(t.shape[1] * 4), str(degree), str(m), str(form), str(bs), *map(str, paths)], capture_output=True,
                               text=True, timeout=120, env=ENV)
            assert r.returncode == 0, what + "\n" + r.stderr[-3000:]
            want = gs4d.rotate_sh_host(t, xf, degree, bind, form if bind is not None else None, bs or None)
            got = np.fromfile(paths[3], f32).reshape(want.shape)
            # the NaN rule of gs4d.h: the library's host code and this program come from two compilers
            rc.assert_rows(got, want, source_rows(t, xf, form), rc.rotated_mask(gs4d, xf, n, bind, form, bs), degree, what)


def test_the_matrices_of_the_stand_alone_text(gs4d, check_program, tmp_path):
    for name, l in list(rc.maps(gs4d).items()) + [(k, v[0]) for k, v in rc.hostile_maps(gs4d).items()]:
        l.tofile(tmp_path / "xf.bin")
        r = subprocess.run([check_program, "matrices", str(tmp_path / "xf.bin"), str(tmp_path / "d.bin")], capture_output=True, text=True, timeout=120, env=ENV)
        assert r.returncode == 0, name + "\n" + r.stderr[-3000:]
        got = np.fromfile(tmp_path / "d.bin", f32)
        ok, d = gs4d.sh_rotation(l)
        assert bool(got[84]) == ok and np.array_equal(got[:84].view(u32), d.view(u32)), name


def test_the_calls_checks_on_the_cpu(check_program):
    r = subprocess.run([check_program, "args"], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([check_program, "rows", "4", "24", "1", "1", "2", "0", "a", "b", "c", "d"], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 3, "a stride the call refuses must end the program before it opens a file"


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_the_constants_and_the_abi(gs4d):
    assert gs4d.SH_EACH == 2 == rc.EACH and (gs4d.POSE_INDEX, gs4d.POSE_BLEND4) == (rc.INDEX, rc.BLEND4)
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert "#define GS4D_SH_EACH 2u" in hdr
    assert "gs4d_rotate_sh(gs4d_ctx* ctx, gs4d_buf src, size_t n, size_t stride, int degree," in hdr
    assert "gs4d_host_sh_rotation(const float l[16], float d[84]);" in hdr
    internal = open(os.path.join(ROOT, "4dgaussiansplatrendering_amd", "csrc", "gs4d_internal.h")).read()
    for name, v in (("SHROT_TILE", rc.TILE[0]), ("SHROT_TILE_3", rc.TILE[3])):
        assert f"constexpr uint32_t {name} = {v};" in internal, name          # the thresholds the GPU tests are laid around
    assert rc.TILE[1] == rc.TILE[2] == rc.TILE[0]
    assert {"gs4d_rotate_sh", "gs4d_host_sh_rotation", "gs4d_host_rotate_sh"} <= set(gs4d.EXPORTS)
    assert gs4d._lib.gs4d_rotate_sh(None, 1, 1, 192, 3, 2, 1, 0, 2, 0, 3, 0) == -1        # GS4D_E_INVALID: no context
    # struct-free: the maps are gs4d_affine4 rows, the matrices plain floats
    assert ctypes.sizeof(gs4d.Affine4) == 80
    ok, d = gs4d.sh_rotation(gs4d.affine4())
    assert ok and d.shape == (84,) and d.dtype == f32

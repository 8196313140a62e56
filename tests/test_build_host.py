"""CPU: the host side of gs4d_build_records (include/gs4d.h) — the new batch builders against the pinned per-splat functions, and the
per-record text the kernel and the host builders share (csrc/build_record.h) compiled stand-alone with g++ against the host builders, bit for bit (NaN words: NaN on both sides), on every clean and hostile case."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import build_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def assert_same(got, want, what):
    ok = bc.same_bits(got, want)
    assert ok.all(), f"{what}: {int((~ok).sum())} words differ, first at {np.argwhere(~ok)[0].tolist()}"


# ---- the batch builders -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("clean", "hostile"))
def test_tvar_builder_equals_the_lifetime_fade_builder(gs4d, kind):
    n = 600
    p = bc.clean(gs4d, "4d_vel", n) if kind == "clean" else bc.hostile(gs4d, "4d_vel")
    n = p["pos"].shape[0]
    rng = np.random.default_rng(0x4255)
    life, fade = rng.uniform(0.5, 2.0, n).astype(f32), np.array(bc.FADES, f32)[np.arange(n) % len(bc.FADES)]
    if kind == "hostile":
        life[::7], fade[::5], fade[3::11], life[4::13] = 0.0, 1.0, 0.0, np.inf      # variances of 0 / 0, x / -0, 0, inf
    tvar = gs4d.time_variance(life, fade)
    assert tvar.dtype == f32 and tvar.shape == (n,)
    want = gs4d.build_records_4d(p["pos"], p["rot"], p["scale"], life, fade, p["dir"], p["rgba"])
    got = gs4d.build_records_4d_tvar(p["pos"], p["rot"], p["scale"], p["dir"], tvar, p["rgba"])
    assert_same(got, want, kind)
    assert np.array_equal(bc.bits(got[:, 23]), bc.bits(tvar)) or kind == "hostile"
    if kind == "clean":
        assert np.isfinite(got).all() and np.unique(bc.bits(got[:, 8:])).size > 10 * n


@pytest.mark.parametrize("kind", ("clean", "hostile"))
def test_2q_builder_equals_a_loop_over_splat4d_cov2q(gs4d, kind):
    p = bc.clean(gs4d, "4d_2q", 400) if kind == "clean" else bc.hostile(gs4d, "4d_2q")
    got = gs4d.build_records_4d_2q(p["pos"], p["rot"], p["rot_r"], p["scale"], p["rgba"])
    n = got.shape[0]
    want = np.empty((n, 24), f32)
    want[:, :4], want[:, 4:8] = p["pos"], p["rgba"]
    for i in range(n):
        want[i, 8:] = gs4d.splat4d_cov2q(p["rot"][i], p["rot_r"][i], p["scale"][i])
    assert_same(got, want, kind)
    if kind == "clean":
        assert np.isfinite(got).all()
    else:
        assert np.isnan(got).any() and np.isinf(got).any()      # the block does reach the non-finite paths


def test_time_variance_is_the_expression_of_the_reference(gs4d):
    """lifetime^2 in float32, the quotient in double: fade 0.5 takes the reference's constant ln 4 as a float, any other fade -2 * logf(fade)"""
    for life, fade in ((1.0, 0.5), (0.6, 0.5), (1.7, 0.3), (2.0, 0.9)):
        sq = float(f32(life) * f32(life))
        denom = float(f32(1.3862943611198906)) if f32(fade) == f32(0.5) else -2.0 * float(np.log(f32(fade)))
        want = f32(sq / denom)
        got = gs4d.time_variance(life, fade)
        assert isinstance(got, f32) and bc.bits(got) == bc.bits(want), (life, fade, got, want)
        cov = gs4d.splat4d_cov((1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), life, fade, (0.0, 0.0, 0.0))
        assert bc.bits(cov[15]) == bc.bits(got)
    both = gs4d.time_variance([1.0, 1.7], [0.5, 0.3])
    assert both.shape == (2,) and bc.bits(both[1]) == bc.bits(gs4d.time_variance(1.7, 0.3))


# ---- the kernel's per-record text on the CPU --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("build_record_check") / "build_record_check"
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "build_record_check.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return str(exe)


def run_check(exe, tmp_path, gs4d, form, p):
    n = p["pos"].shape[0]
    src, out = tmp_path / "params.bin", tmp_path / "records.bin"
    with open(src, "wb") as f:
        for name, width in bc.ROWS[form].items():
            assert p[name].shape == (n, width) and p[name].dtype == f32
            f.write(np.ascontiguousarray(p[name]).tobytes())
    r = subprocess.run([exe, str(bc.form_id(gs4d, form)), str(n), str(src), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.fromfile(out, f32).reshape(n, 24)


@pytest.mark.parametrize("form", bc.FORMS)
def test_the_kernels_record_text_gives_the_host_builders_bits_on_the_cpu(gs4d, check_program, tmp_path, form):
    sets = [("hostile block", bc.hostile(gs4d, form))]
    for n in bc.SIZES:
        sets += [(f"{name}, n = {n}", p) for name, p in bc.cases(gs4d, form, n)]
    for what, p in sets:
        got, want = run_check(check_program, tmp_path, gs4d, form, p), bc.host_records(gs4d, form, p)
        # Every word that is not a NaN on both sides must be equal as uint32.  The NaN rule of gs4d.h is needed even on one CPU: the library's host
        # code and this program come from two compilers, x86 gives a product or sum of two NaNs the sign and payload of its FIRST operand, and the
        # compilers order the operands of these commutative operations differently (seen here: 0x7FC00000 against 0xFFC00000 behind the negated
        # entries of the 4D_2Q matrices).
        assert_same(got, want, f"{form}, {what}")
    block = bc.host_records(gs4d, form, sets[0][1])
    assert np.isnan(block).any() and np.isinf(block).any() and (bc.bits(block) == 0x80000000).any()      # NaNs, infinities and negative zeros are reached


def test_the_parameter_structure_is_40_bytes(gs4d):
    assert ctypes.sizeof(gs4d.SplatParams) == 40
    assert [n for n, _ in gs4d.SplatParams._fields_] == ["form", "flags", "pos", "rot", "rot_r", "scale", "rgba", "dir", "tvar", "reserved"]
    assert (gs4d.PARAMS_3D, gs4d.PARAMS_4D_VEL, gs4d.PARAMS_4D_2Q) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert "gs4d_build_records(gs4d_ctx* ctx, const gs4d_splat_params* params, size_t n, gs4d_buf dst)" in hdr


def test_the_package_imports_without_torch():
    code = ("import sys, importlib; sys.modules['torch'] = None; m = importlib.import_module('4dgaussiansplatrendering_amd'); "
            "assert hasattr(m.Context, 'write_tensor') and hasattr(m.Context, 'build_records')")
    r = subprocess.run([__import__("sys").executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]

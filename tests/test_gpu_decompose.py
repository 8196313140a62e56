"""GPU: gs4d_decompose_records — the splat parameters of a set of 96-byte records, taken out on the device (include/gs4d.h).

Built to the plan of tests/test_gpu_build.py and tests/test_gpu_warp.py: every output row is compared word for word with the host definition
(tests/decompose_cases.py: equal as uint32, a word that is a NaN on both sides counting as equal), with the bytes behind row n of every destination,
guard buffers between the allocations and src compared against what was uploaded; destinations in every subset the argument check allows; the round
trip decompose -> build on the device against the host's; ordering behind a call that writes src and in front of a reader on the caller's stream;
every refusal through the C ABI.  All calls go through the Python binding over the C ABI."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import decompose_cases as dc
from test_gpu_build import GUARD, SENTINEL, fill, untouched

pytestmark = pytest.mark.gpu
f32 = np.float32
EXTRA = 3                                                    # rows >= n of a destination that must stay as they are


def sentinel_rows(ctx, rows, n, guards=None):
    """{name: buffer} of n + EXTRA rows and 32 bytes more, all SENTINEL, each followed by a guard buffer when `guards` is given"""
    bufs = {}
    for k, width in rows.items():
        bufs[k] = fill(ctx, (n + EXTRA) * 4 * width + 32)
        if guards is not None:
            guards.append(fill(ctx, GUARD))
    return bufs


def check_rows(ctx, bufs, rows, n, want, what):
    """the first n rows of every buffer named in `want` are the host's, the bytes behind them SENTINEL; a buffer not in `want` is all SENTINEL"""
    for k, width in rows.items():
        size = (n + EXTRA) * 4 * width + 32
        got = ctx.read(bufs[k], np.uint8, size)
        if k not in want:
            assert (got == SENTINEL).all(), f"{what}: {k} was not given and changed"
            continue
        dc.assert_same({k: got[:n * 4 * width].view(f32).reshape(n, width)}, {k: want[k]}, what)
        assert (got[n * 4 * width:] == SENTINEL).all(), f"{what}: bytes of {k} behind row n - 1 changed"


# ---- 1. the rows -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", dc.SETS)
def test_rows_equal_the_host_definition(gs4d, which):
    ctx = gs4d.Context(64, 64)
    total = max(dc.SIZES) + max(dc.FIRSTS)
    rec = dc.records(gs4d, which, total)
    own = dc.form_of(gs4d, which)
    other = gs4d.PARAMS_3D if own == gs4d.PARAMS_4D_VEL else gs4d.PARAMS_4D_VEL
    runs = [(own, n, first) for n in dc.SIZES for first in dc.FIRSTS] + [(other, 257, 7)]      # (the other form reads the same words differently)
    for form, n, first in runs:
        what = f"{which} as form {form}, n = {n}, src_first = {first}"
        rows = gs4d.PARAM_ROWS[form]
        guards = [fill(ctx, GUARD)]
        src = ctx.buffer(rec[:first + n])                       # exactly src_first + n records
        guards.append(fill(ctx, GUARD))
        bufs = sentinel_rows(ctx, rows, n, guards)
        params = ctx.decompose_records(src, n, form, src_first=first, **bufs)
        assert params.form == form and params.buffers() == bufs
        check_rows(ctx, bufs, rows, n, gs4d.decompose_records_host(rec[first:first + n], form), what)
        assert all(untouched(ctx, g) for g in guards), f"{what}: a guard buffer changed"
        assert np.array_equal(ctx.read(src, np.uint32, (first + n) * 24), dc.bits(rec[:first + n]).reshape(-1)), f"{what}: src changed"
        assert ctx.shadow_builds(src) == 0
        for b in guards + [src] + list(bufs.values()):
            ctx.delete(b)
    ctx.finish()                                                # reports device-side check failures
    ctx.close()


def test_destinations_are_allocated_and_read_params_reads_them(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 300
    rec = dc.records(gs4d, "4d_2q", n + 7)
    src = ctx.buffer(rec)
    want = gs4d.decompose_records_host(rec[7:], gs4d.PARAMS_4D_VEL)
    params = ctx.decompose_records(src, n, gs4d.PARAMS_4D_VEL, src_first=7)
    assert set(params.buffers()) == set(want) and ctx.device_ptr(params.scale)[1] >= 12 * n
    dc.assert_same(ctx.read_params(params, n), want, "every destination allocated")
    mine = fill(ctx, 16 * n)
    some = ctx.decompose_records(src, n, gs4d.PARAMS_4D_VEL, src_first=7, only=("rot", "tvar"), rot=mine)
    assert set(some.buffers()) == {"rot", "tvar"} and some.rot == mine
    dc.assert_same(ctx.read_params(some, n), {k: want[k] for k in ("rot", "tvar")}, "only rot and tvar")
    with pytest.raises(ValueError):
        ctx.decompose_records(src, n, gs4d.PARAMS_4D_2Q)
    with pytest.raises(ValueError):
        ctx.decompose_records(src, n, gs4d.PARAMS_3D, only=("dir",))
    ctx.close()


def test_no_records_is_a_no_op(gs4d):
    ctx = gs4d.Context(64, 64)
    rec = dc.records(gs4d, "hard_4d", 8)
    rows = gs4d.PARAM_ROWS[gs4d.PARAMS_4D_VEL]
    src, bufs = ctx.buffer(rec), sentinel_rows(ctx, rows, 0)
    ctx.decompose_records(src, 0, gs4d.PARAMS_4D_VEL, **bufs)
    ctx.decompose_records(src, 0, gs4d.PARAMS_4D_VEL, src_first=8, **bufs)
    ctx.finish()
    check_rows(ctx, bufs, rows, 0, {}, "n == 0")
    assert np.array_equal(ctx.read(src, np.uint32, 8 * 24), dc.bits(rec).reshape(-1))
    ctx.close()


# ---- 2. selective outputs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("3d", "4d_2q", "hard_3d", "hard_4d"))
def test_every_subset_of_the_destinations(gs4d, which):
    """the destinations given in every subset the argument check allows; with neither rot nor scale the instance without the eigen-solve runs"""
    ctx = gs4d.Context(64, 64)
    n, first = 300, 7
    form, rows = dc.form_of(gs4d, which), dc.rows_of(gs4d, which)
    rec = dc.records(gs4d, which, first + n)
    src = ctx.buffer(rec)
    full = gs4d.decompose_records_host(rec[first:], form)
    subsets = [s for r in range(1, len(rows) + 1) for s in itertools.combinations(rows, r)]
    assert len(subsets) == 2 ** len(rows) - 1
    for only in subsets:
        bufs = sentinel_rows(ctx, rows, n)
        ctx.decompose_records(src, n, form, src_first=first, **{k: bufs[k] for k in only})
        check_rows(ctx, bufs, rows, n, {k: full[k] for k in only}, f"{which}, only {only}")
        for b in bufs.values():
            ctx.delete(b)
    ctx.finish()
    ctx.close()


# ---- 3. the round trip on the device ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", dc.SETS)
def test_decompose_then_build_on_the_device_equals_the_hosts(gs4d, which):
    ctx = gs4d.Context(64, 64)
    n = 769
    form = dc.form_of(gs4d, which)
    rec = dc.records(gs4d, which, n)
    src, kb, ib = ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
    ctx.keygen(src, 0.0, (0.0, 0.0, 150.0), kb, ib, n)          # src has a shadow: the call must neither rebuild it nor make it stale
    ctx.finish()
    before = ctx.shadow_builds(src)
    assert before == 1
    params = ctx.decompose_records(src, n, form)
    back = ctx.build_records(params, n)                          # no read-back in between
    ctx.keygen(src, 0.0, (0.0, 0.0, 150.0), kb, ib, n)
    got = ctx.read(back, f32, n * 24).reshape(n, 24)
    assert ctx.shadow_builds(src) == before, "the call touched the shadow of src"
    want = dc.rebuild(gs4d, form, gs4d.decompose_records_host(rec, form))
    ok = dc.same_bits(got, want)
    assert ok.all(), f"{which}: {int((~ok).any(1).sum())} of {n} rebuilt records differ from the host's decompose-then-build"
    if not which.startswith("hard"):                            # and the set has come back, as far as float32 goes
        err = dc.round_trip_error(gs4d, rec, form, ctx.read_params(params, n))
        assert err.max() < 1e-5, err.max()
    ctx.close()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------------------------
def test_a_call_behind_a_transform_sees_the_transformed_records(gs4d):
    ctx = gs4d.Context(64, 64)
    n = 1000
    rec = dc.records(gs4d, "4d_vel", n)
    row = gs4d.affine4((0.8, 0.6, 0.0, 0.0), 1.5, (10.0, -20.0, 30.0), (0.5, 0.0, -0.25), 2.0, 3.0)
    moved = gs4d.transform_records_host(rec, row)
    want = gs4d.decompose_records_host(moved, gs4d.PARAMS_4D_VEL)
    assert not np.array_equal(want["scale"], gs4d.decompose_records_host(rec, gs4d.PARAMS_4D_VEL)["scale"]), "the transform changes nothing: the test shows nothing"
    first, xf = ctx.buffer(rec), ctx.buffer(np.ascontiguousarray(row, f32).reshape(1, 20))
    src = fill(ctx, n * 96)
    ctx.finish()
    ctx.transform_records(first, n, xf, 1, dst=src)              # writes src ...
    params = ctx.decompose_records(src, n, gs4d.PARAMS_4D_VEL)   # ... which the call right behind it reads
    ctx.subdata(src, np.zeros(n * 24, f32))                      # directly behind: the call must not see the zeros
    dc.assert_same(ctx.read_params(params, n), want, "behind a transform")
    ctx.close()


def test_decompose_into_torch_tensors():
    """a destination handed to torch on the caller's stream holds the rows: a program of its own (tests/gpu_decompose_to_torch.py) because torch has
    to initialise its HIP runtime before libgs4d.so is loaded."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_decompose_to_torch.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "decompose to torch ok" in r.stdout


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form_name", ("3d", "4d_vel"))
def test_argument_errors_leave_everything_as_it_was(gs4d, form_name):
    n, first = 300, 5
    ctx, lib = gs4d.Context(64, 64), gs4d._lib
    form = dc.form_of(gs4d, form_name)
    rows = gs4d.PARAM_ROWS[form]
    rec = dc.records(gs4d, form_name, first + n)
    src, short_src = ctx.buffer(rec), ctx.buffer(rec.reshape(-1)[:-1])
    bufs = {k: fill(ctx, n * 4 * w) for k, w in rows.items()}
    short = {k: fill(ctx, n * 4 * w - 4) for k, w in rows.items()}
    spare, dead = fill(ctx, 96 * n), fill(ctx, 64)
    ctx.delete(dead)                                            # (last: a buffer made from here on could take its name)
    names = gs4d.Context.PARAM_BUFFERS

    def call(src=src, n=n, first=first, form=form, flags=0, reserved=0, null=False, none=False, **over):
        use = {k: 0 if none else bufs.get(k, 0) for k in names}
        use.update(over)
        params = gs4d.SplatParams(form, flags, *(use[k] for k in names), reserved)
        return lib.gs4d_decompose_records(ctx._h, src, ctypes.c_size_t(n), ctypes.c_size_t(first), None if null else ctypes.byref(params))

    big = 1 << 32
    bad = {"out == NULL": (dict(null=True), b"out"), "form 2Q": (dict(form=gs4d.PARAMS_4D_2Q), b"form"), "form 3": (dict(form=3), b"form"),
           "form 0xFFFFFFFF": (dict(form=0xFFFFFFFF), b"form"), "flags": (dict(flags=1), b"flags"), "reserved": (dict(reserved=1), b"reserved"),
           "n > 0xFFFFFFFF": (dict(n=big), b"n"), "src_first > 0xFFFFFFFF": (dict(first=big), b"src_first"), "src_first + n > 0xFFFFFFFF": (dict(first=big - n), b"src_first"),
           "no destination": (dict(none=True), b"destination"), "rot_r given": (dict(rot_r=spare), b"rot_r"),
           "src too small": (dict(src=short_src), b"src"), "src too small for src_first": (dict(first=first + 1), b"src"),
           "dead src": (dict(src=dead), b"src"), "no src": (dict(src=0), b"src"), "unknown src": (dict(src=9999), b"src")}
    for k in rows:
        bad.update({f"dead {k}": ({k: dead}, k.encode()), f"unknown {k}": ({k: 9999}, k.encode()), f"{k} too small": ({k: short[k]}, k.encode()),
                    f"{k} == src": ({k: src}, k.encode())})
    for k in ("dir", "tvar"):
        if k not in rows:
            bad[f"{k} given in the 3D form"] = ({k: spare}, k.encode())
    for a, b in itertools.combinations(rows, 2):
        bad[f"{a} == {b}"] = ({b: bufs[a]}, b.encode())
    for what, (kw, operand) in bad.items():
        assert call(**kw) == -1, what
        message = lib.gs4d_last_error(ctx._h)
        assert b"decompose_records" in message and operand in message, (what, message)
    ctx.finish()
    everything = list(bufs.items()) + list(short.items())
    assert all(untouched(ctx, b, n * 4 * rows[k] - 4) for k, b in everything) and untouched(ctx, spare, 96 * n), "a refused call wrote something"
    assert np.array_equal(ctx.read(src, np.uint32, (first + n) * 24), dc.bits(rec).reshape(-1))
    assert call(n=0) == 0 and call(n=0, first=first + n) == 0 and call(n=0, first=first + n + 1) == -1      # (a no-op still needs src_first records)
    ctx.finish()
    assert all(untouched(ctx, b, n * 4 * rows[k]) for k, b in bufs.items())
    # the call works after the refusals, and with a single destination
    assert call() == 0
    want = gs4d.decompose_records_host(rec[first:], form)
    dc.assert_same({k: ctx.read(bufs[k], f32, n * w).reshape(n, w) for k, w in rows.items()}, want, "after the refusals")
    assert np.array_equal(ctx.read(src, np.uint32, (first + n) * 24), dc.bits(rec).reshape(-1)) and ctx.shadow_builds(src) == 0
    ctx.close()

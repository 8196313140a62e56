"""CPU: the depth-key bounds as a pure function (gs4d_host_key_bounds) and the checker's side of the hostile-record contract.

* The bounds are a proof: every float32 key of every record inside the box lies in [bias, bias + span] — on every key-bounds case of
  tests/hostile_cases.py and on seeded random boxes with offsets up to 1e30.  The keys are the checker's (oracle.keygen), restated here in
  numpy float32 and compared bit for bit; a float64 evaluation of the same formula tells rounding cases from overflow cases.
* The formula gs4d_keygen used before (margins relative to the distance: `parent_bounds`, restated from commit c92f0bf) is NOT one: the
  same property fails on it, which is what test_parent_formula_was_no_proof records.
* The bounds stay useful: for the headline shapes the span has no more bits than that commit's.
* The checker meets, by itself, everything tests/test_gpu_hostile.py asks of the GPU on every case.
"""
import math

import numpy as np
import pytest

import hostile_cases as hc
import scenes

FULL = 0xFFFFFFFF


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------
def keys_f32(rec, t, cam):
    """Scenes.h:28-36, 314-319 in numpy float32, operation for operation as gs4do_keygen / k_keygen evaluate it."""
    f = np.float32
    rec = np.asarray(rec, f).reshape(-1, 24)
    with np.errstate(all="ignore"):
        ct = f(t) - rec[:, 3]
        d = [(rec[:, ax] + rec[:, 20 + ax] * ct) - f(cam[ax]) for ax in range(3)]
        return f(1.0) / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def keys_f64(rec, t, cam):
    """The same formula in float64 on the same float32 inputs: the reference the float32 key is a rounding of."""
    rec = np.asarray(rec, np.float32).reshape(-1, 24).astype(np.float64)
    with np.errstate(all="ignore"):
        ct = float(np.float32(t)) - rec[:, 3]
        d = [(rec[:, ax] + rec[:, 20 + ax] * ct) - float(np.float32(cam[ax])) for ax in range(3)]
        return 1.0 / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def same_keys(a, b):
    """bit-equal where not NaN, NaN where NaN (payloads and signs of NaNs are nobody's contract)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def box_of(rec):
    """What k_soa_repack reduces: (lo[7], hi[7]) over position, mu_t and the velocity sig[3].xyz, or None when a value is not finite
    (bbox[14]: gs4d_keygen then claims no bound at all)."""
    q = np.asarray(rec, np.float32).reshape(-1, 24)[:, [0, 1, 2, 3, 20, 21, 22]]
    if not np.isfinite(q).all():
        return None
    return q.min(0), q.max(0)


def parent_bounds(lo, hi, t, cam):
    """gs4d_keygen's formula at commit c92f0bf (doubles; margins (1 +- 1e-4) +- 1e-3 on the distance, (1 -+ 1e-5) on the key)."""
    lo, hi, cam, t = [float(v) for v in lo], [float(v) for v in hi], [float(np.float32(v)) for v in cam], float(np.float32(t))
    bits = lambda x: int(np.float32(x).view(np.uint32))
    c_lo, c_hi = t - hi[3], t - lo[3]
    d2 = n2 = 0.0
    for ax in range(3):
        p = [lo[4 + ax] * c_lo, lo[4 + ax] * c_hi, hi[4 + ax] * c_lo, hi[4 + ax] * c_hi]
        m_lo, m_hi = lo[ax] + min(p), hi[ax] + max(p)
        far = max(abs(m_lo - cam[ax]), abs(m_hi - cam[ax]))
        near = max(0.0, m_lo - cam[ax], cam[ax] - m_hi)
        d2 += far * far
        n2 += near * near
    bias, span = 0, FULL
    with np.errstate(all="ignore"):
        dmax = math.sqrt(d2) * (1.0 + 1e-4) + 1e-3 if math.isfinite(d2) else math.inf
        lb = np.float32((1.0 / dmax) * (1.0 - 1e-5)) if dmax > 0 else np.float32(np.inf)
        if math.isfinite(dmax) and lb > 0 and np.isfinite(lb):
            bias = bits(lb)
            dmin = math.sqrt(n2) * (1.0 - 1e-4) - 1e-3
            if dmin > 0.0:
                ub = np.float32((1.0 / dmin) * (1.0 + 1e-5))
                if np.isfinite(ub) and bits(ub) >= bias:
                    span = bits(ub) - bias
    return bias, span


def outside(keys, bias, span):
    """indices of the keys outside [bias, bias + span], as k_keygen re-checks them (NaN keys: their bit patterns, like any other)"""
    kb = np.asarray(keys, np.float32).view(np.uint32).astype(np.int64)
    return np.flatnonzero((kb < bias) | (kb - bias > span))


def span_bits(span):
    return 32 if span == FULL else max(1, int(span).bit_length())


# ---- random boxes ------------------------------------------------------------------------------------------------------------------------
OFFSETS = (0.0, 1e3, 1e5, 5e6, 1e9, 1e19, 1e30)
N_RANDOM = 2400


def random_box(k):
    """Box k of the seeded family: (records at the corners and at random points, t, camera)."""
    rng = np.random.default_rng(0x5EED + k)
    off = np.array([rng.choice(OFFSETS) * rng.choice((-1.0, 1.0)) for _ in range(3)])
    ext = 10.0 ** rng.uniform(-3.0, 4.0, 3)
    vmax = rng.choice((0.0, 10.0 ** rng.uniform(-3.0, 6.0)))
    trange = rng.choice((0.0, 10.0 ** rng.uniform(-3.0, 6.0)))
    lo = np.concatenate([off, [0.0], -vmax * rng.uniform(0.0, 1.0, 3)]).astype(np.float32)
    hi = np.concatenate([off + ext, [trange], vmax * rng.uniform(0.0, 1.0, 3)]).astype(np.float32)
    corners = np.array([[(hi if (c >> b) & 1 else lo)[b] for b in range(7)] for c in range(128)], np.float32)
    inner = (lo + (hi.astype(np.float64) - lo) * rng.uniform(0.0, 1.0, (64, 7))).astype(np.float32)
    q = np.clip(np.concatenate([corners, inner]), lo, hi)
    rec = np.zeros((len(q), 24), np.float32)
    rec[:, 0:4], rec[:, 20:23], rec[:, 23] = q[:, 0:4], q[:, 4:7], 1.0
    t = np.float32(rng.choice((0.0, trange, rng.uniform(-1.0, 2.0) * max(trange, 1.0))))
    where = k % 5
    cam = lo[:3].astype(np.float64) + (hi[:3].astype(np.float64) - lo[:3]) * rng.uniform(0.0, 1.0, 3)      # 0: inside
    ax = int(rng.integers(3))
    if where == 1:
        cam[ax] = hi[ax]                                                                   # on a face
    elif where == 2:
        cam[ax] = np.nextafter(hi[ax], np.float32(np.inf)) if k % 2 else np.nextafter(lo[ax], np.float32(-np.inf))      # an ulp off a face
    elif where == 3:
        cam = cam + (ext.max() + abs(off).max()) * 10.0 ** rng.uniform(0.0, 3.0) * rng.choice((-1.0, 1.0), 3)      # far away
    elif where == 4:
        cam[ax] = hi[ax] + ext[ax] * 10.0 ** rng.uniform(-3.0, 1.0)                          # near, outside
    return rec, float(t), np.clip(cam, -3e38, 3e38).astype(np.float32)


def violations(bounds_fn, rec, t, cam):
    box = box_of(rec)
    if box is None:
        return np.zeros(0, np.int64), (0, FULL)
    bias, span = bounds_fn(box[0], box[1], t, cam)
    return outside(keys_f32(rec, t, cam), bias, span), (bias, span)


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.names())
def test_float32_restatement_equals_the_checkers_keys(oracle, name):
    c = hc.get(name)
    _, ekeys = oracle.keygen(c.rec, c.t, c.cam[0])
    assert same_keys(keys_f32(c.rec, c.t, c.cam[0]), ekeys)
    assert bool(np.isnan(ekeys).any()) == c.nan_key


@pytest.mark.parametrize("name", hc.names())
def test_bounds_hold_on_every_case(gs4d, oracle, name):
    c = hc.get(name)
    _, ekeys = oracle.keygen(c.rec, c.t, c.cam[0])
    box = box_of(c.rec)
    if box is None:
        return                                              # non-finite input: no bound is claimed (tests/test_gpu_hostile.py checks the frame)
    bias, span = gs4d.key_bounds(box[0], box[1], c.t, c.cam[0])
    bad = outside(ekeys, bias, span)
    k64 = keys_f64(c.rec, c.t, c.cam[0])
    assert bad.size == 0, (name, bias, span, [(int(i), float(ekeys[i]), float(k64[i])) for i in bad[:4]])


def test_bounds_hold_on_random_boxes(gs4d):
    failures, claimed, rounding, overflow = [], 0, 0, 0
    for k in range(N_RANDOM):
        rec, t, cam = random_box(k)
        bad, (bias, span) = violations(gs4d.key_bounds, rec, t, cam)
        claimed += (bias, span) != (0, FULL)
        k32, k64 = keys_f32(rec, t, cam), keys_f64(rec, t, cam)
        with np.errstate(all="ignore"):
            overflow += bool(((k32 == 0.0) & (k64 > 0.0)).any() or np.isnan(k32).any())
            rounding += bool((np.abs(k32.astype(np.float64) - k64) > 1e-4 * k64).any())
        if bad.size:
            failures.append((k, t, cam.tolist(), bias, span, [(int(i), float(k32[i]), float(k64[i])) for i in bad[:3]]))
    print(f"{N_RANDOM} boxes: bounds claimed on {claimed}; float32 keys off their float64 value by more than the old margin on {rounding}, "
          f"overflowing on {overflow}")
    assert not failures, failures[:5]
    assert claimed > N_RANDOM // 2 and rounding > 100 and overflow > 100      # the family reaches what it is meant to reach


def test_parent_formula_was_no_proof():
    """The property above, run against the formula gs4d_keygen had: the four sets of the issue's table and the random boxes break it."""
    broken = {}
    for name in ("far_x_2e19", "utm_below_bias", "utm_above_span", "utm_slab_20000"):
        c = hc.get(name)
        bad, _ = violations(parent_bounds, c.rec, c.t, c.cam[0])
        broken[name] = (int(bad.size), c.n)
    nbox = sum(violations(parent_bounds, *random_box(k))[0].size > 0 for k in range(0, N_RANDOM, 4))
    print("keys outside the parent's bounds:", broken, f"; random boxes with one: {nbox} of {N_RANDOM // 4}")
    assert broken == {"far_x_2e19": (1, 2), "utm_below_bias": (2, 2), "utm_above_span": (2, 2), "utm_slab_20000": (20000, 20000)}
    assert nbox > 0


def _shape_nine_bit(gs4d):
    n = 150000
    pos4, q, sc, life, fade, vel, rgba = scenes.cube_params_4d(n, seed=71)
    return gs4d.build_records_4d(pos4, q, sc * 3.0, life, fade, vel * 0.3, rgba), 21.5


def _shape_bench(gs4d):
    n = 1000000
    pos = scenes.cube_params(n)[0]
    rec = np.zeros((n, 24), np.float32)                    # the box reads position, mu_t (0) and velocity (0) only
    rec[:, 0:3] = pos
    return rec, 0.0


# (bias, span) of gs4d_keygen at commit c92f0bf for the shape's box (parent_bounds above reproduces them)
PARENT = {"nine_bit": (978833838, 20322948), "bench": (981601492, 11098194)}


@pytest.mark.parametrize("shape", ["nine_bit", "bench"])
def test_bounds_stay_useful(gs4d, shape):
    """test_nine_bit_digits_for_wide_key_spans' moving set (25 bits: three 9-bit passes) and bench.py's 10^6 cube seen from outside (24 bits:
    three 8-bit passes): the proven span needs no more bits than before, and still holds every key."""
    rec, t = (_shape_nine_bit if shape == "nine_bit" else _shape_bench)(gs4d)
    cam = scenes.CAM_CUBE[0]
    lo, hi = box_of(rec)
    assert parent_bounds(lo, hi, t, cam) == PARENT[shape]
    bias, span = gs4d.key_bounds(lo, hi, t, cam)
    print(shape, "parent", PARENT[shape], span_bits(PARENT[shape][1]), "now", (bias, span), span_bits(span))
    assert span_bits(span) <= span_bits(PARENT[shape][1])
    assert bias >= PARENT[shape][0] and bias + span <= sum(PARENT[shape])      # inside the old interval on both sides
    assert outside(keys_f32(rec, t, cam), bias, span).size == 0


def test_no_bound_is_claimed_for_what_is_not_finite(gs4d):
    lo, hi = np.zeros(7, np.float32), np.ones(7, np.float32)
    cam = (5.0, 5.0, 5.0)
    assert gs4d.key_bounds(lo, hi, 0.5, cam) != (0, FULL)
    assert gs4d.key_bounds(lo, hi, 0.5, cam, gs4d.KEY_VIEW_Z) == (0, FULL)
    assert gs4d.key_bounds(lo, hi, float("nan"), cam) == (0, FULL)
    assert gs4d.key_bounds(lo, hi, 0.5, (5.0, float("inf"), 5.0)) == (0, FULL)
    bad = hi.copy()
    bad[5] = np.nan
    assert gs4d.key_bounds(lo, bad, 0.5, cam) == (0, FULL)
    assert gs4d.key_bounds(hi, lo, 0.5, cam) == (0, FULL)                                   # an empty box
    wide = hi.copy()
    wide[3] = 3e38
    assert gs4d.key_bounds(lo, wide, -3e38, cam) == (0, FULL)                               # t - mu_t overflows: 0 * inf is possible
    bias, span = gs4d.key_bounds(lo, hi, 0.5, (0.5, 0.5, 0.5))                              # camera inside: a lower bound only
    assert bias > 0 and span == FULL


# ---- the checker on every case: the contract the GPU is held to ---------------------------------------------------------------------------
def checker_frame(oracle, rec, c, order=None):
    """(keys, permutation, projected records, image) of the checker for records `rec` under case c's time and camera"""
    eidx, ekeys = oracle.keygen(rec, c.t, c.cam[0])
    if order is None:
        _, order = oracle.sort_pairs(ekeys.view(np.uint32), eidx, "std")
    eproj = oracle.preprocess(oracle.MODE_4D, rec, c.view, c.proj, hc.W, hc.H, c.t, c.min_opacity)
    img = oracle.composite(eproj, order, oracle.MODE_4D, hc.W, hc.H, oracle.clear_image(hc.W, hc.H), nthreads=4)
    return ekeys, order, eproj, img


@pytest.mark.parametrize("name", hc.names())
def test_checker_meets_the_contract(oracle, name):
    c = hc.get(name)
    ekeys, order, eproj, img = checker_frame(oracle, c.rec, c)
    valid = eproj["valid"] != 0
    wrong = np.flatnonzero(valid == c.dead)
    assert wrong.size == 0, (name, [(int(i), bool(c.dead[i]), bool(c.hostile[i])) for i in wrong[:8]])
    assert np.isfinite(img).all()
    # the dead records removed, the order remapped: the same image, bit for bit
    rec2, remap = hc.without_dead(c)
    order2 = remap[order][~c.dead[order]].astype(np.uint32)
    _, _, eproj2, img2 = checker_frame(oracle, rec2, c, order=order2)
    assert (eproj2["valid"] != 0).all()
    assert np.array_equal(img.view(np.uint32), img2.view(np.uint32))
    if c.whole_screen:
        assert float(np.abs(img - oracle.CLEAR).max(axis=2).min()) > 0.05, "a whole-screen footprint leaves no pixel at the clear colour"

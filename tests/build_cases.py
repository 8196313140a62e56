"""Inputs for the gs4d_build_records tests (include/gs4d.h): parameter sets of the three forms as dicts {buffer name: float32 [n, k]},
clean and hostile, and the host builders they are compared with.

clean     seeded: unit and non-unit quaternions, scales over five decades, positions and times of the scale of scenes.py, temporal variances from
          time_variance of lifetimes and fades (fade 0.5, the reference's special case, among them).
hostile   one fault per row on a clean row: 0, -0, a denormal, NaN, +Inf, -Inf and 1e30 in every component of every parameter in turn; zero and
          vanishing quaternions (unit's identity case); whole scale rows of 0, -0, +-Inf and 1e30; temporal variances of 0, -0, a negative value,
          Inf and NaN; velocities of +-Inf.  These are the rows where a kernel that skipped an `x * 0` term would give other bits.
"""
import numpy as np

f32 = np.float32
TILE = 256                                                   # BUILD_TILE (csrc/gs4d_internal.h)
SIZES = (1, 63, 255, 256, 257, 3 * 256 + 1)                  # one lane, short of a wave, either side of a tile, several tiles plus one
FORMS = ("3d", "4d_vel", "4d_2q")
# floats per row of every parameter buffer of a form, in the order of gs4d_splat_params
ROWS = {
    "3d": {"pos": 3, "rot": 4, "scale": 3, "rgba": 4},
    "4d_vel": {"pos": 4, "rot": 4, "scale": 3, "rgba": 4, "dir": 3, "tvar": 1},
    "4d_2q": {"pos": 4, "rot": 4, "rot_r": 4, "scale": 4, "rgba": 4},
}
READ_BYTES = {"3d": 56, "4d_vel": 72, "4d_2q": 80}            # per record: DESIGN.md's traffic figures
DENORMAL = f32(1e-42)
FAULTS = (f32(0.0), f32(-0.0), DENORMAL, f32(np.nan), f32(np.inf), f32(-np.inf), f32(1e30))
FADES = (0.5, 0.3, 0.9, 0.01)
T = 25.0                                                     # the time of the picture sets


def form_id(gs4d, form):
    return {"3d": gs4d.PARAMS_3D, "4d_vel": gs4d.PARAMS_4D_VEL, "4d_2q": gs4d.PARAMS_4D_2Q}[form]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want):
    """the comparison of gs4d.h: equal as uint32, except that a word that is a NaN in both counts as equal"""
    g, w = bits(got), bits(want)
    return (g == w) | (np.isnan(g.view(f32)) & np.isnan(w.view(f32)))


def quaternions(rng, n):
    """every other one of unit length (in float32), the others as they come, over four decades of length"""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[1::2] *= 10.0 ** rng.uniform(-2.0, 2.0, (q[1::2].shape[0], 1))
    return q.astype(f32)


def clean(gs4d, form, n, seed=0x4252):
    rng = np.random.default_rng([seed, FORMS.index(form)])
    rows = ROWS[form]
    p = {"pos": rng.uniform(-200.0, 200.0, (n, rows["pos"])).astype(f32), "rot": quaternions(rng, n),
         "scale": (10.0 ** rng.uniform(-3.0, 2.0, (n, rows["scale"]))).astype(f32), "rgba": rng.uniform(0.0, 1.0, (n, 4)).astype(f32)}
    if rows["pos"] == 4:
        p["pos"][:, 3] = rng.uniform(0.0, 50.0, n).astype(f32)
    if form == "4d_2q":
        p["rot_r"] = quaternions(rng, n)
    if form == "4d_vel":
        p["dir"] = rng.uniform(-5.0, 5.0, (n, 3)).astype(f32)
        life, fade = rng.uniform(0.5, 2.0, n).astype(f32), np.array(FADES, f32)[np.arange(n) % len(FADES)]
        p["tvar"] = gs4d.time_variance(life, fade).reshape(n, 1)
    return {k: np.ascontiguousarray(p[k]) for k in rows}


def hostile(gs4d, form):
    """the hostile block of a form: one row per fault, each on a clean row of its own"""
    rows = ROWS[form]
    faults = [(name, k, v) for name, width in rows.items() for k in range(width) for v in FAULTS]
    whole = [(name, None, v) for name in ("rot", "rot_r") if name in rows for v in (f32(0.0), f32(-0.0), DENORMAL, f32(1e-30), f32(1e30))]
    whole += [("scale", None, v) for v in (f32(0.0), f32(-0.0), f32(np.inf), f32(-np.inf), f32(1e30))]
    if form == "4d_vel":
        whole += [("tvar", None, f32(-0.75)), ("dir", None, f32(np.inf)), ("dir", None, f32(-np.inf))]
    p = clean(gs4d, form, len(faults) + len(whole), seed=0x4253)
    for i, (name, k, v) in enumerate(faults + whole):
        if k is None:
            p[name][i, :] = v
        else:
            p[name][i, k] = v
    return p


def resized(p, n):
    """n rows of a block, taken round and round (starting at row n, so that small sizes do not all see the same first rows)"""
    rows = next(iter(p.values())).shape[0]
    take = (np.arange(n) + n) % rows
    return {k: np.ascontiguousarray(v[take]) for k, v in p.items()}


def cases(gs4d, form, n):
    """(name, parameters) of the clean and the hostile set of n rows"""
    return (("clean", clean(gs4d, form, n, seed=0x4252 + n)), ("hostile", resized(hostile(gs4d, form), n)))


def host_records(gs4d, form, p):
    """the definition: the host builders (host/gs4d_host.cpp)"""
    if form == "3d":
        return gs4d.build_records_3d(p["pos"], p["rot"], p["scale"], p["rgba"])
    if form == "4d_vel":
        return gs4d.build_records_4d_tvar(p["pos"], p["rot"], p["scale"], p["dir"], p["tvar"], p["rgba"])
    return gs4d.build_records_4d_2q(p["pos"], p["rot"], p["rot_r"], p["scale"], p["rgba"])


def picture_time(form):
    """a 3D record has mu_t = 0 and Sigma44 = 1: it shows at time 0 only"""
    return 0.0 if form == "3d" else T


def picture_set(gs4d, form, n=300, seed=0x4254):
    """a clean set in front of the camera of the picture tests ((0, 0, 150) looking down -z): a cloud of 80 units with splats of some size, alive at T"""
    rng = np.random.default_rng([seed, FORMS.index(form)])
    p = clean(gs4d, form, n, seed)
    p["pos"][:, :3] = rng.uniform(-40.0, 40.0, (n, 3)).astype(f32)
    p["scale"][:, :3] = rng.uniform(4.0, 16.0, (n, 3)).astype(f32)
    p["rgba"][:, 3] = rng.uniform(0.3, 1.0, n).astype(f32)
    if form != "3d":
        p["pos"][:, 3] = (T + rng.uniform(-0.5, 0.5, n)).astype(f32)
    if form == "4d_vel":
        p["tvar"] = gs4d.time_variance(rng.uniform(2.0, 8.0, n).astype(f32), f32(0.5)).reshape(n, 1)
    if form == "4d_2q":
        p["scale"][:, 3] = rng.uniform(2.0, 8.0, n).astype(f32)
    return p

"""Inputs for the gs4d_transform_selected tests (include/gs4d.h): sizes, selection tables, pivot forms, measurements, and the definition
restated as a numpy float32 loop of the header's text.

Test infrastructure only (tests/test_xfsel_host.py pins the restatement against gs4d_host_transform_selected on the CPU; tests/test_gpu_transform_selected.py
runs the device call against it).  Record sets and transform rows are those of tests/transform_cases.py, the table builders those of tests/edit_cases.py.

The kernel gives one workgroup of TILE threads a tile of TILE records, waves of 64 inside it, and a workgroup in which nothing is selected writes
nothing; a wave with fewer than STAGE_MIN selected records stores them thread by thread, a fuller one stages them in LDS: SIZES hits the edges of a
wave and of a tile, and the tables hold tiles and waves that are full, empty, hold one record, and hold STAGE_MIN - 1 and STAGE_MIN records.
"""
import ctypes

import numpy as np

import edit_cases as ec
import transform_cases as tc

f32, f64 = np.float32, np.float64
TILE = 256                                                   # XFSEL_TILE (csrc/gs4d_internal.h)
STAGE_MIN = 8                                                # XFSEL_STAGE_MIN (csrc/transform_selected.hip)
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1)      # one record, either side of a wave and of a tile, three tiles plus one
EXTRA = 3                                                    # records behind n that no call may touch
SETS = tc.SETS
PIVOT = (1.5, -2.25, 40.0)
PIVOT_FORMS = ("none", "explicit", "measure", "count0", "hostile")
WIDE = (5, 0x3B808081, ec.WSUM_MIN)                          # every field has a threshold, the wsum one above 2^32
bits, same_bits = tc.bits, tc.same_bits


# ---- the selection ------------------------------------------------------------------------------------------------------------------------------
def masks(n):
    """name -> bool [n]"""
    i = np.arange(n)
    tile, slot = i // TILE, i % TILE
    out = {"all": np.ones(n, bool), "none_selected": np.zeros(n, bool), "alternating": i % 2 == 0,
           "one_per_tile": slot == np.minimum((37 * tile + 5) % TILE, n - 1 - tile * TILE),
           "first": i == 0, "last": i == n - 1,
           # 7 selected records in the even waves, 8 in the odd ones: either side of the count from which a wave stages its stores (XFSEL_STAGE_MIN)
           "at_the_staging_threshold": (i % 64 % 9 == 0) & (i % 64 < 9 * (7 + i // 64 % 2))}
    if n > 2 * TILE:
        out["a_tile_unselected"] = tile != 1                 # a whole tile that is not selected between two that are
    return out


def tables(n):
    """name -> (STAT table of n rows or None, rule, invert): no table, every mask of masks(n), and each of them under GS4D_KEEP_INVERT"""
    out = {"no_table": (None, (1, 0, 0), False)}
    for k, (name, m) in enumerate(masks(n).items()):
        rule = WIDE if k % 2 else (1, 0, 0)
        if m.all():
            rule = (1, 0, 0)
        st = ec.mask_table(m, rule)
        assert np.array_equal(ec.selected(n, st, rule), m)
        out[name] = (st, rule, False)
        out[name + "_inverted"] = (st, rule, True)
    return out


def selected(n, table):
    st, rule, invert = table
    return ec.selected(n, st, rule, invert)


def keywords(table):
    """the stats= and rule keywords of transform_selected_host for a table (the device call takes a buffer for stats)"""
    st, rule, invert = table
    return {} if st is None else dict(stats=st, **ec.rule_keywords(rule, invert))


# ---- measurements -------------------------------------------------------------------------------------------------------------------------------
def measure_of(gs4d, count=0, lo=(0, 0, 0), hi=(0, 0, 0), cell_sum=(0, 0, 0), **other):
    m = gs4d.Measure()
    m.count = count
    m.lo[:], m.hi[:] = [float(f32(v)) for v in lo], [float(f32(v)) for v in hi]
    m.cell_sum[:] = [int(v) for v in cell_sum]
    for k, v in other.items():
        setattr(m, k, v)
    return m


def hostile_measures(gs4d):
    """measurements no gs4d_measure_records call writes: NaN and infinite ends, a cell_sum that is huge, count 0 beside garbage"""
    inf, nan, big = np.inf, np.nan, (1 << 63) + 12345
    return [measure_of(gs4d, 3, (nan, -1.0, 2.0), (1.0, inf, 2.0), (1 << 20, 1 << 21, 0)),
            measure_of(gs4d, 1, (-inf, -3e38, 1e-40), (inf, 3e38, -1e-40), (5, 1 << 20, 1 << 19)),
            measure_of(gs4d, 0xFFFFFFFF, (-5.0, 0.0, 7.0), (9.0, 1e30, 7.5), (big, (1 << 64) - 1, (1 << 52) + 1)),
            measure_of(gs4d, 7, (1.0, 2.0, 3.0), (-1.0, 2.0, -0.0), (3 << 20, 7 << 20, 1))]


def count0_measure(gs4d):
    """count == 0 beside fields that would give something else: the centre is (0, 0, 0)"""
    return measure_of(gs4d, 0, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0), (1 << 20, 1 << 20, 1 << 20), unplaced=4, skipped=2)


def measure_bytes(m):
    return np.frombuffer(bytes(m), np.uint8).copy()


def centre_by_the_text(m):
    """the header's line in numpy float64, one operation at a time, rounded to float32; count == 0: zeros"""
    if m.count == 0:
        return np.zeros(3, f32)
    lo, hi = np.array(m.lo[:], f32).astype(f64), np.array(m.hi[:], f32).astype(f64)
    with np.errstate(all="ignore"):
        cells = f64(m.count) * f64(1048576.0)
        frac = np.array(m.cell_sum[:], np.uint64).astype(f64) / cells
        return (lo + (hi - lo) * frac).astype(f32)


def pivot_case(gs4d, form, rec, n, table, k=0):
    """(pivot 3-tuple or None, Measure or None) of a pivot form for the selection `table` of the first n records of rec"""
    if form == "none":
        return None, None
    if form == "explicit":
        return PIVOT, None
    if form == "measure":
        return None, gs4d.measure_records_host(rec[:n], t=0.25, **keywords(table))
    if form == "count0":
        return None, count0_measure(gs4d)
    h = hostile_measures(gs4d)
    return None, h[k % len(h)]


# ---- the definition, restated -------------------------------------------------------------------------------------------------------------------
def by_the_text(rec, xf, sel, c=None, n=None):
    """the header's text in numpy float32, one operation at a time: a copy of rec [total, 24] whose first n records (default: all) are, where sel,
    themselves under the row xf (20 floats) about the pivot c (3 floats; None: no pivot)"""
    rec, xf = np.ascontiguousarray(rec, f32).reshape(-1, 24), np.ascontiguousarray(xf, f32).reshape(20)
    n = rec.shape[0] if n is None else n
    l, o = [f32(v) for v in xf[:16]], [f32(v) for v in xf[16:]]
    new = np.array(rec[:n], copy=True)
    with np.errstate(all="ignore"):
        q = [rec[:n, k] for k in range(4)]
        if c is not None:
            c = [f32(v) for v in np.asarray(c, f32)]
            q[:3] = [q[a] - c[a] for a in range(3)]
        for r in range(4):
            u = ((((l[r] * q[0]) + (l[4 + r] * q[1])) + (l[8 + r] * q[2])) + (l[12 + r] * q[3])) + o[r]
            new[:, r] = u + c[r] if c is not None and r < 3 else u
        S = [[rec[:n, 8 + 4 * col + k] for k in range(4)] for col in range(4)]
        T = [[(((l[r] * S[col][0]) + (l[4 + r] * S[col][1])) + (l[8 + r] * S[col][2])) + (l[12 + r] * S[col][3]) for r in range(4)] for col in range(4)]
        for col in range(4):
            for r in range(4):
                new[:, 8 + 4 * col + r] = (((T[0][r] * l[col]) + (T[1][r] * l[4 + col])) + (T[2][r] * l[8 + col])) + (T[3][r] * l[12 + col])
    assert new.dtype == f32
    out = np.array(rec, copy=True)
    out[:n][sel] = new[sel]
    return out


def expected(gs4d, rec, xf, n, table, pivot, measure):
    """what a call leaves in the records [total, 24], from the restatement"""
    c = pivot if pivot is not None else centre_by_the_text(measure) if measure is not None else None
    return by_the_text(rec, xf, selected(n, table), c, n)


def assert_records(got, want, rec, sel, n, what):
    """got against want under the NaN rule for the selected records, and byte for byte against the input everywhere else"""
    got, want = np.ascontiguousarray(got, f32).reshape(-1, 24), np.ascontiguousarray(want, f32).reshape(-1, 24)
    ok = same_bits(got, want)
    assert ok.all(), f"{what}: {int((~ok).any(1).sum())} records differ from the restatement, first word at {np.argwhere(~ok)[0].tolist()}"
    keep = np.ones(got.shape[0], bool)
    keep[:n] = ~sel
    assert np.array_equal(bits(got[keep]), bits(rec[keep])), f"{what}: a record that is not selected, or one behind n, changed"


def sizeof_selection_xf(gs4d):
    return ctypes.sizeof(gs4d.SelectionXf)

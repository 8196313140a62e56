"""gs4d_count_ids (include/gs4d.h) restated in numpy, and the scenes, rectangles, tables and masks of its tests.

Test infrastructure only (tests/test_select_host.py pins it on the CPU, tests/test_gpu_select.py runs it).  The bar is restate(): np.add.at /
np.maximum.at over the pixels that take part, which shares nothing with the kernel's ballots, shuffles and carries.  An integer problem: every
comparison is exact.  The planes a GPU test restates are the ones it reads back itself (gs4d_read_ids of the same frame).

Sizes: a wave of the kernel reads row segments of 64 pixels, WAVE_ROWS rows of one column band, a workgroup 64 x GROUP_ROWS pixels (SEL_* in
csrc/select.hip).  The images are no multiple of either and wider and taller than one workgroup's share, so a launch has partial waves, partial
batches and more than one workgroup each way.
"""
import numpy as np

import compact_cases as cc
import stats_cases as sc

ID_NONE = 0xFFFFFFFF
STAT = cc.STAT                                            # wmax as its bit pattern
WAVE_COLS, WAVE_ROWS, GROUP_ROWS = 64, 16, 64             # SEL_WAVE_ROWS, SEL_GROUP_ROWS
W, H = 101, 70                                            # the image of the scenes made here
SENTINEL = 0xA5
EVERY_DRAW = (0, 0xFFFFFFFF)


def region(x, y, w, h, draws=EVERY_DRAW, min_weight=0):
    """the fields of gs4d_id_region but `reserved`: x, y, w, h, draw_first, draw_last, min_weight (a uint32 bit pattern)"""
    return (int(x), int(y), int(w), int(h), int(draws[0]), int(draws[1]), int(min_weight))


def weight_bits(w):
    return int(np.array([w], np.float32).view(np.uint32)[0])


def takes_part(record, draw, weight, reg, mask, nrecords):
    """(h, w) bool over the rectangle: the five conditions of gs4d.h.  record, draw: (H, W) uint32; weight: (H, W) float32 (or its bit
    patterns as uint32); mask: None or (h, w) bytes"""
    x, y, w, h, d0, d1, mw = reg
    rec = np.asarray(record, np.uint32)[y:y + h, x:x + w]
    drw = np.asarray(draw, np.uint32)[y:y + h, x:x + w]
    wb = np.ascontiguousarray(weight).view(np.uint32)[y:y + h, x:x + w]
    on = (rec != np.uint32(ID_NONE)) & (rec.astype(np.uint64) < np.uint64(nrecords)) & (drw >= np.uint32(d0)) & (drw <= np.uint32(d1)) & (wb >= np.uint32(mw))
    if mask is not None:
        on &= np.asarray(mask).reshape(h, w) != 0
    return on, rec, wb


def restate(record, draw, weight, reg, mask, table_in, nrecords):
    """-> the table after gs4d_count_ids(reg, mask, table, nrecords) on a table that held table_in (STAT rows, at least nrecords of them)"""
    out = np.array(table_in, STAT)
    on, rec, wb = takes_part(record, draw, weight, reg, mask, nrecords)
    r = rec[on].astype(np.int64)
    b = wb[on]
    q = sc.quantise(b.view(np.float32))                    # (uint32) rint(w * 2^24), the product in float32
    pixels, wmax, wsum = out["pixels"].copy(), out["wmax"].copy(), out["wsum"].copy()
    np.add.at(pixels, r, np.uint32(1))
    np.maximum.at(wmax, r, b)
    np.add.at(wsum, r, q.astype(np.uint64))
    out["pixels"], out["wmax"], out["wsum"] = pixels, wmax, wsum
    return out


def add_tables(a, b):
    """the sum of two calls: pixels and wsum by +, wmax by max"""
    out = np.array(a, STAT)
    out["pixels"] = a["pixels"] + b["pixels"]
    out["wmax"] = np.maximum(a["wmax"], b["wmax"])
    out["wsum"] = a["wsum"] + b["wsum"]
    return out


# ---- rectangles, tables, masks -------------------------------------------------------------------------------------------------------------------
def rectangles(w, h):
    """name -> (x, y, w, h) inside a w x h image wider than one wave segment and taller than one wave's rows"""
    assert w > WAVE_COLS + 8 and h > WAVE_ROWS + 8
    return {
        "full": (0, 0, w, h),
        "corner00": (0, 0, 1, 1), "corner10": (w - 1, 0, 1, 1), "corner01": (0, h - 1, 1, 1), "corner11": (w - 1, h - 1, 1, 1),
        "row": (0, h // 2, w, 1),
        "column": (w // 3, 0, 1, h),
        # odd offset, odd size; 67 columns from column 3 (a full wave segment and a partial one), 37 rows from row 5 (two whole waves' rows and a partial batch)
        "straddle": (3, 5, min(67, w - 3), min(37, h - 5)),
    }


TABLES = ("zero", "filled")
TAIL_ROWS = 8                                              # sentinel rows behind the n rows of a table buffer


def table(kind, n, name=""):
    """n STAT rows: all zero, or non-zero everywhere — a third of the wmax above every weight a plane can hold (w <= 1), wsum beyond 32 bits"""
    t = np.zeros(n, STAT)
    if kind == "filled":
        rng = np.random.default_rng(cc.seed("select/table/" + name))
        t["pixels"] = rng.integers(1, 1 << 31, n)
        t["wmax"] = np.where(np.arange(n) % 3 == 0, np.uint32(weight_bits(1.5)), rng.uniform(1e-6, 0.5, n).astype(np.float32).view(np.uint32))
        t["wsum"] = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    else:
        assert kind == "zero"
    return t


def table_bytes(t):
    """what a table buffer holds: the rows, then TAIL_ROWS rows of sentinel bytes"""
    return np.concatenate([np.ascontiguousarray(t).view(np.uint8), np.full(TAIL_ROWS * STAT.itemsize, SENTINEL, np.uint8)])


MASKS = ("zeros", "ones", "checker", "random")


def mask(kind, w, h):
    """(h, w) bytes: all zero, all 0xFF, a checkerboard of 0 and 1, random bytes from {0, 1, 0x80}"""
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "ones":
        return np.full((h, w), 0xFF, np.uint8)
    if kind == "checker":
        return ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2).astype(np.uint8)
    assert kind == "random"
    return np.random.default_rng(cc.seed(f"select/mask/{w}x{h}")).choice(np.array([0, 1, 0x80], np.uint8), (h, w))


# ---- scenes: 96-byte records for GS4D_MODE_4D_DIRECT, by stats_cases' pixel placement --------------------------------------------------------------
SCENES = ("one", "grid", "layered", "clear")


GRID_STEP, GRID_SCALE = 4.3, 2.0                          # pixels between the centres; stats_cases' scale unit: records about three pixels wide


def grid_params():
    """px, py, z, s, rgba of the grid scene: a record every GRID_STEP pixels, each its own depth and colour, alphas in [0.05, 1]"""
    rng = np.random.default_rng(11)
    gx, gy = np.meshgrid(np.arange(2.0, W - 1.0, GRID_STEP), np.arange(2.0, H - 1.0, GRID_STEP))
    px, py = gx.ravel(), gy.ravel()
    n = px.size
    rgba = np.concatenate([rng.uniform(0.0, 1.0, (n, 3)), rng.uniform(0.05, 1.0, (n, 1))], 1)
    return px, py, rng.uniform(-5.0, 5.0, n), np.full(n, GRID_SCALE), rgba


def scene(gs4d, name):
    """-> (W, H, records).  one: a single record whose footprint holds the whole image with cg >= 1e-4 — every lane of every wave the same
    record; grid: records a few pixels wide on a grid (grid_params), so neighbouring lanes differ and pixels between them hold the sentinel; layered:
    stats_cases' `overlap` (96 x 96, records over each other and over the edges); clear: the grid's records, which the test does not draw."""
    if name == "one":
        rec = sc.records(gs4d, W, H, [W / 2.0], [H / 2.0], [0.0], [400.0], [[0.9, 0.4, 0.1, 0.9]])
        return W, H, rec
    if name in ("grid", "clear"):
        return W, H, sc.records(gs4d, W, H, *grid_params())
    assert name == "layered"
    w, h, params = sc.layered("overlap")
    return w, h, sc.records(gs4d, w, h, *params)

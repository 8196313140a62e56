"""Scenes for tests/test_gpu_staged_misses.py, and the host's guesses for staged tile lists recomputed from projected records.

A staged draw (csrc/preprocess.hip, k_project_count<SRC, Stage, ..>; csrc/tilelist.hip, k_bucket_tiles_staged) runs on guesses the host made from the
statistics of earlier draws of the same scene (csrc/gs4d_api.hip, run_draw / resolve_lane):

* scap       entries a segment block holds: the fullest segment + an eighth + 64, rounded up to 64;
* bcap       entries a bucket (tile % nb) holds: the fullest bucket + an eighth + 512, rounded up to 64;
* list hint  the compositor's list capacity: shrinks to v2_list_capacity(longest + longest / 8) after 8 draws whose lists were that short;
* box        the blocks of 4 x 4 tiles the last staged draw had entries in, stage_box_margin (1) blocks wider on every side.

Every scene is a set of small fixed splats facing the camera plus a few MOVERS: 4D records that lie far outside the image at T0 and arrive
on chosen tiles at T1 through their velocity.  Against the guesses that frames at T0 teach, the T1 frame crosses exactly the guesses its case
names.  `Load` recomputes from the pixel rectangles of the projected records what the device counts — entries per segment, per bucket, per
tile — and `crossed` says which guesses a frame crosses: the tests assert that as their premise, so that a scene that drifts (or a margin
that changes in the product) fails instead of passing without reaching its miss.
"""
import numpy as np

import scenes

W, H = 640, 360
TILE = 8                                  # gs4d_internal.h
TX, TY = W // TILE, H // TILE             # 80 x 45 tiles
NB = 64                                   # buckets (pinned with GS4D_NB): bucket of a tile = tile % NB
SEG_THREADS = 512                         # gs4d_internal.h
STAGE_MAX_SCAP, STAGE_MAX_BCAP = 5120, 32 * 512       # run_draw stages a draw only within these
BOX_BLOCK, STAGE_BOX_MARGIN = 4, 1        # gs4d_internal.h; gs4d_ctx::stage_box_margin before any box miss
LIST_HINT0, V2_MAX_LIST = 256, 1024       # gs4d_ctx::list_hint of a new context; gs4d_internal.h
LADDER = (64, 128, 192, 256, 384, 512, 768, 1024)     # v2_list_capacity

SEG = 2048
N = 8 * SEG                               # 8 segments of 2048 records (tile_lists_plan)
T0, T1, DT = 0.0, 5.0, 0.004              # warm-up time, miss time, step of the frames after the miss (case f)
DIST = 200.0
CAM = ((0.0, 0.0, DIST), (0.0, 0.0, -1.0))
SPEED = 100.0                             # movers: world units per unit of time along x (500 between T0 and T1; the image is 410 wide)
S_SMALL, S_BIG = 1.6, 8.2                 # splat scales: a footprint inside one tile; one of 3 x 3 tiles

# what the miss frame of each case crosses
TARGETS = {"a": {"segment"}, "b": {"segment"}, "c": {"bucket"}, "d": {"list"}, "e": {"segment", "box"}, "f": {"segment"}}


# ---- the host's arithmetic -------------------------------------------------------------------------------------------------------------
def plan(n):
    """(rows, seg) of tile_lists_plan (tilelist.hip): segments of >= 2048 records, at most 1024 of them"""
    rows = min((n + 2047) // 2048, 1024)
    seg = ((n + rows - 1) // rows + SEG_THREADS - 1) // SEG_THREADS * SEG_THREADS
    return (n + seg - 1) // seg, seg


def scap_for(max_seg):
    return (max_seg + max_seg // 8 + 64 + 63) & ~63


def bcap_for(max_bucket):
    return (max_bucket + max_bucket // 8 + 512 + 63) & ~63


def list_capacity(n):
    return next((c for c in LADDER if n <= c), V2_MAX_LIST)


def shrunk_hint(longest):
    return list_capacity(min(V2_MAX_LIST, longest + longest // 8))


# ---- pixel rectangles -> entries ---------------------------------------------------------------------------------------------------------
def rects_from_device(proj16):
    """gs4d_debug_read_projected: the rectangle is (x0 | y0 << 16, x1 | y1 << 16) in floats 10 and 11 (preprocess.hip, emit)"""
    r0 = np.ascontiguousarray(proj16[:, 10]).view(np.uint32).astype(np.int64)
    r1 = np.ascontiguousarray(proj16[:, 11]).view(np.uint32).astype(np.int64)
    return r0 & 0xFFFF, r0 >> 16, r1 & 0xFFFF, r1 >> 16


def rects_from_checker(p, w=W, h=H):
    """the same rectangle from the checker's projected records (oracle_lib.preprocess), in the float32 arithmetic of emit (w, h: the image)"""
    f = np.float32
    cx, cy, hx, hy = (p[k].astype(f) for k in ("cx", "cy", "hx", "hy"))
    mx, my = f(0.01) + f(1e-5) * hx, f(0.01) + f(1e-5) * hy
    x0, x1 = np.maximum(np.ceil(cx - hx - mx - f(0.5)), f(0.0)), np.minimum(np.floor(cx + hx + mx - f(0.5)), f(w - 1))
    y0, y1 = np.maximum(np.ceil(cy - hy - my - f(0.5)), f(0.0)), np.minimum(np.floor(cy + hy + my - f(0.5)), f(h - 1))
    ok = (p["valid"] != 0) & (x0 <= x1) & (y0 <= y1)
    return tuple(np.where(ok, v, e).astype(np.int64) for v, e in ((x0, 1), (y0, 0), (x1, 0), (y1, 0)))


class Load:
    """entries per segment, per bucket and per tile of one frame, its longest list and the box of blocks that hold entries"""

    def __init__(self, rects, w=W, h=H):
        x0, y0, x1, y1 = rects
        TX, TY = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE             # (the module's own image unless told otherwise)
        n = x0.size
        rows, seg = plan(n)
        ok = (x0 <= x1) & (y0 <= y1)
        tx0, ty0 = x0 // TILE, y0 // TILE                                    # tile_rect (gs4d_internal.h)
        wx, wy = np.where(ok, x1 // TILE - tx0 + 1, 0), np.where(ok, y1 // TILE - ty0 + 1, 0)
        self.seg = np.bincount(np.arange(n) // seg, weights=wx * wy, minlength=rows).astype(np.int64)
        tiles = np.zeros(TX * TY, np.int64)
        for dy in range(int(wy.max(initial=0))):
            for dx in range(int(wx.max(initial=0))):
                m = (dx < wx) & (dy < wy)
                tiles += np.bincount((ty0[m] + dy) * TX + tx0[m] + dx, minlength=TX * TY)
        self.tiles = tiles
        self.bucket = np.bincount(np.arange(TX * TY) % NB, weights=tiles, minlength=NB).astype(np.int64)
        self.longest = int(tiles.max())
        used = np.nonzero(tiles)[0]
        bx, by = (used % TX) // BOX_BLOCK, (used // TX) // BOX_BLOCK
        self.box = (int(bx.min()), int(by.min()), int(bx.max()), int(by.max())) if used.size else None

    def __repr__(self):
        return f"Load(segments {self.seg.tolist()}, fullest bucket {self.bucket.max()}, longest list {self.longest}, box {self.box})"


def crossed(warm, frame):
    """the guesses that a staged draw of `frame` crosses when frames like `warm` taught them (the list hint as it stands once it has shrunk,
    the smallest it can be)"""
    scap, bcap, hint = scap_for(int(warm.seg.max())), bcap_for(int(warm.bucket.max())), shrunk_hint(warm.longest)
    assert scap <= STAGE_MAX_SCAP and bcap <= STAGE_MAX_BCAP, (scap, bcap)        # (else the draws would never be staged)
    nbx, nby = (TX + BOX_BLOCK - 1) // BOX_BLOCK, (TY + BOX_BLOCK - 1) // BOX_BLOCK
    m = STAGE_BOX_MARGIN
    bx0, by0, bx1, by1 = max(warm.box[0] - m, 0), max(warm.box[1] - m, 0), min(warm.box[2] + m, nbx - 1), min(warm.box[3] + m, nby - 1)
    out = set()
    if frame.seg.max() > scap:
        out.add("segment")
    if frame.bucket.max() > bcap:
        out.add("bucket")
    if frame.longest > hint:
        assert frame.longest <= V2_MAX_LIST and hint < LIST_HINT0, (frame.longest, hint)      # a capacity that fits, below a new context's
        out.add("list")
    if frame.box is not None and not (bx0 <= frame.box[0] and by0 <= frame.box[1] and frame.box[2] <= bx1 and frame.box[3] <= by1):
        out.add("box")
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def mats(gs4d):
    return gs4d.look_at(CAM[0], CAM[1]), gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)


def build(gs4d, case):
    """the records (N, 24) of the scene of `case` and the times of its miss frame(s)"""
    rng = np.random.default_rng(ord(case))
    _, proj = mats(gs4d)
    tx, ty = np.zeros(N, np.int64), np.zeros(N, np.int64)
    big = np.zeros(N, bool)
    if case in ("a", "b", "e", "f"):
        # 56 large movers at the end of one segment (the last; b: a middle one): 56 * 9 = 504 entries arrive in it — more than the eighth and
        # the 64 entries scap adds, fewer than the 512 that bcap adds — on tiles 4 apart (one more entry on each)
        w = 3 if case == "b" else 7
        mv = np.arange(w * SEG + SEG - 56, (w + 1) * SEG)
        gx, gy = np.meshgrid(np.arange(8), np.arange(7))
        tx[mv], ty[mv] = (48 if case == "e" else 8) + 4 * gx.ravel(), 6 + 5 * gy.ravel()      # e: right of every fixed splat, outside the box
        big[mv] = True
    elif case == "c":
        # 100 small movers at the end of every segment, onto the tiles of bucket 5: 800 entries more in that bucket, none more in any segment
        mv = np.concatenate([np.arange(w * SEG + SEG - 100, (w + 1) * SEG) for w in range(8)])
        dest = np.arange(5, TX * TY, NB)
        dest = dest[np.arange(mv.size) % dest.size]
        tx[mv], ty[mv] = dest % TX, dest // TX
    elif case == "d":
        # 12 small movers at the end of every segment, all onto one tile: a list of ~100 entries, longer than the shrunk hint (64)
        mv = np.concatenate([np.arange(w * SEG + SEG - 12, (w + 1) * SEG) for w in range(8)])
        tx[mv], ty[mv] = 37, 21
    else:
        raise ValueError(case)
    moving = np.zeros(N, bool)
    moving[mv] = True
    # the fixed splats, one tile each, dealt round the image (e: its left half) so that every tile and every bucket gets about as many
    fixed = np.nonzero(~moving)[0]
    cols = TX // 2 if case == "e" else TX
    deal = (np.arange(fixed.size) * 1031) % (cols * TY)
    tx[fixed], ty[fixed] = deal % cols, deal // cols
    jitter = np.where(moving, 0.0, 1.0)[:, None] * rng.uniform(-0.5, 0.5, (N, 2))
    px, py = tx * TILE + TILE / 2 + jitter[:, 0], ty * TILE + TILE / 2 + jitter[:, 1]       # pixel positions (pixel p's centre: p + 0.5)
    z = rng.uniform(-10.0, 10.0, N)
    x = (px * 2.0 / W - 1.0) * (DIST - z) / proj[0]                          # the point of depth DIST - z the camera sees there
    y = (py * 2.0 / H - 1.0) * (DIST - z) / proj[5]
    mu_t = 0.5 * (T0 + T1)
    vel = np.zeros((N, 3))
    vel[moving, 0] = SPEED
    x = x - vel[:, 0] * (T1 - mu_t)                                          # the conditioned mean at time t: position + velocity * (t - mu_t)
    pos4 = np.stack([x, y, z, np.full(N, mu_t)], 1).astype(np.float32)
    q = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (N, 1))
    s = np.where(big, S_BIG, S_SMALL).astype(np.float32)
    rgba = np.concatenate([rng.uniform(0.0, 1.0, (N, 3)), rng.uniform(0.3, 0.9, (N, 1))], 1).astype(np.float32)
    life = np.full(N, 20.0, np.float32)                                       # opacity between T0 and T1: exp(-0.5 dt^2 ln 4 / 20^2) > 0.98
    rec = gs4d.build_records_4d(pos4, q, np.stack([s, s, s], 1), life, np.full(N, 0.5, np.float32), vel.astype(np.float32), rgba)
    times = [T1 + DT * k for k in range(8)] if case == "f" else [T1]
    return rec, times

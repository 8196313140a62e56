"""ID outputs restated in numpy: for one draw, per pixel, the fragment with the largest weight w = T * al.

Test infrastructure only (tests/test_ids_host.py, tests/test_gpu_ids.py).  The compositor's rules, in float32 and in its order of
operations (composite_common.h):
  - coverage: dx = (i + 0.5) - cx, dy = (j + 0.5) - cy, u = fma(a0x, dx, a0y * dy), v = fma(a1x, dx, a1y * dy), |u| <= 0.5 and |v| <= 0.5;
  - cg = exp(-32 (u^2 + v^2)); al = clamp(alpha * cg, 0, 1) if cg >= 1e-4 else 0;
  - front to back: w = T * al, C += w * c, T *= (1 - al); the candidate is the first fragment whose w beats every earlier one (w > best).
The device evaluates exp with v_exp_f32 and may contract u * u + v * v into an FMA: a few ulp apart from numpy.  Pixels whose two best
candidates lie within TIE_REL of each other may therefore pick either: they are returned as a mask, with both records.
"""
import numpy as np

ID_NONE = 0xFFFFFFFF
TIE_REL = 1e-5
F = np.float32


def _fma(a, b, c):
    """fused multiply-add of float32 operands, rounded once (float64 holds the product exactly)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def from_device(pj):
    """the device's projected records (Context.debug_projected: 16 floats each) as the fields the restatement reads"""
    out = np.zeros(pj.shape[0], [("cx", "f4"), ("cy", "f4"), ("a0x", "f4"), ("a0y", "f4"), ("a1x", "f4"), ("a1y", "f4"), ("alpha", "f4"),
                                 ("r", "f4"), ("g", "f4"), ("b", "f4"), ("hx", "f4"), ("hy", "f4"), ("valid", "u4")])
    for k, f in enumerate(("cx", "cy", "a0x", "a0y", "a1x", "a1y", "alpha", "r", "g", "b")):
        out[f] = pj[:, k]
    out["hx"], out["hy"] = pj[:, 12], pj[:, 13]
    out["valid"] = (pj[:, 14] != 0).astype(np.uint32)
    return out


def restate(proj, order, W, H, premult=False, clamp_rgb=True):
    """One draw of the records `proj` (fields cx, cy, a0x, a0y, a1x, a1y, alpha, r, g, b, hx, hy, valid) in instance order `order`
    (None: record k at instance k).  Returns a dict of (H, W) arrays, row 0 at the bottom:
      record (u32, ID_NONE where no fragment has w > 0), weight (f32), T (final transmittance), rgb (H, W, 3: sum of w * c),
      tie (bool: the two best candidates within TIE_REL), second (u32: the runner-up's record, ID_NONE if none),
      fragile (bool: a covering fragment's cg lies within TIE_REL of the 1e-4 discard, where an ulp decides whether it blends at all)."""
    n = proj.shape[0] if order is None else len(order)
    seq = np.arange(n, dtype=np.int64) if order is None else np.asarray(order, np.int64)
    T = np.ones((H, W), F)
    C = np.zeros((H, W, 3), F)
    bw = np.zeros((H, W), F)
    sw = np.zeros((H, W), F)
    br = np.full((H, W), ID_NONE, np.uint32)
    sr = np.full((H, W), ID_NONE, np.uint32)
    fragile = np.zeros((H, W), bool)
    for k in range(n - 1, -1, -1):                    # front to back: the last instance is blended first
        rec = int(seq[k])
        if rec >= proj.shape[0]:
            continue
        p = proj[rec]
        if not p["valid"]:
            continue
        cx, cy, hx, hy = F(p["cx"]), F(p["cy"]), F(p["hx"]), F(p["hy"])
        i0, i1 = max(0, int(np.floor(cx - hx - F(1.5)))), min(W - 1, int(np.ceil(cx + hx + F(1.5))))
        j0, j1 = max(0, int(np.floor(cy - hy - F(1.5)))), min(H - 1, int(np.ceil(cy + hy + F(1.5))))
        if i0 > i1 or j0 > j1:
            continue
        fx = np.arange(i0, i1 + 1, dtype=F) + F(0.5)
        fy = np.arange(j0, j1 + 1, dtype=F) + F(0.5)
        dx = (fx - cx)[None, :]
        dy = (fy - cy)[:, None]
        dx, dy = np.broadcast_arrays(dx, dy)
        u = _fma(np.full_like(dx, p["a0x"]), dx, F(p["a0y"]) * dy)
        v = _fma(np.full_like(dx, p["a1x"]), dx, F(p["a1y"]) * dy)
        cov = (np.abs(u) <= F(0.5)) & (np.abs(v) <= F(0.5))
        if not cov.any():
            continue
        cg = np.exp2((u * u + v * v) * F(-46.16624130844683)).astype(F)
        al = np.where(cov & (cg >= F(0.0001)), np.clip(F(p["alpha"]) * cg, F(0.0), F(1.0)), F(0.0)).astype(F)
        sl = (slice(j0, j1 + 1), slice(i0, i1 + 1))
        fragile[sl] |= cov & (np.abs(cg - F(0.0001)) <= F(TIE_REL * 0.0001))
        t = T[sl]
        w = (t * al).astype(F)
        c = np.array([p["r"], p["g"], p["b"]], F)
        if premult:
            col = np.clip(c[None, None, :] * cg[..., None], F(0.0), F(1.0))
        else:
            col = np.broadcast_to(np.clip(c, F(0.0), F(1.0)) if clamp_rgb else c, w.shape + (3,))
        C[sl] = C[sl] + w[..., None] * col
        b, s = bw[sl], sw[sl]
        take = w > b
        second = ~take & (w > s)
        sr[sl] = np.where(take, br[sl], np.where(second, rec, sr[sl]))
        sw[sl] = np.where(take, b, np.where(second, w, s))
        br[sl] = np.where(take, rec, br[sl])
        bw[sl] = np.where(take, w, b)
        T[sl] = (t * (F(1.0) - al)).astype(F)
    tie = (sw > 0) & (bw - sw <= F(TIE_REL) * bw)
    return {"record": br, "weight": bw, "T": T, "rgb": C, "tie": tie, "second": sr, "fragile": fragile}


def over(T_new, cand_rec, cand_w, draw_ord, old):
    """The draw's candidate composed over the stored planes old = (record, draw, weight): DESIGN.md §4's rule, float32."""
    rec0, drw0, w0 = old
    w0 = (T_new * w0).astype(F)
    take = (cand_w > 0) & (cand_w >= w0)
    return (np.where(take, cand_rec, rec0).astype(np.uint32), np.where(take, np.uint32(draw_ord), drw0).astype(np.uint32),
            np.where(take, cand_w, w0).astype(F))


def sentinel(H, W):
    return np.full((H, W), ID_NONE, np.uint32), np.full((H, W), ID_NONE, np.uint32), np.zeros((H, W), F)

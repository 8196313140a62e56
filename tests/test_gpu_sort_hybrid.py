"""GPU parity of the depth sort's MSD/LSD hybrid (csrc/sort.hip: k_os_pass on the 9-bit top digit, then k_os_tail), through the C ABI.

The hybrid is planned from the key span the host proves from the records' bounding box, so every case here is a record set: record i lies on
the x axis at distance 1 / key_i from a camera at the origin, and two records BEHIND the n keyed ones pin the box — hence bias and span — to the
case's range whatever the keyed keys are (the box covers the whole buffer).  Keys are what oracle.keygen computes from the records, never the
targets they were built from.

Bar: keys AND permutation equal, element for element, both checkers (oracle.sort_pairs(..., "std") and numpy's stable argsort); no tolerance.
The image of the fused frame: the suite's TOL against the CPU renderer, and bit-equal to the frame of GS4D_SORT_HYBRID=0.
Every case asserts through Context.sort_stats() that the path it is about really ran.  GS4D_SORT_HYBRID=1 lets the small sizes take the hybrid.
"""
import numpy as np
import pytest

import scenes
import sort_cases as sc
from hybrid_cases import CAM0, KEY_LO, _records, _proven, _uniform, _crowded      # the record sets: shared with test_gpu_sort_hybrid_edges.py
from test_gpu_paths import _ctx
from test_gpu_render import cam_mats, linf, TOL

pytestmark = pytest.mark.gpu

SPAN24 = (1 << 24) - (1 << 19)                              # a 24-bit span: three 8-bit LSD passes, top digit = bits 15..23 of (key - bias)
TAIL_TILE = 8192                                            # k_os_tail's LDS tile (OT_TILE)


class _Set:
    """one record set on one context: the buffers, the expected sort (computed once), and sort() = keygen + sort + read + check"""

    def __init__(self, ctx, gs4d, oracle, key_bits, span=SPAN24):
        self.ctx, self.n = ctx, len(key_bits)
        rec = _records(gs4d, key_bits, span)
        self.bias, self.bits = _proven(gs4d, rec)
        _, ek = oracle.keygen(rec[:self.n], 0.0, np.array(CAM0, np.float32))
        self.keys = ek.view(np.uint32)
        assert self.keys.min() >= self.bias and int(self.keys.max() - self.bias).bit_length() <= self.bits
        ident = np.arange(self.n, dtype=np.uint32)
        self.want = sc.reference(self.keys, ident)
        sk, sv = oracle.sort_pairs(self.keys, ident, "std")
        assert np.array_equal(sk, self.want[0]) and np.array_equal(sv, self.want[1])      # the two checkers agree
        self.db, self.kb, self.ib = ctx.buffer(rec), ctx.buffer(nbytes=4 * self.n), ctx.buffer(nbytes=4 * self.n)

    def top_counts(self):
        return np.bincount((self.keys - np.uint32(self.bias)) >> np.uint32(self.bits - 9), minlength=512)

    def sort(self):
        """-> the change of the sort statistics over this one sort"""
        ctx, n = self.ctx, self.n
        before = ctx.sort_stats()
        ctx.keygen(self.db, 0.0, CAM0, self.kb, self.ib, n)
        ctx.sort_pairs(self.kb, self.ib, n)
        k, v = ctx.read(self.kb, np.uint32, n), ctx.read(self.ib, np.uint32, n)
        after = ctx.sort_stats()
        for what, got, want in (("keys", k, self.want[0]), ("permutation", v, self.want[1])):
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{what}: {bad.size} of {n} slots differ, the first at {int(bad[0])}: got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x}"
        return {"hybrid": after["hybrid_sorts"] - before["hybrid_sorts"], "launches": after["sort_launches"] - before["sort_launches"],
                "largest": after["largest_bucket"], "slow": after["slow_buckets"]}


def _hybrid_ctx(gs4d, monkeypatch, **env):
    monkeypatch.delenv("GS4D_SORT_TAILCAP", raising=False)
    return _ctx(gs4d, 64, 64, monkeypatch, GS4D_SORT_HYBRID=1, **env)


@pytest.mark.parametrize("n,bits", [(50003, 24), (200003, 24), (50003, 26)])
def test_uniform_keys_above_a_bias(gs4d, oracle, monkeypatch, n, bits):
    """Sizes that are a multiple of no tile; every bucket is a few hundred keys and is finished in LDS.  24 bits: local digits of 8 + 7 bits
    (k_os_tail<256>); 26 bits: 9 + 8 (k_os_tail<512>, three 9-bit passes in the LSD plan)."""
    span = SPAN24 if bits == 24 else (1 << 26) - (1 << 21)
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        s = _Set(ctx, gs4d, oracle, _uniform(n, span, n + bits), span=span)
        assert s.bits == bits
        d = s.sort()
        assert d["hybrid"] == 1 and d["launches"] == 2 and d["slow"] == 0
        assert d["largest"] == s.top_counts().max() <= TAIL_TILE
        assert ctx.stats()["depth_sort_passes"] == 3               # still the digit passes of the LSD plan
        ctx.finish()
    finally:
        ctx.close()


def test_ties_stay_in_the_callers_order(gs4d, oracle, monkeypatch):
    """300 distinct key values over 120,000 keys."""
    n = 120000
    rng = np.random.default_rng(300)
    pool = np.unique(_uniform(400, SPAN24, 301))[:300]
    assert pool.size == 300
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        s = _Set(ctx, gs4d, oracle, pool[rng.integers(0, 300, n)])
        assert np.unique(s.keys).size <= 300
        d = s.sort()
        assert d["hybrid"] == 1 and d["slow"] == 0 and d["largest"] == s.top_counts().max()
        ctx.finish()
    finally:
        ctx.close()


def test_one_crowded_bucket_takes_the_slow_path(gs4d, oracle, monkeypatch):
    """40 % of 60,000 keys share one top digit; with a capacity of 2048 that bucket runs three chunks through global memory, twice, while every
    other bucket is finished in LDS."""
    n = 60000
    keys, m = _crowded(n, 0.4, 3)
    ctx = _hybrid_ctx(gs4d, monkeypatch, GS4D_SORT_TAILCAP=2048)
    try:
        s = _Set(ctx, gs4d, oracle, keys)
        tc = s.top_counts()
        assert s.bits == 24 and tc.max() >= m > 2 * TAIL_TILE and np.count_nonzero(tc > 2048) == 1
        d = s.sort()
        assert d["hybrid"] == 1 and d["slow"] == 1 and d["largest"] == tc.max()
        ctx.finish()
    finally:
        ctx.close()


def test_all_keys_equal(gs4d, oracle, monkeypatch):
    """One bucket, on the slow path (10,000 keys against a capacity of 2048): the output is the input."""
    n = 10000
    ctx = _hybrid_ctx(gs4d, monkeypatch, GS4D_SORT_TAILCAP=2048)
    try:
        s = _Set(ctx, gs4d, oracle, np.full(n, KEY_LO + (123 << 15) + 4567, np.uint32))
        assert s.bits == 24 and np.unique(s.keys).size == 1
        d = s.sort()
        assert d["hybrid"] == 1 and d["slow"] == 1 and d["largest"] == n
        ctx.finish()
    finally:
        ctx.close()


def test_top_digits_partly_used(gs4d, oracle, monkeypatch):
    """A span of 66 % of 2^24, as the headline scene's: the upper third of the top digits is empty, the last used bucket ends at n."""
    n, span = 70001, int(0.66 * (1 << 24))
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        s = _Set(ctx, gs4d, oracle, _uniform(n, span, 66), span=span)
        tc = s.top_counts()
        assert s.bits == 24 and 300 < np.count_nonzero(tc) < 345 and tc[345:].sum() == 0
        d = s.sort()
        assert d["hybrid"] == 1 and d["slow"] == 0 and d["largest"] == tc.max()
        ctx.finish()
    finally:
        ctx.close()


def _fused_frames(gs4d, monkeypatch, rec, cam, view, proj, W, H, t, hybrid):
    """two frames keygen -> sort -> draw with nothing read in between (the draw's projection generates the keys): [(keys, permutation, image)], statistics"""
    n = rec.shape[0]
    monkeypatch.delenv("GS4D_SORT_TAILCAP", raising=False)
    ctx = _ctx(gs4d, W, H, monkeypatch, GS4D_SORT_HYBRID=hybrid)
    try:
        db, kb, ib = ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        out = []
        for _ in range(2):
            ctx.clear()
            ctx.set_uniforms(time=t, min_opacity=0.0, view=view, proj=proj)
            ctx.keygen(db, t, cam[0], kb, ib, n)
            ctx.sort_pairs(kb, ib, n)
            ctx.set_mode(gs4d.MODE_4D_SORTED)
            ctx.bind(1, ib)
            ctx.bind(2, db)
            ctx.draw_instanced(n)
            img = ctx.read_pixels()
            out.append((ctx.read(kb, np.uint32, n), ctx.read(ib, np.uint32, n), img))
        st, ss = ctx.stats(), ctx.sort_stats()
        ctx.finish()
        return out, st, ss
    finally:
        ctx.close()


def test_fused_frame_path(gs4d, oracle, monkeypatch):
    """cube_params_4d(30000) through keygen -> sort -> draw, twice (the two histogram slots): the projection kernel counts the top-digit row alone.
    Seen from three times CAM_CUBE's distance at t = 25, the camera is outside the box the records can reach, and the proven span is 24 bits
    (from CAM_CUBE itself the box holds the camera and the span is open-ended: no hybrid); the splats are 30 times their size to cover pixels."""
    n, W, H, t = 30000, 320, 180, 25.0
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)
    rec = gs4d.build_records_4d(pos4, q, scale * 30.0, life, fade, vel, rgba)
    cam = (tuple(3.0 * v for v in scenes.CAM_CUBE[0]), scenes.CAM_CUBE[1])
    view, proj = cam_mats(gs4d, cam, W, H)
    _, ek = oracle.keygen(rec, t, np.array(cam[0], np.float32))
    ek = ek.view(np.uint32)
    esk, eperm = sc.reference(ek, np.arange(n, dtype=np.uint32))
    sk2, sv2 = oracle.sort_pairs(ek, np.arange(n, dtype=np.uint32), "std")
    assert np.array_equal(sk2, esk) and np.array_equal(sv2, eperm)
    eimg, _, _ = oracle.render_4d(rec, True, t, 0.0, cam[0], view, proj, W, H)
    assert float(np.abs(eimg - np.array(gs4d.CLEAR_COLOR, np.float32)).max()) > 0.05, "empty frame"
    new, st, ss = _fused_frames(gs4d, monkeypatch, rec, cam, view, proj, W, H, t, 1)
    old, st0, ss0 = _fused_frames(gs4d, monkeypatch, rec, cam, view, proj, W, H, t, 0)
    assert st["fused_keygen_draws"] == 2 and st0["fused_keygen_draws"] == 2
    # (a draw that was re-run after an overflow regenerates its order: more sorts, of the same kind)
    assert ss["hybrid_sorts"] >= 2 and ss["sort_launches"] == 2 * ss["hybrid_sorts"] and ss["slow_buckets"] == 0
    assert ss0["hybrid_sorts"] == 0 and ss0["sort_launches"] >= 2 * st0["depth_sort_passes"] and ss0["sort_launches"] % st0["depth_sort_passes"] == 0
    for (k, p, img), (k0, p0, img0) in zip(new, old):
        assert np.array_equal(k, esk) and np.array_equal(p, eperm)
        err = linf(img, eimg)
        print(f"fused frame: Linf against the CPU renderer = {err:.3e}")
        assert err <= TOL
        assert np.array_equal(k, k0) and np.array_equal(p, p0) and np.array_equal(img.view(np.uint32), img0.view(np.uint32))


def test_feedback_falls_back_and_returns(gs4d, oracle, monkeypatch):
    """A crowded set at the default capacity: its first sorts are hybrids with a slow bucket, the report makes the host plan the LSD passes within
    (frame lanes + 1) sorts; a spread set brings the hybrid back as quickly.  Every sort exact."""
    n = 60000
    keys, m = _crowded(n, 0.4, 7)
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        lanes = ctx.stats()["lanes"]
        crowded, spread = _Set(ctx, gs4d, oracle, keys), _Set(ctx, gs4d, oracle, _uniform(n, SPAN24, 8))
        assert crowded.top_counts().max() >= m > TAIL_TILE and spread.top_counts().max() <= TAIL_TILE
        seen = [crowded.sort() for _ in range(lanes + 3)]
        print("crowded:", seen)
        assert seen[0]["hybrid"] == 1 and seen[0]["slow"] == 1
        assert all(d["hybrid"] == 0 for d in seen[lanes + 1:]), "the plan did not fall back to the LSD passes"
        assert seen[-1]["launches"] == 3 + 1 and seen[-1]["largest"] == crowded.top_counts().max()      # three passes and the report
        seen = [spread.sort() for _ in range(lanes + 3)]
        print("spread:", seen)
        assert all(d["hybrid"] == 1 and d["slow"] == 0 for d in seen[lanes + 1:]), "the plan did not return to the hybrid"
        ctx.finish()
    finally:
        ctx.close()

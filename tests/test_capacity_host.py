"""The premises of tests/test_gpu_capacity.py, checked on the CPU with the checker alone (tests/capacity_cases.py builds the scenes).

For every case and both record forms: the longest list is the long tile's and lies in the window of the case's rung; the short neighbours
hold 1, 2, 63, 64 and 65 entries; the chunks of the long list take both branches of composite_chunk; keys tie in pairs and in a run of 70
across entry 64, and the order among ties shows; the probe frame of the rungs below 256 crosses the list capacity and nothing else; removing
the entry at each probed position of the long list, and swapping it with its successor, moves a pixel of the checker's image by more than
ten times the 1e-4 bar of the GPU test (only the order array is changed); the near-tie and fragile masks of the ID restatement stay under
the caps check_parity enforces."""
import numpy as np
import pytest

import capacity_cases as cc
import id_cases
import staged_cases as sc

TOL = 1e-4                       # tests/test_gpu_render.py: the bar of every float image
FORMS = ["4d", "quads"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(cc.CASES))
def test_longest_list_is_in_its_rungs_window(gs4d, oracle, case, form):
    p = cc.prepared(gs4d, oracle, case, form)
    lo, hi = cc.window(case)
    tiles = p.load.tiles.reshape(sc.TY, sc.TX)
    print(f"{case} {form}: L = {p.L}, window {lo} .. {hi}")
    assert lo <= p.L <= hi and p.L == p.scene.K
    assert tiles[cc.LONG[1], cc.LONG[0]] == p.L and p.list.size == p.L and (tiles == p.L).sum() == 1
    for n, (tx, ty) in cc.SHORT.items():
        assert tiles[ty, tx] == (n if n < p.L else 0), (n, tiles[ty, tx])
    if case not in ("full", "over"):
        assert sc.shrunk_hint(p.L) == cc.CASES[case][0]
    if cc.CASES[case][2]:
        q = cc.prepared(gs4d, oracle, case, form, probe=True)
        assert cc.CASES[case][0] < q.L == cc.CASES[case][2] < sc.LIST_HINT0
        assert sc.crossed(p.load, q.load) == {"list"}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(cc.CASES))
def test_chunks_take_both_branches_and_keys_tie(gs4d, oracle, case, form):
    p = cc.prepared(gs4d, oracle, case, form)
    x0, y0, x1, y1 = sc.rects_from_checker(p.eproj)
    recs = cc.order_array(p)[p.list].astype(np.int64)
    tx0, ty0 = cc.LONG[0] * 8, cc.LONG[1] * 8
    bw = np.minimum(x1[recs] - tx0, 7) - np.maximum(x0[recs] - tx0, 0) + 1
    bh = np.minimum(y1[recs] - ty0, 7) - np.maximum(y0[recs] - ty0, 0) + 1
    big = (bw > 4) | (bh > 4)
    kinds = set()
    for hi in range(p.L, 0, -64):                                       # the compositor's chunks: from the end of the list
        c = big[max(hi - 64, 0):hi]
        kinds.add("pixel" if 2 * c.sum() > c.size else ("mixed" if c.any() else "splat"))
    assert "mixed" in kinds and (p.L < 128 or "pixel" in kinds), kinds
    assert (~big).sum() > p.L // 2 and len(np.unique(np.maximum(x0[recs] - tx0, 0) + 8 * np.maximum(y0[recs] - ty0, 0))) >= 32      # small ones on at least half of the tile's pixels
    if form == "4d":
        k = p.keys.view(np.uint32)[recs]
        assert (np.diff(k.astype(np.int64)) >= 0).all() and (np.diff(recs)[np.diff(k.astype(np.int64)) == 0] > 0).all()      # ascending (key, record)
        runs = np.diff(np.flatnonzero(np.concatenate([[True], np.diff(k.astype(np.int64)) != 0, [True]])))
        assert (runs == 2).sum() >= 2
        if p.L >= 100:
            assert runs.max() == 70 and (k[cc.RUN[0]:cc.RUN[1]] == k[cc.RUN[0]]).all() and cc.RUN[0] < 64 < cc.RUN[1]
        # blending the ties the other way round is another picture
        flipped = np.lexsort((-np.arange(p.n, dtype=np.int64), p.keys.view(np.uint32))).astype(np.uint32)
        d = np.abs(cc.reference_image(oracle, p, flipped).astype(np.float64) - cc.reference_image(oracle, p)).max()
        assert d > 10 * TOL, d


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(cc.CASES))
def test_removing_or_swapping_a_probed_entry_shows(gs4d, oracle, case, form):
    p = cc.prepared(gs4d, oracle, case, form)
    base = cc.reference_image(oracle, p).astype(np.float64)
    order = cc.order_array(p)
    worst = np.inf
    for pos in cc.probed(p.L):
        k = p.list[pos]
        d = np.abs(cc.reference_image(oracle, p, np.delete(order, k)) - base).max()
        assert d > 10 * TOL, (pos, "removed", d)
        # the last entry has no successor in the list: its swap is the one of position L - 2
        a, b = (p.list[pos], p.list[pos + 1]) if pos + 1 < p.L else (p.list[pos - 1], p.list[pos])
        o = order.copy()
        o[a], o[b] = order[b], order[a]
        e = np.abs(cc.reference_image(oracle, p, o) - base).max()
        assert e > 10 * TOL, (pos, "swapped", e)
        worst = min(worst, d, e)
    print(f"{case} {form}: smallest change {worst:.3g}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(cc.CASES))
def test_tie_and_fragile_masks_stay_under_the_caps(gs4d, oracle, case, form):
    p = cc.prepared(gs4d, oracle, case, form)
    want = id_cases.restate(p.eproj, p.order, p.w, p.h, premult=(form == "quads"))
    assert want["tie"].mean() < 0.01 and want["fragile"].mean() < 1e-3, (want["tie"].mean(), want["fragile"].mean())
    assert (want["record"] != id_cases.ID_NONE).mean() > 0.001

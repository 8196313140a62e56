"""Record statistics (gs4d_set_record_stats) without a GPU: the ABI, the numpy restatement against hand-computed cases, and the
premise of the GPU tests' scenes (tests/test_gpu_record_stats.py): few fragile pixels, no subnormal weight."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import id_cases
import scenes
import stats_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_header_declares_and_binding_binds_the_entry_point(gs4d):
    hdr = open(os.path.join(ROOT, "include", "gs4d.h")).read()
    assert re.search(r"GS4D_API\s+int\s+gs4d_set_record_stats\s*\(\s*gs4d_ctx\s*\*\s*\w*\s*,\s*gs4d_buf\s+\w+\s*,\s*size_t\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"typedef\s+struct\s+gs4d_record_stat\s*\{", hdr)
    assert "gs4d_set_record_stats" in gs4d.EXPORTS
    for name in ("record_stats", "set_record_stats", "read_record_stats"):
        assert callable(getattr(gs4d.Context, name))
    assert gs4d.Context.RECORD_STAT.itemsize == 16 and gs4d.Context.RECORD_STAT.fields["wsum"][1] == 8
    st = np.zeros(2, gs4d.Context.RECORD_STAT)
    st["wsum"] = [1 << 24, 3 << 23]
    assert np.array_equal(gs4d.record_weight_sum(st), [1.0, 1.5])


def test_record_stat_layout_in_c99(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "gs4d.h"
int main(void) {
    printf("%u %u %u %u\n", (unsigned)sizeof(gs4d_record_stat), (unsigned)offsetof(gs4d_record_stat, pixels), (unsigned)offsetof(gs4d_record_stat, wmax),
           (unsigned)offsetof(gs4d_record_stat, wsum));
    return 0;
}
''')
    exe = tmp_path / "layout"
    cc = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()
    assert out == ["16", "0", "4", "8"], out


# ---- the restatement against hand-computed cases ------------------------------------------------------------------------------------------
def hand(rows):
    """projected records by hand: (cx, cy, half-width in pixels of an axis-aligned square quad, alpha)"""
    p = id_cases.from_device(np.zeros((len(rows), 16), np.float32))
    for k, (cx, cy, half, alpha) in enumerate(rows):
        p[k]["cx"], p[k]["cy"], p[k]["alpha"], p[k]["valid"] = cx, cy, alpha, 1
        p[k]["a0x"] = p[k]["a1y"] = 0.5 / half                        # |u| <= 0.5 <=> |dx| <= half
        p[k]["hx"] = p[k]["hy"] = half
    return p


def cg_of(dx, dy, half):
    """exp(-32 (u^2 + v^2)) in float32, one scalar operation at a time"""
    a = F(0.5 / half)
    u, v = F(a * F(dx)), F(a * F(dy))
    return F(np.exp2(F(F(F(u * u) + F(v * v)) * F(-46.16624130844683))))


def test_restatement_one_record_alone():
    # a quad of one pixel, its centre on pixel (2, 3)'s centre: u = v = 0, cg = 1, w = alpha
    r = sc.restate(hand([(2.5, 3.5, 0.5, 0.5)]), None, 8, 8)
    st = r["stats"]
    assert st["pixels"][0] == 1 and st["wmax"][0] == F(0.5) and st["wsum"][0] == 1 << 23
    assert r["covered"] == 1 and not r["fragile"].any() and not r["subnormal"] and r["layers"][3, 2] == 1 and r["layers"].sum() == 1
    # three pixels wide: nine fragments, the centre's weight is the largest, the sum is the sum of the nine roundings
    r = sc.restate(hand([(2.5, 3.5, 1.5, 0.75)]), None, 8, 8)
    ws = [F(F(0.75) * cg_of(dx, dy, 1.5)) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]
    assert all(cg_of(dx, dy, 1.5) >= F(1e-4) for dx in (-1, 0, 1) for dy in (-1, 0, 1))
    st = r["stats"]
    assert st["pixels"][0] == 9 and st["wmax"][0] == F(0.75) and st["wsum"][0] == sum(int(np.rint(w * F(16777216.0))) for w in ws)
    # a record index beyond the table is drawn and not counted; the others are unchanged
    r2 = sc.restate(hand([(2.5, 3.5, 1.5, 0.75), (5.5, 5.5, 0.5, 0.5)]), None, 8, 8, nrecords=1)
    assert r2["stats"].size == 1 and r2["stats"][0] == st[0] and r2["covered"] == 10


def test_restatement_two_layers():
    # instance 1 is in front (blended first): w = 0.5; instance 0 behind it: w = T * al = 0.5 * 0.25
    r = sc.restate(hand([(2.5, 3.5, 0.5, 0.25), (2.5, 3.5, 0.5, 0.5)]), None, 8, 8)
    st = r["stats"]
    assert list(st["pixels"]) == [1, 1] and st["wmax"][1] == F(0.5) and st["wmax"][0] == F(0.125)
    assert st["wsum"][1] == 1 << 23 and st["wsum"][0] == 1 << 21 and r["T"][3, 2] == F(0.375) and r["layers"][3, 2] == 2
    # the same through an explicit order that puts record 0 in front
    r = sc.restate(hand([(2.5, 3.5, 0.5, 0.25), (2.5, 3.5, 0.5, 0.5)]), [1, 0], 8, 8)
    assert r["stats"]["wmax"][0] == F(0.25) and r["stats"]["wmax"][1] == F(0.375) and r["stats"]["wsum"][1] == 3 << 21


def test_restatement_a_pixel_whose_T_reaches_zero():
    # in front: one pixel, alpha 1, cg = 1: T = 0 exactly.  Behind: three pixels wide over the same centre: that pixel is not counted
    r = sc.restate(hand([(2.5, 3.5, 1.5, 0.75), (2.5, 3.5, 0.5, 1.0)]), None, 8, 8)
    st = r["stats"]
    assert r["T"][3, 2] == 0.0
    assert st["pixels"][1] == 1 and st["wmax"][1] == F(1.0) and st["wsum"][1] == 1 << 24
    ws = [F(F(0.75) * cg_of(dx, dy, 1.5)) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy) != (0, 0)]
    assert st["pixels"][0] == 8 and st["wmax"][0] == max(ws) and st["wsum"][0] == sum(int(np.rint(w * F(16777216.0))) for w in ws)
    assert r["layers"][3, 2] == 1


# ---- the premise of the GPU tests' scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.LAYERED))
def test_layered_scenes_have_few_fragile_pixels_and_no_subnormal_weight(gs4d, oracle, name):
    """From the checker's projection (no GPU): fragile pixels are at most 1 % of the covered pixels and no counted w is subnormal; the scene has
    the lists its name promises."""
    import staged_cases
    W, H, params = sc.layered(name)
    rec = sc.records(gs4d, W, H, *params)
    view, proj = sc.mats(gs4d, W, H)
    eproj = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H, 0.0, 0.0)
    r = sc.restate(eproj, None, W, H)
    print(f"{name}: {rec.shape[0]} records, {r['covered']} covered pixels, {int(r['fragile'].sum())} fragile, at most {int(r['layers'].max())} layers, "
          f"{int((r['stats']['pixels'] > 0).sum())} records count")
    assert r["covered"] > 0.5 * W * H
    assert r["fragile"].sum() <= 0.01 * r["covered"]
    assert not r["subnormal"]
    assert r["layers"].max() >= 4
    longest = staged_cases.Load(staged_cases.rects_from_checker(eproj, W, H), W, H).longest
    cluster = sc.LAYERED[name][4]
    assert longest > (256 if cluster >= 300 else 64 if cluster else 0), longest
    assert (r["stats"]["pixels"] == 0).any()                       # some records never matter: hidden, or outside the image


@pytest.mark.parametrize("kind", ["small", "large", "mixed"])
def test_disjoint_scenes_do_not_overlap(gs4d, oracle, kind):
    W = H = 96
    params = sc.disjoint(kind, W, H)
    rec = sc.records(gs4d, W, H, *params)
    view, proj = sc.mats(gs4d, W, H)
    eproj = oracle.preprocess(oracle.MODE_4D, rec, view, proj, W, H, 0.0, 0.0)
    r = sc.restate(eproj, None, W, H)
    assert r["layers"].max() == 1 and (r["stats"]["pixels"] > 0).all()
    # footprints of <= 4 pixels and of more, as the case names; some records lie on 2 - 4 tiles
    x0, y0, x1, y1 = __import__("staged_cases").rects_from_checker(eproj, W, H)
    side = np.maximum(x1 - x0, y1 - y0) + 1
    tiles = (x1 // 8 - x0 // 8 + 1) * (y1 // 8 - y0 // 8 + 1)
    print(f"{kind}: {rec.shape[0]} records, box sides {side.min()}..{side.max()}, tiles per record {tiles.min()}..{tiles.max()}")
    if kind in ("small", "mixed"):
        assert (side <= 4).any()
    if kind in ("large", "mixed"):
        assert (side > 4).any()
    if kind == "small":
        assert (side <= 4).all()
    if kind == "large":
        assert (side > 4).all()
    assert (tiles >= 2).any() and tiles.max() <= 4

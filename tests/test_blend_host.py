"""CPU only: the scenes of tests/blend_cases.py show what they claim to show, by the CPU checker alone.

* the checker's blend step against OpenGL 4.4 tables 17.1 / 17.2 restated independently (blend_cases.gl_blend), for all 196 factor pairs;
* the matrix scene: the 100 distinct functions give pairwise distinct pictures, no function amplifies the kernel's exp error beyond a quarter of
  the bar, and no fragment's weight lies close enough to the discard threshold for that error to decide it;
* the order probes: the last entry of every list shows, bit for bit, and the picture notices a dropped or a swapped entry;
* the re-run scene: the entry counts overflow the capacities they are meant to overflow, and a draw blended twice would show.
"""
import itertools

import numpy as np
import pytest

import blend_cases as bc

TOL = bc.TOL
PAIRS = [(s, d) for s in bc.FACTORS for d in bc.FACTORS]
DISTINCT = [(s, d) for s in bc.CLASSES for d in bc.CLASSES]


def linf(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# ---- 1. the factor table --------------------------------------------------------------------------------------------------------------------
def test_the_checkers_blend_step_is_the_gl_tables(oracle):
    """One step is two float32 products and one sum of values <= 2: 3 * 2^-23 bounds its distance from the exact value."""
    assert len(PAIRS) == 196 and len(DISTINCT) == 100
    rng = np.random.default_rng(17)
    src = rng.uniform(0.0, 1.0, (4000, 4)).astype(np.float32)
    dst = rng.uniform(0.0, 1.0, (4000, 4)).astype(np.float32)
    corners = np.array(list(itertools.product((0.0, 1.0), repeat=8)), np.float32)         # 0 and 1 on every channel of both
    mixed = rng.uniform(0.0, 1.0, (512, 8)).astype(np.float32)
    snap = rng.uniform(size=mixed.shape)
    mixed = np.where(snap < 0.25, 0.0, np.where(snap < 0.5, 1.0, mixed)).astype(np.float32)      # corners on some channels, interior on others
    src = np.concatenate([src, corners[:, :4], mixed[:, :4]])
    dst = np.concatenate([dst, corners[:, 4:], mixed[:, 4:]])
    worst = 0.0
    for pair in PAIRS:
        got = oracle.blend_step(bc.enums(pair), src, dst)
        want = bc.gl_blend(pair, src, dst)
        err = linf(got, want)
        worst = max(worst, err)
        assert err <= 3 * 2.0 ** -23, (pair, err)
        assert got.min() >= 0.0 and got.max() <= 1.0
    assert worst > 0.0                                          # float32 against float64: the comparison is not vacuous


def test_constant_factors_fold_into_zero_and_one(oracle):
    rng = np.random.default_rng(18)
    src, dst = rng.uniform(0, 1, (256, 4)).astype(np.float32), rng.uniform(0, 1, (256, 4)).astype(np.float32)
    for s, d in PAIRS:
        a = oracle.blend_step(bc.enums((s, d)), src, dst)
        b = oracle.blend_step(bc.enums((bc.CLASS[s], bc.CLASS[d])), src, dst)
        assert np.array_equal(a, b), (s, d)


# ---- 2. the matrix scene --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matrix(gs4d, oracle):
    return bc.matrix(gs4d, oracle)


def test_matrix_scene_layout(matrix, oracle):
    m = matrix
    assert m.W % 8 and m.H % 8 and (m.W // 8 + 1, m.H // 8 + 1) == (13, 7)
    total = m.NB + m.NC + m.ND
    assert 150 <= total <= 400
    assert all(p["valid"].all() for p in (m.eproj_b, m.eproj_c, m.eproj_d))
    # record indices are shuffled against depth
    assert not np.array_equal(m.order_b, np.arange(m.NB)) and not np.array_equal(m.order_b, np.arange(m.NB)[::-1])
    # colours: three distinct channels, none equal to the alpha
    for p in (m.eproj_b, m.eproj_c, m.eproj_d):
        c = np.stack([p["r"], p["g"], p["b"], p["alpha"]], 1).astype(np.float64)
        gaps = [np.abs(c[:, i] - c[:, j]).min() for i in range(4) for j in range(i)]
        assert min(gaps) > 0.01, gaps
    lc = m.LINE_COLOUR.astype(np.float64)
    assert min(abs(lc[i] - lc[j]) for i in range(4) for j in range(i)) > 0.05
    cl = m.CLEAR.astype(np.float64)
    assert min(abs(cl[i] - cl[j]) for i in range(4) for j in range(i)) > 0.05 and 0.0 < cl[3] < 1.0
    # tiles: some untouched (clear colour in every picture), fragments on the partial edge tiles
    depth, lines = m.depth()
    assert lines[m.CROSS[1], m.CROSS[0]] >= 3, lines.max()                  # at least three segments cross in one pixel
    for tx, ty in m.UNTOUCHED:
        assert depth[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].sum() == 0, (tx, ty)
    assert depth[:, 96:].sum() > 0 and depth[48:, :].sum() > 0 and depth[48:, 96:].sum() > 0
    assert 4 <= depth.max() <= 8, depth.max()                               # short stacks: saturation does not merge functions
    for pair in (("ONE", "ONE"), ("DST_COLOR", "ZERO"), bc.OVER):
        for img in m.expected(pair):
            for tx, ty in m.UNTOUCHED:
                assert np.array_equal(img[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8], np.broadcast_to(m.CLEAR, (min(8, m.H - ty * 8), 8, 4)))


def test_matrix_scene_tells_the_functions_apart(matrix):
    """A kernel that mixes up two factors cannot pass: the pictures of any two functions differ by more than 100 * TOL somewhere, at the end
    and after the lines alone.  The 100 pairs of distinct factors are fewer functions than that: src * DST_COLOR is dst * SRC_COLOR, so for
    instance (ZERO, SRC_COLOR) and (DST_COLOR, ZERO) are one polynomial (blend_cases.same_function) — a mix-up inside such a group changes
    nothing anybody could see, and every pair of DIFFERENT functions is held to the bar."""
    fn = bc.same_function(DISTINCT)
    nfn = int(fn.max()) + 1
    assert 90 <= nfn < 100, nfn
    assert fn[DISTINCT.index(("ZERO", "SRC_COLOR"))] == fn[DISTINCT.index(("DST_COLOR", "ZERO"))]
    differ = fn[:, None] != fn[None, :]
    finals = np.stack([matrix.expected(p)[4] for p in DISTINCT]).astype(np.float64).reshape(len(DISTINCT), -1)
    lines = np.stack([matrix.expected(p)[0] for p in DISTINCT]).astype(np.float64).reshape(len(DISTINCT), -1)
    for what, imgs in (("final", finals), ("lines", lines)):
        d = np.full((len(DISTINCT), len(DISTINCT)), np.inf)
        for i in range(len(DISTINCT)):
            d[i, i + 1:] = np.abs(imgs[i + 1:] - imgs[i]).max(axis=1)
        same = d[~differ & np.isfinite(d)]
        assert same.size == 0 or same.max() <= TOL / 4                            # one function: the same picture, up to the rounding of its two forms
        d[~differ] = np.inf
        i, j = np.unravel_index(np.argmin(d), d.shape)
        assert d[i, j] > 100 * TOL, f"{what}: smallest pairwise distance {d[i, j]:.3e} between {DISTINCT[i]} and {DISTINCT[j]} (need > {100 * TOL:.0e}; {nfn} functions)"
        print(f"{what}: smallest pairwise distance {d[i, j]:.3e} between {DISTINCT[i]} and {DISTINCT[j]}; {nfn} distinct functions")


def test_matrix_scene_is_well_conditioned(matrix):
    """gauss_weight is the hardware 2^x of a rounded argument: |argument| <= 24 makes that about 24 * 2^-24 = 1.4e-6 relative, plus one ulp.
    Every record's alpha (and a premultiplied colour) scaled by 1 +- 2^-18 — 2.5 times that — moves no picture of any function by more than
    TOL / 4."""
    worst, at = 0.0, None
    for pair in DISTINCT:
        for k, (a, b) in enumerate(zip(matrix.expected(pair), matrix.perturbed_steps(pair))):
            e = linf(a, b)
            if e > worst:
                worst, at = e, (pair, "abcde"[k])
    assert worst <= TOL / 4, f"worst conditioning {worst:.3e} = {worst / TOL:.3f} TOL at {at} (bar TOL / 4)"
    assert worst > 0.0
    print(f"worst conditioning {worst:.3e} = {worst / TOL:.3f} TOL at {at}")


def test_matrix_scene_keeps_clear_of_the_discard_threshold(matrix):
    """Under (ONE, ZERO) a fragment on the other side of c >= 1e-4 moves a pixel by a whole colour: no weight, in either form, within 2^-16 relative."""
    w = matrix.weights()
    assert w.size > 4000 and (w < bc.DISCARD).any() and (w > 0.5).any()
    margin = bc.discard_margin(w)
    assert margin > bc.DISCARD_MARGIN, f"closest weight to the threshold: {margin:.3e} (need > {bc.DISCARD_MARGIN:.3e})"


# ---- 3. draw order --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def order(gs4d, oracle):
    return bc.order_scene(gs4d, oracle)


def test_order_lists_sit_alone_on_their_tiles(order):
    o = order
    for eproj in (o.eproj, o.eproj_q):
        assert eproj["valid"].all()
        tiles = bc.entries_of(eproj, o.W, o.H).reshape(7, 13)
        for li, (k, (cx, cy)) in enumerate(zip(o.KS, o.CENTRES)):
            assert tiles[cy // 8, cx // 8] == k, (li, tiles[cy // 8, cx // 8])
        assert tiles.sum() == o.n                                               # nothing reaches another tile
    assert o.CENTRES[-1][0] // 8 == 12 and o.CENTRES[-1][1] // 8 == 6           # the 4 x 4 corner tile
    assert set(o.KS) >= {1, 63, 64, 65, 127, 128, 129, 200}
    # small and large footprints, alone and mixed (the chunk's two ways: SMALL_SIDE = 4)
    import staged_cases as sc
    x0, y0, x1, y1 = sc.rects_from_checker(o.eproj, o.W, o.H)
    side = np.maximum(x1 - x0, y1 - y0) + 1
    for li in range(len(o.KS) - 1):                                             # (the corner tile's boxes are cut by the image's edge)
        big = side[o.lst == li] > 4
        assert (not big.any()) if li % 3 == 0 else big.all() if li % 3 == 2 else (big.any() and not big.all()), li
    # every entry covers its probed pixels well above the discard
    rows, cols = zip(*(o.probes(li) for li in range(len(o.KS))))
    for eproj in (o.eproj, o.eproj_q):
        p = eproj
        dx = np.array([c[0] for c in cols])[o.lst] + 0.5 - p["cx"].astype(np.float64)
        dy = np.array([r[0] for r in rows])[o.lst] + 0.5 - p["cy"].astype(np.float64)
        u, v = p["a0x"] * dx + p["a0y"] * dy, p["a1x"] * dx + p["a1y"] * dy
        assert np.all(np.abs(u) < 0.25) and np.all(np.abs(v) < 0.25)
        assert np.exp(-32.0 * (u * u + v * v)).min() > 0.05
    margin = bc.discard_margin(o.weights())
    assert margin > bc.DISCARD_MARGIN, f"closest weight to the threshold: {margin:.3e}"


def test_order_keys_tie_where_they_should(order):
    o = order
    assert np.unique(o.keys_ref.view(np.uint32)).size > o.n - 8                 # the reference's key: (next to) no ties, record indices shuffled
    assert not np.array_equal(o.order_ref, np.sort(o.order_ref))
    for li, k in enumerate(o.KS):
        seq = o.list_order("viewz", li)
        keys = o.keys_vz.view(np.uint32)[seq]
        assert np.all(np.diff(keys.astype(np.int64)) >= 0)
        if k >= 3:
            assert keys[-1] == keys[-2] == keys[-3] and (k == 3 or keys[-4] != keys[-3])
            assert seq[-1] == seq[-3:].max() and np.all(np.diff(seq[-3:].astype(np.int64)) > 0)      # the higher record index is last
            assert not np.array_equal(seq[-3:], o.list_order("ref", li)[-3:])                        # ... which is not the other key's order
        if k >= 127:
            run = seq[o.RUN[0]:o.RUN[1]]
            assert np.unique(keys[o.RUN[0]:o.RUN[1]]).size == 1 and o.RUN[0] < 63 and o.RUN[1] > 65   # one run across entries 63 | 64
            assert np.all(np.diff(run.astype(np.int64)) > 0)
            assert keys[o.RUN[0] - 1] != keys[o.RUN[0]] and keys[o.RUN[1]] != keys[o.RUN[1] - 1]
        assert np.array_equal(o.list_order("direct", li), np.sort(seq))


@pytest.mark.parametrize("way", ["ref", "viewz", "direct", "quads"])
def test_order_probes_show_the_last_entry_and_notice_its_loss(order, way):
    o = order
    full, less, swapped = o.image(way), o.image(way, drop=1), o.image(way, swap=True)
    for li, k in enumerate(o.KS):
        r, c = o.probes(li)
        seq = o.list_order(way, li)
        last = o.rgba[seq[-1]]
        if way != "quads":
            assert np.array_equal(full[r, c, :3], np.broadcast_to(last[:3], (1, 3))), li       # src * 1 + dst * 0: bit for bit
            if k >= 2:
                assert np.array_equal(less[r, c, :3], np.broadcast_to(o.rgba[seq[-2]][:3], (1, 3))), li
        if k >= 2:
            # dropping the last entry, or swapping the last two, moves the probed pixel by far more than the bar
            assert np.abs(full[r, c].astype(np.float64) - less[r, c]).max(axis=1).min() > 100 * TOL, li
            assert np.abs(full[r, c].astype(np.float64) - swapped[r, c]).max(axis=1).min() > 100 * TOL, li
        else:
            assert np.array_equal(less[r, c], np.broadcast_to(o.CLEAR, (1, 4)))


# ---- 4. a re-run blends once ------------------------------------------------------------------------------------------------------------------
def test_rerun_scene_overflows_twice_and_a_second_blend_would_show(gs4d, oracle):
    s = bc.rerun_scene(gs4d, oracle)
    tiles = (s.W // 8) * (s.H // 8)
    e0 = int(bc.entries_of(s.eproj(0, 0.0), s.W, s.H).sum())
    e1, e2 = s.entries(s.N1), s.entries(s.N2)
    assert e1 == tiles * s.N1 and e2 == tiles * s.N2                            # every splat of the two general draws covers every tile
    # a fresh lane: the default draw reserves 2 N0 + 65536 and fits; the first general draw overflows; so does the second, after the growth
    cap = bc.ordered_capacity(0, 0, s.N0)
    assert e0 <= cap
    r1, cap = bc.expected_reruns(cap, e0, s.N1, e1)
    r2, cap2 = bc.expected_reruns(cap, e1, s.N2, e2)
    assert (r1, r2) == (1, 1), (e0, e1, e2, cap, cap2)
    assert bc.expected_reruns(cap2, e2, s.N2, e2) == (0, cap2)                  # and the same draw again fits
    assert 0 < np.count_nonzero(bc.entries_of(s.eproj(0, 0.0), s.W, s.H)) < tiles // 2      # the default draw leaves most tiles lazily clear
    first, second = s.frame()
    _, twice = s.frame(twice=True)
    assert second[..., :3].max() < 0.5 and first.max() < 1.0
    assert np.abs(twice.astype(np.float64) - second).min(axis=(0, 1)).max() > 100 * TOL     # some channel moves at EVERY pixel when the draw blends twice
    assert linf(first, oracle.clear_image(s.W, s.H, s.CLEAR)) > 100 * TOL

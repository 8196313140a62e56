"""GPU parity of every instantiation of the radix sort's pass kernel (csrc/sort.hip, k_os_pass<THREADS, ITEMS, ATOMIC_RANK, RB>: 24 forms) past
one round of tiles, through the C ABI.

tests/sort_cases.py is the table (tests/test_sort_cases_host.py pins it): each form runs at the tile counts on either side of every
group / super-group condition of the look-back and at a count no device holds at once (persistent workgroups: second ticket, LDS reused);
shape 7 runs at 4400 tiles, where the loop over earlier super-groups takes its second round; banded and sorted keys drive the packed
look-back fields to their largest values.
Bar: bit-exact, keys and payload, against numpy's stable argsort (sort_cases.reference).  No tolerance anywhere.
"""
import numpy as np
import pytest

import scenes
import sort_cases as sc
from test_gpu_paths import _ctx

pytestmark = pytest.mark.gpu


def _sort_and_check(ctx, gen, n, form):
    tk = sc.tile_keys(form[0])
    keys, vals, ek, ev = sc.case(gen, n, tk)
    kb, vb = ctx.buffer(keys), ctx.buffer(vals)
    ctx.sort_pairs(kb, vb, n)
    k, v = ctx.read(kb, np.uint32, n), ctx.read(vb, np.uint32, n)
    ctx.delete(kb)
    ctx.delete(vb)
    for what, got, want in (("keys", k, ek), ("values", v, ev)):
        if not np.array_equal(got, want):
            msg = f"{gen}: " + sc.describe_mismatch(what, got, want, keys, tk, form, n)
            print(msg)
            pytest.fail(msg)


@pytest.mark.parametrize("shape,rb,rank", sc.FORMS)
def test_form_at_the_lookback_edges(gs4d, monkeypatch, shape, rb, rank):
    """One context: the large sort first (the scratch grows to it), the small ones in what it left, the large one again."""
    form = (shape, rb, rank)
    cases = sc.edge_tile_counts(shape, rb)
    (_, large), small = cases[-1], cases[:-1]
    ctx = _ctx(gs4d, 64, 64, monkeypatch, GS4D_SORT_RANK=rank, GS4D_SORT_SHAPE=shape, GS4D_SORT_RB=rb)
    try:
        for gen in ("random32", "ascending"):
            _sort_and_check(ctx, gen, large, form)
        for _, n in small:
            for gen in ("random32", "few"):
                _sort_and_check(ctx, gen, n, form)
        for gen in ("super_bands", "one_stray"):
            _sort_and_check(ctx, gen, large, form)
        ctx.finish()                                               # a raised device error word (look-back time-out, key bound, o >= n) fails here
    finally:
        ctx.close()


@pytest.mark.parametrize("rb,rank", sc.DEEP)
def test_third_lookback_level(gs4d, monkeypatch, rb, rank):
    """4400 tiles of 2048 keys: tiles 4352 .. 4399 sum seventeen earlier super-groups, sixteen in the first round and one in the second."""
    form = (sc.DEEP_SHAPE, rb, rank)
    ctx = _ctx(gs4d, 64, 64, monkeypatch, GS4D_SORT_RANK=rank, GS4D_SORT_SHAPE=sc.DEEP_SHAPE, GS4D_SORT_RB=rb)
    try:
        for gen in ("random32", "super_bands", "descending", "group_bands"):
            _sort_and_check(ctx, gen, sc.DEEP_N, form)
        ctx.finish()
    finally:
        ctx.close()


@pytest.mark.parametrize("rb", [8, 9])
def test_fused_keygen_sort_beyond_one_round(gs4d, oracle, monkeypatch, rb):
    """Depth keys from k_keygen into the persistent loop: the producer's digit histograms, the bias, the identity payload and the passes the
    device skips (the sign + exponent digit of positive keys).  Once with the keys read in between, as
    test_gpu_sort.py::test_keygen_and_permutation_bit_exact does, once with the sort right behind the key generation."""
    shape = 7
    tk = sc.tile_keys(shape)
    n = (sc.resident_bound(shape, rb) + 36) * tk + 5
    assert -(-n // tk) == sc.resident_bound(shape, rb) + 37
    pos4, q, scale, life, fade, vel, rgba = scenes.cube_params_4d(n)
    rec = gs4d.build_records_4d(pos4, q, scale, life, fade, vel, rgba)
    cam = np.array(scenes.CAM_CUBE[0], np.float32)
    ctx = _ctx(gs4d, 64, 64, monkeypatch, GS4D_SORT_SHAPE=shape, GS4D_SORT_RB=rb)
    try:
        db = ctx.buffer(rec)
        kb, ib = ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
        identity = np.arange(n, dtype=np.uint32)
        for t, read_between in ((0.0, True), (17.25, False)):
            ctx.keygen(db, t, cam, kb, ib, n)
            _, ekeys = oracle.keygen(rec, t, cam)
            ekeys = ekeys.view(np.uint32)
            keys = ekeys
            if read_between:
                keys = ctx.read(kb, np.uint32, n)                  # the GPU's own keys
                assert np.array_equal(keys, ekeys)
            ctx.sort_pairs(kb, ib, n)
            perm, sk = ctx.read(ib, np.uint32, n), ctx.read(kb, np.uint32, n)
            esk, eperm = sc.reference(keys, identity)              # (not read in between: the sorted keys must be the checker's, sorted)
            for what, got, want in (("keys", sk, esk), ("permutation", perm, eperm)):
                assert np.array_equal(got, want), sc.describe_mismatch(what, got, want, keys, tk, (shape, rb, 0), n)
        ctx.finish()
    finally:
        ctx.close()

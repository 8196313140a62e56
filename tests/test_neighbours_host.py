"""CPU: gs4d_host_count_neighbours — the brute-force definition of gs4d_count_neighbours (include/gs4d.h) — equals the numpy restatement
of the header's text byte for byte; the cell function of the device's search structure encloses every near pair; and the premises of
tests/test_gpu_neighbours.py hold, so that no GPU case is vacuous."""
import ctypes

import numpy as np
import pytest

import edit_cases as ec
import neighbour_cases as nc

f32 = np.float32


def check(case, form, cap, flags, prefilled):
    """one host call against the restatement; returns c"""
    n = case.n
    source, rule, invert = nc.selection(n, form)
    table = nc.table("random" if prefilled else "zero", n)
    want, c = nc.restate(case.rec, case.t, case.r, cap, flags, table, source, rule, invert, near=case.near_f32)
    got = nc.host(case.rec, case.t, case.r, cap, flags, table, source, rule, invert)
    assert got.tobytes() == want.tobytes(), f"{case}, {form}, cap = {cap}, flags = {flags}: rows {np.flatnonzero(got != want)[:8]}"
    return c


@pytest.mark.parametrize("kind", nc.KINDS)
def test_the_host_definition_equals_the_restatement_byte_for_byte(gs4d, kind):
    """every size, source form, cap and flag combination; and every kind has rows with c == 0, rows with 0 < c < cap and saturated rows"""
    zero = between = saturated = 0
    for k, (n, form, cap, flags) in enumerate(nc.matrix()):
        case = nc.case(kind, n)
        c = check(case, form, cap, flags, prefilled=k % 2 == 1)
        part = nc.takes_part(case.rec, case.t, flags)[0]
        zero += int((part & (c == 0)).sum())
        between += int(((c > 0) & (c < cap)).sum())
        saturated += int((c == cap).sum())
    assert zero > 0 and between > 0 and saturated > 0, (kind, zero, between, saturated)


def test_hostile_record_sets(gs4d):
    unplaced = counted = 0
    for k, case in enumerate(nc.hostile_sets()):
        for j, form in enumerate(nc.FORMS):
            for flags in (nc.FLAGS if (k + j) % 5 == 0 else (0, 7)):
                c = check(case, form, nc.CAPS[(k + j + flags) % 3], flags, prefilled=(k + j) % 2 == 0)
                counted += int(c.sum())
        unplaced += int((~np.isfinite(nc.takes_part(case.rec, case.t, 0)[1]).all(1)).sum())
    assert unplaced > 0 and counted > 0


def all_cases():
    return [nc.case(kind, n) for kind in nc.KINDS for n in nc.SIZES] + list(nc.hostile_sets())


def test_every_near_pair_lies_in_the_cell_range_of_its_query_and_no_range_is_longer_than_three(gs4d):
    pairs = 0
    for case in all_cases():
        part, m = nc.takes_part(case.rec, case.t, 0)
        lo, hi = nc.cell_range(m, case.r)
        c = nc.cell(m, nc.grid(case.r)[1])
        assert (hi[part] - lo[part] <= 2).all() and (hi[part] >= lo[part]).all(), case
        near = case.near[0] & part[:, None] & part[None, :]
        inside = np.ones_like(near)
        for a in range(3):
            inside &= (c[None, :, a] >= lo[:, None, a]) & (c[None, :, a] <= hi[:, None, a])
        assert not (near & ~inside).any(), case
        pairs += int(near.sum())
    assert pairs > 100000


def test_the_lattice_has_pairs_at_exactly_r_and_they_count(gs4d):
    case = nc.case("lattice", 4097)
    near, exact = case.near
    assert exact.sum() > 4097 and (near & exact).sum() == exact.sum()
    part = nc.takes_part(case.rec, case.t, 0)[0]
    assert part.all() and (case.rec[:, :3] < 0).any() and (case.rec[:, :3] > 0).any()
    c = nc.restate(case.rec, case.t, case.r, 0xFFFFFFFF, 0, nc.table("zero", 4097))[1]
    assert c.max() == 6 and (c == exact.sum(1)).all()              # the six axis neighbours, all of them at exactly r
    assert np.array_equal(c, nc.lattice_counts(4097))               # ... which is what the large GPU case is checked against


def test_buckets_are_shared_inside_a_query_range_and_between_occupied_cells(gs4d):
    """the two traps of the device's structure occur in the cases: a query whose range holds two distinct cells with the same bucket (walked
    once, or its candidates count twice), and two distinct occupied cells with the same bucket (candidates `near` has to reject)"""
    in_range = occupied = 0
    for case in all_cases():
        part, m = nc.takes_part(case.rec, case.t, 0)
        if not part.any():
            continue
        kb = nc.bucket_bits(case.n)
        lo, hi = nc.cell_range(m[part], case.r)
        b, cells, valid = nc.range_buckets(lo, hi, kb)
        for row in range(b.shape[0]):
            bb, cl = b[row][valid[row]], cells[row][valid[row]]
            assert np.unique(cl).size == cl.size
            in_range += int(np.unique(bb).size < bb.size)
        c = np.unique(nc.cell(m[part], nc.grid(case.r)[1]), axis=0)
        occupied += int(np.unique(nc.bucket(c[:, 0], c[:, 1], c[:, 2], kb)).size < c.shape[0])
    assert in_range > 0 and occupied > 0, (in_range, occupied)


def test_the_restated_cell_function_and_hash(gs4d):
    R, inv_h = nc.grid(0.5)
    assert R == f32(0.50048828125) and inv_h == f32(1.0) / f32(1.0009765625)
    v = np.array([-1e30, -np.inf, -1.5, -1e-30, -0.0, 0.0, 0.99, 1.01, 1e30, np.inf, np.nan], f32)
    assert nc.cell(v, inv_h).tolist() == [nc.CELL_MIN, nc.CELL_MIN, -2, -1, 0, 0, 0, 1, nc.CELL_MAX, nc.CELL_MAX, nc.CELL_MIN]
    assert [nc.bucket_bits(n) for n in (1, 128, 129, 4097, 1 << 28, 1 << 29, 1 << 31)] == [8, 8, 9, 14, 29, 30, 30]
    assert int(nc.bucket(0, 0, 0, 8)) == 0 and int(nc.bucket(1, 0, 0, 30)) == ((73856093 * 2654435761) & 0xFFFFFFFF) >> 2
    assert int(nc.bucket(-1, 2, -3, 12)) == (((((-73856093) & 0xFFFFFFFF) ^ (2 * 19349663) ^ ((-3 * 83492791) & 0xFFFFFFFF)) * 2654435761) & 0xFFFFFFFF) >> 20


def test_a_host_call_the_device_would_refuse_changes_nothing(gs4d):
    case = nc.case("cube", 257)
    n = case.n
    table = nc.table("random", n)
    source, rule, _ = nc.selection(n, "rule")
    lib = gs4d._lib
    good_rule = gs4d._keep_rule(**ec.rule_keywords(rule))

    def call(q, src=None, k=None):
        st = table.copy()
        lib.gs4d_host_count_neighbours(n, case.rec.ctypes.data, None if q is None else ctypes.byref(q), None if src is None else src.ctypes.data,
                                       None if k is None else k.ctypes.data, st.ctypes.data)
        return st

    def q(r=case.r, cap=3, flags=7, reserved=None):
        s = nc.struct(case.t, r, cap, flags)
        if reserved is not None:
            s.reserved[reserved] = 1
        return s

    bad_rule_flag, bad_rule_reserved = good_rule.copy(), good_rule.copy()
    bad_rule_flag["flags"], bad_rule_reserved["reserved"] = 2, 1
    bad = {"query == NULL": (None,), "flag 8": (q(flags=8),), "flag bit 31": (q(flags=0x80000001),), "cap == 0": (q(cap=0),),
           **{f"reserved[{k}]": (q(reserved=k),) for k in range(4)},
           "r = 0": (q(r=0.0),), "r = -0": (q(r=-0.0),), "r < 0": (q(r=-1.0),), "r = NaN": (q(r=np.nan),), "r = inf": (q(r=np.inf),),
           "r * r overflows": (q(r=2.0 ** 64),), "r * r below FLT_MIN": (q(r=float(np.nextafter(f32(2.0 ** -63), f32(0.0)))),),
           "source without a rule": (q(), source, None), "rule flag 2": (q(), source, bad_rule_flag), "rule reserved": (q(), source, bad_rule_reserved)}
    for what, args in bad.items():
        assert call(*args).tobytes() == table.tobytes(), what
    # the ends of the radius range, and the call after the refusals
    for r in (2.0 ** -63, float(np.nextafter(f32(2.0 ** 64), f32(0.0)))):
        got = call(q(r=r, cap=0xFFFFFFFF, flags=4))
        assert got.tobytes() == nc.restate(case.rec, case.t, r, 0xFFFFFFFF, 4, table)[0].tobytes() and got.tobytes() != table.tobytes()
    assert call(q(), source, good_rule).tobytes() == nc.restate(case.rec, case.t, case.r, 3, 7, table, source, rule, False)[0].tobytes()

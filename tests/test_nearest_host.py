"""CPU: gs4d_host_nearest_neighbours — the brute-force definition of gs4d_nearest_neighbours (include/gs4d.h) — equals the numpy
restatement of the header's text byte for byte, hit table and statistics table; and the premises of tests/test_gpu_nearest.py hold, so that no GPU
case is vacuous: rows without a hit, rows that are not full, truncated rows, cuts inside a tie of dist2, a smaller-index twin in front of the
record itself, records that take no part."""
import ctypes

import numpy as np
import pytest

import edit_cases as ec
import nearest_cases as nn
import neighbour_cases as nc

f32 = np.float32


def check(case, form, k, flags, hit_stride, with_stats, prefilled):
    """one host call against the restatement; returns (the slots [n, k], f, the number of candidates, part)"""
    n = case.n
    source, rule, invert = nc.selection(n, form)
    table = nc.table("random" if prefilled else "zero", n) if with_stats else None
    hits = nn.sentinel_hits(n, hit_stride)
    want_h, want_s, f, ncand = nn.restate(case.rec, case.t, case.r, k, flags, hits, table, source, rule, invert, d2=nn.case_dist2(case))
    got_h, got_s = nn.host(case.rec, case.t, case.r, k, flags, hits, table, source, rule, invert)
    what = f"{case}, {form}, k = {k}, flags = {flags}, stride {hit_stride}"
    assert got_h.tobytes() == want_h.tobytes(), f"{what}: rows {np.flatnonzero((got_h != want_h).any(1))[:8]}"
    assert (got_h[:, 8 * k:] == nn.SENTINEL).all(), f"{what}: bytes past 8 k were written"
    if with_stats:
        assert got_s.tobytes() == want_s.tobytes(), f"{what}: table rows {np.flatnonzero(got_s != want_s)[:8]}"
    return nn.slots(got_h, k), f, ncand, nc.takes_part(case.rec, case.t, flags & 3)[0]


class Premises:
    def __init__(self):
        self.empty = self.partial = self.truncated = self.tie_cut = self.twin_first = self.no_part = 0
        self.ks, self.flags, self.forms, self.tables, self.wide = set(), set(), set(), set(), set()

    def add(self, case, form, k, flags, hit_stride, with_stats, prefilled, slots, f, ncand, part):
        self.ks.add(k); self.flags.add(flags); self.forms.add(form); self.wide.add((k, hit_stride))
        if with_stats:
            self.tables.add(prefilled)
        self.empty += int((part & (f == 0)).sum())
        self.partial += int(((f > 0) & (f < k)).sum())
        self.truncated += int((ncand > k).sum())
        self.no_part += int((~part).sum())
        # the cut inside a tie: the first candidate left out is as far as the last one kept
        if (ncand > k).any():
            source, rule, invert = nc.selection(case.n, form)
            bits = nn.candidates(case.rec, case.t, case.r, flags, source, rule, invert, d2=nn.case_dist2(case))[0]
            b = np.sort(bits, axis=1)
            if b.shape[1] > k:
                self.tie_cut += int(((b[:, k] != nn.NOT_A_CANDIDATE) & (b[:, k] == b[:, k - 1])).sum())
        if flags & nn.INCLUDE_SELF and k > 1:
            i = np.arange(case.n)[:, None]
            own = slots["record"][:, 1:] == i                                                     # the record itself, not in slot 0 ...
            ahead = (slots["record"][:, :-1] < i) & (slots["dist2"][:, :-1] == 0)                 # ... behind a twin of a smaller index at dist2 == +0
            self.twin_first += int((own & ahead).sum())


@pytest.mark.parametrize("kind", nc.KINDS)
def test_the_host_definition_equals_the_restatement_byte_for_byte(gs4d, kind):
    p = Premises()
    for n, form, k, flags, hit_stride, with_stats, prefilled in nn.matrix(kind):
        case = nc.case(kind, n)
        p.add(case, form, k, flags, hit_stride, with_stats, prefilled, *check(case, form, k, flags, hit_stride, with_stats, prefilled))
    assert p.ks == set(nn.KS) and p.flags == set(range(8)) and p.forms == set(nc.FORMS) and p.tables == {False, True}, kind
    assert {(3, 32), (1, 1024)} <= p.wide, kind
    assert p.no_part > 0 and p.truncated > 0 and p.empty + p.partial > 0, (kind, vars(p))


def test_the_premises_hold_over_the_matrix(gs4d):
    """over the matrix there are rows without a hit, rows 0 < f < k, truncated rows, cuts inside a tie of dist2 (the lattice with k = 4: an
    interior point has six neighbours at one distance, so the indices decide; the twins), a smaller-index twin in front of the record itself under
    INCLUDE_SELF, and records that take no part"""
    p = Premises()
    lattice_ties = 0
    for kind in nc.KINDS:
        for args in nn.matrix(kind, (63, 65, 257)):
            case = nc.case(kind, args[0])
            q = Premises()
            q.add(case, *args[1:], *check(case, *args[1:]))
            if kind == "lattice" and args[2] == 4:
                lattice_ties += q.tie_cut
            for name, v in vars(q).items():
                if isinstance(v, int):
                    setattr(p, name, getattr(p, name) + v)
    assert p.empty > 0 and p.partial > 0 and p.truncated > 0 and p.tie_cut > 0 and p.twin_first > 0 and p.no_part > 0, vars(p)
    assert lattice_ties > 0


def test_hostile_record_sets(gs4d):
    """every hostile set with flags 0 and 7 and one more value.  Records that take no part: every set that has any under some flag value has them
    under flags 7 (the skips only remove), and flags 7 runs for every set — so each such set is met with its empty rows.  (Most hostile sets are
    hostile in fields the centre does not read — colours, the spatial covariance — and all of their records take part whatever the flags.)"""
    filled = 0
    met = {c.name: False for c in nc.hostile_sets()}
    for case, form, k, flags, hit_stride, with_stats, prefilled in nn.hostile_matrix():
        slots, f, ncand, part = check(case, form, k, flags, hit_stride, with_stats, prefilled)
        filled += int(f.sum())
        met[case.name] |= not part.all()
        assert (slots["record"][~part] == nn.ID_NONE).all() and (slots["dist2"][~part] == nn.INF_BITS).all()
    assert filled > 0
    for case in nc.hostile_sets():
        assert met[case.name] == (not nc.takes_part(case.rec, case.t, 7)[0].all()), case.name
    assert sum(met.values()) >= 10, "sets with records that take no part"


def test_the_stable_argsort_is_the_lexsort_of_the_issue(gs4d):
    case = nc.case("twins", 257)
    bits = nn.candidates(case.rec, case.t, case.r, nn.INCLUDE_SELF)[0]
    j = np.broadcast_to(np.arange(case.n), bits.shape)
    assert np.array_equal(np.lexsort((j, bits), axis=1)[:, :nn.K_MAX], nn.ordered(bits)[0])
    assert ((bits != nn.NOT_A_CANDIDATE).sum(1) > 1).sum() > 100


def test_a_host_call_the_device_would_refuse_changes_nothing(gs4d):
    case = nc.case("cube", 257)
    n = case.n
    table = nc.table("random", n)
    source, rule, _ = nc.selection(n, "rule")
    lib = gs4d._lib
    good_rule = gs4d._keep_rule(**ec.rule_keywords(rule))

    def call(q, src=None, kr=None, stride=32):
        st, ht = table.copy(), nn.sentinel_hits(n, 1024)
        lib.gs4d_host_nearest_neighbours(n, case.rec.ctypes.data, None if q is None else ctypes.byref(q), None if src is None else src.ctypes.data,
                                         None if kr is None else kr.ctypes.data, ht.ctypes.data, ctypes.c_size_t(stride), st.ctypes.data)
        return st.tobytes() + ht.tobytes()

    def q(r=case.r, k=3, flags=7, reserved=None):
        s = nn.struct(case.t, r, k, flags)
        if reserved is not None:
            s.reserved[reserved] = 1
        return s

    untouched = table.tobytes() + nn.sentinel_hits(n, 1024).tobytes()
    bad_rule_flag, bad_rule_reserved = good_rule.copy(), good_rule.copy()
    bad_rule_flag["flags"], bad_rule_reserved["reserved"] = 2, 1
    bad = {"query == NULL": (None,), "flag 8": (q(flags=8),), "flag bit 31": (q(flags=0x80000001),), "k == 0": (q(k=0),), "k == 17": (q(k=17),),
           **{f"reserved[{k}]": (q(reserved=k),) for k in range(4)},
           "r = 0": (q(r=0.0),), "r < 0": (q(r=-1.0),), "r = NaN": (q(r=np.nan),), "r = inf": (q(r=np.inf),), "r * r overflows": (q(r=2.0 ** 64),),
           "r * r below FLT_MIN": (q(r=float(np.nextafter(f32(2.0 ** -63), f32(0.0)))),),
           "source without a rule": (q(), source, None), "rule flag 2": (q(), source, bad_rule_flag), "rule reserved": (q(), source, bad_rule_reserved),
           "stride 0": (q(), None, None, 0), "stride 8": (q(k=1), None, None, 8), "stride 24": (q(), None, None, 24), "stride 1040": (q(), None, None, 1040),
           "stride below 8 k": (q(k=5), None, None, 32)}
    for what, args in bad.items():
        assert call(*args) == untouched, what
    assert call(q(), source, good_rule) != untouched and call(q(k=16), None, None, 128) != untouched

"""CPU: gs4d_host_label_components and gs4d_host_count_labels — the brute-force definitions of gs4d_label_components and gs4d_count_labels
(include/gs4d.h) — equal the numpy restatement of the header's text byte for byte (a label propagation to the fixed point: no
union–find); the premises of tests/test_gpu_components.py hold, so that no GPU case is vacuous; and the union–find text the kernels compile
(csrc/component_union.h) survives 16 contending threads in a stand-alone program, under ThreadSanitizer where its runtime is installed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import component_cases as cp
import edit_cases as ec
import neighbour_cases as nc

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(sc, selection, flags, cap, prefilled):
    """one host call against the restatement; returns the labels"""
    case = sc.case
    source, rule, invert = selection
    table = cp.table(prefilled, sc.n)
    want_l, want_t = cp.restate(case.rec, case.t, case.r, cap, flags, table, source, rule, invert, near=case.near[0])
    got_l, got_t = cp.host(case.rec, case.t, case.r, cap, flags, table, source, rule, invert)
    what = f"{sc}, flags = {flags}, cap = {cap}, source {'given' if source is not None else 'none'}"
    assert got_l.dtype == np.uint32 and got_l.tobytes() == want_l.tobytes(), f"{what}: labels {np.flatnonzero(got_l != want_l)[:8]}"
    assert (table is None and got_t is None) or got_t.tobytes() == want_t.tobytes(), f"{what}: rows {np.flatnonzero(got_t != want_t)[:8]}"
    return got_l


@pytest.mark.parametrize("n", cp.SIZES)
def test_the_host_definition_equals_the_restatement_byte_for_byte(gs4d, n):
    """every scenario of the size, every call of it; and the component sizes the constructions promise"""
    members = linked = alone = 0
    for sc in cp.by_size(n):
        for k, (selection, flags, cap, prefilled) in enumerate(cp.calls(sc)):
            labels = check(sc, selection, flags, cap, prefilled)
            if k == 0 and sc.sizes is not None:
                assert cp.component_sizes(labels) == sc.sizes, sc
            sizes = cp.component_sizes(labels)
            members += sum(sizes); linked += sum(s for s in sizes if s > 1); alone += sum(s == 1 for s in sizes)
    assert members > 0 and alone > 0 and (n == 1 or linked > 0)


def test_the_clumps_and_the_large_sets(gs4d):
    for sc in (cp.clump(), cp.clumps()):
        for cap in (1, 3, cp.NOCAP):
            for prefilled in (False, True):
                labels = check(sc, sc.selection, 0, cap, prefilled)
        assert cp.component_sizes(labels) == sc.sizes
    # the contention case: every pair of the 256 is an edge, and at less than r / 2
    near = cp.clump().case.near[0]
    assert near.all() and nc.near_matrix(cp.clump().case.rec[:, :3], 0.5)[0].all() and near.sum() - 256 == 2 * 32640
    # saturation shows in the rows: with cap 3 the clumps of 1 and 2 stay below it and 62 clumps reach it
    sc = cp.clumps()
    labels, t3 = cp.host(sc.case.rec, 0.0, 1.0, 3, 0, nc.table("zero", sc.n))
    size = np.bincount(labels)[labels]
    assert np.array_equal(t3["pixels"], np.minimum(size, 3)) and set(t3["pixels"].tolist()) == {1, 2, 3} and size.max() == 64
    assert (np.diff(np.flatnonzero(labels == labels[-1])) > 1).sum() == 62, "the records of a clump are spread over the indices"


@pytest.mark.parametrize("order", cp.ORDERS)
def test_premises_of_the_chains(gs4d, order):
    for n in cp.SIZES:
        sc = cp.chain(n, order)
        labels, _ = cp.host(sc.case.rec, 0.0, 1.0, cp.NOCAP, 0)
        assert (labels == 0).all(), "one component, whose label is record 0"
        near = sc.case.near[0]
        assert near.sum() - n == 2 * (n - 1), "every record is near its two neighbours on the line and nobody else"
        g = cp.chain(n, order, gap=True)
        labels, _ = cp.host(g.case.rec, 0.0, 1.0, cp.NOCAP, 0)
        assert cp.component_sizes(labels) == g.sizes and len(g.sizes) == min(n, 2)
        if n >= 3:
            # the two bends: the pair at exactly r links, the pair at the next float above r does not
            perm, (_, (a, b)) = cp.order_of(n, order), cp.chain_positions(n, True)
            near, exact = g.case.near
            assert near[perm[a - 1], perm[a]] and exact[perm[a - 1], perm[a]] and labels[perm[a - 1]] == labels[perm[a]]
            assert not near[perm[b - 1], perm[b]] and labels[perm[b - 1]] != labels[perm[b]]
            d = g.case.rec[perm[b], :3] - g.case.rec[perm[b - 1], :3]
            assert d[0] == 0 and d[1] == 0 and d[2] == f32(cp.ABOVE_ONE) and exact.sum() == 2
    if order == "shuffled":
        assert not np.array_equal(cp.order_of(4097, order), np.arange(4097))


def test_premises_of_the_lattices_the_bodies_and_the_bridges(gs4d):
    for n in cp.SIZES:
        near, exact = cp.lattice(n).case.near
        assert n < 2 or ((near & exact).sum() > 0 and (near & exact).sum() == near.sum() - n), "every link of the lattice is a pair at exactly r"
        assert cp.lattice(n, apart=True).case.near[0].sum() == n, "just below the spacing nobody is near anybody"
        # two bodies: one component at t0, two at t1 — the same records
        b0, b1 = cp.bodies(n, cp.BODIES_T0), cp.bodies(n, cp.BODIES_T1)
        assert np.array_equal(b0.case.rec, b1.case.rec) and b0.sizes == [n] and (n < 2 or len(b1.sizes) == 2)
        for how in cp.BRIDGES:
            on, off = cp.bridge(n, how), cp.bridge(n, how, on=False)
            source, rule, invert = on.selection
            labels, _ = cp.host(on.case.rec, 0.0, 1.0, cp.NOCAP, on.flags, None, source, rule, invert)
            assert labels[n // 2] == cp.NONE and cp.component_sizes(labels) == on.sizes, (n, how)
            assert n < 3 or (len(on.sizes) == 2 and labels[0] == 0 and labels[n - 1] == n // 2 + 1)
            labels, _ = cp.host(off.case.rec, 0.0, 1.0, cp.NOCAP, off.flags)
            assert (labels == 0).all(), "without the skip / the table the middle record joins the two halves"
            if source is not None:
                assert int(ec.selected(n, source, rule, invert).sum()) == n - 1


def test_the_slab_labels_are_the_host_definition(gs4d):
    """the closed form the n = 70001 GPU case is checked against, pinned to the host definition and to the restatement at 4097"""
    sc = cp.slabs(4097)
    labels = check(sc, sc.selection, 0, cp.NOCAP, False)
    want = cp.slab_labels(4097)
    assert np.array_equal(labels, want) and np.unique(want).size == 3 and cp.component_sizes(labels) == sc.sizes
    # the same construction at the large size: gaps of 0.75 > r between slabs, exact coordinates, several slabs
    big = cp.slabs(cp.N_BIG)
    z = np.unique(big.case.rec[:, 2])
    assert np.unique(cp.slab_labels(cp.N_BIG)).size == 8 and np.isin(np.diff(z), (0.5, 0.75)).all() and (np.diff(z) == 0.75).sum() == 7
    assert (big.case.rec[:, :3] * 4 == np.round(big.case.rec[:, :3] * 4)).all()


def test_hostile_record_sets(gs4d):
    none = some = 0
    for k, case in enumerate(nc.hostile_sets()):
        sc = cp.Scenario(case.name, case.rec, case.t, case.r)
        for j, form in enumerate(nc.FORMS):
            for flags in (0, 3):
                labels = check(sc, nc.selection(sc.n, form), flags, nc.CAPS[(k + j + flags) % 3], (None, False, True)[(k + j) % 3])
                none += int((labels == cp.NONE).sum()); some += int((labels != cp.NONE).sum())
    assert none > 0 and some > 0


def test_count_labels_equals_the_restatement(gs4d):
    sc = cp.clumps()
    n = sc.n
    labels, _ = cp.host(sc.case.rec, 0.0, 1.0, cp.NOCAP, 0)
    planted = labels.copy()
    planted[[5, 70, 300, 2000]] = (n, n + 5, 0xFFFFFFFE, cp.NONE)      # out of range: neither hit nor hitting
    rule = nc.RULE
    for lab in (labels, planted):
        for name, seeds_of in SEEDS.items():
            mask = seeds_of(lab, n)
            for invert in (False, True):
                seeds = ec.mask_table(mask ^ invert, rule)
                for prefilled in (False, True):
                    table = nc.table("random" if prefilled else "zero", n)
                    got = cp.host_count_labels(lab, seeds, rule, invert, table)
                    want = cp.restate_count_labels(lab, seeds, rule, invert, table)
                    assert got.tobytes() == want.tobytes(), (name, invert, prefilled)
                    hit = int((got["pixels"] != table["pixels"]).sum())
                    assert hit == HITS[name](lab, n), (name, hit)
    # a seed whose own label is out of range hits nothing, and a record whose label is out of range is not hit by its old component
    seeds = ec.mask_table(np.arange(n) == 2000, rule)
    assert cp.host_count_labels(planted, seeds, rule, False, nc.table("zero", n))["pixels"].sum() == 0
    seeds = ec.mask_table(np.arange(n) == int(labels[2000]), rule)
    got = cp.host_count_labels(planted, seeds, rule, False, nc.table("zero", n))["pixels"]
    assert got[2000] == 0 and got.sum() == (labels == labels[2000]).sum() - 1


# seed masks that hit no, one, several and all components (labels below n only)
SEEDS = {
    "none": lambda lab, n: np.zeros(n, bool),
    "one": lambda lab, n: np.arange(n) == n - 1,
    "several": lambda lab, n: np.isin(np.arange(n), (63, 64, 1000, n - 1)),
    "all": lambda lab, n: np.ones(n, bool),
}
HITS = {
    "none": lambda lab, n: 0,
    "one": lambda lab, n: int((lab == lab[n - 1]).sum()),
    "several": lambda lab, n: int(np.isin(lab, lab[[63, 64, 1000, n - 1]]).sum()),
    "all": lambda lab, n: int((lab < n).sum()),
}


def test_the_floater_clumps_pass_isolated_and_fail_small_components(gs4d):
    rec, planted, r = cp.floaters()
    n = rec.shape[0]
    c = nc.host(rec, 0.0, r, 2, 0, nc.table("zero", n))["pixels"]
    assert (c >= 2).all(), "isolated(k = 2) flags none of the records: each planted one has four neighbours"
    labels, table = cp.host(rec, 0.0, r, 10, 0, nc.table("zero", n))
    assert np.array_equal(np.flatnonzero(table["pixels"] < 10), planted) and (table["pixels"][planted] == 5).all()
    assert np.unique(labels[planted]).size == 5


def test_the_two_bodies_are_two_components(gs4d):
    rec, first, r = cp.two_bodies()
    labels, _ = cp.host(rec, 0.0, r, cp.NOCAP, 0)
    assert (labels[:first] == 0).all() and (labels[first:] == first).all()


def test_a_host_call_the_device_would_refuse_changes_nothing(gs4d):
    sc = cp.generic("cube", 257)
    case, n = sc.case, sc.n
    table = nc.table("random", n)
    source, rule, _ = nc.selection(n, "rule")
    lib = gs4d._lib
    good_rule = gs4d._keep_rule(**ec.rule_keywords(rule))

    def call(q, src=None, k=None):
        st, lab = table.copy(), np.full(n, cp.SENTINEL_WORD, np.uint32)
        lib.gs4d_host_label_components(n, case.rec.ctypes.data, None if q is None else ctypes.byref(q), None if src is None else src.ctypes.data,
                                       None if k is None else k.ctypes.data, lab.ctypes.data, st.ctypes.data)
        return lab, st

    def q(r=case.r, cap=3, flags=3, reserved=None):
        s = cp.struct(case.t, r, cap, flags)
        if reserved is not None:
            s.reserved[reserved] = 1
        return s

    bad_rule_flag, bad_rule_reserved = good_rule.copy(), good_rule.copy()
    bad_rule_flag["flags"], bad_rule_reserved["reserved"] = 2, 1
    bad = {"query == NULL": (None,), "flag 4": (q(flags=4),), "flag bit 31": (q(flags=0x80000001),), "cap == 0": (q(cap=0),),
           **{f"reserved[{k}]": (q(reserved=k),) for k in range(4)},
           "r = 0": (q(r=0.0),), "r < 0": (q(r=-1.0),), "r = NaN": (q(r=np.nan),), "r = inf": (q(r=np.inf),),
           "r * r overflows": (q(r=2.0 ** 64),), "r * r below FLT_MIN": (q(r=float(np.nextafter(f32(2.0 ** -63), f32(0.0)))),),
           "source without a rule": (q(), source, None), "rule flag 2": (q(), source, bad_rule_flag), "rule reserved": (q(), source, bad_rule_reserved)}
    for what, args in bad.items():
        lab, st = call(*args)
        assert st.tobytes() == table.tobytes() and (lab == cp.SENTINEL_WORD).all(), what
    lab, st = call(q(), source, good_rule)
    want_l, want_t = cp.restate(case.rec, case.t, case.r, 3, 3, table, source, rule, False)
    assert lab.tobytes() == want_l.tobytes() and st.tobytes() == want_t.tobytes() and st.tobytes() != table.tobytes()
    # gs4d_host_count_labels: no rule, a bad rule
    seeds = ec.mask_table(np.ones(n, bool), rule)
    for k in (None, bad_rule_flag, bad_rule_reserved):
        st = table.copy()
        lib.gs4d_host_count_labels(n, want_l.ctypes.data, seeds.ctypes.data, None if k is None else k.ctypes.data, st.ctypes.data)
        assert st.tobytes() == table.tobytes()


def test_the_union_find_text_under_sixteen_threads(gs4d, tmp_path):
    """tests/component_union_stress.cpp — a program of its own over csrc/component_union.h — built with -fsanitize=thread where the compiler can
    link that runtime, else plain -O1 -pthread, and run: exit status 0 means every label was the component's minimum, no trip bound ran out and,
    under the sanitizer, no data race was reported"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler"
    src, exe = os.path.join(ROOT, "tests", "component_union_stress.cpp"), str(tmp_path / "component_union_stress")
    base = [cxx, "-std=c++17", "-O1", "-g", "-pthread", src, "-o", exe]
    built = subprocess.run(base + ["-fsanitize=thread"], capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600) if built.returncode == 0 else None
    if run is None or "FATAL: ThreadSanitizer" in run.stderr:      # no runtime to link, or one that cannot start on this kernel: the plain build
        built = subprocess.run(base, capture_output=True, text=True)
        assert built.returncode == 0, built.stderr[-2000:]
        run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "component_union_stress: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])

"""GPU: the depth sort's MSD/LSD hybrid (csrc/sort.hip: k_os_pass<512, 12, true, 9> on the 9-bit top digit, then k_os_tail<256> / <512>) at every
decision point tests/hybrid_cases.py names: every span 19..27, bucket 0 and bucket 511, bucket sizes either side of a lane, a wave's row, one row
per wave, the LDS tile and the slow path's chunk, the capacity edges, the top pass past its look-back levels and with persistent workgroups, plans
that are abandoned between key generation and sort, a payload that is not the index, the epoch wrap, and the second caller (gs4d_count_neighbours
through k_os_hist).  tests/test_hybrid_cases_host.py pins the premises of every case on the CPU.

Bar: keys AND payload equal to sort_cases.reference (numpy's stable argsort), element for element, no tolerance; every case ends in ctx.finish(),
which raises when a kernel has set the error word, and asserts through Context.sort_stats() that the path it is about ran.  Through the C ABI, with
GS4D_SORT_HYBRID=1; a context that has sorted a slow bucket is not used for a case that needs the hybrid afterwards (the report turns the next
plans to the LSD passes)."""
import functools
import os

import numpy as np
import pytest

import edit_cases as ec
import hybrid_cases as hc
import neighbour_cases as nc
import sort_cases as sc
from test_gpu_paths import _ctx

pytestmark = pytest.mark.gpu


def _hybrid_ctx(gs4d, monkeypatch, cap=None):
    monkeypatch.delenv("GS4D_SORT_TAILCAP", raising=False)
    return _ctx(gs4d, 64, 64, monkeypatch, GS4D_SORT_HYBRID=1, **({} if cap is None else {"GS4D_SORT_TAILCAP": cap}))


class Keyed:
    """one record set on one context: the record buffer (the targets' records, then the two pins of a span_for(bits) box), key, index and payload
    buffers, the keys the records yield, and sort() = keygen + sort + read + check against the reference"""

    def __init__(self, ctx, gs4d, oracle, targets, bits, cap=hc.TAIL_TILE):
        self.ctx, self.n, self.cap = ctx, len(targets), cap
        rec = hc._records(gs4d, targets, hc.span_for(bits))
        self.bias, self.bits = hc._proven(gs4d, rec)
        assert (self.bias, self.bits) == (hc.KEY_LO, bits)
        _, ek = oracle.keygen(rec[:self.n], 0.0, np.array(hc.CAM0, np.float32))
        self.keys = ek.view(np.uint32)
        self.oracle = oracle
        self.db, self.kb, self.ib = ctx.buffer(rec), ctx.buffer(nbytes=4 * self.n), ctx.buffer(nbytes=4 * self.n)
        self._want = {}

    def top_counts(self, n=None):
        return np.bincount(hc.top_digit(self.keys[:n], self.bias, self.bits), minlength=512)

    def want(self, n=None, vals=None):
        """the expected (keys, payload) of a sort of the first n keys (computed once per n for the index payload)"""
        n = self.n if n is None else n
        if vals is not None:
            return sc.reference(self.keys[:n], vals)
        if n not in self._want:
            ident = np.arange(n, dtype=np.uint32)
            self._want[n] = sc.reference(self.keys[:n], ident)
            if n <= 300000:                                     # the second checker (the first is numpy alone)
                sk, sv = self.oracle.sort_pairs(np.ascontiguousarray(self.keys[:n]), ident, "std")
                assert np.array_equal(sk, self._want[n][0]) and np.array_equal(sv, self._want[n][1])
        return self._want[n]

    def keygen(self, n=None):
        self.ctx.keygen(self.db, 0.0, hc.CAM0, self.kb, self.ib, self.n if n is None else n)

    def check(self, want, vb=None, keys=None, what=""):
        n = len(want[0])
        k, v = self.ctx.read(self.kb, np.uint32, n), self.ctx.read(self.ib if vb is None else vb, np.uint32, n)
        keys = self.keys[:n] if keys is None else keys
        for name, got, w in (("keys", k, want[0]), ("payload", v, want[1])):
            assert np.array_equal(got, w), hc.describe_mismatch(f"{what} {name}", got, w, keys, self.bias, self.bits, self.cap)

    def sort(self, n=None, keygen=True, what=""):
        """keygen (unless the caller has done it) + sort of the first n + check -> the change of the sort statistics over it"""
        ctx = self.ctx
        n = self.n if n is None else n
        before = ctx.sort_stats()
        if keygen:
            self.keygen(n)
        ctx.sort_pairs(self.kb, self.ib, n)
        self.check(self.want(n), what=what)
        return delta(before, ctx.sort_stats())


def delta(before, after):
    return {"hybrid": after["hybrid_sorts"] - before["hybrid_sorts"], "launches": after["sort_launches"] - before["sort_launches"],
            "largest": after["largest_bucket"], "slow": after["slow_buckets"]}


HYBRID = {"hybrid": 1, "launches": 2}                          # the top pass and the tail; the producer counted the histogram


def ran(d, **want):
    want = {**HYBRID, **want}
    assert {k: d[k] for k in want} == want, d


# ---- a. every span -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", hc.WIDTHS)
def test_every_span_every_bucket_size(gs4d, oracle, monkeypatch, bits):
    """The fit profile twice (the two histogram slots), then the slow profile: buckets of every size of FIT_SIZES / SLOW_SIZES, in bucket 0 and
    in bucket 511, sorted on rem = bits - 9 bits as local digits of (w0, w1) bits by k_os_tail<LB>."""
    rem, w0, w1, lb = hc.edges(bits)
    print(f"{bits} bits: rem = {rem}, local digits {w0} + {w1}, k_os_tail<{lb}>; bucket sizes {hc.SLOW_SIZES} in top digits {hc.DIGITS}")
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        fit = Keyed(ctx, gs4d, oracle, hc.fit_profile(bits), bits)
        assert fit.bits == bits and fit.top_counts()[511] == hc.TAIL_TILE and fit.top_counts()[0] == 1
        for k in range(2):
            ran(fit.sort(what=f"fit profile, sort {k},"), slow=0, largest=hc.TAIL_TILE)
        slow = Keyed(ctx, gs4d, oracle, hc.slow_profile(bits), bits)
        assert slow.bits == bits and slow.n == 46787 and slow.top_counts()[510] == hc.TAIL_TILE + 1
        ran(slow.sort(what="slow profile,"), slow=2, largest=2 * hc.TAIL_TILE)
        ctx.finish()
    finally:
        ctx.close()


# ---- b. capacity edges -------------------------------------------------------------------------------------------------------------------------------
def test_buckets_of_cap_minus_one_cap_and_cap_plus_one(gs4d, oracle, monkeypatch):
    """GS4D_SORT_TAILCAP=2048: 2047, 2048 and 2049 keys in neighbouring top digits, the middle one the first of a wave of the bucket scan"""
    sizes, digits = [300, 2047, 2048, 2049, 500], [0, 255, 256, 257, 511]
    ctx = _hybrid_ctx(gs4d, monkeypatch, cap=2048)
    try:
        s = Keyed(ctx, gs4d, oracle, hc.profile(24, sizes, digits, 2048), 24, cap=2048)
        assert np.array_equal(s.top_counts(), hc.profile_counts(sizes, digits))
        ran(s.sort(), slow=1, largest=2049)
        ctx.finish()
    finally:
        ctx.close()


def test_a_capacity_of_one_key(gs4d, oracle, monkeypatch):
    """GS4D_SORT_TAILCAP=1: every bucket of two keys and more takes the slow path (chunks of 2, 3, ... keys), buckets of one key the LDS path"""
    rng = np.random.default_rng(1)
    sizes = [1, 2, 1, 3, 1, 2, 1, 64] + [int(v) for v in rng.integers(50, 140, 32)]
    digits = [0, 511] + [int(v) for v in rng.choice(np.arange(1, 511), 38, replace=False)]
    assert len(sizes) == len(digits) == 40 and 2500 < sum(sizes) < 3500
    ctx = _hybrid_ctx(gs4d, monkeypatch, cap=1)
    try:
        s = Keyed(ctx, gs4d, oracle, hc.profile(24, sizes, digits, 11), 24, cap=1)
        tc = s.top_counts()
        assert np.array_equal(tc, hc.profile_counts(sizes, digits)) and np.count_nonzero(tc == 1) == 4
        ran(s.sort(), slow=int(np.count_nonzero(tc >= 2)), largest=int(tc.max()))
        ctx.finish()
    finally:
        ctx.close()


# ---- c. a slow bucket that only one local digit orders -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [24, 27])
def test_a_slow_bucket_of_six_values(gs4d, oracle, monkeypatch, bits):
    """3 x 8192 + 5 keys of six values in one bucket — three that differ in bits [0, w0) alone, three in bits [w0, rem) alone: each slow pass moves
    long runs of ties across the chunks by its running digit offsets alone; the rest of the set is uniform"""
    targets, _ = hc.one_digit_case(gs4d, oracle, bits, 20000, 40 + bits)
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        s = Keyed(ctx, gs4d, oracle, targets, bits)
        tc = s.top_counts()
        assert tc[hc.ONE_DIGIT_TOP] == hc.ONE_DIGIT_BUCKET == tc.max() and np.unique(s.keys[hc.top_digit(s.keys, s.bias, bits) == hc.ONE_DIGIT_TOP]).size == 6
        ran(s.sort(), slow=1, largest=hc.ONE_DIGIT_BUCKET)
        ctx.finish()
    finally:
        ctx.close()


# ---- d. payload --------------------------------------------------------------------------------------------------------------------------------------
def test_a_payload_that_is_not_the_index(gs4d, oracle, monkeypatch):
    """The fit profile at 25 bits, sorted with a random permutation in a buffer of its own instead of the index keygen wrote: the histogram is of
    those keys, so it is the hybrid, and the top pass reads the payload instead of making the index up."""
    bits = 25
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        s = Keyed(ctx, gs4d, oracle, hc.fit_profile(bits), bits)
        vals = hc.payload(s.n, 25)
        pb = ctx.buffer(vals)
        before = ctx.sort_stats()
        s.keygen()
        ctx.sort_pairs(s.kb, pb, s.n)
        s.check(s.want(vals=vals), vb=pb)
        ran(delta(before, ctx.sort_stats()), slow=0, largest=hc.TAIL_TILE)
        assert np.array_equal(ctx.read(s.ib, np.uint32, s.n), np.arange(s.n, dtype=np.uint32)), "the index buffer was not part of the sort"
        ctx.finish()
    finally:
        ctx.close()


# ---- e. abandoned plans ------------------------------------------------------------------------------------------------------------------------------
def test_a_hybrid_planned_histogram_that_another_sort_meets(gs4d, oracle, monkeypatch):
    """Key generation plans the hybrid and leaves a top-digit row in the histogram slot (hist_rows, hist_top, hist_hybrid, hist_bias).  Every way of
    not running the sort it was planned for: other keys, another n, a second key generation, a key generation of another span."""
    n = 40003
    lsd = {"hybrid": 0, "launches": 1 + 4}                      # 32 key bits: k_os_hist and four 8-bit passes, no report
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        x = Keyed(ctx, gs4d, oracle, hc._uniform(n, hc.span_for(24), 24), 24)
        y = Keyed(ctx, gs4d, oracle, hc._uniform(n, hc.span_for(26), 26), 26)
        assert hc.edges(y.bits)[3] == 512 and max(x.top_counts().max(), y.top_counts().max()) <= hc.TAIL_TILE
        ident = np.arange(n, dtype=np.uint32)
        # another n: the first n - 1 of the keys keygen wrote; the last pair stays where it is
        x.keygen()
        d = x.sort(n - 1, keygen=False, what="n - 1 keys,")
        assert {k: d[k] for k in lsd} == lsd, d
        assert ctx.read(x.kb, np.uint32, n)[-1] == x.keys[-1] and ctx.read(x.ib, np.uint32, n)[-1] == n - 1
        ran(x.sort(what="after the sort of n - 1 keys,"), slow=0)
        # a second key generation before the sort
        before = ctx.sort_stats()
        x.keygen()
        ran(x.sort(what="two key generations,"), slow=0)
        assert delta(before, ctx.sort_stats())["hybrid"] == 1
        # a key generation of another span in between: 15 -> 17 bits below the top digit, k_os_tail<256> -> <512>
        x.keygen()
        ran(y.sort(what="keygen X, keygen Y, sort Y,"), slow=0, largest=int(y.top_counts().max()))
        # other keys: 16 of them replaced behind the key generation (any 32-bit patterns, some below the bias)
        x.keygen()
        where = np.arange(16) * 2501 + 7
        changed = np.array(x.keys)
        changed[where] = np.random.default_rng(16).integers(0, 2 ** 32, 16, dtype=np.uint64).astype(np.uint32)
        changed[where[:2]] = (0, 0xFFFFFFFF)
        for i in where:
            ctx.subdata(x.kb, changed[i:i + 1], offset=4 * int(i))
        before = ctx.sort_stats()
        ctx.sort_pairs(x.kb, x.ib, n)
        x.check(sc.reference(changed, ident), keys=changed, what="16 keys changed,")
        d = delta(before, ctx.sort_stats())
        assert {k: d[k] for k in lsd} == lsd, d
        ran(x.sort(what="after the sort of other keys,"), slow=0)
        ran(y.sort(what="Y again,"), slow=0)
        ctx.finish()
    finally:
        ctx.close()


# ---- f. small n --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 65, 6144, 6145])
def test_small_sorts(gs4d, oracle, monkeypatch, n):
    """one tile of the top pass with 2 keys, a row and a key, every slot; a second tile of one key"""
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        s = Keyed(ctx, gs4d, oracle, hc._uniform(n, hc.span_for(24), n), 24)
        for k in range(2):
            ran(s.sort(what=f"sort {k},"), slow=0, largest=int(s.top_counts().max()))
        ctx.finish()
    finally:
        ctx.close()


# ---- g. the top pass past its look-back edges --------------------------------------------------------------------------------------------------------
def test_the_top_pass_at_17_257_273_and_549_tiles(gs4d, oracle, monkeypatch):
    """548 x 6144 + 1 uniform 24-bit keys; prefixes of 549, 17, 257, 273 and again 549 tiles on one context: group totals handed up (more than 256
    tiles), persistent workgroups (more tiles than are resident), bucket starts above 2^21"""
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        s = Keyed(ctx, gs4d, oracle, hc._uniform(hc.LOOKBACK_N, hc.span_for(24), 548), 24)
        for tiles, n in hc.lookback_sizes():
            tc = s.top_counts(n)
            assert tc.max() <= hc.TAIL_TILE
            print(f"{tiles} tiles, n = {n}, largest bucket {tc.max()}")
            ran(s.sort(n, what=f"{tiles} tiles,"), slow=0, largest=int(tc.max()))
        ctx.finish()
    finally:
        ctx.close()


def test_the_top_pass_at_273_tiles_of_descending_keys(gs4d, oracle, monkeypatch):
    """every tile is one or two top digits: tile words and group totals of a digit as large as they come, every key crosses the whole array"""
    n = 272 * hc.TOP_TILE + 1
    ctx = _hybrid_ctx(gs4d, monkeypatch)
    try:
        s = Keyed(ctx, gs4d, oracle, hc.descending(n), 24)
        tc = s.top_counts()
        for k in range(2):
            ran(s.sort(what=f"sort {k},"), slow=0, largest=int(tc.max()))
        ctx.finish()
    finally:
        ctx.close()


# ---- h. epoch wrap -----------------------------------------------------------------------------------------------------------------------------------
def test_hybrid_sorts_across_the_epoch_wrap(gs4d, oracle, monkeypatch):
    """GS4D_TEST_EPOCH0 starts the launch counter 16 launches before the wrap of the 18-bit tile-word epoch; a hybrid sort is one launch of the pass
    kernel, so 24 sorts of 33 tiles cross it: the words are cleared once and the look-back goes on."""
    old = os.environ.get("GS4D_TEST_EPOCH0")
    os.environ["GS4D_TEST_EPOCH0"] = str(0x3FFF0)
    try:
        ctx = _hybrid_ctx(gs4d, monkeypatch)
        try:
            n = 32 * hc.TOP_TILE + 5
            s = Keyed(ctx, gs4d, oracle, hc._uniform(n, hc.span_for(24), 33), 24)
            for k in range(24):
                ran(s.sort(what=f"sort {k} of 24,"), slow=0)
            ctx.finish()
        finally:
            ctx.close()
    finally:
        if old is None:
            del os.environ["GS4D_TEST_EPOCH0"]
        else:
            os.environ["GS4D_TEST_EPOCH0"] = old


# ---- i. the neighbours caller ------------------------------------------------------------------------------------------------------------------------
NB_SETTINGS = {"default": {}, "hybrid_off": {"GS4D_SORT_HYBRID": 0}, "hybrid_on_cap_64": {"GS4D_SORT_HYBRID": 1, "GS4D_SORT_TAILCAP": 64}}
_nb_tables = {}                                                 # setting -> the three tables it gave


@functools.lru_cache(maxsize=None)
def _nb_expected():
    """the calls of test_gpu_neighbours' n = 70001 test and what they must give, computed once: [(form, flags, expected table)], the lattice's table"""
    n, dense = nc.N_BIG, nc.dense_case()
    calls = []
    for form, flags in (("rule", nc.COUNT_SELF | nc.SKIP_HIDDEN), ("all", nc.SKIP_DEAD)):
        source, rule, invert = nc.selection(n, form)
        calls.append((form, flags, nc.host(dense.rec, dense.t, dense.r, 3, flags, nc.table("random", n), source, rule, invert)))
    c = nc.lattice_counts(n)
    lattice = np.zeros(n, nc.STAT)
    lattice["pixels"], lattice["wmax"], lattice["wsum"] = c, np.where(c > 0, nc.ONE_BITS, 0), c.astype(np.uint64) << np.uint64(24)
    return calls, lattice


@pytest.mark.parametrize("setting", list(NB_SETTINGS))
def test_count_neighbours_with_the_hybrid_on_and_off(gs4d, monkeypatch, setting):
    """gs4d_count_neighbours sorts kb + 1 = 19 key bits (local digits of 5 + 5 bits) on the lane's pair_sort scratch, with k_os_hist as the producer
    and bias 0.  Unset and with GS4D_SORT_HYBRID=0 that is the LSD passes; with GS4D_SORT_HYBRID=1 and a capacity of 64 the first call is the hybrid
    with nearly every bucket on the slow path, and its report turns the next two into LSD sorts that count the top digit beside their rows.  Three
    calls in a row on one context; every table byte-equal to the expectation of test_gpu_neighbours and to the other settings'.
    (gs4d_get_sort_stats counts the depth-sort scratches only: which sort ran here is not visible to the test.)"""
    n = nc.N_BIG
    assert nc.bucket_bits(n) + 1 in hc.WIDTHS and hc.edges(nc.bucket_bits(n) + 1)[1:3] == (5, 5) and n >= 32768
    calls, lattice = _nb_expected()
    for k in ("GS4D_SORT_HYBRID", "GS4D_SORT_TAILCAP"):
        monkeypatch.delenv(k, raising=False)
    ctx = _ctx(gs4d, nc.W, nc.H, monkeypatch, **NB_SETTINGS[setting])
    try:
        dense = nc.dense_case()
        data, stats, src = ctx.buffer(dense.rec), ctx.buffer(nbytes=16 * n), ctx.buffer(nbytes=16 * n)
        got = []
        for form, flags, want in calls:
            source, rule, invert = nc.selection(n, form)
            if source is not None:
                ctx.subdata(src, source)
            ctx.subdata(stats, nc.table("random", n))
            kw = ec.rule_keywords(rule, invert) if source is not None else {}
            ctx.count_neighbours(stats, n, data, source=src if source is not None else None, query=nc.struct(dense.t, dense.r, 3, flags), **kw)
            got.append(ctx.read(stats, nc.STAT, n))
            assert got[-1].tobytes() == want.tobytes(), f"{setting}, dense, {form}: rows {np.flatnonzero(got[-1] != want)[:8]}"
        case = nc.case("lattice", n)
        ldata, lstats = ctx.buffer(case.rec), ctx.record_stats(n)
        ctx.count_neighbours(lstats, n, ldata, case.r)
        got.append(ctx.read(lstats, nc.STAT, n))
        assert got[-1].tobytes() == lattice.tobytes(), f"{setting}, lattice: rows {np.flatnonzero(got[-1] != lattice)[:8]}"
        ctx.finish()
    finally:
        ctx.close()
    _nb_tables[setting] = got
    for other, tables in _nb_tables.items():
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, tables)), f"{setting} and {other} differ"

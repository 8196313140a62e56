"""gs4d_label_components and gs4d_count_labels (include/gs4d.h) restated in numpy, and the record sets of their tests.

Test infrastructure only (tests/test_components_host.py pins the host definitions to the restatement on the CPU and asserts the premises of the GPU
cases; tests/test_gpu_components.py runs the device calls against the host definitions).  The pieces of the definition that gs4d_count_neighbours
shares — takes_part, the near matrix, the selection, the tables — are neighbour_cases'.  The components are restated as a plain label
propagation to the fixed point: every member takes the smallest label among itself and its near members, then every label is replaced by its
label's label, until nothing moves.  No union–find: the restatement shares no text with the code under test.
"""
import functools
import importlib

import numpy as np

import edit_cases as ec
import neighbour_cases as nc

f32 = np.float32
NONE = 0xFFFFFFFF                                         # GS4D_ID_NONE
NOCAP = 0xFFFFFFFF
SIZES = nc.SIZES                                          # 1, 2, 63, 64, 65, 257, 4097
EXTRA = nc.EXTRA
W, H = nc.W, nc.H
SKIP_HIDDEN, SKIP_DEAD = 1, 2                             # GS4D_CC_*
STAT = nc.STAT
ONE_BITS = nc.ONE_BITS
N_BIG = nc.N_BIG
ABOVE_ONE = float(np.nextafter(f32(1.0), f32(2.0)))      # the next float32 above 1
SENTINEL_WORD = 0xA5A5A5A5


def _gs4d():
    return importlib.import_module("4dgaussiansplatrendering_amd")


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------------
def members(rec, t, flags, source=None, rule=nc.RULE, invert=False):
    """(member [n] bool, m [n, 3])"""
    part, m = nc.takes_part(rec, t, flags)
    return part & ec.selected(part.shape[0], source, rule, invert), m


def propagate(near, member):
    """labels [n] uint32 of the graph near & member x member: the smallest member index of each component, NONE for a non-member"""
    n = member.shape[0]
    ei, ej = np.nonzero(near & member[:, None] & member[None, :])      # (row-major: ei ascends)
    starts = np.flatnonzero(np.r_[True, ei[1:] != ei[:-1]]) if ei.size else np.zeros(0, np.int64)
    rows = ei[starts]
    lab = np.arange(n, dtype=np.int64)
    while True:
        new = lab.copy()
        if rows.size:                                           # the smallest label among a member and its near members
            new[rows] = np.minimum(lab[rows], np.minimum.reduceat(lab[ej], starts))
        while True:                                             # labels of labels: a label names a member of the same component
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(member, lab, NONE).astype(np.uint32)


def add_fragments(table, rows, c):
    """a copy of `table` with c[k] fragments of weight 1 added to row rows[k]"""
    out = np.array(table, STAT, copy=True)
    add = np.asarray(c).astype(np.uint64)
    out["pixels"][rows] = (out["pixels"][rows].astype(np.uint64) + add).astype(np.uint32)          # (mod 2^32, as the device's)
    out["wmax"][rows] = np.maximum(out["wmax"][rows], ONE_BITS)
    out["wsum"][rows] = out["wsum"][rows] + (add << np.uint64(24))                                 # (mod 2^64)
    return out


def restate(rec, t, r, cap, flags, table=None, source=None, rule=nc.RULE, invert=False, near=None):
    """(labels, the table after the call or None)"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 24)
    member, m = members(rec, t, flags, source, rule, invert)
    if near is None:
        near = nc.near_matrix(m, r)[0]
    labels = propagate(near, member)
    if table is None:
        return labels, None
    rows = np.flatnonzero(member)
    own = labels[rows].astype(np.int64)
    size = np.bincount(own, minlength=rec.shape[0] + 1)
    return labels, add_fragments(table, rows, np.minimum(size[own], int(cap)))


def restate_count_labels(labels, seeds, rule, invert, table, n=None):
    labels = np.asarray(labels, np.uint32)
    n = labels.shape[0] if n is None else n
    lab = labels[:n].astype(np.int64)
    ok = lab < n
    hit = np.zeros(n + 1, bool)
    hit[lab[ok & ec.selected(n, seeds, rule, invert)]] = True
    rows = np.flatnonzero(ok & hit[np.where(ok, lab, n)])
    return add_fragments(table, rows, np.ones(rows.size, np.int64))


def component_sizes(labels):
    """the sizes of the components, ascending"""
    lab = np.asarray(labels)
    return np.sort(np.unique(lab[lab != NONE], return_counts=True)[1]).tolist()


def struct(t, r, cap, flags):
    q = _gs4d().ComponentQuery()
    q.t, q.radius, q.cap, q.flags = float(f32(t)), float(f32(r)), int(cap), int(flags)
    return q


def host(rec, t, r, cap, flags, table=None, source=None, rule=nc.RULE, invert=False):
    """gs4d_host_label_components through the binding: (labels, the table after the call as STAT, or None)"""
    kw = ec.rule_keywords(rule, invert) if source is not None else {}
    labels, st = _gs4d().label_components_host(rec, source=source, query=struct(t, r, cap, flags), stats=table, with_stats=table is not None, **kw)
    return labels, None if st is None else st.view(STAT)


def host_count_labels(labels, seeds, rule, invert, table, n=None):
    return _gs4d().count_labels_host(labels, seeds, stats=table, n=n, **ec.rule_keywords(rule, invert)).view(STAT)


# ---- record sets -------------------------------------------------------------------------------------------------------------------------------------
def plain_records(pos):
    """static 3D records at the positions, every one visible and alive: the centre at any time is the position, bit for bit"""
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    rec = np.zeros((pos.shape[0], 24), f32)
    rec[:, 0:3] = pos
    rec[:, 4:8] = (0.5, 0.25, 0.75, 0.9)
    rec[:, 8], rec[:, 13], rec[:, 18], rec[:, 23] = 1.0, 1.0, 1.0, 1.0
    return rec


def order_of(n, order, seed=0x4343):
    """perm [n]: the record index of the k-th position along a chain"""
    if order == "ascending":
        return np.arange(n)
    if order == "descending":
        return np.arange(n)[::-1].copy()
    return np.random.default_rng(seed + n).permutation(n)


ORDERS = ("ascending", "descending", "shuffled")


def chain_positions(n, gap):
    """n positions 0.9 r apart on a line (r = 1): x = float32(0.9 k).  gap: the line is bent twice, a third and two thirds along — the first bend
    is a step of exactly r on y (dx = 0, dy = 1.0f: the pair links), the second a step of the next float32 above r on z (dz = 1 + 2^-23, whose
    square rounds to 1 + 2^-22 > r * r: the pair does not link).  Returns (pos [n, 3], pieces: the number of positions before each bend)."""
    if not gap or n < 2:
        return np.stack([(0.9 * np.arange(n)).astype(f32), np.zeros(n, f32), np.zeros(n, f32)], 1), (n, n)
    a = max(1, n // 3)
    b = max(a, (2 * n) // 3) if n >= 3 else a               # positions before the second bend (n == 2: the exact bend is left out)
    k = np.arange(n)
    step = k - (k >= a) - ((k >= b) & (b > a))              # x stays where it was across a bend
    x = (0.9 * step).astype(f32)
    y = np.where((k >= a) & (b > a), f32(1.0), f32(0.0)).astype(f32)
    z = np.where(k >= b, f32(ABOVE_ONE), f32(0.0)).astype(f32)
    return np.stack([x, y, z], 1), (a, b)


class Scenario:
    """a record set with the call it is meant for: case (neighbour_cases.Case: rec, t, r), flags, the member selection (source, rule, invert) or
    None, and — where the construction gives them — the sizes of the components, ascending"""

    def __init__(self, name, rec, t, r, flags=0, selection=None, sizes=None):
        self.name, self.case, self.flags = name, nc.Case(name, rec, t, r), flags
        self.selection = selection if selection is not None else (None, nc.RULE, False)
        self.sizes = None if sizes is None else sorted(sizes)

    n = property(lambda self: self.case.n)

    def __repr__(self):
        return f"Scenario({self.name}, n = {self.n})"


def _place(pos, perm):
    """records such that record perm[k] sits at pos[k]"""
    out = np.empty_like(pos)
    out[perm] = pos
    return plain_records(out)


@functools.lru_cache(maxsize=None)
def chain(n, order, gap=False):
    pos, (a, b) = chain_positions(n, gap)
    sizes = [n] if not gap or n < 2 else [b, n - b]
    return Scenario(f"chain-{order}{'-gap' if gap else ''}", _place(pos, order_of(n, order)), 0.0, 1.0, sizes=sizes)


@functools.lru_cache(maxsize=None)
def clump(n=256):
    """n records within r / 2 of each other (r = 1: a ball of diameter 0.49): every pair is an edge, all hooking onto one root"""
    d = nc._uniform3(n, 0x4351) - 0.5
    pos = 3.0 + 0.245 * d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 0.5)
    return Scenario("clump", plain_records(pos), 0.0, 1.0, sizes=[n])


@functools.lru_cache(maxsize=None)
def clumps(largest=64):
    """clumps of 1 .. largest records, each inside a ball of diameter 0.4 r, 10 r apart on a grid, their records interleaved in index"""
    owner = np.concatenate([np.arange(first, largest) for first in range(largest)])      # round k gives one record to each clump >= k
    n = owner.size
    centre = np.stack([owner % 8, (owner // 8) % 8, owner // 64], 1) * 10.0
    pos = centre + 0.2 * (nc._uniform3(n, 0x4352) - 0.5)
    return Scenario("clumps", plain_records(pos), 0.0, 1.0, sizes=list(range(1, largest + 1)))


@functools.lru_cache(maxsize=None)
def lattice(n, apart=False):
    """neighbour_cases' lattice, spacing exactly 0.5 — with r = 0.5 one component; apart: r the float32 below 0.5, and every record is alone"""
    c = nc.case("lattice", n)
    r = float(np.nextafter(f32(0.5), f32(0.0))) if apart else 0.5
    return Scenario("lattice-apart" if apart else "lattice", c.rec, 0.0, r, sizes=[1] * n if apart else [n])


def slab_labels(n, layers=5):
    """the labels of slabs(n): record i sits in layer i // side^2, `layers` layers make a slab, and the label is the first record of the slab"""
    side = int(np.ceil(n ** (1.0 / 3.0)))
    i = np.arange(n)
    return ((i // (side * side)) // layers * layers * side * side).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def slabs(n, layers=5):
    """the lattice cut into slabs of `layers` layers by gaps of 1.5 r on z (r = 0.5; every coordinate a small multiple of 2^-2: the sums are
    exact).  Inside a slab every record has an axis neighbour of smaller index at exactly r (i - 1, i - side or i - side^2), down to the slab's
    first; across a gap the distance is at least 0.75.  The labels are slab_labels(n)."""
    side = int(np.ceil(n ** (1.0 / 3.0)))
    i = np.arange(n)
    z = i // (side * side)
    pos = np.stack([(i % side) - side // 2, ((i // side) % side) - side // 2, z], 1).astype(np.float64) * 0.5
    pos[:, 2] += 0.25 * (z // layers)
    lab = slab_labels(n, layers)
    return Scenario("slabs", nc.static_records(pos), 0.0, 0.5, sizes=np.bincount(lab)[np.unique(lab)].tolist())


BODIES_T0, BODIES_T1 = 0.0, 1.0


@functools.lru_cache(maxsize=None)
def bodies(n, t):
    """two bodies, each a chain along x (r = 1): the first static at y = 0, the second at y = 0.9 at time 0 and moving 5 a unit of time on y
    (sig3 = (0, 5, 0), s44 = 1, mu_t = 0).  One component at BODIES_T0, two at BODIES_T1 (n >= 2)."""
    a = (n + 1) // 2
    k = np.arange(n)
    pos = np.stack([0.9 * np.where(k < a, k, k - a), np.where(k < a, 0.0, 0.9), np.zeros(n)], 1)
    rec = plain_records(pos)
    rec[a:, 21] = 5.0
    return Scenario(f"bodies-t{t:g}", rec, t, 1.0, sizes=[n] if t == BODIES_T0 or n < 2 else [a, n - a])


BRIDGES = ("hidden", "dead", "rule", "inverted")


@functools.lru_cache(maxsize=None)
def bridge(n, how, on=True):
    """a chain (ascending) whose middle record is no member: hidden (alpha -0, with SKIP_HIDDEN), dead at time 0 (with SKIP_DEAD), or not selected
    by the source table ("rule": the only failing row; "inverted": the only passing row of an inverted rule).  on=False: the same records with
    the skip flag off / no table — one component, which shows that the middle record is what separates them."""
    mid = n // 2
    rec = chain(n, "ascending").case.rec.copy()
    flags, selection = 0, None
    if how == "hidden":
        rec[mid, 7], flags = -0.0, SKIP_HIDDEN if on else 0
    elif how == "dead":
        rec[mid, 3], flags = 20.0, SKIP_DEAD if on else 0
    elif on:
        mask = np.ones(n, bool)
        mask[mid] = False
        selection = (ec.mask_table(mask ^ (how == "inverted"), nc.RULE), nc.RULE, how == "inverted")
    sizes = [n] if not on else [s for s in (mid, n - 1 - mid) if s > 0]
    return Scenario(f"bridge-{how}{'' if on else '-off'}", rec, 0.0, 1.0, flags, selection, sizes)


def generic(kind, n):
    """neighbour_cases' cube, clump, twins, far and 4d sets (hidden and dead records among them): no closed form, checked against the host"""
    c = nc.case(kind, n)
    return Scenario(kind, c.rec, c.t, c.r)


GENERIC = ("cube", "clump", "twins", "far", "4d")


def by_size(n):
    """every scenario of size n"""
    out = [chain(n, order, gap) for order in ORDERS for gap in (False, True)]
    out += [lattice(n), lattice(n, apart=True), bodies(n, BODIES_T0), bodies(n, BODIES_T1)]
    out += [bridge(n, how) for how in BRIDGES] + [generic(kind, n) for kind in GENERIC]
    return out


# (form, flags, cap, prefilled table or None: no table) of the calls every scenario gets beside its own
COMBOS = (("all", 0, NOCAP, False), ("all", 3, 3, True), ("rule", 0, 1, True), ("rule", 3, NOCAP, False), ("inverted", 1, 3, False),
          ("inverted", 2, 1, True), ("all", 0, NOCAP, None), ("rule", 3, 3, None))


def calls(sc):
    """(selection, flags, cap, prefilled) of every call of a scenario: its own call first — its flags, its selection, no cap, a zeroed table —
    then COMBOS with neighbour_cases' selections of its size"""
    yield sc.selection, sc.flags, NOCAP, False
    for form, flags, cap, prefilled in COMBOS:
        yield nc.selection(sc.n, form), flags, cap, prefilled


def table(prefilled, n):
    return None if prefilled is None else nc.table("random" if prefilled else "zero", n)


# ---- the two chains ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def floaters():
    """(rec, planted [25], r): a dense cube of 1000 records in [-10, 10]^3 (r = 4: about 30 neighbours each) and five clumps of 5 records 0.1 r
    apart, 500 away from everything, their indices spread through the set"""
    n, r = 1025, 4.0
    planted = np.array([100 + 200 * g + 3 * j for g in range(5) for j in range(5)])
    pos = np.zeros((n, 3))
    pos[np.setdiff1d(np.arange(n), planted)] = nc._uniform3(1000, 0x4353) * 20.0 - 10.0
    far = np.array([(500.0, 500.0, 500.0), (-500.0, 500.0, 0.0), (500.0, -500.0, 100.0), (-500.0, -500.0, -500.0), (0.0, 900.0, 0.0)])
    pos[planted] = np.repeat(far, 5, 0) + 0.1 * r * np.tile(np.arange(5), 5)[:, None] * np.array([1.0, 0.0, 0.0])
    return plain_records(pos), planted, r


@functools.lru_cache(maxsize=None)
def two_bodies():
    """(rec, first of the second body, r): 300 records in [-10, 10]^3 and 200 in the same cube moved 100 along x; r = 5"""
    pos = nc._uniform3(500, 0x4354) * 20.0 - 10.0
    pos[300:, 0] += 100.0
    return plain_records(pos), 300, 5.0

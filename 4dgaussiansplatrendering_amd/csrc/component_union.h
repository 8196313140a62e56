// component_union.h — the union–find of gs4d_label_components (include/gs4d.h) as plain C++ templates: the one text of `find` and
// `unite`.  csrc/components.hip runs it on the device, many threads at once (agent-scope atomics); host/gs4d_host.cpp runs it sequentially on plain
// words; tests/component_union_stress.cpp runs it from 16 std::threads over std::atomic.  The memory is a policy object M over an array of n parents:
//     uint32_t M::load(uint32_t x)                          the parent of x, read so that a value another thread has written is seen eventually
//     bool     M::cas(uint32_t x, uint32_t is, uint32_t to) parent[x] <- to iff it is `is`; whether it was
//     void     M::lower(uint32_t x, uint32_t v)             parent[x] <- min(parent[x], v), atomically
// Nodes are 0 .. n - 1; before the first call parent[x] == x for every node in use (a node that is not in use is never named).
//
// Three arguments (DESIGN.md §4 has them at length):
//   1. parent[x] <= x always.  It holds at the start; `unite` stores small < big into parent[big]; `lower` only lowers.  A non-root therefore has a
//      parent strictly below itself: there are no cycles, and `find` — every step goes to a smaller node — ends within n steps, whatever the other
//      threads do meanwhile.  Every value ever stored into parent[x] is a node of x's tree at that moment (the other root of an edge; an ancestor's
//      parent), and trees only merge: two nodes that once had one root have one root ever after.
//   2. Once every `unite` has returned, the trees are the connected components: a tree never leaves a component (only edges hook), and the two ends
//      of every edge share a tree from the moment their `unite` returns.  The smallest node m of a component has parent[m] <= m inside the component,
//      so parent[m] == m: m is never hooked, it is a root, and a tree has one root.  The final root is the component's smallest node — unique, though
//      the order of the hooks is not.
//   3. `unite` repeats only when its cas fails, and the cas on parent[big] fails only when big has stopped being a root: another thread's cas on the
//      same word succeeded (`lower` never touches a root: it is applied to a node whose parent was read to differ from it).  A node stops being a root
//      once, so there are at most n - 1 successes in all and a thread repeats at most n - 1 times.  Nobody holds a lock and nobody waits for a
//      particular thread: lock-free.  Lanes of one wave that contend on one root all leave the cas with an answer; the losers re-read and go on.
// Both loops carry the bound all the same — n + 1 trips — and report an overrun instead of spinning: a bug has to become a failed check.
#ifndef GS4D_COMPONENT_UNION_H
#define GS4D_COMPONENT_UNION_H

#include <stdint.h>
#include "hd.h"

namespace gs4d_union {

constexpr uint32_t OVERRUN = 0xFFFFFFFFu;        // what find returns when its trip bound ran out (no node: n < 0xFFFFFFFF)

// the root of x's tree.  Path halving on the way: a node whose grandparent differs from its parent is lowered to it (argument 1: still an ancestor).
template <class M>
GS4D_HD inline uint32_t find(M& mem, uint32_t x, uint32_t n) {
    for (uint64_t trips = 0; trips <= (uint64_t)n; ++trips) {
        const uint32_t p = mem.load(x);
        if (p == x) return x;
        if (p > x) return OVERRUN;                // (argument 1 says never: reported like an overrun, and no word beyond x is ever read)
        const uint32_t g = mem.load(p);
        if (g == p) return p;
        if (g > p) return OVERRUN;
        mem.lower(x, g);
        x = g;
    }
    return OVERRUN;
}

// one tree for a and b: the larger root goes under the smaller.  false: a trip bound ran out.
template <class M>
GS4D_HD inline bool unite(M& mem, uint32_t a, uint32_t b, uint32_t n) {
    for (uint64_t trips = 0; trips <= (uint64_t)n; ++trips) {
        a = find(mem, a, n);
        b = find(mem, b, n);
        if (a == OVERRUN || b == OVERRUN) return false;
        if (a == b) return true;
        const uint32_t big = a > b ? a : b, small = a > b ? b : a;
        if (mem.cas(big, big, small)) return true;
    }
    return false;
}

} // namespace gs4d_union
#endif

// components.hip — gs4d_label_components and gs4d_count_labels (include/gs4d.h): the connected components of a record set — members
// linked iff their time-conditioned centres are near in the sense of gs4d_count_neighbours — as one label per record (the smallest record index of
// the component) and, optionally, the component's size as rows of a record-statistics table; and the records whose label a seed selection touches.
// The definition is the brute-force double loop over the text of neighbour_query.h with a sequential union–find (gs4d_host_label_components); this
// file is built with the flags of neighbours.hip (no contraction).  The device finds the near pairs through the hashed grid of neighbours.hip, whose
// phases it calls as they are (launch_neighbour_grid: k_nb_keys with "source" read as "member", the stable sort, the memset, k_nb_buckets — the proof
// that the walk of at most 27 cells misses no near pair is DESIGN.md §4's), and joins them with a lock-free union–find whose parent array is `labels`
// itself (component_union.h: one text of find / unite, compiled here, by the host definition and by tests/component_union_stress.cpp).
//
// Why the result is unique although the order of the unions is not (component_union.h has the three arguments, DESIGN.md §4 at length):
//   1. parent[x] <= x always — unite stores the smaller root into the larger, halving only lowers (atomicMin) — so there are no cycles and find,
//      which goes to a smaller node with every step, ends within n steps whatever the other threads do.
//   2. The smallest index of a component is never hooked and every other root eventually is: the final root is the smallest index.
//   3. A CAS fails only because another CAS succeeded, and there are at most n - 1 successes: the loop is lock-free.  No thread or workgroup waits
//      for another, and lanes of one wave that contend on one root still make progress, because nobody holds a lock.
// Two traps.  Every read of a parent is an agent-scope relaxed atomic load, which is served by the L2 and not by the CU's L1: a plain load can keep
// returning a stale "x is a root" from L1 while the CAS at L2 keeps failing, and the loop would never end.  And every loop carries a hard trip bound
// all the same — n + 1 steps of find, n + 1 retries of unite; find also refuses a parent above its node: on overrun the thread raises the lane's
// error word (the device-side check gs4d_finish reports) and returns.  A bug becomes a failed check, not a hung machine.
//
// Launches on one stream behind the grid phases, no LDS, kernel boundaries are the only dependencies:
//   k_cc_init      one thread per sorted slot s: labels[index[s]] = index[s] for a member (bit kb of keys[s] clear), GS4D_ID_NONE otherwise.  The sort
//                  permutes 0 .. n - 1, so all n words are written.
//   k_cc_link      one thread per sorted slot that holds a member i (neighbour_grid.h: slot_source), walking its candidates (walk_candidates).  For
//                  every near candidate j < i it calls unite(i, j): each edge is handled once, by its larger endpoint.
//   k_cc_flatten   one thread per record: labels[i] = find(i) for a member, stored with atomicMin.  Roots no longer change here — every unite has
//                  returned at the kernel boundary — and every value a concurrent reader can meet in labels[i] is an ancestor of i (the old parent,
//                  a halved one, or the root itself), so the finds of the other threads still end at the same root.
//   with stats:    a memset of the keys array — dead by then — to zero as the size array; k_cc_sizes, integer atomicAdds into size[labels[i]], the
//                  lanes of a wave that hold the same label adding once between them (a few rounds of ballots: with one component that holds most
//                  of the set every add lands on one word otherwise, measured at 8 times the rest of the call); k_cc_rows, the row
//                  update (add_fragments) with c = min(cap, size[labels[i]]): row i belongs to one thread alone.
// gs4d_count_labels: a memset of n flag words; k_cl_seeds, one thread per record j whose row of `seeds` passes the rule: flag[labels[j]] = 1 (a relaxed
// atomic store of the same value by everybody, left out where a relaxed atomic load already shows it) iff labels[j] < n; k_cl_rows, the row
// update with c = 1 for every i with labels[i] < n and flag[labels[i]] set.
// Scratch: that of gs4d_count_neighbours (neighbour_scratch_words()), nothing more.  All byte offsets are 64-bit.  Nothing but the n labels, rows
// < n of stats and the scratch is written; records, source, seeds are only read, and only records / rows < n.
#include "gs4d_internal.h"
#include "neighbour_query.h"
#include "neighbour_grid.h"
#include "component_union.h"

namespace gs4d {

namespace un = gs4d_union;

// the parent array on the device (component_union.h's policy): reads that bypass the L1, a CAS and a min at the L2
struct DeviceParents {
    uint32_t* p;
    __device__ __forceinline__ uint32_t load(uint32_t x) const { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ bool cas(uint32_t x, uint32_t is, uint32_t to) { return atomicCAS(p + x, is, to) == is; }
    __device__ __forceinline__ void lower(uint32_t x, uint32_t v) { (void)atomicMin(p + x, v); }
};
__device__ __forceinline__ void cc_raise(uint32_t* err) { __hip_atomic_store(err, 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

__global__ __launch_bounds__(COMPONENTS_TILE) void k_cc_init(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ index, uint32_t n, int kb,
                                                             uint32_t* __restrict__ labels) {
    const uint64_t s = (uint64_t)blockIdx.x * COMPONENTS_TILE + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = index[s];
    if (i >= n) return;                                        // (the sort permutes 0 .. n - 1: never)
    labels[i] = (keys[s] >> kb) ? (uint32_t)GS4D_ID_NONE : i;
}

__global__ __launch_bounds__(COMPONENTS_TILE) void k_cc_link(uint32_t n, GridArgs a, const float4* __restrict__ cand, const uint2* __restrict__ table,
                                                             const uint32_t* __restrict__ keys, uint32_t* labels, uint32_t* err) {
    const uint64_t s0 = (uint64_t)blockIdx.x * COMPONENTS_TILE + threadIdx.x;
    uint32_t i;
    float m[3];
    if (s0 >= n || (keys[s0] >> a.kb) != 0u || !slot_source(cand, n, s0, i, m)) return;      // not a member
    DeviceParents parents{ labels };
    walk_candidates(m, a.g, a.kb, n, table, cand, [&](const float4 v) {
        const uint32_t j = __float_as_uint(v.w);
        if (j >= i) return true;                               // the edge belongs to its larger endpoint (and j == i is no edge)
        const float mj[3] = { v.x, v.y, v.z };
        if (!nb::near(m, mj, a.rr)) return true;
        if (un::unite(parents, i, j, n)) return true;
        cc_raise(err);
        return false;
    });
}

__global__ __launch_bounds__(COMPONENTS_TILE) void k_cc_flatten(uint32_t n, uint32_t* labels, uint32_t* err) {
    const uint64_t i = (uint64_t)blockIdx.x * COMPONENTS_TILE + threadIdx.x;
    if (i >= n) return;
    DeviceParents parents{ labels };
    if (parents.load((uint32_t)i) == (uint32_t)GS4D_ID_NONE) return;      // not a member (no index is GS4D_ID_NONE: n < 0xFFFFFFFF)
    const uint32_t root = un::find(parents, (uint32_t)i, n);
    if (root == un::OVERRUN) { cc_raise(err); return; }
    // the roots are final, so this is the last value of labels[i]; a reader that meets an earlier one meets an ancestor of i
    parents.lower((uint32_t)i, root);
}

constexpr int CC_SIZE_ROUNDS = 4;

__global__ __launch_bounds__(COMPONENTS_TILE) void k_cc_sizes(const uint32_t* __restrict__ labels, uint32_t n, uint32_t* __restrict__ size) {
    const uint64_t i = (uint64_t)blockIdx.x * COMPONENTS_TILE + threadIdx.x;
    const uint32_t l = i < n ? labels[i] : (uint32_t)GS4D_ID_NONE;
    // In-wave aggregation of equal labels, CC_SIZE_ROUNDS rounds of it: the lanes that hold the label of the first lane still to do are counted by
    // a ballot and that lane adds the count.  One component that holds most of the set puts every lane's add on one word otherwise, and a word
    // takes about 88 adds a microsecond (measured: DESIGN.md §9).  Whoever is left after the rounds — many small components in one wave — adds for
    // itself.  Every lane of the wave runs the loop: its condition is a ballot, the same in every lane.
    bool todo = l < n;
    for (int round = 0; round < CC_SIZE_ROUNDS; ++round) {
        const unsigned long long open = __ballot(todo);
        if (open == 0ull) return;
        const int first = __ffsll((long long)open) - 1;
        const uint32_t lf = (uint32_t)__shfl((int)l, first);
        const bool same = todo && l == lf;
        const unsigned long long mine = __ballot(same);
        if ((int)__lane_id() == first) (void)atomicAdd(size + lf, (uint32_t)__popcll(mine));
        todo = todo && !same;
    }
    if (todo) (void)atomicAdd(size + l, 1u);
}

__global__ __launch_bounds__(COMPONENTS_TILE) void k_cc_rows(const uint32_t* __restrict__ labels, uint32_t n, uint32_t cap, const uint32_t* __restrict__ size,
                                                             uint4* __restrict__ stats) {
    const uint64_t i = (uint64_t)blockIdx.x * COMPONENTS_TILE + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = labels[i];
    if (l >= n) return;
    const uint32_t c = size[l] < cap ? size[l] : cap;
    if (c != 0u) add_fragments(stats, i, c, WEIGHT_ONE_BITS);  // (a member counts itself: c >= 1)
}

hipError_t launch_label_components(hipStream_t st, SortScratch& sort, const void* records, size_t n, const gs4d_component_query& q,
                                   const gs4d_record_stat* source, const KeepRule& rule, uint32_t* scratch, uint32_t* labels, gs4d_record_stat* stats,
                                   uint32_t* err) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    static_assert(sizeof(gs4d_component_query) == 32, "the query is 32 bytes");
    static_assert((int)GS4D_CC_SKIP_HIDDEN == (int)GS4D_NB_SKIP_HIDDEN && (int)GS4D_CC_SKIP_DEAD == (int)GS4D_NB_SKIP_DEAD, "the skips are takes_part's");
    if (!n) return hipSuccess;
    NeighbourGrid g;
    hipError_t e = launch_neighbour_grid(st, sort, records, n, q.t, q.radius, q.flags, source, rule, scratch, 3, g);
    if (e != hipSuccess) return e;
    const GridArgs a{ q.t, q.flags, q.radius * q.radius, nb::grid(q.radius), g.kb };
    const dim3 grid((uint32_t)((n + COMPONENTS_TILE - 1) / COMPONENTS_TILE)), block(COMPONENTS_TILE);
    k_cc_init<<<grid, block, 0, st>>>(g.keys, g.index, (uint32_t)n, g.kb, labels);
    k_cc_link<<<grid, block, 0, st>>>((uint32_t)n, a, g.cand, g.table, g.keys, labels, err);
    k_cc_flatten<<<grid, block, 0, st>>>((uint32_t)n, labels, err);
    if ((e = hipGetLastError()) != hipSuccess || !stats) return e;
    // the keys are dead: their n words are the size array
    if ((e = hipMemsetAsync(g.keys, 0, sizeof(uint32_t) * n, st)) != hipSuccess) return e;
    k_cc_sizes<<<grid, block, 0, st>>>(labels, (uint32_t)n, g.keys);
    k_cc_rows<<<grid, block, 0, st>>>(labels, (uint32_t)n, q.cap, g.keys, (uint4*)stats);
    return hipGetLastError();
}

// ---- gs4d_count_labels ----
__global__ __launch_bounds__(COMPONENTS_TILE) void k_cl_seeds(const uint32_t* __restrict__ labels, uint32_t n, const uint4* __restrict__ seeds, KeepRule k,
                                                              uint32_t* flags) {
    const uint64_t j = (uint64_t)blockIdx.x * COMPONENTS_TILE + threadIdx.x;
    if (j >= n || !keep_row(seeds[j], k)) return;
    const uint32_t l = labels[j];
    // (the load only saves stores: many seeds of one component would otherwise queue on one word; a seed that still reads 0 stores the same 1)
    if (l < n && __hip_atomic_load(flags + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) __hip_atomic_store(flags + l, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(COMPONENTS_TILE) void k_cl_rows(const uint32_t* __restrict__ labels, uint32_t n, const uint32_t* __restrict__ flags,
                                                             uint4* __restrict__ stats) {
    const uint64_t i = (uint64_t)blockIdx.x * COMPONENTS_TILE + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = labels[i];
    if (l < n && flags[l] != 0u) add_fragments(stats, i, 1u, WEIGHT_ONE_BITS);
}

hipError_t launch_count_labels(hipStream_t st, const uint32_t* labels, size_t n, const gs4d_record_stat* seeds, const KeepRule& rule, uint32_t* flags,
                               gs4d_record_stat* stats) {
    if (!n) return hipSuccess;
    const hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t) * n, st);
    if (e != hipSuccess) return e;
    const dim3 grid((uint32_t)((n + COMPONENTS_TILE - 1) / COMPONENTS_TILE)), block(COMPONENTS_TILE);
    k_cl_seeds<<<grid, block, 0, st>>>(labels, (uint32_t)n, (const uint4*)seeds, rule, flags);
    k_cl_rows<<<grid, block, 0, st>>>(labels, (uint32_t)n, flags, (uint4*)stats);
    return hipGetLastError();
}

} // namespace gs4d

// neighbours.hip — gs4d_count_neighbours (include/gs4d.h): for every record of a set, how many records of a source set have their
// time-conditioned centre within r of its own, as rows of a record-statistics table.  The definition is the brute-force double loop over the text
// of neighbour_query.h, which the host definition compiles too; this file is built with the flags of centres.hip (round to nearest, no
// contraction, every product and sum rounded on its own).  The device gives that result from a hashed grid of cells of edge 2 R, R = r (1 + 2^-10):
// a pair that is near differs by less than R on every axis, so the cells of a record's neighbours lie in [cell(m - R), cell(m + R)] per axis — at
// most three cells, 27 in all, usually 8 (the argument: neighbour_query.h and DESIGN.md §4).
//
// Launches on one stream, no LDS, no workgroup ever waits for another (kernel boundaries are the only dependencies):
//   k_nb_keys<COL>     one thread per record: the pieces 0 (position, mu_t) and 5 (sig[3]) of the 96-byte record, COL only (GS4D_NB_SKIP_HIDDEN) the
//                      colour piece for the alpha, and the record's row of the source table.  A source — it takes part and its row passes the rule
//                      — gets the bucket of its cell as its key, kb bits; any other record gets a key with bit kb set — it sorts behind every source
//                      and is never looked up — whose low bits are the bucket of its cell too if it takes part (0 if not): the query kernel
//                      walks the records in sorted order, and records of one cell then sit in one wave.
//   the sort           radix_sort_pairs of the identity by key, kb + 1 bits, stable (sort.hip; on the lane's pair_sort scratch, which plans the LSD passes unless GS4D_SORT_HYBRID is set: then 19..27 key bits — 65537 records and more — take the MSD/LSD hybrid through k_os_hist).
//   the memset         the bucket table, 2^kb rows of {first, end}, to zero: an empty bucket is first == end.
//   k_nb_buckets       one thread per sorted slot s that holds a source j: the centre of record j again (two 16-byte loads at a scattered record,
//                      the same function on the same bits) stored as float4 {m.x, m.y, m.z, bits(j)} into cand[s]; and the marks: s is the first
//                      slot of its key -> table[key].first = s, the last -> table[key].end = s + 1.
//   k_nb_query<COL>    one thread per record, in SORTED order (neighbour_grid.h: slot_record, and why the sorted order pays).  A record that takes
//                      part walks its candidates (neighbour_grid.h: walk_candidates), applies `near`, leaves out j == i by index unless COUNT_SELF,
//                      and stops at cap.  Then the row update of k_count_centres (add_fragments): a plain 16-byte load, modify, store, scattered
//                      here — row i belongs to one thread alone, and the call has the table to itself (queue_on_lane's "out").
// Scratch (the lane's, neighbour_scratch_words()): cand 16 n bytes, the table 8 * 2^kb, keys and sorted indices 4 n each — 24 n bytes and the table,
// beside the sort's own.  All byte offsets are 64-bit.  Nothing but rows < n of the table `stats` and the scratch is written; records and source are
// only read, and only records / rows < n.
#include "gs4d_internal.h"
#include "neighbour_query.h"
#include "neighbour_grid.h"

namespace gs4d {

bool neighbour_radius_ok(float r) { return nb::radius_ok(r); }
int neighbour_bucket_bits(size_t n) { return nb::bucket_bits((uint64_t)n); }

template <bool COL>
__global__ __launch_bounds__(NEIGHBOURS_TILE) void k_nb_keys(const float4* __restrict__ rec, uint32_t n, GridArgs a, const uint4* __restrict__ source, KeepRule k,
                                                             uint32_t* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * NEIGHBOURS_TILE + threadIdx.x;
    if (i >= n) return;
    float m[3];
    const bool part = nb::takes_part(a.t, a.flags, grid_fields<COL>(rec, i), m);
    const bool src = part && (!source || keep_row(source[i], k));
    const uint32_t b = part ? nb::bucket(nb::cell(m[0], a.g.inv_h), nb::cell(m[1], a.g.inv_h), nb::cell(m[2], a.g.inv_h), a.kb) : 0u;
    keys[i] = src ? b : (1u << a.kb) | b;
}

__global__ __launch_bounds__(NEIGHBOURS_TILE) void k_nb_buckets(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ index, uint32_t n, GridArgs a,
                                                                const float4* __restrict__ rec, float4* __restrict__ cand, uint2* __restrict__ table) {
    const uint64_t s = (uint64_t)blockIdx.x * NEIGHBOURS_TILE + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = keys[s];
    if (key >> a.kb) return;                                   // not a source
    const uint32_t j = index[s];
    if (j >= n) return;                                        // (the sort permutes 0 .. n - 1: never)
    float m[3];
    (void)gs4d_centre::centre_at(a.t, grid_fields<false>(rec, j), m);
    cand[s] = make_float4(m[0], m[1], m[2], __uint_as_float(j));
    if (s == 0u || keys[s - 1u] != key) table[key].x = (uint32_t)s;
    if (s + 1u == n || keys[s + 1u] != key) table[key].y = (uint32_t)s + 1u;
}

template <bool COL>
__global__ __launch_bounds__(NEIGHBOURS_TILE) void k_nb_query(const float4* __restrict__ rec, uint32_t n, GridArgs a, uint32_t cap, const float4* __restrict__ cand,
                                                              const uint2* __restrict__ table, const uint32_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ index, uint4* __restrict__ stats) {
    const uint64_t s0 = (uint64_t)blockIdx.x * NEIGHBOURS_TILE + threadIdx.x;
    if (s0 >= n) return;
    uint32_t i;
    float m[3];
    if (slot_record<COL>(rec, n, a, cand, keys, index, s0, i, m) < SLOT_PART) return;
    const bool self = (a.flags & (uint32_t)GS4D_NB_COUNT_SELF) != 0u;
    uint32_t c = 0;
    walk_candidates(m, a.g, a.kb, n, table, cand, [&](const float4 v) {
        const float mj[3] = { v.x, v.y, v.z };
        if (!nb::near(m, mj, a.rr)) return true;
        if (!self && __float_as_uint(v.w) == i) return true;
        return ++c < cap;                                      // (cap >= 1)
    });
    if (c != 0u) add_fragments(stats, i, c, WEIGHT_ONE_BITS);
}

// the grid phases: keys, sort, memset, bucket table — what gs4d_count_neighbours and gs4d_label_components (components.hip) share
hipError_t launch_neighbour_grid(hipStream_t st, SortScratch& sort, const void* records, size_t n, float t, float radius, uint32_t flags,
                                 const gs4d_record_stat* source, const KeepRule& rule, uint32_t* scratch, int phases, NeighbourGrid& g) {
    const int kb = neighbour_bucket_bits(n);
    const GridArgs a{ t, flags, radius * radius, nb::grid(radius), kb };
    // the scratch, in the order of neighbour_scratch_words(): candidates (16-byte aligned: first), table, keys, sorted indices
    float4* const cand = (float4*)scratch;
    uint2* const table = (uint2*)(scratch + 4 * n);
    uint32_t* const keys = scratch + 4 * n + 2 * ((size_t)1 << kb);
    uint32_t* const index = keys + n;
    g = NeighbourGrid{ cand, table, keys, index, kb };
    const dim3 grid((uint32_t)((n + NEIGHBOURS_TILE - 1) / NEIGHBOURS_TILE)), block(NEIGHBOURS_TILE);
    const bool col = (flags & (uint32_t)GS4D_NB_SKIP_HIDDEN) != 0u;
    const float4* const rec = (const float4*)records;
    if (col) k_nb_keys<true><<<grid, block, 0, st>>>(rec, (uint32_t)n, a, (const uint4*)source, rule, keys);
    else k_nb_keys<false><<<grid, block, 0, st>>>(rec, (uint32_t)n, a, (const uint4*)source, rule, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || phases < 2) return e;
    // the stable sort of the identity by key: the first pass that moves keys makes the indices up
    if ((e = radix_sort_pairs(st, sort, keys, index, n, nullptr, kb + 1, false, true)) != hipSuccess || phases < 3) return e;
    if ((e = hipMemsetAsync(table, 0, sizeof(uint2) << kb, st)) != hipSuccess) return e;
    k_nb_buckets<<<grid, block, 0, st>>>(keys, index, (uint32_t)n, a, rec, cand, table);
    return hipGetLastError();
}

hipError_t launch_count_neighbours(hipStream_t st, SortScratch& sort, const void* records, size_t n, const gs4d_neighbour_query& q,
                                   const gs4d_record_stat* source, const KeepRule& rule, uint32_t* scratch, gs4d_record_stat* stats, int phases) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    static_assert(sizeof(gs4d_neighbour_query) == 32, "the query is 32 bytes");
    if (!n) return hipSuccess;
    NeighbourGrid g;
    const hipError_t e = launch_neighbour_grid(st, sort, records, n, q.t, q.radius, q.flags, source, rule, scratch, phases, g);
    if (e != hipSuccess || phases < 4) return e;
    const GridArgs a{ q.t, q.flags, q.radius * q.radius, nb::grid(q.radius), g.kb };
    const dim3 grid((uint32_t)((n + NEIGHBOURS_TILE - 1) / NEIGHBOURS_TILE)), block(NEIGHBOURS_TILE);
    const float4* const rec = (const float4*)records;
    if ((q.flags & (uint32_t)GS4D_NB_SKIP_HIDDEN) != 0u) k_nb_query<true><<<grid, block, 0, st>>>(rec, (uint32_t)n, a, q.cap, g.cand, g.table, g.keys, g.index, (uint4*)stats);
    else k_nb_query<false><<<grid, block, 0, st>>>(rec, (uint32_t)n, a, q.cap, g.cand, g.table, g.keys, g.index, (uint4*)stats);
    return hipGetLastError();
}

} // namespace gs4d

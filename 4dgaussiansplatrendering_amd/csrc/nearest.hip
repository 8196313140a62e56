// nearest.hip — gs4d_nearest_neighbours (include/gs4d.h): for every record of a set the k nearest records of a source set whose
// time-conditioned centre lies within r of its own, as a row of {record, dist2} hits in a table of the caller's stride, and — optionally — the
// number of hits and the squared distance of the last one as rows of a record-statistics table.  The definition is the brute-force double loop
// over the texts of neighbour_query.h and nearest_query.h, which the host definition compiles too; this file is built with the flags of
// neighbours.hip (round to nearest, no contraction).  The device finds the near pairs through the hashed grid of neighbours.hip, whose phases it
// calls as they are (launch_neighbour_grid: k_nb_keys, the stable sort, the memset, k_nb_buckets — the proof that the walk of at most 27 cells
// misses no near pair is DESIGN.md §4's).
//
// Why the rows are unique although the walk order is not: a candidate's key (bits(dist2), j) is unique per j, every near source is met exactly
// once (bucket_seen leaves out the second cell of a shared bucket), and the K smallest keys of a set do not depend on the order the set is
// inserted in.  Nothing is exchanged between threads: row i belongs to one thread alone.
//
// One launch on the stream behind the grid phases, no LDS, no workgroup waits for another:
//   k_nn_query<COL, K>   K in {4, 8, 16}, k rounded up to it; one thread per record, in SORTED order (neighbour_grid.h: slot_record; COL: with the
//                        colour piece for the alpha, GS4D_NN_SKIP_HIDDEN).  A record that takes part walks its candidates (neighbour_grid.h:
//                        walk_candidates).  No cap and no early exit: every candidate that is near (and is not i itself, unless INCLUDE_SELF)
//                        competes.  The K best live in registers as K 64-bit keys (nearest_query.h's insert, fully unrolled: no
//                        dynamically indexed private array, no scratch memory); once the list is full a candidate that does not beat the worst
//                        costs one 64-bit compare.  Then the row: slot pairs as 16-byte stores, the last slot of an odd k as an 8-byte store (the
//                        bytes past 8 k keep their contents), empty slots {GS4D_ID_NONE, +inf} included — a record that does not take part writes
//                        k of them.  Rows are scattered by i, like the row update of k_nb_query: the walk is what the sorted order pays for.  With
//                        a stats table, the row update (add_fragments) with the dist2 bits of the last hit as wmax.
// Scratch: that of gs4d_count_neighbours (neighbour_scratch_words()), nothing more.  All byte offsets are 64-bit.  Nothing but the first 8 k bytes
// of rows < n of hits, rows < n of stats and the scratch is written; records and source are only read, and only records / rows < n.
#include "gs4d_internal.h"
#include "nearest_query.h"
#include "neighbour_grid.h"

namespace gs4d {

namespace nn = gs4d_nearest;

// what only this query kernel is given beside the grid's arguments
struct NnRows { uint32_t k; uint64_t hit_stride; };

// the first k slots of a row from the K keys: low word = record, high word = bits(dist2)
template <int K>
__device__ __forceinline__ void nn_write_row(unsigned char* __restrict__ hits, uint64_t i, const NnRows& r, const uint64_t (&best)[K]) {
    unsigned char* const row = hits + i * r.hit_stride;
#pragma unroll
    for (int p = 0; p < K; p += 2) {
        if ((uint32_t)p + 1u < r.k)
            *(uint4*)(row + 8 * p) = make_uint4((uint32_t)best[p], (uint32_t)(best[p] >> 32), (uint32_t)best[p + 1], (uint32_t)(best[p + 1] >> 32));
        else if ((uint32_t)p < r.k)
            *(uint2*)(row + 8 * p) = make_uint2((uint32_t)best[p], (uint32_t)(best[p] >> 32));
    }
}

template <bool COL, int K>
__global__ __launch_bounds__(NEAREST_TILE) void k_nn_query(const float4* __restrict__ rec, uint32_t n, GridArgs a, NnRows r, const float4* __restrict__ cand,
                                                           const uint2* __restrict__ table, const uint32_t* __restrict__ keys,
                                                           const uint32_t* __restrict__ index, unsigned char* __restrict__ hits, uint4* __restrict__ stats) {
    const uint64_t s0 = (uint64_t)blockIdx.x * NEAREST_TILE + threadIdx.x;
    if (s0 >= n) return;
    uint64_t best[K];
#pragma unroll
    for (int p = 0; p < K; ++p) best[p] = nn::EMPTY;
    uint32_t i;
    float m[3];
    const SlotKind kind = slot_record<COL>(rec, n, a, cand, keys, index, s0, i, m);
    if (kind == SLOT_NONE) return;
    if (kind == SLOT_IDLE) { nn_write_row<K>(hits, i, r, best); return; }      // the empty row
    const bool self = (a.flags & (uint32_t)GS4D_NN_INCLUDE_SELF) != 0u;
    walk_candidates(m, a.g, a.kb, n, table, cand, [&](const float4 v) {
        const float mj[3] = { v.x, v.y, v.z };
        const float d2 = nn::dist2(m, mj);
        const uint32_t j = __float_as_uint(v.w);
        if (d2 <= a.rr && (self || j != i)) nn::insert<K>(best, nn::order_key(d2, j));      // near, and not i itself
        return true;
    });
    nn_write_row<K>(hits, i, r, best);
    if (!stats) return;
    // f hits, the last of them at bits(dist2) = last
    uint32_t f = 0, last = 0;
#pragma unroll
    for (int p = 0; p < K; ++p)
        if ((uint32_t)p < r.k && best[p] != nn::EMPTY) { f = (uint32_t)p + 1u; last = (uint32_t)(best[p] >> 32); }
    if (f != 0u) add_fragments(stats, i, f, last);
}

template <bool COL, int K>
static void nn_launch(hipStream_t st, const float4* rec, size_t n, const GridArgs& a, const NnRows& r, const NeighbourGrid& g, void* hits, gs4d_record_stat* stats) {
    const dim3 grid((uint32_t)((n + NEAREST_TILE - 1) / NEAREST_TILE)), block(NEAREST_TILE);
    k_nn_query<COL, K><<<grid, block, 0, st>>>(rec, (uint32_t)n, a, r, g.cand, g.table, g.keys, g.index, (unsigned char*)hits, (uint4*)stats);
}

hipError_t launch_nearest_neighbours(hipStream_t st, SortScratch& sort, const void* records, size_t n, const gs4d_nearest_query& q,
                                     const gs4d_record_stat* source, const KeepRule& rule, uint32_t* scratch, void* hits, size_t hit_stride,
                                     gs4d_record_stat* stats) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    static_assert(sizeof(gs4d_nearest_query) == 32 && sizeof(gs4d_neighbour_hit) == 8, "the query is 32 bytes, a hit 8");
    static_assert((int)GS4D_NN_SKIP_HIDDEN == (int)GS4D_NB_SKIP_HIDDEN && (int)GS4D_NN_SKIP_DEAD == (int)GS4D_NB_SKIP_DEAD, "the skips are takes_part's");
    if (!n) return hipSuccess;
    NeighbourGrid g;
    const uint32_t skips = q.flags & (uint32_t)(GS4D_NN_SKIP_HIDDEN | GS4D_NN_SKIP_DEAD);
    const hipError_t e = launch_neighbour_grid(st, sort, records, n, q.t, q.radius, skips, source, rule, scratch, 3, g);
    if (e != hipSuccess) return e;
    const GridArgs a{ q.t, q.flags, q.radius * q.radius, nb::grid(q.radius), g.kb };
    const NnRows r{ q.k, (uint64_t)hit_stride };
    const float4* const rec = (const float4*)records;
    const bool col = (q.flags & (uint32_t)GS4D_NN_SKIP_HIDDEN) != 0u;
    if (q.k <= 4u) { if (col) nn_launch<true, 4>(st, rec, n, a, r, g, hits, stats); else nn_launch<false, 4>(st, rec, n, a, r, g, hits, stats); }
    else if (q.k <= 8u) { if (col) nn_launch<true, 8>(st, rec, n, a, r, g, hits, stats); else nn_launch<false, 8>(st, rec, n, a, r, g, hits, stats); }
    else { if (col) nn_launch<true, 16>(st, rec, n, a, r, g, hits, stats); else nn_launch<false, 16>(st, rec, n, a, r, g, hits, stats); }
    return hipGetLastError();
}

} // namespace gs4d

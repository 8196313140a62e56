// neighbour_grid.h — the device side of the hashed grid that launch_neighbour_grid (neighbours.hip) leaves in the lane's scratch: the one text of how
// a kernel obtains the record of a sorted slot and of how it walks the candidates of a centre.  k_nb_query (neighbours.hip), k_cc_link
// (components.hip) and k_nn_query (nearest.hip) differ only in what they do with a candidate.  The pieces the host compiles too (takes_part, near,
// cell_range, bucket, bucket_seen) are neighbour_query.h's; the proof that the walk misses no near pair is there and in DESIGN.md §4.
// Include it after gs4d_internal.h and neighbour_query.h, in a file built without contraction.
#ifndef GS4D_NEIGHBOUR_GRID_H
#define GS4D_NEIGHBOUR_GRID_H

namespace gs4d {

namespace nb = gs4d_neighbour;

// what every kernel of the grid is given: the time and the GS4D_NB_* skips of takes_part (the callers' own flag bits ride along), rr = r * r
// rounded once, the cells, and kb — the table has 2^kb rows, bit kb of a key says "not a source"
struct GridArgs { float t; uint32_t flags; float rr; nb::Grid g; int kb; };

// what takes_part and centre_at read of record i: the 16-byte pieces 0 (position, mu_t) and 5 (sig[3]), COL only the colour piece for the alpha
template <bool COL>
__device__ __forceinline__ nb::Fields grid_fields(const float4* __restrict__ rec, uint64_t i) {
    const float4 p = rec[i * 6u], g = rec[i * 6u + 5u];
    const float alpha = COL ? rec[i * 6u + 1u].w : 0.0f;
    return nb::Fields{ { p.x, p.y, p.z }, p.w, alpha, { g.x, g.y, g.z }, g.w };
}

// ---- the record of a sorted slot ----
// The walking kernels run one thread per SORTED slot, not per record: the sort puts the records of one cell next to each other (k_nb_keys gives a
// record that is no source the bucket of its cell as low key bits too), so the lanes of a wave hold records of the same few cells, load the same
// table rows and walk the same candidate runs, which the memory system serves as broadcasts instead of 64 scattered loads (measured: DESIGN.md
// §4).  The price is that whatever a thread writes for its record is scattered by i.
// The source in slot s0, whose key the caller has found to be a source's (bit kb clear): k_nb_buckets left its centre and its index in cand[s0].
// False: no record (the sort permutes 0 .. n - 1: never).
__device__ __forceinline__ bool slot_source(const float4* __restrict__ cand, uint32_t n, uint64_t s0, uint32_t& i, float m[3]) {
    const float4 v = cand[s0];
    m[0] = v.x; m[1] = v.y; m[2] = v.z; i = __float_as_uint(v.w);
    return i < n;
}
// What slot s0 < n holds.  SLOT_NONE: no record (never; i is not an index then).  Otherwise i is the record: SLOT_IDLE, it does not take part;
// SLOT_PART, it takes part and m is its centre; SLOT_SOURCE, it is a source as well.  Any record but a source is loaded through the sorted index
// and asked.
enum SlotKind { SLOT_NONE, SLOT_IDLE, SLOT_PART, SLOT_SOURCE };
template <bool COL>
__device__ __forceinline__ SlotKind slot_record(const float4* __restrict__ rec, uint32_t n, const GridArgs& a, const float4* __restrict__ cand,
                                                const uint32_t* __restrict__ keys, const uint32_t* __restrict__ index, uint64_t s0, uint32_t& i, float m[3]) {
    if ((keys[s0] >> a.kb) == 0u) return slot_source(cand, n, s0, i, m) ? SLOT_SOURCE : SLOT_NONE;
    i = index[s0];
    if (i >= n) return SLOT_NONE;
    return nb::takes_part(a.t, a.flags, grid_fields<COL>(rec, i), m) ? SLOT_PART : SLOT_IDLE;
}

// ---- the walk ----
// Every source whose centre can be near m is shown to visit(float4 {centre, bits(index)}) exactly once, with others that `near` has to reject;
// visit returns false to end the walk.  The cells of the range of m (cell_range: at most three per axis, 27 in all, usually 8), z outermost, x
// innermost; per cell the bucket, the 8-byte table row {first, end} and the run of 16-byte candidates in slot order — the order of visits is fixed,
// which a visitor that stops early (k_nb_query's cap) relies on.
//   bucket_seen   two different cells of one range can share a bucket, and walking it twice would show its candidates twice: the bucket is walked
//                 for the first of them only.  Different cells that share a bucket otherwise only add candidates that are not near.
//   the clamp     a run ends at min(end, n): cand has n slots, and no table row may lead a load past them (k_nb_buckets writes end <= n: never).
// No LDS, few registers: the dependent loads (table row, then candidates) are hidden by the other waves of the SIMD — eight of them, which
// 62 VGPRs allow and which more than 96 SGPRs do not: the visitor's verdict is therefore carried as a condition of all four loops.  A `return`
// out of the nest costs an exec mask per level, 97 to 99 SGPRs in all, and measured 6 to 11 % of k_nb_query and k_cc_link at 10^7 records
// (profiles/r07_grid_walk.md), although the compiler reports eight waves for both forms.
template <class Visit>
__device__ __forceinline__ void walk_candidates(const float m[3], const nb::Grid& g, int kb, uint32_t n, const uint2* __restrict__ table,
                                                const float4* __restrict__ cand, Visit visit) {
    int32_t lo[3], hi[3];
    nb::cell_range(m, g, lo, hi);
    bool go = true;
    for (int32_t cz = lo[2]; cz <= hi[2] && go; ++cz)
        for (int32_t cy = lo[1]; cy <= hi[1] && go; ++cy)
            for (int32_t cx = lo[0]; cx <= hi[0] && go; ++cx) {
                const uint32_t b = nb::bucket(cx, cy, cz, kb);
                if (nb::bucket_seen(lo, hi, cx, cy, cz, b, kb)) continue;
                const uint2 run = table[b];
                const uint32_t end = run.y < n ? run.y : n;
                for (uint32_t s = run.x; s < end && go; ++s) go = visit(cand[s]);
            }
}

} // namespace gs4d
#endif

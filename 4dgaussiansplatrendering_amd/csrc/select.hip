// select.hip — gs4d_count_ids: a region of a frame's ID planes {record, draw, weight} added into a record-statistics table, one fragment per
// pixel that takes part (include/gs4d.h).  One launch, no workgroup waits for another.
//
// A wave reads the rectangle in row segments of 64 pixels (the planes are linear: 256 contiguous bytes per plane and load) — SEL_WAVE_ROWS rows
// of one 64-pixel column band, SEL_BATCH rows loaded before the first is used; a workgroup of SEL_WAVES waves takes 64 x SEL_GROUP_ROWS pixels.
// The cost is contention, not bandwidth: one splat in front owns thousands of pixels, and each of them would fire three global atomics at the
// same 16-byte row.  So a wave aggregates before it touches memory (the shape of cut_count, cut.hip): the lanes that share the record of the
// first lane still to count are found with a ballot, their count, largest weight and 64-bit sum are reduced with shuffles, SEL_PEEL times a
// row; what is left after that goes one atomic set a lane.  A peeled group is not written at once: round k of the peel keeps it as the wave's
// CARRY k, and a group of the same record in the next row joins it — a uniform column band costs one atomic set a wave, and the border between
// two large splats one set a wave and side.  All three fields are integers (+, max, +): the table does not depend on the grid, on the order of
// the waves or on what was aggregated where.  GS4D_COUNT_IDS_PLAIN (a build-time switch for the measurement in DESIGN.md §4) turns the
// aggregation off: every pixel that takes part issues its own three atomics.
#include "gs4d_internal.h"

namespace gs4d {

constexpr uint32_t SEL_WAVES = 4, SEL_BATCH = 4, SEL_BATCHES = 4, SEL_WAVE_ROWS = SEL_BATCH * SEL_BATCHES, SEL_GROUP_ROWS = SEL_WAVES * SEL_WAVE_ROWS;
#ifdef GS4D_COUNT_IDS_PLAIN
constexpr int SEL_PEEL = 0;
#else
constexpr int SEL_PEEL = 2;
#endif

// what one or more fragments of one record add to its row; cnt == 0: nothing
struct SelGroup { uint32_t rec, cnt, wmax; uint64_t wsum; };

// exactly what the compositor's statistics flush issues per entry (composite_chunk, composite_common.h); the caller has checked g.rec < nrecords
__device__ __forceinline__ void sel_add(gs4d_record_stat* __restrict__ stats, const SelGroup& g) {
    gs4d_record_stat* const o = stats + g.rec;
    __hip_atomic_fetch_add(&o->pixels, g.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&o->wmax, g.wmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&o->wsum, g.wsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One fragment {rec, wbits, q} per lane with `in` (call with the whole wave converged; carry: wave-uniform).
__device__ __forceinline__ void sel_accumulate(gs4d_record_stat* __restrict__ stats, SelGroup* carry, uint32_t rec, uint32_t wbits, uint32_t q, bool in, uint32_t lane) {
    uint64_t todo = __ballot(in);
#pragma unroll
    for (int it = 0; it < SEL_PEEL; ++it) {
        if (!todo) break;                                            // (wave-uniform)
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const uint32_t rl = (uint32_t)__shfl((int)rec, lead, 64);
        const uint64_t same = __ballot(in && rec == rl) & todo;      // (lane `lead` is in it)
        const bool member = (same >> lane) & 1ull;
        uint32_t mx = member ? wbits : 0u;
        uint64_t sm = member ? (uint64_t)q : 0ull;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t omx = (uint32_t)__shfl_xor((int)mx, d, 64);
            const uint64_t osm = (uint64_t)__shfl_xor((unsigned long long)sm, d, 64);
            mx = omx > mx ? omx : mx;
            sm += osm;
        }
        SelGroup& cy = carry[it];
        if (cy.cnt != 0u && cy.rec == rl) { cy.cnt += (uint32_t)__popcll(same); cy.wmax = mx > cy.wmax ? mx : cy.wmax; cy.wsum += sm; }
        else {
            if (cy.cnt != 0u && lane == 0u) sel_add(stats, cy);
            cy = SelGroup{ rl, (uint32_t)__popcll(same), mx, sm };
        }
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) sel_add(stats, SelGroup{ rec, 1u, wbits, (uint64_t)q });
}

// ids: the planes record, draw, weight at ids, ids + P, ids + 2 P, rows of W words; g: a rectangle inside the image (validated on the host); mask:
// g.w * g.h bytes or null.  Lane l of a wave looks after column 64 * blockIdx.x + l of the rectangle: nothing outside it is read.
__global__ __launch_bounds__(SEL_WAVES * 64) void k_count_ids(const uint32_t* __restrict__ ids, size_t P, uint32_t W, gs4d_id_region g, const uint8_t* __restrict__ mask,
                                                               gs4d_record_stat* __restrict__ stats, uint32_t nrecords) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t col = blockIdx.x * 64u + lane, row0 = (blockIdx.y * SEL_WAVES + wave) * SEL_WAVE_ROWS;
    const uint32_t gw = (uint32_t)g.w, gh = (uint32_t)g.h;
    SelGroup carry[SEL_PEEL > 0 ? SEL_PEEL : 1];
#pragma unroll
    for (int k = 0; k < (SEL_PEEL > 0 ? SEL_PEEL : 1); ++k) carry[k] = SelGroup{ 0u, 0u, 0u, 0ull };
    for (uint32_t b = 0; b < SEL_BATCHES; ++b) {
        const uint32_t brow = row0 + b * SEL_BATCH;
        if (brow >= gh) break;                                       // (wave-uniform)
        uint32_t rec[SEL_BATCH], drw[SEL_BATCH], wt[SEL_BATCH], mk[SEL_BATCH];      // all rows of a batch are loaded before the first is used
#pragma unroll
        for (uint32_t i = 0; i < SEL_BATCH; ++i) {
            const uint32_t r = brow + i;
            const bool inside = col < gw && r < gh;
            const size_t o = (size_t)((uint32_t)g.y + r) * W + (uint32_t)g.x + col;
            rec[i] = inside ? ids[o] : GS4D_ID_NONE;
            drw[i] = inside ? ids[P + o] : 0u;
            wt[i] = inside ? ids[2 * P + o] : 0u;
            mk[i] = (inside && mask) ? (uint32_t)mask[(size_t)r * gw + col] : 1u;
        }
#pragma unroll
        for (uint32_t i = 0; i < SEL_BATCH; ++i) {
            const bool in = rec[i] != GS4D_ID_NONE && rec[i] < nrecords && drw[i] >= g.draw_first && drw[i] <= g.draw_last && wt[i] >= g.min_weight && mk[i] != 0u;
            // q of the record statistics (blend_fragment, composite_common.h): the same two float32 operations
            const uint32_t q = (uint32_t)rintf(__fmul_rn(__uint_as_float(wt[i]), 16777216.0f));
            sel_accumulate(stats, carry, rec[i], wt[i], q, in, lane);
        }
    }
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < SEL_PEEL; ++k) if (carry[k].cnt != 0u) sel_add(stats, carry[k]);
    }
}

hipError_t launch_count_ids(hipStream_t st, const uint32_t* ids, int W, int H, const gs4d_id_region& g, const uint8_t* mask, gs4d_record_stat* stats, uint32_t nrecords) {
    static_assert(sizeof(gs4d_id_region) == 32, "the region travels as a kernel argument");
    if (!nrecords || g.w <= 0 || g.h <= 0) return hipSuccess;
    const dim3 grid(((uint32_t)g.w + 63u) / 64u, ((uint32_t)g.h + SEL_GROUP_ROWS - 1u) / SEL_GROUP_ROWS);      // (images are 65535 pixels at most either way)
    k_count_ids<<<grid, dim3(SEL_WAVES * 64), 0, st>>>(ids, (size_t)W * H, (uint32_t)W, g, mask, stats, nrecords);
    return hipGetLastError();
}

} // namespace gs4d

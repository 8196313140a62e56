// measure.hip — gs4d_measure_records (include/gs4d.h): where a selection is — the counts, the box of the time-conditioned centres, the
// box of centre -/+ reach and the integer cell sums the centroid comes from, as one 96-byte gs4d_measure.  What a record adds is the text of
// measure_record.h, which the host definition compiles too; this file is built with the flags of shade.hip (round to nearest, no contraction, every
// product and sum rounded on its own, correctly rounded division and square root).
//
// Three launches on one stream, no workgroup ever waits for another (kernel boundaries are the only dependencies):
//   k_measure_box        up to MEASURE_GROUPS workgroups walk the records with a grid stride.  Per record a thread loads the statistics row first (16 B)
//                        and applies the rule; only for a selected record it loads the 16-byte pieces of the record the definition reads: 0 (position,
//                        mu_t), 5 (sig[3]), the diagonal pieces 2, 3 and 4, and piece 1 (the alpha) under GS4D_MS_SKIP_HIDDEN.  The three counters and
//                        the twelve keyed extrema are kept in registers, reduced across the wave with shuffles, across the waves in LDS — ONE partial
//                        row of 16 words per workgroup, plain stores;
//   k_measure_box_final  one workgroup folds the partial rows (a loop: any number of rows) the same way and writes bytes 0..63 of out — the keys
//                        turned back into floats — and zeroes bytes 64..95.  Sums of integers and extrema under a total order: the row does not
//                        depend on the grid, on the launch order or on which wave ran first;
//   k_measure_cells      the same walk with the box read from out: the cell of every measured centre, 64-bit sums per thread, the wave, LDS, one
//                        64-bit atomicAdd per workgroup and axis into out.cell_sum (integer addition is order-free).  It does not read the diagonal.
// Partials live in the lane's scratch (measure_scratch_words()).  All byte offsets are 64-bit.  Nothing but the 96 bytes of out and the scratch is
// written; records and table are only read, and only records and rows < n.  The kernels read the 96-byte records, never a SoA shadow: the diagonal
// lies in different planes of each shadow layout (gs4d.h).
#include "gs4d_internal.h"
#include "measure_record.h"

namespace gs4d {

namespace ms = gs4d_measure_rec;
constexpr uint32_t MS_WAVES = MEASURE_THREADS / 64;
static_assert(ms::ROW_WORDS == MEASURE_ROW_WORDS && sizeof(gs4d_measure) == 96 && offsetof(gs4d_measure, lo) == 4 * ms::ROW_LO &&
              offsetof(gs4d_measure, ext_hi) == 4 * ms::ROW_EXT_HI && offsetof(gs4d_measure, cell_sum) == 4 * ms::ROW_WORDS, "a row is the first 64 bytes of gs4d_measure");

struct MeasureSrc { const float4* rec; const uint4* stats; KeepRule rule; uint32_t n; float t; uint32_t flags; };

// whether record i is selected, and then what the definition reads of it (DIAG: the diagonal too)
template <bool DIAG>
__device__ __forceinline__ bool load_selected(const MeasureSrc& s, uint64_t i, ms::Fields& r) {
    if (s.stats && !keep_row(s.stats[i], s.rule)) return false;
    const float4* __restrict__ rec = s.rec + i * 6u;
    const float4 p = rec[0], g = rec[5];
    float alpha = 0.0f;
    if (s.flags & (uint32_t)GS4D_MS_SKIP_HIDDEN) alpha = rec[1].w;
    r.c = gs4d_centre::Fields{ { p.x, p.y, p.z }, p.w, alpha, { g.x, g.y, g.z }, g.w };
    if (DIAG) { r.diag[0] = rec[2].x; r.diag[1] = rec[3].y; r.diag[2] = rec[4].z; }
    return true;
}

// the rows of the calling workgroup's threads -> one row: word w is returned to thread w < ROW_WORDS (other threads: undefined)
__device__ __forceinline__ uint32_t reduce_row(uint32_t (&row)[ms::ROW_WORDS]) {
    __shared__ uint32_t part[MS_WAVES][ms::ROW_WORDS];
#pragma unroll
    for (int w = 0; w < ms::ROW_WORDS; ++w) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) row[w] = ms::row_join(w, row[w], __shfl_xor(row[w], d, 64));
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int w = 0; w < ms::ROW_WORDS; ++w) part[threadIdx.x >> 6][w] = row[w];
    }
    __syncthreads();
    uint32_t v = 0u;
    if (threadIdx.x < (uint32_t)ms::ROW_WORDS) {
        const int w = (int)threadIdx.x;
        v = part[0][w];
        for (uint32_t k = 1; k < MS_WAVES; ++k) v = ms::row_join(w, v, part[k][w]);
    }
    return v;
}

__global__ __launch_bounds__(MEASURE_THREADS) void k_measure_box(MeasureSrc s, uint32_t* __restrict__ partials) {
    uint32_t row[ms::ROW_WORDS];
#pragma unroll
    for (int w = 0; w < ms::ROW_WORDS; ++w) row[w] = ms::row_empty(w);
    for (uint64_t i = (uint64_t)blockIdx.x * MEASURE_THREADS + threadIdx.x; i < s.n; i += (uint64_t)gridDim.x * MEASURE_THREADS) {
        ms::Fields r;
        if (load_selected<true>(s, i, r)) ms::add_record(s.t, s.flags, r, row);
    }
    const uint32_t v = reduce_row(row);
    if (threadIdx.x < (uint32_t)ms::ROW_WORDS) partials[(uint64_t)blockIdx.x * ms::ROW_WORDS + threadIdx.x] = v;
}

// out: the 24 words of a gs4d_measure
__global__ __launch_bounds__(MEASURE_THREADS) void k_measure_box_final(const uint32_t* __restrict__ partials, uint32_t groups, uint32_t* __restrict__ out) {
    uint32_t row[ms::ROW_WORDS];
#pragma unroll
    for (int w = 0; w < ms::ROW_WORDS; ++w) row[w] = ms::row_empty(w);
    for (uint32_t g = threadIdx.x; g < groups; g += MEASURE_THREADS) {
#pragma unroll
        for (int w = 0; w < ms::ROW_WORDS; ++w) row[w] = ms::row_join(w, row[w], partials[(uint64_t)g * ms::ROW_WORDS + w]);
    }
    const uint32_t v = reduce_row(row);
    if (threadIdx.x < (uint32_t)ms::ROW_WORDS) out[threadIdx.x] = ms::row_word((int)threadIdx.x, v);
    else if (threadIdx.x < sizeof(gs4d_measure) / 4u) out[threadIdx.x] = 0u;         // cell_sum, reserved1
}

__global__ __launch_bounds__(MEASURE_THREADS) void k_measure_cells(MeasureSrc s, gs4d_measure* __restrict__ out) {
    __shared__ uint64_t part[MS_WAVES][3];
    if (out->count == 0u) return;                                // (uniform: nothing is measured, the sums stay 0)
    const float lo[3] = { out->lo[0], out->lo[1], out->lo[2] }, hi[3] = { out->hi[0], out->hi[1], out->hi[2] };
    uint64_t sum[3] = { 0ull, 0ull, 0ull };
    for (uint64_t i = (uint64_t)blockIdx.x * MEASURE_THREADS + threadIdx.x; i < s.n; i += (uint64_t)gridDim.x * MEASURE_THREADS) {
        ms::Fields r;
        float m[3];
        if (load_selected<false>(s, i, r) && ms::place(s.t, s.flags, r.c, m) == ms::MEASURED) {
#pragma unroll
            for (int a = 0; a < 3; ++a) sum[a] += ms::cell(m[a], lo[a], hi[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        uint32_t l = (uint32_t)sum[a], h = (uint32_t)(sum[a] >> 32);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t other = (uint64_t)__shfl_xor(l, d, 64) | ((uint64_t)__shfl_xor(h, d, 64) << 32);
            const uint64_t both = (((uint64_t)h << 32) | l) + other;
            l = (uint32_t)both; h = (uint32_t)(both >> 32);
        }
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][a] = ((uint64_t)h << 32) | l;
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        uint64_t v = part[0][threadIdx.x];
        for (uint32_t k = 1; k < MS_WAVES; ++k) v += part[k][threadIdx.x];
        if (v) atomicAdd((unsigned long long*)&out->cell_sum[threadIdx.x], (unsigned long long)v);
    }
}

hipError_t launch_measure_records(hipStream_t st, const void* records, size_t n, float t, uint32_t flags, const gs4d_record_stat* stats, const KeepRule& rule,
                                  uint32_t* scratch, gs4d_measure* out) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    const uint32_t groups = measure_groups(n);
    const MeasureSrc s{ (const float4*)records, (const uint4*)stats, rule, (uint32_t)n, t, flags };
    if (groups) k_measure_box<<<dim3(groups), dim3(MEASURE_THREADS), 0, st>>>(s, scratch);
    k_measure_box_final<<<dim3(1), dim3(MEASURE_THREADS), 0, st>>>(scratch, groups, (uint32_t*)out);
    if (groups) k_measure_cells<<<dim3(groups), dim3(MEASURE_THREADS), 0, st>>>(s, out);
    return hipGetLastError();
}

} // namespace gs4d

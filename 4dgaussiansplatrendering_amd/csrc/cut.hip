// cut.hip — gs4d_stat_cut: the k-th largest value of one field of a record-statistics table, with the number of rows above it and equal to it
// (include/gs4d.h).  A radix select, most significant digit first, CUT_DIGIT_BITS bits a digit: no sort, no permutation, nothing
// written but the caller's 16 bytes.
//
// Two launches per digit on one stream, no workgroup ever waits for another (kernel boundaries are the only dependencies):
//   k_cut_hist   up to CUT_GROUPS workgroups walk the table in tiles of CUT_TILE rows with a grid stride.  A row takes part iff the bits of its
//                field above the current digit equal the prefix chosen so far (the first digit: every row); the rows that take part are counted
//                by digit in an LDS histogram with integer LDS atomics, and each workgroup stores its CUT_BINS counts as ONE partial with plain
//                vector stores (no global atomics: the shape of k_order_box / k_order_box_final, reorder.hip);
//   k_cut_pick   one workgroup: sums the partials per bin, scans the bins from the top one down for the bin in which the remaining rank falls
//                and writes {prefix, rank remaining, above so far} to the state block for the next digit — or, after the last digit, the
//                caller's gs4d_cut (equal = the count of the last digit's bin).
// The state block lives in the lane's scratch, is written by a pick kernel and read by the kernels of the next digit only: the host never reads
// it.  Every sum is a sum of integers below 2^32 (n < 2^32): the result does not depend on the grid, on which workgroup or wave arrived first,
// or on anything else that varies between runs.  The field is taken as a uint64 throughout (pixels and wmax zero-extended).
#include "gs4d_internal.h"

namespace gs4d {

constexpr uint32_t CUT_THREADS = 256, CUT_ROUNDS = CUT_TILE / CUT_THREADS, CUT_PICK_THREADS = 1024, CUT_PICK_SLICES = CUT_PICK_THREADS / CUT_BINS;
static_assert(CUT_BINS == CUT_THREADS, "thread t of a histogram workgroup looks after bin t");
static_assert(CUT_TILE % CUT_THREADS == 0 && CUT_ROUNDS >= 2 && CUT_ROUNDS <= 16, "several rows per thread in flight");
static_assert(CUT_PICK_SLICES * CUT_BINS == CUT_PICK_THREADS && CUT_BINS % 64 == 0, "whole waves of bins, whole slices of partials");

struct CutState { uint64_t prefix; uint32_t rank, above; };      // the chosen digits so far; the rank still to go among the rows that carry them; rows above them
static_assert(sizeof(CutState) == CUT_STATE_WORDS * 4, "the state block of cut_scratch_words()");

__device__ __forceinline__ uint64_t cut_field(const uint4 row, int field) {          // gs4d_record_stat: pixels, wmax, wsum (little endian)
    return field == GS4D_STAT_PIXELS ? (uint64_t)row.x : field == GS4D_STAT_WMAX ? (uint64_t)row.y : ((uint64_t)row.z | ((uint64_t)row.w << 32));
}

// Adds one to h[d] for every lane with `in` (call with the whole wave converged).  The high digits of real tables take one or two values (the top
// bytes of wsum and pixels are zero): 64 LDS atomics on one address would queue up.  The lanes that share the digit of the first lane still to
// count are counted with a ballot and added by that lane, twice; what is left goes one atomic a lane.
__device__ __forceinline__ void cut_count(uint32_t* h, uint32_t d, bool in, uint32_t lane) {
    uint64_t todo = __ballot(in);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (!todo) return;                                           // (wave-uniform)
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const uint32_t dl = (uint32_t)__shfl((int)d, lead, 64);
        const uint64_t same = __ballot(in && d == dl) & todo;        // (lane `lead` is in it)
        if ((int)lane == lead) atomicAdd(&h[dl], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[d], 1u);
}

// shift: the position of the digit's lowest bit; first: the most significant digit (no prefix yet, the state block is not read)
__global__ __launch_bounds__(CUT_THREADS) void k_cut_hist(const uint4* __restrict__ stats, uint64_t n, uint32_t ntiles, int field, uint32_t shift, int first,
                                                          const CutState* __restrict__ state, uint32_t* __restrict__ partials) {
    __shared__ uint32_t h[CUT_BINS];
    h[threadIdx.x] = 0u;
    const uint64_t prefix = first ? 0ull : state->prefix;
    const uint32_t lane = threadIdx.x & 63u;
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t tile0 = (uint64_t)tile * CUT_TILE;
        uint4 row[CUT_ROUNDS];                                       // all rows of a thread are loaded before the first is used
#pragma unroll
        for (uint32_t r = 0; r < CUT_ROUNDS; ++r) {
            const uint64_t i = tile0 + r * CUT_THREADS + threadIdx.x;
            row[r] = i < n ? stats[i] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (uint32_t r = 0; r < CUT_ROUNDS; ++r) {
            const uint64_t f = cut_field(row[r], field);
            const bool in = tile0 + r * CUT_THREADS + threadIdx.x < n && (first || ((f >> shift) >> CUT_DIGIT_BITS) == prefix);      // (two shifts: shift + CUT_DIGIT_BITS is 64 for the first digit of wsum)
            cut_count(h, (uint32_t)(f >> shift) & (CUT_BINS - 1u), in, lane);
        }
    }
    __syncthreads();
    partials[(size_t)blockIdx.x * CUT_BINS + threadIdx.x] = h[threadIdx.x];
}

// k: the rank asked for (first digit only: min(budget, n) >= 1); last: write *out instead of the state.  Thread t sums bin t % CUT_BINS over the
// partials t / CUT_BINS, + CUT_PICK_SLICES, ...; the first CUT_BINS threads then take the bins from the top one down (thread t: bin CUT_BINS - 1 - t)
// through an inclusive scan: incl = rows whose digit is >= the thread's bin.  Among the rows that carry the prefix there are at least `rank`
// (the invariant of the selection, true at the start because k <= n), so exactly one bin has  incl - count < rank <= incl.
__global__ __launch_bounds__(CUT_PICK_THREADS) void k_cut_pick(const uint32_t* __restrict__ partials, uint32_t groups, uint32_t k, int first, int last,
                                                               CutState* __restrict__ state, gs4d_cut* __restrict__ out) {
    __shared__ uint32_t part[CUT_PICK_SLICES][CUT_BINS];
    __shared__ uint32_t wave_sum[CUT_BINS / 64];
    const uint32_t bin = threadIdx.x % CUT_BINS, slice = threadIdx.x / CUT_BINS;
    uint32_t s = 0;
    for (uint32_t g0 = slice; g0 < groups; g0 += 8u * CUT_PICK_SLICES) {               // eight loads in flight per thread
        uint32_t v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) { const uint32_t g = g0 + u * CUT_PICK_SLICES; v[u] = partials[(size_t)(g < groups ? g : g0) * CUT_BINS + bin]; }
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) if (g0 + u * CUT_PICK_SLICES < groups) s += v[u];
    }
    part[slice][bin] = s;
    const CutState before = first ? CutState{ 0ull, k, 0u } : *state;                // (read by every thread before the barrier; written after it)
    __syncthreads();
    const bool scans = threadIdx.x < CUT_BINS;                                        // (whole waves)
    const uint32_t mybin = (CUT_BINS - 1u - threadIdx.x) & (CUT_BINS - 1u), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t count = 0;
#pragma unroll
    for (uint32_t q = 0; q < CUT_PICK_SLICES; ++q) count += part[q][mybin];
    uint32_t incl = wave_incl_scan_u32(count, lane);
    if (scans && lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    if (!scans) return;
    for (uint32_t w = 0; w < wave; ++w) incl += wave_sum[w];
    const uint32_t excl = incl - count;
    if (excl < before.rank && before.rank <= incl) {
        const CutState after{ (before.prefix << CUT_DIGIT_BITS) | mybin, before.rank - excl, before.above + excl };
        if (last) { out->value = after.prefix; out->above = after.above; out->equal = count; }
        else *state = after;
    }
}

__global__ void k_cut_empty(gs4d_cut* __restrict__ out) { out->value = 0ull; out->above = 0u; out->equal = 0u; }

hipError_t launch_stat_cut(hipStream_t st, const gs4d_record_stat* stats, size_t n, int field, uint32_t k, uint32_t* scratch, gs4d_cut* out) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4) && sizeof(gs4d_cut) == 16, "a statistics row is one uint4; the result is 16 bytes");
    if (!n) { k_cut_empty<<<dim3(1), dim3(1), 0, st>>>(out); return hipGetLastError(); }
    const uint32_t ntiles = (uint32_t)((n + CUT_TILE - 1) / CUT_TILE), groups = cut_groups(n);
    const int passes = cut_passes(field);
    CutState* const state = (CutState*)scratch;
    uint32_t* const partials = scratch + CUT_STATE_WORDS;
    for (int p = 0; p < passes; ++p) {
        const uint32_t shift = (uint32_t)(passes - 1 - p) * CUT_DIGIT_BITS;
        k_cut_hist<<<dim3(groups), dim3(CUT_THREADS), 0, st>>>((const uint4*)stats, (uint64_t)n, ntiles, field, shift, p == 0, state, partials);
        k_cut_pick<<<dim3(1), dim3(CUT_PICK_THREADS), 0, st>>>(partials, groups, k, p == 0, p == passes - 1, state, out);
    }
    return hipGetLastError();
}

} // namespace gs4d

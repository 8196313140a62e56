// compact.hip — stable stream compaction of a record set by a table of one row per record (include/gs4d.h):
// gs4d_compact_records (16-byte statistics rows, KeepRule), gs4d_compact_time_window (8-byte time spans, WindowRule) and the last step of gs4d_lod_cut
// (1-byte node states, DrawRule; lod.hip) are the three instantiations of the same three kernels; k_time_spans, at the end, writes the table of the
// second (gs4d_record_time_spans).
//
// Three launches on one stream, no workgroup ever waits for another (kernel boundaries are the only dependencies):
//   k_compact_count    one workgroup per tile of COMPACT_TILE records: loads the table rows (16 bytes of statistics here; in general sizeof(Row)),
//                      evaluates the keep rule, counts the kept rows of the tile with wave ballots and stores ONE word per tile;
//   k_compact_scan     one workgroup: exclusive sum of the tile counts, in place (the words become the tiles' first destination slots), and the
//                      caller's gs4d_compact_count {kept, written};
//   k_compact_scatter  one workgroup per tile: evaluates the rule again (16 bytes per record read twice instead of a flag array written and
//                      read back), lists the tile's kept records in LDS in ascending order (ballot prefix within a wave, wave offsets within
//                      the workgroup) and copies them cooperatively in 16-byte pieces: the tile's destination is one contiguous, coalesced range.
// Every destination slot is compared against the capacity before it is stored; all byte offsets are 64-bit.
#include "gs4d_internal.h"

namespace gs4d {

constexpr uint32_t CT_THREADS = 256, CT_WAVES = CT_THREADS / 64, CT_ROUNDS = COMPACT_TILE / CT_THREADS;
static_assert(COMPACT_TILE >= 256 && COMPACT_TILE <= 4096 && (COMPACT_TILE & (COMPACT_TILE - 1)) == 0, "a power of two between 256 and 4096");
static_assert(CT_ROUNDS * CT_WAVES <= 64, "one wave scans the (round, wave) counts of a tile");

// (keep_row, the rule of either table: gs4d_internal.h)
// a row past the end of the table (never kept: keep_flags tests the index as well)
__device__ __forceinline__ uint4 zero_row(const uint4*) { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ float2 zero_row(const float2*) { return make_float2(0.0f, 0.0f); }
__device__ __forceinline__ uint8_t zero_row(const uint8_t*) { return (uint8_t)0; }

// Round r of a tile: thread t looks at local record r * CT_THREADS + t, so that a wave reads 1 KiB of consecutive rows and ascending
// (round, wave, lane) is ascending record order.  All rows of a thread are loaded before the first is used.
template <class Row, class Rule>
__device__ __forceinline__ void keep_flags(const Row* __restrict__ stats, uint64_t tile0, uint64_t n, const Rule k, bool (&keep)[CT_ROUNDS]) {
    Row row[CT_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CT_ROUNDS; ++r) {
        const uint64_t i = tile0 + r * CT_THREADS + threadIdx.x;
        row[r] = i < n ? stats[i] : zero_row(stats);
    }
#pragma unroll
    for (uint32_t r = 0; r < CT_ROUNDS; ++r) keep[r] = tile0 + r * CT_THREADS + threadIdx.x < n && keep_row(row[r], k);
}

template <class Row, class Rule>
__global__ __launch_bounds__(CT_THREADS) void k_compact_count(const Row* __restrict__ stats, uint64_t n, Rule k, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_total[CT_WAVES];
    bool keep[CT_ROUNDS];
    keep_flags(stats, (uint64_t)blockIdx.x * COMPACT_TILE, n, k, keep);
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t r = 0; r < CT_ROUNDS; ++r) mine += (uint32_t)__popcll(__ballot(keep[r]));      // wave-uniform
    if ((threadIdx.x & 63u) == 0u) wave_total[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0u) { uint32_t s = 0; for (uint32_t w = 0; w < CT_WAVES; ++w) s += wave_total[w]; counts[blockIdx.x] = s; }
}

// counts[0 .. ntiles) -> exclusive sums, in place; count[0] = {kept, min(kept, cap)}.  One workgroup of 1024 threads walks the array in
// rounds of 1024 words (10^7 records: 5 rounds).
__global__ __launch_bounds__(1024) void k_compact_scan(uint32_t* __restrict__ counts, uint32_t ntiles, uint32_t cap, uint2* __restrict__ count) {
    __shared__ uint32_t wave_sum[16];
    __shared__ uint32_t carry_s;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0u) carry_s = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < ntiles; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < ntiles ? counts[i] : 0u;
        const uint32_t incl = wave_incl_scan_u32(v, lane);
        if (lane == 63u) wave_sum[wave] = incl;
        const uint32_t carry = carry_s;
        __syncthreads();
        uint32_t before = carry;
        for (uint32_t w = 0; w < wave; ++w) before += wave_sum[w];
        if (i < ntiles) counts[i] = before + incl - v;
        if (threadIdx.x == 1023u) carry_s = before + incl;      // (everybody took the old carry before the barrier above)
        __syncthreads();
    }
    if (threadIdx.x == 0u) { const uint32_t kept = carry_s; *count = make_uint2(kept, kept < cap ? kept : cap); }
}

template <class Row, class Rule>
__global__ __launch_bounds__(CT_THREADS) void k_compact_scatter(const Row* __restrict__ stats, uint64_t n, Rule k, const uint32_t* __restrict__ bases,
                                                               const uint4* __restrict__ src, uint32_t q, uint4* __restrict__ dst, uint32_t* __restrict__ kept_index, uint32_t cap) {
    __shared__ uint32_t part[64];                  // kept rows of (round, wave), then their exclusive sums
    __shared__ uint32_t total_s;
    __shared__ uint16_t list[COMPACT_TILE];        // local indices of the tile's kept records, ascending
    const uint64_t tile0 = (uint64_t)blockIdx.x * COMPACT_TILE;
    const uint32_t base = bases[blockIdx.x];
    if (base >= cap) return;                       // (uniform) every slot of this tile lies beyond the capacity
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool keep[CT_ROUNDS];
    keep_flags(stats, tile0, n, k, keep);
    uint64_t mask[CT_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < CT_ROUNDS; ++r) {
        mask[r] = __ballot(keep[r]);
        if (lane == 0u) part[r * CT_WAVES + wave] = (uint32_t)__popcll(mask[r]);
    }
    __syncthreads();
    if (threadIdx.x < 64u) {
        const uint32_t v = threadIdx.x < CT_ROUNDS * CT_WAVES ? part[threadIdx.x] : 0u;
        const uint32_t incl = wave_incl_scan_u32(v, lane);
        part[threadIdx.x] = incl - v;
        if (threadIdx.x == 63u) total_s = incl;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < CT_ROUNDS; ++r)
        if (keep[r]) list[part[r * CT_WAVES + wave] + (uint32_t)__popcll(mask[r] & ((1ull << lane) - 1ull))] = (uint16_t)(r * CT_THREADS + threadIdx.x);
    __syncthreads();
    const uint32_t room = cap - base, total = total_s < room ? total_s : room;      // kept records of the tile whose slot is below the capacity
    if (kept_index)
        for (uint32_t j = threadIdx.x; j < total; j += CT_THREADS) kept_index[(uint64_t)base + j] = (uint32_t)(tile0 + list[j]);
    if (dst) {
        uint4* const out = dst + (uint64_t)base * q;                                 // pieces [0, total * q) of it are this tile's
        const uint32_t pieces = total * q;                                            // (<= 4096 * 64)
        for (uint32_t j0 = threadIdx.x; j0 < pieces; j0 += 4u * CT_THREADS) {          // four loads in flight per thread
            uint4 v[4];                                                                 // every element is loaded (a clamped address past the end): registers, no private memory
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t j = min(j0 + u * CT_THREADS, pieces - 1u);              // (j0 < pieces: there is a last piece)
                const uint32_t rec = j / q, piece = j - rec * q;
                v[u] = src[(tile0 + list[rec]) * q + piece];
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) { const uint32_t j = j0 + u * CT_THREADS; if (j < pieces) out[j] = v[u]; }
        }
    }
}

template <class Row, class Rule>
static hipError_t launch_compact_rows(hipStream_t st, const Row* table, size_t n, const Rule& rule, uint32_t* tile_counts,
                                      const void* src, size_t stride, void* dst, uint32_t* kept_index, uint32_t cap, gs4d_compact_count* count) {
    const uint32_t ntiles = (uint32_t)((n + COMPACT_TILE - 1) / COMPACT_TILE);
    if (ntiles) k_compact_count<Row, Rule><<<dim3(ntiles), dim3(CT_THREADS), 0, st>>>(table, (uint64_t)n, rule, tile_counts);
    k_compact_scan<<<dim3(1), dim3(1024), 0, st>>>(tile_counts, ntiles, cap, (uint2*)count);
    if (ntiles && cap && (dst || kept_index))
        k_compact_scatter<Row, Rule><<<dim3(ntiles), dim3(CT_THREADS), 0, st>>>(table, (uint64_t)n, rule, tile_counts, (const uint4*)src, (uint32_t)(stride / 16), (uint4*)dst, kept_index, cap);
    return hipGetLastError();
}

hipError_t launch_compact(hipStream_t st, const gs4d_record_stat* stats, size_t n, const KeepRule& rule, uint32_t* tile_counts,
                          const void* src, size_t stride, void* dst, uint32_t* kept_index, uint32_t cap, gs4d_compact_count* count) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    return launch_compact_rows(st, (const uint4*)stats, n, rule, tile_counts, src, stride, dst, kept_index, cap, count);
}
hipError_t launch_compact(hipStream_t st, const gs4d_time_span* spans, size_t n, const WindowRule& rule, uint32_t* tile_counts,
                          const void* src, size_t stride, void* dst, uint32_t* kept_index, uint32_t cap, gs4d_compact_count* count) {
    static_assert(sizeof(gs4d_time_span) == sizeof(float2), "a time span is one float2");
    return launch_compact_rows(st, (const float2*)spans, n, rule, tile_counts, src, stride, dst, kept_index, cap, count);
}
// gs4d_lod_cut's state plane: a row is one byte, a wave reads 64 consecutive bytes a round
hipError_t launch_compact(hipStream_t st, const uint8_t* states, size_t n, const DrawRule& rule, uint32_t* tile_counts,
                          const void* src, size_t stride, void* dst, uint32_t* kept_index, uint32_t cap, gs4d_compact_count* count) {
    return launch_compact_rows(st, states, n, rule, tile_counts, src, stride, dst, kept_index, cap, count);
}

// ---- gs4d_record_time_spans ----
// The draw's own expression (project_4d, preprocess.hip): the argument of the opacity's exponential at time t, in float32, round to nearest, no
// contraction (this file is built with the flags of preprocess.hip).  inv = 1.0f / s44, finite and positive.
__device__ __forceinline__ float time_arg(float t, float mu, float inv) {
    const float dt = t - mu;
    return -0.5f * dt * inv * dt;
}
// float32 <-> a uint32 in the order of the floats (-0 just below +0)
__device__ __forceinline__ uint32_t time_key(float t) { const uint32_t b = __float_as_uint(t); return (b & 0x80000000u) ? ~b : b | 0x80000000u; }
__device__ __forceinline__ float key_time(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k); }
// The last time, walking from mu towards `end` (+-FLT_MAX), whose argument is still >= GS4D_TIME_DEAD_ARG.  time_arg is monotone non-increasing in
// |t - mu| and 0 at mu: the alive times on this side are a run of consecutive keys from mu's, and its end is found by bisection —
// `a` alive, `d` dead, at most 32 halvings of a distance below 2^32.
__device__ __forceinline__ float time_edge(float mu, float inv, float end) {
    if (time_arg(end, mu, inv) >= GS4D_TIME_DEAD_ARG) return end;
    uint32_t a = time_key(mu), d = time_key(end);
    const bool up = d > a;
    for (int step = 0; step < 32 && (up ? d - a : a - d) > 1u; ++step) {
        const uint32_t m = up ? a + (d - a) / 2u : d + (a - d) / 2u;
        if (time_arg(key_time(m), mu, inv) >= GS4D_TIME_DEAD_ARG) a = m; else d = m;
    }
    return key_time(a);
}
// One thread per record: three floats of the 96-byte record in, one float2 out.
__global__ __launch_bounds__(256) void k_time_spans(const float* __restrict__ data, uint32_t n, float min_opacity, float2* __restrict__ spans) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* rec = data + (size_t)i * 24;
    const float mu = rec[3], cw = rec[7], s44 = rec[23];
    const float inv = 1.0f / s44;
    constexpr float INF = __builtin_huge_valf(), MAXF = 3.402823466e+38f;
    float2 span;
    if (!(cw > 0.0f)) span = make_float2(INF, -INF);                                              // never: alpha <= 0 or not finite
    else if (!(min_opacity <= 0.0f) || !(s44 > 0.0f && s44 < INF) || !(inv > 0.0f && inv < INF) || !(fabsf(mu) < INF)) span = make_float2(-INF, INF);      // always
    else span = make_float2(time_edge(mu, inv, -MAXF), time_edge(mu, inv, MAXF));
    spans[i] = span;
}

hipError_t launch_time_spans(hipStream_t st, const void* data, size_t n, float min_opacity, gs4d_time_span* spans) {
    if (n) k_time_spans<<<dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st>>>((const float*)data, (uint32_t)n, min_opacity, (float2*)spans);
    return hipGetLastError();
}

} // namespace gs4d

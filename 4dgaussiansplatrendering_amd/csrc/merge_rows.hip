// merge_rows.hip — gs4d_merge_rows and gs4d_copy_rows (include/gs4d.h): the mass-weighted mean of the members' rows of a float32 table
// per value of member_group — the SH row of a merged record — and the copy that lays a forest's rows out level by level.  The arithmetic is the text
// of merge_rows_record.h, which the host definition compiles too; this file is built with the flags of preprocess.hip (round to nearest, no
// contraction, correctly rounded division).
//
// gs4d_merge_rows is the segmented reduction of merge.hip over another payload, on one stream; no workgroup ever waits for another:
//   k_rows_keys      one thread per record: the member_group word first, then (with records) the record's six 16-byte pieces and its mass, then the
//                    row's 16-byte pieces that hold words below `width`; key = member_group[i] of a member, GS4D_ID_NONE otherwise; the mass goes
//                    to one scratch word per record (make lib ROWS_MASS_RECOMPUTE=1: it is not kept, and the reduction computes it again);
//   the sort         radix_sort_pairs of the identity by key, 32 bits, stable: every run of equal keys is in ascending record index;
//   the run starts   launch_merge_run_starts of merge.hip (k_merge_count, k_merge_scan, k_merge_heads), unchanged: start[r] = sorted slot of the
//                    first member of run r, the state block {runs, members}, and the caller's count with written = runs;
//   k_rows_written   one thread: the runs are in ascending key, so the ones whose row dst_first + key lies below the capacity are a prefix — a
//                    bisection of start[] gives their number, which replaces count.written;
//   k_rows_reduce    one sub-group of 8 lanes per (run, chunk of ROWS_CHUNK = 8 words of the row; make lib ROWS_CHUNK=4, 16 or 32: the sizes it
//                    was measured against).  Lane l walks members l, l + 8, ... of the run,
//                    gathers the chunk's 16-byte pieces of each member's row through the sorted index and adds them into its slot of ROWS_CHUNK + 1
//                    doubles, which stay in registers (the chunk is a compile-time size: no accumulator is indexed dynamically).  A butterfly
//                    of __shfl_xor over lane distances 1, 2 and 4 is the definition's tree in every lane.  Lanes 0 .. ROWS_CHUNK / 4 - 1 then
//                    each divide and store one 16-byte piece: a sub-group writes ROWS_CHUNK * 4 contiguous bytes.  The chunks cover the whole
//                    stride, so the words from `width` on are written as +0.0 by the same stores; a padding word that shares a piece with words
//                    below `width` is loaded and added but replaced by +0.0 before the store.  No LDS, no atomics, no private memory.
// Scratch (the lane's, merge_rows_scratch_words()): the layout of merge.hip, then the mass words.  All byte offsets are 64-bit.  No row >= capacity
// of dst is written; records, member_group and rows are only read, and only rows < n.
#include "gs4d_internal.h"
#include "merge_rows_record.h"
#include "record_tile.h"      // f32x4

namespace gs4d {

namespace mg = gs4d_merge;
namespace mr = gs4d_rows;
#ifndef GS4D_ROWS_CHUNK
#define GS4D_ROWS_CHUNK 8
#endif
constexpr uint32_t RW_THREADS = 256;
constexpr uint32_t RW_SUB = 8;                          // lanes of a sub-group: the slots of the definition
constexpr uint32_t RW_UNITS_PER_WG = RW_THREADS / RW_SUB;
constexpr uint32_t ROWS_CHUNK = GS4D_ROWS_CHUNK;        // words of a row one sub-group reduces
constexpr uint32_t CHUNK_PIECES = ROWS_CHUNK / 4;
static_assert(RW_SUB == (uint32_t)mr::SLOTS, "one lane per slot");
static_assert(ROWS_CHUNK % 4 == 0 && CHUNK_PIECES >= 1 && CHUNK_PIECES <= RW_SUB, "a lane of the sub-group stores one 16-byte piece of the chunk");
static_assert(sizeof(gs4d_rows_query) == 16 && sizeof(gs4d_merge_count) == sizeof(uint4), "the structures of gs4d.h");

__device__ __forceinline__ void load_record24(const f32x4* __restrict__ rec, uint64_t i, float r[24]) {
    const f32x4* const p = rec + i * 6u;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) { const f32x4 v = p[k]; r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w; }
}
// piece `piece` of row i
__device__ __forceinline__ f32x4 load_piece(const unsigned char* __restrict__ rows, uint64_t i, uint32_t stride, uint32_t piece) {
    return *(const f32x4*)(rows + i * (uint64_t)stride + (uint64_t)piece * 16u);
}
// the words of piece `piece` at or past `width` as +0.0
__device__ __forceinline__ f32x4 below_width(f32x4 v, uint32_t piece, uint32_t width) {
    const uint32_t w = piece * 4u;
    return f32x4{ w < width ? v.x : 0.0f, w + 1u < width ? v.y : 0.0f, w + 2u < width ? v.z : 0.0f, w + 3u < width ? v.w : 0.0f };
}

template <bool WEIGHTED>
__global__ __launch_bounds__(RW_THREADS) void k_rows_keys(const f32x4* __restrict__ rec, uint32_t n, const uint32_t* __restrict__ member_group,
                                                          const unsigned char* __restrict__ rows, uint32_t stride, uint32_t width,
                                                          uint32_t* __restrict__ keys, float* __restrict__ mass) {
    const uint64_t i = (uint64_t)blockIdx.x * RW_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t group = member_group[i];
    uint32_t key = mg::NONE;
    if (group != mg::NONE) {
        bool ok = true;
        if (WEIGHTED) {
            float r[24], a;
            load_record24(rec, i, r);
            ok = mg::member_mass(r, a);
            if (mass) mass[i] = a;
        }
        if (ok) {
            const uint32_t pieces = (width + 3u) / 4u;
            for (uint32_t p = 0; p < pieces; ++p) {
                const f32x4 v = below_width(load_piece(rows, i, stride, p), p, width);
                ok = ok && mg::finite(v.x) && mg::finite(v.y) && mg::finite(v.z) && mg::finite(v.w);
            }
            if (ok) key = group;
        }
    }
    keys[i] = key;
}

// *count holds {runs, runs, members, left_out}: written <- the runs whose key lies below `limit`, a prefix of the runs
__global__ void k_rows_written(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ start, const uint32_t* __restrict__ state, uint64_t limit,
                               uint4* __restrict__ count) {
    uint32_t lo = 0u, hi = state[0];                            // the first run whose key is >= limit
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if ((uint64_t)keys[start[mid]] < limit) lo = mid + 1u; else hi = mid; }
    count->y = lo;
}

__device__ __forceinline__ double xor_lane_f64(double v, int d) { return __shfl_xor(v, d, 64); }

template <bool WEIGHTED>
__global__ __launch_bounds__(RW_THREADS) void k_rows_reduce(const f32x4* __restrict__ rec, const float* __restrict__ mass, const unsigned char* __restrict__ rows,
                                                            uint32_t stride, uint32_t width, const uint32_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ index, const uint32_t* __restrict__ start,
                                                            const uint32_t* __restrict__ state, uint32_t chunks, uint64_t limit, uint64_t dst_first,
                                                            unsigned char* __restrict__ dst) {
    const uint32_t runs = state[0], members = state[1];
    const uint64_t unit = ((uint64_t)blockIdx.x * RW_THREADS + threadIdx.x) / RW_SUB;      // (the same in all eight lanes of a sub-group)
    const uint32_t l = threadIdx.x & (RW_SUB - 1u);
    const uint64_t run = unit / chunks;
    const uint32_t chunk = (uint32_t)(unit - run * chunks);
    bool live = run < runs;
    uint32_t first = 0u, end = 0u, group = 0u;
    if (live) { first = start[run]; group = keys[first]; live = (uint64_t)group < limit; }
    if (live) end = run + 1u < runs ? start[run + 1u] : members;
    const uint32_t size = end - first;
    const uint32_t piece0 = chunk * CHUNK_PIECES;               // the chunk's first piece of the row
    const uint32_t data_pieces = (width + 3u) / 4u;             // pieces that hold a word below width
    const uint32_t here = piece0 < data_pieces ? (data_pieces - piece0 < CHUNK_PIECES ? data_pieces - piece0 : CHUNK_PIECES) : 0u;
    double W = 0.0, R[ROWS_CHUNK];
#pragma unroll
    for (uint32_t j = 0; j < ROWS_CHUNK; ++j) R[j] = 0.0;
    f32x4 single = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    if (size == 1u) {
        if (l < here) single = load_piece(rows, index[first], stride, piece0 + l);      // a group of one member: its words as they are
    } else if (size > 1u && here != 0u) {
        for (uint64_t k = (uint64_t)first + l; k < end; k += RW_SUB) {
            const uint32_t i = index[k];
            float a = 1.0f;
            if (WEIGHTED) {
#ifdef GS4D_ROWS_MASS_RECOMPUTE
                float r[24];
                load_record24(rec, i, r);
                (void)mg::member_mass(r, a);                    // the mass the key kernel found finite and > 0
#else
                a = mass[i];
#endif
            }
            const double ad = (double)a;
            W += ad;
#pragma unroll
            for (uint32_t p = 0; p < CHUNK_PIECES; ++p) {
                if (p < here) {
                    const f32x4 v = load_piece(rows, i, stride, piece0 + p);
                    R[4 * p] += mr::term(ad, v.x); R[4 * p + 1] += mr::term(ad, v.y); R[4 * p + 2] += mr::term(ad, v.z); R[4 * p + 3] += mr::term(ad, v.w);
                }
            }
        }
    }
    // every lane of the wave takes part in the butterfly; the lanes of a sub-group without a run exchange zeros
#pragma unroll
    for (int d = 1; d < (int)RW_SUB; d <<= 1) {
        W += xor_lane_f64(W, d);
#pragma unroll
        for (uint32_t j = 0; j < ROWS_CHUNK; ++j) R[j] += xor_lane_f64(R[j], d);
    }
    const uint32_t piece = piece0 + l;
    if (!live || l >= CHUNK_PIECES || piece >= stride / 16u) return;
    f32x4 out = single;
    if (size > 1u) {
        double r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3];
#pragma unroll
        for (uint32_t p = 1; p < CHUNK_PIECES; ++p) if (l == p) { r0 = R[4 * p]; r1 = R[4 * p + 1]; r2 = R[4 * p + 2]; r3 = R[4 * p + 3]; }
        out = l < here ? f32x4{ mr::quotient(r0, W), mr::quotient(r1, W), mr::quotient(r2, W), mr::quotient(r3, W) } : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    }
    *(f32x4*)(dst + (dst_first + group) * (uint64_t)stride + (uint64_t)piece * 16u) = below_width(out, piece, width);
}

__global__ void k_rows_empty(uint4* __restrict__ count) { *count = make_uint4(0u, 0u, 0u, 0u); }

hipError_t launch_merge_rows(hipStream_t st, SortScratch& sort, const void* records, size_t n, const uint32_t* member_group, const void* rows,
                             const gs4d_rows_query& q, uint32_t* scratch, void* dst, size_t dst_first, size_t capacity, gs4d_merge_count* count) {
    if (n >= 0xFFFFFFFFull || dst_first >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (!n) { k_rows_empty<<<dim3(1), dim3(1), 0, st>>>((uint4*)count); return hipGetLastError(); }
    // the scratch, in the order of merge_rows_scratch_words(): keys, sorted indices, run starts, tile counts, state (merge.hip), mass words
    const size_t n4 = (n + 3) & ~(size_t)3;
    const uint32_t ntiles = (uint32_t)merge_tiles(n);
    uint32_t* const keys = scratch;
    uint32_t* const index = keys + n4;
    uint32_t* const start = index + n4;
    uint32_t* const counts = start + n4;
    uint32_t* const state = counts + ((ntiles + 3u) & ~3u);
    float* mass = (float*)(state + 4);
#ifdef GS4D_ROWS_MASS_RECOMPUTE
    mass = nullptr;
#endif
    const uint32_t per_record = (uint32_t)((n + RW_THREADS - 1) / RW_THREADS);
    const unsigned char* const table = (const unsigned char*)rows;
    hipError_t e;
    if (records) k_rows_keys<true><<<dim3(per_record), dim3(RW_THREADS), 0, st>>>((const f32x4*)records, (uint32_t)n, member_group, table, q.stride, q.width, keys, mass);
    else k_rows_keys<false><<<dim3(per_record), dim3(RW_THREADS), 0, st>>>(nullptr, (uint32_t)n, member_group, table, q.stride, q.width, keys, nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = radix_sort_pairs(st, sort, keys, index, n, nullptr, 32, false, true)) != hipSuccess) return e;
    if ((e = launch_merge_run_starts(st, keys, index, n, counts, 0xFFFFFFFFu, count, state, start, nullptr)) != hipSuccess) return e;
    // rows the call may write: dst_first + key < capacity
    const uint64_t limit = (uint64_t)capacity > (uint64_t)dst_first ? (uint64_t)capacity - (uint64_t)dst_first : 0ull;
    k_rows_written<<<dim3(1), dim3(1), 0, st>>>(keys, start, state, limit, (uint4*)count);
    if ((e = hipGetLastError()) != hipSuccess || limit == 0ull) return e;
    const uint32_t chunks = (q.stride / 4u + ROWS_CHUNK - 1u) / ROWS_CHUNK;
    const uint64_t most = (uint64_t)n < limit ? (uint64_t)n : limit;       // runs that can be written
    const uint64_t wgs = (most * chunks + RW_UNITS_PER_WG - 1) / RW_UNITS_PER_WG;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;      // (more than 2^36 words of rows)
    if (records) k_rows_reduce<true><<<dim3((uint32_t)wgs), dim3(RW_THREADS), 0, st>>>((const f32x4*)records, mass, table, q.stride, q.width, keys, index, start, state,
                                                                                       chunks, limit, (uint64_t)dst_first, (unsigned char*)dst);
    else k_rows_reduce<false><<<dim3((uint32_t)wgs), dim3(RW_THREADS), 0, st>>>(nullptr, nullptr, table, q.stride, q.width, keys, index, start, state, chunks, limit,
                                                                                (uint64_t)dst_first, (unsigned char*)dst);
    return hipGetLastError();
}

// ---- gs4d_copy_rows ----
__global__ __launch_bounds__(RW_THREADS) void k_copy_rows(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t pieces) {
    const uint64_t t = (uint64_t)blockIdx.x * RW_THREADS + threadIdx.x;
    if (t < pieces) dst[t] = src[t];
}

hipError_t launch_copy_rows(hipStream_t st, const void* src, size_t src_first, size_t m, size_t stride, void* dst, size_t dst_first) {
    if (!m) return hipSuccess;
    const uint64_t per_row = stride / 16, pieces = (uint64_t)m * per_row;
    const uint64_t wgs = (pieces + RW_THREADS - 1) / RW_THREADS;
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    k_copy_rows<<<dim3((uint32_t)wgs), dim3(RW_THREADS), 0, st>>>((const uint4*)src + (uint64_t)src_first * per_row, (uint4*)dst + (uint64_t)dst_first * per_row, pieces);
    return hipGetLastError();
}

} // namespace gs4d

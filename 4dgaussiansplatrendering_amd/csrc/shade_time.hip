// shade_time.hip — gs4d_shade_sh_t and gs4d_collapse_sh (include/gs4d.h): the colour of a trained 4D set, whose rows hold degree_t + 1
// blocks of spherical-harmonic coefficients, block n weighted by cos(2 pi n (t - mu_t) / T).  The per-record text — the weights, the effective row
// e, the colour of a record from e — is csrc/sh_time_record.h, which the host library compiles too.
//
// One launch each, no workgroup ever waits for another; one workgroup of SHADE_T_TILE threads per SHADE_T_TILE records, thread r owning record r:
//   the read side   A 4D row is QT = ceil(12 K (DEGREE_T + 1) / 16) pieces of 16 bytes (K = (DEGREE + 1)^2) — 36 at degree 3 / degree_t 2, which
//                   for 256 records would be 151 KB of LDS.  The row is therefore taken in ROUNDS rounds of at most R consecutive pieces (R = QT
//                   where that is at most 13, else the pieces of one 3DGS row of the degree: 7, 12), so that LDS holds what k_shade_sh's holds: at
//                   most 256 * 13 * 16 = 53 248 bytes.  A round is staged as in k_shade_sh — coalesced 16-byte loads from a clamped address, four
//                   in flight per thread, written to LDS with the odd row pitch R | 1, which makes the per-record 16-byte reads conflict-free — and
//                   then every thread folds the words of its row's pieces into e, which it keeps in registers: word g of the row is word g % 3K of
//                   block g / 3K, both known at compile time (blocks need not start on a piece: 108 bytes at degree 2), and the rounds arrive in
//                   the order the definition folds in — block 0, then 1, then 2.
//   k_shade_sh_t    the record side of k_shade_sh (two 16-byte loads, issued before the table is staged), then the colour from e, stored to the
//                   record and, if asked, to the shadow's plane 1.  DEGREE_T 1..2: degree_t 0 is k_shade_sh itself (launch_shade_sh).
//   k_collapse_sh   of the record only mu_t (4 bytes).  e goes back through LDS, a thread's row as Q pieces with the words past 3 K zeroed, and the
//                   tile's dst rows leave as whole 16-byte pieces in address order, zeros past piece Q.  DEGREE_T 0..2 (0: a prefix copy).
// Built with the flags of shade.o.  All byte offsets are 64-bit.  Of sh only the first 16 QT bytes of rows < n are read; k_shade_sh_t writes nothing
// but floats 4..6 of records < n (and .xyz of the same entries of the plane), k_collapse_sh nothing but rows < n of dst.
#include "gs4d_internal.h"
#include "record_tile.h"      // f32x4
#include "sh_time_record.h"

namespace gs4d {

using namespace gs4d_sht;

constexpr uint32_t SHT_THREADS = SHADE_T_TILE;
constexpr uint32_t SHT_MAX_ROUND = 13;

constexpr uint32_t sht_round(int degree, int degree_t) {
    return row_pieces_t(degree, degree_t) <= SHT_MAX_ROUND ? row_pieces_t(degree, degree_t) : row_pieces(degree);
}
constexpr uint32_t sht_pitch(int degree, int degree_t) { return sht_round(degree, degree_t) | 1u; }

// e <- the effective row of the thread's record (threadIdx.x; a thread past `slots` folds what LDS holds, which nobody reads), through `rows`.
// tile: row 0 of the tile.  Every thread of the workgroup calls it; on return the last round's reads of `rows` may still be in flight.
template <int DEGREE, int DEGREE_T>
__device__ __forceinline__ void effective_row_of_tile(const f32x4* __restrict__ tile, uint32_t row_pieces_sh, uint32_t slots, f32x4* rows, const float w[2],
                                                      uint32_t mask, float* e) {
    constexpr uint32_t W = row_words(DEGREE), WT = row_words_t(DEGREE, DEGREE_T), QT = row_pieces_t(DEGREE, DEGREE_T);
    constexpr uint32_t R = sht_round(DEGREE, DEGREE_T), P = sht_pitch(DEGREE, DEGREE_T), ROUNDS = (QT + R - 1u) / R;
#pragma unroll
    for (uint32_t round = 0; round < ROUNDS; ++round) {
        const uint32_t first = round * R, count = QT - first < R ? QT - first : R;
        const uint32_t pieces = slots * count;
        if (round) __syncthreads();                                                      // the reads of the round before
        // work item j of the round is piece first + j % count of row j / count
        for (uint32_t j0 = threadIdx.x; j0 < pieces; j0 += 4u * SHT_THREADS) {
            uint32_t row[4], piece[4];
            f32x4 v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t j = min(j0 + u * SHT_THREADS, pieces - 1u);
                row[u] = j / count;
                piece[u] = j - row[u] * count;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) v[u] = tile[(uint64_t)row[u] * row_pieces_sh + (first + piece[u])];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) if (j0 + u * SHT_THREADS < pieces) rows[row[u] * P + piece[u]] = v[u];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t p = 0; p < R; ++p) {
            if (p >= count) break;
            // (the empty asm takes the piece whole: one 16-byte LDS read, as in k_shade_sh)
            f32x4 v = rows[threadIdx.x * P + p];
            asm volatile("" : "+v"(v));
            const float word[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) {
                const uint32_t g = 4u * (first + p) + q;
                if (g < WT) { const uint32_t block = g / W, j = g - block * W; e[j] = fold((int)block, e[j], word[q], w, mask); }
            }
        }
    }
}

template <int DEGREE, int DEGREE_T>
__global__ __launch_bounds__(SHT_THREADS) void k_shade_sh_t(f32x4* __restrict__ rec, uint32_t n, const f32x4* __restrict__ sh, uint32_t row_pieces_sh,
                                                             float t, float inv_period, float camx, float camy, float camz, f32x4* __restrict__ plane1) {
    __shared__ f32x4 rows[SHADE_T_TILE * sht_pitch(DEGREE, DEGREE_T)];
    const uint64_t rec0 = (uint64_t)blockIdx.x * SHADE_T_TILE;
    const uint64_t left = (uint64_t)n - rec0;                                            // (the grid has no workgroup past the end: left >= 1)
    const uint32_t slots = left < SHADE_T_TILE ? (uint32_t)left : SHADE_T_TILE;
    // the record side first: its two sectors travel while the table is staged (a thread past the end reads the tile's last record)
    const uint32_t r = threadIdx.x < slots ? threadIdx.x : slots - 1u;
    const uint64_t i = rec0 + r;
    const f32x4 pmv = rec[i * 6u], sgv = rec[i * 6u + 5u];
    const float pm[4] = { pmv.x, pmv.y, pmv.z, pmv.w }, sg[4] = { sgv.x, sgv.y, sgv.z, sgv.w };
    float w[2];
    const uint32_t mask = weights(DEGREE_T, t, inv_period, pm[3], w);
    float e[row_words(DEGREE)] = {};
    effective_row_of_tile<DEGREE, DEGREE_T>(sh + rec0 * row_pieces_sh, row_pieces_sh, slots, rows, w, mask, e);
    if (threadIdx.x >= slots) return;
    float out[3];
    colour<DEGREE>(pm, sg, t, camx, camy, camz, e, out);
    float* const dst = (float*)(rec + i * 6u + 1u);
    dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
    if (plane1) { float* const col = (float*)(plane1 + i); col[0] = out[0]; col[1] = out[1]; col[2] = out[2]; }
}

template <int DEGREE, int DEGREE_T>
__global__ __launch_bounds__(SHT_THREADS) void k_collapse_sh(const float* __restrict__ rec, uint32_t n, const f32x4* __restrict__ sh, uint32_t row_pieces_sh,
                                                              float t, float inv_period, f32x4* __restrict__ dst, uint32_t dst_pieces) {
    constexpr uint32_t W = row_words(DEGREE), Q = row_pieces(DEGREE), P = sht_pitch(DEGREE, DEGREE_T);
    static_assert(Q <= P, "a thread's effective row fits its LDS row");
    __shared__ f32x4 rows[SHADE_T_TILE * P];
    const uint64_t rec0 = (uint64_t)blockIdx.x * SHADE_T_TILE;
    const uint64_t left = (uint64_t)n - rec0;
    const uint32_t slots = left < SHADE_T_TILE ? (uint32_t)left : SHADE_T_TILE;
    float w[2] = { 0.0f, 0.0f };
    uint32_t mask = 0u;
    if (DEGREE_T > 0) {                                                                  // the only record traffic: mu_t
        const uint32_t r = threadIdx.x < slots ? threadIdx.x : slots - 1u;
        mask = weights(DEGREE_T, t, inv_period, rec[(rec0 + r) * 24u + 3u], w);
    }
    float e[W] = {};
    effective_row_of_tile<DEGREE, DEGREE_T>(sh + rec0 * row_pieces_sh, row_pieces_sh, slots, rows, w, mask, e);
    __syncthreads();                                                                     // the reads of the last round
#pragma unroll
    for (uint32_t p = 0; p < Q; ++p) {
        float word[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) word[q] = 4u * p + q < W ? e[4u * p + q] : 0.0f;
        rows[threadIdx.x * P + p] = f32x4{ word[0], word[1], word[2], word[3] };
    }
    __syncthreads();
    // work item j of the tile is piece j % dst_pieces of row j / dst_pieces, which is piece j of the tile's part of dst
    f32x4* const out = dst + rec0 * dst_pieces;
    const uint32_t pieces = slots * dst_pieces;
    for (uint32_t j = threadIdx.x; j < pieces; j += SHT_THREADS) {
        const uint32_t row = j / dst_pieces, piece = j - row * dst_pieces;
        out[j] = piece < Q ? rows[row * P + piece] : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    }
}

hipError_t launch_shade_sh_t(hipStream_t st, void* records, size_t n, const void* sh, size_t sh_stride, const gs4d_sh_time& q, float4* plane1) {
    if (q.degree_t == 0) return launch_shade_sh(st, records, n, sh, sh_stride, q.degree, q.t, q.cam_pos, plane1);
    if (!n) return hipSuccess;
    const dim3 grid((uint32_t)((n + SHADE_T_TILE - 1) / SHADE_T_TILE)), block(SHT_THREADS);
    const uint32_t row_pieces_sh = (uint32_t)(sh_stride / 16);
#define GS4D_SHADE_T(D, DT) k_shade_sh_t<D, DT><<<grid, block, 0, st>>>((f32x4*)records, (uint32_t)n, (const f32x4*)sh, row_pieces_sh, q.t, q.inv_period, \
                                                                        q.cam_pos[0], q.cam_pos[1], q.cam_pos[2], (f32x4*)plane1)
    switch (q.degree * 4 + q.degree_t) {
        case 1: GS4D_SHADE_T(0, 1); break;
        case 2: GS4D_SHADE_T(0, 2); break;
        case 5: GS4D_SHADE_T(1, 1); break;
        case 6: GS4D_SHADE_T(1, 2); break;
        case 9: GS4D_SHADE_T(2, 1); break;
        case 10: GS4D_SHADE_T(2, 2); break;
        case 13: GS4D_SHADE_T(3, 1); break;
        case 14: GS4D_SHADE_T(3, 2); break;
        default: return hipErrorInvalidValue;
    }
#undef GS4D_SHADE_T
    return hipGetLastError();
}

hipError_t launch_collapse_sh(hipStream_t st, const void* records, size_t n, const void* sh, size_t sh_stride, const gs4d_sh_time& q, void* dst, size_t dst_stride) {
    if (!n) return hipSuccess;
    const dim3 grid((uint32_t)((n + SHADE_T_TILE - 1) / SHADE_T_TILE)), block(SHT_THREADS);
    const uint32_t row_pieces_sh = (uint32_t)(sh_stride / 16), dst_pieces = (uint32_t)(dst_stride / 16);
#define GS4D_COLLAPSE(D, DT) k_collapse_sh<D, DT><<<grid, block, 0, st>>>((const float*)records, (uint32_t)n, (const f32x4*)sh, row_pieces_sh, q.t, q.inv_period, \
                                                                          (f32x4*)dst, dst_pieces)
    switch (q.degree * 4 + q.degree_t) {
        case 0: GS4D_COLLAPSE(0, 0); break;
        case 1: GS4D_COLLAPSE(0, 1); break;
        case 2: GS4D_COLLAPSE(0, 2); break;
        case 4: GS4D_COLLAPSE(1, 0); break;
        case 5: GS4D_COLLAPSE(1, 1); break;
        case 6: GS4D_COLLAPSE(1, 2); break;
        case 8: GS4D_COLLAPSE(2, 0); break;
        case 9: GS4D_COLLAPSE(2, 1); break;
        case 10: GS4D_COLLAPSE(2, 2); break;
        case 12: GS4D_COLLAPSE(3, 0); break;
        case 13: GS4D_COLLAPSE(3, 1); break;
        case 14: GS4D_COLLAPSE(3, 2); break;
        default: return hipErrorInvalidValue;
    }
#undef GS4D_COLLAPSE
    return hipGetLastError();
}

} // namespace gs4d

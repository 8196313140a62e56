// gs4d_internal.h — shared declarations of libgs4d.so's translation units (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include "../../include/gs4d.h"

namespace gs4d {

constexpr int TILE = 8;             // 8x8-pixel tiles: one wave64 composites one tile
constexpr int PROJ_FLOATS = 16;     // projected record: 64 B, one aligned segment per splat

// Projected record layout (float4 A,B,C,D), written by preprocess, gathered by binning/composite.
//  A = cx, cy, a0x, a1x      B = a0y, a1y, r, g      C = b, alpha, rect0 (x0 | y0<<16), rect1 (x1 | y1<<16)   [pixel rect, inclusive]
//  D = hx, hy, valid(1/0), depth   (depth = -z_view of the centre when the draw has aux outputs or a depth test, else 0; gs4d_debug_read_projected hands them out in the order documented in gs4d.h)
// rect0 > rect1 in x (x0 = 1, x1 = 0) marks "no coverage".

// ---- the outputs of a frame ----
// What the compositing kernels write per pixel, fixed for a frame by its gs4d_clear; each level includes the ones below it.
//   Colour  the RGBA32F image.
//   Aux     also (D, O) per pixel in a float2 plane: D = sum of w * depth with the weight w the colour uses and the depth of the entry's
//           projected record (slot 15), O = 1 - T; a draw is composed onto what the plane holds with the colour's "over":
//           (D, O) <- (D_draw + T * D, (1 - T) + T * O).  A tile not in memory holds (0, 0).
//   Ids     also three W x H planes of u32 in one allocation — record, draw ordinal within the frame, bits of the weight: per draw the
//           fragment of the largest weight w > 0 (front-most on a tie), composed over the stored triple by id_over (composite_common.h).  A
//           pixel no fragment has reached, and a tile not in memory, hold the sentinel {0xFFFFFFFF, 0xFFFFFFFF, 0.0f}.
// Aux and Ids are the transmittance form of the default blend function (SRC_ALPHA, ONE_MINUS_SRC_ALPHA); any other function has Colour only.
enum class Outputs : int { Colour = 0, Aux = 1, Ids = 2 };
constexpr bool has_aux(Outputs o) { return o >= Outputs::Aux; }
constexpr bool has_ids(Outputs o) { return o >= Outputs::Ids; }
// An image as a draw or a fill sees it.  tstate / epoch: the tile state (composite.hip): tstate[tile] == epoch <=> the tile's pixels are in
// memory, else it is still the clear colour.  aux, ids: the planes of `out`, null above that level.  Made by Framebuffer::target (gs4d_api.hip).
// z: a draw's depth-test plane (gs4d_set_depth_test: W x H floats, -z_view units; a fragment of depth d is blended only where d < z), or
// null: no test.  Only the default blend function has one.
// stats: where the draw adds its record statistics (gs4d_set_record_stats), rec == null: nowhere.  An entry whose record index is
// >= n is skipped on the device.  Only a draw of the default blend function into a Colour frame without a depth test has them.
static_assert(sizeof(gs4d_record_stat) == 16 && offsetof(gs4d_record_stat, wsum) == 8, "the 64-bit sum is naturally aligned in a 16-byte record");
struct StatOut { gs4d_record_stat* rec = nullptr; uint32_t n = 0; };
struct Target {
    float4* fb; uint32_t* tstate; uint32_t epoch; float4 clear;
    Outputs out; float2* aux; uint32_t* ids;
    const float* z = nullptr;
    StatOut stats;
};

struct Uniforms {
    float view[16];
    float proj[16];
    float time;
    float min_opacity;
};

// ---- the verdict of a draw: two arrays of VERDICT_WORDS words ----
// Every draw is validated after the fact.  Its kernels leave what they found in the lane's DEVICE words (BinScratch::total, TOT_*), the kernels that
// follow read them there, and a copy for the host lands in the lane's pinned, mapped HOST words (Lane::host_total, HT_*), which resolve_lane
// decodes behind the lane's event.  The two arrays do NOT share a layout.  Paths: ordered (binning.hip, composite.hip), exact = unordered with
// exact lists (k_bucket_scan, k_bucket_scatter, k_bucket_tiles, k_composite_v2), staged = unordered with staged lists (k_project_count<SRC, Stage, ..>,
// k_bucket_tiles_staged, k_composite_v2).  A word that a path does not write keeps what an earlier draw of the lane left.
constexpr int VERDICT_WORDS = 16;                // 64 bytes each: bin_scratch_reserve, gs4d_create
// Device words, zeroed when they are allocated:
//   TOT_ENTRIES        tile-list entries of the draw, saturated at 2^32 - 1.  Written by the last workgroup of k_bin_emit (ordered) or of k_bucket_scan
//                      (exact); read by the tile sort as its element count and by k_tile_ranges (ordered), copied to the host by k_composite_v2 (exact)
//   TOT_FLAGS          VF_* (below).  Stored whole by the same two writers (VF_CAPACITY or 0); k_bucket_tiles ORs VF_LIST into it.  k_tile_ranges,
//                      k_composite and k_composite_v2 (exact) stop on ANY flag; k_bucket_scatter and k_bucket_tiles stop on VF_CAPACITY only: other
//                      workgroups of k_bucket_tiles raise VF_LIST while they run.  Copied to the host by k_bin_emit, k_composite_v2 (exact)
//   TOT_COUNT_LO, _HI  the same count in 64 bits; writers and host copies as TOT_ENTRIES, no reader on the device
//   TOT_LONGEST_LIST   exact: zeroed by k_bucket_scan, atomicMax by k_bucket_tiles, copied to HT_LONGEST_LIST by k_composite_v2
//   TOT_UNUSED_5, _6   nothing writes or reads them
//   TOT_SCAN_ARRIVALS  exact: workgroups of k_bucket_scan that have arrived; the last one sets it back to 0
//   TOT_TICKET         ordered: ticket counter of the k_bin_emit workgroups, never reset (BinScratch::ticket_base is its value at the launch)
//   TOT_ABORT          staged: == TileLists::seq <=> the draw was aborted.  Stored by k_project_count (a segment overflowed its block: TileCount::abort_word)
//                      and k_bucket_tiles_staged (a bucket, a list or the box did not fit); read by k_composite_v2
enum TotalWord : int { TOT_ENTRIES = 0, TOT_FLAGS = 1, TOT_COUNT_LO = 2, TOT_COUNT_HI = 3, TOT_LONGEST_LIST = 4, TOT_UNUSED_5 = 5, TOT_UNUSED_6 = 6, TOT_SCAN_ARRIVALS = 7, TOT_TICKET = 8, TOT_ABORT = 9 };
// Host words, zeroed at gs4d_create; read by resolve_lane (HT_ERROR: device_error too):
//   HT_ENTRIES         as TOT_ENTRIES.  Written by k_bin_emit (ordered), k_bucket_scan (exact, only when the capacity overflowed) and the first workgroup
//                      of k_composite_v2 (exact: a copy; staged: the sum of the bucket statistics); the host reads the 64-bit count instead
//   HT_FLAGS           VF_*; writers as HT_ENTRIES (staged: k_composite_v2 makes it up from TOT_ABORT and the statistics)
//   HT_COUNT_LO, _HI   the entry count in 64 bits; writers as HT_ENTRIES
//   HT_ERROR           raised by any kernel whose device-side check fails (Lane::err_word), never cleared: the context is unusable from then on
//   HT_LONGEST_LIST    exact, staged: longest (sub-)list of a tile.  k_composite_v2; k_bucket_scan stores 0 when the capacity overflowed
//   HT_LONGEST_RUN, HT_FULLEST_BUCKET, HT_FULLEST_SEG   exact, staged: longest (bucket, segment) run, entries of the fullest bucket and of the fullest
//                      segment (TileLists::bstat, sstat), reduced by k_composite_v2: what sizes the staged draws that follow
//   HT_USED_BOX        staged: the box of the tiles that hold entries (BOX_EMPTY: none); exact: BOX_NONE.  k_composite_v2
enum HostWord : int { HT_ENTRIES = 0, HT_FLAGS = 1, HT_COUNT_LO = 2, HT_COUNT_HI = 3, HT_ERROR = 4, HT_LONGEST_LIST = 5, HT_LONGEST_RUN = 6, HT_FULLEST_BUCKET = 7, HT_FULLEST_SEG = 8, HT_USED_BOX = 9 };
static_assert(TOT_ABORT < VERDICT_WORDS && HT_USED_BOX < VERDICT_WORDS, "the highest word of either layout fits the arrays");
// The flags of TOT_FLAGS / HT_FLAGS: why a draw does not stand (resolve_lane re-runs it).  VF_CAPACITY: more entries than the lane's entry storage
// holds (every path).  VF_LIST: a tile's (sub-)list is longer than the compositor was launched for (exact, staged).  VF_STAGED_MISS: a staged
// guess missed — a segment, a bucket or the launch box (host word only).
constexpr uint32_t VF_CAPACITY = 1u, VF_LIST = 2u, VF_STAGED_MISS = 4u;

// ---- sort.hip ----
struct SortScratch {
    uint32_t* keys2 = nullptr; uint32_t* vals2 = nullptr; size_t cap = 0;   // scratch B and C (keys2[2*cap], vals2[2*cap]; one allocation) — radix_sort.hpp:192-216 scratch
    uint32_t* hist = nullptr; size_t hist_cap = 0;                          // two [OS_REPL][4][256] digit-histogram slots (alternating), then the look-back words
    int flip = 0;
    bool hist_pending = false;         // the current slot holds a histogram accumulated by a producer kernel, not yet consumed by a sort
    int acc_flip = 0;                  // which accumulator set the next launch uses (the other one it zeroes)
    int hist_bits = 32;                // host-proven width of (key - hist_bias): passes above it are not even launched
    int hist_rb = 8;                   // digit width the producer of the pending histogram counted in (sort_plan_rb, chosen together with hist_bits)
    int rb_knob = 0;                   // test hook GS4D_SORT_RB (8 / 9): the digit width of every sort whose tile shape allows it
    uint32_t hist_bias = 0;            // ... of (key - hist_bias): a lower bound of all keys, which makes the high digits constant (and their passes skipped)
    // The plan of the pending histogram (sort_plan_hist, chosen with hist_rb / hist_bits before the keys are produced: the producer must count the right digits):
    //   hist_rows  how many LSD digit rows the producer counted (OS_MAX_PASSES: all, the plain LSD plan)
    //   hist_top   >= 0: the producer also counted the 9-bit top digit (key - bias) >> hist_top into row OS_TOP_ROW
    //   hist_hybrid  the sort is the MSD/LSD hybrid: one global pass on the top digit, then k_os_tail (hist_rows == 0)
    //   hist_segfeed the hybrid is segment-fed: a staged projection (k_project_count<SRC, Stage, SegmentFed>) leaves every segment's (key, index) pairs grouped by top digit
    //                in seg_pairs and one {count, offset} word per (digit, segment) in seg_runs[512][hist_seg_rows]; the sort is k_os_tail alone, which gathers
    //                its bucket from the segments' runs (no k_os_pass launch; the caller's key buffer holds no unsorted keys in between)
    int hist_rows = 4, hist_top = -1; bool hist_hybrid = false, hist_segfeed = false; uint32_t hist_seg_rows = 0;
    // the segment blocks of a segment-fed sort: SEGFEED_BLOCK pairs per segment, and the run table.  Never scratch 1 / 2: k_os_tail's slow path writes its
    // bucket's range of those while other workgroups still read their runs.  Grown by sort_scratch_reserve while `segfeed` is set.
    uint2* seg_pairs = nullptr; size_t seg_cap = 0;      // in pairs
    uint32_t* seg_runs = nullptr; size_t runs_cap = 0;   // in words
    bool segfeed = false;              // GS4D_SORT_SEGFEED: 0 = never, 1 = wherever a staged fused frame plans the hybrid, unset = on while GS4D_SORT_HYBRID is unset too
    int hybrid_knob = -1;              // GS4D_SORT_HYBRID: 0 = never (the LSD passes, nothing else counted), 1 = for every eligible span at any n, unset = eligible spans of >= OS_HYBRID_MIN_N keys
    uint32_t tail_cap = 8192;          // GS4D_SORT_TAILCAP: buckets above it take k_os_tail's slow path (at most the kernel's LDS tile)
    // pinned + mapped status words of the latest top-digit report (k_os_tail's first workgroup, or k_os_top_stats behind a fallback sort), and the same
    // memory as the device sees it.  [0] largest bucket, [1] buckets above tail_cap, [2] non-zero once anything was reported
    uint32_t* fb = nullptr; uint32_t* fb_dev = nullptr;
    uint64_t stat_hybrid = 0, stat_launches = 0;      // hybrid sorts and sort kernel launches (histogram launches included) of this scratch
    uint32_t epoch = 0;                // tag of the look-back words of the latest pass launch
    bool atomic_rank = false;          // LDS-atomic ranking verified on this device (lds_atomic_order_selftest)
    int shape_knob = 0, rank_knob = 0; // test / tuning hooks read at context creation: GS4D_SORT_SHAPE (1..6: tile shape of a pass), GS4D_SORT_RANK (1 = ballot ranking, 2 = LDS-atomic ranking)
    uint32_t* totals = nullptr;                                             // [256] spare words (err word when `err` is not set)
    uint32_t* err = nullptr;                                                // not owned: device word raised when a look-back spin times out
    // persistent workgroups a pass may launch (occupancy x compute units of THIS scratch's device), per kernel instance: asked of the runtime once per
    // scratch — a scratch belongs to one context, a context to one device; no process-wide cache (two contexts on two devices, or created on two threads)
    struct Resident { const void* fn = nullptr; uint32_t groups = 0; } resident[16];
};
hipError_t sort_scratch_reserve(hipStream_t st, SortScratch& s, size_t n);
void sort_scratch_free(SortScratch& s);
// Stable LSD radix sort of (key,val) pairs on bits [0, key_bits).  n_dev == nullptr: n is exact.  Otherwise the element
// count is read on the device from *n_dev (<= n, n is the launch capacity); the result always lands back in keys/vals.
// have_hist: the digit histograms of `keys` were already accumulated (by the kernel that wrote the keys) into sort_hist_slot(s).
// identity_vals: the payload is the identity index 0..n-1 and `vals` has NOT been written: the first pass that moves keys makes the indices up
// instead of reading them (4 bytes per key less to write for whoever produced the keys, 4 less to read here).
hipError_t radix_sort_pairs(hipStream_t st, SortScratch& s, uint32_t* keys, uint32_t* vals, size_t n, const uint32_t* n_dev, int key_bits, bool have_hist, bool identity_vals = false);
uint32_t* sort_hist_slot(hipStream_t st, SortScratch& s, size_t n_hint, hipError_t* e_out);
int sort_plan_rb(const SortScratch& s, size_t n, int key_bits);      // digit width (8 or 9 bits) of a sort of key_bits-bit keys
int sort_plan_passes(int key_bits, int rb);                          // ... and the launches it takes
// The plan of a depth sort of n keys of key_bits bits whose histograms a producer kernel is about to count: sets s.hist_rb, hist_rows, hist_top and
// hist_hybrid (what the producer is launched with, and what radix_sort_pairs(have_hist) then executes).  The hybrid is planned for spans of 19..27 bits
// when LDS-atomic ranking is verified, no sort test hook is set and the latest report's largest bucket fits k_os_tail's tile; a span that is eligible
// but crowded keeps the LSD passes and has the top digit counted beside them, so that the plan can return.
// seg_rows != 0: the producer is the staged projection, with that many segments of at most SEGFEED_BLOCK records: the hybrid is then planned segment-fed
// (hist_segfeed) where the scratch allows it (SortScratch::segfeed, storage reserved).
constexpr size_t OS_HYBRID_MIN_N = 32768;
constexpr uint32_t SEGFEED_BLOCK = 2048;                     // pairs per segment block == STAGE_R * SEG_THREADS (static_assert in preprocess.hip)
constexpr uint32_t SEGFEED_MAX_ROWS = 1024;                  // k_os_tail scans a run-table row with two segments per thread
void sort_plan_hist(SortScratch& s, size_t n, int key_bits, uint32_t seg_rows = 0);
hipError_t lds_atomic_order_selftest(const hipStream_t* streams, int nstreams, bool* ordered);      // on all the streams at once
// Layout of the SoA shadow (preprocess.hip).  The repack kernel verifies what a compact layout assumes, bit for bit, for every record, and
// reports a violation in bbox[15]; the caller then repacks in the next layout down.
//   SOA_STATIC3D  64 B/record: a static 3D splat in the reference's 4D record — mu_t, the time row and the time column of sig are the same
//                 eight values in every record (SoaInfo::consts; Scenes.h ObjectDisplay / a 3D covariance with Sigma44 = 1) — keeps position,
//                 colour and the nine spatial elements of sig: planes (px py pz s00), col, (s01 s02 s10 s11), (s12 s20 s21 s22)
//   SOA_SYM       72 B/record: a symmetric sig without its mirrored half
//   SOA_FULL      96 B/record: pos, col, sig[0..3]
enum { SOA_FULL = 0, SOA_SYM = 1, SOA_STATIC3D = 2 };
struct SoaInfo { int layout = SOA_FULL; float consts[8] = { 0 }; };      // consts: pos.w, sig[0][3], sig[1][3], sig[2][3], sig[3][0..3] of a static set
// sig3 == nullptr: a static set (SOA_STATIC3D) — mu_t and sig[3] are info.consts for every record
// ks: what the keys are computed from (KEYSRC_REF / KEYSRC_VIEWZ, below); span: what k_keygen checks (key - ks.bias) against
struct KeySrc;
hipError_t launch_keygen(hipStream_t st, const float4* pos, const float4* sig3, const SoaInfo& info, size_t n, const KeySrc& ks, float* keys, uint32_t* idx, uint32_t* ghist, int rb, int hist_rows, int hist_top, uint32_t span, uint32_t* err);

// A grow-only device array used by kernels queued on `st`: nothing when `cap` elements suffice; else the stream is waited for, the old block freed
// and one of `want` elements allocated.  After a failed allocation pointer and capacity are null / zero.
template <class T> inline hipError_t grow_device_array(hipStream_t st, T*& p, size_t& cap, size_t want, size_t elem_bytes = sizeof(T)) {
    if (cap >= want) return hipSuccess;
    hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) return e;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    if ((e = hipMalloc(&p, want * elem_bytes)) != hipSuccess) { p = nullptr; return e; }
    cap = want;
    return hipSuccess;
}

// ---- digit histograms for the radix sort, accumulated by whichever kernel produces the keys ----
constexpr int OS_MAX_PASSES = 4;
constexpr int OS_REPL = 8;                                   // replicas of the global histogram: bounds same-address atomic traffic
constexpr uint32_t OS_MAX_BINS = 512;                        // digits are 8 or 9 bits wide (sort_plan_rb); a histogram row always has room for 512 bins
constexpr size_t OS_SLOT_WORDS = (size_t)OS_REPL * OS_MAX_PASSES * OS_MAX_BINS;
constexpr int OS_TOP_ROW = OS_MAX_PASSES - 1;                // the row of the hybrid sort's 9-bit top digit (a span of <= 27 bits has at most three LSD rows)
#ifdef __HIPCC__
// the one wave scan of the kernels: the inclusive sum of v over lanes 0..lane of the wave (lane = threadIdx.x & 63; every lane of the wave calls it)
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(v, off, 64); if (lane >= (unsigned)off) v += t; }
    return v;
}
// (threads 0..255 of the workgroup call clear and flush: each looks after bins tid and tid + 256)
__device__ __forceinline__ void os_hist_clear(uint32_t (*h)[OS_MAX_BINS], uint32_t tid) {
#pragma unroll
    for (int p = 0; p < OS_MAX_PASSES; ++p) { h[p][tid] = 0; h[p][tid + 256u] = 0; }
}
// Wave-cooperative add of one key per active lane (`in` marks the lanes that carry a key; call with the whole wave converged).
// Skewed digits (e.g. the sign/exponent bytes of depth keys take 2-3 values) would serialise 64 LDS atomics on 2-3 addresses:
// the lanes sharing the digit of the first unresolved lane are counted with a ballot and added by one lane, twice; the lanes
// left after that (most lanes of a uniformly distributed digit, almost none of a skewed one) use plain LDS atomics.
// top_shift >= 0: row OS_TOP_ROW counts the 9-bit digit key >> top_shift instead (passes <= OS_TOP_ROW then; passes == 0: that row alone).
__device__ __forceinline__ void os_hist_add(uint32_t (*h)[OS_MAX_BINS], uint32_t key, bool in, int passes, int rb, int top_shift = -1) {
    const uint64_t act = __ballot(in);
    if (act == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int p = 0; p < OS_MAX_PASSES; ++p) {
        const bool top = top_shift >= 0 && p == OS_TOP_ROW;
        if (p >= passes && !top) continue;
        const uint32_t d = top ? (key >> top_shift) & (OS_MAX_BINS - 1u) : (key >> (rb * p)) & ((1u << rb) - 1u);
        uint64_t rem = act;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            if (rem == 0ull) break;
            const uint32_t first = (uint32_t)__ffsll((long long)rem) - 1u;
            const uint32_t d0 = __shfl(d, (int)first, 64);
            const uint64_t peers = __ballot(((rem >> lane) & 1ull) && d == d0);
            if (lane == first) atomicAdd(&h[p][d0], (uint32_t)__popcll(peers));
            rem &= ~peers;
        }
        if ((rem >> lane) & 1ull) atomicAdd(&h[p][d], 1u);
    }
}
__device__ __forceinline__ void os_hist_flush(uint32_t (*h)[OS_MAX_BINS], uint32_t* __restrict__ ghist, int passes, uint32_t tid, int top_shift = -1) {
    uint32_t* g = ghist + (size_t)(blockIdx.x % OS_REPL) * OS_MAX_PASSES * OS_MAX_BINS;
    for (int p = 0; p < OS_MAX_PASSES; ++p) {
        if (p >= passes && !(top_shift >= 0 && p == OS_TOP_ROW)) continue;
        const uint32_t v = h[p][tid], v2 = h[p][tid + 256u];
        if (v) atomicAdd(&g[p * OS_MAX_BINS + tid], v);
        if (v2) atomicAdd(&g[p * OS_MAX_BINS + tid + 256u], v2);
    }
}
#endif

// ---- the unordered draw path (tilelist.hip, composite2.hip): per-tile lists built with atomics, ordered inside the compositor ----
// Blend order of the instances = ascending (key, record index).  Where that key comes from:
//   KEYSRC_INDEX   instance k draws record k (4D-direct, 3D-full, 2D): key = k
//   KEYSRC_REF / KEYSRC_VIEWZ   the bound sort index is the library's own stable sort of the keys gs4d_keygen produced for exactly
//                  these records (tracked by buffer versions): "instance order" == ascending (depth key, record index), so the key
//                  is recomputed per record with k_keygen's arithmetic and the sort index is never read.
enum { KEYSRC_INDEX = 0, KEYSRC_REF = 1, KEYSRC_VIEWZ = 2 };
struct KeySrc {
    int mode = KEYSRC_INDEX;
    float t = 0, camx = 0, camy = 0, camz = 0;
    float vr0 = 0, vr1 = 0, vr2 = 0, vr3 = 0;   // view row 2 at keygen time (KEYSRC_VIEWZ)
    uint32_t bias = 0;                           // subtracted from the key's bit pattern (host-proven lower bound, as in the depth sort)
};
// A blend order and how wide its keys are: span = the host-proven largest (key - ks.bias), which the depth slabs divide evenly; bits = its width.
// gs4d_keygen builds it (KEYSRC_INDEX: draw_common); the queued launch, the lane, the sort index and the draw hold copies of the whole record.
struct BlendOrder { KeySrc ks; int bits = 32; uint32_t span = 0xFFFFFFFFu; };
// "The n records of buffer `data` at version data_ver, in that order": what a lane's last gs4d_keygen keyed, and what a sort index holds once
// gs4d_sort_pairs has sorted exactly those keys with their identity index.
struct SortedBy { BlendOrder order; gs4d_buf data = 0; uint64_t data_ver = 0; size_t n = 0; };
// What the projection kernel does beside projecting, as a named form (fill_tile_count decides it; launch_pre switches on it).  The seven legal pairs:
//   lists None,  keys None | Write                 the ordered path (None, None: k_preprocess, one thread per record; every other pair: k_project_count)
//   lists Count, keys None | Write                 the unordered path with exact lists: entries counted per bucket (k_bucket_scan and k_bucket_scatter follow)
//   lists Stage, keys None | Write | SegmentFed    staged lists: the entries are counted, placed and written by the projection kernel itself
// keys Write and SegmentFed (fused key generation) exist for the 4D sources only: no quad or 2D draw is ever fused (draw_common).  Any other pair:
// hipErrorInvalidValue.
enum class ProjLists : uint8_t { None, Count, Stage };
enum class ProjKeys : uint8_t { None, Write, SegmentFed };
// The struct is the kernels' argument block: its fields keep the order they had before the form got its name (moving them moves the kernel's argument
// loads, and three of the staged 4D instances then allocate other registers: profiles/r12_kernel_resources_*.txt), so each field says which form reads it.
struct TileCount {
    // lists Count, Stage:
    uint32_t* hist = nullptr;                    // [nb][rows]: entries that the records of segment `row` put into bucket b = tile % nb
    uint32_t rows = 0;
    uint32_t* skey = nullptr;                    // [records] blend-order key of every record (lists Count, keys None writes it: k_bucket_scatter reads it)
    uint32_t nb = 0, seg = 0;                    // buckets (a power of two); seg, every k_project_count form: records per segment (a multiple of SEG_THREADS; one workgroup walks one segment)
    int tiles_x = 0, shard_rank = 0, shard_world = 1;
    // every form: the blend order's key (default: the record index)
    KeySrc ks;
    // keys Write, SegmentFed — fused key generation (the draw executes a gs4d_keygen + gs4d_sort_pairs that were queued just before it): the projection
    // kernel also generates the depth keys, bounds-checks them and accumulates the digit histograms of the depth sort, exactly as k_keygen would.
    // keys_out, idx_out, keys Write alone: the caller's key buffer (idx_out null: the sort that follows makes the identity index up itself)
    float* keys_out = nullptr; uint32_t* idx_out = nullptr; uint32_t* ghist = nullptr; int hist_rb = 8, hist_rows = OS_MAX_PASSES, hist_top = -1 /* SortScratch::hist_rows, hist_top */; uint32_t span = 0xFFFFFFFFu; uint32_t* err = nullptr;
    // keys SegmentFed (SortScratch::hist_segfeed; with lists Stage only): instead of keys_out[i] the workgroup writes its segment's (key + bias, record) pairs,
    // grouped by the 9-bit top digit key >> hist_top and stable in record order inside a digit, to seg_pairs[segment * SEGFEED_BLOCK ...], and one word
    // count | offset << 12 per (digit, segment) to seg_runs[digit * rows + segment]
    uint2* seg_pairs = nullptr; uint32_t* seg_runs = nullptr;
    // lists Count, Stage:
    uint32_t* sstat = nullptr;                   // [rows]: entries of every segment (statistics for the host; every counting launch writes them)
    // lists Stage (tilelist.hip): the projection kernel itself WRITES the entries.  A workgroup counts its segment's entries per bucket, scans
    // the counts, places the entries bucket by bucket in LDS and writes them out as ONE dense block: stage_out[segment * scap + offs[b][segment] + k],
    // k < hist[b][segment].  A segment with more than scap entries stores `seq` into *abort_word instead.
    uint2* stage_out = nullptr; uint32_t scap = 0; uint32_t* offs = nullptr; uint32_t* abort_word = nullptr; uint32_t seq = 0;
    // the form (the host reads it: launch_pre; the kernels have it as template arguments)
    ProjLists lists = ProjLists::None;
    ProjKeys keys = ProjKeys::None;
};
constexpr uint32_t V2_MAX_LIST = 1024;           // longest list the compositor sorts in LDS (beyond ~1000 entries per tile its LDS footprint costs more occupancy than the ordered path's two sort passes cost time).  Longer per-tile lists are cut into depth slabs (below); beyond V2_MAX_SLABS a draw uses the ordered path
constexpr uint32_t V2_MAX_SLABS = 64;           // a tile's list is kept as `slabs` sub-lists by equal ranges of the blend key: far slab first, each ordered by itself in the compositor (one wave lane holds a sub-list's table entry: <= 64)
constexpr int STAGE_R = 4;                       // staged lists: records per thread of a segment (kept in registers between the counting and the placing pass): seg <= STAGE_R * SEG_THREADS
constexpr uint32_t STAGE_MAX_SCAP = 5120;        // ... and entries of a segment block (LDS: 8 bytes each beside the 12 KB the projection kernel has already)
constexpr int SEG_THREADS = 512;                 // workgroup size of the kernels that walk a segment of records (k_project_count, k_bucket_scatter)
// list capacities the compositor is instantiated for (64 entries per lane-register): the smallest one >= n
inline uint32_t v2_list_capacity(uint32_t n) {
    static const uint32_t ladder[] = { 64, 128, 192, 256, 384, 512, 768, 1024 };
    for (uint32_t c : ladder) if (n <= c) return c;
    return V2_MAX_LIST;
}
constexpr uint32_t V2_MAX_RECORDS = 1u << 24;    // an entry carries (tile / nb) in the top byte of its record word
struct TileLists {
    uint32_t* hist = nullptr; size_t hist_cap = 0;            // [nb][rows] counts, turned in place into the slot of every (segment, bucket) run inside its bucket
    uint32_t* bbase = nullptr; uint32_t* btot = nullptr; uint32_t* tstart = nullptr; uint32_t* tcnt = nullptr; size_t tiles_cap = 0, nb_cap = 0, slabs_cap = 0;   // [nb + 1] bucket starts, [nb] bucket totals; per tile: first entry, entries
    uint32_t* skey = nullptr; size_t skey_cap = 0;
    uint32_t counters = 0;                                    // LDS counters of k_bucket_tiles: (tiles per bucket) * slabs
    uint32_t nb = 0, rows = 0, seg = 0, slabs = 1, slab_shift = 0;   // geometry of the current draw (tile_lists_plan): slab of an entry = min(slabs - 1, key >> slab_shift)
    // staged lists: segment blocks [rows][scap] entries; per-bucket statistics {entries, longest run, longest list, 0} written by k_bucket_tiles_staged
    // (staged draws) or k_bucket_scan (exact draws), per-segment entry counts written by the projection kernel; the compositing kernel's first
    // workgroup reduces both for the host
    uint2* blocks = nullptr; size_t blocks_cap = 0;           // in entries
    uint4* bstat = nullptr;                                    // [nb_cap]
    uint32_t* sstat = nullptr;                                 // [1024]
    bool staged = false; uint32_t scap = 0, bcap = 0;         // the current draw is staged; entries a segment block holds, bucket capacity in the tile-ordered entry array
    uint32_t seq = 0;                                          // sequence number of the lane's staged draws: total[TOT_ABORT] == seq <=> this draw was aborted
    // staged draws: the BOX of tiles (in blocks of BOX_BLOCK x BOX_BLOCK tiles, both ends inclusive, box_pack) outside which the host expects no entry — a third guess
    // from the previous frames' statistics (bstat[b].w: the box of bucket b's non-empty tiles), checked by k_bucket_tiles_staged like the two capacities;
    // the compositor is launched for these tiles only.  BOX_NONE: the whole image.
    uint32_t box = 0xFFFFFFFFu;
};
constexpr uint32_t BOX_BLOCK = 4u, BOX_NONE = 0xFFFFFFFFu, BOX_EMPTY = 0x0000FFFFu;      // BOX_EMPTY: min 255, max 0 in both directions — the neutral element of box_join
__host__ __device__ __forceinline__ uint32_t box_pack(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) { return x0 | (y0 << 8) | (x1 << 16) | (y1 << 24); }
__host__ __device__ __forceinline__ uint32_t box_x0(uint32_t box) { return box & 255u; }
__host__ __device__ __forceinline__ uint32_t box_y0(uint32_t box) { return (box >> 8) & 255u; }
__host__ __device__ __forceinline__ uint32_t box_x1(uint32_t box) { return (box >> 16) & 255u; }
__host__ __device__ __forceinline__ uint32_t box_y1(uint32_t box) { return box >> 24; }
// (the fields are taken out by hand here: through the accessors the compiler orders the wave reductions of k_bucket_tiles_staged and k_composite_v2 differently)
__host__ __device__ __forceinline__ uint32_t box_join(uint32_t a, uint32_t b) {
    const uint32_t x0 = (a & 255u) < (b & 255u) ? (a & 255u) : (b & 255u), y0 = ((a >> 8) & 255u) < ((b >> 8) & 255u) ? ((a >> 8) & 255u) : ((b >> 8) & 255u);
    const uint32_t x1 = ((a >> 16) & 255u) > ((b >> 16) & 255u) ? ((a >> 16) & 255u) : ((b >> 16) & 255u), y1 = (a >> 24) > (b >> 24) ? (a >> 24) : (b >> 24);
    return box_pack(x0, y0, x1, y1);
}
__host__ __device__ __forceinline__ bool box_holds(uint32_t box, uint32_t bx, uint32_t by) {      // block (bx, by) inside the box
    return box == BOX_NONE || (bx >= box_x0(box) && bx <= box_x1(box) && by >= box_y0(box) && by <= box_y1(box));
}
// both corners of `inner` inside `outer` (always, for outer == BOX_NONE; what BOX_EMPTY or BOX_NONE as the inner box means is the caller's to decide).
// Host code.  The two kernels that make this test (k_bucket_tiles_staged, k_composite_v2) spell out its two box_holds calls: wrapped in one
// function they come out as different instructions.
__host__ __device__ __forceinline__ bool box_within(uint32_t outer, uint32_t inner) { return box_holds(outer, box_x0(inner), box_y0(inner)) && box_holds(outer, box_x1(inner), box_y1(inner)); }
// false: this frame / record count cannot use the unordered path (more than 256 * 1024 tiles, or 2^24 records)
// key_span: host-proven largest blend key (the slabs divide [0, key_span] evenly)
bool tile_lists_plan(TileLists& t, size_t ntiles, size_t nrecords, uint32_t slabs, int keybits, uint32_t key_span = 0xFFFFFFFFu, size_t expect_entries = 0);
hipError_t tile_lists_reserve(hipStream_t st, TileLists& t, size_t ntiles, size_t nrecords);
void tile_lists_free(TileLists& t);
// total, total_host: the lane's device and host verdict words (TOT_*, HT_* above); the host words are written only when more than `cap` entries abort the draw here
hipError_t launch_bucket_scan(hipStream_t st, TileLists& t, uint32_t* total, uint32_t* total_host, size_t cap);
// skey == nullptr: the blend keys the projection left in t.skey; else an array of key bit patterns from which skey_bias is still to be subtracted (the caller's key buffer of a fused draw)
hipError_t launch_bucket_scatter(hipStream_t st, TileLists& t, const uint32_t* trects, const float4* proj, const uint32_t* skey, uint32_t skey_bias, size_t nrecords, const uint32_t* total, uint2* tmp, int tiles_x, int shard_rank, int shard_world);
hipError_t launch_bucket_tiles(hipStream_t st, TileLists& t, size_t ntiles, uint32_t* total, const uint2* tmp, uint2* entries, uint32_t hint);
// staged draws: the segment blocks the projection kernel wrote (t.blocks, t.scap) -> tile lists at entries[b * t.bcap ...]; per-bucket statistics into t.bstat;
// total[TOT_ABORT] = t.seq when a segment's run, a bucket, a list or the box (t.box) does not fit
hipError_t launch_bucket_tiles_staged(hipStream_t st, TileLists& t, size_t ntiles, int tiles_x, uint32_t* total, uint2* entries, uint32_t hint);
hipError_t tile_lists_reserve_blocks(hipStream_t st, TileLists& t, size_t entries);
// tl: the draw's lists — the tile table, the per-bucket and per-segment statistics for the host report (bstat / nb, sstat / rows) and, of a staged draw
// (tl.staged: aborted <=> total[TOT_ABORT] == tl.seq, the entry total is the sum of the statistics), what the host guessed for it: scap, bcap, box
// t: the image; draw_ord: the draw's ordinal within its frame (Outputs::Ids)
hipError_t launch_composite_v2(hipStream_t st, const float4* proj, const uint2* entries, const TileLists& tl, const uint32_t* total, uint32_t* total_host, int tiles_x, int tiles_y, int W, int H,
                               int premult_c, const Target& t, uint32_t hint, int keybits, int recbits, uint32_t draw_ord);

#ifdef __HIPCC__
// tiles touched by a pixel rectangle (x0|y0<<16, x1|y1<<16; x0 > x1: none), restricted to the tile rows ty % world == rank
struct TRect { uint32_t tx0, ty0, wx, rows, tstep, count; };
// tiles tx0 .. tx0 + wx - 1, ty0 .. ty1
__device__ __forceinline__ TRect tile_rect_of(uint32_t tx0, uint32_t ty0, uint32_t wx, uint32_t ty1, uint32_t shard_rank, uint32_t shard_world) {
    TRect r{ tx0, ty0, wx, ty1 - ty0 + 1u, 1u, 0u };
    if (shard_world > 1u) {
        const uint32_t first = r.ty0 + (shard_rank + shard_world - r.ty0 % shard_world) % shard_world;
        r.rows = first > ty1 ? 0u : (ty1 - first) / shard_world + 1u;
        r.ty0 = first; r.tstep = shard_world;
    }
    r.count = r.wx * r.rows;
    return r;
}
__device__ __forceinline__ TRect tile_rect(uint32_t rect0, uint32_t rect1, uint32_t shard_rank, uint32_t shard_world) {
    const uint32_t x0 = rect0 & 0xFFFFu, y0 = rect0 >> 16, x1 = rect1 & 0xFFFFu, y1 = rect1 >> 16;
    if (x0 > x1 || y0 > y1) return TRect{ 0u, 0u, 0u, 0u, 1u, 0u };
    return tile_rect_of(x0 / TILE, y0 / TILE, x1 / TILE - x0 / TILE + 1u, y1 / TILE, shard_rank, shard_world);
}
// The per-record input of the list-building kernels: the tile rectangle packed into 4 bytes — tx0:10 | ty0:10 | wx-1:6 | wy-1:6 — read in
// record order by the scatter (streaming) and in depth order by the binning (a gather: 4 bytes instead of the 8-byte pixel rectangle of
// rounds 1-2 halves the table).  TRECT_NONE: the record touches no tile.  TRECT_WIDE: more than 63 tiles across or down, or beyond tile
// 1022 (images wider than 8184 pixels): the consumer takes the pixel rectangle from the projected record (C.z, C.w) instead.
constexpr uint32_t TRECT_NONE = 0xFFFFFFFFu, TRECT_WIDE = 0xFFFFFFFEu;
__device__ __forceinline__ uint32_t pack_trect(uint32_t rect0, uint32_t rect1) {
    const uint32_t x0 = rect0 & 0xFFFFu, y0 = rect0 >> 16, x1 = rect1 & 0xFFFFu, y1 = rect1 >> 16;
    if (x0 > x1 || y0 > y1) return TRECT_NONE;
    const uint32_t tx0 = x0 / TILE, ty0 = y0 / TILE, wx = x1 / TILE - tx0, wy = y1 / TILE - ty0;      // widths minus one
    if (tx0 >= 1023u || ty0 >= 1023u || wx >= 63u || wy >= 63u) return TRECT_WIDE;
    return tx0 | (ty0 << 10) | (wx << 20) | (wy << 26);
}
__device__ __forceinline__ TRect unpack_trect(uint32_t w, const float4* __restrict__ proj, uint32_t rec, uint32_t shard_rank, uint32_t shard_world) {
    if (w == TRECT_NONE) return TRect{ 0u, 0u, 0u, 0u, 1u, 0u };
    if (w == TRECT_WIDE) { const float4 c = proj[(size_t)rec * 4 + 2]; return tile_rect(__float_as_uint(c.z), __float_as_uint(c.w), shard_rank, shard_world); }
    const uint32_t tx0 = w & 1023u, ty0 = (w >> 10) & 1023u;
    return tile_rect_of(tx0, ty0, ((w >> 20) & 63u) + 1u, ty0 + (w >> 26), shard_rank, shard_world);
}
__device__ __forceinline__ uint32_t tile_of(const TRect& r, uint32_t j, uint32_t tiles_x) { return (r.ty0 + (j / r.wx) * r.tstep) * tiles_x + r.tx0 + j % r.wx; }
// every tile of a small footprint, row by row (no division: this runs once per record in two kernels)
template <class F> __device__ __forceinline__ void for_each_tile(const TRect& r, uint32_t tiles_x, F f) {
    uint32_t rowbase = r.ty0 * tiles_x + r.tx0;
    for (uint32_t y = 0; y < r.rows; ++y) { for (uint32_t x = 0; x < r.wx; ++x) f(rowbase + x); rowbase += r.tstep * tiles_x; }
}
#endif

// ---- preprocess.hip ----
hipError_t launch_soa_repack(hipStream_t st, const float* aos96, size_t n, float4* soa /* n * 96 bytes */, uint32_t* bbox /* [16], preset: min = ~0, max = 0 */, const SoaInfo& info);
// plane 0 holds pos.xyz in every layout; the plane of sig[3] (what key generation reads beside it), or null when it is one of the constants
inline const float4* soa_sig3(const float4* soa, size_t n, const SoaInfo& info) { return info.layout == SOA_STATIC3D ? nullptr : soa + (info.layout == SOA_SYM ? 3 : 5) * n; }
// Each preprocess launch also writes the packed tile rectangle of every record (pack_trect).
// aux: the draw's image has aux outputs or the draw has a depth test — the projection stores each record's depth in the last float of its record (else 0).
// cull_alpha0, tight: set for draws of the default blend function only (enqueue_projection).  cull_alpha0: a record whose alpha compares equal to 0 gets
// no tile-list entry (its projected record is unchanged); tight: the pixel rectangle is cut down to the box of the fragment test's discard disc (footprint_rect.h).
struct PreOut { float4* proj; uint32_t* trects; bool aux = false; bool cull_alpha0 = false; bool tight = false; };
hipError_t launch_preprocess_4d(hipStream_t st, const float4* soa, size_t soa_n /* records in the buffer: the plane stride */, const SoaInfo& info, size_t n, const Uniforms& u, int W, int H, PreOut out, const TileCount& tc);
hipError_t launch_preprocess_3d(hipStream_t st, const float* verts72, size_t n, const Uniforms& u, int W, int H, PreOut out, const TileCount& tc);
hipError_t launch_preprocess_2d(hipStream_t st, const float* rec48, size_t n, const Uniforms& u, int W, int H, PreOut out, const TileCount& tc);

// ---- binning.hip ----
struct BinScratch {
    uint32_t* total = nullptr;        // [VERDICT_WORDS]: the lane's device verdict words (TOT_*, above)
    uint32_t* ranges = nullptr; size_t tiles_cap = 0;           // [2*tiles] start,end — followed in the same allocation by
    unsigned long long* status = nullptr; size_t block_cap = 0; // the chained-scan words of the binning workgroups (epoch-tagged, never zeroed)
    uint32_t epoch = 0;
    uint32_t ticket_base = 0;         // value of total[TOT_TICKET], the ticket counter of the binning workgroups, before the next launch
    // ranges are all-zero between draws: k_tile_ranges fills the non-empty tiles, the composite kernel clears each range it has read
};
hipError_t bin_scratch_reserve(hipStream_t st, BinScratch& b, size_t ninst, size_t ntiles);
void bin_scratch_free(BinScratch& b);
// order == nullptr: instance k draws record k
// trects_in_order: trects[k] belongs to INSTANCE k (it travelled through the depth sort as a second payload); else to record k (gathered through `order`)
hipError_t launch_binning(hipStream_t st, BinScratch& b, const uint32_t* trects, bool trects_in_order, const float4* proj, const uint32_t* order, uint32_t* order_copy, size_t ninst, size_t nrecords, int tiles_x, int tiles_y,
                          uint32_t* pair_keys, uint32_t* pair_vals, size_t pair_cap, uint32_t* err, uint32_t* ghist, int passes, uint32_t* total_host, int shard_rank, int shard_world);
hipError_t launch_tile_ranges(hipStream_t st, BinScratch& b, const uint32_t* pair_keys, size_t pair_cap, size_t ntiles);

// ---- composite.hip ----
// t: the image (Target); draw_ord: the draw's ordinal within its frame (Outputs::Ids)
hipError_t launch_composite(hipStream_t st, const float4* proj, const uint32_t* pair_vals, uint32_t* ranges, const uint32_t* total, int tiles_x, int tiles_y,
                            int W, int H, int premult_c, const Target& t, int blend_src, int blend_dst, uint32_t draw_ord);
hipError_t launch_fill_unwritten(hipStream_t st, const Target& t, int tiles_x, int tiles_y, int W, int H);
// tstate / epoch / clear: as in Target
hipError_t launch_pack_rgba8(hipStream_t st, const float4* fb, const uint32_t* tstate, uint32_t epoch, const float clear[4], int W, int H, int tiles_x, uint32_t* out);
// the pixel rows of the tile rows ty % world == rank, top of the band = the context's first tile row; band_rows pixel rows in all
hipError_t launch_pack_rgba8_band(hipStream_t st, const float4* fb, const uint32_t* tstate, uint32_t epoch, const float clear[4], int W, int H, int tiles_x, int rank, int world, int band_rows, uint32_t* out);

// ---- lines.hip ----
struct LineParams { float vp[16]; float rgba[4]; int W, H; int blend_src, blend_dst; };
// verts_dev: nverts positions of `dims` floats on the device; cnt: W*H fragment counters, all-zero between calls
hipError_t launch_lines(hipStream_t st, const float* verts_dev, size_t nverts, int dims, int strip, const LineParams& p, float width, uint32_t* cnt, float4* fb);

// ---- compact.hip ----
// gs4d_compact_records (gs4d.h): count per tile, scan of the tile counts, scatter — three launches on `st`, no workgroup waits for another.
constexpr uint32_t COMPACT_TILE = 2048;          // records per workgroup of the counting and the scattering kernel (8 rows per thread; 4 KiB of LDS for the tile's kept list)
struct KeepRule { uint32_t min_pixels, min_wmax; uint64_t min_wsum; uint32_t invert; };      // gs4d_keep_rule, validated
inline size_t compact_tiles(size_t n) { return (n + COMPACT_TILE - 1) / COMPACT_TILE; }
// tile_counts: compact_tiles(n) words of scratch (the lane's); src / dst: records of `stride` bytes (a multiple of 16), dst == null: none; kept_index == null:
// none; cap: slots the outputs hold (no slot >= cap is written); count: receives {kept, min(kept, cap)}
hipError_t launch_compact(hipStream_t st, const gs4d_record_stat* stats, size_t n, const KeepRule& rule, uint32_t* tile_counts,
                          const void* src, size_t stride, void* dst, uint32_t* kept_index, uint32_t cap, gs4d_compact_count* count);
// gs4d_compact_time_window: the same three kernels on a table of gs4d_time_span rows; record i is kept iff t_first <= t1 && t_last >= t0
struct WindowRule { float t0, t1; };
hipError_t launch_compact(hipStream_t st, const gs4d_time_span* spans, size_t n, const WindowRule& rule, uint32_t* tile_counts,
                          const void* src, size_t stride, void* dst, uint32_t* kept_index, uint32_t cap, gs4d_compact_count* count);
// gs4d_lod_cut: the same three kernels on a plane of one state byte per node; node i is kept iff its byte equals rule.state.  `count` receives
// {kept, min(kept, cap)} in its first 8 bytes
struct DrawRule { uint32_t state; };
hipError_t launch_compact(hipStream_t st, const uint8_t* states, size_t n, const DrawRule& rule, uint32_t* tile_counts,
                          const void* src, size_t stride, void* dst, uint32_t* kept_index, uint32_t cap, gs4d_compact_count* count);
// gs4d_record_time_spans: spans[i] of the n 96-byte records in `data` (one launch; n == 0: none)
hipError_t launch_time_spans(hipStream_t st, const void* data, size_t n, float min_opacity, gs4d_time_span* spans);
#ifdef __HIPCC__
// the rule of a table row, for every kernel that selects by one (compact.hip, edit.hip)
__device__ __forceinline__ bool keep_row(const uint4 row, const KeepRule k) {
    const uint64_t wsum = (uint64_t)row.z | ((uint64_t)row.w << 32);          // gs4d_record_stat: pixels, wmax, wsum (little endian)
    return (row.x >= k.min_pixels && row.y >= k.min_wmax && wsum >= k.min_wsum) != (k.invert != 0u);
}
// c fragments of weight 1 into row i of a table, for every kernel that owns the row it updates (centres.hip, neighbours.hip, components.hip,
// nearest.hip): pixels += c, wmax = max(wmax, wmax_bits), wsum += c * 2^24 (64-bit, low word first).  A plain 16-byte load, modify, store.
constexpr uint32_t WEIGHT_ONE_BITS = 0x3F800000u;          // the bits of 1.0f: the wmax of a fragment of weight 1
__device__ __forceinline__ void add_fragments(uint4* __restrict__ stats, uint64_t i, uint32_t c, uint32_t wmax_bits) {
    uint4 row = stats[i];
    row.x += c;
    row.y = row.y > wmax_bits ? row.y : wmax_bits;
    const uint64_t sum = (((uint64_t)row.w << 32) | row.z) + ((uint64_t)c << 24);
    row.z = (uint32_t)sum; row.w = (uint32_t)(sum >> 32);
    stats[i] = row;
}
// gs4d_time_span {t_first, t_last} against the window [t0, t1]: the two closed intervals meet (an empty span, {+inf, -inf}, meets nothing)
__device__ __forceinline__ bool keep_row(const float2 row, const WindowRule k) { return row.x <= k.t1 && row.y >= k.t0; }
// a state byte of gs4d_lod_cut's plane against the state that is kept
__device__ __forceinline__ bool keep_row(const uint8_t row, const DrawRule k) { return (uint32_t)row == k.state; }
#endif

// ---- reorder.hip ----
// gs4d_spatial_order (gs4d.h): the box of the placed records, then one 31-bit key per record — the 30-bit Morton code of its cell, or
// ORDER_KEY_UNPLACED — three launches on `st`, no workgroup waits for another; the caller sorts the identity by the keys (radix_sort_pairs).
constexpr uint32_t ORDER_KEY_UNPLACED = 0x40000000u;
constexpr int ORDER_KEY_BITS = 31;
constexpr uint32_t ORDER_BOX_GROUPS = 1024;      // workgroups of the box kernel at most (256 threads each, a grid stride beyond): one partial of 6 floats each
inline uint32_t order_box_groups(size_t n) { const size_t g = (n + 255) / 256; return g < ORDER_BOX_GROUPS ? (uint32_t)g : ORDER_BOX_GROUPS; }
// box_scratch: order_box_words() floats of scratch (the lane's): the box (lo[3], hi[3], 2 unused), then the partials
inline size_t order_box_words() { return 8 + (size_t)ORDER_BOX_GROUPS * 6; }
hipError_t launch_order_keys(hipStream_t st, const void* src, size_t n, size_t stride, size_t pos_offset, float* box_scratch, uint32_t* keys);
// gs4d_gather_records: dst slot j <- the `stride` bytes (a multiple of 16; or 4 or 8) of src record index[j], j < m; an entry >= nsrc leaves its slot as it is
hipError_t launch_gather_records(hipStream_t st, const uint32_t* index, size_t m, const void* src, size_t nsrc, size_t stride, void* dst);

// ---- shade.hip ----
// gs4d_shade_sh (gs4d.h): floats 4..6 of the first n 96-byte records <- the colour of row i of `sh` (sh_stride bytes per row, a multiple
// of 16 that holds 12 (degree + 1)^2 bytes) seen from cam at time t.  plane1: the colour plane of the records' SoA shadow (soa + soa_n), which gets the
// same three floats in .xyz, or null.  One workgroup per SHADE_TILE records.
constexpr uint32_t SHADE_TILE = 256;
hipError_t launch_shade_sh(hipStream_t st, void* records, size_t n, const void* sh, size_t sh_stride, int degree, float t, const float cam[3], float4* plane1);

// ---- shade_time.hip ----
// gs4d_shade_sh_t (gs4d.h): floats 4..6 of the first n 96-byte records <- the colour of row i of `sh`, a row of q.degree_t + 1 blocks of
// 12 (q.degree + 1)^2 bytes (sh_stride bytes per row, a multiple of 16 that holds them), folded at time q.t and seen from q.cam_pos; q validated.
// plane1 as in launch_shade_sh, which serves q.degree_t == 0.  One workgroup per SHADE_T_TILE records.
constexpr uint32_t SHADE_T_TILE = 256;
hipError_t launch_shade_sh_t(hipStream_t st, void* records, size_t n, const void* sh, size_t sh_stride, const gs4d_sh_time& q, float4* plane1);
// gs4d_collapse_sh: row i of dst (dst_stride bytes per row, a multiple of 16 that holds 12 (q.degree + 1)^2 bytes) <- the effective row of row i of
// `sh` at time q.t for the mu_t of record i, zeros behind it.  n <= 0xFFFFFFFF; nothing past row n - 1 of dst is touched.
hipError_t launch_collapse_sh(hipStream_t st, const void* records, size_t n, const void* sh, size_t sh_stride, const gs4d_sh_time& q, void* dst, size_t dst_stride);

// ---- edit.hip ----
// gs4d_edit_colours (gs4d.h): floats 4..7 of the selected ones of the first n 96-byte records edited by e (validated).  stats: the table
// whose row i selects record i by `rule` (keep_row), or null: every record.  from: the n 96-byte records GS4D_EDIT_COPY takes the colour from, else
// null.  plane1: the colour plane of the records' SoA shadow (soa + soa_n) — it is current: the old colour is read from it and the new one written to
// it as well — or null.  One workgroup per EDIT_TILE records.
constexpr uint32_t EDIT_TILE = 256;
struct EditOp { uint32_t op, channels; float value[4]; float amount; };      // gs4d_colour_edit, validated
hipError_t launch_edit_colours(hipStream_t st, void* records, size_t n, const EditOp& e, const gs4d_record_stat* stats, const KeepRule& rule,
                               const void* from, float4* plane1);

// ---- build.hip ----
// gs4d_build_records (gs4d.h): the first n 96-byte records of dst from row i of each parameter array of the form (GS4D_PARAMS_*; rows of
// tightly packed float32, the arrays the form does not use: null).  One workgroup per BUILD_TILE records; nothing past row / record n - 1 is touched.
constexpr uint32_t BUILD_TILE = 256;
struct BuildParams { const void *pos, *rot, *rot_r, *scale, *rgba, *dir, *tvar; };
hipError_t launch_build_records(hipStream_t st, int form, const BuildParams& p, size_t n, void* dst);

// ---- decompose.hip ----
// gs4d_decompose_records (gs4d.h): row i of every destination array given (null: not wanted; rows of tightly packed float32 with the
// sizes of BuildParams) from record i of the n 96-byte records of src, in the form GS4D_PARAMS_3D or GS4D_PARAMS_4D_VEL.  One workgroup per
// DECOMPOSE_TILE records; the instance without the eigen-solve runs when neither rot nor scale is given.  n <= 0xFFFFFFFF; nothing past row n - 1 is
// touched.
constexpr uint32_t DECOMPOSE_TILE = 256;
struct DecomposeOut { void *pos, *rot, *scale, *rgba, *dir, *tvar; };
hipError_t launch_decompose_records(hipStream_t st, int form, const void* src, size_t n, const DecomposeOut& o);

// ---- transform.hip ----
// gs4d_transform_records (gs4d.h): record j * n + i of dst <- record i of the n 96-byte records of src under row j of the m rows of xf.
// One workgroup per TRANSFORM_TILE records and row; m * n <= 0xFFFFFFFF; nothing else of dst is touched.
constexpr uint32_t TRANSFORM_TILE = 256;
hipError_t launch_transform_records(hipStream_t st, const void* src, size_t n, const gs4d_affine4* xf, size_t m, void* dst);

// ---- pose.hip ----
// gs4d_pose_records (gs4d.h): record i of dst <- record i of the n 96-byte records of src under the row(s) of the m rows of xf that row
// i of bind (at byte i * bind_stride; form and stride validated) names, or copied.  One workgroup per POSE_TILE records; a table of at most
// POSE_LDS_ROWS rows is copied into LDS by every workgroup, a larger one is read from global memory.  n, m <= 0xFFFFFFFF; nothing else of dst is touched.
constexpr uint32_t POSE_TILE = 256;
constexpr uint32_t POSE_LDS_ROWS = 128;
hipError_t launch_pose_records(hipStream_t st, const void* src, size_t n, const gs4d_affine4* xf, size_t m, const void* bind, uint32_t form,
                               size_t bind_stride, void* dst);

// ---- sh_rotate.hip ----
// gs4d_rotate_sh (gs4d.h): rows of dst (from the pointer given: row j * n + i with GS4D_SH_EACH, else row i) <- row i of the n rows of
// `stride` bytes of src under the map of the m rows of xf that the form (validated, bind and bind_stride with it) chooses, or copied.  One workgroup
// per SHROT_TILE rows (SHROT_TILE_3 at degree 3) and, with GS4D_SH_EACH, per map; every thread builds the matrices of its row's map in registers.
// n, m, m * n <= 0xFFFFFFFF; nothing else of dst is touched.
constexpr uint32_t SHROT_TILE = 256;
constexpr uint32_t SHROT_TILE_3 = 128;
hipError_t launch_rotate_sh(hipStream_t st, const void* src, size_t n, size_t stride, int degree, const gs4d_affine4* xf, size_t m, const void* bind,
                            uint32_t form, size_t bind_stride, void* dst);

// ---- warp.hip ----
// gs4d_warp_records (gs4d.h): record i of dst <- record i of the n 96-byte records of src through the lattice `lat` (validated: `count`
// is its node count) of 16-byte nodes, or copied.  One workgroup per WARP_TILE records; a lattice of at most WARP_LDS_NODES nodes is copied into LDS
// by every workgroup, a larger one is read from global memory — 0: the shipped build reads every lattice from global memory, which measured faster or
// equal at every size (make lib WARP_LDS_NODES=512 builds the other).  n <= 0xFFFFFFFF; nothing else of dst is touched.
constexpr uint32_t WARP_TILE = 256;
constexpr uint32_t WARP_LDS_NODES = 0;
hipError_t launch_warp_records(hipStream_t st, const void* src, size_t n, const void* nodes, uint32_t count, const gs4d_lattice& lat, void* dst);

// ---- slice.hip ----
// gs4d_slice_records (gs4d.h): record i of dst <- record i of the n 96-byte records of src conditioned at q.t (q validated).
// One workgroup per SLICE_TILE records; n <= 0xFFFFFFFF; nothing else of dst is touched.
constexpr uint32_t SLICE_TILE = 256;
hipError_t launch_slice_records(hipStream_t st, const void* src, size_t n, const gs4d_slice& q, void* dst);

// ---- transform_selected.hip ----
// gs4d_transform_selected (gs4d.h): the selected ones of the first n 96-byte records of data <- themselves under xf (validated) — stats:
// the table whose row i selects record i by `rule` (keep_row), or null: every record; measure: the measurement GS4D_XS_PIVOT_MEASURE takes the pivot
// from, else null.  One workgroup per XFSEL_TILE records; nothing but the selected records < n is written.
constexpr uint32_t XFSEL_TILE = 256;
hipError_t launch_transform_selected(hipStream_t st, void* data, size_t n, const gs4d_selection_xf& xf, const gs4d_record_stat* stats, const KeepRule& rule,
                                     const gs4d_measure* measure);

// ---- cut.hip ----
// gs4d_stat_cut (gs4d.h): a radix select over one field of a statistics table, most significant digit first — per digit one histogram
// launch and one pick launch on `st`, no workgroup waits for another.
constexpr uint32_t CUT_DIGIT_BITS = 8, CUT_BINS = 1u << CUT_DIGIT_BITS;      // 4 digits for pixels and wmax, 8 for wsum
constexpr uint32_t CUT_TILE = 2048;              // rows per workgroup and round of the histogram kernel (256 threads, 8 rows each in flight)
constexpr uint32_t CUT_GROUPS = 1024;            // workgroups of the histogram kernel at most (a grid stride beyond): one partial of CUT_BINS words each
constexpr uint32_t CUT_STATE_WORDS = 4;          // {prefix (64 bits), rank remaining, above so far}: written by a pick kernel, read by the next digit's kernels
inline int cut_passes(int field) { return (field == GS4D_STAT_WSUM ? 64 : 32) / (int)CUT_DIGIT_BITS; }
inline uint32_t cut_groups(size_t n) { const size_t g = (n + CUT_TILE - 1) / CUT_TILE; return g < CUT_GROUPS ? (uint32_t)g : CUT_GROUPS; }
// scratch: cut_scratch_words(n) words (the lane's): the state block, then the partials
inline size_t cut_scratch_words(size_t n) { return CUT_STATE_WORDS + (size_t)cut_groups(n) * CUT_BINS; }
// n rows of `stats`, field GS4D_STAT_*, k = min(budget, n) (>= 1 unless n == 0): *out receives the gs4d_cut; n == 0: {0, 0, 0}, one launch
hipError_t launch_stat_cut(hipStream_t st, const gs4d_record_stat* stats, size_t n, int field, uint32_t k, uint32_t* scratch, gs4d_cut* out);

// ---- select.hip ----
// gs4d_count_ids (gs4d.h): every pixel of rectangle g of the ID planes (ids, ids + W*H, ids + 2*W*H: record, draw, weight) that takes
// part adds one fragment to stats[record] — one launch on `st`.  g: validated (inside the W x H image, draw_first <= draw_last); mask: g.w * g.h
// bytes, or null: none.  No row >= nrecords is touched and nothing outside the rectangle is read.
hipError_t launch_count_ids(hipStream_t st, const uint32_t* ids, int W, int H, const gs4d_id_region& g, const uint8_t* mask, gs4d_record_stat* stats, uint32_t nrecords);

// ---- centres.hip ----
// gs4d_count_centres (gs4d.h): row i < n of stats gets one fragment of weight 1 (GS4D_CQ_ADD) or becomes {0, 0, 0} (GS4D_CQ_REMOVE) iff
// record i takes part in q (validated; W, H: the context's image) — one launch on `st`, one workgroup per CENTRES_TILE records.  The fields come from
// the 96-byte records, or — soa != null: the records' SoA shadow, which is current, its planes soa_n float4 apart, its layout info — from the shadow's
// planes, which hold the same bits.  mask: q.w * q.h bytes, or null: none.  Rows of records that do not take part are neither read nor written.
constexpr uint32_t CENTRES_TILE = 256;
hipError_t launch_count_centres(hipStream_t st, const void* records, const float4* soa, size_t soa_n, const SoaInfo& info, size_t n, const gs4d_centre_query& q,
                                int W, int H, const uint8_t* mask, gs4d_record_stat* stats);

// ---- neighbours.hip ----
// gs4d_count_neighbours (gs4d.h): row i < n of stats gets c_i fragments of weight 1, c_i the number (at most q.cap) of sources whose
// centre lies within q.radius of record i's — source: the table whose row j makes record j a source by `rule` (keep_row), or null: every record
// that takes part.  q: validated.  Key kernel, the sort of the identity by key (`sort`: the lane's pair_sort, reserved for n), a memset, the bucket
// kernel and the query kernel on `st`; no workgroup waits for another.  Nothing but rows < n of stats and the scratch is written.  phases < 4 (the
// measurement hook of tools/neighbours_cost.py): stop behind the keys (1), the sort (2), the table (3) — stats is then not written.
constexpr uint32_t NEIGHBOURS_TILE = 256;
bool neighbour_radius_ok(float r);               // 2^-63 <= r < 2^64: r * r is a normal float32 number (neighbour_query.h)
int neighbour_bucket_bits(size_t n);             // kb: the bucket table has 2^kb rows, 2 n <= 2^kb < 4 n inside 2^8 .. 2^30
// scratch: neighbour_scratch_words(n) words (the lane's): n candidates of 16 bytes, the table of 2^kb rows of 8 bytes, n keys, n sorted indices
inline size_t neighbour_scratch_words(size_t n) { return 4 * n + 2 * ((size_t)1 << neighbour_bucket_bits(n)) + 2 * n; }
hipError_t launch_count_neighbours(hipStream_t st, SortScratch& sort, const void* records, size_t n, const gs4d_neighbour_query& q,
                                   const gs4d_record_stat* source, const KeepRule& rule, uint32_t* scratch, gs4d_record_stat* stats, int phases = 4);
// The grid phases alone (keys, sort, memset, bucket table; `phases` as above, 3 and more: all of them), which gs4d_label_components builds on: g
// receives where they left the structure in `scratch` — cand[s] = {centre, bits(index)} of the source in sorted slot s, table[b] = {first, end} of
// bucket b's run of slots, keys[s] (bit kb set: not a source) and index[s] of every slot.  flags: GS4D_NB_SKIP_HIDDEN / GS4D_NB_SKIP_DEAD.
struct NeighbourGrid { float4* cand; uint2* table; uint32_t* keys; uint32_t* index; int kb; };
hipError_t launch_neighbour_grid(hipStream_t st, SortScratch& sort, const void* records, size_t n, float t, float radius, uint32_t flags,
                                 const gs4d_record_stat* source, const KeepRule& rule, uint32_t* scratch, int phases, NeighbourGrid& g);

// ---- components.hip ----
// gs4d_label_components (gs4d.h): labels[i] <- the smallest record index of the connected component of member i < n (members: the
// sources of launch_neighbour_grid; linked iff near), GS4D_ID_NONE for a non-member; stats != null: row i of a member gets min(q.cap, size of its
// component) fragments of weight 1.  q: validated.  The grid phases, then the init, link and flatten kernels (a lock-free union–find on `labels`,
// component_union.h; err: the lane's error word, raised if a trip bound runs out), with stats a memset and the size and row kernels, all on `st`; no
// workgroup waits for another.  scratch: neighbour_scratch_words(n) words.  Nothing but the n labels, rows < n of stats and the scratch is written.
constexpr uint32_t COMPONENTS_TILE = 256;
hipError_t launch_label_components(hipStream_t st, SortScratch& sort, const void* records, size_t n, const gs4d_component_query& q,
                                   const gs4d_record_stat* source, const KeepRule& rule, uint32_t* scratch, uint32_t* labels, gs4d_record_stat* stats,
                                   uint32_t* err);
// gs4d_nearest_neighbours (gs4d.h; nearest.hip): the first q.k gs4d_neighbour_hit slots of row i < n of hits (rows hit_stride bytes
// apart, a multiple of 16 that is at least 8 q.k) <- the q.k nearest sources of launch_neighbour_grid within q.radius of record i by (bits(dist2),
// index), {GS4D_ID_NONE, +inf} behind them; stats != null: row i gets the number of hits and the dist2 bits of the last one.  q: validated.  The
// grid phases, then one query kernel on `st`; no workgroup waits for another.  scratch: neighbour_scratch_words(n) words.  Nothing but those slots,
// rows < n of stats and the scratch is written.
constexpr uint32_t NEAREST_TILE = 256;
hipError_t launch_nearest_neighbours(hipStream_t st, SortScratch& sort, const void* records, size_t n, const gs4d_nearest_query& q,
                                     const gs4d_record_stat* source, const KeepRule& rule, uint32_t* scratch, void* hits, size_t hit_stride,
                                     gs4d_record_stat* stats);
// gs4d_count_labels (gs4d.h): row i < n of stats gets one fragment of weight 1 iff labels[i] < n is the label of some j < n whose row of `seeds`
// passes `rule`.  flags: n words of scratch (the lane's).  A memset and two kernels on `st`.  Nothing but rows < n of stats and the flags is written.
hipError_t launch_count_labels(hipStream_t st, const uint32_t* labels, size_t n, const gs4d_record_stat* seeds, const KeepRule& rule, uint32_t* flags,
                               gs4d_record_stat* stats);

// ---- measure.hip ----
// gs4d_measure_records (gs4d.h): *out <- the measurement at time t, under the GS4D_MS_* flags (validated), of the selected ones of the
// first n 96-byte records — stats: the table whose row i selects record i by `rule` (keep_row), or null: every record.  Three launches on `st`, no
// workgroup waits for another; n == 0: the empty measurement, one launch.  Nothing but the 96 bytes of out and the scratch is written.
constexpr uint32_t MEASURE_THREADS = 256;        // threads of a workgroup of every kernel of the call
constexpr uint32_t MEASURE_GROUPS = 1024;        // workgroups of the two walking kernels at most (a grid stride beyond): one partial row each
constexpr uint32_t MEASURE_ROW_WORDS = 16;       // a partial row: the first 64 bytes of a gs4d_measure, the floats as their keys (measure_record.h)
inline uint32_t measure_groups(size_t n) { const size_t g = (n + MEASURE_THREADS - 1) / MEASURE_THREADS; return g < MEASURE_GROUPS ? (uint32_t)g : MEASURE_GROUPS; }
// scratch: measure_scratch_words() words (the lane's): the partial rows, sized by the grid cap
inline size_t measure_scratch_words() { return (size_t)MEASURE_GROUPS * MEASURE_ROW_WORDS; }
hipError_t launch_measure_records(hipStream_t st, const void* records, size_t n, float t, uint32_t flags, const gs4d_record_stat* stats, const KeepRule& rule,
                                  uint32_t* scratch, gs4d_measure* out);

// ---- merge.hip ----
// gs4d_cell_labels (gs4d.h): labels[i] <- the cell of record i < n of the 96-byte records in `grid` (validated).  One launch; n == 0: none.
hipError_t launch_cell_labels(hipStream_t st, const void* records, size_t n, const gs4d_cell_grid& grid, uint32_t* labels);
// gs4d_merge_records (gs4d.h): one record per group of members with one label — the key kernel, the stable sort of the identity by key
// (`sort`: the lane's pair_sort, reserved for n), the count / scan / head kernels over the sorted keys and the group kernel, all on `st`; no workgroup
// waits for another.  alpha_max: validated; stats: the table whose row i lets record i be a member by `rule` (keep_row), or null: every record;
// groups, member_group: null: none; cap: slots dst and groups hold (no slot >= cap is written); *count always receives the gs4d_merge_count
// (n == 0: zeros, one launch).  n <= 0xFFFFFFFE.  Nothing but those outputs, the n words of member_group and the scratch is written.
constexpr uint32_t MERGE_TILE = 2048;            // sorted keys per workgroup of the counting and the head kernel (8 per thread)
inline size_t merge_tiles(size_t n) { return (n + MERGE_TILE - 1) / MERGE_TILE; }
// scratch: merge_scratch_words(n) words (the lane's neighbour scratch): keys, sorted indices and run starts of n words each (each rounded up to 16
// bytes), one word per tile (rounded up likewise), the state block {groups, members, 0, 0}
inline size_t merge_scratch_words(size_t n) { return 3 * ((n + 3) & ~(size_t)3) + ((merge_tiles(n) + 3) & ~(size_t)3) + 4; }
hipError_t launch_merge_records(hipStream_t st, SortScratch& sort, const void* records, size_t n, const uint32_t* labels, float alpha_max,
                                const gs4d_record_stat* stats, const KeepRule& rule, uint32_t* scratch, void* dst, gs4d_merge_group* groups,
                                uint32_t* member_group, uint32_t cap, gs4d_merge_count* count);
// The run starts of n > 0 sorted keys, members first and GS4D_ID_NONE behind them (k_merge_count, k_merge_scan, k_merge_heads): start[g] <- the
// sorted slot of group g's first member, state <- {groups, members}, *count <- {groups, min(groups, cap), members, n - members}, and with
// member_group given member_group[index[s]] <- the group of sorted slot s.  counts: one word per tile of MERGE_TILE keys.
hipError_t launch_merge_run_starts(hipStream_t st, const uint32_t* keys, const uint32_t* index, size_t n, uint32_t* counts, uint32_t cap,
                                   gs4d_merge_count* count, uint32_t* state, uint32_t* start, uint32_t* member_group);

// ---- merge_rows.hip ----
// gs4d_merge_rows (gs4d.h): one row per value of member_group among the members — a key kernel, the stable sort of the identity by key
// (`sort`: the lane's pair_sort, reserved for n), the run starts of merge.hip, one thread that counts the written rows, and the row reduction, all on
// `st`; no workgroup waits for another.  records: null: unit weights; q: validated; capacity: rows of `stride` bytes dst holds (no row >= capacity is
// written); *count always receives the gs4d_merge_count (n == 0: zeros, one launch).  n, dst_first <= 0xFFFFFFFE.  Nothing but those rows, the count
// and the scratch is written.
// scratch: merge_rows_scratch_words(n) words (the lane's neighbour scratch): the layout of merge_scratch_words(n), then one mass word per record
inline size_t merge_rows_scratch_words(size_t n) { return merge_scratch_words(n) + ((n + 3) & ~(size_t)3); }
hipError_t launch_merge_rows(hipStream_t st, SortScratch& sort, const void* records, size_t n, const uint32_t* member_group, const void* rows,
                             const gs4d_rows_query& q, uint32_t* scratch, void* dst, size_t dst_first, size_t capacity, gs4d_merge_count* count);
// gs4d_copy_rows (gs4d.h): rows dst_first .. of dst <- the m rows of `stride` bytes from src_first on of src, in 16-byte pieces.  One launch; m == 0: none.
hipError_t launch_copy_rows(hipStream_t st, const void* src, size_t src_first, size_t m, size_t stride, void* dst, size_t dst_first);

// ---- lod.hip ----
// gs4d_lod_append (gs4d.h): nodes[first + j] <- the 96 bytes of level[j], parent[first + j] <- GS4D_ID_NONE, j < m; parent[child_first + i]
// <- first + member_group[i] where that word is below m, else GS4D_ID_NONE, i < c (member_group null: c == 0).  child_first + c <= first and
// first + m <= 0xFFFFFFFE (validated).  One launch; m == 0 and c == 0: none.  Nothing else is written.
hipError_t launch_lod_append(hipStream_t st, const void* level, size_t m, const uint32_t* member_group, size_t child_first, size_t c,
                             void* nodes, uint32_t* parent, size_t first);
// gs4d_lod_cut (gs4d.h): the cut of q (validated for n) through the forest of n 96-byte nodes and n parent words — a clearing launch, one
// launch per level (or run of small levels) from the top down over the state plane, and the three compaction kernels over the plane, all on `st`; no
// workgroup waits for another.  state: n bytes of scratch, tile_counts: compact_tiles(n) words (the lane's); dst, cut_index, stats: null: none; cap:
// slots dst and cut_index hold (no slot >= cap is written); *count always receives the gs4d_lod_count (n == 0: zeros, one launch).  Nothing but those
// outputs, the rows of the DRAW nodes in stats and the scratch is written.
constexpr uint32_t LOD_TILE = 1024;              // nodes per workgroup of the level kernel (4 per thread)
hipError_t launch_lod_cut(hipStream_t st, const void* nodes, const uint32_t* parent, size_t n, const gs4d_lod_query& q, uint8_t* state,
                          uint32_t* tile_counts, void* dst, uint32_t* cut_index, gs4d_record_stat* stats, uint32_t cap, gs4d_lod_count* count);

} // namespace gs4d

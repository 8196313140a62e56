// gs4d_api.hip — the C ABI (include/gs4d.h): context, buffer objects, pipeline state and the draw sequence.
//
// Stands in for the OpenGL objects and calls the reference's scenes use on this path:
//   ShareStorageBuffer ctor/SubData/Bind                    4DSplatRendering/ShareStorageBuffer.cpp:3-40
//   glGenBuffers/glBufferStorage/glBufferSubData/glBindBufferBase/glDeleteBuffers in the scenes   Scenes.h:241-247, 282-283, 321-325, 336, 220-224
//   Shader::Bind/SetUniform1f/SetUniformMat4f               4DSplatRendering/Shader.cpp:171-174, 206-209
//   radix_sort::sorter::sort                                Dependencies/GPU_RADIX_SORT/radix_sort.hpp:258-392
//   Renderer::Clear / Renderer::Draw                        4DSplatRendering/Renderer.cpp:20-39
//
// Execution model: FRAME LANES.  A context owns a few lanes (4 by default, GS4D_LANES=1..8); a lane is one HIP stream with its own framebuffer,
// projected records, tile lists and sort scratch.  Every call of one frame (key generation, depth sort, draw) is queued on the
// current lane, in order — no events inside a frame.  The first frame-starting call (clear, keygen, sort) after a draw moves to the
// next lane, so whole frames overlap on the device: the latency-bound kernels of one frame (the radix sort's chained scans) fill the
// gaps of the bandwidth-bound kernels of its neighbours.  Lanes only meet through buffer objects and framebuffers; each of those
// remembers which lane wrote it last and which lanes read it since, and a lane about to touch it waits on the other lane's event —
// on the device, never on the host.  Only read-back/finish calls block, plus the validation of a draw's tile-list capacity, which
// is deferred to the next call that could observe the draw (see resolve_pending).
#include "gs4d_internal.h"
#include "operands.h"
#include "merge_record.h"
#include "warp_record.h"
#include "lod_query.h"
#include "lod_operands.h"
#include "rows_operands.h"
#include "sh_rotate_operands.h"
#include "sh_time_record.h"
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <algorithm>
#include <functional>
#include <vector>
#include <cmath>

using namespace gs4d;

namespace {

constexpr int MAX_LANES = 8;

struct Buffer {
    void* d = nullptr;
    size_t bytes = 0;
    uint64_t version = 0;          // bumped by every write; the SoA shadow and the keygen-histogram hand-off compare against it
    float4* soa = nullptr;         // lazily built SoA shadow of 96-B SplatData records
    SoaInfo soa_info;              // ... its layout (preprocess.hip): 64 B/record for static 3D splats, 72 for a symmetric sig, 96 otherwise
    size_t soa_n = 0;
    uint64_t soa_version = ~0ull;
    uint64_t soa_builds = 0;       // times ensure_soa has (re)built the shadow (gs4d_debug_shadow_builds)
    uint32_t* bbox_dev = nullptr;  // 16 words: bounding box of pos / mu_t / velocity, reduced by the repack kernel
    double bb_lo[7] = { 0 }, bb_hi[7] = { 0 }; bool bb_ok = false;
    // cross-lane hazards
    int wr_lane = -1;              // lane whose kernels wrote the buffer last (-1: the host did, synchronously)
    unsigned ordered_mask = 0;     // lanes that have already ordered themselves after that write
    unsigned rd_mask = 0;          // lanes whose DRAWS have read it since that write (their binning-done event covers the reads)
    unsigned tail_mask = 0;        // lanes whose other kernels (key generation) have read it since that write (their tail event does)
    uint64_t touch = 0;            // context op counter at the last device-side use (host writes compare it with the last full sync)
    bool alive = false;
    bool stats_target = false;     // draws have added record statistics to it since the host last waited for it (gs4d_set_record_stats): a host read settles every lane's draws first
    bool ptr_exposed = false;      // gs4d_buffer_device_ptr has handed the storage's address out: the storage may never be exchanged (see Lane::spare)
    // The caller announced (gs4d_buffer_invalidate) that work on ITS stream rewrites the buffer: every lane that uses it afterwards first
    // waits for an event recorded on that stream at the first such use (the caller has queued the writes by then: that is the contract).
    hipEvent_t ev_fill = nullptr; unsigned fill_mask = 0; bool fill_recorded = false;
    // A gs4d_compact_records whose kernels read the buffer as their statistics table: draws ADD to a table as readers do (order_record_stats), and
    // a reader waits for nobody but a writer — so the compaction leaves an event of its own behind its kernels, and a draw that is about to add to
    // the table on another lane waits for it first (scan_wait: the lanes that have not yet).  Both of its kernels evaluate the rule: they must see one table.
    hipEvent_t ev_scan = nullptr; unsigned scan_wait = 0;
    // Provenance of a sort index: set when gs4d_sort_pairs has sorted exactly the keys and the identity index gs4d_keygen wrote for
    // prov.data — the contents are then "records of prov.data in ascending (depth key, record index)" for as long as `version`
    // still equals prov_ver, and a draw that binds it can take its blend order from the keys instead of reading it (tilelist.hip).
    bool prov_valid = false; uint64_t prov_ver = 0; SortedBy prov;
    void sorted_by(bool valid, const SortedBy& by) { prov_valid = valid; if (valid) { prov = by; prov_ver = version; } }      // (after the sort has bumped `version`)
};

struct DrawArgs {
    int mode = 0;
    Uniforms u;
    gs4d_buf data = 0, order = 0;
    size_t instances = 0;
    bool quads = false;
    int lane = 0, fb = 0;          // where the draw ran
    bool v2 = false;               // unordered tile lists (tilelist.hip); false: instance-ordered lists (binning.hip)
    BlendOrder blend_order;        // v2, fuse, regen_order: where the blend order comes from, the largest blend key and its width
    // the draw also executes the gs4d_keygen + gs4d_sort_pairs that were queued for it (first run only: a re-run finds the buffers sorted).  Its keys
    // are blend_order's: draw_common fuses only the keygen whose sort made the draw's own index — one BlendOrder, copied to both; no span of its own.
    bool fuse = false; gs4d_buf fuse_keys = 0, fuse_idx = 0;
    int blend_src = GS4D_SRC_ALPHA, blend_dst = GS4D_ONE_MINUS_SRC_ALPHA;       // glBlendFunc state at the draw
    float clear[4] = { 0, 0, 0, 0 };   // what "clear" meant for the image when the draw was issued (a re-run must not pick up a later glClearColor)
    int shard_rank = 0, shard_world = 1;       // ... and the tile-row shard
    // The re-run of an unordered draw on the ordered path: the draw never read the caller's sort index (it took its order from the keys), and by
    // now the application may have overwritten it for a later frame.  The re-run regenerates "records in ascending (key, index)" from `blend_order`
    // into the lane's private index instead of reading the caller's buffer.
    bool regen_order = false;
    bool exact_lists = false;         // the re-run of a staged draw whose blocks, runs or buckets did not fit: builds its lists exactly (scan + scatter)
    uint64_t stage_geom = 0;        // set by run_draw: the list geometry the draw's bucket statistics belong to (resolve_lane files them under it)
    Outputs out = Outputs::Colour;  // what the image's frame was cleared with: from Aux on the projection stores depths in its records
    uint32_t draw_ord = 0;          // the draw's ordinal within its frame (a re-run keeps it)
    gs4d_buf zplane = 0;            // the depth-test plane bound when the draw was issued (gs4d_set_depth_test; 0: no test) — it, too, makes the projection store depths
    gs4d_buf stats = 0; size_t stats_n = 0;      // the record-statistics buffer bound when the draw was issued and its records (gs4d_set_record_stats; 0: none)
    // The draw builds no tile-list entry that cannot change a pixel (records of alpha 0, tiles only the discarded part of a footprint reaches: DESIGN.md §4).
    // Decided when the draw is issued, kept by its re-runs: the default blend function (a fragment of alpha 0 and a discarded one are no-ops there; any other
    // function is applied fragment by fragment and its entry counts are the quad's), and not a context's first splat draw, which builds every entry.
    bool lean = false;
};

struct Framebuffer {
    float4* mem = nullptr;
    uint32_t* linecnt = nullptr;   // per-pixel fragment counters of the overlay-line kernels (lines.hip), allocated on first use, all-zero between calls
    bool is_clear = true;          // no draw has touched the image since its gs4d_clear
    // Tile state ("fast clear", composite.hip): tstate[tile] == epoch <=> the tile's pixels are in memory; any other tile is still the clear
    // colour.  gs4d_clear takes a new epoch (no memset, no fill); the compositing kernels write the tiles that have list entries; readers
    // substitute the clear colour (RGBA8 packs) or have the rest written first (materialise_fb: host read-backs, float copies, overlay lines).
    uint32_t* tstate = nullptr; uint32_t epoch = 1; bool all_in_memory = false;
    float clear[4] = { 0, 0, 0, 0 };   // the clear colour: the context's at the gs4d_clear that cleared this image
    int last_lane = -1;            // lane that touched it last
    // The planes of the other outputs (Outputs, gs4d_internal.h), allocated with the image up to the level the context has asked for so far
    // (reserve_planes).  out: what this image's frame was cleared with — its compositing kernels and k_fill_unwritten keep those planes valid
    // for every tile in memory.  draws: splat draws into the frame since its clear.
    float2* aux = nullptr; uint32_t* ids = nullptr; Outputs out = Outputs::Colour; uint32_t draws = 0;
    // the image as a draw or a fill of output set `o` sees it, with what "clear" means for it (a draw: DrawArgs::clear)
    Target target(Outputs o, const float c[4]) const { return Target{ mem, tstate, epoch, make_float4(c[0], c[1], c[2], c[3]), o, has_aux(o) ? aux : nullptr, has_ids(o) ? ids : nullptr }; }
    Target target() const { return target(out, clear); }
    // planes up to level `want` for a w x h image (the one place that knows their sizes); free_planes: all of them
    hipError_t reserve_planes(Outputs want, int w, int h) {
        hipError_t e = hipSuccess;
        if (has_aux(want) && !aux) e = hipMalloc(&aux, (size_t)w * h * sizeof(float2));
        if (e == hipSuccess && has_ids(want) && !ids) e = hipMalloc(&ids, (size_t)w * h * 3 * sizeof(uint32_t));
        return e;
    }
    void free_planes() { if (aux) (void)hipFree(aux); if (ids) (void)hipFree(ids); aux = nullptr; ids = nullptr; out = Outputs::Colour; }
};

struct Lane {
    hipStream_t s = nullptr;
    hipEvent_t ev_emit = nullptr;      // the lane's latest binning kernel has finished (it read and copied the sort index; its entry count is final)
    hipEvent_t ev_tail = nullptr;      // recorded when the lane is left: everything queued on it so far
    bool drawn = false;                // the lane's current frame has a draw in it: the next frame-starting call moves on
    float4* proj = nullptr; uint32_t* trects = nullptr; size_t proj_cap = 0, proj_n = 0;   // projected records (64 B) and their packed tile rectangles (4 B)
    bool trects_in_order = false;      // the last draw's tile rectangles are in INSTANCE order (they went through its depth sort), not in record order
    uint32_t* pair_keys = nullptr; uint32_t* pair_vals = nullptr; size_t pair_cap = 0;   // tile-list entries: one allocation of 8 * pair_cap bytes — (tile ids | records) on the ordered path, (key, record) pairs on the unordered one
    TileLists tl;                      // unordered path: per-tile counts / starts / cursors, per-record blend keys
    uint32_t* order_copy = nullptr; size_t order_cap = 0;   // private copy of the last draw's sort index (for a re-run after overflow)
    uint32_t* regen_keys = nullptr; size_t regen_cap = 0;   // keys of a regenerated sort index (DrawArgs::regen_order), allocated on first use
    SortScratch depth_sort, pair_sort;
    BinScratch bin;
    float* line_verts = nullptr; size_t line_cap = 0;   // device copy of the vertices of the latest gs4d_draw_lines (the lane's stream orders its reuse)
    uint32_t* compact_counts = nullptr; size_t compact_cap = 0;   // gs4d_compact_records: one word per tile of COMPACT_TILE records (counts, then first slots); the lane's stream orders its reuse
    uint32_t* spatial_scratch = nullptr; size_t spatial_cap = 0;      // gs4d_spatial_order: the box and its partials (order_box_words()), then one key per record; the lane's stream orders its reuse
    uint32_t* cut_scratch = nullptr; size_t cut_cap = 0;               // gs4d_stat_cut: the state block and one partial histogram per workgroup (cut_scratch_words()); the lane's stream orders its reuse
    uint32_t* measure_scratch = nullptr; size_t measure_cap = 0;       // gs4d_measure_records: one partial row per workgroup (measure_scratch_words()); the lane's stream orders its reuse
    uint32_t* neighbour_scratch = nullptr; size_t neighbour_cap = 0;   // gs4d_count_neighbours, gs4d_label_components and gs4d_nearest_neighbours: candidates, bucket table, keys and sorted indices (neighbour_scratch_words()); gs4d_count_labels: n flag words; the lane's stream orders its reuse
    uint8_t* lod_state = nullptr; size_t lod_cap = 0;                  // gs4d_lod_cut: the state plane, one byte per node (its tile counts: compact_counts); the lane's stream orders its reuse
    uint32_t* host_total = nullptr; uint32_t* host_total_dev = nullptr;   // the host verdict words of the last draw (HT_*, gs4d_internal.h), pinned + mapped, and the same memory as the device sees it
    uint32_t* err_word() const { return &host_total_dev[HT_ERROR]; }     // the error word every kernel may raise
    gs4d_buf kg_buf = 0; uint64_t kg_ver = 0;         // key buffer whose digit histograms k_keygen left for the next sort
    gs4d_buf kg_idx = 0; uint64_t kg_idx_ver = 0;     // ... the identity index it wrote beside them
    SortedBy keyed;                                    // ... and what the lane's last gs4d_keygen keyed: which records, in which order
    // Storage renaming for per-frame key / index buffers.  A buffer object is a NAME; its device storage is the library's.  gs4d_keygen
    // overwrites its two output buffers entirely, so when their storage is still being written or read by ANOTHER lane's frame (an
    // application with one key / index pair for all frames: the reference's layout, Scenes.h m_key_buf / m_values_buf) the new frame
    // does not wait for it: the buffers exchange their storage with this lane's spare pair and the earlier frame finishes on what is now
    // the spare.  When storage leaves a buffer everything that uses it has already been queued (API calls are sequential): an event is
    // recorded right then on every lane that wrote or still reads it, and the lane that takes the storage back later waits for exactly
    // those events — not for the lanes' tail events, which by then cover later frames as well and would chain the lanes to each other.
    struct Spare { void* d = nullptr; size_t bytes = 0; uint64_t touch = 0; unsigned wait_mask = 0; hipEvent_t ev[MAX_LANES] = { nullptr }; } spare[2];
    bool pending = false;              // the lane's last draw has not had its tile-list capacity validated yet
    bool discarded = false;            // ... and its image has been cleared since: validated (counted, learned from) but never re-run
    DrawArgs pending_args;
};

thread_local std::string g_create_error;

} // namespace

struct gs4d_ctx {
    int device = 0;
    int W = 0, H = 0, tiles_x = 0, tiles_y = 0;
    int nlanes = 4, cur = 0;
    Lane lanes[MAX_LANES];
    Framebuffer fbs[MAX_LANES];        // fbs[i] belongs to lane i; a clear makes the current lane's own framebuffer the current one
    int cur_fb = 0;
    hipStream_t user = nullptr;        // the caller's stream (gs4d_set_stream), or null
    hipEvent_t ev_user = nullptr;      // user stream -> lane: what the caller queued before an API call
    hipEvent_t ev_readback = nullptr;  // lane -> user stream: a device-side read-back
    std::string err;
    std::vector<Buffer> bufs;          // index = name; bufs[0] unused
    gs4d_buf slots[8] = { 0 };
    int mode = GS4D_MODE_4D_SORTED;
    Uniforms u;
    float clear[4] = { 0.0f, 0.0f, 0.0f, 0.0f };     // GL's initial clear colour; the app sets its own (Application.cpp:125)
    bool atomic_rank = false;          // result of the LDS-atomic ordering self-test
    uint64_t ops = 0, synced = 0;      // device-side uses so far / at the last sync of every lane
    int shard_rank = 0, shard_world = 1;   // single-frame sharding: this context bins and composites the tile rows ty % world == rank
    int prev_fb = -1;                  // the image the last gs4d_clear moved away from (still intact until its lane comes round again)
    uint64_t stat_entries = 0, stat_reruns = 0, stat_depth_passes = 0, stat_tile_passes = 0;
    uint64_t stat_aborted_discarded = 0;   // draws that aborted on the device (capacity, list length) and were cleared away before anybody observed them
    // draw path selection: the unordered path needs lists short enough to be sorted in LDS (<= V2_MAX_LIST entries per tile)
    int path_pref = 0;                 // GS4D_DRAW_PATH: 0 auto, 1 ordered path only, 2 = auto (kept for symmetry)
    bool long_lists = false;           // the last unordered draw met a list longer than V2_MAX_LIST: draws use the ordered path ...
    uint64_t ordered_draws = 0;        // ... and probe the unordered one again every so often when the lists look short on average
    // A gs4d_keygen (and the gs4d_sort_pairs of its output) is not launched at once: if the draw that follows takes its blend order from
    // exactly that sort, the projection kernel generates the keys as a by-product (it recomputes them anyway) and the sort is queued
    // behind the draw.  Any other call that could observe the buffers launches the stand-alone kernels first (flush_order).
    struct { bool keygen = false, sorted = false; int lane = 0; gs4d_buf data = 0, keys = 0, idx = 0; size_t n = 0; BlendOrder order; } po;
    int blend_src = GS4D_SRC_ALPHA, blend_dst = GS4D_ONE_MINUS_SRC_ALPHA;     // glBlendFunc state (Application.cpp:137-138, 150)
    bool defer_order = true;           // GS4D_FUSE_KEYGEN=0 switches the deferral off (test hook)
    uint64_t stat_composited_tiles = 0;      // tiles the compositing kernel of the last unordered draw was launched for (staged draws: the launch box)
    int neighbour_phases = 4;          // measurement hook GS4D_NEIGHBOURS_PHASES (1..4), read at context creation: gs4d_count_neighbours stops behind its k-th phase (launch_count_neighbours)
    uint64_t stat_fused = 0, stat_renamed = 0, stat_shadow_bytes = 0, stat_streams_rejected = 0, stat_lanes_sharing = 0;      // lanes_sharing: lanes that had to take a stream which shares a hardware queue with another lane
    bool rename_storage = true;        // GS4D_RENAME=0 switches the storage exchange off (test hook)
    bool aux_enable = false, ids_enable = false;      // gs4d_set_aux_outputs, gs4d_set_id_outputs: what the frames cleared from now on have (gs4d_clear)
    gs4d_buf record_stats = 0; size_t record_stats_n = 0;      // gs4d_set_record_stats: draw state like the depth test's (survives gs4d_clear; deleting the buffer turns it off); 0: off
    gs4d_buf depth_plane = 0;          // gs4d_set_depth_test: draw state like glBlendFunc's (survives gs4d_clear; deleting the buffer unbinds it); 0: no test
    Outputs planes = Outputs::Colour;  // the highest level that has been asked for so far: every image has its planes (gs4d_resize reallocates them)
    int shrink_votes = 0;
    // Two ways to get a tile's list into blend order.  Lists of up to V2_MAX_LIST entries: built unordered, ordered by the wave that
    // composites the tile (k_composite_v2).  Longer lists, or a blend order that is not a key the library knows: the instance-ordered path
    // (binning.hip) — at 10^7 splats (1500 entries on the average non-empty tile) it is the faster one by 7-17 % against every way of
    // keeping such lists on the unordered path that round 3 built and measured: depth slabs of the lists, a bucket-wide LDS sort.
    uint32_t slabs = 1;                // depth slabs per tile list (tilelist.hip): only GS4D_SLABS sets it — an experiment knob whose mechanism stays tested
    uint32_t list_hint = 256;          // LDS list capacity the compositor is launched with (64 << k); grows on demand, validated per draw on the device
    // Staged lists (tilelist.hip): once a draw of a scene has reported its fullest segment, its longest (bucket, segment) run and its fullest bucket,
    // the draws that follow let the projection kernel write the list entries itself — one dense block per segment, sized by those statistics plus a
    // margin — no scan and no scatter kernel.  The device checks the guess; a draw that does not fit is re-run exactly.  GS4D_STAGED=0 switches it
    // off (test hook).
    bool stage_enable = true, stage_known = false, stage_box_enable = true;
    // Entries that cannot change a pixel (preprocess.hip emit(), draws of the default blend function): records of alpha 0 get none (GS4D_CULL_ALPHA0=0
    // switches that off), and the pixel rectangle is the smaller of the quad's box and the discard disc's (GS4D_TIGHT_RECT=0: the quad's).  Test hooks.
    bool cull_alpha0 = true, tight_rect = true;
    // Splat draws issued so far.  A context's FIRST draw builds every entry of every quad's box: its verdict is the first measurement the entry storage, the list
    // capacity and the staged capacities of the following draws are sized from, and tests/test_gpu_render.py (configs[4] at full size: 5.4e8 entries, one re-run)
    // and tests/test_gpu_capacity.py (the long tile in the image corner) pin its entry count and longest list to the quads' boxes of all records.
    uint64_t splat_draws = 0;
    uint32_t stage_max_run = 0, stage_max_bucket = 0, stage_max_seg = 0; uint64_t stage_geom = 0;
    uint32_t stage_box_margin = 1;  // blocks added on every side of it; doubled (up to 16) whenever a draw had entries outside its box
    uint32_t stage_box = BOX_NONE;  // blocks of tiles that held entries in the last staged draw of this geometry (TileLists::box); BOX_NONE: not known
    uint64_t stat_staged = 0, stat_staged_misses = 0;
    uint64_t stat_v2_draws = 0, stat_longest = 0;
    // profiling: a ring of per-frame event pairs; a frame ends with its draw
    static constexpr int PROF_FRAMES = 128;
    unsigned profiling = 0;                    // bit s set: stage s is timed
    int prof_frame = 0;
    int prof_every = 1;                        // only every prof_every-th frame is timed ...
    uint64_t prof_tick = 0;                    // ... counted here (a frame ends with its draw)
    std::vector<hipEvent_t> ev0, ev1;          // [PROF_FRAMES][GS4D_T_COUNT], created on first use
    std::vector<uint8_t> ran;
};

namespace {

int fail(gs4d_ctx* c, int code, const char* msg) { if (c) c->err = msg; else g_create_error = msg; return code; }
int hipfail(gs4d_ctx* c, hipError_t e, const char* where) {
    char b[256]; snprintf(b, sizeof b, "%s: %s", where, hipGetErrorString(e));
    if (c) c->err = b; else g_create_error = b;
    return e == hipErrorOutOfMemory ? GS4D_E_NOMEM : GS4D_E_DEVICE;
}
#define HIPCHK(c, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hipfail((c), e__, #call); } while (0)

const char* const DEVICE_CHECK_MSG = "device-side check failed (a bounded look-back wait timed out, a sort key fell outside its proven bounds, a union-find loop of gs4d_label_components ran past its trip bound, or a key buffer changed under a queued sort without gs4d_buffer_invalidate): results are invalid";

Buffer* getbuf(gs4d_ctx* c, gs4d_buf b) { return (b != 0 && b < c->bufs.size() && c->bufs[b].alive) ? &c->bufs[b] : nullptr; }
Lane& lane(gs4d_ctx* c) { return c->lanes[c->cur]; }
// the image as draw `a` sees it, with the draw's depth-test plane and record-statistics buffer (run_draw has checked that they are alive and large enough)
Target draw_target(gs4d_ctx* c, const Framebuffer& F, const DrawArgs& a) {
    Target t = F.target(a.out, a.clear);
    if (const Buffer* Z = getbuf(c, a.zplane)) t.z = (const float*)Z->d;
    if (const Buffer* S = getbuf(c, a.stats)) t.stats = StatOut{ (gs4d_record_stat*)S->d, (uint32_t)std::min<size_t>(a.stats_n, 0xFFFFFFFFull) };
    return t;
}

struct StageTimer {
    gs4d_ctx* c; int slot; hipStream_t s;
    StageTimer(gs4d_ctx* c_, int id) : c(c_), slot(-1), s(c_->lanes[c_->cur].s) {      // run_draw re-runs make their lane current first (resolve_lane); id < 0: times nothing
        if (id >= 0 && ((c->profiling >> id) & 1u) && c->prof_frame < gs4d_ctx::PROF_FRAMES && c->prof_tick % (uint64_t)c->prof_every == 0) { slot = c->prof_frame * GS4D_T_COUNT + id; (void)hipEventRecord(c->ev0[slot], s); }
    }
    ~StageTimer() { if (slot >= 0) { (void)hipEventRecord(c->ev1[slot], s); c->ran[slot] = 1; } }
};

int sync_all(gs4d_ctx* c) {
    for (int i = 0; i < c->nlanes; ++i) HIPCHK(c, hipStreamSynchronize(c->lanes[i].s));
    c->synced = c->ops;
    return GS4D_OK;
}

bool device_error(gs4d_ctx* c) { for (int i = 0; i < c->nlanes; ++i) if (c->lanes[i].host_total[HT_ERROR]) return true; return false; }

// The current frame is complete (it has a draw in it) and a new one starts: move to the next lane.
int next_frame_if_drawn(gs4d_ctx* c) {
    Lane& L = lane(c);
    if (!L.drawn) return GS4D_OK;
    HIPCHK(c, hipEventRecord(L.ev_tail, L.s));
    L.drawn = false;
    c->cur = (c->cur + 1) % c->nlanes;
    lane(c).drawn = false;
    return GS4D_OK;
}

// What the caller queued on its own stream before this API call happens before what the call queues.
int after_user_stream(gs4d_ctx* c) {
    if (!c->user) return GS4D_OK;
    HIPCHK(c, hipEventRecord(c->ev_user, c->user));
    HIPCHK(c, hipStreamWaitEvent(lane(c).s, c->ev_user, 0));
    return GS4D_OK;
}

// The current lane is about to read (or overwrite) buffer B with a kernel: order it after the other lanes' kernels that wrote B
// (or, for a write, still read it).  Device-side waits only.  A lane other than the current one has been left since it last touched
// B, so its tail event (recorded on leaving) covers that use; a draw's reads are already covered by its binning-done event.
int resolve_lane(gs4d_ctx* c, int li);
int after_user_fill(gs4d_ctx* c, Buffer& B) {
    const unsigned me = 1u << c->cur;
    if (!(B.fill_mask & me)) return GS4D_OK;
    B.fill_mask &= ~me;
    if (!c->user) { B.fill_mask = 0; return GS4D_OK; }
    if (!B.ev_fill) HIPCHK(c, hipEventCreateWithFlags(&B.ev_fill, hipEventDisableTiming));
    if (!B.fill_recorded) { HIPCHK(c, hipEventRecord(B.ev_fill, c->user)); B.fill_recorded = true; }
    HIPCHK(c, hipStreamWaitEvent(lane(c).s, B.ev_fill, 0));
    return GS4D_OK;
}
int lane_access(gs4d_ctx* c, Buffer& B, bool write) {
    { int rc = after_user_fill(c, B); if (rc) return rc; }
    // (An unordered draw never read its sort index, and its re-run does not either — DrawArgs::regen_order — so overwriting the index a
    // still-unvalidated draw was given needs no validation first: an application with ONE key / index buffer pair, the reference's layout
    // (Scenes.h m_key_buf / m_values_buf), is ordered lane after lane on the device by the events below, never on the host.)
    Lane& L = lane(c);
    const unsigned me = 1u << c->cur;
    if (B.wr_lane >= 0 && B.wr_lane != c->cur && !(B.ordered_mask & me)) {
        HIPCHK(c, hipStreamWaitEvent(L.s, c->lanes[B.wr_lane].ev_tail, 0));
        B.ordered_mask |= me;
    }
    if (write) {
        for (int r = 0; r < c->nlanes; ++r) {
            if (r == c->cur) continue;
            if ((B.tail_mask >> r) & 1u) HIPCHK(c, hipStreamWaitEvent(L.s, c->lanes[r].ev_tail, 0));
            else if ((B.rd_mask >> r) & 1u) HIPCHK(c, hipStreamWaitEvent(L.s, c->lanes[r].ev_emit, 0));
        }
        B.rd_mask = 0; B.tail_mask = 0; B.wr_lane = c->cur; B.ordered_mask = me;
    }
    B.touch = ++c->ops;
    return GS4D_OK;
}

// The host is about to write, read or free B: wait for every kernel that may still use it.
int host_access(gs4d_ctx* c, Buffer& B);

int ensure_pairs(gs4d_ctx* c, Lane& L, size_t cap) {
    const hipError_t e = grow_device_array(L.s, L.pair_keys, L.pair_cap, cap, 16);      // ordered path: tile ids | records (4 + 4 bytes per slot); unordered path: two arrays of (key, record)
    L.pair_vals = L.pair_keys ? L.pair_keys + L.pair_cap : nullptr;
    return e == hipSuccess ? GS4D_OK : hipfail(c, e, "grow_device_array(L.pair_keys)");
}

int ensure_soa(gs4d_ctx* c, Buffer& b) {
    const size_t n = b.bytes / 96;
    if (b.soa && b.soa_n == n && b.soa_version == b.version) return GS4D_OK;
    if (b.touch > c->synced) { int rc = sync_all(c); if (rc) return rc; }      // a running draw may still project from the old shadow
    { int rc = after_user_fill(c, b); if (rc) return rc; }                     // the repack reads what the caller's stream is writing
    Lane& L = lane(c);
    if (!b.soa || b.soa_n != n) {
        if (b.soa) { (void)hipFree(b.soa); b.soa = nullptr; }
        if (n) HIPCHK(c, hipMalloc(&b.soa, n * 96));
        b.soa_n = n;
    }
    // bounding box of everything the sort key depends on (upload-time work: one small read-back per refresh)
    uint32_t init[16]; for (int i = 0; i < 16; ++i) init[i] = i < 7 ? 0xFFFFFFFFu : 0u;
    if (!b.bbox_dev) HIPCHK(c, hipMalloc(&b.bbox_dev, 64));
    uint32_t got[16];
    // the most compact layout the records allow: static 3D splats (the time row / column of sig and mu_t the same in every record: those of
    // record 0), else a symmetric sig, else everything.  The kernel verifies the assumption for every record; a violation sends the round again.
    const bool allow_compact = !(getenv("GS4D_SOA_FULL") && atoi(getenv("GS4D_SOA_FULL")));             // test hook: always the 96-byte layout (upload-time code: read per repack)
    float rec0[24] = { 0 };
    if (n) { HIPCHK(c, hipMemcpyAsync(rec0, b.d, 96, hipMemcpyDeviceToHost, L.s)); HIPCHK(c, hipStreamSynchronize(L.s)); }
    static const int order[3] = { SOA_STATIC3D, SOA_SYM, SOA_FULL };
    for (int attempt = allow_compact ? 0 : 2; attempt < 3; ++attempt) {
        b.soa_info = SoaInfo();
        b.soa_info.layout = order[attempt];
        if (order[attempt] == SOA_STATIC3D) { const float cs[8] = { rec0[3], rec0[11], rec0[15], rec0[19], rec0[20], rec0[21], rec0[22], rec0[23] }; memcpy(b.soa_info.consts, cs, sizeof cs); }
        HIPCHK(c, hipMemcpyAsync(b.bbox_dev, init, 64, hipMemcpyHostToDevice, L.s));
        HIPCHK(c, launch_soa_repack(L.s, (const float*)b.d, n, b.soa, b.bbox_dev, b.soa_info));
        HIPCHK(c, hipMemcpyAsync(got, b.bbox_dev, 64, hipMemcpyDeviceToHost, L.s));
        HIPCHK(c, hipStreamSynchronize(L.s));      // the shadow is complete before any lane can be asked to read it
        if (order[attempt] == SOA_FULL || got[15] == 0) break;
    }
    auto ord2f = [](uint32_t u) { u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u; float f; memcpy(&f, &u, 4); return (double)f; };
    b.bb_ok = n > 0 && got[14] == 0;
    for (int k = 0; k < 7; ++k) { b.bb_lo[k] = ord2f(got[k]); b.bb_hi[k] = ord2f(got[7 + k]); if (!(b.bb_lo[k] <= b.bb_hi[k])) b.bb_ok = false; }
    b.soa_version = b.version;
    b.soa_builds++;
    return GS4D_OK;
}

// The current lane is about to use framebuffer F: order it after the lane that touched F last.
int fb_access(gs4d_ctx* c, Framebuffer& F) {
    if (F.last_lane >= 0 && F.last_lane != c->cur) HIPCHK(c, hipStreamWaitEvent(lane(c).s, c->lanes[F.last_lane].ev_tail, 0));
    F.last_lane = c->cur;
    return GS4D_OK;
}

// every tile of the current image into memory (the lazily clear ones get their clear colour): for whoever reads or writes single pixels
// (on lane L, which the caller has ordered after the image's last user)
int materialise_fb(gs4d_ctx* c, Framebuffer& F, Lane& L) {
    if (!F.all_in_memory) {
        HIPCHK(c, launch_fill_unwritten(L.s, F.target(), c->tiles_x, c->tiles_y, c->W, c->H));
        F.all_in_memory = true;
        F.is_clear = false;
    }
    return GS4D_OK;
}
// ... the current image, on the current lane
int materialise_fb(gs4d_ctx* c) {
    Framebuffer& F = c->fbs[c->cur_fb];
    if (!F.all_in_memory) { int rc = fb_access(c, F); if (rc) return rc; }
    return materialise_fb(c, F, lane(c));
}

// Enqueue binning -> tile sort -> ranges -> composite for the projected records in L.proj.
int enqueue_raster(gs4d_ctx* c, Lane& L, Framebuffer& F, const DrawArgs& a, const uint32_t* order, uint32_t* order_copy, size_t ninst, size_t nrecords, int premult_c) {
    const int blend_src = a.blend_src, blend_dst = a.blend_dst;
    const size_t ntiles = (size_t)c->tiles_x * c->tiles_y;
    int tile_bits = 1; while (((size_t)1 << tile_bits) < ntiles) ++tile_bits;
    // (4K: 129 600 tiles = 17 bits — three passes of 8-bit digits, two of 9-bit ones)
    const int tile_rb = L.pair_sort.hist_rb = sort_plan_rb(L.pair_sort, L.pair_cap, tile_bits), tile_passes = sort_plan_passes(tile_bits, tile_rb);
    {
        StageTimer t(c, GS4D_T_BINNING);
        hipError_t he = hipSuccess;
        uint32_t* ph = sort_hist_slot(L.s, L.pair_sort, L.pair_cap, &he);      // the emit kernel also counts the tile-id digits
        if (!ph) return hipfail(c, he, "sort_hist_slot");
        HIPCHK(c, launch_binning(L.s, L.bin, L.trects, L.trects_in_order, L.proj, order, order_copy, ninst, nrecords, c->tiles_x, c->tiles_y, L.pair_keys, L.pair_vals, L.pair_cap, L.err_word(),
                                 ph, tile_passes | (tile_rb << 8), L.host_total_dev, a.shard_rank, a.shard_world));
    }
    HIPCHK(c, hipEventRecord(L.ev_emit, L.s));     // the last binning workgroup wrote the total straight into pinned host memory
    {
        StageTimer t(c, GS4D_T_PAIRSORT);
        HIPCHK(c, radix_sort_pairs(L.s, L.pair_sort, L.pair_keys, L.pair_vals, L.pair_cap, L.bin.total + TOT_ENTRIES, tile_bits, true));
    }
    c->stat_tile_passes = (uint64_t)tile_passes;
    {
        StageTimer t(c, GS4D_T_COMPOSITE);      // the per-tile ranges and the compositing kernel
        HIPCHK(c, launch_tile_ranges(L.s, L.bin, L.pair_keys, L.pair_cap, ntiles));
        HIPCHK(c, launch_composite(L.s, L.proj, L.pair_vals, L.bin.ranges, L.bin.total, c->tiles_x, c->tiles_y, c->W, c->H, premult_c, draw_target(c, F, a), blend_src, blend_dst, a.draw_ord));
    }
    return GS4D_OK;
}

// Unordered path: the projection kernel has counted the entries per tile; scan, scatter, composite (tilelist.hip, composite2.hip).
// fused_keys: the caller's key buffer of a fused draw (the projection wrote the keys there and nowhere else), else null
int enqueue_raster_v2(gs4d_ctx* c, Lane& L, Framebuffer& F, const DrawArgs& a, size_t nrecords, int premult_c, const uint32_t* fused_keys) {
    const size_t ntiles = (size_t)c->tiles_x * c->tiles_y;
    uint2* tmp = (uint2*)L.pair_keys;              // the lane's entry storage holds 16 bytes per slot: [0, cap) bucket order, [cap, 2 cap) tile order
    uint2* entries = tmp + L.pair_cap;
    int recbits = 1; while (recbits < 32 && ((size_t)1 << recbits) < nrecords) ++recbits;
    {
        StageTimer t(c, GS4D_T_BINNING);
        bool skip_lists = false;
#ifdef GS4D_TUNING
        { static const bool sk = getenv("GS4D_ABLATE_SCATTER") != nullptr; static int warm = 0; skip_lists = sk && ++warm > 16; }      // ablation: steady-state frames reuse the bucket array of an earlier frame of their lane (same scene): what scan + scatter cost the frame
#endif
        if (L.tl.staged) {
            // staged: the projection kernel wrote the segment blocks; one kernel turns them into tile lists and checks what the host guessed
            HIPCHK(c, launch_bucket_tiles_staged(L.s, L.tl, ntiles, c->tiles_x, L.bin.total, entries, c->list_hint));
            c->stat_staged++;
        } else {
            if (!skip_lists) {
            HIPCHK(c, launch_bucket_scan(L.s, L.tl, L.bin.total, L.host_total_dev, L.pair_cap));
            HIPCHK(c, launch_bucket_scatter(L.s, L.tl, L.trects, L.proj, fused_keys, a.blend_order.ks.bias, nrecords, L.bin.total, tmp, c->tiles_x, a.shard_rank, a.shard_world));
            }
            HIPCHK(c, launch_bucket_tiles(L.s, L.tl, ntiles, L.bin.total, tmp, entries, c->list_hint));
        }
    }
    c->stat_tile_passes = 0;
#ifdef GS4D_TUNING
    { static const bool skip = getenv("GS4D_ABLATE_COMPOSITE") != nullptr; if (skip) { HIPCHK(c, hipEventRecord(L.ev_emit, L.s)); return GS4D_OK; } }      // ablation: the frame without its compositing kernel (steady state only: the verdict words keep their last values)
#endif
    {
        StageTimer t(c, GS4D_T_COMPOSITE);
        HIPCHK(c, launch_composite_v2(L.s, L.proj, entries, L.tl, L.bin.total, L.host_total_dev, c->tiles_x, c->tiles_y, c->W, c->H, premult_c, draw_target(c, F, a), c->list_hint, a.blend_order.bits, recbits, a.draw_ord));
    }
    // (the box's width and height clipped to the image's: more tiles than tile_box() launches when a box starts away from the left / top edge and overhangs the far one)
    { const uint32_t b = L.tl.staged ? L.tl.box : BOX_NONE; c->stat_composited_tiles = b == BOX_NONE ? ntiles : (uint64_t)std::min<uint32_t>((box_x1(b) - box_x0(b) + 1u) * BOX_BLOCK, (uint32_t)c->tiles_x) * std::min<uint32_t>((box_y1(b) - box_y0(b) + 1u) * BOX_BLOCK, (uint32_t)c->tiles_y); }
    HIPCHK(c, hipEventRecord(L.ev_emit, L.s));         // totals, flags and the longest list are in pinned host memory behind this event (the compositor's first workgroup wrote them)
    return GS4D_OK;
}

// width of a key span in bits (what the depth sort and the compositor's list sort have to look at)
static int span_bits(uint32_t span) { return span == 0xFFFFFFFFu ? 32 : std::max(1, 32 - __builtin_clz(span | 1u)); }

// Enqueue on lane L: k_keygen for the first n records of D in order `ks` into (keys, idx), every key checked against `span`, and — `sort` — the
// stable sort of those pairs on `bits` bits: idx then holds "records in ascending (depth key, record index)".  timed: as GS4D_T_KEYGEN / GS4D_T_SORT.
int enqueue_keygen_sort(gs4d_ctx* c, Lane& L, const Buffer& D, size_t n, const KeySrc& ks, uint32_t span, int bits, uint32_t* keys, uint32_t* idx, bool sort, bool timed) {
    {
        hipError_t he = hipSuccess;
        uint32_t* kh = sort_hist_slot(L.s, L.depth_sort, n, &he);
        if (!kh) return hipfail(c, he, "sort_hist_slot");
        StageTimer tm(c, timed ? GS4D_T_KEYGEN : -1);
        sort_plan_hist(L.depth_sort, n, bits);             // LSD passes or the hybrid: chosen before the keys exist, the producer counts the digits of that plan
        HIPCHK(c, launch_keygen(L.s, D.soa, soa_sig3(D.soa, D.soa_n, D.soa_info), D.soa_info, n, ks, (float*)keys, idx, kh, L.depth_sort.hist_rb, L.depth_sort.hist_rows, L.depth_sort.hist_top, span, L.err_word()));
        L.depth_sort.hist_bias = ks.bias;
    }
    StageTimer t(c, sort && timed ? GS4D_T_SORT : -1);
    if (sort) HIPCHK(c, radix_sort_pairs(L.s, L.depth_sort, keys, idx, n, nullptr, bits, true));
    return GS4D_OK;
}

// ---- the steps of run_draw, in the order it takes them ----
// The shape of a draw, from its mode and buffers.  npre: records to project; ob: the caller's sort index (null when the draw regenerates its order)
struct DrawShape { Buffer* data = nullptr; Buffer* ob = nullptr; size_t nrec = 0, npre = 0; int premult = 0; bool empty = false; };
int draw_shape(gs4d_ctx* c, const DrawArgs& a, DrawShape& s) {
    s.data = getbuf(c, a.data);
    if (!s.data) return fail(c, GS4D_E_INVALID, "draw: no splat data buffer bound");
    const size_t bytes = s.data->bytes;
    if (a.quads) { s.nrec = bytes / 288; s.npre = std::min(s.nrec, a.instances); s.premult = 1; }
    else if (a.mode == GS4D_MODE_4D_SORTED) {
        if (!a.regen_order) {
            s.ob = getbuf(c, a.order);
            if (!s.ob) return fail(c, GS4D_E_INVALID, "draw: GS4D_MODE_4D_SORTED needs the sort-index buffer at slot 1");
            if (s.ob->bytes < a.instances * 4) return fail(c, GS4D_E_INVALID, "draw: sort-index buffer smaller than the instance count");
        }
        s.nrec = s.npre = bytes / 96;
    } else if (a.mode == GS4D_MODE_4D_DIRECT) { s.nrec = bytes / 96; s.npre = std::min(s.nrec, a.instances); }
    else if (a.mode == GS4D_MODE_2D) { s.nrec = bytes / 48; s.npre = std::min(s.nrec, a.instances); }
    else return fail(c, GS4D_E_INVALID, "draw: mode does not match the draw call");
    s.empty = a.instances == 0 || s.nrec == 0;
    if (!s.empty && (a.instances >= 0xFFFFFFFFull || s.nrec >= 0xFFFFFFFFull)) return fail(c, GS4D_E_UNSUPPORTED, "draw: more than 2^32-1 instances");
    return GS4D_OK;
}

// the statistics of a draw belong to a list geometry (buckets, segments, tiles, records, shard, data buffer): another one starts from scratch
uint64_t list_geometry(const gs4d_ctx* c, const TileLists& tl, const DrawArgs& a, size_t npre) {
    uint64_t geom = 0xcbf29ce484222325ull;
    for (uint64_t v : { (uint64_t)tl.nb, (uint64_t)tl.rows, (uint64_t)tl.seg, (uint64_t)c->tiles_x, (uint64_t)c->tiles_y, (uint64_t)npre, (uint64_t)a.shard_world, (uint64_t)a.shard_rank, (uint64_t)a.data })
        geom = (geom ^ v) * 0x100000001b3ull;
    return geom;
}
// Staged lists for an unordered draw whose geometry (a.stage_geom) has reported its statistics: capacities, blocks, sequence number and launch
// box.  Leaves L.tl as it is (not staged) when the draw has to build exact lists.
int plan_staged(gs4d_ctx* c, Lane& L, const DrawArgs& a) {
    if (!(c->stage_enable && c->stage_known && c->stage_geom == a.stage_geom && !a.exact_lists && L.tl.seg <= (uint32_t)(STAGE_R * SEG_THREADS))) return GS4D_OK;
    // margins: an eighth on the fullest segment and on the fullest bucket (the longest run is no capacity of anything any more: statistics only)
    const uint64_t scap = ((uint64_t)c->stage_max_seg + c->stage_max_seg / 8 + 64 + 63) & ~63ull;
    const uint64_t bcap = ((uint64_t)c->stage_max_bucket + c->stage_max_bucket / 8 + 512 + 63) & ~63ull;
    if (!(scap <= STAGE_MAX_SCAP && bcap <= 32u * 512u && (uint64_t)L.tl.nb * bcap < 0xFFFFFFF0ull)) return GS4D_OK;      // (k_bucket_tiles_staged: a thread holds at most 32 of its bucket's entries)
    HIPCHK(c, tile_lists_reserve_blocks(L.s, L.tl, (size_t)L.tl.rows * scap));
    L.tl.staged = true; L.tl.scap = (uint32_t)scap; L.tl.bcap = (uint32_t)bcap;
    if (++L.tl.seq == 0u) L.tl.seq = 1u;
    // the compositor's launch box: where the last staged draw had entries, stage_box_margin blocks (of 4 x 4 tiles) wider on every side
    const uint32_t nbx = (uint32_t)(c->tiles_x + BOX_BLOCK - 1) / BOX_BLOCK, nby = (uint32_t)(c->tiles_y + BOX_BLOCK - 1) / BOX_BLOCK;
    if (c->stage_box_enable && c->stage_box != BOX_NONE && c->stage_box != BOX_EMPTY && nbx <= 256u && nby <= 256u) {
        const uint32_t b = c->stage_box, m = c->stage_box_margin;
        L.tl.box = box_pack(box_x0(b) > m ? box_x0(b) - m : 0u, box_y0(b) > m ? box_y0(b) - m : 0u, std::min(box_x1(b) + m, nbx - 1u), std::min(box_y1(b) + m, nby - 1u));
    }
    return GS4D_OK;
}

// The sort index of an ordered draw: `order` (in: the caller's, or null) is what the binning reads, `order_copy` where its emit kernel keeps a copy.
int order_source(gs4d_ctx* c, Lane& L, const DrawArgs& a, bool regen, bool preprocess, const uint32_t*& order, uint32_t*& order_copy) {
    if (!order && !regen) return GS4D_OK;
    HIPCHK(c, grow_device_array(L.s, L.order_copy, L.order_cap, a.instances));
    if (regen) order = L.order_copy;                   // filled by regenerate_order (first re-run) or by an earlier re-run of this draw
    else if (preprocess) order_copy = L.order_copy;   // first run: the emit kernel reads the caller's buffer and keeps a copy
    else order = L.order_copy;                         // re-run: the caller's buffer may have been overwritten since
    return GS4D_OK;
}
// the key and index buffers of the queued key generation a fused draw executes, looked up once per run (null: deleted since)
struct FusedBuffers { Buffer* keys = nullptr; Buffer* idx = nullptr; };
// what the projection kernel does beside projecting: count or write the list entries (unordered: L.tl), generate depth keys and their histograms (fused)
int fill_tile_count(gs4d_ctx* c, Lane& L, const DrawArgs& a, size_t npre, bool v2, const FusedBuffers& fused, TileCount& tc) {
    const bool staged = v2 && L.tl.staged;
    uint32_t* kh = nullptr;
    if (a.fuse) {
        if (!fused.keys || !fused.idx) return fail(c, GS4D_E_INVALID, "draw: the key buffers of the queued key generation have been deleted");
        hipError_t he = hipSuccess;
        kh = sort_hist_slot(L.s, L.depth_sort, npre, &he);
        if (!kh) return hipfail(c, he, "sort_hist_slot");
        L.depth_sort.hist_bias = a.blend_order.ks.bias;
        // A staged draw reads no key back (k_bucket_scatter, which takes the keys of an exact-list draw from the caller's buffer, does not run) and nothing
        // observes the buffers before the sort queued behind this draw: its hybrid sort may be segment-fed — the projection leaves each segment's keys
        // grouped by top digit in the sort's own blocks instead of the caller's key buffer, and the sort is k_os_tail alone.
        sort_plan_hist(L.depth_sort, npre, a.blend_order.bits, staged && L.tl.seg <= SEGFEED_BLOCK ? L.tl.rows : 0u);
    }
    // the form, decided here and nowhere else (hist_segfeed: what sort_plan_hist has just planned — with segments only, so SegmentFed comes with Stage)
    tc.lists = !v2 ? ProjLists::None : staged ? ProjLists::Stage : ProjLists::Count;
    tc.keys = !a.fuse ? ProjKeys::None : L.depth_sort.hist_segfeed ? ProjKeys::SegmentFed : ProjKeys::Write;
    if (v2 || a.fuse) tc.ks = a.blend_order.ks;
    if (tc.lists != ProjLists::None) { tc.seg = L.tl.seg; tc.hist = L.tl.hist; tc.rows = L.tl.rows; tc.skey = L.tl.skey; tc.nb = L.tl.nb; tc.tiles_x = c->tiles_x; tc.shard_rank = a.shard_rank; tc.shard_world = a.shard_world; tc.sstat = L.tl.sstat; }
    if (tc.lists == ProjLists::Stage) { tc.stage_out = L.tl.blocks; tc.scap = L.tl.scap; tc.offs = L.tl.hist + L.tl.hist_cap; tc.abort_word = L.bin.total + TOT_ABORT; tc.seq = L.tl.seq; }
    if (tc.keys != ProjKeys::None) { tc.ghist = kh; tc.hist_rb = L.depth_sort.hist_rb; tc.hist_rows = L.depth_sort.hist_rows; tc.hist_top = L.depth_sort.hist_top; tc.span = a.blend_order.span; tc.err = L.err_word(); }
    if (tc.keys == ProjKeys::Write) tc.keys_out = (float*)fused.keys->d;      // (idx_out stays null: the depth sort that follows makes the identity index up)
    if (tc.keys == ProjKeys::SegmentFed) { tc.seg_pairs = L.depth_sort.seg_pairs; tc.seg_runs = L.depth_sort.seg_runs; }
    return GS4D_OK;
}

// The projection of the draw's records into L.proj / L.trects, behind whoever wrote the data (and, on the ordered path, the sort index).
int enqueue_projection(gs4d_ctx* c, Lane& L, const DrawArgs& a, const DrawShape& s, bool v2, const FusedBuffers& fused) {
    Buffer* const data = s.data;
    if (L.proj_cap < s.npre) {      // two arrays, one capacity: it stands only when both do
        size_t pcap = L.proj_cap, tcap = L.proj_cap;
        hipError_t e = grow_device_array(L.s, L.proj, pcap, s.npre, PROJ_FLOATS * 4);
        if (e == hipSuccess) e = grow_device_array(L.s, L.trects, tcap, s.npre);
        L.proj_cap = std::min(pcap, tcap);
        if (e != hipSuccess) return hipfail(c, e, "grow_device_array(L.proj, L.trects)");
    }
    if (!a.quads && (a.mode == GS4D_MODE_4D_SORTED || a.mode == GS4D_MODE_4D_DIRECT)) { int rc = ensure_soa(c, *data); if (rc) return rc; }
    { int rc = lane_access(c, *data, false); if (rc) return rc; data->rd_mask |= 1u << a.lane; }
    if (s.ob && !v2) { int rc = lane_access(c, *s.ob, false); if (rc) return rc; s.ob->rd_mask |= 1u << a.lane; }
    {
        StageTimer t(c, GS4D_T_PREPROCESS);
        // entries that cannot change a pixel are not built (a.lean: decided when the draw was issued, draw_common)
        const PreOut po = { L.proj, (v2 && L.tl.staged) ? nullptr : L.trects, has_aux(a.out) || a.zplane != 0, a.lean && c->cull_alpha0, a.lean && c->tight_rect };
        L.trects_in_order = false;
        TileCount tc;
        { int rc = fill_tile_count(c, L, a, s.npre, v2, fused, tc); if (rc) return rc; }
        if (a.quads) HIPCHK(c, launch_preprocess_3d(L.s, (const float*)data->d, s.npre, a.u, c->W, c->H, po, tc));
        else if (a.mode == GS4D_MODE_2D) HIPCHK(c, launch_preprocess_2d(L.s, (const float*)data->d, s.npre, a.u, c->W, c->H, po, tc));
        else {
            HIPCHK(c, launch_preprocess_4d(L.s, data->soa, data->soa_n, data->soa_info, s.npre, a.u, c->W, c->H, po, tc));
            c->stat_shadow_bytes = data->soa_info.layout == SOA_STATIC3D ? 64 : data->soa_info.layout == SOA_SYM ? 72 : 96;
        }
    }
    L.proj_n = s.npre;
    return GS4D_OK;
}

// "Records in ascending (depth key, record index)" — what the caller's index held when the draw was issued — from the order the draw
// carries: k_keygen + the stable sort, into the lane's own buffers (DrawArgs::regen_order)
int regenerate_order(gs4d_ctx* c, Lane& L, const DrawArgs& a, const Buffer& data, size_t npre) {
    HIPCHK(c, grow_device_array(L.s, L.regen_keys, L.regen_cap, npre));
    return enqueue_keygen_sort(c, L, data, npre, a.blend_order.ks, 0xFFFFFFFFu, a.blend_order.bits, L.regen_keys, L.order_copy, true, false);
}
// The depth sort a fused draw executes for the application, on the keys and digit histograms its projection left.  Ordered path: between projection
// and binning, which reads the sorted index.  Unordered (`after_raster`): nothing in the draw waits for it; it fills the caller's buffers for the next reader.
int enqueue_fused_sort(gs4d_ctx* c, Lane& L, const DrawArgs& a, const FusedBuffers& fused, size_t npre, bool after_raster) {
    StageTimer t(c, GS4D_T_SORT);
#ifdef GS4D_TUNING
    static const bool skip_sort = getenv("GS4D_ABLATE_SORT") != nullptr;      // ablation (make TUNING=1): what the frame costs without its depth sort — an upper bound for any re-scheduling of it
    if (after_raster && skip_sort) { L.depth_sort.hist_pending = false; L.depth_sort.flip ^= 1; return GS4D_OK; }
#endif
    HIPCHK(c, radix_sort_pairs(L.s, L.depth_sort, (uint32_t*)fused.keys->d, (uint32_t*)fused.idx->d, npre, nullptr, a.blend_order.bits, true, true));
    return GS4D_OK;
}

// the depth-test plane: read by the compositing kernel (first run and re-runs alike), so the lane waits for whoever wrote it, and a
// later write waits for this lane's tail event (the compositor runs after the draw's binning-done event)
int order_depth_plane(gs4d_ctx* c, const DrawArgs& a) {
    Buffer* Z = getbuf(c, a.zplane);
    if (!Z || Z->bytes < (size_t)c->W * c->H * 4) return fail(c, GS4D_E_INVALID, "draw: the depth-test plane holds fewer than width*height floats");
    int rc = lane_access(c, *Z, false); if (rc) return rc;
    Z->tail_mask |= 1u << a.lane;
    return GS4D_OK;
}
// The record-statistics buffer: the compositing kernel ADDS to it with atomics (first run and re-runs alike — an aborted run adds nothing), so
// lanes need no order among themselves: the draw takes it as a reader does (behind whoever WROTE it with a kernel), and a later kernel write waits
// for this lane's tail event.  A host access (read, subdata, invalidate, destroy) settles every lane's pending draws and waits for all of them.
int order_record_stats(gs4d_ctx* c, const DrawArgs& a) {
    Buffer* S = getbuf(c, a.stats);
    if (!S || S->bytes / sizeof(gs4d_record_stat) < a.stats_n) return fail(c, GS4D_E_INVALID, "draw: the record-statistics buffer holds fewer than nrecords entries");
    int rc = lane_access(c, *S, false); if (rc) return rc;
    if (S->scan_wait & (1u << c->cur)) {                       // behind a compaction that is still reading the table on another lane
        HIPCHK(c, hipStreamWaitEvent(lane(c).s, S->ev_scan, 0));
        S->scan_wait &= ~(1u << c->cur);
    }
    S->tail_mask |= 1u << a.lane;
    S->stats_target = true;
    S->version++;
    return GS4D_OK;
}
// entry storage for the draw: twice its instances, or one and a half times what the last draw needed, or the bucket regions of a staged draw
int reserve_entries(gs4d_ctx* c, Lane& L, const DrawArgs& a, bool v2) {
    size_t want = a.instances * 2 + 65536;
    if (want < c->stat_entries + c->stat_entries / 2) want = c->stat_entries + c->stat_entries / 2;
    if (v2 && L.tl.staged && want < (size_t)L.tl.nb * L.tl.bcap) want = (size_t)L.tl.nb * L.tl.bcap;      // staged: the tile-ordered array holds a region of bcap entries per bucket
    return ensure_pairs(c, L, want);
}

// `preprocess` false: the re-run of a draw whose tile lists overflowed (projected records and the sort-index copy are still valid).  Sets a.stage_geom.
int run_draw(gs4d_ctx* c, DrawArgs& a, bool preprocess) {
    Lane& L = c->lanes[a.lane];
    Framebuffer& F = c->fbs[a.fb];
    const size_t ntiles = (size_t)c->tiles_x * c->tiles_y;
    DrawShape s;
    { int rc = draw_shape(c, a, s); if (rc || s.empty) return rc; }
    HIPCHK(c, bin_scratch_reserve(L.s, L.bin, a.instances, ntiles));
    const bool v2 = a.v2 && tile_lists_plan(L.tl, ntiles, s.npre, c->slabs, a.blend_order.bits, a.blend_order.span);
    if (v2) { HIPCHK(c, tile_lists_reserve(L.s, L.tl, ntiles, s.npre)); preprocess = true; }   // an unordered draw is always re-run from the projection
    L.tl.staged = false; L.tl.scap = L.tl.bcap = 0; L.tl.box = BOX_NONE;
    if (v2) { a.stage_geom = list_geometry(c, L.tl, a, s.npre); int rc = plan_staged(c, L, a); if (rc) return rc; }
    const bool regen = a.regen_order && !v2 && a.mode == GS4D_MODE_4D_SORTED && !a.quads;
    const uint32_t* order = (s.ob && !v2) ? (const uint32_t*)s.ob->d : nullptr;      // (an unordered draw never reads its sort index)
    uint32_t* order_copy = nullptr;
    { int rc = order_source(c, L, a, regen, preprocess, order, order_copy); if (rc) return rc; }
    const FusedBuffers fused = a.fuse ? FusedBuffers{ getbuf(c, a.fuse_keys), getbuf(c, a.fuse_idx) } : FusedBuffers{};
    if (preprocess) {
        { int rc = enqueue_projection(c, L, a, s, v2, fused); if (rc) return rc; }
        if (regen) { int rc = regenerate_order(c, L, a, *s.data, s.npre); if (rc) return rc; }
        { int rc = fb_access(c, F); if (rc) return rc; }
        if (a.fuse && !v2) { int rc = enqueue_fused_sort(c, L, a, fused, s.npre, false); if (rc) return rc; }
    }
    if (a.zplane) { int rc = order_depth_plane(c, a); if (rc) return rc; }
    if (a.stats) { int rc = order_record_stats(c, a); if (rc) return rc; }
    { int rc = reserve_entries(c, L, a, v2); if (rc) return rc; }
    if (!v2) return enqueue_raster(c, L, F, a, order, order_copy, a.instances, s.npre, s.premult);
    int rc = enqueue_raster_v2(c, L, F, a, s.npre, s.premult, fused.keys ? (const uint32_t*)fused.keys->d : nullptr);
    if (rc == GS4D_OK && a.fuse) rc = enqueue_fused_sort(c, L, a, fused, s.npre, true);
    return rc;
}

// What a draw's kernels left in the lane's host verdict words (HT_*, gs4d_internal.h), decoded once behind the lane's event.
struct Verdict { uint64_t entries; uint32_t flags, longest_list, longest_run, fullest_bucket, fullest_seg, used_box; };
Verdict read_verdict(const uint32_t* ht) { return Verdict{ (uint64_t)ht[HT_COUNT_LO] | ((uint64_t)ht[HT_COUNT_HI] << 32), ht[HT_FLAGS], ht[HT_LONGEST_LIST], ht[HT_LONGEST_RUN], ht[HT_FULLEST_BUCKET], ht[HT_FULLEST_SEG], ht[HT_USED_BOX] }; }

// A draw's tile-list capacity is validated after the fact: the entry count comes back through pinned memory behind an event.
// Called by every entry point that could observe the draw's result.  On overflow the raster stages are re-run with exact capacity
// (the projected records and the copy of the sort index are still valid).
int resolve_lane(gs4d_ctx* c, int li) {
    Lane& L = c->lanes[li];
    while (L.pending) {
        HIPCHK(c, hipEventSynchronize(L.ev_emit));     // the entry count is final once the binning kernel (ordered path) / the tile scan (unordered path) has run
        L.pending = false;
        const bool discarded = L.discarded;             // the image was cleared before anybody looked: learn from the draw, do not repeat it
        L.discarded = false;
        if (L.host_total[HT_ERROR]) return fail(c, GS4D_E_DEVICE, DEVICE_CHECK_MSG);
        const Verdict v = read_verdict(L.host_total);
        if (L.pending_args.v2 && !(v.flags & VF_CAPACITY)) {
            // longest (bucket, segment) run and fullest bucket of this draw: what sizes the staged blocks of the draws that follow
            c->stage_max_run = v.longest_run; c->stage_max_bucket = v.fullest_bucket; c->stage_max_seg = v.fullest_seg; c->stage_geom = L.pending_args.stage_geom; c->stage_known = true;
            c->stage_box = v.used_box;
            if ((v.flags & VF_STAGED_MISS) && L.tl.box != BOX_NONE && v.used_box != BOX_NONE && v.used_box != BOX_EMPTY && !box_within(L.tl.box, v.used_box))
                c->stage_box_margin = std::min(16u, c->stage_box_margin * 2u);      // the picture moves faster than the margin allowed
        }
        if (L.pending_args.v2) {
            c->stat_longest = v.longest_list;
            // the compositor's occupancy falls with the list capacity it is launched for: give capacity back when the lists stay short
            const uint32_t fit = v2_list_capacity(std::min<uint32_t>(V2_MAX_LIST, v.longest_list + v.longest_list / 8u));
            if (!v.flags && fit < c->list_hint) { if (++c->shrink_votes >= 8) { c->list_hint = fit; c->shrink_votes = 0; } } else c->shrink_votes = 0;
        }
        if (!v.flags) { c->stat_entries = v.entries; break; }
        if (v.entries >= 0xFFFFFFF0ull) { if (discarded) break; return fail(c, GS4D_E_UNSUPPORTED, "draw: more than 2^32 tile-list entries (splats cover too many tiles)"); }
        if (discarded) c->stat_aborted_discarded++; else c->stat_reruns++;
        c->stat_entries = v.entries;
        const bool was_v2 = L.pending_args.v2;     // an unordered draw kept no copy of its sort index: whatever path the re-run takes, it starts from the projection
        if (L.pending_args.v2 && (v.flags & VF_STAGED_MISS)) { L.pending_args.exact_lists = true; c->stat_staged_misses++; }      // a run or a bucket did not fit the guess: exact lists this time
        if (L.pending_args.v2 && (v.flags & VF_LIST)) {
            // A (sub-)list longer than the compositing wave was launched for.  What it can hold is a launch parameter (64 entries per lane
            // register: v2_list_capacity) that costs registers and LDS.  Up to V2_MAX_LIST entries: a capacity that fits.  Longer: this is a
            // scene for the instance-ordered path (the re-run regenerates the order the draw was issued with: DrawArgs::regen_order).
            if (v.longest_list <= V2_MAX_LIST) c->list_hint = std::max(c->list_hint, v2_list_capacity(v.longest_list + v.longest_list / 8u));
            else { c->long_lists = true; c->ordered_draws = 0; L.pending_args.v2 = false; L.pending_args.regen_order = true; }
        }
        int rc = ensure_pairs(c, L, (size_t)(v.entries + v.entries / 8 + 1024));
        if (rc) return rc;
        if (discarded) break;                           // the lane's next draw starts with what this one found out
        // the re-run goes to the draw's own lane: make it current while its kernels are queued
        const int saved = c->cur;
        c->cur = li;
        rc = run_draw(c, L.pending_args, was_v2);
        // Other lanes order themselves after this lane through its tail event (fb_access, lane_access), which was recorded when the lane was
        // left — before this re-run.  Record it again so that it keeps covering everything queued on the lane.
        if (rc == GS4D_OK && li != saved) { hipError_t he = hipEventRecord(L.ev_tail, L.s); if (he != hipSuccess) { c->cur = saved; return hipfail(c, he, "hipEventRecord"); } }
        c->cur = saved;
        if (rc) return rc;
        L.pending = true;
    }
    return GS4D_OK;
}

int flush_order(gs4d_ctx* c);

// every lane (calls that observe or tear down everything)
int resolve_pending(gs4d_ctx* c) {
    { int rc = flush_order(c); if (rc) return rc; }
    for (int i = 0; i < c->nlanes; ++i) { int rc = resolve_lane(c, i); if (rc) return rc; }
    return GS4D_OK;
}

// the draws that rendered into image `fb` (calls that observe that image)
int resolve_image(gs4d_ctx* c, int fb) {
    for (int i = 0; i < c->nlanes; ++i)
        if (c->lanes[i].pending && c->lanes[i].pending_args.fb == fb) { int rc = resolve_lane(c, i); if (rc) return rc; }
    return GS4D_OK;
}

int host_access(gs4d_ctx* c, Buffer& B) {
    if (B.touch <= c->synced) return GS4D_OK;
    int rc = resolve_pending(c); if (rc) return rc;
    rc = sync_all(c); if (rc) return rc;
    B.wr_lane = -1; B.rd_mask = 0; B.tail_mask = 0; B.ordered_mask = 0; B.stats_target = false; B.scan_wait = 0;
    return GS4D_OK;
}

// Launch a queued gs4d_keygen (+ gs4d_sort_pairs) as kernels of their own: somebody is about to look at the buffers, or the draw that
// follows cannot use them.  The lane has not changed since they were queued (only frame-starting calls change it, and they flush first).
int flush_order(gs4d_ctx* c) {
    if (!c->po.keygen) return GS4D_OK;
    auto po = c->po;
    c->po.keygen = c->po.sorted = false;
    Lane& L = c->lanes[po.lane];
    Buffer* D = getbuf(c, po.data); Buffer* K = getbuf(c, po.keys); Buffer* I = getbuf(c, po.idx);
    if (!D || !K || !I || !D->soa) return fail(c, GS4D_E_INVALID, "queued keygen: a buffer it names has been deleted");
    return enqueue_keygen_sort(c, L, *D, po.n, po.order.ks, po.order.span, po.order.bits, (uint32_t*)K->d, (uint32_t*)I->d, po.sorted, true);
}

int alloc_fbs(gs4d_ctx* c, int w, int h) {
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return fail(c, GS4D_E_INVALID, "framebuffer size must be 1..65535");
    { int rc = sync_all(c); if (rc) return rc; }
    for (int i = 0; i < c->nlanes; ++i) {
        if (c->fbs[i].mem) { (void)hipFree(c->fbs[i].mem); c->fbs[i].mem = nullptr; }
        if (c->fbs[i].tstate) { (void)hipFree(c->fbs[i].tstate); c->fbs[i].tstate = nullptr; }
        if (c->fbs[i].linecnt) { (void)hipFree(c->fbs[i].linecnt); c->fbs[i].linecnt = nullptr; }
        c->fbs[i].free_planes();                                 // (no frame of this size has been cleared yet: back to Outputs::Colour)
        HIPCHK(c, hipMalloc(&c->fbs[i].mem, (size_t)w * h * 16));
        HIPCHK(c, c->fbs[i].reserve_planes(c->planes, w, h));
        const size_t nt = (size_t)((w + TILE - 1) / TILE) * ((h + TILE - 1) / TILE);
        HIPCHK(c, hipMalloc(&c->fbs[i].tstate, nt * 4));
        HIPCHK(c, hipMemset(c->fbs[i].tstate, 0, nt * 4));      // no tile is in memory: epochs start at 1
        c->fbs[i].epoch = 1; c->fbs[i].all_in_memory = false;
        c->fbs[i].is_clear = true; c->fbs[i].last_lane = -1; memcpy(c->fbs[i].clear, c->clear, 16);
    }
    c->W = w; c->H = h; c->tiles_x = (w + TILE - 1) / TILE; c->tiles_y = (h + TILE - 1) / TILE;
    c->cur_fb = c->cur; c->prev_fb = -1;
    return GS4D_OK;
}

// ---- frame-lane streams on hardware queues of their own ----
// HIP maps streams onto a few hardware queues (four by default) in an order that depends on every stream the process has created so far;
// two streams on one queue run their kernels one after the other.  Two frame lanes that share a queue do not overlap — measured: 0.110 ->
// 0.122 ms/frame at 10^6 splats when ONE foreign stream (a communicator's, a framework's) was alive while the context was created, or a
// context with another number of lanes had existed before (tools/order_effect.py, tools/queue_probe.hip).  So the lanes' streams are chosen
// by experiment: a candidate stream is accepted if a short kernel on it runs WHILE a spinning kernel occupies each stream accepted so far.
__global__ void k_lane_probe_spin(unsigned long long ticks, unsigned long long* out) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) { }                // bounded: the 100 MHz counter always advances
    out[0] = wall_clock64();
}
__global__ void k_lane_probe_stamp(unsigned long long* out) { out[0] = wall_clock64(); }

// false also when anything fails: the caller then simply keeps the stream
static bool streams_run_concurrently(hipStream_t a, hipStream_t b, unsigned long long* scratch /* device, 2 words */) {
    k_lane_probe_spin<<<dim3(1), dim3(1), 0, a>>>(10000ull /* 100 us of the 100 MHz counter: long against a launch, even under a tracing tool */, scratch);
    k_lane_probe_stamp<<<dim3(1), dim3(1), 0, b>>>(scratch + 1);
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return false;
    unsigned long long h[2] = { 0, 0 };
    if (hipMemcpy(h, scratch, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return false;
    return h[1] < h[0];                                     // the stamp was taken before the spin ended
}

#ifdef GS4D_TUNING
static unsigned long long* g_tuning_spin_out() { static unsigned long long* p = nullptr; if (!p && hipMalloc(&p, 16) != hipSuccess) p = nullptr; return p; }
#endif

static hipError_t create_lane_streams(gs4d_ctx* c) {
    hipError_t e;
    const bool probe = c->nlanes > 1 && !(getenv("GS4D_PROBE_QUEUES") && atoi(getenv("GS4D_PROBE_QUEUES")) == 0);      // test hook: 0 = take the streams as they come
    unsigned long long* scratch = nullptr;
    if (probe && hipMalloc(&scratch, 16) != hipSuccess) scratch = nullptr;
    std::vector<hipStream_t> good, rejected;
    const int max_tries = 3 * c->nlanes + 4;
    for (int t = 0; (int)good.size() < c->nlanes && t < max_tries; ++t) {
        hipStream_t s = nullptr;
        if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) break;
        bool ok = true;
        // (the test is a race against a 100-us spin: a host stall between the two launches looks like a shared queue — a stream is rejected only if it
        // fails against the same lane twice)
        if (scratch) for (hipStream_t g : good) if (!streams_run_concurrently(g, s, scratch) && !streams_run_concurrently(g, s, scratch)) { ok = false; break; }
        (ok ? good : rejected).push_back(s);
    }
    c->stat_lanes_sharing = 0;
    while ((int)good.size() < c->nlanes && !rejected.empty()) { good.push_back(rejected.back()); rejected.pop_back(); c->stat_lanes_sharing++; }      // fewer hardware queues than lanes: lanes will share
    c->stat_streams_rejected = rejected.size();
    for (hipStream_t s : rejected) (void)hipStreamDestroy(s);
    if (scratch) (void)hipFree(scratch);
    if ((int)good.size() < c->nlanes) { for (hipStream_t s : good) (void)hipStreamDestroy(s); return hipErrorOutOfMemory; }
    for (int i = 0; i < c->nlanes; ++i) c->lanes[i].s = good[i];
    return hipSuccess;
}

// ---- what the calls on record sets and tables share: a call makes its own scalar and query checks, declares its buffer arguments once (operands.h),
// ---- has them checked (check_operands), decides what n == 0 means, and queues its kernels from the same list (queue_operands) ----
// the stride rule of every such call
bool record_stride_ok(size_t stride) { return stride >= 16 && stride <= 1024 && stride % 16 == 0; }
// "<fn>: <msg>" as the refusal of a call: GS4D_E_INVALID
int refuse(gs4d_ctx* c, const char* fn, const std::string& msg) { return fail(c, GS4D_E_INVALID, (std::string(fn) + ": " + msg).c_str()); }
// The buffer arguments of a call, each declared once, with the buffers check_operands has found for them (null: not given)
struct Operands {
    static constexpr int MAX = 8;
    Operand op[MAX]; Buffer* buf[MAX] = {}; int count = 0; bool fits;      // (a list longer than MAX is refused by check_operands, never cut short)
    Operands(std::initializer_list<Operand> list) : fits(list.size() <= (size_t)MAX) { for (const Operand& o : list) if (count < MAX) op[count++] = o; }
    // the buffer of the argument `name`, and its storage (null: not given)
    Buffer* buffer(gs4d_buf name) const { for (int i = 0; i < count; ++i) if (name != 0 && op[i].name == name) return buf[i]; return nullptr; }
    void* ptr(gs4d_buf name) const { Buffer* B = buffer(name); return B ? B->d : nullptr; }
};
// The check of operands.h over the context's buffers; finds the buffers.  A fault: GS4D_E_INVALID with "<fn>: <operand> ...".
int check_operands(gs4d_ctx* c, const char* fn, Operands& ops) {
    if (!ops.fits) return refuse(c, fn, "more operands than Operands::MAX");
    const OperandVerdict v = check_operand_list(ops.op, ops.count, [&](uint32_t name) { Buffer* B = getbuf(c, name); return BufferFacts{ B != nullptr, B ? B->bytes : 0 }; });
    if (v.fault != OperandFault::None) return fail(c, GS4D_E_INVALID, operand_message(fn, ops.op, v).c_str());
    for (int i = 0; i < ops.count; ++i) ops.buf[i] = getbuf(c, ops.op[i].name);
    return GS4D_OK;
}

// A statistics table as a host read takes it: behind every draw issued so far, on every lane, re-runs included (settling draws does not move the
// current lane)
int settle_stats_table(gs4d_ctx* c, Buffer& S) { return S.stats_target ? host_access(c, S) : (int)GS4D_OK; }
// Kernels on lane L that read a table draws ADD to (Buffer::ev_scan, scan_wait) — three steps around their launch.  reserve: the event, with
// everything else that can fail without a kernel.
int scan_reserve(gs4d_ctx* c, Buffer& S) {
    if (!S.ev_scan) HIPCHK(c, hipEventCreateWithFlags(&S.ev_scan, hipEventDisableTiming));
    return GS4D_OK;
}
// before the launch: an earlier scan of the same table that another lane's draws still have to wait for — this lane waits for it, so that the event
// recorded behind the launch covers both
int scan_begin(gs4d_ctx* c, Lane& L, Buffer& S) {
    if (S.scan_wait & (1u << c->cur)) HIPCHK(c, hipStreamWaitEvent(L.s, S.ev_scan, 0));
    return GS4D_OK;
}
// behind the launch: draws that add to the table on the other lanes from now on wait until these kernels have read it (order_record_stats)
int scan_end(gs4d_ctx* c, Lane& L, Buffer& S) {
    HIPCHK(c, hipEventRecord(S.ev_scan, L.s));
    S.scan_wait = ((1u << c->nlanes) - 1u) & ~(1u << c->cur);
    return GS4D_OK;
}
// Kernels on the current frame lane over checked operands, each treated as its roles say (operands.h; an operand that is not given has none).
// prepare(lane): everything that can fail without a kernel — it comes before any buffer's state is touched; launch(lane) queues the kernels.
template <class Prepare, class Launch>
int queue_operands(gs4d_ctx* c, const Operands& ops, Prepare prepare, Launch launch) {
    auto each = [&](unsigned role, auto step) { int rc = GS4D_OK; for (int i = 0; i < ops.count && !rc; ++i) if (ops.buf[i] && (ops.op[i].roles & role)) rc = step(*ops.buf[i]); return rc; };
    // a queued key generation / sort that names one of the buffers runs first
    if (c->po.keygen) for (int i = 0; i < ops.count; ++i) if (ops.buf[i] && (ops.op[i].name == c->po.data || ops.op[i].name == c->po.keys || ops.op[i].name == c->po.idx)) { int rc = flush_order(c); if (rc) return rc; break; }
    { int rc = each(OP_SETTLE, [&](Buffer& B) { return settle_stats_table(c, B); }); if (rc) return rc; }
    // a draw that is still unvalidated may have to be run again from the buffers it was given: none of those is overwritten before that is settled
    bool touched = false;
    (void)each(OP_WRITE, [&](Buffer& B) { touched |= B.touch > c->synced; return (int)GS4D_OK; });
    if (touched) { int rc = resolve_pending(c); if (rc) return rc; }
    Lane& L = lane(c);
    { int rc = prepare(L); if (rc) return rc; }
    { int rc = each(OP_SCAN, [&](Buffer& B) { return scan_reserve(c, B); }); if (rc) return rc; }
    const unsigned me = 1u << c->cur;
    { int rc = each(OP_READ, [&](Buffer& B) { int r = lane_access(c, B, false); if (!r) B.tail_mask |= me; return r; }); if (rc) return rc; }
    { int rc = each(OP_WRITE, [&](Buffer& B) { int r = lane_access(c, B, true); if (!r) { B.version++; B.prov_valid = false; } return r; }); if (rc) return rc; }
    { int rc = each(OP_SCAN, [&](Buffer& B) { return scan_begin(c, L, B); }); if (rc) return rc; }
    { int rc = launch(L); if (rc) return rc; }
    return each(OP_SCAN, [&](Buffer& B) { return scan_end(c, L, B); });
}
// ... for a call that has nothing to prepare
template <class Launch>
int queue_operands(gs4d_ctx* c, const Operands& ops, Launch launch) { return queue_operands(c, ops, [](Lane&) { return (int)GS4D_OK; }, launch); }

// gs4d_keep_rule as the kernels take it; null — a call whose table is optional was given none — is the rule no kernel reads.  False: an unknown flag
// or a non-zero reserved field.
bool keep_rule_of(const gs4d_keep_rule* rule, KeepRule& out) {
    out = KeepRule{ 0u, 0u, 0ull, 0u };
    if (!rule) return true;
    if (rule->reserved != 0u || (rule->flags & ~(uint32_t)GS4D_KEEP_INVERT) != 0u) return false;
    out = KeepRule{ rule->min_pixels, rule->min_wmax, rule->min_wsum, rule->flags & (uint32_t)GS4D_KEEP_INVERT };
    return true;
}

// What gs4d_compact_records and gs4d_compact_time_window share: a table of one row of `row_bytes` per record (`what` names it in the messages) decides
// which of n records go from src to dst.  stats_table: the table is one that draws ADD to (Buffer::ev_scan).  launch(lane, table, records or null,
// dst or null, kept_index or null, cap) queues the kernels.
template <class Launch>
int compact_by_table(gs4d_ctx* c, const char* fn, const char* what, bool stats_table, gs4d_buf table, size_t row_bytes, size_t n,
                            gs4d_buf src, size_t stride, gs4d_buf dst, gs4d_buf kept_index, gs4d_buf count, Launch launch) {
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    if (!record_stride_ok(stride)) return refuse(c, fn, "stride must be a multiple of 16 from 16 to 1024");
    if (dst != 0 && src == 0) return refuse(c, fn, "dst given without src");
    // src holds its records whenever it is given, and is read only when there is somewhere to put them; dst and kept_index hold what they hold (cap)
    Operands ops{ { what, table, false, row_bytes, n, OP_READ | OP_SETTLE | (stats_table ? OP_SCAN : 0u) },
                  { "src", src, true, stride, n, dst ? OP_READ : 0u },
                  { "dst", dst, true, stride, 0, OP_WRITE },
                  { "kept_index", kept_index, true, 4, 0, OP_WRITE },
                  { "count", count, false, 1, sizeof(gs4d_compact_count), OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    // slots the outputs hold: no slot >= cap is ever written
    uint32_t cap = 0xFFFFFFFFu;
    if (Buffer* D = ops.buffer(dst)) cap = (uint32_t)std::min<size_t>(cap, D->bytes / stride);
    if (Buffer* X = ops.buffer(kept_index)) cap = (uint32_t)std::min<size_t>(cap, X->bytes / 4);
    return queue_operands(c, ops,
        [&](Lane& L) {
            HIPCHK(c, grow_device_array(L.s, L.compact_counts, L.compact_cap, std::max<size_t>(1, compact_tiles(n))));
            return (int)GS4D_OK;
        },
        [&](Lane& L) {
            HIPCHK(c, launch(L, ops.ptr(table), dst ? ops.ptr(src) : nullptr, ops.ptr(dst), (uint32_t*)ops.ptr(kept_index), cap, (gs4d_compact_count*)ops.ptr(count)));
            return (int)GS4D_OK;
        });
}

// What gs4d_count_neighbours, gs4d_label_components and gs4d_nearest_neighbours share: everything but the call's own checks, its names and its
// launch.  The checks are decided in this order: the query's, the call's own two among them, then the buffers'.
// The common fields of the three 32-byte queries — flags against the call's own known mask — with the verdict of the call's own check of the
// query (cap; k): its message, or null
struct GridQuery { float radius; uint32_t flags, known; const uint32_t* reserved; const char* query_fault; };
// The outputs behind data: `first` (first_arg: what the call calls it) is required, a row of first_row bytes per record (first_is_table: it is the
// statistics table itself, settled like one), `stats` is the optional table behind it (0: none, or none to give).  output_fault: the verdict of the
// call's own check of its outputs (hit_stride): its message, or null — first_row is not divided by before that.
struct GridOutputs { const char* first_arg; gs4d_buf first; size_t first_row; bool first_is_table; gs4d_buf stats; const char* output_fault; };
// launch(lane, records, source rows or null, rule, first, stats rows or null) queues the kernels on the lane's neighbour scratch and pair_sort.
template <class Launch>
int grid_query(gs4d_ctx* c, const char* fn, const GridQuery& q, size_t n, gs4d_buf data, gs4d_buf source, const gs4d_keep_rule* rule, const GridOutputs& o,
               Launch launch) {
    if ((q.flags & ~q.known) != 0u) return refuse(c, fn, "unknown flag");
    if (q.reserved[0] != 0u || q.reserved[1] != 0u || q.reserved[2] != 0u || q.reserved[3] != 0u) return refuse(c, fn, "non-zero reserved field in the query");
    if (q.query_fault) return refuse(c, fn, q.query_fault);
    if (!neighbour_radius_ok(q.radius)) return refuse(c, fn, "the radius must be finite with 2^-63 <= radius < 2^64");
    if (n >= 0xFFFFFFFFull) return refuse(c, fn, "the sort takes 2^32 - 2 records at most");
    if ((source != 0) != (rule != nullptr)) return refuse(c, fn, "source and rule are given together or not at all");
    KeepRule k;
    if (!keep_rule_of(rule, k)) return refuse(c, fn, "unknown flag or non-zero reserved field in the rule");
    if (o.output_fault) return refuse(c, fn, o.output_fault);
    // data and source are read (the 96-byte records, never a shadow: a reader leaves `version` alone; source as gs4d_edit_colours reads its table).
    // first is written; a statistics table among the outputs is a read-modify-write the lane has the table to itself for, as in gs4d_count_centres.
    // The tables are settled in this order: first, stats, source.
    Operands ops{ { "data", data, false, 96, n, OP_READ },
                  { o.first_arg, o.first, false, o.first_row, n, OP_WRITE | (o.first_is_table ? OP_SETTLE : 0u) },
                  { "stats", o.stats, true, sizeof(gs4d_record_stat), n, OP_WRITE | OP_SETTLE },
                  { "source", source, true, sizeof(gs4d_record_stat), n, OP_READ | OP_SETTLE | OP_SCAN } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops,
        [&](Lane& L) {
            HIPCHK(c, grow_device_array(L.s, L.neighbour_scratch, L.neighbour_cap, neighbour_scratch_words(n)));
            HIPCHK(c, sort_scratch_reserve(L.s, L.pair_sort, n));      // (the tile sort's scratch, as gs4d_spatial_order: a histogram a queued keygen has left in depth_sort stays where it is)
            return (int)GS4D_OK;
        },
        [&](Lane& L) { return launch(L, ops.ptr(data), (const gs4d_record_stat*)ops.ptr(source), k, ops.ptr(o.first), (gs4d_record_stat*)ops.ptr(o.stats)); });
}

} // namespace

extern "C" {

const char* gs4d_version(void) { return "gs4d 0.2 (gfx950)"; }

const char* gs4d_last_error(gs4d_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int gs4d_create(int device, int width, int height, gs4d_ctx** out) {
    if (!out) return fail(nullptr, GS4D_E_INVALID, "gs4d_create: out == NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(nullptr, GS4D_E_DEVICE, "gs4d_create: no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, GS4D_E_INVALID, "gs4d_create: bad device index");
    if ((e = hipSetDevice(device)) != hipSuccess) return hipfail(nullptr, e, "hipSetDevice");
    gs4d_ctx* c = new (std::nothrow) gs4d_ctx();
    if (!c) return fail(nullptr, GS4D_E_NOMEM, "gs4d_create: out of host memory");
    c->device = device;
    c->bufs.resize(1);
    memset(&c->u, 0, sizeof c->u);
    for (int i = 0; i < 4; ++i) c->u.view[5 * i] = c->u.proj[5 * i] = 1.0f;
    if (const char* ev = getenv("GS4D_LANES")) { const int v = atoi(ev); if (v >= 1 && v <= MAX_LANES) c->nlanes = v; }     // tuning knob
    if (const char* ev = getenv("GS4D_FUSE_KEYGEN")) c->defer_order = atoi(ev) != 0;                                       // test hook: 0 = launch key generation and sort at once
    if (const char* ev = getenv("GS4D_DRAW_PATH")) { if (!strcmp(ev, "ordered")) c->path_pref = 1; }
    if (const char* ev = getenv("GS4D_RENAME")) c->rename_storage = atoi(ev) != 0;
    if (const char* ev = getenv("GS4D_STAGED_BOX")) c->stage_box_enable = atoi(ev) != 0;                                   // test hook: 0 = the compositor of a staged draw is launched for every tile
    if (const char* ev = getenv("GS4D_STAGED")) c->stage_enable = atoi(ev) != 0;                                          // test hook: 0 = every unordered draw builds its lists exactly (scan + scatter)
    if (const char* ev = getenv("GS4D_CULL_ALPHA0")) c->cull_alpha0 = atoi(ev) != 0;                                      // test hook: 0 = records of alpha 0 keep their tile-list entries
    if (const char* ev = getenv("GS4D_TIGHT_RECT")) c->tight_rect = atoi(ev) != 0;                                        // test hook: 0 = the pixel rectangle is the quad's box
    if (const char* ev = getenv("GS4D_SLABS")) { const int v = atoi(ev); if (v >= 1 && v <= (int)V2_MAX_SLABS) { c->slabs = 1; while ((int)c->slabs < v) c->slabs *= 2u; } }      // test hook: depth slabs (a power of two)                         // test hook: instance-ordered tile lists for every draw
    auto bail = [&](int rc) { g_create_error = c->err; gs4d_destroy(c); return rc; };
    if ((e = create_lane_streams(c)) != hipSuccess) return bail(hipfail(c, e, "hipStreamCreate"));
    for (int i = 0; i < c->nlanes; ++i) {
        Lane& L = c->lanes[i];
        for (hipEvent_t* ev : { &L.ev_emit, &L.ev_tail }) {
            if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return bail(hipfail(c, e, "hipEventCreate"));
            if ((e = hipEventRecord(*ev, L.s)) != hipSuccess) return bail(hipfail(c, e, "hipEventRecord"));      // "already happened"
        }
        if ((e = hipHostMalloc((void**)&L.host_total, VERDICT_WORDS * 4, hipHostMallocMapped)) != hipSuccess) return bail(hipfail(c, e, "hipHostMalloc"));
        memset(L.host_total, 0, VERDICT_WORDS * 4);
        if ((e = hipHostGetDevicePointer((void**)&L.host_total_dev, L.host_total, 0)) != hipSuccess) return bail(hipfail(c, e, "hipHostGetDevicePointer"));
        L.depth_sort.err = L.pair_sort.err = L.err_word();
    }
    for (hipEvent_t* ev : { &c->ev_user, &c->ev_readback }) {
        if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return bail(hipfail(c, e, "hipEventCreate"));
    }
    {
        bool ordered = false;
        hipStream_t ls[MAX_LANES];
        for (int i = 0; i < c->nlanes; ++i) ls[i] = c->lanes[i].s;
        if ((e = lds_atomic_order_selftest(ls, c->nlanes, &ordered)) != hipSuccess) return bail(hipfail(c, e, "lds_atomic_order_selftest"));      // on every lane at once: beside other waves on the CUs
        c->atomic_rank = ordered;
    }
    const int shape_knob = getenv("GS4D_SORT_SHAPE") ? atoi(getenv("GS4D_SORT_SHAPE")) : 0, rank_knob = getenv("GS4D_SORT_RANK") ? atoi(getenv("GS4D_SORT_RANK")) : 0;
    for (int i = 0; i < c->nlanes; ++i) {
        for (SortScratch* ss : { &c->lanes[i].depth_sort, &c->lanes[i].pair_sort }) { ss->atomic_rank = c->atomic_rank; ss->shape_knob = shape_knob; ss->rank_knob = rank_knob; ss->rb_knob = getenv("GS4D_SORT_RB") ? atoi(getenv("GS4D_SORT_RB")) : 0; }
        // GS4D_SORT_HYBRID: 0 = depth sorts are the LSD passes, as before the hybrid existed; 1 = the hybrid for every eligible span, whatever n.  GS4D_SORT_TAILCAP: keys above
        // which a bucket of the hybrid takes the tail kernel's slow path (test hook: a runtime compare).  Both apply to both scratches of the lane.  Without
        // GS4D_SORT_HYBRID the lane's other scratch (pair_sort) never plans the hybrid; with it, the one sort there that can is gs4d_count_neighbours' (kb + 1 key
        // bits, 19..27 from 65537 records on, no producer: os_plan at the sort, k_os_hist counts the top-digit row alone, bias 0) — how the tests take the hybrid
        // through k_os_hist.  The others stay what they are: the tile-pair sort executes the plan of hist_rows / hist_top / hist_hybrid, which only sort_plan_hist
        // sets and nobody calls for pair_sort (every sort leaves them at the LSD plan), and has a device-side count (os_plan is not even asked); the reorder sort
        // has ORDER_KEY_BITS = 31 key bits, outside 19..27.
        c->lanes[i].pair_sort.hybrid_knob = 0;
        for (SortScratch* ss : { &c->lanes[i].depth_sort, &c->lanes[i].pair_sort }) {
            if (const char* ev = getenv("GS4D_SORT_HYBRID")) ss->hybrid_knob = atoi(ev) != 0 ? 1 : 0;
            if (const char* ev = getenv("GS4D_SORT_TAILCAP")) { const long v = atol(ev); if (v >= 1) ss->tail_cap = (uint32_t)std::min<long>(v, 1l << 30); }
        }
        // GS4D_SORT_SEGFEED: 0 = no hybrid sort is segment-fed; 1 = the hybrid sort of every staged fused frame is (sort_plan_hist), also with GS4D_SORT_HYBRID set;
        // unset = on, but only while GS4D_SORT_HYBRID is unset too: an explicit GS4D_SORT_HYBRID means the plans exactly as they were before the segment-fed form
        // existed.  The depth sort's scratch only: the lane's other scratch has no producer that writes segment blocks.
        if (const char* ev = getenv("GS4D_SORT_SEGFEED")) c->lanes[i].depth_sort.segfeed = atoi(ev) != 0;
        else c->lanes[i].depth_sort.segfeed = getenv("GS4D_SORT_HYBRID") == nullptr;
    }
    if (const char* ev = getenv("GS4D_NEIGHBOURS_PHASES")) c->neighbour_phases = std::min(4, std::max(1, atoi(ev)));
    int rc = alloc_fbs(c, width, height);
    if (rc) return bail(rc);
    *out = c;
    return GS4D_OK;
}

void gs4d_destroy(gs4d_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (int i = 0; i < MAX_LANES; ++i) if (c->lanes[i].s) (void)hipStreamSynchronize(c->lanes[i].s);
    for (auto& b : c->bufs) { if (b.d) (void)hipFree(b.d); if (b.soa) (void)hipFree(b.soa); if (b.bbox_dev) (void)hipFree(b.bbox_dev); if (b.ev_fill) (void)hipEventDestroy(b.ev_fill); if (b.ev_scan) (void)hipEventDestroy(b.ev_scan); }
    for (int i = 0; i < MAX_LANES; ++i) {
        Lane& L = c->lanes[i];
        if (c->fbs[i].mem) (void)hipFree(c->fbs[i].mem);
        if (c->fbs[i].tstate) (void)hipFree(c->fbs[i].tstate);
        if (c->fbs[i].linecnt) (void)hipFree(c->fbs[i].linecnt);
        c->fbs[i].free_planes();
        if (L.line_verts) (void)hipFree(L.line_verts);
        if (L.order_copy) (void)hipFree(L.order_copy);
        if (L.regen_keys) (void)hipFree(L.regen_keys);
        if (L.compact_counts) (void)hipFree(L.compact_counts);
        if (L.spatial_scratch) (void)hipFree(L.spatial_scratch);
        if (L.cut_scratch) (void)hipFree(L.cut_scratch);
        if (L.measure_scratch) (void)hipFree(L.measure_scratch);
        if (L.neighbour_scratch) (void)hipFree(L.neighbour_scratch);
        if (L.lod_state) (void)hipFree(L.lod_state);
        for (auto& sp : L.spare) { if (sp.d) (void)hipFree(sp.d); for (hipEvent_t e : sp.ev) if (e) (void)hipEventDestroy(e); }
        if (L.proj) (void)hipFree(L.proj);
        if (L.trects) (void)hipFree(L.trects);
        if (L.pair_keys) (void)hipFree(L.pair_keys);
        tile_lists_free(L.tl);
        sort_scratch_free(L.depth_sort); sort_scratch_free(L.pair_sort); bin_scratch_free(L.bin);
        if (L.host_total) (void)hipHostFree(L.host_total);
        if (L.ev_emit) (void)hipEventDestroy(L.ev_emit);
        if (L.ev_tail) (void)hipEventDestroy(L.ev_tail);
        if (L.s) (void)hipStreamDestroy(L.s);
    }
    for (auto e : c->ev0) if (e) (void)hipEventDestroy(e);
    for (auto e : c->ev1) if (e) (void)hipEventDestroy(e);
    if (c->ev_user) (void)hipEventDestroy(c->ev_user);
    if (c->ev_readback) (void)hipEventDestroy(c->ev_readback);
    delete c;
}

int gs4d_resize(gs4d_ctx* c, int width, int height) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    int rc = resolve_pending(c); if (rc) return rc;
    if (width == c->W && height == c->H) return GS4D_OK;
    return alloc_fbs(c, width, height);
}

// ---- buffers ----
int gs4d_buffer_create(gs4d_ctx* c, const void* data, size_t bytes, gs4d_buf* out) {
    if (!c || !out) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    gs4d_buf name = 0;
    for (size_t i = 1; i < c->bufs.size(); ++i) if (!c->bufs[i].alive && !c->bufs[i].d) { name = (gs4d_buf)i; break; }
    if (!name) { c->bufs.emplace_back(); name = (gs4d_buf)(c->bufs.size() - 1); }
    Buffer nb;
    if (bytes) {
        HIPCHK(c, hipMalloc(&nb.d, bytes));
        if (data) { hipError_t e = hipMemcpy(nb.d, data, bytes, hipMemcpyHostToDevice); if (e != hipSuccess) { (void)hipFree(nb.d); return hipfail(c, e, "buffer upload"); } }
    }
    nb.bytes = bytes; nb.alive = true; nb.version = 1;
    c->bufs[name] = nb;
    *out = name;
    return GS4D_OK;
}

int gs4d_buffer_subdata(gs4d_ctx* c, gs4d_buf b, size_t offset, const void* data, size_t bytes) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    Buffer* B = getbuf(c, b);
    if (!B) return fail(c, GS4D_E_INVALID, "buffer_subdata: bad buffer name");
    if (offset > B->bytes || bytes > B->bytes - offset) return fail(c, GS4D_E_INVALID, "buffer_subdata: range outside the buffer");   // GL_INVALID_VALUE
    if (!bytes) return GS4D_OK;
    if (!data) return fail(c, GS4D_E_INVALID, "buffer_subdata: data == NULL");
    { int rc = host_access(c, *B); if (rc) return rc; }
    // the caller keeps ownership of `data` and may reuse it on return (glBufferSubData semantics): copy synchronously
    HIPCHK(c, hipMemcpy((char*)B->d + offset, data, bytes, hipMemcpyHostToDevice));
    B->version++;
    return GS4D_OK;
}

int gs4d_buffer_read(gs4d_ctx* c, gs4d_buf b, size_t offset, void* out, size_t bytes) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    Buffer* B = getbuf(c, b);
    if (!B) return fail(c, GS4D_E_INVALID, "buffer_read: bad buffer name");
    if (offset > B->bytes || bytes > B->bytes - offset || (!out && bytes)) return fail(c, GS4D_E_INVALID, "buffer_read: range outside the buffer");
    if (!bytes) return GS4D_OK;
    // a buffer draws add record statistics to: after every draw issued so far, on every lane, re-runs included
    if (B->stats_target) { int rc = host_access(c, *B); if (rc) return rc; }
    // after the kernels that wrote it: they sit on the current lane, or on the lane recorded in the buffer
    HIPCHK(c, hipStreamSynchronize(lane(c).s));
    if (B->wr_lane >= 0 && B->wr_lane != c->cur) HIPCHK(c, hipStreamSynchronize(c->lanes[B->wr_lane].s));
    HIPCHK(c, hipMemcpy(out, (const char*)B->d + offset, bytes, hipMemcpyDeviceToHost));
    if (device_error(c)) return fail(c, GS4D_E_DEVICE, DEVICE_CHECK_MSG);
    return GS4D_OK;
}

int gs4d_buffer_destroy(gs4d_ctx* c, gs4d_buf b) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    Buffer* B = getbuf(c, b);
    if (!B) return GS4D_OK;                         // 0, unknown or already deleted: silently ignored, like glDeleteBuffers
    { int rc = resolve_pending(c); if (rc) return rc; rc = sync_all(c); if (rc) return rc; }
    if (B->d) (void)hipFree(B->d);
    if (B->soa) (void)hipFree(B->soa);
    if (B->bbox_dev) (void)hipFree(B->bbox_dev);
    if (B->ev_fill) (void)hipEventDestroy(B->ev_fill);
    if (B->ev_scan) (void)hipEventDestroy(B->ev_scan);
    *B = Buffer();
    for (auto& s : c->slots) if (s == b) s = 0;     // a deleted buffer is unbound
    if (c->depth_plane == b) c->depth_plane = 0;    // ... the depth-test plane too: the test is off
    if (c->record_stats == b) { c->record_stats = 0; c->record_stats_n = 0; }      // ... and the record statistics
    for (int i = 0; i < c->nlanes; ++i) if (c->lanes[i].kg_buf == b) c->lanes[i].kg_buf = 0;
    return GS4D_OK;
}

int gs4d_buffer_device_ptr(gs4d_ctx* c, gs4d_buf b, void** dptr, size_t* bytes) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    Buffer* B = getbuf(c, b);
    if (!B) return fail(c, GS4D_E_INVALID, "buffer_device_ptr: bad buffer name");
    if (dptr) *dptr = B->d;
    if (bytes) *bytes = B->bytes;
    B->ptr_exposed = true;                          // the address is the caller's to keep: this storage stays with this name
    B->version++;                                   // the caller may write through the pointer
    return GS4D_OK;
}

int gs4d_buffer_invalidate(gs4d_ctx* c, gs4d_buf b) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    Buffer* B = getbuf(c, b);
    if (!B) return fail(c, GS4D_E_INVALID, "buffer_invalidate: bad buffer name");
    int rc = resolve_pending(c); if (rc) return rc;           // a draw that has to be re-run reads the old contents: settle those first
    if (B->touch > c->synced) {
        if (c->user) {
            // the caller's stream waits for everything queued on the lanes so far (a superset of the kernels that use this buffer)
            for (int i = 0; i < c->nlanes; ++i) {
                HIPCHK(c, hipEventRecord(c->lanes[i].ev_tail, c->lanes[i].s));
                HIPCHK(c, hipStreamWaitEvent(c->user, c->lanes[i].ev_tail, 0));
            }
        } else { rc = sync_all(c); if (rc) return rc; }
    }
    B->version++;                                             // SoA shadow, key bounds, histogram hand-off and sort-index provenance all compare against it
    B->prov_valid = false;
    if (c->user) { B->fill_mask = (1u << c->nlanes) - 1u; B->fill_recorded = false; }      // whoever uses it next waits for the caller's stream
    return GS4D_OK;
}

int gs4d_bind_storage(gs4d_ctx* c, int slot, gs4d_buf b) {
    if (!c) return GS4D_E_INVALID;
    if (slot < 0 || slot >= 8) return fail(c, GS4D_E_INVALID, "bind_storage: slot out of range");
    if (b != 0 && !getbuf(c, b)) return fail(c, GS4D_E_INVALID, "bind_storage: bad buffer name");
    c->slots[slot] = b;
    return GS4D_OK;
}

// ---- state ----
int gs4d_set_mode(gs4d_ctx* c, int mode) {
    if (!c) return GS4D_E_INVALID;
    if (mode < GS4D_MODE_4D_SORTED || mode > GS4D_MODE_2D) return fail(c, GS4D_E_INVALID, "set_mode: unknown mode");
    c->mode = mode; return GS4D_OK;
}
int gs4d_set_uniform_1f(gs4d_ctx* c, int id, float v) {
    if (!c) return GS4D_E_INVALID;
    if (id == GS4D_U_TIME) c->u.time = v; else if (id == GS4D_U_MIN_OPACITY) c->u.min_opacity = v; else return fail(c, GS4D_E_INVALID, "set_uniform_1f: unknown uniform");
    return GS4D_OK;
}
int gs4d_set_uniform_mat4(gs4d_ctx* c, int id, const float m[16]) {
    if (!c || !m) return GS4D_E_INVALID;
    if (id == GS4D_U_VIEW) memcpy(c->u.view, m, 64); else if (id == GS4D_U_PROJ) memcpy(c->u.proj, m, 64); else return fail(c, GS4D_E_INVALID, "set_uniform_mat4: unknown uniform");
    return GS4D_OK;
}
int gs4d_set_clear_color(gs4d_ctx* c, const float rgba[4]) {
    if (!c || !rgba) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    memcpy(c->clear, rgba, 16);          // glClearColor does not touch pixels: an image that is (lazily) clear keeps the colour it was cleared with (Framebuffer::clear)
    return GS4D_OK;
}
int gs4d_set_blend(gs4d_ctx* c, int src, int dst) {
    if (!c) return GS4D_E_INVALID;
    auto known = [](int f) { return f == GS4D_ZERO || f == GS4D_ONE || (f >= GS4D_SRC_COLOR && f <= GS4D_ONE_MINUS_DST_COLOR) || (f >= GS4D_CONSTANT_COLOR && f <= GS4D_ONE_MINUS_CONSTANT_ALPHA); };
    if (!known(src) || !known(dst)) return fail(c, GS4D_E_INVALID, "set_blend: not a glBlendFunc factor of the reference's menu (GL_INVALID_ENUM)");
    c->blend_src = src; c->blend_dst = dst;              // like the GL's: state for the draws that follow
    return GS4D_OK;
}
int gs4d_set_depth_test(gs4d_ctx* c, gs4d_buf plane) {
    if (!c) return GS4D_E_INVALID;
    if (plane != 0 && !getbuf(c, plane)) return fail(c, GS4D_E_INVALID, "set_depth_test: bad buffer name");
    c->depth_plane = plane;                              // like glBlendFunc: state for the draws that follow (their size is checked when they are issued)
    return GS4D_OK;
}
int gs4d_set_record_stats(gs4d_ctx* c, gs4d_buf stats, size_t nrecords) {
    if (!c) return GS4D_E_INVALID;
    if (stats != 0) {
        const Buffer* S = getbuf(c, stats);
        if (!S) return fail(c, GS4D_E_INVALID, "set_record_stats: bad buffer name");
        if (S->bytes / sizeof(gs4d_record_stat) < nrecords) return fail(c, GS4D_E_INVALID, "set_record_stats: the buffer holds fewer than nrecords * 16 bytes");
    }
    c->record_stats = stats; c->record_stats_n = stats ? nrecords : 0;      // like gs4d_set_depth_test: state for the draws that follow
    return GS4D_OK;
}
int gs4d_clear(gs4d_ctx* c) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    int rc = next_frame_if_drawn(c); if (rc) return rc;
    // the new frame renders into the current lane's own framebuffer (a swap chain with one image per lane); the clear itself is
    // lazy: the compositing kernel starts from the clear colour instead of reading the pixels.  The image left behind stays intact
    // (and readable: gs4d_read_frame_*) until its lane comes round again.
    if (c->cur != c->cur_fb) c->prev_fb = c->cur_fb;
    else if (c->nlanes == 1) c->prev_fb = -1;
    c->cur_fb = c->cur;
    {
        Framebuffer& F = c->fbs[c->cur_fb];
        F.is_clear = true; F.all_in_memory = false;
        // the new epoch makes every tile clear — (D, O) = (0, 0), the ID sentinel — without touching the planes; ID outputs include aux outputs
        F.out = (c->ids_enable && F.ids && F.aux) ? Outputs::Ids : ((c->ids_enable || c->aux_enable) && F.aux) ? Outputs::Aux : Outputs::Colour;
        F.draws = 0;
        if (++F.epoch == 0u) {                              // the 32-bit epoch wraps: forget every old tile word (the lane that used the image last has long finished)
            HIPCHK(c, fb_access(c, F) == GS4D_OK ? hipMemsetAsync(F.tstate, 0, (size_t)c->tiles_x * c->tiles_y * 4, lane(c).s) : hipErrorUnknown);
            F.epoch = 1;
        }
    }
    memcpy(c->fbs[c->cur_fb].clear, c->clear, 16);
    // Whatever a still-unvalidated draw left in the image that is being cleared is discarded with it — the draw is never re-run — but its
    // verdict is still read (resolve_lane, at the latest when its lane draws again): what it found out about the scene's lists feeds the next
    // draw, and a draw that had aborted on the device is counted (gs4d_get_stats: a frame loop that never reads back can prove its frames complete).
    for (int i = 0; i < c->nlanes; ++i) if (c->lanes[i].pending && c->lanes[i].pending_args.fb == c->cur_fb) c->lanes[i].discarded = true;
    return GS4D_OK;
}

// ---- ordering ----
int gs4d_sort_pairs(gs4d_ctx* c, gs4d_buf keys, gs4d_buf vals, size_t n) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    if (n <= 1) return GS4D_OK;
    Buffer* K = getbuf(c, keys); Buffer* V = getbuf(c, vals);
    if (!K || !V) return fail(c, GS4D_E_INVALID, "sort_pairs: bad buffer name");
    if (K == V) return fail(c, GS4D_E_INVALID, "sort_pairs: keys and values must be different buffers");
    if (n >= 0xFFFFFFFFull || K->bytes < n * 4 || V->bytes < n * 4) return fail(c, GS4D_E_INVALID, "sort_pairs: buffers smaller than n elements");
    if (c->po.keygen && !c->po.sorted && keys == c->po.keys && vals == c->po.idx && n == c->po.n && c->cur == c->po.lane && !lane(c).drawn) {
        // the sort of a queued key generation's own output: queued with it; what the index will have been sorted by is known now
        Lane& Lq = lane(c);
        { int rc = lane_access(c, *K, true); if (rc) return rc; rc = lane_access(c, *V, true); if (rc) return rc; }
        c->po.sorted = true;
        c->stat_depth_passes = (uint64_t)sort_plan_passes(Lq.depth_sort.hist_bits, sort_plan_rb(Lq.depth_sort, n, Lq.depth_sort.hist_bits));
        K->version++; V->version++;
        V->sorted_by(true, Lq.keyed);                 // (n == po.n == keyed.n)
        return GS4D_OK;
    }
    { int rc = flush_order(c); if (rc) return rc; rc = next_frame_if_drawn(c); if (rc) return rc; }
    { int rc = lane_access(c, *K, true); if (rc) return rc; rc = lane_access(c, *V, true); if (rc) return rc; }
    Lane& L = lane(c);
    // k_keygen leaves the digit histograms of the keys it wrote: no histogram launch when this sort is of exactly those keys
    const bool have_hist = L.depth_sort.hist_pending && keys == L.kg_buf && K->version == L.kg_ver && n == L.keyed.n;
    const int key_bits = have_hist ? L.depth_sort.hist_bits : 32;
    c->stat_depth_passes = (uint64_t)sort_plan_passes(key_bits, have_hist ? L.depth_sort.hist_rb : sort_plan_rb(L.depth_sort, n, key_bits));
    // ... and when the payload is the identity index the same call wrote, the sorted payload is "the records in ascending (key, index)"
    const bool identity_payload = have_hist && vals == L.kg_idx && V->version == L.kg_idx_ver;
    StageTimer t(c, GS4D_T_SORT);
    HIPCHK(c, radix_sort_pairs(L.s, L.depth_sort, (uint32_t*)K->d, (uint32_t*)V->d, n, nullptr, key_bits, have_hist));
    K->version++; V->version++;
    V->sorted_by(identity_payload, L.keyed);          // (have_hist: n == keyed.n)
    return GS4D_OK;
}

int gs4d_keygen(gs4d_ctx* c, gs4d_buf data, float t, const float cam[3], gs4d_buf keys, gs4d_buf idx, size_t n, int key_mode) {
    if (!c || !cam) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    Buffer* D = getbuf(c, data); Buffer* K = getbuf(c, keys); Buffer* I = getbuf(c, idx);
    if (!D || !K || !I) return fail(c, GS4D_E_INVALID, "keygen: bad buffer name");
    if (key_mode != GS4D_KEY_REF_INV_EUCLID && key_mode != GS4D_KEY_VIEW_Z) return fail(c, GS4D_E_INVALID, "keygen: unknown key mode");
    if (n >= 0xFFFFFFFFull || D->bytes < n * 96 || K->bytes < n * 4 || I->bytes < n * 4) return fail(c, GS4D_E_INVALID, "keygen: buffers smaller than n elements");
    if (n == 0) return GS4D_OK;
    { int rc = flush_order(c); if (rc) return rc; rc = next_frame_if_drawn(c); if (rc) return rc; }
    int rc = ensure_soa(c, *D); if (rc) return rc;
    {
        // both outputs are overwritten entirely: if another lane's frame still uses their storage, take this lane's spare storage instead of waiting (Lane::spare)
        Lane& Lr = lane(c);
        auto busy_elsewhere = [&](const Buffer& B) { return (B.wr_lane >= 0 && B.wr_lane != c->cur) || ((B.rd_mask | B.tail_mask) & ~(1u << c->cur)) != 0u; };
        auto renamable = [&](const Buffer& B) { return !B.ptr_exposed && B.bytes == n * 4 && B.fill_mask == 0u && B.touch > c->synced; };
        if (c->rename_storage && c->nlanes > 1 && K != I && K != D && I != D && renamable(*K) && renamable(*I) && (busy_elsewhere(*K) || busy_elsewhere(*I))) {
            Buffer* out[2] = { K, I };
            bool ok = true;
            for (int k = 0; k < 2 && ok; ++k) {
                Lane::Spare& sp = Lr.spare[k];
                if (sp.d && sp.bytes != n * 4) {            // another size than last time: the old spare is given back once nothing can still use it
                    if (sp.touch > c->synced) { rc = sync_all(c); if (rc) return rc; }
                    (void)hipFree(sp.d);
                    sp.d = nullptr; sp.bytes = 0; sp.touch = 0; sp.wait_mask = 0u;      // the events stay with the spare (gs4d_destroy destroys them): resetting the whole struct leaked them
                }
                if (!sp.d) { if (hipMalloc(&sp.d, n * 4) != hipSuccess) { (void)hipGetLastError(); sp.d = nullptr; ok = false; } else sp.bytes = n * 4; }
            }
            if (ok) {
                for (int k = 0; k < 2; ++k) {
                    Buffer& B = *out[k]; Lane::Spare& sp = Lr.spare[k];
                    // the storage coming in: after what used it when it left its buffer (waits capture the events as recorded now)
                    for (int r = 0; r < c->nlanes; ++r) if (((sp.wait_mask >> r) & 1u) && r != c->cur) HIPCHK(c, hipStreamWaitEvent(Lr.s, sp.ev[r], 0));
                    // the storage going out: mark, on every other lane that uses it, the point up to which it does
                    unsigned users = B.rd_mask | B.tail_mask | (B.wr_lane >= 0 ? 1u << B.wr_lane : 0u);
                    users &= ~(1u << c->cur);                // this lane's own earlier uses are ordered by its stream
                    for (int r = 0; r < c->nlanes; ++r) if ((users >> r) & 1u) {
                        if (!sp.ev[r]) HIPCHK(c, hipEventCreateWithFlags(&sp.ev[r], hipEventDisableTiming));
                        HIPCHK(c, hipEventRecord(sp.ev[r], c->lanes[r].s));
                    }
                    sp.wait_mask = users;
                    std::swap(B.d, sp.d);
                    std::swap(B.touch, sp.touch);
                    B.wr_lane = -1; B.ordered_mask = 0; B.rd_mask = 0; B.tail_mask = 0;      // nothing but the waits above stands between this lane and the storage
                    B.touch = ++c->ops;                      // (kernels may still be running on it: a host access has to synchronise)
                }
                c->stat_renamed++;
            }
        }
    }
    { rc = lane_access(c, *D, false); if (rc) return rc; D->tail_mask |= 1u << c->cur; rc = lane_access(c, *K, true); if (rc) return rc; rc = lane_access(c, *I, true); if (rc) return rc; }
    Lane& L = lane(c);
    // A proven lower bound of every key (the key of the farthest point the records' bounding box allows) is subtracted inside the sort's
    // digit extraction: when the keys span less than 2^24 bit patterns above it (camera outside the cloud, far/near < 4) the top digit
    // becomes constant.  When the camera is provably outside the box the same reasoning gives an upper bound, hence the number of key bits
    // above the bias: with <= 24 the sort is launched with three passes instead of four.  The bounds are gs4d_host_key_bounds' (gs4d_host.cpp:
    // the kernel's own float32 operations on the ends of the box); k_keygen re-checks both for every key and raises the error word if one
    // does not hold.
    uint32_t bias = 0, span = 0xFFFFFFFFu;
    if (D->bb_ok) {                                                 // the box covers all records of the buffer, a superset of the n keyed
        float lo[7], hi[7];
        for (int k = 0; k < 7; ++k) { lo[k] = (float)D->bb_lo[k]; hi[k] = (float)D->bb_hi[k]; }      // (float values, kept as doubles)
        gs4d_host_key_bounds(lo, hi, t, cam, key_mode, &bias, &span);
    }
    // Not launched yet (see gs4d_ctx::po): everything the launch needs is recorded, everything a later call may ask about the buffers
    // (versions, what the index will have been sorted by) is settled now.
    BlendOrder bo;                                                  // the one place that builds an order from the call's arguments
    bo.ks.mode = key_mode == GS4D_KEY_REF_INV_EUCLID ? KEYSRC_REF : KEYSRC_VIEWZ;
    bo.ks.t = t; bo.ks.camx = cam[0]; bo.ks.camy = cam[1]; bo.ks.camz = cam[2];
    bo.ks.vr0 = c->u.view[2]; bo.ks.vr1 = c->u.view[6]; bo.ks.vr2 = c->u.view[10]; bo.ks.vr3 = c->u.view[14];
    bo.ks.bias = bias; bo.span = span; bo.bits = span_bits(span);
    c->po.keygen = true; c->po.sorted = false; c->po.lane = c->cur; c->po.data = data; c->po.keys = keys; c->po.idx = idx; c->po.n = n; c->po.order = bo;
    L.depth_sort.hist_bits = bo.bits;
    K->version++; I->version++;
    L.kg_buf = keys; L.kg_ver = K->version; L.kg_idx = idx; L.kg_idx_ver = I->version;
    L.keyed = SortedBy{ bo, data, D->version, n };
    if (!c->defer_order) return flush_order(c);
    return GS4D_OK;
}

// ---- compaction ----
int gs4d_compact_records(gs4d_ctx* c, gs4d_buf stats, size_t n, const gs4d_keep_rule* rule, gs4d_buf src, size_t stride, gs4d_buf dst, gs4d_buf kept_index, gs4d_buf count) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    if (!rule) return fail(c, GS4D_E_INVALID, "compact_records: rule == NULL");
    KeepRule k;
    if (!keep_rule_of(rule, k)) return fail(c, GS4D_E_INVALID, "compact_records: unknown flag or non-zero reserved field in the rule");
    return compact_by_table(c, "compact_records", "stats", true, stats, sizeof(gs4d_record_stat), n, src, stride, dst, kept_index, count,
        [&](Lane& L, const void* table, const void* records, void* out, uint32_t* index, uint32_t cap, gs4d_compact_count* cnt) {
            return launch_compact(L.s, (const gs4d_record_stat*)table, n, k, L.compact_counts, records, stride, out, index, cap, cnt);
        });
}

// ---- to a budget ----
int gs4d_stat_cut(gs4d_ctx* c, gs4d_buf stats, size_t n, int field, size_t budget, gs4d_buf out) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "stat_cut";
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 rows");
    if (budget == 0) return refuse(c, fn, "budget == 0");
    if (field != GS4D_STAT_PIXELS && field != GS4D_STAT_WMAX && field != GS4D_STAT_WSUM) return refuse(c, fn, "unknown field");
    Operands ops{ { "stats", stats, false, sizeof(gs4d_record_stat), n, OP_READ | OP_SETTLE | OP_SCAN },
                  { "out", out, false, 1, sizeof(gs4d_cut), OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    const uint32_t k = (uint32_t)std::min(budget, n);
    return queue_operands(c, ops,
        [&](Lane& L) {
            HIPCHK(c, grow_device_array(L.s, L.cut_scratch, L.cut_cap, cut_scratch_words(n)));
            return (int)GS4D_OK;
        },
        [&](Lane& L) {
            HIPCHK(c, launch_stat_cut(L.s, (const gs4d_record_stat*)ops.ptr(stats), n, field, k, L.cut_scratch, (gs4d_cut*)ops.ptr(out)));
            return (int)GS4D_OK;
        });
}

// ---- time windows ----
int gs4d_record_time_spans(gs4d_ctx* c, gs4d_buf data, size_t n, float min_opacity, gs4d_buf spans) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "record_time_spans";
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    Operands ops{ { "data", data, false, 96, n, OP_READ }, { "spans", spans, false, sizeof(gs4d_time_span), n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_time_spans(L.s, ops.ptr(data), n, min_opacity, (gs4d_time_span*)ops.ptr(spans)));
        return (int)GS4D_OK;
    });
}

int gs4d_compact_time_window(gs4d_ctx* c, gs4d_buf spans, size_t n, float t0, float t1, gs4d_buf src, size_t stride, gs4d_buf dst, gs4d_buf kept_index, gs4d_buf count) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    if (!(t0 <= t1)) return fail(c, GS4D_E_INVALID, "compact_time_window: t0 or t1 is NaN, or t0 > t1");
    const WindowRule k{ t0, t1 };
    return compact_by_table(c, "compact_time_window", "spans", false, spans, sizeof(gs4d_time_span), n, src, stride, dst, kept_index, count,
        [&](Lane& L, const void* table, const void* records, void* out, uint32_t* index, uint32_t cap, gs4d_compact_count* cnt) {
            return launch_compact(L.s, (const gs4d_time_span*)table, n, k, L.compact_counts, records, stride, out, index, cap, cnt);
        });
}

// ---- spatial order ----
int gs4d_spatial_order(gs4d_ctx* c, gs4d_buf src, size_t n, size_t stride, size_t pos_offset, gs4d_buf order_index) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "spatial_order";
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    if (n == 0xFFFFFFFFull) return refuse(c, fn, "the sort takes 2^32 - 2 records at most");
    if (!record_stride_ok(stride)) return refuse(c, fn, "stride must be a multiple of 16 from 16 to 1024");
    if (pos_offset % 4 != 0 || pos_offset + 12 > stride) return refuse(c, fn, "pos_offset must be a multiple of 4 with pos_offset + 12 <= stride");
    Operands ops{ { "src", src, false, stride, n, OP_READ }, { "order_index", order_index, false, 4, n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    const size_t box_words = order_box_words();
    return queue_operands(c, ops,
        [&](Lane& L) {
            HIPCHK(c, grow_device_array(L.s, L.spatial_scratch, L.spatial_cap, box_words + n));
            HIPCHK(c, sort_scratch_reserve(L.s, L.pair_sort, n));      // (the tile sort's scratch: a histogram a queued keygen has left in depth_sort stays where it is)
            return (int)GS4D_OK;
        },
        [&](Lane& L) {
            uint32_t* const keys = L.spatial_scratch + box_words;
            HIPCHK(c, launch_order_keys(L.s, ops.ptr(src), n, stride, pos_offset, (float*)L.spatial_scratch, keys));
            // the stable sort of the identity by key: the first pass that moves keys makes the indices up
            HIPCHK(c, radix_sort_pairs(L.s, L.pair_sort, keys, (uint32_t*)ops.ptr(order_index), n, nullptr, ORDER_KEY_BITS, false, true));
            return (int)GS4D_OK;
        });
}

int gs4d_gather_records(gs4d_ctx* c, gs4d_buf index, size_t m, gs4d_buf src, size_t nsrc, size_t stride, gs4d_buf dst) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "gather_records";
    if (m > 0xFFFFFFFFull || nsrc > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 entries or records");
    if (!record_stride_ok(stride) && stride != 4 && stride != 8) return refuse(c, fn, "stride must be a multiple of 16 from 16 to 1024, or 4 or 8");
    Operands ops{ { "index", index, false, 4, m, OP_READ }, { "src", src, false, stride, nsrc, OP_READ }, { "dst", dst, false, stride, m, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (m == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_gather_records(L.s, (const uint32_t*)ops.ptr(index), m, ops.ptr(src), nsrc, stride, ops.ptr(dst)));
        return (int)GS4D_OK;
    });
}

// ---- view-dependent colour ----
int gs4d_shade_sh(gs4d_ctx* c, gs4d_buf data, size_t n, gs4d_buf sh, size_t sh_stride, int degree, float t, const float cam_pos[3]) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "shade_sh";
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    if (degree < 0 || degree > 3) return refuse(c, fn, "degree must be 0, 1, 2 or 3");
    if (!record_stride_ok(sh_stride)) return refuse(c, fn, "sh_stride must be a multiple of 16 from 16 to 1024");
    if (sh_stride < 12u * (size_t)((degree + 1) * (degree + 1))) return refuse(c, fn, "sh_stride holds fewer than 12 (degree + 1)^2 bytes");
    if (!cam_pos) return refuse(c, fn, "cam_pos == NULL");
    Operands ops{ { "data", data, false, 96, n, OP_WRITE }, { "sh", sh, false, sh_stride, n, OP_READ } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    Buffer* const D = ops.buffer(data);
    // A colour-only write: the shadow's layout choice, the bounding box and the key bounds read no colour, so a shadow that is current stays current —
    // the kernel patches its colour plane (plane 1 in every layout: k_soa_repack) and soa_version moves on with version.  Decided once the pending
    // draws are settled (a re-run may rebuild the shadow) and before any buffer state is touched.
    bool patch = false;
    const float cam[3] = { cam_pos[0], cam_pos[1], cam_pos[2] };
    return queue_operands(c, ops,
        [&](Lane&) { patch = D->soa && D->soa_n == D->bytes / 96 && D->soa_version == D->version; return (int)GS4D_OK; },
        [&](Lane& L) {
            HIPCHK(c, launch_shade_sh(L.s, D->d, n, ops.ptr(sh), sh_stride, degree, t, cam, patch ? D->soa + D->soa_n : nullptr));
            if (patch) D->soa_version = D->version;
            return (int)GS4D_OK;
        });
}

// ---- time-varying view-dependent colour ----
int gs4d_shade_sh_t(gs4d_ctx* c, gs4d_buf data, size_t n, gs4d_buf sh, size_t sh_stride, const gs4d_sh_time* q) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "shade_sh_t";
    if (!q) return refuse(c, fn, "q == NULL");
    const gs4d_sh_time query = *q;
    if (const char* fault = gs4d_sht::query_fault(n, query.degree, query.degree_t, query.reserved, sh_stride)) return refuse(c, fn, fault);
    Operands ops{ { "data", data, false, 96, n, OP_WRITE }, { "sh", sh, false, sh_stride, n, OP_READ } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    Buffer* const D = ops.buffer(data);
    // the colour-only write of gs4d_shade_sh: the same decision, at the same point
    bool patch = false;
    return queue_operands(c, ops,
        [&](Lane&) { patch = D->soa && D->soa_n == D->bytes / 96 && D->soa_version == D->version; return (int)GS4D_OK; },
        [&](Lane& L) {
            HIPCHK(c, launch_shade_sh_t(L.s, D->d, n, ops.ptr(sh), sh_stride, query, patch ? D->soa + D->soa_n : nullptr));
            if (patch) D->soa_version = D->version;
            return (int)GS4D_OK;
        });
}

int gs4d_collapse_sh(gs4d_ctx* c, gs4d_buf data, size_t n, gs4d_buf sh, size_t sh_stride, const gs4d_sh_time* q, gs4d_buf dst, size_t dst_stride) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "collapse_sh";
    if (!q) return refuse(c, fn, "q == NULL");
    const gs4d_sh_time query = *q;
    if (const char* fault = gs4d_sht::query_fault(n, query.degree, query.degree_t, query.reserved, sh_stride)) return refuse(c, fn, fault);
    if (const char* fault = gs4d_sht::dst_stride_fault(query.degree, dst_stride)) return refuse(c, fn, fault);
    // tables are not record buffers, and data is a read operand: the ordering of gs4d_rotate_sh
    Operands ops{ { "data", data, false, 96, n, OP_READ }, { "sh", sh, false, sh_stride, n, OP_READ }, { "dst", dst, false, dst_stride, n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_collapse_sh(L.s, ops.ptr(data), n, ops.ptr(sh), sh_stride, query, ops.ptr(dst), dst_stride));
        return (int)GS4D_OK;
    });
}

// ---- colour edits by a selection ----
int gs4d_edit_colours(gs4d_ctx* c, gs4d_buf data, size_t n, const gs4d_colour_edit* edit, gs4d_buf stats, const gs4d_keep_rule* rule, gs4d_buf from) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "edit_colours";
    if (!edit) return refuse(c, fn, "edit == NULL");
    if (edit->op != GS4D_EDIT_SET && edit->op != GS4D_EDIT_MUL && edit->op != GS4D_EDIT_LERP && edit->op != GS4D_EDIT_COPY) return refuse(c, fn, "unknown op");
    if (edit->channels == 0u || edit->channels > 15u) return refuse(c, fn, "channels must be 1 .. 15");
    if (edit->reserved != 0u) return refuse(c, fn, "non-zero reserved field in the edit");
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    if ((stats != 0) != (rule != nullptr)) return refuse(c, fn, "stats and rule are given together or not at all");
    KeepRule k;
    if (!keep_rule_of(rule, k)) return refuse(c, fn, "unknown flag or non-zero reserved field in the rule");
    const bool copy = edit->op == GS4D_EDIT_COPY;
    if (copy && from == 0) return refuse(c, fn, "GS4D_EDIT_COPY needs from");
    if (!copy && from != 0) return refuse(c, fn, "from must be 0 unless the op is GS4D_EDIT_COPY");
    Operands ops{ { "data", data, false, 96, n, OP_WRITE },
                  { "stats", stats, true, sizeof(gs4d_record_stat), n, OP_READ | OP_SETTLE | OP_SCAN },
                  { "from", from, true, 96, n, OP_READ } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    const EditOp e{ edit->op, edit->channels, { edit->value[0], edit->value[1], edit->value[2], edit->value[3] }, edit->amount };
    Buffer* const D = ops.buffer(data);
    // A colour-only write, as gs4d_shade_sh's, extended to the alpha: nothing the library derives from a record buffer reads floats 4..7 (k_soa_repack
    // copies them to plane 1 whole; the bounding box and the key bounds read position, mu_t and sig[3].xyz, the layout choice sig and mu_t), so a shadow
    // that is current stays current — the kernel reads the old colour from its plane 1 and writes the new one there too.  Decided once the pending
    // draws are settled (a re-run may rebuild the shadow) and before any buffer state is touched.
    bool patch = false;
    return queue_operands(c, ops,
        [&](Lane&) { patch = D->soa && D->soa_n == D->bytes / 96 && D->soa_version == D->version; return (int)GS4D_OK; },
        [&](Lane& L) {
            HIPCHK(c, launch_edit_colours(L.s, D->d, n, e, (const gs4d_record_stat*)ops.ptr(stats), k, ops.ptr(from), patch ? D->soa + D->soa_n : nullptr));
            if (patch) D->soa_version = D->version;
            return (int)GS4D_OK;
        });
}

// ---- records from parameters ----
int gs4d_build_records(gs4d_ctx* c, const gs4d_splat_params* params, size_t n, gs4d_buf dst) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "build_records";
    if (!params) return refuse(c, fn, "params == NULL");
    const gs4d_splat_params& p = *params;
    if (p.form != GS4D_PARAMS_3D && p.form != GS4D_PARAMS_4D_VEL && p.form != GS4D_PARAMS_4D_2Q) return refuse(c, fn, "unknown form");
    if (p.flags != 0u || p.reserved != 0u) return refuse(c, fn, "flags and reserved must be 0");
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    // a parameter the form does not use is 0; every other one is required
    const bool vel = p.form == GS4D_PARAMS_4D_VEL, twoq = p.form == GS4D_PARAMS_4D_2Q;
    if (!twoq && p.rot_r != 0) return refuse(c, fn, "rot_r must be 0 in this form");
    if (!vel && p.dir != 0) return refuse(c, fn, "dir must be 0 in this form");
    if (!vel && p.tvar != 0) return refuse(c, fn, "tvar must be 0 in this form");
    Operands ops{ { "pos", p.pos, false, p.form == GS4D_PARAMS_3D ? 12u : 16u, n, OP_READ }, { "rot", p.rot, false, 16, n, OP_READ },
                  { "rot_r", p.rot_r, !twoq, 16, n, OP_READ }, { "scale", p.scale, false, twoq ? 16u : 12u, n, OP_READ },
                  { "rgba", p.rgba, false, 16, n, OP_READ }, { "dir", p.dir, !vel, 12, n, OP_READ }, { "tvar", p.tvar, !vel, 4, n, OP_READ },
                  { "dst", dst, false, 96, n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        const BuildParams bp = { ops.ptr(p.pos), ops.ptr(p.rot), ops.ptr(p.rot_r), ops.ptr(p.scale), ops.ptr(p.rgba), ops.ptr(p.dir), ops.ptr(p.tvar) };
        HIPCHK(c, launch_build_records(L.s, (int)p.form, bp, n, ops.ptr(dst)));
        return (int)GS4D_OK;
    });
}

// ---- records back to parameters ----
int gs4d_decompose_records(gs4d_ctx* c, gs4d_buf src, size_t n, size_t src_first, const gs4d_splat_params* out) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "decompose_records";
    if (!out) return refuse(c, fn, "out == NULL");
    const gs4d_splat_params& p = *out;
    if (p.form == GS4D_PARAMS_4D_2Q) return refuse(c, fn, "form GS4D_PARAMS_4D_2Q is not decomposed: take a 4D record out as GS4D_PARAMS_4D_VEL");
    if (p.form != GS4D_PARAMS_3D && p.form != GS4D_PARAMS_4D_VEL) return refuse(c, fn, "unknown form");
    if (p.flags != 0u || p.reserved != 0u) return refuse(c, fn, "flags and reserved must be 0");
    if (n > 0xFFFFFFFFull || src_first > 0xFFFFFFFFull || (uint64_t)n + src_first > 0xFFFFFFFFull) return refuse(c, fn, "n, src_first or src_first + n above 2^32 - 1");
    const bool vel = p.form == GS4D_PARAMS_4D_VEL;
    if (p.rot_r != 0) return refuse(c, fn, "rot_r must be 0");
    if (!vel && p.dir != 0) return refuse(c, fn, "dir must be 0 in this form");
    if (!vel && p.tvar != 0) return refuse(c, fn, "tvar must be 0 in this form");
    if (!(p.pos | p.rot | p.scale | p.rgba | p.dir | p.tvar)) return refuse(c, fn, "no destination given: at least one of pos, rot, scale, rgba, dir, tvar");
    // every destination is optional; src is read as records, never through its SoA shadow
    Operands ops{ { "src", src, false, 96, (uint64_t)src_first + n, OP_READ }, { "pos", p.pos, true, vel ? 16u : 12u, n, OP_WRITE },
                  { "rot", p.rot, true, 16, n, OP_WRITE }, { "scale", p.scale, true, 12, n, OP_WRITE }, { "rgba", p.rgba, true, 16, n, OP_WRITE },
                  { "dir", p.dir, true, 12, n, OP_WRITE }, { "tvar", p.tvar, true, 4, n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        const DecomposeOut o = { ops.ptr(p.pos), ops.ptr(p.rot), ops.ptr(p.scale), ops.ptr(p.rgba), ops.ptr(p.dir), ops.ptr(p.tvar) };
        HIPCHK(c, launch_decompose_records(L.s, (int)p.form, (const char*)ops.ptr(src) + src_first * 96, n, o));
        return (int)GS4D_OK;
    });
}

// ---- records under affine maps ----
int gs4d_transform_records(gs4d_ctx* c, gs4d_buf src, size_t n, gs4d_buf xf, size_t m, gs4d_buf dst, size_t dst_first) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "transform_records";
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull || dst_first > 0xFFFFFFFFull) return refuse(c, fn, "n, m or dst_first above 2^32 - 1");
    const uint64_t total = (uint64_t)n * m;                    // (both below 2^32: no overflow)
    if (total > 0xFFFFFFFFull || dst_first + total > 0xFFFFFFFFull) return refuse(c, fn, "dst_first + m * n above 2^32 - 1");
    Operands ops{ { "src", src, false, 96, n, OP_READ }, { "xf", xf, false, sizeof(gs4d_affine4), m, OP_READ }, { "dst", dst, false, 96, dst_first + total, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0 || m == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_transform_records(L.s, ops.ptr(src), n, (const gs4d_affine4*)ops.ptr(xf), m, (char*)ops.ptr(dst) + dst_first * 96));
        return (int)GS4D_OK;
    });
}

// ---- one affine map per record, indexed or blended ----
int gs4d_pose_records(gs4d_ctx* c, gs4d_buf src, size_t n, gs4d_buf xf, size_t m, gs4d_buf bind, uint32_t form, size_t bind_stride, gs4d_buf dst, size_t dst_first) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "pose_records";
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull || dst_first > 0xFFFFFFFFull || (uint64_t)n + dst_first > 0xFFFFFFFFull) return refuse(c, fn, "n, m, dst_first or dst_first + n above 2^32 - 1");
    if (form != GS4D_POSE_INDEX && form != GS4D_POSE_BLEND4) return refuse(c, fn, "form is neither GS4D_POSE_INDEX nor GS4D_POSE_BLEND4");
    if (form == GS4D_POSE_INDEX ? (bind_stride < 4 || bind_stride % 4 != 0) : (bind_stride < 32 || bind_stride % 16 != 0))
        return refuse(c, fn, form == GS4D_POSE_INDEX ? "bind_stride must be a multiple of 4, at least 4" : "bind_stride must be a multiple of 16, at least 32");
    Operands ops{ { "src", src, false, 96, n, OP_READ }, { "xf", xf, false, sizeof(gs4d_affine4), m, OP_READ }, { "bind", bind, false, bind_stride, n, OP_READ },
                  { "dst", dst, false, 96, (uint64_t)dst_first + n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_pose_records(L.s, ops.ptr(src), n, (const gs4d_affine4*)ops.ptr(xf), m, ops.ptr(bind), form, bind_stride, (char*)ops.ptr(dst) + dst_first * 96));
        return (int)GS4D_OK;
    });
}

// ---- an SH table turned with the maps that move its records ----
int gs4d_rotate_sh(gs4d_ctx* c, gs4d_buf src, size_t n, size_t stride, int degree, gs4d_buf xf, size_t m, gs4d_buf bind, uint32_t form, size_t bind_stride, gs4d_buf dst,
                   size_t dst_first) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "rotate_sh";
    static_assert(SHROT_INDEX == GS4D_POSE_INDEX && SHROT_BLEND4 == GS4D_POSE_BLEND4 && SHROT_EACH == GS4D_SH_EACH && sizeof(gs4d_affine4) == 80, "the forms and rows of sh_rotate_operands.h");
    if (const char* fault = rotate_sh_fault(n, stride, degree, m, bind != 0, form, bind_stride, dst_first)) return refuse(c, fn, fault);
    Operand list[ROTATE_SH_OPERANDS];                          // (sh_rotate_operands.h: what the call does with each)
    rotate_sh_operands(list, src, n, stride, xf, m, bind, form, bind_stride, dst, dst_first);
    Operands ops{ list[0], list[1], list[2], list[3] };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0 || (form == GS4D_SH_EACH && m == 0)) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_rotate_sh(L.s, ops.ptr(src), n, stride, degree, (const gs4d_affine4*)ops.ptr(xf), m, bind ? ops.ptr(bind) : nullptr, form, bind_stride,
                                   (char*)ops.ptr(dst) + dst_first * stride));
        return (int)GS4D_OK;
    });
}

// ---- a set deformed through a 4D lattice ----
int gs4d_warp_records(gs4d_ctx* c, gs4d_buf src, size_t n, gs4d_buf nodes, const gs4d_lattice* lat, gs4d_buf dst, size_t dst_first) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "warp_records";
    if (!lat) return refuse(c, fn, "lat == NULL");
    const gs4d_lattice q = *lat;
    const uint64_t count = gs4d_warp::node_count(q.dims, q.clamp, q.pad);
    if (!count) return refuse(c, fn, "a dim that is 0 or above 65535, more than 2^28 nodes, clamp bits above 3 or a non-zero pad");
    if (n > 0xFFFFFFFFull || dst_first > 0xFFFFFFFFull || (uint64_t)n + dst_first > 0xFFFFFFFFull) return refuse(c, fn, "n, dst_first or dst_first + n above 2^32 - 1");
    Operands ops{ { "src", src, false, 96, n, OP_READ }, { "nodes", nodes, false, 16, count, OP_READ }, { "dst", dst, false, 96, (uint64_t)dst_first + n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_warp_records(L.s, ops.ptr(src), n, ops.ptr(nodes), (uint32_t)count, q, (char*)ops.ptr(dst) + dst_first * 96));
        return (int)GS4D_OK;
    });
}

// ---- a 4D set baked at one time ----
int gs4d_slice_records(gs4d_ctx* c, gs4d_buf src, size_t n, const gs4d_slice* q, gs4d_buf dst, size_t dst_first) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "slice_records";
    if (!q) return refuse(c, fn, "q == NULL");
    const gs4d_slice s = *q;
    if (!std::isfinite(s.t) || !std::isfinite(s.mu_t_out)) return refuse(c, fn, "t and mu_t_out must be finite");
    if (std::isnan(s.min_opacity)) return refuse(c, fn, "min_opacity is a NaN");
    if (!(s.s44_out > 0.0f)) return refuse(c, fn, "s44_out must be above 0");
    if (n > 0xFFFFFFFFull || dst_first > 0xFFFFFFFFull || (uint64_t)n + dst_first > 0xFFFFFFFFull) return refuse(c, fn, "n, dst_first or dst_first + n above 2^32 - 1");
    Operands ops{ { "src", src, false, 96, n, OP_READ }, { "dst", dst, false, 96, (uint64_t)dst_first + n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_slice_records(L.s, ops.ptr(src), n, s, (char*)ops.ptr(dst) + dst_first * 96));
        return (int)GS4D_OK;
    });
}

// ---- a selection under an affine map about a pivot, in place ----
int gs4d_transform_selected(gs4d_ctx* c, gs4d_buf data, size_t n, const gs4d_selection_xf* xf, gs4d_buf stats, const gs4d_keep_rule* rule, gs4d_buf measure) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "transform_selected";
    if (!xf) return refuse(c, fn, "xf == NULL");
    const gs4d_selection_xf x = *xf;
    if (x.flags != 0u && x.flags != (uint32_t)GS4D_XS_PIVOT && x.flags != (uint32_t)GS4D_XS_PIVOT_MEASURE) return refuse(c, fn, "flags must be 0, GS4D_XS_PIVOT or GS4D_XS_PIVOT_MEASURE");
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    if ((stats != 0) != (rule != nullptr)) return refuse(c, fn, "stats and rule are given together or not at all");
    KeepRule k;
    if (!keep_rule_of(rule, k)) return refuse(c, fn, "unknown flag or non-zero reserved field in the rule");
    const bool measured = x.flags == (uint32_t)GS4D_XS_PIVOT_MEASURE;
    if (measured && measure == 0) return refuse(c, fn, "GS4D_XS_PIVOT_MEASURE needs measure");
    if (!measured && measure != 0) return refuse(c, fn, "measure must be 0 unless the flag is GS4D_XS_PIVOT_MEASURE");
    // The table and the measurement are read (gs4d_edit_colours' table; an ordinary read buffer, behind the kernels that wrote it), data is written as
    // gs4d_transform_records writes its dst: a full write whatever the table selects — position, mu_t and sig move, so the shadow, the bounding box
    // and the key bounds of data are all stale.  The shadow is not patched: the next draw or gs4d_keygen rebuilds it.
    Operands ops{ { "data", data, false, 96, n, OP_WRITE },
                  { "stats", stats, true, sizeof(gs4d_record_stat), n, OP_READ | OP_SETTLE | OP_SCAN },
                  { "measure", measure, true, 1, sizeof(gs4d_measure), OP_READ } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_transform_selected(L.s, ops.ptr(data), n, x, (const gs4d_record_stat*)ops.ptr(stats), k, (const gs4d_measure*)ops.ptr(measure)));
        return (int)GS4D_OK;
    });
}

// ---- draw ----
static int draw_common(gs4d_ctx* c, DrawArgs& a) {
    (void)hipSetDevice(c->device);
    if (a.quads || a.mode == GS4D_MODE_4D_SORTED || a.mode == GS4D_MODE_4D_DIRECT) {
        // The quad set-up takes uProj * vec4(offset, 0, 1) + ps as "centre + (P00 * x, P11 * y)" at w = 1, which is what the shader computes
        // for a matrix with glm::perspective's sparsity (Camera.cpp:55-58) — the only kind the reference produces.  Anything else is refused
        // rather than drawn differently.
        const float* P = a.u.proj;
        const bool ok = P[1] == 0.0f && P[2] == 0.0f && P[3] == 0.0f && P[4] == 0.0f && P[6] == 0.0f && P[7] == 0.0f && P[8] == 0.0f && P[9] == 0.0f
                     && P[12] == 0.0f && P[13] == 0.0f && P[15] == 0.0f && P[11] != 0.0f && P[0] != 0.0f && P[5] != 0.0f;
        if (!ok) return fail(c, GS4D_E_UNSUPPORTED, "draw: uProj must have the sparsity of glm::perspective (P00, P11, P22, P23, P32 only)");
    }
    // aux and ID outputs are the transmittance form of the default blend function: any other function has none (nothing is drawn)
    if (c->fbs[c->cur_fb].out != Outputs::Colour && !(c->blend_src == GS4D_SRC_ALPHA && c->blend_dst == GS4D_ONE_MINUS_SRC_ALPHA))
        return fail(c, GS4D_E_UNSUPPORTED, has_ids(c->fbs[c->cur_fb].out) ? "draw: ID outputs are defined for the default blend function (SRC_ALPHA, ONE_MINUS_SRC_ALPHA) only"
                                                                    : "draw: aux outputs are defined for the default blend function (SRC_ALPHA, ONE_MINUS_SRC_ALPHA) only");
    // so is the depth test, against a plane of at least W x H floats (a resize can leave it too small)
    if (c->depth_plane) {
        const Buffer* Z = getbuf(c, c->depth_plane);
        if (!Z || Z->bytes < (size_t)c->W * c->H * 4) return fail(c, GS4D_E_INVALID, "draw: the depth-test plane holds fewer than width*height floats");
        if (!(c->blend_src == GS4D_SRC_ALPHA && c->blend_dst == GS4D_ONE_MINUS_SRC_ALPHA))
            return fail(c, GS4D_E_UNSUPPORTED, "draw: the depth test is defined for the default blend function (SRC_ALPHA, ONE_MINUS_SRC_ALPHA) only");
    }
    // record statistics: built for the default blend function into a colour-only frame without a depth test
    if (c->record_stats) {
        if (!getbuf(c, c->record_stats)) return fail(c, GS4D_E_INVALID, "draw: the record-statistics buffer has been deleted");
        if (!(c->blend_src == GS4D_SRC_ALPHA && c->blend_dst == GS4D_ONE_MINUS_SRC_ALPHA))
            return fail(c, GS4D_E_UNSUPPORTED, "draw: record statistics are built for the default blend function (SRC_ALPHA, ONE_MINUS_SRC_ALPHA) only");
        if (c->fbs[c->cur_fb].out != Outputs::Colour) return fail(c, GS4D_E_UNSUPPORTED, "draw: record statistics are not built for frames with aux or ID outputs");
        if (c->depth_plane) return fail(c, GS4D_E_UNSUPPORTED, "draw: record statistics are not built for draws with a depth test");
    }
    // the lane's scratch still belongs to its previous draw, and the image this draw blends onto must be complete: validate those
    // (not the other lanes' draws: their frames are still in flight and nothing here depends on them)
    int rc = resolve_lane(c, c->cur); if (rc) return rc;
    rc = resolve_image(c, c->cur_fb); if (rc) return rc;
    Lane& L = lane(c);
    a.lane = c->cur; a.fb = c->cur_fb;
    memcpy(a.clear, c->fbs[c->cur_fb].clear, 16);
    a.shard_rank = c->shard_rank; a.shard_world = c->shard_world;
    // Which path: the unordered one whenever the blend order is known without reading a sort index — instance k draws record k, or the
    // bound index is this library's sort of its own depth keys for exactly these records — and the lists are short enough to be
    // ordered in LDS (validated on the device; a draw that turns out otherwise is re-run on the ordered path).
    a.v2 = false;
    a.blend_src = c->blend_src; a.blend_dst = c->blend_dst;
    const bool over = a.blend_src == GS4D_SRC_ALPHA && a.blend_dst == GS4D_ONE_MINUS_SRC_ALPHA;       // any other function is applied in draw order: instance-ordered lists
    a.out = c->fbs[c->cur_fb].out; a.draw_ord = c->fbs[c->cur_fb].draws; a.zplane = c->depth_plane;
    a.stats = c->record_stats; a.stats_n = c->record_stats_n;
    a.lean = over && c->splat_draws > 0;
    if (c->atomic_rank && c->path_pref != 1 && over) {
        Buffer* data = getbuf(c, a.data);
        bool ok = false;
        size_t nkeys = 0;
        if (data && (a.quads || a.mode == GS4D_MODE_4D_DIRECT || a.mode == GS4D_MODE_2D)) {
            nkeys = std::min(a.instances, data->bytes / (a.quads ? 288 : a.mode == GS4D_MODE_2D ? 48 : 96));
            int keybits = 1; while (keybits < 32 && ((size_t)1 << keybits) < nkeys) ++keybits;
            a.blend_order = BlendOrder{ KeySrc(), keybits, nkeys ? (uint32_t)(nkeys - 1) : 0u };      // KEYSRC_INDEX: key = instance
            ok = nkeys > 0;
        } else if (data && a.mode == GS4D_MODE_4D_SORTED) {
            const Buffer* ob = getbuf(c, a.order);
            if (ob && ob->prov_valid && ob->version == ob->prov_ver && a.data == ob->prov.data && data->version == ob->prov.data_ver && a.instances == ob->prov.n && data->bytes / 96 == ob->prov.n) {
                a.blend_order = ob->prov.order; ok = true;
            }
        }
        if (ok && (nkeys > V2_MAX_RECORDS || (a.mode == GS4D_MODE_4D_SORTED && a.instances > V2_MAX_RECORDS) || (size_t)c->tiles_x * c->tiles_y > 256u * 1024u)) ok = false;   // tilelist.hip's entry format
        if (ok && c->long_lists) {
            // the lists were too long last time: stay on the ordered path, but probe again now and then if they look short on average
            const uint64_t tiles = (uint64_t)c->tiles_x * c->tiles_y;
            if (++c->ordered_draws >= 64 && c->stat_entries / (tiles ? tiles : 1) <= V2_MAX_LIST / 8) c->long_lists = false; else ok = false;
        }
        a.v2 = ok;
    }
    a.fuse = false;
    if (c->po.keygen) {
        // a queued key generation + sort: executed by this draw if it is the draw they were made for (it takes its blend order from exactly
        // that sort, on the same lane, and the unordered path can run), else launched on their own first
        const Buffer* pd = getbuf(c, a.data);
        bool mine = a.mode == GS4D_MODE_4D_SORTED && !a.quads && c->po.sorted && c->po.idx == a.order && c->po.data == a.data && c->po.lane == c->cur
                 && pd && a.instances == c->po.n && pd->bytes / 96 == c->po.n;
        if (mine && a.v2 && !tile_lists_plan(lane(c).tl, (size_t)c->tiles_x * c->tiles_y, a.instances, c->slabs, a.blend_order.bits, a.blend_order.span)) a.v2 = false;
        if (mine) {
            // on the ordered path too: the projection writes the keys, the sort follows it, the binning reads the sorted index
            if (!a.v2) a.blend_order = lane(c).keyed.order;      // (a.v2: the same record, through the index's provenance)
            a.fuse = true; a.fuse_keys = c->po.keys; a.fuse_idx = c->po.idx; c->po.keygen = c->po.sorted = false; c->stat_fused++;
        }
        else { int rc2 = flush_order(c); if (rc2) return rc2; }
    }
    const size_t before = L.proj_n;
    L.proj_n = 0;
    rc = run_draw(c, a, true);
    a.fuse = false;                    // a re-run of this draw finds the keys written and the sort queued
    if (rc) { L.proj_n = before; return rc; }
    c->fbs[a.fb].draws++;                                   // the next splat draw into this frame has the next ordinal
    c->splat_draws++;
    if (L.proj_n) { L.pending = true; L.pending_args = a; c->fbs[c->cur_fb].is_clear = false; L.drawn = true; if (a.v2) c->stat_v2_draws++; }   // proj_n != 0 <=> raster work was enqueued
    else L.proj_n = before;
    if (c->profiling) { if (c->prof_frame < gs4d_ctx::PROF_FRAMES && c->prof_tick % (uint64_t)c->prof_every == 0) c->prof_frame++; c->prof_tick++; }
    return GS4D_OK;
}

int gs4d_draw_instanced(gs4d_ctx* c, size_t instances) {
    if (!c) return GS4D_E_INVALID;
    DrawArgs a; a.mode = c->mode; a.u = c->u; a.instances = instances; a.quads = false;
    if (c->mode == GS4D_MODE_4D_SORTED) { a.data = c->slots[2]; a.order = c->slots[1]; }
    else if (c->mode == GS4D_MODE_4D_DIRECT || c->mode == GS4D_MODE_2D) { a.data = c->slots[1]; a.order = 0; }
    else return fail(c, GS4D_E_INVALID, "draw_instanced: GS4D_MODE_3D_FULL draws with gs4d_draw_quads");
    return draw_common(c, a);
}

int gs4d_draw_quads(gs4d_ctx* c, gs4d_buf vertices, size_t nquads) {
    if (!c) return GS4D_E_INVALID;
    if (c->mode != GS4D_MODE_3D_FULL) return fail(c, GS4D_E_INVALID, "draw_quads: mode must be GS4D_MODE_3D_FULL");
    DrawArgs a; a.mode = c->mode; a.u = c->u; a.instances = nquads; a.quads = true; a.data = vertices; a.order = 0;
    return draw_common(c, a);
}

// ---- overlay lines (Renderer.cpp:41-215) ----
int gs4d_draw_lines(gs4d_ctx* c, const float* verts, size_t nverts, int dims, int strip, const float viewproj[16], const float rgba[4], float width) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    if (dims != 2 && dims != 3) return fail(c, GS4D_E_INVALID, "draw_lines: dims must be 2 (NDC positions) or 3 (positions transformed by viewproj)");
    if (!rgba || (dims == 3 && !viewproj) || (nverts && !verts)) return fail(c, GS4D_E_INVALID, "draw_lines: NULL argument");
    if (nverts < 2) return GS4D_OK;
    if (nverts > 0x7FFFFFFFull) return fail(c, GS4D_E_UNSUPPORTED, "draw_lines: too many vertices");
    // lines blend into the image in call order: a splat draw into it that still awaits validation (and may be re-run) goes first
    int rc = resolve_image(c, c->cur_fb); if (rc) return rc;
    rc = materialise_fb(c); if (rc) return rc;
    Framebuffer& F = c->fbs[c->cur_fb];
    rc = fb_access(c, F); if (rc) return rc;
    Lane& L = lane(c);
    if (!F.linecnt) {
        HIPCHK(c, hipMalloc(&F.linecnt, (size_t)c->W * c->H * 4));
        HIPCHK(c, hipMemsetAsync(F.linecnt, 0, (size_t)c->W * c->H * 4, L.s));
    }
    const size_t floats = nverts * (size_t)dims;
    if (L.line_cap < floats) HIPCHK(c, grow_device_array(L.s, L.line_verts, L.line_cap, std::max<size_t>(floats, 4096)));
    HIPCHK(c, hipMemcpyAsync(L.line_verts, verts, floats * 4, hipMemcpyHostToDevice, L.s));     // the caller's array is reusable on return (pageable source)
    LineParams p;
    for (int i = 0; i < 16; ++i) p.vp[i] = viewproj ? viewproj[i] : (i % 5 == 0 ? 1.0f : 0.0f);
    for (int i = 0; i < 4; ++i) p.rgba[i] = std::min(std::max(rgba[i], 0.0f), 1.0f);      // the GL clamps fragment colours before blending into a fixed-point framebuffer
    p.W = c->W; p.H = c->H; p.blend_src = c->blend_src; p.blend_dst = c->blend_dst;
    HIPCHK(c, launch_lines(L.s, L.line_verts, nverts, dims, strip ? 1 : 0, p, width, F.linecnt, F.mem));
    ++c->ops;
    return GS4D_OK;
}

// ---- read-back ----
int gs4d_finish(gs4d_ctx* c) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    int rc = resolve_pending(c); if (rc) return rc;
    rc = sync_all(c); if (rc) return rc;
    if (device_error(c)) return fail(c, GS4D_E_DEVICE, DEVICE_CHECK_MSG);
    return GS4D_OK;
}

// What every gs4d_read_* checks first, in this order (after its own null check): the queued order, the size, the frame's outputs.
static int read_begin(gs4d_ctx* c, bool size_ok, const char* size_msg, Outputs need = Outputs::Colour, const char* need_msg = nullptr) {
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    if (!size_ok) return fail(c, GS4D_E_INVALID, size_msg);
    if (c->fbs[c->cur_fb].out < need) return fail(c, GS4D_E_INVALID, need_msg);
    return GS4D_OK;
}

// A read of the current image into host memory: every tile in memory, copy(F, stream) queued on the current lane, and waited for.
static int read_host(gs4d_ctx* c, const std::function<hipError_t(Framebuffer&, hipStream_t)>& copy) {
    int rc = resolve_image(c, c->cur_fb); if (rc) return rc;
    rc = materialise_fb(c); if (rc) return rc;
    Framebuffer& F = c->fbs[c->cur_fb];
    rc = fb_access(c, F); if (rc) return rc;
    HIPCHK(c, copy(F, lane(c).s));
    HIPCHK(c, hipStreamSynchronize(lane(c).s));
    if (device_error(c)) return fail(c, GS4D_E_DEVICE, DEVICE_CHECK_MSG);
    return GS4D_OK;
}

int gs4d_read_pixels(gs4d_ctx* c, float* rgba, size_t bytes) {
    if (!c || !rgba) return GS4D_E_INVALID;
    int rc = read_begin(c, bytes == (size_t)c->W * c->H * 16, "read_pixels: bytes != width*height*16"); if (rc) return rc;
    return read_host(c, [&](Framebuffer& F, hipStream_t st) { return hipMemcpyAsync(rgba, F.mem, bytes, hipMemcpyDeviceToHost, st); });
}

// What a device read copies out of an image: its colour as floats or packed to RGBA8, its aux plane (W * H float2), or its ID planes
// (W * H u32 each, into the non-null ones of dst[0..2] = record, draw, weight).  Aux and Ids: frames_back 0 only.
enum class ReadPlane { ColourF32, ColourRGBA8, Aux, Ids };
// frames_back 0: the image the last clear / draw used.  1: the image the last gs4d_clear moved away from (the previous frame of the
// swap chain) — it is packed on the lane that rendered it, behind its compositing kernel, so an application that reads frame f-1
// after queueing frame f never waits for frame f.
static int read_device_common(gs4d_ctx* c, int frames_back, ReadPlane what, void* const* dst, bool named_event = false, hipEvent_t after = nullptr) {
    if (frames_back != 0 && frames_back != 1) return fail(c, GS4D_E_INVALID, "read_frame: frames_back must be 0 or 1");
    const int fi = frames_back == 0 ? c->cur_fb : c->prev_fb;
    if (fi < 0) return fail(c, GS4D_E_INVALID, "read_frame: no previous image is retained (one frame lane, or no gs4d_clear yet)");
    int rc = resolve_image(c, fi); if (rc) return rc;
    Framebuffer& F = c->fbs[fi];
    const int li = (fi == c->cur_fb || F.last_lane < 0) ? c->cur : F.last_lane;
    Lane& L = c->lanes[li];
    if (named_event) { if (after) HIPCHK(c, hipStreamWaitEvent(L.s, after, 0)); }      // the caller says exactly what the destination has to wait for
    else if (c->user) {                                     // the destination may still be in use by the caller's earlier work
        HIPCHK(c, hipEventRecord(c->ev_user, c->user));
        HIPCHK(c, hipStreamWaitEvent(L.s, c->ev_user, 0));
    }
    if (li == c->cur) { rc = fb_access(c, F); if (rc) return rc; }
    const size_t npix = (size_t)c->W * c->H;
    if (what == ReadPlane::ColourRGBA8) HIPCHK(c, launch_pack_rgba8(L.s, F.mem, F.tstate, F.epoch, F.clear, c->W, c->H, c->tiles_x, (uint32_t*)dst[0]));      // lazily clear tiles are packed as the clear colour
    else {
        rc = materialise_fb(c, F, L); if (rc) return rc;
        if (what == ReadPlane::Ids) { for (int k = 0; k < 3; ++k) if (dst[k]) HIPCHK(c, hipMemcpyAsync(dst[k], F.ids + (size_t)k * npix, npix * 4, hipMemcpyDeviceToDevice, L.s)); }
        else if (what == ReadPlane::Aux) HIPCHK(c, hipMemcpyAsync(dst[0], F.aux, npix * 8, hipMemcpyDeviceToDevice, L.s));
        else HIPCHK(c, hipMemcpyAsync(dst[0], F.mem, npix * 16, hipMemcpyDeviceToDevice, L.s));
    }
    if (li != c->cur) HIPCHK(c, hipEventRecord(L.ev_tail, L.s));      // the lane's tail event keeps covering everything queued on it
    if (c->user) {                                          // work the caller queues on its stream after this call sees the pixels
        HIPCHK(c, hipEventRecord(c->ev_readback, L.s));
        HIPCHK(c, hipStreamWaitEvent(c->user, c->ev_readback, 0));
    }
    return GS4D_OK;
}

int gs4d_read_pixels_device(gs4d_ctx* c, void* dptr, size_t bytes) {
    if (!c || !dptr) return GS4D_E_INVALID;
    int rc = read_begin(c, bytes == (size_t)c->W * c->H * 16, "read_pixels_device: bytes != width*height*16"); if (rc) return rc;
    return read_device_common(c, 0, ReadPlane::ColourF32, &dptr);
}

// ---- aux and ID outputs ----
// the user's two switches; the planes are made the first time a level is asked for (nothing running reads or writes them yet: no frame
// has been cleared with it on), and the switch takes effect at the next gs4d_clear
static int set_outputs(gs4d_ctx* c, bool& enable_flag, int enable, Outputs level) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    if (enable && c->planes < level) {
        for (int i = 0; i < c->nlanes; ++i) HIPCHK(c, c->fbs[i].reserve_planes(level, c->W, c->H));
        c->planes = level;
    }
    enable_flag = enable != 0;
    return GS4D_OK;
}
int gs4d_set_aux_outputs(gs4d_ctx* c, int enable) { return c ? set_outputs(c, c->aux_enable, enable, Outputs::Aux) : GS4D_E_INVALID; }
int gs4d_set_id_outputs(gs4d_ctx* c, int enable) { return c ? set_outputs(c, c->ids_enable, enable, Outputs::Ids) : GS4D_E_INVALID; }

int gs4d_read_aux(gs4d_ctx* c, float* depth_opacity, size_t bytes) {
    if (!c || !depth_opacity) return GS4D_E_INVALID;
    int rc = read_begin(c, bytes == (size_t)c->W * c->H * 8, "read_aux: bytes != width*height*8", Outputs::Aux, "read_aux: the current frame was not cleared with aux outputs on"); if (rc) return rc;
    return read_host(c, [&](Framebuffer& F, hipStream_t st) { return hipMemcpyAsync(depth_opacity, F.aux, bytes, hipMemcpyDeviceToHost, st); });
}

int gs4d_read_aux_device(gs4d_ctx* c, void* dptr, size_t bytes) {
    if (!c || !dptr) return GS4D_E_INVALID;
    int rc = read_begin(c, bytes == (size_t)c->W * c->H * 8, "read_aux_device: bytes != width*height*8", Outputs::Aux, "read_aux_device: the current frame was not cleared with aux outputs on"); if (rc) return rc;
    return read_device_common(c, 0, ReadPlane::Aux, &dptr);
}

int gs4d_read_ids(gs4d_ctx* c, int x, int y, int w, int h, uint32_t* record, uint32_t* draw, float* weight) {
    if (!c) return GS4D_E_INVALID;
    int rc = read_begin(c, !(x < 0 || y < 0 || w <= 0 || h <= 0 || w > c->W - x || h > c->H - y), "read_ids: the rectangle is not inside the image", Outputs::Ids,
                        "read_ids: the current frame was not cleared with ID outputs on"); if (rc) return rc;
    void* const dst[3] = { record, draw, weight };
    return read_host(c, [&](Framebuffer& F, hipStream_t st) {
        const size_t plane = (size_t)c->W * c->H, pitch = (size_t)c->W * 4;
        for (int k = 0; k < 3; ++k)
            if (dst[k]) { const hipError_t e = hipMemcpy2DAsync(dst[k], (size_t)w * 4, F.ids + k * plane + (size_t)y * c->W + x, pitch, (size_t)w * 4, (size_t)h, hipMemcpyDeviceToHost, st); if (e != hipSuccess) return e; }
        return hipSuccess;
    });
}

int gs4d_read_ids_device(gs4d_ctx* c, void* record, void* draw, void* weight, size_t bytes_per_plane) {
    if (!c || (!record && !draw && !weight)) return GS4D_E_INVALID;
    int rc = read_begin(c, bytes_per_plane == (size_t)c->W * c->H * 4, "read_ids_device: bytes_per_plane != width*height*4", Outputs::Ids, "read_ids_device: the current frame was not cleared with ID outputs on"); if (rc) return rc;
    void* const dst[3] = { record, draw, weight };
    return read_device_common(c, 0, ReadPlane::Ids, dst);
}

// ---- selection: a statistics table from a region of the ID planes ----
int gs4d_count_ids(gs4d_ctx* c, const gs4d_id_region* region, gs4d_buf mask, gs4d_buf stats, size_t nrecords) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "count_ids";
    const gs4d_id_region g = region ? *region : gs4d_id_region{ 0, 0, c->W, c->H, 0u, 0xFFFFFFFFu, 0u, 0u };
    if (g.reserved != 0u) return refuse(c, fn, "non-zero reserved field in the region");
    if (g.draw_first > g.draw_last) return refuse(c, fn, "draw_first > draw_last");
    if (nrecords > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    if (g.x < 0 || g.y < 0 || g.w <= 0 || g.h <= 0 || g.w > c->W - g.x || g.h > c->H - g.y) return refuse(c, fn, "the rectangle is empty or not inside the image");
    if (c->fbs[c->cur_fb].out < Outputs::Ids) return refuse(c, fn, "the current frame was not cleared with ID outputs on");      // (before read_begin launches the queued order: a refused call queues nothing)
    // stats as WRITE: the lane waits for whoever wrote the table AND for whoever still reads it or adds to it, which is what a read-modify-write
    // needs; the new version and the dropped provenance are those of any kernel write
    Operands ops{ { "stats", stats, false, sizeof(gs4d_record_stat), nrecords, OP_WRITE | OP_SETTLE },
                  { "mask", mask, true, 1, (uint64_t)g.w * (uint64_t)g.h, OP_READ } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (nrecords == 0) return GS4D_OK;
    // the planes as gs4d_read_ids_device takes them: the queued order launched, the frame's draws settled, every tile in memory
    { int rc = flush_order(c); if (rc) return rc; }
    { int rc = resolve_image(c, c->cur_fb); if (rc) return rc; }
    return queue_operands(c, ops, [&](Lane& L) {
        Framebuffer& F = c->fbs[c->cur_fb];
        { int rc = fb_access(c, F); if (rc) return rc; }
        { int rc = materialise_fb(c, F, L); if (rc) return rc; }
        HIPCHK(c, launch_count_ids(L.s, F.ids, c->W, c->H, g, (const uint8_t*)ops.ptr(mask), (gs4d_record_stat*)ops.ptr(stats), (uint32_t)nrecords));
        return (int)GS4D_OK;
    });
}

// ---- selection by where a record is: a statistics table from a volume or a screen region ----
int gs4d_count_centres(gs4d_ctx* c, gs4d_buf data, size_t n, const gs4d_centre_query* query, gs4d_buf mask, gs4d_buf stats) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "count_centres";
    if (!query) return refuse(c, fn, "query == NULL");
    const gs4d_centre_query q = *query;
    constexpr uint32_t known = GS4D_CQ_BOX | GS4D_CQ_SPHERE | GS4D_CQ_SCREEN | GS4D_CQ_FRAME | GS4D_CQ_SKIP_HIDDEN | GS4D_CQ_SKIP_DEAD;
    if ((q.tests & ~known) != 0u) return refuse(c, fn, "unknown test bit");
    if (q.op != (uint32_t)GS4D_CQ_ADD && q.op != (uint32_t)GS4D_CQ_REMOVE) return refuse(c, fn, "unknown op");
    if (q.reserved != 0u) return refuse(c, fn, "non-zero reserved field in the query");
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    const bool screen = (q.tests & (uint32_t)GS4D_CQ_SCREEN) != 0u;
    if (mask != 0 && !screen) return refuse(c, fn, "a mask is given without GS4D_CQ_SCREEN");
    if (screen && (q.x < 0 || q.y < 0 || q.w <= 0 || q.h <= 0 || q.w > c->W - q.x || q.h > c->H - q.y)) return refuse(c, fn, "the rectangle is empty or not inside the image");
    // stats as WRITE, as in gs4d_count_ids: a read-modify-write the lane has the table to itself for.  data and mask are read (a mask comes with a
    // rectangle that has been checked: w * h is its size).
    Operands ops{ { "data", data, false, 96, n, OP_READ },
                  { "stats", stats, false, sizeof(gs4d_record_stat), n, OP_WRITE | OP_SETTLE },
                  { "mask", mask, true, 1, (uint64_t)q.w * (uint64_t)q.h, OP_READ } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    Buffer* const D = ops.buffer(data);
    // Where the fields are read: a shadow of data that is current holds the bits of the records in dense planes (k_soa_repack) — decided once the
    // pending draws are settled (a re-run may rebuild the shadow) and before any buffer state is touched.  The call reads: it never builds a shadow,
    // and a reader leaves `version` alone, so a current shadow stays current.
    bool shadow = false;
    return queue_operands(c, ops,
        [&](Lane&) { shadow = D->soa && D->soa_n == D->bytes / 96 && D->soa_version == D->version; return (int)GS4D_OK; },
        [&](Lane& L) {
            HIPCHK(c, launch_count_centres(L.s, D->d, shadow ? D->soa : nullptr, D->soa_n, D->soa_info, n, q, c->W, c->H, (const uint8_t*)ops.ptr(mask), (gs4d_record_stat*)ops.ptr(stats)));
            return (int)GS4D_OK;
        });
}

// ---- where a selection is: bounds and centroid of selected records ----
int gs4d_measure_records(gs4d_ctx* c, gs4d_buf data, size_t n, const gs4d_measure_query* query, gs4d_buf stats, const gs4d_keep_rule* rule, gs4d_buf out) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "measure_records";
    if (!query) return refuse(c, fn, "query == NULL");
    const gs4d_measure_query q = *query;
    if ((q.flags & ~(uint32_t)(GS4D_MS_SKIP_HIDDEN | GS4D_MS_SKIP_DEAD)) != 0u) return refuse(c, fn, "unknown flag");
    if (q.reserved[0] != 0u || q.reserved[1] != 0u) return refuse(c, fn, "non-zero reserved field in the query");
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    if ((stats != 0) != (rule != nullptr)) return refuse(c, fn, "stats and rule are given together or not at all");
    KeepRule k;
    if (!keep_rule_of(rule, k)) return refuse(c, fn, "unknown flag or non-zero reserved field in the rule");
    // data and the table are read (gs4d_count_centres' data, gs4d_edit_colours' table), out is written whole (gs4d_stat_cut's out).  The kernels read
    // the 96-byte records, never a shadow, and a reader leaves `version` alone: a current shadow stays current and none is built.
    Operands ops{ { "data", data, false, 96, n, OP_READ },
                  { "stats", stats, true, sizeof(gs4d_record_stat), n, OP_READ | OP_SETTLE | OP_SCAN },
                  { "out", out, false, 1, sizeof(gs4d_measure), OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    return queue_operands(c, ops,
        [&](Lane& L) {
            HIPCHK(c, grow_device_array(L.s, L.measure_scratch, L.measure_cap, measure_scratch_words()));
            return (int)GS4D_OK;
        },
        [&](Lane& L) {
            HIPCHK(c, launch_measure_records(L.s, ops.ptr(data), n, q.t, q.flags, (const gs4d_record_stat*)ops.ptr(stats), k, L.measure_scratch, (gs4d_measure*)ops.ptr(out)));
            return (int)GS4D_OK;
        });
}

// ---- records relative to each other: the sources within a radius of each record, as a statistics table ----
int gs4d_count_neighbours(gs4d_ctx* c, gs4d_buf data, size_t n, const gs4d_neighbour_query* query, gs4d_buf source, const gs4d_keep_rule* rule, gs4d_buf stats) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    if (!query) return fail(c, GS4D_E_INVALID, "count_neighbours: query == NULL");
    const gs4d_neighbour_query q = *query;
    const GridQuery g{ q.radius, q.flags, (uint32_t)(GS4D_NB_SKIP_HIDDEN | GS4D_NB_SKIP_DEAD | GS4D_NB_COUNT_SELF), q.reserved, q.cap == 0u ? "cap == 0" : nullptr };
    const GridOutputs o{ "stats", stats, sizeof(gs4d_record_stat), true, 0, nullptr };
    return grid_query(c, "count_neighbours", g, n, data, source, rule, o,
        [&](Lane& L, const void* records, const gs4d_record_stat* rows, const KeepRule& k, void* table, gs4d_record_stat*) {
            HIPCHK(c, launch_count_neighbours(L.s, L.pair_sort, records, n, q, rows, k, L.neighbour_scratch, (gs4d_record_stat*)table, c->neighbour_phases));
            return (int)GS4D_OK;
        });
}

// ---- connected clusters: one label per record, optionally the cluster's size as a statistics table ----
int gs4d_label_components(gs4d_ctx* c, gs4d_buf data, size_t n, const gs4d_component_query* query, gs4d_buf source, const gs4d_keep_rule* rule, gs4d_buf labels,
                          gs4d_buf stats) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    if (!query) return fail(c, GS4D_E_INVALID, "label_components: query == NULL");
    const gs4d_component_query q = *query;
    const GridQuery g{ q.radius, q.flags, (uint32_t)(GS4D_CC_SKIP_HIDDEN | GS4D_CC_SKIP_DEAD), q.reserved, q.cap == 0u ? "cap == 0" : nullptr };
    const GridOutputs o{ "labels", labels, sizeof(uint32_t), false, stats, nullptr };
    return grid_query(c, "label_components", g, n, data, source, rule, o,
        [&](Lane& L, const void* records, const gs4d_record_stat* rows, const KeepRule& k, void* words, gs4d_record_stat* table) {
            HIPCHK(c, launch_label_components(L.s, L.pair_sort, records, n, q, rows, k, L.neighbour_scratch, (uint32_t*)words, table, L.err_word()));
            return (int)GS4D_OK;
        });
}

// ---- what a selection touches, by label: the records whose label is the label of a seed ----
int gs4d_count_labels(gs4d_ctx* c, gs4d_buf labels, size_t n, gs4d_buf seeds, const gs4d_keep_rule* rule, gs4d_buf stats) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "count_labels";
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    if (!rule) return refuse(c, fn, "rule == NULL");
    KeepRule k;
    if (!keep_rule_of(rule, k)) return refuse(c, fn, "unknown flag or non-zero reserved field in the rule");
    // labels and seeds are read (seeds as gs4d_edit_colours reads its table), stats is a read-modify-write the lane has the table to itself for: it
    // is declared before seeds because it is settled before seeds.  The flag words live in the lane's neighbour scratch, whose reuse the lane's
    // stream orders.
    Operands ops{ { "labels", labels, false, sizeof(uint32_t), n, OP_READ },
                  { "stats", stats, false, sizeof(gs4d_record_stat), n, OP_WRITE | OP_SETTLE },
                  { "seeds", seeds, false, sizeof(gs4d_record_stat), n, OP_READ | OP_SETTLE | OP_SCAN } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops,
        [&](Lane& L) {
            HIPCHK(c, grow_device_array(L.s, L.neighbour_scratch, L.neighbour_cap, n));
            return (int)GS4D_OK;
        },
        [&](Lane& L) {
            HIPCHK(c, launch_count_labels(L.s, (const uint32_t*)ops.ptr(labels), n, (const gs4d_record_stat*)ops.ptr(seeds), k, L.neighbour_scratch, (gs4d_record_stat*)ops.ptr(stats)));
            return (int)GS4D_OK;
        });
}

// ---- the k nearest sources of every record: a table of hits, optionally the count and the last distance as a statistics table ----
int gs4d_nearest_neighbours(gs4d_ctx* c, gs4d_buf data, size_t n, const gs4d_nearest_query* query, gs4d_buf source, const gs4d_keep_rule* rule, gs4d_buf hits,
                            size_t hit_stride, gs4d_buf stats) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    if (!query) return fail(c, GS4D_E_INVALID, "nearest_neighbours: query == NULL");
    const gs4d_nearest_query q = *query;
    const GridQuery g{ q.radius, q.flags, (uint32_t)(GS4D_NN_SKIP_HIDDEN | GS4D_NN_SKIP_DEAD | GS4D_NN_INCLUDE_SELF), q.reserved,
                       q.k == 0u || q.k > 16u ? "k must be 1 to 16" : nullptr };
    const bool stride_ok = record_stride_ok(hit_stride) && hit_stride >= 8 * (size_t)q.k;
    const GridOutputs o{ "hits", hits, hit_stride, false, stats, stride_ok ? nullptr : "hit_stride must be a multiple of 16 from 16 to 1024 that is at least 8 k" };
    return grid_query(c, "nearest_neighbours", g, n, data, source, rule, o,
        [&](Lane& L, const void* records, const gs4d_record_stat* rows, const KeepRule& k, void* slots, gs4d_record_stat* table) {
            HIPCHK(c, launch_nearest_neighbours(L.s, L.pair_sort, records, n, q, rows, k, L.neighbour_scratch, slots, hit_stride, table));
            return (int)GS4D_OK;
        });
}

// ---- a label per record from a 4D cell grid ----
int gs4d_cell_labels(gs4d_ctx* c, gs4d_buf data, size_t n, const gs4d_cell_grid* grid, gs4d_buf labels) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "cell_labels";
    if (!grid) return refuse(c, fn, "grid == NULL");
    const gs4d_cell_grid g = *grid;
    if (!gs4d_merge::grid_ok(g.edge, g.dims, g.reserved))
        return refuse(c, fn, "dims must be 1 .. 65536 with a product of at most 0xFFFFFFFE, edge finite and > 0 where dims > 1, reserved 0");
    if (n > 0xFFFFFFFFull) return refuse(c, fn, "more than 2^32 - 1 records");
    // data is read (the 96-byte records, never a shadow: a reader leaves `version` alone), labels is written
    Operands ops{ { "data", data, false, 96, n, OP_READ }, { "labels", labels, false, sizeof(uint32_t), n, OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (n == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_cell_labels(L.s, ops.ptr(data), n, g, (uint32_t*)ops.ptr(labels)));
        return (int)GS4D_OK;
    });
}

// ---- one moment-matched record per labelled group ----
int gs4d_merge_records(gs4d_ctx* c, gs4d_buf data, size_t n, gs4d_buf labels, const gs4d_merge_query* query, gs4d_buf stats, const gs4d_keep_rule* rule,
                       gs4d_buf dst, gs4d_buf groups, gs4d_buf member_group, gs4d_buf count) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "merge_records";
    if (!query) return refuse(c, fn, "q == NULL");
    const gs4d_merge_query q = *query;
    if (!(gs4d_merge::finite(q.alpha_max) && q.alpha_max > 0.0f)) return refuse(c, fn, "alpha_max must be finite and > 0");
    if (q.flags != 0u || q.reserved[0] != 0u || q.reserved[1] != 0u) return refuse(c, fn, "flags or a reserved field of the query is not 0");
    if (n >= 0xFFFFFFFFull) return refuse(c, fn, "the sort takes 2^32 - 2 records at most");
    if ((stats != 0) != (rule != nullptr)) return refuse(c, fn, "stats and rule are given together or not at all");
    KeepRule k;
    if (!keep_rule_of(rule, k)) return refuse(c, fn, "unknown flag or non-zero reserved field in the rule");
    // data, labels and the table are read (gs4d_measure_records' data and table); dst is written as gs4d_transform_records writes its own (a full
    // write: the next draw repacks the shadow once), and holds what it holds (cap), like groups; member_group and count are written whole.
    Operands ops{ { "data", data, false, 96, n, OP_READ },
                  { "labels", labels, false, sizeof(uint32_t), n, OP_READ },
                  { "stats", stats, true, sizeof(gs4d_record_stat), n, OP_READ | OP_SETTLE | OP_SCAN },
                  { "dst", dst, false, 96, 0, OP_WRITE },
                  { "groups", groups, true, sizeof(gs4d_merge_group), 0, OP_WRITE },
                  { "member_group", member_group, true, sizeof(uint32_t), n, OP_WRITE },
                  { "count", count, false, 1, sizeof(gs4d_merge_count), OP_WRITE } };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    // slots the outputs hold: no slot >= cap is ever written
    uint32_t cap = (uint32_t)std::min<size_t>(0xFFFFFFFFu, ops.buffer(dst)->bytes / 96);
    if (Buffer* G = ops.buffer(groups)) cap = (uint32_t)std::min<size_t>(cap, G->bytes / sizeof(gs4d_merge_group));
    return queue_operands(c, ops,
        [&](Lane& L) {
            if (n == 0) return (int)GS4D_OK;
            HIPCHK(c, grow_device_array(L.s, L.neighbour_scratch, L.neighbour_cap, merge_scratch_words(n)));
            HIPCHK(c, sort_scratch_reserve(L.s, L.pair_sort, n));      // (the tile sort's scratch, as gs4d_spatial_order: a histogram a queued keygen has left in depth_sort stays where it is)
            return (int)GS4D_OK;
        },
        [&](Lane& L) {
            HIPCHK(c, launch_merge_records(L.s, L.pair_sort, ops.ptr(data), n, (const uint32_t*)ops.ptr(labels), q.alpha_max, (const gs4d_record_stat*)ops.ptr(stats), k,
                                           L.neighbour_scratch, ops.ptr(dst), (gs4d_merge_group*)ops.ptr(groups), (uint32_t*)ops.ptr(member_group), cap,
                                           (gs4d_merge_count*)ops.ptr(count)));
            return (int)GS4D_OK;
        });
}

// ---- one merged row of a table per group: the SH row of a merged record ----
int gs4d_merge_rows(gs4d_ctx* c, gs4d_buf data, size_t n, gs4d_buf member_group, gs4d_buf rows, const gs4d_rows_query* query, gs4d_buf dst, size_t dst_first,
                    gs4d_buf count) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "merge_rows";
    const gs4d_rows_query q = query ? *query : gs4d_rows_query{ 0u, 0u, 0u, 0u };
    if (const char* fault = merge_rows_fault(query != nullptr, q.stride, q.width, q.flags, q.reserved, n, dst_first)) return refuse(c, fn, fault);
    static_assert(sizeof(gs4d_merge_count) == 16, "the rows of rows_operands.h");
    Operand list[MERGE_ROWS_OPERANDS];                         // (rows_operands.h: what the call does with each)
    merge_rows_operands(list, data, n, member_group, rows, q.stride, dst, count);
    Operands ops{ list[0], list[1], list[2], list[3], list[4] };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    const size_t capacity = ops.buffer(dst)->bytes / q.stride;  // rows dst holds: no row >= capacity is ever written
    return queue_operands(c, ops,
        [&](Lane& L) {
            if (n == 0) return (int)GS4D_OK;
            HIPCHK(c, grow_device_array(L.s, L.neighbour_scratch, L.neighbour_cap, merge_rows_scratch_words(n)));
            HIPCHK(c, sort_scratch_reserve(L.s, L.pair_sort, n));      // (the tile sort's scratch, as gs4d_merge_records)
            return (int)GS4D_OK;
        },
        [&](Lane& L) {
            HIPCHK(c, launch_merge_rows(L.s, L.pair_sort, ops.ptr(data), n, (const uint32_t*)ops.ptr(member_group), ops.ptr(rows), q, L.neighbour_scratch, ops.ptr(dst),
                                        dst_first, capacity, (gs4d_merge_count*)ops.ptr(count)));
            return (int)GS4D_OK;
        });
}

int gs4d_copy_rows(gs4d_ctx* c, gs4d_buf src, size_t src_first, size_t m, size_t stride, gs4d_buf dst, size_t dst_first) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "copy_rows";
    if (const char* fault = copy_rows_fault(src_first, m, stride, dst_first)) return refuse(c, fn, fault);
    Operand list[COPY_ROWS_OPERANDS];                          // (rows_operands.h: what the call does with each)
    copy_rows_operands(list, src, src_first, m, stride, dst, dst_first);
    Operands ops{ list[0], list[1] };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (m == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_copy_rows(L.s, ops.ptr(src), src_first, m, stride, ops.ptr(dst), dst_first));
        return (int)GS4D_OK;
    });
}

// ---- the view's cut through a forest of merged levels ----
int gs4d_lod_append(gs4d_ctx* c, gs4d_buf level, size_t m, gs4d_buf member_group, size_t child_first, size_t cn, gs4d_buf nodes, gs4d_buf parent, size_t first) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "lod_append";
    if (const char* fault = lod_append_fault(m, member_group != 0, child_first, cn, first)) return refuse(c, fn, fault);
    Operand list[LOD_APPEND_OPERANDS];                         // (lod_operands.h: what the call does with each)
    lod_append_operands(list, level, m, member_group, cn, nodes, parent, first);
    Operands ops{ list[0], list[1], list[2], list[3] };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    if (m == 0 && cn == 0) return GS4D_OK;
    return queue_operands(c, ops, [&](Lane& L) {
        HIPCHK(c, launch_lod_append(L.s, ops.ptr(level), m, (const uint32_t*)ops.ptr(member_group), child_first, cn, ops.ptr(nodes), (uint32_t*)ops.ptr(parent), first));
        return (int)GS4D_OK;
    });
}

int gs4d_lod_cut(gs4d_ctx* c, gs4d_buf nodes, gs4d_buf parent, size_t n, const gs4d_lod_query* query, gs4d_buf dst, gs4d_buf cut_index, gs4d_buf stats, gs4d_buf count) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    const char* const fn = "lod_cut";
    if (!query) return refuse(c, fn, "q == NULL");
    const gs4d_lod_query q = *query;
    if (!gs4d_lod::query_ok(q, n))
        return refuse(c, fn, "n at most 2^32 - 2; levels 1 .. 16; level_first from 0, not decreasing, to n; ratio >= 0; near_dist finite and >= 0; flags and reserved 0");
    static_assert(sizeof(gs4d_record_stat) == 16 && sizeof(gs4d_lod_count) == 16, "the rows of lod_operands.h");
    Operand list[LOD_CUT_OPERANDS];                            // (lod_operands.h: what the call does with each)
    lod_cut_operands(list, nodes, parent, n, dst, cut_index, stats, count);
    Operands ops{ list[0], list[1], list[2], list[3], list[4], list[5] };
    { int rc = check_operands(c, fn, ops); if (rc) return rc; }
    // slots the outputs hold: no slot >= cap is ever written
    uint32_t cap = 0xFFFFFFFFu;
    if (Buffer* D = ops.buffer(dst)) cap = (uint32_t)std::min<size_t>(cap, D->bytes / 96);
    if (Buffer* X = ops.buffer(cut_index)) cap = (uint32_t)std::min<size_t>(cap, X->bytes / 4);
    return queue_operands(c, ops,
        [&](Lane& L) {
            if (n == 0) return (int)GS4D_OK;
            HIPCHK(c, grow_device_array(L.s, L.lod_state, L.lod_cap, (n + 15) & ~(size_t)15));
            HIPCHK(c, grow_device_array(L.s, L.compact_counts, L.compact_cap, std::max<size_t>(1, compact_tiles(n))));
            return (int)GS4D_OK;
        },
        [&](Lane& L) {
            HIPCHK(c, launch_lod_cut(L.s, ops.ptr(nodes), (const uint32_t*)ops.ptr(parent), n, q, L.lod_state, L.compact_counts, ops.ptr(dst), (uint32_t*)ops.ptr(cut_index),
                                     (gs4d_record_stat*)ops.ptr(stats), cap, (gs4d_lod_count*)ops.ptr(count)));
            return (int)GS4D_OK;
        });
}

int gs4d_read_pixels_rgba8_device(gs4d_ctx* c, void* dptr, size_t bytes) {
    if (!c || !dptr) return GS4D_E_INVALID;
    int rc = read_begin(c, bytes == (size_t)c->W * c->H * 4, "read_pixels_rgba8_device: bytes != width*height*4"); if (rc) return rc;
    return read_device_common(c, 0, ReadPlane::ColourRGBA8, &dptr);
}

int gs4d_read_frame_rgba8_device(gs4d_ctx* c, int frames_back, void* dptr, size_t bytes) {
    if (!c || !dptr) return GS4D_E_INVALID;
    int rc = read_begin(c, bytes == (size_t)c->W * c->H * 4, "read_frame_rgba8_device: bytes != width*height*4"); if (rc) return rc;
    return read_device_common(c, frames_back, ReadPlane::ColourRGBA8, &dptr);
}

int gs4d_read_frame_rgba8_device_after(gs4d_ctx* c, int frames_back, void* dptr, size_t bytes, void* hip_event) {
    if (!c || !dptr) return GS4D_E_INVALID;
    int rc = read_begin(c, bytes == (size_t)c->W * c->H * 4, "read_frame_rgba8_device_after: bytes != width*height*4"); if (rc) return rc;
    return read_device_common(c, frames_back, ReadPlane::ColourRGBA8, &dptr, true, (hipEvent_t)hip_event);
}

static int band_pixel_rows(const gs4d_ctx* c) {
    int rows = 0;
    for (int ty = c->shard_rank; ty < c->tiles_y; ty += c->shard_world) rows += std::min(TILE, c->H - ty * TILE);
    return rows;
}

int gs4d_set_tile_shard(gs4d_ctx* c, int rank, int world) {
    if (!c) return GS4D_E_INVALID;
    if (world < 1 || world > 1024 || rank < 0 || rank >= world) return fail(c, GS4D_E_INVALID, "set_tile_shard: need 0 <= rank < world <= 1024");
    c->shard_rank = rank; c->shard_world = world;
    return GS4D_OK;
}

int gs4d_band_rows(gs4d_ctx* c, int* rows) {
    if (!c || !rows) return GS4D_E_INVALID;
    *rows = band_pixel_rows(c);
    return GS4D_OK;
}

int gs4d_read_band_rgba8_device(gs4d_ctx* c, void* dptr, size_t bytes) {
    if (!c || !dptr) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    const int rows = band_pixel_rows(c);
    if (bytes != (size_t)rows * c->W * 4) return fail(c, GS4D_E_INVALID, "read_band_rgba8_device: bytes != band_rows*width*4");
    int rc = resolve_image(c, c->cur_fb); if (rc) return rc;
    rc = after_user_stream(c); if (rc) return rc;
    Framebuffer& F = c->fbs[c->cur_fb];
    rc = fb_access(c, F); if (rc) return rc;
    Lane& L = lane(c);
    HIPCHK(c, launch_pack_rgba8_band(L.s, F.mem, F.tstate, F.epoch, F.clear, c->W, c->H, c->tiles_x, c->shard_rank, c->shard_world, rows, (uint32_t*)dptr));
    if (c->user) {
        HIPCHK(c, hipEventRecord(c->ev_readback, L.s));
        HIPCHK(c, hipStreamWaitEvent(c->user, c->ev_readback, 0));
    }
    return GS4D_OK;
}

int gs4d_set_stream(gs4d_ctx* c, void* hip_stream) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    int rc = resolve_pending(c); if (rc) return rc;
    rc = sync_all(c); if (rc) return rc;             // everything queued so far completes before the ordering contract changes
    c->user = (hipStream_t)hip_stream;
    return GS4D_OK;
}

// ---- measurement / test hooks ----
int gs4d_set_profiling(gs4d_ctx* c, int stage_mask) {
    if (!c) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    if (stage_mask && c->ev0.empty()) {
        const size_t n = (size_t)gs4d_ctx::PROF_FRAMES * GS4D_T_COUNT;
        c->ev0.assign(n, nullptr); c->ev1.assign(n, nullptr); c->ran.assign(n, 0);
        for (size_t i = 0; i < n; ++i) { HIPCHK(c, hipEventCreate(&c->ev0[i])); HIPCHK(c, hipEventCreate(&c->ev1[i])); }
    }
    c->profiling = (unsigned)stage_mask & 0x3Fu;
    c->prof_every = ((stage_mask >> 8) & 0xFF) ? ((stage_mask >> 8) & 0xFF) : 1;
    c->prof_tick = 0;
    c->prof_frame = 0;
    std::fill(c->ran.begin(), c->ran.end(), 0);
    return GS4D_OK;
}

int gs4d_get_timings(gs4d_ctx* c, float ms[GS4D_T_COUNT]) {
    if (!c || !ms) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    int rc = resolve_pending(c); if (rc) return rc;
    rc = sync_all(c); if (rc) return rc;
    // average per stage over the frames recorded since profiling was switched on (or since the last call); then restart
    for (int i = 0; i < GS4D_T_COUNT; ++i) {
        double sum = 0; int cnt = 0;
        for (int f = 0; f < gs4d_ctx::PROF_FRAMES && !c->ran.empty(); ++f) {
            const int slot = f * GS4D_T_COUNT + i;
            if (!c->ran[slot]) continue;
            float t = 0;
            if (hipEventElapsedTime(&t, c->ev0[slot], c->ev1[slot]) == hipSuccess) { sum += t; ++cnt; }
        }
        ms[i] = cnt ? (float)(sum / cnt) : -1.0f;
    }
    c->prof_frame = 0;
    std::fill(c->ran.begin(), c->ran.end(), 0);
    return GS4D_OK;
}

int gs4d_get_timeline(gs4d_ctx* c, float* ms, int max_frames, int* frames_out) {
    if (!c || !ms || !frames_out || max_frames < 0) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    int rc = resolve_pending(c); if (rc) return rc;
    rc = sync_all(c); if (rc) return rc;
    const int frames = std::min(std::min(max_frames, c->prof_frame), (int)gs4d_ctx::PROF_FRAMES);
    *frames_out = frames;
    if (c->ran.empty() || frames == 0) { *frames_out = 0; return GS4D_OK; }
    int base = -1;                                   // first stage of frame 0 that ran: time zero
    for (int i = 0; i < GS4D_T_COUNT && base < 0; ++i) if (c->ran[i]) base = i;
    if (base < 0) { *frames_out = 0; return GS4D_OK; }
    for (int f = 0; f < frames; ++f)
        for (int i = 0; i < GS4D_T_COUNT; ++i) {
            const int slot = f * GS4D_T_COUNT + i;
            float t0 = -1.0f, t1 = -1.0f;
            if (c->ran[slot]) {
                if (hipEventElapsedTime(&t0, c->ev0[base], c->ev0[slot]) != hipSuccess) t0 = -1.0f;
                if (hipEventElapsedTime(&t1, c->ev0[base], c->ev1[slot]) != hipSuccess) t1 = -1.0f;
            }
            ms[(size_t)slot * 2] = t0; ms[(size_t)slot * 2 + 1] = t1;
        }
    return GS4D_OK;
}

int gs4d_get_stats(gs4d_ctx* c, uint64_t stats[8]) {
    if (!c || !stats) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    int rc = resolve_pending(c); if (rc) return rc;
    stats[0] = (c->stat_entries & 0xFFFFFFFFull) | (c->stat_staged << 32); stats[1] = ((uint64_t)lane(c).pair_cap & 0xFFFFFFFFFFull) | (c->stat_staged_misses << 40); stats[2] = (c->stat_reruns & 0xFFFFFFFFull) | (c->stat_aborted_discarded << 32); stats[3] = (uint64_t)c->tiles_x * c->tiles_y | ((c->stat_shadow_bytes & 0xFFull) << 32) | ((c->stat_composited_tiles & 0xFFFFFFull) << 40);
    stats[4] = (c->stat_depth_passes & 0xFFFFFFFFull) | (c->stat_streams_rejected << 32); stats[5] = (c->stat_tile_passes & 0xFFFFFFFFull) | (c->stat_renamed << 32); stats[6] = (uint64_t)(c->nlanes & 0xFFFF) | (c->stat_lanes_sharing << 16) | (c->stat_fused << 32); stats[7] = c->stat_v2_draws | (c->stat_longest << 32);
    return GS4D_OK;
}

int gs4d_get_sort_stats(gs4d_ctx* c, uint64_t stats[4]) {
    if (!c || !stats) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    int rc = resolve_pending(c); if (rc) return rc;
    rc = sync_all(c); if (rc) return rc;                // the report words are final: every queued sort has run
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    for (int i = 0; i < c->nlanes; ++i) {
        const SortScratch& s = c->lanes[i].depth_sort;
        stats[0] += s.stat_hybrid; stats[1] += s.stat_launches;
        if (s.fb && s.fb[2]) { stats[2] = std::max<uint64_t>(stats[2], s.fb[0]); stats[3] += s.fb[1]; }
    }
    return GS4D_OK;
}

#ifdef GS4D_TUNING
// tuning builds only (make TUNING=1; looked up by name by host/gs4d_sweep --fake-comm-us): occupy `stream` for `usec` microseconds with one spinning
// thread — a stand-in for a communication kernel that holds the stream's hardware queue while it moves data over a slow link
__attribute__((visibility("default"))) int gs4d_tuning_spin(void* stream, unsigned usec) {
    k_lane_probe_spin<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>((unsigned long long)usec * 100ull, g_tuning_spin_out());
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif

int gs4d_debug_read_projected(gs4d_ctx* c, float* out16, size_t nrecords) {
    if (!c || !out16) return GS4D_E_INVALID;
    (void)hipSetDevice(c->device);
    { int rcq = flush_order(c); if (rcq) return rcq; }
    Lane& L = lane(c);
    if (nrecords > L.proj_n) return fail(c, GS4D_E_INVALID, "debug_read_projected: more records than the last draw projected");
    int rc = resolve_pending(c); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out16, L.proj, nrecords * 64, hipMemcpyDeviceToHost, L.s));
    HIPCHK(c, hipStreamSynchronize(L.s));
    // expose the layout documented in gs4d.h: cx,cy,a0x,a0y,a1x,a1y,alpha,r,g,b,rect0,rect1,hx,hy,valid,0
    // stored (gs4d_internal.h):               cx,cy,a0x,a1x,a0y,a1y,r,g,b,alpha,rect0,rect1,hx,hy,valid,0
    for (size_t i = 0; i < nrecords; ++i) {
        float* r = out16 + 16 * i;
        const float a1x = r[3], a0y = r[4], cr = r[6], cg = r[7], cb = r[8], al = r[9];
        r[3] = a0y; r[4] = a1x; r[6] = al; r[7] = cr; r[8] = cg; r[9] = cb;
    }
    return GS4D_OK;
}

int gs4d_debug_shadow_builds(gs4d_ctx* c, gs4d_buf buf, uint64_t* builds) {
    if (!c || !builds) return GS4D_E_INVALID;
    const Buffer* B = getbuf(c, buf);
    if (!B) return fail(c, GS4D_E_INVALID, "debug_shadow_builds: bad buffer name");
    *builds = B->soa_builds;
    return GS4D_OK;
}

} // extern "C"

/* gs4d.h — C ABI of libgs4d.so, the MI355X (gfx950) forward Gaussian-splat rasteriser.
 *
 * This is the drop-in boundary for ONE path of EndMy5uffering/4DGaussianSplatRendering: everything
 * from the upload of the splat SSBO to pixels.  The reference has no FFI of its own:
 * the surface it exposes to its scenes is a set of C++ classes over OpenGL (Renderer, ShareStorageBuffer,
 * Shader, radix_sort::sorter) plus six raw GL calls.  Every entry point below names the reference call
 * it stands in for (file:line relative to the reference tree); the C++ mirror of those classes that a
 * maintainer would compile Scenes.h against lives in 4dgaussiansplatrendering_amd/host/ and is a thin
 * wrapper over these functions.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns 0 on success or a
 * negative GS4D_E_* code (no exception crosses the ABI); gs4d_last_error() returns a description.
 * Matrices are 16 floats, column-major (m[4*c + r]), exactly what glUniformMatrix4fv(…, GL_FALSE, …)
 * receives from glm::mat4.  Buffers are named by small integers like GL buffer names; 0 is "none";
 * deleting 0 or an already-deleted name is tolerated (the reference double-deletes, Scenes.h:220-224, 291-299).
 * Calls return as soon as their work is queued; only the read-back / finish calls block.  Results are as if the calls had run one
 * after another.  Internally a context spreads consecutive FRAMES over a few HIP streams ("frame lanes", 4 by default) so that they
 * overlap on the device: a frame is everything from one gs4d_clear / gs4d_keygen / gs4d_sort_pairs that follows a draw up to and
 * including the next draw(s); buffers and the framebuffer carry their own cross-lane ordering.  A gs4d_clear starts rendering into the
 * next image of a small swap chain (one RGBA32F image per lane); gs4d_read_pixels* read the image the last clear/draw used.
 * One context = one GPU; contexts are independent (one process per GPU for multi-GPU runs).
 * The framebuffer is RGBA float32, row 0 = bottom row (OpenGL window origin).
 */
#ifndef GS4D_H
#define GS4D_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define GS4D_API __attribute__((visibility("default")))
#else
#define GS4D_API
#endif

typedef struct gs4d_ctx gs4d_ctx;
typedef uint32_t gs4d_buf;

enum {
    GS4D_OK = 0,
    GS4D_E_INVALID = -1,      /* bad argument / bad buffer name / size mismatch          */
    GS4D_E_DEVICE = -2,       /* HIP runtime error (message in gs4d_last_error)          */
    GS4D_E_UNSUPPORTED = -3,  /* state the path does not implement (e.g. other blend funcs) */
    GS4D_E_NOMEM = -4
};

/* Pipeline selection = which shader pair the reference scene would have bound (Shader::AddShaderSource paths). */
enum {
    GS4D_MODE_4D_SORTED = 0, /* Shader/Splats4D/Splat4DVertexShaderInstanced.GLSL + Splat4DFragShader.GLSL: slot 1 = sortidx[], slot 2 = SplatData[] (96 B) */
    GS4D_MODE_4D_DIRECT = 1, /* Shader/Splats4D/Splat4DVertexShaderMod.GLSL: slot 1 = SplatData[], instance id indexes it directly                         */
    GS4D_MODE_3D_FULL   = 2, /* Shader/Splats3D/Splat3DVertexShaderFull.GLSL + Splat3DFragShaderFull.GLSL: 4 x 72-B vertices per splat (gs4d_draw_quads) */
    GS4D_MODE_2D        = 3  /* Shader/Splats2D/Splat2DVSI.GLSL + Splat2DFragShader.GLSL: slot 1 = 48-B records                                         */
};

enum { GS4D_U_TIME = 0, GS4D_U_MIN_OPACITY = 1 };  /* uTime, uMinOpacity (Scenes.h:331-332) */
enum { GS4D_U_VIEW = 0, GS4D_U_PROJ = 1 };         /* uView, uProj       (Scenes.h:333-334) */

enum { GS4D_KEY_REF_INV_EUCLID = 0,  /* 1/|mean'(t) - cam|, the reference's key (Scenes.h:28-36, 314-319) */
       GS4D_KEY_VIEW_Z = 1 };        /* extra: key = 1/(-z_view) of the time-conditioned mean              */

/* glBlendFunc factors: GL enum values (Application.cpp:137-138, 150); the set is the one the reference's blend menu offers (DebugMenus.h:41-59) */
enum { GS4D_ZERO = 0, GS4D_ONE = 1, GS4D_SRC_COLOR = 0x0300, GS4D_ONE_MINUS_SRC_COLOR = 0x0301, GS4D_SRC_ALPHA = 0x0302, GS4D_ONE_MINUS_SRC_ALPHA = 0x0303,
       GS4D_DST_ALPHA = 0x0304, GS4D_ONE_MINUS_DST_ALPHA = 0x0305, GS4D_DST_COLOR = 0x0306, GS4D_ONE_MINUS_DST_COLOR = 0x0307,
       GS4D_CONSTANT_COLOR = 0x8001, GS4D_ONE_MINUS_CONSTANT_COLOR = 0x8002, GS4D_CONSTANT_ALPHA = 0x8003, GS4D_ONE_MINUS_CONSTANT_ALPHA = 0x8004 };

/* Per-stage device timings of the most recent calls, measured with HIP events on the context's stream. */
enum { GS4D_T_KEYGEN = 0, GS4D_T_SORT = 1, GS4D_T_PREPROCESS = 2, GS4D_T_BINNING = 3, GS4D_T_PAIRSORT = 4, GS4D_T_COMPOSITE = 5, GS4D_T_COUNT = 6 };

/* ---- context (stands in for the GL context + default framebuffer; Application.cpp:89-97, glViewport :69) ---- */
GS4D_API int  gs4d_create(int device, int width, int height, gs4d_ctx** out);
GS4D_API void gs4d_destroy(gs4d_ctx* ctx);
GS4D_API int  gs4d_resize(gs4d_ctx* ctx, int width, int height);                 /* glViewport / Camera::Resize            */
GS4D_API const char* gs4d_last_error(gs4d_ctx* ctx);                             /* ctx may be NULL: error of a failed create */

/* ---- buffers: glGenBuffers+glBufferData / glBufferStorage (ShareStorageBuffer.cpp:3-8, Scenes.h:241-247),
 *      glBufferSubData (ShareStorageBuffer.cpp:30-40, Scenes.h:321-325), glDeleteBuffers (ShareStorageBuffer.cpp:10-13) ---- */
GS4D_API int gs4d_buffer_create(gs4d_ctx* ctx, const void* data /* may be NULL */, size_t bytes, gs4d_buf* out);
GS4D_API int gs4d_buffer_subdata(gs4d_ctx* ctx, gs4d_buf buf, size_t offset, const void* data, size_t bytes);
GS4D_API int gs4d_buffer_read(gs4d_ctx* ctx, gs4d_buf buf, size_t offset, void* out, size_t bytes);  /* blocking; no reference counterpart (tests/tools) */
GS4D_API int gs4d_buffer_destroy(gs4d_ctx* ctx, gs4d_buf buf);
GS4D_API int gs4d_buffer_device_ptr(gs4d_ctx* ctx, gs4d_buf buf, void** dptr, size_t* bytes);        /* zero-copy interop with a caller that owns HIP memory */
/* The caller is about to overwrite `buf` through that pointer with work on its own stream (gs4d_set_stream).  Call this BEFORE queueing
 * the write, every time: (a) the caller's stream is made to wait for every kernel the library has queued that still uses the buffer
 * (without a caller stream the call blocks until they have finished), (b) the contents count as changed from here on — the library keeps
 * derived data per buffer version (a repacked copy of the records, bounds of the sort keys, what a sorted index was sorted by) and
 * otherwise goes on using it.  The library's next call that uses the buffer is ordered after the caller's stream as gs4d_set_stream says. */
GS4D_API int gs4d_buffer_invalidate(gs4d_ctx* ctx, gs4d_buf buf);
/* glBindBufferBase(GL_SHADER_STORAGE_BUFFER, slot, buf) (Scenes.h:336, ShareStorageBuffer.cpp:20-23); slots 0..7 */
GS4D_API int gs4d_bind_storage(gs4d_ctx* ctx, int slot, gs4d_buf buf);

/* ---- pipeline state: Shader::Bind / SetUniform1f / SetUniformMat4f (Shader.cpp:171-174, 206-209), glClearColor
 *      (Application.cpp:125), glBlendFunc (Application.cpp:150), Renderer::Clear (Renderer.cpp:20-23) ---- */
GS4D_API int gs4d_set_mode(gs4d_ctx* ctx, int mode);
GS4D_API int gs4d_set_uniform_1f(gs4d_ctx* ctx, int id, float v);
GS4D_API int gs4d_set_uniform_mat4(gs4d_ctx* ctx, int id, const float m[16]);
GS4D_API int gs4d_set_clear_color(gs4d_ctx* ctx, const float rgba[4]);
/* glBlendFunc(sfactor, dfactor) (Application.cpp:150): equation FUNC_ADD on all four channels, result clamped to [0, 1].  Default
 * (SRC_ALPHA, ONE_MINUS_SRC_ALPHA).  The blend colour is (0, 0, 0, 0) as in the reference (no glBlendColor): CONSTANT_* act as ZERO,
 * ONE_MINUS_CONSTANT_* as ONE.  Any other value: GS4D_E_INVALID (GL_INVALID_ENUM).  Draws with a function other than the default take
 * the instance-ordered tile lists and blend them in draw order. */
GS4D_API int gs4d_set_blend(gs4d_ctx* ctx, int src_factor, int dst_factor);
GS4D_API int gs4d_clear(gs4d_ctx* ctx);

/* ---- ordering ---- */
/* radix_sort::sorter::sort(key_buf, val_buf, n) (radix_sort.hpp:258-392): stable ascending sort of n (uint32 key, uint32 value)
 * pairs, in place.  Output == std::stable_sort by key; n <= 1 is a no-op (radix_sort.hpp:260). */
GS4D_API int gs4d_sort_pairs(gs4d_ctx* ctx, gs4d_buf keys, gs4d_buf vals, size_t n);
/* GPU replacement for the CPU key loop + two glBufferSubData uploads (Scenes.h:314-325): writes keys_f32[i] and idx_u32[i] = i
 * for the n 96-byte SplatData records in `data`. */
GS4D_API int gs4d_keygen(gs4d_ctx* ctx, gs4d_buf data, float t, const float cam_pos[3], gs4d_buf keys_f32, gs4d_buf idx_u32, size_t n, int key_mode);

/* ---- draw: Renderer::Draw(va, ib, instances) -> glDrawElementsInstanced(GL_TRIANGLES, 6, …, instances) (Renderer.cpp:33-39)
 *      with the state set above; blends `instances` quads into the framebuffer in instance order. ---- */
GS4D_API int gs4d_draw_instanced(gs4d_ctx* ctx, size_t instances);
/* Renderer::Draw(va, ib) -> glDrawElements on 4 vertices x 72 B per splat (Scenes.h:1690-1692): GS4D_MODE_3D_FULL */
GS4D_API int gs4d_draw_quads(gs4d_ctx* ctx, gs4d_buf vertices, size_t nquads);

/* Overlay lines: Renderer::DrawLine / DrawGrid / DrawAxis (Renderer.cpp:41-215) with the flat-colour programs under Shader/Lines.
 * nverts positions of `dims` floats each: dims == 3: gl_Position = viewproj * vec4(p, 1) (LineVert.GLSL:11); dims == 2: gl_Position =
 * vec4(p, 0, 1), i.e. NDC (Line2DVert.GLSL:11; viewproj may be NULL).  strip == 0: GL_LINES (vertices 2k, 2k+1), else GL_LINE_STRIP.
 * Segments are clipped to the view volume and rasterised as non-antialiased lines of `width` pixels (rounded, at least 1) — GL 4.4
 * section 14.5.2 — and every fragment is blended into the current image with the context's blend function, after what was drawn
 * before and before what is drawn next.  All fragments of one call carry the same colour. */
GS4D_API int gs4d_draw_lines(gs4d_ctx* ctx, const float* verts, size_t nverts, int dims, int strip, const float viewproj[16], const float rgba[4], float width);

/* ---- read-back (no reference counterpart: the reference never reads its framebuffer) ---- */
GS4D_API int gs4d_read_pixels(gs4d_ctx* ctx, float* rgba, size_t bytes);          /* blocking; bytes == width*height*16     */
GS4D_API int gs4d_read_pixels_device(gs4d_ctx* ctx, void* dptr, size_t bytes);    /* device-to-device, asynchronous: ordered into the caller's stream if one was given (gs4d_set_stream), else call gs4d_finish before using dptr */
/* Presentation format of the reference's window framebuffer (RGBA8 unorm, Application.cpp:89): clamp to [0,1], round to nearest.
 * Device-to-device, asynchronous like gs4d_read_pixels_device, width*height*4 bytes. */
GS4D_API int gs4d_read_pixels_rgba8_device(gs4d_ctx* ctx, void* dptr, size_t bytes);
/* The same for an image of the swap chain: frames_back 0 = the current image, 1 = the image the last gs4d_clear moved away from (the
 * previous frame), which stays intact until its lane comes round again.  An application that reads frame f-1 after queueing frame f
 * (clear, keygen, sort, draw) never waits for frame f: its host thread stays ahead of the device.  GS4D_E_INVALID when there is no such
 * image (frames_back > 1, one frame lane, or no gs4d_clear yet). */
GS4D_API int gs4d_read_frame_rgba8_device(gs4d_ctx* ctx, int frames_back, void* dptr, size_t bytes);
/* The same, for callers that cycle through several destination buffers (a double-buffered gather batch): the pack does NOT wait for
 * everything queued on the caller's stream — which would include the transfer still reading the OTHER buffer — but only for `hip_event`
 * (a hipEvent_t passed as void*, recorded by the caller behind the last work that used `dptr`; NULL: `dptr` is free, wait for nothing).
 * As with the call above, work the caller queues on its stream afterwards sees the pixels. */
GS4D_API int gs4d_read_frame_rgba8_device_after(gs4d_ctx* ctx, int frames_back, void* dptr, size_t bytes, void* hip_event);
/* Name the caller's HIP stream (hipStream_t passed as void*; NULL: none — note that the legacy default stream's handle IS NULL: give a
 * stream of your own).  The library keeps running on its own streams, but from now on
 *  (a) a buffer the caller rewrites on that stream (gs4d_buffer_device_ptr + gs4d_buffer_invalidate, in that call order, THEN the
 *      caller's writes) is not used by the library before those writes are done: the first call that uses the buffer after
 *      gs4d_buffer_invalidate records an event on the caller's stream and every frame lane waits for it before touching the buffer;
 *  (b) a device read-back waits for what the caller queued before it (the destination may still be read by, e.g., the RCCL send of the
 *      previous batch), and whatever the caller queues after it sees the pixels — e.g. an RCCL gather of the frames.
 * No host synchronisation.  Calls that hand nothing over (clear, uniforms, keygen / sort / draw on buffers the caller did not announce)
 * do not look at the caller's stream: frames keep overlapping across the lanes. */
GS4D_API int gs4d_set_stream(gs4d_ctx* ctx, void* hip_stream);
/* Single-frame sharding over several GPUs (secondary mode; config 5): rows of 8x8-pixel tiles are dealt round-robin,
 * tile row ty belongs to rank ty % world.  After gs4d_set_tile_shard(rank, world) a draw bins and composites only the context's own
 * tile rows (every rank still generates keys and sorts all splats: the blend order is global); the other rows of its image keep the
 * clear colour.  gs4d_read_band_rgba8_device packs the context's rows — band_rows pixel rows, its first tile row on top (bottom-up like
 * the framebuffer) — for a gather; bytes == band_rows * width * 4.  rank 0 / world 1 restores the default. */
GS4D_API int gs4d_set_tile_shard(gs4d_ctx* ctx, int rank, int world);
GS4D_API int gs4d_band_rows(gs4d_ctx* ctx, int* rows);
GS4D_API int gs4d_read_band_rgba8_device(gs4d_ctx* ctx, void* dptr, size_t bytes);
GS4D_API int gs4d_finish(gs4d_ctx* ctx);                                          /* blocks until every lane is idle; reports device-side check failures */

/* ---- aux outputs: per-pixel depth and opacity (no reference counterpart) ----
 * A frame cleared with aux outputs on keeps, beside its colour, one float2 {D, O} per pixel.  A draw with the default blend function
 * accumulates, with exactly the weights w_i = T_i * al_i of its colour, D_draw = sum w_i * d_i (d_i = -z_view of record i's centre, 0 for
 * GS4D_MODE_2D) and O_draw = 1 - T_final, and composes them over what the frame holds: D <- D_draw + T_final * D, O <- O_draw + T_final * O.
 * A clear gives (0, 0); overlay lines (gs4d_draw_lines) leave D and O as they are.  Expected depth = D / O where O > 0.  While a frame has
 * aux outputs, a draw with any other blend function returns GS4D_E_UNSUPPORTED and draws nothing. */
/* enable != 0: the frames cleared from the next gs4d_clear on have aux outputs; 0: they do not (every draw then behaves as without this
 * call).  The first enable allocates one W*H*8-byte plane per image of the swap chain (gs4d_resize reallocates them); nothing is allocated
 * while aux outputs have never been on. */
GS4D_API int gs4d_set_aux_outputs(gs4d_ctx* ctx, int enable);
/* Blocking; bytes == width*height*8: interleaved {D, O} per pixel, rows in gs4d_read_pixels' order (row 0 = bottom).  GS4D_E_INVALID when
 * the current frame was not cleared with aux outputs on. */
GS4D_API int gs4d_read_aux(gs4d_ctx* ctx, float* depth_opacity, size_t bytes);
/* The same, device-to-device and asynchronous, ordered as gs4d_read_pixels_device (into the caller's stream if one was given). */
GS4D_API int gs4d_read_aux_device(gs4d_ctx* ctx, void* dptr, size_t bytes);

/* ---- ID outputs: which splat record a pixel shows, for picking and selection (no reference counterpart) ----
 * A frame cleared with ID outputs on keeps, beside its colour, three values per pixel: the record that contributes most to the pixel's
 * final colour, the draw of the frame it came from, and its weight in that colour.  Default blend function only.  Within one draw, each
 * fragment has the weight w_j = T_j * al_j its colour accumulates with (T draw-local, from 1, front to back); the draw's candidate is the
 * fragment with the largest w_j > 0, the front-most on a tie.  With T_final the draw's final transmittance at the pixel, the draw then
 * composes its candidate over the stored {record, draw, weight} with the colour's "over":
 *     weight <- T_final * weight;  if a candidate exists and w_cand >= weight: {record, draw, weight} <- {rec_cand, draw ordinal, w_cand}.
 * record: the index into the data buffer of the record the fragment came from (GS4D_MODE_4D_SORTED: the sort index's entry, not the
 * instance; GS4D_MODE_4D_DIRECT, GS4D_MODE_2D: the instance; gs4d_draw_quads: the quad).  draw: 0 for the first gs4d_draw_instanced /
 * gs4d_draw_quads after gs4d_clear, 1 for the next, ...; overlay lines (gs4d_draw_lines) are no draw and leave the planes as they are.
 * A pixel no fragment has reached holds record = draw = 0xFFFFFFFF and weight 0.  A frame with ID outputs also has aux outputs
 * (gs4d_read_aux*), and a draw with any other blend function returns GS4D_E_UNSUPPORTED and draws nothing. */
/* enable != 0: the frames cleared from the next gs4d_clear on have ID (and aux) outputs; 0: they do not.  The first enable allocates three
 * W*H*4-byte planes (and the aux plane) per image of the swap chain (gs4d_resize reallocates them); nothing is allocated while ID outputs
 * have never been on. */
GS4D_API int gs4d_set_id_outputs(gs4d_ctx* ctx, int enable);
/* Blocking: the w x h rectangle at (x, y) into w*h-element arrays, rows in gs4d_read_pixels' order (row 0 = bottom; element [r * w + c] is
 * pixel (x + c, y + r)).  Any output pointer may be NULL.  A 1x1 read is a pick.  GS4D_E_INVALID for a rectangle not inside the image, or
 * when the current frame was not cleared with ID outputs on. */
GS4D_API int gs4d_read_ids(gs4d_ctx* ctx, int x, int y, int w, int h, uint32_t* record, uint32_t* draw, float* weight);
/* The full planes (bytes_per_plane == width*height*4 each; NULL skips a plane, not all three), device-to-device and asynchronous, ordered as
 * gs4d_read_aux_device. */
GS4D_API int gs4d_read_ids_device(gs4d_ctx* ctx, void* record, void* draw, void* weight, size_t bytes_per_plane);

/* ---- depth test against the caller's depth plane: splats among opaque geometry (no reference counterpart) ----
 * What a GL application gets with glEnable(GL_DEPTH_TEST), glDepthFunc(GL_LESS), glDepthMask(GL_FALSE) when it draws the splats after its
 * opaque meshes.  The plane is a buffer of W*H float32 view depths Z[y*W + x], rows in gs4d_read_pixels' order (row 0 = bottom), in the unit
 * of the aux outputs: -z_view, positive in front of the camera (a frame's D/O, or a mesh renderer's linear depth); +inf = no geometry.
 * A fragment of record i at pixel p is blended only if d_i < Z[p] in float32 (GL_LESS: a NaN hides everything at its pixel), where d_i is
 * the record depth the aux outputs use (slot 15 of gs4d_debug_read_projected; 0 for GS4D_MODE_2D).  A fragment that fails is treated like
 * a discarded one: the colour and transmittance stay as they are, its aux weight is 0 and it never becomes the ID candidate.  The plane is
 * read when the draw runs, in call order: a later gs4d_buffer_subdata does not change an earlier draw; writes through
 * gs4d_buffer_device_ptr follow the gs4d_buffer_invalidate contract.  gs4d_draw_lines ignores the test. */
/* plane != 0: the gs4d_draw_instanced / gs4d_draw_quads calls issued from now on test against it (draw state like gs4d_set_blend: it survives
 * gs4d_clear); 0: no test (the default).  A name that is not a live buffer: GS4D_E_INVALID, the state stays as it was.  gs4d_buffer_destroy
 * of the plane turns the test off.  A draw issued while the plane holds fewer than width*height*4 bytes (e.g. after gs4d_resize) returns
 * GS4D_E_INVALID, and one with a blend function other than the default GS4D_E_UNSUPPORTED; neither draws anything. */
GS4D_API int gs4d_set_depth_test(gs4d_ctx* ctx, gs4d_buf plane);

/* ---- record statistics: what each record contributed to the picture (no reference counterpart) ----
 * The ID outputs keep one record per pixel; this is the opposite question.  Within one draw a fragment of record i at pixel p enters the
 * colour with the weight w = T * al (T draw-local, from 1, front to back; al after the 1e-4 discard and the clamp).  Every fragment with
 * w > 0 at a pixel inside the image counts for its record:
 *     pixels += 1;   wmax = max(wmax, w)  (as float32 bit patterns: w >= 0, so unsigned order is float order);
 *     wsum += q(w),  q(w) = (uint32) rint(w * 2^24) in float32, round to nearest even — wsum is in units of 2^-24.
 * Behind a pixel whose T has reached exactly 0 every w is 0 and nothing counts.  A tile-row shard (gs4d_set_tile_shard) counts its own tile
 * rows only.  The record index is the one the ID outputs use (GS4D_MODE_4D_SORTED: the sort index's entry; GS4D_MODE_4D_DIRECT, GS4D_MODE_2D:
 * the instance; gs4d_draw_quads: the quad).  All three fields are integers accumulated with atomics: the result does not depend on the order of
 * anything, and it adds up across tiles, draws, frames, frame lanes and shards (pixels and wsum by +, wmax by max).  A draw the library has
 * to run again (a tile-list capacity or a staged guess that did not fit) counts once: an attempt that aborts on the device adds nothing. */
typedef struct gs4d_record_stat {
    uint32_t pixels;   /* (pixel, draw) pairs in which the record had a fragment with w > 0 */
    uint32_t wmax;     /* bit pattern of the largest such w (float32)                       */
    uint64_t wsum;     /* sum of q(w) over those fragments, units of 2^-24                  */
} gs4d_record_stat;
/* stats != 0: every gs4d_draw_instanced / gs4d_draw_quads issued from now on ADDS its statistics into the buffer, an array of nrecords
 * gs4d_record_stat (draw state like gs4d_set_depth_test: it survives gs4d_clear).  Nothing ever zeroes the buffer: upload zeros
 * (gs4d_buffer_subdata) where a new count should start.  0: off (the default).  A name that is not a live buffer, or a buffer of fewer than
 * nrecords * 16 bytes: GS4D_E_INVALID, the state stays as it was.  gs4d_buffer_destroy of the buffer turns the statistics off.  A list entry
 * whose record index is >= nrecords is skipped on the device (it is still drawn).  gs4d_draw_lines never counts.
 * The buffer is an ordinary buffer: gs4d_buffer_read, gs4d_buffer_subdata and gs4d_buffer_invalidate on it are ordered after every draw issued
 * before them, on every frame lane (re-runs included); draws on different lanes accumulate concurrently.
 * Out of scope, though meaningful — such a draw returns GS4D_E_UNSUPPORTED and draws nothing: statistics with a blend function other than the
 * default, into a frame cleared with aux or ID outputs, or with a depth test set. */
GS4D_API int gs4d_set_record_stats(gs4d_ctx* ctx, gs4d_buf stats, size_t nrecords);

/* ---- compaction: prune a record set by its record statistics, on the device (no reference counterpart) ----
 * A stable, order-preserving stream compaction.  Record i (0 <= i < n) has the statistics row stats[i] and the `stride` bytes at src + i*stride.
 * It is KEPT iff (pixels >= min_pixels && wmax >= min_wmax && wsum >= min_wsum) != invert: {1, 0, 0, 0} is the visible set, {1, bits(1/255f), 0, 0}
 * drops what never reached one 8-bit step of any pixel.  The kept records appear in dst in ascending i: record i goes to slot rank(i), the number
 * of kept records before it, so time-ordered or spatially ordered uploads stay so; if kept_index != 0, kept_index[rank(i)] = i (uint32).  `count`
 * always receives a gs4d_compact_count at offset 0: kept = the true number of kept records; written = min(kept, capacity), where capacity =
 * min(dst bytes / stride, kept_index bytes / 4) over the outputs that are given (no outputs: written = kept).  Slots >= capacity are never
 * written — no byte outside a buffer is touched, whatever the table holds — and bytes of dst / kept_index beyond `written` slots keep their
 * contents: a caller that sees kept > written allocates and calls again.  dst == 0 && src == 0: index list and count only; dst == 0 &&
 * kept_index == 0: count only.  stride: a multiple of 16, 16 .. 1024 (96: SplatData, 48: GS4D_MODE_2D records, 288: the four 72-byte vertices of
 * a quad, 16: a statistics table itself).  n == 0 writes {0, 0}.
 * GS4D_E_INVALID, with nothing queued and nothing written: n > 0xFFFFFFFF; a bad stride; a name that is not a live buffer; a buffer too small for n
 * rows, n records or the 8-byte count; dst without src; any two of the named buffers being the same buffer; rule == NULL, reserved != 0 or an
 * unknown flag.
 * Ordering: the table is taken as gs4d_buffer_read takes it — every draw issued before the call, on every frame lane, has been settled (re-runs
 * included) — and a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first.  The kernels are then queued on the
 * current frame lane and the call returns without waiting for them, like gs4d_sort_pairs; dst, kept_index and count are ordinary buffers
 * afterwards (gs4d_keygen, gs4d_sort_pairs, draws, gs4d_buffer_read and other lanes order themselves behind the call; what the library derives
 * from dst's contents is rebuilt).  The result is that of the table as it stands at the call: a draw issued afterwards that adds to the same
 * table — statistics left on, the next frame on the next lane — waits on the device until the call's kernels have read it, and a host write
 * (gs4d_buffer_subdata) waits as it does for any reader.  gs4d_buffer_invalidate hand-offs of any of the buffers are honoured. */
enum { GS4D_KEEP_INVERT = 1 };            /* keep exactly the records the rule would drop */
typedef struct gs4d_keep_rule {
    uint32_t min_pixels;   /* keep needs stat.pixels >= min_pixels                                  */
    uint32_t min_wmax;     /* ... and stat.wmax >= min_wmax, as uint32 bit patterns (float order)   */
    uint64_t min_wsum;     /* ... and stat.wsum >= min_wsum (units of 2^-24)                         */
    uint32_t flags;        /* 0 or GS4D_KEEP_INVERT; any other bit: GS4D_E_INVALID                   */
    uint32_t reserved;     /* must be 0                                                              */
} gs4d_keep_rule;
typedef struct gs4d_compact_count { uint32_t kept, written; } gs4d_compact_count;
GS4D_API int gs4d_compact_records(gs4d_ctx* ctx, gs4d_buf stats, size_t n, const gs4d_keep_rule* rule,
                                  gs4d_buf src, size_t stride, gs4d_buf dst, gs4d_buf kept_index, gs4d_buf count);

/* ---- to a budget: the threshold of one statistics field that keeps the k records that matter most (no reference counterpart) ----
 * A k-th-largest selection over one field of the table, on the device: no sort, no permutation — the compaction that follows stays stable.
 * f[i] is the chosen field of row i of the n rows of gs4d_record_stat in `stats`, as a uint64: GS4D_STAT_PIXELS and GS4D_STAT_WMAX are the
 * uint32 zero-extended (wmax as its bit pattern, which is in float order: w >= 0), GS4D_STAT_WSUM is the uint64.  With k = min(budget, n):
 *     value = the k-th largest of f[0 .. n), counted with multiplicity (the value at position k - 1 of f sorted in descending order);
 *     above = #{i : f[i] >  value}, which is < k;
 *     equal = #{i : f[i] == value}, and above + equal >= k.
 * n == 0 writes {0, 0, 0}.  `out` receives the 16 bytes of a gs4d_cut at offset 0; no other byte of any buffer is written.
 * What the caller does with it: a gs4d_keep_rule whose threshold for the field is `value` (the other two 0) keeps above + equal records — at
 * least k, exactly k when there is no tie at the cut — and one whose threshold is value + 1 keeps `above` records, fewer than k (value at the
 * field's maximum: above = 0, nothing to keep); in both cases `kept` is known without a count-only compaction pass.
 * GS4D_E_INVALID, with nothing queued and nothing written: n > 0xFFFFFFFF; budget == 0; a field other than the three; a name that is not a live
 * buffer; stats == out; stats smaller than 16 n bytes; out smaller than 16 bytes.
 * Ordering: exactly that of gs4d_compact_records.  The table is taken as gs4d_buffer_read takes it — every draw issued before the call, on every
 * frame lane, has been settled (re-runs included) — and a queued gs4d_keygen / gs4d_sort_pairs that names one of the two buffers is launched
 * first.  The kernels are then queued on the current frame lane, the call returns without waiting for them and starts no new frame; `out` is an
 * ordinary written buffer afterwards (gs4d_buffer_read of it waits for the kernels).  The result is that of the table as it stands at the call: a
 * draw issued afterwards that adds to the same table, on any lane, waits on the device until the call's kernels have read it, and a host write
 * (gs4d_buffer_subdata) waits as it does for any reader.  All sums are sums of integers: the result does not depend on the order of anything. */
enum { GS4D_STAT_PIXELS = 0, GS4D_STAT_WMAX = 1, GS4D_STAT_WSUM = 2 };
typedef struct gs4d_cut {
    uint64_t value;    /* the k-th largest value of the field (a uint32 field zero-extended) */
    uint32_t above;    /* rows whose field is greater than value: < k                       */
    uint32_t equal;    /* rows whose field equals value: above + equal >= k                 */
} gs4d_cut;
GS4D_API int gs4d_stat_cut(gs4d_ctx* ctx, gs4d_buf stats, size_t n, int field, size_t budget, gs4d_buf out);

/* ---- selection: a statistics table from a region of the ID planes (no reference counterpart) ----
 * "What do I see in this region of this frame?", answered on the device as rows of an ordinary gs4d_record_stat table — so that everything
 * that consumes such a table works on a selection unchanged: gs4d_compact_records with {1, 0, 0, 0} builds the selected set, its stable
 * kept_index and its count; gs4d_stat_cut gives "the k most visible records of the region"; repeated calls add up into union selections.
 * The call reads the planes {record, draw, weight} of the current frame, the ones gs4d_read_ids reads.  Pixel p = (x + c, y + r) of the
 * rectangle (0 <= c < w, 0 <= r < h, row 0 = bottom) TAKES PART iff
 *     record[p] != GS4D_ID_NONE  &&  record[p] < nrecords  &&  draw_first <= draw[p] <= draw_last  &&  bits(weight[p]) >= min_weight
 *     && (mask == 0 || mask[r * w + c] != 0)
 * where bits() is the weight's uint32 bit pattern (float order: w >= 0) and the mask is one byte per pixel of the rectangle, rows bottom-up,
 * at least w*h bytes, any non-zero byte counting: a lasso is the rectangle around it and a mask.  Every pixel that takes part adds to row
 * record[p] of `stats` exactly as one fragment of weight w = weight[p] adds in a draw with record statistics:
 *     pixels += 1;   wmax = max(wmax, bits(w));   wsum += q(w),  the q of gs4d_record_stat.
 * The call ADDS: nothing zeroes the table, and no byte outside rows [0, nrecords) is written, whatever the planes hold.  All three fields are
 * integers: the result does not depend on the order of anything, and a table filled by several calls is the sum of the calls (pixels and wsum
 * by +, wmax by max) — across rectangles, frames and tile-row shards (a sharded context's foreign rows hold the sentinel and count nothing),
 * and on top of what draws have added to the same table.  region == NULL: the whole image, every draw, every weight.  nrecords == 0, with
 * arguments that are otherwise valid, is a no-op: nothing is queued.  Not covered: the image the last gs4d_clear moved away from (frames_back 1 of gs4d_read_frame_*), and what lies behind the record a
 * pixel shows — the planes keep one record per pixel; everything that contributes is a draw with gs4d_set_record_stats.
 * GS4D_E_INVALID, with nothing queued and nothing written: the current frame was not cleared with ID outputs on; a rectangle that is empty or
 * not inside the image; draw_first > draw_last; reserved != 0; nrecords > 0xFFFFFFFF; stats not a live buffer, or smaller than nrecords * 16
 * bytes; mask neither 0 nor a live buffer, or smaller than w*h bytes; mask == stats.
 * Ordering.  The planes are taken as gs4d_read_ids_device takes them: a queued gs4d_keygen / gs4d_sort_pairs is launched first, the frame's
 * draws are settled (re-runs included), lazily clear tiles are materialised; the kernel is then queued on the current frame lane, and the
 * call returns at once and starts no new frame.  A later draw into the same frame, or a later gs4d_clear that brings this image round again,
 * does not change the result.  `stats` is a buffer the call writes with a kernel while keeping its contents: draws that add to it
 * (gs4d_set_record_stats) and were issued before the call, on every frame lane, are settled first, as for gs4d_compact_records; draws issued
 * afterwards, other lanes, the record-set calls and host accesses order themselves behind the call.  `mask` is a buffer the call reads: a
 * later gs4d_buffer_subdata of it waits as it does for any reader.  gs4d_buffer_invalidate hand-offs of both buffers are honoured. */
#define GS4D_ID_NONE 0xFFFFFFFFu          /* the record and draw of a pixel no fragment has reached */
typedef struct gs4d_id_region {
    int32_t  x, y, w, h;             /* rectangle inside the image, row 0 = bottom, as gs4d_read_ids                     */
    uint32_t draw_first, draw_last;  /* a pixel takes part iff draw_first <= its draw ordinal <= draw_last                */
    uint32_t min_weight;             /* ... and its weight, as a uint32 bit pattern, is >= min_weight (0: every weight)   */
    uint32_t reserved;               /* must be 0                                                                         */
} gs4d_id_region;                    /* 32 bytes */
GS4D_API int gs4d_count_ids(gs4d_ctx* ctx, const gs4d_id_region* region /* NULL: whole image, every draw, every weight */,
                            gs4d_buf mask /* 0: none */, gs4d_buf stats, size_t nrecords);

/* ---- time windows: the records of a 4D set that can show anything between two times (no reference counterpart) ----
 * A 4D draw gives record i the opacity ot = max(expf(arg(uTime)), uMinOpacity) and the alpha ot * colour.a, with
 *     arg(t) = ((-0.5f * dt) * (1.0f / s44)) * dt,  dt = t - mu_t     (float32, round to nearest, no contraction: the draw's own operations)
 * where mu_t = float 3, colour.a = float 7 and s44 = float 23 of the 96-byte SplatData record.  Far from mu_t the exponential is exactly 0, and
 * with it the alpha: no float32 exponential is non-zero below GS4D_TIME_DEAD_ARG (e^-106 is 0.13 x half the smallest denormal).  Such a record
 * is still keyed, sorted, projected, binned and blended — with the default blend function as an exact no-op (C += 0, T *= 1, weight 0).
 * gs4d_record_time_spans writes, for each of the n records of `data`, the closed interval of float32 times OUTSIDE which it provably contributes
 * nothing — one gs4d_time_span per record at spans[i], once per upload:
 *     never  {+inf, -inf}: !(colour.a > 0) — the alpha is <= 0 (clamped to 0 when blended) or not finite (the record is invalid) at every time;
 *     always {-inf, +inf}: min_opacity > 0 or NaN (the floor keeps ot > 0), s44 not finite or not positive, 1.0f / s44 not finite (s44 below
 *                          2^-128), mu_t not finite — the conservative answer for hostile records;
 *     otherwise t_last = the largest and t_first = the smallest finite float32 t with arg(t) >= GS4D_TIME_DEAD_ARG.  arg is monotone non-increasing
 *                          in |t - mu_t| and arg(mu_t) = 0: both ends are found by bisection over the ordered bit patterns of t, exactly.
 * GS4D_E_INVALID, nothing queued: n > 0xFFFFFFFF, a name that is not a live buffer, data == spans, data smaller than n * 96 bytes or spans smaller
 * than n * 8.  n == 0 is a no-op.  Ordering as gs4d_compact_records: queued on the current frame lane, the call returns at once; `spans` is an
 * ordinary buffer that the call writes, `data` one that it reads.
 *
 * gs4d_compact_time_window keeps record i iff its span meets the window: t_first <= t1 && t_last >= t0.  EVERYTHING else is gs4d_compact_records
 * with `spans` in the place of `stats`: the stable order, kept_index, gs4d_compact_count {kept, written}, the capacity clamp (no byte outside a
 * buffer is touched, whatever the table holds), the stride rules, the count-only and index-only forms, the distinct-buffer rule, GS4D_E_INVALID
 * with nothing queued and nothing written — additionally when t0 or t1 is NaN or t0 > t1 (infinite ends are allowed) or spans holds fewer than
 * n * 8 bytes — and the ordering (a table needs no draws settled: it is a buffer the call reads).
 *
 * The guarantee.  With the default blend function, uMinOpacity equal to the min_opacity the spans were computed with, any finite uTime in
 * [t0, t1], and GS4D_MODE_4D_SORTED after gs4d_keygen + gs4d_sort_pairs (of the respective set) or GS4D_MODE_4D_DIRECT: a draw of the compacted
 * set gives the same bits as a draw of the full set in the colour image, the aux planes, the ID planes (record indices mapped through kept_index)
 * and the record statistics (rows mapped through kept_index; the rows of the full set that were dropped are zero).  Nothing is promised for any
 * other blend function: there a fragment of alpha 0 can change the destination (e.g. (ONE, ONE) adds its colour). */
#define GS4D_TIME_DEAD_ARG (-106.0f)
typedef struct gs4d_time_span { float t_first, t_last; } gs4d_time_span;
GS4D_API int gs4d_record_time_spans(gs4d_ctx* ctx, gs4d_buf data, size_t n, float min_opacity, gs4d_buf spans);
GS4D_API int gs4d_compact_time_window(gs4d_ctx* ctx, gs4d_buf spans, size_t n, float t0, float t1,
                                      gs4d_buf src, size_t stride, gs4d_buf dst, gs4d_buf kept_index, gs4d_buf count);

/* ---- spatial order: a record set reordered so that neighbours in space are neighbours in memory (no reference counterpart) ----
 * The draws gather projected records per tile: a set uploaded in Morton order of its positions draws faster than the same set in random order
 * (12 % at 10^7 splats), and the compactions above keep such an order.  Two explicit calls, once per upload:
 * gs4d_spatial_order computes the permutation, gs4d_gather_records applies it — or any other index list — to the records and to every table that
 * has a row per record (time spans, statistics rows, the caller's own attributes).
 *
 * gs4d_spatial_order: order_index[j] = the record that comes j-th in spatial order (uint32), j < n.  All arithmetic is float32, round to
 * nearest, no contraction, correctly rounded division.  The position p of record i is the three floats at src + i*stride + pos_offset
 * (SplatData: 0; the four 72-byte vertices of a quad: 0, its first vertex).
 *     placed    record i is PLACED iff p[0], p[1] and p[2] are all finite; any other record is UNPLACED;
 *     box       lo[a] / hi[a] = the smallest / largest p[a] over the placed records, a = 0, 1, 2;
 *     cell      of a placed record: d = p[a] - lo[a], e = hi[a] - lo[a], g = (d / e) * 1023.0f, cell[a] = g >= 0 ? (uint32) min(g, 1023.0f) : 0 — a NaN
 *               gives 0, so a degenerate axis (e == 0: 0 / 0) and a box whose extent overflows (e == inf) need no special case; the sign of a
 *               zero lo or hi cannot change a cell;
 *     key       placed: the 30-bit Morton code of the cell — bit k of cell[0] at bit 3k, of cell[1] at 3k + 1, of cell[2] at 3k + 2; unplaced:
 *               0x40000000, so these records come last;
 *     order     order_index = the stable ascending sort of 0 .. n-1 by key: records of equal key keep the caller's order, and nothing depends
 *               on the order in which anything runs on the device.
 * GS4D_E_INVALID, with nothing queued and nothing written: n > 0xFFFFFFFF (and n == 0xFFFFFFFF: the sort takes 2^32 - 2 elements at most); a stride
 * that is not a multiple of 16 in 16 .. 1024; pos_offset % 4 != 0 or pos_offset + 12 > stride; a name that is not a live buffer; src ==
 * order_index; src smaller than n * stride bytes or order_index smaller than 4n.  n == 0 is a no-op.
 *
 * gs4d_gather_records: slot j of dst (the `stride` bytes at dst + j*stride) <- the `stride` bytes of src record index[j], j < m; src holds nsrc
 * records.  An entry index[j] >= nsrc leaves slot j as it is; no byte outside any buffer is read or written, whatever the list holds; entries may
 * repeat.  With the order_index above it reorders a set; with the kept_index of a compaction it carries a side table along.  stride: a multiple of
 * 16, 16 .. 1024, as everywhere — or 4 or 8, the rows of a table of words (an index list) or of gs4d_time_span.
 * GS4D_E_INVALID, nothing queued, nothing written: m or nsrc > 0xFFFFFFFF; any other stride; a name that is not a live buffer; any two of the three
 * buffers being the same buffer; index smaller than 4m bytes, src smaller than nsrc * stride or dst smaller than m * stride.  m == 0 is a no-op.
 *
 * Ordering of both, as gs4d_compact_time_window: a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first; the
 * kernels are queued on the current frame lane and the call returns at once; src and index are buffers the call reads, order_index and dst
 * ordinary buffers it writes (draws that may still need them are settled first; later calls, other lanes and the host order themselves behind
 * it; what the library derives from dst's contents is rebuilt).  gs4d_buffer_invalidate hand-offs of any of the buffers are honoured.
 *
 * The guarantee.  With the default blend function and GS4D_MODE_4D_SORTED after gs4d_keygen + gs4d_sort_pairs (of the respective set): if no two
 * records of the set have the same depth key, a draw of the set gathered through order_index gives the same bits as a draw of the original set
 * in the colour image, the aux planes, the ID planes (record r of the gathered set is record order_index[r] of the original) and the record
 * statistics (row r of the gathered set's table equals row order_index[r] of the original's).  Records of EQUAL depth key blend in buffer order,
 * which a reorder may swap: the picture then stays within the checker's tolerance but is not promised bit-equal.  GS4D_MODE_4D_DIRECT,
 * GS4D_MODE_2D and gs4d_draw_quads blend in instance order: reordering their records changes the blend order and with it the picture. */
GS4D_API int gs4d_spatial_order(gs4d_ctx* ctx, gs4d_buf src, size_t n, size_t stride, size_t pos_offset, gs4d_buf order_index);
GS4D_API int gs4d_gather_records(gs4d_ctx* ctx, gs4d_buf index, size_t m, gs4d_buf src, size_t nsrc, size_t stride, gs4d_buf dst);

/* ---- view-dependent colour: a record's rgb from spherical harmonics, evaluated on the device (no reference counterpart) ----
 * Trained 3DGS-style sets store colour as spherical-harmonic (SH) coefficients per splat; the draws know the constant rgba at floats 4..7 of the
 * record.  gs4d_shade_sh evaluates degree 0..3 for a camera position and a time and writes floats 4, 5 and 6 (r, g, b) of each record i < n of the
 * 96-byte records in `data`.  Float 7 (alpha) and every other byte of the record stay as they are; no byte of data beyond record n - 1 is written;
 * no byte of sh is written.
 *
 * The table.  Row i is the sh_stride bytes at sh + i*sh_stride.  sh_stride: a multiple of 16, 16 .. 1024, as everywhere — so gs4d_gather_records
 * and both compactions carry a table along through kept_index / order_index unchanged — and sh_stride >= 12 (degree + 1)^2 (minimal rows: 16 / 48 /
 * 112 / 192 bytes for degree 0 / 1 / 2 / 3).  A row is float32, coefficient-major with the channels interleaved: c_k of channel ch is row[3k + ch],
 * k = 0 .. (degree + 1)^2 - 1, ch = 0, 1, 2 (r, g, b).  A lower degree reads a prefix of the same row: a degree-3 table shaded at degree 1 costs a
 * quarter of the traffic.  The row is read in 16-byte pieces: nothing past the 12 (degree + 1)^2 bytes, rounded up to 16, is ever read, and
 * nothing past the 12 (degree + 1)^2 bytes can change a result.
 *
 * The definition.  All arithmetic is float32, round to nearest, no contraction (every product and every sum below is rounded on its own, in the
 * order its parentheses give), with correctly rounded division and square root.  p = floats 0..2 of the record, mu_t = float 3, sig3 = floats
 * 20..22, s44 = float 23: the direction runs from the camera to the time-conditioned mean the draw projects (GS4D_KEY_VIEW_Z's mean, not the
 * reference's Euclidean key):
 *     k    = (1.0f / s44) * (t - mu_t)
 *     m    = p + (k * sig3)                              per component: one product, one sum
 *     d    = m - cam_pos
 *     len2 = ((d.x*d.x) + (d.y*d.y)) + (d.z*d.z)
 *     inv  = 1.0f / sqrtf(len2)
 *     x = d.x*inv,  y = d.y*inv,  z = d.z*inv
 * If !(len2 > 0) or len2 is not finite — a NaN or Inf position, s44 == 0, a camera on the mean — the record is DC-ONLY: the sum below stops after
 * k = 0.  The basis, with the constants and signs of the 3DGS reference implementation (computeColorFromSH), each constant rounded to float32:
 *     C0 = 0.28209479177387814   C1 = 0.4886025119029199
 *     C2 = { 1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396 }
 *     C3 = { -0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
 *            -0.5900435899266435 }
 *     xx = x*x, yy = y*y, zz = z*z, xy = x*y, yz = y*z, xz = x*z
 *     b_0  = C0
 *     b_1  = (-C1)*y             b_2  = C1*z                               b_3  = (-C1)*x
 *     b_4  = C2[0]*xy            b_5  = C2[1]*yz                           b_6  = C2[2]*(((2.0f*zz) - xx) - yy)
 *     b_7  = C2[3]*xz            b_8  = C2[4]*(xx - yy)
 *     b_9  = (C3[0]*y)*((3.0f*xx) - yy)                                    b_10 = (C3[1]*xy)*z
 *     b_11 = (C3[2]*y)*(((4.0f*zz) - xx) - yy)                             b_12 = (C3[3]*z)*(((2.0f*zz) - (3.0f*xx)) - (3.0f*yy))
 *     b_13 = (C3[4]*x)*(((4.0f*zz) - xx) - yy)                             b_14 = (C3[5]*z)*(xx - yy)
 *     b_15 = (C3[6]*x)*(xx - (3.0f*yy))
 * and the colour, per channel:
 *     acc = b_0*c_0
 *     for k = 1 .. (degree + 1)^2 - 1 (DC-only: none):   acc = acc + (b_k*c_k)
 *     v = acc + 0.5f
 *     colour = v > 0 ? v : 0                             a NaN gives 0; +inf stays (the draws treat out-of-range colours as data)
 * Nothing depends on the order in which anything runs on the device: the same inputs give the same bits.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: n > 0xFFFFFFFF; degree outside 0 .. 3; an sh_stride that is not a multiple of 16 in
 * 16 .. 1024 or is smaller than 12 (degree + 1)^2; cam_pos == NULL; a name that is not a live buffer; data == sh; data smaller than 96 n bytes or
 * sh smaller than n * sh_stride.  n == 0 is a no-op.  t and cam_pos may be non-finite: they are data, and the DC-only rule applies.
 *
 * Ordering, as gs4d_gather_records: a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first; draws that may still
 * have to be run again from data are settled; the kernel is queued on the current frame lane, the call returns at once and starts no new frame;
 * sh is a buffer the call reads, data one it writes (it waits, on the device, for the lanes whose draws or key generation still read data or its
 * shadow; later calls, other lanes and the host order themselves behind it).  gs4d_buffer_invalidate hand-offs of both buffers are honoured.
 *
 * What the write keeps.  Any other write to a record buffer makes the library rebuild what it derives from the contents at the next draw: the SoA
 * shadow the draws and gs4d_keygen read, its layout choice, the bounding box and the key bounds — a blocking repack of the whole set.  None of those
 * reads a colour, so gs4d_shade_sh is a COLOUR-ONLY write: if the shadow was current when the call was made, the same kernel writes the three floats
 * into the shadow's colour plane as well (its alpha is left alone) and the shadow stays current — the next draw neither repacks nor waits.  If the
 * shadow was not current (no draw or keygen since the last upload), only the records are written and the next draw builds the shadow, as it would
 * have anyway.  What is NOT kept is the provenance of a sort index: a draw whose gs4d_keygen + gs4d_sort_pairs ran BEFORE the shade no longer
 * takes its blend order from the keys but reads the sort index, which is correct but slower.  The call order per frame is therefore
 * shade -> gs4d_keygen -> gs4d_sort_pairs -> draw. */
GS4D_API int gs4d_shade_sh(gs4d_ctx* ctx, gs4d_buf data, size_t n, gs4d_buf sh, size_t sh_stride, int degree,
                           float t, const float cam_pos[3]);

/* ---- records from parameters: the 96-byte records of a splat set built on the device (Splat4D / Splat3D constructors, Splat.h:91-159, 334-344) ----
 * A caller whose splat parameters live on the device — an optimisation or animation loop, a trained 3DGS / 4DGS model, a simulation — gets its
 * SplatData records without a round trip over the host: gs4d_build_records writes record i < n of dst from row i of each parameter buffer.  All rows
 * are tightly packed float32, row i at i * row_bytes.  The call writes the first n 96-byte records of dst; it writes no other byte of dst and no byte
 * of any parameter buffer.
 *
 * The definition is the host code below ("host-side parameterisation"), which the fixtures pin.  All arithmetic is float32, round to nearest, no
 * contraction (every product and every sum is rounded on its own, in the order the host code gives), with correctly rounded division and square
 * root.  Matrix products are FULL products, the zeros of the scale matrices included (inf * 0 is a NaN, and a signed zero term decides the sign of a
 * zero sum).  The records have the bits of the host builders, except that a word that is a NaN on both sides may differ in sign and payload:
 *     GS4D_PARAMS_3D      record i of gs4d_host_build_records_3d(pos, rot, scale, rgba): Sigma3 = ((R S) S) R^T with R the matrix of the quaternion
 *                         as given (not normalised), each element ((a0*b0) + (a1*b1)) + (a2*b2); mu_t = 0, Sigma44 = 1, zeros in between;
 *     GS4D_PARAMS_4D_VEL  record i of gs4d_host_build_records_4d_tvar(pos, rot, scale, dir, tvar, rgba): gs4d_host_splat4d_cov from td = dir * sd
 *                         onwards with sd = tvar[i]: Sigma3 + (td td^T) * (1 / sd), td in row and column 3, Sigma44 = sd.  (lifetime, fade) -> sd is
 *                         gs4d_host_time_variance, on the host: it takes a double-precision logarithm;
 *     GS4D_PARAMS_4D_2Q   record i of gs4d_host_build_records_4d_2q(pos, rot, rot_r, scale, rgba): floats 8..23 = gs4d_host_splat4d_cov2q(rot[i],
 *                         rot_r[i], scale[i]): both quaternions normalised (a length <= 0 gives the identity), rot = L R, ((rot S) S^T) rot^T, each
 *                         element ((a0*b0 + a1*b1) + a2*b2) + a3*b3.
 * Nothing depends on the order in which anything runs on the device: the same inputs give the same bits.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: params == NULL; an unknown form; flags or reserved != 0; n > 0xFFFFFFFF; a buffer the form
 * needs that is not a live buffer; a buffer the form does not use that is not 0; any two of the named buffers (dst included) being the same buffer; a
 * parameter buffer smaller than n rows; dst smaller than 96 n bytes.  n == 0 with otherwise valid arguments is a no-op.
 *
 * Ordering, as gs4d_gather_records: a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first; draws that may still
 * have to be run again from dst are settled; the kernel is queued on the current frame lane, the call returns at once and starts no new frame; the
 * parameter buffers are buffers the call reads, dst one it writes (it waits, on the device, for the lanes whose draws or key generation still read
 * dst or its shadow; later calls, other lanes and the host order themselves behind it).  gs4d_buffer_invalidate hand-offs of all the buffers are
 * honoured: parameters written through gs4d_buffer_device_ptr on the caller's stream are read after those writes.
 * It is a full write of dst, like an upload: the buffer's version moves, what a sort index was sorted by is forgotten, and the next draw or
 * gs4d_keygen rebuilds the SoA shadow, its layout choice, the bounding box and the key bounds (gs4d_debug_shadow_builds goes up by one).  The call
 * order per frame is therefore build -> (gs4d_shade_sh) -> gs4d_keygen -> gs4d_sort_pairs -> draw. */
enum { GS4D_PARAMS_3D = 0, GS4D_PARAMS_4D_VEL = 1, GS4D_PARAMS_4D_2Q = 2 };
typedef struct gs4d_splat_params {
    uint32_t form;      /* GS4D_PARAMS_*                                                                 */
    uint32_t flags;     /* must be 0                                                                     */
    gs4d_buf pos;       /* 3D: 3 floats per record (x, y, z); 4D forms: 4 floats (x, y, z, mu_t)          */
    gs4d_buf rot;       /* 4 floats, w x y z (3D, 4D_VEL: the rotation; 4D_2Q: the left quaternion)       */
    gs4d_buf rot_r;     /* 4D_2Q: 4 floats, the right quaternion; other forms: must be 0                  */
    gs4d_buf scale;     /* 3D, 4D_VEL: 3 floats; 4D_2Q: 4 floats                                          */
    gs4d_buf rgba;      /* 4 floats, copied to floats 4..7 of the record                                  */
    gs4d_buf dir;       /* 4D_VEL: 3 floats; other forms: must be 0                                       */
    gs4d_buf tvar;      /* 4D_VEL: 1 float, the temporal variance (Sigma44); other forms: must be 0       */
    uint32_t reserved;  /* must be 0                                                                     */
} gs4d_splat_params;    /* 40 bytes */
GS4D_API int gs4d_build_records(gs4d_ctx* ctx, const gs4d_splat_params* params, size_t n, gs4d_buf dst);

/* ---- records back to parameters: the inverse of gs4d_build_records ----
 * A set that was merged, sliced, warped, posed or compacted on the device goes back to a trainer, a 3DGS / 4DGS file or another viewer as position,
 * quaternion, scales and colour: row i of every buffer named in *out is written from record src_first + i of src, i < n.  *out is read as the list
 * of DESTINATIONS, with the row sizes of gs4d_build_records.  Any destination may be 0, "not wanted" (only rot: normals — the last column of its
 * matrix is the shortest axis; only scale: a regulariser); at least one must be given; rot_r must be 0; dir and tvar must be 0 in the 3D form.
 * The call writes rows [0, n) of the named buffers and no other byte of any buffer; src is never written.
 *
 * The definition (gs4d_host_decompose_records is this text; csrc/decompose_record.h holds it once for the host and the kernel).  All arithmetic is
 * float32, round to nearest, no contraction, correctly rounded division and square root; only + - * / and the square root are used.
 *     GS4D_PARAMS_3D      pos = floats 0..2.  Sigma3 = the spatial block of the record, of which the LOWER triangle is read (floats 8, 9, 10, 13, 14,
 *                         18); the upper triangle, mu_t, the time row and column and Sigma44 are not looked at.  A 4D set whose CONDITIONAL
 *                         covariance at a time is meant goes through gs4d_slice_records first.
 *     GS4D_PARAMS_4D_VEL  pos = floats 0..3, tvar = Sigma44 (float 23), td = floats 20..22, dir = td / tvar (one division each), Sigma3 = the
 *                         lower triangle of the spatial block - (td_r * td_c) * (1 / tvar): the builder's own terms, subtracted.  Every 4x4
 *                         covariance with Sigma44 > 0 has this decomposition, so every 4D record — 2Q-built, merged, warped, posed — can be taken out
 *                         in this form.
 *     GS4D_PARAMS_4D_2Q   refused (it needs a 4x4 eigen-solve and the factoring of an SO(4) matrix into two quaternions).
 *     rgba                floats 4..7, bit copies.
 *     rot, scale          Sigma3 -> (q, s) with Sigma3 ~ ((R S) S) R^T, R the matrix of q, by a cyclic Jacobi eigen-solve of a fixed number of
 *                         sweeps over the pairs (0,1), (0,2), (1,2).  The canonical choice makes the outputs a function of the record: s holds the
 *                         standard deviations in descending order, ties keeping the lower original axis first; an eigenvalue that is negative or a
 *                         zero of either sign gives the scale +0; R's third column is the cross product of the first two (a proper rotation); q
 *                         (w x y z) is of unit length with w >= 0, and of the two quaternions with w == 0 (a zero of either sign, which is kept)
 *                         the one whose first non-zero component of x, y, z is positive.
 * Hostile records are data: a NaN, an Inf, 1e30, an indefinite Sigma3 or Sigma44 <= 0 give what this arithmetic gives, with no trap and no
 * device-side check.  The rows have the bits of the host function, except that a word that is a NaN on both sides may differ in sign and payload
 * (the rule of gs4d_build_records).  Anisotropy beyond what a float32 covariance resolves (variance ratios from about 2^24) comes back with a smallest
 * scale of 0: the record itself has lost the short axis.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: out == NULL; an unknown form or GS4D_PARAMS_4D_2Q; flags or reserved != 0; n, src_first
 * or src_first + n > 0xFFFFFFFF; no destination given; rot_r given, or dir or tvar given in the 3D form; a name that is not a live buffer; any two
 * of the named buffers (src included) being the same buffer; src smaller than src_first + n records; a destination smaller than n rows.  n == 0 with
 * otherwise valid arguments is a no-op.
 *
 * Ordering, as gs4d_build_records with the roles exchanged: src is a buffer the call reads — its 96-byte records, never its SoA shadow, which is
 * neither built nor invalidated (gs4d_debug_shadow_builds does not move) — and every destination one it writes.  The kernel is queued on the
 * current frame lane and the call returns at once.  gs4d_buffer_invalidate hand-offs are honoured in both directions: a destination handed to the
 * caller's stream with gs4d_buffer_device_ptr + gs4d_buffer_invalidate after the call holds the rows when read on that stream, with no host copy. */
GS4D_API int gs4d_decompose_records(gs4d_ctx* ctx, gs4d_buf src, size_t n, size_t src_first, const gs4d_splat_params* out);

/* ---- placing a record set: the records under a 4D affine map ----
 * A record carries a world-space mean and a 4x4 space-time covariance, and the draws have no model matrix.  gs4d_transform_records places a set
 * on the device: a Gaussian under x' = L x + o stays a Gaussian, with mean L mu + o and covariance L Sigma L^T, and with L a full 4x4 matrix one
 * call covers rotation, scale and translation; a time offset and a time scale (a clip played later, slower or faster); and a velocity column, which
 * makes a static object move.  The time conditioning of the draws then gives the right picture; no draw changes.
 *
 * xf is a buffer of m rows of gs4d_affine4 (80 bytes, a multiple of 16: gs4d_gather_records can carry a table of them; written through
 * gs4d_buffer_device_ptr + gs4d_buffer_invalidate the transforms come from the device).  The call writes m * n 96-byte records: record
 * dst_first + j * n + i of dst is transform j applied to record i of src, i < n, j < m.  m = 1, dst_first = 0 is a plain placement, m > 1 makes
 * instances, dst_first lets several calls assemble one scene buffer from several sets.  It writes no other byte of dst and no byte of src or xf.
 *
 * The definition (gs4d_host_transform_records is this text, for one transform).  All arithmetic is float32, round to nearest, no contraction:
 * every product and every sum is rounded on its own, in the order given.  The products are FULL products, as in gs4d_build_records: inf * 0 is a
 * NaN, and a signed zero decides the sign of a zero sum.  With l, o the row's fields, p = floats 0, 1, 2, 3 of the record and
 * S[c][k] = float 8 + 4c + k:
 *     p'[r]    = ((((l[r]*p[0]) + (l[4+r]*p[1])) + (l[8+r]*p[2])) + (l[12+r]*p[3])) + o[r]         r = 0..3   (floats 0..3; float 3 is mu_t)
 *     T[c][r]  = (((l[r]*S[c][0]) + (l[4+r]*S[c][1])) + (l[8+r]*S[c][2])) + (l[12+r]*S[c][3])       T = L Sigma
 *     S'[c][r] = (((T[0][r]*l[c]) + (T[1][r]*l[4+c])) + (T[2][r]*l[8+c])) + (T[3][r]*l[12+c])       Sigma' = T L^T  (floats 8 + 4c + r)
 *     floats 4..7 (rgba) are copied.
 * All 16 elements of Sigma' are evaluated; nothing is mirrored, so a symmetric Sigma does not promise a bit-symmetric Sigma'.  The records have the
 * bits of the host function, except that a word that is a NaN on both sides may differ in sign and payload (the rule of gs4d_build_records).
 * Nothing depends on the order in which anything runs on the device: the same inputs give the same bits.
 *
 * The other per-record tables of the set:
 *     time spans (gs4d_record_time_spans)  are those of the SOURCE records.  When L touches time — a time row other than (0, 0, 0, 1), a time offset
 *                or a velocity column — they must be computed again for the transformed set; a purely spatial placement keeps them.
 *     SH table (gs4d_shade_sh)  is not rotated by this call; gs4d_rotate_sh (below) writes the rotated table, with the same xf and m
 *                (GS4D_SH_EACH: row j*n + i for instance j), and the moved set is shaded with it and the true camera:
 *                transform -> rotate_sh -> shade_sh -> gs4d_keygen -> gs4d_sort_pairs -> draw.  For ONE rigid map M over a whole set the cheaper
 *                route moves no table: shade the SOURCE set with the camera mapped through the inverse (cam_pos' = M^-1 cam_pos, the time mapped
 *                back likewise), then transform: shade -> transform -> gs4d_keygen -> gs4d_sort_pairs -> draw.  That route cannot serve m > 1
 *                instances that face different ways, nor a set that is written back out with gs4d_decompose_records.  Under a map that is
 *                not a similarity gs4d_rotate_sh turns the table by the Gram-Schmidt frame of the map's spatial block.
 *     depth keys (gs4d_keygen, GS4D_KEY_REF_INV_EUCLID)  move a centre by sig[3].xyz * (t - mu_t) without the division by Sigma44 that the draws'
 *                conditioning has, as the reference does: the key's centre is the conditional centre only where Sigma44 == 1.  A time scale a gives
 *                both factors an a, so the key's displacement takes a^2 where the conditional centre's takes none: every splat of a retimed set is
 *                drawn where it belongs, but GS4D_MODE_4D_SORTED blends the set in the order of ITS keys, which for |a| != 1 is not the order of
 *                the source's.  Rotation, translation and a time offset keep the order.  A set baked at the draw's time (gs4d_slice_records,
 *                below) has no such gap: its stored centre is the conditional centre, so its reference key is the key of the centre that is drawn.
 *     statistics, spatial order and kept_index tables are indexed by record: instance j's record i is record dst_first + j * n + i.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: n, m, dst_first or dst_first + m * n above 0xFFFFFFFF; a name that is not a live buffer;
 * any two of the three buffers being the same; src smaller than 96 n bytes; xf smaller than 80 m bytes; dst holding fewer than dst_first + m * n
 * records.  n == 0 or m == 0 with otherwise valid arguments is a no-op.  The rows of xf are data: non-finite and singular maps give what the
 * definition gives.
 *
 * Ordering, exactly that of gs4d_build_records: a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first; draws that
 * may still have to be run again from dst are settled; the kernel is queued on the current frame lane, the call returns at once and starts no new
 * frame; src and xf are buffers the call reads, dst one it writes (it waits, on the device, for the lanes whose draws or key generation still read
 * dst or its shadow; later calls, other lanes and the host order themselves behind it).  gs4d_buffer_invalidate hand-offs of all three buffers are
 * honoured.  It counts as a full write of dst, even with dst_first > 0: the buffer's version moves, what a sort index was sorted by is forgotten, and
 * the next draw or gs4d_keygen rebuilds the SoA shadow once (gs4d_debug_shadow_builds goes up by one) — assemble a scene buffer with all its calls
 * before the frame's gs4d_keygen. */
typedef struct gs4d_affine4 {
    float l[16];        /* L, column-major: L[r, c] = l[4 * c + r]; row / column 3 = time */
    float o[4];         /* the offset (x, y, z, t)                                        */
} gs4d_affine4;         /* 80 bytes */
GS4D_API int gs4d_transform_records(gs4d_ctx* ctx, gs4d_buf src, size_t n, gs4d_buf xf, size_t m, gs4d_buf dst, size_t dst_first);

/* ---- one transform per record: a set posed by a table of maps, indexed or blended (no reference counterpart) ----
 * gs4d_transform_records applies ONE map to every record it touches.  An articulated avatar whose splats are bound to the joints of a skeleton, a
 * scene of rigid objects that each move on their own (one object id per record) and a particle system need a per-record choice among m maps, every
 * frame.  gs4d_pose_records is that call: record dst_first + i of dst is written from record i < n of src, under the map that row i of bind — which
 * starts at byte i * bind_stride of the bind buffer — takes from the m rows of xf (gs4d_affine4, 80 bytes).  It writes no other byte of dst and no
 * byte of src, xf or bind.  src is the set in its REST pose and is never changed: every frame poses it anew into dst.
 *
 * The definition (gs4d_host_pose_records is this text).  All arithmetic is float32, round to nearest, no contraction, full products, in the order
 * the parentheses give; record(l, o, in) stands for the four lines of gs4d_transform_records' definition with the row (l, o).
 *   GS4D_POSE_INDEX   bind_stride is a multiple of 4, at least 4; the first uint32 of the row is j.
 *       j <  m:  the record is record(xf[j].l, xf[j].o, in) — the bits of gs4d_host_transform_records with that row.
 *       j >= m  (GS4D_ID_NONE included):  the 96 bytes are copied, NaN payloads and all.
 *       A uint32 buffer of object ids is a bind table as it is (bind_stride 4); so is a word at the start of the rows of a wider per-record table.
 *   GS4D_POSE_BLEND4  bind_stride is a multiple of 16, at least 32 (gs4d_gather_records and the compactions can carry the table); the row is
 *       uint32 j[4] followed by float w[4].  Slot k = 0..3 takes part iff j[k] < m, whatever w[k] is.  For each of the 20 floats e of a row
 *       (l[0..15], o[0..3]), going through the slots in order:
 *           the first slot that takes part:        a[e] = w[k] * xf[j[k]][e]
 *           every later slot that takes part:      a[e] = a[e] + (w[k] * xf[j[k]][e])
 *       and the record is record(a.l, a.o, in): linear blend skinning.  The weights are data and are not normalised; a weight of 0 is a full product
 *       (a NaN row under weight 0 gives NaN — leave a slot out with j[k] = GS4D_ID_NONE, not with a zero weight).  If no slot takes part the 96 bytes
 *       are copied as above.
 *       Consequence: a row with one participating slot of weight 1.0f gives the bits of GS4D_POSE_INDEX with that j (1.0f * x is x, -0 included).
 * The records have the bits of the host function, except that a word that is a NaN on both sides in a transformed (not copied) record may differ in
 * sign and payload (the rule of gs4d_transform_records).  Nothing depends on the order in which anything runs on the device.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: n, m, dst_first or dst_first + n above 0xFFFFFFFF; an unknown form; a bind_stride that
 * breaks the form's rule; a name that is not a live buffer; any two of the four buffers being the same; src smaller than 96 n bytes; xf smaller than
 * 80 m bytes; bind smaller than n * bind_stride bytes; dst holding fewer than dst_first + n records.  n == 0 with otherwise valid arguments is a
 * no-op; m == 0 is valid: every record is copied.  The rows of xf and bind are data.
 *
 * Ordering, exactly that of gs4d_transform_records: a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first; draws
 * that may still have to be run again from dst are settled; the kernel is queued on the current frame lane, the call returns at once and starts no
 * new frame; src, xf and bind are buffers the call reads (a gs4d_buffer_subdata of the next frame's xf orders itself behind it), dst one it writes.
 * It counts as a full write of dst: the next draw or gs4d_keygen rebuilds the SoA shadow once.  Per frame: (shade) -> pose -> gs4d_keygen ->
 * gs4d_sort_pairs -> draw for a set of constant colours; a set with an SH table takes gs4d_rotate_sh (below) with the same xf, m, bind, form and
 * bind_stride, since every record has a map of its own and no one camera serves them all:
 *     pose -> rotate_sh -> shade_sh (on the posed set, with the true camera) -> gs4d_keygen -> gs4d_sort_pairs -> draw.
 * The notes of gs4d_transform_records on time spans and the depth keys hold per record.
 * Out of scope: dual-quaternion blending, more than 4 influences, an in-place pose (src == dst), dense ids from gs4d_label_components labels. */
#define GS4D_POSE_INDEX  0u   /* bind row: one uint32 j                                  */
#define GS4D_POSE_BLEND4 1u   /* bind row: uint32 j[4], float w[4]  (32 bytes)           */
GS4D_API int gs4d_pose_records(gs4d_ctx* ctx, gs4d_buf src, size_t n, gs4d_buf xf, size_t m, gs4d_buf bind, uint32_t form, size_t bind_stride,
                               gs4d_buf dst, size_t dst_first);

/* ---- turning an SH table with the maps that move its records (no reference counterpart) ----
 * gs4d_transform_records and gs4d_pose_records move records and copy their colour; the view-dependent part of a trained set's colour lives in its
 * SH table (gs4d_shade_sh), whose rows belong to the orientation the set was trained in.  gs4d_rotate_sh writes a rotated copy of such a table on
 * the device, the map of every row chosen exactly as the record calls choose it: the xf buffer and the bind table of the record call are passed
 * again unchanged, and shading the moved set with the rotated table and the true camera gives the colours the set would show had it been trained
 * in its new place.
 *
 * Rows are those of gs4d_shade_sh: float32, c_k of channel ch at row[3k + ch]; stride is a multiple of 16, 16 .. 1024, at least 12 (degree + 1)^2.
 * Where a row goes:
 *   GS4D_SH_EACH       bind must be 0, bind_stride is not looked at.  Row dst_first + j*n + i of dst is row i < n of src under map j < m of xf: the
 *                      layout of gs4d_transform_records.
 *   GS4D_POSE_INDEX, GS4D_POSE_BLEND4   row dst_first + i of dst is row i < n of src under the map that row i of bind chooses among the m rows of
 *                      xf, by the rules of gs4d_pose_records word for word: INDEX takes row j < m and copies for j >= m (GS4D_ID_NONE included);
 *                      BLEND4 slots take part iff j[k] < m, the 16 floats of l are the blended a[0..15] of that definition (full products, a weight of
 *                      0 is multiplied like any other), and a row no slot of which takes part is copied.  bind_stride as there: a multiple of 4, at
 *                      least 4 / a multiple of 16, at least 32.
 * What is written: always the whole row.  Words 0..2 (the DC term) and every byte past 12 (degree + 1)^2 are copied bit for bit from the source
 * row: a table with a payload behind the coefficients keeps it.  At degree 0 the call is a tiled row copy (the m * n rows of instancing).  A row
 * whose map does not rotate (below), or that names no map, is copied byte for byte, NaN payloads included.  No other byte of dst is written; no
 * byte of src, xf or bind is written.
 *
 * The rotation of a map (gs4d_host_sh_rotation is this text).  Only the spatial block is looked at: a_c[r] = l[4c + r], r, c < 3; time row, time
 * column and offset take no part.  R is the Gram-Schmidt frame of the columns in the order 0, 1, 2, in float32, round to nearest, no contraction
 * (every product and every sum below is rounded on its own, in the order its parentheses give), with correctly rounded division and square root:
 *     dot(a, b) = ((a[0]*b[0]) + (a[1]*b[1])) + (a[2]*b[2])
 *     n0 = dot(a0, a0)                                              e0 = a0 * (1.0f / sqrtf(n0))
 *     u1 = a1 - (dot(e0, a1) * e0)                                  n1 = dot(u1, u1)      e1 = u1 * (1.0f / sqrtf(n1))
 *     u2 = (a2 - (dot(e0, a2) * e0)) - (dot(e1, a2) * e1)           n2 = dot(u2, u2)      e2 = u2 * (1.0f / sqrtf(n2))
 * per component.  If any of n0, n1, n2 is not > 0 or not finite — a zero, singular, NaN or overflowing block, or one so small that its squared
 * length underflows — the map DOES NOT ROTATE (the later steps are not evaluated).  R[r][c] = e_c[r].  A similarity (a rotation times a uniform
 * scale, all gs4d_host_affine4 produces) gives its rotation back up to rounding; a mirror stays a mirror (e2 is not forced right-handed); a blended
 * skinning matrix gets the frame its columns span.
 *
 * The band matrices, defined by the basis, constants and signs of gs4d_shade_sh: for every unit d and every band L = 1, 2, 3
 *     sum_k c'_k b_k(d) = sum_k c_k b_k(R^T d)          which gives c'_L = D_L c_L, D_L of size 3x3, 5x5, 7x7.
 * D_L(m, n) has m, n = -L .. L; coefficient k = L^2 + L + m.
 *   D_1 needs no arithmetic: b_1..b_3 = C1 * (-y, z, -x), so D_1 = P R P^T with the signed permutation P of (x, y, z) -> (-y, z, -x):
 *     D_1(i, j) = s_i s_j R[a_i][a_j],  a = (1, 2, 0), s = (-1, +1, -1) for i, j = -1, 0, 1        (a move or a negation)
 *   D_2 from D_1 and D_1, D_3 from D_1 and D_2 by the recurrences of Ivanic and Ruedenberg (J. Phys. Chem. 100 (1996) 6342; 102 (1998) 9099): the
 *   basis of gs4d_shade_sh is the real spherical harmonics seen through the half turn about z, (x, y, z) -> (-x, -y, z), which is what the signs of
 *   P carry, so the recurrences apply to D_1 as it stands.  With Dp = D_(L-1) and E = L - 1:
 *     P(i, a, n) =  (D_1(i, 1)*Dp(a, E)) - (D_1(i, -1)*Dp(a, -E))        for n ==  L
 *                   (D_1(i, 1)*Dp(a, -E)) + (D_1(i, -1)*Dp(a, E))        for n == -L
 *                   D_1(i, 0)*Dp(a, n)                                   otherwise
 *     U = P(0, m, n)
 *     V = P(1, 1, n) + P(-1, -1, n)            m == 0           W = P(1, m+1, n) + P(-1, -m-1, n)       m > 0
 *         P(1, 0, n)                           m == 1               P(1, m-1, n) - P(-1, -m+1, n)       m < 0
 *         P(-1, 0, n)                          m == -1
 *         P(1, m-1, n) - P(-1, -m+1, n)        m > 1
 *         P(1, m+1, n) + P(-1, -m-1, n)        m < -1
 *     D_L(m, n) = ((u*U) + (v*V)) + (w*W)      a term whose coefficient is a zero of the tables is left out (u: |m| == L; w: m == 0 or |m| >= L - 1)
 *   The coefficients depend on |m| and |n|, each rounded to float32 from
 *     u = sqrt((L+m)(L-m) / den)     v = (m == 0 ? -1 : 1) * sqrt((1 + [m == 0]) (L+|m|-1)(L+|m|) / den) / 2, times sqrt 2 where |m| == 1
 *     w = -sqrt((L-|m|-1)(L-|m|) / den) / 2          den = (L+n)(L-n) for |n| < L, 2L(2L-1) for |n| == L
 *   row |m| = 0 .. L, column |n| = 0 .. L:
 *     u, L = 2: { 1, 1.1547005383792515, 0.57735026918962573 }  { 0.8660254037844386, 1, 0.5 }  { 0, 0, 0 }
 *     v, L = 2: { -0.5, -0.57735026918962573, -0.28867513459481287 }  { 0.8660254037844386, 1, 0.5 }  { 0.8660254037844386, 1, 0.5 }
 *     w, L = 2: all 0
 *     u, L = 3: { 1, 1.0606601717798212, 1.3416407864998738, 0.54772255750516607 }  { 0.94280904158206336, 1, 1.2649110640673518, 0.5163977794943222 }
 *               { 0.7453559924999299, 0.79056941504209488, 1, 0.40824829046386302 }  { 0, 0, 0, 0 }
 *     v, L = 3: { -0.57735026918962573, -0.61237243569579447, -0.7745966692414834, -0.31622776601683794 }
 *               { 0.81649658092772603, 0.8660254037844386, 1.0954451150103321, 0.44721359549995793 }
 *               { 0.7453559924999299, 0.79056941504209488, 1, 0.40824829046386302 }  { 0.9128709291752769, 0.96824583655185426, 1.2247448713915889, 0.5 }
 *     w, L = 3: row 1 = { -0.23570226039551584, -0.25, -0.31622776601683794, -0.12909944487358055 }, every other row 0
 *   Only + - * are used.  Being homogeneous of degree L in R, D_L of a mirror is what the defining identity asks of it.
 * Layout of d[84], all row-major: D_1 at 0, D_2 at 9, D_3 at 34, word 83 is 0.
 * The application, per channel and output coefficient i of a band, in ascending j:
 *     acc = D[i][0]*c_0      then      acc = acc + (D[i][j]*c_j)      j = 1 .. 2L
 * Consequences.  Under the identity map (any positive power-of-two scale of it included) the frame is exact, every D_L is the unit matrix with
 * zeros of either sign around it, and every finite row comes back with its values and, for every word that is not a zero, its bits; a -0
 * coefficient does NOT promise to keep its sign (a sum of zeros of both signs is +0).  A non-finite coefficient spreads through its band and
 * channel as the products give.  Two quarter turns about z give the half turn's bits.
 * The device gives the bits of gs4d_host_rotate_sh, except that a word that is a NaN on both sides in a rotated (not copied) row may differ in sign
 * and payload.  Nothing depends on the order in which anything runs on the device.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: n, m or dst_first above 0xFFFFFFFF, and so m * n and dst_first + m * n (GS4D_SH_EACH) or
 * dst_first + n (the other forms); a degree outside 0 .. 3; a stride that breaks the rule; an unknown form; bind != 0 with GS4D_SH_EACH, bind == 0
 * with the other two; a bind_stride that breaks the form's rule; a name that is not a live buffer; any two buffers being the same; src smaller than
 * n * stride bytes; xf smaller than 80 m; bind smaller than n * bind_stride; dst holding fewer rows than the call writes past dst_first.  n == 0 is
 * a no-op, and so is m == 0 with GS4D_SH_EACH; m == 0 with a bind table copies every row.  The rows of xf, bind and src are data.
 *
 * Ordering, that of gs4d_copy_rows: the kernel is queued on the current frame lane and the call returns at once; src, xf and bind are buffers the
 * call reads, dst one it writes, keeping the rows it does not name.  A table is not a record buffer: no shadow is built or invalidated.  The frame
 * loops:
 *     pose -> rotate_sh -> shade_sh (on the posed set, with the true camera) -> gs4d_keygen -> gs4d_sort_pairs -> draw
 *     transform -> rotate_sh -> shade_sh -> ...        for instances (GS4D_SH_EACH, the same xf and m)
 * For ONE rigid map over a whole set the camera-inverse route of gs4d_transform_records stays the cheaper choice: it moves no table.
 * Out of scope: gs4d_warp_records (a warp needs the local rotation of its Jacobian) and gs4d_transform_selected (a selection needs a rule operand);
 * degrees above 3; an in-place rotation (src == dst). */
#define GS4D_SH_EACH 2u   /* no bind table: every map to every row, the layout of gs4d_transform_records */
GS4D_API int gs4d_rotate_sh(gs4d_ctx* ctx, gs4d_buf src, size_t n, size_t stride, int degree,
                            gs4d_buf xf, size_t m, gs4d_buf bind /* 0 with GS4D_SH_EACH */, uint32_t form, size_t bind_stride,
                            gs4d_buf dst, size_t dst_first);

/* ---- time-varying view-dependent colour: spherical harmonics times a cosine series in time (no reference counterpart) ----
 * The colour model of trained 4D sets (4DGS and its successors; the sets GS4D_PARAMS_4D_2Q builds the records of) is not the 3DGS table of
 * gs4d_shade_sh: per channel it holds degree_t + 1 BLOCKS of SH coefficients, block n weighted by cos(2 pi n (t - mu_t) / T).  gs4d_shade_sh_t
 * evaluates that model every frame, as gs4d_shade_sh evaluates a 3DGS table; gs4d_collapse_sh writes, for one time, the ordinary 3DGS row every 4D
 * row comes to — the table of a frame frozen by gs4d_slice_records, which gs4d_shade_sh then shades from any camera.  Both are one definition:
 *     gs4d_shade_sh_t(data, sh)  writes the bits of  gs4d_shade_sh(data, gs4d_collapse_sh(data, sh))  at q->degree, q->t, q->cam_pos.
 *
 * The table.  Row i is the sh_stride bytes at sh + i*sh_stride, float32 with the channels interleaved as in gs4d_shade_sh, block after block: with
 * K = (degree + 1)^2, coefficient k of block n, channel ch, is row[3 (n K + k) + ch] — at degree 3 the 4DGS tensor [N, 16 (degree_t + 1), 3] as
 * it stands.  sh_stride: a multiple of 16, 16 .. 1024, and >= 12 K (degree_t + 1) (minimal rows: 576 bytes at degree 3 / degree_t 2).  A lower
 * degree_t reads a prefix of the same row.  A lower degree does NOT: the pitch of the blocks is K, so a table laid out for degree 3 cannot be read
 * at degree 2 (lay the rows out again; reading a lower degree out of a higher one is out of scope).  Only the first 12 K (degree_t + 1) bytes,
 * rounded up to 16, are ever read.
 *
 * The weights.  Arithmetic as everywhere: float32, round to nearest, no contraction, every product and sum rounded on its own in the order
 * written.  With mu_t = float 3 of record i:
 *     u = (t - mu_t) * inv_period
 *     for n = 1 .. degree_t:
 *         v = (float)n * u
 *         block n TAKES PART iff v is finite          (else it is left out: a NaN / Inf t, mu_t or inv_period is data)
 *         r = v - rintf(v)                            (exact; |v| >= 2^23 gives r = 0 and w = 1)
 *         a = fabsf(r);  neg = a > 0.25f;  x = neg ? 0.5f - a : a        (exact)
 *         s = x*x
 *         p = T6;  p = (p*s) + T5;  p = (p*s) + T4;  p = (p*s) + T3;  p = (p*s) + T2;  p = (p*s) + T1
 *         c = (p*s) + 1.0f
 *         w_n = neg ? -c : c
 *     T_j = float32((-1)^j (2 pi)^(2j) / (2j)!), j = 1 .. 6:
 *         -19.739208802178716, 64.93939402266828, -85.45681720669371, 60.24464137187664, -26.426256783374388, 7.903536371318465
 *         (bits c19de9e6 4281e0f8 c2aae9e4 4270fa83 c1d368f9 40fce9c5)
 * Over every float32 x in [0, 0.25], |c - cos(2 pi x)| <= 1.561e-7, c stays in [0, 1], c(0) = 1 and c(0.25) = 0 exactly: w(0) = 1, w(+-1/2) = -1, w
 * is even and |w| <= 1.  r, a and x being exact, 1.561e-7 is the whole error of w_n against cos(2 pi v) of the float32 v (cosf(2 pi v) in float32 is
 * off by 2.0e-7 at |v| <= 1/2, 7.9e-7 at |v| <= 2, 4.8e-5 at |v| <= 100).
 *
 * The effective row.  Per word j < 3 K, c_(n,j) being word j of block n:
 *     e_j = c_(0,j);   if block 1 takes part: e_j = e_j + (w_1 * c_(1,j));   if block 2 takes part: e_j = e_j + (w_2 * c_(2,j))
 *
 * gs4d_collapse_sh writes e_0 .. e_(3K-1) to row i < n of dst and zeros from word 3 K to dst_stride / 4.  dst_stride: a multiple of 16, 16 .. 1024,
 * >= 12 K.  Nothing past row n - 1 of dst is written; data and sh are read only, and of a record only float 3 is used; q->cam_pos is ignored.
 * degree_t == 0 copies the prefix.
 *
 * gs4d_shade_sh_t writes floats 4..6 of record i < n with exactly what gs4d_shade_sh at q->degree, q->t and q->cam_pos writes from the row e: its
 * direction, basis, sum order, DC-only rule and clamp, unchanged.  degree_t == 0, or no block taking part, gives the bits of gs4d_shade_sh on the
 * same table.  UNLIKE the 4DGS rasterizer, whose direction runs from the camera to the REST mean of the splat, the direction runs to the
 * time-conditioned mean the draw projects, as in gs4d_shade_sh.  The device gives the bits of gs4d_host_collapse_sh and gs4d_host_shade_sh_t,
 * except that a word of a collapsed row that is a NaN on both sides may differ in sign and payload.  Nothing depends on the order in which
 * anything runs on the device.
 *
 * gs4d_merge_rows and 4D tables: the effective row is linear in the coefficients only among members with EQUAL mu_t (the weights are the
 * record's); merging 4D rows word by word is right for such groups only.  Posing a 4D table: every block rotates with the same band matrices, so
 * at degree 3 with sh_stride == 192 (degree_t + 1) a table of n rows IS a table of (degree_t + 1) n rows of 192 bytes, which gs4d_rotate_sh turns
 * as it stands — GS4D_SH_EACH with one map, or GS4D_POSE_INDEX with every bind word repeated degree_t + 1 times.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: q == NULL; degree outside 0 .. 3; degree_t outside 0 .. 2; reserved != 0; n >
 * 0xFFFFFFFF; an sh_stride or dst_stride that breaks its rule; a name that is not a live buffer; any two named buffers being the same; data smaller
 * than 96 n bytes, sh smaller than n * sh_stride, dst smaller than n * dst_stride.  n == 0 is a no-op.  t, inv_period and cam_pos are data.
 *
 * Ordering.  gs4d_shade_sh_t: that of gs4d_shade_sh, gs4d_buffer_invalidate hand-offs included, and the same COLOUR-ONLY write — a current SoA
 * shadow gets its colour plane patched and stays current; per frame shade_sh_t -> gs4d_keygen -> gs4d_sort_pairs -> draw.  gs4d_collapse_sh: that
 * of gs4d_rotate_sh — tables are not record buffers, data and sh are buffers the call reads, dst one it writes; no shadow is built or invalidated.
 * A frozen frame that keeps its view dependence: gs4d_slice_records at t (kept_index), gs4d_collapse_sh of the source at t, gs4d_gather_records of
 * the collapsed rows through kept_index; gs4d_shade_sh of the frozen set at t == mu_t_out then gives the colours gs4d_shade_sh_t gives the source
 * (bit for bit where the time column and the time row of a record's sig hold the same bits: the slice conditions with the column, the shade
 * with the row).
 * Out of scope: degree_t > 2; fp16 tables; a lower degree out of a higher-degree 4D table; collapsing into the shadow. */
typedef struct gs4d_sh_time {
    int32_t  degree;      /* 0 .. 3: the SH degree, K = (degree + 1)^2 coefficients per block */
    int32_t  degree_t;    /* 0 .. 2: blocks 0 .. degree_t are read */
    float    t;           /* the time */
    float    inv_period;  /* 1 / T of the cosine series (4DGS: 1 / time_duration), computed by the caller */
    float    cam_pos[3];  /* gs4d_shade_sh_t only; gs4d_collapse_sh ignores it */
    uint32_t reserved;    /* 0 */
} gs4d_sh_time;           /* 32 bytes */
GS4D_API int gs4d_shade_sh_t(gs4d_ctx* ctx, gs4d_buf data, size_t n, gs4d_buf sh, size_t sh_stride, const gs4d_sh_time* q);
GS4D_API int gs4d_collapse_sh(gs4d_ctx* ctx, gs4d_buf data, size_t n, gs4d_buf sh, size_t sh_stride, const gs4d_sh_time* q,
                              gs4d_buf dst, size_t dst_stride);

/* ---- a map that varies from point to point: a set deformed through a 4D lattice (no reference counterpart) ----
 * gs4d_transform_records and gs4d_pose_records apply affine maps.  A cage or free-form deformation in an editor (bend, bulge, taper), a baked
 * deformation field with a time axis (how a static or a 4D set is animated non-rigidly) and a retiming field (a region that plays slower or later
 * than the rest) need a map that varies smoothly from point to point.  gs4d_warp_records is that call: record dst_first + i of dst is written from
 * record i < n of src through the map x' = x + D(x), D being the multilinear interpolant of a lattice of displacement nodes, linearised at the
 * record's own centre: mean' = mu + D(mu), Sigma' = L Sigma L^T with L = I + grad D(mu), a full 4x4 matrix.  A time column of grad D gives velocity,
 * a dt component retiming.  It writes no other byte of dst and no byte of src or nodes.  src is never changed: every frame warps it anew into dst.
 *
 * The lattice (gs4d_lattice, read on the host at the call) has dims[a] nodes along axis a = 0..3 (x, y, z, t); node 0 stands at lo[a] and there are
 * inv[a] nodes per unit.  nodes holds dims[0] * dims[1] * dims[2] * dims[3] nodes of 16 bytes: float d[4], the displacement (dx, dy, dz, dt) at the
 * node; node (x, y, z, t) is at index ((t * dims[2] + z) * dims[1] + y) * dims[0] + x.
 *
 * The definition (gs4d_host_warp_records is this text).  All arithmetic follows the rules of gs4d_transform_records: float32, round to nearest, no
 * contraction, full products, in the order the parentheses give.  p[a] = float a of the record (float 3 is mu_t).
 *   Per axis a, with d = dims[a]:
 *     d == 1   the axis does not take part: its node index is 0, the tree below has no level for it, and column a of G is four +0.0f, not
 *              computed.  A static lattice has dims[3] == 1; a 2D sheet and a single node (a pure translation) fall out of the same rule.
 *     d >= 2   u = (p[a] - lo[a]) * inv[a];  top = (float)(d - 1).
 *              If bit a of clamp is set: u < 0.0f becomes 0.0f, u > top becomes top; whether either happened is remembered.
 *              The record is INSIDE on a iff u >= 0.0f && u <= top (a NaN is never inside, with or without the clamp).
 *              i = min((uint32)u, d - 2), converted only when inside;  f = u - (float)i  (u == top gives i = d - 2, f = 1).
 *              If the clamp changed u, column a of G is four +0.0f: the clamped field is constant along a.
 *   A record that is not inside on every axis with d >= 2 is copied: the 96 bytes, NaN payloads and all (the rule of gs4d_pose_records for
 *   j >= m).  Consequence: for every bit pattern of the record, of lo and of inv, only nodes of the lattice are read, and no value but
 *   0 <= u <= 65534 is converted to an integer.  lo and inv are data and are not validated.
 *   The interpolation is one fixed tree per component k = 0..3 of d, over the 2 x 2 x 2 x 2 nodes at i[a], i[a] + 1 (one node on an axis with
 *   d == 1), reducing x, then y, then z, then t; a level whose axis has d == 1 is skipped.
 *     a value step of a pair (a, b) along axis a:    a + (f[a] * (b - a))
 *     D[k]      the tree of value steps.
 *     G[k][a]   (d D_k / d x_a of that interpolant) the levels before a are value steps, those of D; level a is (b - a) * inv[a] in the place of
 *               the value step; the levels after a are value steps on those differences.
 *     l[4c + r] = (r == c ? 1.0f : 0.0f) + G[r][c]
 *   The record of an inside centre:  floats 0..3 = p[r] + D[r];  floats 4..7 copied;  Sigma' by the T = L Sigma and Sigma' = T L^T lines of
 *   gs4d_transform_records' definition with this l — all 16 elements are evaluated, nothing is mirrored.  A folded map (det L <= 0) gives what the
 *   lines give.
 *   Consequences:  a lattice whose nodes are all +0.0f leaves Sigma with the bits of gs4d_host_transform_records under the identity row (and the
 *   mean as p[r] + 0.0f).  An axis of two equal finite nodes without a -0 gives, on a finite set inside it, the same bits as that axis with one node.
 * The records have the bits of the host function, except that a word that is a NaN on both sides of a warped (not copied) record may differ in sign
 * and payload (the rule of gs4d_transform_records).  Nothing depends on the order in which anything runs on the device.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: lat == NULL; a dim that is 0 or above 65535; more than 1 << 28 nodes; clamp bits above 3
 * or a non-zero pad; n, dst_first or dst_first + n above 0xFFFFFFFF; a name that is not a live buffer; any two of the three buffers being the same;
 * src smaller than 96 n bytes; nodes smaller than 16 bytes times the node count; dst holding fewer than dst_first + n records.  n == 0 with
 * otherwise valid arguments is a no-op.  The nodes are data: NaN, Inf and huge displacements give what the definition gives.
 *
 * Ordering, exactly that of gs4d_pose_records: a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first; draws that
 * may still have to be run again from dst are settled; the kernel is queued on the current frame lane, the call returns at once and starts no new
 * frame; src and nodes are buffers the call reads (a gs4d_buffer_subdata of the next frame's nodes orders itself behind it), dst one it writes.
 * It counts as a full write of dst: the next draw or gs4d_keygen rebuilds the SoA shadow once.  Per frame: (shade) -> warp -> gs4d_keygen ->
 * gs4d_sort_pairs -> draw.  The notes of gs4d_transform_records hold per record: time spans must be computed again when the lattice has a time axis
 * or a dt component; the SH table is not rotated, and gs4d_rotate_sh does not serve a warp (it takes affine maps; a warp would need the local
 * rotation of its Jacobian at every record); the depth-key remark holds.
 * Out of scope: an in-place warp (src == dst), a statistics rule that selects which records warp, higher-order (B-spline) lattices, rotating SH
 * rows by the warp's local rotation, reporting folded records. */
typedef struct gs4d_lattice {
    float    lo[4];     /* where node 0 stands on x, y, z, t                         */
    float    inv[4];    /* nodes per unit along each axis (1 / spacing)              */
    uint32_t dims[4];   /* nodes per axis, each 1..65535, their product <= 1 << 28   */
    uint32_t clamp;     /* bit a set: axis a clamps; bits 4..31 must be 0            */
    uint32_t pad[3];    /* must be 0                                                 */
} gs4d_lattice;         /* 64 bytes */
GS4D_API int gs4d_warp_records(gs4d_ctx* ctx, gs4d_buf src, size_t n, gs4d_buf nodes, const gs4d_lattice* lat, gs4d_buf dst, size_t dst_first);

/* ---- a frame of a clip as a 3D set: the records baked at one time (no reference counterpart) ----
 * The draws condition a 4D record at uTime — the time opacity, the conditional centre, the conditional 3x3 covariance — inside the projection
 * kernel, every frame.  gs4d_slice_records does that once and writes the result as records: the 3D set that the 4D set IS at time q->t, to be drawn
 * while playback is paused, edited as a static object or exported as one frame.  The call writes record dst_first + i of dst from record i < n of
 * src; it writes no other byte of dst and no byte of src.
 *
 * The definition (gs4d_host_slice_records is this text).  All arithmetic is float32, round to nearest, no contraction, full products; the order of
 * the operations is that of the draw's conditioning.  With p = floats 0..3 of the record, S[c][r] = float 8 + 4c + r and maxf(a, b) = a >= b ? a : b:
 *     s44 = S[3][3];  dt = t - p[3];  inv = 1.0f / s44
 *     ot  = maxf(expf(((-0.5f * dt) * inv) * dt), min_opacity)
 *     k   = inv * dt
 *     a[r]  = S[r][3]      (floats 11, 15, 19: the time COLUMN, as the draw reads it)
 *     tv[c] = inv * S[3][c]      (floats 20, 21, 22: the time row)
 *     floats 0..2       = p[r] + (k * a[r])
 *     float 3           = mu_t_out
 *     floats 4..6       copied;  float 7 = ot * (float 7)
 *     float 8 + 4c + r  = S[c][r] - (a[r] * tv[c])        c, r = 0..2
 *     floats 11, 15, 19 (time column) and 20, 21, 22 (time row) = -0.0f;  float 23 = s44_out
 * The zeros are NEGATIVE on purpose: at uTime == mu_t_out the draw of the slice computes dt = +0 and k = +0; k * (-0) = -0 and x + (-0) = x for
 * every x, -0 included; (-0) * (inv * (-0)) = +0 and x - (+0) = x; expf(-0) = 1 and 1 * alpha = alpha.  With +0 in those words a coordinate or
 * covariance element that is -0 would come back as +0.
 *
 * The guarantee.  With uTime == q->mu_t_out and uMinOpacity <= 1 and equal to q->min_opacity, a draw of the slice gives the bits of a draw of the
 * source at uTime == q->t — the colour image, the aux planes, the ID planes and the record statistics, for every blend function under which the
 * draw has them (no record is dropped: record i of the slice is record i of the source, and the projected records of the two draws are the same
 * bits) — in GS4D_MODE_4D_DIRECT, or in GS4D_MODE_4D_SORTED with the same index buffer.
 * The two sets' OWN keys (gs4d_keygen) are bit-equal under GS4D_KEY_VIEW_Z for records whose Sigma is bit-symmetric in its time row and column
 * (the key reads the row, the draw the column), and under GS4D_KEY_REF_INV_EUCLID additionally only where Sigma44 is exactly 1: the reference's key
 * does not divide by Sigma44 (the note at gs4d_transform_records).  Elsewhere the slice's reference key is the key of the centre that is DRAWN —
 * in a slice the stored centre is the conditional centre, so both keys are right.
 *
 * Device precision.  Words 0..6 and 8..23 have the bits of the host function, except that a word that is a NaN on both sides may differ in sign and
 * payload.  Word 7 goes through the device's expf: it is bit-equal to the alpha the device's own draw computes for the source record, which is what
 * the guarantee needs, and within 5e-6 relative of the host's (the project's bar for that expression).
 *
 * What the slice buys.  Its eight time-related words are the same in every record, so the SoA shadow of a buffer that holds only slice records
 * (of one mu_t_out and s44_out) is the 64-byte static-3D layout, where the 4D source reads 96 bytes per record and frame; and its records with
 * alpha 0 are dead at every time, so gs4d_count_centres with GS4D_CQ_SKIP_HIDDEN + gs4d_compact_records remove them for good.  For a long clip
 * gs4d_compact_time_window(spans, n, t, t) first and a slice of the survivors is the cheaper order.  Away from uTime == mu_t_out a slice fades like any static
 * record of that Sigma44; with s44_out == +inf it does not (1 / s44_out is 0: the opacity factor is expf(-0) = 1 and the centre stays where it is,
 * up to the sign of a zero coordinate, at every finite uTime).  Time spans are those of the slice's own time words.  The SH table is not touched
 * (shade the source at t first).
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: q == NULL; t or mu_t_out not finite; min_opacity a NaN; s44_out a NaN or <= 0 (+inf is
 * allowed); n, dst_first or their sum above 0xFFFFFFFF; a name that is not a live buffer; src == dst; src smaller than 96 n bytes; dst holding fewer
 * than dst_first + n records.  n == 0 with otherwise valid arguments is a no-op.  Records are data: hostile ones give what the definition gives.
 *
 * Ordering, exactly that of gs4d_transform_records: a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first; draws
 * that may still have to be run again from dst are settled; the kernel is queued on the current frame lane, the call returns at once and starts no
 * new frame; src is a buffer the call reads, dst one it writes (it waits, on the device, for the lanes whose draws or key generation still read dst
 * or its shadow; later calls, other lanes and the host order themselves behind it).  gs4d_buffer_invalidate hand-offs of both buffers are honoured.
 * It counts as a full write of dst, even with dst_first > 0: the buffer's version moves, what a sort index was sorted by is forgotten, and the next
 * draw or gs4d_keygen rebuilds the SoA shadow once (gs4d_debug_shadow_builds goes up by one). */
typedef struct gs4d_slice {
    float t;            /* the time the source is conditioned at; finite                                   */
    float min_opacity;  /* the draw's uMinOpacity: the floor of the time opacity; not a NaN                */
    float mu_t_out;     /* float 3 of every slice record: the uTime the slice is to be drawn at; finite    */
    float s44_out;      /* float 23 of every slice record; > 0, +inf allowed                               */
} gs4d_slice;           /* 16 bytes */
GS4D_API int gs4d_slice_records(gs4d_ctx* ctx, gs4d_buf src, size_t n, const gs4d_slice* q, gs4d_buf dst, size_t dst_first);

/* ---- colour edits by a selection: recolour, hide or restore selected records (no reference counterpart) ----
 * What a selection is shown with.  The selection chain ends in a statistics table — gs4d_count_ids for what a region of the ID planes shows,
 * gs4d_set_record_stats for what a draw showed, a gs4d_stat_cut threshold for the k most visible records; gs4d_edit_colours edits the rgba (floats
 * 4..7) of the records of `data` that such a table selects, in place and on the device.
 *
 * Selection.  Record i < n of the 96-byte records in data is SELECTED iff stats == 0 (every record), or row i of the gs4d_record_stat table
 * `stats` passes `rule` under exactly the predicate of gs4d_compact_records: (pixels >= min_pixels && wmax >= min_wmax && wsum >= min_wsum) != invert.
 * A gs4d_count_ids table with {1, 0, 0, 0} selects what the region shows, the same with GS4D_KEEP_INVERT everything else (isolate).
 *
 * The edit.  For a selected record and each channel ch whose bit is set in `channels`, with c = float 4 + ch of the record:
 *     GS4D_EDIT_SET    c' = value[ch]                                     (the bits)
 *     GS4D_EDIT_MUL    c' = c * value[ch]
 *     GS4D_EDIT_LERP   c' = c + (amount * (value[ch] - c))
 *     GS4D_EDIT_COPY   c' = float 4 + ch of record i of `from`             (the bits)
 * The arithmetic is float32, round to nearest, no contraction: every product and every sum is rounded on its own, in the order its parentheses
 * give.  value and amount are data: non-finite operands give what these lines give.  A result that is a NaN may differ from
 * gs4d_host_edit_colours' in sign and payload for MUL and LERP (the rule of gs4d_build_records); SET and COPY are bit copies, NaNs included.
 *
 * What is written.  Every other word of a selected record, every byte of a record that is not selected and every byte of data beyond record n - 1
 * keep their bits; stats and from are never written.  Nothing depends on the order in which anything runs on the device.
 *
 * An alpha of 0.  What the time-window section says of a dead record holds for a record whose float 7 is exactly 0 (+0 or -0): with the default
 * blend function and a finite time opacity its alpha is 0 at every pixel, so it is an exact no-op in the colour image and in the aux planes
 * (C += 0, T *= 1, weight 0), it never becomes an ID candidate and it adds nothing to record statistics.  Hiding a selection with {GS4D_EDIT_SET,
 * channels = 8, value[3] = 0} therefore gives the bits of a draw of the compacted complement (gs4d_compact_records with the inverted rule; record
 * indices in the ID planes and statistics rows mapped through kept_index), in GS4D_MODE_4D_SORTED after gs4d_keygen + gs4d_sort_pairs of the
 * respective set and in GS4D_MODE_4D_DIRECT — without moving a record, so the set, its tables and its shadow stay what they were.  A later
 * GS4D_EDIT_COPY from a pristine copy puts the colours back.  Nothing is promised for any other blend function.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: edit == NULL, an unknown op, channels == 0 or > 15, reserved != 0; n > 0xFFFFFFFF; data not
 * a live buffer or smaller than 96 n bytes; exactly one of stats / rule given; a rule with an unknown flag or reserved != 0; stats not a live buffer
 * or smaller than 16 n bytes; GS4D_EDIT_COPY without a live `from` of at least 96 n bytes; any other op with from != 0; any two of the named buffers
 * being the same buffer.  n == 0 with otherwise valid arguments is a no-op.
 *
 * Ordering: that of gs4d_shade_sh for data and from, that of gs4d_compact_records for stats.  A queued gs4d_keygen / gs4d_sort_pairs that names one
 * of the buffers is launched first.  The table is taken as gs4d_buffer_read takes it: draws that add to it (gs4d_set_record_stats), issued before the
 * call on any frame lane, are settled first, re-runs included; a draw issued afterwards that adds to it waits on the device until the call's kernel
 * has read it, and a host write waits as it does for any reader.  Draws that may still have to be run again from data are settled before it is
 * overwritten.  The kernel is queued on the current frame lane, the call returns at once and starts no new frame; data waits, on the device, for the
 * lanes whose draws or key generation still read it or its shadow; later calls, other lanes and the host order themselves behind the call.
 * gs4d_buffer_invalidate hand-offs of all three buffers are honoured.
 *
 * What the write keeps: gs4d_shade_sh's colour-only contract, extended to the alpha.  Nothing the library derives from a record buffer reads floats
 * 4..7 — the shadow carries them in its colour plane, the bounding box and the key bounds read position, mu_t and sig[3].xyz, the layout choice sig
 * and mu_t — so if the SoA shadow of data is current when the call is made, the same kernel writes the edited rgba into the shadow's colour plane and
 * the shadow stays current: the next draw neither repacks nor waits, and gs4d_debug_shadow_builds does not move.  If it is not current, only the
 * records are written and the next draw builds it, as it would have anyway.  As with gs4d_shade_sh the provenance of a sort index is NOT kept: the
 * call order per frame is (gs4d_shade_sh) -> gs4d_edit_colours -> gs4d_keygen -> gs4d_sort_pairs -> draw.  Tables of the caller's that depend on
 * the alpha (gs4d_record_time_spans: a record of alpha <= 0 has the span "never") are the caller's to recompute. */
enum { GS4D_EDIT_SET = 0, GS4D_EDIT_MUL = 1, GS4D_EDIT_LERP = 2, GS4D_EDIT_COPY = 3 };
typedef struct gs4d_colour_edit {
    uint32_t op;         /* GS4D_EDIT_*                                                          */
    uint32_t channels;   /* bit ch set: channel ch of rgba is edited (1 r, 2 g, 4 b, 8 a); 1 .. 15 */
    float    value[4];   /* SET, MUL, LERP: the operand per channel; COPY: ignored                 */
    float    amount;     /* LERP only; ignored otherwise                                           */
    uint32_t reserved;   /* must be 0                                                              */
} gs4d_colour_edit;      /* 32 bytes */
GS4D_API int gs4d_edit_colours(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_colour_edit* edit,
                               gs4d_buf stats /* 0: every record */, const gs4d_keep_rule* rule /* NULL iff stats == 0 */,
                               gs4d_buf from /* GS4D_EDIT_COPY: the source records; otherwise 0 */);

/* ---- selection by where a record IS: a statistics table from a volume or a screen region (no reference counterpart) ----
 * The second way into the selection chain.  gs4d_count_ids selects what a region of the ID planes SHOWS, one record per pixel; gs4d_count_centres
 * selects the records whose centre at time t lies in a box or a sphere of the world and / or projects into a rectangle (a lasso) of the screen —
 * visible or not, through every occluder — and writes the answer where gs4d_compact_records, gs4d_stat_cut and gs4d_edit_colours take it from: a
 * gs4d_record_stat table.  gs4d_host_count_centres is this text as code.
 *
 * All arithmetic is float32, round to nearest, no contraction: every product and every sum is rounded on its own, in the order the parentheses
 * give; division is correctly rounded; the two fmaf below are real fused operations.  For record i < n of the 96-byte records in data, with
 * p = floats 0..2, mu_t = float 3, a = float 7, sig3 = floats 20..22, s44 = float 23:
 *
 * Centre (that of gs4d_shade_sh and GS4D_KEY_VIEW_Z).
 *     dt = t - mu_t;   k = (1.0f / s44) * dt;   m = p + (k * sig3)   per component.
 * The draws take floats 11, 15 and 19 in the place of sig3.  A symmetric covariance holds those bit-equal to sig3, and for such records m is the
 * centre the draws project.
 *
 * Skips.  GS4D_CQ_SKIP_HIDDEN skips a record iff !(a > 0): the time-span table's "never", and what hiding with gs4d_edit_colours produces.
 * GS4D_CQ_SKIP_DEAD skips a record iff ((-0.5f * dt) * (1.0f / s44)) * dt < GS4D_TIME_DEAD_ARG; a NaN is not skipped.
 *
 * Volume.  q = m; with GS4D_CQ_FRAME, f = frame: q[r] = (((f[r] * m.x) + (f[3 + r] * m.y)) + (f[6 + r] * m.z)) + f[9 + r].
 *     GS4D_CQ_BOX     passes iff box_lo[a] <= q[a] && q[a] <= box_hi[a] for a = 0, 1, 2;
 *     GS4D_CQ_SPHERE  with d = q - (sphere[0..2]) and r = sphere[3]: passes iff ((d.x * d.x) + (d.y * d.y)) + (d.z * d.z) <= r * r.
 * A NaN anywhere fails the test it is in.  GS4D_CQ_FRAME without BOX or SPHERE is allowed and has no effect.
 *
 * Screen (GS4D_CQ_SCREEN).  The draws' own expressions for the centre, with W x H the context's image:
 *     pc = view * (m, 1);   ps = proj * pc          ((a + b) + c) + d per row, column-major, the `* 1.0f` of the last product of pc included
 *     rw = 1.0f / ps.w;   nx = rw * ps.x;   ny = rw * ps.y
 *     hw = W * 0.5f;   hh = H * 0.5f;   wx = fmaf(nx, hw, hw);   wy = fmaf(ny, hh, hh)
 * It passes iff  ps.w > 0  &&  depth_min <= -pc.z && -pc.z <= depth_max  &&  wx >= (float)x && wx < (float)(x + w)  &&  wy >= (float)y &&
 * wy < (float)(y + h)  &&  (mask == 0 || mask[(floorf(wy) - y) * w + (floorf(wx) - x)] != 0).  The mask byte is looked at only once the comparisons
 * have passed, so the index is inside the mask.  The mask is a gs4d_count_ids mask — w * h bytes, rows bottom-up, any non-zero byte counts — and
 * one uploaded lasso serves both calls.  The draws' clip tests are NOT applied: a centre the draws would clip is selected if it passes the above.
 *
 * Taking part.  Record i takes part iff it is not skipped and every enabled test passes; with no test bit set, every record that is not skipped.
 *
 * The row.  GS4D_CQ_ADD adds to row i of stats what one fragment of weight 1 adds in a draw: pixels += 1; wmax = max(wmax, 0x3F800000);
 * wsum += 1 << 24.  GS4D_CQ_REMOVE sets row i to {0, 0, 0}.  Rows of records that do not take part keep their bits; no byte beyond row n - 1, no
 * byte of data and no byte of mask is written; nothing depends on the order in which anything runs.  On a zeroed table each ADD call adds at most
 * one to pixels: after k calls the rule {1, 0, 0, 0} gives their union, {k, 0, 0, 0} their intersection, and REMOVE subtracts.  Rows also add on
 * top of what draws and gs4d_count_ids put there.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: query == NULL; an unknown test bit or op; reserved != 0; n > 0xFFFFFFFF; data or stats
 * not a live buffer; data smaller than 96 n bytes; stats smaller than 16 n bytes; mask neither 0 nor a live buffer; mask given without
 * GS4D_CQ_SCREEN; mask smaller than w * h bytes; with GS4D_CQ_SCREEN a rectangle that is empty or not inside the image; any two of the three
 * buffers being the same buffer.  n == 0 with otherwise valid arguments is a no-op.  Box ends, sphere, frame, matrices, t and the depth range are
 * data, not errors: hostile values select what the lines above say they select.
 *
 * Ordering.  stats is handled exactly as in gs4d_count_ids: draws that add to it (gs4d_set_record_stats), issued before the call on any frame
 * lane, are settled first, re-runs included; the call is a kernel write that keeps the contents, and later draws, other lanes and the host order
 * themselves behind it.  data and mask are buffers the call reads (gs4d_record_time_spans' data, gs4d_count_ids' mask): a later write of either
 * waits for the kernel.  A queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first.  The kernel is queued on the
 * current frame lane; the call returns at once and starts no frame; it needs no frame and no outputs mode.  gs4d_buffer_invalidate hand-offs of
 * all three buffers are honoured.  If the SoA shadow of data is current the kernel reads the shadow's planes, which hold the same bits, instead of
 * the records; the call never builds or invalidates a shadow (gs4d_debug_shadow_builds does not move).
 *
 * Out of scope: per-pixel footprint selection (records whose quad merely touches the region); brush strokes as anything but a mask; 72-byte quad
 * vertices and 48-byte 2D records; more than one volume per call; a tie-break of the centre using floats 11, 15 and 19. */
enum { GS4D_CQ_BOX = 1, GS4D_CQ_SPHERE = 2, GS4D_CQ_SCREEN = 4, GS4D_CQ_FRAME = 8, GS4D_CQ_SKIP_HIDDEN = 16, GS4D_CQ_SKIP_DEAD = 32 };
enum { GS4D_CQ_ADD = 0, GS4D_CQ_REMOVE = 1 };
typedef struct gs4d_centre_query {
    uint32_t tests;        /* OR of GS4D_CQ_*; any other bit: GS4D_E_INVALID            */
    uint32_t op;           /* GS4D_CQ_ADD or GS4D_CQ_REMOVE                             */
    float    t;            /* the time the centre is taken at                           */
    uint32_t reserved;     /* must be 0                                                 */
    float    frame[12];    /* GS4D_CQ_FRAME: 3x4, column-major, world -> the volume's frame */
    float    box_lo[3], box_hi[3];
    float    sphere[4];    /* centre x y z, radius                                      */
    float    view[16], proj[16];   /* GS4D_CQ_SCREEN: as gs4d_set_uniform_mat4 takes them */
    int32_t  x, y, w, h;   /* GS4D_CQ_SCREEN: rectangle inside the image, row 0 = bottom, as gs4d_count_ids */
    float    depth_min, depth_max; /* GS4D_CQ_SCREEN: -z_view of the centre, the unit of the aux outputs */
} gs4d_centre_query;       /* 256 bytes */
GS4D_API int gs4d_count_centres(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_centre_query* query,
                                gs4d_buf mask /* 0: none; GS4D_CQ_SCREEN only */, gs4d_buf stats);

/* ---- where a selection is: bounds and centroid of selected records (no reference counterpart) ----
 * gs4d_count_ids, gs4d_count_centres and record statistics say WHICH records; gs4d_compact_records, gs4d_stat_cut, gs4d_edit_colours and
 * gs4d_transform_records act on them.  gs4d_measure_records says WHERE they are: how many, the box of their centres at time t, the box of what
 * they reach, and the sums their centroid comes from — the pivot of a rotate or scale gizmo (gs4d_host_affine4 rotates about the origin), the
 * camera's "frame selection" (gs4d_host_frame_box), the box drawn around a selection (gs4d_draw_lines), the box a follow-up gs4d_count_centres
 * query grows from — as one 96-byte gs4d_measure in a buffer.  gs4d_host_measure_records is this text as code.
 *
 * All arithmetic is float32, round to nearest, no contraction: every product and every sum is rounded on its own, in the order the parentheses
 * give; division and sqrtf are correctly rounded.  For record i < n of the 96-byte records in data, with p = floats 0..2, mu_t = float 3,
 * a = float 7, S[0][0], S[1][1], S[2][2] = floats 8, 13, 18, sig3 = floats 20..22, s44 = float 23:
 *
 * Selected.  Exactly the predicate of gs4d_edit_colours: stats == 0 selects every record; otherwise record i is selected iff row i of the
 * gs4d_record_stat table `stats` passes `rule`: (pixels >= min_pixels && wmax >= min_wmax && wsum >= min_wsum) != invert (GS4D_KEEP_INVERT).
 * A record that is not selected adds nothing to any field.
 *
 * Centre and skips (the text of gs4d_count_centres).
 *     dt = t - mu_t;   k = (1.0f / s44) * dt;   m = p + (k * sig3)   per component.
 * GS4D_MS_SKIP_HIDDEN skips a record iff !(a > 0).  GS4D_MS_SKIP_DEAD skips a record iff ((-0.5f * dt) * (1.0f / s44)) * dt < GS4D_TIME_DEAD_ARG;
 * a NaN is not skipped.  A selected record that is skipped adds 1 to `skipped` and nothing else.
 *
 * Placed.  A selected record that is not skipped is PLACED iff m[0], m[1] and m[2] are all finite.  One that is not placed adds 1 to `unplaced`
 * and nothing else.  The others are the MEASURED records: `count` is their number.
 *
 * Box.  lo[a] / hi[a] are the minimum / maximum of m[a] over the measured records in the total order of the key
 *     key(v) = bits(v) ^ (sign bit set ? 0xFFFFFFFF : 0x80000000)        compared as unsigned integers.
 * Under that key -0 < +0, so the BITS of a box end do not depend on the order in which anything is evaluated (with fminf they would: it may
 * return either zero).  count == 0: lo = {+inf}, hi = {-inf}.
 *
 * Reach.  Three standard deviations of the spatial variance conditioned on the time, per axis a:
 *     var = S[a][a] - ((sig3[a] * sig3[a]) * (1.0f / s44));   r = var > 0 ? 3.0f * sqrtf(var) : 0.0f        (a NaN gives 0)
 * m[a] - r enters ext_lo[a] and m[a] + r enters ext_hi[a], each only if it is finite, as a minimum / maximum under the same key order.  An axis
 * without a finite end holds +inf / -inf.
 *
 * Cell (once the box is known).  For a measured record and axis a:
 *     d = m[a] - lo[a];   e = hi[a] - lo[a];   g = (d / e) * 1048576.0f;   cell = g >= 0 ? (uint32) min(g, 1048576.0f) : 0
 * — the form of gs4d_spatial_order: a NaN from e == 0 or an overflowed e gives cell 0.  cell_sum[a] is the 64-bit integer sum of cell over the
 * measured records; it is below 2^52 and never overflows.
 *
 * Centre.  gs4d_host_measure_centre gives, in double precision, lo + (hi - lo) * (cell_sum / (count * 2^20)) per axis, rounded to float: the
 * centroid of the measured centres to within (hi - lo) * 2^-19 (each cell truncates by at most 2^-20 of the extent, and the float32 quotient
 * adds less than that again).  It is unweighted: every measured record counts once.
 *
 * Every field is a count, an integer sum or an extremum under a total order: the same inputs give the same 96 bytes, whatever runs first.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: query == NULL, an unknown flag, a non-zero reserved word; n > 0xFFFFFFFF; data or out
 * not a live buffer; data smaller than 96 n bytes; out smaller than 96 bytes; exactly one of stats / rule given; a rule with an unknown flag or
 * reserved != 0; stats not a live buffer or smaller than 16 n bytes; any two of the three buffers being the same buffer.  n == 0 with otherwise
 * valid arguments writes the empty measurement (zeros, lo = ext_lo = {+inf}, hi = ext_hi = {-inf}).  t is data, not an error.
 *
 * What is written: bytes 0..95 of out (reserved0, reserved1 as 0), nothing else; data and stats are never written.
 *
 * Ordering.  data is read as gs4d_count_centres reads its data: a later write of it waits for the kernels.  stats is read as gs4d_edit_colours
 * reads its table: draws that add to it (gs4d_set_record_stats), issued before the call on any frame lane, are settled first, re-runs included; a
 * draw issued afterwards that adds to it waits on the device until the kernels have read it, and a host write waits as it does for any reader.
 * out is an ordinary written buffer, as gs4d_stat_cut's out is.  A queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is
 * launched first.  The kernels are queued on the current frame lane; the call returns at once and starts no frame.  gs4d_buffer_invalidate
 * hand-offs of all three buffers are honoured.  The call never builds or invalidates a SoA shadow (gs4d_debug_shadow_builds does not move), and
 * it does not read one either: it reads the 96-byte records even where a shadow of data is current, because the diagonal of S lies in different
 * planes of each shadow layout — reading a shadow is out of scope here.
 *
 * Out of scope: weighted (alpha or wsum) centroids, second moments and oriented boxes; 72-byte quad vertices and 48-byte 2D records; building a
 * gs4d_affine4 row on the device.  (Transforming only the selected records in place, about this call's centre, is gs4d_transform_selected.) */
enum { GS4D_MS_SKIP_HIDDEN = 1, GS4D_MS_SKIP_DEAD = 2 };
typedef struct gs4d_measure_query {
    float    t;            /* the time the centres are taken at      */
    uint32_t flags;        /* OR of GS4D_MS_*; any other bit: GS4D_E_INVALID */
    uint32_t reserved[2];  /* must be 0                              */
} gs4d_measure_query;      /* 16 bytes */
typedef struct gs4d_measure {
    uint32_t count;        /* records measured: selected, not skipped, placed                                    */
    uint32_t unplaced;     /* selected, not skipped, centre not finite                                           */
    uint32_t skipped;      /* selected, left out by a GS4D_MS_SKIP_* flag                                        */
    uint32_t reserved0;    /* written as 0                                                                       */
    float    lo[3], hi[3];         /* box of the centres; count == 0: {+inf}, {-inf}                             */
    float    ext_lo[3], ext_hi[3]; /* box of centre -/+ reach; no finite end on an axis: +inf / -inf             */
    uint64_t cell_sum[3];  /* sum over the measured records of cell[a], units of 2^-20 of (hi[a] - lo[a])        */
    uint64_t reserved1;    /* written as 0                                                                       */
} gs4d_measure;            /* 96 bytes */
GS4D_API int gs4d_measure_records(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_measure_query* query,
                                  gs4d_buf stats /* 0: every record */, const gs4d_keep_rule* rule /* NULL iff stats == 0 */, gs4d_buf out);

/* ---- moving a selection: the selected records under a 4D affine map about a pivot, in place (no reference counterpart) ----
 * The step between the two calls above and gs4d_transform_records: grab what a statistics table selects and move, rotate or scale it where it
 * lies — a gizmo drag on part of a set — without reading a record or a measurement back.  gs4d_transform_records places a whole set into another
 * buffer and refuses src == dst; gs4d_transform_selected rewrites the selected records of `data` themselves, about a pivot the caller gives or
 * about the centre of a gs4d_measure that gs4d_measure_records has left in a buffer.  gs4d_host_transform_selected is this text as code.
 *
 * Selected.  Exactly the predicate of gs4d_edit_colours and gs4d_measure_records: stats == 0 selects every record i < n; otherwise record i is
 * selected iff row i of the gs4d_record_stat table `stats` passes `rule`: (pixels >= min_pixels && wmax >= min_wmax && wsum >= min_wsum) != invert
 * (GS4D_KEEP_INVERT).  There are no skip flags: hidden and dead records that are selected move with the rest, so an object stays whole.
 *
 * Pivot c.  flags == 0: there is no pivot.  GS4D_XS_PIVOT: c = pivot.  GS4D_XS_PIVOT_MEASURE: c is what gs4d_host_measure_centre gives for the 96
 * bytes at offset 0 of `measure` — per axis, in double precision, lo + (hi - lo) * ((double)cell_sum / ((double)count * 1048576.0)), rounded to
 * float; c = (0, 0, 0) when count == 0.  It is evaluated on the device, without contraction: double add, multiply, divide and the conversion from a
 * 64-bit integer are correctly rounded there, so the bits equal the host's.  The bytes of `measure` are data: hostile values (NaN or infinite ends,
 * a huge cell_sum) give what the line gives.
 *
 * The map.  All arithmetic is float32, round to nearest, no contraction, full products.  With l, o the fields of xf.xf, and p, S as in
 * gs4d_transform_records:
 *     q[a]  = pivot ? p[a] - c[a] : p[a]   (a = 0, 1, 2);     q[3] = p[3]
 *     u[r]  = ((((l[r]*q[0]) + (l[4+r]*q[1])) + (l[8+r]*q[2])) + (l[12+r]*q[3])) + o[r]      r = 0..3
 *     p'[r] = pivot ? u[r] + c[r] : u[r]   (r = 0, 1, 2);     p'[3] = u[3]
 *     Sigma' = (L Sigma) L^T, rgba copied:  the text of gs4d_transform_records, all 16 elements, nothing mirrored.
 * Without a pivot flag a selected record gets exactly the bits of gs4d_host_transform_records.  With a pivot flag the two extra operations are
 * always performed, also for c = 0: a -0 coordinate can then become +0 — that follows from the lines above and is no exception to them.  A word
 * that is a NaN on both sides may differ from the host's in sign and payload (the rule of gs4d_build_records).  Nothing depends on the order in
 * which anything runs on the device.
 *
 * What is written.  Only the 96 bytes of the selected records < n.  A record that is not selected, every byte of data beyond record n - 1 and
 * every byte of stats and measure are not written at all — which is more than keeping their bits.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: xf == NULL; a flags value other than 0, GS4D_XS_PIVOT or GS4D_XS_PIVOT_MEASURE;
 * n > 0xFFFFFFFF; data not a live buffer or smaller than 96 n bytes; exactly one of stats / rule given; a rule with an unknown flag or reserved != 0;
 * stats not a live buffer or smaller than 16 n bytes; GS4D_XS_PIVOT_MEASURE without a live `measure` of at least 96 bytes; measure != 0 without that
 * flag; any two of the three buffers being the same buffer.  n == 0 with otherwise valid arguments is a no-op.  The map and the pivot are data:
 * singular, non-finite and 1e30 rows give what the lines give.
 *
 * Ordering.  data is ordered as gs4d_transform_records orders its dst: draws that may still have to be run again from data are settled, and the
 * kernel waits, on the device, for the lanes whose draws or key generation still read data or its shadow.  stats is ordered as gs4d_edit_colours
 * orders its table: draws that add to it, issued before the call on any frame lane, are settled first, re-runs included; a draw issued afterwards
 * that adds to it waits on the device until the kernel has read it.  measure is a buffer the call reads: the call orders itself, on the device,
 * behind the gs4d_measure_records kernels that wrote it — no gs4d_finish and no read-back in between — and a later write of measure waits for this
 * call.  A queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first.  The kernel is queued on the current frame lane;
 * the call returns at once and starts no frame.  gs4d_buffer_invalidate hand-offs of all three buffers are honoured.
 *
 * The write counts as a full write of data, like gs4d_transform_records', whatever the table turns out to select: the buffer's version moves, what
 * a sort index was sorted by is forgotten, and the next draw or gs4d_keygen rebuilds the SoA shadow once (gs4d_debug_shadow_builds goes up by
 * exactly one per call followed by a draw).  The call order per frame is (shade) -> (edit) -> transform_selected -> keygen -> sort_pairs -> draw.
 *
 * The caller's other tables — the notes of gs4d_transform_records, for the selected rows only: time spans are to be recomputed when L touches
 * time; SH tables are not rotated, and gs4d_rotate_sh does not serve a selection (it has no rule operand: rotate a compacted copy of the
 * selected rows, or pose with a bind table, instead); the key-order note for a time scale still applies; statistics, spatial order and kept_index rows are
 * unaffected, because no record moves in memory.
 *
 * Out of scope: patching the SoA shadow instead of rebuilding it; one transform per record; a time component of the pivot; weighted pivots;
 * 72-byte quad vertices and 48-byte 2D records; duplicating a selection, which is gs4d_compact_records followed by gs4d_transform_records. */
enum { GS4D_XS_PIVOT = 1, GS4D_XS_PIVOT_MEASURE = 2 };
typedef struct gs4d_selection_xf {
    gs4d_affine4 xf;      /* the map, as a row of gs4d_transform_records' table            */
    float    pivot[3];    /* GS4D_XS_PIVOT: the pivot c; otherwise ignored                  */
    uint32_t flags;       /* 0, GS4D_XS_PIVOT or GS4D_XS_PIVOT_MEASURE; anything else: GS4D_E_INVALID */
} gs4d_selection_xf;      /* 96 bytes */
GS4D_API int gs4d_transform_selected(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_selection_xf* xf,
                                     gs4d_buf stats /* 0: every record */, const gs4d_keep_rule* rule /* NULL iff stats == 0 */,
                                     gs4d_buf measure /* GS4D_XS_PIVOT_MEASURE: a gs4d_measure at offset 0; otherwise 0 */);

/* ---- records relative to each other: how many source records lie within a radius of each record (no reference counterpart) ----
 * Every selection above is against a fixed region.  gs4d_count_neighbours counts, for every record, the records of a SOURCE set whose centre at
 * time t lies within r of its own, and writes the counts as rows of a gs4d_record_stat table — which makes two editor tools out of the calls that
 * exist.  Grow a selection ("what lies within r of what I have selected"): source = the selection's table with its rule, GS4D_NB_COUNT_SELF, into
 * a zeroed table B; B with the rule {1, 0, 0} is then a superset of the part of the selection that takes part and holds everything within r of
 * that part, and calling again with B as the source grows further.  Isolated records, the floaters of a trained set ("fewer than k neighbours
 * within r"): source == 0 into a zeroed table, then the rule {k, 0, 0} with GS4D_KEEP_INVERT for gs4d_compact_records (delete) or
 * gs4d_edit_colours (hide); a cap of k is enough, and it is what keeps dense regions cheap.  gs4d_stat_cut over pixels gives the K most crowded
 * records.  gs4d_host_count_neighbours is this text as code: the brute-force double loop.
 *
 * All arithmetic is float32, round to nearest, no contraction: every product and every sum is rounded on its own, in the order the parentheses
 * give; division is correctly rounded (the convention of gs4d_count_centres).  For record i < n of the 96-byte records in data, with
 * p = floats 0..2, mu_t = float 3, a = float 7, sig3 = floats 20..22, s44 = float 23:
 *
 * Centre (the text of gs4d_count_centres).
 *     dt = t - mu_t;   k = (1.0f / s44) * dt;   m_i = p + (k * sig3)   per component.
 *
 * Takes part.  Record i takes part iff it is not skipped by GS4D_NB_SKIP_HIDDEN, which skips iff !(a > 0); it is not skipped by
 * GS4D_NB_SKIP_DEAD, which skips iff ((-0.5f * dt) * (1.0f / s44)) * dt < GS4D_TIME_DEAD_ARG (a NaN is not skipped); and m_i[0], m_i[1], m_i[2]
 * are all finite.  A record that does not take part is nobody's neighbour, and its own row keeps its bits.
 *
 * Source.  Record j is a source iff it takes part and is selected by exactly the predicate of gs4d_edit_colours: source == 0 selects every
 * record; otherwise row j of the gs4d_record_stat table `source` must pass `rule`: (pixels >= min_pixels && wmax >= min_wmax &&
 * wsum >= min_wsum) != invert (GS4D_KEEP_INVERT).
 *
 * Near.  With the difference taken per component, d = m_i - m_j, the pair (i, j) is near iff
 *     ((d.x * d.x) + (d.y * d.y)) + (d.z * d.z) <= r * r.
 * The test is symmetric in i and j.
 *
 * Count.  For a record i that takes part,
 *     c_i = min(cap, #{ j < n : j is a source, j near i, and (j != i or GS4D_NB_COUNT_SELF) }).
 * With GS4D_NB_COUNT_SELF a record that is a source counts itself.  Every record < n that takes part is a query, selected or not.
 *
 * The row.  If c_i >= 1, row i of stats gets what c_i fragments of weight 1 add in a draw: pixels += c_i; wmax = max(wmax, 0x3F800000);
 * wsum += (uint64) c_i << 24 (pixels modulo 2^32, wsum modulo 2^64, as in gs4d_count_centres).  If c_i == 0, or i does not take part, the row is
 * not written.  The call ADDS: nothing zeroes the table.  No byte beyond row n - 1 is written, and no byte of data or source is written.  Every
 * field is an integer that depends on a set and not on an order: the same inputs give the same bytes, whatever runs first.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: query == NULL; an unknown flag; a non-zero reserved word; cap == 0; a radius that is
 * not finite or not above 0, or whose float32 square r * r is not finite or is below FLT_MIN (that is 2^-63 <= r < 2^64: it keeps r * r a normal
 * number, which the exactness of the search structure rests on); n >= 0xFFFFFFFF (the sort's limit, as in gs4d_spatial_order); data or stats not a live buffer;
 * data smaller than 96 n bytes; stats smaller than 16 n bytes; exactly one of source / rule given; a rule with an unknown flag or reserved != 0;
 * source not a live buffer or smaller than 16 n bytes; any two of the three buffers being the same buffer.  n == 0 with otherwise valid
 * arguments is a no-op.  t is data, not an error.
 *
 * Ordering.  data is read as gs4d_count_centres reads its data: a later write of it waits for the kernels.  source is read as gs4d_edit_colours
 * reads its table: draws that add to it (gs4d_set_record_stats), issued before the call on any frame lane, are settled first, re-runs included; a
 * draw issued afterwards that adds to it waits on the device until the kernels have read it.  stats is a kernel write that keeps the contents,
 * exactly as in gs4d_count_centres.  A queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first.  The kernels are
 * queued on the current frame lane; the call returns at once and starts no frame.  gs4d_buffer_invalidate hand-offs of all three buffers are
 * honoured.  The call reads the 96-byte records: it never builds, reads or invalidates a SoA shadow (gs4d_debug_shadow_builds does not move).
 *
 * Cost.  The device gives the brute-force result without the brute-force work: the sources are hashed by the cell of edge about 2 r their centre
 * lies in, and a record looks only at the cells its ball can reach — at most 27, usually 8 (DESIGN.md §4 has the structure and the proof that
 * it misses nothing).  The cost therefore depends on the data: a query costs the population of those cells.  Many sources inside one cell of
 * edge 2 r cost O(candidates) per query even with a small cap, because candidates that are not near do not count towards it.  The lane keeps
 * scratch of about 24 n bytes plus a bucket table of 8 bytes for each of 2 n .. 4 n buckets (at least 256), beside the sort's.  Environment, read
 * at gs4d_create: GS4D_NEIGHBOURS_PHASES=1, 2 or 3 makes the call stop behind its key, sort or bucket-table phase — a measurement hook
 * (tools/neighbours_cost.py): stats is then not written.
 *
 * Out of scope: reading a SoA shadow; a query-side selection (every record that takes part is a query); distances that use the covariance
 * (Mahalanobis, overlap of extents); 72-byte quad vertices and 48-byte 2D records; source == stats.  (Connected components, meaning growing
 * to a fixed point in one call, are gs4d_label_components below; the k nearest sources and their distances are gs4d_nearest_neighbours.) */
enum { GS4D_NB_SKIP_HIDDEN = 1, GS4D_NB_SKIP_DEAD = 2, GS4D_NB_COUNT_SELF = 4 };
typedef struct gs4d_neighbour_query {
    float    t;           /* the time the centres are taken at                                  */
    float    radius;      /* r                                                                  */
    uint32_t cap;         /* the count saturates here; >= 1                                     */
    uint32_t flags;       /* OR of GS4D_NB_*; any other bit: GS4D_E_INVALID                     */
    uint32_t reserved[4]; /* must be 0                                                          */
} gs4d_neighbour_query;   /* 32 bytes */
GS4D_API int gs4d_count_neighbours(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_neighbour_query* query,
                                   gs4d_buf source /* 0: every record */, const gs4d_keep_rule* rule /* NULL iff source == 0 */,
                                   gs4d_buf stats);

/* ---- connected clusters of a record set: which object a record belongs to (no reference counterpart) ----
 * gs4d_count_neighbours takes one radius step.  gs4d_label_components grows to the fixed point in one call: it labels every member of a record set
 * with the smallest record index of its connected component, where two members are linked iff they are near in the sense of
 * gs4d_count_neighbours, and — optionally — writes the size of its component into every member's row of a gs4d_record_stat table.  Two editor
 * tools follow.  Select connected ("the object this splat belongs to"): gs4d_count_labels marks every record whose label a seed selection
 * touches.  Floater clumps ("clusters of fewer than k records"): cap = k into a zeroed table, then the rule {k, 0, 0} with GS4D_KEEP_INVERT for
 * gs4d_compact_records or gs4d_edit_colours — five records 0.1 r apart and far from everything else each have four neighbours, but a cluster of
 * five.  gs4d_host_label_components is this text as code: the brute-force double loop with a sequential union–find.
 *
 * Centre, Takes part and Near are the texts of gs4d_count_neighbours, word for word (float32, no contraction; GS4D_CC_SKIP_HIDDEN and
 * GS4D_CC_SKIP_DEAD are GS4D_NB_SKIP_HIDDEN and GS4D_NB_SKIP_DEAD).
 *
 * Member.  Record i < n is a member iff it takes part and is selected by exactly the predicate of gs4d_edit_colours: source == 0 selects every
 * record; otherwise row i of the table `source` must pass `rule`.  A non-member links nothing: a chain whose middle record is hidden (with
 * GS4D_CC_SKIP_HIDDEN), dead at t (GS4D_CC_SKIP_DEAD), of a non-finite centre or unselected is two components.
 *
 * Graph.  Members i != j are linked iff the pair is near: ((d.x * d.x) + (d.y * d.y)) + (d.z * d.z) <= r * r, d = m_i - m_j per component.  The
 * components are the connected components of that graph; a member without a link is a component of one.
 *
 * Label.  labels is n uint32 words.  For a member, labels[i] = the smallest record index in its component (its own, iff it is that record); for
 * a non-member, labels[i] = GS4D_ID_NONE.  All n words are written; nothing beyond word n - 1 is.
 *
 * The row, only if stats != 0.  For a member i, c_i = min(cap, size of its component) >= 1, and row i of stats gets what c_i fragments of weight 1
 * add in a draw, exactly as in gs4d_count_neighbours: pixels += c_i; wmax = max(wmax, 0x3F800000); wsum += (uint64) c_i << 24.  A non-member's row
 * keeps its bits.  The call ADDS: nothing zeroes the table.  No byte beyond row n - 1 is written, and no byte of data or source is written.
 * Every output depends on a set and not on an order: the same inputs give the same bytes, whatever runs first.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: the list of gs4d_count_neighbours (query == NULL; a flag other than GS4D_CC_*; a non-zero
 * reserved word; cap == 0; a radius outside 2^-63 <= r < 2^64; n >= 0xFFFFFFFF; data not a live buffer or smaller than 96 n bytes; exactly one of
 * source / rule given; a rule with an unknown flag or reserved != 0; source not a live buffer or smaller than 16 n bytes); labels not a live buffer
 * or smaller than 4 n bytes (labels may not be 0); stats, when given, not a live buffer or smaller than 16 n bytes; any two of the four buffers
 * being the same buffer.  n == 0 with otherwise valid arguments is a no-op.  t is data, not an error.
 *
 * Ordering.  As in gs4d_count_neighbours: data and source are read, and draws that add to source, issued before the call on any frame lane, are
 * settled first; a draw issued afterwards that adds to it waits on the device until the kernels have read it.  labels is a kernel write of all n
 * words.  stats is a kernel write that keeps the contents.  A queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched
 * first.  The kernels are queued on the current frame lane; the call returns at once and starts no frame.  gs4d_buffer_invalidate hand-offs of
 * all four buffers are honoured.  The call reads the 96-byte records: it never builds, reads or invalidates a SoA shadow.
 *
 * Cost.  The hashed grid of gs4d_count_neighbours (keys, sort, bucket table), then a lock-free union–find over the same walk of at most 27 cells:
 * every near pair is united once, by its larger index (DESIGN.md §4 has the kernels and why the labels are unique though the order of the unions
 * is not).  The walk is that of gs4d_count_neighbours without a cap: many members inside one cell of edge 2 r cost O(candidates) per member.  The
 * lane's scratch is that of gs4d_count_neighbours; GS4D_NEIGHBOURS_PHASES does not apply.  Every loop of the union–find carries a trip bound; if
 * one ever runs out the lane's device-side check is raised and gs4d_finish reports it.
 *
 * gs4d_count_labels: what a selection touches, by label.  A label L is hit iff L < n and some j < n has labels[j] == L and row j of the table
 * `seeds` passing `rule`.  Row i < n of stats gets one fragment of weight 1 (the row update of gs4d_count_centres) iff labels[i] is hit; every
 * other row keeps its bits.  A word >= n counts as GS4D_ID_NONE, whatever it holds: it is neither hit nor does it hit, and no byte outside the
 * buffers is touched.  Labels are computed once per edit state and clicked on many times, hence a call of its own.  gs4d_host_count_labels is
 * this text as code.  GS4D_E_INVALID, with nothing queued and nothing written: n > 0xFFFFFFFF; labels, seeds or stats not a live buffer; labels
 * smaller than 4 n bytes; seeds or stats smaller than 16 n bytes; rule == NULL, or with an unknown flag or reserved != 0; any two of the three
 * buffers being the same buffer.  n == 0 is a no-op.  Ordering: labels is read; seeds is read as gs4d_edit_colours reads its table (draws that
 * add to it are settled first); stats is a kernel write that keeps the contents.  The lane keeps n words of scratch.
 *
 * Out of scope: components over a SoA shadow; links that use the covariance; components of the kNN graph; relabelling incrementally after an edit;
 * 72-byte quad vertices and 48-byte 2D records. */
enum { GS4D_CC_SKIP_HIDDEN = 1, GS4D_CC_SKIP_DEAD = 2 };
typedef struct gs4d_component_query {
    float    t;           /* the time the centres are taken at                                  */
    float    radius;      /* r: two members are linked iff they are near                        */
    uint32_t cap;         /* the size written to a row saturates here; >= 1                     */
    uint32_t flags;       /* OR of GS4D_CC_*; any other bit: GS4D_E_INVALID                     */
    uint32_t reserved[4]; /* must be 0                                                          */
} gs4d_component_query;   /* 32 bytes */
GS4D_API int gs4d_label_components(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_component_query* query,
                                   gs4d_buf source /* 0: every record */, const gs4d_keep_rule* rule /* NULL iff source == 0 */,
                                   gs4d_buf labels /* n uint32 */, gs4d_buf stats /* 0: labels only */);
GS4D_API int gs4d_count_labels(gs4d_ctx* ctx, gs4d_buf labels, size_t n, gs4d_buf seeds, const gs4d_keep_rule* rule, gs4d_buf stats);

/* ---- the k nearest sources of every record: a neighbour list and a density-adaptive distance (no reference counterpart) ----
 * gs4d_count_neighbours says how many sources are near a record and gs4d_label_components which cluster it belongs to; both discard WHICH sources
 * those are.  gs4d_nearest_neighbours keeps them: for every record the k nearest sources within r, as a row of {record, dist2} hits in a table of
 * the caller's stride, and — optionally — the squared distance to the last of them in a gs4d_record_stat table.  Three tools follow.  Scales for
 * records built from points: the mean dist2 of the 3 nearest points is what 3DGS-style pipelines initialise the scales of gs4d_build_records from.
 * Floaters where the density varies: one radius for gs4d_count_neighbours either marks a sparse background or finds nothing in it; the distance to
 * the k-th neighbour adapts.  A neighbour list per record: what smoothing, colour propagation from a selection and as-rigid-as-possible drags start
 * from.  gs4d_host_nearest_neighbours is this text as code: the brute-force double loop.
 *
 * Centre, Takes part, Source and Near are the texts of gs4d_count_neighbours, word for word: float32, round to nearest, no contraction;
 * GS4D_NN_SKIP_HIDDEN and GS4D_NN_SKIP_DEAD are GS4D_NB_SKIP_HIDDEN and GS4D_NB_SKIP_DEAD; the pair (i, j) is near iff
 *     ((d.x * d.x) + (d.y * d.y)) + (d.z * d.z) <= r * r,   d = m_i - m_j per component, r * r rounded once.
 *
 * Candidates.  The candidates of a record i that takes part are the sources j < n near i, with j != i unless GS4D_NN_INCLUDE_SELF.  Each has
 *     dist2 = ((d.x * d.x) + (d.y * d.y)) + (d.z * d.z),
 * the very value `near` compared.  It is >= +0 and not a NaN, so its bit pattern is in float order.
 *
 * Order.  Candidates are ordered by (bits(dist2), j) ascending: by distance, equal distances by record index.  The key is unique per j, so the
 * first k candidates are a property of the set; nothing depends on the order in which anything runs.
 *
 * Row.  Row i is the hit_stride bytes at hits + i * hit_stride.  Its first k gs4d_neighbour_hit slots receive the first f_i = min(k, #candidates)
 * candidates in that order, {j, dist2}; the remaining ones of the k receive {GS4D_ID_NONE, +inf}.  A record that does not take part gets k such
 * empty slots.  All n rows are written; bytes of a row past 8 k keep their contents, and nothing past row n - 1 is written.  hit_stride follows
 * the stride rule of every record call — a multiple of 16 from 16 to 1024 — with hit_stride >= 8 k: gs4d_gather_records, gs4d_compact_records and
 * gs4d_compact_time_window then carry the table along with the records.  k is 1 .. 16.
 *
 * The row of stats, only if stats != 0.  A record that takes part and has f_i >= 1 gets: pixels += f_i; wmax = max(wmax, bits(dist2 of its last
 * filled slot)), compared as the unsigned words they are; wsum += (uint64) f_i << 24.  Every other row keeps its bits.  The call ADDS: nothing
 * zeroes the table.  Into a zeroed table this buys three selections without another kernel: the rule {k, 0, 0} with GS4D_KEEP_INVERT selects
 * "fewer than k sources within r" (gs4d_count_neighbours' floaters); min_wmax = bits(x) selects "k-th neighbour — or the last one found — farther
 * than about sqrt(x)" (>= in bits); and gs4d_stat_cut over GS4D_STAT_WMAX gives the threshold for "the K records whose k-th neighbour is
 * farthest", ready for gs4d_compact_records or gs4d_edit_colours.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: the list of gs4d_count_neighbours with k == 0 || k > 16 in the place of cap == 0
 * (query == NULL; a flag other than GS4D_NN_*; a non-zero reserved word; a radius outside 2^-63 <= r < 2^64; n >= 0xFFFFFFFF; data not a live
 * buffer or smaller than 96 n bytes; exactly one of source / rule given; a rule with an unknown flag or reserved != 0; source not a live buffer
 * or smaller than 16 n bytes); hits not a live buffer, or smaller than n * hit_stride bytes; a hit_stride that is not a multiple of 16 in
 * 16 .. 1024 or is below 8 k; stats, when given, not a live buffer or smaller than 16 n bytes; any two of the four buffers being the same buffer.
 * n == 0 with otherwise valid arguments is a no-op.  t is data, not an error.
 *
 * Ordering.  As in gs4d_label_components: data and source are read, and draws that add to source, issued before the call on any frame lane, are
 * settled first; a draw issued afterwards that adds to it waits on the device until the kernels have read it.  hits is a kernel write.  stats is
 * a kernel write that keeps the contents.  A queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first.  The kernels
 * are queued on the current frame lane; the call returns at once and starts no frame.  gs4d_buffer_invalidate hand-offs of all four buffers are
 * honoured.  The call reads the 96-byte records: it never builds, reads or invalidates a SoA shadow.
 *
 * Cost.  The hashed grid of gs4d_count_neighbours (keys, sort, bucket table), then one walk of at most 27 cells per record without a cap and
 * without an early exit — every candidate that is near competes — with the k best kept in registers, and one scattered row write (DESIGN.md §4 has
 * the kernel, the measured times beside gs4d_count_neighbours, and why the rows are unique though the walk order is not).  The lane's scratch is
 * that of gs4d_count_neighbours; GS4D_NEIGHBOURS_PHASES does not apply.
 *
 * Out of scope: a search without a radius (a record with fewer than k sources within r gets fewer hits — the caller chooses r); k > 16;
 * distances that use the covariance; reading a SoA shadow; 72-byte quad vertices and 48-byte 2D records. */
enum { GS4D_NN_SKIP_HIDDEN = 1, GS4D_NN_SKIP_DEAD = 2, GS4D_NN_INCLUDE_SELF = 4 };   /* the values of GS4D_NB_* */
typedef struct gs4d_nearest_query {
    float    t;           /* the time the centres are taken at                                  */
    float    radius;      /* r: only sources that are near compete                              */
    uint32_t k;           /* hits per row; 1 .. 16                                              */
    uint32_t flags;       /* OR of GS4D_NN_*; any other bit: GS4D_E_INVALID                     */
    uint32_t reserved[4]; /* must be 0                                                          */
} gs4d_nearest_query;     /* 32 bytes */
typedef struct gs4d_neighbour_hit {
    uint32_t record;      /* the source's record index, or GS4D_ID_NONE: an empty slot          */
    float    dist2;       /* the squared distance `near` compared, or +inf: an empty slot       */
} gs4d_neighbour_hit;     /* 8 bytes */
GS4D_API int gs4d_nearest_neighbours(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_nearest_query* query,
                                     gs4d_buf source /* 0: every record */, const gs4d_keep_rule* rule /* NULL iff source == 0 */,
                                     gs4d_buf hits, size_t hit_stride, gs4d_buf stats /* 0: hits only */);

/* ---- a label per record from a 4D cell grid (no reference counterpart) ----
 * gs4d_cell_labels writes labels[i], i < n: the cell of record i of the 96-byte records in data in a regular grid of space-time.  The cell of axis
 * a (x, y, z, t) is taken from the record's REST mean, words 0..3: there is no time conditioning.  gs4d_host_cell_labels is this text as code.
 *   An axis with dims[a] == 1 has cell 0; its coordinate, lo[a] and edge[a] are not looked at (a static or sliced set: dims[3] = 1).
 *   Otherwise  g = (p - lo[a]) / edge[a]  in float32, the difference and the quotient each rounded on its own.
 *       g a NaN:  the record's label is GS4D_ID_NONE, whatever the other axes give.
 *       else      cell = g >= 0 ? (uint32_t)fminf(floorf(g), (float)(dims[a] - 1)) : 0 — the border cells take what lies outside.
 *   label = ((c3 * dims[2] + c2) * dims[1] + c1) * dims[0] + c0.
 * All n words are written and nothing else; data is only read, the 16-byte mean of each record.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: grid == NULL; a dims[a] of 0 or above 65536; a product of the four above 0xFFFFFFFE
 * (every label is below GS4D_ID_NONE); an edge[a] that is not finite and > 0 on an axis with dims[a] > 1; a non-zero reserved word;
 * n > 0xFFFFFFFF; data or labels not a live buffer, the same buffer, data smaller than 96 n bytes or labels smaller than 4 n bytes.  lo is data.
 * n == 0 with otherwise valid arguments is a no-op.
 *
 * Ordering: data is read, labels is a kernel write of n words; a queued gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched
 * first; one launch of one thread per record on the current frame lane; the call returns at once and starts no frame.  It reads the 96-byte
 * records: it never builds, reads or invalidates a SoA shadow. */
typedef struct gs4d_cell_grid {
    float    lo[4];        /* the low corner of cell 0 along x, y, z, t                              */
    float    edge[4];      /* the cell's edge along each axis; finite and > 0 where dims[a] > 1      */
    uint32_t dims[4];      /* cells along each axis, 1 .. 65536; the product at most 0xFFFFFFFE      */
    uint32_t reserved[4];  /* must be 0                                                              */
} gs4d_cell_grid;          /* 64 bytes */
GS4D_API int gs4d_cell_labels(gs4d_ctx* ctx, gs4d_buf data, size_t n, const gs4d_cell_grid* grid, gs4d_buf labels /* uint32[n] */);

/* ---- one moment-matched record per labelled group: a coarser level of detail (no reference counterpart) ----
 * Frame time follows the number of records.  gs4d_merge_records replaces the members of every group of equal label by ONE Gaussian with the group's
 * first and second moments — the merge step of the level-of-detail hierarchies of 3DGS — and writes the smaller set.  The labels come from
 * gs4d_cell_labels (a coarser set for what is far away), from gs4d_label_components ("collapse this clump into one splat") or from the caller.
 * The result is inexact by design; the definition below is exact: gs4d_host_merge_records is this text as code, and the device gives its bits.
 *
 * Area-time and mass, float32, every product, difference and sum rounded on its own in the order the parentheses give, sqrtf correctly rounded.
 * S(c,r) is float 8 + 4c + r of the record, Sxx = S(0,0), Syy = S(1,1), Szz = S(2,2), S44 = S(3,3):
 *     e2 = ((Sxx*Syy - S(1,0)*S(0,1)) + (Sxx*Szz - S(2,0)*S(0,2))) + (Syy*Szz - S(2,1)*S(1,2))
 *     area_time(rec) = sqrtf(S44 * e2)          mass(rec) = alpha * area_time(rec)          (alpha: float 7)
 * e2 is the second elementary symmetric polynomial of the spatial block, a proxy of the mean projected area: a flat disc (one scale 0) has
 * e2 > 0 where a determinant would give 0.  S44 is the time extent.  A needle (two scales 0) has no area: where its e2 cancels to <= 0 in
 * float32 it has no mass and is no member.
 *
 * Member.  Record i < n is a member iff labels[i] != GS4D_ID_NONE; stats == 0 or row i of the gs4d_record_stat table `stats` passes `rule`
 * (the predicate of gs4d_edit_colours); a_i = mass(rec_i) is finite and > 0; and words 0..6 and 8..23 are all finite.  Everything a member adds
 * is finite: no NaN arises, and the outputs are compared bit for bit without an exemption.  A non-member is counted in left_out and appears
 * nowhere in dst.
 *
 * Groups.  A group is the set of members with one label.  Groups are numbered g = 0, 1, ... in ascending label.  The members of a group are taken
 * in ascending record index, k = 0, 1, ....
 *
 * A group of one member gives that member's 24 words as they are.
 *
 * A larger group accumulates in double, every operation rounded on its own, with the origin c = words 0..3 of member 0, d = (double)mu_k - (double)c
 * (four components) and a = (double)a_k.  Member k adds into slot s = k mod 8:
 *     W[s]       += a
 *     M[s][r]    += a * d[r]                                       r = 0..3
 *     Q[s][c][r] += a * ((double)S(c,r) + d[r] * d[c])             r <= c: the stored triangle, read from float 8 + 4c + r
 *     C[s][j]    += a * (double)rgb[j]                             j = 0..2 (floats 4..6)
 * The eight slots — an empty one is +0.0 — are always combined as ((0+1)+(2+3))+((4+5)+(6+7)), field by field.  Then
 *     m[r] = M[r] / W                     mu_out[r] = (float)((double)c[r] + m[r])
 *     S_out(c,r) = S_out(r,c) = (float)(Q[c][r] / W - m[r] * m[c])
 *     rgb_out[j] = (float)(C[j] / W)
 *     v = W / (double)area_time(out), taken on the output words just written
 *     alpha_out = v < (double)alpha_max ? (float)v : alpha_max
 * A zero or NaN area gives alpha_max.  Mass is preserved unless the clamp acts.  The eight interleaved slots with a fixed tree are what lets
 * eight lanes share a group and still give the host's bits.  Tables with a row per record — SH tables — are merged by gs4d_merge_rows, below,
 * under member_group.
 *
 * Outputs.  Group g writes slot g of dst (96 bytes) and groups[g] = {label, size, first = its smallest member index, 0}.  member_group[i], i < n,
 * is g for a member of group g and GS4D_ID_NONE for a non-member: true group numbers, also beyond `written`.  count always receives
 * {groups, written = min(groups, capacity), members, left_out = n - members}, where capacity = min(dst bytes / 96, groups bytes / 16) over the
 * outputs given.  Slots >= capacity are never written and keep their bytes, the rule of gs4d_compact_records.  n == 0 writes {0, 0, 0, 0}.  No
 * byte of data, labels or stats is written.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: q == NULL; alpha_max not finite or not > 0; flags or a reserved word != 0;
 * n > 0xFFFFFFFE (the sort takes 2^32 - 2 keys at most); exactly one of stats / rule given; a rule with an unknown flag or reserved != 0; data,
 * labels, dst or count not a live buffer; stats, groups or member_group, when given, not a live buffer; data smaller than 96 n bytes, labels or
 * member_group smaller than 4 n bytes, stats smaller than 16 n bytes, count smaller than 16 bytes; any two of the buffers being the same buffer.
 *
 * Ordering.  data, labels and stats are read, the table as gs4d_measure_records reads its own: draws that add to it, issued before the call on
 * any frame lane, are settled first, and a draw issued afterwards that adds to it waits on the device until the kernels have read it.  dst is
 * written as gs4d_transform_records writes its own: draws that may still have to be run again from it are settled, and the call counts as a full
 * write — the next draw or gs4d_keygen rebuilds its SoA shadow once.  groups, member_group and count are kernel writes.  A queued gs4d_keygen /
 * gs4d_sort_pairs that names one of the buffers is launched first.  The kernels are queued on the current frame lane; the call returns at once
 * and starts no frame.  Read count with gs4d_buffer_read.
 *
 * Cost.  A key kernel, the library's stable 32-bit sort of the identity by key, a count / scan / scatter over the sorted keys, and a segmented
 * reduction with eight lanes per group.  The lane keeps about 12 n bytes of scratch beside the sort's.  A group of a million
 * members is walked by eight lanes: a documented corner.
 * SH tables are merged by gs4d_merge_rows, below.  Choosing a level per view at draw time is gs4d_lod_cut, over a forest of such levels. */
typedef struct gs4d_merge_query {
    float    alpha_max;    /* the clamp of a merged record's alpha; finite and > 0                   */
    uint32_t flags;        /* must be 0                                                              */
    uint32_t reserved[2];  /* must be 0                                                              */
} gs4d_merge_query;        /* 16 bytes */
typedef struct gs4d_merge_group { uint32_t label, size, first, reserved; } gs4d_merge_group;       /* 16 bytes */
typedef struct gs4d_merge_count { uint32_t groups, written, members, left_out; } gs4d_merge_count; /* 16 bytes */
GS4D_API int gs4d_merge_records(gs4d_ctx* ctx, gs4d_buf data, size_t n, gs4d_buf labels, const gs4d_merge_query* q,
                                gs4d_buf stats /* 0: every record */, const gs4d_keep_rule* rule /* NULL iff stats == 0 */,
                                gs4d_buf dst, gs4d_buf groups /* 0 ok */, gs4d_buf member_group /* 0 ok */, gs4d_buf count);

/* ---- merged rows of a table: the SH row of a merged record (no reference counterpart) ----
 * A trained set keeps its colour in an SH table that gs4d_shade_sh evaluates every frame.  That evaluation is linear in the coefficients before
 * its clamp, and gs4d_merge_records defines a merged colour as the mass-weighted mean of the members' colours: so the mass-weighted mean of the
 * members' rows is the SH row of a merged record.  gs4d_merge_rows is that mean over any float32 table with a row per record, under the
 * member_group a gs4d_merge_records call wrote (or any other grouping).  gs4d_host_merge_rows is this text as code, and the device gives its bits.
 *
 * The table.  Row i is the q->stride bytes at rows + i*stride; stride is a multiple of 16, 16 .. 1024 (the rule of gs4d_shade_sh), the same for
 * rows and dst.  Words 0 .. width-1 of a row (float32) are merged, 1 <= width <= stride / 4; the words at or past width are padding: never looked
 * at, whatever their bits.
 *
 * Weight.  With data given, a_i = mass(rec_i) of gs4d_merge_records, float32, and ok_i is that call's condition on the record: a_i finite and
 * > 0, words 0..6 and 8..23 finite.  With data == 0, a_i = 1.0f and ok_i holds: a plain mean of rows, for tables that are not colour.
 *
 * Member.  Record i < n is a member iff member_group[i] != GS4D_ID_NONE, ok_i, and words 0 .. width-1 of row i are all finite.  Everything a
 * member adds is finite: the outputs are compared bit for bit without an exemption.
 *
 * Groups.  A group is the set of members with one value g of member_group; the values need not be dense.  The members of a group are taken in
 * ascending record index, k = 0, 1, ....
 *
 * A group of one member gives words 0 .. width-1 of its member's row with their bits kept.
 *
 * A larger group accumulates in double, every operation rounded on its own, a = (double)a_k.  Member k adds into slot s = k mod 8:
 *     W[s]    += a
 *     R[s][j] += a * (double)row_k[j]                              j < width
 * The eight slots — an empty one is +0.0 — are combined as ((0+1)+(2+3))+((4+5)+(6+7)), then out[j] = (float)(R[j] / W).  This is the rule by
 * which gs4d_merge_records forms rgb_out: a table whose row is floats 4..6 of its record, merged under the member_group that call wrote, gives
 * that call's rgb_out bits for every group.
 *
 * Outputs.  Group g writes row dst_first + g of dst (computed in 64 bits): words 0 .. width-1 as above, the words from width to stride / 4 as
 * +0.0.  A row at or beyond capacity = dst bytes / stride is never written, and neither is the row of a g without members: both keep their bytes
 * (the capacity rule of gs4d_compact_records).  count always receives a gs4d_merge_count: groups = distinct values among the members, written =
 * those whose row lies below capacity, members, left_out = n - members.  n == 0 writes {0, 0, 0, 0}.  No byte of data, member_group or rows is
 * written.
 *
 * GS4D_E_INVALID, with nothing queued and nothing written: q == NULL; a stride that breaks the rule; width == 0 or 4 width > stride; flags or
 * reserved != 0; n > 0xFFFFFFFE (the sort takes 2^32 - 2 keys at most); dst_first > 0xFFFFFFFE; member_group, rows, dst or count — or data, when
 * given — not a live buffer; any two of the buffers being the same buffer; data smaller than 96 n bytes, member_group smaller than 4 n bytes, rows
 * smaller than n * stride bytes, count smaller than 16 bytes.  Every word of the buffers is data.
 *
 * Ordering.  data, member_group and rows are read.  dst and count are kernel writes; dst keeps the rows the call does not name.  A queued
 * gs4d_keygen / gs4d_sort_pairs that names one of the buffers is launched first.  The kernels are queued on the current frame lane; the call
 * returns at once and starts no frame.  It reads the 96-byte records: it never builds, reads or invalidates a SoA shadow.
 *
 * Cost.  The key kernel, sort and run starts of gs4d_merge_records, then a reduction with eight lanes per (group, 8 words of the row)
 * (DESIGN.md §4).  The lane keeps about 16 n bytes of scratch beside the sort's.
 *
 * gs4d_copy_rows: rows src_first .. src_first + m - 1 of src go to rows dst_first .. of dst, `stride` bytes each (the rule above) with their bits
 * kept, in 16-byte pieces, one launch: the table counterpart of gs4d_lod_append's record copy, which lays the rows of a forest out level by level.
 * src is read; dst is a kernel write that keeps the rest of its contents.  m == 0 with otherwise valid arguments is a no-op.  GS4D_E_INVALID, with
 * nothing queued and nothing written: a stride that breaks the rule; m, src_first or dst_first above 2^32 - 1; src or dst not a live buffer, or
 * the same buffer; src smaller than (src_first + m) * stride bytes, dst smaller than (dst_first + m) * stride bytes. */
typedef struct gs4d_rows_query {
    uint32_t stride;       /* bytes per row of rows AND of dst: a multiple of 16, 16 .. 1024 (the rule of gs4d_shade_sh) */
    uint32_t width;        /* float32 words of a row that are merged: 1 .. stride / 4                */
    uint32_t flags;        /* must be 0                                                              */
    uint32_t reserved;     /* must be 0                                                              */
} gs4d_rows_query;         /* 16 bytes */
GS4D_API int gs4d_merge_rows(gs4d_ctx* ctx, gs4d_buf data /* 0: unit weights */, size_t n, gs4d_buf member_group, gs4d_buf rows,
                             const gs4d_rows_query* q, gs4d_buf dst, size_t dst_first, gs4d_buf count);
GS4D_API int gs4d_copy_rows(gs4d_ctx* ctx, gs4d_buf src, size_t src_first, size_t m, size_t stride, gs4d_buf dst, size_t dst_first);

/* ---- the view's cut through a hierarchy of merged levels (no reference counterpart) ----
 * gs4d_merge_records builds one coarser level of a set.  A camera inside a large scene wants fine records near the eye and merged records far
 * away, chosen again every frame: gs4d_lod_append assembles the levels into a forest on the device, once, and gs4d_lod_cut walks the forest for a
 * camera and a time and writes the records to draw.  gs4d_host_lod_cut is the definition below as code, and the device gives its words.
 *
 * The forest is two buffers: nodes, N 96-byte records, and parent, N uint32; N <= 0xFFFFFFFE.  The nodes are laid out level by level: level 0, the
 * leaves (the full set), first, each coarser level behind it.  level_first[0 .. levels] gives the first node of every level: level_first[0] == 0,
 * the entries do not decrease, level_first[levels] == N, levels is 1 .. 16.  Node i of level k is a CHILD iff
 * level_first[k + 1] <= parent[i] && parent[i] < N; otherwise it is a ROOT — GS4D_ID_NONE, a parent in its own level or a lower one, a parent past
 * the end.  Parent words are data, never an error.  A parent lies in a strictly higher level, so a walk over the levels from the top down has
 * decided every parent when it reaches a child.
 *
 * gs4d_lod_append, one level per call.  nodes[first + j] receives the 96 bytes of level[j], j < m, with their bits kept (NaN payloads included);
 * parent[first + j] = GS4D_ID_NONE, j < m; with member_group given, parent[child_first + i] = member_group[i] < m ? first + member_group[i] :
 * GS4D_ID_NONE, i < c — a record gs4d_merge_records left out and a group beyond `written` become roots.  member_group == 0 requires c == 0: the
 * leaf level.  Nothing else is written.  m == 0 and c == 0 with otherwise valid arguments is a no-op.
 * GS4D_E_INVALID, with nothing queued and nothing written: child_first + c > first; first + m > 0xFFFFFFFE; level, nodes or parent — or
 * member_group, when given — not a live buffer; two arguments naming the same buffer; level smaller than 96 m bytes, member_group smaller than 4 c
 * bytes, nodes smaller than 96 (first + m) bytes, parent smaller than 4 (first + m) bytes; member_group == 0 with c != 0.
 * Ordering: level and member_group are read; nodes is written as gs4d_transform_records writes a dst with dst_first; parent is a kernel write that
 * keeps the rest of its contents.  One launch on the current frame lane; the records travel in 16-byte pieces, the parent words one by one (first
 * and child_first are any index: a run of words has no alignment to rely on).
 *
 * gs4d_lod_cut.  Fine — float32, every product and every sum rounded on its own in the order the parentheses give, no contraction, no square root:
 *     m     = the centre of the node at q.t: with dt = t - mu_t and k = (1 / S44) * dt, m = p + k * sig3 per component (floats 0..2, 3, 20..22, 23:
 *             the centre of gs4d_count_centres)
 *     d     = m - eye per component             dist2 = ((d.x*d.x) + (d.y*d.y)) + (d.z*d.z)
 *     n2    = near_dist * near_dist             e = dist2 > n2 ? dist2 : n2          (a NaN distance counts as near)
 *     v     = Sxx; if (Syy > v) v = Syy; if (Szz > v) v = Szz         (floats 8, 13, 18: the rest variances, which bound the conditional ones)
 *     fine  = v <= (ratio * ratio) * e
 * A NaN on either side of the last comparison is not fine.  ratio = 0 makes nothing with a positive extent fine; ratio = +inf makes everything
 * with a non-NaN extent fine at a distance e > 0.
 * State, the levels taken from the top down: a root is TESTED; a child is tested iff its parent's state is DESCEND, otherwise its state is STOP and
 * nothing of its record is looked at; a tested node is DRAW iff it is fine or it is a leaf (i < level_first[1]), otherwise DESCEND.  On every chain
 * of valid parent links exactly one node is DRAW: the topmost fine one, or the leaf — whether or not the extents grow towards the roots.
 * Outputs.  The DRAW nodes in ascending node index go to dst, 96 bytes each with their bits kept, their indices to cut_index; slots at or beyond
 * capacity = min(dst bytes / 96, cut_index bytes / 4) over the outputs given are never written and keep their bytes, the rule of
 * gs4d_compact_records.  count always receives {drawn, written = min(drawn, capacity), tested, drawn_leaves}; n == 0 writes {0, 0, 0, 0}.  With
 * stats given, every DRAW node adds one fragment of weight 1 to its row of the gs4d_record_stat table (n rows), the GS4D_CQ_ADD of
 * gs4d_count_centres; other rows keep their bits — gs4d_edit_colours (tint the levels) and the rest of the selection chain then act on the cut.
 * No byte of nodes or parent is written.
 * GS4D_E_INVALID, with nothing queued and nothing written: q == NULL; levels outside 1 .. 16; a level_first that is not as above; ratio a NaN or
 * below 0; near_dist not finite or below 0; flags or a reserved word != 0; n > 0xFFFFFFFE; nodes, parent or count not a live buffer; dst, cut_index
 * or stats, when given, not a live buffer; nodes smaller than 96 n bytes, parent smaller than 4 n bytes, stats smaller than 16 n bytes, count smaller
 * than 16 bytes; two arguments naming the same buffer.  eye, t and every word of the buffers are data.
 * Ordering.  nodes and parent are read.  dst is written as gs4d_transform_records writes its own: a full write, the next draw repacks its shadow
 * once.  cut_index and count are kernel writes; stats is handled exactly as gs4d_count_centres handles its table.  A queued gs4d_keygen /
 * gs4d_sort_pairs that names one of the buffers is launched first.  The kernels are queued on the current frame lane; the call returns at once and
 * starts no frame.  It reads the 96-byte records: it never builds or invalidates a SoA shadow.  The frame loop is
 * gs4d_lod_cut -> gs4d_keygen -> gs4d_sort_pairs -> draw on (dst, count.drawn), with count read back or dst sized for the worst case.
 * Cost.  One launch per level from the top down over a plane of one state byte per node in lane scratch (consecutive levels that fit one workgroup
 * together share a launch), then the three kernels of gs4d_compact_records over the plane.  A node whose parent is not DESCEND costs its parent
 * word, the parent's state byte and its own: the cost follows the cut, not the forest.
 * A forest's SH table has one row per node, the merged levels' rows from gs4d_merge_rows laid out with gs4d_copy_rows; gs4d_gather_records
 * through cut_index gives the rows of the cut, and the frame loop becomes gs4d_lod_cut -> gs4d_gather_records (rows) -> gs4d_shade_sh ->
 * gs4d_keygen -> gs4d_sort_pairs -> draw.
 * Out of scope: blending between a node and its children across the threshold; frustum tests
 * (gs4d_count_centres has the screen test); choosing the grids; a forest that skips the state plane. */
GS4D_API int gs4d_lod_append(gs4d_ctx* ctx, gs4d_buf level, size_t m,
                             gs4d_buf member_group /* 0 ok */, size_t child_first, size_t c,
                             gs4d_buf nodes, gs4d_buf parent, size_t first);
typedef struct gs4d_lod_query {
    float    eye[3];          /* camera position, world                                  */
    float    t;               /* the time the centres are taken at                       */
    float    ratio;           /* extent / distance at or below which a node is fine      */
    float    near_dist;       /* distances below it count as it; finite, >= 0            */
    uint32_t levels;          /* 1 .. 16                                                 */
    uint32_t flags;           /* must be 0                                               */
    uint32_t level_first[17];
    uint32_t reserved[3];     /* must be 0 */
} gs4d_lod_query;             /* 112 bytes */
typedef struct gs4d_lod_count { uint32_t drawn, written, tested, drawn_leaves; } gs4d_lod_count;   /* 16 bytes */
GS4D_API int gs4d_lod_cut(gs4d_ctx* ctx, gs4d_buf nodes, gs4d_buf parent, size_t n, const gs4d_lod_query* q,
                          gs4d_buf dst /* 0 ok */, gs4d_buf cut_index /* 0 ok */, gs4d_buf stats /* 0 ok */, gs4d_buf count);

/* ---- measurement / test hooks ---- */
GS4D_API int gs4d_set_profiling(gs4d_ctx* ctx, int stage_mask);                   /* bit (1 << GS4D_T_x) times stage x; 0 = off, 0x3F = every stage; bits 8..15 = k: time only every k-th frame (0 = every frame).
                                                                                      Each timed stage costs two event records in a timed frame (they break back-to-back kernel dispatch: ~2 us each on the device) */
GS4D_API int gs4d_get_timings(gs4d_ctx* ctx, float ms[GS4D_T_COUNT]);             /* blocking; -1.0f for stages that did not run */
/* Start and end of every timed stage of the frames recorded so far (at most 128), in ms since the first timed stage of frame 0:
 * ms[frame][stage][2].  Shows how consecutive frames overlap.  Blocking; does not restart the ring (gs4d_get_timings does). */
GS4D_API int gs4d_get_timeline(gs4d_ctx* ctx, float* ms, int max_frames, int* frames);
GS4D_API int gs4d_get_stats(gs4d_ctx* ctx, uint64_t stats[8]);                    /* [0] low 32 bits: tile-list entries of the last draw, high 32 bits: draws so far whose projection kernel wrote the list entries itself (staged lists: DESIGN.md 3c), [1] low 40 bits: capacity, high 24 bits: staged draws whose guess did not fit and that were re-run exactly, [2] low 32 bits: re-runs after overflow, high 32 bits: draws that aborted on the device and were cleared away unobserved (never re-run; a frame loop without read-backs checks this stays 0), [3] low 32 bits: tiles, bits 32-39: bytes per record the last 4D draw's projection read (64: static 3D splats, 72: symmetric sig, 96: anything), bits 40-63: tiles the compositing kernel of the last unordered draw was launched for (a staged draw: the box of tiles that held entries in the frames before, a few tiles wider — an entry outside it is found on the device and the draw re-run exactly, counted with the staged misses),
                                                                                      [4] low 32 bits: radix passes launched by the last gs4d_sort_pairs, high 32 bits: candidate streams gs4d_create discarded because they shared a hardware queue with a frame lane chosen before them (0 in a process without other streams), [5] low 32 bits: by the last draw's tile sort (0: the draw built unordered tile lists), high 32 bits: gs4d_keygen calls that gave their output buffers fresh storage instead of waiting for another frame lane (one key / index pair shared by all frames),
                                                                                      [6] bits 0..15: frame lanes, bits 16..31: lanes whose stream shares a hardware queue with another lane's (0 unless the process has fewer free queues than lanes: such a context runs ~10 % slower), high 32 bits: draws that generated the depth keys of the preceding gs4d_keygen themselves (see gs4d_keygen), [7] low 32 bits: draws so far on the unordered tile-list path, high 32 bits: longest tile list of the last such draw */
/* Tile-list entries that cannot change a pixel are not built, in draws of the default blend function (GL_SRC_ALPHA, GL_ONE_MINUS_SRC_ALPHA):
 * a record whose alpha compares equal to 0 gets no entry (its projected record is unchanged), and a record's pixel rectangle is the smaller, per axis, of
 * its quad's box and the box of the disc outside which the fragment test discards.  Pixels, aux and ID planes, record statistics, sorted keys and permutation
 * are bit for bit what they are without; stats[0] counts fewer entries.  A context's first splat draw builds every entry all the same.  Environment, read at gs4d_create like GS4D_STAGED (test hooks):
 * GS4D_CULL_ALPHA0=0 keeps the entries of alpha-0 records, GS4D_TIGHT_RECT=0 keeps the quad's box. */
/* What the depth sorts did, beside gs4d_get_stats (whose eight words keep their meaning: depth_sort_passes stays the digit passes of the LSD plan).
 * Depth keys whose host-proven span is 19..27 bits are sorted by an MSD/LSD hybrid — one global pass on the 9-bit top digit, then one launch that
 * finishes every bucket in LDS — unless the latest bucket report says that a bucket does not fit (a crowded key distribution: the LSD passes again).
 * stats[0] hybrid sorts so far, [1] sort kernel launches so far (histogram, pass, tail and report launches of the depth sorts of every frame lane),
 * [2] the largest top-digit bucket of the latest report (the largest over the frame lanes), [3] buckets of the latest reports that were above the
 * tail's capacity (summed over the frame lanes).  Waits for everything queued.  Environment, read at gs4d_create: GS4D_SORT_HYBRID=0 never plans the
 * hybrid, =1 plans it for every eligible span whatever the size (otherwise: >= 32768 keys); GS4D_SORT_TAILCAP=<keys> lowers the tail's capacity (8192). */
GS4D_API int gs4d_get_sort_stats(gs4d_ctx* ctx, uint64_t stats[4]);
/* Projected records of the last draw, 16 floats per record in record order:
 * cx, cy, a0x, a0y, a1x, a1y, alpha, r, g, b, tile-rect (2 words, bit patterns), hx, hy, valid(1/0), depth.
 * depth (slot 15) is -z_view of the record's (time-conditioned) centre when the draw's frame has aux outputs (gs4d_set_aux_outputs) or the
 * draw has a depth test (gs4d_set_depth_test), and the record is valid, else 0; GS4D_MODE_2D records always have 0. */
GS4D_API int gs4d_debug_read_projected(gs4d_ctx* ctx, float* out16, size_t nrecords);
/* How many times the library has (re)built the SoA shadow of this record buffer (a repack of the whole set, at the first draw or gs4d_keygen after a
 * write to it): gs4d_shade_sh or gs4d_edit_colours on a buffer whose shadow is current does not add to it. */
GS4D_API int gs4d_debug_shadow_builds(gs4d_ctx* ctx, gs4d_buf buf, uint64_t* builds);

/* ---- host-side parameterisation (CPU code inside libgs4d.so; mirrors the reference's host math so that a caller
 *      without GLM can build SSBO contents).  Quaternions are w,x,y,z (GLM 0.9.9.9 order). ---- */
GS4D_API void gs4d_host_look_at(const float eye[3], const float orientation[3], const float up[3], float view[16]);            /* Camera.cpp:50-53 */
GS4D_API void gs4d_host_perspective(float fov_deg, int width, int height, float znear, float zfar, float proj[16]);             /* Camera.cpp:55-58 */
GS4D_API void gs4d_host_quat_look_at(const float dir[3], const float up[3], float q_wxyz[4]);                                   /* Scenes.h:268     */
GS4D_API void gs4d_host_splat3d_cov(const float q_wxyz[4], const float scale[3], float cov9[9]);                                /* Splat.h:334-344  */
GS4D_API void gs4d_host_splat3d_mesh(const float pos3[3], const float q_wxyz[4], const float scale[3], const float color4[4], float verts72[72]); /* Splat.h:433-473, Geometry.h:37-50: the 4 x 72-byte vertices gs4d_draw_quads takes */
GS4D_API void gs4d_host_splat2d_sigma_inv(const float v0[2], float l0, float l1, float sigma_inv4[4]);                             /* Splat.h:551-582  */
GS4D_API void gs4d_host_gaussians2d_record(float angle, float s0, float s1, float px, float py, const float rgb[3], float rec12[12]); /* Scenes.h:1490-1496: one 48-byte GS4D_MODE_2D record */
GS4D_API void gs4d_host_splat4d_cov(const float q_wxyz[4], const float scale[3], float lifetime, float fade, const float dir[3], float cov16[16]); /* Splat.h:132-159 */
GS4D_API void gs4d_host_splat4d_cov2q(const float q0_wxyz[4], const float q1_wxyz[4], const float scale4[4], float cov16[16]);   /* Splat.h:91-130   */
/* Batch builders: n splats -> n 96-byte SplatData records (Scenes.h:22-37 layout).
 * static 3D embedding (Scenes.h:2487 ObjectDisplay): Sigma3 in the upper 3x3, Sigma[i][3]=Sigma[3][i]=0, Sigma44=1, mu_t=0. */
GS4D_API void gs4d_host_build_records_3d(size_t n, const float* pos3, const float* q_wxyz, const float* scale3, const float* rgba, float* records24);
GS4D_API void gs4d_host_build_records_4d(size_t n, const float* pos4, const float* q_wxyz, const float* scale3, const float* lifetime, const float* fade,
                                const float* dir3, const float* rgba, float* records24);
/* The temporal variance sd of gs4d_host_splat4d_cov (Splat.h:139): lifetime^2 / (-2 log(fade)), the quotient in double, rounded to float. */
GS4D_API float gs4d_host_time_variance(float lifetime, float fade);
GS4D_API void gs4d_host_time_variances(size_t n, const float* lifetime, const float* fade, float* out);
/* The batch restatements gs4d_build_records is compared with.  _4d_tvar: gs4d_host_build_records_4d with the temporal variance given instead of
 * (lifetime, fade): tvar[i] = gs4d_host_time_variance(lifetime[i], fade[i]) gives the same bits.  _4d_2q: floats 0..3 = pos4, 4..7 = rgba, 8..23 =
 * gs4d_host_splat4d_cov2q(q0[i], q1[i], scale4[i]). */
GS4D_API void gs4d_host_build_records_4d_tvar(size_t n, const float* pos4, const float* q_wxyz, const float* scale3, const float* dir3, const float* tvar,
                                              const float* rgba, float* records24);
GS4D_API void gs4d_host_build_records_4d_2q(size_t n, const float* pos4, const float* q0_wxyz, const float* q1_wxyz, const float* scale4, const float* rgba,
                                            float* records24);
/* The definition of gs4d_decompose_records: row i of every array given from records24 record i, i < n, in the form GS4D_PARAMS_3D (pos: 3 floats a
 * row; dir3 and tvar are not written) or GS4D_PARAMS_4D_VEL (pos: 4 floats a row) — the text above the declaration of gs4d_decompose_records.  An
 * array that is NULL is not wanted.  Any other form writes nothing. */
GS4D_API void gs4d_host_decompose_records(size_t n, const float* records24, uint32_t form, float* pos, float* q_wxyz, float* scale3, float* rgba, float* dir3, float* tvar);
/* The definition of gs4d_transform_records for one transform: out24 record i = records24 record i under *xf, i < n (the text above the declaration
 * of gs4d_transform_records).  out24 must not overlap records24. */
GS4D_API void gs4d_host_transform_records(size_t n, const float* records24, const gs4d_affine4* xf, float* out24);
/* The definition of gs4d_pose_records: out24 record i = records24 record i under what row i of bind (at byte i * bind_stride) takes from the m rows
 * of xf, i < n (the text above the declaration of gs4d_pose_records).  out24 must not overlap records24.  An unknown form, or a bind_stride that
 * breaks the form's rule, writes nothing. */
GS4D_API void gs4d_host_pose_records(size_t n, const float* records24, const gs4d_affine4* xf, size_t m, const void* bind, uint32_t form,
                                     size_t bind_stride, float* out24);
/* The rotation of a map, of gs4d_rotate_sh (the text above its declaration): from the 16 floats of l, the band matrices D_1 at d[0], D_2 at d[9],
 * D_3 at d[34], all row-major, word 83 = 0, and 1; or 0, with d not written, where the map does not rotate. */
GS4D_API int  gs4d_host_sh_rotation(const float l[16], float d[84]);   /* 1: d holds the matrices; 0: this map does not rotate */
/* The definition of gs4d_rotate_sh: the rows of `out` (stride bytes each; m * n of them with GS4D_SH_EACH, row j*n + i = row i under map j, else n)
 * from the n rows of `rows` under the maps the form chooses among the m rows of xf (bind: NULL with GS4D_SH_EACH).  out must not overlap rows.
 * Arguments the device call would refuse write nothing. */
GS4D_API void gs4d_host_rotate_sh(size_t n, const void* rows, size_t stride, int degree, const gs4d_affine4* xf, size_t m,
                                  const void* bind, uint32_t form, size_t bind_stride, void* out);
/* The weights of gs4d_shade_sh_t / gs4d_collapse_sh (the text above their declarations) for a record whose float 3 is mu_t: w[n - 1] = w_n of block
 * n = 1 .. q->degree_t, bit n - 1 of *mask set iff block n takes part (w of a block that does not, or that is above degree_t: 0).  q->degree,
 * q->cam_pos and q->reserved are not looked at; a degree_t outside 0 .. 2 gives no block. */
GS4D_API void gs4d_host_sh_time_weights(const gs4d_sh_time* q, float mu_t, float w[2], int* mask);
/* The definition of gs4d_collapse_sh: row i of dst (dst_stride bytes) = the effective row of row i of sh (sh_stride bytes) at q->t for record i of
 * records24, zeros behind it, i < n.  dst must not overlap sh.  Arguments the device call would refuse write nothing. */
GS4D_API void gs4d_host_collapse_sh(size_t n, const float* records24, const void* sh, size_t sh_stride, const gs4d_sh_time* q, void* dst, size_t dst_stride);
/* The definition of gs4d_shade_sh_t, in place on floats 4..6 of the n records of records24.  Arguments the device call would refuse write nothing. */
GS4D_API void gs4d_host_shade_sh_t(size_t n, float* records24, const void* sh, size_t sh_stride, const gs4d_sh_time* q);
/* The definition of gs4d_warp_records: out24 record i = records24 record i through the lattice *lat of the nodes nodes4 (4 floats each), i < n (the
 * text above the declaration of gs4d_warp_records).  out24 must not overlap records24.  A lattice the device call would refuse (NULL included)
 * writes nothing. */
GS4D_API void gs4d_host_warp_records(size_t n, const float* records24, const float* nodes4, const gs4d_lattice* lat, float* out24);
/* The definition of gs4d_slice_records: out24 record i = records24 record i conditioned at q->t, i < n (the text above the declaration of
 * gs4d_slice_records; expf is the C library's).  out24 must not overlap records24.  A query the device call would refuse is evaluated as it stands. */
GS4D_API void gs4d_host_slice_records(size_t n, const float* records24, const gs4d_slice* q, float* out24);
/* The definition of gs4d_edit_colours, in place on the n records of records24 (the text above its declaration): stats == NULL selects every record
 * (rule is then ignored), else rule is not NULL; from24 is read by GS4D_EDIT_COPY only and must not overlap records24.  An edit the device call
 * would refuse (an unknown op, channels outside 1 .. 15) edits nothing. */
GS4D_API void gs4d_host_edit_colours(size_t n, float* records24, const gs4d_record_stat* stats, const gs4d_keep_rule* rule,
                                     const gs4d_colour_edit* edit, const float* from24);
/* The definition of gs4d_count_centres, in place on the n rows of stats (the text above its declaration), for a context whose image is width x
 * height; mask is read with GS4D_CQ_SCREEN only.  A query the device call would refuse (NULL, an unknown test bit or op, reserved != 0, a mask
 * without GS4D_CQ_SCREEN, with GS4D_CQ_SCREEN a rectangle that is empty or not inside the image) changes nothing. */
GS4D_API void gs4d_host_count_centres(size_t n, const float* records24, const gs4d_centre_query* query, int width, int height,
                                      const uint8_t* mask /* may be NULL */, gs4d_record_stat* stats);
/* The definition of gs4d_measure_records (the text above its declaration): *out <- the measurement of the n records of records24.  stats == NULL
 * selects every record (rule is then ignored), else rule is not NULL.  A query the device call would refuse (NULL, an unknown flag, a non-zero
 * reserved word) gives the empty measurement. */
GS4D_API void gs4d_host_measure_records(size_t n, const float* records24, const gs4d_measure_query* query, const gs4d_record_stat* stats,
                                        const gs4d_keep_rule* rule, gs4d_measure* out);
/* The centroid of a measurement: lo + (hi - lo) * (cell_sum / (count * 2^20)) per axis, in double precision, rounded to float.  Returns 1, or 0
 * with centre3 = {0, 0, 0} when count == 0. */
GS4D_API int  gs4d_host_measure_centre(const gs4d_measure* m, float centre3[3]);
/* The definition of gs4d_transform_selected, in place on the n records of records24 (the text above its declaration): stats == NULL selects every
 * record (rule is then ignored), else rule is not NULL; measure is read with GS4D_XS_PIVOT_MEASURE only.  A call the device would refuse for its xf
 * (NULL, an unknown flags value, GS4D_XS_PIVOT_MEASURE without a measure) changes nothing. */
GS4D_API void gs4d_host_transform_selected(size_t n, float* records24, const gs4d_record_stat* stats, const gs4d_keep_rule* rule,
                                           const gs4d_selection_xf* xf, const gs4d_measure* measure);
/* The definition of gs4d_count_neighbours, in place on the n rows of stats (the text above its declaration): the brute-force double loop, with
 * the early exit at cap.  source == NULL selects every record (rule is then ignored), else rule is not NULL; source and stats must not overlap.
 * A query the device call would refuse (NULL, an unknown flag, a non-zero reserved word, cap == 0, a radius outside 2^-63 <= r < 2^64) changes
 * nothing. */
GS4D_API void gs4d_host_count_neighbours(size_t n, const float* records24, const gs4d_neighbour_query* query,
                                         const gs4d_record_stat* source, const gs4d_keep_rule* rule, gs4d_record_stat* stats);
/* The definition of gs4d_label_components (the text above its declaration): the brute-force double loop over every pair of members, a sequential
 * union–find, then the n words of labels and — stats != NULL — the rows of the members.  source == NULL selects every record (rule is then
 * ignored), else rule is not NULL.  A query the device call would refuse (NULL, an unknown flag, a non-zero reserved word, cap == 0, a radius
 * outside 2^-63 <= r < 2^64, a rule with an unknown flag or reserved != 0) changes nothing: labels is not written either. */
GS4D_API void gs4d_host_label_components(size_t n, const float* records24, const gs4d_component_query* query,
                                         const gs4d_record_stat* source, const gs4d_keep_rule* rule, uint32_t* labels, gs4d_record_stat* stats);
/* The definition of gs4d_count_labels, in place on the n rows of stats.  rule == NULL, or one with an unknown flag or reserved != 0, changes nothing. */
GS4D_API void gs4d_host_count_labels(size_t n, const uint32_t* labels, const gs4d_record_stat* seeds, const gs4d_keep_rule* rule,
                                     gs4d_record_stat* stats);
/* The definition of gs4d_cell_labels (the text above its declaration): labels[i] of the n records of records24.  A grid the device call would
 * refuse (NULL included) writes nothing. */
GS4D_API void gs4d_host_cell_labels(size_t n, const float* records24, const gs4d_cell_grid* grid, uint32_t* labels);
/* The definition of gs4d_merge_records (the text above its declaration): out24 receives one record per group (room for n records covers every
 * case), groups one row per group and member_group n words (either may be NULL), *count the four counts; there is no capacity: written == groups.
 * stats == NULL (with rule == NULL) lets every record be a member.  A query the device call would refuse (NULL, an alpha_max that is not finite
 * and > 0, flags or reserved != 0), n > 0xFFFFFFFE, exactly one of stats / rule given, or a rule with an unknown flag or reserved != 0 writes
 * nothing. */
GS4D_API void gs4d_host_merge_records(size_t n, const float* records24, const uint32_t* labels, const gs4d_merge_query* q,
                                      const gs4d_record_stat* stats, const gs4d_keep_rule* rule,
                                      float* out24, gs4d_merge_group* groups, uint32_t* member_group, gs4d_merge_count* count);
/* The definition of gs4d_merge_rows (the text above its declaration) over the text of csrc/merge_rows_record.h: group g of the n rows of `rows`
 * under member_group goes to row dst_first + g of the `capacity` rows of dst, and *count receives the four counts.  records24 == NULL: unit
 * weights.  A query the device call would refuse (NULL included), n or dst_first > 0xFFFFFFFE writes nothing. */
GS4D_API void gs4d_host_merge_rows(size_t n, const float* records24, const uint32_t* member_group, const void* rows, const gs4d_rows_query* q,
                                   void* dst, size_t dst_first, size_t capacity, gs4d_merge_count* count);
/* The definition of gs4d_lod_cut (the text above its declaration) as a plain loop over the levels from the top down, over the text of
 * csrc/lod_query.h: the states of the n nodes of records24 under parent, then the DRAW nodes in ascending index into the first
 * min(drawn, capacity) slots of dst24 and cut_index (either may be NULL), one fragment into the row of every DRAW node of stats (may be NULL),
 * and *count.  A query the device call would refuse (NULL included) writes nothing. */
GS4D_API void gs4d_host_lod_cut(size_t n, const float* records24, const uint32_t* parent, const gs4d_lod_query* q,
                                float* dst24, uint32_t* cut_index, gs4d_record_stat* stats, gs4d_lod_count* count, size_t capacity);
/* The definition of gs4d_nearest_neighbours (the text above its declaration): the brute-force double loop, every source that is near inserted
 * into the sorted list of the k smallest (bits(dist2), j); then the k slots of row i at hits + i * hit_stride and — stats != NULL — the row of
 * the table.  source == NULL selects every record (rule is then ignored), else rule is not NULL.  A call the device would refuse for its query,
 * rule or hit_stride (NULL, an unknown flag, a non-zero reserved word, k outside 1 .. 16, a radius outside 2^-63 <= r < 2^64, a hit_stride that
 * is not a multiple of 16 in 16 .. 1024 or is below 8 k) changes nothing. */
GS4D_API void gs4d_host_nearest_neighbours(size_t n, const float* records24, const gs4d_nearest_query* query,
                                           const gs4d_record_stat* source, const gs4d_keep_rule* rule,
                                           void* hits, size_t hit_stride, gs4d_record_stat* stats /* may be NULL */);
/* "Frame selection": the eye from which a camera of gs4d_host_look_at(eye, orientation, up) and gs4d_host_perspective(fov_deg, width, height, ..)
 * sees the whole box lo .. hi with its centre in the middle of the image.  The box's bounding sphere (centre (lo + hi) / 2, radius half the
 * diagonal; a degenerate box — a radius that is zero or not finite — gets radius 1) is fitted into the narrower of the projection's two
 * half-angles: eye = centre - normalize(orientation) * radius / sin(half_angle).  In double precision, rounded to float. */
GS4D_API void gs4d_host_frame_box(const float lo[3], const float hi[3], const float orientation[3], float fov_deg, int width, int height, float eye3[3]);
/* One row of gs4d_transform_records' table: the upper 3x3 of L is scale * R(q) with the R of gs4d_host_splat3d_cov (the matrix of the quaternion as
 * given, not normalised), each element one product; column 3, rows 0..2 = velocity (a source at time t lands velocity * t further on);
 * L[3, 3] = time_scale and the time row is otherwise 0; o = (translate, time_offset).  A source time t shows at time_scale * t + time_offset. */
GS4D_API void gs4d_host_affine4(const float q_wxyz[4], float scale, const float translate[3], const float velocity[3], float time_scale, float time_offset,
                                gs4d_affine4* out);

/* Scene generators and the .vdata loader (f2): the CPU loops that fill the SSBO before the path starts. */
GS4D_API void gs4d_host_scene_linear(size_t nverts, const float* verts6, int steps, float time_multiplier, float object_scale, const float splat_scale[3],
                                     float lifetime, float fade, float speed, float* records24);                      /* Scenes.h:258-279, defaults :186-201 */
GS4D_API void gs4d_host_scene_nonlinear(size_t nverts, const float* verts6, int steps, float angle_multiplier, float radius, float object_scale,
                                        const float splat_scale[3], float lifetime, float fade, float speed, size_t max_records, float* records24); /* Scenes.h:517-545, defaults :451-467 */
GS4D_API void gs4d_host_scene_rotation(size_t nverts, const float* verts6, int steps, float angle_multiplier, float object_scale, const float splat_scale[3],
                                       float lifetime, float fade, float speed, size_t max_records, float* records24);  /* Scenes.h:775-803, defaults :711-727 */
GS4D_API void gs4d_host_scene_combined(size_t nverts, const float* verts6, int steps, float angle_multiplier, float lin_multiplier, float amplitude, float frequency,
                                       float object_scale, const float splat_scale[3], float lifetime, float fade, float speed, size_t max_records,
                                       float* records24);                                                               /* Scenes.h:1035-1068, defaults :959-976 */
GS4D_API void gs4d_host_scene_broken(size_t nverts, const float* verts6, int steps, float object_scale, const float splat_scale[3],
                                     float lifetime, float fade, float speed, size_t max_records, float* records24);    /* Scenes.h:1965-1989, defaults :1899-1912 */
GS4D_API void gs4d_host_scene_square(size_t nverts, const float* verts6, int steps, float square_size, float object_scale, const float splat_scale[3],
                                     float lifetime, float fade, float speed, size_t max_records, float* records24);    /* Scenes.h:2216-2259, defaults :2151-2165 */
GS4D_API long gs4d_host_parse_vdata(const char* path, float* verts6, size_t cap_vertices);                            /* VDataParser.h:25-58 */
/* .sd splat files (23 numbers per splat) -> 96-byte records as ObjectDisplay::init builds them; returns the splat count or -1 */
GS4D_API long gs4d_host_parse_sd(const char* path, float object_scale, float* records24, size_t cap_records);           /* VDataParser.h:60-123, Scenes.h:2483-2491 */

/* Camera input model: Camera::HandleInput / HandleCamRotation / SetIsViewFixedOnPoint / GetViewport / GetFocal
 * (Camera.cpp:90-99, 116-220) as a pure state machine — no window: the caller says which keys are down and where the cursor is. */
enum { GS4D_CAMKEY_W = 1, GS4D_CAMKEY_S = 2, GS4D_CAMKEY_A = 4, GS4D_CAMKEY_D = 8, GS4D_CAMKEY_E = 16, GS4D_CAMKEY_Q = 32, GS4D_CAMKEY_SPACE = 64,
       GS4D_CAMKEY_LCTRL = 128, GS4D_CAMKEY_LSHIFT = 256, GS4D_CAMKEY_C = 512, GS4D_CAMKEY_ESC = 1024 };
typedef struct gs4d_camera_state {
    float position[3], orientation[3], up[3];
    int width, height;
    float sensitivity, speed, fast_speed;                 /* Camera.h:78-80: 100, 0.5, 2 */
    int capture_mouse, first_capture, fix_view, fix_position, lock_x, lock_y;
} gs4d_camera_state;
typedef struct gs4d_camera_input { unsigned keys; double mouse_x, mouse_y; int imgui_active; } gs4d_camera_input;
/* One HandleInput call.  *recenter_cursor != 0: the reference moved the cursor to the window centre (glfwSetCursorPos) during the call;
 * *hide_cursor != 0: it hid the cursor (glfwSetInputMode).  When C captures the mouse in this very call the rotation that follows reads
 * the re-centred cursor, as the reference does. */
GS4D_API void gs4d_host_camera_input(gs4d_camera_state* st, const gs4d_camera_input* in, int* recenter_cursor, int* hide_cursor);
GS4D_API void gs4d_host_camera_rotate(gs4d_camera_state* st, double mouse_x, double mouse_y);            /* Camera.cpp:191-207 */
GS4D_API void gs4d_host_camera_look_at_point(gs4d_camera_state* st, const float point[3]);              /* Camera.cpp:209-220 */
GS4D_API void gs4d_host_camera_viewport(int width, int height, float out2[2]);                           /* Camera.cpp:90-93  */
GS4D_API void gs4d_host_camera_focal(float fov, int width, int height, float out2[2]);                   /* Camera.cpp:95-99  */
/* Picking: the world point at view depth `depth` (-z_view, e.g. D/O of gs4d_read_aux) on the ray through the centre of pixel (px, py) of a
 * width x height image — window coordinates (px + 0.5, py + 0.5), row 0 = bottom, as the images; fractional px, py allowed.  With
 * gs4d_read_aux and gs4d_host_camera_look_at_point this turns the press of a cursor into a camera that looks at what lies under it. */
GS4D_API void gs4d_host_unproject(const float view[16], const float proj[16], int width, int height, float px, float py, float depth, float world3[3]);
/* The bounds gs4d_keygen derives for its keys, as a pure function: every key (as a uint32 bit pattern) of a record whose position, mu_t and
 * velocity sig[3].xyz lie in the box lo[7] .. hi[7] (x, y, z, mu_t, vx, vy, vz) is in [*bias, *bias + *span] at time t for a camera at cam.
 * Proven by evaluating the kernel's own float32 operations, all monotone, on the ends of the box; *bias = 0 and *span = 0xFFFFFFFF where
 * nothing can be claimed (non-finite arguments, t - mu_t overflowing, GS4D_KEY_VIEW_Z); no upper bound with the camera inside or on the box. */
GS4D_API void gs4d_host_key_bounds(const float lo[7], const float hi[7], float t, const float cam[3], int key_mode, uint32_t* bias, uint32_t* span);

/* Presentation: an RGBA8 frame as produced by gs4d_read_pixels_rgba8_device (bottom row first) -> PNG file */
GS4D_API int gs4d_host_write_png(const char* path, const uint8_t* rgba8, int width, int height);

GS4D_API const char* gs4d_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GS4D_H */

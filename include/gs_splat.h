/*
 * gs_splat.h -- C ABI of the MI355X-native Gaussian-splat hot path.
 *
 * Drop-in boundary for the hot path of the A-Frame `gaussian_splatting`
 * component (reference: quadjr/aframe-gaussian-splatting, file index.js).
 * Every entry point names the reference interface it replaces (file:line).
 * Plain pointers and sizes only; no C++ / torch types.  All functions return
 * GS_OK (0) or a negative gs_status; the message for the last failure on a
 * context is available from gs_last_error().
 *
 * Threading: a gs_ctx is single-caller (the reference is single-flight too:
 * `sortReady`, index.js:206/220/439-440).  Several contexts may coexist (the
 * reference allows several component instances per page, cutout-demo.html:24-25).
 *
 * There is NO CPU fallback: if no HIP device is usable gs_create() fails with
 * GS_E_NODEVICE / GS_E_HIP and nothing else can be called.
 */
#ifndef GS_SPLAT_H
#define GS_SPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_API __attribute__((visibility("default")))

typedef struct gs_ctx gs_ctx;

typedef enum gs_status {
    GS_OK = 0,
    GS_E_BADARG = -1,      /* null / out-of-range argument                                              */
    GS_E_PLY_HEADER = -2,  /* "Unable to read .ply file header"           (index.js:606-607)            */
    GS_E_PLY_PROP = -3,    /* "<prop> not found"                          (index.js:643)                */
    GS_E_HIP = -4,         /* a HIP runtime call failed                                                 */
    GS_E_OOM = -5,         /* host or device allocation failed                                          */
    GS_E_NODEVICE = -6,    /* no usable gfx950 device                                                   */
    GS_E_STATE = -7,       /* call not valid in this state (e.g. render after matrices-only push)       */
    GS_E_PLY_DATA = -8,    /* vertex data shorter than the header promises (DataView RangeError in JS)  */
    GS_E_RETRY = -9        /* gs_sync(): an asynchronous frame came back incomplete (it outgrew the pair buffers, or needed the
                              binning round it had skipped) AND the library could not draw it again by itself: gathered frames
                              (every rank has to take part), frames that share an output buffer, data pushed meanwhile, or
                              GS_OPT_AUTO_RETRY = 0.  The frames since the previous gs_sync() must be rendered again.  Otherwise
                              gs_sync() re-renders such frames into the same buffers before it returns.                  */
} gs_status;

/* ---- lifetime ----------------------------------------------------------------------------------- */

/* One context = one component instance on one GPU (replaces the Worker spawn + GL resource creation,
 * index.js:229-236 and initGL index.js:25-66).  `device` is the HIP device ordinal. */
GS_API int gs_create(int device, gs_ctx **out);
GS_API int gs_destroy(gs_ctx *ctx);
/* Last error text for ctx; ctx == NULL returns the last gs_create() failure of the calling thread. */
GS_API const char *gs_last_error(const gs_ctx *ctx);
/* Library/ABI version, e.g. 0x000100 = 0.1.0 */
GS_API uint32_t gs_version(void);
/* HIP devices this process can use (0 = none: gs_create will fail) -- what a host would pass to gs_create_multi */
GS_API int gs_device_count(void);

/* ---- data ingest (reference: worker `clear`/`push`, pushDataBuffer, processPlyBuffer) --------------- */

/* worker {method:"clear"} (index.js:573-575) + loadedVertexCount = 0 (index.js:226). */
GS_API int gs_clear(gs_ctx *ctx);

/* pushDataBuffer(buffer, vertexCount) (index.js:328-437): append `nrows` 32-byte .splat rows
 * (f32 pos[3], f32 scale[3], u8 rgba[4], u8 quat_wxyz[4]).  Packs on the GPU, bit-exactly as the
 * reference does, into the 16 B centre/scale record, the 16 B covariance/colour record and the
 * worker's sort row.  Rows are borrowed for the duration of the call. */
GS_API int gs_push_splat(gs_ctx *ctx, const void *rows, size_t nrows);

/* worker {method:"push", matrices} (index.js:576-586): append `nrows` 16-float worker rows; only
 * elements 12..15 are read, as in sortSplats (index.js:520-548).  A context fed this way can sort
 * but not render. */
GS_API int gs_push_matrices(gs_ctx *ctx, const float *matrices, size_t nrows);

/* processPlyBuffer(inputBuffer) (index.js:600-745) followed by pushDataBuffer: parse a binary
 * little-endian PLY, order rows by importance, convert to .splat rows, append.  The header is parsed on
 * the host; importance, the stable descending sort and the row conversion run on the GPU and the rows go
 * from HBM straight into the pack kernel. */
GS_API int gs_load_ply(gs_ctx *ctx, const void *bytes, size_t nbytes);

/* processPlyBuffer alone, converted on the context's GPU: same bytes as gs_ply_to_splat (both evaluate the
 * same f64 arithmetic, incl. the engine's Math.exp).  out_rows == NULL: size query (header and property
 * checks only).  Errors are reported through gs_last_error(). */
GS_API int gs_ply_to_splat_gpu(gs_ctx *ctx, const void *bytes, size_t nbytes, void *out_rows, size_t *out_nrows);

/* processPlyBuffer alone (host side): PLY bytes -> .splat rows.  Call with out_rows == NULL to get
 * *out_nrows, then again with a buffer of 32 * *out_nrows bytes.  err (optional) receives the message
 * the reference would throw. */
GS_API int gs_ply_to_splat(const void *bytes, size_t nbytes, void *out_rows, size_t *out_nrows, char *err,
                           size_t errlen);

/* ---- view-dependent colour (no reference counterpart: processPlyBuffer keeps f_dc_* only, index.js:725-729) ----------------
 * An INRIA .ply carries 45 f_rest_* coefficients per splat next to f_dc_*: real spherical harmonics of degree 1..3 (Kerbl et al.
 * 2023), the view-dependent part of the colour.  With GS_OPT_SH_DEGREE above 0 the context keeps them -- one SH ROW per splat:
 * 3 * (D+1)^2 f32, channel-major sh[c][k], k = 0 is f_dc_c -- and the projection kernel replaces the RGB bytes of every splat it
 * projects by `clamped_u8((0.5 + SH_C0*sh[c][0] + sum_k basis_k(d)*sh[c][k]) * 255)`, d = the unit vector from the camera to the
 * splat in object space (f64, fixed operation order: csrc/gs_sh.h).  Degree 0, and any splat whose higher coefficients are all
 * zero, give exactly the byte processPlyBuffer bakes.  Alpha stays the packed byte.  Off by default. */

/* The SH rows of a PLY in the order of the rows gs_ply_to_splat_gpu / gs_ply_to_splat return for it (descending importance, ties
 * stable, index.js:668), for callers that convert and then push (gaussian_splatting.js:66-69).  degree 0..3: the highest band
 * wanted; *out_degree = min(degree, what the file carries: 0, 9, 24 or 45 f_rest_* -> 0..3), rows of 3 * (*out_degree+1)^2 f32.
 * A file with another count, a gap in the numbering or no f_dc_*: *out_degree = -1, *out_nrows = 0, GS_OK.  out_sh == NULL: size
 * query.  Properties of any declared type are read as processPlyBuffer reads them and rounded to f32.  Runs on the host. */
GS_API int gs_ply_sh(gs_ctx *ctx, const void *bytes, size_t nbytes, int degree, float *out_sh, size_t *out_nrows, int *out_degree);
/* ... the same without a context (as gs_ply_to_splat is to gs_ply_to_splat_gpu); err (optional) receives the message. */
GS_API int gs_ply_sh_host(const void *bytes, size_t nbytes, int degree, float *out_sh, size_t *out_nrows, int *out_degree, char *err,
                          size_t errlen);
/* Append `nrows` SH rows of `degree` (1..3), parallel to gs_push_splat: row i of the SH store belongs to splat i.  Splats beyond
 * the last SH row draw with their packed byte colour (progressive loading, .splat data).  A degree other than that of the rows
 * already stored: GS_E_BADARG.  gs_clear empties the store.  gs_load_ply with GS_OPT_SH_DEGREE at 1..3 does this by itself when
 * the store is still parallel to the splats (as many SH rows as splats before the call, of the same degree). */
GS_API int gs_push_sh(gs_ctx *ctx, const float *sh_rows, size_t nrows, int degree);
/* Rows in the SH store and their degree (0 rows: *out_degree = 0); gs_download(GS_BUF_SH) returns them. */
GS_API int gs_sh_count(const gs_ctx *ctx, size_t *out_nrows, int *out_degree);
/* One colour on the host, by the very arithmetic of the kernel: sh_row of `degree` (0..3), camera and splat position in the
 * rows' object space (positions as a .ply / .splat row stores them: the space the coefficients were trained in) -> rgb bytes.  gs_sh_eval_unrounded: the three values before clamped_u8, in units of one colour byte. */
GS_API int gs_sh_eval(const float *sh_row, int degree, const double cam[3], const float pos[3], uint8_t rgb[3]);
GS_API int gs_sh_eval_unrounded(const float *sh_row, int degree, const double cam[3], const float pos[3], double out[3]);
/* The camera position in object space a frame with this model_view evaluates its colours for: the inverse of the affine 4x4
 * applied to the origin, in f64 by cofactors of the upper 3x3 in a fixed order -- the very bits the kernel is handed.
 * GS_E_BADARG for a singular matrix (a render refuses it likewise, but only while SH is active).  model_view acts on the packed
 * centre (x, y, -z) (index.js:350-354), so this is the camera in that mirrored space; a frame negates out[2] -- exactly -- to get
 * the camera in the rows' space, which is what the kernel and gs_sh_eval take. */
GS_API int gs_camera_in_object(const float model_view[16], double out[3]);
/* The opacity factor of GS_OPT_ANTIALIAS on the host, by the very arithmetic of the kernel: cov = {cov00, cov01, cov11}, a splat's
 * projected 2x2 covariance in px^2 BEFORE the 0.3 px^2 dilation -> *out_c in [0, 1] (the formula is spelt out at the option).
 * GS_E_BADARG for null pointers. */
GS_API int gs_antialias_factor(const float cov[3], float *out_c);

/* Number of splats resident (reference: loadedVertexCount / matrices.length/16). */
GS_API size_t gs_count(const gs_ctx *ctx);

/* ---- sort (reference: worker {method:"sort"} -> sortSplats, index.js:507-570, 587-596) --------------- */

/* view = row 2 of gsModelViewMatrix (index.js:441-442); cutout16 = column-major object->unit-box
 * matrix or NULL (index.js:443-452).  The order is kept on the device for gs_render().
 * out_idx (optional, capacity >= max(gs_count(),1)) receives the reference's Uint32Array bit-exactly,
 * *out_n its length.  Before any push the reference answers Uint32Array(1) = [0] (index.js:588-590):
 * so does this (out_n = 1, out_idx[0] = 0). */
GS_API int gs_sort(gs_ctx *ctx, const float view[4], const float *cutout16, uint32_t *out_idx, uint32_t *out_n);

/* The reference's single-flight rhythm (index.js:201-207, 438-455): tick() POSTS the sort to the worker and returns; every frame
 * three.js draws until the worker's reply arrives uses the last COMPLETED order (the reply handler installs the new index list and
 * re-arms sortReady).  One caller thread, no blocking:
 *   gs_sort_begin  enqueues the whole sort for (view, cutout16) on a pipeline lane other than the one the current order lives on and
 *                  returns at once.  GS_E_STATE while a begun sort has not been collected (the reference's `sortReady` guard,
 *                  index.js:439-440).  gs_render* / gs_render_stereo keep drawing from the order of the last completed gs_sort /
 *                  gs_sort_poll meanwhile (before the first one: nothing, as the reference's instanceCount starts at 0).
 *   gs_sort_poll   *done = 0 if the sort is still running (wait == 0), else installs its order as the one gs_render* draws from,
 *                  hands it back like gs_sort (out_idx optional, capacity >= max(gs_count(), 1); *out_n its length; begun before any
 *                  push: [0], index.js:588-590) and sets *done = 1.  wait != 0 blocks until then.  Nothing begun: *done = 1, *out_n = 0.
 * Splats pushed between the two calls: the sort is run again over what is resident when it is collected. */
GS_API int gs_sort_begin(gs_ctx *ctx, const float view[4], const float *cutout16);
GS_API int gs_sort_poll(gs_ctx *ctx, int wait, uint32_t *out_idx, uint32_t *out_n, int *done);

/* ---- render (reference: vertex shader + rasteriser + fragment shader + blend, index.js:77-195) ------- */

#define GS_RENDER_FLIP_Y 1u      /* rows bottom-up (WebGL readPixels order) instead of top-down              */
#define GS_RENDER_COUNT_FRAGS 2u /* no early termination; count reference-equivalent splat-fragments         */
#define GS_RENDER_NO_EARLY_OUT 4u/* blend every fragment (parity debugging)                                   */
#define GS_RENDER_COUNT_EVALUATED 16u /* with GS_RENDER_COUNT_FRAGS: leave early termination ON and count the fragments
                                    the blend really evaluates (one binning round; what the reference-equivalent count shrinks to) */
#define GS_RENDER_ASYNC 8u       /* enqueue the frame and return; completion, status and statistics are collected by
                                    gs_sync().  The reference renders every frame without waiting for the GPU either
                                    (index.js:184-207).  gs_render_device: the frame stays in HBM.  gs_render: the frame
                                    is copied to rgba_out behind its kernels, on the frame's own stream -- rgba_out must
                                    stay valid and unread until gs_sync(), one buffer per frame in flight, and should be
                                    page-locked (gs_host_alloc) for the copy to overlap the following frames.           */

#define GS_RENDER_PARALLEL 32u   /* a PARALLEL-PROJECTION camera (orthographic, sheared or not): "Parallel-projection cameras" below.  (Bit 5 was free:
                                    the library keeps no internal flags in gs_render_params.flags or in its frame uniforms.)               */

typedef struct gs_render_params {
    float model_view[16]; /* gsModelViewMatrix, column-major (getModelViewMatrix, index.js:467-487)      */
    float projection[16]; /* gsProjectionMatrix, column-major (getProjectionMatrix, index.js:456-466)    */
    int32_t fb_width;     /* `viewport` uniform, device pixels (index.js:189-193)                        */
    int32_t fb_height;
    int32_t x0, x1;       /* column strip [x0,x1) to produce; x0 = 0, x1 = fb_width for the whole frame  */
    float focal;          /* `focal` uniform; <= 0: computed as fb_height/2*|projection[5]| (index.js:191) */
    float background[4];  /* destination before blending; demos: opaque black sky (index.html:14)        */
    uint32_t flags;       /* GS_RENDER_*                                                                  */
} gs_render_params;

/* Draw the last gs_sort() order into a tightly described RGBA8 image in caller-owned host memory.
 * rgba_out: (x1-x0) x fb_height pixels, `stride` bytes per row (0 = tight), row 0 = top. */
GS_API int gs_render(gs_ctx *ctx, const gs_render_params *p, uint8_t *rgba_out, size_t stride);
/* Strips [x0,x1) whose x0 is a multiple of 4 (the multi-GPU partition uses multiples of 16), whatever x1, reproduce the
 * corresponding columns of the full frame bit for bit; other strips within 1 LSB (early termination works on groups of 4
 * pixels counted from x0). */
/* Same, but the strip stays on the GPU: device_rgba is a device pointer (e.g. a torch tensor's
 * data_ptr, tight rows) or NULL to render into the context's own framebuffer only.  device_rgba needs 4-byte alignment;
 * 16-byte-aligned strips whose width is a multiple of 4 are stored four pixels at a time. */
GS_API int gs_render_device(gs_ctx *ctx, const gs_render_params *p, void *device_rgba);
/* gs_sort for ONE column strip of a frame that is then drawn with exactly these parameters (strip->x0, x1; NULL = gs_sort):
 * splats whose quad cannot reach the strip are left out by a conservative bound (4 min(sqrt(2 lambda1), 1024) + 2 pixels
 * around the projected centre, lambda1 <= (|J| |A| sigma_max)^2 + 0.3, index.js:127-149), the others come in the reference's
 * order -- the bucket scale still uses the depth range of EVERY splat the reference keeps (index.js:552-558).  The strip's
 * pixels are bit-identical to those drawn from the full order; what shrinks is the sort (and everything downstream) on a GPU
 * that owns one strip of eight.  out_idx / out_n: the strip's sub-sequence of the reference's Uint32Array.  Not for a sort
 * that outlives its camera (the reference draws with the latest completed order, index.js:201-207): render with the pose
 * it was sorted for. */
GS_API int gs_sort_for(gs_ctx *ctx, const float view[4], const float *cutout16, const gs_render_params *strip,
                       uint32_t *out_idx, uint32_t *out_n);

/* XR: two eyes share one sort order from the head camera (index.js:441) -- two params, two images. */
GS_API int gs_render_stereo(gs_ctx *ctx, const gs_render_params eyes[2], uint8_t *rgba_out[2], size_t stride);

/* ---- Parallel-projection cameras (no reference counterpart: the vertex shader's Jacobian is the perspective focal / camz, index.js:127-131) ----
 * Axis-aligned top, front and side views of an editing host: a rectangle or lasso selects a prism, not a frustum, and sizes compare across
 * depth.  Params whose flags carry GS_RENDER_PARALLEL are projected by the rule below -- a frame, a strip, each eye of gs_render_stereo, a
 * surface or contribution frame, gs_pick, gs_select_rect / gs_select_mask, gathered and gs_multi frames (there the camera model is the
 * VIEW's own: the bit is taken from views[v].flags, or from the call's `flags` for all views).  Without the flag nothing changes: such a
 * frame launches the kernels it launched before (the rule sits behind a template flag of k_project and of the two selection kernels).
 *   - projection must have P[3] == 0, P[7] == 0, P[11] == 0 and P[15] == 1, compared as f32 (a -0 passes); otherwise the call -- any entry
 *     point that takes params, gs_sort_for / gs_sort_gathered / gs_multi_sort included -- returns GS_E_BADARG with a message.  Rows 0..2 are
 *     free: sheared (oblique) parallel projections work.  gs_ortho_matrix + gs_projection_matrix give the usual box.  `focal` is ignored.
 *   - THE RULE (csrc/gs_device_math.h: gsm::parallel_jacobian, called by the kernels and by gs_project_record), f32, un-fused, in this order:
 *       hx = 0.5f * vw;  hy = 0.5f * vh;
 *       j00 = hx * P[0]; j01 = hx * P[4]; j02 = hx * P[8];     j10 = hy * P[1]; j11 = hy * P[5]; j12 = hy * P[9];
 *       M0k = (j00 * mv[4k] + j01 * mv[4k+1]) + j02 * mv[4k+2];   M1k = (j10 * mv[4k] + j11 * mv[4k+1]) + j12 * mv[4k+2];   k = 0, 1, 2
 *     M replaces the reference's M = J * mat3(modelView) (index.js:127-133); it is the exact derivative of the centre the projection already
 *     computes, the same for every splat of the frame.  Everything else is the perspective text: the clip-space position, the 1.2 bounds
 *     and near-plane culls (pw is camw: 1 for an affine model_view), the covariance, the 0.3 px^2 dilation, the eigenvalues and axes, the
 *     zndc > 1 cull, the record, and the factor of GS_OPT_ANTIALIAS.  Binning, every blend path and write-out see the record only.
 *   - THE DEPTH SORT is untouched: along the view row it is already the right order for a parallel camera, and both of its culls stay --
 *     splats behind the camera plane are dropped, and so are splats smaller than 0.0001 |depth| (index.js:548).  Depth influences nothing
 *     else in such a frame, so a host should PARK A PARALLEL CAMERA JUST OUTSIDE THE CLOUD, not far away: at a large distance the size cull
 *     removes small splats that the frame would draw at full size.
 *   - gs_sort_for / gs_sort_gathered with the flag keep every splat (the strip's reach bound is the perspective Jacobian's): the returned
 *     order is gs_sort's and the pixels are bit-identical.  A parallel reach bound in the strip depth kernels is out of scope.
 *   - GS_OPT_SH_DEGREE frames keep evaluating the colour from the point gs_camera_in_object gives (the camera's position, not a constant
 *     view direction: out of scope).  GS_OPT_ANTIALIAS and GS_OPT_HIGHLIGHT combine unchanged.
 *   - GS_OPT_FRAME_BATCH: two queued frames that both carry the flag pair up; a frame with it and one without go out alone, as frames
 *     with different flags always have.
 * Out of scope: a parallel reach bound for strip sorts, a constant SH direction, fisheye or other camera models. */
/* One packed record (cs = the centre/scale texel, cc = the covariance/colour texel: gs_download(GS_BUF_SPLAT) rows) through the kernels' own
 * projection function, with or without GS_RENDER_PARALLEL in p->flags; host only, no context.  The `focal` rule is gs_render's.  record:
 * the eight words GS_BUF_PROJECTED holds (cx, cy, ax, ay, bx, by, the colour word, alpha -- NOT compensated by GS_OPT_ANTIALIAS);
 * *zwin = zndc * 0.5f + 0.5f; *visible = 0 where the projection emits nothing (record and *zwin are then zero).  NULL pointers, a
 * non-positive frame size, or the flag with a matrix that fails the check above: GS_E_BADARG. */
GS_API int gs_project_record(const float cs[4], const uint32_t cc[4], const gs_render_params *p, float record[8], float *zwin, int *visible);
/* Whether the last frame of the current frame's lane was projected by the parallel kernels (1 / 0), as gs_highlight_info reports the
 * highlight.  The pointer may be NULL. */
GS_API int gs_projection_info(const gs_ctx *ctx, uint32_t *last_frame_parallel);

/* ---- surface output (no reference counterpart: the material has depthWrite: false, index.js:177-181, so nothing tells a host what
 * lies under a pixel) ------------------------------------------------------------------------------------------------------
 * A pixel's fragments are its list entries that pass the discard test (q <= 4, index.js:172) and, while a scene depth is set, the
 * LEQUAL test, nearest first -- exactly what the blend takes -- with the blend's own transmittance T_k = fma(-alpha, e T_{k-1}, T_{k-1}).
 * The SURFACE of the pixel is the first fragment k with T_{k-1} >= 0.5 and T_k < 0.5: the median of the blending weights (strict: a T
 * of exactly 0.5 has not crossed).  Three planes, each (x1-x0) x fb_height, tight, row 0 = top (GS_RENDER_FLIP_Y applies to all three):
 *   id     u32  the surface splat's index as gs_sort numbers it (the value of the sorted order at that position); 0xFFFFFFFF: T never crosses
 *   depth  f32  that splat's window depth zndc*0.5+0.5 (0 = near plane, 1 = far plane: the convention gs_set_scene takes); 1.0f: no surface
 *   alpha  f32  1 - T where the pixel stopped: the value the colour's alpha byte is rounded from
 * The colour of such a frame is bit-identical to gs_render's on the tile lists with the same GS_OPT_NEAR_PERMILLE.  A surface frame
 * draws from the last completed order like gs_render; it is always synchronous (GS_RENDER_ASYNC is cleared) and always takes tile
 * lists -- the row walk, sub-tile lists, the split blend and paired launches are off for that frame only, the options stay as set;
 * both binning rounds work.  GS_RENDER_COUNT_FRAGS: GS_E_BADARG.  GS_RENDER_NO_EARLY_OUT is allowed.
 * (The strict rule at T == 0.5 exactly is specified, not tested: byte alphas give no scene whose f32 transmittance lands on it.)
 * Out of scope: gathered and gs_multi frames, gs_render_stereo (call once per eye), asynchronous surface frames. */
typedef struct gs_surface { uint32_t *id; float *depth; float *alpha; } gs_surface;   /* any may be NULL: that plane is not written */
/* host planes; rgba_out may be NULL (no colour wanted) */
GS_API int gs_render_surface(gs_ctx *ctx, const gs_render_params *p, uint8_t *rgba_out, size_t stride, const gs_surface *host_out);
/* device planes (tight; 16-byte aligned planes are stored four pixels at a time); device_rgba may be NULL.  device_rgba needs 4-byte
 * alignment; 16-byte-aligned strips whose width is a multiple of 4 are stored four pixels at a time. */
GS_API int gs_render_surface_device(gs_ctx *ctx, const gs_render_params *p, void *device_rgba, const gs_surface *device_out);
/* What the full-frame planes of `p` (its x0 / x1 are ignored) hold at npoints pixels xy = (column, row; row 0 = top) -- exactly -- and
 * the hit splat's centre in the rows' object space, as a .splat row stores it (NaN where id is none).  Draws one 16-pixel column
 * strip per distinct tile column among the points.  A point outside the frame: GS_E_BADARG; a context fed with gs_push_matrices
 * only: GS_E_STATE. */
typedef struct gs_hit { uint32_t id; float depth; float alpha; float pos[3]; } gs_hit;
GS_API int gs_pick(gs_ctx *ctx, const gs_render_params *p, const int32_t *xy, size_t npoints, gs_hit *out);

/* ---- editing the resident cloud (no reference counterpart: the worker only ever appends, index.js:573-586; the one cull the reference
 * has is the single cutoutEntity box, evaluated again in every sort, index.js:525-554) ------------------------------------------------
 * One STATE byte per splat, parallel to the splats like the SH rows.  A splat whose byte has GS_STATE_HIDDEN is, in every depth sort,
 * a splat outside the cutout (`cutoutArea == false`, index.js:548): not kept, not counted, no part in minDepth / maxDepth -- so the
 * order of a context with the set H hidden is exactly the reference's order of the scene without the rows of H (indices of the full
 * scene).  Nothing downstream knows about states: the order does not contain the splat, so projection, binning, every blend path,
 * surface frames and gs_pick never see it.  This holds for gs_sort, gs_sort_for, gs_sort_begin / gs_sort_poll, gs_sort_gathered, the
 * rank that sorts under GS_OPT_SORT_SHARE and the whole-order sorts a render or gs_download(GS_BUF_SORTED) runs by itself.
 *   - GS_STATE_SELECTED changes no pixel by itself: it is the caller's mark (what a later call hides, shows or reads back), and what
 *     GS_OPT_HIGHLIGHT tints.  Bits 2..7 belong to the caller and are kept untouched by the library.
 *   - Splats beyond the store's length have state 0 (progressive loading keeps working); gs_clear empties the store.  While the store
 *     is empty the sorts launch the very kernels of a context that never edits.
 *   - Every call that changes the store behaves like a push: frames in flight are drained first, every lane's order is dropped (a
 *     render before the next sort draws the background only, as after a push), and gs_sync() does not draw frames of before the change again by itself.
 *     A state change takes effect at the NEXT sort: a draw uses the last completed order (index.js:201-207).
 *   - gs_stats.n_hidden: the hidden splats the last collected sort skipped.
 * Moving, rotating and scaling part of the cloud on the device is gs_transform (below, "Changing resident splats in place").
 * Out of scope: undo of in-place edits, or of any other call. */
#define GS_STATE_HIDDEN 1u
#define GS_STATE_SELECTED 2u
#define GS_SELECT_INVERT 1u      /* region calls: apply the rule to the splats NOT in the region */
/* states[0, n) -> splats [first, first + n); the store grows to first + n, zero-filled.  first + n > gs_count(): GS_E_BADARG. */
GS_API int gs_set_state(gs_ctx *ctx, size_t first, const uint8_t *states, size_t n);
/* state = (state & ~clear_bits) | set_bits for the listed splats -- ids as gs_pick and the surface id plane return them.  A duplicate
 * id is harmless; an id >= gs_count() is GS_E_BADARG and changes nothing.  The store grows to gs_count(). */
GS_API int gs_set_state_ids(gs_ctx *ctx, const uint32_t *ids, size_t n, uint8_t set_bits, uint8_t clear_bits);
/* the store's length and the number of hidden splats in it (counted on the GPU when the store last changed) */
GS_API int gs_state_count(const gs_ctx *ctx, size_t *rows, size_t *hidden);
/* Region selection on the GPU, one streaming kernel each: state = (state & ~clear_bits) | set_bits for the splats in the region (with
 * GS_SELECT_INVERT in flags: for those not in it); *out_hit (optional) = the splats the rule was applied to.  The store grows to gs_count().
 *   box     the matrix and the f64 arithmetic of gs_sort's cutout16 on the sort rows (index.js:526-545): a position whose comparisons are
 *           all false (NaN) is inside, as in the reference.  Works on a context fed with gs_push_matrices.
 *   sphere  centre in the rows' object space, as a .splat row stores it; in f64, un-fused: d2 = (dx*dx + dy*dy) + dz*dz, inside iff
 *           d2 <= (double)radius * (double)radius (a NaN d2 is outside).  Matrices-only context: GS_E_STATE.
 *   rect    screen space, among what is drawn: rect = { x0, y0, x1, y1 } in pixels of the frame `p` describes, row 0 = top, clipped to the
 *           frame (p->x0 / x1 are ignored).  Walks the last completed WHOLE order (sorting again in full first if the last sort was
 *           near-only or for a strip, as gs_download(GS_BUF_SORTED) does) and takes a splat iff the projection of that frame accepts it
 *           (the very function the render calls), x0 <= floor(cx) < x1 and y0 <= fb_height - 1 - floor(cy) < y1.  Hidden splats are not
 *           in the order and so are never hit; INVERT: the splats of the order that are not in the rectangle.  *out_hit counts positions
 *           of the order.  No completed order, or a matrices-only context: GS_E_STATE. */
GS_API int gs_select_box(gs_ctx *ctx, const float box16[16], uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit);
GS_API int gs_select_sphere(gs_ctx *ctx, const float centre[3], float radius, uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit);
GS_API int gs_select_rect(gs_ctx *ctx, const gs_render_params *p, const int32_t rect[4], uint8_t set_bits, uint8_t clear_bits, uint32_t flags,
                          size_t *out_hit);
/*   mask    screen space like rect, any shape: mask = fb_width x fb_height bytes in HOST memory, row 0 = top, mask_stride bytes per row
 *           (0 = tight; a non-zero stride below fb_width: GS_E_BADARG), non-zero = the pixel is in the region.  depth_max (optional):
 *           fb_width x fb_height f32, tight, window depths in the convention of gs_set_scene and the surface depth plane.  Walks the
 *           whole order as rect does and takes a position iff the projection of that frame accepts the splat, col = floor(cx) lies in
 *           [0, fb_width), row = fb_height - 1 - floor(cy) lies in [0, fb_height), mask[row][col] != 0 and -- with depth_max --
 *           zndc * 0.5f + 0.5f <= depth_max[row][col] (f32, the value the projection writes for depth tests; a NaN on either side is
 *           false).  Passing the depth plane of gs_render_surface of the same frame selects what is visible: the surface splats and
 *           what lies in front of them; a caller who wants slack adds it to the plane.  INVERT, *out_hit and the errors: as rect; NULL
 *           mask or p: GS_E_BADARG.  Mask and plane are uploaded for the call (the context keeps the device buffer, grow-only). */
GS_API int gs_select_mask(gs_ctx *ctx, const gs_render_params *p, const uint8_t *mask, size_t mask_stride, const float *depth_max, uint8_t set_bits,
                          uint8_t clear_bits, uint32_t flags, size_t *out_hit);
/* A lasso as a mask, on the host (no context, no GPU): even-odd fill of the closed polygon xy = npoints x (x, y) in pixels, row 0 = top,
 * the last vertex joins the first.  mask_out: fb_height rows of `stride` bytes (0 = tight); the first fb_width bytes of every row are
 * written 1 or 0, bytes beyond them stay untouched.  Pixel (x, y) is tested at its centre (px, py) = (x + 0.5, y + 0.5), all in f64,
 * un-fused: an edge a -> b counts iff (ya <= py) != (yb <= py) and px < xa + (py - ya) * (xb - xa) / (yb - ya), evaluated in that
 * order; the pixel is 1 iff the count is odd.  npoints < 3: an all-zero mask, GS_OK.  NULL pointers, non-positive sizes, a non-zero
 * stride below fb_width: GS_E_BADARG. */
GS_API int gs_mask_polygon(const float *xy, size_t npoints, int fb_width, int fb_height, uint8_t *mask_out, size_t stride);
/* GS_OPT_HIGHLIGHT as it stands (*option_value) and whether the last frame of the current frame's lane was projected by the
 * highlighting kernels (*last_frame: 1 / 0; 0 while the option is off or the store is empty).  Either pointer may be NULL. */
GS_API int gs_highlight_info(const gs_ctx *ctx, uint32_t *option_value, uint32_t *last_frame);
/* The colour word GS_OPT_HIGHLIGHT = option_value gives a selected splat whose word is rgba (R | G << 8 | B << 16 | A << 24), by the
 * kernel's own function; W = 0 returns rgba.  out NULL: GS_E_BADARG. */
GS_API int gs_highlight_word(uint32_t rgba, uint32_t option_value, uint32_t *out);
/* Real deletion: every hidden splat leaves the resident arrays (both 16-byte records, the sort rows, the strip bounds, the SH rows of
 * the kept splats among those that have one, the states -- hidden bit gone by definition, the other bits travel with the splat), in
 * stable order.  out_old_index (optional, capacity gs_count() BEFORE the call): out_old_index[k] = the old index of new splat k;
 * *out_n (optional) = gs_count() afterwards.  The arrays are compacted into fresh ones that are then swapped in: for the duration of
 * the call the resident bytes are held TWICE.  Afterwards the context is indistinguishable from one that was pushed the kept rows
 * (orders, hints and measured shares are dropped as by gs_clear).  A sort posted with gs_sort_begin and not yet collected is run
 * again over the kept splats when gs_sort_poll collects it (nothing kept: its reply is the empty context's [0]).  Nothing hidden:
 * nothing happens (*out_n = gs_count()). */
GS_API int gs_compact(gs_ctx *ctx, uint32_t *out_old_index, size_t *out_n);
/* Changing resident splats in place.
 * COLOUR AND OPACITY, on the GPU: an affine map of the colour and a linear one of alpha for the splats with (state & state_mask) ==
 * state_value.  THE RULE -- one function, csrc/gs_adjust.h, called by the kernels and by the two host evaluators below -- is, every
 * operation IEEE f64, un-fused, on the parameters widened from f32, in this order:
 *   word   of R | G << 8 | B << 16 | A << 24:  v_c = ((m[3c] * R + m[3c+1] * G) + m[3c+2] * B) + offset[c];  byte c = clamped_u8(v_c);
 *          A' = clamped_u8(alpha_scale * A + alpha_offset);  clamped_u8: clamp to [0, 255], round to nearest, ties to even, NaN -> 0.
 *   SH row of degree D, K = (D+1)^2 coefficients per channel (the colour before the clamp is affine in them, so the same map applies):
 *          sh'[c][k] = (float)((m[3c] * sh[0][k] + m[3c+1] * sh[1][k]) + m[3c+2] * sh[2][k])  for k >= 1, and for k = 0 the same sum
 *          + ((0.5 * ((m[3c] + m[3c+1]) + m[3c+2]) + offset[c] / 255) - 0.5) / SH_C0, SH_C0 = 0.28209479177387814, before the f32
 *          rounding.  The three new values of a k come from the three old ones.  Alpha has no SH part.
 * The identity (unit matrix, zero offsets, alpha 1 and 0) gives back every word, and every finite SH row (its constant is exactly 0; a
 * coefficient -0 may come back +0).  The byte and the SH row of one splat are adjusted INDEPENDENTLY: bytes clamp, coefficients do
 * not, so afterwards the degree-0 evaluation of a row need not equal the byte any more.  A parameter that is not finite: GS_E_BADARG. */
typedef struct gs_colour_adjust {
    float m[9];          /* row-major 3x3: out channel c reads m[3c+0..2] */
    float offset[3];     /* in units of one colour byte */
    float alpha_scale, alpha_offset;   /* alpha' from the alpha byte, byte units */
} gs_colour_adjust;
/* The colour word of every passing splat (a splat beyond the state store has state 0) is rewritten in place -- a 4-byte read-modify-write;
 * nothing else of the record is touched -- and, where the splat has an SH row, that row too.  *out_hit (optional): the passing splats.
 * Frames in flight read both arrays, so every lane is drained first; the depth sort never reads colour, so NO order is dropped: the
 * next render of the last completed order shows the change.  gs_sync() does not draw frames of before the change again by itself.
 * ONE thing the sort does hold of the alpha byte: the sort row's fourth word, (largest scale) x alpha / 255 as packed at push time, on which
 * the sort culls splats smaller than 0.0001 |depth| (index.js:397, 548).  The sort rows are left alone, so that cull keeps judging by the
 * alpha of the push: a splat faded to alpha 0 stays in the order (and draws with weight 0), one that was culled stays culled.  A host that
 * wants the cull to follow writes the rows back with gs_replace_splat, which packs them again.  The
 * state store is neither grown nor changed; the hidden count and the contribution store stay.  Two streaming kernels of their own on
 * the context's stream; the call waits for them.  Matrices-only context: GS_E_STATE.  Nothing resident: hit 0, GS_OK. */
GS_API int gs_adjust_colour(gs_ctx *ctx, const gs_colour_adjust *adjust, uint8_t state_mask, uint8_t state_value, size_t *out_hit);
/* host, no context, no GPU: one word, and one SH row (tight, as gs_push_sh takes it; degree 0..3; out_row may be sh_row), by the rule
 * above.  NULL pointers, a parameter that is not finite, a degree out of range: GS_E_BADARG. */
GS_API int gs_adjust_word(uint32_t rgba, const gs_colour_adjust *adjust, uint32_t *out);
GS_API int gs_adjust_sh_row(const float *sh_row, int degree, const gs_colour_adjust *adjust, float *out_row);
/* ROWS: splats [first, first + nrows) are overwritten with .splat rows packed by the pack kernel of gs_push_splat: both records, the sort
 * row and the strip bound.  States, SH rows, contribution words and gs_count() stay.  Otherwise like a push: lanes drained, every
 * lane's order dropped, a sort posted with gs_sort_begin is run again when it is collected.  With gs_export_splat (and its wide parts)
 * a host can rewrite whatever it likes of the rows it touched; to move, rotate or scale part of the cloud use gs_transform (below), which
 * keeps the record's precision (a row's quaternion is four bytes), turns the SH rows along and moves no row across the bus.
 * first + nrows > gs_count(): GS_E_BADARG, nothing changed.  Matrices-only context: GS_E_STATE.  nrows == 0: GS_OK. */
GS_API int gs_replace_splat(gs_ctx *ctx, size_t first, const void *rows, size_t nrows);
/* SH rows [first, first + nrows) of the store are overwritten (tight rows in, padded as by gs_push_sh).  Lanes drained, no order dropped.
 * A degree other than the store's, or a range beyond gs_sh_count(): GS_E_BADARG. */
GS_API int gs_replace_sh(gs_ctx *ctx, size_t first, const float *sh_rows, size_t nrows, int degree);
/* POSITION, ROTATION AND SIZE, on the GPU: the similarity p' = scale * R p + translation, baked once into the splats with (state &
 * state_mask) == state_value (there is no per-frame pose).  THE RULE -- one function, csrc/gs_transform.h: transform_record, called by the
 * kernel and by gs_transform_record below -- is, every operation IEEE f64, un-fused, on the parameters widened from f32, in this order:
 *   1. q = rotation / n, n = sqrt(((w^2 + x^2) + y^2) + z^2).
 *   2. R (rows' space) from q by the expressions of the pack loop (csrc/gs_device_math.h: pack_row, the r00 .. r22 lines).
 *   3. Rm = R in the packed, z-mirrored space: Rm[i][j] = R[i][j], negated where exactly one of i, j is 2.
 *   4. p = (cs[0], cs[1], -cs[2]);  p'_i = scale * ((R_i0 p_0 + R_i1 p_1) + R_i2 p_2) + translation_i;  cs'[0..2] = (f32 p'_0, f32 p'_1, f32 -p'_2).
 *   5. A record whose cs[3] is not finite (decided on its bits) keeps cs[3] and cc[0..2].  Otherwise, if all nine entries of R compare equal
 *      to the identity's, cc[0..2] are copied and cs'[3] = cs[3] if scale == 1, else f32(cs[3] * (scale * scale)): a pure translation never
 *      touches the covariance, a pure scale never touches the int16 words.
 *   6. Otherwise A = the symmetric matrix the export dequantises (int16 * cs[3], f64); B_ik = (Rm_i0 A_0k + Rm_i1 A_1k) + Rm_i2 A_2k;
 *      E_ij = ((B_i0 Rm_j0 + B_i1 Rm_j1) + B_i2 Rm_j2) * (scale * scale) for (0,0), (1,0), (2,0), (1,1), (2,1), (2,2); max_value = the largest
 *      |E|; cs'[3] = f32(max_value / 32767); each int16 = E * 32767 / max_value rounded to nearest, ties to even, clamped to [-32767, 32767],
 *      NaN -> 0.  (NOT the truncation of the pack loop's parseInt: a truncating quantiser shrinks the splat with every edit.)
 *   7. cc[3], the colour word, stays.
 *   8. sort row = (cs'[0], cs'[1], cs'[2], f32(sort_row[3] * scale)): the size cull of the sort follows the scale.
 *   9. The strip bound is the pack kernel's expression on cs'[3].
 * The identity gives back every bit of a record with a finite position (a coordinate -0 may come back +0; a NaN is a NaN: its sign and
 * payload are not part of the rule, and one NaN coordinate makes all three NaN).  Each general edit costs at
 * most half a quantisation step of cs'[3] per covariance entry; translations and scales cost the covariance nothing.
 *   SH rows: scale and translation leave them alone.  Under a rotation the coefficients of band l = 1..3 (k = 1..3, 4..8, 9..15) go through
 * the band's matrix D_l: sh'[c][k0 + i] = f32(sum_j D_l[i][j] * sh[c][k0 + j]), summed in ascending j; k = 0 stays.  The matrices are built on
 * the host, once per call, in f64 from + - * / sqrt, for the basis exactly as csrc/gs_sh.h orders and signs it, so that for every camera
 * and position gs_sh_eval_unrounded(sh', D, scale R cam + t, scale R pos + t) = gs_sh_eval_unrounded(sh, D, cam, pos) up to the rounding of
 * the coefficients.  An exact identity R gives exact identity matrices, and the SH kernel is not launched at all. */
typedef struct gs_similarity {
    float rotation[4];      /* quaternion (w, x, y, z) in the ROWS' object space (as a .ply / .splat row stores positions: the space of
                               gs_select_sphere and GS_PROP_X..Z); need not be normalised */
    float scale;            /* uniform, finite, > 0 */
    float translation[3];   /* rows' object space */
} gs_similarity;            /* p' = scale * R p + translation */
/* Rewrites, for every passing splat (a splat beyond the state store has state 0): both halves of the 32-byte record except the colour
 * word, the sort row, the strip bound and, where the splat has one, its SH row.  *out_hit (optional): the passing splats.  States (the
 * store neither grows nor changes), the contribution store, gs_count(), the SH store's length and degree, every option and statistic
 * stay.  Otherwise like gs_replace_splat: lanes drained, every lane's order dropped (a render before the next sort draws the background
 * only), a sort posted with gs_sort_begin is run again when it is collected, gs_sync() does not draw frames of before the change again
 * by itself.  Two streaming kernels of their own on the context's stream; the call waits for them.  Matrices-only context: GS_E_STATE.
 * Nothing resident: hit 0, GS_OK.  NULL t, a parameter that is not finite, scale <= 0, a quaternion of norm 0: GS_E_BADARG.
 * Out of scope: non-uniform scale, shear and mirroring; per-frame poses or groups; a transform applied at push time. */
GS_API int gs_transform(gs_ctx *ctx, const gs_similarity *t, uint8_t state_mask, uint8_t state_value, size_t *out_hit);
/* host, no context, no GPU: the kernels' own functions.  One record (the outputs may be the inputs; bound_out, optional: the strip bound),
 * one SH row (tight, as gs_push_sh takes it; degree 0..3; out_row may be sh_row), the band matrices the kernel is handed (3x3, 5x5, 7x7,
 * row-major, in that order: 83 doubles), and the similarity that rotates and scales about a pivot: rotation and scale copied, translation
 * = f32(pivot - scale * R pivot), R as in steps 1-2, the sum as in step 4, f64, rounded once.  NULL pointers (but bound_out), a bad
 * similarity as above, a degree out of range: GS_E_BADARG. */
GS_API int gs_transform_record(const float cs[4], const uint32_t cc[4], const float sort_row[4], const gs_similarity *t,
                               float cs_out[4], uint32_t cc_out[4], float sort_row_out[4], float *bound_out /* optional */);
/* ... and n records in one call: arrays of n x 4 as gs_download returns them, each through gs_transform_record's function (bounds_out optional) */
GS_API int gs_transform_records(const float *cs, const uint32_t *cc, const float *sort_rows, size_t n, const gs_similarity *t,
                                float *cs_out, uint32_t *cc_out, float *sort_rows_out, float *bounds_out /* optional */);
GS_API int gs_transform_sh_row(const float *sh_row, int degree, const gs_similarity *t, float *out_row);
GS_API int gs_sh_rotation(const gs_similarity *t, double out[83]);
GS_API int gs_similarity_about(const float pivot[3], const float rotation[4], float scale, gs_similarity *out);

/* Scene compositing inputs (reference: the splat mesh is drawn in three.js' transparent pass with depthTest: true,
 * depthWrite: false over the opaque scene, index.js:177-181): an optional window-space depth buffer of that scene
 * (GL convention: 0 = near plane, 1 = far plane; a fragment survives iff its depth zndc*0.5+0.5 <= the buffer, LEQUAL)
 * and an optional RGBA8 colour image that replaces the constant background.  Both fb_width x fb_height, tightly packed,
 * row 0 = top, host memory (copied); NULL for either = not used; gs_set_scene(ctx, NULL, NULL, 0, 0) clears.
 * Renders whose fb_width/fb_height differ from the scene's fail with GS_E_BADARG (gs_render, gs_render_surface, gs_render_contrib,
 * gs_render_stereo alike; after gs_set_scene(ctx, NULL, NULL, 0, 0) the context draws as before).
 * Pinned by tests/test_scene_edges_gpu.py on every blend path:
 *   - the test is zwin <= depth in f32, zwin = zndc * 0.5f + 0.5f: EQUALITY SURVIVES (a host that passes the depth plane of
 *     gs_render_surface back in keeps the surface splat), one ulp below rejects.  A NaN depth (either sign, any payload) rejects every fragment of the
 *     pixel.  Depth values are compared as they are, not clamped: zwin lies in [0, 1], so negatives and -inf reject all, +inf and
 *     anything >= 1 accept all, and 0, -0 and denormals reject every splat behind the near plane.
 *   - the scene's alpha byte takes part as dst.a: out.a = a + dst.a * (1 - a), dst.a = byte / 255; where nothing is drawn all four
 *     bytes of the scene come back exactly.  With rgba set the background is not used; with depth alone it is the destination.
 *   - GS_RENDER_FLIP_Y flips the output, not the scene: depth and rgba are read at the image row (row 0 = top), the pixel is
 *     written at the flipped row -- the flipped frame is the plain frame upside down.
 *   - a strip reads the depth plane under the pixels it blends, up to its right edge rounded up to four pixels inside the frame. */
GS_API int gs_set_scene(gs_ctx *ctx, const float *depth, const uint8_t *rgba, int fb_width, int fb_height);

/* Page-locked host memory for framebuffers (gs_render copies into it at PCIe speed, no staging copy; the N-API addon hands
 * it to JavaScript as an external ArrayBuffer).  Free with gs_host_free. */
GS_API void *gs_host_alloc(size_t nbytes);
GS_API void gs_host_free(void *p);

/* Block until all work queued on the context's stream is done; collects the status and statistics of frames
 * rendered with GS_RENDER_ASYNC on any lane (GS_E_RETRY if one of them overflowed the pair buffers). */
GS_API int gs_sync(gs_ctx *ctx);
/* Run the context's kernels on a caller-owned hipStream_t (e.g. torch's current stream). NULL = own stream.
 * On a caller-owned stream every frame is ordered with the caller's other work on it, so frames are not pipelined
 * over lanes (GS_OPT_PIPELINE_DEPTH is ignored); use the two calls below to couple pipelined frames to other streams. */
GS_API int gs_set_stream(gs_ctx *ctx, void *hip_stream);
/* GPU-side ordering between pipelined frames and the caller's own streams (no host blocking; what such a consumer reads may be an
 * INCOMPLETE frame: test gs_frame_status_device()'s word, below):
 * gs_wait_stream: the NEXT frame (next gs_sort + its renders) starts only after everything queued on hip_stream so
 *                 far, e.g. a collective that still reads the buffer that frame will render into;
 * gs_stream_wait_frame: hip_stream waits for the frame enqueued LAST (its gs_sort + renders so far), e.g. before a
 *                 collective or copy on that stream consumes the frame's device_rgba. */
/* The hipStream_t the current frame (last gs_sort + its renders) was enqueued on: work the caller queues on it -- a
 * collective over the frame's device_rgba, a copy -- is ordered after the frame and before the frame that will reuse
 * this lane, without any cross-stream event (those cost ~50 us of pipeline stall each on this platform). */
GS_API void *gs_frame_stream(gs_ctx *ctx);
/* ASYNCHRONOUS FRAMES ARE SPECULATIVE until gs_sync().  A frame queued with GS_RENDER_ASYNC may skip its second binning round (the
 * share of splats binned first has been measured over the frames before) or bin into buffers sized from the frames before; if a tile
 * then turns out not to be saturated, or the buffers to be too small, the frame is INCOMPLETE and gs_sync() draws it again (or asks
 * for it: GS_E_RETRY).  The reference never draws from an incomplete order either (index.js:201-207: the draw uses the latest
 * COMPLETED sort).  A consumer that reads the frame on the GPU before gs_sync() -- work queued on gs_frame_stream(), a stream coupled
 * through gs_stream_wait_frame(), the library's own gather -- must therefore test the frame's completion word:
 *   gs_frame_status_device(): *device_word = the device address of ONE uint32 of the current frame's lane, written by the frame's own
 *   kernels: 0 = complete; non-zero = the frame will be drawn again at gs_sync() (bit 0: a tile was not saturated, bit 1: the pair
 *   buffers overflowed, bit 2: the sorted order was incomplete).  Valid once the frame's kernels have run (in stream order behind
 *   the frame) until the lane has been handed 64 more renders (every lane keeps a ring of 64 words: gs_sync() itself reads them and
 *   draws again exactly the frames whose word is not 0); for a gathered frame,
 *   on the root: the OR of the words of all its pieces (each piece travels with its own word, the root's gs_sync() reports the
 *   frame even if only a peer's piece was incomplete).  Several renders of one frame on one context (gs_render_stereo): the word
 *   describes the last of them. */
GS_API int gs_frame_status_device(gs_ctx *ctx, void **device_word);
/* The same in two steps, for callers that want to keep enqueuing: gs_frame_lane() names the lane of the current frame
 * (no waiting); gs_lane_stream() returns that lane's stream once its worker thread has enqueued everything handed to
 * the lane so far.  Queuing the follow-up work of frame k only after frame k+1 (or k+2) has been handed over keeps the
 * caller from waiting for the worker; it must still be queued before the lane is given its next frame. */
GS_API int gs_frame_lane(gs_ctx *ctx);
GS_API void *gs_lane_stream(gs_ctx *ctx, int lane);
GS_API int gs_wait_stream(gs_ctx *ctx, void *hip_stream);
GS_API int gs_stream_wait_frame(gs_ctx *ctx, void *hip_stream);

/* ---- several GPUs (no reference counterpart: the reference draws on one WebGL context) ------------------------------
 * The viewport is split into tile-aligned column strips (or, for XR, the two eyes go to different GPUs), the splat buffer is
 * replicated, every context sorts for the same view and renders its own pieces, and the pieces are gathered on one root
 * over RCCL (xGMI).  One gs_ctx per GPU: one process per GPU (the launcher distributes the id: torch.distributed, MPI, a
 * file) or several contexts in one process.  RCCL is loaded (dlopen "librccl.so.1") by gs_comm_init, not before: a
 * single-GPU user never needs it.  Every rank must issue the same sequence of gs_sort / gs_render_*_gathered calls. */
#define GS_COMM_ID_BYTES 128
/* rank 0: create the id all ranks pass to gs_comm_init (ncclGetUniqueId) */
GS_API int gs_comm_unique_id(gs_ctx *ctx, void *id_out);
/* join the communicator as `rank` of `world` (ncclCommInitRank; collective: returns when every rank has called).
 * In-process transport (GS_OPT_COMM_TRANSPORT = 1): never blocks.  A receive of that transport waits ON THE HOST for its sender to
 * post (GS_COMM_TIMEOUT_S, default 60 s), so ONE thread that drives several such ranks with SYNCHRONOUS gathered frames has to call
 * the non-root ranks first and the root last (queued frames -- GS_RENDER_ASYNC -- and gs_create_multi, one thread per rank, have no
 * such order).  A failed exchange is final, as with an aborted RCCL communicator: the rank that gave up has skipped an operation
 * its peers performed; destroy the communicator on every rank and join a new one. */
GS_API int gs_comm_init(gs_ctx *ctx, const void *id, int rank, int world);
GS_API int gs_comm_destroy(gs_ctx *ctx);

/* Who renders what: nviews images of widths[v] pixels over `world` ranks -> pieces (view, [x0,x1), owner rank), in the
 * order they are gathered.  One view: tile-aligned column strips, as even as possible, the last strip takes the ragged
 * edge.  Two views (XR eyes, index.js:13-15): world 1 renders both; otherwise the ranks are divided between the eyes (eye k ->
 * rank k at world 2) and each eye is split in strips over its ranks.  Returns the number of pieces (<= max_pieces) or < 0. */
typedef struct gs_piece { int32_t view, x0, x1, owner; } gs_piece;
GS_API int gs_partition(int nviews, const int *widths, int world, gs_piece *out, int max_pieces);

/* One frame over all ranks: each renders its pieces of the view(s) with the order of its last gs_sort() and sends them to
 * `root`, where they are assembled into row-major RGBA8 images: device_frames[v] (device memory, fb_width x fb_height x 4
 * tight) or, if NULL, buffers of the context readable with gs_read_gathered().  views[v].x0/x1 are ignored (the partition
 * sets them).  flags: GS_RENDER_ASYNC enqueues and returns (completion and status at gs_sync()); GS_RENDER_FLIP_Y applies
 * per view.  nviews = 2 is the XR frame: two eyes, ONE shared sort from the head camera (index.js:441). */
GS_API int gs_render_gathered(gs_ctx *ctx, const gs_render_params *views, int nviews, int root, void *const *device_frames,
                              uint32_t flags);
/* The sort of a gathered frame: gs_sort_for the piece gs_partition gives this rank when it owns exactly one column strip of
 * one view (the sort, projection and binning of an 8-GPU frame then shrink with the strip instead of being replicated), a plain
 * gs_sort otherwise.  Call it with the views the following gs_render_gathered draws. */
GS_API int gs_sort_gathered(gs_ctx *ctx, const float view[4], const float *cutout16, const gs_render_params *views, int nviews);
/* root: copy view `view` of the last gathered frame (after gs_sync() for asynchronous frames) to host memory */
GS_API int gs_read_gathered(gs_ctx *ctx, int view, uint8_t *rgba_out, size_t stride);
/* ... and its size in pixels (so that a binding can check the caller's buffer before the copy) */
GS_API int gs_gathered_size(gs_ctx *ctx, int view, int *width, int *height);
/* ---- one host process, several GPUs (the reference is one JavaScript thread per page, index.js:1-23, with
 * several component instances allowed, cutout-demo.html:24-25 -- a Node.js consumer cannot be one process per GPU) ----------
 * A gs_multi owns one context per entry of `devices` (an ordinal may repeat: several "devices" on one GPU, which is how the
 * single-GPU test tier runs it), keeps the splat buffer replicated on them and splits every frame as gs_partition says: column
 * strips of one view, or the two XR eyes over the devices.  The calls have the single-context meaning and signatures; each
 * context is fed by its own thread, so an asynchronous frame costs the caller the same whatever the number of GPUs.
 * The communicator between the contexts is the in-process transport (GS_OPT_COMM_TRANSPORT = 1), set up by gs_create_multi. */
typedef struct gs_multi gs_multi;
GS_API int gs_create_multi(const int *devices, int ndev, gs_multi **out);
GS_API int gs_multi_destroy(gs_multi *m);
GS_API const char *gs_multi_last_error(const gs_multi *m);   /* m == NULL: the last gs_create_multi failure of the calling thread */
GS_API int gs_multi_devices(const gs_multi *m);
/* the context on devices[i] (statistics, downloads, per-context options); only between gs_multi_sync() and the next frame */
GS_API gs_ctx *gs_multi_ctx(gs_multi *m, int i);
GS_API int gs_multi_clear(gs_multi *m);                                              /* gs_clear on every device          */
GS_API int gs_multi_push_splat(gs_multi *m, const void *rows, size_t nrows);         /* gs_push_splat, uploads in parallel */
GS_API int gs_multi_load_ply(gs_multi *m, const void *bytes, size_t nbytes);
GS_API int gs_multi_push_sh(gs_multi *m, const float *sh_rows, size_t nrows, int degree);   /* gs_push_sh on every device     */
/* the editing calls on every device; hit counts and the index map are those of devices[0] (every device holds the same splats; a
 * gs_multi_select_rect walks each device's own whole order of the same view) */
GS_API int gs_multi_set_state(gs_multi *m, size_t first, const uint8_t *states, size_t n);
GS_API int gs_multi_set_state_ids(gs_multi *m, const uint32_t *ids, size_t n, uint8_t set_bits, uint8_t clear_bits);
GS_API int gs_multi_select_box(gs_multi *m, const float box16[16], uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit);
GS_API int gs_multi_select_sphere(gs_multi *m, const float centre[3], float radius, uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit);
GS_API int gs_multi_select_rect(gs_multi *m, const gs_render_params *p, const int32_t rect[4], uint8_t set_bits, uint8_t clear_bits, uint32_t flags,
                                size_t *out_hit);
GS_API int gs_multi_select_mask(gs_multi *m, const gs_render_params *p, const uint8_t *mask, size_t mask_stride, const float *depth_max, uint8_t set_bits,
                                uint8_t clear_bits, uint32_t flags, size_t *out_hit);
GS_API int gs_multi_compact(gs_multi *m, uint32_t *out_old_index, size_t *out_n);
/* the in-place changes on every device; the hit count is devices[0]'s */
GS_API int gs_multi_adjust_colour(gs_multi *m, const gs_colour_adjust *adjust, uint8_t state_mask, uint8_t state_value, size_t *out_hit);
GS_API int gs_multi_replace_splat(gs_multi *m, size_t first, const void *rows, size_t nrows);
GS_API int gs_multi_replace_sh(gs_multi *m, size_t first, const float *sh_rows, size_t nrows, int degree);
GS_API int gs_multi_transform(gs_multi *m, const gs_similarity *t, uint8_t state_mask, uint8_t state_value, size_t *out_hit);
GS_API size_t gs_multi_count(const gs_multi *m);
GS_API int gs_multi_set_option(gs_multi *m, int option, int64_t value);              /* gs_set_option on every device     */
/* tick + worker sort for the frame `views` describe (one view, or the two XR eyes with the head camera's view row, index.js:441):
 * every device sorts what its own piece of the frame needs (gs_sort_gathered).  Asynchronous: failures surface at the next
 * synchronous render or gs_multi_sync(). */
GS_API int gs_multi_sort(gs_multi *m, const float view[4], const float *cutout16, const gs_render_params *views, int nviews);
/* HOST-DIRECT frame: host_frames[v] is the caller's fb_width x fb_height RGBA8 image (`stride` bytes per row, 0 = tight; page-
 * locked memory from gs_host_alloc lets the copies overlap the next frames); every device copies its strip straight into its
 * columns behind its kernels -- no collective, no staging, no assembly.  Without GS_RENDER_ASYNC the call returns with the frame
 * complete (and has drawn it again by itself if a device reported GS_E_RETRY); with it, completion and status come from
 * gs_multi_sync(), one frame buffer per frame in flight. */
GS_API int gs_multi_render(gs_multi *m, const gs_render_params *views, int nviews, uint8_t *const *host_frames, size_t stride, uint32_t flags);
/* DEVICE frame: gathered on devices[0] through the in-process transport (peer copies on the frames' own streams) into
 * device_frames[v] (memory of devices[0]) or, if NULL, into buffers read with gs_multi_read(). */
GS_API int gs_multi_render_device(gs_multi *m, const gs_render_params *views, int nviews, void *const *device_frames, uint32_t flags);
GS_API int gs_multi_read(gs_multi *m, int view, uint8_t *rgba_out, size_t stride);
/* gs_sync on every device: GS_E_RETRY if any asynchronous frame since the last sync has to be drawn again */
GS_API int gs_multi_sync(gs_multi *m);

#define GS_OPT_BLEND_SPLIT 9    /* 0 (default): one wavefront blends each tile, 4 pixels per lane.  L > 0: tiles whose list has at least
                                   L entries (try 512) are blended by FOUR wavefronts, one pixel per lane -- for frames in which few
                                   tiles carry long lists (a cut-out scene: the kernel otherwise lasts as long as ONE wavefront's
                                   serial walk of the busiest tile's list).  Same fragments and per-pixel operations; a pixel of such
                                   a tile stops exactly when it falls below the termination threshold instead of with its lane's
                                   other three (within the 1 LSB tolerance), so images are bit-identical only between renders with
                                   the same setting AND the same binning share: off by default.  The rule is per tile: strips
                                   still equal the full frame bit for bit. */
#define GS_OPT_FRAME_BATCH 10   /* 1 (default): every frame is its own chain of launches.  2: consecutive asynchronous frames
                                   (gs_sort without an output array + gs_render / gs_render_device with GS_RENDER_ASYNC) are
                                   paired: the two frames of a pair share every kernel launch (grid (x, 2): each frame keeps
                                   its own sort, projection, binning and blend on its own scratch; pixels are identical to
                                   unpaired rendering), and 2 x GS_OPT_PIPELINE_DEPTH frames are in flight.  A frame of
                                   ~1 M splats is a chain of 18 short kernels at the launch floor: sharing them is worth
                                   ~20 % in frames/s.  Pairing happens in the lanes' enqueue threads when both frames are
                                   queued (needs GS_OPT_ENQUEUE_THREADS); gathered frames of one piece per rank pair as well
                                   (their gathers follow the shared kernels in frame order); frames that differ in size,
                                   flags or path go out alone.                                                              */
#define GS_OPT_SORT_NEAR 11     /* near-only depth sorts.  A frame whose second binning round is skipped (the share has been clean
                                   for a few frames) reads only the nearest share of the order; its gs_sort then leaves out the
                                   splats that cannot be among those, so that the positions the frame reads hold exactly what the
                                   whole order holds there.  Up to 2 M splats (the four-launch sort): a TAIL sort -- the order is cut
                                   at the boundary of the 256 depth segments the sort works in anyway, the segments before the cut
                                   are neither scattered nor sorted.  Longer inputs: an exact threshold on the sort key from a
                                   histogram of the depths, applied before the radix passes.  A render that needs more of the
                                   order after all (another share, a counting render, round 1, gs_download of the order) sorts
                                   again in full by itself.  Sorts that return the order (out_idx / out_n) are always complete.
                                   0: off; 1 (default): tail sorts up to 2 M splats, the histogram form from 4 M (between the two
                                   its extra work costs what it saves); 2: always.                                               */
#define GS_OPT_SORT_SHARE 15    /* several ranks (gs_sort_gathered), value = permille P of the splats, 0 = off (default).  The depth sort is the
                                   part of a frame that does not shrink with a rank's strip: every rank keys and sorts all N splats of every
                                   frame (at 20 M splats 230 of a strip frame's 290 us).  With P > 0 the ranks take turns: frame f is
                                   sorted by rank f mod world alone -- a near-only sort of the nearest P/1000 * N splats of the WHOLE view,
                                   the same kernels, hence the same order -- which sends it (a few MB, one send per peer, each over its own
                                   xGMI link) to the others; those receive it where their own sort would have run.  Every rank then draws
                                   its pieces from that order exactly as after gs_sort(): same pixels.  A frame that needs more of the
                                   order than was exchanged (its first binning round reads more than P/1000 * N splats, or did not skip
                                   the second one) sorts again in full locally, as after any near-only sort.  Set the same value on every
                                   rank, before the frames; needs N <= 2^25.                                                        */
/* (option 14, GS_OPT_HOST_WRITE -- the blend kernel storing its tiles straight into a page-locked host frame -- was measured in rounds 3
   and 4: no faster for a frame alone, 25 % slower with frames in flight; removed in round 5.  The copy engine delivers host frames.) */
#define GS_OPT_AUTO_RETRY 13    /* 1 (default): gs_sync() draws an asynchronous frame that came back incomplete again by itself -- same sort
                                   arguments, same uniforms, same output buffers, both binning rounds -- before it returns; GS_E_RETRY is
                                   left for the cases it cannot decide alone (see gs_status).  0: every such frame is reported.       */
#define GS_OPT_COMM_TRANSPORT 12 /* what gs_comm_unique_id makes an id for.  0 (default): RCCL over xGMI, one process per GPU or several contexts
                                   of one process.  1: the in-process transport -- contexts of ONE process (on different GPUs, or all on
                                   the same one) exchange their pieces through mailbox buffers and peer copies on their own streams,
                                   ncclSend / ncclRecv semantics, no RCCL; gs_comm_init with such an id never blocks, so one thread can
                                   bring all ranks up (gs_create_multi does).  Set it on the context that creates the id; the other
                                   ranks recognise the id.                                                                      */
#define GS_OPT_COMM_SELF_COPY 8 /* value != 0: the root sends its own pieces to itself through RCCL too instead of rendering them
                                   in place (exercises send/recv on a single-GPU box; slower) */

/* ---- uniforms / camera helpers (host side; reference: tick + camera matrices, index.js:438-487) ------ */

/* getModelViewMatrix: camera.matrixWorld, object.matrixWorld (column-major f64) -> gsModelViewMatrix */
GS_API void gs_model_view_matrix(const double cam_world[16], const double obj_world[16], double out[16]);
/* getProjectionMatrix: camera.projectionMatrix -> gsProjectionMatrix */
GS_API void gs_projection_matrix(const double proj[16], double out[16]);
/* three.js Matrix4.makeOrthographic(left, right, top, bottom, near, far), WebGL convention (z to [-1, 1]), column-major f64, in three.js'
 * operation order: an OrthographicCamera's projectionMatrix.  Feed it through gs_projection_matrix like any camera.projectionMatrix and
 * draw with GS_RENDER_PARALLEL.  out NULL: GS_E_BADARG. */
GS_API int gs_ortho_matrix(double left, double right, double top, double bottom, double near_plane, double far_plane, double out[16]);
/* tick: the two messages posted to the worker: view[4] and (if cutout_world != NULL) cutout[16] */
GS_API void gs_tick_uniforms(const double cam_world[16], const double obj_world[16], const double *cutout_world,
                             float view[4], float cutout[16]);
/* onBeforeRender focal (index.js:191) */
GS_API double gs_focal(const double gs_proj[16], double viewport_h);
/* init: pixelRatio / xrPixelRatio (index.js:10-15): drawing-buffer size = floor(css * ratio) when ratio > 0 */
GS_API void gs_scaled_size(int css_w, int css_h, double ratio, int *out_w, int *out_h);

/* ---- stats / introspection ---------------------------------------------------------------------- */

typedef struct gs_stats {
    uint64_t n_splats;    /* N resident                                                               */
    uint64_t n_sorted;    /* V  = length of the last sort result                                      */
    uint64_t n_visible;   /* Vp = splats surviving the vertex-shader culls in the last render          */
    uint64_t n_pairs;     /* I  = (tile,splat) pairs binned in the last render                         */
    uint64_t n_frags;     /* reference-equivalent fragments (last GS_RENDER_COUNT_FRAGS render)        */
    uint64_t n_tiles;     /* tiles in the last rendered strip                                         */
    float ms_sort;        /* GPU time of the last gs_sort (HIP events; 0 unless profiling is on)       */
    float ms_project;
    float ms_bin;
    float ms_blend;
    float ms_render;      /* project + bin + blend                                                    */
    uint32_t blend_launches;
    /* accumulated since GS_OPT_PROFILE was last switched on (collected at gs_sync / synchronous renders)     */
    uint32_t prof_frames; /* frames whose HIP-event timings are summed below                                  */
    float sum_ms_sort, sum_ms_project, sum_ms_bin, sum_ms_blend;
    uint64_t acc_frames;  /* frames rendered (device-side counter)                                            */
    uint64_t acc_sorted;  /* sum of V over those frames                                                       */
    uint64_t acc_visible; /* sum of Vp                                                                        */
    uint64_t acc_pairs;   /* sum of I                                                                         */
    uint32_t unsat_tiles; /* tiles the nearest-splats round left unsaturated in the last collected frame             */
    uint32_t near_permille;/* share of the splats binned in that first round (adapted, or GS_OPT_NEAR_PERMILLE)        */
    uint32_t sort_records;/* records the last collected frame's depth sort carried through its second pass: the kept
                             splats with a valid bucket, or the nearest few of them (GS_OPT_SORT_NEAR)               */
    uint32_t retried_frames;/* asynchronous frames gs_sync() drew again by itself since the context was created (GS_OPT_AUTO_RETRY) */
    uint32_t spec_sorts;  /* collected frames whose near-only sort took its candidates from the depth pass' own stash (no depth
                             array written: a threshold hint from the previous frames decides what is stashed) ...              */
    uint32_t spec_misses; /* ... and those of them whose candidates could not be vouched for (drawn again from a whole sort)    */
    uint32_t need_splats; /* how many of the NEAREST splats the last collected frames' tiles read before they were saturated (max over
                             the tiles; 0xFFFFFFFF: a tile no share saturates): what near_permille is set from, with a margin of
                             15 % that shrinks to 4 % while no frame misses                                                        */
    uint32_t sort_mode;   /* how the last collected frame's depth sort ran: 0 = the whole order (the reference's, index.js:507-570); near-only
                             forms (GS_OPT_SORT_NEAR): 1 = threshold from a depth histogram, 2 = candidates from the depth pass' own stash,
                             3 = tail sort (the segments the frame does not read neither scattered nor sorted)                       */
    uint32_t subtile;     /* 1 if the last frame's blend walked sub-tile lists (GS_OPT_SUBTILE)                                        */
    uint32_t row_walk;    /* 1 if the last frame's first binning round built no tile lists: its blend walked the tile rows' runs (GS_OPT_ROW_WALK) */
    uint32_t binning;     /* how the last frame's first binning round binned (GS_OPT_BINNING): 0 = span lists, 1 = (tile, splat) pair records
                             (asked for, or a strip of more than 256 tile columns or rows, or a row-count table beyond its limit); a frame
                             that runs no round (nothing resident) reports what its round would have taken                             */
    uint32_t sh_degree;   /* the spherical-harmonics degree the last frame's projection evaluated (GS_OPT_SH_DEGREE): 0 = packed byte colours   */
    uint32_t n_hidden;    /* hidden splats (GS_STATE_HIDDEN) the last collected sort skipped (in front of `surface`: every field that a build
                             without the editing calls has keeps its place up to here)                                                  */
    uint32_t surface;     /* 1 if the last frame wrote surface planes (gs_render_surface, gs_pick)                                        */
    uint32_t antialias;   /* 1 if the last frame's projection compensated its opacities (GS_OPT_ANTIALIAS)                                */
    uint32_t seg_count;   /* 1 if the last frame's first binning round counted its runs per (tile row, segment) in a launch of its own
                             (k_seg_count + the k_lists form that adds those counts up: GS_OPT_SEG_COUNT); 0 where every k_lists item counted
                             its row itself, and for rounds that build no span lists (row walk, pair records, nothing resident)            */
    uint32_t n_runs;      /* tile-row runs of the last collected frame, both rounds (span-list binning: a splat meets a tile row in one run of
                             tiles); what GS_OPT_SEG_COUNT 1 and GS_OPT_ROW_WALK 1 decide from.  A pair-record frame leaves it as it was.
                             (These two sit at the end: every older field keeps its offset.)                                              */
} gs_stats;

#define GS_OPT_PROFILE 1        /* 1: bracket every stage with HIP events on the frame's stream (7 per frame); 2: only
                                   the blend kernel (2 per frame; sum_ms_blend / prof_frames); 3: like 2 but only on every
                                   4th frame of a lane (an event pair costs ~5 % of the pipelined frame rate); 0: off */
#define GS_OPT_TERMINATION 2    /* value = 1/eps: a pixel stops blending once its transmittance T < eps (default 1024, SURVEY.md 8a row 9:
                                   what lies behind then weighs < eps = 0.25 LSB of RGBA8 in total; the image stays within 1 LSB of the
                                   back-to-front result for any eps < 1/256 -- held by tests/test_scene_edges_gpu.py::test_termination_bound
                                   on every blend path, with and without a scene, for 256, 257, 1024, 4096 and 2^24 against the
                                   GS_RENDER_NO_EARLY_OUT frame.  4096 was the round-1 default: 9 % fewer frames/s) */
#define GS_OPT_NEAR_PERMILLE 3  /* occlusion-aware binning: 0 = adapt (default), 1..999 = bin that share of the nearest
                                   splats first and the rest only against unsaturated tiles, 1000 = single round      */
#define GS_OPT_RECORD_STAGED 4  /* value != 0: each render overwrites the tile-range table with (list entries staged,
                                   list length) per tile, readable with gs_download(GS_BUF_TILE_STATS) (measurement aid);
                                   value 2 records the entries the tile evaluated before it saturated instead of staged */
#define GS_OPT_PIPELINE_DEPTH 5 /* 1..4 (default 3): frames enqueued with GS_RENDER_ASYNC rotate over this many internal lanes
                                   (own HIP stream + own per-frame scratch, resident splat data shared), so the kernel
                                   chain of frame k+1 runs under the tail of frame k -- as the reference overlaps its
                                   worker sort with drawing.  A gs_sort() begins a frame; it moves to the next lane when
                                   the previous frame was handed off asynchronously.  1 = strictly one frame at a time   */
#define GS_OPT_WIDE_PAIRS 6     /* 1: the depth sort carries its general 8-byte (key, index) records whatever the number of splats -- the format of
                                   N > 2^25, where 4-byte records no longer hold bucket and index -- (same order; a test hook for that format on
                                   small inputs).  0 (default): 4-byte records up to 2^25 splats.  (Rounds 2-5: also the binning's record
                                   formats; since round 6 its (tile, position) records have ONE form, 8 bytes.)                     */
#define GS_OPT_BINNING 16       /* how a binning round turns visible splats into per-tile lists (same lists, same images).  0 (default): span
                                   lists -- every splat becomes one run of tiles per tile row it touches, and the runs of a tile row, in
                                   sorted order, are expanded into the row's tile lists by one thread per tile column: four launches per
                                   round (project, row scan, runs, lists; five with the segment counts of frames that hold many runs per
                                   tile row) -- wherever a strip has at most 256 tile columns and rows (4096 x 4096 pixels), i.e. for every
                                   BASELINE configuration; beyond that, and with 1: (tile, splat) pair records sorted by two stable radix
                                   passes (rounds 1-3; eight launches per round).                                                */
#define GS_OPT_SUBTILE 17       /* how the blend walks a tile's list (same pixels, bit for bit, whatever the value).  The reference's rasteriser shades
                                   only the fragments a quad covers (index.js:52-66, 166-176); a 16x16 tile's wavefront evaluates a list entry for
                                   all 256 pixels.  With sub-tile lists the wavefront splits every batch of 64 entries into the lists of the
                                   tile's sixteen 4x4-pixel blocks (which blocks an entry's ellipse can reach is worked out from its record when
                                   it is staged) and takes as many steps as the longest of them -- worth it where splats are small against a
                                   tile (the cloud seen from outside: a list entry covers a fifth of its tile).  0: never; 1 (default): in
                                   frames that follow collected frames whose visible splats touched fewer than 16 tiles each on average
                                   (GS_SUBTILE_RATIO in the environment overrides the 16); 2: always (a batch of large splats is still walked
                                   whole: the decision is per batch).                                                              */
#define GS_OPT_ROW_WALK 18       /* how the first binning round hands a tile its entries (same pixels, bit for bit, whatever the value).  With span
                                   lists (GS_OPT_BINNING 0) a tile's list is the runs of its tile row that cover its column, in order; the blend
                                   reads a list from its nearest end and stops where the tile saturates, so where splats are large most of the
                                   lists are written and never read.  With the row walk no lists are built (one launch less per frame): the
                                   blend collects each tile's entries from its row's runs, 64 runs per step, as far as it blends.  0: never
                                   (the lists); 1 (default): in frames that follow collected frames whose visible splats touched at least 32
                                   tiles each on average and whose tile rows held at most 8192 runs each; 2: always.  Renders that count
                                   fragments or record staged entries, sub-tile lists (GS_OPT_SUBTILE), the split blend (GS_OPT_BLEND_SPLIT)
                                   and the second binning round keep the lists.                                                     */
#define GS_OPT_SH_DEGREE 19      /* view-dependent colour.  0 (default): the reference's behaviour -- gs_load_ply keeps f_dc_* only, baked into the
                                   colour byte (index.js:725-729); nothing is retained, nothing evaluated, and the kernels are the ones that run
                                   without this option.  1..3: the highest spherical-harmonics band gs_load_ply keeps and a frame evaluates; the
                                   effective degree of a frame is min(value, degree of the stored rows) and may change between frames.  Such a
                                   frame's projection evaluates the colour of every splat it projects for the frame's camera (each eye and each
                                   strip its own) where it writes the projected record; binning and blend see that record only.  A singular
                                   model_view is GS_E_BADARG for such a frame.                                                       */
#define GS_OPT_ANTIALIAS 20      /* anti-aliased splats.  The vertex shader adds 0.3 px^2 to both diagonal terms of every projected covariance
                                   (index.js:139-141): the EWA low-pass filter WITHOUT its normalisation -- the drawn Gaussian gets wider and keeps
                                   its peak, so a splat whose variance is comparable to 0.3 px^2 gains energy (isotropic: (v + 0.3) / v).
                                   0 (default): the reference's behaviour; the kernels are the ones that run without this option.  1: every
                                   frame's projection writes alpha' = alpha * c into its record, all in f32, in this order, un-fused:
                                     det = cov00 * cov11 - cov01 * cov01      (the un-dilated covariance; two products, then the difference)
                                     c   = sqrt(min(max(det / (l1 * l2), 0), 1))   (l1, l2: the eigenvalues the quad is drawn with, l2 AFTER its
                                                                                    clamp at 0.1; a NaN ratio counts as 0)
                                   (Mip-Splatting / gsplat's `antialiased` mode, with the eigenvalues really drawn in the denominator so that
                                   the energy of what is drawn is conserved).  Only that float changes: quad geometry, bounds, tile coverage,
                                   runs, lists, n_visible, n_pairs and fragment counts are those of option 0, and a splat with c = 0 is still
                                   written, counted and binned.  The colour word keeps the packed alpha byte.  Taken per frame (each eye, each
                                   strip), may change between frames; combines with GS_OPT_SH_DEGREE; paired frames (GS_OPT_FRAME_BATCH) share
                                   the setting.  Any other value: GS_E_BADARG.  gs_antialias_factor evaluates c on the host.        */
#define GS_OPT_SEG_COUNT 21      /* how round 0 of a span-list frame that builds tile lists counts the runs that cover a tile column (same lists, same
                                   pixels, bit for bit, whatever the value).  A tile row's runs are cut into at most 16 segments, one k_lists
                                   workgroup each, and each needs per column the runs before its segment and in the whole row.  Either every
                                   workgroup counts its whole row itself, or a launch of its own (k_seg_count) leaves one difference array per
                                   segment and k_lists adds them up -- less work where rows hold many runs, one launch more where they hold few.
                                   0: never the separate launch; 1 (default): in frames that follow a collected frame of more than 4096 runs per
                                   tile row (gs_stats.n_runs; a fresh or cleared context has none: its first frame takes none); 2: always.
                                   The second binning round, row-walk rounds (GS_OPT_ROW_WALK) and pair-record rounds (GS_OPT_BINNING 1, strips
                                   beyond 256 tile columns or rows) are unaffected.  gs_stats.seg_count says what a frame took.  Any other
                                   value: GS_E_BADARG.                                                                               */
#define GS_OPT_ENQUEUE_THREADS 7 /* default 1: gs_sort() (without an output array) and gs_render_device(GS_RENDER_ASYNC) hand the
                                   frame to a worker thread of its pipeline lane, which does the ~18 kernel launches, so the
                                   launches of the frames in flight run in parallel; failures surface at gs_sync().  0: the
                                   calling thread launches everything itself                                            */
#define GS_OPT_SORT_NEAR_FORCE 22 /* a test hook (tests/test_near_sort_gpu.py), host only.  P > 0: a gs_sort / gs_sort_for that is not asked for the
                                   index list runs as a near-only sort of the nearest P positions whatever the share policy says -- share settled or
                                   not, GS_OPT_SORT_NEAR, the size thresholds and the last kept count are not looked at.  What a near-only sort needs
                                   stays required: compact records (no GS_OPT_WIDE_PAIRS, at most 2^25 splats) and a renderable context; without
                                   them the sort is a whole one.  The form is chosen from the size as always (gs_sort_info.form).  Frames drawn
                                   from such an order are right without further ado: a frame that reads more of the order than the lane holds
                                   sorts again in full first, as after any near-only sort.  0 (default): the policy decides.  Negative values, and
                                   values beyond 2^32 - 1: GS_E_BADARG.                                                              */
#define GS_OPT_HIGHLIGHT 23      /* a highlight colour for the selected splats.  value = R | G << 8 | B << 16 | W << 24 (u32): the colour and its
                                   weight W; W = 0 (default: 0) switches the option off whatever the colour bytes are.  With W > 0 and a non-empty
                                   state store, every frame's projection changes the colour word of each splat it writes a record for whose
                                   index is below the store's length and whose byte has GS_STATE_SELECTED: for each of the three colour bytes
                                     c' = (c * (255 - W) + h * W + 127) / 255      (unsigned integers, truncating; h = R, G or B)
                                   AFTER the spherical-harmonics colour where GS_OPT_SH_DEGREE is active; independent of GS_OPT_ANTIALIAS.  The
                                   alpha byte and the alpha float stay.  Only that word changes: geometry, coverage, runs, lists and every
                                   count are those of a frame without the option, and every binning and blend path, surface frames and
                                   gs_pick, strips, gathered and gs_multi frames see the record only.  Splats beyond the store are never
                                   highlighted; hidden ones are not in the order.  Taken per frame like GS_OPT_ANTIALIAS (each eye, each
                                   strip); changing it drops no order, while state changes take effect at the next sort as always; paired
                                   frames (GS_OPT_FRAME_BATCH) share the value.  While the option is off or the store is empty a frame
                                   launches the kernels it launches without the option (gs_highlight_info says what a frame took;
                                   gs_highlight_word evaluates the rule on the host).  Negative values and values beyond 2^32 - 1:
                                   GS_E_BADARG.                                                                                     */
GS_API int gs_set_option(gs_ctx *ctx, int option, int64_t value);
GS_API int gs_get_stats(gs_ctx *ctx, gs_stats *out);

/* The order of the current frame's lane AS IT LIES (a test hook; gs_download(GS_BUF_SORTED) sorts again in full first): waits for the lane,
   reads its control block and copies the n_records entries the lane's last sort left -- the whole order's positions
   [n_valid - n_records, n_valid) after a near-only sort, all n_kept positions (zero tail included) after a whole one.
   out_idx may be NULL (the counts only); cap: the entries out_idx has room for (fewer than n_records: GS_E_BADARG, info is filled).
   GS_E_STATE if the lane holds no order.
   The call is also a COLLECTION of that sort as far as the near-only sorts' own bookkeeping goes (what gs_sync / a synchronous frame
   do with near_overflow, spec_fail and the threshold-bin hint; the share policy sees nothing of it): after a sort whose chunk stash
   overflowed the context keeps to the histogram form, after a collected histogram / stash / spec sort the next one may take the spec
   form, a failed spec sort backs the form off.  An order reported incomplete is replaced by a whole sort of the same view before the
   call returns (the flags are cleared), so the lane never keeps an order a frame must not be drawn from. */
typedef struct gs_sort_info {
    uint32_t form;             /* 0 whole order, 1 histogram (threshold bucket from the depth histogram, whole-length passes), 2 spec (candidates
                                  stashed by the depth pass), 3 tail (cut at a segment boundary), 4 stash (survivors through per-chunk stashes) */
    uint32_t near_req;         /* positions the lane's sort was asked for (0: all) */
    uint32_t n_kept;           /* V: splats that survive the sort's culls */
    uint32_t n_valid;          /* V': of those, the ones with a bucket inside the table (whole order, 8-byte records: not counted, = V) */
    uint32_t n_records;        /* P: entries the lane holds */
    uint32_t order_incomplete; /* the lane does not hold what it claims (a stash overflowed, the spec form could not vouch for its candidates) */
    uint32_t near_overflow;    /* a chunk of the stash form had more survivors than its stash holds */
    uint32_t spec_fail;        /* spec form: 1 the threshold-bin hint was behind, 2 a candidate stash overflowed / the depth range does not suit it */
    uint32_t threshold_bin;    /* the context's threshold depth bin (sign-less f32 depth bits >> 20) as the last histogram / stash / spec sort of
                                  any lane left it: what the next spec sort's depth pass goes by */
    uint32_t reserved[3];
} gs_sort_info;
GS_API int gs_sort_inspect(gs_ctx *ctx, gs_sort_info *info, uint32_t *out_idx, size_t cap);

/* Copy a device-resident array back to the host (parity tests / debugging). */
#define GS_BUF_CENTER_SCALE 0 /* N x 4 f32   centerAndScaleData                                         */
#define GS_BUF_COV_COLOR 1    /* N x 4 u32   covAndColorData                                            */
#define GS_BUF_SORT_ROWS 2    /* N x 4 f32   worker row elements 12..15                                 */
#define GS_BUF_SORTED 3       /* V u32       last sort result                                           */
#define GS_BUF_PROJECTED 4    /* V x 8 f32   projected records of the last render (sorted order)         */
#define GS_BUF_TILE_COUNT 5   /* V u32       tiles touched per sorted splat in the last render            */
#define GS_BUF_TILE_STATS 6   /* tiles x 2 u32  (entries staged, list length) after a GS_OPT_RECORD_STAGED render  */
#define GS_BUF_UNSAT_MASK 7   /* tiles_y x ceil(tiles_x / 32) u32: one bit per tile the first binning round of the last render left
                                 unsaturated (measurement aid)                                                         */
#define GS_BUF_SH 8           /* rows x 3 (D+1)^2 f32  the SH store, tight rows as pushed (gs_sh_count: rows and D)                   */
#define GS_BUF_STATE 9        /* rows u8     the state store (gs_state_count: rows)                                                      */
#define GS_BUF_CONTRIB 10     /* rows u64    the contribution store (gs_contrib_info: rows); whole words only                            */
GS_API int gs_download(gs_ctx *ctx, int which, void *out, size_t nbytes);

/* ---- per-splat properties: histograms and selection by value over the resident cloud (no reference counterpart; part of "editing
 * the resident cloud" above) -----------------------------------------------------------------------------------------------------
 * A property is a function of a splat's packed record (cs[4], cc[4], as GS_BUF_CENTER_SCALE and GS_BUF_COV_COLOR return them) to an
 * f64; every operation is f64 and un-fused, and the kernels and gs_prop_eval call ONE function:
 *   GS_PROP_X, _Y, _Z    (double)cs[0], (double)cs[1], -(double)cs[2]: the rows' object space, as gs_select_sphere reads it
 *   GS_PROP_RED ... _ALPHA   bytes 0..3 of cc[3] as a double, 0..255
 *   GS_PROP_SIZE2        the trace of the dequantised covariance in object units^2 -- the sum of the three squared axis lengths, the same
 *                        under every rotation: ((double)q11 + (double)q22 + (double)q33) * (double)cs[3] with q11 = (int16)(cc[0] & 0xFFFF),
 *                        q22 = (int16)(cc[1] >> 16), q33 = (int16)(cc[2] >> 16).  No square root anywhere: a caller who thinks in radii
 *                        squares the bounds.
 * Any other id: GS_E_BADARG.
 * A splat PASSES THE FILTER (state_mask, state_value) iff (state & state_mask) == state_value, where a splat beyond the store's length
 * has state 0: (0, 0) is every splat, (GS_STATE_HIDDEN, 0) what is drawn, (3, GS_STATE_SELECTED) the visible selection.
 * gs_prop_range and gs_histogram only read: one streaming kernel each on a stream of their own, no drain, no order dropped, no option
 * or statistic changed -- a frame drawn after one is the frame drawn without it.  gs_select_range is a region call like gs_select_sphere
 * (it drains, drops the lanes' orders and counts the hidden splats again).  All three: a context fed with gs_push_matrices only is
 * GS_E_STATE; with nothing resident the counts are zero, the range is empty, the hit count is 0 and the result is GS_OK. */
#define GS_PROP_X 0
#define GS_PROP_Y 1
#define GS_PROP_Z 2
#define GS_PROP_RED 3
#define GS_PROP_GREEN 4
#define GS_PROP_BLUE 5
#define GS_PROP_ALPHA 6
#define GS_PROP_SIZE2 7
#define GS_HIST_MAX_BINS 4096
/* one record's property on the host, by the kernels' own function (no context, no GPU).  NULL pointers, an unknown prop: GS_E_BADARG. */
GS_API int gs_prop_eval(const float cs[4], const uint32_t cc[4], int prop, double *out);
/* The binning rule (no context, no GPU): scale = (double)nbins / (hi - lo); *out_bin = min((int64)floor((v - lo) * scale), nbins - 1),
 * so v == hi lands in the last bin; -1 for v < lo, -2 for v > hi, -3 for a NaN v.  Valid: lo < hi, both finite, 1 <= nbins <=
 * GS_HIST_MAX_BINS; anything else, or out_bin NULL: GS_E_BADARG.  The kernel is handed lo, hi and this scale and evaluates exactly this. */
GS_API int gs_hist_bin(double v, double lo, double hi, uint32_t nbins, int32_t *out_bin);
/* minimum and maximum of the non-NaN values among the splats that pass (+-inf take part; none: *out_min = +inf, *out_max = -inf) and
 * *out_n = the splats that pass, NaN ones included.  Each output is optional, but not all three: GS_E_BADARG. */
GS_API int gs_prop_range(gs_ctx *ctx, int prop, uint8_t state_mask, uint8_t state_value, double *out_min, double *out_max, size_t *out_n);
/* counts[b] (nbins words, required) = the passing splats whose gs_hist_bin(v, lo, hi, nbins) is b; tally (optional) = { passing, below lo,
 * above hi, NaN }: sum(counts) + below + above + NaN == passing.  Arguments as gs_hist_bin. */
GS_API int gs_histogram(gs_ctx *ctx, int prop, double lo, double hi, uint32_t nbins, uint8_t state_mask, uint8_t state_value, uint32_t *counts,
                        uint64_t tally[4]);
/* state = (state & ~clear_bits) | set_bits for every splat with lo <= v && v <= hi (a NaN v is outside); GS_SELECT_INVERT and *out_hit as
 * in gs_select_sphere.  lo == hi is allowed, lo > hi selects nothing (with INVERT: everything); a NaN bound: GS_E_BADARG. */
GS_API int gs_select_range(gs_ctx *ctx, int prop, double lo, double hi, uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit);
/* gs_select_range on every device (the hit count of devices[0]); the two reading calls on devices[0] only: every device holds the same splats */
GS_API int gs_multi_select_range(gs_multi *m, int prop, double lo, double hi, uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit);
GS_API int gs_multi_prop_range(gs_multi *m, int prop, uint8_t state_mask, uint8_t state_value, double *out_min, double *out_max, size_t *out_n);
GS_API int gs_multi_histogram(gs_multi *m, int prop, double lo, double hi, uint32_t nbins, uint8_t state_mask, uint8_t state_value, uint32_t *counts,
                              uint64_t tally[4]);

/* ---- per-splat contribution: what a splat adds to the pictures (no reference counterpart; part of "editing the resident cloud") ------
 * The contribution store holds one uint64_t per splat, parallel to the splats like the SH rows and the states and owned by the context:
 * the sum, over the contribution frames drawn so far, of the blend weights of the splat's fragments.  Splats beyond the store's length
 * have contribution 0; gs_clear and gs_contrib_clear empty it; a context that never calls gs_render_contrib allocates nothing and
 * launches exactly the kernels it launches without this section.  (Device memory: 16 bytes per splat of capacity -- the store and the
 * copy of it a frame takes, on its own stream, so that a frame the library has to draw again counts once.)
 * gs_render_contrib draws a frame as gs_render_surface does -- synchronous (GS_RENDER_ASYNC is cleared), always on the tile lists (the
 * row walk, sub-tile lists, the split blend and paired launches are off for that frame only; the options stay as set), either binning,
 * one round or two, the scene's depth and colour honoured -- and its colour is bit-identical to gs_render's on the lists with the same
 * GS_OPT_NEAR_PERMILLE.  rgba_out / device_rgba may be NULL.  The store first grows, zero-filled, to gs_count().
 * GS_RENDER_COUNT_FRAGS: GS_E_BADARG; GS_RENDER_NO_EARLY_OUT is allowed; a matrices-only context: GS_E_STATE; with no completed order
 * the frame is the background and adds nothing.  A contribution frame is a collected frame like any other: what the adaptive options
 * go by afterwards (the measured share, GS_OPT_SUBTILE / GS_OPT_ROW_WALK = 1) is what gs_render of the same frame would have left; with
 * those options pinned, a later plain frame and its gs_stats are what they are without the call.
 * WHAT IS ADDED: store[sorted[j]] receives every fragment the blend really applies -- it passes the discard test (q <= 4), the LEQUAL
 * test where a scene depth is set, and is evaluated before its lane (4 pixels of one row) has left the list: early termination is
 * honoured, and a pixel below the threshold whose lane is still live still counts, exactly as the colour accumulators received it --
 * and that belongs to a pixel of the strip [x0, x1) itself.  Per fragment, with e = exp(-q) * T_before (the factor its colour is
 * multiplied by) and alpha the record's opacity:  w = alpha * e (one f32 multiplication),  wq = (uint32_t)(w * 65536.0f + 0.5f).
 * Integer sums do not depend on the order of the additions: frames whose transmittance chains are bit-identical leave identical stores
 * (one round or two, span lists or pair records, a frame or its strips with x0 % 4 == 0 added up, a run repeated).  Hidden and culled
 * splats receive nothing.  Frames gathered from several ranks or devices (gs_comm, gs_multi) and gs_render_stereo never accumulate.
 * The store survives sorts, pushes (new splats start at 0), state and option changes; gs_compact carries it along in stable order for
 * the kept splats among those that have a word.
 * GS_PROP_SEEN is the store as a property for gs_prop_range, gs_histogram, gs_select_range and their gs_multi_ forms (each device's
 * own store): (double)store[i] / 65536.0, in pixels, exact below 2^53, 0 beyond the store.  It is no function of the record:
 * gs_prop_eval refuses it, and ids 8..15 stay unknown. */
GS_API int gs_render_contrib(gs_ctx *ctx, const gs_render_params *p, uint8_t *rgba_out, size_t stride);   /* rgba_out may be NULL */
/* device_rgba needs 4-byte alignment; 16-byte-aligned strips whose width is a multiple of 4 are stored four pixels at a time. */
GS_API int gs_render_contrib_device(gs_ctx *ctx, const gs_render_params *p, void *device_rgba);           /* may be NULL */
GS_API int gs_contrib_clear(gs_ctx *ctx);                                 /* store -> length 0, frames -> 0 */
/* rows: the store's length; frames: contribution frames that drew since the store was last emptied.  Either may be NULL. */
GS_API int gs_contrib_info(const gs_ctx *ctx, size_t *rows, uint64_t *frames);
#define GS_PROP_SEEN 16

/* ---- export: the resident cloud back to the host as .splat rows and as a .ply (no reference counterpart: the reference's README
 * describes scan -> .ply -> .splat, and processPlyBuffer / gs_ply_to_splat is that converter; nothing there leaves a page again.  Part of
 * "editing the resident cloud": what remains after hiding, selecting and gs_compact is saved with these calls) ------------------------
 * gs_download returns the packed records only; pushDataBuffer (index.js:343-402) has folded scale and rotation into six int16 covariance
 * entries times cs[3] and kept neither.  THE RULE that makes a 32-byte row of a record (cs[4], cc[4]) again -- one function,
 * csrc/gs_export.h: gsm::export_row, called by the kernel and by gs_export_row -- is, every operation IEEE f64, un-fused, built from
 * + - * / sqrt and comparisons only, in this order:
 *   position   f32 (cs[0], cs[1], -cs[2]): the exact inverse of index.js:350-354.   colour   cc[3], unchanged.
 *   matrix     s = (double)cs[3]; with q(h) the int16 in a 16-bit half:  a00 = q(cc[0] lo) * s, a01 = q(cc[0] hi) * s, a02 = q(cc[1] lo) * s,
 *              a11 = q(cc[1] hi) * s, a12 = q(cc[2] lo) * s, a22 = q(cc[2] hi) * s -- the covariance in the packed (z-mirrored) space,
 *              R^T diag(scale^2) R for the matrix R pack builds from the quaternion bytes.   V = identity (v[row][column]).
 *   Jacobi     8 sweeps, each the pairs (p, q) = (0, 1), (0, 2), (1, 2) in that order, r the third index.  A pair whose apq is exactly 0 is
 *              skipped; else  theta = (aqq - app) / (apq + apq);  root = sqrt(theta * theta + 1);
 *              t = theta >= 0 ? 1 / (theta + root) : -1 / (root - theta);  c = 1 / sqrt(t * t + 1);  s = t * c;  h = t * apq;
 *              app -= h;  aqq += h;  apq = 0;  (arp, arq) = (c * arp - s * arq, s * arp + c * arq)  from the old pair;  and for each row i
 *              of V  (vip, viq) = (c * vip - s * viq, s * vip + c * viq).
 *   scales     l_k = akk > 0 ? akk : 0;  ordered descending together with V's columns by three exchanges of neighbours on strict
 *              comparisons -- if l0 < l1 swap (0, 1); if l1 < l2 swap (1, 2); if l0 < l1 swap (0, 1) -- so ties keep the Jacobi order;
 *              det = (v00 * (v11 * v22 - v12 * v21) - v01 * (v10 * v22 - v12 * v20)) + v02 * (v10 * v21 - v11 * v20); det < 0: column 2 of V
 *              is negated.  scale_k = (float)sqrt(l_k).
 *   quaternion r[k][i] = v[i][k] (row k of R is eigenvector k), three.js' makeRotationFromQuaternion convention;  tr = (r00 + r11) + r22;
 *              the first of tr, r00, r11, r22 that is >= the ones after it and (for tr) >= all three diagonals picks the branch:
 *                tr:   S = sqrt(tr + 1) * 2;                  w = S / 4;           x = (r21 - r12) / S;  y = (r02 - r20) / S;  z = (r10 - r01) / S
 *                r00:  S = sqrt(((1 + r00) - r11) - r22) * 2;  w = (r21 - r12) / S;  x = S / 4;            y = (r01 + r10) / S;  z = (r02 + r20) / S
 *                r11:  S = sqrt(((1 + r11) - r00) - r22) * 2;  w = (r02 - r20) / S;  x = (r01 + r10) / S;  y = S / 4;            z = (r12 + r21) / S
 *                r22:  S = sqrt(((1 + r22) - r00) - r11) * 2;  w = (r10 - r01) / S;  x = (r02 + r20) / S;  y = (r12 + r21) / S;  z = S / 4
 *              all four negated if w < 0, or w == 0 and the first non-zero of x, y, z is negative.  Stored: (w, x, y, -z), index.js:344-349;
 *              byte = clamped_u8(v * 128 + 128): clamp to [0, 255], round to nearest, ties to even (Uint8ClampedArray, index.js:704-707).
 *   wide       (optional) the three scales and the stored quaternion (w, x, y, -z) as f32, before the byte rounding: what a .ply keeps.
 *   degenerate cs[3] not finite (decided on its bits): the three scales are cs[3], the quaternion (1, 0, 0, 0) -> bytes (255, 128, 128, 128).
 *              cs[3] == +-0, or all six entries 0: scales 0 and the same quaternion.  No NaN reaches a comparison.
 * Re-packing an exported row gives back cs[0..2], cc[3] and the sort row's position exactly; the covariance comes back within what the
 * format itself loses (8-bit quaternion bytes, int16 entries): docs/LAB_NOTES.md 9n.
 * gs_export_splat, gs_export_sh and gs_export_ply ONLY READ, like gs_prop_range and gs_histogram: three kernels of their own (count,
 * offsets, scatter: gs_compact's scheme with the filter (state & state_mask) == state_value as the predicate, a splat beyond the store
 * has state 0) on the same stream of their own, no drain, no order dropped, no option or statistic changed -- a frame drawn after an
 * export is the frame drawn without it, and a context that never exports launches exactly the kernels it launched before (the export
 * kernels are launched by these calls alone; gs_compact and every frame path are untouched).  The rows are staged in device memory for
 * the call (32 + 28 + 4 bytes per exported splat) and released before it returns.
 * Matrices-only context: GS_E_STATE.  Nothing resident or nothing passing: 0 rows, GS_OK. */
/* host, no GPU: one record by the rule above; row32: 32 bytes; wide may be NULL.  NULL cs, cc or row32: GS_E_BADARG. */
GS_API int gs_export_row(const float cs[4], const uint32_t cc[4], void *row32, float wide[7]);
/* The passing splats in ascending old index: out_rows[k] (32 bytes each), out_wide[k] (7 f32, optional), out_index[k] = the old index of
 * row k (optional); *out_nrows = their number (required: NULL is GS_E_BADARG).  out_rows == NULL: size query (counts only; at most
 * gs_count() rows).  With (GS_STATE_HIDDEN, 0) the rows and the index map are those gs_compact followed by a (0, 0) export gives. */
GS_API int gs_export_splat(gs_ctx *ctx, uint8_t state_mask, uint8_t state_value, void *out_rows, float *out_wide, uint32_t *out_index, size_t *out_nrows);
/* The SH rows (tight, 3 (D+1)^2 f32, D = the store's degree -> *out_degree, optional) of the exported splats that have one: the SH store is
 * a prefix of the splats and the order is stable, so they belong to the FIRST *out_nrows exported rows (gs_compact treats them the same
 * way).  out_sh == NULL: size query.  An empty store: 0 rows, degree 0. */
GS_API int gs_export_sh(gs_ctx *ctx, uint8_t state_mask, uint8_t state_value, float *out_sh, size_t *out_nrows, int *out_degree);
/* host, no context: rows (+ optional wide parts, + optional SH rows of `degree` 0..3 for the first sh_rows <= nrows of them, tight) -> a
 * binary little-endian INRIA .ply of f32 properties  x y z nx ny nz f_dc_0..2 [f_rest_0 .. 3 ((degree+1)^2 - 1) - 1] opacity scale_0..2
 * rot_0..3  that gs_ply_to_splat / gs_load_ply / gs_ply_sh read back:
 *   nx ny nz  0.   scale_k = (float)log((double)scale_k).   rot = the wide quaternion, or (byte - 128) / 128 when wide is NULL.
 *   f_dc_c    the stored sh[c][0] where the splat has an SH row, else (float)((byte / 255 - 0.5) / SH_C0): the byte comes back exactly.
 *   f_rest    channel-major (f_rest_(c * per + k - 1) = sh[c][k], per = (degree+1)^2 - 1); zeros for the splats without an SH row.
 *   opacity   (float)log(a / (255 - a)), a = the alpha byte kept inside [0.25, 254.75]: every byte 0..255 comes back exactly.
 * *out_nbytes = the file's length (required).  out_bytes == NULL: size query (rows may be NULL then).  nrows = 0: the header alone, with
 * `element vertex 0`.  A degree outside 0..3, sh_rows > nrows, sh_rows > 0 with sh NULL, nrows > 0 with rows NULL: GS_E_BADARG. */
GS_API int gs_splat_to_ply(const void *rows, const float *wide, const float *sh, size_t sh_rows, int degree, size_t nrows, void *out_bytes, size_t *out_nbytes);
/* gs_export_splat (with the wide parts) + gs_export_sh + gs_splat_to_ply: the file carries min(sh_degree, the store's degree) bands, the
 * leading ones of every stored channel.  out_bytes == NULL: size query.  sh_degree outside 0..3, NULL out_nbytes: GS_E_BADARG. */
GS_API int gs_export_ply(gs_ctx *ctx, uint8_t state_mask, uint8_t state_value, int sh_degree, void *out_bytes, size_t *out_nbytes);
/* on devices[0]: every device holds the same splats and states */
GS_API int gs_multi_export_splat(gs_multi *m, uint8_t state_mask, uint8_t state_value, void *out_rows, float *out_wide, uint32_t *out_index, size_t *out_nrows);
GS_API int gs_multi_export_ply(gs_multi *m, uint8_t state_mask, uint8_t state_value, int sh_degree, void *out_bytes, size_t *out_nbytes);

/* ---- Compressed .ply: the chunked 16-byte splat format (16 bytes per splat + one bounds record per 256 splats + optional SH bytes).
 * The rules below are restated from memory of the published format (PlayCanvas / SuperSplat).  No file written by those tools was at
 * hand: INTEROPERABILITY WITH THEIR FILES IS SUPPOSED, NOT VERIFIED (docs/LAB_NOTES.md 9s).  What is verified: the host and the GPU
 * forms below agree byte for byte, and a written file reads back within the format's own quantisation.
 *
 * Header   ASCII, lines end in \n: "ply", "format binary_little_endian 1.0", then EXACTLY these elements in this order (`comment` lines
 *          are allowed anywhere before end_header):
 *            element chunk C     12 or 18 `property float`: min_x min_y min_z max_x max_y max_z, min_scale_x min_scale_y min_scale_z
 *                                max_scale_x max_scale_y max_scale_z and, in the 18 form, min_r min_g min_b max_r max_g max_b
 *            element vertex N    `property uint` packed_position, packed_rotation, packed_scale, packed_color
 *            element sh N        (optional) `property uchar` f_rest_0 .. f_rest_(3 * per - 1), per = 3, 8 or 15 (degree 1, 2, 3), channel-major
 *                                as in INRIA files: f_rest_(c * per + k - 1) = sh[c][k]
 *          C must be ceil(N / 256).  Any other name, type, order or count, a wrong C, an sh count != N: GS_E_PLY_HEADER with a message
 *          (a valid INRIA .ply is therefore GS_E_PLY_HEADER here: that is the sniff).  A body shorter than promised: GS_E_PLY_DATA.
 * Decode   (gsm::cply_decode, csrc/gs_cply.h: ONE function, called by the kernel and by the host evaluator; IEEE f64, un-fused, in this
 *          order.)  Splat i uses chunk i >> 8.  u(v, b) = (double)(v & (2^b - 1)) / (2^b - 1).  The chunk's floats are widened first.
 *            position  t = (u(p >> 21, 11), u(p >> 11, 10), u(p, 11)): 11 + 10 + 11 bits tile the word;  x = (float)(min_x + (max_x - min_x) * t_x), likewise y, z
 *            scale     the same split of packed_scale against min_scale / max_scale gives the log scale l;  scale = (float)js_exp(l)
 *                      (csrc/gs_ply.h: Math.exp as the .ply converter evaluates it)
 *            rotation  w = packed_rotation, k = w >> 30;  a = (u(w >> 20, 10) - 0.5) * sqrt(2), b from w >> 10, c from w;
 *                      m = sqrt(max(0, 1 - ((a * a + b * b) + c * c)));  the quaternion (rot_0 .. rot_3) = (w, x, y, z) as a .ply stores it
 *                      has m at index k and a, b, c at the other three indices in ascending order.  Bytes as the .ply converter makes
 *                      them: q / sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3), then clamped_u8(q * 128 + 128).  Wide part (optional,
 *                      7 f32 per row: the three scales, then the quaternion): the normalised quaternion before the byte rounding.
 *            colour    t = (u(c >> 24, 8), u(c >> 16, 8), u(c >> 8, 8)), alpha u(c, 8);  18-float chunks: v_c = min_c + (max_c - min_c) * t_c,
 *                      12-float chunks: v_c = t_c;  byte = clamped_u8(v_c * 255), alpha byte = clamped_u8(alpha * 255)
 *            SH row    (files with `element sh`)  sh[c][0] = (float)((v_c - 0.5) / SH_C0),  sh[c][k] = (float)(byte * (8.0 / 255.0) - 4.0), k >= 1
 * Encode   (gsm::cply_encode + the bounds rule; the inputs of gs_splat_to_ply.)  Where wide is NULL the scales come from the row and the
 *          quaternion from (byte - 128) / 128.
 *            code(t, b)  t is NaN or t <= 0 ? 0 : min(2^b - 1, (uint32)floor(t * (2^b - 1) + 0.5));  against bounds (lo, hi):
 *                        t = hi > lo ? (v - lo) / (hi - lo) : 0
 *            values      position: the row's f32;  log scale: (float)clamp(log_fixed((double)scale), -20, 20), -20 for a scale <= 0 or NaN;
 *                        colour: (float)(0.5 + SH_C0 * sh[c][0]) where the splat has an SH row, else (float)(byte / 255.0);  alpha code: the byte
 *            log_fixed   x = m * 2^e, m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), z = s * s,
 *                        log = e * ln2 + 2 * (s + s * (z * (1/3 + z * (1/5 + ... + z * (1/21))))): + - * / and the exponent field only, so the
 *                        host's and the device's bits are the same.  Denormals are scaled by 2^54 first.  0: -inf; negative, NaN: NaN.
 *            bounds      per chunk and per value the smallest and the largest, as f32, over the chunk's splats whose value is finite (-0
 *                        orders below +0); the last chunk is partial: real splats only.  No finite value: lo = hi = 0.  Always 18 floats.
 *            rotation    normalise; a zero or non-finite quaternion becomes (1, 0, 0, 0);  k = the first index of the largest |q_i|;  all four
 *                        negated if q_k < 0;  the three others are code(q_i / sqrt(2) + 0.5, 10)
 *            SH          byte = clamped_u8((v + 4) * (255.0 / 8.0));  splats without an SH row take zeros (byte 128)
 *            order       GS_CPLY_MORTON: rows in ascending 30-bit Morton code, STABLE (ties keep ascending input index); else input order.
 *                        (lo, hi) per axis = the smallest and largest finite position over all rows;  i_axis = t is NaN or t < 0 ? 0 :
 *                        min(1023, (uint32)floor(t * 1024));  code = spread(ix) | spread(iy) << 1 | spread(iz) << 2.  The resident
 *                        cloud is in importance order, which is spatially incoherent: without the flag every chunk's box is the scene's.
 * The GPU forms: gs_load_cply and gs_cply_to_splat_gpu decode with one kernel (k_cply_decode) on lane 0's stream after draining the lanes,
 * like gs_load_ply.  gs_export_cply ONLY READS, like gs_export_ply: the passing splats are staged by the export scheme, then ordered
 * (k_cply_bounds_pos, k_cply_keys, four stable radix passes with scratch of the call's own) and encoded (k_cply_encode: one workgroup per
 * chunk) on the reading calls' stream: no drain, no order dropped, no option or statistic changed.  A context that never calls them
 * launches exactly the kernels it launched before. */
#define GS_CPLY_MORTON 1u
/* host, no context: what the header says.  Every out pointer is optional.  GS_E_PLY_DATA still reports the header's figures. */
GS_API int gs_cply_info(const void *bytes, size_t nbytes, size_t *out_nsplats, size_t *out_nchunks, int *out_sh_degree, int *out_chunk_floats, char *err, size_t errlen);
/* host: the file's rows in file order (32 bytes each) and, optionally, their wide parts (7 f32 each).  out_rows == NULL: size query. */
GS_API int gs_cply_to_splat(const void *bytes, size_t nbytes, void *out_rows, float *out_wide, size_t *out_nrows, char *err, size_t errlen);
/* host: the SH rows (tight, 3 (D+1)^2 f32, D = min(degree, the file's) -> *out_degree) in file order; a file without `element sh` has
 * degree 0: the DC terms alone.  out_sh == NULL: size query. */
GS_API int gs_cply_sh_host(const void *bytes, size_t nbytes, int degree, float *out_sh, size_t *out_nrows, int *out_degree, char *err, size_t errlen);
/* host: gs_splat_to_ply's inputs -> a compressed file.  flags: 0 or GS_CPLY_MORTON.  out_index (optional): the input row of output row j.
 * out_bytes == NULL: size query.  Unknown flags and gs_splat_to_ply's bad arguments: GS_E_BADARG. */
GS_API int gs_splat_to_cply(const void *rows, const float *wide, const float *sh, size_t sh_rows, int degree, size_t nrows, uint32_t flags, uint32_t *out_index,
                            void *out_bytes, size_t *out_nbytes);
/* host: gsm::log_fixed, the logarithm the encoder takes of a scale */
GS_API int gs_log_fixed(double x, double *out);
/* Decode on the GPU and append the rows IN FILE ORDER (no importance sort) straight from HBM through the pack kernel.  With GS_OPT_SH_DEGREE
 * at 1..3 the file's SH rows (min(option, file) bands) are appended under gs_load_ply's rule: only while the store is parallel to the
 * splats and the degrees agree. */
GS_API int gs_load_cply(gs_ctx *ctx, const void *bytes, size_t nbytes);
/* gs_cply_to_splat by the kernel; out_wide optional; out_rows == NULL: size query (header checks only). */
GS_API int gs_cply_to_splat_gpu(gs_ctx *ctx, const void *bytes, size_t nbytes, void *out_rows, float *out_wide, size_t *out_nrows);
/* The bytes gs_splat_to_cply makes of gs_export_splat (with the wide parts) + gs_export_sh of the same filter, the SH rows cut to
 * min(sh_degree, the store's degree) bands -- encoded on the device.  out_index (optional): the resident index of output row j.
 * out_bytes == NULL: size query. */
GS_API int gs_export_cply(gs_ctx *ctx, uint8_t state_mask, uint8_t state_value, int sh_degree, uint32_t flags, uint32_t *out_index, void *out_bytes, size_t *out_nbytes);
GS_API int gs_multi_load_cply(gs_multi *m, const void *bytes, size_t nbytes);
/* on devices[0]: every device holds the same splats and states */
GS_API int gs_multi_export_cply(gs_multi *m, uint8_t state_mask, uint8_t state_value, int sh_degree, uint32_t flags, uint32_t *out_index, void *out_bytes, size_t *out_nbytes);

#ifdef __cplusplus
}
#endif
#endif /* GS_SPLAT_H */

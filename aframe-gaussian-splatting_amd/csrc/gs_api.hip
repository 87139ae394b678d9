// gs_api.hip -- the C ABI (include/gs_splat.h) outside the frame: context lifetime, HBM residency, ingest, scene inputs, options,
// stats and downloads.  (A frame's sort, render and sync: gs_frame.hip; the lanes they run on: gs_lanes.hip; editing: gs_edit.hip.)
// No compute happens on the host here; every hot-path stage is a HIP kernel and the library refuses to exist without a device
// (no CPU fallback).
#include <stddef.h>
#include <stdlib.h>
#include "gs_lanes.h"
#include "gs_ply.h"
#include "gs_sh.h"
#include "gs_host_tables.h"

static thread_local char g_create_err[512] = "";
thread_local char *gs_tl_err = nullptr;

extern "C" {

GS_API uint32_t gs_version(void) { return 0x000500; }

GS_API int gs_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

GS_API const char *gs_last_error(const gs_ctx *ctx) { return ctx ? ctx->err : g_create_err; }

GS_API int gs_create(int device, gs_ctx **out)
{
    if (!out) return GS_E_BADARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        snprintf(g_create_err, sizeof g_create_err, "no HIP device available (%s); this library has no CPU fallback",
                 e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return GS_E_NODEVICE;
    }
    if (device < 0 || device >= ndev) {
        snprintf(g_create_err, sizeof g_create_err, "device %d out of range (have %d)", device, ndev);
        return GS_E_BADARG;
    }
    gs_ctx *ctx = new (std::nothrow) gs_ctx();
    if (!ctx) { snprintf(g_create_err, sizeof g_create_err, "out of host memory"); return GS_E_OOM; }
    memset(ctx, 0, sizeof *ctx);
    ctx->device = device; ctx->renderable = true; ctx->t_eps = 1.0f / 1024.0f; gs_share_reset_create(ctx->share);
    ctx->lanes[0] = ctx; ctx->pipe_depth = 3; ctx->enqueue_threads = true; ctx->frame_batch = 1; ctx->exec = ctx; ctx->sort_near_opt = 1; ctx->auto_retry = true; ctx->subtile_opt = 1; ctx->row_walk_opt = 1; ctx->seg_count_opt = 1;
    { const char *e = getenv("GS_SPEC_STASH"); ctx->near_spec_opt = !(e && e[0] == '0'); }   // (A/B: near-only sorts without the speculative stash)
#define CREATE_HIP(call) do { hipError_t _e = (call); if (_e != hipSuccess) {                                              \
        snprintf(g_create_err, sizeof g_create_err, "%s failed: %s", #call, hipGetErrorString(_e)); gs_destroy(ctx);      \
        return GS_E_HIP; } } while (0)
    CREATE_HIP(hipSetDevice(device));
    CREATE_HIP(init_frame_resources(ctx));
    {
        double tab[GS_POW10_ENTRIES];                           // a few KB: on the stack
        gs_build_pow10_table(tab);
        CREATE_HIP(hipMalloc((void **)&ctx->pow10tab, sizeof tab));
        CREATE_HIP(hipMemcpy(ctx->pow10tab, tab, sizeof tab, hipMemcpyHostToDevice));
    }
#undef CREATE_HIP
    *out = ctx;
    return GS_OK;
}

GS_API int gs_destroy(gs_ctx *ctx)
{
    if (!ctx) return GS_OK;
    (void)hipSetDevice(ctx->device);
    (void)gs_comm_destroy(ctx);
    for (int i = GS_MAX_LANES - 1; i >= 1; i--)                  // twins before the lanes whose streams they borrow
        if (ctx->lanes[i]) { free_frame_resources(ctx->lanes[i]); delete ctx->lanes[i]; ctx->lanes[i] = nullptr; }
    free_frame_resources(ctx);
    dev_free(ctx->splat); dev_free(ctx->sort_rows); dev_free(ctx->bound_r); dev_free(ctx->pow10tab); dev_free(ctx->sh);
    dev_free(ctx->edit_state); dev_free(ctx->edit_cnt); dev_free(ctx->mask_buf);
    dev_free(ctx->scene_depth); dev_free(ctx->scene_rgba);
    dev_free(ctx->prop_buf); dev_free(ctx->contrib);
    if (ctx->prop_stream) (void)hipStreamDestroy(ctx->prop_stream);
    if (ctx->ev_sort) (void)hipEventDestroy(ctx->ev_sort);
    delete ctx;
    return GS_OK;
}

GS_API int gs_clear(gs_ctx *ctx)
{
    CHECK_CTX(ctx);
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    if (ctx->edit_state && ctx->edit_n) GS_HIP(hipMemset(ctx->edit_state, 0, ctx->edit_n));   // (the allocation stays, all zero: a store grows zero-filled)
    ctx->edit_n = 0; ctx->edit_hidden = 0;
    TRY(gs_contrib_clear(ctx));                                  // (the contribution store empties with the cloud)
    ctx->n = 0; ctx->sh_n = 0; ctx->sh_deg = 0; ctx->renderable = true;
    reset_cloud_measurements(ctx);
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (!L) continue;
        L->have_sort = false; L->sorted = nullptr; L->n = 0;
        memset(&L->stats, 0, sizeof L->stats);
    }
    set_current_lane(ctx, 0, 0); ctx->pend_lane = 0;   // (a sort begun before the clear is dropped, like the worker's data: index.js:573-575)
    return GS_OK;
}

GS_API size_t gs_count(const gs_ctx *ctx) { return ctx ? ctx->n : 0; }

// pack `nrows` .splat rows that already sit in device memory behind the resident splats (capacity ensured by the caller)
static int append_device_rows(gs_ctx *ctx, const uint4 *rows_dev, size_t nrows)
{
    int rc = gs_launch_pack(ctx, rows_dev, ctx->n, nrows);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc == GS_OK && e != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "pack failed: %s", hipGetErrorString(e)); rc = GS_E_HIP; }
    if (rc != GS_OK) return rc;
    ctx->n += nrows; ctx->renderable = true;
    for (int i = 0; i < GS_MAX_LANES; i++) if (ctx->lanes[i]) ctx->lanes[i]->have_sort = false;
    ctx->stats.n_splats = ctx->n;
    return GS_OK;
}

GS_API int gs_push_splat(gs_ctx *ctx, const void *rows, size_t nrows)
{
    CHECK_CTX(ctx);
    if (nrows == 0) return GS_OK;                               // pushDataBuffer: vertexCount <= 0 -> return (index.js:333-335)
    if (!rows) FAIL(GS_E_BADARG, "gs_push_splat: rows is NULL");
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "gs_push_splat after gs_push_matrices: mixed ingest is not supported");
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    TRY(ensure_capacity(ctx, ctx->n + nrows));
    uint4 *stage = nullptr;
    TRY(dev_alloc(ctx, &stage, nrows * 2));
    hipError_t e = hipMemcpyAsync(stage, rows, nrows * 32, hipMemcpyHostToDevice, ctx->stream);
    int rc = GS_OK;
    if (e != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "upload failed: %s", hipGetErrorString(e)); rc = GS_E_HIP; }
    if (rc == GS_OK) rc = append_device_rows(ctx, stage, nrows);
    else (void)hipStreamSynchronize(ctx->stream);
    dev_free(stage);
    return rc;
}

GS_API int gs_push_matrices(gs_ctx *ctx, const float *matrices, size_t nrows)
{
    CHECK_CTX(ctx);
    if (nrows == 0) return GS_OK;
    if (!matrices) FAIL(GS_E_BADARG, "gs_push_matrices: matrices is NULL");
    if (ctx->renderable && ctx->n) FAIL(GS_E_STATE, "gs_push_matrices after gs_push_splat: mixed ingest is not supported");
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    TRY(ensure_capacity(ctx, ctx->n + nrows));
    // strided H2D copy: only elements 12..15 of every 16-float row are ever read (index.js:520-548)
    GS_HIP(hipMemcpy2DAsync(ctx->sort_rows + ctx->n, 16, matrices + 12, 64, 16, nrows, hipMemcpyHostToDevice, ctx->stream));
    GS_HIP(hipStreamSynchronize(ctx->stream));
    ctx->n += nrows; ctx->renderable = false;
    for (int i = 0; i < GS_MAX_LANES; i++) if (ctx->lanes[i]) ctx->lanes[i]->have_sort = false;
    ctx->stats.n_splats = ctx->n;
    return GS_OK;
}

// ---- view-dependent colour: the SH store (gs_sh.h).  Rows parallel to the splats, owner only; a frame gets the pointer, the row
// count and the camera through its uniforms (gs_fill_uniforms), so the lanes hold nothing.
static int sh_ensure_capacity(gs_ctx *ctx, size_t want, int degree)
{
    if (want <= ctx->sh_cap) return GS_OK;
    size_t cap = ctx->sh_cap ? ctx->sh_cap : (size_t)1 << 16;
    while (cap < want) cap *= 2;
    const size_t row = 3 * (size_t)gsm::sh_channel_stride(degree);
    float *nw = nullptr;
    TRY(dev_alloc(ctx, &nw, cap * row));
    if (ctx->sh_n) {
        const hipError_t e = hipMemcpy(nw, ctx->sh, ctx->sh_n * row * sizeof(float), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { dev_free(nw); FAIL(GS_E_HIP, "copying the SH rows failed: %s", hipGetErrorString(e)); }
    }
    dev_free(ctx->sh);
    ctx->sh = nw; ctx->sh_cap = cap;
    return GS_OK;
}

GS_API int gs_push_sh(gs_ctx *ctx, const float *sh_rows, size_t nrows, int degree)
{
    CHECK_CTX(ctx);
    if (degree < 1 || degree > GS_SH_MAX_DEGREE) FAIL(GS_E_BADARG, "gs_push_sh: degree must be 1..3");
    if (ctx->sh_n && degree != ctx->sh_deg) FAIL(GS_E_BADARG, "gs_push_sh: rows of degree %d behind stored rows of degree %d", degree, ctx->sh_deg);
    if (nrows == 0) return GS_OK;
    if (!sh_rows) FAIL(GS_E_BADARG, "gs_push_sh: sh_rows is NULL");
    if (ctx->sh_n + nrows > 0x7FFFFFF0ull) FAIL(GS_E_BADARG, "more than 2^31 SH rows");
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));                                        // frames in flight read the store
    if (!ctx->sh_n && ctx->sh_deg != degree) { dev_free(ctx->sh); ctx->sh_cap = 0; }   // (an emptied store of another row size)
    TRY(sh_ensure_capacity(ctx, ctx->sh_n + nrows, degree));
    // tight rows in, channels padded to whole 16-byte words in the store
    const int K = gsm::sh_coefs(degree), KS = gsm::sh_channel_stride(degree);
    const float *src = sh_rows;
    std::vector<float> padded;
    if (KS != K) {
        try { padded.assign(nrows * 3 * (size_t)KS, 0.0f); } catch (...) { FAIL(GS_E_OOM, "out of host memory for %zu SH rows", nrows); }
        for (size_t i = 0; i < nrows; i++)
            for (int c = 0; c < 3; c++) memcpy(&padded[(i * 3 + c) * KS], sh_rows + (i * 3 + c) * K, (size_t)K * sizeof(float));
        src = padded.data();
    }
    GS_HIP(hipMemcpy(ctx->sh + ctx->sh_n * 3 * (size_t)KS, src, nrows * 3 * (size_t)KS * sizeof(float), hipMemcpyHostToDevice));
    ctx->sh_n += nrows; ctx->sh_deg = degree;
    return GS_OK;
}

GS_API int gs_sh_count(const gs_ctx *ctx, size_t *out_nrows, int *out_degree)
{
    if (!ctx) return GS_E_BADARG;
    if (out_nrows) *out_nrows = ctx->sh_n;
    if (out_degree) *out_degree = ctx->sh_n ? ctx->sh_deg : 0;
    return GS_OK;
}

GS_API int gs_ply_sh(gs_ctx *ctx, const void *bytes, size_t nbytes, int degree, float *out_sh, size_t *out_nrows, int *out_degree)
{
    CHECK_CTX(ctx);
    return gs_ply_sh_host(bytes, nbytes, degree, out_sh, out_nrows, out_degree, ctx->err, sizeof ctx->err);
}

// gs_load_ply with GS_OPT_SH_DEGREE at 1..3: the file's SH rows behind the store, while the store is parallel to the splats
static int load_ply_sh(gs_ctx *ctx, const void *bytes, size_t nbytes, size_t n_before, size_t n_loaded)
{
    if (ctx->sh_opt < 1 || ctx->sh_n != n_before) return GS_OK;
    size_t n = 0; int D = -1;
    TRY(gs_ply_sh_host(bytes, nbytes, ctx->sh_opt, nullptr, &n, &D, ctx->err, sizeof ctx->err));
    if (D < 1 || n != n_loaded || (ctx->sh_n && D != ctx->sh_deg)) return GS_OK;
    std::vector<float> rows;
    try { rows.resize(n * 3 * (size_t)gsm::sh_coefs(D)); } catch (...) { FAIL(GS_E_OOM, "out of host memory for %zu SH rows", n); }
    TRY(gs_ply_sh_host(bytes, nbytes, ctx->sh_opt, rows.data(), &n, &D, ctx->err, sizeof ctx->err));
    return gs_push_sh(ctx, rows.data(), n, D);
}

// .ply -> .splat rows on the GPU (gs_ply.hip); rows_dev receives a device buffer of *nrows x 32 B that the caller frees.
// A NaN importance (engine-defined order in the reference) is handed to the host converter so that there is ONE
// definition of that case.
static int ply_rows_to_device(gs_ctx *ctx, const void *bytes, size_t nbytes, uint4 **rows_dev, size_t *nrows)
{
    *rows_dev = nullptr; *nrows = 0;
    gsm::PlyLayout L;
    size_t n = 0, data_start = 0;
    int rc = gs_ply_plan(bytes, nbytes, &L, &n, &data_start, ctx->err, sizeof ctx->err);
    *nrows = n;
    if (rc != GS_OK || !n) return rc;
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));                                        // the converter borrows lane 0's stream and radix scratch
    uint4 *rows = nullptr;
    TRY(dev_alloc(ctx, &rows, n * 2));
    bool had_nan = false;
    rc = gs_ply_rows_device(ctx, (const uint8_t *)bytes + data_start, L, n, rows, &had_nan);
    if (rc == GS_OK && had_nan) {
        std::vector<uint8_t> host;
        try { host.resize(n * 32); } catch (...) { dev_free(rows); FAIL(GS_E_OOM, "out of host memory for %zu rows", n); }
        rc = gs_ply_to_splat(bytes, nbytes, host.data(), &n, ctx->err, sizeof ctx->err);
        if (rc == GS_OK && hipMemcpy(rows, host.data(), n * 32, hipMemcpyHostToDevice) != hipSuccess) {
            snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "upload failed"); rc = GS_E_HIP;
        }
    }
    if (rc != GS_OK) { dev_free(rows); return rc; }
    *rows_dev = rows;
    return GS_OK;
}

GS_API int gs_load_ply(gs_ctx *ctx, const void *bytes, size_t nbytes)
{
    CHECK_CTX(ctx);
    if (!bytes) FAIL(GS_E_BADARG, "gs_load_ply: bytes is NULL");
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "gs_load_ply after gs_push_matrices: mixed ingest is not supported");
    uint4 *rows = nullptr; size_t n = 0;
    TRY(ply_rows_to_device(ctx, bytes, nbytes, &rows, &n));
    if (!n) return GS_OK;
    const size_t n_before = ctx->n;
    int rc = ensure_capacity(ctx, ctx->n + n);
    if (rc == GS_OK) rc = append_device_rows(ctx, rows, n);         // the rows never leave HBM
    dev_free(rows);
    if (rc == GS_OK) rc = load_ply_sh(ctx, bytes, nbytes, n_before, n);
    return rc;
}

GS_API int gs_ply_to_splat_gpu(gs_ctx *ctx, const void *bytes, size_t nbytes, void *out_rows, size_t *out_nrows)
{
    CHECK_CTX(ctx);
    if (!bytes || !out_nrows) FAIL(GS_E_BADARG, "gs_ply_to_splat_gpu: NULL argument");
    if (!out_rows) {                                             // size query: header + property checks only
        gsm::PlyLayout L; size_t ds = 0;
        return gs_ply_plan(bytes, nbytes, &L, out_nrows, &ds, ctx->err, sizeof ctx->err);
    }
    uint4 *rows = nullptr;
    TRY(ply_rows_to_device(ctx, bytes, nbytes, &rows, out_nrows));
    if (!*out_nrows) return GS_OK;
    const hipError_t e = hipMemcpy(out_rows, rows, *out_nrows * 32, hipMemcpyDeviceToHost);
    dev_free(rows);
    if (e != hipSuccess) FAIL(GS_E_HIP, "download failed: %s", hipGetErrorString(e));
    return GS_OK;
}

GS_API int gs_set_scene(gs_ctx *ctx, const float *depth, const uint8_t *rgba, int fb_width, int fb_height)
{
    CHECK_CTX(ctx);
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    dev_free(ctx->scene_depth); dev_free(ctx->scene_rgba);
    ctx->scene_w = ctx->scene_h = 0;
    refresh_lanes(ctx);
    if (!depth && !rgba) return GS_OK;
    if (fb_width <= 0 || fb_height <= 0) FAIL(GS_E_BADARG, "gs_set_scene: bad size %dx%d", fb_width, fb_height);
    const size_t px = (size_t)fb_width * fb_height;
    if (depth) { TRY(dev_alloc(ctx, &ctx->scene_depth, px)); GS_HIP(hipMemcpy(ctx->scene_depth, depth, px * 4, hipMemcpyHostToDevice)); }
    if (rgba) { TRY(dev_alloc(ctx, &ctx->scene_rgba, px)); GS_HIP(hipMemcpy(ctx->scene_rgba, rgba, px * 4, hipMemcpyHostToDevice)); }
    ctx->scene_w = fb_width; ctx->scene_h = fb_height;
    refresh_lanes(ctx);
    return GS_OK;
}

GS_API void *gs_host_alloc(size_t nbytes)
{
    void *p = nullptr;
    if (!nbytes || hipHostMalloc(&p, nbytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

GS_API void gs_host_free(void *p) { if (p) (void)hipHostFree(p); }

// The options that are a range, a message for a value outside it, perhaps every lane idle first, and one store.  drains: whether the
// lanes are drained (their enqueue threads or frames in flight read the field), and on which side of the range check -- a refused
// value has drained the lanes where the check comes second.
enum { OPT_NO_DRAIN, OPT_CHECK_DRAIN, OPT_DRAIN_CHECK };
struct GsOptionRow { int option; int64_t lo, hi; const char *message; int drains; void (*store)(gs_ctx *, int64_t); };
static const GsOptionRow option_rows[] = {
    { GS_OPT_RECORD_STAGED, INT64_MIN, INT64_MAX, nullptr, OPT_NO_DRAIN, [](gs_ctx *c, int64_t v) { c->record_staged = v == 2 ? 2u : (v != 0 ? 1u : 0u); } },
    { GS_OPT_WIDE_PAIRS, 0, 1, "wide records: 0 (automatic) or 1 (the depth sort's general 8-byte records whatever the number of splats)", OPT_DRAIN_CHECK, [](gs_ctx *c, int64_t v) { c->wide_pairs = v == 1; refresh_lanes(c); } },
    { GS_OPT_BINNING, 0, 1, "binning: 0 (span lists wherever the strip fits) or 1 (pair records and two stable radix passes)", OPT_DRAIN_CHECK, [](gs_ctx *c, int64_t v) { c->bin_mode = (int)v; } },
    { GS_OPT_ENQUEUE_THREADS, INT64_MIN, INT64_MAX, nullptr, OPT_CHECK_DRAIN, [](gs_ctx *c, int64_t v) { c->enqueue_threads = v != 0; } },
    { GS_OPT_BLEND_SPLIT, 0, 0x7FFFFFFF, "blend split: 0 (off) or the list length from which a tile is split", OPT_NO_DRAIN, [](gs_ctx *c, int64_t v) { c->blend_split_min = (uint32_t)v; } },
    { GS_OPT_SORT_SHARE, 0, 1000, "sort share: 0 (off) or the permille of the splats whose order the ranks exchange", OPT_CHECK_DRAIN, [](gs_ctx *c, int64_t v) { c->sort_share_permille = (int)v; } },
    { GS_OPT_AUTO_RETRY, INT64_MIN, INT64_MAX, nullptr, OPT_CHECK_DRAIN, [](gs_ctx *c, int64_t v) { c->auto_retry = v != 0; } },
    { GS_OPT_SUBTILE, 0, 2, "sub-tile lists: 0 (off), 1 (where splats are small) or 2 (always)", OPT_NO_DRAIN, [](gs_ctx *c, int64_t v) { c->subtile_opt = (int)v; } },
    { GS_OPT_ROW_WALK, 0, 2, "row walk: 0 (off), 1 (where splats are large) or 2 (always)", OPT_NO_DRAIN, [](gs_ctx *c, int64_t v) { c->row_walk_opt = (int)v; } },
    // (segment counts: the lanes' enqueue threads read it where they launch a round)
    { GS_OPT_SEG_COUNT, 0, 2, "segment counts: 0 (never), 1 (where tile rows hold many runs) or 2 (always)", OPT_CHECK_DRAIN, [](gs_ctx *c, int64_t v) { c->seg_count_opt = (int)v; } },
    { GS_OPT_SH_DEGREE, 0, GS_SH_MAX_DEGREE, "spherical-harmonics degree: 0 (off) to 3", OPT_NO_DRAIN, [](gs_ctx *c, int64_t v) { c->sh_opt = (int)v; } },
    { GS_OPT_ANTIALIAS, 0, 1, "anti-aliased splats: 0 (off) or 1 (opacity compensated for the 0.3 px^2 dilation)", OPT_NO_DRAIN, [](gs_ctx *c, int64_t v) { c->aa_opt = (int)v; } },
    { GS_OPT_HIGHLIGHT, 0, 0xFFFFFFFFll, "highlight: R | G << 8 | B << 16 | W << 24 (W = 0: off)", OPT_NO_DRAIN, [](gs_ctx *c, int64_t v) { c->hl_opt = (uint32_t)v; } },
    { GS_OPT_SORT_NEAR, 0, 2, "near-only sorts: 0 (off), 1 (scenes of 4 M splats and more) or 2 (always)", OPT_CHECK_DRAIN, [](gs_ctx *c, int64_t v) { c->sort_near_opt = (int)v; } },
    { GS_OPT_SORT_NEAR_FORCE, 0, 0xFFFFFFFFll, "forced near-only sorts: 0 (the policy decides) or the positions every sort without an index list is asked for", OPT_CHECK_DRAIN, [](gs_ctx *c, int64_t v) { c->sort_near_force = (uint32_t)v; } },
};

GS_API int gs_set_option(gs_ctx *ctx, int option, int64_t value)
{
    CHECK_CTX(ctx);
    for (const GsOptionRow &r : option_rows) {
        if (r.option != option) continue;
        const bool outside = value < r.lo || value > r.hi;
        if (outside && r.drains != OPT_DRAIN_CHECK) FAIL(GS_E_BADARG, "%s", r.message);
        if (r.drains != OPT_NO_DRAIN) { GS_HIP(hipSetDevice(ctx->device)); TRY(drain_all(ctx)); }
        if (outside) FAIL(GS_E_BADARG, "%s", r.message);
        r.store(ctx, value);
        return GS_OK;
    }
    switch (option) {                                            // the options that do more
    case GS_OPT_PROFILE:
        GS_HIP(hipSetDevice(ctx->device));
        for (int i = 0; i < GS_MAX_LANES; i++)
            if (ctx->lanes[i]) TRY(lane_rc(ctx, ctx->lanes[i], set_profile(ctx->lanes[i], value != 0, value == 2 || value == 3, value == 3 ? 4u : 1u)));
        return GS_OK;
    case GS_OPT_NEAR_PERMILLE:
        if (value < 0 || value > 1000) FAIL(GS_E_BADARG, "near permille must be 0 (adaptive) .. 1000 (single round)");
        ctx->share.near_fixed_permille = (int)value;
        if (value == 0) {
            // adapt from scratch: the default share, nothing measured -- on the device too (each lane's next frame clears its need words:
            // a word that still says "a tile no share saturates" from frames long gone would keep the share at 100 % for 64 collections)
            gs_share_reset_unpin(ctx->share); reseed_lanes(ctx);
        }
        return GS_OK;
    case GS_OPT_TERMINATION:
        if (value < 2) FAIL(GS_E_BADARG, "termination 1/eps must be >= 2");
        ctx->t_eps = 1.0f / (float)value; return GS_OK;
    case GS_OPT_COMM_SELF_COPY:
        GS_HIP(hipSetDevice(ctx->device));
        TRY(drain_all(ctx));
        return gs_comm_set_self_copy(ctx, value != 0);
    case GS_OPT_COMM_TRANSPORT:
        if (value != 0 && value != 1) FAIL(GS_E_BADARG, "comm transport: 0 (RCCL) or 1 (in-process)");
        return gs_comm_set_transport(ctx, (int)value);
    case GS_OPT_PIPELINE_DEPTH:
        if (value < 1 || value > GS_MAX_PRIMARY) FAIL(GS_E_BADARG, "pipeline depth must be 1..%d", GS_MAX_PRIMARY);
        GS_HIP(hipSetDevice(ctx->device));
        TRY(drain_all(ctx));
        ctx->pipe_depth = (int)value;
        set_current_lane(ctx, 0, 0);
        return prepare_lanes(ctx);
    case GS_OPT_FRAME_BATCH:
        if (value != 1 && value != 2) FAIL(GS_E_BADARG, "frame batch must be 1 (off) or 2");
        GS_HIP(hipSetDevice(ctx->device));
        TRY(drain_all(ctx));
        ctx->frame_batch = (int)value;
        set_current_lane(ctx, 0, 0);
        return prepare_lanes(ctx);
    default: FAIL(GS_E_BADARG, "unknown option %d", option);
    }
}

GS_API int gs_get_stats(gs_ctx *ctx, gs_stats *out)
{
    CHECK_CTX(ctx);
    if (!out) FAIL(GS_E_BADARG, "gs_get_stats: out is NULL");
    // per-frame figures: the current frame's lane; accumulators: summed over the lanes
    for (int i = 0; i < GS_MAX_LANES; i++) if (ctx->lanes[i]) (void)lane_drain(ctx->lanes[i]);
    gs_stats s = ctx->lanes[ctx->cur]->stats;
    s.prof_frames = 0; s.sum_ms_sort = s.sum_ms_project = s.sum_ms_bin = s.sum_ms_blend = 0;
    s.acc_frames = 0; s.acc_sorted = s.acc_visible = s.acc_pairs = 0;
    for (int i = 0; i < GS_MAX_LANES; i++) {
        const gs_ctx *L = ctx->lanes[i];
        if (!L) continue;
        s.prof_frames += L->stats.prof_frames;
        s.sum_ms_sort += L->stats.sum_ms_sort; s.sum_ms_project += L->stats.sum_ms_project;
        s.sum_ms_bin += L->stats.sum_ms_bin; s.sum_ms_blend += L->stats.sum_ms_blend;
        s.acc_frames += L->stats.acc_frames; s.acc_sorted += L->stats.acc_sorted;
        s.acc_visible += L->stats.acc_visible; s.acc_pairs += L->stats.acc_pairs;
    }
    s.n_splats = ctx->n;
    s.retried_frames = ctx->stats.retried_frames; s.spec_sorts = ctx->stats.spec_sorts; s.spec_misses = ctx->stats.spec_misses; s.need_splats = ctx->stats.need_splats;
    s.near_permille = (uint32_t)(ctx->share.near_frac * 1000.0f + 0.5f);
    *out = s;
    return GS_OK;
}

GS_API int gs_sort_inspect(gs_ctx *ctx, gs_sort_info *info, uint32_t *out_idx, size_t cap)
{
    CHECK_CTX(ctx);
    if (!info) FAIL(GS_E_BADARG, "gs_sort_inspect: info is NULL");
    memset(info, 0, sizeof *info);
    GS_HIP(hipSetDevice(ctx->device));
    gs_ctx *L = ctx->lanes[ctx->cur];
    TRY(lane_rc(ctx, L, lane_drain(L)));
    if (!L->have_sort || !ctx->n) FAIL(GS_E_STATE, "gs_sort_inspect: the current frame's lane holds no order");
    TRY(lane_rc(ctx, L, lane_read_control(L, true)));
    const GsControl *c = L->ctl_host;
    const bool whole = L->sort_form == 0u;
    info->form = L->sort_form; info->near_req = L->sort_near_req;
    info->n_kept = c->n_kept;
    info->n_valid = whole ? (ctx->wide_pairs || ctx->n > ((size_t)1 << 25) ? c->n_kept : c->n_sorted) : c->n_valid;
    info->n_records = whole ? c->n_kept : c->n_sorted;
    info->order_incomplete = c->order_incomplete; info->near_overflow = c->near_overflow; info->spec_fail = c->spec_fail;
    GS_HIP(hipMemcpy(&info->threshold_bin, &ctx->ctl->near_bin_hint, sizeof(uint32_t), hipMemcpyDeviceToHost));   // (the owner's block: any lane's kernels write it)
    const bool fits = !out_idx || cap >= info->n_records;
    if (fits && out_idx && info->n_records) GS_HIP(hipMemcpy(out_idx, L->sorted, (size_t)info->n_records * 4, hipMemcpyDeviceToHost));
    // the collection (the near-only sorts' bookkeeping alone).  An incomplete order: what a synchronous frame does -- flags down, a whole sort
    TRY(collect_near_sort(L, c, nullptr));
    if (c->order_incomplete) {
        GS_HIP(hipMemsetAsync(&L->ctl->order_incomplete, 0, sizeof(uint32_t), L->stream));
        GS_HIP(hipMemsetAsync(&L->ctl->round1_missed, 0, sizeof(uint32_t), L->stream));
        TRY(lane_rc(ctx, L, ensure_full_sort(L)));
        GS_HIP(hipStreamSynchronize(L->stream));
    }
    if (!fits) FAIL(GS_E_BADARG, "gs_sort_inspect: the lane holds %u entries, room for %zu", info->n_records, cap);
    return GS_OK;
}

GS_API int gs_download(gs_ctx *ctx, int which, void *out, size_t nbytes)
{
    CHECK_CTX(ctx);
    if (!out) FAIL(GS_E_BADARG, "gs_download: out is NULL");
    GS_HIP(hipSetDevice(ctx->device));
    gs_ctx *L = ctx->lanes[ctx->cur];                           // per-frame buffers: the current frame's lane
    TRY(lane_rc(ctx, L, lane_drain(L)));
    GS_HIP(hipStreamSynchronize(L->stream));
    const void *src = nullptr; size_t have = 0;
    const size_t V = L->stats.n_sorted;
    if (which == GS_BUF_CENTER_SCALE || which == GS_BUF_COV_COLOR) {     // de-interleave the 32-byte splat records
        if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "context holds worker rows only");
        if (nbytes > ctx->n * 16 || nbytes % 16) FAIL(GS_E_BADARG, "buffer %d holds %zu bytes, %zu requested", which, ctx->n * 16, nbytes);
        if (nbytes) GS_HIP(hipMemcpy2D(out, 16, (const char *)ctx->splat + (which == GS_BUF_COV_COLOR ? 16 : 0), 32, 16, nbytes / 16,
                                        hipMemcpyDeviceToHost));
        return GS_OK;
    }
    if (which == GS_BUF_STATE) {
        if (nbytes > ctx->edit_n) FAIL(GS_E_BADARG, "buffer %d holds %zu bytes, %zu requested", which, ctx->edit_n, nbytes);
        if (nbytes) GS_HIP(hipMemcpy(out, ctx->edit_state, nbytes, hipMemcpyDeviceToHost));
        return GS_OK;
    }
    if (which == GS_BUF_CONTRIB) {
        if (nbytes > ctx->contrib_n * 8 || nbytes % 8) FAIL(GS_E_BADARG, "buffer %d holds %zu bytes, %zu requested", which, ctx->contrib_n * 8, nbytes);
        if (nbytes) GS_HIP(hipMemcpy(out, ctx->contrib, nbytes, hipMemcpyDeviceToHost));
        return GS_OK;
    }
    if (which == GS_BUF_SH) {                                    // tight rows out of the padded store
        const size_t K = (size_t)gsm::sh_coefs(ctx->sh_deg), KS = (size_t)gsm::sh_channel_stride(ctx->sh_deg);
        if (nbytes > ctx->sh_n * 3 * K * 4 || nbytes % (K * 4)) FAIL(GS_E_BADARG, "buffer %d holds %zu bytes, %zu requested", which, ctx->sh_n * 3 * K * 4, nbytes);
        if (nbytes) GS_HIP(hipMemcpy2D(out, K * 4, ctx->sh, KS * 4, K * 4, nbytes / (K * 4), hipMemcpyDeviceToHost));
        return GS_OK;
    }
    switch (which) {
    case GS_BUF_SORT_ROWS: src = ctx->sort_rows; have = ctx->n * 16; break;
    case GS_BUF_SORTED:
        if (L->have_sort && L->sort_near_req) { TRY(lane_rc(ctx, L, ensure_full_sort(L))); GS_HIP(hipStreamSynchronize(L->stream)); }
        src = L->sorted; have = L->have_sort ? V * 4 : 0; break;
    case GS_BUF_PROJECTED: src = L->proj; have = L->have_sort ? V * 32 : 0; break;
    case GS_BUF_TILE_COUNT: src = L->tile_count; have = L->have_sort ? V * 4 : 0; break;
    case GS_BUF_TILE_STATS: src = L->tile_range; have = L->tile_cap * 8; break;
    case GS_BUF_UNSAT_MASK: src = L->unsat_mask; have = L->mask_cap * 4; break;
    default: FAIL(GS_E_BADARG, "unknown buffer %d", which);
    }
    if (nbytes > have) FAIL(GS_E_BADARG, "buffer %d holds %zu bytes, %zu requested", which, have, nbytes);
    if (nbytes && (!ctx->renderable && (which == GS_BUF_CENTER_SCALE || which == GS_BUF_COV_COLOR)))
        FAIL(GS_E_STATE, "context holds worker rows only");
    if (nbytes) GS_HIP(hipMemcpy(out, src, nbytes, hipMemcpyDeviceToHost));
    return GS_OK;
}

}  // extern "C"

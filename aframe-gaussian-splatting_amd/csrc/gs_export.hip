// gs_export.hip -- the resident cloud back to the host as .splat rows and as a .ply (include/gs_splat.h: gs_export_splat,
// gs_export_sh, gs_export_ply): the splats that pass a state filter, compacted in stable order, each packed record turned into a
// row again by gsm::export_row (gs_export.h: a symmetric 3x3 eigen-decomposition per splat, f64).
//
// The compaction is the one gs_compact uses (gs_cloud_pass.h: count -> offsets -> slot) with the state filter as its predicate; the two
// scatters are this file's own, and a context that never exports launches none of them.
// Like gs_prop_range and gs_histogram the calls only read the resident arrays: they run on the owner's prop_stream, wait for
// their own kernels and copies alone, drain no lane, drop no order and touch no option or statistic.
//
// Launch shape of the scatter: 256 threads, a thread's eight splats walked by a rolled loop, the sweep loop rolled too (one copy of
// the three rotations: the instruction cache).  The eigen-solver keeps the matrix (6 f64) and the vectors (9 f64) in registers, a
// rotation's temporaries die with it: the compiler reports 58 vector registers, no private memory, 8 waves per SIMD -- far below the
// spill line, so no register budget is set.  The kernel is bound by f64 divisions and square roots (two of each per rotation, 24
// rotations per splat), not by memory (32 bytes in and 32 + 28 + 4 out per splat): many waves per SIMD to hide their latency is
// what helps, and the skipped rotations (an entry that is exactly 0) only diverge within a wave.
#include "gs_lanes.h"
#include "gs_sh.h"
#include "gs_cloud_pass.h"
#include "gs_export.h"
#include "gs_export_stage.h"

namespace {

// (earlier versions of the tests read this name out of this file; the constant is gs_cloud_pass.h's GS_EDIT_IPT)
#define GS_EXPORT_IPT 8u
static_assert(GS_EXPORT_IPT == GS_EDIT_IPT, "the exports run the shared compaction: one chunk size");

// o_rows: 2 x 16 bytes per row; o_wide (may be null): 7 f32 per row; o_index (may be null): the old index
__global__ __launch_bounds__(GS_BLOCK) void k_export_scatter(StateFilter pass, uint32_t n, const uint32_t *__restrict__ blk, const uint4 *__restrict__ splat,
                                                             uint4 *__restrict__ o_rows, float *__restrict__ o_wide, uint32_t *__restrict__ o_index)
{
    uint32_t i0, take;
    uint32_t k = compact_slot(pass, n, blk, i0, take);
#pragma unroll 1
    for (uint32_t j = 0; j < GS_EDIT_IPT; j++) {
        if (!((take >> j) & 1u)) continue;
        const uint32_t i = i0 + j;
        const uint4 cs4 = splat[2 * (size_t)i], cc4 = splat[2 * (size_t)i + 1];
        const float cs[4] = { __uint_as_float(cs4.x), __uint_as_float(cs4.y), __uint_as_float(cs4.z), __uint_as_float(cs4.w) };
        const uint32_t cc[4] = { cc4.x, cc4.y, cc4.z, cc4.w };
        uint32_t w[8];
        float wide[7];
        gsm::export_row(cs, cc, w, wide);
        o_rows[2 * (size_t)k] = make_uint4(w[0], w[1], w[2], w[3]);
        o_rows[2 * (size_t)k + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        if (o_wide) {
#pragma unroll
            for (int q = 0; q < 7; q++) o_wide[7 * (size_t)k + q] = wide[q];
        }
        if (o_index) o_index[k] = i;
        k++;
    }
}
// the SH rows of the passing splats among the first n (= those that have a row): padded store rows -> padded rows, in stable order
__global__ __launch_bounds__(GS_BLOCK) void k_export_sh(StateFilter pass, uint32_t n, const uint32_t *__restrict__ blk, const uint4 *__restrict__ sh, uint32_t row_q,
                                                        uint4 *__restrict__ o_sh)
{
    uint32_t i0, take;
    uint32_t k = compact_slot(pass, n, blk, i0, take);
#pragma unroll 1
    for (uint32_t j = 0; j < GS_EDIT_IPT; j++) {
        if (!((take >> j) & 1u)) continue;
        for (uint32_t q = 0; q < row_q; q++) o_sh[(size_t)k * row_q + q] = sh[(size_t)(i0 + j) * row_q + q];
        k++;
    }
}

// everything a call holds on the device for its duration
struct ExportScratch {
    uint32_t *blk = nullptr, *index = nullptr;
    uint4 *rows = nullptr, *sh = nullptr;
    float *wide = nullptr;
    ~ExportScratch() { dev_free(blk); dev_free(index); dev_free(rows); dev_free(sh); dev_free(wide); }
};

int export_begin(gs_ctx *ctx, const char *name)
{
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "%s: context was fed worker matrices only (gs_push_matrices): it holds no packed records", name);
    return ctx->n ? reading_stream(ctx) : GS_OK;
}

// One filter over the whole cloud, on the reading stream: count and offsets (S.blk, *total = the passing splats), then -- rows wanted and
// some pass -- *rows, *wide and *index are allocated (wide, index: may be null, that part is not wanted) and the scatter is launched.
// Not waited for: S.blk lives until the caller has
int export_rows(gs_ctx *ctx, ExportScratch &S, uint8_t mask, uint8_t value, uint4 **rows /* null: the count alone */, float **wide, uint32_t **index, size_t *total)
{
    const uint32_t n = (uint32_t)ctx->n;
    const StateFilter pass = { ctx->edit_state, filter_rows(ctx, mask), mask, value };
    TRY(compact_offsets(ctx, ctx->prop_stream, pass, n, &S.blk, total));
    if (!rows || !*total) return GS_OK;
    TRY(dev_alloc(ctx, rows, *total * 2));
    if (wide) TRY(dev_alloc(ctx, wide, *total * 7));
    if (index) TRY(dev_alloc(ctx, index, *total));
    hipLaunchKernelGGL(k_export_scatter, dim3(gs_div_up(n, GS_EDIT_CHUNK)), dim3(GS_BLOCK), 0, ctx->prop_stream, pass, n, (const uint32_t *)S.blk,
                       (const uint4 *)ctx->splat, *rows, wide ? *wide : nullptr, index ? *index : nullptr);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
// ... and the same over the first ns splats, those that have an SH row: *sh = the passing ones' padded rows, row_q 16-byte words each
int export_sh(gs_ctx *ctx, ExportScratch &S, uint32_t ns, uint8_t mask, uint8_t value, uint32_t row_q, uint4 **sh /* null: the count alone */, size_t *total)
{
    const StateFilter pass = { ctx->edit_state, filter_rows(ctx, mask), mask, value };
    TRY(compact_offsets(ctx, ctx->prop_stream, pass, ns, &S.blk, total));
    if (!sh || !*total) return GS_OK;
    TRY(dev_alloc(ctx, sh, *total * row_q));
    hipLaunchKernelGGL(k_export_sh, dim3(gs_div_up(ns, GS_EDIT_CHUNK)), dim3(GS_BLOCK), 0, ctx->prop_stream, pass, ns, (const uint32_t *)S.blk, (const uint4 *)ctx->sh,
                       row_q, *sh);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// gs_export_sh: the rows of the store's degree, tight
int export_sh_rows(gs_ctx *ctx, uint8_t mask, uint8_t value, float *out_sh, size_t *out_nrows, int *out_degree)
{
    *out_nrows = 0;
    if (out_degree) *out_degree = 0;
    TRY(export_begin(ctx, "gs_export_sh"));
    const size_t n = ctx->sh_n < ctx->n ? ctx->sh_n : ctx->n;
    if (!n) return GS_OK;
    if (out_degree) *out_degree = ctx->sh_deg;
    const size_t K = (size_t)gsm::sh_coefs(ctx->sh_deg), KS = (size_t)gsm::sh_channel_stride(ctx->sh_deg);
    ExportScratch S;
    TRY(export_sh(ctx, S, (uint32_t)n, mask, value, (uint32_t)(3 * KS / 4), out_sh ? &S.sh : nullptr, out_nrows));
    if (!out_sh || !*out_nrows) return GS_OK;
    GS_HIP(hipMemcpy2DAsync(out_sh, K * 4, S.sh, KS * 4, K * 4, *out_nrows * 3, hipMemcpyDeviceToHost, ctx->prop_stream));   // tight rows out of the padded ones
    GS_HIP(hipStreamSynchronize(ctx->prop_stream));
    return GS_OK;
}

}  // namespace

// the passing splats staged for a writer that stays on the device (gs_export_stage.h): gs_export_splat's and gs_export_sh's launches without the copies
int gs_export_stage(gs_ctx *ctx, const char *name, uint8_t mask, uint8_t value, bool with_rows, GsExportStage *out)
{
    *out = GsExportStage();
    TRY(export_begin(ctx, name));
    if (!ctx->n) return GS_OK;
    {
        ExportScratch S;
        TRY(export_rows(ctx, S, mask, value, with_rows ? &out->rows : nullptr, &out->wide, &out->index, &out->total));
        if (with_rows && out->total) GS_HIP(hipStreamSynchronize(ctx->prop_stream));   // (S.blk is released with this block)
    }
    const size_t ns = ctx->sh_n < ctx->n ? ctx->sh_n : ctx->n;
    if (!ns) return GS_OK;
    out->sh_deg = ctx->sh_deg;
    out->sh_row_q = (uint32_t)(3 * (size_t)gsm::sh_channel_stride(ctx->sh_deg) / 4);
    ExportScratch S;
    TRY(export_sh(ctx, S, (uint32_t)ns, mask, value, out->sh_row_q, with_rows ? &out->sh : nullptr, &out->sh_total));
    if (with_rows && out->sh_total) GS_HIP(hipStreamSynchronize(ctx->prop_stream));
    return GS_OK;
}
void gs_export_stage_free(GsExportStage *s) { dev_free(s->rows); dev_free(s->wide); dev_free(s->index); dev_free(s->sh); *s = GsExportStage(); }

extern "C" {

GS_API int gs_export_splat(gs_ctx *ctx, uint8_t state_mask, uint8_t state_value, void *out_rows, float *out_wide, uint32_t *out_index, size_t *out_nrows)
{
    CHECK_CTX(ctx);
    if (!out_nrows) FAIL(GS_E_BADARG, "gs_export_splat: out_nrows is NULL");
    *out_nrows = 0;
    TRY(export_begin(ctx, "gs_export_splat"));
    if (!ctx->n) return GS_OK;
    ExportScratch S;
    TRY(export_rows(ctx, S, state_mask, state_value, out_rows ? &S.rows : nullptr, out_wide ? &S.wide : nullptr, out_index ? &S.index : nullptr, out_nrows));
    const size_t total = *out_nrows;
    if (!out_rows || !total) return GS_OK;                       // the size query, or nothing passes
    hipStream_t st = ctx->prop_stream;
    GS_HIP(hipMemcpyAsync(out_rows, S.rows, total * 32, hipMemcpyDeviceToHost, st));
    if (out_wide) GS_HIP(hipMemcpyAsync(out_wide, S.wide, total * 7 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_index) GS_HIP(hipMemcpyAsync(out_index, S.index, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    return GS_OK;
}

GS_API int gs_export_sh(gs_ctx *ctx, uint8_t state_mask, uint8_t state_value, float *out_sh, size_t *out_nrows, int *out_degree)
{
    CHECK_CTX(ctx);
    if (!out_nrows) FAIL(GS_E_BADARG, "gs_export_sh: out_nrows is NULL");
    return export_sh_rows(ctx, state_mask, state_value, out_sh, out_nrows, out_degree);
}

GS_API int gs_export_ply(gs_ctx *ctx, uint8_t state_mask, uint8_t state_value, int sh_degree, void *out_bytes, size_t *out_nbytes)
{
    CHECK_CTX(ctx);
    if (!out_nbytes) FAIL(GS_E_BADARG, "gs_export_ply: out_nbytes is NULL");
    *out_nbytes = 0;
    if (sh_degree < 0 || sh_degree > GS_SH_MAX_DEGREE) FAIL(GS_E_BADARG, "gs_export_ply: sh_degree must be 0..3");
    TRY(export_begin(ctx, "gs_export_ply"));
    // the degree written: what is asked for, at most what is stored
    const int stored = (ctx->sh_n && ctx->n) ? ctx->sh_deg : 0, D = sh_degree < stored ? sh_degree : stored;
    size_t n = 0;
    TRY(gs_export_splat(ctx, state_mask, state_value, nullptr, nullptr, nullptr, &n));
    if (!out_bytes) {
        if (gs_splat_to_ply(nullptr, nullptr, nullptr, 0, D, n, nullptr, out_nbytes) != GS_OK) FAIL(GS_E_BADARG, "gs_export_ply: size query failed");
        return GS_OK;
    }
    std::vector<uint8_t> rows;
    std::vector<float> wide, sh, cut;
    size_t sh_rows = 0;
    int sh_deg = 0;
    try {
        rows.resize(n * 32 + 1); wide.resize(n * 7 + 1);
        if (n) TRY(gs_export_splat(ctx, state_mask, state_value, rows.data(), wide.data(), nullptr, &n));
        if (stored) {
            TRY(export_sh_rows(ctx, state_mask, state_value, nullptr, &sh_rows, &sh_deg));
            const size_t Ks = (size_t)gsm::sh_coefs(stored), Kd = (size_t)gsm::sh_coefs(D);
            sh.resize(sh_rows * 3 * Ks + 1);
            if (sh_rows) TRY(export_sh_rows(ctx, state_mask, state_value, sh.data(), &sh_rows, &sh_deg));
            // the leading bands of every channel: rows of degree `stored` -> rows of degree D
            cut.resize(sh_rows * 3 * Kd + 1);
            for (size_t i = 0; i < sh_rows; i++)
                for (size_t c = 0; c < 3; c++) memcpy(&cut[(i * 3 + c) * Kd], &sh[(i * 3 + c) * Ks], Kd * sizeof(float));
        }
    } catch (...) { FAIL(GS_E_OOM, "gs_export_ply: out of host memory for %zu rows", n); }
    const int rc = gs_splat_to_ply(rows.data(), wide.data(), sh_rows ? cut.data() : nullptr, sh_rows, D, n, out_bytes, out_nbytes);
    if (rc != GS_OK) FAIL(rc, "gs_export_ply: writing the file failed");
    return GS_OK;
}

}  // extern "C"

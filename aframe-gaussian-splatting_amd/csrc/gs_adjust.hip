// gs_adjust.hip -- changing resident splats in place (include/gs_splat.h: gs_adjust_colour, gs_replace_splat, gs_replace_sh): the colour
// word and the SH row of the splats that pass a state filter through the affine map of gs_adjust.h, and rows [first, first + nrows) packed
// again by the pack kernel (gs_pack.hip) or copied over the SH store.
//
// Editor actions, not frame paths: the two kernels here are launched by gs_adjust_colour alone, on the owner's stream after every lane has
// been drained, and the call waits for them.  A context that never adjusts launches exactly the kernels it launched before.
//   k_adjust_colour  one thread per splat, grid-strided: the state byte (where the store has one), then a 4-byte read-modify-write of the
//                    colour word -- the last word of the record's second half; the other twelve bytes are neither loaded nor stored.
//   k_adjust_sh      one thread per (row, k) over the rows that have a splat, k innermost: a wave's 64 loads of one channel are
//                    contiguous (rows of K = 4 or 16 coefficients: whole 16-byte words; K = 9: runs of nine).  Three loads (one per channel,
//                    sh_channel_stride apart), three stores; a row's threads share one state byte.
// Both are f64 like the property and export kernels; neither uses LDS beyond the four words of the count.
#include "gs_lanes.h"
#include "gs_sh.h"
#include "gs_cloud_pass.h"
#include "gs_adjust.h"

namespace {

// (earlier versions of the tests read this name out of this file; the kernels' cap is pass_grid's default, gs_cloud_pass.h's GS_EDIT_GRID)
#define GS_ADJUST_GRID 2048u
static_assert(GS_ADJUST_GRID == GS_EDIT_GRID, "the adjust kernels run under the editing kernels' cap");

// words: the records as 32-bit words, eight per splat; rows = 0 when the mask is 0 or the store is empty (no state byte is loaded then)
__global__ __launch_bounds__(GS_BLOCK) void k_adjust_colour(const uint8_t *__restrict__ state, uint32_t rows, uint32_t n, uint32_t mask, uint32_t value,
                                                            gsm::AdjustParams p, uint32_t *__restrict__ words, uint32_t *__restrict__ hit)
{
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        if (!state_passes(state, rows, i, mask, value)) continue;
        uint32_t *w = words + 8 * (size_t)i + 7;                 // splat[2 i + 1].w
        *w = gsm::adjust_word(*w, p);
        c++;
    }
    block_count(c, hit);
}

// sh: the store's padded rows (3 channels of KS f32, K of them used); n: the rows that belong to a resident splat
__global__ __launch_bounds__(GS_BLOCK) void k_adjust_sh(const uint8_t *__restrict__ state, uint32_t rows, uint32_t n, uint32_t mask, uint32_t value,
                                                        gsm::AdjustParams p, float *__restrict__ sh, uint32_t K, uint32_t KS)
{
    const uint64_t total = (uint64_t)n * K;
    for (uint64_t t = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; t < total; t += (uint64_t)gridDim.x * GS_BLOCK) {
        const uint32_t i = (uint32_t)(t / K), k = (uint32_t)(t % K);
        if (!state_passes(state, rows, i, mask, value)) continue;
        float *r = sh + (size_t)i * 3 * KS + k;
        const float in[3] = { r[0], r[KS], r[2 * KS] };
        float out[3];
        gsm::adjust_sh_coef(in, (int)k, p, out);
        r[0] = out[0]; r[KS] = out[1]; r[2 * KS] = out[2];
    }
}

int adjust_run(gs_ctx *ctx, const gsm::AdjustParams &p, uint8_t mask, uint8_t value, size_t *hit)
{
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));                                         // frames in flight read both arrays
    TRY(counters(ctx));
    const uint32_t n = (uint32_t)ctx->n, rows = filter_rows(ctx, mask);
    hipLaunchKernelGGL(k_adjust_colour, dim3(pass_grid(n)), dim3(GS_BLOCK), 0, ctx->stream, (const uint8_t *)ctx->edit_state, rows, n, (uint32_t)mask, (uint32_t)value,
                       p, reinterpret_cast<uint32_t *>(ctx->splat), ctx->edit_cnt);
    const uint32_t sh_rows = (uint32_t)(ctx->sh_n < ctx->n ? ctx->sh_n : ctx->n);
    if (sh_rows) {
        const uint32_t K = (uint32_t)gsm::sh_coefs(ctx->sh_deg), KS = (uint32_t)gsm::sh_channel_stride(ctx->sh_deg);
        hipLaunchKernelGGL(k_adjust_sh, dim3(pass_grid((uint64_t)sh_rows * K)), dim3(GS_BLOCK), 0, ctx->stream, (const uint8_t *)ctx->edit_state, rows, sh_rows,
                           (uint32_t)mask, (uint32_t)value, p, ctx->sh, K, KS);
    }
    return read_counter(ctx, hit);
}

}  // namespace

extern "C" {

GS_API int gs_adjust_colour(gs_ctx *ctx, const gs_colour_adjust *adjust, uint8_t state_mask, uint8_t state_value, size_t *out_hit)
{
    CHECK_CTX(ctx);
    if (out_hit) *out_hit = 0;
    if (!adjust) FAIL(GS_E_BADARG, "gs_adjust_colour: adjust is NULL");
    gsm::AdjustParams p;
    if (!gsm::adjust_widen(adjust->m, adjust->offset, adjust->alpha_scale, adjust->alpha_offset, p)) FAIL(GS_E_BADARG, "gs_adjust_colour: a parameter is not finite");
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "gs_adjust_colour: context was fed worker matrices only (gs_push_matrices): it holds no packed records");
    if (!ctx->n) return GS_OK;
    return adjust_run(ctx, p, state_mask, state_value, out_hit);
}

GS_API int gs_replace_splat(gs_ctx *ctx, size_t first, const void *rows, size_t nrows)
{
    CHECK_CTX(ctx);
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "gs_replace_splat: context was fed worker matrices only (gs_push_matrices): it holds no packed records");
    if (first > ctx->n || nrows > ctx->n - first) FAIL(GS_E_BADARG, "gs_replace_splat: rows [%zu, %zu) of %zu splats", first, first + nrows, ctx->n);
    if (nrows == 0) return GS_OK;
    if (!rows) FAIL(GS_E_BADARG, "gs_replace_splat: rows is NULL");
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    uint4 *stage = nullptr;
    TRY(dev_alloc(ctx, &stage, nrows * 2));
    int rc = GS_OK;
    hipError_t e = hipMemcpyAsync(stage, rows, nrows * 32, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "upload failed: %s", hipGetErrorString(e)); rc = GS_E_HIP; }
    if (rc == GS_OK) rc = gs_launch_pack(ctx, stage, first, nrows);   // both records, the sort row and bound_r of [first, first + nrows)
    e = hipStreamSynchronize(ctx->stream);
    if (rc == GS_OK && e != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "pack failed: %s", hipGetErrorString(e)); rc = GS_E_HIP; }
    dev_free(stage);
    drop_orders(ctx);
    return rc;
}

GS_API int gs_replace_sh(gs_ctx *ctx, size_t first, const float *sh_rows, size_t nrows, int degree)
{
    CHECK_CTX(ctx);
    if (degree < 1 || degree > GS_SH_MAX_DEGREE) FAIL(GS_E_BADARG, "gs_replace_sh: degree must be 1..3");
    if (first > ctx->sh_n || nrows > ctx->sh_n - first) FAIL(GS_E_BADARG, "gs_replace_sh: rows [%zu, %zu) of %zu SH rows", first, first + nrows, ctx->sh_n);
    if (ctx->sh_n && degree != ctx->sh_deg) FAIL(GS_E_BADARG, "gs_replace_sh: rows of degree %d over stored rows of degree %d", degree, ctx->sh_deg);
    if (nrows == 0) return GS_OK;
    if (!sh_rows) FAIL(GS_E_BADARG, "gs_replace_sh: sh_rows is NULL");
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));                                         // frames in flight read the store
    // tight rows in, channels padded to whole 16-byte words in the store (as gs_push_sh)
    const int K = gsm::sh_coefs(degree), KS = gsm::sh_channel_stride(degree);
    const float *src = sh_rows;
    std::vector<float> padded;
    if (KS != K) {
        try { padded.assign(nrows * 3 * (size_t)KS, 0.0f); } catch (...) { FAIL(GS_E_OOM, "out of host memory for %zu SH rows", nrows); }
        for (size_t i = 0; i < nrows; i++)
            for (int c = 0; c < 3; c++) memcpy(&padded[(i * 3 + c) * KS], sh_rows + (i * 3 + c) * K, (size_t)K * sizeof(float));
        src = padded.data();
    }
    GS_HIP(hipMemcpy(ctx->sh + first * 3 * (size_t)KS, src, nrows * 3 * (size_t)KS * sizeof(float), hipMemcpyHostToDevice));
    return GS_OK;
}

}  // extern "C"

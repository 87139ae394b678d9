// gs_transform.hip -- moving resident splats in place (include/gs_splat.h: gs_transform): the splats that pass a state filter go through
// the similarity of gs_transform.h -- both 16-byte records, the sort row, the strip bound and, under a rotation, the SH row.
//
// An editor action, not a frame path: the two kernels here are launched by gs_transform alone, on the owner's stream after every lane
// has been drained, and the call waits for them.  A context that never transforms launches exactly the kernels it launched before.
//   k_transform_records  one thread per splat, grid-strided: the state byte (where the store has one); a passing splat's record as two
//                        16-byte loads and two 16-byte stores, its sort row as one float4 load and one store, one bound_r store.  A
//                        splat that does not pass stores nothing.  R, scale, scale^2 and the translation travel by value.
//   k_transform_sh       one thread per (row, channel) over the rows that have a splat.  The work is in place and every output of a band
//                        reads all of the band's inputs, so one thread owns the whole channel: its sh_channel_stride floats come in as
//                        16-byte words, all of them before the first goes out (what goes back unchanged -- k = 0, a degree-2 channel's
//                        padding -- the compiler leaves out of both).  The 83 matrix entries travel by value and are read at
//                        compile-time offsets (the degree is a template parameter, every loop unrolled): uniform loads.
// Both are f64 like the property and export kernels; neither uses LDS beyond the four words of the count.
#include "gs_lanes.h"
#include "gs_sh.h"
#include "gs_cloud_pass.h"
#include "gs_transform.h"

namespace {

// rows = 0 when the mask is 0 or the store is empty (no state byte is loaded then)
__global__ __launch_bounds__(GS_BLOCK) void k_transform_records(const uint8_t *__restrict__ state, uint32_t rows, uint32_t n, uint32_t mask, uint32_t value,
                                                                gsm::TransformParams p, uint4 *__restrict__ splat, float4 *__restrict__ sort_rows,
                                                                float *__restrict__ bound_r, uint32_t *__restrict__ hit)
{
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        if (!state_passes(state, rows, i, mask, value)) continue;
        const uint4 a = splat[2 * (size_t)i], b = splat[2 * (size_t)i + 1];
        const float4 r = sort_rows[i];
        const float cs[4] = { __uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w) };
        const uint32_t cc[4] = { b.x, b.y, b.z, b.w };
        const float sr[4] = { r.x, r.y, r.z, r.w };
        float cs2[4], sr2[4], bound;
        uint32_t cc2[4];
        gsm::transform_record(cs, cc, sr, p, cs2, cc2, sr2, bound);
        splat[2 * (size_t)i] = make_uint4(__float_as_uint(cs2[0]), __float_as_uint(cs2[1]), __float_as_uint(cs2[2]), __float_as_uint(cs2[3]));
        splat[2 * (size_t)i + 1] = make_uint4(cc2[0], cc2[1], cc2[2], cc2[3]);
        sort_rows[i] = make_float4(sr2[0], sr2[1], sr2[2], sr2[3]);
        bound_r[i] = bound;
        c++;
    }
    block_count(c, hit);
}

// sh: the store's padded rows (3 channels of KS f32, K of them used; KS a multiple of 4); n: the rows that belong to a resident splat
template <int DEG>
__global__ __launch_bounds__(GS_BLOCK) void k_transform_sh(const uint8_t *__restrict__ state, uint32_t rows, uint32_t n, uint32_t mask, uint32_t value,
                                                           gsm::ShRotation rot, float4 *__restrict__ sh)
{
    constexpr int K = (DEG + 1) * (DEG + 1), W = ((K + 3) & ~3) / 4;   // coefficients, and 16-byte words per channel
    const uint64_t total = (uint64_t)n * 3;
    for (uint64_t t = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; t < total; t += (uint64_t)gridDim.x * GS_BLOCK) {
        const uint32_t i = (uint32_t)(t / 3);
        if (!state_passes(state, rows, i, mask, value)) continue;
        float4 *ch = sh + t * W;                                  // channel t % 3 of row i: (i * 3 + c) * KS floats in
        float v[4 * W];
#pragma unroll
        for (int w = 0; w < W; w++) { const float4 q = ch[w]; v[4 * w] = q.x; v[4 * w + 1] = q.y; v[4 * w + 2] = q.z; v[4 * w + 3] = q.w; }
        gsm::transform_sh_channel<DEG>(v, rot, v);                // (the padding beyond K goes back as it came)
#pragma unroll
        for (int w = 0; w < W; w++) ch[w] = make_float4(v[4 * w], v[4 * w + 1], v[4 * w + 2], v[4 * w + 3]);
    }
}

int transform_run(gs_ctx *ctx, const gsm::TransformParams &p, uint8_t mask, uint8_t value, size_t *hit)
{
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));                                         // frames in flight read every array
    TRY(counters(ctx));
    const uint32_t n = (uint32_t)ctx->n, rows = filter_rows(ctx, mask);
    hipLaunchKernelGGL(k_transform_records, dim3(pass_grid(n)), dim3(GS_BLOCK), 0, ctx->stream, (const uint8_t *)ctx->edit_state, rows, n, (uint32_t)mask,
                       (uint32_t)value, p, ctx->splat, ctx->sort_rows, ctx->bound_r, ctx->edit_cnt);
    const uint32_t sh_rows = (uint32_t)(ctx->sh_n < ctx->n ? ctx->sh_n : ctx->n);
    if (sh_rows && !p.rot_identity) {                            // scale and translation leave SH alone
        gsm::ShRotation rot;
        gsm::sh_rotation(p, rot);
        const dim3 grid(pass_grid((uint64_t)sh_rows * 3)), block(GS_BLOCK);
        const uint8_t *st = (const uint8_t *)ctx->edit_state;
        float4 *sh = reinterpret_cast<float4 *>(ctx->sh);
        if (ctx->sh_deg == 1) hipLaunchKernelGGL(k_transform_sh<1>, grid, block, 0, ctx->stream, st, rows, sh_rows, (uint32_t)mask, (uint32_t)value, rot, sh);
        else if (ctx->sh_deg == 2) hipLaunchKernelGGL(k_transform_sh<2>, grid, block, 0, ctx->stream, st, rows, sh_rows, (uint32_t)mask, (uint32_t)value, rot, sh);
        else hipLaunchKernelGGL(k_transform_sh<3>, grid, block, 0, ctx->stream, st, rows, sh_rows, (uint32_t)mask, (uint32_t)value, rot, sh);
    }
    const int rc = read_counter(ctx, hit);                       // (waits for both kernels)
    drop_orders(ctx);                                            // positions changed: as after a push
    return rc;
}

}  // namespace

extern "C" {

GS_API int gs_transform(gs_ctx *ctx, const gs_similarity *t, uint8_t state_mask, uint8_t state_value, size_t *out_hit)
{
    CHECK_CTX(ctx);
    if (out_hit) *out_hit = 0;
    if (!t) FAIL(GS_E_BADARG, "gs_transform: t is NULL");
    gsm::TransformParams p;
    if (!gsm::transform_widen(t->rotation, t->scale, t->translation, p))
        FAIL(GS_E_BADARG, "gs_transform: a parameter is not finite, the scale is not positive or the quaternion's norm is 0");
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "gs_transform: context was fed worker matrices only (gs_push_matrices): it holds no packed records");
    if (!ctx->n) return GS_OK;
    return transform_run(ctx, p, state_mask, state_value, out_hit);
}

}  // extern "C"

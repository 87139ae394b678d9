// gs_cply.hip -- the chunked compressed .ply on the GPU (include/gs_splat.h: "Compressed .ply"; the arithmetic: gs_cply.h, shared
// with the host evaluators of gs_host.cpp so that both produce the same bytes by construction).
//
//   decode (gs_load_cply, gs_cply_to_splat_gpu), on lane 0's stream after a drain, like gs_ply.hip:
//     host           the strict header reader (gs_cply_plan)
//     H2D            the body's three arrays, once (bounds records, 16 bytes per splat, the SH bytes)
//     k_cply_decode  one thread per splat, grid-stride: two uint4 per row, the wide part where asked, the padded SH row where kept
//     the rows stay in HBM and go straight into the pack kernel, in file order.
//   encode (gs_export_cply), on the reading calls' own stream: no drain, no order dropped (gs_export.hip's rule):
//     stage              the passing splats as rows, wide parts and SH rows by the export scheme (gs_export_stage)
//     k_cply_bounds_pos  GS_CPLY_MORTON: the box of all finite positions (wave reductions, one atomic per wave on ordered keys)
//     k_cply_keys        (30-bit Morton code, staged index) records, then four stable 8-bit radix passes: ties keep the index order.
//                        The passes run on the reading stream with histogram rows of the call's own (a private sorter), so a
//                        frame in flight keeps lane 0's.
//     k_cply_encode      one 256-thread workgroup per chunk: gather through the order, the nine values per thread, eighteen min / max
//                        by __shfl_xor within the wave and one LDS step across the four waves, then the record, the four words and
//                        the SH bytes.  Min and max are taken on unsigned keys (gsm::cply_key): exact, and the same in any order.
// Both are byte-shuffling and f64-ALU work on a one-time path; a context that never calls them launches none of these kernels.
#include "gs_lanes.h"
#include "gs_sh.h"
#include "gs_cloud_pass.h"
#include "gs_cply.h"
#include "gs_export_stage.h"

extern "C" int gs_cply_plan(const void *bytes, size_t nbytes, gsm::CplyInfo *info, char *err, size_t errlen);
extern "C" int gs_cply_write_header(size_t n, int degree, void *out, size_t *len);

namespace {

#define GS_CPLY_GRID 16384u                                      // workgroups at most for the grid-strided kernels here

// sh_out (may be null): rows of 3 x KS f32 (the store's padded layout, pad 0), K coefficients kept per channel
__global__ __launch_bounds__(GS_BLOCK) void k_cply_decode(const float *__restrict__ chunks, int cf, const uint4 *__restrict__ verts,
                                                          const uint8_t *__restrict__ shb, int per, uint32_t n, uint4 *__restrict__ rows,
                                                          float *__restrict__ wide, float *__restrict__ sh_out, int K, int KS)
{
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        float chunk[18];
        const float *src = chunks + (size_t)(i >> 8) * cf;
#pragma unroll
        for (int q = 0; q < 12; q++) chunk[q] = src[q];
#pragma unroll
        for (int q = 12; q < 18; q++) chunk[q] = cf == 18 ? src[q] : 0.0f;
        const uint4 v = verts[i];
        const uint32_t packed[4] = { v.x, v.y, v.z, v.w };
        uint32_t w[8];
        float wd[7];
        double colour[3];
        gsm::cply_decode(chunk, cf, packed, w, wd, colour);
        rows[2 * (size_t)i] = make_uint4(w[0], w[1], w[2], w[3]);
        rows[2 * (size_t)i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        if (wide) {
#pragma unroll
            for (int q = 0; q < 7; q++) wide[7 * (size_t)i + q] = wd[q];
        }
        if (sh_out) {
            float *o = sh_out + (size_t)i * 3 * KS;
            const uint8_t *s = shb + (size_t)i * 3 * per;
            for (int c = 0; c < 3; c++) {
                o[c * KS] = gsm::cply_sh_dc(c == 0 ? colour[0] : c == 1 ? colour[1] : colour[2]);
                for (int k = 1; k < K; k++) o[c * KS + k] = gsm::cply_sh_rest(s[c * per + (k - 1)]);
                for (int k = K; k < KS; k++) o[c * KS + k] = 0.0f;
            }
        }
    }
}

// box[0..2] = the smallest key per axis, box[3..5] = the largest (the identities before the launch)
__global__ __launch_bounds__(GS_BLOCK) void k_cply_bounds_pos(const uint4 *__restrict__ rows, uint32_t n, uint32_t *__restrict__ box)
{
    uint32_t mn[3] = { GS_CPLY_KEY_MIN_ID, GS_CPLY_KEY_MIN_ID, GS_CPLY_KEY_MIN_ID }, mx[3] = { GS_CPLY_KEY_MAX_ID, GS_CPLY_KEY_MAX_ID, GS_CPLY_KEY_MAX_ID };
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        const uint4 r = rows[2 * (size_t)i];
        const float p[3] = { __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z) };
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!gsm::cply_finite(p[a])) continue;
            const uint32_t k = gsm::cply_key(p[a]);
            mn[a] = k < mn[a] ? k : mn[a]; mx[a] = k > mx[a] ? k : mx[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const uint32_t lo = wave_min(mn[a]), hi = wave_max(mx[a]);
        if ((threadIdx.x & 63) == 0) { atomicMin(&box[a], lo); atomicMax(&box[3 + a], hi); }
    }
}

__global__ __launch_bounds__(GS_BLOCK) void k_cply_keys(const uint4 *__restrict__ rows, uint32_t n, const uint32_t *__restrict__ box, uint2 *__restrict__ kv)
{
    float b[6];
#pragma unroll
    for (int a = 0; a < 3; a++) gsm::cply_bounds_of(box[a], box[3 + a], b[a], b[3 + a]);
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        const uint4 r = rows[2 * (size_t)i];
        const float p[3] = { __uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z) };
        kv[i] = make_uint2(gsm::cply_morton(p, b), i);
    }
}

// One workgroup per chunk (GS_BLOCK == GS_CPLY_CHUNK).  order (may be null: staged order): .y = the staged row of output row j.
// sh: the staged padded SH rows of the first sh_total staged rows (KS_in f32 per channel), K coefficients written per channel.
__global__ __launch_bounds__(GS_BLOCK) void k_cply_encode(const uint4 *__restrict__ rows, const float *__restrict__ wide, const uint32_t *__restrict__ index,
                                                          const float *__restrict__ sh, uint32_t sh_total, int KS_in, int K, const uint2 *__restrict__ order,
                                                          uint32_t n, float *__restrict__ o_chunks, uint4 *__restrict__ o_verts, uint8_t *__restrict__ o_sh,
                                                          uint32_t *__restrict__ o_index)
{
    __shared__ uint32_t s_k[GS_BLOCK / 64][18];
    const uint32_t j = blockIdx.x * GS_CPLY_CHUNK + threadIdx.x;
    const bool live = j < n;
    uint32_t src = 0;
    uint32_t row[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    float wd[7] = { 0, 0, 0, 0, 0, 0, 0 }, v[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    const float *shrow = nullptr;
    uint32_t kmin[9], kmax[9];
#pragma unroll
    for (int q = 0; q < 9; q++) { kmin[q] = GS_CPLY_KEY_MIN_ID; kmax[q] = GS_CPLY_KEY_MAX_ID; }
    if (live) {
        src = order ? order[j].y : j;
        const uint4 r0 = rows[2 * (size_t)src], r1 = rows[2 * (size_t)src + 1];
        row[0] = r0.x; row[1] = r0.y; row[2] = r0.z; row[3] = r0.w; row[4] = r1.x; row[5] = r1.y; row[6] = r1.z; row[7] = r1.w;
#pragma unroll
        for (int q = 0; q < 7; q++) wd[q] = wide[7 * (size_t)src + q];
        if (src < sh_total) shrow = sh + (size_t)src * 3 * KS_in;
        gsm::cply_values(row, wd, shrow, KS_in, v);
#pragma unroll
        for (int q = 0; q < 9; q++)
            if (gsm::cply_finite(v[q])) { kmin[q] = kmax[q] = gsm::cply_key(v[q]); }
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 9; q++) {
        const uint32_t lo = wave_min(kmin[q]), hi = wave_max(kmax[q]);
        if ((threadIdx.x & 63) == 0) { s_k[wv][q] = lo; s_k[wv][9 + q] = hi; }
    }
    __syncthreads();
    // the record's layout: min xyz, max xyz | min scale, max scale | min rgb, max rgb
    float bounds[18];
#pragma unroll
    for (int q = 0; q < 9; q++) {
        uint32_t lo = s_k[0][q], hi = s_k[0][9 + q];
#pragma unroll
        for (int w = 1; w < GS_BLOCK / 64; w++) { lo = s_k[w][q] < lo ? s_k[w][q] : lo; hi = s_k[w][9 + q] > hi ? s_k[w][9 + q] : hi; }
        gsm::cply_bounds_of(lo, hi, bounds[6 * (q / 3) + q % 3], bounds[6 * (q / 3) + 3 + q % 3]);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 18; q++) o_chunks[(size_t)blockIdx.x * 18 + q] = bounds[q];
    }
    if (!live) return;
    uint32_t w[4];
    gsm::cply_encode(v, bounds, row, wd, w);
    o_verts[j] = make_uint4(w[0], w[1], w[2], w[3]);
    const int per = K - 1;
    for (int c = 0; c < 3; c++)
        for (int k = 1; k < K; k++) o_sh[(size_t)j * 3 * per + c * per + (k - 1)] = shrow ? gsm::cply_sh_byte(shrow[c * KS_in + k]) : (uint8_t)128;
    if (o_index) o_index[j] = index[src];
}

// everything the decoder holds on the device for a call
struct DecodeScratch {
    float *chunks = nullptr; uint4 *verts = nullptr; uint8_t *shb = nullptr;
    ~DecodeScratch() { dev_free(chunks); dev_free(verts); dev_free(shb); }
};

// rows (n x 2 uint4), wide (n x 7 f32, may be null) and sh_out (may be null; n padded rows of degree D) are device buffers of the caller's.
// On ctx->stream (the caller has drained the lanes); the stream is idle on return.
int decode_to_device(gs_ctx *ctx, const void *bytes, const gsm::CplyInfo &I, uint4 *rows, float *wide, float *sh_out, int D)
{
    if (!I.n) return GS_OK;
    hipStream_t st = ctx->stream;
    DecodeScratch S;
    const uint8_t *body = (const uint8_t *)bytes + I.data_start;
    const size_t chunk_bytes = I.chunks * (size_t)I.chunk_floats * 4, vert_bytes = I.n * 16, sh_bytes = I.n * 3 * (size_t)I.per;
    const bool want_sh = sh_out && I.per;
    TRY(dev_alloc(ctx, &S.chunks, chunk_bytes / 4));
    TRY(dev_alloc(ctx, &S.verts, I.n));
    GS_HIP(hipMemcpyAsync(S.chunks, body, chunk_bytes, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemcpyAsync(S.verts, body + chunk_bytes, vert_bytes, hipMemcpyHostToDevice, st));
    if (want_sh) {
        TRY(dev_alloc(ctx, &S.shb, sh_bytes));
        GS_HIP(hipMemcpyAsync(S.shb, body + chunk_bytes + vert_bytes, sh_bytes, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_cply_decode, dim3(pass_grid(I.n, GS_CPLY_GRID)), dim3(GS_BLOCK), 0, st, (const float *)S.chunks, I.chunk_floats, (const uint4 *)S.verts,
                       (const uint8_t *)S.shb, I.per, (uint32_t)I.n, rows, wide, sh_out, gsm::sh_coefs(D), gsm::sh_channel_stride(D));
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(st));
    return GS_OK;
}

// room for `want` rows of `degree` in the SH store, the stored rows kept (gs_push_sh's growth rule)
int sh_reserve(gs_ctx *ctx, size_t want, int degree)
{
    if (!ctx->sh_n && ctx->sh_deg != degree) { dev_free(ctx->sh); ctx->sh_cap = 0; }   // (an emptied store of another row size)
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

// A sorter of the call's own for the reading stream: gs_radix_pass reads a lane's stream, histogram rows and digit totals, nothing else.
struct PrivateSorter {
    gs_ctx *lane = nullptr;
    ~PrivateSorter() { if (lane) { dev_free(lane->hist); dev_free(lane->radix_aux); delete lane; } }
    int init(gs_ctx *ctx, size_t items)
    {
        lane = new (std::nothrow) gs_ctx();
        if (!lane) FAIL(GS_E_OOM, "out of host memory");
        memset(lane, 0, sizeof *lane);
        lane->device = ctx->device; lane->stream = ctx->prop_stream;
        TRY(dev_alloc(ctx, &lane->hist, (size_t)GS_RADIX_MAX_BINS * (gs_div_up(items, GS_CHUNK_S) + 16)));
        TRY(dev_alloc(ctx, &lane->radix_aux, (size_t)GS_RADIX_MAX_BINS * 2));
        return GS_OK;
    }
};

struct EncodeScratch {
    float *chunks = nullptr; uint4 *verts = nullptr; uint8_t *shb = nullptr; uint32_t *index = nullptr, *small = nullptr; uint2 *kv_a = nullptr, *kv_b = nullptr;
    GsExportStage stage;
    ~EncodeScratch() { dev_free(chunks); dev_free(verts); dev_free(shb); dev_free(index); dev_free(small); dev_free(kv_a); dev_free(kv_b); gs_export_stage_free(&stage); }
};

}  // namespace

extern "C" {

GS_API int gs_cply_to_splat_gpu(gs_ctx *ctx, const void *bytes, size_t nbytes, void *out_rows, float *out_wide, size_t *out_nrows)
{
    CHECK_CTX(ctx);
    if (!bytes || !out_nrows) FAIL(GS_E_BADARG, "gs_cply_to_splat_gpu: NULL argument");
    *out_nrows = 0;
    gsm::CplyInfo I;
    TRY(gs_cply_plan(bytes, nbytes, &I, ctx->err, sizeof ctx->err));
    *out_nrows = I.n;
    if (!out_rows || !I.n) return GS_OK;
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));                                         // the decoder borrows lane 0's stream
    uint4 *rows = nullptr; float *wide = nullptr;
    int rc = dev_alloc(ctx, &rows, I.n * 2);
    if (rc == GS_OK && out_wide) rc = dev_alloc(ctx, &wide, I.n * 7);
    if (rc == GS_OK) rc = decode_to_device(ctx, bytes, I, rows, wide, nullptr, 0);
    if (rc == GS_OK && hipMemcpy(out_rows, rows, I.n * 32, hipMemcpyDeviceToHost) != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "download failed"); rc = GS_E_HIP; }
    if (rc == GS_OK && out_wide && hipMemcpy(out_wide, wide, I.n * 7 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "download failed"); rc = GS_E_HIP; }
    dev_free(rows); dev_free(wide);
    return rc;
}

GS_API int gs_load_cply(gs_ctx *ctx, const void *bytes, size_t nbytes)
{
    CHECK_CTX(ctx);
    if (!bytes) FAIL(GS_E_BADARG, "gs_load_cply: bytes is NULL");
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "gs_load_cply after gs_push_matrices: mixed ingest is not supported");
    gsm::CplyInfo I;
    TRY(gs_cply_plan(bytes, nbytes, &I, ctx->err, sizeof ctx->err));
    if (!I.n) return GS_OK;
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    const size_t n_before = ctx->n;
    // gs_load_ply's rule for a parallel store: the option is on, the store is as long as the cloud, the file has bands, the degrees agree
    const int D = ctx->sh_opt < I.degree ? ctx->sh_opt : I.degree;
    const bool keep_sh = ctx->sh_opt >= 1 && ctx->sh_n == n_before && D >= 1 && !(ctx->sh_n && D != ctx->sh_deg);
    if (keep_sh && ctx->sh_n + I.n > 0x7FFFFFF0ull) FAIL(GS_E_BADARG, "more than 2^31 SH rows");
    TRY(ensure_capacity(ctx, ctx->n + I.n));
    if (keep_sh) TRY(sh_reserve(ctx, ctx->sh_n + I.n, D));
    uint4 *rows = nullptr;
    TRY(dev_alloc(ctx, &rows, I.n * 2));
    float *sh_out = keep_sh ? ctx->sh + ctx->sh_n * 3 * (size_t)gsm::sh_channel_stride(D) : nullptr;   // (rows behind sh_n: no frame reads them yet)
    int rc = decode_to_device(ctx, bytes, I, rows, nullptr, sh_out, D);
    if (rc == GS_OK) {                                           // the rows never leave HBM, and keep the file's order
        rc = gs_launch_pack(ctx, rows, ctx->n, I.n);
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (rc == GS_OK && e != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "pack failed: %s", hipGetErrorString(e)); rc = GS_E_HIP; }
    }
    dev_free(rows);
    if (rc != GS_OK) return rc;
    ctx->n += I.n; ctx->renderable = true;
    for (int i = 0; i < GS_MAX_LANES; i++) if (ctx->lanes[i]) ctx->lanes[i]->have_sort = false;
    ctx->stats.n_splats = ctx->n;
    if (keep_sh) { ctx->sh_n += I.n; ctx->sh_deg = D; }
    return GS_OK;
}

GS_API int gs_export_cply(gs_ctx *ctx, uint8_t state_mask, uint8_t state_value, int sh_degree, uint32_t flags, uint32_t *out_index, void *out_bytes, size_t *out_nbytes)
{
    CHECK_CTX(ctx);
    if (!out_nbytes) FAIL(GS_E_BADARG, "gs_export_cply: out_nbytes is NULL");
    *out_nbytes = 0;
    if (sh_degree < 0 || sh_degree > GS_SH_MAX_DEGREE) FAIL(GS_E_BADARG, "gs_export_cply: sh_degree must be 0..3");
    if (flags & ~(uint32_t)GS_CPLY_MORTON) FAIL(GS_E_BADARG, "gs_export_cply: unknown flags 0x%x", flags);
    // the degree written: what is asked for, at most what is stored
    const int stored = (ctx->sh_n && ctx->n) ? ctx->sh_deg : 0, D = sh_degree < stored ? sh_degree : stored;
    EncodeScratch S;
    TRY(gs_export_stage(ctx, "gs_export_cply", state_mask, state_value, out_bytes != nullptr, &S.stage));
    const size_t n = S.stage.total;
    size_t head = 0;
    if (gs_cply_write_header(n, D, nullptr, &head) != GS_OK) FAIL(GS_E_BADARG, "gs_export_cply: size query failed");
    const int K = gsm::sh_coefs(D), per = K - 1;
    const size_t C = gs_div_up(n, GS_CPLY_CHUNK), chunk_bytes = C * 72, vert_bytes = n * 16, sh_bytes = n * 3 * (size_t)per;
    *out_nbytes = head + chunk_bytes + vert_bytes + sh_bytes;
    if (!out_bytes) return GS_OK;
    if (gs_cply_write_header(n, D, out_bytes, &head) != GS_OK) FAIL(GS_E_OOM, "gs_export_cply: writing the header failed");
    if (!n) return GS_OK;
    hipStream_t st = ctx->prop_stream;
    const uint32_t n32 = (uint32_t)n;
    TRY(dev_alloc(ctx, &S.chunks, C * 18)); TRY(dev_alloc(ctx, &S.verts, n)); TRY(dev_alloc(ctx, &S.shb, sh_bytes));
    if (out_index) TRY(dev_alloc(ctx, &S.index, n));
    const uint2 *order = nullptr;
    PrivateSorter sorter;
    if (flags & GS_CPLY_MORTON) {
        TRY(dev_alloc(ctx, &S.small, 8)); TRY(dev_alloc(ctx, &S.kv_a, n)); TRY(dev_alloc(ctx, &S.kv_b, n));
        TRY(sorter.init(ctx, n));
        // [0] = n for the radix kernels, [1..6] = the box's keys
        const uint32_t host_small[8] = { n32, GS_CPLY_KEY_MIN_ID, GS_CPLY_KEY_MIN_ID, GS_CPLY_KEY_MIN_ID, GS_CPLY_KEY_MAX_ID, GS_CPLY_KEY_MAX_ID, GS_CPLY_KEY_MAX_ID, 0u };
        GS_HIP(hipMemcpyAsync(S.small, host_small, sizeof host_small, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cply_bounds_pos, dim3(pass_grid(n, 1024)), dim3(GS_BLOCK), 0, st, (const uint4 *)S.stage.rows, n32, S.small + 1);
        hipLaunchKernelGGL(k_cply_keys, dim3(pass_grid(n, GS_CPLY_GRID)), dim3(GS_BLOCK), 0, st, (const uint4 *)S.stage.rows, n32, (const uint32_t *)(S.small + 1), S.kv_a);
        GS_HIP(hipGetLastError());
        int rc = GS_OK;
        for (int pass = 0; pass < 4 && rc == GS_OK; pass++) {
            const GsRadixIO io = { (pass & 1) ? S.kv_b : S.kv_a, (pass & 1) ? S.kv_a : S.kv_b, S.small, nullptr, nullptr };
            rc = gs_radix_pass<1>(&sorter.lane, &io, GS_RADIX_PACKED, GS_RADIX_PACKED, n32, n32, 8 * pass, 8);
        }
        if (rc != GS_OK) { memcpy(ctx->err, sorter.lane->err, sizeof ctx->err); (void)hipStreamSynchronize(st); return rc; }
        order = S.kv_a;                                          // 4 passes: back in kv_a
    }
    hipLaunchKernelGGL(k_cply_encode, dim3((uint32_t)C), dim3(GS_BLOCK), 0, st, (const uint4 *)S.stage.rows, (const float *)S.stage.wide, (const uint32_t *)S.stage.index,
                       (const float *)S.stage.sh, (uint32_t)S.stage.sh_total, gsm::sh_channel_stride(S.stage.sh_deg), K, order, n32, S.chunks, S.verts, S.shb, S.index);
    GS_HIP(hipGetLastError());
    uint8_t *out = (uint8_t *)out_bytes + head;
    GS_HIP(hipMemcpyAsync(out, S.chunks, chunk_bytes, hipMemcpyDeviceToHost, st));
    GS_HIP(hipMemcpyAsync(out + chunk_bytes, S.verts, vert_bytes, hipMemcpyDeviceToHost, st));
    if (sh_bytes) GS_HIP(hipMemcpyAsync(out + chunk_bytes + vert_bytes, S.shb, sh_bytes, hipMemcpyDeviceToHost, st));
    if (out_index) GS_HIP(hipMemcpyAsync(out_index, S.index, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    return GS_OK;
}

}  // extern "C"

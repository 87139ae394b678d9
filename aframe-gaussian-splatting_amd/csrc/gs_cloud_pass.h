// gs_cloud_pass.h -- private to the editor passes over the resident cloud: gs_edit.hip, gs_export.hip, gs_adjust.hip, gs_cply.hip and
// gs_transform.hip include it, no other file does.  What those passes share, once: the wave and workgroup reductions, the state filter, the rule a
// selection ends in, the stable compaction (count -> offsets -> scatter over a predicate) and the host sequences around them.
// None of this is a per-frame path.  The frame kernels (gs_render.hip, gs_sort.hip, gs_prims.hip, gs_pack.hip, gs_frame.hip) keep
// their own helpers on purpose: their DPP / NW-templated reductions are tuned for the frame and are not these.
#pragma once
#include "gs_lanes.h"

namespace {

#define GS_EDIT_IPT 8u                                           // the compaction's items per thread: consecutive ones (a thread's items keep their order)
#define GS_EDIT_CHUNK (GS_EDIT_IPT * GS_BLOCK)                   // ... and per workgroup
#define GS_EDIT_GRID 2048u                                       // workgroups at most for the grid-strided editing kernels

// ---- a wave's sum, minimum and maximum in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
template <typename T> __device__ __forceinline__ T wave_min(T v)  // (u32 and f64; a NaN compares false: it never wins)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const T o = __shfl_xor(v, m, 64); if (o < v) v = o; }
    return v;
}
template <typename T> __device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const T o = __shfl_xor(v, m, 64); if (o > v) v = o; }
    return v;
}
// one atomic per workgroup: every thread calls it (a barrier inside)
__device__ __forceinline__ void block_count(uint32_t mine, uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_w[GS_BLOCK / 64];
    const uint32_t t = wave_sum(mine);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) { const uint32_t s = s_w[0] + s_w[1] + s_w[2] + s_w[3]; if (s) atomicAdd(out, s); }
}
// exclusive scan of one value per thread over the workgroup (256 threads), in thread order; total: the sum (every thread calls it)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_w /* [GS_BLOCK / 64] */, uint32_t &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    __syncthreads();                                               // (s_w may still be read from the previous call)
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int k = 0; k < w; k++) base += s_w[k];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return base + inc - v;
}

// ---- the state filter: splat i takes part iff (state & mask) == value, its state 0 beyond the store's `rows` bytes.  rows = 0 when the
// mask is 0 or the store is empty (filter_rows): no byte is loaded then, and a store that was never allocated is never read
__device__ __forceinline__ bool state_passes(const uint8_t *__restrict__ state, uint32_t rows, uint32_t i, uint32_t mask, uint32_t value)
{
    const uint32_t st = i < rows ? (uint32_t)state[i] : 0u;
    return (st & mask) == value;
}
uint32_t filter_rows(const gs_ctx *ctx, uint8_t mask) { return (mask && ctx->edit_state) ? (uint32_t)ctx->edit_n : 0u; }

// ---- what a selection ends in: the splat is taken iff inside != invert, and a taken splat's byte becomes (byte & ~clear) | set
__device__ __forceinline__ bool take_if(bool inside, uint32_t invert, uint8_t *__restrict__ state, uint32_t i, uint32_t set, uint32_t clear)
{
    if (inside == (invert != 0u)) return false;
    state[i] = (uint8_t)((state[i] & ~clear) | set);
    return true;
}

// ---- stable compaction of the first n splats by a predicate: flags -> offsets -> scatter.  A workgroup owns GS_EDIT_CHUNK consecutive
// splats, a thread GS_EDIT_IPT consecutive ones.  The two predicates (plain structs, passed by value):
struct NotHidden {                                               // gs_compact: what stays
    const uint8_t *__restrict__ state; uint32_t rows;
    __device__ __forceinline__ bool operator()(uint32_t i) const { return state_passes(state, rows, i, GS_STATE_HIDDEN, 0u); }
};
struct StateFilter {                                             // the exports: what the caller's filter passes
    const uint8_t *__restrict__ state; uint32_t rows, mask, value;
    __device__ __forceinline__ bool operator()(uint32_t i) const { return state_passes(state, rows, i, mask, value); }
};
template <typename P>
__global__ __launch_bounds__(GS_BLOCK) void k_compact_count(P pred, uint32_t n, uint32_t *__restrict__ blk)
{
    __shared__ uint32_t s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    uint32_t c = 0;
    const uint32_t i0 = blockIdx.x * GS_EDIT_CHUNK + threadIdx.x * GS_EDIT_IPT;
    for (uint32_t j = 0; j < GS_EDIT_IPT; j++) c += (i0 + j < n && pred(i0 + j)) ? 1u : 0u;
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s_c;
}
// one workgroup: blk[0, nblk) -> their exclusive sums in place, blk[nblk] = the total.  (Not a template: gs_adjust.hip, gs_transform.hip and gs_cply.hip,
// which launch no compaction, carry an unused copy of it in their code objects -- a few hundred bytes, accepted)
__global__ __launch_bounds__(GS_BLOCK) void k_compact_offsets(uint32_t *__restrict__ blk, uint32_t nblk)
{
    __shared__ uint32_t s_w[GS_BLOCK / 64];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += GS_BLOCK) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < nblk ? blk[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan(v, s_w, total);
        if (b < nblk) blk[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) blk[nblk] = carry;
}
// what every scatter starts from: the new index of this thread's first passing splat, and which of its splats pass (bit j: splat i0 + j).
// Every thread of the workgroup calls it (barriers inside); k + passing <= blk[nblk], which is what the outputs hold
template <typename P>
__device__ __forceinline__ uint32_t compact_slot(P pred, uint32_t n, const uint32_t *__restrict__ blk, uint32_t &i0, uint32_t &take)
{
    __shared__ uint32_t s_w[GS_BLOCK / 64];
    i0 = blockIdx.x * GS_EDIT_CHUNK + threadIdx.x * GS_EDIT_IPT;
    take = 0;
#pragma unroll
    for (uint32_t j = 0; j < GS_EDIT_IPT; j++) take |= (i0 + j < n && pred(i0 + j)) ? (1u << j) : 0u;
    uint32_t total;
    return blk[blockIdx.x] + block_excl_scan((uint32_t)__popc(take), s_w, total);
}
// count and offsets on stream st: *blk (allocated here, the caller's to free) [0, nblk) = where each workgroup's splats begin, [nblk] =
// the passing splats; total (may be null: the caller reads that word behind its own scatter) = the same on the host, the stream idle
template <typename P> int compact_offsets(gs_ctx *ctx, hipStream_t st, P pred, uint32_t n, uint32_t **blk, size_t *total)
{
    const uint32_t nblk = gs_div_up(n, GS_EDIT_CHUNK);
    TRY(dev_alloc(ctx, blk, (size_t)nblk + 1));
    hipLaunchKernelGGL(k_compact_count<P>, dim3(nblk), dim3(GS_BLOCK), 0, st, pred, n, *blk);
    hipLaunchKernelGGL(k_compact_offsets, dim3(1), dim3(GS_BLOCK), 0, st, *blk, nblk);
    if (!total) return GS_OK;
    GS_HIP(hipGetLastError());
    uint32_t t = 0;
    GS_HIP(hipMemcpyAsync(&t, *blk + nblk, sizeof t, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    *total = t;
    return GS_OK;
}

// ---- host sequences
// workgroups of a grid-strided pass over `items`: one per GS_BLOCK of them, at least one, at most `cap`
uint32_t pass_grid(uint64_t items, uint32_t cap = GS_EDIT_GRID)
{
    const uint64_t g = (items + GS_BLOCK - 1) / GS_BLOCK;
    return g > cap ? cap : (uint32_t)(g ? g : 1);
}
// the reading passes' stream (made once): they wait for their own kernels and copies alone
int reading_stream(gs_ctx *ctx)
{
    GS_HIP(hipSetDevice(ctx->device));
    if (!ctx->prop_stream) GS_HIP(hipStreamCreateWithFlags(&ctx->prop_stream, hipStreamNonBlocking));
    return GS_OK;
}
// the two device words the editing kernels count into (made once), cleared on the owner's stream; and the first one read back, the
// stream idle behind it
int counters(gs_ctx *ctx)
{
    if (!ctx->edit_cnt) GS_HIP(hipMalloc((void **)&ctx->edit_cnt, 2 * sizeof(uint32_t)));
    GS_HIP(hipMemsetAsync(ctx->edit_cnt, 0, 2 * sizeof(uint32_t), ctx->stream));
    return GS_OK;
}
int read_counter(gs_ctx *ctx, size_t *out)
{
    uint32_t v = 0;
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(&v, ctx->edit_cnt, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    GS_HIP(hipStreamSynchronize(ctx->stream));
    if (out) *out = v;
    return GS_OK;
}
// after a change of the resident splats or their states, as after a push: no lane's order survives, and a sort begun before the
// change is run again when it is collected
void drop_orders(gs_ctx *ctx)
{
    for (int i = 0; i < GS_MAX_LANES; i++) if (ctx->lanes[i]) ctx->lanes[i]->have_sort = false;
    if (ctx->pend_lane > 0) ctx->pend_n = (size_t)-1;
}

}  // namespace

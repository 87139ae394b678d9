// gs_edit.hip -- editing the resident cloud (include/gs_splat.h: "editing the resident cloud"): the kernels behind the per-splat state
// store -- counting, id lists, region selection (box, sphere, screen rectangle, mask image), selection by a property's value and the
// properties' histogram and range -- and the stable compaction of gs_compact.
//
// None of this is a per-frame path: every kernel is one streaming pass over the rows (or over the order), its counts go to two device
// words through one atomic per workgroup, and every launcher waits for its kernel and hands the count back on the host.  What a frame
// pays for a state store is ONE byte load per splat in the depth pass (gs_sort.hip: the HID instantiations).
// (The two reading passes, gs_prop_range and gs_histogram, run on a stream of their own and wait for their kernel alone.)
// Behind the launchers: the entry points of the C ABI that call them (gs_set_state ... gs_compact).
#include "gs_lanes.h"
#include "gs_sh.h"
#include "gs_cloud_pass.h"

namespace {

// Earlier versions of the tests read these two names out of THIS file.  The constants live in gs_cloud_pass.h; the lines below restate
// them token for token, and one that differs does not compile
#pragma clang diagnostic error "-Wmacro-redefined"
#define GS_EDIT_IPT 8u
#define GS_EDIT_GRID 2048u

__global__ __launch_bounds__(GS_BLOCK) void k_edit_count_hidden(const uint8_t *__restrict__ state, uint32_t n, uint32_t *__restrict__ out)
{
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) c += state[i] & GS_STATE_HIDDEN;
    block_count(c, out);
}

// (a duplicate id: both threads write the value the rule gives -- the rule is idempotent)
__global__ __launch_bounds__(GS_BLOCK) void k_edit_apply_ids(uint8_t *__restrict__ state, uint32_t rows, const uint32_t *__restrict__ ids, uint32_t n,
                                                             uint32_t set, uint32_t clear)
{
    for (uint32_t k = blockIdx.x * GS_BLOCK + threadIdx.x; k < n; k += gridDim.x * GS_BLOCK) {
        const uint32_t id = ids[k];
        if (id < rows) state[id] = (uint8_t)((state[id] & ~clear) | set);
    }
}

struct BoxUniforms { double c[16]; int affine; };                 // widened on the host (exact), as gs_sort.hip's SortUniforms
__global__ __launch_bounds__(GS_BLOCK) void k_edit_select_box(const float4 *__restrict__ rows, uint32_t n, BoxUniforms b, uint8_t *__restrict__ state,
                                                              uint32_t set, uint32_t clear, uint32_t invert, uint32_t *__restrict__ hit)
{
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        const float4 m = rows[i];
        // the depth pass' own test (index.js:526-545)
        const bool inside = b.affine ? gsm::in_cutout_affine(b.c, m.x, m.y, m.z) : gsm::in_cutout(b.c, m.x, m.y, m.z);
        c += take_if(inside, invert, state, i, set, clear);
    }
    block_count(c, hit);
}

__global__ __launch_bounds__(GS_BLOCK) void k_edit_select_sphere(const uint4 *__restrict__ splat, uint32_t n, double cx, double cy, double cz, double r2,
                                                                 uint8_t *__restrict__ state, uint32_t set, uint32_t clear, uint32_t invert, uint32_t *__restrict__ hit)
{
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        const uint4 cs = splat[2 * (size_t)i];                       // the packed centre (x, y, -z): index.js:350-354
        const double dx = (double)__uint_as_float(cs.x) - cx, dy = (double)__uint_as_float(cs.y) - cy, dz = (double)(-__uint_as_float(cs.z)) - cz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;             // (un-fused: the library is built with -ffp-contract=off)
        c += take_if(d2 <= r2, invert, state, i, set, clear);       // (NaN: outside)
    }
    block_count(c, hit);
}

// ---- the two selections made on the screen: one walk over the whole order, the centre projected by the frame's own function, then a test
// of the centre's pixel.  The rectangle, clipped to the frame; hm1 = fb_height - 1
struct ScreenUniforms { float mv[16], proj[16]; float focal, vw, vh; };
struct InRect {
    float x0, y0, x1, y1, hm1;
    __device__ __forceinline__ bool operator()(const gsm::Projected &p, const gsm::ProjExtra &) const
    {
        const float px = floorf(p.cx), py = hm1 - floorf(p.cy);      // GL rows (y up) -> image rows (top-down); NaN compares false
        return px >= x0 && px < x1 && py >= y0 && py < y1;
    }
};
// A mask image: one byte per pixel, tight rows of W, row 0 = top (non-zero = inside), and an optional plane of window depths, tight too: a
// position is taken iff its centre's pixel lies in the frame, the mask is set there and -- with a plane -- the depth k_project writes to
// zwin is <= the plane's value there (a NaN on either side: not taken)
struct InMask {
    int32_t W, H; const uint8_t *__restrict__ mask; const float *__restrict__ depth_max;
    __device__ __forceinline__ bool operator()(const gsm::Projected &p, const gsm::ProjExtra &x) const
    {
        const float fx = floorf(p.cx), fy = floorf(p.cy);
        if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) return false;   // (NaN compares false; inside the frame: exact integers)
        const size_t px = (size_t)(H - 1 - (int32_t)fy) * (size_t)W + (size_t)(int32_t)fx;   // GL rows (y up) -> image rows (top-down)
        return mask[px] != 0 && (!depth_max || x.zndc * 0.5f + 0.5f <= depth_max[px]);       // k_project's zwin
    }
};
template <bool PAR, typename T>
__global__ __launch_bounds__(GS_BLOCK) void k_edit_select_screen(const uint32_t *__restrict__ sorted, const GsControl *__restrict__ ctl, uint32_t n,
                                                                 const uint4 *__restrict__ splat, ScreenUniforms u, T test, uint8_t *__restrict__ state,
                                                                 uint32_t set, uint32_t clear, uint32_t invert, uint32_t *__restrict__ hit)
{
    const uint32_t V = ctl->n_kept < n ? ctl->n_kept : n;           // the whole order: V positions, every value an index below n
    uint32_t c = 0;
    for (uint32_t j = blockIdx.x * GS_BLOCK + threadIdx.x; j < V; j += gridDim.x * GS_BLOCK) {
        const uint32_t idx = sorted[j];
        if (idx >= n) continue;
        const uint4 cs4 = splat[2 * (size_t)idx], cc4 = splat[2 * (size_t)idx + 1];
        const float cs[4] = { __uint_as_float(cs4.x), __uint_as_float(cs4.y), __uint_as_float(cs4.z), __uint_as_float(cs4.w) };
        const uint32_t cc[4] = { cc4.x, cc4.y, cc4.z, cc4.w };
        gsm::Projected p; gsm::ProjExtra x;
        // what k_project<.., PAR> calls, with the frame's uniforms
        const bool inside = gsm::project_splat<PAR>(cs, cc, u.mv, u.proj, u.focal, u.vw, u.vh, p, x) && test(p, x);
        c += take_if(inside, invert, state, idx, set, clear);
    }
    block_count(c, hit);
}

// ---- gs_compact: the shared compaction (gs_cloud_pass.h) over NotHidden, and the scatter of every resident array
__global__ __launch_bounds__(GS_BLOCK) void k_compact_scatter(NotHidden kept, uint32_t n, const uint32_t *__restrict__ blk,
                                                              const uint4 *__restrict__ splat, const float4 *__restrict__ sort_rows, const float *__restrict__ bound_r,
                                                              uint32_t renderable, uint4 *__restrict__ o_splat, float4 *__restrict__ o_rows, float *__restrict__ o_bound,
                                                              uint8_t *__restrict__ o_state, uint32_t *__restrict__ o_old)
{
    uint32_t i0, take;
    uint32_t k = compact_slot(kept, n, blk, i0, take);              // the new index of this thread's first kept splat (k + kept < blk[nblk] <= n)
#pragma unroll
    for (uint32_t j = 0; j < GS_EDIT_IPT; j++) {
        if (!((take >> j) & 1u)) continue;
        const uint32_t i = i0 + j;
        if (renderable) { o_splat[2 * (size_t)k] = splat[2 * (size_t)i]; o_splat[2 * (size_t)k + 1] = splat[2 * (size_t)i + 1]; }
        o_rows[k] = sort_rows[i];
        o_bound[k] = bound_r[i];
        o_state[k] = i < kept.rows ? kept.state[i] : (uint8_t)0;    // (the hidden bit is clear: the splat was kept)
        o_old[k] = i;
        k++;
    }
}
// the SH rows of the kept splats among those that have one: new row k < sh_kept is old row old[k] (a prefix stays a prefix: stable order)
__global__ __launch_bounds__(GS_BLOCK) void k_compact_sh(const uint4 *__restrict__ sh, const uint32_t *__restrict__ old, uint32_t sh_kept, uint32_t sh_n, uint32_t row_q,
                                                         uint4 *__restrict__ o_sh)
{
    const size_t words = (size_t)sh_kept * row_q;
    for (size_t t = (size_t)blockIdx.x * GS_BLOCK + threadIdx.x; t < words; t += (size_t)gridDim.x * GS_BLOCK) {
        const uint32_t k = (uint32_t)(t / row_q), q = (uint32_t)(t % row_q);
        const uint32_t i = old[k];
        if (i < sh_n) o_sh[t] = sh[(size_t)i * row_q + q];
    }
}

// ... and their words of the contribution store, by the same rule
__global__ __launch_bounds__(GS_BLOCK) void k_compact_contrib(const unsigned long long *__restrict__ store, const uint32_t *__restrict__ old, uint32_t kept, uint32_t rows,
                                                              unsigned long long *__restrict__ o_store)
{
    for (uint32_t k = blockIdx.x * GS_BLOCK + threadIdx.x; k < kept; k += gridDim.x * GS_BLOCK) {
        const uint32_t i = old[k];
        if (i < rows) o_store[k] = store[i];
    }
}

// ---- per-splat properties (gs_splat.h: gs_prop_range / gs_histogram / gs_select_range).  One streaming pass each, grid-strided in whole
// workgroup steps (every lane of a wave stays in the loop until the workgroup leaves it: the wave-wide votes below see all 64 lanes).
// CC: the property reads the second half of the record (colour bytes, SIZE2); the position properties cost one 16-byte load per splat.
template <bool CC> __device__ __forceinline__ double prop_load(const uint4 *__restrict__ splat, uint32_t i, int prop)
{
    const uint4 cs4 = splat[2 * (size_t)i];
    uint4 cc4 = make_uint4(0u, 0u, 0u, 0u);
    if (CC) cc4 = splat[2 * (size_t)i + 1];
    const float cs[4] = { __uint_as_float(cs4.x), __uint_as_float(cs4.y), __uint_as_float(cs4.z), __uint_as_float(cs4.w) };
    const uint32_t cc[4] = { cc4.x, cc4.y, cc4.z, cc4.w };
    return gsm::prop_value(cs, cc, prop);
}
// GS_PROP_SEEN is no function of the record: the splat's word of the contribution store (gs_frame.hip) in pixels, 0 beyond the store's
// length -- exact below 2^53.  SEEN instantiations of the three kernels below take the store and its length and load nothing else; the
// <false> and <true> kernels are what they were.  (No new ordering: the store is written by synchronous contribution frames only, which
// have returned before a property call is made -- on prop_stream or the owner's.)
typedef const unsigned long long *__restrict__ SeenStore;
template <bool CC, bool SEEN> __device__ __forceinline__ double prop_load_any(const uint4 *__restrict__ splat, uint32_t i, int prop, SeenStore seen, uint32_t seen_n)
{
    if (SEEN) return i < seen_n ? (double)seen[i] / 65536.0 : 0.0;
    return prop_load<CC>(splat, i, prop);
}
template <bool CC, bool SEEN>
__device__ __forceinline__ void prop_select_body(const uint4 *__restrict__ splat, uint32_t n, int prop, double lo, double hi, uint8_t *__restrict__ state,
                                                 uint32_t set, uint32_t clear, uint32_t invert, uint32_t *__restrict__ hit, SeenStore seen, uint32_t seen_n)
{
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        const double v = prop_load_any<CC, SEEN>(splat, i, prop, seen, seen_n);
        c += take_if(lo <= v && v <= hi, invert, state, i, set, clear);   // (NaN: outside)
    }
    block_count(c, hit);
}
template <bool CC>
__global__ __launch_bounds__(GS_BLOCK) void k_prop_select(const uint4 *__restrict__ splat, uint32_t n, int prop, double lo, double hi, uint8_t *__restrict__ state,
                                                          uint32_t set, uint32_t clear, uint32_t invert, uint32_t *__restrict__ hit)
{
    prop_select_body<CC, false>(splat, n, prop, lo, hi, state, set, clear, invert, hit, nullptr, 0u);
}
__global__ __launch_bounds__(GS_BLOCK) void k_prop_select_seen(SeenStore seen, uint32_t seen_n, uint32_t n, double lo, double hi, uint8_t *__restrict__ state,
                                                               uint32_t set, uint32_t clear, uint32_t invert, uint32_t *__restrict__ hit)
{
    prop_select_body<false, true>(nullptr, n, GS_PROP_SEEN, lo, hi, state, set, clear, invert, hit, seen, seen_n);
}

// Per-workgroup partials, reduced on the host (as the depth pass' range: no f64 atomics on one address): part[blockIdx.x] = { min, max }
// of the non-NaN values of the workgroup's passing splats (+inf, -inf where it saw none), cnt[blockIdx.x] = its passing splats.
template <bool CC, bool SEEN>
__device__ __forceinline__ void prop_range_body(const uint4 *__restrict__ splat, uint32_t n, int prop, const uint8_t *__restrict__ state, uint32_t rows,
                                                uint32_t mask, uint32_t value, double2 *__restrict__ part, uint32_t *__restrict__ cnt, SeenStore seen, uint32_t seen_n)
{
    __shared__ double s_mn[GS_BLOCK / 64], s_mx[GS_BLOCK / 64];
    __shared__ uint32_t s_c[GS_BLOCK / 64];
    double mn = INFINITY, mx = -INFINITY;
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += gridDim.x * GS_BLOCK) {
        if (!state_passes(state, rows, i, mask, value)) continue;
        const double v = prop_load_any<CC, SEEN>(splat, i, prop, seen, seen_n);
        c++;
        if (v < mn) mn = v;                                          // (a NaN compares false twice)
        if (v > mx) mx = v;
    }
    mn = wave_min(mn); mx = wave_max(mx); c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; s_c[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < GS_BLOCK / 64; w++) { if (s_mn[w] < mn) mn = s_mn[w]; if (s_mx[w] > mx) mx = s_mx[w]; c += s_c[w]; }
        part[blockIdx.x] = make_double2(mn, mx);
        cnt[blockIdx.x] = c;
    }
}
template <bool CC>
__global__ __launch_bounds__(GS_BLOCK) void k_prop_range(const uint4 *__restrict__ splat, uint32_t n, int prop, const uint8_t *__restrict__ state, uint32_t rows,
                                                         uint32_t mask, uint32_t value, double2 *__restrict__ part, uint32_t *__restrict__ cnt)
{
    prop_range_body<CC, false>(splat, n, prop, state, rows, mask, value, part, cnt, nullptr, 0u);
}
__global__ __launch_bounds__(GS_BLOCK) void k_prop_range_seen(SeenStore seen, uint32_t seen_n, uint32_t n, const uint8_t *__restrict__ state, uint32_t rows,
                                                              uint32_t mask, uint32_t value, double2 *__restrict__ part, uint32_t *__restrict__ cnt)
{
    prop_range_body<false, true>(nullptr, n, GS_PROP_SEEN, state, rows, mask, value, part, cnt, seen, seen_n);
}

// The histogram: ONE table of nbins words in LDS per workgroup, cleared at the start and added to global memory at the end with one
// atomic per non-empty bin, and equal bins of a wave COMBINED BEFORE they touch LDS.  Of the two ways to survive a pile-up (most alpha
// bytes of a trained scene are 255: all 64 lanes of a wave want one word) this one was chosen because the pile-up is INSIDE a wave: the
// 64 adds of one LDS instruction on one address are taken one after the other whichever table they go to, so a table per wave
// changes nothing about them -- and four tables of 4096 words are the whole 64 KB of static LDS, with no room left for the tally.
// Combining: up to GS_HIST_PEEL times, the first lane that still holds a bin names it, a vote finds every lane holding the same one, and
// the first lane adds their number once.  A wave whose lanes agree is done after one round and one add; where the values are spread,
// the rounds cost a few scalar instructions each and the lanes left over add 1 each, to words that are then mostly different.
// out: nbins counts, then { passing, below, above, NaN }.
#define GS_HIST_PEEL 4
template <bool CC, bool SEEN>
__device__ __forceinline__ void prop_hist_body(const uint4 *__restrict__ splat, uint32_t n, int prop, double lo, double hi, double scale, uint32_t nbins,
                                               const uint8_t *__restrict__ state, uint32_t rows, uint32_t mask, uint32_t value, uint32_t *__restrict__ out,
                                               SeenStore seen, uint32_t seen_n)
{
    __shared__ uint32_t s_h[GS_HIST_MAX_BINS];
    __shared__ uint32_t s_t[4];
    for (uint32_t b = threadIdx.x; b < nbins; b += GS_BLOCK) s_h[b] = 0;
    if (threadIdx.x < 4) s_t[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    uint32_t passing = 0, below = 0, above = 0, nan = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * GS_BLOCK; base < n; base += (uint64_t)gridDim.x * GS_BLOCK) {
        const uint64_t i64 = base + threadIdx.x;
        const uint32_t i = (uint32_t)(i64 < n ? i64 : n);            // (i == n: no splat)
        int32_t bin = -4;                                            // not a passing splat
        if (i < n && state_passes(state, rows, i, mask, value)) bin = gsm::hist_bin(prop_load_any<CC, SEEN>(splat, i, prop, seen, seen_n), lo, hi, scale, nbins);
        passing += bin != -4; below += bin == -1; above += bin == -2; nan += bin == -3;
        unsigned long long todo = __ballot(bin >= 0);
        for (int r = 0; r < GS_HIST_PEEL && todo; r++) {
            const int first = __ffsll(todo) - 1;
            const int32_t fb = __shfl(bin, first, 64);                // (>= 0: the lane was named by the vote)
            const unsigned long long same = __ballot(bin == fb);
            if (lane == first) atomicAdd(&s_h[fb], (uint32_t)__popcll(same));
            if (bin == fb) bin = -4;
            todo &= ~same;
        }
        if (bin >= 0) atomicAdd(&s_h[bin], 1u);
    }
    passing = wave_sum(passing); below = wave_sum(below); above = wave_sum(above); nan = wave_sum(nan);
    if (lane == 0) {
        if (passing) atomicAdd(&s_t[0], passing);
        if (below) atomicAdd(&s_t[1], below);
        if (above) atomicAdd(&s_t[2], above);
        if (nan) atomicAdd(&s_t[3], nan);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbins; b += GS_BLOCK) { const uint32_t c = s_h[b]; if (c) atomicAdd(&out[b], c); }
    if (threadIdx.x < 4 && s_t[threadIdx.x]) atomicAdd(&out[nbins + threadIdx.x], s_t[threadIdx.x]);
}
template <bool CC>
__global__ __launch_bounds__(GS_BLOCK) void k_prop_hist(const uint4 *__restrict__ splat, uint32_t n, int prop, double lo, double hi, double scale, uint32_t nbins,
                                                        const uint8_t *__restrict__ state, uint32_t rows, uint32_t mask, uint32_t value, uint32_t *__restrict__ out)
{
    prop_hist_body<CC, false>(splat, n, prop, lo, hi, scale, nbins, state, rows, mask, value, out, nullptr, 0u);
}
__global__ __launch_bounds__(GS_BLOCK) void k_prop_hist_seen(SeenStore seen, uint32_t seen_n, uint32_t n, double lo, double hi, double scale, uint32_t nbins,
                                                             const uint8_t *__restrict__ state, uint32_t rows, uint32_t mask, uint32_t value, uint32_t *__restrict__ out)
{
    prop_hist_body<false, true>(nullptr, n, GS_PROP_SEEN, lo, hi, scale, nbins, state, rows, mask, value, out, seen, seen_n);
}

// what gs_edit_select_rect and gs_edit_select_mask do alike, around their test of a pixel
template <typename T> int select_screen(gs_ctx *ctx, gs_ctx *L, const GsFrameUniforms &f, T test, uint8_t set, uint8_t clear, bool invert, size_t *hit)
{
    TRY(counters(ctx));
    ScreenUniforms u;
    memcpy(u.mv, f.mv, sizeof u.mv); memcpy(u.proj, f.proj, sizeof u.proj);
    u.focal = f.focal; u.vw = f.vw; u.vh = f.vh;
    // (the uploads and the counters went to the owner's stream, which is otherwise idle -- the lanes were drained; the lane's stream holds the order)
    GS_HIP(hipStreamSynchronize(ctx->stream));
    gs_flag((f.flags & GS_RENDER_PARALLEL) != 0, [&](auto PAR) {   // (the camera model of the frame, as launch_project picks k_project's)
        hipLaunchKernelGGL((k_edit_select_screen<decltype(PAR)::value, T>), dim3(pass_grid(ctx->n)), dim3(GS_BLOCK), 0, L->stream, (const uint32_t *)L->sorted,
                           (const GsControl *)L->ctl, (uint32_t)ctx->n, (const uint4 *)ctx->splat, u, test, ctx->edit_state, (uint32_t)set, (uint32_t)clear,
                           invert ? 1u : 0u, ctx->edit_cnt);
    });
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(L->stream));
    return read_counter(ctx, hit);
}

}  // namespace

int gs_edit_count_hidden(gs_ctx *ctx, const uint8_t *state, size_t n, size_t *out)
{
    *out = 0;
    if (!n) return GS_OK;
    int rc = counters(ctx);
    if (rc != GS_OK) return rc;
    hipLaunchKernelGGL(k_edit_count_hidden, dim3(pass_grid(n)), dim3(GS_BLOCK), 0, ctx->stream, state, (uint32_t)n, ctx->edit_cnt);
    return read_counter(ctx, out);
}

int gs_edit_apply_ids(gs_ctx *ctx, const uint32_t *ids_dev, size_t n, uint8_t set, uint8_t clear)
{
    if (!n) return GS_OK;
    hipLaunchKernelGGL(k_edit_apply_ids, dim3(pass_grid(n)), dim3(GS_BLOCK), 0, ctx->stream, ctx->edit_state, (uint32_t)ctx->edit_n, ids_dev, (uint32_t)n,
                       (uint32_t)set, (uint32_t)clear);
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(ctx->stream));
    return GS_OK;
}

int gs_edit_select_box(gs_ctx *ctx, const float box16[16], uint8_t set, uint8_t clear, bool invert, size_t *hit)
{
    int rc = counters(ctx);
    if (rc != GS_OK) return rc;
    BoxUniforms b;
    for (int i = 0; i < 16; i++) b.c[i] = (double)box16[i];
    b.affine = (b.c[3] == 0.0 && b.c[7] == 0.0 && b.c[11] == 0.0 && b.c[15] == 1.0) ? 1 : 0;   // (gs_sort.hip: fill_sort_uniforms)
    hipLaunchKernelGGL(k_edit_select_box, dim3(pass_grid(ctx->n)), dim3(GS_BLOCK), 0, ctx->stream, (const float4 *)ctx->sort_rows, (uint32_t)ctx->n, b,
                       ctx->edit_state, (uint32_t)set, (uint32_t)clear, invert ? 1u : 0u, ctx->edit_cnt);
    return read_counter(ctx, hit);
}

int gs_edit_select_sphere(gs_ctx *ctx, const float centre[3], float radius, uint8_t set, uint8_t clear, bool invert, size_t *hit)
{
    int rc = counters(ctx);
    if (rc != GS_OK) return rc;
    const double r2 = (double)radius * (double)radius;
    hipLaunchKernelGGL(k_edit_select_sphere, dim3(pass_grid(ctx->n)), dim3(GS_BLOCK), 0, ctx->stream, (const uint4 *)ctx->splat, (uint32_t)ctx->n,
                       (double)centre[0], (double)centre[1], (double)centre[2], r2, ctx->edit_state, (uint32_t)set, (uint32_t)clear, invert ? 1u : 0u, ctx->edit_cnt);
    return read_counter(ctx, hit);
}

int gs_edit_select_range(gs_ctx *ctx, int prop, double lo, double hi, uint8_t set, uint8_t clear, bool invert, size_t *hit)
{
    int rc = counters(ctx);
    if (rc != GS_OK) return rc;
    if (prop == GS_PROP_SEEN)
        hipLaunchKernelGGL(k_prop_select_seen, dim3(pass_grid(ctx->n)), dim3(GS_BLOCK), 0, ctx->stream, (const unsigned long long *)ctx->contrib, (uint32_t)ctx->contrib_n,
                           (uint32_t)ctx->n, lo, hi, ctx->edit_state, (uint32_t)set, (uint32_t)clear, invert ? 1u : 0u, ctx->edit_cnt);
    else gs_flag(gsm::prop_reads_cc(prop), [&](auto CC) {
        hipLaunchKernelGGL((k_prop_select<decltype(CC)::value>), dim3(pass_grid(ctx->n)), dim3(GS_BLOCK), 0, ctx->stream, (const uint4 *)ctx->splat,
                           (uint32_t)ctx->n, prop, lo, hi, ctx->edit_state, (uint32_t)set, (uint32_t)clear, invert ? 1u : 0u, ctx->edit_cnt);
    });
    return read_counter(ctx, hit);
}

// the reading passes' stream and device words (made once), the words cleared on that stream
static int prop_begin(gs_ctx *ctx, size_t clear_bytes)
{
    TRY(reading_stream(ctx));
    if (!ctx->prop_buf) GS_HIP(hipMalloc(&ctx->prop_buf, GS_PROP_BUF_BYTES));
    if (clear_bytes) GS_HIP(hipMemsetAsync(ctx->prop_buf, 0, clear_bytes, ctx->prop_stream));
    return GS_OK;
}

int gs_prop_run_range(gs_ctx *ctx, int prop, uint8_t mask, uint8_t value, double *mn, double *mx, size_t *n)
{
    const uint32_t grid = pass_grid(ctx->n);                       // (grid x (16 + 4) bytes <= GS_PROP_BUF_BYTES)
    static_assert(GS_EDIT_GRID * (sizeof(double2) + sizeof(uint32_t)) <= GS_PROP_BUF_BYTES, "the partials fit the buffer");
    int rc = prop_begin(ctx, 0);
    if (rc != GS_OK) return rc;
    double2 *part = reinterpret_cast<double2 *>(ctx->prop_buf);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(part + GS_EDIT_GRID);
    if (prop == GS_PROP_SEEN)
        hipLaunchKernelGGL(k_prop_range_seen, dim3(grid), dim3(GS_BLOCK), 0, ctx->prop_stream, (const unsigned long long *)ctx->contrib, (uint32_t)ctx->contrib_n, (uint32_t)ctx->n,
                           (const uint8_t *)ctx->edit_state, filter_rows(ctx, mask), (uint32_t)mask, (uint32_t)value, part, cnt);
    else gs_flag(gsm::prop_reads_cc(prop), [&](auto CC) {
        hipLaunchKernelGGL((k_prop_range<decltype(CC)::value>), dim3(grid), dim3(GS_BLOCK), 0, ctx->prop_stream, (const uint4 *)ctx->splat, (uint32_t)ctx->n, prop,
                           (const uint8_t *)ctx->edit_state, filter_rows(ctx, mask), (uint32_t)mask, (uint32_t)value, part, cnt);
    });
    GS_HIP(hipGetLastError());
    std::vector<double2> hp(grid);
    std::vector<uint32_t> hc(grid);
    GS_HIP(hipMemcpyAsync(hp.data(), part, grid * sizeof(double2), hipMemcpyDeviceToHost, ctx->prop_stream));
    GS_HIP(hipMemcpyAsync(hc.data(), cnt, grid * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->prop_stream));
    GS_HIP(hipStreamSynchronize(ctx->prop_stream));
    double lo = INFINITY, hi = -INFINITY;
    size_t c = 0;
    for (uint32_t b = 0; b < grid; b++) { if (hp[b].x < lo) lo = hp[b].x; if (hp[b].y > hi) hi = hp[b].y; c += hc[b]; }
    *mn = lo; *mx = hi; *n = c;
    return GS_OK;
}

int gs_prop_run_histogram(gs_ctx *ctx, int prop, double lo, double hi, double scale, uint32_t nbins, uint8_t mask, uint8_t value, uint32_t *counts, uint64_t tally[4])
{
    static_assert((GS_HIST_MAX_BINS + 4) * sizeof(uint32_t) <= GS_PROP_BUF_BYTES, "the counts fit the buffer");
    int rc = prop_begin(ctx, ((size_t)nbins + 4) * sizeof(uint32_t));
    if (rc != GS_OK) return rc;
    uint32_t *out = reinterpret_cast<uint32_t *>(ctx->prop_buf);
    if (prop == GS_PROP_SEEN)
        hipLaunchKernelGGL(k_prop_hist_seen, dim3(pass_grid(ctx->n)), dim3(GS_BLOCK), 0, ctx->prop_stream, (const unsigned long long *)ctx->contrib, (uint32_t)ctx->contrib_n,
                           (uint32_t)ctx->n, lo, hi, scale, nbins, (const uint8_t *)ctx->edit_state, filter_rows(ctx, mask), (uint32_t)mask, (uint32_t)value, out);
    else gs_flag(gsm::prop_reads_cc(prop), [&](auto CC) {
        hipLaunchKernelGGL((k_prop_hist<decltype(CC)::value>), dim3(pass_grid(ctx->n)), dim3(GS_BLOCK), 0, ctx->prop_stream, (const uint4 *)ctx->splat,
                           (uint32_t)ctx->n, prop, lo, hi, scale, nbins, (const uint8_t *)ctx->edit_state, filter_rows(ctx, mask), (uint32_t)mask, (uint32_t)value, out);
    });
    GS_HIP(hipGetLastError());
    uint32_t t[4];
    GS_HIP(hipMemcpyAsync(counts, out, (size_t)nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->prop_stream));
    GS_HIP(hipMemcpyAsync(t, out + nbins, sizeof t, hipMemcpyDeviceToHost, ctx->prop_stream));
    GS_HIP(hipStreamSynchronize(ctx->prop_stream));
    for (int k = 0; k < 4; k++) tally[k] = t[k];
    return GS_OK;
}

int gs_edit_select_rect(gs_ctx *ctx, gs_ctx *L, const GsFrameUniforms &f, const int32_t rect[4], uint8_t set, uint8_t clear, bool invert, size_t *hit)
{
    const int32_t x0 = rect[0] > 0 ? rect[0] : 0, y0 = rect[1] > 0 ? rect[1] : 0;
    const int32_t x1 = rect[2] < f.W ? rect[2] : f.W, y1 = rect[3] < f.H ? rect[3] : f.H;
    const InRect test = { (float)x0, (float)y0, (float)x1, (float)y1, (float)(f.H - 1) };
    return select_screen(ctx, L, f, test, set, clear, invert, hit);
}

int gs_edit_select_mask(gs_ctx *ctx, gs_ctx *L, const GsFrameUniforms &f, const uint8_t *mask_dev, const float *depth_dev, uint8_t set, uint8_t clear,
                        bool invert, size_t *hit)
{
    const InMask test = { f.W, f.H, mask_dev, depth_dev };
    return select_screen(ctx, L, f, test, set, clear, invert, hit);
}

int gs_edit_compact(gs_ctx *ctx, const GsCompactTo &to, size_t *kept)
{
    const uint32_t n = (uint32_t)ctx->n, nblk = gs_div_up(n, GS_EDIT_CHUNK);
    const NotHidden pred = { ctx->edit_state, (uint32_t)ctx->edit_n };
    hipStream_t st = ctx->stream;
    uint32_t *blk = nullptr;
    TRY(compact_offsets(ctx, st, pred, n, &blk, nullptr));       // (the total is read behind the scatter: one wait for the three kernels)
    hipLaunchKernelGGL(k_compact_scatter, dim3(nblk), dim3(GS_BLOCK), 0, st, pred, n, (const uint32_t *)blk,
                       (const uint4 *)ctx->splat, (const float4 *)ctx->sort_rows, (const float *)ctx->bound_r, ctx->renderable ? 1u : 0u,
                       to.splat, to.sort_rows, to.bound_r, to.state, to.old_index);
    uint32_t total = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&total, blk + nblk, sizeof total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(blk);
    if (e != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "gs_compact failed: %s", hipGetErrorString(e)); return GS_E_HIP; }
    *kept = total;
    return GS_OK;
}

// ... and the contribution store's words of the kept splats among those that have one: new word k < kept = old word to.old_index[k]
int gs_edit_compact_contrib(gs_ctx *ctx, const uint32_t *old_index, size_t kept, unsigned long long *to)
{
    if (!kept) return GS_OK;
    hipLaunchKernelGGL(k_compact_contrib, dim3(pass_grid(kept)), dim3(GS_BLOCK), 0, ctx->stream, (const unsigned long long *)ctx->contrib, old_index, (uint32_t)kept,
                       (uint32_t)ctx->contrib_n, to);
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(ctx->stream));
    return GS_OK;
}

// (separate: the number of SH rows that stay is known on the host only after the scatter)
int gs_edit_compact_sh(gs_ctx *ctx, const GsCompactTo &to, size_t sh_words, size_t sh_kept)
{
    if (!sh_kept || !to.sh) return GS_OK;
    hipLaunchKernelGGL(k_compact_sh, dim3(pass_grid(sh_kept * sh_words)), dim3(GS_BLOCK), 0, ctx->stream, (const uint4 *)ctx->sh, (const uint32_t *)to.old_index,
                       (uint32_t)sh_kept, (uint32_t)ctx->sh_n, (uint32_t)sh_words, reinterpret_cast<uint4 *>(to.sh));
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(ctx->stream));
    return GS_OK;
}

// ---- editing the resident cloud (include/gs_splat.h; kernels: above).  The state store is the owner's, like the SH store; a sort
// is handed the pointer and the length when it is launched (gs_sort.hip: run_sort), so the lanes hold nothing.
// Before a change: every lane idle (frames in flight read the store; drain_all marks logged frames stale), the allocation in place, and
// the store grown to `rows` -- the bytes behind the old length are zero (the allocation is zero-filled, and whoever shortens the store
// clears what it gives up).
static int edit_begin(gs_ctx *ctx, size_t rows)
{
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    TRY(edit_ensure_alloc(ctx));
    if (rows > ctx->edit_n) ctx->edit_n = rows;
    return GS_OK;
}
// after a change: the hidden count, and no lane's order survives (as after a push)
static int edit_end(gs_ctx *ctx)
{
    drop_orders(ctx);
    return gs_edit_count_hidden(ctx, ctx->edit_state, ctx->edit_n, &ctx->edit_hidden);
}

// one change of the store: `fn` between edit_begin and edit_end; its failure goes before the count's
template <typename F> static int edit_apply(gs_ctx *ctx, size_t rows, F fn)
{
    TRY(edit_begin(ctx, rows));
    const int rc = fn();
    const int rc2 = edit_end(ctx);
    return rc != GS_OK ? rc : rc2;
}

// gs_select_rect / gs_select_mask (`name`): the arguments both take (`what`: the rectangle, the mask) and the full-width frame the
// selection is made in ...
static int screen_select_begin(gs_ctx *ctx, const gs_render_params *p, const void *what, uint32_t flags, const char *name, GsFrameUniforms &u)
{
    if (!p || !what) FAIL(GS_E_BADARG, "%s: NULL argument", name);
    if (flags & ~GS_SELECT_INVERT) FAIL(GS_E_BADARG, "%s: unknown flags %#x", name, flags);
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "context was fed worker matrices only (gs_push_matrices): it can sort but not project");
    gs_render_params q = *p;
    q.x0 = 0; q.x1 = p->fb_width;
    return gs_fill_uniforms(ctx, &q, u);
}
// ... and, every lane idle, the WHOLE order on the current frame's lane: a near-only or a strip sort is run again in full first (what
// gs_download(GS_BUF_SORTED) does for the former)
static int screen_select_order(gs_ctx *ctx, const char *name, gs_ctx **lane)
{
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));                                         // (the current frame's lane is idle and its have_sort is the worker's last word)
    gs_ctx *L = *lane = ctx->lanes[ctx->cur];
    if (!ctx->n || !L->have_sort || !L->sorted) FAIL(GS_E_STATE, "%s: no completed sort to select from", name);
    if (L->sort_near_req || L->sv_has_strip) TRY(lane_rc(ctx, L, gs_run_sort(L, L->sv_view, L->sv_has_cutout ? L->sv_cutout : nullptr, nullptr, 0)));
    return GS_OK;
}

// gs_select_mask's inputs on the device, in the owner's grow-only scratch, on its stream: the mask as tight rows of W bytes and -- 256-byte
// aligned behind it, at depth_at -- the depth plane.  An editor action, not a frame path: pageable memory, one copy each
static int mask_upload(gs_ctx *ctx, const uint8_t *mask, size_t stride, const float *depth_max, size_t W, size_t H, size_t depth_at)
{
    const size_t need = depth_at + (depth_max ? W * H * sizeof(float) : 0);
    if (need > ctx->mask_cap_bytes) {
        dev_free(ctx->mask_buf); ctx->mask_buf = nullptr; ctx->mask_cap_bytes = 0;
        TRY(dev_alloc(ctx, &ctx->mask_buf, need));
        ctx->mask_cap_bytes = need;
    }
    if (stride == W) GS_HIP(hipMemcpyAsync(ctx->mask_buf, mask, W * H, hipMemcpyHostToDevice, ctx->stream));
    else GS_HIP(hipMemcpy2DAsync(ctx->mask_buf, W, mask, stride, W, H, hipMemcpyHostToDevice, ctx->stream));
    if (depth_max) GS_HIP(hipMemcpyAsync(ctx->mask_buf + depth_at, depth_max, W * H * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return GS_OK;
}

extern "C" {

GS_API int gs_set_state(gs_ctx *ctx, size_t first, const uint8_t *states, size_t n)
{
    CHECK_CTX(ctx);
    if (first > ctx->n || n > ctx->n - first) FAIL(GS_E_BADARG, "gs_set_state: states [%zu, %zu) of %zu splats", first, first + n, ctx->n);
    if (n == 0) return GS_OK;
    if (!states) FAIL(GS_E_BADARG, "gs_set_state: states is NULL");
    TRY(edit_begin(ctx, first + n));
    GS_HIP(hipMemcpy(ctx->edit_state + first, states, n, hipMemcpyHostToDevice));
    return edit_end(ctx);
}

GS_API int gs_set_state_ids(gs_ctx *ctx, const uint32_t *ids, size_t n, uint8_t set_bits, uint8_t clear_bits)
{
    CHECK_CTX(ctx);
    if (n == 0) return GS_OK;
    if (!ids) FAIL(GS_E_BADARG, "gs_set_state_ids: ids is NULL");
    for (size_t k = 0; k < n; k++) if (ids[k] >= ctx->n) FAIL(GS_E_BADARG, "gs_set_state_ids: id %u (entry %zu) of %zu splats", ids[k], k, ctx->n);
    TRY(edit_begin(ctx, ctx->n));
    uint32_t *dev = nullptr;
    TRY(dev_alloc(ctx, &dev, n));
    int rc = GS_OK;
    const hipError_t e = hipMemcpy(dev, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "upload failed: %s", hipGetErrorString(e)); rc = GS_E_HIP; }
    if (rc == GS_OK) rc = gs_edit_apply_ids(ctx, dev, n, set_bits, clear_bits);
    dev_free(dev);
    const int rc2 = edit_end(ctx);
    return rc != GS_OK ? rc : rc2;
}

GS_API int gs_state_count(const gs_ctx *ctx, size_t *rows, size_t *hidden)
{
    if (!ctx) return GS_E_BADARG;
    if (rows) *rows = ctx->edit_n;
    if (hidden) *hidden = ctx->edit_hidden;
    return GS_OK;
}

GS_API int gs_select_box(gs_ctx *ctx, const float box16[16], uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit)
{
    CHECK_CTX(ctx);
    if (!box16) FAIL(GS_E_BADARG, "gs_select_box: box16 is NULL");
    if (flags & ~GS_SELECT_INVERT) FAIL(GS_E_BADARG, "gs_select_box: unknown flags %#x", flags);
    if (out_hit) *out_hit = 0;
    if (!ctx->n) return GS_OK;
    return edit_apply(ctx, ctx->n, [&] { return gs_edit_select_box(ctx, box16, set_bits, clear_bits, (flags & GS_SELECT_INVERT) != 0, out_hit); });
}

GS_API int gs_select_sphere(gs_ctx *ctx, const float centre[3], float radius, uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit)
{
    CHECK_CTX(ctx);
    if (!centre) FAIL(GS_E_BADARG, "gs_select_sphere: centre is NULL");
    if (flags & ~GS_SELECT_INVERT) FAIL(GS_E_BADARG, "gs_select_sphere: unknown flags %#x", flags);
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "context was fed worker matrices only (gs_push_matrices): no positions in the rows' space");
    if (out_hit) *out_hit = 0;
    if (!ctx->n) return GS_OK;
    return edit_apply(ctx, ctx->n, [&] { return gs_edit_select_sphere(ctx, centre, radius, set_bits, clear_bits, (flags & GS_SELECT_INVERT) != 0, out_hit); });
}

// what the three property calls refuse alike
static int prop_check(gs_ctx *ctx, int prop, const char *name)
{
    if (prop != GS_PROP_SEEN && !gsm::prop_valid(prop)) FAIL(GS_E_BADARG, "%s: unknown property %d", name, prop);   // (SEEN: the contribution store, no function of the record)
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "context was fed worker matrices only (gs_push_matrices): it holds no packed records");
    return GS_OK;
}

GS_API int gs_select_range(gs_ctx *ctx, int prop, double lo, double hi, uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit)
{
    CHECK_CTX(ctx);
    if (lo != lo || hi != hi) FAIL(GS_E_BADARG, "gs_select_range: a bound is NaN");
    if (flags & ~GS_SELECT_INVERT) FAIL(GS_E_BADARG, "gs_select_range: unknown flags %#x", flags);
    TRY(prop_check(ctx, prop, "gs_select_range"));
    if (out_hit) *out_hit = 0;
    if (!ctx->n) return GS_OK;
    return edit_apply(ctx, ctx->n, [&] { return gs_edit_select_range(ctx, prop, lo, hi, set_bits, clear_bits, (flags & GS_SELECT_INVERT) != 0, out_hit); });
}

GS_API int gs_prop_range(gs_ctx *ctx, int prop, uint8_t state_mask, uint8_t state_value, double *out_min, double *out_max, size_t *out_n)
{
    CHECK_CTX(ctx);
    if (!out_min && !out_max && !out_n) FAIL(GS_E_BADARG, "gs_prop_range: no output");
    TRY(prop_check(ctx, prop, "gs_prop_range"));
    double mn = INFINITY, mx = -INFINITY;
    size_t n = 0;
    if (ctx->n) TRY(gs_prop_run_range(ctx, prop, state_mask, state_value, &mn, &mx, &n));
    if (out_min) *out_min = mn;
    if (out_max) *out_max = mx;
    if (out_n) *out_n = n;
    return GS_OK;
}

GS_API int gs_histogram(gs_ctx *ctx, int prop, double lo, double hi, uint32_t nbins, uint8_t state_mask, uint8_t state_value, uint32_t *counts, uint64_t tally[4])
{
    CHECK_CTX(ctx);
    int32_t bin;
    if (!counts) FAIL(GS_E_BADARG, "gs_histogram: counts is NULL");
    if (gs_hist_bin(lo, lo, hi, nbins, &bin) != GS_OK) FAIL(GS_E_BADARG, "gs_histogram: lo < hi, both finite, and 1 .. %d bins expected", GS_HIST_MAX_BINS);
    TRY(prop_check(ctx, prop, "gs_histogram"));
    uint64_t t[4] = { 0, 0, 0, 0 };
    memset(counts, 0, (size_t)nbins * sizeof(uint32_t));
    if (ctx->n) TRY(gs_prop_run_histogram(ctx, prop, lo, hi, (double)nbins / (hi - lo), nbins, state_mask, state_value, counts, t));
    if (tally) memcpy(tally, t, sizeof t);
    return GS_OK;
}

GS_API int gs_select_rect(gs_ctx *ctx, const gs_render_params *p, const int32_t rect[4], uint8_t set_bits, uint8_t clear_bits, uint32_t flags, size_t *out_hit)
{
    CHECK_CTX(ctx);
    GsFrameUniforms u;
    gs_ctx *L = nullptr;
    TRY(screen_select_begin(ctx, p, rect, flags, "gs_select_rect", u));
    if (out_hit) *out_hit = 0;
    TRY(screen_select_order(ctx, "gs_select_rect", &L));
    return edit_apply(ctx, ctx->n, [&] { return gs_edit_select_rect(ctx, L, u, rect, set_bits, clear_bits, (flags & GS_SELECT_INVERT) != 0, out_hit); });
}

GS_API int gs_select_mask(gs_ctx *ctx, const gs_render_params *p, const uint8_t *mask, size_t mask_stride, const float *depth_max, uint8_t set_bits,
                          uint8_t clear_bits, uint32_t flags, size_t *out_hit)
{
    CHECK_CTX(ctx);
    GsFrameUniforms u;
    gs_ctx *L = nullptr;
    TRY(screen_select_begin(ctx, p, mask, flags, "gs_select_mask", u));
    const size_t W = (size_t)u.W, H = (size_t)u.H;
    if (mask_stride && mask_stride < W) FAIL(GS_E_BADARG, "gs_select_mask: stride %zu smaller than a row (%zu bytes)", mask_stride, W);
    if (out_hit) *out_hit = 0;
    TRY(screen_select_order(ctx, "gs_select_mask", &L));
    return edit_apply(ctx, ctx->n, [&] {
        const size_t depth_at = (W * H + 255) & ~(size_t)255;
        int rc = mask_upload(ctx, mask, mask_stride ? mask_stride : W, depth_max, W, H, depth_at);
        if (rc == GS_OK) rc = gs_edit_select_mask(ctx, L, u, ctx->mask_buf, depth_max ? reinterpret_cast<const float *>(ctx->mask_buf + depth_at) : nullptr, set_bits,
                                                  clear_bits, (flags & GS_SELECT_INVERT) != 0, out_hit);
        if (rc != GS_OK) (void)hipStreamSynchronize(ctx->stream);     // (no copy out of the caller's memory is left behind)
        return rc;
    });
}

GS_API int gs_highlight_info(const gs_ctx *ctx, uint32_t *option_value, uint32_t *last_frame)
{
    if (!ctx) return GS_E_BADARG;
    if (option_value) *option_value = ctx->hl_opt;
    if (last_frame) {
        gs_ctx *c = const_cast<gs_ctx *>(ctx);
        for (int i = 0; i < GS_MAX_LANES; i++) if (c->lanes[i]) (void)lane_drain(c->lanes[i]);   // (as gs_get_stats: what the workers were handed is settled)
        *last_frame = c->lanes[c->cur]->hl_frame;
    }
    return GS_OK;
}

GS_API int gs_projection_info(const gs_ctx *ctx, uint32_t *last_frame_parallel)
{
    if (!ctx) return GS_E_BADARG;
    if (last_frame_parallel) {
        gs_ctx *c = const_cast<gs_ctx *>(ctx);
        for (int i = 0; i < GS_MAX_LANES; i++) if (c->lanes[i]) (void)lane_drain(c->lanes[i]);   // (as gs_highlight_info)
        *last_frame_parallel = c->lanes[c->cur]->par_frame;
    }
    return GS_OK;
}

GS_API int gs_compact(gs_ctx *ctx, uint32_t *out_old_index, size_t *out_n)
{
    CHECK_CTX(ctx);
    if (out_n) *out_n = ctx->n;
    if (!ctx->edit_hidden) {                                     // nothing hidden: nothing to do
        if (out_old_index) for (size_t k = 0; k < ctx->n; k++) out_old_index[k] = (uint32_t)k;
        return GS_OK;
    }
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    // fresh arrays of the same capacity (the resident bytes are held twice until the swap below)
    const size_t sh_q = ctx->sh_n ? 3 * (size_t)gsm::sh_channel_stride(ctx->sh_deg) / 4 : 0;   // 16-byte words per SH row
    GsCompactTo to = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    int rc = dev_alloc(ctx, &to.splat, ctx->cap * 2);
    if (rc == GS_OK) rc = dev_alloc(ctx, &to.sort_rows, ctx->cap);
    if (rc == GS_OK) rc = dev_alloc(ctx, &to.bound_r, ctx->cap);
    if (rc == GS_OK) rc = dev_alloc(ctx, &to.state, ctx->edit_cap);
    if (rc == GS_OK) rc = dev_alloc(ctx, &to.old_index, ctx->n);
    if (rc == GS_OK && sh_q) rc = dev_alloc(ctx, &to.sh, ctx->sh_cap * sh_q * 4);
    if (rc == GS_OK && hipMemset(to.state, 0, ctx->edit_cap) != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "gs_compact: clearing the new state store failed"); rc = GS_E_HIP; }
    // how many of the splats that have an SH row are hidden (the store ends at or before gs_count(): bytes beyond it are state 0)
    size_t sh_hidden = 0, kept = 0, seen_hidden = 0;
    unsigned long long *to_seen = nullptr;                       // the contribution store moves along like the states (both halves of its allocation: gs_frame.hip)
    if (rc == GS_OK && ctx->contrib_n) rc = dev_alloc(ctx, &to_seen, 2 * ctx->contrib_cap);
    if (rc == GS_OK && to_seen && hipMemset(to_seen, 0, ctx->contrib_cap * sizeof(unsigned long long)) != hipSuccess) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "gs_compact: clearing the new contribution store failed"); rc = GS_E_HIP; }
    if (rc == GS_OK && to_seen) rc = gs_edit_count_hidden(ctx, ctx->edit_state, ctx->contrib_n < ctx->edit_n ? ctx->contrib_n : ctx->edit_n, &seen_hidden);
    if (rc == GS_OK && sh_q) rc = gs_edit_count_hidden(ctx, ctx->edit_state, ctx->sh_n < ctx->edit_n ? ctx->sh_n : ctx->edit_n, &sh_hidden);
    if (rc == GS_OK) rc = gs_edit_compact(ctx, to, &kept);
    if (rc == GS_OK && sh_q) rc = gs_edit_compact_sh(ctx, to, sh_q, ctx->sh_n - sh_hidden);
    if (rc == GS_OK && to_seen) rc = gs_edit_compact_contrib(ctx, to.old_index, ctx->contrib_n - seen_hidden, to_seen);
    if (rc == GS_OK && kept != ctx->n - ctx->edit_hidden) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "gs_compact: kept %zu splats, expected %zu", kept, ctx->n - ctx->edit_hidden); rc = GS_E_HIP; }
    if (rc == GS_OK && out_old_index && kept && hipMemcpy(out_old_index, to.old_index, kept * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
        snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "gs_compact: download of the index map failed"); rc = GS_E_HIP;
    }
    if (rc != GS_OK) {
        dev_free(to.splat); dev_free(to.sort_rows); dev_free(to.bound_r); dev_free(to.state); dev_free(to.old_index); dev_free(to.sh); dev_free(to_seen);
        return rc;
    }
    dev_free(ctx->splat); dev_free(ctx->sort_rows); dev_free(ctx->bound_r); dev_free(ctx->edit_state); dev_free(to.old_index);
    ctx->splat = to.splat; ctx->sort_rows = to.sort_rows; ctx->bound_r = to.bound_r; ctx->edit_state = to.state;
    if (sh_q) { dev_free(ctx->sh); ctx->sh = to.sh; ctx->sh_n -= sh_hidden; }
    if (to_seen) { dev_free(ctx->contrib); ctx->contrib = to_seen; ctx->contrib_n -= seen_hidden; }
    ctx->edit_n -= ctx->edit_hidden; ctx->edit_hidden = 0;       // (every hidden splat lay inside the store; stable order: a prefix stays a prefix)
    ctx->n = kept; ctx->stats.n_splats = kept;
    if (!kept) { ctx->renderable = true; ctx->sh_n = 0; ctx->sh_deg = 0; }   // (an empty context, as after gs_clear)
    reset_cloud_measurements(ctx);
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (!L) continue;
        L->have_sort = false; L->sorted = nullptr;
        memset(&L->stats, 0, sizeof L->stats);
    }
    ctx->stats.n_splats = kept;
    refresh_lanes(ctx);
    set_current_lane(ctx, 0, 0);
    // a sort posted before the call: run again over the kept splats when it is collected (as after any other edit); nothing kept: the
    // empty context's reply [0] is owed (index.js:588-590)
    if (ctx->pend_lane > 0) { if (kept) ctx->pend_n = (size_t)-1; else ctx->pend_lane = -1; }
    if (out_n) *out_n = kept;
    return GS_OK;
}

}  // extern "C"

// gs_sort.hip -- the worker's sortSplats (index.js:507-570) as HIP kernels.
//
// Bit-exact contract: view depth, min/max and the bucket scale are IEEE f64 evaluated
// left to right without FMA (library is built -ffp-contract=off); only the stored depth is rounded to
// f32; the result is ordered by (bucket, original index).  The 17-bit key (16-bit bucket + one value for dropped
// buckets) is sorted by two stable radix passes of 8 + 9 bits.  Culled splats leave in pass A (GS_RADIX_SKIP records are
// neither counted nor scattered), so pass B runs over the V kept splats.  Kept splats whose bucket falls outside
// [0,65535] (f32 rounding of the stored depth >> depth range) carry key 65536, sort behind every bucket and store 0 --
// exactly like the reference's out-of-bounds typed-array writes leave 0 in the tail [V',V) of its result.
#include "gs_internal.h"
#include "gs_strip_uniforms.h"

namespace {

struct SortUniforms {                                            // widened on the host (exact): scalar registers
    double view[4]; double cutout[16]; int has_cutout;          // has_cutout 2: the matrix is affine (last row 0 0 0 1): gsm::in_cutout_affine
    int has_strip;
};
// gs_sort_for: rows 0, 1, 2 of gsModelViewMatrix, rows 0, 3 of gsProjectionMatrix, and the strip in pixels
// the per-splat state store (gs_set_state ...; gs_edit.hip): a splat whose byte has GS_STATE_HIDDEN counts as outside the cutout.  Read by the
// HID instantiations only -- a context whose store is empty launches the others, which never look at it
struct HiddenArgs { const uint8_t *state; uint32_t rows; };      // rows: the store's length (<= n; the allocation holds n bytes at least)
using gsm::StripUniforms;                                        // (gs_device_math.h, with the reach test gsm::strip_may_touch)
// the depth kernel's chunking is its own (no histogram depends on it)
#ifndef GS_DEPTH_IPT
#define GS_DEPTH_IPT 4             // items per thread and pass: 52 vector registers, 8 waves per SIMD (8 items: 92, 5 waves)
#endif
#ifndef GS_DEPTH_GRID
#define GS_DEPTH_GRID 2048u        // workgroups at most (one partial min/max/count slot each)
#endif

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m)
{
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl_xor(lo, m, 64); hi = __shfl_xor(hi, m, 64);
    return ((unsigned long long)hi << 32) | lo;
}
// min / max of two doubles that are not NaN, one instruction each (the builtins first canonicalise both operands: three more)
__device__ __forceinline__ double min_f64(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double max_f64(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double shfl_xor_f64(double v, int m)
{
    return __longlong_as_double((long long)shfl_xor_u64((unsigned long long)__double_as_longlong(v), m));
}

// Near-only sorts (gs_run_sort with near_req): the pass also histograms the kept depths by the top 11 bits of the stored f32
// |depth| (kept depths are negative, so the sign-less bit pattern grows with the distance: exponent + 3 mantissa bits, 12 %
// steps); k_sort_bucket derives from it a bucket below which no splat can be among the nearest near_req.  Workgroups add
// their LDS histogram to one of GS_DH_COPIES global copies (same-address atomics serialise at ~11 ns: 2048 workgroups on one
// copy cost 22 us).  (Measured and dropped: the workgroup that finishes last reducing the copies to the threshold itself --
// the release / acquire fences that takes across the 8 XCDs' L2s cost 70 us per sort.)
// fill: this sort's histogram (nullptr: none wanted); zero: the one the lane's previous near-only sort filled, cleared here
// (its reader finished long ago: stream order); zero_word: the control block's count of valid buckets, recounted by k_sort_bucket.
struct DepthHist { uint32_t *fill, *zero, *zero_word; uint32_t *zero_grp; uint32_t zero_grp_words; };   // zero_grp: the MSD sort's group rows (below), cleared for k_sort_bucket<.., MSD>'s atomics
__device__ __forceinline__ uint32_t depth_bin(float d) { return (__float_as_uint(d) & 0x7FFFFFFFu) >> 20; }
__device__ __forceinline__ void depth_hist_begin(const DepthHist &dh, uint32_t *s_dh)
{
    if (dh.fill) for (uint32_t d = threadIdx.x; d < GS_DEPTH_BINS; d += GS_BLOCK) s_dh[d] = 0;
    if (blockIdx.x == 0) {
        if (dh.zero) for (uint32_t d = threadIdx.x; d < GS_DH_WORDS / 4u; d += GS_BLOCK) reinterpret_cast<uint4 *>(dh.zero)[d] = make_uint4(0, 0, 0, 0);
        if (dh.zero_word && threadIdx.x == 0) *dh.zero_word = 0;
        if (dh.zero_grp) for (uint32_t d = threadIdx.x; d < dh.zero_grp_words / 4u; d += GS_BLOCK) reinterpret_cast<uint4 *>(dh.zero_grp)[d] = make_uint4(0, 0, 0, 0);
    }
}
// (after a barrier that follows the last LDS atomic)  Two levels: the bins, and behind them sums over 32 consecutive bins each
// (GS_DEPTH_COARSE = 64 words per copy), so that a reader finds the bin it wants with ~800 loads instead of all 16 K words
__device__ __forceinline__ void depth_hist_end(const DepthHist &dh, const uint32_t *s_dh)
{
    if (!dh.fill) return;
    const uint32_t cp = blockIdx.x % GS_DH_COPIES;
    uint32_t *fine = dh.fill + cp * GS_DEPTH_BINS, *coarse = dh.fill + GS_DH_COPIES * GS_DEPTH_BINS + cp * GS_DEPTH_COARSE;
    for (uint32_t d = threadIdx.x; d < GS_DEPTH_BINS; d += GS_BLOCK) {
        const uint32_t v = s_dh[d];
        if (v) atomicAdd(&fine[d], v);
        uint32_t t = v;                                              // lanes 0..31 / 32..63 of a wave hold 32 consecutive bins
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
        if ((threadIdx.x & 31u) == 0u && t) atomicAdd(&coarse[d >> 5], t);
    }
}

// pass 1 (index.js:517-555): depth, culls, f64 min/max of survivors.  16 B/splat in, 4 B/splat out.
// Each workgroup leaves its (min, max, count) in a partial slot; no global atomics.
// (the strip test of gs_sort_for: gsm::strip_may_touch, gs_device_math.h)

// SPEC (near-only sorts of long inputs, round 4): the pass hands the candidates on itself.  A near-only sort keeps the splats whose
// bucket reaches a threshold that is only known after the pass (it comes from this pass' depth histogram and min / max) -- so the
// depths of all N splats were written (80 MB at 20 M) and read again by k_near_stash, which recomputed 20 M buckets in f64 to keep
// 1.5 % of them.  But the threshold BIN moves slowly from frame to frame: with the bin the context's last near-only sort found
// (*bin_hint) plus GS_SPEC_PAD the pass stashes every splat whose depth falls in those bins -- (stored f32 depth, index), in index
// order, GS_SPEC_SLOT records per chunk of 1024 -- and writes no depth array at all; k_near_filter then applies the EXACT rule to
// the candidates alone (same f32 depth, same min / max, same bucket arithmetic: the same records as before) after checking that
// the candidates were a superset of what the exact threshold keeps.  If they were not (the camera jumped; a stash overflowed; the
// depth range is so short that buckets could be dropped, which only a pass over every depth can count), the frame is flagged like
// an overflowed stash: drawn again from a whole sort, and the hint is exact for the next frame.
#ifndef GS_SPEC_SLOT
#define GS_SPEC_SLOT 128u          // candidates a 1024-item chunk of the depth pass may stash (the share asked for is <= 1/32: 32 on average)
#endif
#ifndef GS_SPEC_PAD
#define GS_SPEC_PAD 2u             // bins (12 % of depth each) beyond the last sort's threshold bin that are stashed too (one is needed when the bin
                                   // has not moved: the threshold BUCKET lies inside the next bin; the second is the margin for a moving camera)
#endif
#define GS_SPEC_GROUP 32u          // chunks (of 1024 items) one k_near_filter workgroup compacts: 4096 stash slots

// What belongs to ONE view of the pass: its uniforms, where its depths, partials and histogram go, and (SPEC) its stash
struct DepthView {
    SortUniforms u; StripUniforms su;
    float *depth; unsigned long long *part_min, *part_max; uint32_t *part_cnt; DepthHist dh;
    uint2 *stash; uint32_t *cnt; const uint32_t *bin_hint; GsControl *ctl;     // SPEC: candidates, per-chunk counts, the threshold-bin hint
};
template <int NV> struct DepthViews { DepthView v[NV]; };        // the views of one sweep over the splats
// ... and what a thread carries for one view: min / max / count of what it kept, and (SPEC) the chunk's depth bits and stash flags
struct DepthAcc { double mn, mx; uint32_t cnt, lim, rec; uint32_t fb[GS_DEPTH_IPT]; bool sp[GS_DEPTH_IPT]; };
constexpr uint32_t GS_DEPTH_CHUNK = GS_DEPTH_IPT * GS_BLOCK;     // this pass' own chunking (no histogram depends on it)

// item r of a chunk (splat i: row m, bound sigma; shown = not hidden) as view v sees it
template <bool STRIP, bool SPEC>
__device__ __forceinline__ void depth_view_step(const DepthView &v, const float4 m, float sigma, bool shown, uint32_t i, int r, uint32_t *s_dh, DepthAcc &a)
{
    const double d = gsm::view_depth(v.u.view, m.x, m.y, m.z);
    // a hidden splat is a splat outside the cutout (index.js:548)
    const bool inside = shown && (v.u.has_cutout ? (v.u.has_cutout == 2 ? gsm::in_cutout_affine(v.u.cutout, m.x, m.y, m.z) : gsm::in_cutout(v.u.cutout, m.x, m.y, m.z)) : true);
    const bool keep = gsm::sort_keep(d, m.w, inside);
    // the bucket scale comes from EVERY splat the reference keeps (index.js:552-553), so a strip's order is the
    // reference's order restricted to the strip's splats; only those are handed on
    const bool mine = keep && (!STRIP || gsm::strip_may_touch(v.su, m.x, m.y, m.z, sigma));
    if (!SPEC) v.depth[i] = mine ? (float)d : INFINITY;
    if (mine && v.dh.fill) atomicAdd(&s_dh[depth_bin((float)d)], 1u);
    if (SPEC) { a.fb[r] = __float_as_uint((float)d); a.sp[r] = mine && depth_bin((float)d) <= a.lim; }
    if (keep) {
        a.mn = min_f64(a.mn, d); a.mx = max_f64(a.mx, d);
        if (mine) a.cnt++;
    }
}

// the stash step of chunk c for one view: ranks by (row, wavefront, lane) = index order
__device__ __forceinline__ void spec_stash_step(const DepthView &v, const DepthAcc &a, uint32_t c, uint32_t *s_srow)
{
    uint32_t bef[GS_DEPTH_IPT];
#pragma unroll
    for (int r = 0; r < GS_DEPTH_IPT; r++) {
        const unsigned long long bal = __ballot(a.sp[r]);
        bef[r] = (uint32_t)__popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull));
        if ((threadIdx.x & 63) == 0) s_srow[r * 4 + (threadIdx.x >> 6)] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const uint32_t cv = threadIdx.x < 4u * GS_DEPTH_IPT ? s_srow[threadIdx.x] : 0u;
        uint32_t inc = cv;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d, 64); if ((int)threadIdx.x >= d) inc += t; }
        if (threadIdx.x < 4u * GS_DEPTH_IPT) s_srow[threadIdx.x] = inc - cv;
        const uint32_t total = __shfl(inc, 63, 64);
        if (threadIdx.x == 0) {
            v.cnt[c] = (total < GS_SPEC_SLOT ? total : GS_SPEC_SLOT) | (a.rec << 16);   // the bins THIS chunk was stashed by: checked per chunk
            if (total > GS_SPEC_SLOT) v.ctl->spec_fail = 2u;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GS_DEPTH_IPT; r++) {
        if (a.sp[r]) {
            const uint32_t slot = s_srow[r * 4 + (threadIdx.x >> 6)] + bef[r];
            if (slot < GS_SPEC_SLOT) v.stash[(size_t)c * GS_SPEC_SLOT + slot] = make_uint2(a.fb[r], c * GS_DEPTH_CHUNK + r * GS_BLOCK + threadIdx.x);
        }
    }
    __syncthreads();
}

// The pass for NV views in ONE sweep over the splats: rows, bounds and state bytes are loaded once per item, then every view takes its
// step.  NV = 2 is the two frames of a pair (GS_OPT_FRAME_BATCH): at 20 M splats the sort rows are 320 MB of the 400 MB this pass
// streams per frame, and both frames read the same rows -- one read, two view rows / cutout matrices, two depth arrays and two sets
// of partials (20 M @ 4K: 2464 -> 2606 frames/s; no difference at 1 M, where the rows are cache-resident).
// (instantiations: the strip test / the stash / the state bytes must not cost the plain sort registers)
template <int NV, bool STRIP, bool SPEC, bool HID>
__device__ __forceinline__ void k_sort_depth_body(const float4 *__restrict__ rows, const float *__restrict__ bound_r, uint32_t n, const DepthViews<NV> &vs, HiddenArgs hid)
{
    __shared__ unsigned long long s_min[NV], s_max[NV];
    __shared__ uint32_t s_cnt[NV];
    __shared__ uint32_t s_srow[NV][SPEC ? 4 * GS_DEPTH_IPT : 1];
    extern __shared__ uint32_t s_dh[];                           // GS_DEPTH_BINS words per view for a near-only sort, none otherwise (LDS the other frames' blends can use)
    // min / max of the kept depths as doubles (kept depths are finite and negative: sort_keep), encoded once per wavefront at the end
    // -- on the ordered-u64 encoding a splat cost two 64-bit compares and four selects
    DepthAcc acc[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        // the bins this workgroup stashes: up to the last sort's threshold bin + pad.  The hint is one word shared by the context's lanes
        // and may change while this kernel runs: every chunk records the limit it was stashed by, and the filter checks chunk by chunk
        const uint32_t hint = SPEC ? *vs.v[k].bin_hint : 0u;
        acc[k].lim = (SPEC && hint != 0xFFFFFFFFu) ? hint + GS_SPEC_PAD : 0u;
        acc[k].rec = (SPEC && hint != 0xFFFFFFFFu) ? acc[k].lim : 0xFFFFu;
        acc[k].mn = INFINITY; acc[k].mx = -INFINITY; acc[k].cnt = 0;
        depth_hist_begin(vs.v[k].dh, s_dh + k * GS_DEPTH_BINS);
    }
    if (threadIdx.x < NV) { s_min[threadIdx.x] = ~0ull; s_max[threadIdx.x] = 0ull; s_cnt[threadIdx.x] = 0; }
    __syncthreads();
    const uint32_t nchunks = (n + GS_DEPTH_CHUNK - 1) / GS_DEPTH_CHUNK;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        float4 mm[GS_DEPTH_IPT];                                     // all loads first: their latencies overlap
        float sg[GS_DEPTH_IPT];
        uint8_t hs[HID ? GS_DEPTH_IPT : 1];
#pragma unroll
        for (int r = 0; r < GS_DEPTH_IPT; r++) {
            const uint32_t i = c * GS_DEPTH_CHUNK + r * GS_BLOCK + threadIdx.x;
            // (unconditional, the index clamped: a conditional load put each item's wait and f64 conversions into its own branch, so the
            // four loads of a thread went out one after the other; items beyond n are dropped below)
            const uint32_t ic = i < n ? i : n - 1u;
            mm[r] = rows[ic];
            sg[r] = STRIP ? bound_r[ic] : 0.0f;
            if (HID) hs[r] = hid.state[ic];                              // (with the rows: same index, same clamp)
        }
#pragma unroll
        for (int k = 0; k < NV; k++) {
#pragma unroll
            for (int r = 0; r < GS_DEPTH_IPT; r++) { acc[k].fb[r] = 0u; acc[k].sp[r] = false; }
        }
#pragma unroll
        for (int r = 0; r < GS_DEPTH_IPT; r++) {
            const uint32_t i = c * GS_DEPTH_CHUNK + r * GS_BLOCK + threadIdx.x;
            if (i < n) {
                const bool shown = !(HID && i < hid.rows && (hs[r] & GS_STATE_HIDDEN));   // (one state load for all views)
#pragma unroll
                for (int k = 0; k < NV; k++) depth_view_step<STRIP, SPEC>(vs.v[k], mm[r], sg[r], shown, i, r, s_dh + k * GS_DEPTH_BINS, acc[k]);
            }
        }
        if (SPEC) {
#pragma unroll
            for (int k = 0; k < NV; k++) spec_stash_step(vs.v[k], acc[k], c, s_srow[k]);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {                           // wavefront butterfly, then one LDS atomic per wave and view
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const double omn = shfl_xor_f64(acc[k].mn, m), omx = shfl_xor_f64(acc[k].mx, m);
            acc[k].mn = omn < acc[k].mn ? omn : acc[k].mn; acc[k].mx = omx > acc[k].mx ? omx : acc[k].mx;
            acc[k].cnt += __shfl_xor(acc[k].cnt, m, 64);
        }
    }
#pragma unroll
    for (int k = 0; k < NV; k++) {
        if ((threadIdx.x & 63) == 0 && acc[k].mx > -INFINITY) {   // (the wave kept something)
            atomicMin(&s_min[k], gsm::f64_to_ordered(acc[k].mn)); atomicMax(&s_max[k], gsm::f64_to_ordered(acc[k].mx)); atomicAdd(&s_cnt[k], acc[k].cnt);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; k++) {
        if (threadIdx.x == 0) { vs.v[k].part_min[blockIdx.x] = s_min[k]; vs.v[k].part_max[blockIdx.x] = s_max[k]; vs.v[k].part_cnt[blockIdx.x] = s_cnt[k]; }
        depth_hist_end(vs.v[k].dh, s_dh + k * GS_DEPTH_BINS);
    }
}

// one view per sweep: a single frame, and -- twinned by gs_launch<2, ..> -- the frames of a short pair (run_sort)
template <bool STRIP, bool SPEC, bool HID>
__global__ __launch_bounds__(GS_BLOCK) void k_sort_depth(const float4 *__restrict__ rows, const float *__restrict__ bound_r, uint32_t n, DepthViews<1> vs, HiddenArgs hid)
{
    k_sort_depth_body<1, STRIP, SPEC, HID>(rows, bound_r, n, vs, hid);
}
// both views of a pair in one sweep
#ifndef GS_DEPTH_PAIR_MIN_N
#define GS_DEPTH_PAIR_MIN_N (1u << 22)   // paired sorts of fewer splats run k_sort_depth's body twice (run_sort<2>)
#endif
template <bool STRIP, bool SPEC, bool HID>
__global__ __launch_bounds__(GS_BLOCK) void k_sort_depth_pair(const float4 *__restrict__ rows, const float *__restrict__ bound_r, uint32_t n, DepthViews<2> vs, HiddenArgs hid)
{
    k_sort_depth_body<2, STRIP, SPEC, HID>(rows, bound_r, n, vs, hid);
}

// pass 2 (index.js:558-561): 16-bit bucket of the stored depth; culled -> GS_RADIX_SKIP, dropped bucket -> GS_CULLED_KEY.
// Every workgroup first folds pass 1's partials (<= 2048 slots, L2-resident) into the global min/max.  One workgroup per
// radix chunk (geometry NW as in gs_prims.hip): it also leaves radix pass A's histogram row of the chunk.
// COMPACT (N <= 2^25): pass A sorts by the low 9 bucket bits and writes 4-byte records `bucket >> 9 << 25 | index`, pass B
// by the 7 bits on top of the index: half the bytes of (key, index) records through three of the five streaming passes.
// A 17th key bit has no room there, so kept splats with a dropped bucket leave the sort here as well; the final pass
// zero-fills their slots [V', V) behind the sorted records (the reference's never-written tail).
// NEAR (a near-only sort, COMPACT records): only the splats that can be among the nearest near_req of the order go on.
// The depth histogram gives the first bin T with (kept splats in bins <= T) >= near_req; its far edge -e is a depth, b* = its
// bucket, and a splat goes on iff its bucket >= b*: the bucket is monotonic in the stored depth, so every splat nearer than
// the edge qualifies (at least near_req of them), and the rule is a threshold on the sort key itself -- the survivors are
// exactly the last P valid positions of the whole order, in the same relative order.  The others leave like culled splats
// (GS_RADIX_SKIP).  The kernel also counts V' (valid buckets among ALL kept splats): the survivors sit at positions
// [V' - P, V') of the order (k_project subtracts V' - P).
// MSD (round 5, N <= 2^24: "the MSD sort" further down): the chunk's histogram row is that of the HIGH bucket byte -- H[chunk][bucket >> 8],
// 256 words -- and the row is also added to the row of the chunk's GROUP of GS_MSD_GROUP chunks (one atomicAdd per digit the chunk
// holds: 4096 distinct words at 1 M splats, each hit 32 times; cleared by the depth pass), so that k_msd_scatter finds the chunk's
// offsets with ~50 row reads instead of a scan launch.  NEAR + MSD: a near-only sort through the same four launches.
template <int NW, bool COMPACT, bool NEAR, bool MSD = false>
__device__ __forceinline__ void k_sort_bucket_body(const float *__restrict__ depth, uint32_t n, uint32_t *__restrict__ keys,
                                                   const unsigned long long *__restrict__ part_min,
                                                   const unsigned long long *__restrict__ part_max,
                                                   const uint32_t *__restrict__ part_cnt, uint32_t nparts,
                                                   uint32_t *__restrict__ hist, GsControl *ctl, const uint32_t *__restrict__ dhist, uint32_t near_req,
                                                   uint32_t *__restrict__ bin_hint, uint32_t *__restrict__ grp)
{
    static_assert(!NEAR || COMPACT, "near-only sorts use the compact records");
    static_assert(!MSD || COMPACT, "the MSD sort takes compact records");
    constexpr int NT = 64 * NW, IPT = 8, CH = NT * IPT;
    __shared__ unsigned long long s_min, s_max;
    __shared__ uint32_t s_cnt;
    constexpr uint32_t BINS = MSD ? 256u : (COMPACT ? 512u : 256u);
    __shared__ uint32_t s_hist[BINS];                             // low-digit histogram of this chunk = radix pass A's input
    __shared__ uint32_t s_nvalid;
    __shared__ int32_t s_bcut;
    if (threadIdx.x == 0) { s_min = ~0ull; s_max = 0ull; s_cnt = 0; s_nvalid = 0; s_bcut = 0; }
    // The depths of this workgroup's (first) chunk depend on nothing the kernel computes: they go out HERE, with the partials' loads below,
    // not behind the fold of min / max and its two barriers -- one dependent round trip where there were two (round 5: what the short
    // kernels of the sort wait for in the pipelined loop is round trips).  Unconditional, index clamped; what lies behind n is masked.
    const uint32_t nchunks = (n + CH - 1) / CH, vend = (nchunks + 7u) & ~7u;
    float dd[IPT];
    uint32_t c = 0;
    auto load_chunk = [&](uint32_t cc) {
#pragma unroll
        for (int r = 0; r < IPT; r++) {
            const uint32_t i = cc * CH + r * NT + threadIdx.x;
            dd[r] = depth[i < n ? i : n - 1u];                           // (n >= 1: there is a chunk)
        }
    };
    bool preloaded = blockIdx.x < vend && gs_xcd_chunk(blockIdx.x, nchunks, c);
    if (preloaded) load_chunk(c);
    __syncthreads();
    {
        unsigned long long mn = ~0ull, mx = 0ull; uint32_t cnt = 0;
        for (uint32_t i = threadIdx.x; i < nparts; i += NT) {
            const unsigned long long a = part_min[i], b = part_max[i];
            mn = a < mn ? a : mn; mx = b > mx ? b : mx; cnt += part_cnt[i];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long omn = shfl_xor_u64(mn, m), omx = shfl_xor_u64(mx, m);
            mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx;
            cnt += __shfl_xor(cnt, m, 64);
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&s_min, mn); atomicMax(&s_max, mx); atomicAdd(&s_cnt, cnt); }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->min_enc = s_min; ctl->max_enc = s_max; ctl->n_kept = s_cnt; ctl->n_total = n; ctl->near_sorted = NEAR ? 1u : 0u; }
    const double mn = gsm::ordered_to_f64(s_min), mx = gsm::ordered_to_f64(s_max);
    const double inv = 65535.0 / (mx - mn);                       // (256*256-1)/(maxDepth-minDepth)
    if (NEAR) {
        // the first bin T with (kept splats in bins <= T) >= near_req, by the first wavefront: the 64 coarse sums (over the
        // copies), a scan, then the 32 bins of the coarse bin where the count is reached
        if (threadIdx.x < 64) {
            const int l = threadIdx.x;
            auto wave_scan = [&](uint32_t v) { for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, d, 64); if (l >= d) v += t; } return v; };
            uint32_t cs = 0;
#pragma unroll
            for (uint32_t c = 0; c < GS_DH_COPIES; c++) cs += dhist[GS_DH_COPIES * GS_DEPTH_BINS + c * GS_DEPTH_COARSE + l];
            const uint32_t cinc = wave_scan(cs);
            const unsigned long long m = __ballot(cinc >= near_req);
            uint32_t T = GS_DEPTH_BINS - 1u;                         // (fewer kept splats than near_req: all of them)
            if (m) {
                const int C = __ffsll((long long)m) - 1;
                const uint32_t before = __shfl(cinc - cs, C, 64);    // kept splats nearer than coarse bin C
                uint32_t fs = 0;
                if (l < 32) {
#pragma unroll
                    for (uint32_t c = 0; c < GS_DH_COPIES; c++) fs += dhist[c * GS_DEPTH_BINS + (uint32_t)C * 32u + l];
                }
                const uint32_t finc = wave_scan(fs);
                const unsigned long long m2 = __ballot(l < 32 && before + finc >= near_req);
                T = (uint32_t)C * 32u + (m2 ? (uint32_t)(__ffsll((long long)m2) - 1) : 31u);
            }
            if (l == 0) {
                int32_t bc = 0;
                if (T < GS_DEPTH_BINS - 1u && inv > 0.0 && inv < 1.0e300) {   // (a degenerate depth range maps everything to bucket 0: keep all)
                    const double x = ((double)(-__uint_as_float((T + 1u) << 20)) - mn) * inv;   // the far edge's place in the bucket table
                    bc = !(x >= 0.0) ? 0 : (x >= 65535.0 ? 65535 : (int32_t)x);                // (NaN / before the table: everything valid)
                }
                s_bcut = bc;
                if (blockIdx.x == 0 && bin_hint) *bin_hint = T;      // (what the next frames' speculative stash goes by)
            }
        }
        __syncthreads();
    }
    const int32_t bcut = s_bcut;
    uint32_t nvalid = 0;
    for (uint32_t v = blockIdx.x; v < vend; v += gridDim.x) {
        if (!preloaded) { if (!gs_xcd_chunk(v, nchunks, c)) continue; load_chunk(c); }   // XCD-aware chunk order (as the radix kernels); all loads first
        preloaded = false;
        for (uint32_t d = threadIdx.x; d < BINS; d += NT) s_hist[d] = 0;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < IPT; r++) {
            const uint32_t i = c * CH + r * NT + threadIdx.x;
            if (i < n) {
                // culled splats leave the sort here: GS_RADIX_SKIP records are not counted and not scattered by pass A.
                // Kept splats whose bucket falls outside the table (the reference drops their writes) carry GS_CULLED_KEY:
                // they sort behind every bucket and store 0, the reference's never-written tail slots
                const float d = dd[r];
                uint32_t k = GS_RADIX_SKIP;
                if (d != INFINITY) {
                    const int32_t b = gsm::sort_bucket(d, mn, inv);
                    if (NEAR) { if (b >= 0) { nvalid++; if (b >= bcut) { k = (uint32_t)b; atomicAdd(&s_hist[MSD ? k >> 8 : k & 511u], 1u); } } }
                    else if (MSD) { if (b >= 0) { k = (uint32_t)b; atomicAdd(&s_hist[k >> 8], 1u); } }
                    else if (COMPACT) { if (b >= 0) { k = (uint32_t)b; atomicAdd(&s_hist[k & 511u], 1u); } }
                    else { k = b >= 0 ? (uint32_t)b : GS_CULLED_KEY; atomicAdd(&s_hist[k & 255u], 1u); }
                }
                keys[i] = k;
            }
        }
        __syncthreads();
        for (uint32_t d = threadIdx.x; d < BINS; d += NT) {
            const uint32_t hv = s_hist[d];
            hist[(size_t)c * BINS + d] = hv;                       // row c of hist[chunk][digit]
            if (MSD && hv) atomicAdd(&grp[(size_t)(c / GS_MSD_GROUP) * BINS + d], hv);   // ... and into the row of the chunk's group
        }
        __syncthreads();
    }
    if (NEAR) {                                                      // V' of the whole order: one global atomic per workgroup
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nvalid += __shfl_xor(nvalid, m, 64);
        if ((threadIdx.x & 63) == 0 && nvalid) atomicAdd(&s_nvalid, nvalid);
        __syncthreads();
        if (threadIdx.x == 0 && s_nvalid) atomicAdd(&ctl->n_valid, s_nvalid);
    }
}

template <int NW, bool COMPACT, bool NEAR, bool MSD = false>
__global__ __launch_bounds__(64 * NW) void k_sort_bucket(const float *__restrict__ depth, uint32_t n, uint32_t *__restrict__ keys,
                                                         const unsigned long long *__restrict__ part_min,
                                                         const unsigned long long *__restrict__ part_max,
                                                         const uint32_t *__restrict__ part_cnt, uint32_t nparts,
                                                         uint32_t *__restrict__ hist, GsControl *ctl, const uint32_t *__restrict__ dhist, uint32_t near_req,
                                                         uint32_t *__restrict__ bin_hint, uint32_t *__restrict__ grp)
{
    k_sort_bucket_body<NW, COMPACT, NEAR, MSD>(depth, n, keys, part_min, part_max, part_cnt, nparts, hist, ctl, dhist, near_req, bin_hint, grp);
}

// Near-only sorts of LONG inputs (round 3).  k_sort_bucket<.., NEAR> still wrote a key for every one of the N splats and pass A
// still read, ranked and scanned all of them (20 M: 80 MB of keys, 5120 x 512 histogram rows) to move the 1.5 % that survive the
// threshold.  Here the bucket pass hands the survivors on directly: every 4096-item chunk stashes its survivors -- (bucket, index)
// records in INDEX order: items r * NT + t of a chunk are ranked by (r, t) through one ballot per row and a 64-entry scan of
// the (row, wave) counts -- in a fixed slot of GS_NEAR_STASH records and leaves their count; k_near_gather turns the stashes into
// one contiguous list (each workgroup sums the counts before its chunks itself: 20 KB of L2 reads at most, no scan launch), in
// chunk order, i.e. in index order, and two stable passes over the P' records (9 + 7 bucket bits) give the order the
// whole-length passes give.  A chunk with more survivors than its stash holds raises near_overflow + round1_missed: the frame
// is drawn again from a whole sort and the context stops using the stash (gs_frame.hip).
template <int NW>
__device__ __forceinline__ void k_near_stash_body(const float *__restrict__ depth, uint32_t n, const unsigned long long *__restrict__ part_min,
                                                  const unsigned long long *__restrict__ part_max, const uint32_t *__restrict__ part_cnt, uint32_t nparts,
                                                  uint2 *__restrict__ stash, uint32_t *__restrict__ cnt_out, GsControl *ctl,
                                                  const uint32_t *__restrict__ dhist, uint32_t near_req, uint32_t *__restrict__ bin_hint)
{
    constexpr int NT = 64 * NW, IPT = 8, CH = NT * IPT;
    __shared__ unsigned long long s_min, s_max;
    __shared__ uint32_t s_cnt, s_nvalid;
    __shared__ int32_t s_bcut;
    __shared__ uint32_t s_row[IPT * NW];                           // survivors per (row, wave) -> their first slot
    if (threadIdx.x == 0) { s_min = ~0ull; s_max = 0ull; s_cnt = 0; s_nvalid = 0; s_bcut = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    {
        unsigned long long mn = ~0ull, mx = 0ull; uint32_t cnt = 0;
        for (uint32_t i = threadIdx.x; i < nparts; i += NT) {
            const unsigned long long a = part_min[i], b = part_max[i];
            mn = a < mn ? a : mn; mx = b > mx ? b : mx; cnt += part_cnt[i];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long omn = shfl_xor_u64(mn, m), omx = shfl_xor_u64(mx, m);
            mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx;
            cnt += __shfl_xor(cnt, m, 64);
        }
        if (lane == 0) { atomicMin(&s_min, mn); atomicMax(&s_max, mx); atomicAdd(&s_cnt, cnt); }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->min_enc = s_min; ctl->max_enc = s_max; ctl->n_kept = s_cnt; ctl->n_total = n; ctl->near_sorted = 1u; }
    const double mn = gsm::ordered_to_f64(s_min), mx = gsm::ordered_to_f64(s_max);
    const double inv = 65535.0 / (mx - mn);
    if (threadIdx.x < 64) {                                         // the threshold bucket: exactly k_sort_bucket<.., NEAR>'s rule
        const int l = threadIdx.x;
        auto wave_scan = [&](uint32_t v) { for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, d, 64); if (l >= d) v += t; } return v; };
        uint32_t cs = 0;
#pragma unroll
        for (uint32_t c = 0; c < GS_DH_COPIES; c++) cs += dhist[GS_DH_COPIES * GS_DEPTH_BINS + c * GS_DEPTH_COARSE + l];
        const uint32_t cinc = wave_scan(cs);
        const unsigned long long m = __ballot(cinc >= near_req);
        uint32_t T = GS_DEPTH_BINS - 1u;
        if (m) {
            const int C = __ffsll((long long)m) - 1;
            const uint32_t before = __shfl(cinc - cs, C, 64);
            uint32_t fs = 0;
            if (l < 32) {
#pragma unroll
                for (uint32_t c = 0; c < GS_DH_COPIES; c++) fs += dhist[c * GS_DEPTH_BINS + (uint32_t)C * 32u + l];
            }
            const uint32_t finc = wave_scan(fs);
            const unsigned long long m2 = __ballot(l < 32 && before + finc >= near_req);
            T = (uint32_t)C * 32u + (m2 ? (uint32_t)(__ffsll((long long)m2) - 1) : 31u);
        }
        if (l == 0) {
            int32_t bc = 0;
            if (T < GS_DEPTH_BINS - 1u && inv > 0.0 && inv < 1.0e300) {
                const double x = ((double)(-__uint_as_float((T + 1u) << 20)) - mn) * inv;
                bc = !(x >= 0.0) ? 0 : (x >= 65535.0 ? 65535 : (int32_t)x);
            }
            s_bcut = bc;
            if (blockIdx.x == 0 && bin_hint) *bin_hint = T;
        }
    }
    __syncthreads();
    const int32_t bcut = s_bcut;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t nvalid = 0;
    const uint32_t nchunks = (n + CH - 1) / CH;
    for (uint32_t v = blockIdx.x; v < ((nchunks + 7u) & ~7u); v += gridDim.x) {
        uint32_t c;
        if (!gs_xcd_chunk(v, nchunks, c)) continue;
        float dd[IPT];
#pragma unroll
        for (int r = 0; r < IPT; r++) {
            const uint32_t i = c * CH + r * NT + threadIdx.x;
            dd[r] = i < n ? depth[i] : INFINITY;
        }
        int32_t bk[IPT];
        uint32_t before[IPT];
#pragma unroll
        for (int r = 0; r < IPT; r++) {
            bk[r] = -1;
            if (dd[r] != INFINITY) {
                const int32_t b = gsm::sort_bucket(dd[r], mn, inv);
                if (b >= 0) { nvalid++; if (b >= bcut) bk[r] = b; }
            }
            const unsigned long long bal = __ballot(bk[r] >= 0);
            before[r] = (uint32_t)__popcll(bal & lt);
            if (lane == 0) s_row[r * NW + w] = (uint32_t)__popcll(bal);
        }
        __syncthreads();
        uint32_t total = 0;
        if (threadIdx.x < 64) {                                     // exclusive scan of the IPT * NW (= 64 at NW = 8) counts, row-major = index order
            uint32_t cv = threadIdx.x < IPT * NW ? s_row[threadIdx.x] : 0u, inc = cv;
            for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
            if (threadIdx.x < IPT * NW) s_row[threadIdx.x] = inc - cv;
            total = __shfl(inc, 63, 64);
            if (threadIdx.x == 0) {
                cnt_out[c] = total < GS_NEAR_STASH ? total : GS_NEAR_STASH;
                if (total > GS_NEAR_STASH) { ctl->near_overflow = 1u; ctl->order_incomplete = 1u; ctl->round1_missed = 1u; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < IPT; r++) {
            if (bk[r] >= 0) {
                const uint32_t slot = s_row[r * NW + w] + before[r];
                if (slot < GS_NEAR_STASH) stash[(size_t)c * GS_NEAR_STASH + slot] = make_uint2((uint32_t)bk[r], c * CH + r * NT + threadIdx.x);
            }
        }
        __syncthreads();                                             // s_row is rewritten by the next chunk
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) nvalid += __shfl_xor(nvalid, m, 64);
    if (lane == 0 && nvalid) atomicAdd(&s_nvalid, nvalid);
    __syncthreads();
    if (threadIdx.x == 0 && s_nvalid) atomicAdd(&ctl->n_valid, s_nvalid);
}

// the stashes -> one list in chunk (= index) order; GS_GATHER_CHUNKS chunks per workgroup, which first sums the counts before them
#define GS_GATHER_CHUNKS 8u
__device__ __forceinline__ void k_near_gather_body(const uint2 *__restrict__ stash, const uint32_t *__restrict__ cnt, uint32_t n, uint32_t chunk,
                                                   uint2 *__restrict__ out, GsControl *ctl)
{
    __shared__ uint32_t s_w[4];
    const uint32_t nchunks = (n + chunk - 1) / chunk;
    const uint32_t ngroups = (nchunks + GS_GATHER_CHUNKS - 1) / GS_GATHER_CHUNKS;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint32_t c0 = g * GS_GATHER_CHUNKS;
        uint32_t s = 0;
        for (uint32_t i = threadIdx.x; i < c0; i += GS_BLOCK) s += cnt[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        __syncthreads();
        if (lane == 0) s_w[w] = s;
        __syncthreads();
        uint32_t base = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        for (uint32_t c = c0; c < c0 + GS_GATHER_CHUNKS && c < nchunks; c++) {
            const uint32_t k = cnt[c];
            for (uint32_t t = threadIdx.x; t < k; t += GS_BLOCK) out[base + t] = stash[(size_t)c * GS_NEAR_STASH + t];
            base += k;
        }
        if (g == ngroups - 1 && threadIdx.x == 0) ctl->n_sorted = base;    // P': what the two passes sort
    }
}

// The exact rule applied to the candidates the depth pass stashed (k_sort_depth<.., SPEC>): fold the partials, find the threshold
// bin and bucket exactly as k_near_stash does, CHECK that the candidates were a superset of what the rule keeps, and compact each
// group of GS_SPEC_GROUP chunks' survivors -- (bucket, index), in index order -- into the group's buffer.
//   superset: the first depth that was NOT stashed is the far edge of bin `lim` (= hint + pad); its bucket must lie below the
//             threshold bucket (the bucket is monotonic in the stored depth), and the exact bin must not lie beyond lim;
//   no dropped bucket anywhere: a kept splat's bucket leaves [0, 65535] only if rounding its depth to f32 moves it by a whole
//             bucket -- impossible while one f32 ulp of the largest |depth| is narrower than a bucket; V' = V then (k_near_stash
//             COUNTS V' over all depths, which this path never reads);
//   no chunk's stash overflowed (raised by the depth pass).
// A frame that fails is flagged like an overflowed stash (order_incomplete: drawn again from a whole sort); spec_fail says
// why: 1 = the hint was behind (transient: it is exact now), 2 = this scene does not suit the path (the context stops using it).
__device__ __forceinline__ void k_near_filter_body(const uint2 *__restrict__ stash, const uint32_t *__restrict__ cnt, uint32_t n,
                                                   const unsigned long long *__restrict__ part_min, const unsigned long long *__restrict__ part_max,
                                                   const uint32_t *__restrict__ part_cnt, uint32_t nparts, uint2 *__restrict__ group_out,
                                                   uint32_t *__restrict__ gcnt, GsControl *ctl, const uint32_t *__restrict__ dhist, uint32_t near_req,
                                                   uint32_t *__restrict__ bin_hint)
{
    __shared__ unsigned long long s_min, s_max;
    __shared__ uint32_t s_cnt, s_T, s_lmin, s_w[4];
    __shared__ int32_t s_bcut;
    if (threadIdx.x == 0) { s_min = ~0ull; s_max = 0ull; s_cnt = 0; s_bcut = 0; s_T = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    {
        unsigned long long mn = ~0ull, mx = 0ull; uint32_t c = 0;
        for (uint32_t i = threadIdx.x; i < nparts; i += GS_BLOCK) {
            const unsigned long long a = part_min[i], b = part_max[i];
            mn = a < mn ? a : mn; mx = b > mx ? b : mx; c += part_cnt[i];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long omn = shfl_xor_u64(mn, m), omx = shfl_xor_u64(mx, m);
            mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx;
            c += __shfl_xor(c, m, 64);
        }
        if (lane == 0) { atomicMin(&s_min, mn); atomicMax(&s_max, mx); atomicAdd(&s_cnt, c); }
    }
    __syncthreads();
    const double mn = gsm::ordered_to_f64(s_min), mx = gsm::ordered_to_f64(s_max);
    const double inv = 65535.0 / (mx - mn);
    if (threadIdx.x < 64) {                                         // the threshold bin and bucket: exactly k_sort_bucket<.., NEAR>'s rule
        const int l = threadIdx.x;
        auto wave_scan = [&](uint32_t v) { for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, d, 64); if (l >= d) v += t; } return v; };
        uint32_t cs = 0;
#pragma unroll
        for (uint32_t c = 0; c < GS_DH_COPIES; c++) cs += dhist[GS_DH_COPIES * GS_DEPTH_BINS + c * GS_DEPTH_COARSE + l];
        const uint32_t cinc = wave_scan(cs);
        const unsigned long long m = __ballot(cinc >= near_req);
        uint32_t T = GS_DEPTH_BINS - 1u;
        if (m) {
            const int C = __ffsll((long long)m) - 1;
            const uint32_t before = __shfl(cinc - cs, C, 64);
            uint32_t fs = 0;
            if (l < 32) {
#pragma unroll
                for (uint32_t c = 0; c < GS_DH_COPIES; c++) fs += dhist[c * GS_DEPTH_BINS + (uint32_t)C * 32u + l];
            }
            const uint32_t finc = wave_scan(fs);
            const unsigned long long m2 = __ballot(l < 32 && before + finc >= near_req);
            T = (uint32_t)C * 32u + (m2 ? (uint32_t)(__ffsll((long long)m2) - 1) : 31u);
        }
        if (l == 0) {
            int32_t bc = 0;
            if (T < GS_DEPTH_BINS - 1u && inv > 0.0 && inv < 1.0e300) {
                const double x = ((double)(-__uint_as_float((T + 1u) << 20)) - mn) * inv;
                bc = !(x >= 0.0) ? 0 : (x >= 65535.0 ? 65535 : (int32_t)x);
            }
            s_bcut = bc; s_T = T;
        }
    }
    __syncthreads();
    const int32_t bcut = s_bcut;
    const uint32_t T = s_T;
    // what cannot be decided chunk by chunk (every workgroup finds the same): the depth range, a stash that overflowed
    uint32_t fail = 0;
    {
        const double big = fmax(fabs(mn), fabs(mx));
        const uint32_t eb = (__float_as_uint((float)big) >> 23) & 0xFFu;
        const double ulp = eb > 23u ? (double)__uint_as_float((eb - 23u) << 23) : 0.0;   // one f32 ulp of the largest |depth|
        if (!(inv > 0.0 && inv < 1.0e300) || !(ulp * inv < 1.0) || ctl->spec_fail == 2u) fail = 2u;
    }
    // the smallest limit a chunk may have been stashed by: the exact bin, and far enough that the first depth NOT stashed (the far
    // edge of that bin) has a bucket below the threshold's (a threshold bucket of 0 keeps every splat: never this path's case)
    if (threadIdx.x == 0) {
        uint32_t L = 0xFFFFu;
        if (!s_cnt) L = 0u;
        else if (bcut > 0 && !fail)
            for (uint32_t c = T; c < T + 8u && c < GS_DEPTH_BINS - 1u; c++)
                if (gsm::sort_bucket(-__uint_as_float((c + 1u) << 20), mn, inv) < bcut) { L = c; break; }
        s_lmin = L;
    }
    __syncthreads();
    const uint32_t lmin = s_lmin;
    if (lmin == 0xFFFFu && !fail) fail = 2u;                         // (buckets coarser than depth bins, or everything kept: the whole-length passes do this scene)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->min_enc = s_min; ctl->max_enc = s_max; ctl->n_kept = s_cnt; ctl->n_total = n; ctl->near_sorted = 2u;   // (2: by this path; read as "not 0" on the device)
        ctl->n_valid = s_cnt;                                        // V' = V: no bucket can be dropped (checked above)
        *bin_hint = T;
        if (fail) { ctl->spec_fail = 2u; ctl->order_incomplete = 1u; ctl->round1_missed = 1u; }
    }
    const uint32_t nchunks = (n + GS_DEPTH_IPT * GS_BLOCK - 1) / (GS_DEPTH_IPT * GS_BLOCK);
    const uint32_t ngroups = (nchunks + GS_SPEC_GROUP - 1) / GS_SPEC_GROUP;
    constexpr uint32_t PER = GS_SPEC_GROUP * GS_SPEC_SLOT / GS_BLOCK;   // 16 consecutive stash slots per thread: index order
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint32_t slot0 = threadIdx.x * PER, c = g * GS_SPEC_GROUP + slot0 / GS_SPEC_SLOT, pos0 = slot0 % GS_SPEC_SLOT;
        const uint32_t cw = (!fail && c < nchunks) ? cnt[c] : 0u, cc = cw & 0xFFFFu;
        if (!fail && c < nchunks && pos0 == 0u && s_cnt && ((cw >> 16) < lmin || (cw >> 16) == 0xFFFFu)) {
            // this chunk was stashed by a limit that does not cover what the exact rule keeps (the hint was behind, or absent): the
            // frame is drawn again from a whole sort; the hint is exact for the next one
            if (ctl->spec_fail != 2u) ctl->spec_fail = 1u;
            ctl->order_incomplete = 1u; ctl->round1_missed = 1u;
            ctl->spec_dbg = (T << 16) | (cw >> 16);
        }
        uint2 rec[PER];
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) rec[k] = pos0 + k < cc ? stash[(size_t)c * GS_SPEC_SLOT + pos0 + k] : make_uint2(0u, 0u);
        uint32_t keep = 0, nk = 0;
        int32_t bk[PER];
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            bk[k] = -1;
            if (pos0 + k < cc) { const int32_t b = gsm::sort_bucket(__uint_as_float(rec[k].x), mn, inv); if (b >= bcut) { bk[k] = b; keep |= 1u << k; nk++; } }
        }
        // exclusive scan of the threads' counts (threads hold consecutive slots: index order)
        uint32_t inc = nk;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
        __syncthreads();
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        uint32_t base = inc - nk, total = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { if (k < w) base += s_w[k]; total += s_w[k]; }
        uint2 *out = group_out + (size_t)g * (GS_SPEC_GROUP * GS_SPEC_SLOT);
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) if (keep & (1u << k)) out[base++] = make_uint2((uint32_t)bk[k], rec[k].y);
        if (threadIdx.x == 0) gcnt[g] = total;
    }
}

// the groups' survivors -> one list in group (= index) order; every workgroup first sums the counts of the groups before its own
__device__ __forceinline__ void k_near_gather_groups_body(const uint2 *__restrict__ group_out, const uint32_t *__restrict__ gcnt, uint32_t n,
                                                          uint2 *__restrict__ out, GsControl *ctl)
{
    __shared__ uint32_t s_w[4];
    const uint32_t nchunks = (n + GS_DEPTH_IPT * GS_BLOCK - 1) / (GS_DEPTH_IPT * GS_BLOCK);
    const uint32_t ngroups = (nchunks + GS_SPEC_GROUP - 1) / GS_SPEC_GROUP;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        uint32_t sv = 0;
        for (uint32_t i = threadIdx.x; i < g; i += GS_BLOCK) sv += gcnt[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sv += __shfl_xor(sv, m, 64);
        __syncthreads();
        if (lane == 0) s_w[w] = sv;
        __syncthreads();
        const uint32_t base = s_w[0] + s_w[1] + s_w[2] + s_w[3], k = gcnt[g];
        const uint2 *src = group_out + (size_t)g * (GS_SPEC_GROUP * GS_SPEC_SLOT);
        for (uint32_t t = threadIdx.x; t < k; t += GS_BLOCK) out[base + t] = src[t];
        if (g == ngroups - 1 && threadIdx.x == 0) ctl->n_sorted = base + k;   // P': what the two passes sort
    }
}
__global__ __launch_bounds__(GS_BLOCK) void k_near_filter(const uint2 *__restrict__ stash, const uint32_t *__restrict__ cnt, uint32_t n,
                                                          const unsigned long long *__restrict__ part_min, const unsigned long long *__restrict__ part_max,
                                                          const uint32_t *__restrict__ part_cnt, uint32_t nparts, uint2 *__restrict__ group_out,
                                                          uint32_t *__restrict__ gcnt, GsControl *ctl, const uint32_t *__restrict__ dhist, uint32_t near_req,
                                                          uint32_t *__restrict__ bin_hint)
{
    k_near_filter_body(stash, cnt, n, part_min, part_max, part_cnt, nparts, group_out, gcnt, ctl, dhist, near_req, bin_hint);
}
__global__ __launch_bounds__(GS_BLOCK) void k_near_gather_groups(const uint2 *__restrict__ group_out, const uint32_t *__restrict__ gcnt, uint32_t n,
                                                                 uint2 *__restrict__ out, GsControl *ctl)
{
    k_near_gather_groups_body(group_out, gcnt, n, out, ctl);
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_near_stash(const float *__restrict__ depth, uint32_t n, const unsigned long long *__restrict__ part_min,
                                                        const unsigned long long *__restrict__ part_max, const uint32_t *__restrict__ part_cnt, uint32_t nparts,
                                                        uint2 *__restrict__ stash, uint32_t *__restrict__ cnt_out, GsControl *ctl,
                                                        const uint32_t *__restrict__ dhist, uint32_t near_req, uint32_t *__restrict__ bin_hint)
{
    k_near_stash_body<NW>(depth, n, part_min, part_max, part_cnt, nparts, stash, cnt_out, ctl, dhist, near_req, bin_hint);
}
__global__ __launch_bounds__(GS_BLOCK) void k_near_gather(const uint2 *__restrict__ stash, const uint32_t *__restrict__ cnt, uint32_t n, uint32_t chunk,
                                                          uint2 *__restrict__ out, GsControl *ctl)
{
    k_near_gather_body(stash, cnt, n, chunk, out, ctl);
}

// the sort's kernels as body functors with their plain kernels (gs_internal.h: GS_BODY; what run_sort<NF> launches through gs_launch)
GS_BODY(F_near_filter, (k_near_filter), (k_near_filter_body));
GS_BODY(F_near_gather_groups, (k_near_gather_groups), (k_near_gather_groups_body));
template <int NW> GS_BODY(F_near_stash, (k_near_stash<NW>), (k_near_stash_body<NW>));
GS_BODY(F_near_gather, (k_near_gather), (k_near_gather_body));
template <int NW, bool COMPACT, bool NEAR, bool MSD = false> GS_BODY(F_sort_bucket, (k_sort_bucket<NW, COMPACT, NEAR, MSD>), (k_sort_bucket_body<NW, COMPACT, NEAR, MSD>));
template <bool STRIP, bool SPEC, bool HID> GS_BODY(F_sort_depth, (k_sort_depth<STRIP, SPEC, HID>), (k_sort_depth_body<1, STRIP, SPEC, HID>));

}  // namespace

static void fill_sort_uniforms(const gs_ctx *ctx, const float view[4], const float *cutout16, const GsSortStrip *strip, SortUniforms &u, StripUniforms &su);

// what the lane's order was made from and how much of it exists (the render re-sorts in full if it turns out to need more)
void gs_remember_sort(gs_ctx *L, const float view[4], const float *cutout16, const GsSortStrip *strip, uint32_t near_req)
{
    memcpy(L->sv_view, view, sizeof L->sv_view);
    L->sv_has_cutout = cutout16 != nullptr;
    if (cutout16) memcpy(L->sv_cutout, cutout16, sizeof L->sv_cutout);
    L->sv_has_strip = strip != nullptr;
    if (strip) L->sv_strip = *strip;
    L->sort_near_req = near_req;
}

// the depth-histogram buffers of this sort: fill the next one (near-only sorts), clear the one the previous near-only sort filled
static DepthHist next_depth_hist(gs_ctx *L, bool near)
{
    DepthHist dh;
    dh.zero = L->dh_dirty; L->dh_dirty = nullptr;
    dh.fill = nullptr; dh.zero_word = nullptr; dh.zero_grp = nullptr; dh.zero_grp_words = 0;
    if (near) {
        dh.fill = L->dhist[L->dh_next]; L->dh_next ^= 1;
        L->dh_dirty = dh.fill;
        dh.zero_word = &L->ctl->n_valid;
    }
    return dh;
}

// The MSD sort (round 5; kernels and rationale in gs_prims.hip): sorts with compact records of at most GS_MSD_MAX_N splats take four
// launches -- depth, bucket (+ rows of the high bucket byte per chunk and per group of chunks), k_msd_scatter, k_seg_sort -- instead
// of seven.  A near-only sort on this path is a TAIL sort: the same four launches, k_msd_scatter drops the segments before the one
// that holds position V' - near_req (it has the segment totals in its hands anyway) and k_seg_sort sorts the rest -- no depth
// histogram, no threshold.  GS_SORT_MSD=0 in the environment keeps the two LSD passes (A/B runs; longer sorts use them anyway).
bool gs_msd_enabled() { static const bool on = []() { const char *e = getenv("GS_SORT_MSD"); return !(e && e[0] == '0'); }(); return on; }
static bool gs_msd_ok(const gs_ctx *L, uint32_t n, bool compact)
{
    return gs_msd_enabled() && compact && n <= GS_MSD_MAX_N && L->msd_grp &&
           (size_t)256 * (gs_div_up(gs_div_up(n, gs_radix_chunk(n)), GS_MSD_GROUP) + 1u) <= L->msd_grp_cap;
}
static void gs_msd_arm(const gs_ctx *L, uint32_t n, DepthHist &dh)   // the depth pass clears the group rows the bucket pass adds to
{
    dh.zero_grp = L->msd_grp;
    dh.zero_grp_words = 256u * gs_div_up(gs_div_up(n, gs_radix_chunk(n)), GS_MSD_GROUP);
}

// may this near-only sort hand its survivors on through the chunk stashes?  Long inputs only (the 4096-item geometry), a share of
// at most 1/32 of the splats (a stash holds 1/8 of its chunk), and not after a stash has overflowed on this context
static bool gs_near_stash_ok(const gs_ctx *L, uint32_t n, uint32_t near_req)
{
    return near_req && gs_radix_chunk(n) == GS_CHUNK_L && (uint64_t)near_req * 32u <= n && !__atomic_load_n(&gs_root(const_cast<gs_ctx *>(L))->near_stash_off, __ATOMIC_RELAXED) &&
           (size_t)(gs_div_up(n, GS_CHUNK_L) + 1u) * GS_NEAR_STASH <= L->scratch_cap / 2;
}
// ... and may its depth pass stash the candidates itself (k_sort_depth<.., SPEC>)?  Only once a near-only sort of this context has
// been collected (the hint exists), and not while the path is held back after a failure (gs_spec_back_off)
static bool gs_near_spec_ok(const gs_ctx *L, uint32_t n)
{
    const gs_ctx *P = gs_root(const_cast<gs_ctx *>(L));
    return __atomic_load_n(&P->near_spec, __ATOMIC_RELAXED) && !__atomic_load_n(&P->near_spec_hold, __ATOMIC_RELAXED) && P->near_spec_opt &&
           (size_t)(gs_div_up(n, (uint32_t)(GS_DEPTH_IPT * GS_BLOCK)) + GS_SPEC_GROUP) * GS_SPEC_SLOT <= L->scratch_cap / 4 &&
           (size_t)gs_div_up(n, (uint32_t)(GS_DEPTH_IPT * GS_BLOCK)) * 2u + 64u <= L->hist_cap;
}
static uint32_t gs_spec_groups(uint32_t n) { return gs_div_up(gs_div_up(n, (uint32_t)(GS_DEPTH_IPT * GS_BLOCK)), GS_SPEC_GROUP); }
static uint32_t gs_near_gather_grid(uint32_t n)
{
    const uint32_t g = gs_div_up(gs_div_up(n, GS_CHUNK_L), 8u);
    return g < 1 ? 1u : (g > 1024u ? 1024u : g);
}

// records the second pass of a near-only sort should expect (its geometry and grid: a matter of speed only)
static uint32_t near_hint(const gs_ctx *L, uint32_t n)
{
    const uint64_t h = (uint64_t)L->sort_near_req * 2u + 65536u;
    return h < n ? (uint32_t)h : n;
}

// The sort of NF frames, one launch per kernel: NF = 1, or the two frames of a pair (GS_OPT_FRAME_BATCH) -- S[0] and S[1] are then sibling
// lanes on ONE stream holding the same resident data; each keeps its own depths, keys, tables, partial slots and control block.  A pair
// takes ONE path: every predicate below is the conjunction over the frames (strip sorts pair with strip sorts, near-only with near-only).
// strip / near_req: null = none for any frame.
template <int NF>
static int run_sort(gs_ctx *const S[], const float *const view[], const float *const cutout16[], const GsSortStrip *const strip[], const uint32_t near_req[])
{
    gs_ctx *ctx = S[0];
    for (int k = 0; k < NF; k++) S[k]->sort_gen++;
    const uint32_t n = (uint32_t)ctx->n;
    SortUniforms u[NF];
    StripUniforms su[NF];
    for (int k = 0; k < NF; k++) fill_sort_uniforms(S[k], view[k], cutout16[k], strip ? strip[k] : nullptr, u[k], su[k]);
    // record format of the two passes: 4 bytes while the index fits in 25 bits (GS_OPT_WIDE_PAIRS forces the general form)
    const bool compact = !ctx->wide_pairs && n <= (1u << 25);
    bool near_all = compact && near_req, msd_ok = true, stash_ok = true, spec_ok = true, strips = true;
    for (int k = 0; k < NF; k++) {
        near_all = near_all && near_req[k];
        msd_ok = msd_ok && gs_msd_ok(S[k], n, compact);
        stash_ok = stash_ok && near_req && gs_near_stash_ok(S[k], n, near_req[k]);
        spec_ok = spec_ok && gs_near_spec_ok(S[k], n);
        strips = strips && u[k].has_strip;
    }
    // Long near-only sorts keep their stashes.  A single frame's lane may also ask for the histogram form by name (no_tail_sort: the shared
    // sort of gs_comm.hip, whose exchange buffer holds ~2 x near_req records) -- that sort is never paired, so a pair does not look at the flag
    const bool msd = msd_ok && !(near_all && (stash_ok || (NF == 1 && ctx->no_tail_sort)));
    // a near-only sort on the MSD path is a TAIL sort (k_msd_scatter cuts the order at a segment boundary: no histogram, no threshold
    // search -- each frame for itself); `near` below is the histogram form of the longer inputs
    uint32_t tail[NF];
    for (int k = 0; k < NF; k++) tail[k] = msd && compact && near_req ? near_req[k] : 0u;
    const bool near = near_all && !msd;
    DepthHist dh[NF];
    for (int k = 0; k < NF; k++) { gs_remember_sort(S[k], view[k], cutout16[k], strip ? strip[k] : nullptr, near ? near_req[k] : tail[k]); dh[k] = next_depth_hist(S[k], near); }
    if (msd) for (int k = 0; k < NF; k++) gs_msd_arm(S[k], n, dh[k]);
    if (!strips) for (int k = 0; k < NF; k++) u[k].has_strip = 0;   // (frames that disagree: all plain)
    const uint32_t g = gs_radix_grid(n);                         // same chunking as the radix kernels (pre-filled histogram rows)
    hipStream_t st = ctx->stream;
    GS_PROF_RECORD(ctx, 0);
    uint32_t gd = gs_div_up(n, (uint32_t)(GS_DEPTH_IPT * GS_BLOCK));
    if (gd < 1) gd = 1;
    if (gd > GS_DEPTH_GRID) gd = GS_DEPTH_GRID;
    // near-only sorts of long inputs hand their survivors on through per-chunk stashes instead of two whole-length passes (above);
    // with a threshold hint the depth pass stashes the candidates itself and writes no depths (SPEC)
    const bool stash = near && stash_ok;
    const bool spec = stash && spec_ok;
    uint32_t *const bin_hint = &gs_root(ctx)->ctl->near_bin_hint;
    for (int k = 0; k < NF; k++) S[k]->sort_form = spec ? 2u : (stash ? 4u : (near ? 1u : (tail[k] ? 3u : 0u)));   // (gs_sort_inspect)
    // the owner's state store (edits drain every lane first: nothing changes it under a sort).  Empty: the kernels of a context that never edits
    const gs_ctx *const R = gs_root(ctx);
    const HiddenArgs hid = { R->edit_n ? R->edit_state : nullptr, R->edit_n ? (uint32_t)R->edit_n : 0u };
    const bool hidden = hid.rows != 0u;
    for (int k = 0; k < NF; k++) S[k]->sort_hidden = hidden ? (uint32_t)R->edit_hidden : 0u;

    // ---- the depth pass: one view per sweep (k_sort_depth: a single frame, and twice through gs_launch<2> for a short pair), or both views of a
    // pair in ONE sweep (k_sort_depth_pair: the rows are read once -- the lanes of a context alias the owner's resident arrays)
    if (NF == 2 && S[0]->sort_rows != S[NF - 1]->sort_rows) { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "paired sort: the two lanes hold different splat arrays"); return GS_E_STATE; }
    DepthViews<NF> dv;
    for (int k = 0; k < NF; k++) dv.v[k] = DepthView{ u[k], su[k], S[k]->depth, S[k]->part_min, S[k]->part_max, S[k]->part_cnt, dh[k], S[k]->kv_b, S[k]->hist, bin_hint, S[k]->ctl };
    // ... where one sweep saves memory traffic: inputs the caches do not hold.  Below GS_DEPTH_PAIR_MIN_N splats the rows stay resident
    // between the two frames' reads, and the one-sweep kernel pays for holding two frames' uniforms (two view rows, two cut-out matrices,
    // two strips' 31 words each: more than the scalar registers hold -- the compiler parks them in lanes of a vector register, and 39 % of
    // that kernel's vector instructions at 1 M splats were v_readlane).  Near-only and speculative pairs always take the one sweep: a twin
    // has no histogram in LDS and no stash
    const bool sweep2 = NF == 2 && (near || spec || n >= GS_DEPTH_PAIR_MIN_N);
    const size_t dlds = near ? (sweep2 ? 2u : 1u) * GS_DEPTH_BINS * sizeof(uint32_t) : 0u;   // one depth histogram per view of the sweep
    gs_flag(strips, [&](auto ST) { gs_flag(spec, [&](auto SP) { gs_flag(hidden, [&](auto HD) {
        constexpr bool STRIP = decltype(ST)::value, SPEC = decltype(SP)::value, HID = decltype(HD)::value;
        if constexpr (NF == 2) {
            if (sweep2) { hipLaunchKernelGGL((k_sort_depth_pair<STRIP, SPEC, HID>), dim3(gd), dim3(GS_BLOCK), dlds, st, (const float4 *)ctx->sort_rows, (const float *)ctx->bound_r, n, dv, hid); return; }
        }
        if constexpr (NF == 1 || !SPEC)                             // (no twin stashes: spec implies sweep2)
            gs_launch<NF, F_sort_depth<STRIP, SPEC, HID>, GS_BLOCK>(gd, st, dlds, [&](int k) {
                return gs_pack_make((const float4 *)S[k]->sort_rows, (const float *)S[k]->bound_r, n, DepthViews<1>{ { dv.v[k] } }, hid); });
    }); }); });
    // ---- end of the depth pass

    GsRadixIO io[NF];
    int rc;
    if (stash) {
        // survivors through per-chunk stashes (k_near_stash / k_near_gather above), or -- the depth pass stashed the candidates -- k_near_filter
        uint2 *list[NF];
        for (int k = 0; k < NF; k++) list[k] = S[k]->kv_b + S[k]->scratch_cap / 2;
        if (spec) {
            uint2 *grp[NF];
            for (int k = 0; k < NF; k++) grp[k] = S[k]->kv_b + S[k]->scratch_cap / 4;
            const uint32_t nch = gs_div_up(n, (uint32_t)(GS_DEPTH_IPT * GS_BLOCK)), ng = gs_spec_groups(n);
            gs_launch<NF, F_near_filter, GS_BLOCK>(ng, st, 0, [&](int k) {
                return gs_pack_make((const uint2 *)S[k]->kv_b, (const uint32_t *)S[k]->hist, n, (const unsigned long long *)S[k]->part_min, (const unsigned long long *)S[k]->part_max,
                                    (const uint32_t *)S[k]->part_cnt, gd, grp[k], S[k]->hist + nch, S[k]->ctl, (const uint32_t *)dh[k].fill, S[k]->sort_near_req, bin_hint); });
            gs_launch<NF, F_near_gather_groups, GS_BLOCK>(ng, st, 0, [&](int k) {
                return gs_pack_make((const uint2 *)grp[k], (const uint32_t *)(S[k]->hist + nch), n, list[k], S[k]->ctl); });
        } else {
            gs_launch<NF, F_near_stash<8>, 512>(g, st, 0, [&](int k) {
                return gs_pack_make((const float *)S[k]->depth, n, (const unsigned long long *)S[k]->part_min, (const unsigned long long *)S[k]->part_max, (const uint32_t *)S[k]->part_cnt, gd,
                                    S[k]->kv_b, S[k]->hist, S[k]->ctl, (const uint32_t *)dh[k].fill, S[k]->sort_near_req, bin_hint); });
            gs_launch<NF, F_near_gather, GS_BLOCK>(gs_near_gather_grid(n), st, 0, [&](int k) {
                return gs_pack_make((const uint2 *)S[k]->kv_b, (const uint32_t *)S[k]->hist, n, (uint32_t)GS_CHUNK_L, list[k], S[k]->ctl); });
        }
        GS_HIP(hipGetLastError());
        for (int k = 0; k < NF; k++) io[k] = GsRadixIO{ list[k], S[k]->key_a, &S[k]->ctl->n_sorted, nullptr, nullptr };
        rc = gs_radix_pass<NF>(S, io, GS_RADIX_PACKED, GS_RADIX_KEYIDX, n, near_hint(ctx, n), 0, 9, false, 0xFFFFFFFFu, 25);
        if (rc != GS_OK) return rc;
        for (int k = 0; k < NF; k++) { io[k].in = S[k]->key_a; io[k].out = S[k]->val_a; }
        rc = gs_radix_pass<NF>(S, io, GS_RADIX_KEYIDX, GS_RADIX_KEYS, n, near_hint(ctx, n), 25, 7);
        if (rc != GS_OK) return rc;
    } else {
        // bucket keys (+ the histogram rows of the first digit); MSD: rows of the high bucket byte per chunk and per group of chunks
        const auto bucket = [&](auto NW, auto C, auto NR, auto M) {
            gs_launch<NF, F_sort_bucket<decltype(NW)::value, decltype(C)::value, decltype(NR)::value, decltype(M)::value>, 64 * decltype(NW)::value>(g, st, 0, [&](int k) {
                return gs_pack_make((const float *)S[k]->depth, n, S[k]->key_a, (const unsigned long long *)S[k]->part_min, (const unsigned long long *)S[k]->part_max,
                                    (const uint32_t *)S[k]->part_cnt, gd, S[k]->hist, S[k]->ctl, (const uint32_t *)dh[k].fill, S[k]->sort_near_req, bin_hint,
                                    decltype(M)::value ? S[k]->msd_grp : (uint32_t *)nullptr); });
        };
        const auto bucket_nw = [&](auto C, auto NR, auto M) {
            if (gs_radix_chunk(n) == GS_CHUNK_L) bucket(std::integral_constant<int, 8>(), C, NR, M); else bucket(std::integral_constant<int, 4>(), C, NR, M);
        };
        const std::true_type yes; const std::false_type no;
        if (msd) bucket_nw(yes, no, yes);
        else if (near) bucket_nw(yes, yes, no);
        else if (compact) bucket_nw(yes, no, no);
        else bucket_nw(no, no, no);
        GS_HIP(hipGetLastError());
        if (msd) {
            // four launches: depth (above), bucket + rows, one stable scatter by the high bucket byte, one LDS sort per segment
            rc = gs_msd_sort<NF>(S, n, tail);
            if (rc != GS_OK) return rc;
        } else if (compact) {
            for (int k = 0; k < NF; k++) io[k] = GsRadixIO{ S[k]->key_a, S[k]->kv_b, &S[k]->ctl->n_total, &S[k]->ctl->n_sorted, nullptr };
            rc = gs_radix_pass<NF>(S, io, GS_RADIX_KEYS, GS_RADIX_KEYIDX, n, n, 0, 9, /*have_hist=*/true, 0xFFFFFFFFu, 25);
            if (rc != GS_OK) return rc;
            // V' records are left (culled splats and dropped buckets took no slot); slots [V', V) of the result are zero-filled:
            // the reference's never-written Uint32Array tail
            // (a near-only sort leaves no zero tail: k_project supplies the zeros of the positions behind its records)
            for (int k = 0; k < NF; k++) io[k] = GsRadixIO{ S[k]->kv_b, S[k]->val_a, &S[k]->ctl->n_sorted, nullptr, near ? nullptr : &S[k]->ctl->n_kept };
            rc = gs_radix_pass<NF>(S, io, GS_RADIX_KEYIDX, GS_RADIX_KEYS, n, near ? near_hint(ctx, n) : n, 25, 7);
            if (rc != GS_OK) return rc;
        } else {
            for (int k = 0; k < NF; k++) io[k] = GsRadixIO{ S[k]->key_a, S[k]->kv_b, &S[k]->ctl->n_total, nullptr, nullptr };
            rc = gs_radix_pass<NF>(S, io, GS_RADIX_KEYS, GS_RADIX_PACKED, n, n, 0, 8, /*have_hist=*/true);
            if (rc != GS_OK) return rc;
            // pass A dropped the culled splats: V records are left.  Splats with a dropped bucket (key 65536) sort behind every
            // bucket and store 0: the tail [V',V) of the result is 0 like the reference's never-written Uint32Array slots
            for (int k = 0; k < NF; k++) io[k] = GsRadixIO{ S[k]->kv_b, S[k]->val_a, &S[k]->ctl->n_kept, nullptr, nullptr };
            rc = gs_radix_pass<NF>(S, io, GS_RADIX_PACKED, GS_RADIX_KEYS, n, n, 8, 9, false, GS_CULLED_KEY);
            if (rc != GS_OK) return rc;
        }
    }
    GS_PROF_RECORD(ctx, 1);
    for (int k = 0; k < NF; k++) { S[k]->sorted = S[k]->val_a; S[k]->have_sort = true; }
    return GS_OK;
}

int gs_run_sort(gs_ctx *ctx, const float view[4], const float *cutout16, const GsSortStrip *strip, uint32_t near_req)
{
    return run_sort<1>(&ctx, &view, &cutout16, &strip, &near_req);
}

int gs_run_sort2(gs_ctx *const S[2], const float *const view[2], const float *const cutout16[2], const GsSortStrip *const strip[2], const uint32_t near_req[2])
{
    return run_sort<2>(S, view, cutout16, strip, near_req);
}

// the uniforms of one sort: view row and cutout matrix widened to f64; for a strip sort (gs_sort_for) the rows of the frame's
// matrices the reach test needs and an upper bound of ||mat3(modelView)||_2 (gs_strip_uniforms.h)
static void fill_sort_uniforms(const gs_ctx *ctx, const float view[4], const float *cutout16, const GsSortStrip *strip, SortUniforms &u, StripUniforms &su)
{
    for (int i = 0; i < 4; i++) u.view[i] = (double)view[i];
    u.has_cutout = cutout16 != nullptr;
    for (int i = 0; i < 16; i++) u.cutout[i] = cutout16 ? (double)cutout16[i] : 0.0;
    // an entity's inverse world matrix is affine: w = 1 / (0 x + 0 y + 0 z + 1) is exactly 1 for finite positions, the division and
    // the three multiplications by it change nothing (in_cutout_affine takes the general path for a position that is not finite)
    if (cutout16 && u.cutout[3] == 0.0 && u.cutout[7] == 0.0 && u.cutout[11] == 0.0 && u.cutout[15] == 1.0) u.has_cutout = 2;
    u.has_strip = 0;
    memset(&su, 0, sizeof su);
    if (strip && ctx->renderable) {
        u.has_strip = gs_fill_strip_uniforms(strip->mv, strip->proj, strip->focal, strip->vw, strip->vh, strip->x0, strip->x1, su);
    }

}

// TEST INFRASTRUCTURE.  Compiles the product's per-splat arithmetic header
// (csrc/gs_device_math.h) for the HOST so its formulas can be compared with the
// oracle and the golden vectors in the CPU-only test tier.  Nothing here is
// part of, linked into or reachable from the product library.
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
#include "gs_device_math.h"
#include "gs_ply.h"
#include "gs_host_tables.h"
#include "gs_strip_uniforms.h"

extern "C" {

__attribute__((visibility("default")))
void hc_pack(const uint8_t *rows, size_t n, float *cs, uint32_t *cc, float *sort_rows)
{
    std::vector<double> tab(GS_POW10_ENTRIES);
    gs_build_pow10_table(tab.data());
    for (size_t i = 0; i < n; i++) {
        uint32_t w[8]; memcpy(w, rows + 32 * i, 32);
        gsm::PackOut o; gsm::pack_row(w, tab.data(), o);
        memcpy(cs + 4 * i, o.cs, 16); memcpy(cc + 4 * i, o.cc, 16); memcpy(sort_rows + 4 * i, o.sort_row, 16);
    }
}

// the sort restated with the product's key functions + a trivially correct stable sort
__attribute__((visibility("default")))
size_t hc_sort(const float *rows4, size_t n, const float *view, const float *cutout, uint32_t *out)
{
    std::vector<float> depth(n); std::vector<uint32_t> idx; idx.reserve(n);
    double mn = INFINITY, mx = -INFINITY;
    for (size_t i = 0; i < n; i++) {
        const float *r = rows4 + 4 * i;
        const double d = gsm::view_depth(view, r[0], r[1], r[2]);
        const bool inside = cutout ? gsm::in_cutout(cutout, r[0], r[1], r[2]) : true;
        if (gsm::sort_keep(d, r[3], inside)) { depth[i] = (float)d; idx.push_back((uint32_t)i); if (d > mx) mx = d; if (d < mn) mn = d; }
    }
    // round-trip the extrema through the ordered-u64 encoding the GPU atomics use
    mn = gsm::ordered_to_f64(gsm::f64_to_ordered(mn)); mx = gsm::ordered_to_f64(gsm::f64_to_ordered(mx));
    const double inv = 65535.0 / (mx - mn);
    std::vector<std::vector<uint32_t>> bins(65536);
    for (uint32_t i : idx) { int32_t b = gsm::sort_bucket(depth[i], mn, inv); if (b >= 0) bins[b].push_back(i); }
    size_t k = 0;
    for (auto &b : bins) for (uint32_t i : b) out[k++] = i;
    for (; k < idx.size(); k++) out[k] = 0;
    return idx.size();
}

__attribute__((visibility("default")))
int hc_project(const float *cs, const uint32_t *cc, uint32_t idx, const float *mv, const float *P, float focal,
               float vw, float vh, float *out16)
{
    gsm::Projected p; gsm::ProjExtra x;
    memset(&p, 0, sizeof p); memset(&x, 0, sizeof x);
    const bool vis = gsm::project_splat(cs + 4 * idx, cc + 4 * idx, mv, P, focal, vw, vh, p, x);
    if (!vis) return 0;
    out16[0] = p.cx; out16[1] = p.cy; out16[2] = p.ax; out16[3] = p.ay; out16[4] = p.bx; out16[5] = p.by;
    out16[6] = x.v1x; out16[7] = x.v1y; out16[8] = x.v2x; out16[9] = x.v2y; out16[10] = x.zndc; out16[11] = p.alpha;
    memcpy(out16 + 12, &p.rgba, 4);
    float b[4]; gsm::splat_pixel_bounds(p, x, b[0], b[1], b[2], b[3]);
    // ints as floats for transport
    out16[13] = b[0]; out16[14] = b[1]; out16[15] = b[2]; out16[16] = b[3];
    return 1;
}


// exact per-tile-row coverage: returns rows written; out[3*k] = ty, tx0, n.  Also the AABB rect in rect[4].
__attribute__((visibility("default")))
int hc_tile_rows(const float *rec8, int W, int H, int x0, int x1, int *out, int max_rows, int *rect)
{
    gsm::Projected p; memcpy(&p, rec8, 32);
    gsm::ProjExtra x; memcpy(&x, rec8 + 8, 5 * sizeof(float));
    float xmin, xmax, ymin, ymax;
    gsm::splat_pixel_bounds(p, x, xmin, xmax, ymin, ymax);
    const float fy0 = fmaxf(ymin, 0.0f), fy1 = fminf(ymax, (float)(H - 1));
    const float fx0 = fmaxf(xmin, (float)x0), fx1 = fminf(xmax, (float)(x1 - 1));
    if (!(fx0 <= fx1 && fy0 <= fy1)) return 0;
    const int r0 = H - 1 - (int)fy1, r1 = H - 1 - (int)fy0;
    rect[0] = ((int)fx0 - x0) / 16; rect[1] = r0 / 16; rect[2] = ((int)fx1 - x0) / 16; rect[3] = r1 / 16;
    gsm::EllipseRows e; gsm::ellipse_rows_setup(p, e);
    int k = 0;
    for (int ty = r0 / 16; ty <= r1 / 16 && k < max_rows; ty++) {
        uint32_t tx0, n; gsm::splat_tile_row(p, e, ty, H, x0, x1, tx0, n);
        out[3 * k] = ty; out[3 * k + 1] = (int)tx0; out[3 * k + 2] = (int)n; k++;
    }
    return k;
}

__attribute__((visibility("default")))
float hc_frag_power(float dx, float dy, float ax, float ay, float bx, float by) { return gsm::frag_power(dx, dy, ax, ay, bx, by); }

__attribute__((visibility("default")))
int32_t hc_toint32(double d) { return gsm::js_toint32(d); }

__attribute__((visibility("default")))
int hc_xcd_chunk(uint32_t v, uint32_t nchunks, uint32_t *chunk) { return gsm::xcd_chunk(v, nchunks, *chunk) ? 1 : 0; }

// positions (x, y, z) x n against an affine cut-out matrix: how many differ between the general test and the affine path
__attribute__((visibility("default")))
size_t hc_cutout_affine_mismatches(const float *pos3, size_t n, const double *c16)
{
    size_t bad = 0;
    for (size_t i = 0; i < n; i++)
        bad += gsm::in_cutout(c16, pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2]) != gsm::in_cutout_affine(c16, pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2]);
    return bad;
}

__attribute__((visibility("default")))
void hc_js_exp(const double *x, size_t n, double *out) { for (size_t i = 0; i < n; i++) out[i] = gsm::js_exp(x[i]); }
}

// ---------------------------------------------------------------- coverage sweep (tests/test_coverage_cpu.py)
// Records (cx, cy, s1, s2, theta): a screen ellipse with its centre at (cx, cy) (GL orientation, as Projected), semi-axes s1 >= s2
// and its long axis at angle theta.  For each one the truth -- gsm::frag_power(dx, dy, ...) <= 4.0f at every pixel centre of the
// strip, the blend's own function and comparison -- is brute-forced, and the two conservative bounds are held against it:
//   tile check      every tile that holds a passing pixel lies in a tile row k_project visits (splat_pixel_bounds) and inside
//                   that row's run [tx0, tx0 + n) (splat_tile_row);
//   sub-tile check  in every such tile, every 4x4-pixel block that holds a passing pixel has its bit in gsm::subtile_mask.
// Both in all nine settings of the emulated 1-ulp reciprocal and square root (GS_HOST_CHECK_ULP), or at the IEEE setting alone.

namespace {

void cov_record(const float *r, gsm::Projected &p, gsm::ProjExtra &x)
{
    // project_splat's own lines from its unit eigenvector (dvx, dvy) = (cos, sin) on, f32, in that order
    const float s1 = r[2], s2 = r[3];
    const float dvx = (float)cos((double)r[4]), dvy = (float)sin((double)r[4]);
    memset(&p, 0, sizeof p); memset(&x, 0, sizeof x);
    x.v1x = s1 * dvx; x.v1y = s1 * dvy;
    x.v2x = s2 * dvy; x.v2y = s2 * -dvx;
    p.cx = r[0]; p.cy = r[1];
    const float n1 = x.v1x * x.v1x + x.v1y * x.v1y, n2 = x.v2x * x.v2x + x.v2y * x.v2y;
    p.ax = x.v2x / n2; p.ay = x.v2y / n2;
    p.bx = x.v1x / n1; p.by = x.v1y / n1;
}

// one image row of the truth.  (fmaf is correctly rounded whether it is the FMA instruction or libm's: the clones differ in speed only)
__attribute__((target_clones("arch=haswell", "default"), flatten))
void cov_pass_row(const gsm::Projected &p, float dy, int x0, int x1, uint8_t *pass)
{
    for (int i = x0; i < x1; i++) {
        const float dx = ((float)i + 0.5f) - p.cx;
        pass[i - x0] = gsm::frag_power(dx, dy, p.ax, p.ay, p.bx, p.by) <= 4.0f;
    }
}

struct CovAcc {
    int64_t tile_miss = 0, blk_miss = 0, claimed = 0, touched = 0, live = 0;
    int64_t first[6] = { -1, 0, 0, 0, 0, 0 };          // record, pixel x, image row, ulp of rcp, ulp of sqrt, check (1 tile, 2 sub-tile)
};

// a passing pixel of tile (ty, tx), inside the blocks `bits` (bit 4 * band + column)
void cov_find_pixel(const gsm::Projected &p, int H, int x0, int x1, int ty, int tx, uint32_t bits, int64_t &px, int64_t &row)
{
    for (int r = 16 * ty; r < 16 * ty + 16 && r < H; r++)
        for (int i = x0 + 16 * tx; i < x0 + 16 * tx + 16 && i < x1; i++) {
            if (!((bits >> (4 * ((r & 15) >> 2) + (((i - x0) & 15) >> 2))) & 1u)) continue;
            const float dx = ((float)i + 0.5f) - p.cx, dy = ((float)(H - 1 - r) + 0.5f) - p.cy;
            if (gsm::frag_power(dx, dy, p.ax, p.ay, p.bx, p.by) <= 4.0f) { px = i; row = r; return; }
        }
}

void cov_one(const float *rec, int64_t ri, int H, int x0, int x1, int checks, int nine, CovAcc &acc,
             std::vector<uint16_t> &blk, std::vector<uint8_t> &pass)
{
    gsm::Projected p; gsm::ProjExtra x;
    cov_record(rec, p, x);
    const int SW = x1 - x0, TX = (SW + 15) / 16, TY = (H + 15) / 16;
    std::fill(blk.begin(), blk.begin() + (size_t)TX * TY, (uint16_t)0);
    bool any = false;
    for (int row = 0; row < H; row++) {
        const float dy = ((float)(H - 1 - row) + 0.5f) - p.cy;
        cov_pass_row(p, dy, x0, x1, pass.data());
        uint16_t *b = blk.data() + (size_t)(row >> 4) * TX;
        const int band = (row & 15) >> 2;
        for (int i0 = 0; i0 < SW; i0 += 8) {
            uint64_t w; memcpy(&w, pass.data() + i0, 8);               // (pass is padded with zeros to a multiple of 8)
            if (!w) continue;
            for (int i = i0; i < i0 + 8 && i < SW; i++)
                if (pass[i]) { b[i >> 4] |= (uint16_t)(1u << (4 * band + ((i & 15) >> 2))); any = true; }
        }
    }
    if (any) acc.live++;
    // the tile rows k_project visits (gs_render.hip: its clamp of splat_pixel_bounds to the strip and the frame)
    float xmin, xmax, ymin, ymax;
    gsm::splat_pixel_bounds(p, x, xmin, xmax, ymin, ymax);
    const float fx0 = fmaxf(xmin, (float)x0), fx1 = fminf(xmax, (float)(x1 - 1));
    const float fy0 = fmaxf(ymin, 0.0f), fy1 = fminf(ymax, (float)(H - 1));
    int ty0 = 0, ty1 = -1;
    if (fx0 <= fx1 && fy0 <= fy1) { ty0 = (H - 1 - (int)fy1) / 16; ty1 = (H - 1 - (int)fy0) / 16; }
    for (int s = 0; s < (nine ? 9 : 1); s++) {
        static const int order[9][2] = { {0, 0}, {-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 1}, {1, -1}, {1, 0}, {1, 1} };
        const int ur = order[s][0], us = order[s][1];
        gsm::hc_ulp_rcp = ur; gsm::hc_ulp_sqrt = us;
        gsm::EllipseRows e; gsm::ellipse_rows_setup(p, e);
        for (int ty = 0; ty < TY; ty++) {
            uint32_t tx0 = 0, n = 0;
            if (ty >= ty0 && ty <= ty1) gsm::splat_tile_row(p, e, ty, H, x0, x1, tx0, n);
            if (s == 0) acc.claimed += n;
            if (!any) continue;
            for (int tx = 0; tx < TX; tx++) {
                const uint32_t have = blk[(size_t)ty * TX + tx];
                if (!have) continue;
                if (s == 0) acc.touched++;
                const bool in_run = (uint32_t)tx >= tx0 && (uint32_t)tx < tx0 + n;
                int bad = 0; uint32_t bits = 0;
                if ((checks & 1) && !in_run) { acc.tile_miss++; bad = 1; bits = have; }
                if ((checks & 2) && in_run) {
                    const uint32_t m = gsm::subtile_mask(p.cx, p.cy, p.ax, p.ay, p.bx, p.by, (float)(x0 + 16 * tx), 16 * ty, H);
                    if (have & ~m) { acc.blk_miss += __builtin_popcount(have & ~m); bad = 2; bits = have & ~m; }
                }
                if (bad && acc.first[0] < 0) {
                    acc.first[0] = ri; acc.first[3] = ur; acc.first[4] = us; acc.first[5] = bad;
                    cov_find_pixel(p, H, x0, x1, ty, tx, bits, acc.first[1], acc.first[2]);
                }
            }
        }
    }
    gsm::hc_ulp_rcp = 0; gsm::hc_ulp_sqrt = 0;
}

}  // namespace

extern "C" {

// out[12]: misses, tile misses, block misses, tiles claimed and tiles touched (both at the IEEE setting), records with a passing
// pixel, then the first offender (lowest record index): record, pixel x, image row, ulp of rcp, ulp of sqrt, check.  Returns misses.
__attribute__((visibility("default")))
int64_t hc_coverage_sweep(const float *recs, size_t n, int W, int H, int x0, int x1, int checks, int nine, int64_t *out)
{
    if (W <= 0 || H <= 0 || x0 < 0 || x1 > W || x0 >= x1) return -1;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    std::vector<CovAcc> accs(nt);
    std::atomic<size_t> next(0);
    auto work = [&](unsigned t) {
        const int TX = (x1 - x0 + 15) / 16, TY = (H + 15) / 16;
        std::vector<uint16_t> blk((size_t)TX * TY);
        std::vector<uint8_t> pass((size_t)(x1 - x0 + 15) & ~(size_t)7, 0);
        for (;;) {
            const size_t a = next.fetch_add(64);
            if (a >= n) break;
            for (size_t i = a; i < a + 64 && i < n; i++) cov_one(recs + 5 * i, (int64_t)i, H, x0, x1, checks, nine, accs[t], blk, pass);
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    memset(out, 0, 12 * sizeof(int64_t)); out[6] = -1;
    for (const CovAcc &a : accs) {
        out[1] += a.tile_miss; out[2] += a.blk_miss; out[3] += a.claimed; out[4] += a.touched; out[5] += a.live;
        if (a.first[0] >= 0 && (out[6] < 0 || a.first[0] < out[6])) memcpy(out + 6, a.first, sizeof a.first);
    }
    out[0] = out[1] + out[2];
    return out[0];
}

// the Projected record of each sweep record (cx, cy, ax, ay, bx, by) and, where px is given, frag_power at pixel (px[i], row[i])
__attribute__((visibility("default")))
void hc_coverage_records(const float *recs, size_t n, int H, float *out6, const int *px, const int *row, float *q)
{
    for (size_t i = 0; i < n; i++) {
        gsm::Projected p; gsm::ProjExtra x;
        cov_record(recs + 5 * i, p, x);
        if (out6) { float *o = out6 + 6 * i; o[0] = p.cx; o[1] = p.cy; o[2] = p.ax; o[3] = p.ay; o[4] = p.bx; o[5] = p.by; }
        if (px) {
            const float dx = ((float)px[i] + 0.5f) - p.cx, dy = ((float)(H - 1 - row[i]) + 0.5f) - p.cy;
            q[i] = gsm::frag_power(dx, dy, p.ax, p.ay, p.bx, p.by);
        }
    }
}
}

// ---------------------------------------------------------------- reach sweep (tests/test_reach_cpu.py)
// gs_sort_for's reach test (gsm::strip_may_touch with the uniforms of gs_fill_strip_uniforms) against the truth, per .splat row:
//   truth   the row, packed (gsm::pack_row) and projected (gsm::project_splat), is visible and some pixel centre with column in
//           [x0, x1) and row in [0, H) has gsm::frag_power <= 4.0f -- brute force over the strip's intersection with the ellipse's
//           f64 bounding box widened by one pixel;
//   miss    truth, and strip_may_touch says false in one of the nine (or the one IEEE) settings of the emulated reciprocal / square root.

namespace {

struct ReachAcc {
    int64_t miss = 0, truth = 0, kept = 0, truth_kept = 0, idle_culled = 0;
    int64_t first[5] = { -1, 0, 0, 0, 0 };             // row, pixel x, image row, ulp of rcp, ulp of sqrt
};

// the first passing pixel of the box, rows top-down; false if none
bool reach_truth(const gsm::Projected &p, const gsm::ProjExtra &x, int H, int x0, int x1, std::vector<uint8_t> &pass, int64_t &px, int64_t &row)
{
    const double hw = 2.0 * sqrt((double)x.v1x * x.v1x + (double)x.v2x * x.v2x), hh = 2.0 * sqrt((double)x.v1y * x.v1y + (double)x.v2y * x.v2y);
    if (!(hw == hw) || !(hh == hh) || !(p.cx == p.cx) || !(p.cy == p.cy)) return false;      // (no such record is visible)
    // pixel i has its centre at i + 0.5; GL row g likewise; one more pixel on every side
    const double fx0 = floor((double)p.cx - hw - 0.5) - 1.0, fx1 = ceil((double)p.cx + hw - 0.5) + 1.0;
    const double fy0 = floor((double)p.cy - hh - 0.5) - 1.0, fy1 = ceil((double)p.cy + hh - 0.5) + 1.0;
    const int i0 = (int)fmax(fx0, (double)x0), i1 = (int)fmin(fx1, (double)(x1 - 1));
    const int g0 = (int)fmax(fy0, 0.0), g1 = (int)fmin(fy1, (double)(H - 1));
    if (i0 > i1 || g0 > g1) return false;
    for (int g = g1; g >= g0; g--) {
        const float dy = ((float)g + 0.5f) - p.cy;
        cov_pass_row(p, dy, i0, i1 + 1, pass.data());
        for (int i = i0; i <= i1; i++) if (pass[i - i0]) { px = i; row = H - 1 - g; return true; }
    }
    return false;
}

}  // namespace

extern "C" {

__attribute__((visibility("default")))
float hc_norm_bound(const float *mv16) { return gs_norm_bound(mv16); }

// the uniforms as the library fills them (31 floats, the struct's layout); returns has_strip
__attribute__((visibility("default")))
int hc_strip_uniforms(const float *mv, const float *proj, float focal, float vw, float vh, int x0, int x1, float *su31)
{
    gsm::StripUniforms su;
    const int has = gs_fill_strip_uniforms(mv, proj, focal, vw, vh, x0, x1, su);
    static_assert(sizeof su == 31 * sizeof(float), "StripUniforms layout");
    memcpy(su31, &su, sizeof su);
    return has;
}

// rows: n x 32-byte .splat rows.  norm_a > 0 replaces the bound gs_fill_strip_uniforms derives (the test feeds the parent commit's
// formula through the same strip_may_touch).  flags (n bytes, may be null): bit 0 truth, bit 1 kept at the IEEE setting, bit 2 visible.
// out[10]: misses, truth, kept (IEEE), truth and kept, neither, then the first offender (lowest row): row, pixel x, image row, ulp of
// rcp, ulp of sqrt.  Returns misses, -1 for a bad strip, -2 when has_strip is 0 (nothing is tested then: the sort keeps every splat).
__attribute__((visibility("default")))
int64_t hc_reach_sweep(const uint8_t *rows, size_t n, const float *mv, const float *proj, float focal, int W, int H, int x0, int x1,
                       float norm_a, int nine, int64_t *out, uint8_t *flags)
{
    if (W <= 0 || H <= 0 || x0 < 0 || x1 > W || x0 >= x1) return -1;
    gsm::StripUniforms su;
    if (!gs_fill_strip_uniforms(mv, proj, focal, (float)W, (float)H, x0, x1, su)) return -2;
    if (norm_a > 0.0f) su.norm_a = norm_a;
    std::vector<double> tab(GS_POW10_ENTRIES);
    gs_build_pow10_table(tab.data());
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    std::vector<ReachAcc> accs(nt);
    std::atomic<size_t> next(0);
    auto work = [&](unsigned t) {
        ReachAcc &acc = accs[t];
        std::vector<uint8_t> pass((size_t)(x1 - x0 + 15) & ~(size_t)7, 0);
        for (;;) {
            const size_t a = next.fetch_add(64);
            if (a >= n) break;
            for (size_t i = a; i < a + 64 && i < n; i++) {
                uint32_t w[8]; memcpy(w, rows + 32 * i, 32);
                gsm::PackOut o; gsm::pack_row(w, tab.data(), o);
                const float mx = o.cs[3] * 32767.0f;                                            // k_pack's line (gs_pack.hip)
                const float bound_r = (mx == mx && mx < 3.0e37f) ? sqrtf(3.0f * mx) * 1.001f : INFINITY;
                gsm::Projected p; gsm::ProjExtra x;
                memset(&p, 0, sizeof p); memset(&x, 0, sizeof x);
                const bool vis = gsm::project_splat(o.cs, o.cc, mv, proj, focal, (float)W, (float)H, p, x);
                int64_t px = 0, row = 0;
                const bool truth = vis && reach_truth(p, x, H, x0, x1, pass, px, row);
                gsm::hc_ulp_rcp = 0; gsm::hc_ulp_sqrt = 0;
                const bool kept = gsm::strip_may_touch(su, o.sort_row[0], o.sort_row[1], o.sort_row[2], bound_r);
                acc.truth += truth; acc.kept += kept; acc.truth_kept += truth && kept; acc.idle_culled += !truth && !kept;
                if (flags) flags[i] = (uint8_t)((truth ? 1 : 0) | (kept ? 2 : 0) | (vis ? 4 : 0));
                if (!truth) continue;
                for (int s = 0; s < (nine ? 9 : 1); s++) {
                    gsm::hc_ulp_rcp = s / 3 - 1 + (nine ? 0 : 1); gsm::hc_ulp_sqrt = s % 3 - 1 + (nine ? 0 : 1);
                    if (gsm::strip_may_touch(su, o.sort_row[0], o.sort_row[1], o.sort_row[2], bound_r)) continue;
                    acc.miss++;
                    if (acc.first[0] < 0 || (int64_t)i < acc.first[0]) { acc.first[0] = (int64_t)i; acc.first[1] = px; acc.first[2] = row; acc.first[3] = gsm::hc_ulp_rcp; acc.first[4] = gsm::hc_ulp_sqrt; }
                }
                gsm::hc_ulp_rcp = 0; gsm::hc_ulp_sqrt = 0;
            }
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    memset(out, 0, 10 * sizeof(int64_t)); out[5] = -1;
    for (const ReachAcc &a : accs) {
        out[0] += a.miss; out[1] += a.truth; out[2] += a.kept; out[3] += a.truth_kept; out[4] += a.idle_culled;
        if (a.first[0] >= 0 && (out[5] < 0 || a.first[0] < out[5])) memcpy(out + 5, a.first, sizeof a.first);
    }
    return out[0];
}
}

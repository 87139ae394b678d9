// gs_cply.h -- the chunked compressed .ply (include/gs_splat.h: "Compressed .ply" spells the rules out): 16 bytes per splat against
// one bounds record per 256 splats.  The per-splat arithmetic of both directions, written once and called by the kernels
// (gs_cply.hip) and by the host entry points (gs_host.cpp), so that both produce the same bytes by construction.
//
// The format is restated from memory of the published one (PlayCanvas / SuperSplat); no file written by those tools was at hand:
// interoperability with their files is SUPPOSED, NOT VERIFIED (docs/LAB_NOTES.md 9s).
//
// Everything is IEEE f64 built from + - * / sqrt, floor and comparisons only (all correctly rounded on the host and on gfx950),
// un-fused (-ffp-contract=off), in the order written out below.  No array is indexed by a run-time value.
#pragma once
#include "gs_ply.h"                                               // js_exp, clamped_u8

#define GS_CPLY_CHUNK 256u                                        // splats per bounds record
#define GS_CPLY_SQRT2 1.4142135623730951                          // sqrt(2.0), correctly rounded
#define GS_CPLY_SH_C0 0.28209479177387814

namespace gsm {

// what the header says (gs_cply_plan, gs_host.cpp)
struct CplyInfo {
    size_t n, chunks, data_start;
    int chunk_floats;                                             // 12 or 18
    int per;                                                      // f_rest_* per channel in the file: 0 (no `element sh`), 3, 8, 15
    int degree;                                                   // 0..3
};

// ---- min / max of f32 values as unsigned keys: ascending key = ascending value, -0 below +0; a value that is not finite takes no part
GS_PLY_HD bool cply_finite(float f) { union { float f; uint32_t u; } c; c.f = f; return (c.u & 0x7F800000u) != 0x7F800000u; }
GS_PLY_HD uint32_t cply_key(float f) { union { float f; uint32_t u; } c; c.f = f; return (c.u >> 31) ? ~c.u : (c.u | 0x80000000u); }
GS_PLY_HD float cply_unkey(uint32_t k) { union { float f; uint32_t u; } c; c.u = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k; return c.f; }
#define GS_CPLY_KEY_MIN_ID 0xFFFFFFFFu                            // the identities: no finite value's key is either
#define GS_CPLY_KEY_MAX_ID 0u
// (lo, hi) of a reduction's keys; nothing finite took part: lo = hi = 0
GS_PLY_HD void cply_bounds_of(uint32_t kmin, uint32_t kmax, float &lo, float &hi)
{
    if (kmin > kmax) { lo = 0.0f; hi = 0.0f; } else { lo = cply_unkey(kmin); hi = cply_unkey(kmax); }
}

// ---- gsm::log_fixed: the natural logarithm from + - * / and the exponent field alone, the same bits on the host and on the device.
// x = m * 2^e with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), log = e * ln2 + 2 * (s + s^3/3 + ... + s^21/21): Horner in z = s * s,
// innermost term first.  Denormals are scaled by 2^54 first.  0 -> -inf, x < 0 or NaN -> NaN, +inf -> +inf.
GS_PLY_HD double log_fixed(double x)
{
    union { double d; uint64_t u; } c; c.d = x;
    if (x != x || (c.u >> 63)) { if (x == 0.0) { c.u = 0xFFF0000000000000ull; return c.d; } c.u = 0x7FF8000000000000ull; return c.d; }
    if (x == 0.0) { c.u = 0xFFF0000000000000ull; return c.d; }
    if ((c.u >> 52) == 0x7FFull) return x;                       // +inf
    int e = 0;
    if ((c.u >> 52) == 0) { c.d = x * 18014398509481984.0; e = -54; }   // * 2^54: exact
    e += (int)(c.u >> 52) - 1023;
    c.u = (c.u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;  // m in [1, 2)
    double m = c.d;
    if (m >= GS_CPLY_SQRT2) { m = m * 0.5; e += 1; }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double q = 1.0 / 21.0;
    q = 1.0 / 19.0 + z * q; q = 1.0 / 17.0 + z * q; q = 1.0 / 15.0 + z * q; q = 1.0 / 13.0 + z * q; q = 1.0 / 11.0 + z * q;
    q = 1.0 / 9.0 + z * q; q = 1.0 / 7.0 + z * q; q = 1.0 / 5.0 + z * q; q = 1.0 / 3.0 + z * q;
    return (double)e * 0.6931471805599453 + 2.0 * (s + s * (z * q));
}

// ---- decode
// (position and scale words: 11 bits at 21, 10 bits at 11, 11 bits at 0 -- the three fields tile the word)
GS_PLY_HD double cply_u(uint32_t v, uint32_t bits) { const uint32_t m = (1u << bits) - 1u; return (double)(v & m) / (double)m; }
GS_PLY_HD double cply_lerp(float lo, float hi, double t) { return (double)lo + ((double)hi - (double)lo) * t; }

// chunk: the splat's bounds record (chunk_floats = 12 or 18 f32).  packed: position, rotation, scale, colour.  row: the 32-byte row as
// 8 little-endian words.  wide (may be null): scale[3], then the quaternion (w, x, y, z as a .ply stores it) as f32, before the byte
// rounding.  colour (may be null): the three unrounded colour values v_c the SH row's DC terms are made from.
GS_PLY_HD void cply_decode(const float *chunk, int chunk_floats, const uint32_t packed[4], uint32_t row[8], float *wide, double *colour)
{
    union { float f; uint32_t u; } cv;
    const uint32_t p = packed[0], w = packed[1], sc = packed[2], col = packed[3];
    cv.f = (float)cply_lerp(chunk[0], chunk[3], cply_u(p >> 21, 11)); row[0] = cv.u;
    cv.f = (float)cply_lerp(chunk[1], chunk[4], cply_u(p >> 11, 10)); row[1] = cv.u;
    cv.f = (float)cply_lerp(chunk[2], chunk[5], cply_u(p, 11)); row[2] = cv.u;
    const float s0 = (float)js_exp(cply_lerp(chunk[6], chunk[9], cply_u(sc >> 21, 11)));
    const float s1 = (float)js_exp(cply_lerp(chunk[7], chunk[10], cply_u(sc >> 11, 10)));
    const float s2 = (float)js_exp(cply_lerp(chunk[8], chunk[11], cply_u(sc, 11)));
    cv.f = s0; row[3] = cv.u; cv.f = s1; row[4] = cv.u; cv.f = s2; row[5] = cv.u;
    // the three smaller components, the largest from the unit length
    const uint32_t k = w >> 30;
    const double a = (cply_u(w >> 20, 10) - 0.5) * GS_CPLY_SQRT2, b = (cply_u(w >> 10, 10) - 0.5) * GS_CPLY_SQRT2, c = (cply_u(w, 10) - 0.5) * GS_CPLY_SQRT2;
    const double rest = 1.0 - ((a * a + b * b) + c * c);
    const double m = sqrt(rest > 0.0 ? rest : 0.0);
    double q0 = k == 0 ? m : a;
    double q1 = k == 0 ? a : k == 1 ? m : b;
    double q2 = k <= 1 ? b : k == 2 ? m : c;
    double q3 = k == 3 ? m : c;
    const double len = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    q0 = q0 / len; q1 = q1 / len; q2 = q2 / len; q3 = q3 / len;
    row[7] = (uint32_t)clamped_u8(q0 * 128.0 + 128.0) | ((uint32_t)clamped_u8(q1 * 128.0 + 128.0) << 8) |
             ((uint32_t)clamped_u8(q2 * 128.0 + 128.0) << 16) | ((uint32_t)clamped_u8(q3 * 128.0 + 128.0) << 24);
    double v0 = cply_u(col >> 24, 8), v1 = cply_u(col >> 16, 8), v2 = cply_u(col >> 8, 8);
    if (chunk_floats == 18) { v0 = cply_lerp(chunk[12], chunk[15], v0); v1 = cply_lerp(chunk[13], chunk[16], v1); v2 = cply_lerp(chunk[14], chunk[17], v2); }
    row[6] = (uint32_t)clamped_u8(v0 * 255.0) | ((uint32_t)clamped_u8(v1 * 255.0) << 8) | ((uint32_t)clamped_u8(v2 * 255.0) << 16) |
             ((uint32_t)clamped_u8(cply_u(col, 8) * 255.0) << 24);
    if (wide) { wide[0] = s0; wide[1] = s1; wide[2] = s2; wide[3] = (float)q0; wide[4] = (float)q1; wide[5] = (float)q2; wide[6] = (float)q3; }
    if (colour) { colour[0] = v0; colour[1] = v1; colour[2] = v2; }
}
// the SH row's entries: the DC term from the unrounded colour, the others from their byte
GS_PLY_HD float cply_sh_dc(double v) { return (float)((v - 0.5) / GS_CPLY_SH_C0); }
GS_PLY_HD float cply_sh_rest(uint8_t byte) { return (float)((double)byte * (8.0 / 255.0) - 4.0); }

// ---- encode
GS_PLY_HD uint32_t cply_code(double t, uint32_t bits)
{
    const double top = (double)((1u << bits) - 1u);
    if (t != t || t <= 0.0) return 0u;
    const double r = floor(t * top + 0.5);
    return r >= top ? (uint32_t)top : (uint32_t)r;
}
GS_PLY_HD double cply_t(float v, float lo, float hi) { return hi > lo ? ((double)v - (double)lo) / ((double)hi - (double)lo) : 0.0; }
GS_PLY_HD uint8_t cply_sh_byte(float v) { return clamped_u8(((double)v + 4.0) * (255.0 / 8.0)); }

// the nine values a chunk's bounds are taken over: position, log scale, colour.  row: the 32-byte row as 8 words; wide: 7 f32 or null;
// sh: the splat's SH row or null, sh_stride = floats between its channels.
GS_PLY_HD float cply_log_scale(float scale)
{
    if (!(scale > 0.0f)) return -20.0f;                          // 0, negative, NaN
    const double l = log_fixed((double)scale);
    return (float)(l < -20.0 ? -20.0 : l > 20.0 ? 20.0 : l);
}
GS_PLY_HD void cply_values(const uint32_t row[8], const float *wide, const float *sh, int sh_stride, float v[9])
{
    union { float f; uint32_t u; } cv;
    cv.u = row[0]; v[0] = cv.f; cv.u = row[1]; v[1] = cv.f; cv.u = row[2]; v[2] = cv.f;
    float s0, s1, s2;
    if (wide) { s0 = wide[0]; s1 = wide[1]; s2 = wide[2]; }
    else { cv.u = row[3]; s0 = cv.f; cv.u = row[4]; s1 = cv.f; cv.u = row[5]; s2 = cv.f; }
    v[3] = cply_log_scale(s0); v[4] = cply_log_scale(s1); v[5] = cply_log_scale(s2);
    if (sh) {
        v[6] = (float)(0.5 + GS_CPLY_SH_C0 * (double)sh[0]); v[7] = (float)(0.5 + GS_CPLY_SH_C0 * (double)sh[sh_stride]);
        v[8] = (float)(0.5 + GS_CPLY_SH_C0 * (double)sh[2 * sh_stride]);
    } else {
        v[6] = (float)((double)(row[6] & 0xFFu) / 255.0); v[7] = (float)((double)((row[6] >> 8) & 0xFFu) / 255.0);
        v[8] = (float)((double)((row[6] >> 16) & 0xFFu) / 255.0);
    }
}
// v: cply_values' nine; bounds: the chunk record (18 f32); row, wide: as above.  out: position, rotation, scale, colour.
GS_PLY_HD void cply_encode(const float v[9], const float bounds[18], const uint32_t row[8], const float *wide, uint32_t out[4])
{
    out[0] = (cply_code(cply_t(v[0], bounds[0], bounds[3]), 11) << 21) | (cply_code(cply_t(v[1], bounds[1], bounds[4]), 10) << 11) |
             cply_code(cply_t(v[2], bounds[2], bounds[5]), 11);
    out[2] = (cply_code(cply_t(v[3], bounds[6], bounds[9]), 11) << 21) | (cply_code(cply_t(v[4], bounds[7], bounds[10]), 10) << 11) |
             cply_code(cply_t(v[5], bounds[8], bounds[11]), 11);
    out[3] = (cply_code(cply_t(v[6], bounds[12], bounds[15]), 8) << 24) | (cply_code(cply_t(v[7], bounds[13], bounds[16]), 8) << 16) |
             (cply_code(cply_t(v[8], bounds[14], bounds[17]), 8) << 8) | (row[6] >> 24);
    double q0, q1, q2, q3;
    if (wide) { q0 = (double)wide[3]; q1 = (double)wide[4]; q2 = (double)wide[5]; q3 = (double)wide[6]; }
    else {
        q0 = ((double)(row[7] & 0xFFu) - 128.0) / 128.0; q1 = ((double)((row[7] >> 8) & 0xFFu) - 128.0) / 128.0;
        q2 = ((double)((row[7] >> 16) & 0xFFu) - 128.0) / 128.0; q3 = ((double)(row[7] >> 24) - 128.0) / 128.0;
    }
    const double len = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    if (!(len > 0.0) || !(len <= 1.7976931348623157e308)) { q0 = 1.0; q1 = 0.0; q2 = 0.0; q3 = 0.0; }   // zero, or a component that is not finite
    else { q0 = q0 / len; q1 = q1 / len; q2 = q2 / len; q3 = q3 / len; }
    // the first index of the largest magnitude
    uint32_t k = 0; double big = fabs(q0);
    if (fabs(q1) > big) { k = 1; big = fabs(q1); }
    if (fabs(q2) > big) { k = 2; big = fabs(q2); }
    if (fabs(q3) > big) { k = 3; big = fabs(q3); }
    const double qk = k == 0 ? q0 : k == 1 ? q1 : k == 2 ? q2 : q3;
    if (qk < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
    const double a = k == 0 ? q1 : q0, b = k <= 1 ? q2 : q1, c = k == 3 ? q2 : q3;
    out[1] = (k << 30) | (cply_code(a / GS_CPLY_SQRT2 + 0.5, 10) << 20) | (cply_code(b / GS_CPLY_SQRT2 + 0.5, 10) << 10) | cply_code(c / GS_CPLY_SQRT2 + 0.5, 10);
}

// ---- the Morton order (GS_CPLY_MORTON): 10 bits per axis against the box of all finite positions
GS_PLY_HD uint32_t cply_spread(uint32_t v)
{
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu; v = (v | (v << 8)) & 0x0300F00Fu; v = (v | (v << 4)) & 0x030C30C3u; v = (v | (v << 2)) & 0x09249249u;
    return v;
}
GS_PLY_HD uint32_t cply_axis(float v, float lo, float hi)
{
    const double t = cply_t(v, lo, hi);
    if (t != t || t < 0.0) return 0u;
    const double r = floor(t * 1024.0);
    return r >= 1023.0 ? 1023u : (uint32_t)r;
}
GS_PLY_HD uint32_t cply_morton(const float pos[3], const float box[6] /* lo x y z, hi x y z */)
{
    return cply_spread(cply_axis(pos[0], box[0], box[3])) | (cply_spread(cply_axis(pos[1], box[1], box[4])) << 1) |
           (cply_spread(cply_axis(pos[2], box[2], box[5])) << 2);
}

}  // namespace gsm

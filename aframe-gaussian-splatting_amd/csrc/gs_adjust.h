// gs_adjust.h -- the colour adjustment of include/gs_splat.h (gs_colour_adjust: an affine map of a splat's colour and a linear one of
// its alpha), written once and called by the kernels (gs_adjust.hip: k_adjust_colour, k_adjust_sh) and by the host entry points
// (gs_host.cpp: gs_adjust_word, gs_adjust_sh_row), so that both produce the same bytes by construction.
//
// Everything is IEEE f64 built from + * / only (all correctly rounded on the host and on gfx950), un-fused (-ffp-contract=off), on the
// f32 parameters widened (exact), in the order written out below.  The colour word's bytes clamp (clamped_u8); SH coefficients do not.
// The colour before the clamp, (0.5 + SH_C0 * sh[c][0] + sum_k basis_k * sh[c][k]) * 255 (gs_sh.h), is affine in the coefficients, so
// the map M v + offset on it is the matrix on every band and, on band 0 alone, the constant that carries the 0.5 and the offset across.
#pragma once
#include "gs_ply.h"                                               // clamped_u8: the Uint8ClampedArray store (index.js:704-707)

namespace gsm {

// the parameters as the arithmetic takes them; dc[c]: what channel c's band-0 coefficient gains (exactly 0 for the identity)
struct AdjustParams { double m[9], offset[3], alpha_scale, alpha_offset, dc[3]; };

// false: a parameter is not finite (decided on the bits: no NaN reaches a comparison), p is not to be used
GS_PLY_HD bool adjust_widen(const float m[9], const float offset[3], float alpha_scale, float alpha_offset, AdjustParams &p)
{
    const double SH_C0 = 0.28209479177387814;                    // (gs_sh.h)
    union { float f; uint32_t u; } cv;
    bool finite = true;
    for (int i = 0; i < 9; i++) { cv.f = m[i]; finite = finite && (cv.u & 0x7F800000u) != 0x7F800000u; p.m[i] = (double)m[i]; }
    for (int c = 0; c < 3; c++) { cv.f = offset[c]; finite = finite && (cv.u & 0x7F800000u) != 0x7F800000u; p.offset[c] = (double)offset[c]; }
    cv.f = alpha_scale; finite = finite && (cv.u & 0x7F800000u) != 0x7F800000u; p.alpha_scale = (double)alpha_scale;
    cv.f = alpha_offset; finite = finite && (cv.u & 0x7F800000u) != 0x7F800000u; p.alpha_offset = (double)alpha_offset;
    for (int c = 0; c < 3; c++) p.dc[c] = ((0.5 * ((p.m[3 * c] + p.m[3 * c + 1]) + p.m[3 * c + 2]) + p.offset[c] / 255) - 0.5) / SH_C0;
    return finite;
}

// the colour word R | G << 8 | B << 16 | A << 24
GS_PLY_HD uint32_t adjust_word(uint32_t rgba, const AdjustParams &p)
{
    const double R = (double)(rgba & 0xFFu), G = (double)((rgba >> 8) & 0xFFu), B = (double)((rgba >> 16) & 0xFFu), A = (double)(rgba >> 24);
    const double v0 = ((p.m[0] * R + p.m[1] * G) + p.m[2] * B) + p.offset[0];
    const double v1 = ((p.m[3] * R + p.m[4] * G) + p.m[5] * B) + p.offset[1];
    const double v2 = ((p.m[6] * R + p.m[7] * G) + p.m[8] * B) + p.offset[2];
    const double va = p.alpha_scale * A + p.alpha_offset;
    return (uint32_t)clamped_u8(v0) | ((uint32_t)clamped_u8(v1) << 8) | ((uint32_t)clamped_u8(v2) << 16) | ((uint32_t)clamped_u8(va) << 24);
}

// coefficient k of the three channels: all three new values from the three old ones (out may be in).  Alpha has no SH part.
GS_PLY_HD void adjust_sh_coef(const float in[3], int k, const AdjustParams &p, float out[3])
{
    const double s0 = (double)in[0], s1 = (double)in[1], s2 = (double)in[2];
    double v0 = (p.m[0] * s0 + p.m[1] * s1) + p.m[2] * s2;
    double v1 = (p.m[3] * s0 + p.m[4] * s1) + p.m[5] * s2;
    double v2 = (p.m[6] * s0 + p.m[7] * s1) + p.m[8] * s2;
    if (k == 0) { v0 = v0 + p.dc[0]; v1 = v1 + p.dc[1]; v2 = v2 + p.dc[2]; }
    out[0] = (float)v0; out[1] = (float)v1; out[2] = (float)v2;
}

}  // namespace gsm

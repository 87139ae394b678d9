// gs_sh.h -- view-dependent colour: real spherical harmonics of degree 0..3 as published with 3D Gaussian Splatting
// (Kerbl et al. 2023: the eval_sh formulae and constants), shared by the host (gs_host.cpp: gs_sh_eval) and the projection
// kernel (gs_render.hip: k_project<.., SH>) so that both produce the same bytes by construction.
//
// The reference knows only the degree-0 term: processPlyBuffer bakes `(0.5 + SH_C0 * f_dc) * 255` into the colour byte
// (index.js:725-729, gs_ply.h:ply_row) and drops the 45 f_rest_* coefficients.  Here, with d = (pos - cam) / |pos - cam| in
// the splat's object space and K = (degree + 1)^2,
//
//     unrounded_c = (0.5 + SH_C0 * sh[c][0] + sum_{k = 1..K-1} basis_k(d) * sh[c][k]) * 255,   byte_c = clamped_u8(unrounded_c)
//
// Everything is IEEE f64 built from + - * / sqrt only, unfused (-ffp-contract=off), in the order written out below: the sum
// runs in ascending k and starts from `0.5 + SH_C0 * sh[c][0]`.  Degree 0, and any splat whose higher coefficients are all
// zero, therefore give EXACTLY the byte the reference bakes.  A splat at the camera (|pos - cam| == 0) has d = (0, 0, 0).
//
// WHICH object space: the rows' -- the positions as the .ply / .splat row stores them, the space the coefficients were trained
// in.  The reference mirrors z when it packs (the centre texel is (x, y, -z), index.js:350-354) and gsModelViewMatrix acts on
// that texel, so camera_in_object(model_view) comes out in the mirrored space: a frame negates its z (exact) before it hands the
// camera to the kernel, and the kernel negates the texel's z back.  Evaluating in the mirrored space instead would reflect every
// highlight through the xy plane.
//
// An SH row is 3 * K f32, channel-major: sh[c][k], k = 0 is f_dc_c (a PLY stores f_rest_0..14 for red, 15..29 for green,
// 30..44 for blue).  The coefficients reach the arithmetic through an accessor `coef(c, k)` so that the kernel can hand over
// registers and the host a pointer.
#pragma once
#include "gs_ply.h"

#define GS_SH_MAX_DEGREE 3

namespace gsm {

GS_PLY_HD int sh_coefs(int degree) { return (degree + 1) * (degree + 1); }
// f32 per channel of a row in the DEVICE store: K rounded up to whole 16-byte loads (4, 12, 16: a degree-2 row is padded so
// that every channel starts on a 16-byte boundary); rows handed over the C ABI are tight (3 * K)
GS_PLY_HD int sh_channel_stride(int degree) { return (sh_coefs(degree) + 3) & ~3; }

// coefficients behind a pointer: channel c starts at p + c * stride
struct ShRowPtr {
    const float *p; int stride;
    GS_PLY_HD float operator()(int c, int k) const { return p[c * stride + k]; }
};

// the three unrounded colour values (in units of one colour byte) of one splat for one camera position
template <class Coef>
GS_PLY_HD void sh_unrounded(const Coef &coef, int degree, const double cam[3], const float pos[3], double out[3])
{
    const double SH_C0 = 0.28209479177387814, SH_C1 = 0.4886025119029199;
    const double SH_C2_0 = 1.0925484305920792, SH_C2_1 = -1.0925484305920792, SH_C2_2 = 0.31539156525252005;
    const double SH_C2_3 = -1.0925484305920792, SH_C2_4 = 0.5462742152960396;
    const double SH_C3_0 = -0.5900435899266435, SH_C3_1 = 2.890611442640554, SH_C3_2 = -0.4570457994644658;
    const double SH_C3_3 = 0.3731763325901154, SH_C3_4 = -0.4570457994644658, SH_C3_5 = 1.445305721320277;
    const double SH_C3_6 = -0.5900435899266435;
    const double dx = (double)pos[0] - cam[0], dy = (double)pos[1] - cam[1], dz = (double)pos[2] - cam[2];
    const double len = sqrt((dx * dx + dy * dy) + dz * dz);
    double x = 0.0, y = 0.0, z = 0.0;
    if (len != 0.0) { x = dx / len; y = dy / len; z = dz / len; }     // (NaN lengths divide too: the colour comes out 0)
    double r[3];
#define GS_SH_TERM(k, basis) do { const double b_ = (basis); for (int c = 0; c < 3; c++) r[c] = r[c] + b_ * (double)coef(c, k); } while (0)
    for (int c = 0; c < 3; c++) r[c] = 0.5 + SH_C0 * (double)coef(c, 0);
    if (degree >= 1) {
        GS_SH_TERM(1, -SH_C1 * y);
        GS_SH_TERM(2, SH_C1 * z);
        GS_SH_TERM(3, -SH_C1 * x);
    }
    if (degree >= 2) {
        const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        GS_SH_TERM(4, SH_C2_0 * xy);
        GS_SH_TERM(5, SH_C2_1 * yz);
        GS_SH_TERM(6, SH_C2_2 * ((2.0 * zz - xx) - yy));
        GS_SH_TERM(7, SH_C2_3 * xz);
        GS_SH_TERM(8, SH_C2_4 * (xx - yy));
        if (degree >= 3) {
            GS_SH_TERM(9, (SH_C3_0 * y) * (3.0 * xx - yy));
            GS_SH_TERM(10, (SH_C3_1 * xy) * z);
            GS_SH_TERM(11, (SH_C3_2 * y) * ((4.0 * zz - xx) - yy));
            GS_SH_TERM(12, (SH_C3_3 * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy));
            GS_SH_TERM(13, (SH_C3_4 * x) * ((4.0 * zz - xx) - yy));
            GS_SH_TERM(14, (SH_C3_5 * z) * (xx - yy));
            GS_SH_TERM(15, (SH_C3_6 * x) * (xx - 3.0 * yy));
        }
    }
#undef GS_SH_TERM
    for (int c = 0; c < 3; c++) out[c] = r[c] * 255;
}

template <class Coef>
GS_PLY_HD void sh_color(const Coef &coef, int degree, const double cam[3], const float pos[3], uint8_t rgb[3])
{
    double v[3];
    sh_unrounded(coef, degree, cam, pos, v);
    for (int c = 0; c < 3; c++) rgb[c] = clamped_u8(v[c]);
}

// The camera in object space: the inverse of the affine model-view matrix (column-major, p_cam = A p + t) applied to the
// origin, -A^-1 t, by the cofactors of A in this fixed order, in f64 from the f32 uniforms.  False when A is singular
// (determinant 0 or not finite).
inline bool camera_in_object(const float mv[16], double out[3])
{
    const double a00 = mv[0], a10 = mv[1], a20 = mv[2], a01 = mv[4], a11 = mv[5], a21 = mv[6], a02 = mv[8], a12 = mv[9], a22 = mv[10];
    const double t0 = mv[12], t1 = mv[13], t2 = mv[14];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;   // cofactors of row 0
    const double c10 = a02 * a21 - a01 * a22, c11 = a00 * a22 - a02 * a20, c12 = a01 * a20 - a00 * a21;
    const double c20 = a01 * a12 - a02 * a11, c21 = a02 * a10 - a00 * a12, c22 = a00 * a11 - a01 * a10;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    out[0] = out[1] = out[2] = 0.0;
    if (det == 0.0 || !(fabs(det) <= 1.7976931348623157e308)) return false;
    // A^-1 = adj(A) / det, adj(A)[i][j] = cofactor c_ji
    out[0] = -(((c00 * t0 + c10 * t1) + c20 * t2) / det);
    out[1] = -(((c01 * t0 + c11 * t1) + c21 * t2) / det);
    out[2] = -(((c02 * t0 + c12 * t1) + c22 * t2) / det);
    return true;
}

}  // namespace gsm

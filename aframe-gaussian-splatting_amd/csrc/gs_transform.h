// gs_transform.h -- moving resident splats by a similarity p' = scale * R p + translation (include/gs_splat.h: gs_similarity,
// gs_transform), written once and called by the kernels (gs_transform.hip: k_transform_records, k_transform_sh) and by the host entry
// points (gs_host.cpp: gs_transform_record, gs_transform_sh_row, gs_sh_rotation, gs_similarity_about), so that both produce the same
// bytes by construction.
//
// Everything is IEEE f64 built from + - * / sqrt, rint, fabs and comparisons (all correctly rounded on the host and on gfx950), un-fused
// (-ffp-contract=off), on the f32 parameters widened (exact), in the order written out below.  The square roots -- the quaternion's norm
// and the sample directions of the SH matrices -- are taken on the host alone: the kernels are handed R, scale, scale^2, the translation
// and the band matrices as they are.  No array is indexed by a run-time value in the code the kernels run.
//
// Two spaces: the similarity is given in the ROWS' object space (a .ply / .splat row's positions); the packed record lives in the
// z-mirrored one (the centre texel is (x, y, -z), index.js:350-354, and the covariance was built from a quaternion whose z was negated,
// gs_device_math.h: pack_row).  With M = diag(1, 1, -1) the covariance therefore turns by Rm = M R M: R with the entries negated that
// have exactly one index equal to 2.
#pragma once
#include "gs_device_math.h"
#include "gs_sh.h"

namespace gsm {

// the parameters as the arithmetic takes them.  rot_identity: all nine entries of R compare equal to the identity's
struct TransformParams { double R[9] /* row-major, rows' space */, s, ss, t[3]; int rot_identity; };
// the band matrices D1 (3x3), D2 (5x5), D3 (7x7), row-major, in that order: sh'[c][k0 + i] = sum_j D_l[i][j] sh[c][k0 + j]
#define GS_SH_ROT_DOUBLES 83
struct ShRotation { double d[GS_SH_ROT_DOUBLES]; };

GS_HD bool transform_f32_finite(float f)                      // (decided on the bits: no NaN reaches a comparison)
{
    union { float f; uint32_t u; } cv; cv.f = f;
    return (cv.u & 0x7F800000u) != 0x7F800000u;
}

// false: a parameter is not finite, scale <= 0 or the quaternion's norm is 0 -- p is not to be used.  rotation = (w, x, y, z)
GS_HD bool transform_widen(const float rotation[4], float scale, const float translation[3], TransformParams &p)
{
    bool ok = transform_f32_finite(scale);
    for (int i = 0; i < 4; i++) ok = ok && transform_f32_finite(rotation[i]);
    for (int i = 0; i < 3; i++) ok = ok && transform_f32_finite(translation[i]);
    if (!ok || !(scale > 0.0f)) return false;
    double qw = (double)rotation[0], qx = (double)rotation[1], qy = (double)rotation[2], qz = (double)rotation[3];
    const double n = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    if (n == 0.0) return false;
    qw = qw / n; qx = qx / n; qy = qy / n; qz = qz / n;
    // Matrix4.makeRotationFromQuaternion, the very expressions of pack_row (r_ij: row i, column j)
    const double x2 = qx + qx, y2 = qy + qy, z2 = qz + qz;
    const double xx = qx * x2, xy = qx * y2, xz = qx * z2;
    const double yy = qy * y2, yz = qy * z2, zz = qz * z2;
    const double wx = qw * x2, wy = qw * y2, wz = qw * z2;
    const double r00 = 1 - (yy + zz), r10 = xy + wz, r20 = xz - wy;
    const double r01 = xy - wz, r11 = 1 - (xx + zz), r21 = yz + wx;
    const double r02 = xz + wy, r12 = yz - wx, r22 = 1 - (xx + yy);
    p.R[0] = r00; p.R[1] = r01; p.R[2] = r02;
    p.R[3] = r10; p.R[4] = r11; p.R[5] = r12;
    p.R[6] = r20; p.R[7] = r21; p.R[8] = r22;
    p.rot_identity = (r00 == 1.0 && r01 == 0.0 && r02 == 0.0 && r10 == 0.0 && r11 == 1.0 && r12 == 0.0 && r20 == 0.0 && r21 == 0.0 && r22 == 1.0) ? 1 : 0;
    p.s = (double)scale;
    p.ss = p.s * p.s;
    for (int i = 0; i < 3; i++) p.t[i] = (double)translation[i];
    return true;
}

// the strip bound of a record whose scale word is cs3: the expression of the pack kernel (gs_pack.hip: k_pack), f32
GS_HD float transform_bound(float cs3)
{
    const float mx = cs3 * 32767.0f;
    return (mx == mx && mx < 3.0e37f) ? sqrtf(3.0f * mx) * 1.001f : INFINITY;
}

// one int16 half of the new covariance: e * 32767 / max_value rounded to nearest, ties to even; clamped; NaN -> 0
GS_HD uint32_t transform_half(double e, double max_value)
{
    double v = rint(e * 32767.0 / max_value);
    if (!(v == v)) v = 0.0;
    if (v > 32767.0) v = 32767.0;
    if (v < -32767.0) v = -32767.0;
    return (uint32_t)(uint16_t)(int16_t)(int32_t)v;
}

// THE RECORD RULE.  cs, cc: the record as GS_BUF_CENTER_SCALE / GS_BUF_COV_COLOR return it; sort_row: its GS_BUF_SORT_ROWS row.
// The outputs may be the inputs.
GS_HD void transform_record(const float cs[4], const uint32_t cc[4], const float sort_row[4], const TransformParams &p,
                            float cs_out[4], uint32_t cc_out[4], float sort_row_out[4], float &bound_out)
{
    const double *R = p.R;
    // position: out of the mirrored space, through the similarity, back
    const double p0 = (double)cs[0], p1 = (double)cs[1], p2 = -(double)cs[2];
    const double n0 = p.s * ((R[0] * p0 + R[1] * p1) + R[2] * p2) + p.t[0];
    const double n1 = p.s * ((R[3] * p0 + R[4] * p1) + R[5] * p2) + p.t[1];
    const double n2 = p.s * ((R[6] * p0 + R[7] * p1) + R[8] * p2) + p.t[2];
    const float c0 = (float)n0, c1 = (float)n1, c2 = (float)(-n2);
    const float scl = cs[3], size = sort_row[3];
    const uint32_t w0 = cc[0], w1 = cc[1], w2 = cc[2], rgba = cc[3];
    float scl_out = scl;
    uint32_t o0 = w0, o1 = w1, o2 = w2;
    if (!transform_f32_finite(scl)) {
        // (a record without a finite scale word keeps it, and its int16 words)
    } else if (p.rot_identity) {
        // a pure translation never touches the covariance, a pure scale never touches the int16 words
        if (!(p.s == 1.0)) scl_out = (float)((double)scl * p.ss);
    } else {
        const double s = (double)scl;
        // the symmetric matrix of export_row (gs_export.h): pack_row's layout, elements[0], [1], [2] | [5], [6] | [10]
        const double a00 = (double)(int16_t)(w0 & 0xFFFFu) * s, a01 = (double)(int16_t)(w0 >> 16) * s, a02 = (double)(int16_t)(w1 & 0xFFFFu) * s;
        const double a11 = (double)(int16_t)(w1 >> 16) * s, a12 = (double)(int16_t)(w2 & 0xFFFFu) * s, a22 = (double)(int16_t)(w2 >> 16) * s;
        // Rm = M R M: negated where exactly one index is 2
        const double m00 = R[0], m01 = R[1], m02 = -R[2];
        const double m10 = R[3], m11 = R[4], m12 = -R[5];
        const double m20 = -R[6], m21 = -R[7], m22 = R[8];
        // B = Rm A
        const double b00 = (m00 * a00 + m01 * a01) + m02 * a02, b01 = (m00 * a01 + m01 * a11) + m02 * a12, b02 = (m00 * a02 + m01 * a12) + m02 * a22;
        const double b10 = (m10 * a00 + m11 * a01) + m12 * a02, b11 = (m10 * a01 + m11 * a11) + m12 * a12, b12 = (m10 * a02 + m11 * a12) + m12 * a22;
        const double b20 = (m20 * a00 + m21 * a01) + m22 * a02, b21 = (m20 * a01 + m21 * a11) + m22 * a12, b22 = (m20 * a02 + m21 * a12) + m22 * a22;
        // E = (B Rm^T) scale^2, the six entries in pack_row's order
        const double e0 = ((b00 * m00 + b01 * m01) + b02 * m02) * p.ss;   // (0, 0)
        const double e1 = ((b10 * m00 + b11 * m01) + b12 * m02) * p.ss;   // (1, 0)
        const double e2 = ((b20 * m00 + b21 * m01) + b22 * m02) * p.ss;   // (2, 0)
        const double e3 = ((b10 * m10 + b11 * m11) + b12 * m12) * p.ss;   // (1, 1)
        const double e4 = ((b20 * m10 + b21 * m11) + b22 * m12) * p.ss;   // (2, 1)
        const double e5 = ((b20 * m20 + b21 * m21) + b22 * m22) * p.ss;   // (2, 2)
        double max_value = 0.0;
        if (fabs(e0) > max_value) max_value = fabs(e0);
        if (fabs(e1) > max_value) max_value = fabs(e1);
        if (fabs(e2) > max_value) max_value = fabs(e2);
        if (fabs(e3) > max_value) max_value = fabs(e3);
        if (fabs(e4) > max_value) max_value = fabs(e4);
        if (fabs(e5) > max_value) max_value = fabs(e5);
        scl_out = (float)(max_value / 32767.0);
        o0 = transform_half(e0, max_value) | (transform_half(e1, max_value) << 16);
        o1 = transform_half(e2, max_value) | (transform_half(e3, max_value) << 16);
        o2 = transform_half(e4, max_value) | (transform_half(e5, max_value) << 16);
    }
    cs_out[0] = c0; cs_out[1] = c1; cs_out[2] = c2; cs_out[3] = scl_out;
    cc_out[0] = o0; cc_out[1] = o1; cc_out[2] = o2; cc_out[3] = rgba;
    sort_row_out[0] = c0; sort_row_out[1] = c1; sort_row_out[2] = c2; sort_row_out[3] = (float)((double)size * p.s);
    bound_out = transform_bound(scl_out);
}

// THE SH RULE: one channel of a row of degree DEG, all K inputs read before an output is written (out may be in).  Band l occupies
// k = l^2 .. l^2 + 2 l; band 0 is unchanged.  in, out: at least (DEG + 1)^2 floats
template <int DEG>
GS_HD void transform_sh_channel(const float *in, const ShRotation &rot, float *out)
{
    constexpr int K = (DEG + 1) * (DEG + 1);
    double v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = (double)in[k];
#pragma unroll
    for (int l = 1; l <= DEG; l++) {
        const int k0 = l * l, w = 2 * l + 1, base = l == 1 ? 0 : (l == 2 ? 9 : 34);
#pragma unroll
        for (int i = 0; i < w; i++) {
            double acc = rot.d[base + i * w] * v[k0];
#pragma unroll
            for (int j = 1; j < w; j++) acc = acc + rot.d[base + i * w + j] * v[k0 + j];
            out[k0 + i] = (float)acc;
        }
    }
    out[0] = in[0];
}

// ---------------------------------------------------------------- host only: the band matrices

// the basis of band l (1..3) at the unit vector (x, y, z), exactly as sh_unrounded (gs_sh.h) orders and signs it
inline void sh_band_basis(int l, double x, double y, double z, double *b)
{
    const double SH_C1 = 0.4886025119029199;
    const double SH_C2_0 = 1.0925484305920792, SH_C2_1 = -1.0925484305920792, SH_C2_2 = 0.31539156525252005;
    const double SH_C2_3 = -1.0925484305920792, SH_C2_4 = 0.5462742152960396;
    const double SH_C3_0 = -0.5900435899266435, SH_C3_1 = 2.890611442640554, SH_C3_2 = -0.4570457994644658;
    const double SH_C3_3 = 0.3731763325901154, SH_C3_4 = -0.4570457994644658, SH_C3_5 = 1.445305721320277;
    const double SH_C3_6 = -0.5900435899266435;
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    if (l == 1) {
        b[0] = -SH_C1 * y; b[1] = SH_C1 * z; b[2] = -SH_C1 * x;
    } else if (l == 2) {
        b[0] = SH_C2_0 * xy; b[1] = SH_C2_1 * yz; b[2] = SH_C2_2 * ((2.0 * zz - xx) - yy); b[3] = SH_C2_3 * xz; b[4] = SH_C2_4 * (xx - yy);
    } else {
        b[0] = (SH_C3_0 * y) * (3.0 * xx - yy); b[1] = (SH_C3_1 * xy) * z; b[2] = (SH_C3_2 * y) * ((4.0 * zz - xx) - yy);
        b[3] = (SH_C3_3 * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy); b[4] = (SH_C3_4 * x) * ((4.0 * zz - xx) - yy);
        b[5] = (SH_C3_5 * z) * (xx - yy); b[6] = (SH_C3_6 * x) * (xx - 3.0 * yy);
    }
}

// D_l for the rotation R of p.  The rotated row has to show direction R d what the old one showed direction d: with b(d) the band's
// basis, b(d')^T D = b(R^T d')^T for every unit d'.  Written down at 2 l + 1 fixed sample directions d_j (rows of Y: b(d_j), rows of
// Z: b(R^T d_j)) that is Y D = Z, solved by Gauss-Jordan elimination with partial pivoting (the pivots depend on Y alone: the same
// for every call).  The directions were chosen among small integer vectors for a well conditioned Y (condition numbers 1, 1.9, 2.6).
// An exact identity R gives exact identity matrices.
inline void sh_rotation(const TransformParams &p, ShRotation &rot)
{
    static const int dirs1[3][3] = { { 0, 0, 1 }, { 1, 0, 0 }, { 0, 1, 0 } };
    static const int dirs2[5][3] = { { -1, 2, -3 }, { -2, 2, 0 }, { 0, -1, 0 }, { -3, -3, 3 }, { -1, 1, 2 } };
    static const int dirs3[7][3] = { { 0, 2, -3 }, { 3, 1, 0 }, { 2, -1, 2 }, { -1, 0, -2 }, { 3, 3, 2 }, { -3, -1, 3 }, { -2, -2, 1 } };
    const double *R = p.R;
    int base = 0;
    for (int l = 1; l <= 3; l++) {
        const int w = 2 * l + 1;
        double *D = rot.d + base;
        base += w * w;
        if (p.rot_identity) {
            for (int i = 0; i < w; i++) for (int j = 0; j < w; j++) D[i * w + j] = i == j ? 1.0 : 0.0;
            continue;
        }
        double Y[7][7], Z[7][7];
        for (int j = 0; j < w; j++) {
            const int *dv = l == 1 ? dirs1[j] : (l == 2 ? dirs2[j] : dirs3[j]);
            const double dx = (double)dv[0], dy = (double)dv[1], dz = (double)dv[2];
            const double len = sqrt((dx * dx + dy * dy) + dz * dz);
            const double x = dx / len, y = dy / len, z = dz / len;
            sh_band_basis(l, x, y, z, Y[j]);
            // R^T d: column i of R against d
            const double tx = (R[0] * x + R[3] * y) + R[6] * z, ty = (R[1] * x + R[4] * y) + R[7] * z, tz = (R[2] * x + R[5] * y) + R[8] * z;
            sh_band_basis(l, tx, ty, tz, Z[j]);
        }
        for (int c = 0; c < w; c++) {
            int piv = c;
            for (int r = c + 1; r < w; r++) if (fabs(Y[r][c]) > fabs(Y[piv][c])) piv = r;
            if (piv != c)
                for (int k = 0; k < w; k++) {
                    const double ty = Y[c][k]; Y[c][k] = Y[piv][k]; Y[piv][k] = ty;
                    const double tz = Z[c][k]; Z[c][k] = Z[piv][k]; Z[piv][k] = tz;
                }
            const double d = Y[c][c];
            for (int k = 0; k < w; k++) { Y[c][k] = Y[c][k] / d; Z[c][k] = Z[c][k] / d; }
            for (int r = 0; r < w; r++) {
                if (r == c) continue;
                const double f = Y[r][c];
                for (int k = 0; k < w; k++) { Y[r][k] = Y[r][k] - f * Y[c][k]; Z[r][k] = Z[r][k] - f * Z[c][k]; }
            }
        }
        for (int i = 0; i < w; i++) for (int j = 0; j < w; j++) D[i * w + j] = Z[i][j];
    }
}


}  // namespace gsm

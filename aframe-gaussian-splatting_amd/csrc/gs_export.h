// gs_export.h -- a packed record back to a .splat row (include/gs_splat.h: gs_export_row spells the rule out), written once and
// called by the export kernel (gs_export.hip: k_export_scatter) and by the host entry point (gs_host.cpp: gs_export_row), so that
// both produce the same bytes by construction.
//
// pack_row (gs_device_math.h, index.js:343-402) folds scale and rotation into six int16 covariance entries times cs[3] and keeps
// neither; a row needs three scales and a quaternion again: the eigen-decomposition of a symmetric 3x3 matrix.  Everything is IEEE
// f64 built from + - * / sqrt, fabs and comparisons only (all correctly rounded on the host and on gfx950), un-fused
// (-ffp-contract=off), in the order written out below.  No array is indexed by a run-time value: every matrix entry is a
// named scalar, so the kernel keeps them in registers (no LDS, no private memory).
#pragma once
#include "gs_ply.h"                                               // clamped_u8: the Uint8ClampedArray store (index.js:704-707)

#define GS_EXPORT_SWEEPS 8

namespace gsm {

// One Jacobi rotation in the (p, q) plane of the symmetric matrix (r: the third index); vp, vq: the accumulated vectors' columns.
// Skipped when the off-diagonal entry is exactly 0.  theta = +-inf (a tiny apq) gives t = +-0, c = 1: no NaN arises from finite entries.
GS_PLY_HD void export_jacobi(double &app, double &aqq, double &apq, double &arp, double &arq,
                             double &v0p, double &v0q, double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (apq + apq);
    const double root = sqrt(theta * theta + 1.0);
    const double t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (root - theta);   // sgn(theta) / (|theta| + sqrt(theta^2 + 1))
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h; aqq = aqq + h; apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq; arq = s * rp + c * rq;
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

GS_PLY_HD void export_swap(double &a, double &b) { const double t = a; a = b; b = t; }

// cs, cc: the record as GS_BUF_CENTER_SCALE / GS_BUF_COV_COLOR return it.  row: the 32-byte row as 8 little-endian words.
// wide (may be null): scale[3], then the quaternion (w, x, y, z as a row stores it) as f32, before the byte rounding.
GS_PLY_HD void export_row(const float cs[4], const uint32_t cc[4], uint32_t row[8], float *wide)
{
    union { float f; uint32_t u; } cv;
    cv.f = cs[0]; row[0] = cv.u; cv.f = cs[1]; row[1] = cv.u; cv.f = -cs[2]; row[2] = cv.u;      // the inverse of index.js:350-354
    row[6] = cc[3];
    cv.f = cs[3];
    const uint32_t sbits = cv.u;
    const bool finite = (sbits & 0x7F800000u) != 0x7F800000u;    // (decided on the bits: no NaN reaches a comparison)
    const bool empty = (cc[0] | cc[1] | cc[2]) == 0u || (sbits & 0x7FFFFFFFu) == 0u;
    float sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f;
    double qw = 1.0, qx = 0.0, qy = 0.0, qz = 0.0;               // the stored quaternion: b0 = w, b1 = x, b2 = y, b3 = z (z negated already)
    if (!finite) { sc0 = sc1 = sc2 = cs[3]; }
    else if (!empty) {
        const double s = (double)cs[3];
        // pack_row's layout: elements[0], [1], [2] | [5], [6] | [10] of the column-major symmetric matrix
        double a00 = (double)(int16_t)(cc[0] & 0xFFFFu) * s, a01 = (double)(int16_t)(cc[0] >> 16) * s, a02 = (double)(int16_t)(cc[1] & 0xFFFFu) * s;
        double a11 = (double)(int16_t)(cc[1] >> 16) * s, a12 = (double)(int16_t)(cc[2] & 0xFFFFu) * s, a22 = (double)(int16_t)(cc[2] >> 16) * s;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int sweep = 0; sweep < GS_EXPORT_SWEEPS; sweep++) {
            export_jacobi(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), r = 2
            export_jacobi(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), r = 1
            export_jacobi(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), r = 0
        }
        double l0 = a00 > 0.0 ? a00 : 0.0, l1 = a11 > 0.0 ? a11 : 0.0, l2 = a22 > 0.0 ? a22 : 0.0;
        // descending, ties keep the Jacobi order: three adjacent exchanges on strict comparisons
        if (l0 < l1) { export_swap(l0, l1); export_swap(v00, v01); export_swap(v10, v11); export_swap(v20, v21); }
        if (l1 < l2) { export_swap(l1, l2); export_swap(v01, v02); export_swap(v11, v12); export_swap(v21, v22); }
        if (l0 < l1) { export_swap(l0, l1); export_swap(v00, v01); export_swap(v10, v11); export_swap(v20, v21); }
        const double det = (v00 * (v11 * v22 - v12 * v21) - v01 * (v10 * v22 - v12 * v20)) + v02 * (v10 * v21 - v11 * v20);
        if (det < 0.0) { v02 = -v02; v12 = -v12; v22 = -v22; }
        sc0 = (float)sqrt(l0); sc1 = (float)sqrt(l1); sc2 = (float)sqrt(l2);
        // Sigma = R^T diag(s^2) R with R the matrix pack_row builds (makeRotationFromQuaternion): row k of R is eigenvector k
        const double r00 = v00, r01 = v10, r02 = v20, r10 = v01, r11 = v11, r12 = v21, r20 = v02, r21 = v12, r22 = v22;
        const double tr = (r00 + r11) + r22;
        double w, x, y, z;
        if (tr >= r00 && tr >= r11 && tr >= r22) {
            const double S = sqrt(tr + 1.0) * 2.0;
            w = S / 4.0; x = (r21 - r12) / S; y = (r02 - r20) / S; z = (r10 - r01) / S;
        } else if (r00 >= r11 && r00 >= r22) {
            const double S = sqrt(((1.0 + r00) - r11) - r22) * 2.0;
            w = (r21 - r12) / S; x = S / 4.0; y = (r01 + r10) / S; z = (r02 + r20) / S;
        } else if (r11 >= r22) {
            const double S = sqrt(((1.0 + r11) - r00) - r22) * 2.0;
            w = (r02 - r20) / S; x = (r01 + r10) / S; y = S / 4.0; z = (r12 + r21) / S;
        } else {
            const double S = sqrt(((1.0 + r22) - r00) - r11) * 2.0;
            w = (r10 - r01) / S; x = (r02 + r20) / S; y = (r12 + r21) / S; z = S / 4.0;
        }
        // canonical sign: w > 0, or else the first non-zero of x, y, z positive
        const bool neg = w < 0.0 || (w == 0.0 && (x < 0.0 || (x == 0.0 && (y < 0.0 || (y == 0.0 && z < 0.0)))));
        if (neg) { w = -w; x = -x; y = -y; z = -z; }
        qw = w; qx = x; qy = y; qz = -z;                         // b3 = -z (index.js:344-349)
    }
    cv.f = sc0; row[3] = cv.u; cv.f = sc1; row[4] = cv.u; cv.f = sc2; row[5] = cv.u;
    row[7] = (uint32_t)clamped_u8(qw * 128.0 + 128.0) | ((uint32_t)clamped_u8(qx * 128.0 + 128.0) << 8) |
             ((uint32_t)clamped_u8(qy * 128.0 + 128.0) << 16) | ((uint32_t)clamped_u8(qz * 128.0 + 128.0) << 24);
    if (wide) {
        wide[0] = sc0; wide[1] = sc1; wide[2] = sc2;
        wide[3] = (float)qw; wide[4] = (float)qx; wide[5] = (float)qy; wide[6] = (float)qz;
    }
}

}  // namespace gsm

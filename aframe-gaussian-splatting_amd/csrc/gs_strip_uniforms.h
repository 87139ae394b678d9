// gs_strip_uniforms.h -- the uniforms of gs_sort_for's reach test (gsm::strip_may_touch, gs_device_math.h), filled on the host.
// Plain C++, no HIP: gs_sort.hip calls it per strip sort, tests/host_check compiles it to check the bound on the CPU.
#pragma once
#include <math.h>
#include <string.h>
#include "gs_device_math.h"

// An upper bound of ||A||_2, A = mat3 of the column-major 4x4 matrix mv, that needs no start vector: with B = A^T A (symmetric,
// positive semi-definite, eigenvalues l1 >= l2 >= l3 >= 0)
//     l1^64 <= tr(B^64) = l1^64 + l2^64 + l3^64 <= 3 l1^64,
// so tr(B^64)^(1/128) lies in [||A||_2, 3^(1/128) ||A||_2] = [1, 1.00862] ||A||_2 for EVERY A.  B^64 comes from six squarings, each
// divided by its trace t_k so that nothing over- or underflows (the trace of a square of a PSD matrix of trace 1 is in [1/3, 1]):
// tr(B^64) = t_0^64 t_1^32 ... t_6^1.  f64 throughout (relative error ~1e-14); 1.0001 on top covers that and the rounding to f32.
// A zero matrix gives 0; a matrix with an entry that is not finite gives NaN (the caller then keeps every splat).
// (Before: 64 power iterations from (1, 0.7, 0.4) + 2 % -- which returned 0.887 of the norm for singular values (1.15, 1, 1) with the top
// right-singular vector orthogonal to that start: docs/LAB_NOTES.md 9j, tests/test_reach_cpu.py.)
static inline float gs_norm_bound(const float *mv)
{
    double c[3][3], t[7];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
        c[i][j] = 0.0;
        for (int r = 0; r < 3; r++) c[i][j] += (double)mv[4 * i + r] * (double)mv[4 * j + r];
    }
    t[0] = c[0][0] + c[1][1] + c[2][2];
    if (!(t[0] <= 1.7e308)) return NAN;                       // an Inf or NaN entry (a finite f32 squared is far below)
    if (!(t[0] > 0.0)) return 0.0f;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) c[i][j] /= t[0];
    for (int k = 1; k <= 6; k++) {
        double q[3][3];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) q[i][j] = (c[i][0] * c[0][j] + c[i][1] * c[1][j]) + c[i][2] * c[2][j];
        t[k] = q[0][0] + q[1][1] + q[2][2];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) c[i][j] = q[i][j] / t[k];
    }
    double r = t[6];                                          // tr(B^64)^(1/64) = t_0 sqrt(t_1 sqrt(t_2 ... sqrt(t_6)))
    for (int k = 5; k >= 1; k--) r = t[k] * sqrt(r);
    return (float)(sqrt(t[0] * sqrt(r)) * 1.0001);
}

// su for the strip [x0, x1) of a vw x vh frame drawn with (mv, proj, focal); returns has_strip: 0 = the test cannot be trusted for
// these uniforms (a matrix entry that is not finite, no focal length, an empty strip) and the sort keeps every splat.
static inline int gs_fill_strip_uniforms(const float *mv, const float *proj, float focal, float vw, float vh, int x0, int x1, gsm::StripUniforms &su)
{
    memset(&su, 0, sizeof su);
    for (int k = 0; k < 4; k++) { su.mvr0[k] = mv[4 * k]; su.mvr1[k] = mv[4 * k + 1]; su.mvr2[k] = mv[4 * k + 2]; su.pr0[k] = proj[4 * k]; su.pr1[k] = proj[4 * k + 1]; su.pr3[k] = proj[4 * k + 3]; }
    su.norm_a = gs_norm_bound(mv);
    su.focal = focal; su.half_w = 0.5f * vw; su.sx0 = (float)x0; su.sx1 = (float)x1;
    su.half_h = 0.5f * vh; su.sy1 = vh > 0.0f ? vh : 0.0f;
    return (su.norm_a <= 3.402823466e+38f && su.focal > 0.0f && x1 > x0) ? 1 : 0;
}

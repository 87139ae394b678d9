// gs_host.cpp -- host-side pieces of the boundary that are not on the per-frame GPU path:
//   * the uniform producers (tick / getModelViewMatrix / getProjectionMatrix, index.js:438-487): a dozen 4x4
//     f64 operations per frame, in three.js' operation order so the f32 uniforms match the reference's;
//   * processPlyBuffer (index.js:600-745): the one-time .ply -> .splat row conversion;
//   * view-dependent colour (gs_sh.h): the SH rows of a .ply in the converter's order, one colour on the host, and the
//     camera position the projection kernel evaluates them for;
//   * the chunked compressed .ply (include/gs_splat.h: "Compressed .ply"; at the end of this file): the strict header reader both
//     directions share (gs_cply_plan), the host evaluators of the decode and of the writer (gs_cply_to_splat, gs_cply_sh_host,
//     gs_splat_to_cply) and gs_log_fixed.  The per-splat arithmetic is gs_cply.h's, the functions the kernels call (gs_cply.hip).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/gs_splat.h"
#include "gs_ply.h"
#include "gs_sh.h"
#include "gs_device_math.h"
#include "gs_export.h"
#include "gs_adjust.h"
#include "gs_transform.h"
#include "gs_cply.h"

namespace {

// three.js Matrix4.multiplyMatrices: o = a * b, column-major, each element summed left to right
void mat_mul(const double *a, const double *b, double *o)
{
    double r[16];
    for (int c = 0; c < 4; c++)
        for (int rw = 0; rw < 4; rw++)
            r[c * 4 + rw] = a[rw] * b[c * 4] + a[4 + rw] * b[c * 4 + 1] + a[8 + rw] * b[c * 4 + 2] + a[12 + rw] * b[c * 4 + 3];
    memcpy(o, r, sizeof r);
}

// three.js Matrix4.invert (cofactor expansion in three.js' term order; det == 0 -> zero matrix)
void mat_inv(const double *m, double *o)
{
    const double n11 = m[0], n21 = m[1], n31 = m[2], n41 = m[3], n12 = m[4], n22 = m[5], n32 = m[6], n42 = m[7];
    const double n13 = m[8], n23 = m[9], n33 = m[10], n43 = m[11], n14 = m[12], n24 = m[13], n34 = m[14], n44 = m[15];
    const double t11 = n23 * n34 * n42 - n24 * n33 * n42 + n24 * n32 * n43 - n22 * n34 * n43 - n23 * n32 * n44 + n22 * n33 * n44;
    const double t12 = n14 * n33 * n42 - n13 * n34 * n42 - n14 * n32 * n43 + n12 * n34 * n43 + n13 * n32 * n44 - n12 * n33 * n44;
    const double t13 = n13 * n24 * n42 - n14 * n23 * n42 + n14 * n22 * n43 - n12 * n24 * n43 - n13 * n22 * n44 + n12 * n23 * n44;
    const double t14 = n14 * n23 * n32 - n13 * n24 * n32 - n14 * n22 * n33 + n12 * n24 * n33 + n13 * n22 * n34 - n12 * n23 * n34;
    const double det = n11 * t11 + n21 * t12 + n31 * t13 + n41 * t14;
    if (det == 0) { for (int i = 0; i < 16; i++) o[i] = 0; return; }
    const double s = 1 / det;
    double r[16];
    r[0] = t11 * s;
    r[1] = (n24 * n33 * n41 - n23 * n34 * n41 - n24 * n31 * n43 + n21 * n34 * n43 + n23 * n31 * n44 - n21 * n33 * n44) * s;
    r[2] = (n22 * n34 * n41 - n24 * n32 * n41 + n24 * n31 * n42 - n21 * n34 * n42 - n22 * n31 * n44 + n21 * n32 * n44) * s;
    r[3] = (n23 * n32 * n41 - n22 * n33 * n41 - n23 * n31 * n42 + n21 * n33 * n42 + n22 * n31 * n43 - n21 * n32 * n43) * s;
    r[4] = t12 * s;
    r[5] = (n13 * n34 * n41 - n14 * n33 * n41 + n14 * n31 * n43 - n11 * n34 * n43 - n13 * n31 * n44 + n11 * n33 * n44) * s;
    r[6] = (n14 * n32 * n41 - n12 * n34 * n41 - n14 * n31 * n42 + n11 * n34 * n42 + n12 * n31 * n44 - n11 * n32 * n44) * s;
    r[7] = (n12 * n33 * n41 - n13 * n32 * n41 + n13 * n31 * n42 - n11 * n33 * n42 - n12 * n31 * n43 + n11 * n32 * n43) * s;
    r[8] = t13 * s;
    r[9] = (n14 * n23 * n41 - n13 * n24 * n41 - n14 * n21 * n43 + n11 * n24 * n43 + n13 * n21 * n44 - n11 * n23 * n44) * s;
    r[10] = (n12 * n24 * n41 - n14 * n22 * n41 + n14 * n21 * n42 - n11 * n24 * n42 - n12 * n21 * n44 + n11 * n22 * n44) * s;
    r[11] = (n13 * n22 * n41 - n12 * n23 * n41 - n13 * n21 * n42 + n11 * n23 * n42 + n12 * n21 * n43 - n11 * n22 * n43) * s;
    r[12] = t14 * s;
    r[13] = (n13 * n24 * n31 - n14 * n23 * n31 + n14 * n21 * n33 - n11 * n24 * n33 - n13 * n21 * n34 + n11 * n23 * n34) * s;
    r[14] = (n14 * n22 * n31 - n12 * n24 * n31 - n14 * n21 * n32 + n11 * n24 * n32 + n12 * n21 * n34 - n11 * n22 * n34) * s;
    r[15] = (n12 * n23 * n31 - n13 * n22 * n31 + n13 * n21 * n32 - n11 * n23 * n32 - n12 * n21 * n33 + n11 * n22 * n33) * s;
    memcpy(o, r, sizeof r);
}

// conjugation by S = diag(1,-1,1,1) as the reference spells it (index.js:472-476, 479-483)
void flip_y(double *e) { e[1] *= -1.0; e[4] *= -1.0; e[6] *= -1.0; e[9] *= -1.0; e[13] *= -1.0; }

// ---------------------------------------------------------------- PLY

typedef gsm::PlyType PType;
const size_t kSize[] = { 8, 4, 4, 4, 2, 2, 1, 1 };

struct Prop { std::string name; PType type; size_t offset; };

struct Header {
    std::vector<Prop> props;
    size_t row_bytes = 0, data_start = 0, vertex_count = 0;
    const Prop *find(const char *name) const
    {
        const Prop *hit = nullptr;
        for (const Prop &p : props) if (p.name == name) hit = &p;     // later duplicates win (JS object assignment)
        return hit;
    }
};

PType parse_type(const std::string &t)       // TYPE_MAP, anything else reads as getInt8 (index.js:613-628)
{
    if (t == "double") return gsm::PLY_F64; if (t == "int") return gsm::PLY_I32; if (t == "uint") return gsm::PLY_U32;
    if (t == "float") return gsm::PLY_F32; if (t == "short") return gsm::PLY_I16; if (t == "ushort") return gsm::PLY_U16;
    if (t == "uchar") return gsm::PLY_U8;
    return gsm::PLY_I8;
}

int fail(char *err, size_t errlen, int code, const char *fmt, const char *arg = "")
{
    if (err && errlen) snprintf(err, errlen, fmt, arg);
    return code;
}

int parse_header(const uint8_t *buf, size_t len, Header &h, char *err, size_t errlen)
{
    const size_t hl = std::min<size_t>(len, 10240);                  // "10KB ought to be enough for a header"
    const std::string head((const char *)buf, hl);
    const size_t end = head.find("end_header\n");
    if (end == std::string::npos) return fail(err, errlen, GS_E_PLY_HEADER, "Unable to read .ply file header");
    // /element vertex (\d+)\n/ over the decoded 10 KiB
    bool have_count = false;
    for (size_t at = head.find("element vertex "); at != std::string::npos && !have_count; at = head.find("element vertex ", at + 1)) {
        size_t j = at + 15, v = 0, nd = 0;
        while (j < hl && head[j] >= '0' && head[j] <= '9') { v = v * 10 + (size_t)(head[j] - '0'); j++; nd++; }
        if (nd && j < hl && head[j] == '\n') { h.vertex_count = v; have_count = true; }
    }
    if (!have_count) return fail(err, errlen, GS_E_PLY_HEADER, "Unable to read .ply file header");
    size_t ls = 0;
    while (ls < end) {
        size_t le = head.find('\n', ls);
        if (le == std::string::npos || le > end) le = end;
        const std::string line = head.substr(ls, le - ls);
        if (line.compare(0, 9, "property ") == 0) {                  // const [p, type, name] = prop.split(" ")
            std::vector<std::string> parts;
            size_t s = 0;
            while (parts.size() < 3) {
                const size_t sp = line.find(' ', s);
                parts.push_back(line.substr(s, sp == std::string::npos ? std::string::npos : sp - s));
                if (sp == std::string::npos) break;
                s = sp + 1;
            }
            const PType t = parse_type(parts.size() > 1 ? parts[1] : "");
            h.props.push_back({ parts.size() > 2 ? parts[2] : "undefined", t, h.row_bytes });
            h.row_bytes += kSize[t];
        }
        ls = le + 1;
    }
    h.data_start = end + 11;
    return GS_OK;
}

}  // namespace

extern "C" {

GS_API void gs_model_view_matrix(const double cam_world[16], const double obj_world[16], double out[16])
{
    double view[16], m[16];
    memcpy(view, cam_world, sizeof view); flip_y(view);              // viewMatrix = camera.matrixWorld, flipped
    mat_inv(obj_world, m); flip_y(m);                                // mtx = object.matrixWorld^-1, flipped
    mat_mul(m, view, m);                                             // mtx.multiply(viewMatrix)
    mat_inv(m, out);                                                 // mtx.invert()
}

GS_API void gs_projection_matrix(const double proj[16], double out[16])
{
    memcpy(out, proj, 16 * sizeof(double));
    out[4] *= -1; out[5] *= -1; out[6] *= -1; out[7] *= -1;
}

GS_API void gs_tick_uniforms(const double cam_world[16], const double obj_world[16], const double *cutout_world, float view[4],
                             float cutout[16])
{
    double mv[16];
    gs_model_view_matrix(cam_world, obj_world, mv);
    view[0] = (float)mv[2]; view[1] = (float)mv[6]; view[2] = (float)mv[10]; view[3] = (float)mv[14];
    if (cutout_world && cutout) {
        double w[16];
        mat_inv(cutout_world, w);                                    // worldToCutout.copy(cutout.matrixWorld).invert()
        mat_mul(w, obj_world, w);                                    // .multiply(object.matrixWorld)
        for (int i = 0; i < 16; i++) cutout[i] = (float)w[i];
    }
}

GS_API double gs_focal(const double gs_proj[16], double viewport_h) { return (viewport_h / 2.0) * fabs(gs_proj[5]); }

GS_API void gs_scaled_size(int css_w, int css_h, double ratio, int *out_w, int *out_h)
{
    // renderer.setPixelRatio / xr.setFramebufferScaleFactor are only applied when the property is > 0
    // (index.js:10-15); three.js sizes the drawing buffer as floor(css * pixelRatio).
    if (ratio > 0) { css_w = (int)floor(css_w * ratio); css_h = (int)floor(css_h * ratio); }
    if (out_w) *out_w = css_w;
    if (out_h) *out_h = css_h;
}

// Header parse + resolution of every property processPlyBuffer reads, with the reference's error messages in the
// reference's order (index.js:606-607 header, :643 "<prop> not found").  Shared by the host converter below and the
// HIP converter (gs_ply.hip).
static int ply_plan(const void *bytes, size_t nbytes, gsm::PlyLayout *layout, size_t *nrows, size_t *data_start, char *err, size_t errlen)
{
    const uint8_t *buf = (const uint8_t *)bytes;
    Header h;
    int rc = parse_header(buf, nbytes, h, err, errlen);
    if (rc != GS_OK) return rc;
    const size_t n = h.vertex_count;
    if (n && h.row_bytes * n > nbytes - h.data_start)
        return fail(err, errlen, GS_E_PLY_DATA, "Offset is outside the bounds of the DataView");
    gsm::PlyLayout L;
    memset(&L, 0, sizeof L);
    L.row_bytes = (uint32_t)h.row_bytes;
    auto need = [&](int slot, const char *nm) -> bool {
        const Prop *p = h.find(nm);
        if (!p) { fail(err, errlen, GS_E_PLY_PROP, "%s not found", nm); return false; }
        L.offset[slot] = (uint32_t)p->offset; L.type[slot] = (uint8_t)p->type;
        return true;
    };
    L.has_scale = h.find("scale_0") != nullptr;
    L.has_dc = h.find("f_dc_0") != nullptr;
    L.has_opacity = h.find("opacity") != nullptr;
    *nrows = n; *data_start = h.data_start; *layout = L;
    // importance pass (index.js:656-664) touches scale_0..2 and opacity; it only runs when there are rows
    if (L.has_scale && n) {
        if (!need(gsm::PP_S0, "scale_0") || !need(gsm::PP_S1, "scale_1") || !need(gsm::PP_S2, "scale_2") || !need(gsm::PP_OPACITY, "opacity"))
            return GS_E_PLY_PROP;
    }
    if (!n) return GS_OK;
    // row pass (index.js:680-742)
    if (L.has_scale) {
        if (!need(gsm::PP_R0, "rot_0") || !need(gsm::PP_R1, "rot_1") || !need(gsm::PP_R2, "rot_2") || !need(gsm::PP_R3, "rot_3")) return GS_E_PLY_PROP;
        if (!need(gsm::PP_S0, "scale_0") || !need(gsm::PP_S1, "scale_1") || !need(gsm::PP_S2, "scale_2")) return GS_E_PLY_PROP;
    }
    if (!need(gsm::PP_X, "x") || !need(gsm::PP_Y, "y") || !need(gsm::PP_Z, "z")) return GS_E_PLY_PROP;
    if (L.has_dc) { if (!need(gsm::PP_C0, "f_dc_0") || !need(gsm::PP_C1, "f_dc_1") || !need(gsm::PP_C2, "f_dc_2")) return GS_E_PLY_PROP; }
    else { if (!need(gsm::PP_C0, "red") || !need(gsm::PP_C1, "green") || !need(gsm::PP_C2, "blue")) return GS_E_PLY_PROP; }
    if (L.has_opacity && !need(gsm::PP_OPACITY, "opacity")) return GS_E_PLY_PROP;
    *layout = L;
    return GS_OK;
}

// no C++ exception crosses the C ABI: the header strings and the order arrays below are the only host allocations
int gs_ply_plan(const void *bytes, size_t nbytes, gsm::PlyLayout *layout, size_t *nrows, size_t *data_start, char *err, size_t errlen)
{
    try { return ply_plan(bytes, nbytes, layout, nrows, data_start, err, errlen); }
    catch (...) { return fail(err, errlen, GS_E_OOM, "out of host memory while reading the .ply header"); }
}

static int ply_to_splat(const void *bytes, size_t nbytes, void *out_rows, size_t *out_nrows, char *err, size_t errlen)
{
    if (!bytes || !out_nrows) return fail(err, errlen, GS_E_BADARG, "gs_ply_to_splat: NULL argument");
    gsm::PlyLayout L;
    size_t n = 0, data_start = 0;
    // the size query (out_rows == NULL) stops where the reference would have thrown so far: header and importance pass
    int rc = gs_ply_plan(bytes, nbytes, &L, &n, &data_start, err, errlen);
    *out_nrows = n;
    if (rc != GS_OK) return rc;
    if (!out_rows || !n) return GS_OK;
    const uint8_t *data = (const uint8_t *)bytes + data_start;

    // importance = exp(s0)*exp(s1)*exp(s2) * sigmoid(opacity), stored f32; 0 when there is no scale_0 (index.js:653-664)
    std::vector<float> importance(n, 0.0f);
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    if (L.has_scale)
        for (size_t i = 0; i < n; i++) importance[i] = gsm::ply_importance(data + i * L.row_bytes, L);
    // sizeIndex.sort((b, a) => sizeList[a] - sizeList[b]): descending, stable (index.js:668)
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t b, uint32_t a) { return (double)importance[a] - (double)importance[b] < 0; });
    uint32_t *out = (uint32_t *)out_rows;
    for (size_t j = 0; j < n; j++) {                                  // index.js:680-742
        uint32_t w[8];
        gsm::ply_row(data + (size_t)order[j] * L.row_bytes, L, w);
        memcpy(out + 8 * j, w, 32);
    }
    return GS_OK;
}

// The spherical-harmonics rows of a PLY (gs_sh.h), in the order ply_to_splat emits the splat rows.  The degree a file
// carries follows from how many f_rest_* it declares (0 -> 0, 9 -> 1, 24 -> 2, 45 -> 3); any other count, a gap in the
// numbering or a missing f_dc_* means "no SH": degree -1, no rows, no error.
static int ply_sh(const void *bytes, size_t nbytes, int degree, float *out_sh, size_t *out_nrows, int *out_degree, char *err, size_t errlen)
{
    if (!bytes || !out_nrows || !out_degree) return fail(err, errlen, GS_E_BADARG, "gs_ply_sh: NULL argument");
    if (degree < 0 || degree > GS_SH_MAX_DEGREE) return fail(err, errlen, GS_E_BADARG, "gs_ply_sh: degree must be 0..3");
    *out_nrows = 0; *out_degree = -1;
    const uint8_t *buf = (const uint8_t *)bytes;
    gsm::PlyLayout L;
    size_t n = 0, data_start = 0;
    int rc = gs_ply_plan(bytes, nbytes, &L, &n, &data_start, err, errlen);
    if (rc != GS_OK) return rc;
    Header h;
    rc = parse_header(buf, nbytes, h, err, errlen);
    if (rc != GS_OK) return rc;
    size_t n_rest = 0;
    for (const Prop &p : h.props) if (p.name.compare(0, 7, "f_rest_") == 0) n_rest++;
    int file_degree = n_rest == 0 ? 0 : n_rest == 9 ? 1 : n_rest == 24 ? 2 : n_rest == 45 ? 3 : -1;
    const Prop *src[3][16];
    for (int c = 0; c < 3 && file_degree >= 0; c++) {
        char nm[32];
        snprintf(nm, sizeof nm, "f_dc_%d", c);
        if (!(src[c][0] = h.find(nm))) file_degree = -1;
        const int per = (int)n_rest / 3;                              // f_rest_* per channel in the file
        for (int k = 1; k <= per && file_degree >= 0; k++) {
            snprintf(nm, sizeof nm, "f_rest_%d", c * per + (k - 1));
            if (!(src[c][k] = h.find(nm))) file_degree = -1;
        }
    }
    if (file_degree < 0) return GS_OK;
    const int D = degree < file_degree ? degree : file_degree, K = gsm::sh_coefs(D);
    *out_degree = D; *out_nrows = n;
    if (!out_sh || !n) return GS_OK;
    const uint8_t *data = buf + data_start;
    // the converter's order (index.js:653-668): descending importance, ties stable
    std::vector<float> importance(n, 0.0f);
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    if (L.has_scale)
        for (size_t i = 0; i < n; i++) importance[i] = gsm::ply_importance(data + i * L.row_bytes, L);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t b, uint32_t a) { return (double)importance[a] - (double)importance[b] < 0; });
    for (size_t j = 0; j < n; j++) {
        const uint8_t *row = data + (size_t)order[j] * L.row_bytes;
        float *o = out_sh + j * 3 * (size_t)K;
        for (int c = 0; c < 3; c++)
            for (int k = 0; k < K; k++) o[c * K + k] = (float)gsm::ply_read(row + src[c][k]->offset, src[c][k]->type);
    }
    return GS_OK;
}

GS_API int gs_ply_to_splat(const void *bytes, size_t nbytes, void *out_rows, size_t *out_nrows, char *err, size_t errlen)
{
    try { return ply_to_splat(bytes, nbytes, out_rows, out_nrows, err, errlen); }
    catch (...) { return fail(err, errlen, GS_E_OOM, "out of host memory while converting the .ply"); }
}

GS_API int gs_ply_sh_host(const void *bytes, size_t nbytes, int degree, float *out_sh, size_t *out_nrows, int *out_degree, char *err, size_t errlen)
{
    try { return ply_sh(bytes, nbytes, degree, out_sh, out_nrows, out_degree, err, errlen); }
    catch (...) { return fail(err, errlen, GS_E_OOM, "out of host memory while reading the .ply coefficients"); }
}

GS_API int gs_sh_eval(const float *sh_row, int degree, const double cam[3], const float pos[3], uint8_t rgb[3])
{
    if (!sh_row || !cam || !pos || !rgb || degree < 0 || degree > GS_SH_MAX_DEGREE) return GS_E_BADARG;
    const gsm::ShRowPtr coef = { sh_row, gsm::sh_coefs(degree) };
    gsm::sh_color(coef, degree, cam, pos, rgb);
    return GS_OK;
}

GS_API int gs_sh_eval_unrounded(const float *sh_row, int degree, const double cam[3], const float pos[3], double out[3])
{
    if (!sh_row || !cam || !pos || !out || degree < 0 || degree > GS_SH_MAX_DEGREE) return GS_E_BADARG;
    const gsm::ShRowPtr coef = { sh_row, gsm::sh_coefs(degree) };
    gsm::sh_unrounded(coef, degree, cam, pos, out);
    return GS_OK;
}

GS_API int gs_antialias_factor(const float cov[3], float *out_c)
{
    if (!cov || !out_c) return GS_E_BADARG;
    float l1, l2;
    gsm::dilated_eigenvalues(cov[0], cov[1], cov[2], l1, l2);
    *out_c = gsm::antialias_factor(cov[0], cov[1], cov[2], l1, l2);
    return GS_OK;
}

// one packed record through the kernels' own projection (gsm::project_splat<PAR>), with gs_render's focal rule (gs_fill_uniforms)
GS_API int gs_project_record(const float cs[4], const uint32_t cc[4], const gs_render_params *p, float record[8], float *zwin, int *visible)
{
    if (!cs || !cc || !p || !record || !zwin || !visible) return GS_E_BADARG;
    if (p->fb_width <= 0 || p->fb_height <= 0) return GS_E_BADARG;
    const bool par = (p->flags & GS_RENDER_PARALLEL) != 0;
    if (par && !gsm::parallel_matrix_ok(p->projection)) return GS_E_BADARG;
    const float focal = p->focal > 0 ? p->focal : (float)(((double)p->fb_height / 2.0) * fabs((double)p->projection[5]));
    const float vw = (float)p->fb_width, vh = (float)p->fb_height;
    gsm::Projected o; gsm::ProjExtra x;
    memset(&o, 0, sizeof o); memset(&x, 0, sizeof x);
    const bool vis = par ? gsm::project_splat<true>(cs, cc, p->model_view, p->projection, focal, vw, vh, o, x)
                         : gsm::project_splat<false>(cs, cc, p->model_view, p->projection, focal, vw, vh, o, x);
    *visible = vis ? 1 : 0;
    memset(record, 0, 8 * sizeof(float));
    *zwin = 0.0f;
    if (vis) {
        memcpy(record, &o, 8 * sizeof(float));                       // (Projected is the record: cx, cy, ax, ay, bx, by, the colour word, alpha)
        *zwin = x.zndc * 0.5f + 0.5f;
    }
    return GS_OK;
}

// three.js Matrix4.makeOrthographic, WebGL coordinate system (z in [-1, 1]), in its operation order
GS_API int gs_ortho_matrix(double left, double right, double top, double bottom, double near_, double far_, double out[16])
{
    if (!out) return GS_E_BADARG;
    const double w = 1.0 / (right - left), h = 1.0 / (top - bottom), pp = 1.0 / (far_ - near_);
    const double x = (right + left) * w, y = (top + bottom) * h;
    const double z = (far_ + near_) * pp, zinv = -2.0 * pp;
    out[0] = 2.0 * w; out[4] = 0.0;     out[8] = 0.0;   out[12] = -x;
    out[1] = 0.0;     out[5] = 2.0 * h; out[9] = 0.0;   out[13] = -y;
    out[2] = 0.0;     out[6] = 0.0;     out[10] = zinv; out[14] = -z;
    out[3] = 0.0;     out[7] = 0.0;     out[11] = 0.0;  out[15] = 1.0;
    return GS_OK;
}

GS_API int gs_highlight_word(uint32_t rgba, uint32_t option_value, uint32_t *out)
{
    if (!out) return GS_E_BADARG;
    *out = (option_value >> 24) ? gsm::highlight_word(rgba, option_value) : rgba;   // (W = 0: the option is off)
    return GS_OK;
}

GS_API int gs_prop_eval(const float cs[4], const uint32_t cc[4], int prop, double *out)
{
    if (!cs || !cc || !out || !gsm::prop_valid(prop)) return GS_E_BADARG;
    *out = gsm::prop_value(cs, cc, prop);
    return GS_OK;
}

GS_API int gs_hist_bin(double v, double lo, double hi, uint32_t nbins, int32_t *out_bin)
{
    if (!out_bin || !(lo < hi) || !(fabs(lo) <= 1.7976931348623157e308) || !(fabs(hi) <= 1.7976931348623157e308) || nbins < 1 || nbins > GS_HIST_MAX_BINS)
        return GS_E_BADARG;
    *out_bin = gsm::hist_bin(v, lo, hi, (double)nbins / (hi - lo), nbins);
    return GS_OK;
}

// even-odd fill, pixel centres, f64; the crossing test's operations in the header's order (un-fused: -ffp-contract=off)
GS_API int gs_mask_polygon(const float *xy, size_t npoints, int fb_width, int fb_height, uint8_t *mask_out, size_t stride)
{
    if (!mask_out || (!xy && npoints) || fb_width <= 0 || fb_height <= 0 || (stride && stride < (size_t)fb_width)) return GS_E_BADARG;
    const size_t st = stride ? stride : (size_t)fb_width;
    for (int y = 0; y < fb_height; y++) memset(mask_out + (size_t)y * st, 0, (size_t)fb_width);
    if (npoints < 3) return GS_OK;
    for (int y = 0; y < fb_height; y++) {
        const double py = (double)y + 0.5;
        uint8_t *row = mask_out + (size_t)y * st;
        for (size_t k = 0; k < npoints; k++) {
            const size_t k1 = k + 1 < npoints ? k + 1 : 0;
            const double xa = (double)xy[2 * k], ya = (double)xy[2 * k + 1], xb = (double)xy[2 * k1], yb = (double)xy[2 * k1 + 1];
            if ((ya <= py) == (yb <= py)) continue;               // the edge does not cross this row of centres
            const double xc = xa + (py - ya) * (xb - xa) / (yb - ya);
            for (int x = 0; x < fb_width; x++) if ((double)x + 0.5 < xc) row[x] ^= 1u;
        }
    }
    return GS_OK;
}

GS_API int gs_export_row(const float cs[4], const uint32_t cc[4], void *row32, float wide[7])
{
    if (!cs || !cc || !row32) return GS_E_BADARG;
    uint32_t w[8];
    gsm::export_row(cs, cc, w, wide);
    memcpy(row32, w, 32);
    return GS_OK;
}

// the colour adjustment by the kernels' own functions (gs_adjust.h)
GS_API int gs_adjust_word(uint32_t rgba, const gs_colour_adjust *adjust, uint32_t *out)
{
    gsm::AdjustParams p;
    if (!adjust || !out || !gsm::adjust_widen(adjust->m, adjust->offset, adjust->alpha_scale, adjust->alpha_offset, p)) return GS_E_BADARG;
    *out = gsm::adjust_word(rgba, p);
    return GS_OK;
}

GS_API int gs_adjust_sh_row(const float *sh_row, int degree, const gs_colour_adjust *adjust, float *out_row)
{
    gsm::AdjustParams p;
    if (!sh_row || !out_row || !adjust || degree < 0 || degree > GS_SH_MAX_DEGREE) return GS_E_BADARG;
    if (!gsm::adjust_widen(adjust->m, adjust->offset, adjust->alpha_scale, adjust->alpha_offset, p)) return GS_E_BADARG;
    const int K = gsm::sh_coefs(degree);
    for (int k = 0; k < K; k++) {                                // (the three old values are read before the three new ones are written: out_row may be sh_row)
        const float in[3] = { sh_row[k], sh_row[K + k], sh_row[2 * K + k] };
        float o[3];
        gsm::adjust_sh_coef(in, k, p, o);
        out_row[k] = o[0]; out_row[K + k] = o[1]; out_row[2 * K + k] = o[2];
    }
    return GS_OK;
}

// the similarity of gs_transform by the kernels' own functions (gs_transform.h)
GS_API int gs_transform_record(const float cs[4], const uint32_t cc[4], const float sort_row[4], const gs_similarity *t,
                               float cs_out[4], uint32_t cc_out[4], float sort_row_out[4], float *bound_out)
{
    gsm::TransformParams p;
    if (!cs || !cc || !sort_row || !t || !cs_out || !cc_out || !sort_row_out) return GS_E_BADARG;
    if (!gsm::transform_widen(t->rotation, t->scale, t->translation, p)) return GS_E_BADARG;
    float bound;
    gsm::transform_record(cs, cc, sort_row, p, cs_out, cc_out, sort_row_out, bound);
    if (bound_out) *bound_out = bound;
    return GS_OK;
}

GS_API int gs_transform_records(const float *cs, const uint32_t *cc, const float *sort_rows, size_t n, const gs_similarity *t,
                                float *cs_out, uint32_t *cc_out, float *sort_rows_out, float *bounds_out)
{
    gsm::TransformParams p;
    if (!t || !gsm::transform_widen(t->rotation, t->scale, t->translation, p)) return GS_E_BADARG;
    if (n && (!cs || !cc || !sort_rows || !cs_out || !cc_out || !sort_rows_out)) return GS_E_BADARG;
    for (size_t i = 0; i < n; i++) {
        float bound;
        gsm::transform_record(cs + 4 * i, cc + 4 * i, sort_rows + 4 * i, p, cs_out + 4 * i, cc_out + 4 * i, sort_rows_out + 4 * i, bound);
        if (bounds_out) bounds_out[i] = bound;
    }
    return GS_OK;
}

GS_API int gs_transform_sh_row(const float *sh_row, int degree, const gs_similarity *t, float *out_row)
{
    gsm::TransformParams p;
    if (!sh_row || !out_row || !t || degree < 0 || degree > GS_SH_MAX_DEGREE) return GS_E_BADARG;
    if (!gsm::transform_widen(t->rotation, t->scale, t->translation, p)) return GS_E_BADARG;
    gsm::ShRotation rot;
    gsm::sh_rotation(p, rot);
    const int K = gsm::sh_coefs(degree);
    if (p.rot_identity) {                                        // scale and translation leave SH alone (gs_transform launches no SH kernel then)
        memmove(out_row, sh_row, 3 * (size_t)K * sizeof(float));
        return GS_OK;
    }
    for (int c = 0; c < 3; c++) {                                // (a channel's inputs are read before its outputs are written: out_row may be sh_row)
        const float *in = sh_row + c * K;
        float *out = out_row + c * K;
        if (degree == 0) out[0] = in[0];
        else if (degree == 1) gsm::transform_sh_channel<1>(in, rot, out);
        else if (degree == 2) gsm::transform_sh_channel<2>(in, rot, out);
        else gsm::transform_sh_channel<3>(in, rot, out);
    }
    return GS_OK;
}

GS_API int gs_sh_rotation(const gs_similarity *t, double out[83])
{
    gsm::TransformParams p;
    if (!t || !out || !gsm::transform_widen(t->rotation, t->scale, t->translation, p)) return GS_E_BADARG;
    gsm::ShRotation rot;
    gsm::sh_rotation(p, rot);
    memcpy(out, rot.d, sizeof rot.d);
    return GS_OK;
}

GS_API int gs_similarity_about(const float pivot[3], const float rotation[4], float scale, gs_similarity *out)
{
    gsm::TransformParams p;
    const float zero[3] = { 0.0f, 0.0f, 0.0f };
    if (!pivot || !rotation || !out || !gsm::transform_widen(rotation, scale, zero, p)) return GS_E_BADARG;
    float tr[3];
    for (int i = 0; i < 3; i++) {
        if (!gsm::transform_f32_finite(pivot[i])) return GS_E_BADARG;
        tr[i] = (float)((double)pivot[i] - p.s * ((p.R[3 * i] * (double)pivot[0] + p.R[3 * i + 1] * (double)pivot[1]) + p.R[3 * i + 2] * (double)pivot[2]));
    }
    for (int i = 0; i < 4; i++) out->rotation[i] = rotation[i];
    out->scale = scale;
    for (int i = 0; i < 3; i++) out->translation[i] = tr[i];
    return GS_OK;
}

// The INRIA header for n vertices whose rows carry K coefficients per channel; the text only
static std::string ply_header(size_t n, int K)
{
    std::string h = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(n) + "\n";
    for (const char *p : { "x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2" }) h += std::string("property float ") + p + "\n";
    for (int k = 0; k < 3 * (K - 1); k++) h += "property float f_rest_" + std::to_string(k) + "\n";
    for (const char *p : { "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3" }) h += std::string("property float ") + p + "\n";
    return h + "end_header\n";
}

static int splat_to_ply(const void *rows, const float *wide, const float *sh, size_t sh_rows, int degree, size_t nrows, void *out_bytes, size_t *out_nbytes)
{
    if (!out_nbytes || degree < 0 || degree > GS_SH_MAX_DEGREE) return GS_E_BADARG;
    if (sh_rows > nrows || (sh_rows && !sh)) return GS_E_BADARG;
    const int K = gsm::sh_coefs(degree);
    const size_t floats = 17 + 3 * (size_t)(K - 1);
    const std::string head = ply_header(nrows, K);
    *out_nbytes = head.size() + nrows * floats * sizeof(float);
    if (!out_bytes) return GS_OK;
    if (nrows && !rows) return GS_E_BADARG;
    uint8_t *out = (uint8_t *)out_bytes;
    memcpy(out, head.data(), head.size());
    out += head.size();
    const double SH_C0 = 0.28209479177387814;
    std::vector<float> f(floats);
    for (size_t i = 0; i < nrows; i++) {
        const uint8_t *r = (const uint8_t *)rows + 32 * i;
        float pos_scale[6];
        memcpy(pos_scale, r, 24);
        size_t at = 0;
        f[at++] = pos_scale[0]; f[at++] = pos_scale[1]; f[at++] = pos_scale[2];
        f[at++] = 0.0f; f[at++] = 0.0f; f[at++] = 0.0f;                              // normals: unused by every loader of the format
        const float *row_sh = i < sh_rows ? sh + i * 3 * (size_t)K : nullptr;
        for (int c = 0; c < 3; c++) f[at++] = row_sh ? row_sh[c * K] : (float)(((double)r[24 + c] / 255.0 - 0.5) / SH_C0);
        for (int c = 0; c < 3; c++) for (int k = 1; k < K; k++) f[at++] = row_sh ? row_sh[c * K + k] : 0.0f;   // channel-major, as gs_ply_sh reads it
        // the logit of alpha / 255, alpha kept inside [0.25, 254.75]: 0 and 255 come back as 0 and 255 through clamped_u8(sigmoid * 255)
        double a = (double)r[27];
        a = a < 0.25 ? 0.25 : a > 254.75 ? 254.75 : a;
        f[at++] = (float)log(a / (255.0 - a));
        for (int k = 0; k < 3; k++) f[at++] = (float)log((double)pos_scale[3 + k]);
        for (int k = 0; k < 4; k++) f[at++] = wide ? wide[7 * i + 3 + k] : (float)(((double)r[28 + k] - 128.0) / 128.0);
        memcpy(out + i * floats * sizeof(float), f.data(), floats * sizeof(float));
    }
    return GS_OK;
}

GS_API int gs_splat_to_ply(const void *rows, const float *wide, const float *sh, size_t sh_rows, int degree, size_t nrows, void *out_bytes, size_t *out_nbytes)
{
    try { return splat_to_ply(rows, wide, sh, sh_rows, degree, nrows, out_bytes, out_nbytes); }
    catch (...) { return GS_E_OOM; }
}

GS_API int gs_camera_in_object(const float model_view[16], double out[3])
{
    if (!model_view || !out) return GS_E_BADARG;
    return gsm::camera_in_object(model_view, out) ? GS_OK : GS_E_BADARG;
}

}  // extern "C"

// ---------------------------------------------------------------- compressed .ply

namespace {

const char *const kChunkProps[18] = { "min_x", "min_y", "min_z", "max_x", "max_y", "max_z",
                                      "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x", "max_scale_y", "max_scale_z",
                                      "min_r", "min_g", "min_b", "max_r", "max_g", "max_b" };
const char *const kVertexProps[4] = { "packed_position", "packed_rotation", "packed_scale", "packed_color" };

// "element <name> <count>" with a plain decimal count
bool element_line(const std::string &line, const char *name, size_t *count)
{
    const std::string head = std::string("element ") + name + " ";
    if (line.compare(0, head.size(), head) != 0 || line.size() == head.size() || line.size() > head.size() + 18) return false;
    size_t v = 0;
    for (size_t j = head.size(); j < line.size(); j++) {
        if (line[j] < '0' || line[j] > '9') return false;
        v = v * 10 + (size_t)(line[j] - '0');
    }
    *count = v;
    return true;
}

int cply_plan(const void *bytes, size_t nbytes, gsm::CplyInfo *info, char *err, size_t errlen)
{
    memset(info, 0, sizeof *info);
    if (!bytes) return fail(err, errlen, GS_E_BADARG, "compressed .ply: bytes is NULL");
    const size_t hl = std::min<size_t>(nbytes, 65536);
    const std::string head((const char *)bytes, hl);
    // the end of the header: the first line that is exactly "end_header"
    size_t end = std::string::npos;
    if (head.compare(0, 11, "end_header\n") == 0) end = 0;
    else { const size_t at = head.find("\nend_header\n"); if (at != std::string::npos) end = at + 1; }
    if (end == std::string::npos) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: no end_header line");
    std::vector<std::string> lines;
    for (size_t ls = 0; ls < end;) {
        const size_t le = head.find('\n', ls);
        const std::string line = head.substr(ls, le - ls);
        if (!(line.compare(0, 8, "comment ") == 0 || line == "comment")) lines.push_back(line);
        ls = le + 1;
    }
    size_t at = 0;
    auto next = [&]() -> const std::string & { static const std::string none; return at < lines.size() ? lines[at++] : none; };
    if (next() != "ply") return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: the file does not begin with \"ply\"");
    if (next() != "format binary_little_endian 1.0") return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: format is not binary_little_endian 1.0");
    size_t C = 0, N = 0, NS = 0;
    if (!element_line(next(), "chunk", &C)) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: \"element chunk\" expected first (not a compressed file)");
    int cf = 0;
    while (cf < 18 && at < lines.size() && lines[at] == std::string("property float ") + kChunkProps[cf]) { cf++; at++; }
    if (cf != 12 && cf != 18) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: element chunk: property float %s expected", kChunkProps[cf < 18 ? cf : 17]);
    if (!element_line(next(), "vertex", &N)) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: \"element vertex\" expected after the 12 or 18 chunk properties");
    for (int k = 0; k < 4; k++)
        if (next() != std::string("property uint ") + kVertexProps[k]) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: element vertex: property uint %s expected", kVertexProps[k]);
    int per = 0;
    if (at < lines.size()) {
        if (!element_line(next(), "sh", &NS)) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: \"element sh\" or end_header expected after the vertex properties");
        while (at < lines.size()) {
            if (lines[at] != "property uchar f_rest_" + std::to_string(per)) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: element sh: property uchar f_rest_<k> in ascending k expected, found \"%s\"", lines[at].c_str());
            per++; at++;
        }
        if (per != 9 && per != 24 && per != 45) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: element sh: 9, 24 or 45 f_rest_* properties expected");
        if (NS != N) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: element sh and element vertex differ in count");
        per /= 3;
    }
    if (N > 0x7FFFFFF0ull) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: more than 2^31 splats");
    if (C != (N + GS_CPLY_CHUNK - 1) / GS_CPLY_CHUNK) return fail(err, errlen, GS_E_PLY_HEADER, "compressed .ply: element chunk count is not ceil(vertices / 256)");
    info->n = N; info->chunks = C; info->chunk_floats = cf; info->per = per;
    info->degree = per == 3 ? 1 : per == 8 ? 2 : per == 15 ? 3 : 0;
    info->data_start = end + 11;
    const size_t body = C * (size_t)cf * 4 + N * 16 + N * 3 * (size_t)per;
    if (body > nbytes - info->data_start) return fail(err, errlen, GS_E_PLY_DATA, "compressed .ply: the body is shorter than the header promises");
    return GS_OK;
}

// where the three arrays of the body begin
struct Body { const uint8_t *chunks, *verts, *sh; };
Body body_of(const void *bytes, const gsm::CplyInfo &I)
{
    Body b;
    b.chunks = (const uint8_t *)bytes + I.data_start;
    b.verts = b.chunks + I.chunks * (size_t)I.chunk_floats * 4;
    b.sh = b.verts + I.n * 16;
    return b;
}

int cply_to_splat(const void *bytes, size_t nbytes, void *out_rows, float *out_wide, size_t *out_nrows, char *err, size_t errlen)
{
    if (!bytes || !out_nrows) return fail(err, errlen, GS_E_BADARG, "gs_cply_to_splat: NULL argument");
    *out_nrows = 0;
    gsm::CplyInfo I;
    const int rc = cply_plan(bytes, nbytes, &I, err, errlen);
    if (rc != GS_OK) return rc;
    *out_nrows = I.n;
    if (!out_rows) return GS_OK;
    const Body B = body_of(bytes, I);
    for (size_t i = 0; i < I.n; i++) {
        float chunk[18]; uint32_t packed[4], row[8];
        memcpy(chunk, B.chunks + (i >> 8) * (size_t)I.chunk_floats * 4, (size_t)I.chunk_floats * 4);
        memcpy(packed, B.verts + i * 16, 16);
        gsm::cply_decode(chunk, I.chunk_floats, packed, row, out_wide ? out_wide + 7 * i : nullptr, nullptr);
        memcpy((uint8_t *)out_rows + 32 * i, row, 32);
    }
    return GS_OK;
}

int cply_sh(const void *bytes, size_t nbytes, int degree, float *out_sh, size_t *out_nrows, int *out_degree, char *err, size_t errlen)
{
    if (!bytes || !out_nrows || !out_degree) return fail(err, errlen, GS_E_BADARG, "gs_cply_sh_host: NULL argument");
    if (degree < 0 || degree > GS_SH_MAX_DEGREE) return fail(err, errlen, GS_E_BADARG, "gs_cply_sh_host: degree must be 0..3");
    *out_nrows = 0; *out_degree = -1;
    gsm::CplyInfo I;
    const int rc = cply_plan(bytes, nbytes, &I, err, errlen);
    if (rc != GS_OK) return rc;
    const int D = degree < I.degree ? degree : I.degree, K = gsm::sh_coefs(D);
    *out_degree = D; *out_nrows = I.n;
    if (!out_sh) return GS_OK;
    const Body B = body_of(bytes, I);
    for (size_t i = 0; i < I.n; i++) {
        float chunk[18]; uint32_t packed[4], row[8]; double colour[3];
        memcpy(chunk, B.chunks + (i >> 8) * (size_t)I.chunk_floats * 4, (size_t)I.chunk_floats * 4);
        memcpy(packed, B.verts + i * 16, 16);
        gsm::cply_decode(chunk, I.chunk_floats, packed, row, nullptr, colour);
        float *o = out_sh + i * 3 * (size_t)K;
        const uint8_t *s = B.sh + i * 3 * (size_t)I.per;
        for (int c = 0; c < 3; c++) {
            o[c * K] = gsm::cply_sh_dc(colour[c]);
            for (int k = 1; k < K; k++) o[c * K + k] = gsm::cply_sh_rest(s[c * I.per + (k - 1)]);
        }
    }
    return GS_OK;
}

std::string cply_header(size_t n, int per)
{
    std::string h = "ply\nformat binary_little_endian 1.0\nelement chunk " + std::to_string((n + GS_CPLY_CHUNK - 1) / GS_CPLY_CHUNK) + "\n";
    for (const char *p : kChunkProps) h += std::string("property float ") + p + "\n";
    h += "element vertex " + std::to_string(n) + "\n";
    for (const char *p : kVertexProps) h += std::string("property uint ") + p + "\n";
    if (per) {
        h += "element sh " + std::to_string(n) + "\n";
        for (int k = 0; k < 3 * per; k++) h += "property uchar f_rest_" + std::to_string(k) + "\n";
    }
    return h + "end_header\n";
}

int splat_to_cply(const void *rows, const float *wide, const float *sh, size_t sh_rows, int degree, size_t nrows, uint32_t flags, uint32_t *out_index,
                  void *out_bytes, size_t *out_nbytes)
{
    if (!out_nbytes || degree < 0 || degree > GS_SH_MAX_DEGREE || (flags & ~GS_CPLY_MORTON)) return GS_E_BADARG;
    if (sh_rows > nrows || (sh_rows && !sh) || nrows > 0x7FFFFFF0ull) return GS_E_BADARG;
    const int K = gsm::sh_coefs(degree), per = K - 1;
    const std::string head = cply_header(nrows, per);
    const size_t C = (nrows + GS_CPLY_CHUNK - 1) / GS_CPLY_CHUNK;
    *out_nbytes = head.size() + C * 72 + nrows * 16 + nrows * 3 * (size_t)per;
    if (!out_bytes) return GS_OK;
    if (nrows && !rows) return GS_E_BADARG;
    uint8_t *out = (uint8_t *)out_bytes;
    memcpy(out, head.data(), head.size());
    uint8_t *o_chunks = out + head.size(), *o_verts = o_chunks + C * 72, *o_sh = o_verts + nrows * 16;
    // the nine values of every row
    std::vector<float> val(nrows * 9 + 1);
    for (size_t i = 0; i < nrows; i++) {
        uint32_t row[8];
        memcpy(row, (const uint8_t *)rows + 32 * i, 32);
        gsm::cply_values(row, wide ? wide + 7 * i : nullptr, i < sh_rows ? sh + i * 3 * (size_t)K : nullptr, K, &val[9 * i]);
    }
    std::vector<uint32_t> order(nrows);
    for (size_t i = 0; i < nrows; i++) order[i] = (uint32_t)i;
    if (flags & GS_CPLY_MORTON) {
        uint32_t kmin[3] = { GS_CPLY_KEY_MIN_ID, GS_CPLY_KEY_MIN_ID, GS_CPLY_KEY_MIN_ID }, kmax[3] = { GS_CPLY_KEY_MAX_ID, GS_CPLY_KEY_MAX_ID, GS_CPLY_KEY_MAX_ID };
        for (size_t i = 0; i < nrows; i++)
            for (int a = 0; a < 3; a++) {
                const float v = val[9 * i + a];
                if (!gsm::cply_finite(v)) continue;
                const uint32_t k = gsm::cply_key(v);
                kmin[a] = std::min(kmin[a], k); kmax[a] = std::max(kmax[a], k);
            }
        float box[6];
        for (int a = 0; a < 3; a++) gsm::cply_bounds_of(kmin[a], kmax[a], box[a], box[3 + a]);
        std::vector<uint32_t> code(nrows);
        for (size_t i = 0; i < nrows; i++) code[i] = gsm::cply_morton(&val[9 * i], box);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return code[a] < code[b]; });
    }
    for (size_t ch = 0; ch < C; ch++) {
        const size_t j0 = ch * GS_CPLY_CHUNK, j1 = std::min(nrows, j0 + GS_CPLY_CHUNK);
        uint32_t kmin[9], kmax[9];
        for (int q = 0; q < 9; q++) { kmin[q] = GS_CPLY_KEY_MIN_ID; kmax[q] = GS_CPLY_KEY_MAX_ID; }
        for (size_t j = j0; j < j1; j++)
            for (int q = 0; q < 9; q++) {
                const float v = val[9 * (size_t)order[j] + q];
                if (!gsm::cply_finite(v)) continue;
                const uint32_t k = gsm::cply_key(v);
                kmin[q] = std::min(kmin[q], k); kmax[q] = std::max(kmax[q], k);
            }
        // the record's layout: min xyz, max xyz | min scale, max scale | min rgb, max rgb
        float bounds[18];
        for (int g = 0; g < 3; g++)
            for (int a = 0; a < 3; a++) gsm::cply_bounds_of(kmin[3 * g + a], kmax[3 * g + a], bounds[6 * g + a], bounds[6 * g + 3 + a]);
        memcpy(o_chunks + ch * 72, bounds, 72);
        for (size_t j = j0; j < j1; j++) {
            const size_t i = order[j];
            uint32_t row[8], w[4];
            memcpy(row, (const uint8_t *)rows + 32 * i, 32);
            gsm::cply_encode(&val[9 * i], bounds, row, wide ? wide + 7 * i : nullptr, w);
            memcpy(o_verts + 16 * j, w, 16);
            for (int c = 0; c < 3; c++)
                for (int k = 1; k < K; k++) o_sh[j * 3 * (size_t)per + c * per + (k - 1)] = i < sh_rows ? gsm::cply_sh_byte(sh[(i * 3 + c) * K + k]) : (uint8_t)128;
            if (out_index) out_index[j] = (uint32_t)i;
        }
    }
    return GS_OK;
}

}  // namespace

// shared with gs_cply.hip; no C++ exception crosses it
extern "C" int gs_cply_plan(const void *bytes, size_t nbytes, gsm::CplyInfo *info, char *err, size_t errlen)
{
    try { return cply_plan(bytes, nbytes, info, err, errlen); }
    catch (...) { return fail(err, errlen, GS_E_OOM, "out of host memory while reading the compressed .ply header"); }
}

// the header text of a file of n splats with `degree` bands (out == NULL: its length alone)
extern "C" int gs_cply_write_header(size_t n, int degree, void *out, size_t *len)
{
    try {
        const std::string h = cply_header(n, gsm::sh_coefs(degree) - 1);
        *len = h.size();
        if (out) memcpy(out, h.data(), h.size());
        return GS_OK;
    } catch (...) { return GS_E_OOM; }
}

extern "C" {

GS_API int gs_cply_info(const void *bytes, size_t nbytes, size_t *out_nsplats, size_t *out_nchunks, int *out_sh_degree, int *out_chunk_floats, char *err, size_t errlen)
{
    gsm::CplyInfo I;
    const int rc = gs_cply_plan(bytes, nbytes, &I, err, errlen);
    if (rc != GS_OK && rc != GS_E_PLY_DATA) return rc;           // (a short body: the header's figures are still reported)
    if (out_nsplats) *out_nsplats = I.n;
    if (out_nchunks) *out_nchunks = I.chunks;
    if (out_sh_degree) *out_sh_degree = I.degree;
    if (out_chunk_floats) *out_chunk_floats = I.chunk_floats;
    return rc;
}

GS_API int gs_cply_to_splat(const void *bytes, size_t nbytes, void *out_rows, float *out_wide, size_t *out_nrows, char *err, size_t errlen)
{
    try { return cply_to_splat(bytes, nbytes, out_rows, out_wide, out_nrows, err, errlen); }
    catch (...) { return fail(err, errlen, GS_E_OOM, "out of host memory while decoding the compressed .ply"); }
}

GS_API int gs_cply_sh_host(const void *bytes, size_t nbytes, int degree, float *out_sh, size_t *out_nrows, int *out_degree, char *err, size_t errlen)
{
    try { return cply_sh(bytes, nbytes, degree, out_sh, out_nrows, out_degree, err, errlen); }
    catch (...) { return fail(err, errlen, GS_E_OOM, "out of host memory while reading the compressed .ply coefficients"); }
}

GS_API int gs_splat_to_cply(const void *rows, const float *wide, const float *sh, size_t sh_rows, int degree, size_t nrows, uint32_t flags, uint32_t *out_index,
                            void *out_bytes, size_t *out_nbytes)
{
    try { return splat_to_cply(rows, wide, sh, sh_rows, degree, nrows, flags, out_index, out_bytes, out_nbytes); }
    catch (...) { return GS_E_OOM; }
}

GS_API int gs_log_fixed(double x, double *out)
{
    if (!out) return GS_E_BADARG;
    *out = gsm::log_fixed(x);
    return GS_OK;
}

}  // extern "C"

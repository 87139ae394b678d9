// gs_export_stage.h -- what gs_export.hip stages in device memory for a writer that encodes on the device (gs_cply.hip): the splats
// that pass a state filter in stable order, by the export scheme's own kernels (count, offsets, scatter, gsm::export_row).
#pragma once
#include "gs_internal.h"

struct GsExportStage {
    uint4 *rows = nullptr;                                         // total x 2: the 32-byte rows
    float *wide = nullptr;                                         // total x 7
    uint32_t *index = nullptr;                                     // total: the resident index of row k
    uint4 *sh = nullptr;                                           // sh_total padded store rows of sh_row_q 16-byte words (the first sh_total rows' own)
    size_t total = 0, sh_total = 0;
    uint32_t sh_row_q = 0;
    int sh_deg = 0;                                                // the store's degree (0: no row staged)
};
// On ctx->prop_stream (created here if need be), idle again on return.  with_rows = false: the counts alone.
int gs_export_stage(gs_ctx *ctx, const char *name, uint8_t mask, uint8_t value, bool with_rows, GsExportStage *out);
void gs_export_stage_free(GsExportStage *s);

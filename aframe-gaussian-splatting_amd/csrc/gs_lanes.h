// gs_lanes.h -- private to the host controller: what crosses between gs_lanes.hip (lanes, their scratch and enqueue threads),
// gs_frame.hip (sort / render / sync entry points, frame log, share collection), gs_edit.hip (editing entry points) and gs_api.hip
// (the rest of the C ABI).  Nothing a frame calls per launch sits behind a call that was inlined while these were one file: what
// was inlined then is `static inline` here.
#pragma once
#include <functional>
#include <new>
#include <vector>
#include "gs_internal.h"

#define CHECK_CTX(ctx) do { if (!(ctx)) return GS_E_BADARG; } while (0)
#define FAIL(code, ...) do { snprintf(GS_ERRBUF(ctx), GS_ERRLEN, __VA_ARGS__); return (code); } while (0)
#define TRY(x) do { int _rc = (x); if (_rc != GS_OK) return _rc; } while (0)

template <typename T> static int dev_alloc(gs_ctx *ctx, T **p, size_t count)
{
    *p = nullptr;
    if (!count) count = 1;
    hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? GS_E_OOM : GS_E_HIP;
    }
    return GS_OK;
}
template <typename T> static void dev_free(T *&p) { if (p) { (void)hipFree(p); p = nullptr; } }

// ---- transparent re-rendering (GS_OPT_AUTO_RETRY).  An asynchronous frame can come back incomplete: it skipped its second
// binning round and a tile had not saturated, or it outgrew the pair buffers.  The lane's control block says so at gs_sync() --
// per lane, not per frame -- so every lane keeps a log of what it was asked since the last gs_sync(): the sort's arguments and
// the renders that followed (uniforms, output pointers).  gs_sync() then draws the logged frames of a flagged lane (and of the
// lane / twin that shares its stream) again, synchronously, both rounds, into the same buffers.  Written and read on the caller's
// thread only.  Not decided here: gathered frames (the other ranks have to take part), frames sharing an output buffer with
// another logged frame (drawing the older one again would overwrite the newer), data or scene changed meanwhile.
// (gs_frame.hip keeps the log; gs_lanes.hip frees it and reads it in drain_all)
struct GsFrameRec {
    float view[4], cutout[16]; bool has_cutout, has_strip; GsSortStrip strip;
    int nrender; bool undecidable;
    struct { GsFrameUniforms u; void *dev; uint8_t *host; size_t stride; } r[2];
};
struct GsFrameLog { std::vector<GsFrameRec> recs; bool open = false; };

// what a lane's enqueue thread is handed (gs_lanes.hip: lane_push)
enum { GS_CMD_SORT, GS_CMD_RENDER /* asynchronous */, GS_CMD_CALL /* gs_comm.hip: the frame's gather */ };
struct GsLaneCmd {
    gs_ctx *target;                                            // the lane (or twin) the command is for
    int type;                                                  // GS_CMD_*
    float view[4], cutout[16]; bool has_cutout;
    bool has_strip; GsSortStrip strip; uint32_t near_req;      // (sort: how much of the order the frame is expected to need; 0 = all)
    GsFrameUniforms u; void *device_rgba; uint8_t *host_rgba; size_t stride;
    std::function<int(gs_ctx *)> call;
};

// (in a namespace of their own: short names that no static link or addon build can collide with)
namespace gs_ctl {
// ---- gs_lanes.hip
int lane_drain(gs_ctx *L, bool flush = false);
int lane_push(gs_ctx *L, GsLaneCmd c);
int drain_all(gs_ctx *ctx);
int lane_read_control(gs_ctx *L, bool wait);
int get_lane(gs_ctx *ctx, int i, gs_ctx **out);
int prepare_lanes(gs_ctx *ctx);
void refresh_lanes(gs_ctx *ctx);
hipError_t init_frame_resources(gs_ctx *c, gs_ctx *primary = nullptr);
void free_frame_resources(gs_ctx *c);
int ensure_capacity(gs_ctx *ctx, size_t want);
int edit_ensure_alloc(gs_ctx *ctx);
int set_profile(gs_ctx *ctx, bool on, bool blend_only, uint32_t every = 1);
int prof_drain(gs_ctx *ctx);
int prof_advance(gs_ctx *ctx);
// ---- gs_frame.hip
int render_async_on_lane(gs_ctx *ctx, const GsFrameUniforms &u, void *device_rgba, uint8_t *host_rgba, size_t stride);
int ensure_frame_buffers(gs_ctx *ctx, const GsFrameUniforms &u, bool need_fb);
int ensure_full_sort(gs_ctx *L);
int collect_near_sort(gs_ctx *lane, const GsControl *c, uint32_t *spec_failed);
void reseed_lanes(gs_ctx *ctx /* owner */);
void reset_cloud_measurements(gs_ctx *ctx /* owner */);
}  // namespace gs_ctl
using namespace gs_ctl;

// do asynchronous frames move on to another lane / twin?  (more than one lane, or one lane whose frames pair with its twin's)
static inline bool gs_rotates(const gs_ctx *ctx) { return ctx->pipe_depth > 1 || (ctx->frame_batch == 2 && ctx->enqueue_threads); }

// the lane a NEW frame goes to: the next one if the current frame was handed off asynchronously
static inline int next_frame_lane(const gs_ctx *ctx, int *rot = nullptr, bool solo = false)
{
    if (!(ctx->cur_async && !ctx->user_stream && gs_rotates(ctx))) { if (rot) *rot = ctx->rot; return ctx->cur; }
    if (ctx->frame_batch == 2 && ctx->enqueue_threads && solo) {
        // a frame of two views (XR eyes on one GPU): primary lanes only -- the twin's scratch is the second view's
        const int lane = (ctx->cur % GS_MAX_PRIMARY + 1) % ctx->pipe_depth;
        if (rot) *rot = 2 * lane;
        return lane;
    }
    if (ctx->frame_batch == 2 && ctx->enqueue_threads) {
        // lane 0, its twin, lane 1, its twin, ...: the two frames of a pair sit behind each other in one enqueue thread's queue
        const int r = (ctx->rot + 1) % (2 * ctx->pipe_depth);
        if (rot) *rot = r;
        return r / 2 + (r % 2) * GS_MAX_PRIMARY;
    }
    if (rot) *rot = 0;
    return ctx->cur >= GS_MAX_PRIMARY ? 0 : (ctx->cur + 1) % ctx->pipe_depth;
}

// lane `lane` (at `rot` of the rotation) holds the current frame, and nothing of it has been handed off yet
static inline void set_current_lane(gs_ctx *ctx, int lane, int rot) { ctx->cur = lane; ctx->rot = rot; ctx->cur_async = false; }

static inline int lane_rc(gs_ctx *ctx, gs_ctx *L, int rc)
{
    if (rc != GS_OK && L != ctx) memcpy(ctx->err, L->err, sizeof ctx->err);
    return rc;
}

// does a sort asked for the nearest `near_req` positions (0: the whole order) give frame `u` all it reads?
static inline bool sort_covers(uint32_t near_req, const GsFrameUniforms &u)
{
    return near_req == 0 || (u.near_count != 0xFFFFFFFFu && u.skip_round1 && u.near_count <= near_req);
}

// gs_frame.hip -- a frame from its sort to its collection: the sort, render, surface, pick and sync entry points of the C ABI
// (include/gs_splat.h), the frame log behind transparent re-rendering, what a collected frame tells the share policy
// (gs_share.h) and the near-only sorts, and the entry points that couple frames to other streams.
#include <stdlib.h>
#include <chrono>
#include <set>
#include "gs_lanes.h"
#include "gs_sh.h"

#define GS_LOG_MAX 4096

static GsFrameRec *log_open_rec(gs_ctx *L) { return (L->log && L->log->open && !L->log->recs.empty()) ? &L->log->recs.back() : nullptr; }
static void log_sort(gs_ctx *L, const float view[4], const float *cutout16, const GsSortStrip *strip)
{
    if (!gs_root(L)->auto_retry) return;
    if (!L->log) { L->log = new (std::nothrow) GsFrameLog(); if (!L->log) return; }
    GsFrameLog *g = L->log;
    if (g->open && !g->recs.empty() && g->recs.back().nrender == 0) g->recs.pop_back();   // a sort nothing was drawn from
    if (g->recs.size() >= GS_LOG_MAX) { g->recs.back().undecidable = true; g->open = true; return; }   // (a caller that never syncs)
    GsFrameRec r;
    memcpy(r.view, view, sizeof r.view);
    r.has_cutout = cutout16 != nullptr;
    if (cutout16) memcpy(r.cutout, cutout16, sizeof r.cutout);
    r.has_strip = strip != nullptr;
    if (strip) r.strip = *strip;
    r.nrender = 0; r.undecidable = false;
    try { g->recs.push_back(r); g->open = true; } catch (...) { g->open = false; }
}
static void log_render(gs_ctx *L, const GsFrameUniforms &u, void *dev, uint8_t *host, size_t stride)
{
    GsFrameRec *r = log_open_rec(L);
    if (!r) return;
    if (r->nrender >= 2) { r->undecidable = true; return; }
    r->r[r->nrender].u = u; r->r[r->nrender].dev = dev; r->r[r->nrender].host = host; r->r[r->nrender].stride = stride;
    r->nrender++;
}
static void log_undecidable(gs_ctx *L) { GsFrameRec *r = log_open_rec(L); if (r) r->undecidable = true; }
// after gs_sync: only the open frame stays (renders may still follow its sort), with nothing drawn
static void log_reset(gs_ctx *L)
{
    if (!L->log) return;
    GsFrameLog *g = L->log;
    if (g->open && !g->recs.empty()) { GsFrameRec last = g->recs.back(); last.nrender = 0; last.undecidable = false; g->recs.clear(); g->recs.push_back(last); }
    else g->recs.clear();
}

// the speculative stash of near-only sorts failed: at once out of use for a while if the view does not suit it (kind 2), at the second
// miss within a few collections if the threshold bin keeps outrunning the hint -- one miss is a camera jump, two in a row are a view
// whose threshold is not smooth (the 20 M cloud seen from outside: the bin moves by up to three from one 3-degree pose to the next), and
// every miss costs the redraw of the lanes' logged frames.  (A collected sort that took the path pays one unit of the 24 back.)
static void gs_spec_back_off(gs_ctx *ctx /* owner */, bool unsuited)
{
    ctx->near_spec_miss_credit += 24u;
    if (!unsuited && ctx->near_spec_miss_credit <= 32u) return;
    ctx->near_spec_miss_credit = 0;
    ctx->near_spec_backoff = ctx->near_spec_backoff ? (ctx->near_spec_backoff >= 32768u ? 65536u : ctx->near_spec_backoff * 2u) : 512u;
    __atomic_store_n(&ctx->near_spec_hold, ctx->near_spec_backoff, __ATOMIC_RELAXED);
}

// what was measured on another cloud (gs_clear, gs_compact): the sizing hints, the share, the near-only sorts' speculation
void gs_ctl::reset_cloud_measurements(gs_ctx *ctx /* owner */)
{
    ctx->pair_hint = 0; ctx->run_hint = 0; ctx->last_pairs = 0; ctx->last_visible = 0;
    gs_share_reset_clear(ctx->share);
    ctx->near_stash_off = false; ctx->near_spec = false; ctx->near_spec_hold = 0; ctx->near_spec_backoff = 0; ctx->near_spec_miss_credit = 0;
}

// The lanes' need words are brought near what the collected frames measured (gs_share_lane_seed says which lanes and with what).
static void seed_need_words(gs_ctx *ctx /* owner */, uint32_t need, bool idle_only)
{
    if (!need) return;
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (!L || !L->ctl) continue;
        // (from a synchronous frame: a lane with queued, uncollected frames keeps its words -- the seed its next projection would store is the
        // host's ESTIMATE, and the larger maxima the frames in flight recorded would be lost before gs_sync reads them: ADVICE r5)
        if (idle_only && L->async_pending) continue;
        gs_share_lane_seed(L->share_lane, need);
    }
}

// every lane's next frame clears its need words (with the owner's gs_share_reset_kind_switch / _unpin)
void gs_ctl::reseed_lanes(gs_ctx *ctx /* owner */)
{
    for (int i = 0; i < GS_MAX_LANES; i++) if (ctx->lanes[i]) gs_share_lane_reseed(ctx->lanes[i]->share_lane);
}

// The share policy's step for a whole collection (after the lanes' collect_status): gs_share_decide once, then the seeds.
static void decide_share(gs_ctx *ctx /* owner */, float frac_used, const GsShareTally &tally, bool idle_only)
{
    const uint32_t need = gs_share_decide(ctx->share, ctx->n, frac_used, tally);
    if (need) ctx->stats.need_splats = need;
    seed_need_words(ctx, need, idle_only);
}

// What a collected sort says about the near-only forms (a collection: collect_status below, or gs_sort_inspect): a stash that overflowed,
// a threshold-bin hint that exists now, a speculative stash that failed.  spec_failed: the caller backs off once for all its lanes
// (gs_sync); null: here
int gs_ctl::collect_near_sort(gs_ctx *lane, const GsControl *c, uint32_t *spec_failed)
{
    gs_ctx *ctx = gs_root(lane);
    if (c->near_overflow) {
        // a chunk of a near-only sort had more survivors than its stash holds (the frame was flagged and is drawn again from a
        // whole sort): this context keeps to the whole-length passes from now on
        __atomic_store_n(&ctx->near_stash_off, true, __ATOMIC_RELAXED);   // (the lanes' enqueue threads read these flags while they launch sorts)
        GS_HIP(hipMemsetAsync(&lane->ctl->near_overflow, 0, sizeof(uint32_t), lane->stream));
    }
    if (c->near_sorted == 1u || c->near_sorted == 2u) {          // (3: a tail sort -- no threshold, no hint)
        __atomic_store_n(&ctx->near_spec, true, __ATOMIC_RELAXED);    // a near-only sort has run: the threshold-bin hint exists (gs_near_spec_ok)
        const uint32_t h = __atomic_load_n(&ctx->near_spec_hold, __ATOMIC_RELAXED);
        if (h) __atomic_store_n(&ctx->near_spec_hold, h - 1u, __ATOMIC_RELAXED);
    }
    if (c->near_sorted == 2u) { ctx->stats.spec_sorts++; if (ctx->near_spec_miss_credit) ctx->near_spec_miss_credit--; }
    if (c->spec_fail) {
        // a near-only sort could not vouch for the candidates its depth pass had stashed (the frame was flagged and is drawn again
        // from a whole sort).  1: the hint was behind -- it is exact now; 2: a stash overflowed / the depth range does not suit the path
        ctx->stats.spec_misses++;
        // (the frames a gs_sync collects were sorted by ONE hint: the lanes that missed it together -- a camera jump -- are one event)
        if (spec_failed) { if (c->spec_fail > *spec_failed) *spec_failed = c->spec_fail; }
        else gs_spec_back_off(ctx, c->spec_fail == 2u);
        GS_HIP(hipMemsetAsync(&lane->ctl->spec_fail, 0, sizeof(uint32_t), lane->stream));
    }
    return GS_OK;
}

// after a stream sync: publish the counters of the last completed frame, hand what they say about the share of splats binned first
// to the policy (gs_share.h) and react to pair-buffer overflow
static int collect_status(gs_ctx *lane, bool *overflowed, GsShareTally &tally, uint32_t *spec_failed)
{
    gs_ctx *ctx = gs_root(lane);                                // the adaptive share is one state for all lanes ...
    const GsControl *c = lane->ctl_host;                        // ... fed by each lane's own counters
    lane->stats.n_sorted = c->n_kept; lane->stats.n_visible = c->n_visible; lane->stats.n_pairs = c->n_pairs_frame;
    lane->stats.acc_frames = c->acc_frames; lane->stats.acc_sorted = c->acc_sorted; lane->stats.acc_visible = c->acc_visible;
    lane->stats.acc_pairs = c->acc_pairs; lane->stats.sort_records = c->n_sorted;
    lane->stats.sort_mode = c->near_sorted;
    lane->stats.n_hidden = lane->sort_hidden;
    lane->stats.n_runs = c->n_runs;
    if (c->n_pairs_frame) { ctx->last_pairs = c->n_pairs_frame; ctx->last_visible = c->n_visible; }
    if (c->n_pairs_frame) __atomic_store_n(&ctx->run_hint, c->n_runs, __ATOMIC_RELAXED);
    if (c->n_pairs_frame) {                                     // sizing hint for the next frames' pair sort (any lane's worker may read it)
        const uint64_t h = (uint64_t)c->n_pairs_frame + c->n_pairs_frame / 4 + GS_CHUNK_L;
        __atomic_store_n(&ctx->pair_hint, h > 0xFFFFFFFFull ? 0u : (uint32_t)h, __ATOMIC_RELAXED);
    }
    // The share of splats binned in round 0 (gs_share.h).  A frame whose round 0 left tiles unsaturated either had them finished by
    // round 1 -- an "event": a failure of a share that is walked (no measurement: x 0.9 per collection, x 0.98 above the floor a
    // failure leaves), nothing but a larger need where the blend measures -- or, round 1 skipped, was flagged (round1_missed) and is
    // drawn again: a failure either way.  The lane's counters go in here; the collection's caller decides once for all its lanes.
    GsShareObs obs;
    obs.need = 0;
    for (uint32_t k = 0; k < GS_NEED_WORDS; k++) if (c->need_near[k] > obs.need) obs.need = c->need_near[k];
    obs.unsat_events = c->unsat_events; obs.acc_frames = c->acc_frames; obs.round1_missed = c->round1_missed;
    obs.order_incomplete = c->order_incomplete; obs.n_kept = c->n_kept; obs.tiles = lane->stats.n_tiles != 0;
    gs_share_observe(ctx->share, lane->share_lane, obs, tally);
    TRY(collect_near_sort(lane, c, spec_failed));
    lane->stats.unsat_tiles = lane->share_lane.last_two_rounds ? c->unsat_round0 : 0;
    lane->stats.near_permille = (uint32_t)(ctx->share.near_frac * 1000.0f + 0.5f);
    *overflowed = c->overflow_sticky != 0;
    if (*overflowed) {
        const size_t need = (size_t)c->max_total + c->max_total / 4 + 1;
        GS_HIP(hipMemsetAsync(&lane->ctl->overflow_sticky, 0, 2 * sizeof(uint32_t), lane->stream));
        GS_HIP(hipStreamSynchronize(lane->stream));
        if (gs_ensure_pair_capacity(lane, need) != GS_OK) { if (lane != ctx) memcpy(ctx->err, lane->err, sizeof ctx->err); return GS_E_OOM; }
    }
    return GS_OK;
}

// Near-only sorts (GS_OPT_SORT_NEAR).  A frame whose single binning round covers the nearest near_count splats (round 1 skipped
// optimistically, gs_fill_uniforms) reads nothing else of the order, so its sort lets only the splats go on that can be among
// them (gs_sort.hip: an exact rule on the sort key; the positions it fills equal the whole order's).  The request is made when
// the sort is issued, from the state the render's uniforms will be made from; a render that turns out to need more of the
// order (another share, a counting render, round 1 after all, gs_download of the order) sorts again in full first.
static uint32_t sort_near_request(const gs_ctx *ctx /* owner */)
{
    if (!ctx->sort_near_opt || !ctx->renderable) return 0;
    // (short sorts are bound by their launches and dependent round trips, not by their records: measured again in round 5 with the
    // four-launch MSD sort -- at 1 M splats the depth histogram and the threshold search cost the depth and bucket kernels 10 us, the
    // two kernels behind them save 2 with a fifth of the records: 7 170 against 7 590 frames/s one frame at a time, the same pipelined)
    // ... so up to GS_MSD_MAX_N splats a near-only sort is a TAIL sort (gs_sort.hip): the four launches of the whole sort, of which the
    // last two leave out the segments before the one the frame's first position lies in -- nothing is added in front
    const bool tail = gs_msd_enabled() && ctx->n <= (size_t)GS_MSD_MAX_N && !ctx->wide_pairs;
    if (ctx->sort_near_opt == 1 && ctx->n < ((size_t)1 << 22) && !tail) return 0;
    if (ctx->wide_pairs || ctx->n > ((size_t)1 << 25)) return 0;
    if (!gs_share_round1_skippable(ctx->share)) return 0;                // (skippable: the share is not pinned)
    const uint32_t nc = gs_share_near_count(ctx->share, ctx->n);
    if (nc == 0xFFFFFFFFu) return 0;
    // (a cutout or a strip that keeps little more than the frame reads anyway: the histogram and the threshold would buy nothing)
    if (ctx->sort_near_opt == 1 && ctx->share.last_kept && (double)nc * 2.0 > (double)ctx->share.last_kept) return 0;
    return nc;
}
// GS_OPT_SORT_NEAR_FORCE: the request itself, behind what a near-only sort cannot do without (compact records, a renderable context)
static uint32_t sort_near_forced(const gs_ctx *ctx /* owner */)
{
    return (ctx->renderable && !ctx->wide_pairs && ctx->n <= ((size_t)1 << 25)) ? ctx->sort_near_force : 0u;
}
int gs_ctl::ensure_full_sort(gs_ctx *L)
{
    if (!L->have_sort || !L->sort_near_req) return GS_OK;
    return gs_run_sort(L, L->sv_view, L->sv_has_cutout ? L->sv_cutout : nullptr, L->sv_has_strip ? &L->sv_strip : nullptr, 0);
}
static int ensure_sort_covers(gs_ctx *L, const GsFrameUniforms &u) { return sort_covers(L->sort_near_req, u) ? GS_OK : ensure_full_sort(L); }

// per-frame buffers of lane `ctx` for the viewport of `u`
int gs_ctl::ensure_frame_buffers(gs_ctx *ctx, const GsFrameUniforms &u, bool need_fb)
{
    const size_t sw = (size_t)(u.x1 - u.x0), fb_bytes = sw * (size_t)u.H * 4;
    const size_t ntiles = (size_t)u.tiles_x * u.tiles_y;
    if (ntiles > ctx->tile_cap) { dev_free(ctx->tile_range); TRY(dev_alloc(ctx, &ctx->tile_range, ntiles)); ctx->tile_cap = ntiles; }
    if (need_fb && fb_bytes > ctx->fb_cap) { dev_free(ctx->fb); TRY(dev_alloc(ctx, &ctx->fb, fb_bytes)); ctx->fb_cap = fb_bytes; }
    if (!ctx->pair_cap) TRY(gs_ensure_pair_capacity(ctx, (size_t)1 << 22));
    const size_t mask_total = (size_t)u.tiles_y * u.mask_words;
    if (mask_total > ctx->mask_cap) { dev_free(ctx->unsat_mask); TRY(dev_alloc(ctx, &ctx->unsat_mask, mask_total)); ctx->mask_cap = mask_total; }
    if (ntiles * 256 > ctx->state_cap) { dev_free(ctx->state); TRY(dev_alloc(ctx, &ctx->state, ntiles * 256)); ctx->state_cap = ntiles * 256; }
    ctx->share_lane.last_two_rounds = u.near_count != 0xFFFFFFFFu && ctx->n && ctx->have_sort;
    ctx->stats.n_tiles = ntiles; ctx->stats.blend_launches = 1;
    return GS_OK;
}

// pipelined frame on lane `ctx`: enqueue and return; gs_sync() reads the control block back (its flags and accumulators
// are cumulative, so one read-back per gs_sync() covers every frame since the last one -- a per-frame copy would be one
// more queue entry per frame).  An overflowing frame shows the background only and is reported (GS_E_RETRY) there.
// Runs on the lane's worker thread when GS_OPT_ENQUEUE_THREADS is on.
int gs_ctl::render_async_on_lane(gs_ctx *ctx, const GsFrameUniforms &u, void *device_rgba, uint8_t *host_rgba, size_t stride)
{
    TRY(ensure_frame_buffers(ctx, u, device_rgba == nullptr));
    TRY(ensure_sort_covers(ctx, u));
    TRY(gs_run_render(ctx, u, (uint8_t *)device_rgba));
    if (host_rgba) {
        // the frame follows its kernels on the lane's stream (page-locked destination: a real asynchronous copy that
        // overlaps the next frames' kernels; pageable memory works too, through the runtime's staging)
        const size_t sw = (size_t)(u.x1 - u.x0);
        const uint8_t *src = device_rgba ? (const uint8_t *)device_rgba : ctx->fb;
        GS_HIP(hipMemcpy2DAsync(host_rgba, stride ? stride : sw * 4, src, sw * 4, sw * 4, (size_t)u.H, hipMemcpyDeviceToHost, ctx->stream));
    }
    return prof_advance(ctx);
}

// a collected sort's order to the caller: its length (the control block has been read back), the statistics that go with it, the list
static int deliver_order(gs_ctx *ctx /* the sort's lane */, uint32_t *out_idx, uint32_t *out_n)
{
    const uint32_t V = ctx->ctl_host->n_kept;
    ctx->stats.n_sorted = V; ctx->sorted_n_host = V; ctx->stats.n_hidden = ctx->sort_hidden;
    if (out_n) *out_n = V;
    if (out_idx && V) GS_HIP(hipMemcpy(out_idx, ctx->sorted, (size_t)V * 4, hipMemcpyDeviceToHost));
    return GS_OK;
}

extern "C" {

static int sort_common(gs_ctx *ctx, const float view[4], const float *cutout16, const GsSortStrip *strip, uint32_t *out_idx, uint32_t *out_n, bool solo = false);

GS_API int gs_sort(gs_ctx *ctx, const float view[4], const float *cutout16, uint32_t *out_idx, uint32_t *out_n)
{
    return sort_common(ctx, view, cutout16, nullptr, out_idx, out_n);
}

// the sort of a frame of two views drawn by this context (gs_sort_gathered): with GS_OPT_FRAME_BATCH the frame stays on a primary lane
int gs_sort_two_views(gs_ctx *ctx, const float view[4], const float *cutout16) { return sort_common(ctx, view, cutout16, nullptr, nullptr, nullptr, true); }

GS_API int gs_sort_for(gs_ctx *ctx, const float view[4], const float *cutout16, const gs_render_params *strip, uint32_t *out_idx, uint32_t *out_n)
{
    CHECK_CTX(ctx);
    if (!strip) return sort_common(ctx, view, cutout16, nullptr, out_idx, out_n);
    if (strip->fb_width <= 0 || strip->x0 < 0 || strip->x1 > strip->fb_width || strip->x0 >= strip->x1)
        FAIL(GS_E_BADARG, "gs_sort_for: bad strip [%d,%d) for width %d", strip->x0, strip->x1, strip->fb_width);
    GsSortStrip st;
    memcpy(st.mv, strip->model_view, sizeof st.mv); memcpy(st.proj, strip->projection, sizeof st.proj);
    st.focal = strip->focal > 0 ? strip->focal : (float)(((double)strip->fb_height / 2.0) * fabs((double)strip->projection[5]));
    st.vw = (float)strip->fb_width; st.vh = (float)strip->fb_height; st.x0 = strip->x0; st.x1 = strip->x1;
    // a perspective projection whose w does not depend on x or y (three.js PerspectiveCamera, WebXR eye frusta); anything else
    // is sorted whole
    const float *P = strip->projection;
    const bool parallel = (strip->flags & GS_RENDER_PARALLEL) != 0;
    if (parallel && !gsm::parallel_matrix_ok(P))
        FAIL(GS_E_BADARG, "gs_sort_for: GS_RENDER_PARALLEL: the projection's bottom row is (%g, %g, %g, %g), not (0, 0, 0, 1)", (double)P[3], (double)P[7], (double)P[11], (double)P[15]);
    // (a parallel camera: the reach test's bound is the perspective Jacobian's, so such a strip keeps every splat -- the order is gs_sort's)
    const bool persp = !parallel && P[3] == 0.0f && P[7] == 0.0f && P[15] == 0.0f && P[11] != 0.0f;
    return sort_common(ctx, view, cutout16, persp ? &st : nullptr, out_idx, out_n);
}

static int sort_common(gs_ctx *ctx, const float view[4], const float *cutout16, const GsSortStrip *strip, uint32_t *out_idx, uint32_t *out_n, bool solo)
{
    CHECK_CTX(ctx);
    if (!view) FAIL(GS_E_BADARG, "gs_sort: view is NULL");
    if (ctx->n == 0) {                                          // sort before any push (index.js:588-590)
        if (out_idx) out_idx[0] = 0;
        if (out_n) *out_n = 1;
        ctx->lanes[ctx->cur]->have_sort = false; ctx->lanes[ctx->cur]->stats.n_sorted = 0;
        if (ctx->lanes[ctx->cur]->log) ctx->lanes[ctx->cur]->log->open = false;
        return GS_OK;
    }
    GS_HIP(hipSetDevice(ctx->device));
    // a sort starts a frame: it goes to the next lane if the previous frame was handed off with GS_RENDER_ASYNC
    gs_ctx *L = nullptr;
    int rot = 0;
    const int lane = next_frame_lane(ctx, &rot, solo);
    TRY(get_lane(ctx, lane, &L));
    if (solo && ctx->frame_batch == 2 && lane < GS_MAX_PRIMARY) { gs_ctx *T = nullptr; TRY(get_lane(ctx, lane + GS_MAX_PRIMARY, &T)); }   // (the second view's scratch)
    if (ctx->pend_lane > 0 && lane == ctx->pend_lane - 1) FAIL(GS_E_STATE, "gs_sort: this frame's lane holds the sort begun with gs_sort_begin: collect it with gs_sort_poll first");
    set_current_lane(ctx, lane, rot);
    log_sort(L, view, cutout16, strip);
    {   // The share of splats binned first is measured in POSITIONS of the order the frames are drawn from.  A strip's order (gs_sort_for: the
        // splats that can reach the strip -- the whole frame: the frustum) is a sub-sequence of the whole one: "the nearest 30 000" of it reach
        // five times as deep.  When the kind of order changes, what was measured on the other kind is dropped (round 6: bench.py's frames sorted
        // for their frustum, then its one-frame-at-a-time extras with gs_sort, drew those with a share a fifth of what they needed and were
        // drawn again by gs_sync until the share had crept up).
        const uint32_t kind = strip ? 2u : 1u;                      // (strips of one frame differ less from each other than any of them from the whole order:
                                                                    // a context that draws several strips in turn keeps one measurement, as before)
        if (ctx->share.share_kind && ctx->share.share_kind != kind && ctx->share.near_fixed_permille <= 0) { gs_share_reset_kind_switch(ctx->share); reseed_lanes(ctx); }
        ctx->share.share_kind = kind;
    }
    const uint32_t near_req = (out_idx || out_n) ? 0u : (ctx->sort_near_force ? sort_near_forced(ctx) : sort_near_request(ctx));     // (the caller wants the order itself: all of it)
    // (a context that has not measured its share yet draws its next frame synchronously -- gs_render_uniforms --: its sort on the caller's
    // thread then, not on an enqueue thread that was created a moment ago and has to be woken first: 0.14 ms of that call's 0.7)
    // (... at most two sorts in a row: a context whose frames never measure -- counting renders -- keeps its threads)
    const bool cold = !ctx->share.share_measured && ctx->share.near_fixed_permille <= 0 && ctx->share.cold_sorts < 2u;   // (get_lane has drained the lane: nothing of it is waiting on its thread)
    if (cold) ctx->share.cold_sorts++; else if (ctx->share.share_measured) { ctx->share.cold_sorts = 0; ctx->share.cold_frames = 0; }
    if (ctx->enqueue_threads && gs_rotates(ctx) && !ctx->user_stream && !out_idx && !out_n && !cold) {
        // nothing to hand back: the lane's worker thread does the launching (a failure surfaces at gs_sync())
        GsLaneCmd c;
        c.type = GS_CMD_SORT; memcpy(c.view, view, sizeof c.view);
        c.has_cutout = cutout16 != nullptr;
        if (cutout16) memcpy(c.cutout, cutout16, sizeof c.cutout);
        c.has_strip = strip != nullptr;
        if (strip) c.strip = *strip;
        c.near_req = near_req;
        c.device_rgba = nullptr; c.host_rgba = nullptr; c.stride = 0;
        L->have_sort = true;                                    // (set again by the worker; the render command follows it)
        if (lane_push(L, c) != GS_OK) FAIL(GS_E_OOM, "out of host memory");
        return GS_OK;
    }
    TRY(lane_rc(ctx, L, gs_run_sort(L, view, cutout16, strip, near_req)));
    if (out_idx || out_n) {
        TRY(lane_rc(ctx, L, lane_read_control(L, true)));
        TRY(lane_rc(ctx, L, deliver_order(L, out_idx, out_n)));
    }
    return GS_OK;
}

// ---- the reference's single-flight rhythm (include/gs_splat.h: gs_sort_begin / gs_sort_poll; index.js:201-207, 438-455)
GS_API int gs_sort_begin(gs_ctx *ctx, const float view[4], const float *cutout16)
{
    CHECK_CTX(ctx);
    if (!view) FAIL(GS_E_BADARG, "gs_sort_begin: view is NULL");
    if (ctx->pend_lane) FAIL(GS_E_STATE, "gs_sort_begin: a sort is in flight (sortReady is false, index.js:439-440): collect it with gs_sort_poll");
    if (ctx->n == 0) { ctx->pend_lane = -1; return GS_OK; }     // sort before any push: the reply will be [0] (index.js:588-590)
    GS_HIP(hipSetDevice(ctx->device));
    // the lane the sort runs on: a primary lane other than the one whose order the draws use (created on first use, whatever
    // GS_OPT_PIPELINE_DEPTH says: the order in flight needs scratch of its own)
    const int front = ctx->cur % GS_MAX_PRIMARY;
    const int back = (front + 1) % (ctx->pipe_depth > 2 ? ctx->pipe_depth : 2);
    gs_ctx *B = nullptr;
    TRY(get_lane(ctx, back, &B));                                // (drained: nothing of it waits on its enqueue thread)
    if (!ctx->ev_sort) GS_HIP(hipEventCreateWithFlags(&ctx->ev_sort, hipEventDisableTiming));
    const int rc = lane_rc(ctx, B, gs_run_sort(B, view, cutout16, nullptr, 0));
    B->have_sort = false;                                        // (not an order to draw from until it has been collected)
    if (rc != GS_OK) return rc;
    TRY(lane_rc(ctx, B, lane_read_control(B, false)));
    GS_HIP(hipEventRecord(ctx->ev_sort, B->stream));
    ctx->pend_lane = back + 1; ctx->pend_n = ctx->n; ctx->pend_gen = B->sort_gen;
    memcpy(ctx->pend_view, view, sizeof ctx->pend_view); ctx->pend_has_cutout = cutout16 != nullptr;
    if (cutout16) memcpy(ctx->pend_cutout, cutout16, sizeof ctx->pend_cutout);
    return GS_OK;
}

GS_API int gs_sort_poll(gs_ctx *ctx, int wait, uint32_t *out_idx, uint32_t *out_n, int *done)
{
    CHECK_CTX(ctx);
    if (!done) FAIL(GS_E_BADARG, "gs_sort_poll: done is NULL");
    *done = 1;
    if (out_n) *out_n = 0;
    if (!ctx->pend_lane) return GS_OK;
    if (ctx->pend_lane < 0) {                                    // begun before any push
        ctx->pend_lane = 0;
        if (ctx->n == 0) { if (out_idx) out_idx[0] = 0; if (out_n) *out_n = 1; return GS_OK; }
        FAIL(GS_E_STATE, "gs_sort_poll: the sort was begun on an empty context and splats were pushed since: begin it again");
    }
    GS_HIP(hipSetDevice(ctx->device));
    const int back = ctx->pend_lane - 1;
    gs_ctx *B = ctx->lanes[back];
    if (!wait) {
        const hipError_t e = hipEventQuery(ctx->ev_sort);
        if (e == hipErrorNotReady) { *done = 0; return GS_OK; }
        if (e != hipSuccess) { ctx->pend_lane = 0; FAIL(GS_E_HIP, "hipEventQuery failed: %s", hipGetErrorString(e)); }
    } else GS_HIP(hipEventSynchronize(ctx->ev_sort));
    ctx->pend_lane = 0;
    if (ctx->pend_n != ctx->n || B->n != ctx->n || !B->sorted || B->sort_gen != ctx->pend_gen) {
        // the resident data changed under the sort (pushes drain every lane and drop the lanes' orders), or another sort has used the lane's
        // scratch since (gs_sync drawing a flagged frame of this lane again): over what is resident now
        gs_ctx *L = nullptr;
        TRY(get_lane(ctx, back, &L));
        TRY(lane_rc(ctx, L, gs_run_sort(L, ctx->pend_view, ctx->pend_has_cutout ? ctx->pend_cutout : nullptr, nullptr, 0)));
        TRY(lane_rc(ctx, L, lane_read_control(L, true)));
        B = L;
    }
    B->have_sort = true;
    TRY(lane_rc(ctx, B, deliver_order(B, out_idx, out_n)));
    // the new order is the one the draws use from here on (the reply handler, index.js:201-207)
    set_current_lane(ctx, back, 2 * back);
    log_sort(B, B->sv_view, B->sv_has_cutout ? B->sv_cutout : nullptr, nullptr);
    return GS_OK;
}

// Begin a frame whose sort is a call (gs_comm.hip: the order comes from -- or goes to -- the other ranks).  Two steps, so that the
// caller can take what must stay in step across the ranks (its turn in the sort rota, the communicator ticket) only after
// everything that can fail without the call having been queued -- here: lane selection and the lane's scratch -- has succeeded.
int gs_sort_call_begin(gs_ctx *ctx, const float view[4], const float *cutout16)
{
    CHECK_CTX(ctx);
    GS_HIP(hipSetDevice(ctx->device));
    gs_ctx *L = nullptr;
    int rot = 0;
    const int lane = next_frame_lane(ctx, &rot, false);
    TRY(get_lane(ctx, lane, &L));
    set_current_lane(ctx, lane, rot);
    log_sort(L, view, cutout16, nullptr);
    log_undecidable(L);                                            // (the other ranks are part of this frame's sort)
    L->have_sort = true;
    return GS_OK;
}

// ... and hand the call to the frame's lane: queued behind the lane's work, or run here.  The call is ALWAYS run.
int gs_sort_call_issue(gs_ctx *ctx, void *call_p)
{
    std::function<int(gs_ctx *)> &call = *static_cast<std::function<int(gs_ctx *)> *>(call_p);
    gs_ctx *L = ctx->lanes[ctx->cur];
    if (ctx->enqueue_threads && gs_rotates(ctx) && !ctx->user_stream) {
        GsLaneCmd c;
        c.type = GS_CMD_CALL; c.has_cutout = false; c.has_strip = false; c.device_rgba = nullptr; c.host_rgba = nullptr; c.stride = 0;
        bool queued = false;
        try { c.call = call; queued = lane_push(L, c) == GS_OK; } catch (...) { queued = false; }
        if (queued) return GS_OK;                                  // (not a frame's end: the rotation is decided by its render)
    }
    const int rc = lane_rc(ctx, L, lane_drain(L));                 // run here, whatever came before: the other ranks wait for this exchange
    const int rc2 = lane_rc(ctx, L, call(L));
    return rc != GS_OK ? rc : rc2;
}

int gs_sort_by_call(gs_ctx *ctx, const float view[4], const float *cutout16, void *call_p)
{
    TRY(gs_sort_call_begin(ctx, view, cutout16));
    return gs_sort_call_issue(ctx, call_p);
}

// GS_OPT_ROW_WALK = 1 walks the rows in frames that follow a collected frame whose visible splats touched at least GS_ROW_WALK_RATIO tiles
// each on average and whose tile rows held at most GS_ROW_WALK_RUNS runs each (docs/LAB_NOTES.md, round 7: the measurements)
#ifndef GS_ROW_WALK_RATIO
#define GS_ROW_WALK_RATIO 32.0
#endif
#ifndef GS_ROW_WALK_RUNS
#define GS_ROW_WALK_RUNS 8192.0
#endif
int gs_fill_uniforms(gs_ctx *ctx /* owner: options, adaptive share, scene */, const gs_render_params *p, GsFrameUniforms &u)
{
    if (!p) FAIL(GS_E_BADARG, "render params NULL");
    if (p->fb_width <= 0 || p->fb_height <= 0 || p->fb_width > 65535 * GS_TILE || p->fb_height > 65535 * GS_TILE)
        FAIL(GS_E_BADARG, "bad framebuffer size %dx%d", p->fb_width, p->fb_height);
    if (p->x0 < 0 || p->x1 > p->fb_width || p->x0 >= p->x1) FAIL(GS_E_BADARG, "bad strip [%d,%d) for width %d", p->x0, p->x1, p->fb_width);
    // a parallel camera (GS_RENDER_PARALLEL): w must not depend on the position -- checked here, the one door every frame, strip, eye, pick
    // and screen-space selection goes through
    if ((p->flags & GS_RENDER_PARALLEL) && !gsm::parallel_matrix_ok(p->projection))
        FAIL(GS_E_BADARG, "GS_RENDER_PARALLEL: the projection's bottom row is (%g, %g, %g, %g), not (0, 0, 0, 1)", (double)p->projection[3], (double)p->projection[7],
             (double)p->projection[11], (double)p->projection[15]);
    memcpy(u.mv, p->model_view, sizeof u.mv); memcpy(u.proj, p->projection, sizeof u.proj);
    u.W = p->fb_width; u.H = p->fb_height; u.x0 = p->x0; u.x1 = p->x1;
    u.out_pitch = p->x1 - p->x0;
    u.rc_stride = 0;                                               // (the binning is chosen per round: gs_render.hip)
    u.status = nullptr;                                            // (the frame's lane supplies its own word: gs_render_uniforms)
    u.need_seed = 0;
    u.x1b = p->x0 + ((p->x1 - p->x0 + 3) & ~3);
    if (u.x1b > p->fb_width) u.x1b = p->fb_width;
    u.vw = (float)p->fb_width; u.vh = (float)p->fb_height;
    // focal = (viewport.w / 2) * |P[5]| in JS f64, uploaded as a float uniform (index.js:191-194)
    u.focal = p->focal > 0 ? p->focal : (float)(((double)p->fb_height / 2.0) * fabs((double)p->projection[5]));
    u.tiles_x = (p->x1 - p->x0 + GS_TILE - 1) / GS_TILE; u.tiles_y = (p->fb_height + GS_TILE - 1) / GS_TILE;
    // the pair sort keys on the tile id in two digits of at most 9 bits (GS_RADIX_MAX_BINS): 2^18 tiles = 67 Mpixel per strip
    if ((uint64_t)u.tiles_x * (uint64_t)u.tiles_y > (1ull << 18))
        FAIL(GS_E_BADARG, "strip of %dx%d pixels has %llu tiles; at most 262144 (16x16-pixel tiles) are supported: render it in column strips",
             p->x1 - p->x0, p->fb_height, (unsigned long long)u.tiles_x * (unsigned long long)u.tiles_y);
    memcpy(u.bg, p->background, sizeof u.bg);
    u.t_eps = ctx->t_eps; u.flags = p->flags; u.record_staged = ctx->record_staged; u.split_min = ctx->blend_split_min;
    u.mask_words = (uint32_t)(u.tiles_x + 31) / 32;
    // round 0 covers the nearest near_frac * N splats; counting / no-early-out renders need every fragment -> one round
    u.near_count = (p->flags & (GS_RENDER_COUNT_FRAGS | GS_RENDER_NO_EARLY_OUT)) ? 0xFFFFFFFFu : gs_share_near_count(ctx->share, ctx->n);
    u.has_depth = ctx->scene_depth != nullptr; u.has_scene_rgba = ctx->scene_rgba != nullptr;
    if ((u.has_depth || u.has_scene_rgba) && (ctx->scene_w != p->fb_width || ctx->scene_h != p->fb_height))
        FAIL(GS_E_BADARG, "scene inputs are %dx%d but the frame is %dx%d", ctx->scene_w, ctx->scene_h, p->fb_width, p->fb_height);
    u.skip_round1 = (u.near_count != 0xFFFFFFFFu && gs_share_round1_skippable(ctx->share)) ? 1u : 0u;
    // sub-tile lists in the blend (GS_OPT_SUBTILE): where the last collected frame's visible splats touched few tiles each
    static const double subtile_ratio = getenv("GS_SUBTILE_RATIO") ? atof(getenv("GS_SUBTILE_RATIO")) : 16.0;
    u.subtile = ctx->subtile_opt == 2 ? 1u : (ctx->subtile_opt == 1 && ctx->last_visible && (double)ctx->last_pairs < subtile_ratio * (double)ctx->last_visible ? 1u : 0u);
    // row walk in the blend (GS_OPT_ROW_WALK): where the last collected frame's visible splats were large (a tile's nearest runs mostly
    // cover it: the walk finds its entries in few steps) and its tile rows held few runs; never with sub-tile lists (small splats)
    // (GS_ROW_WALK_RATIO / GS_ROW_WALK_RUNS in the environment override the two bounds)
    static const double walk_ratio = getenv("GS_ROW_WALK_RATIO") ? atof(getenv("GS_ROW_WALK_RATIO")) : GS_ROW_WALK_RATIO;
    static const double walk_runs = getenv("GS_ROW_WALK_RUNS") ? atof(getenv("GS_ROW_WALK_RUNS")) : GS_ROW_WALK_RUNS;
    const uint32_t runs = __atomic_load_n(&ctx->run_hint, __ATOMIC_RELAXED);
    u.row_walk = ctx->row_walk_opt == 2 ? 1u : (ctx->row_walk_opt == 1 && !u.subtile && ctx->last_visible && runs &&
                                                (double)ctx->last_pairs >= walk_ratio * (double)ctx->last_visible &&
                                                (double)runs <= walk_runs * (double)u.tiles_y ? 1u : 0u);
    // (measurement renders, sub-tile lists and the split blend keep the tile lists)
    if ((u.flags & GS_RENDER_COUNT_FRAGS) || u.record_staged || u.subtile || u.split_min) u.row_walk = 0;
    u.walk_ref = 0;
    // view-dependent colour (GS_OPT_SH_DEGREE): the degree the frame evaluates and the camera it evaluates for
    u.sh_degree = 0; u.sh_n = 0; u.sh_row_q = 0; u.sh_rows = nullptr; u.sh_cam[0] = u.sh_cam[1] = u.sh_cam[2] = 0.0;
    if (ctx->sh_opt > 0 && ctx->sh_n) {
        u.sh_degree = (uint32_t)(ctx->sh_opt < ctx->sh_deg ? ctx->sh_opt : ctx->sh_deg);
        u.sh_n = (uint32_t)ctx->sh_n; u.sh_row_q = 3u * (uint32_t)gsm::sh_channel_stride(ctx->sh_deg) / 4u;
        u.sh_rows = reinterpret_cast<const uint4 *>(ctx->sh);
        const bool regular = gsm::camera_in_object(u.mv, u.sh_cam);
        u.sh_cam[2] = -u.sh_cam[2];                                  // model_view acts on (x, y, -z): back to the rows' space (gs_sh.h)
        if (!regular) FAIL(GS_E_BADARG, "model_view is singular: no camera position to evaluate the spherical harmonics for");
    }
    u.surf_id = nullptr; u.surf_depth = nullptr; u.surf_alpha = nullptr; u.surface = 0;   // (gs_render_surface sets them)
    u.contrib = nullptr; u.contrib_rows = 0; u.contribute = 0;      // (gs_render_contrib sets them)
    u.antialias = ctx->aa_opt ? 1u : 0u;                            // compensated opacity (GS_OPT_ANTIALIAS), per frame like the SH degree
    // highlighted selection (GS_OPT_HIGHLIGHT), per frame too: only with a weight AND a store -- a context that never edits keeps its kernels
    const bool hl = (ctx->hl_opt >> 24) != 0u && ctx->edit_n != 0 && ctx->edit_state;
    u.highlight = hl ? ctx->hl_opt : 0u; u.hl_rows = hl ? (uint32_t)ctx->edit_n : 0u; u.hl_state = hl ? ctx->edit_state : nullptr;
    return GS_OK;
}

static bool gs_debug_cold() { static const bool on = getenv("GS_DEBUG_COLD") != nullptr; return on; }   // (diagnostic: what a synchronous frame's call spends where)

// synchronous frame on lane `ctx` (the owner supplies options and the adaptive share through fill_uniforms)
static int render_sync_on_lane(gs_ctx *ctx, const GsFrameUniforms &u, void *device_rgba, uint8_t *host_rgba, size_t stride)
{
    const size_t sw = (size_t)(u.x1 - u.x0);
    TRY(ensure_frame_buffers(ctx, u, device_rgba == nullptr));
    TRY(ensure_sort_covers(ctx, u));
    if (host_rgba) {
        if (!stride) stride = sw * 4;
        if (stride < sw * 4) FAIL(GS_E_BADARG, "stride %zu smaller than a row (%zu bytes)", stride, sw * 4);
    }
    // the frame's way to the host is queued right behind its kernels, before the control block has told whether the frame is
    // complete (one stream synchronisation per frame instead of two); the rare frame that is not is drawn and copied again
    auto queue_copy = [&]() -> int {
        if (!host_rgba) return GS_OK;
        const uint8_t *src = device_rgba ? (const uint8_t *)device_rgba : ctx->fb;
        // (a tight frame is ONE linear copy: the 2-D form goes through a slower path of the runtime even when pitch == width)
        if (stride == sw * 4) GS_HIP(hipMemcpyAsync(host_rgba, src, sw * 4 * (size_t)u.H, hipMemcpyDeviceToHost, ctx->stream));
        else GS_HIP(hipMemcpy2DAsync(host_rgba, stride, src, sw * 4, sw * 4, (size_t)u.H, hipMemcpyDeviceToHost, ctx->stream));
        return GS_OK;
    };
    for (int attempt = 0;; attempt++) {
        // (a contribution frame that is drawn again must not count twice: the store is copied behind itself in front of the frame's kernels,
        // on their stream -- no wait --, and comes back from there in front of a second attempt)
        if (u.contribute) {
            gs_ctx *P = gs_root(ctx);
            unsigned long long *store = P->contrib, *copy = P->contrib + P->contrib_cap;
            if (P->contrib_n) GS_HIP(hipMemcpyAsync(attempt ? store : copy, attempt ? copy : store, P->contrib_n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, ctx->stream));
            P->contrib_copied = true;
        }
        TRY(gs_run_render(ctx, u, (uint8_t *)device_rgba));
        TRY(lane_read_control(ctx, false));
        TRY(queue_copy());
        GS_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->profile && ctx->ring) { ctx->ring_head++; ctx->ring_pending++; TRY(prof_drain(ctx)); }
        if (ctx->ctl_host->order_incomplete) {
            // the order this frame was drawn from was incomplete (a near-only sort whose survivors overflowed a chunk's stash, an
            // exchanged order cut short): round 0 itself was blended from the wrong positions.  Sort in full, draw the whole frame again.
            gs_ctx *P = gs_root(ctx);
            GS_HIP(hipMemsetAsync(&ctx->ctl->order_incomplete, 0, sizeof(uint32_t), ctx->stream));
            GS_HIP(hipMemsetAsync(&ctx->ctl->round1_missed, 0, sizeof(uint32_t), ctx->stream));
            if (ctx->ctl_host->near_overflow) { __atomic_store_n(&P->near_stash_off, true, __ATOMIC_RELAXED); GS_HIP(hipMemsetAsync(&ctx->ctl->near_overflow, 0, sizeof(uint32_t), ctx->stream)); }
            if (ctx->ctl_host->spec_fail) { P->stats.spec_misses++; gs_spec_back_off(P, ctx->ctl_host->spec_fail == 2u); GS_HIP(hipMemsetAsync(&ctx->ctl->spec_fail, 0, sizeof(uint32_t), ctx->stream)); }
            if (attempt >= 2) FAIL(GS_E_HIP, "the sorted order keeps coming back incomplete");
            TRY(gs_run_sort(ctx, ctx->sv_view, ctx->sv_has_cutout ? ctx->sv_cutout : nullptr, ctx->sv_has_strip ? &ctx->sv_strip : nullptr, 0));
            P->stats.retried_frames++;
            continue;
        }
        if (ctx->ctl_host->round1_missed) {
            // round 1 was skipped but a tile did not saturate: its mask bit and per-pixel state are intact -- finish it now
            GS_HIP(hipMemsetAsync(&ctx->ctl->round1_missed, 0, sizeof(uint32_t), ctx->stream));
            TRY(ensure_full_sort(ctx));                             // (round 1 reads the far part of the order)
            TRY(gs_run_round1(ctx, u, (uint8_t *)device_rgba));
            TRY(lane_read_control(ctx, false));
            TRY(queue_copy());
            GS_HIP(hipStreamSynchronize(ctx->stream));
            ctx->ctl_host->round1_missed = 1;                      // seen by the adaptation below
        }
        bool over = false;
        GsShareTally tally{};
        const float frac_used = gs_root(ctx)->share.near_frac;
        TRY(collect_status(ctx, &over, tally, nullptr));
        decide_share(gs_root(ctx), frac_used, tally, true);
        if (!over) break;
        if (attempt >= 2) FAIL(GS_E_OOM, "pair list keeps overflowing (%u pairs)", ctx->ctl_host->scan_total);
    }
    ctx->async_pending = false;
    if (u.flags & GS_RENDER_COUNT_FRAGS) ctx->stats.n_frags = ctx->ctl_host->n_frags;
    return GS_OK;
}

// the frame's lane runs `call` after everything handed to it so far: on its worker thread for asynchronous frames (so the
// caller keeps enqueuing), on the caller's thread otherwise.  The call's failure surfaces like a render's.
// always: the call runs even if something handed to the lane before it has failed, or the hand-over itself fails (the gather of
// a frame, which the other ranks wait for); the earlier failure is what is returned.
int gs_lane_call(gs_ctx *ctx, bool async, std::function<int(gs_ctx *)> call, bool always)
{
    gs_ctx *L = ctx->lanes[ctx->cur];
    if (always) log_undecidable(L);                                // (a frame's gather: every rank would have to draw it again)
    if (async && ctx->enqueue_threads && gs_rotates(ctx) && !ctx->user_stream) {
        GsLaneCmd c;
        c.type = GS_CMD_CALL; c.has_cutout = false; c.has_strip = false; c.device_rgba = nullptr; c.host_rgba = nullptr; c.stride = 0; c.call = call;
        L->async_pending = true; ctx->cur_async = true;
        if (lane_push(L, c) == GS_OK) return GS_OK;
        if (!always) FAIL(GS_E_OOM, "out of host memory");
    }
    const int rc = lane_rc(ctx, L, lane_drain(L));
    if (rc != GS_OK && !always) return rc;
    const int rc2 = lane_rc(ctx, L, call(L));
    return rc != GS_OK ? rc : rc2;
}

// whether round 0 of frame `u` on lane L walks its tile rows: chosen, and the frame is binned by span lists (run_round: at most 256
// tile columns and rows, a row-count table within its limit, not GS_OPT_BINNING = 1)
static bool row_walk_taken(const gs_ctx *L, const GsFrameUniforms &u)
{
    const gs_ctx *P = gs_root(const_cast<gs_ctx *>(L));
    return u.row_walk && P->bin_mode != 1 && u.tiles_x <= 256 && u.tiles_y <= 256 && gs_row_tables_entries(P->n, (uint32_t)u.tiles_y) != 0;
}

static int render_common(gs_ctx *ctx, const gs_render_params *p, void *device_rgba, uint8_t *host_rgba, size_t stride)
{
    GsFrameUniforms u;
    TRY(gs_fill_uniforms(ctx, p, u));
    return gs_render_uniforms(ctx, u, device_rgba, host_rgba, stride);
}

int gs_render_uniforms(gs_ctx *ctx, const GsFrameUniforms &u_in, void *device_rgba, uint8_t *host_rgba, size_t stride)
{
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "context was fed worker matrices only (gs_push_matrices): it can sort but not render");
    GS_HIP(hipSetDevice(ctx->device));
    GsFrameUniforms u = u_in;
    if (host_rgba && !device_rgba) {
        const size_t row = (size_t)(u.x1 - u.x0) * 4, st = stride ? stride : row;
        if (st < row) FAIL(GS_E_BADARG, "stride %zu smaller than a row (%zu bytes)", st, row);
    }
    gs_ctx *L = ctx->lanes[ctx->cur];                           // the frame's lane: where its gs_sort ran
    // the completion word of this frame: the next word of the lane's ring (a gathered piece brings its own: the piece's trailer)
    if (!L->async_pending) L->status_base = L->status_seq;       // (nothing of the lane waits for a collection: the frames to come count from here)
    if (!u.status) { u.status = &L->ctl->status_ring[L->status_seq % GS_STATUS_RING]; L->status_seq++; }
    L->status_cur = u.status;
    L->stats.subtile = u.subtile;
    L->stats.row_walk = row_walk_taken(L, u) ? 1u : 0u;
    L->stats.binning = gs_round0_binning(L, u);
    L->stats.sh_degree = u.sh_degree;
    L->stats.surface = u.surface ? 1u : 0u;
    L->stats.antialias = u.antialias ? 1u : 0u;
    L->hl_frame = u.highlight ? 1u : 0u;
    L->par_frame = (u.flags & GS_RENDER_PARALLEL) ? 1u : 0u;
    u.need_seed = L->share_lane.need_seed_pending; L->share_lane.need_seed_pending = 0;  // (a seed for the lane's need words travels with its next frame)
    bool async = (u.flags & GS_RENDER_ASYNC) && !(u.flags & GS_RENDER_COUNT_FRAGS);
    // A context that has not MEASURED its share yet (fresh, cleared, the share un-pinned) draws its first two-round frame synchronously
    // even when asked to queue it: the frames queued behind it then use the share it measured instead of the 25 % every context starts
    // with (at 20 M splats: 5 M positions in the first round of every frame until the first gs_sync).  The call returns with the frame
    // complete; its status needs no gs_sync.
    // (... at most two such frames in a row, like the cold sorts: a context whose blends never record a need -- counting renders, every tile
    // saturated by round 0 of a walked share -- would otherwise draw EVERY queued frame synchronously,
    // with a drain of every other lane each time: ADVICE r5)
    if (async && !ctx->share.share_measured && ctx->share.near_fixed_permille <= 0 && u.near_count != 0xFFFFFFFFu && ctx->n && ctx->share.cold_frames < 2u) {
        async = false; u.flags &= ~(uint32_t)GS_RENDER_ASYNC;
        ctx->share.cold_frames++;
        // ... and the lanes that exist get their per-frame buffers for this frame's size now (tile ranges, per-pixel state, row tables:
        // a dozen allocations each), while nothing is in flight, instead of one lane per frame over the next five.  (BEFORE the frame's
        // kernels go out, not under them: allocations made while the device works take longer than the wait they would hide -- the
        // call 0.93 ms instead of 0.66, tools/cold_probe.py)
        const auto dbg_t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < GS_MAX_LANES; i++) {
            gs_ctx *Li = ctx->lanes[i];
            if (!Li || Li == L || Li->scratch_cap < ctx->cap) continue;
            if (lane_drain(Li) != GS_OK) continue;
            (void)ensure_frame_buffers(Li, u, device_rgba == nullptr);
            if (const size_t e = (u.tiles_x <= 256 && u.tiles_y <= 256 && !ctx->bin_mode) ? gs_row_tables_entries(ctx->n, (uint32_t)u.tiles_y) : 0) (void)gs_row_tables_ensure(Li, e);
        }
        if (gs_debug_cold()) fprintf(stderr, "[gs] cold frame: the other lanes' buffers took %.0f us\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - dbg_t0).count());
    }
    if (async) {
        if (host_rgba && stride && stride < (size_t)(u.x1 - u.x0) * 4) FAIL(GS_E_BADARG, "stride %zu smaller than a row (%zu bytes)", stride, (size_t)(u.x1 - u.x0) * 4);
        L->async_pending = true; ctx->cur_async = true;
        log_render(L, u, device_rgba, host_rgba, stride);
        if (ctx->enqueue_threads && gs_rotates(ctx) && !ctx->user_stream) {
            GsLaneCmd c;
            c.type = GS_CMD_RENDER; c.has_cutout = false; c.has_strip = false; c.u = u; c.device_rgba = device_rgba; c.host_rgba = host_rgba; c.stride = stride;
            if (lane_push(L, c) != GS_OK) FAIL(GS_E_OOM, "out of host memory");
            return GS_OK;
        }
        TRY(lane_rc(ctx, L, lane_drain(L)));
        return lane_rc(ctx, L, render_async_on_lane(L, u, device_rgba, host_rgba, stride));
    }
    const auto dbg_t1 = std::chrono::steady_clock::now();
    TRY(lane_rc(ctx, L, lane_drain(L)));                         // whatever its worker still had to enqueue comes first
    const auto dbg_t2 = std::chrono::steady_clock::now();
    const int rcs = lane_rc(ctx, L, render_sync_on_lane(L, u, device_rgba, host_rgba, stride));
    if (gs_debug_cold()) fprintf(stderr, "[gs] synchronous frame: drain %.0f us, draw %.0f us\n", std::chrono::duration<double, std::micro>(dbg_t2 - dbg_t1).count(),
                                         std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - dbg_t2).count());
    return rcs;
}

GS_API int gs_render(gs_ctx *ctx, const gs_render_params *p, uint8_t *rgba_out, size_t stride)
{
    CHECK_CTX(ctx);
    if (!rgba_out) FAIL(GS_E_BADARG, "gs_render: rgba_out is NULL");
    return render_common(ctx, p, nullptr, rgba_out, stride);
}

GS_API int gs_render_device(gs_ctx *ctx, const gs_render_params *p, void *device_rgba)
{
    CHECK_CTX(ctx);
    return render_common(ctx, p, device_rgba, nullptr, 0);
}

GS_API int gs_render_stereo(gs_ctx *ctx, const gs_render_params eyes[2], uint8_t *rgba_out[2], size_t stride)
{
    CHECK_CTX(ctx);
    if (!eyes || !rgba_out || !rgba_out[0] || !rgba_out[1]) FAIL(GS_E_BADARG, "gs_render_stereo: NULL argument");
    TRY(render_common(ctx, &eyes[0], nullptr, rgba_out[0], stride));
    return render_common(ctx, &eyes[1], nullptr, rgba_out[1], stride);
}

// ---- surface output: per pixel the splat at which the transmittance falls below one half, its window depth, the accumulated alpha
// A surface frame is a synchronous frame on the tile lists (as a counting render is): the row walk, sub-tile lists and the split blend
// are switched off in ITS uniforms, the context's options stay what they are; paired launches serve queued frames only.
static int surface_common(gs_ctx *ctx, const gs_render_params *p, void *device_rgba, uint8_t *host_rgba, size_t stride, const gs_surface *dev)
{
    if (p && (p->flags & GS_RENDER_COUNT_FRAGS)) FAIL(GS_E_BADARG, "a surface frame cannot count fragments (GS_RENDER_COUNT_FRAGS)");
    GsFrameUniforms u;
    TRY(gs_fill_uniforms(ctx, p, u));
    u.flags &= ~(uint32_t)GS_RENDER_ASYNC;
    u.subtile = 0; u.row_walk = 0; u.split_min = 0;
    u.surface = 1; u.surf_id = dev->id; u.surf_depth = dev->depth; u.surf_alpha = dev->alpha;
    return gs_render_uniforms(ctx, u, device_rgba, host_rgba, stride);
}

// the context's own planes for a strip of sw x h pixels (owner; surface frames are synchronous: nothing in flight reads them)
static int surface_scratch(gs_ctx *ctx, size_t sw, size_t h, gs_surface *dev)
{
    const size_t plane = (sw * h * 4 + 255) & ~(size_t)255;
    if (3 * plane > ctx->surf_cap) {
        GS_HIP(hipSetDevice(ctx->device));
        dev_free(ctx->surf_buf); ctx->surf_cap = 0;
        TRY(dev_alloc(ctx, &ctx->surf_buf, 3 * plane));
        ctx->surf_cap = 3 * plane;
    }
    dev->id = reinterpret_cast<uint32_t *>(ctx->surf_buf);
    dev->depth = reinterpret_cast<float *>(ctx->surf_buf + plane);
    dev->alpha = reinterpret_cast<float *>(ctx->surf_buf + 2 * plane);
    return GS_OK;
}

GS_API int gs_render_surface_device(gs_ctx *ctx, const gs_render_params *p, void *device_rgba, const gs_surface *device_out)
{
    CHECK_CTX(ctx);
    if (!device_out) FAIL(GS_E_BADARG, "gs_render_surface_device: device_out is NULL");
    return surface_common(ctx, p, device_rgba, nullptr, 0, device_out);
}

GS_API int gs_render_surface(gs_ctx *ctx, const gs_render_params *p, uint8_t *rgba_out, size_t stride, const gs_surface *host_out)
{
    CHECK_CTX(ctx);
    if (!host_out) FAIL(GS_E_BADARG, "gs_render_surface: host_out is NULL");
    if (p && (p->flags & GS_RENDER_COUNT_FRAGS)) FAIL(GS_E_BADARG, "a surface frame cannot count fragments (GS_RENDER_COUNT_FRAGS)");
    GsFrameUniforms chk;
    TRY(gs_fill_uniforms(ctx, p, chk));                          // (the strip's size is known to be sane from here on)
    const size_t sw = (size_t)(p->x1 - p->x0), h = (size_t)p->fb_height;
    gs_surface dev;
    TRY(surface_scratch(ctx, sw, h, &dev));
    TRY(surface_common(ctx, p, nullptr, rgba_out, stride, &dev));
    // (the frame is complete: a synchronous frame returns behind its kernels)
    if (host_out->id) GS_HIP(hipMemcpy(host_out->id, dev.id, sw * h * 4, hipMemcpyDeviceToHost));
    if (host_out->depth) GS_HIP(hipMemcpy(host_out->depth, dev.depth, sw * h * 4, hipMemcpyDeviceToHost));
    if (host_out->alpha) GS_HIP(hipMemcpy(host_out->alpha, dev.alpha, sw * h * 4, hipMemcpyDeviceToHost));
    return GS_OK;
}

// ---- contribution frames: every splat's blend weights, summed over the frames drawn (include/gs_splat.h: "per-splat contribution")
// The store is the owner's, parallel to the splats like the SH rows and the states, made by the first contribution frame: one 64-bit sum of
// 16.16 weights per splat, the words behind contrib_n zero (whoever shortens the store clears what it gives up).  A contribution frame is a
// synchronous frame on the tile lists, as a surface frame is, whose blend (k_blend_contrib) adds to the store; a copy of the store, queued
// on the frame's stream in front of its kernels, lies behind it in the same allocation, for the frame that has to be drawn again -- an
// incomplete order, pair buffers that overflowed: any frame can meet the latter -- or fails (render_sync_on_lane).
// The property calls that read the store (gs_edit.hip: GS_PROP_SEEN) come after such a frame has returned: nothing is left to order.
static int contrib_ensure(gs_ctx *ctx)
{
    GS_HIP(hipSetDevice(ctx->device));
    const size_t want = ctx->n;
    if (want > ctx->contrib_cap) {
        size_t cap = ctx->contrib_cap ? ctx->contrib_cap : (size_t)1 << 16;
        while (cap < want) cap *= 2;
        unsigned long long *nw = nullptr;
        TRY(dev_alloc(ctx, &nw, 2 * cap));
        hipError_t e = hipMemsetAsync(nw, 0, cap * sizeof(unsigned long long), ctx->stream);
        if (e == hipSuccess && ctx->contrib_n) e = hipMemcpyAsync(nw, ctx->contrib, ctx->contrib_n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { dev_free(nw); FAIL(GS_E_HIP, "growing the contribution store failed: %s", hipGetErrorString(e)); }
        dev_free(ctx->contrib);
        ctx->contrib = nw; ctx->contrib_cap = cap;
    }
    if (want > ctx->contrib_n) ctx->contrib_n = want;             // (zero-filled: the words behind the old length are zero)
    return GS_OK;
}

static int contrib_common(gs_ctx *ctx, const gs_render_params *p, void *device_rgba, uint8_t *host_rgba, size_t stride)
{
    if (p && (p->flags & GS_RENDER_COUNT_FRAGS)) FAIL(GS_E_BADARG, "a contribution frame cannot count fragments (GS_RENDER_COUNT_FRAGS)");
    GsFrameUniforms u;
    TRY(gs_fill_uniforms(ctx, p, u));
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "context was fed worker matrices only (gs_push_matrices): it can sort but not render");
    TRY(contrib_ensure(ctx));
    u.flags &= ~(uint32_t)GS_RENDER_ASYNC;
    u.subtile = 0; u.row_walk = 0; u.split_min = 0;
    u.contribute = 1; u.contrib = ctx->contrib; u.contrib_rows = (uint32_t)ctx->contrib_n;
    ctx->contrib_copied = false;                                   // (render_sync_on_lane: set once this frame's copy of the store is queued)
    const int rc = gs_render_uniforms(ctx, u, device_rgba, host_rgba, stride);
    const gs_ctx *L = ctx->lanes[ctx->cur];
    if (rc != GS_OK) {
        // (whatever the frame added before it failed is taken back; the failure is the frame's)
        if (ctx->contrib_copied && ctx->contrib_n && hipStreamSynchronize(L->stream) == hipSuccess)
            (void)hipMemcpy(ctx->contrib, ctx->contrib + ctx->contrib_cap, ctx->contrib_n * sizeof(unsigned long long), hipMemcpyDeviceToDevice);
        return rc;
    }
    if (L->n && L->have_sort) ctx->contrib_frames++;              // (gs_run_render: without a completed order the frame is the background)
    return GS_OK;
}

GS_API int gs_render_contrib(gs_ctx *ctx, const gs_render_params *p, uint8_t *rgba_out, size_t stride)
{
    CHECK_CTX(ctx);
    return contrib_common(ctx, p, nullptr, rgba_out, stride);
}

GS_API int gs_render_contrib_device(gs_ctx *ctx, const gs_render_params *p, void *device_rgba)
{
    CHECK_CTX(ctx);
    return contrib_common(ctx, p, device_rgba, nullptr, 0);
}

GS_API int gs_contrib_clear(gs_ctx *ctx)
{
    CHECK_CTX(ctx);
    if (ctx->contrib && ctx->contrib_n) {
        GS_HIP(hipSetDevice(ctx->device));
        GS_HIP(hipMemsetAsync(ctx->contrib, 0, ctx->contrib_n * sizeof(unsigned long long), ctx->stream));
        GS_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->contrib_n = 0; ctx->contrib_frames = 0;
    return GS_OK;
}

GS_API int gs_contrib_info(const gs_ctx *ctx, size_t *rows, uint64_t *frames)
{
    if (!ctx) return GS_E_BADARG;
    if (rows) *rows = ctx->contrib_n;
    if (frames) *frames = ctx->contrib_frames;
    return GS_OK;
}

// One 16-pixel-aligned column strip per distinct tile column among the points: such a strip reproduces the full frame's columns bit
// for bit (include/gs_splat.h: strips whose x0 is a multiple of 4), and costs a sixteenth of a tile row's blend per tile row.
GS_API int gs_pick(gs_ctx *ctx, const gs_render_params *p, const int32_t *xy, size_t npoints, gs_hit *out)
{
    CHECK_CTX(ctx);
    if (!p) FAIL(GS_E_BADARG, "render params NULL");
    if (!out || (npoints && !xy)) FAIL(GS_E_BADARG, "gs_pick: NULL argument");
    if (p->flags & GS_RENDER_COUNT_FRAGS) FAIL(GS_E_BADARG, "a surface frame cannot count fragments (GS_RENDER_COUNT_FRAGS)");
    if (!ctx->renderable && ctx->n) FAIL(GS_E_STATE, "context was fed worker matrices only (gs_push_matrices): it can sort but not render");
    gs_render_params q = *p;
    q.x0 = 0; q.x1 = p->fb_width;
    GsFrameUniforms chk;
    TRY(gs_fill_uniforms(ctx, &q, chk));
    for (size_t i = 0; i < npoints; i++)
        if (xy[2 * i] < 0 || xy[2 * i] >= p->fb_width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= p->fb_height)
            FAIL(GS_E_BADARG, "gs_pick: point %zu (%d, %d) lies outside the %dx%d frame", i, xy[2 * i], xy[2 * i + 1], p->fb_width, p->fb_height);
    const size_t h = (size_t)p->fb_height;
    std::vector<bool> done(npoints, false);
    std::vector<uint32_t> host;                                  // the strip's three planes as the scratch holds them: one copy
    for (size_t i = 0; i < npoints; i++) {
        if (done[i]) continue;
        q.x0 = xy[2 * i] / GS_TILE * GS_TILE;
        q.x1 = q.x0 + GS_TILE < p->fb_width ? q.x0 + GS_TILE : p->fb_width;
        const size_t sw = (size_t)(q.x1 - q.x0);
        gs_surface dev;
        TRY(surface_scratch(ctx, sw, h, &dev));
        TRY(surface_common(ctx, &q, nullptr, nullptr, 0, &dev));
        const size_t plane = (size_t)(reinterpret_cast<uint8_t *>(dev.depth) - reinterpret_cast<uint8_t *>(dev.id)) / 4;   // words between two planes
        host.resize(2 * plane + sw * h);
        GS_HIP(hipMemcpy(host.data(), dev.id, host.size() * 4, hipMemcpyDeviceToHost));
        for (size_t k = i; k < npoints; k++) {
            if (done[k] || xy[2 * k] < q.x0 || xy[2 * k] >= q.x1) continue;
            const size_t o = (size_t)xy[2 * k + 1] * sw + (size_t)(xy[2 * k] - q.x0);
            gs_hit &hit = out[k];
            hit.id = host[o];
            memcpy(&hit.depth, &host[plane + o], 4); memcpy(&hit.alpha, &host[2 * plane + o], 4);
            hit.pos[0] = hit.pos[1] = hit.pos[2] = nanf("");
            if (hit.id != 0xFFFFFFFFu && hit.id < ctx->n) {
                float c[3];                                         // the packed centre (x, y, -z): index.js:350-354
                GS_HIP(hipMemcpy(c, ctx->splat + 2 * (size_t)hit.id, sizeof c, hipMemcpyDeviceToHost));
                hit.pos[0] = c[0]; hit.pos[1] = c[1]; hit.pos[2] = -c[2];
            }
            done[k] = true;
        }
    }
    return GS_OK;
}

// gs_sync found incomplete asynchronous frames on the lanes of bad_unit[]: draw the frames logged for those lanes again, in the
// order they were asked, synchronously (both binning rounds; a pair overflow grows the buffers and repeats inside
// render_sync_on_lane).  Every lane is drained and idle.  GS_E_RETRY when the library cannot decide alone (see GsFrameRec).
static int redraw_flagged_frames_impl(gs_ctx *ctx, const bool bad_unit[GS_MAX_PRIMARY]);
static int redraw_flagged_frames(gs_ctx *ctx, const bool bad_unit[GS_MAX_PRIMARY])
{
    // (the walk copies the log and keeps a set of outputs: out of host memory there, the caller draws the frames again itself)
    try { return redraw_flagged_frames_impl(ctx, bad_unit); } catch (...) { ctx->share.adapt_frozen = false; return GS_E_RETRY; }
}
static int redraw_flagged_frames_impl(gs_ctx *ctx, const bool bad_unit[GS_MAX_PRIMARY])
{
    // an output written by more than one logged frame (any lane): drawing one of them again could overwrite a newer image
    std::set<const void *> outs;
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (!L || !L->log) continue;
        for (const GsFrameRec &r : L->log->recs)
            for (int k = 0; k < r.nrender; k++) {
                const void *o = r.r[k].host ? (const void *)r.r[k].host : (r.r[k].dev ? (const void *)r.r[k].dev : (const void *)L);   // (the lane's own framebuffer)
                if (o != (const void *)L && !outs.insert(o).second) return GS_E_RETRY;
            }
    }
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (!L || !L->log || !bad_unit[i % GS_MAX_PRIMARY]) continue;
        for (const GsFrameRec &r : L->log->recs) if (r.nrender && r.undecidable) return GS_E_RETRY;
    }
    uint32_t redrawn = 0;
    struct Thaw { gs_ctx *c; ~Thaw() { c->share.adapt_frozen = false; } } thaw{ ctx };
    ctx->share.adapt_frozen = true;
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (!L || !L->log || !bad_unit[i % GS_MAX_PRIMARY]) continue;
        const std::vector<GsFrameRec> recs = L->log->recs;          // (render_sync_on_lane does not log, but keep the walk independent of it)
        // which of them: the frames whose completion word (read back with the control block) is not 0 -- as long as the lane's ring still
        // holds the word of every render since the last collection; else, or for a render whose word is not in the ring, all of them
        const bool words_valid = L->status_seq - L->status_base <= GS_STATUS_RING;
        for (const GsFrameRec &r : recs) {
            if (!r.nrender) continue;
            bool complete = words_valid;
            for (int k = 0; k < r.nrender && complete; k++) {
                const uint32_t *w = r.r[k].u.status;
                if (!w || w < L->ctl->status_ring || w >= L->ctl->status_ring + GS_STATUS_RING) complete = false;
                else if (L->ctl_host->status_ring[w - L->ctl->status_ring] != 0u) complete = false;
            }
            if (complete) continue;
            TRY(lane_rc(ctx, L, gs_run_sort(L, r.view, r.has_cutout ? r.cutout : nullptr, r.has_strip ? &r.strip : nullptr, 0)));
            for (int k = 0; k < r.nrender; k++) {
                GsFrameUniforms u = r.r[k].u;
                u.flags &= ~(uint32_t)GS_RENDER_ASYNC;
                u.skip_round1 = 0;                                   // both rounds: complete by construction
                u.need_seed = 0;                                     // (the seed it carried has been written)
                TRY(lane_rc(ctx, L, render_sync_on_lane(L, u, r.r[k].dev, r.r[k].host, r.r[k].stride)));
                redrawn++;
            }
        }
    }
    ctx->stats.retried_frames += redrawn;
    return GS_OK;
}

GS_API int gs_sync(gs_ctx *ctx)
{
    CHECK_CTX(ctx);
    GS_HIP(hipSetDevice(ctx->device));
    bool any_missed = false, any_over = false;
    uint32_t spec_failed = 0;
    GsShareTally tally{};
    const float frac_used = ctx->share.near_frac;                       // what every frame queued since the last collection was drawn with
    // whatever way this call ends, the frames logged so far are not drawn again by a LATER gs_sync (their output buffers may be
    // gone by then): a failure below leaves no records behind
    struct LogGuard { gs_ctx *c; ~LogGuard() { for (int i = 0; i < GS_MAX_LANES; i++) if (c->lanes[i]) log_reset(c->lanes[i]); } } log_guard{ ctx };
    bool bad_unit[GS_MAX_PRIMARY] = { false, false, false, false };   // a lane or its twin (one stream, one worker) reported an incomplete frame
    uint32_t want = 0;
    // everything is about to be drained: the first frame after this goes to a twin's slot, i.e. out at once and alone (an idle GPU
    // should not wait for a partner frame), the pairs start with the frame after it
    if (ctx->frame_batch == 2) ctx->rot &= ~1;
    // The control blocks of the lanes with asynchronous frames follow the frames' kernels on the lanes' own streams, ALL of them before
    // the first stream is waited for: six blocking copies one after the other (three lanes and their twins, 20-30 us each) were the
    // last 150 us of every gs_sync() -- a tenth of a region of twenty frames (tools/prof_lanes.py).
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (L) TRY(lane_rc(ctx, L, lane_drain(L, true)));        // (every launch of every lane is in its stream)
    }
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (L && L->async_pending) TRY(lane_rc(ctx, L, lane_read_control(L, false)));
    }
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = ctx->lanes[i];
        if (!L) continue;
        GS_HIP(hipStreamSynchronize(L->stream));
        TRY(lane_rc(ctx, L, prof_drain(L)));
        if (!L->async_pending) continue;
        L->async_pending = false;
        const bool missed = L->ctl_host->round1_missed != 0;
        static const bool dbg_near = getenv("GS_DEBUG_NEAR") != nullptr;       // (what raised the share: printed per collected lane)
        if (dbg_near && (L->ctl_host->round1_missed || L->ctl_host->unsat_events != L->share_lane.seen_unsat_events)) {
            const GsControl *c = L->ctl_host;
            fprintf(stderr, "[gs] sync lane %d: order_incomplete %u spec_fail %u (T %u chunk limit %u) near_overflow %u missed %u unsat_events %u (seen %u) V %u P %u V' %u near_sorted %u req %u frames %u two_rounds %d near_frac %.4f clean %u hold %u\n", i, c->order_incomplete, c->spec_fail, c->spec_dbg >> 16, c->spec_dbg & 0xFFFFu, c->near_overflow, c->round1_missed,
                    c->unsat_events, L->share_lane.seen_unsat_events, c->n_kept, c->n_sorted, c->n_valid, c->near_sorted, L->sort_near_req, c->acc_frames, (int)L->share_lane.last_two_rounds,
                    ctx->share.near_frac, ctx->share.clean_frames, ctx->share.skip_hold);
        }
        if (missed) GS_HIP(hipMemsetAsync(&L->ctl->round1_missed, 0, sizeof(uint32_t), L->stream));
        if (L->ctl_host->order_incomplete) GS_HIP(hipMemsetAsync(&L->ctl->order_incomplete, 0, sizeof(uint32_t), L->stream));
        bool over = false;
        TRY(collect_status(L, &over, tally, &spec_failed));
        any_missed |= missed; any_over |= over;
        if (missed || over) bad_unit[i % GS_MAX_PRIMARY] = true;
        if (over && L->ctl_host->max_total > want) want = L->ctl_host->max_total;
    }
    decide_share(ctx, frac_used, tally, false);                  // (once, whatever the number of lanes that saw a failure)
    if (spec_failed) gs_spec_back_off(ctx, spec_failed == 2u);
    if (any_over)                                                // one retry for all lanes: each gets room for the largest demand seen
        for (int i = 0; i < GS_MAX_LANES; i++)
            if (ctx->lanes[i] && ctx->lanes[i]->pair_cap)
                TRY(lane_rc(ctx, ctx->lanes[i], gs_ensure_pair_capacity(ctx->lanes[i], (size_t)want + want / 4 + 1)));
    const bool stale = ctx->log_stale;
    ctx->log_stale = false;
    int rc = GS_OK;
    if (any_missed || any_over) {
        rc = (ctx->auto_retry && !stale) ? redraw_flagged_frames(ctx, bad_unit) : GS_E_RETRY;
        if (rc == GS_E_RETRY) {
            if (any_missed) snprintf(ctx->err, sizeof ctx->err, "an asynchronous frame skipped its second binning round but a tile had not saturated; "
                                     "the share of splats binned first was raised - render the frames since the previous gs_sync() again");
            else snprintf(ctx->err, sizeof ctx->err, "an asynchronous frame needed %u pairs and overflowed the pair buffers; they were enlarged - "
                          "render the frames since the previous gs_sync() again", want);
        }
    }
    return rc;                                                       // (log_guard resets the logs)
}

GS_API int gs_set_stream(gs_ctx *ctx, void *hip_stream)
{
    CHECK_CTX(ctx);
    GS_HIP(hipSetDevice(ctx->device));
    TRY(drain_all(ctx));
    if (ctx->own_stream) { (void)hipStreamDestroy(ctx->stream); ctx->own_stream = false; }
    if (hip_stream) ctx->stream = (hipStream_t)hip_stream;
    else { GS_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
    // on a caller-owned stream every frame is ordered with the caller's own work on it: no lane rotation
    ctx->user_stream = hip_stream != nullptr;
    set_current_lane(ctx, 0, 0);
    return GS_OK;
}

GS_API int gs_wait_stream(gs_ctx *ctx, void *hip_stream)
{
    CHECK_CTX(ctx);
    GS_HIP(hipSetDevice(ctx->device));
    gs_ctx *L = nullptr;
    TRY(get_lane(ctx, next_frame_lane(ctx), &L));               // the lane the next gs_sort() will use
    GS_HIP(hipEventRecord(L->ev_gate, (hipStream_t)hip_stream));
    GS_HIP(hipStreamWaitEvent(L->stream, L->ev_gate, 0));
    return GS_OK;
}

GS_API int gs_frame_lane(gs_ctx *ctx) { return ctx ? ctx->cur : -1; }

GS_API void *gs_lane_stream(gs_ctx *ctx, int lane)
{
    if (!ctx || lane < 0 || lane >= GS_MAX_LANES || !ctx->lanes[lane]) return nullptr;
    (void)lane_drain(ctx->lanes[lane]);                          // everything handed to the lane so far is in its stream
    return (void *)ctx->lanes[lane]->stream;
}

GS_API int gs_stream_wait_frame(gs_ctx *ctx, void *hip_stream)
{
    CHECK_CTX(ctx);
    GS_HIP(hipSetDevice(ctx->device));
    gs_ctx *L = ctx->lanes[ctx->cur];
    TRY(lane_rc(ctx, L, lane_drain(L)));
    GS_HIP(hipEventRecord(L->ev_frame, L->stream));
    GS_HIP(hipStreamWaitEvent((hipStream_t)hip_stream, L->ev_frame, 0));
    return GS_OK;
}

GS_API int gs_frame_status_device(gs_ctx *ctx, void **device_word)
{
    CHECK_CTX(ctx);
    if (!device_word) FAIL(GS_E_BADARG, "gs_frame_status_device: device_word is NULL");
    gs_ctx *L = ctx->lanes[ctx->cur];
    TRY(lane_rc(ctx, L, lane_drain(L)));                         // (the frame's kernels are in the stream: the word is theirs from here on)
    // (the word the frame's last render was given; on the root of a gathered frame: where k_assemble ORs the pieces' words)
    *device_word = (L->status_cur && L->status_cur >= L->ctl->status_ring && L->status_cur < L->ctl->status_ring + GS_STATUS_RING) ? (void *)L->status_cur
                                                                                                                          : (void *)&L->ctl->frame_status;
    return GS_OK;
}

GS_API void *gs_frame_stream(gs_ctx *ctx)
{
    if (!ctx) return nullptr;
    (void)lane_drain(ctx->lanes[ctx->cur]);                      // the frame's kernels are in the stream when this returns
    return (void *)ctx->lanes[ctx->cur]->stream;
}

}  // extern "C"

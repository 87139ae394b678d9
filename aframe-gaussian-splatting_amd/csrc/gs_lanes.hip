// gs_lanes.hip -- the lanes frames are pipelined over: their creation, their scratch and profiling rings, the owner state they
// alias, and the enqueue threads that do their launching (with the queue classifier that pairs frames).
#include <stdlib.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include "gs_lanes.h"

static void lane_stop_worker(gs_ctx *L);

static int ensure_radix_tables(gs_ctx *ctx, size_t items)
{
    // a histogram row per radix chunk (sized for the short geometry's chunks) + the digit totals
    const size_t need_hist = (size_t)GS_RADIX_MAX_BINS * (gs_div_up(items, GS_CHUNK_S) + 16);
    if (need_hist > ctx->hist_cap) { dev_free(ctx->hist); ctx->hist_cap = 0; TRY(dev_alloc(ctx, &ctx->hist, need_hist)); ctx->hist_cap = need_hist; }
    // the MSD depth sort's group rows: 256 words per GS_MSD_GROUP chunks (of the short geometry), for at most GS_MSD_MAX_N splats
    const size_t msd_items = items < GS_MSD_MAX_N ? items : (size_t)GS_MSD_MAX_N;
    const size_t need_grp = (size_t)256 * (gs_div_up(gs_div_up(msd_items, GS_CHUNK_S), GS_MSD_GROUP) + 2);
    // (+ k_seg_sort's work items behind them: 4 words of header and 4 per item, at most 256 segments + one block per 4096 records)
    const size_t need_tab = 4 + 4 * ((size_t)512 + 256 + msd_items / 4096 + 16);   // (room for GS_SEG_GRID items at least: every workgroup reads ITS first item unconditionally)
    if (need_grp > ctx->msd_grp_cap) {
        dev_free(ctx->msd_grp); ctx->msd_grp_cap = 0; ctx->msd_tab = nullptr;
        TRY(dev_alloc(ctx, &ctx->msd_grp, need_grp + need_tab));
        ctx->msd_grp_cap = need_grp; ctx->msd_tab = ctx->msd_grp + need_grp;
    }
    const size_t need_aux = (size_t)GS_RADIX_MAX_BINS * 2;
    if (need_aux > ctx->aux_cap) { dev_free(ctx->radix_aux); TRY(dev_alloc(ctx, &ctx->radix_aux, need_aux)); ctx->aux_cap = need_aux; }
    return GS_OK;
}

static int ensure_scan_scratch(gs_ctx *ctx)
{
    TRY(ensure_radix_tables(ctx, ctx->scratch_cap > ctx->pair_cap ? ctx->scratch_cap : ctx->pair_cap));   // the larger of the two sorts
    const size_t need_spine = gs_div_up(ctx->scratch_cap, GS_BLOCK) + 16;   // project/emit chunks of 256 splats
    if (need_spine > ctx->spine_cap) {
        dev_free(ctx->spine); ctx->spine_cap = 0;
        TRY(dev_alloc(ctx, &ctx->spine, need_spine)); ctx->spine_cap = need_spine;
    }
    return GS_OK;
}

int gs_ensure_radix_scratch(gs_ctx *ctx, size_t items) { return ensure_radix_tables(ctx, items); }

int gs_ensure_pair_capacity(gs_ctx *ctx, size_t pairs)
{
    if (pairs <= ctx->pair_cap) return GS_OK;
    size_t cap = ctx->pair_cap ? ctx->pair_cap : (size_t)1 << 22;
    while (cap < pairs) cap += cap / 2 + 1;
    cap = (cap + GS_CHUNK_L - 1) / GS_CHUNK_L * GS_CHUNK_L;
    if (cap > 0xFFFF0000ull) FAIL(GS_E_OOM, "pair list of %zu entries exceeds the 32-bit index space", pairs);
    dev_free(ctx->pair_a); dev_free(ctx->pair_b); dev_free(ctx->emit_extra);
    ctx->pair_cap = 0;
    TRY(dev_alloc(ctx, &ctx->pair_a, cap)); TRY(dev_alloc(ctx, &ctx->pair_b, cap));
    TRY(dev_alloc(ctx, &ctx->emit_extra, cap / GS_EMIT_PAIRS + 2));
    ctx->pair_cap = cap;
    return ensure_scan_scratch(ctx);
}

// every lane idle (the resident arrays are about to change, or the caller wants the device quiet)
int gs_ctl::drain_all(gs_ctx *ctx)
{
    gs_ctx *P = gs_root(ctx);
    int first = GS_OK;
    // what follows may change what the frames in the logs were drawn from (more splats, another scene image, other options):
    // gs_sync() will not draw such frames again by itself
    for (int i = 0; i < GS_MAX_LANES; i++)
        if (P->lanes[i] && P->lanes[i]->log) for (const GsFrameRec &r : P->lanes[i]->log->recs) if (r.nrender) P->log_stale = true;
    for (int i = 0; i < GS_MAX_LANES; i++) {
        gs_ctx *L = P->lanes[i];
        if (!L) continue;
        const int rc = lane_drain(L, true);                        // a worker's failure surfaces at the next gs_sync()
        if (rc != GS_OK && first == GS_OK) { first = rc; if (L != ctx) memcpy(ctx->err, L->err, sizeof ctx->err); }
        if (L->stream) GS_HIP(hipStreamSynchronize(L->stream));
    }
    return first;
}

// per-frame scratch of one lane (sort keys, projected records, pair lists, scan tables) for `cap` splats
static int ensure_lane_scratch(gs_ctx *ctx, size_t cap)
{
    if (cap <= ctx->scratch_cap) return GS_OK;
    GS_HIP(hipStreamSynchronize(ctx->stream));
    dev_free(ctx->depth); dev_free(ctx->key_a); dev_free(ctx->kv_b); dev_free(ctx->val_a);
    dev_free(ctx->proj); dev_free(ctx->rect); dev_free(ctx->tile_count); dev_free(ctx->zwin);
    ctx->scratch_cap = 0; ctx->have_sort = false; ctx->sorted = nullptr;
    TRY(dev_alloc(ctx, &ctx->depth, cap));
    TRY(dev_alloc(ctx, &ctx->key_a, cap)); TRY(dev_alloc(ctx, &ctx->kv_b, cap)); TRY(dev_alloc(ctx, &ctx->val_a, cap));
    TRY(dev_alloc(ctx, &ctx->proj, cap)); TRY(dev_alloc(ctx, &ctx->rect, cap));
    TRY(dev_alloc(ctx, &ctx->tile_count, cap)); TRY(dev_alloc(ctx, &ctx->zwin, cap));
    ctx->scratch_cap = cap;
    TRY(gs_ensure_pair_capacity(ctx, cap * 8 > ((size_t)1 << 22) ? cap * 8 : (size_t)1 << 22));
    return ensure_scan_scratch(ctx);
}

// the state store's allocation (owner): ctx->cap zero-filled bytes at least, the first edit_n of them kept
int gs_ctl::edit_ensure_alloc(gs_ctx *ctx)
{
    const size_t want = ctx->cap ? ctx->cap : (size_t)1 << 16;
    if (ctx->edit_state && ctx->edit_cap >= want) return GS_OK;
    uint8_t *nw = nullptr;
    TRY(dev_alloc(ctx, &nw, want));
    hipError_t e = hipMemset(nw, 0, want);
    if (e == hipSuccess && ctx->edit_state && ctx->edit_n) e = hipMemcpy(nw, ctx->edit_state, ctx->edit_n, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { dev_free(nw); FAIL(GS_E_HIP, "growing the state store failed: %s", hipGetErrorString(e)); }
    dev_free(ctx->edit_state);
    ctx->edit_state = nw; ctx->edit_cap = want;
    return GS_OK;
}

// grow the resident per-splat arrays (owner only) to hold at least `want` splats, preserving the data
int gs_ctl::ensure_capacity(gs_ctx *ctx, size_t want)
{
    if (want <= ctx->cap) return GS_OK;
    if (want > 0x7FFFFFF0ull) FAIL(GS_E_BADARG, "more than 2^31 splats");
    size_t cap = ctx->cap ? ctx->cap : (size_t)1 << 16;
    while (cap < want) cap *= 2;
    TRY(drain_all(ctx));
    float4 *sr = nullptr; uint4 *sp = nullptr; float *br = nullptr;
    TRY(dev_alloc(ctx, &sp, cap * 2)); TRY(dev_alloc(ctx, &sr, cap)); TRY(dev_alloc(ctx, &br, cap));
    if (ctx->n) {
        GS_HIP(hipMemcpyAsync(sp, ctx->splat, ctx->n * 2 * sizeof(uint4), hipMemcpyDeviceToDevice, ctx->stream));
        GS_HIP(hipMemcpyAsync(sr, ctx->sort_rows, ctx->n * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
        GS_HIP(hipMemcpyAsync(br, ctx->bound_r, ctx->n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        GS_HIP(hipStreamSynchronize(ctx->stream));
    }
    dev_free(ctx->splat); dev_free(ctx->sort_rows); dev_free(ctx->bound_r);
    ctx->splat = sp; ctx->sort_rows = sr; ctx->bound_r = br;
    ctx->cap = cap;
    if (ctx->edit_state) TRY(edit_ensure_alloc(ctx));           // the state store's allocation follows the resident capacity
    for (int i = 0; i < GS_MAX_LANES; i++) if (ctx->lanes[i]) { ctx->lanes[i]->have_sort = false; ctx->lanes[i]->sorted = nullptr; }
    return ensure_lane_scratch(ctx, cap);                       // lane 0 now; the other lanes when they are next used
}


// ---------------------------------------------------------------- profiling ring (HIP events on the context's stream)

hipEvent_t gs_prof_event(gs_ctx *ctx, int k)
{
    if (!ctx->profile || !ctx->ring) return nullptr;
    if (ctx->profile_blend_only && k != 4 && k != 5) return nullptr;   // GS_OPT_PROFILE = 2 / 3: only the events around the blend
    if (ctx->profile_every > 1 && (ctx->profile_tick % ctx->profile_every) != 0) return nullptr;   // ... of every 4th frame
    const uint32_t slot = ctx->ring_head % GS_PROF_RING;
    ctx->ring_flags[slot] |= (uint8_t)(1u << k);
    return ctx->ring[slot * GS_PROF_EVENTS + k];
}

// fold the timings of every pending slot into the stats; the stream must be idle
int gs_ctl::prof_drain(gs_ctx *ctx)
{
    for (; ctx->ring_pending; ctx->ring_pending--) {
        const uint32_t slot = (ctx->ring_head - ctx->ring_pending) % GS_PROF_RING;
        hipEvent_t *e = ctx->ring + slot * GS_PROF_EVENTS;
        const uint8_t f = ctx->ring_flags[slot];
        ctx->ring_flags[slot] = 0;
        float ms;
        if ((f & 3) == 3) { GS_HIP(hipEventElapsedTime(&ms, e[0], e[1])); ctx->stats.ms_sort = ms; ctx->stats.sum_ms_sort += ms; }
        if ((f & 0x7C) == 0x30) {                            // blend-only profiling
            float d;
            GS_HIP(hipEventElapsedTime(&d, e[4], e[5]));
            ctx->stats.ms_blend = d; ctx->stats.sum_ms_blend += d;
            ctx->stats.prof_frames++;
        }
        if ((f & 0x7C) == 0x7C) {
            float a, b, d, r1;
            GS_HIP(hipEventElapsedTime(&a, e[2], e[3])); GS_HIP(hipEventElapsedTime(&b, e[3], e[4])); GS_HIP(hipEventElapsedTime(&d, e[4], e[5]));
            GS_HIP(hipEventElapsedTime(&r1, e[5], e[6]));
            b += r1;                                       // round 1 (binning against the unsaturated tiles + their blend)
            ctx->stats.ms_project = a; ctx->stats.ms_bin = b; ctx->stats.ms_blend = d; ctx->stats.ms_render = a + b + d;
            ctx->stats.sum_ms_project += a; ctx->stats.sum_ms_bin += b; ctx->stats.sum_ms_blend += d;
            ctx->stats.prof_frames++;
        }
    }
    return GS_OK;
}

// a frame has been enqueued: move to the next slot (draining first if the ring is full)
int gs_ctl::prof_advance(gs_ctx *ctx)
{
    if (!ctx->profile || !ctx->ring) return GS_OK;
    ctx->profile_tick++;
    ctx->ring_head++; ctx->ring_pending++;
    if (ctx->ring_pending >= GS_PROF_RING - 1) {
        GS_HIP(hipStreamSynchronize(ctx->stream));
        return prof_drain(ctx);
    }
    return GS_OK;
}

// ---------------------------------------------------------------- enqueue threads
// Enqueuing one frame costs the host ~100 us (18 kernel launches), about what the GPU needs for a frame once three of
// them overlap -- so each lane gets a worker thread that does the launching: gs_sort() / gs_render_device(ASYNC) only
// hand it the frame's uniforms, and the launches of the frames in flight proceed in parallel on the lanes' own streams.
// Everything a worker touches is lane-local; the caller's thread touches a lane only after lane_drain().

struct GsLaneWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv_work, cv_idle;
    std::deque<GsLaneCmd> q;
    bool busy = false, stop = false;
    bool flush = false;                                        // a drain is waiting: do not hold a frame back for a partner
    uint64_t n_pairs = 0, n_single = 0;                        // frames sent out in pairs / alone (GS_DEBUG_PAIRS=1 prints them at shutdown)
    int rc = GS_OK;                                            // first failure since the last drain ...
    char err[GS_ERRLEN] = "";                                  // ... and its message: the worker never writes the lane's err itself
};

// the renders r0 (lane A) and r1 (lane B: A's twin) behind their sort(s), as ONE chain of launches on A's stream; a frame wanted on
// the host follows its kernels there (two views of one frame never are: classify_queue)
static int run_render_pair(gs_ctx *A, gs_ctx *B, const GsLaneCmd &r0, const GsLaneCmd &r1)
{
    gs_ctx *ctx = A;
    gs_ctx *S[2] = { A, B };
    const GsFrameUniforms U[2] = { r0.u, r1.u };
    uint8_t *dev[2] = { (uint8_t *)r0.device_rgba, (uint8_t *)r1.device_rgba };
    TRY(ensure_frame_buffers(A, U[0], dev[0] == nullptr));
    TRY(ensure_frame_buffers(B, U[1], dev[1] == nullptr));
    TRY(gs_run_render2(S, U, dev));
    const GsLaneCmd *r[2] = { &r0, &r1 };
    for (int k = 0; k < 2; k++) {
        if (!r[k]->host_rgba) continue;
        const size_t sw = (size_t)(U[k].x1 - U[k].x0);
        const uint8_t *src = dev[k] ? dev[k] : S[k]->fb;
        GS_HIP(hipMemcpy2DAsync(r[k]->host_rgba, r[k]->stride ? r[k]->stride : sw * 4, src, sw * 4, sw * 4, (size_t)U[k].H, hipMemcpyDeviceToHost, A->stream));
    }
    return prof_advance(A);                                     // (the pair's HIP events sit in the primary lane's ring)
}

// GS_OPT_FRAME_BATCH: the frames of a lane and of its twin, when both are waiting, go out as ONE chain of launches
static int run_frame_pair(gs_ctx *A, gs_ctx *B, const GsLaneCmd &s0, const GsLaneCmd &r0, const GsLaneCmd &s1, const GsLaneCmd &r1)
{
    gs_ctx *S[2] = { A, B };
    const float *view[2] = { s0.view, s1.view };
    const float *cut[2] = { s0.has_cutout ? s0.cutout : nullptr, s1.has_cutout ? s1.cutout : nullptr };
    const GsSortStrip *strip[2] = { s0.has_strip ? &s0.strip : nullptr, s1.has_strip ? &s1.strip : nullptr };
    const uint32_t near[2] = { sort_covers(s0.near_req, r0.u) ? s0.near_req : 0u, sort_covers(s1.near_req, r1.u) ? s1.near_req : 0u };
    TRY(gs_run_sort2(S, view, cut, strip, near));
    return run_render_pair(A, B, r0, r1);
}

// What follows the sort `s0` that was just popped (a frame on the primary lane L) in the queue?
//   GS_Q_PAIR    its render [+ its gather call] and the twin's sort, render [+ gather call], of a kind that may share launches
//                (n_take commands to pop; calls = 1: gathered frames of one piece each, the gathers issued after the shared
//                kernels in frame order);
//   GS_Q_STEREO  the renders of TWO views of this frame (both XR eyes drawn by this context), which may share launches;
//   GS_Q_SINGLE  enough to know that neither will form;  GS_Q_WAIT  not enough yet.
enum { GS_Q_WAIT, GS_Q_PAIR, GS_Q_STEREO, GS_Q_SINGLE };
static int classify_queue(const gs_ctx *L, const GsLaneCmd &s0, const std::deque<GsLaneCmd> &q, int *n_take, int *calls)
{
    const gs_ctx *T = L->twin;
    if (q.empty()) return GS_Q_WAIT;
    if (q[0].type != GS_CMD_RENDER || q[0].target != L) return GS_Q_SINGLE;
    if (q.size() < 2) return GS_Q_WAIT;
    if (q[1].type == GS_CMD_RENDER) {                                          // a second view of the same frame
        // (neither view wanted on the host: run_render_pair issues a host copy for a render that has one, and two views must not)
        const bool ok = q[1].target == L && !s0.has_strip && !q[0].host_rgba && !q[1].host_rgba && gs_frames_batchable(q[0].u, q[1].u) && L->n == T->n;
        return ok ? GS_Q_STEREO : GS_Q_SINGLE;
    }
    const int c = (q[1].type == GS_CMD_CALL && q[1].target == L) ? 1 : 0;
    const size_t need = 3 + 2 * (size_t)c;
    if (q.size() < (size_t)(2 + c)) return GS_Q_WAIT;
    const GsLaneCmd &s1 = q[1 + c];
    if (s1.type != GS_CMD_SORT || s1.target != T || s1.has_strip != s0.has_strip) return GS_Q_SINGLE;
    if (q.size() < (size_t)(3 + c)) return GS_Q_WAIT;
    const GsLaneCmd &r1 = q[2 + c];
    if (r1.type != GS_CMD_RENDER || r1.target != T || !gs_frames_batchable(q[0].u, r1.u) || L->n != T->n) return GS_Q_SINGLE;
    if (c) {
        if (q.size() < need) return GS_Q_WAIT;
        if (q[3 + c].type != GS_CMD_CALL || q[3 + c].target != T) return GS_Q_SINGLE;
    }
    *n_take = (int)need; *calls = c;
    return GS_Q_PAIR;
}

// one sort, then the two views in ONE chain of launches: the second view on the twin's scratch, from the lane's order
static int run_two_views(gs_ctx *A, gs_ctx *B, const GsLaneCmd &s0, const GsLaneCmd &r0, const GsLaneCmd &r1)
{
    gs_ctx *ctx = A;
    const uint32_t near = (sort_covers(s0.near_req, r0.u) && sort_covers(s0.near_req, r1.u)) ? s0.near_req : 0u;
    TRY(gs_run_sort(A, s0.view, s0.has_cutout ? s0.cutout : nullptr, nullptr, near));
    // the twin's kernels read the order and its length through THEIR lane: point it at the lane's (counts: the head of the control block)
    GS_HIP(hipMemcpyAsync(B->ctl, A->ctl, offsetof(GsControl, n_visible), hipMemcpyDeviceToDevice, A->stream));
    B->sorted = A->sorted; B->have_sort = true; B->sort_near_req = 0;   // (nothing of its own to sort again: the pair was checked above)
    return run_render_pair(A, B, r0, r1);
}

static void lane_worker_main(gs_ctx *L)
{
    GsLaneWorker *w = L->worker;
    (void)hipSetDevice(L->device);
    char scratch[GS_ERRLEN] = "";
    gs_tl_err = scratch;                                       // GS_HIP / FAIL on this thread write here
    std::unique_lock<std::mutex> lk(w->m);
    for (;;) {
        w->cv_work.wait(lk, [&] { return w->stop || !w->q.empty(); });
        if (w->q.empty()) break;                               // stop requested and nothing left to do
        GsLaneCmd c = w->q.front(); w->q.pop_front();
        w->busy = true;
        int rc = GS_OK;
        gs_ctx *T = c.target;
        bool paired = false, stereo = false;
        int n_take = 0, calls = 0;
        GsLaneCmd pc[5];                                           // the rest of a pair: render 0 [call 0] sort 1 render 1 [call 1]
        if (c.type == GS_CMD_SORT && T == L && L->twin && gs_root(L)->frame_batch == 2 && w->rc == GS_OK) {
            // the sort of a frame on the primary lane: if its render and the twin's frame are queued behind it (the caller is
            // normally several frames ahead of this thread; give it a moment if not), the two frames share their launches
            int kind = GS_Q_WAIT;
            w->cv_work.wait_for(lk, std::chrono::microseconds(200), [&] { kind = classify_queue(L, c, w->q, &n_take, &calls); return w->stop || w->flush || kind != GS_Q_WAIT; });
            if (kind == GS_Q_PAIR) {
                for (int k = 0; k < n_take; k++) { pc[k] = w->q.front(); w->q.pop_front(); }
                paired = true;
            } else if (kind == GS_Q_STEREO) {
                pc[0] = w->q.front(); w->q.pop_front(); pc[1] = w->q.front(); w->q.pop_front();
                stereo = true;
                L->twin->inflight++;                               // the second view runs on the twin's scratch: a drain of the twin waits for it
            }
        }
        // (w->rc is the caller's to reset under the mutex -- lane_drain of the lane OR of its twin, which shares this thread -- so the
        // launches below decide on a copy taken while the mutex is still held: ThreadSanitizer, round 4)
        const int prior_rc = w->rc;
        lk.unlock();
        static const bool dbg_slow = getenv("GS_DEBUG_WORKER") != nullptr;   // (diagnostic: commands that kept this thread longer than 60 us)
        const auto dbg_t0 = std::chrono::steady_clock::now();
        // (a call is run even after a failure: the gather of a frame must be issued on every rank, or the others wait for it)
        if (stereo) rc = run_two_views(L, L->twin, c, pc[0], pc[1]);
        else if (paired) {
            rc = run_frame_pair(L, L->twin, c, pc[0], pc[1 + calls], pc[2 + calls]);
            if (calls) {                                           // the two gathers, in frame order, behind the shared kernels
                const int g0 = pc[1].call(L), g1 = pc[4].call(L->twin);
                if (rc == GS_OK) rc = g0 != GS_OK ? g0 : g1;
            }
        }
        else if (c.type == GS_CMD_CALL) { const int r2 = c.call(T); if (prior_rc == GS_OK) rc = r2; }
        else if (prior_rc == GS_OK) rc = c.type == GS_CMD_SORT ? gs_run_sort(T, c.view, c.has_cutout ? c.cutout : nullptr, c.has_strip ? &c.strip : nullptr, c.near_req)
                                                  : render_async_on_lane(T, c.u, c.device_rgba, c.host_rgba, c.stride);
        if (dbg_slow) {
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - dbg_t0).count();
            if (us > (getenv("GS_DEBUG_WORKER_US") ? atof(getenv("GS_DEBUG_WORKER_US")) : 60.0)) fprintf(stderr, "[gs] worker %p: %s for lane %p took %.0f us\n", (void *)L, stereo ? "two views" : paired ? "a pair" : c.type == GS_CMD_SORT ? "a sort" : c.type == GS_CMD_RENDER ? "a render" : "a call", (void *)T, us);
        }
        lk.lock();
        if (rc != GS_OK && w->rc == GS_OK) { w->rc = rc; memcpy(w->err, scratch, sizeof w->err); }
        w->busy = false;
        if (w->q.empty()) w->flush = false;
        if (stereo) { L->inflight -= 3; L->twin->inflight--; w->n_pairs += 2; L->twin->async_pending = true; }   // (the second view's counters sit in the twin's control block)
        else if (paired) { L->inflight -= 2 + calls; L->twin->inflight -= 2 + calls; w->n_pairs += 2; } else { T->inflight -= 1; if (c.type == GS_CMD_RENDER) w->n_single++; }
        w->cv_idle.notify_all();
    }
}

// wait until the lane's worker has enqueued everything it was given; returns (and clears) its first failure
int gs_ctl::lane_drain(gs_ctx *L, bool flush)
{
    GsLaneWorker *w = L->exec ? L->exec->worker : L->worker;
    if (!w) return GS_OK;
    std::unique_lock<std::mutex> lk(w->m);
    if (flush && L->inflight) { w->flush = true; w->cv_work.notify_all(); }   // (gs_sync / drain_all: a frame waiting for its partner goes out now)
    // everything handed over FOR THIS LANE has been executed (its twin's commands may still be queued: the two only share the thread)
    w->cv_idle.wait(lk, [&] { return L->inflight == 0; });
    const int rc = w->rc; w->rc = GS_OK;
    if (rc != GS_OK) memcpy(L->err, w->err, sizeof L->err);    // on the caller's thread, under the worker's mutex
    return rc;
}

static int ensure_worker(gs_ctx *L)
{
    gs_ctx *E = L->exec ? L->exec : L;
    if (!E->worker) {
        E->worker = new (std::nothrow) GsLaneWorker();
        if (!E->worker) return GS_E_OOM;
        try { E->worker->th = std::thread(lane_worker_main, E); }
        catch (...) {                                              // no exception crosses the C ABI
            delete E->worker; E->worker = nullptr;
            snprintf(L->err, sizeof L->err, "could not start the lane's enqueue thread");
            return GS_E_OOM;
        }
    }
    return GS_OK;
}

int gs_ctl::lane_push(gs_ctx *L, GsLaneCmd c)
{
    gs_ctx *E = L->exec ? L->exec : L;
    if (ensure_worker(L) != GS_OK) return GS_E_OOM;
    GsLaneWorker *w = E->worker;
    c.target = L;
    { std::lock_guard<std::mutex> lk(w->m); w->q.push_back(c); L->inflight++; }
    w->cv_work.notify_all();
    return GS_OK;
}

static void lane_stop_worker(gs_ctx *L)
{
    GsLaneWorker *w = L->worker;
    if (!w) return;
    { std::lock_guard<std::mutex> lk(w->m); w->stop = true; }
    w->cv_work.notify_one();
    if (w->th.joinable()) w->th.join();
    if (getenv("GS_DEBUG_PAIRS")) fprintf(stderr, "[gs] lane %p: %llu frames in pairs, %llu alone\n", (void *)L, (unsigned long long)w->n_pairs, (unsigned long long)w->n_single);
    delete w;
    L->worker = nullptr;
}

// ---------------------------------------------------------------- lanes (frame pipelining)

// The first dispatch of a hardware queue that asks for PRIVATE (scratch) memory -- or for more of it per lane than the queue has had
// so far -- stops at the command processor until the runtime has allocated it: ~140 us, once per queue.  A few kernels here ask
// for some (k_project<0, true>: 36 bytes of spill slots the compiler keeps although every SGPR spill went to VGPR lanes; the paired
// k_seg_sort: 12), and which of the lanes' queues has met one of them before a caller starts timing is a matter of which frames
// went out alone and which in pairs: round 5's twenty-frame region lost 80 us to one such stop on a queue the pre-roll had only
// fed pairs (tools/prof_api.py: the launch call returned, the kernel started 140 us later).  So every lane's stream asks for more
// than any kernel will, once, when the lane is made.
__global__ void k_touch_private(uint32_t *out, uint32_t n)
{
    volatile uint32_t a[GS_TOUCH_PRIVATE_WORDS];                  // (volatile + a run-time index: stays in private memory)
    for (uint32_t i = 0; i < GS_TOUCH_PRIVATE_WORDS; i++) a[i] = i * n;
    out[0] = a[n % GS_TOUCH_PRIVATE_WORDS];
}

// stream, control block, per-workgroup partial slots, pinned mirror: what every lane owns besides its scratch
hipError_t gs_ctl::init_frame_resources(gs_ctx *c, gs_ctx *primary)
{
    hipError_t e;
#define IFR(call) do { e = (call); if (e != hipSuccess) return e; } while (0)
    if (primary) { c->stream = primary->stream; c->own_stream = false; c->exec = primary; }   // a twin: frames on its primary's stream and thread
    else { IFR(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; c->exec = c; }
    IFR(hipMalloc((void **)&c->ctl, sizeof(GsControl)));
    IFR(hipMemset(c->ctl, 0, sizeof(GsControl)));
    IFR(hipMalloc((void **)&c->part_min, GS_MAX_PART * sizeof(unsigned long long)));
    IFR(hipMalloc((void **)&c->part_max, GS_MAX_PART * sizeof(unsigned long long)));
    IFR(hipMalloc((void **)&c->part_cnt, GS_MAX_PART * sizeof(uint32_t)));
    IFR(hipMalloc((void **)&c->part_valid, GS_MAX_PART * sizeof(uint32_t)));
    IFR(hipMalloc((void **)&c->part_vis, GS_MAX_PART * sizeof(uint32_t)));
    for (int k = 0; k < 2; k++) { IFR(hipMalloc((void **)&c->dhist[k], GS_DH_WORDS * sizeof(uint32_t))); IFR(hipMemset(c->dhist[k], 0, GS_DH_WORDS * sizeof(uint32_t))); }
    c->dh_next = 0; c->dh_dirty = nullptr;
    c->sort_near_req = 0;
    IFR(hipHostMalloc((void **)&c->ctl_host, sizeof(GsControl), hipHostMallocDefault));
    memset(c->ctl_host, 0, sizeof(GsControl));
    IFR(hipEventCreateWithFlags(&c->ev_frame, hipEventDisableTiming | hipEventReleaseToDevice));
    IFR(hipEventCreateWithFlags(&c->ev_gate, hipEventDisableTiming | hipEventReleaseToDevice));
    // (the queue's private memory: above.  One launch: 32 .. 512 of them -- a deeper warm-up of the new queue -- changed nothing)
    if (!primary) { k_touch_private<<<1, 64, 0, c->stream>>>(c->part_cnt, 1u); IFR(hipGetLastError()); }
#undef IFR
    return hipSuccess;
}

void gs_ctl::free_frame_resources(gs_ctx *c)
{
    if (c->exec == c || !c->exec) lane_stop_worker(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c->log; c->log = nullptr;
    dev_free(c->depth); dev_free(c->key_a); dev_free(c->kv_b); dev_free(c->val_a);
    dev_free(c->hist); dev_free(c->radix_aux); dev_free(c->msd_grp); dev_free(c->spine);
    dev_free(c->proj); dev_free(c->rect); dev_free(c->tile_count); dev_free(c->zwin);
    dev_free(c->pair_a); dev_free(c->pair_b); dev_free(c->emit_extra); dev_free(c->row_cnt); dev_free(c->row_tot); dev_free(c->seg_diff);
    gs_comm_free_lane(c);
    dev_free(c->tile_range); dev_free(c->fb); dev_free(c->ctl); dev_free(c->state); dev_free(c->unsat_mask); dev_free(c->surf_buf);
    dev_free(c->part_min); dev_free(c->part_max); dev_free(c->part_cnt); dev_free(c->part_valid); dev_free(c->part_vis); dev_free(c->dhist[0]); dev_free(c->dhist[1]);
    if (c->ctl_host) { (void)hipHostFree(c->ctl_host); c->ctl_host = nullptr; }
    if (c->ring) { for (int i = 0; i < GS_PROF_RING * GS_PROF_EVENTS; i++) if (c->ring[i]) (void)hipEventDestroy(c->ring[i]); free(c->ring); c->ring = nullptr; }
    free(c->ring_flags); c->ring_flags = nullptr;
    if (c->ev_frame) (void)hipEventDestroy(c->ev_frame);
    if (c->ev_gate) (void)hipEventDestroy(c->ev_gate);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = nullptr;
}

// switch the HIP-event profiling of one lane on/off (allocates its ring on first use, restarts its accumulators)
int gs_ctl::set_profile(gs_ctx *ctx, bool on, bool blend_only, uint32_t every)
{
    TRY(lane_drain(ctx));
    GS_HIP(hipStreamSynchronize(ctx->stream));
    TRY(prof_drain(ctx));
    if (on && !ctx->ring) {
        ctx->ring = (hipEvent_t *)calloc(GS_PROF_RING * GS_PROF_EVENTS, sizeof(hipEvent_t));
        ctx->ring_flags = (uint8_t *)calloc(GS_PROF_RING, 1);
        if (!ctx->ring || !ctx->ring_flags) FAIL(GS_E_OOM, "out of host memory");
        for (int i = 0; i < GS_PROF_RING * GS_PROF_EVENTS; i++) GS_HIP(hipEventCreate(&ctx->ring[i]));
    }
    if (on && !ctx->profile) {                                   // (re)start accumulation
        ctx->stats.prof_frames = 0;
        ctx->stats.sum_ms_sort = ctx->stats.sum_ms_project = ctx->stats.sum_ms_bin = ctx->stats.sum_ms_blend = 0;
        GS_HIP(hipMemsetAsync(&ctx->ctl->acc_frames, 0, offsetof(GsControl, need_near) - offsetof(GsControl, acc_frames), ctx->stream));
        ctx->share_lane.seen_acc_frames = 0;
    }
    ctx->profile = on; ctx->profile_blend_only = on && blend_only; ctx->profile_every = on ? every : 1; ctx->profile_tick = 0;
    return GS_OK;
}

// what a lane aliases of its owner: the resident arrays, the scene inputs and the options its kernels read through the lane
static void lane_adopt_owner(gs_ctx *L, const gs_ctx *ctx)
{
    L->splat = ctx->splat; L->sort_rows = ctx->sort_rows; L->bound_r = ctx->bound_r; L->pow10tab = ctx->pow10tab;
    L->n = ctx->n; L->cap = ctx->cap; L->renderable = ctx->renderable;
    L->scene_depth = ctx->scene_depth; L->scene_rgba = ctx->scene_rgba; L->scene_w = ctx->scene_w; L->scene_h = ctx->scene_h;
    L->record_staged = ctx->record_staged; L->t_eps = ctx->t_eps; L->wide_pairs = ctx->wide_pairs;
}

// lane i of the owner `ctx`, created on first use, with the owner's current resident arrays / options and scratch for them
int gs_ctl::get_lane(gs_ctx *ctx, int i, gs_ctx **out)
{
    gs_ctx *L = ctx->lanes[i];
    if (!L) {
        gs_ctx *primary = nullptr;
        if (i >= GS_MAX_PRIMARY) TRY(get_lane(ctx, i - GS_MAX_PRIMARY, &primary));   // a twin: its primary lane first
        L = new (std::nothrow) gs_ctx();
        if (!L) FAIL(GS_E_OOM, "out of host memory");
        memset(L, 0, sizeof *L);
        L->parent = ctx; L->device = ctx->device;
        const hipError_t e = init_frame_resources(L, primary);
        if (e != hipSuccess) {
            snprintf(GS_ERRBUF(ctx), GS_ERRLEN, "creating pipeline lane %d failed: %s", i, hipGetErrorString(e));
            free_frame_resources(L); delete L;
            return e == hipErrorOutOfMemory ? GS_E_OOM : GS_E_HIP;
        }
        ctx->lanes[i] = L;
        if (primary) {                                           // (the primary's enqueue thread reads `twin` under its mutex)
            if (primary->worker) { std::lock_guard<std::mutex> lk(primary->worker->m); primary->twin = L; }
            else primary->twin = L;
        }
        if (ctx->profile && set_profile(L, true, ctx->profile_blend_only, ctx->profile_every) != GS_OK) { memcpy(ctx->err, L->err, sizeof ctx->err); return GS_E_HIP; }
    }
    if (lane_drain(L) != GS_OK) { if (L != ctx) memcpy(ctx->err, L->err, sizeof ctx->err); return GS_E_HIP; }   // its worker is idle from here on
    if (L != ctx) {
        lane_adopt_owner(L, ctx);
        if (ensure_lane_scratch(L, ctx->cap) != GS_OK) { memcpy(ctx->err, L->err, sizeof ctx->err); return GS_E_OOM; }
    }
    *out = L;
    return GS_OK;
}

// Every lane the options imply -- GS_OPT_PIPELINE_DEPTH lanes, their twins with GS_OPT_FRAME_BATCH = 2 -- created now, with scratch for the
// resident splats and their enqueue threads: a caller that asks for pipelining on a loaded context pays for the lanes THERE (half a
// millisecond each: a stream, a pinned control block, two dozen allocations, a thread) and not in its first six frames
// (`cold_orbit`: 2.6 of the first lap's 11.5 ms).  Lanes of a context nobody asked to pipeline are still created on first use.
int gs_ctl::prepare_lanes(gs_ctx *ctx)
{
    if (!ctx->n || ctx->user_stream || !ctx->renderable) return GS_OK;
    for (int i = 0; i < ctx->pipe_depth; i++) {
        gs_ctx *L = nullptr;
        TRY(get_lane(ctx, i, &L));
        if (ctx->enqueue_threads && ensure_worker(L) != GS_OK) FAIL(GS_E_OOM, "out of host memory");
        if (ctx->frame_batch == 2 && ctx->enqueue_threads) TRY(get_lane(ctx, i + GS_MAX_PRIMARY, &L));
    }
    return GS_OK;
}

// after drain_all(): give every lane the owner's current resident arrays, scene inputs and options
void gs_ctl::refresh_lanes(gs_ctx *ctx)
{
    for (int i = 1; i < GS_MAX_LANES; i++) if (ctx->lanes[i]) lane_adopt_owner(ctx->lanes[i], ctx);
}

// the lane's control block into its pinned mirror, behind what its stream holds; `wait`: until it has arrived
int gs_ctl::lane_read_control(gs_ctx *ctx /* a lane */, bool wait)
{
    GS_HIP(hipMemcpyAsync(ctx->ctl_host, ctx->ctl, sizeof(GsControl), hipMemcpyDeviceToHost, ctx->stream));
    if (wait) GS_HIP(hipStreamSynchronize(ctx->stream));
    return GS_OK;
}

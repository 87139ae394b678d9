// The round-0 share policy: how much of the sorted order a frame's first binning round covers, whether its second round is left out,
// and what the lanes' need words are seeded with.  Host-only plain C++17 -- no HIP, no gs_internal.h: gs_frame.hip fills a GsShareObs
// from each collected lane's GsControl, calls gs_share_observe per lane and gs_share_decide once per collection; tests/host_check/
// compiles this header with g++ alone and replays recorded collections against it (tests/test_share_policy_cpu.py).
// Every float expression here has a fixed type (f32 / f64), operation order and comparison direction: compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef GS_NEAR_FLOOR_MULT
#define GS_NEAR_FLOOR_MULT 1.3f     // the adaptive share never again shrinks below this x the share that failed (1.2: 5 % faster on one orbit, redraws on another)
#endif
#ifndef GS_NEED_MARGIN_MIN
#define GS_NEED_MARGIN_MIN 1.04f    // what the margin on the measured share shrinks to while no frame misses (it starts at GS_NEED_MARGIN)
#endif
#ifndef GS_NEED_MARGIN
#define GS_NEED_MARGIN 1.15         // the share binned first = what the collected frames' tiles needed x this (the walked share ended 1.17-1.3 x above the share that had failed)
#endif
#define GS_SHARE_DEFAULT 0.25f          // the share every context starts with, and starts again with after a reset
#define GS_SHARE_RAISE_MULT 1.5f        // a walked share that failed: now 1.5 x that (and never again below GS_NEAR_FLOOR_MULT x that)
#define GS_SHARE_MISS_MULT 1.3f         // a measured share that missed: 1.3 x that until the frames drawn again have measured
#define GS_NEED_MARGIN_MAX 1.3f         // the margin on the measured need: + GS_NEED_MARGIN_MISS per miss, up to this
#define GS_NEED_MARGIN_MISS 0.1f
#define GS_NEED_MARGIN_STEP 0.01f       // ... and a hundredth less per collection (per GS_NEED_MARGIN_STEP_FRAMES frames of it) that nothing missed
#define GS_NEED_MARGIN_STEP_FRAMES 8u
#define GS_SHARE_ONE_ROUND 0.85f        // a share above this becomes 100 %: two rounds over nearly everything cost more than one
#define GS_SHARE_COVER_MAX 0.85         // ... and so does a cover share that is not below this (an f64 comparison, unlike the one above)
#define GS_SHARE_COVER_MULT 1.25        // one round over the V splats the sort keeps: a share of V x this + GS_SHARE_COVER_PAD positions
#define GS_SHARE_COVER_PAD 4096.0
#define GS_SHARE_MIN_POSITIONS 4096.0f  // never fewer positions than this in round 0
#define GS_SHARE_WALK_MIN 0.001f        // the walked share's minimum ...
#define GS_SHARE_WALK_MIN_SKIP 0.0011f  // ... and what counts as having arrived there (round 1 skippable without a floor)
#define GS_SHARE_WALK_FAST 0.9f         // the unmeasured walk: x this per collection until a share has proved too small once ...
#define GS_SHARE_WALK_SLOW 0.98f        // ... x this afterwards, above the floor
#define GS_NEED_HIST 16                 // the window the measured share follows: this many buckets ...
#define GS_NEED_HIST_FRAMES 16u         // ... of at least this many frames each
#define GS_SKIP_HOLD_FRAMES 32u         // frames that keep round 1 on after a share has failed or missed
#define GS_CLEAN_MEASURED 4u            // clean frames before round 1 is left out: under a measured share ...
#define GS_CLEAN_WALKED 16u             // ... under a walked one
#define GS_REPROBE_FRAMES 64u           // collected single-round frames without a measurement before the share goes back to GS_SHARE_REPROBE
#define GS_SHARE_REPROBE 0.5f
#define GS_NEED_NONE 0xFFFFFFFFu        // need: a tile that no share saturates (sky)

// the owner context's state (one for all its lanes)
struct GsShare {
    float near_frac;               // round 0 covers the nearest near_frac * N splats (adapted from unsat_round0)
    float near_floor;              // never shrink the share below this (1.3 x the share that last proved too small)
    int near_fixed_permille;       // > 0: fixed by GS_OPT_NEAR_PERMILLE instead of adapted
    bool share_measured;           // near_frac comes from a measurement (GsControl::need_near) -- gs_share_from_need
    uint32_t share_kind;           // what kind of order the share was measured on -- 1: whole orders (gs_sort), 2: strips' orders (gs_sort_for);
                                   // 0: nothing yet.  A sort of another kind starts the measurement afresh (positions of a strip's order are not positions of the whole)
    float need_margin;             // the factor on top of the measured need (1.15 ... 1.04 while nothing misses, + 0.1 per miss)
    uint32_t need_hist[GS_NEED_HIST], need_hist_frames[GS_NEED_HIST]; int need_hist_pos;   // the needs of the last collections and the frames each covered (gs_share_from_need)
    uint32_t clean_frames, skip_hold;   // collected frames since the last unsaturated one / frames to keep round 1 on
    uint32_t single_round_frames;  // consecutive collected frames at near_frac == 1 (re-probe occlusion now and then)
    uint32_t cold_sorts;           // sorts run on the caller's thread because the share had not been measured yet (at most two in a row)
    uint32_t cold_frames;          // queued frames drawn synchronously for the same reason (at most two in a row: a context whose frames
                                   // never measure -- counting renders -- keeps its pipelining)
    uint32_t last_kept;            // V of the last collected frame (a near-only sort pays only where V is well above the share read)
    bool adapt_frozen;             // gs_sync is drawing flagged frames again: their counters do not feed the adaptive share
};

// each lane's own state
struct GsShareLane {
    uint32_t need_probe;           // its collections with a measurement (every fourth re-seeds its words)
    uint32_t need_word_est;        // what its need_near words hold at least (host-side estimate: gs_share_lane_seed)
    uint32_t need_seed_pending;    // the seed its next frame's projection writes into the words (GsFrameUniforms::need_seed; 0 = none)
    uint32_t seen_unsat_events; uint64_t seen_acc_frames;   // the lane's cumulative counters at its last collection
    bool last_two_rounds;          // the last enqueued frame ran the two-round path (its unsat count is meaningful)
};

// what one lane's control block says at a collection
struct GsShareObs {
    uint32_t need;                 // the maximum of GsControl::need_near[]
    uint32_t unsat_events; uint64_t acc_frames;
    uint32_t round1_missed, order_incomplete, n_kept;
    bool tiles;                    // the lane's last frame had tiles (gs_stats::n_tiles != 0)
};

// what the lanes of one collection add up to
struct GsShareTally { bool failed; uint32_t need, frames; };

// the share of splats binned first was too small for a frame drawn with `frac_used`: never again below 1.3 x that, now 1.5 x that
static inline void gs_share_raise(GsShare &S, float frac_used)
{
    const float fl = frac_used * GS_NEAR_FLOOR_MULT > 1.0f ? 1.0f : frac_used * GS_NEAR_FLOOR_MULT;
    if (fl > S.near_floor) S.near_floor = fl;
    float nf = frac_used * GS_SHARE_RAISE_MULT;
    if (nf < S.near_floor) nf = S.near_floor;
    if (nf > 1.0f) nf = 1.0f;
    if (nf > S.near_frac) S.near_frac = nf;
    S.clean_frames = 0; S.skip_hold = GS_SKIP_HOLD_FRAMES;
}

// The share of splats binned first, from what the blends of the collected frames MEASURED (GsControl::need_near: per tile, how many of
// the nearest splats it read before its pixels were saturated).  Rounds 1-4 walked the share: x 0.9 per collection from 25 % until a
// share failed, x 1.5 then -- a fresh context needed dozens of collections (and one failure) to arrive, and a 20 M-splat scene drew
// its first hundred frames with 5 M positions in the first round (`cold_orbit`: 63 frames/s).  One collection is enough now.
static inline void gs_share_from_need(GsShare &S, size_t n, uint32_t need, uint32_t frames)
{
    if (!need || S.near_fixed_permille > 0 || !n) return;
    // what the share follows: the largest need of the recent past -- sixteen buckets of at least sixteen frames each (a collection of
    // queued frames is a bucket; synchronous frames, a collection each, share one) -- so that a pose which needs less does not take
    // away what another pose of the same orbit needs: bench.py's orbit is 120 poses whose needs lie between 80 and 125 permille, and a
    // caller may queue hundreds of frames, all drawn with ONE share, before it collects.  Up at once, down when the window has moved on.
    if (S.need_hist_frames[S.need_hist_pos] >= GS_NEED_HIST_FRAMES) {
        S.need_hist_pos = (S.need_hist_pos + 1) % GS_NEED_HIST;
        S.need_hist[S.need_hist_pos] = 0; S.need_hist_frames[S.need_hist_pos] = 0;
    }
    if (need > S.need_hist[S.need_hist_pos]) S.need_hist[S.need_hist_pos] = need;
    // (frames gs_sync is drawing AGAIN -- adapt_frozen -- measure, but are no new evidence of a camera at rest: they neither age the window
    // nor shrink the margin that their own miss has just raised)
    if (!S.adapt_frozen) S.need_hist_frames[S.need_hist_pos] += frames ? frames : 1u;
    uint32_t m = 0;
    for (int k = 0; k < GS_NEED_HIST; k++) if (S.need_hist[k] > m) m = S.need_hist[k];
    float target = 1.0f;                                         // 0xFFFFFFFF: a tile that no share saturates (sky): one round over everything
    if (m != GS_NEED_NONE) {
        // the margin on top follows what the camera does: 1.15 to begin with, a hundredth less with every collection that nothing missed
        // -- with every eight frames of a collection of queued frames: a caller that collects every 24 frames was at 1.10 after a whole
        // lap of 120 new poses without a miss, i.e. had binned 6 % more than it came to need for all of it --
        // (down to 1.04: a still or periodic camera needs none, and 10 % of share are 10 % of the binning and the blend's staging), a tenth
        // more after a miss
        if (S.need_margin < GS_NEED_MARGIN_MIN) S.need_margin = (float)GS_NEED_MARGIN;
        const float less = S.adapt_frozen ? 0.0f : GS_NEED_MARGIN_STEP * (float)(frames > GS_NEED_MARGIN_STEP_FRAMES ? frames / GS_NEED_MARGIN_STEP_FRAMES : 1u);
        S.need_margin = S.need_margin - less < GS_NEED_MARGIN_MIN ? GS_NEED_MARGIN_MIN : S.need_margin - less;
        target = (float)((double)m * (double)S.need_margin / (double)n);
        if (target > GS_SHARE_ONE_ROUND) target = 1.0f;          // (two rounds over nearly everything cost more than one)
    }
    if (target >= 1.0f && S.last_kept) {
        // One round over everything -- but "everything" is the V splats the sort KEEPS, and a cut-out or a strip may keep a few per cent
        // of the N resident ones (the cut-out demo: 226 K of 6.3 M).  A share of 100 % sizes the round for N positions: grids, and row
        // tables of N / 256 chunks per tile row that the row scan reads in full -- project 34 us instead of 24, binning 73 instead of 61.
        // A share that covers V with a quarter to spare draws the same single round (nothing lies beyond it: no tile is flagged) on
        // tables of that size; should V grow past it between two collections, the tiles that want more flag their frames like any
        // other share that was too small.
        const double cover = ((double)S.last_kept * GS_SHARE_COVER_MULT + GS_SHARE_COVER_PAD) / (double)n;
        if (cover < GS_SHARE_COVER_MAX) target = (float)cover;
    }
    if (target < S.near_floor) target = S.near_floor;            // (a walked share's floor, where there is one)
    // (never fewer than 4096 positions: until round 6 never less than one permille -- 21 K positions of a 20 M scene, eight times what a
    // frame sorted for its frustum needs there)
    { const float fl = GS_SHARE_MIN_POSITIONS / (float)n; if (target < fl) target = fl > 1.0f ? 1.0f : fl; }
    S.near_frac = target;
    S.share_measured = true;
}

// a MISS under a measured share (round 1 skipped, a tile unsaturated; the frames are drawn again): the frames that missed needed more
// than `frac_used`, how much more the frames drawn again will measure.  No floor -- the walk's "never again below 1.3 x the share that
// failed" ratchets (1.3 x 92, then 1.3 x 120 = 156 permille over poses that need 80-115) where the measurement simply follows.
static inline void gs_share_missed(GsShare &S, size_t n, float frac_used)
{
    float nf = frac_used * GS_SHARE_MISS_MULT; if (nf > 1.0f) nf = 1.0f;
    if (nf > S.near_frac) S.near_frac = nf;
    if (S.need_margin < GS_NEED_MARGIN_MIN) S.need_margin = (float)GS_NEED_MARGIN;
    S.need_margin = S.need_margin + GS_NEED_MARGIN_MISS > GS_NEED_MARGIN_MAX ? GS_NEED_MARGIN_MAX : S.need_margin + GS_NEED_MARGIN_MISS;
    const uint32_t as_need = (uint32_t)((double)nf * (double)n / (double)S.need_margin);   // (the window remembers it like a measurement)
    if (as_need > S.need_hist[S.need_hist_pos]) S.need_hist[S.need_hist_pos] = as_need;
    S.clean_frames = 0; S.skip_hold = GS_SKIP_HOLD_FRAMES;
}

// One collected lane: what its control block says about the share its frames were drawn with.  The share itself moves here only along
// the unmeasured walk; a failure, the need and the frames go into the tally for gs_share_decide.
static inline void gs_share_observe(GsShare &S, GsShareLane &L, const GsShareObs &o, GsShareTally &T)
{
    S.last_kept = o.n_kept;
    uint32_t need = o.need;
    if (need) {
        // The words are not cleared but SEEDED with 0.9 x the maximum: a tile issues its atomic only when it needs more than the word it
        // read when it started, so after a clear every tile of the first frames would -- 8160 atomics on one cache line serialise at
        // ~11 ns each: the first six frames after every gs_sync took twice as long.  Seeded, only the tiles within 10 % of the maximum
        // speak up; a need that falls is followed 10 % per collection (the word is then an upper bound), one that rises at once.
        // 0xFFFFFFFF (a tile nothing saturates) is kept, and dropped once in sixteen seedings: the scene may have changed.
        // (... every fourth collection of the lane: the host follows the maximum of the last eight collections anyway, and a queue entry
        // per lane and gs_sync is 60 us of a twenty-frame region)
        L.need_word_est = need;                                    // (what the lane's words hold now: their maximum)
        if ((++L.need_probe & 3u) == 0u) {
            const uint32_t seed = need == GS_NEED_NONE ? ((L.need_probe & 63u) ? GS_NEED_NONE : 0u) : (uint32_t)((uint64_t)need * 9u / 10u);
            L.need_seed_pending = seed ? seed : 1u;                // (written by the lane's next frame itself: GsFrameUniforms::need_seed)
            L.need_word_est = seed;
        }
    }
    // (frames drawn from a truncated order measure nothing.  Frames gs_sync draws AGAIN do -- both rounds, every tile's need recorded, the
    // sky's 0xFFFFFFFF included -- and what they measure is what the frames that missed had needed: the share is right after ONE miss.
    // Ignored like the rest of their counters, a camera that left the cloud took eight collections x 24 redrawn frames to get to 100 %)
    if (o.order_incomplete) need = 0;
    if (need > T.need) T.need = need;
    if (S.adapt_frozen || o.order_incomplete) {
        // gs_sync is drawing flagged frames again (redraw_flagged_frames) with the uniforms they were queued with: their share has
        // been dealt with once already -- every one of them would count as a new failure and multiply the share by 1.5.
        // order_incomplete: the frames were drawn from an order that lacked splats (a stash overflowed, the speculative stash could
        // not be vouched for): tiles that did not saturate say nothing about the SHARE -- the frames are drawn again from a whole
        // sort either way.  (Counting them raised the share 23 -> 40 permille outside the cloud at 20 M, past the 1/32 the chunk
        // stashes need: 3 718 -> 1 898 frames/s for good, after one overflow.)
        L.seen_unsat_events = o.unsat_events; L.seen_acc_frames = o.acc_frames;
    } else if (S.near_fixed_permille <= 0 && o.tiles) {
        const uint32_t events = o.unsat_events - L.seen_unsat_events;
        const uint64_t frames = o.acc_frames >= L.seen_acc_frames ? o.acc_frames - L.seen_acc_frames : 1;
        L.seen_unsat_events = o.unsat_events; L.seen_acc_frames = o.acc_frames;
        T.frames += (uint32_t)(frames ? frames : 1);
        if (L.last_two_rounds) {
            // An "event" -- round 0 left tiles unsaturated and round 1 finished them -- is a failure of a WALKED share; with the blend's
            // measurement it is not: round 1 recorded what those tiles needed, and the share is set from that (gs_share_from_need).  Counted as a
            // failure it left a floor of 1.3 x a share that the measurement already covers (bench.py's region: need 111 K splats, the walk of
            // the pre-roll's two-round frames ended at 1.3 x 120 = 156 permille where 1.15 x 106 = 122 do).  A MISS -- round 1 skipped and a
            // tile unsaturated: the frame is drawn again -- is a failure either way.
            // (need == 0xFFFFFFFF -- a tile no share saturates: sky -- is a measurement too: gs_share_from_need goes to one round, or to the share that
            // covers V, at once; counted as a failure it walked there x 1.3 per collection and came back with the margin at 1.3 and a hold: ADVICE r5)
            if ((events && !need) || o.round1_missed) {
                // the share proved too small: raised ONCE per collection (gs_share_decide) -- the frames of all the lanes a
                // gs_sync collects were drawn with the same share, and six lanes reporting the same failure used to multiply it by
                // 1.5^6 and to leave the floor at 1.3 x 1.5^5 of the share that had really failed (a cold context ended up at 70 %)
                T.failed = true;
            } else {
                S.clean_frames += (uint32_t)(frames ? frames : 1);
                if (!need) {
                    // no measurement (counting renders, the pixel-split blend: no need word recorded): the walk of rounds 1-4 -- fast descent (x0.9) until a share
                    // has proved too small once, then a slow drift (x0.98) above the floor
                    float nf = S.near_frac * (S.near_floor > 0.0f ? GS_SHARE_WALK_SLOW : GS_SHARE_WALK_FAST);
                    if (nf < S.near_floor) nf = S.near_floor;
                    if (nf < GS_SHARE_WALK_MIN) nf = GS_SHARE_WALK_MIN;
                    if (nf < S.near_frac) S.near_frac = nf;
                }
                const uint32_t fr = (uint32_t)(frames ? frames : 1);     // the hold is counted in frames, not in collections
                S.skip_hold = S.skip_hold > fr ? S.skip_hold - fr : 0;
            }
            S.single_round_frames = 0;
        } else if (!need && S.near_frac >= 1.0f && ++S.single_round_frames >= GS_REPROBE_FRAMES) {
            S.near_frac = GS_SHARE_REPROBE; S.near_floor = 0.0f; S.single_round_frames = 0; S.clean_frames = 0;   // (unmeasured: re-probe occlusion now and then)
        }
    }
}

// Once per collection, whatever the number of lanes that saw a failure: the share drawn with (`frac_used`) proved too small -> raised;
// else it follows what the collected frames' tiles needed (the maximum over the lanes).  Returns the need the lanes' words are to be
// seeded towards (gs_share_lane_seed), 0 for none.
static inline uint32_t gs_share_decide(GsShare &S, size_t n, float frac_used, const GsShareTally &T)
{
    if (T.failed) {
        if (S.share_measured) gs_share_missed(S, n, frac_used); else gs_share_raise(S, frac_used);
        return 0;
    }
    gs_share_from_need(S, n, T.need, T.frames);
    return T.need;
}

// Every lane's words are brought near what the collected frames measured: a lane whose words are far below it (a lane that has drawn
// nothing yet -- its block is zero --, or nothing of this view) would have EVERY tile of its next frame issue its atomic: 8160 on one
// line, ~90 us -- the first frame of five lanes after a run of synchronous frames, i.e. the fill of bench.py's twenty-frame region.
static inline void gs_share_lane_seed(GsShareLane &L, uint32_t need)
{
    const uint32_t seed = need == GS_NEED_NONE ? need : (uint32_t)((uint64_t)need * 9u / 10u);
    const uint32_t have = L.need_word_est;
    const bool stale = need == GS_NEED_NONE ? have != GS_NEED_NONE : (have != GS_NEED_NONE && (uint64_t)have * 10u < (uint64_t)need * 8u);
    if (!stale) return;
    L.need_seed_pending = seed ? seed : 1u;
    L.need_word_est = seed;
}

// the lane's next frame clears its need words (with the owner's _kind_switch and _unpin resets: a word that still says "a tile no
// share saturates" from frames long gone would keep the share at 100 % for 64 collections)
static inline void gs_share_lane_reseed(GsShareLane &L) { L.need_seed_pending = 1u; L.need_word_est = 0; }

// May a frame leave its second binning round out (and its sort be near-only)?  After 16 clean frames -- but not while the share is
// still on its fast way DOWN from the default (no floor yet): that descent ends with a share that is too small, and with round 1
// still launched the frame that finds it is completed by round 1 (an "event") instead of being flagged and drawn again with
// everything queued behind it.  (A scene that never fails ends at the minimum share: skippable from there.)
static inline bool gs_share_round1_skippable(const GsShare &S)
{
    // (a MEASURED share -- gs_share_from_need -- needs neither the failure that gives the walked share its floor nor sixteen frames of proof)
    return S.near_fixed_permille <= 0 && S.clean_frames >= (S.share_measured ? GS_CLEAN_MEASURED : GS_CLEAN_WALKED) && !S.skip_hold &&
           (S.near_floor > 0.0f || S.near_frac <= GS_SHARE_WALK_MIN_SKIP || S.share_measured);
}

// round 0 covers the nearest near_frac * N splats (or the pinned share of them); 0xFFFFFFFF: everything, one round
static inline uint32_t gs_share_near_count(const GsShare &S, size_t n)
{
    const float frac = S.near_fixed_permille > 0 ? S.near_fixed_permille / 1000.0f : S.near_frac;
    if (frac >= 1.0f) return 0xFFFFFFFFu;
    const double nc = ceil((double)frac * (double)n);
    return nc < 1 ? 1u : (uint32_t)nc;
}

// The four resets.  They differ, and which differences are meant is not decided here (docs/LAB_NOTES.md lists them).
// gs_create: everything
static inline void gs_share_reset_create(GsShare &S) { S = GsShare{}; S.near_frac = GS_SHARE_DEFAULT; }
// gs_clear: leaves need_hist_frames, need_hist_pos, near_fixed_permille, adapt_frozen and the lanes' state alone
static inline void gs_share_reset_clear(GsShare &S)
{
    S.near_frac = GS_SHARE_DEFAULT; S.near_floor = 0.0f; S.clean_frames = 0; S.skip_hold = 0; S.single_round_frames = 0; S.last_kept = 0;
    S.share_measured = false; S.need_margin = 0.0f; S.cold_sorts = 0; S.cold_frames = 0; S.share_kind = 0;
    memset(S.need_hist, 0, sizeof S.need_hist);
}
// a sort of the other kind: leaves single_round_frames, need_hist_pos, last_kept, near_fixed_permille and adapt_frozen alone (share_kind
// is the caller's to set; every lane is reseeded: gs_share_lane_reseed)
static inline void gs_share_reset_kind_switch(GsShare &S)
{
    S.near_frac = GS_SHARE_DEFAULT; S.near_floor = 0.0f; S.share_measured = false; S.need_margin = 0.0f; S.cold_sorts = 0; S.cold_frames = 0;
    S.clean_frames = 0; S.skip_hold = 0;
    memset(S.need_hist, 0, sizeof S.need_hist); memset(S.need_hist_frames, 0, sizeof S.need_hist_frames);
}
// GS_OPT_NEAR_PERMILLE = 0: leaves near_floor, clean_frames, skip_hold, single_round_frames, share_kind, need_hist_frames, need_hist_pos,
// last_kept and adapt_frozen alone (near_fixed_permille is the caller's to set; every lane is reseeded)
static inline void gs_share_reset_unpin(GsShare &S)
{
    S.near_frac = GS_SHARE_DEFAULT; S.share_measured = false; S.need_margin = 0.0f; S.cold_sorts = 0; S.cold_frames = 0;
    memset(S.need_hist, 0, sizeof S.need_hist);
}

// csrc/gs_share.h behind the replay interpreter of share_replay.h: a shared object for tests/test_share_policy_cpu.py, or -- with
// -DSHARE_REPLAY_MAIN -- a program that prints the trace of the script file named on its command line (what a sanitizer build runs).
// Host-only: g++ -std=c++17 -ffp-contract=off, no HIP.
#include "gs_share.h"
#include "share_replay.h"

struct ShareBackend {
    GsShare S;
    struct Lane { GsShareLane L; bool exists, tiles, pending; } lanes[SHARE_REPLAY_LANES];
    size_t n;
    uint32_t need_splats;                                          // gs_stats::need_splats as gs_frame.hip fills it

    void create() { memset(this, 0, sizeof *this); gs_share_reset_create(S); }
    void set_n(size_t v) { n = v; }
    void lane(int i, bool two, bool tiles, bool pending) { Lane &l = lanes[i % SHARE_REPLAY_LANES]; l.exists = true; l.L.last_two_rounds = two; l.tiles = tiles; l.pending = pending; }
    void reseed_lanes() { for (Lane &l : lanes) if (l.exists) gs_share_lane_reseed(l.L); }

    ReplayOut collect(const int *which, int k, const ReplayCtl *ctl, bool idle_only)
    {
        GsShareTally tally{};
        const float frac_used = S.near_frac;
        for (int j = 0; j < k; j++) {
            const ReplayCtl &c = ctl[which[j]];
            Lane &l = lanes[which[j]];
            GsShareObs o;
            o.need = c.need; o.unsat_events = c.unsat_events; o.acc_frames = c.acc_frames; o.round1_missed = c.round1_missed;
            o.order_incomplete = c.order_incomplete; o.n_kept = c.n_kept; o.tiles = l.tiles;
            gs_share_observe(S, l.L, o, tally);
        }
        const uint32_t need = gs_share_decide(S, n, frac_used, tally);
        if (need) {
            need_splats = need;
            for (Lane &l : lanes) if (l.exists && !(idle_only && l.pending)) gs_share_lane_seed(l.L, need);
        }
        return ReplayOut{ tally.failed, need };
    }
    void frozen(bool f) { S.adapt_frozen = f; }
    void pin(int p) { S.near_fixed_permille = p; if (p == 0) { gs_share_reset_unpin(S); reseed_lanes(); } }
    void kind(uint32_t k)
    {
        if (S.share_kind && S.share_kind != k && S.near_fixed_permille <= 0) { gs_share_reset_kind_switch(S); reseed_lanes(); }
        S.share_kind = k;
    }
    void clear() { gs_share_reset_clear(S); }
    void cold(uint32_t sorts, uint32_t frames) { S.cold_sorts = sorts; S.cold_frames = frames; }
    bool skippable() const { return gs_share_round1_skippable(S); }
    uint32_t near_count(size_t of) const { return gs_share_near_count(S, of); }

    std::string state() const
    {
        char b[256];
        std::string s = "frac=" + replay_hex(S.near_frac) + " floor=" + replay_hex(S.near_floor) + " margin=" + replay_hex(S.need_margin);
        snprintf(b, sizeof b, " pin=%d meas=%d kind=%u clean=%u hold=%u single=%u cold=%u,%u kept=%u frozen=%d need_splats=%u pos=%d hist", S.near_fixed_permille,
                 (int)S.share_measured, S.share_kind, S.clean_frames, S.skip_hold, S.single_round_frames, S.cold_sorts, S.cold_frames, S.last_kept, (int)S.adapt_frozen,
                 need_splats, S.need_hist_pos);
        s += b;
        for (int k = 0; k < 16; k++) if (S.need_hist[k] || S.need_hist_frames[k]) { snprintf(b, sizeof b, " %d=%u:%u", k, S.need_hist[k], S.need_hist_frames[k]); s += b; }   // (the buckets that are not 0:0)
        for (int i = 0; i < SHARE_REPLAY_LANES; i++) {
            if (!lanes[i].exists) continue;
            const GsShareLane &L = lanes[i].L;
            snprintf(b, sizeof b, " | L%d probe=%u est=%u pend=%u seen=%u,%llu two=%d", i, L.need_probe, L.need_word_est, L.need_seed_pending, L.seen_unsat_events,
                     (unsigned long long)L.seen_acc_frames, (int)L.last_two_rounds);
            s += b;
        }
        return s;
    }
};

// the trace of `script` into out[0 .. cap); returns its length (nothing is written beyond cap)
extern "C" __attribute__((visibility("default"))) size_t share_replay(const char *script, int full, char *out, size_t cap)
{
    ShareReplay<ShareBackend> r;
    r.full = full != 0;
    const std::string &t = r.replay(script);
    if (out && cap) memcpy(out, t.data(), t.size() < cap ? t.size() : cap);
    return t.size();
}

#ifdef SHARE_REPLAY_MAIN
int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s SCRIPT [full]\n", argv[0]); return 2; }
    ShareReplay<ShareBackend> r;
    r.full = argc > 2;
    const std::string &t = r.replay(replay_read_file(argv[1]).c_str());
    fwrite(t.data(), 1, t.size(), stdout);
    return 0;
}
#endif

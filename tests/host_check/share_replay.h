// Replays scripted collections against the round-0 share policy and prints the whole policy state after every step
// (tests/test_share_policy_cpu.py compares the trace with tests/golden/share_policy.trace, recorded from the functions that
// csrc/gs_share.h replaced).  The interpreter is a template over a backend so that the same scripts can drive another
// implementation of the policy.  Floats are printed as bit patterns: the trace is compared byte for byte.
//
// Script lines (# starts a comment; numbers in C notation, "sky" = 0xFFFFFFFF):
//   script NAME                      a fresh context (everything zero, then the create reset), no lanes
//   n N                              the resident splat count
//   lane I TWO_ROUNDS TILES PENDING  lane I exists; its last frame ran two rounds / had tiles / it has queued, uncollected frames
//   ctl I NEED +EVENTS +FRAMES MISSED INCOMPLETE KEPT   lane I's control block: need word, unsat_events and acc_frames advance
//   acc I FRAMES                     lane I's acc_frames set outright (backwards: the counters were cleared)
//   sync I J ...                     a gs_sync that collects these lanes: observe each, decide once, seed every lane
//   frame I                          a synchronous frame on lane I: observe, decide, seed the idle lanes
//   frozen 0|1                       gs_sync is drawing flagged frames again
//   pin P                            GS_OPT_NEAR_PERMILLE = P (0: the unpin reset)
//   kind K                           a sort of kind K (1 whole, 2 strip): the kind-switch reset where it differs
//   clear                            gs_clear
//   cold SORTS FRAMES                the cold sorts / cold frames gs_frame.hip has counted (only the resets touch them here)
//   show                             print the state
//   repeat N ... end                 (may nest)
// A step that can change the policy state prints one line: script, frozen, pin, kind, clear and show the whole state and the outputs,
// sync and frame a 32-bit hash of that same line (FNV-1a, folded), sixteen to a line behind "= ": 1 600 collections in full are 680 KB.
// `full` prints them so; a state that has gone wrong stays wrong, so a step whose hash collides is caught at the next.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sstream>
#include <string>
#include <vector>

#define SHARE_REPLAY_LANES 6

struct ReplayCtl { uint32_t need, unsat_events; uint64_t acc_frames; uint32_t round1_missed, order_incomplete, n_kept; };
struct ReplayOut { bool failed; uint32_t seed; };

static inline std::string replay_hex(float f) { uint32_t u; memcpy(&u, &f, 4); char b[16]; snprintf(b, sizeof b, "%08x", u); return b; }

// Backend: create(), set_n(size_t), lane(i, two, tiles, pending), collect(const int *lanes, int k, const ReplayCtl *ctl, bool idle_only) -> ReplayOut,
// frozen(bool), pin(int), kind(uint32_t), clear(), cold(uint32_t, uint32_t), state() -> std::string, skippable() -> bool, near_count(size_t n) -> uint32_t
template <class Backend> struct ShareReplay {
    Backend B;
    unsigned hashes = 0;
    bool full = false;                                             // every line in full (to look at; the golden trace is the short form)
    ReplayCtl ctl[SHARE_REPLAY_LANES];
    std::string out;
    std::vector<std::vector<std::string>> prog;

    static uint64_t num(const std::string &s) { return s == "sky" ? 0xFFFFFFFFull : strtoull(s.c_str(), nullptr, 0); }

    // one line per step: the whole state and the outputs -- or, for a collection in the short form, the folded FNV-1a hash of that line
    void step(const char *what, const ReplayOut *o)
    {
        char b[160];
        std::string l = std::string(what) + ' ' + B.state();
        if (o) { snprintf(b, sizeof b, " | failed=%d seed=%u", (int)o->failed, o->seed); l += b; }
        snprintf(b, sizeof b, " | skip=%d nc=%u,%u,%u,%u", (int)B.skippable(), B.near_count(1), B.near_count(4095), B.near_count(1048576), B.near_count(20000000));
        l += b;
        if (o && !full) {
            uint64_t h = 0xcbf29ce484222325ull;
            for (unsigned char ch : l) h = (h ^ ch) * 0x100000001b3ull;
            snprintf(b, sizeof b, "%s%08x", hashes % 16 ? " " : "= ", (uint32_t)(h ^ (h >> 32)));
            out += b;
            if (++hashes % 16 == 0) out += '\n';
            return;
        }
        flush();
        out += l + "\n";
    }
    void flush() { if (hashes % 16) out += '\n'; hashes = 0; }    // (the hashes of consecutive collections stand sixteen to a line, behind "= ")

    size_t run(size_t pc, size_t end)
    {
        for (; pc < end; pc++) {
            const std::vector<std::string> &t = prog[pc];
            const std::string &op = t[0];
            if (op == "repeat") {
                size_t depth = 1, close = pc + 1;
                for (; close < end; close++) { if (prog[close][0] == "repeat") depth++; else if (prog[close][0] == "end" && --depth == 0) break; }
                for (uint64_t k = 0, n = num(t.at(1)); k < n; k++) run(pc + 1, close);
                pc = close;
            } else if (op == "script") {
                memset(ctl, 0, sizeof ctl); B.create(); flush(); out += "# " + t.at(1) + "\n"; step("script", nullptr);
            } else if (op == "n") B.set_n((size_t)num(t.at(1)));
            else if (op == "lane") B.lane((int)num(t.at(1)), num(t.at(2)) != 0, num(t.at(3)) != 0, num(t.at(4)) != 0);
            else if (op == "ctl") {
                ReplayCtl &c = ctl[num(t.at(1)) % SHARE_REPLAY_LANES];
                c.need = (uint32_t)num(t.at(2)); c.unsat_events += (uint32_t)num(t.at(3)); c.acc_frames += num(t.at(4));
                c.round1_missed = (uint32_t)num(t.at(5)); c.order_incomplete = (uint32_t)num(t.at(6)); c.n_kept = (uint32_t)num(t.at(7));
            } else if (op == "acc") ctl[num(t.at(1)) % SHARE_REPLAY_LANES].acc_frames = num(t.at(2));
            else if (op == "sync" || op == "frame") {
                int lanes[SHARE_REPLAY_LANES], k = 0;
                for (size_t a = 1; a < t.size() && k < SHARE_REPLAY_LANES; a++) lanes[k++] = (int)(num(t[a]) % SHARE_REPLAY_LANES);
                const ReplayOut o = B.collect(lanes, k, ctl, op == "frame");
                step(op.c_str(), &o);
            } else if (op == "frozen") { B.frozen(num(t.at(1)) != 0); step("frozen", nullptr); }
            else if (op == "pin") { B.pin((int)num(t.at(1))); step("pin", nullptr); }
            else if (op == "kind") { B.kind((uint32_t)num(t.at(1))); step("kind", nullptr); }
            else if (op == "clear") { B.clear(); step("clear", nullptr); }
            else if (op == "show") step("show", nullptr);
            else if (op == "cold") B.cold((uint32_t)num(t.at(1)), (uint32_t)num(t.at(2)));
            else if (op != "end") { flush(); out += "?? " + op + "\n"; }
        }
        return pc;
    }

    const std::string &replay(const char *script)
    {
        std::istringstream in(script);
        std::string line;
        while (std::getline(in, line)) {
            out += "> " + line + "\n";                              // (the trace carries its script: one file holds both)
            const size_t h = line.find('#');
            if (h != std::string::npos) line.resize(h);
            std::istringstream ls(line);
            std::vector<std::string> t;
            for (std::string w; ls >> w;) t.push_back(w);
            if (!t.empty()) prog.push_back(t);
        }
        run(0, prog.size());
        flush();
        return out;
    }
};

static inline std::string replay_read_file(const char *path)
{
    std::string s;
    if (FILE *f = fopen(path, "rb")) { char b[4096]; for (size_t k; (k = fread(b, 1, sizeof b, f)) > 0;) s.append(b, k); fclose(f); }
    return s;
}

// The blend's coverage factor, checked on every float (csrc/gs_render.hip, GS_BLEND_FACTOR 0 / 1 / 2).
//
// Per pixel and list entry the blend turns the coverage value q = |p|^2 into a weight: 1 where the fragment is kept (q <= qm), 0 where
// it is discarded.  qm is 4 for a pixel inside the strip and -1 for one outside.  Three forms of it exist:
//   0  the compare:   w = q <= qm ? 1 : 0
//   1  two roundings: w = clamp(fma(qm - q, K, 1))          (qm - q rounded first)
//   2  one rounding:  w = clamp(fma(q, -K, c))              (c per pixel: C_IN inside, C_OUT outside)
// with K = (float)1e30 and clamp the [0, 1] clamp of v_pk_fma_f32 (NaN -> 0).  Form 2 needs a float C_IN with
// 0 < C_IN - 4 K < K ulp(4) in exact arithmetic; this program looks for it among the floats around 4 K, fails if there is none or
// more than one, prints it as a hex float, and then compares the three forms:
//   inside  (qm = 4,  c = C_IN):  every one of the 2^32 bit patterns
//   outside (qm = -1, c = C_OUT): every non-negative float, -0, both infinities and every NaN of either sign -- q is a sum of
//                                 squares, so the kernel never holds a negative one, and C_OUT = -1 is not built for them
// Plain C++, fmaf() where the kernel fuses, compiled with -ffp-contract=off so that nothing else is fused.
//
//   c++ -O2 -std=c++17 -ffp-contract=off -pthread blend_factor.cpp -o blend_factor && ./blend_factor
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

static const float K = 1.0e30f;
static const float C_OUT = -1.0f;

static inline float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static inline uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
// the instruction's clamp: NaN -> 0, below 0 -> 0, above 1 -> 1
static inline float clamp01(float x) { return std::isnan(x) ? 0.0f : x < 0.0f ? 0.0f : x > 1.0f ? 1.0f : x; }
static inline float w_compare(float q, float qm) { return q <= qm ? 1.0f : 0.0f; }
static inline float w_two(float q, float qm) { const float d = qm - q; return clamp01(fmaf(d, K, 1.0f)); }
static inline float w_one(float q, float c) { return clamp01(fmaf(q, -K, c)); }

// c is good iff 0 < c - 4 K < K ulp(4), exactly: 4 K, c and K ulp(4) = K 2^-21 are all multiples of 2^76 below 2^103, so long double
// (64-bit significand) or even double holds every term and the differences exactly
static bool c_is_good(float c)
{
    const double d = (double)c - 4.0 * (double)K;
    return d > 0.0 && d < (double)K * std::ldexp(1.0, -21);
}

int main()
{
    // the floats around 4 K, a few hundred to either side
    std::vector<float> good;
    float c = 4.0f * K;
    for (int i = 0; i < 256; i++) c = std::nextafterf(c, 0.0f);
    for (int i = 0; i < 512; i++, c = std::nextafterf(c, INFINITY))
        if (c_is_good(c)) good.push_back(c);
    if (good.size() != 1) {
        std::printf("FAIL: %zu floats c with 0 < c - 4 K < K ulp(4)\n", good.size());
        return 1;
    }
    const float C_IN = good[0];
    std::printf("K = %a  C_IN = %a  C_OUT = %a\n", (double)K, (double)C_IN, (double)C_OUT);

    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
    std::atomic<uint64_t> bad{0}, seen_in{0}, seen_out{0};
    std::atomic<uint32_t> first_bad{0};
    std::vector<std::thread> pool;
    const uint64_t total = 1ull << 32, chunk = (total + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++)
        pool.emplace_back([&, t] {
            uint64_t b_ = 0, ni = 0, no = 0;
            uint32_t fb = 0;
            const uint64_t lo = t * chunk, hi = lo + chunk < total ? lo + chunk : total;
            for (uint64_t i = lo; i < hi; i++) {
                const uint32_t bits = (uint32_t)i;
                const float q = from_bits(bits);
                const float a = w_compare(q, 4.0f), b = w_two(q, 4.0f), d = w_one(q, C_IN);
                ni++;
                // equal as bit patterns: +0 and -0 would not blend alike (they would: e * 0 -- but the claim is "the same value")
                if (to_bits(a) != to_bits(b) || to_bits(a) != to_bits(d)) { if (!b_) fb = bits; b_++; }
                const bool dom = !(bits >> 31) || bits == 0x80000000u || std::isinf(q) || std::isnan(q);
                if (dom) {
                    const float oa = w_compare(q, -1.0f), ob = w_two(q, -1.0f), od = w_one(q, C_OUT);
                    no++;
                    if (to_bits(oa) != to_bits(ob) || to_bits(oa) != to_bits(od)) { if (!b_) fb = bits; b_++; }
                }
            }
            bad += b_; seen_in += ni; seen_out += no;
            if (b_) first_bad = fb;
        });
    for (auto &th : pool) th.join();
    std::printf("inside: %llu values, outside: %llu values, disagreements: %llu\n", (unsigned long long)seen_in.load(),
                (unsigned long long)seen_out.load(), (unsigned long long)bad.load());
    if (seen_in.load() != total) { std::printf("FAIL: not every bit pattern was visited\n"); return 1; }
    if (bad.load()) { std::printf("FAIL: e.g. q = %a (0x%08x)\n", (double)from_bits(first_bad.load()), first_bad.load()); return 1; }
    std::printf("OK\n");
    return 0;
}

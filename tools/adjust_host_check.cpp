// adjust_host_check.cpp -- csrc/gs_adjust.h on the host, stand-alone, for a sanitizer run on the CPU (no GPU, no library, nothing preloaded):
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I aframe-gaussian-splatting_amd/csrc \
//       tools/adjust_host_check.cpp -o /tmp/adjust_host_check && /tmp/adjust_host_check
//
// The hand-made colour words of tests/test_adjust_cpu.py (all-0, all-255, bytes that land on x.5) and every byte value per channel through
// gsm::adjust_word under an identity, a halving, a clamping and a negative map, with the ties' expected bytes spelled out; SH rows of degree
// 1..3 through gsm::adjust_sh_coef, separate output and in place, the identity giving every bit back.  Exit status 0 and "ok" when all hold.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "gs_adjust.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | g << 8 | b << 16 | a << 24; }

static bool params(const float m[9], float o0, float o1, float o2, float as, float ao, gsm::AdjustParams &p)
{
    const float off[3] = { o0, o1, o2 };
    return gsm::adjust_widen(m, off, as, ao, p);
}

int main()
{
    const float I[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, HALF[9] = { 0.5f, 0, 0, 0, 0.5f, 0, 0, 0, 0.5f };
    const float NEG[9] = { -1, 0, 0, 0.25f, -1.5f, 0.75f, 0, 1, -0.5f };
    gsm::AdjustParams ident, half, clamp, neg, bad;
    CHECK(params(I, 0, 0, 0, 1, 0, ident), "identity refused");
    CHECK(params(HALF, 0, 0, 0, 0.5f, 0, half), "halving refused");
    CHECK(params(I, 300, -300, 0.5f, 1, -300, clamp), "clamping refused");
    CHECK(params(NEG, 255, 64, 12.5f, 0, 77.5f, neg), "negative refused");
    CHECK(ident.dc[0] == 0.0 && ident.dc[1] == 0.0 && ident.dc[2] == 0.0, "the identity's band-0 constant is not 0");
    CHECK(!params(I, NAN, 0, 0, 1, 0, bad) && !params(I, 0, 0, 0, INFINITY, 0, bad) && !params(I, 0, 0, 0, 1, -INFINITY, bad), "a non-finite parameter passed");
    float nanm[9]; memcpy(nanm, I, sizeof nanm); nanm[4] = NAN;
    CHECK(!params(nanm, 0, 0, 0, 1, 0, bad), "a NaN matrix entry passed");

    const uint32_t hand[] = { 0u, 0xFFFFFFFFu, rgba(1, 3, 5, 7), rgba(253, 255, 251, 1), rgba(5, 1, 3, 255), rgba(255, 0, 255, 0), rgba(0, 255, 0, 128),
                              rgba(127, 128, 129, 77), rgba(2, 4, 6, 8) };
    for (uint32_t w : hand) CHECK(gsm::adjust_word(w, ident) == w, "identity changed %#x", w);
    for (uint32_t v = 0; v < 256; v++) {
        const uint32_t w = rgba(v, 255 - v, v ^ 0x55u, v);
        CHECK(gsm::adjust_word(w, ident) == w, "identity changed %#x", w);
        const uint32_t h = gsm::adjust_word(w, half);
        const uint32_t want = (v >> 1) + ((v & 1u) && ((v >> 1) & 1u) ? 1u : 0u);          // v / 2, ties to even
        CHECK((h & 0xFFu) == want && (h >> 24) == want, "half of %u is %u, expected %u", v, h & 0xFFu, want);
        const uint32_t c = gsm::adjust_word(w, clamp);
        CHECK((c & 0xFFu) == 255u && ((c >> 8) & 0xFFu) == 0u && (c >> 24) == 0u, "clamps of %#x: %#x", w, c);
        CHECK((gsm::adjust_word(w, neg) >> 24) == 78u, "alpha scale 0, offset 77.5: %u", gsm::adjust_word(w, neg) >> 24);
        CHECK((gsm::adjust_word(w, neg) & 0xFFu) == 255u - v, "255 - %u", v);
    }
    CHECK(gsm::adjust_word(rgba(1, 3, 5, 7), half) == rgba(0, 2, 2, 4), "ties: 0.5 1.5 2.5 3.5");
    CHECK(gsm::adjust_word(rgba(253, 255, 251, 1), half) == rgba(126, 128, 126, 0), "ties: 126.5 127.5 125.5 0.5");
    CHECK(gsm::adjust_word(rgba(10, 200, 7, 250), clamp) == rgba(255, 0, 8, 0) && gsm::adjust_word(rgba(10, 200, 8, 250), clamp) == rgba(255, 0, 8, 0), "7.5 and 8.5 -> 8");

    for (int degree = 1; degree <= 3; degree++) {
        const int K = (degree + 1) * (degree + 1);
        std::vector<float> row(3 * (size_t)K), out(3 * (size_t)K), inplace;
        for (int i = 0; i < 3 * K; i++) row[(size_t)i] = (float)((i * 37 % 101) - 50) / 64.0f;
        const gsm::AdjustParams *ps[] = { &ident, &half, &neg };
        for (const gsm::AdjustParams *p : ps) {
            inplace = row;
            for (int k = 0; k < K; k++) {
                const float in[3] = { row[(size_t)k], row[(size_t)(K + k)], row[(size_t)(2 * K + k)] };
                float o[3];
                gsm::adjust_sh_coef(in, k, *p, o);
                out[(size_t)k] = o[0]; out[(size_t)(K + k)] = o[1]; out[(size_t)(2 * K + k)] = o[2];
                float io[3] = { inplace[(size_t)k], inplace[(size_t)(K + k)], inplace[(size_t)(2 * K + k)] };
                gsm::adjust_sh_coef(io, k, *p, io);                                           // out == in
                inplace[(size_t)k] = io[0]; inplace[(size_t)(K + k)] = io[1]; inplace[(size_t)(2 * K + k)] = io[2];
            }
            CHECK(memcmp(out.data(), inplace.data(), out.size() * sizeof(float)) == 0, "degree %d: in place differs", degree);
            if (p == &ident) CHECK(memcmp(out.data(), row.data(), out.size() * sizeof(float)) == 0, "degree %d: the identity changed a row", degree);
            if (p == &half) for (int i = 0; i < 3 * K; i++) if (i % K) CHECK(out[(size_t)i] == row[(size_t)i] * 0.5f, "degree %d: half of coefficient %d", degree, i);
        }
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}

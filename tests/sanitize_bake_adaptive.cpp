// sanitize_bake_adaptive.cpp — the host half of the bake's statistics and adaptive sampling
// (csrc/prt_bake_adaptive_contract.h, csrc/prt_adaptive.h) under AddressSanitizer + UBSan: a stand-alone program over the
// HIP-free headers, built and run by tests/test_sanitize_bake_adaptive.py.  It drives the settings' refusals in the header's
// order, the block count, the noise formula over exactly sized heap arrays (ASan watches every bound) with counts below 2,
// black texels, NaN, infinities and huge values, and the stopping rule on the same inputs.
// usage: sanitize_bake_adaptive [rounds]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "prt_bake_adaptive_contract.h"

static int g_bad = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            ++g_bad;                           \
            printf("UNEXPECTED: " __VA_ARGS__); \
            printf("\n");                      \
        }                                      \
    } while (0)

static bool says(const char* why, const char* text) { return why && strstr(why, text); }

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 20000;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::numeric_limits<float>::max();

    // ---- blocks ----
    EXPECT(prt_bake_block_count(5, 3) == 1u && prt_bake_block_count(13, 11) == 4u && prt_bake_block_count(24, 16) == 6u &&
               prt_bake_block_count(72, 40) == 45u && prt_bake_block_count(16384, 16384) == 2048u * 2048u && prt_bake_block_count(1, 9) == 2u,
           "block counts");

    // ---- the settings' refusals, in the header's order: an entry wrong in everything reports the first ----
    {
        PrtBakeAdaptive c{0u, 0u, 5000u, -1.0f, nan, {0u, 1u, 0u}};
        EXPECT(says(prt_bake_adaptive_refusal(nullptr, 4, 4), "null settings"), "null");
        EXPECT(says(prt_bake_adaptive_refusal(&c, 4, 4), "reserved"), "reserved first");
        c.reserved[1] = 0u;
        EXPECT(says(prt_bake_adaptive_refusal(&c, 4, 4), "min_spp = 0"), "min_spp");
        c.min_spp = 8u;
        c.max_spp = 4u;
        EXPECT(says(prt_bake_adaptive_refusal(&c, 4, 4), ">= 0"), "negative threshold");
        c.threshold = nan, c.noise_floor = 0.0f;
        EXPECT(says(prt_bake_adaptive_refusal(&c, 4, 4), ">= 0"), "NaN threshold");
        c.threshold = 0.0f, c.noise_floor = -0.0f;
        EXPECT(says(prt_bake_adaptive_refusal(&c, 4, 4), "both 0"), "both 0 (a negative zero is a zero)");
        c.threshold = 0.05f;
        EXPECT(says(prt_bake_adaptive_refusal(&c, 4, 4), "max_spp < min_spp"), "max < min");
        c.max_spp = 5000u;
        EXPECT(says(prt_bake_adaptive_refusal(&c, 4, 4), "step_spp is 0"), "step 0");
        c.step_spp = 1u;
        EXPECT(says(prt_bake_adaptive_refusal(&c, 4, 4), "PRT_RADIANCE_MAX_SAMPLES"), "above the limit");
        c.max_spp = PRT_RADIANCE_MAX_SAMPLES;
        EXPECT(prt_bake_adaptive_refusal(&c, 4, 4) == nullptr && prt_bake_adaptive_refusal(&c, 1024, 1023) == nullptr, "valid");
        EXPECT(says(prt_bake_adaptive_refusal(&c, 1024, 1024), "2^32 - 1") && says(prt_bake_adaptive_refusal(&c, 16384, 16384), "2^32 - 1"), "paths");
        c = PrtBakeAdaptive{8u, 0u, 8u, inf, 0.0f, {0u, 0u, 0u}};
        EXPECT(prt_bake_adaptive_refusal(&c, 4, 4) == nullptr, "step 0 with max == min, an infinite threshold");
        EXPECT(says(prt_bake_rule_refusal(0.1f, -1e-30f), ">= 0") && says(prt_bake_rule_refusal(0.1f, nan), ">= 0") &&
                   prt_bake_rule_refusal(0.0f, 1e-30f) == nullptr,
               "the rule's pair alone");
    }

    // ---- the noise formula and the rule over exactly sized arrays ----
    std::mt19937 rng(71u);
    std::uniform_real_distribution<float> u(0.0f, 4.0f);
    const float odd[] = {0.0f, -0.0f, 1.0f, 1.5f, 2.0f, nan, inf, -inf, big, -1.0f, 1e-40f, 16777216.0f};
    for (int r = 0; r < rounds; ++r) {
        const size_t n = 1u + (size_t)(rng() % 37u);
        std::vector<float> cnt(n), A(n), Q(n), out(n, -7.0f);
        for (size_t t = 0; t < n; ++t) {
            const bool weird = rng() % 5u == 0u;
            cnt[t] = weird ? odd[rng() % 12u] : (float)(rng() % 300u);
            A[t] = rng() % 7u == 0u ? odd[rng() % 12u] : u(rng) * cnt[t];
            Q[t] = rng() % 7u == 0u ? odd[rng() % 12u] : u(rng) * u(rng) * cnt[t];
        }
        const float floor = r % 3 == 0 ? 0.0f : 0.01f;
        EXPECT(prt_bake_noise_rule(n, cnt.data(), A.data(), Q.data(), floor, out.data()), "noise refused");
        for (size_t t = 0; t < n; ++t) {
            if (cnt[t] == 0.0f) EXPECT(out[t] == 0.0f && !std::signbit(out[t]), "count 0 gives 0");
            else if (!(cnt[t] >= 2.0f)) EXPECT(out[t] == inf, "count %g gives +inf, got %g", (double)cnt[t], (double)out[t]);
            else if (std::isfinite(cnt[t]) && std::isfinite(A[t]) && std::isfinite(Q[t]) && A[t] > 0.0f)
                EXPECT(out[t] >= 0.0f, "a finite texel with light has a noise >= 0, got %g", (double)out[t]);
            // the rule and the formula agree where both are defined: unconverged iff rel_err > threshold
            const float thr = 0.05f;
            const bool un = prt_adaptive_rule(cnt[t], A[t], Q[t], thr, floor);
            if (cnt[t] < 2.0f) EXPECT(un, "count < 2 is unconverged");
            if (cnt[t] != cnt[t] || A[t] != A[t] || Q[t] != Q[t]) EXPECT(cnt[t] < 2.0f || !un, "a NaN is converged");
            if (cnt[t] >= 2.0f && std::isfinite(cnt[t]) && std::isfinite(A[t]) && std::isfinite(Q[t]) && A[t] > 0.0f && std::isfinite(out[t])) {
                // (away from the boundary: the formula is rounded to fp32, the rule compares squares in double)
                if (out[t] > thr * 1.001f) EXPECT(un, "noise %g above the threshold but converged", (double)out[t]);
                if (out[t] < thr * 0.999f) EXPECT(!un, "noise %g below the threshold but unconverged", (double)out[t]);
            }
        }
    }
    {
        float one = 1.0f, o = 0.0f;
        EXPECT(!prt_bake_noise_rule(1, &one, &one, &one, -0.1f, &o) && !prt_bake_noise_rule(1, &one, &one, &one, nan, &o), "floor refused");
        EXPECT(!prt_bake_noise_rule(1, nullptr, &one, &one, 0.1f, &o) && !prt_bake_noise_rule(1, &one, nullptr, &one, 0.1f, &o) &&
                   !prt_bake_noise_rule(1, &one, &one, nullptr, 0.1f, &o) && !prt_bake_noise_rule(1, &one, &one, &one, 0.1f, nullptr),
               "null arrays refused");
        EXPECT(prt_bake_noise_rule(0, nullptr, nullptr, nullptr, 0.1f, nullptr), "n = 0 needs no array");
        // a constant texel: Q / n rounds below m^2, V clamps to 0
        const float c8 = 8.0f, A8 = 8.0f * 0.7f, Q8 = 8.0f * 0.49f;
        EXPECT(prt_bake_noise_rule(1, &c8, &A8, &Q8, 0.0f, &o) && o >= 0.0f && o < 1e-3f, "constant texel: %g", (double)o);
        EXPECT(!prt_adaptive_rule(c8, A8, Q8, 0.01f, 0.0f), "constant texel is converged");
        const float z = 0.0f;
        EXPECT(prt_bake_noise_rule(1, &c8, &z, &z, 0.0f, &o) && o != o, "black texel, floor 0: 0 / 0");
        EXPECT(prt_bake_noise_rule(1, &c8, &z, &z, 0.01f, &o) && o == 0.0f, "black texel with a floor: 0");
    }
    printf(g_bad ? "%d UNEXPECTED results\n" : "no sanitizer report, %d unexpected results\n", g_bad);
    return g_bad ? 1 : 0;
}

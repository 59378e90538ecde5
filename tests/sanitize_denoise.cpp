// sanitize_denoise.cpp — the host half of the film denoiser (csrc/prt_denoise_contract.h) under AddressSanitizer + UBSan:
// a stand-alone program over the HIP-free header, built and run by tests/test_sanitize_denoise.py.  It holds the variance of
// the mean luminance to a long double restatement on the edge inputs (n = 0, 1, 2, a huge Q, Q / n below m^2, NaN and
// negative weights) and on random ones, and fuzzes the validation against an independent statement of the rules.
// usage: sanitize_denoise [rounds]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "prt_denoise_contract.h"

static int g_bad = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            ++g_bad;                           \
            printf("UNEXPECTED: " __VA_ARGS__); \
            printf("\n");                      \
        }                                      \
    } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// the rule again, from its wording, in double (a long double here would round twice)
static float want_variance(float n, float A, float Q) {
    if (!(n > 0.0f)) return 0.0f;
    volatile double m = (double)A / (double)n;
    if (n < 2.0f) {
        volatile float mf = (float)m;
        volatile float v = mf * mf;
        return v;
    }
    volatile double q = (double)Q / (double)n;
    volatile double mm = m * m;
    volatile double d = q - mm;
    volatile double V = d > 0.0 ? d : 0.0;
    volatile double r = V / ((double)n - 1.0);
    return (float)r;
}

static bool want_ok(const PrtDenoise* k, uint32_t W, uint32_t H, bool arrays) {
    if (k) {
        if (k->iterations > 6u || k->normal_power_log2 > 8u) return false;
        if (std::isnan(k->sigma_l) || std::isnan(k->sigma_z) || k->sigma_l <= 0.0f || k->sigma_z <= 0.0f) return false;
    }
    if (!arrays) return false;
    const unsigned long long n = (unsigned long long)W * H;
    return n != 0ull && n <= (1ull << 28);
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 20000;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::numeric_limits<float>::max();

    // ---- the moments: edge inputs ----
    EXPECT(same_bits(prt_denoise_variance_rule(0.0f, 0.0f, 0.0f), 0.0f), "n = 0");
    EXPECT(same_bits(prt_denoise_variance_rule(0.0f, 3.0f, 9.0f), 0.0f), "n = 0 with moments");
    EXPECT(same_bits(prt_denoise_variance_rule(-1.0f, 3.0f, 9.0f), 0.0f), "negative n");
    EXPECT(same_bits(prt_denoise_variance_rule(nan, 3.0f, 9.0f), 0.0f), "NaN n");
    EXPECT(same_bits(prt_denoise_variance_rule(1.0f, 0.5f, 0.25f), 0.25f), "n = 1: m^2");
    EXPECT(same_bits(prt_denoise_variance_rule(1.0f, 0.0f, 0.0f), 0.0f), "n = 1, black");
    EXPECT(same_bits(prt_denoise_variance_rule(2.0f, 1.0f, 0.5f), 0.0f), "n = 2, equal samples");
    EXPECT(same_bits(prt_denoise_variance_rule(2.0f, 1.0f, 1.0f), 0.25f), "n = 2, samples 0 and 1: V = 1/4, / 1");
    EXPECT(same_bits(prt_denoise_variance_rule(3.0f, 0.3f, 0.03f * 0.9999f), 0.0f), "Q / n below m^2 clamps to 0");
    EXPECT(std::isfinite(prt_denoise_variance_rule(8.0f, 1.0f, big)) && prt_denoise_variance_rule(8.0f, 1.0f, big) > 1e36f, "huge Q stays finite in double");
    EXPECT(prt_denoise_variance_rule(2.0f, 0.0f, big) == inf || std::isfinite(prt_denoise_variance_rule(2.0f, 0.0f, big)), "huge Q, n = 2");
    EXPECT(prt_denoise_variance_rule(8.0f, big, big) == 0.0f, "m^2 above Q / n: 0, no overflow to NaN");
    EXPECT(prt_denoise_variance_rule(1.0f, big, 0.0f) == inf, "n = 1: fl(m)^2 overflows to +inf in fp32");
    EXPECT(prt_denoise_variance_rule(8.0f, 1.0f, inf) == inf, "infinite Q");
    EXPECT(std::isnan(prt_denoise_variance_rule(8.0f, nan, 1.0f)) || prt_denoise_variance_rule(8.0f, nan, 1.0f) == 0.0f, "NaN A does not trap");
    EXPECT(same_bits(prt_denoise_mean_rule(3.0f, 0.0f), 0.0f) && same_bits(prt_denoise_mean_rule(3.0f, 2.0f), 1.5f), "mean rule");
    EXPECT(same_bits(prt_denoise_mean_rule(nan, 0.0f), 0.0f) && same_bits(prt_denoise_mean_rule(1.0f, nan), 0.0f), "mean rule, weight 0 / NaN");

    // ---- the moments: random inputs against the restatement ----
    std::mt19937 rng(12345u);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    const float weights[] = {0.0f, 1.0f, 2.0f, 3.0f, 8.0f, 64.0f, 1000.0f, 16777216.0f};
    for (int i = 0; i < rounds; ++i) {
        const float n = weights[rng() % 8u];
        const float scale = std::ldexp(1.0f, (int)(rng() % 80u) - 40);
        const float y = u01(rng) * scale, spread = (rng() & 1u) ? u01(rng) * scale : 0.0f;
        const float A = n * y, Q = n * (y * y + spread * spread) * ((rng() % 16u) ? 1.0f : 0.999f);
        const float got = prt_denoise_variance_rule(n, A, Q), want = want_variance(n, A, Q);
        EXPECT(same_bits(got, want), "variance(%g, %g, %g) = %g, want %g", n, A, Q, got, want);
        EXPECT(!(got < 0.0f), "negative variance");
    }

    // ---- validation: fuzzed against the rules as the header states them ----
    EXPECT(prt_denoise_check(nullptr, 4u, 3u, true) == nullptr, "NULL = the defaults");
    const PrtDenoise def = prt_denoise_default_config();
    EXPECT(def.iterations == 5u && def.sigma_l == 4.0f && def.sigma_z == 0.1f && def.normal_power_log2 == 6u && def.demodulate == 1u, "defaults");
    EXPECT(prt_denoise_check(&def, 1u << 14, 1u << 14, true) == nullptr, "2^28 pixels");
    EXPECT(prt_denoise_check(&def, (1u << 14) + 1u, 1u << 14, true) != nullptr, "above 2^28 pixels");
    EXPECT(prt_denoise_check(&def, 0xFFFFFFFFu, 0xFFFFFFFFu, true) != nullptr, "the product does not wrap");
    const float sigmas[] = {4.0f, 0.1f, 1e-30f, big, inf, 0.0f, -0.0f, -1.0f, nan, -inf, 1.0f};
    const uint32_t sizes[] = {0u, 1u, 2u, 44u, 1u << 14, (1u << 14) + 1u, 1u << 16, 0x7FFFFFFFu, 0xFFFFFFFFu};
    int refused = 0, accepted = 0;
    for (int i = 0; i < rounds; ++i) {
        PrtDenoise k;
        k.iterations = (rng() % 4u) ? rng() % 7u : rng();
        k.normal_power_log2 = (rng() % 4u) ? rng() % 9u : rng();
        k.sigma_l = sigmas[rng() % 11u];
        k.sigma_z = sigmas[rng() % 11u];
        k.demodulate = rng();
        const uint32_t W = sizes[rng() % 9u], H = sizes[rng() % 9u];
        const bool arrays = (rng() % 8u) != 0u, null_cfg = (rng() % 16u) == 0u;
        const char* msg = prt_denoise_check(null_cfg ? nullptr : &k, W, H, arrays);
        const bool ok = want_ok(null_cfg ? nullptr : &k, W, H, arrays);
        EXPECT((msg == nullptr) == ok, "check(it %u, sl %g, sz %g, np %u, %u x %u, arrays %d) says %s", k.iterations, k.sigma_l, k.sigma_z,
               k.normal_power_log2, W, H, (int)arrays, msg ? msg : "ok");
        EXPECT(!msg || std::strncmp(msg, "denoise:", 8) == 0, "message prefix");
        (msg ? refused : accepted)++;
    }
    EXPECT(refused > rounds / 10 && accepted > rounds / 100, "the fuzz reaches both sides (%d refused, %d accepted)", refused, accepted);

    if (g_bad) {
        printf("%d UNEXPECTED results\n", g_bad);
        return 1;
    }
    printf("no sanitizer report: %d rounds, %d settings refused, %d accepted\n", rounds, refused, accepted);
    return 0;
}

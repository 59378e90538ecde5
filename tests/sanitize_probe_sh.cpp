// sanitize_probe_sh.cpp — the host half of the SH probes (csrc/prt_sh_contract.h) under AddressSanitizer + UBSan: a
// stand-alone program over the HIP-free header, built and run by tests/test_sanitize_probe_sh.py.  It drives the basis and
// the irradiance rule over exactly sized heap arrays (ASan watches every bound) for every order, with random directions,
// the axes, non-unit directions, NaN, infinities and huge values, holds the values to closed forms where there are some,
// and checks the refusals.
// usage: sanitize_probe_sh [rounds]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "prt_sh_contract.h"

static int g_bad = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            ++g_bad;                           \
            printf("UNEXPECTED: " __VA_ARGS__); \
            printf("\n");                      \
        }                                      \
    } while (0)

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 20000;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::numeric_limits<float>::max();
    std::mt19937 rng(97u);
    std::normal_distribution<float> g(0.0f, 1.0f);

    // ---- counts, constants, the axes ----
    EXPECT(prt_sh_count(0u) == 1u && prt_sh_count(1u) == 4u && prt_sh_count(2u) == 9u, "counts");
    EXPECT(prt_sh_basis(0u, 0.3f, -0.2f, 0.9f) == 0.282094792f && prt_sh_basis(9u, 1.0f, 1.0f, 1.0f) == 0.0f, "Y0 and past the end");
    EXPECT(prt_sh_basis(1u, 0.0f, 1.0f, 0.0f) == 0.488602512f && prt_sh_basis(2u, 0.0f, 0.0f, -1.0f) == -0.488602512f &&
               prt_sh_basis(3u, 1.0f, 0.0f, 0.0f) == 0.488602512f,
           "band 1 on the axes");
    EXPECT(prt_sh_basis(6u, 0.0f, 0.0f, 1.0f) == 0.315391565f * 2.0f && prt_sh_basis(6u, 1.0f, 0.0f, 0.0f) == -0.315391565f, "Y6 on the axes");
    EXPECT(prt_sh_basis(8u, 1.0f, 0.0f, 0.0f) == 0.546274215f && prt_sh_basis(8u, 0.0f, 1.0f, 0.0f) == -0.546274215f, "Y8 on the axes");
    EXPECT(prt_sh_cosine_factor(0u) == 3.14159274f && prt_sh_cosine_factor(3u) == 2.09439516f && prt_sh_cosine_factor(4u) == 0.785398185f &&
               prt_sh_cosine_factor(8u) == 0.785398185f,
           "the cosine's band factors");

    // ---- refusals ----
    float one[3] = {0.0f, 1.0f, 0.0f}, nine[9], three[3];
    EXPECT(!prt_sh_eval_rule(1, one, 3u, nine) && !prt_sh_eval_rule(1, nullptr, 2u, nine) && !prt_sh_eval_rule(1, one, 2u, nullptr), "eval refusals");
    EXPECT(prt_sh_eval_rule(0, nullptr, 2u, nullptr) && prt_sh_irradiance_rule(0, nullptr, nullptr, 0u, nullptr), "n = 0 needs no array");
    EXPECT(!prt_sh_irradiance_rule(1, nine, one, 0xFFFFFFFFu, three) && !prt_sh_irradiance_rule(1, nullptr, one, 2u, three) &&
               !prt_sh_irradiance_rule(1, nine, nullptr, 2u, three) && !prt_sh_irradiance_rule(1, nine, one, 2u, nullptr),
           "irradiance refusals");

    // ---- exactly sized arrays of every order; orthonormality and the addition theorem over random unit directions ----
    const float special[] = {nan, inf, -inf, big, -big, 1e30f, 0.0f, -0.0f, 1e-38f, 0.125f, 3.7f, -1.0f};
    double gram[9][9] = {};
    int n_unit = 0;
    for (uint32_t order = 0; order <= PRT_SH_MAX_ORDER; ++order) {
        const uint32_t K = prt_sh_count(order);
        const size_t n = (size_t)rounds;
        std::vector<float> d(3 * n), Y(n * K), c(n * K * 3), E(3 * n);
        for (size_t i = 0; i < n; ++i) {
            float v[3] = {g(rng), g(rng), g(rng)};
            const float l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            const bool odd = (rng() % 16u) == 0u;
            for (int a = 0; a < 3; ++a) d[3 * i + a] = odd ? special[rng() % 12u] : v[a] / (l > 0.0f ? l : 1.0f);
            for (uint32_t k = 0; k < 3 * K; ++k) c[i * K * 3 + k] = (rng() % 64u) == 0u ? special[rng() % 12u] : g(rng);
        }
        EXPECT(prt_sh_eval_rule(n, d.data(), order, Y.data()), "eval, order %u", order);
        EXPECT(prt_sh_irradiance_rule(n, c.data(), d.data(), order, E.data()), "irradiance, order %u", order);
        for (size_t i = 0; i < n; ++i) {
            const float x = d[3 * i], y = d[3 * i + 1], z = d[3 * i + 2];
            const bool finite = std::isfinite(x) && std::isfinite(y) && std::isfinite(z) && std::fabs(x) < 1e18f && std::fabs(y) < 1e18f && std::fabs(z) < 1e18f;
            for (uint32_t k = 0; k < K; ++k) {
                EXPECT(Y[i * K + k] == prt_sh_basis(k, x, y, z) || (std::isnan(Y[i * K + k]) && std::isnan(prt_sh_basis(k, x, y, z))), "row %zu, k %u", i, k);
                EXPECT(!finite || std::isfinite(Y[i * K + k]), "a finite direction gives a finite value");
            }
            const double l2 = (double)x * x + (double)y * y + (double)z * z;
            if (order == 2u && finite && std::fabs(l2 - 1.0) < 1e-5) {
                double s1 = 0.0, s2 = 0.0;
                for (uint32_t k = 1; k < 4; ++k) s1 += (double)Y[i * K + k] * Y[i * K + k];
                for (uint32_t k = 4; k < 9; ++k) s2 += (double)Y[i * K + k] * Y[i * K + k];
                // the addition theorem: the squares of band l sum to (2 l + 1) / (4 pi) on the unit sphere
                EXPECT(std::fabs(s1 - 3.0 / (4.0 * M_PI)) < 1e-5 && std::fabs(s2 - 5.0 / (4.0 * M_PI)) < 1e-5, "addition theorem: %g %g", s1, s2);
                for (uint32_t j = 0; j < 9; ++j)
                    for (uint32_t k = 0; k < 9; ++k) gram[j][k] += (double)Y[i * K + j] * Y[i * K + k];
                ++n_unit;
            }
        }
    }
    EXPECT(n_unit > rounds / 2, "the fuzz keeps unit directions (%d)", n_unit);
    double worst = 0.0;
    for (uint32_t j = 0; j < 9; ++j)
        for (uint32_t k = 0; k < 9; ++k) worst = std::fmax(worst, std::fabs(4.0 * M_PI / n_unit * gram[j][k] - (j == k ? 1.0 : 0.0)));
    EXPECT(worst < 8.0 / std::sqrt((double)n_unit), "orthonormal over %d directions: worst entry %g", n_unit, worst);

    // ---- a constant sky: only coefficient 0, E = pi c whatever the normal and the order ----
    for (uint32_t order = 0; order <= PRT_SH_MAX_ORDER; ++order) {
        const uint32_t K = prt_sh_count(order);
        std::vector<float> c(K * 3, 0.0f);
        const float sky[3] = {0.75f, 1.5f, 0.1f};
        for (int a = 0; a < 3; ++a) c[a] = sky[a] * 3.54490770f;  // c 2 sqrt(pi)
        const float normals[3][3] = {{0.0f, 1.0f, 0.0f}, {0.6f, 0.0f, -0.8f}, {-0.57735027f, 0.57735027f, 0.57735027f}};
        for (const float* nn : normals) {
            float e[3];
            EXPECT(prt_sh_irradiance_rule(1, c.data(), nn, order, e), "constant sky");
            for (int a = 0; a < 3; ++a) EXPECT(std::fabs(e[a] / (M_PI * sky[a]) - 1.0) < 1e-6, "E = pi c: %g for %g", e[a], sky[a]);
        }
    }

    if (g_bad) {
        printf("%d UNEXPECTED results\n", g_bad);
        return 1;
    }
    printf("no sanitizer report: %d rounds per order, %d unit directions, worst Gram entry %g\n", rounds, n_unit, worst);
    return 0;
}

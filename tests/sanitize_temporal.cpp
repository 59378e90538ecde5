// sanitize_temporal.cpp — the host half of the temporal reprojection (csrc/prt_temporal_contract.h) under AddressSanitizer +
// UBSan: a stand-alone program over the HIP-free header, built and run by tests/test_sanitize_temporal.py.  It fuzzes the
// validation against an independent statement of the rules, and drives the projection rule, the copy lookup and the
// previous-surface rule with NaN, infinities, points at and behind the camera, huge coordinates and an empty instance list;
// whatever the projection accepts must lead to tap indices the kernel can test against the image without overflow.
// usage: sanitize_temporal [rounds]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "prt_temporal_contract.h"

static int g_bad = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            ++g_bad;                           \
            printf("UNEXPECTED: " __VA_ARGS__); \
            printf("\n");                      \
        }                                      \
    } while (0)

static bool want_ok(const PrtTemporal* k, uint32_t W, uint32_t H, const PrtCameraBasis* K, bool arrays) {
    if (k) {
        if (std::isnan(k->max_history) || k->max_history < 1.0f) return false;
        if (std::isnan(k->normal_min) || k->normal_min < -1.0f || k->normal_min > 1.0f) return false;
        if (std::isnan(k->plane_tol) || k->plane_tol < 0.0f) return false;
    }
    if (!arrays) return false;
    const unsigned long long n = (unsigned long long)W * H;
    if (n == 0ull || n > (1ull << 28) || H > 262140u) return false;
    if (K && (K->W != (float)W || K->H != (float)H)) return false;
    return true;
}

static PrtCameraBasis basis(uint32_t W, uint32_t H, float tan_fov_y) {
    return PrtCameraBasis{{0.5f, 1.0f, 3.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, -1.0f}, (float)W, (float)H, tan_fov_y};
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 20000;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::numeric_limits<float>::max();
    std::mt19937 rng(4321u);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);

    // ---- validation ----
    const PrtTemporal def = prt_temporal_default_config();
    EXPECT(def.max_history == 32.0f && def.normal_min == 0.9f && def.plane_tol == 0.01f, "defaults");
    EXPECT(prt_temporal_check(nullptr, 4u, 3u, nullptr, true) == nullptr, "NULL = the defaults");
    EXPECT(prt_temporal_check(&def, 1u << 14, 1u << 14, nullptr, true) == nullptr, "2^28 pixels");
    EXPECT(prt_temporal_check(&def, (1u << 14) + 1u, 1u << 14, nullptr, true) != nullptr, "above 2^28 pixels");
    EXPECT(prt_temporal_check(&def, 0xFFFFFFFFu, 0xFFFFFFFFu, nullptr, true) != nullptr, "the product does not wrap");
    const float vals[] = {32.0f, 1.0f, 0.99f, 0.0f, -0.0f, -1.0f, 1.0001f, 0.9f, 0.01f, big, inf, -inf, nan, 1000.0f, -1.0001f, 1e-30f};
    EXPECT(prt_temporal_check(&def, 1u, 262140u, nullptr, true) == nullptr && prt_temporal_check(&def, 1u, 262141u, nullptr, true) != nullptr,
           "the rows one launch covers");
    const uint32_t sizes[] = {0u, 1u, 2u, 44u, 1u << 14, (1u << 14) + 1u, 1u << 16, 262140u, 262141u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    int refused = 0, accepted = 0;
    for (int i = 0; i < rounds; ++i) {
        PrtTemporal k{vals[rng() % 16u], vals[rng() % 16u], vals[rng() % 16u]};
        if (rng() % 3u == 0u) k = PrtTemporal{32.0f, 0.9f, 0.01f};
        const uint32_t W = sizes[rng() % 11u], H = sizes[rng() % 11u];
        PrtCameraBasis K = basis(W, H, 0.5f);
        const unsigned kk = rng() % 8u;
        if (kk == 0u) K.W = K.W + 1.0f;
        if (kk == 1u) K.H = nan;
        const bool arrays = (rng() % 8u) != 0u, null_cfg = (rng() % 16u) == 0u, null_K = (rng() % 4u) == 0u;
        const char* msg = prt_temporal_check(null_cfg ? nullptr : &k, W, H, null_K ? nullptr : &K, arrays);
        const bool ok = want_ok(null_cfg ? nullptr : &k, W, H, null_K ? nullptr : &K, arrays);
        EXPECT((msg == nullptr) == ok, "check(%g, %g, %g, %u x %u, arrays %d) says %s", k.max_history, k.normal_min, k.plane_tol, W, H, (int)arrays,
               msg ? msg : "ok");
        EXPECT(!msg || std::strncmp(msg, "temporal:", 9) == 0, "message prefix");
        (msg ? refused : accepted)++;
    }
    EXPECT(refused > rounds / 10 && accepted > rounds / 100, "the fuzz reaches both sides (%d refused, %d accepted)", refused, accepted);

    // ---- the projection rule ----
    const uint32_t W = 44u, H = 28u;
    const PrtCameraBasis K = basis(W, H, 0.5463f);
    float fx, fy, vv, z;
    EXPECT(prt_temporal_project(K, PrtTpV3{0.5f, 1.0f, 2.0f}, &fx, &fy, &vv, &z) && fx == 21.5f && fy == 13.5f && z == 1.0f, "the centre: %g %g", fx, fy);
    EXPECT(!prt_temporal_project(K, PrtTpV3{0.5f, 1.0f, 3.0f}, &fx, &fy, &vv, &z) && z == 0.0f, "z = 0: at the camera");
    EXPECT(!prt_temporal_project(K, PrtTpV3{0.5f, 1.0f, 4.0f}, &fx, &fy, &vv, &z) && z < 0.0f, "behind the camera");
    EXPECT(!prt_temporal_project(K, PrtTpV3{100.0f, 1.0f, 2.0f}, &fx, &fy, &vv, &z), "off-screen");
    const float special[] = {nan, inf, -inf, big, -big, 1e30f, -1e30f, 0.0f, -0.0f, 1e-38f, 1.0f, -1.0f};
    int inside = 0, outside = 0;
    std::vector<uint8_t> image((size_t)W * H, 1);   // what a tap index is read from: ASan watches the bounds
    for (int i = 0; i < rounds; ++i) {
        float p3[3] = {u(rng) * 6.0f, u(rng) * 6.0f, u(rng) * 8.0f};
        if (rng() % 4u == 0u) p3[rng() % 3u] = special[rng() % 12u];
        PrtTpV3 P{p3[0], p3[1], p3[2]};
        if (rng() % 16u == 0u) P = PrtTpV3{special[rng() % 12u], special[rng() % 12u], special[rng() % 12u]};
        fx = fy = vv = z = nan;
        const bool in = prt_temporal_project(K, P, &fx, &fy, &vv, &z);
        (in ? inside : outside)++;
        if (!in) continue;
        EXPECT(z > 0.0f && fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H && vv >= 0.0f, "accepted outside the image: %g %g %g", fx, fy, z);
        const int ix = (int)std::floor(fx), iy = (int)std::floor(fy);   // (UBSan: the conversion must be in range)
        const float tx = fx - std::floor(fx), ty = fy - std::floor(fy);
        EXPECT(ix >= -1 && ix < (int)W && iy >= -1 && iy < (int)H && tx >= 0.0f && tx < 1.0f && ty >= 0.0f && ty < 1.0f, "tap origin %d %d", ix, iy);
        unsigned sum = 0;
        for (int t = 0; t < 4; ++t) {
            const int xx = ix + (t & 1), yy = iy + (t >> 1);
            if (xx < 0 || xx >= (int)W || yy < 0 || yy >= (int)H) continue;
            sum += image[(size_t)yy * W + (size_t)xx];
        }
        EXPECT(sum >= 1u, "a point inside (-1, W) x (-1, H) has a tap in the image");
    }
    EXPECT(inside > rounds / 20 && outside > rounds / 20, "the fuzz reaches both sides (%d inside, %d outside)", inside, outside);

    // ---- the tap test and the blend on edge inputs ----
    const PrtTpV3 N0{0.0f, 0.0f, 1.0f}, P0{0.0f, 0.0f, 0.0f};
    EXPECT(prt_temporal_tap_valid(1.0f, 0, N0, P0, P0, N0, 0.9f, 0.0f), "the point itself");
    EXPECT(!prt_temporal_tap_valid(0.0f, 0, N0, P0, P0, N0, 0.9f, 1.0f), "hn = 0");
    EXPECT(!prt_temporal_tap_valid(nan, 0, N0, P0, P0, N0, 0.9f, 1.0f), "hn NaN");
    EXPECT(!prt_temporal_tap_valid(1.0f, -1, N0, P0, P0, N0, 0.9f, 1.0f), "a miss");
    EXPECT(!prt_temporal_tap_valid(1.0f, 0, PrtTpV3{nan, 0.0f, 1.0f}, P0, P0, N0, -1.0f, 1.0f), "NaN normal");
    EXPECT(!prt_temporal_tap_valid(1.0f, 0, N0, PrtTpV3{0.0f, 0.0f, inf}, P0, N0, 0.9f, big), "infinite position");
    EXPECT(!prt_temporal_tap_valid(1.0f, 0, N0, PrtTpV3{0.0f, 0.0f, 0.5f}, P0, N0, 0.9f, 0.25f), "off the plane");
    EXPECT(prt_temporal_tap_valid(1.0f, 0, N0, PrtTpV3{5.0f, -3.0f, 0.25f}, P0, N0, 0.9f, 0.25f), "on the plane's tolerance");
    EXPECT(prt_temporal_variance_rule(1.0f, 0.5f, 0.5f) == 0.25f && prt_temporal_variance_rule(5.0f, 1.0f, 0.5f) == 0.0f, "variance rule");
    EXPECT(prt_temporal_variance_rule(3.0f, 0.0f, 1.0f) == 0.5f && !(prt_temporal_variance_rule(8.0f, big, big) < 0.0f), "variance rule, N' - 1");

    // ---- the copy lookup and the previous-surface rule ----
    EXPECT(prt_temporal_find_copy(nullptr, 0u, 5) == -1 && prt_temporal_find_copy(nullptr, 0u, -1) == -1, "an empty instance list");
    const uint32_t range[] = {100u, 12u, 112u, 20u, 132u, 1u, 0x7FFFFFF0u, 0x20u};
    EXPECT(prt_temporal_find_copy(range, 4u, 99) == -1 && prt_temporal_find_copy(range, 4u, 100) == 0 && prt_temporal_find_copy(range, 4u, 111) == 0, "copy 0");
    EXPECT(prt_temporal_find_copy(range, 4u, 112) == 1 && prt_temporal_find_copy(range, 4u, 131) == 1 && prt_temporal_find_copy(range, 4u, 132) == 2, "copies 1, 2");
    EXPECT(prt_temporal_find_copy(range, 4u, 133) == -1 && prt_temporal_find_copy(range, 4u, 0x7FFFFFFF) == 3 && prt_temporal_find_copy(range, 4u, -5) == -1, "gaps and the last prim");
    for (int i = 0; i < rounds; ++i) {
        const uint32_t n = rng() % 5u;
        const int32_t prim = (int32_t)(rng() % 200u) - 20;
        const int32_t k = prt_temporal_find_copy(range, n, prim);
        int32_t want = -1;
        for (uint32_t j = 0; j < n; ++j)
            if (prim >= 0 && (uint32_t)prim >= range[2 * j] && (uint32_t)prim - range[2 * j] < range[2 * j + 1]) want = (int32_t)j;
        EXPECT(k == want, "find_copy(%u, %d) = %d, want %d", n, prim, k, want);
    }
    const float ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const float half_moved[12] = {0.5f, 0, 0, 0, 0.5f, 0, 0, 0, 0.5f, 1000.0f, -2.0f, 3.0f};
    PrtTpV3 Pp, Np;
    prt_temporal_prev_surface_rule(ident, ident, PrtTpV3{1.0f, 2.0f, 3.0f}, N0, &Pp, &Np);
    EXPECT(Pp.x == 1.0f && Pp.y == 2.0f && Pp.z == 3.0f && Np.z == 1.0f && Np.x == 0.0f, "identity");
    prt_temporal_prev_surface_rule(ident, half_moved, PrtTpV3{2.0f, 2.0f, 2.0f}, N0, &Pp, &Np);
    EXPECT(Pp.x == 1001.0f && Pp.y == -1.0f && Pp.z == 4.0f && Np.z == 1.0f, "scale 1/2, 1000 away: %g %g %g %g", Pp.x, Pp.y, Pp.z, Np.z);
    for (int i = 0; i < rounds; ++i) {   // non-finite points and normals go through without a trap; a projection of them is refused or in range
        PrtTpV3 P{special[rng() % 12u], u(rng), special[rng() % 12u]}, N{special[rng() % 12u], u(rng), u(rng)};
        prt_temporal_prev_surface_rule(ident, half_moved, P, N, &Pp, &Np);
        if (prt_temporal_project(K, Pp, &fx, &fy, &vv, &z)) EXPECT(fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H, "accepted out of range");
    }

    if (g_bad) {
        printf("%d UNEXPECTED results\n", g_bad);
        return 1;
    }
    printf("no sanitizer report: %d rounds, %d settings refused, %d accepted, %d points inside, %d outside\n", rounds, refused, accepted, inside, outside);
    return 0;
}

// prt_sh_contract.h — the real spherical-harmonic basis of the SH probes (include/prt.h "SH probes"), up to order 2, and
// the irradiance its coefficients give.  Plain C++ with no HIP header, as prt_temporal_contract.h: k_sh_project
// (prt_probe_sh.hip), prt_sh_eval / prt_sh_irradiance (prt_api.cpp) and tests/sanitize_probe_sh.cpp compile these same
// lines, so the basis is written once.  The library is built without floating-point contraction, so the device and the
// host evaluate the same IEEE operations in the same order: every line below is one rounding per written operation.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)
#define PRT_SH_FN __host__ __device__ inline
#else
#define PRT_SH_FN inline
#endif

#define PRT_SH_MAX_ORDER 2u
#define PRT_SH_MAX_COEFFS 9u

// (order + 1)^2: 1, 4, 9
PRT_SH_FN uint32_t prt_sh_count(uint32_t order) { return (order + 1u) * (order + 1u); }

// Y_k of the direction (x, y, z), k = 0 .. 8: the usual real-SH ordering (l, m) = (0,0) (1,-1) (1,0) (1,1) (2,-2) (2,-1)
// (2,0) (2,1) (2,2) with z the polar axis.  The direction is used as given; k > 8 gives 0.
PRT_SH_FN float prt_sh_basis(uint32_t k, float x, float y, float z) {
    switch (k) {
        case 0u: return 0.282094792f;
        case 1u: return 0.488602512f * y;
        case 2u: return 0.488602512f * z;
        case 3u: return 0.488602512f * x;
        case 4u: return 1.092548431f * (x * y);
        case 5u: return 1.092548431f * (y * z);
        case 6u: return 0.315391565f * (3.0f * (z * z) - 1.0f);
        case 7u: return 1.092548431f * (x * z);
        case 8u: return 0.546274215f * ((x * x) - (y * y));
        default: return 0.0f;
    }
}

// The clamped cosine's band factors: pi, 2 pi / 3, pi / 4
PRT_SH_FN float prt_sh_cosine_factor(uint32_t k) { return k == 0u ? 3.14159274f : (k < 4u ? 2.09439516f : 0.785398185f); }

// Y[i][k] = Y_k(dirs[i]) for k < (order + 1)^2.  false: order > 2 or a null array with n != 0.
inline bool prt_sh_eval_rule(size_t n, const float* dirs, uint32_t order, float* Y) {
    if (order > PRT_SH_MAX_ORDER || (n != 0u && (!dirs || !Y))) return false;
    const uint32_t K = prt_sh_count(order);
    for (size_t i = 0; i < n; ++i)
        for (uint32_t k = 0; k < K; ++k) Y[i * K + k] = prt_sh_basis(k, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    return true;
}

// E[i][c] = the fp32 sum, from 0.0f over k ascending, of fl(fl(A_k * Y_k(normals[i])) * coeffs[i][k][c]); not clamped.
inline bool prt_sh_irradiance_rule(size_t n, const float* coeffs, const float* normals, uint32_t order, float* E) {
    if (order > PRT_SH_MAX_ORDER || (n != 0u && (!coeffs || !normals || !E))) return false;
    const uint32_t K = prt_sh_count(order);
    for (size_t i = 0; i < n; ++i) {
        float e[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t k = 0; k < K; ++k) {
            const float w = prt_sh_cosine_factor(k) * prt_sh_basis(k, normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
            for (int c = 0; c < 3; ++c) e[c] = e[c] + w * coeffs[(i * K + k) * 3 + c];
        }
        for (int c = 0; c < 3; ++c) E[3 * i + c] = e[c];
    }
    return true;
}

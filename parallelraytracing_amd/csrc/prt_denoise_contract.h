// prt_denoise_contract.h — the host-visible half of the film denoiser (include/prt.h "First-hit feature images and the
// edge-avoiding film denoiser"): the defaults, the validation of every entry point and the variance of the mean luminance
// that prt_film_denoise feeds the filter with.  Plain C++ with no HIP header, as prt_adaptive.h: k_dn_film_prepare
// (prt_denoise.hip), prt_denoise_variance (prt_api.cpp), prt_group_film_denoise (prt_group.cpp) and
// tests/sanitize_denoise.cpp compile these same lines.  The library is built without floating-point contraction, so the
// device and the host evaluate the same IEEE operations in the same order.
#pragma once
#include <stdint.h>

#include "../../include/prt.h"

#if defined(__HIP__)
#define PRT_DENOISE_FN __host__ __device__ inline
#else
#define PRT_DENOISE_FN inline
#endif

#define PRT_DENOISE_MAX_ITERATIONS 6u
#define PRT_DENOISE_MAX_NORMAL_POWER_LOG2 8u

inline PrtDenoise prt_denoise_default_config() { return PrtDenoise{5u, 4.0f, 0.1f, 6u, 1u}; }

// n = the pixel's film weight, A = sum of y, Q = sum of y^2 (fp32 sums in sample order).  In double, rounded once:
// m = A / n, V = max(0, Q / n - m m) (the rounding of the fp32 sums can leave Q / n below m^2), var = V / (n - 1): the squared
// standard error of the mean.  0 < n < 2: fl(m) * fl(m) in fp32.  n = 0 (or negative, or NaN): 0.
PRT_DENOISE_FN float prt_denoise_variance_rule(float n, float A, float Q) {
    if (!(n > 0.0f)) return 0.0f;
    const double dn = (double)n;
    const double m = (double)A / dn;
    if (n < 2.0f) {
        const float mf = (float)m;
        return mf * mf;
    }
    const double d = (double)Q / dn - m * m;
    const double V = d > 0.0 ? d : 0.0;
    return (float)(V / (dn - 1.0));
}

// The mean of one film channel: rgb_sum / weight in fp32, 0 for a pixel of weight 0.
PRT_DENOISE_FN float prt_denoise_mean_rule(float sum, float n) { return n > 0.0f ? sum / n : 0.0f; }

// nullptr: the settings and the image size are usable; otherwise what is wrong with them.  cfg == nullptr means the
// defaults.  arrays_ok: the caller's own "no required array is null".
inline const char* prt_denoise_check(const PrtDenoise* cfg, uint32_t W, uint32_t H, bool arrays_ok) {
    if (cfg) {
        if (cfg->iterations > PRT_DENOISE_MAX_ITERATIONS) return "denoise: iterations must be 0..6";
        if (!(cfg->sigma_l > 0.0f)) return "denoise: sigma_l must be > 0";
        if (!(cfg->sigma_z > 0.0f)) return "denoise: sigma_z must be > 0";
        if (cfg->normal_power_log2 > PRT_DENOISE_MAX_NORMAL_POWER_LOG2) return "denoise: normal_power_log2 must be 0..8";
    }
    if (!arrays_ok) return "denoise: null array";
    const uint64_t n = (uint64_t)W * (uint64_t)H;
    if (n == 0u) return "denoise: empty image";
    if (n > (uint64_t)PRT_DENOISE_MAX_PIXELS) return "denoise: more than 2^28 pixels";
    return nullptr;
}

// prt_adaptive.h — the stopping rule of prt_render_adaptive (include/prt.h "Film
// statistics and adaptive sampling").  Plain C++ with no HIP header: k_tile_select (prt_kernels.hip) and the exported
// prt_adaptive_unconverged (prt_api.cpp) compile these same lines, once for the device and once for the
// host.  The library is built without floating-point contraction, so both evaluate the same IEEE operations in the same order.
#pragma once

#if defined(__HIP__)
#define PRT_ADAPTIVE_FN __host__ __device__ inline
#else
#define PRT_ADAPTIVE_FN inline
#endif

// n = the pixel's film weight (its sample count), A = sum of y, Q = sum of y^2 (fp32 sums in sample order).  In double:
// m = A / n, V = max(0, Q / n - m m) (the rounding of the fp32 sums can leave Q / n below m^2), lhs = V / (n - 1) = the squared
// standard error of the mean, t = threshold (m + noise_floor); unconverged = n < 2 || lhs > t t.
PRT_ADAPTIVE_FN bool prt_adaptive_rule(float n, float A, float Q, float threshold, float noise_floor) {
    if (n < 2.0f) return true;
    const double dn = (double)n;
    const double m = (double)A / dn;
    const double d = (double)Q / dn - m * m;
    const double V = d > 0.0 ? d : 0.0;
    const double lhs = V / (dn - 1.0);
    const double t = (double)threshold * (m + (double)noise_floor);
    return lhs > t * t;
}

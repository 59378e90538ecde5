// prt_temporal_contract.h — the host-visible half of the temporal reprojection (include/prt.h "Temporal reprojection"):
// the defaults, the validation of every entry point and every rule the host evaluates as well as the device: the
// previous-surface rule, the projection into the previous frame, the tap test, the blend and the variance.  Plain C++ with
// no HIP header, as prt_denoise_contract.h: k_tp_reproject (prt_temporal.hip), prt_temporal_prev_surface (prt_api.cpp) and
// tests/sanitize_temporal.cpp compile these same lines.  The library is built without floating-point contraction, so the
// device and the host evaluate the same IEEE operations in the same order.
#pragma once
#include <stdint.h>

#include "../../include/prt.h"
#include "prt_denoise_contract.h"  // prt_denoise_variance_rule: the variance of a pixel without history

#if defined(__HIP__)
#define PRT_TEMPORAL_FN __host__ __device__ inline
#else
#define PRT_TEMPORAL_FN inline
#endif

#define PRT_TEMPORAL_SB_MIN 0.015625f  // 2^-6: the least valid tap weight that counts as history
#define PRT_TEMPORAL_MAX_ROWS 262140u  // 4 rows a block x 65535 blocks: what one launch of k_tp_reproject covers

struct PrtTpV3 {
    float x, y, z;
};

inline PrtTemporal prt_temporal_default_config() { return PrtTemporal{32.0f, 0.9f, 0.01f}; }

// nullptr: the settings, the image size and the basis are usable; otherwise what is wrong with them.  cfg == nullptr means
// the defaults, K == nullptr "no basis to check" (prt_film_temporal keeps its own).  arrays_ok: the caller's own "no
// required array is null".
inline const char* prt_temporal_check(const PrtTemporal* cfg, uint32_t W, uint32_t H, const PrtCameraBasis* K, bool arrays_ok) {
    if (cfg) {
        if (!(cfg->max_history >= 1.0f)) return "temporal: max_history must be >= 1";
        if (!(cfg->normal_min >= -1.0f && cfg->normal_min <= 1.0f)) return "temporal: normal_min must be in [-1, 1]";
        if (!(cfg->plane_tol >= 0.0f)) return "temporal: plane_tol must be >= 0";
    }
    if (!arrays_ok) return "temporal: null array";
    const uint64_t n = (uint64_t)W * (uint64_t)H;
    if (n == 0u) return "temporal: empty image";
    if (n > (uint64_t)PRT_TEMPORAL_MAX_PIXELS) return "temporal: more than 2^28 pixels";
    if (H > PRT_TEMPORAL_MAX_ROWS) return "temporal: more than 262140 rows";
    if (K && !(K->W == (float)W && K->H == (float)H)) return "temporal: the previous basis is not of this image's size";
    return nullptr;
}

PRT_TEMPORAL_FN float prt_tp_dot(PrtTpV3 a, PrtTpV3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// mat4 * (p, 1) with the project's grouping (prt_device.h transform_point); m: rows 0..2 of the column-major mat4, m[c * 3 + r]
PRT_TEMPORAL_FN PrtTpV3 prt_tp_point(const float* m, PrtTpV3 p) {
    PrtTpV3 r;
    r.x = (m[0] * p.x + m[3] * p.y) + (m[6] * p.z + m[9] * 1.0f);
    r.y = (m[1] * p.x + m[4] * p.y) + (m[7] * p.z + m[10] * 1.0f);
    r.z = (m[2] * p.x + m[5] * p.y) + (m[8] * p.z + m[11] * 1.0f);
    return r;
}
// lin(M) * n: the upper 3 x 3 of the same matrix, (x + y) + z
PRT_TEMPORAL_FN PrtTpV3 prt_tp_lin(const float* m, PrtTpV3 n) {
    PrtTpV3 r;
    r.x = (m[0] * n.x + m[3] * n.y) + m[6] * n.z;
    r.y = (m[1] * n.x + m[4] * n.y) + m[7] * n.z;
    r.z = (m[2] * n.x + m[5] * n.y) + m[8] * n.z;
    return r;
}
PRT_TEMPORAL_FN PrtTpV3 prt_tp_normalize(PrtTpV3 v) {
    const float s = 1.0f / __builtin_sqrtf(prt_tp_dot(v, v));
    return PrtTpV3{v.x * s, v.y * s, v.z * s};
}

// The placed copy whose primitive range holds prim: the last k with prim_base[k] <= prim (prim_base ascends), if prim <
// prim_base[k] + n_tris[k]; -1 otherwise (a miss, an analytic primitive, a world-space triangle, an empty table).
// range: n records {prim_base, n_tris}.
PRT_TEMPORAL_FN int32_t prt_temporal_find_copy(const uint32_t* range, uint32_t n, int32_t prim) {
    if (prim < 0 || n == 0u) return -1;
    const uint32_t p = (uint32_t)prim;
    uint32_t lo = 0u, hi = n;  // the first k with prim_base[k] > p
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (range[2u * mid] <= p) lo = mid + 1u;
        else hi = mid;
    }
    if (lo == 0u) return -1;
    const uint32_t k = lo - 1u;
    return p - range[2u * k] < range[2u * k + 1u] ? (int32_t)k : -1;
}

// The previous surface of a point of copy k: inv_cur / mat_prev are 12 floats each (rows 0..2, column-major).
PRT_TEMPORAL_FN void prt_temporal_prev_surface_rule(const float* inv_cur, const float* mat_prev, PrtTpV3 P, PrtTpV3 N, PrtTpV3* Pprev,
                                                    PrtTpV3* Nprev) {
    *Pprev = prt_tp_point(mat_prev, prt_tp_point(inv_cur, P));
    *Nprev = prt_tp_normalize(prt_tp_lin(mat_prev, prt_tp_lin(inv_cur, N)));
}

// The projection of Pprev into the previous frame.  false: behind the camera (!(z > 0)) or outside the image (a NaN fails
// both).  true: *fx in (-1, W), *fy in (-1, H) are the continuous pixel coordinates, *vv = v . v.  *z_out gets z always.
PRT_TEMPORAL_FN bool prt_temporal_project(const PrtCameraBasis& K, PrtTpV3 Pprev, float* fx, float* fy, float* vv, float* z_out) {
    const PrtTpV3 v{Pprev.x - K.pos[0], Pprev.y - K.pos[1], Pprev.z - K.pos[2]};
    const float z = prt_tp_dot(v, PrtTpV3{K.front[0], K.front[1], K.front[2]});
    *z_out = z;
    if (!(z > 0.0f)) return false;
    const float x = prt_tp_dot(v, PrtTpV3{K.right[0], K.right[1], K.right[2]});
    const float y = prt_tp_dot(v, PrtTpV3{K.up[0], K.up[1], K.up[2]});
    const float aspect = K.W / K.H;
    const float ndcX = (x / z) / (aspect * K.tan_fov_y);
    const float ndcY = (y / z) / K.tan_fov_y;
    const float px = ((ndcX + 1.0f) * 0.5f) * K.W - 0.5f;
    const float py = ((1.0f - ndcY) * 0.5f) * K.H - 0.5f;
    *fx = px;
    *fy = py;
    *vv = prt_tp_dot(v, v);
    return px > -1.0f && px < K.W && py > -1.0f && py < K.H;
}

// A tap of the previous frame (inside the image already): its history length, prim, normal and position against the
// previous surface.  lim = plane_tol * sqrtf(v . v).
PRT_TEMPORAL_FN bool prt_temporal_tap_valid(float hn, int32_t hprim, PrtTpV3 hN, PrtTpV3 hP, PrtTpV3 Pprev, PrtTpV3 Nprev, float normal_min,
                                            float lim) {
    if (!(hn > 0.0f) || hprim < 0) return false;
    if (!(prt_tp_dot(Nprev, hN) >= normal_min)) return false;
    const PrtTpV3 D{hP.x - Pprev.x, hP.y - Pprev.y, hP.z - Pprev.z};
    const float d = prt_tp_dot(D, Nprev);
    return (d < 0.0f ? -d : d) <= lim;
}

// The variance of the blended mean luminance, in double and rounded once.
PRT_TEMPORAL_FN float prt_temporal_variance_rule(float N1, float m1, float m2) {
    const double d = (double)m2 - (double)m1 * (double)m1;
    const double V = d > 0.0 ? d : 0.0;
    const double k = (double)N1 - 1.0;
    return (float)(V / (k > 1.0 ? k : 1.0));
}

// a = min(n / N', 1) with N' = min(Nh + n, max_history)
PRT_TEMPORAL_FN float prt_temporal_blend(float h, float c, float a) { return h + a * (c - h); }

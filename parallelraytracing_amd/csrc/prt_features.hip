// prt_features.hip — the device code of the guide features through specular chains (include/prt.h "Guide features through
// specular chains").  A translation unit of its own: nothing in prt_kernels.hip, prt_denoise.hip or prt_temporal.hip
// changes for it.  Built with the flags of prt_kernels.hip: no contraction, so every line below is the IEEE operation it
// spells, and tests/guide_features_replay.py restates them in numpy float32.  The vertex math is the shade kernels' own
// (prt_device.h): reflect3, refract3, fresnel_reflectance, normalize3, dot3, glm_min.
#include <hip/hip_runtime.h>

#include "prt_features.h"
#include "prt_device.h"

namespace {

inline uint32_t blocks_for(uint32_t n) { return (n + 255u) / 256u; }

PRT_DEV bool finite3(f3 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }

// Steps 2 and 3 of the contract for the chain of `pixel` (k vertices followed so far, length L, throughput T) whose
// segment of direction d has the closest hit hits[j]: the pixel's three guide records, or the next segment appended to
// `out`.  Called by every lane of the wave (live = false: a lane beyond the list), because the append is a stream
// compaction: ballot of "continues", rank = popcount below the lane, one integer atomicAdd per wave (wave_alloc).  The
// list's order therefore varies from run to run; nothing written does, since every record is keyed by the pixel carried
// in the state.
PRT_DEV void chain_vertex(bool live, uint32_t j, uint32_t pixel, uint32_t k, float L, f3 T, f3 d, const PrtChainArgs& a,
                          const PrtChainList& out) {
    bool follow = false;
    f3 nd = mk3(0.0f, 0.0f, 0.0f), np = nd, nT = T;
    float nL = L;
    if (live) {
        const PrtHit h = a.hits[j];
        float4 alb = make_float4(T.x, T.y, T.z, (float)k);
        float4 nr = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        float4 ps = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (h.prim >= 0) {
            const uint32_t t = a.mat_type[h.material_id];
            const float4 m = a.mat_rgbs[h.material_id];
            const f3 rgb = a.albedo ? mk3(a.albedo[3 * (size_t)j], a.albedo[3 * (size_t)j + 1], a.albedo[3 * (size_t)j + 2]) : mk3(m.x, m.y, m.z);
            const f3 N = mk3(h.normal[0], h.normal[1], h.normal[2]);
            const float seg = __builtin_sqrtf(h.d2);
            if (k < a.ft.max_specular) {
                if (t == (uint32_t)PRT_MAT_METAL && m.w <= a.ft.roughness_max) {
                    const f3 r = normalize3(normalize3(reflect3(d, N)));
                    if (dot3(r, N) > 0.0f && finite3(r)) {
                        follow = true;
                        nd = r;
                        nT = T * rgb;
                    }
                } else if (t == (uint32_t)PRT_MAT_DIELECTRIC) {
                    const float ri = h.front_face ? (1.0f / m.w) : m.w;
                    const float cos_theta = glm_min(dot3(-d, N), 1.0f);
                    const float sin_theta = __builtin_sqrtf(1.0f - cos_theta * cos_theta);
                    const bool cannot = ri * sin_theta > 1.0f;
                    const bool refl = cannot || fresnel_reflectance(cos_theta, ri) > 0.5f;
                    const f3 a_refl = reflect3(d, N);
                    const f3 a_refr = refract3(d, N, ri);
                    const f3 r = normalize3(mk3(refl ? a_refl.x : a_refr.x, refl ? a_refl.y : a_refr.y, refl ? a_refl.z : a_refr.z));
                    if (finite3(r)) {
                        follow = true;
                        nd = r;
                    }
                }
            }
            if (follow) {
                nL = L + seg;
                np = mk3(h.position[0], h.position[1], h.position[2]);
            } else {
                const bool coloured = t == (uint32_t)PRT_MAT_LAMBERTIAN || t == (uint32_t)PRT_MAT_METAL;
                const f3 av = T * (coloured ? rgb : mk3(1.0f, 1.0f, 1.0f));
                alb = make_float4(av.x, av.y, av.z, (float)k);
                nr = make_float4(N.x, N.y, N.z, __int_as_float(h.prim));
                ps = make_float4(h.position[0], h.position[1], h.position[2], L + seg);
            }
        }
        if (!follow) {
            a.guide.alb[pixel] = alb;
            a.guide.nrm[pixel] = nr;
            a.guide.pos[pixel] = ps;
        }
    }
    const uint32_t slot = wave_alloc(a.count, follow);
    if (follow) {
        const size_t s = 3 * (size_t)slot;
        out.o[s] = np.x;
        out.o[s + 1] = np.y;
        out.o[s + 2] = np.z;
        out.d[s] = nd.x;
        out.d[s + 1] = nd.y;
        out.d[s + 2] = nd.z;
        out.s0[slot] = make_float4(__uint_as_float(pixel), __uint_as_float(k + 1u), nL, 0.0f);
        out.s1[slot] = make_float4(nT.x, nT.y, nT.z, 0.0f);
    }
}

__global__ __launch_bounds__(256) void k_ft_start(uint32_t n, const float* __restrict__ dirs, PrtChainArgs a, PrtChainList out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n;
    f3 d = mk3(0.0f, 0.0f, 0.0f);
    if (live) d = mk3(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
    chain_vertex(live, i, i, 0u, 0.0f, mk3(1.0f, 1.0f, 1.0f), d, a, out);
}

__global__ __launch_bounds__(256) void k_ft_step(uint32_t n, PrtChainList in, PrtChainArgs a, PrtChainList out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const bool live = j < n;
    f3 d = mk3(0.0f, 0.0f, 0.0f), T = d;
    uint32_t pixel = 0u, k = 0u;
    float L = 0.0f;
    if (live) {
        const float4 s0 = in.s0[j], s1 = in.s1[j];
        pixel = __float_as_uint(s0.x);
        k = __float_as_uint(s0.y);
        L = s0.z;
        T = mk3(s1.x, s1.y, s1.z);
        d = mk3(in.d[3 * (size_t)j], in.d[3 * (size_t)j + 1], in.d[3 * (size_t)j + 2]);
    }
    chain_vertex(live, j, pixel, k, L, T, d, a, out);
}

}  // namespace

void prt_launch_ft_start(hipStream_t st, uint32_t n, const float* dirs, const PrtChainArgs& a, PrtChainList out) {
    hipLaunchKernelGGL(k_ft_start, dim3(blocks_for(n)), dim3(256), 0, st, n, dirs, a, out);
}

void prt_launch_ft_step(hipStream_t st, uint32_t n, PrtChainList in, const PrtChainArgs& a, PrtChainList out) {
    hipLaunchKernelGGL(k_ft_step, dim3(blocks_for(n)), dim3(256), 0, st, n, in, a, out);
}

// prt_bake_light.hip — the texel's light sample of surface baking (include/prt.h "Surface baking", the texel's light
// sample): the texel as the Lambertian vertex of albedo 1 it is, taking the light sample a render's vertex takes, and the
// pdf of its own ray for the lit query to weight what that ray meets.  A translation unit of its own: prt_bake.hip and
// prt_radiance_lit.hip keep their kernel sets.  Built with the flags of prt_kernels.hip: no contraction.  The light
// functions are the shade kernels' own (prt_light_device.h).
#include <hip/hip_runtime.h>

#include "prt_bake_light.h"
#include "prt_device.h"
#include "prt_light_device.h"

namespace {

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// k_rdl_step's light sample at the texel: key = the state before the texel's scatter draws, albedo and throughput 1.
template <bool MESHL, bool ENV, bool CLUS>
__global__ __launch_bounds__(256) void k_bkl_sample(uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const uint32_t* __restrict__ list,
                                                    PrtBakeMap m, const float* __restrict__ d, PrtBakeLightArgs A, PrtBakeLightRays out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= (uint64_t)cs * n) return;
    const uint32_t s_local = (uint32_t)(j / n);
    const uint32_t k = (uint32_t)(j - (uint64_t)s_local * n);
    const uint32_t t = list ? list[k] : k;
    f3 p = mk3(0.0f, 0.0f, 0.0f), w = p, contrib = p;
    float tmax = 0.0f, ray_pb = 0.0f;
    uint32_t light = 0xFFFFFFFFu;
    if (m.cov[t] != 0u) {
        p = mk3(m.position[3 * (size_t)t], m.position[3 * (size_t)t + 1], m.position[3 * (size_t)t + 2]);
        const f3 nn = mk3(m.normal[3 * (size_t)t], m.normal[3 * (size_t)t + 1], m.normal[3 * (size_t)t + 2]);
        const uint32_t key = path_seed(t, sample0 + s_local, seed);
        const f3 one = mk3(1.0f, 1.0f, 1.0f);
        LightSample ls;
        float pb = 0.0f, wl = 0.0f;
        f3 C = mk3(0.0f, 0.0f, 0.0f);
        bool have = false;
        if (ENV && (A.env.t_all | A.env.t_env) != 0u && env_selected(A.env, key)) {
            have = env_sample_term(A.env, A.lt.mode, nn, one, one, key, A.clamp, ls, pb, wl, C);
        } else if (A.lt.n_lights) {
            have = light_sample_term<MESHL, CLUS>(A.lt, p, nn, one, one, key, A.clamp, ls, pb, wl, C, &A.ml, &A.lc);
        }
        if (have) {
            w = ls.w;
            light = ls.light;
            if (pb > 0.0f) {
                tmax = ls.tmax;
                contrib = C;
            }
        }
        const f3 dd = mk3(d[3 * (size_t)j], d[3 * (size_t)j + 1], d[3 * (size_t)j + 2]);
        const float c = dot3(nn, dd);
        ray_pb = (c > 0.0f ? c : 0.0f) * PRT_INV_PI;
    }
    const size_t r = 3 * (size_t)j;
    if (out.x) {
        out.x[r] = p.x;
        out.x[r + 1] = p.y;
        out.x[r + 2] = p.z;
    }
    out.w[r] = w.x;
    out.w[r + 1] = w.y;
    out.w[r + 2] = w.z;
    out.tmax[j] = tmax;
    out.contrib[r] = contrib.x;
    out.contrib[r + 1] = contrib.y;
    out.contrib[r + 2] = contrib.z;
    if (out.light) out.light[j] = light;
    out.ray_pb[j] = ray_pb;
}

// The sample value fl(q + e): e = the contribution of a ray that was cast (tmax > 0) and is not occluded.  Every lane of a
// wave reaches the ballots (alive = false: a lane beyond the list).
__global__ __launch_bounds__(256) void k_bkl_add(uint32_t n, PrtBakeLightRays r, const uint8_t* __restrict__ occluded, float* __restrict__ rgb,
                                                 unsigned long long* __restrict__ stats) {
    const uint64_t j64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool alive = j64 < n;
    bool cast = false, occ = false;
    if (alive) {
        const size_t j = (size_t)j64;
        cast = r.tmax[j] > 0.0f;
        occ = cast && occluded[j] != 0u;
        if (cast && !occ) {
            rgb[3 * j] = rgb[3 * j] + r.contrib[3 * j];
            rgb[3 * j + 1] = rgb[3 * j + 1] + r.contrib[3 * j + 1];
            rgb[3 * j + 2] = rgb[3 * j + 2] + r.contrib[3 * j + 2];
        }
    }
    const unsigned long long mc = __ballot(cast), mo = __ballot(occ);
    if (lane_id() == 0u) {
        unsigned long long* s = stats + 2u * (blockIdx.x & (PRT_BKL_STAT_SLOTS - 1u));
        if (mc) atomicAdd(s, (unsigned long long)__popcll(mc));
        if (mo) atomicAdd(s + 1, (unsigned long long)__popcll(mo));
    }
}

}  // namespace

void prt_launch_bkl_sample(hipStream_t st, bool mesh, bool env, bool clus, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed,
                           const uint32_t* list, PrtBakeMap m, const float* d, const PrtBakeLightArgs& a, PrtBakeLightRays out) {
    const dim3 g(blocks_for((uint64_t)cs * n)), b(256);
    if (clus && mesh) {
        if (env) hipLaunchKernelGGL((k_bkl_sample<true, true, true>), g, b, 0, st, n, cs, sample0, seed, list, m, d, a, out);
        else hipLaunchKernelGGL((k_bkl_sample<true, false, true>), g, b, 0, st, n, cs, sample0, seed, list, m, d, a, out);
    } else if (mesh) {
        if (env) hipLaunchKernelGGL((k_bkl_sample<true, true, false>), g, b, 0, st, n, cs, sample0, seed, list, m, d, a, out);
        else hipLaunchKernelGGL((k_bkl_sample<true, false, false>), g, b, 0, st, n, cs, sample0, seed, list, m, d, a, out);
    } else {
        if (env) hipLaunchKernelGGL((k_bkl_sample<false, true, false>), g, b, 0, st, n, cs, sample0, seed, list, m, d, a, out);
        else hipLaunchKernelGGL((k_bkl_sample<false, false, false>), g, b, 0, st, n, cs, sample0, seed, list, m, d, a, out);
    }
}

void prt_launch_bkl_add(hipStream_t st, uint32_t n_rays, PrtBakeLightRays r, const uint8_t* occluded, float* rgb, unsigned long long* stats) {
    hipLaunchKernelGGL(k_bkl_add, dim3(blocks_for(n_rays)), dim3(256), 0, st, n_rays, r, occluded, rgb, stats);
}

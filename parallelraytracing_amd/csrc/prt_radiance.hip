// prt_radiance.hip — the device code of the radiance query (include/prt.h "Radiance query"): whole paths for rays the
// caller supplies.  A translation unit of its own: nothing in a batch route or in another unit's kernel set changes for it.
// Built with the flags of prt_kernels.hip: no contraction, so every line below is the IEEE operation it spells.  The vertex
// math is the shade kernels' own (prt_device.h): material_scatter, normalize3, rnd01, env_radiance; the order of operations
// is advance_path's (prt_kernels.hip), with the running L of the oracle's trace_iterative.
#include <hip/hip_runtime.h>

#include "prt_radiance.h"
#include "prt_device.h"

namespace {

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// The direction whose texel a miss of the caller's own segment reads (include/prt.h "Radiance query", Miss).  env_texel is
// written for unit directions and the caller's is used as given, so: l2 = fl((x*x + y*y) + z*z); |l2 - 1| > 2^-20: the
// normalised direction, else the direction as it is.  A direction normalised in fp32 has l2 within about 2^-22 of 1 and
// keeps its bits.  Every later segment's direction is normalised by the step.
__device__ inline f3 rd_first_lookup_dir(f3 d) {
    const float l2 = dot3(d, d);
    return __builtin_fabsf(l2 - 1.0f) > 9.5367431640625e-07f ? normalize3(d) : d;  // 2^-20
}

// The chunk's paths, sample-major.  The ray is copied per sample so that a round's list is what the ray-query pipeline
// packs from and the compaction moves ray and state together.
__global__ __launch_bounds__(256) void k_rd_start(uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* __restrict__ origins,
                                                  const float* __restrict__ dirs, const uint32_t* __restrict__ rng_state, PrtRadianceList out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= (uint64_t)cs * n) return;
    const uint32_t s_local = (uint32_t)(j / n);
    const uint32_t i = (uint32_t)(j - (uint64_t)s_local * n);
    const uint32_t rng = rng_state ? rng_state[i] : path_seed(i, sample0 + s_local, seed);
    const size_t r = 3 * (size_t)i, w = 3 * (size_t)j;
    out.o[w] = origins[r];
    out.o[w + 1] = origins[r + 1];
    out.o[w + 2] = origins[r + 2];
    out.d[w] = dirs[r];
    out.d[w + 1] = dirs[r + 1];
    out.d[w + 2] = dirs[r + 2];
    out.s0[j] = make_float4(__uint_as_float((uint32_t)j), __uint_as_float(rng), 1.0f, 1.0f);
    out.s1[j] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
}

// One segment of every live path.  Every lane of the wave reaches the append (live = false: a lane beyond the list),
// because it is a stream compaction: ballot of "goes on", rank = popcount below the lane, one integer atomicAdd per wave
// (wave_alloc).  The list's order therefore varies from run to run; nothing written does, since every record is keyed by
// the slot carried in the state.
__global__ __launch_bounds__(256) void k_rd_step(uint32_t n, PrtRadianceList in, PrtRadianceArgs a, PrtRadianceList out) {
    const uint64_t j64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;  // (n may be within a block of 2^32)
    const bool live = j64 < n;
    const uint32_t j = (uint32_t)j64;
    bool goes_on = false;
    uint32_t slot = 0u, rng = 0u;
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = o, thr = o, L = o;
    if (live) {
        const float4 s0 = in.s0[j], s1 = in.s1[j];
        slot = __float_as_uint(s0.x);
        rng = __float_as_uint(s0.y);
        thr = mk3(s0.z, s0.w, s1.x);
        L = mk3(s1.y, s1.z, s1.w);
        d = mk3(in.d[3 * (size_t)j], in.d[3 * (size_t)j + 1], in.d[3 * (size_t)j + 2]);
        const PrtHit h = a.hits[j];
        if (h.prim < 0) {  // a miss: the environment image's texel, or the constant sky
            L = L + thr * (a.env.W ? env_radiance(a.env, a.round == 0u ? rd_first_lookup_dir(d) : d) : mk3(a.sky[0], a.sky[1], a.sky[2]));
        } else {
            const uint32_t type = a.mat_type[h.material_id];
            float4 rgbs = a.mat_rgbs[h.material_id];
            if (a.albedo) {
                rgbs.x = a.albedo[3 * (size_t)j];
                rgbs.y = a.albedo[3 * (size_t)j + 1];
                rgbs.z = a.albedo[3 * (size_t)j + 2];
            }
            f3 atten, emitted, so, sd;
            const bool scattered = material_scatter(type, rgbs, d, mk3(h.position[0], h.position[1], h.position[2]),
                                                    mk3(h.normal[0], h.normal[1], h.normal[2]), h.front_face != 0u, rng, atten, emitted, so, sd);
            L = L + thr * emitted;
            if (scattered) {
                thr = thr * atten;
                o = so;
                d = normalize3(sd);
                goes_on = a.round + 1u < a.max_depth;
                if (goes_on && a.sp.rr_depth != 0u && a.round + 1u >= a.sp.rr_depth) {  // Russian roulette (PrtSampling)
                    float p = thr.x > thr.y ? thr.x : thr.y;
                    p = p > thr.z ? p : thr.z;
                    p = p > 1.0f ? 1.0f : p;
                    p = p < 0.05f ? 0.05f : p;
                    goes_on = rnd01(rng) < p;
                    thr = mk3(thr.x / p, thr.y / p, thr.z / p);
                }
            }
        }
        if (!goes_on) {
            const float c = a.sp.clamp;
            if (c > 0.0f) {
                L.x = L.x > c ? c : L.x;
                L.y = L.y > c ? c : L.y;
                L.z = L.z > c ? c : L.z;
            }
            a.slots[slot] = make_float4(L.x, L.y, L.z, __uint_as_float(a.round + 1u));
            if (a.rng_out) a.rng_out[slot] = rng;
        }
    }
    const uint32_t k = wave_alloc(a.count, goes_on);
    if (goes_on) {
        const size_t w = 3 * (size_t)k;
        out.o[w] = o.x;
        out.o[w + 1] = o.y;
        out.o[w + 2] = o.z;
        out.d[w] = d.x;
        out.d[w + 1] = d.y;
        out.d[w + 2] = d.z;
        out.s0[k] = make_float4(__uint_as_float(slot), __uint_as_float(rng), thr.x, thr.y);
        out.s1[k] = make_float4(thr.z, L.x, L.y, L.z);
    }
}

// Ray i's slots in ascending sample order: the sum does not depend on where the compaction put anything.
__global__ __launch_bounds__(256) void k_rd_sum(uint32_t n, uint32_t cs, uint32_t first, const float4* __restrict__ slots, float* __restrict__ rgb_sum,
                                                uint32_t* __restrict__ segments) {
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    const size_t r = 3 * (size_t)i;
    f3 acc = first ? mk3(0.0f, 0.0f, 0.0f) : mk3(rgb_sum[r], rgb_sum[r + 1], rgb_sum[r + 2]);
    uint32_t seg = (first || !segments) ? 0u : segments[i];
    for (uint32_t s = 0; s < cs; ++s) {
        const float4 v = ld_stream(slots + ((size_t)s * n + i));
        acc = acc + mk3(v.x, v.y, v.z);
        seg += __float_as_uint(v.w);
    }
    rgb_sum[r] = acc.x;
    rgb_sum[r + 1] = acc.y;
    rgb_sum[r + 2] = acc.z;
    if (segments) segments[i] = seg;
}

}  // namespace

void prt_launch_rd_start(hipStream_t st, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* origins,
                         const float* dirs, const uint32_t* rng_state, PrtRadianceList out) {
    hipLaunchKernelGGL(k_rd_start, dim3(blocks_for((uint64_t)cs * n)), dim3(256), 0, st, n, cs, sample0, seed, origins, dirs, rng_state, out);
}

void prt_launch_rd_step(hipStream_t st, uint32_t n, PrtRadianceList in, const PrtRadianceArgs& a, PrtRadianceList out) {
    hipLaunchKernelGGL(k_rd_step, dim3(blocks_for(n)), dim3(256), 0, st, n, in, a, out);
}

void prt_launch_rd_sum(hipStream_t st, uint32_t n, uint32_t cs, bool first, const float4* slots, float* rgb_sum, uint32_t* segments) {
    hipLaunchKernelGGL(k_rd_sum, dim3(blocks_for(n)), dim3(256), 0, st, n, cs, first ? 1u : 0u, slots, rgb_sum, segments);
}

// prt_radiance_lit.hip — the device code of the light-sampled radiance query (include/prt.h "Radiance query",
// prt_radiance_lit): prt_radiance.hip's paths, draw for draw, carrying what advance_path_nee (prt_kernels.hip) carries: one
// light sample per Lambertian vertex and the MIS weight of what the scattered segment meets.  A translation unit of its
// own: no kernel of another unit changes for it.  Built with the flags of prt_kernels.hip: no contraction.  The light
// functions are the shade kernels' own (prt_light_device.h).
#include <hip/hip_runtime.h>

#include "prt_radiance_lit.h"
#include "prt_device.h"
#include "prt_light_device.h"

namespace {

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// prt_radiance.hip's rd_first_lookup_dir: the direction whose texel a miss of the caller's own segment reads.
// l2 = fl((x*x + y*y) + z*z); |l2 - 1| > 2^-20: the normalised direction, else the direction as it is.
__device__ inline f3 rdl_first_lookup_dir(f3 d) {
    const float l2 = dot3(d, d);
    return __builtin_fabsf(l2 - 1.0f) > 9.5367431640625e-07f ? normalize3(d) : d;  // 2^-20
}

// k_rd_start, and pb = -1: the caller's ray was scattered by no vertex; or pb[i], the pdf of the caller's own Lambertian
// scatter along ray i (prt_radiance_lit_pb), for every sample of the ray.
__global__ __launch_bounds__(256) void k_rdl_start(uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* __restrict__ origins,
                                                   const float* __restrict__ dirs, const uint32_t* __restrict__ rng_state,
                                                   const float* __restrict__ pb, PrtRadianceLitList out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= (uint64_t)cs * n) return;
    const uint32_t s_local = (uint32_t)(j / n);
    const uint32_t i = (uint32_t)(j - (uint64_t)s_local * n);
    const uint32_t rng = rng_state ? rng_state[i] : path_seed(i, sample0 + s_local, seed);
    const size_t r = 3 * (size_t)i, w = 3 * (size_t)j;
    out.l.o[w] = origins[r];
    out.l.o[w + 1] = origins[r + 1];
    out.l.o[w + 2] = origins[r + 2];
    out.l.d[w] = dirs[r];
    out.l.d[w + 1] = dirs[r + 1];
    out.l.d[w + 2] = dirs[r + 2];
    out.l.s0[j] = make_float4(__uint_as_float((uint32_t)j), __uint_as_float(rng), 1.0f, 1.0f);
    out.l.s1[j] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    out.pb[j] = pb ? pb[i] : -1.0f;
}

// One segment of every live path: k_rd_step's, in its order, plus the weights and the light sample of advance_path_nee.
// Two stream compactions, survivors and shadow rays; every lane of the wave reaches both (live = false: a lane beyond
// the list).  A path may cast a shadow ray and lose its roulette in the same step, so a shadow record is keyed by the
// slot, not by a list position.
template <bool MESHL, bool ENV, bool CLUS>
__global__ __launch_bounds__(256) void k_rdl_step(uint32_t n, PrtRadianceLitList in, PrtRadianceLitArgs A, PrtRadianceLitList out) {
    const PrtRadianceArgs& a = A.a;
    const uint64_t j64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;  // (n may be within a block of 2^32)
    const bool live = j64 < n;
    const uint32_t j = (uint32_t)j64;
    bool goes_on = false, shadow = false;
    uint32_t slot = 0u, rng = 0u;
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = o, thr = o, L = o;
    f3 sx = o, sw = o, scontrib = o;
    float stmax = 0.0f, pb_next = -1.0f;
    if (live) {
        const float4 s0 = in.l.s0[j], s1 = in.l.s1[j];
        slot = __float_as_uint(s0.x);
        rng = __float_as_uint(s0.y);
        thr = mk3(s0.z, s0.w, s1.x);
        L = mk3(s1.y, s1.z, s1.w);
        o = mk3(in.l.o[3 * (size_t)j], in.l.o[3 * (size_t)j + 1], in.l.o[3 * (size_t)j + 2]);
        d = mk3(in.l.d[3 * (size_t)j], in.l.d[3 * (size_t)j + 1], in.l.d[3 * (size_t)j + 2]);
        const float pb_prev = in.pb[j];
        const PrtHit h = a.hits[j];
        if (h.prim < 0) {  // a miss: the environment's texel, weighted after a Lambertian vertex, or the constant sky
            if (ENV) {
                float wb;
                f3 term = thr * env_miss(a.env, A.lt.mode, a.round == 0u ? rdl_first_lookup_dir(d) : d, pb_prev, wb);
                if (wb != 1.0f) term = term * wb;
                L = L + term;
            } else {
                L = L + thr * mk3(a.sky[0], a.sky[1], a.sky[2]);
            }
        } else {
            const uint32_t type = a.mat_type[h.material_id];
            float4 rgbs = a.mat_rgbs[h.material_id];
            if (a.albedo) {
                rgbs.x = a.albedo[3 * (size_t)j];
                rgbs.y = a.albedo[3 * (size_t)j + 1];
                rgbs.z = a.albedo[3 * (size_t)j + 2];
            }
            const f3 x = mk3(h.position[0], h.position[1], h.position[2]), nrm = mk3(h.normal[0], h.normal[1], h.normal[2]);
            const uint32_t key = rng;  // the path's state at the vertex
            f3 atten, emitted, so, sd;
            const bool scattered = material_scatter(type, rgbs, d, x, nrm, h.front_face != 0u, rng, atten, emitted, so, sd);
            f3 term = thr * emitted;
            if (type == 4u && pb_prev >= 0.0f && (MESHL || (uint32_t)h.prim < A.n_prims)) {
                const float wb = bsdf_hit_weight<MESHL, CLUS>(A.lt, (uint32_t)h.prim, o, d, h.d2, pb_prev, &A.ml, A.n_prims, &A.lc);
                if (wb != 1.0f) term = term * wb;
            }
            L = L + term;
            if (scattered) {
                if (type == 1u && a.round + 1u < a.max_depth) {  // the light sample, with thr before this vertex's attenuation
                    const f3 albedo = mk3(rgbs.x, rgbs.y, rgbs.z);
                    LightSample ls;
                    float pb, wl;
                    if (ENV && (a.env.t_all | a.env.t_env) != 0u && env_selected(a.env, key)) {
                        if (env_sample_term(a.env, A.lt.mode, nrm, albedo, thr, key, a.sp.clamp, ls, pb, wl, scontrib) && pb > 0.0f) {
                            shadow = true;
                            sw = ls.w;
                            stmax = ls.tmax;
                        }
                    } else if (A.lt.n_lights) {
                        if (light_sample_term<MESHL, CLUS>(A.lt, x, nrm, albedo, thr, key, a.sp.clamp, ls, pb, wl, scontrib, &A.ml, &A.lc) &&
                            pb > 0.0f) {
                            shadow = true;
                            sw = ls.w;
                            stmax = ls.tmax;
                        }
                    }
                    sx = x;
                }
                thr = thr * atten;
                o = so;
                d = normalize3(sd);
                if (type == 1u) {
                    const float c = dot3(nrm, d);
                    pb_next = (c > 0.0f ? c : 0.0f) * PRT_INV_PI;
                }
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
        out.l.o[w] = o.x;
        out.l.o[w + 1] = o.y;
        out.l.o[w + 2] = o.z;
        out.l.d[w] = d.x;
        out.l.d[w + 1] = d.y;
        out.l.d[w + 2] = d.z;
        out.l.s0[k] = make_float4(__uint_as_float(slot), __uint_as_float(rng), thr.x, thr.y);
        out.l.s1[k] = make_float4(thr.z, L.x, L.y, L.z);
        out.pb[k] = pb_next;
    }
    const uint32_t ks = wave_alloc(A.scount, shadow);
    if (shadow) {
        const size_t w = 3 * (size_t)ks;
        A.sh.x[w] = sx.x;
        A.sh.x[w + 1] = sx.y;
        A.sh.x[w + 2] = sx.z;
        A.sh.w[w] = sw.x;
        A.sh.w[w + 1] = sw.y;
        A.sh.w[w + 2] = sw.z;
        A.sh.tmax[ks] = stmax;
        A.sh.cs[ks] = make_float4(scontrib.x, scontrib.y, scontrib.z, __uint_as_float(slot));
    }
}

// After the occlusion pipeline: every unoccluded shadow ray adds its contribution to its slot's light sum.  At most one
// shadow ray per slot per round, and the rounds are serial on the stream: no atomics, and the sum runs in vertex order.
// Every thread reaches both barriers (alive = false: a thread beyond the list).
__global__ __launch_bounds__(256) void k_rdl_light(uint32_t n, PrtRadianceShadowList sh, const uint8_t* __restrict__ occluded,
                                                   float4* __restrict__ lsum, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_n[2];
    if (threadIdx.x < 2u) s_n[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t k64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool alive = k64 < n;
    bool occ = false;
    if (alive) {
        const uint32_t k = (uint32_t)k64;
        occ = occluded[k] != 0u;
        if (!occ) {
            const float4 c = sh.cs[k];
            float4* p = &lsum[__float_as_uint(c.w)];
            float4 v = *p;
            v.x = v.x + c.x;
            v.y = v.y + c.y;
            v.z = v.z + c.z;
            *p = v;
        }
    }
    const unsigned long long mn = __ballot(alive), mo = __ballot(occ);
    if (lane_id() == 0u) {
        atomicAdd(&s_n[0], (uint32_t)__popcll(mn));
        atomicAdd(&s_n[1], (uint32_t)__popcll(mo));
    }
    __syncthreads();
    if (threadIdx.x < 2u && s_n[threadIdx.x])
        atomicAdd(&stats[2u * (blockIdx.x & (PRT_RDL_STAT_SLOTS - 1u)) + threadIdx.x], (unsigned long long)s_n[threadIdx.x]);
}

// k_rd_sum with the lit sample value: the clamped path radiance plus the slot's light sum, one add per component.
__global__ __launch_bounds__(256) void k_rdl_sum(uint32_t n, uint32_t cs, uint32_t first, const float4* __restrict__ slots,
                                                 const float4* __restrict__ lsum, float* __restrict__ rgb_sum, uint32_t* __restrict__ segments) {
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    const size_t r = 3 * (size_t)i;
    f3 acc = first ? mk3(0.0f, 0.0f, 0.0f) : mk3(rgb_sum[r], rgb_sum[r + 1], rgb_sum[r + 2]);
    uint32_t seg = (first || !segments) ? 0u : segments[i];
    for (uint32_t s = 0; s < cs; ++s) {
        const float4 v = ld_stream(slots + ((size_t)s * n + i));
        const float4 l = ld_stream(lsum + ((size_t)s * n + i));
        acc = acc + (mk3(v.x, v.y, v.z) + mk3(l.x, l.y, l.z));
        seg += __float_as_uint(v.w);
    }
    rgb_sum[r] = acc.x;
    rgb_sum[r + 1] = acc.y;
    rgb_sum[r + 2] = acc.z;
    if (segments) segments[i] = seg;
}

}  // namespace

void prt_launch_rdl_start(hipStream_t st, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* origins,
                          const float* dirs, const uint32_t* rng_state, const float* pb, PrtRadianceLitList out) {
    hipLaunchKernelGGL(k_rdl_start, dim3(blocks_for((uint64_t)cs * n)), dim3(256), 0, st, n, cs, sample0, seed, origins, dirs, rng_state, pb, out);
}

void prt_launch_rdl_step(hipStream_t st, bool mesh, bool env, bool clus, uint32_t n, PrtRadianceLitList in, const PrtRadianceLitArgs& a,
                         PrtRadianceLitList out) {
    const dim3 g(blocks_for(n)), b(256);
    if (clus && mesh) {
        if (env) hipLaunchKernelGGL((k_rdl_step<true, true, true>), g, b, 0, st, n, in, a, out);
        else hipLaunchKernelGGL((k_rdl_step<true, false, true>), g, b, 0, st, n, in, a, out);
    } else if (mesh) {
        if (env) hipLaunchKernelGGL((k_rdl_step<true, true, false>), g, b, 0, st, n, in, a, out);
        else hipLaunchKernelGGL((k_rdl_step<true, false, false>), g, b, 0, st, n, in, a, out);
    } else {
        if (env) hipLaunchKernelGGL((k_rdl_step<false, true, false>), g, b, 0, st, n, in, a, out);
        else hipLaunchKernelGGL((k_rdl_step<false, false, false>), g, b, 0, st, n, in, a, out);
    }
}

void prt_launch_rdl_light(hipStream_t st, uint32_t n, PrtRadianceShadowList sh, const uint8_t* occluded, float4* lsum,
                          unsigned long long* stats) {
    hipLaunchKernelGGL(k_rdl_light, dim3(blocks_for(n)), dim3(256), 0, st, n, sh, occluded, lsum, stats);
}

void prt_launch_rdl_sum(hipStream_t st, uint32_t n, uint32_t cs, bool first, const float4* slots, const float4* lsum, float* rgb_sum,
                        uint32_t* segments) {
    hipLaunchKernelGGL(k_rdl_sum, dim3(blocks_for(n)), dim3(256), 0, st, n, cs, first ? 1u : 0u, slots, lsum, rgb_sum, segments);
}

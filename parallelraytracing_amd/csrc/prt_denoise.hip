// prt_denoise.hip — the device code of the feature pass and of the edge-avoiding a-trous film denoiser (include/prt.h
// "First-hit feature images and the edge-avoiding film denoiser").  A translation unit of its own: nothing in
// prt_kernels.hip changes for it.  Built with the flags of prt_kernels.hip: no contraction, so every line below is the
// IEEE operation it spells, and tests/denoise_replay.py restates them in numpy float32.
#include <hip/hip_runtime.h>

#include "prt_denoise.h"
#include "prt_denoise_contract.h"

namespace {

constexpr float kRhoMin = 0.015625f;                    // 2^-6
constexpr float kEpsL = 9.5367431640625e-07f;           // 2^-20
constexpr float kTiny = 7.888609052210118e-31f;         // 2^-100
constexpr float kWMin = 9.313225746154785e-10f;         // 2^-30

inline uint32_t blocks_for(uint32_t n) { return (n + 255u) / 256u; }

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// rho of a pixel: max(albedo, RHO_MIN) per channel, (1, 1, 1) for a miss
__device__ __forceinline__ float4 dn_rho(float4 alb, float4 nrm) {
    if (__float_as_int(nrm.w) < 0) return make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    return make_float4(fmaxf(alb.x, kRhoMin), fmaxf(alb.y, kRhoMin), fmaxf(alb.z, kRhoMin), 0.0f);
}

__device__ __forceinline__ float4 dn_start(float r, float g, float b, float var, float4 alb, float4 nrm, uint32_t demodulate) {
    if (!demodulate) return make_float4(r, g, b, var);
    const float4 rho = dn_rho(alb, nrm);
    const float lr = dn_lum(rho.x, rho.y, rho.z);
    return make_float4(r / rho.x, g / rho.y, b / rho.z, var / (lr * lr));
}

__global__ void k_dn_pixel_grid(uint32_t W, uint32_t n, float* __restrict__ px, float* __restrict__ py) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    px[i] = (float)(i % W) + 0.5f;
    py[i] = (float)(i / W) + 0.5f;
}

__global__ void k_dn_pack_features(uint32_t n, const PrtHit* __restrict__ hits, const float* __restrict__ albedo,
                                   const float4* __restrict__ mat_rgbs, const uint32_t* __restrict__ mat_type,
                                   float4* __restrict__ o_alb, float4* __restrict__ o_nrm, float4* __restrict__ o_pos) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const PrtHit h = hits[i];
    float4 a = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    float4 nr = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    float4 ps = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (h.prim >= 0) {
        const uint32_t t = mat_type[h.material_id];
        if (t == (uint32_t)PRT_MAT_LAMBERTIAN || t == (uint32_t)PRT_MAT_METAL) {
            if (albedo) {
                a = make_float4(albedo[3 * (size_t)i], albedo[3 * (size_t)i + 1], albedo[3 * (size_t)i + 2], 0.0f);
            } else {
                const float4 m = mat_rgbs[h.material_id];
                a = make_float4(m.x, m.y, m.z, 0.0f);
            }
        }
        nr = make_float4(h.normal[0], h.normal[1], h.normal[2], __int_as_float(h.prim));
        ps = make_float4(h.position[0], h.position[1], h.position[2], sqrtf(h.d2));
    }
    o_alb[i] = a;
    o_nrm[i] = nr;
    o_pos[i] = ps;
}

__global__ void k_dn_pack_arrays(uint32_t n, const float* __restrict__ albedo, const float* __restrict__ normal,
                                 const float* __restrict__ position, const int32_t* __restrict__ prim, float4* __restrict__ o_alb,
                                 float4* __restrict__ o_nrm, float4* __restrict__ o_pos) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t j = 3 * (size_t)i;
    o_alb[i] = make_float4(albedo[j], albedo[j + 1], albedo[j + 2], 0.0f);
    o_nrm[i] = make_float4(normal[j], normal[j + 1], normal[j + 2], __int_as_float(prim[i]));
    o_pos[i] = make_float4(position[j], position[j + 1], position[j + 2], 0.0f);
}

__global__ void k_dn_prepare(uint32_t n, const float* __restrict__ mean, const float* __restrict__ var, const float4* __restrict__ alb,
                             const float4* __restrict__ nrm, uint32_t demodulate, float4* __restrict__ cv) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t j = 3 * (size_t)i;
    cv[i] = dn_start(mean[j], mean[j + 1], mean[j + 2], var[i], alb[i], nrm[i], demodulate);
}

// The context's own film (world_size 1: local tile = global tile) in Film layout, read only.
__global__ void k_dn_film_prepare(uint32_t W, uint32_t H, uint32_t tiles_x, const float4* __restrict__ film_local,
                                  const float2* __restrict__ film_stat, const float4* __restrict__ alb, const float4* __restrict__ nrm,
                                  uint32_t demodulate, float4* __restrict__ cv) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= W * H) return;
    const uint32_t x = i % W, y = i / W;
    const uint32_t pl = ((y >> 3) * tiles_x + (x >> 3)) * 64u + ((y & 7u) << 3) + (x & 7u);
    const float4 f = film_local[pl];
    const float2 s = film_stat[pl];
    const float r = prt_denoise_mean_rule(f.x, f.w), g = prt_denoise_mean_rule(f.y, f.w), b = prt_denoise_mean_rule(f.z, f.w);
    cv[i] = dn_start(r, g, b, prt_denoise_variance_rule(f.w, s.x, s.y), alb[i], nrm[i], demodulate);
}

// One a-trous iteration.  Block = 64 x 4 threads: a wave takes 64 consecutive pixels of one row, so a tap's offset
// s (dx, dy) is wave-uniform, every record load of a tap is one coalesced 1-KB access whatever the step, and the row
// test of a tap is wave-uniform too; only the column test at the image's sides and the hit / miss cases diverge.
// 25 taps x {colour + variance, normal + prim, position} = 25 x 48 B per pixel, the centre's records and the 3 x 3
// variance prefilter come from lines the taps touch anyway.  The loops are unrolled (the tap weights are immediates):
// no scratch.
// LDS = true (steps 1 and 2 only): the block first stages the records of its footprint, (64 + 4 s) x (4 + 4 s) pixels, in
// LDS and the taps read them there.  The same values go through the same operations in the same order: not a bit of the
// output changes.  Measured on an MI355X (tools/denoise_rate.py, DESIGN.md section 3 "Denoising"): faster at step 1, where a
// block reads each record of its footprint 25 x 256 / 544 = 11.8 times, slower at step 2 (7.4 times, 41 KB of LDS a block),
// so only step 1 takes it by default.
template <bool LDS>
__global__ void __launch_bounds__(256) k_dn_atrous(PrtAtrousParams p, const float4* __restrict__ cv_in, const float4* __restrict__ nrm,
                                                   const float4* __restrict__ pos, float4* __restrict__ cv_out) {
    extern __shared__ float4 s_dn[];
    const int W = (int)p.W, H = (int)p.H, s = (int)p.step;
    const int FW = 64 + 4 * s, FH = 4 + 4 * s;                              // the block's footprint
    const int fx0 = (int)(blockIdx.x * 64u) - 2 * s, fy0 = (int)(blockIdx.y * 4u) - 2 * s;
    float4* s_cv = s_dn;
    float4* s_nr = s_dn + FW * FH;
    float4* s_ps = s_dn + 2 * FW * FH;
    if (LDS) {
        for (int k = (int)(threadIdx.y * 64u + threadIdx.x); k < FW * FH; k += 256) {
            const int gx = fx0 + k % FW, gy = fy0 + k / FW;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {                   // (a slot outside the image is never read)
                const uint32_t ig = (uint32_t)gy * p.W + (uint32_t)gx;
                s_cv[k] = cv_in[ig];
                s_nr[k] = nrm[ig];
                s_ps[k] = pos[ig];
            }
        }
        __syncthreads();
    }
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
    if (x >= p.W || y >= p.H) return;
    const uint32_t ip = y * p.W + x;
    // a pixel (xx, yy) of the image within the footprint: its slot in LDS, or its index in the image
    auto at = [&](int xx, int yy) -> uint32_t { return LDS ? (uint32_t)((yy - fy0) * FW + (xx - fx0)) : (uint32_t)yy * p.W + (uint32_t)xx; };
    const float4* cvs = LDS ? s_cv : cv_in;
    const float4* nrs = LDS ? s_nr : nrm;
    const float4* pss = LDS ? s_ps : pos;
    // variance prefilter: 3 x 3 at step 1 over the pixels in the image, row-major
    float num = 0.0f, ksum = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = (int)y + dy;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = (int)x + dx;
            if (xx < 0 || xx >= W) continue;
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            num += k * cvs[at(xx, yy)].w;
            ksum += k;
        }
    }
    const float g = num / ksum;
    const float den = p.sigma_l * sqrtf(g) + kEpsL;

    const uint32_t jp = at((int)x, (int)y);
    const float4 cp = cvs[jp], np = nrs[jp], pp = pss[jp];
    const bool hit_p = __float_as_int(np.w) >= 0;
    const float lp = dn_lum(cp.x, cp.y, cp.z);
    float Sw = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, Sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = (int)y + dy * s;
        if (yy < 0 || yy >= H) continue;
        const float ky = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = (int)x + dx * s;
            if (xx < 0 || xx >= W) continue;
            const float kx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
            const float h = ky * kx;
            const uint32_t iq = at(xx, yy);
            const float4 cq = cvs[iq];
            float w;
            if (dy == 0 && dx == 0) {
                w = h;
            } else {
                const float4 nq = nrs[iq];
                const bool hit_q = __float_as_int(nq.w) >= 0;
                if (hit_p != hit_q) {
                    w = 0.0f;
                } else {
                    float wn = 1.0f, xz = 0.0f;
                    if (hit_p) {
                        const float4 pq = pss[iq];
                        wn = fmaxf(0.0f, (np.x * nq.x + np.y * nq.y) + np.z * nq.z);
                        for (uint32_t k = 0; k < p.normal_power_log2; ++k) wn = wn * wn;
                        const float Dx = pq.x - pp.x, Dy = pq.y - pp.y, Dz = pq.z - pp.z;
                        const float dn = (Dx * np.x + Dy * np.y) + Dz * np.z;
                        const float dd = (Dx * Dx + Dy * Dy) + Dz * Dz;
                        xz = fabsf(dn) / (p.sigma_z * sqrtf(dd) + kTiny);
                    }
                    const float xl = fabsf(lp - dn_lum(cq.x, cq.y, cq.z)) / den;
                    const float xs = xl + xz;
                    w = (h * wn) / ((1.0f + xs) + (0.5f * xs) * xs);
                    if (w < kWMin) w = 0.0f;
                }
            }
            Sw += w;
            Sr += w * cq.x;
            Sg += w * cq.y;
            Sb += w * cq.z;
            Sv += (w * w) * cq.w;
        }
    }
    cv_out[ip] = make_float4(Sr / Sw, Sg / Sw, Sb / Sw, Sv / (Sw * Sw));
}

__global__ void k_dn_finish(uint32_t n, const float4* __restrict__ cv, const float4* __restrict__ alb, const float4* __restrict__ nrm,
                            uint32_t demodulate, float* __restrict__ out, float* __restrict__ var_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 c = cv[i];
    if (demodulate) {
        const float4 rho = dn_rho(alb[i], nrm[i]);
        const float lr = dn_lum(rho.x, rho.y, rho.z);
        c = make_float4(c.x * rho.x, c.y * rho.y, c.z * rho.z, c.w * (lr * lr));
    }
    const size_t j = 3 * (size_t)i;
    out[j] = c.x;
    out[j + 1] = c.y;
    out[j + 2] = c.z;
    if (var_out) var_out[i] = c.w;
}

}  // namespace

void prt_launch_dn_pixel_grid(hipStream_t st, uint32_t W, uint32_t H, float* px, float* py) {
    const uint32_t n = W * H;
    hipLaunchKernelGGL(k_dn_pixel_grid, dim3(blocks_for(n)), dim3(256), 0, st, W, n, px, py);
}

void prt_launch_dn_pack_features(hipStream_t st, uint32_t n, const PrtHit* hits, const float* albedo, const float4* mat_rgbs,
                                 const uint32_t* mat_type, PrtFeatureBufs out) {
    hipLaunchKernelGGL(k_dn_pack_features, dim3(blocks_for(n)), dim3(256), 0, st, n, hits, albedo, mat_rgbs, mat_type, out.alb, out.nrm,
                       out.pos);
}

void prt_launch_dn_pack_arrays(hipStream_t st, uint32_t n, const float* albedo, const float* normal, const float* position,
                               const int32_t* prim, PrtFeatureBufs out) {
    hipLaunchKernelGGL(k_dn_pack_arrays, dim3(blocks_for(n)), dim3(256), 0, st, n, albedo, normal, position, prim, out.alb, out.nrm,
                       out.pos);
}

void prt_launch_dn_prepare(hipStream_t st, uint32_t n, const float* mean, const float* var, PrtFeatureBufs f, uint32_t demodulate,
                           float4* cv) {
    hipLaunchKernelGGL(k_dn_prepare, dim3(blocks_for(n)), dim3(256), 0, st, n, mean, var, f.alb, f.nrm, demodulate, cv);
}

void prt_launch_dn_film_prepare(hipStream_t st, const PrtTileMap& tm, const float4* film_local, const float2* film_stat,
                                PrtFeatureBufs f, uint32_t demodulate, float4* cv) {
    hipLaunchKernelGGL(k_dn_film_prepare, dim3(blocks_for(tm.W * tm.H)), dim3(256), 0, st, tm.W, tm.H, tm.tiles_x, film_local, film_stat,
                       f.alb, f.nrm, demodulate, cv);
}

void prt_launch_dn_atrous(hipStream_t st, const PrtAtrousParams& p, const float4* cv_in, PrtFeatureBufs f, float4* cv_out) {
    hipLaunchKernelGGL(k_dn_atrous<false>, dim3((p.W + 63u) / 64u, (p.H + 3u) / 4u), dim3(64, 4), 0, st, p, cv_in, f.nrm, f.pos, cv_out);
}

bool prt_launch_dn_atrous_lds(hipStream_t st, const PrtAtrousParams& p, const float4* cv_in, PrtFeatureBufs f, float4* cv_out) {
    if (p.step != 1u && p.step != 2u) return false;
    const size_t bytes = 3 * (size_t)(64u + 4u * p.step) * (4u + 4u * p.step) * sizeof(float4);   // 26 112 / 41 472 B
    hipLaunchKernelGGL(k_dn_atrous<true>, dim3((p.W + 63u) / 64u, (p.H + 3u) / 4u), dim3(64, 4), bytes, st, p, cv_in, f.nrm, f.pos, cv_out);
    return true;
}

void prt_launch_dn_finish(hipStream_t st, uint32_t n, const float4* cv, PrtFeatureBufs f, uint32_t demodulate, float* out,
                          float* var_out) {
    const uint32_t blocks = blocks_for(n);
    hipLaunchKernelGGL(k_dn_finish, dim3(blocks), dim3(256), 0, st, n, cv, f.alb, f.nrm, demodulate, out, var_out);
}

// prt_bake.hip — the device code of surface baking (include/prt.h "Surface baking"): from a mesh's UV layout to the rays
// of its texels, and from the radiance query's per-ray results back to the map.  A translation unit of its own: nothing
// in a batch route or in another unit's kernel set changes for it.  Built with the flags of prt_kernels.hip: no
// contraction, so every line below is the IEEE operation it spells.  The coverage rule is evaluated in double on the UVs
// widened from fp32; everything after the barycentrics is fp32 and the shade kernels' own (prt_device.h): transform_point,
// transform_normal, material_scatter, normalize3, path_seed.
#include <hip/hip_runtime.h>

#include "prt_bake.h"
#include "prt_device.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// One face's UV triangle, widened to double, and twice its signed area.
struct BkFace {
    double ax, ay, bx, by, cx, cy, A2;
};

// False: the face covers nothing (a non-finite UV, or no area).
__device__ inline bool bk_face(const float* __restrict__ uv, uint32_t f, BkFace& e) {
    const float* u = uv + 6 * (size_t)f;
    const float u0 = u[0], u1 = u[1], u2 = u[2], u3 = u[3], u4 = u[4], u5 = u[5];
    const bool finite = __builtin_isfinite(u0) && __builtin_isfinite(u1) && __builtin_isfinite(u2) && __builtin_isfinite(u3) &&
                        __builtin_isfinite(u4) && __builtin_isfinite(u5);
    e.ax = (double)u0;
    e.ay = (double)u1;
    e.bx = (double)u2;
    e.by = (double)u3;
    e.cx = (double)u4;
    e.cy = (double)u5;
    e.A2 = (e.bx - e.ax) * (e.cy - e.ay) - (e.by - e.ay) * (e.cx - e.ax);
    return finite && e.A2 != 0.0;
}

__device__ inline void bk_centre(uint32_t i, uint32_t j, uint32_t W, uint32_t H, double& px, double& py) {
    px = ((double)j + 0.5) / (double)W;
    py = 1.0 - ((double)i + 0.5) / (double)H;
}

// The edge functions of a face with area at (px, py); true: the face covers the point, edges included: the signs agree
// with the area's and the point lies in the face's closed UV box.  (In exact arithmetic the box follows from the signs; in
// rounded arithmetic it bounds what a sliver, whose edge functions round to zero all along its line, can claim.)
__device__ inline bool bk_covers(const BkFace& e, double px, double py, double& E1, double& E2) {
    const double E0 = (e.bx - px) * (e.cy - py) - (e.by - py) * (e.cx - px);
    E1 = (e.cx - px) * (e.ay - py) - (e.cy - py) * (e.ax - px);
    E2 = (e.ax - px) * (e.by - py) - (e.ay - py) * (e.bx - px);
    const bool in_box = fmin(e.ax, fmin(e.bx, e.cx)) <= px && px <= fmax(e.ax, fmax(e.bx, e.cx)) &&
                        fmin(e.ay, fmin(e.by, e.cy)) <= py && py <= fmax(e.ay, fmax(e.by, e.cy));
    const bool signs = e.A2 > 0.0 ? (E0 >= 0.0 && E1 >= 0.0 && E2 >= 0.0) : (E0 <= 0.0 && E1 <= 0.0 && E2 <= 0.0);
    return signs && in_box;
}

// One wave per face: its 64 lanes stride the texels of the face's bounding box, clipped to the map and widened by a texel
// on every side (the widened box only bounds the work: bk_covers decides, closed box included).  The owner is the lowest covering face, by an
// integer atomicMin: the result does not depend on the order the waves run in.
__global__ __launch_bounds__(256) void k_bk_cover(PrtBakeFaces fc, PrtBakeMap m, uint32_t* __restrict__ counts) {
    const uint64_t f64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (f64 >= fc.n_faces) return;  // (a whole wave leaves)
    const uint32_t f = (uint32_t)f64, lane = threadIdx.x & 63u;
    BkFace e;
    if (!bk_face(fc.uv, f, e)) {
        if (lane == 0u) atomicAdd(counts + PRT_BAKE_CNT_SKIPPED, 1u);
        return;
    }
    const double W = (double)m.W, H = (double)m.H;
    const double minx = fmin(e.ax, fmin(e.bx, e.cx)), maxx = fmax(e.ax, fmax(e.bx, e.cx));
    const double miny = fmin(e.ay, fmin(e.by, e.cy)), maxy = fmax(e.ay, fmax(e.by, e.cy));
    double jlo = floor(minx * W - 0.5) - 1.0, jhi = ceil(maxx * W - 0.5) + 1.0;
    double ilo = floor((1.0 - maxy) * H - 0.5) - 1.0, ihi = ceil((1.0 - miny) * H - 0.5) + 1.0;
    if (jhi < 0.0 || ihi < 0.0 || jlo > W - 1.0 || ilo > H - 1.0) return;
    jlo = fmax(jlo, 0.0);
    ilo = fmax(ilo, 0.0);
    jhi = fmin(jhi, W - 1.0);
    ihi = fmin(ihi, H - 1.0);
    const uint32_t j0 = (uint32_t)jlo, i0 = (uint32_t)ilo;
    const uint32_t bw = (uint32_t)jhi - j0 + 1u, bh = (uint32_t)ihi - i0 + 1u;
    const uint64_t n = (uint64_t)bw * bh;
    for (uint64_t k = lane; k < n; k += 64u) {
        const uint32_t i = i0 + (uint32_t)(k / bw), j = j0 + (uint32_t)(k % bw);
        double px, py, E1, E2;
        bk_centre(i, j, m.W, m.H, px, py);
        if (bk_covers(e, px, py, E1, E2)) atomicMin(m.owner + ((size_t)i * m.W + j), f);
    }
}

// Per texel: the owner's barycentrics by the UV rule's own line, position and shading normal interpolated in fp32 in the
// hit reconstruction's order, then the copy's transform.  A texel whose interpolated normal has no direction is not covered.
__global__ __launch_bounds__(256) void k_bk_surface(PrtBakeFaces fc, PrtBakeMap m, uint32_t* __restrict__ counts) {
    const uint64_t t64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t64 >= (uint64_t)m.W * m.H) return;
    const size_t t = (size_t)t64;
    const uint32_t f = m.owner[t];
    float b1 = 0.0f, b2 = 0.0f;
    f3 p = mk3(0.0f, 0.0f, 0.0f), n = p;
    bool cov = false;
    if (f != kNone) {
        BkFace e;
        (void)bk_face(fc.uv, f, e);
        double px, py, E1, E2;
        bk_centre((uint32_t)(t64 / m.W), (uint32_t)(t64 % m.W), m.W, m.H, px, py);
        (void)bk_covers(e, px, py, E1, E2);
        b1 = (float)(E1 / e.A2);
        b2 = (float)(E2 / e.A2);
        const float w0 = 1.0f - b1 - b2;
        const float* P = fc.pos + 9 * (size_t)f;
        const float* N = fc.nrm + 9 * (size_t)f;
        p = mk3((w0 * P[0] + b1 * P[3]) + b2 * P[6], (w0 * P[1] + b1 * P[4]) + b2 * P[7], (w0 * P[2] + b1 * P[5]) + b2 * P[8]);
        const f3 ns = mk3((w0 * N[0] + b1 * N[3]) + b2 * N[6], (w0 * N[1] + b1 * N[4]) + b2 * N[7], (w0 * N[2] + b1 * N[5]) + b2 * N[8]);
        const float l2 = dot3(ns, ns);
        cov = l2 > 0.0f && l2 < __builtin_huge_valf();
        if (cov) {
            n = normalize3(ns);
            if (fc.placed) {
                p = transform_point(fc.mat, p);
                n = transform_normal(fc.inv, n);
            }
        } else {
            atomicAdd(counts + PRT_BAKE_CNT_DEGENERATE, 1u);
            m.owner[t] = kNone;
            b1 = b2 = 0.0f;
            p = mk3(0.0f, 0.0f, 0.0f);
            n = p;
        }
    }
    m.cov[t] = cov ? 1u : 0u;
    m.bary[2 * t] = b1;
    m.bary[2 * t + 1] = b2;
    m.position[3 * t] = p.x;
    m.position[3 * t + 1] = p.y;
    m.position[3 * t + 2] = p.z;
    m.normal[3 * t] = n.x;
    m.normal[3 * t + 1] = n.y;
    m.normal[3 * t + 2] = n.z;
}

// The covered texels in ascending order: one block walks the map 1024 texels at a time; inside a step a texel's place is
// the covered texels below it (ballot and popcount inside its wave, the sixteen wave totals before it).  No atomics: the
// list is the same in every run.
__global__ __launch_bounds__(1024) void k_bk_compact(uint32_t n, const uint8_t* __restrict__ cov, uint32_t* __restrict__ list,
                                                     uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t base = 0u;
    for (uint64_t start = 0; start < n; start += 1024u) {
        const uint64_t t = start + tid;
        const bool want = t < n && cov[t] != 0u;
        const unsigned long long mask = __ballot(want);
        if (lane == 0u) wsum[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint32_t v = wsum[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        if (want) list[base + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)t;
        base += total;
        __syncthreads();
    }
    if (tid == 0u) counts[PRT_BAKE_CNT_COVERED] = base;
}

// The texel as a Lambertian path vertex of albedo 1: the shade kernels' scatter from path_seed(t, sample, seed), the
// direction normalised as k_rd_step normalises it, the state the advanced one.
__global__ __launch_bounds__(256) void k_bk_rays(uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const uint32_t* __restrict__ list,
                                                 PrtBakeMap m, float* __restrict__ o, float* __restrict__ d, uint32_t* __restrict__ rng_out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= (uint64_t)cs * n) return;
    const uint32_t s_local = (uint32_t)(j / n);
    const uint32_t k = (uint32_t)(j - (uint64_t)s_local * n);
    const uint32_t t = list ? list[k] : k;
    f3 so = mk3(0.0f, 0.0f, 0.0f), sd = so;
    uint32_t rng = 0u;
    if (m.cov[t] != 0u) {
        const f3 p = mk3(m.position[3 * (size_t)t], m.position[3 * (size_t)t + 1], m.position[3 * (size_t)t + 2]);
        const f3 nn = mk3(m.normal[3 * (size_t)t], m.normal[3 * (size_t)t + 1], m.normal[3 * (size_t)t + 2]);
        rng = path_seed(t, sample0 + s_local, seed);
        f3 atten, emitted, out_d;
        (void)material_scatter(1u, make_float4(1.0f, 1.0f, 1.0f, 0.0f), -nn, p, nn, true, rng, atten, emitted, so, out_d);
        sd = normalize3(out_d);
    }
    const size_t w = 3 * (size_t)j;
    o[w] = so.x;
    o[w + 1] = so.y;
    o[w + 2] = so.z;
    d[w] = sd.x;
    d[w + 1] = sd.y;
    d[w + 2] = sd.z;
    rng_out[j] = rng;
}

// Entry k's values in ascending sample order into its texel; the segments are integers, summed per wave and added once.
__global__ __launch_bounds__(256) void k_bk_sum(uint32_t n, uint32_t cs, uint32_t first, const uint32_t* __restrict__ list, const float* __restrict__ rgb,
                                                const uint32_t* __restrict__ seg, float* __restrict__ rgb_sum, uint32_t* __restrict__ counts) {
    const uint64_t k64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t segs = 0u;
    if (k64 < n) {
        const uint32_t k = (uint32_t)k64;
        const size_t r = 3 * (size_t)list[k];
        f3 acc = first ? mk3(0.0f, 0.0f, 0.0f) : mk3(rgb_sum[r], rgb_sum[r + 1], rgb_sum[r + 2]);
        for (uint32_t s = 0; s < cs; ++s) {
            const size_t q = (size_t)s * n + k;
            acc = acc + mk3(rgb[3 * q], rgb[3 * q + 1], rgb[3 * q + 2]);
            segs += seg[q];
        }
        rgb_sum[r] = acc.x;
        rgb_sum[r + 1] = acc.y;
        rgb_sum[r + 2] = acc.z;
    }
    for (int off = 32; off > 0; off >>= 1) segs += (uint32_t)__shfl_xor((int)segs, off, 64);
    if ((threadIdx.x & 63u) == 0u && segs != 0u) atomicAdd((unsigned long long*)(counts + PRT_BAKE_CNT_SEGMENTS), (unsigned long long)segs);
}

// One pass of the gutter fill: an uncovered texel next to covered ones takes their mean, neighbours in row-major order.
__global__ __launch_bounds__(256) void k_bk_dilate(uint32_t W, uint32_t H, const uint8_t* __restrict__ cov_in, const float* __restrict__ rgb_in,
                                                   uint8_t* __restrict__ cov_out, float* __restrict__ rgb_out, uint32_t* __restrict__ counts) {
    const uint64_t t64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t64 >= (uint64_t)W * H) return;
    const size_t t = (size_t)t64;
    const uint32_t i = (uint32_t)(t64 / W), j = (uint32_t)(t64 % W);
    uint8_t c = cov_in[t];
    f3 v = mk3(rgb_in[3 * t], rgb_in[3 * t + 1], rgb_in[3 * t + 2]);
    if (c == 0u) {
        f3 acc = mk3(0.0f, 0.0f, 0.0f);
        uint32_t cnt = 0u;
        for (int di = -1; di <= 1; ++di)
            for (int dj = -1; dj <= 1; ++dj) {
                if (di == 0 && dj == 0) continue;
                const int64_t ii = (int64_t)i + di, jj = (int64_t)j + dj;
                if (ii < 0 || jj < 0 || ii >= (int64_t)H || jj >= (int64_t)W) continue;
                const size_t q = (size_t)ii * W + (size_t)jj;
                if (cov_in[q] == 0u) continue;
                acc = acc + mk3(rgb_in[3 * q], rgb_in[3 * q + 1], rgb_in[3 * q + 2]);
                ++cnt;
            }
        if (cnt != 0u) {
            v = acc / (float)cnt;
            c = 2u;
            atomicAdd(counts + PRT_BAKE_CNT_FILLED, 1u);
        }
    }
    cov_out[t] = c;
    rgb_out[3 * t] = v.x;
    rgb_out[3 * t + 1] = v.y;
    rgb_out[3 * t + 2] = v.z;
}

}  // namespace

void prt_launch_bk_cover(hipStream_t st, const PrtBakeFaces& f, PrtBakeMap m, uint32_t* counts) {
    hipLaunchKernelGGL(k_bk_cover, dim3((f.n_faces + 3u) / 4u), dim3(256), 0, st, f, m, counts);
}

void prt_launch_bk_surface(hipStream_t st, const PrtBakeFaces& f, PrtBakeMap m, uint32_t* counts) {
    hipLaunchKernelGGL(k_bk_surface, dim3(blocks_for((uint64_t)m.W * m.H)), dim3(256), 0, st, f, m, counts);
}

void prt_launch_bk_compact(hipStream_t st, uint32_t n_texels, const uint8_t* cov, uint32_t* list, uint32_t* counts) {
    hipLaunchKernelGGL(k_bk_compact, dim3(1), dim3(1024), 0, st, n_texels, cov, list, counts);
}

void prt_launch_bk_rays(hipStream_t st, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const uint32_t* list, PrtBakeMap m,
                        float* o, float* d, uint32_t* rng) {
    hipLaunchKernelGGL(k_bk_rays, dim3(blocks_for((uint64_t)cs * n)), dim3(256), 0, st, n, cs, sample0, seed, list, m, o, d, rng);
}

void prt_launch_bk_sum(hipStream_t st, uint32_t n, uint32_t cs, bool first, const uint32_t* list, const float* rgb, const uint32_t* seg,
                       float* rgb_sum, uint32_t* counts) {
    hipLaunchKernelGGL(k_bk_sum, dim3(blocks_for(n)), dim3(256), 0, st, n, cs, first ? 1u : 0u, list, rgb, seg, rgb_sum, counts);
}

void prt_launch_bk_dilate(hipStream_t st, uint32_t W, uint32_t H, const uint8_t* cov_in, const float* rgb_in, uint8_t* cov_out, float* rgb_out,
                          uint32_t* counts) {
    hipLaunchKernelGGL(k_bk_dilate, dim3(blocks_for((uint64_t)W * H)), dim3(256), 0, st, W, H, cov_in, rgb_in, cov_out, rgb_out, counts);
}

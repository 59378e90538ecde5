// prt_bake_adaptive.hip — the device code of the bake's statistics and block-adaptive sampling (include/prt.h "Bake
// statistics and adaptive sampling"): the ordered sum with luminance moments, the per-block stopping decision, the ordered
// compaction of the block list and the mean.  A translation unit of its own: prt_bake.hip and prt_bake_light.hip keep their
// kernels, and the rays, the paths and the texel's light sample of a pass are theirs.  Built with the flags of
// prt_kernels.hip: no contraction, so every line below is the IEEE operation it spells.  The rule is prt_adaptive.h's, the
// lines the film's k_tile_select and the host compile.
#include <hip/hip_runtime.h>

#include "prt_adaptive.h"
#include "prt_bake_adaptive.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// Entry k's values in ascending sample order into its texel: k_bk_sum's colour sum, and beside it the film's luminance
// moments (k_accumulate_stat's single fp32 operations) and the count.  Rays are sample-major over the list, so consecutive
// lanes read consecutive rays.  The segments are integers, summed per wave and added once.
__global__ __launch_bounds__(256) void k_bka_sum(uint32_t n, uint32_t cs, uint32_t first, const uint32_t* __restrict__ list,
                                                 const float* __restrict__ rgb, const uint32_t* __restrict__ seg, PrtBakeMoments m,
                                                 uint32_t* __restrict__ counts) {
    const uint64_t k64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t segs = 0u;
    if (k64 < n) {
        const uint32_t k = (uint32_t)k64;
        const size_t t = list[k], r = 3 * t;
        float ax = 0.0f, ay = 0.0f, az = 0.0f, A = 0.0f, Q = 0.0f, cnt = 0.0f;
        if (!first) {
            ax = m.rgb_sum[r];
            ay = m.rgb_sum[r + 1];
            az = m.rgb_sum[r + 2];
            A = m.sum_y[t];
            Q = m.sum_y2[t];
            cnt = m.count[t];
        }
        for (uint32_t s = 0; s < cs; ++s) {
            const size_t q = (size_t)s * n + k;
            const float vr = rgb[3 * q], vg = rgb[3 * q + 1], vb = rgb[3 * q + 2];
            ax = __fadd_rn(ax, vr);
            ay = __fadd_rn(ay, vg);
            az = __fadd_rn(az, vb);
            const float lum = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, vr), __fmul_rn(0.7152f, vg)), __fmul_rn(0.0722f, vb));
            A = __fadd_rn(A, lum);
            Q = __fadd_rn(Q, __fmul_rn(lum, lum));
            segs += seg[q];
        }
        m.rgb_sum[r] = ax;
        m.rgb_sum[r + 1] = ay;
        m.rgb_sum[r + 2] = az;
        m.sum_y[t] = A;
        m.sum_y2[t] = Q;
        m.count[t] = cnt + (float)cs;  // (exact: a count stays far below 2^24)
    }
    for (int off = 32; off > 0; off >>= 1) segs += (uint32_t)__shfl_xor((int)segs, off, 64);
    if ((threadIdx.x & 63u) == 0u && segs != 0u) atomicAdd((unsigned long long*)(counts + PRT_BAKE_CNT_SEGMENTS), (unsigned long long)segs);
}

// One wave per entry of prev.  Lane l holds texel (8 by + l / 8, 8 bx + l % 8) of block (by, bx); a lane outside the map or on
// a texel that is not owned (cov != 1) is converged.  The block is active iff the ballot of the rule is not empty: no
// floating-point reduction, so the decision cannot depend on an order.
__global__ __launch_bounds__(256) void k_bka_select(uint32_t W, uint32_t H, const uint8_t* __restrict__ cov, PrtBakeMoments m,
                                                    const uint32_t* __restrict__ prev, uint32_t n_prev, float threshold, float noise_floor,
                                                    uint32_t at_cap, uint32_t* __restrict__ flags, uint8_t* __restrict__ active,
                                                    uint32_t* __restrict__ sel) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);  // wave-uniform
    if (i >= n_prev) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = prev ? prev[i] : i;
    const uint32_t bx_n = (W + 7u) >> 3;
    const uint32_t row = (b / bx_n) * 8u + (lane >> 3), col = (b % bx_n) * 8u + (lane & 7u);
    const bool inside = row < H && col < W;
    const size_t t = inside ? (size_t)row * W + col : 0;
    const bool covered = inside && cov[t] == 1u;
    bool unconverged = false;
    if (covered) unconverged = prt_adaptive_rule(m.count[t], m.sum_y[t], m.sum_y2[t], threshold, noise_floor);
    const bool on = __ballot(unconverged) != 0ull;
    if (inside) active[t] = (covered && on) ? 1u : 0u;
    if (lane == 0u) {
        flags[i] = on ? 1u : 0u;
        if (!on) atomicAdd(sel + PRT_BKA_CNT_CONVERGED, 1u);
        else if (at_cap) atomicAdd(sel + PRT_BKA_CNT_CAPPED, 1u);
    }
}

// Ordered compaction of k_bka_select's flags: one block walks them 1024 at a time; inside a step an entry's place is the
// flagged entries before it (ballot and popcount inside its wave, the sixteen wave totals before it).  No atomics: the list
// is the same in every run.  The entries past the list read 0xFFFFFFFF.
__global__ __launch_bounds__(1024) void k_bka_blocks(uint32_t n_prev, const uint32_t* __restrict__ prev, const uint32_t* __restrict__ flags,
                                                     uint32_t* __restrict__ out, uint32_t* __restrict__ sel) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t base = 0u;
    for (uint32_t start = 0; start < n_prev; start += 1024u) {  // block-uniform trip count
        const uint32_t i = start + tid;
        const bool want = i < n_prev && flags[i] != 0u;
        const uint32_t b = want ? (prev ? prev[i] : i) : 0u;  // (read before the barrier: out may not alias prev)
        const unsigned long long mask = __ballot(want);
        if (lane == 0u) wsum[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint32_t v = wsum[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        if (want) out[base + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = b;
        base += total;
        __syncthreads();
    }
    for (uint32_t i = base + tid; i < n_prev; i += 1024u) out[i] = kNone;
    if (tid == 0u) sel[PRT_BKA_CNT_ACTIVE] = base;
}

// One thread per texel: a single fp32 division per component.
__global__ __launch_bounds__(256) void k_bka_mean(uint32_t n, const float* __restrict__ rgb_sum, const float* __restrict__ count,
                                                  float* __restrict__ rgb_mean) {
    const uint64_t t64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t64 >= n) return;
    const size_t r = 3 * (size_t)t64;
    const float c = count[t64];
    const bool any = c > 0.0f;
    rgb_mean[r] = any ? __fdiv_rn(rgb_sum[r], c) : 0.0f;
    rgb_mean[r + 1] = any ? __fdiv_rn(rgb_sum[r + 1], c) : 0.0f;
    rgb_mean[r + 2] = any ? __fdiv_rn(rgb_sum[r + 2], c) : 0.0f;
}

}  // namespace

void prt_launch_bka_sum(hipStream_t st, uint32_t n, uint32_t cs, bool first, const uint32_t* list, const float* rgb, const uint32_t* seg,
                        PrtBakeMoments m, uint32_t* counts) {
    hipLaunchKernelGGL(k_bka_sum, dim3(blocks_for(n)), dim3(256), 0, st, n, cs, first ? 1u : 0u, list, rgb, seg, m, counts);
}

void prt_launch_bka_select(hipStream_t st, uint32_t W, uint32_t H, const uint8_t* cov, PrtBakeMoments m, const uint32_t* prev, uint32_t n_prev,
                           float threshold, float noise_floor, bool at_cap, uint32_t* flags, uint8_t* active, uint32_t* sel) {
    if (n_prev)
        hipLaunchKernelGGL(k_bka_select, dim3((n_prev + 3u) / 4u), dim3(256), 0, st, W, H, cov, m, prev, n_prev, threshold, noise_floor,
                           at_cap ? 1u : 0u, flags, active, sel);
}

void prt_launch_bka_blocks(hipStream_t st, uint32_t n_prev, const uint32_t* prev, const uint32_t* flags, uint32_t* out, uint32_t* sel) {
    hipLaunchKernelGGL(k_bka_blocks, dim3(1), dim3(1024), 0, st, n_prev, prev, flags, out, sel);
}

void prt_launch_bka_mean(hipStream_t st, uint32_t n_texels, const float* rgb_sum, const float* count, float* rgb_mean) {
    hipLaunchKernelGGL(k_bka_mean, dim3(blocks_for(n_texels)), dim3(256), 0, st, n_texels, rgb_sum, count, rgb_mean);
}

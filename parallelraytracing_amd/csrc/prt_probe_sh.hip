// prt_probe_sh.hip — the device code of the SH probes (include/prt.h "SH probes"): from probe positions to uniformly
// distributed rays, and from the radiance query's per-ray results to nine spherical-harmonic sums per probe and channel.
// A translation unit of its own: nothing in a batch route or in another unit's kernel set changes for it.  Built with the
// flags of prt_kernels.hip: no contraction, so every line below is the IEEE operation it spells.  The sampler and the seed
// are the shade kernels' own (prt_device.h); the basis is prt_sh_contract.h's, which the host compiles too.
#include <hip/hip_runtime.h>

#include "prt_device.h"
#include "prt_probe_sh.h"
#include "prt_sh_contract.h"

namespace {

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// One thread per (sample, probe), sample-major: the probe index stands where the pixel index stands in a render.  The
// direction is the rejection sampler's, as returned.
__global__ __launch_bounds__(256) void k_sh_rays(uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* __restrict__ pos,
                                                 float* __restrict__ o, float* __restrict__ d, uint32_t* __restrict__ rng_out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= (uint64_t)cs * n) return;
    const uint32_t s_local = (uint32_t)(j / n);
    const uint32_t p = (uint32_t)(j - (uint64_t)s_local * n);
    uint32_t rng = path_seed(p, sample0 + s_local, seed);
    const f3 dir = random_unit_vector(rng);
    const size_t w = 3 * (size_t)j;
    o[w] = pos[3 * (size_t)p];
    o[w + 1] = pos[3 * (size_t)p + 1];
    o[w + 2] = pos[3 * (size_t)p + 2];
    d[w] = dir.x;
    d[w + 1] = dir.y;
    d[w + 2] = dir.z;
    rng_out[j] = rng;
}

// One thread per (k, probe), probe fastest: consecutive lanes read consecutive rays of a sample.  Three accumulators per
// thread, the samples in ascending order; the threads of k = 0 also count the segments, which are integers, summed per wave
// and added once.
__global__ __launch_bounds__(256) void k_sh_project(uint32_t n, uint32_t cs, uint32_t K, uint32_t first, const float* __restrict__ d,
                                                    const float* __restrict__ rgb, const uint32_t* __restrict__ seg, float* __restrict__ sh_sum,
                                                    uint32_t* __restrict__ counts) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t segs = 0u;
    if (t < (uint64_t)K * n) {
        const uint32_t k = (uint32_t)(t / n);
        const uint32_t p = (uint32_t)(t - (uint64_t)k * n);
        const size_t r = 3 * ((size_t)p * K + k);
        f3 acc = first ? mk3(0.0f, 0.0f, 0.0f) : mk3(sh_sum[r], sh_sum[r + 1], sh_sum[r + 2]);
        for (uint32_t s = 0; s < cs; ++s) {
            const size_t q = (size_t)s * n + p;
            const float y = prt_sh_basis(k, d[3 * q], d[3 * q + 1], d[3 * q + 2]);
            acc = acc + mk3(rgb[3 * q] * y, rgb[3 * q + 1] * y, rgb[3 * q + 2] * y);
            if (k == 0u) segs += seg[q];
        }
        sh_sum[r] = acc.x;
        sh_sum[r + 1] = acc.y;
        sh_sum[r + 2] = acc.z;
    }
    for (int off = 32; off > 0; off >>= 1) segs += (uint32_t)__shfl_xor((int)segs, off, 64);
    if ((threadIdx.x & 63u) == 0u && segs != 0u)
        atomicAdd((unsigned long long*)(counts + PRT_PROBE_SH_CNT_SEGMENTS), (unsigned long long)segs);
}

}  // namespace

void prt_launch_sh_rays(hipStream_t st, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* pos, float* o, float* d,
                        uint32_t* rng) {
    hipLaunchKernelGGL(k_sh_rays, dim3(blocks_for((uint64_t)cs * n)), dim3(256), 0, st, n, cs, sample0, seed, pos, o, d, rng);
}

void prt_launch_sh_project(hipStream_t st, uint32_t n, uint32_t cs, uint32_t K, bool first, const float* d, const float* rgb, const uint32_t* seg,
                           float* sh_sum, uint32_t* counts) {
    hipLaunchKernelGGL(k_sh_project, dim3(blocks_for((uint64_t)K * n)), dim3(256), 0, st, n, cs, K, first ? 1u : 0u, d, rgb, seg, sh_sum, counts);
}

// prt_feature_samples.hip — the device code of the sampled guide features (include/prt.h "Sampled guide features"): the
// render's own primary rays of K samples per pixel, the ordered sums of their feature records, and the finish.  A
// translation unit of its own: nothing in prt_kernels.hip, prt_features.hip, prt_denoise.hip or prt_temporal.hip changes
// for it.  Built with the flags of prt_kernels.hip: no contraction, so every line below is the IEEE operation it spells, and
// tests/feature_samples_replay.py restates the sums and the finish in numpy float32.  The rays come from the render's own
// device functions (prt_device.h): path_seed, rnd01, camera_ray, lens_camera_ray.
#include <hip/hip_runtime.h>

#include "prt_feature_samples.h"
#include "prt_device.h"

namespace {

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// One 16-byte store per record (spelled as a vector so that it is never split into 4 + 12 bytes).
PRT_DEV void st4(float4* p, float4 v) { *(prt_v4f*)p = prt_v4f{v.x, v.y, v.z, v.w}; }

// One thread per slot, sample-major: the lanes of a wave are neighbouring pixels of one sample, so the hits the query
// pipeline writes for them, and the records the reduce reads, are contiguous per sample.
__global__ __launch_bounds__(256) void k_fs_rays(DevCamera cam, DevLens lens, PrtSampleChunk ch, float* __restrict__ o,
                                                 float* __restrict__ d) {
    const uint32_t n = ch.W * ch.H;
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;  // (the host keeps cs * n below 2^32)
    if (j >= ch.cs * n) return;
    const uint32_t sl = j / n, p = j - sl * n;
    const uint32_t y = p / ch.W, x = p - y * ch.W;
    uint32_t rng = path_seed(p, ch.first_sample + ch.s0 + sl, ch.seed);
    // (x + u1, y + u2): the path's first two draws, as raygen_step forms them; then the two lens draws
    const float u1 = ch.jitter ? rnd01(rng) : 0.5f;
    const float u2 = ch.jitter ? rnd01(rng) : 0.5f;
    f3 ro, rd;
    if (lens.aperture > 0.0f) lens_camera_ray(cam, lens, (float)x + u1, (float)y + u2, rng, ro, rd);
    else camera_ray(cam, (float)x + u1, (float)y + u2, ro, rd);
    const size_t b = 3 * (size_t)j;
    o[b] = ro.x;
    o[b + 1] = ro.y;
    o[b + 2] = ro.z;
    d[b] = rd.x;
    d[b + 1] = rd.y;
    d[b + 2] = rd.z;
}

// One thread per pixel; the chunk's samples in order, sums in registers, one read-modify-write of the pixel's running sums.
// No atomics and nothing crosses lanes: the order of every addition is the sample order, whatever the chunking.
__global__ __launch_bounds__(256) void k_fs_reduce(PrtSampleChunk ch, PrtFeatureBufs rec, PrtFeatureBufs sums) {
    const uint32_t n = ch.W * ch.H;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    float4 Sa = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                   // .w: hits (an integer <= 64: exact)
    float4 Sn = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));     // .w: prim of the first sample that hit
    float4 Sp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                   // .w: Sd
    if (ch.s0 != 0u) {
        Sa = ld_stream(sums.alb + p);
        Sn = ld_stream(sums.nrm + p);
        Sp = ld_stream(sums.pos + p);
    }
    for (uint32_t sl = 0; sl < ch.cs; ++sl) {
        const size_t j = (size_t)sl * n + p;
        const float4 a = ld_stream(rec.alb + j), nr = ld_stream(rec.nrm + j), ps = ld_stream(rec.pos + j);  // (read once: 16-byte loads)
        Sa.x = Sa.x + a.x;
        Sa.y = Sa.y + a.y;
        Sa.z = Sa.z + a.z;
        if (__float_as_int(nr.w) >= 0) {
            if (Sa.w == 0.0f) Sn.w = nr.w;
            Sn.x = Sn.x + nr.x;
            Sn.y = Sn.y + nr.y;
            Sn.z = Sn.z + nr.z;
            Sp.x = Sp.x + ps.x;
            Sp.y = Sp.y + ps.y;
            Sp.z = Sp.z + ps.z;
            Sp.w = Sp.w + ps.w;
            Sa.w = Sa.w + 1.0f;
        }
    }
    st4(sums.alb + p, Sa);
    st4(sums.nrm + p, Sn);
    st4(sums.pos + p, Sp);
}

__global__ __launch_bounds__(256) void k_fs_finish(uint32_t n, uint32_t K, bool copy, PrtFeatureBufs src, PrtFeatureBufs set) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    if (copy) {  // every sample is the centre ray: the centre-ray set itself, hits = 0 or 1
        const float4 a = ld_stream(src.alb + p), nr = ld_stream(src.nrm + p), ps = ld_stream(src.pos + p);
        st4(set.alb + p, make_float4(a.x, a.y, a.z, __float_as_int(nr.w) >= 0 ? 1.0f : 0.0f));
        st4(set.nrm + p, nr);
        st4(set.pos + p, ps);
        return;
    }
    const float4 Sa = ld_stream(set.alb + p), Sn = ld_stream(set.nrm + p), Sp = ld_stream(set.pos + p);
    const float ik = 1.0f / (float)K;
    float4 a = make_float4(Sa.x * ik, Sa.y * ik, Sa.z * ik, Sa.w);
    float4 nr = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    float4 ps = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (Sa.w > 0.0f) {
        const float ih = 1.0f / Sa.w;
        ps = make_float4(Sp.x * ih, Sp.y * ih, Sp.z * ih, Sp.w * ih);
        const float l2 = (Sn.x * Sn.x + Sn.y * Sn.y) + Sn.z * Sn.z;  // dot3
        const bool some = l2 > 0.0f;
        const float il = 1.0f / __builtin_sqrtf(l2);
        nr = make_float4(some ? Sn.x * il : 0.0f, some ? Sn.y * il : 0.0f, some ? Sn.z * il : 0.0f, Sn.w);
    }
    st4(set.alb + p, a);
    st4(set.nrm + p, nr);
    st4(set.pos + p, ps);
}

}  // namespace

void prt_launch_fs_rays(hipStream_t st, const DevCamera& cam, const DevLens& lens, const PrtSampleChunk& ch, float* o, float* d) {
    const uint32_t blocks = blocks_for((uint64_t)ch.cs * ch.W * ch.H);
    hipLaunchKernelGGL(k_fs_rays, dim3(blocks), dim3(256), 0, st, cam, lens, ch, o, d);
}

void prt_launch_fs_reduce(hipStream_t st, const PrtSampleChunk& ch, PrtFeatureBufs rec, PrtFeatureBufs sums) {
    hipLaunchKernelGGL(k_fs_reduce, dim3(blocks_for((uint64_t)ch.W * ch.H)), dim3(256), 0, st, ch, rec, sums);
}

void prt_launch_fs_finish(hipStream_t st, uint32_t n, uint32_t K, const PrtFeatureBufs* copy_from, PrtFeatureBufs set) {
    hipLaunchKernelGGL(k_fs_finish, dim3(blocks_for(n)), dim3(256), 0, st, n, K, copy_from != nullptr, copy_from ? *copy_from : set, set);
}

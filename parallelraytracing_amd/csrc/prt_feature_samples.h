// prt_feature_samples.h — launcher prototypes of the sampled guide features (prt_feature_samples.hip; include/prt.h
// "Sampled guide features").  No kernel syntax here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "../../include/prt.h"
#include "prt_denoise.h"  // PrtFeatureBufs
#include "prt_kernels.h"  // DevCamera, DevLens

// The samples of one chunk: cs samples s0 .. s0 + cs - 1 of every pixel of a W x H film, sample-major: slot
// j = (s - s0) * W * H + p holds sample s of pixel p = y * W + x.
struct PrtSampleChunk {
    uint32_t W, H;
    uint32_t s0, cs;        // first sample of the chunk (0-based within the K samples) and how many
    uint32_t first_sample;  // PrtFeatureSampling.first_sample
    uint32_t seed;          // PrtFeatureSampling.seed
    uint32_t jitter;        // PrtSampling.jitter
};

// The primary ray of every slot, exactly the one prt_render traces for that (pixel, sample, seed): the render's key, its two
// jitter draws, then lens_camera_ray (lens.aperture > 0) or camera_ray.  o, d: 3 floats per slot, the layout the ray-query
// pipeline packs from.
void prt_launch_fs_rays(hipStream_t st, const DevCamera& cam, const DevLens& lens, const PrtSampleChunk& ch, float* o, float* d);
// Adds the chunk's per-slot records (rec) to the running sums of every pixel, in sample order.  The sums live in the sampled
// set's own records: alb {Sa, hits as a float}, nrm {Sn, prim}, pos {Sp, Sd}.  The chunk with s0 == 0 starts them.
void prt_launch_fs_reduce(hipStream_t st, const PrtSampleChunk& ch, PrtFeatureBufs rec, PrtFeatureBufs sums);
// Sums to records in place (K samples): alb {albedo, hits as a float}, nrm {normal, prim}, pos {position, depth}.
// copy_from != nullptr (the degenerate case, K ignored): set = *copy_from with hits = prim >= 0 ? 1 : 0.
void prt_launch_fs_finish(hipStream_t st, uint32_t n, uint32_t K, const PrtFeatureBufs* copy_from, PrtFeatureBufs set);

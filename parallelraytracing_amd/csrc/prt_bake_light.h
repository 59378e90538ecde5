// prt_bake_light.h — launcher prototypes of the texel's light sample of surface baking (prt_bake_light.hip; include/prt.h
// "Surface baking", the texel's light sample).  No kernel syntax here.
#pragma once
#include "prt_bake.h"
#include "prt_radiance_lit.h"

#define PRT_BKL_STAT_SLOTS 16u  // copies of the two shadow-ray counters: block b adds to copy b mod SLOTS, the host sums

// What the sample kernel reads beside the map: the light tables of prt_sample_light (ml / lc / env are read only by the
// instances that know them) and PrtSampling.clamp.
struct PrtBakeLightArgs {
    DevLights lt;
    DevMeshLights ml;
    DevLightClusters lc;
    DevEnv env;
    float clamp;
};

// One entry per ray of prt_launch_bk_rays' layout (ray s_local * n + k; entry k is texel list[k], or texel k with list ==
// null): x = the texel's position, w = the sampled direction (zero without a sample), tmax = the shadow ray's bound, 0
// where none is cast (no sample, or n.w <= 0), contrib = the clamped term, zero where no ray is cast.
struct PrtBakeLightRays {
    float* x;        // 3 per ray; may be null
    float* w;        // 3 per ray
    float* tmax;
    float* contrib;  // 3 per ray
    uint32_t* light; // the candidate / light index, PRT_LIGHT_ENVIRONMENT, 0xFFFFFFFF: no sample; may be null
    float* ray_pb;   // the pdf of the texel's own ray d: max(0, n.d) / pi
};

// The light sample of cs samples of n entries with key = path_seed(texel, sample0 + s_local, seed), and the pdf of the
// texel's ray d (prt_launch_bk_rays' output).  mesh / env / clus choose the instance as prt_launch_rdl_step's do.
void prt_launch_bkl_sample(hipStream_t st, bool mesh, bool env, bool clus, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed,
                           const uint32_t* list, PrtBakeMap m, const float* d, const PrtBakeLightArgs& a, PrtBakeLightRays out);
// After the occlusion pipeline over the n_rays rays of `r`: rgb[j] += contrib[j] where tmax[j] > 0 and the ray is not
// occluded, one fp32 add per component; stats [PRT_BKL_STAT_SLOTS][2] counts the rays cast and the occluded ones.
void prt_launch_bkl_add(hipStream_t st, uint32_t n_rays, PrtBakeLightRays r, const uint8_t* occluded, float* rgb, unsigned long long* stats);

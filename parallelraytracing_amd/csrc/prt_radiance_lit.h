// prt_radiance_lit.h — launcher prototypes of the light-sampled radiance query (prt_radiance_lit.hip; include/prt.h
// "Radiance query", prt_radiance_lit).  No kernel syntax here.
#pragma once
#include "prt_radiance.h"

// A list of live paths: PrtRadianceList's ray and state, plus pb: the pdf of the Lambertian scatter that started the
// entry's segment (-1: the caller's ray, or a metal / dielectric vertex), which moves with them.
struct PrtRadianceLitList {
    PrtRadianceList l;
    float* pb;
};

// The shadow rays of one round, in the layout the ray-query pipeline packs occlusion rays from: x, w 3 floats per ray,
// tmax one; cs = {contrib.rgb, the path's slot as its bit pattern}.
struct PrtRadianceShadowList {
    float* x;
    float* w;
    float* tmax;
    float4* cs;
};

#define PRT_RDL_STAT_SLOTS 16u  // copies of the query's two shadow-ray counters: block b adds to copy b mod SLOTS, the host sums

// What a lit round needs beside PrtRadianceArgs (whose env stays empty when no environment image is set).  The light
// tables are those of prt_sample_light; ml / lc are read only by the instances that know them.
struct PrtRadianceLitArgs {
    PrtRadianceArgs a;
    DevLights lt;
    DevMeshLights ml;
    DevLightClusters lc;
    uint32_t n_prims;    // analytic primitives: a hit with prim below it is analytic
    PrtRadianceShadowList sh;
    uint32_t* scount;    // the shadow list's length: zero before the launch
};

// prt_launch_rd_start's paths with pb = -1 (pb == null), or pb[i] for every sample of ray i.
void prt_launch_rdl_start(hipStream_t st, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* origins,
                          const float* dirs, const uint32_t* rng_state, const float* pb, PrtRadianceLitList out);
// prt_launch_rd_step's round with light sampling: the emission of a light-set emitter met after a Lambertian vertex (and
// the environment's texel after one) weighted, and one light sample per Lambertian vertex that scatters before the last
// segment, appended to a.sh.  mesh / env / clus choose the instance as prt_sample_light's do (clus implies mesh).
void prt_launch_rdl_step(hipStream_t st, bool mesh, bool env, bool clus, uint32_t n, PrtRadianceLitList in, const PrtRadianceLitArgs& a,
                         PrtRadianceLitList out);
// After the occlusion pipeline over the n shadow rays of `sh`: an unoccluded ray adds its contrib to lsum[slot]; stats
// [PRT_RDL_STAT_SLOTS][2] counts rays and occluded rays.
void prt_launch_rdl_light(hipStream_t st, uint32_t n, PrtRadianceShadowList sh, const uint8_t* occluded, float4* lsum,
                          unsigned long long* stats);
// prt_launch_rd_sum with the sample value slot.rgb + lsum[slot].
void prt_launch_rdl_sum(hipStream_t st, uint32_t n, uint32_t cs, bool first, const float4* slots, const float4* lsum, float* rgb_sum,
                        uint32_t* segments);

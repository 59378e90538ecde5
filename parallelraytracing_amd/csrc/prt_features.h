// prt_features.h — launcher prototypes of the guide features through specular chains (prt_features.hip; include/prt.h
// "Guide features through specular chains").  No kernel syntax here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "../../include/prt.h"
#include "prt_denoise.h"  // PrtFeatureBufs
#include "prt_kernels.h"  // DevScene

// A list of live chains: entry j is a ray (o, d: 3 floats each, the layout the ray-query pipeline packs from) and the state
// that moves with it, two float4: s0 = {pixel as its uint32 bit pattern, k as its uint32 bit pattern, L, 0}, s1 = {T, 0}.
struct PrtChainList {
    float* o;
    float* d;
    float4* s0;
    float4* s1;
};

// What both kernels need beside the lists.  albedo: prt_launch_hit_uv's output for the rays whose hits are in `hits`
// (3 floats per ray) while a binding textures something, else null: the material's constant rgb is gathered.
struct PrtChainArgs {
    const PrtHit* hits;
    const float* albedo;
    const float4* mat_rgbs;
    const uint32_t* mat_type;
    PrtFeatureTrace ft;
    PrtFeatureBufs guide;
    uint32_t* count;  // the output list's length: zero before the launch
};

// From the first-hit pass's n centre rays (dirs) and their hit records: pixel i either gets its guide records (terminal at
// k = 0) or appends its next segment to `out`.
void prt_launch_ft_start(hipStream_t st, uint32_t n, const float* dirs, const PrtChainArgs& a, PrtChainList out);
// One round over the n live entries of `in`, whose closest hits are a.hits[0 .. n): the same decision for k >= 1.  `out`
// never shares a buffer with `in`.
void prt_launch_ft_step(hipStream_t st, uint32_t n, PrtChainList in, const PrtChainArgs& a, PrtChainList out);

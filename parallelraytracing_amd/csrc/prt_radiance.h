// prt_radiance.h — launcher prototypes of the radiance query (prt_radiance.hip; include/prt.h "Radiance query").  No kernel
// syntax here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "../../include/prt.h"
#include "prt_kernels.h"  // DevEnv

// A list of live paths: entry j is a ray (o, d: 3 floats each, the layout the ray-query pipeline packs from) and the state
// that moves with it, two float4: s0 = {slot as its uint32 bit pattern, rng state as its bit pattern, thr.x, thr.y},
// s1 = {thr.z, L.x, L.y, L.z}.  Slot s_local * n + i holds sample s_local of the chunk of ray i.
struct PrtRadianceList {
    float* o;
    float* d;
    float4* s0;
    float4* s1;
};

// What a round needs beside the lists.  albedo: prt_launch_hit_uv's output for the rays whose hits are in `hits` (3 floats
// per ray) while a binding textures something, else null: the material's constant rgb is gathered.  env.W == 0: a miss
// delivers `sky`.  round is the segment index of the rays in the list, the same for all of them.
struct PrtRadianceArgs {
    const PrtHit* hits;
    const float* albedo;
    const float4* mat_rgbs;
    const uint32_t* mat_type;
    DevEnv env;
    float sky[3];
    PrtSampling sp;
    uint32_t max_depth;
    uint32_t round;
    float4* slots;       // per slot, written once when its path ends: the clamped L, the segments walked (bits)
    uint32_t* rng_out;   // per slot: the state the path ended with, or null
    uint32_t* count;     // the output list's length: zero before the launch
};

// The chunk's cs x n paths into `out`, sample-major: the n rays copied cs times, throughput 1, L = 0.  rng_state given
// (cs = 1): the state of ray i is rng_state[i]; null: path_seed(i, sample0 + s_local, seed).
void prt_launch_rd_start(hipStream_t st, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* origins,
                         const float* dirs, const uint32_t* rng_state, PrtRadianceList out);
// One round over the n live entries of `in`, whose closest hits are a.hits[0 .. n): miss, emission, scatter, roulette.  A
// path that ends writes its slot; a survivor is appended to `out`, which never shares a buffer with `in`.
void prt_launch_rd_step(hipStream_t st, uint32_t n, PrtRadianceList in, const PrtRadianceArgs& a, PrtRadianceList out);
// rgb_sum[i] (and segments[i], unless null) += the cs slots of ray i in ascending sample order; first: from zero.
void prt_launch_rd_sum(hipStream_t st, uint32_t n, uint32_t cs, bool first, const float4* slots, float* rgb_sum, uint32_t* segments);

// prt_probe_sh.h — launcher prototypes of the SH probes (prt_probe_sh.hip; include/prt.h "SH probes").  No kernel syntax here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/prt.h"

// counts: PRT_PROBE_SH_COUNTERS words, zero before the first launch of a call
#define PRT_PROBE_SH_CNT_SEGMENTS 0u  // two words: the 64-bit sum of the paths' segments
#define PRT_PROBE_SH_COUNTERS 4u

// The rays of cs samples of n probes, sample-major (ray s_local * n + p): o = the probe's position, d = the uniform
// direction of path_seed(p, sample0 + s_local, seed), rng = the advanced state.  pos, o, d: 3 floats each.
void prt_launch_sh_rays(hipStream_t st, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const float* pos, float* o, float* d,
                        uint32_t* rng);
// sh_sum[p][k][c] (+)= fl(rgb_c * Y_k(d)) of the cs samples of probe p in ascending sample order (first: from 0.0f), for
// k < K = (order + 1)^2; the segments go to the counter.
void prt_launch_sh_project(hipStream_t st, uint32_t n, uint32_t cs, uint32_t K, bool first, const float* d, const float* rgb, const uint32_t* seg,
                           float* sh_sum, uint32_t* counts);

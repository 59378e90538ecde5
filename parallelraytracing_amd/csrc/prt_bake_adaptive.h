// prt_bake_adaptive.h — launcher prototypes of the bake's statistics and block-adaptive sampling (prt_bake_adaptive.hip;
// include/prt.h "Bake statistics and adaptive sampling").  No kernel syntax here.
#pragma once
#include "prt_bake.h"

// The per-texel maps of an adaptive bake (W x H entries each, rgb 3 per texel): the colour sum, the sample count as an exact
// fp32 integer, and the moments A = sum of y, Q = sum of y^2 of the samples' luminance.
struct PrtBakeMoments {
    float* rgb_sum;
    float* count;
    float* sum_y;
    float* sum_y2;
};

// sel: PRT_BKA_COUNTERS words, zero before prt_launch_bka_select.  Word PRT_BAKE_CNT_COVERED is left to prt_launch_bk_compact,
// which writes the length of the texel list there.
#define PRT_BKA_CNT_ACTIVE 0u     // the length of the block list (written by the block compaction)
#define PRT_BKA_CNT_CONVERGED 3u  // blocks of prev the rule stopped
#define PRT_BKA_CNT_CAPPED 4u     // blocks of prev still active, counted only where the launch says the cap is reached
#define PRT_BKA_COUNTERS 8u

// k_bk_sum with statistics: the cs values of entry k in ascending sample order into rgb_sum, sum_y, sum_y2 and count of
// texel list[k] (first: from 0.0f); the segments go to counts[PRT_BAKE_CNT_SEGMENTS].
void prt_launch_bka_sum(hipStream_t st, uint32_t n, uint32_t cs, bool first, const uint32_t* list, const float* rgb, const uint32_t* seg,
                        PrtBakeMoments m, uint32_t* counts);
// One wave per entry of prev (null: blocks 0 .. n_prev - 1): flags[i] = 1 iff block prev[i] holds a texel with cov == 1 that
// the rule calls unconverged; active[t] = 1 iff cov[t] == 1 and t's block is active, for the texels of the blocks of prev.
void prt_launch_bka_select(hipStream_t st, uint32_t W, uint32_t H, const uint8_t* cov, PrtBakeMoments m, const uint32_t* prev, uint32_t n_prev,
                           float threshold, float noise_floor, bool at_cap, uint32_t* flags, uint8_t* active, uint32_t* sel);
// out = the flagged entries of prev in prev's order, 0xFFFFFFFF in the entries past them up to n_prev;
// sel[PRT_BKA_CNT_ACTIVE] = how many.
void prt_launch_bka_blocks(hipStream_t st, uint32_t n_prev, const uint32_t* prev, const uint32_t* flags, uint32_t* out, uint32_t* sel);
// rgb_mean[t] = rgb_sum[t] / count[t] per component, 0 where count[t] is 0.
void prt_launch_bka_mean(hipStream_t st, uint32_t n_texels, const float* rgb_sum, const float* count, float* rgb_mean);

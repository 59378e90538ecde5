// prt_bake.h — launcher prototypes of surface baking (prt_bake.hip; include/prt.h "Surface baking").  No kernel syntax here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/prt.h"

// The target's faces as the host lays them out per call, in FACE order: 6 floats of UV (u0 v0 u1 v1 u2 v2), 9 floats of
// position and 9 of vertex normal per face, in the mesh's own space.  placed: the copy's Mat / Inv (rows 0..2 of the
// column-major mat4, DevInstance's layout) apply to the interpolated position and normal.
struct PrtBakeFaces {
    const float* uv;
    const float* pos;
    const float* nrm;
    uint32_t n_faces;
    uint32_t placed;
    float mat[12];
    float inv[12];
};

// The map's per-texel arrays (W x H texels, texel t = row * W + column, row 0 on top).  owner: the lowest covering face,
// 0xFFFFFFFF for none; cov: 0 / 1; the rest is zero where cov is 0.
struct PrtBakeMap {
    uint32_t W, H;
    uint32_t* owner;
    uint8_t* cov;
    float* bary;      // 2 per texel: b1, b2
    float* position;  // 3 per texel, world space
    float* normal;    // 3 per texel, unit, world space
};

// counts: PRT_BAKE_COUNTERS words, zero before the first launch of a call
#define PRT_BAKE_CNT_SKIPPED 0u     // faces with A2 == 0 or a non-finite UV
#define PRT_BAKE_CNT_DEGENERATE 1u  // texels whose interpolated normal has no direction
#define PRT_BAKE_CNT_COVERED 2u     // the length of the texel list
#define PRT_BAKE_CNT_FILLED 3u      // texels the gutter fill wrote
#define PRT_BAKE_CNT_SEGMENTS 4u    // two words: the 64-bit sum of the paths' segments
#define PRT_BAKE_COUNTERS 8u

// owner[t] = the lowest face whose UV triangle covers the centre of texel t (owner is 0xFFFFFFFF everywhere before).
void prt_launch_bk_cover(hipStream_t st, const PrtBakeFaces& f, PrtBakeMap m, uint32_t* counts);
// Barycentrics, position and normal of every owned texel; a degenerate texel gives its owner up.
void prt_launch_bk_surface(hipStream_t st, const PrtBakeFaces& f, PrtBakeMap m, uint32_t* counts);
// list = the texels with cov != 0 in ascending order, counts[PRT_BAKE_CNT_COVERED] = their number.
void prt_launch_bk_compact(hipStream_t st, uint32_t n_texels, const uint8_t* cov, uint32_t* list, uint32_t* counts);
// The rays of cs samples of n entries, sample-major (ray s_local * n + k): entry k is texel list[k], or texel k of the
// whole map with list == null (zeros where cov is 0).  o, d: 3 floats per ray, rng: the advanced state.
void prt_launch_bk_rays(hipStream_t st, uint32_t n, uint32_t cs, uint32_t sample0, uint32_t seed, const uint32_t* list, PrtBakeMap m,
                        float* o, float* d, uint32_t* rng);
// rgb_sum[list[k]] (+)= the cs values of entry k in ascending sample order (first: from 0.0f); the segments go to the counter.
void prt_launch_bk_sum(hipStream_t st, uint32_t n, uint32_t cs, bool first, const uint32_t* list, const float* rgb, const uint32_t* seg,
                       float* rgb_sum, uint32_t* counts);
// One pass of the gutter fill from (cov_in, rgb_in) into (cov_out, rgb_out), which are other buffers.
void prt_launch_bk_dilate(hipStream_t st, uint32_t W, uint32_t H, const uint8_t* cov_in, const float* rgb_in, uint8_t* cov_out, float* rgb_out,
                          uint32_t* counts);

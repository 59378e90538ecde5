// prt_temporal.h — launcher prototypes of the temporal reprojection (prt_temporal.hip) and the record layout they share
// with prt_api.cpp.  No kernel syntax here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "../../include/prt.h"
#include "prt_kernels.h"  // PrtTileMap

// One frame's history, Film layout (pixel = y * W + x): 56 bytes per pixel.
//   cn   {colour r, g, b, history length in samples}
//   mm   {first, second luminance moment}
//   nrm  {normal x, y, z, prim as its int32 bit pattern}   (PrtFeatureBufs' layout)
//   pos  {position x, y, z, -}
struct PrtHistoryBufs {
    float4* cn;
    float2* mm;
    float4* nrm;
    float4* pos;
};

// The placed copies a pixel's previous surface is looked up in: range = n records {prim_base, n_tris}, ascending; xf = n
// records of 6 float4: the copy's current inverse (12 floats), then its previous matrix (12 floats).  n = 0: nothing moved.
struct PrtMotionTable {
    const uint32_t* range;
    const float4* xf;
    uint32_t n;
};

// The current frame of the array entry points: cn {c, n}, aq {A, Q}, nrm {Nprev, prim}, pos {Pprev, -}.
struct PrtTemporalFrame {
    const float4* cn;
    const float2* aq;
    const float4* nrm;
    const float4* pos;
};

// Planar arrays -> records.  c / P / N: 3 floats per pixel.
void prt_launch_tp_pack_frame(hipStream_t st, uint32_t n, const float* c, const float* w, const float* A, const float* Q, const int32_t* prim,
                              const float* P, const float* N, float4* cn, float2* aq, float4* nrm, float4* pos);
// History records -> planar N', m1', m2'.
void prt_launch_tp_unpack(hipStream_t st, uint32_t n, PrtHistoryBufs h, float* n_out, float* m1_out, float* m2_out);
// One reprojection of W x H pixels.  prev.cn == null: no history at all.  Writes next (never the buffers of prev), the planar
// mean (3 floats) and, where not null, var, status and counts[0] += hit pixels, counts[1] += pixels with status 1.
void prt_launch_tp_reproject(hipStream_t st, uint32_t W, uint32_t H, const PrtTemporal& cfg, const PrtCameraBasis& K, PrtTemporalFrame cur,
                             PrtHistoryBufs prev, PrtHistoryBufs next, float* mean, float* var, uint8_t* status, uint32_t* counts);
// The same for the context's own film (tm.world == 1) and moments, with the features' records as the current surface and
// the previous surface of a placed copy's pixel evaluated inline from mt.
void prt_launch_tp_reproject_film(hipStream_t st, const PrtTileMap& tm, const PrtTemporal& cfg, const PrtCameraBasis& K,
                                  const float4* film_local, const float2* film_stat, const float4* feat_nrm, const float4* feat_pos,
                                  PrtMotionTable mt, PrtHistoryBufs prev, PrtHistoryBufs next, float* mean, float* var, uint8_t* status,
                                  uint32_t* counts);

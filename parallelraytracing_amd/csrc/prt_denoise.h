// prt_denoise.h — launcher prototypes of the feature pass and of the a-trous film denoiser (prt_denoise.hip), and the
// record layout they share with prt_api.cpp.  No kernel syntax here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "../../include/prt.h"
#include "prt_kernels.h"  // PrtTileMap

// Three 16-byte records per pixel, Film layout (pixel = y * W + x):
//   alb  {albedo r, g, b, 0}
//   nrm  {normal x, y, z, prim as its int32 bit pattern}   (prim < 0: a miss)
//   pos  {position x, y, z, depth}
struct PrtFeatureBufs {
    float4* alb;
    float4* nrm;
    float4* pos;
};

// What one a-trous iteration needs beside the buffers (PrtDenoise, include/prt.h).
struct PrtAtrousParams {
    uint32_t W, H, step;
    float sigma_l, sigma_z;
    uint32_t normal_power_log2;
};

// px[i] = x + 0.5f, py[i] = y + 0.5f for pixel i = y * W + x: the pixel-centre grid prt_launch_camera_rays is given.
void prt_launch_dn_pixel_grid(hipStream_t st, uint32_t W, uint32_t H, float* px, float* py);
// The feature records from the hit records of the centre rays.  albedo: prt_launch_hit_uv's output (3 floats per ray)
// while a binding textures something, else null: the material's constant rgb is gathered.
void prt_launch_dn_pack_features(hipStream_t st, uint32_t n, const PrtHit* hits, const float* albedo, const float4* mat_rgbs,
                                 const uint32_t* mat_type, PrtFeatureBufs out);
// The records from planar arrays (prt_denoise / prt_denoise_device); depth is not an input (0).
void prt_launch_dn_pack_arrays(hipStream_t st, uint32_t n, const float* albedo, const float* normal, const float* position,
                               const int32_t* prim, PrtFeatureBufs out);
// c_0 / var_0 as {r, g, b, var} from planar mean (3 floats) and var, demodulated if asked.
void prt_launch_dn_prepare(hipStream_t st, uint32_t n, const float* mean, const float* var, PrtFeatureBufs f, uint32_t demodulate,
                           float4* cv);
// The same from the context's own film (tm.world == 1) and its moments: mean = rgb_sum / weight, var = the contract's rule.
void prt_launch_dn_film_prepare(hipStream_t st, const PrtTileMap& tm, const float4* film_local, const float2* film_stat,
                                PrtFeatureBufs f, uint32_t demodulate, float4* cv);
// One iteration: cv_in -> cv_out (never the same buffer).
void prt_launch_dn_atrous(hipStream_t st, const PrtAtrousParams& p, const float4* cv_in, PrtFeatureBufs f, float4* cv_out);
// The same iteration with the block's footprint staged in LDS: what step 1 runs by default (measured faster there on an
// MI355X, slower at step 2: prt_set_param("denoise_lds", n), tools/denoise_rate.py).  Steps 1 and 2 only; false (nothing
// launched) for any other step.
bool prt_launch_dn_atrous_lds(hipStream_t st, const PrtAtrousParams& p, const float4* cv_in, PrtFeatureBufs f, float4* cv_out);
// out = c_K (* rho), var_out = var_K (* lum(rho)^2): planar arrays; var_out may be null.
void prt_launch_dn_finish(hipStream_t st, uint32_t n, const float4* cv, PrtFeatureBufs f, uint32_t demodulate, float* out,
                          float* var_out);

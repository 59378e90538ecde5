// prt_kernels.h — POD types shared by the HIP kernels (prt_kernels.hip) and the C-ABI host code
// (prt_api.cpp), plus the launcher prototypes.  No kernel syntax here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

#include "../../include/prt.h"
#include "prt_path_id.h"    // how a batch numbers its paths: (local pixel, sample) <-> path id
#include "prt_route.h"      // the instance lists and the plan of a batch
#include "prt_walk.h"       // PrtTravTuning; the walk kernels' instance lists and the plan of a tree walk
#include "prt_scene_pod.h"  // DevPrim, DevInstance

struct f3 {
    float x, y, z;
};

struct DevCamera {  // the Camera members GetCameraRay reads (reference: src/core/camera.h:134-141)
    f3 pos, front, right, up;
    float W, H, tan_fov_y;  // tan_fov_y: tanf(0.5f) (the reference's 1 rad), or tanf(0.5f * PrtLens.fov_y)
};
// Thin lens (PrtLens, include/prt.h "Thin lens and field of view"), passed only to the kernel instances of its own
// (k_raygen_lens, k_raygen_lens_env, k_camera_rays_lens) while aperture > 0: DevCamera and the other instances stay as they are.
struct DevLens {
    float aperture, focus;
};

// Smallest |component| of a unit direction that the slab tests of every walk divide by (a smaller one, zero included, is
// replaced by +-PRT_DIR_MIN with its sign).  Conservative: along such an axis the ray moves less than t * 2^-40, and every
// t that can matter is below 2 (|o|_1 + extent), so the ray stays within 2^-39 (|o|_1 + extent) of its origin, 2^-21 of
// the per-ray pad 2^-18 (|o|_1 + extent) the planes are moved out by; the slab of a box the ray can hit therefore still
// contains [0, t].  Scale-free, and the reciprocal is at most 2^40: (coordinate +- pad) * 2^40 and cell * 2^40 stay finite
// for every coordinate whose squared distances are finite (< 2^63).  (It was 1e-30: (o +- pad) * 1e30 overflowed once a
// coordinate exceeded 3.4e8, the slab became [-inf, -inf] and the root was culled: DESIGN.md section 0b.)
#define PRT_DIR_MIN 9.094947017729282e-13f  // 2^-40

struct DevScene {
    const DevPrim* prims;
    const float4* mat_rgbs;     // rgb + scalar
    const uint32_t* mat_type;
    const float4* nodes;        // 4 x float4 per BVH2 node (see bvh.h)
    const float4* nodes4;       // 8 x float4 per BVH4 node (see bvh.h)
    const uint4* nodes8;        // 5 x uint4 per compressed 8-wide node (see bvh.h); null if the tree has none
    const float4* tris;         // 3 x float4 per triangle, leaf order: {P0, prim}, {P1, material}, {P2, 0}
    const float4* tri_normals;  // 3 x float4 per triangle, leaf order
    // BVH over the ANALYTIC primitives' world boxes (scenes with many of them, e.g. the RANDOM_BALLS presets: the
    // reference scans all of them per ray, primitive.cpp:26): 4-wide nodes in the bvh.h layout, leaf slot -> primitive
    const float4* abvh_nodes;   // null: the producers scan the primitives linearly
    const uint32_t* abvh_order;
    const DevInstance* insts;   // placed mesh copies; with n_insts > 0 nodes8 starts with a top-level tree over them
    const uint32_t* tlas_inst;  // top-level leaf slot -> instance index
    uint32_t n_insts;
    uint32_t node_stride;       // uint4 per 8-wide node slot: 5 (packed, 80 B) or 8 (one node per 128-B line: big trees, see upload_scene)
    uint32_t depth8;            // levels of the 8-wide tree (two-level scenes: top level + deepest mesh tree)
    uint32_t n_prims;
    uint32_t n_nodes;
    uint32_t n_tris;
    float pad;     // culling pad coefficient (2^-18): pad_ray = pad * (|o|_1 + extent)
    // primitive walk only: + (abvh_q[0] * A + abvh_q[1]) * A + abvh_q[2] with A = |o|_1, an upper envelope of
    // K / R_i * (A + |c_i|_1)^2 over the scene's spheres (world radius R_i, centre c_i): how far OUTSIDE a sphere a ray may
    // pass and still be a hit in the reference's fp32 arithmetic (see build_prim_bvh in prt_scene.cpp)
    float abvh_q[3];
    float extent;  // max |coordinate| of any mesh vertex
    float root_min[3], root_max[3];  // bounds of all triangles (BVH root box)
    float sky[3];
};

struct PrtTileMap {
    uint32_t W, H, tiles_x, tiles_y, rank, world;
    uint32_t n_tiles_local;  // tiles owned by this rank
    uint32_t n_pix_local;    // n_tiles_local * 64
    uint32_t stride;         // ceil(tiles_total / world) * 64: per-rank payload (float4 units), equal on all ranks
};

// What a batch renders (run_batch, prt_api.cpp).  list = null: the whole film, tm = the context's tile map.  list != null (a
// pass of prt_render_adaptive): the ascending local tile indices that are still active; tm is the context's tile map with
// n_tiles_local = the number of listed tiles and n_pix_local = 64 x that, so compact local pixel pl (what path ids and ray
// grids are made of) is lane pl & 63 of local tile list[pl >> 6], film pixel (list[pl >> 6] << 6) + (pl & 63) of film_local.
struct PrtBatchView {
    PrtTileMap tm;
    const uint32_t* list;
};

// Timeline of one launch of the instrumented 8-wide kernel, in s_memrealtime ticks (100 MHz), 8 words per launch:
// (of XCD 0's waves:) [0] first wave start (min), [1] last wave end (max), [2] / [3] first / last wave to find the ray buffer exhausted,
// [4] sum over waves of (end - exhausted) = wave time spent draining, [5] sum over waves of (end - start), [6] waves,
// [7] node steps of the longest ray
#define PRT_TIMELINE_WORDS 8
// k_accumulate's per-depth ray counters exist PRT_RAY_STAT_SLOTS times ([slot][PRT_MAX_DEPTH], block b adds to slot
// b mod SLOTS); the host sums the slots when it reads them
#define PRT_RAY_STAT_SLOTS 256u

struct PrtRayBuf {
    float4* o;      // origin.xyz, path id
    float4* d;      // direction.xyz, rng state
    float4* t;      // throughput.rgb, -
    uint32_t* hit;  // closest-hit id so far (producer: analytic scan; traversal: final)
    float* hd2;     // its world distance^2
};

// Compact primary rays.  Without jitter the primary ray of a path, its RNG seed, throughput (1,1,1) and segment index
// (0) are functions of the path id alone, so k_raygen stores 12 B per path (path id, the analytic scan's hit id and
// distance) instead of 56 B plus ONE 16-B record per pixel (direction, pixel index), and the first bounce's traversal
// and k_shade rebuild the ray from those (C3: 372 M stored primary rays per 256-spp batch = 16 GB less written by
// k_raygen and 12 GB less read by the first k_shade; round 3: the analytic scan's hit of a primary ray is per pixel too, so a
// path's slot holds its id only).  pid aliases the `t` array of the ray buffer (first 4 bytes per slot).
// One walk per pixel (walk = 1, the default; prt_set_param("primary_walk", 0) restores one walk per sample): all samples
// of a pixel share the pixel-centre ray, so k_raygen also writes a dense LIST of the front pixels (local pixel index = the
// path id of the pixel's sample 0; its counter is word PRT_CNT_LIST of bounce 0's counters), the first traversal runs
// over that list (its PrtPrimary has pid = the list) and leaves the closest hit in hit[list slot], and the first k_shade
// and k_primary_hit take a front path's hit from there through the pixel's end record.  The list lives in the hd2 array of
// bounce 0's ray buffer and the hits in its hit array: compact k_raygen writes neither per ray slot.
struct PrtPrimary {
    const uint32_t* pid;  // path id per ray slot (the traversal's copy with walk = 1: per list slot)
    const float4* pix;    // per local pixel: camera-ray direction, pixel index y * W + x (bits); then n_pix_local more records:
                          // what the pixel's paths deliver if they end with their primary ray (read by k_accumulate; for
                          // pixels whose paths go on: y, z = the analytic scan's hit and distance^2, x = the pixel's list
                          // slot, 0xFFFFFFFF for a back pixel; with walk = 0 the ray slot of the first stored sample); then
                          // 2 x n_pix_local more: the primary hit's surface interaction (k_primary_hit): {position, hit id},
                          // {normal, material | front << 31}
    float origin[3];      // camera position
    PrtPathIdOrder ids;   // the batch's path ids (prt_path_id.h; n_pix_local is in there).  The traversal's copy with walk = 1:
                          // always sample-major, a list entry is a local pixel = the sample-major id of its sample 0
    uint32_t first_sample, seed;
    uint32_t walk;        // 1: the first traversal walked one ray per front pixel (hit[] is indexed by list slot), 0: one per path slot
};

// The PATH instance of k_traverse8_persistent (small batches: the reference's one sample per ProgressiveRender call): ONE
// persistent launch carries whole paths.  A lane generates its path's primary ray, walks it, shades the hit when the walk is
// over (advance_path, the code of k_shade) and goes on with the scattered ray, until the path ends (rad[path] written) and
// the lane takes the next path.  What the launch needs beyond the scene:
struct PrtPathArgs {
    DevCamera cam;
    PrtTileMap tm;
    PrtSampling sp;
    float4* rad;
    uint32_t first_sample, seed, max_depth, n_paths;
};

#define PRT_CNT_STRIDE 64u  // uint32 per bounce in the counter array: [0] front, [32] back, [16] finished-in-producer counts, [48] shadow rays (lighting modes)
#define PRT_CNT_LIST 8u     // bounce 0 only: entries of the front-pixel list (PrtPrimary, walk = 1)

// Light table (PrtLighting, include/prt.h), read-only, PRT_LIGHT_F4 = 5 (prt_scene_pod.h) x float4 per light:
//   [0] centre.xyz, R (sphere) | area w h s^2 (quad)   [1] edge u = w * column 0 of Mat, pmf   [2] edge v = h * column 2, cdf
//   [3] unit normal of the quad plane, kind (0 sphere, 1 quad; bits)   [4] emission rgb, primitive index (bits)
// prim_light[p]: light index of analytic primitive p, 0xFFFFFFFF if it is not in the light set.  Passed only to the
// lighting kernels (DevScene stays as it is: the lighting-off instances keep their code).
struct DevLights {
    const float4* lights;
    const uint32_t* prim_light;
    uint32_t n_lights;
    uint32_t mode;  // PRT_LIGHTING_NEE_MIS / PRT_LIGHTING_NEE
};
// Triangle lights (prt_set_light_sources with PRT_LIGHT_SOURCES_MESH; host side: PrtMeshLights, prt_scene.h).  DevLights
// then holds the CANDIDATE table (same records; triangles: [0] v0, area  [1] e1, pmf  [2] e2, -  [3] n_g, kind 2
// [4] emission, primitive index) with n_lights = the candidates the search can return, and this goes with it, to the
// kernel instances of their own that sample triangles (the default instances keep their arguments and their code):
//   thr[i] = T_{i+1}: the light of the 32-bit draw r0 is the smallest i with r0 < thr[i], else n_lights - 1
//   bucket[r0 >> bucket_shift] .. bucket[(r0 >> bucket_shift) + 1] brackets that i (null: search all of thr)
//   runs: per emissive mesh / placed copy, ascending prim_first: triangle with global primitive index p in
//   [prim_first, prim_first + n_tris) is candidate light_first + (p - prim_first)
struct DevLightRun {
    uint32_t prim_first, n_tris, light_first, world;
};
struct DevMeshLights {
    const uint32_t* thr;
    const uint32_t* bucket;
    const DevLightRun* runs;
    uint32_t bucket_shift;
    uint32_t n_runs;
};
// Clustered light selection (PrtLightSelection, include/prt.h; host side: PrtLightClusters, prt_scene.h), passed only to
// the kernel instances of its own (k_shade_nee_clus*, k_sample_light_test_clus*, k_light_cluster_pmf) beside DevLights /
// DevMeshLights.  boxes: per cluster {lo.xyz, phi}, {hi.xyz, r2}; range: per cluster {first member, last member with a
// non-empty inner interval, members, 0}; members: cluster-major, the candidate; thr: cluster-major, U_{c,j} of member j (the
// member of the 32-bit draw r3 is the smallest j in [first, last] with r3 < thr[j], else last); per candidate its cluster
// (0xFFFFFFFF: none) and fl32 pmf_in (with the environment's factor).
struct DevLightClusters {
    const float4* boxes;
    const uint4* range;
    const uint32_t* members;
    const uint32_t* thr;
    const uint32_t* cand_cluster;
    const float* cand_pmf_in;
    uint32_t n_clusters;
};
// Environment light (PrtEnvironment, include/prt.h; host side: PrtEnvTables, prt_scene.h), passed only to the kernel
// instances of its own (k_raygen_env, k_shade_env, k_shade_nee_env, k_shade_nee_mesh_env): DevScene and the other instances
// stay as they are.  texels: rgb, pdf_w x sin(theta) of the texel; row_thr / col_thr: the 32-bit thresholds, searched up to
// row_last / col_last[row] (the last entry's 2^32 is implicit).
struct DevEnv {
    const float4* texels;
    const uint32_t* row_thr;
    const uint32_t* col_thr;
    const uint32_t* col_last;
    uint32_t W, H;
    uint32_t row_last;
    uint32_t t_env;    // low 32 bits of T_e: the environment is sampled iff t_all or r_e < t_env
    uint32_t t_all;    // T_e = 2^32
    float p_env;       // fl(T_e / 2^32)
};

// Image textures (PrtTextureSet, include/prt.h "Image textures"; host side: PrtTexTables, prt_scene.h), passed only to the
// kernel instances of its own (k_shade_tex, k_shade_nee_tex, k_texture_eval, k_hit_uv): DevScene and the other instances
// stay as they are.  texels: one pool, rgb + 0; desc[t] = {first texel, W, H, filter | wrap << 1}; mat_tex[material] = texture
// or PRT_TEXTURE_NONE; uvs: 3 x float2 per mesh triangle in FACE order, the world-space meshes first (entry = the global
// primitive index the record carries - n_prims), then every instanced mesh once; inst_uv_base[instance] + the index the
// record carries is the entry of a triangle met through an instance (unsigned arithmetic; null without placed copies).
struct DevTex {
    const float4* texels;
    const uint4* desc;
    const uint32_t* mat_tex;
    const float2* uvs;
    const uint32_t* inst_uv_base;
    uint32_t n_textures;
};

// What the lighting shade step needs beyond k_shade's arguments: the shadow-ray buffer (o = x, path id; d = w, -;
// t = clamped contribution rgb, tmax; hit / hd2 seeded as k_pack_occlusion_rays seeds them), the per-path pdf of the
// previous scatter (pB, < 0: the previous vertex was not Lambertian) and the per-path light radiance.
struct PrtLightBufs {
    PrtRayBuf sh;
    float* pdf_b;
    float4* lrad;
    unsigned long long* stats;  // [PRT_RAY_STAT_SLOTS][2]: shadow rays, occluded (block b adds to slot b mod SLOTS)
};

// The three stage launchers of a batch.  Each takes the instance prt_plan_route (prt_route.h) chose and one argument struct;
// the optional pointers are read only by the instances whose kernels take them (null otherwise).  false: no such instance.
struct PrtRaygenArgs {
    const DevScene* sc;
    DevCamera cam;
    PrtTileMap tm;
    uint32_t n_paths, first_sample, seed, max_depth;
    PrtRayBuf out;
    float4* rad;
    uint32_t* counts;
    uint32_t* work;
    PrtSampling sp;
    float4* compact_pix;   // the compact instance: the pixel records (PrtPrimary.pix)
    bool primary_walk;     // the compact instance: write the front-pixel list into out.hd2 (PrtPrimary)
    bool pixel_major_ids;  // the compact instance: path id = pixel * S + sample (prt_path_id.h)
    const DevEnv* env;     // the instances with an environment image
    const DevLens* lens;   // the instances with a thin lens (one full record per sample)
    const uint32_t* list;  // k_raygen_list: the tiles of a PrtBatchView
};
bool prt_launch_raygen(hipStream_t st, PrtRaygenInst inst, const PrtRaygenArgs& a);
void prt_launch_scan_prims(hipStream_t st, const DevScene& sc, const PrtRayBuf& in, const uint32_t* count_ptr,
                           uint32_t* work, uint32_t max_rays, unsigned long long* stats);
// A tree walk of a prepared ray buffer (analytic scan done, hit / hd2 seeded): the launches of prt_plan_walk's plan (prt_walk.h),
// closest hit, any-hit (prt_occluded, shadow rays) or seeded any-hit alike.
struct PrtWalkArgs {
    const DevScene* sc;
    PrtRayBuf rays;
    const uint32_t* count;      // the rays to walk, on the device
    uint32_t* work;             // cursors, error flags, overflow list
    uint32_t* spill;
    unsigned long long* stats;  // the instrumented launches
    const PrtPrimary* primary;  // the PRIM launch (compact primary rays)
    const PrtTravTuning* tune;  // the caller's tunables (perm, probe_slot); a launch overrides what the plan resolved
};
void prt_launch_walk(hipStream_t st, const PrtWalkPlan& plan, const PrtWalkArgs& a);
// one launch for a whole batch of paths (PrtPathArgs, the plan of a PRT_WALK_PATH request); `work` (cursors + error flags) must
// have been zeroed on the stream
void prt_launch_path(hipStream_t st, const PrtWalkPlan& plan, const DevScene& sc, const PrtPathArgs& pa, uint32_t* work, const PrtTravTuning& tune);
int prt_walk_occupancy(const PrtWalkPlan& plan, int* blocks_per_cu, int* vgprs, int* sgprs, int* lds_bytes);
// The last-segment route reaches k_shade / k_shade_env / k_shade_tex as this bit of their max_depth argument (a run-time flag:
// their instances and names stay what they are); max_depth itself is at most PRT_MAX_DEPTH.
#define PRT_LAST_SEGMENT_FLAG 0x80000000u
struct PrtShadeArgs {
    const DevScene* sc;
    PrtRayBuf in, out;
    float4* rad;
    uint32_t* counts;
    uint32_t* work;
    uint32_t depth, max_depth, cap;
    PrtSampling sp;
    uint32_t n_rays_known;             // the bounce's ray count if the host has it (0xFFFFFFFF: the grid is sized for `cap`)
    const PrtPrimary* primary;         // bounce 0 of compact primary rays
    uint32_t last_segment;             // PrtRoutePlan.last_segment: non-zero sets PRT_LAST_SEGMENT_FLAG in the max_depth of k_shade / _env / _tex
    const DevEnv* env;
    const DevTex* tex;
    const DevLights* lights;           // lighting modes: the shade step takes a light sample per Lambertian vertex (shadow rays
    const DevMeshLights* mesh_lights;  // into lb->sh, counted in counts[depth * stride + 48]); mesh_lights: triangle lights
    const PrtLightBufs* lb;
    const DevLightClusters* clusters;  // clustered light selection (the k_shade_nee_clus* instances)
};
bool prt_launch_shade(hipStream_t st, PrtShadeInst inst, const PrtShadeArgs& a);
// diagnostic: per-wave material mix of what k_shade of bounce `iter` is about to shade (16 words per bounce in `out`)
void prt_launch_shade_divstats(hipStream_t st, const DevScene& sc, const PrtRayBuf& in, const uint32_t* counts, uint32_t iter,
                               uint32_t cap, unsigned long long* out, const PrtPrimary* primary = nullptr);
// compact primary rays: per-pixel surface interaction of the primary hit (records 2n.. and 3n.. of `pix`), between the
// first traversal and the first k_shade of a batch
void prt_launch_primary_hit(hipStream_t st, const DevScene& sc, const PrtPrimary& pr, const uint32_t* hit, float4* pix,
                            const uint32_t* counts);
// film += the batch's samples.  k_accumulate (pix_end optional), k_accumulate_lit (rad + lrad), or k_accumulate_stat<LIT, LIST>,
// which also adds every sample's luminance and its square to stat[pixel] = {A, Q} and with `list` scatters pixels through it.
struct PrtAccumulateArgs {
    const float4* rad;
    const float4* lrad;  // the paths' light radiance (lit instances)
    float4* film_local;
    float2* stat;
    PrtTileMap tm;
    uint32_t S, max_depth;
    bool update_film;
    unsigned long long* ray_stats;
    const float4* pix_end;  // compact primary rays: what a pixel's paths deliver if they end with their primary ray
    const uint32_t* list;
    bool pixel_major_ids;   // compact primary rays: rad[] is indexed pixel * S + sample (prt_path_id.h)
};
bool prt_launch_accumulate(hipStream_t st, PrtAccumulateInst inst, const PrtAccumulateArgs& a);
void prt_launch_resolve(hipStream_t st, const float4* gathered, uint32_t world, uint32_t stride, uint32_t W,
                        uint32_t H, float* rgb, float* weight);
void prt_launch_tonemap(hipStream_t st, const float* rgb, const float* weight, uint32_t n_pix, float exposure,
                        float inv_gamma, uint8_t* out);
void prt_launch_camera_rays(hipStream_t st, const DevCamera& cam, uint32_t n, const float* px, const float* py,
                            float* o, float* d);
// prt_camera_rays_lens: lens_camera_ray for n points; keys (RNG states) are advanced in place
void prt_launch_camera_rays_lens(hipStream_t st, const DevCamera& cam, const DevLens& lens, uint32_t n, const float* px,
                                 const float* py, uint32_t* keys, float* o, float* d);
void prt_launch_pack_rays(hipStream_t st, uint32_t n, const float* o, const float* d, const PrtRayBuf& out,
                          uint32_t* counts);
void prt_launch_hit_records(hipStream_t st, const DevScene& sc, uint32_t n, const PrtRayBuf& in, PrtHit* out);
// occlusion queries (prt_occluded): pack + seed (hit = HIT_MISS at hd2 = tmax^2, or HIT_DEAD), the analytic scan from that
// bound, the any-hit walk, one byte per ray
void prt_launch_pack_occlusion_rays(hipStream_t st, uint32_t n, const float* o, const float* d, const float* tmax,
                                    const PrtRayBuf& out, uint32_t* counts);
void prt_launch_scan_prims_bounded(hipStream_t st, const DevScene& sc, const PrtRayBuf& in, const uint32_t* count_ptr,
                                   uint32_t* work, uint32_t max_rays);
void prt_launch_occlusion_bytes(hipStream_t st, const DevScene& sc, uint32_t n, const PrtRayBuf& in, const float* tmax,
                                uint8_t* out);
void prt_launch_scatter_test(hipStream_t st, const DevScene& sc, uint32_t n, const float* in_d, const PrtHit* hits,
                             uint32_t* rng_io, uint32_t* scattered, float* atten, float* emitted, float* o_out,
                             float* d_out);
// lighting modes (PrtLighting): after the shadow walk, the unoccluded contributions into lb.lrad (and the traversal cursors
// reset for the next bounce)
void prt_launch_light_accum(hipStream_t st, const DevScene& sc, const PrtLightBufs& lb, const uint32_t* count_ptr,
                            uint32_t* work, uint32_t max_rays);
void prt_launch_sample_light_test(hipStream_t st, const DevScene& sc, const DevLights& lt, uint32_t n, const float* in_d,
                                  const PrtHit* hits, const uint32_t* keys, float* out_f, uint32_t* out_light,
                                  const DevMeshLights* ml = nullptr, const DevEnv* env = nullptr, const DevLightClusters* lc = nullptr);
// prt_light_cluster_pmf: the cluster thresholds M_c of n points (3 floats each), n x n_clusters
void prt_launch_light_cluster_pmf(hipStream_t st, const DevLightClusters& lc, uint32_t n, const float* x, uint32_t* M);
// prt_environment_eval: lookup of n directions (3 floats each): rgb (3 floats), texel, pdf_w; any output may be null
void prt_launch_environment_eval(hipStream_t st, const DevEnv& env, uint32_t n, const float* dirs, float* rgb, uint32_t* texel,
                                 float* pdf_w);
// Image textures: the two function-level kernels that run the device functions of the texture shade instances
// prt_texture_eval: texture_lookup for n (texture, uv) pairs
void prt_launch_texture_eval(hipStream_t st, const DevTex& tex, uint32_t n, const uint32_t* texture, const float* uv, float* rgb);
// prt_hit_uv: after the closest-hit pipeline on `in`: uv (2 floats) and albedo (3 floats) of every ray's hit; either may be null
void prt_launch_hit_uv(hipStream_t st, const DevScene& sc, const DevTex& tex, uint32_t n, const PrtRayBuf& in, float* uv, float* albedo);

// Film statistics and adaptive sampling (include/prt.h "Film statistics and adaptive sampling")
// k_tile_select + k_tile_compact: of the n_in tiles of `prev` (null: local tiles 0 .. n_in - 1) those with an unconverged pixel
// (prt_adaptive.h), in the same (ascending) order, into `out`; their number into *count.  flags: n_in words of scratch.
void prt_launch_tile_select(hipStream_t st, const float4* film_local, const float2* stat, const PrtTileMap& tm, const uint32_t* prev,
                            uint32_t n_in, float threshold, float noise_floor, uint32_t* flags, uint32_t* out, uint32_t* count);

// prt_route.h — the route of a batch as data: the facts run_batch (prt_api.cpp) collects, the one function that turns them
// into a plan, and the one list of the raygen / shade / accumulate kernel instances a batch can launch.  Plain C++ with no HIP
// header (g++ compiles it alone: tests/route_table.cpp holds every combination of the facts to the table recorded from the
// hand-written launchers this replaced).  The launchers (prt_kernels.hip) expand the same lists into their `case`s, so an
// instance's name and its launch are one spelling.  DESIGN.md section 3 "Routes of a batch" is the table in prose.
#pragma once
#include <cstdint>

#include "prt_walk.h"  // the tree walk's own facts and plan; prt_route_walk8

// One row per instance: T(argument list of the kernel, kernel, tag, template arguments...).  The tag spells the arguments
// (f / t per bool) and makes the enumerator.  A family with every combination of 2, 3 or 4 bools is one PRT_ROWSn line, its rows
// in counting order of the arguments: the plan's index arithmetic relies on that order.
#define PRT_ROWS2(T, s, k) T(s, k, ff, false, false) T(s, k, ft, false, true) T(s, k, tf, true, false) T(s, k, tt, true, true)
#define PRT_ROWS3(T, s, k) \
    T(s, k, fff, false, false, false) T(s, k, fft, false, false, true) T(s, k, ftf, false, true, false) T(s, k, ftt, false, true, true) \
    T(s, k, tff, true, false, false) T(s, k, tft, true, false, true) T(s, k, ttf, true, true, false) T(s, k, ttt, true, true, true)
#define PRT_ROWS4(T, s, k) \
    T(s, k, ffff, false, false, false, false) T(s, k, ffft, false, false, false, true) T(s, k, fftf, false, false, true, false) T(s, k, fftt, false, false, true, true) \
    T(s, k, ftff, false, true, false, false) T(s, k, ftft, false, true, false, true) T(s, k, fttf, false, true, true, false) T(s, k, fttt, false, true, true, true) \
    T(s, k, tfff, true, false, false, false) T(s, k, tfft, true, false, false, true) T(s, k, tftf, true, false, true, false) T(s, k, tftt, true, false, true, true) \
    T(s, k, ttff, true, true, false, false) T(s, k, ttft, true, true, false, true) T(s, k, tttf, true, true, true, false) T(s, k, tttt, true, true, true, true)
#define PRT_RAYGEN_INSTANCES(T) \
    T(PLAIN, k_raygen, fttf, false, true, true, false) \
    T(PLAIN, k_raygen, tttf, true, true, true, false) \
    T(PLAIN, k_raygen, ffff, false, false, false, false) \
    T(PLAIN, k_raygen, ftff, false, true, false, false) \
    T(PLAIN, k_raygen, tfff, true, false, false, false) \
    T(PLAIN, k_raygen, ttff, true, true, false, false) \
    T(COMPACT, k_raygen, ffft, false, false, false, true) \
    PRT_ROWS2(T, ENV, k_raygen_env) \
    PRT_ROWS2(T, LENS, k_raygen_lens) \
    PRT_ROWS2(T, LENS_ENV, k_raygen_lens_env) \
    PRT_ROWS4(T, LIST, k_raygen_list)
#define PRT_SHADE_INSTANCES(T) \
    T(PLAIN, k_shade, 0ffft, 0, false, false, false, true) \
    T(PLAIN, k_shade, 0tftf, 0, true, false, true, false) \
    T(PLAIN, k_shade, 0tttf, 0, true, true, true, false) \
    T(PLAIN, k_shade, 0ttff, 0, true, true, false, false) \
    T(PLAIN, k_shade, 1ffff, 1, false, false, false, false) \
    T(PLAIN, k_shade, 1tfff, 1, true, false, false, false) \
    T(PLAIN, k_shade, 0ffff, 0, false, false, false, false) \
    T(PLAIN, k_shade, 0tfff, 0, true, false, false, false) \
    PRT_ROWS2(T, ENV, k_shade_env) \
    PRT_ROWS3(T, TEX, k_shade_tex) \
    PRT_ROWS2(T, NEE, k_shade_nee) \
    PRT_ROWS2(T, NEE_ENV, k_shade_nee_env) \
    PRT_ROWS2(T, NEE_MESH, k_shade_nee_mesh) \
    PRT_ROWS2(T, NEE_MESH_ENV, k_shade_nee_mesh_env) \
    PRT_ROWS4(T, NEE_TEX, k_shade_nee_tex) \
    PRT_ROWS2(T, NEE_CLUS, k_shade_nee_clus) \
    PRT_ROWS2(T, NEE_CLUS_ENV, k_shade_nee_clus_env) \
    PRT_ROWS3(T, NEE_CLUS_TEX, k_shade_nee_clus_tex)
#define PRT_ACCUMULATE_INSTANCES(N, T) \
    N(PLAIN, k_accumulate) \
    N(LIT, k_accumulate_lit) \
    PRT_ROWS2(T, STAT, k_accumulate_stat)

#define PRT_INST(kernel, tag) PRT_I_##kernel##_##tag
#define PRT_INST_ENUM_N(sig, kernel) PRT_I_##kernel,
#define PRT_INST_ENUM_T(sig, kernel, tag, ...) PRT_INST(kernel, tag),
#define PRT_INST_NAME_N(sig, kernel) #kernel,
#define PRT_INST_NAME_T(sig, kernel, tag, ...) #kernel "<" #__VA_ARGS__ ">",
enum PrtRaygenInst : uint32_t { PRT_RAYGEN_INSTANCES(PRT_INST_ENUM_T) PRT_RAYGEN_NONE };  // NONE: the path route generates its rays itself
enum PrtShadeInst : uint32_t { PRT_SHADE_INSTANCES(PRT_INST_ENUM_T) PRT_SHADE_NONE };
enum PrtAccumulateInst : uint32_t { PRT_ACCUMULATE_INSTANCES(PRT_INST_ENUM_N, PRT_INST_ENUM_T) PRT_ACCUMULATE_NONE };
// The names as the compiler demangles the kernels, every template argument spelled out (prt_shade_instance reports the shade
// one); static storage.  NONE is the empty string.
inline const char* prt_raygen_name(PrtRaygenInst i) {
    static const char* const names[] = {PRT_RAYGEN_INSTANCES(PRT_INST_NAME_T) ""};
    return names[i <= PRT_RAYGEN_NONE ? i : PRT_RAYGEN_NONE];
}
inline const char* prt_shade_name(PrtShadeInst i) {
    static const char* const names[] = {PRT_SHADE_INSTANCES(PRT_INST_NAME_T) ""};
    return names[i <= PRT_SHADE_NONE ? i : PRT_SHADE_NONE];
}
inline const char* prt_accumulate_name(PrtAccumulateInst i) {
    static const char* const names[] = {PRT_ACCUMULATE_INSTANCES(PRT_INST_NAME_N, PRT_INST_NAME_T) ""};
    return names[i <= PRT_ACCUMULATE_NONE ? i : PRT_ACCUMULATE_NONE];
}

// What run_batch knows before it launches anything.  One field per term that a route decision or an instance choice reads.
struct PrtRouteFacts {
    // features, each with kernel instances of its own
    bool lit;          // lighting != PRT_LIGHTING_OFF: a light sample per Lambertian vertex (k_shade_nee*)
    bool mesh_lights;  // light_sources has PRT_LIGHT_SOURCES_MESH: triangle lights in the light set (read only with lit)
    bool light_clusters;  // clustered light selection is set (read only with lit and mesh_lights: k_shade_nee_clus*)
    bool env;          // an environment image is set
    bool tex;          // a texture binding textures a material
    bool lens;         // lens.aperture > 0: a primary ray of its own per sample
    bool listed;       // the batch renders a tile list (prt_render_adaptive)
    bool film_stats;   // per-pixel film statistics are on
    // the scene
    bool has_nodes;    // dsc.n_nodes != 0: there are triangles to walk to
    bool has_bvh2;     // dsc.nodes != nullptr: the binary tree exists (host-built scenes)
    bool insts;        // dsc.n_insts != 0: placed mesh copies
    bool abvh;         // dsc.abvh_nodes != nullptr: a BVH over many analytic primitives
    bool few_prims;    // dsc.n_prims <= 16
    // sampling options
    bool jitter;       // sampling.jitter != 0
    bool sa;           // sampling.rr_depth != 0 || sampling.clamp > 0: roulette or clamp
    bool multi_sample; // S_cur > 1
    // tunables and diagnostics
    bool variant0;         // variant == 0: the persistent traversal kernels (1, 2: k_intersect, A/B)
    bool compact_primary;  // the compact_primary switch
    bool primary_walk;     // the primary_walk switch
    bool takes_primary;    // prt_traverse_takes_primary(walk facts)
    bool primary_hit;      // tune.primary_hit != 0
    bool path_gate;        // !trav_stats && !d_shade_div && sort_rays == 0 && n_paths <= tune.path_max && prt_path_kernel_applies(walk facts)
    uint32_t path_kernel;  // tune.path_kernel: 0 off, 1 batches of one sample, 2 any batch
    uint32_t fuse;         // tune.fuse
    // the last segment of a path as a visibility query (DESIGN.md section 3 "The last segment")
    bool mesh_emissive;     // a mesh or a placed copy has an emissive material (PrtHostScene::mesh_emissive)
    bool depth_ge2;         // max_depth >= 2: the last segment has a shade launch as its producer
    bool sort_rays;         // the sort_rays measurement aid is on
    uint32_t last_segment;  // the last_segment tunable: 0 off, 1 end decided last segments in their producer, 2 = 1 + the last walk is any-hit
};

struct PrtRoutePlan {
    bool path;         // the whole batch is one launch of the path instance of the 8-wide kernel (then only `accumulate` is launched)
    bool compact;      // compact primary rays (PrtPrimary): bounce 0 rebuilds its rays from the pixel records
    bool walk;         // bounce 0 walks one ray per front pixel
    bool primary_hit;  // k_primary_hit runs between bounce 0's walk and its shade
    bool walk8;        // a tree walk runs the persistent kernels (false: k_intersect, variants 1 and 2): prt_route_walk8
    uint32_t fuse;     // k_shade's fuse_max
    PrtRaygenInst raygen;
    PrtShadeInst shade0, shade;  // bounce 0, later bounces
    PrtAccumulateInst accumulate;
    uint32_t last_segment;  // 0: every stored ray is walked and shaded; 1: the producer of a path's last segment ends it when the
                            // analytic scan decides what the film gets, and the last shade launch does not rebuild a triangle hit;
                            // 2: and the last walk is the seeded any-hit walk (k_occluded8_seeded)
};

inline PrtRoutePlan prt_plan_route(const PrtRouteFacts& f) {
    PrtRoutePlan p{};
    // No special route: nothing that brings shade instances of its own, which all shade one segment per call from full ray
    // records.  (A lens changes the primary rays only: it rules out what rebuilds or generates them, not fusion.)
    const bool plain_shade = !f.lit && !f.env && !f.tex && !f.listed;
    const bool plain = plain_shade && !f.lens;
    // k_shade shades one analytic-only segment in place per call when the scene has a BVH and few analytic primitives
    p.fuse = (plain_shade && f.has_nodes && f.few_prims) ? f.fuse : 0u;
    p.path = plain && f.path_kernel != 0u && (f.path_kernel == 2u || !f.multi_sample) && f.path_gate && f.variant0 && p.fuse == 0u;
    // the default pipeline without jitter / roulette / clamp / fusion
    p.compact = !p.path && plain && f.compact_primary && f.variant0 && f.has_nodes && !f.abvh && !f.jitter && !f.sa && p.fuse == 0u &&
                f.takes_primary;
    // (a batch of ONE sample keeps its path slots, which are the front-pixel list, and has no hit to share)
    p.walk = p.compact && f.primary_walk && f.multi_sample;
    p.primary_hit = p.compact && f.primary_hit && f.multi_sample;
    p.walk8 = prt_route_walk8(f.variant0, f.insts, f.has_bvh2);

    const uint32_t j = f.jitter, ab = f.abvh, in = f.insts, en = f.env, ml = f.mesh_lights;
    if (p.path) p.raygen = PRT_RAYGEN_NONE;
    else if (f.listed) p.raygen = PrtRaygenInst(PRT_INST(k_raygen_list, ffff) + (j << 3 | ab << 2 | en << 1 | (uint32_t)f.lens));
    else if (f.lens) p.raygen = PrtRaygenInst((f.env ? PRT_INST(k_raygen_lens_env, ff) : PRT_INST(k_raygen_lens, ff)) + (j << 1 | ab));
    else if (f.env) p.raygen = PrtRaygenInst(PRT_INST(k_raygen_env, ff) + (j << 1 | ab));
    else if (f.abvh) p.raygen = f.jitter ? PRT_INST(k_raygen, tttf) : PRT_INST(k_raygen, fttf);  // the general instances with the BVH scan
    else if (f.jitter) p.raygen = f.sa ? PRT_INST(k_raygen, ttff) : PRT_INST(k_raygen, tfff);
    else if (p.compact) p.raygen = PRT_INST(k_raygen, ffft);
    else p.raygen = f.sa ? PRT_INST(k_raygen, ftff) : PRT_INST(k_raygen, ffff);

    const bool cl = f.mesh_lights && f.light_clusters;
    if (p.path) p.shade = PRT_SHADE_NONE;
    else if (f.lit && f.tex && cl) p.shade = PrtShadeInst(PRT_INST(k_shade_nee_clus_tex, fff) + (in << 2 | ab << 1 | en));
    else if (f.lit && cl) p.shade = PrtShadeInst((f.env ? PRT_INST(k_shade_nee_clus_env, ff) : PRT_INST(k_shade_nee_clus, ff)) + (in << 1 | ab));
    else if (f.lit && f.tex) p.shade = PrtShadeInst(PRT_INST(k_shade_nee_tex, ffff) + (in << 3 | ab << 2 | ml << 1 | en));
    else if (f.lit)
        p.shade = PrtShadeInst((f.mesh_lights ? (f.env ? PRT_INST(k_shade_nee_mesh_env, ff) : PRT_INST(k_shade_nee_mesh, ff))
                                              : (f.env ? PRT_INST(k_shade_nee_env, ff) : PRT_INST(k_shade_nee, ff))) + (in << 1 | ab));
    else if (f.tex) p.shade = PrtShadeInst(PRT_INST(k_shade_tex, fff) + (in << 2 | ab << 1 | en));
    else if (f.env) p.shade = PrtShadeInst(PRT_INST(k_shade_env, ff) + (in << 1 | ab));
    else if (f.abvh) p.shade = f.insts ? PRT_INST(k_shade, 0tttf) : PRT_INST(k_shade, 0tftf);  // general instances with the BVH scan
    else if (f.insts) p.shade = PRT_INST(k_shade, 0ttff);  // placed mesh copies: one general instance
    else if (p.fuse) p.shade = f.sa ? PRT_INST(k_shade, 1tfff) : PRT_INST(k_shade, 1ffff);
    else p.shade = f.sa ? PRT_INST(k_shade, 0tfff) : PRT_INST(k_shade, 0ffff);
    p.shade0 = p.compact ? PRT_INST(k_shade, 0ffft) : p.shade;  // bounce 0 of compact primary rays rebuilds them

    if (f.film_stats || f.listed) p.accumulate = PrtAccumulateInst(PRT_INST(k_accumulate_stat, ff) + ((uint32_t)f.lit << 1 | (uint32_t)f.listed));
    else p.accumulate = f.lit ? PRT_I_k_accumulate_lit : PRT_I_k_accumulate;  // (the path route is never lit)

    // Without fusion every ray of shade launch d has segment index d, so launch max_depth - 2 produces exactly the last segments
    // and launch max_depth - 1 consumes them; with no emissive triangle a last segment whose analytic hit does not emit
    // delivers throughput x 0 whatever the walk finds.  (The NEE family weights the last hit by MIS and stays as it is.)
    const bool last_ok = !p.path && p.fuse == 0u && !f.lit && !f.mesh_emissive && f.has_nodes && p.walk8 && !f.sort_rays && f.depth_ge2;
    p.last_segment = last_ok ? f.last_segment : 0u;
    return p;
}

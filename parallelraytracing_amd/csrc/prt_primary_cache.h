// prt_primary_cache.h — what a context's persistent primary buffers hold, as data: the key run_batch (prt_api.cpp) records when
// a batch has (re)built the primary stage, and the one function that says whether the next batch may use that stage as it
// stands.  Plain C++ with no HIP header (g++ compiles it alone: tests/primary_cache.cpp flips every field).  DESIGN.md
// section 2 "One walk per pixel" says what the buffers are.
//
// Without jitter and without a lens everything a batch computes before its first k_shade (k_raygen's path ids, front-pixel
// list, pixel records and bounce-0 counters; the bounce-0 walk's hits; k_primary_hit's records) is a function of the camera,
// the scene, the tile map, the batch size, max_depth and the route, not of the sample index or the seed: those reach the first
// k_shade as kernel arguments (PrtPrimary.first_sample / seed).  A stale record is a wrong image and a spurious rebuild is half
// a millisecond, so the key is coarse: generations that every setter bumps, and every fact of the batch spelled out.
#pragma once
#include <cstdint>

#include "prt_route.h"  // PrtRoutePlan; prt_walk.h: PrtWalkRow

struct PrtPrimaryKey {
    bool valid;                 // false: the buffers hold nothing (a cleared key)
    uint64_t camera_gen;        // bumped by prt_set_camera and prt_set_lens (the field of view is the camera's)
    uint64_t scene_gen;         // bumped by whatever can change geometry, materials, sky, environment, lights, textures or a tunable
    // the tile map (PrtTileMap)
    uint32_t W, H, rank, world, n_pix_local;
    // the batch
    uint32_t S_cur, max_depth;
    PrtRoutePlan plan;          // every field of it
    uint32_t walk_row;          // the bounce-0 walk's kernel instance (PrtWalkLaunch.row of its plan)
    bool walk_prim;             // and whether that launch rebuilds compact primary rays (PrtWalkLaunch.prim)
    // the route's switches as the batch's plan took them, and the facts that rule the stage out
    bool compact, walk, primary_hit, lens, jitter;
    uint32_t rr_depth;          // the sampling fields k_raygen is handed (PrtSampling)
    float clamp;
    bool listed;                // view.list != nullptr (a pass of prt_render_adaptive)
    bool instrumented;          // trav_stats or d_shade_div: a measurement batch
    bool exact;                 // the host reads the bounces' ray counts back (bounce 0's are then kept on the host as well)
};

inline bool prt_route_plan_equal(const PrtRoutePlan& a, const PrtRoutePlan& b) {
    return a.path == b.path && a.compact == b.compact && a.walk == b.walk && a.primary_hit == b.primary_hit && a.walk8 == b.walk8 &&
           a.fuse == b.fuse && a.raygen == b.raygen && a.shade0 == b.shade0 && a.shade == b.shade && a.accumulate == b.accumulate &&
           a.last_segment == b.last_segment;
}

// True if a batch described by `now` may skip k_raygen, the bounce-0 walk and k_primary_hit and start at its first k_shade on
// the buffers `held` describes.  Never for a batch that is jittered, uses a lens, renders a tile list or is instrumented,
// whatever `held` says; never from a cleared key.
inline bool prt_primary_reusable(const PrtPrimaryKey& held, const PrtPrimaryKey& now) {
    if (!held.valid || !now.valid) return false;
    if (now.jitter || now.lens || now.listed || now.instrumented || !now.compact) return false;
    return held.camera_gen == now.camera_gen && held.scene_gen == now.scene_gen && held.W == now.W && held.H == now.H &&
           held.rank == now.rank && held.world == now.world && held.n_pix_local == now.n_pix_local && held.S_cur == now.S_cur &&
           held.max_depth == now.max_depth && prt_route_plan_equal(held.plan, now.plan) && held.walk_row == now.walk_row &&
           held.walk_prim == now.walk_prim && held.compact == now.compact && held.walk == now.walk && held.primary_hit == now.primary_hit &&
           held.lens == now.lens && held.jitter == now.jitter && held.rr_depth == now.rr_depth && held.clamp == now.clamp &&
           held.listed == now.listed && held.instrumented == now.instrumented && held.exact == now.exact;
}

// What a context holds: the key above, and how the kept stage numbers its paths (prt_path_id.h).  The stage stores a path-id
// list per ray slot, so a batch may only start from ids of its own order and, pixel-major, of its own sample count: id_S is
// the divisor the ids were built for (0 with sample-major ids).  (The batch size is in the key above as S_cur and setting the
// path_id_order tunable bumps scene_gen, so these repeat what the key implies: spelled out all the same, a stale id is a
// sample added to the wrong pixel.)
struct PrtPrimaryStageKey {
    PrtPrimaryKey batch;
    uint32_t id_order;  // 0 sample-major, 1 pixel-major
    uint32_t id_S;
};

inline bool prt_primary_stage_reusable(const PrtPrimaryStageKey& held, const PrtPrimaryStageKey& now) {
    return prt_primary_reusable(held.batch, now.batch) && held.id_order == now.id_order && held.id_S == now.id_S;
}

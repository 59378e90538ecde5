// prt_walk.h — a tree walk as data: the facts walk_rays (prt_api.cpp) collects, the one list of the walk kernels' instances and
// the one function that turns the facts into the launches of a walk.  Plain C++ with no HIP header (g++ compiles it alone:
// tests/walk_table.cpp holds every combination of the facts to the table recorded from the hand-written launchers this
// replaced).  The launchers (prt_kernels.hip) expand the same lists into their `case`s and only follow the plan.
#pragma once
#include <cstdint>

// Tunables of the persistent walk kernels (prt_set_param).  A kernel argument.
struct PrtTravTuning {
    uint32_t grid_blocks;  // resident 256-thread blocks of the persistent grid
    uint32_t chunk;        // rays a wave grabs per global atomic (multiple of 64)
    uint32_t refill_min;   // idle lanes of a wave that trigger a refill
    uint32_t exit_max;     // leave the node loop when at most this many lanes still search for a leaf (0xFFFFFFFF = per instance: 32 two-level, 16 otherwise)
    uint32_t xcd_affinity; // 4-wide / binary kernels, A/B: 1 = each XCD drains its own eighth of the ray buffer first (L2 locality), then steals
    uint32_t wide;         // 2: walk the compressed 8-wide tree (default), 1: the 4-wide tree, 0: the binary tree
    uint32_t tri_min;      // 8-wide kernel: start a triangle phase once this many lane-steps have queued triangles (0 = per tree: 12 for one-level trees with one node per 128-B line, 24 otherwise)
    uint32_t fuse;         // k_shade: 1 = shade one analytic-only segment in place per call (default), 0 = store every ray
    uint32_t stack_cap;    // test hook: the 8-wide kernel treats its stack as this many entries (0 = all of them)
    uint32_t stack_lds;    // selects the kernel instance (stack entries in LDS / waves per SIMD), see prt_plan_walk below
    uint32_t exact_grids;  // host: size k_shade's grid from the bounce's ray count read back during the traversal (big batches)
    uint32_t steal;        // 8-wide kernel at 5 waves/SIMD: a draining wave with at least this many idle lanes lets them take pending subtrees of its remaining rays (0 = off)
    uint32_t tail;         // 8-wide kernel: the last `tail` 64-ray granules per resident wave are handed out one at a time
    uint32_t probe_slot;   // instrumented instance only: this launch's timeline goes to stats[16 + 8 * probe_slot ..] (see PRT_TIMELINE)
    const uint32_t* perm;  // measurement aid (sort_rays): the 8-wide kernel takes ray perm[i] where it would take ray i (nullptr = identity)
    uint32_t path_kernel;  // host: 0 = off (default); 1 = a batch of ONE sample with at most path_max paths runs as one launch of the path instance of the 8-wide kernel (below); 2 = any batch of at most path_max paths
    uint32_t path_max;
    uint32_t big;          // 8-wide kernel: launches with >= big_min granules per resident wave hand out the front of their bulk `big` chunks per grab (1 = off)
    uint32_t static_small; // 8-wide kernel: launches of single granules only (< 8 per resident wave) deal them to the waves round-robin instead of through the cursor
    uint32_t big_min;      // (granules per resident wave)
    uint32_t big_keep;     // granules per resident wave at the end of the bulk that stay ordinary chunks
    uint32_t primary_hit;  // host: with compact primary rays, rebuild the primary hit's surface interaction once per pixel (k_primary_hit); 0 = per sample in k_shade (A/B)
};

// One row per family member with its template arguments.  The request crosses a row with STATS, PRIM (LEAN row only), PATH (deep15
// row only) and the any-hit kernels k_occluded8_persistent / _seeded (8-wide rows): 47 instances.  8-wide: T(public name, STACK_L, WAVES, INST, LEAN)
//   inst12_4waves  placed mesh copies: two-level walk, 12 stack entries + the lanes' world rays in LDS, 4 waves per SIMD
//   wide11_5waves  A/B (stack_lds = 5): 11 entries, 5 waves per SIMD, ray and best hit in registers
//   lean8_5waves   default: 8 entries, 5 waves per SIMD (ray and best hit in LDS); trees of <= 9 levels, and deeper
//                  HOST-built trees, whose rare deeper rays go through the overflow list to the 4-wide tree (C5)
//   deep15_4waves  deeper trees without a 4-wide fallback (device-built): 15 entries, 4 waves per SIMD
#define PRT_WALK8_ROWS(T) \
    T(inst12_4waves, 12, 4, true, false) T(wide11_5waves, 11, 5, false, false) T(lean8_5waves, 8, 5, false, true) T(deep15_4waves, 15, 4, false, false)
// 4-wide and binary: T(tag, STACK_L, WAVES, MODE).  MODE 0: LDS-only stack that the tree's bound fits; 1: LDS + global spill
// rows; 2, 3 (4-wide): LDS-only with an overflow check (3: branch-free node step), the overflow list re-walked in MODE 1
#define PRT_WALK4_ROWS(T) \
    T(22_6_0, 22, 6, 0) T(27_5_0, 27, 5, 0) T(35_4_0, 35, 4, 0) T(27_5_2, 27, 5, 2) T(24_5_3, 24, 5, 3) T(27_5_1, 27, 5, 1) T(32_4_3, 32, 4, 3)
#define PRT_WALK2_ROWS(T) T(24_6_0, 24, 6, 0) T(31_5_0, 31, 5, 0) T(31_5_1, 31, 5, 1)
// k_intersect, one thread per ray (variants 1 while-while and 2 one-loop, A/B): T(tag, STACK, VARIANT)
#define PRT_INTERSECT_ROWS(T) T(31_0, 31, 0) T(31_1, 31, 1) T(63_0, 63, 0) T(63_1, 63, 1)

#define PRT_WALK8_ENUM(name, ...) PRT_W8_##name,
#define PRT_WALK4_ENUM(tag, ...) PRT_W4_##tag,
#define PRT_WALK2_ENUM(tag, ...) PRT_W2_##tag,
#define PRT_INTERSECT_ENUM(tag, ...) PRT_WI_##tag,
enum PrtWalkRow : uint32_t {
    PRT_WALK8_ROWS(PRT_WALK8_ENUM) PRT_WALK4_ROWS(PRT_WALK4_ENUM) PRT_WALK2_ROWS(PRT_WALK2_ENUM) PRT_INTERSECT_ROWS(PRT_INTERSECT_ENUM) PRT_WALK_ROWS
};
// A row's family (8: 8-wide, 4, 2, 0: k_intersect), its public name (prt_kernel_instance) and its template arguments
struct PrtWalkRowInfo {
    uint32_t family;
    const char* name;
    int arg[4];
};
inline const PrtWalkRowInfo& prt_walk_row(PrtWalkRow r) {
#define PRT_WALK8_INFO(name, L, W, IN, LN) {8u, #name, {L, W, IN, LN}},
#define PRT_WALK4_INFO(tag, L, W, MODE) {4u, "bvh4", {L, W, MODE, 0}},
#define PRT_WALK2_INFO(tag, L, W, MODE) {2u, "bvh2", {L, W, MODE, 0}},
#define PRT_INTERSECT_INFO(tag, S, V) {0u, "", {S, V, 0, 0}},
    static const PrtWalkRowInfo rows[] = {PRT_WALK8_ROWS(PRT_WALK8_INFO) PRT_WALK4_ROWS(PRT_WALK4_INFO) PRT_WALK2_ROWS(PRT_WALK2_INFO)
                                              PRT_INTERSECT_ROWS(PRT_INTERSECT_INFO){0u, "", {0, 0, 0, 0}}};
    return rows[r <= PRT_WALK_ROWS ? r : PRT_WALK_ROWS];
}

// CLOSEST: the closest hit.  ANY: prt_occluded and the shadow rays (hit[] = HIT_MISS marks the rays to walk).  SEEDED: the last
// segment's any-hit walk over a closest-hit walk's buffer.  PATH: whole paths in one launch (PrtPathArgs), max_rays = the paths.
enum PrtWalkRequest : uint32_t { PRT_WALK_CLOSEST, PRT_WALK_ANY, PRT_WALK_SEEDED, PRT_WALK_PATH };

// What a walk's choice reads, and nothing else.
struct PrtWalkFacts {
    bool has8, has4, has2;  // dsc.nodes8 / nodes4 / nodes: the trees that exist (device-built and refitted scenes: the 8-wide one only)
    bool insts, abvh;       // dsc.n_insts != 0: placed mesh copies; dsc.abvh_nodes: a primitive BVH (prt_path_kernel_applies only)
    uint32_t depth8, node_stride, depth2, max_stack4;  // dsc.depth8, dsc.node_stride; the binary tree's max_depth; the 4-wide bound
    int variant;            // 0: the persistent kernels; forced 1, 2: k_intersect
    uint32_t wide, stack_lds, stack_cap, exit_max, tri_min, grid_blocks, steal;  // PrtTravTuning
    uint32_t max_rays;
    PrtWalkRequest request;
    bool stats, primary;    // instrumented; compact primary rays are offered (PrtPrimary)
};

struct PrtWalkLaunch {
    PrtWalkRow row;
    PrtWalkRequest form;  // the row's kernel: CLOSEST (with stats / prim), ANY, SEEDED or PATH
    bool stats, prim;
    uint32_t grid, exit_max, tri_min, stack_cap, steal;  // the tunables as resolved; the launch's other tunables are the caller's
    bool keep_perm;   // false: the launch gets perm = nullptr
    bool overflow;    // reads the overflow list (count and ray slots) instead of the caller's count
    bool reset;       // k_reset_cursors precedes it
};
struct PrtWalkPlan {
    uint32_t n;               // launches, in order: the walk, and where one exists the re-walk of its overflow list
    PrtWalkLaunch launch[2];
    const char* name;         // prt_kernel_instance: the persistent kernels' row, also where k_intersect is forced
    uint32_t stack_entries;   // of that row
    // What prt_kernel_occupancy describes: the 8-wide row, plain closest hit, and for EVERY scene without the 8-wide walk
    // k_traverse4_persistent<32, 4, 3, false>, whatever is launched (the answer it always gave; not this header's to change).
    PrtWalkRow occupancy;
    uint32_t resident_grid;   // grid_blocks, as the 5-wave instance sizes it where that is the row
};

// Persistent kernels, or with variant 1 or 2 forced k_intersect: placed copies and device-built trees (no binary tree) have the 8-wide kernel only.
inline bool prt_route_walk8(bool variant0, bool insts, bool has_bvh2) { return variant0 || insts || !has_bvh2; }
inline bool prt_route_walk8(const PrtWalkFacts& f) { return prt_route_walk8(f.variant == 0, f.insts, f.has2); }
// True if the walk runs the instance that can rebuild compact primary rays: the LEAN row, and a tree shallow enough that no ray
// can reach the overflow list (its re-walk reads full ray records).  (The RAW stack_cap: on a scene without a 4-wide tree, where
// the plan ignores the hook, a set hook still sends bounce 0 down the general route.  Same rays, same hits.)
inline bool prt_traverse_takes_primary(const PrtWalkFacts& f) {
    return f.has8 && !f.insts && (f.wide == 2u || !f.has4) && (f.stack_lds == 0u || f.stack_lds == 6u) && f.stack_cap == 0u && f.depth8 <= 9u;
}
// The PATH instance: one-level scenes with the 8-wide tree, a tree its 15-entry stack holds, and no primitive BVH
// (classify_ray's walk keeps a per-thread LDS stack of its own).  (The RAW stack_cap here too: a set hook selects the pipeline.)
inline bool prt_path_kernel_applies(const PrtWalkFacts& f) {
    return f.has8 && !f.insts && !f.abvh && f.depth8 <= 16u && f.wide == 2u && f.stack_cap == 0u;
}

inline PrtWalkPlan prt_plan_walk(const PrtWalkFacts& f) {
    PrtWalkPlan p{};
    // The persistent row, and whether the spill-capable 4-wide row re-walks an overflow list (`again`).  Without a 4-wide tree
    // (device-built and refitted scenes) nothing does, so a forced row whose stack the tree's depth exceeds (stack_lds 5 beyond 12
    // levels, 6 beyond 9) is not taken, and the stack_cap test hook is ignored.  Such scenes have at most 16 levels (the device
    // builders stop at 15, prt_refit_meshes refuses deeper trees), which deep15_4waves holds.
    const bool tree8 = f.has8 && (f.wide == 2u || f.insts || !f.has4);
    const uint32_t sl = f.stack_lds, pushes = f.depth2 ? f.depth2 - 1u : 0u;
    PrtWalkRow row;
    bool again = false;
    if (tree8) {
        if (f.insts) row = PRT_W8_inst12_4waves;
        else if (sl == 5u && (f.has4 || f.depth8 <= 12u)) row = PRT_W8_wide11_5waves;
        else row = ((sl == 0u || sl == 6u) && (f.has4 || f.depth8 <= 9u)) ? PRT_W8_lean8_5waves : PRT_W8_deep15_4waves;
    } else if (f.wide) {  // max_stack4: the host's worst-case bound of the entries a ray of the 4-wide tree holds
        if (f.max_stack4 <= 22u && sl == 24u) row = PRT_W4_22_6_0;
        else if (f.max_stack4 <= 27u) row = PRT_W4_27_5_0;
        else if (sl == 39u && f.max_stack4 <= 35u) row = PRT_W4_35_4_0;
        // default: 32 entries at 4 waves/SIMD so that the 116 VGPRs need no scratch (the 5-wave rows spill 50-70 B/lane and are
        // 9 % slower); A/B 1: 28 entries in LDS + global spill; 2, 3: measured equal on C3
        else row = sl == 1u ? PRT_W4_27_5_1 : sl == 2u ? PRT_W4_27_5_2 : sl == 3u ? PRT_W4_24_5_3 : PRT_W4_32_4_3;
        again = prt_walk_row(row).arg[2] >= 2;  // MODE 2, 3: the overflow list is re-walked
    } else {
        row = (pushes <= 24u && sl == 24u) ? PRT_W2_24_6_0 : pushes <= 31u ? PRT_W2_31_5_0 : PRT_W2_31_5_1;
    }
    const bool two_level = row == PRT_W8_inst12_4waves, five = row == PRT_W8_lean8_5waves, path = f.request == PRT_WALK_PATH;
    p.name = prt_walk_row(row).name;
    p.stack_entries = (uint32_t)prt_walk_row(row).arg[0];
    p.occupancy = tree8 ? row : PRT_W4_32_4_3;
    p.resident_grid = five ? f.grid_blocks + f.grid_blocks / 4u : f.grid_blocks;

    PrtWalkLaunch& l = p.launch[p.n++];
    const uint32_t need = (uint32_t)(((uint64_t)f.max_rays + 255u) / 256u);
    if (!path && !prt_route_walk8(f)) {  // no tunables, one block per 256 rays
        l.row = f.depth2 <= 31u ? (f.variant == 2 ? PRT_WI_31_1 : PRT_WI_31_0) : (f.variant == 2 ? PRT_WI_63_1 : PRT_WI_63_0);
        l.stats = f.stats;
        l.grid = need;
        return p;
    }
    uint32_t g = f.grid_blocks < need ? f.grid_blocks : need;
    if (g == 0u) g = 1u;
    // the any-hit kernels exist for the 8-wide rows; elsewhere the closest hit from the seeded bound answers the query as well
    const bool any = tree8 && (f.request == PRT_WALK_ANY || f.request == PRT_WALK_SEEDED);
    l.row = path ? PRT_W8_deep15_4waves : row;
    l.form = (any || path) ? f.request : PRT_WALK_CLOSEST;
    l.stats = f.request == PRT_WALK_CLOSEST && f.stats;
    l.prim = five && f.primary && f.request == PRT_WALK_CLOSEST;  // bounce 0 of compact primary rays
    l.grid = (five && !path && g == f.grid_blocks) ? g + g / 4u : g;  // 5 instead of 4 resident blocks per CU
    // exit_max "auto" (0xFFFFFFFF, the context's default): the two-level row leaves its node loop at <= 32 walkers (its lanes wait
    // for level switches that the wave does together; C5I +4.4 % against 16), every other row at <= 16.  tri_min "auto" (0): a
    // triangle phase starts after 24 queueing lane-steps, but after 12 on one-level trees far beyond the caches (one node per 128-B
    // line: C5 +1.7 %; elsewhere 12 / 16 lose 0.5-2 %, TUNING.md).  The PATH request keeps 16 and 24 whatever the node stride.
    l.exit_max = f.exit_max != 0xFFFFFFFFu ? f.exit_max : (two_level && !path) ? 32u : 16u;
    l.tri_min = f.tri_min != 0u ? f.tri_min : (path || two_level || f.node_stride != 8u) ? 24u : 12u;
    l.stack_cap = (!path && !f.has4 && !f.insts) ? 0u : f.stack_cap;
    l.steal = f.steal;
    l.keep_perm = !any;
    if (path) return p;
    // (the two-level row has no overflow list: a stack overflow is an error, the host checks the depths)
    const bool overflow = tree8 && !two_level && (l.stack_cap != 0u || f.depth8 > p.stack_entries + 1u);
    if (tree8) again = overflow && f.has4;
    // (not launched when the tree is too shallow for any ray to overflow: two tiny launches and their gaps are ~12 us per bounce)
    if (again) {
        PrtWalkLaunch& r = p.launch[p.n++] = l;
        r.row = PRT_W4_27_5_1, r.form = PRT_WALK_CLOSEST, r.prim = false, r.grid = 8u, r.overflow = r.reset = true;
    }
    if (five && overflow) l.steal = 0u;  // (a helper cannot hand a ray to the overflow list)
    return p;
}

// prt_scene.h — the scene compiler: PrtSceneDesc (include/prt.h) -> PrtHostScene, everything the kernels need about a
// scene as host arrays (flattened primitives, light table, trees, triangle records in leaf order, instance table).
// HIP-free: prt_scene.cpp builds with a plain C++ compiler (tests/sanitize_host.cpp runs it under ASan / UBSan); the
// C-ABI layer (prt_api.cpp) owns the device copies and supplies the device-side tree builder as a callable.
#pragma once
#include <stdint.h>

#include <array>
#include <functional>
#include <string>
#include <vector>

#include "../../include/prt.h"
#include "bvh.h"
#include "prt_scene_pod.h"

// The scalar half of DevScene (prt_kernels.h; same names, same meaning); upload_scene puts the device pointers next to it.
struct PrtSceneScalars {
    uint32_t n_insts;
    uint32_t n_prims;
    uint32_t n_nodes;
    uint32_t n_tris;
    float pad;
    float abvh_q[3];
    float extent;
    float root_min[3], root_max[3];
    float sky[3];
};

// One emissive world-space mesh or placed copy in the candidate table: its triangles' global primitive indices are
// [prim_first, prim_first + n_tris) and candidate light_first + k is its face k (DevLightRun, prt_kernels.h, is this struct).
struct PrtLightRun {
    uint32_t prim_first, n_tris, light_first, world;  // world: 1 = a world-space mesh (prt_rebuild_mesh_lights rewrites it)
};

// The light set under PRT_LIGHT_SOURCES_ANALYTIC | PRT_LIGHT_SOURCES_MESH (include/prt.h "Triangle lights"), built with
// every scene whatever the context's mask.  CANDIDATES, in global primitive order: the analytic lights of
// PrtHostScene::lights, then every triangle of an Emissive world-space mesh, then every triangle of an Emissive placed
// copy.  A candidate without power keeps its slot with an empty interval, so that a mesh is one contiguous run and the
// primitive -> light lookup is one base per run.  The light set proper (`visible`) is the candidates whose interval
// [T_{i-1}, T_i) is not empty.
struct PrtMeshLights {
    std::vector<float> records;      // 4 * PRT_LIGHT_F4 floats per candidate (prt_kernels.h DevLights; triangles: kind 2)
    std::vector<double> power;       // per candidate; 0: not a light
    std::vector<uint32_t> thr;       // thr[i] = T_{i+1} for i + 1 < n_search: the search is "smallest i with r0 < thr[i], else n_search - 1"
    uint32_t n_search = 0;           // 1 + the last candidate with a non-empty interval (every T before it is < 2^32)
    std::vector<uint32_t> bucket;    // bucket[b] = the candidate picked by r0 = b << bucket_shift; 2^(32 - bucket_shift) + 1 entries
    uint32_t bucket_shift = 32;
    std::vector<PrtLightRun> runs;   // ascending prim_first
    std::vector<uint32_t> visible;   // light of the set -> candidate
    std::vector<uint32_t> cand_visible;  // candidate -> light of the set, 0xFFFFFFFF for an empty interval
    std::vector<uint64_t> width;     // per light of the set: T_i - T_{i-1}; pmf = width / 2^32
    std::vector<float> box;          // per candidate: its world box lo.xyz, hi.xyz ("Clustered light selection": a light's world box)
    uint32_t n_emitters_unsampled = 0;
};

// Clustered light selection (include/prt.h "Clustered light selection"): a flat list of at most max_clusters spatial
// clusters over the light set of PrtMeshLights, built with it (finish of every candidate table: prt_compile_scene,
// prt_rebuild_mesh_lights) and by prt_build_light_clusters when max_clusters changes.  Members are cluster-major, in
// candidate order inside a cluster.
struct PrtLightClusters {
    uint32_t max_clusters = 32;          // what the table was built for (1..PRT_LIGHT_MAX_CLUSTERS)
    std::vector<float> boxes;            // 8 floats per cluster: lo.xyz | phi, hi.xyz | r2
    std::vector<uint32_t> range;         // 4 per cluster: first member, last member with a non-empty inner interval, members, 0
    std::vector<uint64_t> power_width;   // per cluster: W_c, the sum of its members' global widths (they sum to 2^32)
    std::vector<uint32_t> members;       // cluster-major: candidate
    std::vector<uint32_t> thr;           // cluster-major: low 32 bits of U_{c,j} of member j (the last non-empty member's 2^32 is implicit)
    std::vector<uint64_t> inner_width;   // cluster-major: U_{c,j} - U_{c,j-1}
    std::vector<uint32_t> cand_cluster;  // per candidate: its cluster, 0xFFFFFFFF outside the light set
    std::vector<uint32_t> cand_member;   // per candidate: its slot in members / inner_width
    uint32_t n_empty_inner = 0;          // members whose inner interval is empty (never picked under clustered selection)
    uint32_t n_clusters() const { return (uint32_t)power_width.size(); }
};

// The environment light (include/prt.h "Environment light"): the image and its sampling tables, a property of the
// context, not of a scene.  Built on the host in double.
struct PrtEnvTables {
    uint32_t W = 0, H = 0;           // 0 x 0: no environment
    float light_share = 0.0f;
    std::vector<float> texels;       // 4 floats per texel: rgb, fl(p_ij W H / (2 pi^2)) = pdf_w x sin(theta)
    std::vector<uint64_t> row_width; // R_i - R_{i-1}; empty: no distribution
    std::vector<uint64_t> col_width; // C_ij - C_{i,j-1}, H x W
    std::vector<uint32_t> row_thr;   // row_thr[i] = R_{i+1} for i < row_last: the row is "smallest i with r < row_thr[i], else row_last"
    std::vector<uint32_t> col_thr;   // H x W, col_thr[i W + j] = C_{i,j+1} for j < col_last[i]
    std::vector<uint32_t> col_last;  // per row: the last column with a non-empty interval
    uint32_t row_last = 0;           // the last row with a non-empty interval
    uint32_t n_sampled = 0;          // texels with a non-empty interval
};
// Checks `env` (PRT_ERR_INVALID, message in *err, *out untouched) and builds its tables.
int prt_build_environment(const PrtEnvironment* env, PrtEnvTables* out, std::string* err);
// T_e for an environment and a light set of n_lights lights (0 without an environment).
uint64_t prt_environment_threshold(const PrtEnvTables& env, uint32_t n_lights);
// fl32(pmf (2^32 - T_e) / 2^32) for a pmf given in double
float prt_scaled_pmf(double pmf, uint64_t t_env);

// One instanced mesh of a compiled scene: what moving its copies needs to know about it (prt_update_instances)
struct PrtPlacedMesh {
    float mn[3], mx[3];  // its box in its own space
    uint32_t slot_base;  // first triangle slot of its records
    uint32_t node_base;  // its tree's root in nodes8_all
    uint32_t depth8;     // levels of its tree
    uint32_t n_tris;
};

struct PrtHostScene {
    std::vector<PrtMaterial> materials;
    std::vector<DevPrim> prims;
    BvhBuild bvh;                      // the world-space meshes' tree
    std::vector<float> tri_records;    // 12 floats per triangle, leaf order
    std::vector<float> nrm_records;    // 12 floats per triangle, leaf order
    double gpu_build_ms = 0.0;
    bool scene_device_built = false;   // the scene's 8-wide tree came from the device-side builder (no binary / 4-wide tree)
    std::vector<uint32_t> mesh_sizes;  // per world-space mesh of the scene: n_vertices, n_triangles (prt_refit_meshes checks them)
    std::vector<uint32_t> nodes8_all;  // scenes with placed mesh copies: top-level tree + every mesh's tree
    std::vector<DevInstance> dev_insts;
    std::vector<uint32_t> tlas_inst;   // top-level leaf slot -> instance
    std::vector<PrtPlacedMesh> placed_meshes;  // per instanced mesh (scenes with placed copies)
    std::vector<uint32_t> inst_mesh;   // per placed copy: its instanced mesh
    std::array<float, 6> world_box{};  // the world box of that identity instance
    uint32_t n_world_insts = 0;        // 1: dev_insts[0] is the identity instance of the world-space meshes
    uint32_t top_nodes = 0;            // nodes of the top-level tree: nodes8_all[0 .. 20 * top_nodes)
    uint32_t top_depth = 0;            // its levels
    uint32_t max_mesh_depth = 0;       // levels of the deepest tree below it
    float extent_base = 0.0f;          // sc.extent before the copies' world boxes went into it
    uint32_t builder = 0;              // prt_set_param("gpu_build") the scene was built with (set by the C-ABI layer)
    BvhBuild abvh;                     // BVH over the analytic primitives' world boxes (scenes with many of them)
    PrtBvhInfo bvh_info{};
    PrtSceneScalars sc{};
    std::vector<float> lights;         // the light table: 4 * PRT_LIGHT_F4 floats per light (prt_kernels.h DevLights)
    std::vector<uint32_t> prim_light;  // per analytic primitive: its light index, 0xFFFFFFFF if not in the light set
    uint32_t n_emitters_unsampled = 0;
    std::vector<double> light_power;   // per light of `lights`: emitting area x mean(rgb)
    uint32_t ml_tris_counted = 0;      // the part of n_emitters_unsampled that is mesh / placed triangles
    bool mesh_emissive = false;        // a mesh or a placed copy has an emissive material (prt_route.h: the last-segment route needs none)
    PrtMeshLights ml;                  // the light set with emissive triangles in it (PRT_LIGHT_SOURCES_MESH)
    PrtLightClusters lc;               // its spatial clusters (PRT_LIGHT_SELECTION_CLUSTERED)
    // what a texture binding needs of the description beyond the above (prt_build_textures): the index buffers in face order
    std::vector<uint32_t> mesh_indices;    // the world-space meshes', mesh and face order: 3 per triangle
    std::vector<uint32_t> mesh_material;   // per world-space mesh
    std::vector<std::vector<uint32_t>> placed_indices;  // per instanced mesh (scenes with placed copies)
    std::vector<uint32_t> placed_vertices; // per instanced mesh: n_vertices
    uint32_t n_instanced_meshes = 0;       // of the description (they are compiled only when it has placed copies)
};

// The texture binding of a scene (include/prt.h "Image textures"): one pool of texels, a descriptor per texture, the
// texture of every material and the UV table.  The UV table is per mesh triangle in FACE order (6 floats: u0 v0 u1 v1 u2
// v2), the world-space meshes' triangles first (entry = global primitive index - n_prims), then every instanced mesh's
// once, shared by its placed copies; inst_uv_base[i] + (the index a triangle record of instance i carries) is the entry
// (unsigned arithmetic: the identity instance of the world-space meshes gets -n_prims).  No tree, builder, refit or
// instance update touches it.  A mesh without UVs has zeros.
struct PrtTexTables {
    bool is_set = false;
    uint32_t n_textures = 0;
    uint32_t n_textured_materials = 0;
    std::vector<float> texels;           // 4 floats per texel: rgb, 0
    std::vector<uint32_t> desc;          // 4 per texture: first texel, W, H, filter | wrap << 1
    std::vector<uint32_t> mat_tex;       // per material: texture or PRT_TEXTURE_NONE
    std::vector<float> uvs;              // 6 floats per triangle
    std::vector<uint32_t> inst_uv_base;  // per instance of PrtHostScene::dev_insts
    std::vector<uint8_t> mesh_has_uv;    // per world-space mesh, then per instanced mesh: 1 = the set gave it UVs
};
// Checks `set` against the compiled scene (PRT_ERR_INVALID, message in *err, *out untouched) and builds the tables.
int prt_build_textures(const PrtHostScene& hs, const PrtTextureSet* set, PrtTexTables* out, std::string* err);

// The light tables as the kernels get them under an environment with threshold t_env: copies of hs.lights / hs.ml.records
// whose pmf entries are prt_scaled_pmf of the exact pmf (t_env = 0: the tables themselves).  Either output may be null.
void prt_scaled_light_tables(const PrtHostScene& hs, uint64_t t_env, std::vector<float>* lights, std::vector<float>* ml_records);

// The clusters of hs->ml for at most max_clusters clusters (0: the default 32) into hs->lc.
void prt_build_light_clusters(PrtHostScene* hs, uint32_t max_clusters);
// Per candidate fl32(pmf_in (2^32 - T_e) / 2^32), what the kernels multiply P_c with (0 outside the light set / empty inner interval)
void prt_cluster_pmf_in(const PrtHostScene& hs, uint64_t t_env, std::vector<float>* out);

// The device-side builder of the 8-wide tree over n triangles given as 9 floats each (+ normals, + a material per
// triangle; both may be null): nodes8 / depth and the triangle / normal records in the tree's slot order come back
// (nrm_rec may be null); its device time is added to *ms.  keep: the device arrays stay with the supplier (the world
// meshes' tree of a scene without placed copies).  Returns PRT_OK, kPrtDeviceBuildGaveUp (the builder could not cope
// with this input; the host builder can) or a PRT_ERR_* code with *err set.
constexpr int kPrtDeviceBuildGaveUp = -1000;  // internal: not a PRT_ERR_* code
using PrtDeviceBuilder = std::function<int(const float* verts, const float* norms, const uint32_t* tri_mat, uint32_t n, uint32_t n_prims,
                                           float leaf_cost, bool keep, std::vector<uint32_t>& nodes8, uint32_t& depth, float* tri_rec,
                                           float* nrm_rec, double* ms, std::string* err)>;

struct PrtSceneOptions {
    float pad_coeff;                // culling pad = pad_coeff x the coordinates' magnitude
    bool prim_bvh;                  // build a BVH over the analytic primitives when there are many
    PrtDeviceBuilder device_build;  // null: every tree is built on the host
    uint32_t light_clusters = 0;    // PrtLightSelection.max_clusters of the context (0: the default 32)
};

// The description's top-level arrays: none null with a non-zero count (PRT_ERR_INVALID, message in *err).  First step of
// prt_compile_scene; prt_set_scene asks on its own beforehand, because a description this malformed leaves the context's
// present scene alone.
int prt_check_scene_arrays(const PrtSceneDesc* s, std::string* err);

// Compiles `s` into *out, of which nothing survives but the storage of its record arrays.  On failure (PRT_ERR_*, message
// in *err) *out is unspecified.
int prt_compile_scene(const PrtSceneDesc* s, const PrtSceneOptions& opt, PrtHostScene* out, std::string* err);

// prt_refit_meshes: the world-space meshes' triangles moved (verts: 9 floats per triangle, mesh and face order, all
// of them; null: they stayed).  prt_set_instance_transforms: the placed copies moved (placed: the scene's n_instances
// copies with their new transforms; null: they stayed).  Rewrites the records and powers of the runs that moved and every
// threshold; the result equals what prt_compile_scene builds for the new geometry.  O(candidates) on the host.
void prt_rebuild_mesh_lights(PrtHostScene* hs, const float* verts, const PrtInstance* placed = nullptr);

// ---- refit from device arrays (prt_refit_meshes_device) ----
// What the device form of the refit keeps per scene, built once from the compiled scene's index buffers and tree.
struct PrtRefitTables {
    std::vector<uint32_t> tri_first;    // per world-space mesh, + 1: its first triangle in mesh and face order
    std::vector<uint32_t> vert_first;   // per world-space mesh, + 1: its first vertex among all world-space vertices
    std::vector<uint32_t> corner;       // 3 per triangle, mesh and face order: the corner's vertex, vert_first of its mesh added
    std::vector<uint32_t> csr_start;    // per vertex, + 1: its run in csr_corner
    std::vector<uint32_t> csr_corner;   // per vertex its incident corners (3 * triangle + corner), ascending: compute_normals' order
    std::vector<uint32_t> level_nodes;  // prt_tree_levels of the world-space meshes' tree
    std::vector<uint32_t> level_start;
    std::vector<uint32_t> light_tris;   // the triangles (mesh and face order) of the emissive world-space runs of hs.ml, run by run
};
// The nodes of every level of the 8-wide tree whose n_nodes nodes lead the array n8, root first (breadth-first search from
// node 0: the builders emit their nodes in different orders, none of which a refit relies on).  0, or 1 + the node at
// which the tree turned out malformed; a tree that does not reach all of its nodes leaves level_nodes short.
uint32_t prt_tree_levels(const std::vector<uint32_t>& n8, uint32_t n_nodes, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_start);
// The tables of a scene without placed copies that has the 8-wide tree (PRT_ERR_INVALID, message in *err: the index
// buffers do not match mesh_sizes, or the tree is malformed).
int prt_build_refit_tables(const PrtHostScene& hs, PrtRefitTables* out, std::string* err);
// prt_rebuild_mesh_lights for world-space meshes that moved, from the vertices of the emissive triangles alone:
// packed = 9 floats per entry of PrtRefitTables::light_tris, in its order.  The result is that of the full form.
void prt_rebuild_mesh_lights_packed(PrtHostScene* hs, const float* packed);
// compute_normals' rule (prt_host.cpp: area-weighted vertex normals, double sums in ascending face order) through the
// incident-corner table of one mesh: corner / csr_* are PrtRefitTables' with vert_first = 0.  The host statement of what
// the device kernel computes.
void prt_normals_from_corners(const float* positions, uint32_t n_vertices, const uint32_t* corner, const uint32_t* csr_start,
                              const uint32_t* csr_corner, float* normals);

// ---- moving placed copies (prt_set_instance_transforms) ----
// What an update works out before anything of the scene is written.
struct PrtInstanceUpdate {
    std::vector<DevInstance> insts;               // the whole instance table with the new mat / inv / inv_scale (root: as in the scene)
    std::vector<std::array<float, 6>> boxes;      // every instance's world box (build_instance_table's rule)
    std::vector<uint32_t> top_nodes8, top_order;  // prt_build_top_level: the new top-level tree (child_base from 0) and slot -> instance
    uint32_t top_depth = 0;
};

// The checks of prt_set_instance_transforms: the scene has placed copies, n is their number, mesh and material of every
// copy are what prt_set_scene got, every transform passes prt_set_scene's test (PRT_ERR_INVALID, message in *err).
int prt_check_instance_update(const PrtHostScene& hs, const PrtInstance* instances, uint32_t n, std::string* err);
// insts / boxes of `up` for checked transforms.
void prt_instance_tables(const PrtHostScene& hs, const PrtInstance* instances, PrtInstanceUpdate* up);
// A new top-level tree over up->boxes with the builder prt_compile_scene used, into `up`; PRT_ERR_INVALID if it would be
// too deep for the traversal stack.  *gpu_ms grows by the device builder's time.  The scene is not written.
int prt_build_top_level(const PrtSceneOptions& opt, const PrtHostScene& hs, PrtInstanceUpdate* up, double* gpu_ms, std::string* err);
// The tree of prt_build_top_level goes in front of the mesh trees of hs->nodes8_all (their child_base and the instances'
// root rebased if the node count changed), tlas_inst, depths and bvh_info follow.  Before prt_commit_instances.
void prt_commit_top_level(PrtHostScene* hs, const PrtInstanceUpdate& up);
// dev_insts (root stays), the scene-wide bounds and the placed copies' triangle lights follow the new transforms.
void prt_commit_instances(PrtHostScene* hs, const PrtInstanceUpdate& up, const PrtInstance* instances);

// One PrtMesh as 9 floats per triangle into verts / norms (n_triangles x 9 each), with the checks every consumer of
// caller-supplied index buffers needs: indices in range, vertices finite ("<what> <m>: ..." in *err, PRT_ERR_INVALID).
// *extent grows to the largest |coordinate|; mn / mx (may be null) grow to the box.
int prt_flatten_mesh(const PrtMesh& me, const char* what, uint32_t m, float* verts, float* norms, float* extent, float* mn, float* mx,
                     std::string* err);

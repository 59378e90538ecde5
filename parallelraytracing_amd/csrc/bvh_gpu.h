// bvh_gpu.h — device-side builder of the compressed 8-wide tree (see bvh_gpu.hip, bvh.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

struct PrtGpuBvh {
    uint32_t* d_nodes8;  // n_nodes x 20 dwords (ownership passes to the caller, hipFree)
    float4* d_tris;      // 3 x float4 per triangle in the tree's slot order
    float4* d_nrms;
    uint32_t n_nodes;
    uint32_t depth;      // levels of the tree
};

// d_verts / d_norms: 9 floats per triangle (P0,P1,P2 / N0,N1,N2), d_tri_mat: material per triangle, all on the device.
// cmin / cmax: bounds of the triangle centroids.  Returns 0 on success (synchronous: the stream is drained).
int prt_gpu_bvh8_build(hipStream_t st, const float* d_verts, const float* d_norms, const uint32_t* d_tri_mat, uint32_t n_tris,
                       uint32_t n_prims, const float cmin[3], const float cmax[3], PrtGpuBvh* out);
// The quality builder (round 2): the same Morton sort, then PLOC (locally-ordered agglomerative clustering) for the binary
// topology and the SAH-optimal collapse to 8-wide nodes by dynamic programming, all on the device.  Same contract.
// leaf_cost: cost of testing one primitive of a leaf relative to one 8-wide node visit (0 = the builder's default for
// triangles; large for a top-level tree, whose "primitives" are whole instances that are entered without a box test of
// their own: every instance then gets a leaf to itself, except copies whose boxes coincide).
int prt_gpu_bvh8_build_ploc(hipStream_t st, const float* d_verts, const float* d_norms, const uint32_t* d_tri_mat, uint32_t n_tris,
                            uint32_t n_prims, const float cmin[3], const float cmax[3], PrtGpuBvh* out, float leaf_cost = 0.0f);

// Measurement aid (prt_set_param("sort_rays", 1 | 2)): idx2[0..n) = the order of rays 0..n-1 by (Morton cell of the origin
// in a 32^3 grid over [bmin, bmax], direction octant) (mode 1) or (octant, cell) (mode 2).  keys, keys2, idx, idx2: n
// uint32 each; temp: prt_sort_rays_temp_bytes(n) bytes.
size_t prt_sort_rays_temp_bytes(uint32_t n);
int prt_sort_rays(hipStream_t st, const float4* ro, const float4* rd, uint32_t n, const float bmin[3], const float bmax[3],
                  uint32_t mode, uint32_t* keys, uint32_t* keys2, uint32_t* idx, uint32_t* idx2, void* temp, size_t temp_bytes);

// Refit: new vertex positions over an existing 8-wide tree on the device.  d_nodes8: n_nodes nodes at a stride of
// stride_dwords (20 packed / 32 one node per 128-B line); level_nodes (HOST array, n_nodes entries): the node indices sorted
// by tree level, level l = level_nodes[level_start[l] .. level_start[l + 1]) (level_start: host array of n_levels + 1
// entries); d_verts / d_norms: 9 floats per triangle in INPUT order (d_norms may be null);
// d_tris / d_nrms: the scene's records in slot order, rewritten in place.  root_box[6] receives the new root bounds.
// Synchronous.  Returns 0, a hipError_t, or -6 if a box does not fit its node's quantization grid.
// tally (may be null) grows by the bytes the call copies between host and device.
struct PrtCopyTally {
    uint64_t h2d, d2h;
};
int prt_gpu_bvh8_refit(hipStream_t st, uint32_t* d_nodes8, uint32_t stride_dwords, uint32_t n_nodes, const uint32_t* level_nodes,
                       const uint32_t* level_start, uint32_t n_levels, const float* d_verts, const float* d_norms, uint32_t n_tris,
                       uint32_t n_prims, float4* d_tris, float4* d_nrms, float root_box[6], PrtCopyTally* tally = nullptr);

// ---- refit from device arrays (prt_refit_meshes_device) ----
// The meshes' vertex arrays: HOST arrays of n_meshes DEVICE pointers (n_vertices x 3 floats each) and the prefixes of
// PrtRefitTables (prt_scene.h; n_meshes + 1 entries).  The d_* tables below are PrtRefitTables' arrays on the device.
#define PRT_REFIT_CHUNK 16  // meshes a launch serves; their pointers and ranges are kernel arguments
struct PrtRefitInputs {
    uint32_t n_meshes;
    const float* const* pos;
    const uint32_t* tri_first;
    const uint32_t* vert_first;
};
// The working arrays of a refit and the tree's level list, kept on the device with the scene:
// cbox 48 floats, nbox 6 floats per node, 4 counters, level_nodes one entry per node.
struct PrtRefitScratch {
    float *cbox, *nbox;
    uint32_t *counters, *level_nodes;
};
// d_out[0] = the bits of the largest finite |position coordinate| over the vertices the index buffers reference,
// d_out[1] = 1 (a non-finite position) | 2 (a non-finite supplied normal); nrm_supplied: n_meshes device pointers, null
// entries are skipped.  d_out: 4 words.  Enqueues; returns 0 or a hipError_t.
int prt_gpu_refit_validate(hipStream_t st, const PrtRefitInputs& in, const float* const* nrm_supplied, const uint32_t* d_corner, uint32_t* d_out);
// Vertex normals by compute_normals' rule (prt_host.cpp) into nout[m] (n_vertices x 3 floats on the device) for every
// mesh with nout[m] != null.  Enqueues; returns 0 or a hipError_t.
int prt_gpu_mesh_normals(hipStream_t st, const PrtRefitInputs& in, float* const* nout, const uint32_t* d_corner, const uint32_t* d_csr_start,
                         const uint32_t* d_csr_corner);
// prt_gpu_bvh8_refit with the records gathered through d_corner from `in` and nrm (n_meshes device pointers, none null),
// over the arrays of `keep` (level_nodes filled).  Synchronous; the same return values.
int prt_gpu_bvh8_refit_indexed(hipStream_t st, uint32_t* d_nodes8, uint32_t stride_dwords, uint32_t n_nodes, const uint32_t* level_start,
                               uint32_t n_levels, const PrtRefitInputs& in, const float* const* nrm, const uint32_t* d_corner, uint32_t n_tris,
                               uint32_t n_prims, float4* d_tris, float4* d_nrms, const PrtRefitScratch& keep, float root_box[6], PrtCopyTally* tally);
// d_out[9 i ..] = the three vertices of triangle d_light_tris[i] (mesh and face order).  Enqueues; returns 0 or a hipError_t.
int prt_gpu_light_gather(hipStream_t st, const PrtRefitInputs& in, const uint32_t* d_corner, const uint32_t* d_light_tris, uint32_t n_light_tris,
                         float* d_out);

// ---- moving placed copies (prt_set_instance_transforms); all three enqueue on `st` and return 0 or a hipError_t ----
// One thread per top-level leaf slot.  d_xf: 32 floats per placed copy (PrtInstance::mat, ::inv); d_inst_mesh[i]: the row
// of d_mesh_box (6 floats: min, max) instance i takes its box from: its mesh's box in its own space, or, for the n_world
// (0 | 1) leading identity instance of the world-space meshes, its world box as it is.  d_slot_inst: leaf slot ->
// instance (n_insts entries).  Writes mat / inv / inv_scale of every placed copy of d_insts (DevInstance) and, into
// d_recs[3 * slot ..], every instance's world box as the builders' degenerate triangle with the instance in word 3.
int prt_gpu_place_copies(hipStream_t st, const float* d_xf, const float* d_mesh_box, const uint32_t* d_inst_mesh, const uint32_t* d_slot_inst,
                         uint32_t n_insts, uint32_t n_world, void* d_insts, float4* d_recs);
// The refit of prt_gpu_bvh8_refit over records that are already in place (d_recs of prt_gpu_place_copies): boxes
// bottom-up, nodes re-quantized.  Synchronous.  Returns 0, a hipError_t, or -6 like prt_gpu_bvh8_refit.
int prt_gpu_bvh8_refit_top(hipStream_t st, uint32_t* d_nodes8, uint32_t stride_dwords, uint32_t n_nodes, const uint32_t* level_nodes,
                           const uint32_t* level_start, uint32_t n_levels, const float4* d_recs, float root_box[6]);
// child_base of nodes [first_node, n_nodes) and root of n_insts instances (DevInstance) grow by delta (mod 2^32).
int prt_gpu_rebase(hipStream_t st, uint32_t* d_nodes8, uint32_t stride_dwords, uint32_t first_node, uint32_t n_nodes, void* d_insts,
                   uint32_t n_insts, uint32_t delta);

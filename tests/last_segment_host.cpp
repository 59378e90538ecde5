// last_segment_host.cpp — the HIP-free half of the last-segment route (DESIGN.md section 3 "The last segment"): the plan's
// last_segment against the conditions spelled out here, over every combination of the facts (prt_route.h), and the scene fact
// mesh_emissive of compiled scenes (prt_scene.cpp).
//   g++ -std=c++17 -O1 -I include -I parallelraytracing_amd/csrc tests/last_segment_host.cpp parallelraytracing_amd/csrc/prt_host.cpp
//       parallelraytracing_amd/csrc/bvh.cpp parallelraytracing_amd/csrc/prt_scene.cpp -pthread -o /tmp/last_segment_host
//   /tmp/last_segment_host assets/models
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "prt.h"
#include "prt_route.h"
#include "prt_scene.h"

static int n_fail = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        printf("UNEXPECTED: %s\n", what);
        ++n_fail;
    }
}

// every combination of the 23 boolean facts of a batch, the three-valued ones and the tunable's settings
static uint64_t check_plans() {
    uint64_t n_on = 0, n = 0;
    for (uint32_t idx = 0; idx < (1u << 23); ++idx) {
        PrtRouteFacts f{};
        uint32_t b = 0;
        auto bit = [&]() { return ((idx >> b++) & 1u) != 0u; };
        f.lit = bit(), f.mesh_lights = bit(), f.env = bit(), f.tex = bit(), f.lens = bit(), f.listed = bit(), f.film_stats = bit();
        f.has_nodes = bit(), f.has_bvh2 = bit(), f.insts = bit(), f.abvh = bit(), f.few_prims = bit();
        f.jitter = bit(), f.sa = bit(), f.multi_sample = bit();
        f.variant0 = bit(), f.compact_primary = bit(), f.primary_walk = bit(), f.takes_primary = bit(), f.path_gate = bit();
        f.mesh_emissive = bit(), f.depth_ge2 = bit(), f.sort_rays = bit();
        f.primary_hit = true;
        for (uint32_t pk = 0; pk < 3; ++pk)
            for (uint32_t fuse = 0; fuse < 2; ++fuse)
                for (uint32_t ls = 0; ls < 3; ++ls) {
                    f.path_kernel = pk, f.fuse = fuse, f.last_segment = ls;
                    const PrtRoutePlan p = prt_plan_route(f);
                    const bool on = !p.path && p.fuse == 0u && !f.lit && !f.mesh_emissive && f.has_nodes && p.walk8 && !f.sort_rays && f.depth_ge2;
                    if (p.last_segment != (on ? ls : 0u)) {
                        if (n_fail < 10) printf("UNEXPECTED: facts %08x path_kernel %u fuse %u setting %u: plan says %u\n", idx, pk, fuse, ls, p.last_segment);
                        ++n_fail;
                    }
                    n_on += p.last_segment != 0u;
                    ++n;
                }
    }
    printf("%llu plans, %llu with the route on\n", (unsigned long long)n, (unsigned long long)n_on);
    return n_on;
}

// Rows written by hand, independent of the plan's own path / fuse / walk8: the facts of the headline batch (a one-level
// host-built tree, two analytic primitives, 256 samples, no jitter, the defaults of every tunable), then one fact changed at a time.
static void check_rows() {
    PrtRouteFacts c3{};
    c3.has_nodes = c3.has_bvh2 = c3.few_prims = c3.multi_sample = c3.variant0 = c3.compact_primary = c3.primary_walk = c3.takes_primary = true;
    c3.primary_hit = true, c3.path_gate = false, c3.path_kernel = 0u, c3.fuse = 0u, c3.depth_ge2 = true;
    auto plan = [](PrtRouteFacts f, uint32_t setting) {
        f.last_segment = setting;
        return prt_plan_route(f).last_segment;
    };
    for (uint32_t s = 0; s < 3; ++s) expect(plan(c3, s) == s, "the headline batch takes the tunable as it is");
    PrtRouteFacts f = c3;
    f.depth_ge2 = false;
    expect(plan(f, 2) == 0u, "max_depth 1: off");
    f = c3, f.fuse = 1u;
    expect(plan(f, 2) == 0u, "fused segments: off");
    f = c3, f.fuse = 1u, f.few_prims = false;
    expect(plan(f, 2) == 2u, "the fuse tunable without a scene that fuses (more than 16 analytic primitives): on");
    f = c3, f.lit = true;
    expect(plan(f, 1) == 0u, "lighting: off");
    f = c3, f.mesh_emissive = true;
    expect(plan(f, 1) == 0u, "an emissive triangle: off");
    f = c3, f.has_nodes = false;
    expect(plan(f, 1) == 0u, "no tree: off");
    f = c3, f.sort_rays = true;
    expect(plan(f, 1) == 0u, "sort_rays: off");
    f = c3, f.variant0 = false;
    expect(plan(f, 1) == 0u, "variant 1 / 2 on a one-level host-built scene walks with k_intersect: off");
    f = c3, f.variant0 = false, f.insts = true;
    expect(plan(f, 1) == 1u, "placed copies have the 8-wide kernel only, whatever the variant: on");
    f = c3, f.variant0 = false, f.has_bvh2 = false;
    expect(plan(f, 1) == 1u, "a device-built tree has the 8-wide kernel only: on");
    f = c3, f.path_kernel = 2u, f.path_gate = true;
    expect(plan(f, 1) == 0u, "the path instance: off");
    f = c3, f.path_kernel = 2u, f.path_gate = false;
    expect(plan(f, 1) == 1u, "path_kernel without its gate: the pipeline, on");
    f = c3, f.path_kernel = 1u, f.path_gate = true;
    expect(plan(f, 1) == 1u, "path_kernel 1 with more than one sample: the pipeline, on");
    f = c3, f.path_kernel = 1u, f.path_gate = true, f.multi_sample = false;
    expect(plan(f, 1) == 0u, "path_kernel 1 with one sample: the path instance, off");
    f = c3, f.env = true, f.tex = true, f.lens = true, f.jitter = true, f.sa = true, f.abvh = true, f.film_stats = true, f.listed = true;
    expect(plan(f, 2) == 2u, "environment, textures, lens, jitter, roulette, a primitive BVH, film statistics and a tile list leave it on");
}

static PrtMesh mesh_of(const PrtMeshData* m, uint32_t material) {
    return PrtMesh{prt_mesh_positions(m), prt_mesh_normals(m), prt_mesh_indices(m), prt_mesh_vertex_count(m), prt_mesh_triangle_count(m), material};
}

// materials 0 ground (Lambertian), 1 light (emissive), 2 body (Lambertian): the layout of the benchmark scenes (scenes.py
// mesh_scene): a ground quad, an emissive quad, the mesh
static bool mesh_emissive_of(const PrtMeshData* world, uint32_t world_mat, const PrtMeshData* placed, uint32_t placed_mat, bool emissive_quad, bool* ok) {
    const std::vector<PrtMaterial> mats = {{PRT_MAT_LAMBERTIAN, {0.5f, 0.5f, 0.5f}, 0.0f}, {PRT_MAT_EMISSIVE, {15.0f, 15.0f, 15.0f}, 0.0f},
                                           {PRT_MAT_LAMBERTIAN, {0.8f, 0.8f, 0.8f}, 0.0f}};
    const float zero[3] = {0, 0, 0}, flip[3] = {180.0f, 0, 0}, one[3] = {1, 1, 1}, t0[3] = {0, -1, 0}, t1[3] = {0, 5, 0}, t2[3] = {3, 0, 0};
    std::vector<PrtPrimitive> prims(emissive_quad ? 2 : 1);
    prims[0] = PrtPrimitive{};
    prims[0].shape_type = PRT_SHAPE_QUAD, prims[0].shape_param[0] = 20, prims[0].shape_param[1] = 20, prims[0].material_id = 0;
    prt_make_transform(one, zero, t0, prims[0].mat, prims[0].inv);
    if (emissive_quad) {
        prims[1] = PrtPrimitive{};
        prims[1].shape_type = PRT_SHAPE_QUAD, prims[1].shape_param[0] = 4, prims[1].shape_param[1] = 4, prims[1].material_id = 1;
        prt_make_transform(one, flip, t1, prims[1].mat, prims[1].inv);
    }
    std::vector<PrtMesh> meshes, imeshes;
    std::vector<PrtInstance> insts;
    if (world) meshes.push_back(mesh_of(world, world_mat));
    if (placed) {
        imeshes.push_back(mesh_of(placed, 2));
        insts.resize(2);
        for (size_t k = 0; k < insts.size(); ++k) {
            insts[k] = PrtInstance{};
            insts[k].mesh = 0;
            insts[k].material_id = k == 1 ? placed_mat : 2u;
            prt_make_transform(one, zero, k == 1 ? t2 : zero, insts[k].mat, insts[k].inv);
        }
    }
    PrtSceneDesc d{};
    d.materials = mats.data(), d.n_materials = (uint32_t)mats.size();
    d.primitives = prims.data(), d.n_primitives = (uint32_t)prims.size();
    d.meshes = meshes.data(), d.n_meshes = (uint32_t)meshes.size();
    d.instanced_meshes = imeshes.data(), d.n_instanced_meshes = (uint32_t)imeshes.size();
    d.instances = insts.data(), d.n_instances = (uint32_t)insts.size();
    d.sky[0] = 0.4f, d.sky[1] = 0.3f, d.sky[2] = 0.6f;
    PrtHostScene hs;
    std::string e;
    const PrtSceneOptions opt{1.0f / 262144.0f, true, nullptr};
    if (prt_compile_scene(&d, opt, &hs, &e)) {
        printf("compile failed: %s\n", e.c_str());
        *ok = false;
        return false;
    }
    return hs.mesh_emissive;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "assets/models";
    expect(check_plans() != 0u, "no combination of the facts turns the route on");
    check_rows();
    char err[256];
    PrtMeshData *dragon = nullptr, *ico = nullptr;
    if (prt_mesh_load_ply((dir + "/dragon.ply").c_str(), &dragon, err, sizeof(err)) || prt_mesh_load_ply((dir + "/icosahedron.ply").c_str(), &ico, err, sizeof(err))) {
        printf("load failed: %s\n", err);
        return 1;
    }
    bool ok = true;
    expect(!mesh_emissive_of(dragon, 2, nullptr, 0, true, &ok), "the benchmark scene (Lambertian dragon, emissive quad) has no emissive triangle");
    expect(!mesh_emissive_of(ico, 2, ico, 2, true, &ok), "a scene whose only emitter is an analytic quad");
    expect(!mesh_emissive_of(ico, 0, nullptr, 0, false, &ok), "a scene without any emitter");
    expect(mesh_emissive_of(ico, 1, nullptr, 0, true, &ok), "an emissive world-space mesh");
    expect(mesh_emissive_of(ico, 1, nullptr, 0, false, &ok), "an emissive world-space mesh and no analytic emitter");
    expect(mesh_emissive_of(nullptr, 0, ico, 1, true, &ok), "an emissive placed copy");
    expect(mesh_emissive_of(ico, 2, ico, 1, false, &ok), "an emissive placed copy next to a Lambertian world mesh");
    expect(ok, "a scene did not compile");
    prt_mesh_free(dragon);
    prt_mesh_free(ico);
    if (n_fail) return 1;
    printf("last-segment host checks passed\n");
    return 0;
}

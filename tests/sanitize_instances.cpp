// sanitize_instances.cpp — the host half of prt_set_instance_transforms (prt_scene.cpp: the checks, the instance table and
// world boxes, a new top-level tree from the host builder, the splice in front of the untouched mesh trees, the triangle
// lights of placed copies) under AddressSanitizer + UBSan on the CPU.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I parallelraytracing_amd/csrc \
//       tests/sanitize_instances.cpp parallelraytracing_amd/csrc/prt_host.cpp parallelraytracing_amd/csrc/bvh.cpp \
//       parallelraytracing_amd/csrc/prt_scene.cpp -pthread -o /tmp/sanitize_instances
//   /tmp/sanitize_instances assets/models [n_transform_sets]
// The scene: a world bunny (and a variant without it), 12 copies of the icosahedron and of cube_uv, two of them emissive, 3
// analytic primitives.  n random valid transform sets (scales over six binary orders of magnitude, copies onto one spot
// now and then) are applied in sequence; every 20th result is compared field by field with a fresh prt_compile_scene of
// the moved description.  Every invalid set must be refused with PRT_ERR_INVALID and leave the scene untouched, and a
// top level too deep for the traversal stack must be refused before anything is written.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "prt.h"
#include "prt_scene.h"

static const PrtSceneOptions kOpt{1.0f / 262144.0f, true, nullptr};
static int n_fail = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        printf("  ^^^ UNEXPECTED: %s\n", what);
        ++n_fail;
    }
}

static PrtMesh mesh_of(const PrtMeshData* m, uint32_t material) {
    return PrtMesh{prt_mesh_positions(m), prt_mesh_normals(m), prt_mesh_indices(m), prt_mesh_vertex_count(m), prt_mesh_triangle_count(m), material};
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// everything of a compiled scene that an update may write
static bool same_scene(const PrtHostScene& a, const PrtHostScene& b) {
    return same(a.nodes8_all, b.nodes8_all) && same(a.tlas_inst, b.tlas_inst) && same(a.dev_insts, b.dev_insts) && same(a.tri_records, b.tri_records) &&
           same(a.nrm_records, b.nrm_records) && memcmp(&a.sc, &b.sc, sizeof(a.sc)) == 0 && a.top_nodes == b.top_nodes && a.top_depth == b.top_depth &&
           a.bvh_info.n_nodes8 == b.bvh_info.n_nodes8 && a.bvh_info.depth8 == b.bvh_info.depth8 && same(a.ml.records, b.ml.records) &&
           same(a.ml.thr, b.ml.thr) && same(a.ml.width, b.ml.width) && same(a.ml.visible, b.ml.visible) && same(a.ml.bucket, b.ml.bucket) &&
           a.ml.n_search == b.ml.n_search && a.ml.n_emitters_unsampled == b.ml.n_emitters_unsampled && same(a.ml.power, b.ml.power) &&
           a.placed_meshes.size() == b.placed_meshes.size() &&
           (a.placed_meshes.empty() || memcmp(a.placed_meshes.data(), b.placed_meshes.data(), a.placed_meshes.size() * sizeof(PrtPlacedMesh)) == 0);
}

static int update(PrtHostScene& hs, const std::vector<PrtInstance>& insts, uint32_t n, std::string* err) {
    int rc = prt_check_instance_update(hs, insts.empty() ? nullptr : insts.data(), n, err);
    if (rc) return rc;
    PrtInstanceUpdate up;
    prt_instance_tables(hs, insts.data(), &up);
    if ((rc = prt_build_top_level(kOpt, hs, &up, &hs.gpu_build_ms, err))) return rc;
    prt_commit_top_level(&hs, up);
    prt_commit_instances(&hs, up, insts.data());
    return PRT_OK;
}

static void place(PrtInstance& in, float s, const float* eu, const float* tr) {
    const float sc[3] = {s, s, s};
    prt_make_transform(sc, eu, tr, in.mat, in.inv);
}

static int run(const std::string& dir, bool world, int n_sets) {
    char err[256];
    PrtMeshData *bunny = nullptr, *ico = nullptr, *cube = nullptr;
    if (prt_mesh_load_ply((dir + "/bunny.ply").c_str(), &bunny, err, sizeof(err)) || prt_mesh_load_ply((dir + "/icosahedron.ply").c_str(), &ico, err, sizeof(err)) ||
        prt_mesh_load_ply((dir + "/cube_uv.ply").c_str(), &cube, err, sizeof(err))) {
        printf("load failed: %s\n", err);
        return 1;
    }
    const std::vector<PrtMaterial> mats = {{PRT_MAT_LAMBERTIAN, {0.8f, 0.8f, 0.8f}, 0.0f}, {PRT_MAT_EMISSIVE, {6.0f, 5.0f, 4.0f}, 0.0f},
                                           {PRT_MAT_METAL, {0.9f, 0.9f, 0.9f}, 0.05f}};
    std::vector<PrtPrimitive> prims(3);
    const float zero[3] = {0, 0, 0}, flip[3] = {180.0f, 0, 0}, one[3] = {1, 1, 1};
    const float t0[3] = {0, -3, 0}, t1[3] = {0, 8, 0}, t2[3] = {2.5f, -2.2f, 1.5f};
    prims[0] = PrtPrimitive{};
    prims[0].shape_type = PRT_SHAPE_QUAD, prims[0].shape_param[0] = 40, prims[0].shape_param[1] = 40, prims[0].material_id = 0;
    prt_make_transform(one, zero, t0, prims[0].mat, prims[0].inv);
    prims[1] = PrtPrimitive{};
    prims[1].shape_type = PRT_SHAPE_QUAD, prims[1].shape_param[0] = 4, prims[1].shape_param[1] = 4, prims[1].material_id = 1;
    prt_make_transform(one, flip, t1, prims[1].mat, prims[1].inv);
    prims[2] = PrtPrimitive{};
    prims[2].shape_type = PRT_SHAPE_CIRCLE, prims[2].shape_param[0] = 0.8f, prims[2].material_id = 2;
    prt_make_transform(one, zero, t2, prims[2].mat, prims[2].inv);
    std::vector<PrtMesh> meshes;
    if (world) meshes.push_back(mesh_of(bunny, 0));
    const std::vector<PrtMesh> imeshes = {mesh_of(ico, 0), mesh_of(cube, 0)};
    std::mt19937 rng(world ? 7u : 8u);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    auto random_set = [&](std::vector<PrtInstance>& insts) {
        const bool one_spot = u01(rng) < 0.1f;
        const float spot[3] = {10.0f * u01(rng), 10.0f * u01(rng), 10.0f * u01(rng)};
        for (size_t k = 0; k < insts.size(); ++k) {
            const float s = std::ldexp(0.5f + u01(rng), (int)(u01(rng) * 6.0f) - 3);
            const float eu[3] = {360.0f * u01(rng) - 180.0f, 360.0f * u01(rng) - 180.0f, 360.0f * u01(rng) - 180.0f};
            const float span = u01(rng) < 0.2f ? 1e4f : 6.0f;
            const float tr[3] = {span * (2 * u01(rng) - 1), span * (2 * u01(rng) - 1), span * (2 * u01(rng) - 1)};
            place(insts[k], s, eu, one_spot ? spot : tr);
        }
    };
    std::vector<PrtInstance> insts(12);
    for (size_t k = 0; k < insts.size(); ++k) {
        insts[k] = PrtInstance{};
        insts[k].mesh = (uint32_t)(k & 1);
        insts[k].material_id = (k == 1 || k == 6) ? 1u : (uint32_t)(k % 3 == 2 ? 2 : 0);
    }
    random_set(insts);
    PrtSceneDesc d{};
    d.materials = mats.data(), d.n_materials = (uint32_t)mats.size();
    d.primitives = prims.data(), d.n_primitives = (uint32_t)prims.size();
    d.meshes = meshes.data(), d.n_meshes = (uint32_t)meshes.size();
    d.instanced_meshes = imeshes.data(), d.n_instanced_meshes = (uint32_t)imeshes.size();
    d.instances = insts.data(), d.n_instances = (uint32_t)insts.size();
    d.sky[0] = 0.4f, d.sky[1] = 0.3f, d.sky[2] = 0.6f;
    PrtHostScene hs;
    std::string e;
    if (prt_compile_scene(&d, kOpt, &hs, &e)) {
        printf("compile failed: %s\n", e.c_str());
        return 1;
    }
    expect(hs.ml.runs.size() == 2u && hs.inst_mesh.size() == 12u && hs.placed_meshes.size() == 2u, "the compiled scene's tables");
    // ---- valid transform sets, in sequence ----
    uint32_t n_counts = 0, last_top = hs.top_nodes;
    for (int it = 0; it < n_sets; ++it) {
        random_set(insts);
        const int rc = update(hs, insts, (uint32_t)insts.size(), &e);
        if (rc) {
            printf("  set %d refused (%d): %s\n", it, rc, e.c_str());
            ++n_fail;
            continue;
        }
        n_counts += hs.top_nodes != last_top;
        last_top = hs.top_nodes;
        if (it % 20 == 19 || it + 1 == n_sets) {
            PrtHostScene fresh;
            if (prt_compile_scene(&d, kOpt, &fresh, &e)) {
                printf("  set %d: the moved description does not compile: %s\n", it, e.c_str());
                ++n_fail;
            } else {
                expect(same_scene(hs, fresh), "an updated scene differs from a fresh compile of the moved description");
            }
        }
    }
    printf("  %s world mesh: %d transform sets, the top level changed its node count %u times; %zu light candidates, %zu lights\n", world ? "with" : "without",
           n_sets, n_counts, hs.ml.power.size(), hs.ml.visible.size());
    // ---- invalid sets: PRT_ERR_INVALID, the scene untouched ----
    const PrtHostScene before = hs;
    auto refused = [&](const char* what, const std::vector<PrtInstance>& bad, uint32_t n, const char* msg) {
        std::string er;
        const int rc = update(hs, bad, n, &er);
        const bool ok = rc == PRT_ERR_INVALID && er.find(msg) != std::string::npos && same_scene(hs, before);
        printf("  update %-36s %s (%d): %s\n", what, ok ? "refused" : "^^^ UNEXPECTED", rc, er.c_str());
        n_fail += !ok;
    };
    std::vector<PrtInstance> bad = insts;
    bad.pop_back();
    refused("one copy fewer", bad, (uint32_t)bad.size(), "placed copies, not");
    bad = insts;
    bad.push_back(insts[0]);
    refused("one copy more", bad, (uint32_t)bad.size(), "placed copies, not");
    refused("null array", {}, 12, "null instance array");
    bad = insts;
    bad[4].mesh ^= 1u;
    refused("another mesh", bad, 12, "another mesh or material");
    bad = insts;
    bad[11].mesh = 7;
    refused("mesh out of range", bad, 12, "another mesh or material");
    bad = insts;
    bad[0].material_id = 2;
    refused("another material", bad, 12, "another mesh or material");
    bad = insts;
    bad[3].mat[0] *= 2.0f;
    refused("non-uniform scale", bad, 12, "uniform scale");
    bad = insts;
    bad[5].inv[13] += 0.75f;
    refused("inv is not the inverse", bad, 12, "uniform scale");
    bad = insts;
    bad[6].mat[7] = 0.5f;
    refused("bottom row", bad, 12, "uniform scale");
    bad = insts;
    bad[7].mat[12] = NAN;
    refused("NaN translation", bad, 12, "uniform scale");
    bad = insts;
    bad[8].mat[5] = INFINITY;
    refused("infinite entry", bad, 12, "uniform scale");
    bad = insts;
    {
        const float tiny[3] = {0, 0, 0};
        place(bad[9], std::ldexp(1.0f, -40), tiny, tiny);
    }
    refused("scale 2^-40", bad, 12, "uniform scale");
    // a top level too deep for the stack: refused by prt_build_top_level, which does not write the scene
    {
        PrtHostScene deep = hs;
        deep.max_mesh_depth = 13u - deep.top_depth;
        std::string er;
        const int rc = update(deep, insts, 12, &er);
        deep.max_mesh_depth = hs.max_mesh_depth;
        expect(rc == PRT_ERR_INVALID && er.find("too deep") != std::string::npos && same_scene(deep, hs), "a top level too deep was not refused cleanly");
    }
    // a scene without placed copies
    {
        PrtSceneDesc d0 = d;
        d0.n_instances = 0;
        d0.n_instanced_meshes = 0;
        PrtHostScene plain;
        std::string er;
        expect(prt_compile_scene(&d0, kOpt, &plain, &er) == PRT_OK && update(plain, insts, 12, &er) == PRT_ERR_INVALID && er.find("no placed copies") != std::string::npos,
               "a scene without placed copies accepted an update");
    }
    // the scene is still usable
    random_set(insts);
    expect(update(hs, insts, 12, &e) == PRT_OK, "a valid update after the refusals");
    prt_mesh_free(bunny);
    prt_mesh_free(ico);
    prt_mesh_free(cube);
    return 0;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "assets/models";
    const int n_sets = argc > 2 ? atoi(argv[2]) : 200;
    if (run(dir, true, n_sets) || run(dir, false, n_sets)) return 1;
    if (n_fail) {
        printf("%d unexpected results\n", n_fail);
        return 1;
    }
    printf("no sanitizer report\n");
    return 0;
}

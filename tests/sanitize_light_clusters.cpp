// sanitize_light_clusters.cpp — the cluster builder of clustered light selection (prt_scene.cpp: prt_build_light_clusters, and
// the rebuild with the candidate table in prt_rebuild_mesh_lights) under AddressSanitizer + UBSan on the CPU.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I parallelraytracing_amd/csrc \
//       tests/sanitize_light_clusters.cpp parallelraytracing_amd/csrc/prt_host.cpp parallelraytracing_amd/csrc/bvh.cpp \
//       parallelraytracing_amd/csrc/prt_scene.cpp -pthread -o /tmp/sanitize_light_clusters
//   /tmp/sanitize_light_clusters assets/models [n_transform_sets]
// Scenes with emissive meshes and emissive placed copies: a mesh with zero-area and coincident triangles, a scene with one
// light, a scene with none; each compiled for every max_clusters 1..64 with the invariants of the contract checked; then n
// random instance transform sets through the rebuild, every result compared with a fresh compile of the moved description.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "prt.h"
#include "prt_scene.h"

static int n_fail = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        printf("  ^^^ UNEXPECTED: %s\n", what);
        ++n_fail;
    }
}

static PrtSceneOptions options(uint32_t clusters) {
    PrtSceneOptions o{1.0f / 262144.0f, true, nullptr};
    o.light_clusters = clusters;
    return o;
}

static PrtMesh mesh_of(const PrtMeshData* m, uint32_t material) {
    return PrtMesh{prt_mesh_positions(m), prt_mesh_normals(m), prt_mesh_indices(m), prt_mesh_vertex_count(m), prt_mesh_triangle_count(m), material};
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static bool same_clusters(const PrtLightClusters& a, const PrtLightClusters& b) {
    return a.max_clusters == b.max_clusters && same(a.boxes, b.boxes) && same(a.range, b.range) && same(a.power_width, b.power_width) &&
           same(a.members, b.members) && same(a.thr, b.thr) && same(a.inner_width, b.inner_width) && same(a.cand_cluster, b.cand_cluster) &&
           same(a.cand_member, b.cand_member) && a.n_empty_inner == b.n_empty_inner;
}

// the invariants of include/prt.h "Clustered light selection" that need no second implementation
static void check_clusters(const PrtHostScene& hs, uint32_t max_clusters, const char* what) {
    const PrtLightClusters& lc = hs.lc;
    const PrtMeshLights& ml = hs.ml;
    const uint32_t K = lc.n_clusters();
    bool ok = K <= max_clusters && lc.max_clusters == max_clusters && lc.members.size() == ml.visible.size() && (K != 0u || ml.visible.empty());
    uint64_t sum_w = 0;
    std::vector<uint32_t> seen(ml.power.size(), 0u);
    uint32_t empty = 0;
    for (uint32_t c = 0; c < K && ok; ++c) {
        const uint32_t first = lc.range[4 * c], last = lc.range[4 * c + 1], n = lc.range[4 * c + 2];
        ok = ok && n > 0u && first + n <= lc.members.size() && last >= first && last < first + n;
        uint64_t inner = 0, w = 0;
        for (uint32_t j = first; j < first + n && ok; ++j) {
            const uint32_t cand = lc.members[j];
            ok = ok && cand < seen.size() && ml.cand_visible[cand] != 0xFFFFFFFFu && lc.cand_cluster[cand] == c && lc.cand_member[cand] == j;
            if (!ok) break;
            ++seen[cand];
            inner += lc.inner_width[j];
            empty += lc.inner_width[j] == 0u;
            w += ml.width[ml.cand_visible[cand]];
            for (int a = 0; a < 3; ++a)
                ok = ok && lc.boxes[8 * c + a] <= ml.box[6 * (size_t)cand + a] && lc.boxes[8 * c + 4 + a] >= ml.box[6 * (size_t)cand + 3 + a];
            if (j > first) ok = ok && lc.members[j] > lc.members[j - 1];
        }
        ok = ok && inner == (1ull << 32) && w == lc.power_width[c] && lc.inner_width[last] != 0u && lc.boxes[8 * c + 7] >= 1e-30f;
        sum_w += w;
    }
    for (uint32_t cand : ml.visible) ok = ok && seen[cand] == 1u;
    ok = ok && (K == 0u || sum_w == (1ull << 32)) && empty == lc.n_empty_inner;
    if (!ok) printf("  %s, max_clusters %u, %u clusters\n", what, max_clusters, K);
    expect(ok, "a cluster table breaks an invariant");
}

static int run(const std::string& dir, int n_sets) {
    char err[256];
    PrtMeshData *bunny = nullptr, *ico = nullptr;
    if (prt_mesh_load_ply((dir + "/bunny.ply").c_str(), &bunny, err, sizeof(err)) || prt_mesh_load_ply((dir + "/icosahedron.ply").c_str(), &ico, err, sizeof(err))) {
        printf("load failed: %s\n", err);
        return 1;
    }
    const std::vector<PrtMaterial> mats = {{PRT_MAT_LAMBERTIAN, {0.8f, 0.8f, 0.8f}, 0.0f}, {PRT_MAT_EMISSIVE, {6.0f, 5.0f, 4.0f}, 0.0f}};
    // zero-area, coincident, tiny and ordinary triangles in one emissive mesh
    const float dv[] = {0, 0, 0, 1, 0, 0, 0, 1, 0,  2, 0, 0, 3, 0, 0, 4, 0, 0,  5, 0, 0, 5, 0, 0, 5, 1, 0,  0, 0, 0, 1, 0, 0, 0, 1, 0,
                        0, 0, 0, 1, 0, 0, 0, 1, 0,  0, 0, 6, 1e-6f, 0, 6, 0, 1e-6f, 6,  7, 0, 0, 8, 0, 0, 7, 1, 0,  9, 9, 9, 9, 9, 9, 9, 9, 9};
    const uint32_t n_dv = sizeof(dv) / sizeof(dv[0]) / 3;
    std::vector<float> dn(3 * n_dv, 0.0f);
    std::vector<uint32_t> di(n_dv);
    for (uint32_t i = 0; i < n_dv; ++i) dn[3 * i + 2] = 1.0f, di[i] = i;
    const PrtMesh degenerate{dv, dn.data(), di.data(), n_dv, n_dv / 3, 1u};
    const PrtMesh one_tri{dv, dn.data(), di.data(), 3u, 1u, 1u};
    const PrtMesh no_area{dv + 9, dn.data(), di.data(), 3u, 1u, 1u};
    std::vector<PrtPrimitive> prims(2);
    const float zero[3] = {0, 0, 0}, flip[3] = {180.0f, 0, 0}, one[3] = {1, 1, 1}, t0[3] = {0, -3, 0}, t1[3] = {0, 8, 0};
    prims[0] = PrtPrimitive{};
    prims[0].shape_type = PRT_SHAPE_QUAD, prims[0].shape_param[0] = 40, prims[0].shape_param[1] = 40, prims[0].material_id = 0;
    prt_make_transform(one, zero, t0, prims[0].mat, prims[0].inv);
    prims[1] = PrtPrimitive{};
    prims[1].shape_type = PRT_SHAPE_QUAD, prims[1].shape_param[0] = 4, prims[1].shape_param[1] = 4, prims[1].material_id = 1;
    prt_make_transform(one, flip, t1, prims[1].mat, prims[1].inv);
    std::mt19937 rng(5u);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    std::vector<PrtInstance> insts(8);
    auto random_set = [&]() {
        const bool one_spot = u01(rng) < 0.1f;
        const float spot[3] = {10.0f * u01(rng), 10.0f * u01(rng), 10.0f * u01(rng)};
        for (PrtInstance& in : insts) {
            const float s = std::ldexp(0.5f + u01(rng), (int)(u01(rng) * 6.0f) - 3);
            const float sc[3] = {s, s, s};
            const float eu[3] = {360.0f * u01(rng) - 180.0f, 360.0f * u01(rng) - 180.0f, 360.0f * u01(rng) - 180.0f};
            const float span = u01(rng) < 0.2f ? 1e4f : 6.0f;
            const float tr[3] = {span * (2 * u01(rng) - 1), span * (2 * u01(rng) - 1), span * (2 * u01(rng) - 1)};
            prt_make_transform(sc, eu, one_spot ? spot : tr, in.mat, in.inv);
        }
    };
    for (size_t k = 0; k < insts.size(); ++k) {
        insts[k] = PrtInstance{};
        insts[k].mesh = 0;
        insts[k].material_id = (k % 3 == 1) ? 1u : 0u;  // copies 1, 4, 7 emit
    }
    random_set();
    const PrtMesh imesh = mesh_of(ico, 0);
    std::string e;
    // ---- every max_clusters on four scenes ----
    struct Case {
        const char* name;
        std::vector<PrtMesh> meshes;
        uint32_t n_prims, n_insts;
    };
    const std::vector<Case> cases = {{"bunny + degenerate mesh + copies", {mesh_of(bunny, 1), degenerate}, 2u, 8u},
                                     {"one light", {one_tri}, 1u, 0u},
                                     {"no light", {no_area}, 1u, 0u},
                                     {"degenerate mesh alone", {degenerate}, 0u, 0u}};
    for (const Case& cs : cases) {
        PrtSceneDesc d{};
        d.materials = mats.data(), d.n_materials = (uint32_t)mats.size();
        d.primitives = prims.data(), d.n_primitives = cs.n_prims;
        d.meshes = cs.meshes.data(), d.n_meshes = (uint32_t)cs.meshes.size();
        d.instanced_meshes = cs.n_insts ? &imesh : nullptr, d.n_instanced_meshes = cs.n_insts ? 1u : 0u;
        d.instances = cs.n_insts ? insts.data() : nullptr, d.n_instances = cs.n_insts;
        PrtHostScene hs;
        uint32_t most = 0;
        for (uint32_t K = 1; K <= PRT_LIGHT_MAX_CLUSTERS; ++K) {
            if (K == 1u || K == 32u) {  // through the compiler, then through the rebuild alone
                if (prt_compile_scene(&d, options(K), &hs, &e)) {
                    printf("compile failed: %s\n", e.c_str());
                    return 1;
                }
            } else {
                prt_build_light_clusters(&hs, K);
            }
            check_clusters(hs, K, cs.name);
            most = std::max(most, hs.lc.n_clusters());
        }
        prt_build_light_clusters(&hs, 0u);
        expect(hs.lc.max_clusters == 32u, "0 is the default of 32 clusters");
        printf("  %-34s %zu candidates, %zu lights, at most %u clusters, %u empty inner intervals at 64\n", cs.name, hs.ml.power.size(), hs.ml.visible.size(),
               most, hs.lc.n_empty_inner);
    }
    // ---- random transform sets through the rebuild ----
    const std::vector<PrtMesh> meshes = {mesh_of(bunny, 1), degenerate};
    PrtSceneDesc d{};
    d.materials = mats.data(), d.n_materials = (uint32_t)mats.size();
    d.primitives = prims.data(), d.n_primitives = 2u;
    d.meshes = meshes.data(), d.n_meshes = 2u;
    d.instanced_meshes = &imesh, d.n_instanced_meshes = 1u;
    d.instances = insts.data(), d.n_instances = (uint32_t)insts.size();
    const PrtSceneOptions opt = options(24u);
    PrtHostScene hs;
    if (prt_compile_scene(&d, opt, &hs, &e)) {
        printf("compile failed: %s\n", e.c_str());
        return 1;
    }
    for (int it = 0; it < n_sets; ++it) {
        random_set();
        int rc = prt_check_instance_update(hs, insts.data(), (uint32_t)insts.size(), &e);
        PrtInstanceUpdate up;
        if (!rc) {
            prt_instance_tables(hs, insts.data(), &up);
            rc = prt_build_top_level(opt, hs, &up, &hs.gpu_build_ms, &e);
        }
        if (rc) {
            printf("  set %d refused (%d): %s\n", it, rc, e.c_str());
            ++n_fail;
            continue;
        }
        prt_commit_top_level(&hs, up);
        prt_commit_instances(&hs, up, insts.data());
        check_clusters(hs, 24u, "after an instance update");
        if (it % 10 == 9 || it + 1 == n_sets) {
            PrtHostScene fresh;
            expect(prt_compile_scene(&d, opt, &fresh, &e) == PRT_OK && same_clusters(hs.lc, fresh.lc) && same(hs.ml.box, fresh.ml.box),
                   "rebuilt clusters differ from a fresh compile of the moved description");
        }
    }
    printf("  %d transform sets: %u clusters over %zu lights\n", n_sets, hs.lc.n_clusters(), hs.ml.visible.size());
    prt_mesh_free(bunny);
    prt_mesh_free(ico);
    return 0;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "assets/models";
    const int n_sets = argc > 2 ? atoi(argv[2]) : 100;
    if (run(dir, n_sets)) return 1;
    if (n_fail) {
        printf("%d unexpected results\n", n_fail);
        return 1;
    }
    printf("no sanitizer report\n");
    return 0;
}

// sanitize_host.cpp — the host-only parts of the library (PLY ingest, mesh tools, scene presets, image dumps: prt_host.cpp;
// the BVH builder: bvh.cpp; the scene compiler behind prt_set_scene: prt_scene.cpp) under AddressSanitizer + UBSan on the
// CPU (the GPU pool has no sanitizer runs).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I parallelraytracing_amd/csrc \
//       tests/sanitize_host.cpp parallelraytracing_amd/csrc/prt_host.cpp parallelraytracing_amd/csrc/bvh.cpp \
//       parallelraytracing_amd/csrc/prt_scene.cpp -pthread -o /tmp/sanitize_host
//   /tmp/sanitize_host assets/models [n_mutations]
// Exercises: every asset PLY (ascii / binary, with and without normals, quads), byte-level and header-level mutations of the
// small ones (must fail cleanly or load), refinement, transform, append, the host BVH builder at several sizes (incl. the
// degenerate ones: no triangle, one triangle, identical triangles, zero-area triangles), every preset, PPM / PFM writers;
// the scene compiler (host builder only) on every preset, mesh, many-primitive, instanced, empty and one-triangle scenes,
// and on hostile descriptions (bad indices, counts, materials, transforms, null arrays), which must be refused with
// PRT_ERR_INVALID and the documented message.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "bvh.h"
#include "prt.h"
#include "prt_scene.h"

static std::string slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static void flatten(const PrtMeshData* m, std::vector<float>& verts) {
    const uint32_t nt = prt_mesh_triangle_count(m);
    const float* P = prt_mesh_positions(m);
    const uint32_t* I = prt_mesh_indices(m);
    verts.resize(9 * (size_t)nt);
    for (uint32_t t = 0; t < nt; ++t)
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) verts[9 * (size_t)t + 3 * v + a] = P[3 * (size_t)I[3 * (size_t)t + v] + a];
}

static int build(const std::vector<float>& verts, const char* what) {
    BvhBuild b;
    const bool ok = bvh_build(verts.data(), (uint32_t)(verts.size() / 9), 3, 4, 63, &b);
    printf("  bvh %-28s %8zu triangles: %s, %zu binary nodes, %zu wide8 nodes, depth8 %u\n", what, verts.size() / 9, ok ? "ok" : "too deep",
           b.nodes.size() / 16, b.nodes8.size() / 20, b.depth8);
    return ok ? 0 : 1;
}

static PrtSceneDesc scene_desc(const std::vector<PrtMaterial>& mats, const std::vector<PrtPrimitive>& prims, const std::vector<PrtMesh>& meshes,
                               const std::vector<PrtMesh>& imeshes = {}, const std::vector<PrtInstance>& insts = {}) {
    PrtSceneDesc d{};
    d.materials = mats.data();
    d.n_materials = (uint32_t)mats.size();
    d.primitives = prims.data();
    d.n_primitives = (uint32_t)prims.size();
    d.meshes = meshes.data();
    d.n_meshes = (uint32_t)meshes.size();
    d.sky[0] = 0.4f, d.sky[1] = 0.3f, d.sky[2] = 0.6f;
    d.instanced_meshes = imeshes.data();
    d.n_instanced_meshes = (uint32_t)imeshes.size();
    d.instances = insts.data();
    d.n_instances = (uint32_t)insts.size();
    return d;
}

static PrtMesh mesh_of(const PrtMeshData* m, uint32_t material) {
    return PrtMesh{prt_mesh_positions(m), prt_mesh_normals(m), prt_mesh_indices(m), prt_mesh_vertex_count(m), prt_mesh_triangle_count(m), material};
}

static PrtPrimitive make_prim(uint32_t shape, float p0, float p1, uint32_t material, float scale, const float* euler, const float* tr) {
    PrtPrimitive p{};
    p.shape_type = shape;
    p.shape_param[0] = p0;
    p.shape_param[1] = p1;
    p.material_id = material;
    const float sc[3] = {scale, scale, scale};
    prt_make_transform(sc, euler, tr, p.mat, p.inv);
    return p;
}

// the scene compiler, host builder only: `want` = PRT_OK, or PRT_ERR_INVALID with `msg` in the error text
static int n_compile_fail = 0;
static PrtHostScene compile(const char* what, const PrtSceneDesc& d, int want = PRT_OK, const char* msg = "", bool prim_bvh = true) {
    PrtHostScene hs;
    std::string err;
    const PrtSceneOptions opt{1.0f / 262144.0f, prim_bvh, nullptr};
    const int rc = prt_compile_scene(&d, opt, &hs, &err);
    const bool ok = rc == want && (rc == PRT_OK || err.find(msg) != std::string::npos);
    if (rc == PRT_OK)
        printf("  scene %-44s ok: %zu prims, %u triangles, %zu+%zu nodes8, %zu prim-BVH nodes, %zu instances, %zu lights\n", what, hs.prims.size(),
               hs.sc.n_tris, hs.bvh.nodes8.size() / 20, hs.nodes8_all.size() / 20, hs.abvh.nodes4.size() / 32, hs.dev_insts.size(),
               hs.lights.size() / (4 * PRT_LIGHT_F4));
    else
        printf("  scene %-44s refused (%d): %s\n", what, rc, err.c_str());
    if (!ok) {
        printf("  ^^^ UNEXPECTED: wanted rc %d, message containing \"%s\"\n", want, msg);
        ++n_compile_fail;
    }
    return hs;
}

static int scene_compiler_cases(const std::string& dir) {
    char err[256];
    PrtMeshData *bunny = nullptr, *ico = nullptr;
    if (prt_mesh_load_ply((dir + "/bunny.ply").c_str(), &bunny, err, sizeof(err)) || prt_mesh_load_ply((dir + "/icosahedron.ply").c_str(), &ico, err, sizeof(err))) {
        printf("scene compiler: load failed: %s\n", err);
        return 1;
    }
    prt_mesh_refine(ico, 400);
    const std::vector<PrtMaterial> mats = {{PRT_MAT_LAMBERTIAN, {0.8f, 0.8f, 0.8f}, 0.0f}, {PRT_MAT_EMISSIVE, {4.0f, 4.0f, 4.0f}, 0.0f}};
    const std::vector<PrtPrimitive> no_prims;
    const std::vector<PrtMesh> no_meshes;
    // ---- scenes that compile ----
    for (int p = 0; p < 7; ++p) {
        std::vector<PrtMaterial> pm(2048);
        std::vector<PrtPrimitive> pp(2048);
        uint32_t nm = (uint32_t)pm.size(), np = (uint32_t)pp.size();
        if (prt_scene_preset(p, pm.data(), &nm, pp.data(), &np)) return 1;
        pm.resize(nm);
        pp.resize(np);
        compile(("preset " + std::to_string(p)).c_str(), scene_desc(pm, pp, no_meshes));
        if (p == 6) compile("preset 6, prim_bvh off", scene_desc(pm, pp, no_meshes), PRT_OK, "", false);
    }
    compile("bunny", scene_desc(mats, no_prims, {mesh_of(bunny, 0)}));
    std::vector<PrtPrimitive> many;
    for (int i = 0; i < 40; ++i) {
        const float eu[3] = {7.0f * i, 13.0f * i, 0.0f}, tr[3] = {(float)(i % 8), 0.5f * (float)(i / 8), -1.5f * (float)(i % 5)};
        many.push_back(i % 4 ? make_prim(PRT_SHAPE_CIRCLE, 0.3f, 0.0f, (uint32_t)(i % 7 == 0), 1.0f + 0.1f * i, eu, tr)
                             : make_prim(PRT_SHAPE_QUAD, 1.0f, 2.0f, (uint32_t)(i % 8 == 0), 0.5f, eu, tr));
    }
    if (compile("40 primitives", scene_desc(mats, many, {mesh_of(ico, 0)})).abvh.nodes4.empty()) {
        printf("  ^^^ UNEXPECTED: no primitive BVH\n");
        ++n_compile_fail;
    }
    {
        std::vector<PrtPrimitive> sheared = many;
        sheared[17].mat[4] += 0.25f;  // x += 0.25 y: not rotation + uniform scale
        const PrtHostScene hs = compile("40 primitives, one sheared", scene_desc(mats, sheared, {mesh_of(ico, 0)}));
        if (!hs.abvh.nodes4.empty() || hs.sc.n_prims != 40u) {
            printf("  ^^^ UNEXPECTED: the primitive BVH was kept\n");
            ++n_compile_fail;
        }
    }
    std::vector<PrtInstance> insts;
    for (int k = 0; k < 5; ++k) {
        PrtInstance in{};
        in.mesh = 0;
        in.material_id = (uint32_t)(k & 1);
        const float s = 0.5f + 0.25f * k, sc[3] = {s, s, s}, eu[3] = {10.0f * k, 25.0f * k, 0.0f}, tr[3] = {3.0f * k, 0.5f, -2.0f * k};
        prt_make_transform(sc, eu, tr, in.mat, in.inv);
        insts.push_back(in);
    }
    {
        const PrtHostScene hs = compile("mesh + 5 placed copies", scene_desc(mats, many, {mesh_of(ico, 0)}, {mesh_of(ico, 0)}, insts));
        if (hs.dev_insts.size() != 6u || hs.tlas_inst.size() != 6u || hs.sc.n_tris != 2 * prt_mesh_triangle_count(ico)) {
            printf("  ^^^ UNEXPECTED: instance table\n");
            ++n_compile_fail;
        }
    }
    compile("placed copies only", scene_desc(mats, no_prims, no_meshes, {mesh_of(ico, 0), mesh_of(bunny, 0)}, insts));
    compile("empty", scene_desc({}, no_prims, no_meshes));
    const float tri_p[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, tri_n[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
    const uint32_t tri_i[3] = {0, 1, 2};
    const PrtMesh one{tri_p, tri_n, tri_i, 3, 1, 0};
    compile("one triangle", scene_desc(mats, no_prims, {one}));
    {  // into a scene object that held a bigger scene before: nothing of that survives but the record arrays' storage
        PrtHostScene hs = compile("mesh + 5 placed copies, to be replaced", scene_desc(mats, many, {mesh_of(ico, 0)}, {mesh_of(ico, 0)}, insts));
        const std::vector<PrtMesh> one_mesh = {one};
        const PrtSceneDesc d1 = scene_desc(mats, no_prims, one_mesh);
        std::string e;
        if (prt_compile_scene(&d1, PrtSceneOptions{1.0f / 262144.0f, true, nullptr}, &hs, &e) || hs.tri_records.size() != 12u || hs.nrm_records.size() != 12u ||
            hs.sc.n_tris != 1u || hs.sc.n_insts != 0u || !hs.dev_insts.empty() || !hs.nodes8_all.empty() || !hs.abvh.nodes4.empty() || !hs.prims.empty()) {
            printf("  ^^^ UNEXPECTED: a recompiled scene object kept something of its previous scene\n");
            ++n_compile_fail;
        }
    }
    compile("a mesh without triangles", scene_desc(mats, no_prims, {PrtMesh{nullptr, nullptr, nullptr, 0, 0, 0}}));
    // ---- hostile descriptions: PRT_ERR_INVALID, the message callers see through prt_last_error, no sanitizer report ----
    const int bad = PRT_ERR_INVALID;
    const uint32_t idx_hi[3] = {0, 1, 3}, idx_max[3] = {0xFFFFFFFFu, 1, 2};
    const float inf_p[9] = {0, 0, 0, 1, INFINITY, 0, 0, 1, 0}, nan_p[9] = {0, 0, 0, 1, 0, 0, 0, NAN, 0};
    compile("world mesh: index = n_vertices", scene_desc(mats, no_prims, {one, PrtMesh{tri_p, tri_n, idx_hi, 3, 1, 0}}), bad, "mesh 1: vertex index out of range");
    compile("world mesh: index 2^32 - 1", scene_desc(mats, no_prims, {PrtMesh{tri_p, tri_n, idx_max, 3, 1, 0}}), bad, "mesh 0: vertex index out of range");
    compile("instanced mesh: index out of range", scene_desc(mats, no_prims, no_meshes, {PrtMesh{tri_p, tri_n, idx_hi, 3, 1, 0}}, insts), bad,
            "instanced mesh 0: vertex index out of range");
    compile("world mesh: infinite vertex", scene_desc(mats, no_prims, {PrtMesh{inf_p, tri_n, tri_i, 3, 1, 0}}), bad, "mesh 0: non-finite vertex");
    compile("instanced mesh: NaN vertex", scene_desc(mats, no_prims, no_meshes, {PrtMesh{nan_p, tri_n, tri_i, 3, 1, 0}}, insts), bad,
            "instanced mesh 0: non-finite vertex");
    {
        std::vector<PrtPrimitive> pr = many;
        pr[39].material_id = 2;
        compile("primitive: material out of range", scene_desc(mats, pr, no_meshes), bad, "primitive 39: material out of range");
        pr = many;
        pr[3].shape_type = PRT_SHAPE_TRIANGLE;
        compile("primitive: unknown shape type", scene_desc(mats, pr, no_meshes), bad, "primitive 3: analytic shapes are CIRCLE or QUAD");
        pr[3].shape_type = 0xFFFFFFFFu;
        compile("primitive: shape type 2^32 - 1", scene_desc(mats, pr, no_meshes), bad, "primitive 3: analytic shapes are CIRCLE or QUAD");
    }
    compile("mesh: material out of range", scene_desc(mats, no_prims, {PrtMesh{tri_p, tri_n, tri_i, 3, 1, 0xFFFFFFFFu}}), bad, "mesh 0: material out of range");
    compile("mesh: no materials at all", scene_desc({}, no_prims, {one}), bad, "mesh 0: material out of range");
    compile("mesh: null normals", scene_desc(mats, no_prims, {PrtMesh{tri_p, nullptr, tri_i, 3, 1, 0}}), bad, "mesh 0: positions, normals and indices are required");
    {
        std::vector<PrtInstance> in2 = insts;
        in2[4].material_id = 2;
        compile("instance: material out of range", scene_desc(mats, no_prims, {one}, {mesh_of(ico, 0)}, in2), bad, "instance 4: material out of range");
        in2 = insts;
        in2[2].mesh = 1;
        compile("instance of a missing mesh", scene_desc(mats, no_prims, {one}, {mesh_of(ico, 0)}, in2), bad, "instance 2: mesh out of range");
        compile("instances without any instanced mesh", scene_desc(mats, no_prims, {one}, {}, insts), bad, "instance 0: mesh out of range");
        in2 = insts;
        in2[1].mat[0] *= 2.0f;  // non-uniform scale
        compile("instance: non-uniform scale", scene_desc(mats, no_prims, {one}, {mesh_of(ico, 0)}, in2), bad, "uniform scale");
        in2 = insts;
        in2[3].inv[12] += 1.0f;  // inv is not the inverse of mat
        compile("instance: inv != inverse(mat)", scene_desc(mats, no_prims, {one}, {mesh_of(ico, 0)}, in2), bad, "uniform scale");
        in2 = insts;
        for (float& x : in2[0].mat) x = NAN;
        compile("instance: NaN transform", scene_desc(mats, no_prims, {one}, {mesh_of(ico, 0)}, in2), bad, "uniform scale");
    }
    compile("instanced mesh: zero triangles", scene_desc(mats, no_prims, no_meshes, {PrtMesh{tri_p, tri_n, tri_i, 3, 0, 0}}, insts), bad,
            "instanced mesh 0: positions, normals and indices are required");
    compile("instanced mesh: null arrays", scene_desc(mats, no_prims, no_meshes, {PrtMesh{nullptr, nullptr, nullptr, 3, 1, 0}}, insts), bad,
            "instanced mesh 0: positions, normals and indices are required");
    for (int k = 0; k < 5; ++k) {  // a null array with a non-zero count, each of the five arrays in turn
        PrtSceneDesc d = scene_desc(mats, many, {one}, {mesh_of(ico, 0)}, insts);
        if (k == 0) d.materials = nullptr;
        if (k == 1) d.primitives = nullptr;
        if (k == 2) d.meshes = nullptr;
        if (k == 3) d.instanced_meshes = nullptr;
        if (k == 4) d.instances = nullptr;
        compile(("null array " + std::to_string(k) + " with a non-zero count").c_str(), d, bad, "null array in scene description");
    }
    prt_mesh_free(bunny);
    prt_mesh_free(ico);
    if (n_compile_fail) printf("scene compiler: %d unexpected outcomes\n", n_compile_fail);
    return n_compile_fail ? 1 : 0;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "assets/models";
    const int n_mut = argc > 2 ? atoi(argv[2]) : 3000;
    char err[256];
    const char* names[] = {"icosahedron.ply", "cube_uv.ply", "hand.ply", "bunny.ply", "dragon.ply"};
    for (const char* n : names) {
        PrtMeshData* m = nullptr;
        const int rc = prt_mesh_load_ply((dir + "/" + n).c_str(), &m, err, sizeof(err));
        if (rc) {
            printf("%s: load failed: %s\n", n, err);
            return 1;
        }
        printf("%s: %u vertices, %u triangles, normals in file: %d\n", n, prt_mesh_vertex_count(m), prt_mesh_triangle_count(m), prt_mesh_had_normals(m));
        std::vector<float> verts;
        flatten(m, verts);
        build(verts, "as loaded");
        const uint32_t target = prt_mesh_triangle_count(m) * 3 + 17;
        if (prt_mesh_refine(m, target) == 0) {
            flatten(m, verts);
            build(verts, "refined x3");
        } else {
            printf("  refine refused (non-manifold)\n");
        }
        float mat[16], inv[16];
        const float sc[3] = {1.5f, 1.5f, 1.5f}, eu[3] = {30.f, 40.f, 50.f}, tr[3] = {1.f, 2.f, 3.f};
        prt_make_transform(sc, eu, tr, mat, inv);
        prt_mesh_transform(m, mat, inv);
        PrtMeshData* m2 = nullptr;
        prt_mesh_create(prt_mesh_positions(m), prt_mesh_normals(m), prt_mesh_vertex_count(m), prt_mesh_indices(m), prt_mesh_triangle_count(m), &m2);
        prt_mesh_append(m, m2);
        prt_mesh_free(m2);
        prt_mesh_free(m);
    }
    // degenerate inputs of the builder
    {
        std::vector<float> v;
        build(v, "no triangle");
        v.assign(9, 0.0f);
        build(v, "one zero-area triangle");
        v.assign(9 * 1000, 1.0f);
        build(v, "1000 identical points");
        v.resize(9 * 5000);
        std::mt19937 g(1);
        std::uniform_real_distribution<float> u(-1.f, 1.f);
        for (auto& x : v) x = u(g);
        build(v, "5000 random big triangles");
        for (size_t i = 0; i < v.size(); ++i) v[i] = (i % 9 < 3) ? u(g) * 1e-3f : v[i - (i % 9) + (i % 3)];
        build(v, "5000 collapsed triangles");
        for (auto& x : v) x = u(g) * 1e30f;
        build(v, "huge coordinates");
    }
    // presets + image writers
    for (int p = 0; p < 8; ++p) {
        std::vector<PrtMaterial> mats(2048);
        std::vector<PrtPrimitive> prims(2048);
        uint32_t nm = (uint32_t)mats.size(), np = (uint32_t)prims.size();
        const int rc = prt_scene_preset(p, mats.data(), &nm, prims.data(), &np);
        printf("preset %d: rc %d, %u materials, %u primitives\n", p, rc, nm, np);
    }
    {
        std::vector<uint8_t> img(4 * 33 * 17, 128);
        std::vector<float> f(3 * 33 * 17, 0.5f);
        prt_write_ppm("/tmp/sanitize_host.ppm", img.data(), 33, 17);
        prt_write_pfm("/tmp/sanitize_host.pfm", f.data(), 33, 17);
        prt_write_ppm("/nonexistent_dir/x.ppm", img.data(), 33, 17);
    }
    if (scene_compiler_cases(dir)) return 1;
    // mutation fuzz of the PLY parser
    std::mt19937 g(7);
    std::vector<std::string> src = {slurp(dir + "/icosahedron.ply"), slurp(dir + "/cube_uv.ply")};
    {  // a binary variant of the icosahedron
        PrtMeshData* m = nullptr;
        prt_mesh_load_ply((dir + "/icosahedron.ply").c_str(), &m, err, sizeof(err));
        std::string b = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(prt_mesh_vertex_count(m)) +
                        "\nproperty float x\nproperty float y\nproperty float z\nelement face " + std::to_string(prt_mesh_triangle_count(m)) +
                        "\nproperty list uchar int vertex_indices\nend_header\n";
        b.append((const char*)prt_mesh_positions(m), 12 * (size_t)prt_mesh_vertex_count(m));
        for (uint32_t t = 0; t < prt_mesh_triangle_count(m); ++t) {
            b.push_back(3);
            b.append((const char*)(prt_mesh_indices(m) + 3 * (size_t)t), 12);
        }
        src.push_back(b);
        prt_mesh_free(m);
    }
    int ok = 0, bad = 0;
    for (int it = 0; it < n_mut; ++it) {
        std::string b = src[g() % src.size()];
        const int kind = g() % 5;
        if (kind == 0)
            for (int k = 0, n = 1 + g() % 8; k < n; ++k) b[g() % b.size()] = (char)(g() & 255);
        else if (kind == 1)
            b.resize(g() % b.size());
        else if (kind == 2) {
            const size_t h = b.find("end_header");
            std::vector<size_t> digits;
            for (size_t i = 0; i < h && i < b.size(); ++i)
                if (b[i] >= '0' && b[i] <= '9' && (i == 0 || b[i - 1] < '0' || b[i - 1] > '9')) digits.push_back(i);
            if (!digits.empty()) {
                const size_t p = digits[g() % digits.size()];
                size_t e = p;
                while (e < b.size() && b[e] >= '0' && b[e] <= '9') ++e;
                const char* reps[] = {"0", "-1", "4294967295", "99999999999999999999", "1e9", "7"};
                b.replace(p, e - p, reps[g() % 6]);
            }
        } else if (kind == 3) {
            std::string ins;
            for (int k = 0, n = 1 + g() % 64; k < n; ++k) ins.push_back((char)(g() & 255));
            b.insert(g() % b.size(), ins);
        } else {
            const size_t p = g() % b.size();
            b.erase(p, 1 + g() % 200);
        }
        {
            std::ofstream f("/tmp/sanitize_host_mut.ply", std::ios::binary);
            f.write(b.data(), (std::streamsize)b.size());
        }
        PrtMeshData* m = nullptr;
        if (prt_mesh_load_ply("/tmp/sanitize_host_mut.ply", &m, err, sizeof(err)) == 0) {
            ++ok;
            std::vector<float> verts;
            flatten(m, verts);
            BvhBuild bb;
            bool finite = true;
            for (float x : verts) finite = finite && std::isfinite(x);
            if (finite) bvh_build(verts.data(), (uint32_t)(verts.size() / 9), 3, 1, 63, &bb);
            prt_mesh_free(m);
        } else {
            ++bad;
        }
    }
    printf("PLY mutations: %d loaded, %d refused, no sanitizer report\n", ok, bad);
    return 0;
}

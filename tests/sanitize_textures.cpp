// sanitize_textures.cpp — the host half of image textures (prt_scene.cpp prt_build_textures: validation, the face-order UV
// table, the texel pool; prt_host.cpp: UVs through PLY ingest, refine and append) under AddressSanitizer + UBSan on the CPU.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I parallelraytracing_amd/csrc \
//       tests/sanitize_textures.cpp parallelraytracing_amd/csrc/prt_host.cpp parallelraytracing_amd/csrc/bvh.cpp \
//       parallelraytracing_amd/csrc/prt_scene.cpp -pthread -o /tmp/sanitize_textures
//   /tmp/sanitize_textures assets/models [n_sets]
// The scene: a world bunny (planar UVs) and a world cube, 6 placed copies of cube_uv and of the icosahedron (no UVs), three
// analytic primitives (two quads, a sphere).  n random texture sets: sizes 1 .. 40 a side, every filter and wrap, random
// material bindings; each is made invalid in one random way half of the time.  A valid set must build tables whose every
// entry is checked against the description; an invalid one must be refused with PRT_ERR_INVALID and leave the output
// untouched.  Then UV-carrying PLY files, mutated byte by byte, go through the reader, refine and append.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
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

static bool same_tables(const PrtTexTables& a, const PrtTexTables& b) {
    return a.is_set == b.is_set && a.n_textures == b.n_textures && a.n_textured_materials == b.n_textured_materials && a.texels == b.texels &&
           a.desc == b.desc && a.mat_tex == b.mat_tex && a.uvs == b.uvs && a.inst_uv_base == b.inst_uv_base;
}

static int run_sets(const std::string& dir, int n_sets) {
    char err[256];
    PrtMeshData *bunny = nullptr, *ico = nullptr, *cube = nullptr, *wcube = nullptr;
    if (prt_mesh_load_ply((dir + "/bunny.ply").c_str(), &bunny, err, sizeof(err)) || prt_mesh_load_ply((dir + "/icosahedron.ply").c_str(), &ico, err, sizeof(err)) ||
        prt_mesh_load_ply((dir + "/cube_uv.ply").c_str(), &cube, err, sizeof(err)) || prt_mesh_load_ply((dir + "/cube_uv.ply").c_str(), &wcube, err, sizeof(err))) {
        printf("load failed: %s\n", err);
        return 1;
    }
    std::mt19937 rng(11u);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    {  // planar UVs on the bunny
        std::vector<float> uv(2 * (size_t)prt_mesh_vertex_count(bunny));
        for (size_t v = 0; v < uv.size() / 2; ++v) {
            uv[2 * v] = prt_mesh_positions(bunny)[3 * v] * 3.0f;
            uv[2 * v + 1] = prt_mesh_positions(bunny)[3 * v + 1] * 3.0f;
        }
        prt_mesh_set_uvs(bunny, uv.data());
    }
    // materials: 0 Lambertian (ground), 1 emissive, 2 Lambertian (bunny), 3 metal (cubes), 4 dielectric (sphere), 5 Lambertian (icosahedra)
    const std::vector<PrtMaterial> mats = {{PRT_MAT_LAMBERTIAN, {0.5f, 0.5f, 0.5f}, 0.0f}, {PRT_MAT_EMISSIVE, {6.0f, 5.0f, 4.0f}, 0.0f},
                                           {PRT_MAT_LAMBERTIAN, {0.8f, 0.7f, 0.6f}, 0.0f}, {PRT_MAT_METAL, {0.9f, 0.9f, 0.9f}, 0.05f},
                                           {PRT_MAT_DIELECTRIC, {0, 0, 0}, 1.5f},         {PRT_MAT_LAMBERTIAN, {0.3f, 0.4f, 0.5f}, 0.0f}};
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
    prims[2].shape_type = PRT_SHAPE_CIRCLE, prims[2].shape_param[0] = 0.8f, prims[2].material_id = 4;
    prt_make_transform(one, zero, t2, prims[2].mat, prims[2].inv);
    const std::vector<PrtMesh> meshes = {mesh_of(bunny, 2), mesh_of(wcube, 3)};
    const std::vector<PrtMesh> imeshes = {mesh_of(ico, 0), mesh_of(cube, 0)};
    std::vector<PrtInstance> insts(6);
    for (size_t k = 0; k < insts.size(); ++k) {
        insts[k] = PrtInstance{};
        insts[k].mesh = (uint32_t)(k & 1);
        insts[k].material_id = (k & 1) ? 3u : 5u;  // cubes metal, icosahedra Lambertian
        const float s = 0.3f + u01(rng), sc[3] = {s, s, s};
        const float eu[3] = {360.0f * u01(rng), 360.0f * u01(rng), 0.0f}, tr[3] = {6 * u01(rng) - 3, 2 * u01(rng), 6 * u01(rng) - 3};
        prt_make_transform(sc, eu, tr, insts[k].mat, insts[k].inv);
    }
    PrtSceneDesc d{};
    d.materials = mats.data(), d.n_materials = (uint32_t)mats.size();
    d.primitives = prims.data(), d.n_primitives = (uint32_t)prims.size();
    d.meshes = meshes.data(), d.n_meshes = (uint32_t)meshes.size();
    d.instanced_meshes = imeshes.data(), d.n_instanced_meshes = (uint32_t)imeshes.size();
    d.instances = insts.data(), d.n_instances = (uint32_t)insts.size();
    PrtHostScene hs;
    std::string e;
    if (prt_compile_scene(&d, kOpt, &hs, &e)) {
        printf("compile failed: %s\n", e.c_str());
        return 1;
    }
    const uint32_t n_world = prt_mesh_triangle_count(bunny) + prt_mesh_triangle_count(wcube);
    const uint32_t n_uv_tris = n_world + prt_mesh_triangle_count(ico) + prt_mesh_triangle_count(cube);
    int n_valid = 0, n_refused = 0;
    PrtTexTables kept;  // the last accepted binding: a refusal must leave it alone
    for (int it = 0; it < n_sets; ++it) {
        const uint32_t nt = 1u + (uint32_t)(u01(rng) * 4.0f);
        std::vector<std::vector<float>> img(nt);
        std::vector<PrtTexture> tex(nt);
        for (uint32_t k = 0; k < nt; ++k) {
            const uint32_t w = 1u + (uint32_t)(u01(rng) * 40.0f), h = 1u + (uint32_t)(u01(rng) * 40.0f);
            img[k].resize((size_t)w * h * 3);
            for (float& x : img[k]) x = u01(rng);
            tex[k] = PrtTexture{img[k].data(), w, h, (uint32_t)(u01(rng) * 2.0f), (uint32_t)(u01(rng) * 2.0f)};
        }
        // bindings: ground, bunny, metal cubes may be textured; the icosahedra (no UVs), the emitter and the glass never
        std::vector<uint32_t> mt(mats.size(), PRT_TEXTURE_NONE);
        for (uint32_t m : {0u, 2u, 3u})
            if (u01(rng) < 0.7f) mt[m] = (uint32_t)(u01(rng) * (float)nt) % nt;
        std::vector<float> buv(prt_mesh_uvs(bunny), prt_mesh_uvs(bunny) + 2 * (size_t)prt_mesh_vertex_count(bunny));
        std::vector<const float*> muv = {buv.data(), prt_mesh_uvs(wcube)};
        std::vector<const float*> iuv = {nullptr, prt_mesh_uvs(cube)};
        PrtTextureSet set{tex.data(), nt, mt.data(), (uint32_t)mt.size(), muv.data(), (uint32_t)muv.size(), iuv.data(), (uint32_t)iuv.size()};
        const char* broke = nullptr;
        if (u01(rng) < 0.5f) {
            switch ((int)(u01(rng) * 14.0f)) {
                case 0: set.n_materials += 1; broke = "n_materials"; break;
                case 1: set.n_meshes -= 1; broke = "n_meshes"; break;
                case 2: set.n_instanced_meshes += 3; broke = "n_instanced_meshes"; break;
                case 3: mt[0] = nt; broke = "texture index"; break;
                case 4: tex[0].width = 0; broke = "zero width"; break;
                case 5: tex[nt - 1].height = PRT_TEX_MAX_SIZE + 1u; broke = "height above the limit"; break;
                case 6: tex[nt / 2].rgb = nullptr; broke = "null image"; break;
                case 7: img[0][img[0].size() - 1] = -0.25f; broke = "negative texel"; break;
                case 8: img[nt - 1][0] = NAN; broke = "NaN texel"; break;
                case 9: tex[0].filter = 2; broke = "filter"; break;
                case 10: tex[0].wrap = 7; broke = "wrap"; break;
                case 11: buv[buv.size() - 1] = INFINITY; broke = "infinite UV"; break;
                case 12: mt[1] = 0; broke = "textured emitter"; break;
                default: mt[5] = 0; broke = "textured copies without UVs"; break;
            }
        }
        PrtTexTables out = kept;
        std::string er;
        const int rc = prt_build_textures(hs, &set, &out, &er);
        if (broke) {
            const bool ok = rc == PRT_ERR_INVALID && !er.empty() && same_tables(out, kept);
            if (!ok) printf("  set %d (%s): ^^^ UNEXPECTED rc %d: %s\n", it, broke, rc, er.c_str());
            n_fail += !ok;
            ++n_refused;
            continue;
        }
        if (rc) {
            printf("  set %d: ^^^ UNEXPECTED refusal (%d): %s\n", it, rc, er.c_str());
            ++n_fail;
            continue;
        }
        ++n_valid;
        // the tables against the description
        size_t texels = 0;
        bool ok = out.is_set && out.n_textures == nt && out.desc.size() == 4u * nt && out.mat_tex == mt && out.uvs.size() == 6u * (size_t)n_uv_tris &&
                  out.inst_uv_base.size() == hs.dev_insts.size();
        for (uint32_t k = 0; ok && k < nt; ++k) {
            ok = out.desc[4 * k] == texels && out.desc[4 * k + 1] == tex[k].width && out.desc[4 * k + 2] == tex[k].height &&
                 out.desc[4 * k + 3] == (tex[k].filter | (tex[k].wrap << 1));
            const size_t n = (size_t)tex[k].width * tex[k].height;
            for (size_t i = 0; ok && i < n; ++i)
                ok = out.texels[4 * (texels + i)] == img[k][3 * i] && out.texels[4 * (texels + i) + 1] == img[k][3 * i + 1] &&
                     out.texels[4 * (texels + i) + 2] == img[k][3 * i + 2] && out.texels[4 * (texels + i) + 3] == 0.0f;
            texels += n;
        }
        ok = ok && out.texels.size() == 4 * texels;
        // every face's three UVs, reached the way the kernels reach them
        const uint32_t* bidx = prt_mesh_indices(bunny);
        for (uint32_t f = 0; ok && f < prt_mesh_triangle_count(bunny); ++f)
            for (int v = 0; v < 3; ++v)
                ok = ok && out.uvs[6 * (size_t)f + 2 * v] == buv[2 * (size_t)bidx[3 * f + v]] && out.uvs[6 * (size_t)f + 2 * v + 1] == buv[2 * (size_t)bidx[3 * f + v] + 1];
        for (size_t i = 0; ok && i < hs.dev_insts.size(); ++i) {
            const DevInstance& I = hs.dev_insts[i];
            const bool world = i < hs.n_world_insts;
            const PrtMeshData* m = world ? wcube : (hs.inst_mesh[i - hs.n_world_insts] ? cube : ico);
            // the first face of the mesh (world: the cube's first face sits behind the bunny's, and its record carries the global index)
            const uint32_t carried = world ? hs.sc.n_prims + prt_mesh_triangle_count(bunny) : 0u;
            const uint32_t entry = out.inst_uv_base[i] + carried;
            ok = entry < n_uv_tris && I.n_tris > 0;
            const float* uv = prt_mesh_uvs(m);
            for (int v = 0; ok && v < 3; ++v) {
                const uint32_t vi = prt_mesh_indices(m)[v];
                ok = out.uvs[6 * (size_t)entry + 2 * v] == (uv ? uv[2 * vi] : 0.0f) && out.uvs[6 * (size_t)entry + 2 * v + 1] == (uv ? uv[2 * vi + 1] : 0.0f);
            }
        }
        expect(ok, "the tables of a valid set do not match the description");
        kept = out;
    }
    // NULL set, and a scene without placed copies (instanced meshes declared but unused: their UVs are not read)
    {
        PrtTexTables out = kept;
        std::string er;
        expect(prt_build_textures(hs, nullptr, &out, &er) == PRT_ERR_INVALID && same_tables(out, kept), "a null set was not refused cleanly");
        PrtSceneDesc d0 = d;
        d0.n_instances = 0;
        PrtHostScene plain;
        expect(prt_compile_scene(&d0, kOpt, &plain, &er) == PRT_OK, "the scene without placed copies compiles");
        std::vector<float> one_texel = {0.5f, 0.25f, 1.0f};
        PrtTexture t{one_texel.data(), 1, 1, PRT_TEX_BILINEAR, PRT_TEX_CLAMP};
        std::vector<uint32_t> mt(mats.size(), PRT_TEXTURE_NONE);
        mt[2] = 0;
        std::vector<const float*> muv = {prt_mesh_uvs(bunny), nullptr};
        const float* bogus = reinterpret_cast<const float*>(uintptr_t(16));  // must never be dereferenced
        std::vector<const float*> iuv = {bogus, bogus};
        PrtTextureSet set{&t, 1, mt.data(), (uint32_t)mt.size(), muv.data(), 2, iuv.data(), 2};
        expect(prt_build_textures(plain, &set, &out, &er) == PRT_OK && out.uvs.size() == 6u * (size_t)n_world && out.inst_uv_base.empty(),
               "a scene without placed copies");
        mt[3] = 0;  // the world cube's material, and its UVs are missing
        expect(prt_build_textures(plain, &set, &out, &er) == PRT_ERR_INVALID, "a textured world mesh without UVs was accepted");
        mt[3] = PRT_TEXTURE_NONE;
        mt[4] = 0;
        expect(prt_build_textures(plain, &set, &out, &er) == PRT_ERR_INVALID, "a textured dielectric was accepted");
    }
    printf("  %d texture sets: %d valid, %d refused; %u UV triangles\n", n_sets, n_valid, n_refused, n_uv_tris);
    prt_mesh_free(bunny);
    prt_mesh_free(ico);
    prt_mesh_free(cube);
    prt_mesh_free(wcube);
    return 0;
}

// UV-carrying PLY files with mutated bytes through the reader, refine and append: any outcome is fine except a report
static int run_ply(const std::string& dir, const std::string& tmp, int n_files) {
    std::ifstream f(dir + "/cube_uv.ply", std::ios::binary);
    const std::string good((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (good.empty()) {
        printf("cannot read cube_uv.ply\n");
        return 1;
    }
    // a binary variant with double / uchar UVs under the other spellings
    std::string bin = "ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                      "property double texture_u\nproperty uchar texture_v\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n";
    const float P[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
    for (int v = 0; v < 4; ++v) {
        bin.append((const char*)P[v], 12);
        const double u = 0.25 * v;
        bin.append((const char*)&u, 8);
        bin.push_back((char)(v * 60));
    }
    const int32_t F[2][3] = {{0, 1, 2}, {0, 2, 3}};
    for (int t = 0; t < 2; ++t) {
        bin.push_back(3);
        bin.append((const char*)F[t], 12);
    }
    std::mt19937 rng(5u);
    int loaded = 0, with_uv = 0;
    const std::string path = tmp + "/mutated.ply";
    for (int it = 0; it < n_files; ++it) {
        std::string s = (it & 1) ? bin : good;
        const int n_mut = it < 2 ? 0 : 1 + (int)(rng() % 4u);
        for (int k = 0; k < n_mut; ++k) {
            const size_t at = rng() % s.size();
            switch (rng() % 4u) {
                case 0: s[at] = (char)(rng() & 0xFF); break;
                case 1: s.erase(at, 1 + rng() % 8u); break;
                case 2: s.insert(at, 1 + rng() % 4u, (char)('0' + rng() % 10u)); break;
                default: s.resize(at); break;
            }
            if (s.empty()) s = "ply\n";
        }
        {
            std::ofstream o(path, std::ios::binary);
            o.write(s.data(), (std::streamsize)s.size());
        }
        PrtMeshData* m = nullptr;
        char err[256];
        if (prt_mesh_load_ply(path.c_str(), &m, err, sizeof(err)) != PRT_OK) continue;
        ++loaded;
        const uint32_t nv = prt_mesh_vertex_count(m);
        if (prt_mesh_had_uvs(m)) {
            ++with_uv;
            float sum = 0.0f;
            for (uint32_t v = 0; v < 2 * nv; ++v) sum += prt_mesh_uvs(m)[v];  // every UV is readable
            (void)sum;
        }
        if (it < 2) expect(prt_mesh_had_uvs(m) == 1, "the unmutated files carry UVs");
        if (prt_mesh_triangle_count(m) && prt_mesh_triangle_count(m) < 64u) (void)prt_mesh_refine(m, 200);
        if (prt_mesh_had_uvs(m)) expect(prt_mesh_uvs(m) != nullptr, "UVs after refine");
        PrtMeshData* other = nullptr;
        if (prt_mesh_load_ply((dir + "/icosahedron.ply").c_str(), &other, err, sizeof(err)) == PRT_OK) {
            const int had = prt_mesh_had_uvs(m);
            expect(prt_mesh_append(other, m) == PRT_OK && prt_mesh_had_uvs(other) == 0, "append onto a mesh without UVs");
            expect(prt_mesh_append(m, m) == PRT_OK, "self append");
            expect(prt_mesh_had_uvs(m) == had || prt_mesh_vertex_count(m) == 0u, "UVs survive an append of a mesh that has them");
            prt_mesh_free(other);
        }
        prt_mesh_free(m);
    }
    printf("  %d mutated PLY files: %d loaded, %d of them with UVs\n", n_files, loaded, with_uv);
    expect(loaded >= 2 && with_uv >= 2, "the unmutated files load");
    return 0;
}

// Files with two `vertex` elements, each with or without UVs and of its own count: the last one stands, and the mesh that
// comes out has two UV floats per vertex or none (what every reader of prt_mesh_uvs relies on)
static int run_two_vertex_elements(const std::string& tmp) {
    const std::string path = tmp + "/two_vertex_elements.ply";
    const int counts[3] = {1, 3, 5};
    int n = 0;
    for (int uv1 = 0; uv1 < 2; ++uv1)
        for (int uv2 = 0; uv2 < 2; ++uv2)
            for (int c1 : counts)
                for (int c2 : counts) {
                    std::string s = "ply\nformat ascii 1.0\n";
                    const int uv[2] = {uv1, uv2}, cnt[2] = {c1, c2};
                    for (int e = 0; e < 2; ++e) {
                        s += "element vertex " + std::to_string(cnt[e]) + "\nproperty float x\nproperty float y\nproperty float z\n";
                        if (uv[e]) s += "property float s\nproperty float t\n";
                    }
                    s += "element face 1\nproperty list uchar uint vertex_indices\nend_header\n";
                    for (int e = 0; e < 2; ++e)
                        for (int v = 0; v < cnt[e]; ++v) {
                            s += std::to_string(v) + " " + std::to_string(v % 2) + " " + std::to_string(v / 2);
                            if (uv[e]) s += " 0." + std::to_string(v) + " 0.5";
                            s += "\n";
                        }
                    s += c2 >= 3 ? "3 0 1 2\n" : "3 0 0 0\n";
                    {
                        std::ofstream o(path, std::ios::binary);
                        o.write(s.data(), (std::streamsize)s.size());
                    }
                    PrtMeshData* m = nullptr;
                    char err[256];
                    expect(prt_mesh_load_ply(path.c_str(), &m, err, sizeof(err)) == PRT_OK, "a file with two vertex elements loads");
                    if (!m) continue;
                    ++n;
                    expect(prt_mesh_vertex_count(m) == (uint32_t)c2, "the last vertex element's count stands");
                    expect(prt_mesh_had_uvs(m) == uv2 && (prt_mesh_uvs(m) != nullptr) == (uv2 != 0), "UVs are the last vertex element's, or none");
                    float sum = 0.0f;
                    for (uint32_t v = 0; prt_mesh_had_uvs(m) && v < 2 * prt_mesh_vertex_count(m); ++v) sum += prt_mesh_uvs(m)[v];
                    (void)sum;
                    if (c2 >= 3) (void)prt_mesh_refine(m, 20);
                    expect(prt_mesh_append(m, m) == PRT_OK && prt_mesh_had_uvs(m) == uv2, "self append keeps the rule");
                    for (uint32_t v = 0; prt_mesh_had_uvs(m) && v < 2 * prt_mesh_vertex_count(m); ++v) sum += prt_mesh_uvs(m)[v];
                    prt_mesh_free(m);
                }
    printf("  %d files with two vertex elements\n", n);
    return 0;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "assets/models";
    const int n_sets = argc > 2 ? atoi(argv[2]) : 300;
    const std::string tmp = argc > 3 ? argv[3] : "/tmp";
    if (run_sets(dir, n_sets) || run_ply(dir, tmp, 400) || run_two_vertex_elements(tmp)) return 1;
    if (n_fail) {
        printf("%d unexpected results\n", n_fail);
        return 1;
    }
    printf("no sanitizer report\n");
    return 0;
}

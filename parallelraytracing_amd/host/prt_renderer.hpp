// prt_renderer.hpp — C++ host-side mirror of the reference's Scene / Camera / Film / Renderer interfaces over
// the C-ABI of include/prt.h (header-only).  Same method names and call contract as the reference:
//   class Renderer { Init(Film&, const Scene&, const Camera&); ProgressiveRender(); SetCamera(const Camera&); }
//   (reference: src/core/renderer.h:8-16)
// Nothing here computes pixels; the bodies only marshal PODs into prt_* calls.  INTEGRATION.md shows the same
// adapter written against the reference's own headers.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/prt.h"

namespace prt {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// Scene(preset) (reference: src/core/scene.h:17-62); materials/primitives flattened as PrtSceneDesc wants them.
class Scene {
public:
    explicit Scene(int preset = PRT_PRESET_RANDOM_BALLS_LARGE) {  // default preset: src/core/scene.h:20
        uint32_t nm = 0, np = 0;
        if (prt_scene_preset(preset, nullptr, &nm, nullptr, &np)) throw Error("unknown scene preset");
        materials.resize(nm);
        primitives.resize(np);
        prt_scene_preset(preset, materials.data(), &nm, primitives.data(), &np);
    }
    struct Empty {};
    explicit Scene(Empty) {}
    ~Scene() {
        for (PrtMeshData* m : owned_) prt_mesh_free(m);
    }
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;

    uint32_t AddMaterial(uint32_t type, float r, float g, float b, float scalar) {
        materials.push_back(PrtMaterial{type, {r, g, b}, scalar});
        return (uint32_t)materials.size() - 1;
    }
    void AddPrimitive(uint32_t shape, float p0, float p1, uint32_t material, const float scale[3], const float euler_deg[3],
                      const float translation[3]) {  // Scene::AddPrimitive + MakeTransform, src/core/scene.cpp:9-36
        PrtPrimitive p{};
        p.shape_type = shape;
        p.shape_param[0] = p0;
        p.shape_param[1] = p1;
        p.material_id = material;
        prt_make_transform(scale, euler_deg, translation, p.mat, p.inv);
        primitives.push_back(p);
    }
    // Mesh(plyFilePath) (reference: src/core/mesh.h:8-21), appended as world-space triangles
    void AddMeshPly(const std::string& path, uint32_t material, uint32_t refine_to = 0) {
        PrtMeshData* m = nullptr;
        char err[256] = {0};
        if (prt_mesh_load_ply(path.c_str(), &m, err, sizeof(err))) throw Error(std::string("PLY: ") + err);
        if (refine_to > prt_mesh_triangle_count(m) && prt_mesh_refine(m, refine_to)) {
            prt_mesh_free(m);
            throw Error("mesh refinement failed (non-manifold edge)");
        }
        owned_.push_back(m);
        meshes.push_back(PrtMesh{prt_mesh_positions(m), prt_mesh_normals(m), prt_mesh_indices(m), prt_mesh_vertex_count(m),
                                 prt_mesh_triangle_count(m), material});
        mesh_uvs.push_back(prt_mesh_uvs(m));  // the file's s/t (u/v, texture_u/texture_v), or null
    }
    // A mesh that is placed, not flattened (PrtInstance): returns its index for AddInstance
    uint32_t AddInstancedMeshPly(const std::string& path) {
        PrtMeshData* m = nullptr;
        char err[256] = {0};
        if (prt_mesh_load_ply(path.c_str(), &m, err, sizeof(err))) throw Error(std::string("PLY: ") + err);
        owned_.push_back(m);
        instanced_meshes.push_back(PrtMesh{prt_mesh_positions(m), prt_mesh_normals(m), prt_mesh_indices(m), prt_mesh_vertex_count(m),
                                           prt_mesh_triangle_count(m), 0u});
        instanced_mesh_uvs.push_back(prt_mesh_uvs(m));
        return (uint32_t)instanced_meshes.size() - 1;
    }
    // Image textures (include/prt.h "Image textures"): rgb = height * width * 3 floats, row 0 = top, copied
    uint32_t AddTexture(const float* rgb, uint32_t width, uint32_t height, uint32_t filter = PRT_TEX_NEAREST, uint32_t wrap = PRT_TEX_REPEAT) {
        texels_.emplace_back(rgb, rgb + (size_t)width * height * 3);
        tex_meta_.push_back(PrtTexture{nullptr, width, height, filter, wrap});
        return (uint32_t)tex_meta_.size() - 1;
    }
    // ... from a colour PFM file (prt_read_pfm)
    uint32_t AddTexturePfm(const std::string& path, uint32_t filter = PRT_TEX_NEAREST, uint32_t wrap = PRT_TEX_REPEAT) {
        float* rgb = nullptr;
        uint32_t w = 0, h = 0;
        if (prt_read_pfm(path.c_str(), &rgb, &w, &h)) throw Error("cannot read " + path + " as a colour PFM");
        const uint32_t t = AddTexture(rgb, w, h, filter, wrap);
        prt_image_free(rgb);
        return t;
    }
    // the albedo of a Lambertian / Metal material comes from `texture` (PRT_TEXTURE_NONE: its rgb again)
    void SetMaterialTexture(uint32_t material, uint32_t texture) {
        if (material_texture.size() < materials.size()) material_texture.resize(materials.size(), PRT_TEXTURE_NONE);
        material_texture.at(material) = texture;
    }
    bool HasTextures() const { return !tex_meta_.empty(); }
    bool MeshHasUVs(uint32_t mesh) const { return mesh_uvs.at(mesh) != nullptr; }
    // valid while the scene lives and is not changed (the arrays it points into are caches of this scene: the scene's own
    // description is not touched).  mesh_uvs / instanced_mesh_uvs hold one entry per mesh: a scene whose mesh vectors were
    // filled by hand keeps them in step, or is refused here
    PrtTextureSet textureSet() const {
        if (mesh_uvs.size() != meshes.size() || instanced_mesh_uvs.size() != instanced_meshes.size())
            throw Error("Scene: mesh_uvs / instanced_mesh_uvs need one entry (or null) per mesh");
        if (material_texture.size() > materials.size()) throw Error("Scene: material_texture is longer than materials");
        set_material_texture_ = material_texture;
        set_material_texture_.resize(materials.size(), PRT_TEXTURE_NONE);
        set_textures_ = tex_meta_;
        for (size_t k = 0; k < set_textures_.size(); ++k) set_textures_[k].rgb = texels_[k].data();
        PrtTextureSet t{};
        t.textures = set_textures_.data();
        t.n_textures = (uint32_t)set_textures_.size();
        t.material_texture = set_material_texture_.data();
        t.n_materials = (uint32_t)materials.size();
        t.mesh_uvs = mesh_uvs.data();
        t.n_meshes = (uint32_t)meshes.size();
        t.instanced_mesh_uvs = instanced_mesh_uvs.data();
        t.n_instanced_meshes = (uint32_t)instanced_meshes.size();
        return t;
    }
    // A placed copy (uniform scale only); SetInstanceTransform moves it, HipWavefrontRenderer::UpdateInstances follows
    uint32_t AddInstance(uint32_t mesh, uint32_t material, float scale, const float euler_deg[3], const float translation[3]) {
        PrtInstance in{};
        in.mesh = mesh;
        in.material_id = material;
        instances.push_back(in);
        SetInstanceTransform((uint32_t)instances.size() - 1, scale, euler_deg, translation);
        return (uint32_t)instances.size() - 1;
    }
    void SetInstanceTransform(uint32_t i, float scale, const float euler_deg[3], const float translation[3]) {
        const float sc[3] = {scale, scale, scale};
        prt_make_transform(sc, euler_deg, translation, instances.at(i).mat, instances.at(i).inv);
    }
    PrtSceneDesc desc() const {
        PrtSceneDesc d{};
        d.materials = materials.data();
        d.primitives = primitives.data();
        d.meshes = meshes.data();
        d.n_materials = (uint32_t)materials.size();
        d.n_primitives = (uint32_t)primitives.size();
        d.n_meshes = (uint32_t)meshes.size();
        d.sky[0] = sky[0];
        d.sky[1] = sky[1];
        d.sky[2] = sky[2];
        d.instanced_meshes = instanced_meshes.data();
        d.instances = instances.data();
        d.n_instanced_meshes = (uint32_t)instanced_meshes.size();
        d.n_instances = (uint32_t)instances.size();
        return d;
    }
    std::vector<PrtMaterial> materials;
    std::vector<PrtPrimitive> primitives;
    std::vector<PrtMesh> meshes;
    std::vector<PrtMesh> instanced_meshes;
    std::vector<PrtInstance> instances;
    std::vector<const float*> mesh_uvs, instanced_mesh_uvs;  // per mesh: its per-vertex UVs, or null
    std::vector<uint32_t> material_texture;                  // per material (shorter: the rest has none)
    float sky[3] = {0.4f, 0.3f, 0.6f};  // src/backend/cpu/renderer.h:31

private:
    std::vector<PrtMeshData*> owned_;
    std::vector<std::vector<float>> texels_;
    std::vector<PrtTexture> tex_meta_;
    mutable std::vector<PrtTexture> set_textures_;  // what the last textureSet() points into
    mutable std::vector<uint32_t> set_material_texture_;
};

// Camera(position, front, width, height) (reference: src/core/camera.h:10-16)
struct Camera {
    float position[3] = {5.0f, 5.0f, 8.0f};  // src/main.cpp:142
    float front[3] = {-5.0f, -5.0f, -8.0f};
    float width = 1920.0f, height = 1080.0f;
    PrtCameraDesc desc() const {
        PrtCameraDesc d{};
        for (int k = 0; k < 3; ++k) {
            d.position[k] = position[k];
            d.front[k] = front[k];
        }
        d.width = width;
        d.height = height;
        return d;
    }
};

// Film(width, height) (reference: src/core/film.h:10-76): host copies of the accumulation buffers.
class Film {
public:
    Film(uint32_t w, uint32_t h) : width(w), height(h), accum((size_t)w * h * 3), weights((size_t)w * h), display((size_t)w * h * 4) {}
    uint32_t GetWidth() const { return width; }
    uint32_t GetHeight() const { return height; }
    uint32_t width, height;
    std::vector<float> accum, weights;
    std::vector<uint8_t> display;
};

class Renderer {
public:
    virtual ~Renderer() = default;
    virtual void Init(Film& film, const Scene& scene, const Camera& camera) = 0;
    virtual void ProgressiveRender() = 0;
    virtual void SetCamera(const Camera& camera) = 0;
};

// One renderer, one or several GPUs of a node.  devices = {0} is the single-GPU backend; devices = {0, 1, ..., 7} tiles the
// image over eight GPUs (8x8-pixel tiles dealt round-robin, scene replicated, RNG keyed by global pixel and sample, so the
// image does not depend on the device count) and gathers the per-tile radiance to devices[0] once per Render call: RCCL
// (ncclSend / ncclRecv over xGMI) when every rank has its own GPU, peer copies otherwise (include/prt.h, prt_group_*).
class HipWavefrontRenderer : public Renderer {
public:
    explicit HipWavefrontRenderer(int device = 0, uint32_t max_depth = 20 /* src/backend/cpu/renderer.h:34 */, uint32_t seed = 0)
        : HipWavefrontRenderer(std::vector<int>{device}, max_depth, seed) {}
    explicit HipWavefrontRenderer(const std::vector<int>& devices, uint32_t max_depth = 20, uint32_t seed = 0) : max_depth_(max_depth), seed_(seed) {
        if (prt_group_create(devices.data(), (uint32_t)devices.size(), &grp_)) {
            std::string msg = prt_group_last_error(grp_);
            prt_group_destroy(grp_);
            grp_ = nullptr;
            throw Error("prt_group_create: " + msg);
        }
    }
    ~HipWavefrontRenderer() override { prt_group_destroy(grp_); }
    HipWavefrontRenderer(const HipWavefrontRenderer&) = delete;
    HipWavefrontRenderer& operator=(const HipWavefrontRenderer&) = delete;
    void Init(Film& film, const Scene& scene, const Camera& camera) override {
        PrtSceneDesc d = scene.desc();
        check(prt_group_set_scene(grp_, &d));  // flattened + BVH built once, cloned to the other GPUs
        if (scene.HasTextures()) SetTextures(scene);
        check(prt_group_set_film(grp_, film.width, film.height));
        film_ = &film;
        frame_ = 0;
        SetCamera(camera);
    }
    void SetCamera(const Camera& camera) override {
        PrtCameraDesc d = camera.desc();
        check(prt_group_set_camera(grp_, &d));
    }
    void ProgressiveRender() override { Render(1); }  // exactly one sample per pixel
    void Render(uint32_t spp) {
        check(prt_group_render(grp_, spp, max_depth_, seed_, frame_));
        frame_ += spp;
    }
    // Film statistics (prt_set_film_statistics): second moments of every pixel's luminance beside the film; switching them
    // clears the film.  RenderAdaptive needs them on.
    void SetFilmStatistics(bool on) {
        check(prt_group_set_film_statistics(grp_, on ? 1 : 0));
        if (on != stats_on_) frame_ = 0;
        stats_on_ = on;
    }
    // Tile-adaptive sampling (prt_render_adaptive): min_spp samples everywhere, then step_spp at a time to the 8x8 tiles that
    // still hold a pixel whose standard error exceeds threshold * (mean + noise_floor), up to max_spp.  After Download() the
    // film's weights are the per-pixel sample counts.  The next Render / RenderAdaptive continues after max_spp indices.
    PrtAdaptiveInfo RenderAdaptive(const PrtAdaptive& cfg) {
        PrtAdaptiveInfo info{};
        check(prt_group_render_adaptive(grp_, &cfg, max_depth_, seed_, frame_, &info));
        frame_ += cfg.max_spp;
        return info;
    }
    // Per-pixel relative standard error (prt_film_noise_read), width * height floats: every pixel from the rank that owns its tile
    void NoiseMap(float noise_floor, std::vector<float>& out) {
        const uint32_t n = prt_group_size(grp_), W = film_->width, H = film_->height, tiles_x = (W + 7u) / 8u;
        out.assign((size_t)W * H, 0.0f);
        std::vector<float> part((size_t)W * H);
        for (uint32_t r = 0; r < n; ++r) {
            PrtContext* c = prt_group_context(grp_, r);
            if (prt_film_noise_read(c, noise_floor, part.data())) throw Error(std::string("prt_film_noise_read: ") + prt_last_error(c));
            for (uint32_t y = 0; y < H; ++y)
                for (uint32_t x = 0; x < W; ++x)
                    if (((y / 8u) * tiles_x + x / 8u) % n == r) out[(size_t)y * W + x] = part[(size_t)y * W + x];
        }
    }
    // First-hit feature images of the pixel-centre rays (prt_render_features, on the first device: every GPU holds the
    // scene): albedo / normal / position width * height * 3 floats, depth and prim width * height.  They do not follow mirrors
    // or glass and do not average over a lens or jitter.
    struct Features {
        std::vector<float> albedo, normal, position, depth;
        std::vector<int32_t> prim;
    };
    void RenderFeatures(Features& out) {
        const size_t n = (size_t)film_->width * film_->height;
        out.albedo.assign(3 * n, 0.0f);
        out.normal.assign(3 * n, 0.0f);
        out.position.assign(3 * n, 0.0f);
        out.depth.assign(n, 0.0f);
        out.prim.assign(n, -1);
        PrtContext* c = prt_group_context(grp_, 0);
        if (prt_render_features(c) || prt_features_read(c, out.albedo.data(), out.normal.data(), out.position.data(), out.depth.data(), out.prim.data()))
            throw Error(std::string("prt_render_features: ") + prt_last_error(c));
    }
    // The guide set through specular chains (prt_features_read_guide, SetFeatureTrace): the same images at the end of each
    // pixel's chain, and the vertices it followed.  With max_specular = 0: the first-hit set and bounces = 0.
    void RenderGuideFeatures(Features& out, std::vector<uint32_t>& bounces) {
        const size_t n = (size_t)film_->width * film_->height;
        out.albedo.assign(3 * n, 0.0f);
        out.normal.assign(3 * n, 0.0f);
        out.position.assign(3 * n, 0.0f);
        out.depth.assign(n, 0.0f);
        out.prim.assign(n, -1);
        bounces.assign(n, 0u);
        PrtContext* c = prt_group_context(grp_, 0);
        if (prt_render_features(c) || prt_features_read_guide(c, out.albedo.data(), out.normal.data(), out.position.data(), out.depth.data(),
                                                              out.prim.data(), bounces.data()))
            throw Error(std::string("prt_render_features: ") + prt_last_error(c));
    }
    // The sampled set (prt_features_read_sampled, SetFeatureSampling): the same images averaged over the render's own primary
    // rays of every pixel, and how many of them hit something.  Needs SetFeatureSampling(samples > 0).
    void RenderSampledFeatures(Features& out, std::vector<uint32_t>& hits) {
        const size_t n = (size_t)film_->width * film_->height;
        out.albedo.assign(3 * n, 0.0f);
        out.normal.assign(3 * n, 0.0f);
        out.position.assign(3 * n, 0.0f);
        out.depth.assign(n, 0.0f);
        out.prim.assign(n, -1);
        hits.assign(n, 0u);
        PrtContext* c = prt_group_context(grp_, 0);
        if (prt_render_features(c) || prt_features_read_sampled(c, out.albedo.data(), out.normal.data(), out.position.data(), out.depth.data(),
                                                                out.prim.data(), hits.data()))
            throw Error(std::string("prt_render_features: ") + prt_last_error(c));
    }
    // The gathered film through the edge-avoiding filter (prt_group_film_denoise; include/prt.h "The filter contract"):
    // width * height * 3 floats of denoised mean radiance, and the filtered variance if asked.  Needs SetFilmStatistics(true).
    // cfg = nullptr: the defaults.
    void Denoise(const PrtDenoise* cfg, std::vector<float>& rgb, std::vector<float>* var = nullptr) {
        const size_t n = (size_t)film_->width * film_->height;
        rgb.assign(3 * n, 0.0f);
        if (var) var->assign(n, 0.0f);
        check(prt_group_film_denoise(grp_, cfg, rgb.data(), var ? var->data() : nullptr));
    }
    // One frame step of the temporal reprojection (prt_film_temporal; include/prt.h "Temporal reprojection") on the first
    // device, which must own the whole image (one GPU: a group form does not exist yet): the film blended with the history
    // the context keeps, through the spatial filter if dn is not null.  width * height * 3 floats; var / history (N' per
    // pixel) if asked.  Needs SetFilmStatistics(true); the film is not touched: Clear() it between frames and keep the sample
    // index running with SetFrameIndex.  tp = nullptr: the defaults.
    void TemporalStep(const PrtTemporal* tp, const PrtDenoise* dn, std::vector<float>& rgb, std::vector<float>* var = nullptr,
                      std::vector<float>* history = nullptr) {
        const size_t n = (size_t)film_->width * film_->height;
        rgb.assign(3 * n, 0.0f);
        if (var) var->assign(n, 0.0f);
        if (history) history->assign(n, 0.0f);
        PrtContext* c = prt_group_context(grp_, 0);
        if (prt_film_temporal(c, tp, dn, rgb.data(), var ? var->data() : nullptr, history ? history->data() : nullptr))
            throw Error(std::string("prt_film_temporal: ") + prt_last_error(c));
    }
    void TemporalReset() {
        PrtContext* c = prt_group_context(grp_, 0);
        if (prt_temporal_reset(c)) throw Error(std::string("prt_temporal_reset: ") + prt_last_error(c));
    }
    // The sample index the next Render starts at (Clear() sets it to 0): an animation keeps it running across its frames.
    void SetFrameIndex(uint32_t first_sample) { frame_ = first_sample; }
    // The placed copies of `scene` moved (Scene::SetInstanceTransform): every GPU's top level follows, no mesh tree is
    // rebuilt and the film is not cleared.  mode: PRT_INSTANCES_REFIT (topology kept) / PRT_INSTANCES_REBUILD
    void UpdateInstances(const Scene& scene, uint32_t mode = PRT_INSTANCES_REFIT) {
        check(prt_group_set_instance_transforms(grp_, scene.instances.data(), (uint32_t)scene.instances.size(), mode));
    }
    // The scene's world-space meshes deformed on the GPU (prt_refit_meshes_device): meshes[m] holds DEVICE pointers to the
    // new positions (and normals, or null: computed on the device) of mesh m, n_vertices x 3 floats each, read in stream
    // order on the context's stream.  A renderer over one GPU only: a device array lives on one device.
    void RefitDevice(const std::vector<PrtMeshDeviceArrays>& meshes) {
        if (prt_group_size(grp_) != 1u) throw Error("RefitDevice: a renderer over several GPUs refits from host arrays");
        PrtContext* c = prt_group_context(grp_, 0);
        if (prt_refit_meshes_device(c, meshes.data(), (uint32_t)meshes.size())) throw Error(std::string("prt_refit_meshes_device: ") + prt_last_error(c));
    }
    PrtRefitInfo RefitInfo(uint32_t rank = 0) {
        PrtRefitInfo info{};
        PrtContext* c = prt_group_context(grp_, rank);
        if (prt_refit_info(c, &info)) throw Error(std::string("prt_refit_info: ") + prt_last_error(c));
        return info;
    }
    PrtInstanceUpdateInfo InstanceUpdateInfo(uint32_t rank = 0) {
        PrtInstanceUpdateInfo info{};
        PrtContext* c = prt_group_context(grp_, rank);
        if (prt_instance_update_info(c, &info)) throw Error(std::string("prt_instance_update_info: ") + prt_last_error(c));
        return info;
    }
    void SetSamplesInFlight(uint32_t n) { check(prt_group_set_samples_in_flight(grp_, n)); }
    void SetParam(const char* name, int value) { check(prt_group_set_param(grp_, name, value)); }
    // Thin lens and field of view (PrtLens): fov_y in radians (0 = the reference's 1 rad), aperture = lens radius in world
    // units (0 = pinhole), focus_distance along the camera's front; kept across SetCamera / Init
    void SetLens(float fov_y = 0.0f, float aperture = 0.0f, float focus_distance = 0.0f) {
        const PrtLens l{fov_y, aperture, focus_distance};
        check(prt_group_set_lens(grp_, &l));
    }
    // Guide features through specular chains (PrtFeatureTrace): the denoiser's features follow up to max_specular (0..8)
    // mirror / glass vertices; a Metal with roughness <= roughness_max is a mirror.  0 = first hit only (the default)
    void SetFeatureTrace(uint32_t max_specular = 0u, float roughness_max = 0.1f) {
        const PrtFeatureTrace ft{max_specular, roughness_max};
        check(prt_group_set_feature_trace(grp_, &ft));
    }
    // Sampled guide features (PrtFeatureSampling): the denoiser's features are averaged over `samples` (0..64) of the
    // render's own primary rays per pixel, those of sample indices first_sample ... under `seed`.  0 = off (the default)
    void SetFeatureSampling(uint32_t samples = 0u, uint32_t seed = 0u, uint32_t first_sample = 0u) {
        const PrtFeatureSampling fs{samples, seed, first_sample};
        check(prt_group_set_feature_sampling(grp_, &fs));
    }
    // Light sampling toward the analytic emitters (PrtLighting): PRT_LIGHTING_OFF / _NEE_MIS / _NEE
    void SetLighting(uint32_t mode) {
        const PrtLighting l{mode};
        check(prt_group_set_lighting(grp_, &l));
    }
    // Which emitters the light set holds: PRT_LIGHT_SOURCES_ANALYTIC (default) or ANALYTIC | MESH (emissive triangles too)
    void SetLightSources(uint32_t mask) { check(prt_group_set_light_sources(grp_, mask)); }
    // Clustered light selection (include/prt.h "Clustered light selection"); it takes effect with PRT_LIGHT_SOURCES_MESH
    void SetLightSelection(const PrtLightSelection& sel) { check(prt_group_set_light_selection(grp_, &sel)); }
    // Environment light (PrtEnvironment): rgb = height * width * 3 floats, row 0 = the +Y pole; null = the constant sky again
    void SetEnvironment(const float* rgb, uint32_t width, uint32_t height, float light_share = 0.5f) {
        if (!rgb) {
            check(prt_group_set_environment(grp_, nullptr));
            return;
        }
        const PrtEnvironment e{rgb, width, height, light_share};
        check(prt_group_set_environment(grp_, &e));
    }
    // ... from a colour PFM file (prt_read_pfm)
    void SetEnvironmentPfm(const std::string& path, float light_share = 0.5f) {
        float* rgb = nullptr;
        uint32_t w = 0, h = 0;
        if (prt_read_pfm(path.c_str(), &rgb, &w, &h)) throw Error("cannot read " + path + " as a colour PFM");
        const PrtEnvironment e{rgb, w, h, light_share};
        const int rc = prt_group_set_environment(grp_, &e);
        prt_image_free(rgb);
        check(rc);
    }
    // Binds the scene's textures (Scene::AddTexture / SetMaterialTexture, the meshes' UVs) on every GPU; `scene` must be the
    // one Init got.  Init does this itself; UpdateInstances keeps the binding.
    void SetTextures(const Scene& scene) {
        const PrtTextureSet t = scene.textureSet();
        check(prt_group_set_textures(grp_, &t));
    }
    void ClearTextures() { check(prt_group_set_textures(grp_, nullptr)); }
    PrtLightStats LightStats() {
        PrtLightStats s{};
        check(prt_group_get_light_stats(grp_, &s));
        return s;
    }
    void Clear() {
        check(prt_group_film_clear(grp_));
        frame_ = 0;
    }
    void Download() { check(prt_group_film_read(grp_, film_->accum.data(), film_->weights.data())); }
    void UpdateDisplay(float exposure = 1.0f, float gamma = 2.2f) { check(prt_group_film_display(grp_, exposure, gamma, film_->display.data())); }
    PrtStats Stats() {
        PrtStats s{};
        check(prt_group_get_stats(grp_, &s));
        return s;
    }
    uint32_t DeviceCount() const { return prt_group_size(grp_); }
    const char* Transport() const { return prt_group_transport(grp_); }
    PrtContext* context(uint32_t rank = 0) { return prt_group_context(grp_, rank); }
    // Occlusion (shadow-ray) query on the first GPU's context: occluded[i] = 1 iff something blocks ray i
    // (origins / dirs: n x 3 floats, host memory) before distance tmax[i] (prt_occluded)
    void Occluded(uint32_t n, const float* origins, const float* dirs, const float* tmax, uint8_t* occluded) {
        PrtContext* c = prt_group_context(grp_, 0);
        if (prt_occluded(c, n, origins, dirs, tmax, occluded)) throw Error(std::string("prt_occluded: ") + prt_last_error(c));
    }
    // Radiance query on the first GPU's context (prt_radiance, include/prt.h "Radiance query"): the fp32 SUM over `samples`
    // paths per ray of the radiance arriving along n caller-supplied rays (origins / dirs: n x 3 floats, host memory) into
    // rgb_sum (3 n floats); sample s of ray i starts from the renderer's seed, the ray index and first_sample + s.
    // rng_state (n, in / out) gives the paths their states instead and needs samples == 1; segments (n) may be null.
    // lighting: the light-sampled query (prt_radiance_lit): the estimator a render would use now (SetLighting,
    // SetLightSources, SetLightSelection, the environment's light share); lit_info (may be null): its shadow-ray counts.
    // pb (n floats, may be null; needs lighting): the pdf of the caller's own Lambertian scatter along each ray, so that what
    // the first segment meets is weighted as after a vertex of the path's own (prt_radiance_lit_pb).
    void Radiance(uint32_t n, const float* origins, const float* dirs, float* rgb_sum, uint32_t samples = 1, uint32_t first_sample = 0,
                  uint32_t* rng_state = nullptr, uint32_t* segments = nullptr, bool lighting = false, PrtRadianceLitInfo* lit_info = nullptr,
                  const float* pb = nullptr) {
        PrtContext* c = prt_group_context(grp_, 0);
        const PrtRadianceQuery q{max_depth_, samples, seed_, first_sample};
        if (pb && !lighting) throw Error("Radiance: pb weights light-sampled paths only: pass lighting = true");
        if (lighting) {
            if (prt_radiance_lit_pb(c, &q, n, origins, dirs, rng_state, pb, rgb_sum, segments, lit_info))
                throw Error(std::string("prt_radiance_lit: ") + prt_last_error(c));
            return;
        }
        if (prt_radiance(c, &q, n, origins, dirs, rng_state, rgb_sum, segments)) throw Error(std::string("prt_radiance: ") + prt_last_error(c));
    }
    // A lat-long radiance probe at `position`: width x height x 3 floats, the mean over `samples` paths along the unit
    // direction of every texel centre, in prt_set_environment's layout (row 0 = the +Y pole), so that a probe written with
    // prt_write_pfm can light another scene through SetEnvironmentPfm.  The directions are those of the Python package's
    // probe_directions: float64, the C library's sin / cos, rounded once.  lighting: Radiance's.
    void RenderProbe(const float position[3], uint32_t width, uint32_t height, uint32_t samples, std::vector<float>& rgb,
                     bool lighting = false) {
        const size_t n = (size_t)width * height;
        const double pi = 3.141592653589793;
        std::vector<float> o(3 * n), d(3 * n);
        for (uint32_t i = 0; i < height; ++i) {
            const double theta = pi * ((i + 0.5) / height), ct = std::cos(theta), st = std::sin(theta);
            for (uint32_t j = 0; j < width; ++j) {
                const double phi = 2.0 * pi * ((j + 0.5) / width) - pi;
                const double x = st * std::cos(phi), y = ct, z = st * std::sin(phi);
                const double inv = 1.0 / std::sqrt((x * x + y * y) + z * z);
                const size_t k = 3 * ((size_t)i * width + j);
                d[k] = (float)(x * inv), d[k + 1] = (float)(y * inv), d[k + 2] = (float)(z * inv);
                o[k] = position[0], o[k + 1] = position[1], o[k + 2] = position[2];
            }
        }
        rgb.assign(3 * n, 0.0f);
        Radiance((uint32_t)n, o.data(), d.data(), rgb.data(), samples, 0u, nullptr, nullptr, lighting);
        for (float& v : rgb) v = v / (float)samples;
    }
    // Surface baking on the first GPU's context (prt_bake_irradiance, include/prt.h "Surface baking"): the irradiance map of
    // world-space mesh `index` (kind = PRT_BAKE_INSTANCE: placed copy `index`) over its UV layout, width x height x 3 floats,
    // pi * sum / samples, row 0 on top.  uvs: n_vertices x 2 floats for this call, null: the texture binding's.  dilate:
    // passes of the gutter fill.  coverage (may be null): width x height bytes, 0 none, 1 owned, 2 filled.  lighting:
    // Radiance's.  info (may be null): the counts of the call.  texel_light (needs lighting): a light sample at the texel
    // itself and the texel's own ray MIS-weighted (prt_bake_irradiance_opt).
    void BakeIrradiance(uint32_t index, const float* uvs, uint32_t width, uint32_t height, uint32_t samples, std::vector<float>& irradiance,
                        uint32_t dilate = 0, bool lighting = false, std::vector<uint8_t>* coverage = nullptr, PrtBakeInfo* info = nullptr,
                        uint32_t kind = PRT_BAKE_MESH, uint32_t first_sample = 0, bool texel_light = false) {
        PrtContext* c = prt_group_context(grp_, 0);
        const PrtBakeTarget t{kind, index, uvs, width, height};
        const PrtRadianceQuery q{max_depth_, samples, seed_, first_sample};
        const size_t n = (size_t)width * height;
        irradiance.assign(3 * n, 0.0f);
        if (coverage) coverage->assign(n, 0);
        if (texel_light && !lighting) throw Error("BakeIrradiance: texel_light belongs to a light-sampled bake: pass lighting = true");
        const PrtBakeOptions opt{lighting ? 1u : 0u, texel_light ? 1u : 0u, dilate, 0u};
        if (prt_bake_irradiance_opt(c, &t, &q, &opt, irradiance.data(), coverage ? coverage->data() : nullptr, info))
            throw Error(std::string("prt_bake_irradiance: ") + prt_last_error(c));
        for (float& v : irradiance) v = v * 3.14159274f / (float)samples;
    }
    // The bake with per-texel statistics and block-adaptive sampling (prt_bake_irradiance_adaptive, include/prt.h "Bake
    // statistics and adaptive sampling"): cfg.min_spp samples for every covered texel, then cfg.step_spp at a time for the
    // covered texels of the 8x8 blocks that still hold an unconverged one, up to cfg.max_spp.  irradiance: pi * the mean
    // (after `dilate` passes of the gutter fill, which touch the mean alone).  count / sum_y / sum_y2 / coverage (each may be
    // null): the per-texel sample counts, the luminance moments and the coverage bytes.  The other arguments: BakeIrradiance's.
    void BakeIrradianceAdaptive(uint32_t index, const float* uvs, uint32_t width, uint32_t height, const PrtBakeAdaptive& cfg,
                                std::vector<float>& irradiance, std::vector<float>* count = nullptr, std::vector<float>* sum_y = nullptr,
                                std::vector<float>* sum_y2 = nullptr, uint32_t dilate = 0, bool lighting = false,
                                std::vector<uint8_t>* coverage = nullptr, PrtBakeInfo* info = nullptr, PrtBakeAdaptiveInfo* adaptive_info = nullptr,
                                uint32_t kind = PRT_BAKE_MESH, uint32_t first_sample = 0, bool texel_light = false) {
        PrtContext* c = prt_group_context(grp_, 0);
        const PrtBakeTarget t{kind, index, uvs, width, height};
        const PrtRadianceQuery q{max_depth_, 0u, seed_, first_sample};
        const size_t n = (size_t)width * height;
        std::vector<float> sum(3 * n, 0.0f);
        irradiance.assign(3 * n, 0.0f);
        for (std::vector<float>* v : {count, sum_y, sum_y2})
            if (v) v->assign(n, 0.0f);
        if (coverage) coverage->assign(n, 0);
        if (texel_light && !lighting) throw Error("BakeIrradianceAdaptive: texel_light belongs to a light-sampled bake: pass lighting = true");
        const PrtBakeOptions opt{lighting ? 1u : 0u, texel_light ? 1u : 0u, dilate, 0u};
        if (prt_bake_irradiance_adaptive(c, &t, &q, &opt, &cfg, sum.data(), count ? count->data() : nullptr, sum_y ? sum_y->data() : nullptr,
                                         sum_y2 ? sum_y2->data() : nullptr, irradiance.data(), coverage ? coverage->data() : nullptr, info,
                                         adaptive_info))
            throw Error(std::string("prt_bake_irradiance_adaptive: ") + prt_last_error(c));
        for (float& v : irradiance) v = v * 3.14159274f;
    }
    // Light probes on the first GPU's context (prt_probe_sh, include/prt.h "SH probes"): the radiance arriving at n_probes
    // points (positions: 3 floats each) as real spherical-harmonic coefficients, n_probes x (order + 1)^2 x 3 floats,
    // 4 pi * sum / samples.  lighting: Radiance's.  info (may be null): the counts of the call.
    void ProbeSH(uint32_t n_probes, const float* positions, uint32_t order, uint32_t samples, std::vector<float>& coeffs, bool lighting = false,
                 PrtProbeShInfo* info = nullptr, uint32_t first_sample = 0) {
        PrtContext* c = prt_group_context(grp_, 0);
        const PrtProbeShOptions opt{order, lighting ? 1u : 0u, {0u, 0u}};
        const PrtRadianceQuery q{max_depth_, samples, seed_, first_sample};
        coeffs.assign((size_t)n_probes * (order <= 2u ? (order + 1u) * (order + 1u) : 1u) * 3u, 0.0f);
        if (prt_probe_sh(c, &opt, &q, n_probes, positions, coeffs.data(), info)) throw Error(std::string("prt_probe_sh: ") + prt_last_error(c));
        for (float& v : coeffs) v = v * (4.0f * 3.14159274f) / (float)samples;
    }

private:
    void check(int rc) {
        if (rc) throw Error(prt_group_last_error(grp_));
    }
    PrtGroup* grp_ = nullptr;
    Film* film_ = nullptr;
    uint32_t max_depth_, seed_, frame_ = 0;
    bool stats_on_ = false;
};

}  // namespace prt

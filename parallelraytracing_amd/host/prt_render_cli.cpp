// prt_render — offline framebuffer dump: the stand-in for the reference's GLFW/ImGui/OpenGL viewer
// (src/main.cpp:138-170 builds Film/Scene/Camera and Inits the backends; :504-527 is the frame loop).
//   prt_render [--preset NAME | --ply FILE [--refine N]] [--width W --height H] [--spp N] [--depth D]
//              [--seed S] [--camera x y z] [--out PREFIX] [--gpus N | --devices a,b,c] [--sif S] [--frames K]
//              [--lighting off|nee|mis] [--light-sources analytic|all] [--light-selection power|clustered [--light-clusters N]]
//              [--env FILE.pfm [--env-share Q]]
//              [--fov-deg D] [--aperture R --focus F]
//              [--ground-texture FILE.pfm] [--mesh-texture FILE.pfm] [--texture-filter nearest|bilinear]
//              [--adaptive THRESHOLD [--min-spp N --spp-step N --max-spp N --noise-floor F]
//               [--samples-out FILE.pfm] [--noise-out FILE.pfm]]
//              [--denoise [--denoise-iterations N --denoise-sigma-l S --denoise-sigma-z S --no-demodulate]
//               [--follow-specular N [--mirror-roughness R]] [--feature-samples K]]
//              [--features-out PREFIX]
//              [--frames N --orbit-deg D [--temporal [--temporal-max-history H]]]
//              [--probe X,Y,Z --probe-size WxH --probe-lighting]
//              [--bake WxH --bake-dilate N --bake-texel-light]
//              [--bake WxH --bake-adaptive T [--min-spp N --spp-step N --max-spp N --noise-floor F] [--samples-out S.pfm] [--noise-out N.pfm]]
//              [--probe-grid NXxNYxNZ --probe-box x0,y0,z0,x1,y1,z1 [--probe-order N] [--probe-lighting]]
// --probe-grid NXxNYxNZ with --probe-box renders no frame: it writes PREFIX.pfm, the light probes of a cell-centred grid over
// the box (x fastest; the Python package's probe_grid) as real spherical-harmonic coefficients (prt_probe_sh): one row per
// probe, (order + 1)^2 texels wide (--probe-order 0 | 1 | 2, default 2), each texel the rgb coefficient 4 pi * sum / spp of
// --spp uniformly distributed paths of up to --depth segments.  The first GPU; --probe-lighting as for --probe.
// --bake WxH (with --ply) renders no frame: it writes PREFIX.pfm, the irradiance map of the mesh over the PLY's own UVs
// (prt_bake_irradiance): --spp paths of up to --depth segments per covered texel, pi * sum / spp, top row first;
// --bake-dilate N fills the gutters with N passes.  The first GPU; --lighting applies as it would to a frame.
// --bake-texel-light (with --lighting nee|mis) also samples the lights at the texel itself (prt_bake_irradiance_opt).
// --bake-adaptive T (with --bake) bakes with block-adaptive sampling (prt_bake_irradiance_adaptive) instead of --spp samples for
// every texel: --min-spp (default 8) samples for every covered texel, then --spp-step (8) at a time for the 8x8 blocks of texels
// that still hold one whose standard error exceeds T times (its mean luminance + --noise-floor), up to --max-spp (64);
// PREFIX.pfm is pi * the mean.  --samples-out and --noise-out write the per-texel sample counts and the relative standard
// errors (prt_bake_noise) as grey PFMs of the map's size.
// --probe X,Y,Z renders no frame: it writes PREFIX.pfm, a lat-long radiance probe of --probe-size WxH texels (default 64x32)
// at that point, --spp paths of up to --depth segments per texel along the texel centre's direction (prt_radiance), in the
// layout --env reads (top row = the +Y pole): a probe of one scene can light another.  The first GPU; the estimator is the
// unidirectional one whatever --lighting says, unless --probe-lighting is given: then --lighting, --light-sources and
// --light-selection apply to the probe as they would to a frame (prt_radiance_lit).
// --orbit-deg D turns --frames N into an animation: frame f is rendered with --spp samples (sample indices f * spp ...) from the
// camera turned f * D degrees about the vertical axis through the origin, looking at the origin, on a cleared film, and written
// as PREFIX_fNNN.pfm.  --temporal carries the film history across the frames (prt_film_temporal: reprojection, disocclusion
// test, blend; then the a-trous filter if --denoise is given) and writes PREFIX_fNNN_temporal.pfm beside each frame.  One GPU.
// --denoise turns the film statistics on and, beside the noisy frame, writes PREFIX_denoised.pfm / .ppm: the film through the
// edge-avoiding a-trous filter (prt_group_film_denoise; 5 iterations, sigma_l 4, sigma_z 0.1 unless set), guided by the
// variance of every pixel's mean and by the first hit of its centre ray.  --features-out P writes those first-hit images as
// colour PFMs: P_albedo.pfm, P_normal.pfm, P_position.pfm and P_depth.pfm (the value in all three channels).
// --follow-specular N (1..8) lets the filter's features follow up to N mirror / glass vertices of the centre ray
// (prt_set_feature_trace; a Metal with roughness <= --mirror-roughness, default 0.1, is a mirror): the reflected image is
// filtered by what is seen in the mirror, not as the mirror's plane.  --features-out then also writes P_guide_albedo.pfm,
// P_guide_normal.pfm, P_guide_position.pfm, P_guide_depth.pfm and P_guide_bounces.pfm.
// --feature-samples K (1..64) averages the filter's features over the first K of each pixel's own primary rays, through the
// lens and the jitter (prt_set_feature_sampling with the run's seed and first sample index; with --frames N --orbit-deg D,
// every frame's own): a defocused pixel gets the mixture of surfaces its film holds.  It needs --denoise or
// --features-out; --features-out then also writes P_sampled_albedo.pfm, P_sampled_normal.pfm, P_sampled_position.pfm,
// P_sampled_depth.pfm and P_sampled_hits.pfm.
// --adaptive T renders with tile-adaptive sampling (prt_render_adaptive) instead of --spp samples everywhere: --min-spp
// (default 8) samples for every pixel, then --spp-step (8) at a time for the 8x8 tiles that still hold a pixel whose standard
// error exceeds T x (mean luminance + --noise-floor (0.01)), up to --max-spp (64).  --samples-out writes every pixel's sample
// count and --noise-out its relative standard error, as colour PFMs with the value in all three channels.
// --ground-texture / --mesh-texture (with --ply) take the albedo of the ground quad / of the mesh from a colour PFM (top
// row first, repeated outside [0, 1]); the mesh needs per-vertex UVs in its PLY (s/t, u/v or texture_u/texture_v).
// --fov-deg sets the vertical field of view in degrees (default: the reference's 1 rad); --aperture R (lens radius, world
// units) with --focus F (distance of the plane in focus along the view direction) renders with a thin lens.
// --env lights the scene with a lat-long colour PFM (top row = the +Y pole) instead of the constant sky; with a lighting
// mode, a light sample goes to the image with probability Q (default 0.5).
// --gpus N tiles the image over devices 0..N-1 (--devices: any list; a device may repeat, which rehearses the multi-GPU
// path on one GPU); the frame is gathered to the first device once per frame (RCCL over xGMI, or peer copies).
// Writes PREFIX.ppm (tonemapped RGBA8 as PPM) and PREFIX.pfm (mean radiance).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "prt_renderer.hpp"

static int preset_id(const std::string& n) {
    const char* names[] = {"DEFAULT", "LIGHT_TEST", "MATERIAL_TEST", "CORNELL", "RANDOM_BALLS_SMALL", "RANDOM_BALLS_MEDIUM", "RANDOM_BALLS_LARGE"};
    for (int i = 0; i < 7; ++i)
        if (n == names[i]) return i;
    return -1;
}

int main(int argc, char** argv) {
    std::string preset = "CORNELL", ply, out = "frame", env, ground_tex, mesh_tex;
    uint32_t tex_filter = PRT_TEX_NEAREST;
    float env_share = 0.5f, aperture = 0.0f, focus = 0.0f;
    double fov_deg = 0.0;
    uint32_t W = 256, H = 256, spp = 1, depth = 2, seed = 0, refine = 0, sif = 0, frames = 1, lighting = PRT_LIGHTING_OFF;
    uint32_t light_sources = PRT_LIGHT_SOURCES_ANALYTIC;
    PrtLightSelection light_selection{PRT_LIGHT_SELECTION_POWER, 0u};
    bool adaptive = false;
    PrtAdaptive ad{8u, 8u, 64u, 0.0f, 0.01f};
    std::string samples_out, noise_out, features_out;
    bool denoise = false;
    PrtDenoise dn;
    prt_denoise_defaults(&dn);
    PrtFeatureTrace ftrace;
    prt_feature_trace_defaults(&ftrace);
    uint32_t feature_samples = 0;
    bool orbit = false, temporal = false;
    double orbit_deg = 0.0;
    PrtTemporal tp;
    prt_temporal_defaults(&tp);
    bool probe = false, probe_lighting = false;
    float probe_pos[3] = {0.0f, 0.0f, 0.0f};
    uint32_t probe_w = 64, probe_h = 32;
    bool probe_grid = false, probe_box_set = false;
    uint32_t grid_n[3] = {0, 0, 0}, probe_order = 2;
    double probe_box[6] = {0, 0, 0, 0, 0, 0};
    bool bake = false;
    uint32_t bake_w = 0, bake_h = 0, bake_dilate = 0;
    bool bake_texel_light = false, bake_adaptive = false;
    std::vector<int> devices{0};
    float cam[3] = {5.0f, 5.0f, 8.0f};
    bool cam_set = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--preset") preset = next();
        else if (a == "--ply") ply = next();
        else if (a == "--refine") refine = (uint32_t)atoi(next());
        else if (a == "--width") W = (uint32_t)atoi(next());
        else if (a == "--height") H = (uint32_t)atoi(next());
        else if (a == "--spp") spp = (uint32_t)atoi(next());
        else if (a == "--depth") depth = (uint32_t)atoi(next());
        else if (a == "--seed") seed = (uint32_t)atoi(next());
        else if (a == "--out") out = next();
        else if (a == "--sif") sif = (uint32_t)atoi(next());
        else if (a == "--frames") frames = (uint32_t)atoi(next());
        else if (a == "--lighting") {
            const std::string m = next();
            if (m == "off") lighting = PRT_LIGHTING_OFF;
            else if (m == "nee") lighting = PRT_LIGHTING_NEE;
            else if (m == "mis") lighting = PRT_LIGHTING_NEE_MIS;
            else { fprintf(stderr, "--lighting takes off, nee or mis\n"); return 2; }
        }
        else if (a == "--light-sources") {
            const std::string m = next();
            if (m == "analytic") light_sources = PRT_LIGHT_SOURCES_ANALYTIC;
            else if (m == "all") light_sources = PRT_LIGHT_SOURCES_ANALYTIC | PRT_LIGHT_SOURCES_MESH;
            else { fprintf(stderr, "--light-sources takes analytic or all\n"); return 2; }
        }
        else if (a == "--light-selection") {
            const std::string m = next();
            if (m == "power") light_selection.mode = PRT_LIGHT_SELECTION_POWER;
            else if (m == "clustered") light_selection.mode = PRT_LIGHT_SELECTION_CLUSTERED;
            else { fprintf(stderr, "--light-selection takes power or clustered\n"); return 2; }
        }
        else if (a == "--light-clusters") {
            const int n = atoi(next());
            if (n < 1 || n > (int)PRT_LIGHT_MAX_CLUSTERS) { fprintf(stderr, "--light-clusters takes 1 to %u\n", PRT_LIGHT_MAX_CLUSTERS); return 2; }
            light_selection.max_clusters = (uint32_t)n;
        }
        else if (a == "--env") env = next();
        else if (a == "--env-share") env_share = (float)atof(next());
        else if (a == "--fov-deg") fov_deg = atof(next());
        else if (a == "--aperture") aperture = (float)atof(next());
        else if (a == "--focus") focus = (float)atof(next());
        else if (a == "--ground-texture") ground_tex = next();
        else if (a == "--mesh-texture") mesh_tex = next();
        else if (a == "--texture-filter") {
            const std::string m = next();
            if (m == "nearest") tex_filter = PRT_TEX_NEAREST;
            else if (m == "bilinear") tex_filter = PRT_TEX_BILINEAR;
            else { fprintf(stderr, "--texture-filter takes nearest or bilinear\n"); return 2; }
        }
        else if (a == "--adaptive") { ad.threshold = (float)atof(next()); adaptive = true; }
        else if (a == "--min-spp") ad.min_spp = (uint32_t)atoi(next());
        else if (a == "--spp-step") ad.step_spp = (uint32_t)atoi(next());
        else if (a == "--max-spp") ad.max_spp = (uint32_t)atoi(next());
        else if (a == "--noise-floor") ad.noise_floor = (float)atof(next());
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-iterations") dn.iterations = (uint32_t)atoi(next());
        else if (a == "--denoise-sigma-l") dn.sigma_l = (float)atof(next());
        else if (a == "--denoise-sigma-z") dn.sigma_z = (float)atof(next());
        else if (a == "--no-demodulate") dn.demodulate = 0u;
        else if (a == "--follow-specular") ftrace.max_specular = (uint32_t)atoi(next());
        else if (a == "--mirror-roughness") ftrace.roughness_max = (float)atof(next());
        else if (a == "--feature-samples") feature_samples = (uint32_t)atoi(next());
        else if (a == "--features-out") features_out = next();
        else if (a == "--orbit-deg") { orbit_deg = atof(next()); orbit = true; }
        else if (a == "--temporal") temporal = true;
        else if (a == "--temporal-max-history") tp.max_history = (float)atof(next());
        else if (a == "--probe") {
            if (sscanf(next(), "%f,%f,%f", &probe_pos[0], &probe_pos[1], &probe_pos[2]) != 3) { fprintf(stderr, "--probe takes X,Y,Z\n"); return 2; }
            probe = true;
        }
        else if (a == "--probe-lighting") probe_lighting = true;
        else if (a == "--probe-grid") {
            if (sscanf(next(), "%ux%ux%u", &grid_n[0], &grid_n[1], &grid_n[2]) != 3 || !grid_n[0] || !grid_n[1] || !grid_n[2]) { fprintf(stderr, "--probe-grid takes NXxNYxNZ\n"); return 2; }
            probe_grid = true;
        }
        else if (a == "--probe-box") {
            if (sscanf(next(), "%lf,%lf,%lf,%lf,%lf,%lf", &probe_box[0], &probe_box[1], &probe_box[2], &probe_box[3], &probe_box[4], &probe_box[5]) != 6) { fprintf(stderr, "--probe-box takes x0,y0,z0,x1,y1,z1\n"); return 2; }
            probe_box_set = true;
        }
        else if (a == "--probe-order") probe_order = (uint32_t)atoi(next());
        else if (a == "--bake") {
            if (sscanf(next(), "%ux%u", &bake_w, &bake_h) != 2 || !bake_w || !bake_h) { fprintf(stderr, "--bake takes WxH\n"); return 2; }
            bake = true;
        }
        else if (a == "--bake-dilate") bake_dilate = (uint32_t)atoi(next());
        else if (a == "--bake-texel-light") bake_texel_light = true;
        else if (a == "--bake-adaptive") { ad.threshold = (float)atof(next()); bake_adaptive = true; }
        else if (a == "--probe-size") {
            if (sscanf(next(), "%ux%u", &probe_w, &probe_h) != 2 || !probe_w || !probe_h) { fprintf(stderr, "--probe-size takes WxH\n"); return 2; }
        }
        else if (a == "--samples-out") samples_out = next();
        else if (a == "--noise-out") noise_out = next();
        else if (a == "--gpus") { const int n = atoi(next()); devices.clear(); for (int d = 0; d < n; ++d) devices.push_back(d); }
        else if (a == "--devices") { devices.clear(); std::string l = next(); for (size_t p = 0; p < l.size();) { size_t e = l.find(',', p); if (e == std::string::npos) e = l.size(); devices.push_back(atoi(l.substr(p, e - p).c_str())); p = e + 1; } }
        else if (a == "--camera") { for (int k = 0; k < 3; ++k) cam[k] = (float)atof(next()); cam_set = true; }
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if ((!ground_tex.empty() || !mesh_tex.empty()) && ply.empty()) {
        fprintf(stderr, "--ground-texture and --mesh-texture go with --ply (the presets have no ground quad or mesh of their own)\n");
        return 2;
    }
    if (!adaptive && !bake_adaptive && (!samples_out.empty() || !noise_out.empty())) {
        fprintf(stderr, "--samples-out and --noise-out go with --adaptive or --bake-adaptive\n");
        return 2;
    }
    if (bake_adaptive && !bake) {
        fprintf(stderr, "--bake-adaptive goes with --bake\n");
        return 2;
    }
    if (feature_samples && !denoise && features_out.empty()) {
        fprintf(stderr, "--feature-samples goes with --denoise or --features-out\n");
        return 2;
    }
    if (temporal && !orbit) {
        fprintf(stderr, "--temporal goes with --frames N --orbit-deg D\n");
        return 2;
    }
    if (orbit && adaptive) {
        fprintf(stderr, "--orbit-deg renders --spp samples per frame: it does not go with --adaptive\n");
        return 2;
    }
    if (probe && (orbit || adaptive || denoise || !features_out.empty())) {
        fprintf(stderr, "--probe renders no frame: it does not go with --orbit-deg, --adaptive, --denoise or --features-out\n");
        return 2;
    }
    if (bake && (ply.empty() || probe || orbit || adaptive || denoise || temporal || !features_out.empty())) {
        fprintf(stderr, "--bake goes with --ply and renders no frame: it does not go with --probe, --orbit-deg, --adaptive, --denoise, --temporal or --features-out\n");
        return 2;
    }
    if (bake_texel_light && (!bake || lighting == PRT_LIGHTING_OFF)) {
        fprintf(stderr, "--bake-texel-light goes with --bake and --lighting nee or mis\n");
        return 2;
    }
    if (probe_lighting && !probe && !probe_grid) {
        fprintf(stderr, "--probe-lighting goes with --probe or --probe-grid\n");
        return 2;
    }
    if (probe_grid != probe_box_set || (probe_grid && (probe || bake || orbit || adaptive || denoise || temporal || !features_out.empty()))) {
        fprintf(stderr, "--probe-grid goes with --probe-box and renders no frame: it does not go with --probe, --bake, --orbit-deg, --adaptive, --denoise, --temporal or --features-out\n");
        return 2;
    }
    if (probe_order > 2u || (uint64_t)grid_n[0] * grid_n[1] * grid_n[2] > 0xFFFFFFFFull) {
        fprintf(stderr, "--probe-order takes 0, 1 or 2, and --probe-grid at most 2^32 - 1 probes\n");
        return 2;
    }
    if (temporal && devices.size() != 1) {
        fprintf(stderr, "--temporal runs on one GPU: a group form of the temporal step does not exist yet\n");
        return 2;
    }
    try {
        std::unique_ptr<prt::Scene> scene;
        if (!ply.empty()) {
            scene.reset(new prt::Scene(prt::Scene::Empty{}));
            const uint32_t ground = scene->AddMaterial(PRT_MAT_LAMBERTIAN, 0.5f, 0.5f, 0.5f, 0);
            const uint32_t light = scene->AddMaterial(PRT_MAT_EMISSIVE, 15, 15, 15, 0);
            const uint32_t body = scene->AddMaterial(PRT_MAT_LAMBERTIAN, 0.8f, 0.8f, 0.8f, 0);
            const float one[3] = {1, 1, 1}, zero[3] = {0, 0, 0}, flip[3] = {180, 0, 0}, gt[3] = {0, -1, 0}, lt[3] = {0, 5, 0};
            scene->AddPrimitive(PRT_SHAPE_QUAD, 20, 20, ground, one, zero, gt);
            scene->AddPrimitive(PRT_SHAPE_QUAD, 4, 4, light, one, flip, lt);
            scene->AddMeshPly(ply, body, refine);
            if (!ground_tex.empty()) scene->SetMaterialTexture(ground, scene->AddTexturePfm(ground_tex, tex_filter));
            if (!mesh_tex.empty()) {
                if (!scene->MeshHasUVs(0)) { fprintf(stderr, "error: --mesh-texture: %s has no per-vertex UVs\n", ply.c_str()); return 1; }
                scene->SetMaterialTexture(body, scene->AddTexturePfm(mesh_tex, tex_filter));
            }
            if (!cam_set) { cam[0] = 1.2f; cam[1] = 0.4f; cam[2] = 1.9f; }
        } else {
            const int id = preset_id(preset);
            if (id < 0) { fprintf(stderr, "unknown preset %s\n", preset.c_str()); return 2; }
            scene.reset(new prt::Scene(id));
        }
        prt::Camera camera;
        for (int k = 0; k < 3; ++k) { camera.position[k] = cam[k]; camera.front[k] = -cam[k]; }
        camera.width = (float)W;
        camera.height = (float)H;
        prt::Film film(W, H);
        if (devices.empty()) { fprintf(stderr, "no devices\n"); return 2; }
        prt::HipWavefrontRenderer r(devices, depth, seed);
        r.Init(film, *scene, camera);
        if (sif) r.SetSamplesInFlight(sif);
        if (lighting != PRT_LIGHTING_OFF) r.SetLighting(lighting);
        if (light_sources != (uint32_t)PRT_LIGHT_SOURCES_ANALYTIC) r.SetLightSources(light_sources);
        if (light_selection.mode != (uint32_t)PRT_LIGHT_SELECTION_POWER || light_selection.max_clusters) r.SetLightSelection(light_selection);
        if (!env.empty()) r.SetEnvironmentPfm(env, env_share);
        if (fov_deg != 0.0 || aperture != 0.0f) r.SetLens((float)(fov_deg * 3.14159265358979323846 / 180.0), aperture, focus);
        if (ftrace.max_specular) r.SetFeatureTrace(ftrace.max_specular, ftrace.roughness_max);
        if (feature_samples) r.SetFeatureSampling(feature_samples, seed, 0u);
        if (adaptive || denoise || temporal) r.SetFilmStatistics(true);
        if (probe) {
            std::vector<float> rgb;
            r.RenderProbe(probe_pos, probe_w, probe_h, spp, rgb, probe_lighting);
            if (prt_write_pfm((out + ".pfm").c_str(), rgb.data(), probe_w, probe_h)) { fprintf(stderr, "cannot write %s.pfm\n", out.c_str()); return 1; }
            printf("probe at (%g, %g, %g): %ux%u texels, %u spp, max_depth %u -> %s.pfm\n", probe_pos[0], probe_pos[1], probe_pos[2], probe_w, probe_h, spp,
                   depth, out.c_str());
            return 0;
        }
        if (probe_grid) {  // cell centres in double, rounded once, x fastest: the Python package's probe_grid
            const uint32_t n_probes = grid_n[0] * grid_n[1] * grid_n[2], K = (probe_order + 1u) * (probe_order + 1u);
            std::vector<float> pos(3 * (size_t)n_probes), coeffs;
            for (uint32_t k = 0, p = 0; k < grid_n[2]; ++k)
                for (uint32_t j = 0; j < grid_n[1]; ++j)
                    for (uint32_t i = 0; i < grid_n[0]; ++i, ++p) {
                        const uint32_t cell[3] = {i, j, k};
                        for (int a = 0; a < 3; ++a)
                            pos[3 * (size_t)p + a] = (float)(probe_box[a] + ((double)cell[a] + 0.5) * ((probe_box[3 + a] - probe_box[a]) / (double)grid_n[a]));
                    }
            PrtProbeShInfo pi{};
            r.ProbeSH(n_probes, pos.data(), probe_order, spp, coeffs, probe_lighting, &pi);
            if (prt_write_pfm((out + ".pfm").c_str(), coeffs.data(), K, n_probes)) { fprintf(stderr, "cannot write %s.pfm\n", out.c_str()); return 1; }
            printf("probes: %ux%ux%u grid, order %u, %u spp, max_depth %u, %llu segments, %.3f ms on the device -> %s.pfm (%u x %u)\n", grid_n[0], grid_n[1],
                   grid_n[2], probe_order, spp, depth, (unsigned long long)pi.segments, pi.device_ms, out.c_str(), K, n_probes);
            return 0;
        }
        if (bake) {
            if (!scene->MeshHasUVs(0)) { fprintf(stderr, "error: --bake: %s has no per-vertex UVs\n", ply.c_str()); return 1; }
            std::vector<float> irr;
            PrtBakeInfo bi{};
            if (bake_adaptive) {
                const PrtBakeAdaptive cfg{ad.min_spp, ad.step_spp, ad.max_spp, ad.threshold, ad.noise_floor, {0u, 0u, 0u}};
                PrtBakeAdaptiveInfo ai{};
                std::vector<float> count, sum_y, sum_y2;
                r.BakeIrradianceAdaptive(0u, scene->mesh_uvs.at(0), bake_w, bake_h, cfg, irr, &count, &sum_y, &sum_y2, bake_dilate,
                                         lighting != PRT_LIGHTING_OFF, nullptr, &bi, &ai, PRT_BAKE_MESH, 0u, bake_texel_light);
                auto write_grey = [&](const std::string& path, const std::vector<float>& v) {
                    std::vector<float> rgb(3 * v.size());
                    for (size_t i = 0; i < v.size(); ++i) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = v[i];
                    return prt_write_pfm(path.c_str(), rgb.data(), bake_w, bake_h);
                };
                if (prt_write_pfm((out + ".pfm").c_str(), irr.data(), bake_w, bake_h)) { fprintf(stderr, "cannot write %s.pfm\n", out.c_str()); return 1; }
                if (!samples_out.empty() && write_grey(samples_out, count)) { fprintf(stderr, "cannot write %s\n", samples_out.c_str()); return 1; }
                if (!noise_out.empty()) {
                    std::vector<float> noise(count.size());
                    if (prt_bake_noise(count.size(), count.data(), sum_y.data(), sum_y2.data(), cfg.noise_floor, noise.data()) ||
                        write_grey(noise_out, noise)) { fprintf(stderr, "cannot write %s\n", noise_out.c_str()); return 1; }
                }
                printf("adaptive bake: %ux%u texels, %llu covered, %llu filled, threshold %g, %u..%u spp in steps of %u: %u passes, %llu texel-samples, "
                       "%u blocks: %u converged, %u at the cap, %u..%u spp per texel, max_depth %u, %llu segments, %.3f ms on the device -> %s.pfm\n",
                       bake_w, bake_h, (unsigned long long)bi.n_covered, (unsigned long long)bi.n_filled, cfg.threshold, cfg.min_spp, cfg.max_spp,
                       cfg.step_spp, ai.passes, (unsigned long long)ai.texel_samples, ai.blocks, ai.blocks_converged, ai.blocks_capped, ai.min_texel_spp,
                       ai.max_texel_spp, depth, (unsigned long long)bi.segments, bi.device_ms, out.c_str());
                return 0;
            }
            r.BakeIrradiance(0u, scene->mesh_uvs.at(0), bake_w, bake_h, spp, irr, bake_dilate, lighting != PRT_LIGHTING_OFF, nullptr, &bi, PRT_BAKE_MESH, 0u,
                             bake_texel_light);
            if (prt_write_pfm((out + ".pfm").c_str(), irr.data(), bake_w, bake_h)) { fprintf(stderr, "cannot write %s.pfm\n", out.c_str()); return 1; }
            printf("bake: %ux%u texels, %llu covered, %llu filled, %u spp, max_depth %u, %llu segments, %.3f ms on the device -> %s.pfm\n", bake_w, bake_h,
                   (unsigned long long)bi.n_covered, (unsigned long long)bi.n_filled, spp, depth, (unsigned long long)bi.segments, bi.device_ms, out.c_str());
            return 0;
        }
        if (orbit) {  // the animation: one cleared film per frame, the camera on a circle about the vertical axis
            std::vector<float> mean((size_t)W * H * 3), trgb;
            for (uint32_t f = 0; f < frames; ++f) {
                const double a = (double)f * orbit_deg * 3.14159265358979323846 / 180.0;
                const float px = (float)((double)cam[0] * std::cos(a) + (double)cam[2] * std::sin(a));
                const float pz = (float)(-(double)cam[0] * std::sin(a) + (double)cam[2] * std::cos(a));
                camera.position[0] = px, camera.position[1] = cam[1], camera.position[2] = pz;
                for (int k = 0; k < 3; ++k) camera.front[k] = -camera.position[k];
                r.SetCamera(camera);
                r.Clear();
                r.SetFrameIndex(f * spp);
                if (feature_samples) r.SetFeatureSampling(feature_samples, seed, f * spp);
                r.Render(spp);
                r.Download();
                for (size_t i = 0; i < (size_t)W * H; ++i)
                    for (int c = 0; c < 3; ++c) mean[3 * i + c] = film.weights[i] > 0 ? film.accum[3 * i + c] / film.weights[i] : 0.0f;
                char tag[32];
                snprintf(tag, sizeof(tag), "_f%03u", f);
                bool bad = prt_write_pfm((out + tag + ".pfm").c_str(), mean.data(), W, H) != 0;
                if (temporal && !bad) {
                    r.TemporalStep(&tp, denoise ? &dn : nullptr, trgb);
                    bad = prt_write_pfm((out + tag + "_temporal.pfm").c_str(), trgb.data(), W, H) != 0;
                }
                if (bad) { fprintf(stderr, "cannot write %s%s*.pfm\n", out.c_str(), tag); return 1; }
            }
            printf("%u frames of %u spp, %g degrees per frame%s%s -> %s_fNNN%s.pfm\n", frames, spp, orbit_deg, temporal ? ", temporal" : "",
                   temporal && denoise ? " + a-trous" : "", out.c_str(), temporal ? "[_temporal]" : "");
            return 0;
        }
        PrtAdaptiveInfo ainfo{};
        if (frames > 1) {  // warm-up frame (first-touch allocations, clocks), then the timed ones
            r.Render(spp);
            r.Clear();
        }
        const PrtStats st0 = r.Stats();
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t f = 0; f < frames; ++f) {  // each call ends with the gather to the first device
            if (adaptive) ainfo = r.RenderAdaptive(ad);
            else r.Render(spp);
        }
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        r.Download();
        r.UpdateDisplay();
        const PrtStats st = r.Stats();
        std::vector<float> mean((size_t)W * H * 3);
        for (size_t i = 0; i < (size_t)W * H; ++i)
            for (int c = 0; c < 3; ++c) mean[3 * i + c] = film.weights[i] > 0 ? film.accum[3 * i + c] / film.weights[i] : 0.0f;
        if (prt_write_ppm((out + ".ppm").c_str(), film.display.data(), W, H) || prt_write_pfm((out + ".pfm").c_str(), mean.data(), W, H)) {
            fprintf(stderr, "cannot write %s.ppm/.pfm\n", out.c_str());
            return 1;
        }
        auto write_grey = [&](const std::string& path, const std::vector<float>& v) {
            std::vector<float> rgb((size_t)W * H * 3);
            for (size_t i = 0; i < (size_t)W * H; ++i) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = v[i];
            return prt_write_pfm(path.c_str(), rgb.data(), W, H);
        };
        if (!samples_out.empty() && write_grey(samples_out, film.weights)) { fprintf(stderr, "cannot write %s\n", samples_out.c_str()); return 1; }
        if (!noise_out.empty()) {
            std::vector<float> noise;
            r.NoiseMap(ad.noise_floor, noise);
            if (write_grey(noise_out, noise)) { fprintf(stderr, "cannot write %s\n", noise_out.c_str()); return 1; }
        }
        if (denoise) {
            std::vector<float> dmean;
            r.Denoise(&dn, dmean);
            // the preview: Film::UpdateDisplay's Reinhard + gamma 2.2 of the denoised mean (exposure 1), on the host
            std::vector<uint8_t> rgba((size_t)W * H * 4, 255);
            for (size_t i = 0; i < (size_t)W * H; ++i)
                for (int c = 0; c < 3; ++c) {
                    const float v = dmean[3 * i + c] > 0.0f ? dmean[3 * i + c] : 0.0f;
                    const float t = std::pow(v / (1.0f + v), 1.0f / 2.2f);
                    rgba[4 * i + c] = (uint8_t)((t < 1.0f ? t : 1.0f) * 255.0f + 0.5f);
                }
            if (prt_write_pfm((out + "_denoised.pfm").c_str(), dmean.data(), W, H) || prt_write_ppm((out + "_denoised.ppm").c_str(), rgba.data(), W, H)) {
                fprintf(stderr, "cannot write %s_denoised.pfm/.ppm\n", out.c_str());
                return 1;
            }
            printf("denoised: %u iterations, sigma_l %g, sigma_z %g, demodulate %u -> %s_denoised.pfm, %s_denoised.ppm\n", dn.iterations, dn.sigma_l,
                   dn.sigma_z, dn.demodulate, out.c_str(), out.c_str());
        }
        if (!features_out.empty()) {
            prt::HipWavefrontRenderer::Features ft;
            r.RenderFeatures(ft);
            if (prt_write_pfm((features_out + "_albedo.pfm").c_str(), ft.albedo.data(), W, H) ||
                prt_write_pfm((features_out + "_normal.pfm").c_str(), ft.normal.data(), W, H) ||
                prt_write_pfm((features_out + "_position.pfm").c_str(), ft.position.data(), W, H) ||
                write_grey(features_out + "_depth.pfm", ft.depth)) {
                fprintf(stderr, "cannot write %s_*.pfm\n", features_out.c_str());
                return 1;
            }
            if (ftrace.max_specular) {
                std::vector<uint32_t> bounces;
                r.RenderGuideFeatures(ft, bounces);
                const std::vector<float> fb(bounces.begin(), bounces.end());
                if (prt_write_pfm((features_out + "_guide_albedo.pfm").c_str(), ft.albedo.data(), W, H) ||
                    prt_write_pfm((features_out + "_guide_normal.pfm").c_str(), ft.normal.data(), W, H) ||
                    prt_write_pfm((features_out + "_guide_position.pfm").c_str(), ft.position.data(), W, H) ||
                    write_grey(features_out + "_guide_depth.pfm", ft.depth) || write_grey(features_out + "_guide_bounces.pfm", fb)) {
                    fprintf(stderr, "cannot write %s_guide_*.pfm\n", features_out.c_str());
                    return 1;
                }
            }
            if (feature_samples) {
                std::vector<uint32_t> hits;
                r.RenderSampledFeatures(ft, hits);
                const std::vector<float> fh(hits.begin(), hits.end());
                if (prt_write_pfm((features_out + "_sampled_albedo.pfm").c_str(), ft.albedo.data(), W, H) ||
                    prt_write_pfm((features_out + "_sampled_normal.pfm").c_str(), ft.normal.data(), W, H) ||
                    prt_write_pfm((features_out + "_sampled_position.pfm").c_str(), ft.position.data(), W, H) ||
                    write_grey(features_out + "_sampled_depth.pfm", ft.depth) || write_grey(features_out + "_sampled_hits.pfm", fh)) {
                    fprintf(stderr, "cannot write %s_sampled_*.pfm\n", features_out.c_str());
                    return 1;
                }
            }
        }
        if (adaptive)
            printf("adaptive (last frame): threshold %g, %u..%u spp in steps of %u: %u passes, %llu pixel-samples, %u tiles: %u converged, %u at the cap, %u..%u spp per tile\n",
                   ad.threshold, ad.min_spp, ad.max_spp, ad.step_spp, ainfo.passes, (unsigned long long)ainfo.pixel_samples, ainfo.tiles_local,
                   ainfo.tiles_converged, ainfo.tiles_capped, ainfo.min_tile_spp, ainfo.max_tile_spp);
        printf("%ux%u, %u spp, max_depth %u, %u GPU(s) [gather: %s]: %llu rays in %.3f s = %.1f Mrays/s -> %s.ppm, %s.pfm\n", W, H,
               (adaptive ? ad.max_spp : spp) * frames, depth, r.DeviceCount(), r.Transport(), (unsigned long long)(st.rays_total - st0.rays_total), s,
               (st.rays_total - st0.rays_total) / s / 1e6,
               out.c_str(), out.c_str());
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

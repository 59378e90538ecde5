// prt_api.cpp — implementation of the C-ABI in include/prt.h on top of the HIP kernels.
//
// Host-side mirror of what the reference's CudaWavefrontRenderer does around its kernels
// (src/backend/cuda_wavefront/renderer.cu:351-547: Init / ProgressiveRender / SetCamera / Allocate*),
// re-designed: flat SoA scene upload in one piece (no per-object cudaMalloc, soa.cpp:60-61,86-87),
// dense double-buffered ray records, device-side counters (no 1-thread reset kernels,
// renderer.cu:399-414), no host synchronisation inside a sample.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../include/prt.h"
#include "bvh.h"
#include "bvh_gpu.h"
#include "prt_adaptive.h"
#include "prt_denoise.h"
#include "prt_denoise_contract.h"
#include "prt_devmem.h"
#include "prt_feature_samples.h"
#include "prt_features.h"
#include "prt_kernels.h"
#include "prt_primary_cache.h"
#include "prt_radiance.h"
#include "prt_radiance_lit.h"
#include "prt_bake.h"
#include "prt_bake_light.h"
#include "prt_bake_adaptive.h"
#include "prt_bake_adaptive_contract.h"
#include "prt_probe_sh.h"
#include "prt_sh_contract.h"
#include "prt_scene.h"
#include "prt_temporal.h"
#include "prt_temporal_contract.h"
#include "prt_workspace.h"

// ---- the seam of prt_devmem.h over HIP, and the process-wide books prt_device_memory_info reads.  These definitions are the
// only place in this file that allocates or frees device memory, pinned memory or events. ----
static std::atomic<uint64_t> g_live_bytes{0}, g_alloc_calls{0};

int prt_dev_alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) g_live_bytes += bytes, ++g_alloc_calls;
    return (int)e;
}
void prt_dev_free(void* p, size_t bytes) {
    (void)hipFree(p);
    g_live_bytes -= bytes;
}
int prt_dev_copy_in(void* dst, const void* src, size_t bytes) { return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
void prt_dev_adopted(size_t bytes) { g_live_bytes += bytes; }
void prt_dev_taken(size_t bytes) { g_live_bytes -= bytes; }
int prt_pinned_alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
void prt_pinned_free(void* p) { (void)hipHostFree(p); }
int prt_event_create(void** ev, bool timing) {
    return (int)(timing ? hipEventCreate((hipEvent_t*)ev) : hipEventCreateWithFlags((hipEvent_t*)ev, hipEventDisableTiming));
}
void prt_event_destroy(void* ev) { (void)hipEventDestroy((hipEvent_t)ev); }

namespace {

constexpr float kPadCoeff = 1.0f / 262144.0f;  // 2^-18, see traverse() in prt_kernels.hip
constexpr size_t kRayStatWords = (size_t)PRT_RAY_STAT_SLOTS * PRT_MAX_DEPTH;
constexpr uint32_t kTravStatsWords = 16 + PRT_TIMELINE_WORDS * (PRT_MAX_DEPTH + 1);  // counters + one launch timeline per bounce
constexpr size_t kLightStatWords = 2 * (size_t)PRT_RAY_STAT_SLOTS;  // k_light_accum's [slot][shadow rays, occluded]

struct EventPair {
    DevEvent a, b;
    int kind = 0;  // 0 raygen, 1 intersect (dominant kernel), 2 shade, 3 accumulate, 4 analytic-primitive scan
};

hipEvent_t ev(const DevEvent& e) { return (hipEvent_t)e.h; }

// ---- what a context owns on the device, grouped by lifetime (prt_devmem.h): a group is reset by assigning a fresh value ----
struct RayMem {  // the arrays of one PrtRayBuf
    DevBuf o, d, t, hit, hd2;
    int alloc(uint64_t n) {
        int e = o.ensure(n * sizeof(float4));
        if (!e) e = d.ensure(n * sizeof(float4));
        if (!e) e = t.ensure(n * sizeof(float4));
        if (!e) e = hit.ensure(n * sizeof(uint32_t));
        if (!e) e = hd2.ensure(n * sizeof(float));
        return e;
    }
    PrtRayBuf view() const { return PrtRayBuf{o.as<float4>(), d.as<float4>(), t.as<float4>(), hit.as<uint32_t>(), hd2.as<float>()}; }
};
struct BuiltTree {  // the world meshes' tree as the device-side builder left it (PrtGpuBvh's arrays, adopted)
    DevBuf nodes8, tris, nrms;
    uint32_t n_nodes = 0;
};
struct SceneMem {  // prt_set_scene .. the next one
    DevBuf prims, mat_rgbs, mat_type, nodes, nodes4, nodes8, insts, tlas_inst, abvh_nodes, abvh_order, tris, nrms, lights, prim_light;
    DevBuf refit_keep;  // what prt_refit_meshes_device keeps with the scene (RefitKeep's arrays)
};
struct MeshLightMem {  // PrtMeshLights and PrtLightClusters (prt_scene.h), on the device only while the MESH bit is set
    DevBuf records, thr, bucket, runs;
    DevBuf lc_boxes, lc_range, lc_members, lc_thr, lc_cand, lc_pmf;  // lc_pmf, per candidate: fl32(pmf_in (2^32 - T_e) / 2^32)
};
struct EnvMem {
    DevBuf texels, row, col, last;
};
struct TexMem {
    DevBuf texels, desc, mat, uvs, inst;
};
struct PathMem {  // cap_paths paths
    RayMem rays[2];
    DevBuf rad;
};
struct LightMem {  // cap_light paths: shadow rays, pdf of the previous scatter, light radiance
    RayMem sh;
    DevBuf pdf_b, lrad;
};
struct PrimaryMem {  // the persistent primary stage (prt_primary_cache.h)
    DevBuf pid, list, hit;
};
struct FilmMem {
    DevBuf local;     // float4 per local pixel
    DevBuf stat;      // float2 {A, Q} per local pixel, only while film statistics are on
    DevBuf tile_sel;  // [0] the active count, then flags / list A / list B of tile_sel_entries tiles each
    PinnedBuf tile_count;  // the active count of a pass
};
struct WorkMem {  // counters and work arrays, allocated once (ensure_counters) or grown on demand
    DevBuf counts;       // (PRT_MAX_DEPTH + 2) x PRT_CNT_STRIDE: front/back ray counts per bounce
    DevBuf ray_stats;    // [2][PRT_RAY_STAT_SLOTS][PRT_MAX_DEPTH]: the context's counters, then a scratch set for measurement runs
    DevBuf trav_stats;
    DevBuf work;         // chunk cursors of the persistent traversal kernel, flags, overflow list
    DevBuf pix;          // compact primary rays: one record per local pixel (PrtPrimary)
    DevBuf sort;         // keys, keys2, idx, idx2 (n_paths each) + rocPRIM's temporary storage
    DevBuf light_stats;  // [slot][shadow rays, occluded], since prt_reset_stats
    PinnedBuf flag;      // the traversal kernels' error flags (work[256]) as of the last prt_synchronize
    PinnedBuf counts_host;  // the front / back ray counts of each bounce as the host learns them
    DevEvent ev_counts[PRT_MAX_DEPTH + 2];
    DevEvent ev_prod[PRT_MAX_DEPTH + 2];  // "the producer of bounce d's counts is done" (render stream -> count stream)
};

}  // namespace

struct PrtContext {
    int device = -1;
    bool has_device = false;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;

    // ---- scene ----
    bool has_scene = false;
    PrtHostScene hs;                   // the compiled scene (prt_scene.h): every host array the device copies come from
    double refit_ms = 0.0;             // device time of the last prt_refit_meshes (records + boxes + quantization)
    // refit from device arrays (prt_refit_meshes_device): what the scene keeps on the device after the first call (one
    // allocation, laid out by prt_workspace.h), and whether hs.bvh.nodes8 / tri_records / nrm_records lag behind the device
    struct RefitKeep {
        bool ready = false;
        std::vector<uint32_t> tri_first, vert_first, level_start;  // PrtRefitTables' small arrays
        uint32_t n_nodes = 0, n_light_tris = 0;
        uint32_t *d_corner = nullptr, *d_csr_start = nullptr, *d_csr_corner = nullptr, *d_light_tris = nullptr, *d_valid = nullptr;
        float *d_normals = nullptr, *d_light_verts = nullptr;  // computed normals of every world-space vertex; the packed emissive triangles
        PrtRefitScratch scratch{};
    } rk;
    bool host_copies_stale = false;
    PrtRefitInfo rinfo{};              // of the last refit, either form (refits: from hs.bvh_info)
    PrtCopyTally* tally = nullptr;     // while a refit runs: the copies of the helpers it calls are counted here
    PrtInstanceUpdateInfo inst_info{}; // prt_set_instance_transforms calls since the scene was set (top_nodes / top_depth: from hs)
    DevScene dsc{};  // the kernels' view of `scene` (fill_dev_scene)
    SceneMem scene;

    // ---- camera ----
    bool has_camera = false;
    DevCamera cam{};

    // ---- film / partition ----
    bool has_film = false;
    PrtTileMap tm{};
    uint32_t valid_local = 0;  // pixels of this rank inside the image
    // film statistics (prt_set_film_statistics, include/prt.h "Film statistics and adaptive sampling"): {A, Q} per local pixel
    // beside film.local, allocated only while they are on; the tile flags and the two tile lists of prt_render_adaptive
    FilmMem film;
    bool film_stats = false;
    uint32_t tile_sel_entries = 0;

    // ---- path state ----
    uint32_t S = 1;
    uint64_t cap_paths = 0;
    PathMem path;
    PrtRayBuf rb[2] = {{nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr}};  // views of path.rays
    WorkMem wk;
    unsigned long long* ray_stats_target = nullptr;  // the set k_accumulate adds to (wk.ray_stats, or its scratch half during a measurement)
    bool pix_records_blank = false;  // wk.pix's primary-hit records all say "no record" (batches of one sample)

    // ---- scratch for the function-level entry points ----
    DevBuf scratch;

    // ---- stats ----
    bool timing = false;
    std::vector<EventPair> events;
    std::vector<EventPair> event_pool;
    PrtStats stats{};
    uint64_t dead_paths = 0;
    int variant = 0;
    int abvh_enabled = 1;  // prt_set_param("prim_bvh", 0): keep the reference's linear scan over the analytic primitives
    int measure_spp = 1;  // samples of the instrumented batch of prt_measure_traversal
    float pad_coeff = kPadCoeff;  // prt_set_param("pad_log2", n): culling pad = 2^-n of the coordinates' magnitude (A/B; before prt_set_scene)
    int node_stride = 0;      // prt_set_param("node_stride", 5 | 8): uint4 per 8-wide node slot, 0 = by tree size (upload_scene); before prt_set_scene
    int compact_primary = 1;  // prt_set_param("compact_primary", 0): k_raygen stores full ray records (A/B)
    int path_id_order = 1;    // prt_set_param("path_id_order", 0): every batch numbers its paths sample-major (prt_path_id.h; A/B)
    int primary_walk = 1;     // prt_set_param("primary_walk", 0): compact primary rays are walked once per sample, not once per pixel (A/B)
    const char* shade_instance = "";  // the shade kernel instance the last run_batch launched, as its launch macro spelled it (prt_shade_instance)
    const char* batch_instance[4] = {"", "", "", ""};  // what the last run_batch launched, by PRT_STAGE_* (prt_batch_instance)
    bool batch_walked = false;  // the last run_batch took the one-walk-per-pixel route (prt_measure_traversal counts its list)
    int gpu_build = 0;  // prt_set_param("gpu_build", 1): the next prt_set_scene builds the 8-wide tree on the device
    PrtSampling sampling{0u, 0u, 0.0f};
    PrtLens lens{0.0f, 0.0f, 0.0f};  // prt_set_lens: a property of the context, kept across camera / scene / film
    // grid 256 CUs x 4 blocks, 256-ray chunks, refill at 16 idle lanes, leave the node loop at <= 16 walkers, triangle
    // phase after 24 queueing lane-steps, 8-wide tree (all measured best on C3, tools/sweep.py); XCD affinity off
    PrtTravTuning tune{1024u, 256u, 16u, 0xFFFFFFFFu /* exit_max: auto */, 0u, 2u, 0u /* tri_min: auto */, 0u, 0u, 0u, 1u, 8u, 1u, 0u, nullptr, 0u, 2500000u, 2u /* big */, 8u /* static_small */, 96u /* big_min */, 32u /* big_keep */, 1u};
    unsigned long long* d_shade_div = nullptr;  // diagnostic (prt_measure_shade_divergence): 16 words per bounce, or null
    uint32_t last_segment = 2;    // a path's last segment (prt_route.h): 1 = it ends in its producer where the analytic scan decides it, 2 = and the rest is walked any-hit; 0 / 1: A/B
    uint32_t last_segment_active = 0;  // what the last run_batch's plan made of it (prt_last_segment)
    uint32_t last_batch_depth = 0;     // max_depth of the last run_batch that ran the pipeline (0: none, or the path route)
    uint32_t sort_rays = 0;       // measurement aid: 1 / 2 = bounces >= 1 (and jittered bounce 0) walk their rays in sorted order
    size_t sort_entries = 0, sort_temp = 0;
    hipStream_t count_stream = nullptr;          // the counts' copies to the host run beside the render stream, not in it
    uint32_t pix_entries = 0;
    // ---- the primary stage of a still camera, kept across batches and calls (prt_primary_cache.h) ----
    // What k_raygen, the bounce-0 walk and k_primary_hit leave behind on the compact route, besides wk.pix and bounce 0's words
    // of wk.counts: the path-id list (4 B per path; in rb[0].t it would be overwritten by bounce 2's rays), the front-pixel list
    // and the walk's hits (4 B per local pixel each; in rb[0].hd2 / .hit likewise).  Nothing after the first k_shade writes them.
    PrimaryMem prim;
    uint64_t prim_pid_entries = 0;
    uint32_t prim_pix_entries = 0;
    PrtPrimaryStageKey primary_key{};   // what the buffers hold (batch.valid = false: nothing)
    uint64_t camera_gen = 1, scene_gen = 1;  // PrtPrimaryKey: bumped by every setter that can change what the stage computes
    uint32_t primary_counts[2] = {0u, 0u};   // bounce 0's front / back ray counts as the host read them at the refresh (exact grids)
    int primary_reuse = 1;              // prt_set_param("primary_reuse", 0): every batch rebuilds its primary stage (A/B)
    uint32_t primary_reuse_active = 0;  // the last run_batch started at its first k_shade (prt_primary_reuse)
    uint32_t primary_reused_batches = 0;  // batches that did, since the context was created
    DevBuf spill;                 // global part of the per-lane traversal stacks (uint32_t entries)

    // ---- light sampling (PrtLighting, include/prt.h) ----
    uint32_t lighting = PRT_LIGHTING_OFF;
    uint32_t light_sources = PRT_LIGHT_SOURCES_ANALYTIC;  // prt_set_light_sources
    uint32_t light_selection = PRT_LIGHT_SELECTION_POWER;  // prt_set_light_selection (PrtLightSelection.mode)
    uint32_t light_max_clusters = 0;   // PrtLightSelection.max_clusters as given (0: the default)
    int light_buckets = 1;             // the bucket table brackets the search over the thresholds (0: plain binary search; A/B)
    MeshLightMem ml;
    LightMem light;
    PrtLightBufs lb{};                 // the kernels' view of `light` and wk.light_stats
    uint64_t cap_light = 0;

    // ---- environment light (PrtEnvironment, include/prt.h): a property of the context, kept across scenes ----
    PrtEnvTables env;                  // W = 0: the constant sky
    EnvMem envm;
    uint64_t t_env_dev = 0;            // the T_e the pmfs of the light tables on the device are scaled with

    // ---- image textures (PrtTextureSet, include/prt.h): a property of the current scene ----
    PrtTexTables tex;                  // is_set = false: no binding
    TexMem texm;
    uint64_t tex_bytes = 0;            // device bytes of the binding

    // ---- first-hit features and the film denoiser (include/prt.h): the records of prt_render_features, valid until a call
    // that changes what the centre rays see; the filter's workspace (packed records of the array entry points, the two
    // colour + variance buffers, staging for host arrays) ----
    DevBuf feat;                                     // 3 x feat_W x feat_H float4 (feature_view)
    uint32_t feat_W = 0, feat_H = 0;
    bool feat_valid = false;
    // the guide set through specular chains (PrtFeatureTrace): written beside the first-hit set while max_specular > 0,
    // current only while feat_valid is (every site that drops the one drops the other)
    PrtFeatureTrace ftrace{0u, 0.1f};                // prt_set_feature_trace: a property of the context, like the lens
    DevBuf guide;
    bool guide_valid = false;
    // the sampled set (PrtFeatureSampling): written beside the others while samples > 0, current only while feat_valid is
    PrtFeatureSampling fsamp{0u, 0u, 0u};            // prt_set_feature_sampling: a property of the context, like ftrace
    DevBuf samp;                                     // the running sums until finished
    bool samp_valid = false;
    int feature_chunk = 0;  // prt_set_param("feature_chunk", n): samples per chunk of the sampled pass, 0 = by the ray budget
    int radiance_chunk = 0;  // prt_set_param("radiance_chunk", n): samples per chunk of the radiance query, 0 = by the ray budget
    int bake_chunk = 0;      // prt_set_param("bake_chunk", n): samples per chunk of a bake, 0 = by the ray budget of radiance_chunk
    int probe_chunk = 0;     // prt_set_param("probe_chunk", n): samples per chunk of prt_probe_sh, 0 = by the ray budget of radiance_chunk
    DevBuf bake;             // the faces and the map of a bake (prt_bake.h); its rays and the query's lists are in scratch
    DevBuf dn;
    // ---- temporal reprojection (include/prt.h): two history sets that ping-pong, the blended planar frame, status and
    // counters in one allocation; the basis and the placed copies' matrices of the step that wrote the history ----
    DevBuf tp;
    DevBuf tp_mt;                      // the motion table of a step (PrtMotionTable)
    DevBuf tpa;                        // workspace of the array entry points
    uint32_t tp_W = 0, tp_H = 0;
    int tp_set = 0;                    // which set holds the history
    bool tp_valid = false;
    PrtCameraBasis tp_K{};
    std::vector<float> tp_mats;        // 12 floats per placed copy
    std::vector<uint32_t> tp_mt_host;  // staging of the motion table
    PrtTemporalInfo tp_info{};
    int dn_lds = 1;  // prt_set_param("denoise_lds", n): which iterations stage their block's footprint in LDS: 0 none, 1 step 1 (default: measured faster there, slower at step 2), 2 steps 1 and 2; the same bits
};

namespace {

int fail(PrtContext* c, int code, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

// (call: a hipError_t, or the same code as the int an owner of prt_devmem.h returns)
#define HIPCHECK(c, call)                                                                              \
    do {                                                                                               \
        const hipError_t e_ = (hipError_t)(call);                                                      \
        if (e_ != hipSuccess) return fail((c), PRT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

int need_device(PrtContext* c) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_device)
        return fail(c, PRT_ERR_NO_DEVICE,
                    "no HIP device bound to this context: the MI355X kernels are the only compute path (no CPU fallback)");
    // every device entry point starts here: make the context's GPU the calling thread's current device (a process may
    // hold contexts on several GPUs, each driven from its own host thread: prt_group_*)
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(c, PRT_ERR_HIP, "hipSetDevice(%d) failed: %s", c->device, hipGetErrorString(e));
    return PRT_OK;
}

void drop_history(PrtContext* c) {
    c->tp_valid = false;
    c->tp_info.steps = 0;
    c->tp_info.hit_pixels = 0;
    c->tp_info.reprojected = 0;
    ++c->tp_info.resets;
}

int ensure(PrtContext* c, DevBuf& buf, size_t need) {
    HIPCHECK(c, buf.ensure(need));
    return PRT_OK;
}

// Grows buf to the size of a layout (prt_workspace.h) and hands out the pointers the layout declared, inside buf.
int commit(PrtContext* c, const PrtWorkspace& ws, DevBuf& buf) {
    const int rc = ensure(c, buf, ws.bytes());
    if (rc || ws.bind(buf.p, buf.bytes)) return rc;
    return fail(c, PRT_ERR_INVALID, "a workspace of %d arrays in %zu bytes does not fit its buffer of %zu", ws.regions(), ws.bytes(), buf.bytes);
}

// count elements host -> device / device -> host, asynchronously on the context's stream
template <class T>
int upload(PrtContext* c, T* dst, const T* src, size_t count) {
    HIPCHECK(c, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return PRT_OK;
}
template <class T>
int download(PrtContext* c, T* dst, const T* src, size_t count) {
    HIPCHECK(c, hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return PRT_OK;
}

// A feature set of n pixels in one array of 3 n records: albedo, normal, position.
PrtFeatureBufs feature_view(void* base, size_t n) {
    float4* a = (float4*)base;
    return PrtFeatureBufs{a, a + n, a + 2 * n};
}

// ---- the layouts several entry points share ----
// What enqueue_chains needs beside its arguments for up to n rays: a second ray list, two state lists of two float4 each,
// and one live count per round.  A caller declares it behind its own arrays, in the same layout.
struct ChainScratch {
    float *o, *d;
    float4* s[4];
    uint32_t* cnt;
    void declare(PrtWorkspace& ws, size_t n) {
        ws.add(&o, 3 * n).add(&d, 3 * n);
        for (float4*& p : s) ws.add(&p, n);
        ws.add(&cnt, PRT_FEATURE_MAX_SPECULAR + 1u);
    }
};

// The filter's workspace for n pixels: the two colour + variance buffers; for the array entry points the packed records
// (a feature set) before them, for the film's forms the planar outputs behind them.
struct FilterScratch {
    float4 *rec = nullptr, *cv0 = nullptr, *cv1 = nullptr;
    float *out = nullptr, *var = nullptr;
    void declare_arrays(PrtWorkspace& ws, size_t n) { ws.add(&rec, 3 * n).add(&cv0, n).add(&cv1, n); }
    int commit_film(PrtContext* c, size_t n) {
        PrtWorkspace ws;
        ws.add(&cv0, n).add(&cv1, n).add(&out, 3 * n).add(&var, n);
        return commit(c, ws, c->dn);
    }
};

// A history set of n pixels: cn, nrm, pos and mm, one array each
void declare_history(PrtWorkspace& ws, PrtHistoryBufs* h, size_t n) { ws.add(&h->cn, n).add(&h->nrm, n).add(&h->pos, n).add(&h->mm, n); }

// The array entry points' records of n pixels: the current frame's, the history's, the new cn / mm
struct TemporalScratch {
    PrtHistoryBufs cur, prev, next;
    void declare(PrtWorkspace& ws, size_t n) {
        declare_history(ws, &cur, n);
        declare_history(ws, &prev, n);
        next.nrm = next.pos = nullptr;
        ws.add(&next.cn, n).add(&next.mm, n);
    }
};

int ensure_path_state(PrtContext* c, uint64_t n_paths) {
    if (n_paths <= c->cap_paths) return PRT_OK;
    c->path = PathMem();
    c->cap_paths = 0;
    const uint64_t n = std::max<uint64_t>(n_paths, 256);
    int e = c->path.rays[0].alloc(n);
    if (!e) e = c->path.rays[1].alloc(n);
    if (!e) e = c->path.rad.ensure(n * sizeof(float4));
    for (int i = 0; i < 2; ++i) c->rb[i] = c->path.rays[i].view();
    HIPCHECK(c, e);
    c->cap_paths = n;
    return PRT_OK;
}

// A setter changed what a batch's primary stage computes from (PrtPrimaryKey, prt_primary_cache.h).
void touch_scene(PrtContext* c) { ++c->scene_gen; }
void touch_camera(PrtContext* c) { ++c->camera_gen; }

// The persistent primary buffers of the compact route (sized with the path state; they only grow, and growing drops what they held)
int ensure_primary_state(PrtContext* c, uint64_t n_paths, uint32_t n_pix_local) {
    if (n_paths > c->prim_pid_entries) {
        c->primary_key.batch.valid = false;
        c->prim_pid_entries = 0;  // (a growing ensure releases before it allocates, and a failed one leaves nothing)
        const uint64_t n = std::max<uint64_t>(n_paths, 256);
        HIPCHECK(c, c->prim.pid.ensure(n * sizeof(uint32_t)));
        c->prim_pid_entries = n;
    }
    if (n_pix_local > c->prim_pix_entries) {
        c->primary_key.batch.valid = false;
        c->prim_pix_entries = 0;
        const uint32_t n = std::max<uint32_t>(n_pix_local, 256u);
        HIPCHECK(c, c->prim.list.ensure((size_t)n * sizeof(uint32_t)));
        HIPCHECK(c, c->prim.hit.ensure((size_t)n * sizeof(uint32_t)));
        c->prim_pix_entries = n;
    }
    return PRT_OK;
}

// the lighting pipeline's per-path buffers (sized with the path state; the statistics words once)
int ensure_light_state(PrtContext* c, uint64_t n_paths) {
    if (!c->wk.light_stats.p) {
        HIPCHECK(c, c->wk.light_stats.ensure(kLightStatWords * sizeof(unsigned long long)));
        // on the context's stream: a hipMemset of device memory on the null stream may return before it has run and is not
        // ordered against the (non-blocking) render stream, so the first batch's counts could be zeroed after they were
        // added (seen with the three contexts of a group on one GPU: one rank's first sample missing from the shadow rays)
        HIPCHECK(c, hipMemsetAsync(c->wk.light_stats.p, 0, kLightStatWords * sizeof(unsigned long long), c->stream));
    }
    c->lb.stats = c->wk.light_stats.as<unsigned long long>();
    if (n_paths <= c->cap_light) return PRT_OK;
    c->light = LightMem();
    c->cap_light = 0;
    const uint64_t n = std::max<uint64_t>(n_paths, 256);
    int e = c->light.sh.alloc(n);
    if (!e) e = c->light.pdf_b.ensure(n * sizeof(float));
    if (!e) e = c->light.lrad.ensure(n * sizeof(float4));
    c->lb.sh = c->light.sh.view();
    c->lb.pdf_b = c->light.pdf_b.as<float>();
    c->lb.lrad = c->light.lrad.as<float4>();
    HIPCHECK(c, e);
    c->cap_light = n;
    return PRT_OK;
}

bool mesh_lights_on(const PrtContext* c) { return (c->light_sources & PRT_LIGHT_SOURCES_MESH) != 0u; }

// with the MESH bit: the candidate table, n_lights = the candidates the search can return (0: nothing to sample)
DevLights dev_lights(const PrtContext* c) {
    const uint32_t mode = c->lighting == PRT_LIGHTING_NEE ? (uint32_t)PRT_LIGHTING_NEE : (uint32_t)PRT_LIGHTING_NEE_MIS;
    if (mesh_lights_on(c)) return DevLights{c->ml.records.as<float4>(), c->scene.prim_light.as<uint32_t>(), c->hs.ml.n_search, mode};
    return DevLights{c->scene.lights.as<float4>(), c->scene.prim_light.as<uint32_t>(), (uint32_t)(c->hs.lights.size() / (4 * PRT_LIGHT_F4)), mode};
}

DevMeshLights dev_mesh_lights(const PrtContext* c) {
    return DevMeshLights{c->ml.thr.as<uint32_t>(), c->light_buckets ? c->ml.bucket.as<uint32_t>() : nullptr,
                         c->ml.runs.as<DevLightRun>(), c->hs.ml.bucket_shift, (uint32_t)c->hs.ml.runs.size()};
}

// clustered selection takes effect only while the integer rule selects lights
bool clusters_on(const PrtContext* c) { return mesh_lights_on(c) && c->light_selection == (uint32_t)PRT_LIGHT_SELECTION_CLUSTERED; }

DevLightClusters dev_light_clusters(const PrtContext* c) {
    const MeshLightMem& m = c->ml;
    return DevLightClusters{m.lc_boxes.as<float4>(), m.lc_range.as<uint4>(), m.lc_members.as<uint32_t>(),
                            m.lc_thr.as<uint32_t>(), m.lc_cand.as<uint32_t>(), m.lc_pmf.as<float>(), c->hs.lc.n_clusters()};
}

uint32_t light_set_size(const PrtContext* c) {
    return mesh_lights_on(c) ? (uint32_t)c->hs.ml.visible.size() : (uint32_t)(c->hs.lights.size() / (4 * PRT_LIGHT_F4));
}

// ---- environment light ----
bool env_on(const PrtContext* c) { return c->env.W != 0u; }
// T_e for the current scene and light source mask (no scene: an empty light set)
uint64_t env_threshold(const PrtContext* c) { return prt_environment_threshold(c->env, light_set_size(c)); }

DevEnv dev_env(const PrtContext* c) {
    const uint64_t te = env_threshold(c);
    return DevEnv{c->envm.texels.as<float4>(), c->envm.row.as<uint32_t>(), c->envm.col.as<uint32_t>(),
                  c->envm.last.as<uint32_t>(), c->env.W, c->env.H, c->env.row_last, (uint32_t)te, te == 4294967296ull ? 1u : 0u,
                  (float)((double)te / 4294967296.0)};
}

// c->env onto the device (prt_set_environment, prt_clone_scene)
int upload_env(PrtContext* c) {
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    c->envm = EnvMem();
    if (!env_on(c)) return PRT_OK;
    HIPCHECK(c, c->envm.texels.alloc_copy(c->env.texels.data(), c->env.texels.size() * 4));
    HIPCHECK(c, c->envm.row.alloc_copy(c->env.row_thr.data(), c->env.row_thr.size() * 4));
    HIPCHECK(c, c->envm.col.alloc_copy(c->env.col_thr.data(), c->env.col_thr.size() * 4));
    HIPCHECK(c, c->envm.last.alloc_copy(c->env.col_last.data(), c->env.col_last.size() * 4));
    return PRT_OK;
}

// ---- image textures ----
// true: the binding changes what a batch computes (and the route it takes)
bool tex_on(const PrtContext* c) { return c->tex.is_set && c->tex.n_textured_materials != 0u; }

DevTex dev_tex(const PrtContext* c) {
    return DevTex{c->texm.texels.as<float4>(), c->texm.desc.as<uint4>(), c->texm.mat.as<uint32_t>(), c->texm.uvs.as<float2>(),
                  c->texm.inst.as<uint32_t>(), c->tex.n_textures};
}

void free_tex(PrtContext* c) {
    c->texm = TexMem();
    c->tex_bytes = 0;
}

// c->tex onto the device (prt_set_textures, prt_clone_scene); waits for the context's stream
int upload_tex(PrtContext* c) {
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    free_tex(c);
    if (!c->tex.is_set) return PRT_OK;
    auto up = [&](DevBuf& dst, const auto& src) {  // (every table has 4-byte elements)
        const int e = dst.alloc_copy(src.data(), src.size() * 4);
        if (!e) c->tex_bytes += src.size() * 4;
        return e;
    };
    const PrtTexTables& t = c->tex;
    HIPCHECK(c, up(c->texm.texels, t.texels));
    HIPCHECK(c, up(c->texm.desc, t.desc));
    HIPCHECK(c, up(c->texm.mat, t.mat_tex));
    HIPCHECK(c, up(c->texm.uvs, t.uvs));
    HIPCHECK(c, up(c->texm.inst, t.inst_uv_base));
    return PRT_OK;
}

// prt_set_scene: the binding goes with the scene it was made for
void drop_tex(PrtContext* c) {
    if (c->has_device && c->texm.texels.p) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        free_tex(c);
    }
    c->tex = PrtTexTables();
}

// The pmfs of the light tables on the device carry the factor (2^32 - T_e) / 2^32 (include/prt.h "Environment light"):
// rewrites both tables in place from the host copies when T_e is not what they were scaled with.
int sync_light_tables(PrtContext* c) {
    const uint64_t te = env_threshold(c);
    if (te == c->t_env_dev || !c->has_device) return PRT_OK;
    std::vector<float> a, b;
    const bool ml = mesh_lights_on(c) && c->ml.records.p;
    prt_scaled_light_tables(c->hs, te, &a, ml ? &b : nullptr);
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if (!a.empty() && c->scene.lights.p) HIPCHECK(c, hipMemcpy(c->scene.lights.p, a.data(), a.size() * 4, hipMemcpyHostToDevice));
    if (!a.empty() && c->scene.lights.p && c->tally) c->tally->h2d += a.size() * 4;
    if (ml && !b.empty()) HIPCHECK(c, hipMemcpy(c->ml.records.p, b.data(), b.size() * 4, hipMemcpyHostToDevice));
    if (ml && !b.empty() && c->tally) c->tally->h2d += b.size() * 4;
    if (ml && c->ml.lc_pmf.p) {
        prt_cluster_pmf_in(c->hs, te, &a);
        if (!a.empty()) HIPCHECK(c, hipMemcpy(c->ml.lc_pmf.p, a.data(), a.size() * 4, hipMemcpyHostToDevice));
        if (!a.empty() && c->tally) c->tally->h2d += a.size() * 4;
    }
    c->t_env_dev = te;
    return PRT_OK;
}

// the candidate table of the current scene onto the device (prt_set_light_sources, upload_scene, prt_refit_meshes)
int upload_mesh_lights(PrtContext* c) {
    static_assert(sizeof(DevLightRun) == sizeof(PrtLightRun), "DevLightRun is PrtLightRun");
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    c->ml = MeshLightMem();
    const PrtMeshLights& ml = c->hs.ml;
    auto up = [&](DevBuf& dst, const void* src, size_t bytes) {
        const int e = dst.alloc_copy(src, bytes);
        if (!e && c->tally) c->tally->h2d += bytes;
        return e;
    };
    HIPCHECK(c, up(c->ml.records, ml.records.data(), ml.records.size() * 4));
    HIPCHECK(c, up(c->ml.thr, ml.thr.data(), ml.thr.size() * 4));
    HIPCHECK(c, up(c->ml.bucket, ml.bucket.data(), ml.bucket.size() * 4));
    HIPCHECK(c, up(c->ml.runs, ml.runs.data(), ml.runs.size() * sizeof(PrtLightRun)));
    const PrtLightClusters& lc = c->hs.lc;  // (12 bytes per candidate more; they go up whatever the selection mode)
    std::vector<float> pmf_in;
    prt_cluster_pmf_in(c->hs, 0u, &pmf_in);
    HIPCHECK(c, up(c->ml.lc_boxes, lc.boxes.data(), lc.boxes.size() * 4));
    HIPCHECK(c, up(c->ml.lc_range, lc.range.data(), lc.range.size() * 4));
    HIPCHECK(c, up(c->ml.lc_members, lc.members.data(), lc.members.size() * 4));
    HIPCHECK(c, up(c->ml.lc_thr, lc.thr.data(), lc.thr.size() * 4));
    HIPCHECK(c, up(c->ml.lc_cand, lc.cand_cluster.data(), lc.cand_cluster.size() * 4));
    HIPCHECK(c, up(c->ml.lc_pmf, pmf_in.data(), pmf_in.size() * 4));
    c->t_env_dev = c->t_env_dev ? ~0ull : 0ull;  // (the records went up unscaled: a scaled default table is rewritten with them)
    return sync_light_tables(c);
}

int ensure_counters(PrtContext* c) {
    WorkMem& w = c->wk;
    if (w.counts.p) return PRT_OK;
    HIPCHECK(c, w.counts.ensure((PRT_MAX_DEPTH + 2) * PRT_CNT_STRIDE * sizeof(uint32_t)));
    HIPCHECK(c, w.ray_stats.ensure(kRayStatWords * 2 * sizeof(unsigned long long)));
    c->ray_stats_target = w.ray_stats.as<unsigned long long>();
    HIPCHECK(c, w.trav_stats.ensure(kTravStatsWords * sizeof(unsigned long long)));
    HIPCHECK(c, hipMemset(w.counts.p, 0, w.counts.bytes));
    HIPCHECK(c, hipMemset(w.ray_stats.p, 0, w.ray_stats.bytes));
    HIPCHECK(c, hipMemset(w.trav_stats.p, 0, w.trav_stats.bytes));
    // [0..255] chunk cursors (one 128-B line per XCD), [256] watchdog flag, [512] overflow count, [513..] overflow list
    HIPCHECK(c, w.work.ensure((513 + (1u << 20)) * sizeof(uint32_t)));
    HIPCHECK(c, hipMemset(w.work.p, 0, w.work.bytes));
    return PRT_OK;
}

// global spill area of the traversal stacks: [prt_spill_rows of the scene's trees][grid threads]
int ensure_spill(PrtContext* c) {
    const size_t need = (size_t)c->tune.grid_blocks * 256u * prt_spill_rows(c->hs.bvh.max_stack4, c->hs.bvh.max_depth);
    return ensure(c, c->spill, need * sizeof(uint32_t));
}

// What prt_refit_meshes_device keeps with a scene goes with it
void drop_refit_keep(PrtContext* c) {
    c->scene.refit_keep = DevBuf();
    c->rk = PrtContext::RefitKeep();
    c->host_copies_stale = false;
    c->rinfo = PrtRefitInfo{};
}

// The host copies of the world-space meshes' tree and records after a refit from device arrays left them behind: every
// reader of hs.bvh.nodes8 / hs.tri_records / hs.nrm_records comes through here first.
int refresh_host_copies(PrtContext* c) {
    if (!c->host_copies_stale) return PRT_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    PrtHostScene& hs = c->hs;
    const size_t n_nodes = hs.bvh.nodes8.size() / 20, n_tris = c->dsc.n_tris;
    if (n_nodes) HIPCHECK(c, hipMemcpy2D(hs.bvh.nodes8.data(), 80, c->scene.nodes8.p, (size_t)c->dsc.node_stride * 16, 80, n_nodes, hipMemcpyDeviceToHost));
    if (hs.tri_records.size() == 12 * n_tris) HIPCHECK(c, hipMemcpy(hs.tri_records.data(), c->scene.tris.p, 48 * n_tris, hipMemcpyDeviceToHost));
    if (hs.nrm_records.size() == 12 * n_tris) HIPCHECK(c, hipMemcpy(hs.nrm_records.data(), c->scene.nrms.p, 48 * n_tris, hipMemcpyDeviceToHost));
    c->host_copies_stale = false;
    return PRT_OK;
}

void free_scene(PrtContext* c) {
    drop_refit_keep(c);
    c->scene = SceneMem();
    c->ml = MeshLightMem();
    c->has_scene = false;
}

// timing helpers ----------------------------------------------------------------------------------
// the per-depth ray counters of one set: the sum over its slots (prt_kernels.h PRT_RAY_STAT_SLOTS)
int read_ray_stats(PrtContext* c, const unsigned long long* d_set, unsigned long long (&out)[PRT_MAX_DEPTH]) {
    std::vector<unsigned long long> h(kRayStatWords);
    HIPCHECK(c, hipMemcpy(h.data(), d_set, kRayStatWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int d = 0; d < PRT_MAX_DEPTH; ++d) {
        out[d] = 0;
        for (size_t sl = 0; sl < PRT_RAY_STAT_SLOTS; ++sl) out[d] += h[sl * PRT_MAX_DEPTH + (size_t)d];
    }
    return PRT_OK;
}

int begin_event(PrtContext* c, int kind, EventPair* ep) {
    if (!c->timing) return PRT_OK;
    if (!c->event_pool.empty()) {
        *ep = std::move(c->event_pool.back());
        c->event_pool.pop_back();
    } else {
        HIPCHECK(c, ep->a.create(true));
        HIPCHECK(c, ep->b.create(true));
    }
    ep->kind = kind;
    HIPCHECK(c, hipEventRecord(ev(ep->a), c->stream));
    return PRT_OK;
}
int end_event(PrtContext* c, EventPair* ep) {
    if (!c->timing) return PRT_OK;
    HIPCHECK(c, hipEventRecord(ev(ep->b), c->stream));
    c->events.push_back(std::move(*ep));
    return PRT_OK;
}
int drain_events(PrtContext* c) {
    for (EventPair& ep : c->events) {
        float ms = 0.0f;
        HIPCHECK(c, hipEventSynchronize(ev(ep.b)));
        HIPCHECK(c, hipEventElapsedTime(&ms, ev(ep.a), ev(ep.b)));
        switch (ep.kind) {
            case 0: c->stats.raygen_ms += ms; break;
            case 1: c->stats.intersect_ms += ms; break;
            case 2: c->stats.shade_ms += ms; break;
            case 4: c->stats.scan_ms += ms; break;
            default: c->stats.accumulate_ms += ms; break;
        }
        c->event_pool.push_back(std::move(ep));
    }
    c->events.clear();
    return PRT_OK;
}

// PrtLens.fov_y -> DevCamera.tan_fov_y; 0 = the reference's 1 rad (src/core/camera.h:111)
float lens_tan_fov_y(const PrtLens& l) { return l.fov_y == 0.0f ? tanf(0.5f) : tanf(0.5f * l.fov_y); }

// glm-order helpers for the camera basis (Camera::Camera, src/core/camera.h:10-16)
f3 h_normalize(f3 v) {
    const float d = (v.x * v.x + v.y * v.y) + v.z * v.z;
    const float s = 1.0f / std::sqrt(d);
    return f3{v.x * s, v.y * s, v.z * s};
}
f3 h_cross(f3 a, f3 b) { return f3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }

// The whole film as a batch view (PrtBatchView, prt_kernels.h): the context's own tile map, no tile list.
PrtBatchView whole_film(const PrtContext* c) { return PrtBatchView{c->tm, nullptr}; }

// What the choice of a tree walk's kernel instances reads (PrtWalkFacts, prt_walk.h), from c->dsc (fill_dev_scene), the compiled
// scene's tree bounds and `tune` (the context's tunables, or a bounce's copy of them).
PrtWalkFacts walk_facts(const PrtContext* c, const PrtTravTuning& tune, PrtWalkRequest request, uint32_t max_rays, bool stats, bool primary) {
    PrtWalkFacts f{};
    f.has8 = c->dsc.nodes8 != nullptr, f.has4 = c->dsc.nodes4 != nullptr, f.has2 = c->dsc.nodes != nullptr;
    f.insts = c->dsc.n_insts != 0u, f.abvh = c->dsc.abvh_nodes != nullptr;
    f.depth8 = c->dsc.depth8, f.node_stride = c->dsc.node_stride, f.depth2 = c->hs.bvh.max_depth, f.max_stack4 = c->hs.bvh.max_stack4;
    f.wide = tune.wide, f.stack_lds = tune.stack_lds, f.stack_cap = tune.stack_cap, f.exit_max = tune.exit_max, f.tri_min = tune.tri_min;
    f.grid_blocks = tune.grid_blocks, f.steal = tune.steal, f.variant = c->variant, f.max_rays = max_rays, f.request = request, f.stats = stats, f.primary = primary;
    return f;
}

// The tree walk of a prepared ray buffer (analytic scan done, hit / hd2 seeded) on the context's stream: the closest hit, or
// with `any` the any-hit walk behind prt_occluded and the shadow rays (`seeded`: over a closest-hit walk's buffer, every ray
// walked).  Fill the facts, plan (prt_plan_walk, prt_walk.h), launch.
void walk_rays(PrtContext* c, const PrtRayBuf& rays, const uint32_t* count, uint32_t max_rays, bool any, const PrtTravTuning& tune,
               unsigned long long* stats, const PrtPrimary* primary, bool seeded = false) {
    const PrtWalkRequest request = !any ? PRT_WALK_CLOSEST : seeded ? PRT_WALK_SEEDED : PRT_WALK_ANY;
    const PrtWalkPlan plan = prt_plan_walk(walk_facts(c, tune, request, max_rays, stats != nullptr, primary != nullptr));
    prt_launch_walk(c->stream, plan, PrtWalkArgs{&c->dsc, rays, count, c->wk.work.as<uint32_t>(), c->spill.as<uint32_t>(), stats, primary, &tune});
}

// Measurement aid (sort_rays, tools/sort_ab.py): the front rays of `in` in sorted order through tune->perm.  The host needs
// the ray count, so this synchronises; the sort is timed as its own stage (scan_ms), the traversal that follows (`ep`) as usual.
int sort_front_rays(PrtContext* c, const PrtRayBuf& in, const uint32_t* front_count, uint32_t n_paths, EventPair* ep, PrtTravTuning* tune) {
    int rc;
    uint32_t n_front = 0;
    HIPCHECK(c, hipMemcpyAsync(&n_front, front_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if (n_front <= 1u) return PRT_OK;
    if (c->sort_entries < n_paths) {
        c->wk.sort = DevBuf();
        c->sort_entries = 0;
        c->sort_temp = prt_sort_rays_temp_bytes(n_paths);
        HIPCHECK(c, c->wk.sort.ensure(4 * (size_t)n_paths * sizeof(uint32_t) + c->sort_temp));
        c->sort_entries = n_paths;
    }
    EventPair es{};
    if ((rc = begin_event(c, 4, &es))) return rc;
    uint32_t* q = c->wk.sort.as<uint32_t>();
    if (prt_sort_rays(c->stream, in.o, in.d, n_front, c->dsc.root_min, c->dsc.root_max, c->sort_rays, q, q + n_paths,
                      q + 2 * (size_t)n_paths, q + 3 * (size_t)n_paths, q + 4 * (size_t)n_paths, c->sort_temp))
        return fail(c, PRT_ERR_HIP, "ray sort failed");
    if ((rc = end_event(c, &es))) return rc;
    if (c->timing) HIPCHECK(c, hipEventRecord(ev(ep->a), c->stream));  // the traversal's own time starts after the sort
    tune->perm = q + 3 * (size_t)n_paths;
    return PRT_OK;
}

// One batch of S_cur samples: raygen -> (intersect, shade) x max_depth -> [accumulate].  `view` says which pixels: the whole
// film (whole_film), or the tiles of a list (prt_render_adaptive): view.tm then counts the listed tiles only and compact local
// pixel pl is lane pl & 63 of tile view.list[pl >> 6].  The route (which stages run, which kernel instances) is prt_plan_route's
// (prt_route.h; DESIGN.md section 3 "Routes of a batch"): this function collects the facts and follows the plan.
int run_batch(PrtContext* c, const PrtBatchView& view, uint32_t S_cur, uint32_t max_depth, uint32_t seed, uint32_t first_sample,
              bool accumulate, unsigned long long* trav_stats) {
    const PrtTileMap& tm = view.tm;
    if (view.list && !c->film.stat.p) return fail(c, PRT_ERR_INVALID, "a tile list needs film statistics");
    const uint64_t n_paths64 = (uint64_t)S_cur * tm.n_pix_local;
    c->batch_walked = false;
    c->primary_reuse_active = 0u;
    if (n_paths64 == 0) return PRT_OK;
    if (n_paths64 > 0xFFFFFF00ull) return fail(c, PRT_ERR_INVALID, "too many paths in flight");
    const uint32_t n_paths = (uint32_t)n_paths64;
    int rc = ensure_path_state(c, n_paths);
    if (rc) return rc;
    if ((rc = ensure_spill(c))) return rc;
    if ((rc = sync_light_tables(c))) return rc;
    const PrtWalkFacts wf = walk_facts(c, c->tune, PRT_WALK_PATH, n_paths, trav_stats != nullptr, false);  // (as the PATH route asks)
    PrtRouteFacts f{};
    f.lit = c->lighting != PRT_LIGHTING_OFF;
    f.mesh_lights = mesh_lights_on(c);
    f.light_clusters = clusters_on(c);
    f.env = env_on(c);
    f.tex = tex_on(c);
    f.lens = c->lens.aperture > 0.0f;
    f.listed = view.list != nullptr;
    f.film_stats = c->film_stats;
    f.has_nodes = c->dsc.n_nodes != 0u;
    f.has_bvh2 = wf.has2;
    f.insts = wf.insts;
    f.abvh = wf.abvh;
    f.few_prims = c->dsc.n_prims <= 16u;
    f.jitter = c->sampling.jitter != 0u;
    f.sa = c->sampling.rr_depth != 0u || c->sampling.clamp > 0.0f;
    f.multi_sample = S_cur > 1u;
    f.variant0 = wf.variant == 0;
    f.compact_primary = c->compact_primary;
    f.primary_walk = c->primary_walk;
    f.takes_primary = prt_traverse_takes_primary(wf);
    f.primary_hit = c->tune.primary_hit != 0u;
    f.path_gate = !trav_stats && !c->d_shade_div && c->sort_rays == 0u && n_paths <= c->tune.path_max && prt_path_kernel_applies(wf);
    f.path_kernel = c->tune.path_kernel;
    f.fuse = c->tune.fuse;
    f.mesh_emissive = c->hs.mesh_emissive;
    f.depth_ge2 = max_depth >= 2u;
    f.sort_rays = c->sort_rays != 0u;
    f.last_segment = c->last_segment;
    const PrtRoutePlan plan = prt_plan_route(f);
    const bool lit = f.lit, compact = plan.compact, walk = plan.walk;
    // how this batch numbers its paths (prt_path_id.h): a function of the plan, the batch's sample count and the tunable
    const bool pixel_major_ids = prt_path_id_pixel_major(compact, S_cur, c->path_id_order);
    const DevEnv denv = dev_env(c);
    const DevTex dtex = dev_tex(c);
    const DevLens dlens{c->lens.aperture, c->lens.focus_distance};
    // The ray count of a bounce is only known on the device.  With big batches a k_shade grid sized for the worst case is
    // a million blocks, most of which find nothing to do (~0.5 ms per launch, 4 % of a C3 step).  The host therefore
    // reads the counts of bounce d back WHILE the traversal kernel of bounce d runs (the copy is enqueued right after
    // the producer that wrote them, the host waits for it after enqueueing the traversal): the GPU never waits for the
    // host, k_shade gets an exact grid, and a batch stops at the first bounce without rays.
    const bool exact = c->dsc.n_nodes != 0u && c->tune.exact_grids != 0u && (n_paths > (16384u * 512u) || c->tune.exact_grids == 2u);  // 2: always (tests)
    if (exact && !c->wk.counts_host.p) {
        HIPCHECK(c, c->wk.counts_host.alloc((PRT_MAX_DEPTH + 2) * 64 * sizeof(uint32_t)));
        for (DevEvent& e : c->wk.ev_counts) HIPCHECK(c, e.create(false));
        for (DevEvent& e : c->wk.ev_prod) HIPCHECK(c, e.create(false));
        HIPCHECK(c, hipStreamCreateWithFlags(&c->count_stream, hipStreamNonBlocking));
    }
    // the work arrays as the kernels take them (allocated with the scene and the film: ensure_counters)
    uint32_t* const d_counts = c->wk.counts.as<uint32_t>();
    uint32_t* const d_work = c->wk.work.as<uint32_t>();
    uint32_t* const h_counts = c->wk.counts_host.as<uint32_t>();
    float4* const d_rad = c->path.rad.as<float4>();
    auto read_back = [&](uint32_t d) -> hipError_t {  // counts of bounce d: words 0 (front) and 32 (back) of its stride
        // (on a stream of its own behind an event: in the render stream the 4-us copy kernel and the gaps around it were
        // 10-20 us per bounce, 1 % of a step of a rank of eight)
        hipError_t e = hipEventRecord(ev(c->wk.ev_prod[d]), c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->count_stream, ev(c->wk.ev_prod[d]), 0);
        if (e == hipSuccess)
            e = hipMemcpyAsync(h_counts + 64 * (size_t)d, d_counts + (size_t)d * PRT_CNT_STRIDE, 33 * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, c->count_stream);
        return e != hipSuccess ? e : hipEventRecord(ev(c->wk.ev_counts[d]), c->count_stream);
    };
    EventPair ep{};
    // film += the batch's samples (unless this is a measurement run) and per-depth ray counts from the paths' last segment indices
    auto accumulate_batch = [&]() -> int {
        if ((rc = begin_event(c, 3, &ep))) return rc;
        const PrtAccumulateArgs aa{d_rad, lit ? c->lb.lrad : nullptr, c->film.local.as<float4>(), c->film.stat.as<float2>(), tm, S_cur, max_depth,
                                   accumulate, c->ray_stats_target, compact ? c->wk.pix.as<float4>() + tm.n_pix_local : nullptr, view.list,
                                   pixel_major_ids};
        if (!prt_launch_accumulate(c->stream, plan.accumulate, aa)) return fail(c, PRT_ERR_INVALID, "no such accumulate instance");
        c->batch_instance[PRT_STAGE_ACCUMULATE] = prt_accumulate_name(plan.accumulate);
        if ((rc = end_event(c, &ep))) return rc;
        if (accumulate && !view.list) c->stats.samples += S_cur;  // (whole-film samples only)
        HIPCHECK(c, hipGetLastError());
        return PRT_OK;
    };
    c->shade_instance = "";  // (the path route launches no shade kernel)
    for (const char*& n : c->batch_instance) n = "";
    c->last_segment_active = plan.last_segment;
    c->last_batch_depth = plan.path ? 0u : max_depth;
    // Small batches (the reference's contract: ONE sample per ProgressiveRender call, cpu/renderer.cpp:49) can run as one
    // launch of the PATH instance of the traversal kernel, which carries whole paths (prt_kernels.h PrtPathArgs), instead
    // of raygen + 2 x max_depth launches.  Same arithmetic, same draws, same rad[] / k_accumulate: the frame is
    // bit-identical (tests run both routes).  OFF by default (prt_set_param("path_kernel", 1 | 2)): measured, it ties with
    // the pipeline up to ~250 k paths per call and loses above (profiles/r3_path_kernel.txt, TUNING.md): both are bound
    // by a path's chain of dependent node fetches, and the pipeline shades with full waves.
    if (plan.path) {
        HIPCHECK(c, hipMemsetAsync(d_work, 0, 256 * sizeof(uint32_t), c->stream));  // the cursors; the error flags in [256] stay for prt_synchronize
        PrtPathArgs pa{c->cam, tm, c->sampling, d_rad, first_sample, seed, max_depth, n_paths};
        if ((rc = begin_event(c, 1, &ep))) return rc;
        prt_launch_path(c->stream, prt_plan_walk(wf), c->dsc, pa, d_work, c->tune);
        if ((rc = end_event(c, &ep))) return rc;
        ++c->stats.intersect_launches;
        return accumulate_batch();
    }
    if (compact && c->pix_entries < tm.n_pix_local) {
        c->pix_entries = 0;
        c->primary_key.batch.valid = false;
        HIPCHECK(c, c->wk.pix.ensure(4 * (size_t)tm.n_pix_local * sizeof(float4)));
        c->pix_entries = tm.n_pix_local;
        c->pix_records_blank = false;
    }
    // The primary stage of a still camera (prt_primary_cache.h): on the compact route everything before the
    // first k_shade is a function of camera, scene, tile map, batch size, max_depth and route, so a batch whose key equals the
    // held one starts at its first k_shade (REUSE); every other batch runs k_raygen (REFRESH) and, if eligible, leaves a key.
    // The stage lives where no later bounce writes: d_pix, bounce 0's words of d_counts, and the persistent buffers, which stand
    // in for rb[0].t / .hd2 / .hit where the hits are per list slot (one walk per pixel; a batch of ONE sample, whose path slots
    // are that list: at most n_pix_local of them).  One walk per SAMPLE of a multi-sample batch (primary_walk = 0) has a hit per
    // path slot: it keeps rb[0] and is never reused.
    const bool instrumented = trav_stats != nullptr || c->d_shade_div != nullptr;
    const bool persistent = compact && (walk || S_cur == 1u);
    if (persistent && (rc = ensure_primary_state(c, n_paths, tm.n_pix_local))) return rc;
    float4* const d_pix = c->wk.pix.as<float4>();
    PrtRayBuf rb0 = c->rb[0];
    if (persistent) rb0.t = c->prim.pid.as<float4>(), rb0.hd2 = c->prim.list.as<float>(), rb0.hit = c->prim.hit.as<uint32_t>();
    PrtPrimaryStageKey now_stage{};
    PrtPrimaryKey& now = now_stage.batch;
    now.valid = persistent && c->primary_reuse != 0 && !instrumented;  // eligible (compact: no jitter, no lens, no tile list)
    if (now.valid) {
        const PrtWalkPlan wp0 = prt_plan_walk(walk_facts(c, c->tune, PRT_WALK_CLOSEST, walk ? tm.n_pix_local : n_paths, false, true));
        now.camera_gen = c->camera_gen, now.scene_gen = c->scene_gen;
        now.W = tm.W, now.H = tm.H, now.rank = tm.rank, now.world = tm.world, now.n_pix_local = tm.n_pix_local;
        now.S_cur = S_cur, now.max_depth = max_depth;
        now.plan = plan;
        now.walk_row = (uint32_t)wp0.launch[0].row, now.walk_prim = wp0.launch[0].prim;
        now.compact = compact, now.walk = walk, now.primary_hit = plan.primary_hit, now.lens = f.lens, now.jitter = f.jitter;
        now.rr_depth = c->sampling.rr_depth, now.clamp = c->sampling.clamp;
        now.listed = view.list != nullptr, now.instrumented = instrumented, now.exact = exact;
    }
    now_stage.id_order = pixel_major_ids ? 1u : 0u, now_stage.id_S = pixel_major_ids ? S_cur : 0u;
    const bool reuse = prt_primary_stage_reusable(c->primary_key, now_stage);
    c->primary_reuse_active = reuse ? 1u : 0u;
    if (reuse) ++c->primary_reused_batches;
    // front/back counters of every bounce start at zero (the producers add to them atomically).  REUSE: from bounce 1's stride.
    // Bounce 0's words are written by k_raygen alone (front, back, finished, list; k_shade of bounce d adds to bounce d + 1's,
    // and word 48, the shadow rays, belongs to the lighting modes, which are never compact) and read by the bounce-0 walk,
    // k_primary_hit and the first k_shade: they stand as the refresh left them.
    if (reuse) HIPCHECK(c, hipMemsetAsync(d_counts + PRT_CNT_STRIDE, 0, (size_t)max_depth * PRT_CNT_STRIDE * sizeof(uint32_t), c->stream));
    else HIPCHECK(c, hipMemsetAsync(d_counts, 0, (size_t)(max_depth + 1) * PRT_CNT_STRIDE * sizeof(uint32_t), c->stream));
    const DevLights lt = dev_lights(c);
    const DevMeshLights mlt = dev_mesh_lights(c);
    const DevLightClusters lct = dev_light_clusters(c);
    if (lit) {  // the paths' light radiance starts at zero (paths that end with their primary ray never get a light sample)
        if ((rc = ensure_light_state(c, n_paths))) return rc;
        HIPCHECK(c, hipMemsetAsync(c->lb.lrad, 0, (size_t)n_paths * sizeof(float4), c->stream));
    }
    // One walk per pixel (PrtPrimary): bounce 0's traversal runs over the list of front pixels that k_raygen writes into
    // rb0.hd2, counted in word PRT_CNT_LIST of bounce 0's counters (zeroed above), and leaves its hits in rb0.hit per list
    // slot.  A batch of ONE sample keeps its path slots: they ARE that list (one path per pixel, in the same order), and
    // k_raygen saves the second store and atomic.
    c->batch_walked = walk;
    const PrtPrimary primary{(const uint32_t*)rb0.t, d_pix, {c->cam.pos.x, c->cam.pos.y, c->cam.pos.z},
                             prt_path_id_order(tm.n_pix_local, S_cur, pixel_major_ids), first_sample, seed, walk ? 1u : 0u};
    PrtPrimary primary_list = primary;  // what the traversal sees: list slots in place of path slots, each entry a local pixel,
                                        // which is the sample-major id of the pixel's sample 0 whatever the batch's order
    if (walk) primary_list.pid = (const uint32_t*)rb0.hd2, primary_list.ids = prt_path_id_order(tm.n_pix_local, S_cur, false);
    // (REUSE: the name of the instance whose output the batch uses)
    c->batch_instance[PRT_STAGE_RAYGEN] = prt_raygen_name(plan.raygen);
    if (!reuse) {
        c->primary_key.batch.valid = false;  // k_raygen overwrites d_pix and bounce 0's counters: set again below, once the stage stands
        if ((rc = begin_event(c, 0, &ep))) return rc;
        const PrtRaygenArgs ra{&c->dsc, c->cam, tm, n_paths, first_sample, seed, max_depth, rb0, d_rad, d_counts, d_work, c->sampling,
                               compact ? d_pix : nullptr, walk, pixel_major_ids, f.env ? &denv : nullptr, f.lens ? &dlens : nullptr, view.list};
        if (!prt_launch_raygen(c->stream, plan.raygen, ra)) return fail(c, PRT_ERR_INVALID, "no such raygen instance");
        if ((rc = end_event(c, &ep))) return rc;
        if (exact) HIPCHECK(c, read_back(0));
    }
    for (uint32_t d = 0; d < max_depth; ++d) {
        const PrtRayBuf& in = d == 0 ? rb0 : c->rb[d & 1];
        const PrtRayBuf& out = c->rb[(d + 1) & 1];
        const uint32_t* front_count = d_counts + (size_t)d * PRT_CNT_STRIDE;
        const PrtPrimary* prim_d = (compact && d == 0) ? &primary : nullptr;
        const bool held = reuse && d == 0;  // bounce 0's hits and the pixels' hit records stand
        // (REUSE starts at the first k_shade: the cursors and the overflow counter k_raygen zeroes are the bounce-0 walk's, and
        // every k_shade zeroes them for the walk that follows it)
        if (c->dsc.n_nodes && !held) {  // only the front part of the buffer can hit a triangle
            if ((rc = begin_event(c, 1, &ep))) return rc;
            PrtTravTuning tune = c->tune;
            tune.probe_slot = d;
            tune.perm = nullptr;
            if (plan.walk8 && c->sort_rays && !prim_d && (d > 0 || c->sampling.jitter || f.lens))
                if ((rc = sort_front_rays(c, in, front_count, n_paths, &ep, &tune))) return rc;
            if (walk && d == 0)
                walk_rays(c, in, d_counts + PRT_CNT_LIST, tm.n_pix_local, false, tune, trav_stats, &primary_list);
            else if (plan.last_segment == 2u && d + 1u == max_depth && !trav_stats)
                // the last segment's stored rays only ask whether a triangle lies in front of their seed: the seeded any-hit walk
                // (instrumented batches keep the closest-hit walk, which answers the same question)
                walk_rays(c, in, front_count, n_paths, true, tune, nullptr, nullptr, true);
            else
                walk_rays(c, in, front_count, n_paths, false, tune, trav_stats, prim_d);
            if ((rc = end_event(c, &ep))) return rc;
            ++c->stats.intersect_launches;
            if (prim_d) {
                // (a batch of ONE sample has nothing to share: k_shade rebuilds the hit itself, one launch less)
                if (plan.primary_hit) {  // (timed with the shade stage)
                    if ((rc = begin_event(c, 2, &ep))) return rc;
                    prt_launch_primary_hit(c->stream, c->dsc, primary, in.hit, d_pix, d_counts);
                    if ((rc = end_event(c, &ep))) return rc;
                    c->pix_records_blank = false;
                } else if (!c->pix_records_blank) {  // "no record" for every pixel (hit id 0xFFFFFFFF never equals a hit k_shade looks up); stays so until k_primary_hit runs again
                    HIPCHECK(c, hipMemsetAsync(d_pix + 2 * (size_t)tm.n_pix_local, 0xFF, 2 * (size_t)tm.n_pix_local * sizeof(float4), c->stream));
                    c->pix_records_blank = true;
                }
            }
        }
        uint32_t n_rays_known = 0xFFFFFFFFu;
        if (exact && held) {  // bounce 0's counts as the refresh read them: no copy, no wait
            n_rays_known = c->primary_counts[0] + c->primary_counts[1];
        } else if (exact) {
            HIPCHECK(c, hipEventSynchronize(ev(c->wk.ev_counts[d])));
            n_rays_known = h_counts[64 * (size_t)d] + h_counts[64 * (size_t)d + 32];
            if (d == 0) c->primary_counts[0] = h_counts[0], c->primary_counts[1] = h_counts[32];
        }
        if (n_rays_known == 0u) break;  // every path has ended: the later bounces have nothing to do
        if (d == 0 && !reuse && now.valid) c->primary_key = now_stage;  // the stage stands: what the next batch may start from
        if (c->d_shade_div) prt_launch_shade_divstats(c->stream, c->dsc, in, d_counts, d, n_paths, c->d_shade_div, prim_d);
        if ((rc = begin_event(c, 2, &ep))) return rc;
        const PrtShadeInst shade = d == 0 ? plan.shade0 : plan.shade;
        const PrtShadeArgs sa{&c->dsc, in, out, d_rad, d_counts, d_work, d, max_depth, n_paths, c->sampling, n_rays_known, prim_d, plan.last_segment,
                              f.env ? &denv : nullptr, f.tex ? &dtex : nullptr, lit ? &lt : nullptr, (lit && f.mesh_lights) ? &mlt : nullptr,
                              lit ? &c->lb : nullptr, (lit && f.light_clusters) ? &lct : nullptr};
        if (!prt_launch_shade(c->stream, shade, sa)) return fail(c, PRT_ERR_INVALID, "no such shade instance");
        c->shade_instance = prt_shade_name(shade);
        // (bounce 0 is a stage of its own only where its instance differs from the later bounces')
        c->batch_instance[(d == 0 && plan.shade0 != plan.shade) ? PRT_STAGE_SHADE0 : PRT_STAGE_SHADE] = c->shade_instance;
        if (lit && (lt.n_lights || (f.env && (denv.t_all | denv.t_env)))) {
            // the bounce's shadow rays: prt_occluded's pipeline on the device-side count (at most one per ray of the
            // bounce), then their contributions into the paths' light radiance (timed with the shade stage)
            const uint32_t* scount = d_counts + (size_t)d * PRT_CNT_STRIDE + 48u;
            const uint32_t nmax = n_rays_known == 0xFFFFFFFFu ? n_paths : n_rays_known;
            prt_launch_scan_prims_bounded(c->stream, c->dsc, c->lb.sh, scount, d_work, nmax);
            if (c->dsc.n_nodes) walk_rays(c, c->lb.sh, scount, nmax, true, c->tune, nullptr, nullptr);
            prt_launch_light_accum(c->stream, c->dsc, c->lb, scount, d_work, nmax);
        }
        if ((rc = end_event(c, &ep))) return rc;
        if (exact && d + 1 < max_depth) HIPCHECK(c, read_back(d + 1));
    }
    return accumulate_batch();
}

// The one place that fills c->dsc: the compiled scene's scalars next to the context's device pointers (all null on a
// host-only context, which has no node stride and no tree depth for the launchers either).
void fill_dev_scene(PrtContext* c, uint32_t node_stride, uint32_t depth8) {
    const PrtSceneScalars& k = c->hs.sc;
    DevScene d{};
    const SceneMem& m = c->scene;
    d.prims = m.prims.as<DevPrim>();
    d.mat_rgbs = m.mat_rgbs.as<float4>();
    d.mat_type = m.mat_type.as<uint32_t>();
    d.nodes = m.nodes.as<float4>();
    d.nodes4 = m.nodes4.as<float4>();
    d.nodes8 = m.nodes8.as<uint4>();  // null when the tree has no compressed 8-wide form: the 4-wide kernel runs
    d.tris = m.tris.as<float4>();
    d.tri_normals = m.nrms.as<float4>();
    d.abvh_nodes = m.abvh_nodes.as<float4>();
    d.abvh_order = m.abvh_order.as<uint32_t>();
    d.insts = m.insts.as<DevInstance>();
    d.tlas_inst = m.tlas_inst.as<uint32_t>();
    d.n_insts = k.n_insts;
    d.node_stride = node_stride;
    d.depth8 = depth8;
    d.n_prims = k.n_prims;
    d.n_nodes = k.n_nodes;
    d.n_tris = k.n_tris;
    d.pad = k.pad;
    memcpy(d.abvh_q, k.abvh_q, sizeof(d.abvh_q));
    d.extent = k.extent;
    memcpy(d.root_min, k.root_min, sizeof(d.root_min));
    memcpy(d.root_max, k.root_max, sizeof(d.root_max));
    memcpy(d.sky, k.sky, sizeof(d.sky));
    c->dsc = d;
    touch_scene(c);  // (whatever filled the scene anew: a held primary stage is of the scene before)
}

// Second half of prt_set_scene / prt_clone_scene: the context's host copies -> its device.  `gb` (device-side build):
// the builder's arrays on this device become the scene's arrays; otherwise trees and triangle records are uploaded from
// the host copies (a scene built on ANOTHER device arrives that way too: its 8-wide tree and records were read back).
int upload_scene(PrtContext* c, BuiltTree* gb) {
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    free_scene(c);
    SceneMem& m = c->scene;
    if (gb) {  // the scene's from here on
        m.nodes8 = std::move(gb->nodes8);
        m.tris = std::move(gb->tris);
        m.nrms = std::move(gb->nrms);
    }
    // Node slots.  An 80-B node at a 16-B aligned address lies across two 128-B lines half of the time, so a visit that
    // misses the caches moves 1.5 lines = 192 B (tools/gather_calib.hip).  Trees far beyond the L2s (C5: 1.6 M nodes =
    // 131 MB, HBM-bound traversal) get one node per 128-B line instead: every miss is one line, at 1.6x the array size;
    // trees the caches hold (C3: 16 MB) stay packed, where the smaller footprint is worth more than the line count.
    const std::vector<uint32_t>& n8 = c->hs.nodes8_all.empty() ? c->hs.bvh.nodes8 : c->hs.nodes8_all;
    const size_t n_nodes8 = gb ? (size_t)gb->n_nodes : n8.size() / 20;
    const uint32_t node_stride = c->node_stride ? (uint32_t)c->node_stride : (n_nodes8 * 80 > ((size_t)64 << 20) ? 8u : 5u);
    if (node_stride == 8u && n_nodes8) {
        DevBuf wide;
        HIPCHECK(c, wide.ensure(128 * n_nodes8));
        hipError_t e = hipMemset(wide.p, 0, 128 * n_nodes8);
        if (e == hipSuccess)
            e = gb ? hipMemcpy2D(wide.p, 128, m.nodes8.p, 80, 80, n_nodes8, hipMemcpyDeviceToDevice)
                   : hipMemcpy2D(wide.p, 128, n8.data(), 80, 80, n_nodes8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipDeviceSynchronize();  // (device-to-device copies on the null stream return early; renders use c->stream)
        HIPCHECK(c, e);
        m.nodes8 = std::move(wide);
    }
    std::vector<float> rgbs(4 * c->hs.materials.size());
    std::vector<uint32_t> mtype(c->hs.materials.size());
    for (size_t i = 0; i < c->hs.materials.size(); ++i) {
        rgbs[4 * i + 0] = c->hs.materials[i].rgb[0];
        rgbs[4 * i + 1] = c->hs.materials[i].rgb[1];
        rgbs[4 * i + 2] = c->hs.materials[i].rgb[2];
        rgbs[4 * i + 3] = c->hs.materials[i].scalar;
        mtype[i] = c->hs.materials[i].type;
    }
    HIPCHECK(c, m.prims.alloc_copy(c->hs.prims.data(), c->hs.prims.size() * sizeof(DevPrim)));
    HIPCHECK(c, m.mat_rgbs.alloc_copy(rgbs.data(), rgbs.size() * 4));
    HIPCHECK(c, m.mat_type.alloc_copy(mtype.data(), mtype.size() * 4));
    if (!c->hs.scene_device_built) {  // (device-built scenes have no binary / 4-wide tree: null pointers select the 8-wide kernel)
        HIPCHECK(c, m.nodes.alloc_copy(c->hs.bvh.nodes.data(), c->hs.bvh.nodes.size() * 4));
        HIPCHECK(c, m.nodes4.alloc_copy(c->hs.bvh.nodes4.data(), c->hs.bvh.nodes4.size() * 4));
    }
    if (!gb && !n8.empty() && node_stride != 8u) HIPCHECK(c, m.nodes8.alloc_copy(n8.data(), n8.size() * 4));
    if (!c->hs.abvh.nodes4.empty()) {
        HIPCHECK(c, m.abvh_nodes.alloc_copy(c->hs.abvh.nodes4.data(), c->hs.abvh.nodes4.size() * 4));
        HIPCHECK(c, m.abvh_order.alloc_copy(c->hs.abvh.order.data(), c->hs.abvh.order.size() * 4));
    }
    if (!c->hs.dev_insts.empty()) {
        HIPCHECK(c, m.insts.alloc_copy(c->hs.dev_insts.data(), c->hs.dev_insts.size() * sizeof(DevInstance)));
        HIPCHECK(c, m.tlas_inst.alloc_copy(c->hs.tlas_inst.data(), c->hs.tlas_inst.size() * 4));
    }
    HIPCHECK(c, m.lights.alloc_copy(c->hs.lights.data(), c->hs.lights.size() * 4));
    HIPCHECK(c, m.prim_light.alloc_copy(c->hs.prim_light.data(), c->hs.prim_light.size() * 4));
    if (!gb) {
        HIPCHECK(c, m.tris.alloc_copy(c->hs.tri_records.data(), c->hs.tri_records.size() * 4));
        HIPCHECK(c, m.nrms.alloc_copy(c->hs.nrm_records.data(), c->hs.nrm_records.size() * 4));
    }
    if (mesh_lights_on(c)) {
        const int rc_ml = upload_mesh_lights(c);
        if (rc_ml) return rc_ml;
    }
    fill_dev_scene(c, node_stride, c->hs.bvh_info.depth8);
    const int rc_cnt = ensure_counters(c);
    if (rc_cnt) return rc_cnt;
    c->has_scene = true;
    c->t_env_dev = 0;  // (both tables went up unscaled)
    return sync_light_tables(c);
}

// Device-side build (csrc/bvh_gpu.hip) of the 8-wide tree over n triangles given as 9 floats each (+ normals, + a material
// per triangle): nodes and the triangle / normal records in the tree's slot order come back to the host copies the
// scene compiler works with (prt_scene.h PrtDeviceBuilder); with `keep` the device arrays stay allocated and are handed
// to the caller.  The builder's time is added to *ms.
int device_build(PrtContext* c, const float* verts, const float* norms, const uint32_t* tri_mat, uint32_t n, uint32_t n_prims,
                 std::vector<uint32_t>& nodes8, uint32_t& depth, float* tri_rec, float* nrm_rec, BuiltTree* keep, float leaf_cost, double* ms,
                 int builder) {
    float cmin[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, cmax[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (size_t t = 0; t < (size_t)n; ++t)
        for (int a = 0; a < 3; ++a) {
            const float* v = &verts[9 * t];
            const float lo = std::min(v[a], std::min(v[3 + a], v[6 + a])), hi = std::max(v[a], std::max(v[3 + a], v[6 + a]));
            const float cc = 0.5f * lo + 0.5f * hi;
            cmin[a] = std::min(cmin[a], cc);
            cmax[a] = std::max(cmax[a], cc);
        }
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    PrtGpuBvh gb{};
    int brc = 0;
    {  // the builder's inputs: gone before anything is read back
        DevBuf dv, dn, dm;
        hipError_t e = (hipError_t)dv.ensure(36 * (size_t)n);
        if (e == hipSuccess) e = (hipError_t)dn.ensure(36 * (size_t)n);
        if (e == hipSuccess) e = (hipError_t)dm.ensure(4 * (size_t)n);
        if (e == hipSuccess) e = hipMemcpy(dv.p, verts, 36 * (size_t)n, hipMemcpyHostToDevice);
        // (fills on the stream the builder's kernels run on: c->stream is non-blocking, nothing orders it after the null stream)
        if (e == hipSuccess) e = norms ? hipMemcpy(dn.p, norms, 36 * (size_t)n, hipMemcpyHostToDevice) : hipMemsetAsync(dn.p, 0, 36 * (size_t)n, c->stream);
        if (e == hipSuccess) e = tri_mat ? hipMemcpy(dm.p, tri_mat, 4 * (size_t)n, hipMemcpyHostToDevice) : hipMemsetAsync(dm.p, 0, 4 * (size_t)n, c->stream);
        if (e != hipSuccess) return fail(c, PRT_ERR_HIP, "device-side BVH build: %s", hipGetErrorString(e));
        const auto t0 = std::chrono::steady_clock::now();
        // gpu_build 1: the quality builder (PLOC + optimal collapse); 2: the Morton octree (fastest build, slower to traverse)
        brc = builder == 2 ? prt_gpu_bvh8_build(c->stream, dv.as<float>(), dn.as<float>(), dm.as<uint32_t>(), n, n_prims, cmin, cmax, &gb)
                           : prt_gpu_bvh8_build_ploc(c->stream, dv.as<float>(), dn.as<float>(), dm.as<uint32_t>(), n, n_prims, cmin, cmax, &gb, leaf_cost);
        *ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (brc < 0) {  // the builder itself gave up (too many passes / levels for this input): the caller may take the host builder
        (void)fail(c, PRT_ERR_INVALID, "device-side BVH build gave up (%d)", brc);
        return kPrtDeviceBuildGaveUp;
    }
    if (brc) return fail(c, PRT_ERR_HIP, "device-side BVH build failed (%d)", brc);
    BuiltTree bt;  // the builder's arrays are ours from here on
    bt.nodes8.adopt(gb.d_nodes8, 80 * (size_t)gb.n_nodes);
    bt.tris.adopt(gb.d_tris, 48 * (size_t)n);
    bt.nrms.adopt(gb.d_nrms, 48 * (size_t)n);
    bt.n_nodes = gb.n_nodes;
    nodes8.resize(20 * (size_t)gb.n_nodes);
    depth = gb.depth;
    hipError_t e = hipMemcpy(nodes8.data(), bt.nodes8.p, nodes8.size() * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(tri_rec, bt.tris.p, 48 * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && nrm_rec) e = hipMemcpy(nrm_rec, bt.nrms.p, 48 * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, PRT_ERR_HIP, "device-side BVH build: %s", hipGetErrorString(e));
    if (keep) *keep = std::move(bt);
    return PRT_OK;
}

int check_ready(PrtContext* c) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (!c->has_camera) return fail(c, PRT_ERR_INVALID, "prt_set_camera has not been called");
    if (!c->has_film) return fail(c, PRT_ERR_INVALID, "prt_set_film has not been called");
    return PRT_OK;
}

// This rank's film_local (float4 per local pixel) and moments (float2) on the host, for the two read-back calls below.
int read_local_moments(PrtContext* c, std::vector<float>* film, std::vector<float>* stat) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_film) return fail(c, PRT_ERR_INVALID, "prt_set_film has not been called");
    if (!c->film_stats || !c->film.stat.p) return fail(c, PRT_ERR_INVALID, "film statistics are off (prt_set_film_statistics)");
    const size_t n = c->tm.n_pix_local;
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if (film) {
        film->assign(4 * n, 0.0f);
        if (n) HIPCHECK(c, hipMemcpy(film->data(), c->film.local.as<float4>(), n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    stat->assign(2 * n, 0.0f);
    if (n) HIPCHECK(c, hipMemcpy(stat->data(), c->film.stat.as<float2>(), n * sizeof(float2), hipMemcpyDeviceToHost));
    return PRT_OK;
}

// fn(local pixel, film pixel) for every pixel of this rank's tiles that lies in the image (the device's tile_pixel)
template <class F>
void for_each_local_pixel(const PrtTileMap& tm, F fn) {
    for (uint32_t lt = 0; lt < tm.n_tiles_local; ++lt) {
        const uint32_t gt = lt * tm.world + tm.rank;
        const uint32_t tx = gt % tm.tiles_x, ty = gt / tm.tiles_x;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint32_t x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
            if (x < tm.W && y < tm.H) fn((size_t)lt * 64u + lane, (size_t)y * tm.W + x);
        }
    }
}

}  // namespace

extern "C" {

int prt_version(void) { return PRT_VERSION; }

int prt_create(int device_id, PrtContext** out) {
    if (!out) return PRT_ERR_INVALID;
    PrtContext* c = new PrtContext();
    *out = c;
    c->device = device_id;
    if (device_id < 0) return PRT_OK;  // host-only context
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(c, PRT_ERR_NO_DEVICE, "no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device_id >= n) return fail(c, PRT_ERR_NO_DEVICE, "device %d out of range (%d devices)", device_id, n);
    HIPCHECK(c, hipSetDevice(device_id));
    HIPCHECK(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    c->has_device = true;
    return PRT_OK;
}

void prt_destroy(PrtContext* c) {
    if (!c) return;
    if (c->has_device) {  // (a host-only context owns nothing on a device: its destructor makes no HIP call)
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (c->count_stream) (void)hipStreamDestroy(c->count_stream);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    }
    delete c;  // every allocation, pinned word and event goes with its owner (prt_devmem.h)
}

void prt_device_memory_info(uint64_t* live_bytes, uint64_t* alloc_calls) {
    if (live_bytes) *live_bytes = g_live_bytes.load();
    if (alloc_calls) *alloc_calls = g_alloc_calls.load();
}

const char* prt_last_error(const PrtContext* c) { return c ? c->err.c_str() : "null context"; }

int prt_set_stream(PrtContext* c, void* hip_stream) {
    int rc = need_device(c);
    if (rc) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    touch_scene(c);  // (coarse: the held primary stage was written on the other stream)
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return PRT_OK;
}

int prt_get_stream(PrtContext* c, void** hip_stream) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!hip_stream) return PRT_ERR_INVALID;
    *hip_stream = (void*)c->stream;
    return PRT_OK;
}

int prt_get_device(const PrtContext* c) { return c ? c->device : -1; }

int prt_set_scene(PrtContext* c, const PrtSceneDesc* s) {
    if (!c || !s) return PRT_ERR_INVALID;
    c->feat_valid = false;
    touch_scene(c);
    drop_history(c);
    int rc = prt_check_scene_arrays(s, &c->err);
    if (rc) return rc;
    // A scene the context held before is gone whatever happens: a failure below leaves the context WITHOUT a scene (the
    // next render fails with PRT_ERR_INVALID); has_scene is set again only after the last upload.
    c->has_scene = false;
    c->host_copies_stale = false;  // (of the scene that goes; its tables on the device go with free_scene)
    c->rk.ready = false;
    c->rinfo = PrtRefitInfo{};
    drop_tex(c);
    PrtHostScene hs = std::move(c->hs);  // (the compiler recycles the record arrays' storage; everything else goes)
    c->hs = PrtHostScene();
    PrtSceneOptions opt{c->pad_coeff, c->abvh_enabled != 0, nullptr, c->light_max_clusters};
    // device-side build (prt_set_param("gpu_build", 1 | 2)) on a context with a device: world meshes, placed copies and the
    // top-level tree.  The world meshes' device arrays (`keep`) stay with this layer: they become the scene's arrays below,
    // or go if the compiler did not take that tree after all (deeper than the kernels' stacks: the host builder's stands)
    BuiltTree gb;
    if (c->gpu_build && c->has_device)
        opt.device_build = [&](const float* verts, const float* norms, const uint32_t* tri_mat, uint32_t n, uint32_t n_prims, float leaf_cost,
                               bool keep, std::vector<uint32_t>& nodes8, uint32_t& depth, float* tri_rec, float* nrm_rec, double* ms, std::string* err) {
            const int brc = device_build(c, verts, norms, tri_mat, n, n_prims, nodes8, depth, tri_rec, nrm_rec, keep ? &gb : nullptr, leaf_cost, ms,
                                         c->gpu_build);
            if (brc) *err = c->err;
            return brc;
        };
    rc = prt_compile_scene(s, opt, &hs, &c->err);
    const bool use_gb = !rc && gb.nodes8.p && hs.scene_device_built;
    if (!use_gb) gb = BuiltTree();
    if (rc) return rc;
    c->hs = std::move(hs);
    c->hs.builder = opt.device_build ? (uint32_t)c->gpu_build : 0u;
    c->inst_info = PrtInstanceUpdateInfo{};
    if (!c->has_device) {  // host-only context: BVH built, nothing to upload
        fill_dev_scene(c, 0u, 0u);
        c->has_scene = true;
        return PRT_OK;
    }
    return upload_scene(c, use_gb ? &gb : nullptr);
}

// Replicates the scene of `src` (host copies of the flattened primitives, trees and triangle records) onto the device
// of `dst` without building anything again: the multi-GPU host path builds the BVH once and clones it N - 1 times.
int prt_clone_scene(PrtContext* dst, const PrtContext* src) {
    if (!dst || !src) return PRT_ERR_INVALID;
    if (!src->has_scene) return fail(dst, PRT_ERR_INVALID, "prt_clone_scene: the source context has no scene");
    if (dst == src) return PRT_OK;
    // (the source's host copies are a cache of its device arrays: bringing them up to date changes nothing a caller can see)
    if (const int rc = refresh_host_copies(const_cast<PrtContext*>(src))) return fail(dst, rc, "prt_clone_scene: %s", src->err.c_str());
    dst->feat_valid = false;
    touch_scene(dst);
    drop_history(dst);
    dst->has_scene = false;
    drop_tex(dst);
    dst->hs = src->hs;
    dst->tex = src->tex;
    dst->inst_info = PrtInstanceUpdateInfo{};
    dst->light_sources = src->light_sources;
    dst->light_selection = src->light_selection;
    dst->light_max_clusters = src->light_max_clusters;
    dst->env = src->env;
    if (!dst->has_device) {
        fill_dev_scene(dst, 0u, 0u);
        dst->has_scene = true;
        return PRT_OK;
    }
    const int rc_env = upload_env(dst);
    if (rc_env) return rc_env;
    const int rc_tex = upload_tex(dst);
    if (rc_tex) return rc_tex;
    return upload_scene(dst, nullptr);
}

// What a refit leaves of the scene besides its records and tree, either form: root_box from the refitted root, extent the
// largest |coordinate| of the new vertices.
static void commit_refit(PrtContext* c, const float root_box[6], float extent) {
    // the binary and 4-wide trees (A/B kernels, overflow fallback of deep host-built trees) still describe the OLD
    // geometry: they go, and the instance selection falls to the 8-wide kernels that need neither (prt_plan_walk)
    c->scene.nodes = DevBuf();
    c->scene.nodes4 = DevBuf();
    c->dsc.nodes = nullptr;
    c->dsc.nodes4 = nullptr;
    c->hs.bvh.nodes.clear();
    c->hs.bvh.nodes4.clear();
    c->hs.scene_device_built = true;
    c->variant = 0;
    PrtSceneScalars& k = c->hs.sc;  // (a clone of this scene starts from the refitted bounds too)
    for (int a = 0; a < 3; ++a) {
        c->dsc.root_min[a] = k.root_min[a] = root_box[a];
        c->dsc.root_max[a] = k.root_max[a] = root_box[3 + a];
    }
    float ext_all = extent;
    if (!c->hs.abvh.nodes4.empty()) ext_all = std::max(ext_all, k.extent);  // (the primitive walk's pad scales with the larger of the two)
    c->dsc.extent = k.extent = ext_all;
    c->hs.bvh_info.refit_ms = (float)c->refit_ms;
    ++c->hs.bvh_info.refits;
    c->hs.bvh_info.n_nodes = 0;      // (the binary and 4-wide trees are gone)
    c->hs.bvh_info.n_nodes4 = 0;
    c->hs.bvh_info.node_bytes = 0;
    c->hs.bvh_info.max_stack4 = 0;
}

// PrtRefitInfo of a refit that went through
static void refit_done(PrtContext* c, uint32_t form, uint32_t normals_computed, const PrtCopyTally& tally,
                       std::chrono::steady_clock::time_point t_call) {
    c->rinfo.last_form = form;
    c->rinfo.normals_computed = normals_computed;
    c->rinfo.device_ms = (float)c->refit_ms;
    c->rinfo.wall_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    c->rinfo.h2d_bytes = tally.h2d;
    c->rinfo.d2h_bytes = tally.d2h;
}

// Deforming geometry: the world-space meshes of the current scene with NEW vertex positions / normals (same vertex and
// triangle counts, same index buffers as at prt_set_scene).  The 8-wide tree keeps its topology and is refitted on the
// device (csrc/bvh_gpu.hip prt_gpu_bvh8_refit): records rewritten, boxes recomputed bottom-up, nodes re-quantized.
int prt_refit_meshes(PrtContext* c, const PrtMesh* meshes, uint32_t n_meshes) {
    if (c) c->feat_valid = false;
    if (c) touch_scene(c);
    if (c) drop_history(c);
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (!meshes && n_meshes) return fail(c, PRT_ERR_INVALID, "null mesh array");
    if (c->dsc.n_insts) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes: scenes with placed copies are rebuilt, not refitted");
    if (!c->dsc.nodes8 || c->hs.bvh.nodes8.empty()) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes needs the compressed 8-wide tree");
    if (2 * (size_t)n_meshes != c->hs.mesh_sizes.size()) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes: the scene has %zu meshes", c->hs.mesh_sizes.size() / 2);
    // the refit drops the 4-wide tree, and with it the re-walk of the rays that overflow the 8-wide kernels' stacks: the deepest
    // of those (deep15_4waves, 15 entries) holds every ray of a tree of 16 levels and no more
    if (c->hs.bvh_info.depth8 > 16u)
        return fail(c, PRT_ERR_INVALID, "prt_refit_meshes: a tree of %u levels (depth8 > 16) is rebuilt with prt_set_scene, not refitted",
                    c->hs.bvh_info.depth8);
    uint64_t n_tris = 0;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        const PrtMesh& me = meshes[m];
        if (me.n_vertices != c->hs.mesh_sizes[2 * m] || me.n_triangles != c->hs.mesh_sizes[2 * m + 1])
            return fail(c, PRT_ERR_INVALID, "prt_refit_meshes: mesh %u has another topology than at prt_set_scene", m);
        if (me.n_triangles && (!me.positions || !me.normals || !me.indices)) return fail(c, PRT_ERR_INVALID, "mesh %u: positions, normals and indices are required", m);
        n_tris += me.n_triangles;
    }
    if (n_tris != c->dsc.n_tris || n_tris == 0) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes: triangle count mismatch");
    if ((rc = refresh_host_copies(c))) return rc;  // (a refit from device arrays left them behind; not part of this call's traffic)
    const auto t_call = std::chrono::steady_clock::now();
    PrtCopyTally tally{0, 0};
    struct TallyScope {  // the light tables' uploads below count too
        PrtContext* c;
        ~TallyScope() { c->tally = nullptr; }
    } scope{c};
    c->tally = &tally;
    std::vector<float> verts(9 * (size_t)n_tris), norms(9 * (size_t)n_tris);
    float extent = 0.0f;
    for (size_t m = 0, t = 0; m < n_meshes; t += meshes[m++].n_triangles)
        if ((rc = prt_flatten_mesh(meshes[m], "mesh", (uint32_t)m, verts.data() + 9 * t, norms.data() + 9 * t, &extent, nullptr, nullptr, &c->err))) return rc;
    // the nodes of every tree level, from the host copy of the tree
    const std::vector<uint32_t>& n8 = c->hs.bvh.nodes8;
    const uint32_t n_nodes = (uint32_t)(n8.size() / 20);
    std::vector<uint32_t> level_nodes, level_start;
    if (const uint32_t bad = prt_tree_levels(n8, n_nodes, level_nodes, level_start))
        return fail(c, PRT_ERR_INVALID, "prt_refit_meshes: malformed tree (node %u)", bad - 1u);
    if (level_nodes.size() != n_nodes) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes: %zu of %u nodes reachable from the root", level_nodes.size(), n_nodes);
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    const SceneMem& m = c->scene;
    float root_box[6] = {0, 0, 0, 0, 0, 0};
    int brc = 0;
    hipError_t e;
    {  // the new vertices and normals on the device: gone before the host copies are read back
        DevBuf dv, dn;
        e = (hipError_t)dv.ensure(36 * (size_t)n_tris);
        if (e == hipSuccess) e = (hipError_t)dn.ensure(36 * (size_t)n_tris);
        if (e == hipSuccess) e = hipMemcpy(dv.p, verts.data(), 36 * (size_t)n_tris, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dn.p, norms.data(), 36 * (size_t)n_tris, hipMemcpyHostToDevice);
        tally.h2d += 72 * (uint64_t)n_tris;
        if (e == hipSuccess) {
            const auto t0 = std::chrono::steady_clock::now();
            brc = prt_gpu_bvh8_refit(c->stream, m.nodes8.as<uint32_t>(), c->dsc.node_stride * 4u, n_nodes, level_nodes.data(), level_start.data(),
                                     (uint32_t)level_start.size() - 1u, dv.as<float>(), dn.as<float>(), (uint32_t)n_tris, c->dsc.n_prims,
                                     m.tris.as<float4>(), m.nrms.as<float4>(), root_box, &tally);
            c->refit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
    }
    if (e != hipSuccess || brc) {
        c->has_scene = false;  // the device arrays may be half rewritten
        return fail(c, PRT_ERR_HIP, "prt_refit_meshes: %s (%d)", e != hipSuccess ? hipGetErrorString(e) : "refit failed", brc);
    }
    // host copies (prt_bvh_read8 / prt_bvh_read, prt_clone_scene) follow the device
    e = hipMemcpy2D(c->hs.bvh.nodes8.data(), 80, c->scene.nodes8.p, (size_t)c->dsc.node_stride * 16, 80, n_nodes, hipMemcpyDeviceToHost);
    tally.d2h += 80 * (uint64_t)n_nodes;
    if (e == hipSuccess && c->hs.tri_records.size() == 12 * (size_t)n_tris) {
        e = hipMemcpy(c->hs.tri_records.data(), c->scene.tris.p, 48 * (size_t)n_tris, hipMemcpyDeviceToHost);
        tally.d2h += 48 * (uint64_t)n_tris;
    }
    if (e == hipSuccess && c->hs.nrm_records.size() == 12 * (size_t)n_tris) {
        e = hipMemcpy(c->hs.nrm_records.data(), c->scene.nrms.p, 48 * (size_t)n_tris, hipMemcpyDeviceToHost);
        tally.d2h += 48 * (uint64_t)n_tris;
    }
    HIPCHECK(c, e);
    commit_refit(c, root_box, extent);
    // triangle lights follow the geometry: the candidate table again from the new vertices (host), uploaded if in use
    prt_rebuild_mesh_lights(&c->hs, verts.data());
    if (mesh_lights_on(c) && (rc = upload_mesh_lights(c))) return rc;
    refit_done(c, 1u, 0u, tally, t_call);
    return PRT_OK;
}

// The tables and working arrays a refit from device arrays keeps with the scene: built (prt_scene.cpp) and uploaded at the
// first call, in one allocation; free_scene drops them.
static int ensure_refit_keep(PrtContext* c, PrtCopyTally* tally) {
    PrtContext::RefitKeep& rk = c->rk;
    if (rk.ready) return PRT_OK;
    PrtRefitTables t;
    int rc = prt_build_refit_tables(c->hs, &t, &c->err);
    if (rc) return rc;
    const size_t n_nodes = t.level_nodes.size(), n_vert = t.vert_first.back(), n_corner = t.corner.size(), n_light = t.light_tris.size();
    PrtWorkspace ws;
    ws.add(&rk.d_corner, n_corner).add(&rk.d_csr_start, n_vert + 1).add(&rk.d_csr_corner, n_corner).add(&rk.d_light_tris, n_light);
    ws.add(&rk.d_valid, 4).add(&rk.d_normals, 3 * n_vert).add(&rk.d_light_verts, 9 * n_light);
    ws.add(&rk.scratch.cbox, 48 * n_nodes).add(&rk.scratch.nbox, 6 * n_nodes).add(&rk.scratch.counters, 4).add(&rk.scratch.level_nodes, n_nodes);
    if ((rc = commit(c, ws, c->scene.refit_keep))) {
        rk = PrtContext::RefitKeep();
        return rc;
    }
    auto up = [&](uint32_t* dst, const std::vector<uint32_t>& src) -> hipError_t {
        if (src.empty()) return hipSuccess;
        if (tally) tally->h2d += 4 * (uint64_t)src.size();
        return hipMemcpyAsync(dst, src.data(), 4 * src.size(), hipMemcpyHostToDevice, c->stream);
    };
    hipError_t e = up(rk.d_corner, t.corner);
    if (e == hipSuccess) e = up(rk.d_csr_start, t.csr_start);
    if (e == hipSuccess) e = up(rk.d_csr_corner, t.csr_corner);
    if (e == hipSuccess) e = up(rk.d_light_tris, t.light_tris);
    if (e == hipSuccess) e = up(rk.scratch.level_nodes, t.level_nodes);
    const hipError_t es = hipStreamSynchronize(c->stream);  // (the tables go out of scope below)
    if (e != hipSuccess || es != hipSuccess) {
        rk = PrtContext::RefitKeep();
        HIPCHECK(c, e != hipSuccess ? e : es);
    }
    rk.tri_first = std::move(t.tri_first);
    rk.vert_first = std::move(t.vert_first);
    rk.level_start = std::move(t.level_start);
    rk.n_nodes = (uint32_t)n_nodes;
    rk.n_light_tris = (uint32_t)n_light;
    rk.ready = true;
    return PRT_OK;
}

// prt_refit_meshes for vertex arrays on the device (include/prt.h): validated there, records gathered through the scene's
// index buffers (bvh_gpu.hip prt_gpu_bvh8_refit_indexed), host copies left to refresh_host_copies.
int prt_refit_meshes_device(PrtContext* c, const PrtMeshDeviceArrays* meshes, uint32_t n_meshes) {
    if (c) c->feat_valid = false;
    if (c) touch_scene(c);
    if (c) drop_history(c);
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (!meshes && n_meshes) return fail(c, PRT_ERR_INVALID, "null mesh array");
    if (c->dsc.n_insts) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes_device: scenes with placed copies are rebuilt, not refitted");
    if (!c->dsc.nodes8 || c->hs.bvh.nodes8.empty()) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes_device needs the compressed 8-wide tree");
    if (2 * (size_t)n_meshes != c->hs.mesh_sizes.size())
        return fail(c, PRT_ERR_INVALID, "prt_refit_meshes_device: the scene has %zu meshes", c->hs.mesh_sizes.size() / 2);
    if (c->hs.bvh_info.depth8 > 16u)  // (prt_refit_meshes says why)
        return fail(c, PRT_ERR_INVALID, "prt_refit_meshes_device: a tree of %u levels (depth8 > 16) is rebuilt with prt_set_scene, not refitted",
                    c->hs.bvh_info.depth8);
    uint64_t n_tris = 0;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        if (c->hs.mesh_sizes[2 * m + 1] && !meshes[m].positions) return fail(c, PRT_ERR_INVALID, "mesh %u: positions are required", m);
        n_tris += c->hs.mesh_sizes[2 * m + 1];
    }
    if (n_tris != c->dsc.n_tris || n_tris == 0) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes_device: triangle count mismatch");
    const auto t_call = std::chrono::steady_clock::now();
    PrtCopyTally tally{0, 0};
    struct TallyScope {
        PrtContext* c;
        ~TallyScope() { c->tally = nullptr; }
    } scope{c};
    c->tally = &tally;
    if ((rc = ensure_refit_keep(c, &tally))) return rc;
    PrtContext::RefitKeep& rk = c->rk;
    if (rk.n_nodes != c->hs.bvh.nodes8.size() / 20 || rk.level_start.size() < 2) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes_device: no level lists for this tree");
    std::vector<const float*> pos(n_meshes), nrm_in(n_meshes), nrm(n_meshes);
    std::vector<float*> nout(n_meshes);
    uint32_t n_computed = 0;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        pos[m] = meshes[m].positions;
        nrm_in[m] = meshes[m].normals;
        nout[m] = meshes[m].normals || !c->hs.mesh_sizes[2 * m] ? nullptr : rk.d_normals + 3 * (size_t)rk.vert_first[m];
        nrm[m] = meshes[m].normals ? meshes[m].normals : rk.d_normals + 3 * (size_t)rk.vert_first[m];
        n_computed += nout[m] ? 1u : 0u;
    }
    const PrtRefitInputs in{n_meshes, pos.data(), rk.tri_first.data(), rk.vert_first.data()};
    // 1. the inputs, before anything of the scene is written
    uint32_t valid[2] = {0u, 0u};
    hipError_t e = (hipError_t)prt_gpu_refit_validate(c->stream, in, nrm_in.data(), rk.d_corner, rk.d_valid);
    if (e == hipSuccess) e = hipMemcpyAsync(valid, rk.d_valid, sizeof(valid), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    tally.d2h += sizeof(valid);
    HIPCHECK(c, e);
    if (valid[1]) return fail(c, PRT_ERR_INVALID, "prt_refit_meshes_device: non-finite vertex%s", (valid[1] & 1u) ? "" : " normal");
    float extent = 0.0f;
    memcpy(&extent, &valid[0], 4);
    // 2. normals where none came, the emissive triangles for the host's candidate table, records, boxes, quantization
    float root_box[6] = {0, 0, 0, 0, 0, 0};
    const auto t0 = std::chrono::steady_clock::now();
    int brc = n_computed ? prt_gpu_mesh_normals(c->stream, in, nout.data(), rk.d_corner, rk.d_csr_start, rk.d_csr_corner) : 0;
    if (!brc) brc = prt_gpu_light_gather(c->stream, in, rk.d_corner, rk.d_light_tris, rk.n_light_tris, rk.d_light_verts);
    if (!brc)
        brc = prt_gpu_bvh8_refit_indexed(c->stream, c->scene.nodes8.as<uint32_t>(), c->dsc.node_stride * 4u, rk.n_nodes, rk.level_start.data(),
                                         (uint32_t)rk.level_start.size() - 1u, in, nrm.data(), rk.d_corner, (uint32_t)n_tris, c->dsc.n_prims,
                                         c->scene.tris.as<float4>(), c->scene.nrms.as<float4>(), rk.scratch, root_box, &tally);
    c->refit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::vector<float> packed(9 * (size_t)rk.n_light_tris);
    if (!brc && !packed.empty()) {
        brc = (int)hipMemcpy(packed.data(), rk.d_light_verts, 4 * packed.size(), hipMemcpyDeviceToHost);
        tally.d2h += 4 * (uint64_t)packed.size();
    }
    if (brc) {
        c->has_scene = false;  // the device arrays may be half rewritten
        return fail(c, PRT_ERR_HIP, "prt_refit_meshes_device: refit failed (%d)", brc);
    }
    c->host_copies_stale = true;
    commit_refit(c, root_box, extent);
    prt_rebuild_mesh_lights_packed(&c->hs, packed.data());
    if (mesh_lights_on(c) && (rc = upload_mesh_lights(c))) return rc;
    refit_done(c, 2u, n_computed, tally, t_call);
    return PRT_OK;
}

int prt_mesh_normals_device(PrtContext* c, uint32_t mesh, const float* positions, float* normals_out) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (2 * (size_t)mesh + 1 >= c->hs.mesh_sizes.size()) return fail(c, PRT_ERR_INVALID, "prt_mesh_normals_device: the scene has %zu meshes", c->hs.mesh_sizes.size() / 2);
    if (!c->hs.mesh_sizes[2 * mesh]) return PRT_OK;
    if (!positions || !normals_out) return fail(c, PRT_ERR_INVALID, "prt_mesh_normals_device: null array");
    if ((rc = ensure_refit_keep(c, nullptr))) return rc;
    const PrtContext::RefitKeep& rk = c->rk;
    const PrtRefitInputs in{1u, &positions, &rk.tri_first[mesh], &rk.vert_first[mesh]};
    hipError_t e = (hipError_t)prt_gpu_mesh_normals(c->stream, in, &normals_out, rk.d_corner, rk.d_csr_start, rk.d_csr_corner);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIPCHECK(c, e);
    return PRT_OK;
}

int prt_refit_info(PrtContext* c, PrtRefitInfo* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    *out = c->rinfo;
    out->refits = c->has_scene ? c->hs.bvh_info.refits : 0u;
    out->host_copies_stale = c->host_copies_stale ? 1u : 0u;
    return PRT_OK;
}

// Rigid-body motion of the placed copies (include/prt.h "Moving placed copies"): only the top level follows.  The host
// half (checks, instance table, world boxes, host / device build of a new top level, light candidates) is prt_scene.cpp's;
// this function owns the device half: bvh_gpu.hip's k_place_copies, the top-level refit and the rebase pass.
int prt_set_instance_transforms(PrtContext* c, const PrtInstance* instances, uint32_t n, uint32_t mode) {
    if (!c) return PRT_ERR_INVALID;
    c->feat_valid = false;
    touch_scene(c);
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (mode != (uint32_t)PRT_INSTANCES_REFIT && mode != (uint32_t)PRT_INSTANCES_REBUILD)
        return fail(c, PRT_ERR_INVALID, "prt_set_instance_transforms: mode is PRT_INSTANCES_REFIT or PRT_INSTANCES_REBUILD, not %u", mode);
    int rc = prt_check_instance_update(c->hs, instances, n, &c->err);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    PrtHostScene& hs = c->hs;
    PrtInstanceUpdate up;
    prt_instance_tables(hs, instances, &up);
    PrtSceneOptions opt{c->pad_coeff, c->abvh_enabled != 0, nullptr};
    const int builder = c->has_device ? (int)hs.builder : 0;
    if (builder)
        opt.device_build = [&](const float* verts, const float* norms, const uint32_t* tri_mat, uint32_t nt, uint32_t n_prims, float leaf_cost, bool,
                               std::vector<uint32_t>& nodes8, uint32_t& depth, float* tri_rec, float* nrm_rec, double* ms, std::string* err) {
            const int brc = device_build(c, verts, norms, tri_mat, nt, n_prims, nodes8, depth, tri_rec, nrm_rec, nullptr, leaf_cost, ms, builder);
            if (brc) *err = c->err;
            return brc;
        };
    auto done = [&](uint32_t ran) {
        ++c->inst_info.updates;
        c->inst_info.last_mode = ran;
        c->inst_info.last_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return PRT_OK;
    };
    if (!c->has_device) {  // host-only context: the host rebuild, whatever the mode
        if ((rc = prt_build_top_level(opt, hs, &up, &hs.gpu_build_ms, &c->err))) return rc;
        prt_commit_top_level(&hs, up);
        prt_commit_instances(&hs, up, instances);
        fill_dev_scene(c, 0u, 0u);
        return done(PRT_INSTANCES_REBUILD);
    }
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    // what the device pass reads: the transforms, the mesh boxes (+ the world meshes' world box as the last row), the row
    // of every instance, and the records it writes
    const uint32_t n_total = (uint32_t)hs.dev_insts.size(), n_world = hs.n_world_insts, n_meshes = (uint32_t)hs.placed_meshes.size();
    const uint32_t stride = c->dsc.node_stride, old_top = hs.top_nodes, n_all = (uint32_t)(hs.nodes8_all.size() / 20);
    std::vector<float> xf(32 * (size_t)n), mesh_box(6 * ((size_t)n_meshes + 1));
    std::vector<uint32_t> inst_mesh(n_total, n_meshes);
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(&xf[32 * (size_t)i], instances[i].mat, 64);
        memcpy(&xf[32 * (size_t)i + 16], instances[i].inv, 64);
        inst_mesh[n_world + i] = hs.inst_mesh[i];
    }
    for (uint32_t m = 0; m < n_meshes; ++m) {
        memcpy(&mesh_box[6 * (size_t)m], hs.placed_meshes[m].mn, 12);
        memcpy(&mesh_box[6 * (size_t)m + 3], hs.placed_meshes[m].mx, 12);
    }
    memcpy(&mesh_box[6 * (size_t)n_meshes], hs.world_box.data(), 24);
    SceneMem& m = c->scene;
    DevBuf d_xf, d_box, d_im, d_recs, d_new;  // (freed when the function returns)
    hipError_t e = (hipError_t)d_xf.alloc_copy(xf.data(), xf.size() * 4);
    if (e == hipSuccess) e = (hipError_t)d_box.alloc_copy(mesh_box.data(), mesh_box.size() * 4);
    if (e == hipSuccess) e = (hipError_t)d_im.alloc_copy(inst_mesh.data(), inst_mesh.size() * 4);
    if (e == hipSuccess) e = (hipError_t)d_recs.ensure(std::max<size_t>(48 * (size_t)n_total, 16));
    if (e != hipSuccess) return fail(c, PRT_ERR_HIP, "prt_set_instance_transforms: %s", hipGetErrorString(e));  // (nothing of the scene written yet)
    auto broken = [&](hipError_t he, int brc) {
        c->has_scene = false;  // the device arrays may be half rewritten
        return fail(c, PRT_ERR_HIP, "prt_set_instance_transforms: %s (%d)", he != hipSuccess ? hipGetErrorString(he) : "device pass failed", brc);
    };
    const size_t node_bytes = (size_t)stride * 16;
    bool top_dirty = false;  // the device's top level no longer matches the host copy
    if (mode == (uint32_t)PRT_INSTANCES_REFIT) {
        std::vector<uint32_t> level_nodes, level_start;
        if (prt_tree_levels(hs.nodes8_all, old_top, level_nodes, level_start) || level_nodes.size() != old_top) {
            return fail(c, PRT_ERR_INVALID, "prt_set_instance_transforms: malformed top-level tree");
        }
        int brc = prt_gpu_place_copies(c->stream, d_xf.as<float>(), d_box.as<float>(), d_im.as<uint32_t>(), m.tlas_inst.as<uint32_t>(),
                                       n_total, n_world, m.insts.p, d_recs.as<float4>());
        float root_box[6];
        if (!brc)
            brc = prt_gpu_bvh8_refit_top(c->stream, m.nodes8.as<uint32_t>(), stride * 4u, old_top, level_nodes.data(), level_start.data(),
                                         (uint32_t)level_start.size() - 1u, d_recs.as<float4>(), root_box);
        if (brc && brc != -6) return broken(hipSuccess, brc);
        if (!brc) {
            prt_commit_instances(&hs, up, instances);
            // the host copies follow the device: the re-quantized top level and the instance table
            e = hipMemcpy2D(hs.nodes8_all.data(), 80, c->scene.nodes8.p, node_bytes, 80, old_top, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(hs.dev_insts.data(), c->scene.insts.p, (size_t)n_total * sizeof(DevInstance), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return broken(e, 0);
            fill_dev_scene(c, stride, hs.bvh_info.depth8);
            if (mesh_lights_on(c) && (rc = upload_mesh_lights(c))) return rc;
            return done(PRT_INSTANCES_REFIT);
        }
        top_dirty = true;  // a box did not fit its node's grid: a new topology it is
    }
    rc = prt_build_top_level(opt, hs, &up, &hs.gpu_build_ms, &c->err);
    if (rc) {
        if (top_dirty) {  // the scene stays what it was: the refit's half-written top level and instances go back
            e = hipMemcpy2D(c->scene.nodes8.p, node_bytes, hs.nodes8_all.data(), 80, 80, old_top, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(c->scene.insts.p, hs.dev_insts.data(), (size_t)n_total * sizeof(DevInstance), hipMemcpyHostToDevice);
            if (e != hipSuccess) return broken(e, 0);
        }
        return rc;
    }
    const uint32_t new_top = (uint32_t)(up.top_nodes8.size() / 20), delta = new_top - old_top, new_all = n_all - old_top + new_top;
    uint32_t* d_n8 = m.nodes8.as<uint32_t>();
    if (delta) {  // the mesh trees move behind the new top level, device to device
        e = (hipError_t)d_new.ensure(node_bytes * new_all);
        if (e == hipSuccess && stride != 5u) e = hipMemset(d_new.p, 0, node_bytes * new_top);
        if (e == hipSuccess)
            e = hipMemcpy(d_new.as<char>() + node_bytes * new_top, m.nodes8.as<char>() + node_bytes * old_top, node_bytes * (n_all - old_top),
                          hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {  // (the scene is still whole unless the refit wrote to it)
            if (top_dirty) return broken(e, 0);
            return fail(c, PRT_ERR_HIP, "prt_set_instance_transforms: %s", hipGetErrorString(e));
        }
        d_n8 = d_new.as<uint32_t>();
    }
    e = hipMemcpy2D(d_n8, node_bytes, up.top_nodes8.data(), 80, 80, new_top, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->scene.tlas_inst.p, up.top_order.data(), (size_t)n_total * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();  // (copies on the null stream return early; the kernels run on c->stream)
    if (e != hipSuccess) return broken(e, 0);
    int brc = prt_gpu_place_copies(c->stream, d_xf.as<float>(), d_box.as<float>(), d_im.as<uint32_t>(), m.tlas_inst.as<uint32_t>(), n_total,
                                   n_world, m.insts.p, d_recs.as<float4>());
    if (!brc && delta) brc = prt_gpu_rebase(c->stream, d_n8, stride * 4u, new_top, new_all, m.insts.p, n_total, delta);
    e = hipStreamSynchronize(c->stream);
    if (brc || e != hipSuccess) return broken(e, brc);
    if (delta) m.nodes8 = std::move(d_new);
    prt_commit_top_level(&hs, up);
    prt_commit_instances(&hs, up, instances);
    e = hipMemcpy(hs.dev_insts.data(), c->scene.insts.p, (size_t)n_total * sizeof(DevInstance), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return broken(e, 0);
    fill_dev_scene(c, stride, hs.bvh_info.depth8);
    if (mesh_lights_on(c) && (rc = upload_mesh_lights(c))) return rc;
    return done(PRT_INSTANCES_REBUILD);
}

int prt_instance_update_info(PrtContext* c, PrtInstanceUpdateInfo* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    *out = c->inst_info;
    out->top_nodes = c->hs.top_nodes;
    out->top_depth = c->hs.top_depth;
    return PRT_OK;
}

int prt_instances_read(PrtContext* c, uint32_t capacity, uint32_t* n_instances, uint32_t* slot_instance, uint32_t* root, uint32_t* slot_base,
                       uint32_t* prim_base) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    const uint32_t n = (uint32_t)c->hs.dev_insts.size();
    if (n_instances) *n_instances = n;
    for (uint32_t k = 0; k < n && k < capacity; ++k) {
        const DevInstance& I = c->hs.dev_insts[k];
        if (slot_instance) slot_instance[k] = c->hs.tlas_inst[k];
        if (root) root[k] = I.root;
        if (slot_base) slot_base[k] = I.slot_base;
        if (prim_base) prim_base[k] = I.prim_base;
    }
    return PRT_OK;
}

int prt_set_camera(PrtContext* c, const PrtCameraDesc* cam) {
    if (!c || !cam) return PRT_ERR_INVALID;
    c->feat_valid = false;
    touch_camera(c);
    if (!(cam->width > 0.0f) || !(cam->height > 0.0f)) return fail(c, PRT_ERR_INVALID, "camera width/height must be > 0");
    DevCamera& k = c->cam;
    k.pos = f3{cam->position[0], cam->position[1], cam->position[2]};
    k.front = h_normalize(f3{cam->front[0], cam->front[1], cam->front[2]});
    k.right = h_normalize(h_cross(k.front, f3{0.0f, 1.0f, 0.0f}));
    k.up = h_normalize(h_cross(k.right, k.front));
    k.W = cam->width;
    k.H = cam->height;
    k.tan_fov_y = lens_tan_fov_y(c->lens);
    c->has_camera = true;
    return PRT_OK;
}

int prt_set_lens(PrtContext* c, const PrtLens* lens) {
    if (!c) return PRT_ERR_INVALID;
    c->feat_valid = false;
    touch_camera(c);  // (the field of view is the camera's)
    const PrtLens l = lens ? *lens : PrtLens{0.0f, 0.0f, 0.0f};
    if (std::isnan(l.fov_y) || std::isnan(l.aperture) || std::isnan(l.focus_distance))
        return fail(c, PRT_ERR_INVALID, "bad lens: NaN");
    if (l.fov_y < 0.0f || !(l.fov_y < 3.14159265358979323846f))  // (the fp32 nearest to pi is above pi: refused as well)
        return fail(c, PRT_ERR_INVALID, "bad lens: fov_y must be 0 (the default, 1 rad) or in (0, pi)");
    if (l.aperture < 0.0f || !std::isfinite(l.aperture)) return fail(c, PRT_ERR_INVALID, "bad lens: aperture must be finite and >= 0");
    if (l.aperture > 0.0f && (!std::isfinite(l.focus_distance) || !(l.focus_distance > 0.0f)))
        return fail(c, PRT_ERR_INVALID, "bad lens: aperture > 0 needs a finite focus_distance > 0");
    c->lens = l;
    c->cam.tan_fov_y = lens_tan_fov_y(l);  // (prt_set_camera writes the rest, and this again)
    return PRT_OK;
}

int prt_get_lens(PrtContext* c, PrtLens* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    *out = c->lens;
    return PRT_OK;
}

int prt_set_film(PrtContext* c, uint32_t width, uint32_t height, uint32_t rank, uint32_t world) {
    if (!c) return PRT_ERR_INVALID;
    c->feat_valid = false;
    touch_scene(c);  // (the tile map is in the key as well)
    drop_history(c);
    if (width == 0 || height == 0 || world == 0 || rank >= world)
        return fail(c, PRT_ERR_INVALID, "bad film size or partition (%ux%u, rank %u of %u)", width, height, rank, world);
    if ((uint64_t)width * height > 0x7FFFFFFFull) return fail(c, PRT_ERR_INVALID, "film too large");
    PrtTileMap& tm = c->tm;
    tm.W = width;
    tm.H = height;
    tm.tiles_x = (width + 7) / 8;
    tm.tiles_y = (height + 7) / 8;
    tm.rank = rank;
    tm.world = world;
    const uint32_t tiles = tm.tiles_x * tm.tiles_y;
    tm.n_tiles_local = tiles > rank ? (tiles - rank + world - 1) / world : 0;
    tm.n_pix_local = tm.n_tiles_local * 64;
    tm.stride = ((tiles + world - 1) / world) * 64;
    uint32_t valid = 0;
    for (uint32_t lt = 0; lt < tm.n_tiles_local; ++lt) {
        const uint32_t gt = lt * world + rank;
        const uint32_t tx = gt % tm.tiles_x, ty = gt / tm.tiles_x;
        const uint32_t w = std::min(8u, width - tx * 8), h = std::min(8u, height - ty * 8);
        valid += w * h;
    }
    c->valid_local = valid;
    c->has_film = true;
    c->pix_records_blank = false;  // (the records' place in wk.pix depends on the pixel count)
    if (!c->has_device) return PRT_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    c->film.local = DevBuf();
    c->film.stat = DevBuf();
    HIPCHECK(c, c->film.local.ensure(std::max<size_t>((size_t)tm.stride, 64) * sizeof(float4)));
    if (c->film_stats) HIPCHECK(c, c->film.stat.ensure(std::max<size_t>((size_t)tm.stride, 64) * sizeof(float2)));
    int rc = ensure_counters(c);
    if (rc) return rc;
    return prt_film_clear(c);
}

int prt_film_clear(PrtContext* c) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_film) return fail(c, PRT_ERR_INVALID, "prt_set_film has not been called");
    HIPCHECK(c, hipMemsetAsync(c->film.local.p, 0, std::max<size_t>((size_t)c->tm.stride, 64) * sizeof(float4), c->stream));
    if (c->film.stat.p)
        HIPCHECK(c, hipMemsetAsync(c->film.stat.p, 0, std::max<size_t>((size_t)c->tm.stride, 64) * sizeof(float2), c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_set_film_statistics(PrtContext* c, int on) {
    if (!c) return PRT_ERR_INVALID;
    const bool want = on != 0;
    if (want == c->film_stats) return PRT_OK;
    touch_scene(c);
    c->film_stats = want;
    drop_history(c);
    if (!c->has_device) return PRT_OK;  // host-only: the setting is all there is
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    c->film.stat = DevBuf();
    if (!c->has_film) return PRT_OK;  // (prt_set_film allocates the moments with the film)
    if (want) HIPCHECK(c, c->film.stat.ensure(std::max<size_t>((size_t)c->tm.stride, 64) * sizeof(float2)));
    return prt_film_clear(c);
}

int prt_get_film_statistics(const PrtContext* c) { return (c && c->film_stats) ? 1 : 0; }

int prt_set_sampling(PrtContext* c, const PrtSampling* sp) {
    if (!c) return PRT_ERR_INVALID;
    if (sp && (sp->jitter > 1u || sp->rr_depth > PRT_MAX_DEPTH || !(sp->clamp >= 0.0f)))
        return fail(c, PRT_ERR_INVALID, "bad sampling options");
    touch_scene(c);
    const PrtSampling ns = sp ? *sp : PrtSampling{0u, 0u, 0.0f};
    if (c->fsamp.samples > 0u && ns.jitter != c->sampling.jitter) c->feat_valid = false;  // the sampled set's rays are the render's
    c->sampling = ns;
    return PRT_OK;
}

int prt_set_samples_in_flight(PrtContext* c, uint32_t n) {
    if (!c || n == 0 || n > 1024) return fail(c, PRT_ERR_INVALID, "samples in flight must be 1..1024");
    c->S = n;
    return PRT_OK;
}

int prt_set_lighting(PrtContext* c, const PrtLighting* l) {
    if (!c) return PRT_ERR_INVALID;
    if (l && l->mode != PRT_LIGHTING_OFF && l->mode != PRT_LIGHTING_NEE_MIS && l->mode != PRT_LIGHTING_NEE)
        return fail(c, PRT_ERR_INVALID, "bad lighting mode %u", l->mode);
    touch_scene(c);
    c->lighting = l ? l->mode : (uint32_t)PRT_LIGHTING_OFF;
    return PRT_OK;
}

int prt_set_light_sources(PrtContext* c, uint32_t mask) {
    if (!c) return PRT_ERR_INVALID;
    if (mask != (uint32_t)PRT_LIGHT_SOURCES_ANALYTIC && mask != (uint32_t)(PRT_LIGHT_SOURCES_ANALYTIC | PRT_LIGHT_SOURCES_MESH))
        return fail(c, PRT_ERR_INVALID, "light sources: PRT_LIGHT_SOURCES_ANALYTIC or ANALYTIC | MESH, not %u", mask);
    const bool was_on = mesh_lights_on(c);
    touch_scene(c);
    c->light_sources = mask;
    if (!c->has_device || !c->has_scene || was_on == mesh_lights_on(c)) return PRT_OK;
    if (mesh_lights_on(c)) return upload_mesh_lights(c);
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    c->ml = MeshLightMem();
    return PRT_OK;
}

int prt_set_light_selection(PrtContext* c, const PrtLightSelection* sel) {
    if (!c) return PRT_ERR_INVALID;
    const PrtLightSelection s = sel ? *sel : PrtLightSelection{PRT_LIGHT_SELECTION_POWER, 0u};
    if (s.mode != (uint32_t)PRT_LIGHT_SELECTION_POWER && s.mode != (uint32_t)PRT_LIGHT_SELECTION_CLUSTERED)
        return fail(c, PRT_ERR_INVALID, "light selection: PRT_LIGHT_SELECTION_POWER or CLUSTERED, not %u", s.mode);
    if (s.max_clusters > PRT_LIGHT_MAX_CLUSTERS)
        return fail(c, PRT_ERR_INVALID, "light selection: at most %u clusters, not %u", PRT_LIGHT_MAX_CLUSTERS, s.max_clusters);
    touch_scene(c);
    c->light_selection = s.mode;
    c->light_max_clusters = s.max_clusters;
    const uint32_t K = s.max_clusters ? s.max_clusters : 32u;
    if (!c->has_scene || c->hs.lc.max_clusters == K) return PRT_OK;
    if (c->has_device && mesh_lights_on(c)) {  // (nothing in flight reads the tables that are about to go)
        HIPCHECK(c, hipSetDevice(c->device));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
    }
    prt_build_light_clusters(&c->hs, K);
    if (c->has_device && mesh_lights_on(c)) return upload_mesh_lights(c);
    return PRT_OK;
}

int prt_light_cluster_info(PrtContext* c, PrtLightClusterInfo* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    out->mode = c->light_selection;
    out->active = clusters_on(c) ? 1u : 0u;
    out->max_clusters = c->light_max_clusters ? c->light_max_clusters : 32u;
    if (!c->has_scene) return PRT_OK;
    out->n_clusters = c->hs.lc.n_clusters();
    out->n_empty_inner = c->hs.lc.n_empty_inner;
    return PRT_OK;
}

int prt_light_clusters(PrtContext* c, uint32_t capacity, uint32_t* n_clusters, float* lo, float* hi, float* r2, float* phi,
                       uint64_t* power_width, uint32_t* n_members) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    const PrtLightClusters& lc = c->hs.lc;
    if (n_clusters) *n_clusters = lc.n_clusters();
    for (uint32_t k = 0; k < lc.n_clusters() && k < capacity; ++k) {
        const float* b = &lc.boxes[8 * (size_t)k];
        if (lo) memcpy(&lo[3 * k], b, 12);
        if (hi) memcpy(&hi[3 * k], b + 4, 12);
        if (phi) phi[k] = b[3];
        if (r2) r2[k] = b[7];
        if (power_width) power_width[k] = lc.power_width[k];
        if (n_members) n_members[k] = lc.range[4 * (size_t)k + 2];
    }
    return PRT_OK;
}

int prt_light_cluster_members(PrtContext* c, uint32_t capacity, uint32_t* n_lights, uint32_t* cluster, uint64_t* inner_width) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    const PrtMeshLights& ml = c->hs.ml;
    const PrtLightClusters& lc = c->hs.lc;
    const uint32_t n = (uint32_t)ml.visible.size();
    if (n_lights) *n_lights = n;
    for (uint32_t l = 0; l < n && l < capacity; ++l) {
        const uint32_t cand = ml.visible[l];
        if (cluster) cluster[l] = lc.cand_cluster[cand];
        if (inner_width) inner_width[l] = lc.inner_width[lc.cand_member[cand]];
    }
    return PRT_OK;
}

int prt_light_cluster_pmf(PrtContext* c, uint32_t n, const float* x, uint32_t* M) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (!mesh_lights_on(c)) return fail(c, PRT_ERR_INVALID, "prt_light_cluster_pmf: the cluster tables are on the device only with PRT_LIGHT_SOURCES_MESH");
    const uint32_t K = c->hs.lc.n_clusters();
    if (!K) return fail(c, PRT_ERR_INVALID, "prt_light_cluster_pmf: the scene has no light");
    if (n == 0) return PRT_OK;
    if (!x || !M) return fail(c, PRT_ERR_INVALID, "null array");
    const size_t n3 = 3 * (size_t)n, nK = (size_t)n * K;
    float* d_x;
    uint32_t* d_m;
    PrtWorkspace ws;
    ws.add(&d_x, n3).add(&d_m, nK);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_x, x, n3))) return rc;
    prt_launch_light_cluster_pmf(c->stream, dev_light_clusters(c), n, d_x, d_m);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, M, d_m, nK))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_set_environment(PrtContext* c, const PrtEnvironment* e) {
    if (!c) return PRT_ERR_INVALID;
    touch_scene(c);
    PrtEnvTables t;  // (built aside: a refused image leaves the context's environment as it was)
    if (e) {
        const int rc = prt_build_environment(e, &t, &c->err);
        if (rc) return rc;
    }
    if (c->has_device) {
        const int rc = need_device(c);
        if (rc) return rc;
        HIPCHECK(c, hipStreamSynchronize(c->stream));
    }
    c->env = std::move(t);
    if (!c->has_device) return PRT_OK;
    const int rc = upload_env(c);
    if (rc) return rc;
    return c->has_scene ? sync_light_tables(c) : PRT_OK;
}

int prt_set_textures(PrtContext* c, const PrtTextureSet* set) {
    if (!c) return PRT_ERR_INVALID;
    c->feat_valid = false;
    touch_scene(c);
    drop_history(c);
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_textures: prt_set_scene has not been called");
    PrtTexTables t;  // (built aside: a refused set leaves the context's binding as it was)
    if (set) {
        const int rc = prt_build_textures(c->hs, set, &t, &c->err);
        if (rc) return rc;
    }
    c->tex = std::move(t);
    if (!c->has_device) return PRT_OK;
    const int rc = upload_tex(c);
    if (rc) {  // a HIP failure midway: no binding rather than half of one
        free_tex(c);
        c->tex = PrtTexTables();
    }
    return rc;
}

int prt_texture_info(PrtContext* c, PrtTextureInfo* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    *out = PrtTextureInfo{};
    if (!c->tex.is_set) return PRT_OK;
    out->is_set = 1u;
    out->n_textures = c->tex.n_textures;
    out->n_textured_materials = c->tex.n_textured_materials;
    out->n_uv_triangles = (uint32_t)(c->tex.uvs.size() / 6);
    out->n_texels = c->tex.texels.size() / 4;
    out->device_bytes = c->tex_bytes;
    return PRT_OK;
}

int prt_texture_eval(PrtContext* c, uint32_t n, const uint32_t* texture, const float* uv, float* rgb) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->tex.is_set) return fail(c, PRT_ERR_INVALID, "prt_texture_eval: no textures are bound");
    if (n == 0) return PRT_OK;
    if (!texture || !uv || !rgb) return fail(c, PRT_ERR_INVALID, "null array");
    for (uint32_t i = 0; i < n; ++i) {
        if (texture[i] >= c->tex.n_textures) return fail(c, PRT_ERR_INVALID, "prt_texture_eval: texture %u out of range (pair %u)", texture[i], i);
        for (int k = 0; k < 2; ++k)
            if (!std::isfinite(uv[2 * (size_t)i + k]) || std::fabs(uv[2 * (size_t)i + k]) > 1048576.0f)
                return fail(c, PRT_ERR_INVALID, "prt_texture_eval: uv %u is not finite or above 2^20", i);
    }
    const size_t n1 = n;
    uint32_t* d_t;
    float *d_u, *d_r;
    PrtWorkspace ws;
    ws.add(&d_t, n1).add(&d_u, 2 * n1).add(&d_r, 3 * n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_t, texture, n1)) || (rc = upload(c, d_u, uv, 2 * n1))) return rc;
    prt_launch_texture_eval(c->stream, dev_tex(c), n, d_t, d_u, d_r);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, rgb, d_r, 3 * n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_environment_info(PrtContext* c, PrtEnvironmentInfo* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    if (!env_on(c)) return PRT_OK;
    out->is_set = 1u;
    out->width = c->env.W;
    out->height = c->env.H;
    out->n_sampled = c->env.n_sampled;
    out->t_env = env_threshold(c);
    out->light_share = c->env.light_share;
    return PRT_OK;
}

int prt_environment_intervals(PrtContext* c, uint64_t* row_width, uint64_t* col_width) {
    if (!c) return PRT_ERR_INVALID;
    if (!env_on(c)) return fail(c, PRT_ERR_INVALID, "prt_environment_intervals: no environment is set");
    if (c->env.row_width.empty()) return fail(c, PRT_ERR_INVALID, "prt_environment_intervals: an all-black map has no distribution");
    if (row_width) memcpy(row_width, c->env.row_width.data(), c->env.row_width.size() * sizeof(uint64_t));
    if (col_width) memcpy(col_width, c->env.col_width.data(), c->env.col_width.size() * sizeof(uint64_t));
    return PRT_OK;
}

int prt_environment_eval(PrtContext* c, uint32_t n, const float* dirs, float* rgb, uint32_t* texel, float* pdf_w) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!env_on(c)) return fail(c, PRT_ERR_INVALID, "prt_environment_eval: no environment is set");
    if (n == 0) return PRT_OK;
    if (!dirs) return fail(c, PRT_ERR_INVALID, "null array");
    const size_t n1 = n;
    float *d_d, *d_rgb, *d_p;
    uint32_t* d_t;
    PrtWorkspace ws;
    ws.add(&d_d, 3 * n1).add(&d_rgb, 3 * n1).add(&d_t, n1).add(&d_p, n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_d, dirs, 3 * n1))) return rc;
    prt_launch_environment_eval(c->stream, dev_env(c), n, d_d, d_rgb, d_t, d_p);
    HIPCHECK(c, hipGetLastError());
    if (rgb && (rc = download(c, rgb, d_rgb, 3 * n1))) return rc;
    if (texel && (rc = download(c, texel, d_t, n1))) return rc;
    if (pdf_w && (rc = download(c, pdf_w, d_p, n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_light_intervals(PrtContext* c, uint32_t capacity, uint32_t* n_lights, uint64_t* width) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (!mesh_lights_on(c)) return fail(c, PRT_ERR_INVALID, "prt_light_intervals: the default light sources have no thresholds");
    const uint32_t n = (uint32_t)c->hs.ml.visible.size();
    if (n_lights) *n_lights = n;
    const uint64_t te = env_threshold(c);  // (T_e > 0: the exact product with 2^32 - T_e, in units of 2^-64)
    for (uint32_t l = 0; l < n && l < capacity && width; ++l) width[l] = te ? c->hs.ml.width[l] * (4294967296ull - te) : c->hs.ml.width[l];
    return PRT_OK;
}

int prt_light_info(PrtContext* c, uint32_t capacity, uint32_t* n_lights, uint32_t* prim, float* pmf) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    std::vector<float> lights_s, records_s;  // (the pmfs with the environment's factor: what the kernels use)
    prt_scaled_light_tables(c->hs, env_threshold(c), mesh_lights_on(c) ? nullptr : &lights_s, mesh_lights_on(c) ? &records_s : nullptr);
    if (mesh_lights_on(c)) {
        const PrtMeshLights& ml = c->hs.ml;
        const uint32_t nv = (uint32_t)ml.visible.size();
        if (n_lights) *n_lights = nv;
        for (uint32_t l = 0; l < nv && l < capacity; ++l) {
            const float* r = &records_s[4 * PRT_LIGHT_F4 * (size_t)ml.visible[l]];
            if (prim) memcpy(&prim[l], &r[19], 4);
            if (pmf) pmf[l] = r[7];
        }
        return PRT_OK;
    }
    const uint32_t n = (uint32_t)(c->hs.lights.size() / (4 * PRT_LIGHT_F4));
    if (n_lights) *n_lights = n;
    for (uint32_t l = 0; l < n && l < capacity; ++l) {
        const float* r = &lights_s[4 * PRT_LIGHT_F4 * l];
        if (prim) memcpy(&prim[l], &r[19], 4);
        if (pmf) pmf[l] = r[7];
    }
    return PRT_OK;
}

int prt_get_light_stats(PrtContext* c, PrtLightStats* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    out->n_lights = light_set_size(c);
    out->n_emitters_unsampled = mesh_lights_on(c) ? c->hs.ml.n_emitters_unsampled : c->hs.n_emitters_unsampled;
    if (clusters_on(c)) out->n_emitters_unsampled += c->hs.lc.n_empty_inner;
    if (!c->has_device || !c->wk.light_stats.p) return PRT_OK;
    int rc = need_device(c);
    if (rc) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> h(kLightStatWords);
    HIPCHECK(c, hipMemcpy(h.data(), c->wk.light_stats.p, kLightStatWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t sl = 0; sl < PRT_RAY_STAT_SLOTS; ++sl) {
        out->shadow_rays += h[2 * sl];
        out->shadow_occluded += h[2 * sl + 1];
    }
    return PRT_OK;
}

int prt_render_async(PrtContext* c, uint32_t spp, uint32_t max_depth, uint32_t seed, uint32_t first_sample) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (max_depth == 0 || max_depth > PRT_MAX_DEPTH) return fail(c, PRT_ERR_INVALID, "max_depth must be 1..%d", PRT_MAX_DEPTH);
    HIPCHECK(c, hipSetDevice(c->device));
    uint32_t done = 0;
    while (done < spp) {
        const uint32_t S_cur = std::min(c->S, spp - done);
        rc = run_batch(c, whole_film(c), S_cur, max_depth, seed, first_sample + done, true, nullptr);
        if (rc) return rc;
        done += S_cur;
    }
    return PRT_OK;
}

int prt_synchronize(PrtContext* c) {
    int rc = need_device(c);
    if (rc) return rc;
    // (the flag's copy is enqueued behind the kernels and ONE wait covers both: a blocking copy after the wait was a second
    // host round trip, ~30 us of a 0.9 ms one-sample call)
    if (c->wk.work.p && !c->wk.flag.p) {
        HIPCHECK(c, c->wk.flag.alloc(64));
        *c->wk.flag.as<uint32_t>() = 0u;
    }
    if (c->wk.work.p) HIPCHECK(c, hipMemcpyAsync(c->wk.flag.p, c->wk.work.as<uint32_t>() + 256, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if (c->wk.work.p) {  // watchdog flag of the persistent traversal kernel
        const uint32_t w = *c->wk.flag.as<uint32_t>();
        if (w) {
            HIPCHECK(c, hipMemset(c->wk.work.p, 0, 2052));
            return fail(c, PRT_ERR_HIP, w & 2u ? "traversal stack-overflow list full" : "traversal watchdog tripped: a wave exceeded its iteration cap");
        }
    }
    return PRT_OK;
}

int prt_render(PrtContext* c, uint32_t spp, uint32_t max_depth, uint32_t seed, uint32_t first_sample) {
    int rc = prt_render_async(c, spp, max_depth, seed, first_sample);
    if (rc) return rc;
    return prt_synchronize(c);
}

int prt_film_local(PrtContext* c, void** d_ptr, uint64_t* n_floats) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_film) return fail(c, PRT_ERR_INVALID, "prt_set_film has not been called");
    if (d_ptr) *d_ptr = c->film.local.as<float4>();
    if (n_floats) *n_floats = (uint64_t)c->tm.stride * 4;
    return PRT_OK;
}

int prt_film_resolve_on(PrtContext* c, void* hip_stream, const void* d_gathered, uint32_t world, void* d_rgb, void* d_weight) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_film || !d_gathered || !d_rgb || !d_weight || world != c->tm.world)
        return fail(c, PRT_ERR_INVALID, "bad arguments to prt_film_resolve");
    HIPCHECK(c, hipSetDevice(c->device));
    prt_launch_resolve(hip_stream ? (hipStream_t)hip_stream : c->stream, (const float4*)d_gathered, world, c->tm.stride, c->tm.W,
                       c->tm.H, (float*)d_rgb, (float*)d_weight);
    HIPCHECK(c, hipGetLastError());
    return PRT_OK;
}

int prt_film_resolve(PrtContext* c, const void* d_gathered, uint32_t world, void* d_rgb, void* d_weight) {
    return prt_film_resolve_on(c, nullptr, d_gathered, world, d_rgb, d_weight);
}

int prt_film_tonemap(PrtContext* c, const void* d_rgb, const void* d_weight, float exposure, float gamma, void* d_rgba8) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_film || !d_rgb || !d_weight || !d_rgba8) return fail(c, PRT_ERR_INVALID, "bad arguments to prt_film_tonemap");
    prt_launch_tonemap(c->stream, (const float*)d_rgb, (const float*)d_weight, c->tm.W * c->tm.H, exposure, 1.0f / gamma,
                       (uint8_t*)d_rgba8);
    HIPCHECK(c, hipGetLastError());
    return PRT_OK;
}

// Builds [world][stride] with only this rank's payload filled, resolves it, and leaves rgb / weight in scratch.
static int resolve_own(PrtContext* c, float** d_rgb, float** d_w, uint8_t** d_rgba) {
    const PrtTileMap& tm = c->tm;
    const size_t npix = (size_t)tm.W * tm.H;
    const size_t gathered = (size_t)tm.world * tm.stride * sizeof(float4);
    const size_t off_rgb = (gathered + 255) & ~(size_t)255;
    const size_t off_w = off_rgb + ((npix * 12 + 255) & ~(size_t)255);
    const size_t off_b = off_w + ((npix * 4 + 255) & ~(size_t)255);
    int rc = ensure(c, c->scratch, off_b + npix * 4);
    if (rc) return rc;
    char* base = (char*)c->scratch.p;
    HIPCHECK(c, hipMemsetAsync(base, 0, gathered, c->stream));
    HIPCHECK(c, hipMemcpyAsync(base + (size_t)tm.rank * tm.stride * sizeof(float4), c->film.local.as<float4>(),
                               (size_t)tm.stride * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    *d_rgb = (float*)(base + off_rgb);
    *d_w = (float*)(base + off_w);
    *d_rgba = (uint8_t*)(base + off_b);
    prt_launch_resolve(c->stream, (const float4*)base, tm.world, tm.stride, tm.W, tm.H, *d_rgb, *d_w);
    HIPCHECK(c, hipGetLastError());
    return PRT_OK;
}

int prt_film_read(PrtContext* c, float* rgb_sum, float* weight) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_film) return fail(c, PRT_ERR_INVALID, "prt_set_film has not been called");
    float *d_rgb, *d_w;
    uint8_t* d_b;
    if ((rc = resolve_own(c, &d_rgb, &d_w, &d_b))) return rc;
    const size_t npix = (size_t)c->tm.W * c->tm.H;
    if (rgb_sum) HIPCHECK(c, hipMemcpyAsync(rgb_sum, d_rgb, npix * 12, hipMemcpyDeviceToHost, c->stream));
    if (weight) HIPCHECK(c, hipMemcpyAsync(weight, d_w, npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_film_statistics_read(PrtContext* c, float* sum_y, float* sum_y2) {
    std::vector<float> stat;
    int rc = read_local_moments(c, nullptr, &stat);
    if (rc) return rc;
    const size_t npix = (size_t)c->tm.W * c->tm.H;
    if (sum_y) std::fill(sum_y, sum_y + npix, 0.0f);
    if (sum_y2) std::fill(sum_y2, sum_y2 + npix, 0.0f);
    for_each_local_pixel(c->tm, [&](size_t pl, size_t p) {
        if (sum_y) sum_y[p] = stat[2 * pl];
        if (sum_y2) sum_y2[p] = stat[2 * pl + 1];
    });
    return PRT_OK;
}

int prt_film_noise_read(PrtContext* c, float noise_floor, float* rel_err) {
    if (!c) return PRT_ERR_INVALID;
    if (!(noise_floor >= 0.0f) || !rel_err) return fail(c, PRT_ERR_INVALID, "bad arguments to prt_film_noise_read");
    std::vector<float> film, stat;
    int rc = read_local_moments(c, &film, &stat);
    if (rc) return rc;
    const size_t npix = (size_t)c->tm.W * c->tm.H;
    std::fill(rel_err, rel_err + npix, std::numeric_limits<float>::infinity());
    for_each_local_pixel(c->tm, [&](size_t pl, size_t p) {
        const float n = film[4 * pl + 3];
        if (n < 2.0f) return;
        const double dn = (double)n, m = (double)stat[2 * pl] / dn;
        const double d = (double)stat[2 * pl + 1] / dn - m * m;
        const double V = d > 0.0 ? d : 0.0;
        rel_err[p] = (float)(std::sqrt(V / (dn - 1.0)) / (m + (double)noise_floor));
    });
    return PRT_OK;
}

int prt_adaptive_unconverged(float n, float A, float Q, float threshold, float noise_floor) {
    return prt_adaptive_rule(n, A, Q, threshold, noise_floor) ? 1 : 0;
}

int prt_render_adaptive(PrtContext* c, const PrtAdaptive* cfg, uint32_t max_depth, uint32_t seed, uint32_t first_sample,
                        PrtAdaptiveInfo* out) {
    if (!c) return PRT_ERR_INVALID;
    if (!cfg) return fail(c, PRT_ERR_INVALID, "prt_render_adaptive: null settings");
    if (!c->film_stats) return fail(c, PRT_ERR_INVALID, "prt_render_adaptive needs film statistics (prt_set_film_statistics)");
    if (!(cfg->threshold >= 0.0f) || !(cfg->noise_floor >= 0.0f))
        return fail(c, PRT_ERR_INVALID, "threshold and noise_floor must be >= 0 (and not NaN)");
    if (cfg->threshold == 0.0f && cfg->noise_floor == 0.0f) return fail(c, PRT_ERR_INVALID, "threshold and noise_floor are both 0");
    if (cfg->max_spp < cfg->min_spp) return fail(c, PRT_ERR_INVALID, "max_spp < min_spp");
    if (cfg->step_spp == 0u && cfg->max_spp > cfg->min_spp) return fail(c, PRT_ERR_INVALID, "step_spp is 0 with max_spp > min_spp");
    if (max_depth == 0 || max_depth > PRT_MAX_DEPTH) return fail(c, PRT_ERR_INVALID, "max_depth must be 1..%d", PRT_MAX_DEPTH);
    int rc = check_ready(c);
    if (rc) return rc;
    HIPCHECK(c, hipSetDevice(c->device));
    PrtAdaptiveInfo info{};
    const uint32_t n_tiles = c->tm.n_tiles_local;
    info.tiles_local = n_tiles;
    if (out) *out = info;
    // count words, flags and two lists of n_tiles entries each; the pinned words the count is read into
    if (c->tile_sel_entries < n_tiles || !c->film.tile_sel.p) {
        c->tile_sel_entries = 0;
        HIPCHECK(c, c->film.tile_sel.ensure((16 + 3 * (size_t)std::max(n_tiles, 1u)) * sizeof(uint32_t)));
        c->tile_sel_entries = std::max(n_tiles, 1u);
    }
    if (!c->film.tile_count.p) HIPCHECK(c, c->film.tile_count.alloc(64));
    uint32_t* d_count = c->film.tile_sel.as<uint32_t>();
    uint32_t* d_flags = c->film.tile_sel.as<uint32_t>() + 16;
    uint32_t* d_list[2] = {d_flags + c->tile_sel_entries, d_flags + 2 * (size_t)c->tile_sel_entries};
    uint32_t added = 0;
    if (cfg->min_spp) {  // pass 0: every tile, the ordinary route
        if ((rc = prt_render_async(c, cfg->min_spp, max_depth, seed, first_sample))) return rc;
        added = cfg->min_spp;
        info.pixel_samples = (uint64_t)cfg->min_spp * c->valid_local;
    }
    const uint32_t* prev = nullptr;
    uint32_t n_prev = n_tiles, cur = 0;
    bool any = false;
    auto stopped_at = [&](uint32_t spp) {
        info.min_tile_spp = any ? std::min(info.min_tile_spp, spp) : spp;
        info.max_tile_spp = any ? std::max(info.max_tile_spp, spp) : spp;
        any = true;
    };
    while (n_prev) {
        // which of the tiles that were active until now still are; ONE small wait per pass for their number
        prt_launch_tile_select(c->stream, c->film.local.as<float4>(), c->film.stat.as<float2>(), c->tm, prev, n_prev, cfg->threshold, cfg->noise_floor,
                               d_flags, d_list[cur], d_count);
        HIPCHECK(c, hipGetLastError());
        HIPCHECK(c, hipMemcpyAsync(c->film.tile_count.p, d_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        const uint32_t n_act = c->film.tile_count.as<uint32_t>()[0], pix_act = c->film.tile_count.as<uint32_t>()[1];
        if (n_act > n_prev) return fail(c, PRT_ERR_HIP, "tile selection returned %u of %u tiles", n_act, n_prev);
        if (n_act < n_prev) {
            info.tiles_converged += n_prev - n_act;
            stopped_at(added);
        }
        if (n_act == 0u) break;
        if (added >= cfg->max_spp) {
            info.tiles_capped = n_act;
            stopped_at(added);
            break;
        }
        const uint32_t k = std::min(cfg->step_spp, cfg->max_spp - added);
        PrtBatchView view{c->tm, d_list[cur]};
        view.tm.n_tiles_local = n_act;
        view.tm.n_pix_local = n_act * 64u;
        for (uint32_t done = 0; done < k;) {  // split by samples_in_flight as prt_render splits
            const uint32_t S_cur = std::min(c->S, k - done);
            if ((rc = run_batch(c, view, S_cur, max_depth, seed, first_sample + added + done, true, nullptr))) return rc;
            done += S_cur;
        }
        added += k;
        info.pixel_samples += (uint64_t)k * pix_act;
        ++info.passes;
        prev = d_list[cur];
        n_prev = n_act;
        cur ^= 1u;
    }
    if (out) *out = info;
    return prt_synchronize(c);
}

int prt_film_display(PrtContext* c, float exposure, float gamma, uint8_t* rgba8) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_film || !rgba8) return fail(c, PRT_ERR_INVALID, "bad arguments to prt_film_display");
    float *d_rgb, *d_w;
    uint8_t* d_b;
    if ((rc = resolve_own(c, &d_rgb, &d_w, &d_b))) return rc;
    const uint32_t npix = c->tm.W * c->tm.H;
    prt_launch_tonemap(c->stream, d_rgb, d_w, npix, exposure, 1.0f / gamma, d_b);
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipMemcpyAsync(rgba8, d_b, (size_t)npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// ---- function-level entry points ------------------------------------------------------------------
int prt_camera_rays(PrtContext* c, uint32_t n, const float* px, const float* py, float* origins, float* dirs) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_camera) return fail(c, PRT_ERR_INVALID, "prt_set_camera has not been called");
    if (n == 0) return PRT_OK;
    if (!px || !py || !origins || !dirs) return fail(c, PRT_ERR_INVALID, "null array");
    const size_t n1 = n;
    float *d_px, *d_py, *d_o, *d_d;
    PrtWorkspace ws;
    ws.add(&d_px, n1).add(&d_py, n1).add(&d_o, 3 * n1).add(&d_d, 3 * n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_px, px, n1)) || (rc = upload(c, d_py, py, n1))) return rc;
    prt_launch_camera_rays(c->stream, c->cam, n, d_px, d_py, d_o, d_d);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, origins, d_o, 3 * n1)) || (rc = download(c, dirs, d_d, 3 * n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_camera_rays_lens(PrtContext* c, uint32_t n, const float* px, const float* py, uint32_t* keys, float* origins,
                         float* dirs) {
    if (c && !(c->lens.aperture > 0.0f)) return prt_camera_rays(c, n, px, py, origins, dirs);  // pinhole: no draw, keys left alone
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_camera) return fail(c, PRT_ERR_INVALID, "prt_set_camera has not been called");
    if (n == 0) return PRT_OK;
    if (!px || !py || !keys || !origins || !dirs) return fail(c, PRT_ERR_INVALID, "null array");
    const size_t n1 = n;
    float *d_px, *d_py, *d_o, *d_d;
    uint32_t* d_keys;
    PrtWorkspace ws;
    ws.add(&d_px, n1).add(&d_py, n1).add(&d_keys, n1).add(&d_o, 3 * n1).add(&d_d, 3 * n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_px, px, n1)) || (rc = upload(c, d_py, py, n1)) || (rc = upload(c, d_keys, keys, n1))) return rc;
    prt_launch_camera_rays_lens(c->stream, c->cam, DevLens{c->lens.aperture, c->lens.focus_distance}, n, d_px, d_py, d_keys, d_o, d_d);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, keys, d_keys, n1)) || (rc = download(c, origins, d_o, 3 * n1)) || (rc = download(c, dirs, d_d, 3 * n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// The ray-query pipeline on the context's stream, from device arrays (n x 3 origins / directions): closest hit
// (d_tmax == nullptr: PrtHit records into d_hits) or occlusion (one byte per ray into d_occ).  No host wait.
static int enqueue_query(PrtContext* c, uint32_t n, const float* d_o, const float* d_d, const float* d_tmax, PrtHit* d_hits,
                         uint8_t* d_occ) {
    int rc;
    if ((rc = ensure_path_state(c, n))) return rc;
    if ((rc = ensure_counters(c))) return rc;
    if ((rc = ensure_spill(c))) return rc;
    uint32_t* cnt = c->wk.counts.as<uint32_t>() + (size_t)(PRT_MAX_DEPTH + 1) * PRT_CNT_STRIDE;  // a counter slot the render loop never uses
    if (d_tmax) {
        // occlusion: every ray seeded with "miss at d2 = tmax^2", the analytic scan from that bound, the any-hit walk
        // (or, with another traversal variant forced, the closest hit, which k_occlusion_bytes compares with the bound)
        prt_launch_pack_occlusion_rays(c->stream, n, d_o, d_d, d_tmax, c->rb[0], cnt);
        prt_launch_scan_prims_bounded(c->stream, c->dsc, c->rb[0], cnt, c->wk.work.as<uint32_t>(), n);
    } else {
        prt_launch_pack_rays(c->stream, n, d_o, d_d, c->rb[0], cnt);
        prt_launch_scan_prims(c->stream, c->dsc, c->rb[0], cnt, c->wk.work.as<uint32_t>(), n, nullptr);
    }
    if (c->dsc.n_nodes) walk_rays(c, c->rb[0], cnt, n, d_tmax != nullptr, c->tune, nullptr, nullptr);
    if (d_tmax) prt_launch_occlusion_bytes(c->stream, c->dsc, n, c->rb[0], d_tmax, d_occ);
    else prt_launch_hit_records(c->stream, c->dsc, n, c->rb[0], d_hits);
    HIPCHECK(c, hipGetLastError());
    return PRT_OK;
}

int prt_closest_hit(PrtContext* c, uint32_t n, const float* origins, const float* dirs, PrtHit* hits) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (n == 0) return PRT_OK;
    if (!origins || !dirs || !hits) return fail(c, PRT_ERR_INVALID, "null array");
    const size_t n1 = n;
    float *d_o, *d_d;
    PrtHit* d_h;
    PrtWorkspace ws;
    ws.add(&d_o, 3 * n1).add(&d_d, 3 * n1).add(&d_h, n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_o, origins, 3 * n1)) || (rc = upload(c, d_d, dirs, 3 * n1))) return rc;
    if ((rc = enqueue_query(c, n, d_o, d_d, nullptr, d_h, nullptr))) return rc;
    if ((rc = download(c, hits, d_h, n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_hit_uv(PrtContext* c, uint32_t n, const float* origins, const float* dirs, PrtHit* hits, float* uv, float* albedo) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (!c->tex.is_set) return fail(c, PRT_ERR_INVALID, "prt_hit_uv: no textures are bound");
    if (n == 0) return PRT_OK;
    if (!origins || !dirs) return fail(c, PRT_ERR_INVALID, "null array");
    const size_t n1 = n;
    float *d_o, *d_d, *d_uv, *d_a;
    PrtHit* d_h;
    PrtWorkspace ws;
    ws.add(&d_o, 3 * n1).add(&d_d, 3 * n1).add(&d_h, n1).add(&d_uv, 2 * n1).add(&d_a, 3 * n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_o, origins, 3 * n1)) || (rc = upload(c, d_d, dirs, 3 * n1))) return rc;
    if ((rc = enqueue_query(c, n, d_o, d_d, nullptr, d_h, nullptr))) return rc;
    prt_launch_hit_uv(c->stream, c->dsc, dev_tex(c), n, c->rb[0], d_uv, d_a);  // (the query left rays and final hit ids in rb[0])
    HIPCHECK(c, hipGetLastError());
    if (hits && (rc = download(c, hits, d_h, n1))) return rc;
    if (uv && (rc = download(c, uv, d_uv, 2 * n1))) return rc;
    if (albedo && (rc = download(c, albedo, d_a, 3 * n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_closest_hit_device(PrtContext* c, uint32_t n, const void* d_origins, const void* d_dirs, void* d_hits) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (n == 0) return PRT_OK;
    if (!d_origins || !d_dirs || !d_hits) return fail(c, PRT_ERR_INVALID, "null array");
    return enqueue_query(c, n, (const float*)d_origins, (const float*)d_dirs, nullptr, (PrtHit*)d_hits, nullptr);
}

int prt_occluded(PrtContext* c, uint32_t n, const float* origins, const float* dirs, const float* tmax, uint8_t* occluded) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (n == 0) return PRT_OK;
    if (!origins || !dirs || !tmax || !occluded) return fail(c, PRT_ERR_INVALID, "null array");
    const size_t n1 = n;
    float *d_o, *d_d, *d_t;
    uint8_t* d_b;
    PrtWorkspace ws;
    ws.add(&d_o, 3 * n1).add(&d_d, 3 * n1).add(&d_t, n1).add(&d_b, n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_o, origins, 3 * n1)) || (rc = upload(c, d_d, dirs, 3 * n1)) || (rc = upload(c, d_t, tmax, n1))) return rc;
    if ((rc = enqueue_query(c, n, d_o, d_d, d_t, nullptr, d_b))) return rc;
    if ((rc = download(c, occluded, d_b, n1))) return rc;
    // waits for the stream and reports a ray the walk had to give up (two-level stack overflow): never a silent "not occluded"
    return prt_synchronize(c);
}

int prt_occluded_device(PrtContext* c, uint32_t n, const void* d_origins, const void* d_dirs, const void* d_tmax,
                        void* d_occluded) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (n == 0) return PRT_OK;
    if (!d_origins || !d_dirs || !d_tmax || !d_occluded) return fail(c, PRT_ERR_INVALID, "null array");
    return enqueue_query(c, n, (const float*)d_origins, (const float*)d_dirs, (const float*)d_tmax, nullptr,
                         (uint8_t*)d_occluded);
}

// ---- first-hit features and the film denoiser (include/prt.h) ---------------------------------------
void prt_denoise_defaults(PrtDenoise* out) {
    if (out) *out = prt_denoise_default_config();
}

float prt_denoise_variance(float n, float A, float Q) { return prt_denoise_variance_rule(n, A, Q); }

// The specular chains of n rays (d_o, d_d) whose closest hits are in d_h (and whose textured albedo is in d_a, or null): the
// start kernel decides every ray at k = 0 from those records (nothing is traced twice) and leaves the live chains in list 1;
// each round reads the 4-byte live count (one small wait, as prt_render_adaptive has per pass), queries the live rays only,
// and steps them into the other list.  After round r every live chain has followed r + 2 vertices, so round
// max_specular - 1 ends them all.  Ray i's records go to out[i].  d_o, d_d, d_h and d_a are overwritten.
static int enqueue_chains(PrtContext* c, uint32_t n, float* d_o, float* d_d, PrtHit* d_h, float* d_a, const ChainScratch& x,
                          PrtFeatureBufs out) {
    int rc;
    PrtChainList lists[2] = {{d_o, d_d, x.s[0], x.s[1]}, {x.o, x.d, x.s[2], x.s[3]}};
    uint32_t* d_cnt = x.cnt;
    HIPCHECK(c, hipMemsetAsync(d_cnt, 0, (PRT_FEATURE_MAX_SPECULAR + 1u) * sizeof(uint32_t), c->stream));
    PrtChainArgs a{d_h, d_a, c->dsc.mat_rgbs, c->dsc.mat_type, c->ftrace, out, d_cnt};
    prt_launch_ft_start(c->stream, n, d_d, a, lists[1]);
    HIPCHECK(c, hipGetLastError());
    int cur = 1;
    for (uint32_t r = 0; r < c->ftrace.max_specular; ++r) {
        uint32_t live = 0;
        HIPCHECK(c, hipMemcpyAsync(&live, d_cnt + r, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        if (live == 0u) break;
        if (live > n) return fail(c, PRT_ERR_HIP, "prt_render_features: live count %u above %u rays", live, n);
        if ((rc = enqueue_query(c, live, lists[cur].o, lists[cur].d, nullptr, d_h, nullptr))) return rc;
        if (d_a) prt_launch_hit_uv(c->stream, c->dsc, dev_tex(c), live, c->rb[0], nullptr, d_a);
        a.count = d_cnt + r + 1;
        prt_launch_ft_step(c->stream, live, lists[cur], a, lists[cur ^ 1]);
        HIPCHECK(c, hipGetLastError());
        cur ^= 1;
    }
    return PRT_OK;
}

// The sampled set (include/prt.h "Sampled guide features") of the n = W x H pixels, after the other sets are enqueued.
// Degenerate (no jitter, no lens): a copy of the centre-ray set.  Otherwise chunks of whole samples: the render's primary
// rays of the chunk, sample-major; the ray-query pipeline and the per-ray records exactly as above, with the slot in the
// place of the pixel (following: the chain kernels write every slot's record, so the first-hit pack is not needed); the
// ordered reduce into the set's own records; the finish after the last chunk.
static int enqueue_feature_samples(PrtContext* c, uint32_t n) {
    int rc;
    const uint32_t K = c->fsamp.samples;
    const bool follow = c->ftrace.max_specular > 0u;
    if ((rc = ensure(c, c->samp, 3 * (size_t)n * sizeof(float4)))) return rc;
    const PrtFeatureBufs samp = feature_view(c->samp.p, n);
    if (c->sampling.jitter == 0u && !(c->lens.aperture > 0.0f)) {
        const PrtFeatureBufs src = feature_view(follow ? c->guide.p : c->feat.p, n);
        prt_launch_fs_finish(c->stream, n, K, &src, samp);
        HIPCHECK(c, hipGetLastError());
        return PRT_OK;
    }
    // samples per chunk: about 2^22 rays unless a chunk size is forced, never more than 2^28 rays, at least one sample
    uint32_t cs = c->feature_chunk > 0 ? (uint32_t)c->feature_chunk : std::max<uint32_t>(1u, (1u << 22) / n);
    cs = std::min(std::min(cs, K), std::max<uint32_t>(1u, (uint32_t)PRT_DENOISE_MAX_PIXELS / n));
    const uint32_t m = cs * n;
    // the scratch below and the path state of m rays may be reallocated: nothing enqueued above may still be using them
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    const size_t m1 = m;
    float *d_o, *d_d, *d_a;
    PrtHit* d_h;
    float4* d_r;
    ChainScratch chain;
    PrtWorkspace ws;
    ws.add(&d_o, 3 * m1).add(&d_d, 3 * m1).add(&d_a, 3 * m1).add(&d_h, m1).add(&d_r, 3 * m1);
    if (follow) chain.declare(ws, m1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    const bool textured = tex_on(c);
    const DevLens dlens{c->lens.aperture, c->lens.focus_distance};
    for (uint32_t s0 = 0; s0 < K; s0 += cs) {
        const PrtSampleChunk ch{c->tm.W, c->tm.H, s0, std::min(cs, K - s0), c->fsamp.first_sample, c->fsamp.seed, c->sampling.jitter};
        const uint32_t mc = ch.cs * n;
        const PrtFeatureBufs rec = feature_view(d_r, mc);
        prt_launch_fs_rays(c->stream, c->cam, dlens, ch, d_o, d_d);
        HIPCHECK(c, hipGetLastError());
        if ((rc = enqueue_query(c, mc, d_o, d_d, nullptr, d_h, nullptr))) return rc;
        if (textured) prt_launch_hit_uv(c->stream, c->dsc, dev_tex(c), mc, c->rb[0], nullptr, d_a);
        if (follow) {
            if ((rc = enqueue_chains(c, mc, d_o, d_d, d_h, textured ? d_a : nullptr, chain, rec))) return rc;
        } else {
            prt_launch_dn_pack_features(c->stream, mc, d_h, textured ? d_a : nullptr, c->dsc.mat_rgbs, c->dsc.mat_type, rec);
        }
        prt_launch_fs_reduce(c->stream, ch, rec, samp);
        HIPCHECK(c, hipGetLastError());
    }
    prt_launch_fs_finish(c->stream, n, K, nullptr, samp);
    HIPCHECK(c, hipGetLastError());
    return PRT_OK;
}

int prt_render_features(PrtContext* c) {
    int rc = check_ready(c);
    if (rc) return rc;
    c->feat_valid = false;
    c->guide_valid = false;
    const PrtTileMap& tm = c->tm;
    const uint64_t n64 = (uint64_t)tm.W * tm.H;
    if (n64 > (uint64_t)PRT_DENOISE_MAX_PIXELS) return fail(c, PRT_ERR_INVALID, "prt_render_features: more than 2^28 pixels");
    const uint32_t n = (uint32_t)n64;
    const bool follow = c->ftrace.max_specular > 0u;
    const size_t n1 = n;
    if (follow && (rc = ensure(c, c->guide, 3 * n1 * sizeof(float4)))) return rc;
    if ((rc = ensure(c, c->feat, 3 * n1 * sizeof(float4)))) return rc;
    // one pinhole ray through every pixel centre (k_camera_rays: fov_y honoured, no lens, no draw), the ray-query pipeline
    // of prt_closest_hit_device, the textured albedo of prt_hit_uv while a binding textures something, then the records
    float *d_px, *d_py, *d_o, *d_d, *d_a;
    PrtHit* d_h;
    ChainScratch chain;
    PrtWorkspace ws;
    ws.add(&d_px, n1).add(&d_py, n1).add(&d_o, 3 * n1).add(&d_d, 3 * n1).add(&d_h, n1).add(&d_a, 3 * n1);
    if (follow) chain.declare(ws, n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    prt_launch_dn_pixel_grid(c->stream, tm.W, tm.H, d_px, d_py);
    prt_launch_camera_rays(c->stream, c->cam, n, d_px, d_py, d_o, d_d);
    HIPCHECK(c, hipGetLastError());
    if ((rc = enqueue_query(c, n, d_o, d_d, nullptr, d_h, nullptr))) return rc;
    const bool textured = tex_on(c);
    if (textured) prt_launch_hit_uv(c->stream, c->dsc, dev_tex(c), n, c->rb[0], nullptr, d_a);  // (rays and final hit ids are in rb[0])
    prt_launch_dn_pack_features(c->stream, n, d_h, textured ? d_a : nullptr, c->dsc.mat_rgbs, c->dsc.mat_type, feature_view(c->feat.p, n1));
    HIPCHECK(c, hipGetLastError());
    if (follow && (rc = enqueue_chains(c, n, d_o, d_d, d_h, textured ? d_a : nullptr, chain, feature_view(c->guide.p, n1)))) return rc;
    if (c->fsamp.samples > 0u && (rc = enqueue_feature_samples(c, n))) return rc;
    if ((rc = prt_synchronize(c))) return rc;
    c->feat_W = tm.W;
    c->feat_H = tm.H;
    c->feat_valid = true;
    c->guide_valid = follow;
    c->samp_valid = c->fsamp.samples > 0u;
    return PRT_OK;
}

void prt_feature_trace_defaults(PrtFeatureTrace* out) {
    if (out) *out = PrtFeatureTrace{0u, 0.1f};
}

int prt_set_feature_trace(PrtContext* c, const PrtFeatureTrace* ft) {
    if (!c) return PRT_ERR_INVALID;
    c->feat_valid = false;
    c->guide_valid = false;
    const PrtFeatureTrace t = ft ? *ft : PrtFeatureTrace{0u, 0.1f};
    if (t.max_specular > PRT_FEATURE_MAX_SPECULAR) return fail(c, PRT_ERR_INVALID, "bad feature trace: max_specular must be 0..8");
    if (!std::isfinite(t.roughness_max) || t.roughness_max < 0.0f)
        return fail(c, PRT_ERR_INVALID, "bad feature trace: roughness_max must be finite and >= 0");
    c->ftrace = t;
    return PRT_OK;
}

int prt_get_feature_trace(PrtContext* c, PrtFeatureTrace* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    *out = c->ftrace;
    return PRT_OK;
}

void prt_feature_sampling_defaults(PrtFeatureSampling* out) {
    if (out) *out = PrtFeatureSampling{0u, 0u, 0u};
}

int prt_set_feature_sampling(PrtContext* c, const PrtFeatureSampling* fs) {
    if (!c) return PRT_ERR_INVALID;
    c->feat_valid = false;
    c->guide_valid = false;
    c->samp_valid = false;
    const PrtFeatureSampling t = fs ? *fs : PrtFeatureSampling{0u, 0u, 0u};
    if (t.samples > PRT_FEATURE_MAX_SAMPLES) return fail(c, PRT_ERR_INVALID, "bad feature sampling: samples must be 0..64");
    c->fsamp = t;
    return PRT_OK;
}

int prt_get_feature_sampling(PrtContext* c, PrtFeatureSampling* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    *out = c->fsamp;
    return PRT_OK;
}

// A set as the last prt_render_features wrote it.
static PrtFeatureBufs current_set(const PrtContext* c, const DevBuf& set) { return feature_view(set.p, (size_t)c->feat_W * c->feat_H); }
// The centre-ray set the guide readers return: the guide set while that mode is on, else the first-hit set.
static PrtFeatureBufs centre_features(const PrtContext* c) { return current_set(c, c->guide_valid ? c->guide : c->feat); }
// The set the spatial filter is guided by: the sampled set while that mode is on, else the centre-ray set.
static PrtFeatureBufs filter_features(const PrtContext* c) { return c->samp_valid ? current_set(c, c->samp) : centre_features(c); }

// A feature set's records to planar host arrays (each may be null); bounces: the albedo record's .w.
static int read_feature_records(PrtContext* c, PrtFeatureBufs f, float* albedo, float* normal, float* position, float* depth, int32_t* prim,
                                uint32_t* bounces) {
    if (!c->feat_valid) return fail(c, PRT_ERR_INVALID, "no current feature set (prt_render_features)");
    int rc = need_device(c);
    if (rc) return rc;
    const size_t n = (size_t)c->feat_W * c->feat_H;
    std::vector<float> rec(12 * n);
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    HIPCHECK(c, hipMemcpy(rec.data(), f.alb, 3 * n * sizeof(float4), hipMemcpyDeviceToHost));
    const float *a = rec.data(), *nr = rec.data() + 4 * n, *ps = rec.data() + 8 * n;
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) {
            if (albedo) albedo[3 * i + k] = a[4 * i + k];
            if (normal) normal[3 * i + k] = nr[4 * i + k];
            if (position) position[3 * i + k] = ps[4 * i + k];
        }
        if (depth) depth[i] = ps[4 * i + 3];
        if (prim) memcpy(&prim[i], &nr[4 * i + 3], sizeof(int32_t));
        if (bounces) bounces[i] = (uint32_t)a[4 * i + 3];
    }
    return PRT_OK;
}

int prt_features_read_guide(PrtContext* c, float* albedo, float* normal, float* position, float* depth, int32_t* prim, uint32_t* bounces) {
    if (!c) return PRT_ERR_INVALID;
    return read_feature_records(c, centre_features(c), albedo, normal, position, depth, prim, bounces);
}

int prt_features_read_sampled(PrtContext* c, float* albedo, float* normal, float* position, float* depth, int32_t* prim, uint32_t* hits) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->feat_valid || !c->samp_valid) return fail(c, PRT_ERR_INVALID, "no current sampled feature set (prt_set_feature_sampling, prt_render_features)");
    return read_feature_records(c, current_set(c, c->samp), albedo, normal, position, depth, prim, hits);
}

int prt_features_read(PrtContext* c, float* albedo, float* normal, float* position, float* depth, int32_t* prim) {
    if (!c) return PRT_ERR_INVALID;
    return read_feature_records(c, current_set(c, c->feat), albedo, normal, position, depth, prim, nullptr);
}

// The iterations and the finish on the context's stream.  cv[0] holds c_0 / var_0; cv[0] and cv[1] ping-pong.
static int enqueue_filter(PrtContext* c, const PrtDenoise& cfg, uint32_t W, uint32_t H, PrtFeatureBufs f, float4* cv0, float4* cv1,
                          float* d_out, float* d_var_out) {
    float4* cv[2] = {cv0, cv1};
    int cur = 0;
    for (uint32_t i = 0; i < cfg.iterations; ++i) {
        const PrtAtrousParams p{W, H, 1u << i, cfg.sigma_l, cfg.sigma_z, cfg.normal_power_log2};
        const bool staged = (c->dn_lds == 1 && p.step == 1u) || (c->dn_lds == 2 && p.step <= 2u);
        if (!(staged && prt_launch_dn_atrous_lds(c->stream, p, cv[cur], f, cv[cur ^ 1])))
            prt_launch_dn_atrous(c->stream, p, cv[cur], f, cv[cur ^ 1]);
        cur ^= 1;
    }
    prt_launch_dn_finish(c->stream, W * H, cv[cur], f, cfg.demodulate, d_out, d_var_out);
    HIPCHECK(c, hipGetLastError());
    return PRT_OK;
}

// prt_denoise_device's work; s: declare_arrays for W x H pixels
static int enqueue_denoise_arrays(PrtContext* c, const PrtDenoise& cfg, uint32_t W, uint32_t H, const float* d_mean, const float* d_var,
                                  const float* d_albedo, const float* d_normal, const float* d_position, const int32_t* d_prim,
                                  float* d_out, float* d_var_out, const FilterScratch& s) {
    const uint32_t n = W * H;
    const PrtFeatureBufs f = feature_view(s.rec, n);
    prt_launch_dn_pack_arrays(c->stream, n, d_albedo, d_normal, d_position, d_prim, f);
    prt_launch_dn_prepare(c->stream, n, d_mean, d_var, f, cfg.demodulate, s.cv0);
    return enqueue_filter(c, cfg, W, H, f, s.cv0, s.cv1, d_out, d_var_out);
}

int prt_denoise_device(PrtContext* c, const PrtDenoise* cfg, uint32_t W, uint32_t H, const void* d_mean, const void* d_var,
                       const void* d_albedo, const void* d_normal, const void* d_position, const void* d_prim, void* d_out,
                       void* d_var_out) {
    if (!c) return PRT_ERR_INVALID;
    const char* bad = prt_denoise_check(cfg, W, H, d_mean && d_var && d_albedo && d_normal && d_position && d_prim && d_out);
    if (bad) return fail(c, PRT_ERR_INVALID, "%s", bad);
    int rc = need_device(c);
    if (rc) return rc;
    const PrtDenoise k = cfg ? *cfg : prt_denoise_default_config();
    const size_t n = (size_t)W * H;
    FilterScratch s;
    PrtWorkspace ws;
    s.declare_arrays(ws, n);
    if ((rc = commit(c, ws, c->dn))) return rc;
    return enqueue_denoise_arrays(c, k, W, H, (const float*)d_mean, (const float*)d_var, (const float*)d_albedo, (const float*)d_normal,
                                  (const float*)d_position, (const int32_t*)d_prim, (float*)d_out, (float*)d_var_out, s);
}

int prt_denoise(PrtContext* c, const PrtDenoise* cfg, uint32_t W, uint32_t H, const float* mean, const float* var, const float* albedo,
                const float* normal, const float* position, const int32_t* prim, float* out, float* var_out) {
    if (!c) return PRT_ERR_INVALID;
    const char* bad = prt_denoise_check(cfg, W, H, mean && var && albedo && normal && position && prim && out);
    if (bad) return fail(c, PRT_ERR_INVALID, "%s", bad);
    int rc = need_device(c);
    if (rc) return rc;
    const PrtDenoise k = cfg ? *cfg : prt_denoise_default_config();
    const size_t n = (size_t)W * H;
    // workspace: the filter's, then the staged arrays
    FilterScratch s;
    float *d_mean, *d_alb, *d_nrm, *d_pos, *d_out, *d_var, *d_vout;
    int32_t* d_prim;
    PrtWorkspace ws;
    s.declare_arrays(ws, n);
    ws.add(&d_mean, 3 * n).add(&d_alb, 3 * n).add(&d_nrm, 3 * n).add(&d_pos, 3 * n).add(&d_out, 3 * n);
    ws.add(&d_var, n).add(&d_prim, n).add(&d_vout, n);
    if ((rc = commit(c, ws, c->dn))) return rc;
    if ((rc = upload(c, d_mean, mean, 3 * n)) || (rc = upload(c, d_var, var, n)) || (rc = upload(c, d_alb, albedo, 3 * n))) return rc;
    if ((rc = upload(c, d_nrm, normal, 3 * n)) || (rc = upload(c, d_pos, position, 3 * n)) || (rc = upload(c, d_prim, prim, n))) return rc;
    if ((rc = enqueue_denoise_arrays(c, k, W, H, d_mean, d_var, d_alb, d_nrm, d_pos, d_prim, d_out, var_out ? d_vout : nullptr, s))) return rc;
    if ((rc = download(c, out, d_out, 3 * n))) return rc;
    if (var_out && (rc = download(c, var_out, d_vout, n))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_film_denoise(PrtContext* c, const PrtDenoise* cfg, float* rgb_out, float* var_out) {
    if (!c) return PRT_ERR_INVALID;
    const char* bad = prt_denoise_check(cfg, 1u, 1u, rgb_out != nullptr);
    if (bad) return fail(c, PRT_ERR_INVALID, "%s", bad);
    if (!c->film_stats) return fail(c, PRT_ERR_INVALID, "prt_film_denoise: film statistics are off (prt_set_film_statistics)");
    if (c->has_film && c->tm.world != 1u)
        return fail(c, PRT_ERR_INVALID,
                    "prt_film_denoise: this context owns rank %u of %u of the image; the gathered film is filtered by prt_group_film_denoise",
                    c->tm.rank, c->tm.world);
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->film.stat.p) return fail(c, PRT_ERR_INVALID, "prt_film_denoise: film statistics are off (prt_set_film_statistics)");
    const PrtTileMap& tm = c->tm;
    if ((uint64_t)tm.W * tm.H > (uint64_t)PRT_DENOISE_MAX_PIXELS) return fail(c, PRT_ERR_INVALID, "denoise: more than 2^28 pixels");
    if (!c->feat_valid && (rc = prt_render_features(c))) return rc;
    const PrtDenoise k = cfg ? *cfg : prt_denoise_default_config();
    const size_t n = (size_t)tm.W * tm.H;
    FilterScratch s;
    if ((rc = s.commit_film(c, n))) return rc;
    const PrtFeatureBufs gf = filter_features(c);
    prt_launch_dn_film_prepare(c->stream, tm, c->film.local.as<float4>(), c->film.stat.as<float2>(), gf, k.demodulate, s.cv0);
    if ((rc = enqueue_filter(c, k, tm.W, tm.H, gf, s.cv0, s.cv1, s.out, var_out ? s.var : nullptr))) return rc;
    if ((rc = download(c, rgb_out, s.out, 3 * n))) return rc;
    if (var_out && (rc = download(c, var_out, s.var, n))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// ---- temporal reprojection (include/prt.h) -----------------------------------------------------------
void prt_temporal_defaults(PrtTemporal* out) {
    if (out) *out = prt_temporal_default_config();
}

int prt_get_camera_basis(PrtContext* c, PrtCameraBasis* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    if (!c->has_camera) return fail(c, PRT_ERR_INVALID, "prt_set_camera has not been called");
    const DevCamera& k = c->cam;
    *out = PrtCameraBasis{{k.pos.x, k.pos.y, k.pos.z}, {k.right.x, k.right.y, k.right.z}, {k.up.x, k.up.y, k.up.z},
                          {k.front.x, k.front.y, k.front.z}, k.W, k.H, k.tan_fov_y};
    return PRT_OK;
}

int prt_temporal_reset(PrtContext* c) {
    if (!c) return PRT_ERR_INVALID;
    drop_history(c);
    return PRT_OK;
}

int prt_temporal_info(PrtContext* c, PrtTemporalInfo* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    *out = c->tp_info;
    out->device_bytes = (uint64_t)c->tp.bytes + c->tp_mt.bytes + c->tpa.bytes;
    return PRT_OK;
}

// prt_temporal_reproject_device's work; s: declared for W x H pixels
static int enqueue_temporal_arrays(PrtContext* c, const PrtTemporal& cfg, uint32_t W, uint32_t H, const PrtCameraBasis& K, const float* d_c,
                                   const float* d_n, const float* d_A, const float* d_Q, const int32_t* d_prim, const float* d_P,
                                   const float* d_N, const float* d_hc, const float* d_hn, const float* d_h1, const float* d_h2,
                                   const float* d_hP, const float* d_hN, const int32_t* d_hprim, float* d_c_out, float* d_n_out,
                                   float* d_m1_out, float* d_m2_out, float* d_var_out, uint8_t* d_status, const TemporalScratch& s) {
    const size_t n = (size_t)W * H;
    const PrtHistoryBufs cur = s.cur, next = s.next;
    PrtHistoryBufs prev = s.prev;
    prt_launch_tp_pack_frame(c->stream, (uint32_t)n, d_c, d_n, d_A, d_Q, d_prim, d_P, d_N, cur.cn, cur.mm, cur.nrm, cur.pos);
    if (d_hc) prt_launch_tp_pack_frame(c->stream, (uint32_t)n, d_hc, d_hn, d_h1, d_h2, d_hprim, d_hP, d_hN, prev.cn, prev.mm, prev.nrm, prev.pos);
    else prev = PrtHistoryBufs{nullptr, nullptr, nullptr, nullptr};
    prt_launch_tp_reproject(c->stream, W, H, cfg, K, PrtTemporalFrame{cur.cn, cur.mm, cur.nrm, cur.pos}, prev, next, d_c_out, d_var_out, d_status,
                            nullptr);
    prt_launch_tp_unpack(c->stream, (uint32_t)n, next, d_n_out, d_m1_out, d_m2_out);
    HIPCHECK(c, hipGetLastError());
    return PRT_OK;
}

int prt_temporal_reproject_device(PrtContext* c, const PrtTemporal* cfg, uint32_t W, uint32_t H, const PrtCameraBasis* K, const void* d_c,
                                  const void* d_n, const void* d_A, const void* d_Q, const void* d_prim, const void* d_Pprev,
                                  const void* d_Nprev, const void* d_hc, const void* d_hn, const void* d_h1, const void* d_h2,
                                  const void* d_hP, const void* d_hN, const void* d_hprim, void* d_c_out, void* d_n_out, void* d_m1_out,
                                  void* d_m2_out, void* d_var_out, void* d_status) {
    if (!c) return PRT_ERR_INVALID;
    const bool hist_ok = !d_hc || (d_hn && d_h1 && d_h2 && d_hP && d_hN && d_hprim);
    const char* bad = prt_temporal_check(cfg, W, H, K, K && d_c && d_n && d_A && d_Q && d_prim && d_Pprev && d_Nprev && hist_ok && d_c_out &&
                                                            d_n_out && d_m1_out && d_m2_out);
    if (bad) return fail(c, PRT_ERR_INVALID, "%s", bad);
    int rc = need_device(c);
    if (rc) return rc;
    const PrtTemporal k = cfg ? *cfg : prt_temporal_default_config();
    const size_t n = (size_t)W * H;
    TemporalScratch s;
    PrtWorkspace ws;
    s.declare(ws, n);
    if ((rc = commit(c, ws, c->tpa))) return rc;
    return enqueue_temporal_arrays(c, k, W, H, *K, (const float*)d_c, (const float*)d_n, (const float*)d_A, (const float*)d_Q,
                                   (const int32_t*)d_prim, (const float*)d_Pprev, (const float*)d_Nprev, (const float*)d_hc, (const float*)d_hn,
                                   (const float*)d_h1, (const float*)d_h2, (const float*)d_hP, (const float*)d_hN, (const int32_t*)d_hprim,
                                   (float*)d_c_out, (float*)d_n_out, (float*)d_m1_out, (float*)d_m2_out, (float*)d_var_out, (uint8_t*)d_status,
                                   s);
}

int prt_temporal_reproject(PrtContext* c, const PrtTemporal* cfg, uint32_t W, uint32_t H, const PrtCameraBasis* K, const float* cc,
                           const float* nn, const float* A, const float* Q, const int32_t* prim, const float* Pprev, const float* Nprev,
                           const float* hc, const float* hn, const float* h1, const float* h2, const float* hP, const float* hN,
                           const int32_t* hprim, float* c_out, float* n_out, float* m1_out, float* m2_out, float* var_out, uint8_t* status) {
    if (!c) return PRT_ERR_INVALID;
    const bool hist_ok = !hc || (hn && h1 && h2 && hP && hN && hprim);
    const char* bad =
        prt_temporal_check(cfg, W, H, K, K && cc && nn && A && Q && prim && Pprev && Nprev && hist_ok && c_out && n_out && m1_out && m2_out);
    if (bad) return fail(c, PRT_ERR_INVALID, "%s", bad);
    int rc = need_device(c);
    if (rc) return rc;
    const PrtTemporal k = cfg ? *cfg : prt_temporal_default_config();
    const size_t n = (size_t)W * H;
    // workspace: the records, then the staged arrays: the frame, the history, the outputs
    TemporalScratch s;
    float *d_c, *d_P, *d_N, *d_n, *d_A, *d_Q, *d_hc, *d_hP, *d_hN, *d_hn, *d_h1, *d_h2, *d_co, *d_no, *d_m1o, *d_m2o, *d_vo;
    int32_t *d_prim, *d_hprim;
    uint8_t* d_st;
    PrtWorkspace ws;
    s.declare(ws, n);
    ws.add(&d_c, 3 * n).add(&d_P, 3 * n).add(&d_N, 3 * n).add(&d_n, n).add(&d_A, n).add(&d_Q, n).add(&d_prim, n);
    ws.add(&d_hc, 3 * n).add(&d_hP, 3 * n).add(&d_hN, 3 * n).add(&d_hn, n).add(&d_h1, n).add(&d_h2, n).add(&d_hprim, n);
    ws.add(&d_co, 3 * n).add(&d_no, n).add(&d_m1o, n).add(&d_m2o, n).add(&d_vo, n).add(&d_st, n);
    if ((rc = commit(c, ws, c->tpa))) return rc;
    if ((rc = upload(c, d_c, cc, 3 * n)) || (rc = upload(c, d_P, Pprev, 3 * n)) || (rc = upload(c, d_N, Nprev, 3 * n))) return rc;
    if ((rc = upload(c, d_n, nn, n)) || (rc = upload(c, d_A, A, n)) || (rc = upload(c, d_Q, Q, n)) || (rc = upload(c, d_prim, prim, n))) return rc;
    if (hc) {
        if ((rc = upload(c, d_hc, hc, 3 * n)) || (rc = upload(c, d_hP, hP, 3 * n)) || (rc = upload(c, d_hN, hN, 3 * n))) return rc;
        if ((rc = upload(c, d_hn, hn, n)) || (rc = upload(c, d_h1, h1, n)) || (rc = upload(c, d_h2, h2, n)) || (rc = upload(c, d_hprim, hprim, n))) return rc;
    }
    if ((rc = enqueue_temporal_arrays(c, k, W, H, *K, d_c, d_n, d_A, d_Q, d_prim, d_P, d_N, hc ? d_hc : nullptr, d_hn, d_h1, d_h2, d_hP, d_hN,
                                      d_hprim, d_co, d_no, d_m1o, d_m2o, var_out ? d_vo : nullptr, status ? d_st : nullptr, s)))
        return rc;
    if ((rc = download(c, c_out, d_co, 3 * n)) || (rc = download(c, n_out, d_no, n))) return rc;
    if ((rc = download(c, m1_out, d_m1o, n)) || (rc = download(c, m2_out, d_m2o, n))) return rc;
    if (var_out && (rc = download(c, var_out, d_vo, n))) return rc;
    if (status && (rc = download(c, status, d_st, n))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_temporal_prev_surface(PrtContext* c, uint32_t n, const float* position, const float* normal, const int32_t* prim,
                              const PrtInstance* prev_instances, uint32_t n_prev, float* Pprev, float* Nprev) {
    if (!c) return PRT_ERR_INVALID;
    if (!position || !normal || !prim || !Pprev || !Nprev || (n_prev && !prev_instances)) return fail(c, PRT_ERR_INVALID, "temporal: null array");
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    const PrtHostScene& hs = c->hs;
    const uint32_t n_copies = (uint32_t)hs.dev_insts.size() - hs.n_world_insts;
    if (n_prev && n_prev != n_copies)
        return fail(c, PRT_ERR_INVALID, "prt_temporal_prev_surface: %u previous transforms for a scene of %u placed copies", n_prev, n_copies);
    std::vector<uint32_t> range(2 * (size_t)n_prev);
    std::vector<float> prev(12 * (size_t)n_prev);
    for (uint32_t k = 0; k < n_prev; ++k) {
        const DevInstance& I = hs.dev_insts[hs.n_world_insts + k];
        range[2 * (size_t)k] = I.prim_base;
        range[2 * (size_t)k + 1] = I.n_tris;
        for (int col = 0; col < 4; ++col)
            for (int r = 0; r < 3; ++r) prev[12 * (size_t)k + col * 3 + r] = prev_instances[k].mat[col * 4 + r];
    }
    for (uint32_t i = 0; i < n; ++i) {
        PrtTpV3 P{position[3 * (size_t)i], position[3 * (size_t)i + 1], position[3 * (size_t)i + 2]};
        PrtTpV3 N{normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2]};
        const int32_t k = prt_temporal_find_copy(range.data(), n_prev, prim[i]);
        if (k >= 0) prt_temporal_prev_surface_rule(hs.dev_insts[hs.n_world_insts + (uint32_t)k].inv, &prev[12 * (size_t)k], P, N, &P, &N);
        Pprev[3 * (size_t)i] = P.x, Pprev[3 * (size_t)i + 1] = P.y, Pprev[3 * (size_t)i + 2] = P.z;
        Nprev[3 * (size_t)i] = N.x, Nprev[3 * (size_t)i + 1] = N.y, Nprev[3 * (size_t)i + 2] = N.z;
    }
    return PRT_OK;
}

int prt_film_temporal(PrtContext* c, const PrtTemporal* cfg, const PrtDenoise* dn, float* rgb_out, float* var_out, float* history_out) {
    if (!c) return PRT_ERR_INVALID;
    const char* bad = prt_temporal_check(cfg, 1u, 1u, nullptr, rgb_out != nullptr);
    if (!bad && dn) bad = prt_denoise_check(dn, 1u, 1u, true);
    if (bad) return fail(c, PRT_ERR_INVALID, "%s", bad);
    if (!c->film_stats) return fail(c, PRT_ERR_INVALID, "prt_film_temporal: film statistics are off (prt_set_film_statistics)");
    if (c->has_film && c->tm.world != 1u)
        return fail(c, PRT_ERR_INVALID,
                    "prt_film_temporal: this context owns rank %u of %u of the image; a group form of the temporal step does not exist yet",
                    c->tm.rank, c->tm.world);
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->film.stat.p) return fail(c, PRT_ERR_INVALID, "prt_film_temporal: film statistics are off (prt_set_film_statistics)");
    const PrtTileMap& tm = c->tm;
    if ((bad = prt_temporal_check(cfg, tm.W, tm.H, nullptr, true))) return fail(c, PRT_ERR_INVALID, "%s", bad);
    if (!c->feat_valid && (rc = prt_render_features(c))) return rc;
    const PrtTemporal k = cfg ? *cfg : prt_temporal_default_config();
    const size_t n = (size_t)tm.W * tm.H;
    // two history sets, the blended planar frame (mean, var, N' / m1' / m2'), the counters, the status: a layout of W x H
    // alone, so that a step finds the sets where the step before it at this size left them
    PrtHistoryBufs set[2];
    float *d_mean, *d_var, *d_hist, *d_m1, *d_m2;
    uint32_t* d_counts;
    uint8_t* d_status;
    PrtWorkspace ws;
    declare_history(ws, &set[0], n);
    declare_history(ws, &set[1], n);
    ws.add(&d_mean, 3 * n).add(&d_var, n).add(&d_hist, n).add(&d_m1, n).add(&d_m2, n).add(&d_counts, 4).add(&d_status, n);
    if (ws.bytes() > c->tp.bytes) c->tp_valid = false;  // (a grown buffer holds no history; prt_set_film dropped it anyway)
    if ((rc = commit(c, ws, c->tp))) return rc;
    if (c->tp_valid && (c->tp_W != tm.W || c->tp_H != tm.H)) c->tp_valid = false;
    // (a camera whose width / height is not the film's: its basis projects into another image, so the history does not apply)
    if (c->tp_valid && !(c->tp_K.W == (float)tm.W && c->tp_K.H == (float)tm.H)) c->tp_valid = false;
    const PrtHistoryBufs prev = c->tp_valid ? set[c->tp_set] : PrtHistoryBufs{nullptr, nullptr, nullptr, nullptr};
    const int next_set = c->tp_valid ? (c->tp_set ^ 1) : 0;
    const PrtHistoryBufs next = set[next_set];
    // the placed copies now against their matrices at the previous step
    const PrtHostScene& hs = c->hs;
    const uint32_t n_copies = (uint32_t)hs.dev_insts.size() - hs.n_world_insts;
    PrtMotionTable mt{nullptr, nullptr, 0u};
    if (c->tp_valid && n_copies && c->tp_mats.size() == 12 * (size_t)n_copies) {
        std::vector<uint32_t>& h = c->tp_mt_host;  // {prim_base, n_tris} x n_copies (padded to 16 bytes), then 24 floats per copy
        const size_t r_words = (2 * (size_t)n_copies + 3) & ~(size_t)3;
        h.assign(r_words + 24 * (size_t)n_copies, 0u);
        for (uint32_t i = 0; i < n_copies; ++i) {
            const DevInstance& I = hs.dev_insts[hs.n_world_insts + i];
            h[2 * (size_t)i] = I.prim_base;
            h[2 * (size_t)i + 1] = I.n_tris;
            memcpy(&h[r_words + 24 * (size_t)i], I.inv, 48);
            memcpy(&h[r_words + 24 * (size_t)i + 12], &c->tp_mats[12 * (size_t)i], 48);
        }
        if ((rc = ensure(c, c->tp_mt, h.size() * sizeof(uint32_t)))) return rc;
        uint32_t* d_mt = (uint32_t*)c->tp_mt.p;
        if ((rc = upload(c, d_mt, h.data(), h.size()))) return rc;
        mt = PrtMotionTable{d_mt, (const float4*)(d_mt + r_words), n_copies};
    }
    HIPCHECK(c, hipMemsetAsync(d_counts, 0, 16, c->stream));
    const PrtFeatureBufs first = current_set(c, c->feat);
    prt_launch_tp_reproject_film(c->stream, tm, k, c->tp_K, c->film.local.as<float4>(), c->film.stat.as<float2>(), first.nrm, first.pos, mt, prev, next, d_mean, d_var,
                                 d_status, d_counts);
    HIPCHECK(c, hipGetLastError());
    if (history_out) prt_launch_tp_unpack(c->stream, (uint32_t)n, next, d_hist, d_m1, d_m2);
    const float *d_rgb = d_mean, *d_v = d_var;
    if (dn) {
        FilterScratch s;
        if ((rc = s.commit_film(c, n))) return rc;
        const PrtFeatureBufs gf = filter_features(c);
        prt_launch_dn_prepare(c->stream, (uint32_t)n, d_mean, d_var, gf, dn->demodulate, s.cv0);
        if ((rc = enqueue_filter(c, *dn, tm.W, tm.H, gf, s.cv0, s.cv1, s.out, s.var))) return rc;
        d_rgb = s.out;
        d_v = s.var;
    }
    uint32_t counts[4] = {0u, 0u, 0u, 0u};
    if ((rc = download(c, rgb_out, d_rgb, 3 * n))) return rc;
    if (var_out && (rc = download(c, var_out, d_v, n))) return rc;
    if (history_out && (rc = download(c, history_out, d_hist, n))) return rc;
    if ((rc = download(c, counts, d_counts, 4))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    // the new history: the set just written, the basis and the copies' matrices of this frame
    c->tp_set = next_set;
    c->tp_W = tm.W;
    c->tp_H = tm.H;
    (void)prt_get_camera_basis(c, &c->tp_K);
    c->tp_mats.resize(12 * (size_t)n_copies);
    for (uint32_t i = 0; i < n_copies; ++i) memcpy(&c->tp_mats[12 * (size_t)i], hs.dev_insts[hs.n_world_insts + i].mat, 48);
    c->tp_valid = true;
    ++c->tp_info.steps;
    c->tp_info.hit_pixels = counts[0];
    c->tp_info.reprojected = counts[1];
    return PRT_OK;
}

int prt_scatter(PrtContext* c, uint32_t n, const float* in_dirs, const PrtHit* hits, uint32_t* rng_state,
                uint32_t* scattered, float* attenuation, float* emitted, float* out_origins, float* out_dirs) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (n == 0) return PRT_OK;
    if (!in_dirs || !hits || !rng_state || !scattered || !attenuation || !emitted || !out_origins || !out_dirs)
        return fail(c, PRT_ERR_INVALID, "null array");
    for (uint32_t i = 0; i < n; ++i)
        if (hits[i].material_id >= c->hs.materials.size()) return fail(c, PRT_ERR_INVALID, "hit %u: material out of range", i);
    const size_t n1 = n;
    PrtHit* d_h;
    float *d_in, *d_at, *d_em, *d_oo, *d_od;
    uint32_t *d_rng, *d_sc;
    PrtWorkspace ws;
    ws.add(&d_h, n1).add(&d_in, 3 * n1).add(&d_rng, n1).add(&d_sc, n1).add(&d_at, 3 * n1).add(&d_em, 3 * n1).add(&d_oo, 3 * n1).add(&d_od, 3 * n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_h, hits, n1)) || (rc = upload(c, d_in, in_dirs, 3 * n1)) || (rc = upload(c, d_rng, rng_state, n1))) return rc;
    prt_launch_scatter_test(c->stream, c->dsc, n, d_in, d_h, d_rng, d_sc, d_at, d_em, d_oo, d_od);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, rng_state, d_rng, n1)) || (rc = download(c, scattered, d_sc, n1))) return rc;
    if ((rc = download(c, attenuation, d_at, 3 * n1)) || (rc = download(c, emitted, d_em, 3 * n1))) return rc;
    if ((rc = download(c, out_origins, d_oo, 3 * n1)) || (rc = download(c, out_dirs, d_od, 3 * n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// ---- radiance query (include/prt.h "Radiance query") --------------------------------------------------
// What enqueue_radiance needs beside its arguments for chunks of up to m paths: two lists (a ray and two float4 of state
// each), the hit records and the textured albedo of a round's live rays, one record per slot, and the two live counts that
// take turns.  A caller declares it behind its own arrays, in the same layout.
struct RadianceScratch {
    PrtRadianceList list[2];
    PrtHit* hits;
    float* albedo;
    float4* slots;
    uint32_t* cnt;
    void declare(PrtWorkspace& ws, size_t m, bool textured) {
        for (PrtRadianceList& l : list) ws.add(&l.o, 3 * m).add(&l.d, 3 * m).add(&l.s0, m).add(&l.s1, m);
        ws.add(&hits, m).add(&slots, m).add(&cnt, (size_t)2);
        albedo = nullptr;
        if (textured) ws.add(&albedo, 3 * m);
    }
};

// Samples per chunk: about 2^22 rays unless a chunk size is forced, at least one sample (enqueue_feature_samples' rule)
static uint32_t radiance_chunk(const PrtContext* c, const PrtRadianceQuery& q, uint32_t n) {
    const uint32_t cs = c->radiance_chunk > 0 ? (uint32_t)c->radiance_chunk : std::max<uint32_t>(1u, (1u << 22) / n);
    return std::min(cs, q.samples);
}

// The refusals of both forms, in the order of the header; everything here is decided without a device.
static int check_radiance(PrtContext* c, const PrtRadianceQuery* q, uint32_t n, const void* origins, const void* dirs, const void* rng_state,
                          const void* rgb_sum) {
    if (!c) return PRT_ERR_INVALID;
    if (!q) return fail(c, PRT_ERR_INVALID, "prt_radiance: null query");
    if (q->samples == 0u || q->samples > PRT_RADIANCE_MAX_SAMPLES)
        return fail(c, PRT_ERR_INVALID, "prt_radiance: samples = %u, expected 1 .. %u", q->samples, PRT_RADIANCE_MAX_SAMPLES);
    if (rng_state && q->samples > 1u)
        return fail(c, PRT_ERR_INVALID, "prt_radiance: rng_state carries one state per ray: samples must be 1, not %u", q->samples);
    if ((uint64_t)n * q->samples > 0xFFFFFFFFull)
        return fail(c, PRT_ERR_INVALID, "prt_radiance: %u rays x %u samples exceed 2^32 - 1 paths", n, q->samples);
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (n != 0u && (!origins || !dirs || !rgb_sum)) return fail(c, PRT_ERR_INVALID, "prt_radiance: null array");
    return PRT_OK;
}

// The paths of n rays (device arrays) on the context's stream.  Chunks of cs whole samples; per chunk the start kernel
// leaves every path live in list 0, and each round reads the 4-byte live count (one small wait, as enqueue_chains has),
// queries the live rays only, looks up the textured albedo of their hits, and steps them into the other list.  Round
// max_depth - 1 ends every path, so after the rounds every slot is written and the ordered sum adds the chunk to the
// outputs.  Nothing but x, the outputs, d_rng and the ray-query pipeline's own buffers is written.
static int enqueue_radiance(PrtContext* c, const PrtRadianceQuery& q, uint32_t n, uint32_t cs, const float* d_o, const float* d_d,
                            uint32_t* d_rng, float* d_rgb, uint32_t* d_seg, const RadianceScratch& x) {
    int rc;
    if (q.max_depth == 0u) {
        HIPCHECK(c, hipMemsetAsync(d_rgb, 0, 3 * (size_t)n * sizeof(float), c->stream));
        if (d_seg) HIPCHECK(c, hipMemsetAsync(d_seg, 0, (size_t)n * sizeof(uint32_t), c->stream));
        return PRT_OK;
    }
    PrtRadianceArgs a{x.hits, x.albedo, c->dsc.mat_rgbs, c->dsc.mat_type, env_on(c) ? dev_env(c) : DevEnv{}, {c->dsc.sky[0], c->dsc.sky[1], c->dsc.sky[2]},
                      c->sampling, q.max_depth, 0u, x.slots, d_rng, nullptr};
    for (uint32_t s0 = 0; s0 < q.samples; s0 += cs) {
        const uint32_t ccs = std::min(cs, q.samples - s0);
        const uint32_t m = ccs * n;
        prt_launch_rd_start(c->stream, n, ccs, q.first_sample + s0, q.seed, d_o, d_d, d_rng, x.list[0]);
        HIPCHECK(c, hipGetLastError());
        uint32_t live = m;
        int cur = 0;
        for (uint32_t r = 0; r < q.max_depth; ++r) {
            if (r > 0u) {
                HIPCHECK(c, hipMemcpyAsync(&live, x.cnt + (r & 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                HIPCHECK(c, hipStreamSynchronize(c->stream));
                if (live == 0u) break;
                if (live > m) return fail(c, PRT_ERR_HIP, "prt_radiance: live count %u above %u paths", live, m);
            }
            if ((rc = enqueue_query(c, live, x.list[cur].o, x.list[cur].d, nullptr, x.hits, nullptr))) return rc;
            if (x.albedo) prt_launch_hit_uv(c->stream, c->dsc, dev_tex(c), live, c->rb[0], nullptr, x.albedo);  // (rays and final hit ids are in rb[0])
            a.round = r;
            a.count = x.cnt + ((r + 1u) & 1u);
            HIPCHECK(c, hipMemsetAsync(a.count, 0, sizeof(uint32_t), c->stream));
            prt_launch_rd_step(c->stream, live, x.list[cur], a, x.list[cur ^ 1]);
            HIPCHECK(c, hipGetLastError());
            cur ^= 1;
        }
        prt_launch_rd_sum(c->stream, n, ccs, s0 == 0u, x.slots, d_rgb, d_seg);
        HIPCHECK(c, hipGetLastError());
    }
    return PRT_OK;
}

int prt_radiance(PrtContext* c, const PrtRadianceQuery* q, uint32_t n, const float* origins, const float* dirs, uint32_t* rng_state,
                 float* rgb_sum, uint32_t* segments) {
    int rc = check_radiance(c, q, n, origins, dirs, rng_state, rgb_sum);
    if (rc || n == 0u) return rc;
    if ((rc = need_device(c))) return rc;
    const uint32_t cs = radiance_chunk(c, *q, n);
    const size_t n1 = n;
    // the scratch below and the path state of a chunk's rays may be reallocated: nothing enqueued before may still be using them
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    float *d_o, *d_d, *d_rgb;
    uint32_t *d_rng = nullptr, *d_seg = nullptr;
    RadianceScratch x;
    PrtWorkspace ws;
    ws.add(&d_o, 3 * n1).add(&d_d, 3 * n1).add(&d_rgb, 3 * n1);
    if (rng_state) ws.add(&d_rng, n1);
    if (segments) ws.add(&d_seg, n1);
    x.declare(ws, (size_t)cs * n1, tex_on(c));
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_o, origins, 3 * n1)) || (rc = upload(c, d_d, dirs, 3 * n1))) return rc;
    if (rng_state && (rc = upload(c, d_rng, rng_state, n1))) return rc;
    if ((rc = enqueue_radiance(c, *q, n, cs, d_o, d_d, d_rng, d_rgb, d_seg, x))) return rc;
    if ((rc = download(c, rgb_sum, d_rgb, 3 * n1))) return rc;
    if (rng_state && (rc = download(c, rng_state, d_rng, n1))) return rc;
    if (segments && (rc = download(c, segments, d_seg, n1))) return rc;
    return prt_synchronize(c);  // waits for the stream and reports a ray the walk had to give up
}

int prt_radiance_device(PrtContext* c, const PrtRadianceQuery* q, uint32_t n, const void* d_origins, const void* d_dirs, void* d_rng_state,
                        void* d_rgb_sum, void* d_segments) {
    int rc = check_radiance(c, q, n, d_origins, d_dirs, d_rng_state, d_rgb_sum);
    if (rc || n == 0u) return rc;
    if ((rc = need_device(c))) return rc;
    const uint32_t cs = radiance_chunk(c, *q, n);
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (as above)
    RadianceScratch x;
    PrtWorkspace ws;
    x.declare(ws, (size_t)cs * n, tex_on(c));
    if ((rc = commit(c, ws, c->scratch))) return rc;
    return enqueue_radiance(c, *q, n, cs, (const float*)d_origins, (const float*)d_dirs, (uint32_t*)d_rng_state, (float*)d_rgb_sum,
                            (uint32_t*)d_segments, x);
}

// ---- light-sampled radiance query (include/prt.h "Radiance query", prt_radiance_lit) -----------------------
// RadianceScratch's layout for the lit paths: the lists carry pb, and a chunk of up to m paths has its shadow list, the
// occlusion bytes, one light sum per slot, the live / shadow count pairs that take turns, and the query's counters.
struct RadianceLitScratch {
    PrtRadianceLitList list[2];
    PrtRadianceShadowList sh;
    PrtHit* hits;
    float* albedo;
    float4* slots;
    float4* lsum;
    uint8_t* occ;
    uint32_t* cnt;                // [2][2]: {live, shadow rays} written by the rounds of either parity
    unsigned long long* stats;    // [PRT_RDL_STAT_SLOTS][2]
    void declare(PrtWorkspace& ws, size_t m, bool textured) {
        for (PrtRadianceLitList& l : list) ws.add(&l.l.o, 3 * m).add(&l.l.d, 3 * m).add(&l.l.s0, m).add(&l.l.s1, m).add(&l.pb, m);
        ws.add(&sh.x, 3 * m).add(&sh.w, 3 * m).add(&sh.tmax, m).add(&sh.cs, m);
        ws.add(&hits, m).add(&slots, m).add(&lsum, m).add(&occ, m).add(&cnt, (size_t)4).add(&stats, (size_t)2 * PRT_RDL_STAT_SLOTS);
        albedo = nullptr;
        if (textured) ws.add(&albedo, 3 * m);
    }
};

// enqueue_radiance with light sampling (the context's lighting mode is not OFF).  The shadow rays a round's step appended
// are resolved at the top of the next round, after the one wait that reads the live count and the shadow count in one
// 8-byte copy, and before that round's closest-hit query: both pipelines pack into rb[0], one after the other.  The last
// round (segment max_depth - 1) takes no light sample, and a chunk whose paths all end earlier resolves before it
// leaves the loop: so there is no wait beyond the unlit query's one per round.  info (host, may be null): one more read.
// d_pb (may be null): the pdf of the caller's own Lambertian scatter along each ray (prt_radiance_lit_pb).
static int enqueue_radiance_lit(PrtContext* c, const PrtRadianceQuery& q, uint32_t n, uint32_t cs, const float* d_o, const float* d_d,
                                uint32_t* d_rng, const float* d_pb, float* d_rgb, uint32_t* d_seg, const RadianceLitScratch& x,
                                PrtRadianceLitInfo* info) {
    int rc;
    if (info) *info = PrtRadianceLitInfo{0u, 0u};
    if (q.max_depth == 0u) {
        HIPCHECK(c, hipMemsetAsync(d_rgb, 0, 3 * (size_t)n * sizeof(float), c->stream));
        if (d_seg) HIPCHECK(c, hipMemsetAsync(d_seg, 0, (size_t)n * sizeof(uint32_t), c->stream));
        return PRT_OK;
    }
    if ((rc = sync_light_tables(c))) return rc;
    const bool mesh = mesh_lights_on(c), env = env_on(c), clus = clusters_on(c);
    PrtRadianceLitArgs a{{x.hits, x.albedo, c->dsc.mat_rgbs, c->dsc.mat_type, env ? dev_env(c) : DevEnv{}, {c->dsc.sky[0], c->dsc.sky[1], c->dsc.sky[2]},
                          c->sampling, q.max_depth, 0u, x.slots, d_rng, nullptr},
                         dev_lights(c), dev_mesh_lights(c), dev_light_clusters(c), c->dsc.n_prims, x.sh, nullptr};
    HIPCHECK(c, hipMemsetAsync(x.stats, 0, 2 * PRT_RDL_STAT_SLOTS * sizeof(unsigned long long), c->stream));
    for (uint32_t s0 = 0; s0 < q.samples; s0 += cs) {
        const uint32_t ccs = std::min(cs, q.samples - s0);
        const uint32_t m = ccs * n;
        prt_launch_rdl_start(c->stream, n, ccs, q.first_sample + s0, q.seed, d_o, d_d, d_rng, d_pb, x.list[0]);
        HIPCHECK(c, hipGetLastError());
        HIPCHECK(c, hipMemsetAsync(x.lsum, 0, (size_t)m * sizeof(float4), c->stream));
        uint32_t live = m;
        int cur = 0;
        for (uint32_t r = 0; r < q.max_depth; ++r) {
            if (r > 0u) {
                uint32_t two[2] = {0u, 0u};
                HIPCHECK(c, hipMemcpyAsync(two, x.cnt + 2u * (r & 1u), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                HIPCHECK(c, hipStreamSynchronize(c->stream));
                live = two[0];
                const uint32_t n_sh = two[1];
                if (live > m || n_sh > m) return fail(c, PRT_ERR_HIP, "prt_radiance_lit: live count %u or shadow count %u above %u paths", live, n_sh, m);
                if (n_sh != 0u) {  // the shadow rays of round r - 1: prt_occluded's pipeline, then their contributions
                    if ((rc = enqueue_query(c, n_sh, x.sh.x, x.sh.w, x.sh.tmax, nullptr, x.occ))) return rc;
                    prt_launch_rdl_light(c->stream, n_sh, x.sh, x.occ, x.lsum, x.stats);
                    HIPCHECK(c, hipGetLastError());
                }
                if (live == 0u) break;
            }
            if ((rc = enqueue_query(c, live, x.list[cur].l.o, x.list[cur].l.d, nullptr, x.hits, nullptr))) return rc;
            if (x.albedo) prt_launch_hit_uv(c->stream, c->dsc, dev_tex(c), live, c->rb[0], nullptr, x.albedo);  // (rays and final hit ids are in rb[0])
            uint32_t* next = x.cnt + 2u * ((r + 1u) & 1u);
            a.a.round = r;
            a.a.count = next;
            a.scount = next + 1;
            HIPCHECK(c, hipMemsetAsync(next, 0, 2 * sizeof(uint32_t), c->stream));
            prt_launch_rdl_step(c->stream, mesh, env, clus, live, x.list[cur], a, x.list[cur ^ 1]);
            HIPCHECK(c, hipGetLastError());
            cur ^= 1;
        }
        prt_launch_rdl_sum(c->stream, n, ccs, s0 == 0u, x.slots, x.lsum, d_rgb, d_seg);
        HIPCHECK(c, hipGetLastError());
    }
    if (info) {
        unsigned long long st[2 * PRT_RDL_STAT_SLOTS];
        HIPCHECK(c, hipMemcpyAsync(st, x.stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < PRT_RDL_STAT_SLOTS; ++k) {
            info->shadow_rays += st[2 * k];
            info->shadow_occluded += st[2 * k + 1];
        }
    }
    return PRT_OK;
}

int prt_radiance_lit_pb(PrtContext* c, const PrtRadianceQuery* q, uint32_t n, const float* origins, const float* dirs, uint32_t* rng_state,
                        const float* pb, float* rgb_sum, uint32_t* segments, PrtRadianceLitInfo* info) {
    int rc = check_radiance(c, q, n, origins, dirs, rng_state, rgb_sum);
    if (info) *info = PrtRadianceLitInfo{0u, 0u};
    if (rc || n == 0u) return rc;
    if ((rc = need_device(c))) return rc;
    if (c->lighting == (uint32_t)PRT_LIGHTING_OFF) return prt_radiance(c, q, n, origins, dirs, rng_state, rgb_sum, segments);
    const uint32_t cs = radiance_chunk(c, *q, n);
    const size_t n1 = n;
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (as prt_radiance: the scratch may be reallocated)
    float *d_o, *d_d, *d_rgb, *d_pb = nullptr;
    uint32_t *d_rng = nullptr, *d_seg = nullptr;
    RadianceLitScratch x;
    PrtWorkspace ws;
    ws.add(&d_o, 3 * n1).add(&d_d, 3 * n1).add(&d_rgb, 3 * n1);
    if (rng_state) ws.add(&d_rng, n1);
    if (segments) ws.add(&d_seg, n1);
    if (pb) ws.add(&d_pb, n1);
    x.declare(ws, (size_t)cs * n1, tex_on(c));
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_o, origins, 3 * n1)) || (rc = upload(c, d_d, dirs, 3 * n1))) return rc;
    if (rng_state && (rc = upload(c, d_rng, rng_state, n1))) return rc;
    if (pb && (rc = upload(c, d_pb, pb, n1))) return rc;
    if ((rc = enqueue_radiance_lit(c, *q, n, cs, d_o, d_d, d_rng, d_pb, d_rgb, d_seg, x, info))) return rc;
    if ((rc = download(c, rgb_sum, d_rgb, 3 * n1))) return rc;
    if (rng_state && (rc = download(c, rng_state, d_rng, n1))) return rc;
    if (segments && (rc = download(c, segments, d_seg, n1))) return rc;
    return prt_synchronize(c);  // waits for the stream and reports a ray a walk (closest hit or shadow) had to give up
}

int prt_radiance_lit(PrtContext* c, const PrtRadianceQuery* q, uint32_t n, const float* origins, const float* dirs, uint32_t* rng_state,
                     float* rgb_sum, uint32_t* segments, PrtRadianceLitInfo* info) {
    return prt_radiance_lit_pb(c, q, n, origins, dirs, rng_state, nullptr, rgb_sum, segments, info);
}

int prt_radiance_lit_pb_device(PrtContext* c, const PrtRadianceQuery* q, uint32_t n, const void* d_origins, const void* d_dirs, void* d_rng_state,
                               const void* d_pb, void* d_rgb_sum, void* d_segments, PrtRadianceLitInfo* info) {
    int rc = check_radiance(c, q, n, d_origins, d_dirs, d_rng_state, d_rgb_sum);
    if (info) *info = PrtRadianceLitInfo{0u, 0u};
    if (rc || n == 0u) return rc;
    if ((rc = need_device(c))) return rc;
    if (c->lighting == (uint32_t)PRT_LIGHTING_OFF) return prt_radiance_device(c, q, n, d_origins, d_dirs, d_rng_state, d_rgb_sum, d_segments);
    const uint32_t cs = radiance_chunk(c, *q, n);
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (as above)
    RadianceLitScratch x;
    PrtWorkspace ws;
    x.declare(ws, (size_t)cs * n, tex_on(c));
    if ((rc = commit(c, ws, c->scratch))) return rc;
    return enqueue_radiance_lit(c, *q, n, cs, (const float*)d_origins, (const float*)d_dirs, (uint32_t*)d_rng_state, (const float*)d_pb,
                                (float*)d_rgb_sum, (uint32_t*)d_segments, x, info);
}

int prt_radiance_lit_device(PrtContext* c, const PrtRadianceQuery* q, uint32_t n, const void* d_origins, const void* d_dirs, void* d_rng_state,
                            void* d_rgb_sum, void* d_segments, PrtRadianceLitInfo* info) {
    return prt_radiance_lit_pb_device(c, q, n, d_origins, d_dirs, d_rng_state, nullptr, d_rgb_sum, d_segments, info);
}

// ---- surface baking (include/prt.h "Surface baking") -------------------------------------------------------
// What the refusals leave behind: the map's size, which records hold the target's faces, and the faces' UVs in face order.
struct BakeTarget {
    uint32_t W = 0, H = 0, n_faces = 0;
    bool placed = false;
    uint32_t inst = 0;        // a placed copy: its entry of hs.dev_insts
    uint32_t mesh = 0;        // a placed copy: its instanced mesh
    uint32_t face_first = 0;  // a world-space mesh: its first triangle in mesh and face order
    std::vector<float> uv6, pos9, nrm9;
};

// The bake's own arrays in c->bake.
struct BakeBufs {
    PrtBakeFaces faces{};
    PrtBakeMap map{};
    uint32_t* list = nullptr;
    uint32_t* counts = nullptr;
    float* rgb[2] = {nullptr, nullptr};
    uint8_t* cov2 = nullptr;
};

// What an adaptive bake keeps beside them for the length of a call, in c->bake too (c->scratch is laid out anew by every
// pass): the count and the moments, the second buffer of the mean's gutter fill, the `active` bytes, the texel list of a
// pass, the flags and the two block lists that ping-pong, and the selection's counters.
struct BakeAdaptiveBufs {
    float *count = nullptr, *sum_y = nullptr, *sum_y2 = nullptr, *mean2 = nullptr;
    uint8_t* active = nullptr;
    uint32_t *tlist = nullptr, *flags = nullptr, *blist[2] = {nullptr, nullptr}, *sel = nullptr;
};

// The refusals, in the order of the header; everything here is decided without a device.  q: null for the entry points
// that trace nothing.
static int check_bake(PrtContext* c, const PrtBakeTarget* t, const PrtRadianceQuery* q, bool with_query, BakeTarget* b) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (!t) return fail(c, PRT_ERR_INVALID, "prt_bake: null target");
    const PrtHostScene& hs = c->hs;
    const uint32_t n_meshes = (uint32_t)(hs.mesh_sizes.size() / 2);
    const uint32_t* indices = nullptr;
    uint32_t n_vertices = 0;
    size_t has_uv_entry = 0;
    if (t->kind == PRT_BAKE_MESH) {
        if (t->index >= n_meshes) return fail(c, PRT_ERR_INVALID, "prt_bake: mesh %u of %u", t->index, n_meshes);
        for (uint32_t m = 0; m < t->index; ++m) b->face_first += hs.mesh_sizes[2 * m + 1];
        b->n_faces = hs.mesh_sizes[2 * t->index + 1];
        n_vertices = hs.mesh_sizes[2 * t->index];
        if (hs.mesh_indices.size() < 3 * ((size_t)b->face_first + b->n_faces)) return fail(c, PRT_ERR_INVALID, "prt_bake: the scene keeps no index buffer of mesh %u", t->index);
        indices = hs.mesh_indices.data() + 3 * (size_t)b->face_first;
        has_uv_entry = t->index;
    } else if (t->kind == PRT_BAKE_INSTANCE) {
        if (t->index >= hs.inst_mesh.size()) return fail(c, PRT_ERR_INVALID, "prt_bake: placed copy %u of %zu", t->index, hs.inst_mesh.size());
        b->placed = true;
        b->inst = hs.n_world_insts + t->index;
        b->mesh = hs.inst_mesh[t->index];
        if (b->mesh >= hs.placed_indices.size() || b->mesh >= hs.placed_meshes.size()) return fail(c, PRT_ERR_INVALID, "prt_bake: the scene keeps no index buffer of instanced mesh %u", b->mesh);
        b->n_faces = (uint32_t)(hs.placed_indices[b->mesh].size() / 3);
        n_vertices = hs.placed_vertices[b->mesh];
        indices = hs.placed_indices[b->mesh].data();
        has_uv_entry = (size_t)n_meshes + b->mesh;
    } else {
        return fail(c, PRT_ERR_INVALID, "prt_bake: unknown target kind %u", t->kind);
    }
    if (b->n_faces == 0u) return fail(c, PRT_ERR_INVALID, "prt_bake: the target has no faces");
    if (t->width == 0u || t->height == 0u || t->width > PRT_TEX_MAX_SIZE || t->height > PRT_TEX_MAX_SIZE)
        return fail(c, PRT_ERR_INVALID, "prt_bake: a %u x %u map, expected 1 .. %u each way", t->width, t->height, PRT_TEX_MAX_SIZE);
    b->W = t->width;
    b->H = t->height;
    b->uv6.resize(6 * (size_t)b->n_faces);
    if (t->uvs) {
        for (size_t k = 0; k < 3 * (size_t)b->n_faces; ++k) {
            if (indices[k] >= n_vertices) return fail(c, PRT_ERR_INVALID, "prt_bake: vertex index out of range");
            b->uv6[2 * k] = t->uvs[2 * (size_t)indices[k]];
            b->uv6[2 * k + 1] = t->uvs[2 * (size_t)indices[k] + 1];
        }
    } else {
        const PrtTexTables& tx = c->tex;
        if (!tx.is_set || has_uv_entry >= tx.mesh_has_uv.size() || !tx.mesh_has_uv[has_uv_entry])
            return fail(c, PRT_ERR_INVALID, "prt_bake: no UVs: none given and the texture binding has none for this mesh");
        const size_t first = b->placed ? (size_t)tx.inst_uv_base[b->inst] : (size_t)b->face_first;
        if (tx.uvs.size() < 6 * (first + b->n_faces)) return fail(c, PRT_ERR_INVALID, "prt_bake: the texture binding's UV table is short");
        memcpy(b->uv6.data(), tx.uvs.data() + 6 * first, 24 * (size_t)b->n_faces);
    }
    for (float v : b->uv6)
        if (!(std::fabs(v) <= 1048576.0f)) return fail(c, PRT_ERR_INVALID, "prt_bake: a UV is not finite or above 2^20");
    if (with_query) {
        if (!q) return fail(c, PRT_ERR_INVALID, "prt_bake: null query");
        if (q->samples == 0u || q->samples > PRT_RADIANCE_MAX_SAMPLES)
            return fail(c, PRT_ERR_INVALID, "prt_bake: samples = %u, expected 1 .. %u", q->samples, PRT_RADIANCE_MAX_SAMPLES);
        if ((uint64_t)b->W * b->H * q->samples > 0xFFFFFFFFull)
            return fail(c, PRT_ERR_INVALID, "prt_bake: %u x %u texels x %u samples exceed 2^32 - 1 paths", b->W, b->H, q->samples);
    }
    return PRT_OK;
}

// The target's faces out of the triangle and normal records (leaf order, current after either refit) into face order
static int bake_geometry(PrtContext* c, BakeTarget* b) {
    if (const int rc = refresh_host_copies(c)) return rc;
    const PrtHostScene& hs = c->hs;
    size_t slot0 = 0, n_slots = hs.mesh_indices.size() / 3;
    uint32_t base = hs.sc.n_prims + b->face_first;  // what face 0's record carries
    if (b->placed) {
        slot0 = hs.placed_meshes[b->mesh].slot_base;
        n_slots = hs.placed_meshes[b->mesh].n_tris;
        base = 0u;
    }
    if (hs.tri_records.size() < 12 * (slot0 + n_slots) || hs.nrm_records.size() < 12 * (slot0 + n_slots))
        return fail(c, PRT_ERR_INVALID, "prt_bake: the scene keeps no triangle records of the target");
    b->pos9.assign(9 * (size_t)b->n_faces, 0.0f);
    b->nrm9.assign(9 * (size_t)b->n_faces, 0.0f);
    size_t found = 0;
    for (size_t sl = slot0; sl < slot0 + n_slots; ++sl) {
        const float* r = &hs.tri_records[12 * sl];
        const float* nr = &hs.nrm_records[12 * sl];
        uint32_t prim;
        memcpy(&prim, &r[3], 4);
        const uint32_t f = prim - base;
        if (f >= b->n_faces) continue;
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) {
                b->pos9[9 * (size_t)f + 3 * v + a] = r[4 * v + a];
                b->nrm9[9 * (size_t)f + 3 * v + a] = nr[4 * v + a];
            }
        ++found;
    }
    if (found != b->n_faces) return fail(c, PRT_ERR_INVALID, "prt_bake: %zu of the target's %u faces are in the scene's records", found, b->n_faces);
    return PRT_OK;
}

// Coverage, surface and the texel list of a checked target on the context's stream; counts (host) as of the list.  The
// arrays are in c->bake; with_rgb: the two value buffers and the second coverage buffer of the gutter fill too.
static int enqueue_bake_surface(PrtContext* c, BakeTarget* b, bool with_rgb, BakeBufs* x, uint32_t* counts, BakeAdaptiveBufs* ax = nullptr) {
    int rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (c->bake may be reallocated: nothing enqueued before may still be using it)
    if ((rc = bake_geometry(c, b))) return rc;
    const size_t F = b->n_faces, n = (size_t)b->W * b->H;
    float *d_uv, *d_pos, *d_nrm;
    PrtWorkspace ws;
    ws.add(&d_uv, 6 * F).add(&d_pos, 9 * F).add(&d_nrm, 9 * F);
    ws.add(&x->map.owner, n).add(&x->map.cov, n).add(&x->map.bary, 2 * n).add(&x->map.position, 3 * n).add(&x->map.normal, 3 * n);
    ws.add(&x->list, n).add(&x->counts, (size_t)PRT_BAKE_COUNTERS);
    if (with_rgb) ws.add(&x->rgb[0], 3 * n).add(&x->rgb[1], 3 * n).add(&x->cov2, n);
    if (ax) {  // (behind the bake's own arrays, which lie where they lie without these)
        const size_t nb = prt_bake_block_count(b->W, b->H);
        ws.add(&ax->count, n).add(&ax->sum_y, n).add(&ax->sum_y2, n).add(&ax->mean2, 3 * n).add(&ax->active, n).add(&ax->tlist, n);
        ws.add(&ax->flags, nb).add(&ax->blist[0], nb).add(&ax->blist[1], nb).add(&ax->sel, (size_t)PRT_BKA_COUNTERS);
    }
    if ((rc = commit(c, ws, c->bake))) return rc;
    if ((rc = upload(c, d_uv, b->uv6.data(), 6 * F)) || (rc = upload(c, d_pos, b->pos9.data(), 9 * F)) || (rc = upload(c, d_nrm, b->nrm9.data(), 9 * F)))
        return rc;
    x->map.W = b->W;
    x->map.H = b->H;
    x->faces.uv = d_uv;
    x->faces.pos = d_pos;
    x->faces.nrm = d_nrm;
    x->faces.n_faces = b->n_faces;
    x->faces.placed = b->placed ? 1u : 0u;
    if (b->placed) {
        memcpy(x->faces.mat, c->hs.dev_insts[b->inst].mat, 48);
        memcpy(x->faces.inv, c->hs.dev_insts[b->inst].inv, 48);
    }
    HIPCHECK(c, hipMemsetAsync(x->map.owner, 0xFF, n * sizeof(uint32_t), c->stream));
    HIPCHECK(c, hipMemsetAsync(x->counts, 0, PRT_BAKE_COUNTERS * sizeof(uint32_t), c->stream));
    prt_launch_bk_cover(c->stream, x->faces, x->map, x->counts);
    HIPCHECK(c, hipGetLastError());
    prt_launch_bk_surface(c->stream, x->faces, x->map, x->counts);
    HIPCHECK(c, hipGetLastError());
    prt_launch_bk_compact(c->stream, (uint32_t)n, x->map.cov, x->list, x->counts);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, counts, x->counts, (size_t)PRT_BAKE_COUNTERS))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (the host arrays of the uploads above are the caller's until here)
    if (counts[PRT_BAKE_CNT_COVERED] > n) return fail(c, PRT_ERR_HIP, "prt_bake: %u covered texels of %zu", counts[PRT_BAKE_CNT_COVERED], n);
    return PRT_OK;
}

static void bake_info_surface(PrtBakeInfo* info, const BakeTarget& b, const uint32_t* counts) {
    if (!info) return;
    *info = PrtBakeInfo{};
    info->n_texels = (uint64_t)b.W * b.H;
    info->n_covered = counts[PRT_BAKE_CNT_COVERED];
    info->n_degenerate = counts[PRT_BAKE_CNT_DEGENERATE];
    info->n_faces_skipped = counts[PRT_BAKE_CNT_SKIPPED];
}

int prt_bake_surface(PrtContext* c, const PrtBakeTarget* target, uint32_t* owner, float* bary, float* position, float* normal, PrtBakeInfo* info) {
    BakeTarget b;
    int rc = check_bake(c, target, nullptr, false, &b);
    if (rc) return rc;
    if ((rc = need_device(c))) return rc;
    BakeBufs x;
    uint32_t counts[PRT_BAKE_COUNTERS] = {};
    if ((rc = enqueue_bake_surface(c, &b, false, &x, counts))) return rc;
    const size_t n = (size_t)b.W * b.H;
    if (owner && (rc = download(c, owner, x.map.owner, n))) return rc;
    if (bary && (rc = download(c, bary, x.map.bary, 2 * n))) return rc;
    if (position && (rc = download(c, position, x.map.position, 3 * n))) return rc;
    if (normal && (rc = download(c, normal, x.map.normal, 3 * n))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    bake_info_surface(info, b, counts);
    return PRT_OK;
}

int prt_bake_rays(PrtContext* c, const PrtBakeTarget* target, uint32_t seed, uint32_t sample, float* origins, float* dirs, uint32_t* rng_state) {
    BakeTarget b;
    int rc = check_bake(c, target, nullptr, false, &b);
    if (rc) return rc;
    if (!origins || !dirs || !rng_state) return fail(c, PRT_ERR_INVALID, "prt_bake_rays: null array");
    if ((rc = need_device(c))) return rc;
    BakeBufs x;
    uint32_t counts[PRT_BAKE_COUNTERS] = {};
    if ((rc = enqueue_bake_surface(c, &b, false, &x, counts))) return rc;
    const size_t n = (size_t)b.W * b.H;
    float *d_o, *d_d;
    uint32_t* d_rng;
    PrtWorkspace ws;
    ws.add(&d_o, 3 * n).add(&d_d, 3 * n).add(&d_rng, n);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    prt_launch_bk_rays(c->stream, (uint32_t)n, 1u, sample, seed, nullptr, x.map, d_o, d_d, d_rng);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, origins, d_o, 3 * n)) || (rc = download(c, dirs, d_d, 3 * n)) || (rc = download(c, rng_state, d_rng, n))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// Where the ordered sum of a chunk goes: moments.count == null: k_bk_sum into rgb_sum alone; else k_bka_sum into all four maps.
struct BakeSums {
    PrtBakeMoments moments{};
    uint32_t* counts = nullptr;
};

// q.samples samples, indices q.first_sample .., of the n_list texels of d_list (ascending texel indices of the map) into
// `out`.  The rays of a chunk of whole samples go through the radiance query's own rounds (enqueue_radiance /
// enqueue_radiance_lit with the states given, one sample per ray), sample-major over the list, and the sum kernel adds a
// texel's values in ascending sample order: nothing depends on the chunk.
// With the texel's light sample (texel): per chunk k_bkl_sample takes the
// samples and the pdfs of the texels' rays, the lit query starts its paths from those pdfs, one pass of the occlusion
// pipeline resolves the texels' shadow rays (dense: a ray that is not cast has tmax = 0 and never occludes, so there is no
// count to wait for) and k_bkl_add adds what arrives to the query's values before the ordered sum.
// first: the maps of `out` hold nothing yet (the first chunk starts from 0.0f).  shadow += the shadow rays cast / occluded,
// where want_info.  The rays and the query's lists are in c->scratch.
static int enqueue_bake_samples(PrtContext* c, const PrtRadianceQuery& q, bool lit, bool texel, const uint32_t* d_list, uint32_t n_list,
                                const PrtBakeMap& map, bool first, const BakeSums& out, bool want_info, uint64_t shadow[2]) {
    int rc;
    const uint32_t cs = c->bake_chunk > 0 ? std::min((uint32_t)c->bake_chunk, q.samples) : radiance_chunk(c, q, n_list);
    const size_t m = (size_t)cs * n_list;
    float *d_o, *d_d, *d_rgb;
    uint32_t *d_rng, *d_seg;
    RadianceScratch xs;
    RadianceLitScratch xl;
    PrtBakeLightRays tl{};
    uint8_t* d_tocc = nullptr;
    unsigned long long* d_tstats = nullptr;
    PrtWorkspace ws;
    ws.add(&d_o, 3 * m).add(&d_d, 3 * m).add(&d_rng, m).add(&d_rgb, 3 * m).add(&d_seg, m);
    if (lit) xl.declare(ws, m, tex_on(c));
    else xs.declare(ws, m, tex_on(c));
    if (texel)
        ws.add(&tl.x, 3 * m).add(&tl.w, 3 * m).add(&tl.tmax, m).add(&tl.contrib, 3 * m).add(&tl.ray_pb, m).add(&d_tocc, m).add(
            &d_tstats, (size_t)2 * PRT_BKL_STAT_SLOTS);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    PrtBakeLightArgs la{};
    if (texel) {
        if ((rc = sync_light_tables(c))) return rc;
        la = PrtBakeLightArgs{dev_lights(c), dev_mesh_lights(c), dev_light_clusters(c), env_on(c) ? dev_env(c) : DevEnv{}, c->sampling.clamp};
        HIPCHECK(c, hipMemsetAsync(d_tstats, 0, 2 * PRT_BKL_STAT_SLOTS * sizeof(unsigned long long), c->stream));
    }
    const PrtRadianceQuery q1{q.max_depth, 1u, q.seed, q.first_sample};  // (one sample per ray: the states are given)
    for (uint32_t s0 = 0; s0 < q.samples; s0 += cs) {
        const uint32_t ccs = std::min(cs, q.samples - s0);
        const uint32_t mm = ccs * n_list;
        prt_launch_bk_rays(c->stream, n_list, ccs, q.first_sample + s0, q.seed, d_list, map, d_o, d_d, d_rng);
        HIPCHECK(c, hipGetLastError());
        if (texel) {
            prt_launch_bkl_sample(c->stream, mesh_lights_on(c), env_on(c), clusters_on(c), n_list, ccs, q.first_sample + s0, q.seed, d_list, map,
                                  d_d, la, tl);
            HIPCHECK(c, hipGetLastError());
        }
        if (lit) {
            PrtRadianceLitInfo li{0u, 0u};
            if ((rc = enqueue_radiance_lit(c, q1, mm, 1u, d_o, d_d, d_rng, texel ? tl.ray_pb : nullptr, d_rgb, d_seg, xl, want_info ? &li : nullptr)))
                return rc;
            shadow[0] += li.shadow_rays;
            shadow[1] += li.shadow_occluded;
        } else if ((rc = enqueue_radiance(c, q1, mm, 1u, d_o, d_d, d_rng, d_rgb, d_seg, xs))) {
            return rc;
        }
        if (texel) {  // the texels' shadow rays: prt_occluded's pipeline, then e onto the query's values
            if ((rc = enqueue_query(c, mm, tl.x, tl.w, tl.tmax, nullptr, d_tocc))) return rc;
            prt_launch_bkl_add(c->stream, mm, tl, d_tocc, d_rgb, d_tstats);
            HIPCHECK(c, hipGetLastError());
        }
        if (out.moments.count) prt_launch_bka_sum(c->stream, n_list, ccs, first && s0 == 0u, d_list, d_rgb, d_seg, out.moments, out.counts);
        else prt_launch_bk_sum(c->stream, n_list, ccs, first && s0 == 0u, d_list, d_rgb, d_seg, out.moments.rgb_sum, out.counts);
        HIPCHECK(c, hipGetLastError());
    }
    if (texel && want_info) {  // (once per call of this function, and only where info is given)
        unsigned long long st[2 * PRT_BKL_STAT_SLOTS];
        HIPCHECK(c, hipMemcpyAsync(st, d_tstats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < PRT_BKL_STAT_SLOTS; ++k) {
            shadow[0] += st[2 * k];
            shadow[1] += st[2 * k + 1];
        }
    }
    return PRT_OK;
}

// Both forms of prt_bake_irradiance: the surface, q.samples samples of every covered texel, the gutter fill.
static int bake_irradiance(PrtContext* c, const PrtBakeTarget* target, const PrtRadianceQuery* q, const PrtBakeOptions* opt, void* out_rgb,
                           void* out_cov, bool device_out, PrtBakeInfo* info) {
    if (!c) return PRT_ERR_INVALID;
    if (!opt) return fail(c, PRT_ERR_INVALID, "prt_bake_irradiance_opt: null options");
    if (opt->reserved != 0u) return fail(c, PRT_ERR_INVALID, "prt_bake_irradiance_opt: reserved = %u, expected 0", opt->reserved);
    const uint32_t dilate = opt->dilate;
    BakeTarget b;
    int rc = check_bake(c, target, q, true, &b);
    if (rc) return rc;
    if (!out_rgb) return fail(c, PRT_ERR_INVALID, "prt_bake_irradiance: null rgb_sum");
    if ((rc = need_device(c))) return rc;
    EventPair tm;  // around the call's device work (PrtBakeInfo.device_ms)
    if (info) {
        HIPCHECK(c, tm.a.create(true));
        HIPCHECK(c, tm.b.create(true));
        HIPCHECK(c, hipEventRecord(ev(tm.a), c->stream));
    }
    BakeBufs x;
    uint32_t counts[PRT_BAKE_COUNTERS] = {};
    if ((rc = enqueue_bake_surface(c, &b, true, &x, counts))) return rc;
    bake_info_surface(info, b, counts);
    const size_t n = (size_t)b.W * b.H;
    const uint32_t n_cov = counts[PRT_BAKE_CNT_COVERED];
    HIPCHECK(c, hipMemsetAsync(x.rgb[0], 0, 3 * n * sizeof(float), c->stream));
    const bool lit = opt->lighting != 0u && c->lighting != (uint32_t)PRT_LIGHTING_OFF;
    const bool texel = lit && opt->texel_light != 0u && q->max_depth != 0u;
    uint64_t shadow[2] = {0u, 0u};
    if (n_cov != 0u) {
        BakeSums out;
        out.moments.rgb_sum = x.rgb[0];
        out.counts = x.counts;
        if ((rc = enqueue_bake_samples(c, *q, lit, texel, x.list, n_cov, x.map, true, out, info != nullptr, shadow))) return rc;
    }
    int cur = 0;
    uint8_t* cov[2] = {x.map.cov, x.cov2};
    for (uint32_t p = 0; p < dilate; ++p) {
        prt_launch_bk_dilate(c->stream, b.W, b.H, cov[cur], x.rgb[cur], cov[cur ^ 1], x.rgb[cur ^ 1], x.counts);
        HIPCHECK(c, hipGetLastError());
        cur ^= 1;
    }
    const hipMemcpyKind kind = device_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHECK(c, hipMemcpyAsync(out_rgb, x.rgb[cur], 3 * n * sizeof(float), kind, c->stream));
    if (out_cov) HIPCHECK(c, hipMemcpyAsync(out_cov, cov[cur], n, kind, c->stream));
    if (info) {
        if ((rc = download(c, counts, x.counts, (size_t)PRT_BAKE_COUNTERS))) return rc;
        HIPCHECK(c, hipEventRecord(ev(tm.b), c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        HIPCHECK(c, hipEventElapsedTime(&ms, ev(tm.a), ev(tm.b)));
        info->n_filled = counts[PRT_BAKE_CNT_FILLED];
        info->rays = (uint64_t)n_cov * q->samples;
        info->segments = (uint64_t)counts[PRT_BAKE_CNT_SEGMENTS] | ((uint64_t)counts[PRT_BAKE_CNT_SEGMENTS + 1u] << 32);
        info->shadow_rays = shadow[0];
        info->shadow_occluded = shadow[1];
        info->device_ms = (double)ms;
    }
    return device_out ? PRT_OK : prt_synchronize(c);  // (host form: waits for the stream and reports a ray a walk had to give up)
}

int prt_bake_irradiance(PrtContext* c, const PrtBakeTarget* target, const PrtRadianceQuery* q, int lighting, uint32_t dilate, float* rgb_sum,
                        uint8_t* coverage, PrtBakeInfo* info) {
    const PrtBakeOptions opt{lighting != 0 ? 1u : 0u, 0u, dilate, 0u};
    return bake_irradiance(c, target, q, &opt, rgb_sum, coverage, false, info);
}

int prt_bake_irradiance_device(PrtContext* c, const PrtBakeTarget* target, const PrtRadianceQuery* q, int lighting, uint32_t dilate, void* d_rgb_sum,
                               void* d_coverage, PrtBakeInfo* info) {
    const PrtBakeOptions opt{lighting != 0 ? 1u : 0u, 0u, dilate, 0u};
    return bake_irradiance(c, target, q, &opt, d_rgb_sum, d_coverage, true, info);
}

int prt_bake_irradiance_opt(PrtContext* c, const PrtBakeTarget* target, const PrtRadianceQuery* q, const PrtBakeOptions* options, float* rgb_sum,
                            uint8_t* coverage, PrtBakeInfo* info) {
    return bake_irradiance(c, target, q, options, rgb_sum, coverage, false, info);
}

int prt_bake_irradiance_opt_device(PrtContext* c, const PrtBakeTarget* target, const PrtRadianceQuery* q, const PrtBakeOptions* options,
                                   void* d_rgb_sum, void* d_coverage, PrtBakeInfo* info) {
    return bake_irradiance(c, target, q, options, d_rgb_sum, d_coverage, true, info);
}

int prt_bake_light_samples(PrtContext* c, const PrtBakeTarget* target, uint32_t seed, uint32_t sample, float* dirs, float* tmax, uint32_t* light,
                           float* contrib, float* ray_pb) {
    BakeTarget b;
    int rc = check_bake(c, target, nullptr, false, &b);
    if (rc) return rc;
    if ((rc = need_device(c))) return rc;
    BakeBufs x;
    uint32_t counts[PRT_BAKE_COUNTERS] = {};
    if ((rc = enqueue_bake_surface(c, &b, false, &x, counts))) return rc;
    const size_t n = (size_t)b.W * b.H;
    float *d_o, *d_d;
    uint32_t* d_rng;
    PrtBakeLightRays tl{};
    PrtWorkspace ws;
    ws.add(&d_o, 3 * n).add(&d_d, 3 * n).add(&d_rng, n);
    ws.add(&tl.w, 3 * n).add(&tl.tmax, n).add(&tl.contrib, 3 * n).add(&tl.light, n).add(&tl.ray_pb, n);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = sync_light_tables(c))) return rc;
    const PrtBakeLightArgs la{dev_lights(c), dev_mesh_lights(c), dev_light_clusters(c), env_on(c) ? dev_env(c) : DevEnv{}, c->sampling.clamp};
    prt_launch_bk_rays(c->stream, (uint32_t)n, 1u, sample, seed, nullptr, x.map, d_o, d_d, d_rng);
    HIPCHECK(c, hipGetLastError());
    prt_launch_bkl_sample(c->stream, mesh_lights_on(c), env_on(c), clusters_on(c), (uint32_t)n, 1u, sample, seed, nullptr, x.map, d_d, la, tl);
    HIPCHECK(c, hipGetLastError());
    std::vector<uint32_t> cand(light ? n : 0);
    if (dirs && (rc = download(c, dirs, tl.w, 3 * n))) return rc;
    if (tmax && (rc = download(c, tmax, tl.tmax, n))) return rc;
    if (light && (rc = download(c, cand.data(), tl.light, n))) return rc;
    if (contrib && (rc = download(c, contrib, tl.contrib, 3 * n))) return rc;
    if (ray_pb && (rc = download(c, ray_pb, tl.ray_pb, n))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    // (the kernel reports the candidate; the light set proper leaves out the candidates with an empty interval)
    for (size_t i = 0; light && i < n; ++i)
        light[i] = (mesh_lights_on(c) && cand[i] != 0xFFFFFFFFu && cand[i] != PRT_LIGHT_ENVIRONMENT) ? c->hs.ml.cand_visible[cand[i]] : cand[i];
    return PRT_OK;
}

// ---- bake statistics and adaptive sampling (include/prt.h "Bake statistics and adaptive sampling") -----------
struct BakeAdaptiveOut {
    void *rgb_sum, *count, *sum_y, *sum_y2, *rgb_mean, *coverage;
};

// Both forms of prt_bake_irradiance_adaptive: prt_render_adaptive's loop over 8 x 8 blocks of texels.  Pass 0 is the bake's
// own sequence over the covered texels; every later pass selects (k_bka_select, k_bka_blocks), lists the covered texels of the
// active blocks in ascending order (k_bk_compact over the `active` bytes), reads the two lengths back and runs the same
// sequence over that list.  k_bka_sum stands where k_bk_sum stands.
static int bake_irradiance_adaptive(PrtContext* c, const PrtBakeTarget* target, const PrtRadianceQuery* q, const PrtBakeOptions* opt,
                                    const PrtBakeAdaptive* cfg, const BakeAdaptiveOut& o, bool device_out, PrtBakeInfo* info,
                                    PrtBakeAdaptiveInfo* ainfo) {
    if (!c) return PRT_ERR_INVALID;
    const char* who = "prt_bake_irradiance_adaptive";
    if (!opt) return fail(c, PRT_ERR_INVALID, "%s: null options", who);
    if (opt->reserved != 0u) return fail(c, PRT_ERR_INVALID, "%s: options.reserved = %u, expected 0", who, opt->reserved);
    BakeTarget b;
    int rc = check_bake(c, target, nullptr, false, &b);
    if (rc) return rc;
    if (!q) return fail(c, PRT_ERR_INVALID, "%s: null query", who);
    if (const char* why = prt_bake_adaptive_refusal(cfg, b.W, b.H)) return fail(c, PRT_ERR_INVALID, "%s: %s", who, why);
    if (!o.rgb_sum) return fail(c, PRT_ERR_INVALID, "%s: null rgb_sum", who);
    if ((rc = need_device(c))) return rc;
    EventPair tm;  // around the call's device work (PrtBakeInfo.device_ms)
    if (info) {
        HIPCHECK(c, tm.a.create(true));
        HIPCHECK(c, tm.b.create(true));
        HIPCHECK(c, hipEventRecord(ev(tm.a), c->stream));
    }
    BakeBufs x;
    BakeAdaptiveBufs ax;
    uint32_t counts[PRT_BAKE_COUNTERS] = {};
    if ((rc = enqueue_bake_surface(c, &b, true, &x, counts, &ax))) return rc;
    bake_info_surface(info, b, counts);
    const size_t n = (size_t)b.W * b.H;
    const uint32_t n_cov = counts[PRT_BAKE_CNT_COVERED], n_blocks = prt_bake_block_count(b.W, b.H);
    HIPCHECK(c, hipMemsetAsync(x.rgb[0], 0, 3 * n * sizeof(float), c->stream));
    HIPCHECK(c, hipMemsetAsync(ax.count, 0, n * sizeof(float), c->stream));
    HIPCHECK(c, hipMemsetAsync(ax.sum_y, 0, n * sizeof(float), c->stream));
    HIPCHECK(c, hipMemsetAsync(ax.sum_y2, 0, n * sizeof(float), c->stream));
    const bool lit = opt->lighting != 0u && c->lighting != (uint32_t)PRT_LIGHTING_OFF;
    const bool texel = lit && opt->texel_light != 0u && q->max_depth != 0u;
    uint64_t shadow[2] = {0u, 0u};
    BakeSums out;
    out.moments = PrtBakeMoments{x.rgb[0], ax.count, ax.sum_y, ax.sum_y2};
    out.counts = x.counts;
    PrtBakeAdaptiveInfo ai{};
    ai.blocks = n_blocks;
    uint32_t added = cfg->min_spp;
    if (n_cov != 0u) {  // pass 0: every covered texel, as prt_bake_irradiance_opt has it
        const PrtRadianceQuery q0{q->max_depth, cfg->min_spp, q->seed, q->first_sample};
        if ((rc = enqueue_bake_samples(c, q0, lit, texel, x.list, n_cov, x.map, true, out, info != nullptr, shadow))) return rc;
        ai.texel_samples = (uint64_t)cfg->min_spp * n_cov;
        ai.min_texel_spp = ai.max_texel_spp = cfg->min_spp;
    }
    if (cfg->max_spp > cfg->min_spp) {
        bool any = false;
        auto stopped_at = [&](uint32_t spp) {  // some covered texels end with this count
            ai.min_texel_spp = any ? std::min(ai.min_texel_spp, spp) : spp;
            ai.max_texel_spp = any ? std::max(ai.max_texel_spp, spp) : spp;
            any = true;
        };
        HIPCHECK(c, hipMemsetAsync(ax.active, 0, n, c->stream));
        const uint32_t* prev = nullptr;
        uint32_t n_prev = n_blocks, len_prev = n_cov, cur = 0;
        while (n_prev) {
            // which of the blocks that were active until now still are, and their covered texels; ONE small wait per pass
            const bool at_cap = added >= cfg->max_spp;
            HIPCHECK(c, hipMemsetAsync(ax.sel, 0, PRT_BKA_COUNTERS * sizeof(uint32_t), c->stream));
            prt_launch_bka_select(c->stream, b.W, b.H, x.map.cov, out.moments, prev, n_prev, cfg->threshold, cfg->noise_floor, at_cap, ax.flags,
                                  ax.active, ax.sel);
            HIPCHECK(c, hipGetLastError());
            prt_launch_bka_blocks(c->stream, n_prev, prev, ax.flags, ax.blist[cur], ax.sel);
            HIPCHECK(c, hipGetLastError());
            prt_launch_bk_compact(c->stream, (uint32_t)n, ax.active, ax.tlist, ax.sel);
            HIPCHECK(c, hipGetLastError());
            uint32_t sel[PRT_BKA_COUNTERS] = {};
            if ((rc = download(c, sel, ax.sel, (size_t)PRT_BKA_COUNTERS))) return rc;
            HIPCHECK(c, hipStreamSynchronize(c->stream));
            const uint32_t n_act = sel[PRT_BKA_CNT_ACTIVE], len = sel[PRT_BAKE_CNT_COVERED];
            if (n_act > n_prev || len > len_prev || sel[PRT_BKA_CNT_CONVERGED] != n_prev - n_act)
                return fail(c, PRT_ERR_HIP, "%s: the selection returned %u of %u blocks, %u of %u texels", who, n_act, n_prev, len, len_prev);
            ai.blocks_converged += n_prev - n_act;
            if (len < len_prev) stopped_at(added);
            if (n_act == 0u) break;
            if (at_cap) {
                ai.blocks_capped = sel[PRT_BKA_CNT_CAPPED];
                stopped_at(added);
                break;
            }
            const uint32_t k = std::min(cfg->step_spp, cfg->max_spp - added);
            const PrtRadianceQuery qk{q->max_depth, k, q->seed, q->first_sample + added};
            if ((rc = enqueue_bake_samples(c, qk, lit, texel, ax.tlist, len, x.map, false, out, info != nullptr, shadow))) return rc;
            added += k;
            ai.texel_samples += (uint64_t)k * len;
            ++ai.passes;
            prev = ax.blist[cur];
            n_prev = n_act;
            len_prev = len;
            cur ^= 1u;
        }
    }
    // the mean, and the gutter fill on (coverage, mean) only: x.rgb[1] and ax.mean2 ping-pong
    float* mean[2] = {x.rgb[1], ax.mean2};
    uint8_t* cov[2] = {x.map.cov, x.cov2};
    int cur = 0;
    const bool want_mean = o.rgb_mean != nullptr || opt->dilate != 0u;
    if (want_mean) {
        prt_launch_bka_mean(c->stream, (uint32_t)n, x.rgb[0], ax.count, mean[0]);
        HIPCHECK(c, hipGetLastError());
        for (uint32_t p = 0; p < opt->dilate; ++p) {
            prt_launch_bk_dilate(c->stream, b.W, b.H, cov[cur], mean[cur], cov[cur ^ 1], mean[cur ^ 1], x.counts);
            HIPCHECK(c, hipGetLastError());
            cur ^= 1;
        }
    }
    const hipMemcpyKind kind = device_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHECK(c, hipMemcpyAsync(o.rgb_sum, x.rgb[0], 3 * n * sizeof(float), kind, c->stream));
    if (o.count) HIPCHECK(c, hipMemcpyAsync(o.count, ax.count, n * sizeof(float), kind, c->stream));
    if (o.sum_y) HIPCHECK(c, hipMemcpyAsync(o.sum_y, ax.sum_y, n * sizeof(float), kind, c->stream));
    if (o.sum_y2) HIPCHECK(c, hipMemcpyAsync(o.sum_y2, ax.sum_y2, n * sizeof(float), kind, c->stream));
    if (o.rgb_mean) HIPCHECK(c, hipMemcpyAsync(o.rgb_mean, mean[cur], 3 * n * sizeof(float), kind, c->stream));
    if (o.coverage) HIPCHECK(c, hipMemcpyAsync(o.coverage, cov[cur], n, kind, c->stream));
    if (info) {
        if ((rc = download(c, counts, x.counts, (size_t)PRT_BAKE_COUNTERS))) return rc;
        HIPCHECK(c, hipEventRecord(ev(tm.b), c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        HIPCHECK(c, hipEventElapsedTime(&ms, ev(tm.a), ev(tm.b)));
        info->n_filled = counts[PRT_BAKE_CNT_FILLED];
        info->rays = ai.texel_samples;
        info->segments = (uint64_t)counts[PRT_BAKE_CNT_SEGMENTS] | ((uint64_t)counts[PRT_BAKE_CNT_SEGMENTS + 1u] << 32);
        info->shadow_rays = shadow[0];
        info->shadow_occluded = shadow[1];
        info->device_ms = (double)ms;
    }
    if (ainfo) *ainfo = ai;
    return device_out ? PRT_OK : prt_synchronize(c);  // (host form: waits for the stream and reports a ray a walk had to give up)
}

int prt_bake_irradiance_adaptive(PrtContext* c, const PrtBakeTarget* target, const PrtRadianceQuery* q, const PrtBakeOptions* options,
                                 const PrtBakeAdaptive* cfg, float* rgb_sum, float* count, float* sum_y, float* sum_y2, float* rgb_mean,
                                 uint8_t* coverage, PrtBakeInfo* info, PrtBakeAdaptiveInfo* adaptive_info) {
    return bake_irradiance_adaptive(c, target, q, options, cfg, BakeAdaptiveOut{rgb_sum, count, sum_y, sum_y2, rgb_mean, coverage}, false, info,
                                    adaptive_info);
}

int prt_bake_irradiance_adaptive_device(PrtContext* c, const PrtBakeTarget* target, const PrtRadianceQuery* q, const PrtBakeOptions* options,
                                        const PrtBakeAdaptive* cfg, void* d_rgb_sum, void* d_count, void* d_sum_y, void* d_sum_y2,
                                        void* d_rgb_mean, void* d_coverage, PrtBakeInfo* info, PrtBakeAdaptiveInfo* adaptive_info) {
    return bake_irradiance_adaptive(c, target, q, options, cfg, BakeAdaptiveOut{d_rgb_sum, d_count, d_sum_y, d_sum_y2, d_rgb_mean, d_coverage},
                                    true, info, adaptive_info);
}

int prt_bake_block_select(PrtContext* c, uint32_t W, uint32_t H, const uint8_t* coverage, const float* count, const float* sum_y,
                          const float* sum_y2, const uint32_t* prev, uint32_t n_prev, float threshold, float noise_floor, uint32_t* block_list,
                          uint32_t* texel_list, uint32_t* counts) {
    if (!c) return PRT_ERR_INVALID;
    const char* who = "prt_bake_block_select";
    if (W == 0u || H == 0u || W > PRT_TEX_MAX_SIZE || H > PRT_TEX_MAX_SIZE)
        return fail(c, PRT_ERR_INVALID, "%s: a %u x %u map, expected 1 .. %u each way", who, W, H, PRT_TEX_MAX_SIZE);
    if (!coverage || !count || !sum_y || !sum_y2 || !block_list || !texel_list || !counts) return fail(c, PRT_ERR_INVALID, "%s: null array", who);
    const uint32_t n_blocks = prt_bake_block_count(W, H);
    if (n_prev > n_blocks) return fail(c, PRT_ERR_INVALID, "%s: n_prev %u above the map's %u blocks", who, n_prev, n_blocks);
    for (uint32_t i = 0; prev && i < n_prev; ++i)
        if (prev[i] >= n_blocks) return fail(c, PRT_ERR_INVALID, "%s: prev[%u] = %u is not one of the %u blocks", who, i, prev[i], n_blocks);
    if (const char* why = prt_bake_rule_refusal(threshold, noise_floor)) return fail(c, PRT_ERR_INVALID, "%s: %s", who, why);
    int rc = need_device(c);
    if (rc) return rc;
    const size_t n = (size_t)W * H, n_ent = std::max(n_prev, 1u);
    PrtBakeMoments m{};
    uint8_t *d_cov, *d_active;
    uint32_t *d_prev, *d_flags, *d_blist, *d_tlist, *d_sel;
    PrtWorkspace ws;
    ws.add(&d_cov, n).add(&m.count, n).add(&m.sum_y, n).add(&m.sum_y2, n).add(&d_active, n).add(&d_tlist, n);
    ws.add(&d_prev, n_ent).add(&d_flags, n_ent).add(&d_blist, n_ent).add(&d_sel, (size_t)PRT_BKA_COUNTERS);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_cov, coverage, n)) || (rc = upload(c, m.count, count, n)) || (rc = upload(c, m.sum_y, sum_y, n)) ||
        (rc = upload(c, m.sum_y2, sum_y2, n)))
        return rc;
    if (prev && n_prev && (rc = upload(c, d_prev, prev, n_prev))) return rc;
    HIPCHECK(c, hipMemsetAsync(d_active, 0, n, c->stream));  // (the texels of blocks outside prev)
    HIPCHECK(c, hipMemsetAsync(d_tlist, 0xFF, n * sizeof(uint32_t), c->stream));
    HIPCHECK(c, hipMemsetAsync(d_blist, 0xFF, n_ent * sizeof(uint32_t), c->stream));
    HIPCHECK(c, hipMemsetAsync(d_sel, 0, PRT_BKA_COUNTERS * sizeof(uint32_t), c->stream));
    prt_launch_bka_select(c->stream, W, H, d_cov, m, prev ? d_prev : nullptr, n_prev, threshold, noise_floor, false, d_flags, d_active, d_sel);
    HIPCHECK(c, hipGetLastError());
    prt_launch_bka_blocks(c->stream, n_prev, prev ? d_prev : nullptr, d_flags, d_blist, d_sel);
    HIPCHECK(c, hipGetLastError());
    prt_launch_bk_compact(c->stream, (uint32_t)n, d_active, d_tlist, d_sel);
    HIPCHECK(c, hipGetLastError());
    uint32_t sel[PRT_BKA_COUNTERS] = {};
    if ((rc = download(c, sel, d_sel, (size_t)PRT_BKA_COUNTERS))) return rc;
    if (n_prev && (rc = download(c, block_list, d_blist, n_prev))) return rc;
    if ((rc = download(c, texel_list, d_tlist, n))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    counts[0] = sel[PRT_BKA_CNT_ACTIVE];
    counts[1] = sel[PRT_BAKE_CNT_COVERED];
    return PRT_OK;
}

int prt_bake_noise(uint64_t n, const float* count, const float* sum_y, const float* sum_y2, float noise_floor, float* rel_err) {
    return prt_bake_noise_rule(n, count, sum_y, sum_y2, noise_floor, rel_err) ? PRT_OK : PRT_ERR_INVALID;
}

// ---- SH probes (include/prt.h "SH probes") -----------------------------------------------------------------
// The refusals of both forms, in the order of the header; everything here is decided without a device.
static int check_probe_sh(PrtContext* c, const PrtProbeShOptions* opt, const PrtRadianceQuery* q, uint32_t n, const void* positions,
                          const void* sh_sum, bool host_positions) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (!opt) return fail(c, PRT_ERR_INVALID, "prt_probe_sh: null options");
    if (n != 0u && (!positions || !sh_sum)) return fail(c, PRT_ERR_INVALID, "prt_probe_sh: null array");
    if (opt->reserved[0] != 0u || opt->reserved[1] != 0u)
        return fail(c, PRT_ERR_INVALID, "prt_probe_sh: reserved = %u, %u, expected 0", opt->reserved[0], opt->reserved[1]);
    if (opt->order > PRT_SH_MAX_ORDER) return fail(c, PRT_ERR_INVALID, "prt_probe_sh: order = %u, expected 0 .. %u", opt->order, PRT_SH_MAX_ORDER);
    if (host_positions) {
        const float* x = (const float*)positions;
        for (size_t i = 0; i < 3 * (size_t)n; ++i)
            if (!std::isfinite(x[i])) return fail(c, PRT_ERR_INVALID, "prt_probe_sh: the position of probe %zu is not finite", i / 3);
    }
    if (q && (uint64_t)n * q->samples > 0xFFFFFFFFull)
        return fail(c, PRT_ERR_INVALID, "prt_probe_sh: %u probes x %u samples exceed 2^32 - 1 paths", n, q->samples);
    return check_radiance(c, q, n, positions, positions, nullptr, sh_sum);
}

// Both forms of prt_probe_sh.  The rays of a chunk of whole samples go through the radiance query's own rounds
// (enqueue_radiance / enqueue_radiance_lit with the states given, one sample per ray), sample-major over the probes, and
// k_sh_project adds a probe's projected values in ascending sample order: nothing depends on the chunk.
static int probe_sh(PrtContext* c, const PrtProbeShOptions* opt, const PrtRadianceQuery* q, uint32_t n, const void* positions, void* out,
                    bool device_form, PrtProbeShInfo* info) {
    int rc = check_probe_sh(c, opt, q, n, positions, out, !device_form);
    if (info) *info = PrtProbeShInfo{};
    if (rc || n == 0u) return rc;
    if ((rc = need_device(c))) return rc;
    EventPair tm;  // around the call's device work (PrtProbeShInfo.device_ms)
    if (info) {
        HIPCHECK(c, tm.a.create(true));
        HIPCHECK(c, tm.b.create(true));
        HIPCHECK(c, hipEventRecord(ev(tm.a), c->stream));
    }
    const uint32_t K = prt_sh_count(opt->order);
    const bool lit = opt->lighting != 0u && c->lighting != (uint32_t)PRT_LIGHTING_OFF;
    const uint32_t cs = c->probe_chunk > 0 ? std::min((uint32_t)c->probe_chunk, q->samples) : radiance_chunk(c, *q, n);
    const size_t n1 = n, m = (size_t)cs * n1;
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (as prt_radiance: the scratch may be reallocated)
    float *d_pos = nullptr, *d_sh = nullptr, *d_o, *d_d, *d_rgb;
    uint32_t *d_rng, *d_seg, *d_counts;
    RadianceScratch xs;
    RadianceLitScratch xl;
    PrtWorkspace ws;
    if (!device_form) ws.add(&d_pos, 3 * n1).add(&d_sh, 3 * n1 * K);
    ws.add(&d_counts, (size_t)PRT_PROBE_SH_COUNTERS).add(&d_o, 3 * m).add(&d_d, 3 * m).add(&d_rng, m).add(&d_rgb, 3 * m).add(&d_seg, m);
    if (lit) xl.declare(ws, m, tex_on(c));
    else xs.declare(ws, m, tex_on(c));
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if (device_form) {
        d_pos = (float*)const_cast<void*>(positions);
        d_sh = (float*)out;
    } else if ((rc = upload(c, d_pos, (const float*)positions, 3 * n1))) {
        return rc;
    }
    HIPCHECK(c, hipMemsetAsync(d_counts, 0, PRT_PROBE_SH_COUNTERS * sizeof(uint32_t), c->stream));
    uint64_t shadow[2] = {0u, 0u};
    const PrtRadianceQuery q1{q->max_depth, 1u, q->seed, q->first_sample};  // (one sample per ray: the states are given)
    for (uint32_t s0 = 0; s0 < q->samples; s0 += cs) {
        const uint32_t ccs = std::min(cs, q->samples - s0);
        const uint32_t mm = ccs * n;
        prt_launch_sh_rays(c->stream, n, ccs, q->first_sample + s0, q->seed, d_pos, d_o, d_d, d_rng);
        HIPCHECK(c, hipGetLastError());
        if (lit) {
            PrtRadianceLitInfo li{0u, 0u};
            if ((rc = enqueue_radiance_lit(c, q1, mm, 1u, d_o, d_d, d_rng, nullptr, d_rgb, d_seg, xl, info ? &li : nullptr))) return rc;
            shadow[0] += li.shadow_rays;
            shadow[1] += li.shadow_occluded;
        } else if ((rc = enqueue_radiance(c, q1, mm, 1u, d_o, d_d, d_rng, d_rgb, d_seg, xs))) {
            return rc;
        }
        prt_launch_sh_project(c->stream, n, ccs, K, s0 == 0u, d_d, d_rgb, d_seg, d_sh, d_counts);
        HIPCHECK(c, hipGetLastError());
    }
    if (!device_form && (rc = download(c, (float*)out, d_sh, 3 * n1 * K))) return rc;
    if (info) {
        uint32_t counts[PRT_PROBE_SH_COUNTERS] = {};
        if ((rc = download(c, counts, d_counts, (size_t)PRT_PROBE_SH_COUNTERS))) return rc;
        HIPCHECK(c, hipEventRecord(ev(tm.b), c->stream));
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        HIPCHECK(c, hipEventElapsedTime(&ms, ev(tm.a), ev(tm.b)));
        info->n_probes = n;
        info->rays = (uint64_t)n * q->samples;
        info->segments = (uint64_t)counts[PRT_PROBE_SH_CNT_SEGMENTS] | ((uint64_t)counts[PRT_PROBE_SH_CNT_SEGMENTS + 1u] << 32);
        info->shadow_rays = shadow[0];
        info->shadow_occluded = shadow[1];
        info->device_ms = (double)ms;
    }
    return device_form ? PRT_OK : prt_synchronize(c);  // (host form: waits for the stream and reports a ray a walk had to give up)
}

int prt_probe_sh(PrtContext* c, const PrtProbeShOptions* options, const PrtRadianceQuery* q, uint32_t n_probes, const float* positions,
                 float* sh_sum, PrtProbeShInfo* info) {
    return probe_sh(c, options, q, n_probes, positions, sh_sum, false, info);
}

int prt_probe_sh_device(PrtContext* c, const PrtProbeShOptions* options, const PrtRadianceQuery* q, uint32_t n_probes, const void* d_positions,
                        void* d_sh_sum, PrtProbeShInfo* info) {
    return probe_sh(c, options, q, n_probes, d_positions, d_sh_sum, true, info);
}

int prt_probe_sh_rays(PrtContext* c, uint32_t n, const float* positions, uint32_t seed, uint32_t sample, float* origins, float* dirs,
                      uint32_t* rng_state) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (n != 0u && (!positions || !origins || !dirs || !rng_state)) return fail(c, PRT_ERR_INVALID, "prt_probe_sh_rays: null array");
    for (size_t i = 0; i < 3 * (size_t)n; ++i)
        if (!std::isfinite(positions[i])) return fail(c, PRT_ERR_INVALID, "prt_probe_sh_rays: the position of probe %zu is not finite", i / 3);
    if (n == 0u) return PRT_OK;
    int rc = need_device(c);
    if (rc) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (the scratch may be reallocated)
    const size_t n1 = n;
    float *d_pos, *d_o, *d_d;
    uint32_t* d_rng;
    PrtWorkspace ws;
    ws.add(&d_pos, 3 * n1).add(&d_o, 3 * n1).add(&d_d, 3 * n1).add(&d_rng, n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_pos, positions, 3 * n1))) return rc;
    prt_launch_sh_rays(c->stream, n, 1u, sample, seed, d_pos, d_o, d_d, d_rng);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, origins, d_o, 3 * n1)) || (rc = download(c, dirs, d_d, 3 * n1)) || (rc = download(c, rng_state, d_rng, n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

int prt_sh_eval(uint32_t n, const float* dirs, uint32_t order, float* Y) {
    return prt_sh_eval_rule(n, dirs, order, Y) ? PRT_OK : PRT_ERR_INVALID;
}

int prt_sh_irradiance(uint32_t n, const float* coeffs, const float* normals, uint32_t order, float* E) {
    return prt_sh_irradiance_rule(n, coeffs, normals, order, E) ? PRT_OK : PRT_ERR_INVALID;
}

int prt_sample_light(PrtContext* c, uint32_t n, const float* in_dirs, const PrtHit* hits, const uint32_t* keys,
                     float* shadow_dirs, float* tmax, uint32_t* light, float* contrib, float* pdf_light, float* pdf_bsdf,
                     float* w_light, float* w_bsdf) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (n == 0) return PRT_OK;
    if (!in_dirs || !hits || !keys || !shadow_dirs || !tmax || !light || !contrib || !pdf_light || !pdf_bsdf || !w_light || !w_bsdf)
        return fail(c, PRT_ERR_INVALID, "null array");
    for (uint32_t i = 0; i < n; ++i)
        if (hits[i].prim >= 0 && hits[i].material_id >= c->hs.materials.size())
            return fail(c, PRT_ERR_INVALID, "hit %u: material out of range", i);
    const size_t n1 = n;
    PrtHit* d_h;
    float *d_in, *d_f;  // d_f: 11 floats per ray
    uint32_t *d_k, *d_l;
    PrtWorkspace ws;
    ws.add(&d_h, n1).add(&d_in, 3 * n1).add(&d_k, n1).add(&d_l, n1).add(&d_f, 11 * n1);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, d_h, hits, n1)) || (rc = upload(c, d_in, in_dirs, 3 * n1)) || (rc = upload(c, d_k, keys, n1))) return rc;
    const DevMeshLights mlt = dev_mesh_lights(c);
    const DevLightClusters lct = dev_light_clusters(c);
    if ((rc = sync_light_tables(c))) return rc;
    const DevEnv denv = dev_env(c);
    prt_launch_sample_light_test(c->stream, c->dsc, dev_lights(c), n, d_in, d_h, d_k, d_f, d_l, mesh_lights_on(c) ? &mlt : nullptr,
                                 env_on(c) ? &denv : nullptr, clusters_on(c) ? &lct : nullptr);
    HIPCHECK(c, hipGetLastError());
    std::vector<float> f(11 * n1);
    if ((rc = download(c, f.data(), d_f, 11 * n1)) || (rc = download(c, light, d_l, n1))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        const float* r = &f[11 * i];
        for (int a = 0; a < 3; ++a) {
            shadow_dirs[3 * i + a] = r[a];
            contrib[3 * i + a] = r[4 + a];
        }
        tmax[i] = r[3];
        pdf_light[i] = r[7];
        pdf_bsdf[i] = r[8];
        w_light[i] = r[9];
        w_bsdf[i] = r[10];
        // (the kernel reports the candidate; the light set proper leaves out the candidates with an empty interval)
        if (mesh_lights_on(c) && light[i] != 0xFFFFFFFFu && light[i] != PRT_LIGHT_ENVIRONMENT) light[i] = c->hs.ml.cand_visible[light[i]];
    }
    return PRT_OK;
}

int prt_tile_select(PrtContext* c, const float* n, const float* sum_y, const float* sum_y2, const uint32_t* prev, uint32_t n_prev,
                    float threshold, float noise_floor, uint32_t* list, uint32_t* counts) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_film) return fail(c, PRT_ERR_INVALID, "prt_set_film has not been called");
    if (!n || !sum_y || !sum_y2 || !list || !counts) return fail(c, PRT_ERR_INVALID, "prt_tile_select: null array");
    if (!(threshold >= 0.0f) || !(noise_floor >= 0.0f))
        return fail(c, PRT_ERR_INVALID, "threshold and noise_floor must be >= 0 (and not NaN)");
    if (threshold == 0.0f && noise_floor == 0.0f) return fail(c, PRT_ERR_INVALID, "threshold and noise_floor are both 0");
    const PrtTileMap& tm = c->tm;
    if (n_prev > tm.n_tiles_local)
        return fail(c, PRT_ERR_INVALID, "prt_tile_select: n_prev %u above the %u local tiles", n_prev, tm.n_tiles_local);
    for (uint32_t i = 0; prev && i < n_prev; ++i)
        if (prev[i] >= tm.n_tiles_local)
            return fail(c, PRT_ERR_INVALID, "prt_tile_select: prev[%u] = %u is not one of the %u local tiles", i, prev[i], tm.n_tiles_local);
    int rc = need_device(c);
    if (rc) return rc;
    // the images in tile layout, as the film and its moments lie on the device; padding lanes (of partial tiles and of the
    // tail) stay zero, which the rule calls unconverged (n < 2): only the kernel's `inside` test keeps them out
    const size_t n_pix = std::max<size_t>(tm.n_pix_local, 64), n_ent = std::max(n_prev, 1u);
    std::vector<float> film(4 * n_pix, 0.0f), stat(2 * n_pix, 0.0f);
    for_each_local_pixel(tm, [&](size_t pl, size_t p) {
        film[4 * pl + 3] = n[p];
        stat[2 * pl] = sum_y[p];
        stat[2 * pl + 1] = sum_y2[p];
    });
    float4* d_film;
    float2* d_stat;
    uint32_t *d_count, *d_prev, *d_flags, *d_list;
    PrtWorkspace ws;
    ws.add(&d_film, n_pix).add(&d_stat, n_pix).add(&d_count, 16).add(&d_prev, n_ent).add(&d_flags, n_ent).add(&d_list, n_ent);
    if ((rc = commit(c, ws, c->scratch))) return rc;
    if ((rc = upload(c, (float*)d_film, film.data(), 4 * n_pix)) || (rc = upload(c, (float*)d_stat, stat.data(), 2 * n_pix))) return rc;
    if (prev && n_prev && (rc = upload(c, d_prev, prev, n_prev))) return rc;
    HIPCHECK(c, hipMemsetAsync(d_list, 0xFF, n_ent * sizeof(uint32_t), c->stream));  // (an entry the kernel leaves unwritten shows as one)
    prt_launch_tile_select(c->stream, d_film, d_stat, tm, prev ? d_prev : nullptr, n_prev, threshold, noise_floor, d_flags, d_list,
                           d_count);
    HIPCHECK(c, hipGetLastError());
    if ((rc = download(c, counts, d_count, 2))) return rc;
    if (n_prev && (rc = download(c, list, d_list, n_prev))) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return PRT_OK;
}

// ---- measurement -----------------------------------------------------------------------------------
int prt_enable_timing(PrtContext* c, int on) {
    if (!c) return PRT_ERR_INVALID;
    c->timing = on != 0;
    return PRT_OK;
}

int prt_get_stats(PrtContext* c, PrtStats* out) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!out) return PRT_ERR_INVALID;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if ((rc = drain_events(c))) return rc;
    PrtStats s = c->stats;
    if (c->wk.ray_stats.p) {
        unsigned long long h[PRT_MAX_DEPTH];
        if ((rc = read_ray_stats(c, c->wk.ray_stats.as<unsigned long long>(), h))) return rc;
        s.rays_total = 0;
        for (int d = 0; d < PRT_MAX_DEPTH; ++d) {
            s.rays_per_depth[d] = h[d];
            s.rays_total += h[d];
        }
    }
    *out = s;
    return PRT_OK;
}

int prt_reset_stats(PrtContext* c) {
    int rc = need_device(c);
    if (rc) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if ((rc = drain_events(c))) return rc;
    memset(&c->stats, 0, sizeof(c->stats));
    c->dead_paths = 0;
    // (stream-ordered, like the counting kernels that follow: see ensure_light_state)
    if (c->wk.ray_stats.p) HIPCHECK(c, hipMemsetAsync(c->wk.ray_stats.p, 0, kRayStatWords * sizeof(unsigned long long), c->stream));
    if (c->wk.light_stats.p) HIPCHECK(c, hipMemsetAsync(c->wk.light_stats.p, 0, kLightStatWords * sizeof(unsigned long long), c->stream));
    return PRT_OK;
}

int prt_measure_traversal(PrtContext* c, uint32_t max_depth, uint32_t seed, uint32_t sample, PrtStats* out) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!out || max_depth == 0 || max_depth > PRT_MAX_DEPTH) return fail(c, PRT_ERR_INVALID, "bad arguments");
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    {
        std::vector<unsigned long long> init(kTravStatsWords, 0ull);
        for (uint32_t d = 0; d <= PRT_MAX_DEPTH; ++d) init[16 + PRT_TIMELINE_WORDS * d] = init[16 + PRT_TIMELINE_WORDS * d + 2] = ~0ull;  // minima
        HIPCHECK(c, hipMemcpy(c->wk.trav_stats.p, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    }
    const bool timing = c->timing;
    const uint64_t launches = c->stats.intersect_launches;
    c->timing = false;
    // the per-depth ray counters are cumulative: this run counts into the scratch set
    unsigned long long before[PRT_MAX_DEPTH] = {}, after[PRT_MAX_DEPTH];
    HIPCHECK(c, hipMemsetAsync(c->wk.ray_stats.as<unsigned long long>() + kRayStatWords, 0, kRayStatWords * sizeof(unsigned long long), c->stream));
    c->ray_stats_target = c->wk.ray_stats.as<unsigned long long>() + kRayStatWords;
    // measure_spp (prt_set_param) samples in one batch: the counters scale, the per-phase cycle split becomes that of a
    // loaded kernel
    rc = run_batch(c, whole_film(c), (uint32_t)std::max(1, c->measure_spp), max_depth, seed, sample, false, c->wk.trav_stats.as<unsigned long long>());
    c->ray_stats_target = c->wk.ray_stats.as<unsigned long long>();
    c->timing = timing;
    c->stats.intersect_launches = launches;
    if (rc) return rc;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    if ((rc = read_ray_stats(c, c->wk.ray_stats.as<unsigned long long>() + kRayStatWords, after))) return rc;
    unsigned long long t[kTravStatsWords];
    std::vector<uint32_t> cnt((size_t)(PRT_MAX_DEPTH + 2) * PRT_CNT_STRIDE);
    HIPCHECK(c, hipMemcpy(t, c->wk.trav_stats.as<unsigned long long>(), sizeof(t), hipMemcpyDeviceToHost));
    if (getenv("PRT_TAIL_PROBE")) {  // diagnostic: where a launch of the 8-wide kernel spends its wall time (100 MHz ticks -> us)
        for (uint32_t d = 0; d < max_depth; ++d) {
            const unsigned long long* tl = t + 16 + PRT_TIMELINE_WORDS * d;
            if (tl[6] == 0ull) continue;
            fprintf(stderr,
                    "[prt tail probe] bounce %u: launch %.1f us, first wave out of rays at %.1f us, last at %.1f us, drain after "
                    "the first %.1f us; per wave: mean life %.1f us, mean drain %.1f us (%llu waves); longest ray %llu node steps\n",
                    d, (tl[1] - tl[0]) * 0.01, (tl[2] - tl[0]) * 0.01, (tl[3] - tl[0]) * 0.01, (tl[1] - tl[2]) * 0.01,
                    tl[5] * 0.01 / tl[6], tl[4] * 0.01 / tl[6], tl[6], tl[7]);
        }
    }
    HIPCHECK(c, hipMemcpy(cnt.data(), c->wk.counts.p, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    uint64_t front = 0;
    for (uint32_t d = 0; d < max_depth; ++d) {
        // rays handed to the traversal kernel in bounce iteration d (bounce 0 with one walk per pixel: the front-pixel list)
        front += cnt[(size_t)d * PRT_CNT_STRIDE + ((d == 0 && c->batch_walked) ? PRT_CNT_LIST : 0u)];
        out->rays_per_depth[d] = after[d] - before[d];
        out->rays_total += out->rays_per_depth[d];
    }
    out->rays_traversed = front;
    out->samples = (uint64_t)std::max(1, c->measure_spp);
    out->bvh_node_visits = t[0];
    out->bvh_tri_tests = t[1];
    out->prim_tests = (uint64_t)c->hs.prims.size() * out->rays_total;  // every ray scans every analytic primitive
    out->node_lane_slots = t[3];
    out->tri_lane_slots = t[4];
    out->max_stack_used = t[5];
    out->wave_cycles_refill = t[6];
    out->wave_cycles_node = t[7];
    out->wave_cycles_tri = t[8];
    return PRT_OK;
}

// Diagnostic: one batch of measure_spp samples (film untouched) with k_shade_divstats in front of every k_shade.
int prt_measure_shade_divergence(PrtContext* c, uint32_t max_depth, uint32_t seed, uint32_t sample, uint64_t* out) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (!out || max_depth == 0 || max_depth > PRT_MAX_DEPTH) return PRT_ERR_INVALID;
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    const size_t bytes = 16 * (size_t)PRT_MAX_DEPTH * sizeof(unsigned long long);
    DevBuf buf;  // (freed when the function returns)
    HIPCHECK(c, buf.ensure(bytes));
    hipError_t e = hipMemsetAsync(buf.p, 0, bytes, c->stream);
    if (e == hipSuccess) {
        c->d_shade_div = buf.as<unsigned long long>();
        c->ray_stats_target = c->wk.ray_stats.as<unsigned long long>() + kRayStatWords;  // (the run's rays are not the context's)
        const bool timing = c->timing;
        const uint64_t launches = c->stats.intersect_launches;
        c->timing = false;
        rc = run_batch(c, whole_film(c), (uint32_t)std::max(1, c->measure_spp), max_depth, seed, sample, false, nullptr);
        c->timing = timing;
        c->stats.intersect_launches = launches;
        c->d_shade_div = nullptr;
        c->ray_stats_target = c->wk.ray_stats.as<unsigned long long>();
        if (!rc) e = hipStreamSynchronize(c->stream);
        if (!rc && e == hipSuccess) e = hipMemcpy(out, buf.p, 16 * (size_t)max_depth * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    }
    if (rc) return rc;
    HIPCHECK(c, e);
    return PRT_OK;
}

int prt_kernel_occupancy(PrtContext* c, PrtOccupancy* out) {
    int rc = need_device(c);
    if (rc) return rc;
    if (!out) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    int nb = 0, vg = 0, sg = 0, lds = 0;
    const PrtWalkPlan plan = prt_plan_walk(walk_facts(c, c->tune, PRT_WALK_CLOSEST, 0u, false, false));
    if (prt_walk_occupancy(plan, &nb, &vg, &sg, &lds)) return fail(c, PRT_ERR_HIP, "occupancy query failed");
    hipDeviceProp_t prop;
    HIPCHECK(c, hipGetDeviceProperties(&prop, c->device));
    out->blocks_per_cu = (uint32_t)nb;
    out->waves_per_cu = (uint32_t)nb * 4u;  // 256-thread blocks = 4 wave64
    out->max_waves_per_cu = (uint32_t)(prop.maxThreadsPerMultiProcessor / 64);
    out->vgprs = (uint32_t)vg;
    out->lds_bytes_per_block = (uint32_t)lds;
    out->compute_units = (uint32_t)prop.multiProcessorCount;
    out->resident_grid_blocks = plan.resident_grid;
    return PRT_OK;
}

int prt_kernel_instance(PrtContext* c, char* name, uint32_t capacity) {
    if (!c || !name || capacity == 0u) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    snprintf(name, capacity, "%s", prt_plan_walk(walk_facts(c, c->tune, PRT_WALK_CLOSEST, 0u, false, false)).name);
    return PRT_OK;
}

int prt_shade_instance(PrtContext* c, char* name, uint32_t capacity) {
    if (!c || !name || capacity == 0u) return PRT_ERR_INVALID;
    snprintf(name, capacity, "%s", c->shade_instance);
    return PRT_OK;
}

int prt_batch_instance(PrtContext* c, uint32_t stage, char* name, uint32_t capacity) {
    if (!c || !name || capacity == 0u || stage > PRT_STAGE_ACCUMULATE) return PRT_ERR_INVALID;
    snprintf(name, capacity, "%s", c->batch_instance[stage]);
    return PRT_OK;
}

int prt_instance_name(uint32_t stage, uint32_t index, char* name, uint32_t capacity) {
    if (!name || capacity == 0u) return PRT_ERR_INVALID;
    const char* s = nullptr;
    if (stage == PRT_STAGE_RAYGEN && index < PRT_RAYGEN_NONE) s = prt_raygen_name(PrtRaygenInst(index));
    else if ((stage == PRT_STAGE_SHADE0 || stage == PRT_STAGE_SHADE) && index < PRT_SHADE_NONE) s = prt_shade_name(PrtShadeInst(index));
    else if (stage == PRT_STAGE_ACCUMULATE && index < PRT_ACCUMULATE_NONE) s = prt_accumulate_name(PrtAccumulateInst(index));
    if (!s) return PRT_ERR_INVALID;
    snprintf(name, capacity, "%s", s);
    return PRT_OK;
}

int prt_last_segment(PrtContext* c, uint32_t* active, uint32_t* front_rays) {
    if (!c || !active) return PRT_ERR_INVALID;
    *active = c->last_segment_active;
    if (front_rays) {
        *front_rays = 0u;
        if (c->last_batch_depth != 0u && c->wk.counts.p) {
            HIPCHECK(c, hipSetDevice(c->device));
            HIPCHECK(c, hipStreamSynchronize(c->stream));
            HIPCHECK(c, hipMemcpy(front_rays, c->wk.counts.as<uint32_t>() + (size_t)(c->last_batch_depth - 1u) * PRT_CNT_STRIDE, sizeof(uint32_t),
                                  hipMemcpyDeviceToHost));
        }
    }
    return PRT_OK;
}

int prt_primary_reuse(PrtContext* c, uint32_t* active, uint32_t* reused_batches) {
    if (!c || !active) return PRT_ERR_INVALID;
    *active = c->primary_reuse_active;
    if (reused_batches) *reused_batches = c->primary_reused_batches;
    return PRT_OK;
}

int prt_bvh_info(PrtContext* c, PrtBvhInfo* out) {
    if (!c || !out) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    *out = c->hs.bvh_info;
    return PRT_OK;
}

int prt_bvh_read4(PrtContext* c, float* nodes4) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (nodes4) memcpy(nodes4, c->hs.bvh.nodes4.data(), c->hs.bvh.nodes4.size() * 4);
    return PRT_OK;
}

int prt_bvh_read8(PrtContext* c, uint32_t* nodes8) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (const int rc = refresh_host_copies(c)) return rc;
    const std::vector<uint32_t>& n8 = c->hs.nodes8_all.empty() ? c->hs.bvh.nodes8 : c->hs.nodes8_all;
    if (nodes8) memcpy(nodes8, n8.data(), n8.size() * 4);
    return PRT_OK;
}

int prt_bvh_read(PrtContext* c, float* nodes, float* tris) {
    if (!c) return PRT_ERR_INVALID;
    if (!c->has_scene) return fail(c, PRT_ERR_INVALID, "prt_set_scene has not been called");
    if (const int rc = refresh_host_copies(c)) return rc;
    if (nodes) memcpy(nodes, c->hs.bvh.nodes.data(), c->hs.bvh.nodes.size() * 4);
    if (tris) memcpy(tris, c->hs.tri_records.data(), c->hs.tri_records.size() * 4);
    return PRT_OK;
}

int prt_set_param(PrtContext* c, const char* name, int value) {
    if (!c || !name) return PRT_ERR_INVALID;
    touch_scene(c);  // any name: a stale primary stage is a wrong image, a spurious rebuild is half a millisecond
    const std::string n = name;
    if (n == "variant") c->variant = value;
    else if (n == "primary_reuse" && (value == 0 || value == 1)) c->primary_reuse = value;
    else if (n == "grid_blocks" && value > 0 && value <= 8192) c->tune.grid_blocks = (uint32_t)value;
    else if (n == "chunk" && value >= 64 && value % 64 == 0) c->tune.chunk = (uint32_t)value;
    else if (n == "xcd_affinity" && (value == 0 || value == 1)) c->tune.xcd_affinity = (uint32_t)value;
    else if (n == "wide" && (value == 0 || value == 1 || value == 2)) c->tune.wide = (uint32_t)value;
    else if (n == "stack_lds" && (value == 0 || value == 1 || value == 2 || value == 3 || value == 4 || value == 5 || value == 6 || value == 24 || value == 39)) c->tune.stack_lds = (uint32_t)value;
    else if (n == "exact_grids" && (value == 0 || value == 1 || value == 2)) c->tune.exact_grids = (uint32_t)value;
    else if (n == "steal" && value >= 0 && value <= 64) c->tune.steal = (uint32_t)value;
    else if (n == "primary_hit" && (value == 0 || value == 1)) c->tune.primary_hit = (uint32_t)value;
    else if (n == "path_kernel" && value >= 0 && value <= 2) c->tune.path_kernel = (uint32_t)value;
    else if (n == "path_max" && value >= 1) c->tune.path_max = (uint32_t)value;
    else if (n == "sort_rays" && value >= 0 && value <= 2) c->sort_rays = (uint32_t)value;
    else if (n == "last_segment" && value >= 0 && value <= 2) c->last_segment = (uint32_t)value;
    else if (n == "compact_primary" && (value == 0 || value == 1)) c->compact_primary = value;
    else if (n == "primary_walk" && (value == 0 || value == 1)) c->primary_walk = value;
    else if (n == "path_id_order" && (value == 0 || value == 1)) c->path_id_order = value;
    else if (n == "node_stride" && (value == 0 || value == 5 || value == 8)) c->node_stride = value;
    else if (n == "pad_log2" && value >= 8 && value <= 22) c->pad_coeff = std::ldexp(1.0f, -value);
    else if (n == "tail" && value >= 0 && value <= 64) c->tune.tail = (uint32_t)value;
    else if (n == "big" && value >= 1 && value <= 16) c->tune.big = (uint32_t)value;
    else if (n == "static_small" && value >= 0 && value <= 4096) c->tune.static_small = (uint32_t)value;
    else if (n == "big_min" && value >= 1 && value <= 100000) c->tune.big_min = (uint32_t)value;
    else if (n == "big_keep" && value >= 0 && value <= 1024) c->tune.big_keep = (uint32_t)value;
    else if (n == "stack_cap" && value >= 0 && value <= 64) c->tune.stack_cap = (uint32_t)value;
    else if (n == "prim_bvh" && (value == 0 || value == 1)) c->abvh_enabled = value;
    else if (n == "measure_spp" && value >= 1 && value <= 1024) c->measure_spp = value;
    else if (n == "gpu_build" && (value == 0 || value == 1 || value == 2)) c->gpu_build = value;
    else if (n == "fuse" && (value == 0 || value == 1)) c->tune.fuse = (uint32_t)value;
    else if (n == "tri_min" && value >= 0 && value <= 1024) c->tune.tri_min = (uint32_t)value;  // 0 = auto
    else if (n == "refill_min" && value >= 1 && value <= 64) c->tune.refill_min = (uint32_t)value;
    else if (n == "light_buckets" && (value == 0 || value == 1)) c->light_buckets = value;
    else if (n == "denoise_lds" && value >= 0 && value <= 2) c->dn_lds = value;
    else if (n == "feature_chunk" && value >= 0 && value <= (int)PRT_FEATURE_MAX_SAMPLES) c->feature_chunk = value;
    else if (n == "radiance_chunk" && value >= 0 && value <= (int)PRT_RADIANCE_MAX_SAMPLES) c->radiance_chunk = value;
    else if (n == "bake_chunk" && value >= 0 && value <= (int)PRT_RADIANCE_MAX_SAMPLES) c->bake_chunk = value;
    else if (n == "probe_chunk" && value >= 0 && value <= (int)PRT_RADIANCE_MAX_SAMPLES) c->probe_chunk = value;
    else if (n == "exit_max" && value >= 0 && value < 64) c->tune.exit_max = (uint32_t)value;
    else return fail(c, PRT_ERR_INVALID, "unknown parameter or bad value: %s = %d", name, value);
    return PRT_OK;
}

int prt_set_variant(PrtContext* c, int variant) {
    if (!c) return PRT_ERR_INVALID;
    touch_scene(c);
    c->variant = variant;
    return PRT_OK;
}

}  // extern "C"

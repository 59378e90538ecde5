/*
 * prt.h — C-ABI of the MI355X-native wavefront path tracer (libprt.so).
 *
 * This is the drop-in boundary for ONE hot path of Rickyeeeeee/ParallelRayTracing:
 *   camera-ray generation -> closest-hit (BVH traversal + shape intersection)
 *   -> material shade/scatter -> film accumulation.
 * It replaces what the reference's `class Renderer` backends do
 * (reference: src/core/renderer.h:8-16 — Init / ProgressiveRender / SetCamera) and the
 * Film accumulate/display entry points they call (src/core/film.h:10-47).
 *
 * Conventions
 *  - Plain C, no torch / C++ types.  Every call returns 0 on success, nonzero on error;
 *    prt_last_error() gives the message.  No exception crosses this boundary.
 *  - Matrices are column-major float[16], exactly glm::mat4's memory layout
 *    (reference: Transform::m_Mat / m_InvMat, src/core/geometry.h:129-130).
 *  - The film is row-major, row 0 = top of the image, interleaved RGB fp32 *sums* plus a
 *    per-pixel weight (reference: Film::m_Accum / m_Weights, src/core/film.h:54-60).
 *  - All data passed in is COPIED; the library keeps no pointer into caller memory
 *    (the reference backends keep raw non-owning pointers, src/backend/cpu/renderer.cpp:8-15).
 *  - Not thread-safe per context; one context drives one GPU.
 *  - There is NO CPU fallback.  Compute entry points fail with PRT_ERR_NO_DEVICE when no
 *    HIP device is usable.
 */
#ifndef PRT_H
#define PRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRT_VERSION 1

/* status codes */
enum {
    PRT_OK = 0,
    PRT_ERR_INVALID = 1,   /* bad argument / call order */
    PRT_ERR_NO_DEVICE = 2, /* no usable HIP device */
    PRT_ERR_HIP = 3,       /* a HIP runtime call failed */
    PRT_ERR_IO = 4,        /* file could not be read / parsed / written */
    PRT_ERR_NOMEM = 5
};

/* reference: enum class ShapeType, src/core/shape.h:10-15 */
enum { PRT_SHAPE_CIRCLE = 0, PRT_SHAPE_QUAD = 1, PRT_SHAPE_TRIANGLE = 2 };
/* reference: enum MatType, src/core/material_handle.h:13-19 */
enum { PRT_MAT_NONE = 0, PRT_MAT_LAMBERTIAN = 1, PRT_MAT_METAL = 2, PRT_MAT_DIELECTRIC = 3, PRT_MAT_EMISSIVE = 4 };
/* reference: enum class ScenePreset, src/core/scene.h:6-15 */
enum {
    PRT_PRESET_DEFAULT = 0, PRT_PRESET_LIGHT_TEST = 1, PRT_PRESET_MATERIAL_TEST = 2, PRT_PRESET_CORNELL = 3,
    PRT_PRESET_RANDOM_BALLS_SMALL = 4, PRT_PRESET_RANDOM_BALLS_MEDIUM = 5, PRT_PRESET_RANDOM_BALLS_LARGE = 6
};

/* One material.  rgb = albedo (Lambertian, Metal) or emission (Emissive); scalar = roughness
 * (Metal) or refraction index (Dielectric).
 * reference: LambertianMaterial/MetalMaterial/DielectricMaterial/EmissiveMaterial getters,
 * src/core/material.h:38,64-65,102,129. */
typedef struct PrtMaterial {
    uint32_t type;
    float rgb[3];
    float scalar;
} PrtMaterial;

/* One analytic primitive = Shape + Material + Transform.
 * shape_param: CIRCLE {radius, -}; QUAD {width, height}.
 * reference: struct Primitive, src/core/primitive.h:7-12; Circle::getRadius / Quad::GetWidth/GetHeight,
 * src/core/shape.h:25,39-40. */
typedef struct PrtPrimitive {
    uint32_t shape_type;
    float shape_param[2];
    uint32_t material_id;
    float mat[16];
    float inv[16];
} PrtPrimitive;

/* One triangle mesh in WORLD space (its Transform is the identity).  Semantically it is a run of
 * Triangle primitives (src/core/shape.h:50-81) appended to the primitive list after all analytic
 * primitives, in face order; vertex data as Mesh exposes it (src/core/mesh.h:12-14):
 * positions/normals are n_vertices*3 floats, indices n_triangles*3 uint32. normals must not be NULL. */
typedef struct PrtMesh {
    const float* positions;
    const float* normals;
    const uint32_t* indices;
    uint32_t n_vertices;
    uint32_t n_triangles;
    uint32_t material_id;
} PrtMesh;

/* One placed copy of a mesh.  Semantically a run of Triangle primitives that share one Transform:
 * struct Primitive {Shape = Triangle, Material, Transform{Mat, Inv}} (src/core/primitive.h:7-12), intersected exactly as
 * PrimitiveList::Intersect does it (src/core/primitive.cpp:29-43): local origin = Inv * o, local direction =
 * normalize(transpose(mat3(Mat)) * d), Triangle::Intersect in the mesh's own space, position back through Mat, normal
 * through Inv, distance measured in world space.  The transform must be rotation + uniform scale + translation
 * (prt_set_scene rejects anything else): only then is the reference's direction transform a ray transform, so that
 * an acceleration structure in the mesh's space returns what the reference's linear scan returns.
 * Bounds of that check: the scale must exceed 1e-10 (s^2 > 1e-20) and inv * mat = I must hold to 1e-3 of the largest term of
 * each entry (absolute 1e-3 where the terms are below 1): (1e-5 of it in the translation column, never below 1e-3): a copy at scale 2^-10 placed 1e4 away passes, one at 2^-40 is
 * refused with PRT_ERR_INVALID.
 * Coordinate range: results do not depend on the tree, the builder, a tunable or a refit for any unit of length, as long as
 * squared distances stay finite, normal binary32 numbers (coordinates between about 2^-60 and 2^60); tested bit for bit against
 * the linear scan for scales 2^-40 .. 2^40 and offsets up to 1e5 (tests/test_gpu_scale.py).  The
 * reference's own absolute length remains: a hit needs a ray parameter t >= 1e-3.
 * `mesh` indexes PrtSceneDesc.instanced_meshes (their own material_id is ignored). */
typedef struct PrtInstance {
    uint32_t mesh;
    uint32_t material_id;
    float mat[16];
    float inv[16];
} PrtInstance;

/* Primitive order (= tie-break order of the closest hit): analytic primitives, then the triangles of `meshes` in mesh
 * and face order, then the triangles of `instances` in instance and face order. */
typedef struct PrtSceneDesc {
    const PrtMaterial* materials;
    const PrtPrimitive* primitives;
    const PrtMesh* meshes;
    uint32_t n_materials;
    uint32_t n_primitives;
    uint32_t n_meshes;
    float sky[3]; /* reference literal (0.4,0.3,0.6): src/backend/cpu/renderer.h:31 */
    const PrtMesh* instanced_meshes; /* meshes that only exist through `instances` (may be NULL) */
    const PrtInstance* instances;
    uint32_t n_instanced_meshes;
    uint32_t n_instances;
} PrtSceneDesc;

/* Pinhole camera; right/up are derived exactly as Camera::Camera does (src/core/camera.h:10-16);
 * vertical FoV is 1 rad (src/core/camera.h:111) unless PrtLens below sets another. */
typedef struct PrtCameraDesc {
    float position[3];
    float front[3];
    float width;
    float height;
} PrtCameraDesc;

/* Optional sampling upgrades; all zero = the reference CPU backend's behaviour.
 *  jitter   1: the primary ray goes through (x + u1, y + u2), u1/u2 = the path's first two RNG draws (reference OptiX
 *           backend, src/backend/optix/device_programs.cu:172-173); 0: pixel centres (src/backend/cpu/renderer.cpp:45).
 *  rr_depth > 0: Russian roulette (reference roadmap, wavefront.md:98-100): a scatter that would start segment index
 *           >= rr_depth survives with p = clamp(max component of the new throughput, 0.05, 1), one RNG draw after the
 *           material's own; survivors carry throughput / p.
 *  clamp    > 0: every component of the radiance a path delivers is limited to it (wavefront.md:102-104). */
typedef struct PrtSampling {
    uint32_t jitter;
    uint32_t rr_depth;
    float clamp;
} PrtSampling;

/* Thin lens and field of view (prt_set_lens; NULL = all zero = the pinhole above with its 1 rad, bit for bit).  A property
 * of the context like PrtSampling: kept across prt_set_camera, prt_set_scene and prt_set_film, host-only contexts too
 * (they only record it).  PrtCameraDesc is not touched.
 *  fov_y          vertical field of view in radians, 0 < fov_y < pi; 0 = the reference's 1 rad
 *  aperture       lens RADIUS in world units, >= 0; 0 = pinhole
 *  focus_distance distance along `front` of the plane in focus (the plane perpendicular to `front`, not a sphere round
 *                 the camera); > 0 required while aperture > 0, ignored otherwise
 * Arithmetic (fp32, no contraction, in this order):
 *    tan_fov_y = tanf(0.5f * fov_y), or tanf(0.5f) when fov_y == 0
 *    ndcX = (px / W) * 2 - 1, ndcY = 1 - (py / H) * 2, aspect = W / H      (Camera::GetCameraRay, as before)
 *    pcx = ndcX * aspect * tan_fov_y, pcy = ndcY * tan_fov_y
 *  aperture == 0: the pinhole ray, d = normalize3(dc.x right + dc.y up + dc.z (-front)) with dc = normalize3((pcx, pcy,
 *    -1)), o = pos; no RNG draw.
 *  aperture > 0:
 *    u3 = rnd01(rng); u4 = rnd01(rng)      after the two jitter draws when jitter is on, else the path's first two draws
 *    r = aperture * sqrtf(u3), phi = 6.2831855f * u4, lx = r * cosf(phi), ly = r * sinf(phi)
 *    dc = normalize3((pcx * focus - lx, pcy * focus - ly, -focus))
 *    d = normalize3(dc.x * right + dc.y * up + dc.z * (-front))
 *    o = pos + lx * right + ly * up        ((pos + lx * right) + ly * up, component-wise)
 *    Without jitter (px, py) is the pixel centre.  The rest of the path is draw for draw what it is without a lens, from
 *    the advanced state.
 * Routes: with aperture > 0 every batch generates one full ray record per sample (what jitter does); compact primary rays,
 * the one-walk-per-pixel list and the one-launch path instance are not taken.  With aperture == 0 a fov_y only changes
 * tan_fov_y and every route stays available.  Results never depend on a tunable. */
typedef struct PrtLens {
    float fov_y;
    float aperture;
    float focus_distance;
} PrtLens;

/* Next-event estimation toward analytic emitters (DESIGN.md §3 "Light sampling"); NULL / mode OFF = the reference's
 * estimator, where direct light is found only by a scattered ray that hits an emitter.
 *  Light set: analytic primitives with an Emissive material, positive mean emission and a rotation + uniform scale +
 *    translation transform (with inv = inverse(mat)).  Quads are sampled uniformly by area (both faces emit); spheres
 *    uniformly in the cone they subtend from the shading point (not at all from inside or within PRT_LIGHT_SPHERE_MARGIN
 *    of their surface: pdf 0).  A light is picked with pmf proportional to emitting area x mean(rgb): quads 2 w h s^2,
 *    spheres 4 pi r^2 s^2.  Emissive mesh triangles, placed copies and analytic emitters with any other transform are
 *    never sampled by default (prt_set_light_sources adds the triangles: "Triangle lights" below); their emission counts
 *    on scattered hits at weight 1 (PrtLightStats.n_emitters_unsampled).
 *  Where: one light sample at every Lambertian vertex that scatters (segment index k with k + 1 < max_depth); never at
 *    metal, dielectric or emissive vertices.  It adds thr * (albedo / pi) * Le * max(0, n.w) * w_L / (pmf * pdf_w) if the
 *    shadow ray (x, w) with tmax = t_light * (1 - PRT_LIGHT_SHADOW_EPS) is not occluded (prt_occluded's semantics), with
 *    the throughput before that vertex's roulette, and clamped on its own (PrtSampling.clamp).
 *  Weights: NEE_MIS: power heuristic, w_L = pL^2 / (pL^2 + pB^2), pL = pmf * pdf_w, pB = max(0, n.w) / pi; a scattered
 *    segment from a Lambertian vertex that hits a light-set emitter counts its emission at w_B = 1 - w_L for that pair
 *    of vertices.  NEE: w_L = 1, w_B = 0 except w_B = 1 where pL = 0.  Emission seen from the camera or after a metal /
 *    dielectric vertex keeps weight 1; the constant sky is never sampled (an environment image is: "Environment light").
 *  RNG: the light sample draws from pcg_hash(state at the vertex + a constant of its own) and never advances the path's
 *    own state, so the scattered path, its segments and rays_per_depth are draw for draw those of lighting OFF. */
enum { PRT_LIGHTING_OFF = 0, PRT_LIGHTING_NEE_MIS = 1, PRT_LIGHTING_NEE = 2 };
/* relative: a blocker within the last 1e-3 of the shadow segment is missed (bias).  Not smaller: the reference's fp32 sphere
 * test (Circle::Intersect's b^2 - 4ac) places a grazing hit up to ~3e-4 of t early, so a tighter bound lets a sphere light
 * block its own samples near the rim of its cone. */
#define PRT_LIGHT_SHADOW_EPS 1e-3f
#define PRT_LIGHT_SPHERE_MARGIN 1e-3f  /* relative: no sphere sample from within (1 + margin) R of its centre */
typedef struct PrtLighting {
    uint32_t mode;
} PrtLighting;
/* Shadow rays cast / found occluded by the render calls since the last prt_reset_stats; the current scene's light set. */
typedef struct PrtLightStats {
    uint64_t shadow_rays;
    uint64_t shadow_occluded;
    uint32_t n_lights;
    uint32_t n_emitters_unsampled; /* emissive primitives outside the light set (mesh / placed triangles, other transforms) */
} PrtLightStats;
/* Triangle lights (prt_set_light_sources; default PRT_LIGHT_SOURCES_ANALYTIC = everything above, unchanged).  With
 * ANALYTIC | MESH the candidates are the analytic lights above (primitive order) followed by every triangle of an
 * Emissive world-space mesh (mesh and face order) and of an Emissive placed copy (instance and face order): global
 * primitive order.
 *  Triangle: world vertices v0, v1, v2 as fp32 (placed copies: Mat * v evaluated in double, rounded once), e1 = v1 - v0,
 *    e2 = v2 - v0, area A = |e1 x e2| / 2, geometric normal n_g = (e1 x e2) / |e1 x e2|, both in double, stored as fp32.
 *    Emission Le = the material's rgb; both faces emit (as quads do).  Power 2 A mean(rgb); zero or non-finite power: not
 *    a light and not counted as unsampled.
 *  Point: with the stream's u1, u2: s = sqrt(u1), p = v0 + (s (1 - u2)) e1 + (s u2) e2; w = (p - x) / |p - x|,
 *    t_light = |p - x|, tmax = t_light (1 - PRT_LIGHT_SHADOW_EPS).
 *  pdf: pdf_w = d2 / (A |n_g . w|), the quad's formula; 0 where the denominator is 0.  For the light sample
 *    d2 = |p - x|^2; for a scattered segment that hits the triangle, d2 of the hit.
 *  Selection (all candidates, analytic ones too, while the MESH bit is set): P_i the powers in candidate order, C_i their
 *    running sum in double, T_i = floor(C_i / C_n * 2^32 + 0.5) as a 64-bit integer (T_0 = 0, T_n = 2^32),
 *    r0 = pcg_hash(pcg_hash(key + the light stream's constant)): the 32-bit state after the stream's first step, whose
 *    top 24 bits are u0 of the default rule.  The light is the smallest i with r0 < T_i, and its pmf is
 *    (T_i - T_{i-1}) / 2^32: the number the estimator, the MIS weights and prt_light_info use, equal to the selection
 *    probability exactly for any number of lights (the kernels hold it rounded to fp32).  A candidate with an empty
 *    interval is never picked and is NOT in the light set: n_lights, prt_light_info, the `light` output of
 *    prt_sample_light and the MIS weights see the candidates with T_i > T_{i-1}, in global primitive order.  u1, u2 are
 *    the stream's second and third draws, as above.
 *  Weights, estimator, where samples are taken, clamp, roulette, RNG stream: as above.  A scattered segment from a
 *    Lambertian vertex that hits a light-set triangle is weighted w_B = 1 - w_L for that pair; a triangle outside the
 *    set, or with pmf 0, keeps weight 1.
 *  n_emitters_unsampled then counts analytic emitters with a non-similarity transform plus candidates with positive
 *    power and an empty interval. */
enum { PRT_LIGHT_SOURCES_ANALYTIC = 1, PRT_LIGHT_SOURCES_MESH = 2 }; /* bit mask */
/* Clustered light selection (prt_set_light_selection; default PRT_LIGHT_SELECTION_POWER = everything above, unchanged).
 * A property of the context like the lighting mode and the source mask: set before or after prt_set_scene, kept across it,
 * copied by prt_clone_scene, host-only contexts too.  It takes effect only while PRT_LIGHT_SOURCES_MESH is set (only then
 * does the integer rule select lights); with the default mask it is recorded and inactive (PrtLightClusterInfo.active).
 * With it a light is picked in two steps: one of at most PRT_LIGHT_MAX_CLUSTERS spatial clusters by power / distance^2 to
 * the cluster's box from the vertex, then a light inside the cluster by integer thresholds.  No hierarchy, no orientation
 * term.  The light set, the point on the light, pdf_w, the MIS weights, the shadow rays, the RNG stream and the
 * environment-or-lights draw (which runs first) are those of "Triangle lights" / "Environment light".
 *  Clusters (host, double, built with every scene whatever the context's settings, and again by prt_refit_meshes /
 *    prt_set_instance_transforms with the candidate table: equal to a fresh prt_set_scene of the moved geometry):
 *    Members: the light set (candidates with a non-empty global interval); every member lies in exactly one cluster; at
 *      most max_clusters clusters, none empty.
 *    A light's world box: triangle: min / max of its fp32 world vertices; quad: the corners c +- u/2 +- v/2 from the
 *      record in double, rounded outward; sphere: c +- R, rounded outward.  A cluster's box lo, hi (fp32): the union.
 *    r2: the squared half diagonal of the box in double, rounded up to fp32, never below 1e-30f.
 *    W_c: the sum of the members' global widths T_i - T_{i-1} (64-bit; the W_c sum to 2^32); phi_c = fl32(W_c / 2^32).
 *    Inside a cluster the members are in candidate order, P_i their powers (the candidate table's doubles), S_j the
 *      running sums: U_{c,j} = floor(S_j / S_n * 2^32 + 0.5), U_{c,0} = 0, U_{c,n} = 2^32; pmf_in = (U_j - U_{j-1}) / 2^32,
 *      held by the kernels rounded once to fp32 (under an environment multiplied by (2^32 - T_e) / 2^32 in double before
 *      that one rounding, as the global pmf is).  A member with an empty inner interval is never picked under clustered
 *      selection, has pmf 0, keeps weight 1 when a scattered segment hits it and counts in n_emitters_unsampled while the
 *      selection is active.  Light indices (prt_light_info, prt_sample_light's `light`) stay the global light set's;
 *      prt_light_info's pmf stays the global one.
 *    Grouping (deterministic): start with one cluster; split the cluster with the largest W_c r2_c that can be split until
 *      max_clusters is reached or none can.  A split orders the members by box centre along an axis (ties: candidate
 *      order) and cuts the order in two.  Where a plane perpendicular to an axis separates the members' boxes (no box
 *      straddles it) the cut is the separating plane whose halves are nearest in power, on the first axis that has one in
 *      descending order of the extent of the centres; otherwise the cut is the power median along the longest axis.  A
 *      cluster whose members' centres coincide is not split.  So two emissive meshes with disjoint boxes, alone in a
 *      scene, end in different clusters when max_clusters >= 2.
 *  Cluster choice at a vertex x (fp32, every operation rounded once in this order, no contraction; comparisons as
 *    selects, so that a NaN falls through), K clusters:
 *      for c = 0 .. K-1, per axis k: t = lo_k - x_k; u = x_k - hi_k; d_k = t > u ? t : u; d_k = d_k > 0 ? d_k : 0
 *        D2 = (d_x d_x + d_y d_y) + d_z d_z; den = D2 > r2_c ? D2 : r2_c; w_c = phi_c / den; cum_c = cum_{c-1} + w_c (cum_{-1} = 0)
 *      total = cum_{K-1}; if !(total > 0 && total < inf): w_c = phi_c for every c, cum and total again
 *      inv = 1.0f / total
 *      q_c = (cum_c inv) 16777216.0f; M_c = q_c < 16777216.0f ? (uint32) q_c : 2^24 for c < K-1 (q_c >= 0, so the
 *        conversion is the floor; a NaN gives 2^24); M_{K-1} = 2^24; M_{-1} = 0
 *      m = r0 >> 8 (r0: the state after the light stream's first step: u0's 24-bit integer)
 *      cluster = the smallest c with m < M_c; P_c = (M_c - M_{c-1}) 2^-24 (exact in fp32; 0 where M_c <= M_{c-1})
 *    Member: the smallest j with r3 < U_{c,j}, r3 the 32-bit state after the stream's FOURTH step; u1, u2 stay the second
 *    and third draws.  The light's pmf is fl(P_c pmf_in), pdf_light = pmf pdf_w as before.  P_c is both the probability
 *    that the cluster is drawn (m uniform on 24 bits) and the number divided by; pmf_in likewise for r3.  A cluster with
 *    M_c = M_{c-1} is never drawn from x: its lights have pmf 0 there.
 *  A scattered segment from a Lambertian vertex x (the segment's origin) that hits light i of cluster c is weighted with
 *    pL = fl(fl(P_c(x) pmf_in_i) pdf_w), P_c(x) from the same evaluation; pL = 0: weight 1. */
enum { PRT_LIGHT_SELECTION_POWER = 0, PRT_LIGHT_SELECTION_CLUSTERED = 1 };
#define PRT_LIGHT_MAX_CLUSTERS 64u
typedef struct PrtLightSelection {
    uint32_t mode;
    uint32_t max_clusters; /* 1..64; 0 = default 32 */
} PrtLightSelection;
typedef struct PrtLightClusterInfo {
    uint32_t mode;          /* the recorded PRT_LIGHT_SELECTION_* */
    uint32_t active;        /* 1: CLUSTERED and PRT_LIGHT_SOURCES_MESH is set */
    uint32_t n_clusters;    /* of the current scene (0: no scene or no light) */
    uint32_t max_clusters;  /* what the clusters were built for (the default resolved) */
    uint32_t n_empty_inner; /* members whose interval inside their cluster is empty */
} PrtLightClusterInfo;
/* Environment light (prt_set_environment; NULL = the constant `sky`, bit for bit the behaviour above).  A lat-long
 * image of radiance, piecewise constant (nearest texel), a property of the context like the lighting mode and the light
 * source mask: set before or after prt_set_scene, kept across it, copied by prt_clone_scene, host-only contexts too (they
 * only build the tables).  While it is set PrtSceneDesc.sky is ignored.
 *  Lookup of a unit direction d: phi = atan2f(d.z, d.x), u = phi / (2 pi) + 0.5, column j = min(W - 1, floor(u W));
 *    theta = acosf(clamp(d.y, -1, 1)), v = theta / pi, row i = min(H - 1, floor(v H)).  Every miss delivers
 *    thr * env[i][j] where it delivered thr * sky: camera rays, scattered rays, and the segments the producers end
 *    themselves because they cannot hit a triangle; the clamp applies as before.
 *  Distribution (host, double): texel weight w_ij = mean(rgb_ij) Omega_i, Omega_i = (2 pi / W) (cos(pi i / H) -
 *    cos(pi (i + 1) / H)).  Row thresholds R_i = floor(sum_{k <= i} sum_j w_kj / total * 2^32 + 0.5) as 64-bit integers
 *    (R_H = 2^32); per row, column thresholds C_ij the same way from w_ij over the row's sum.  Texel pmf
 *    p_ij = (R_i - R_{i-1}) (C_ij - C_{i,j-1}) / 2^64 exactly.  A texel or row with an empty interval is never sampled
 *    (pmf 0); an all-black map has no distribution.
 *  Selection: T_e = floor(light_share 2^32 + 0.5); T_e = 2^32 if the current light set is empty; T_e = 0 if the map has
 *    no distribution or light_share is 0.  r_e = pcg_hash(key + PRT_ENV_RNG) (key: the path's state at the vertex): the
 *    environment is sampled iff r_e < T_e, otherwise the selection above runs unchanged (default and threshold rule).
 *    Every other light's pmf is multiplied by (2^32 - T_e) / 2^32 in double and rounded once to fp32: the number the
 *    estimator, the MIS weights and prt_light_info use.  prt_light_intervals reports the exact product: while T_e > 0,
 *    width[l] = (T_l - T_{l-1}) (2^32 - T_e) and pmf = width / 2^64; with T_e = 0 the factor is exactly 1 and nothing
 *    changes (width in units of 2^-32).
 *  Sample (the light stream, pcg_hash(key + its constant), stepped by pcg_hash): row = smallest i with s1 < R_i, column =
 *    smallest j with s2 < C_ij (s1, s2: the 32-bit states after the first and second step), u1, u2 = the top 24 bits of the
 *    states after the third and fourth step.  u = (j + u1) / W, v = (i + u2) / H, phi = 2 pi u - pi, theta = pi v,
 *    w = (sin theta cos phi, cos theta, sin theta sin phi).  Le = env[i][j] (no second lookup), pdf_w = p_ij W H /
 *    (2 pi^2 sin theta) (0 where sin theta = 0), pL = (T_e / 2^32) pdf_w, shadow ray (x, w) with tmax = +inf.  Where
 *    samples are taken, estimator, clamp, throughput before roulette, power heuristic: as for the other lights.
 *  Miss after a Lambertian vertex: weighted w_B = 1 / (1 + (pL / pB)^2), pL at the texel the lookup of d gives with
 *    sin theta = sqrt(max(0, 1 - d.y^2)) (evaluated as (1 - d.y)(1 + d.y)); NEE: 0 where pL > 0, else 1.  Misses seen from the camera or after a metal /
 *    dielectric vertex keep weight 1.  Lighting OFF, or T_e = 0: the environment is just the radiance of a miss.
 *  Results do not depend on a tunable: with an environment set every batch takes the unfused pipeline. */
#define PRT_ENV_RNG 0x3C6EF372u          /* the environment-or-lights draw: pcg_hash(path state at the vertex + this) */
#define PRT_LIGHT_ENVIRONMENT 0xFFFFFFFEu /* prt_sample_light's `light` for an environment sample */
#define PRT_ENV_MAX_WIDTH 16384u
#define PRT_ENV_MAX_HEIGHT 8192u
typedef struct PrtEnvironment {
    const float* rgb;      /* height*width*3 floats, row 0 = +Y pole (top), copied */
    uint32_t width, height;
    float light_share;     /* probability that a light sample goes to the environment, [0,1]; 0: never sampled */
} PrtEnvironment;
typedef struct PrtEnvironmentInfo {
    uint32_t is_set;       /* 0: the constant sky (everything else is 0 then) */
    uint32_t width, height;
    uint32_t n_sampled;    /* texels with a non-empty interval (0: no distribution) */
    uint64_t t_env;        /* T_e for the current scene and light source mask */
    float light_share;
} PrtEnvironmentInfo;

/* Image textures (prt_set_textures; NULL = none, bit for bit the behaviour above).  A texture replaces the constant rgb of
 * a Lambertian or Metal material as ALBEDO: the attenuation of Lambertian / Metal::Scatter (and so the throughput, the
 * roulette and everything after it) and the albedo / pi of the light sample in every lighting mode.  Emission and the
 * dielectric's attenuation are never textured.  Scatter directions, RNG draws, segments, rays_per_depth, MIS weights and
 * hit records do not depend on the albedo: with roulette off they are draw for draw those of the untextured scene.
 * prt_scatter and prt_sample_light keep the material's constant rgb: their inputs carry no UV.
 *  UV of a hit (fp32, no contraction, in this order):
 *    triangle of a world-space mesh or of a placed copy: b1, b2 as Triangle::Intersect computes them for the winning triangle
 *      (a copy: in the mesh's space, from the local ray); w0 = 1.0f - b1 - b2; u = (w0 * u0 + b1 * u1) + b2 * u2, v likewise;
 *      u0, u1, u2: the UVs of the face's three vertices in index order.  The placed copies of a mesh share its UVs.
 *    quad: p = the local hit point of Quad::Intersect (before Mat); u = p.x / w + 0.5f, v = p.z / h + 0.5f.
 *    A sphere cannot carry a textured material (no parametrisation: PRT_ERR_INVALID).
 *  Lookup of (u, v) in a W x H texture; v = 0 is the BOTTOM row:
 *    wrap: REPEAT a = u - floorf(u); CLAMP a = fminf(fmaxf(u, 0.0f), 1.0f); b from v the same way
 *    X = a * W, Y = (1.0f - b) * H
 *    NEAREST: j = min(W - 1, (uint32)floorf(X)), i = min(H - 1, (uint32)floorf(Y)), rgb = texel[i][j]
 *    BILINEAR: x = X - 0.5f, x0 = floorf(x), fx = x - x0; y0, fy from Y - 0.5f the same way; columns (int)x0 and (int)x0 + 1,
 *      rows likewise; an index k of an axis of size N becomes ((k % N) + N) % N under REPEAT and min(max(k, 0), N - 1) under
 *      CLAMP; per channel c = (c00 * (1.0f - fx) + c01 * fx) * (1.0f - fy) + (c10 * (1.0f - fx) + c11 * fx) * fy (first
 *      index: the row).
 *  The binding belongs to the current scene: prt_set_textures needs one, prt_set_scene drops the binding, prt_clone_scene
 *  copies it, prt_refit_meshes and prt_set_instance_transforms keep it (the UV table is stored per mesh triangle in face order,
 *  outside every tree).  Host-only contexts validate the set and build the tables.
 *  Routes: while a binding textures at least one material every batch takes the unfused full-record pipeline (no fused
 *  segment, no compact primary rays, no one-walk-per-pixel list, no path instance): the rule of the environment image.
 *  Results never depend on a tunable, on batching or on the partition. */
enum { PRT_TEX_NEAREST = 0, PRT_TEX_BILINEAR = 1 };
enum { PRT_TEX_REPEAT = 0, PRT_TEX_CLAMP = 1 };
#define PRT_TEXTURE_NONE 0xFFFFFFFFu
#define PRT_TEX_MAX_SIZE 16384u
typedef struct PrtTexture {
    const float* rgb;      /* height*width*3 floats, row 0 = top, copied */
    uint32_t width, height, filter, wrap;
} PrtTexture;
typedef struct PrtTextureSet {
    const PrtTexture* textures;
    uint32_t n_textures;
    const uint32_t* material_texture;       /* texture index or PRT_TEXTURE_NONE per material */
    uint32_t n_materials;
    const float* const* mesh_uvs;           /* per PrtSceneDesc.meshes[i]: n_vertices*2 floats, or NULL */
    uint32_t n_meshes;
    const float* const* instanced_mesh_uvs; /* per instanced_meshes[i], shared by its placed copies; or NULL */
    uint32_t n_instanced_meshes;
} PrtTextureSet;
typedef struct PrtTextureInfo {
    uint32_t is_set;               /* 0: no binding (everything else is 0 then) */
    uint32_t n_textures;
    uint32_t n_textured_materials; /* 0: the binding changes no route and no result */
    uint32_t n_uv_triangles;       /* triangles of the face-order UV table (24 bytes each) */
    uint64_t n_texels;             /* texels of the pool (16 bytes each) */
    uint64_t device_bytes;         /* what the binding occupies on the device (0 on a host-only context) */
} PrtTextureInfo;

/* Closest-hit record of one ray (what Scene::Intersect returns, src/core/surface_interaction.h:6-13,
 * plus the winning primitive index and the world distance^2 the reference minimises,
 * src/core/primitive.cpp:42-48).  prim < 0: miss. */
typedef struct PrtHit {
    int32_t prim;
    uint32_t front_face;
    uint32_t material_id;
    float d2;
    float position[3];
    float normal[3];
} PrtHit;

/* Counters and timings of the render calls since the last prt_reset_stats. */
#define PRT_MAX_DEPTH 64
typedef struct PrtStats {
    uint64_t rays_total;               /* ray segments for which a closest-hit query ran */
    uint64_t rays_per_depth[PRT_MAX_DEPTH];
    uint64_t samples;                  /* ProgressiveRender-equivalents done */
    uint64_t intersect_launches;       /* launches of the dominant (closest-hit) kernel */
    double intersect_ms;               /* summed HIP-event time of those launches (timing enabled) */
    double shade_ms;
    double raygen_ms;
    double accumulate_ms;
    uint64_t bvh_node_visits;          /* only from prt_measure_traversal */
    uint64_t bvh_tri_tests;
    uint64_t prim_tests;
    uint64_t node_lane_slots;          /* 64 x node-loop iterations of all waves: visits / slots = lane efficiency */
    double scan_ms;                    /* analytic-primitive scan kernel (function-level entry points only) */
    uint64_t rays_traversed;           /* prt_measure_traversal: rays that entered the BVH root box (walked the tree) */
    uint64_t tri_lane_slots;           /* 64 x triangle-loop iterations of all waves: tri tests / slots = lane efficiency */
    uint64_t max_stack_used;           /* deepest traversal stack any ray reached (prt_measure_traversal) */
    /* prt_measure_traversal, 8-wide kernel: shader cycles (s_memtime) summed over all waves, by section of the wave's
     * outer loop: finish + refill (+ level switches), node loop, triangle phase */
    uint64_t wave_cycles_refill;
    uint64_t wave_cycles_node;
    uint64_t wave_cycles_tri;
} PrtStats;

typedef struct PrtBvhInfo {
    uint32_t n_nodes;
    uint32_t n_triangles;
    uint32_t max_depth;
    uint32_t max_leaf_size;
    float sah_cost;
    float pad_abs;     /* absolute AABB padding applied (conservative culling) */
    uint64_t node_bytes;   /* bytes of the 4-wide tree the default kernel walks */
    uint64_t tri_bytes;
    uint32_t n_nodes4;     /* 4-wide nodes (128 B each) */
    uint32_t max_stack4;   /* worst-case traversal stack entries of the 4-wide tree */
    uint32_t n_nodes8;     /* compressed 8-wide nodes (80 B each) the default kernel walks; 0 = not available */
    uint32_t depth8;       /* levels of the 8-wide tree (the traversal stacks at most depth8 - 1 node groups) */
    float build_ms;        /* wall time of the BVH construction (device-side build: without the vertex upload) */
    uint32_t built_on_device; /* 1: built by the device-side builder (prt_set_param("gpu_build", 1)) */
    float refit_ms;        /* device time of the last prt_refit_meshes (records + boxes bottom-up + re-quantization), 0 = never */
    uint32_t refits;       /* prt_refit_meshes calls since prt_set_scene */
} PrtBvhInfo;

/* Static wavefront occupancy of the traversal kernel (the dominant kernel) for the current scene. */
typedef struct PrtOccupancy {
    uint32_t blocks_per_cu;        /* resident 256-thread blocks per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor) */
    uint32_t waves_per_cu;         /* = 4 x blocks_per_cu */
    uint32_t max_waves_per_cu;     /* hardware limit (32 on gfx950) */
    uint32_t vgprs;                /* per lane */
    uint32_t lds_bytes_per_block;
    uint32_t compute_units;
    uint32_t resident_grid_blocks; /* blocks of the persistent grid the library launches */
} PrtOccupancy;

typedef struct PrtContext PrtContext;

/* ---- lifetime ---------------------------------------------------------------------------------- */
/* device_id < 0: host-only context (scene/mesh/BVH utilities work, compute calls fail loudly).
 * Side effect of every call that touches the device: it makes the context's GPU the CALLING THREAD's current HIP device
 * (hipSetDevice) and leaves it so; a host that holds several devices (a torch process, say) restores its own afterwards
 * or calls from a thread of its own, as prt_group_* does. */
int prt_create(int device_id, PrtContext** out);
void prt_destroy(PrtContext* ctx);
const char* prt_last_error(const PrtContext* ctx);
int prt_version(void);
/* The process-wide books of what the contexts of this library own on the devices (either may be NULL): bytes of device memory
 * currently allocated, and allocation calls made so far.  live_bytes returns to its earlier value when a context is destroyed;
 * alloc_calls stands still across calls in the steady state (a second identical prt_render, a second query of the same size).
 * prt_group_*'s own exchange buffers and the device-side builder's temporaries are not counted. */
void prt_device_memory_info(uint64_t* live_bytes, uint64_t* alloc_calls);
/* Launch on this hipStream_t (e.g. torch's current stream); NULL = the context's own stream. */
int prt_set_stream(PrtContext* ctx, void* hip_stream);
/* The hipStream_t the context launches on / its device id (-1: host-only context). */
int prt_get_stream(PrtContext* ctx, void** hip_stream);
int prt_get_device(const PrtContext* ctx);

/* ---- Renderer::Init / SetCamera (src/core/renderer.h:13-15) ---------------------------------- */
/* Flattens + uploads the scene and builds the BVH over all mesh triangles.  Replaces
 * BuildWavefrontSceneBuffers (src/backend/cuda_wavefront/soa.cpp:37-114). */
int prt_set_scene(PrtContext* ctx, const PrtSceneDesc* scene);
/* Replicates the scene `src` holds (flattened primitives, trees, triangle records) onto dst's device without building
 * anything again: the scene is read-only and every GPU of a multi-GPU render needs its own copy. */
int prt_clone_scene(PrtContext* dst, const PrtContext* src);
/* Deforming geometry (SURVEY.md §8f-3 "refit"; the reference rebuilds its OptiX acceleration structures from scratch,
 * src/backend/optix/renderer.cpp:736-871): the scene's world-space meshes again, with NEW positions / normals and the SAME
 * vertex counts, triangle counts and index buffers as at prt_set_scene.  The compressed 8-wide tree keeps its topology; its
 * triangle records are rewritten and its boxes refitted bottom-up and re-quantized on the device.  Scenes with placed
 * copies (PrtInstance) are not refitted (PRT_ERR_INVALID): their copies move through prt_set_instance_transforms
 * below, which leaves every mesh tree alone.  After a refit the A/B kernels over the binary / 4-wide
 * trees are unavailable (those trees are dropped).  Results equal a fresh prt_set_scene of the new geometry bit for bit
 * (the closest hit does not depend on the tree); traversal gets slower as the deformation grows.
 * A tree of more than 16 levels (PrtBvhInfo.depth8 > 16; only the host builder makes those) is not refitted:
 * PRT_ERR_INVALID with a message that names the depth, before anything is written, the scene exactly what it was and
 * usable.  Without the 4-wide tree no kernel instance holds its deepest rays (the deepest stack, 15 entries, covers 16
 * levels); the caller rebuilds with prt_set_scene. */
int prt_refit_meshes(PrtContext* ctx, const PrtMesh* meshes, uint32_t n_meshes);
/* Refit from device arrays: prt_refit_meshes for vertex arrays that are on the context's device already (the output of a
 * skinning, cloth or simulation step there).  meshes[m] is world-space mesh m of the current scene: the vertex counts and
 * the index buffers are those of prt_set_scene, which the scene kept; nothing is read from the host.  The scenes it takes,
 * the scene it leaves and the rendered results are those of prt_refit_meshes with the same arrays on the host, bit for
 * bit; so are the refusals (placed copies, no 8-wide tree, depth8 > 16, a wrong n_meshes), each with the scene intact.
 *   Stream order: the arrays are read in stream order on the context's stream (prt_set_stream): a producer enqueued on
 *   that stream needs no synchronisation before the call.  The call is synchronous on return.
 *   Validation: a first device pass finds the largest |coordinate| of the referenced vertices (prt_refit_meshes' rule,
 *   so the culling pad is the same) and any non-finite position or supplied normal; its few bytes are read before anything
 *   of the scene is written.  A non-finite value is PRT_ERR_INVALID with the scene exactly what it was and usable.
 *   normals == NULL: the mesh gets area-weighted vertex normals computed on the device by the rule of prt_mesh_create
 *   without normals, bit for bit: per face e1 = b - a, e2 = c - a and e1 x e2 in double without contraction; per vertex the
 *   double sum over its incident corners in ascending face order (a face's repeated vertex once per corner);
 *   n = (float)(sum / |sum|), and (0, 1, 0) where |sum| is not > 0.  No floating-point atomics: the order is fixed.
 *   Host copies: the tree and the records are NOT read back by the call; prt_bvh_read8, prt_bvh_read, prt_clone_scene and
 *   prt_refit_meshes fetch them when they need them (PrtRefitInfo.host_copies_stale).  With the MESH bit of
 *   prt_set_light_sources in use or not, the candidate table follows as after prt_refit_meshes; only the emissive
 *   world-space triangles' vertices (36 bytes each) come back for it.
 *   What the scene keeps: index and incident-corner tables, the tree's level lists and the refit's working arrays go to the
 *   device at the first call after prt_set_scene / prt_clone_scene and stay until the scene goes (24 bytes per
 *   triangle, 16 per vertex, 220 per node, 40 per emissive triangle); from the second call on nothing is allocated and
 *   nothing is copied up.
 * Not offered: the group (prt_group_*); a device array lives on one device. */
typedef struct PrtMeshDeviceArrays {
    const float* positions;  /* DEVICE pointer, n_vertices*3 floats of world-space mesh m, as at prt_set_scene */
    const float* normals;    /* DEVICE pointer, n_vertices*3 floats, or NULL: computed on the device (above) */
} PrtMeshDeviceArrays;
int prt_refit_meshes_device(PrtContext* ctx, const PrtMeshDeviceArrays* meshes, uint32_t n_meshes);
/* vertex normals of world-space mesh `mesh` of the current scene for positions on the device, into a device array
 * (n_vertices*3 floats each; the rule above; stream order as above, synchronous on return; the scene is not touched) */
int prt_mesh_normals_device(PrtContext* ctx, uint32_t mesh, const float* positions, float* normals_out);
typedef struct PrtRefitInfo {
    uint32_t refits;            /* both forms, since prt_set_scene (= PrtBvhInfo.refits) */
    uint32_t last_form;         /* 0 none, 1 host arrays, 2 device arrays */
    uint32_t normals_computed;  /* meshes whose normals the last call computed on the device */
    uint32_t host_copies_stale; /* 1: the host copies of tree and records lag behind the device (refreshed on demand) */
    float device_ms, wall_ms;   /* of the last call */
    uint64_t h2d_bytes, d2h_bytes; /* what the last call moved over the bus, every copy it issued counted */
} PrtRefitInfo;
/* Works on a host-only context and before the first refit (zeros). */
int prt_refit_info(PrtContext* ctx, PrtRefitInfo* out);
/* Moving placed copies (rigid-body animation for the price of the top level; the reference's OptiX backend rebuilds its
 * instance level only when transforms change, src/backend/optix/renderer.cpp:703-871): instances[i] replaces mat / inv of
 * placed copy i of the current scene.  PRT_ERR_INVALID, with the scene exactly what it was and usable: n is not the
 * scene's n_instances, a copy's mesh or material_id is not what prt_set_scene got, the scene has no placed copies, a
 * transform fails prt_set_scene's test (rotation + uniform scale + translation, inv = inverse(mat)), or the new
 * two-level tree would be too deep for the traversal stack.  Everything is checked before anything is written.
 *   PRT_INSTANCES_REFIT    the top-level tree keeps its topology: a device pass recomputes every copy's transform
 *                          record and world box, the top-level boxes are recomputed bottom-up and re-quantized in
 *                          place.  A box that does not fit its node's grid makes the call fall back to the rebuild.
 *   PRT_INSTANCES_REBUILD  a new top-level tree over the new boxes from the builder the scene was built with goes in
 *                          front of the mesh trees; if its node count differs, a device pass rebases the mesh trees'
 *                          child_base and the instances' root.
 * Neither mode rebuilds, re-uploads or refits a mesh tree or a triangle record; primitive order and hit ids stay.
 * The scene-wide bounds, the host copies (prt_bvh_read8, prt_clone_scene) and the triangle lights of placed copies
 * follow (the light table is uploaded again while the MESH bit is set).  The call waits for the context's stream; film,
 * camera, sampling, lighting mode, tunables and statistics are not touched.  A host-only context performs the host
 * rebuild whatever the mode.  Results equal a fresh prt_set_scene of the moved description bit for bit.  A HIP
 * failure midway leaves the context without a scene. */
enum { PRT_INSTANCES_REFIT = 0, PRT_INSTANCES_REBUILD = 1 };
int prt_set_instance_transforms(PrtContext* ctx, const PrtInstance* instances, uint32_t n, uint32_t mode);
typedef struct PrtInstanceUpdateInfo {
    uint32_t updates;   /* successful prt_set_instance_transforms calls since the scene was set */
    uint32_t last_mode; /* what the last one actually ran (a refit that did not fit reports PRT_INSTANCES_REBUILD) */
    uint32_t top_nodes; /* nodes of the top-level tree now: the first top_nodes nodes of prt_bvh_read8 */
    uint32_t top_depth; /* its levels */
    float last_ms;      /* host wall time of the last call, its wait for the device included */
} PrtInstanceUpdateInfo;
int prt_instance_update_info(PrtContext* ctx, PrtInstanceUpdateInfo* out);
/* The instance level of a scene with placed copies, next to prt_bvh_read8: *n_instances = the instances of the top-level
 * tree (the identity instance of the world-space meshes first, if the scene has any, then the placed copies in input
 * order) = its leaf slots.  For k < min(capacity, *n_instances), each array that is not null: slot_instance[k] = the
 * instance in top-level leaf slot k; root[k] = the root node of instance k's mesh tree in prt_bvh_read8; slot_base[k] =
 * the first triangle record of its mesh in prt_bvh_read; prim_base[k] = the global primitive index of its first
 * triangle (0 for the world-space meshes, whose records carry their own). */
int prt_instances_read(PrtContext* ctx, uint32_t capacity, uint32_t* n_instances, uint32_t* slot_instance, uint32_t* root,
                       uint32_t* slot_base, uint32_t* prim_base);
int prt_set_camera(PrtContext* ctx, const PrtCameraDesc* cam);
/* Film::Resize + Clear (src/core/film.cu:11-35) and the image partition of this context:
 * 8x8-pixel tiles, tile t (row-major) belongs to rank t % world_size. */
int prt_set_film(PrtContext* ctx, uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size);
int prt_film_clear(PrtContext* ctx);

/* ---- Renderer::ProgressiveRender (src/core/renderer.h:14) ------------------------------------- */
/* Adds `spp` samples per pixel (sample indices first_sample .. first_sample+spp-1) to the film.
 * spp = 1 is exactly one ProgressiveRender.  max_depth = max ray segments per path
 * (reference m_Depth = 20, src/backend/cpu/renderer.h:34).  Result is independent of batching and
 * of world_size because the RNG is keyed by (global pixel, sample, seed). Synchronous on return. */
int prt_render(PrtContext* ctx, uint32_t spp, uint32_t max_depth, uint32_t seed, uint32_t first_sample);
/* Same, but only enqueues on the stream (no host sync). */
int prt_render_async(PrtContext* ctx, uint32_t spp, uint32_t max_depth, uint32_t seed, uint32_t first_sample);
int prt_synchronize(PrtContext* ctx);
/* Sampling upgrades for the following prt_render calls (NULL = all off). */
int prt_set_sampling(PrtContext* ctx, const PrtSampling* sampling);
/* The lens for the following prt_render calls ("Thin lens and field of view" above; NULL = all zero).  PRT_ERR_INVALID,
 * with the previous lens intact: a NaN in any field, fov_y < 0 or >= pi, aperture < 0 or not finite, aperture > 0 with a
 * focus_distance that is not finite or <= 0. */
int prt_set_lens(PrtContext* ctx, const PrtLens* lens);
int prt_get_lens(PrtContext* ctx, PrtLens* out);
/* Samples kept in flight together (paths = local pixels * n); default 1. */
int prt_set_samples_in_flight(PrtContext* ctx, uint32_t n);
/* Light sampling for the following prt_render calls (PrtLighting above; NULL = off).  A mode other than PRT_LIGHTING_*
 * returns PRT_ERR_INVALID.  Works on host-only contexts too (it only records the mode). */
int prt_set_lighting(PrtContext* ctx, const PrtLighting* l);
int prt_get_light_stats(PrtContext* ctx, PrtLightStats* out);
/* Which emitters the light set holds ("Triangle lights" above): PRT_LIGHT_SOURCES_ANALYTIC (default) or ANALYTIC | MESH;
 * 0, MESH alone or unknown bits: PRT_ERR_INVALID.  Before or after prt_set_scene, host-only contexts too; the mask stays
 * with the context across prt_set_scene, and prt_clone_scene copies the source's mask with its tables.  The table with
 * triangles in it is built on the host with every scene (80 bytes + one threshold per candidate) and uploaded only while
 * the MESH bit is set.  prt_refit_meshes with the MESH bit set rebuilds that table on the host from the new vertices
 * and uploads it again: O(candidates), about 90 bytes per candidate over the bus, not part of the reported refit time. */
int prt_set_light_sources(PrtContext* ctx, uint32_t mask);
/* How a light is picked ("Clustered light selection" above; NULL = power, 32 clusters).  An unknown mode or
 * max_clusters > PRT_LIGHT_MAX_CLUSTERS: PRT_ERR_INVALID, the previous selection intact.  A new max_clusters rebuilds the
 * current scene's clusters on the host (and uploads them while the MESH bit is set). */
int prt_set_light_selection(PrtContext* ctx, const PrtLightSelection* sel);
int prt_light_cluster_info(PrtContext* ctx, PrtLightClusterInfo* out);
/* The clusters of the current scene (host-only contexts too; they exist whatever the mode): n_clusters, and for the first
 * min(n_clusters, capacity): lo, hi (3 floats each), r2, phi, the power width W_c and the number of members.  Each output
 * may be NULL. */
int prt_light_clusters(PrtContext* ctx, uint32_t capacity, uint32_t* n_clusters, float* lo, float* hi, float* r2, float* phi,
                       uint64_t* power_width, uint32_t* n_members);
/* Per light of the global light set (prt_light_info's order), the first min(n_lights, capacity): its cluster and the width
 * U_j - U_{j-1} of its interval inside the cluster.  Host-only contexts too. */
int prt_light_cluster_members(PrtContext* ctx, uint32_t capacity, uint32_t* n_lights, uint32_t* cluster, uint64_t* inner_width);
/* The device's own M_c for n points (x: 3 floats each; M: n x n_clusters, point-major) through the code the render uses.
 * Needs a device, a scene with a light and the MESH bit (the tables are on the device only then); any selection mode. */
int prt_light_cluster_pmf(PrtContext* ctx, uint32_t n, const float* x, uint32_t* M);
/* The environment light ("Environment light" above).  PRT_ERR_INVALID, with the previous environment intact: width or
 * height 0, width > PRT_ENV_MAX_WIDTH, height > PRT_ENV_MAX_HEIGHT, a null image, a negative or non-finite texel,
 * light_share outside [0, 1] (NaN included).  Waits for the context's stream; the light tables are uploaded again when
 * T_e changed. */
int prt_set_environment(PrtContext* ctx, const PrtEnvironment* env);
int prt_environment_info(PrtContext* ctx, PrtEnvironmentInfo* out);
/* The exact interval widths: row_width[i] = R_i - R_{i-1} (H entries), col_width[i * W + j] = C_ij - C_{i,j-1} (H * W
 * entries; a row without weight has none).  Either may be NULL.  Host-only contexts too; no environment or no
 * distribution: PRT_ERR_INVALID. */
int prt_environment_intervals(PrtContext* ctx, uint64_t* row_width, uint64_t* col_width);
/* The render's own device lookup for n unit directions (host arrays, each output may be NULL): rgb (3 floats),
 * texel = i * W + j, pdf_w = the solid-angle density with which the environment sample picks that direction (without T_e). */
int prt_environment_eval(PrtContext* ctx, uint32_t n, const float* dirs, float* rgb, uint32_t* texel, float* pdf_w);
/* The texture binding of the current scene ("Image textures" above; NULL = none).  PRT_ERR_INVALID, with the previous
 * binding intact and everything checked before anything is written: no scene; n_materials, n_meshes or n_instanced_meshes
 * differ from the scene's; a texture index out of range; a width or height of 0 or above PRT_TEX_MAX_SIZE; a null image; a
 * negative or non-finite texel; an unknown filter or wrap; a UV that is not finite or of magnitude above 2^20; a textured
 * material that is not Lambertian or Metal; a mesh or placed copy with a textured material and no UVs; an analytic sphere
 * with a textured material.  Waits for the context's stream. */
int prt_set_textures(PrtContext* ctx, const PrtTextureSet* set);
int prt_texture_info(PrtContext* ctx, PrtTextureInfo* out);
/* The render's own device lookup for n (texture, uv) pairs: host arrays, uv 2 floats and rgb 3 floats per pair.  Needs a
 * device and a binding; a texture index out of range or a uv that is not finite or above 2^20 in magnitude: PRT_ERR_INVALID. */
int prt_texture_eval(PrtContext* ctx, uint32_t n, const uint32_t* texture, const float* uv, float* rgb);
/* prt_closest_hit plus what the shade kernels derive from the hit under the binding: uv (2 floats; 0 for a miss or a
 * sphere) and albedo (3 floats: the looked-up colour where the hit's material is textured, else the material's rgb; 0
 * for a miss).  Each output may be NULL.  Needs a device and a binding. */
int prt_hit_uv(PrtContext* ctx, uint32_t n, const float* origins, const float* dirs, PrtHit* hits, float* uv, float* albedo);
/* The exact pmf of the current light set: width[l] = T_l - T_{l-1}, pmf = width / 2^32 (prt_light_info's float is this
 * number rounded).  With the default mask there are no thresholds: PRT_ERR_INVALID. */
int prt_light_intervals(PrtContext* ctx, uint32_t capacity, uint32_t* n_lights, uint64_t* width);
/* The light set of the current scene (host-only contexts too): n_lights, and for the first min(n_lights, capacity)
 * lights the primitive index and the pmf (prim / pmf may be NULL). */
int prt_light_info(PrtContext* ctx, uint32_t capacity, uint32_t* n_lights, uint32_t* prim, float* pmf);
/* One light sample per (hit, in_dir, key) through the device code the render uses (keys = the path's RNG state at the
 * vertex, not advanced).  Host arrays.  Per i: shadow_dirs (3 floats), tmax, light (0xFFFFFFFF: none: not Lambertian,
 * no light, or pdf 0), contrib (3 floats: (albedo / pi) Le max(0, n.w) w_L / pdf_light, throughput 1, unclamped),
 * pdf_light = pmf * pdf_w, pdf_bsdf = max(0, n.w) / pi, w_light under the context's lighting mode (OFF is taken as
 * NEE_MIS), and w_bsdf: the weight a scattered segment from the same vertex along the same direction gets when it meets
 * that light (the render's own evaluation; 1 - w_light up to rounding).  hits[i].normal is the shading normal as
 * prt_closest_hit returns it (flipped to the incoming side).  An environment sample reports light =
 * PRT_LIGHT_ENVIRONMENT, tmax = +inf and w_bsdf = the weight of a miss along that direction.  The light is picked by the
 * active selection (prt_set_light_selection): under clustered selection pdf_light = fl(P_c pmf_in) pdf_w. */
int prt_sample_light(PrtContext* ctx, uint32_t n, const float* in_dirs, const PrtHit* hits, const uint32_t* keys,
                     float* shadow_dirs, float* tmax, uint32_t* light, float* contrib, float* pdf_light, float* pdf_bsdf,
                     float* w_light, float* w_bsdf);

/* ---- Film statistics and adaptive sampling ------------------------------------------------------
 * Film statistics.  While they are on (prt_set_film_statistics; off by default) the context keeps, beside every local
 * pixel's {r, g, b, weight} sums, the first two moments {A, Q} of its samples' luminance.  For every sample added to the
 * film, in sample order, with r, g, b exactly the three numbers that are added to the film (under a lighting mode the
 * component-wise fp32 sums rad + lrad):
 *     y = fl(fl(fl(0.2126f r) + fl(0.7152f g)) + fl(0.0722f b));   A = fl(A + y);   Q = fl(Q + fl(y y))
 * single fp32 operations, never contracted.  Statistics change neither the route of a batch (compact primary rays, the
 * one-walk-per-pixel list and the path kernel all still run; prt_kernel_instance / prt_shade_instance report what they
 * reported) nor one bit of the film: the accumulate kernels of their own (k_accumulate_stat) add the same samples in the
 * same order.  prt_film_clear and prt_set_film clear (resize) the moments with the film.  A pixel outside the image or not
 * owned by this rank has none.
 *
 * The stopping rule, in double, in this order, of a pixel's film weight n and moments A, Q:
 *     m = A / n;  V = max(0, Q / n - m m);  lhs = V / (n - 1);  t = threshold (m + noise_floor);
 *     unconverged = n < 2 || lhs > t t
 * i.e. a pixel is converged once the standard error of its mean luminance is at most `threshold` times (the mean +
 * noise_floor).  It is written once (csrc/prt_adaptive.h) and compiled for the device and for the host;
 * prt_adaptive_unconverged is the host's copy.  A pixel outside the image is converged.  An 8x8 tile is ACTIVE while any of
 * its pixels is unconverged: a wave ballot, no floating-point reduction, so the decision cannot depend on an order.
 *
 * prt_render_adaptive adds a different number of samples to every tile.  Pass 0 adds min_spp samples (indices first_sample
 * .. first_sample + min_spp - 1) to every tile exactly as prt_render would; min_spp = 0 skips it and starts from what the
 * film holds (that is how a finished frame is refined further: a later first_sample, so that no index is used twice).
 * Then, with `added` = the samples this call has given the still-active tiles so far (min_spp after pass 0):
 *     1. select: of the tiles active so far (at first: all local tiles) those that are active by the rule now;
 *     2. read their number back (one small wait per pass);
 *     3. stop if there is none, or if added >= max_spp;
 *     4. add k = min(step_spp, max_spp - added) samples, indices first_sample + added .. + k - 1, to the active tiles only,
 *        split into batches of samples_in_flight as prt_render splits; added += k.
 * A tile that drops out never returns (it receives nothing, so the rule keeps saying what it said), hence all tiles of a
 * pass share one index range, and a pixel that ends with weight n more than it had holds samples first_sample ..
 * first_sample + n - 1 of this call: since the RNG is keyed by (global pixel, sample, seed) and samples are added in sample
 * order, it equals that pixel of a uniform n-sample prt_render bit for bit, and its film weight is its sample count.  The
 * passes over a tile list always take the unfused full-record pipeline (no fused segment, no compact primary rays, no path
 * kernel; every shade instance, lighting mode, environment, lens and texture binding works under it), which computes the
 * samples the other routes compute.  The result does not depend on a tunable, on samples_in_flight, on the tree's builder
 * or on the partition (tiles are decided one by one: a 3-rank partition assembles to the 1-rank film).
 * rays_per_depth, rays_total and the light statistics count what ran; PrtStats.samples counts whole-film samples only
 * (pass 0).  Synchronous on return.
 * PRT_ERR_INVALID, with nothing rendered (checked before the device is, so host-only contexts refuse the same way):
 * statistics off; threshold or noise_floor negative or NaN; both 0; max_spp < min_spp; step_spp == 0 with max_spp >
 * min_spp; max_depth out of range. */
typedef struct PrtAdaptive {
    uint32_t min_spp, step_spp, max_spp;
    float threshold, noise_floor;
} PrtAdaptive;
typedef struct PrtAdaptiveInfo {
    uint32_t passes;          /* passes over a tile list that rendered (pass 0 is not one) */
    uint32_t tiles_local;     /* tiles of this rank */
    uint32_t tiles_converged; /* tiles the rule stopped (at any count, max_spp included) */
    uint32_t tiles_capped;    /* tiles still active when max_spp was reached */
    uint32_t min_tile_spp;    /* fewest / most samples this call gave a tile (0 / 0 for a rank without tiles) */
    uint32_t max_tile_spp;
    uint64_t pixel_samples;   /* samples this call added to pixels inside the image */
} PrtAdaptiveInfo;
/* on != 0 / 0.  A call that changes the setting clears the film (and waits for the stream); one that does not is a no-op.
 * Host-only contexts only record the setting.  The setting stays with the context across prt_set_film / prt_set_scene. */
int prt_set_film_statistics(PrtContext* ctx, int on);
int prt_get_film_statistics(const PrtContext* ctx); /* 1 / 0 */
/* The moments in Film layout (H*W floats each, either may be NULL): A into sum_y, Q into sum_y2; 0 for pixels this rank
 * does not own.  Statistics off: PRT_ERR_INVALID. */
int prt_film_statistics_read(PrtContext* ctx, float* sum_y, float* sum_y2);
/* Per pixel (H*W floats), evaluated in double on the host and rounded once: sqrt(V / (n - 1)) / (m + noise_floor) with n,
 * m, V as in the rule; +inf where n < 2 (pixels this rank does not own included); IEEE 0 / 0 = NaN where a black pixel
 * meets noise_floor = 0.  noise_floor negative or NaN, or statistics off: PRT_ERR_INVALID. */
int prt_film_noise_read(PrtContext* ctx, float noise_floor, float* rel_err);
int prt_adaptive_unconverged(float n, float A, float Q, float threshold, float noise_floor); /* 1 / 0 */
int prt_render_adaptive(PrtContext* ctx, const PrtAdaptive* cfg, uint32_t max_depth, uint32_t seed, uint32_t first_sample,
                        PrtAdaptiveInfo* out /* may be NULL */);
/* Function level: step 1 of the loop (select) on caller-supplied moments, through the kernels the loop launches.  n, sum_y,
 * sum_y2: H*W floats each in Film layout (the film weight and the moments A, Q of every pixel); pixels this rank does not
 * own are ignored.  prev: n_prev local tile indices (tile lt of this rank is global tile lt * world + rank), or NULL for
 * local tiles 0 .. n_prev - 1.  list (room for n_prev entries) receives the entries of prev that are active by the rule,
 * in the order of prev, and 0xFFFFFFFF in the entries past them; counts[0] = how many, counts[1] = the pixels of those
 * tiles that lie inside the image.  Needs only
 * prt_set_film; the context's film and statistics are neither read nor written (the images go to scratch memory in tile
 * layout, padding lanes zero).  Synchronous on return.
 * PRT_ERR_INVALID (checked on the host before the device is): a null array; n_prev above the local tile count; a
 * prev[i] >= the local tile count; threshold or noise_floor negative or NaN; both 0. */
int prt_tile_select(PrtContext* ctx, const float* n, const float* sum_y, const float* sum_y2, const uint32_t* prev /* may be NULL */,
                    uint32_t n_prev, float threshold, float noise_floor, uint32_t* list, uint32_t* counts /* [2] */);

/* ---- First-hit feature images and the edge-avoiding film denoiser ---------------------------------
 * Feature images (prt_render_features).  For every pixel of the film ONE pinhole ray through the pixel centre
 * (x + 0.5, y + 0.5): the context's camera with PrtLens.fov_y honoured and the aperture ignored (prt_camera_rays' ray), no
 * jitter, no random number.  The pass covers the whole W x H image whatever rank / world_size the film has (the scene is
 * replicated on every rank: nothing is gathered).  The ray's closest hit is exactly what prt_closest_hit returns for it.
 * Per pixel, Film layout (row 0 on top):
 *    albedo[3]    Lambertian or Metal hit: the material's rgb, or the textured colour prt_hit_uv reports while a binding
 *                 textures at least one material; Dielectric hit, Emissive hit or a miss: (1, 1, 1)
 *    normal[3], position[3]   PrtHit.normal (already flipped to the incoming side) and PrtHit.position; zeros for a miss
 *    prim (int32) PrtHit.prim, -1 for a miss
 *    depth        sqrtf(d2), 0 for a miss (exported only: the filter uses positions)
 * The pass is its own: no render route, kernel instance, film bit, ray count or statistic of a render call changes.  The
 * records stay on the device with the context (three 16-byte records per pixel) until one of prt_set_scene,
 * prt_clone_scene (into this context), prt_set_camera, prt_set_film, prt_set_lens, prt_set_textures, prt_refit_meshes or
 * prt_set_instance_transforms is called, successful or not; prt_features_read without a current set is PRT_ERR_INVALID.
 * Limitations: the features are the FIRST hit of the CENTRE ray.  This set does not follow mirrors or glass (a mirror
 * shows its own plane, a glass ball its own surface; "Guide features through specular chains" below is the opt-in that
 * does), and it does not average over a lens or over jitter (a defocused or anti-aliased edge has the features of one side).
 *
 * Guide features through specular chains (PrtFeatureTrace below; off by default: with max_specular = 0 no route, kernel
 * instance, film bit, ray count, statistic or feature record differs from what is described above).
 * Two sets.  The FIRST-HIT set is exactly what is described above (same kernels, same bits; prt_features_read).  While
 * max_specular > 0, prt_render_features also writes a GUIDE set, three more 16-byte records per pixel, which
 * prt_features_read_guide reads; with max_specular = 0 there is none, and prt_features_read_guide returns the first-hit set
 * with bounces = 0.  The spatial filter of prt_film_denoise, prt_group_film_denoise and the dn != NULL stage of
 * prt_film_temporal takes the guide set while max_specular > 0; the reprojection of prt_film_temporal keeps the first-hit
 * set (a mirror is reprojected as its own plane, which is right for geometry); prt_denoise and prt_denoise_device take the
 * caller's arrays.  Both sets are dropped together by every call of the list above and by prt_set_feature_trace.
 * The chain.  fp32, one rounding per written operation, never contracted; reflect3, refract3, fresnel_reflectance,
 * normalize3, dot3 and glm_min are the device functions of the shade kernels (csrc/prt_device.h).  Per pixel, start with
 * (o, d) = the centre ray, T = (1, 1, 1), L = 0, k = 0.
 *  1. h = the closest hit of (o, d), exactly what prt_closest_hit returns (for k = 0 it is the first-hit pass's record).
 *     A miss is a terminal miss.
 *  2. The hit's material has type t, colour rgb (the colour prt_hit_uv reports for this segment's hit while a binding
 *     textures at least one material) and scalar s; N = h.normal (flipped to the incoming side).
 *     Metal, s <= roughness_max and k < max_specular: r = normalize3(normalize3(reflect3(d, N))) (material_scatter's Metal
 *       branch without its roughness term); follow iff dot3(r, N) > 0 and r is finite; then T = T * rgb per channel, d' = r.
 *     Dielectric, k < max_specular: ri, cos_theta, sin_theta and cannot as material_scatter computes them;
 *       refl = cannot || fresnel_reflectance(cos_theta, ri) > 0.5f (the more probable branch of the stochastic scatter; no
 *       random number); d' = normalize3(refl ? reflect3(d, N) : refract3(d, N, ri)); follow iff d' is finite; T unchanged.
 *     Following: L = L + sqrtf(h.d2), o = h.position, d = d', k = k + 1, back to 1 (the closest hit's own t >= 1e-3 keeps
 *       the next segment off the surface it starts on).
 *     Everything else is terminal: Lambertian, Emissive, a rough Metal, a test above that fails, k = max_specular.
 *  3. Terminal hit: albedo = T * a per channel (a = rgb or the textured colour for Lambertian / Metal, (1, 1, 1) for
 *     Dielectric / Emissive); normal, position, prim = h's; depth = L + sqrtf(h.d2); bounces = k.
 *     Terminal miss: albedo = T, normal = position = 0, prim = -1, depth = 0, bounces = k (the filter's rho for a miss stays
 *     (1, 1, 1), as the filter contract says).
 *  4. bounces is stored as a float in the .w of the guide set's albedo record; the first-hit set's .w stays 0.
 * Limitations: one deterministic branch per dielectric vertex (at a glass surface whose reflectance is near 0.5, half of
 * the light went the other way); the features after a chain are those of the surface SEEN (a floor seen in a mirror and
 * the same floor seen directly may be filtered together: after demodulation by T x albedo this is intended for Lambertian
 * surfaces); a Metal rougher than roughness_max is an ordinary surface; the temporal history still reprojects by the first
 * hit; the centre ray only, no lens, no jitter ("Sampled guide features" below is the opt-in that averages over both).
 * tests/guide_features_replay.py restates the chain in numpy float32.
 *
 * Sampled guide features (PrtFeatureSampling below; off by default: with samples = 0 no route, kernel instance, film bit,
 * ray count, statistic, feature record or denoised pixel differs from what is described above).
 * A third set, the SAMPLED set: the average, over K = samples of the render's own primary rays per pixel, of the features at
 * the end of each ray's specular chain.  While samples > 0, prt_render_features also writes it (three more 16-byte records
 * per pixel; the first-hit and guide sets keep their bits) and prt_features_read_sampled reads it; without a current
 * sampled set prt_features_read_sampled is PRT_ERR_INVALID.  The spatial filter of prt_film_denoise, prt_group_film_denoise
 * (rank 0's set) and the dn != NULL stage of prt_film_temporal takes the sampled set while samples > 0, otherwise the guide
 * set while max_specular > 0, otherwise the first-hit set; the reprojection of prt_film_temporal keeps the first-hit set;
 * prt_features_read and prt_features_read_guide return what they return with samples = 0.  The sampled set is dropped with
 * the other sets by every call of the list above, by prt_set_feature_trace and by prt_set_feature_sampling; while
 * samples > 0 a prt_set_sampling that changes jitter drops all sets too (with samples = 0 it drops nothing).
 * The rule.  fp32, one rounding per written operation, never contracted.  The film has W x H pixels, pixel p = y W + x,
 * samples s = 0 .. K - 1.
 *  1. Sample rays.  key = path_seed(p, first_sample + s, seed), the render's seed function.  The pixel-space point is the
 *     centre (x + 0.5f, y + 0.5f); with PrtSampling.jitter it is (x + u1, y + u2), u1 and u2 the key's first two draws, as
 *     the render forms it.  (o, d) is what prt_camera_rays_lens returns for that point and the advanced key under the
 *     context's PrtLens.  These are the primary rays prt_render(spp = K, seed, first_sample) traces; the whole image is
 *     covered whatever the partition, as for the other sets.
 *  2. Per-sample record.  The rule of "Guide features through specular chains" started from (o, d) of the sample instead of
 *     the centre ray, with the context's PrtFeatureTrace (max_specular = 0: the ray is terminal at its first hit, the
 *     first-hit rule): albedo_s, normal_s, position_s, depth_s, prim_s; a terminal miss has albedo_s = T.  The texture
 *     binding applies as it does there.
 *  3. Sums, in sample order s = 0, 1, ..., running fp32.  Sa += albedo_s per channel for every sample; for the samples with
 *     prim_s >= 0: Sn += normal_s, Sp += position_s, Sd += depth_s, hits += 1.  prim = prim_s of the lowest such s.
 *  4. Finish.  albedo = Sa * (1.0f / (float)K).  hits == 0: normal = position = 0, depth = 0, prim = -1.  Otherwise, with
 *     ih = 1.0f / (float)hits: position = Sp * ih, depth = Sd * ih, l2 = dot3(Sn, Sn),
 *     normal = l2 > 0 ? Sn * (1.0f / sqrtf(l2)) : 0.  The normal is renormalised on purpose: the filter raises N_p . N_q to
 *     the 64th power, so an unnormalised mean would switch the filter off exactly where it is needed.
 *  5. Degenerate case.  With jitter == 0 and aperture == 0 every sample is the centre ray: the sampled set is then a bit
 *     for bit copy of the guide set (of the first-hit set when max_specular = 0) with hits = prim >= 0 ? 1 : 0, and nothing
 *     is traced K times.
 * The samples are traced in chunks of whole samples (about 2^22 rays; prt_set_param("feature_chunk", samples per chunk),
 * 0 = by that budget); the sums are ordered, so no result depends on the chunking.
 * Limitations: a pixel with at least one hit counts as a hit for the filter's hit / miss test (partial coverage is not
 * weighted); positions and depths are means of possibly distant surfaces; the temporal history still reprojects by the
 * centre ray's first hit; no variance of the features.  tests/feature_samples_replay.py restates the sums and the finish in
 * numpy float32.
 *
 * The filter contract (prt_denoise and everything built on it): an edge-avoiding a-trous wavelet filter guided by the
 * variance of the mean luminance and by the features above.
 * Inputs per pixel p: mean colour c(p), variance of the mean luminance var(p), albedo, normal N_p, position P_p, prim
 * (prim < 0: a miss).  Parameters: PrtDenoise below (NULL = the defaults).
 * Arithmetic: everything is fp32, one rounding per written operation, never contracted; a dot product is (x + y) + z;
 * lum(c) = (0.2126f r + 0.7152f g) + 0.0722f b as in the film statistics; / and sqrtf are correctly rounded.
 * Constants: k5 = (1/16, 1/4, 3/8, 1/4, 1/16), k3 = (1/4, 1/2, 1/4), RHO_MIN = 2^-6, EPS_L = 2^-20, TINY = 2^-100,
 * W_MIN = 2^-30.
 * Demodulation (demodulate != 0): rho = max(albedo, RHO_MIN) per channel, (1, 1, 1) for a miss; c_0 = c / rho per
 *   channel, var_0 = var / (lum(rho) * lum(rho)).  Otherwise c_0 = c, var_0 = var.  l_0 = lum(c_0).
 * Iteration i = 0 .. iterations - 1, step s = 2^i:
 *   variance prefilter  g(p) = (sum of (k3[dy] k3[dx]) * var_i(q)) / (sum of k3[dy] k3[dx]) over the in-image pixels q of
 *     the 3 x 3 neighbourhood of p at step 1, row-major, each term k * var added to a running sum (the k's sum likewise: it
 *     is exact); den(p) = sigma_l * sqrtf(g(p)) + EPS_L.
 *   taps (dy, dx) in [-2, 2]^2, row-major (dy outer), q = p + s (dx, dy); a tap outside the image is skipped;
 *     h = k5[dy] * k5[dx] (exact).
 *   weight of a tap:
 *     the centre tap: w = h
 *     off-centre, one of p, q a miss and the other a hit: w = 0
 *     off-centre, both misses: wn = 1, xz = 0
 *     off-centre, both hits: wn = max(0, N_p . N_q), then wn = wn * wn repeated normal_power_log2 times;
 *       D = P_q - P_p; xz = |D . N_p| / (sigma_z * sqrtf(D . D) + TINY): the sine of the offset's angle to p's tangent
 *       plane, free of the unit of length
 *     and for both of the last two: xl = |l_i(p) - l_i(q)| / den(p); x = xl + xz;
 *       w = (h * wn) / ((1 + x) + (0.5f * x) * x); w < W_MIN becomes 0
 *   running fp32 sums in tap order, every tap in the image included (w = 0 adds 0):
 *     Sw += w;  Sc += w * c_i(q) per channel;  Sv += (w * w) * var_i(q)
 *   c_{i+1}(p) = Sc / Sw per channel; var_{i+1}(p) = Sv / (Sw * Sw); l_{i+1} = lum(c_{i+1}).  Sw >= 9/64 always.
 * Outputs (K = iterations): out = c_K * rho per channel and var_out = var_K * (lum(rho) * lum(rho)) with demodulation,
 *   c_K and var_K without.  iterations = 0 without demodulation returns the inputs.
 * The falloff 1 / (1 + x + x^2 / 2) is deliberate: exp(-x) for small x, made of exact operations; no expf, no powf.  The
 * variance prefilter is NOT edge-aware: a pixel's output depends on a neighbouring region only through that region's
 * variance images, never through its colours (a region behind a feature edge gets weight 0 exactly).
 * Non-finite inputs give unspecified values in the pixels whose footprint reaches them; never a fault, never an access
 * out of range.  Subnormal intermediates are outside what "bit for bit" covers.  tests/denoise_replay.py restates these
 * lines in numpy float32.  Results depend on no tunable, not on samples_in_flight, the tree builder or the partition. */
typedef struct PrtDenoise {
    uint32_t iterations;        /* 0..6, default 5 */
    float sigma_l;              /* > 0, default 4 */
    float sigma_z;              /* > 0, default 0.1 */
    uint32_t normal_power_log2; /* 0..8, default 6 (the normal weight is max(0, N.N)^64) */
    uint32_t demodulate;        /* 0 / not 0, default 1 */
} PrtDenoise;
#define PRT_DENOISE_MAX_PIXELS (1u << 28)
void prt_denoise_defaults(PrtDenoise* out);
/* The variance of the mean luminance prt_film_denoise feeds the filter with, from a pixel's film weight n and moments
 * A, Q, in double and rounded once: m = A / n; V = max(0, Q / n - m m); var = V / (n - 1).  Where 0 < n < 2:
 * var = fl(m) * fl(m) (one sample says nothing about its spread: the filter takes the pixel for as noisy as it is
 * bright).  n = 0: 0.  Written once (csrc/prt_denoise_contract.h) for the device and the host; this is the host's copy. */
float prt_denoise_variance(float n, float A, float Q);
/* Needs a scene, a camera and a film; synchronous.  PRT_ERR_INVALID beyond the usual: a film above 2^28 pixels. */
int prt_render_features(PrtContext* ctx);
/* Copies the current feature set out (host arrays, H*W*3 floats / H*W floats / H*W int32; each may be NULL). */
int prt_features_read(PrtContext* ctx, float* albedo, float* normal, float* position, float* depth, int32_t* prim);
/* "Guide features through specular chains" above.  A property of the context, like PrtLens: kept across prt_set_scene,
 * prt_set_camera and prt_set_film, and recorded by host-only contexts too. */
typedef struct PrtFeatureTrace {
    uint32_t max_specular;  /* 0..8 specular vertices followed; 0 = first hit only (default) */
    float roughness_max;    /* a Metal with scalar <= this is a mirror; >= 0, finite; default 0.1f */
} PrtFeatureTrace;
#define PRT_FEATURE_MAX_SPECULAR 8u
void prt_feature_trace_defaults(PrtFeatureTrace* out);          /* {0, 0.1f} */
/* NULL = the defaults.  PRT_ERR_INVALID with the previous setting intact (checked before the device is asked for):
 * max_specular > 8; roughness_max negative, NaN or infinite.  Drops the current feature set, as prt_set_lens does. */
int prt_set_feature_trace(PrtContext* ctx, const PrtFeatureTrace* ft);
int prt_get_feature_trace(PrtContext* ctx, PrtFeatureTrace* out);
/* Copies the guide set out (arrays as for prt_features_read, bounces: H*W uint32; each may be NULL); with max_specular = 0
 * the first-hit set and bounces = 0.  PRT_ERR_INVALID without a current feature set. */
int prt_features_read_guide(PrtContext* ctx, float* albedo, float* normal, float* position, float* depth, int32_t* prim,
                            uint32_t* bounces);
/* "Sampled guide features" above.  A property of the context, like PrtFeatureTrace: kept across prt_set_scene,
 * prt_set_camera and prt_set_film, and recorded by host-only contexts too. */
typedef struct PrtFeatureSampling {   /* 12 bytes */
    uint32_t samples;       /* 0 = off (default); 1..PRT_FEATURE_MAX_SAMPLES */
    uint32_t seed;          /* the seed of the prt_render calls whose samples are meant */
    uint32_t first_sample;  /* their first sample index */
} PrtFeatureSampling;
#define PRT_FEATURE_MAX_SAMPLES 64u
void prt_feature_sampling_defaults(PrtFeatureSampling* out);    /* {0, 0, 0} */
/* NULL = the defaults.  PRT_ERR_INVALID with the previous setting intact (checked before the device is asked for):
 * samples > 64.  Every call drops all feature sets, refusals included, as prt_set_feature_trace does. */
int prt_set_feature_sampling(PrtContext* ctx, const PrtFeatureSampling* fs);
int prt_get_feature_sampling(PrtContext* ctx, PrtFeatureSampling* out);
/* Copies the sampled set out (arrays as for prt_features_read, hits: H*W uint32, the samples of the pixel that hit
 * something; each may be NULL).  PRT_ERR_INVALID without a current sampled set (samples = 0 included). */
int prt_features_read_sampled(PrtContext* ctx, float* albedo, float* normal, float* position, float* depth, int32_t* prim,
                              uint32_t* hits);
/* The filter on host arrays (mean, albedo, normal, position, out: W*H*3 floats; var, var_out: W*H floats; prim: W*H
 * int32; var_out may be NULL).  Synchronous.  Needs a device, but neither a scene nor a film.  PRT_ERR_INVALID, checked
 * before the device is asked for (host-only contexts refuse alike): iterations > 6, a sigma <= 0 or NaN,
 * normal_power_log2 > 8, a null array, W * H = 0 or above 2^28. */
int prt_denoise(PrtContext* ctx, const PrtDenoise* cfg, uint32_t W, uint32_t H, const float* mean, const float* var,
                const float* albedo, const float* normal, const float* position, const int32_t* prim, float* out,
                float* var_out);
/* The same on DEVICE arrays, enqueued on the context's stream with no host wait. */
int prt_denoise_device(PrtContext* ctx, const PrtDenoise* cfg, uint32_t W, uint32_t H, const void* d_mean, const void* d_var,
                       const void* d_albedo, const void* d_normal, const void* d_position, const void* d_prim, void* d_out,
                       void* d_var_out);
/* The context's own film through the filter: mean = rgb_sum / weight per channel (fp32), var = prt_denoise_variance of the
 * pixel's weight and moments; a pixel of weight 0 has mean 0 and variance 0.  rgb_out: H*W*3 floats, var_out: H*W floats or
 * NULL, host arrays; synchronous.  Film statistics must be on (PRT_ERR_INVALID otherwise, before the device is asked
 * for); the feature set is rendered first if there is no current one; the film must own the whole image (world_size 1: a
 * partitioned context is refused with a message that names prt_group_film_denoise).  Everything stays on the device (a
 * prepare kernel of its own reads the film and the moments); neither is modified by a bit. */
int prt_film_denoise(PrtContext* ctx, const PrtDenoise* cfg, float* rgb_out, float* var_out);

/* ---- Temporal reprojection: film history carried across moving frames ------------------------------
 * The temporal half of SVGF in front of the spatial filter above: last frame's accumulated colour and luminance moments
 * are carried to where each surface point is now, rejected at disocclusions, and blended with the new frame's samples;
 * the blended moments give the a-trous filter a variance even where a frame holds one sample.
 * Arithmetic: everything is fp32, one rounding per written operation, never contracted; a dot product a . b is
 * (a.x b.x + a.y b.y) + a.z b.z; /, sqrtf and floorf are exact IEEE; the one variance line is in double, rounded once.
 * Previous camera K (PrtCameraBasis): what prt_set_camera / prt_set_lens gave the kernels at the previous step.  K.W and
 *   K.H must equal the image's W and H (PRT_ERR_INVALID otherwise).
 * Inputs per current pixel p: mean colour c, film weight n, luminance sums A, Q with m1 = A / n, m2 = Q / n (both 0
 *   where !(n > 0)), prim, and Pprev, Nprev: the first-hit point and normal AS THEY WERE in the previous frame.
 * History per pixel q of the previous frame: colour hc, length hn (a float counted in samples), moments h1, h2, and that
 *   frame's hP, hN, hprim.
 * Previous surface: (Pprev, Nprev) = (P, N) unless prim lies in the primitive range [prim_base[k], prim_base[k] + the
 *   triangles of its mesh) of placed copy k (prim_base as prt_instances_read reports it; the identity instance of the
 *   world-space meshes is not a placed copy) and a previous transform of copy k is given.  Then, with M = mat, I = inv as
 *   column-major 4 x 4 (PrtInstance), transform_point(M, p) component r = (M[r] p.x + M[4 + r] p.y) + (M[8 + r] p.z +
 *   M[12 + r] * 1.0f) and lin(M, n) component r = (M[r] n.x + M[4 + r] n.y) + M[8 + r] n.z:
 *     Pprev = transform_point(Mprev_k, transform_point(Inv_cur_k, P))
 *     Nprev = normalize3(lin(Mprev_k, lin(Inv_cur_k, N))),  normalize3(v) = v * (1.0f / sqrtf(v . v)) per component
 *   (rotation + uniform scale: exact in direction).  Deformed world-space meshes are not followed: prt_refit_meshes drops
 *   the history.
 * No history for p: there is no history at all; prim < 0 (a miss is deterministic without jitter and needs none);
 *   !(z > 0) with v = Pprev - K.pos, z = v . K.front; the projected point is outside the image; the valid tap weight
 *   Sb < 2^-6.  Then the outputs are c, N' = n, m1, m2, var = prt_denoise_variance(n, A, Q), status 0.
 * Projection, aspect = K.W / K.H:  x = v . K.right;  y = v . K.up;
 *     ndcX = (x / z) / (aspect * K.tan_fov_y);  ndcY = (y / z) / K.tan_fov_y
 *     fx = ((ndcX + 1.0f) * 0.5f) * K.W - 0.5f;  fy = ((1.0f - ndcY) * 0.5f) * K.H - 0.5f
 *   inside iff fx > -1 && fx < K.W && fy > -1 && fy < K.H (a NaN fails).  ix = floorf(fx), tx = fx - ix; iy, ty likewise.
 * Taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) in that order; bilinear weight b = bx * by with bx =
 *   1.0f - tx for the tap at ix and tx for the tap at ix + 1, by likewise (the x factor first).  A tap q is valid iff it is
 *   inside the image, hn(q) > 0, hprim(q) >= 0, Nprev . hN(q) >= normal_min, and |D . Nprev| <= plane_tol * sqrtf(v . v)
 *   with D = hP(q) - Pprev: a plane distance relative to the distance from the previous camera, free of the unit of
 *   length.  A NaN fails each test.
 *   Running fp32 sums in tap order over the valid taps: Sb += b; S += b * hc per channel; b * hn; b * h1; b * h2.  Each sum
 *   divided by Sb: hc, Nh, H1, H2.
 * Blend:  N' = fminf(Nh + n, max_history);  a = fminf(n / N', 1.0f);  c' = hc + a * (c - hc) per channel;
 *   m1' = H1 + a * (m1 - H1);  m2' = H2 + a * (m2 - H2).
 * Variance, in double, rounded once:  V = max(0, m2' - m1' m1');  var' = (float)(V / max(N' - 1, 1)).  Status 1.
 * New history: c', N', m1', m2', the current frame's position, normal and prim, the current basis and the current
 *   transforms of the placed copies.  The a-trous output is display only and is never fed back.
 * Limits: the reprojection uses first-hit features only (no specular chains: a mirror carries the history of its own plane,
 * also while PrtFeatureTrace lets the spatial stage follow them); no 3 x 3 fallback
 *   search where the four taps fail; deforming meshes reset the history; a colour border inside one plane (a texture, a
 *   shadow edge) bleeds by up to a pixel per frame of history, because nothing geometric tells its sides apart; no
 *   multi-GPU form.  Non-finite positions make a pixel take no history; a tap index is never read out of range.
 *   Subnormal intermediates are outside what "bit for bit" covers.  tests/temporal_replay.py restates these lines in numpy
 *   float32. */
typedef struct PrtTemporal {
    float max_history; /* >= 1, default 32: the history length is capped here, so a = n / N' never falls below n / max_history */
    float normal_min;  /* in [-1, 1], default 0.9 */
    float plane_tol;   /* >= 0, default 0.01 */
} PrtTemporal;
typedef struct PrtCameraBasis {
    float pos[3], right[3], up[3], front[3];
    float W, H, tan_fov_y;
} PrtCameraBasis;
typedef struct PrtTemporalInfo {
    uint32_t steps;        /* successful prt_film_temporal calls since the history was last dropped */
    uint32_t resets;       /* how often the history was dropped since the context was created (prt_temporal_reset and every
                              call of the list below, whether a history existed or not) */
    uint32_t hit_pixels;   /* last step: pixels with prim >= 0 */
    uint32_t reprojected;  /* last step: pixels with status 1 */
    uint64_t device_bytes; /* device bytes held for all of this: the history sets and the step's workspace, the motion table,
                              and the workspace of prt_temporal_reproject / _device */
} PrtTemporalInfo;
#define PRT_TEMPORAL_MAX_PIXELS (1u << 28)
void prt_temporal_defaults(PrtTemporal* out);
/* The basis the kernels have now (prt_set_camera's right / up / normalised front, prt_set_lens' tan_fov_y).  Needs a
 * camera. */
int prt_get_camera_basis(PrtContext* ctx, PrtCameraBasis* out);
/* The pure function on host arrays (c, Pprev, Nprev, hc, hP, hN, c_out: W*H*3 floats; n, A, Q, hn, h1, h2, n_out, m1_out,
 * m2_out, var_out: W*H floats; prim, hprim: W*H int32; status: W*H bytes).  hc == NULL (then every history array is
 * ignored): no history at all.  var_out and status may be NULL.  Synchronous; needs a device but neither a scene nor a
 * film.  PRT_ERR_INVALID, checked before the device is asked for (host-only contexts refuse alike): max_history < 1 or
 * NaN, normal_min outside [-1, 1] or NaN, plane_tol negative or NaN, a null array, W * H = 0 or above 2^28, H above
 * 262140 (one launch covers 65535 blocks of 4 rows), K's W / H not the image's. */
int prt_temporal_reproject(PrtContext* ctx, const PrtTemporal* cfg, uint32_t W, uint32_t H, const PrtCameraBasis* K, const float* c,
                           const float* n, const float* A, const float* Q, const int32_t* prim, const float* Pprev, const float* Nprev,
                           const float* hc, const float* hn, const float* h1, const float* h2, const float* hP, const float* hN,
                           const int32_t* hprim, float* c_out, float* n_out, float* m1_out, float* m2_out, float* var_out,
                           uint8_t* status);
/* The same on DEVICE arrays, enqueued on the context's stream with no host wait. */
int prt_temporal_reproject_device(PrtContext* ctx, const PrtTemporal* cfg, uint32_t W, uint32_t H, const PrtCameraBasis* K, const void* d_c,
                                  const void* d_n, const void* d_A, const void* d_Q, const void* d_prim, const void* d_Pprev,
                                  const void* d_Nprev, const void* d_hc, const void* d_hn, const void* d_h1, const void* d_h2,
                                  const void* d_hP, const void* d_hN, const void* d_hprim, void* d_c_out, void* d_n_out, void* d_m1_out,
                                  void* d_m2_out, void* d_var_out, void* d_status);
/* The previous-surface rule against the context's current scene, on the host (the lines the film kernel compiles): n points
 * with their normals and prims; prev_instances: the n_prev placed copies as they were (mat is read), n_prev = the scene's
 * placed copies, or 0 (nothing moved: the outputs are the inputs).  Needs a scene, no device.  PRT_ERR_INVALID: a null
 * array, n_prev neither 0 nor the scene's count. */
int prt_temporal_prev_surface(PrtContext* ctx, uint32_t n, const float* position, const float* normal, const int32_t* prim,
                              const PrtInstance* prev_instances, uint32_t n_prev, float* Pprev, float* Nprev);
/* One frame step on the context's own film: c = rgb_sum / weight, n = weight, A, Q = the moments, the current feature set
 * as the surface (rendered first if there is no current one), the history the context keeps from the previous step.  The
 * blended frame then goes through the spatial filter (dn, the contract above, the variance being var'), or is returned
 * as it is (dn == NULL).  rgb_out: H*W*3 floats; var_out, history_out (N' per pixel): H*W floats or NULL; host arrays,
 * synchronous; nothing else leaves the device.  Film statistics must be on; the film must own the whole image (world_size
 * 1: a partitioned context is refused; a group form does not exist yet).  Film and moments are not modified by a bit: the
 * caller clears the film between frames (prt_film_clear), and a film that was not cleared is counted again.
 * The history is dropped by prt_temporal_reset, prt_set_scene, prt_clone_scene into the context, prt_set_film,
 * prt_refit_meshes, prt_set_textures and a prt_set_film_statistics that changes the setting; prt_set_camera, prt_set_lens
 * and prt_set_instance_transforms keep it: motion is what it is for. */
int prt_film_temporal(PrtContext* ctx, const PrtTemporal* cfg, const PrtDenoise* dn /* NULL: no spatial filter */, float* rgb_out,
                      float* var_out, float* history_out);
int prt_temporal_reset(PrtContext* ctx);
int prt_temporal_info(PrtContext* ctx, PrtTemporalInfo* out);

/* ---- Film read-back (Film::m_Accum / m_Weights; src/core/film.h:54-60) ------------------------ */
/* Whole film to host, row-major, top-left origin; only pixels owned by this rank are non-zero. */
int prt_film_read(PrtContext* ctx, float* rgb_sum, float* weight);
/* Device pointer + float count of this rank's tile-ordered accumulation ([local_tile][64][4] =
 * r,g,b,weight) — the payload of the per-frame RCCL gather. Padded so every rank has the same count. */
int prt_film_local(PrtContext* ctx, void** d_ptr, uint64_t* n_floats);
/* Un-tile a gathered buffer (world_size consecutive rank payloads) into film layout on the device:
 * d_rgb_sum [H*W*3], d_weight [H*W].  Equivalent of Film::AddSampleBufferGPU's target layout
 * (src/core/film.cu:79-99). */
int prt_film_resolve(PrtContext* ctx, const void* d_gathered, uint32_t world_size, void* d_rgb_sum, void* d_weight);
/* The same on a stream of the caller's choice (NULL = the context's stream): the per-frame gather and this un-tiling can
 * then run on a side stream from a snapshot of the payload while the context's stream already renders the next frame. */
int prt_film_resolve_on(PrtContext* ctx, void* hip_stream, const void* d_gathered, uint32_t world_size, void* d_rgb_sum,
                        void* d_weight);
/* Film::UpdateDisplayGPU (src/core/film.cu:101-132): mean -> Reinhard -> gamma -> RGBA8, from device
 * film buffers to a device RGBA8 buffer [H*W*4]. */
int prt_film_tonemap(PrtContext* ctx, const void* d_rgb_sum, const void* d_weight, float exposure, float gamma, void* d_rgba8);
/* Convenience: resolve this context's own film (world_size==1) and tonemap to host RGBA8. */
int prt_film_display(PrtContext* ctx, float exposure, float gamma, uint8_t* rgba8);

/* ---- function-level entry points (used by the parity tests; all go through the same kernels) -- */
/* Camera::GetCameraRay at pixel-space points (px,py)  (src/core/camera.h:103-132). Host in/out. */
int prt_camera_rays(PrtContext* ctx, uint32_t n, const float* px, const float* py, float* origins, float* dirs);
/* The render's own device code for n pixel-space points under the context's lens.  keys = the path's RNG state BEFORE the
 * lens draws, advanced in place by two draws while aperture > 0 and left alone otherwise.  Host in/out. */
int prt_camera_rays_lens(PrtContext* ctx, uint32_t n, const float* px, const float* py, uint32_t* keys, float* origins,
                         float* dirs);
/* Scene::Intersect for n rays (src/core/scene.h:22-25).  Host in/out. */
int prt_closest_hit(PrtContext* ctx, uint32_t n, const float* origins, const float* dirs, PrtHit* hits);
/* The same from DEVICE arrays (n x 3 floats each; d_hits: n PrtHit records), enqueued on the context's stream with no
 * host wait. */
int prt_closest_hit_device(PrtContext* ctx, uint32_t n, const void* d_origins, const void* d_dirs, void* d_hits);
/* Occlusion (shadow-ray) query: occluded[i] = 1 iff tmax[i] > 0 and the closest hit of ray i (exactly what
 * prt_closest_hit returns) lies at d2 < fl32(tmax[i] * tmax[i]); else 0.  A blocker at exactly tmax does not occlude,
 * tmax = +inf occludes on any hit, a NaN / zero / negative tmax or a zero direction never occludes.  The walk stops at
 * the first blocker it accepts.  Host arrays; synchronous, like prt_closest_hit; a ray the walk had to give up
 * (two-level stack overflow) is an error, never a silent 0. */
int prt_occluded(PrtContext* ctx, uint32_t n, const float* origins, const float* dirs, const float* tmax,
                 uint8_t* occluded);
/* The same from DEVICE arrays (n x 3 floats, n floats, n bytes), enqueued on the context's stream with no host wait; a
 * traversal error is reported by the next prt_synchronize. */
int prt_occluded_device(PrtContext* ctx, uint32_t n, const void* d_origins, const void* d_dirs, const void* d_tmax,
                        void* d_occluded);
/* MaterialHandle::Scatter + Emit for n (ray, hit, rng state) tuples (src/core/material.h:139-161).
 * rng_state is advanced in place. scattered[i] = 0/1.  The attenuation is the material's constant rgb whatever textures are
 * bound (the inputs carry no UV); so is the albedo of prt_sample_light's contrib. */
int prt_scatter(PrtContext* ctx, uint32_t n, const float* in_dirs, const PrtHit* hits, uint32_t* rng_state,
                uint32_t* scattered, float* attenuation, float* emitted, float* out_origins, float* out_dirs);

/* ---- Radiance query: whole paths for rays the caller supplies ----------------------------------
 * "What radiance arrives along this ray?" for n rays from outside a render: light probes, lightmap texels, panoramic,
 * fisheye or orthographic cameras, training data.  The path of ray i, sample s is the reference's iterative path
 * (TraceRayGPU, src/backend/cuda_megakernel/renderer.cu:81-119), which is what a render follows:
 *  RNG state: with rng_state given the path starts from rng_state[i], `samples` must be 1 and the state the path ends with
 *    is written back (as prt_scatter advances its states).  With rng_state NULL the path starts from
 *    path_seed(i, first_sample + s, seed): the ray index stands where the pixel index stands in a render, so the query
 *    over a film's own primary rays, ray index = pixel index, follows the render's paths draw for draw.
 *  Path: up to max_depth segments.  Each takes the closest hit exactly as prt_closest_hit returns it (directions are used
 *    as given, not normalised); then L += thr * emitted, Material::Scatter, thr *= attenuation, the scattered direction
 *    normalised: fp32, no contraction, the order of the shade kernels.  The material's draws are made on the last
 *    segment too (the state written back is the reference's; a render skips them there, its radiance is the same).
 *  Miss: L += thr * sky, or thr * the environment image's texel of the direction while one is set (prt_set_environment).
 *    The lookup is defined for unit directions and the caller's direction is used as given, so on the caller's own
 *    segment (k = 0) the texel is that of the normalised direction: with l2 = fl((x*x + y*y) + z*z) in fp32, where
 *    |l2 - 1| > 2^-20 the lookup takes d * (1 / sqrt(l2)) (glm::normalize), otherwise d itself.  A direction normalised
 *    in fp32 has l2 within about 2^-22 of 1 and is looked up bit for bit as given.  The path's direction is not touched:
 *    hits, scatter and segments are the reference's for the direction as given.  Later segments are unit by construction.
 *  Textures: a textured Lambertian or Metal takes its albedo from the binding at the hit's UV, as a render does.
 *  Sampling: PrtSampling.rr_depth (one draw after the material's own, before segment index >= rr_depth) and clamp (on the
 *    radiance a path delivers) apply as in a render; jitter has no meaning here and is ignored.  So is the lens.
 *  Lighting: the estimator is always the reference's unidirectional one.  prt_set_lighting, prt_set_light_sources and
 *    prt_set_light_selection do not change a bit of the result; the expectation is the same for every setting.
 *  Outputs: rgb_sum[i] = the fp32 sum over s ascending (from 0.0f) of the clamped path radiance: a sum, not a mean, as in
 *    the film.  segments[i] = the segments walked, summed over the samples.  max_depth == 0: every output is zero and
 *    rng_state is left alone.
 *  Side effects: none on the film, film statistics, feature sets, temporal history, ray / light statistics and batch
 *    instance names; a render after a query equals the same render without it bit for bit.
 *  PRT_ERR_INVALID: no scene; a null query, origins, dirs or rgb_sum; samples == 0 or > PRT_RADIANCE_MAX_SAMPLES; rng_state
 *    together with samples > 1; n * samples > 2^32 - 1.  n == 0 is OK and does nothing.
 *  Cost: chunks of whole samples (about 2^22 rays, at least one sample), and per chunk up to max_depth rounds of: one
 *    4-byte read of the live count, the ray-query pipeline of prt_closest_hit_device over the live rays only, the UV pass
 *    while a binding textures something, one step kernel that compacts the survivors.  Results never depend on the chunk
 *    size (prt_set_param("radiance_chunk", samples per chunk; 0 = by the ray budget)) or on any other tunable.
 * Light sampling: prt_radiance_lit, below.  Not offered: the group (prt_group_*). */
#define PRT_RADIANCE_MAX_SAMPLES 4096u
typedef struct PrtRadianceQuery {
    uint32_t max_depth;     /* segments per path at most; 0: every output is zero */
    uint32_t samples;       /* >= 1, <= PRT_RADIANCE_MAX_SAMPLES */
    uint32_t seed;
    uint32_t first_sample;
} PrtRadianceQuery;
/* Host arrays: origins, dirs n x 3 floats; rng_state NULL or n, in / out; rgb_sum 3 n; segments NULL or n.  Synchronous. */
int prt_radiance(PrtContext* ctx, const PrtRadianceQuery* q, uint32_t n, const float* origins, const float* dirs,
                 uint32_t* rng_state, float* rgb_sum, uint32_t* segments);
/* The same from DEVICE arrays, on the context's stream: enqueued, with one small wait per bounce (the live count, as
 * prt_render_adaptive has one per pass); the outputs are complete in stream order when the call returns. */
int prt_radiance_device(PrtContext* ctx, const PrtRadianceQuery* q, uint32_t n, const void* d_origins, const void* d_dirs,
                        void* d_rng_state, void* d_rgb_sum, void* d_segments);

/* The light-sampled radiance query: prt_radiance's paths with the estimator a prt_render would use now: the context's
 * lighting mode (prt_set_lighting), light source mask, light selection and environment share.  prt_radiance and
 * prt_radiance_device keep their contract, their bits and their cost.
 *  Mode PRT_LIGHTING_OFF: rgb_sum, segments and rng_state are prt_radiance's bit for bit, and no shadow ray is cast.
 *  Otherwise the path of ray i, sample s is the unlit query's draw for draw: segments and the rng_state written back are
 *    prt_radiance's (the light stream never advances the path's state), and the path carries what a lit render's path
 *    carries.  Per segment k, with pb = -1 at k = 0 and the light sum lsum = 0:
 *    Miss: L += thr * sky; under an environment image thr * its texel, times the MIS weight of (d, pb) where that is not 1
 *      (pb < 0: weight 1).  At k = 0 the texel is looked up by prt_radiance's rule for the caller's own segment: the
 *      normalised direction where |l2 - 1| > 2^-20, else the direction as given.  The path ends.
 *    Hit: key = the state before the material's draws; Material::Scatter as in the unlit query, on the last segment too;
 *      L += thr * emitted, times the weight 1 - w_L of the emitter where the material is Emissive, pb >= 0, the emitter is
 *      analytic or the MESH bit is set, and the weight is not 1 (the segment's own origin and direction, the hit's d2).
 *    Light sample: only at a Lambertian vertex that scattered, with k + 1 < max_depth: toward the environment if its draw
 *      of `key` says so, else toward the light set if it is not empty; with the hit's position and normal, the albedo the
 *      step attenuates by (the texture binding's where one applies), thr before this vertex's attenuation, `key` and
 *      PrtSampling.clamp: prt_sample_light's sample, scaled by thr.  A shadow ray (x, w, tmax) is cast iff there is a
 *      sample and pb(w) > 0; it is occluded by prt_occluded's rule (tmax = +inf toward the environment).  Unoccluded:
 *      lsum += contrib (clamped on its own), in vertex order.
 *    Carry on: thr *= attenuation, d = the scattered direction normalised, pb = max(0, n.d) / pi after a Lambertian vertex,
 *      else -1; the roulette is the unlit step's.
 *  Sample value: clamp(L) + lsum, one fp32 add per component: what a lit render adds to its film.  rgb_sum[i] = the fp32
 *    sum of the sample values over s ascending, from 0.0f, whatever the chunking.  So the lit query over a film's own
 *    primary rays, ray index = pixel index, is the lit render, bit for bit.
 *  info (may be NULL): the shadow rays this call cast and how many were occluded.  prt_get_light_stats does not move; the
 *    other side effects are prt_radiance's: none.
 *  Refusals: prt_radiance's, decided without a device; then PRT_ERR_NO_DEVICE on a host-only context.
 *  Cost: prt_radiance's rounds; a round's shadow rays are resolved at the top of the next round (the occlusion pipeline
 *    of prt_occluded_device and one small kernel), after the one wait that reads the live count and the shadow count
 *    together.  The last segment takes no light sample, so the host waits at most once per round, as in the unlit query,
 *    plus once per call where info is given.  "radiance_chunk" applies to both queries. */
typedef struct PrtRadianceLitInfo {
    uint64_t shadow_rays, shadow_occluded;
} PrtRadianceLitInfo;
int prt_radiance_lit(PrtContext* ctx, const PrtRadianceQuery* q, uint32_t n, const float* origins, const float* dirs,
                     uint32_t* rng_state, float* rgb_sum, uint32_t* segments, PrtRadianceLitInfo* info);
/* The same from DEVICE arrays on the context's stream.  info is a HOST pointer; NULL: no final wait for it. */
int prt_radiance_lit_device(PrtContext* ctx, const PrtRadianceQuery* q, uint32_t n, const void* d_origins, const void* d_dirs,
                            void* d_rng_state, void* d_rgb_sum, void* d_segments, PrtRadianceLitInfo* info);
/* The lit query for rays that a Lambertian vertex of the caller's scattered: pb[i] (n floats) is the pdf of that scatter
 * along ray i, max(0, n.d) / pi, and path (i, s) starts with pb = pb[i] where prt_radiance_lit starts with -1.  The value
 * is used as given, for every sample of ray i; everything else is prt_radiance_lit's contract.  So an Emissive hit of a
 * light-set emitter on segment 0, and an environment miss on segment 0, carry the weight 1 - w_L of (origin, direction,
 * pb[i]) exactly as on a later segment after a Lambertian vertex: a caller who takes the first vertex's light sample
 * themselves and continues here counts direct light once under PRT_LIGHTING_NEE_MIS and PRT_LIGHTING_NEE.
 *  pb == NULL: prt_radiance_lit / prt_radiance_lit_device, bit for bit.  A value that is not >= 0 (negative, NaN): no
 *    weighting on segment 0, as with -1.
 *  Mode PRT_LIGHTING_OFF: pb is ignored and the result is prt_radiance's.
 *  Refusals and cost: prt_radiance_lit's. */
int prt_radiance_lit_pb(PrtContext* ctx, const PrtRadianceQuery* q, uint32_t n, const float* origins, const float* dirs,
                        uint32_t* rng_state, const float* pb, float* rgb_sum, uint32_t* segments, PrtRadianceLitInfo* info);
int prt_radiance_lit_pb_device(PrtContext* ctx, const PrtRadianceQuery* q, uint32_t n, const void* d_origins, const void* d_dirs,
                               void* d_rng_state, const void* d_pb, void* d_rgb_sum, void* d_segments, PrtRadianceLitInfo* info);

/* ---- Surface baking: irradiance maps over a mesh's UV layout ------------------------------------
 * From a mesh to the rays of its texels, on the device: the UV layout is rasterised into a W x H map, every covered texel
 * becomes a Lambertian path vertex of albedo 1, its rays are followed by the radiance query and summed per texel.
 *  Target: world-space mesh `index` of the current scene (PRT_BAKE_MESH) or placed copy `index` (PRT_BAKE_INSTANCE), on a
 *    width x height map, 1 <= width, height <= PRT_TEX_MAX_SIZE.  uvs: n_vertices x 2 floats (host) for this call, a
 *    lightmap layout being usually a second UV set; NULL: the UVs the current texture binding gave that mesh (a placed
 *    copy: its instanced mesh).  The convention is the textures': row 0 is the top, v = 0 the bottom row.  UVs are not
 *    wrapped: what lies outside [0,1]^2 is clipped.  The geometry is the scene's current one, after either refit too.
 *  Texel t = i * W + j has the centre px = (j + 0.5) / W, py = 1 - (i + 0.5) / H, in double.
 *  Coverage: face f with UVs a, b, c (fp32 widened to double; every operation below rounded once, no contraction):
 *      A2 = (bx-ax)(cy-ay) - (by-ay)(cx-ax)
 *      E0 = (bx-px)(cy-py) - (by-py)(cx-px)   E1 = (cx-px)(ay-py) - (cy-py)(ax-px)   E2 = (ax-px)(by-py) - (ay-py)(bx-px)
 *    covers the texel iff its UVs are finite, A2 != 0, E0, E1, E2 are all >= 0 (A2 > 0) or all <= 0 (A2 < 0), and the centre
 *    lies in the face's closed UV box: min(ax,bx,cx) <= px <= max(ax,bx,cx) and min(ay,by,cy) <= py <= max(ay,by,cy),
 *    plain double comparisons.  Edges are inclusive, so a shared edge leaves no crack.  In exact arithmetic the box follows
 *    from the edge functions; it is part of the rule because the rounded edge functions of a near-collinear face can all be
 *    exactly zero along its whole line, far from the face: the box bounds what rounding can claim.  The owner is the lowest
 *    covering face index, whatever the launch order.
 *  Surface: b1 = (float)(E1 / A2), b2 = (float)(E2 / A2), w0 = 1.0f - b1 - b2; then in fp32 per component
 *    x = (w0 * X0 + b1 * X1) + b2 * X2, for the position from the face's vertices and for ns from its vertex normals (the
 *    hit reconstruction's order).  l2 = dot(ns, ns), (x*x + y*y) + z*z: a texel with !(l2 > 0 && l2 < inf) is degenerate:
 *    it is not covered, its owner reads 0xFFFFFFFF and n_degenerate counts it.  Otherwise n = ns * (1 / sqrt(l2)).  A placed
 *    copy's position then goes through Mat and its normal through Inv (renormalised) as a hit's do.
 *  Rays: sample s of texel t starts from rng = path_seed(t, first_sample + s, seed): the index in the full map, so a
 *    texel's samples do not depend on coverage elsewhere.  Material::Scatter of a Lambertian of albedo (1,1,1) with the
 *    incoming direction -n, position p, normal n, front face; o = p, d = the scattered direction normalised once more,
 *    as the radiance query's step does; the state is the advanced one.
 *  Paths: from there the path is prt_radiance's path for (o, d, rng_state) with q.max_depth segments, bit for bit (segment
 *    index 0 is the texel's ray; hit rule, textures, environment, roulette and clamp as there).  lighting != 0: it is
 *    prt_radiance_lit's path under the context's lighting settings, pb = -1 on segment 0: emission met directly from the
 *    texel counts at weight 1 and no light sample is taken at the texel itself (unless texel_light is set: below).
 *  Texel value: rgb_sum[t] = the fp32 sum, from 0.0f in ascending sample order, of the q.samples path values, whatever the
 *    chunking (prt_set_param("bake_chunk", samples per chunk; 0 = by the ray budget of "radiance_chunk")).  A sum, as in
 *    the film: irradiance on the +n side is pi * sum / samples, the exit radiance of a Lambertian of albedo rho is
 *    rho * sum / samples.  Uncovered texels are 0.
 *  Gutter fill: `dilate` = N runs N passes.  A texel with coverage 0 whose 8-neighbourhood inside the map holds texels
 *    with coverage != 0 at the start of the pass gets the fp32 sum of those neighbours' values, in the order (-1,-1),
 *    (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0), (1,1) as (row, col), divided by their count as a float, and coverage 2.
 *  Coverage bytes: 0 = none, 1 = owned, 2 = filled.
 *  Refusals (PRT_ERR_INVALID, decided before anything is written; scene, film, statistics and histories untouched): no
 *    scene; a null target; an unknown kind or an index out of range; a bad size, or width * height * samples > 2^32 - 1;
 *    no UVs (uvs NULL and no binding, or a binding without UVs for that mesh); a UV that is not finite or of magnitude
 *    above 2^20; prt_radiance's own refusals for q.  After those a host-only context returns PRT_ERR_NO_DEVICE.
 *  Side effects: prt_radiance's: none.
 *  Cost: three small passes over faces and texels (one wave per face striding its clipped bounding box; one thread per
 *    texel; one block compacting the covered texels in ascending order), then per chunk of whole samples one ray kernel,
 *    the radiance query's rounds over covered texels x samples of the chunk, and one ordered sum.
 *  The texel's light sample (prt_bake_irradiance_opt with lighting != 0 and texel_light != 0, under a lighting mode that is
 *    not PRT_LIGHTING_OFF, with q.max_depth >= 1): the texel is treated as the Lambertian vertex it is, so direct light is
 *    sampled at the texel and what the texel's own ray meets is MIS-weighted.  For sample s of covered texel t with
 *    position p and normal n:
 *    Key: key = path_seed(t, first_sample + s, seed), the state BEFORE the texel's scatter draws (what the lit query's step
 *      calls `key`).  The light stream never advances the path's state: prt_bake_rays and every path are draw for draw
 *      what they are without the sample.
 *    Sample: the one a render's Lambertian vertex takes with albedo (1,1,1) and throughput (1,1,1): toward the environment
 *      if its draw of `key` says so, else toward the light set if it is not empty; position p, normal n,
 *      PrtSampling.clamp; the context's mode, source mask, selection and environment share: prt_sample_light's sample for
 *      a hit at p with normal n on a white Lambertian, its contrib clamped per component.
 *    Shadow ray: (p, w, tmax) is cast iff there is a sample and n.w > 0; it is occluded by prt_occluded's rule.
 *      e = the clamped contrib if unoccluded, else 0.
 *    The texel ray's pdf: ray_pb = (c > 0 ? c : 0) * 0.318309886183790672f with c = (nx dx + ny dy) + nz dz in fp32, d the
 *      texel's ray direction as prt_bake_rays returns it: the lit step's pdf of a Lambertian scatter.
 *    Sample value: fl(q + e) per component, q = prt_radiance_lit_pb's sample value for (o, d, rng_state, ray_pb) with
 *      q.max_depth segments.  e is added after q, not inside the query's light sum: the bake is then a composition of
 *      public functions (prt_bake_rays, prt_bake_light_samples, prt_occluded, prt_radiance_lit_pb) that can be redone bit
 *      for bit.  rgb_sum[t] = the fp32 sum of the values in ascending sample order from 0.0f, whatever the chunking.
 *    max_depth == 0: every output is zero and no sample is taken.  Mode OFF, lighting == 0 or texel_light == 0: no texel
 *      sample; the result is prt_bake_irradiance's, bit for bit.
 *    PrtBakeInfo.shadow_rays / shadow_occluded include the texels' shadow rays.
 *    Cost: per chunk one sample kernel, one more pass of the occlusion pipeline over the chunk's rays (a ray that is not
 *      cast rides along with tmax = 0, which never occludes) and one add kernel; no host wait beyond the lit bake's.
 * Not offered: the group (prt_group_*). */
#define PRT_BAKE_MESH 0u
#define PRT_BAKE_INSTANCE 1u
typedef struct PrtBakeTarget {
    uint32_t kind;      /* PRT_BAKE_MESH | PRT_BAKE_INSTANCE */
    uint32_t index;
    const float* uvs;   /* n_vertices * 2 floats, or NULL: the texture binding's */
    uint32_t width, height;
} PrtBakeTarget;
typedef struct PrtBakeInfo {
    uint64_t n_texels, n_covered, n_degenerate;
    uint64_t n_faces_skipped;  /* A2 == 0 (or a non-finite UV) */
    uint64_t n_filled;
    uint64_t rays, segments, shadow_rays, shadow_occluded;
    double device_ms;
} PrtBakeInfo;
/* Host outputs over the full map, each may be NULL: owner [H*W] (0xFFFFFFFF: none), bary [2*H*W] (b1, b2), position and
 * normal [3*H*W]; zero where uncovered.  info (may be NULL): the texel and face counts. */
int prt_bake_surface(PrtContext* ctx, const PrtBakeTarget* target, uint32_t* owner, float* bary, float* position,
                     float* normal, PrtBakeInfo* info);
/* The rays of sample `sample` of every texel (host, [3*H*W], [3*H*W], [H*W]; zero where uncovered): the function-level
 * view of the ray kernel, in the manner of prt_camera_rays_lens. */
int prt_bake_rays(PrtContext* ctx, const PrtBakeTarget* target, uint32_t seed, uint32_t sample, float* origins,
                  float* dirs, uint32_t* rng_state);
/* rgb_sum [3*H*W] floats and coverage [H*W] bytes on the host (coverage may be NULL).  Synchronous. */
int prt_bake_irradiance(PrtContext* ctx, const PrtBakeTarget* target, const PrtRadianceQuery* q, int lighting,
                        uint32_t dilate, float* rgb_sum, uint8_t* coverage, PrtBakeInfo* info);
/* The same with the two outputs as DEVICE pointers (the target's uvs stay a host array): enqueued on the context's stream,
 * with the waits the query has (and one for the covered count); complete in stream order on return. */
int prt_bake_irradiance_device(PrtContext* ctx, const PrtBakeTarget* target, const PrtRadianceQuery* q, int lighting,
                               uint32_t dilate, void* d_rgb_sum, void* d_coverage, PrtBakeInfo* info);
/* The same two calls with their options in a struct; prt_bake_irradiance[_device] are these with texel_light = 0.
 * texel_light != 0: the texel's light sample, above.  Refusals: a null options pointer, reserved != 0, then
 * prt_bake_irradiance's in their order, all decided without a device. */
typedef struct PrtBakeOptions {
    uint32_t lighting;     /* != 0: prt_radiance_lit's paths */
    uint32_t texel_light;  /* != 0: a light sample at the texel itself (needs lighting != 0 to have an effect) */
    uint32_t dilate;
    uint32_t reserved;     /* must be 0 */
} PrtBakeOptions;
int prt_bake_irradiance_opt(PrtContext* ctx, const PrtBakeTarget* target, const PrtRadianceQuery* q, const PrtBakeOptions* options,
                            float* rgb_sum, uint8_t* coverage, PrtBakeInfo* info);
int prt_bake_irradiance_opt_device(PrtContext* ctx, const PrtBakeTarget* target, const PrtRadianceQuery* q,
                                   const PrtBakeOptions* options, void* d_rgb_sum, void* d_coverage, PrtBakeInfo* info);
/* The light sample of sample `sample` of every texel: the function-level view of the light kernel, in the manner of
 * prt_bake_rays.  Host arrays over the full map, zero / none where uncovered, each may be NULL: dirs [3*H*W] (the sampled
 * direction w, also where n.w <= 0), tmax [H*W] (0: no shadow ray is cast), light [H*W] (the light-set index,
 * PRT_LIGHT_ENVIRONMENT, or 0xFFFFFFFF: no sample), contrib [3*H*W] (clamped, before visibility; 0 where no ray is cast),
 * ray_pb [H*W].  Under PRT_LIGHTING_OFF the sample is PRT_LIGHTING_NEE_MIS's, as prt_sample_light's is.  Refusals:
 * prt_bake_rays's. */
int prt_bake_light_samples(PrtContext* ctx, const PrtBakeTarget* target, uint32_t seed, uint32_t sample, float* dirs, float* tmax,
                           uint32_t* light, float* contrib, float* ray_pb);

/* ---- Bake statistics and adaptive sampling ---------------------------------------------------------
 * What "Film statistics and adaptive sampling" gives the film, for the lightmap: per-texel moments of the samples'
 * luminance, and a bake that goes on sampling only where the map is unconverged.  Every fp32 operation below is a single
 * one, rounded once, never contracted.
 *  Moments: for every sample value (r, g, b) the bake adds to texel t (under texel_light the value fl(q + e)), in ascending
 *    sample order:
 *        y = fl(fl(fl(0.2126f r) + fl(0.7152f g)) + fl(0.0722f b));   A = fl(A + y);   Q = fl(Q + fl(y y))
 *    from A = Q = 0.0f: the film's luminance and the film's moments.  count[t] (fp32, an exact integer) is the number of
 *    samples added.  rgb_sum[t] is prt_bake_irradiance's sum: from 0.0f in ascending sample order, whatever the chunking.
 *  Rule: prt_adaptive_unconverged(count, A, Q, threshold, noise_floor), the film's rule (csrc/prt_adaptive.h, written once
 *    and compiled for the device and for the host).  A texel is COVERED iff its coverage byte is 1; a texel that is not
 *    (coverage 0, or 2 in a map that went through the gutter fill) is converged.  The comparisons of the rule are false on
 *    a NaN, so a texel whose moments are NaN (count >= 2) is converged.
 *  Blocks: the map is cut into aligned 8 x 8 blocks of texels, block (by, bx) = rows 8 by .. 8 by + 7 and columns 8 bx ..
 *    8 bx + 7 clipped to the map, numbered row-major: block index by * ceil(W / 8) + bx.  A block is ACTIVE while any covered
 *    texel in it is unconverged: one wave per block, a ballot, no floating-point reduction, so the decision cannot depend on
 *    an order.  A block without covered texels is never active.
 *  Loop (prt_bake_irradiance_adaptive; prt_render_adaptive's).  Pass 0 gives every covered texel min_spp samples, indices
 *    q.first_sample .. q.first_sample + min_spp - 1, exactly as prt_bake_irradiance_opt would.  min_spp = 0 is refused: unlike
 *    the film, the call keeps no state between calls.  If max_spp == min_spp the call ends there: the uniform bake with
 *    statistics, without a selection and without a host wait beyond the bake's (that is how a caller gets the variance for
 *    the denoiser without adapting; blocks_converged and blocks_capped are then 0).  Otherwise, with added = min_spp:
 *      1. select: of the blocks active so far (at first: all blocks) those that are active by the rule now;
 *      2. list the covered texels of those blocks in ascending texel order and read both lengths back (one small wait);
 *      3. stop if the list is empty, or if added >= max_spp;
 *      4. add k = min(step_spp, max_spp - added) samples, indices q.first_sample + added .. + k - 1, to the listed texels
 *         only, by the bake's own per-chunk sequence over that list (the ray kernel, the radiance query unlit or lit, under
 *         texel_light the light sample, the occlusion pass and the add); added += k.
 *    A block that drops out never returns.  A texel that ends with count n therefore holds samples q.first_sample ..
 *    q.first_sample + n - 1, and since the bake is keyed by (texel, sample, seed) and sums in sample order, its rgb_sum
 *    equals that texel of prt_bake_irradiance_opt with samples = n, bit for bit: lit or unlit, with or without texel_light,
 *    whatever bake_chunk / radiance_chunk, tree builder or tunable.  q.samples is ignored: cfg decides, and every bound on
 *    the sample count is checked with max_spp in its place.  The chunk of a pass is bake_chunk, or else what radiance_chunk
 *    gives for the pass's sample count and list length.
 *  Outputs: rgb_sum [3*H*W], count, sum_y (A), sum_y2 (Q) [H*W], rgb_mean [3*H*W], coverage [H*W] bytes; each but rgb_sum
 *    may be NULL.  rgb_mean[t] = rgb_sum[t] / count[t] per component, one fp32 division; 0 where count is 0.  The
 *    options.dilate passes of the gutter fill run on the pair (coverage, rgb_mean) only, and `coverage` is the pair's
 *    (0 / 1 / 2).  The mean and not the sum is filled because neighbouring texels have different counts: a mean of sums
 *    over texels of 16 and of 256 samples is no quantity at all, while their means estimate the same kind of thing.  Sums,
 *    counts and moments are never dilated: a filled texel has count 0.  Irradiance on the +n side is pi * rgb_mean.
 *  Info: PrtBakeInfo as prt_bake_irradiance fills it, with rays = the sum of all counts.  PrtBakeAdaptiveInfo: below.
 *  Refusals (PRT_ERR_INVALID, decided before the device is touched, in this order): null options; options.reserved != 0;
 *    prt_bake_surface's for the target (no scene, null target, kind, index, size, UVs); null q; null cfg; a cfg.reserved
 *    word != 0; min_spp == 0; threshold or noise_floor negative or NaN; both 0; max_spp < min_spp; step_spp == 0 with max_spp
 *    > min_spp; max_spp > PRT_RADIANCE_MAX_SAMPLES; width * height * max_spp > 2^32 - 1; null rgb_sum.  After those a
 *    host-only context returns PRT_ERR_NO_DEVICE.  Side effects: the bake's: none.
 *  Cost: the bake's, plus per later pass one wave per previously active block, one block compacting the block list in its
 *    order, one block compacting the `active` bytes of the map, and the wait for two words; one division per texel at the
 *    end.  With info != NULL under texel_light each pass also waits once for its shadow-ray counters.
 *  Memory: the maps of a call lie behind the bake's own arrays in the context's bake buffer, the rays and the query's lists
 *    of a pass in scratch; from the second identical call on nothing is allocated (prt_device_memory_info).
 * Not offered: the group (prt_group_*); per-texel (rather than per-block) stopping; carrying moments across calls. */
typedef struct PrtBakeAdaptive {
    uint32_t min_spp, step_spp, max_spp;
    float threshold, noise_floor;
    uint32_t reserved[3];  /* must be 0 */
} PrtBakeAdaptive;
typedef struct PrtBakeAdaptiveInfo {
    uint32_t passes;           /* passes over a texel list that sampled (pass 0 is not one) */
    uint32_t blocks;           /* ceil(W / 8) * ceil(H / 8) */
    uint32_t blocks_converged; /* blocks the rule stopped (at any count, max_spp included; blocks without covered texels too) */
    uint32_t blocks_capped;    /* blocks still active when max_spp was reached */
    uint32_t min_texel_spp;    /* fewest / most samples a covered texel ends with (0 / 0 for a map without one) */
    uint32_t max_texel_spp;
    uint64_t texel_samples;    /* the sum of all counts */
} PrtBakeAdaptiveInfo;
/* Host outputs.  Synchronous. */
int prt_bake_irradiance_adaptive(PrtContext* ctx, const PrtBakeTarget* target, const PrtRadianceQuery* q, const PrtBakeOptions* options,
                                 const PrtBakeAdaptive* cfg, float* rgb_sum, float* count, float* sum_y, float* sum_y2, float* rgb_mean,
                                 uint8_t* coverage, PrtBakeInfo* info /* may be NULL */, PrtBakeAdaptiveInfo* adaptive_info /* may be NULL */);
/* The same with the six outputs as DEVICE pointers, as prt_bake_irradiance_opt_device has its two: enqueued on the
 * context's stream with the waits above; complete in stream order on return. */
int prt_bake_irradiance_adaptive_device(PrtContext* ctx, const PrtBakeTarget* target, const PrtRadianceQuery* q,
                                        const PrtBakeOptions* options, const PrtBakeAdaptive* cfg, void* d_rgb_sum, void* d_count,
                                        void* d_sum_y, void* d_sum_y2, void* d_rgb_mean, void* d_coverage, PrtBakeInfo* info,
                                        PrtBakeAdaptiveInfo* adaptive_info);
/* Function level, in the manner of prt_tile_select: steps 1 and 2 of the loop on caller-supplied host arrays, through the
 * kernels the loop launches.  coverage [H*W] bytes, count, sum_y, sum_y2 [H*W] floats.  prev: n_prev distinct block indices,
 * or NULL for blocks 0 .. n_prev - 1.  block_list (room for n_prev entries) receives the entries of prev that are active,
 * in prev's order, and 0xFFFFFFFF in the entries past them; texel_list (room for H*W entries) the covered texels of those
 * blocks in ascending order, and 0xFFFFFFFF past them; counts[0], counts[1] = the two lengths.  Needs a device and a
 * context, no scene; of the context only scratch memory is read or written.  Synchronous on return.
 * PRT_ERR_INVALID (checked on the host, in this order): a bad size; a null array (prev aside); n_prev above the block
 * count; a prev[i] >= the block count; threshold or noise_floor negative or NaN; both 0. */
int prt_bake_block_select(PrtContext* ctx, uint32_t W, uint32_t H, const uint8_t* coverage, const float* count, const float* sum_y,
                          const float* sum_y2, const uint32_t* prev /* may be NULL */, uint32_t n_prev, float threshold, float noise_floor,
                          uint32_t* block_list, uint32_t* texel_list, uint32_t* counts /* [2] */);
/* Pure host function, no context: per texel t < n, evaluated in double and rounded once,
 *     count[t] == 0: 0 (a texel without samples is an uncovered one: every covered texel of an adaptive bake has min_spp >= 1);
 *     else count[t] < 2 (or NaN): +inf;
 *     else sqrt(V / (count - 1)) / (m + noise_floor) with m = A / count, V = max(0, Q / count - m m): prt_film_noise_read's
 *     formula, IEEE 0 / 0 = NaN where a black texel meets noise_floor = 0.
 * PRT_ERR_INVALID: noise_floor negative or NaN; a null array with n != 0. */
int prt_bake_noise(uint64_t n, const float* count, const float* sum_y, const float* sum_y2, float noise_floor, float* rel_err);

/* ---- SH probes: radiance at points projected on spherical harmonics ------------------------------
 * For n_probes points: `samples` uniformly distributed directions per point are followed by the radiance query and the
 * results are projected, on the device and in a fixed order, onto the real spherical harmonics up to order 2: what a grid of
 * irradiance probes stores to light objects a lightmap cannot.  All arithmetic is fp32, one rounding per written
 * operation, no contraction.
 *  Ray (p, s) of probe p with position x_p: key = path_seed(p, first_sample + s, seed): the probe index stands where the
 *    pixel index stands in a render.  d = RandomUnitVector(key): the shade kernels' own rejection sampler (draws x, y, z in
 *    that order, accepted when 1e-8f < l2 <= 1, p / sqrt(l2)): uniform on the sphere, pdf 1 / (4 pi); d is used as
 *    returned, not normalised again.  o = x_p.  The state is the advanced one.
 *  Path: prt_radiance's path for (o, d, rng_state) with q.max_depth segments, bit for bit.  lighting != 0: prt_radiance_lit's
 *    path under the context's lighting settings, pb = -1 on segment 0.  The sample value L (rgb) is what the query returns
 *    for one sample: clamp, roulette, textures and environment apply as there.
 *  Basis, with (x, y, z) = d and k = 0 .. 8:
 *      Y0 = 0.282094792f                 Y1 = 0.488602512f*y               Y2 = 0.488602512f*z
 *      Y3 = 0.488602512f*x               Y4 = 1.092548431f*(x*y)           Y5 = 1.092548431f*(y*z)
 *      Y6 = 0.315391565f*(3.0f*(z*z) - 1.0f)    Y7 = 1.092548431f*(x*z)    Y8 = 0.546274215f*((x*x) - (y*y))
 *    `order` in {0, 1, 2} keeps the first (order + 1)^2 of them, so a lower order is a prefix of a higher one.  This is the
 *    usual real-SH ordering with z as the polar axis.  It has no relation to the environment image's +Y pole: the basis is
 *    a function of the world-space direction alone, and a caller who wants another frame rotates the direction.
 *  Coefficient sums: sh_sum[p][k][c] = the fp32 sum, from 0.0f in ascending sample order, of fl(L_c * Y_k(d)), whatever
 *    the chunking (prt_set_param("probe_chunk", samples per chunk; 0 = by the ray budget of "radiance_chunk")).  A sum, as
 *    in the film and the bake: the radiance coefficient is (4 pi / samples) * sum.  No floating-point atomics are used.
 *  Irradiance from coefficients (prt_sh_irradiance; a pure host function, no context): E_c(n) = the fp32 sum, from 0.0f
 *    over k ascending, of fl(fl(A_k * Y_k(n)) * coeff[k][c]) with A = 3.14159274f for k = 0, 2.09439516f for k = 1 .. 3 and
 *    0.785398185f for k = 4 .. 8.  Not clamped.
 *  Refusals (PRT_ERR_INVALID), decided without a device and in this order: no scene; null options, or null positions
 *    or output with n_probes != 0 (prt_radiance's rule for its arrays); reserved != 0; order > 2; a position that is not finite (the host form only: the device form takes positions as they
 *    are); n_probes * samples > 2^32 - 1; prt_radiance's own refusals for q.  Then PRT_ERR_NO_DEVICE on a host-only context.
 *    n_probes == 0 is OK and does nothing.  max_depth == 0 gives zeros.
 *  Side effects: prt_radiance's: none.  Film, statistics, feature sets, temporal history, light statistics and batch
 *    instance names are untouched; the next render is bit for bit what it would have been.
 *  Cost: per chunk of whole samples one ray kernel, the query's rounds over n_probes x chunk rays, and one projection kernel.
 *    No host wait beyond the query's own; with info one more per call.  From the second identical call on nothing is
 *    allocated.
 * Not offered: the group (prt_group_*); orders above 2; interpolation in a grid, which callers do on the coefficients. */
typedef struct PrtProbeShOptions {
    uint32_t order;        /* 0, 1 or 2: (order + 1)^2 coefficients per channel */
    uint32_t lighting;     /* != 0: prt_radiance_lit's paths */
    uint32_t reserved[2];  /* must be 0 */
} PrtProbeShOptions;
typedef struct PrtProbeShInfo {
    uint64_t n_probes, rays, segments, shadow_rays, shadow_occluded;
    double device_ms;
} PrtProbeShInfo;
/* Host arrays: positions [3*n_probes], sh_sum [n_probes][(order+1)^2][3].  Synchronous.  info may be NULL. */
int prt_probe_sh(PrtContext* ctx, const PrtProbeShOptions* options, const PrtRadianceQuery* q, uint32_t n_probes, const float* positions,
                 float* sh_sum, PrtProbeShInfo* info);
/* The same with positions and sh_sum as DEVICE pointers: enqueued on the context's stream, with the waits the query has;
 * complete in stream order on return.  The positions are taken as they are: a position that is not finite is not refused. */
int prt_probe_sh_device(PrtContext* ctx, const PrtProbeShOptions* options, const PrtRadianceQuery* q, uint32_t n_probes,
                        const void* d_positions, void* d_sh_sum, PrtProbeShInfo* info);
/* The rays of sample `sample` of every probe (host, [3*n_probes], [3*n_probes], [n_probes]): the function-level view of the
 * ray kernel, as prt_bake_rays is.  Refusals: no scene, a null array, a position that is not finite. */
int prt_probe_sh_rays(PrtContext* ctx, uint32_t n_probes, const float* positions, uint32_t seed, uint32_t sample, float* origins,
                      float* dirs, uint32_t* rng_state);
/* Host only, no context.  Y [n][(order+1)^2] = the basis at dirs [n][3], directions used as given.  E [n][3] from
 * coeffs [n][(order+1)^2][3] and normals [n][3] by the rule above.  PRT_ERR_INVALID: order > 2, or a null array with n != 0. */
int prt_sh_eval(uint32_t n, const float* dirs, uint32_t order, float* Y);
int prt_sh_irradiance(uint32_t n, const float* coeffs, const float* normals, uint32_t order, float* E);

/* ---- measurement ----------------------------------------------------------------------------- */
int prt_enable_timing(PrtContext* ctx, int on); /* HIP events around every kernel launch */
int prt_get_stats(PrtContext* ctx, PrtStats* out);
int prt_reset_stats(PrtContext* ctx);
/* Runs ONE sample with the instrumented traversal kernel (film untouched) and fills
 * bvh_node_visits / bvh_tri_tests / prim_tests / rays_per_depth in `out`. */
int prt_measure_traversal(PrtContext* ctx, uint32_t max_depth, uint32_t seed, uint32_t sample, PrtStats* out);
/* Diagnostic (wavefront.md:92-93 "material-coherent queues"): runs one batch (film untouched) and reports, per
 * bounce d, what the waves of the shade kernel find in their 64 ray slots by the material of the hit; out[16 * d + ...]:
 * [0] waves, [1] lanes with a ray, [2 + t] lanes of material type t (0 = miss, 1..4 = PRT_MAT_*), [8 + t] waves holding type t,
 * [14] sum over waves of distinct scattering types present, [15] waves with a scattering lane.  out: 16 * max_depth words. */
int prt_measure_shade_divergence(PrtContext* ctx, uint32_t max_depth, uint32_t seed, uint32_t sample, uint64_t* out);
int prt_bvh_info(PrtContext* ctx, PrtBvhInfo* out);
/* Rows per thread of the global spill area behind the LDS stacks of the spill-capable kernels, for a scene whose 4-wide
 * tree stacks at most max_stack4 entries (PrtBvhInfo.max_stack4) and whose binary tree has max_depth levels
 * (PrtBvhInfo.max_depth): the 4-wide instance keeps 27 entries in LDS, the binary one 31 of its max_depth - 1; one row of
 * slack; never fewer than 64.  A pure function (no context); the library sizes the area with it per scene. */
uint32_t prt_spill_rows(uint32_t max_stack4, uint32_t max_depth);
int prt_kernel_occupancy(PrtContext* ctx, PrtOccupancy* out);
/* Name of the traversal kernel instance the current scene and tunables select (what prt_render launches and what
 * prt_kernel_occupancy describes): "lean8_5waves", "deep15_4waves", "inst12_4waves", "wide11_5waves", "bvh4", "bvh2".
 * Written NUL-terminated into name[capacity].  The same decision function drives the launch (csrc/prt_kernels.hip). */
int prt_kernel_instance(PrtContext* ctx, char* name, uint32_t capacity);
/* Name of the shade kernel instance that the context's last batch launched (the last bounce's, if a batch's bounces differ:
 * compact primary rays shade bounce 0 with an instance of their own), with its template arguments as the compiler's symbol
 * table spells them: "k_shade<0, true, false, false, false>", "k_shade_env<false, true>", "k_shade_nee_mesh<true, false>",
 * "k_shade_tex<INST, ABVH, ENV>", "k_shade_nee_tex<INST, ABVH, MESHL, ENV>", ...  The string is written by the launch macro
 * itself from the template arguments it launches with (csrc/prt_kernels.hip), so it cannot differ from what ran.  Empty
 * before the first batch and after a batch on the path-kernel route, which launches no shade kernel.  Read-only; written
 * NUL-terminated into name[capacity]. */
int prt_shade_instance(PrtContext* ctx, char* name, uint32_t capacity);
/* What the context's last batch launched, stage by stage: the raygen instance, the shade instance of bounce 0 when it differs
 * from the later bounces' (compact primary rays; empty otherwise), the shade instance of the later bounces (what
 * prt_shade_instance reports) and the accumulate instance, each recorded where it is launched.  A stage that launched nothing
 * reports the empty string: raygen and both shades on the path-kernel route, every stage before the first batch.
 * prt_instance_name enumerates the instance lists of csrc/prt_route.h (index 0, 1, ...; PRT_STAGE_SHADE0 walks the shade list)
 * and returns PRT_ERR_INVALID past the end, so a test can hold the set of names it saw to the whole list. */
enum { PRT_STAGE_RAYGEN = 0, PRT_STAGE_SHADE0 = 1, PRT_STAGE_SHADE = 2, PRT_STAGE_ACCUMULATE = 3 };
int prt_batch_instance(PrtContext* ctx, uint32_t stage, char* name, uint32_t capacity);
int prt_instance_name(uint32_t stage, uint32_t index, char* name, uint32_t capacity);
/* The last-segment route of the context's last batch (the "last_segment" tunable as the batch's plan took it: 0 = every stored
 * ray was walked and shaded, 1 = last segments that the analytic scan decides ended in their producer, 2 = and the last walk
 * was the seeded any-hit walk),
 * and, if front_rays is not NULL, the number of rays that batch handed to its last tree walk (segment max_depth - 1; 0 after
 * a batch on the path-kernel route).  Reading the count waits for the context's stream. */
int prt_last_segment(PrtContext* ctx, uint32_t* active, uint32_t* front_rays);
/* The primary stage of a still camera (DESIGN.md section 2 "One walk per pixel"): without jitter and without a lens what a
 * batch computes before its first shade launch (k_raygen, the bounce-0 walk, k_primary_hit) does not depend on the sample
 * index or the seed, so the context keeps it and a batch with the same camera, scene, film, batch size, max_depth and route
 * starts at its first shade launch.  *active: 1 if the context's last batch did, 0 if it rebuilt the stage (or took another
 * route); *reused_batches (may be NULL): the batches that did since the context was created.  The film never depends on it;
 * prt_set_param("primary_reuse", 0) makes every batch rebuild the stage. */
int prt_primary_reuse(PrtContext* ctx, uint32_t* active, uint32_t* reused_batches);
/* Copies the built BVH out (host arrays): nodes n_nodes*16 floats (layout: csrc/bvh.h), tris
 * n_triangles*12 floats in leaf order.  Either pointer may be NULL.  Works on host-only contexts. */
int prt_bvh_read(PrtContext* ctx, float* nodes, float* tris);
/* The 4-wide tree: n_nodes4*32 floats (layout: csrc/bvh.h). */
int prt_bvh_read4(PrtContext* ctx, float* nodes4);
/* The compressed 8-wide tree: n_nodes8*20 uint32 (layout: csrc/bvh.h). */
int prt_bvh_read8(PrtContext* ctx, uint32_t* nodes8);
/* Selects the traversal kernel variant (0 = default). For A/B benchmarking only. */
int prt_set_variant(PrtContext* ctx, int variant);
/* Tunables (A/B benchmarking; defaults = measured best on C3): "variant", "grid_blocks", "chunk", "refill_min",
 * "exit_max", "tri_min", "wide" (2 = compressed 8-wide tree, default; 1 = 4-wide; 0 = binary), "stack_lds" (kernel
 * instance), "xcd_affinity" (4-wide / binary kernels), "tail" (64-ray granules per resident wave handed out singly at
 * the end of the ray buffer), "steal" (idle lanes a draining wave needs before they take over pending subtrees; 0 = off),
 * "exact_grids" (0/1/2: k_shade grids from the ray counts read back during the traversal: never / big batches / always),
 * "fuse", "prim_bvh" (0: linear scan over the analytic primitives as in the reference), "measure_spp", "stack_cap"
 * (test hook), "gpu_build" (the next prt_set_scene builds the 8-wide tree(s) on the device, placed copies and the top level
 * included: 1 = PLOC + SAH top + optimal collapse, ~20 ms for 870 k triangles, traverses within 2-3 % of the host tree;
 * 2 = Morton octree, ~3 ms, ~20 % slower to traverse), "node_stride" (before prt_set_scene: 5 = 8-wide nodes packed at
 * 80 B, 8 = one node per 128-B line, 0 = by tree size, default), "pad_log2" (before prt_set_scene: the culling pad is 2^-n of
 * the coordinates' magnitude, default 18; A/B only), "last_segment" (the last segment of a path in scenes without emissive
 * triangles, prt_last_segment: 0 = walked and shaded like any other; 1 = it ends in the shade launch that produces it where
 * the analytic scan alone decides what the film gets; 2, default = 1, and the rays still walked get the any-hit walk seeded
 * with their analytic hit), "primary_reuse" (1, default: a still camera's primary stage is kept across batches and calls,
 * prt_primary_reuse; 0 = every batch rebuilds it; setting ANY tunable makes the next batch rebuild it), "path_id_order" (how a
 * batch of compact primary rays with at least 8 samples numbers its paths: 1, default = pixel * samples + sample, so the waves
 * of the shade launches, which hold runs of one pixel's samples, store their path results next to each other; 0 = sample *
 * pixels + pixel, as every other batch; A/B), "denoise_lds" (which iterations of the denoiser stage their block's footprint in LDS: 0 = none, 1, default = step 1,
 * 2 = steps 1 and 2; A/B), "feature_chunk" / "radiance_chunk" (samples per chunk of the sampled feature pass / of prt_radiance; 0, default = by
 * the ray budget).  Results never depend on a tunable.  Unknown names / bad values
 * return PRT_ERR_INVALID. */
int prt_set_param(PrtContext* ctx, const char* name, int value);

/* ---- several GPUs of one node behind one Renderer (the reference is single-GPU:
 *      cudaSetDevice(0), src/backend/optix/renderer.cpp:217) ------------------------------------------
 * A group owns one context per entry of device_ids and drives each from its own host thread.  The image is tiled over
 * the contexts (prt_set_film(w, h, rank, n): 8x8 tiles dealt round-robin), the scene is built once and cloned, every
 * rank renders all samples of its tiles (RNG keyed by global pixel and sample: the image does not depend on n), and ONE
 * gather of the per-tile radiance brings the payloads to rank 0's device, which un-tiles them into the Film layout:
 *   transport "rccl": ncclSend / ncclRecv inside one group call over xGMI (librccl.so, loaded on demand; needs distinct devices)
 *   transport "peer": hipMemcpyPeerAsync into rank 0's buffer (also the fallback, and what several ranks on ONE device use)
 * PRT_GROUP_TRANSPORT=rccl|peer overrides the choice (rccl with a single rank runs a 1-rank ncclAllGather: a hardware
 * smoke test of the RCCL path).  The same device may appear several times in device_ids (rehearsal / tests on one GPU).
 * All calls are synchronous and are made from one caller thread.
 * prt_group_create ALWAYS stores a group in *out, also when it returns an error (so that prt_group_last_error can say why):
 * the caller destroys it with prt_group_destroy in either case.  The "rccl" transport with n > 1 distinct devices has not
 * run on hardware yet (no multi-GPU box was available to the builder; prt_group_transport says which one a group uses). */
typedef struct PrtGroup PrtGroup;
int prt_group_create(const int* device_ids, uint32_t n, PrtGroup** out);
void prt_group_destroy(PrtGroup* g);
const char* prt_group_last_error(const PrtGroup* g);
uint32_t prt_group_size(const PrtGroup* g);
const char* prt_group_transport(const PrtGroup* g);          /* "rccl" | "peer" | "none" (one rank) */
PrtContext* prt_group_context(PrtGroup* g, uint32_t rank);   /* per-rank tunables / stats; owned by the group */
int prt_group_set_scene(PrtGroup* g, const PrtSceneDesc* scene);   /* built on rank 0, cloned to the others */
/* prt_refit_meshes on every rank (each refits the tree on its own device, in parallel; the meshes are read by all ranks). */
int prt_group_refit_meshes(PrtGroup* g, const PrtMesh* meshes, uint32_t n_meshes);
/* prt_set_instance_transforms on every rank (each updates the top level on its own device, in parallel). */
int prt_group_set_instance_transforms(PrtGroup* g, const PrtInstance* instances, uint32_t n, uint32_t mode);
int prt_group_set_camera(PrtGroup* g, const PrtCameraDesc* cam);
int prt_group_set_film(PrtGroup* g, uint32_t width, uint32_t height);
int prt_group_film_clear(PrtGroup* g);
int prt_group_set_sampling(PrtGroup* g, const PrtSampling* s);
int prt_group_set_lens(PrtGroup* g, const PrtLens* lens);
int prt_group_set_feature_trace(PrtGroup* g, const PrtFeatureTrace* ft); /* every rank; prt_group_film_denoise: rank 0's guide set */
int prt_group_set_feature_sampling(PrtGroup* g, const PrtFeatureSampling* fs); /* every rank; prt_group_film_denoise: rank 0's sampled set */
int prt_group_set_samples_in_flight(PrtGroup* g, uint32_t n);
int prt_group_set_lighting(PrtGroup* g, const PrtLighting* l);
int prt_group_set_light_sources(PrtGroup* g, uint32_t mask);
int prt_group_set_light_selection(PrtGroup* g, const PrtLightSelection* sel);
int prt_group_set_environment(PrtGroup* g, const PrtEnvironment* env);   /* on every rank */
int prt_group_set_textures(PrtGroup* g, const PrtTextureSet* set);     /* on every rank, after prt_group_set_scene */
/* shadow-ray counts summed over the ranks; n_lights / n_emitters_unsampled as rank 0 has them */
int prt_group_get_light_stats(PrtGroup* g, PrtLightStats* out);
int prt_group_set_param(PrtGroup* g, const char* name, int value);
/* Renderer::ProgressiveRender x spp on every rank's tiles, then the gather + un-tiling on rank 0's device. */
int prt_group_render(PrtGroup* g, uint32_t spp, uint32_t max_depth, uint32_t seed, uint32_t first_sample);
/* prt_set_film_statistics on every rank; prt_render_adaptive on every rank's own tiles in parallel (each rank runs its own
 * loop: tiles are decided one by one), then the gather.  Info: sums over the ranks; passes = the most any rank ran;
 * min_tile_spp / max_tile_spp over the ranks that own tiles.  prt_group_film_read's weights are the sample-count map. */
int prt_group_set_film_statistics(PrtGroup* g, int on);
int prt_group_render_adaptive(PrtGroup* g, const PrtAdaptive* cfg, uint32_t max_depth, uint32_t seed, uint32_t first_sample,
                              PrtAdaptiveInfo* out);
/* prt_film_denoise for the gathered film: the ranks' moments are summed on the host (a pixel its rank does not own holds 0,
 * so the sum is exact), mean and variance are computed on the host by the lines prt_film_denoise's prepare kernel
 * compiles, and rank 0 renders the features and runs the filter: the result equals the single context's bit for bit. */
int prt_group_film_denoise(PrtGroup* g, const PrtDenoise* cfg, float* rgb_out, float* var_out);
/* Whole film (all ranks' tiles) to host / tonemapped to host RGBA8, as prt_film_read / prt_film_display. */
int prt_group_film_read(PrtGroup* g, float* rgb_sum, float* weight);
int prt_group_film_display(PrtGroup* g, float exposure, float gamma, uint8_t* rgba8);
/* Ray counters summed over the ranks; the *_ms fields are the maxima over the ranks. */
int prt_group_get_stats(PrtGroup* g, PrtStats* out);

/* ---- host-side data formats either side of the path ------------------------------------------- */
/* PLY ingest with the subset the reference's Mesh asks tinyply for (src/core/mesh.cpp:79-97,113-144):
 * vertex x,y,z (+ optional nx,ny,nz), face vertex_indices list; ascii and binary_little_endian.
 * Missing normals are computed (area-weighted); polygons are fan-triangulated. */
typedef struct PrtMeshData PrtMeshData;
int prt_mesh_load_ply(const char* path, PrtMeshData** out, char* err, size_t err_len);
int prt_mesh_create(const float* positions, const float* normals, uint32_t n_vertices, const uint32_t* indices,
                    uint32_t n_triangles, PrtMeshData** out);
void prt_mesh_free(PrtMeshData* m);
uint32_t prt_mesh_vertex_count(const PrtMeshData* m);
uint32_t prt_mesh_triangle_count(const PrtMeshData* m);
const float* prt_mesh_positions(const PrtMeshData* m);
const float* prt_mesh_normals(const PrtMeshData* m);
const uint32_t* prt_mesh_indices(const PrtMeshData* m);
int prt_mesh_had_normals(const PrtMeshData* m);
/* Deterministic longest-edge bisection up to >= target_triangles (SURVEY §8d synthetic inputs). */
int prt_mesh_refine(PrtMeshData* m, uint32_t target_triangles);
/* positions = mat * positions, normals = normalize(mat3(inverse-transpose) * normals). */
int prt_mesh_transform(PrtMeshData* m, const float mat[16], const float inv[16]);
/* dst keeps (gets) UVs only if both sides have them or dst is empty; otherwise the result has none (never an error). */
int prt_mesh_append(PrtMeshData* dst, const PrtMeshData* src);
/* Per-vertex UVs (n_vertices*2 floats, NULL: none): the PLY properties s/t, u/v or texture_u/texture_v of any scalar
 * type.  prt_mesh_refine gives a new vertex (uv_a + uv_b) * 0.5f; prt_mesh_transform leaves UVs alone. */
const float* prt_mesh_uvs(const PrtMeshData* m);
int prt_mesh_had_uvs(const PrtMeshData* m);
int prt_mesh_set_uvs(PrtMeshData* m, const float* uvs); /* n_vertices*2 floats, copied; NULL drops them */

/* Scene presets (src/core/scene.cpp:62-350) flattened into materials + primitives.
 * Pass NULL arrays to query counts. */
int prt_scene_preset(int preset, PrtMaterial* materials, uint32_t* n_materials, PrtPrimitive* primitives,
                     uint32_t* n_primitives);
/* Scene::MakeTransform (src/core/scene.cpp:9-17): T * eulerAngleXYZ(radians(deg)) * S and its inverse. */
void prt_make_transform(const float scale[3], const float euler_deg[3], const float translation[3], float mat[16],
                        float inv[16]);

/* Offline framebuffer dump (stands in for the GLFW/OpenGL viewer, src/main.cpp:504-527). */
int prt_write_ppm(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);
int prt_write_pfm(const char* path, const float* rgb, uint32_t width, uint32_t height);
/* Colour PFM ("PF", either byte order; stored bottom-to-top, returned top-to-bottom, width*height*3 floats to be released
 * with prt_image_free).  Greyscale files, bad headers, short bodies, sizes beyond 2^28 pixels: PRT_ERR_IO. */
int prt_read_pfm(const char* path, float** rgb, uint32_t* width, uint32_t* height);
void prt_image_free(float* rgb);

#ifdef __cplusplus
}
#endif
#endif /* PRT_H */

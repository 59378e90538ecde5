// prt_scene.cpp — the scene compiler (prt_scene.h): validates a PrtSceneDesc and turns it into the host arrays the kernels
// walk.  No HIP in here; the device-side tree builder arrives as a callable (PrtSceneOptions::device_build).
#include "prt_scene.h"

#include <algorithm>
#include <array>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <utility>

// include/prt.h: the 4-wide spill-capable instance keeps 27 entries in LDS (k_traverse4_persistent<27, 5, 1>), the binary one
// 31 of its max_depth - 1 pushes (k_traverse_persistent<31, 5, 1>); row r of the area holds stack entry STACK_L + r
extern "C" uint32_t prt_spill_rows(uint32_t max_stack4, uint32_t max_depth) {
    const uint32_t rows4 = max_stack4 > 27u ? max_stack4 - 27u : 0u;
    const uint32_t rows2 = max_depth > 32u ? max_depth - 32u : 0u;
    return std::max(64u, std::max(rows4, rows2) + 1u);
}

namespace {

constexpr uint32_t kMaxLeaf = 3;  // the compressed 8-wide node encodes at most 3 triangles per leaf (bvh.h)
constexpr uint32_t kMaxStack = 63;  // LDS stack entries per lane: 31 (5 blocks/CU) or 63 (2 blocks/CU)
constexpr int kHostBuildFailed = -1001;  // build_tree: the host builder refused (the caller words the message)

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

int fail(std::string* err, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    *err = buf;
    return PRT_ERR_INVALID;
}

void to_dev_mat(const float* m16, float* m12) {
    for (int col = 0; col < 4; ++col)
        for (int r = 0; r < 3; ++r) m12[col * 3 + r] = m16[col * 4 + r];
}

// g = transpose(M3) * M3 of a column-major mat4's upper 3x3, in double; true if it is s^2 * I (s^2 = g[0][0] = *s2_out)
bool gram_is_uniform_scale(const float* M, double* s2_out) {
    double g[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            g[a][b] = (double)M[4 * a] * M[4 * b] + (double)M[4 * a + 1] * M[4 * b + 1] + (double)M[4 * a + 2] * M[4 * b + 2];
    const double s2 = g[0][0];
    bool ok = s2 > 1e-20 && std::isfinite(s2);
    for (int a = 0; a < 3 && ok; ++a)
        for (int b = 0; b < 3; ++b)
            if (std::fabs(g[a][b] - (a == b ? s2 : 0.0)) > 1e-4 * s2) ok = false;
    *s2_out = s2;
    return ok;
}

bool affine_bottom_row(const float* M) { return M[3] == 0.0f && M[7] == 0.0f && M[11] == 0.0f && M[15] == 1.0f; }

// Rotation + uniform scale + translation with inv = inverse(mat) (column-major mat4s): transpose(M3) * M3 = s^2 * I, bottom row
// (0, 0, 0, 1), inv * mat = I.  Only for such transforms is the reference's local ray (primitive.cpp:29-30) a ray transform.
// *s2_out = s^2.
bool is_similarity(const float* M, const float* inv, double* s2_out) {
    bool ok = gram_is_uniform_scale(M, s2_out);
    for (int r = 0; r < 4 && ok; ++r)
        for (int cc = 0; cc < 4; ++cc) {
            // relative to the terms' magnitude: the translation column of inv * mat sums terms of size |t| / s, each known
            // to fp32 only (a copy at scale 2^-10 placed 1e4 away: terms of 1e7, their rounding alone is 1); for the
            // rotation part the terms are below 1 and the bound is the absolute 1e-3 it always was, which is also the floor
            double acc = 0.0, mag = 1.0;
            for (int kk = 0; kk < 4; ++kk) {
                const double term = (double)inv[4 * kk + r] * (double)M[4 * cc + kk];
                acc += term;
                mag = std::max(mag, std::fabs(term));
            }
            // (translation column: 1e-5 of the largest term, 170 x the rounding of an fp32 term)
            if (!(std::fabs(acc - (r == cc ? 1.0 : 0.0)) <= (cc == 3 ? std::max(1e-3, 1e-5 * mag) : 1e-3 * mag))) ok = false;
        }
    return ok && affine_bottom_row(M);
}

// The light set of a scene (include/prt.h PrtLighting): emissive analytic primitives with positive mean emission and a
// rotation + uniform scale + translation transform with inv = inverse(mat) (the test compile_instances applies to placed
// copies: only then is the surface the reference intersects, primitive.cpp:29-30, the one sampled here).  pmf ~ emitting
// area x mean(rgb), computed in double.  Every other emissive primitive (mesh and placed triangles, other transforms)
// counts in n_emitters_unsampled.
void build_light_table(PrtHostScene* c, const PrtSceneDesc* s) {
    c->lights.clear();
    c->prim_light.assign(s->n_primitives, 0xFFFFFFFFu);
    c->n_emitters_unsampled = 0;
    auto emissive = [&](uint32_t m) { return m < s->n_materials && s->materials[m].type == PRT_MAT_EMISSIVE; };
    std::vector<double> power;
    for (uint32_t i = 0; i < s->n_primitives; ++i) {
        const PrtPrimitive& p = s->primitives[i];
        if (!emissive(p.material_id)) continue;
        const float* M = p.mat;
        double s2 = 0.0;
        if (!is_similarity(p.mat, p.inv, &s2)) {
            ++c->n_emitters_unsampled;
            continue;
        }
        const float* rgb = s->materials[p.material_id].rgb;
        const double mean = ((double)rgb[0] + (double)rgb[1] + (double)rgb[2]) / 3.0;
        const bool quad = p.shape_type == PRT_SHAPE_QUAD;
        const double w = p.shape_param[0], h = p.shape_param[1];
        const double area = quad ? std::fabs(w * h) * s2 : 4.0 * M_PI * w * w * s2;
        const double pw = (quad ? 2.0 * area : area) * mean;  // a quad emits from both faces
        if (!(pw > 0.0) || !std::isfinite(pw)) continue;      // emits nothing: not a light, nothing unsampled either
        float rec[4 * PRT_LIGHT_F4] = {};
        rec[0] = M[12];
        rec[1] = M[13];
        rec[2] = M[14];
        rec[3] = quad ? (float)area : (float)(std::fabs(w) * std::sqrt(s2));
        const double nx = (double)M[1] * M[10] - (double)M[2] * M[9], ny = (double)M[2] * M[8] - (double)M[0] * M[10],
                     nz = (double)M[0] * M[9] - (double)M[1] * M[8];
        const double nl = std::sqrt(nx * nx + ny * ny + nz * nz);
        for (int a = 0; a < 3; ++a) {
            rec[4 + a] = quad ? (float)(w * M[a]) : 0.0f;
            rec[8 + a] = quad ? (float)(h * M[8 + a]) : 0.0f;
        }
        if (quad) {
            rec[12] = (float)(nx / nl);
            rec[13] = (float)(ny / nl);
            rec[14] = (float)(nz / nl);
        }
        const uint32_t kind = quad ? 1u : 0u;
        memcpy(&rec[15], &kind, 4);
        rec[16] = rgb[0];
        rec[17] = rgb[1];
        rec[18] = rgb[2];
        memcpy(&rec[19], &i, 4);
        c->prim_light[i] = (uint32_t)power.size();
        power.push_back(pw);
        c->lights.insert(c->lights.end(), rec, rec + 4 * PRT_LIGHT_F4);
    }
    double total = 0.0;
    for (double pw : power) total += pw;
    double acc = 0.0;
    for (size_t l = 0; l < power.size(); ++l) {
        acc += power[l];
        c->lights[4 * PRT_LIGHT_F4 * l + 7] = (float)(power[l] / total);                                 // pmf
        c->lights[4 * PRT_LIGHT_F4 * l + 11] = l + 1 == power.size() ? 1.0f : (float)(acc / total);  // cdf
    }
    c->light_power = power;
    const uint32_t n_not_similar = c->n_emitters_unsampled;
    c->mesh_emissive = false;  // (by material alone: an emissive mesh without triangles counts, which only keeps a route off)
    for (uint32_t m = 0; m < s->n_meshes; ++m)
        if (emissive(s->meshes[m].material_id)) {
            c->n_emitters_unsampled += s->meshes[m].n_triangles;
            c->mesh_emissive = true;
        }
    for (uint32_t i = 0; i < s->n_instances; ++i) {
        const PrtInstance& pi = s->instances[i];
        if (!emissive(pi.material_id)) continue;
        c->mesh_emissive = true;
        if (pi.mesh < s->n_instanced_meshes) c->n_emitters_unsampled += s->instanced_meshes[pi.mesh].n_triangles;
    }
    c->ml_tris_counted = c->n_emitters_unsampled - n_not_similar;
}

// Triangle / normal records of n triangles in leaf order: {P0, prim_base + input index}, {P1, material}, {P2, -}.  norms /
// nrm_rec and tri_mat may be null (no normal records; word 7 stays as it is).
void pack_records(const std::vector<uint32_t>& order, const float* verts, const float* norms, uint32_t n, uint32_t prim_base,
                  const uint32_t* tri_mat, float* tri_rec, float* nrm_rec) {
    for (size_t slot = 0; slot < (size_t)n; ++slot) {
        const uint32_t t = order[slot];
        float* r = &tri_rec[12 * slot];
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) {
                r[4 * v + a] = verts[9 * (size_t)t + 3 * v + a];
                if (nrm_rec) nrm_rec[12 * slot + 4 * v + a] = norms[9 * (size_t)t + 3 * v + a];
            }
        const uint32_t prim = prim_base + t;
        memcpy(&r[3], &prim, 4);
        if (tri_mat) memcpy(&r[7], &tri_mat[t], 4);
    }
}

// A box as the builders take it: one degenerate "triangle" that spans it
void box_triangle(const float* mn, const float* mx, float* tri) {
    const float t9[9] = {mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], mn[0], mx[1], mn[2]};
    memcpy(tri, t9, sizeof(t9));
}

// What build_tree builds a tree over: n triangles as 9 floats each (+ normals, + a material per triangle, both may be null)
struct TreeInput {
    const float* verts;
    const float* norms;
    const uint32_t* tri_mat;
    uint32_t n, n_prims;
};

// One tree: the device builder first where there is one (opt.device_build; records come back in tri_rec / nrm_rec and
// *on_device is set), else the host builder (the caller packs the records from out->order).  A valid mesh is never
// refused because the DEVICE builder could not cope with it (a tree deeper than device_depth_limit allows, or more
// clustering passes than its guard allows: degenerate inputs such as thousands of coincident triangles): the host
// builder, with its forced median splits, takes over.  The one exception, host_fallback = false (the top-level tree):
// kPrtDeviceBuildGaveUp goes back to the caller.  Returns PRT_OK, kHostBuildFailed, or the device builder's error.
int build_tree(const PrtSceneOptions& opt, const TreeInput& in, float leaf_cost, bool keep, uint32_t device_depth_limit, bool host_fallback,
               int host_threads, BvhBuild* out, float* tri_rec, float* nrm_rec, bool* on_device, double* gpu_ms, std::string* err) {
    *on_device = false;
    if (opt.device_build && in.n > 0) {
        // host copies for the read-back entry points (prt_bvh_read / prt_bvh_read8) and for scenes whose node array is put
        // together on the host (placed copies); the binary and 4-wide trees of the A/B kernels are not built in this mode
        *out = BvhBuild();
        out->max_leaf = 3;
        const int brc = opt.device_build(in.verts, in.norms, in.tri_mat, in.n, in.n_prims, leaf_cost, keep, out->nodes8, out->depth8, tri_rec,
                                         nrm_rec, gpu_ms, err);
        if (brc && brc != kPrtDeviceBuildGaveUp) return brc;
        if (!brc && out->depth8 <= device_depth_limit) {
            *on_device = true;
            return PRT_OK;
        }
        if (!host_fallback) return kPrtDeviceBuildGaveUp;
        *out = BvhBuild();
        std::fill_n(tri_rec, 12 * (size_t)in.n, 0.0f);  // (a tree that came back too deep came back with its records)
        if (nrm_rec) std::fill_n(nrm_rec, 12 * (size_t)in.n, 0.0f);
    }
    return bvh_build(in.verts, in.n, kMaxLeaf, host_threads, kMaxStack, out) ? PRT_OK : kHostBuildFailed;
}

// What the steps of prt_compile_scene hand on to each other
struct Work {
    std::vector<float> verts, norms;  // the world-space meshes, 9 floats per triangle
    std::vector<uint32_t> tri_mat;
    uint32_t n_world = 0;             // their triangles
    bool world_on_device = false;     // their tree came from the device builder
    Clock::time_point t_build0;
    double host_build_ms = 0.0;       // wall time of the tree builds (reported when the host built them)
    uint32_t depth8 = 0;              // levels of the 8-wide tree (two-level scenes: top level + deepest mesh tree)
};

// ---- the light set with emissive triangles (PrtMeshLights, prt_scene.h; contract: include/prt.h "Triangle lights") ----

// Candidate records of n triangles given as fp32 world vertices (9 floats each), appended to ml.records / ml.power at
// candidate `at`: {v0 | A}, {e1 | pmf}, {e2 | -}, {n_g | kind 2}, {Le | global primitive index}.  e1, e2, A, n_g in double,
// stored as fp32; power 2 A mean(rgb), 0 where that is not a positive finite number.
void write_tri_candidates(PrtMeshLights& ml, size_t at, const float* verts, uint32_t n, const float* rgb, uint32_t prim_first) {
    const double mean = ((double)rgb[0] + (double)rgb[1] + (double)rgb[2]) / 3.0;
    for (uint32_t t = 0; t < n; ++t) {
        const float* v = &verts[9 * (size_t)t];
        float* rec = &ml.records[4 * PRT_LIGHT_F4 * (at + t)];
        std::fill_n(rec, 4 * PRT_LIGHT_F4, 0.0f);
        double e1[3], e2[3];
        for (int a = 0; a < 3; ++a) {
            ml.box[6 * (at + t) + a] = std::min(v[a], std::min(v[3 + a], v[6 + a]));
            ml.box[6 * (at + t) + 3 + a] = std::max(v[a], std::max(v[3 + a], v[6 + a]));
            e1[a] = (double)v[3 + a] - (double)v[a];
            e2[a] = (double)v[6 + a] - (double)v[a];
            rec[a] = v[a];
            rec[4 + a] = (float)e1[a];
            rec[8 + a] = (float)e2[a];
        }
        const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        const double cl = std::sqrt(cx * cx + cy * cy + cz * cz);
        const double area = 0.5 * cl;
        rec[3] = (float)area;
        if (cl > 0.0 && std::isfinite(cl)) {
            rec[12] = (float)(cx / cl);
            rec[13] = (float)(cy / cl);
            rec[14] = (float)(cz / cl);
        }
        const uint32_t kind = 2u, prim = prim_first + t;
        memcpy(&rec[15], &kind, 4);
        rec[16] = rgb[0];
        rec[17] = rgb[1];
        rec[18] = rgb[2];
        memcpy(&rec[19], &prim, 4);
        const double pw = 2.0 * area * mean;
        ml.power[at + t] = (pw > 0.0 && std::isfinite(pw)) ? pw : 0.0;
    }
}

// ---- a light's world box (include/prt.h "Clustered light selection") ----
float round_down(double d) {
    const float f = (float)d;
    return (double)f > d ? std::nextafterf(f, -INFINITY) : f;
}
float round_up(double d) {
    const float f = (float)d;
    return (double)f < d ? std::nextafterf(f, INFINITY) : f;
}

// World box of an analytic light from its record: the quad's corners c +- u/2 +- v/2, the sphere's c +- R; in double,
// rounded outward.
void analytic_light_box(const float* rec, float* box) {
    uint32_t kind = 0;
    memcpy(&kind, &rec[15], 4);
    for (int a = 0; a < 3; ++a) {
        const double c = rec[a];
        const double h = kind == 1u ? 0.5 * std::fabs((double)rec[4 + a]) + 0.5 * std::fabs((double)rec[8 + a]) : std::fabs((double)rec[3]);
        box[a] = round_down(c - h);
        box[3 + a] = round_up(c + h);
    }
}

// Thresholds T_i = floor(C_i / C_n * 2^32 + 0.5) of the running power sums C_i (double, candidate order), the pmf
// (T_i - T_{i-1}) / 2^32 into every record, the light set proper, the search array and its bucket table.
void finish_mesh_lights(PrtHostScene& hs, uint32_t n_not_similar) {
    PrtMeshLights& ml = hs.ml;
    const size_t n = ml.power.size();
    ml.thr.clear();
    ml.bucket.clear();
    ml.visible.clear();
    ml.width.clear();
    ml.cand_visible.assign(n, 0xFFFFFFFFu);
    ml.n_search = 0;
    ml.bucket_shift = 32;
    ml.n_emitters_unsampled = n_not_similar;
    double total = 0.0;
    for (double pw : ml.power) total += pw;  // (the order of the running sum below: C_n = total exactly, T_n = 2^32)
    std::vector<uint64_t> T(n + 1, 0);
    if (total > 0.0 && std::isfinite(total)) {
        double acc = 0.0;
        for (size_t i = 0; i < n; ++i) {
            acc += ml.power[i];
            const double x = std::floor(acc / total * 4294967296.0 + 0.5);
            T[i + 1] = std::min<uint64_t>((uint64_t)x, 1ull << 32);
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const uint64_t wd = T[i + 1] - T[i];
        ml.records[4 * PRT_LIGHT_F4 * i + 7] = (float)((double)wd / 4294967296.0);
        if (wd) {
            ml.cand_visible[i] = (uint32_t)ml.visible.size();
            ml.visible.push_back((uint32_t)i);
            ml.width.push_back(wd);
            ml.n_search = (uint32_t)i + 1u;
        } else if (ml.power[i] > 0.0) {
            ++ml.n_emitters_unsampled;
        }
    }
    prt_build_light_clusters(&hs, hs.lc.max_clusters);
    if (!ml.n_search) return;
    ml.thr.resize(ml.n_search - 1u);
    for (uint32_t i = 0; i + 1u < ml.n_search; ++i) ml.thr[i] = (uint32_t)T[i + 1];  // (< 2^32: a non-empty interval follows)
    // about one bucket per candidate, at most 2^20 (4 MiB): the bucket of r0's top bits brackets the search
    uint32_t bits = 0;
    while (bits < 20u && (1u << bits) < ml.n_search) ++bits;
    ml.bucket_shift = 32u - bits;
    ml.bucket.resize(((size_t)1 << bits) + 1);
    uint32_t i = 0;
    for (size_t b = 0; b < ((size_t)1 << bits); ++b) {
        const uint64_t r0 = bits ? (uint64_t)b << ml.bucket_shift : 0ull;
        while (i + 1u < ml.n_search && !(r0 < ml.thr[i])) ++i;
        ml.bucket[b] = i;
    }
    ml.bucket.back() = ml.n_search - 1u;
}

uint32_t count_not_similar(const PrtHostScene& hs) {
    // (build_light_table: the analytic emitters it counted; the mesh and placed triangles it counted are candidates here)
    return hs.n_emitters_unsampled - hs.ml_tris_counted;
}

// The candidate table of a compiled scene.  w.verts: the world-space meshes as flattened by compile_world_meshes.
void build_mesh_lights(const PrtSceneDesc* s, PrtHostScene& hs, const Work& w) {
    PrtMeshLights& ml = hs.ml;
    ml = PrtMeshLights();
    auto emissive = [&](uint32_t m) { return m < s->n_materials && s->materials[m].type == PRT_MAT_EMISSIVE; };
    const size_t n_analytic = hs.lights.size() / (4 * PRT_LIGHT_F4);
    size_t n = n_analytic;
    uint32_t prim = (uint32_t)hs.prims.size();
    for (uint32_t m = 0; m < s->n_meshes; ++m) {
        const uint32_t nt = s->meshes[m].n_triangles;
        if (emissive(s->meshes[m].material_id) && nt) {
            ml.runs.push_back(PrtLightRun{prim, nt, (uint32_t)n, 1u});
            n += nt;
        }
        prim += nt;
    }
    for (uint32_t i = 0; i < s->n_instances; ++i) {
        const PrtInstance& pi = s->instances[i];
        const uint32_t nt = s->instanced_meshes[pi.mesh].n_triangles;
        if (emissive(pi.material_id)) {
            ml.runs.push_back(PrtLightRun{prim, nt, (uint32_t)n, 0u});
            n += nt;
        }
        prim += nt;
    }
    ml.records.assign(4 * PRT_LIGHT_F4 * n, 0.0f);
    ml.power.assign(n, 0.0);
    ml.box.assign(6 * n, 0.0f);
    std::copy(hs.lights.begin(), hs.lights.end(), ml.records.begin());
    std::copy(hs.light_power.begin(), hs.light_power.end(), ml.power.begin());
    for (size_t l = 0; l < n_analytic; ++l) ml.records[4 * PRT_LIGHT_F4 * l + 11] = 0.0f;  // (no float CDF in this table)
    for (size_t l = 0; l < n_analytic; ++l) analytic_light_box(&ml.records[4 * PRT_LIGHT_F4 * l], &ml.box[6 * l]);
    size_t run = 0;
    prim = (uint32_t)hs.prims.size();
    for (uint32_t m = 0; m < s->n_meshes; ++m) {
        const uint32_t nt = s->meshes[m].n_triangles;
        if (emissive(s->meshes[m].material_id) && nt) {
            const PrtLightRun& r = ml.runs[run++];
            write_tri_candidates(ml, r.light_first, &w.verts[9 * (size_t)(prim - hs.prims.size())], nt, s->materials[s->meshes[m].material_id].rgb, prim);
        }
        prim += nt;
    }
    std::vector<float> v;
    for (uint32_t i = 0; i < s->n_instances; ++i) {
        const PrtInstance& pi = s->instances[i];
        const PrtMesh& me = s->instanced_meshes[pi.mesh];
        if (emissive(pi.material_id)) {
            // world vertices of the copy: Mat * v in double, rounded once (indices and vertices were checked by
            // build_instanced_meshes)
            v.resize(9 * (size_t)me.n_triangles);
            const float* M = pi.mat;
            for (size_t k = 0; k < 3 * (size_t)me.n_triangles; ++k) {
                const float* q = &me.positions[3 * (size_t)me.indices[k]];
                for (int a = 0; a < 3; ++a)
                    v[3 * k + a] = (float)(((double)M[a] * q[0] + (double)M[4 + a] * q[1]) + ((double)M[8 + a] * q[2] + (double)M[12 + a]));
            }
            const PrtLightRun& r = ml.runs[run++];
            write_tri_candidates(ml, r.light_first, v.data(), me.n_triangles, s->materials[pi.material_id].rgb, prim);
        }
        prim += me.n_triangles;
    }
    finish_mesh_lights(hs, count_not_similar(hs));
}

int compile_prims(const PrtSceneDesc* s, PrtHostScene& hs, std::string* err) {
    hs.materials.assign(s->materials, s->materials + s->n_materials);
    for (uint32_t i = 0; i < s->n_primitives; ++i) {
        const PrtPrimitive& p = s->primitives[i];
        if (p.shape_type != PRT_SHAPE_CIRCLE && p.shape_type != PRT_SHAPE_QUAD)
            return fail(err, "primitive %u: analytic shapes are CIRCLE or QUAD (triangles come as meshes)", i);
        if (p.material_id >= s->n_materials) return fail(err, "primitive %u: material out of range", i);
        DevPrim d;
        d.shape_type = p.shape_type;
        d.p0 = p.shape_param[0];
        d.p1 = p.shape_param[1];
        d.material = p.material_id;
        to_dev_mat(p.mat, d.mat);
        to_dev_mat(p.inv, d.inv);
        hs.prims.push_back(d);
    }
    return PRT_OK;
}

// The world-space meshes: validated, flattened, one tree over all of them, records in its leaf order; the scene-wide
// scalars as far as they are known here
int compile_world_meshes(const PrtSceneDesc* s, const PrtSceneOptions& opt, PrtHostScene& hs, Work& w, std::string* err) {
    uint64_t n_tris = 0;
    for (uint32_t m = 0; m < s->n_meshes; ++m) {
        const PrtMesh& me = s->meshes[m];
        if (me.n_triangles && (!me.positions || !me.normals || !me.indices))
            return fail(err, "mesh %u: positions, normals and indices are required", m);
        if (me.material_id >= s->n_materials) return fail(err, "mesh %u: material out of range", m);
        n_tris += me.n_triangles;
    }
    if (n_tris >= (1ull << 26)) return fail(err, "too many triangles (limit 2^26 - 1)");
    w.n_world = (uint32_t)n_tris;
    w.verts.resize(9 * (size_t)n_tris);
    w.norms.resize(9 * (size_t)n_tris);
    w.tri_mat.resize((size_t)n_tris);
    PrtSceneScalars& d = hs.sc;
    for (int k = 0; k < 3; ++k) {
        d.root_min[k] = FLT_MAX;
        d.root_max[k] = -FLT_MAX;
    }
    size_t t = 0;
    for (uint32_t m = 0; m < s->n_meshes; ++m) {
        const PrtMesh& me = s->meshes[m];
        const int rc = prt_flatten_mesh(me, "mesh", m, w.verts.data() + 9 * t, w.norms.data() + 9 * t, &d.extent, d.root_min, d.root_max, err);
        if (rc) return rc;
        std::fill_n(w.tri_mat.begin() + (ptrdiff_t)t, me.n_triangles, me.material_id);
        t += me.n_triangles;
        hs.mesh_sizes.push_back(me.n_vertices);
        hs.mesh_sizes.push_back(me.n_triangles);
        hs.mesh_material.push_back(me.material_id);
        if (me.n_triangles) hs.mesh_indices.insert(hs.mesh_indices.end(), me.indices, me.indices + 3 * (size_t)me.n_triangles);
    }
    const uint32_t n_prims = (uint32_t)hs.prims.size();
    hs.tri_records.assign(12 * (size_t)n_tris, 0.0f);
    hs.nrm_records.assign(12 * (size_t)n_tris, 0.0f);
    w.t_build0 = Clock::now();
    // (only a scene without placed copies walks the device builder's arrays as they are: `keep`)
    const int rc = build_tree(opt, TreeInput{w.verts.data(), w.norms.data(), w.tri_mat.data(), w.n_world, n_prims}, 0.0f, s->n_instances == 0, 15u,
                              true, 0, &hs.bvh, hs.tri_records.data(), hs.nrm_records.data(), &w.world_on_device, &hs.gpu_build_ms, err);
    if (rc == kHostBuildFailed) return fail(err, "BVH deeper than the traversal stack (%u > %u)", hs.bvh.max_depth, kMaxStack);
    if (rc) return rc;
    w.host_build_ms = ms_since(w.t_build0);
    w.depth8 = hs.bvh.depth8;
    // global primitive index: analytic first, then triangles in input order
    if (!w.world_on_device)
        pack_records(hs.bvh.order, w.verts.data(), w.norms.data(), w.n_world, n_prims, w.tri_mat.data(), hs.tri_records.data(), hs.nrm_records.data());
    d.n_prims = n_prims;
    // "the scene has a BVH" for the producers' classification
    d.n_nodes = w.world_on_device ? (uint32_t)(hs.bvh.nodes8.size() / 20) : (uint32_t)(hs.bvh.nodes.size() / 16);
    d.n_tris = w.n_world;
    d.pad = opt.pad_coeff;
    memcpy(d.sky, s->sky, sizeof(d.sky));
    return PRT_OK;
}

// World box of one analytic primitive under a uniform-scale transform (s2 = scale^2), widened by a relative slack; for
// spheres quad_pad grows to the envelope described at DevScene::abvh_q.  False if the box is not finite.
bool prim_world_box(const PrtPrimitive& p, double s2, float* mn, float* mx, double* quad_pad) {
    const float* M = p.mat;
    for (int a = 0; a < 3; ++a) {
        mn[a] = FLT_MAX;
        mx[a] = -FLT_MAX;
    }
    if (p.shape_type == PRT_SHAPE_CIRCLE) {  // sphere of radius r around the local origin
        const double R = std::fabs((double)p.shape_param[0]) * std::sqrt(s2);
        for (int a = 0; a < 3; ++a) {
            mn[a] = (float)((double)M[12 + a] - R);
            mx[a] = (float)((double)M[12 + a] + R);
        }
        // phantom hits of the fp32 discriminant: up to K * dist^2 / R outside the sphere, dist <= |o|_1 + |c|_1
        // (K = 1e-6: measured worst 2.0e-7 over 3.6e7 grazing rays at 3..1000 units, analytic bound 4.8e-7)
        if (R > 0.0) {
            const double q = 1e-6 / R, c1 = std::fabs((double)M[12]) + std::fabs((double)M[13]) + std::fabs((double)M[14]);
            quad_pad[0] = std::max(quad_pad[0], q);
            quad_pad[1] = std::max(quad_pad[1], 2.0 * q * c1);
            quad_pad[2] = std::max(quad_pad[2], q * c1 * c1);
        }
    } else {  // quad in the local plane y = 0
        for (int corner = 0; corner < 4; ++corner) {
            const float lx = ((corner & 1) ? 0.5f : -0.5f) * p.shape_param[0], lz = ((corner & 2) ? 0.5f : -0.5f) * p.shape_param[1];
            for (int a = 0; a < 3; ++a) {
                const float wv = (M[a] * lx + M[4 + a] * 0.0f) + (M[8 + a] * lz + M[12 + a]);
                mn[a] = std::min(mn[a], wv);
                mx[a] = std::max(mx[a], wv);
            }
        }
    }
    float mag = 0.0f;
    for (int a = 0; a < 3; ++a) mag = std::max(mag, std::max(std::fabs(mn[a]), std::fabs(mx[a])));
    const float slack = 1e-5f * (mag + (float)std::sqrt(s2) * (std::fabs(p.shape_param[0]) + std::fabs(p.shape_param[1]))) + 1e-30f;
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        mn[a] -= slack;
        mx[a] += slack;
        if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) finite = false;
    }
    return finite;
}

// BVH over the analytic primitives (only when there are many: the reference scans all of them for every ray,
// primitive.cpp:26; its default scene RANDOM_BALLS_LARGE has 809).  World boxes are only valid bounds of the
// reference's hits when the primitive's transform is rotation + uniform scale + translation (inv is not looked at:
// the boxes come from mat alone); one primitive that is not keeps the linear scan for the whole scene.
void build_prim_bvh(const PrtSceneDesc* s, const PrtSceneOptions& opt, PrtHostScene& hs) {
    const uint32_t n_prims = (uint32_t)hs.prims.size();
    if (!opt.prim_bvh || n_prims <= 16u) return;
    float extent_prims = 0.0f;
    double quad_pad[3] = {0.0, 0.0, 0.0};
    std::vector<float> pv(9 * (size_t)n_prims);
    bool ok = true;
    for (uint32_t i = 0; i < n_prims && ok; ++i) {
        const PrtPrimitive& p = s->primitives[i];
        double s2 = 0.0;
        if (!gram_is_uniform_scale(p.mat, &s2) || !affine_bottom_row(p.mat)) {
            ok = false;
            break;
        }
        float mn[3], mx[3];
        ok = prim_world_box(p, s2, mn, mx, quad_pad);
        for (int a = 0; a < 3; ++a) extent_prims = std::max(extent_prims, std::max(std::fabs(mn[a]), std::fabs(mx[a])));
        box_triangle(mn, mx, &pv[9 * (size_t)i]);
    }
    // (a walk that would need more than ABVH_STACK entries falls back to the scan)
    if (ok && (!bvh_build(pv.data(), n_prims, kMaxLeaf, 1, kMaxStack, &hs.abvh) || hs.abvh.nodes4.empty())) ok = false;
    if (!ok) hs.abvh = BvhBuild();
    if (hs.abvh.nodes4.empty()) return;
    hs.sc.extent = std::max(hs.sc.extent, extent_prims);  // the culling pad of the primitive walk scales with the scene
    for (int k = 0; k < 3; ++k) hs.sc.abvh_q[k] = (float)(quad_pad[k] * 1.0000002);  // (rounded up)
}

struct Blas {  // one instanced mesh: its tree in its own space and where its triangles / nodes went
    BvhBuild bvh;
    uint32_t slot_base = 0, node_base = 0, n_tris = 0;
    float mn[3], mx[3], extent = 0.0f;
};

// One tree per instanced mesh in its own space; its records go behind the world meshes' (and each other's) in
// hs.tri_records / nrm_records.  *slots_io: triangle slots so far.
int build_instanced_meshes(const PrtSceneDesc* s, const PrtSceneOptions& opt, PrtHostScene& hs, std::vector<Blas>& blas, uint64_t* slots_io,
                           std::string* err) {
    uint64_t slots = *slots_io;
    for (uint32_t m = 0; m < s->n_instanced_meshes; ++m) {
        const PrtMesh& me = s->instanced_meshes[m];
        if (!me.n_triangles || !me.positions || !me.normals || !me.indices)
            return fail(err, "instanced mesh %u: positions, normals and indices are required", m);
        Blas& B = blas[m];
        B.n_tris = me.n_triangles;
        std::vector<float> v(9 * (size_t)me.n_triangles), nn(9 * (size_t)me.n_triangles);
        for (int a = 0; a < 3; ++a) {
            B.mn[a] = FLT_MAX;
            B.mx[a] = -FLT_MAX;
        }
        int rc = prt_flatten_mesh(me, "instanced mesh", m, v.data(), nn.data(), &B.extent, B.mn, B.mx, err);
        if (rc) return rc;
        hs.placed_indices.emplace_back(me.indices, me.indices + 3 * (size_t)me.n_triangles);
        hs.placed_vertices.push_back(me.n_vertices);
        B.slot_base = (uint32_t)slots;
        slots += me.n_triangles;
        if (slots >= (1ull << 26)) return fail(err, "too many triangles (limit 2^26 - 1)");
        // triangle / normal records in this mesh's leaf order: {P0, face index}, {P1, -}, {P2, -}
        hs.tri_records.resize(12 * (size_t)slots, 0.0f);
        hs.nrm_records.resize(12 * (size_t)slots, 0.0f);
        float* tri_rec = &hs.tri_records[12 * (size_t)B.slot_base];
        float* nrm_rec = &hs.nrm_records[12 * (size_t)B.slot_base];
        bool on_device = false;
        rc = build_tree(opt, TreeInput{v.data(), nn.data(), nullptr, me.n_triangles, 0u}, 0.0f, false, 0xFFFFFFFFu, true, 0, &B.bvh, tri_rec, nrm_rec,
                        &on_device, &hs.gpu_build_ms, err);
        if (rc == kHostBuildFailed || (!rc && !on_device && B.bvh.nodes8.empty())) return fail(err, "instanced mesh %u: BVH construction failed", m);
        if (rc) return rc;
        if (!on_device) pack_records(B.bvh.order, v.data(), nn.data(), me.n_triangles, 0u, nullptr, tri_rec, nrm_rec);
    }
    *slots_io = slots;
    return PRT_OK;
}

// mat / inv / inv_scale of one placed copy (s2: scale^2 of its checked transform) and its world box: the 8 corners of its
// mesh's box through Mat, widened by a relative slack for the fp32 rounding of Mat * p anywhere inside the box.  The
// device pass of prt_set_instance_transforms (bvh_gpu.hip k_place_copies) evaluates the same fp32 expressions.
void place_copy(const PrtInstance& pi, double s2, const float* bmn, const float* bmx, DevInstance* I, std::array<float, 6>* box) {
    const float* M = pi.mat;
    to_dev_mat(pi.mat, I->mat);
    to_dev_mat(pi.inv, I->inv);
    I->inv_scale = (float)(1.0 / std::sqrt(s2));
    std::array<float, 6> bx{FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    float mag = 0.0f;
    for (int corner = 0; corner < 8; ++corner) {
        const float p3[3] = {(corner & 1) ? bmx[0] : bmn[0], (corner & 2) ? bmx[1] : bmn[1], (corner & 4) ? bmx[2] : bmn[2]};
        for (int a = 0; a < 3; ++a) {
            const float wv = (M[a] * p3[0] + M[4 + a] * p3[1]) + (M[8 + a] * p3[2] + M[12 + a]);
            bx[a] = std::min(bx[a], wv);
            bx[3 + a] = std::max(bx[3 + a], wv);
            mag = std::max(mag, std::fabs(wv));
        }
    }
    for (int a = 0; a < 3; ++a) {
        bx[a] -= 1e-5f * (mag + 1e-30f);
        bx[3 + a] += 1e-5f * (mag + 1e-30f);
    }
    *box = bx;
}

// The instance table, [identity instance of the world-space meshes] + the placed copies (root = mesh index for now), and
// every instance's world box
int build_instance_table(const PrtSceneDesc* s, PrtHostScene& hs, const Work& w, const std::vector<Blas>& blas,
                         std::vector<std::array<float, 6>>& boxes, std::string* err) {
    const PrtSceneScalars& d = hs.sc;
    auto identity12 = [](float* m12) {
        for (int k = 0; k < 12; ++k) m12[k] = 0.0f;
        m12[0] = m12[4] = m12[8] = 1.0f;
    };
    if (w.n_world) {
        DevInstance I{};
        identity12(I.mat);
        identity12(I.inv);
        I.root = 0;  // fixed up by assemble_two_level
        I.slot_base = 0;
        I.prim_base = 0;  // the world triangles' records carry their full primitive index
        I.virt_base = 0;
        I.material = 0xFFFFFFFFu;  // per triangle record
        I.n_tris = w.n_world;
        I.inv_scale = 1.0f;
        I.extent = d.extent;
        hs.dev_insts.push_back(I);
        boxes.push_back({d.root_min[0], d.root_min[1], d.root_min[2], d.root_max[0], d.root_max[1], d.root_max[2]});
        hs.world_box = boxes.back();
    }
    uint32_t virt = w.n_world, prim = d.n_prims + w.n_world;
    for (uint32_t i = 0; i < s->n_instances; ++i) {
        const PrtInstance& pi = s->instances[i];
        if (pi.mesh >= s->n_instanced_meshes) return fail(err, "instance %u: mesh out of range", i);
        if (pi.material_id >= s->n_materials) return fail(err, "instance %u: material out of range", i);
        // rotation + uniform scale + translation only: transpose(M3) * M3 = s^2 * I, and inv * mat = I
        double s2 = 0.0;
        if (!is_similarity(pi.mat, pi.inv, &s2))
            return fail(err,
                        "instance %u: the transform must be rotation + uniform scale + translation with inv = inverse(mat) "
                        "(the reference's local ray, primitive.cpp:29-30, is only a ray transform for those)", i);
        const Blas& B = blas[pi.mesh];
        DevInstance I{};
        std::array<float, 6> bx;
        place_copy(pi, s2, B.mn, B.mx, &I, &bx);
        I.slot_base = B.slot_base;
        I.prim_base = prim;
        I.virt_base = virt;
        I.material = pi.material_id;
        I.n_tris = B.n_tris;
        I.extent = B.extent;
        I.root = pi.mesh;  // mesh index for now; node base in assemble_two_level
        hs.dev_insts.push_back(I);
        hs.inst_mesh.push_back(pi.mesh);
        virt += B.n_tris;
        prim += B.n_tris;
        boxes.push_back(bx);
    }
    if ((uint64_t)virt + d.n_prims >= 0xFFFFFFF0ull) return fail(err, "too many placed triangles");
    return PRT_OK;
}

// The top-level tree over the instances' world boxes, by the same builders over one degenerate "triangle" per instance
// that spans its world box; order: leaf slot -> instance
int build_top_level(const PrtSceneOptions& opt, const std::vector<std::array<float, 6>>& boxes, BvhBuild& top, double* gpu_ms, std::string* err) {
    const uint32_t n_inst_total = (uint32_t)boxes.size();
    std::vector<float> pv(9 * (size_t)n_inst_total);
    for (uint32_t i = 0; i < n_inst_total; ++i) box_triangle(&boxes[i][0], &boxes[i][3], &pv[9 * (size_t)i]);
    std::vector<float> rec(12 * (size_t)n_inst_total);
    bool on_device = false;
    // (device builder: an instance in a hit leaf is ENTERED, a level switch of ~150 instructions, without a box test of its
    // own: a leaf cost this high makes the optimisation put every instance into a leaf of its own wherever the boxes
    // differ; copies whose boxes coincide may still share a leaf, which costs a redundant entry, never a result)
    const int rc = build_tree(opt, TreeInput{pv.data(), nullptr, nullptr, n_inst_total, 0u}, 64.0f, false, 0xFFFFFFFFu, false, 1, &top, rec.data(),
                              nullptr, &on_device, gpu_ms, err);
    if (rc == kPrtDeviceBuildGaveUp) return fail(err, "top-level tree: the device builder gave up; use gpu_build = 0 for this scene");
    if (rc == kHostBuildFailed || (!rc && !on_device && top.nodes8.empty())) return fail(err, "top-level BVH construction failed");
    if (rc) return rc;
    if (on_device) {  // a record's primitive index is the instance it stands for
        top.order.resize(n_inst_total);
        for (uint32_t sl = 0; sl < n_inst_total; ++sl) memcpy(&top.order[sl], &rec[12 * (size_t)sl + 3], 4);
    }
    return PRT_OK;
}

// The top-level tree over the instances' world boxes and the scene's one node array: [top level][world meshes' tree]
// [instanced meshes' trees], child_base / tri_base made absolute, every instance's root set
int assemble_two_level(const PrtSceneOptions& opt, PrtHostScene& hs, Work& w, std::vector<Blas>& blas, const std::vector<std::array<float, 6>>& boxes,
                       std::string* err) {
    BvhBuild top;
    const int rc = build_top_level(opt, boxes, top, &hs.gpu_build_ms, err);
    if (rc) return rc;
    hs.tlas_inst = top.order;
    hs.nodes8_all = top.nodes8;
    uint32_t max_blas_depth = 0;
    auto append = [&](const std::vector<uint32_t>& n8, uint32_t slot_base) -> uint32_t {
        const uint32_t node_base = (uint32_t)(hs.nodes8_all.size() / 20);
        const size_t at = hs.nodes8_all.size();
        hs.nodes8_all.insert(hs.nodes8_all.end(), n8.begin(), n8.end());
        for (size_t k = at; k < hs.nodes8_all.size(); k += 20) {
            hs.nodes8_all[k + 4] += node_base;
            hs.nodes8_all[k + 5] += slot_base;
        }
        return node_base;
    };
    uint32_t world_root = 0;
    if (w.n_world) {
        world_root = append(hs.bvh.nodes8, 0);
        max_blas_depth = hs.bvh.depth8;
    }
    for (Blas& B : blas) {
        B.node_base = append(B.bvh.nodes8, B.slot_base);
        max_blas_depth = std::max(max_blas_depth, B.bvh.depth8);
    }
    for (size_t i = 0; i < hs.dev_insts.size(); ++i) {
        DevInstance& I = hs.dev_insts[i];
        I.root = (w.n_world && i == 0) ? world_root : blas[I.root].node_base;
    }
    if (top.depth8 + max_blas_depth > 12u)
        return fail(err, "two-level BVH too deep for the traversal stack (%u + %u > 12)", top.depth8, max_blas_depth);
    w.depth8 = top.depth8 + max_blas_depth;
    // what prt_set_instance_transforms starts from
    hs.n_world_insts = w.n_world ? 1u : 0u;
    hs.top_nodes = (uint32_t)(top.nodes8.size() / 20);
    hs.top_depth = top.depth8;
    hs.max_mesh_depth = max_blas_depth;
    for (const Blas& B : blas) {
        PrtPlacedMesh pm{};
        memcpy(pm.mn, B.mn, sizeof(pm.mn));
        memcpy(pm.mx, B.mx, sizeof(pm.mx));
        pm.slot_base = B.slot_base;
        pm.node_base = B.node_base;
        pm.depth8 = B.bvh.depth8;
        pm.n_tris = B.n_tris;
        hs.placed_meshes.push_back(pm);
    }
    return PRT_OK;
}

// root_min / root_max / extent of a scene with placed copies from its instances' world boxes
void scene_bounds(PrtHostScene& hs, const std::vector<std::array<float, 6>>& boxes) {
    PrtSceneScalars& d = hs.sc;
    d.extent = hs.extent_base;
    for (int a = 0; a < 3; ++a) {
        d.root_min[a] = FLT_MAX;
        d.root_max[a] = -FLT_MAX;
    }
    for (const std::array<float, 6>& bx : boxes)
        for (int a = 0; a < 3; ++a) {
            d.root_min[a] = std::min(d.root_min[a], bx[a]);
            d.root_max[a] = std::max(d.root_max[a], bx[3 + a]);
            d.extent = std::max(d.extent, std::max(std::fabs(bx[a]), std::fabs(bx[3 + a])));
        }
}

// Placed mesh copies (PrtInstance): one tree per instanced mesh in its own space + a top-level tree over the copies'
// world boxes; the world-space meshes become one identity instance
int compile_instances(const PrtSceneDesc* s, const PrtSceneOptions& opt, PrtHostScene& hs, Work& w, std::string* err) {
    if (!s->n_instances) return PRT_OK;
    if (w.n_world && hs.bvh.nodes8.empty()) return fail(err, "instances need the 8-wide tree (leaves <= 3 triangles)");
    std::vector<Blas> blas(s->n_instanced_meshes);
    uint64_t slots = w.n_world;
    int rc = build_instanced_meshes(s, opt, hs, blas, &slots, err);
    if (rc) return rc;
    std::vector<std::array<float, 6>> boxes;
    if ((rc = build_instance_table(s, hs, w, blas, boxes, err))) return rc;
    if ((rc = assemble_two_level(opt, hs, w, blas, boxes, err))) return rc;
    // scene-wide quantities the producers use
    PrtSceneScalars& d = hs.sc;
    hs.extent_base = d.extent;
    scene_bounds(hs, boxes);
    d.n_insts = (uint32_t)hs.dev_insts.size();
    d.n_nodes = std::max(d.n_nodes, 1u);  // "the scene has a BVH"
    d.n_tris = (uint32_t)slots;
    w.host_build_ms = ms_since(w.t_build0);  // world meshes + every placed mesh + the top level
    return PRT_OK;
}

void fill_info(const PrtSceneDesc* s, const PrtSceneOptions& opt, PrtHostScene& hs, const Work& w) {
    hs.scene_device_built = w.world_on_device || (opt.device_build && s->n_instances != 0u);
    PrtBvhInfo& bi = hs.bvh_info;
    bi.n_nodes = (uint32_t)(hs.bvh.nodes.size() / 16);
    bi.n_triangles = hs.sc.n_tris;
    bi.max_depth = hs.bvh.max_depth;
    bi.max_leaf_size = hs.bvh.max_leaf;
    bi.sah_cost = hs.bvh.sah_cost;
    bi.pad_abs = opt.pad_coeff;
    bi.node_bytes = (uint64_t)hs.bvh.nodes4.size() * 4;
    bi.n_nodes4 = (uint32_t)(hs.bvh.nodes4.size() / 32);
    bi.max_stack4 = hs.bvh.max_stack4;
    bi.n_nodes8 = (uint32_t)((s->n_instances ? hs.nodes8_all : hs.bvh.nodes8).size() / 20);
    bi.depth8 = w.depth8;
    // device time of the builder's runs, or the host builders' wall time
    bi.build_ms = (float)(hs.scene_device_built ? hs.gpu_build_ms : w.host_build_ms);
    bi.built_on_device = hs.scene_device_built ? 1u : 0u;
    bi.refit_ms = 0.0f;
    bi.refits = 0u;
    bi.tri_bytes = (uint64_t)hs.tri_records.size() * 4;
}

}  // namespace

int prt_flatten_mesh(const PrtMesh& me, const char* what, uint32_t m, float* verts, float* norms, float* extent, float* mn, float* mx,
                     std::string* err) {
    float ext = *extent, lo[3], hi[3];  // (locals: the stores to verts / norms may alias the callers' accumulators)
    for (int a = 0; a < 3; ++a) {
        lo[a] = mn ? mn[a] : 0.0f;
        hi[a] = mn ? mx[a] : 0.0f;
    }
    for (uint32_t k = 0; k < me.n_triangles; ++k)
        for (int v = 0; v < 3; ++v) {
            const uint32_t vi = me.indices[3 * (size_t)k + v];
            if (vi >= me.n_vertices) return fail(err, "%s %u: vertex index out of range", what, m);
            for (int a = 0; a < 3; ++a) {
                const float pv = me.positions[3 * (size_t)vi + a];
                if (!std::isfinite(pv)) return fail(err, "%s %u: non-finite vertex", what, m);
                verts[9 * (size_t)k + 3 * v + a] = pv;
                norms[9 * (size_t)k + 3 * v + a] = me.normals[3 * (size_t)vi + a];
                ext = std::max(ext, std::fabs(pv));
                lo[a] = std::min(lo[a], pv);
                hi[a] = std::max(hi[a], pv);
            }
        }
    *extent = ext;
    for (int a = 0; a < 3 && mn; ++a) {
        mn[a] = lo[a];
        mx[a] = hi[a];
    }
    return PRT_OK;
}

void prt_rebuild_mesh_lights(PrtHostScene* hs, const float* verts, const PrtInstance* placed) {
    PrtMeshLights& ml = hs->ml;
    std::vector<float> v;
    size_t copy = 0;  // (runs and copies both ascend in prim_first / prim_base)
    for (const PrtLightRun& r : ml.runs) {
        if (r.world ? !verts : !placed) continue;
        float rgb[3];
        memcpy(rgb, &ml.records[4 * PRT_LIGHT_F4 * (size_t)r.light_first + 16], sizeof(rgb));
        if (r.world) {
            write_tri_candidates(ml, r.light_first, &verts[9 * (size_t)(r.prim_first - hs->prims.size())], r.n_tris, rgb, r.prim_first);
            continue;
        }
        while (copy < hs->inst_mesh.size() && hs->dev_insts[hs->n_world_insts + copy].prim_base != r.prim_first) ++copy;
        if (copy == hs->inst_mesh.size()) break;  // (cannot happen: every placed run is one copy)
        // world vertices of the copy as build_mesh_lights forms them: Mat * v in double, rounded once.  The mesh's
        // vertices in face order come from its triangle records (word 3 of a record: the face)
        const PrtPlacedMesh& pm = hs->placed_meshes[hs->inst_mesh[copy]];
        const float* M = placed[copy].mat;
        v.assign(9 * (size_t)pm.n_tris, 0.0f);
        for (size_t sl = 0; sl < (size_t)pm.n_tris; ++sl) {
            const float* rec = &hs->tri_records[12 * ((size_t)pm.slot_base + sl)];
            uint32_t face = 0;
            memcpy(&face, &rec[3], 4);
            if (face >= pm.n_tris) continue;
            for (int k = 0; k < 3; ++k) {
                const float* q = &rec[4 * k];
                for (int a = 0; a < 3; ++a)
                    v[9 * (size_t)face + 3 * k + a] = (float)(((double)M[a] * q[0] + (double)M[4 + a] * q[1]) + ((double)M[8 + a] * q[2] + (double)M[12 + a]));
            }
        }
        write_tri_candidates(ml, r.light_first, v.data(), pm.n_tris, rgb, r.prim_first);
    }
    finish_mesh_lights(*hs, count_not_similar(*hs));
}

// ---- refit from device arrays ----
uint32_t prt_tree_levels(const std::vector<uint32_t>& n8, uint32_t n_nodes, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_start) {
    level_nodes.assign(1, 0u);
    level_start.assign({0u, 1u});
    level_nodes.reserve(n_nodes);
    for (;;) {
        const uint32_t b = level_start[level_start.size() - 2], e = level_start.back();
        for (uint32_t li = b; li < e; ++li) {
            const uint32_t nd = level_nodes[li];
            const uint32_t imask = n8[20 * (size_t)nd + 3] >> 24, child_base = n8[20 * (size_t)nd + 4];
            const uint32_t kids = (uint32_t)__builtin_popcount(imask);
            if ((uint64_t)child_base + kids > n_nodes || level_nodes.size() + kids > n_nodes) return nd + 1u;
            for (uint32_t k = 0; k < kids; ++k) level_nodes.push_back(child_base + k);
        }
        if (level_nodes.size() == e) break;
        level_start.push_back((uint32_t)level_nodes.size());
    }
    return 0u;
}

int prt_build_refit_tables(const PrtHostScene& hs, PrtRefitTables* out, std::string* err) {
    PrtRefitTables t;
    const size_t n_meshes = hs.mesh_sizes.size() / 2;
    t.tri_first.assign(1, 0u);
    t.vert_first.assign(1, 0u);
    uint64_t nt = 0, nv = 0;
    for (size_t m = 0; m < n_meshes; ++m) {
        nv += hs.mesh_sizes[2 * m];
        nt += hs.mesh_sizes[2 * m + 1];
        if (nv >= 0xFFFFFFF0ull || 9 * nt >= 0xFFFFFFF0ull) return fail(err, "refit tables: too many vertices or corners");  // (32-bit thread indices)
        t.vert_first.push_back((uint32_t)nv);
        t.tri_first.push_back((uint32_t)nt);
    }
    if (hs.mesh_indices.size() != 3 * (size_t)nt) return fail(err, "refit tables: %zu indices for %llu triangles", hs.mesh_indices.size(), (unsigned long long)nt);
    // corners with their mesh's vertex base; a vertex's incident corners by a counting sort, which keeps ascending order
    t.corner.resize(3 * (size_t)nt);
    t.csr_start.assign((size_t)nv + 1, 0u);
    for (size_t m = 0; m < n_meshes; ++m)
        for (size_t k = 3 * (size_t)t.tri_first[m]; k < 3 * (size_t)t.tri_first[m + 1]; ++k) {
            if (hs.mesh_indices[k] >= hs.mesh_sizes[2 * m]) return fail(err, "refit tables: mesh %zu: vertex index out of range", m);
            t.corner[k] = t.vert_first[m] + hs.mesh_indices[k];
            ++t.csr_start[(size_t)t.corner[k] + 1];
        }
    for (size_t v = 0; v < (size_t)nv; ++v) t.csr_start[v + 1] += t.csr_start[v];
    t.csr_corner.resize(3 * (size_t)nt);
    std::vector<uint32_t> fill(t.csr_start.begin(), t.csr_start.end() - 1);
    for (size_t k = 0; k < t.corner.size(); ++k) t.csr_corner[fill[t.corner[k]]++] = (uint32_t)k;
    const uint32_t n_nodes = (uint32_t)(hs.bvh.nodes8.size() / 20);
    if (n_nodes) {  // (a scene without the 8-wide tree is not refitted; its normals can still be asked for)
        if (const uint32_t bad = prt_tree_levels(hs.bvh.nodes8, n_nodes, t.level_nodes, t.level_start))
            return fail(err, "refit tables: malformed tree (node %u)", bad - 1u);
        if (t.level_nodes.size() != n_nodes) return fail(err, "refit tables: %zu of %u nodes reachable from the root", t.level_nodes.size(), n_nodes);
    }
    for (const PrtLightRun& r : hs.ml.runs) {
        if (!r.world) continue;
        const uint64_t first = (uint64_t)r.prim_first - hs.prims.size();
        if (r.prim_first < hs.prims.size() || first + r.n_tris > nt) return fail(err, "refit tables: a light run lies outside the meshes");
        for (uint32_t k = 0; k < r.n_tris; ++k) t.light_tris.push_back((uint32_t)first + k);
    }
    *out = std::move(t);
    return PRT_OK;
}

void prt_rebuild_mesh_lights_packed(PrtHostScene* hs, const float* packed) {
    PrtMeshLights& ml = hs->ml;
    size_t at = 0;  // (light_tris lists the world runs in the order of ml.runs)
    for (const PrtLightRun& r : ml.runs) {
        if (!r.world) continue;
        float rgb[3];
        memcpy(rgb, &ml.records[4 * PRT_LIGHT_F4 * (size_t)r.light_first + 16], sizeof(rgb));
        write_tri_candidates(ml, r.light_first, &packed[9 * at], r.n_tris, rgb, r.prim_first);
        at += r.n_tris;
    }
    finish_mesh_lights(*hs, count_not_similar(*hs));
}

void prt_normals_from_corners(const float* positions, uint32_t n_vertices, const uint32_t* corner, const uint32_t* csr_start,
                              const uint32_t* csr_corner, float* normals) {
    for (uint32_t v = 0; v < n_vertices; ++v) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (uint32_t j = csr_start[v]; j < csr_start[v + 1]; ++j) {
            const uint32_t f = csr_corner[j] / 3u;
            const float* pa = &positions[3 * (size_t)corner[3 * (size_t)f]];
            const float* pb = &positions[3 * (size_t)corner[3 * (size_t)f + 1]];
            const float* pc = &positions[3 * (size_t)corner[3 * (size_t)f + 2]];
            const double e1[3] = {(double)pb[0] - pa[0], (double)pb[1] - pa[1], (double)pb[2] - pa[2]};
            const double e2[3] = {(double)pc[0] - pa[0], (double)pc[1] - pa[1], (double)pc[2] - pa[2]};
            acc[0] += e1[1] * e2[2] - e1[2] * e2[1];
            acc[1] += e1[2] * e2[0] - e1[0] * e2[2];
            acc[2] += e1[0] * e2[1] - e1[1] * e2[0];
        }
        const double l = std::sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
        for (int k = 0; k < 3; ++k) normals[3 * (size_t)v + k] = l > 0.0 ? (float)(acc[k] / l) : (k == 1 ? 1.0f : 0.0f);
    }
}

int prt_check_instance_update(const PrtHostScene& hs, const PrtInstance* instances, uint32_t n, std::string* err) {
    if (hs.inst_mesh.empty()) return fail(err, "prt_set_instance_transforms: the scene has no placed copies");
    if (n != hs.inst_mesh.size()) return fail(err, "prt_set_instance_transforms: the scene has %zu placed copies, not %u", hs.inst_mesh.size(), n);
    if (!instances) return fail(err, "null instance array");
    for (uint32_t i = 0; i < n; ++i) {
        const PrtInstance& pi = instances[i];
        if (pi.mesh != hs.inst_mesh[i] || pi.material_id != hs.dev_insts[hs.n_world_insts + i].material)
            return fail(err, "prt_set_instance_transforms: copy %u has another mesh or material than at prt_set_scene", i);
        double s2 = 0.0;
        if (!is_similarity(pi.mat, pi.inv, &s2))
            return fail(err, "instance %u: the transform must be rotation + uniform scale + translation with inv = inverse(mat)", i);
    }
    return PRT_OK;
}

void prt_instance_tables(const PrtHostScene& hs, const PrtInstance* instances, PrtInstanceUpdate* up) {
    up->insts = hs.dev_insts;
    up->boxes.clear();
    if (hs.n_world_insts) {  // the identity instance of the world meshes: their box, as prt_compile_scene left it
        up->boxes.push_back(hs.world_box);
    }
    for (size_t i = 0; i < hs.inst_mesh.size(); ++i) {
        const PrtPlacedMesh& pm = hs.placed_meshes[hs.inst_mesh[i]];
        double s2 = 0.0;
        (void)is_similarity(instances[i].mat, instances[i].inv, &s2);
        std::array<float, 6> bx;
        place_copy(instances[i], s2, pm.mn, pm.mx, &up->insts[hs.n_world_insts + i], &bx);
        up->boxes.push_back(bx);
    }
}

int prt_build_top_level(const PrtSceneOptions& opt, const PrtHostScene& hs, PrtInstanceUpdate* up, double* gpu_ms, std::string* err) {
    BvhBuild top;
    const int rc = build_top_level(opt, up->boxes, top, gpu_ms, err);
    if (rc) return rc;
    if (top.depth8 + hs.max_mesh_depth > 12u)
        return fail(err, "two-level BVH too deep for the traversal stack (%u + %u > 12)", top.depth8, hs.max_mesh_depth);
    up->top_nodes8 = std::move(top.nodes8);
    up->top_order = std::move(top.order);
    up->top_depth = top.depth8;
    return PRT_OK;
}

void prt_commit_top_level(PrtHostScene* hs, const PrtInstanceUpdate& up) {
    const uint32_t n_new = (uint32_t)(up.top_nodes8.size() / 20), delta = n_new - hs->top_nodes;  // (mod 2^32)
    std::vector<uint32_t> all(up.top_nodes8);
    all.insert(all.end(), hs->nodes8_all.begin() + 20 * (ptrdiff_t)hs->top_nodes, hs->nodes8_all.end());
    for (size_t k = up.top_nodes8.size(); k < all.size() && delta; k += 20) all[k + 4] += delta;
    hs->nodes8_all.swap(all);
    for (DevInstance& I : hs->dev_insts) I.root += delta;
    for (PrtPlacedMesh& pm : hs->placed_meshes) pm.node_base += delta;
    hs->tlas_inst = up.top_order;
    hs->top_nodes = n_new;
    hs->top_depth = up.top_depth;
    hs->bvh_info.n_nodes8 = (uint32_t)(hs->nodes8_all.size() / 20);
    hs->bvh_info.depth8 = up.top_depth + hs->max_mesh_depth;
}

void prt_commit_instances(PrtHostScene* hs, const PrtInstanceUpdate& up, const PrtInstance* instances) {
    for (size_t i = hs->n_world_insts; i < hs->dev_insts.size(); ++i) {
        DevInstance& I = hs->dev_insts[i];
        memcpy(I.mat, up.insts[i].mat, sizeof(I.mat));
        memcpy(I.inv, up.insts[i].inv, sizeof(I.inv));
        I.inv_scale = up.insts[i].inv_scale;
    }
    scene_bounds(*hs, up.boxes);
    prt_rebuild_mesh_lights(hs, nullptr, instances);
}

// ---- the environment light (PrtEnvTables, prt_scene.h; contract: include/prt.h "Environment light") ----
namespace {
// thresholds floor(C_i / C_n * 2^32 + 0.5) of the running sums of w[0..n) as interval widths; false: no weight at all
bool interval_widths(const double* w, uint32_t n, uint64_t* width) {
    double total = 0.0;
    for (uint32_t i = 0; i < n; ++i) total += w[i];
    if (!(total > 0.0)) {
        for (uint32_t i = 0; i < n; ++i) width[i] = 0;
        return false;
    }
    double acc = 0.0;
    uint64_t prev = 0;
    for (uint32_t i = 0; i < n; ++i) {
        acc += w[i];
        uint64_t T = i + 1u == n ? 4294967296ull : (uint64_t)std::floor(acc / total * 4294967296.0 + 0.5);
        if (T > 4294967296ull) T = 4294967296ull;
        if (T < prev) T = prev;
        width[i] = T - prev;
        prev = T;
    }
    return true;
}
// thr[i] = T_{i+1} for i < last (every one below 2^32: a non-empty interval follows); returns last
uint32_t search_table(const uint64_t* width, uint32_t n, uint32_t* thr) {
    uint32_t last = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (width[i]) last = i;
    uint64_t T = 0;
    for (uint32_t i = 0; i < n; ++i) {
        T += width[i];
        thr[i] = i < last ? (uint32_t)T : 0xFFFFFFFFu;
    }
    return last;
}
}  // namespace

int prt_build_environment(const PrtEnvironment* env, PrtEnvTables* out, std::string* err) {
    if (!env->rgb) return fail(err, "environment: null image");
    if (env->width == 0u || env->height == 0u) return fail(err, "environment: %u x %u", env->width, env->height);
    if (env->width > PRT_ENV_MAX_WIDTH || env->height > PRT_ENV_MAX_HEIGHT)
        return fail(err, "environment: %u x %u exceeds %u x %u", env->width, env->height, PRT_ENV_MAX_WIDTH, PRT_ENV_MAX_HEIGHT);
    if (!(env->light_share >= 0.0f && env->light_share <= 1.0f)) return fail(err, "environment: light_share %g outside [0, 1]", (double)env->light_share);
    const uint32_t W = env->width, H = env->height;
    const size_t n = (size_t)W * H;
    for (size_t k = 0; k < 3 * n; ++k)
        if (!(env->rgb[k] >= 0.0f && env->rgb[k] <= FLT_MAX)) return fail(err, "environment: texel %zu is negative or not finite", k / 3);
    PrtEnvTables t;
    t.W = W;
    t.H = H;
    t.light_share = env->light_share;
    t.texels.assign(4 * n, 0.0f);
    const double kPi = 3.14159265358979323846;
    std::vector<double> w(n), row_w(H);
    for (uint32_t i = 0; i < H; ++i) {
        const double omega = (2.0 * kPi / W) * (std::cos(kPi * i / H) - std::cos(kPi * (i + 1.0) / H));
        double sum = 0.0;
        for (uint32_t j = 0; j < W; ++j) {
            const float* p = env->rgb + 3 * ((size_t)i * W + j);
            w[(size_t)i * W + j] = (((double)p[0] + (double)p[1] + (double)p[2]) / 3.0) * omega;
            sum += w[(size_t)i * W + j];
            for (int ch = 0; ch < 3; ++ch) t.texels[4 * ((size_t)i * W + j) + ch] = p[ch];
        }
        row_w[i] = sum;
    }
    std::vector<uint64_t> rw(H), cw(n);
    if (interval_widths(row_w.data(), H, rw.data())) {
        for (uint32_t i = 0; i < H; ++i) interval_widths(&w[(size_t)i * W], W, &cw[(size_t)i * W]);
        t.row_thr.resize(H);
        t.col_thr.resize(n);
        t.col_last.resize(H);
        t.row_last = search_table(rw.data(), H, t.row_thr.data());
        const double k_pdf = (double)W * (double)H / (2.0 * kPi * kPi);
        for (uint32_t i = 0; i < H; ++i) {
            t.col_last[i] = search_table(&cw[(size_t)i * W], W, &t.col_thr[(size_t)i * W]);
            for (uint32_t j = 0; j < W; ++j) {
                const uint64_t c = rw[i] ? cw[(size_t)i * W + j] : 0u;
                if (c) ++t.n_sampled;
                // p_ij = rw cw / 2^64: both factors are integers <= 2^32, exact in double; the product is rounded once
                const double p = ((double)rw[i] / 4294967296.0) * ((double)c / 4294967296.0);
                t.texels[4 * ((size_t)i * W + j) + 3] = (float)(p * k_pdf);
            }
        }
        t.row_width = std::move(rw);
        t.col_width = std::move(cw);
    }
    *out = std::move(t);
    return PRT_OK;
}

uint64_t prt_environment_threshold(const PrtEnvTables& env, uint32_t n_lights) {
    if (!env.W || env.row_width.empty() || !(env.light_share > 0.0f)) return 0u;
    if (n_lights == 0u) return 4294967296ull;
    return (uint64_t)std::floor((double)env.light_share * 4294967296.0 + 0.5);
}

float prt_scaled_pmf(double pmf, uint64_t t_env) { return (float)(pmf * ((double)(4294967296ull - t_env) / 4294967296.0)); }

void prt_scaled_light_tables(const PrtHostScene& hs, uint64_t t_env, std::vector<float>* lights, std::vector<float>* ml_records) {
    if (lights) {
        *lights = hs.lights;
        double total = 0.0;
        for (double pw : hs.light_power) total += pw;  // (build_light_table's sum)
        for (size_t l = 0; t_env && l < hs.light_power.size(); ++l)
            (*lights)[4 * PRT_LIGHT_F4 * l + 7] = prt_scaled_pmf(hs.light_power[l] / total, t_env);
    }
    if (ml_records) {
        *ml_records = hs.ml.records;
        for (size_t v = 0; t_env && v < hs.ml.visible.size(); ++v)
            (*ml_records)[4 * PRT_LIGHT_F4 * (size_t)hs.ml.visible[v] + 7] = prt_scaled_pmf((double)hs.ml.width[v] / 4294967296.0, t_env);
    }
}

// ---- clustered light selection (PrtLightClusters, prt_scene.h; contract: include/prt.h "Clustered light selection") ----
namespace {
struct ClusterBuild {
    std::vector<uint32_t> m;  // candidates of the light set, ascending
    float lo[3], hi[3];
    uint64_t W = 0;           // sum of the members' global widths
    float r2 = 1e-30f;
    double key = 0.0;         // W r2: the cluster split next has the largest
    bool fixed = false;       // nothing to split
};

void fit_cluster(const PrtMeshLights& ml, ClusterBuild& c) {
    for (int a = 0; a < 3; ++a) c.lo[a] = INFINITY, c.hi[a] = -INFINITY;
    c.W = 0;
    for (uint32_t i : c.m) {
        for (int a = 0; a < 3; ++a) {
            c.lo[a] = std::min(c.lo[a], ml.box[6 * (size_t)i + a]);
            c.hi[a] = std::max(c.hi[a], ml.box[6 * (size_t)i + 3 + a]);
        }
        c.W += ml.width[ml.cand_visible[i]];
    }
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double h = 0.5 * ((double)c.hi[a] - (double)c.lo[a]);
        d2 += h * h;
    }
    c.r2 = round_up(d2);
    if (!(c.r2 >= 1e-30f)) c.r2 = 1e-30f;  // (a NaN too)
    c.key = (double)c.W * (double)c.r2;
    c.fixed = c.m.size() < 2;
}

// Splits c by a plane perpendicular to an axis into the members before and after it, ordered by box centre along that
// axis (ties: candidate order).  Where a plane separates the members' boxes (no box straddles it), the cut is the
// separating plane whose halves' powers are nearest to equal, on the first axis that has one, axes in descending order of
// the extent of the box centres; otherwise it is the power median along the longest axis.  false: the centres coincide.
bool split_cluster(const PrtMeshLights& ml, const ClusterBuild& c, ClusterBuild& left, ClusterBuild& right) {
    const size_t n = c.m.size();
    auto centre2 = [&](uint32_t i, int a) { return (double)ml.box[6 * (size_t)i + a] + (double)ml.box[6 * (size_t)i + 3 + a]; };
    double ext[3];
    int axes[3] = {0, 1, 2};
    for (int a = 0; a < 3; ++a) {
        double mn = INFINITY, mx = -INFINITY;
        for (uint32_t i : c.m) {
            mn = std::min(mn, centre2(i, a));
            mx = std::max(mx, centre2(i, a));
        }
        ext[a] = mx - mn;
    }
    std::stable_sort(axes, axes + 3, [&](int p, int q) { return ext[p] > ext[q]; });
    if (!(ext[axes[0]] > 0.0) || n < 2) return false;
    double total = 0.0;
    for (uint32_t i : c.m) total += ml.power[i];
    std::vector<uint32_t> order, first_order;
    std::vector<float> suffix_lo(n + 1);
    size_t cut = 0, first_median = 0;
    for (int k = 0; k < 3 && !cut && ext[axes[k]] > 0.0; ++k) {
        const int a = axes[k];
        order = c.m;
        std::sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) {
            const double cp = centre2(p, a), cq = centre2(q, a);
            return cp != cq ? cp < cq : p < q;
        });
        suffix_lo[n] = INFINITY;
        for (size_t j = n; j-- > 0;) suffix_lo[j] = std::min(suffix_lo[j + 1], ml.box[6 * (size_t)order[j] + a]);
        float prefix_hi = -INFINITY;
        double acc = 0.0, best = INFINITY;
        size_t median = 0;
        for (size_t j = 0; j + 1 < n; ++j) {  // the cut after member j
            prefix_hi = std::max(prefix_hi, ml.box[6 * (size_t)order[j] + 3 + a]);
            acc += ml.power[order[j]];
            if (!median && acc >= 0.5 * total) median = j + 1;
            const double off = std::fabs(acc - 0.5 * total);
            if (prefix_hi < suffix_lo[j + 1] && off < best) {
                best = off;
                cut = j + 1;
            }
        }
        if (k == 0) {
            first_median = median ? median : n - 1;
            if (!cut) first_order = order;
        }
    }
    if (!cut) {
        order.swap(first_order);
        cut = first_median;
    }
    left.m.assign(order.begin(), order.begin() + cut);
    right.m.assign(order.begin() + cut, order.end());
    std::sort(left.m.begin(), left.m.end());
    std::sort(right.m.begin(), right.m.end());
    fit_cluster(ml, left);
    fit_cluster(ml, right);
    return true;
}
}  // namespace

void prt_build_light_clusters(PrtHostScene* hs, uint32_t max_clusters) {
    const PrtMeshLights& ml = hs->ml;
    PrtLightClusters& lc = hs->lc;
    const uint32_t K = max_clusters ? std::min(max_clusters, PRT_LIGHT_MAX_CLUSTERS) : 32u;
    lc = PrtLightClusters();
    lc.max_clusters = K;
    lc.cand_cluster.assign(ml.power.size(), 0xFFFFFFFFu);
    lc.cand_member.assign(ml.power.size(), 0xFFFFFFFFu);
    if (ml.visible.empty()) return;
    std::vector<ClusterBuild> cl(1);
    cl[0].m = ml.visible;
    fit_cluster(ml, cl[0]);
    while (cl.size() < K) {
        size_t pick = cl.size();
        for (size_t i = 0; i < cl.size(); ++i)
            if (!cl[i].fixed && (pick == cl.size() || cl[i].key > cl[pick].key)) pick = i;
        if (pick == cl.size()) break;
        ClusterBuild l, r;
        if (!split_cluster(ml, cl[pick], l, r)) {
            cl[pick].fixed = true;
            continue;
        }
        cl[pick] = std::move(l);  // (the halves take the parent's place: the order is a function of the splits alone)
        cl.insert(cl.begin() + (std::ptrdiff_t)pick + 1, std::move(r));
    }
    for (size_t ci = 0; ci < cl.size(); ++ci) {
        const ClusterBuild& c = cl[ci];
        const uint32_t first = (uint32_t)lc.members.size(), n = (uint32_t)c.m.size();
        const float phi = (float)((double)c.W / 4294967296.0);
        const float b[8] = {c.lo[0], c.lo[1], c.lo[2], phi, c.hi[0], c.hi[1], c.hi[2], c.r2};
        lc.boxes.insert(lc.boxes.end(), b, b + 8);
        lc.power_width.push_back(c.W);
        double total = 0.0;
        for (uint32_t i : c.m) total += ml.power[i];
        double acc = 0.0;
        uint64_t prev = 0;
        uint32_t last = first;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t i = c.m[j];
            acc += ml.power[i];
            uint64_t U = std::min<uint64_t>((uint64_t)std::floor(acc / total * 4294967296.0 + 0.5), 1ull << 32);
            if (j + 1 == n) U = 1ull << 32;
            lc.cand_cluster[i] = (uint32_t)ci;
            lc.cand_member[i] = first + j;
            lc.members.push_back(i);
            lc.thr.push_back((uint32_t)U);
            lc.inner_width.push_back(U - prev);
            if (U > prev) last = first + j; else ++lc.n_empty_inner;
            prev = U;
        }
        const uint32_t rg[4] = {first, last, n, 0u};
        lc.range.insert(lc.range.end(), rg, rg + 4);
    }
}

void prt_cluster_pmf_in(const PrtHostScene& hs, uint64_t t_env, std::vector<float>* out) {
    const PrtLightClusters& lc = hs.lc;
    out->assign(lc.cand_cluster.size(), 0.0f);
    for (size_t k = 0; k < lc.members.size(); ++k) (*out)[lc.members[k]] = prt_scaled_pmf((double)lc.inner_width[k] / 4294967296.0, t_env);
}

// ---- image textures (include/prt.h "Image textures") ----
int prt_build_textures(const PrtHostScene& hs, const PrtTextureSet* set, PrtTexTables* out, std::string* err) {
    if (!set) return fail(err, "prt_set_textures: null set");
    const uint32_t n_mats = (uint32_t)hs.materials.size();
    const uint32_t n_meshes = (uint32_t)(hs.mesh_sizes.size() / 2);
    if (set->n_materials != n_mats) return fail(err, "prt_set_textures: the scene has %u materials, not %u", n_mats, set->n_materials);
    if (set->n_meshes != n_meshes) return fail(err, "prt_set_textures: the scene has %u meshes, not %u", n_meshes, set->n_meshes);
    if (set->n_instanced_meshes != hs.n_instanced_meshes)
        return fail(err, "prt_set_textures: the scene has %u instanced meshes, not %u", hs.n_instanced_meshes, set->n_instanced_meshes);
    if ((set->n_textures && !set->textures) || (n_mats && !set->material_texture) || (n_meshes && !set->mesh_uvs) ||
        (set->n_instanced_meshes && !set->instanced_mesh_uvs))
        return fail(err, "prt_set_textures: null array in the texture set");
    PrtTexTables t;
    t.is_set = true;
    t.n_textures = set->n_textures;
    // textures: sizes, modes, texels
    uint64_t n_texels = 0;
    for (uint32_t k = 0; k < set->n_textures; ++k) {
        const PrtTexture& tx = set->textures[k];
        if (tx.width == 0u || tx.height == 0u || tx.width > PRT_TEX_MAX_SIZE || tx.height > PRT_TEX_MAX_SIZE)
            return fail(err, "texture %u: %u x %u (each side must be 1 .. %u)", k, tx.width, tx.height, PRT_TEX_MAX_SIZE);
        if (!tx.rgb) return fail(err, "texture %u: null image", k);
        if (tx.filter != PRT_TEX_NEAREST && tx.filter != PRT_TEX_BILINEAR) return fail(err, "texture %u: unknown filter %u", k, tx.filter);
        if (tx.wrap != PRT_TEX_REPEAT && tx.wrap != PRT_TEX_CLAMP) return fail(err, "texture %u: unknown wrap %u", k, tx.wrap);
        n_texels += (uint64_t)tx.width * tx.height;
    }
    if (n_texels >= (1ull << 32)) return fail(err, "prt_set_textures: too many texels (limit 2^32 - 1)");
    for (uint32_t k = 0; k < set->n_textures; ++k) {
        const PrtTexture& tx = set->textures[k];
        const size_t n = (size_t)tx.width * tx.height;
        for (size_t i = 0; i < 3 * n; ++i)
            if (!(tx.rgb[i] >= 0.0f) || !std::isfinite(tx.rgb[i])) return fail(err, "texture %u: negative or non-finite texel", k);
    }
    // materials
    t.mat_tex.assign(set->material_texture, set->material_texture + n_mats);
    std::vector<uint8_t> textured(n_mats, 0);
    for (uint32_t m = 0; m < n_mats; ++m) {
        const uint32_t tx = t.mat_tex[m];
        if (tx == PRT_TEXTURE_NONE) continue;
        if (tx >= set->n_textures) return fail(err, "material %u: texture %u out of range", m, tx);
        if (hs.materials[m].type != PRT_MAT_LAMBERTIAN && hs.materials[m].type != PRT_MAT_METAL)
            return fail(err, "material %u: only Lambertian and Metal materials take a texture", m);
        textured[m] = 1;
        ++t.n_textured_materials;
    }
    // who uses a textured material: no sphere, no mesh or placed copy without UVs
    for (size_t i = 0; i < hs.prims.size(); ++i)
        if (hs.prims[i].shape_type == PRT_SHAPE_CIRCLE && textured[hs.prims[i].material])
            return fail(err, "primitive %zu: a sphere cannot carry a textured material", i);
    for (uint32_t m = 0; m < n_meshes; ++m)
        if (hs.mesh_sizes[2 * m + 1] && textured[hs.mesh_material[m]] && !set->mesh_uvs[m])
            return fail(err, "mesh %u: a textured material needs UVs", m);
    const bool placed = !hs.inst_mesh.empty();
    for (size_t i = 0; placed && i < hs.inst_mesh.size(); ++i)
        if (textured[hs.dev_insts[hs.n_world_insts + i].material] && !set->instanced_mesh_uvs[hs.inst_mesh[i]])
            return fail(err, "instance %zu: a textured material needs UVs on its mesh", i);
    auto uv_ok = [](const float* uv, size_t n_vertices) {
        for (size_t i = 0; i < 2 * n_vertices; ++i)
            if (!std::isfinite(uv[i]) || std::fabs(uv[i]) > 1048576.0f) return false;
        return true;
    };
    for (uint32_t m = 0; m < n_meshes; ++m)
        if (set->mesh_uvs[m] && !uv_ok(set->mesh_uvs[m], hs.mesh_sizes[2 * m])) return fail(err, "mesh %u: a UV is not finite or above 2^20", m);
    for (uint32_t m = 0; placed && m < hs.n_instanced_meshes; ++m)
        if (set->instanced_mesh_uvs[m] && !uv_ok(set->instanced_mesh_uvs[m], hs.placed_vertices[m]))
            return fail(err, "instanced mesh %u: a UV is not finite or above 2^20", m);
    // ---- everything is checked: the tables ----
    t.texels.resize(4 * (size_t)n_texels);
    t.desc.resize(4 * (size_t)set->n_textures);
    size_t at = 0;
    for (uint32_t k = 0; k < set->n_textures; ++k) {
        const PrtTexture& tx = set->textures[k];
        t.desc[4 * (size_t)k + 0] = (uint32_t)at;
        t.desc[4 * (size_t)k + 1] = tx.width;
        t.desc[4 * (size_t)k + 2] = tx.height;
        t.desc[4 * (size_t)k + 3] = tx.filter | (tx.wrap << 1);
        const size_t n = (size_t)tx.width * tx.height;
        for (size_t i = 0; i < n; ++i) {
            t.texels[4 * (at + i) + 0] = tx.rgb[3 * i + 0];
            t.texels[4 * (at + i) + 1] = tx.rgb[3 * i + 1];
            t.texels[4 * (at + i) + 2] = tx.rgb[3 * i + 2];
            t.texels[4 * (at + i) + 3] = 0.0f;
        }
        at += n;
    }
    size_t n_uv_tris = hs.mesh_indices.size() / 3;
    std::vector<uint32_t> placed_base(hs.placed_indices.size(), 0u);
    for (size_t m = 0; m < hs.placed_indices.size(); ++m) {
        placed_base[m] = (uint32_t)n_uv_tris;
        n_uv_tris += hs.placed_indices[m].size() / 3;
    }
    t.uvs.assign(6 * n_uv_tris, 0.0f);
    auto fill = [&](float* dst, const uint32_t* idx, size_t n_idx, const float* uv) {
        for (size_t i = 0; uv && i < n_idx; ++i) {
            dst[2 * i + 0] = uv[2 * (size_t)idx[i] + 0];
            dst[2 * i + 1] = uv[2 * (size_t)idx[i] + 1];
        }
    };
    size_t tri = 0;
    for (uint32_t m = 0; m < n_meshes; ++m) {
        const size_t n = hs.mesh_sizes[2 * m + 1];
        fill(t.uvs.data() + 6 * tri, hs.mesh_indices.data() + 3 * tri, 3 * n, set->mesh_uvs[m]);
        tri += n;
    }
    for (size_t m = 0; m < hs.placed_indices.size(); ++m)
        fill(t.uvs.data() + 6 * (size_t)placed_base[m], hs.placed_indices[m].data(), hs.placed_indices[m].size(), set->instanced_mesh_uvs[m]);
    for (uint32_t m = 0; m < n_meshes; ++m) t.mesh_has_uv.push_back(set->mesh_uvs[m] ? 1u : 0u);
    for (size_t m = 0; m < hs.placed_indices.size(); ++m) t.mesh_has_uv.push_back(set->instanced_mesh_uvs[m] ? 1u : 0u);
    t.inst_uv_base.resize(hs.dev_insts.size());
    for (size_t i = 0; i < hs.dev_insts.size(); ++i)
        t.inst_uv_base[i] = i < hs.n_world_insts ? 0u - hs.sc.n_prims : placed_base[hs.inst_mesh[i - hs.n_world_insts]];
    *out = std::move(t);
    return PRT_OK;
}

int prt_check_scene_arrays(const PrtSceneDesc* s, std::string* err) {
    if ((s->n_materials && !s->materials) || (s->n_primitives && !s->primitives) || (s->n_meshes && !s->meshes) ||
        (s->n_instanced_meshes && !s->instanced_meshes) || (s->n_instances && !s->instances))
        return fail(err, "null array in scene description");
    return PRT_OK;
}

int prt_compile_scene(const PrtSceneDesc* s, const PrtSceneOptions& opt, PrtHostScene* out, std::string* err) {
    int rc = prt_check_scene_arrays(s, err);
    if (rc) return rc;
    // a fresh scene, except that the two big record arrays keep the storage *out came with (96 bytes per triangle that a
    // context which sets its scene again need not unmap and fault in anew; compile_world_meshes overwrites all of it)
    PrtHostScene fresh;
    fresh.tri_records.swap(out->tri_records);
    fresh.nrm_records.swap(out->nrm_records);
    *out = std::move(fresh);
    PrtHostScene& hs = *out;
    hs.lc.max_clusters = opt.light_clusters ? std::min(opt.light_clusters, PRT_LIGHT_MAX_CLUSTERS) : 32u;
    Work w;
    if ((rc = compile_prims(s, hs, err))) return rc;
    hs.n_instanced_meshes = s->n_instanced_meshes;
    build_light_table(&hs, s);
    if ((rc = compile_world_meshes(s, opt, hs, w, err))) return rc;
    build_prim_bvh(s, opt, hs);
    if ((rc = compile_instances(s, opt, hs, w, err))) return rc;
    build_mesh_lights(s, hs, w);
    fill_info(s, opt, hs, w);
    return PRT_OK;
}

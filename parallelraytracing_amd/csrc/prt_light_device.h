// prt_light_device.h — the light-sampling device functions (PrtLighting, include/prt.h; DESIGN.md §3 "Light sampling"): one
// light sample per Lambertian vertex from the analytic, triangle, clustered and environment tables, its MIS weight, and the
// weight of an emitter or of the environment met by the scattered segment.  Shared, verbatim, by the shade kernels
// (prt_kernels.hip) and by the light-sampled radiance query (prt_radiance_lit.hip).  Needs prt_kernels.h and prt_device.h.
#pragma once
#define PRT_LIGHT_RNG 0x68E31DA5u            // the light sample's own stream: pcg_hash(path state at the vertex + this)
#define PRT_INV_PI 0.318309886183790672f
#define PRT_TWO_PI 6.28318530717958648f

// 1 - cos(theta_max) of the cone a sphere light (L0 = centre, R) subtends from x, as (R^2/D^2) / (1 + sqrt(1 - R^2/D^2))
// (no cancellation for small R/D); 0 from inside the sphere or within PRT_LIGHT_SPHERE_MARGIN of its surface
PRT_DEV float sphere_cone_omc(float4 L0, f3 x) {
    const f3 cd = mk3(L0.x, L0.y, L0.z) - x;
    const float D2 = dot3(cd, cd);
    const float lim = L0.w * (1.0f + PRT_LIGHT_SPHERE_MARGIN);
    if (!(D2 > lim * lim)) return 0.0f;
    const float q = (L0.w * L0.w) / D2;
    return q / (1.0f + __builtin_sqrtf(1.0f - q));
}

// Solid-angle pdf with which the light (records L0, L3) samples the unit direction w from x, whose point on the light lies
// at distance^2 d2: quad d2 / (A |n_l.w|), sphere 1 / (2 pi (1 - cos theta_max)); 0 = the light cannot sample w.
// (MESHL: the instances that know triangle lights, kind 2: the quad's formula with the triangle's area and normal)
template <bool MESHL = false>
PRT_DEV float light_pdf_w(float4 L0, float4 L3, f3 x, f3 w, float d2) {
    if (MESHL ? __float_as_uint(L3.w) != 0u : __float_as_uint(L3.w) == 1u) {
        const float den = L0.w * __builtin_fabsf(dot3(mk3(L3.x, L3.y, L3.z), w));
        return den > 0.0f ? d2 / den : 0.0f;
    }
    const float omc = sphere_cone_omc(L0, x);
    return omc > 0.0f ? 1.0f / (PRT_TWO_PI * omc) : 0.0f;
}

struct LightSample {
    f3 w;          // unit direction from x
    float t_light; // distance to the sampled point (quad) / the near intersection (sphere)
    float tmax;    // shadow-ray bound: t_light * (1 - PRT_LIGHT_SHADOW_EPS)
    float pdf_l;   // pmf * pdf_w
    f3 le;         // emission
    uint32_t light;
};

// Triangle lights: the candidate of the 32-bit draw r0, the smallest i with r0 < T_{i+1} = thr[i] (n_lights - 1 if none:
// T_n = 2^32).  thr is a dense uint32 array (4 B per candidate against the records' 80 B: ~3.5 MB for 870 k lights, which
// stays in L2 / MALL where the records do not).  Plain binary search: ceil(log2 n) DEPENDENT loads per lane, and the
// lanes of a wave draw independently, so every step is a fully divergent gather.  The bucket table (about one bucket
// per candidate, at most 2^20) gives the candidates of the first and last draw of r0's bucket, which bracket the
// answer: two independent loads, then a search over the few thresholds that fall inside one bucket (often none).  The
// result is the same index either way.
PRT_DEV uint32_t select_light(const DevLights& lt, const DevMeshLights& ml, uint32_t r0) {
    uint32_t lo = 0u, hi = lt.n_lights - 1u;
    if (ml.bucket) {
        const uint32_t b = ml.bucket_shift < 32u ? r0 >> ml.bucket_shift : 0u;
        lo = ml.bucket[b];
        hi = ml.bucket[b + 1u];
    }
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r0 < ml.thr[mid]) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

// Candidate of the triangle with global primitive index `prim` (a triangle with an Emissive material lies in a run);
// 0xFFFFFFFF if it lies in none.
PRT_DEV uint32_t triangle_light(const DevMeshLights& ml, uint32_t prim) {
    if (!ml.n_runs) return 0xFFFFFFFFu;
    uint32_t lo = 0u, hi = ml.n_runs;  // the last run with prim_first <= prim
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ml.runs[mid].prim_first <= prim) lo = mid; else hi = mid;
    }
    const DevLightRun r = ml.runs[lo];
    return prim - r.prim_first < r.n_tris ? r.light_first + (prim - r.prim_first) : 0xFFFFFFFFu;
}

// ---- clustered light selection (include/prt.h "Clustered light selection"; DevLightClusters) ----
// The thresholds M_c of the cluster choice at x, handed to f(c, M_{c-1}, M_c) for c = 0 .. K-1 in order.  Two passes over the
// cluster records instead of K running sums in registers: the first adds up the total (and the fallback's, the sum of
// phi), the second repeats the same additions and scales each running sum.  c and the record addresses are the same in
// every lane, so the records come through the scalar data cache; per cluster and pass: 6 subtractions, 6 selects, 5 for
// D2, one select, one division, one addition.  (Ending the second pass once every lane of the wave has its cluster was
// measured and is slower: the lanes' draws are independent, so a wave is done only near the end, and the ballot costs more.)
template <class F>
PRT_DEV void cluster_thresholds(const DevLightClusters& lc, f3 x, F f) {
    const uint32_t K = lc.n_clusters;
    float tot = 0.0f, tot_phi = 0.0f;
    for (uint32_t c = 0; c < K; ++c) {
        const float4 lo = lc.boxes[2u * c], hi = lc.boxes[2u * c + 1u];
        float t = lo.x - x.x, u = x.x - hi.x;
        float dx = t > u ? t : u;
        dx = dx > 0.0f ? dx : 0.0f;
        t = lo.y - x.y, u = x.y - hi.y;
        float dy = t > u ? t : u;
        dy = dy > 0.0f ? dy : 0.0f;
        t = lo.z - x.z, u = x.z - hi.z;
        float dz = t > u ? t : u;
        dz = dz > 0.0f ? dz : 0.0f;
        const float D2 = (dx * dx + dy * dy) + dz * dz;
        const float den = D2 > hi.w ? D2 : hi.w;
        tot = tot + lo.w / den;
        tot_phi = tot_phi + lo.w;
    }
    const bool fb = !(tot > 0.0f && tot < __builtin_inff());  // (position-independent fallback: D2 overflowed, or a NaN)
    const float inv = 1.0f / (fb ? tot_phi : tot);
    float cum = 0.0f;
    uint32_t m_prev = 0u;
    for (uint32_t c = 0; c < K; ++c) {
        const float4 lo = lc.boxes[2u * c], hi = lc.boxes[2u * c + 1u];
        float t = lo.x - x.x, u = x.x - hi.x;
        float dx = t > u ? t : u;
        dx = dx > 0.0f ? dx : 0.0f;
        t = lo.y - x.y, u = x.y - hi.y;
        float dy = t > u ? t : u;
        dy = dy > 0.0f ? dy : 0.0f;
        t = lo.z - x.z, u = x.z - hi.z;
        float dz = t > u ? t : u;
        dz = dz > 0.0f ? dz : 0.0f;
        const float D2 = (dx * dx + dy * dy) + dz * dz;
        const float den = D2 > hi.w ? D2 : hi.w;
        cum = cum + (fb ? lo.w : lo.w / den);
        const float q = (cum * inv) * 16777216.0f;
        const uint32_t mc = (c + 1u < K && q < 16777216.0f) ? (uint32_t)q : 16777216u;
        f(c, m_prev, mc);
        m_prev = mc;
    }
}

// P_c = (M_c - M_{c-1}) 2^-24 (exact); 0 for an empty or inverted interval
PRT_DEV float cluster_prob(uint32_t m_prev, uint32_t mc) { return mc > m_prev ? (float)(mc - m_prev) * (1.0f / 16777216.0f) : 0.0f; }

// The cluster of the 24-bit draw m at x (the smallest c with m < M_c) and its probability
PRT_DEV uint32_t select_cluster(const DevLightClusters& lc, f3 x, uint32_t m, float& P) {
    uint32_t cl = lc.n_clusters - 1u;
    bool found = false;
    P = 0.0f;
    cluster_thresholds(lc, x, [&](uint32_t c, uint32_t m_prev, uint32_t mc) {
        if (!found && m < mc) {
            found = true;
            cl = c;
            P = cluster_prob(m_prev, mc);
        }
    });
    return cl;
}

// P_c(x) of a given cluster: the same evaluation
PRT_DEV float cluster_prob_at(const DevLightClusters& lc, f3 x, uint32_t cl) {
    float P = 0.0f;
    cluster_thresholds(lc, x, [&](uint32_t c, uint32_t m_prev, uint32_t mc) {
        if (c == cl) P = cluster_prob(m_prev, mc);
    });
    return P;
}

// One light sample from x with the draws of key's own stream (the path's state is not advanced): the light by its CDF
// (MESHL: by the integer thresholds, select_light), then a point uniform by area (quad, triangle) or a direction uniform
// in the cone (sphere).  false: no sample (pdf 0).
// CLUS (lc: the cluster tables): the cluster by select_cluster with u0's 24 bits, the member by the cluster's own integer
// thresholds with the state after the stream's fourth step; pmf = P_c pmf_in.
template <bool MESHL = false, bool CLUS = false>
PRT_DEV bool sample_light(const DevLights& lt, f3 x, uint32_t key, LightSample& s, const DevMeshLights* ml = nullptr,
                          const DevLightClusters* lc = nullptr) {
    uint32_t ls = pcg_hash(key + PRT_LIGHT_RNG);
    const float u0 = rnd01(ls);
    const uint32_t r0 = ls;  // the state after the stream's first step: u0 is its top 24 bits
    const float u1 = rnd01(ls);
    const float u2 = rnd01(ls);
    uint32_t lo = 0u, hi = lt.n_lights - 1u;  // smallest i with u0 < cdf[i] (cdf[n - 1] = 1)
    float pmf_c = 0.0f;
    if (CLUS) {
        const uint32_t r3 = pcg_hash(ls);
        float P;
        const uint32_t cl = select_cluster(*lc, x, r0 >> 8, P);
        const uint4 rg = lc->range[cl];
        uint32_t ja = rg.x, jb = rg.y;  // the smallest member j in [first, last] with r3 < U_j, else last: log2(members) dependent loads
        while (ja < jb) {
            const uint32_t mid = (ja + jb) >> 1;
            if (r3 < lc->thr[mid]) jb = mid; else ja = mid + 1u;
        }
        lo = lc->members[ja];
        pmf_c = P * lc->cand_pmf_in[lo];
    } else if (MESHL) {
        lo = select_light(lt, *ml, r0);
    } else {
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (u0 < lt.lights[PRT_LIGHT_F4 * mid + 2u].w) hi = mid; else lo = mid + 1u;
        }
    }
    const float4* L = lt.lights + PRT_LIGHT_F4 * lo;
    const float4 L0 = L[0], L1 = L[1], L2 = L[2], L3 = L[3], L4 = L[4];
    s.light = lo;
    s.le = mk3(L4.x, L4.y, L4.z);
    const f3 c = mk3(L0.x, L0.y, L0.z);
    float t_light, pdf_w;
    if (__float_as_uint(L3.w) == 1u) {  // quad: p = c + (u1 - 1/2) u + (u2 - 1/2) v
        const f3 p = c + mk3(L1.x, L1.y, L1.z) * (u1 - 0.5f) + mk3(L2.x, L2.y, L2.z) * (u2 - 0.5f);
        const f3 dv = p - x;
        const float d2 = dot3(dv, dv);
        t_light = __builtin_sqrtf(d2);
        s.w = dv * (1.0f / t_light);
        pdf_w = light_pdf_w(L0, L3, x, s.w, d2);
    } else if (MESHL && __float_as_uint(L3.w) == 2u) {  // triangle: s = sqrt(u1), p = v0 + (s (1 - u2)) e1 + (s u2) e2
        const float sq = __builtin_sqrtf(u1);
        const f3 p = c + mk3(L1.x, L1.y, L1.z) * (sq * (1.0f - u2)) + mk3(L2.x, L2.y, L2.z) * (sq * u2);
        const f3 dv = p - x;
        const float d2 = dot3(dv, dv);
        t_light = __builtin_sqrtf(d2);
        s.w = dv * (1.0f / t_light);
        pdf_w = light_pdf_w<true>(L0, L3, x, s.w, d2);
    } else {  // sphere: 1 - cos theta = u1 (1 - cos theta_max), phi = 2 pi u2 about the direction to the centre
        const float omc = sphere_cone_omc(L0, x);
        if (!(omc > 0.0f)) return false;
        const f3 cd = c - x;
        const float D2 = dot3(cd, cd);
        const float D = __builtin_sqrtf(D2);
        const f3 wc = cd * (1.0f / D);
        const float a = u1 * omc;
        const float cos_t = 1.0f - a;
        const float sin2 = a * (2.0f - a);
        const float sin_t = __builtin_sqrtf(sin2);
        float sp, cp;
        sincosf(PRT_TWO_PI * u2, &sp, &cp);
        // orthonormal frame about wc (Duff et al. 2017)
        const float sg = __builtin_copysignf(1.0f, wc.z);
        const float ia = -1.0f / (sg + wc.z);
        const float b = wc.x * wc.y * ia;
        const f3 t1 = mk3(1.0f + sg * wc.x * wc.x * ia, sg * b, -sg * wc.x);
        const f3 t2 = mk3(b, sg + wc.y * wc.y * ia, -wc.y);
        s.w = (t1 * (sin_t * cp) + t2 * (sin_t * sp)) + wc * cos_t;
        // near intersection along w, D cos - sqrt(R^2 - D^2 sin^2), in the form without cancellation (product of the roots)
        const float h = L0.w * L0.w - D2 * sin2;
        t_light = (D2 - L0.w * L0.w) / (D * cos_t + __builtin_sqrtf(h > 0.0f ? h : 0.0f));
        pdf_w = 1.0f / (PRT_TWO_PI * omc);
    }
    s.t_light = t_light;
    s.tmax = t_light * (1.0f - PRT_LIGHT_SHADOW_EPS);
    s.pdf_l = (CLUS ? pmf_c : L1.w) * pdf_w;
    return s.pdf_l > 0.0f && s.pdf_l < 3.0e38f && s.tmax > 0.0f;
}

// MIS weight of a light sample with pdfs (pl, pb) under the context's mode: power heuristic, or 1 (NEE)
PRT_DEV float light_weight(uint32_t mode, float pl, float pb) {
    if (mode == (uint32_t)PRT_LIGHTING_NEE) return 1.0f;
    const float r = pb / pl;
    return 1.0f / (1.0f + r * r);
}

// Weight of the emission of analytic primitive `prim` met by a segment scattered at x by a Lambertian vertex with pdf pb
// (direction w, hit at distance^2 d2): 1 - w_L of the same pair; 1 for emitters outside the light set or where pL = 0.
// MESHL: `prim` is a global primitive index, analytic (< n_prims) or a triangle's.
// CLUS: the light's pmf is P_c(x) pmf_in of its cluster c, evaluated at the segment's origin x.
template <bool MESHL = false, bool CLUS = false>
PRT_DEV float bsdf_hit_weight(const DevLights& lt, uint32_t prim, f3 x, f3 w, float d2, float pb, const DevMeshLights* ml = nullptr,
                              uint32_t n_prims = 0u, const DevLightClusters* lc = nullptr) {
    const uint32_t li = (MESHL && prim >= n_prims) ? triangle_light(*ml, prim) : lt.prim_light[prim];
    if (li == 0xFFFFFFFFu) return 1.0f;
    const float4* L = lt.lights + PRT_LIGHT_F4 * li;
    float pmf = 0.0f;
    if (CLUS) {
        const float pin = lc->cand_pmf_in[li];
        if (!(pin > 0.0f)) return 1.0f;  // (outside the light set, or an empty interval inside its cluster)
        pmf = cluster_prob_at(*lc, x, lc->cand_cluster[li]) * pin;
    }
    const float pl = (CLUS ? pmf : L[1].w) * light_pdf_w<MESHL>(L[0], L[3], x, w, d2);
    if (!(pl > 0.0f)) return 1.0f;
    if (lt.mode == (uint32_t)PRT_LIGHTING_NEE) return 0.0f;
    const float r = pl / pb;  // pb = 0: r = inf, weight 0
    return 1.0f / (1.0f + r * r);
}

// Light sample of a Lambertian vertex (position x, shading normal n, albedo, throughput thr before its roulette) with the
// key of the path's state at the vertex.  false: no sample (pdf 0).  Otherwise s, pb = max(0, n.w) / pi, the weight wl and
// `contrib`, the clamped term a shadow ray (x, s.w, s.tmax) delivers if unoccluded (zero, and no shadow ray, if n.w <= 0).
template <bool MESHL = false, bool CLUS = false>
PRT_DEV bool light_sample_term(const DevLights& lt, f3 x, f3 n, f3 albedo, f3 thr, uint32_t key, float clamp, LightSample& s,
                               float& pb, float& wl, f3& contrib, const DevMeshLights* ml = nullptr, const DevLightClusters* lc = nullptr) {
    if (!sample_light<MESHL, CLUS>(lt, x, key, s, ml, lc)) return false;
    const float c = dot3(n, s.w);
    pb = (c > 0.0f ? c : 0.0f) * PRT_INV_PI;
    wl = light_weight(lt.mode, s.pdf_l, pb);
    contrib = mk3(0.0f, 0.0f, 0.0f);
    if (c > 0.0f) {
        contrib = ((thr * albedo) * s.le) * ((pb * wl) / s.pdf_l);
        if (clamp > 0.0f) {  // each delivered term is clamped on its own (PrtSampling.clamp)
            contrib.x = contrib.x > clamp ? clamp : contrib.x;
            contrib.y = contrib.y > clamp ? clamp : contrib.y;
            contrib.z = contrib.z > clamp ? clamp : contrib.z;
        }
    }
    return true;
}

// ---- environment light (include/prt.h "Environment light") ----
// The environment-or-lights draw of the vertex with path state `key`: true = this vertex's light sample goes to the image.
PRT_DEV bool env_selected(const DevEnv& env, uint32_t key) {
    const uint32_t re = pcg_hash(key + PRT_ENV_RNG);
    return env.t_all != 0u || re < env.t_env;
}

// smallest i in [0, last] with r < thr[i], else last (the last entry's threshold, 2^32, is implicit): ceil(log2(last + 1))
// dependent loads from a table the L2 holds
PRT_DEV uint32_t env_search(const uint32_t* __restrict__ thr, uint32_t last, uint32_t r) {
    uint32_t lo = 0u, hi = last;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r < thr[mid]) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

// One environment sample with the draws of key's light stream: texel by the row and column thresholds, direction uniform
// in (u, v) inside the texel.  Le is the sampled texel's (no second lookup); tmax = +inf.  false: no sample (pdf 0).
PRT_DEV bool sample_environment(const DevEnv& env, uint32_t key, LightSample& s) {
    uint32_t ls = pcg_hash(key + PRT_LIGHT_RNG);
    ls = pcg_hash(ls);
    const uint32_t i = env_search(env.row_thr, env.row_last, ls);
    ls = pcg_hash(ls);
    const uint32_t j = env_search(env.col_thr + (size_t)i * env.W, env.col_last[i], ls);
    const float u1 = rnd01(ls);
    const float u2 = rnd01(ls);
    const float4 t = env.texels[(size_t)i * env.W + j];
    const float u = ((float)j + u1) / (float)env.W;
    const float v = ((float)i + u2) / (float)env.H;
    float sp, cp, st, ct;
    sincosf(__builtin_fmaf(PRT_TWO_PI, u, -3.14159265358979324f), &sp, &cp);
    sincosf(3.14159265358979324f * v, &st, &ct);
    s.w = mk3(st * cp, ct, st * sp);
    s.t_light = __builtin_inff();
    s.tmax = __builtin_inff();
    s.le = mk3(t.x, t.y, t.z);
    s.light = PRT_LIGHT_ENVIRONMENT;
    s.pdf_l = st > 0.0f ? env.p_env * (t.w / st) : 0.0f;
    return s.pdf_l > 0.0f && s.pdf_l < 3.0e38f;
}

// light_sample_term for the environment sample: the same estimator, weight and clamp
PRT_DEV bool env_sample_term(const DevEnv& env, uint32_t mode, f3 n, f3 albedo, f3 thr, uint32_t key, float clamp, LightSample& s,
                             float& pb, float& wl, f3& contrib) {
    if (!sample_environment(env, key, s)) return false;
    const float c = dot3(n, s.w);
    pb = (c > 0.0f ? c : 0.0f) * PRT_INV_PI;
    wl = light_weight(mode, s.pdf_l, pb);
    contrib = mk3(0.0f, 0.0f, 0.0f);
    if (c > 0.0f) {
        contrib = ((thr * albedo) * s.le) * ((pb * wl) / s.pdf_l);
        if (clamp > 0.0f) {
            contrib.x = contrib.x > clamp ? clamp : contrib.x;
            contrib.y = contrib.y > clamp ? clamp : contrib.y;
            contrib.z = contrib.z > clamp ? clamp : contrib.z;
        }
    }
    return true;
}

// Radiance of a miss along d and its weight after a Lambertian vertex that scattered with pdf pb (pb < 0: the camera, or a
// metal / dielectric vertex: weight 1): 1 - w_L of the same pair; 1 where the environment cannot sample d (pL = 0).
PRT_DEV f3 env_miss(const DevEnv& env, uint32_t mode, f3 d, float pb, float& wb) {
    float pdf_w;
    const f3 le = env_radiance(env, d, pdf_w);
    wb = 1.0f;
    if (pb >= 0.0f) {
        const float pl = env.p_env * pdf_w;
        if (pl > 0.0f) {
            const float r = pl / pb;  // pb = 0: r = inf, weight 0
            wb = mode == (uint32_t)PRT_LIGHTING_NEE ? 0.0f : 1.0f / (1.0f + r * r);
        }
    }
    return le;
}

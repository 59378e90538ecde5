// prt_kernels.hip — hand-written HIP kernels of the wavefront path tracer for gfx950 (MI355X).
//
// Pipeline per sample batch (one batch = `S` samples per local pixel in flight):
//   k_raygen -> [ k_intersect -> k_shade ] x max_depth -> k_accumulate
// replacing GenerateCameraRaysKernel / IntersectClosestKernel / ShadeHitsKernel / BlitRadianceKernel +
// addBufferGPU of the reference (src/backend/cuda_wavefront/renderer.cu:186-348, src/core/film.cu:79-88).
//
// Layout decisions:
//  * ray records are DENSE per bounce (structure of float4 arrays, slot k of bounce d), so every
//    kernel reads coalesced 16-B/lane streams; the reference gathers per-pixel state through a queue of
//    pixel indices instead (renderer.cu:226-228).
//  * the hit buffer is one u32 per ray slot (primitive id); the shade kernel re-derives position/normal
//    with the same device function the traversal used, so nothing else crosses HBM.
//  * wave64 ballot compaction into the next bounce's buffer: one atomic per 1024-thread block.
#include "prt_kernels.h"

#include "prt_adaptive.h"
#include "prt_device.h"

#define HIT_MISS 0xFFFFFFFFu
#define HIT_DEAD 0xFFFFFFFEu

// Blocks are dealt round-robin over the 8 XCDs (b and b+8 share an XCD's L2).  Give each XCD a
// contiguous run of logical blocks so neighbouring rays (= neighbouring BVH subtrees) share an L2.
// Bijective for every n.  Speed only; correctness never depends on placement.
PRT_DEV uint32_t xcd_remap(uint32_t b, uint32_t n) {
    const uint32_t q = n >> 3, r = n & 7u;
    const uint32_t xcd = b & 7u, i = b >> 3;
    const uint32_t start = xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
    return start + i;
}

// ---------------------------------------------------------------------------------------------------------
// Two-sided ray buffers.  Every producer (k_raygen, k_shade) classifies the ray it emits: rays that can still
// hit a triangle (they enter the BVH root box before their analytic hit) are packed from the FRONT of the next
// buffer, all others from the BACK.  The traversal kernel only sees the front part; the shade kernel sees both.
// Per bounce d: counts[d*64] = front count A_d, counts[d*64 + 32] = back count B_d (separate 128-B lines).
// ---------------------------------------------------------------------------------------------------------
#define CNT_STRIDE PRT_CNT_STRIDE
#define CNT_A(c, d) (c)[(d) * CNT_STRIDE]
#define CNT_B(c, d) (c)[(d) * CNT_STRIDE + 32u]
#define CNT_C(c, d) (c)[(d) * CNT_STRIDE + 16u]
#define PRODUCER_BLOCK 1024  // k_raygen
#ifndef SHADE_BLOCK
#define SHADE_BLOCK 512      // k_shade: its variants with 82 SGPRs / 78 VGPRs keep 6 waves per SIMD this way (1024: 4)
#endif

// Slot reservation for a BLOCK-thread block with ONE atomic per side (a counter word sustains only ~88
// returning atomics/us, MI355X_MICROARCH.md "dequeue"; the per-wave form — the wave64 equivalent of the
// reference's warp-aggregated AllocateSlot, renderer.cu:43-67 — costs ~0.9 ms per 8 M rays).
// Returns the buffer slot for this thread, or 0xFFFFFFFF if it emits nothing.  All threads must call.
// A kernel that calls this MORE THAN ONCE per block must put a __syncthreads() between two calls: the per-wave counts
// s_a/s_b/s_c are read by the other waves after the second barrier below, and a wave that ran ahead into the next call
// would overwrite its own entries under them (k_raygen's jitter loop does; k_shade calls once).
// `mult` (block-uniform) reserves that many slots per emitting thread.  With *stride (the block's emitting threads) copy j
// of a thread's ray can go to the returned slot + j * *stride (front) or - j * *stride (back), so that every copy index
// forms one contiguous run; with *base (where the block's reservation starts) the caller can instead give each thread
// `mult` consecutive slots: base + (slot - base) * mult + j (k_raygen's pixel-major order).
template <int BLOCK>
PRT_DEV uint32_t block_alloc2(bool front, bool back, bool done, uint32_t* cntA, uint32_t* cntB, uint32_t* cntC,
                              uint32_t cap, uint32_t mult = 1u, uint32_t* stride = nullptr, uint32_t* base = nullptr) {
    __shared__ uint32_t s_a[BLOCK / 64], s_b[BLOCK / 64], s_c[BLOCK / 64];
    __shared__ uint32_t s_base_a, s_base_b, s_tot_a, s_tot_b;
    const unsigned long long ma = __ballot(front), mb = __ballot(back), mc = __ballot(done);
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_a[wave] = (uint32_t)__popcll(ma);
        s_b[wave] = (uint32_t)__popcll(mb);
        s_c[wave] = (uint32_t)__popcll(mc);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ta = 0, tb = 0, tc = 0;
        for (uint32_t w = 0; w < BLOCK / 64; ++w) {
            ta += s_a[w];
            tb += s_b[w];
            tc += s_c[w];
        }
        s_base_a = ta ? atomicAdd(cntA, ta * mult) : 0u;
        s_base_b = tb ? atomicAdd(cntB, tb * mult) : 0u;
        if (tc) atomicAdd(cntC, tc);  // ray segments finished inside the producer: counted, never stored
        s_tot_a = ta;
        s_tot_b = tb;
    }
    __syncthreads();
    uint32_t slot = 0xFFFFFFFFu;
    if (front) {
        uint32_t j = s_base_a + (uint32_t)__popcll(ma & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; ++w) j += s_a[w];
        slot = j;
        if (stride) *stride = s_tot_a;
        if (base) *base = s_base_a;
    } else if (back) {
        uint32_t j = s_base_b + (uint32_t)__popcll(mb & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; ++w) j += s_b[w];
        slot = cap - 1u - j;
        if (stride) *stride = s_tot_b;
        if (base) *base = s_base_b;
    }
    return slot;
}

// The same reservation for K rays per thread with ONE atomic per side per block (k_raygen with jittered primary rays:
// a counter word executes ~87 returning atomics per microsecond whatever the block size, tools/atomic_rate.hip, so a
// kernel cannot retire more than 87 reserving blocks per microsecond; K rays per reservation divide that floor and the
// two barriers by K).  Within a wave ray k of every lane comes before ray k + 1.  Same contract as block_alloc2.
template <int BLOCK, int K>
PRT_DEV void block_alloc2k(const bool (&front)[K], const bool (&back)[K], uint32_t* cntA, uint32_t* cntB, uint32_t cap,
                           uint32_t (&slot)[K]) {
    __shared__ uint32_t s_a[BLOCK / 64], s_b[BLOCK / 64];
    __shared__ uint32_t s_base_a, s_base_b;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t ja[K], jb[K], na = 0, nb = 0;  // offsets of the lane's rays within the wave's reservation
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long ma = __ballot(front[k]), mb = __ballot(back[k]);
        ja[k] = na + (uint32_t)__popcll(ma & below);
        jb[k] = nb + (uint32_t)__popcll(mb & below);
        na += (uint32_t)__popcll(ma);
        nb += (uint32_t)__popcll(mb);
    }
    if (lane == 0) {
        s_a[wave] = na;
        s_b[wave] = nb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ta = 0, tb = 0;
        for (uint32_t w = 0; w < BLOCK / 64; ++w) {
            ta += s_a[w];
            tb += s_b[w];
        }
        s_base_a = ta ? atomicAdd(cntA, ta) : 0u;
        s_base_b = tb ? atomicAdd(cntB, tb) : 0u;
    }
    __syncthreads();
    uint32_t wa = s_base_a, wb = s_base_b;
    for (uint32_t w = 0; w < wave; ++w) {
        wa += s_a[w];
        wb += s_b[w];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) slot[k] = front[k] ? wa + ja[k] : back[k] ? cap - 1u - (wb + jb[k]) : 0xFFFFFFFFu;
}

// ---------------------------------------------------------------------------------------------------------
// Tile map: 8x8-pixel tiles, tile t (row-major) belongs to rank t % world.
// ---------------------------------------------------------------------------------------------------------
PRT_DEV bool tile_pixel(const PrtTileMap& tm, uint32_t pl, uint32_t& x, uint32_t& y) {
    const uint32_t lt = pl >> 6, lane = pl & 63u;
    const uint32_t gt = lt * tm.world + tm.rank;
    const uint32_t tx = gt % tm.tiles_x, ty = gt / tm.tiles_x;
    x = tx * 8u + (lane & 7u);
    y = ty * 8u + (lane >> 3);
    return gt < tm.tiles_x * tm.tiles_y && x < tm.W && y < tm.H;
}

// The primary ray of path i (no jitter: the pixel centre, cpu/renderer.cpp:45) as k_raygen computed it for the path's
// pixel (PrtPrimary, prt_kernels.h): path id -> (sample, local pixel) in the batch's id order (prt_path_id.h) -> the pixel's record.
PRT_DEV void primary_ray(const PrtPrimary& pr, uint32_t i, f3& o, f3& d, uint32_t& pixel, uint32_t& sample, uint32_t* local_pixel = nullptr) {
    uint32_t r;
    prt_path_id_decode(pr.ids, i, r, sample);
    if (local_pixel) *local_pixel = r;
    const float4 P = pr.pix[r];
    o = mk3(pr.origin[0], pr.origin[1], pr.origin[2]);
    d = mk3(P.x, P.y, P.z);
    pixel = __float_as_uint(P.w);
}

// ---------------------------------------------------------------------------------------------------------
// Ray generation (GenerateCameraRaysKernel, renderer.cu:186-204; pixel centres, cpu/renderer.cpp:45)
// ---------------------------------------------------------------------------------------------------------
template <bool ABVH, int BLOCK>
__device__ bool classify_ray(const DevScene& sc, f3 o, f3 d, uint32_t& id0, float& d2_0);
__device__ bool ends_here(const DevScene& sc, bool front, uint32_t id0, f3 thr, f3& L);

// Fused analytic segments.  A ray that cannot hit a triangle (it does not enter the BVH root box before its closest
// analytic hit) is fully determined by the producer's own scan, so the producer shades it in place and goes on with
// the scattered ray, FUSE segments per kernel call: such rays are never stored or re-read (C3: 62 % of all segments).
// FUSE is a compile-time 0 or 1 and the steps are straight-line code: as a run-time loop the same body needs 94 instead
// of 63 VGPRs (loop-invariant operand copies stay live across the back edge), which halves the occupancy of these
// memory-bound kernels and costs more than the fusion saves (measured); one fused segment already gives all of the
// gain (a second one changes nothing).  k_shade fuses (512-thread blocks: 78 VGPRs / 82 SGPRs = 6 waves per SIMD;
// shade 76 -> 57 ms per 1024 spp on C3); k_raygen does not (its 8-samples-per-thread loop around the shading body needs
// 119 VGPRs and ran 2.4x slower fused): a primary ray that cannot hit a triangle is stored on the back side and
// continued by the first k_shade.  Paths therefore advance by different numbers of segments per bounce iteration; every stored ray
// carries its own segment index (depth) in throughput.w, and every path records the index of its LAST segment in
// rad.w when it ends: k_accumulate derives the per-depth ray counts from those (segments at depth d = paths whose
// last segment index is >= d), so the producers count nothing.
//   returns 0: the path ended here (rad written)   1: (o, d) must be traversed (front)
//           2: budget used up, (o, d) is stored with its known analytic hit id0 (back)
// ONE loop serves both producers: on entry `id` is the final closest hit of segment `depth` = (o, d) over all
// primitives (from the traversal kernel in k_shade, from the primary ray's classification in k_raygen); `budget` is
// the number of segments this call may shade (k_shade: 1 + FUSE, k_raygen: FUSE).
// Radiance a path delivers, with the optional firefly clamp (PrtSampling.clamp; 0 = off).
PRT_DEV float4 path_result(f3 L, float clamp, uint32_t depth) {
    if (clamp > 0.0f) {
        L.x = L.x > clamp ? clamp : L.x;
        L.y = L.y > clamp ? clamp : L.y;
        L.z = L.z > clamp ? clamp : L.z;
    }
    return make_float4(L.x, L.y, L.z, __uint_as_float(depth));
}

// (the environment image's lookup, env_texel / env_radiance, is in prt_device.h: the radiance query's unit calls it too)

// PRE: (pre_a, pre_b) = the hit record k_primary_hit computed for this path's pixel: {position, hit id}, {normal, material
// | front face << 31}.  It replaces world_hit_from_id for the first segment when it was computed for the same hit id (it
// always was: all samples of a pixel trace the same primary ray; the comparison keeps the kernel correct by itself).
// ENV (env: DevEnv): a miss delivers the environment image's texel where it delivers the constant sky.
// TEX (tex: DevTex): the albedo of a vertex whose material is textured is the lookup at the hit's UV (k_shade_tex only).
// LASTSEG && last_route (PRT_LAST_SEGMENT_FLAG, run-time; the plan sets it only without fusion and without emissive triangles;
// LASTSEG = false compiles it out: k_raygen, the fusing k_shade instances and the path instance keep their code): a path's
// last segment delivers throughput x emission of its closest hit and nothing else.  Its producer ends it when the analytic
// scan's hit id0 does not emit: the closest hit is id0 or a triangle, throughput x 0 either way, so the ray is neither
// stored nor walked; only a miss or an emissive id0 that a triangle may block is.  Its consumer writes throughput x 0 for a
// triangle id without rebuilding the hit.  The products are the ones the full route forms (x the zero vector, not a literal
// zero: an infinite throughput gives the same NaN), with the same segment index.
template <int BUDGET, bool INST, bool ABVH, int BLOCK, bool PRE = false, bool ENV = false, bool TEX = false, bool LASTSEG = false>
PRT_DEV int advance_path(const DevScene& sc, uint32_t id, f3& o, f3& d, f3& thr, uint32_t& rng, uint32_t& depth,
                         uint32_t max_depth, const PrtSampling& sp, float4* __restrict__ rad_slot, uint32_t& id0,
                         float& d2_0, float4 pre_a = float4{0.f, 0.f, 0.f, 0.f}, float4 pre_b = float4{0.f, 0.f, 0.f, 0.f},
                         const DevEnv* env = nullptr, const DevTex* tex = nullptr, bool last_route = false) {
#pragma unroll
    for (int it = 0; it <= BUDGET; ++it) {
        if (id == HIT_MISS) {  // the miss branch of IntersectClosestKernel, renderer.cu:263-271
            st_stream(rad_slot, path_result(thr * (ENV ? env_radiance(*env, d) : mk3(sc.sky[0], sc.sky[1], sc.sky[2])), sp.clamp, depth));
            return 0;
        }
        if (LASTSEG && last_route && it == 0 && depth + 1u >= max_depth && id >= sc.n_prims) {  // a triangle ends the path and emits nothing
            st_stream(rad_slot, path_result(thr * mk3(0.f, 0.f, 0.f), sp.clamp, depth));
            return 0;
        }
        if (it == BUDGET) {  // only reached with an analytic id (the ray was classified "cannot hit a triangle")
            const uint32_t m = sc.prims[id].material;
            if (sc.mat_type[m] == 4u) {  // emissive: never scatters (material.h:119-122): the path stops here
                const float4 e = sc.mat_rgbs[m];
                st_stream(rad_slot, path_result(thr * mk3(e.x, e.y, e.z), sp.clamp, depth));
                return 0;
            }
            id0 = id;
            return 2;
        }
        WorldHit w;
        float uv[2] = {0.0f, 0.0f};
        if (PRE && it == 0 && __float_as_uint(pre_a.w) == id) {
            w.pos = mk3(pre_a.x, pre_a.y, pre_a.z);
            w.normal = mk3(pre_b.x, pre_b.y, pre_b.z);
            w.material = __float_as_uint(pre_b.w) & 0x7FFFFFFFu;
            w.front = (__float_as_uint(pre_b.w) >> 31) != 0u;
        } else if (TEX) {
            world_hit_from_id<INST, true>(sc, id, o, d, w, tex, uv);
        } else {
            world_hit_from_id<INST>(sc, id, o, d, w);
        }
        const uint32_t type = sc.mat_type[w.material];
        const float4 rgbs = TEX ? textured_rgbs(sc, *tex, w.material, uv) : sc.mat_rgbs[w.material];
        f3 atten, emitted, so, sd;
        bool scattered = false;
        if (depth + 1u >= max_depth) {
            emitted = (type == 4u) ? mk3(rgbs.x, rgbs.y, rgbs.z) : mk3(0.f, 0.f, 0.f);
        } else {
            scattered = material_scatter(type, rgbs, d, w.pos, w.normal, w.front, rng, atten, emitted, so, sd);
        }
        if (!scattered) {
            st_stream(rad_slot, path_result(thr * emitted, sp.clamp, depth));
            return 0;
        }
        thr = thr * atten;
        o = so;
        d = normalize3(sd);  // scatteredRay.Normalize(), cpu/renderer.cpp:84
        if (sp.rr_depth != 0u && depth + 1u >= sp.rr_depth) {  // Russian roulette (PrtSampling, include/prt.h)
            float p = thr.x > thr.y ? thr.x : thr.y;
            p = p > thr.z ? p : thr.z;
            p = p > 1.0f ? 1.0f : p;
            p = p < 0.05f ? 0.05f : p;
            if (!(rnd01(rng) < p)) {
                st_stream(rad_slot, path_result(mk3(0.f, 0.f, 0.f), 0.0f, depth));
                return 0;
            }
            thr = mk3(thr.x / p, thr.y / p, thr.z / p);
        }
        ++depth;
        if (LASTSEG) {
            const bool front = classify_ray<ABVH, BLOCK>(sc, o, d, id0, d2_0);
            if (last_route && depth + 1u >= max_depth && id0 != HIT_MISS && sc.mat_type[sc.prims[id0].material] != 4u) {
                st_stream(rad_slot, path_result(thr * mk3(0.f, 0.f, 0.f), sp.clamp, depth));
                return 0;
            }
            if (front) return 1;
        } else if (classify_ray<ABVH, BLOCK>(sc, o, d, id0, d2_0)) return 1;
        id = id0;
    }
    return 2;  // not reached
}

// All S samples of a pixel start with the same pixel-centre ray (no jitter: cpu/renderer.cpp:45), so one thread
// computes the camera ray and its classification once and emits it for RAYGEN_GROUP samples, each with its own RNG
// seed and path id.  With compact primary rays the traversal kernel walks the ray once per pixel (PrtPrimary, walk = 1);
// on every other route each sample's primary ray is still traced on its own.
#define RAYGEN_GROUP 8
#ifndef RAYGEN_ALLOC
#define RAYGEN_ALLOC 4  // jittered rays per slot reservation (divides RAYGEN_GROUP)
#endif
#define RAYGEN_GROUP_NOJITTER 64u  // without jitter: one wave's worth of samples per pixel and block (pixel-major slots)
// SAMPLING = false compiles the Russian-roulette / clamp code out: with it in, k_shade needs 82 instead of 74 SGPRs,
// which costs a wave per SIMD, i.e. with 1024-thread blocks one of the two blocks per CU (measured: shade 50 % slower).
// (ENV / env: see advance_path; k_raygen passes false / null and compiles to the code it had before there was an environment
// image, k_raygen_env is the instance with one)
// LENS (lens: DevLens; PrtLens with aperture > 0): every sample has a primary ray of its own, from its own point of the lens,
// so LENS takes the per-sample branch below whether JITTER is on or not (off: the pixel centre) and stores each ray's own
// origin.  The other instances pass false and compile to the code they had before there was a lens.
// LIST (list: PrtBatchView, prt_kernels.h; k_raygen_list only): tm counts the listed tiles, pl is a compact local pixel, and
// only the pixel's place in the image comes from its own tile list[pl >> 6]; slots and path ids are made of compact pixels.
template <bool JITTER, bool SAMPLING, bool ABVH, bool COMPACT, bool ENV, bool LENS = false, bool LIST = false>
PRT_DEV void raygen_step(DevScene sc, DevCamera cam, PrtTileMap tm, uint32_t S, uint32_t first_sample, uint32_t seed,
                         float4* __restrict__ ro, float4* __restrict__ rd, float4* __restrict__ rt, uint32_t* __restrict__ hit,
                         float* __restrict__ hd2, float4* __restrict__ rad, uint32_t* __restrict__ counts,
                         uint32_t* __restrict__ work, uint32_t max_depth, PrtSampling sp_arg, float4* __restrict__ pix,
                         const DevEnv* env, const DevLens* lens = nullptr, const uint32_t* __restrict__ list = nullptr,
                         uint32_t pixel_major_ids = 0u) {
    const PrtSampling sp = SAMPLING ? sp_arg : PrtSampling{0u, 0u, 0.0f};
    // the batch's path ids (prt_path_id.h; encode only: no decode fields).  Pixel-major on the compact instance alone, where the
    // host asks for it: everywhere else S = 0 is a compile-time constant and the id is sample * n_pix_local + pixel as ever
    const PrtPathIdOrder ids{tm.n_pix_local, 0.0f, (COMPACT && pixel_major_ids) ? S : 0u, 0u, 0u};
    const uint32_t pl = blockIdx.x * (uint32_t)PRODUCER_BLOCK + threadIdx.x;
    if (blockIdx.y == 0 && pl < 8u) work[32u * pl] = 0u;  // chunk cursors of the traversal kernel that follows
    if (blockIdx.y == 0 && pl == 8u) work[512] = 0u;      // its overflow-list counter
    const uint32_t n_paths = S * tm.n_pix_local;
    const bool in_range = pl < tm.n_pix_local;
    bool valid = false, front0 = false;
    f3 o0 = mk3(0.f, 0.f, 0.f), d0 = mk3(0.f, 0.f, 1.f);
    uint32_t id00 = HIT_MISS, pixel = 0, px = 0, py = 0;
    float d2_00 = 3.402823466e+38f;
    if (in_range) {
        valid = tile_pixel(tm, LIST ? (list[pl >> 6] << 6) | (pl & 63u) : pl, px, py);
        if (valid) {
            pixel = py * tm.W + px;
            if (!JITTER && !LENS) {  // pixel centre, the same ray for every sample (cpu/renderer.cpp:45)
                camera_ray(cam, (float)px + 0.5f, (float)py + 0.5f, o0, d0);
                if (COMPACT && blockIdx.y == 0) pix[pl] = make_float4(d0.x, d0.y, d0.z, __uint_as_float(pixel));
                front0 = classify_ray<ABVH, PRODUCER_BLOCK>(sc, o0, d0, id00, d2_00);
            }
        }
    }
    const uint32_t group = (JITTER || LENS) ? RAYGEN_GROUP : RAYGEN_GROUP_NOJITTER;
    const uint32_t s0 = blockIdx.y * group;
    const uint32_t s1 = (s0 + group < S) ? s0 + group : S;
    if (!JITTER && !LENS) {
        // Without jitter whether the pixel's primary ray is stored (front / back) or ends right here does not depend
        // on the sample: decide once, reserve the slots of all samples of this group with ONE atomic per side per
        // block, and only the RNG seed and the path id differ per copy.
        f3 o = o0, d = d0, thr = mk3(1.f, 1.f, 1.f);
        uint32_t rng = 0, depth = 0, id0 = id00;
        float d2_0 = d2_00;
        float4 L0 = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));  // outside the image: no path
        bool front = false, back = false;
        if (valid) {
            front = front0;
            if (!front) {
                const int r = advance_path<0, false, ABVH, PRODUCER_BLOCK, false, ENV>(sc, id00, o, d, thr, rng, depth, max_depth, sp, &L0, id0, d2_0,
                                                                                         float4{0.f, 0.f, 0.f, 0.f}, float4{0.f, 0.f, 0.f, 0.f}, env);
                back = r == 2;
            }
        }
        uint32_t stride = 0, base = 0;
        const uint32_t slot0 = block_alloc2<PRODUCER_BLOCK>(front, back, false, &CNT_A(counts, 0), &CNT_B(counts, 0),
                                                            &CNT_C(counts, 0), n_paths, s1 - s0, &stride, &base);
        uint32_t first_slot = slot0;  // slot of this pixel's sample s0
        // One walk per pixel (PrtPrimary, walk = 1; hd2 is then the list, else null): the block's front pixels go on the
        // dense list the first traversal runs over, in the order block_alloc2 ranked them (its ballots; one more atomic
        // per block).  Entry = the local pixel index = the sample-major path id of the pixel's sample 0, which is how the walk
        // decodes it whatever the batch's own id order (PrtPrimary.ids).
        const bool walk = COMPACT && hd2 != nullptr;
        uint32_t list_slot = 0xFFFFFFFFu;  // (what a stored back pixel's record carries)
        if (walk && blockIdx.y == 0) {  // block-uniform
            __shared__ uint32_t s_list_base;
            if (front && slot0 == base) s_list_base = atomicAdd(&counts[PRT_CNT_LIST], stride);
            __syncthreads();
            if (front) {
                list_slot = s_list_base + (slot0 - base);
                ((uint32_t*)hd2)[list_slot] = pl;
            }
        }
        if (s1 - s0 < PRT_PATH_ID_MIN_SAMPLES) {
            // few samples per pixel in this batch (interactive use: ProgressiveRender adds ONE sample per call): SAMPLE-major
            // slots, every thread stores its own pixel's copies, coalesced across the pixels of a wave
            if (in_range && slot0 != 0xFFFFFFFFu) {
                for (uint32_t sl = s0; sl < s1; ++sl) {
                    const uint32_t i = prt_path_id_encode(ids, pl, sl);  // path id
                    const uint32_t slot = front ? slot0 + (sl - s0) * stride : slot0 - (sl - s0) * stride;
                    if (COMPACT) {
                        ((uint32_t*)rt)[slot] = i;
                    } else {
                        ro[slot] = make_float4(o.x, o.y, o.z, __uint_as_float(i));
                        rd[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(path_seed(pixel, first_sample + sl, seed)));
                        rt[slot] = make_float4(1.f, 1.f, 1.f, __uint_as_float(0u));
                    }
                    if (!COMPACT) {  // (compact: the analytic scan's result is the pixel's, in its end record)
                        hit[slot] = id0;
                        hd2[slot] = d2_0;
                    }
                }
            }
        } else {
            // PIXEL-major slots: the (up to 64) samples of a pixel that this block handles sit next to each other, so a
            // wave of the first bounce's traversal / k_shade works on IDENTICAL rays: no divergence in the node loop (and,
            // with placed copies, level switches in lockstep), one cache line per node for the whole wave, one triangle /
            // one material per wave in k_shade.  (Full records: each of them is traced on its own; compact: the first
            // traversal walks the front-pixel list instead, one ray per pixel.)  Written wave-transposed (pixel
            // by pixel, one sample per lane): 256-B stores of path ids (COMPACT) or 1-KB stores of full records.
            const uint32_t mult = s1 - s0;
            const bool stored = slot0 != 0xFFFFFFFFu;
            // slot of the pixel's first sample: rank among the block's stored pixels x mult, from the block's base
            uint32_t first = 0u;
            if (front) first = base + (slot0 - base) * mult;
            if (back) first = n_paths - 1u - (base + ((n_paths - 1u - slot0) - base) * mult);
            first_slot = first;
            const uint32_t lane = lane_id();
            for (unsigned long long m = __ballot(stored); m; m &= m - 1ull) {
                const int p = __builtin_ctzll(m);
                const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)first, p);
                const bool fr = __builtin_amdgcn_readlane((int)front, p) != 0;
                const uint32_t plp = (uint32_t)__builtin_amdgcn_readlane((int)pl, p);
                const uint32_t idp = (uint32_t)__builtin_amdgcn_readlane((int)id0, p);
                const float d2p = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(d2_0), p));
                float4 Op = make_float4(0.f, 0.f, 0.f, 0.f), Dp = Op;
                uint32_t pixp = 0u;
                if (!COMPACT) {
#define PRT_RL(X) __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(X), p))
                    Op = make_float4(PRT_RL(o.x), PRT_RL(o.y), PRT_RL(o.z), 0.f);
                    Dp = make_float4(PRT_RL(d.x), PRT_RL(d.y), PRT_RL(d.z), 0.f);
#undef PRT_RL
                    pixp = (uint32_t)__builtin_amdgcn_readlane((int)pixel, p);
                }
                if (lane < mult) {
                    const uint32_t slot = fr ? f + lane : f - lane;
                    const uint32_t i = prt_path_id_encode(ids, plp, s0 + lane);  // path id
                    if (COMPACT) {  // 12 B per path: bounce 0 rebuilds the rest from the path id (PrtPrimary)
                        ((uint32_t*)rt)[slot] = i;
                    } else {
                        ro[slot] = make_float4(Op.x, Op.y, Op.z, __uint_as_float(i));
                        rd[slot] = make_float4(Dp.x, Dp.y, Dp.z, __uint_as_float(path_seed(pixp, first_sample + s0 + lane, seed)));
                        rt[slot] = make_float4(1.f, 1.f, 1.f, __uint_as_float(0u));
                    }
                    if (!COMPACT) {
                        hit[slot] = idp;
                        hd2[slot] = d2p;
                    }
                }
            }
        }
        {
            const bool stored = slot0 != 0xFFFFFFFFu;
            if (COMPACT) {
                // whether the pixel's paths end with their primary ray, and with what, is the same for all its samples: one
                // record per pixel (w = 0xFFFFFFFE: they go on, look in rad[]) instead of S copies in rad[]
                // (a "they go on" record: x = where the pixel's walked hit will be, for k_primary_hit and the first k_shade:
                // the pixel's list slot, 0xFFFFFFFF for a back pixel (one walk per sample: the ray slot of the pixel's first
                // stored sample); y, z = the analytic scan's closest hit and its distance^2, the same for every sample of
                // the pixel: the paths' slots carry the path id only, 4 B instead of 12)
                if (in_range && blockIdx.y == 0)
                    pix[tm.n_pix_local + pl] = stored ? make_float4(__uint_as_float(walk ? list_slot : first_slot), __uint_as_float(id0), d2_0, __uint_as_float(0xFFFFFFFEu)) : L0;
            } else if (in_range && !stored) {
                // the path ended with its primary ray (sky / light seen directly), or there is none
                for (uint32_t sl = s0; sl < s1; ++sl) rad[sl * tm.n_pix_local + pl] = L0;
            }
        }
        return;
    }
    // Jittered primary rays, RAYGEN_ALLOC samples of the pixel per slot reservation.  What is stored per ray is its
    // direction, RNG state and the analytic scan's result: with no shading budget advance_path never scatters, so the origin
    // stays the camera position, the throughput 1 and the segment index 0 (paths that end right here write rad[] inside).
    // LENS: the origin is the ray's own point of the lens, kept per ray next to its direction.
    // (with 4 rays per reservation the lens instances need 101-105 VGPRs, a wave per SIMD less than the jittered ones at 93-96)
    constexpr int KA = (ABVH || LENS) ? 2 : RAYGEN_ALLOC;  // (the primitive-BVH walk needs the registers: 4 rays would spill)
    for (uint32_t sl = s0; sl < s1; sl += KA) {  // block-uniform trip count
        f3 dk[KA];
        f3 ok[KA];  // (LENS only)
        uint32_t rngk[KA], idk[KA], slotk[KA];
        float d2k[KA];
        bool frontk[KA], backk[KA];
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) {
            const uint32_t sk = sl + (uint32_t)kk;
            const uint32_t i = sk * tm.n_pix_local + pl;  // path id
            f3 o = o0, d = d0, thr = mk3(1.f, 1.f, 1.f);
            uint32_t rng = 0, depth = 0, id0 = id00;
            float d2_0 = d2_00;
            bool front = false, back = false;
            if (sk < s1 && valid) {
                rng = path_seed(pixel, first_sample + sk, seed);
                {  // (x + u1, y + u2): the path's first two draws (optix/device_programs.cu:172-173)
                    const float u1 = JITTER ? rnd01(rng) : 0.5f;
                    const float u2 = JITTER ? rnd01(rng) : 0.5f;
                    if (LENS)  // then the two lens draws (PrtLens, include/prt.h)
                        lens_camera_ray(cam, *lens, (float)px + u1, (float)py + u2, rng, o, d);
                    else
                        camera_ray(cam, (float)px + u1, (float)py + u2, o, d);
                    front = classify_ray<ABVH, PRODUCER_BLOCK>(sc, o, d, id0, d2_0);
                }
                if (!front) {
                    const int r = advance_path<0, false, ABVH, PRODUCER_BLOCK, false, ENV>(sc, id0, o, d, thr, rng, depth, max_depth, sp, &rad[i], id0, d2_0,
                                                                                             float4{0.f, 0.f, 0.f, 0.f}, float4{0.f, 0.f, 0.f, 0.f}, env);
                    front = r == 1;
                    back = r == 2;
                }
            } else if (sk < s1 && in_range) {
                rad[i] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));  // partial tiles outside the image: no path
            }
            dk[kk] = d;
            if (LENS) ok[kk] = o;
            rngk[kk] = rng;
            idk[kk] = id0;
            d2k[kk] = d2_0;
            frontk[kk] = front;
            backk[kk] = back;
        }
        block_alloc2k<PRODUCER_BLOCK, KA>(frontk, backk, &CNT_A(counts, 0), &CNT_B(counts, 0), n_paths, slotk);
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) {
            const uint32_t slot = slotk[kk];
            if (slot != 0xFFFFFFFFu) {
                const uint32_t i = (sl + (uint32_t)kk) * tm.n_pix_local + pl;
                const f3 ok_ = LENS ? ok[kk] : cam.pos;
                ro[slot] = make_float4(ok_.x, ok_.y, ok_.z, __uint_as_float(i));
                rd[slot] = make_float4(dk[kk].x, dk[kk].y, dk[kk].z, __uint_as_float(rngk[kk]));
                rt[slot] = make_float4(1.f, 1.f, 1.f, __uint_as_float(0u));
                hit[slot] = idk[kk];
                hd2[slot] = d2k[kk];
            }
        }
        __syncthreads();  // block_alloc2k's LDS counts are reused by the next trip (see block_alloc2's contract)
    }
}

template <bool JITTER, bool SAMPLING, bool ABVH, bool COMPACT = false>
__global__ void __launch_bounds__(PRODUCER_BLOCK) k_raygen(DevScene sc, DevCamera cam, PrtTileMap tm, uint32_t S,
                                                            uint32_t first_sample, uint32_t seed,
                                                            float4* __restrict__ ro, float4* __restrict__ rd,
                                                            float4* __restrict__ rt, uint32_t* __restrict__ hit,
                                                            float* __restrict__ hd2, float4* __restrict__ rad,
                                                            uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                            uint32_t max_depth, PrtSampling sp_arg, float4* __restrict__ pix,
                                                            uint32_t pixel_major_ids) {
    // (pixel_major_ids: read by the COMPACT instance only)
    raygen_step<JITTER, SAMPLING, ABVH, COMPACT, false>(sc, cam, tm, S, first_sample, seed, ro, rd, rt, hit, hd2, rad, counts, work,
                                                        max_depth, sp_arg, pix, nullptr, nullptr, nullptr, COMPACT ? pixel_major_ids : 0u);
}

// k_raygen under an environment image (prt_set_environment): full ray records always, sampling options compiled in
template <bool JITTER, bool ABVH>
__global__ void __launch_bounds__(PRODUCER_BLOCK) k_raygen_env(DevScene sc, DevEnv env, DevCamera cam, PrtTileMap tm, uint32_t S,
                                                                uint32_t first_sample, uint32_t seed,
                                                                float4* __restrict__ ro, float4* __restrict__ rd,
                                                                float4* __restrict__ rt, uint32_t* __restrict__ hit,
                                                                float* __restrict__ hd2, float4* __restrict__ rad,
                                                                uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                                uint32_t max_depth, PrtSampling sp_arg) {
    raygen_step<JITTER, true, ABVH, false, true>(sc, cam, tm, S, first_sample, seed, ro, rd, rt, hit, hd2, rad, counts, work,
                                                 max_depth, sp_arg, nullptr, &env);
}

// k_raygen with a thin lens (prt_set_lens with aperture > 0): one full ray record per sample with the ray's own origin,
// sampling options compiled in; with an environment image: k_raygen_lens_env
template <bool JITTER, bool ABVH>
__global__ void __launch_bounds__(PRODUCER_BLOCK) k_raygen_lens(DevScene sc, DevLens lens, DevCamera cam, PrtTileMap tm, uint32_t S,
                                                                 uint32_t first_sample, uint32_t seed,
                                                                 float4* __restrict__ ro, float4* __restrict__ rd,
                                                                 float4* __restrict__ rt, uint32_t* __restrict__ hit,
                                                                 float* __restrict__ hd2, float4* __restrict__ rad,
                                                                 uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                                 uint32_t max_depth, PrtSampling sp_arg) {
    raygen_step<JITTER, true, ABVH, false, false, true>(sc, cam, tm, S, first_sample, seed, ro, rd, rt, hit, hd2, rad, counts, work,
                                                        max_depth, sp_arg, nullptr, nullptr, &lens);
}
template <bool JITTER, bool ABVH>
__global__ void __launch_bounds__(PRODUCER_BLOCK) k_raygen_lens_env(DevScene sc, DevEnv env, DevLens lens, DevCamera cam, PrtTileMap tm,
                                                                     uint32_t S, uint32_t first_sample, uint32_t seed,
                                                                     float4* __restrict__ ro, float4* __restrict__ rd,
                                                                     float4* __restrict__ rt, uint32_t* __restrict__ hit,
                                                                     float* __restrict__ hd2, float4* __restrict__ rad,
                                                                     uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                                     uint32_t max_depth, PrtSampling sp_arg) {
    raygen_step<JITTER, true, ABVH, false, true, true>(sc, cam, tm, S, first_sample, seed, ro, rd, rt, hit, hd2, rad, counts, work,
                                                       max_depth, sp_arg, nullptr, &env, &lens);
}

// k_raygen for the tiles of a list (a pass of prt_render_adaptive; PrtBatchView): one full ray record per sample, sampling
// options compiled in, every combination of jitter, primitive BVH, environment image and thin lens in one kernel name
template <bool JITTER, bool ABVH, bool ENV, bool LENS>
__global__ void __launch_bounds__(PRODUCER_BLOCK) k_raygen_list(DevScene sc, DevEnv env, DevLens lens, DevCamera cam, PrtTileMap tm,
                                                                 const uint32_t* __restrict__ list, uint32_t S,
                                                                 uint32_t first_sample, uint32_t seed,
                                                                 float4* __restrict__ ro, float4* __restrict__ rd,
                                                                 float4* __restrict__ rt, uint32_t* __restrict__ hit,
                                                                 float* __restrict__ hd2, float4* __restrict__ rad,
                                                                 uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                                 uint32_t max_depth, PrtSampling sp_arg) {
    raygen_step<JITTER, true, ABVH, false, ENV, LENS, true>(sc, cam, tm, S, first_sample, seed, ro, rd, rt, hit, hd2, rad, counts, work,
                                                            max_depth, sp_arg, nullptr, ENV ? &env : nullptr, LENS ? &lens : nullptr,
                                                            list);
}

// ---------------------------------------------------------------------------------------------------------
// Closest hit (IntersectClosestKernel, renderer.cu:206-272; semantics of PrimitiveList::Intersect,
// src/core/primitive.cpp:21-59): linear scan over the analytic primitives + BVH2 traversal over all
// mesh triangles.  The result equals the reference's linear scan over every primitive: the winner is the
// smallest world distance^2, ties to the lowest primitive index, independent of visiting order.
// ---------------------------------------------------------------------------------------------------------
struct Closest {
    float d2;
    uint32_t id;    // hit id (analytic index, or n_prims + leaf slot)
    uint32_t prim;  // global primitive index (tie-break key)
};

PRT_DEV float limit_from_d2(float d2, float pad) {
    // Upper bound on the local ray parameter of anything that could still win (d2' <= d2).
    return (d2 < 3.0e38f) ? __builtin_sqrtf(d2) * 1.0000153f + 4.0f * pad : 3.4e38f;
}

#define ABVH_STACK 20  // entries of the primitive walk's stack (4-wide tree: at most 3 net pushes per level)
// Closest hit over the analytic primitives.  ABVH = false: the reference's linear scan (primitive.cpp:26-49).
// ABVH = true: a per-thread walk of a 4-wide BVH over the primitives' WORLD boxes (valid because every primitive of
// the scene has a rotation + uniform scale + translation transform, checked on the host: only then is the reference's
// local ray, primitive.cpp:29-30, the geometric ray and the hit lies inside the shape's world box).  Each primitive
// the walk reaches is tested with the reference's own arithmetic and candidates compete on (d2, primitive index), so
// the result equals the linear scan's bit for bit whatever the visiting order.
template <bool ABVH, int BLOCK = 1>
PRT_DEV void scan_analytic(const DevScene& sc, f3 o, f3 d, Closest& best, uint32_t& n_tests) {
    if (!ABVH) {
        for (uint32_t i = 0; i < sc.n_prims; ++i) {
            WorldHit w;
            analytic_hit(sc.prims[i], o, d, w);
            ++n_tests;
            if (w.has && w.d2 < best.d2) {  // strict <, first wins (primitive.cpp:44)
                best.d2 = w.d2;
                best.id = i;
                best.prim = i;
            }
        }
        return;
    }
    const f3 ld = normalize3(d);
    // The per-ray pad has a term that grows with the SQUARE of the distance: Circle::Intersect's discriminant
    // b*b - 4*a*c (shape.h:160-163) cancels catastrophically for a far origin, so a ray that passes up to
    // ~2e-7 * dist^2 / R outside a sphere can still be a hit of the reference's arithmetic (measured; 4.8e-7 is the
    // worst-case bound), which a world box padded in proportion to the distance alone would cull.
    const float A1 = __builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z);
    const float pad = sc.pad * (A1 + sc.extent) + ((sc.abvh_q[0] * A1 + sc.abvh_q[1]) * A1 + sc.abvh_q[2]);
    const float ix = 1.0f / (__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
    const float iy = 1.0f / (__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
    const float iz = 1.0f / (__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
    const float ax = (o.x + pad) * ix, ay = (o.y + pad) * iy, az = (o.z + pad) * iz;
    const float bx = (o.x - pad) * ix, by = (o.y - pad) * iy, bz = (o.z - pad) * iz;
    float tlimit = limit_from_d2(best.d2, pad);
    // per-thread stack in LDS, [entry][thread] (bank = lane: conflict-free): as a register array it costs 60 VGPRs
    __shared__ uint32_t s_astk[ABVH ? ABVH_STACK * BLOCK : 1];
    uint32_t* const stk = &s_astk[threadIdx.x];
    const uint32_t sstride = (uint32_t)BLOCK;
    int sp = 0;
    uint32_t node = 0;
    for (;;) {
        const float4* nb = sc.abvh_nodes + 8 * (size_t)node;
        const float4 mnx = nb[0], mxx = nb[1], mny = nb[2], mxy = nb[3], mnz = nb[4], mxz = nb[5], rf = nb[6];
#define ABVH_CHILD(C)                                                                                              \
    {                                                                                                              \
        const float x0 = __builtin_fmaf(mnx.C, ix, -ax), x1 = __builtin_fmaf(mxx.C, ix, -bx);                      \
        const float y0 = __builtin_fmaf(mny.C, iy, -ay), y1 = __builtin_fmaf(mxy.C, iy, -by);                      \
        const float z0 = __builtin_fmaf(mnz.C, iz, -az), z1 = __builtin_fmaf(mxz.C, iz, -bz);                      \
        const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(x0, x1), __builtin_fminf(y0, y1)),        \
                                         __builtin_fmaxf(__builtin_fminf(z0, z1), 0.0f));                          \
        const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(x0, x1), __builtin_fmaxf(y0, y1)),        \
                                         __builtin_fminf(__builtin_fmaxf(z0, z1), tlimit));                        \
        if (tn <= tf * 1.0000005f) {                                                                               \
            const int ref = __float_as_int(rf.C);                                                                  \
            if (ref >= 0) {                                                                                        \
                stk[(sp++) * sstride] = (uint32_t)ref;                                                             \
            } else {                                                                                               \
                const uint32_t lr = ~(uint32_t)ref, first = lr >> 4, cnt = lr & 15u;                               \
                for (uint32_t k = 0; k < cnt; ++k) {                                                               \
                    const uint32_t i = sc.abvh_order[first + k];                                                   \
                    WorldHit w;                                                                                    \
                    analytic_hit(sc.prims[i], o, d, w);                                                            \
                    ++n_tests;                                                                                     \
                    if (w.has && (w.d2 < best.d2 || (w.d2 == best.d2 && best.id != HIT_MISS && i < best.prim))) {  \
                        best.d2 = w.d2;                                                                            \
                        best.id = i;                                                                               \
                        best.prim = i;                                                                             \
                        tlimit = limit_from_d2(best.d2, pad);                                                      \
                    }                                                                                              \
                }                                                                                                  \
            }                                                                                                      \
        }                                                                                                          \
    }
        if (sp + 4 > ABVH_STACK) {  // cannot happen for the trees the host builds; stay correct anyway
            best.d2 = 3.402823466e+38f;
            best.id = HIT_MISS;
            best.prim = 0xFFFFFFFFu;
            scan_analytic<false, 1>(sc, o, d, best, n_tests);
            return;
        }
        ABVH_CHILD(x)
        ABVH_CHILD(y)
        ABVH_CHILD(z)
        ABVH_CHILD(w)
#undef ABVH_CHILD
        if (sp == 0) break;
        node = stk[(--sp) * sstride];
    }
}


// What every producer does for the ray it emits: the linear scan over the analytic primitives (its result is the
// initial "best" of the traversal) and the decision whether the BVH has to be walked at all: only if the ray enters
// the (per-ray padded) root box before the analytic hit, by the same conservative test the traversal applies.
template <bool ABVH, int BLOCK>
__device__ __forceinline__ bool classify_ray(const DevScene& sc, f3 o, f3 d, uint32_t& id0, float& d2_0) {
    Closest best;
    best.d2 = 3.402823466e+38f;  // FLT_MAX (primitive.cpp:23)
    best.id = HIT_MISS;
    best.prim = 0xFFFFFFFFu;
    uint32_t n_tests = 0;
    scan_analytic<ABVH, BLOCK>(sc, o, d, best, n_tests);
    id0 = best.id;
    d2_0 = best.d2;
    if (sc.n_nodes == 0u) return false;
    // This box test only decides whether the traversal kernel has to look at the ray at all; it is conservative by the
    // per-ray pad (2^-18 of the coordinates' magnitude) and by the 1.0000153 factor in limit_from_d2.  The producers'
    // directions are unit vectors up to rounding (1e-7), and v_rcp_f32 is within 1 ulp (2^-23): both far inside those
    // margins, so neither the reference's re-normalisation of the direction nor IEEE divisions are spent here (the
    // producers are VALU-bound: SQ_ACTIVE_INST_VALU x waves per SIMD > 1 for k_shade).
    const f3 ld = d;
    const float pad = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + sc.extent);
    const float ix = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
    const float iy = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
    const float iz = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
    const float x0 = __builtin_fmaf(sc.root_min[0], ix, -(o.x + pad) * ix), x1 = __builtin_fmaf(sc.root_max[0], ix, -(o.x - pad) * ix);
    const float y0 = __builtin_fmaf(sc.root_min[1], iy, -(o.y + pad) * iy), y1 = __builtin_fmaf(sc.root_max[1], iy, -(o.y - pad) * iy);
    const float z0 = __builtin_fmaf(sc.root_min[2], iz, -(o.z + pad) * iz), z1 = __builtin_fmaf(sc.root_max[2], iz, -(o.z - pad) * iz);
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(x0, x1), __builtin_fminf(y0, y1)),
                                     __builtin_fmaxf(__builtin_fminf(z0, z1), 0.0f));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(x0, x1), __builtin_fmaxf(y0, y1)),
                                     __builtin_fminf(__builtin_fmaxf(z0, z1), limit_from_d2(d2_0, pad)));
    return tn <= tf * 1.0000005f;
}

// A classified ray that cannot hit a triangle AND whose analytic result ends the path (it misses everything, or it
// hits an emissive primitive, which never scatters: material.h:119-122) needs no slot in the next buffer: the
// value the next k_shade would write for it is already known.  Returns true and that radiance in that case.
__device__ __forceinline__ bool ends_here(const DevScene& sc, bool front, uint32_t id0, f3 thr, f3& L) {
    if (front) return false;
    if (id0 == HIT_MISS) {
        L = thr * mk3(sc.sky[0], sc.sky[1], sc.sky[2]);  // the miss branch of k_shade
        return true;
    }
    const uint32_t m = sc.prims[id0].material;
    if (sc.mat_type[m] == 4u) {
        const float4 e = sc.mat_rgbs[m];
        L = thr * mk3(e.x, e.y, e.z);  // throughput * emitted, then the path stops
        return true;
    }
    return false;
}

// Variant 1 (kept for A/B runs): one loop, each iteration is either a node step or a leaf, per lane.
template <int STACK, bool STATS>
PRT_DEV void traverse_ifif(const DevScene& sc, f3 o, f3 d, Closest& best, uint32_t* stk, uint32_t& n_nodes,
                           uint32_t& n_tris) {
    // Triangles carry the identity Transform: local origin = o, local direction = normalize(d)
    // (TransformNormal, primitive.cpp:30).
    const f3 ld = normalize3(d);
    // Culling only (never changes a result): per-ray conservative padding of every box by `pad`.
    const float pad = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + sc.extent);
    const float ix = 1.0f / (__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
    const float iy = 1.0f / (__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
    const float iz = 1.0f / (__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
    // plane "min" is moved by -pad, plane "max" by +pad:  t_min = min*inv - (o+pad)*inv, t_max = max*inv - (o-pad)*inv
    const float ax = (o.x + pad) * ix, ay = (o.y + pad) * iy, az = (o.z + pad) * iz;
    const float bx = (o.x - pad) * ix, by = (o.y - pad) * iy, bz = (o.z - pad) * iz;
    float tlimit = limit_from_d2(best.d2, pad);
    int sp = 0;
    int node = 0;
    while (true) {
        if (node >= 0) {
            const float4 q0 = sc.nodes[4 * (size_t)node + 0];
            const float4 q1 = sc.nodes[4 * (size_t)node + 1];
            const float4 q2 = sc.nodes[4 * (size_t)node + 2];
            const float4 q3 = sc.nodes[4 * (size_t)node + 3];
            if (STATS) ++n_nodes;
            // left: min (q0.x q0.y q0.z) max (q0.w q1.x q1.y); right: min (q1.z q1.w q2.x) max (q2.y q2.z q2.w)
            const float l0x = __builtin_fmaf(q0.x, ix, -ax), l1x = __builtin_fmaf(q0.w, ix, -bx);
            const float l0y = __builtin_fmaf(q0.y, iy, -ay), l1y = __builtin_fmaf(q1.x, iy, -by);
            const float l0z = __builtin_fmaf(q0.z, iz, -az), l1z = __builtin_fmaf(q1.y, iz, -bz);
            const float r0x = __builtin_fmaf(q1.z, ix, -ax), r1x = __builtin_fmaf(q2.y, ix, -bx);
            const float r0y = __builtin_fmaf(q1.w, iy, -ay), r1y = __builtin_fmaf(q2.z, iy, -by);
            const float r0z = __builtin_fmaf(q2.x, iz, -az), r1z = __builtin_fmaf(q2.w, iz, -bz);
            const float tnL = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(l0x, l1x), __builtin_fminf(l0y, l1y)),
                                              __builtin_fmaxf(__builtin_fminf(l0z, l1z), 0.0f));
            const float tfL = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(l0x, l1x), __builtin_fmaxf(l0y, l1y)),
                                              __builtin_fminf(__builtin_fmaxf(l0z, l1z), tlimit));
            const float tnR = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(r0x, r1x), __builtin_fminf(r0y, r1y)),
                                              __builtin_fmaxf(__builtin_fminf(r0z, r1z), 0.0f));
            const float tfR = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(r0x, r1x), __builtin_fmaxf(r0y, r1y)),
                                              __builtin_fminf(__builtin_fmaxf(r0z, r1z), tlimit));
            const bool hL = tnL <= tfL * 1.0000005f;
            const bool hR = tnR <= tfR * 1.0000005f;
            const int left = __float_as_int(q3.x), right = __float_as_int(q3.y);
            if (hL && hR) {
                const bool lfirst = tnL <= tnR;
                const int nearc = lfirst ? left : right;
                const int farc = lfirst ? right : left;
                if (sp < STACK) stk[sp * 256] = (uint32_t)farc;
                ++sp;  // host guarantees STACK >= tree depth; the guard only prevents LDS corruption
                node = nearc;
                continue;
            }
            if (hL) {
                node = left;
                continue;
            }
            if (hR) {
                node = right;
                continue;
            }
        } else {
            const uint32_t ref = ~(uint32_t)node;
            const uint32_t first = ref >> 4, cnt = ref & 15u;
            for (uint32_t t = 0; t < cnt; ++t) {
                const uint32_t slot = first + t;
                const float4 a = sc.tris[3 * (size_t)slot + 0];
                const float4 b = sc.tris[3 * (size_t)slot + 1];
                const float4 c = sc.tris[3 * (size_t)slot + 2];
                if (STATS) ++n_tris;
                f3 pos;
                float b1, b2;
                if (triangle_hit_pos(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), o, ld, pos, b1, b2)) {
                    const float d2 = dist2(o, pos);
                    const uint32_t prim = __float_as_uint(a.w);
                    if (d2 < best.d2 || (d2 == best.d2 && best.id != HIT_MISS && prim < best.prim)) {
                        best.d2 = d2;
                        best.id = sc.n_prims + slot;
                        best.prim = prim;
                        tlimit = limit_from_d2(d2, pad);
                    }
                }
            }
        }
        if (sp == 0) break;
        --sp;
        node = (sp < STACK) ? (int)stk[sp * 256] : -1;  // -1 == ~0 == empty leaf
    }
}

// Variant 0 (default): speculative while-while traversal (Aila & Laine) on wave64.  Each lane walks internal
// nodes until it holds a leaf; the first leaf found is POSTPONED and the lane keeps walking, so the wave
// leaves the node loop only when no lane is still searching (one ballot per step), and then all lanes test
// their leaves together.  Node steps and triangle tests are therefore executed with far fewer idle lanes
// than the one-loop form, where the two code paths alternate within a wave.
typedef float v2f __attribute__((ext_vector_type(2)));
#define NODE_DONE 0x7FFFFFFF
#define LEAF_NONE 0x7FFFFFFE
#define NEED_POP 0x7FFFFFFD
#define PRT_OVF_CAP (1u << 20)  // entries of the stack-overflow list (work[513..])
template <int STACK, bool STATS>
PRT_DEV void traverse_ww(const DevScene& sc, f3 o, f3 d, Closest& best, uint32_t* stk, uint32_t& n_nodes,
                         uint32_t& n_tris) {
    const f3 ld = normalize3(d);  // TransformNormal(identity, d), primitive.cpp:30
    const float pad = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + sc.extent);
    const float ix = 1.0f / (__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
    const float iy = 1.0f / (__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
    const float iz = 1.0f / (__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
    const float ax = (o.x + pad) * ix, ay = (o.y + pad) * iy, az = (o.z + pad) * iz;
    const float bx = (o.x - pad) * ix, by = (o.y - pad) * iy, bz = (o.z - pad) * iz;
    float tlimit = limit_from_d2(best.d2, pad);
    int sp = 0;
    int node = 0;
    int leaf = LEAF_NONE;
    while (node != NODE_DONE) {
        // ---- phase 1: internal nodes ----
        while ((unsigned)node < 0x40000000u) {
            const float4 q0 = sc.nodes[4 * (size_t)node + 0];
            const float4 q1 = sc.nodes[4 * (size_t)node + 1];
            const float4 q2 = sc.nodes[4 * (size_t)node + 2];
            const float4 q3 = sc.nodes[4 * (size_t)node + 3];
            if (STATS) ++n_nodes;
            const float l0x = __builtin_fmaf(q0.x, ix, -ax), l1x = __builtin_fmaf(q0.w, ix, -bx);
            const float l0y = __builtin_fmaf(q0.y, iy, -ay), l1y = __builtin_fmaf(q1.x, iy, -by);
            const float l0z = __builtin_fmaf(q0.z, iz, -az), l1z = __builtin_fmaf(q1.y, iz, -bz);
            const float r0x = __builtin_fmaf(q1.z, ix, -ax), r1x = __builtin_fmaf(q2.y, ix, -bx);
            const float r0y = __builtin_fmaf(q1.w, iy, -ay), r1y = __builtin_fmaf(q2.z, iy, -by);
            const float r0z = __builtin_fmaf(q2.x, iz, -az), r1z = __builtin_fmaf(q2.w, iz, -bz);
            const float tnL = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(l0x, l1x), __builtin_fminf(l0y, l1y)),
                                              __builtin_fmaxf(__builtin_fminf(l0z, l1z), 0.0f));
            const float tfL = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(l0x, l1x), __builtin_fmaxf(l0y, l1y)),
                                              __builtin_fminf(__builtin_fmaxf(l0z, l1z), tlimit));
            const float tnR = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(r0x, r1x), __builtin_fminf(r0y, r1y)),
                                              __builtin_fmaxf(__builtin_fminf(r0z, r1z), 0.0f));
            const float tfR = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(r0x, r1x), __builtin_fmaxf(r0y, r1y)),
                                              __builtin_fminf(__builtin_fmaxf(r0z, r1z), tlimit));
            const bool hL = tnL <= tfL * 1.0000005f;
            const bool hR = tnR <= tfR * 1.0000005f;
            const int left = __float_as_int(q3.x), right = __float_as_int(q3.y);
            if (hL && hR) {
                const bool lfirst = tnL <= tnR;
                node = lfirst ? left : right;
                const int farc = lfirst ? right : left;
                if (sp < STACK) stk[sp * 256] = (uint32_t)farc;  // host guarantees STACK >= tree depth
                ++sp;
            } else if (hL) {
                node = left;
            } else if (hR) {
                node = right;
            } else if (sp > 0) {
                --sp;
                node = (sp < STACK) ? (int)stk[sp * 256] : -1;
            } else {
                node = NODE_DONE;
            }
            if (node < 0 && leaf == LEAF_NONE) {  // first leaf: postpone it, keep walking
                leaf = node;
                if (sp > 0) {
                    --sp;
                    node = (sp < STACK) ? (int)stk[sp * 256] : -1;
                } else {
                    node = NODE_DONE;
                }
            }
            if (__ballot(leaf == LEAF_NONE && node != NODE_DONE) == 0ull) break;  // nobody is still searching
        }
        // ---- phase 2: leaves ----
        while (leaf != LEAF_NONE) {
            const uint32_t ref = ~(uint32_t)leaf;
            const uint32_t first = ref >> 4, cnt = ref & 15u;
            for (uint32_t t = 0; t < cnt; ++t) {
                const uint32_t slot = first + t;
                const float4 a = sc.tris[3 * (size_t)slot + 0];
                const float4 b = sc.tris[3 * (size_t)slot + 1];
                const float4 c = sc.tris[3 * (size_t)slot + 2];
                if (STATS) ++n_tris;
                f3 pos;
                float b1, b2;
                if (triangle_hit_pos(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), o, ld, pos, b1, b2)) {
                    const float d2 = dist2(o, pos);
                    const uint32_t prim = __float_as_uint(a.w);
                    if (d2 < best.d2 || (d2 == best.d2 && best.id != HIT_MISS && prim < best.prim)) {
                        best.d2 = d2;
                        best.id = sc.n_prims + slot;
                        best.prim = prim;
                        tlimit = limit_from_d2(d2, pad);
                    }
                }
            }
            leaf = LEAF_NONE;
            if (node < 0) {  // the walk stopped on a second leaf: take it now
                leaf = node;
                if (sp > 0) {
                    --sp;
                    node = (sp < STACK) ? (int)stk[sp * 256] : -1;
                } else {
                    node = NODE_DONE;
                }
            }
        }
    }
}

template <int STACK, bool STATS, int VARIANT>
PRT_DEV void traverse(const DevScene& sc, f3 o, f3 d, Closest& best, uint32_t* stk, uint32_t& n_nodes,
                      uint32_t& n_tris) {
    if (VARIANT == 1)
        traverse_ifif<STACK, STATS>(sc, o, d, best, stk, n_nodes, n_tris);
    else
        traverse_ww<STACK, STATS>(sc, o, d, best, stk, n_nodes, n_tris);
}

template <int STACK, bool STATS, int VARIANT>
__global__ void __launch_bounds__(256) k_intersect(DevScene sc, const float4* __restrict__ ro,
                                                   const float4* __restrict__ rd, uint32_t* __restrict__ hit,
                                                   const uint32_t* __restrict__ count_ptr,
                                                   unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_stack[STACK * 256];
    const uint32_t count = *count_ptr;
    const uint32_t nb_live = (count + 255u) >> 8;
    if (blockIdx.x >= nb_live) return;
    const uint32_t k = xcd_remap(blockIdx.x, nb_live) * 256u + threadIdx.x;
    uint32_t n_nodes = 0, n_tris = 0, n_ptests = 0;
    if (k < count) {
        const float4 O = ro[k];
        const float4 D = rd[k];
        if (D.x == 0.0f && D.y == 0.0f && D.z == 0.0f) {
            hit[k] = HIT_DEAD;
        } else {
            const f3 o = mk3(O.x, O.y, O.z), d = mk3(D.x, D.y, D.z);
            Closest best;
            best.d2 = 3.402823466e+38f;  // FLT_MAX (primitive.cpp:23)
            best.id = HIT_MISS;
            best.prim = 0xFFFFFFFFu;
            scan_analytic<false>(sc, o, d, best, n_ptests);
            if (sc.n_nodes) traverse<STACK, STATS, VARIANT>(sc, o, d, best, &s_stack[threadIdx.x], n_nodes, n_tris);
            hit[k] = best.id;
        }
    }
    if (STATS) {
        atomicAdd(&stats[0], (unsigned long long)n_nodes);
        atomicAdd(&stats[1], (unsigned long long)n_tris);
        atomicAdd(&stats[2], (unsigned long long)n_ptests);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Default closest-hit pipeline (variant 0): k_scan_prims (coherent linear scan over the analytic primitives,
// one thread per ray) followed by k_traverse_persistent over the triangles' BVH.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_scan_prims(DevScene sc, const float4* __restrict__ ro,
                                                    const float4* __restrict__ rd, uint32_t* __restrict__ hit,
                                                    float* __restrict__ hd2, const uint32_t* __restrict__ count_ptr,
                                                    uint32_t* __restrict__ work,
                                                    unsigned long long* __restrict__ stats) {
    const uint32_t count = *count_ptr;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < 8u) work[32u * k] = 0u;  // chunk cursors of the traversal kernel that follows on the stream (work[256]: watchdog flag)
    if (k == 8u) work[512] = 0u;     // its overflow-list counter
    if (k >= count) return;
    const float4 O = ro[k];
    const float4 D = rd[k];
    Closest best;
    best.d2 = 3.402823466e+38f;  // FLT_MAX (primitive.cpp:23)
    best.id = HIT_MISS;
    best.prim = 0xFFFFFFFFu;
    uint32_t n_ptests = 0;
    if (D.x == 0.0f && D.y == 0.0f && D.z == 0.0f) {
        best.id = HIT_DEAD;
    } else {
        if (sc.abvh_nodes)
            scan_analytic<true, 256>(sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), best, n_ptests);
        else
            scan_analytic<false>(sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), best, n_ptests);
    }
    hit[k] = best.id;
    hd2[k] = best.d2;
    if (stats) atomicAdd(&stats[2], (unsigned long long)n_ptests);
}

// Persistent-wavefront traversal with ray replacement.  A fixed grid of waves stays resident; every wave
// grabs chunks of the bounce's ray buffer with one global atomic per `chunk` rays (a single counter word only
// sustains ~88 returning atomics/us, so rays are never fetched one wave-load at a time) and hands the rays
// to its lanes.  A lane whose ray is finished writes its hit id and goes idle; when at least tune.refill_min
// lanes of the wave are idle they are re-filled together, so the 64 lanes stay busy although incoherent rays
// need very different numbers of steps.  Traversal is the speculative while-while of traverse_ww; the per-lane
// stack keeps its first STACK_L entries in LDS ([entry][lane]: bank = lane, conflict-free) and spills deeper
// entries to a global buffer ([entry][thread], coalesced).
// XCD id of the executing wave (HW_REG_XCC_ID, bits 3:0).  Used for L2 affinity only, never for correctness.
PRT_DEV uint32_t xcc_id() { return (uint32_t)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | ((4 - 1) << 11)) & 7u; }

// Chunk cursor(s) of the persistent traversal kernels: work[32 * x] (own 128-B line each) counts the chunks
// taken from XCD x's contiguous eighth of the ray buffer.  Neighbouring rays start in neighbouring parts of the
// scene, so keeping an eighth of the buffer on one XCD keeps the deep BVH levels it touches in that XCD's 4 MB L2.
// A wave first drains its own XCD's range, then steals from the others, so the grid still balances.
PRT_DEV uint32_t grab_chunk(uint32_t* work, uint32_t n_chunks, uint32_t my_xcd, bool affinity) {
    if (!affinity) {
        const uint32_t c = atomicAdd(work, 1u);
        return c < n_chunks ? c : 0xFFFFFFFFu;
    }
    for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t x = (my_xcd + i) & 7u;
        const uint32_t lo = (uint32_t)(((unsigned long long)n_chunks * x) >> 3);
        const uint32_t hi = (uint32_t)(((unsigned long long)n_chunks * (x + 1u)) >> 3);
        if (work[32u * x] >= hi - lo) continue;  // already drained (plain read: a stale value only costs one atomic)
        const uint32_t c = atomicAdd(&work[32u * x], 1u);
        if (c < hi - lo) return lo + c;
    }
    return 0xFFFFFFFFu;
}

// MODE 0: all entries in LDS, the host guarantees the tree never needs more than STACK_L.
// MODE 1: LDS + global spill behind entry STACK_L (any depth; slower: the compiler merges the two address spaces
//         into flat accesses).
// MODE 2: all entries in LDS with an overflow check: a push beyond STACK_L sets `overflow` instead of writing; the
//         kernel then hands that ray to the MODE-1 instance through the overflow list (never seen in practice: the
//         host's bound is a worst case over all paths with every child hit).
// Wave64 inclusive scans with DPP row shifts / row broadcasts (no LDS round trips): the Hillis-Steele steps
// 1, 2, 4, 8 inside each 16-lane row, then lane 15 of rows 0/2 into rows 1/3 and lane 31 into rows 2/3.  Lanes that
// receive nothing keep the identity (0).  All 64 lanes must be active.
#define PRT_DPP(X, CTRL, ROWMASK) (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(X), CTRL, ROWMASK, 0xF, false)
PRT_DEV uint32_t wave_scan_add(uint32_t x) {
    x += PRT_DPP(x, 0x111, 0xF);  // row_shr:1
    x += PRT_DPP(x, 0x112, 0xF);  // row_shr:2
    x += PRT_DPP(x, 0x114, 0xF);  // row_shr:4
    x += PRT_DPP(x, 0x118, 0xF);  // row_shr:8
    x += PRT_DPP(x, 0x142, 0xA);  // row_bcast:15 -> rows 1, 3
    x += PRT_DPP(x, 0x143, 0xC);  // row_bcast:31 -> rows 2, 3
    return x;
}
PRT_DEV uint32_t wave_scan_or(uint32_t x) {
    x |= PRT_DPP(x, 0x111, 0xF);
    x |= PRT_DPP(x, 0x112, 0xF);
    x |= PRT_DPP(x, 0x114, 0xF);
    x |= PRT_DPP(x, 0x118, 0xF);
    x |= PRT_DPP(x, 0x142, 0xA);
    x |= PRT_DPP(x, 0x143, 0xC);
    return x;
}
PRT_DEV uint32_t wave_scan_max(uint32_t x) {
    uint32_t t;
    t = PRT_DPP(x, 0x111, 0xF); x = x > t ? x : t;
    t = PRT_DPP(x, 0x112, 0xF); x = x > t ? x : t;
    t = PRT_DPP(x, 0x114, 0xF); x = x > t ? x : t;
    t = PRT_DPP(x, 0x118, 0xF); x = x > t ? x : t;
    t = PRT_DPP(x, 0x142, 0xA); x = x > t ? x : t;
    t = PRT_DPP(x, 0x143, 0xC); x = x > t ? x : t;
    return x;
}

template <int STACK_L, int MODE>
struct LaneStack {
    uint32_t* lds;      // &s_stack[threadIdx.x], stride 256
    uint32_t* spill;    // &spill[global thread], stride n_threads (MODE 1 only)
    uint32_t stride;
    int sp;
    bool overflow;
    PRT_DEV void push(uint32_t v) {
        if (MODE == 1) {
            if (sp < STACK_L)
                lds[sp * 256] = v;
            else
                spill[(size_t)(sp - STACK_L) * stride] = v;
            ++sp;
        } else if (MODE == 2) {
            if (sp < STACK_L) {
                lds[sp * 256] = v;
                ++sp;
            } else {
                overflow = true;
            }
        } else {
            lds[sp * 256] = v;
            ++sp;
        }
    }
    // precondition: sp > 0
    PRT_DEV int pop() {
        --sp;
        if (MODE != 1 || sp < STACK_L) return (int)lds[sp * 256];
        return (int)spill[(size_t)(sp - STACK_L) * stride];
    }
};

template <int STACK_L, int WAVES, int MODE, bool STATS>
__global__ void __launch_bounds__(256, WAVES) k_traverse_persistent(DevScene sc, const float4* __restrict__ ro,
                                                                    const float4* __restrict__ rd,
                                                                    uint32_t* __restrict__ hit,
                                                                    const float* __restrict__ hd2,
                                                                    const uint32_t* __restrict__ count_ptr,
                                                                    uint32_t* __restrict__ work,
                                                                    uint32_t* __restrict__ spill,
                                                                    const uint32_t* __restrict__ index_list,
                                                                    uint32_t* __restrict__ ovf, PrtTravTuning tune,
                                                                    unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_stack[STACK_L * 256];
    __shared__ uint32_t s_iters[4];
    uint32_t count = *count_ptr;
    if (index_list && count > PRT_OVF_CAP) count = PRT_OVF_CAP;
    const uint32_t chunk = tune.chunk;
    const uint32_t n_chunks = (count + chunk - 1u) / chunk;
    const uint32_t my_xcd = xcc_id();
    if (STATS) {
        if (threadIdx.x < 4) s_iters[threadIdx.x] = 0;
        __syncthreads();
    }
    LaneStack<STACK_L, MODE> st;
    st.overflow = false;
    st.lds = &s_stack[threadIdx.x];
    st.stride = gridDim.x * 256u;
    st.spill = spill + (blockIdx.x * 256u + threadIdx.x);
    st.sp = 0;
    const uint32_t lane = lane_id();
    uint32_t k = 0xFFFFFFFFu;
    int node = NODE_DONE, leaf = LEAF_NONE;
    f3 o = mk3(0.f, 0.f, 0.f), ld = mk3(0.f, 0.f, 1.f);
    float ix = 0.f, iy = 0.f, iz = 0.f, ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f, pad = 0.f, tlimit = 0.f;
    Closest best;
    best.d2 = 3.402823466e+38f;
    best.id = HIT_MISS;
    best.prim = 0xFFFFFFFFu;
    uint32_t n_nodes = 0, n_tris = 0;
    uint32_t cur = 0, cur_end = 0;  // wave-uniform: this wave's current chunk [cur, cur_end)
    bool exhausted = false;         // wave-uniform
    // Exit condition every wave reaches: the loop ends when the ray buffer is exhausted and the wave's lanes are
    // idle; the iteration cap is a watchdog (a wave handles ~count/waves rays x ~100 steps, orders of magnitude
    // below it) that turns a would-be hang into an error flag the host reports.
    for (uint32_t guard = 0;; ++guard) {
        if (guard > (1u << 22)) {
            if (lane == 0) atomicOr(work + 256, 1u);
            break;
        }
        const bool idle = (node == NODE_DONE) && (leaf == LEAF_NONE);
        if (idle && k != 0xFFFFFFFFu) {
            if (MODE == 2 && st.overflow) {
                const uint32_t j = atomicAdd(ovf, 1u);  // re-done from scratch by the spill-capable instance
                if (j < PRT_OVF_CAP)
                    ovf[1u + j] = k;
                else
                    atomicOr(work + 256, 2u);  // list full: reported by prt_synchronize like the watchdog
                st.overflow = false;
            } else {
                hit[k] = best.id;
            }
            k = 0xFFFFFFFFu;
        }
        const unsigned long long idle_mask = __ballot(idle);
        const uint32_t n_idle = (uint32_t)__popcll(idle_mask);
        if (!exhausted && n_idle >= tune.refill_min) {
            if (cur == cur_end) {  // grab the next chunk (one global atomic per `chunk` rays)
                uint32_t c = 0xFFFFFFFFu;
                if (lane == 0) c = grab_chunk(work, n_chunks, my_xcd, tune.xcd_affinity != 0u);
                c = (uint32_t)__shfl((int)c, 0, 64);
                if (c == 0xFFFFFFFFu) {
                    exhausted = true;
                } else {
                    cur = c * chunk;
                    cur_end = (cur + chunk < count) ? cur + chunk : count;
                }
            }
            if (!exhausted) {
                const uint32_t qi = cur + (uint32_t)__popcll(idle_mask & ((1ull << lane) - 1ull));
                if (idle && qi < cur_end) {
                    const uint32_t kk = index_list ? index_list[qi] : qi;
                    const uint32_t hid = hit[kk];
                    if (hid != HIT_DEAD) {
                        const float4 O = ro[kk];
                        const float4 D = rd[kk];
                        o = mk3(O.x, O.y, O.z);
                        ld = normalize3(mk3(D.x, D.y, D.z));  // TransformNormal(identity, d), primitive.cpp:30
                        pad = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + sc.extent);
                        ix = 1.0f / (__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
                        iy = 1.0f / (__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
                        iz = 1.0f / (__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
                        ax = (o.x + pad) * ix; ay = (o.y + pad) * iy; az = (o.z + pad) * iz;
                        bx = (o.x - pad) * ix; by = (o.y - pad) * iy; bz = (o.z - pad) * iz;
                        best.id = hid;
                        best.prim = hid;  // analytic index, or 0xFFFFFFFF for a miss
                        best.d2 = hd2[kk];
                        tlimit = limit_from_d2(best.d2, pad);
                        k = kk;
                        node = 0;
                        leaf = LEAF_NONE;
                        st.sp = 0;
                    }
                }
                cur = (cur + n_idle < cur_end) ? cur + n_idle : cur_end;
            }
        }
        if (__ballot(k != 0xFFFFFFFFu) == 0ull) {
            if (exhausted) break;
            continue;
        }
        // ---- phase 1: internal nodes (leave when at most exit_max lanes are still looking for a leaf) ----
        while ((unsigned)node < 0x40000000u) {
            const float4 q0 = sc.nodes[4 * (size_t)node + 0];
            const float4 q1 = sc.nodes[4 * (size_t)node + 1];
            const float4 q2 = sc.nodes[4 * (size_t)node + 2];
            const float4 q3 = sc.nodes[4 * (size_t)node + 3];
            if (STATS) {
                ++n_nodes;
                if ((int)lane == __ffsll((long long)__ballot(true)) - 1) ++s_iters[threadIdx.x >> 6];
            }
            const float l0x = __builtin_fmaf(q0.x, ix, -ax), l1x = __builtin_fmaf(q0.w, ix, -bx);
            const float l0y = __builtin_fmaf(q0.y, iy, -ay), l1y = __builtin_fmaf(q1.x, iy, -by);
            const float l0z = __builtin_fmaf(q0.z, iz, -az), l1z = __builtin_fmaf(q1.y, iz, -bz);
            const float r0x = __builtin_fmaf(q1.z, ix, -ax), r1x = __builtin_fmaf(q2.y, ix, -bx);
            const float r0y = __builtin_fmaf(q1.w, iy, -ay), r1y = __builtin_fmaf(q2.z, iy, -by);
            const float r0z = __builtin_fmaf(q2.x, iz, -az), r1z = __builtin_fmaf(q2.w, iz, -bz);
            const float tnL = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(l0x, l1x), __builtin_fminf(l0y, l1y)),
                                              __builtin_fmaxf(__builtin_fminf(l0z, l1z), 0.0f));
            const float tfL = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(l0x, l1x), __builtin_fmaxf(l0y, l1y)),
                                              __builtin_fminf(__builtin_fmaxf(l0z, l1z), tlimit));
            const float tnR = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(r0x, r1x), __builtin_fminf(r0y, r1y)),
                                              __builtin_fmaxf(__builtin_fminf(r0z, r1z), 0.0f));
            const float tfR = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(r0x, r1x), __builtin_fmaxf(r0y, r1y)),
                                              __builtin_fminf(__builtin_fmaxf(r0z, r1z), tlimit));
            const bool hL = tnL <= tfL * 1.0000005f;
            const bool hR = tnR <= tfR * 1.0000005f;
            const int left = __float_as_int(q3.x), right = __float_as_int(q3.y);
            // select chain instead of a 4-way branch: candidate = nearer hit child, or NEED_POP
            const bool both = hL && hR;
            const bool lfirst = tnL <= tnR;
            const int nearc = lfirst ? left : right;
            const int farc = lfirst ? right : left;
            const int cand = both ? nearc : (hL ? left : (hR ? right : NEED_POP));
            if (both) st.push((uint32_t)farc);
            node = cand;
            if (cand == NEED_POP) node = (st.sp > 0) ? st.pop() : NODE_DONE;
            if (node < 0 && leaf == LEAF_NONE) {  // first leaf (a child or a popped entry): postpone it, keep walking
                leaf = node;
                node = (st.sp > 0) ? st.pop() : NODE_DONE;
            }
            if (MODE == 2 && st.overflow) {  // give the ray up; it is re-traversed by the MODE-1 instance
                node = NODE_DONE;
                leaf = LEAF_NONE;
                st.sp = 0;
            }
            if ((uint32_t)__popcll(__ballot(leaf == LEAF_NONE && node != NODE_DONE)) <= tune.exit_max) break;
        }
        // ---- phase 2: leaves ----
        while (leaf != LEAF_NONE) {
            const uint32_t ref = ~(uint32_t)leaf;
            const uint32_t first = ref >> 4, cnt = ref & 15u;
            for (uint32_t t = 0; t < cnt; ++t) {
                const uint32_t slot = first + t;
                const float4 a = sc.tris[3 * (size_t)slot + 0];
                const float4 b = sc.tris[3 * (size_t)slot + 1];
                const float4 c = sc.tris[3 * (size_t)slot + 2];
                if (STATS) ++n_tris;
                f3 pos;
                float b1, b2;
                if (triangle_hit_pos(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), o, ld, pos, b1, b2)) {
                    const float d2 = dist2(o, pos);
                    const uint32_t prim = __float_as_uint(a.w);
                    if (d2 < best.d2 || (d2 == best.d2 && best.id != HIT_MISS && prim < best.prim)) {
                        best.d2 = d2;
                        best.id = sc.n_prims + slot;
                        best.prim = prim;
                        tlimit = limit_from_d2(d2, pad);
                    }
                }
            }
            leaf = LEAF_NONE;
            if (node < 0) {  // the walk stopped on a second leaf: take it now
                leaf = node;
                node = (st.sp > 0) ? st.pop() : NODE_DONE;
            }
        }
    }
    if (STATS) {
        atomicAdd(&stats[0], (unsigned long long)n_nodes);
        atomicAdd(&stats[1], (unsigned long long)n_tris);
        __syncthreads();
        if (threadIdx.x < 4) atomicAdd(&stats[3], 64ull * s_iters[threadIdx.x]);
    }
}

// The same kernel over the 4-wide tree (default): half as many dependent node fetches per ray, one 128-B cache
// line per visit, children visited in entry-distance order (5-comparator sorting network).
template <int STACK_L, int WAVES, int MODE, bool STATS>
__global__ void __launch_bounds__(256, WAVES) k_traverse4_persistent(DevScene sc, const float4* __restrict__ ro,
                                                                    const float4* __restrict__ rd,
                                                                    uint32_t* __restrict__ hit,
                                                                    const float* __restrict__ hd2,
                                                                    const uint32_t* __restrict__ count_ptr,
                                                                    uint32_t* __restrict__ work,
                                                                    uint32_t* __restrict__ spill,
                                                                    const uint32_t* __restrict__ index_list,
                                                                    uint32_t* __restrict__ ovf, PrtTravTuning tune,
                                                                    unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_stack[(STACK_L + (MODE == 3 ? 3 : 0)) * 256];  // MODE 3 writes up to 3 rows past the top
    __shared__ unsigned long long s_key[256];  // per lane: best (d2 bits << 32 | prim) of the cooperative triangle tests
    __shared__ uint32_t s_slot[256];           // per lane: leaf-order slot of that best
    __shared__ uint32_t s_mark[256];           // per item position of a round: owner lane + 1 where an owner's range starts
    __shared__ uint32_t s_iters[8];  // [0..3] node-loop, [4..7] triangle-loop iterations per wave (STATS)
    uint32_t count = *count_ptr;
    if (index_list && count > PRT_OVF_CAP) count = PRT_OVF_CAP;
    const uint32_t chunk = tune.chunk;
    const uint32_t n_chunks = (count + chunk - 1u) / chunk;
    const uint32_t my_xcd = xcc_id();
    if (STATS) {
        if (threadIdx.x < 8) s_iters[threadIdx.x] = 0;
        __syncthreads();
    }
    LaneStack<STACK_L, MODE> st;
    st.overflow = false;
    st.lds = &s_stack[threadIdx.x];
    st.stride = gridDim.x * 256u;
    st.spill = spill + (blockIdx.x * 256u + threadIdx.x);
    st.sp = 0;
    const uint32_t lane = lane_id();
    uint32_t k = 0xFFFFFFFFu;
    int node = NODE_DONE, leaf = LEAF_NONE;
    f3 o = mk3(0.f, 0.f, 0.f), ld = mk3(0.f, 0.f, 1.f);
    float ix = 0.f, iy = 0.f, iz = 0.f, ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f, pad = 0.f, tlimit = 0.f;
    Closest best;
    best.d2 = 3.402823466e+38f;
    best.id = HIT_MISS;
    best.prim = 0xFFFFFFFFu;
    uint32_t n_nodes = 0, n_tris = 0, max_sp = 0;
    uint32_t cur = 0, cur_end = 0;  // wave-uniform: this wave's current chunk [cur, cur_end)
    bool exhausted = false;         // wave-uniform
    // Exit condition every wave reaches: the loop ends when the ray buffer is exhausted and the wave's lanes are
    // idle; the iteration cap is a watchdog (a wave handles ~count/waves rays x ~100 steps, orders of magnitude
    // below it) that turns a would-be hang into an error flag the host reports.
    for (uint32_t guard = 0;; ++guard) {
        if (guard > (1u << 22)) {
            if (lane == 0) atomicOr(work + 256, 1u);
            break;
        }
        const bool idle = (node == NODE_DONE) && (leaf == LEAF_NONE);
        if (idle && k != 0xFFFFFFFFu) {
            if ((MODE == 2 || MODE == 3) && st.overflow) {
                const uint32_t j = atomicAdd(ovf, 1u);  // re-done from scratch by the spill-capable instance
                if (j < PRT_OVF_CAP)
                    ovf[1u + j] = k;
                else
                    atomicOr(work + 256, 2u);  // list full: reported by prt_synchronize like the watchdog
                st.overflow = false;
            } else {
                hit[k] = best.id;
            }
            k = 0xFFFFFFFFu;
        }
        const unsigned long long idle_mask = __ballot(idle);
        const uint32_t n_idle = (uint32_t)__popcll(idle_mask);
        if (!exhausted && n_idle >= tune.refill_min) {
            if (cur == cur_end) {  // grab the next chunk (one global atomic per `chunk` rays)
                uint32_t c = 0xFFFFFFFFu;
                if (lane == 0) c = grab_chunk(work, n_chunks, my_xcd, tune.xcd_affinity != 0u);
                c = (uint32_t)__shfl((int)c, 0, 64);
                if (c == 0xFFFFFFFFu) {
                    exhausted = true;
                } else {
                    cur = c * chunk;
                    cur_end = (cur + chunk < count) ? cur + chunk : count;
                }
            }
            if (!exhausted) {
                const uint32_t qi = cur + (uint32_t)__popcll(idle_mask & ((1ull << lane) - 1ull));
                if (idle && qi < cur_end) {
                    const uint32_t kk = index_list ? index_list[qi] : qi;
                    const uint32_t hid = hit[kk];
                    if (hid != HIT_DEAD) {
                        const float4 O = ro[kk];
                        const float4 D = rd[kk];
                        o = mk3(O.x, O.y, O.z);
                        ld = normalize3(mk3(D.x, D.y, D.z));  // TransformNormal(identity, d), primitive.cpp:30
                        pad = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + sc.extent);
                        ix = 1.0f / (__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
                        iy = 1.0f / (__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
                        iz = 1.0f / (__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
                        ax = (o.x + pad) * ix; ay = (o.y + pad) * iy; az = (o.z + pad) * iz;
                        bx = (o.x - pad) * ix; by = (o.y - pad) * iy; bz = (o.z - pad) * iz;
                        best.id = hid;
                        best.prim = hid;  // analytic index, or 0xFFFFFFFF for a miss
                        best.d2 = hd2[kk];
                        tlimit = limit_from_d2(best.d2, pad);
                        k = kk;
                        node = 0;
                        leaf = LEAF_NONE;
                        st.sp = 0;
                    }
                }
                cur = (cur + n_idle < cur_end) ? cur + n_idle : cur_end;
            }
        }
        if (__ballot(k != 0xFFFFFFFFu) == 0ull) {
            if (exhausted) break;
            continue;
        }
        // ---- phase 1: internal nodes (leave when at most exit_max lanes are still looking for a leaf) ----
        while ((unsigned)node < 0x40000000u) {
            const int sp0 = st.sp;
            int t1 = 0, t2 = 0;
            if (MODE == 3) {  // the two entries under the top, read before anything is written this step
                t1 = (int)st.lds[(sp0 > 0 ? sp0 - 1 : 0) * 256];
                t2 = (int)st.lds[(sp0 > 1 ? sp0 - 2 : 0) * 256];
            }
            const float4* nb = sc.nodes4 + 8 * (size_t)node;
            const float4 mnx = nb[0], mxx = nb[1], mny = nb[2], mxy = nb[3], mnz = nb[4], mxz = nb[5], rf = nb[6];
            if (STATS) {
                ++n_nodes;
                if ((int)lane == __ffsll((long long)__ballot(true)) - 1) ++s_iters[threadIdx.x >> 6];
            }
            const float kInf = __builtin_inff();
            float k0, k1, k2, k3;
            // children are tested two at a time with packed FMAs (v_pk_fma_f32: two independent fp32 FMAs, the same
            // rounding as the scalar form); min/max have no packed fp32 form
#define PRT_PAIR(LO, HI, KA, KB)                                                                                    \
    {                                                                                                               \
        const v2f x0 = __builtin_elementwise_fma((v2f){mnx.LO, mnx.HI}, (v2f){ix, ix}, (v2f){-ax, -ax});            \
        const v2f x1 = __builtin_elementwise_fma((v2f){mxx.LO, mxx.HI}, (v2f){ix, ix}, (v2f){-bx, -bx});            \
        const v2f y0 = __builtin_elementwise_fma((v2f){mny.LO, mny.HI}, (v2f){iy, iy}, (v2f){-ay, -ay});            \
        const v2f y1 = __builtin_elementwise_fma((v2f){mxy.LO, mxy.HI}, (v2f){iy, iy}, (v2f){-by, -by});            \
        const v2f z0 = __builtin_elementwise_fma((v2f){mnz.LO, mnz.HI}, (v2f){iz, iz}, (v2f){-az, -az});            \
        const v2f z1 = __builtin_elementwise_fma((v2f){mxz.LO, mxz.HI}, (v2f){iz, iz}, (v2f){-bz, -bz});            \
        const float tna = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(x0.x, x1.x), __builtin_fminf(y0.x, y1.x)), \
                                          __builtin_fmaxf(__builtin_fminf(z0.x, z1.x), 0.0f));                       \
        const float tfa = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(x0.x, x1.x), __builtin_fmaxf(y0.x, y1.x)), \
                                          __builtin_fminf(__builtin_fmaxf(z0.x, z1.x), tlimit));                     \
        const float tnb = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(x0.y, x1.y), __builtin_fminf(y0.y, y1.y)), \
                                          __builtin_fmaxf(__builtin_fminf(z0.y, z1.y), 0.0f));                       \
        const float tfb = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(x0.y, x1.y), __builtin_fmaxf(y0.y, y1.y)), \
                                          __builtin_fminf(__builtin_fmaxf(z0.y, z1.y), tlimit));                     \
        const v2f tfs = (v2f){tfa, tfb} * (v2f){1.0000005f, 1.0000005f};                                             \
        KA = (tna <= tfs.x) ? tna : kInf;                                                                           \
        KB = (tnb <= tfs.y) ? tnb : kInf;                                                                           \
    }
            PRT_PAIR(x, y, k0, k1)
            PRT_PAIR(z, w, k2, k3)
#undef PRT_PAIR
            int r0 = __float_as_int(rf.x), r1 = __float_as_int(rf.y), r2 = __float_as_int(rf.z), r3 = __float_as_int(rf.w);
            // sort the four (entry distance, ref) pairs ascending: 5-comparator network; misses (+inf) end up last
#define PRT_CSWAP(KA, RA, KB, RB)            \
    {                                        \
        const bool sw = KB < KA;             \
        const float kt = sw ? KB : KA;       \
        KB = sw ? KA : KB;                   \
        KA = kt;                             \
        const int rt = sw ? RB : RA;         \
        RB = sw ? RA : RB;                   \
        RA = rt;                             \
    }
            PRT_CSWAP(k0, r0, k1, r1)
            PRT_CSWAP(k2, r2, k3, r3)
            PRT_CSWAP(k0, r0, k2, r2)
            PRT_CSWAP(k1, r1, k3, r3)
            PRT_CSWAP(k1, r1, k2, r2)
#undef PRT_CSWAP
            if (MODE == 3) {
                // Branch-free step.  The three far children are stored unconditionally above the top (farthest
                // first) and the stack pointer advances only past the ones that were hit; the two entries below
                // the old top were read into t1/t2 at the head of the step, so "next node" and "postpone a leaf"
                // are pure selects.  A step that would leave more than STACK_L entries gives the ray up (it is
                // re-traversed by the spill-capable instance through the overflow list).
                const int h0 = k0 < kInf, h1 = k1 < kInf, h2 = k2 < kInf, h3 = k3 < kInf;
                st.lds[sp0 * 256] = (uint32_t)r3;
                const int s1 = sp0 + h3;
                st.lds[s1 * 256] = (uint32_t)r2;
                const int s2 = s1 + h2;
                st.lds[s2 * 256] = (uint32_t)r1;
                const int sp1 = s2 + h1;
                const int below0 = sp0 > 0 ? t1 : NODE_DONE;  // top of the stack before this step
                const int below1 = sp0 > 1 ? t2 : NODE_DONE;  // the entry under it
                const int nxt = h0 ? r0 : below0;
                const int spn = h0 ? sp1 : (sp0 > 0 ? sp0 - 1 : 0);
                const bool take = (nxt < 0) && (leaf == LEAF_NONE);  // first leaf: postpone it, keep walking
                const int under = h0 ? (h1 ? r1 : below0) : below1;
                const int spu = h0 ? (h1 ? sp1 - 1 : (sp0 > 0 ? sp0 - 1 : 0)) : (sp0 > 1 ? sp0 - 2 : 0);
                leaf = take ? nxt : leaf;
                node = take ? under : nxt;
                st.sp = take ? spu : spn;
                if (sp1 > STACK_L) st.overflow = true;
            } else {
            // farthest first, so that the nearest pending child is popped first
            if (k3 < kInf) st.push((uint32_t)r3);
            if (k2 < kInf) st.push((uint32_t)r2);
            if (k1 < kInf) st.push((uint32_t)r1);
            node = (k0 < kInf) ? r0 : NEED_POP;
            if (node == NEED_POP) node = (st.sp > 0) ? st.pop() : NODE_DONE;
            if (node < 0 && leaf == LEAF_NONE) {  // first leaf (a child or a popped entry): postpone it, keep walking
                leaf = node;
                node = (st.sp > 0) ? st.pop() : NODE_DONE;
            }
            }
            if ((MODE == 2 || MODE == 3) && st.overflow) {  // give the ray up; it is re-traversed by the MODE-1 instance
                node = NODE_DONE;
                leaf = LEAF_NONE;
                st.sp = 0;
            }
            if (STATS && (uint32_t)st.sp > max_sp) max_sp = (uint32_t)st.sp;
            if ((uint32_t)__popcll(__ballot(leaf == LEAF_NONE && node != NODE_DONE)) <= tune.exit_max) break;
        }
        // ---- phase 2: leaves, tested COOPERATIVELY by the wave ----
        // A lane holds 0..2 pending leaves (the postponed one and, if the walk stopped on a second leaf, that one)
        // = 0..8 triangles.  Testing them lane by lane leaves 86 % of the lanes idle (measured), so the wave pools
        // all pending (ray, triangle) pairs and every lane tests ONE pair per round: the pair's owner lane is found
        // by a 6-step search over the running offsets, the owner's ray comes over ds_bpermute, and the results are
        // merged per owner with a 64-bit LDS atomicMin on (d2 bits << 32 | primitive index) -- exactly the
        // reference's rule "smaller d2 wins, ties to the lower primitive index" (primitive.cpp:42-48), since d2 >= 0
        // makes the float order equal to the integer order of its bits.
        {
            const bool second = node < 0;  // NODE_DONE / internal ids are >= 0
            uint32_t f1 = 0, c1 = 0, f2 = 0, c2 = 0;
            if (leaf != LEAF_NONE) {
                const uint32_t ref = ~(uint32_t)leaf;
                f1 = ref >> 4;
                c1 = ref & 15u;
            }
            if (second) {
                const uint32_t ref = ~(uint32_t)node;
                f2 = ref >> 4;
                c2 = ref & 15u;
            }
            const uint32_t total = c1 + c2;
            if (__ballot(total != 0u) != 0ull) {  // wave-uniform
                const uint32_t incl = wave_scan_add(total);
                const uint32_t off = incl - total;
                const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                // a miss is encoded with prim 0 so that a candidate with d2 == FLT_MAX can never win (primitive.cpp:44)
                const unsigned long long key_best =
                    ((unsigned long long)__float_as_uint(best.d2) << 32) | (best.id == HIT_MISS ? 0u : best.prim);
                const uint32_t my = threadIdx.x;             // this lane's LDS cell
                const uint32_t wbase = threadIdx.x & ~63u;  // first cell of this wave
                s_key[my] = key_best;
                uint32_t carry = 0;  // wave-uniform
                for (uint32_t base = 0; base < T; base += 64u) {  // wave-uniform trip count
                    const uint32_t kq = base + lane;
                    // owner of item kq: every owner whose range starts inside this round marks its first position,
                    // a max-scan spreads the marks to the right; positions before the first mark continue the last
                    // owner of the previous round
                    s_mark[my] = 0u;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    if (total != 0u && off >= base && off < base + 64u) s_mark[wbase + (off - base)] = lane + 1u;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    const uint32_t mk = wave_scan_max(((volatile uint32_t*)s_mark)[my]);
                    const uint32_t owner = mk ? mk - 1u : carry;
                    carry = (uint32_t)__builtin_amdgcn_readlane((int)owner, 63);
                    const uint32_t ooff = (uint32_t)__shfl((int)off, (int)owner, 64);
                    const uint32_t oc1 = (uint32_t)__shfl((int)c1, (int)owner, 64);
                    const uint32_t of1 = (uint32_t)__shfl((int)f1, (int)owner, 64);
                    const uint32_t of2 = (uint32_t)__shfl((int)f2, (int)owner, 64);
                    const f3 qo = mk3(__shfl(o.x, (int)owner, 64), __shfl(o.y, (int)owner, 64), __shfl(o.z, (int)owner, 64));
                    const f3 qd = mk3(__shfl(ld.x, (int)owner, 64), __shfl(ld.y, (int)owner, 64), __shfl(ld.z, (int)owner, 64));
                    bool cand = false;
                    unsigned long long key = 0ull;
                    uint32_t slot = 0;
                    if (kq < T) {
                        const uint32_t j = kq - ooff;
                        slot = j < oc1 ? of1 + j : of2 + (j - oc1);
                        const float4 a = sc.tris[3 * (size_t)slot + 0];
                        const float4 b = sc.tris[3 * (size_t)slot + 1];
                        const float4 c = sc.tris[3 * (size_t)slot + 2];
                        if (STATS) ++n_tris;
                        f3 pos;
                        float b1, b2;
                        if (triangle_hit_pos(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), qo, qd, pos, b1, b2)) {
                            const float d2 = dist2(qo, pos);
                            key = ((unsigned long long)__float_as_uint(d2) << 32) | __float_as_uint(a.w);
                            // NaN / inf d2 have bit patterns above FLT_MAX's: they can never win, as in the reference
                            cand = true;
                            atomicMin(&s_key[wbase + owner], key);
                        }
                    }
                    if (STATS && lane == 0) ++s_iters[4 + (threadIdx.x >> 6)];
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    if (cand && ((volatile unsigned long long*)s_key)[wbase + owner] == key) s_slot[wbase + owner] = slot;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                }
                const unsigned long long won = ((volatile unsigned long long*)s_key)[my];
                if (won != key_best) {
                    best.d2 = __uint_as_float((uint32_t)(won >> 32));
                    best.prim = (uint32_t)won;
                    best.id = sc.n_prims + ((volatile uint32_t*)s_slot)[my];
                    tlimit = limit_from_d2(best.d2, pad);
                }
                leaf = LEAF_NONE;
                if (second) node = (st.sp > 0) ? st.pop() : NODE_DONE;
                if (node < 0) {  // a popped leaf: postpone it (and a second one stays in `node`)
                    leaf = node;
                    node = (st.sp > 0) ? st.pop() : NODE_DONE;
                }
            }
        }
    }
    if (STATS) {
        atomicAdd(&stats[0], (unsigned long long)n_nodes);
        atomicAdd(&stats[1], (unsigned long long)n_tris);
        __syncthreads();
        if (threadIdx.x < 4) atomicAdd(&stats[3], 64ull * s_iters[threadIdx.x]);
        if (threadIdx.x < 4) atomicAdd(&stats[4], 64ull * s_iters[4 + threadIdx.x]);
        atomicMax(&stats[5], (unsigned long long)max_sp);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Default traversal: persistent waves over the COMPRESSED 8-WIDE tree (BVH8Q, layout in bvh.h).
//
// Why: the 4-wide kernel above is bound by dependent node fetches that miss the 4 MB per-XCD L2 (C3: 37 MB of
// 128-B nodes, L2 hit 46 %, 3.4 TB/s leaving the L2s, waves parked on s_waitcnt 64 % of their cycles).  An 8-wide
// node with 8-bit quantized child boxes is 80 B for 8 children: the whole C3 node array is ~5 MB, a ray needs
// ~0.6x as many dependent fetches, and a step needs no sorting network: the children sit in octant-ordered slots, a
// step produces a hit MASK, and the stack holds one (child base, pending hit mask) "node group" per level
// (after Ylitie, Karras, Laine: "Efficient Incoherent Ray Traversal on GPUs Through Compressed Wide BVHs", 2017;
// this formulation is for wave64 with the stack in LDS and cooperative triangle tests).
//
// Per lane: G = (child_base, pending internal hits in bits 24..31 by visiting priority | imask in bits 0..7) and
// up to two pending TRIANGLE groups (tri_base, 24-bit mask): the first one found is postponed while the lane keeps
// walking, a second one stops the lane until the wave's next triangle phase.  There all pending (ray, triangle)
// pairs of the wave are written to an LDS work queue and tested one pair per lane per round; results are merged per
// owner with a 64-bit LDS atomicMin on (d2 bits << 32 | primitive index) = the reference's rule (primitive.cpp:42-48).
// Culling stays conservative: the quantized boxes contain the exact ones (bvh.cpp verifies it in exact arithmetic),
// near planes move out by -pad and far planes by +pad exactly as in the 4-wide kernel, so results are bit-identical.
// A ray that would need more than STACK_L stacked groups goes to the overflow list (re-traversed by the 4-wide
// spill-capable instance); the host sizes STACK_L from the tree's depth, so that never happens in practice.
// ---------------------------------------------------------------------------------------------------------
#define T8_QCAP 256u    // (ray, triangle) pairs one pass of a triangle phase tests (4 B each)
#define T8_QGROUPS 128u // triangle groups a wave can queue between two phases (8 B each, the same memory)

// INST = true (scenes with placed mesh copies, PrtInstance): nodes8 starts with a TOP-LEVEL tree whose "triangles" are
// instances.  A lane that finds instance hits there saves its top-level group, pushes a sentinel and restarts in the
// instance's tree with the reference's per-primitive local ray (local origin = Inv * o, local direction =
// normalize(transpose(mat3(Mat)) * d), primitive.cpp:29-30); popping the sentinel restores the world ray.  All
// triangles live in instance space (world-space meshes form one identity instance, which reproduces the
// non-instanced results bit for bit); a candidate's key is its WORLD distance^2 |o - Mat * pos|^2 and its global
// primitive index, as in the reference.  A lane changes level only when none of its items is left in the queue.
// ---- the box tests of one 80-B node (w0..w4) against the lane's ray: expands to `eim` and `hitmask` --------------------
// Quantized planes, children 0..3 (a) and 4..7 (b): w2 = {lox a, lox b, loy a, loy b}, w3 = {loz a, loz b, hix a, hix b},
// w4 = {hiy a, hiy b, hiz a, hiz b}.  The near plane is the hi plane on an axis the ray travels along negatively; selected
// with v_bfi_b32 under per-axis sign masks, not v_cndmask_b32 (the compiler puts some of the twelve selects on vcc; with
// the bit selects the 5-wave instance needs no scratch).  The per-ray pad (2^-18 (|o|_1 + extent) in position space)
// exceeds the rounding of the plane distances (a few 2^-24 of the same magnitude) by a factor > 10, so no relative slack
// is needed on top of it.  Scalar FMAs: v_pk_fma_f32 measured 3.5 % slower here (12.95 -> 12.68 Grays/s on C3).
#ifndef PRT_T8_BFI
#define PRT_T8_BFI 1  // 0: v_cndmask_b32 selects (A/B builds: make EXTRA=-DPRT_T8_BFI=0)
#endif
#if PRT_T8_BFI
#define T8_SEL(M, A, B) (((A) & (M)) | ((B) & ~(M)))
#else
#define T8_SEL(M, A, B) ((M) ? (A) : (B))
#endif
#define T8_CHILD(J, NX, FX, NY, FY, NZ, FZ)                                                                          \
    {                                                                                                                \
        const float tnx = __builtin_fmaf((float)(((NX) >> (8 * J)) & 0xFFu), Ax, Bnx);                               \
        const float tny = __builtin_fmaf((float)(((NY) >> (8 * J)) & 0xFFu), Ay, Bny);                               \
        const float tnz = __builtin_fmaf((float)(((NZ) >> (8 * J)) & 0xFFu), Az, Bnz);                               \
        const float tfx = __builtin_fmaf((float)(((FX) >> (8 * J)) & 0xFFu), Ax, Bfx);                               \
        const float tfy = __builtin_fmaf((float)(((FY) >> (8 * J)) & 0xFFu), Ay, Bfy);                               \
        const float tfz = __builtin_fmaf((float)(((FZ) >> (8 * J)) & 0xFFu), Az, Bfz);                               \
        const float tn = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), __builtin_fmaxf(tnz, 0.0f));                     \
        const float tf = __builtin_fminf(__builtin_fminf(tfx, tfy), __builtin_fminf(tfz, tlimit));                   \
        const uint32_t cb = ((bits4 >> (8 * J)) & 0xFFu) << ((idx4 >> (8 * J)) & 0xFFu);                             \
        hitmask |= (tn <= tf) ? cb : 0u;                                                                             \
    }
#define T8_HALF(META4, NX, FX, NY, FY, NZ, FZ)                                                                       \
    {                                                                                                                \
        const uint32_t meta4 = (META4);                                                                              \
        const uint32_t in4 = ((meta4 & (meta4 << 1)) & 0x10101010u) >> 4; /* 1 in the bytes of internal children */  \
        const uint32_t idx4 = (meta4 ^ (octinv4 & ((in4 << 3) - in4))) & 0x1F1F1F1Fu;                                \
        const uint32_t bits4 = (meta4 >> 5) & 0x07070707u;                                                           \
        T8_CHILD(0, NX, FX, NY, FY, NZ, FZ)                                                                          \
        T8_CHILD(1, NX, FX, NY, FY, NZ, FZ)                                                                          \
        T8_CHILD(2, NX, FX, NY, FY, NZ, FZ)                                                                          \
        T8_CHILD(3, NX, FX, NY, FY, NZ, FZ)                                                                          \
    }
#define T8_BOXTEST()                                                                                                 \
    const uint32_t eim = w0.w;                                                                                       \
    const float Ax = __uint_as_float((eim & 0xFFu) << 23) * ix;                                                      \
    const float Ay = __uint_as_float(((eim >> 8) & 0xFFu) << 23) * iy;                                               \
    const float Az = __uint_as_float(((eim >> 16) & 0xFFu) << 23) * iz;                                              \
    const float px = __uint_as_float(w0.x), py = __uint_as_float(w0.y), pz = __uint_as_float(w0.z);                  \
    const float Bnx = __builtin_fmaf(px, ix, -anx), Bny = __builtin_fmaf(py, iy, -any), Bnz = __builtin_fmaf(pz, iz, -anz); \
    const float Bfx = __builtin_fmaf(px, ix, -afx), Bfy = __builtin_fmaf(py, iy, -afy), Bfz = __builtin_fmaf(pz, iz, -afz); \
    uint32_t mx = (uint32_t)((int32_t)__float_as_uint(ix) >> 31), my = (uint32_t)((int32_t)__float_as_uint(iy) >> 31), \
             mz = (uint32_t)((int32_t)__float_as_uint(iz) >> 31);                                                    \
    asm("" : "+v"(mx), "+v"(my), "+v"(mz)); /* opaque: keeps the and/or form from being folded back into selects */  \
    const uint32_t nxa = T8_SEL(mx, w3.z, w2.x), nxb = T8_SEL(mx, w3.w, w2.y), fxa = T8_SEL(mx, w2.x, w3.z), fxb = T8_SEL(mx, w2.y, w3.w); \
    const uint32_t nya = T8_SEL(my, w4.x, w2.z), nyb = T8_SEL(my, w4.y, w2.w), fya = T8_SEL(my, w2.z, w4.x), fyb = T8_SEL(my, w2.w, w4.y); \
    const uint32_t nza = T8_SEL(mz, w4.z, w3.x), nzb = T8_SEL(mz, w4.w, w3.y), fza = T8_SEL(mz, w3.x, w4.z), fzb = T8_SEL(mz, w3.y, w4.w); \
    uint32_t hitmask = 0u;                                                                                           \
    T8_HALF(w1.z, nxa, fxa, nya, fya, nza, fza)                                                                      \
    T8_HALF(w1.w, nxb, fxb, nyb, fyb, nzb, fzb)

#define T8_SENTINEL 0xFFFFFFFFu
// The body of the 8-wide walk, shared by the closest-hit kernel (k_traverse8_persistent, ANY = false) and the occlusion
// kernel (k_occluded8_persistent, ANY = true).  ANY: any-hit walk.  Every ray arrives seeded with the bound "miss at
// d2 = tmax^2" (k_pack_occlusion_rays + k_scan_prims_bounded); a ray whose seeded hit is already a blocker is not walked,
// and a lane whose ray has a triangle accepted below its bound in a triangle phase is done: its stack and pending group
// are dropped (the phase has tested all queued items, the queue is empty after it) and its helpers end with it.
// SEEDED (ANY only; the last walk of a batch on the last-segment route, setting 2): the seed may be an ANALYTIC id at its
// distance, exactly as the closest-hit walk is seeded, and every ray of the buffer is walked.  The question is whether a
// triangle key lies strictly below the seed key (d2 bits << 32 | id0: the predicate of the closest-hit walk, ties included);
// hit[] gets the first such triangle found, or keeps the seed.  A blocker is then a slot that names a TRIANGLE.
template <int STACK_L, int WAVES, bool STATS, bool INST, bool LEAN, bool PRIM, bool PATH, bool ANY, bool SEEDED = false>
__device__ __forceinline__ void traverse8_body(DevScene sc, const float4* __restrict__ ro, const float4* __restrict__ rd,
                                               uint32_t* __restrict__ hit, const float* __restrict__ hd2,
                                               const uint32_t* __restrict__ count_ptr, uint32_t* __restrict__ work,
                                               uint32_t* __restrict__ ovf, PrtTravTuning tune,
                                               unsigned long long* __restrict__ stats, PrtPrimary pr, PrtPathArgs pa) {
    // PRIM: the rays are compact primary rays (PrtPrimary): origin and direction are rebuilt from the path id
    // PATH (PrtPathArgs, prt_kernels.h): the work items are whole PATHS, not rays.  A lane whose walk is over is not
    // released: it waits (need_shade) until refill_min lanes of the wave wait or are idle, then those lanes run the shade
    // step together (advance_path: the body of k_shade, same draws in the same order) and walk the scattered ray next; a
    // segment that cannot hit a triangle is shaded on the spot, as the producers' classification decides it; idle lanes
    // take new paths from the launch's cursor and generate their primary ray (k_raygen's arithmetic).  One launch per
    // batch instead of 2 x max_depth + 1: a small batch's launches are dominated by their ramp and their longest rays
    // (C3, one sample: 5 traversal launches of ~150 us for ~30 us of work each), which this pays once.
    __shared__ uint2 s_stack[(STACK_L + 1) * 256];  // [entry][thread]; one row of slack above the top
    __shared__ unsigned long long s_key[256];       // per lane: best (d2 bits << 32 | prim) of the cooperative triangle tests
    __shared__ uint32_t s_slot[256];                // per lane: leaf-order slot of that best
    // per wave, between two triangle phases: up to T8_QGROUPS 8-byte GROUP items {first triangle slot, owner lane << 24 |
    // 24-bit triangle mask} appended by the node loop; the triangle phase takes them into registers and expands them IN
    // PLACE into up to T8_QCAP 4-byte PAIR items (owner lane << 26) | triangle slot, one per lane per round
    __shared__ uint32_t s_queue[4 * T8_QCAP];
    __shared__ uint32_t s_qn[8];                    // per wave: [w] group items appended since the last triangle phase
    __shared__ uint32_t s_iters[8];                 // [0..3] node-loop, [4..7] triangle-loop iterations per wave (STATS)
    __shared__ float s_wray[INST ? 6 * 256 : 1];    // INST: the lane's WORLD ray (origin, raw direction), [component][thread]
    // LEAN (5 waves per SIMD: <= 96 VGPRs): what only the triangle phase needs lives in LDS instead of registers: the
    // lane's ray (origin, unit direction) here, its best key in s_key and its best hit id in s_slot for its whole life
    __shared__ float s_lray[LEAN ? 6 * 256 : 1];
    // STEAL (LEAN instance, only while a wave drains, i.e. after the ray buffer is exhausted).  A launch ends with its
    // longest rays: C3's take ~130 node steps against a mean of 10, and a launch of 1 k rays lasts as long as one of
    // 260 k (tools/launch_floor.py: 170 vs 320 us), ~250 us per bounce during which the chip is almost idle.  Idle
    // lanes of a draining wave therefore take over pending subtrees of the wave's remaining rays: a thief copies the
    // ray's constants out of the donor's registers, takes the donor's BOTTOM stack entry (the oldest, usually largest
    // pending node group) and walks it as a helper of the ray's ROOT lane: its triangle tests resolve into the root's
    // key / slot (the queue item names the root as owner), so helper and root share one culling bound and no merge is
    // needed; the root writes its hit once its own walk is over and no helper of it is left.  The closest hit does
    // not depend on the order of the tests, so results stay bit-identical.
    // (No LDS for the bookkeeping: one more KB would cost the fifth block per CU.  Which roots still have helpers is a
    // wave-uniform 64-bit mask rebuilt from the helpers' k every outer iteration of a draining wave.)
    constexpr bool STEAL = LEAN && !INST;
    static_assert(!PATH || (!LEAN && !INST && !PRIM && !STATS), "the path instance is the plain one-level kernel");
    static_assert(!ANY || (!PATH && !PRIM && !STATS), "the any-hit walk reads plain ray buffers");
    static_assert(!SEEDED || ANY, "a seeded walk is an any-hit walk");
    const uint32_t count = PATH ? pa.n_paths : *count_ptr;
    // PATH: the path a busy lane carries (k = its path id): direction as stored (the walk normalises it again, as the
    // reference's TransformNormal does), throughput, RNG state, segment index; need_shade: the walk of the current
    // segment is over, best.id is its closest hit
    f3 pd = mk3(0.f, 0.f, 1.f), pthr = mk3(0.f, 0.f, 0.f);
    uint32_t prng = 0u, pdepth = 0u;
    bool need_shade = false;
    // (tune.stack_cap: test hook that makes the stack look shorter, to exercise the overflow path)
    const int stack_cap = (tune.stack_cap != 0u && tune.stack_cap < (uint32_t)STACK_L) ? (int)tune.stack_cap : STACK_L;
    // Guided hand-out of the ray buffer, in granules of 64 rays.  The bulk goes out in chunks of tune.chunk rays (one
    // global atomic per chunk; coherent neighbours stay together), but the last tune.tail granules per resident wave go out
    // one at a time: otherwise a wave that grabs a full chunk just before the buffer runs dry works four more rounds
    // (~160 us on C3) while the rest of the chip idles, a fixed cost per launch that hurts most when the frame is split
    // over 8 GPUs.  Small launches consist of single granules only.  A wave's FIRST grab needs no atomic (grab number =
    // its index in the grid; 5120 simultaneous atomics on one word take ~60 us); the cursor counts the grabs after it.
    const uint32_t gran_per_chunk = tune.chunk >> 6;
    const uint32_t n_wv = gridDim.x * 4u;
    const uint32_t n_gran = (count + 63u) >> 6;
    // A launch with fewer than 8 granules per resident wave has no bulk at all: a quarter of its waves would start with a
    // four-granule chunk and still be on it when the rest of the buffer is gone (one-sample calls at 1080p, 2 M + 1.2 M
    // rays for 5,120 waves: traversal 764 -> 642 us per call; from ~12 granules per wave on chunks win again, and
    // single granules throughout cost 20-30 % at 4-64 samples per call: one atomic per 64 rays; TUNING.md.  Thinner
    // granules for launches smaller than the grid, 8-32 rays in every wave instead of 64 in a few, change nothing: such a
    // launch lasts as long as its longest ray, whatever shares the wave with it)
    const uint32_t tail_want = (n_gran < n_wv * 8u || n_gran < n_wv * tune.static_small) ? n_gran : n_wv * tune.tail;
    const uint32_t n_bulk = (n_gran - (tail_want < n_gran ? tail_want : n_gran)) / gran_per_chunk;  // chunks
    // Big launches (>= tune.big_min = 96 granules per resident wave; e.g. the first two bounces of a 256-sample batch at 1080p,
    // 190 M and 318 M rays) hand out the FRONT of the bulk in chunks of tune.big chunks each: at 256 rays per grab the 318 M-ray launch
    // asks the cursor 1.24 M times in 13.7 ms = 90 grabs per us, which is all a counter word executes (~87 / us,
    // tools/atomic_rate.hip); any launch that runs at > 20 G rays/s is there.  The last 32 granules per wave stay ordinary chunks,
    // so the end of the launch is balanced as before.  C3 +1.7 % at 256 samples per batch, +1.2 % at 64, +1 % at 32; C4 +2.3 %.
    const uint32_t big = (tune.big > 1u && n_gran >= n_wv * tune.big_min) ? tune.big : 1u;
    const uint32_t mid_keep = n_wv * tune.big_keep / gran_per_chunk;  // ordinary chunks kept for the end of the bulk (32 granules per wave)
    const uint32_t n_big = big > 1u ? (n_bulk - (mid_keep < n_bulk ? mid_keep : n_bulk)) / big : 0u;  // grabs of `big` chunks each
    const uint32_t n_grabs = n_big + (n_bulk - n_big * big) + (n_gran - n_bulk * gran_per_chunk);
    bool first_grab = true;  // wave-uniform
    uint32_t my_grabs = 0u;  // wave-uniform
    // Launches of single granules only (fewer than tune.static_small = 8 per resident wave) do not use the cursor at all: wave w
    // takes granules w, w + n_wv, w + 2 n_wv, ...  A grab through the cursor stalls the whole wave for the atomic's round trip,
    // and a one-sample call's two big launches made 32 k + 19 k of them in ~170 us each (one-sample calls 1,350 -> 1,510 per
    // second, 2 / 4 samples per call +11 / +6 %, 8-32 samples +1 to +3 % through their late bounces; with a threshold of 32 and
    // more the dealt-out launches of 16+ samples lose 2-5 % to imbalance; TUNING.md)
    const bool static_small = n_gran < n_wv * tune.static_small;
    const uint32_t my_xcd = xcc_id();
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = lane_id();
    const uint32_t wv = tid >> 6;
    const uint32_t wbase = tid & ~63u;
    if (tid < 8) {
        s_iters[tid] = 0;
        s_qn[tid] = 0u;
    }
    __syncthreads();
    uint32_t* const queue = &s_queue[wv * T8_QCAP];
    uint32_t k = 0xFFFFFFFFu;
    f3 o = mk3(0.f, 0.f, 0.f), ld = mk3(0.f, 0.f, 1.f);
    float ix = 1.f, iy = 1.f, iz = 1.f, anx = 0.f, any = 0.f, anz = 0.f, afx = 0.f, afy = 0.f, afz = 0.f, pad = 0.f, tlimit = 0.f;
    uint32_t octinv4 = 0x07070707u;  // (7 - direction octant) in every byte
    uint32_t gx = 0u, gy = 0u;    // current node group
    bool pending = false;         // this lane has items in the wave's queue
    // INST only: level (0 = top-level tree, world ray; 1 = inside an instance, local ray), the instance, the pending
    // instance hits of the current top-level node, the culling-bound conversion (world distance -> local parameter)
    bool in_blas = false, stall = false;
    uint32_t inst = 0u, ipb = 0u, ipm = 0u;
    float lscale = 1.0f, padw4 = 0.0f;
    int sp = 0;
    bool overflow = false;
    Closest best;
    best.d2 = 3.402823466e+38f;
    best.id = HIT_MISS;
    best.prim = 0xFFFFFFFFu;
    uint32_t n_nodes = 0, n_tris = 0, max_sp = 0;
    uint32_t cur = 0, cur_end = 0;  // wave-uniform: this wave's current chunk [cur, cur_end)
    bool exhausted = false;         // wave-uniform
    // a triangle phase starts once this many triangle groups are queued; at most 63 more arrive with the step that reaches it
    const uint32_t tri_min = tune.tri_min < T8_QGROUPS - 64u ? tune.tri_min : T8_QGROUPS - 64u;
    // STATS: shader cycles (s_memtime) this wave spent in the three sections of an outer iteration
    unsigned long long cyc_refill = 0, cyc_node = 0, cyc_tri = 0, t_mark = STATS ? __builtin_amdgcn_s_memtime() : 0ull;
    // launch timeline (PRT_TIMELINE_WORDS): s_memrealtime is the constant 100 MHz clock all XCDs share (s_memtime, used
    // for the phase split, counts each XCD's own shader clock)
    const unsigned long long t_start = STATS ? __builtin_amdgcn_s_memrealtime() : 0ull;
    unsigned long long t_exh = 0ull;  // STATS: when this wave found the ray buffer exhausted
    uint32_t ray_steps = 0u, ray_steps_max = 0u;  // STATS: node steps of the lane's current ray / of its longest ray
    // Exit condition every wave reaches: the loop ends when the ray buffer is exhausted and the wave's lanes are
    // idle; every outer iteration makes progress (a node step, a triangle phase or a refill); the iteration cap is
    // a watchdog that turns a would-be hang into an error flag the host reports.
    for (uint32_t guard = 0;; ++guard) {
        if (guard > (1u << 22)) {
            if (lane == 0) atomicOr(work + 256, 1u);
            break;
        }
        unsigned long long helped = 0ull;  // STEAL: root lanes that have helpers at work (wave-uniform)
        if (STEAL && exhausted) {  // (all lanes are active here; two OR scans instead of one readlane per helper: a draining
            // wave has up to 63 of them and pays this in every outer iteration)
            const bool helper = k >= 0xFFFFFF00u && k != 0xFFFFFFFFu;
            if (__ballot(helper) != 0ull) {
                const uint32_t r = k & 63u;
                const uint32_t lo = wave_scan_or((helper && r < 32u) ? 1u << r : 0u);
                const uint32_t hi = wave_scan_or((helper && r >= 32u) ? 1u << (r - 32u) : 0u);
                helped = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)hi, 63) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
            }
        }
        // a lane is released only when nothing of its ray is left in the queue (the testers read the owner's ray)
        if (k != 0xFFFFFFFFu && !pending && !(INST && (in_blas || ipm != 0u))) {
            if (overflow) {
                if (PATH) {  // (the host only uses this instance for trees its stack holds: an error prt_synchronize reports)
                    atomicOr(work + 256, 2u);
                    need_shade = true;
                } else if (INST) {
                    atomicOr(work + 256, 2u);  // no fallback for two-level scenes: prt_synchronize reports it
                } else {
                    const uint32_t j = atomicAdd(ovf, 1u);  // re-done from scratch by the spill-capable 4-wide instance
                    if (j < PRT_OVF_CAP)
                        ovf[1u + j] = k;
                    else
                        atomicOr(work + 256, 2u);
                }
                overflow = false;
                if (!PATH) k = 0xFFFFFFFFu;
            } else if (!(gy > 0x00FFFFFFu) && sp == 0) {
                if (PATH) {
                    need_shade = true;  // the lane keeps its path; the shade step below goes on with it
                } else if (STEAL && k >= 0xFFFFFF00u) {  // a helper (k = 0xFFFFFF00 | root lane): its subtree is done
                    k = 0xFFFFFFFFu;
                } else if (!STEAL || ((helped >> lane) & 1ull) == 0ull) {
                    st_stream(&hit[k], LEAN ? ((volatile uint32_t*)s_slot)[tid] : best.id);
#ifdef PRT_PROBE_REBOUND  // diagnostic build: leave the final distance where the next launch takes its initial bound from
                    ((float*)hd2)[k] = LEAN ? __uint_as_float((uint32_t)(((volatile unsigned long long*)s_key)[tid] >> 32)) : best.d2;
#endif
                    k = 0xFFFFFFFFu;
                }
            }
        }
        // (up to three rounds of pairing per outer iteration: a thief that received a group with several pending children, or a
        // donor with more stack entries, gives again at once; one-sample calls 1,303 -> 1,360 per second, no more from 4 or 6)
#ifndef PRT_STEAL_PASSES
#define PRT_STEAL_PASSES 3
#endif
        if (STEAL && exhausted && tune.steal != 0u)  // wave-uniform
        for (int steal_pass = 0; steal_pass < PRT_STEAL_PASSES; ++steal_pass) {
            // a donor gives its bottom stack entry, or, with an empty stack, the far half of its current group's pending children
            const uint32_t gh = gy >> 24;
            const bool can_give = k != 0xFFFFFFFFu && (sp > 0 || (gh & (gh - 1u)) != 0u);
            const unsigned long long free_m = __ballot(k == 0xFFFFFFFFu);
            const unsigned long long give_m = __ballot(can_give);
            const uint32_t n_free = (uint32_t)__popcll(free_m), n_give = (uint32_t)__popcll(give_m);
            if (n_free >= tune.steal && n_give != 0u) {
                // the queue is empty here (every triangle phase tests all of it): its first words pair thieves and donors
                const uint32_t n_pair = n_free < n_give ? n_free : n_give;
                const unsigned long long below = (1ull << lane) - 1ull;
                const uint32_t give_rank = (uint32_t)__popcll(give_m & below), free_rank = (uint32_t)__popcll(free_m & below);
                const bool donor = can_give && give_rank < n_pair;
                const bool thief = k == 0xFFFFFFFFu && free_rank < n_pair;
                if (donor) {
                    queue[give_rank] = lane;
                    if (sp == 0) {  // split the current group: the lowest-priority half of its hits goes through stack row 0
                        uint32_t far = 0u, rest = gh;
                        for (uint32_t i = (uint32_t)__popc(gh) >> 1; i != 0u; --i) {
                            far |= rest & (0u - rest);
                            rest &= rest - 1u;
                        }
                        s_stack[tid] = make_uint2(gx, (far << 24) | (gy & 0x00FFFFFFu));
                        gy = (rest << 24) | (gy & 0x00FFFFFFu);
                        sp = 1;  // (taken off again right below)
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                const uint32_t src = thief ? ((volatile uint32_t*)queue)[free_rank] : lane;
                const unsigned long long e64 = ((volatile unsigned long long*)s_stack)[wbase + src];  // the donor's bottom entry
                const uint2 e = make_uint2((uint32_t)e64, (uint32_t)(e64 >> 32));
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (donor) {
                    for (int i = 1; i < sp; ++i) s_stack[(i - 1) * 256 + tid] = s_stack[i * 256 + tid];
                    --sp;
                }
                // the ray's constants come out of the donor's registers (every lane takes part in the shuffles)
                const uint32_t k_src = (uint32_t)__shfl((int)k, (int)src, 64);
                const float t_ix = __shfl(ix, (int)src, 64), t_iy = __shfl(iy, (int)src, 64), t_iz = __shfl(iz, (int)src, 64);
                const float t_anx = __shfl(anx, (int)src, 64), t_any = __shfl(any, (int)src, 64), t_anz = __shfl(anz, (int)src, 64);
                const float t_afx = __shfl(afx, (int)src, 64), t_afy = __shfl(afy, (int)src, 64), t_afz = __shfl(afz, (int)src, 64);
                const float t_pad = __shfl(pad, (int)src, 64);
                const uint32_t t_oct = (uint32_t)__shfl((int)octinv4, (int)src, 64);
                if (thief) {
                    const uint32_t root = k_src >= 0xFFFFFF00u ? (k_src & 63u) : src;
                    k = 0xFFFFFF00u | root;
                    ix = t_ix; iy = t_iy; iz = t_iz;
                    anx = t_anx; any = t_any; anz = t_anz;
                    afx = t_afx; afy = t_afy; afz = t_afz;
                    pad = t_pad;
                    octinv4 = t_oct;
                    gx = e.x;
                    gy = e.y;
                    sp = 0;
                    tlimit = limit_from_d2(__uint_as_float((uint32_t)(((volatile unsigned long long*)s_key)[wbase + root] >> 32)), pad);
                }
            } else {
                break;
            }
        }
        const bool idle = k == 0xFFFFFFFFu;
        const unsigned long long idle_mask = __ballot(idle);
        const uint32_t n_idle = (uint32_t)__popcll(idle_mask);
        bool do_sw = false;  // wave-uniform
        if (INST) {
            // Level switches (enter the next instance hit of a top-level node / leave an exhausted instance) cost ~150
            // instructions plus the instance record's gather.  Lanes that need one wait (stall) and the wave does them
            // together, under the same rule as the refill: when refill_min lanes are idle or waiting.  No lane has
            // items in the queue here (the triangle phase of the previous iteration emptied it), so the queued
            // triangles never see a ray other than the one they were found with.
            const uint32_t n_sw = (uint32_t)__popcll(__ballot(stall));
            do_sw = n_sw != 0u && n_idle + n_sw >= tune.refill_min;
            if (do_sw && stall) {
                const int spr = sp > 0 ? sp - 1 : 0;
                const bool has = gy > 0x00FFFFFFu;
                const bool enter = !in_blas;
                f3 dw = mk3(s_wray[3 * 256 + tid], s_wray[4 * 256 + tid], s_wray[5 * 256 + tid]);
                o = mk3(s_wray[0 * 256 + tid], s_wray[1 * 256 + tid], s_wray[2 * 256 + tid]);
                const float pad_w = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + sc.extent);
                // leaving an instance while the same top-level node has more instance hits goes straight into the
                // next one (the sentinel stays): no world-ray round trip in between
                const bool next = ipm != 0u;
                if (next) {
                    inst = sc.tlas_inst[ipb + (uint32_t)__builtin_ctz(ipm)];
                    ipm &= ipm - 1u;
                    if (enter) {
                        if (has) {  // the remaining top-level siblings wait below the sentinel
                            s_stack[sp * 256 + tid] = make_uint2(gx, gy);
                            ++sp;
                        }
                        s_stack[(sp <= STACK_L ? sp : STACK_L) * 256 + tid] = make_uint2(T8_SENTINEL, 0xFF000000u);
                        ++sp;
                    }
                    const DevInstance& I = sc.insts[inst];
                    o = transform_point(I.inv, o);      // primitive.cpp:29
                    ld = transform_normal(I.mat, dw);   // primitive.cpp:30
                    pad = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + I.extent);
                    lscale = I.inv_scale * 1.000001f;
                    padw4 = 4.0f * pad_w;
                    gx = I.root;
                    in_blas = true;
                } else {
                    sp = spr;  // pop the sentinel
                    ld = normalize3(dw);
                    pad = pad_w;
                    lscale = 1.0f;
                    padw4 = 0.0f;
                    gx = 0u;
                    in_blas = false;
                }
                ix = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
                iy = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
                iz = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
                const bool nx = ix < 0.0f, ny = iy < 0.0f, nz = iz < 0.0f;
                anx = (nx ? o.x - pad : o.x + pad) * ix; afx = (nx ? o.x + pad : o.x - pad) * ix;
                any = (ny ? o.y - pad : o.y + pad) * iy; afy = (ny ? o.y + pad : o.y - pad) * iy;
                anz = (nz ? o.z - pad : o.z + pad) * iz; afz = (nz ? o.z + pad : o.z - pad) * iz;
                octinv4 = (7u - ((nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u))) * 0x01010101u;
                tlimit = (limit_from_d2(best.d2, 0.0f) + padw4) * lscale + 4.0f * pad;
                gy = next ? (1u << (24u + (octinv4 & 7u))) : 0u;  // the instance's root "group" / nothing pending
                if (sp > STACK_L) {  // no room left: give the ray up (an error the host reports)
                    overflow = true;
                    gy = 0u;
                    sp = 0;
                    ipm = 0u;
                    in_blas = false;
                }
                stall = false;
            }
        }
        if (PATH) {
            // The shade step of the waiting lanes and new paths for the idle ones, together: when refill_min lanes wait or
            // are idle, or when no lane of the wave has anything left to walk or to test.
            const unsigned long long shade_m = __ballot(need_shade);
            const uint32_t n_wait = n_idle + (uint32_t)__popcll(shade_m);
            const bool others_busy = __ballot(k != 0xFFFFFFFFu && !need_shade) != 0ull;
            if ((shade_m != 0ull || (!exhausted && n_idle != 0u)) && (n_wait >= tune.refill_min || !others_busy)) {
                bool fresh = false;
                if (!exhausted && n_idle != 0u) {
                    if (cur == cur_end) {  // grab the next chunk / granule of path ids (as the ray hand-out above)
                        uint32_t c = blockIdx.x * 4u + wv;
                        if (!first_grab) {
                            if (n_grabs <= n_wv) c = n_grabs;  // (every grab went out with the waves' first ones)
                            else if (lane == 0) c = atomicAdd(work, 1u) + n_wv;
                            c = (uint32_t)__shfl((int)c, 0, 64);
                        }
                        first_grab = false;
                        if (c >= n_grabs) {
                            exhausted = true;
                        } else {
                            // grab c: [0, n_big) big grabs, then the ordinary chunks, then the single granules
                            const uint32_t cb = c - n_big + n_big * big;  // (c >= n_big) the grab's index counted in ordinary chunks
                            const uint32_t g0 = c < n_big ? c * big * gran_per_chunk : cb < n_bulk ? cb * gran_per_chunk : n_bulk * gran_per_chunk + (cb - n_bulk);
                            const uint32_t g1 = c < n_big ? g0 + big * gran_per_chunk : cb < n_bulk ? g0 + gran_per_chunk : g0 + 1u;
                            cur = g0 << 6;
                            cur_end = (g1 << 6) < count ? (g1 << 6) : count;
                        }
                    }
                    if (!exhausted) {
                        const uint32_t qi = cur + (uint32_t)__popcll(idle_mask & ((1ull << lane) - 1ull));
                        fresh = idle && qi < cur_end;
                        if (fresh) k = qi;
                        cur = (cur + n_idle < cur_end) ? cur + n_idle : cur_end;
                    }
                }
                // r: 0 = the path has ended (rad written), 1 = walk (o, pd) from its analytic hit (id0, d2_0),
                //    2 = shade hit `id` of the segment (o, pd) next
                int r = 0;
                uint32_t id = HIT_MISS, id0 = HIT_MISS;
                float d2_0 = 3.402823466e+38f;
                if (fresh) {  // k_raygen's arithmetic for path k = sample * n_pix_local + local pixel
                    const uint32_t smp = k / pa.tm.n_pix_local, pl = k - smp * pa.tm.n_pix_local;
                    uint32_t px, py;
                    if (!tile_pixel(pa.tm, pl, px, py)) {  // a partial tile's pixel outside the image: no path
                        pa.rad[k] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));
                    } else {
                        prng = path_seed(py * pa.tm.W + px, pa.first_sample + smp, pa.seed);
                        float fx = (float)px + 0.5f, fy = (float)py + 0.5f;  // pixel centre (cpu/renderer.cpp:45)
                        if (pa.sp.jitter) {  // (x + u1, y + u2): the path's first two draws (optix/device_programs.cu:172-173)
                            const float u1 = rnd01(prng);
                            const float u2 = rnd01(prng);
                            fx = (float)px + u1;
                            fy = (float)py + u2;
                        }
                        camera_ray(pa.cam, fx, fy, o, pd);
                        pthr = mk3(1.f, 1.f, 1.f);
                        pdepth = 0u;
                        r = classify_ray<false, 256>(sc, o, pd, id0, d2_0) ? 1 : 2;
                        id = id0;
                    }
                }
                if (need_shade) {
                    r = 2;
                    id = best.id;
                    need_shade = false;
                }
                while (r == 2) {  // (a segment that cannot hit a triangle is shaded right away: its hit is the analytic one)
                    r = advance_path<1, false, false, 256>(sc, id, o, pd, pthr, prng, pdepth, pa.max_depth, pa.sp, &pa.rad[k], id0, d2_0);
                    id = id0;
                }
                if (r == 1) {  // start the walk of (o, pd): the set-up of a refill
                    ld = normalize3(pd);  // TransformNormal(identity, d), primitive.cpp:30
                    pad = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + sc.extent);
                    ix = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
                    iy = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
                    iz = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
                    const bool nx = ix < 0.0f, ny = iy < 0.0f, nz = iz < 0.0f;
                    anx = (nx ? o.x - pad : o.x + pad) * ix; afx = (nx ? o.x + pad : o.x - pad) * ix;
                    any = (ny ? o.y - pad : o.y + pad) * iy; afy = (ny ? o.y + pad : o.y - pad) * iy;
                    anz = (nz ? o.z - pad : o.z + pad) * iz; afz = (nz ? o.z + pad : o.z - pad) * iz;
                    octinv4 = (7u - ((nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u))) * 0x01010101u;
                    best.id = id0;
                    best.prim = id0;  // analytic index, or 0xFFFFFFFF for a miss
                    best.d2 = d2_0;
                    tlimit = limit_from_d2(best.d2, pad);
                    gx = 0u;  // the root "group": node 0, one pending hit that decodes to slot 0
                    gy = 1u << (24u + (octinv4 & 7u));
                    sp = 0;
                } else if ((fresh || ((shade_m >> lane) & 1ull)) && r == 0) {
                    k = 0xFFFFFFFFu;  // the path is over: the lane is idle again
                }
            }
        }
        if (!PATH && !exhausted && (n_idle >= tune.refill_min || (INST && do_sw && n_idle != 0u))) {
            if (cur == cur_end) {  // grab the next chunk / granule
                uint32_t c = blockIdx.x * 4u + wv;
                if (!first_grab) {
                    if (n_grabs <= n_wv) c = n_grabs;  // (every grab went out with the waves' first ones)
                    else if (static_small) c += my_grabs * n_wv;  // (a small launch: wave w takes granules w, w + n_wv, ...: no cursor)
                    else if (lane == 0) c = atomicAdd(work, 1u) + n_wv;
                    c = (uint32_t)__shfl((int)c, 0, 64);
                }
                first_grab = false;
                ++my_grabs;
                if (c >= n_grabs) {
                    exhausted = true;
                    if (STATS) t_exh = __builtin_amdgcn_s_memrealtime();
                } else {
                    // grab c: [0, n_big) big grabs, then the ordinary chunks, then the single granules
                    const uint32_t cb = c - n_big + n_big * big;  // (c >= n_big) the grab's index counted in ordinary chunks
                    const uint32_t g0 = c < n_big ? c * big * gran_per_chunk : cb < n_bulk ? cb * gran_per_chunk : n_bulk * gran_per_chunk + (cb - n_bulk);
                    const uint32_t g1 = c < n_big ? g0 + big * gran_per_chunk : cb < n_bulk ? g0 + gran_per_chunk : g0 + 1u;
                    cur = g0 << 6;
                    cur_end = (g1 << 6) < count ? (g1 << 6) : count;
                }
            }
            if (!exhausted) {
                const uint32_t qi_seq = cur + (uint32_t)__popcll(idle_mask & ((1ull << lane) - 1ull));
                if (idle && qi_seq < cur_end) {
                    const uint32_t qi = (!PRIM && tune.perm) ? tune.perm[qi_seq] : qi_seq;  // (sort_rays: a measurement aid)
                    uint32_t hid = PRIM ? HIT_MISS : ld_stream(&hit[qi]);
                    if (hid != HIT_DEAD && !(ANY && !SEEDED && hid != HIT_MISS)) {  // (ANY: an analytic hit below tmax already blocks; SEEDED: it is the seed)
                        float4 O, D;
                        float hd2_0 = 0.0f;
                        if (PRIM) {
                            f3 po, pd;
                            uint32_t pixel, sample, lp;
                            primary_ray(pr, ld_stream(&pr.pid[qi]), po, pd, pixel, sample, &lp);
                            const float4 E = pr.pix[pr.ids.n_pix_local + lp];  // the pixel's analytic hit (k_raygen)
                            hid = __float_as_uint(E.y);
                            hd2_0 = E.z;
                            // every primary ray starts at the camera, a kernel argument: left visible, the compiler hoists
                            // everything that depends on the origin alone (o +- pad, |o|_1, ...) out of the persistent loop
                            // and keeps it in VGPRs for the kernel's life, 8 of which it then spills (36 B of scratch, 8
                            // scratch loads per refill); opaque, the same values cost 8 VALU instructions per refill
#ifndef PRT_NO_OPAQUE_ORIGIN  // (A/B builds)
                            asm volatile("" : "+v"(po.x), "+v"(po.y), "+v"(po.z));
#endif
                            O = make_float4(po.x, po.y, po.z, 0.f);
                            D = make_float4(pd.x, pd.y, pd.z, 0.f);
                        } else {
                            O = ld_stream(&ro[qi]);
                            D = ld_stream(&rd[qi]);
                        }
                        o = mk3(O.x, O.y, O.z);
                        ld = normalize3(mk3(D.x, D.y, D.z));  // TransformNormal(identity, d), primitive.cpp:30
                        pad = sc.pad * (__builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z) + sc.extent);
                        ix = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.x) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.x) : ld.x);
                        iy = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.y) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.y) : ld.y);
                        iz = __builtin_amdgcn_rcpf(__builtin_fabsf(ld.z) < PRT_DIR_MIN ? __builtin_copysignf(PRT_DIR_MIN, ld.z) : ld.z);
                        // (v_rcp_f32, 1 ulp, instead of IEEE divisions: these reciprocals only feed the box tests, whose
                        // pad of 2^-18 of the coordinates' magnitude is 32x the 2^-23 that costs; the triangle tests use the
                        // ray itself)
                        // near planes move out by -pad, far planes by +pad (the near plane is the box's max plane
                        // on an axis the ray travels along negatively):  t = plane * inv - (o +- pad) * inv
                        const bool nx = ix < 0.0f, ny = iy < 0.0f, nz = iz < 0.0f;
                        anx = (nx ? o.x - pad : o.x + pad) * ix; afx = (nx ? o.x + pad : o.x - pad) * ix;
                        any = (ny ? o.y - pad : o.y + pad) * iy; afy = (ny ? o.y + pad : o.y - pad) * iy;
                        anz = (nz ? o.z - pad : o.z + pad) * iz; afz = (nz ? o.z + pad : o.z - pad) * iz;
                        octinv4 = (7u - ((nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u))) * 0x01010101u;
                        best.id = hid;
                        best.prim = hid;  // analytic index, or 0xFFFFFFFF for a miss
                        best.d2 = PRIM ? hd2_0 : ld_stream(&hd2[qi]);
                        tlimit = limit_from_d2(best.d2, pad);
                        if (LEAN) {
                            s_lray[0 * 256 + tid] = o.x; s_lray[1 * 256 + tid] = o.y; s_lray[2 * 256 + tid] = o.z;
                            s_lray[3 * 256 + tid] = ld.x; s_lray[4 * 256 + tid] = ld.y; s_lray[5 * 256 + tid] = ld.z;
                            s_key[tid] = ((unsigned long long)__float_as_uint(best.d2) << 32) | (hid == HIT_MISS ? 0u : hid);
                            s_slot[tid] = hid;
                        }
                        k = qi;
                        if (STATS) ray_steps = 0u;
                        gx = 0u;  // the root "group": node 0, one pending hit that decodes to slot 0
                        gy = 1u << (24u + (octinv4 & 7u));
                        sp = 0;
                        if (INST) {
                            in_blas = false;
                            stall = false;
                            ipm = 0u;
                            lscale = 1.0f;
                            padw4 = 0.0f;
                            s_wray[0 * 256 + tid] = O.x; s_wray[1 * 256 + tid] = O.y; s_wray[2 * 256 + tid] = O.z;
                            s_wray[3 * 256 + tid] = D.x; s_wray[4 * 256 + tid] = D.y; s_wray[5 * 256 + tid] = D.z;
                        }
                    }
                }
                cur = (cur + n_idle < cur_end) ? cur + n_idle : cur_end;
            }
        }
        if (__ballot(k != 0xFFFFFFFFu) == 0ull) {
            if (exhausted) break;
            continue;
        }
        if (STATS) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            cyc_refill += t - t_mark;
            t_mark = t;
        }
        // ---- phase 1: node steps.  Triangles found go straight to the wave's queue and the lane keeps walking;
        // leave when at most exit_max lanes can still walk or enough work for a triangle phase has piled up ----
        bool walk = (k != 0xFFFFFFFFu) && ((gy > 0x00FFFFFFu) || sp > 0 || (INST && ipm != 0u)) && !(INST && stall);
        // Triangle groups queued by this run of the node loop.  The queue is empty on entry (a triangle phase tests all of
        // it), every lane still in the loop adds the same ballot counts, and a lane that has left the loop does not come
        // back before the next phase: the lanes in the loop agree on it, so a slot is base + rank in the ballot, without
        // an atomic and without a per-triangle loop in the node step.
        uint32_t q_groups = 0u;
        while (walk) {
            uint32_t tm = 0u, tb = 0u;
            {
                // current group: G while it has pending internal hits, else the top of the stack (read unconditionally)
                const int spr = sp > 0 ? sp - 1 : 0;
                const uint2 top = s_stack[spr * 256 + tid];
                const bool has = gy > 0x00FFFFFFu;
                bool level_switch = false;
                if (INST) {
                    const bool enter = !in_blas && ipm != 0u;               // instance hits of the last top-level node first
                    const bool leave = in_blas && !has && top.x == T8_SENTINEL;  // the instance's tree is exhausted
                    if (enter || leave) {  // level switches are done by the whole wave together, next to the refill
                        stall = true;
                        walk = false;
                        level_switch = true;
                    }
                }
                if (!level_switch) {
                    const uint32_t cx = has ? gx : top.x;
                    uint32_t cy = has ? gy : top.y;
                    sp = has ? sp : spr;
                    const uint32_t bit = 31u - (uint32_t)__builtin_clz(cy);  // highest pending hit: bits 24..31
                    cy &= ~(1u << bit);
                    s_stack[sp * 256 + tid] = make_uint2(cx, cy);  // the remaining siblings (kept only if there are any)
                    sp += (cy > 0x00FFFFFFu) ? 1 : 0;
                    const uint32_t slot = (bit - 24u) ^ (octinv4 & 7u);
                    const uint32_t idx = cx + (uint32_t)__popc(cy & ((1u << slot) - 1u));  // bits 0..7 of cy: imask
                    const uint4* nb = sc.nodes8 + (size_t)sc.node_stride * idx;
                    const uint4 w0 = nb[0], w1 = nb[1], w2 = nb[2], w3 = nb[3], w4 = nb[4];
                    if (STATS) {
                        ++n_nodes;
                        ++ray_steps;
                        if (ray_steps > ray_steps_max) ray_steps_max = ray_steps;
                        if ((int)lane == __ffsll((long long)__ballot(true)) - 1) ++s_iters[wv];
                        if ((uint32_t)sp > max_sp) max_sp = (uint32_t)sp;
                    }
                    T8_BOXTEST()
                    gx = w1.x;
                    gy = (hitmask & 0xFF000000u) | (eim >> 24);
                    tm = hitmask & 0x00FFFFFFu;
                    tb = w1.y;
                    if (sp > stack_cap) {  // give the ray up; it is re-traversed through the overflow list
                        overflow = true;
                        gy = 0u;
                        sp = 0;
                        tm = 0u;
                        if (INST) {
                            ipm = 0u;
                            in_blas = false;
                        }
                    } else if (INST && !in_blas) {  // top-level node: its "triangles" are instances, entered one by one
                        ipb = tb;
                        ipm = tm;
                        tm = 0u;
                    }
                    walk = (gy > 0x00FFFFFFu) || sp > 0 || (INST && ipm != 0u);
                }
            }
            const unsigned long long qm = __ballot(tm != 0u);
            if (tm != 0u) {
                const uint32_t own = (STEAL && k >= 0xFFFFFF00u) ? (k & 63u) : lane;  // a helper's tests belong to its root
                const uint32_t pos = q_groups + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(qm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)qm, 0u));
                ((uint2*)queue)[pos] = make_uint2(tb, (own << 24) | tm);
                s_qn[wv] = q_groups + (uint32_t)__popcll(qm);  // (the same value from every queueing lane)
                pending = true;
            }
            q_groups += (uint32_t)__popcll(qm);
            if ((uint32_t)__popcll(__ballot(walk)) <= tune.exit_max || q_groups >= tri_min) break;
        }
        if (STATS) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            cyc_node += t - t_mark;
            t_mark = t;
        }
        // ---- phase 2: the queued triangle groups become (ray, triangle) pairs, one pair per lane per round ----
        {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const uint32_t G = ((volatile uint32_t*)s_qn)[wv];  // group items in the queue (wave-uniform)
            if (G != 0u) {
                // a miss is encoded with prim 0 so that a candidate with d2 == FLT_MAX can never win (primitive.cpp:44)
                const unsigned long long key_best =
                    LEAN ? 0ull : ((unsigned long long)__float_as_uint(best.d2) << 32) | (best.id == HIT_MISS ? 0u : best.prim);
                if (!LEAN) s_key[tid] = key_best;
                if (lane == 0) s_qn[wv] = 0u;
                // Sets of 64 group items, one per lane, taken into registers; after that the queue memory holds pair items.
                // While a second set waits (G > 64: rare, the node loop stops at tri_min groups) the pairs of the first one
                // stay in the lower half of the queue's memory, below the second set's items.
                for (uint32_t g0 = 0u; g0 < G; g0 += 64u) {  // wave-uniform, at most two trips
                const uint32_t cap = (G - g0 > 64u) ? T8_QCAP / 2u : T8_QCAP;
                const unsigned long long ga = g0 + lane < G ? ((volatile unsigned long long*)queue)[g0 + lane] : 0ull;
                const uint32_t base_a = (uint32_t)ga, own_a = (uint32_t)(ga >> 56);
                uint32_t ma = (uint32_t)(ga >> 32) & 0x00FFFFFFu;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                // passes of at most `cap` pairs (one pass unless the set holds more: 2-3 triangles per group on average);
                // groups are expanded in queue order, whole groups only (a group has at most 24 triangles: progress)
                while (__ballot(ma != 0u) != 0ull) {  // wave-uniform
                    const uint32_t ca = (uint32_t)__popc(ma);
                    const uint32_t ia = wave_scan_add(ca);
                    const bool fit_a = ia <= cap;  // true for a prefix of the lanes
                    const uint32_t nfa = (uint32_t)__popcll(__ballot(fit_a));
                    const uint32_t T = (uint32_t)__shfl((int)ia, (int)(nfa - 1u), 64);  // (nfa >= 1: the first group fits)
                    if (fit_a && ca) {
                        uint32_t qp = ia - ca;
                        for (uint32_t m = ma; m; m &= m - 1u) queue[qp++] = (own_a << 26) | (base_a + (uint32_t)__builtin_ctz(m));
                        ma = 0u;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    for (uint32_t base = 0; base < T; base += 64u) {  // wave-uniform trip count
                        const uint32_t kq = base + lane;
                        const bool act = kq < T;
                        const uint32_t item = ((volatile uint32_t*)queue)[act ? kq : 0u];
                        const uint32_t owner = act ? (item >> 26) : lane;
                        const uint32_t slot = item & 0x03FFFFFFu;
                        f3 qo, qd;
                        if (LEAN) {
                            const uint32_t oc = wbase + owner;
                            qo = mk3(s_lray[0 * 256 + oc], s_lray[1 * 256 + oc], s_lray[2 * 256 + oc]);
                            qd = mk3(s_lray[3 * 256 + oc], s_lray[4 * 256 + oc], s_lray[5 * 256 + oc]);
                        } else {
                            qo = mk3(__shfl(o.x, (int)owner, 64), __shfl(o.y, (int)owner, 64), __shfl(o.z, (int)owner, 64));
                            qd = mk3(__shfl(ld.x, (int)owner, 64), __shfl(ld.y, (int)owner, 64), __shfl(ld.z, (int)owner, 64));
                        }
                        uint32_t qinst = 0u, win = slot;
                        if (INST) qinst = (uint32_t)__shfl((int)inst, (int)owner, 64);
                        bool cand = false;
                        unsigned long long key = 0ull;
                        if (act) {
                            const float4 a = sc.tris[3 * (size_t)slot + 0];
                            const float4 b = sc.tris[3 * (size_t)slot + 1];
                            const float4 c = sc.tris[3 * (size_t)slot + 2];
                            if (STATS) ++n_tris;
                            f3 pos;
                            float b1, b2;
                            if (triangle_hit_pos(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), qo, qd, pos, b1, b2)) {
                                float d2;
                                uint32_t prim;
                                if (INST) {  // position back through Mat, distance in world space (primitive.cpp:38-43)
                                    const DevInstance& I = sc.insts[qinst];
                                    const uint32_t oc = wbase + owner;
                                    d2 = dist2(mk3(s_wray[0 * 256 + oc], s_wray[1 * 256 + oc], s_wray[2 * 256 + oc]), transform_point(I.mat, pos));
                                    prim = I.prim_base + __float_as_uint(a.w);
                                    win = I.virt_base + (slot - I.slot_base);
                                } else {
                                    d2 = dist2(qo, pos);
                                    prim = __float_as_uint(a.w);
                                }
                                key = ((unsigned long long)__float_as_uint(d2) << 32) | prim;
                                // NaN / inf d2 have bit patterns above FLT_MAX's: they can never win, as in the reference
                                if (ANY)  // only a key below the bound is a blocker: a candidate equal to the seed (prim 0, d2 == tmax^2) is not
                                    cand = key < atomicMin(&s_key[wbase + owner], key);
                                else {
                                    cand = true;
                                    atomicMin(&s_key[wbase + owner], key);
                                }
                            }
                        }
                        if (STATS && lane == 0) ++s_iters[4 + wv];
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                        if (cand && ((volatile unsigned long long*)s_key)[wbase + owner] == key) s_slot[wbase + owner] = LEAN ? sc.n_prims + win : win;
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    }
                }
                }
                const unsigned long long won =
                    ((volatile unsigned long long*)s_key)[(STEAL && k >= 0xFFFFFF00u && k != 0xFFFFFFFFu) ? wbase + (k & 63u) : tid];
                if (LEAN) {
                    tlimit = limit_from_d2(__uint_as_float((uint32_t)(won >> 32)), pad);  // same value if nothing changed
                    // ANY: the ray (of this lane, or of the root it helps) has a blocker once its slot names a triangle
                    if (ANY && k != 0xFFFFFFFFu) {
                        const uint32_t sl = ((volatile uint32_t*)s_slot)[(STEAL && k >= 0xFFFFFF00u) ? wbase + (k & 63u) : tid];
                        if (sl != HIT_MISS && (!SEEDED || sl >= sc.n_prims)) {  // (SEEDED: an analytic id is the seed, not a blocker)
                            gy = 0u;
                            sp = 0;
                        }
                    }
                } else if (won != key_best) {
                    best.d2 = __uint_as_float((uint32_t)(won >> 32));
                    best.prim = (uint32_t)won;
                    best.id = sc.n_prims + ((volatile uint32_t*)s_slot)[tid];
                    tlimit = INST ? (limit_from_d2(best.d2, 0.0f) + padw4) * lscale + 4.0f * pad : limit_from_d2(best.d2, pad);
                    if (ANY && k != 0xFFFFFFFFu) {  // a blocker: drop the stack, the pending group and (INST) the level state
                        gy = 0u;
                        sp = 0;
                        if (INST) {
                            ipm = 0u;
                            in_blas = false;
                            stall = false;
                        }
                    }
                }
                pending = false;  // everything that was queued has been tested
            }
        }
        if (STATS) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            cyc_tri += t - t_mark;
            t_mark = t;
        }
    }
    if (STATS) {
        if (lane == 0) {
            atomicAdd(&stats[6], cyc_refill);
            atomicAdd(&stats[7], cyc_node);
            atomicAdd(&stats[8], cyc_tri);
            unsigned long long* tl = stats + 16 + PRT_TIMELINE_WORDS * tune.probe_slot;
            const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
            if (t_exh == 0ull) t_exh = t_end;
            if (my_xcd == 0u) {  // the XCDs' clocks are offset against each other: launch-level marks from XCD 0's waves only
                atomicMin(&tl[0], t_start);
                atomicMax(&tl[1], t_end);
                atomicMin(&tl[2], t_exh);
                atomicMax(&tl[3], t_exh);
            }
            atomicAdd(&tl[4], t_end - t_exh);
            atomicAdd(&tl[5], t_end - t_start);
            atomicAdd(&tl[6], 1ull);
        }
        // one atomic per wave and counter (1.3 M lanes adding to the same words used to take milliseconds)
        uint32_t w_nodes = n_nodes, w_tris = n_tris, w_steps = ray_steps_max, w_sp = max_sp;
        for (int off = 32; off > 0; off >>= 1) {
            w_nodes += (uint32_t)__shfl_xor((int)w_nodes, off, 64);
            w_tris += (uint32_t)__shfl_xor((int)w_tris, off, 64);
            const uint32_t a = (uint32_t)__shfl_xor((int)w_steps, off, 64), b = (uint32_t)__shfl_xor((int)w_sp, off, 64);
            w_steps = a > w_steps ? a : w_steps;
            w_sp = b > w_sp ? b : w_sp;
        }
        if (lane == 0) {
            atomicMax(&stats[16 + PRT_TIMELINE_WORDS * tune.probe_slot + 7], (unsigned long long)w_steps);
            atomicAdd(&stats[0], (unsigned long long)w_nodes);
            atomicAdd(&stats[1], (unsigned long long)w_tris);
            atomicMax(&stats[5], (unsigned long long)w_sp);
        }
        __syncthreads();
        if (threadIdx.x < 4) atomicAdd(&stats[3], 64ull * s_iters[threadIdx.x]);
        if (threadIdx.x < 4) atomicAdd(&stats[4], 64ull * s_iters[4 + threadIdx.x]);
    }
}

template <int STACK_L, int WAVES, bool STATS, bool INST, bool LEAN = false, bool PRIM = false, bool PATH = false>
__global__ void __launch_bounds__(256, WAVES) k_traverse8_persistent(DevScene sc, const float4* __restrict__ ro,
                                                                    const float4* __restrict__ rd,
                                                                    uint32_t* __restrict__ hit,
                                                                    const float* __restrict__ hd2,
                                                                    const uint32_t* __restrict__ count_ptr,
                                                                    uint32_t* __restrict__ work,
                                                                    uint32_t* __restrict__ ovf, PrtTravTuning tune,
                                                                    unsigned long long* __restrict__ stats, PrtPrimary pr,
                                                                    PrtPathArgs pa) {
    traverse8_body<STACK_L, WAVES, STATS, INST, LEAN, PRIM, PATH, false>(sc, ro, rd, hit, hd2, count_ptr, work, ovf, tune,
                                                                         stats, pr, pa);
}

// Occlusion queries (prt_occluded): the any-hit walk of the 8-wide tree.  hit[] holds HIT_MISS for the rays to walk
// (anything else is final: HIT_DEAD, or an analytic blocker), hd2[] their seeded bound tmax^2.  On return hit[] holds a
// blocker's id or HIT_MISS; rays that overflowed the LDS stack are on the overflow list (one-level trees) as in
// k_traverse8_persistent.
template <int STACK_L, int WAVES, bool INST, bool LEAN = false>
__global__ void __launch_bounds__(256, WAVES) k_occluded8_persistent(DevScene sc, const float4* __restrict__ ro,
                                                                    const float4* __restrict__ rd,
                                                                    uint32_t* __restrict__ hit,
                                                                    const float* __restrict__ hd2,
                                                                    const uint32_t* __restrict__ count_ptr,
                                                                    uint32_t* __restrict__ work,
                                                                    uint32_t* __restrict__ ovf, PrtTravTuning tune) {
    traverse8_body<STACK_L, WAVES, false, INST, LEAN, false, false, true>(sc, ro, rd, hit, hd2, count_ptr, work, ovf, tune,
                                                                          nullptr, PrtPrimary{}, PrtPathArgs{});
}

// The last walk of a batch on the last-segment route, setting 2: the SEEDED any-hit walk (traverse8_body).  hit[] holds the
// closest-hit walk's seeds, an analytic id or HIT_MISS at hd2[], all of them walked; on return a triangle id where one lies
// in front of the seed, the seed elsewhere.  A kernel of its own: the instances of k_occluded8_persistent keep their code.
template <int STACK_L, int WAVES, bool INST, bool LEAN = false>
__global__ void __launch_bounds__(256, WAVES) k_occluded8_seeded(DevScene sc, const float4* __restrict__ ro,
                                                                const float4* __restrict__ rd, uint32_t* __restrict__ hit,
                                                                const float* __restrict__ hd2,
                                                                const uint32_t* __restrict__ count_ptr,
                                                                uint32_t* __restrict__ work, uint32_t* __restrict__ ovf,
                                                                PrtTravTuning tune) {
    traverse8_body<STACK_L, WAVES, false, INST, LEAN, false, false, true, true>(sc, ro, rd, hit, hd2, count_ptr, work, ovf, tune,
                                                                                nullptr, PrtPrimary{}, PrtPathArgs{});
}

// ---------------------------------------------------------------------------------------------------------
// Shade + scatter + compaction (ShadeHitsKernel, renderer.cu:274-335; the miss branch of
// IntersectClosestKernel, renderer.cu:263-271; path logic of TraceRayGPU, cuda_megakernel/renderer.cu:81-119).
// Radiance can only be non-zero at the event that ends a path (emissive materials never scatter,
// material.h:119-122), so the path carries throughput only and writes rad[path] once, when it ends.
// ---------------------------------------------------------------------------------------------------------
// (ENV / env: see advance_path; k_shade passes false / null and keeps its code, k_shade_env is the instance with an image)
template <int FUSE, bool SAMPLING, bool INST, bool ABVH, bool PRIM, bool ENV, bool TEX = false>
PRT_DEV void shade_step(DevScene sc, const float4* __restrict__ ro, const float4* __restrict__ rd, const float4* __restrict__ rt,
                        const uint32_t* __restrict__ hit, float4* __restrict__ no, float4* __restrict__ nd, float4* __restrict__ nt,
                        uint32_t* __restrict__ nhit, float* __restrict__ nhd2, float4* __restrict__ rad, uint32_t* __restrict__ counts,
                        uint32_t* __restrict__ work, uint32_t iter, uint32_t max_depth_arg, uint32_t cap, PrtSampling sp_arg, PrtPrimary pr,
                        const DevEnv* env, const DevTex* tex = nullptr) {
    const bool last_route = (max_depth_arg & PRT_LAST_SEGMENT_FLAG) != 0u;  // (advance_path)
    const uint32_t max_depth = max_depth_arg & ~PRT_LAST_SEGMENT_FLAG;
    // PRIM: the first k_shade of a batch whose k_raygen stored compact primary rays (PrtPrimary): ray, RNG seed,
    // throughput (1,1,1) and segment index (0) follow from the path id
    const PrtSampling sp = SAMPLING ? sp_arg : PrtSampling{0u, 0u, 0.0f};
    const uint32_t nA = CNT_A(counts, iter), nB = CNT_B(counts, iter);
    const uint32_t count = nA + nB;
    if (blockIdx.x * (uint32_t)SHADE_BLOCK >= count) return;  // whole block exits together
    const uint32_t k = blockIdx.x * (uint32_t)SHADE_BLOCK + threadIdx.x;
    if (k < 8u) work[32u * k] = 0u;  // chunk cursors of the next bounce's traversal kernel
    if (k == 8u) work[512] = 0u;     // its overflow-list counter
    bool front = false, back = false;
    f3 o = mk3(0.f, 0.f, 0.f), d = mk3(0.f, 0.f, 1.f), thr = mk3(0.f, 0.f, 0.f);
    uint32_t id0 = HIT_MISS, rng = 0, depth = 0, pid = 0;
    float d2_0 = 3.402823466e+38f;
    float4 pre_a = make_float4(0.f, 0.f, 0.f, 0.f), pre_b = pre_a;
    if (k < count) {
        const uint32_t src = k < nA ? k : cap - 1u - (k - nA);  // front part, then back part
        uint32_t id = (PRIM && (k >= nA || pr.walk)) ? HIT_MISS : ld_stream(&hit[src]);
        if (PRIM) {
            pid = ld_stream(&pr.pid[src]);
            uint32_t pixel, sample, lp;
            primary_ray(pr, pid, o, d, pixel, sample, &lp);
            // a back-side primary ray was never walked: its closest hit is the analytic scan's, kept per pixel (k_raygen);
            // a front-side one was walked once for its pixel (walk = 1): the hit sits at the pixel's list slot (in big
            // batches a wave holds the samples of one pixel: both loads are wave-uniform)
            if (k >= nA) id = __float_as_uint(pr.pix[pr.ids.n_pix_local + lp].y);
            else if (pr.walk) id = hit[__float_as_uint(pr.pix[pr.ids.n_pix_local + lp].x)];
            rng = path_seed(pixel, pr.first_sample + sample, pr.seed);
            depth = 0u;
            thr = mk3(1.f, 1.f, 1.f);
            pre_a = pr.pix[2u * pr.ids.n_pix_local + lp];
            pre_b = pr.pix[3u * pr.ids.n_pix_local + lp];
        } else {
            const float4 O = ld_stream(&ro[src]);
            const float4 D = ld_stream(&rd[src]);
            const float4 T = ld_stream(&rt[src]);
            pid = __float_as_uint(O.w);
            rng = __float_as_uint(D.w);
            depth = __float_as_uint(T.w);  // segment index of this ray (paths advance at different rates, see advance_path)
            thr = mk3(T.x, T.y, T.z);
            o = mk3(O.x, O.y, O.z);
            d = mk3(D.x, D.y, D.z);
        }
        if (id != HIT_DEAD) {
            const int r = advance_path<1 + FUSE, INST, ABVH, SHADE_BLOCK, PRIM, ENV, TEX, FUSE == 0>(sc, id, o, d, thr, rng, depth, max_depth, sp, &rad[pid], id0, d2_0, pre_a, pre_b, env, tex, last_route);
            front = r == 1;
            back = r == 2;
        }
    }
    const uint32_t slot = block_alloc2<SHADE_BLOCK>(front, back, false, &CNT_A(counts, iter + 1u), &CNT_B(counts, iter + 1u),
                                                    &CNT_C(counts, iter + 1u), cap);
    if (slot != 0xFFFFFFFFu) {
        st_stream(&no[slot], make_float4(o.x, o.y, o.z, __uint_as_float(pid)));
        st_stream(&nd[slot], make_float4(d.x, d.y, d.z, __uint_as_float(rng)));
        st_stream(&nt[slot], make_float4(thr.x, thr.y, thr.z, __uint_as_float(depth)));
        st_stream(&nhit[slot], id0);
        st_stream(&nhd2[slot], d2_0);
    }
}

template <int FUSE, bool SAMPLING, bool INST, bool ABVH, bool PRIM = false>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade(DevScene sc, const float4* __restrict__ ro,
                                                      const float4* __restrict__ rd, const float4* __restrict__ rt,
                                                      const uint32_t* __restrict__ hit, float4* __restrict__ no,
                                                      float4* __restrict__ nd, float4* __restrict__ nt,
                                                      uint32_t* __restrict__ nhit, float* __restrict__ nhd2,
                                                      float4* __restrict__ rad, uint32_t* __restrict__ counts,
                                                      uint32_t* __restrict__ work, uint32_t iter, uint32_t max_depth,
                                                      uint32_t cap, PrtSampling sp_arg, PrtPrimary pr) {
    shade_step<FUSE, SAMPLING, INST, ABVH, PRIM, false>(sc, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, rad, counts, work, iter, max_depth,
                                                        cap, sp_arg, pr, nullptr);
}

// k_shade under an environment image: one segment per call, sampling options compiled in
template <bool INST, bool ABVH>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_env(DevScene sc, DevEnv env, const float4* __restrict__ ro,
                                                          const float4* __restrict__ rd, const float4* __restrict__ rt,
                                                          const uint32_t* __restrict__ hit, float4* __restrict__ no,
                                                          float4* __restrict__ nd, float4* __restrict__ nt,
                                                          uint32_t* __restrict__ nhit, float* __restrict__ nhd2,
                                                          float4* __restrict__ rad, uint32_t* __restrict__ counts,
                                                          uint32_t* __restrict__ work, uint32_t iter, uint32_t max_depth,
                                                          uint32_t cap, PrtSampling sp_arg) {
    shade_step<0, true, INST, ABVH, false, true>(sc, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, rad, counts, work, iter, max_depth, cap,
                                                 sp_arg, PrtPrimary{}, &env);
}

// k_shade / k_shade_env under a texture binding (include/prt.h "Image textures"): one segment per call, sampling options
// compiled in; `env` is read only by the ENV instances
template <bool INST, bool ABVH, bool ENV>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_tex(DevScene sc, DevTex tex, DevEnv env, const float4* __restrict__ ro,
                                                          const float4* __restrict__ rd, const float4* __restrict__ rt,
                                                          const uint32_t* __restrict__ hit, float4* __restrict__ no,
                                                          float4* __restrict__ nd, float4* __restrict__ nt,
                                                          uint32_t* __restrict__ nhit, float* __restrict__ nhd2,
                                                          float4* __restrict__ rad, uint32_t* __restrict__ counts,
                                                          uint32_t* __restrict__ work, uint32_t iter, uint32_t max_depth,
                                                          uint32_t cap, PrtSampling sp_arg) {
    shade_step<0, true, INST, ABVH, false, ENV, true>(sc, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, rad, counts, work, iter, max_depth, cap,
                                                      sp_arg, PrtPrimary{}, ENV ? &env : nullptr, &tex);
}

// Compact primary rays: the surface interaction of a pixel's primary hit, ONCE per pixel.  Without jitter every sample of
// a pixel traces the same pixel-centre ray (cpu/renderer.cpp:45) and finds the same closest hit, so the first k_shade of a
// batch used to rebuild the same position / normal / material (Triangle::Intersect or the analytic shape again: ~150 wave
// instructions) once per SAMPLE; a wave there holds 64 samples of one pixel.  This kernel rebuilds it per PIXEL from the
// pixel's walked hit (pr.walk: hit[list slot]; one walk per sample: the hit of the pixel's first stored sample), and
// k_shade<PRIM> uses the record for every sample whose own hit id equals the record's (otherwise it computes the hit itself).
__global__ void __launch_bounds__(256) k_primary_hit(DevScene sc, PrtPrimary pr, const uint32_t* __restrict__ hit,
                                                     float4* __restrict__ pix, const uint32_t* __restrict__ counts) {
    const uint32_t pl = blockIdx.x * 256u + threadIdx.x;
    if (pl >= pr.ids.n_pix_local) return;
    const float4 E = pix[pr.ids.n_pix_local + pl];
    float4 a = make_float4(0.f, 0.f, 0.f, __uint_as_float(HIT_DEAD)), b = make_float4(0.f, 0.f, 0.f, 0.f);  // no record
    if (__float_as_uint(E.w) == 0xFFFFFFFEu) {  // the pixel's paths were stored
        // front pixels (a list slot, not the sentinel; one walk per sample: a ray slot below the front count) were walked:
        // their hit is the traversal's; back-side paths keep the analytic scan's hit of the pixel's record
        const uint32_t first = __float_as_uint(E.x);
        const bool walked = pr.walk ? first != 0xFFFFFFFFu : first < CNT_A(counts, 0);
        const uint32_t id = walked ? hit[first] : __float_as_uint(E.y);
        if (id != HIT_MISS && id != HIT_DEAD) {
            const float4 P = pix[pl];
            WorldHit w;
            world_hit_from_id<false>(sc, id, mk3(pr.origin[0], pr.origin[1], pr.origin[2]), mk3(P.x, P.y, P.z), w);
            if (w.has) {
                a = make_float4(w.pos.x, w.pos.y, w.pos.z, __uint_as_float(id));
                b = make_float4(w.normal.x, w.normal.y, w.normal.z, __uint_as_float(w.material | (w.front ? 0x80000000u : 0u)));
            }
        }
    }
    pix[2u * pr.ids.n_pix_local + pl] = a;
    pix[3u * pr.ids.n_pix_local + pl] = b;
}

// Diagnostic (prt_measure_shade_divergence, tools/shade_divergence.py; SURVEY 8f-4 "material-coherent work queues",
// wavefront.md:92-93): what a wave of k_shade finds in its 64 ray slots, by the material of the hit.  Per bounce, 16 words:
// [0] waves, [1] lanes with a ray, [2 + t] lanes whose hit has material type t (0 = miss / none, 1 Lambertian, 2 Metal,
// 3 Dielectric, 4 Emissive), [8 + t] waves in which type t occurs, [14] sum over waves of the number of distinct SCATTERING
// types (1..3) present, [15] waves with at least one scattering lane.  A wave executes the scatter code of every type it
// holds, so [14] / [15] is the factor by which material divergence multiplies the scatter work.
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_divstats(DevScene sc, const uint32_t* __restrict__ hit,
                                                                 const uint32_t* __restrict__ counts, uint32_t iter, uint32_t cap,
                                                                 unsigned long long* __restrict__ out, PrtPrimary pr, int compact) {
    const uint32_t nA = CNT_A(counts, iter), nB = CNT_B(counts, iter);
    const uint32_t count = nA + nB;
    if (blockIdx.x * (uint32_t)SHADE_BLOCK >= count) return;
    const uint32_t k = blockIdx.x * (uint32_t)SHADE_BLOCK + threadIdx.x;
    uint32_t type = 5u;  // no ray
    if (k < count) {
        const uint32_t src = k < nA ? k : cap - 1u - (k - nA);
        uint32_t id;
        if (compact && (k >= nA || pr.walk)) {  // compact primary rays: a back-side path's hit is its pixel's analytic one, a front-side one its pixel's walked one (k_shade<PRIM>)
            f3 o_, d_;
            uint32_t pixel, sample, lp;
            primary_ray(pr, pr.pid[src], o_, d_, pixel, sample, &lp);
            const float4 E = pr.pix[pr.ids.n_pix_local + lp];
            id = k >= nA ? __float_as_uint(E.y) : hit[__float_as_uint(E.x)];
        } else {
            id = hit[src];
        }
        type = 0u;
        if (id != HIT_MISS && id != HIT_DEAD) {
            uint32_t m;
            if (id < sc.n_prims) {
                m = sc.prims[id].material;
            } else if (sc.n_insts) {
                const uint32_t v = id - sc.n_prims;
                uint32_t lo = 0, hi = sc.n_insts;
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (sc.insts[mid].virt_base <= v) lo = mid; else hi = mid;
                }
                const DevInstance& I = sc.insts[lo];
                m = I.material == 0xFFFFFFFFu ? __float_as_uint(sc.tris[3 * (size_t)(I.slot_base + (v - I.virt_base)) + 1].w) : I.material;
            } else {
                m = __float_as_uint(sc.tris[3 * (size_t)(id - sc.n_prims) + 1].w);
            }
            type = sc.mat_type[m] <= 4u ? sc.mat_type[m] : 0u;
        }
    }
    unsigned long long* o = out + 16u * iter;
    const uint32_t lane = lane_id();
    uint32_t distinct = 0u;
    for (uint32_t t = 0; t < 5u; ++t) {
        const unsigned long long mk = __ballot(type == t);
        if (mk != 0ull && lane == 0u) {
            atomicAdd(&o[2 + t], (unsigned long long)__popcll(mk));
            atomicAdd(&o[8 + t], 1ull);
        }
        if (t >= 1u && t <= 3u && mk != 0ull) ++distinct;
    }
    const unsigned long long any = __ballot(type != 5u);
    if (lane == 0u && any != 0ull) {
        atomicAdd(&o[0], 1ull);
        atomicAdd(&o[1], (unsigned long long)__popcll(any));
        if (distinct) {
            atomicAdd(&o[14], (unsigned long long)distinct);
            atomicAdd(&o[15], 1ull);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Film accumulate (Film::AddSample, src/core/film.cu:37-55; BlitRadianceKernel + addBufferGPU,
// renderer.cu:337-348, film.cu:79-88): samples are added in sample order, weight 1 each.
// film_local is tile-ordered [n_pix_local] float4 {r_sum, g_sum, b_sum, weight}.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_accumulate(const float4* __restrict__ rad, float4* __restrict__ film_local,
                                                    PrtTileMap tm, uint32_t S, uint32_t max_depth, int update_film,
                                                    unsigned long long* __restrict__ ray_stats,
                                                    const float4* __restrict__ pix_end) {
    // pix_end (compact primary rays, optional): per local pixel what its paths deliver if they all ended with their
    // primary ray (w != 0xFFFFFFFE); those S identical values are not in rad[] and are added from the record.
    // rad[path] = {radiance, index of the path's last segment}.  Ray segments at depth d = paths whose last segment
    // index is >= d: a per-block histogram of the last indices (wave ballots -> LDS) gives the per-depth counts.
    // A block takes several groups of 256 pixels (grid-stride): its per-depth counts reach the global counters with ONE
    // atomic per depth per block, and a counter word only executes ~87 atomics per microsecond (tools/atomic_rate.hip): with
    // one block per 256 pixels a 1080p frame was 8,100 atomics per word = 93 us, most of a one-sample k_accumulate.
    __shared__ uint32_t s_ends[PRT_MAX_DEPTH];
    if (threadIdx.x < PRT_MAX_DEPTH) s_ends[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t pl0 = blockIdx.x * 256u; pl0 < tm.n_pix_local; pl0 += gridDim.x * 256u) {  // block-uniform trip count
    const uint32_t pl = pl0 + threadIdx.x;
    uint32_t x, y;
    const bool valid = pl < tm.n_pix_local && tile_pixel(tm, pl, x, y);
    float4 f = valid ? film_local[pl] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 E = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFEu));
    if (valid && pix_end) E = pix_end[pl];
    const bool ended = __float_as_uint(E.w) != 0xFFFFFFFEu;
    const float weight = 1.0f;
    const uint32_t lane = lane_id();
    // Samples are added in sample order (that fixes the fp32 sum), but their loads do not depend on each other: eight
    // at a time are in flight (a rank of an 8-GPU run has only four blocks per CU here, too few to hide the latency of
    // one load per iteration)
    for (uint32_t s0 = 0; s0 < S; s0 += 8u) {  // block-uniform trip counts
        float4 r[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j)
            r[j] = (valid && !ended && s0 + j < S) ? ld_stream(&rad[(size_t)(s0 + j) * tm.n_pix_local + pl]) : E;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            if (s0 + j >= S) break;
            uint32_t e = 0xFFFFFFFFu;
            if (valid) {
                f.x += r[j].x * weight;
                f.y += r[j].y * weight;
                f.z += r[j].z * weight;
                f.w += weight;
                e = __float_as_uint(r[j].w);
            }
            for (uint32_t dd = 0; dd < max_depth; ++dd) {
                const unsigned long long mk = __ballot(e == dd);
                if (mk != 0ull && lane == 0) atomicAdd(&s_ends[dd], (uint32_t)__popcll(mk));
            }
        }
    }
    if (valid && update_film) film_local[pl] = f;
    }
    __syncthreads();
    if (threadIdx.x < max_depth) {
        unsigned long long n = 0;
        for (uint32_t e = threadIdx.x; e < max_depth; ++e) n += s_ends[e];
        // (PRT_RAY_STAT_SLOTS copies of the counters, summed by the host when it reads them: a single word would execute only
        // ~87 of these atomics per microsecond, a floor of 23 us for 2,048 blocks, half of a one-sample k_accumulate)
        if (n) atomicAdd(&ray_stats[(blockIdx.x & (PRT_RAY_STAT_SLOTS - 1u)) * PRT_MAX_DEPTH + threadIdx.x], n);
    }
}

// Lighting modes (PrtLighting): k_accumulate where a sample is rad[path] + lrad[path], the path's terminal radiance plus the
// sum of its light samples (without a light sample lrad is +0 and the sum is rad bit for bit); no compact primary rays.
// (A separate kernel, not a template parameter of k_accumulate: the lighting-off instance keeps its code.)
__global__ void __launch_bounds__(256) k_accumulate_lit(const float4* __restrict__ rad, const float4* __restrict__ lrad,
                                                        float4* __restrict__ film_local, PrtTileMap tm, uint32_t S,
                                                        uint32_t max_depth, int update_film,
                                                        unsigned long long* __restrict__ ray_stats) {
    // rad[path] = {radiance, index of the path's last segment}.  Ray segments at depth d = paths whose last segment
    // index is >= d: a per-block histogram of the last indices (wave ballots -> LDS) gives the per-depth counts.
    // A block takes several groups of 256 pixels (grid-stride): its per-depth counts reach the global counters with ONE
    // atomic per depth per block, and a counter word only executes ~87 atomics per microsecond (tools/atomic_rate.hip): with
    // one block per 256 pixels a 1080p frame was 8,100 atomics per word = 93 us, most of a one-sample k_accumulate.
    __shared__ uint32_t s_ends[PRT_MAX_DEPTH];
    if (threadIdx.x < PRT_MAX_DEPTH) s_ends[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t pl0 = blockIdx.x * 256u; pl0 < tm.n_pix_local; pl0 += gridDim.x * 256u) {  // block-uniform trip count
    const uint32_t pl = pl0 + threadIdx.x;
    uint32_t x, y;
    const bool valid = pl < tm.n_pix_local && tile_pixel(tm, pl, x, y);
    float4 f = valid ? film_local[pl] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 E = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));
    const float weight = 1.0f;
    const uint32_t lane = lane_id();
    // Samples are added in sample order (that fixes the fp32 sum), but their loads do not depend on each other: eight
    // at a time are in flight (a rank of an 8-GPU run has only four blocks per CU here, too few to hide the latency of
    // one load per iteration)
    for (uint32_t s0 = 0; s0 < S; s0 += 8u) {  // block-uniform trip counts
        float4 r[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j)
            r[j] = (valid && s0 + j < S) ? ld_stream(&rad[(size_t)(s0 + j) * tm.n_pix_local + pl]) : E;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            if (valid && s0 + j < S) {
                const float4 l = ld_stream(&lrad[(size_t)(s0 + j) * tm.n_pix_local + pl]);
                r[j].x = r[j].x + l.x;
                r[j].y = r[j].y + l.y;
                r[j].z = r[j].z + l.z;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            if (s0 + j >= S) break;
            uint32_t e = 0xFFFFFFFFu;
            if (valid) {
                f.x += r[j].x * weight;
                f.y += r[j].y * weight;
                f.z += r[j].z * weight;
                f.w += weight;
                e = __float_as_uint(r[j].w);
            }
            for (uint32_t dd = 0; dd < max_depth; ++dd) {
                const unsigned long long mk = __ballot(e == dd);
                if (mk != 0ull && lane == 0) atomicAdd(&s_ends[dd], (uint32_t)__popcll(mk));
            }
        }
    }
    if (valid && update_film) film_local[pl] = f;
    }
    __syncthreads();
    if (threadIdx.x < max_depth) {
        unsigned long long n = 0;
        for (uint32_t e = threadIdx.x; e < max_depth; ++e) n += s_ends[e];
        // (PRT_RAY_STAT_SLOTS copies of the counters, summed by the host when it reads them: a single word would execute only
        // ~87 of these atomics per microsecond, a floor of 23 us for 2,048 blocks, half of a one-sample k_accumulate)
        if (n) atomicAdd(&ray_stats[(blockIdx.x & (PRT_RAY_STAT_SLOTS - 1u)) * PRT_MAX_DEPTH + threadIdx.x], n);
    }
}

// Film statistics (prt_set_film_statistics): k_accumulate / k_accumulate_lit (LIT: a sample is rad + lrad) that also keep the
// second moments of the samples' luminance, stat[pixel] = {A, Q}: per sample, in sample order, y = (0.2126 r + 0.7152 g) +
// 0.0722 b of exactly the r, g, b added to the film, A += y, Q += y y (single fp32 operations, never contracted).  The film
// gets the same additions in the same order as without statistics.  (Kernels of their own: the two above keep their code.)
// LIST (a pass of prt_render_adaptive; PrtBatchView): tm counts the listed tiles; rad / lrad are indexed by compact local
// pixels, film_local and stat by (list[pl >> 6] << 6) + lane.  No pix_end then, and none with LIT.
template <bool LIT, bool LIST>
__global__ void __launch_bounds__(256) k_accumulate_stat(const float4* __restrict__ rad, const float4* __restrict__ lrad,
                                                         float4* __restrict__ film_local, float2* __restrict__ stat, PrtTileMap tm,
                                                         uint32_t S, uint32_t max_depth, int update_film,
                                                         unsigned long long* __restrict__ ray_stats,
                                                         const float4* __restrict__ pix_end, const uint32_t* __restrict__ list) {
    __shared__ uint32_t s_ends[PRT_MAX_DEPTH];  // per-depth ray counts: see k_accumulate
    if (threadIdx.x < PRT_MAX_DEPTH) s_ends[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t pl0 = blockIdx.x * 256u; pl0 < tm.n_pix_local; pl0 += gridDim.x * 256u) {  // block-uniform trip count
    const uint32_t pl = pl0 + threadIdx.x;
    const bool in_range = pl < tm.n_pix_local;
    uint32_t fl = pl;  // the pixel's place in film_local
    if (LIST && in_range) fl = (list[pl >> 6] << 6) | (pl & 63u);
    uint32_t x, y;
    const bool valid = in_range && tile_pixel(tm, fl, x, y);
    float4 f = valid ? film_local[fl] : make_float4(0.f, 0.f, 0.f, 0.f);
    float2 m2 = valid ? stat[fl] : make_float2(0.f, 0.f);
    float4 E = make_float4(0.f, 0.f, 0.f, __uint_as_float((LIT || LIST) ? 0xFFFFFFFFu : 0xFFFFFFFEu));
    if (!LIT && !LIST && valid && pix_end) E = pix_end[pl];
    const bool ended = !LIT && !LIST && __float_as_uint(E.w) != 0xFFFFFFFEu;
    const float weight = 1.0f;
    const uint32_t lane = lane_id();
    for (uint32_t s0 = 0; s0 < S; s0 += 8u) {  // block-uniform trip counts; eight loads in flight (k_accumulate)
        float4 r[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j)
            r[j] = (valid && !ended && s0 + j < S) ? ld_stream(&rad[(size_t)(s0 + j) * tm.n_pix_local + pl]) : E;
        if (LIT) {
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {
                if (valid && s0 + j < S) {
                    const float4 l = ld_stream(&lrad[(size_t)(s0 + j) * tm.n_pix_local + pl]);
                    r[j].x = r[j].x + l.x;
                    r[j].y = r[j].y + l.y;
                    r[j].z = r[j].z + l.z;
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            if (s0 + j >= S) break;
            uint32_t e = 0xFFFFFFFFu;
            if (valid) {
                f.x += r[j].x * weight;
                f.y += r[j].y * weight;
                f.z += r[j].z * weight;
                f.w += weight;
                const float lum = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, r[j].x), __fmul_rn(0.7152f, r[j].y)), __fmul_rn(0.0722f, r[j].z));
                m2.x = __fadd_rn(m2.x, lum);
                m2.y = __fadd_rn(m2.y, __fmul_rn(lum, lum));
                e = __float_as_uint(r[j].w);
            }
            for (uint32_t dd = 0; dd < max_depth; ++dd) {
                const unsigned long long mk = __ballot(e == dd);
                if (mk != 0ull && lane == 0) atomicAdd(&s_ends[dd], (uint32_t)__popcll(mk));
            }
        }
    }
    if (valid && update_film) {
        film_local[fl] = f;
        stat[fl] = m2;
    }
    }
    __syncthreads();
    if (threadIdx.x < max_depth) {
        unsigned long long n = 0;
        for (uint32_t e = threadIdx.x; e < max_depth; ++e) n += s_ends[e];
        if (n) atomicAdd(&ray_stats[(blockIdx.x & (PRT_RAY_STAT_SLOTS - 1u)) * PRT_MAX_DEPTH + threadIdx.x], n);
    }
}

// Pixel-major path ids (prt_path_id.h; compact primary rays, batches of at least 8 samples): k_accumulate (STAT = false) and
// k_accumulate_stat<false, false> (STAT = true) for rad[pixel * S + sample].  Still one thread per pixel, the same additions in
// the same order (s = 0 .. S - 1: that fixes the fp32 sums) and the same per-depth histogram; what differs is who loads.  The
// samples of a pixel are adjacent now, so a lane that loaded its own pixel's next eight samples would touch a 128-B line of
// its own per load instruction, 64 lines per instruction instead of 8 (measured: 4.42 ms instead of 1.25 ms on C3).  Instead a
// wave loads the next eight samples of its 64 pixels COOPERATIVELY, eight lanes per pixel (one full line per pixel where S is
// a multiple of 8), eight pixels per load instruction, eight instructions in flight, and transposes them through LDS: lane p
// then reads pixel p's eight samples.  Rows are padded to nine float4 (stride 36 dwords: the 16 lanes of a ds_read_b128 pass
// fall on distinct banks).  Pixels outside the image or ended by their primary ray (pix_end) are not loaded.
#ifndef PRT_ACC_PM_CHUNK
#define PRT_ACC_PM_CHUNK 8  // samples per chunk: 8, or 16 (A/B: 128-thread blocks, two waves per SIMD, 2.39 ms on C3)
#endif
#define PRT_ACC_PM_BLOCK (PRT_ACC_PM_CHUNK == 8 ? 256 : 128)
template <bool STAT>
__global__ void __launch_bounds__(PRT_ACC_PM_BLOCK) k_accumulate_pixel_major(const float4* __restrict__ rad, float4* __restrict__ film_local,
                                                                float2* __restrict__ stat, PrtTileMap tm, uint32_t S, uint32_t max_depth,
                                                                int update_film, unsigned long long* __restrict__ ray_stats,
                                                                const float4* __restrict__ pix_end) {
    __shared__ uint32_t s_ends[PRT_MAX_DEPTH];  // per-depth ray counts: see k_accumulate
    constexpr uint32_t C = PRT_ACC_PM_CHUNK, ROW = C + 1u, BLOCK = PRT_ACC_PM_BLOCK;
    __shared__ float4 s_t[BLOCK / 64u][64u * ROW];  // per wave: [pixel of the wave][sample of the chunk], rows padded by one
    if (threadIdx.x < PRT_MAX_DEPTH) s_ends[threadIdx.x] = 0u;
    __syncthreads();
    const PrtPathIdOrder ids{tm.n_pix_local, 0.0f, S, 0u, 0u};  // (encode only)
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    float4* const t = s_t[wave];
    for (uint32_t pl0 = blockIdx.x * BLOCK; pl0 < tm.n_pix_local; pl0 += gridDim.x * BLOCK) {  // block-uniform trip count
    const uint32_t pl = pl0 + threadIdx.x;
    const uint32_t wave_pl = pl0 + 64u * wave;  // the wave's first pixel
    uint32_t x, y;
    const bool valid = pl < tm.n_pix_local && tile_pixel(tm, pl, x, y);
    float4 f = valid ? film_local[pl] : make_float4(0.f, 0.f, 0.f, 0.f);
    float2 m2 = make_float2(0.f, 0.f);
    if (STAT && valid) m2 = stat[pl];
    float4 E = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFEu));
    if (valid && pix_end) E = pix_end[pl];
    const bool ended = __float_as_uint(E.w) != 0xFFFFFFFEu;
    const unsigned long long need = __ballot(valid && !ended);  // the wave's pixels whose samples are in rad[]
    const float weight = 1.0f;
    // The per-depth histogram of the last segment indices.  k_accumulate's wave ballot per sample and depth is most of its
    // instructions (40 of ~55 per eight samples at max_depth 5), and with the transposition's LDS this kernel has half its
    // occupancy to hide them behind.  Up to eight depths each lane counts its own pixel's indices in the bytes of one 64-bit
    // register instead (index e adds 1 << 8 e) and adds the bytes to the block's counters every 31 chunks (248 samples: a byte
    // cannot overflow) and after the last one; counts do not depend on the order.  Deeper paths keep the ballots.
    const bool packed = max_depth <= 8u;
    unsigned long long h = 0ull;
    // load instruction j of a chunk: C lanes per pixel, pixel (64 / C) j + lane / C of the wave, sample s0 + lane % C
    const uint32_t cs = lane % C, cq = lane / C;
    float4 v[C];
    auto load_chunk = [&](uint32_t s0) {
#pragma unroll
        for (uint32_t j = 0; j < C; ++j) {
            const uint32_t q = (64u / C) * j + cq;
            v[j] = (((need >> q) & 1ull) != 0ull && s0 + cs < S) ? ld_stream(&rad[prt_path_id_encode(ids, wave_pl + q, s0 + cs)]) : E;
        }
    };
    load_chunk(0u);
    for (uint32_t s0 = 0; s0 < S; s0 += C) {  // block-uniform trip counts
        // The rows belong to this wave alone and a wave's LDS instructions execute in order, so what orders the writes of the
        // eight loaders of a row against its reader (and the reads against the next chunk's writes) is the order of the
        // instructions: wave-level fences keep the compiler from moving them, no other wave has to wait.
#pragma unroll
        for (uint32_t j = 0; j < C; ++j) t[((64u / C) * j + cq) * ROW + cs] = v[j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (s0 + C < S) load_chunk(s0 + C);  // the next chunk's loads fly while this one is summed
#pragma unroll
        for (uint32_t j = 0; j < C; ++j) {
            if (s0 + j >= S) break;
            uint32_t e = 0xFFFFFFFFu;
            if (valid) {
                const float4 r = ended ? E : t[lane * ROW + j];
                f.x += r.x * weight;
                f.y += r.y * weight;
                f.z += r.z * weight;
                f.w += weight;
                if (STAT) {  // (k_accumulate_stat's single fp32 operations)
                    const float lum = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, r.x), __fmul_rn(0.7152f, r.y)), __fmul_rn(0.0722f, r.z));
                    m2.x = __fadd_rn(m2.x, lum);
                    m2.y = __fadd_rn(m2.y, __fmul_rn(lum, lum));
                }
                e = __float_as_uint(r.w);
            }
            if (packed) {
                if (e < 8u) h += 1ull << (8u * e);
            } else {
                for (uint32_t dd = 0; dd < max_depth; ++dd) {
                    const unsigned long long mk = __ballot(e == dd);
                    if (mk != 0ull && lane == 0) atomicAdd(&s_ends[dd], (uint32_t)__popcll(mk));
                }
            }
        }
        if (packed && ((s0 / C) % 31u == 30u || s0 + C >= S)) {
            for (uint32_t dd = 0; dd < max_depth; ++dd) {
                const uint32_t n = (uint32_t)(h >> (8u * dd)) & 0xFFu;
                if (n) atomicAdd(&s_ends[dd], n);
            }
            h = 0ull;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next chunk overwrites the rows)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (valid && update_film) {
        film_local[pl] = f;
        if (STAT) stat[pl] = m2;
    }
    }
    __syncthreads();
    if (threadIdx.x < max_depth) {
        unsigned long long n = 0;
        for (uint32_t e = threadIdx.x; e < max_depth; ++e) n += s_ends[e];
        if (n) atomicAdd(&ray_stats[(blockIdx.x & (PRT_RAY_STAT_SLOTS - 1u)) * PRT_MAX_DEPTH + threadIdx.x], n);
    }
}

// Tile selection of prt_render_adaptive: one wave per tile of the previous list (prev = null: local tile w itself), one pixel
// per lane.  A pixel outside the image is converged; the others by prt_adaptive_rule on their film weight and moments.  The tile
// stays active while any lane is unconverged: a ballot, so the decision involves no floating-point reduction.
__global__ void __launch_bounds__(256) k_tile_select(const float4* __restrict__ film_local, const float2* __restrict__ stat,
                                                     PrtTileMap tm, const uint32_t* __restrict__ prev, uint32_t n_in, float threshold,
                                                     float noise_floor, uint32_t* __restrict__ flags) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);  // wave-uniform
    if (w >= n_in) return;
    const uint32_t t = prev ? prev[w] : w;
    const uint32_t pl = (t << 6) | lane_id();
    uint32_t x, y;
    bool unconverged = false;
    const bool inside = tile_pixel(tm, pl, x, y);
    if (inside) {
        const float2 m2 = stat[pl];
        unconverged = prt_adaptive_rule(film_local[pl].w, m2.x, m2.y, threshold, noise_floor);
    }
    const unsigned long long mk = __ballot(unconverged), in_image = __ballot(inside);
    // the flag of an active tile is its number of pixels inside the image (never 0: an unconverged pixel is one of them)
    if (lane_id() == 0u) flags[w] = mk != 0ull ? (uint32_t)__popcll(in_image) : 0u;
}

// Ordered compaction of k_tile_select's flags: out = the flagged entries of prev (null: their own indices) in their order,
// count[0] = how many, count[1] = the sum of their flags (the pixels of the active tiles inside the image).  ONE block walks the flags 1024 at a time (a 4K film has 130 k tiles: 127 trips), so the order needs no
// second pass: ranks within a trip from wave ballots and a scan of the 16 wave totals, the running total carried in a register.
__global__ void __launch_bounds__(1024) k_tile_compact(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ prev,
                                                       uint32_t n_in, uint32_t* __restrict__ out, uint32_t* __restrict__ count) {
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_pixels;
    if (threadIdx.x == 0u) s_pixels = 0u;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t run = 0u, pixels = 0u;
    for (uint32_t i0 = 0; i0 < n_in; i0 += 1024u) {  // block-uniform trip count
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t flag = i < n_in ? flags[i] : 0u;
        const bool on = flag != 0u;
        pixels += flag;
        const unsigned long long mk = __ballot(on);
        if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(mk);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t nk = s_wave[k];
            if (k < wave) before += nk;
            total += nk;
        }
        if (on) out[run + before + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull))] = prev ? prev[i] : i;
        run += total;
        __syncthreads();  // s_wave is rewritten by the next trip
    }
    __syncthreads();
    if (pixels) atomicAdd(&s_pixels, pixels);  // (integers: the order does not matter)
    __syncthreads();
    if (threadIdx.x == 0u) {
        count[0] = run;
        count[1] = s_pixels;
    }
}


// Un-tile `world` gathered rank payloads (each `stride` float4) into the Film layout
// (m_Accum[3*(y*W+x)+c], m_Weights[y*W+x]; src/core/film.h:54-60).
__global__ void __launch_bounds__(256) k_resolve(const float4* __restrict__ gathered, uint32_t world, uint32_t stride,
                                                 uint32_t W, uint32_t H, float* __restrict__ rgb,
                                                 float* __restrict__ weight) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= W * H) return;
    const uint32_t x = idx % W, y = idx / W;
    const uint32_t tiles_x = (W + 7u) >> 3;
    const uint32_t gt = (y >> 3) * tiles_x + (x >> 3);
    const uint32_t rank = gt % world, lt = gt / world;
    const uint32_t pl = lt * 64u + (y & 7u) * 8u + (x & 7u);
    const float4 f = gathered[(size_t)rank * stride + pl];
    rgb[3 * (size_t)idx + 0] = f.x;
    rgb[3 * (size_t)idx + 1] = f.y;
    rgb[3 * (size_t)idx + 2] = f.z;
    weight[idx] = f.w;
}

// Film::UpdateDisplayGPU (updateDisplayKernel, src/core/film.cu:101-121) with the bounds check the
// reference lacks; one thread per channel.
__global__ void __launch_bounds__(256) k_tonemap(const float* __restrict__ rgb, const float* __restrict__ weight,
                                                 uint32_t n_pix, float exposure, float inv_gamma,
                                                 uint8_t* __restrict__ out) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n_pix * 4u) return;
    const uint32_t p = idx >> 2, c = idx & 3u;
    if (c == 3u) {
        out[idx] = 255;
        return;
    }
    const float w = weight[p];
    float value = 0.0f;
    if (w > 0.0f) {
        const float invW = 1.0f / w;
        value = rgb[3 * (size_t)p + c] * invW;
        value = value * exposure;
        value = value / (1.0f + value);
        value = powf(value, inv_gamma);
    }
    value = __builtin_fmaxf(0.0f, __builtin_fminf(1.0f, value));
    out[idx] = (uint8_t)(value * 255.0f + 0.5f);
}

// ---------------------------------------------------------------------------------------------------------
// Function-level kernels behind prt_camera_rays / prt_closest_hit / prt_scatter (parity tests).
__global__ void k_camera_rays_lens(DevCamera cam, DevLens lens, uint32_t n, const float* __restrict__ px, const float* __restrict__ py,
                                   uint32_t* __restrict__ keys, float* __restrict__ o_out, float* __restrict__ d_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f3 o, d;
    uint32_t rng = keys[i];
    lens_camera_ray(cam, lens, px[i], py[i], rng, o, d);
    keys[i] = rng;
    o_out[3 * (size_t)i + 0] = o.x;
    o_out[3 * (size_t)i + 1] = o.y;
    o_out[3 * (size_t)i + 2] = o.z;
    d_out[3 * (size_t)i + 0] = d.x;
    d_out[3 * (size_t)i + 1] = d.y;
    d_out[3 * (size_t)i + 2] = d.z;
}
// ---------------------------------------------------------------------------------------------------------
__global__ void k_camera_rays(DevCamera cam, uint32_t n, const float* __restrict__ px, const float* __restrict__ py,
                              float* __restrict__ o_out, float* __restrict__ d_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    f3 o, d;
    camera_ray(cam, px[i], py[i], o, d);
    o_out[3 * i + 0] = o.x;
    o_out[3 * i + 1] = o.y;
    o_out[3 * i + 2] = o.z;
    d_out[3 * i + 0] = d.x;
    d_out[3 * i + 1] = d.y;
    d_out[3 * i + 2] = d.z;
}

__global__ void k_pack_rays(uint32_t n, const float* __restrict__ o, const float* __restrict__ d,
                            float4* __restrict__ ro, float4* __restrict__ rd, uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) counts[0] = n;  // front count of the slot it was given
    if (i >= n) return;
    ro[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], __uint_as_float(i));
    rd[i] = make_float4(d[3 * i], d[3 * i + 1], d[3 * i + 2], 0.f);
}

__global__ void k_hit_records(DevScene sc, uint32_t n, const float4* __restrict__ ro, const float4* __restrict__ rd,
                              const uint32_t* __restrict__ hit, PrtHit* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    PrtHit h;
    h.prim = -1;
    h.front_face = 0;
    h.material_id = 0xFFFFFFFFu;
    h.d2 = 3.402823466e+38f;
    h.position[0] = h.position[1] = h.position[2] = 0.f;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.f;
    const uint32_t id = hit[i];
    if (id != HIT_MISS && id != HIT_DEAD) {
        const float4 O = ro[i], D = rd[i];
        WorldHit w;
        if (sc.n_insts)
            world_hit_from_id<true>(sc, id, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), w);
        else
            world_hit_from_id<false>(sc, id, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), w);
        if (w.has) {
            h.prim = w.prim;
            h.front_face = w.front ? 1u : 0u;
            h.material_id = w.material;
            h.d2 = w.d2;
            h.position[0] = w.pos.x;
            h.position[1] = w.pos.y;
            h.position[2] = w.pos.z;
            h.normal[0] = w.normal.x;
            h.normal[1] = w.normal.y;
            h.normal[2] = w.normal.z;
        }
    }
    out[i] = h;
}

// ---- occlusion queries (prt_occluded): occluded[i] = 1 iff tmax[i] > 0 and closest_hit(ray i).d2 < fl32(tmax[i]^2) ----
// The ray buffer as k_pack_rays writes it, plus the seed of every ray's bound: hit = HIT_MISS at hd2 = tmax^2, or
// HIT_DEAD for a ray that can never be occluded (tmax <= 0 or NaN, zero direction).
__global__ void k_pack_occlusion_rays(uint32_t n, const float* __restrict__ o, const float* __restrict__ d,
                                      const float* __restrict__ tmax, float4* __restrict__ ro, float4* __restrict__ rd,
                                      uint32_t* __restrict__ hit, float* __restrict__ hd2, uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) counts[0] = n;
    if (i >= n) return;
    const float dx = d[3 * i], dy = d[3 * i + 1], dz = d[3 * i + 2];
    const float t = tmax[i];
    ro[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], __uint_as_float(i));
    rd[i] = make_float4(dx, dy, dz, 0.f);
    const bool dead = !(t > 0.0f) || (dx == 0.0f && dy == 0.0f && dz == 0.0f);
    hit[i] = dead ? HIT_DEAD : HIT_MISS;
    hd2[i] = t * t;
}

// k_scan_prims from the seeded bound instead of FLT_MAX: an analytic hit below tmax makes the ray's answer final before
// traversal.  Strict < in the linear scan, and the primitive walk's tie rule lets an equal d2 win over a hit only, never
// over the seeded miss: a primitive at exactly d2 == tmax^2 does not block.
__global__ void __launch_bounds__(256) k_scan_prims_bounded(DevScene sc, const float4* __restrict__ ro,
                                                            const float4* __restrict__ rd, uint32_t* __restrict__ hit,
                                                            float* __restrict__ hd2, const uint32_t* __restrict__ count_ptr,
                                                            uint32_t* __restrict__ work) {
    const uint32_t count = *count_ptr;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < 8u) work[32u * k] = 0u;  // chunk cursors of the traversal kernel that follows (as k_scan_prims)
    if (k == 8u) work[512] = 0u;     // its overflow-list counter
    if (k >= count) return;
    if (hit[k] == HIT_DEAD) return;
    const float4 O = ro[k];
    const float4 D = rd[k];
    const float t2 = hd2[k];
    Closest best;
    best.d2 = t2;
    best.id = HIT_MISS;
    best.prim = 0xFFFFFFFFu;
    uint32_t n_ptests = 0;
    if (sc.abvh_nodes)
        scan_analytic<true, 256>(sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), best, n_ptests);
    else
        scan_analytic<false>(sc, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), best, n_ptests);
    if (!(best.d2 < t2)) {  // (the primitive walk's stack fallback restarts from FLT_MAX: keep only blockers)
        best.id = HIT_MISS;
        best.d2 = t2;
    }
    hit[k] = best.id;
    hd2[k] = best.d2;
}

// One byte per ray from the final hit id.  The blocker's world distance^2 is rebuilt by world_hit_from_id, the arithmetic
// the walks accept on, and compared with tmax^2 again: exact whichever pipeline produced the id (any-hit walk, or the
// closest-hit fallbacks, whose result is the closest hit below the bound, or the closest hit outright).
__global__ void k_occlusion_bytes(DevScene sc, uint32_t n, const float4* __restrict__ ro, const float4* __restrict__ rd,
                                  const uint32_t* __restrict__ hit, const float* __restrict__ tmax, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float t = tmax[i];
    const uint32_t id = hit[i];
    uint8_t occ = 0u;
    if (t > 0.0f && id != HIT_MISS && id != HIT_DEAD) {
        const float4 O = ro[i], D = rd[i];
        WorldHit w;
        if (sc.n_insts)
            world_hit_from_id<true>(sc, id, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), w);
        else
            world_hit_from_id<false>(sc, id, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), w);
        occ = (w.has && w.d2 < t * t) ? 1u : 0u;
    }
    out[i] = occ;
}

__global__ void k_scatter_test(DevScene sc, uint32_t n, const float* __restrict__ in_d, const PrtHit* __restrict__ hits,
                               uint32_t* __restrict__ rng_io, uint32_t* __restrict__ scattered,
                               float* __restrict__ atten_o, float* __restrict__ emit_o, float* __restrict__ o_out,
                               float* __restrict__ d_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const PrtHit h = hits[i];
    uint32_t rng = rng_io[i];
    f3 atten, emitted, so, sd;
    const uint32_t m = h.material_id;
    const bool sc_ = material_scatter(sc.mat_type[m], sc.mat_rgbs[m], mk3(in_d[3 * i], in_d[3 * i + 1], in_d[3 * i + 2]),
                                      mk3(h.position[0], h.position[1], h.position[2]),
                                      mk3(h.normal[0], h.normal[1], h.normal[2]), h.front_face != 0u, rng, atten,
                                      emitted, so, sd);
    rng_io[i] = rng;
    scattered[i] = sc_ ? 1u : 0u;
    atten_o[3 * i + 0] = atten.x;
    atten_o[3 * i + 1] = atten.y;
    atten_o[3 * i + 2] = atten.z;
    emit_o[3 * i + 0] = emitted.x;
    emit_o[3 * i + 1] = emitted.y;
    emit_o[3 * i + 2] = emitted.z;
    o_out[3 * i + 0] = so.x;
    o_out[3 * i + 1] = so.y;
    o_out[3 * i + 2] = so.z;
    d_out[3 * i + 0] = sd.x;
    d_out[3 * i + 1] = sd.y;
    d_out[3 * i + 2] = sd.z;
}

// ---------------------------------------------------------------------------------------------------------
// Light sampling (PrtLighting, include/prt.h; DESIGN.md §3 "Light sampling"): next-event estimation toward the analytic
// emitters of the light table (DevLights), combined with the scattered path by multiple importance sampling.  Per bounce:
// k_shade_nee (k_shade's step plus one light sample per Lambertian vertex that scatters; the sample becomes a shadow ray)
// -> k_scan_prims_bounded + the any-hit walk over the shadow rays (prt_occluded's pipeline) -> k_light_accum.
// ---------------------------------------------------------------------------------------------------------
#include "prt_light_device.h"  // sphere_cone_omc .. env_miss

// advance_path<1, INST, ABVH, SHADE_BLOCK> (no fused segment) with light sampling: the same vertex, the same draws, the same
// segments; in addition the light sample (`shadow`) of a Lambertian vertex that scatters, emission of light-set emitters
// met after a Lambertian vertex weighted by bsdf_hit_weight, and pb_next = the pdf of the scatter (-1: not Lambertian).
// MESHL (ml: the triangle lights' tables): the light set holds triangles too, so a segment's triangle hit is weighted as well.
// ENV (env: DevEnv): an environment light: a miss delivers its texel, weighted after a Lambertian vertex (env_miss), and a
// Lambertian vertex whose environment-or-lights draw says so sends its light sample there (sample_environment).
// TEX (tex: DevTex): the albedo (attenuation and light-sample term) of a textured vertex is the lookup at the hit's UV.
// CLUS (lc: DevLightClusters; implies MESHL): clustered light selection in the light sample and in the weight of a hit light.
template <bool INST, bool ABVH, bool MESHL = false, bool ENV = false, bool TEX = false, bool CLUS = false>
PRT_DEV int advance_path_nee(const DevScene& sc, const DevLights& lt, uint32_t id, f3& o, f3& d, f3& thr, uint32_t& rng,
                             uint32_t& depth, uint32_t max_depth, const PrtSampling& sp, float4* __restrict__ rad_slot,
                             uint32_t& id0, float& d2_0, float pb_prev, float& pb_next, bool& shadow, f3& sx, f3& sw,
                             float& stmax, f3& scontrib, const DevMeshLights* ml = nullptr, const DevEnv* env = nullptr,
                             const DevTex* tex = nullptr, const DevLightClusters* lc = nullptr) {
    if (id == HIT_MISS) {
        if (ENV) {
            float wb;
            f3 L = thr * env_miss(*env, lt.mode, d, pb_prev, wb);
            if (wb != 1.0f) L = L * wb;
            st_stream(rad_slot, path_result(L, sp.clamp, depth));
            return 0;
        }
        st_stream(rad_slot, path_result(thr * mk3(sc.sky[0], sc.sky[1], sc.sky[2]), sp.clamp, depth));
        return 0;
    }
    WorldHit w;
    float uv[2] = {0.0f, 0.0f};
    if (TEX)
        world_hit_from_id<INST, true>(sc, id, o, d, w, tex, uv);
    else
        world_hit_from_id<INST>(sc, id, o, d, w);
    const uint32_t type = sc.mat_type[w.material];
    const float4 rgbs = TEX ? textured_rgbs(sc, *tex, w.material, uv) : sc.mat_rgbs[w.material];
    const uint32_t key = rng;  // the path's state at the vertex
    f3 atten, emitted, so, sd;
    bool scattered = false;
    if (depth + 1u >= max_depth) {
        emitted = (type == 4u) ? mk3(rgbs.x, rgbs.y, rgbs.z) : mk3(0.f, 0.f, 0.f);
    } else {
        scattered = material_scatter(type, rgbs, d, w.pos, w.normal, w.front, rng, atten, emitted, so, sd);
    }
    if (!scattered) {
        f3 L = thr * emitted;
        if (type == 4u && (MESHL || id < sc.n_prims) && pb_prev >= 0.0f) {
            const float wb = MESHL ? bsdf_hit_weight<MESHL, CLUS>(lt, (uint32_t)w.prim, o, d, w.d2, pb_prev, ml, sc.n_prims, lc)
                                   : bsdf_hit_weight(lt, id, o, d, w.d2, pb_prev);
            if (wb != 1.0f) L = L * wb;
        }
        st_stream(rad_slot, path_result(L, sp.clamp, depth));
        return 0;
    }
    if (ENV && type == 1u && (env->t_all | env->t_env) != 0u && env_selected(*env, key)) {
        LightSample ls;
        float pb, wl;
        if (env_sample_term(*env, lt.mode, w.normal, mk3(rgbs.x, rgbs.y, rgbs.z), thr, key, sp.clamp, ls, pb, wl, scontrib) && pb > 0.0f) {
            shadow = true;
            sw = ls.w;
            stmax = ls.tmax;
        }
    } else if (type == 1u && lt.n_lights) {  // (scattered: depth + 1 < max_depth)
        LightSample ls;
        float pb, wl;
        if (light_sample_term<MESHL, CLUS>(lt, w.pos, w.normal, mk3(rgbs.x, rgbs.y, rgbs.z), thr, key, sp.clamp, ls, pb, wl, scontrib, ml, lc) &&
            pb > 0.0f) {
            shadow = true;
            sw = ls.w;
            stmax = ls.tmax;
        }
    }
    sx = w.pos;
    thr = thr * atten;
    o = so;
    d = normalize3(sd);
    if (type == 1u) {
        const float c = dot3(w.normal, d);
        pb_next = (c > 0.0f ? c : 0.0f) * PRT_INV_PI;
    }
    if (sp.rr_depth != 0u && depth + 1u >= sp.rr_depth) {
        float p = thr.x > thr.y ? thr.x : thr.y;
        p = p > thr.z ? p : thr.z;
        p = p > 1.0f ? 1.0f : p;
        p = p < 0.05f ? 0.05f : p;
        if (!(rnd01(rng) < p)) {
            st_stream(rad_slot, path_result(mk3(0.f, 0.f, 0.f), 0.0f, depth));
            return 0;
        }
        thr = mk3(thr.x / p, thr.y / p, thr.z / p);
    }
    ++depth;
    if (classify_ray<ABVH, SHADE_BLOCK>(sc, o, d, id0, d2_0)) return 1;
    // the new segment cannot hit a triangle: its closest hit is the analytic scan's (advance_path's budget step)
    if (id0 == HIT_MISS) {
        if (ENV) {
            float wb;
            f3 L = thr * env_miss(*env, lt.mode, d, pb_next, wb);
            if (wb != 1.0f) L = L * wb;
            st_stream(rad_slot, path_result(L, sp.clamp, depth));
            return 0;
        }
        st_stream(rad_slot, path_result(thr * mk3(sc.sky[0], sc.sky[1], sc.sky[2]), sp.clamp, depth));
        return 0;
    }
    const uint32_t m = sc.prims[id0].material;
    if (sc.mat_type[m] == 4u) {
        const float4 e = sc.mat_rgbs[m];
        f3 L = thr * mk3(e.x, e.y, e.z);
        if (pb_next >= 0.0f) {
            const float wb = bsdf_hit_weight<MESHL, CLUS>(lt, id0, o, d, d2_0, pb_next, ml, sc.n_prims, lc);  // (id0: an analytic hit of the scan)
            if (wb != 1.0f) L = L * wb;
        }
        st_stream(rad_slot, path_result(L, sp.clamp, depth));
        return 0;
    }
    return 2;
}

// The lighting shade step; MESHL / ml: see advance_path_nee (k_shade_nee passes false / null and compiles to the code it had
// before there were triangle lights; k_shade_nee_mesh is the instance with them).
template <bool INST, bool ABVH, bool MESHL, bool ENV = false, bool TEX = false, bool CLUS = false>
PRT_DEV void shade_nee_step(DevScene sc, DevLights lt, const DevMeshLights* ml, const float4* __restrict__ ro,
                            const float4* __restrict__ rd, const float4* __restrict__ rt, const uint32_t* __restrict__ hit,
                            float4* __restrict__ no, float4* __restrict__ nd, float4* __restrict__ nt, uint32_t* __restrict__ nhit,
                            float* __restrict__ nhd2, PrtLightBufs lb, float4* __restrict__ rad, uint32_t* __restrict__ counts,
                            uint32_t* __restrict__ work, uint32_t iter, uint32_t max_depth, uint32_t cap, PrtSampling sp,
                            const DevEnv* env = nullptr, const DevTex* tex = nullptr, const DevLightClusters* lc = nullptr) {
    const uint32_t nA = CNT_A(counts, iter), nB = CNT_B(counts, iter);
    const uint32_t count = nA + nB;
    if (blockIdx.x * (uint32_t)SHADE_BLOCK >= count) return;  // whole block exits together
    const uint32_t k = blockIdx.x * (uint32_t)SHADE_BLOCK + threadIdx.x;
    if (k < 8u) work[32u * k] = 0u;  // chunk cursors of the shadow walk / the next bounce's traversal
    if (k == 8u) work[512] = 0u;
    bool front = false, back = false, shadow = false;
    f3 o = mk3(0.f, 0.f, 0.f), d = mk3(0.f, 0.f, 1.f), thr = mk3(0.f, 0.f, 0.f);
    f3 sx = o, sw = d, sc_rgb = o;
    float stmax = 0.0f, pb_next = -1.0f;
    uint32_t id0 = HIT_MISS, rng = 0, depth = 0, pid = 0;
    float d2_0 = 3.402823466e+38f;
    if (k < count) {
        const uint32_t src = k < nA ? k : cap - 1u - (k - nA);
        const uint32_t id = ld_stream(&hit[src]);
        const float4 O = ld_stream(&ro[src]);
        const float4 D = ld_stream(&rd[src]);
        const float4 T = ld_stream(&rt[src]);
        pid = __float_as_uint(O.w);
        rng = __float_as_uint(D.w);
        depth = __float_as_uint(T.w);
        thr = mk3(T.x, T.y, T.z);
        o = mk3(O.x, O.y, O.z);
        d = mk3(D.x, D.y, D.z);
        // pdf of the scatter that started this segment (segment 0 starts at the camera)
        const float pb_prev = depth ? lb.pdf_b[pid] : -1.0f;
        if (id != HIT_DEAD) {
            const int r = advance_path_nee<INST, ABVH, MESHL, ENV, TEX, CLUS>(sc, lt, id, o, d, thr, rng, depth, max_depth, sp, &rad[pid], id0, d2_0,
                                                            pb_prev, pb_next, shadow, sx, sw, stmax, sc_rgb, ml, env, tex, lc);
            front = r == 1;
            back = r == 2;
        }
    }
    const uint32_t slot = block_alloc2<SHADE_BLOCK>(front, back, false, &CNT_A(counts, iter + 1u), &CNT_B(counts, iter + 1u),
                                                    &CNT_C(counts, iter + 1u), cap);
    if (slot != 0xFFFFFFFFu) {
        st_stream(&no[slot], make_float4(o.x, o.y, o.z, __uint_as_float(pid)));
        st_stream(&nd[slot], make_float4(d.x, d.y, d.z, __uint_as_float(rng)));
        st_stream(&nt[slot], make_float4(thr.x, thr.y, thr.z, __uint_as_float(depth)));
        st_stream(&nhit[slot], id0);
        st_stream(&nhd2[slot], d2_0);
        lb.pdf_b[pid] = pb_next;  // (one writer per path; read by the path's next k_shade_nee)
    }
    __syncthreads();  // block_alloc2's LDS counts are reused below (see its contract)
    uint32_t* cs = &counts[iter * CNT_STRIDE + 48u];
    const uint32_t ss = block_alloc2<SHADE_BLOCK>(shadow, false, false, cs, cs, cs, cap);
    if (ss != 0xFFFFFFFFu) {  // seeded as k_pack_occlusion_rays seeds a ray: a miss at hd2 = tmax^2
        lb.sh.o[ss] = make_float4(sx.x, sx.y, sx.z, __uint_as_float(pid));
        lb.sh.d[ss] = make_float4(sw.x, sw.y, sw.z, 0.0f);
        lb.sh.t[ss] = make_float4(sc_rgb.x, sc_rgb.y, sc_rgb.z, stmax);
        lb.sh.hit[ss] = HIT_MISS;
        lb.sh.hd2[ss] = stmax * stmax;
    }
}

template <bool INST, bool ABVH>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_nee(DevScene sc, DevLights lt, const float4* __restrict__ ro,
                                                          const float4* __restrict__ rd, const float4* __restrict__ rt,
                                                          const uint32_t* __restrict__ hit, float4* __restrict__ no,
                                                          float4* __restrict__ nd, float4* __restrict__ nt,
                                                          uint32_t* __restrict__ nhit, float* __restrict__ nhd2,
                                                          PrtLightBufs lb, float4* __restrict__ rad, uint32_t* __restrict__ counts,
                                                          uint32_t* __restrict__ work, uint32_t iter, uint32_t max_depth,
                                                          uint32_t cap, PrtSampling sp) {
    shade_nee_step<INST, ABVH, false>(sc, lt, nullptr, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, lb, rad, counts, work, iter, max_depth, cap, sp);
}

// k_shade_nee with triangle lights in the light set (prt_set_light_sources with PRT_LIGHT_SOURCES_MESH)
template <bool INST, bool ABVH>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_nee_mesh(DevScene sc, DevLights lt, DevMeshLights ml, const float4* __restrict__ ro,
                                                               const float4* __restrict__ rd, const float4* __restrict__ rt,
                                                               const uint32_t* __restrict__ hit, float4* __restrict__ no,
                                                               float4* __restrict__ nd, float4* __restrict__ nt,
                                                               uint32_t* __restrict__ nhit, float* __restrict__ nhd2,
                                                               PrtLightBufs lb, float4* __restrict__ rad, uint32_t* __restrict__ counts,
                                                               uint32_t* __restrict__ work, uint32_t iter, uint32_t max_depth,
                                                               uint32_t cap, PrtSampling sp) {
    shade_nee_step<INST, ABVH, true>(sc, lt, &ml, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, lb, rad, counts, work, iter, max_depth, cap, sp);
}

// k_shade_nee / k_shade_nee_mesh with an environment light (prt_set_environment)
template <bool INST, bool ABVH>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_nee_env(DevScene sc, DevLights lt, DevEnv env, const float4* __restrict__ ro,
                                                              const float4* __restrict__ rd, const float4* __restrict__ rt,
                                                              const uint32_t* __restrict__ hit, float4* __restrict__ no,
                                                              float4* __restrict__ nd, float4* __restrict__ nt,
                                                              uint32_t* __restrict__ nhit, float* __restrict__ nhd2,
                                                              PrtLightBufs lb, float4* __restrict__ rad, uint32_t* __restrict__ counts,
                                                              uint32_t* __restrict__ work, uint32_t iter, uint32_t max_depth,
                                                              uint32_t cap, PrtSampling sp) {
    shade_nee_step<INST, ABVH, false, true>(sc, lt, nullptr, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, lb, rad, counts, work, iter, max_depth, cap, sp, &env);
}

template <bool INST, bool ABVH>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_nee_mesh_env(DevScene sc, DevLights lt, DevMeshLights ml, DevEnv env,
                                                                   const float4* __restrict__ ro, const float4* __restrict__ rd,
                                                                   const float4* __restrict__ rt, const uint32_t* __restrict__ hit,
                                                                   float4* __restrict__ no, float4* __restrict__ nd,
                                                                   float4* __restrict__ nt, uint32_t* __restrict__ nhit,
                                                                   float* __restrict__ nhd2, PrtLightBufs lb, float4* __restrict__ rad,
                                                                   uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                                   uint32_t iter, uint32_t max_depth, uint32_t cap, PrtSampling sp) {
    shade_nee_step<INST, ABVH, true, true>(sc, lt, &ml, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, lb, rad, counts, work, iter, max_depth, cap, sp, &env);
}

// The lighting shade step under a texture binding: every combination of triangle lights (MESHL) and environment light
// (ENV) in one kernel template; `ml` / `env` are read only by the instances that have them
template <bool INST, bool ABVH, bool MESHL, bool ENV>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_nee_tex(DevScene sc, DevTex tex, DevLights lt, DevMeshLights ml, DevEnv env,
                                                              const float4* __restrict__ ro, const float4* __restrict__ rd,
                                                              const float4* __restrict__ rt, const uint32_t* __restrict__ hit,
                                                              float4* __restrict__ no, float4* __restrict__ nd,
                                                              float4* __restrict__ nt, uint32_t* __restrict__ nhit,
                                                              float* __restrict__ nhd2, PrtLightBufs lb, float4* __restrict__ rad,
                                                              uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                              uint32_t iter, uint32_t max_depth, uint32_t cap, PrtSampling sp) {
    shade_nee_step<INST, ABVH, MESHL, ENV, true>(sc, lt, MESHL ? &ml : nullptr, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, lb, rad, counts, work,
                                                 iter, max_depth, cap, sp, ENV ? &env : nullptr, &tex);
}

// The lighting shade step under clustered light selection (prt_set_light_selection; triangle lights are in the light set):
// k_shade_nee_mesh / k_shade_nee_mesh_env / the mesh-light half of k_shade_nee_tex with the cluster tables
template <bool INST, bool ABVH>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_nee_clus(DevScene sc, DevLights lt, DevMeshLights ml, DevLightClusters lc,
                                                               const float4* __restrict__ ro, const float4* __restrict__ rd,
                                                               const float4* __restrict__ rt, const uint32_t* __restrict__ hit,
                                                               float4* __restrict__ no, float4* __restrict__ nd,
                                                               float4* __restrict__ nt, uint32_t* __restrict__ nhit,
                                                               float* __restrict__ nhd2, PrtLightBufs lb, float4* __restrict__ rad,
                                                               uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                               uint32_t iter, uint32_t max_depth, uint32_t cap, PrtSampling sp) {
    shade_nee_step<INST, ABVH, true, false, false, true>(sc, lt, &ml, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, lb, rad, counts, work, iter,
                                                         max_depth, cap, sp, nullptr, nullptr, &lc);
}

template <bool INST, bool ABVH>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_nee_clus_env(DevScene sc, DevLights lt, DevMeshLights ml, DevLightClusters lc, DevEnv env,
                                                                   const float4* __restrict__ ro, const float4* __restrict__ rd,
                                                                   const float4* __restrict__ rt, const uint32_t* __restrict__ hit,
                                                                   float4* __restrict__ no, float4* __restrict__ nd,
                                                                   float4* __restrict__ nt, uint32_t* __restrict__ nhit,
                                                                   float* __restrict__ nhd2, PrtLightBufs lb, float4* __restrict__ rad,
                                                                   uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                                   uint32_t iter, uint32_t max_depth, uint32_t cap, PrtSampling sp) {
    shade_nee_step<INST, ABVH, true, true, false, true>(sc, lt, &ml, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, lb, rad, counts, work, iter,
                                                        max_depth, cap, sp, &env, nullptr, &lc);
}

template <bool INST, bool ABVH, bool ENV>
__global__ void __launch_bounds__(SHADE_BLOCK) k_shade_nee_clus_tex(DevScene sc, DevTex tex, DevLights lt, DevMeshLights ml, DevLightClusters lc,
                                                                   DevEnv env, const float4* __restrict__ ro, const float4* __restrict__ rd,
                                                                   const float4* __restrict__ rt, const uint32_t* __restrict__ hit,
                                                                   float4* __restrict__ no, float4* __restrict__ nd,
                                                                   float4* __restrict__ nt, uint32_t* __restrict__ nhit,
                                                                   float* __restrict__ nhd2, PrtLightBufs lb, float4* __restrict__ rad,
                                                                   uint32_t* __restrict__ counts, uint32_t* __restrict__ work,
                                                                   uint32_t iter, uint32_t max_depth, uint32_t cap, PrtSampling sp) {
    shade_nee_step<INST, ABVH, true, ENV, true, true>(sc, lt, &ml, ro, rd, rt, hit, no, nd, nt, nhit, nhd2, lb, rad, counts, work, iter,
                                                      max_depth, cap, sp, ENV ? &env : nullptr, &tex, &lc);
}

// prt_texture_eval: texture_lookup for n (texture, uv) pairs (the host checked the texture indices)
__global__ void k_texture_eval(DevTex tex, uint32_t n, const uint32_t* __restrict__ texture, const float* __restrict__ uv,
                               float* __restrict__ rgb) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const f3 c = texture_lookup(tex, texture[i], uv[2 * i], uv[2 * i + 1]);
    rgb[3 * i + 0] = c.x;
    rgb[3 * i + 1] = c.y;
    rgb[3 * i + 2] = c.z;
}

// prt_hit_uv: the TEX hit reconstruction of the shade kernels for the rays of a finished closest-hit query
__global__ void k_hit_uv(DevScene sc, DevTex tex, uint32_t n, const float4* __restrict__ ro, const float4* __restrict__ rd,
                         const uint32_t* __restrict__ hit, float* __restrict__ uv_out, float* __restrict__ albedo) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float uv[2] = {0.0f, 0.0f};
    f3 a = mk3(0.0f, 0.0f, 0.0f);
    const uint32_t id = hit[i];
    if (id != HIT_MISS && id != HIT_DEAD) {
        const float4 O = ro[i], D = rd[i];
        WorldHit w;
        if (sc.n_insts)
            world_hit_from_id<true, true>(sc, id, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), w, &tex, uv);
        else
            world_hit_from_id<false, true>(sc, id, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), w, &tex, uv);
        if (w.has) {
            const float4 rgbs = textured_rgbs(sc, tex, w.material, uv);
            a = mk3(rgbs.x, rgbs.y, rgbs.z);
        } else {
            uv[0] = uv[1] = 0.0f;
        }
    }
    if (uv_out) {
        uv_out[2 * i + 0] = uv[0];
        uv_out[2 * i + 1] = uv[1];
    }
    if (albedo) {
        albedo[3 * i + 0] = a.x;
        albedo[3 * i + 1] = a.y;
        albedo[3 * i + 2] = a.z;
    }
}

// After the shadow walk: every unoccluded shadow ray adds its contribution to its path's light radiance (at most one shadow
// ray per path per bounce: no atomics; the sum runs in vertex order).  The blocker test is k_occlusion_bytes': exact
// whichever walk produced the id.  Also resets the traversal cursors for the next bounce and counts the rays.
__global__ void __launch_bounds__(256) k_light_accum(DevScene sc, PrtLightBufs lb, const uint32_t* __restrict__ count_ptr,
                                                     uint32_t* __restrict__ work) {
    __shared__ uint32_t s_n[2];
    const uint32_t count = *count_ptr;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < 8u) work[32u * k] = 0u;
    if (k == 8u) work[512] = 0u;
    if (blockIdx.x * 256u >= count) return;  // whole block exits together
    if (threadIdx.x < 2u) s_n[threadIdx.x] = 0u;
    __syncthreads();
    bool occ = false;
    if (k < count) {
        const uint32_t id = lb.sh.hit[k];
        const float4 O = lb.sh.o[k];
        const float4 T = lb.sh.t[k];
        if (id != HIT_MISS && id != HIT_DEAD) {
            const float4 D = lb.sh.d[k];
            WorldHit w;
            if (sc.n_insts)
                world_hit_from_id<true>(sc, id, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), w);
            else
                world_hit_from_id<false>(sc, id, mk3(O.x, O.y, O.z), mk3(D.x, D.y, D.z), w);
            occ = w.has && w.d2 < T.w * T.w;
        }
        if (!occ) {
            float4* p = &lb.lrad[__float_as_uint(O.w)];
            float4 a = *p;
            a.x = a.x + T.x;
            a.y = a.y + T.y;
            a.z = a.z + T.z;
            *p = a;
        }
    }
    const unsigned long long mn = __ballot(k < count), mo = __ballot(occ);
    if (lane_id() == 0u) {
        atomicAdd(&s_n[0], (uint32_t)__popcll(mn));
        atomicAdd(&s_n[1], (uint32_t)__popcll(mo));
    }
    __syncthreads();
    // (PRT_RAY_STAT_SLOTS copies of the two counters, block b adds to copy b mod SLOTS, summed by the host: one word executes
    // only ~87 atomics per microsecond, as for k_accumulate's ray counters)
    if (threadIdx.x < 2u && s_n[threadIdx.x])
        atomicAdd(&lb.stats[2u * (blockIdx.x & (PRT_RAY_STAT_SLOTS - 1u)) + threadIdx.x], (unsigned long long)s_n[threadIdx.x]);
}

// prt_sample_light: one light sample per (hit, key) through the render's own light_sample_term (throughput 1, no clamp) and,
// for the same pair of vertices, the weight bsdf_hit_weight gives a scattered segment in direction w that meets the light;
// out 11 floats per ray: w.xyz, tmax, contrib.rgb, pdf_light, pdf_bsdf, w_light, w_bsdf
template <bool MESHL, bool ENV = false, bool CLUS = false>
PRT_DEV void sample_light_test(DevScene sc, DevLights lt, const DevMeshLights* ml, uint32_t n, const float* __restrict__ in_d,
                               const PrtHit* __restrict__ hits, const uint32_t* __restrict__ keys, float* __restrict__ out,
                               uint32_t* __restrict__ out_light, const DevEnv* env = nullptr, const DevLightClusters* lc = nullptr) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const PrtHit h = hits[i];
    float r[11] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t light = 0xFFFFFFFFu;
    if (ENV && h.prim >= 0 && sc.mat_type[h.material_id] == 1u && (env->t_all | env->t_env) != 0u && env_selected(*env, keys[i])) {
        const float4 a = sc.mat_rgbs[h.material_id];
        LightSample s;
        float pb = 0.0f, wl = 0.0f, wb = 1.0f;
        f3 C;
        if (env_sample_term(*env, lt.mode, mk3(h.normal[0], h.normal[1], h.normal[2]), mk3(a.x, a.y, a.z), mk3(1.f, 1.f, 1.f), keys[i], 0.0f,
                            s, pb, wl, C)) {
            light = s.light;
            (void)env_miss(*env, lt.mode, s.w, pb, wb);
            const float vals[11] = {s.w.x, s.w.y, s.w.z, s.tmax, C.x, C.y, C.z, s.pdf_l, pb, wl, wb};
            for (int j = 0; j < 11; ++j) r[j] = vals[j];
        }
    } else if (h.prim >= 0 && sc.mat_type[h.material_id] == 1u && lt.n_lights) {
        const float4 a = sc.mat_rgbs[h.material_id];
        const f3 x = mk3(h.position[0], h.position[1], h.position[2]);
        LightSample s;
        float pb = 0.0f, wl = 0.0f;
        f3 C;
        if (light_sample_term<MESHL, CLUS>(lt, x, mk3(h.normal[0], h.normal[1], h.normal[2]), mk3(a.x, a.y, a.z), mk3(1.f, 1.f, 1.f), keys[i],
                                           0.0f, s, pb, wl, C, ml, lc)) {
            light = s.light;
            const uint32_t prim = __float_as_uint(lt.lights[PRT_LIGHT_F4 * s.light + 4u].w);
            const float vals[11] = {s.w.x, s.w.y, s.w.z, s.tmax, C.x, C.y, C.z, s.pdf_l, pb, wl,
                                    bsdf_hit_weight<MESHL, CLUS>(lt, prim, x, s.w, s.t_light * s.t_light, pb, ml, sc.n_prims, lc)};
            for (int j = 0; j < 11; ++j) r[j] = vals[j];
        }
    }
    for (int j = 0; j < 11; ++j) out[11 * (size_t)i + j] = r[j];
    out_light[i] = light;
}

__global__ void k_sample_light_test(DevScene sc, DevLights lt, uint32_t n, const float* __restrict__ in_d,
                                    const PrtHit* __restrict__ hits, const uint32_t* __restrict__ keys, float* __restrict__ out,
                                    uint32_t* __restrict__ out_light) {
    sample_light_test<false>(sc, lt, nullptr, n, in_d, hits, keys, out, out_light);
}

// (the `light` it reports is the candidate; prt_sample_light maps it to the light set)
__global__ void k_sample_light_test_mesh(DevScene sc, DevLights lt, DevMeshLights ml, uint32_t n, const float* __restrict__ in_d,
                                         const PrtHit* __restrict__ hits, const uint32_t* __restrict__ keys, float* __restrict__ out,
                                         uint32_t* __restrict__ out_light) {
    sample_light_test<true>(sc, lt, &ml, n, in_d, hits, keys, out, out_light);
}

__global__ void k_sample_light_test_env(DevScene sc, DevLights lt, DevEnv env, uint32_t n, const float* __restrict__ in_d,
                                        const PrtHit* __restrict__ hits, const uint32_t* __restrict__ keys, float* __restrict__ out,
                                        uint32_t* __restrict__ out_light) {
    sample_light_test<false, true>(sc, lt, nullptr, n, in_d, hits, keys, out, out_light, &env);
}

__global__ void k_sample_light_test_mesh_env(DevScene sc, DevLights lt, DevMeshLights ml, DevEnv env, uint32_t n,
                                             const float* __restrict__ in_d, const PrtHit* __restrict__ hits,
                                             const uint32_t* __restrict__ keys, float* __restrict__ out, uint32_t* __restrict__ out_light) {
    sample_light_test<true, true>(sc, lt, &ml, n, in_d, hits, keys, out, out_light, &env);
}

// prt_sample_light under clustered light selection
__global__ void k_sample_light_test_clus(DevScene sc, DevLights lt, DevMeshLights ml, DevLightClusters lc, uint32_t n,
                                         const float* __restrict__ in_d, const PrtHit* __restrict__ hits,
                                         const uint32_t* __restrict__ keys, float* __restrict__ out, uint32_t* __restrict__ out_light) {
    sample_light_test<true, false, true>(sc, lt, &ml, n, in_d, hits, keys, out, out_light, nullptr, &lc);
}

__global__ void k_sample_light_test_clus_env(DevScene sc, DevLights lt, DevMeshLights ml, DevLightClusters lc, DevEnv env, uint32_t n,
                                             const float* __restrict__ in_d, const PrtHit* __restrict__ hits,
                                             const uint32_t* __restrict__ keys, float* __restrict__ out, uint32_t* __restrict__ out_light) {
    sample_light_test<true, true, true>(sc, lt, &ml, n, in_d, hits, keys, out, out_light, &env, &lc);
}

// prt_light_cluster_pmf: the thresholds M_c of n points through cluster_thresholds, M[i * n_clusters + c]
__global__ void k_light_cluster_pmf(DevLightClusters lc, uint32_t n, const float* __restrict__ x, uint32_t* __restrict__ M) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t* row = M + (size_t)i * lc.n_clusters;
    cluster_thresholds(lc, mk3(x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2]),
                       [&](uint32_t c, uint32_t, uint32_t mc) { row[c] = mc; });
}

// prt_environment_eval: the render's own lookup (env_radiance) per direction
__global__ void k_environment_eval(DevEnv env, uint32_t n, const float* __restrict__ dirs, float* __restrict__ rgb,
                                   uint32_t* __restrict__ texel, float* __restrict__ pdf_w) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const f3 d = mk3(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
    float pw;
    const f3 le = env_radiance(env, d, pw);
    if (rgb) {
        rgb[3 * (size_t)i + 0] = le.x;
        rgb[3 * (size_t)i + 1] = le.y;
        rgb[3 * (size_t)i + 2] = le.z;
    }
    if (texel) texel[i] = env_texel(env, d);
    if (pdf_w) pdf_w[i] = pw;
}

// ---------------------------------------------------------------------------------------------------------
// Host launchers (plain functions; prt_api.cpp has no kernel syntax).
// ---------------------------------------------------------------------------------------------------------
static inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// An optional argument that a kernel takes by value: the caller's, or an empty one for the instances that never read it.
template <class T>
static const T& or_empty(const T* p) {
    static const T none{};
    return p ? *p : none;
}

// The three stage launchers of a batch: `inst` is the instance prt_plan_route (prt_route.h) chose, the `case`s are that
// header's instance lists, so an instance's name and its launch are one spelling.  false: no such instance.
bool prt_launch_raygen(hipStream_t st, PrtRaygenInst inst, const PrtRaygenArgs& a) {
    const uint32_t S = a.tm.n_pix_local ? a.n_paths / a.tm.n_pix_local : 0u;
    const uint32_t group = (a.sp.jitter || a.lens) ? (uint32_t)RAYGEN_GROUP : RAYGEN_GROUP_NOJITTER;
    const dim3 grid((a.tm.n_pix_local + PRODUCER_BLOCK - 1) / PRODUCER_BLOCK, (S + group - 1) / group);
    const DevScene& sc = *a.sc;
    const DevEnv& e = or_empty(a.env);
    const DevLens& l = or_empty(a.lens);
#define PRT_RAYGEN_HEAD a.cam, a.tm, S, a.first_sample, a.seed, a.out.o, a.out.d, a.out.t, a.out.hit
#define PRT_RAYGEN_TAIL a.rad, a.counts, a.work, a.max_depth, a.sp
#define PRT_RAYGEN_ARGS_PLAIN sc, PRT_RAYGEN_HEAD, a.out.hd2, PRT_RAYGEN_TAIL, nullptr, 0u
    // (the compact instance stores nothing in hit / hd2 per ray slot: its hd2 argument is the front-pixel list, or null)
#define PRT_RAYGEN_ARGS_COMPACT sc, PRT_RAYGEN_HEAD, a.primary_walk ? a.out.hd2 : nullptr, PRT_RAYGEN_TAIL, a.compact_pix, a.pixel_major_ids ? 1u : 0u
#define PRT_RAYGEN_ARGS_ENV sc, e, PRT_RAYGEN_HEAD, a.out.hd2, PRT_RAYGEN_TAIL
#define PRT_RAYGEN_ARGS_LENS sc, l, PRT_RAYGEN_HEAD, a.out.hd2, PRT_RAYGEN_TAIL
#define PRT_RAYGEN_ARGS_LENS_ENV sc, e, l, PRT_RAYGEN_HEAD, a.out.hd2, PRT_RAYGEN_TAIL
#define PRT_RAYGEN_ARGS_LIST sc, e, l, a.cam, a.tm, a.list, S, a.first_sample, a.seed, a.out.o, a.out.d, a.out.t, a.out.hit, a.out.hd2, PRT_RAYGEN_TAIL
#define PRT_RAYGEN_CASE(sig, kernel, tag, ...) \
    case PRT_INST(kernel, tag): hipLaunchKernelGGL((kernel<__VA_ARGS__>), grid, dim3(PRODUCER_BLOCK), 0, st, PRT_RAYGEN_ARGS_##sig); return true;
    switch (inst) {
        PRT_RAYGEN_INSTANCES(PRT_RAYGEN_CASE)
        default: return false;
    }
#undef PRT_RAYGEN_CASE
#undef PRT_RAYGEN_ARGS_LIST
#undef PRT_RAYGEN_ARGS_LENS_ENV
#undef PRT_RAYGEN_ARGS_LENS
#undef PRT_RAYGEN_ARGS_ENV
#undef PRT_RAYGEN_ARGS_COMPACT
#undef PRT_RAYGEN_ARGS_PLAIN
#undef PRT_RAYGEN_TAIL
#undef PRT_RAYGEN_HEAD
}

void prt_launch_scan_prims(hipStream_t st, const DevScene& sc, const PrtRayBuf& in, const uint32_t* count_ptr,
                           uint32_t* work, uint32_t max_rays, unsigned long long* stats) {
    hipLaunchKernelGGL(k_scan_prims, dim3(blocks_for(max_rays)), dim3(256), 0, st, sc, in.o, in.d, in.hit, in.hd2,
                       count_ptr, work, stats);
}

// k_fix_cursors: between the fast traversal and its overflow re-run: reset the chunk cursors.
__global__ void k_reset_cursors(uint32_t* work) {
    if (threadIdx.x < 8u) work[32u * threadIdx.x] = 0u;
}

// The tree walk.  Which instances a walk launches, with which grid and tunables, is prt_plan_walk's (prt_walk.h); these only
// follow the plan.  A launch's tunables: the caller's, with what the plan resolved.
static PrtTravTuning walk_tuning(const PrtTravTuning& in, const PrtWalkLaunch& l) {
    PrtTravTuning t = in;
    t.exit_max = l.exit_max, t.tri_min = l.tri_min, t.stack_cap = l.stack_cap, t.steal = l.steal;
    if (!l.keep_perm) t.perm = nullptr;
    return t;
}

// A row of the 8-wide list crossed with the launch's form: the any-hit kernels, or the closest hit with STATS and, on the LEAN
// row only, PRIM (bounce 0 of a batch whose k_raygen stored compact primary rays).
template <int L, int W, bool IN, bool LN>
static void launch_walk8(hipStream_t st, const PrtWalkLaunch& l, const PrtWalkArgs& a, const PrtTravTuning& tune) {
    const dim3 grid(l.grid), block(256);
    const PrtRayBuf& in = a.rays;
    unsigned long long* stats = l.stats ? a.stats : nullptr;
#define PRT_WALK8_ARGS *a.sc, in.o, in.d, in.hit, in.hd2, a.count, a.work, a.work + 512, tune
    if (l.form == PRT_WALK_SEEDED) hipLaunchKernelGGL((k_occluded8_seeded<L, W, IN, LN>), grid, block, 0, st, PRT_WALK8_ARGS);
    else if (l.form == PRT_WALK_ANY) hipLaunchKernelGGL((k_occluded8_persistent<L, W, IN, LN>), grid, block, 0, st, PRT_WALK8_ARGS);
    else if (LN && l.prim) {
        if constexpr (LN) {  // (no PRIM instance of another row exists)
            if (stats) hipLaunchKernelGGL((k_traverse8_persistent<L, W, true, IN, LN, true>), grid, block, 0, st, PRT_WALK8_ARGS, stats, *a.primary, PrtPathArgs{});
            else hipLaunchKernelGGL((k_traverse8_persistent<L, W, false, IN, LN, true>), grid, block, 0, st, PRT_WALK8_ARGS, stats, *a.primary, PrtPathArgs{});
        }
    } else if (stats) hipLaunchKernelGGL((k_traverse8_persistent<L, W, true, IN, LN>), grid, block, 0, st, PRT_WALK8_ARGS, stats, PrtPrimary{}, PrtPathArgs{});
    else hipLaunchKernelGGL((k_traverse8_persistent<L, W, false, IN, LN>), grid, block, 0, st, PRT_WALK8_ARGS, stats, PrtPrimary{}, PrtPathArgs{});
#undef PRT_WALK8_ARGS
}

static void launch_walk_row(hipStream_t st, const PrtWalkLaunch& l, const PrtWalkArgs& a) {
    const PrtTravTuning tune = walk_tuning(*a.tune, l);
    const dim3 grid(l.grid), block(256);
    const PrtRayBuf& in = a.rays;
    uint32_t* ovf = a.work + 512;  // [0] = count, [1..] = ray slots that overflowed the LDS stack
    const uint32_t* count = l.overflow ? ovf : a.count;
    const uint32_t* list = l.overflow ? ovf + 1 : nullptr;
    unsigned long long* stats = l.stats ? a.stats : nullptr;
    if (l.reset) hipLaunchKernelGGL(k_reset_cursors, dim3(1), dim3(64), 0, st, a.work);
#define PRT_WALK_T_ARGS *a.sc, in.o, in.d, in.hit, in.hd2, count, a.work, a.spill, list, ovf, tune, stats
#define PRT_WALK_T(KERNEL, L, W, MODE)                                                                          \
    {                                                                                                           \
        if (stats) hipLaunchKernelGGL((KERNEL<L, W, MODE, true>), grid, block, 0, st, PRT_WALK_T_ARGS);         \
        else hipLaunchKernelGGL((KERNEL<L, W, MODE, false>), grid, block, 0, st, PRT_WALK_T_ARGS);              \
        break;                                                                                                  \
    }
#define PRT_WALK8_CASE(name, L, W, IN, LN) case PRT_W8_##name: launch_walk8<L, W, IN, LN>(st, l, a, tune); break;
#define PRT_WALK4_CASE(tag, L, W, MODE) case PRT_W4_##tag: PRT_WALK_T(k_traverse4_persistent, L, W, MODE)
#define PRT_WALK2_CASE(tag, L, W, MODE) case PRT_W2_##tag: PRT_WALK_T(k_traverse_persistent, L, W, MODE)
#define PRT_INTERSECT_CASE(tag, S, V)                                                                                         \
    case PRT_WI_##tag:                                                                                                        \
        if (stats) hipLaunchKernelGGL((k_intersect<S, true, V>), grid, block, 0, st, *a.sc, in.o, in.d, in.hit, a.count, stats);  \
        else hipLaunchKernelGGL((k_intersect<S, false, V>), grid, block, 0, st, *a.sc, in.o, in.d, in.hit, a.count, stats);       \
        break;
    switch (l.row) {
        PRT_WALK8_ROWS(PRT_WALK8_CASE)
        PRT_WALK4_ROWS(PRT_WALK4_CASE)
        PRT_WALK2_ROWS(PRT_WALK2_CASE)
        PRT_INTERSECT_ROWS(PRT_INTERSECT_CASE)
        case PRT_WALK_ROWS: break;
    }
#undef PRT_INTERSECT_CASE
#undef PRT_WALK2_CASE
#undef PRT_WALK4_CASE
#undef PRT_WALK8_CASE
#undef PRT_WALK_T
#undef PRT_WALK_T_ARGS
}

void prt_launch_walk(hipStream_t st, const PrtWalkPlan& plan, const PrtWalkArgs& a) {
#ifdef PRT_PROBE_REBOUND
    // diagnostic build (tools/bounce_stats.py --rebound): the instrumented walk is preceded by the same plan with stats off, which
    // leaves every ray's FINAL hit distance as its initial culling bound, so the instrumented walk's visit counts are those of a
    // traversal that knew the answer from the start: the floor for any visiting order / triangle-test schedule
    if (plan.launch[0].stats && a.stats && prt_walk_row(plan.launch[0].row).family != 0u) {
        PrtWalkPlan plain = plan;
        plain.launch[0].stats = plain.launch[1].stats = false;
        prt_launch_walk(st, plain, a);
        hipLaunchKernelGGL(k_reset_cursors, dim3(1), dim3(64), 0, st, a.work);
    }
#endif
    for (uint32_t i = 0; i < plan.n; ++i) launch_walk_row(st, plan.launch[i], a);
}

// The PATH instance (PrtPathArgs): whole paths in one launch, for small batches.  (The deep15 row is the only one with one.)
void prt_launch_path(hipStream_t st, const PrtWalkPlan& plan, const DevScene& sc, const PrtPathArgs& pa, uint32_t* work, const PrtTravTuning& tune_in) {
    const PrtTravTuning tune = walk_tuning(tune_in, plan.launch[0]);
    hipLaunchKernelGGL((k_traverse8_persistent<15, 4, false, false, false, false, true>), dim3(plan.launch[0].grid), dim3(256), 0, st, sc,
                       (const float4*)nullptr, (const float4*)nullptr, (uint32_t*)nullptr, (const float*)nullptr, (const uint32_t*)nullptr, work,
                       work + 512, tune, (unsigned long long*)nullptr, PrtPrimary{}, pa);
}

// Static occupancy of the instance plan.occupancy names (what the wavefront-occupancy figure of the bench line is computed from):
// resident 256-thread blocks per CU by the runtime's occupancy calculator, and the kernel's register / LDS footprint.
int prt_walk_occupancy(const PrtWalkPlan& plan, int* blocks_per_cu, int* vgprs, int* sgprs, int* lds_bytes) {
    const void* fn = (const void*)k_traverse4_persistent<32, 4, 3, false>;
#define PRT_WALK8_CASE(name, L, W, IN, LN) if (plan.occupancy == PRT_W8_##name) fn = (const void*)k_traverse8_persistent<L, W, false, IN, LN>;
    PRT_WALK8_ROWS(PRT_WALK8_CASE)
#undef PRT_WALK8_CASE
    hipFuncAttributes at;
    hipError_t e = hipFuncGetAttributes(&at, fn);
    if (e != hipSuccess) return (int)e;
    int nb = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, 0);
    if (e != hipSuccess) return (int)e;
    *blocks_per_cu = nb;
    *vgprs = at.numRegs;
    *sgprs = 0;
    *lds_bytes = (int)at.sharedSizeBytes;
    return 0;
}

bool prt_launch_shade(hipStream_t st, PrtShadeInst inst, const PrtShadeArgs& a) {
    // n_rays_known: the ray count of this bounce if the host has it already (0xFFFFFFFF: size the grid for `cap`)
    const uint32_t n_for_grid = a.n_rays_known == 0xFFFFFFFFu ? a.cap : (a.n_rays_known ? a.n_rays_known : 1u);
    const dim3 grid((uint32_t)((n_for_grid + SHADE_BLOCK - 1) / SHADE_BLOCK));
    const DevScene& sc = *a.sc;
    const PrtPrimary& pr = or_empty(a.primary);
    const DevEnv& e = or_empty(a.env);
    const DevTex& tex = or_empty(a.tex);
    const DevLights& lt = or_empty(a.lights);
    const DevMeshLights& m = or_empty(a.mesh_lights);
    const DevLightClusters& lc = or_empty(a.clusters);
    const PrtLightBufs& lb = or_empty(a.lb);
#define PRT_SHADE_RAYS a.in.o, a.in.d, a.in.t, a.in.hit, a.out.o, a.out.d, a.out.t, a.out.hit, a.out.hd2
#define PRT_SHADE_TAIL_D(D) a.rad, a.counts, a.work, a.depth, D, a.cap, a.sp
#define PRT_SHADE_TAIL PRT_SHADE_TAIL_D(a.max_depth)
    // (only k_shade / k_shade_env / k_shade_tex know the flag bit: the NEE family never sees it, whatever the plan says)
#define PRT_SHADE_TAIL_LS PRT_SHADE_TAIL_D((a.last_segment ? a.max_depth | PRT_LAST_SEGMENT_FLAG : a.max_depth))
#define PRT_SHADE_ARGS_PLAIN sc, PRT_SHADE_RAYS, PRT_SHADE_TAIL_LS, pr
#define PRT_SHADE_ARGS_ENV sc, e, PRT_SHADE_RAYS, PRT_SHADE_TAIL_LS
#define PRT_SHADE_ARGS_TEX sc, tex, e, PRT_SHADE_RAYS, PRT_SHADE_TAIL_LS
#define PRT_SHADE_ARGS_NEE sc, lt, PRT_SHADE_RAYS, lb, PRT_SHADE_TAIL
#define PRT_SHADE_ARGS_NEE_ENV sc, lt, e, PRT_SHADE_RAYS, lb, PRT_SHADE_TAIL
#define PRT_SHADE_ARGS_NEE_MESH sc, lt, m, PRT_SHADE_RAYS, lb, PRT_SHADE_TAIL
#define PRT_SHADE_ARGS_NEE_MESH_ENV sc, lt, m, e, PRT_SHADE_RAYS, lb, PRT_SHADE_TAIL
#define PRT_SHADE_ARGS_NEE_TEX sc, tex, lt, m, e, PRT_SHADE_RAYS, lb, PRT_SHADE_TAIL
#define PRT_SHADE_ARGS_NEE_CLUS sc, lt, m, lc, PRT_SHADE_RAYS, lb, PRT_SHADE_TAIL
#define PRT_SHADE_ARGS_NEE_CLUS_ENV sc, lt, m, lc, e, PRT_SHADE_RAYS, lb, PRT_SHADE_TAIL
#define PRT_SHADE_ARGS_NEE_CLUS_TEX sc, tex, lt, m, lc, e, PRT_SHADE_RAYS, lb, PRT_SHADE_TAIL
#define PRT_SHADE_CASE(sig, kernel, tag, ...) \
    case PRT_INST(kernel, tag): hipLaunchKernelGGL((kernel<__VA_ARGS__>), grid, dim3(SHADE_BLOCK), 0, st, PRT_SHADE_ARGS_##sig); return true;
    switch (inst) {
        PRT_SHADE_INSTANCES(PRT_SHADE_CASE)
        default: return false;
    }
#undef PRT_SHADE_CASE
#undef PRT_SHADE_ARGS_NEE_CLUS_TEX
#undef PRT_SHADE_ARGS_NEE_CLUS_ENV
#undef PRT_SHADE_ARGS_NEE_CLUS
#undef PRT_SHADE_ARGS_NEE_TEX
#undef PRT_SHADE_ARGS_NEE_MESH_ENV
#undef PRT_SHADE_ARGS_NEE_MESH
#undef PRT_SHADE_ARGS_NEE_ENV
#undef PRT_SHADE_ARGS_NEE
#undef PRT_SHADE_ARGS_TEX
#undef PRT_SHADE_ARGS_ENV
#undef PRT_SHADE_ARGS_PLAIN
#undef PRT_SHADE_TAIL_LS
#undef PRT_SHADE_TAIL
#undef PRT_SHADE_TAIL_D
#undef PRT_SHADE_RAYS
}

void prt_launch_shade_divstats(hipStream_t st, const DevScene& sc, const PrtRayBuf& in, const uint32_t* counts, uint32_t iter,
                               uint32_t cap, unsigned long long* out, const PrtPrimary* primary) {
    hipLaunchKernelGGL(k_shade_divstats, dim3((cap + SHADE_BLOCK - 1u) / SHADE_BLOCK), dim3(SHADE_BLOCK), 0, st, sc, in.hit, counts, iter, cap, out,
                       primary ? *primary : PrtPrimary{}, primary ? 1 : 0);
}

void prt_launch_primary_hit(hipStream_t st, const DevScene& sc, const PrtPrimary& pr, const uint32_t* hit, float4* pix,
                            const uint32_t* counts) {
    hipLaunchKernelGGL(k_primary_hit, dim3(blocks_for(pr.ids.n_pix_local)), dim3(256), 0, st, sc, pr, hit, pix, counts);
}

bool prt_launch_accumulate(hipStream_t st, PrtAccumulateInst inst, const PrtAccumulateArgs& a) {
    const uint32_t nb = blocks_for(a.tm.n_pix_local ? a.tm.n_pix_local : 1);
    const dim3 grid(nb < 8192u ? nb : 8192u);
    const int upd = a.update_film ? 1 : 0;
    if (a.pixel_major_ids) {
        // Pixel-major path ids come with compact primary rays, whose plan names k_accumulate or, with film statistics,
        // k_accumulate_stat<false, false>: the same sums from the other layout of rad[] (k_accumulate_pixel_major), launched
        // under the plan's instance, which is what prt_batch_instance goes on reporting
        if (inst != PRT_I_k_accumulate && inst != PRT_INST(k_accumulate_stat, ff)) return false;
        const uint32_t nbp = (a.tm.n_pix_local + PRT_ACC_PM_BLOCK - 1u) / PRT_ACC_PM_BLOCK;
        const dim3 grid_pm(nbp < 8192u ? (nbp ? nbp : 1u) : 8192u);
        if (inst == PRT_I_k_accumulate)
            hipLaunchKernelGGL((k_accumulate_pixel_major<false>), grid_pm, dim3(PRT_ACC_PM_BLOCK), 0, st, a.rad, a.film_local, a.stat, a.tm, a.S, a.max_depth, upd,
                               a.ray_stats, a.pix_end);
        else
            hipLaunchKernelGGL((k_accumulate_pixel_major<true>), grid_pm, dim3(PRT_ACC_PM_BLOCK), 0, st, a.rad, a.film_local, a.stat, a.tm, a.S, a.max_depth, upd,
                               a.ray_stats, a.pix_end);
        return true;
    }
#define PRT_ACC_ARGS_PLAIN a.rad, a.film_local, a.tm, a.S, a.max_depth, upd, a.ray_stats, a.pix_end
#define PRT_ACC_ARGS_LIT a.rad, a.lrad, a.film_local, a.tm, a.S, a.max_depth, upd, a.ray_stats
#define PRT_ACC_ARGS_STAT a.rad, a.lrad, a.film_local, a.stat, a.tm, a.S, a.max_depth, upd, a.ray_stats, a.pix_end, a.list
#define PRT_ACC_CASE_N(sig, kernel) \
    case PRT_I_##kernel: hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, PRT_ACC_ARGS_##sig); return true;
#define PRT_ACC_CASE_T(sig, kernel, tag, ...) \
    case PRT_INST(kernel, tag): hipLaunchKernelGGL((kernel<__VA_ARGS__>), grid, dim3(256), 0, st, PRT_ACC_ARGS_##sig); return true;
    switch (inst) {
        PRT_ACCUMULATE_INSTANCES(PRT_ACC_CASE_N, PRT_ACC_CASE_T)
        default: return false;
    }
#undef PRT_ACC_CASE_T
#undef PRT_ACC_CASE_N
#undef PRT_ACC_ARGS_STAT
#undef PRT_ACC_ARGS_LIT
#undef PRT_ACC_ARGS_PLAIN
}

void prt_launch_resolve(hipStream_t st, const float4* gathered, uint32_t world, uint32_t stride, uint32_t W,
                        uint32_t H, float* rgb, float* weight) {
    hipLaunchKernelGGL(k_resolve, dim3(blocks_for((uint64_t)W * H)), dim3(256), 0, st, gathered, world, stride, W, H,
                       rgb, weight);
}

void prt_launch_tonemap(hipStream_t st, const float* rgb, const float* weight, uint32_t n_pix, float exposure,
                        float inv_gamma, uint8_t* out) {
    hipLaunchKernelGGL(k_tonemap, dim3(blocks_for((uint64_t)n_pix * 4u)), dim3(256), 0, st, rgb, weight, n_pix,
                       exposure, inv_gamma, out);
}

void prt_launch_camera_rays_lens(hipStream_t st, const DevCamera& cam, const DevLens& lens, uint32_t n, const float* px,
                                 const float* py, uint32_t* keys, float* o, float* d) {
    hipLaunchKernelGGL(k_camera_rays_lens, dim3(blocks_for(n)), dim3(256), 0, st, cam, lens, n, px, py, keys, o, d);
}
void prt_launch_camera_rays(hipStream_t st, const DevCamera& cam, uint32_t n, const float* px, const float* py,
                            float* o, float* d) {
    hipLaunchKernelGGL(k_camera_rays, dim3(blocks_for(n)), dim3(256), 0, st, cam, n, px, py, o, d);
}

void prt_launch_pack_rays(hipStream_t st, uint32_t n, const float* o, const float* d, const PrtRayBuf& out,
                          uint32_t* counts) {
    hipLaunchKernelGGL(k_pack_rays, dim3(blocks_for(n)), dim3(256), 0, st, n, o, d, out.o, out.d, counts);
}

void prt_launch_hit_records(hipStream_t st, const DevScene& sc, uint32_t n, const PrtRayBuf& in, PrtHit* out) {
    hipLaunchKernelGGL(k_hit_records, dim3(blocks_for(n)), dim3(256), 0, st, sc, n, in.o, in.d, in.hit, out);
}

void prt_launch_pack_occlusion_rays(hipStream_t st, uint32_t n, const float* o, const float* d, const float* tmax,
                                    const PrtRayBuf& out, uint32_t* counts) {
    hipLaunchKernelGGL(k_pack_occlusion_rays, dim3(blocks_for(n)), dim3(256), 0, st, n, o, d, tmax, out.o, out.d, out.hit,
                       out.hd2, counts);
}

void prt_launch_scan_prims_bounded(hipStream_t st, const DevScene& sc, const PrtRayBuf& in, const uint32_t* count_ptr,
                                   uint32_t* work, uint32_t max_rays) {
    hipLaunchKernelGGL(k_scan_prims_bounded, dim3(blocks_for(max_rays)), dim3(256), 0, st, sc, in.o, in.d, in.hit, in.hd2,
                       count_ptr, work);
}

void prt_launch_occlusion_bytes(hipStream_t st, const DevScene& sc, uint32_t n, const PrtRayBuf& in, const float* tmax,
                                uint8_t* out) {
    hipLaunchKernelGGL(k_occlusion_bytes, dim3(blocks_for(n)), dim3(256), 0, st, sc, n, in.o, in.d, in.hit, tmax, out);
}

void prt_launch_scatter_test(hipStream_t st, const DevScene& sc, uint32_t n, const float* in_d, const PrtHit* hits,
                             uint32_t* rng_io, uint32_t* scattered, float* atten, float* emitted, float* o_out,
                             float* d_out) {
    hipLaunchKernelGGL(k_scatter_test, dim3(blocks_for(n)), dim3(256), 0, st, sc, n, in_d, hits, rng_io, scattered,
                       atten, emitted, o_out, d_out);
}

void prt_launch_light_accum(hipStream_t st, const DevScene& sc, const PrtLightBufs& lb, const uint32_t* count_ptr,
                            uint32_t* work, uint32_t max_rays) {
    hipLaunchKernelGGL(k_light_accum, dim3(blocks_for(max_rays ? max_rays : 1u)), dim3(256), 0, st, sc, lb, count_ptr, work);
}

void prt_launch_sample_light_test(hipStream_t st, const DevScene& sc, const DevLights& lt, uint32_t n, const float* in_d,
                                  const PrtHit* hits, const uint32_t* keys, float* out_f, uint32_t* out_light, const DevMeshLights* ml,
                                  const DevEnv* env, const DevLightClusters* lc) {
    if (lc && ml) {
        if (env)
            hipLaunchKernelGGL(k_sample_light_test_clus_env, dim3(blocks_for(n)), dim3(256), 0, st, sc, lt, *ml, *lc, *env, n, in_d, hits, keys, out_f, out_light);
        else
            hipLaunchKernelGGL(k_sample_light_test_clus, dim3(blocks_for(n)), dim3(256), 0, st, sc, lt, *ml, *lc, n, in_d, hits, keys, out_f, out_light);
        return;
    }
    if (env) {
        if (ml)
            hipLaunchKernelGGL(k_sample_light_test_mesh_env, dim3(blocks_for(n)), dim3(256), 0, st, sc, lt, *ml, *env, n, in_d, hits, keys, out_f, out_light);
        else
            hipLaunchKernelGGL(k_sample_light_test_env, dim3(blocks_for(n)), dim3(256), 0, st, sc, lt, *env, n, in_d, hits, keys, out_f, out_light);
        return;
    }
    if (ml) {
        hipLaunchKernelGGL(k_sample_light_test_mesh, dim3(blocks_for(n)), dim3(256), 0, st, sc, lt, *ml, n, in_d, hits, keys, out_f, out_light);
        return;
    }
    hipLaunchKernelGGL(k_sample_light_test, dim3(blocks_for(n)), dim3(256), 0, st, sc, lt, n, in_d, hits, keys, out_f, out_light);
}

void prt_launch_light_cluster_pmf(hipStream_t st, const DevLightClusters& lc, uint32_t n, const float* x, uint32_t* M) {
    hipLaunchKernelGGL(k_light_cluster_pmf, dim3(blocks_for(n)), dim3(256), 0, st, lc, n, x, M);
}

void prt_launch_environment_eval(hipStream_t st, const DevEnv& env, uint32_t n, const float* dirs, float* rgb, uint32_t* texel,
                                 float* pdf_w) {
    hipLaunchKernelGGL(k_environment_eval, dim3(blocks_for(n)), dim3(256), 0, st, env, n, dirs, rgb, texel, pdf_w);
}

void prt_launch_texture_eval(hipStream_t st, const DevTex& tex, uint32_t n, const uint32_t* texture, const float* uv, float* rgb) {
    hipLaunchKernelGGL(k_texture_eval, dim3(blocks_for(n)), dim3(256), 0, st, tex, n, texture, uv, rgb);
}

void prt_launch_hit_uv(hipStream_t st, const DevScene& sc, const DevTex& tex, uint32_t n, const PrtRayBuf& in, float* uv, float* albedo) {
    hipLaunchKernelGGL(k_hit_uv, dim3(blocks_for(n)), dim3(256), 0, st, sc, tex, n, in.o, in.d, in.hit, uv, albedo);
}


void prt_launch_tile_select(hipStream_t st, const float4* film_local, const float2* stat, const PrtTileMap& tm, const uint32_t* prev,
                            uint32_t n_in, float threshold, float noise_floor, uint32_t* flags, uint32_t* out, uint32_t* count) {
    if (n_in) hipLaunchKernelGGL(k_tile_select, dim3((n_in + 3u) / 4u), dim3(256), 0, st, film_local, stat, tm, prev, n_in, threshold,
                                 noise_floor, flags);
    hipLaunchKernelGGL(k_tile_compact, dim3(1), dim3(1024), 0, st, flags, prev, n_in, out, count);
}

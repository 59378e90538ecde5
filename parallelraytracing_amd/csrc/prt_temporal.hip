// prt_temporal.hip — the device code of the temporal reprojection (include/prt.h "Temporal reprojection").  A translation
// unit of its own: nothing in prt_kernels.hip or prt_denoise.hip changes for it.  Built with the flags of prt_kernels.hip:
// no contraction, so every line below and every line of prt_temporal_contract.h is the IEEE operation it spells, and
// tests/temporal_replay.py restates them in numpy float32.
#include <hip/hip_runtime.h>

#include "prt_temporal.h"
#include "prt_temporal_contract.h"

namespace {

inline uint32_t blocks_for(uint32_t n) { return (n + 255u) / 256u; }

struct TpArgs {
    uint32_t W, H, tiles_x;
    PrtTemporal cfg;
    PrtCameraBasis K;
    // the current frame: records (arrays) or the film, its moments and the feature records (film)
    const float4* cur_cn;
    const float2* cur_aq;
    const float4* cur_nrm;
    const float4* cur_pos;
    PrtMotionTable mt;
    PrtHistoryBufs prev, next;
    float* mean;
    float* var;
    uint8_t* status;
    unsigned long long* counts;  // hit pixels in the low half, pixels with status 1 in the high half
};

__global__ void k_tp_pack_frame(uint32_t n, const float* __restrict__ c, const float* __restrict__ w, const float* __restrict__ A,
                                const float* __restrict__ Q, const int32_t* __restrict__ prim, const float* __restrict__ P,
                                const float* __restrict__ N, float4* __restrict__ cn, float2* __restrict__ aq, float4* __restrict__ nrm,
                                float4* __restrict__ pos) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t j = 3 * (size_t)i;
    cn[i] = make_float4(c[j], c[j + 1], c[j + 2], w[i]);
    aq[i] = make_float2(A[i], Q[i]);
    nrm[i] = make_float4(N[j], N[j + 1], N[j + 2], __int_as_float(prim[i]));
    pos[i] = make_float4(P[j], P[j + 1], P[j + 2], 0.0f);
}

__global__ void k_tp_unpack(uint32_t n, const float4* __restrict__ cn, const float2* __restrict__ mm, float* __restrict__ n_out,
                            float* __restrict__ m1_out, float* __restrict__ m2_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    n_out[i] = cn[i].w;
    const float2 m = mm[i];
    m1_out[i] = m.x;
    m2_out[i] = m.y;
}

// One thread per pixel, block = 64 x 4: a wave takes 64 consecutive pixels of one row, so under coherent motion its four
// tap gathers land on a few neighbouring lines of the previous frame.  Per pixel 56 B of history are gathered per tap and
// 56 B of the current frame are read (film 16, moments 8, nrm 16, pos 16; the array instance: its four records).  The film
// instance writes 56 B of new history and 17 B of mean / variance / status, the array instance 24 B ({c', N'}, {m1', m2'};
// its caller has the surface already) and the same 17 B.  The tap loop is unrolled and indexes no array: no scratch.  The previous set is read, the next one written: never in place.
template <bool FILM>
__global__ void __launch_bounds__(256) k_tp_reproject(TpArgs a) {
    __shared__ unsigned long long s_cnt;
    const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
    const bool active = x < a.W && y < a.H;
    if (a.counts) {
        if (threadIdx.x == 0u && threadIdx.y == 0u) s_cnt = 0ull;
        __syncthreads();
    }
    bool hit = false, reproj = false;
    if (active) {
        const uint32_t ip = y * a.W + x;
        // ---- the current pixel: c, n, m1, m2, its surface now and as it was ----
        float cr, cg, cb, n, A, Q;
        float4 np, pp;
        if (FILM) {
            const uint32_t pl = ((y >> 3) * a.tiles_x + (x >> 3)) * 64u + ((y & 7u) << 3) + (x & 7u);
            const float4 f = a.cur_cn[pl];
            const float2 s = a.cur_aq[pl];
            n = f.w;
            cr = prt_denoise_mean_rule(f.x, n);
            cg = prt_denoise_mean_rule(f.y, n);
            cb = prt_denoise_mean_rule(f.z, n);
            A = s.x;
            Q = s.y;
        } else {
            const float4 f = a.cur_cn[ip];
            const float2 s = a.cur_aq[ip];
            cr = f.x;
            cg = f.y;
            cb = f.z;
            n = f.w;
            A = s.x;
            Q = s.y;
        }
        np = a.cur_nrm[ip];
        pp = a.cur_pos[ip];
        const int32_t prim = __float_as_int(np.w);
        hit = prim >= 0;
        const float m1 = n > 0.0f ? A / n : 0.0f, m2 = n > 0.0f ? Q / n : 0.0f;
        PrtTpV3 Pv{pp.x, pp.y, pp.z}, Nv{np.x, np.y, np.z};
        float o_r = cr, o_g = cg, o_b = cb, o_n = n, o_m1 = m1, o_m2 = m2, o_var;
        if (a.prev.cn && hit) {
            if (FILM) {
                const int32_t k = prt_temporal_find_copy(a.mt.range, a.mt.n, prim);
                if (k >= 0) {
                    const float4* q = a.mt.xf + 6u * (uint32_t)k;
                    const float4 i0 = q[0], i1 = q[1], i2 = q[2], p0 = q[3], p1 = q[4], p2 = q[5];
                    const float inv[12] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w, i2.x, i2.y, i2.z, i2.w};
                    const float mat[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
                    prt_temporal_prev_surface_rule(inv, mat, Pv, Nv, &Pv, &Nv);
                }
            }
            float fx, fy, vv, z;
            if (prt_temporal_project(a.K, Pv, &fx, &fy, &vv, &z)) {
                const float flx = floorf(fx), fly = floorf(fy);
                const float tx = fx - flx, ty = fy - fly;
                const int ix = (int)flx, iy = (int)fly;  // in [-1, W - 1] x [-1, H - 1]
                const float lim = a.cfg.plane_tol * sqrtf(vv);
                float Sb = 0.0f, Sr = 0.0f, Sg = 0.0f, Sbl = 0.0f, Sn = 0.0f, S1 = 0.0f, S2 = 0.0f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int xx = ix + (t & 1), yy = iy + (t >> 1);
                    if (xx < 0 || xx >= (int)a.W || yy < 0 || yy >= (int)a.H) continue;
                    const uint32_t iq = (uint32_t)yy * a.W + (uint32_t)xx;
                    const float4 hcn = a.prev.cn[iq];
                    const float4 hnr = a.prev.nrm[iq];
                    const float4 hps = a.prev.pos[iq];
                    if (!prt_temporal_tap_valid(hcn.w, __float_as_int(hnr.w), PrtTpV3{hnr.x, hnr.y, hnr.z}, PrtTpV3{hps.x, hps.y, hps.z}, Pv, Nv,
                                                a.cfg.normal_min, lim))
                        continue;
                    const float2 hmm = a.prev.mm[iq];
                    const float b = ((t & 1) ? tx : 1.0f - tx) * ((t >> 1) ? ty : 1.0f - ty);
                    Sb += b;
                    Sr += b * hcn.x;
                    Sg += b * hcn.y;
                    Sbl += b * hcn.z;
                    Sn += b * hcn.w;
                    S1 += b * hmm.x;
                    S2 += b * hmm.y;
                }
                if (!(Sb < PRT_TEMPORAL_SB_MIN)) {
                    const float hr = Sr / Sb, hg = Sg / Sb, hb = Sbl / Sb, Nh = Sn / Sb, H1 = S1 / Sb, H2 = S2 / Sb;
                    const float N1 = fminf(Nh + n, a.cfg.max_history);
                    const float al = fminf(n / N1, 1.0f);
                    o_r = prt_temporal_blend(hr, cr, al);
                    o_g = prt_temporal_blend(hg, cg, al);
                    o_b = prt_temporal_blend(hb, cb, al);
                    o_m1 = prt_temporal_blend(H1, m1, al);
                    o_m2 = prt_temporal_blend(H2, m2, al);
                    o_n = N1;
                    reproj = true;
                }
            }
        }
        o_var = reproj ? prt_temporal_variance_rule(o_n, o_m1, o_m2) : prt_denoise_variance_rule(n, A, Q);
        a.next.cn[ip] = make_float4(o_r, o_g, o_b, o_n);
        a.next.mm[ip] = make_float2(o_m1, o_m2);
        if (FILM) {  // the new history keeps the surface as it is now (the arrays' caller has it already)
            a.next.nrm[ip] = np;
            a.next.pos[ip] = pp;
        }
        const size_t j = 3 * (size_t)ip;
        a.mean[j] = o_r;
        a.mean[j + 1] = o_g;
        a.mean[j + 2] = o_b;
        if (a.var) a.var[ip] = o_var;
        if (a.status) a.status[ip] = reproj ? (uint8_t)1 : (uint8_t)0;
    }
    if (a.counts) {  // (block-uniform) a ballot per wave, one LDS atomic per wave, one global atomic per block
        const unsigned long long mh = __ballot(hit), mr = __ballot(reproj);
        if (threadIdx.x == 0u) atomicAdd(&s_cnt, ((unsigned long long)__popcll(mr) << 32) | (unsigned long long)__popcll(mh));
        __syncthreads();
        if (threadIdx.x == 0u && threadIdx.y == 0u) atomicAdd(a.counts, s_cnt);
    }
}

}  // namespace

void prt_launch_tp_pack_frame(hipStream_t st, uint32_t n, const float* c, const float* w, const float* A, const float* Q, const int32_t* prim,
                              const float* P, const float* N, float4* cn, float2* aq, float4* nrm, float4* pos) {
    hipLaunchKernelGGL(k_tp_pack_frame, dim3(blocks_for(n)), dim3(256), 0, st, n, c, w, A, Q, prim, P, N, cn, aq, nrm, pos);
}

void prt_launch_tp_unpack(hipStream_t st, uint32_t n, PrtHistoryBufs h, float* n_out, float* m1_out, float* m2_out) {
    hipLaunchKernelGGL(k_tp_unpack, dim3(blocks_for(n)), dim3(256), 0, st, n, h.cn, h.mm, n_out, m1_out, m2_out);
}

void prt_launch_tp_reproject(hipStream_t st, uint32_t W, uint32_t H, const PrtTemporal& cfg, const PrtCameraBasis& K, PrtTemporalFrame cur,
                             PrtHistoryBufs prev, PrtHistoryBufs next, float* mean, float* var, uint8_t* status, uint32_t* counts) {
    const TpArgs a{W, H, 0u, cfg, K, cur.cn, cur.aq, cur.nrm, cur.pos, PrtMotionTable{nullptr, nullptr, 0u}, prev, next, mean, var, status,
                   (unsigned long long*)counts};
    hipLaunchKernelGGL(k_tp_reproject<false>, dim3((W + 63u) / 64u, (H + 3u) / 4u), dim3(64, 4), 0, st, a);
}

void prt_launch_tp_reproject_film(hipStream_t st, const PrtTileMap& tm, const PrtTemporal& cfg, const PrtCameraBasis& K,
                                  const float4* film_local, const float2* film_stat, const float4* feat_nrm, const float4* feat_pos,
                                  PrtMotionTable mt, PrtHistoryBufs prev, PrtHistoryBufs next, float* mean, float* var, uint8_t* status,
                                  uint32_t* counts) {
    const TpArgs a{tm.W, tm.H, tm.tiles_x, cfg, K, film_local, film_stat, feat_nrm, feat_pos, mt, prev, next, mean, var, status,
                   (unsigned long long*)counts};
    hipLaunchKernelGGL(k_tp_reproject<true>, dim3((tm.W + 63u) / 64u, (tm.H + 3u) / 4u), dim3(64, 4), 0, st, a);
}

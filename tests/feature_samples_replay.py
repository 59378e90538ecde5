"""Restatement of the sampled guide features (include/prt.h "Sampled guide features", steps 3 and 4) in numpy float32: the
ordered running sums over a pixel's per-sample records and the finish, every operation in the contract's order.  The
per-sample records themselves are the guide rule's (tests/guide_features_replay.py) on the render's own primary rays
(tests/lens_replay.py: path_seeds, jittered_points); sample_keys_and_points forms those."""
import numpy as np

import lens_replay as lr

F = np.float32
KEYS = ("albedo", "normal", "position", "depth", "prim", "hits")


def sample_keys_and_points(W, H, K, seed, first_sample, jitter):
    """Sample-major (s, then pixel p = y W + x): the pixel-space points (px, py) of the K * W * H primary rays and each
    path's RNG state after the jitter draws: what prt_camera_rays_lens is given."""
    pix = np.tile(np.arange(W * H), K)
    samp = np.repeat(np.arange(K), W * H) + int(first_sample)
    keys = lr.path_seeds(pix, samp, seed)
    return lr.jittered_points(pix, W, keys, jitter)


def reduce_samples(records):
    """records: per sample s = 0 .. K - 1 a dict of albedo, normal, position (n, 3) float32, depth (n,) float32 and prim (n,)
    int32 (n pixels, any leading shape flattened by the caller).  -> the sampled set of the n pixels: albedo, normal, position
    (n, 3), depth (n,), prim (n,) int32, hits (n,) uint32."""
    K = len(records)
    assert K >= 1
    n = np.asarray(records[0]["prim"]).size
    Sa, Sn, Sp = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros((n, 3), F)
    Sd, hits = np.zeros(n, F), np.zeros(n, F)
    prim = np.full(n, -1, np.int32)
    for rec in records:                                                       # sample order: the sums are running fp32
        a = np.asarray(rec["albedo"], F).reshape(n, 3)
        nr = np.asarray(rec["normal"], F).reshape(n, 3)
        ps = np.asarray(rec["position"], F).reshape(n, 3)
        dp = np.asarray(rec["depth"], F).reshape(n)
        pr = np.asarray(rec["prim"], np.int32).reshape(n)
        hit = pr >= 0
        Sa = (Sa + a).astype(F)
        prim = np.where(hit & (hits == 0), pr, prim).astype(np.int32)
        Sn = np.where(hit[:, None], (Sn + nr).astype(F), Sn)
        Sp = np.where(hit[:, None], (Sp + ps).astype(F), Sp)
        Sd = np.where(hit, (Sd + dp).astype(F), Sd)
        hits = np.where(hit, (hits + F(1)).astype(F), hits)
    with np.errstate(all="ignore"):
        albedo = (Sa * (F(1) / F(K))).astype(F)
        some = hits > 0
        ih = (F(1) / hits).astype(F)
        position = np.where(some[:, None], (Sp * ih[:, None]).astype(F), F(0))
        depth = np.where(some, (Sd * ih).astype(F), F(0))
        l2 = ((Sn[:, 0] * Sn[:, 0] + Sn[:, 1] * Sn[:, 1]) + Sn[:, 2] * Sn[:, 2]).astype(F)   # dot3
        il = (F(1) / np.sqrt(l2)).astype(F)
        normal = np.where((some & (l2 > 0))[:, None], (Sn * il[:, None]).astype(F), F(0))
    return dict(albedo=albedo, normal=normal.astype(F), position=position.astype(F), depth=depth.astype(F),
                prim=np.where(some, prim, -1).astype(np.int32), hits=hits.astype(np.uint32))


def reshape(s, W, H):
    return {k: (v.reshape(H, W, 3) if v.ndim == 2 else v.reshape(H, W)) for k, v in s.items()}

"""numpy restatement of the SH probes (include/prt.h "SH probes"), written from the header text: the rays of a probe from
the RNG of tests/bake_replay.py (pcg_hash, path_seed, the rejection sampler of RandomUnitVector), the real spherical
harmonics up to order 2, the ordered coefficient sums and the irradiance the coefficients give, all in float32 with every
operation rounded once.

  * rays(positions, sample, seed): origin, direction and advanced RNG state of one sample of every probe.
  * ray_set(n_probes, samples, seed, first_sample): the directions and states of every (sample, probe), [S, P, ...].
  * basis(d, order): Y_k(d) [n, (order + 1)^2].
  * project(L, d, order): fl(L_c * Y_k(d)) [n, K, 3]; sums(values): their fp32 sum over the leading axis, in order, from 0.
  * coefficients(total, samples), irradiance(coeffs, normals).
  * hemisphere(d): the radiance of the 1 x 2 environment image of the closed-form tests (HEMI_A above, HEMI_B below).

No kernel code and no GPU is involved."""
from __future__ import annotations

import numpy as np

import bake_replay as br

F = np.float32
M32 = br.M32
C0, C1, C2A, C2B, C2C = F(0.282094792), F(0.488602512), F(1.092548431), F(0.315391565), F(0.546274215)
A_BAND = (F(3.14159274), F(2.09439516), F(0.785398185))      # the clamped cosine: pi, 2 pi / 3, pi / 4
FOUR_PI = F(4.0 * np.pi)
HEMI_A, HEMI_B = 1.0, 0.25


def count(order):
    return (int(order) + 1) ** 2


def keys(n_probes, samples, seed, first_sample=0):
    """path_seed(p, first_sample + s, seed) for every (s, p): [S, P] uint32"""
    p = np.arange(n_probes, dtype=np.uint64)[None, :]
    s = ((np.arange(samples, dtype=np.uint64) + np.uint64(int(first_sample) & 0xFFFFFFFF)) & M32)[:, None]
    k = np.uint64((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)
    return br.pcg_hash(((p ^ ((s * np.uint64(719393)) & M32)) + k) & M32)


def ray_set(n_probes, samples, seed, first_sample=0):
    """-> (d [S, P, 3] float32, rng_state [S, P] uint32): RandomUnitVector of every key, as returned, and the advanced state"""
    state, d = br.random_unit_vector(keys(n_probes, samples, seed, first_sample).ravel())
    return d.reshape(samples, n_probes, 3), state.reshape(samples, n_probes)


def rays(positions, sample, seed):
    """-> dict(o, d [P, 3], rng_state [P]) of sample `sample`"""
    x = np.asarray(positions, F).reshape(-1, 3)
    d, state = ray_set(len(x), 1, seed, sample)
    return dict(o=x.copy(), d=d[0], rng_state=state[0])


def basis(d, order=2):
    """Y_k of the directions as given, [n, K] float32: every product and difference is one fp32 operation"""
    d = np.asarray(d, F).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = [np.full(len(d), C0, F), C1 * y, C1 * z, C1 * x, C2A * (x * y), C2A * (y * z), C2B * (F(3.0) * (z * z) - F(1.0)), C2A * (x * z),
         C2C * ((x * x) - (y * y))]
    return np.stack(Y[:count(order)], axis=1).astype(F)


def project(L, d, order=2):
    """fl(L_c * Y_k(d)): [n, K, 3]"""
    L = np.asarray(L, F).reshape(-1, 3)
    return (L[:, None, :] * basis(d, order)[:, :, None]).astype(F)


def sums(values):
    """The fp32 sum over the leading axis in ascending order, from 0.0f"""
    values = np.asarray(values, F)
    acc = np.zeros(values.shape[1:], F)
    for v in values:
        acc = (acc + v).astype(F)
    return acc


def probe_sums(L, d, order=2):
    """L, d [S, P, 3] -> sh_sum [P, K, 3]"""
    S, P = d.shape[:2]
    return sums(np.stack([project(L[s], d[s], order) for s in range(S)]))


def coefficients(total, samples):
    return (np.asarray(total, F) * FOUR_PI / F(samples)).astype(F)


def irradiance(coeffs, normals):
    """coeffs [n, K, 3], normals [n, 3] -> E [n, 3]: from 0.0f over k ascending, fl(fl(A_k * Y_k(n)) * coeff[k][c])"""
    c = np.asarray(coeffs, F)
    K = c.shape[1]
    order = {1: 0, 4: 1, 9: 2}[K]
    Y = basis(normals, order)
    E = np.zeros((len(c), 3), F)
    for k in range(K):
        A = A_BAND[0] if k == 0 else (A_BAND[1] if k < 4 else A_BAND[2])
        w = (A * Y[:, k]).astype(F)
        E = (E + (w[:, None] * c[:, k, :]).astype(F)).astype(F)
    return E


def hemisphere(d):
    """[..., 3] float32: HEMI_A where d.y > 0, else HEMI_B: what a 1-wide, 2-high environment image over an empty scene delivers"""
    d = np.asarray(d, F)
    return np.where(d[..., 1:2] > 0, F(HEMI_A), F(HEMI_B)).astype(F) * np.ones(3, F)


def hemisphere_image():
    """The environment image [2, 1, 3] (row 0 is the +Y pole)"""
    return np.array([[[HEMI_A] * 3], [[HEMI_B] * 3]], F)

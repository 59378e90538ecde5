"""The numpy restatement of the SH probes (tests/probe_sh_replay.py) against closed forms, without a GPU.  The GPU tests hold
the device to the replay bit for bit, so what is shown here carries over to the device.  Seed 7 throughout.

1. Orthonormality: over the 4096 directions of one probe, (4 pi / N) sum Y_j Y_k is the identity to 0.125 (a wrong band-2
   constant moves a diagonal entry by 0.5 or more).
2. The bands above 0 have zero mean: |mean Y_k| sqrt(4 pi N) <= 4 (the variance of Y_k under the uniform density is 1 / (4 pi)).
3. A sky of HEMI_A above the horizon and HEMI_B below it: the irradiance from nine coefficients is pi a at +y, pi b at -y
   and pi (a + b) / 2 at +x, exactly in expectation (sign(y) has only odd bands, and of those the clamped cosine keeps band
   1 alone), within 4 standard errors estimated from the samples.
4. A constant sky c: coefficient 0 is c 2 sqrt(pi) to N 2^-24 relative and the irradiance is pi c for any normal."""
import numpy as np
import pytest

import probe_sh_replay as ps

F = np.float32
SEED = 7
AXES = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0]], F)


def test_basis_is_orthonormal_over_a_probes_directions():
    N = 4096
    d, _ = ps.ray_set(1, N, SEED)
    Y = ps.basis(d[:, 0], 2).astype(np.float64)
    G = (4.0 * np.pi / N) * (Y.T @ Y)
    worst = np.abs(G - np.eye(9)).max()
    print("orthonormality: worst entry", worst)
    assert worst <= 0.125, G
    l2 = (d.astype(np.float64) ** 2).sum(axis=2)
    assert np.abs(l2 - 1.0).max() <= 4e-7          # unit to fp32 rounding, as returned by the sampler


@pytest.mark.parametrize("P,N", [(3, 256), (1, 4096)])
def test_higher_bands_have_zero_mean(P, N):
    d, _ = ps.ray_set(P, N, SEED)
    z = []
    for p in range(P):
        Y = ps.basis(d[:, p], 2).astype(np.float64)
        z.append(np.abs(Y[:, 1:].mean(axis=0)) * np.sqrt(4.0 * np.pi * N))
    pooled = np.abs(ps.basis(d.reshape(-1, 3), 2).astype(np.float64)[:, 1:].mean(axis=0)) * np.sqrt(4.0 * np.pi * N * P)
    print("zero mean: per probe", np.max(z), "pooled", pooled.max())
    assert np.max(z) <= 4.0 and pooled.max() <= 4.0, (z, pooled)


@pytest.mark.parametrize("P,N", [(3, 256), (1, 4096)])
def test_hemisphere_sky_gives_its_closed_form_irradiance(P, N):
    a, b = ps.HEMI_A, ps.HEMI_B
    d, _ = ps.ray_set(P, N, SEED)
    L = ps.hemisphere(d)
    assert (L[..., 0] == a).sum() > N * P // 4 and (L[..., 0] == b).sum() > N * P // 4
    coeffs = ps.coefficients(ps.probe_sums(L, d, 2), N)
    want = np.pi * np.array([a, b, 0.5 * (a + b)])
    A = np.array([ps.A_BAND[0]] + [ps.A_BAND[1]] * 3 + [ps.A_BAND[2]] * 5, np.float64)
    worst = 0.0
    for i, n in enumerate(AXES):
        E = ps.irradiance(coeffs, np.tile(n, (P, 1)))
        Yn = ps.basis(n[None], 2).astype(np.float64)[0]
        for p in range(P):
            # the estimator is the mean of v_s = 4 pi L_s sum_k A_k Y_k(n) Y_k(d_s): its standard error from the samples
            v = 4.0 * np.pi * L[:, p, 0].astype(np.float64) * (ps.basis(d[:, p], 2).astype(np.float64) @ (A * Yn))
            se = v.std(ddof=1) / np.sqrt(N)
            assert abs(v.mean() - E[p, 0]) <= 1e-4 * abs(want[i])        # the fp32 sums are that estimator
            worst = max(worst, abs(float(E[p, 0]) - want[i]) / se)
            assert np.array_equal(E[p, 0], E[p, 1]) and np.array_equal(E[p, 0], E[p, 2])
    print("hemisphere: worst deviation in standard errors", worst)
    assert worst <= 4.0


def test_constant_sky():
    N, c = 4096, np.array([0.75, 1.5, 0.1], F)
    d, _ = ps.ray_set(1, N, SEED)
    L = np.broadcast_to(c, d.shape).astype(F)
    for order in (0, 2):
        coeffs = ps.coefficients(ps.probe_sums(L, d, order), N)
        want0 = c.astype(np.float64) * 2.0 * np.sqrt(np.pi)
        assert np.abs(coeffs[0, 0] / want0 - 1.0).max() <= N * 2.0 ** -24
        normals = np.array([[0, 1, 0], [0.6, 0.0, -0.8], [-0.57735027, 0.57735027, 0.57735027]], F)
        E = ps.irradiance(np.tile(coeffs, (3, 1, 1)), normals).astype(np.float64)
        if order == 0:          # the constant term alone: pi c whatever the normal
            assert np.abs(E / (np.pi * c) - 1.0).max() <= N * 2.0 ** -24 + 4 * 2.0 ** -24
        else:                   # the higher bands carry noise of zero mean: pi c within 4 standard errors
            A = np.array([ps.A_BAND[0]] + [ps.A_BAND[1]] * 3 + [ps.A_BAND[2]] * 5, np.float64)
            Yd = ps.basis(d[:, 0], 2).astype(np.float64)
            for i, n in enumerate(normals):
                v = 4.0 * np.pi * (Yd @ (A * ps.basis(n[None], 2).astype(np.float64)[0]))
                se = v.std(ddof=1) / np.sqrt(N)
                assert (np.abs(E[i] / c - np.pi) <= 4.0 * se).all(), (i, E[i] / c, se)


def test_lower_order_is_a_prefix_and_sums_are_ordered():
    d, _ = ps.ray_set(3, 5, SEED, first_sample=2)
    L = np.random.default_rng(1).uniform(0.0, 2.0, d.shape).astype(F)
    full = ps.probe_sums(L, d, 2)
    assert np.array_equal(ps.probe_sums(L, d, 0), full[:, :1]) and np.array_equal(ps.probe_sums(L, d, 1), full[:, :4])
    a, b = ps.probe_sums(L[:2], d[:2], 2), ps.sums(np.stack([ps.project(L[s], d[s], 2) for s in range(2, 5)]))
    chunked = a
    for s in range(2, 5):
        chunked = (chunked + ps.project(L[s], d[s], 2)).astype(F)
    assert np.array_equal(chunked, full) and b.shape == full.shape      # adding a chunk onto the first one is the whole sum
    one = ps.rays(np.zeros((3, 3), F), 4, SEED)
    assert np.array_equal(one["d"], d[2]) and np.array_equal(one["rng_state"], ps.ray_set(3, 5, SEED, 2)[1][2])

"""CPU tests of the replay of clustered light selection (tests/light_cluster_replay.py) itself, on host-only contexts:

  * over 2^20 keys at a handful of fixed vertices the cluster frequencies follow P_c binomially (|z| <= 5), and inside the
    chosen cluster the member frequencies follow pmf_in;
  * each of the two wrong estimators (dividing by phi_c instead of P_c; the weight of a hit light from the power pmf) is told
    apart from the right one: more than 1 % of the stable pixel samples move by more than 10x their tolerance;
  * the reference variance ratio: on NEAR_FAR (mode nee, depth 2, 96 x 64, 64 samples in 8 seed groups) the per-pixel
    variance of the ground pixels under clustered selection over that under power selection, R_ref, with the standard error
    se_ref over the seed groups: R_ref + 4 se_ref < 1.  (Measured: R_ref = 0.423, se_ref = 0.007.)"""
import numpy as np
import pytest

import light_cluster_replay as lcr
import mesh_light_replay as mr
from util import orc, prt

TWO24 = float(1 << 24)


def _tables(scene, K):
    r = prt.HipWavefrontRenderer(device=-1)
    r.set_light_sources("all")
    r.set_light_selection("clustered", K)
    r.set_scene_host_only(scene)
    return lcr.read_tables(r)


@pytest.fixture(scope="module")
def bunny():
    c = mr.case("bunny_light", 160, 120)
    return dict(c, osc=orc.OracleScene(c["scene"].desc()), tables=_tables(c["scene"], 8))


def test_cluster_and_member_frequencies_follow_their_probabilities(bunny):
    t = bunny["tables"]
    ls = lcr.light_set(bunny["scene"], t)
    n = 1 << 20
    keys = np.arange(n, dtype=np.uint64).astype(np.uint32)
    pts = np.array([[0.0, -1.0, 0.0], [3.0, -1.0, 2.0], [-2.0, 0.2, 1.4], [0.1, 0.5, 0.0], [50.0, 20.0, -30.0]], np.float32)
    worst = 0.0
    for x in pts:
        X = np.tile(x, (n, 1))
        li, cl, P, pin, M = lcr.select(ls, X, keys)
        Pc = np.diff(np.concatenate([[0.0], M[0].astype(np.float64)])) / TWO24
        assert abs(Pc.sum() - 1.0) == 0.0
        cnt = np.bincount(cl, minlength=ls.K)
        assert np.all(cnt[Pc == 0] == 0)
        var = n * Pc * (1 - Pc)
        z = (cnt - n * Pc)[var > 0] / np.sqrt(var[var > 0])
        worst = max(worst, float(np.abs(z).max()))
        assert np.abs(z).max() <= 5.0, (x, z)
        # inside the most likely cluster: the 8 members with the largest pmf_in
        c = int(np.argmax(Pc))
        rows = cl == c
        mem = ls.members[c]
        top = mem[np.argsort(ls.inner[mem])[-8:]]
        m = int(rows.sum())
        for i in top:
            p = ls.inner[i]
            if p == 1.0:     # a cluster of one light
                assert np.all(li[rows] == i)
                continue
            z = ((li[rows] == i).sum() - m * p) / np.sqrt(m * p * (1 - p))
            assert abs(z) <= 5.0, (x, i, z)
        assert np.all(P == Pc[cl]) and np.all(pin == ls.inner[li])
    print("largest |z| of a cluster count:", worst)


# wrong estimator -> mode on which it must show (the weight of a hit light matters only where the weights are not 0 / 1)
SEPARATES = {"phi_for_P": "nee", "wb_power_pmf": "mis"}


@pytest.mark.parametrize("wrong", lcr.WRONG)
def test_wrong_estimators_are_told_apart(bunny, wrong):
    mode = SEPARATES[wrong]
    right = lcr.replay_case(bunny, mode, bunny["tables"], osc=bunny["osc"])
    other = lcr.replay_case(bunny, mode, bunny["tables"], wrong=wrong, stability=False, osc=bunny["osc"])
    assert mr.unstable_share(right) <= mr.MAX_UNSTABLE
    share = mr.separated_share(right, other, 10.0)
    print(wrong, mode, share)
    assert share > 0.01, (wrong, mode, share)


def test_reference_variance_ratio_on_near_far():
    c = lcr.near_far()
    t = _tables(c["scene"], 2)
    assert list(t["n_members"]) == [80, 80]
    gp = lcr.ground_pixels(c)
    assert len(gp) > 0.5 * c["W"] * c["H"]
    S = 64
    rp = mr.replay_case(c, "nee", samples=range(S), stability=False, pix=gp)
    rc = lcr.replay_case(c, "nee", t, samples=range(S), stability=False, pix=gp)
    yp = lcr.luminance(rp.value).reshape(S, len(gp)).T
    yc = lcr.luminance(rc.value).reshape(S, len(gp)).T
    # both selections estimate the same image
    se = np.sqrt((yp.var(axis=1, ddof=1) + yc.var(axis=1, ddof=1)) / S)
    k = se > 0
    Z = (yp.mean(1) - yc.mean(1))[k].sum() / np.sqrt((se[k] ** 2).sum())
    R_ref, se_ref, per_group = lcr.variance_ratio(yp, yc, 8)
    print(dict(R_ref=R_ref, se_ref=se_ref, per_group=per_group.round(3).tolist(), Z=float(Z)))
    assert abs(Z) <= 5.0
    assert R_ref + 4 * se_ref < 1

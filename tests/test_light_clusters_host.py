"""CPU-side tests of clustered light selection (include/prt.h "Clustered light selection", prt_set_light_selection): the
cluster tables a host-only context builds, read back and held to the contract's invariants (not to the grouping algorithm):
partition, boxes, sums, the inner thresholds against the written rule in numpy float64, cluster counts, separation of
disjoint meshes, determinism, clone, argument checks and lifetime.  The device half: tests/test_gpu_light_clusters.py."""
import ctypes as C

import numpy as np
import pytest

import light_cluster_replay as lcr
import mesh_light_replay as mlr
from test_mesh_lights_host import degenerate_scene, mixed_scene
from util import prt

capi = prt.capi
PRT_ERR_INVALID = 1
TWO32 = 4294967296.0


def _host(scene, selection="clustered", max_clusters=32, sources="all"):
    r = prt.HipWavefrontRenderer(device=-1)
    if sources is not None:
        r.set_light_sources(sources)
    if selection is not None:
        r.set_light_selection(selection, max_clusters)
    r.set_scene_host_only(scene)
    return r


def light_geometry(scene):
    """Per light of the "all" set, float64: (points [n, k, 3] whose hull is the light (triangle vertices / quad corners; a
    sphere: the corners of c +- R), power [n]) from mesh_light_replay's restatement of the set."""
    ls = mlr.MeshLightSet(scene, "all")
    pts = []
    for i in range(ls.n):
        c, u, v = ls.c[i], ls.u[i], ls.v[i]
        if ls.kind[i] == 2:
            pts.append(np.array([c, c + u, c + v]))
        elif ls.kind[i] == 1:
            pts.append(np.array([c + a * u / 2 + b * v / 2 for a in (-1, 1) for b in (-1, 1)]))
        else:
            pts.append(np.array([c - ls.R[i], c + ls.R[i]]))
    power = np.where(ls.kind == 0, ls.area, 2.0 * ls.area) * ls.Le.mean(1)   # (sphere: its whole area; quad, triangle: both faces)
    return ls, pts, power


def check_tables(r, scene, max_clusters):
    info = r.light_cluster_info()
    t = lcr.read_tables(r)
    K = info.n_clusters
    ls, pts, power = light_geometry(scene)
    n = ls.n
    cl, inner = t["cluster"].astype(np.int64), t["inner_width"].astype(np.uint64)
    assert info.max_clusters == max_clusters and 1 <= K <= max_clusters and len(t["phi"]) == K
    # partition: every light in exactly one cluster, none empty
    assert len(cl) == n == len(r.light_info()[0])
    assert cl.min() >= 0 and cl.max() < K
    counts = np.bincount(cl, minlength=K)
    assert np.all(counts > 0) and np.array_equal(counts, t["n_members"].astype(np.int64))
    # boxes contain their members in float64; r2 is not below the squared half diagonal
    lo, hi = t["lo"].astype(np.float64), t["hi"].astype(np.float64)
    for i in range(n):
        assert np.all(pts[i] >= lo[cl[i]] - 0.0) and np.all(pts[i] <= hi[cl[i]] + 0.0), (i, pts[i], lo[cl[i]], hi[cl[i]])
    half2 = (((hi - lo) / 2.0) ** 2).sum(1)
    assert np.all(t["r2"].astype(np.float64) >= half2) and np.all(t["r2"] >= np.float32(1e-30))
    assert np.all(t["r2"].astype(np.float64) <= np.maximum(half2 * (1 + 2.0 ** -22), 1.1e-30))
    # sums: W_c is the sum of the members' global widths, they sum to 2^32, phi is its fp32 rounding
    width = r.light_intervals().astype(np.uint64)
    W = np.array([int(width[cl == c].sum()) for c in range(K)], np.uint64)
    assert np.array_equal(W, t["power_width"]) and int(W.sum()) == 1 << 32
    assert np.array_equal(t["phi"], (W.astype(np.float64) / TWO32).astype(np.float32))
    # inner widths: 2^32 per cluster, the written rule in float64 to within 2 units
    n_empty = 0
    for c in range(K):
        m = np.nonzero(cl == c)[0]
        assert int(inner[m].sum()) == 1 << 32
        S = np.cumsum(power[m])
        U = np.concatenate([[0.0], np.floor(S / S[-1] * TWO32 + 0.5)])
        assert np.all(np.abs(np.diff(U) - inner[m].astype(np.float64)) <= 2.0), (c, np.abs(np.diff(U) - inner[m].astype(np.float64)).max())
        n_empty += int((inner[m] == 0).sum())
    assert info.n_empty_inner == n_empty
    return t, cl


@pytest.mark.parametrize("max_clusters", (1, 2, 7, 32, 64))
def test_partition_boxes_and_sums_on_a_mixed_scene(max_clusters):
    sc = mixed_scene()    # a sphere and a quad light, an emissive bunny, an emissive placed copy
    r = _host(sc, max_clusters=max_clusters)
    t, cl = check_tables(r, sc, max_clusters)
    assert r.light_cluster_info().n_clusters == max_clusters          # thousands of lights spread in space: every split happens
    assert r.light_cluster_info().active == 1
    # the light set itself is what "power" reports: indices stay the global set's
    p = _host(sc, "power")
    assert np.array_equal(p.light_info()[0], r.light_info()[0]) and np.array_equal(p.light_intervals(), r.light_intervals())


def test_fewer_lights_than_clusters_and_degenerate_triangles():
    sc = degenerate_scene()       # two lights (faces 0 and 4); zero-area, coincident and tiny faces are not members
    r = _host(sc, max_clusters=64)
    t, cl = check_tables(r, sc, 64)
    assert r.light_cluster_info().n_clusters == 2 and list(t["n_members"]) == [1, 1]
    assert list(t["inner_width"]) == [1 << 32, 1 << 32]
    one = _host(sc, max_clusters=1)
    check_tables(one, sc, 1)
    assert one.light_cluster_info().n_clusters == 1
    # a scene without any light has no cluster
    sc2 = prt.Scene(preset=None)
    e = sc2.AddEmissive((2.0, 2.0, 2.0))
    v = np.array([[2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32)
    sc2.AddMesh(prt.Mesh(vertices=v, normals=np.tile(np.array([[0, 0, 1.0]], np.float32), (3, 1)), indices=np.array([[0, 1, 2]], np.uint32)), e)
    r2 = _host(sc2)
    assert r2.light_cluster_info().n_clusters == 0 and len(r2.light_clusters()["phi"]) == 0 and len(r2.light_cluster_members()[0]) == 0


def test_unsampled_count_adds_the_empty_inner_intervals_while_active():
    sc = mixed_scene()
    r = _host(sc, max_clusters=8)
    p = _host(sc, "power")
    assert r.light_stats().n_emitters_unsampled == p.light_stats().n_emitters_unsampled + r.light_cluster_info().n_empty_inner
    r.set_light_selection("power", 8)
    assert r.light_stats().n_emitters_unsampled == p.light_stats().n_emitters_unsampled


def test_two_disjoint_meshes_are_separated():
    c = lcr.near_far()
    for K in (2, 3, 64):
        r = _host(c["scene"], max_clusters=K)
        t, cl = check_tables(r, c["scene"], K)
        prim = r.light_info()[0].astype(np.int64)
        first = prim < 1 + 80             # the ground is primitive 0, then 80 + 80 triangles
        assert first.sum() == 80 and (~first).sum() == 80
        assert not set(cl[first]) & set(cl[~first]), K
    t = lcr.read_tables(_host(c["scene"], max_clusters=2))
    assert list(t["n_members"]) == [80, 80] and t["hi"][0][0] < 1.0 and t["lo"][1][0] > 399.0
    # unequal power and a separating plane off the longest axis
    sc = prt.Scene(preset=None)
    e1, e2 = sc.AddEmissive((1.0, 1.0, 1.0)), sc.AddEmissive((30.0, 30.0, 30.0))
    ico = prt.Mesh(prt.scenes.asset("icosahedron.ply"))
    v, nr, idx = ico.GetVertices(), ico.GetNormals(), ico.GetIndices()
    stretch = np.array([10.0, 1.0, 1.0], np.float32)
    sc.AddMesh(prt.Mesh(vertices=v * stretch, normals=nr, indices=idx), e1)
    sc.AddMesh(prt.Mesh(vertices=v * stretch + np.array([0.0, 5.0, 0.0], np.float32), normals=nr, indices=idx), e2)
    r = _host(sc, max_clusters=2)
    t, cl = check_tables(r, sc, 2)
    assert len(set(cl[:20])) == 1 and len(set(cl[20:])) == 1 and cl[0] != cl[20]


def test_two_compilations_agree_and_a_clone_equals_its_source():
    sc = mixed_scene()
    a, b = _host(sc, max_clusters=16), _host(sc, max_clusters=16)
    ta, tb = lcr.read_tables(a), lcr.read_tables(b)
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    # set after the scene: the same tables as set before it
    late = _host(sc, selection=None)
    assert late.light_cluster_info().max_clusters == 32 and late.light_cluster_info().mode == 0
    late.set_light_selection("clustered", 16)
    tl = lcr.read_tables(late)
    for k in ta:
        assert np.array_equal(ta[k], tl[k]), k
    dst = prt.HipWavefrontRenderer(device=-1)
    assert capi.lib().prt_clone_scene(dst._ctx, a._ctx) == 0
    td = lcr.read_tables(dst)
    for k in ta:
        assert np.array_equal(ta[k], td[k]), k
    i = dst.light_cluster_info()
    assert (i.mode, i.active, i.n_clusters, i.max_clusters) == (1, 1, 16, 16)


def test_bad_arguments_and_lifetime():
    L = capi.lib()
    sc = mixed_scene()
    r = _host(sc, max_clusters=5)
    before = lcr.read_tables(r)
    for mode, k in ((2, 8), (7, 0), (0xFFFFFFFF, 1), (1, 65), (0, 65), (1, 0xFFFFFFFF)):
        assert L.prt_set_light_selection(r._ctx, C.byref(capi.PrtLightSelection(mode, k))) == PRT_ERR_INVALID, (mode, k)
        assert "light selection" in L.prt_last_error(r._ctx).decode()
        i = r.light_cluster_info()
        assert (i.mode, i.max_clusters, i.n_clusters) == (1, 5, 5)
    assert L.prt_set_light_selection(None, None) == PRT_ERR_INVALID
    assert L.prt_light_cluster_info(None, None) == PRT_ERR_INVALID and L.prt_light_cluster_info(r._ctx, None) == PRT_ERR_INVALID
    assert L.prt_light_clusters(None, 0, None, None, None, None, None, None, None) == PRT_ERR_INVALID
    assert L.prt_light_cluster_members(None, 0, None, None, None) == PRT_ERR_INVALID
    with pytest.raises(KeyError):
        r.set_light_selection("tree")
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.light_cluster_pmf([[0.0, 0.0, 0.0]])
    # the setting survives prt_set_scene
    r.set_scene_host_only(degenerate_scene())
    i = r.light_cluster_info()
    assert (i.mode, i.active, i.max_clusters, i.n_clusters) == (1, 1, 5, 2)
    r.set_scene_host_only(sc)
    after = lcr.read_tables(r)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    # 0 clusters = the default of 32; NULL = power, 32
    r.set_light_selection("clustered", 0)
    assert r.light_cluster_info().max_clusters == 32 and r.light_cluster_info().n_clusters == 32
    assert L.prt_set_light_selection(r._ctx, None) == 0
    i = r.light_cluster_info()
    assert (i.mode, i.active, i.max_clusters) == (0, 0, 32)
    # before any scene, and without one
    ctx = C.c_void_p()
    assert L.prt_create(-1, C.byref(ctx)) == 0
    try:
        assert L.prt_set_light_selection(ctx, C.byref(capi.PrtLightSelection(1, 9))) == 0
        info = capi.PrtLightClusterInfo()
        assert L.prt_light_cluster_info(ctx, C.byref(info)) == 0 and (info.mode, info.active, info.n_clusters, info.max_clusters) == (1, 0, 0, 9)
        assert L.prt_light_clusters(ctx, 0, None, None, None, None, None, None, None) == PRT_ERR_INVALID
        assert L.prt_light_cluster_members(ctx, 0, None, None, None) == PRT_ERR_INVALID
    finally:
        L.prt_destroy(ctx)


def test_inactive_under_the_default_mask():
    sc = mixed_scene()
    r = _host(sc, max_clusters=8, sources=None)
    i = r.light_cluster_info()
    assert (i.mode, i.active, i.n_clusters) == (1, 0, 8)          # recorded, built with the scene, inactive
    a = _host(sc, "power", sources=None)
    assert np.array_equal(r.light_info()[0], a.light_info()[0]) and np.array_equal(r.light_info()[1], a.light_info()[1])
    assert r.light_stats().n_emitters_unsampled == a.light_stats().n_emitters_unsampled
    r.set_light_sources("all")
    assert r.light_cluster_info().active == 1
    r.set_light_sources("analytic")
    assert r.light_cluster_info().active == 0


def test_header_and_bindings_agree():
    src = open(prt.capi.__file__.replace("parallelraytracing_amd/capi.py", "include/prt.h")).read()
    for name in ("prt_set_light_selection", "prt_group_set_light_selection", "prt_light_cluster_info", "prt_light_clusters",
                 "prt_light_cluster_members", "prt_light_cluster_pmf"):
        assert name + "(" in src and name in capi.SIGNATURES
        assert hasattr(capi.lib(), name)
    assert "PRT_LIGHT_SELECTION_POWER = 0, PRT_LIGHT_SELECTION_CLUSTERED = 1" in src
    assert "#define PRT_LIGHT_MAX_CLUSTERS 64u" in src and capi.LIGHT_MAX_CLUSTERS == 64
    assert capi.LIGHT_SELECTIONS == {"power": 0, "clustered": 1}
    assert C.sizeof(capi.PrtLightSelection) == 8 and C.sizeof(capi.PrtLightClusterInfo) == 20
    assert 'Clustered light selection' in src

"""CPU-side tests of the environment light (include/prt.h "Environment light", prt_set_environment): the tables a host-only
context builds against the float64 restatement (tests/environment_replay.py EnvMap) exactly, argument validation, the factor
(2^32 - T_e) / 2^32 on the other lights' pmf, the PFM reader against the writer in both byte orders, and the table builder and
the reader under AddressSanitizer + UBSan (tests/sanitize_environment.cpp)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import environment_replay as er
import mesh_light_replay as mr
from util import prt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO32 = 1 << 32


def _host(scene=None, sources=None):
    r = prt.HipWavefrontRenderer(device=-1)
    if sources:
        r.set_light_sources(sources)
    if scene is not None:
        r.set_scene_host_only(scene)
    return r


@pytest.mark.parametrize("name", er.MAPS + ("constant16x8",))
def test_intervals_equal_the_float64_tables_exactly(name):
    rgb = np.full((8, 16, 3), 0.25, np.float32) if name == "constant16x8" else er.named_map(name)
    env = er.EnvMap(rgb)
    r = _host()
    r.set_environment(rgb, 0.5)
    info = r.environment_info()
    assert (info.is_set, info.width, info.height) == (1, env.W, env.H)
    row, col = r.environment_intervals()
    assert np.array_equal(row, env.row_width.astype(np.uint64))
    assert np.array_equal(col, env.col_width.astype(np.uint64))
    assert int(row.sum()) == TWO32
    assert all(int(col[i].sum()) == TWO32 for i in range(env.H) if row[i])
    assert info.n_sampled == env.n_sampled and env.n_sampled > 0
    # the pmf is a probability: exactly 1 in units of 2^-64
    assert sum(int(row[i]) * int(c) for i in range(env.H) for c in col[i]) == 1 << 64
    assert info.t_env == TWO32          # no scene: an empty light set
    if name == "blackrows":
        assert row[0] == 0 and row[7] == 0 and col[3, 0] == 0 and col[3, 15] == 0 and col[4, 0] == 0 and col[4, 1] > 0


def test_black_map_has_no_distribution_and_none_goes_back_to_the_sky():
    r = _host()
    r.set_environment(np.zeros((4, 8, 3), np.float32), 0.5)
    info = r.environment_info()
    assert info.is_set == 1 and info.n_sampled == 0 and info.t_env == 0
    with pytest.raises(prt.PrtError):
        r.environment_intervals()
    r.set_environment(None)
    assert r.environment_info().is_set == 0
    with pytest.raises(prt.PrtError):
        r.environment_intervals()
    with pytest.raises(prt.PrtError):       # a compute entry point on a host-only context
        r.set_environment(er.named_map("5x3"))
        r.environment_eval(np.array([[0.0, 1.0, 0.0]], np.float32))


def test_invalid_arguments_leave_the_environment_in_place():
    r = _host()
    good = er.named_map("5x3")
    r.set_environment(good, 0.25)
    row0, col0 = r.environment_intervals()
    L, C = prt.capi.lib(), prt.capi.C
    fp = C.POINTER(C.c_float)

    def refused(rgb, w, h, share):
        a = np.ascontiguousarray(rgb, np.float32)
        e = prt.capi.PrtEnvironment(a.ctypes.data_as(fp) if a.size else None, w, h, share)
        assert L.prt_set_environment(r._ctx, C.byref(e)) == 1       # PRT_ERR_INVALID
        assert L.prt_last_error(r._ctx)
        info = r.environment_info()
        assert (info.width, info.height, info.light_share) == (5, 3, 0.25)
        row, col = r.environment_intervals()
        assert np.array_equal(row, row0) and np.array_equal(col, col0)

    one = np.ones((2, 4, 3), np.float32)
    refused(one, 0, 2, 0.5)
    refused(one, 4, 0, 0.5)
    refused(one, 16385, 1, 0.5)
    refused(one, 1, 8193, 0.5)
    refused(np.zeros(0, np.float32), 4, 2, 0.5)
    for share in (-0.01, 1.01, float("nan"), float("inf")):
        refused(one, 4, 2, share)
    for bad in (-1e-20, float("nan"), float("inf"), -float("inf")):
        b = one.copy()
        b[1, 2, 1] = bad
        refused(b, 4, 2, 0.5)
    r.set_environment(np.ones((8192 // 512, 16384 // 512, 3), np.float32), 1.0)     # (the limits themselves are sizes, not tested at full size)
    assert r.environment_info().width == 32


def test_threshold_follows_share_light_set_and_scene():
    r = _host()
    r.set_environment(er.named_map("sun"), 0.3)
    assert r.environment_info().t_env == TWO32                  # before any scene: no lights
    r.set_scene_host_only(prt.Scene("DEFAULT"))                  # the environment stays across prt_set_scene
    info = r.environment_info()
    assert info.is_set == 1 and info.t_env == int(np.floor(float(np.float32(0.3)) * TWO32 + 0.5))
    sc = prt.Scene(preset=None)
    sc.AddQuad(20.0, 20.0, sc.AddLambertian((0.5, 0.5, 0.5)))
    r.set_scene_host_only(sc)
    assert r.environment_info().t_env == TWO32                  # a scene without lights
    r.set_environment(er.named_map("sun"), 0.0)
    assert r.environment_info().t_env == 0
    r.set_environment(er.named_map("sun"), 1.0)
    r.set_scene_host_only(prt.Scene("DEFAULT"))
    assert r.environment_info().t_env == TWO32


@pytest.mark.parametrize("sources", ["analytic", "all"])
def test_light_pmf_carries_the_factor(sources):
    c = mr.case("placed", 64, 48)
    sc = c["scene"]
    r = _host(sc, sources)
    prim0, pmf0 = r.light_info()
    w0 = r.light_intervals() if sources == "all" else None
    ls = mr.MeshLightSet(sc, sources)
    assert ls.n == len(prim0) > 0
    for share in (0.5, 0.3, 1.0, 0.0):
        r.set_environment(er.named_map("sun"), share)
        te = r.environment_info().t_env
        assert te == int(np.floor(float(np.float32(share)) * TWO32 + 0.5))
        prim, pmf = r.light_info()
        assert np.array_equal(prim, prim0)
        want = (ls.pmf * ((TWO32 - te) / TWO32)).astype(np.float32)      # in double, rounded once
        if sources == "all":
            assert np.array_equal(pmf, want)
            w = r.light_intervals()
            if te:
                assert [int(x) for x in w] == [int(x) * (TWO32 - te) for x in w0]
            else:
                assert np.array_equal(w, w0)
        else:
            np.testing.assert_allclose(pmf, want, rtol=2e-7)            # (the analytic pmf is a quotient of sums in double)
        if te == 0:
            assert np.array_equal(pmf, pmf0)
    r.set_environment(None)
    assert np.array_equal(r.light_info()[1], pmf0)


def test_clone_copies_the_environment():
    L = prt.capi.lib()
    a, b = _host(prt.Scene("DEFAULT")), _host()
    a.set_environment(er.named_map("blackrows"), 0.75)
    assert L.prt_clone_scene(b._ctx, a._ctx) == 0
    ia, ib = a.environment_info(), b.environment_info()
    assert (ib.is_set, ib.width, ib.height, ib.n_sampled, ib.t_env, ib.light_share) == \
           (ia.is_set, ia.width, ia.height, ia.n_sampled, ia.t_env, ia.light_share)
    for x, y in zip(a.environment_intervals(), b.environment_intervals()):
        assert np.array_equal(x, y)


def test_pfm_round_trip_in_both_byte_orders(tmp_path):
    rng = np.random.default_rng(3)
    img = np.exp(rng.normal(0, 2, (5, 7, 3))).astype(np.float32)
    p = str(tmp_path / "a.pfm")
    prt.write_pfm(p, img)
    assert np.array_equal(prt.read_pfm(p).view(np.uint32), img.view(np.uint32))
    raw = open(p, "rb").read()
    assert raw.startswith(b"PF\n7 5\n-1.0\n")
    body = raw[len(b"PF\n7 5\n-1.0\n"):]
    be = struct.pack(">%df" % (len(body) // 4), *struct.unpack("<%df" % (len(body) // 4), body))
    q = str(tmp_path / "b.pfm")
    open(q, "wb").write(b"PF\n7 5\n1.0\n" + be)
    assert np.array_equal(prt.read_pfm(q).view(np.uint32), img.view(np.uint32))
    # rows are stored bottom to top: the file's first row is the image's last
    assert np.array_equal(np.frombuffer(body[:7 * 12], "<f4"), img[4].ravel())
    for bad in (b"Pf\n7 5\n-1.0\n" + body, b"PF\n7 5\n-1.0\n" + body[:-1], b"PF\n7 5\n0.0\n" + body, b"PF\n7 0\n-1.0\n", b""):
        open(q, "wb").write(bad)
        with pytest.raises(prt.PrtError):
            prt.read_pfm(q)
    with pytest.raises(prt.PrtError):
        prt.read_pfm(str(tmp_path / "missing.pfm"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tables_and_pfm_reader_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_environment")
    csrc = os.path.join(ROOT, "parallelraytracing_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "sanitize_environment.cpp"),
           os.path.join(csrc, "prt_host.cpp"), os.path.join(csrc, "bvh.cpp"), os.path.join(csrc, "prt_scene.cpp"), "-pthread",
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path), "300"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "UNEXPECTED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr

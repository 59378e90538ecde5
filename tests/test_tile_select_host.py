"""CPU-side tests of prt_tile_select (include/prt.h): every refusal is decided on the host before the device is looked at, so a
host-only context refuses the same way; valid arguments reach the device check and fail there (no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

from util import prt

capi = prt.capi
NAN = float("nan")
INVALID, NO_DEVICE = 1, 2  # PRT_ERR_INVALID, PRT_ERR_NO_DEVICE
W, H = 44, 28              # 6 x 4 = 24 tiles
_fp, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def _host(rank=0, world=1, film=True):
    r = prt.HipWavefrontRenderer(device=-1, rank=rank, world_size=world)
    if film:
        r.set_film(prt.Film(W, H))
    return r


def _call(r, n_prev=24, prev=None, thr=0.1, floor=0.01, null=None):
    img = np.zeros((H, W), np.float32)
    lst = np.zeros(64, np.uint32)
    counts = np.zeros(2, np.uint32)
    args = dict(n=img.ctypes.data_as(_fp), sum_y=img.ctypes.data_as(_fp), sum_y2=img.ctypes.data_as(_fp),
                list=lst.ctypes.data_as(_u32p), counts=counts.ctypes.data_as(_u32p))
    if null:
        args[null] = None
    if prev is not None:
        prev = np.asarray(prev, np.uint32)
    p_prev = None if prev is None else prev.ctypes.data_as(_u32p)
    rc = capi.lib().prt_tile_select(r._ctx, args["n"], args["sum_y"], args["sum_y2"], p_prev, n_prev, thr, floor, args["list"],
                                    args["counts"])
    return rc, capi.lib().prt_last_error(r._ctx).decode()


REFUSALS = [
    ("null n", dict(null="n")), ("null sum_y", dict(null="sum_y")), ("null sum_y2", dict(null="sum_y2")),
    ("null list", dict(null="list")), ("null counts", dict(null="counts")),
    ("n_prev above the tile count", dict(n_prev=25)), ("n_prev above, with prev", dict(n_prev=25, prev=[0] * 25)),
    ("prev entry out of range", dict(n_prev=3, prev=[0, 24, 1])), ("last prev entry out of range", dict(n_prev=24, prev=list(range(1, 25)))),
    ("prev entry far out of range", dict(n_prev=1, prev=[0xFFFFFFFF])),
    ("nan threshold", dict(thr=NAN)), ("negative threshold", dict(thr=-0.1)), ("nan floor", dict(floor=NAN)),
    ("negative floor", dict(floor=-1e-3)), ("both zero", dict(thr=0.0, floor=0.0)),
]


@pytest.mark.parametrize("what,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_on_a_host_only_context(what, kw):
    rc, msg = _call(_host(), **kw)
    assert rc == INVALID and msg, what


def test_valid_arguments_reach_the_device_check():
    r = _host()
    for kw in (dict(), dict(n_prev=0), dict(n_prev=24, prev=list(range(24))), dict(n_prev=3, prev=[23, 0, 7]), dict(thr=0.0),
               dict(floor=0.0), dict(thr=float("inf"))):
        rc, msg = _call(r, **kw)
        assert rc == NO_DEVICE and "no HIP device" in msg, kw
    assert capi.lib().prt_tile_select(None, None, None, None, None, 0, 0.1, 0.01, None, None) == INVALID
    rc, msg = _call(_host(film=False))
    assert rc == INVALID and "prt_set_film" in msg


def test_the_tile_count_is_the_ranks_own():
    """24 tiles over 5 ranks: ranks 0 .. 3 own 5 and rank 4 owns 4; 30 ranks: ranks 24 .. 29 own none."""
    for rank, local in ((0, 5), (3, 5), (4, 4)):
        r = _host(rank, 5)
        assert r.local_tile_count() == local
        assert _call(r, n_prev=local)[0] == NO_DEVICE and _call(r, n_prev=local + 1)[0] == INVALID
        assert _call(r, n_prev=1, prev=[local - 1])[0] == NO_DEVICE and _call(r, n_prev=1, prev=[local])[0] == INVALID
    r = _host(29, 30)
    assert r.local_tile_count() == 0
    assert _call(r, n_prev=0)[0] == NO_DEVICE and _call(r, n_prev=1)[0] == INVALID


def test_python_layer():
    r = _host()
    img = np.zeros((H, W), np.float32)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.tile_select(img, img, img, 0.1)
    with pytest.raises(prt.PrtError, match="no HIP device"):
        r.tile_select(img, img, img, 0.1, 0.01, prev=[3, 1])
    with pytest.raises(prt.PrtError, match="both 0"):
        r.tile_select(img, img, img, 0.0, 0.0)
    with pytest.raises(prt.PrtError, match="local tiles"):
        r.tile_select(img, img, img, 0.1, 0.01, prev=[24])
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        r.tile_select(img[:-1], img, img, 0.1)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        r.tile_select(img, img.reshape(-1), img, 0.1)
    assert "prt_tile_select" in capi.SIGNATURES and capi.lib().prt_tile_select

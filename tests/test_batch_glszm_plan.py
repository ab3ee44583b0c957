"""Host half of the batched small-ROI GLSZM (prad_batch_glszm_dev, prad_batch_glszm_fill_dev and the route choice of the
Python layer): the cap, the argument checks and the declined domain -- all answered before any device work, so they come back
on a machine without a GPU -- and the looped route when no device is visible.  No compute calls here (no GPU in this tier)."""
import ctypes as C

import numpy as np
import pytest

MAX_VOX = (160 * 1024 - 256) // 3          # PRAD_BATCH_GLSZM_MAX_VOX (csrc/kernels_batch_glszm.h): misc + 1 + 2 bytes per voxel
IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_longlong)


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


def test_cap(lib):
    assert lib.prad_batch_glszm_max_vox() == MAX_VOX == 54528 == 24 * 32 * 71 == 213 * 256
    assert MAX_VOX % 16 == 0 and 37 ** 3 <= MAX_VOX < 38 ** 3 and MAX_VOX < 1 << 16


def _label(lib, sizes, B, Ng, null=None):
    """the raw call with host buffers standing in for the device pointers: every case here is answered before they are used"""
    sizes = np.ascontiguousarray(sizes, dtype=np.intc)
    n = max(int(np.abs(sizes.astype(np.int64)).prod(1).sum()), 1) if len(sizes) else 1
    n = min(n, 1 << 20)
    bufs = {"levels": np.zeros(n, np.int32), "mask": np.zeros(n, np.uint8), "zones": np.full(2 * n, -7, np.int32),
            "summary": np.full(3 * max(B, 1), -7, np.int32), "status": np.full(max(B, 1), -7, np.int32)}
    off = np.zeros(max(B, 1), dtype=np.int64)
    ptr = {k: (None if k == null else C.c_void_p(v.ctypes.data)) for k, v in bufs.items()}
    rc = lib.prad_batch_glszm_dev(ptr["levels"], ptr["mask"], None if null == "sizes" else sizes.ctypes.data_as(IP),
                                  None if null == "off" else off.ctypes.data_as(LP), B, Ng, ptr["zones"], ptr["summary"],
                                  ptr["status"], None)
    for k in ("zones", "summary", "status"):
        assert (bufs[k] == -7).all(), "%s was written" % k
    return rc


def test_argument_errors_need_no_device(lib):
    from pyradiomics_amd import _lib
    ok = [(2, 3, 4), (1, 1, 1)]
    assert _label(lib, ok, -1, 8) == _lib.PRAD_E_ARG
    assert _label(lib, ok, 2, 0) == _lib.PRAD_E_ARG and "Ng=0" in _lib.last_error()
    assert _label(lib, [(2, 3, 4), (1, 0, 1)], 2, 8) == _lib.PRAD_E_ARG and "ROI 1" in _lib.last_error()
    assert _label(lib, [(2, -3, 4)], 1, 8) == _lib.PRAD_E_ARG
    for null in ("sizes", "levels", "mask", "off", "zones", "summary", "status"):
        assert _label(lib, ok, 2, 8, null=null) == _lib.PRAD_E_ARG, null
    assert _label(lib, ok, 0, 8) == _lib.PRAD_OK          # an empty batch: nothing to do


def test_domain_is_declined_without_a_device(lib):
    from pyradiomics_amd import _lib
    assert _label(lib, [(2, 3, 4)], 1, 65) == _lib.PRAD_E_UNSUPPORTED and "Ng=65" in _lib.last_error()
    assert _label(lib, [(2, 3, 4), (1, 1, MAX_VOX + 1)], 2, 8) == _lib.PRAD_E_UNSUPPORTED and "ROI 1" in _lib.last_error()
    assert _label(lib, [(38, 38, 38)], 1, 8) == _lib.PRAD_E_UNSUPPORTED
    # an argument error wins over the domain
    assert _label(lib, [(1, 1, MAX_VOX + 1), (0, 1, 1)], 2, 8) == _lib.PRAD_E_ARG


def test_fill_argument_errors_need_no_device(lib):
    from pyradiomics_amd import _lib
    zones = np.zeros(64, np.int32)
    out = np.full(64, -7.0)
    sizes_out = np.full(8, -7, np.int32)
    off = np.zeros(1, np.int64)

    def fill(summary, B=1, Ng=4, compact=1, out_p=out, sizes_p=sizes_out, out_off=0):
        sm = np.array(summary, dtype=np.intc)
        oo, so = np.array([out_off], np.int64), np.zeros(1, np.int64)
        return lib.prad_batch_glszm_fill_dev(C.c_void_p(zones.ctypes.data), sm.ctypes.data_as(IP), off.ctypes.data_as(LP), B, Ng,
                                             compact, None if out_p is None else C.c_void_p(out_p.ctypes.data),
                                             oo.ctypes.data_as(LP), None if sizes_p is None else C.c_void_p(sizes_p.ctypes.data),
                                             so.ctypes.data_as(LP), None)
    assert fill([2, 3, 2], B=-1) == _lib.PRAD_E_ARG
    assert fill([2, 3, 2], Ng=0) == _lib.PRAD_E_ARG
    assert fill([2, 3, 2], out_p=None) == _lib.PRAD_E_ARG
    assert fill([2, 3, 2], sizes_p=None) == _lib.PRAD_E_ARG          # the compact layout needs the sizes buffer
    assert fill([2, 3, 2], out_off=-8) == _lib.PRAD_E_ARG
    assert fill([-1, 3, 2]) == _lib.PRAD_E_ARG and fill([2, MAX_VOX + 1, 2]) == _lib.PRAD_E_ARG
    assert fill([2, 3, 4]) == _lib.PRAD_E_ARG                         # more distinct sizes than the largest size
    assert fill([2, 3, 2], Ng=65) == _lib.PRAD_E_UNSUPPORTED
    assert fill([2, 3, 2], B=0) == _lib.PRAD_OK
    assert (out == -7.0).all() and (sizes_out == -7).all()


def test_looped_route_without_device(lib):
    """no device: the batch goes to the single calls, which fail loudly (never compute on the host)"""
    if lib.prad_device_count() > 0:
        pytest.skip("a GPU is visible")
    from pyradiomics_amd import cmatrices as cm
    cm._set_batch_route("none")
    imgs = [np.ones(s, int) for s in [(1, 1, 9), (2, 2, 2)]]
    with pytest.raises(RuntimeError, match="no HIP device"):
        cm.calculate_glszm_batch(imgs, [i > 0 for i in imgs], 2)
    assert cm.last_batch_route() == "looped"
    # a batch of 1 x 1 x 1 boxes needs no single call at all: the looped route answers it on its own
    boxes = [np.full((1, 1, 1), 2), np.full((1, 1, 1), 2), np.full((1, 1, 1), 4)]
    msks = [np.ones((1, 1, 1), bool), np.zeros((1, 1, 1), bool), np.ones((1, 1, 1), bool)]
    dense, status = cm.calculate_glszm_batch(boxes, msks, 3)
    assert status == [1, 1, 0] and cm.last_batch_route() == "looped"
    assert [d.tolist() for d in dense] == [[[0], [1], [0]], [[0], [0], [0]], [[0], [0], [0]]]
    comp, status = cm.calculate_glszm_batch(boxes, msks, 3, compact=True)
    assert status == [1, 1, 0]
    assert comp[0][0].tolist() == [[0], [1], [0]] and comp[0][1].tolist() == [1]
    assert comp[1][0].shape == (3, 0) and comp[1][1].tolist() == [] and comp[2][0].shape == (3, 0)
    with pytest.raises(ValueError):
        cm.calculate_glszm_batch([np.ones((2, 2), int)], [np.ones((2, 2), bool)], 2)

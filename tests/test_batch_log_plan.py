"""The planner and the argument checks of the batched LoG (prad_batch_log_plan, prad_batch_log_dev) -- everything that is
answered without a device.  Host buffers stand in for the device pointers; no call of prad_batch_log_dev here gets as far as a
launch (never add an all-valid call with a pair the kernel takes: with a GPU it would run on host memory)."""
import ctypes as C

import numpy as np
import pytest

IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
OK, ARG = 1, -1
NO_IMAGE = 16
TWO = [(6, 6, 6), (4, 4, 5)]
ZERO = [(6, 6, 6), (4, 0, 5)]


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


def _ip(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.intc).ctypes.data_as(IP)


def _lp(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(LP)


def _dp(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return C.c_void_p(a.ctypes.data), a          # (the array must outlive the call)


_BUF = np.zeros(4096, dtype=np.float64)      # stands in for every device pointer


def _vp(null, name):
    return None if name in null else C.c_void_p(_BUF.ctypes.data)


def _check(got, want):
    from pyradiomics_amd import _lib
    code, text = want if isinstance(want, tuple) else (want, None)
    assert got == code, (got, _lib.last_error())
    if text is not None:
        assert text in _lib.last_error(), _lib.last_error()
    assert (_BUF == 0).all(), "a buffer was written"


def test_verdicts():
    from pyradiomics_amd import roi_batch
    assert roi_batch.LOG_NO_IMAGE == NO_IMAGE
    boxes = [(4, 4, 4), (6, 6, 6), (5, 6, 7), (3, 8, 8), (32, 32, 32), (36, 36, 36), (4, 4, 65)]
    verdict, cls = roi_batch.batch_log_plan(boxes, (1.0, 5.0), (1.0, 1.0, 1.0))
    assert verdict.shape == (2, 7) and cls.shape == (7,)
    assert verdict[:, 0].tolist() == [0, NO_IMAGE]             # 4 < ceil(5) + 1
    assert verdict[:, 1].tolist() == [0, 0]
    assert verdict[:, 2].tolist() == [0, NO_IMAGE]
    assert verdict[:, 3].tolist() == [NO_IMAGE, NO_IMAGE]      # "Image too small"
    assert verdict[:, 4].tolist() == [0, 0]
    assert verdict[:, 5].tolist() == [8, 8]                    # 182 KiB of LDS
    assert verdict[:, 6].tolist() == [8, 8]                    # an extent above 64
    one = lambda box, sigma, spacing: int(roi_batch.batch_log_plan([box], [sigma], spacing)[0][0, 0])
    assert one((4, 8, 8), 3.0, (3.0, 1.0, 1.0)) == 0           # ceil(1) + 1 = 2
    assert one((6, 8, 8), 3.0, (0.5, 1.0, 1.0)) == NO_IMAGE    # 6 < 7
    # per-ROI spacing
    verdict, _ = roi_batch.batch_log_plan([(6, 8, 8), (6, 8, 8)], [3.0], [(0.5, 1.0, 1.0), (1.0, 1.0, 1.0)])
    assert verdict.tolist() == [[NO_IMAGE, 0]]


def test_n_items_counts_the_zeros(lib):
    boxes = [(4, 4, 4), (6, 6, 6), (5, 6, 7), (3, 8, 8), (32, 32, 32), (36, 36, 36), (4, 4, 65)]
    sp, keep_sp = _dp(np.ones((len(boxes), 3)))
    sg, keep_sg = _dp([1.0, 5.0, 2.0])
    verdict = np.full((3, len(boxes)), -1, dtype=np.intc)
    cls = np.full(len(boxes), -7, dtype=np.intc)
    n = C.c_longlong(-1)
    assert lib.prad_batch_log_plan(_ip(boxes), len(boxes), sp, sg, 3, verdict.ctypes.data_as(IP), cls.ctypes.data_as(IP), C.byref(n)) == OK
    assert set(verdict.ravel().tolist()) == {0, 8, NO_IMAGE}
    assert n.value == int((verdict == 0).sum()) == 10
    assert cls.tolist() == [0, 0, 0, -1, 2, -1, -1]


def test_lds_classes():
    from pyradiomics_amd import roi_batch
    boxes = [(4, 4, 4), (8, 8, 8), (16, 16, 15), (16, 16, 16), (20, 20, 20), (25, 25, 25), (26, 26, 26), (32, 32, 32), (4, 64, 64),
             (64, 64, 9), (64, 64, 10)] + [(6, 6, 6)] * 40
    _, cls = roi_batch.batch_log_plan(boxes, [1.0])
    foot = np.array([4 * z * y * (x | 1) for z, y, x in boxes])
    native = foot <= 160 * 1024
    assert (cls[~native] == -1).all() and native[:-41].sum() == 10 and not native[10]      # 64 x 64 x 11 floats: 176 KiB
    order = np.argsort(foot[native], kind="stable")
    assert (np.diff(cls[native][order]) >= 0).all()                  # monotone in the footprint
    assert set(cls[native].tolist()) == {0, 1, 2}
    assert cls[1] != cls[7]                                          # (8, 8, 8) and (32, 32, 32)
    assert len(set(cls[-40:].tolist())) == 1                         # forty (6, 6, 6) boxes share one class
    assert cls[2] == 0 and cls[3] == 1 and cls[5] == 1 and cls[6] == 2      # the edges: 16 KiB and 64 KiB
    # a plan is a function of its arguments alone
    again = roi_batch.batch_log_plan(boxes, [1.0])
    assert np.array_equal(again[1], cls)


def _plan(lib, sizes=TWO, B=2, spacing=None, sigmas=(1.0, 2.0), S=2, null=()):
    sp, keep_sp = _dp(np.ones((2, 3)) if spacing is None else spacing)
    sg, keep_sg = _dp(sigmas)
    verdict, cls = np.zeros(32, dtype=np.intc), np.zeros(8, dtype=np.intc)
    n = C.c_longlong(0)
    return lib.prad_batch_log_plan(None if "sizes" in null else _ip(sizes), B, None if "spacing" in null else sp,
                                   None if "sigmas" in null else sg, S, None if "verdict" in null else _ip(verdict),
                                   None if "lds_class" in null else _ip(cls), None if "n_items" in null else C.byref(n))


def test_plan_errors(lib):
    _check(_plan(lib, B=0), (ARG, "B=0"))
    _check(_plan(lib, B=-1), (ARG, "B=-1"))
    _check(_plan(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_plan(lib, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    _check(_plan(lib, S=0), (ARG, "S=0"))
    _check(_plan(lib, sigmas=[1.0] * 9, S=9), (ARG, "S=9"))
    _check(_plan(lib, sigmas=(1.0, 0.0)), (ARG, "sigma[1]"))
    _check(_plan(lib, sigmas=(-1.0, 2.0)), (ARG, "sigma[0]"))
    _check(_plan(lib, spacing=[(1, 1, 1), (1, 0, 1)]), (ARG, "ROI 1 has spacing[1]"))
    _check(_plan(lib, spacing=[(1, 1, -2), (1, 1, 1)]), (ARG, "ROI 0 has spacing[2]"))
    for name in ("spacing", "sigmas"):
        _check(_plan(lib, null=(name,)), (ARG, "NULL pointer"))
    for name in ("verdict", "lds_class", "n_items"):
        _check(_plan(lib, null=(name,)), (ARG, "NULL output"))
    _check(_plan(lib), OK)


# (3, 8, 8) and (36, 36, 36): no pair for the kernel, so an all-valid call returns before anything touches the device
NONE_NATIVE = [(3, 8, 8), (36, 36, 36)]


def _log(lib, sizes=TWO, B=2, dtype=0, off=(0, 216), spacing=None, sigmas=(1.0, 2.0), S=2, row_stride=296, null=(), verdict=None):
    sp, keep_sp = _dp(np.ones((2, 3)) if spacing is None else spacing)
    sg, keep_sg = _dp(sigmas)
    v = np.zeros(32, dtype=np.intc) if verdict is None else verdict
    return lib.prad_batch_log_dev(_vp(null, "in"), dtype, None if "sizes" in null else _ip(sizes), None if "off" in null else _lp(off),
                                  B, None if "spacing" in null else sp, None if "sigmas" in null else sg, S, 1, _vp(null, "out"),
                                  row_stride, None if "verdict" in null else v.ctypes.data_as(IP), None)


def test_entry_errors(lib):
    _check(_log(lib, B=0), (ARG, "B=0"))
    _check(_log(lib, B=-1), (ARG, "B=-1"))
    _check(_log(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_log(lib, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    for name in ("in", "off", "spacing", "sigmas", "out", "verdict"):
        _check(_log(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_log(lib, S=0), (ARG, "S=0"))
    _check(_log(lib, sigmas=[1.0] * 9, S=9), (ARG, "S=9"))
    _check(_log(lib, sigmas=(1.0, 0.0)), (ARG, "sigma[1]"))
    _check(_log(lib, spacing=[(1, 1, 1), (0, 1, 1)]), (ARG, "ROI 1 has spacing[0]"))
    _check(_log(lib, off=(0, -216)), (ARG, "off[1]=-216"))
    _check(_log(lib, off=(0, 215)), (ARG, "off[1]=215 lies before the end of ROI 0 (216)"))      # overlapping offsets
    _check(_log(lib, off=(300, 0), row_stride=600), (ARG, "off[1]=0"))
    _check(_log(lib, row_stride=295), (ARG, "row_stride=295"))
    _check(_log(lib, dtype=4), (ARG, "dtype 4"))
    _check(_log(lib, dtype=-1), (ARG, "dtype -1"))
    # two things wrong: still an argument error
    _check(_log(lib, dtype=7, B=0), (ARG, "dtype 7"))
    _check(_log(lib, sizes=NONE_NATIVE, off=(0, 192), row_stride=10, sigmas=(1.0, 0.0)), (ARG, "sigma[1]"))


def test_a_call_without_a_native_pair_launches_nothing(lib):
    verdict = np.full(32, -1, dtype=np.intc)
    _check(_log(lib, sizes=NONE_NATIVE, off=(0, 192), row_stride=192 + 36 ** 3, verdict=verdict), OK)
    assert verdict[:4].tolist() == [NO_IMAGE, 8, NO_IMAGE, 8] and (verdict[4:] == -1).all()


def test_python_argument_errors():
    from pyradiomics_amd import roi_batch
    with pytest.raises(ValueError):
        roi_batch.batch_log_plan([(6, 6, 6)], [0.0])
    with pytest.raises(ValueError):
        roi_batch.batch_log_plan([(6, 6, 6)], [1.0], (1.0, 1.0))
    with pytest.raises(ValueError):
        roi_batch.batch_log_plan([(6, 6, 6)], [1.0] * 9)


def test_image_types_of_the_table_calls():
    """roi_features_batch_derived takes LoG; roi_features_batch_images keeps naming it, and both name a type neither batches
    (before anything touches a device)"""
    import torch
    from pyradiomics_amd import roi_batch
    x = torch.zeros(8)
    with pytest.raises(NotImplementedError, match="Logarithm"):
        roi_batch.roi_features_batch_derived(x, x, [(2, 2, 2)], imageTypes={"LoG": {"sigma": [1.0]}, "Logarithm": {}})
    with pytest.raises(NotImplementedError, match="roi_features_batch_derived takes LoG"):
        roi_batch.roi_features_batch_images(x, x, [(2, 2, 2)], imageTypes={"Original": {}, "LoG": {"sigma": [1.0]}})
    with pytest.raises(ValueError):          # accepted as a type: the call gets as far as asking for device tensors
        roi_batch.roi_features_batch_derived(x, x, [(2, 2, 2)], imageTypes={"Original": {}, "LoG": {"sigma": [1.0]}})

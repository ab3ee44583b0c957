"""The argument checks of the device resegmentation (prad_resegment_dev, prad_batch_resegment_dev, engine.resegment,
roi_batch.resegment_batch, cmatrices.calculate_resegment_batch) and the host arithmetic the batched call falls back on --
everything that is answered without a device.  Host buffers stand in for the device pointers; no call of either entry point here
gets as far as a launch (never add an all-valid call with B > 0, or an all-valid single call: with a GPU it would run on host
memory)."""
import ctypes as C

import numpy as np
import pytest

IP, LP, DP = C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_double)
OK, ARG, UNSUPPORTED = 1, -1, -4
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


def _single(lib, dtype=3, label_dtype=3, size=(3, 5, 4), Nd=3, label=1, mode=0, rng=(0.0, 1.0), nrange=2, null=()):
    r = np.ascontiguousarray(rng, dtype=np.float64)
    counts, box, thr = np.zeros(2, dtype=np.int64), np.zeros(6, dtype=np.intc), np.zeros(2)
    return lib.prad_resegment_dev(_vp(null, "image"), dtype, _vp(null, "labelmap"), label_dtype,
                                  None if "size" in null else _ip(size), Nd, label, mode,
                                  None if "range" in null else r.ctypes.data_as(DP), nrange, _vp(null, "out_mask"),
                                  None if "counts" in null else counts.ctypes.data_as(LP),
                                  None if "box" in null else box.ctypes.data_as(IP),
                                  None if "thr" in null else thr.ctypes.data_as(DP), None)


def test_single_entry_errors(lib):
    for name in ("image", "labelmap", "size", "range", "out_mask", "counts", "box", "thr"):
        _check(_single(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_single(lib, dtype=4), (ARG, "dtype 4"))
    _check(_single(lib, dtype=-1), (ARG, "dtype -1"))
    _check(_single(lib, label_dtype=1), (ARG, "label dtype code 1"))
    _check(_single(lib, label_dtype=5), (ARG, "label dtype code 5"))
    _check(_single(lib, mode=3), (ARG, "mode=3"))
    _check(_single(lib, mode=-1), (ARG, "mode=-1"))
    _check(_single(lib, nrange=0), (ARG, "nrange=0"))
    _check(_single(lib, nrange=3), (ARG, "nrange=3"))
    _check(_single(lib, rng=(0.0, np.nan)), (ARG, "range[1] is NaN"))
    _check(_single(lib, Nd=0), (ARG, "Nd=0"))
    _check(_single(lib, Nd=4, size=(2, 2, 2, 2)), (ARG, "Nd=4"))
    _check(_single(lib, size=(3, 0, 4)), (ARG, "size[1]=0"))
    _check(_single(lib, size=(3, 5, -4)), (ARG, "size[2]=-4"))
    # numpy accumulates the mean of a float32 array in float32: declined before anything is launched
    _check(_single(lib, dtype=0, mode=2), (UNSUPPORTED, "sigma mode on a float32 image"))


def _batch(lib, sizes=TWO, B=2, dtype=3, off=(0, 216), mode=0, rng=(0.0, 1.0), nrange=2, null=()):
    r = np.ascontiguousarray(rng, dtype=np.float64)
    boxes, thr, verdict = np.zeros((2, 7), dtype=np.intc), np.zeros((2, 2)), np.zeros(2, dtype=np.intc)
    return lib.prad_batch_resegment_dev(_vp(null, "image"), dtype, _vp(null, "mask"), None if "sizes" in null else _ip(sizes),
                                        None if "off" in null else _lp(off), B, mode,
                                        None if "range" in null else r.ctypes.data_as(DP), nrange, _vp(null, "out_mask"),
                                        None if "boxes" in null else boxes.ctypes.data_as(IP),
                                        None if "thr" in null else thr.ctypes.data_as(DP),
                                        None if "verdict" in null else verdict.ctypes.data_as(IP), None)


def test_batch_entry_errors(lib):
    _check(_batch(lib, B=-1), (ARG, "B=-1"))
    _check(_batch(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_batch(lib, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    for name in ("image", "mask", "off", "out_mask", "boxes", "thr", "verdict", "range"):
        _check(_batch(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_batch(lib, dtype=4), (ARG, "dtype 4"))
    _check(_batch(lib, dtype=-1), (ARG, "dtype -1"))
    _check(_batch(lib, mode=3), (ARG, "mode=3"))
    _check(_batch(lib, nrange=0), (ARG, "nrange=0"))
    _check(_batch(lib, nrange=3), (ARG, "nrange=3"))
    _check(_batch(lib, rng=(np.nan, 1.0)), (ARG, "range[0] is NaN"))
    _check(_batch(lib, off=(0, -216)), (ARG, "off[1]=-216"))
    # B = 0 is a valid call that launches nothing, in every mode; nothing but the range is read
    for mode in (0, 1, 2):
        _check(_batch(lib, B=0, mode=mode), OK)
        _check(_batch(lib, B=0, mode=mode, null=("image", "mask", "sizes", "off", "out_mask", "boxes", "thr", "verdict")), OK)
    _check(_batch(lib, B=0, nrange=1), OK)


def test_symbols_are_declared_everywhere(lib):
    from pyradiomics_amd import _lib
    for name in ("prad_resegment_dev", "prad_batch_resegment_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name


def test_python_argument_errors_come_before_any_device_work():
    """host tensors: a call that got as far as the device layer would complain about them instead"""
    import torch
    from pyradiomics_amd import cmatrices, engine, roi_batch
    assert engine.resegment_batch is roi_batch.resegment_batch
    x, m = torch.zeros(8), torch.ones(8, dtype=torch.uint8)
    calls = (lambda **kw: engine.resegment(x.view(2, 2, 2), m.view(2, 2, 2), 1, **kw),
             lambda **kw: roi_batch.resegment_batch(x, m, [(2, 2, 2)], **kw),
             lambda **kw: cmatrices.calculate_resegment_batch([np.zeros((2, 2, 2))], [np.ones((2, 2, 2))], **kw),
             lambda **kw: roi_batch.roi_features_batch(x, m, [(2, 2, 2)], **kw),
             lambda **kw: roi_batch.roi_features_batch_types(x, m, [(2, 2, 2)], **kw))
    for k, call in enumerate(calls):
        if k < 3:
            with pytest.raises(ValueError, match=r"^resegmentRange is None\.$"):
                call(resegmentRange=None)
        for bad in ([], [1, 2, 3], ()):
            with pytest.raises(ValueError, match=r"^Length %d is not allowed for resegmentRange$" % len(bad)):
                call(resegmentRange=bad)
        with pytest.raises(ValueError, match=r"^Resegment mode percent not recognized\.$"):
            call(resegmentRange=[0, 1], resegmentMode="percent")
    # good arguments pass these checks: the calls get as far as asking for device tensors
    with pytest.raises(ValueError, match="expects CUDA/HIP tensors"):
        engine.resegment(x.view(2, 2, 2), m.view(2, 2, 2), 1, [0.0, 1.0], "sigma")
    with pytest.raises(ValueError, match="expects CUDA/HIP tensors"):
        roi_batch.resegment_batch(x, m, [(2, 2, 2)], [0.5], "relative")


def test_threshold_numbers_the_device_reproduces():
    """Python numbers and float64 scalars go to the kernels as float64; anything whose host arithmetic is not float64 (or float32
    for a float32 image) is handed back to the host code"""
    from pyradiomics_amd import engine
    assert engine._resegment_numbers([-1000, 400], 0, True).tolist() == [-1000.0, 400.0]
    assert engine._resegment_numbers([0.1, np.float64(0.9)], 1, True).tolist() == [0.1, 0.9]
    assert engine._resegment_numbers([0, 1], 1, True).tolist() == [0.0, 1.0]
    for rng, mode, integer in (([np.float32(0.1)], 0, False), ([0, 2], 1, True), ([True], 0, True), (["1"], 0, True),
                               ([np.int16(1)], 1, True), ([float("nan")], 0, False), ([2 ** 60], 0, True)):
        with pytest.raises(NotImplementedError):
            engine._resegment_numbers(rng, mode, integer)
    assert engine._resegment_numbers([0, 2], 1, False).tolist() == [0.0, 2.0]          # (a float image: a float product)


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
@pytest.mark.parametrize("mode", ["absolute", "relative", "sigma"])
@pytest.mark.parametrize("rng", [[0.25], [-0.5, 0.75], [0.75, -0.5]])
def test_host_arithmetic_of_the_fallback_equals_resegmentMask(dtype, mode, rng):
    """imageoperations.resegmentArrays (what resegment_batch runs for the ROIs its launch does not serve) against
    resegmentMask itself"""
    from pyradiomics_amd import imageoperations
    from pyradiomics_amd.image import Image
    g = np.random.default_rng(7)
    im = g.integers(-40, 90, (5, 6, 7)).astype(dtype)
    if np.issubdtype(dtype, np.floating):
        im += np.asarray(0.1, dtype=dtype)
    mask = (g.random(im.shape) < 0.6).astype(np.uint8)
    t = rng if mode != "absolute" else [20 * v for v in rng]
    kept, thr = imageoperations.resegmentArrays(im, mask != 0, t, mode)
    assert len(thr) == len(t)
    try:
        want = imageoperations.resegmentMask(Image(im), Image(mask), resegmentRange=t, resegmentMode=mode, label=1).array != 0
    except ValueError as e:
        assert "retained %d voxel" % kept.sum() in str(e) and kept.sum() <= 1
    else:
        assert np.array_equal(kept, want) and kept.sum() > 1
    assert (mask != 0).sum() >= kept.sum() and not (kept & (mask == 0)).any()

"""The planner and the argument checks of the batched wavelet transform (prad_batch_swt_plan, prad_batch_swt_dev) and the
names of its sub-bands -- everything that is answered without a device.  Host buffers stand in for the device pointers; no
call of prad_batch_swt_dev here gets as far as a launch (never add an all-valid call: with a GPU it would run on host memory)."""
import ctypes as C

import numpy as np
import pytest

IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
OK, ARG, UNSUPPORTED = 1, -1, -4
TWO = [(2, 3, 4), (1, 1, 5)]
ZERO = [(2, 3, 4), (1, 0, 5)]
BOXES = [(5, 6, 7), (4, 8, 8), (1, 16, 16), (3, 3, 3), (2, 2, 2), (40, 40, 40)]
# native = every padded extent (n + n % 2) holds the filter
NATIVE = {2: [0, 0, 0, 0, 0, 0], 4: [0, 0, 8, 0, 8, 0], 6: [0, 8, 8, 8, 8, 0]}


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


@pytest.mark.parametrize("flen", [2, 4, 6])
def test_verdicts(lib, flen):
    from pyradiomics_amd import roi_batch
    verdict, items = roi_batch.batch_swt_plan(BOXES, flen)
    assert verdict.tolist() == NATIVE[flen]
    # the cases the kernel's domain is defined by
    one = lambda box, f: int(roi_batch.batch_swt_plan([box], f)[0][0])
    assert one((5, 6, 7), 6) == 0            # extent 5 pads to 6 = F
    assert one((4, 8, 8), 6) == 8
    assert one((1, 16, 16), 2) == 0 and one((1, 16, 16), 4) == 8
    assert set(items[:, 0].tolist()) == set(np.flatnonzero(verdict == 0).tolist())      # non-native ROIs get no item


@pytest.mark.parametrize("flen", [2, 4, 6])
def test_items_tile_every_native_box_exactly_once(lib, flen):
    from pyradiomics_amd import roi_batch
    boxes = BOXES + [(9, 33, 17), (8, 7, 31), (7, 15, 9), (17, 32, 8), (6, 16, 33), (2, 2, 65)] + [(6, 6, 6)] * 40
    verdict, items = roi_batch.batch_swt_plan(boxes, flen)
    covers = [np.zeros(b, dtype=np.int32) for b in boxes]
    for roi, z0, z1, y0, y1, x0, x1, tx in items.tolist():
        assert tx in (8, 16, 32) and 0 < y1 - y0 <= 256 // tx and 0 < x1 - x0 <= tx and z1 > z0
        assert 0 <= z0 and z1 <= boxes[roi][0] and 0 <= y0 and y1 <= boxes[roi][1] and 0 <= x0 and x1 <= boxes[roi][2]
        covers[roi][z0:z1, y0:y1, x0:x1] += 1
    for b, c in enumerate(covers):
        assert (c == (1 if verdict[b] == 0 else 0)).all(), (b, boxes[b])
    # one large box among small ones is spread over many workgroups
    big = boxes.index((40, 40, 40))
    assert (items[:, 0] == big).sum() >= 32
    # a plan is a function of its arguments alone
    again = roi_batch.batch_swt_plan(boxes, flen)
    assert np.array_equal(again[0], verdict) and np.array_equal(again[1], items)


def test_occupancy_counts(lib):
    from pyradiomics_amd import roi_batch
    occ = roi_batch.batch_swt_occupancy([(16, 16, 16)] * 4, 6)
    assert occ["native"] == 4 and occ["items"] == 4 * 2                      # 16 x 16 tiles, two z ranges of 8
    assert occ["active_lanes"] == 1.0 and occ["warmup_planes"] == pytest.approx(5 / 13)
    occ = roi_batch.batch_swt_occupancy([(8, 10, 10)], 2)
    assert occ["items"] == 1 and occ["active_lanes"] == pytest.approx(100 / 256) and occ["warmup_planes"] == pytest.approx(1 / 9)


def _plan(lib, sizes=TWO, B=2, flen=2, null=()):
    sz = np.ascontiguousarray(sizes, dtype=np.intc)
    verdict = np.zeros(8, dtype=np.intc)
    n = C.c_longlong(0)
    return lib.prad_batch_swt_plan(None if "sizes" in null else _ip(sz), B, flen, None if "verdict" in null else _ip(verdict),
                                   None if "n_items" in null else C.byref(n), None)


def test_plan_errors(lib):
    _check(_plan(lib, flen=8), (UNSUPPORTED, "flen=8"))
    _check(_plan(lib, flen=3), (UNSUPPORTED, "flen=3"))
    _check(_plan(lib, flen=1), (ARG, "flen=1"))
    _check(_plan(lib, flen=33), (ARG, "flen=33"))
    _check(_plan(lib, B=0), (ARG, "B=0"))
    _check(_plan(lib, B=-1), (ARG, "B=-1"))
    _check(_plan(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_plan(lib, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    _check(_plan(lib, null=("verdict",)), (ARG, "NULL output"))
    _check(_plan(lib, null=("n_items",)), (ARG, "NULL output"))
    _check(_plan(lib), OK)


def _swt(lib, sizes=TWO, B=2, dtype=0, off=(0, 24), flen=2, band_stride=29, null=()):
    sz = np.ascontiguousarray(sizes, dtype=np.intc)
    verdict = np.zeros(8, dtype=np.intc)
    return lib.prad_batch_swt_dev(_vp(null, "in"), dtype, None if "sizes" in null else _ip(sz), None if "off" in null else _lp(off),
                                  B, _vp(null, "dec_lo"), _vp(null, "dec_hi"), flen, _vp(null, "out"), band_stride,
                                  None if "verdict" in null else _ip(verdict), None)


def test_entry_errors(lib):
    _check(_swt(lib, B=0), (ARG, "B=0"))
    _check(_swt(lib, B=-1), (ARG, "B=-1"))
    _check(_swt(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_swt(lib, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    for name in ("in", "off", "dec_lo", "dec_hi", "out", "verdict"):
        _check(_swt(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_swt(lib, off=(0, -24)), (ARG, "off[1]=-24"))
    _check(_swt(lib, off=(0, 23)), (ARG, "off[1]=23 lies before the end of ROI 0 (24)"))       # decreasing / overlapping offsets
    _check(_swt(lib, off=(30, 0), band_stride=64), (ARG, "off[1]=0"))
    _check(_swt(lib, band_stride=28), (ARG, "band_stride=28"))
    _check(_swt(lib, dtype=4), (ARG, "dtype 4"))
    _check(_swt(lib, dtype=-1), (ARG, "dtype -1"))
    _check(_swt(lib, flen=8), (UNSUPPORTED, "flen=8"))
    _check(_swt(lib, flen=3), (UNSUPPORTED, "flen=3"))
    _check(_swt(lib, flen=0), (ARG, "flen=0"))
    _check(_swt(lib, flen=34), (ARG, "flen=34"))
    _check(_swt(lib, sizes=[(1, 1, 1), (1, 1, 1)], off=(0, 1), flen=4), OK)      # no native ROI: nothing to launch
    # two things wrong: an argument error wins over the domain
    _check(_swt(lib, flen=8, null=("out",)), (ARG, "NULL pointer"))
    _check(_swt(lib, flen=8, off=(0, 23)), (ARG, "off[1]=23"))
    _check(_swt(lib, flen=8, sizes=ZERO), (ARG, "ROI 1"))
    _check(_swt(lib, dtype=7, B=0), (ARG, "dtype 7"))


def test_unbatched_image_type_is_named():
    import torch
    from pyradiomics_amd import roi_batch
    x = torch.zeros(8)
    with pytest.raises(NotImplementedError, match="LoG"):
        roi_batch.roi_features_batch_images(x, x, [(2, 2, 2)], imageTypes={"Original": {}, "LoG": {"sigma": [1.0]}})


@pytest.mark.parametrize("level,force2D", [(1, False), (2, False), (1, True), (3, True)])
def test_names_are_those_getWaveletImage_yields(monkeypatch, level, force2D):
    """getWaveletImage itself names the bands; only the transform under it (the device call) is replaced by a stand-in that
    returns PyWavelets' keys in PyWavelets' order"""
    from pyradiomics_amd import filters, roi_batch

    def swtn_level1(data, lo, hi, axes):
        keys = [""]
        for _ in axes:
            keys = [k + c for k in keys for c in "ad"]
        return {k: np.zeros_like(data, dtype=np.float64) for k in keys}
    monkeypatch.setattr(filters, "swtn_level1", swtn_level1)
    kw = dict(level=level, force2D=force2D, force2Ddimension=0, deviceResident=False)
    want = [name for _img, name, _kw in filters.getWaveletImage(np.zeros((4, 6, 8), dtype=np.float32), None, **kw)]
    names = roi_batch.wavelet_band_names(level, 2 if force2D else 3)
    assert list(names) == want
    assert sorted(names.rows) == list(range(len(want)))
    if level == 1 and not force2D:
        assert want == ["wavelet-LLH", "wavelet-LHL", "wavelet-LHH", "wavelet-HLL", "wavelet-HLH", "wavelet-HHL", "wavelet-HHH",
                        "wavelet-LLL"]
        # the row of a name is the kernels' band index (bx * 2 + by) * 2 + bz, first letter = x, L = 0, H = 1
        for name in names:
            bx, by, bz = (int(c == "H") for c in name[-3:])
            assert names.row(name) == (bx * 2 + by) * 2 + bz

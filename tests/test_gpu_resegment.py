"""GPU: the device resegmentation -- engine.resegment (prad_resegment_dev) and engine.resegment_batch
(prad_batch_resegment_dev) -- against the host code of imageoperations.resegmentMask on numpy copies, which is the oracle: the
device mask must equal it voxel for voxel.

Single call: 4 image element types x 3 modes x {one threshold, two, two given unsorted}, on the shapes (7,), (1, 1, 7), (3, 5, 4),
(5, 7, 67) -- rows that are no multiple of any vector width -- and (64, 64, 65) -- 65 workgroups contribute partials --, with
label 3 in a map that also holds the labels 1 and 5 (those must come out 0), the map as int32, int16 and uint8.

Sigma mode, the margin condition.  The device and numpy sum the same terms in different orders.  For the sizes here (n <= 2^18)
both sums are within n 2^-53 < 2e-11 relative of the exact sum, so a voxel can fall on different sides of a threshold only when
it lies that close to it.  _margin() asserts ON THE CPU, in long double, that no ROI value lies within 1e-9 (|mu| + |sd t| + 1) of
a threshold; the inputs are integer-valued and chosen so that this holds.  This is a condition on the INPUTS, stated here; it is
not a tolerance on the result: the masks are then demanded equal.  One kind of ROI is exempt, with this reasoning: a CONSTANT ROI
of integer value c.  Its sum n c is exact in any order (n |c| < 2^53), so the mean is c, every deviation is 0, sd is 0 and both
thresholds are c exactly -- in numpy and on the device alike: there is no rounding to guard against."""
import re
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "int32", "int16"]
MODES = ["absolute", "relative", "sigma"]
SHAPES = [(7,), (1, 1, 7), (3, 5, 4), (5, 7, 67), (64, 64, 65)]
RANGES = {"absolute": ([12.0], [-7.0, 31.0], [31.0, -7.0]),
          "relative": ([0.37], [0.21, 0.83], [0.83, 0.21]),
          "sigma": ([-0.43], [-1.17, 0.93], [0.93, -1.17])}
BATCH_RANGE = {"absolute": [-3.0, 7.0], "relative": [0.5, 1.0], "sigma": [-0.5, 0.5]}
LABEL = 3
TOO_FEW = "Resegmentation excluded too many voxels with label %s \\(retained %d voxel\\(s\\)\\)! Cannot extract features"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(shape, dtype, seed=0):
    """integer-valued image, label map with the labels 0, 1, 3, 5 (about 40 % of the voxels carry label 3)"""
    g = np.random.default_rng(1000 * seed + DTYPES.index(dtype) + 17 * len(shape) + int(np.prod(shape)))
    im = g.integers(-40, 60, shape).astype(dtype)
    lab = g.choice(np.array([0, 1, 3, 5]), size=shape, p=[0.3, 0.15, 0.4, 0.15])
    if im.size == 7:                     # the smallest shapes: six ROI voxels of which every range above keeps at least two
        lab.reshape(-1)[:] = (LABEL,) * 6 + (1,)
        im.reshape(-1)[:] = (25, 30, 28, 27, 55, 20, -10)
    return im, lab


def _host(im, lab, rng, mode, label=LABEL):
    """the oracle: the host code, on host Images"""
    from pyradiomics_amd import imageoperations
    from pyradiomics_amd.image import Image
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return imageoperations.resegmentMask(Image(im), Image(lab), resegmentRange=rng, resegmentMode=mode, label=label).array


def _margin(im, roi, rng, mode):
    """the sigma-mode condition of the module docstring, in long double, on the CPU"""
    if mode != "sigma":
        return
    x = im[roi].astype(np.longdouble)
    if not x.size:
        return          # an empty ROI has no thresholds
    if (x == x[0]).all() and float(x[0]) == int(x[0]):
        return          # a constant integer ROI: exact everywhere (module docstring)
    mu = x.sum() / x.size
    sd = np.sqrt(((x - mu) ** 2).sum() / x.size)
    for t in rng:
        thr = mu + sd * np.longdouble(t)
        assert np.abs(x - thr).min() > 1e-9 * (abs(mu) + abs(sd * t) + 1), (mode, t, float(thr))


def _box(roi):
    idx = np.nonzero(roi)
    return np.array([i.min() for i in idx]), np.array([i.max() for i in idx])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_call_equals_the_host_code(dtype, mode):
    from pyradiomics_amd import engine
    for k, shape in enumerate(SHAPES):
        im, lab = _case(shape, dtype)
        lab = lab.astype((np.int32, np.int16, np.uint8)[k % 3])
        d_im, d_lab = _dev(im), _dev(lab)
        for rng in RANGES[mode]:
            if dtype == "float32" and mode == "sigma":
                with pytest.raises(NotImplementedError, match="sigma mode on a float32 image"):
                    engine.resegment(d_im, d_lab, LABEL, rng, mode)
                continue
            _margin(im, lab == LABEL, rng, mode)
            want = _host(im, lab, rng, mode)
            out, kept, lo, hi, thr = engine.resegment(d_im, d_lab, LABEL, rng, mode)
            assert engine.last_path() == "resegment" and engine.last_variant() == "resegment-" + mode
            got = out.cpu().numpy()
            assert got.dtype == lab.dtype and got.shape == lab.shape
            assert np.array_equal(got, want), (shape, rng, int((got != want).sum()))
            assert set(np.unique(got)) <= {0, LABEL}
            assert kept == int((want == LABEL).sum())
            wlo, whi = _box(want == LABEL)
            assert lo.tolist() == wlo.tolist() and hi.tolist() == whi.tolist(), (shape, rng, lo, hi)
            assert thr.shape == (2,) and (np.isinf(thr[1]) if len(rng) == 1 else np.isfinite(thr[1]))
            again = engine.resegment(d_im, d_lab, LABEL, rng, mode)
            assert again[4].tobytes() == thr.tobytes() and np.array_equal(again[0].cpu().numpy(), got)


def test_float32_sigma_takes_the_host_route():
    from pyradiomics_amd import engine, imageoperations
    from pyradiomics_amd.image import Image
    im, lab = _case((5, 7, 67), "float32")
    im += np.float32(0.3)
    want = _host(im, lab, [-1.0, 1.0], "sigma")
    engine.resegment(_dev(im), _dev(lab), LABEL, [0.0], "absolute")          # (the device route leaves its mark ...)
    assert engine.last_path() == "resegment"
    engine.label_census(_dev(lab.astype(np.int16)))
    assert engine.last_path() == "label_census"
    got = imageoperations.resegmentMask(Image(tensor=_dev(im)), Image(tensor=_dev(lab)), resegmentRange=[-1.0, 1.0],
                                        resegmentMode="sigma", label=LABEL, deviceResident=True)
    assert engine.last_path() != "resegment"                                  # (... and this call did not go there)
    assert np.array_equal(got.array, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_values_on_the_bounds_are_kept(dtype):
    """absolute and relative mode: ROI voxels exactly equal to both bounds stay"""
    from pyradiomics_amd import engine
    im = np.arange(-6, 18).reshape(2, 3, 4).astype(dtype)          # -6 .. 17, the maximum 17
    lab = np.ones(im.shape, dtype=np.int16)
    for rng, mode, lo, hi in (([-3.0, 7.0], "absolute", -3, 7), ([7, -3], "absolute", -3, 7), ([0.0, 1.0], "relative", 0, 17),
                              ([4.0 / 17.0, 8.0 / 17.0], "relative", None, None), ([17.0], "absolute", 17, 17)):
        want = _host(im, lab, rng, mode, 1) if rng != [17.0] else None
        if want is None:
            with pytest.raises(ValueError, match=TOO_FEW % (1, 1)):          # the maximum alone is kept: one voxel
                engine.resegment(_dev(im), _dev(lab), 1, rng, mode)
            continue
        out, kept, _, _, thr = engine.resegment(_dev(im), _dev(lab), 1, rng, mode)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (rng, mode)
        if lo is not None:
            assert got[im == lo].all() and got[im == hi].all() and kept == hi - lo + 1
            assert not got[im == lo - 1].any() and (hi == 17 or not got[im == hi + 1].any())


def test_float32_bounds_are_compared_in_float32():
    """a float32 image holding np.float32(0.1) under the upper bound 0.1: numpy rounds the bound to float32 and keeps the voxel
    (a float64 comparison would drop it: float32(0.1) > 0.1); the relative bound is ONE float32 product"""
    from pyradiomics_amd import engine
    im = np.array([0.0, 0.05, 0.1, 0.1, 0.3, 0.7], dtype=np.float32).reshape(1, 2, 3)
    assert float(im[0, 0, 2]) > 0.1
    lab = np.ones(im.shape, dtype=np.uint8)
    want = _host(im, lab, [0.0, 0.1], "absolute", 1)
    assert want[0, 0, 2] == 1 and want[0, 1, 0] == 1 and want.sum() == 4
    out, kept, _, _, thr = engine.resegment(_dev(im), _dev(lab), 1, [0.0, 0.1], "absolute")
    assert np.array_equal(out.cpu().numpy(), want) and kept == 4 and thr[1] == float(np.float32(0.1))
    # relative: top = float32(0.7); the bounds are float32(0.7) * float32(t)
    edge = np.float32(0.7) * np.float32(0.43)
    im2 = np.array([edge, np.nextafter(edge, np.float32(0)), 0.7, 0.2, 0.5, 0.31], dtype=np.float32).reshape(1, 2, 3)
    want = _host(im2, lab, [0.43, 1.0], "relative", 1)
    assert want[0, 0, 0] == 1 and want[0, 0, 1] == 0
    out, kept, _, _, thr = engine.resegment(_dev(im2), _dev(lab), 1, [0.43, 1.0], "relative")
    assert np.array_equal(out.cpu().numpy(), want) and thr[0] == float(edge) and thr[1] == float(np.float32(0.7))


@pytest.mark.parametrize("dtype", DTYPES)
def test_relative_mode_with_a_negative_maximum_keeps_nothing(dtype):
    """[top * t for t in sorted(range)] is NOT sorted again: a negative maximum gives a descending pair"""
    from pyradiomics_amd import engine
    im = -np.arange(3, 27).reshape(2, 3, 4).astype(dtype)
    lab = np.full(im.shape, 2, dtype=np.int32)
    with pytest.raises(ValueError, match=TOO_FEW % (2, 0)):
        _host(im, lab, [0.5, 2.0], "relative", 2)
    with pytest.raises(ValueError, match=TOO_FEW % (2, 0)):
        engine.resegment(_dev(im), _dev(lab), 2, [0.5, 2.0], "relative")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,low", [("int16", -32768), ("int32", -2 ** 31)])
def test_the_most_negative_integer_inside_the_roi(dtype, low, mode):
    from pyradiomics_amd import engine
    im, lab = _case((5, 7, 67), dtype, seed=3)
    roi = np.flatnonzero(lab.reshape(-1) == LABEL)
    im.reshape(-1)[roi[:5]] = low
    im.reshape(-1)[roi[5:9]] = low + 1
    rng = {"absolute": [float(low), 0.0], "relative": [-1e9, 0.5], "sigma": [-0.77, 0.31]}[mode]
    _margin(im, lab == LABEL, rng, mode)
    want = _host(im, lab, rng, mode)
    out, kept, _, _, _ = engine.resegment(_dev(im), _dev(lab.astype(np.int16)), LABEL, rng, mode)
    assert np.array_equal(out.cpu().numpy(), want) and kept == int((want == LABEL).sum())
    if mode == "absolute":
        assert (want[im == low] == LABEL).sum() == 5


def test_retained_counts_and_absent_label():
    from pyradiomics_amd import engine
    im = np.arange(1, 25).reshape(2, 3, 4).astype(np.int16)
    lab = np.ones(im.shape, dtype=np.int16)
    d_im, d_lab = _dev(im), _dev(lab)
    for top, n in ((0.5, 0), (1.0, 1)):
        with pytest.raises(ValueError, match=TOO_FEW % (1, n)):
            _host(im, lab, [-5.0, top], "absolute", 1)
        with pytest.raises(ValueError, match=TOO_FEW % (1, n)):
            engine.resegment(d_im, d_lab, 1, [-5.0, top], "absolute")
    out, kept, lo, hi, _ = engine.resegment(d_im, d_lab, 1, [-5.0, 2.0], "absolute")
    assert kept == 2 and np.array_equal(out.cpu().numpy(), _host(im, lab, [-5.0, 2.0], "absolute", 1))
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [0, 0, 1]
    # a label the map does not hold: whatever the host code raises, with its text
    for mode in MODES:
        with pytest.raises(ValueError) as host:
            _host(im, lab, [0.1, 0.9], mode, 4)
        with pytest.raises(ValueError) as dev:
            engine.resegment(d_im, d_lab, 4, [0.1, 0.9], mode)
        assert str(dev.value) == str(host.value), mode


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_roi_ends_as_the_host_route_ends(mode, bad):
    from pyradiomics_amd import engine, imageoperations
    from pyradiomics_amd.image import Image
    im, lab = _case((5, 7, 67), "float64", seed=5)
    im.reshape(-1)[np.flatnonzero(lab.reshape(-1) == LABEL)[7]] = bad
    rng = RANGES[mode][1]
    with pytest.raises(NotImplementedError, match="non-finite"):
        engine.resegment(_dev(im), _dev(lab), LABEL, rng, mode)
    outside = im.copy()                                    # (a NaN OUTSIDE the ROI is nobody's business)
    outside.reshape(-1)[np.flatnonzero(lab.reshape(-1) == 1)[0]] = bad
    outside.reshape(-1)[np.flatnonzero(lab.reshape(-1) == LABEL)[7]] = 11.0
    _margin(outside, lab == LABEL, rng, mode)
    assert np.array_equal(engine.resegment(_dev(outside), _dev(lab), LABEL, rng, mode)[0].cpu().numpy(),
                          _host(outside, lab, rng, mode))
    args = dict(resegmentRange=rng, resegmentMode=mode, label=LABEL)
    try:
        want = _host(im, lab, rng, mode)
    except ValueError as e:
        with pytest.raises(ValueError, match=re.escape(str(e))), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            imageoperations.resegmentMask(Image(tensor=_dev(im)), Image(tensor=_dev(lab)), deviceResident=True, **args)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = imageoperations.resegmentMask(Image(tensor=_dev(im)), Image(tensor=_dev(lab)), deviceResident=True, **args)
        assert np.array_equal(got.array, want)


def test_device_resident_images_get_a_device_mask_with_its_census():
    """imageoperations.resegmentMask on device-resident Images: the mask stays in HBM and the kept count and box are where
    censusLookup and the ("bbox", label) memo find them"""
    from pyradiomics_amd import engine, imageoperations
    from pyradiomics_amd.image import Image
    im, lab = _case((64, 64, 65), "int16", seed=2)
    _margin(im, lab == LABEL, [-1.5, 0.5], "sigma")
    image, mask = Image(tensor=_dev(im)), Image(tensor=_dev(lab.astype(np.int16)))
    new = imageoperations.resegmentMask(image, mask, resegmentRange=[-1.5, 0.5], resegmentMode="sigma", label=LABEL)
    assert engine.last_path() == "resegment"
    assert new.on_device and new._array is None and image._array is None and mask._array is None      # nothing was downloaded
    want = _host(im, lab, [-1.5, 0.5], "sigma")
    count, lo, hi = imageoperations.censusLookup(new, LABEL)
    wlo, whi = _box(want == LABEL)
    assert count == int((want == LABEL).sum()) and lo.tolist() == wlo.tolist() and hi.tolist() == whi.tolist()
    blo, bhi = new._derived[("bbox", LABEL)]
    assert blo.tolist() == wlo.tolist() and bhi.tolist() == whi.tolist()
    assert imageoperations.censusLookup(new, 1)[0] == 0          # the other labels are gone
    assert np.array_equal(new.array, want)
    # host Images without deviceResident keep taking the numpy code
    engine.label_census(_dev(lab.astype(np.int16)))
    host = imageoperations.resegmentMask(Image(im), Image(lab), resegmentRange=[-1.5, 0.5], resegmentMode="sigma", label=LABEL)
    assert engine.last_path() != "resegment" and not host.on_device and np.array_equal(host.array, want)


# ---- the batch ----------------------------------------------------------------------------------------------------------------
def _ragged(dtype, mode):
    """seven ROIs: a 1-voxel box, an empty mask, a ROI that keeps nothing, one that keeps everything, (2, 3, 70), 16^3 and one box
    above batch_max_vox() -- for BATCH_RANGE[mode]"""
    g = np.random.default_rng(DTYPES.index(dtype) + 31)
    fill = lambda shape: g.integers(-20, 30, shape).astype(dtype)
    nothing, everything = {"absolute": (lambda s: g.integers(8, 30, s), lambda s: g.integers(-3, 8, s)),
                           "relative": (lambda s: g.integers(-30, -1, s), lambda s: g.integers(5, 11, s)),
                           "sigma": (lambda s: g.choice(np.array([-10, 10]), s), lambda s: np.full(s, 6))}[mode]
    boxes = [np.full((1, 1, 1), 5).astype(dtype), fill((4, 4, 4)), nothing((3, 4, 5)).astype(dtype),
             everything((4, 3, 6)).astype(dtype), fill((2, 3, 70)), fill((16, 16, 16)), fill((41, 41, 41))]
    if mode == "sigma":                       # exactly half and half: mean 0, sigma 10, thresholds -5 and 5
        boxes[2].reshape(-1)[:] = np.resize(np.array([-10, 10]), boxes[2].size).astype(dtype)
    masks = [(g.random(b.shape) < 0.7).astype(np.uint8) for b in boxes]
    masks[0][:] = 1
    masks[1][:] = 0
    masks[2][:] = 1
    masks[3][:] = 1
    return boxes, masks


def _expect(im, mask, rng, mode):
    """per ROI: (mask uint8, box row [7], status) from the host code; where it raises, the count is read from its message and the
    kept voxels are worked out with the same numpy expressions"""
    from pyradiomics_amd import imageoperations
    roi = mask != 0
    shape = list(im.shape)
    if not roi.any():
        return np.zeros(im.shape, np.uint8), shape + [-1, -1, -1, 0], 1
    try:
        kept = _host(im, mask, rng, mode, 1) != 0
        status = 0
    except ValueError as e:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            kept, _ = imageoperations.resegmentArrays(im, roi, rng, mode)
        n = int(re.search(r"retained (\d+) voxel", str(e)).group(1))
        assert n == kept.sum() <= 1
        status = 3
    if not kept.any():
        return kept.astype(np.uint8), shape + [-1, -1, -1, 0], status
    lo, hi = _box(kept)
    return kept.astype(np.uint8), lo.tolist() + hi.tolist() + [int(kept.sum())], status


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batch_equals_the_host_code_roi_by_roi(dtype, mode):
    from pyradiomics_amd import cmatrices, engine
    boxes, masks = _ragged(dtype, mode)
    rng = BATCH_RANGE[mode]
    assert boxes[6].size > engine.batch_max_vox() >= boxes[5].size
    want = []
    for im, m in zip(boxes, masks):
        _margin(im, m != 0, rng, mode)
        want.append(_expect(im, m, rng, mode))
    assert [w[2] for w in want] == [3, 1, 3, 0, 0, 0, 0]
    assert want[2][1][6] == 0 and want[3][1][6] == boxes[3].size and want[0][1][6] == 1

    def run(idx):
        out, bx, thr, status = engine.resegment_batch([_dev(boxes[b]) for b in idx], [_dev(masks[b]) for b in idx],
                                                      resegmentRange=rng, resegmentMode=mode)
        route = engine.last_batch_route()
        host, o, cut = out.cpu().numpy(), 0, []
        for b in idx:
            cut.append(host[o:o + boxes[b].size].reshape(boxes[b].shape))
            o += boxes[b].size
        assert o == host.size and host.dtype == np.uint8
        return cut, bx, thr, status, route

    order = list(range(7))
    cut, bx, thr, status, route = run(order)
    assert route == ("looped" if dtype == "float32" and mode == "sigma" else "mixed"), route
    assert bx.shape == (7, 7) and thr.shape == (7, 2) and status.tolist() == [w[2] for w in want]
    for b in order:
        assert np.array_equal(cut[b], want[b][0]), (b, int((cut[b] != want[b][0]).sum()))
        assert bx[b].tolist() == want[b][1], (b, bx[b], want[b][1])
    # a ROI's row depends on its values alone: the batch reversed, and every ROI in a batch of one
    rcut, rbx, rthr, rstatus, _ = run(order[::-1])
    for k, b in enumerate(order[::-1]):
        assert np.array_equal(rcut[k], cut[b]) and rbx[k].tolist() == bx[b].tolist() and rstatus[k] == status[b]
        assert rthr[k].tobytes() == thr[b].tobytes(), (b, rthr[k], thr[b])
        one = run([b])
        assert np.array_equal(one[0][0], cut[b]) and one[1][0].tolist() == bx[b].tolist() and one[3][0] == status[b]
        assert one[2][0].tobytes() == thr[b].tobytes(), (b, one[2][0], thr[b])
        native = b != 6 and not (dtype == "float32" and mode == "sigma")
        assert one[4] == ("batch" if native else "looped"), (b, one[4])
    # the numpy twin
    tm, tb, tt, ts = cmatrices.calculate_resegment_batch(boxes, masks, rng, mode)
    assert all(np.array_equal(a, c) for a, c in zip(tm, cut)) and np.array_equal(tb, bx) and ts.tolist() == status.tolist()
    assert tt.tobytes() == thr.tobytes()


def test_batch_verdict_of_a_non_finite_roi_goes_to_the_host():
    from pyradiomics_amd import engine
    g = np.random.default_rng(5)
    boxes = [g.integers(-20, 30, (4, 5, 6)).astype(np.float64) for _ in range(3)]
    masks = [np.ones(b.shape, np.uint8) for b in boxes]
    boxes[1][1, 2, 3] = np.nan
    masks[2][0, 0, 0] = 0
    boxes[2][0, 0, 0] = np.inf                 # outside the ROI: native
    out, bx, thr, status = engine.resegment_batch([_dev(b) for b in boxes], [_dev(m) for m in masks], resegmentRange=[-3.0, 7.0])
    assert engine.last_batch_route() == "mixed"
    want = [_expect(im, m, [-3.0, 7.0], "absolute") for im, m in zip(boxes, masks)]
    assert status.tolist() == [w[2] for w in want] == [0, 0, 0]
    host = out.cpu().numpy().reshape(3, 4, 5, 6)
    for b in range(3):
        assert np.array_equal(host[b], want[b][0]) and bx[b].tolist() == want[b][1]

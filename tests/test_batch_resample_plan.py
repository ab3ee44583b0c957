"""The planner and the argument checks of the batched resampling step -- everything that is answered without a device.

engine.batch_resample_plan against imageoperations.resampleImage(..., deviceResident=False) on seeded random boxes wrapped as
Images: the planner has to give the shape and the origin resampleImage gives when the box is the whole image (both from
resampleImage's float64 expressions, so: equal, not close), and a grid -- start, step -- on which the host route's own values
are reproduced by position.  The boxes are anisotropic and cover up- and down-sampling, a bounding box that touches a face (both
clips), a bounding-box axis of extent 1 (keeps its spacing), a 0 in resampledPixelSpacing, equal spacing (the crop, with the
aligned x extent of the device crop) and an empty mask.

Host buffers stand in for the device pointers of the C calls; no call here gets as far as a launch (never add an all-valid call
with a box the kernels take: with a GPU it would run on host memory)."""
import ctypes as C

import numpy as np
import pytest

IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
OK, ARG = 1, -1


def _mask(shape, lo, hi):
    m = np.zeros(shape, dtype=np.uint8)
    m[tuple(slice(a, b + 1) for a, b in zip(lo, hi))] = 1
    return m


# name -> (shape zyx, mask lo zyx, mask hi zyx, spacing zyx, resampledPixelSpacing xyz, padDistance)
CASES = {
    "up":            ((9, 12, 14), (3, 4, 5), (5, 8, 9), (2.5, 0.9, 0.8), (0.5, 0.5, 1.0), 2),
    "down":          ((20, 18, 16), (6, 5, 5), (13, 12, 10), (0.7, 0.45, 0.55), (1.0, 1.0, 2.0), 1),
    "mixed":         ((10, 22, 15), (3, 6, 4), (6, 15, 10), (3.0, 0.5, 1.3), (1.0, 1.0, 1.0), 3),
    "faces":         ((8, 9, 10), (0, 2, 0), (7, 8, 9), (1.5, 0.75, 0.6), (1.0, 1.0, 1.0), 5),       # both clips apply
    "default-pad":   ((30, 30, 30), (12, 11, 13), (17, 18, 16), (1.25, 0.8, 0.8), (1.0, 1.0, 1.0), 5),
    "extent-1-z":    ((7, 12, 11), (3, 3, 2), (3, 8, 7), (5.0, 0.8, 0.7), (1.0, 1.0, 1.0), 2),       # z keeps 5.0
    "extent-1-x":    ((7, 12, 11), (2, 3, 6), (4, 8, 6), (2.0, 0.8, 0.7), (1.0, 1.0, 1.0), 2),
    "zero-keeps-y":  ((9, 12, 14), (3, 4, 5), (5, 8, 9), (2.5, 0.9, 0.8), (1.0, 0.0, 1.0), 2),
    "zeros-are-crop": ((9, 12, 14), (3, 4, 5), (5, 8, 9), (2.5, 0.9, 0.8), (0.0, 0.0, 0.0), 2),
    "equal-x4":      ((9, 12, 14), (3, 4, 5), (5, 8, 8), (2.5, 0.9, 0.8), (0.8, 0.9, 2.5), 5),       # x extent 4: no growth
    "equal-grow":    ((9, 12, 14), (3, 4, 5), (5, 8, 9), (2.5, 0.9, 0.8), (0.8, 0.9, 2.5), 5),       # 5 -> 8 columns
    "equal-edges":   ((6, 7, 6), (1, 2, 1), (4, 5, 5), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 5),         # 5 columns in a row of 6
}


def _one(name):
    from pyradiomics_amd import engine
    shape, lo, hi, spacing, new, pad = CASES[name]
    plan = engine.batch_resample_plan([shape], [lo], [hi], spacing, new, pad)
    return plan


def _images(name):
    from pyradiomics_amd.image import Image
    shape, lo, hi, spacing, new, pad = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    origin = tuple(rng.uniform(-50, 50, 3))
    img = Image(rng.standard_normal(shape) * 300 + 500, spacing[::-1], origin)
    msk = Image(_mask(shape, lo, hi), spacing[::-1], origin)
    return img, msk


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith(("equal", "zeros"))])
def test_plan_equals_resampleImage(name):
    from pyradiomics_amd import imageoperations
    shape, lo, hi, spacing, new, pad = CASES[name]
    img, msk = _images(name)
    ri, rm = imageoperations.resampleImage(img, msk, resampledPixelSpacing=new, padDistance=pad, deviceResident=False)
    plan = _one(name)
    assert plan.status.tolist() == [0] and plan.interpolator.tolist() == [3]
    assert tuple(plan.newsize[0]) == ri.array.shape == rm.array.shape
    assert tuple(plan.spacing[0][::-1]) == ri.spacing                                   # equal, not close
    assert tuple(np.array(img.origin) + plan.origin_shift[0]) == ri.origin
    # the grid: the host route's nearest-neighbour mask is the box's mask read at floor(start + o * step + 0.5)
    pos = [plan.start[0][d] + np.arange(plan.newsize[0][d]) * plan.step[0][d] for d in range(3)]
    assert all((p >= -0.5).all() and (p < n - 0.5).all() for p, n in zip(pos, shape)), "resampleImage clips the grid to the box"
    near = [np.clip(np.floor(p + 0.5).astype(int), 0, n - 1) for p, n in zip(pos, shape)]
    assert np.array_equal(msk.array[np.ix_(*near)], rm.array)
    kept = [d for d in range(3) if (hi[d] == lo[d]) or new[2 - d] == 0]
    for d in kept:
        assert plan.spacing[0][d] == spacing[d] and plan.step[0][d] == 1.0, (name, d)
    if name in ("extent-1-z", "extent-1-x", "zero-keeps-y"):
        assert kept


def test_the_cases_cover_what_they_claim():
    up = _one("mixed")
    assert (up.step[0] < 1).any() and (up.step[0] > 1).any()                            # an axis up-, another down-sampled
    shape, lo, hi, spacing, new, pad = CASES["faces"]
    free = np.array(spacing) / np.array(new)[::-1]
    L = np.floor((np.array(lo) - 0.5) * free - pad)
    U = np.ceil((np.array(hi) + 1 - 0.5) * free + pad)
    assert (L < 0).any() and (U > np.ceil(np.array(shape) * free) - 1).any()            # both clips
    assert (_one("up").step[0] <= 1).all() and (_one("down").step[0] >= 1).all()


@pytest.mark.parametrize("name", ["equal-x4", "equal-grow", "equal-edges", "zeros-are-crop"])
def test_equal_spacing_is_the_aligned_crop(name):
    from pyradiomics_amd import imageoperations
    shape, lo, hi, spacing, new, pad = CASES[name]
    img, msk = _images(name)
    plan = _one(name)
    a_lo, a_hi = imageoperations.alignedBox(np.array(lo), np.array(hi), shape)           # cropToTumorMask's device box, pad 0
    assert plan.status.tolist() == [0] and plan.interpolator.tolist() == [0]
    assert plan.step[0].tolist() == [1.0, 1.0, 1.0] and plan.start[0].tolist() == [float(v) for v in a_lo]
    assert plan.newsize[0].tolist() == (a_hi - a_lo + 1).tolist()
    assert tuple(plan.spacing[0]) == tuple(spacing)
    assert plan.newsize[0][2] % 4 == 0 or plan.newsize[0][2] == shape[2]
    # resampleImage's own crop (the host route: the reference's exact extent) is this box without the extra columns
    ri, rm = imageoperations.resampleImage(img, msk, resampledPixelSpacing=new, padDistance=pad, deviceResident=False)
    assert ri.array.shape[:2] == tuple(plan.newsize[0][:2]) and ri.spacing == tuple(spacing[::-1])
    assert ri.origin[1:] == tuple(np.array(img.origin) + plan.origin_shift[0])[1:]
    extra = lo[2] - a_lo[2]
    assert np.array_equal(img.array[tuple(slice(a, b + 1) for a, b in zip(a_lo, a_hi))][:, :, extra:extra + ri.array.shape[2]],
                          ri.array)
    if name == "equal-x4":
        assert ri.array.shape == tuple(plan.newsize[0]) and ri.origin == tuple(np.array(img.origin) + plan.origin_shift[0])
    if name == "equal-grow":
        assert plan.newsize[0][2] == 8 and extra == 0                                   # grown to the right first
    if name == "equal-edges":
        assert plan.newsize[0][2] == 6 and extra == 1                                   # the row is used up: short at both edges


def test_an_empty_mask_keeps_its_box():
    from pyradiomics_amd import engine
    sizes = [(5, 6, 7), (9, 12, 14)]
    shape, lo, hi, spacing, new, pad = CASES["up"]
    plan = engine.batch_resample_plan(sizes, [sizes[0], lo], [(-1, -1, -1), hi], spacing, new, pad)
    assert plan.status.tolist() == [engine.RESAMPLE_EMPTY, 0] and plan.interpolator.tolist() == [0, 3]
    assert plan.newsize[0].tolist() == [5, 6, 7] and plan.start[0].tolist() == [0, 0, 0] and plan.step[0].tolist() == [1, 1, 1]
    assert tuple(plan.spacing[0]) == tuple(spacing) and plan.origin_shift[0].tolist() == [0, 0, 0]
    one = _one("up")
    for a, b in zip(plan, one):                                                         # a ROI does not depend on its neighbours
        assert np.array_equal(a[1:], b)


def test_per_roi_spacing_and_interpolators():
    from pyradiomics_amd import engine
    names = ["up", "down", "equal-grow"]
    sizes, lo, hi, spacing = ([CASES[n][i] for n in names] for i in range(4))
    plan = engine.batch_resample_plan(sizes, lo, hi, spacing, (1.0, 1.0, 1.0), 2, ["sitkLinear", 3, "sitkBSpline"])
    assert plan.interpolator.tolist() == [1, 3, 3]
    for b, n in enumerate(names):
        one = engine.batch_resample_plan([sizes[b]], [lo[b]], [hi[b]], spacing[b], (1.0, 1.0, 1.0), 2)
        assert np.array_equal(plan.newsize[b], one.newsize[0]) and np.array_equal(plan.start[b], one.start[0])
    assert engine.batch_resample_plan(sizes, lo, hi, spacing, (1.0, 1.0, 1.0), 2, "sitkNearestNeighbor").interpolator.tolist() == [0] * 3
    assert engine.batch_resample_plan(sizes, lo, hi, spacing, (1.0, 1.0, 1.0), 2, 2).interpolator.tolist() == [1] * 3


def test_python_argument_errors():
    from pyradiomics_amd import engine
    shape, lo, hi, spacing, new, pad = CASES["up"]
    plan = engine.batch_resample_plan
    with pytest.raises(NotImplementedError, match="interpolator"):
        plan([shape], [lo], [hi], spacing, new, pad, "sitkGaussian")
    with pytest.raises(NotImplementedError, match="interpolator"):
        plan([shape], [lo], [hi], spacing, new, pad, 4)
    with pytest.raises(AssertionError, match="dimensionality"):
        plan([shape], [lo], [hi], spacing, (1.0, 1.0), pad)
    with pytest.raises(ValueError, match="spacing"):
        plan([shape], [lo], [hi], (1.0, 1.0), new, pad)
    with pytest.raises(ValueError, match="spacing must be > 0"):
        plan([shape], [lo], [hi], (1.0, 0.0, 1.0), new, pad)
    with pytest.raises(ValueError, match="resampledPixelSpacing"):
        plan([shape], [lo], [hi], spacing, (1.0, -1.0, 1.0), pad)
    with pytest.raises(ValueError, match="leaves its box"):
        plan([shape], [lo], [(5, 8, 14)], spacing, new, pad)
    with pytest.raises(ValueError, match="lower bounds"):
        plan([shape, shape], [lo], [hi], spacing, new, pad)
    with pytest.raises(ValueError, match="one per ROI"):
        plan([shape], [lo], [hi], spacing, new, pad, [3, 3])
    with pytest.raises(ValueError, match="resampledPixelSpacing"):
        engine.resample_batch([], [], None)
    import torch
    host = torch.zeros(8)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        engine.mask_boxes_batch(host.to(torch.uint8), [(2, 2, 2)])
    with pytest.raises(ValueError, match="CUDA/HIP"):
        engine.resample_boxes_batch(host, [(2, 2, 2)], [(0, 0, 0)], [(1, 1, 1)], [(2, 2, 2)])
    with pytest.raises(ValueError, match="works out voxelVolume itself"):
        engine.roi_features_batch_resampled([], [], resampledPixelSpacing=(1, 1, 1), voxelVolume=2.0)


# ---- the C calls: argument errors come back before anything is launched -------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


_BUF = np.zeros(4096, dtype=np.float64)      # stands in for every device pointer


def _call(lib, null=(), dtype=0, B=2, sizes=((2, 2, 2), (2, 3, 2)), off=(0, 8), start=None, step=None, newsize=((2, 2, 2), (3, 3, 3)),
          interp=(3, 0), out_off=(0, 8), mask=True):
    keep = []

    def arr(name, a, dt):
        if name in null:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as({np.intc: IP, np.int64: LP}[dt]) if dt in (np.intc, np.int64) else C.c_void_p(a.ctypes.data)
    dev = lambda name: None if name in null else C.c_void_p(_BUF.ctypes.data)
    verdict = np.full(max(B, 1), -7, dtype=np.intc)
    rc = lib.prad_batch_resample_dev(dev("in"), dtype, dev("mask") if mask else None, arr("sizes", sizes, np.intc),
                                     arr("off", off, np.int64), B, arr("start", np.zeros((2, 3)) if start is None else start, np.float64),
                                     arr("step", np.ones((2, 3)) if step is None else step, np.float64),
                                     arr("newsize", newsize, np.intc), arr("interp", interp, np.intc),
                                     arr("out_off", out_off, np.int64), dev("out"), dev("out_mask") if mask else None,
                                     None if "verdict" in null else verdict.ctypes.data_as(IP), None)
    return rc, verdict


@pytest.mark.parametrize("kw", [
    dict(null=("in",)), dict(null=("sizes",)), dict(null=("off",)), dict(null=("start",)), dict(null=("step",)),
    dict(null=("newsize",)), dict(null=("interp",)), dict(null=("out_off",)), dict(null=("out",)), dict(null=("verdict",)),
    dict(null=("mask",)), dict(null=("out_mask",)), dict(dtype=4), dict(dtype=-1), dict(B=-1),
    dict(sizes=((2, 2, 2), (2, 0, 2))), dict(newsize=((2, 2, 2), (3, 0, 3))), dict(interp=(3, 2)), dict(interp=(-1, 0)),
    dict(off=(0, -8)), dict(out_off=(-1, 8)), dict(out_off=(0, 7)),
    dict(start=((0, 0, 0), (0, np.nan, 0))), dict(step=((1, 1, 1), (1, np.inf, 1))),
], ids=lambda kw: "-".join("%s=%s" % (k, v) for k, v in kw.items()).replace(" ", "").replace("(", "").replace(")", "").replace("'", ""))
def test_resample_argument_errors(lib, kw):
    rc, verdict = _call(lib, **kw)
    assert rc == ARG, (kw, lib.prad_last_error().decode())
    assert (verdict == -7).all()                                                        # nothing was decided, nothing ran


def test_an_empty_batch_is_a_valid_call(lib):
    rc, _ = _call(lib, B=0, null=("in", "sizes", "off", "start", "step", "newsize", "interp", "out_off", "out", "verdict"), mask=False)
    assert rc == OK and lib.prad_last_path().decode() == "batch"
    assert lib.prad_batch_mask_boxes_dev(None, None, None, 0, None, None) == OK


def test_boxes_above_the_cap_get_verdict_8_without_a_launch(lib):
    cap = lib.prad_batch_resample_max_vox()
    assert cap == lib.prad_batch_max_vox() == 65280
    big = ((41, 40, 40), (1, 1, cap + 1))
    rc, verdict = _call(lib, sizes=big, off=(0, 41 * 40 * 40))
    assert rc == OK and verdict.tolist() == [8, 8]


@pytest.mark.parametrize("kw", [dict(null=("mask",)), dict(null=("sizes",)), dict(null=("off",)), dict(null=("boxes",)), dict(B=-1),
                                dict(sizes=((2, 2, 2), (2, 0, 2))), dict(off=(0, -8))], ids=str)
def test_mask_boxes_argument_errors(lib, kw):
    null = kw.get("null", ())
    sizes = np.ascontiguousarray(kw.get("sizes", ((2, 2, 2), (2, 3, 2))), dtype=np.intc)
    off = np.ascontiguousarray(kw.get("off", (0, 8)), dtype=np.int64)
    boxes = np.full((2, 7), -7, dtype=np.intc)
    rc = lib.prad_batch_mask_boxes_dev(None if "mask" in null else C.c_void_p(_BUF.ctypes.data),
                                       None if "sizes" in null else sizes.ctypes.data_as(IP),
                                       None if "off" in null else off.ctypes.data_as(LP), kw.get("B", 2),
                                       None if "boxes" in null else boxes.ctypes.data_as(IP), None)
    assert rc == ARG and (boxes == -7).all()

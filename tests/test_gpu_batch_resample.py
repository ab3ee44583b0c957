"""GPU: the batched resampling step (csrc/kernels_batch_resample.h: batch_mask_boxes_kernel, batch_bspline_prefilter_kernel,
batch_resample_kernel) through engine.mask_boxes_batch, engine.resample_boxes_batch and engine.resample_batch.

Raw call   the case table of tests/resample_reference.py -- every 3-D case of the groups prefilter, geometry, mirror, ties and
           integer, and the 1-D cases of `unfused` as 1 x 1 x N boxes (the single call itself right-aligns a 1-D image in three
           slots) -- in ONE batched call per dtype with a mixed interpolator vector, masks riding along: bit for bit
           engine.resample box by box, image and mask.  The float outputs (and the integer ones) also go to
           resample_reference.assert_case: the long-double reference under the bounds that module derives, independently of the
           single route.
Fallback   the float32 `stride` case (130 x 128 x 127 > batch_max_vox()) in a batch with small ones: verdict 8, route "mixed",
           every ROI still equal to the single route.
Tiny       300 boxes of 2 x 2 x 2 (more ROIs than one 1024-item chunk of the evaluation holds, more than one workgroup of every
           kernel): every slice at its own offset, the sentinel behind the last ROI of preallocated outputs untouched.
Boxes      mask_boxes_batch against numpy on boxes from 1 x 1 x 1 to 5 x 40 x 66: empty, one voxel in each corner, full, one
           blob touching each face.
Planned    resample_batch per ROI against imageoperations.resampleImage(deviceResident=True) on the box as an Image: arrays and
           spacing bit for bit, origin = the Image's origin + origin_shift; one batch mixes resampled, cropped and empty ROIs.
           resampleImage's own crop keeps the reference's exact extent while the batched crop is cropToTumorMask's device box
           (x extent grown to a multiple of four): a crop ROI whose x extent is already one is equal to resampleImage's, the
           other is compared with cropToTumorMask(deviceResident=True)."""
import numpy as np
import pytest

import resample_reference as rr

pytestmark = pytest.mark.gpu

GROUP_PREFIXES = ("prefilter:", "geometry:", "mirror:", "ties", "unfused", "integer:")
DTYPES = ("float64", "float32", "int32", "int16")


def _names(dtype):
    names = [n for g, ns in rr.GROUPS.items() if g.startswith(GROUP_PREFIXES) for n in ns if rr.spec(n)["dtype"] == dtype]
    assert all(len(rr.spec(n)["shape"]) == 3 or n.startswith("unfused") for n in names)
    return names


def _box3(a):
    """a 1-D case as the 1 x 1 x N box the single call makes of it"""
    a = np.asarray(a)
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def _geo3(start, step, newsize):
    k = 3 - len(newsize)
    return np.r_[[0.0] * k, start], np.r_[[1.0] * k, step], np.r_[[1] * k, newsize].astype(np.intc)


def _case_mask(name, shape):
    rng = np.random.default_rng(rr.spec(name)["seed"] ^ 0x5EED)
    return rng.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), size=shape)


_cache = {}


def _raw(dtype):
    """one batched call over every case of a dtype, and the single route box by box: computed once"""
    if dtype not in _cache:
        import torch
        from pyradiomics_amd import engine
        names = _names(dtype)
        boxes, masks, geo, codes = [], [], [], []
        for n in names:
            x, start, step, newsize, interp = rr.case(n)
            boxes.append(torch.from_numpy(np.array(_box3(x))).cuda())
            masks.append(torch.from_numpy(_case_mask(n, boxes[-1].shape)).cuda())
            geo.append(_geo3(start, step, newsize))
            codes.append(interp)
        start, step, newsize = (np.stack([g[i] for g in geo]) for i in range(3))
        out, out_m, verdict = engine.resample_boxes_batch(boxes, None, start, step, newsize, codes, masks=masks, return_verdict=True)
        route, path = engine.last_batch_route(), engine.last_path()
        kernel_ms = engine.last_kernel_ms("batch_resample")
        single = []
        for n, box, m in zip(names, boxes, masks):
            x, s0, st, ns, interp = rr.case(n)
            si = engine.resample(torch.from_numpy(np.array(x)).cuda(), s0, st, ns, interp).cpu().numpy()
            sm = engine.resample(m.to(torch.int16), *_geo3(s0, st, ns), 0).cpu().numpy()
            single.append((si, sm))
        _cache[dtype] = (names, newsize, out.cpu().numpy(), out_m.cpu().numpy(), verdict, route, path, kernel_ms, single)
    return _cache[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_call_equals_the_single_route(dtype):
    names, newsize, out, out_m, verdict, route, path, kernel_ms, single = _raw(dtype)
    assert len(names) >= (100 if dtype.startswith("float") else 6)
    assert set(rr.spec(n)["interp"] for n in names) == {0, 1, 3}                        # a mixed interpolator vector
    assert (verdict == 0).all() and route == "batch" and path == "batch" and kernel_ms > 0
    assert out.dtype == np.dtype(dtype) and out_m.dtype == np.uint8
    off = np.concatenate([[0], np.cumsum(newsize.astype(np.int64).prod(1))])
    assert out.size == off[-1] == out_m.size
    bad = []
    for b, (n, (si, sm)) in enumerate(zip(names, single)):
        got, got_m = out[off[b]:off[b + 1]], out_m[off[b]:off[b + 1]]
        if got.tobytes() != np.ascontiguousarray(si).tobytes() or not np.array_equal(got_m, sm.ravel()):
            bad.append(n)
    assert not bad, (len(bad), bad[:10])


@pytest.mark.skipif(not rr.AVAILABLE, reason=rr.SKIP_REASON)
@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_call_against_the_long_double_reference(dtype):
    names, newsize, out, _, _, _, _, _, _ = _raw(dtype)
    off = np.concatenate([[0], np.cumsum(newsize.astype(np.int64).prod(1))])
    ratios = {}
    for b, n in enumerate(names):
        rr.assert_case(n, out[off[b]:off[b + 1]].reshape(rr.spec(n)["newsize"]), ratios, "batched " + dtype, who="batched")
    rr.report("batched resampling, " + dtype, ratios)


def test_a_box_above_the_cap_takes_the_single_route():
    import torch
    from pyradiomics_amd import engine
    small = rr.GROUPS["geometry:float32:bspline"][:2] + rr.GROUPS["geometry:float32:linear"][:1]
    names = [small[0], "stride-bspline-float32"] + small[1:]
    cases = [rr.case(n) for n in names]
    assert cases[1][0].size > engine.batch_max_vox() == engine.batch_resample_max_vox()
    boxes = [torch.from_numpy(np.array(c[0])).cuda() for c in cases]
    masks = [torch.from_numpy(_case_mask(n, c[0].shape)).cuda() for n, c in zip(names, cases)]
    start, step, newsize = (np.stack([np.asarray(c[i]) for c in cases]) for i in (1, 2, 3))
    codes = [c[4] for c in cases]
    out, out_m, verdict = engine.resample_boxes_batch(boxes, None, start, step, newsize, codes, masks=masks, return_verdict=True)
    assert verdict.tolist() == [0, 8, 0, 0] and engine.last_batch_route() == "mixed"
    out, out_m = out.cpu().numpy(), out_m.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(newsize.astype(np.int64).prod(1))])
    for b, c in enumerate(cases):
        si = engine.resample(boxes[b], c[1], c[2], c[3], c[4]).cpu().numpy()
        sm = engine.resample(masks[b].to(torch.int16), c[1], c[2], c[3], 0).cpu().numpy()
        assert out[off[b]:off[b + 1]].tobytes() == si.tobytes(), names[b]
        assert np.array_equal(out_m[off[b]:off[b + 1]], sm.ravel()), names[b]


def test_many_tiny_boxes_land_at_their_own_offsets():
    import torch
    from pyradiomics_amd import engine
    B, SENTINEL = 300, 64
    rng = np.random.default_rng(300)
    flat = torch.from_numpy((rng.standard_normal(B * 8) * 300 + 500).astype(np.float32)).cuda()
    fmask = torch.from_numpy(rng.integers(0, 2, B * 8).astype(np.uint8)).cuda()
    sizes = np.full((B, 3), 2, dtype=np.intc)
    newsize = np.tile(np.array([[3, 3, 3], [2, 4, 3], [5, 2, 2]], dtype=np.intc), (B // 3, 1))
    start = np.tile(np.array([[-0.25, -0.25, -0.25], [0.0, -0.4, -0.25], [-0.5, 0.0, 0.1]]), (B // 3, 1))
    step = np.tile(np.array([[0.5, 0.5, 0.5], [1.0, 0.45, 0.5], [0.4, 1.0, 0.7]]), (B // 3, 1))
    codes = np.tile(np.array([3, 1, 3, 0, 3], dtype=np.intc), B // 5)
    W = int(newsize.astype(np.int64).prod(1).sum())
    assert W > 4 * 1024                                           # several chunks of the evaluation, some forty ROIs in each
    out = torch.full((W + SENTINEL,), -7.5, dtype=torch.float32, device="cuda")
    out_m = torch.full((W + SENTINEL,), 77, dtype=torch.uint8, device="cuda")
    res, res_m = engine.resample_boxes_batch(flat, sizes, start, step, newsize, codes, masks=fmask, out=out, out_masks=out_m)
    assert res.data_ptr() == out.data_ptr() and res_m.data_ptr() == out_m.data_ptr() and engine.last_batch_route() == "batch"
    host, host_m = out.cpu().numpy(), out_m.cpu().numpy()
    assert (host[W:] == -7.5).all() and (host_m[W:] == 77).all()
    off = np.concatenate([[0], np.cumsum(newsize.astype(np.int64).prod(1))])
    for b in range(B):
        box, m = flat[8 * b:8 * b + 8].view(2, 2, 2), fmask[8 * b:8 * b + 8].view(2, 2, 2)
        si = engine.resample(box, start[b], step[b], newsize[b], int(codes[b])).cpu().numpy()
        sm = engine.resample(m.to(torch.int16), start[b], step[b], newsize[b], 0).cpu().numpy()
        assert host[off[b]:off[b + 1]].tobytes() == si.tobytes(), b
        assert np.array_equal(host_m[off[b]:off[b + 1]], sm.ravel()), b


# ---- mask_boxes_batch ---------------------------------------------------------------------------------------------------------
BOX_SHAPES = [(1, 1, 1), (1, 1, 5), (2, 3, 4), (3, 7, 1), (40, 5, 3), (5, 40, 66)]


def _box_masks(shape):
    masks = [np.zeros(shape, dtype=np.uint8), np.ones(shape, dtype=np.uint8)]
    for corner in np.ndindex(2, 2, 2):
        m = np.zeros(shape, dtype=np.uint8)
        m[tuple(c * (s - 1) for c, s in zip(corner, shape))] = 3                       # (any non-zero value is ROI)
        masks.append(m)
    mid = [s // 2 for s in shape]
    for axis in range(3):
        for end in (0, 1):                                                             # a blob from the middle to one face
            m = np.zeros(shape, dtype=np.uint8)
            sl = [slice(c, c + 1) for c in mid]
            sl[axis] = slice(0, mid[axis] + 1) if end == 0 else slice(mid[axis], shape[axis])
            m[tuple(sl)] = 1
            masks.append(m)
    return masks


def test_mask_boxes_equal_numpy():
    import torch
    from pyradiomics_amd import engine
    masks = [m for shape in BOX_SHAPES for m in _box_masks(shape)]
    lo, hi, count = engine.mask_boxes_batch([torch.from_numpy(m).cuda() for m in masks])
    assert engine.last_path() == "batch" and lo.shape == hi.shape == (len(masks), 3) and count.shape == (len(masks),)
    for b, m in enumerate(masks):
        idx = np.argwhere(m != 0)
        assert count[b] == len(idx), b
        if len(idx):
            assert lo[b].tolist() == idx.min(0).tolist() and hi[b].tolist() == idx.max(0).tolist(), (b, m.shape)
        else:
            assert lo[b].tolist() == list(m.shape) and hi[b].tolist() == [-1, -1, -1]
    # the flat form, bool masks and more ROIs than lanes in a workgroup
    rng = np.random.default_rng(7)
    many = rng.random((300, 2, 3, 4)) < 0.2
    lo, hi, count = engine.mask_boxes_batch(torch.from_numpy(many.reshape(-1)).cuda(), np.tile([[2, 3, 4]], (300, 1)))
    for b in range(300):
        idx = np.argwhere(many[b])
        assert count[b] == len(idx)
        if len(idx):
            assert lo[b].tolist() == idx.min(0).tolist() and hi[b].tolist() == idx.max(0).tolist()


# ---- resample_batch against resampleImage ---------------------------------------------------------------------------------------
def _roi(shape, lo, hi):
    m = np.zeros(shape, dtype=np.uint8)
    m[tuple(slice(a, b + 1) for a, b in zip(lo, hi))] = 1
    m[tuple(l + 1 if h - l >= 2 else l for l, h in zip(lo, hi))] = 0                   # (a hole: not a solid block)
    return m


# (shape, mask lo, mask hi, spacing zyx, kind)
ROIS = [
    ((12, 14, 16), (4, 4, 5), (7, 9, 10), (2.5, 0.6, 0.8), "resample"),        # z up, y and x differently
    ((20, 18, 16), (6, 5, 5), (13, 12, 10), (0.4, 0.45, 1.6), "resample"),     # z, y down, x up
    ((9, 12, 14), (3, 4, 5), (5, 8, 8), (1.0, 1.0, 1.0), "crop-x4"),           # equal spacing, x extent 4
    ((8, 9, 10), (0, 2, 0), (7, 8, 9), (1.5, 0.75, 0.6), "resample"),          # the bounding box touches faces: both clips
    ((9, 12, 14), (3, 4, 5), (5, 8, 9), (1.0, 1.0, 1.0), "crop-grow"),         # equal spacing, x extent 5 -> 8
    ((7, 12, 11), (3, 3, 2), (3, 8, 7), (5.0, 0.8, 0.7), "resample"),          # one slice: z keeps 5.0
    ((5, 6, 7), None, None, (2.0, 0.5, 0.5), "empty"),
    ((30, 30, 30), (12, 11, 13), (17, 18, 16), (1.25, 0.8, 0.8), "resample"),
]
NEW = (1.0, 1.0, 1.0)


@pytest.mark.parametrize("dtype,interpolator", [("float32", "sitkBSpline"), ("int16", "sitkBSpline"), ("float64", "sitkLinear"),
                                                ("int32", "sitkNearestNeighbor"), ("float64", 3)])
def test_resample_batch_equals_resampleImage(dtype, interpolator):
    import torch
    from pyradiomics_amd import engine, imageoperations
    from pyradiomics_amd.image import Image
    rng = np.random.default_rng(11)
    boxes, masks, origins = [], [], []
    for shape, lo, hi, spacing, kind in ROIS:
        boxes.append((rng.standard_normal(shape) * 300 + 500).astype(dtype))
        masks.append(np.zeros(shape, dtype=np.uint8) if kind == "empty" else _roi(shape, lo, hi))
        origins.append(tuple(rng.uniform(-50, 50, 3)))
    spacing = np.array([r[3] for r in ROIS])
    out, out_m, sizes, new_spacing, shift, status = engine.resample_batch(
        [torch.from_numpy(b).cuda() for b in boxes], [torch.from_numpy(m).cuda() for m in masks], spacing=spacing,
        resampledPixelSpacing=NEW, interpolator=interpolator, padDistance=3)
    assert engine.last_batch_route() == "batch"
    assert status.tolist() == [engine.RESAMPLE_EMPTY if r[4] == "empty" else 0 for r in ROIS]
    out, out_m = out.cpu().numpy(), out_m.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(sizes.astype(np.int64).prod(1))])
    assert out.dtype == np.dtype(dtype) and out.size == off[-1] == out_m.size
    for b, (shape, lo, hi, sp, kind) in enumerate(ROIS):
        got = out[off[b]:off[b + 1]].reshape(sizes[b])
        got_m = out_m[off[b]:off[b + 1]].reshape(sizes[b])
        origin = tuple(np.array(origins[b]) + shift[b])
        img, msk = Image(boxes[b], sp[::-1], origins[b]), Image(masks[b], sp[::-1], origins[b])
        if kind == "empty":
            with pytest.raises(ValueError):
                imageoperations.resampleImage(img, msk, resampledPixelSpacing=NEW, interpolator=interpolator, padDistance=3,
                                              deviceResident=True)
            assert got.tobytes() == boxes[b].tobytes() and not got_m.any() and origin == origins[b]
            assert tuple(new_spacing[b]) == tuple(sp)
            continue
        if kind == "crop-grow":                      # the device crop's box; resampleImage cuts the unaligned extent out of it
            ri, rm = imageoperations.cropToTumorMask(img, msk, padDistance=0, deviceResident=True)
            assert got.shape[2] == 8
        else:
            ri, rm = imageoperations.resampleImage(img, msk, resampledPixelSpacing=NEW, interpolator=interpolator, padDistance=3,
                                                   deviceResident=True)
        want, want_m = ri.device_tensor().cpu().numpy(), rm.device_tensor().cpu().numpy()
        assert got.shape == want.shape, (b, kind, got.shape, want.shape)
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (b, kind)
        assert np.array_equal(got_m, want_m), (b, kind)
        assert tuple(new_spacing[b][::-1]) == tuple(ri.spacing) and origin == tuple(ri.origin), (b, kind)
        if kind.startswith("crop"):
            assert tuple(new_spacing[b]) == tuple(sp) and got_m.any()
        else:
            assert got.shape != tuple(shape)

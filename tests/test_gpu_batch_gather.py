"""GPU: engine.gather_rois_batch (prad_batch_gather_dev, csrc/kernels_batch_gather.h) -- the boxes of many labels of one label
map packed into the batch layout in one launch -- against numpy slicing and `== label` on the host, array_equal throughout
(float images are compared as bytes: -0.0, NaN payloads and inf must survive)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IMAGE_DTYPES = [np.float32, np.float64, np.int32, np.int16, np.uint8]
LABEL_DTYPES = [np.uint8, np.int16, np.int32]


def _image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        img = rng.integers(info.min, int(info.max) + 1, n).astype(dtype)
    else:
        img = (rng.standard_normal(n) * 100).astype(dtype)
        special = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf], dtype=dtype)
        img[:: max(1, n // 37)] = np.resize(special, len(img[:: max(1, n // 37)]))
        # a NaN with a payload: its bits are data too
        bits = img.view(np.uint32 if dtype == np.float32 else np.uint64)
        bits[1] = 0x7FC12345 if dtype == np.float32 else 0x7FF8000000ABCDEF
    return img.reshape(shape)


def _expected(img, lab, labels, lo, hi):
    imgs, masks = [], []
    for l, a, b in zip(labels, lo, hi):
        sl = tuple(slice(int(x), int(y) + 1) for x, y in zip(a, b))
        if img is not None:
            imgs.append(np.ascontiguousarray(img[sl]).reshape(-1))
        if lab is not None:
            masks.append((lab[sl] == l).astype(np.uint8).reshape(-1))
    return (np.concatenate(imgs) if imgs else None), (np.concatenate(masks) if masks else None)


def _check(img, lab, labels, lo, hi, **kw):
    import torch
    from pyradiomics_amd import engine
    lo, hi = np.asarray(lo).reshape(-1, 3), np.asarray(hi).reshape(-1, 3)
    d_img = torch.from_numpy(img).cuda() if img is not None else None
    d_lab = torch.from_numpy(lab).cuda() if lab is not None else None
    gi, gm, sizes = engine.gather_rois_batch(d_img, d_lab, labels, lo, hi, **kw)
    assert np.array_equal(sizes, hi - lo + 1) and sizes.dtype == np.intc
    want_img = None if img is None else (img if img.dtype in (np.float32, np.float64, np.int32, np.int16) else img.astype(np.float64))
    wi, wm = _expected(want_img if kw.get("images", True) else None, lab if kw.get("masks", True) else None, labels, lo, hi)
    if wi is None:
        assert gi is None
    else:
        got = gi.cpu().numpy()
        assert got.dtype == wi.dtype and got.shape == wi.shape
        assert got.tobytes() == wi.tobytes()
    if wm is None:
        assert gm is None
    else:
        assert gm.dtype == torch.uint8
        assert np.array_equal(gm.cpu().numpy(), wm)
    return gi, gm, sizes


def test_labels_touching_every_face_and_a_corner():
    lab = np.zeros((5, 6, 7), dtype=np.int16)
    lab[0, 2:4, 2:5] = 1          # z = 0 face
    lab[4, 1:3, 3:6] = 2          # z = 4 face
    lab[1:3, 0, 1:4] = 3          # y = 0
    lab[2:4, 5, 2:6] = 4          # y = 5
    lab[1:4, 2:4, 0] = 5          # x = 0
    lab[1:3, 3:5, 6] = 6          # x = 6
    lab[3:5, 4:6, 5:7] = 7        # the far corner
    lab[0, 0, 0] = 8              # the near corner, one voxel
    img = _image(lab.shape, np.float32, 1)
    labels = list(range(1, 9))
    lo = [np.argwhere(lab == l).min(0) for l in labels]
    hi = [np.argwhere(lab == l).max(0) for l in labels]
    _check(img, lab, labels, lo, hi)


def test_whole_volume_box_and_single_voxel_box():
    lab = (np.random.default_rng(2).integers(0, 3, (5, 6, 7))).astype(np.uint8)
    img = _image(lab.shape, np.int16, 2)
    _check(img, lab, [1], [(0, 0, 0)], [(4, 5, 6)])                  # B = 1, the whole volume
    _check(img, lab, [2], [(3, 4, 5)], [(3, 4, 5)])                  # B = 1, one voxel
    _check(img, lab, [2, 1, 2], [(4, 5, 6), (0, 0, 0), (0, 0, 0)], [(4, 5, 6), (4, 5, 6), (0, 0, 0)])


def test_interleaved_labels_and_foreign_labels_inside_a_box():
    """two labels in a checkerboard share one box: each mask excludes the other's voxels; a third label inside the box is in
    neither; the same box asked for twice with different labels"""
    z, y, x = np.mgrid[0:6, 0:7, 0:9]
    lab = np.where((z + y + x) % 2 == 0, 11, 12).astype(np.int32)
    lab[2:4, 3:5, 4:6] = 99          # not in the request
    lab[0, :, :] = 0
    img = _image(lab.shape, np.float64, 3)
    gi, gm, sizes = _check(img, lab, [11, 12], [(1, 0, 0), (1, 0, 0)], [(5, 6, 8), (5, 6, 8)])
    m = gm.cpu().numpy().reshape(2, -1)
    assert not (m[0] & m[1]).any() and m[0].any() and m[1].any()
    assert int(m.sum()) == int(((lab == 11) | (lab == 12)).sum())      # the voxels of 99 are in neither
    _check(img, lab, [99, 12, 7], [(1, 2, 3), (2, 3, 4), (0, 0, 0)], [(4, 5, 6), (3, 4, 5), (2, 2, 2)])      # (7 does not occur)


@pytest.mark.parametrize("nx", [65, 7])
def test_clipped_alignment(nx):
    """x extents 1, 3, 4, 5, 63, 64, 65 at the left edge, in the middle and at the right edge of a row of 65 (and of 7: clipped
    at both edges), as the extractor asks for them: census bounds through imageoperations.alignedBox.  At the right edge the
    extension is clipped and the box's lo moves left."""
    from pyradiomics_amd import imageoperations
    shape = (3, 4, nx)
    lab = np.zeros(shape, dtype=np.int16)
    img = _image(shape, np.float32, 4)
    labels, lo, hi = [], [], []
    for ext in (1, 3, 4, 5, 63, 64, 65):
        if ext > nx:
            continue
        for x0 in sorted({0, (nx - ext) // 2, nx - ext}):
            labels.append(len(labels) + 1)
            lo.append((1, 1, x0))
            hi.append((2, 2, x0 + ext - 1))
    for l, a, b in zip(labels, lo, hi):
        lab[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1][::1, ::1, ::2] = l      # (boxes overlap: later labels overwrite)
    alo, ahi = imageoperations.alignedBox(np.array(lo), np.array(hi), shape)
    moved_left = [(a[2], b[2]) for a, b in zip(alo, lo) if a[2] < b[2]]
    assert moved_left, "no box had its extension clipped at the right edge"
    ext = ahi[:, 2] - alo[:, 2] + 1
    assert ((ext % 4 == 0) | ((alo[:, 2] == 0) & (ahi[:, 2] == nx - 1))).all()
    if nx == 7:
        assert ((alo[:, 2] == 0) & (ahi[:, 2] == nx - 1) & (ext % 4 != 0)).any()     # clipped at both edges
    _check(img, lab, labels, alo, ahi)


@pytest.mark.parametrize("ldt", LABEL_DTYPES)
@pytest.mark.parametrize("idt", IMAGE_DTYPES)
def test_dtypes(idt, ldt):
    shape = (6, 9, 11)
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 5, shape).astype(ldt)
    lab[0, 0, 0] = np.iinfo(ldt).max if ldt != np.int32 else 70000
    img = _image(shape, idt, 6)
    labels = [1, 2, 3, 4, int(lab[0, 0, 0])]
    lo = [(0, 0, 0), (1, 2, 3), (2, 0, 5), (0, 4, 1), (0, 0, 0)]
    hi = [(5, 8, 10), (4, 6, 9), (5, 8, 10), (3, 7, 2), (1, 1, 1)]
    _check(img, lab, labels, lo, hi)


def test_one_large_box_among_three_hundred_small_ones():
    """300 boxes of 2 x 2 x 2 to 6 x 5 x 7 and one of 41^3 (68 921 voxels: 68 chunks of 1024) in the middle of the table: the
    chunk-to-ROI lookup at every ROI boundary, chunks inside one box, chunks over dozens of boxes"""
    rng = np.random.default_rng(7)
    shape = (48, 50, 52)
    lab = rng.integers(0, 400, shape).astype(np.int16)
    img = _image(shape, np.float32, 8)
    labels, lo, hi = [], [], []
    for k in range(300):
        ext = np.array([rng.integers(2, 7), rng.integers(2, 6), rng.integers(2, 8)])
        a = np.array([rng.integers(0, s - e + 1) for s, e in zip(shape, ext)])
        labels.append(int(rng.integers(1, 400)))
        lo.append(a)
        hi.append(a + ext - 1)
    labels.insert(150, 77)
    lo.insert(150, np.array([3, 5, 7]))
    hi.insert(150, np.array([43, 45, 47]))
    assert int(np.prod(hi[150] - lo[150] + 1)) == 68921
    _check(img, lab, labels, lo, hi)
    _check(img, lab, labels[::-1], lo[::-1], hi[::-1])           # (another table right after: nothing of the first one is reused)


def test_omitted_outputs_and_repeated_tables():
    import torch
    from pyradiomics_amd import engine
    rng = np.random.default_rng(9)
    shape = (10, 11, 12)
    lab = rng.integers(0, 6, shape).astype(np.int16)
    img = _image(shape, np.float64, 10)
    labels, lo, hi = [1, 2, 5], [(0, 0, 0), (2, 3, 4), (5, 5, 5)], [(4, 5, 6), (9, 10, 11), (9, 9, 9)]
    gi, gm, sizes = _check(img, lab, labels, lo, hi)
    oi, om, osz = _check(img, lab, labels, lo, hi, masks=False)
    assert om is None and torch.equal(oi.view(torch.int64), gi.view(torch.int64)) and np.array_equal(osz, sizes)
    mi, mm, msz = _check(img, lab, labels, lo, hi, images=False)
    assert mi is None and torch.equal(mm, gm) and np.array_equal(msz, sizes)
    # without the other tensor at all (what the extractor does: masks once, then one image after the other with one table)
    d_img, d_lab = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
    _, m2, _ = engine.gather_rois_batch(None, d_lab, labels, lo, hi, masks=True, images=False)
    for other in (img, -img, img.astype(np.float32)):
        i2, none, _ = engine.gather_rois_batch(torch.from_numpy(other).cuda(), None, labels, lo, hi, masks=False, images=True)
        assert none is None and i2.cpu().numpy().tobytes() == _expected(other, None, labels, lo, hi)[0].tobytes()
    assert torch.equal(m2, gm)


def test_errors_launch_nothing():
    import torch
    from pyradiomics_amd import engine
    img = torch.zeros((5, 6, 7), dtype=torch.float32, device="cuda")
    lab = torch.zeros((5, 6, 7), dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError, match="leaves the volume"):
        engine.gather_rois_batch(img, lab, [1], [(0, 0, 0)], [(4, 5, 7)])
    with pytest.raises(ValueError, match="leaves the volume"):
        engine.gather_rois_batch(img, lab, [1, 2], [(0, 0, 0), (-1, 0, 0)], [(1, 1, 1), (1, 1, 1)])
    with pytest.raises(ValueError, match="hi < lo"):
        engine.gather_rois_batch(img, lab, [1], [(2, 2, 2)], [(3, 1, 3)])
    with pytest.raises(ValueError):
        engine.gather_rois_batch(img, lab.cpu(), [1], [(0, 0, 0)], [(1, 1, 1)])      # two devices
    with pytest.raises(ValueError):
        engine.gather_rois_batch(img.cpu(), lab.cpu(), [1], [(0, 0, 0)], [(1, 1, 1)])
    with pytest.raises(ValueError):
        engine.gather_rois_batch(img, lab[:, :, :6], [1], [(0, 0, 0)], [(1, 1, 1)])  # shapes differ
    with pytest.raises(ValueError):
        engine.gather_rois_batch(img, lab.to(torch.float32), [1], [(0, 0, 0)], [(1, 1, 1)])
    # the library refuses the same on its own, before launching (PRAD_E_ARG -> ValueError)
    import ctypes as C
    from pyradiomics_amd import _lib
    lib = _lib.load()
    out_i, out_m = torch.full((64,), 7.0, device="cuda"), torch.full((64,), 9, dtype=torch.uint8, device="cuda")
    size = np.array([5, 6, 7], dtype=np.intc)

    def call(lo, box, off, labels=(1, 1)):
        lo, box = np.array(lo, dtype=np.intc), np.array(box, dtype=np.intc)
        off, labels = np.array(off, dtype=np.int64), np.array(labels, dtype=np.intc)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        return lib.prad_batch_gather_dev(C.c_void_p(img.data_ptr()), 0, C.c_void_p(lab.data_ptr()), 3, ip(size), len(off), ip(labels),
                                         ip(lo), ip(box), off.ctypes.data_as(C.POINTER(C.c_longlong)), C.c_void_p(out_i.data_ptr()),
                                         C.c_void_p(out_m.data_ptr()), None)
    assert call([(0, 0, 0), (0, 0, 6)], [(2, 2, 2), (1, 1, 2)], [0, 8]) == _lib.PRAD_E_ARG       # leaves the volume
    assert call([(0, 0, 0), (0, 0, 0)], [(2, 2, 2), (1, -1, 2)], [0, 8]) == _lib.PRAD_E_ARG      # negative extent
    assert call([(0, 0, 0), (0, 0, 0)], [(2, 2, 2), (1, 1, 2)], [8, 0]) == _lib.PRAD_E_ARG       # offsets decrease
    assert call([(0, 0, 0), (0, 0, 0)], [(2, 2, 2), (1, 1, 2)], [0, 7]) == _lib.PRAD_E_ARG       # the pieces overlap
    torch.cuda.synchronize()
    assert bool((out_i == 7.0).all()) and bool((out_m == 9).all())                                # nothing was written
    assert call([(0, 0, 0), (0, 0, 0)], [(2, 2, 2), (1, 1, 2)], [0, 10]) == _lib.PRAD_OK         # (a gap between the pieces is fine)
    torch.cuda.synchronize()
    assert bool((out_i[:8] == 0).all()) and bool((out_i[8:10] == 7.0).all()) and bool((out_i[10:12] == 0).all())


def test_feeding_the_batch_route():
    """roi_features_batch on the gathered buffers == roi_features_batch on lists built by torch slicing, bit for bit"""
    import torch
    from pyradiomics_amd import engine
    rng = np.random.default_rng(12)
    shape = (14, 15, 16)
    z, y, x = np.mgrid[0:14, 0:15, 0:16]
    img = (30 * np.sin(z / 3.0) + 20 * np.cos(y / 4.0) + 2.0 * x + rng.normal(0, 5, shape)).astype(np.float32)
    lab = np.zeros(shape, dtype=np.int16)
    lab[1:7, 2:8, 0:8] = 1
    lab[5:12, 6:13, 4:12] = 2          # overlaps label 1's box
    lab[8:13, 1:6, 8:16] = 3
    lab[2:5, 9:14, 12:16][rng.random((3, 5, 4)) < 0.7] = 4
    labels = [1, 2, 3, 4]
    lo = [np.argwhere(lab == l).min(0) for l in labels]
    hi = [np.argwhere(lab == l).max(0) for l in labels]
    d_img, d_lab = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
    gi, gm, sizes = engine.gather_rois_batch(d_img, d_lab, labels, lo, hi)
    got, gst = engine.roi_features_batch(gi, gm, sizes, binWidth=5, voxelArrayShift=10, voxelVolume=0.5)
    I = [d_img[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1].contiguous() for a, b in zip(lo, hi)]
    M = [(d_lab[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1].contiguous() == l) for l, a, b in zip(labels, lo, hi)]
    want, wst = engine.roi_features_batch(I, M, binWidth=5, voxelArrayShift=10, voxelVolume=0.5)
    assert gst == wst == [1, 1, 1, 1]
    for cls in want:
        assert got[cls].tobytes() == want[cls].tobytes(), cls
        assert not np.isnan(got[cls][:, 0]).any()

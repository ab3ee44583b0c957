"""GPU: engine.lbp2d_batch (prad_batch_lbp2d_dev, ONE launch) against engine.lbp2d on every box alone -- exact equality: both
kernels run the same device function on the box, cells beyond its edge as 0.0 -- and, through it, against tests/lbp_reference.py.

Batches: B = 1; a ragged batch of 40 boxes with a 1-voxel box, boxes with one and two extent-1 axes, extents around the tile
seams and one (41, 41, 41) box (68 921 voxels: above the 65 280-voxel cap of the LDS routes of the other batched kernels, no cap
here).  All four dtypes, three axes; methods and (P, R) rotate over the cases, the halo 2 and 8 settings included."""
import numpy as np
import pytest

import lbp_reference as lr

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "int32", "int16"]
FIXED = [(1, 1, 1), (1, 1, 5), (7, 1, 1), (1, 9, 1), (3, 2, 2), (1, 17, 65), (17, 1, 33), (9, 15, 1), (5, 9, 70), (41, 41, 41)]


def _shapes():
    rng = np.random.default_rng(40)
    return FIXED + [tuple(int(v) for v in rng.integers(1, 21, 3)) for _ in range(40 - len(FIXED))]


def _boxes(dtype, shapes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for s in shapes:
        if dtype.startswith("float"):
            v = np.round(rng.normal(40.0, 25.0, s), 1)
            v[rng.random(s) < 0.3] = 40.0
        else:
            v = rng.integers(-3, 4, s) * 100
        out.append(v.astype(dtype))
    return out


def _split(flat, sizes):
    off = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64).prod(1))])
    return [flat[off[b]:off[b + 1]].reshape(tuple(sizes[b])) for b in range(len(sizes))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ragged_batch_equals_the_single_call_per_box(axis, dtype):
    import torch
    from pyradiomics_amd import engine
    shapes = _shapes()
    assert len(shapes) == 40 and max(int(np.prod(s)) for s in shapes) > 65280
    boxes = _boxes(dtype, shapes, 3 * axis + DTYPES.index(dtype))
    dev = [torch.from_numpy(b).cuda() for b in boxes]
    k = 3 * axis + DTYPES.index(dtype)
    P, R = [(8, 1), (8, 1.5), (16, 2), (9, 1), (3, 0.5), (24, 3), (1, 1)][k % 7]
    method = lr.METHODS[k % 3] if not (dtype == "int16" and P > 15) else "uniform"
    image, name, sizes = engine.lbp2d_batch(dev, None, R, P, method, axis)
    assert name == "lbp-2D" and image.dtype == torch.float64 and engine.last_batch_route() == "batch"
    assert [tuple(s) for s in sizes] == shapes
    got = _split(image.cpu().numpy(), sizes)
    for b, box in enumerate(boxes):
        single = engine.lbp2d(dev[b], R, P, method, axis).cpu().numpy()
        assert np.array_equal(got[b], single.astype(np.float64)), (b, shapes[b])
        if box.size <= 4000:          # (the reference on the small boxes; the single call is held to it everywhere else)
            assert np.array_equal(single, lr.lbp_volume(box, P, R, method, axis)), (b, shapes[b])


def test_one_box_a_wide_halo_and_out():
    import torch
    from pyradiomics_amd import engine
    box = _boxes("int16", [(6, 21, 35)], 5)[0]
    dev = torch.from_numpy(box).cuda()
    for axis in (0, 1, 2):
        image, _, sizes = engine.lbp2d_batch([dev], None, 8, 24, "uniform", axis)                 # ceil(R) = 8
        assert engine.last_batch_route() == "batch"
        assert np.array_equal(image.cpu().numpy().reshape(box.shape), lr.lbp_volume(box, 24, 8, "uniform", axis))
    out = torch.full((box.size,), -1.0, dtype=torch.float64, device="cuda")
    image, _, _ = engine.lbp2d_batch(dev.reshape(-1), [box.shape], 1, 8, "ror", 2, out=out)       # the flat form
    assert image is out and np.array_equal(out.cpu().numpy().reshape(box.shape), lr.lbp_volume(box, 8, 1, "ror", 2))
    with pytest.raises(ValueError):
        engine.lbp2d_batch([dev], None, 1, 8, "uniform", 0, out=out[:-1])
    with pytest.raises(NotImplementedError):
        engine.lbp2d_batch([dev], None, 1, 8, "var")
    with pytest.raises(ValueError):
        engine.lbp2d_batch([dev], None, 1, 8, "uniform", 3)


def test_beyond_the_kernel_the_boxes_take_the_host_route():
    import torch
    from pyradiomics_amd import engine
    boxes = _boxes("float32", [(3, 4, 5), (1, 1, 1)], 9)
    image, _, sizes = engine.lbp2d_batch([torch.from_numpy(b).cuda() for b in boxes], None, 9, 4)
    assert engine.last_batch_route() == "looped"
    for got, box in zip(_split(image.cpu().numpy(), sizes), boxes):
        assert np.array_equal(got, lr.lbp_volume(box, 4, 9, "uniform", 0))


def test_host_twin_and_the_older_table_calls():
    import torch
    from pyradiomics_amd import cmatrices, engine
    boxes = _boxes("int32", [(4, 5, 6), (2, 2, 9)], 2)
    images, name = cmatrices.calculate_lbp2d_batch(boxes, 1.5, 8, "default", 1)
    assert name == "lbp-2D" and cmatrices.last_batch_route() == "batch"
    for got, box in zip(images, boxes):
        assert got.dtype == np.float64 and np.array_equal(got, lr.lbp_volume(box, 8, 1.5, "default", 1))
    x = torch.ones(8, device="cuda")
    for call in (engine.roi_features_batch_images, engine.roi_features_batch_derived):
        with pytest.raises(NotImplementedError, match="LBP2D"):
            call(x, x, [(2, 2, 2)], imageTypes={"LBP2D": {}})
    with pytest.raises(NotImplementedError, match="LBP2D"):
        engine.roi_features_batch_resampled(x, x, [(2, 2, 2)], resampledPixelSpacing=(1, 1, 1), imageTypes={"LBP2D": {}})

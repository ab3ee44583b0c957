"""GPU: engine.lbp2d (prad_lbp2d_dev, csrc/kernels_lbp2d.h) against tests/lbp_reference.py -- exact equality everywhere: the
codes are whole numbers and the contract fixes every rounding.

All three axes x four dtypes x three methods x the (P, R) list on a (5, 6, 7) volume (odd extents, one tile); the degenerate
shapes (1, 1, 1), (1, 1, 5) and (3, 2, 2) with R = 2.5 (the halo is wider than the plane); per axis the extents T - 1 and T + 1
of the tile in both plane axes with a ragged third axis (several workgroups, partial tiles); the float64 plateau fixture whose
codes change under contraction (tests/test_lbp_reference.py shows that); NaN and infinities; a non-contiguous tensor; `out=`;
a 2-D tensor; the domain's edges; filters.getLBP2DImage and cmatrices.calculate_lbp2d on top."""
import numpy as np
import pytest

import lbp_reference as lr

pytestmark = pytest.mark.gpu

SETTINGS = [(1, 1), (3, 0.5), (8, 1), (9, 1), (8, 1.5), (16, 2), (24, 3)]
DTYPES = ["float32", "float64", "int32", "int16"]


@pytest.fixture(scope="module")
def eng():
    import torch
    from pyradiomics_amd import engine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return engine


def _volume(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    if dtype.startswith("float"):
        v = np.round(rng.normal(40.0, 25.0, shape), 1)
        v[rng.random(shape) < 0.3] = 40.0          # ties with the centre
    else:
        v = rng.integers(-3, 4, shape) * 100
    return v.astype(dtype)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fits(dtype, P, method):
    return not (dtype == "int16" and method != "uniform" and P > 15)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axes_dtypes_methods_settings(eng, axis, dtype):
    vol = _volume((5, 6, 7), dtype, 1 + axis)
    x = _dev(vol)
    for P, R in SETTINGS:
        for method in lr.METHODS:
            if not _fits(dtype, P, method):
                continue
            got = eng.lbp2d(x, R, P, method, axis).cpu().numpy()
            assert got.dtype == vol.dtype
            assert np.array_equal(got, lr.lbp_volume(vol, P, R, method, axis)), (P, R, method)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_degenerate_shapes(eng, axis):
    for shape, settings in [((1, 1, 1), SETTINGS), ((1, 1, 5), SETTINGS), ((3, 2, 2), [(8, 2.5), (5, 2.5)])]:
        vol = _volume(shape, "float32", 4)
        for P, R in settings:
            got = eng.lbp2d(_dev(vol), R, P, "default", axis).cpu().numpy()
            assert np.array_equal(got, lr.lbp_volume(vol, P, R, "default", axis)), (shape, P, R)


@pytest.mark.parametrize("dtype", ["int16", "float64"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_tile_seams(eng, axis, dtype):
    tile = eng.lbp2d_plan((300, 300, 300), axis, 1)["tile"]
    a, b = [d for d in range(3) if d != axis]
    for da, db in [(1, 1), (-1, 1), (1, -1)]:
        shape = [3, 3, 70]                                 # the ragged third axis (x = 70 keeps the 64-lane tile of axis 2)
        shape[a], shape[b] = tile[a] + da, tile[b] + db
        vol = _volume(tuple(shape), dtype, 10 + da + 3 * db)
        assert eng.lbp2d_plan(shape, axis, 1)["tile"] == tile
        if (da, db) == (1, 1):
            assert eng.lbp2d_plan(shape, axis, 1)["groups"] >= 4          # a seam along both plane axes
        for P, R, method in [(8, 1, "uniform"), (8, 1.5, "ror")]:
            got = eng.lbp2d(_dev(vol), R, P, method, axis).cpu().numpy()
            assert np.array_equal(got, lr.lbp_volume(vol, P, R, method, axis)), (shape, P, R)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_plateau_fixture_is_not_contracted(eng, axis):
    plane = lr.plateau_plane()
    vol = np.ascontiguousarray(np.stack([plane, plane[::-1].copy()]).swapaxes(0, axis))
    for P, R in [(8, 1), (8, 1.5), (16, 2)]:
        got = eng.lbp2d(_dev(vol), R, P, "uniform", axis).cpu().numpy()
        assert np.array_equal(got, lr.lbp_volume(vol, P, R, "uniform", axis)), (P, R)


def test_nan_and_infinities(eng):
    vol = _volume((4, 9, 10), "float32", 6)
    vol[0, 1, 1], vol[1, 4, 4], vol[2, 7, 2], vol[3, 0, 9] = np.nan, np.inf, -np.inf, np.nan
    for axis in (0, 1, 2):
        for method in lr.METHODS:
            got = eng.lbp2d(_dev(vol), 1, 8, method, axis).cpu().numpy()
            assert np.array_equal(got, lr.lbp_volume(vol, 8, 1, method, axis)), (axis, method)


def test_non_contiguous_input_out_reuse_and_two_dimensions(eng):
    import torch
    vol = _volume((6, 8, 20), "int32", 8)
    x = _dev(vol)
    view = x.permute(2, 0, 1)[::2]                      # (10, 6, 8), no axis contiguous
    assert not view.is_contiguous()
    want = lr.lbp_volume(view.cpu().numpy(), 8, 1, "uniform", 1)
    assert np.array_equal(eng.lbp2d(view, 1, 8, "uniform", 1).cpu().numpy(), want)
    out = torch.full((6, 8, 20), -7, dtype=torch.int32, device="cuda")
    for axis in (0, 2):
        back = eng.lbp2d(x, 1, 8, "uniform", axis, out=out)
        assert back is out and np.array_equal(out.cpu().numpy(), lr.lbp_volume(vol, 8, 1, "uniform", axis))
    with pytest.raises(ValueError):
        eng.lbp2d(x, 1, 8, "uniform", 0, out=x)
    with pytest.raises(ValueError):
        eng.lbp2d(x, 1, 8, "uniform", 0, out=out.to(torch.float32))
    flat = eng.lbp2d(x[0], 1.5, 8, "default")
    assert flat.dtype == torch.float64 and np.array_equal(flat.cpu().numpy(), lr.lbp_plane(vol[0], 8, 1.5, "default"))


def test_domain_edges(eng):
    import torch
    x = _dev(_volume((3, 20, 20), "int16", 2))
    got = eng.lbp2d(x, 8, 24, "uniform", 0).cpu().numpy()                     # ceil(R) = 8, P = 24: the last native settings
    assert np.array_equal(got, lr.lbp_volume(x.cpu().numpy(), 24, 8, "uniform", 0))
    assert eng.lbp2d_native(torch.int16, 8, 24) and not eng.lbp2d_native(torch.int16, 8.5, 8)
    assert not eng.lbp2d_native(torch.uint8, 1, 8)
    with pytest.raises(NotImplementedError):
        eng.lbp2d(x, 8.5, 8)
    with pytest.raises(NotImplementedError):
        eng.lbp2d(x, 1, 8, "var")
    with pytest.raises(NotImplementedError):
        eng.lbp2d(x.to(torch.uint8), 1, 8)
    with pytest.raises(ValueError):
        eng.lbp2d(x, 1, 16, "default")
    with pytest.raises(ValueError):
        eng.lbp2d(x, 1, 25)
    assert np.array_equal(eng.lbp2d(x, 1, 15, "ror").cpu().numpy(), lr.lbp_volume(x.cpu().numpy(), 15, 1, "ror", 0))


def test_filter_route_and_host_array_call(eng):
    from pyradiomics_amd import cmatrices, filters
    from pyradiomics_amd.image import Image
    vol = _volume((5, 9, 11), "int16", 12)
    for kw in ({}, {"force2D": True, "force2Ddimension": 2, "lbp2DRadius": 1.5, "lbp2DMethod": "ror"},
               {"lbp2DRadius": 9, "lbp2DSamples": 4}):                       # the last one: beyond the kernel, the host route
        (dev, name, _), = list(filters.getLBP2DImage(Image(vol), None, **kw))
        (host, _, _), = list(filters.getLBP2DImage(Image(vol), None, deviceResident=False, **kw))
        assert name == "lbp-2D" and dev.array.dtype == np.int16 and np.array_equal(dev.array, host.array)
        assert dev.on_device == (kw.get("lbp2DRadius", 1) <= 8)
        want = lr.lbp_volume(vol, kw.get("lbp2DSamples", 8), kw.get("lbp2DRadius", 1), kw.get("lbp2DMethod", "uniform"),
                             kw.get("force2Ddimension", 0))
        assert np.array_equal(host.array, want)
    with pytest.raises(NotImplementedError):
        list(filters.getLBP2DImage(Image(vol), None, lbp2DMethod="var"))
    with pytest.raises(ValueError):
        list(filters.getLBP2DImage(Image(vol), None, lbp2DSamples=16, lbp2DMethod="default"))
    got = cmatrices.calculate_lbp2d(vol, 1, 8, "uniform", 1)
    assert got.dtype == np.int16 and np.array_equal(got, lr.lbp_volume(vol, 8, 1, "uniform", 1))
    got = cmatrices.calculate_lbp2d(vol[2].astype(np.uint8), 1, 8)
    assert got.dtype == np.float64 and np.array_equal(got, lr.lbp_plane(vol[2].astype(np.uint8), 8, 1))

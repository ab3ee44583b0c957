"""CPU: the LBP2D contract.  tests/lbp_reference.py's three forms against one another and against filters.lbp2d_host (the route
of deviceResident=False and the oracle's twin), hand values, teeth against contraction, the settings the extractor and
paramcheck accept, and -- where scikit-image is installed -- skimage.feature.local_binary_pattern itself.

Hand values (P = 8, R = 1, uniform).  The offsets are (rp, cp) = (0, 1) (-.70711, .70711) (-1, 0) (-.70711, -.70711) (0, -1)
(.70711, -.70711) (1, 0) (.70711, .70711): samples 0, 2, 4, 6 are the right, upper, left and lower 4-neighbour themselves, the odd
samples interpolate inside the diagonal cell.  A single pixel of value 1 at (2, 2) in zeros:
  centre (2, 2)    every sample reads below 1 (the 4-neighbours 0, the diagonals 0.29289^2 = 0.0858), t - 1 < 0: all signs 0, no
                   change, code 0.
  (2, 1) (left neighbour, centre value 0)   every t >= 0 = centre -- all values are >= 0 -- so all eight signs are 1: code 8.
                   The same for (1, 2), (3, 2), (2, 3) and for every other pixel of the zero background: t - 0 >= 0 always.
So a bright pixel is the only pixel whose code is not 8.  The mirror image, a single pixel of value -1 at (2, 2) in zeros, gives
codes that can be derived sample by sample:
  centre (2, 2)    centre -1, all t >= -1 (0 or -0.0858): code 8.
  (2, 1)           centre 0.  Sample 0 (right neighbour) reads -1: sign 0.  Sample 1 (row 2 - .70711, col 1 + .70711: the cell
                   rows 1..2, cols 1..2, dr = dc = .29289) = (1 - dr) top + dr bottom with top = 0 (row 1) and bottom =
                   (1 - dc) 0 + dc (-1): negative, sign 0.  Sample 7 (row 2 + .70711 -> cell rows 2..3, dr = .70711; col cell
                   1..2, dc = .70711): top = dc (-1) < 0, bottom = 0: negative, sign 0.  Samples 2 .. 6 read zeros: sign 1.
                   Signs (0, 0, 1, 1, 1, 1, 1, 0): two changes over the 7 pairs, five ones: code 5.
  (2, 3)           by the mirror symmetry the signs are 0 at samples 3, 4, 5: (1, 1, 1, 0, 0, 0, 1, 1), two changes, code 5.
  (1, 2)           the lower neighbour is -1: samples 5, 6, 7 are 0: (1, 1, 1, 1, 1, 0, 0, 0): ONE change, code 5.
  (3, 2)           samples 1, 2, 3 are 0: (1, 0, 0, 0, 1, 1, 1, 1): two changes, code 5.
A flat plane of an integer level: every interpolation is exact ((1 - d) v + d v = v for small integers v: the products are
exact and their sum is v), t - centre = 0 >= 0 in the interior: code 8."""
import logging

import numpy as np
import pytest

import lbp_reference as lr

SETTINGS = [(1, 1), (3, 0.5), (8, 1), (9, 1), (8, 1.5), (16, 2), (24, 3)]


def _plane(shape, seed):
    rng = np.random.default_rng(seed)
    return np.round(rng.normal(50.0, 20.0, shape), 1)


CASES = [((1, 1), SETTINGS), ((1, 7), SETTINGS), ((2, 2), [(8, 2.5), (3, 2.5)]), ((9, 11), SETTINGS)]


@pytest.mark.parametrize("method", lr.METHODS)
@pytest.mark.parametrize("shape,settings", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_scalar_loop_vectorised_reference_and_host_route_agree(shape, settings, method):
    from pyradiomics_amd import filters
    plane = _plane(shape, 5 + shape[1])
    for P, R in settings:
        want = lr.lbp_plane_scalar(plane, P, R, method)
        assert np.array_equal(lr.lbp_plane(plane, P, R, method), want), (P, R)
        got = filters.lbp2d_host(plane, R, P, method)
        assert got.dtype == np.float64 and np.array_equal(got, want), (P, R)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_host_route_planes_follow_swapaxes(axis):
    """axis 2: rows = y, cols = z (arr.swapaxes(0, 2)[idx] is [y][z]); output in the input's dtype"""
    from pyradiomics_amd import filters
    rng = np.random.default_rng(3)
    vol = rng.integers(-50, 200, (4, 5, 6)).astype(np.int16)
    want = lr.lbp_volume(vol, 8, 1, "uniform", axis, lr.lbp_plane_scalar)
    got = filters.lbp2d_host(vol, 1, 8, "uniform", axis)
    assert got.dtype == np.int16 and got.shape == vol.shape and np.array_equal(got, want)
    if axis == 2:      # spelled out once, without swapaxes
        x = 3
        plane = np.array([[vol[z, y, x] for z in range(4)] for y in range(5)])
        assert np.array_equal(got[:, :, x].T, lr.lbp_plane_scalar(plane, 8, 1))


def test_hand_values_single_pixel():
    bright = np.zeros((5, 5))
    bright[2, 2] = 1.0
    code = lr.lbp_plane_scalar(bright, 8, 1, "uniform")
    assert code[2, 2] == 0
    code[2, 2] = 8
    assert (code == 8).all()
    dark = np.zeros((5, 5))
    dark[2, 2] = -1.0
    code = lr.lbp_plane_scalar(dark, 8, 1, "uniform")
    assert code[2, 2] == 8
    assert code[2, 1] == 5 and code[2, 3] == 5 and code[1, 2] == 5 and code[3, 2] == 5
    assert np.array_equal(lr.lbp_plane(dark, 8, 1), code)


def test_hand_values_flat_integer_plane():
    flat = np.full((6, 7), 37, dtype=np.int32)
    for fn in (lr.lbp_plane, lr.lbp_plane_scalar):
        assert (fn(flat, 8, 1, "uniform")[1:-1, 1:-1] == 8).all()


@pytest.mark.parametrize("P,R", [(8, 1), (8, 1.5), (16, 2)])
def test_plateau_fixture_has_teeth_against_contraction(P, R):
    plane = lr.plateau_plane()
    assert plane.shape == (45, 60) and plane.dtype == np.float64
    exact = lr.lbp_plane(plane, P, R, "uniform")
    fused = lr.lbp_plane_fused(plane, P, R, "uniform")
    differ = int((exact != fused).sum())
    print("plateaus P=%d R=%s: %d of %d pixels differ under fusion" % (P, R, differ, plane.size))
    assert differ >= 1


def test_integer_and_float32_plateaus_do_not_flip():
    plane = lr.plateau_plane()
    for cast in (np.round(plane), plane.astype(np.float32).astype(np.float64)):
        for P, R in [(8, 1), (8, 1.5), (16, 2)]:
            assert np.array_equal(lr.lbp_plane(cast, P, R), lr.lbp_plane_fused(cast, P, R))


def test_nonfinite_values_behave_as_in_numpy():
    from pyradiomics_amd import filters
    plane = _plane((6, 6), 9)
    plane[1, 1], plane[3, 4], plane[4, 1] = np.nan, np.inf, -np.inf
    for method in lr.METHODS:
        want = lr.lbp_plane_scalar(plane, 8, 1, method)
        assert np.array_equal(lr.lbp_plane(plane, 8, 1, method), want)
        assert np.array_equal(filters.lbp2d_host(plane, 1, 8, method), want)


def test_against_scikit_image():
    feature = pytest.importorskip("skimage.feature")
    plane = _plane((9, 11), 2)
    for P, R in SETTINGS:
        for method in lr.METHODS:
            assert np.array_equal(lr.lbp_plane(plane, P, R, method), feature.local_binary_pattern(plane, P, R, method))


def test_var_and_codes_that_do_not_fit():
    from pyradiomics_amd import filters
    vol = np.zeros((2, 3, 3), dtype=np.int16)
    with pytest.raises(NotImplementedError):
        list(filters.getLBP2DImage(vol, None, lbp2DMethod="var", deviceResident=False))
    for method in ("default", "ror"):
        with pytest.raises(ValueError):
            list(filters.getLBP2DImage(vol, None, lbp2DSamples=16, lbp2DMethod=method, deviceResident=False))
    (im, name, _), = list(filters.getLBP2DImage(vol, None, lbp2DSamples=15, lbp2DMethod="default", deviceResident=False))
    assert name == "lbp-2D" and im.array.dtype == np.int16
    (im, _, _), = list(filters.getLBP2DImage(vol, None, lbp2DSamples=16, deviceResident=False))       # uniform: 17 fits
    assert im.array.dtype == np.int16
    with pytest.raises(ValueError):
        filters.lbp2d_host(np.zeros((3, 3)), 1, 25)


def test_defaults_name_and_warning(caplog):
    from pyradiomics_amd import filters
    vol = np.random.default_rng(1).integers(0, 9, (3, 4, 5)).astype(np.int32)
    with caplog.at_level(logging.WARNING, logger="pyradiomics_amd.filters"):
        (im, name, _), = list(filters.getLBP2DImage(vol, None, deviceResident=False))
    assert name == "lbp-2D" and sum("Local Binary Pattern in 2D" in r.message for r in caplog.records) == 1
    assert np.array_equal(im.array, lr.lbp_volume(vol, 8, 1, "uniform", 0))       # P = 8, R = 1, uniform, axis 0
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="pyradiomics_amd.filters"):
        (im2, _, _), = list(filters.getLBP2DImage(vol, None, force2D=True, force2Ddimension=2, deviceResident=False))
    assert not caplog.records and np.array_equal(im2.array, lr.lbp_volume(vol, 8, 1, "uniform", 2))
    (flat, _, _), = list(filters.getLBP2DImage(vol[0], None, deviceResident=False))
    assert flat.array.dtype == np.float64 and np.array_equal(flat.array, lr.lbp_plane(vol[0], 8, 1))


def test_paramcheck_and_extractor_accept_lbp2d():
    from pyradiomics_amd import featureextractor as fe
    ex = fe.RadiomicsFeatureExtractor({"imageType": {"Original": {}, "LBP2D": {"lbp2DRadius": 1.5, "lbp2DSamples": 8,
                                                                                 "lbp2DMethod": "ror"}},
                                       "setting": {"force2D": True, "binWidth": 1}})
    assert ex.enabledImagetypes["LBP2D"] == {"lbp2DRadius": 1.5, "lbp2DSamples": 8, "lbp2DMethod": "ror"}
    assert "LBP2D" in fe.getImageTypes()
    ex.enableImageTypeByName("LBP2D", customArgs={"lbp2DSamples": 16})
    with pytest.raises(NotImplementedError):
        fe.RadiomicsFeatureExtractor({"imageType": {"LBP3D": {}}})

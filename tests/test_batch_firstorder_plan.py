"""The host-only half of the batched first-order front end: prad_batch_firstorder_max_roi / prad_batch_firstorder_plan (capacity,
dynamic LDS, the per-ROI flag, refused arguments) and firstorder.features_from_stats (the class's expressions, vectorised)
against the recorded first-order values of tests/golden/baseline_features.json.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from helpers import load_baseline_features, prepared_case

RAGGED = [(1, 1, 1), (1, 1, 9), (1, 8, 1), (2, 2, 2), (3, 17, 5), (16, 16, 16), (32, 40, 51)]
CAPACITY = (32768, 16384, 32768, 32768)          # float32, float64, int32, int16
KEY_BYTES = (4, 8, 4, 4)
PRAD_OK, PRAD_E_ARG, PRAD_E_UNSUPPORTED = 1, -1, -4


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()
    return _lib.load()


def _plan(lib, sizes, dtype, B=None):
    sizes = np.ascontiguousarray(np.array(sizes, dtype=np.intc).reshape(-1, 3))
    B = len(sizes) if B is None else B
    lds = C.c_longlong(-7)
    inside = np.full(max(len(sizes), 1), -7, dtype=np.intc)
    rc = lib.prad_batch_firstorder_plan(sizes.ctypes.data_as(C.POINTER(C.c_int)), B, dtype, C.byref(lds),
                                        inside.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, int(lds.value), inside[:len(sizes)]


def test_symbols_are_exported(lib):
    from pyradiomics_amd import _lib
    for name in ("prad_batch_firstorder_max_roi", "prad_batch_firstorder_plan", "prad_batch_firstorder_dev",
                 "prad_batch_digitize_max_edges", "prad_batch_digitize_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert (_lib.PRAD_OK, _lib.PRAD_E_ARG, _lib.PRAD_E_UNSUPPORTED) == (PRAD_OK, PRAD_E_ARG, PRAD_E_UNSUPPORTED)


def test_capacity(lib):
    assert tuple(lib.prad_batch_firstorder_max_roi(d) for d in range(4)) == CAPACITY
    assert lib.prad_batch_firstorder_max_roi(4) == PRAD_E_ARG and lib.prad_batch_firstorder_max_roi(-1) == PRAD_E_ARG
    assert lib.prad_batch_digitize_max_edges() >= 4096
    # edges (8 bytes) and counters (4 bytes) share the LDS of a CU
    assert 12 * lib.prad_batch_digitize_max_edges() + 4 + 64 <= 160 * 1024


@pytest.mark.parametrize("dtype", range(4))
def test_lds_grows_with_the_largest_box_and_stays_inside_a_cu(lib, dtype):
    last = 0
    for side in (1, 2, 3, 5, 8, 16, 20, 25, 26, 32, 33, 64, 300):
        rc, lds, inside = _plan(lib, [(1, 1, 1), (side, side, side), (2, 2, 2)], dtype)
        assert rc == PRAD_OK
        assert last <= lds <= 160 * 1024, (side, lds)
        slots = 1 << (min(max(side ** 3, 8), CAPACITY[dtype]) - 1).bit_length()       # (the 2 x 2 x 2 box is the largest at first)
        assert lds == 64 + slots * KEY_BYTES[dtype], (side, lds)
        last = lds
    assert last == 64 + 128 * 1024
    assert _plan(lib, [(16, 16, 16)] * 5, dtype)[1] == 64 + 4096 * KEY_BYTES[dtype]        # many workgroups per CU


@pytest.mark.parametrize("dtype", range(4))
def test_flag_is_set_exactly_for_boxes_within_the_capacity(lib, dtype):
    cap = CAPACITY[dtype]
    sizes = RAGGED + [(1, 1, cap - 1), (1, 1, cap), (1, 1, cap + 1), (2, cap // 2, 1), (2, cap // 2 + 1, 1), (1290, 1290, 1290)]
    rc, _, inside = _plan(lib, sizes, dtype)
    assert rc == PRAD_OK                                  # 1290^3 < 2^31: legal input, decided by the mask
    want = [int(np.prod(s, dtype=np.int64) <= cap) for s in sizes]
    assert inside.tolist() == want
    assert 0 in want and 1 in want
    from pyradiomics_amd import cmatrices
    covered, lds, flags = cmatrices.batch_firstorder_plan(sizes, dtype)
    assert covered and lds == 64 + 128 * 1024 and flags.tolist() == [bool(w) for w in want]


def test_declined_and_refused(lib):
    rc, lds, inside = _plan(lib, [(2, 2, 2), (1291, 1291, 1291)], 0)            # 1291^3 > 2^31 - 1
    assert rc == PRAD_E_UNSUPPORTED and lds == 64 + 128 * 1024 and inside.tolist() == [1, 0]      # outputs filled all the same
    for dtype in (-1, 4, 17):
        assert _plan(lib, RAGGED, dtype)[0] == PRAD_E_ARG
    for B in (0, -1):
        assert _plan(lib, RAGGED, 0, B=B)[0] == PRAD_E_ARG
    assert _plan(lib, [(2, 0, 2)], 0)[0] == PRAD_E_ARG
    null = C.POINTER(C.c_int)()
    sizes = np.array(RAGGED, dtype=np.intc)
    assert lib.prad_batch_firstorder_plan(sizes.ctypes.data_as(C.POINTER(C.c_int)), len(RAGGED), 0, None, null) == PRAD_E_ARG


# ---- features_from_stats ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname", ["brain1", "brain2_resegmentation", "breast1"])
def test_features_from_stats_reproduce_the_recorded_values(cfgname):
    """tolerance: that of tests/test_firstorder.py::test_golden_firstorder_host_and_device_routes"""
    from oracle import firstorder_oracle
    from pyradiomics_amd import firstorder, imageoperations
    cfg = load_baseline_features()[cfgname]
    image, mask, settings = prepared_case(cfg)
    arr = np.asarray(image.array)
    roi = np.asarray(mask.array) == settings.get("label", 1)
    st = firstorder_oracle.firstorder_stats(arr, roi, settings.get("voxelArrayShift", 0))
    binning = {k: settings[k] for k in ("binWidth", "binCount") if k in settings}
    levels, _ = imageoperations.binImage(arr, roi, **binning)
    counts = np.bincount(levels[roi])
    names = sorted(cfg["features"]["firstorder"])
    got = firstorder.features_from_stats(st, counts, float(np.multiply.reduce(image.GetSpacing())), names)
    assert got.shape == (1, len(names)) and len(names) >= 18
    for k, name in enumerate(names):
        ref = cfg["features"]["firstorder"][name]
        assert abs(got[0, k] - ref) <= 1e-9 * abs(ref) + 1e-12, (name, got[0, k], ref)


def test_features_from_stats_rules_and_shapes():
    from pyradiomics_amd import cmatrices, firstorder
    fields = firstorder.STAT_FIELDS
    names = cmatrices.FIRSTORDER_FEATURES
    empty = dict.fromkeys(fields, 0.0)                                  # Np = 0: RootMeanSquared is 0 by rule
    flat = dict(empty, Np=5.0, Energy=5 * 49.0, Minimum=7.0, P10=7.0, P25=7.0, Median=7.0, P75=7.0, P90=7.0, Maximum=7.0,
                Mean=7.0)                                               # m2 = 0: Skewness and Kurtosis are 0 by rule
    wide = dict(flat, Maximum=9.0, P75=8.0, m2=4.0, m3=-8.0, m4=48.0)
    rows = np.array([[d[f] for f in fields] for d in (empty, flat, wide)])
    counts = [np.zeros(0, dtype=np.int64), np.array([5]), np.array([0, 3, 0, 2])]
    got = firstorder.features_from_stats(rows, counts, np.array([1.0, 2.0, 0.5]))
    assert got.shape == (3, 19)
    col = {n: got[:, k] for k, n in enumerate(names)}
    assert col["RootMeanSquared"][0] == 0 and col["RootMeanSquared"][1] == 7
    assert col["Skewness"][1] == 0 and col["Kurtosis"][1] == 0 and col["Variance"][1] == 0
    assert col["Skewness"][2] == -1 and col["Kurtosis"][2] == 3 and col["StandardDeviation"][2] == 2
    assert col["TotalEnergy"].tolist() == [0.0, 490.0, 122.5]
    assert col["Uniformity"][1] == 1 and col["Entropy"][1] == pytest.approx(0, abs=1e-12)
    assert col["Uniformity"][2] == pytest.approx(0.36 + 0.16) and col["InterquartileRange"][2] == 1 and col["Range"][2] == 2
    # the dict form, one ROI, and a subset of the names
    one = firstorder.features_from_stats(wide, np.array([3, 2]), 0.5, ["Kurtosis", "Range"])
    assert one.shape == (1, 2) and one[0].tolist() == [3.0, 2.0]
    with pytest.raises(ValueError):
        firstorder.features_from_stats(rows, counts[:2])

"""prad_batch_features_plan (host only): the layout of the batched feature formulas on the ragged size list of
tests/test_gpu_batch_rois.py -- records, contiguous rows, the box without angles, families that are left out, the declined
domain.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

RAGGED = [(1, 1, 1), (1, 1, 9), (1, 8, 1), (2, 2, 2), (3, 17, 5), (16, 16, 16), (32, 40, 51)]
WIDTH = (24, 16, 16, 5, 16)          # GLCM (23 + MCC), GLRLM, GLDM, NGTDM, GLSZM
ALL = 31
PRAD_OK, PRAD_E_UNSUPPORTED = 1, -4


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()
    return _lib.load()


def _plan(lib, Ng, families, cols=None, sizes=RAGGED):
    from pyradiomics_amd import cmatrices
    sizes = np.ascontiguousarray(np.array(sizes, dtype=np.intc).reshape(-1, 3))
    B = len(sizes)
    _, _, Na = cmatrices.batch_plan(RAGGED, 16, distances=(1,))          # (the angle counts depend on the sizes alone)
    cols = np.ascontiguousarray(np.asarray(cols if cols is not None else np.arange(1, B + 1), dtype=np.intc))
    lay = np.full((2, 5, B + 1), -7, dtype=np.int64)
    nrec = np.full(3, -7, dtype=np.int64)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    rc = lib.prad_batch_features_plan(sizes.ctypes.data_as(ip), B, Ng, families, Na.ctypes.data_as(ip), cols.ctypes.data_as(ip),
                                      lay.ctypes.data_as(lp), nrec.ctypes.data_as(lp))
    return rc, lay, nrec, Na, cols


def test_constants(lib):
    from pyradiomics_amd import _lib
    assert (_lib.PRAD_OK, _lib.PRAD_E_UNSUPPORTED) == (PRAD_OK, PRAD_E_UNSUPPORTED)


def test_records_and_rows(lib):
    rc, lay, nrec, Na, cols = _plan(lib, 16, ALL)
    B = len(RAGGED)
    assert rc == PRAD_OK
    assert nrec[0] == int(Na.sum()) + 3 * B
    assert nrec[1] == int(Na[0].sum())
    # scratch: Ni + Nj doubles per zone-like record
    want = sum(int(Na[1, b]) * (16 + max(RAGGED[b])) + (16 + 4 * int(Na[0, b]) + 1) + (16 + int(cols[b])) for b in range(B))
    assert nrec[2] == want
    rows = [Na[0], Na[1], np.ones(B, int), np.ones(B, int), np.ones(B, int)]
    e = r = 0
    for f in range(5):                   # contiguous, non-overlapping, family after family
        for b in range(B):
            assert (lay[0, f, b], lay[1, f, b]) == (e, r), (f, b)
            e += int(rows[f][b]) * WIDTH[f]
            r += int(rows[f][b])
        assert (lay[0, f, B], lay[1, f, B]) == (e, r)
    assert r == int(Na.sum()) + 3 * B


def test_box_without_angles_has_no_pair_rows(lib):
    rc, lay, nrec, Na, _ = _plan(lib, 16, ALL)
    assert RAGGED[0] == (1, 1, 1) and Na[0, 0] == 0 and Na[1, 0] == 0
    for f in (0, 1):
        assert lay[0, f, 1] == lay[0, f, 0] and lay[1, f, 1] == lay[1, f, 0]
    for f in (2, 3, 4):
        assert lay[1, f, 1] == lay[1, f, 0] + 1 and lay[0, f, 1] == lay[0, f, 0] + WIDTH[f]


@pytest.mark.parametrize("families", [1, 2, 4, 8, 16, 5, 26])
def test_family_left_out_takes_no_space(lib, families):
    rc, lay, nrec, Na, _ = _plan(lib, 16, families)
    B = len(RAGGED)
    assert rc == PRAD_OK
    rows = [int(Na[0].sum()), int(Na[1].sum()), B, B, B]
    total = 0
    for f in range(5):
        on = (families >> f) & 1
        assert lay[1, f, B] - lay[1, f, 0] == (rows[f] if on else 0)
        assert lay[0, f, B] - lay[0, f, 0] == (rows[f] * WIDTH[f] if on else 0)
        total += rows[f] if on else 0
    assert nrec[0] == total and nrec[1] == (rows[0] if families & 1 else 0)


def test_glszm_outside_the_buffer_keeps_its_row(lib):
    cols = [1, 2, 3, 4, 5, 6, 0]          # the last ROI's GLSZM came from the single call
    rc, lay, nrec, Na, _ = _plan(lib, 16, ALL, cols)
    B = len(RAGGED)
    assert rc == PRAD_OK and nrec[0] == int(Na.sum()) + 3 * B - 1
    assert lay[1, 4, B] - lay[1, 4, 0] == B


def test_above_64_levels_declines_with_outputs_filled(lib):
    from pyradiomics_amd import _lib
    rc, lay, nrec, Na, _ = _plan(lib, 65, ALL)
    assert rc == PRAD_E_UNSUPPORTED and "65" in _lib.last_error()
    ok, lay64, nrec64, _, _ = _plan(lib, 64, ALL)
    assert ok == PRAD_OK
    assert np.array_equal(lay, lay64) and (lay >= 0).all()
    assert nrec[0] == nrec64[0] and nrec[1] == nrec64[1] and nrec[2] > nrec64[2]


def test_bad_arguments(lib):
    from pyradiomics_amd import _lib
    assert _plan(lib, 0, ALL)[0] == _lib.PRAD_E_ARG
    assert _plan(lib, 16, 0)[0] == _lib.PRAD_E_ARG
    assert _plan(lib, 16, 32)[0] == _lib.PRAD_E_ARG
    assert _plan(lib, 16, ALL, sizes=[(1, 0, 1)] * 7)[0] == _lib.PRAD_E_ARG

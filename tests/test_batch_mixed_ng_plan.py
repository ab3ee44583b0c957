"""Host half of the per-ROI grey-level count of the batched small-ROI route (prad_batch_plan_ng, prad_batch_features_plan_ng,
prad_batch_merge_plan_ng): the ragged size list of tests/test_batch_plan.py with a count per ROI against numpy sums of the
single calls' shapes, a constant vector against the scalar plans byte for byte, and the domain rules of a vector.  No compute
calls here (no GPU in this tier)."""
import ctypes as C

import numpy as np
import pytest

RAGGED = [(1, 1, 1), (1, 1, 9), (1, 8, 1), (2, 2, 2), (3, 17, 5), (16, 16, 16), (32, 40, 51)]
NG = [64, 1, 2, 7, 33, 63, 5]          # the cap, the smallest, odd counts, one next to the cap
B = len(RAGGED)
ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


def _i(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.intc))


def _angle_counts(oracle, distances):
    """unidirectional angle counts as the single calls obtain them (0 where no offset fits the box and they refuse)"""
    out = []
    for s in RAGGED:
        try:
            out.append(len(oracle.generate_angles(s, list(distances), 0, False, 0)))
        except RuntimeError:
            out.append(0)
    return out


def _numpy_plan(ng, families, na, na1):
    """offsets [4, B + 1] from the single calls' shapes with every ROI's own count: GLCM [Ng, Ng, Na], GLRLM [Ng, max(size), Na1],
    GLDM [Ng, 2 * (2 Na) + 1], NGTDM [Ng, 3]"""
    per = np.array([[g * g * a for g, a in zip(ng, na)],
                    [g * max(s) * a for g, s, a in zip(ng, RAGGED, na1)],
                    [g * (2 * (2 * a) + 1) for g, a in zip(ng, na)],
                    [g * 3 for g in ng]], dtype=np.int64)
    per *= np.array([[(families >> f) & 1] for f in range(4)], dtype=np.int64)
    return np.concatenate([np.zeros((4, 1), np.int64), np.cumsum(per, 1)], 1)


def _plan_ng(lib, ng, families, distances=(1,), f2d=-1, count=B):
    sizes, dist, ng = _i(RAGGED), _i(distances), _i(ng)
    off = np.full((4, B + 1), -7, dtype=np.int64)
    na = np.full((2, B), -7, dtype=np.intc)
    rc = lib.prad_batch_plan_ng(sizes.ctypes.data_as(ip), count, ng.ctypes.data_as(ip), families, dist.ctypes.data_as(ip), len(dist),
                                f2d, off.ctypes.data_as(lp), na.ctypes.data_as(ip))
    return rc, off, na


def _plan_scalar(lib, ng, families, distances=(1,), f2d=-1):
    sizes, dist = _i(RAGGED), _i(distances)
    off = np.full((4, B + 1), -7, dtype=np.int64)
    na = np.full((2, B), -7, dtype=np.intc)
    rc = lib.prad_batch_plan_f2d(sizes.ctypes.data_as(ip), B, ng, families, dist.ctypes.data_as(ip), len(dist), f2d,
                                 off.ctypes.data_as(lp), na.ctypes.data_as(ip))
    return rc, off, na


@pytest.mark.parametrize("distances", [(1,), (1, 2), (2,)], ids=["d1", "d12", "d2"])
@pytest.mark.parametrize("families", [15, 1, 2, 4, 8, 5, 10])
def test_plan_matches_numpy_with_each_rois_own_count(lib, oracle_port, distances, families):
    from pyradiomics_amd import _lib, cmatrices as cm
    rc, off, na = _plan_ng(lib, NG, families, distances)
    assert rc == _lib.PRAD_OK
    uni, uni1 = _angle_counts(oracle_port, distances), _angle_counts(oracle_port, (1,))
    assert na[0].tolist() == uni and na[1].tolist() == uni1
    assert np.array_equal(off, _numpy_plan(NG, families, uni, uni1))
    # the Python layer: the same call, and the shapes the offsets were summed from
    names = tuple(f for i, f in enumerate(cm.BATCH_FAMILIES) if (families >> i) & 1)
    covered, off_py, na_py = cm.batch_plan(RAGGED, NG, names, distances)
    assert covered and np.array_equal(off_py, off) and np.array_equal(na_py, na)
    shapes = cm.batch_shapes(RAGGED, NG, na_py)
    for f, name in enumerate(cm.BATCH_FAMILIES):
        assert [s[0] for s in shapes[name]] == NG
        if (families >> f) & 1:
            assert np.array_equal(np.diff(off[f]), [int(np.prod(s)) for s in shapes[name]])


@pytest.mark.parametrize("f2d", [-1, 0, 2])
@pytest.mark.parametrize("ng", [1, 7, 64])
def test_constant_vector_is_the_scalar_plan(lib, ng, f2d):
    from pyradiomics_amd import _lib
    for families in (15, 5, 10):
        for distances in ((1,), (1, 2)):
            rc_v, off_v, na_v = _plan_ng(lib, [ng] * B, families, distances, f2d)
            rc_s, off_s, na_s = _plan_scalar(lib, ng, families, distances, f2d)
            assert rc_v == rc_s == _lib.PRAD_OK
            assert off_v.tobytes() == off_s.tobytes() and na_v.tobytes() == na_s.tobytes()


def _features_plan(lib, ng, families, vector):
    from pyradiomics_amd import cmatrices
    sizes = _i(RAGGED)
    _, _, Na = cmatrices.batch_plan(RAGGED, 16, distances=(1,))          # (the angle counts depend on the sizes alone)
    cols = _i(np.arange(1, B + 1))
    lay = np.full((2, 5, B + 1), -7, dtype=np.int64)
    nrec = np.full(3, -7, dtype=np.int64)
    if vector:
        g = _i(ng)
        rc = lib.prad_batch_features_plan_ng(sizes.ctypes.data_as(ip), B, g.ctypes.data_as(ip), families, Na.ctypes.data_as(ip),
                                             cols.ctypes.data_as(ip), lay.ctypes.data_as(lp), nrec.ctypes.data_as(lp))
    else:
        rc = lib.prad_batch_features_plan(sizes.ctypes.data_as(ip), B, ng, families, Na.ctypes.data_as(ip), cols.ctypes.data_as(ip),
                                          lay.ctypes.data_as(lp), nrec.ctypes.data_as(lp))
    return rc, lay, nrec, Na, cols


def test_features_plan(lib):
    from pyradiomics_amd import _lib
    rc, lay, nrec, Na, cols = _features_plan(lib, NG, 31, True)
    assert rc == _lib.PRAD_OK
    # rows do not depend on the counts: the layout of any scalar plan
    rc_s, lay_s, nrec_s, _, _ = _features_plan(lib, 16, 31, False)
    assert rc_s == _lib.PRAD_OK and np.array_equal(lay, lay_s) and nrec[0] == nrec_s[0] and nrec[1] == nrec_s[1]
    # scratch: Ni + Nj doubles per zone-like record, Ni the ROI's own count
    want = sum(int(Na[1, b]) * (NG[b] + max(RAGGED[b])) + (NG[b] + 4 * int(Na[0, b]) + 1) + (NG[b] + int(cols[b])) for b in range(B))
    assert nrec[2] == want
    for ng in (1, 7, 64):
        for families in (31, 1, 2, 4, 8, 16, 26):
            v, s = _features_plan(lib, [ng] * B, families, True), _features_plan(lib, ng, families, False)
            assert v[0] == s[0] == _lib.PRAD_OK
            assert v[1].tobytes() == s[1].tobytes() and v[2].tobytes() == s[2].tobytes()


def _merge_plan(lib, ng, families, Na, vector):
    sizes, Na = _i(RAGGED), _i(Na)
    off = np.full((3, B + 1), -7, dtype=np.int64)
    if vector:
        g = _i(ng)
        rc = lib.prad_batch_merge_plan_ng(sizes.ctypes.data_as(ip), B, g.ctypes.data_as(ip), families, Na.ctypes.data_as(ip),
                                          off.ctypes.data_as(lp))
    else:
        rc = lib.prad_batch_merge_plan(sizes.ctypes.data_as(ip), B, ng, families, Na.ctypes.data_as(ip), off.ctypes.data_as(lp))
    return rc, off


@pytest.mark.parametrize("families", [3, 1, 2])
def test_merge_plan(lib, families):
    from pyradiomics_amd import _lib, cmatrices as cm
    _, _, Na = cm.batch_plan(RAGGED, NG, distances=(1, 2))
    rc, off = _merge_plan(lib, NG, families, Na, True)
    assert rc == _lib.PRAD_OK
    per = np.array([[g * g for g in NG], [g * max(s) for g, s in zip(NG, RAGGED)], (Na[0] + Na[1]).tolist()], dtype=np.int64)
    per[0] *= families & 1
    per[1] *= (families >> 1) & 1
    assert np.array_equal(off, np.concatenate([np.zeros((3, 1), np.int64), np.cumsum(per, 1)], 1))
    names = tuple(f for i, f in enumerate(cm.MERGE_FAMILIES) if (families >> i) & 1)
    assert np.array_equal(cm.batch_merge_plan(RAGGED, NG, Na, names), off)
    for ng in (1, 7, 64, 100):          # (the merge has no cap on the counts)
        v, s = _merge_plan(lib, [ng] * B, families, Na, True), _merge_plan(lib, ng, families, Na, False)
        assert v[0] == s[0] == _lib.PRAD_OK and v[1].tobytes() == s[1].tobytes()


def test_a_count_below_one_is_an_argument_error(lib):
    from pyradiomics_amd import _lib, cmatrices as cm
    _, _, Na = cm.batch_plan(RAGGED, 8)
    for k in (0, 3, B - 1):
        ng = list(NG)
        ng[k] = 0
        assert _plan_ng(lib, ng, 15)[0] == _lib.PRAD_E_ARG
        assert "ROI %d" % k in _lib.last_error() and "Ng=0" in _lib.last_error()
        assert _features_plan(lib, ng, 31, True)[0] == _lib.PRAD_E_ARG
        assert _merge_plan(lib, ng, 3, Na, True)[0] == _lib.PRAD_E_ARG
        with pytest.raises(ValueError):
            cm.batch_plan(RAGGED, ng)
    ng = list(NG)
    ng[2] = -5
    assert _plan_ng(lib, ng, 15)[0] == _lib.PRAD_E_ARG
    # a vector is required, and one entry per ROI
    sizes, dist = _i(RAGGED), _i([1])
    off, na = np.zeros((4, B + 1), dtype=np.int64), np.zeros((2, B), dtype=np.intc)
    assert lib.prad_batch_plan_ng(sizes.ctypes.data_as(ip), B, None, 15, dist.ctypes.data_as(ip), 1, -1, off.ctypes.data_as(lp),
                                  na.ctypes.data_as(ip)) == _lib.PRAD_E_ARG
    with pytest.raises(ValueError):
        cm.batch_plan(RAGGED, NG[:-1])
    with pytest.raises(ValueError):
        cm.batch_plan(RAGGED, [8.5] * B)


def test_a_count_above_64_declines_the_batch_with_the_outputs_filled(lib, oracle_port):
    from pyradiomics_amd import _lib, cmatrices as cm
    uni = _angle_counts(oracle_port, (1,))
    for k in (0, 4, B - 1):
        ng = list(NG)
        ng[k] = 65
        rc, off, na = _plan_ng(lib, ng, 15)
        assert rc == _lib.PRAD_E_UNSUPPORTED
        assert "ROI %d" % k in _lib.last_error() and "Ng=65" in _lib.last_error()
        assert na[0].tolist() == uni and np.array_equal(off, _numpy_plan(ng, 15, uni, uni))
        covered, off_py, _ = cm.batch_plan(RAGGED, ng)
        assert not covered and np.array_equal(off_py, off)
        rc, lay, nrec, Na, _ = _features_plan(lib, ng, 31, True)
        ok, lay_ok, nrec_ok, _, _ = _features_plan(lib, NG, 31, True)
        assert rc == _lib.PRAD_E_UNSUPPORTED and ok == _lib.PRAD_OK
        # (the ROI's count enters the scratch once per zone-like record: its GLRLM angles, its GLDM, its GLSZM)
        assert np.array_equal(lay, lay_ok) and nrec[0] == nrec_ok[0] and nrec[2] == nrec_ok[2] + (int(Na[1, k]) + 2) * (65 - NG[k])
    # an empty batch has no count to object to
    assert _plan_ng(lib, NG, 15, count=0)[0] == _lib.PRAD_OK

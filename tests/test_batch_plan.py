"""Host half of the batched small-ROI matrices (prad_batch_plan and the route choice of the Python layer): output offsets,
angle counts and run-length extents of a ragged batch against numpy and the oracle's angle enumeration, the covered domain,
and the looped route when no device is visible.  No compute calls here (no GPU in this tier)."""
import ctypes as C

import numpy as np
import pytest

# PRAD_BATCH_MAX_VOX (csrc/kernels_batch.h): 160 KiB of LDS / 2 workgroups - 16 KiB of tables - 256 bytes
MAX_VOX = 160 * 1024 // 2 - 16384 - 256
# the ragged batch of tests/test_gpu_batch_rois.py: odd voxel counts (the next ROI starts at an element that is no multiple
# of 4 or 16), axes of length 1 and 2 (angles drop out), one box of exactly MAX_VOX voxels with unequal edges
RAGGED = [(1, 1, 1), (1, 1, 9), (1, 8, 1), (2, 2, 2), (3, 17, 5), (16, 16, 16), (32, 40, 51)]


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


def _numpy_plan(sizes, Ng, families, na, na1):
    """offsets [4, B + 1] from the single calls' shapes: GLCM [Ng, Ng, Na], GLRLM [Ng, max(size), Na1], GLDM [Ng, 2 * (2 Na) + 1],
    NGTDM [Ng, 3]"""
    per = np.array([[Ng * Ng * a for a in na],
                    [Ng * max(s) * a for s, a in zip(sizes, na1)],
                    [Ng * (2 * (2 * a) + 1) for a in na],
                    [Ng * 3 for _ in sizes]], dtype=np.int64)
    per *= np.array([[(families >> f) & 1] for f in range(4)], dtype=np.int64)
    return np.concatenate([np.zeros((4, 1), np.int64), np.cumsum(per, 1)], 1)


def _angle_counts(oracle, sizes, distances):
    """unidirectional / bidirectional angle counts as the single calls obtain them (0 where no offset fits the box -- a
    1 x 1 x 1 box, distance 2 in a 2 x 2 x 2 box -- and they refuse)"""
    uni, bi = [], []
    for s in sizes:
        try:
            uni.append(len(oracle.generate_angles(s, distances, 0, False, 0)))
            bi.append(len(oracle.generate_angles(s, distances, 1, False, 0)))
        except RuntimeError:
            uni.append(0)
            bi.append(0)
    return uni, bi


@pytest.mark.parametrize("distances", [(1,), (1, 2), (2,)], ids=["d1", "d12", "d2"])
@pytest.mark.parametrize("families", [15, 1, 2, 4, 8, 5, 10])
def test_plan_matches_numpy(lib, oracle_port, distances, families):
    from pyradiomics_amd import _lib, cmatrices as cm
    assert lib.prad_batch_max_vox() == MAX_VOX == 32 * 40 * 51
    Ng = 7
    names = tuple(f for i, f in enumerate(cm.BATCH_FAMILIES) if (families >> i) & 1)
    covered, offsets, Na = cm.batch_plan(RAGGED, Ng, names, distances)
    assert covered
    uni, bi = _angle_counts(oracle_port, RAGGED, list(distances))
    uni1, _ = _angle_counts(oracle_port, RAGGED, [1])
    assert Na[0].tolist() == uni and Na[1].tolist() == uni1
    assert [2 * a for a in uni] == bi          # the GLDM row width 2 * Nb + 1 of the single call, Nb bidirectional
    assert np.array_equal(offsets, _numpy_plan(RAGGED, Ng, families, uni, uni1))
    shapes = cm.batch_shapes(RAGGED, Ng, Na)
    assert [s[1] for s in shapes["glrlm"]] == [max(s) for s in RAGGED]          # Nr
    assert [s[1] for s in shapes["gldm"]] == [2 * b + 1 for b in bi]
    # axes of length 1 drop angles; distance 2 needs an edge of 3
    if distances == (1,):
        assert uni == [0, 1, 1, 13, 13, 13, 13]
    if distances == (2,):
        assert uni[:4] == [0, 1, 1, 0]


def test_plan_raw_call_and_errors(lib):
    from pyradiomics_amd import _lib
    sizes = np.array(RAGGED, dtype=np.intc)
    B = len(RAGGED)
    dist = np.array([1], dtype=np.intc)
    off = np.full((4, B + 1), -1, dtype=np.int64)
    na = np.full((2, B), -1, dtype=np.intc)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)

    def plan(sz, b, Ng, fam, d=dist):
        return lib.prad_batch_plan(sz.ctypes.data_as(ip), b, Ng, fam, d.ctypes.data_as(ip), len(d), off.ctypes.data_as(lp),
                                   na.ctypes.data_as(ip))
    assert plan(sizes, B, 64, 15) == _lib.PRAD_OK
    assert (off >= 0).all() and (np.diff(off, axis=1) >= 0).all() and (na >= 0).all()
    assert plan(sizes, B, 0, 15) == _lib.PRAD_E_ARG
    assert plan(sizes, B, 8, 0) == _lib.PRAD_E_ARG and plan(sizes, B, 8, 16) == _lib.PRAD_E_ARG
    assert plan(sizes, B, 8, 15, np.array([0], dtype=np.intc)) == _lib.PRAD_E_ARG
    bad = sizes.copy()
    bad[2, 1] = 0
    assert plan(bad, B, 8, 15) == _lib.PRAD_E_ARG
    # outside the covered domain: declined, the layout is filled in all the same (the looped route uses it)
    off[:] = -1
    assert plan(sizes, B, 65, 15) == _lib.PRAD_E_UNSUPPORTED
    assert "Ng=65" in _lib.last_error() and (off >= 0).all()
    over = np.array([(2, 2, 2), (32, 40, 51), (1, 1, MAX_VOX + 1)], dtype=np.intc)
    assert plan(over, 2, 64, 15) == _lib.PRAD_OK
    assert plan(over, 3, 64, 15) == _lib.PRAD_E_UNSUPPORTED and "ROI 2" in _lib.last_error()
    # 127 unidirectional angles at most (u32 NGTDM sums): distances 1..3 give 171
    assert plan(sizes[4:6], 2, 8, 15, np.array([1, 2, 3], dtype=np.intc)) == _lib.PRAD_E_UNSUPPORTED


def test_python_layer_chooses_its_route_on_the_host(lib):
    from pyradiomics_amd import cmatrices as cm
    assert cm.batch_plan(RAGGED, 64)[0] and not cm.batch_plan(RAGGED, 65)[0]
    assert not cm.batch_plan(RAGGED[:-1] + [(32, 40, 52)], 8)[0]
    assert cm.batch_family_bits(("ngtdm", "glcm")) == 9
    with pytest.raises(ValueError):
        cm.batch_family_bits(("glszm",))
    with pytest.raises(ValueError):
        cm.calculate_matrices_batch([np.ones((2, 2), int)], [np.ones((2, 2), bool)], 2)


def test_looped_route_without_device(lib):
    """no device: the batch goes to the single calls, which fail loudly (never compute on the host)"""
    if lib.prad_device_count() > 0:
        pytest.skip("a GPU is visible")
    from pyradiomics_amd import cmatrices as cm
    cm._set_batch_route("none")
    imgs = [np.ones(s, int) for s in RAGGED[1:4]]
    with pytest.raises(RuntimeError, match="no HIP device"):
        cm.calculate_matrices_batch(imgs, [i > 0 for i in imgs], 2)
    assert cm.last_batch_route() == "looped"
    # a batch of 1 x 1 x 1 boxes needs no single call at all: the looped route answers it on its own
    mats, status = cm.calculate_matrices_batch([np.full((1, 1, 1), 2)] * 2, [np.ones((1, 1, 1), bool), np.zeros((1, 1, 1), bool)], 3)
    assert status == [1, 1] and cm.last_batch_route() == "looped"
    assert mats["glcm"][0].shape == (3, 3, 0) and mats["glrlm"][0].shape == (3, 1, 0)
    assert mats["gldm"][0].tolist() == [[0], [1], [0]] and not mats["gldm"][1].any()
    assert mats["ngtdm"][0].tolist() == [[0, 0, 1], [1, 0, 2], [0, 0, 3]]

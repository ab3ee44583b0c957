"""Pins tests/glszm_reference.py (scipy.ndimage.label per grey level), the yardstick of tests/test_gpu_glszm_topology.py,
without a GPU: to the recorded GLSZM matrices of the three golden cases, to the C checker on a few hundred small random volumes
(2-D, 3-D, 4-D, every force2D dimension, matrix AND zone order), and to the closed-form zone census of every constructed volume
of the GPU module -- each generator states how many zones of which size and level it holds, derived from its parameters.
test_the_pin_is_sharp shows that a reference with one neighbour missing does not pass these pins."""
import ctypes as C

import numpy as np
import pytest

import glszm_reference as gr
import test_gpu_glszm_topology as topo
from helpers import feature_class, load_case


class _ScipyBackend:
    """the CPU checker with its GLSZM replaced by the scipy restatement"""

    def __init__(self, port):
        self._port = port

    def __getattr__(self, name):
        return getattr(self._port, name)

    def calculate_glszm(self, image, mask, Ng, Ns, force2D, force2Ddimension, kernelRadius=0, voxels=None):
        assert voxels is None
        return gr.matrix(gr.zones(image, mask, force2D, force2Ddimension), Ng)


@pytest.mark.parametrize("case", ["brain1", "brain2", "breast1"])
def test_golden_matrices(oracle_port, case):
    from pyradiomics_amd import backend
    image, mask, golden = load_case(case)
    old = backend._cmatrices
    backend.set(_ScipyBackend(oracle_port))
    try:
        fc = feature_class("glszm")(image, mask, binWidth=25, distances=[1], gldm_a=0, force2D=False, label=1)
        fc._initCalculation()
        P = fc.P_glszm
    finally:
        backend.set(old)
    assert P.shape[0] == 1 and P[0].shape == golden["glszm"].shape and np.array_equal(P[0], golden["glszm"])


def _checker_zone_list(port, img, mask, force2D, f2d):
    """(level, size) pairs in the order the checker's raster scan finds the zones, closed by -1"""
    img = np.ascontiguousarray(img, dtype=np.intc)
    m2 = np.array(mask, dtype=np.bool_, order="C", copy=True)
    size = np.array(img.shape, dtype=np.intc)
    strides = np.array([s // 4 for s in img.strides], dtype=np.intc)
    bb = np.concatenate([np.zeros(img.ndim, np.intc), size - 1]).astype(np.intc)
    ang = port.generate_angles(size, [1], 1, 1 if force2D else 0, f2d)
    cap = max(int(m2.sum()), 1)
    temp = np.empty(2 * cap + 1, dtype=np.intc)
    ip = C.POINTER(C.c_int)
    r = port.L.calculate_glszm(img.ctypes.data_as(ip), m2.ctypes.data_as(C.c_char_p), size.ctypes.data_as(ip),
                               bb.ctypes.data_as(ip), strides.ctypes.data_as(ip), ang.ctypes.data_as(ip), len(ang), img.ndim,
                               temp.ctypes.data_as(ip), 0, cap, 1)
    assert r >= 0
    return temp[:int(np.flatnonzero(temp == -1)[0]) + 1]


def _random_cases(n):
    rng = np.random.default_rng(2024)
    for i in range(n):
        nd = (3, 3, 3, 2, 4)[i % 5]
        shape = tuple(int(v) for v in rng.integers(1, (12, 12, 8, 5)[nd - 1 if nd < 4 else 3] + 1, size=nd))
        Ng = int(rng.integers(1, 6))
        img = rng.integers(1, Ng + 1, size=shape).astype(np.int32)
        mask = rng.random(shape) < rng.choice([0.5, 0.9, 1.0])
        if not mask.any():
            mask.reshape(-1)[0] = True
        modes = [(False, 0)] + ([(True, d) for d in range(3)] if nd == 3 else [])
        yield img, mask, Ng, modes


def _agrees(port, img, mask, Ng, force2D, f2d, drop=()):
    z = gr.zones(img, mask, force2D, f2d, drop)
    try:
        want = port.calculate_glszm(img, mask, Ng, int(mask.sum()), force2D, f2d)
    except RuntimeError:                   # no angle left for this shape / force2D combination
        return None
    return bool(np.array_equal(gr.matrix(z, Ng), want) and
                np.array_equal(gr.zone_list(z), _checker_zone_list(port, img, mask, force2D, f2d)))


def test_equals_the_checker_on_random_volumes(oracle_port):
    n = 0
    for img, mask, Ng, modes in _random_cases(300):
        for force2D, f2d in modes:
            ok = _agrees(oracle_port, img, mask, Ng, force2D, f2d)
            assert ok is not False, (img.shape, Ng, force2D, f2d)
            n += ok is True
    assert n >= 400


def test_equals_the_checker_on_a_ragged_noise_volume(oracle_port):
    """17 x 19 x 131 noise under a 0.9 mask, both neighbourhoods"""
    rng = np.random.default_rng(5)
    img = rng.integers(1, 4, size=(17, 19, 131)).astype(np.int32)
    mask = rng.random(img.shape) < 0.9
    for force2D in (False, True):
        assert _agrees(oracle_port, img, mask, 3, force2D, 0)


def test_the_pin_is_sharp(oracle_port):
    """without the (-1, -1, -1) corner (and its mirror image) the restatement no longer agrees with the checker on the random
    volumes, nor with the closed forms of the volumes that hang on that diagonal; likewise without an in-plane diagonal"""
    bad = sum(_agrees(oracle_port, img, mask, Ng, False, 0, drop=[(-1, -1, -1)]) is False
              for img, mask, Ng, modes in _random_cases(300) if img.ndim == 3)
    assert bad >= 10, bad
    vol = topo.staircases((17, 17, 130), (1, 1, 1), topo.CORNER)
    assert gr.census(gr.zones(vol.img, vol.mask)) == vol.cen
    assert gr.census(gr.zones(vol.img, vol.mask, drop=[(-1, -1, -1)])) != vol.cen
    vol = topo.checkerboard((9, 17, 65), 3)
    assert gr.census(gr.zones(vol.img, vol.mask, True, 0, drop=[(0, -1, 1)])) != vol.cen2
    bad = sum(_agrees(oracle_port, img, mask, Ng, True, 0, drop=[(0, -1, 1)]) is False
              for img, mask, Ng, modes in _random_cases(300) if img.ndim == 3)
    assert bad >= 10, bad


@pytest.mark.parametrize("case", topo.CATALOGUE_IDS)
def test_closed_form_census(oracle_port, case):
    """the census every generator states == scipy == the C checker, under the full and the in-plane neighbourhood; the
    zones tile the ROI"""
    vol = topo.BY_ID[case]()
    Ns = int(vol.mask.sum())
    for force2D, closed in ((False, vol.cen), (True, vol.cen2)):
        assert closed is not None
        z = vol.zones(force2D, 0)
        assert gr.census(z) == closed, (vol.name, force2D)
        assert sum(s * c for (_, s), c in closed.items()) == Ns
        P, sizes = gr.census_matrix(closed, vol.Ng)
        Pr, sr = gr.compact(z, vol.Ng)
        assert np.array_equal(P, Pr) and np.array_equal(sizes, sr)
        if vol.img.size <= 1 << 18 or case == "corners-131":
            want = oracle_port.calculate_glszm(vol.img, vol.mask, vol.Ng, Ns, force2D, 0)
            assert np.array_equal(gr.matrix(z, vol.Ng), want), (vol.name, force2D)
            assert np.array_equal(gr.zone_list(z), _checker_zone_list(oracle_port, vol.img, vol.mask, force2D, 0))


def test_closed_forms_of_the_other_ranks_and_sizes(oracle_port):
    """the generators at the ranks and sizes the GPU module also uses: 4-D checkerboards, a 64 x 64 x 256 serpentine, the
    random-block volumes (no closed form: scipy against the checker)"""
    for shape in ((3, 5, 9, 66), (2, 8, 8, 64)):
        for m in (2, 3):
            vol = topo.checkerboard(shape, m)
            assert gr.census(vol.zones()) == vol.cen
    vol = topo.serpentine((64, 64, 256))
    z = vol.zones()
    assert gr.census(z) == vol.cen and len(z) == 2
    assert np.array_equal(gr.zone_list(z), _checker_zone_list(oracle_port, vol.img, vol.mask, False, 0))
    vol = topo.random_blocks((72, 72, 264), (4, 0, 0), 3, 2)
    assert vol.nblocks == 2048
    for force2D in (False, True):
        assert _agrees(oracle_port, vol.img, vol.mask, vol.Ng, force2D, 0)
    for axes in ((0, 2, 1), (2, 1, 0), (1, 2, 0)):
        for base in (topo.serpentine((17, 9, 130)), topo.combs((17, 9, 130)), topo.helix((17, 9, 130))):
            vol = base.transposed(axes)
            assert gr.census(vol.zones()) == vol.cen

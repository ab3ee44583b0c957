"""The close of the lines that leave a window-filling row at the window's edge (csrc/kernels_sweepfw.h FwWave::capture_reg /
close_captured, rotate_reg; csrc/kernels_sweepfw2.h Fw2Wave::rotate_reg): on the plain path of the fused-table walk the U = 8
closes of a group are one ds_add of 8 lanes behind the group's last step; the two-table walk closes in every step.

Every row fills its window exactly -- 256 voxels with K = 4 columns per lane, 512 with 8, 1024 with 16 -- and every march holds
several plain groups behind its piece starts.  At 64 levels the first two shapes take the two-table walk and the third the
wrapped-lines kernels; they are compared all the same.

Images: iid levels (a wrong address or a stale buffer lane changes a GLRLM count), 3 x 3 x 3 blocks of one level (runs of
length 1 - 3 meet the edge: the two-table walk leaves out the close of a run of length 1), one constant level (runs as long as
the lines: the checked path next to plain groups).  Masks: full; the columns x = 0 and x = NX - 1 outside the ROI (the leaving
line has previous level 0, its close must land in the scratch words in front of the table); only those two columns inside.

Routes: the synchronous call, and a deferred run of the four volumes of a (shape, levels, mask) with twin pipelines forced on and
forced off.  Every matrix is bit for bit equal to the CPU checker: the counts are integers, there is no tolerance."""
import numpy as np
import pytest

from test_gpu_fin_ride import _assert_equal
from test_gpu_twin_pipeline import _run, _twin

pytestmark = pytest.mark.gpu

SHAPES = [(24, 40, 256), (40, 24, 512), (24, 24, 1024)]
IMAGES = ["iid", "blocks", "constant", "iid2"]
MASKS = ["full", "edges_out", "edges_only"]


@pytest.fixture(scope="module")
def engine():
    from pyradiomics_amd import engine
    return engine


def _variant(shape, Ng):
    """what the planner makes of the shape (prad_sweep_plan.h plan_lines_shape / plan_tables)"""
    if Ng <= 44:
        return "fw"
    return "fw2" if shape[2] <= 512 else "lines"


def _image(kind, shape, Ng):
    rng = np.random.default_rng({"iid": 4100, "iid2": 4101, "blocks": 4102, "constant": 4103}[kind] + shape[2] + Ng)
    if kind == "constant":
        return np.full(shape, 1 + (shape[2] // 256 + 5 * (Ng // 32)) % Ng, np.int32)
    if kind == "blocks":
        small = rng.integers(1, Ng + 1, size=tuple((n + 2) // 3 for n in shape)).astype(np.int32)
        big = np.repeat(np.repeat(np.repeat(small, 3, 0), 3, 1), 3, 2)
        return np.ascontiguousarray(big[:shape[0], :shape[1], :shape[2]])
    return rng.integers(1, Ng + 1, size=shape).astype(np.int32)


def _roi(kind, shape):
    m = np.ones(shape, bool)
    if kind == "edges_out":
        m[:, :, 0] = m[:, :, -1] = False
    elif kind == "edges_only":
        m[:, :, 1:-1] = False
    return m


_want = {}


def _vols(checker, shape, Ng, mkind):
    """the four volumes of (shape, Ng, mask): (device image, device mask, Ng, Nr, checker GLCM, checker GLRLM) each, computed once"""
    import torch
    key = (shape, Ng, mkind)
    if key not in _want:
        mask = _roi(mkind, shape)
        Nr = int(max(shape))
        out = []
        for kind in IMAGES:
            img = _image(kind, shape, Ng)
            g, _ = checker.calculate_glcm(img, mask, [1], Ng, False, 0)
            r, _ = checker.calculate_glrlm(img, mask, Ng, Nr, False, 0)
            out.append((torch.from_numpy(img).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda(), Ng, Nr,
                        torch.from_numpy(np.ascontiguousarray(g[0])).cuda(), torch.from_numpy(np.ascontiguousarray(r[0])).cuda()))
        _want[key] = out
    return _want[key]


@pytest.mark.parametrize("mkind", MASKS)
@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_synchronous_call(engine, checker, shape, Ng, mkind):
    vols = _vols(checker, shape, Ng, mkind)
    got = []
    for v in vols:
        g, r, _ = engine.glcm_glrlm(v[0], v[1], v[2], v[3])
        assert engine.last_path() == "sweep"
        assert engine.last_variant() == _variant(shape, Ng)
        got.append((g.clone(), r.clone()))
    _assert_equal(got, vols)


@pytest.mark.parametrize("twin", ["1", "0"])
@pytest.mark.parametrize("mkind", MASKS)
@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_deferred_run(engine, checker, monkeypatch, shape, Ng, mkind, twin):
    vols = _vols(checker, shape, Ng, mkind)
    _twin(monkeypatch, twin)
    got, _, raised, _ = _run(engine, vols)
    assert engine.last_variant() == _variant(shape, Ng)
    _twin(monkeypatch, None)
    assert not raised
    _assert_equal(got, vols)

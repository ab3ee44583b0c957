"""The finalize of a GLCM + GLRLM volume as ONE launch (csrc/kernels_sweep.h: finalize_volume_kernel): a workgroup per
angle owns everything that depends on multi[a] -- the GLCM diagonal, the restored runs of length 1 of a two-table (SKIP1)
volume, the "some line of the angle holds two masked voxels" verdict (cmatrices.c:524-534) and the length-1 column of the
GLRLM -- and the other workgroups convert the rest element by element.

Every case is compared bit for bit with the CPU checker AND with the same call under PRAD_FINALIZE_ONE=0 (the three
launches), and must have taken the sweep route.  The masks of the `multi` rule leave some angles without any line of two
voxels although the box is large: they reach the exact test inside the angle workgroup."""
import numpy as np
import pytest

from test_gpu_fw import _levels, _mask

pytestmark = pytest.mark.gpu

AXIS_X = (0, 0, 1)


@pytest.fixture(scope="module")
def cm():
    from pyradiomics_amd import cmatrices
    return cmatrices


def _run(cm, img, mask, Ng, Nr, variant=None):
    from pyradiomics_amd import _lib
    g, r, ang = cm.calculate_glcm_glrlm(img, mask, Ng, Nr, False, 0)
    assert _lib.last_path() == "sweep"
    if variant is not None:
        assert _lib.last_variant() == variant
    return g, r, ang


def _three_ways(cm, checker, monkeypatch, img, mask, Ng, variant=None):
    """-> (GLRLM of the one-launch finalize, angles); asserts checker == one launch == three launches, bit for bit"""
    Nr = int(max(img.shape))
    eg, eang = checker.calculate_glcm(img, mask, [1], Ng, False, 0)
    er, _ = checker.calculate_glrlm(img, mask, Ng, Nr, False, 0)
    monkeypatch.delenv("PRAD_FINALIZE_ONE", raising=False)
    g1, r1, ang = _run(cm, img, mask, Ng, Nr, variant)
    monkeypatch.setenv("PRAD_FINALIZE_ONE", "0")
    g0, r0, _ = _run(cm, img, mask, Ng, Nr, variant)
    monkeypatch.delenv("PRAD_FINALIZE_ONE")
    assert np.array_equal(ang, eang)
    assert np.array_equal(g1, eg), "GLCM differs from the checker at (i, j, angle) %s" % (np.argwhere(g1 != eg)[:3],)
    assert np.array_equal(r1, er), "GLRLM differs from the checker at (i, len-1, angle) %s" % (np.argwhere(r1 != er)[:3],)
    assert np.array_equal(g1, g0), "GLCM differs from the three launches at %s" % (np.argwhere(g1 != g0)[:3],)
    assert np.array_equal(r1, r0), "GLRLM differs from the three launches at %s" % (np.argwhere(r1 != r0)[:3],)
    assert r1.shape == er.shape == (1, Ng, Nr, len(eang))
    assert np.array_equal(r1[0][:, 0, :], er[0][:, 0, :])     # the length-1 column of every angle
    return er[0], [tuple(int(c) for c in a) for a in ang]


# ---- fused table (32 levels) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind,mkind", [
    ((2, 2, 65), "uniform", "full"),       # the smallest fixed-window volume
    ((9, 40, 130), "smooth", "random"),
    ((20, 24, 512), "smooth", "ball"),
])
def test_fused_table(cm, checker, monkeypatch, shape, kind, mkind):
    _three_ways(cm, checker, monkeypatch, _levels(11, shape, 32, kind), _mask(3, shape, mkind), 32, "fw")


# ---- two tables: the line angles did not record their runs of length 1 (SKIP1), the angle workgroups restore them ----------
@pytest.mark.parametrize("shape,Ng,kind,mkind,variant", [
    ((9, 40, 130), 64, "uniform", "random", "fw2"),
    ((9, 40, 130), 160, "uniform", "full", "fw2"),
    ((3, 3, 512), 64, "smooth", "full", "fw2"),       # the longest row the two-table walk takes
    ((3, 3, 1024), 64, "smooth", "full", None),       # the longest row: separate tables (no restore), three launches either way
    ((12, 20, 257), 64, "blobs", "ball", "fw2"),
])
def test_two_tables(cm, checker, monkeypatch, shape, Ng, kind, mkind, variant):
    er, ang = _three_ways(cm, checker, monkeypatch, _levels(12, shape, Ng, kind), _mask(4, shape, mkind), Ng, variant)
    assert len(ang) == 13 and er[:, 0, :].any()


# ---- the multi rule ---------------------------------------------------------------------------------------------------------
SHAPE = (9, 40, 130)


def _grid(shape=SHAPE):
    return np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")


def _points(*pts):
    m = np.zeros(SHAPE, bool)
    for p in pts:
        m[p] = True
    return m


def _one_plane():
    m = np.zeros(SHAPE, bool)
    m[4] = True
    return m


def _checkerboard():
    z, y, x = _grid()
    return (z + y + x) % 2 == 0


def _sheet():
    z, y, x = _grid()
    return x + y == 60


# name -> (mask, angles whose length-1 column must survive; None: all; the others must lose it)
MULTI = {
    # z angles open (no run, no pair), the box is not thin: the exact test says 0 for them
    "one-plane": (_one_plane, lambda a: a[0] == 0),
    # no adjacent pair along the axes nor along the diagonals with an odd step sum, but their lines hold many voxels:
    # the cheap test fails, the exact test must say 1
    "checkerboard": (_checkerboard, None),
    # every line of an angle with dy + dx != 0 meets the sheet once
    "sheet": (_sheet, lambda a: a[1] + a[2] == 0),
    "single-voxel": (lambda: _points((4, 20, 60)), lambda a: False),
    # (+3, +5, +11): no angle's line joins them
    "two-voxels-apart": (lambda: _points((2, 10, 30), (5, 15, 41)), lambda a: False),
    # far apart on one x row: the x angle keeps its column, the others lose it
    "two-on-a-row": (lambda: _points((4, 20, 7), (4, 20, 101)), lambda a: a == AXIS_X),
}


@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("name", list(MULTI))
def test_multi_rule(cm, checker, monkeypatch, name, Ng):
    mk, keeps = MULTI[name]
    er, ang = _three_ways(cm, checker, monkeypatch, _levels(13, SHAPE, Ng, "uniform"), mk(), Ng, "fw" if Ng == 32 else "fw2")
    for n, a in enumerate(ang):
        want = True if keeps is None else bool(keeps(a))
        assert bool(er[:, 0, n].any()) == want, (name, a)


# ---- further cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ng", [32, 64])
def test_box_one_voxel_thick(cm, checker, monkeypatch, Ng):
    """the reference generates no angle that moves along a dimension of size 1 (cmatrices.c: get_angle_count): four angles,
    four angle workgroups, all with lines of two voxels"""
    shape = (1, 40, 130)
    er, ang = _three_ways(cm, checker, monkeypatch, _levels(14, shape, Ng, "uniform"), _mask(5, shape, "random"), Ng)
    assert len(ang) == 4 and all(a[0] == 0 for a in ang) and er[:, 0, :].any(axis=0).all()
    one = np.zeros(shape, bool)
    one[0, 20, 60] = True      # every angle open, every exact test says 0
    er, _ = _three_ways(cm, checker, monkeypatch, _levels(14, shape, Ng, "uniform"), one, Ng)
    assert not er.any()


@pytest.mark.parametrize("Ng", [32, 64])
def test_level_missing_from_the_roi(cm, checker, monkeypatch, Ng):
    shape = (9, 40, 130)
    img = _levels(15, shape, Ng, "uniform")
    img[img == 5] = 6
    img[img == Ng] = 1
    er, _ = _three_ways(cm, checker, monkeypatch, img, _mask(6, shape, "random"), Ng)
    assert not er[4].any() and not er[Ng - 1].any() and er[5].any()


SPECS = [((12, 20, 257), 32, "uniform", "ball"), ((9, 40, 130), 64, "smooth", "full"), ((12, 20, 257), 32, "smooth", "random"),
         ((9, 40, 130), 64, "uniform", "random"), ((12, 20, 257), 32, "blobs", "full")]


def _deferred(engine, dev):
    """-> (results, deferred_status raised?)"""
    engine.set_deferred_mode(1)
    try:
        got = []
        for i, m, Ng in dev:
            g, r, _ = engine.glcm_glrlm(i, m, Ng, 512, deferred=True)
            assert engine.last_path() == "sweep"
            got.append((g, r))
        engine.deferred_join()
        raised = False
        try:
            engine.deferred_status()
        except RuntimeError:
            raised = True
        engine.deferred_status()    # the verdict is reported once
        return [(g.clone(), r.clone()) for g, r in got], raised
    finally:
        engine.set_deferred_mode(-1)


def test_deferred_run_of_alternating_volumes(monkeypatch):
    """five volumes of alternating shape and level count through the deferred pipeline: equal to the synchronous results,
    with and without the switch; a level above Ng is reported exactly as by the three launches"""
    import torch
    from pyradiomics_amd import engine
    vols = [(_levels(20 + i, s, Ng, k), _mask(30 + i, s, m), Ng) for i, (s, Ng, k, m) in enumerate(SPECS)]
    dev = [(torch.from_numpy(i).cuda(), torch.from_numpy(m.astype(np.uint8)).cuda(), Ng) for i, m, Ng in vols]
    want = []
    for i, m, Ng in dev:
        g, r, _ = engine.glcm_glrlm(i, m, Ng, 512)
        assert engine.last_path() == "sweep"
        want.append((g.clone(), r.clone()))
    got1, raised1 = _deferred(engine, dev)
    monkeypatch.setenv("PRAD_FINALIZE_ONE", "0")
    got0, raised0 = _deferred(engine, dev)
    monkeypatch.delenv("PRAD_FINALIZE_ONE")
    assert not raised1 and not raised0
    for n in range(len(dev)):
        for k in (0, 1):
            assert torch.equal(got1[n][k], want[n][k]), "volume %d differs from its synchronous result" % n
            assert torch.equal(got0[n][k], want[n][k]), "volume %d differs (three launches)" % n
    # a level above Ng in the third volume
    BAD = 2
    bad = vols[BAD][0].copy()
    bad[5, 6, 7] = 33
    dev[BAD] = (torch.from_numpy(bad).cuda(), dev[BAD][1], 32)
    got1, raised1 = _deferred(engine, dev)
    monkeypatch.setenv("PRAD_FINALIZE_ONE", "0")
    got0, raised0 = _deferred(engine, dev)
    assert raised1 and raised0
    for n in range(len(dev)):
        if n != BAD:
            for k in (0, 1):
                assert torch.equal(got1[n][k], want[n][k]), "volume %d behind or before the irregular one differs" % n
                assert torch.equal(got0[n][k], want[n][k])

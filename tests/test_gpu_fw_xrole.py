"""The x angle as the trailing role of the fixed-window launch (csrc/kernels_sweepfw.h: sweep_fw_kernel, fw_rows_role):
fused-table GLCM + GLRLM calls walk all 13 angles in ONE launch, the x angle in workgroups behind the line roles' that
pull their row groups from counters.  Every case is compared bit for bit with the CPU checker and must have taken the
fixed-window route.

A volume only pulls row groups at the default settings when it has more groups than the x workgroups have walking waves
(more than 131 072 rows on 256 CUs), which no CPU checker answers in seconds, so every case also runs with the hand-out
forced: PRAD_FW_XBLOCKS=2 leaves 16 static groups and sends the rest through the counters, PRAD_FW_XGPD=3 makes the batches
ragged against the ranges' ends.  One large volume runs the default hand-out against the two-launch route instead."""
import numpy as np
import pytest

from test_gpu_fw import _levels, _mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm():
    from pyradiomics_amd import cmatrices
    return cmatrices


def _slab(shape, Ng):
    """a flat slab inside noise: every row crosses it, many rows end a long run at the same step"""
    img = _levels(4, shape, Ng, "uniform")
    img[shape[0] // 4: shape[0] // 2, 3:-3, 10:-10] = 7
    return img


def _planes_mask(shape):
    m = np.ones(shape, bool)
    m[shape[0] // 3: shape[0] // 3 + 3] = False
    m[:, 5:9] = False
    m[:, :, 100:140] = False
    return m


def _edge_mask(shape):
    m = np.ones(shape, bool)
    m[:, :, :3] = False
    m[:, :, -2:] = False
    return m


FULL = "full"
# name -> (shape, Ng, levels, mask)
CASES = {
    # fewer than 64 rows left for the last wave (360 rows: 5 groups and 40 rows), a last tile of one voxel.  At the default
    # settings this volume (and the next) gets ONE x workgroup; "far more x workgroups and waves than groups, most leave without
    # touching anything" is test_xrole_knobs with PRAD_FW_XBLOCKS=64 on the same two volumes: 63 of 64 workgroups leave
    "40x9x65": ((40, 9, 65), 32, lambda s, n: _levels(1, s, n, "uniform"), FULL),
    # the smallest volume that still takes the fixed-window route: rows of 65 voxels, two rows by two planes
    "2x2x65": ((2, 2, 65), 32, lambda s, n: _levels(2, s, n, "uniform"), FULL),
    # 4160 rows: the 8-row interleave with a ragged last block of 512
    "65x64x80": ((65, 64, 80), 32, lambda s, n: _levels(3, s, n, "smooth"), FULL),
    # row ends inside a 16-byte piece
    "9x40x72": ((9, 40, 72), 32, lambda s, n: _levels(4, s, n, "uniform"), FULL),
    # a third tile of two voxels
    "9x40x130": ((9, 40, 130), 32, lambda s, n: _levels(5, s, n, "smooth"), FULL),
    # whole tiles; the row fills the window
    "26x26x128": ((26, 26, 128), 32, lambda s, n: _levels(6, s, n, "uniform"), FULL),
    "20x24x512": ((20, 24, 512), 32, lambda s, n: _levels(7, s, n, "smooth"), FULL),
    # runs longer than the x table's length slots (85 + 64 at 16 levels): the global long-run route
    "24x70x300-flat": ((24, 70, 300), 16, lambda s, n: _levels(3, s, n, "flat"), FULL),
    "24x70x300-blobs": ((24, 70, 300), 16, lambda s, n: _levels(3, s, n, "blobs"), FULL),
    "24x70x300-slab": ((24, 70, 300), 16, lambda s, n: _slab(s, n), FULL),
    # the zero-aware path
    "ball": ((30, 18, 257), 32, lambda s, n: _levels(8, s, n, "blobs"), "ball"),
    "random70": ((30, 18, 257), 32, lambda s, n: _levels(9, s, n, "uniform"), "random"),
    "empty-planes": ((20, 24, 512), 32, lambda s, n: _levels(10, s, n, "uniform"), _planes_mask),
    # rows that begin and end outside the ROI
    "edge-columns": ((9, 40, 130), 32, lambda s, n: _levels(11, s, n, "smooth"), _edge_mask),
}

_built = {}


def _case(name, checker):
    """volume, mask and the checker's matrices of a case: computed once, shared by every hand-out, never written to"""
    if name not in _built:
        shape, Ng, lev, mk = CASES[name]
        img = lev(shape, Ng)
        mask = mk(shape) if callable(mk) else _mask(2, shape, mk)
        Nr = int(max(shape))
        eg, eang = checker.calculate_glcm(img, mask, [1], Ng, False, 0)
        er, _ = checker.calculate_glrlm(img, mask, Ng, Nr, False, 0)
        for a in (img, mask, eg, er, eang):
            a.setflags(write=False)
        _built[name] = (img, mask, Ng, Nr, eg, er, eang)
    return _built[name]


HANDOUTS = {
    "default": {},
    "pulled": {"PRAD_FW_XBLOCKS": "2", "PRAD_FW_XGPD": "3"},
}


def _run(cm, img, mask, Ng, Nr):
    from pyradiomics_amd import _lib
    g, r, ang = cm.calculate_glcm_glrlm(img, mask, Ng, Nr, False, 0)
    assert _lib.last_path() == "sweep"
    assert _lib.last_variant() == "fw"
    return g, r, ang


@pytest.mark.parametrize("handout", list(HANDOUTS))
@pytest.mark.parametrize("name", list(CASES))
def test_xrole_matches_the_checker(cm, checker, name, handout, monkeypatch):
    img, mask, Ng, Nr, eg, er, eang = _case(name, checker)
    for k, v in HANDOUTS[handout].items():
        monkeypatch.setenv(k, v)
    g, r, ang = _run(cm, img, mask, Ng, Nr)
    assert np.array_equal(ang, eang)
    assert np.array_equal(g, eg), "GLCM differs at (i, j, angle) %s" % (np.argwhere(g != eg)[:3],)
    assert np.array_equal(r, er), "GLRLM differs at (i, len-1, angle) %s" % (np.argwhere(r != er)[:3],)


@pytest.mark.parametrize("env", [
    {"PRAD_FW_XBLOCKS": "64"},                                # far more x workgroups than groups: most leave untouched
    {"PRAD_FW_XBLOCKS": "1", "PRAD_FW_XGPD": "1"},            # one workgroup pulls everything, one group at a time
    {"PRAD_FW_XBLOCKS": "3", "PRAD_FW_XGPD": "64"},           # one pull empties a range
    {"PRAD_FW_ROWS_THREADS": "1024"},                         # the 16-wave shape: 16 tiles and the table that still fits
    {"PRAD_FW_ROWS_THREADS": "1024", "PRAD_FW_XBLOCKS": "1", "PRAD_FW_XGPD": "2"},
    {"PRAD_FW_XROLE": "0"},                                   # the switch: the two launches
], ids=lambda e: ",".join("%s=%s" % (k[8:], v) for k, v in e.items()))
@pytest.mark.parametrize("name", ["40x9x65", "2x2x65", "65x64x80", "24x70x300-slab", "random70"])
def test_xrole_knobs(cm, checker, name, env, monkeypatch):
    img, mask, Ng, Nr, eg, er, _ = _case(name, checker)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, r, _ = _run(cm, img, mask, Ng, Nr)
    assert np.array_equal(g, eg) and np.array_equal(r, er)


def test_default_handout_pulls_on_a_large_volume_and_equals_the_two_launches(cm, monkeypatch):
    """133 120 rows: 2080 groups against the 2048 static ones of 256 x workgroups (fewer CUs: more pulled); masked"""
    shape = (520, 256, 80)
    img = np.random.default_rng(5).integers(1, 33, size=shape).astype(np.int32)
    mask = np.random.default_rng(6).random(shape) < 0.9
    g1, r1, _ = _run(cm, img, mask, 32, 520)
    monkeypatch.setenv("PRAD_FW_XROLE", "0")
    g0, r0, _ = _run(cm, img, mask, 32, 520)
    assert np.array_equal(g0, g1) and np.array_equal(r0, r1)


def test_one_launch_per_call(cm, monkeypatch):
    """a fused-table call records one launch of family "sweep" and none of family "rows"; the switch brings the second back"""
    import torch
    from pyradiomics_amd import engine
    shape = (20, 24, 512)
    img = torch.from_numpy(_levels(7, shape, 32, "uniform")).cuda()
    mask = torch.from_numpy(_mask(1, shape, "ball").astype(np.uint8)).cuda()
    engine.glcm_glrlm(img, mask, 32, 512)
    engine.timing_begin()
    try:
        g1, r1, _ = engine.glcm_glrlm(img, mask, 32, 512)
        g1, r1 = g1.clone(), r1.clone()
        assert engine.last_path() == "sweep" and engine.last_variant() == "fw"
        assert engine.timing_count("sweep") == 1
        assert engine.timing_count("rows") == 0
    finally:
        engine.timing_end()
    monkeypatch.setenv("PRAD_FW_XROLE", "0")
    engine.timing_begin()
    try:
        g0, r0, _ = engine.glcm_glrlm(img, mask, 32, 512)
        assert engine.timing_count("sweep") == 1
        assert engine.timing_count("rows") == 1
    finally:
        engine.timing_end()
    assert torch.equal(g0, g1) and torch.equal(r0, r1)


@pytest.mark.parametrize("handout", ["default", "one-workgroup"])
def test_deferred_pipeline_through_the_xrole(cm, checker, handout, monkeypatch):
    """five volumes back to back: three fused-table volumes of different shapes, a 64-level volume between them and one
    with a level outside [1, Ng] under the mask.  The regular ones equal their synchronous results and the checker, the
    irregular one is reported, and the volumes behind it are still right (its x workgroups honour the levels flag like the
    rows kernel, and its launch still packs the next volume).  "one-workgroup": PRAD_FW_XBLOCKS=1, so that all but eight row
    groups of every volume go through the head words, which the pipeline has to hand over zeroed for every volume"""
    import torch
    from pyradiomics_amd import engine
    if handout == "one-workgroup":
        monkeypatch.setenv("PRAD_FW_XBLOCKS", "1")

    def variant(Ng):
        assert engine.last_path() == "sweep"
        assert engine.last_variant() == ("fw" if Ng <= 44 else "fw2")
    specs = [((24, 30, 512), 32, "uniform", "ball"), ((18, 30, 304), 64, "smooth", "full"), ((20, 26, 256), 32, "smooth", "random"),
             ((24, 30, 512), 32, "uniform", "full"), ((18, 22, 304), 32, "blobs", "ball")]
    vols = [(_levels(70 + i, s, Ng, k), _mask(80 + i, s, m), Ng) for i, (s, Ng, k, m) in enumerate(specs)]
    BAD = 3
    bad = vols[BAD][0].copy()
    bad[5, 6, 7] = 33
    vols[BAD] = (bad, vols[BAD][1], 32)
    dev = [(torch.from_numpy(i).cuda(), torch.from_numpy(m.astype(np.uint8)).cuda(), Ng) for i, m, Ng in vols]
    want = {}
    for n, (i, m, Ng) in enumerate(dev):
        if n != BAD:
            g, r, _ = engine.glcm_glrlm(i, m, Ng, 512)
            variant(Ng)
            want[n] = (g.clone(), r.clone())
    engine.set_deferred_mode(1)
    try:
        got = []
        for i, m, Ng in dev:
            got.append(engine.glcm_glrlm(i, m, Ng, 512, deferred=True))
            variant(Ng)
        engine.deferred_join()
        with pytest.raises(RuntimeError):
            engine.deferred_status()
        engine.deferred_status()
        for n, (img, mask, Ng) in enumerate(vols):
            if n == BAD:
                continue
            g, r, _ = got[n]
            assert torch.equal(g, want[n][0]) and torch.equal(r, want[n][1]), "volume %d differs from its synchronous result" % n
            eg, _ = checker.calculate_glcm(img, mask, [1], Ng, False, 0)
            er, _ = checker.calculate_glrlm(img, mask, Ng, 512, False, 0)
            assert np.array_equal(g.cpu().numpy(), eg[0]) and np.array_equal(r.cpu().numpy(), er[0]), "volume %d differs from the checker" % n
    finally:
        engine.set_deferred_mode(-1)

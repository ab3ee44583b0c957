"""The pack of the NEXT volume as a side job of the walk launches (csrc/kernels_sweepfw.h PackWave, csrc/kernels_sweepfw2.h
PackWave16), whose loads and stores go through global -- not flat -- addresses (csrc/kernels_sweep.h global_load16 /
global_store16).

Deferred pipeline runs of four volumes with a seed each, so that three packs ride.  Every result is compared bit for bit with
the CPU checker AND with the same run under PRAD_NO_INLINE_PACK=1 (every pack a launch of its own).  The "pack" timing family
counts stand-alone pack launches only: a run must show no more of them than the ramp of its pipelines, since a volume whose pack
did not ride tests nothing here.

Rows are whole 16-voxel pieces (a pack rides only then) and the number of pieces is no multiple of 64, bar one shape: the last
unit has idle lanes, and most of the launch's 4096 waves own no unit at all.
  (20, 24, 512)  15 360 pieces
  (7, 9, 128)    504 pieces = 7 units + 56 lanes
  (3, 5, 1024)   960 pieces = 15 units exactly.  Its rows are too long for the two-table walk (prad_sweep_plan.h: up to 512
                 voxels), so at 64 levels it runs on the wrapped-lines kernels, outside the pipeline: compared all the same, but
                 no pack rides there
  (5, 7, 80)     175 pieces, an 80-voxel row on the 256-column window: padded window columns
"""
import numpy as np
import pytest

import sweep_plan_cases as spc
from test_gpu_fw import _levels
from test_gpu_fin_ride import _assert_equal
from test_gpu_twin_pipeline import _run, _twin

pytestmark = pytest.mark.gpu

SHAPES = [(20, 24, 512), (7, 9, 128), (3, 5, 1024), (5, 7, 80)]
NVOL = 4


@pytest.fixture(scope="module")
def engine():
    from pyradiomics_amd import engine
    return engine


def _variant(shape, Ng):
    """what the planner makes of the shape (prad_sweep_plan.h plan_lines_shape / plan_tables)"""
    if Ng <= 44:
        return "fw" if 64 < shape[2] <= 1024 else "lines"
    return "fw2" if 64 < shape[2] <= 512 else "lines"


_want = {}


def _vol(checker, key, img, mask, Ng, regular=True):
    """-> (device image, device mask, Ng, Nr, checker GLCM, checker GLRLM) as test_gpu_fin_ride._vol; computed once per key.
    regular=False: a level outside 1..Ng under the mask -- no expectation (the deferred status reports the volume)"""
    import torch
    if key not in _want:
        Nr = int(max(img.shape))
        eg = er = None
        if regular:
            g, _ = checker.calculate_glcm(img, mask, [1], Ng, False, 0)
            r, _ = checker.calculate_glrlm(img, mask, Ng, Nr, False, 0)
            eg, er = torch.from_numpy(np.ascontiguousarray(g[0])).cuda(), torch.from_numpy(np.ascontiguousarray(r[0])).cuda()
        _want[key] = (torch.from_numpy(img).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda(), Ng, Nr, eg, er)
    return _want[key]


def _iid(checker, shape, Ng, seed, mask=None, edit=None, regular=True, tag=""):
    """iid levels 1..Ng of seed `seed` under `mask` (default: full); edit(img) changes the image in place"""
    img = _levels(seed, shape, Ng, "uniform")
    if edit is not None:
        edit(img)
    if mask is None:
        mask = np.ones(shape, bool)
    return _vol(checker, (shape, Ng, seed, tag), img, mask, Ng, regular)


def _both(engine, monkeypatch, vols, variant, ramp=1, skip=(), expect_raise=False):
    """the run with riding packs and with PRAD_NO_INLINE_PACK=1: both equal to the checker, hence to each other -- and compared
    with each other as well, which covers the volumes the checker has no expectation for"""
    import torch
    n = len(vols)
    rides = variant in ("fw", "fw2")
    monkeypatch.delenv("PRAD_NO_INLINE_PACK", raising=False)
    got1, counts1, raised1, _ = _run(engine, vols, timing=True)
    assert engine.last_variant() == variant
    monkeypatch.setenv("PRAD_NO_INLINE_PACK", "1")
    got0, counts0, raised0, _ = _run(engine, vols, timing=True)
    monkeypatch.delenv("PRAD_NO_INLINE_PACK")
    print("stand-alone packs: %d riding run, %d with PRAD_NO_INLINE_PACK=1" % (counts1["pack"], counts0["pack"]))
    assert raised1 == expect_raise and raised0 == expect_raise
    _assert_equal(got1, vols, skip=skip)
    _assert_equal(got0, vols, skip=skip)
    for i, ((g1, r1), (g0, r0)) in enumerate(zip(got1, got0)):
        if i not in skip:
            assert torch.equal(g1, g0) and torch.equal(r1, r0), "volume %d: riding pack != stand-alone pack" % i
    assert counts0["pack"] == n, counts0
    if rides:
        assert counts1["pack"] <= ramp, "only the ramp's packs may be launches of their own: %s" % counts1
    else:
        assert counts1["pack"] == n, counts1


# ---- full mask, iid levels: the fast path of the conversion ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_full_mask_32_levels(engine, checker, monkeypatch, shape):
    vols = [_iid(checker, shape, 32, 1000 + i) for i in range(NVOL)]
    _both(engine, monkeypatch, vols, "fw")


@pytest.mark.parametrize("shape", SHAPES)
def test_full_mask_64_levels(engine, checker, monkeypatch, shape):
    vols = [_iid(checker, shape, 64, 1100 + i) for i in range(NVOL)]
    _both(engine, monkeypatch, vols, _variant(shape, 64))


# ---- both kinds of pipeline --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("twin", ["1", "0"])
def test_twin_on_and_off(engine, checker, monkeypatch, twin, Ng):
    shape = SHAPES[0]
    vols = [_iid(checker, shape, Ng, (1000 if Ng == 32 else 1100) + i) for i in range(NVOL)] + [_iid(checker, shape, Ng, 1200 + Ng)]
    _twin(monkeypatch, twin)
    _both(engine, monkeypatch, vols, _variant(shape, Ng), ramp=2 if twin == "1" else 1)
    _twin(monkeypatch, None)


# ---- holes in the mask: the general path and the row flags -------------------------------------------------------------------------
def _hole_masks(shape):
    """a single voxel; a hole that straddles a row end (rows are whole pieces, so it lies in the last piece of one row and
    the first piece of the next: two lanes on the general path, two row flags)"""
    n, nx = int(np.prod(shape)), shape[2]
    one = np.ones(n, bool)
    one[(n // 2 // nx) * nx + 37] = False
    row = max(1, (n // nx) // 3)
    two = np.ones(n, bool)
    two[row * nx - 3:row * nx + 3] = False
    return one.reshape(shape), two.reshape(shape)


@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_holes_in_the_mask(engine, checker, monkeypatch, shape, Ng):
    one, two = _hole_masks(shape)
    base = 1000 if Ng == 32 else 1100
    vols = [_iid(checker, shape, Ng, base), _iid(checker, shape, Ng, 1300 + Ng, mask=one, tag="one"),
            _iid(checker, shape, Ng, 1301 + Ng, mask=two, tag="two"), _iid(checker, shape, Ng, base + 1),
            _iid(checker, shape, Ng, 1302 + Ng, mask=one & two, tag="both")]
    _both(engine, monkeypatch, vols, _variant(shape, Ng))


# ---- an irregular level under the mask, in the last piece of the last unit ---------------------------------------------------------
@pytest.mark.parametrize("level", [0, 300])
@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_irregular_level_in_the_last_piece(engine, checker, monkeypatch, shape, Ng, level):
    """the deferred status reports the volume, its neighbours are untouched, and the synchronous call ends on the exact kernels
    with what the reference says"""
    from pyradiomics_amd import cmatrices as cm, _lib
    base = 1000 if Ng == 32 else 1100
    n = int(np.prod(shape))

    def edit(img):
        img.reshape(-1)[n - 5] = level

    bad = _iid(checker, shape, Ng, 1400 + Ng, edit=edit, regular=False, tag="level%d" % level)
    vols = [_iid(checker, shape, Ng, base), _iid(checker, shape, Ng, base + 1), bad, _iid(checker, shape, Ng, base + 2)]
    _both(engine, monkeypatch, vols, _variant(shape, Ng), skip=(2,), expect_raise=True)
    img, mask = bad[0].cpu().numpy(), bad[1].cpu().numpy().astype(bool)
    try:
        want = checker.calculate_glcm(img, mask, [1], Ng, False, 0)
    except IndexError:
        with pytest.raises(IndexError):
            cm.calculate_glcm(img, mask, [1], Ng, False, 0)
    else:      # (the reference aliases some out-of-range levels silently)
        assert np.array_equal(cm.calculate_glcm(img, mask, [1], Ng, False, 0)[0], want[0])
    assert _lib.last_path() == "generic"


# ---- runs along z longer than the table's length slots -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_run_longer_than_the_length_slots(engine, checker, monkeypatch, shape):
    """A slab of one level, RS + 2 thick along z: slow steps and chunk boundaries while a unit's loads are in flight.  These
    volumes are thinner than the table's length slots (RS = 25 at 32 levels), so the existing tuning override PRAD_FW_RS
    shortens the table to RS = Nz - 3 (at least 1): the slab then is Nz - 1 planes thick (all 3 planes of the 3-plane shape)."""
    from pyradiomics_amd import _lib
    lib = _lib.load()
    Nz, Ny, Nx = shape
    rs = max(1, Nz - 3)
    monkeypatch.setenv("PRAD_FW_RS", str(rs))
    rec = spc.plan(lib, np.array(shape + (32, 0, 3, 0, 0, -1), np.int32))
    assert rec[0] == 1 and rec[5] == 1 and rec[10] == rs and rec[16] == 1, rec[:20].tolist()      # ok, fw, RSfw, LONGfw
    thick = rs + 2
    z0 = Nz - thick

    def edit_for(level):
        def edit(img):
            img[z0:z0 + thick, 1:Ny - 1, 5:Nx - 9] = level
        return edit

    vols = [_iid(checker, shape, 32, 1000), _iid(checker, shape, 32, 1500, edit=edit_for(7), tag="slab7"),
            _iid(checker, shape, 32, 1501, edit=edit_for(32), tag="slab32"), _iid(checker, shape, 32, 1001)]
    _both(engine, monkeypatch, vols, "fw")
    monkeypatch.delenv("PRAD_FW_RS")

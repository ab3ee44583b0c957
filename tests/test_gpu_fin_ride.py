"""The finalize of a deferred fused-table volume and the zeroing for the next ones as a riding job of the NEXT walk launch
(csrc/kernels_sweepfw.h FinJob; csrc/prad_pipeline.h, csrc/prad_pipe_plan.h: the pipeline's `walked` slot and its four workspace sets): a steady step of
same-shaped volumes is one launch.

Every result is compared bit for bit with the CPU checker AND with the same sequence under PRAD_FIN_RIDE=0 (the stand-alone
finalize_volume_kernel behind every walk launch, zero3_kernel in front of every pack).  The "finalize" timing family counts
stand-alone finalize launches only: that is how a test knows whether the job rode."""
import numpy as np
import pytest

from test_gpu_fw import _levels, _mask
from test_gpu_finalize_one import MULTI, SPECS, SHAPE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pyradiomics_amd import engine
    return engine


_want = {}


def _vol(checker, seed, shape, Ng, kind, mkind, mask=None):
    """-> (device image, device mask, Ng, Nr, checker GLCM [Ng,Ng,Na], checker GLRLM [Ng,Nr,Na], angles); computed once per key"""
    import torch
    key = (seed, shape, Ng, kind, mkind if mask is None else ("given", mask.tobytes()))
    if key not in _want:
        img = _levels(seed, shape, Ng, kind)
        m = _mask(seed + 50, shape, mkind) if mask is None else mask
        Nr = int(max(shape))
        eg, eang = checker.calculate_glcm(img, m, [1], Ng, False, 0)
        er, _ = checker.calculate_glrlm(img, m, Ng, Nr, False, 0)
        _want[key] = (torch.from_numpy(img).cuda(), torch.from_numpy(m.astype(np.uint8)).cuda(), Ng, Nr,
                      torch.from_numpy(np.ascontiguousarray(eg[0])).cuda(), torch.from_numpy(np.ascontiguousarray(er[0])).cuda(),
                      [tuple(int(c) for c in a) for a in eang])
    return _want[key]


def _run(engine, vols, end="join", timing=False, mark_after=None):
    """the volumes through the deferred pipeline -> (results, stand-alone finalize launches or None, raised?)"""
    import torch
    engine.set_deferred_mode(1)
    try:
        if timing:
            engine.timing_begin()
        got, tokens = [], []
        for n, v in enumerate(vols):
            g, r, _ = engine.glcm_glrlm(v[0], v[1], v[2], v[3], deferred=True)
            assert engine.last_path() == "sweep"
            got.append((g, r))
            if mark_after is not None and n == mark_after:
                tokens.append(engine.deferred_mark())
        if end == "join":
            engine.deferred_join()
            # a torch kernel on the same stream reads the outputs without a host synchronisation
            got = [(g.clone(), r.clone()) for g, r in got]
        marked = [engine.deferred_wait(t) for t in tokens]
        raised = False
        try:
            engine.deferred_status()
        except RuntimeError:
            raised = True
        engine.deferred_status()      # the verdict is reported once
        nfin = engine.timing_count("finalize") if timing else None
        if timing:
            engine.timing_end()
        torch.cuda.synchronize()
        return [(g.clone(), r.clone()) for g, r in got], nfin, raised, marked
    finally:
        engine.set_deferred_mode(-1)


def _assert_equal(got, vols, skip=()):
    import torch
    for n, ((g, r), v) in enumerate(zip(got, vols)):
        if n in skip:
            continue
        assert torch.equal(g, v[4]), "volume %d: GLCM differs from the checker at (i, j, angle) %s" % (n, (g != v[4]).nonzero()[:3].tolist())
        assert torch.equal(r, v[5]), "volume %d: GLRLM differs from the checker at (i, len-1, angle) %s" % (n, (r != v[5]).nonzero()[:3].tolist())


def _both(engine, monkeypatch, vols, **kw):
    """the sequence with the route on and off: both equal to the checker (hence to each other) -> (finalize launches on, off)"""
    monkeypatch.delenv("PRAD_FIN_RIDE", raising=False)
    got1, n1, raised1, _ = _run(engine, vols, **kw)
    monkeypatch.setenv("PRAD_FIN_RIDE", "0")
    got0, n0, raised0, _ = _run(engine, vols, **kw)
    monkeypatch.delenv("PRAD_FIN_RIDE")
    assert not raised1 and not raised0
    _assert_equal(got1, vols)
    _assert_equal(got0, vols)
    return n1, n0


# ---- runs of one shape: ramp, steady state, drain -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mkind", [("uniform", "full"), ("smooth", "ball"), ("blobs", "random")])
@pytest.mark.parametrize("shape", [(2, 2, 65), (9, 40, 130), (12, 20, 257), (20, 24, 512)])
def test_runs_of_one_shape(engine, checker, monkeypatch, shape, kind, mkind):
    vols = [_vol(checker, 100 + i, shape, 32, kind, mkind) for i in range(6)]
    for n in (1, 2, 3, 4):
        _both(engine, monkeypatch, vols[:n])
    n1, n0 = _both(engine, monkeypatch, vols, timing=True)
    assert n0 == 6
    assert n1 <= 2, "the finalize of a steady step did not ride: %d stand-alone launches in a run of 6" % n1


# ---- the replayed planner is the live one: it names the stand-alone finalize launches that the device then counts ---------------
def _pipe_event(lib, v):
    """the deferred call of volume v as an event of prad_debug_pipe_plan: what the executor reads off the sweep plan (fin_can_ride,
    fin_host_ok of csrc/prad_pipeline.h) restated on the record of prad_debug_sweep_plan, planned for the device's compute units"""
    import ctypes as C
    from test_pipe_plan import call
    shape, Ng, Nr = tuple(v[0].shape), v[2], v[3]
    angles = np.ascontiguousarray(v[6], dtype=np.int32)
    out = np.zeros(4096, np.int32)
    n = lib.prad_debug_sweep_plan((C.c_int * 3)(*shape), 3, angles.ctypes.data_as(C.POINTER(C.c_int)), len(angles), Ng, Nr, 1, 1, 0,
                                  out.ctypes.data_as(C.POINTER(C.c_int)), len(out))
    assert n > 42 and out[0] == 1
    fused, fw, lds_fw, lds_fw_rows, fw_blocks, row_slot, fw_xblocks, nlines = (int(out[i]) for i in (4, 5, 21, 22, 29, 39, 40, 41))
    Na = int(out[42 + 10 * nlines])
    assert fused and fw and nlines > 0 and Na == len(angles)
    can_ride = not (row_slot >= 0 and fw_xblocks == 0) and Ng <= 255 and Na <= 16 and (Ng * Nr + Ng * Ng) * Na < 2 ** 31
    lds = max(lds_fw, lds_fw_rows) if fw_xblocks > 0 else lds_fw
    host_plan_ok = lds >= 7176 and 1 <= fw_blocks < 32768      # (sizeof(FinScratch), csrc/kernels_sweep.h)
    # (whether the pack rides is not counted below: a stand-alone pack is timed as "pack")
    return call(shape, Ng, can_ride=int(can_ride), host_plan_ok=int(host_plan_ok), inline=0, acc=len(angles) * Ng * (Ng + Nr) + 2000)


@pytest.mark.parametrize("run", ["six of one shape", "large first"])
def test_replayed_plan_counts_the_live_launches(engine, checker, monkeypatch, run):
    """Six (9, 40, 130) volumes, and the `large first` sequence of test_zero_extents: the stand-alone finalize launches that
    prad_debug_pipe_plan plans for the sequence are exactly the ones the "finalize" timing family counts on the device, with the
    route on and with PRAD_FIN_RIDE=0.  (zero3_kernel is timed under no family: its launches are pinned on the host alone,
    tests/test_pipe_plan.py.)"""
    from pyradiomics_amd import _lib
    from test_pipe_plan import FINALIZE, flush, kinds, plan
    lib = _lib.load()
    if run == "large first":
        vols = [_vol(checker, 300 + i, (9, 40, 130), 32, "uniform", "random") for i in range(5)]
        vols += [_vol(checker, 310 + i, (2, 2, 65), 32, "uniform", "full") for i in range(5)]
    else:
        vols = [_vol(checker, 100 + i, (9, 40, 130), 32, "uniform", "full") for i in range(6)]
    for ride in (1, 0):
        monkeypatch.delenv("PRAD_FIN_RIDE", raising=False)
        if not ride:
            monkeypatch.setenv("PRAD_FIN_RIDE", "0")
        records, _ = plan(lib, [dict(_pipe_event(lib, v), fin_ride=ride) for v in vols] + [flush(ride)])
        got, nfin, raised, _ = _run(engine, vols, timing=True)
        assert not raised
        _assert_equal(got, vols)
        assert nfin == kinds(records, FINALIZE), (run, ride, nfin, records)
    monkeypatch.delenv("PRAD_FIN_RIDE")


# ---- the job carries the geometry of volume N-2, not the launch's -------------------------------------------------------------
def test_changing_shapes(engine, checker, monkeypatch):
    shapes = [(24, 30, 512), (20, 26, 256), (18, 22, 300), (30, 30, 64), (24, 30, 512)]
    kinds = ["smooth", "uniform", "blobs", "uniform", "smooth"]
    masks = ["ball", "random", "full", "ball", "random"]
    vols = [_vol(checker, 200 + i, s, 32, k, m) for i, (s, k, m) in enumerate(zip(shapes, kinds, masks))]
    _both(engine, monkeypatch, vols)
    _both(engine, monkeypatch, vols[::-1])


# ---- zero extents: a small and a large volume meet the same workspace set -----------------------------------------------------
@pytest.mark.parametrize("first", ["large", "small"])
def test_zero_extents(engine, checker, monkeypatch, first):
    large = [_vol(checker, 300 + i, (9, 40, 130), 32, "uniform", "random") for i in range(5)]
    small = [_vol(checker, 310 + i, (2, 2, 65), 32, "uniform", "full") for i in range(5)]
    a, b = (large, small) if first == "large" else (small, large)
    _both(engine, monkeypatch, a + b)              # ten calls: every set holds one of each, in this order
    _both(engine, monkeypatch, a[:4] + b[:1] + a[4:] + b[1:])


# ---- a two-table volume finalizes stand-alone and drains the walked volume first ----------------------------------------------
def test_32_and_64_levels_alternating(engine, checker, monkeypatch):
    vols = [_vol(checker, 400 + i, s, Ng, k, m) for i, (s, Ng, k, m) in enumerate(SPECS)]
    _both(engine, monkeypatch, vols)
    _both(engine, monkeypatch, vols + vols[:1] + vols[2:3] + vols[4:] + vols[:2])


# ---- the multi rule inside a riding angle workgroup -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one-plane", "checkerboard", "sheet", "single-voxel", "two-on-a-row"])
def test_multi_rule_rides(engine, checker, monkeypatch, name):
    full = [_vol(checker, 500 + i, SHAPE, 32, "uniform", "full") for i in range(4)]
    odd = _vol(checker, 510, SHAPE, 32, "uniform", name, mask=MULTI[name][0]())
    vols = full[:2] + [odd] + full[2:]      # the third of five: stale multi words or a stale length-1 column would show
    n1, n0 = _both(engine, monkeypatch, vols, timing=True)
    assert n0 == 5 and n1 <= 2
    keeps = MULTI[name][1]
    if keeps is not None:      # (the checker leaves the mask with the intended columns)
        for n, a in enumerate(odd[6]):
            assert bool(odd[5][:, 0, n].any()) == bool(keeps(a)), (name, a)


# ---- a level above Ng: reported once, the other volumes untouched ---------------------------------------------------------------
def test_level_above_ng(engine, checker, monkeypatch):
    import torch
    vols = [_vol(checker, 600 + i, (12, 20, 257), 32, "smooth", "random") for i in range(5)]
    bad = vols[2][0].clone()
    z, y, x = (int(c) for c in vols[2][1].nonzero()[1000])      # a voxel under the mask
    bad[z, y, x] = 33
    seq = vols[:2] + [(bad,) + vols[2][1:]] + vols[3:]
    for ride in (True, False):
        if not ride:
            monkeypatch.setenv("PRAD_FIN_RIDE", "0")
        got, _, raised, _ = _run(engine, seq)
        assert raised
        _assert_equal(got, seq, skip=(2,))
        for n in (0, 1, 3, 4):      # ... and equal to their synchronous results
            g, r, _ = engine.glcm_glrlm(seq[n][0], seq[n][1], 32, seq[n][3])
            assert torch.equal(g, got[n][0]) and torch.equal(r, got[n][1])
    monkeypatch.delenv("PRAD_FIN_RIDE")


# ---- deferred_mark / deferred_wait in the middle of a run -------------------------------------------------------------------------
@pytest.mark.parametrize("after", [0, 1, 2, 4])
def test_mark_in_the_middle(engine, checker, monkeypatch, after):
    vols = [_vol(checker, 700 + i, (9, 40, 130), 32, "smooth", "ball") for i in range(6)]
    monkeypatch.delenv("PRAD_FIN_RIDE", raising=False)
    got, _, raised, marked = _run(engine, vols, end="status", mark_after=after)
    assert not raised and marked == [True]
    _assert_equal(got, vols)


def test_mark_makes_outputs_valid(engine, checker):
    """the outputs of everything in front of a mark are valid once the mark has been waited for, with later volumes queued"""
    import torch
    vols = [_vol(checker, 720 + i, (9, 40, 130), 32, "uniform", "random") for i in range(5)]
    engine.set_deferred_mode(1)
    try:
        got = [engine.glcm_glrlm(v[0], v[1], 32, v[3], deferred=True)[:2] for v in vols[:3]]
        token = engine.deferred_mark()
        got += [engine.glcm_glrlm(v[0], v[1], 32, v[3], deferred=True)[:2] for v in vols[3:]]
        assert engine.deferred_wait(token)
        early = [(g.clone(), r.clone()) for g, r in got[:3]]
        engine.deferred_status()
        _assert_equal(early, vols[:3])
        _assert_equal(got, vols)
    finally:
        engine.set_deferred_mode(-1)


# ---- output buffers from a ring of four ---------------------------------------------------------------------------------------
def test_output_ring(engine, checker, monkeypatch):
    import torch
    shape = (12, 20, 257)
    vols = [_vol(checker, 800 + i, shape, 32, "uniform" if i % 2 else "smooth", "random") for i in range(10)]
    Na = vols[0][4].shape[2]
    for ride in (True, False):
        if not ride:
            monkeypatch.setenv("PRAD_FIN_RIDE", "0")
        ring = [(torch.full((32, 32, Na), -1.0, dtype=torch.float64, device="cuda"),
                 torch.full((32, 257, Na), -1.0, dtype=torch.float64, device="cuda")) for _ in range(4)]
        engine.set_deferred_mode(1)
        try:
            for n, v in enumerate(vols):
                engine.glcm_glrlm(v[0], v[1], 32, v[3], out_glcm=ring[n % 4][0], out_glrlm=ring[n % 4][1], deferred=True)
            engine.deferred_status()
        finally:
            engine.set_deferred_mode(-1)
        for slot in range(4):      # each buffer holds the matrices of the last volume written to it
            last = max(n for n in range(10) if n % 4 == slot)
            _assert_equal([ring[slot]], [vols[last]])
    monkeypatch.delenv("PRAD_FIN_RIDE")


# ---- the route stands aside ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["PRAD_FW_XROLE", "PRAD_FINALIZE_ONE"])
def test_route_stands_aside(engine, checker, monkeypatch, switch):
    vols = [_vol(checker, 900 + i, (12, 20, 257), 32, "blobs", "ball") for i in range(6)]
    monkeypatch.delenv("PRAD_FIN_RIDE", raising=False)
    monkeypatch.setenv(switch, "0")
    got, nfin, raised, _ = _run(engine, vols, timing=True)
    monkeypatch.delenv(switch)
    assert not raised
    _assert_equal(got, vols)
    assert nfin == 6      # every volume was finalized behind its own walk launch

"""Two interleaved deferred pipelines (csrc/prad_pipe_plan.h, "Twin"; csrc/prad_pipeline.h): with PRAD_PIPE_TWIN=1 deferred whole-volume calls are dealt
alternately onto two instances of the pipeline, each on an internal stream of its own with four workspace sets of its own, so
that consecutive walk launches are unordered on the device.

Every result is compared bit for bit with the CPU checker, with twin forced on (these shapes lie far below the automatic
threshold), forced off and with the variable unset.  The "pack" and "finalize" timing families count stand-alone launches only:
a twin run ramps both instances (two stand-alone packs) and drains both (at most two stand-alone finalizes each)."""
import threading

import numpy as np
import pytest

from test_gpu_fin_ride import _vol, _assert_equal

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 65), (9, 40, 130), (12, 20, 257), (20, 24, 512)]


@pytest.fixture(scope="module")
def engine():
    from pyradiomics_amd import engine
    return engine


def _twin(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("PRAD_PIPE_TWIN", raising=False)
    else:
        monkeypatch.setenv("PRAD_PIPE_TWIN", value)


def _run(engine, vols, end="join", timing=False, mark_after=None, outs=None, twins=None, monkeypatch=None):
    """the volumes through the deferred pipeline -> (results, {family: stand-alone launches} or None, raised?, marks)
    outs: output pair of call n (else fresh ones); twins: PRAD_PIPE_TWIN of call n (else left as it is)"""
    import torch
    engine.set_deferred_mode(1)
    try:
        if timing:
            engine.timing_begin()
        got, tokens = [], []
        for n, v in enumerate(vols):
            if twins is not None:
                _twin(monkeypatch, twins[n])
            o = outs[n] if outs is not None else (None, None)
            g, r, _ = engine.glcm_glrlm(v[0], v[1], v[2], v[3], out_glcm=o[0], out_glrlm=o[1], deferred=True)
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
        counts = {f: engine.timing_count(f) for f in ("pack", "finalize", "sweep")} if timing else None
        if timing:
            engine.timing_end()
        torch.cuda.synchronize()
        return [(g.clone(), r.clone()) for g, r in got], counts, raised, marked
    finally:
        engine.set_deferred_mode(-1)


# ---- runs of one shape: ramp, steady state and drain of both instances ---------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_runs_of_one_shape(engine, checker, monkeypatch, shape):
    vols = [_vol(checker, 100 + i, shape, 32, "smooth", "ball") for i in range(6)] + [_vol(checker, 106, shape, 32, "uniform", "random")]
    # a pack rides in the previous walk launch only with rows that are a multiple of 16 voxels: of these shapes, (20, 24, 512);
    # the packs of the others are launches of their own on either kind of pipeline
    rides = shape[2] % 16 == 0
    for twin in ("1", "0"):
        _twin(monkeypatch, twin)
        for n in range(1, 8):
            for end in ("join", "status"):
                got, counts, raised, _ = _run(engine, vols[:n], end=end, timing=True)
                assert not raised
                _assert_equal(got, vols[:n])
                assert counts["sweep"] == n, counts      # one walk launch per volume
                if twin == "1" and n >= 4:
                    assert counts["pack"] == (2 if rides else n), "twin run of %d: %s" % (n, counts)
                    assert counts["finalize"] <= 4, "twin run of %d: %s" % (n, counts)
                if twin == "0" and n >= 4:
                    assert counts["pack"] == (1 if rides else n) and counts["finalize"] <= 2, "single run of %d: %s" % (n, counts)
    _twin(monkeypatch, None)      # unset: these shapes keep the single pipeline
    got, counts, raised, _ = _run(engine, vols, timing=True)
    assert not raised
    _assert_equal(got, vols)
    assert counts["pack"] == (1 if rides else 7) and counts["finalize"] <= 2 and counts["sweep"] == 7, counts


@pytest.mark.parametrize("shape", SHAPES)
def test_mark_after_every_volume(engine, checker, monkeypatch, shape):
    vols = [_vol(checker, 100 + i, shape, 32, "smooth", "ball") for i in range(6)] + [_vol(checker, 106, shape, 32, "uniform", "random")]
    for twin in ("1", "0"):
        _twin(monkeypatch, twin)
        for k in range(7):
            got, _, raised, marked = _run(engine, vols, end="status", mark_after=k)
            assert not raised and marked == [True]
            _assert_equal(got, vols)


def test_mark_makes_outputs_valid(engine, checker, monkeypatch):
    """the outputs of everything in front of a mark -- on both instances -- are valid once the mark has been waited for"""
    vols = [_vol(checker, 720 + i, (9, 40, 130), 32, "uniform", "random") for i in range(5)]
    _twin(monkeypatch, "1")
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


# ---- changing shapes, level counts, routes and kinds of call -------------------------------------------------------------------
def test_changing_shapes_and_kinds(engine, checker, monkeypatch):
    specs = [((24, 30, 512), 32, "smooth", "ball"), ((20, 26, 256), 32, "uniform", "random"), ((9, 40, 130), 64, "smooth", "full"),
             ((18, 22, 300), 32, "blobs", "full"), ((30, 30, 64), 32, "uniform", "ball"), ((12, 20, 257), 32, "smooth", "random"),
             ((9, 40, 130), 64, "uniform", "random"), ((9, 40, 130), 64, "smooth", "full"), ((24, 30, 512), 32, "smooth", "random"),
             ((2, 2, 65), 32, "uniform", "full"), ((12, 20, 257), 32, "blobs", "full")]
    vols = [_vol(checker, 200 + i, s, Ng, k, m) for i, (s, Ng, k, m) in enumerate(specs)]
    for order in (vols, vols[::-1]):
        _twin(monkeypatch, "1")
        for end in ("join", "status"):
            got, _, raised, _ = _run(engine, order, end=end)
            assert not raised
            _assert_equal(got, order)
        # an unset-variable call (single pipeline, caller's stream) between forced-twin calls, and the reverse
        for twins in ([None, "1", "1", None, None, "1", None, "1", "1", "1", None], ["1", None, None, "1", "1", None, "1", None, "0", "1", "1"]):
            got, _, raised, _ = _run(engine, order, twins=twins, monkeypatch=monkeypatch)
            assert not raised
            _assert_equal(got, order)
    _twin(monkeypatch, None)


# ---- output buffers shared between the two instances ---------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [1, 2, 3])
def test_output_buffers_reused(engine, checker, monkeypatch, pairs):
    import torch
    shape = (12, 20, 257)
    vols = [_vol(checker, 800 + i, shape, 32, "uniform" if i % 2 else "smooth", "random") for i in range(10)]
    Na = vols[0][4].shape[2]
    for twin in ("1", "0"):
        _twin(monkeypatch, twin)
        ring = [(torch.full((32, 32, Na), -1.0, dtype=torch.float64, device="cuda"),
                 torch.full((32, 257, Na), -1.0, dtype=torch.float64, device="cuda")) for _ in range(pairs)]
        for count in (10, 7):
            _run(engine, vols[:count], end="status", outs=[ring[n % pairs] for n in range(count)])
            for slot in range(pairs):      # each buffer holds the matrices of the last volume written to it
                last = max(n for n in range(count) if n % pairs == slot)
                _assert_equal([ring[slot]], [vols[last]])


# ---- a level above Ng on either instance: reported once, the other volumes untouched -------------------------------------------
@pytest.mark.parametrize("where", [2, 3])
def test_level_above_ng(engine, checker, monkeypatch, where):
    vols = [_vol(checker, 600 + i, (12, 20, 257), 32, "smooth", "random") for i in range(5)]
    vols.append(_vol(checker, 100, (12, 20, 257), 32, "smooth", "ball"))
    bad = vols[where][0].clone()
    z, y, x = (int(c) for c in vols[where][1].nonzero()[1000])      # a voxel under the mask
    bad[z, y, x] = 33
    seq = vols[:where] + [(bad,) + vols[where][1:]] + vols[where + 1:]
    _twin(monkeypatch, "1")
    got, _, raised, marked = _run(engine, seq, mark_after=where - 1)
    assert raised and marked == [True]      # the mark in front of the volume saw nothing
    _assert_equal(got, seq, skip=(where,))
    got, _, raised, marked = _run(engine, seq, end="status", mark_after=where)
    assert marked == [False] and not raised      # a mark behind it reports it (deferred_wait queries the status: reported once)
    _assert_equal(got, seq, skip=(where,))
    got, _, raised, _ = _run(engine, vols)      # the verdict did not outlive its query
    assert not raised
    _assert_equal(got, vols)


# ---- a caller's stream that is not the default one -----------------------------------------------------------------------------
def test_non_default_stream(engine, checker, monkeypatch):
    import torch
    vols = [_vol(checker, 100 + i, (20, 24, 512), 32, "smooth", "ball") for i in range(6)]
    _twin(monkeypatch, "1")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    engine.set_deferred_mode(1)
    try:
        with torch.cuda.stream(side):
            got = []
            for v in vols:
                img = v[0] + 0      # (a kernel on the caller's stream feeds the call: the internal stream has to wait for it)
                got.append(engine.glcm_glrlm(img, v[1], v[2], v[3], deferred=True)[:2])
            engine.deferred_join()
            copies = [(g.clone(), r.clone()) for g, r in got]      # on `side`, right behind the join: no host synchronisation
        side.synchronize()
        _assert_equal(copies, vols)
        engine.deferred_status()
    finally:
        engine.set_deferred_mode(-1)


# ---- two host threads, each with twin pipelines of its own ---------------------------------------------------------------------
def test_two_host_threads(engine, checker, monkeypatch):
    import torch
    runs = [[_vol(checker, 100 + i, (9, 40, 130), 32, "smooth", "ball") for i in range(6)],
            [_vol(checker, 800 + i, (12, 20, 257), 32, "uniform" if i % 2 else "smooth", "random") for i in range(7)]]
    _twin(monkeypatch, "1")
    sequential = [_run(engine, vols)[0] for vols in runs]
    results, errors = [None, None], []

    def work(t):
        try:
            torch.cuda.set_device(0)
            results[t] = _run(engine, runs[t], end="status" if t else "join")[0]
            engine.release_workspace()
        except Exception as e:      # noqa: BLE001 -- reported by the asserting thread
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        _assert_equal(results[t], runs[t])
        for (g, r), (sg, sr) in zip(results[t], sequential[t]):
            assert torch.equal(g, sg) and torch.equal(r, sr)

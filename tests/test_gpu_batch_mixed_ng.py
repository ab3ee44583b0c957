"""A grey-level count PER ROI on the batched small-ROI route (an int sequence `Ng` [B]; prad_calculate_batch_ng_dev,
prad_batch_glszm[_fill]_ng_dev, prad_batch_merge_angles_ng_dev, prad_batch_features_ng_dev): one batch whose ROIs differ in
their counts against, ROI by ROI, the calls on that ROI alone with its own count -- the single device calls where the box has
an angle, the scalar batched call on the one ROI everywhere -- and, for one small ROI, the reference C through the oracle.

Everything compared here is a count or the output of the same device function on the same matrix values, so every comparison
is bit for bit; the one tolerance is the bound tests/test_gpu_batch_rois.py applies to the NGTDM float column against the
REFERENCE (rtol 1e-12), used for the oracle comparison alone.

Shapes: the ragged list of tests/test_gpu_batch_rois.py (unaligned offsets, axes of length 1 and 2, a 16^3 box, one box of
exactly prad_batch_max_vox() voxels) with the counts 64, 1, 2, 7, 33, 63, 5: the cap, the smallest, odd ones.  What a
uniform count cannot catch is a value of ANOTHER ROI used for this one: the largest count in the range check (a level above
the ROI's own count but below the batch's largest must void that ROI alone), another ROI's count or extents in the table
sizes (the LDS tables are sized once per batch), another ROI's row count in the fill, the merge and the formulas."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMILIES = ("glcm", "glrlm", "gldm", "ngtdm")
NGTDM_RTOL = 1e-12          # tests/test_gpu_batch_rois.py: the NGTDM float column against the reference
RAGGED = [(1, 1, 1), (1, 1, 9), (1, 8, 1), (2, 2, 2), (3, 17, 5), (16, 16, 16), (32, 40, 51)]
NG = [64, 1, 2, 7, 33, 63, 5]
# distances (1, 2, 3): boxes that keep at most 127 angles; (3, 17, 5) has 122, so its GLDM + NGTDM table of 64 levels x 245
# columns x 2 takes eight passes over the levels
NEAR = [(3, 17, 5), (2, 2, 2), (1, 1, 9), (3, 5, 4), (1, 1, 1)]
NEAR_NG = [64, 5, 33, 2, 64]


def _rois(shapes, ngs, seed, fill=0.6):
    """levels 1 .. ngs[b] and a mask per ROI; voxel 0 is masked and holds the ROI's top level"""
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(1, g + 1, size=s).astype(np.int32) for s, g in zip(shapes, ngs)]
    masks = [rng.random(s) < fill for s in shapes]
    for i, m, g in zip(imgs, masks, ngs):
        i.flat[0], m.flat[0] = g, True
    return imgs, masks


def _dev(imgs, masks):
    import torch
    return [torch.from_numpy(i).to("cuda:0") for i in imgs], [torch.from_numpy(m).to("cuda:0") for m in masks]


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _same(a, b, what):
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, "%s: shape %s != %s" % (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), what


def _alone(l, m, ng, **kw):
    """the scalar batched call on the one ROI: ({family: matrix}, status)"""
    from pyradiomics_amd import engine
    mats, status = engine.texture_matrices_batch([l], [m], None, int(ng), **kw)
    return {k: v[0] for k, v in mats.items()}, status[0]


def _single_calls(l, m, ng, dist, alpha, f2, fd):
    from pyradiomics_amd import engine
    return {"glcm": engine.glcm(l, m, ng, dist, f2, fd)[0],
            "glrlm": engine.glcm_glrlm(l, m, ng, max(l.shape), f2, fd, want_glcm=False)[1],
            "gldm": engine.gldm(l, m, ng, alpha, dist, f2, fd),
            "ngtdm": engine.ngtdm(l, m, ng, dist, f2, fd)}


def _check_matrices(shapes, ngs, seed, route="batch", **kw):
    """the mixed batch against every ROI alone; returns what the callers look at further"""
    from pyradiomics_amd import _lib, cmatrices, engine
    imgs, masks = _rois(shapes, ngs, seed)
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, ngs, **kw)
    assert engine.last_batch_route() == route
    assert route != "batch" or _lib.last_path() == "batch"
    assert status == [1] * len(shapes)
    dist, alpha = list(kw.get("distances", (1,))), kw.get("gldm_a", 0)
    f2, fd = kw.get("force2D", False), kw.get("force2Ddimension", 0)
    _, _, Na = cmatrices.batch_plan(shapes, ngs, FAMILIES, dist, f2, fd)
    for b, ng in enumerate(ngs):
        own = dict(kw, spacing=kw["spacing"][b]) if np.ndim(kw.get("spacing", 0)) == 2 else kw      # (a spacing per ROI)
        one, st = _alone(dl[b], dm[b], ng, **own)
        assert st == 1 and set(one) == set(mats)
        for key in one:
            assert mats[key][b].shape[0] == ng
            _same(mats[key][b], one[key], "ROI %d %s %s: the ROI alone" % (b, shapes[b], key))
        if Na[0, b] and Na[1, b]:
            for f, M in _single_calls(dl[b], dm[b], ng, dist, alpha, f2, fd).items():
                _same(mats[f][b], M, "ROI %d %s %s: the single call" % (b, shapes[b], f))
    return imgs, masks, mats


def test_matrices_of_a_mixed_batch(checker):
    imgs, masks, mats = _check_matrices(RAGGED, NG, 1, gldm_a=1)
    # one small ROI against the reference C
    b, ng = 4, NG[4]
    want = {"glcm": checker.calculate_glcm(imgs[b], masks[b], [1], ng, False, 0)[0][0],
            "glrlm": checker.calculate_glrlm(imgs[b], masks[b], ng, max(imgs[b].shape), False, 0)[0][0],
            "gldm": checker.calculate_gldm(imgs[b], masks[b], [1], ng, 1, False, 0)[0]}
    for f, M in want.items():
        assert np.array_equal(_np(mats[f][b]), M), f
    ngtdm = checker.calculate_ngtdm(imgs[b], masks[b], [1], ng, False, 0)[0]
    got = _np(mats["ngtdm"][b])
    assert np.array_equal(got[:, 0], ngtdm[:, 0]) and np.array_equal(got[:, 2], ngtdm[:, 2])
    np.testing.assert_allclose(got[:, 1], ngtdm[:, 1], rtol=NGTDM_RTOL, atol=0)


def test_matrices_three_distances_take_several_level_passes():
    from pyradiomics_amd import cmatrices
    _, _, Na = cmatrices.batch_plan(NEAR, NEAR_NG, FAMILIES, (1, 2, 3))
    assert Na[0, 0] == 122 and Na[0].max() <= 127 and 2 * (2 * 122 + 1) * 64 > 4 * 4096      # more than four times the table budget
    _check_matrices(NEAR, NEAR_NG, 2, distances=(1, 2, 3), gldm_a=2)
    # a box beyond the 127 angles of the native call takes the single calls; the others still share one launch
    _check_matrices(NEAR + [(7, 7, 7)], NEAR_NG + [9], 3, route="mixed", distances=(1, 2, 3))


@pytest.mark.parametrize("dim", [0, 2])
def test_matrices_force2d(dim):
    _check_matrices(RAGGED, NG, 4 + dim, force2D=True, force2Ddimension=dim)


def test_matrices_weighting_norm_covers_the_merge():
    _, _, mats = _check_matrices(RAGGED[:6], NG[:6], 7, weightingNorm="euclidean", spacing=(2.0, 1.0, 0.5))
    assert [tuple(m.shape) for m in mats["glcm_w"]] == [(g, g, 1) for g in NG[:6]]
    assert [tuple(m.shape) for m in mats["glrlm_w"]] == [(g, max(s), 1) for g, s in zip(NG[:6], RAGGED[:6])]
    spacing = np.array([[1.0, 1.0, 1.0], [2.0, 1.0, 0.5]] * 3)          # a spacing per ROI travels with the partition
    _check_matrices(RAGGED[:6], [64, 1, 70, 7, 33, 63], 8, route="mixed", weightingNorm="euclidean", spacing=spacing)


def _glszm_alone(l, m, ng, compact, **kw):
    from pyradiomics_amd import engine
    res, st = engine.glszm_batch([l], [m], None, int(ng), compact=compact, **kw)
    return res[0], st[0]


@pytest.mark.parametrize("compact", [False, True], ids=["dense", "compact"])
@pytest.mark.parametrize("f2d", [None, 0, 2])
def test_glszm_of_a_mixed_batch(checker, compact, f2d):
    from pyradiomics_amd import engine
    kw = {} if f2d is None else {"force2D": True, "force2Ddimension": f2d}
    imgs, masks = _rois(RAGGED, NG, 11, fill=0.7)
    dl, dm = _dev(imgs, masks)
    res, status = engine.glszm_batch(dl, dm, None, NG, compact=compact, **kw)
    assert engine.last_batch_route() == "mixed" and status == [1] * len(RAGGED)      # the 65 280-voxel box is above the GLSZM cap
    for b, ng in enumerate(NG):
        one, st = _glszm_alone(dl[b], dm[b], ng, compact, **kw)
        assert st == 1
        if compact:
            _same(res[b][0], one[0], "ROI %d compact matrix" % b)
            assert np.array_equal(res[b][1], one[1]) and res[b][0].shape[0] == ng
        else:
            _same(res[b], one, "ROI %d dense matrix" % b)
            assert res[b].shape[0] == ng
    if f2d is None:          # the single device call and, for one small ROI, the reference C
        for b in (1, 3, 4, 5):
            Ns = max(1, int(masks[b].sum()))
            if compact:
                P, sizes = engine.glszm_compact(dl[b], dm[b], NG[b], Ns)
                _same(res[b][0], P, "ROI %d: the single compact call" % b)
                assert np.array_equal(res[b][1], sizes)
            else:
                _same(res[b], engine.glszm(dl[b], dm[b], NG[b], Ns), "ROI %d: the single call" % b)
        if not compact:
            b = 4
            ref = checker.calculate_glszm(imgs[b], masks[b], NG[b], max(1, int(masks[b].sum())), False, 0)[0]
            assert np.array_equal(_np(res[b]), ref)
    # inside the GLSZM cap every ROI shares the two launches
    res6, status6 = engine.glszm_batch(dl[:6], dm[:6], None, NG[:6], compact=compact, **kw)
    assert engine.last_batch_route() == "batch" and status6 == [1] * 6
    for b in range(6):
        _same(res6[b][0] if compact else res6[b], res[b][0] if compact else res[b], "ROI %d of the native batch" % b)


def test_range_check_uses_the_rois_own_count():
    """ROI k holds a masked level Ng_k + 1 that the batch's largest count would let through: it alone is void"""
    from pyradiomics_amd import engine
    shapes, ngs = RAGGED[1:6], [5, 64, 7, 33, 2]
    imgs, masks = _rois(shapes, ngs, 21)
    clean = _dev(imgs, masks)
    ref, ref_status = engine.texture_matrices_batch(*clean, None, ngs)
    zref, zref_status = engine.glszm_batch(*clean, None, ngs, compact=False)
    assert ref_status == [1] * 5 and zref_status == [1] * 5
    for k in (0, 2, 4):
        bad = [i.copy() for i in imgs]
        bad[k].flat[0] = ngs[k] + 1          # (voxel 0 is masked)
        assert ngs[k] + 1 <= max(ngs)
        dl, dm = _dev(bad, masks)
        mats, status = engine.texture_matrices_batch(dl, dm, None, ngs)
        assert engine.last_batch_route() == "batch"
        assert status == [0 if b == k else 1 for b in range(5)], (k, status)
        zones, zstatus = engine.glszm_batch(dl, dm, None, ngs, compact=False)
        assert zstatus == [0 if b == k else 1 for b in range(5)], (k, zstatus)
        _, summary, lstatus = engine.glszm_batch_zones(dl, dm, None, ngs)
        assert lstatus.tolist() == zstatus and summary[k].tolist() == [0, 0, 0]
        for b in range(5):
            if b == k:          # void: the matrices of an empty mask, in the ROI's own shapes
                assert not _np(mats["glcm"][b]).any() and not _np(mats["gldm"][b]).any() and not _np(zones[b]).any()
                assert mats["glcm"][b].shape[:2] == (ngs[b], ngs[b]) and zones[b].shape == (ngs[b], 1)
                continue
            for f in FAMILIES:
                _same(mats[f][b], ref[f][b], "neighbour %d of the void ROI %d, %s" % (b, k, f))
            _same(zones[b], zref[b], "neighbour %d of the void ROI %d, GLSZM" % (b, k))
        # and the batch without ROI k
        keep = [b for b in range(5) if b != k]
        rest = ([dl[b] for b in keep], [dm[b] for b in keep], None, [ngs[b] for b in keep])
        without, wstatus = engine.texture_matrices_batch(*rest)
        zwithout, zwstatus = engine.glszm_batch(*rest, compact=False)
        assert wstatus == [1] * 4 and zwstatus == [1] * 4
        for i, b in enumerate(keep):
            for f in FAMILIES:
                _same(mats[f][b], without[f][i], "ROI %d next to the void ROI %d and without it, %s" % (b, k, f))
            _same(zones[b], zwithout[i], "ROI %d next to the void ROI %d and without it, GLSZM" % (b, k))


@pytest.mark.parametrize("order", [0, 1])
def test_table_floor_holds_every_rois_smallest_table(order):
    """a one-voxel box of 64 levels next to a box of ONE level: neither asks for more than its floor -- 64 x 64 words for the
    first --, which the other's needs must not shrink"""
    from pyradiomics_amd import engine
    imgs = [np.full((1, 1, 1), 64, np.int32), np.ones((2, 2, 2), np.int32)]
    masks = [np.ones((1, 1, 1), bool), np.ones((2, 2, 2), bool)]
    ngs = [64, 1]
    if order:
        imgs, masks, ngs = imgs[::-1], masks[::-1], ngs[::-1]
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, ngs, gldm_a=0)
    assert engine.last_batch_route() == "batch" and status == [1, 1]
    one, box = (1, 0) if order else (0, 1)
    gldm = _np(mats["gldm"][one])
    assert gldm.shape == (64, 1) and gldm[63, 0] == 1 and gldm.sum() == 1
    assert _np(mats["ngtdm"][one])[63].tolist() == [1.0, 0.0, 64.0]
    assert mats["glcm"][one].shape == (64, 64, 0) and mats["glcm"][box].shape == (1, 1, 13)
    for b in range(2):
        alone, st = _alone(dl[b], dm[b], ngs[b])
        for f in FAMILIES:
            _same(mats[f][b], alone[f], "ROI %d %s" % (b, f))
    zones, zstatus = engine.glszm_batch(dl, dm, None, ngs, compact=False)
    assert zstatus == [1, 1] and _np(zones[one])[63, 0] == 1 and _np(zones[box]).tolist() == [[0] * 7 + [1]]


def test_glrlm_column_passes_sized_by_another_rois_extents():
    """1 x 1 x 40 at 64 levels (40 run-length columns: 2 560 words per angle) next to 16^3 at 2 levels"""
    _check_matrices([(1, 1, 40), (16, 16, 16)], [64, 2], 31)
    _check_matrices([(16, 16, 16), (1, 1, 40)], [2, 64], 32)
    # run lengths beyond the columns of one pass: 1 x 1 x 300 at 64 levels builds its 300 columns 64 at a time
    imgs, masks, mats = _check_matrices([(2, 2, 2), (1, 1, 300)], [3, 64], 33)
    line = np.full((1, 1, 300), 17, np.int32)
    from pyradiomics_amd import engine
    dl, dm = _dev([imgs[0], line], [masks[0], np.ones(line.shape, bool)])
    runs, status = engine.texture_matrices_batch(dl, dm, None, [3, 64], families=("glrlm",))
    got = _np(runs["glrlm"][1])
    assert status == [1, 1] and got.shape == (64, 300, 1) and got[16, 299, 0] == 1 and got.sum() == 1


def _feature_rois(ngs, seed):
    shapes = [(5, 6, 7), (1, 1, 9), (2, 2, 2), (4, 7, 5), (6, 5, 6), (3, 8, 6), (1, 1, 1), (8, 8, 8)][:len(ngs)]
    imgs, masks = _rois(shapes, ngs, seed, fill=0.7)
    return shapes, imgs, masks


def _rows_by_count(dl, dm, ngs, **kw):
    """the table of scalar calls on the ROIs that share each count"""
    from pyradiomics_amd import engine
    table, status = {}, [None] * len(ngs)
    for ng in sorted(set(ngs)):
        idx = [b for b, g in enumerate(ngs) if g == ng]
        sub, st = engine.texture_features_batch([dl[b] for b in idx], [dm[b] for b in idx], None, ng, mcc=ng <= 64, **kw)
        for cls in sub:
            table.setdefault(cls, np.full((len(ngs), sub[cls].shape[1]), np.nan))[idx] = sub[cls]
        for k, b in enumerate(idx):
            status[b] = st[k]
    return table, status


@pytest.mark.parametrize("kw", [{}, {"weightingNorm": "euclidean", "spacing": (1.0, 2.0, 0.5)}, {"force2D": True, "force2Ddimension": 1}],
                         ids=["plain", "weighted", "force2d"])
def test_features_equal_the_scalar_calls_per_count(kw):
    from pyradiomics_amd import engine
    ngs = [64, 7, 1, 7, 33, 64, 64, 2]
    shapes, imgs, masks = _feature_rois(ngs, 41)
    dl, dm = _dev(imgs, masks)
    table, status = engine.texture_features_batch(dl, dm, None, ngs, **kw)
    assert engine.last_batch_route() == "batch"
    want, want_status = _rows_by_count(dl, dm, ngs, **kw)
    assert status == want_status == [1] * len(ngs)
    assert set(table) == set(want)
    for cls in table:
        assert table[cls].tobytes() == want[cls].tobytes(), cls
    assert np.isfinite(table["glcm"][0, 23])


def test_features_above_64_levels_take_the_single_calls():
    from pyradiomics_amd import cmatrices, engine
    ngs = [64, 7, 100, 7, 33, 65]
    shapes, imgs, masks = _feature_rois(ngs, 43)
    dl, dm = _dev(imgs, masks)
    table, status = engine.texture_features_batch(dl, dm, None, ngs, mcc_angles=True)
    assert engine.last_batch_route() == "mixed"
    want, want_status = _rows_by_count(dl, dm, ngs)
    assert status == want_status == [1] * len(ngs)
    for cls in want:
        assert table[cls].tobytes() == want[cls].tobytes(), cls
    mcc = table["glcm"][:, 23]
    assert np.isnan(mcc[[2, 5]]).all() and np.isfinite(mcc[[0, 1, 3, 4]]).all()
    assert np.isnan(table["glcm_mcc_angles"][2]).all() and np.isfinite(table["glcm_mcc_angles"][0]).any()
    # the host twin takes the vector too
    host = cmatrices.calculate_features_batch(imgs, masks, ngs)
    col, name = next((i, n) for i, n in enumerate(cmatrices.batch_feature_names("glrlm")) if n)
    assert np.array_equal(host["glrlm"][name], table["glrlm"][:, col], equal_nan=True)
    mats, st = cmatrices.calculate_matrices_batch(imgs, masks, ngs)
    assert cmatrices.last_batch_route() == "mixed" and st == [1] * len(ngs)
    assert [m.shape[0] for m in mats["ngtdm"]] == ngs
    zones, st = cmatrices.calculate_glszm_batch(imgs, masks, ngs)
    assert st == [1] * len(ngs) and [z.shape[0] for z in zones] == ngs


class _CountingLib:
    """the library handle with its calls counted by name"""
    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("prad_"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_roi_features_batch_with_a_bin_width_is_one_texture_call(monkeypatch):
    """integer-valued float32 boxes whose ranges give ten distinct counts under binWidth 25, among them 1, 64 and 90: every column
    equals the evaluation grouped by count that the scalar public calls give; the ROIs of at most 64 levels cost ONE matrix call"""
    from pyradiomics_amd import _lib, engine, firstorder
    rng = np.random.default_rng(51)
    counts = [1, 64, 90, 3, 8, 17, 40, 63, 8, 2, 33, 3, 1, 64]
    shapes = [(5, 6, 7), (6, 6, 6), (4, 7, 5), (6, 5, 6), (3, 8, 6), (1, 1, 12), (8, 8, 8), (2, 9, 4), (7, 3, 5), (2, 2, 2),
              (5, 5, 5), (3, 3, 9), (4, 4, 4), (9, 2, 6)]
    imgs, masks = [], []
    for n, s in zip(counts, shapes):
        img = rng.integers(0, 25 * n, size=s).astype(np.float32)          # edges 0, 25, ..., 25 n: n bins
        msk = rng.random(s) < 0.7
        img.flat[0], img.flat[1], msk.flat[0], msk.flat[1] = 0.0, 25.0 * n - 1.0, True, True
        imgs.append(img)
        masks.append(msk)
    masks.append(np.zeros((3, 3, 3), bool))          # an empty ROI: status 0, NaN rows, no part in the texture call
    imgs.append(np.ones((3, 3, 3), np.float32))
    I, M = _dev(imgs, masks)
    B = len(imgs)
    rows, verdict = engine.firstorder_batch(I, M)
    levels, Ng, _, bins = engine.bin_batch(I, M, stats=(rows, verdict), binWidth=25)
    assert Ng.tolist() == counts + [0]
    assert len(set(counts)) >= 8 and {1, 64}.issubset(counts) and max(counts) > 64

    proxy = _CountingLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    table, status = engine.roi_features_batch(I, M, binWidth=25, voxelVolume=0.5)
    monkeypatch.undo()
    assert engine.last_batch_route() == "mixed" and status == [1] * (B - 1) + [0]
    matrix_calls = {k: v for k, v in proxy.calls.items() if k.startswith("prad_calculate_batch")}
    assert matrix_calls == {"prad_calculate_batch_ng_dev": 1}, proxy.calls
    assert proxy.calls.get("prad_batch_glszm_ng_dev") == 1 and proxy.calls.get("prad_batch_features_ng_dev") == 1

    # the grouped evaluation: per distinct count the scalar texture call on bin_batch's levels of the ROIs that share it
    assert list(table) == list(engine.ROI_FEATURE_CLASSES)
    want_fo = firstorder.features_from_stats(rows, [c[1:] for c in bins], 0.5)
    want_fo[B - 1] = np.nan
    assert table["firstorder"].tobytes() == want_fo.tobytes()
    start = np.concatenate([[0], np.cumsum([i.size for i in imgs])])
    for ng in sorted(set(counts)):
        idx = [b for b, g in enumerate(counts) if g == ng]
        sub, st = engine.texture_features_batch([levels[start[b]:start[b + 1]].view(shapes[b]) for b in idx], [M[b] for b in idx], None,
                                                ng, mcc=ng <= 64)
        assert st == [1] * len(idx)
        for cls in sub:
            assert table[cls][idx].tobytes() == sub[cls].tobytes(), (ng, cls)
    for cls in table:
        assert np.isnan(table[cls][B - 1]).all()
    assert np.isnan(table["glcm"][2, 23]) and np.isfinite(table["glcm"][1, 23])

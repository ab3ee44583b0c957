"""Batched feature formulas (engine.batch_features_per_angle, engine.texture_features_batch,
cmatrices.calculate_features_batch, prad_batch_features_dev).  Three witnesses:

1. the single calls (glcm_features, glcm_mcc, zone_matrix_features, ngtdm_features) on every ROI's matrices: the per-angle rows
   and the empty flags must be equal BIT FOR BIT (np.array_equal, NaN positions equal), and the averaged table must equal
   cmatrices._angle_mean of those rows bit for bit;
2. tests/feature_reference.py (long double), because the single calls share the device functions of the batched kernel: bounds
   glcm_bounds / zone_bounds / ngtdm_bounds with the constants tests/test_gpu_segment_feature_limits.py derives (imported, not
   restated).  A derived feature (Correlation, Imc1, Imc2, Busyness) whose divisor is not COND times its own error bound has no
   first-order bound (that module asserts its inputs away from there; random lesions are not built to order): such a value is
   left to witness 1.  MCC: that module's bound 2 n TERM U (1 / (2 s2) + 1) for n occurring levels (it is an expression there,
   not a name); where s2^2 is below the eigenvalue error e = 2 n TERM U the square root is bounded by sqrt(2 e) instead
   (|sqrt(x + d) - sqrt(x)| <= sqrt(|d|));
3. the unchanged suite of the single kernels (test_gpu_segment_feature_limits.py, test_gpu_features.py, test_gpu_configs.py).
"""
import math

import numpy as np
import pytest

import feature_reference as fr
from test_gpu_batch_rois import RAGGED, _dev, _rois
from test_gpu_segment_feature_limits import (COND, TERM, U, c_glcm_entry, c_glcm_marginal, c_ngtdm, c_zone_entry,
                                             c_zone_marginal)

pytestmark = pytest.mark.gpu

CLASSES = ("glcm", "glrlm", "glszm", "gldm", "ngtdm")
WIDTH = {"glcm": 24, "glrlm": 16, "glszm": 16, "gldm": 16, "ngtdm": 5}


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _single(mats, zones, b, symmetric=True, mcc=True):
    """witness 1: the single calls on ROI b's matrices -> {class: (rows, empty)}"""
    from pyradiomics_amd import engine
    out = {}
    if "glcm" in mats:
        G = mats["glcm"][b]
        Na = G.shape[2]
        if Na:
            v, e = engine.glcm_features(G, symmetric)
            m = engine.glcm_mcc(G, symmetric) if mcc else np.full(Na, np.nan)
            out["glcm"] = (np.concatenate([v, m[:, None]], 1), e)
        else:
            out["glcm"] = (np.empty((0, 24)), np.zeros(0, dtype=bool))
    if "glrlm" in mats:
        R = mats["glrlm"][b]
        out["glrlm"] = (engine.zone_matrix_features(R, np.arange(1, R.shape[1] + 1)) if R.shape[2]
                        else (np.empty((0, 16)), np.zeros(0, dtype=bool)))
    if "gldm" in mats:
        D = mats["gldm"][b]
        out["gldm"] = engine.zone_matrix_features(D, np.arange(1, D.shape[1] + 1))
    if "ngtdm" in mats:
        N = mats["ngtdm"][b]
        out["ngtdm"] = (engine.ngtdm_features(N).reshape(1, 5), np.array([not (N[:, 0] > 0).any().item()]))
    if zones is not None:
        z = zones[b]
        P, jv = z if isinstance(z, tuple) else (z, np.arange(1, z.shape[1] + 1))
        if P.shape[1] == 0:          # no zone: the compact matrix has no column; the dense one is a column of zeros
            import torch
            P, jv = torch.zeros((P.shape[0], 1), dtype=torch.float64, device=P.device), np.ones(1)
        out["glszm"] = engine.zone_matrix_features(P, jv)
    return out


def _assert_rows(per, mats, zones, rois, symmetric=True, mcc=True, what=""):
    for b in rois:
        want = _single(mats, zones, b, symmetric, mcc)
        for f, (rows, empty) in want.items():
            got_rows, got_empty = per[f][b]
            assert _eq(got_rows, rows), (what, "ROI %d" % b, f, got_rows, rows)
            assert _eq(got_empty, np.asarray(empty, dtype=bool)), (what, "ROI %d" % b, f, "empty flags")
            assert np.isnan(got_rows[got_empty]).all() or f == "ngtdm"


def _assert_table(table, status, per, rois, what=""):
    from pyradiomics_amd import cmatrices
    for f, rows in table.items():
        assert rows.shape[1] == WIDTH[f] and rows.dtype == np.float64
        for b in rois:
            if not status[b]:
                assert np.isnan(rows[b]).all(), (what, b, f)
                continue
            vals, empty = per[f][b]
            want = vals[0] if f == "ngtdm" else cmatrices._angle_mean(vals, empty)
            assert _eq(rows[b], want), (what, "ROI %d" % b, f, rows[b], want)


def _run(imgs, masks, Ng, classes=CLASSES, distances=(1,), symmetric=True, mcc=True, compact=True):
    """matrices, per-angle rows and the table of one batch (the matrix calls run twice: once for the witnesses' inputs)"""
    from pyradiomics_amd import engine
    dl, dm = _dev(imgs, masks)
    fams = tuple(f for f in ("glcm", "glrlm", "gldm", "ngtdm") if f in classes)
    mats, st = engine.texture_matrices_batch(dl, dm, None, Ng, fams, distances) if fams else ({}, [1] * len(imgs))
    zones = engine.glszm_batch(dl, dm, None, Ng, compact=compact)[0] if "glszm" in classes else None
    per = engine.batch_features_per_angle(mats, Ng, zones, symmetric, mcc)
    table, status = engine.texture_features_batch(dl, dm, None, Ng, classes, distances, 0, symmetric, mcc)
    route = engine.last_batch_route()
    return {"mats": mats, "zones": zones, "per": per, "table": table, "status": status, "route": route, "dev": (dl, dm)}


def _check_batch(imgs, masks, Ng, rois=None, **kw):
    r = _run(imgs, masks, Ng, **kw)
    rois = range(len(imgs)) if rois is None else rois
    _assert_rows(r["per"], r["mats"], r["zones"], rois, kw.get("symmetric", True), kw.get("mcc", True))
    if kw.get("compact", True):      # (the table is built on the compact GLSZM: dense rows add the same terms in another order)
        _assert_table(r["table"], r["status"], r["per"], rois)
    return r


# ---- witness 2 -------------------------------------------------------------------------------------------------------------
def _independent(per, mats, zones, b, symmetric=True):
    if "glcm" in mats and mats["glcm"][b].shape[2]:
        C = mats["glcm"][b].cpu().numpy()
        Ng = C.shape[0]
        got, empty = per["glcm"][b]
        refs, mref = fr.glcm_reference(C, symmetric), fr.mcc_reference(C, symmetric)
        for a, ref in enumerate(refs):
            assert bool(empty[a]) == ref["empty"]
            if ref["empty"]:
                assert np.isnan(got[a]).all()
                continue
            B, cond = fr.glcm_bounds(ref, c_glcm_entry(Ng), c_glcm_marginal(Ng))
            single = np.count_nonzero(ref["p"]) == 1
            for k, n in enumerate(fr.GLCM_NAMES):
                want = float(ref["values"][n])
                if single and n in fr.GLCM_DERIVED:
                    assert got[a, k] == want == {"Correlation": 1, "Imc1": 0, "Imc2": 0}[n], (b, a, n)
                    continue
                if (n in cond and not cond[n] >= COND) or not B[n] == B[n]:
                    continue          # no first-order bound (module docstring): witness 1 has this value
                assert abs(got[a, k] - want) <= B[n], ("ROI %d angle %d" % (b, a), n, got[a, k], want, B[n])
            s2, nocc = mref[a]
            e = 2 * max(nocc, 1) * TERM * U
            bound = e * (1 / (2 * s2) + 1) if s2 * s2 > e else math.sqrt(2 * e)
            assert abs(got[a, 23] - s2) <= bound, ("ROI %d angle %d MCC" % (b, a), got[a, 23], s2, bound)
    zone_like = [(f, mats[f][b].cpu().numpy(), None) for f in ("glrlm", "gldm") if f in mats]
    if zones is not None:
        z = zones[b]
        P, jv = z if isinstance(z, tuple) else (z, None)
        if P.shape[1]:
            zone_like.append(("glszm", P.cpu().numpy(), jv))
    for f, P, jv in zone_like:
        P3 = P if P.ndim == 3 else P[:, :, None]
        Ni, Nj, Na = P3.shape
        jv = np.arange(1, Nj + 1) if jv is None else jv
        got, empty = per[f][b]
        for a in range(Na):
            ref = fr.zone_angle(P3[:, :, a], jv)
            assert bool(empty[a]) == ref["empty"]
            if ref["empty"]:
                assert np.isnan(got[a]).all()
                continue
            B = fr.zone_bounds(ref, c_zone_marginal(Ni, Nj), c_zone_entry(Ni, Nj))
            for k, n in enumerate(fr.ZONE_NAMES):
                want = float(ref["values"][n])
                assert abs(got[a, k] - want) <= B[n], ("ROI %d %s angle %d" % (b, f, a), n, got[a, k], want, B[n])
    if "ngtdm" in mats:
        N = mats["ngtdm"][b].cpu().numpy()
        got, empty = per["ngtdm"][b]
        ref = fr.ngtdm_reference(N)
        ngp = ref["parts"]["ngp"]
        assert bool(empty[0]) == (ngp == 0)
        if ngp == 0:          # ngtdm.py:148-150, 187, 219, 284: the values of the single kernel on an empty matrix
            assert _eq(got[0], np.array([1e6, 0.0, 0.0, np.nan, 0.0]))
        else:
            B, cond = fr.ngtdm_bounds(ref, c_ngtdm(ngp), c_ngtdm(ngp * ngp))
            for k, n in enumerate(fr.NGTDM_NAMES):
                if n == "Busyness" and not cond.get("absdiff", COND) >= COND:
                    continue
                want = float(ref["values"][n])
                assert abs(got[0, k] - want) <= B[n], ("ROI %d NGTDM" % b, n, got[0, k], want, B[n])


# ---- the ragged batch: computed once, shared -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    Ng = 16
    imgs, masks = _rois(RAGGED, Ng, seed=20260)
    masks[0][:] = True
    r = _run(imgs, masks, Ng)
    r.update(Ng=Ng, imgs=imgs, masks=masks)
    return r


def test_ragged_batch_equals_the_single_calls(ragged):
    """zero angles, one angle, 51 GLRLM columns, a box at PRAD_BATCH_MAX_VOX (above the GLSZM cap: "mixed"), unaligned offsets"""
    B = len(RAGGED)
    assert ragged["route"] == "mixed" and ragged["status"] == [1] * B
    assert ragged["per"]["glcm"][0][0].shape == (0, 24) and ragged["per"]["glrlm"][0][0].shape == (0, 16)
    assert ragged["per"]["glcm"][1][0].shape == (1, 24) and ragged["mats"]["glrlm"][6].shape[1] == 51
    _assert_rows(ragged["per"], ragged["mats"], ragged["zones"], range(B))
    _assert_table(ragged["table"], ragged["status"], ragged["per"], range(B))
    # no angle at all: the reference's mean over nothing
    assert np.isnan(ragged["table"]["glcm"][0]).all() and np.isnan(ragged["table"]["glrlm"][0]).all()


def test_ragged_batch_against_the_long_double_reference(ragged):
    for b in range(len(RAGGED)):
        _independent(ragged["per"], ragged["mats"], ragged["zones"], b)


def test_route_of_a_covered_batch():
    from pyradiomics_amd import _lib, engine
    imgs, masks = _rois([(5, 6, 7), (4, 4, 4)], 8, seed=3)
    r = _check_batch(imgs, masks, 8)
    assert r["route"] == "batch" and engine.last_batch_route() == "batch"
    assert _lib.last_path() == "batch" and _lib.last_variant() == "batch-features"
    for b in range(2):
        _independent(r["per"], r["mats"], r["zones"], b)


@pytest.mark.parametrize("Ng", [1, 64])
def test_level_extremes(Ng):
    imgs, masks = _rois([(5, 6, 7)] * 3, Ng, seed=40 + Ng)
    r = _check_batch(imgs, masks, Ng)
    assert r["route"] == "batch"
    for b in range(3):
        _independent(r["per"], r["mats"], r["zones"], b)


def test_mask_extremes():
    """an empty mask, a full mask and a single masked voxel in one batch: flags and NaN rows as the single calls"""
    imgs, masks = _rois([(5, 6, 7)] * 3, 8, seed=5)
    masks[0][:] = False
    masks[1][:] = True
    masks[2][:] = False
    masks[2][2, 3, 4] = True
    r = _check_batch(imgs, masks, 8)
    assert r["status"] == [1, 1, 1]
    for f in ("glcm", "glrlm", "gldm", "glszm"):
        assert r["per"][f][0][1].all() and np.isnan(r["table"][f][0]).all(), f
        assert not r["per"][f][1][1].any(), f
    assert r["per"]["glcm"][2][1].all() and not r["per"]["glszm"][2][1].any()      # one voxel: no pair, one zone
    assert r["per"]["ngtdm"][0][1].all() and not r["per"]["ngtdm"][2][1].any()
    for b in range(3):
        _independent(r["per"], r["mats"], r["zones"], b)


@pytest.mark.parametrize("compact", [True, False])
def test_glszm_shapes(compact):
    """one zone, no zone, several distinct sizes; compact and dense GLSZM input"""
    Ng = 6
    one = np.full((4, 5, 6), 3, dtype=np.int32)
    several = np.ones((4, 5, 6), dtype=np.int32)
    several[0, 0, :3] = 2          # sizes 3, 2, 1 and the rest
    several[2, 2, :2] = 4
    several[3, 4, 5] = 6
    imgs = [one, one.copy(), several]
    masks = [np.ones(one.shape, bool), np.zeros(one.shape, bool), np.ones(one.shape, bool)]
    r = _check_batch(imgs, masks, Ng, classes=("glszm",), compact=compact)
    assert r["route"] == "batch"
    rows = [r["per"]["glszm"][b] for b in range(3)]
    assert not rows[0][1][0] and rows[1][1][0] and not rows[2][1][0]
    assert np.isnan(rows[1][0]).all()
    for b in range(3):
        _independent(r["per"], {}, r["zones"], b)
    if compact:
        assert list(r["zones"][2][1]) == [1, 2, 3, 4 * 5 * 6 - 6] and list(r["zones"][0][1]) == [120] and len(r["zones"][1][1]) == 0


def test_asymmetric_glcm():
    imgs, masks = _rois([(5, 6, 7), (3, 9, 4)], 8, seed=6)
    r = _check_batch(imgs, masks, 8, classes=("glcm",), symmetric=False)
    sym = _run(imgs, masks, 8, classes=("glcm",))
    assert not _eq(r["table"]["glcm"], sym["table"]["glcm"])
    for b in range(2):
        _independent(r["per"], r["mats"], None, b, symmetric=False)


def test_without_mcc_the_last_column_is_nan():
    imgs, masks = _rois([(5, 6, 7)], 8, seed=7)
    r = _check_batch(imgs, masks, 8, classes=("glcm", "ngtdm"), mcc=False)
    assert np.isnan(r["per"]["glcm"][0][0][:, 23]).all() and not np.isnan(r["per"]["glcm"][0][0][:, :23]).all()


def test_two_distances():
    """distances (1, 2): the GLCM and GLRLM angle counts differ"""
    imgs, masks = _rois([(6, 6, 6)] * 2, 8, seed=8)
    r = _check_batch(imgs, masks, 8, distances=(1, 2))
    Na = r["mats"]["glcm"][0].shape[2]
    assert Na > 13 and r["mats"]["glrlm"][0].shape[2] == 13
    assert r["per"]["glcm"][1][0].shape == (Na, 24) and r["per"]["glrlm"][1][0].shape == (13, 16)
    _independent(r["per"], r["mats"], r["zones"], 1)


def test_large_batch():
    """600 ROIs of 4^3: more records than any other case, more ROIs than compute units; 42 of them are compared"""
    B = 600
    imgs, masks = _rois([(4, 4, 4)] * B, 8, seed=9)
    pick = sorted(set([0, B - 1]) | set(np.random.default_rng(10).choice(B, size=40, replace=False).tolist()))
    r = _check_batch(imgs, masks, 8, rois=pick)
    assert r["route"] == "batch" and r["status"] == [1] * B
    for f in CLASSES:
        assert r["table"][f].shape == (B, WIDTH[f])


def test_bad_level_in_the_middle():
    imgs, masks = _rois([(5, 6, 7), (4, 5, 6), (3, 9, 4)], 8, seed=11)
    masks[1][1, 1, 1] = True
    imgs[1][1, 1, 1] = 9
    r = _run(imgs, masks, 8)
    assert r["status"] == [1, 0, 1]
    clean = _run([imgs[0], imgs[2]], [masks[0], masks[2]], 8)
    for f in CLASSES:
        assert np.isnan(r["table"][f][1]).all(), f
        assert _eq(r["table"][f][[0, 2]], clean["table"][f]), f
        for b, c in ((0, 0), (2, 1)):
            assert _eq(r["per"][f][b][0], clean["per"][f][c][0]) and _eq(r["per"][f][b][1], clean["per"][f][c][1])


def test_declined_domain():
    """Ng = 65 declines: the single calls are looped.  The same data with 64 levels is comparable where the matrix of level 65
    only adds zero rows behind the others: the zone-like families (the order of their sums does not depend on Ni) and NGTDM
    (present levels only); a GLCM entry sum strides over Ng * Ng entries, so its order changes with Ng: single calls there"""
    from pyradiomics_amd import engine
    imgs, masks = _rois([(5, 6, 7), (4, 4, 4)], 64, seed=12)
    r = _check_batch(imgs, masks, 65)
    assert r["route"] == "looped" and engine.last_batch_route() == "looped"
    native = _run(imgs, masks, 64)
    assert native["route"] == "batch"
    for f in ("glrlm", "gldm", "glszm", "ngtdm"):
        assert _eq(r["table"][f], native["table"][f]), f


def test_determinism_and_streams(ragged):
    import torch
    from pyradiomics_amd import engine
    dl, dm = ragged["dev"]
    again, _ = engine.texture_features_batch(dl, dm, None, ragged["Ng"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other, _ = engine.texture_features_batch(dl, dm, None, ragged["Ng"])
    side.synchronize()
    for f in CLASSES:
        assert _eq(again[f], ragged["table"][f]) and _eq(other[f], ragged["table"][f]), f


def test_host_boundary(ragged):
    from pyradiomics_amd import cmatrices
    named = cmatrices.calculate_features_batch(ragged["imgs"], ragged["masks"], ragged["Ng"])
    assert set(named) == set(CLASSES)
    assert list(named["glcm"]) == cmatrices.VOXEL_GLCM_FEATURES + ["MCC"]
    assert list(named["glrlm"]) == cmatrices.VOXEL_GLRLM_FEATURES and list(named["glszm"]) == cmatrices.VOXEL_GLSZM_FEATURES
    assert list(named["gldm"]) == cmatrices.VOXEL_GLDM_FEATURES and list(named["ngtdm"]) == cmatrices.VOXEL_NGTDM_FEATURES
    for f in CLASSES:
        cols = [k for k, n in enumerate(cmatrices.batch_feature_names(f)) if n]
        got = np.stack([named[f][n] for n in named[f]], axis=1)
        assert _eq(got, ragged["table"][f][:, cols]), f

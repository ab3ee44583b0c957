"""force2D and weightingNorm on the batched small-ROI route (engine.texture_matrices_batch, glszm_batch, glszm_batch_zones,
texture_features_batch, roi_features_batch, their host-array twins in cmatrices; prad_calculate_batch_f2d_dev,
prad_batch_glszm_f2d_dev, prad_batch_merge_angles_dev).

Witnesses.
* Matrices and GLSZM: the single device calls with the same force2D arguments (pinned against the reference C by the existing
  suite), bit for bit; NGTDM as tests/test_gpu_batch_rois.py compares it.  A box that keeps no angle is refused by the single
  calls: its truth comes from the reference's cmatrices.c on an empty angle table (test_gpu_batch_rois._no_angle_truth through
  the oracle binding).  GLSZM also against the scipy restatement tests/glszm_reference.py, and against geometry alone.
* Merge: a host loop acc = acc + P[..., a] * w[a] over a ascending in float64 on the batched per-angle matrices, bit for bit
  (the launch adds rounded products in that order); the class's np.sum(P * w, axis) to a relative 2 (Na - 1) 2^-53 per entry:
  both add the SAME rounded products, non-negative, in two orders, each order is within (Na - 1) 2^-53 of the exact sum.
* Features with weightingNorm: bit for bit the single device feature calls on copies of the merged matrices; the long double
  restatement tests/feature_reference.py on the merged matrix with the chain constants of
  tests/test_gpu_segment_feature_limits.py; and the feature classes' host numpy route (RadiomicsGLCM / RadiomicsGLRLM with the
  same settings), whose own distance to the restatement is bounded with c_ref of tests/test_feature_reference.py.
  Two additions to the constants, both reasoned, none measured: (1) the merged matrices are not integers, so a marginal of the
  zone-like kernel is no longer exact: any summation of n non-negative terms is within (n - 1) 2^-53 of their sum, n <=
  max(Ni, Nj), which is added to c_zone_marginal; (2) the class merges with np.sum, so every entry it normalises differs from
  the launch's by a relative 2 (Na - 1) 2^-53 at most (above), and so does its total: 4 (Na - 1) is added to the class's
  constant.  A derived GLCM feature without a first-order bound (divisor below COND times its own bound) is left to the
  bit-for-bit witness, as in tests/test_gpu_batch_features.py."""
import ctypes as C
import logging

import numpy as np
import pytest

import feature_reference as fr
import glszm_reference as gr
from test_feature_reference import c_ref
from test_gpu_batch_features import _eq, _independent
from test_gpu_batch_rois import NGTDM_RTOL, _dev, _no_angle_truth
from test_gpu_segment_feature_limits import COND, U, c_glcm_entry, c_glcm_marginal, c_zone_entry, c_zone_marginal

pytestmark = pytest.mark.gpu

SIZES = [(5, 9, 17), (1, 12, 70), (7, 1, 33), (9, 66, 1), (3, 3, 3), (1, 1, 1), (5, 1, 1), (2, 2, 65)]
DISTANCES = [(1,), (1, 2), (2, 3)]
FAMILIES = ("glcm", "glrlm", "gldm", "ngtdm")
NORMS = ("euclidean", "manhattan", "infinity", "no_weighting")
SPACINGS = ((2.5, 0.7, 1.3), (0.9, 1.1, 3.0))
LOG = logging.getLogger("test_gpu_batch_planar")


def _rois(shapes, Ng, seed, fill=0.6):
    rng = np.random.default_rng(seed)
    return ([rng.integers(1, Ng + 1, size=s).astype(np.int32) for s in shapes], [rng.random(s) < fill for s in shapes])


def _ragged(Ng, seed):
    """the eight sizes, a (6,5,4) box with an empty mask and a (4,4,4) box with a masked level outside [1, Ng] between good ROIs"""
    shapes = SIZES[:4] + [(6, 5, 4)] + SIZES[4:6] + [(4, 4, 4)] + SIZES[6:]
    imgs, masks = _rois(shapes, Ng, seed)
    masks[4][:] = False
    imgs[7][1, 2, 3], masks[7][1, 2, 3] = Ng + 1, True
    masks[5][1, 1, 1] = masks[9][0, 0, 0] = True
    return shapes, imgs, masks, 7


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _single_matrices(checker, img, mask, dl, dm, Ng, dist, d, na, na1):
    """the single device calls with force2D (None: they raise IndexError); the reference C on an empty table for the families that
    keep no angle: na counts the angles of `dist` (GLCM, GLDM, NGTDM), na1 those of distance 1 (GLRLM) -- a 2 x 2 x 65 box with
    dimension 2 and distances (2, 3) keeps only the latter"""
    from pyradiomics_amd import engine
    try:
        out = _no_angle_truth(checker, img, mask, Ng, 0) if (na == 0 or na1 == 0) else {}
        if na:
            out.update(glcm=_host(engine.glcm(dl, dm, Ng, dist, True, d)[0]), gldm=_host(engine.gldm(dl, dm, Ng, 0, dist, True, d)),
                       ngtdm=_host(engine.ngtdm(dl, dm, Ng, dist, True, d)))
        if na1:
            out.update(glrlm=_host(engine.glcm_glrlm(dl, dm, Ng, max(img.shape), True, d, want_glcm=False)[1]))
        return out
    except IndexError:
        return None


def _assert_matrices(got, want, what):
    for f in ("glcm", "glrlm", "gldm"):
        assert got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f)
    a, b = got["ngtdm"], want["ngtdm"]
    assert a.shape == b.shape
    assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 2], b[:, 2]), (what, "NGTDM counts / levels")
    np.testing.assert_allclose(a[:, 1], b[:, 1], rtol=NGTDM_RTOL, atol=0, err_msg="%s NGTDM sums" % (what,))


# ---- matrices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", DISTANCES)
@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("Ng", [8, 64])
def test_forced_matrices_equal_the_single_calls(checker, Ng, d, dist):
    from pyradiomics_amd import _lib, cmatrices as cm, engine
    shapes, imgs, masks, bad = _ragged(Ng, 100 * Ng + 10 * d + len(dist) + dist[0])
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng, distances=dist, force2D=True, force2Ddimension=d)
    assert engine.last_batch_route() == "batch" and _lib.last_path() == "batch" and _lib.last_variant() == "batch-lds-f2d"
    assert status == [0 if b == bad else 1 for b in range(len(shapes))]
    Na = cm.batch_plan(shapes, Ng, distances=dist, force2D=True, force2Ddimension=d)[2]
    assert set(mats) == set(FAMILIES)
    for b, shape in enumerate(shapes):
        want = _single_matrices(checker, imgs[b], masks[b], dl[b], dm[b], Ng, list(dist), d, int(Na[0, b]), int(Na[1, b]))
        assert (want is None) == (b == bad)
        got = {f: _host(mats[f][b]) for f in FAMILIES}
        assert got["glcm"].shape == (Ng, Ng, Na[0, b]) and got["glrlm"].shape == (Ng, max(shape), Na[1, b])
        assert got["gldm"].shape == (Ng, 4 * Na[0, b] + 1)
        if want is None:          # the matrices of an empty mask
            assert not got["glcm"].any() and not got["glrlm"].any() and not got["gldm"].any() and not got["ngtdm"][:, :2].any()
            continue
        _assert_matrices(got, want, (b, shape, d, dist))
    assert not _host(mats["gldm"][4]).any()          # the empty mask
    if d == 0:
        b = shapes.index((5, 1, 1))
        assert Na[0, b] == 0 and _host(mats["gldm"][b]).sum() == masks[b].sum() and not _host(mats["ngtdm"][b])[:, 1].any()


def test_forced_matrices_looped_route_and_host_twin(checker):
    """Ng = 65 is outside the native domain: the single calls are looped with the same settings, a box without angles included;
    the host-array twin returns what the device call returns on both routes"""
    from pyradiomics_amd import cmatrices as cm, engine
    d, dist = 0, (1, 2)
    for Ng, route in ((65, "looped"), (8, "batch")):
        shapes, imgs, masks, bad = _ragged(Ng, 7)
        dl, dm = _dev(imgs, masks)
        mats, status = engine.texture_matrices_batch(dl, dm, None, Ng, distances=dist, force2D=True, force2Ddimension=d)
        assert engine.last_batch_route() == route
        Na = cm.batch_plan(shapes, Ng, distances=dist, force2D=True, force2Ddimension=d)[2]
        host, hstatus = cm.calculate_matrices_batch(imgs, masks, Ng, distances=dist, force2D=True, force2Ddimension=d)
        assert cm.last_batch_route() == route and hstatus == status and status[bad] == 0
        for b, shape in enumerate(shapes):
            got = {f: _host(mats[f][b]) for f in FAMILIES}
            for f in FAMILIES:
                assert isinstance(host[f][b], np.ndarray) and np.array_equal(host[f][b], got[f]), (Ng, b, f)
            want = _single_matrices(checker, imgs[b], masks[b], dl[b], dm[b], Ng, list(dist), d, int(Na[0, b]), int(Na[1, b]))
            if want is not None:
                _assert_matrices(got, want, (Ng, b, shape))


# ---- GLSZM ---------------------------------------------------------------------------------------------------------------------
def _zones_of(levels, masks, Ng, **kw):
    from pyradiomics_amd import engine
    dl, dm = _dev(levels, masks)
    zones, summary, status = engine.glszm_batch_zones(dl, dm, None, Ng, **kw)
    return [_host(z) for z in zones], summary, status


def _assert_glszm(imgs, masks, Ng, d, route="batch", skip=()):
    """zone lists (pairs and order), summary, dense and compact matrices of a batch against the restatement and the single calls"""
    from pyradiomics_amd import _lib, cmatrices as cm, engine
    dl, dm = _dev(imgs, masks)
    kw = dict(force2D=True, force2Ddimension=d)
    dense, st_d = engine.glszm_batch(dl, dm, None, Ng, compact=False, **kw)
    assert engine.last_batch_route() == route
    comp, st_c = engine.glszm_batch(dl, dm, None, Ng, compact=True, **kw)
    assert engine.last_batch_route() == route and st_d == st_c
    zones = None
    if route == "batch":
        assert _lib.last_path() == "batch"
        zones, summary, st_z = _zones_of(imgs, masks, Ng, **kw)
        assert _lib.last_variant() == "batch-glszm-lds-f2d%d" % d and list(st_z) == st_d
    one = np.ones(1, dtype=np.intc)
    for b, (img, msk) in enumerate(zip(imgs, masks)):
        if b in skip:
            assert st_d[b] == 0
            continue
        assert st_d[b] == 1
        z = gr.zones(img, msk, True, d)
        if zones is not None:
            assert np.array_equal(zones[b], z[:, :2]), (b, "zone list: pairs and order")
            assert summary[b].tolist() == [len(z), int(z[:, 1].max()) if len(z) else 0, len(np.unique(z[:, 1]))]
        assert np.array_equal(_host(dense[b]), gr.matrix(z, Ng)[0]), (b, "dense")
        P, sizes = gr.compact(z, Ng)
        assert np.array_equal(_host(comp[b][0]), P) and np.array_equal(comp[b][1], sizes), (b, "compact")
        size = np.array(img.shape, dtype=np.intc)
        ip = C.POINTER(C.c_int)
        if _lib.load().prad_get_angle_count(size.ctypes.data_as(ip), one.ctypes.data_as(ip), 3, 1, 1, d) == 0:
            continue          # the single call refuses a box without neighbours
        Ns = max(1, int(msk.sum()))
        assert np.array_equal(_host(dense[b]), _host(engine.glszm(dl[b], dm[b], Ng, Ns, True, d))), (b, "single dense")
        sP, ss = engine.glszm_compact(dl[b], dm[b], Ng, Ns, True, d)
        assert np.array_equal(_host(comp[b][0]), _host(sP)) and np.array_equal(comp[b][1], ss), (b, "single compact")
    # the host-array twin
    hd, hst = cm.calculate_glszm_batch(imgs, masks, Ng, compact=False, **kw)
    assert hst == st_d and all(np.array_equal(a, _host(b)) for a, b in zip(hd, dense))


@pytest.mark.parametrize("d", [0, 1, 2])
def test_forced_glszm_ragged_batch(d):
    shapes, imgs, masks, bad = _ragged(8, 40 + d)
    _assert_glszm(imgs, masks, 8, d, skip=(bad,))


def test_forced_glszm_topologies_follow_from_geometry():
    Ng = 3
    const = np.full((4, 5, 6), 2, dtype=np.int32)
    space = np.full((5, 5, 5), 1, dtype=np.int32)
    plane = space.copy()
    for k in range(5):
        space[k, k, k] = 3
        plane[0, k, k] = 3
    imgs = [const, space, plane]
    masks = [np.ones(i.shape, dtype=bool) for i in imgs]

    def sizes_of(zones, level):
        return sorted(int(s) for g, s in zones if g == level)
    zones, _, status = _zones_of(imgs, masks, Ng)          # unforced
    assert list(status) == [1, 1, 1]
    assert zones[0].tolist() == [[2, 120]] and sizes_of(zones[1], 3) == [5] and sizes_of(zones[2], 3) == [5]
    for d, n, size in ((0, 4, 30), (1, 5, 24), (2, 6, 20)):
        zones, summary, _ = _zones_of(imgs, masks, Ng, force2D=True, force2Ddimension=d)
        assert zones[0].tolist() == [[2, size]] * n and summary[0].tolist() == [n, size, 1]
        assert sizes_of(zones[1], 3) == [1] * 5, "the space diagonal leaves every plane"
        assert sizes_of(zones[2], 3) == ([5] if d == 0 else [1] * 5), "the plane diagonal (0, k, k) lies in the plane across z"
        _assert_glszm(imgs, masks, Ng, d)


def test_forced_glszm_boxes_of_extent_one_along_and_across_the_forced_dimension():
    imgs, masks = _rois([(1, 9, 17), (9, 1, 17)], 4, seed=61, fill=0.85)
    _assert_glszm(imgs, masks, 4, 0)
    # (9, 1, 17) with dimension 0: only the neighbours along x are left -- zones are runs
    z = _zones_of(imgs, masks, 4, force2D=True, force2Ddimension=0)[0][1]
    assert z[:, 1].max() <= 17


@pytest.mark.parametrize("d", [0, 1, 2])
def test_forced_glszm_box_at_the_cap(d):
    from pyradiomics_amd import engine
    assert 37 ** 3 <= engine.batch_glszm_max_vox() < 38 ** 3
    imgs, masks = _rois([(37, 37, 37)], 64, seed=70 + d, fill=0.9)
    _assert_glszm(imgs, masks, 64, d)


def test_forced_glszm_mixed_route():
    """one box above batch_glszm_max_vox() goes through the single call with the same forced dimension"""
    imgs, masks = _rois([(4, 5, 6), (38, 38, 38), (5, 1, 1), (3, 7, 2)], 5, seed=81, fill=0.8)
    _assert_glszm(imgs, masks, 5, 0, route="mixed")
    _assert_glszm(imgs, masks, 5, 2, route="mixed")


# ---- the weighted angle merge --------------------------------------------------------------------------------------------------
MERGE_CASES = {          # name -> (shapes, distances, force2D, dimension, angle counts expected); one status-0 ROI in the middle
    "3d": ([(1, 1, 1), (1, 1, 5), (4, 4, 4), (1, 4, 5), (4, 5, 6)], (1,), False, 0, [0, 1, 13, 4, 13]),
    "3d-two-distances": ([(1, 1, 1), (5, 5, 5), (2, 2, 2), (1, 1, 5)], (1, 2), False, 0, [0, 62, 13, 2]),
    "forced-two-distances": ([(5, 6, 7), (1, 1, 1), (4, 4, 4), (6, 1, 1), (4, 5, 5)], (1, 2), True, 0, [12, 0, 12, 0, 12]),
}
assert {0, 1, 4, 12, 13, 62} <= {n for c in MERGE_CASES.values() for n in c[4]}


@pytest.mark.parametrize("Ng", [1, 8, 64])
@pytest.mark.parametrize("case", sorted(MERGE_CASES))
def test_merge_equals_the_host_loop_bit_for_bit(case, Ng):
    from pyradiomics_amd import _lib, engine
    from pyradiomics_amd.glcm import _weights
    shapes, dist, f2, d, counts = MERGE_CASES[case]
    imgs, masks = _rois(shapes, Ng, seed=len(case) + Ng, fill=0.8)
    bad = 2
    imgs[bad].flat[5], masks[bad].flat[5] = Ng + 1, True
    dl, dm = _dev(imgs, masks)
    spacing = np.array([SPACINGS[b % 2] for b in range(len(shapes))])
    for sym in (True, False):
        for norm in NORMS:
            mats, status = engine.texture_matrices_batch(dl, dm, None, Ng, ("glcm", "glrlm"), dist, 0, f2, d, norm, spacing, sym)
            assert engine.last_batch_route() == "batch" and _lib.last_variant() == "batch-merge"
            assert status == [0 if b == bad else 1 for b in range(len(shapes))]
            assert [m.shape[2] for m in mats["glcm"]] == counts
            for b, shape in enumerate(shapes):
                G, R = _host(mats["glcm"][b]), _host(mats["glrlm"][b])
                Gw, Rw = _host(mats["glcm_w"][b]), _host(mats["glrlm_w"][b])
                assert Gw.shape == (Ng, Ng, 1) and Rw.shape == (Ng, max(shape), 1)
                if b == bad or counts[b] == 0:
                    assert not Gw.any() and not Rw.any(), (case, b)
                    continue
                wg = _weights(engine.pair_angles(shape, dist, f2, d), spacing[b], norm, "glcm", LOG)
                wr = _weights(engine.pair_angles(shape, (1,), f2, d), spacing[b], norm, "glrlm", LOG)
                assert len(wg) == G.shape[2] and len(wr) == R.shape[2]
                if norm != "no_weighting" and len(wg) > 1:
                    assert len(set(wg.tolist())) > 1
                S = G + G.transpose(1, 0, 2) if sym else G
                for P, w, got, what in ((S, wg, Gw, "glcm"), (R, wr, Rw, "glrlm")):
                    acc = np.zeros(P.shape[:2])
                    for a in range(P.shape[2]):
                        acc = acc + P[..., a] * w[a]
                    assert np.array_equal(got[..., 0], acc), (case, Ng, sym, norm, b, what)
                    cls = np.sum(P * w[None, None, :], 2)          # glcm.py / glrlm.py
                    assert (np.abs(got[..., 0] - cls) <= 2 * (len(w) - 1) * U * np.maximum(got[..., 0], cls)).all(), (case, b, what)


def test_merge_looped_route_gives_the_same_bits():
    """65 levels: the single calls are looped and merged on the host with the launch's arithmetic; the same data at 64 levels runs
    natively -- level 65 only adds zero rows and columns"""
    from pyradiomics_amd import engine
    shapes = [(4, 5, 6), (1, 1, 1), (3, 7, 5)]
    imgs, masks = _rois(shapes, 64, seed=5, fill=0.8)
    dl, dm = _dev(imgs, masks)
    args = (("glcm", "glrlm"), (1,), 0, True, 1, "euclidean", SPACINGS[0], True)
    looped, _ = engine.texture_matrices_batch(dl, dm, None, 65, *args)
    assert engine.last_batch_route() == "looped"
    native, _ = engine.texture_matrices_batch(dl, dm, None, 64, *args)
    assert engine.last_batch_route() == "batch"
    for b in range(len(shapes)):
        assert np.array_equal(_host(looped["glcm_w"][b])[:64, :64], _host(native["glcm_w"][b]))
        assert np.array_equal(_host(looped["glrlm_w"][b])[:64], _host(native["glrlm_w"][b]))
        assert not _host(looped["glcm_w"][b])[64].any() and not _host(looped["glcm_w"][b])[:, 64].any()


def test_unknown_weighting_norm_raises():
    from pyradiomics_amd import engine
    imgs, masks = _rois([(3, 3, 3)], 4, seed=1)
    dl, dm = _dev(imgs, masks)
    for call in (engine.texture_matrices_batch, engine.texture_features_batch, engine.glszm_batch, engine.glszm_batch_zones):
        with pytest.raises(ValueError):
            call(dl, dm, None, 4, weightingNorm="euclid")
    with pytest.raises(ValueError):
        engine.texture_features_batch(dl, dm, None, 4, force2D=True, force2Ddimension=3)


# ---- features ------------------------------------------------------------------------------------------------------------------
FEATURE_SHAPES = [(4, 9, 11), (1, 1, 1), (6, 5, 7), (5, 1, 1), (3, 12, 4)]


@pytest.fixture(scope="module")
def weighted():
    """one batch, forced dimension 0, euclidean weights, two spacings: matrices, table and per-ROI single-call rows, computed once"""
    from pyradiomics_amd import engine
    Ng, d, norm = 8, 0, "euclidean"
    imgs, masks = _rois(FEATURE_SHAPES, Ng, seed=2026, fill=0.75)
    for i, m in zip(imgs, masks):          # level 1 under the mask at one corner, the opposite corner masked: the classes see the
        i.flat[0], m.flat[0], m.flat[-1] = 1, True, True          # same box and the same levels
    dl, dm = _dev(imgs, masks)
    spacing = np.array([SPACINGS[b % 2] for b in range(len(imgs))])
    kw = dict(force2D=True, force2Ddimension=d, weightingNorm=norm, spacing=spacing)
    mats, _ = engine.texture_matrices_batch(dl, dm, None, Ng, **kw)
    table, status = engine.texture_features_batch(dl, dm, None, Ng, mcc_angles=True, **kw)
    route = engine.last_batch_route()
    return dict(Ng=Ng, d=d, norm=norm, imgs=imgs, masks=masks, dev=(dl, dm), spacing=spacing, kw=kw, mats=mats, table=table,
                status=status, route=route)


def test_weighted_rows_equal_the_single_calls_on_copies_of_the_merged_matrices(weighted):
    from pyradiomics_amd import cmatrices as cm, engine
    w = weighted
    assert w["route"] == "batch" and w["status"] == [1] * len(FEATURE_SHAPES)
    copies = {f: [w["mats"][f + "_w"][b].clone() for b in range(len(FEATURE_SHAPES))] for f in ("glcm", "glrlm")}
    per = engine.batch_features_per_angle(copies, w["Ng"], None, False, True)          # separate tensors: the single calls
    for f, width in (("glcm", 24), ("glrlm", 16)):
        assert w["table"][f].shape == (len(FEATURE_SHAPES), width)
        for b in range(len(FEATURE_SHAPES)):
            vals, empty = per[f][b]
            assert vals.shape == (1, width)
            assert _eq(w["table"][f][b], cm._angle_mean(vals, empty)), (f, b)
    for b, shape in enumerate(FEATURE_SHAPES):
        ang = w["table"]["glcm_mcc_angles"][b]
        assert ang.shape == (1,) and _eq(ang, per["glcm"][b][0][:, 23])
        if shape in ((1, 1, 1), (5, 1, 1)):          # no angle: an all-zero merged matrix, the mean over nothing
            assert np.isnan(w["table"]["glcm"][b]).all() and np.isnan(w["table"]["glrlm"][b]).all()
        else:
            assert not np.isnan(w["table"]["glcm"][b][:23]).any() and not np.isnan(w["table"]["glrlm"][b]).any()
    # GLDM, NGTDM and GLSZM ignore the weights, as the classes do
    plain, _ = engine.texture_features_batch(*w["dev"], None, w["Ng"], force2D=True, force2Ddimension=w["d"])
    for f in ("gldm", "ngtdm", "glszm"):
        assert _eq(w["table"][f], plain[f]), f
    assert not _eq(w["table"]["glcm"], plain["glcm"])


def test_weighted_rows_against_the_long_double_reference(weighted):
    """witness 2 of tests/test_gpu_batch_features.py on the merged matrices; the zone-like marginal constant carries the
    summation of non-integer entries (module docstring)"""
    w = weighted
    merged = {"glcm": w["mats"]["glcm_w"]}
    per = {"glcm": [(w["table"]["glcm"][b][None, :], np.isnan(w["table"]["glcm"][b][:1])) for b in range(len(FEATURE_SHAPES))]}
    for b in range(len(FEATURE_SHAPES)):
        _independent(per, merged, None, b, symmetric=False)
        R = _host(w["mats"]["glrlm_w"][b])[:, :, 0]
        ref = fr.zone_angle(R, np.arange(1, R.shape[1] + 1))
        got = w["table"]["glrlm"][b]
        if ref["empty"]:
            assert np.isnan(got).all()
            continue
        Ni, Nj = R.shape
        B = fr.zone_bounds(ref, c_zone_marginal(Ni, Nj) + max(Ni, Nj), c_zone_entry(Ni, Nj))
        for k, n in enumerate(fr.ZONE_NAMES):
            assert abs(got[k] - float(ref["values"][n])) <= B[n], (b, n, got[k], ref["values"][n], B[n])


@pytest.mark.parametrize("sym", [True, False])
def test_weighted_rows_against_the_feature_classes(weighted, sym):
    from pyradiomics_amd import backend, cmatrices, engine
    from pyradiomics_amd.glcm import RadiomicsGLCM
    from pyradiomics_amd.glrlm import RadiomicsGLRLM
    from pyradiomics_amd.image import Image
    w = weighted
    Ng = w["Ng"]
    kw = dict(w["kw"])
    mats, _ = engine.texture_matrices_batch(*w["dev"], None, Ng, ("glcm", "glrlm"), symmetricalGLCM=sym, **kw)
    table, _ = engine.texture_features_batch(*w["dev"], None, Ng, ("glcm", "glrlm"), symmetricalGLCM=sym, **kw)
    backend.set(cmatrices)
    try:
        for b, shape in enumerate(FEATURE_SHAPES):
            if shape in ((1, 1, 1), (5, 1, 1)):
                continue          # the classes refuse a box without angles
            sp = tuple(float(s) for s in w["spacing"][b][::-1])          # Image takes (x, y, z)
            image = Image(w["imgs"][b].astype(np.float64) - 0.5, spacing=sp)          # binWidth 1 from 0.5: level = value + 0.5
            mask = Image(w["masks"][b].astype(np.int32), spacing=sp)
            settings = dict(binWidth=1, distances=[1], force2D=True, force2Ddimension=w["d"], weightingNorm=w["norm"],
                            symmetricalGLCM=sym)
            Na = len(engine.pair_angles(shape, (1,), True, w["d"]))
            extra = 4 * (Na - 1)
            # GLCM
            fc = RadiomicsGLCM(image, mask, **settings)
            for n in fr.GLCM_NAMES:
                fc.enableFeatureByName(n)
            vals = fc.execute()
            ref = fr.glcm_angle(_host(mats["glcm_w"][b])[:, :, 0], False)
            Bd, cond = fr.glcm_bounds(ref, c_glcm_entry(Ng), c_glcm_marginal(Ng))
            Bh, _ = fr.glcm_bounds(ref, c_ref(Ng) + extra, c_ref(Ng) + extra)
            for k, n in enumerate(fr.GLCM_NAMES):
                if (n in cond and not cond[n] >= COND) or not Bd[n] == Bd[n] or not Bh[n] == Bh[n]:
                    continue
                assert abs(table["glcm"][b, k] - float(vals[n])) <= Bd[n] + Bh[n], (b, n, table["glcm"][b, k], vals[n], Bd[n], Bh[n])
            # GLRLM
            fc = RadiomicsGLRLM(image, mask, **settings)
            for n in fr.ZONE_CLASS_NAMES["glrlm"]:
                fc.enableFeatureByName(n)
            vals = fc.execute()
            R = _host(mats["glrlm_w"][b])[:, :, 0]
            Ni, Nj = R.shape
            ref = fr.zone_angle(R, np.arange(1, Nj + 1))
            Bd = fr.zone_bounds(ref, c_zone_marginal(Ni, Nj) + max(Ni, Nj), c_zone_entry(Ni, Nj))
            Bh = fr.zone_bounds(ref, c_ref(max(Ni, Nj)) + extra, c_ref(max(Ni, Nj)) + extra)
            for k, (n, cn) in enumerate(zip(fr.ZONE_NAMES, fr.ZONE_CLASS_NAMES["glrlm"])):
                assert abs(table["glrlm"][b, k] - float(vals[cn])) <= Bd[n] + Bh[n], (b, cn, table["glrlm"][b, k], vals[cn], Bd[n], Bh[n])
    finally:
        backend.set(None)


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_roi_features_from_raw_boxes(dtype):
    """raw boxes -> roi_features_batch with force2D and euclidean weights equals texture_features_batch on its own levels; the
    first-order columns do not depend on the new settings"""
    import torch
    from pyradiomics_amd import cmatrices as cm, engine
    shapes = [(4, 9, 11), (6, 5, 7), (1, 8, 9), (3, 12, 4)]
    rng = np.random.default_rng(17)
    raws = [rng.uniform(0, 200, size=s) for s in shapes]
    masks = [rng.random(s) < 0.8 for s in shapes]
    for r, m in zip(raws, masks):          # binWidth 25 from 0 to 199: eight levels in every ROI
        r.flat[0], r.flat[-1], m.flat[0], m.flat[-1] = 0, 199, True, True
    raws = [r.astype(dtype) for r in raws]
    di = [torch.from_numpy(r).to("cuda:0") for r in raws]
    dm = [torch.from_numpy(m).to("cuda:0") for m in masks]
    spacing = np.array([SPACINGS[b % 2] for b in range(len(shapes))])
    kw = dict(force2D=True, force2Ddimension=0, weightingNorm="euclidean", spacing=spacing)
    table, status = engine.roi_features_batch(di, dm, binWidth=25, **kw)
    assert engine.last_batch_route() == "batch" and status == [1] * len(shapes)
    levels, Ng, _, _ = engine.bin_batch(di, dm, binWidth=25)
    assert Ng.tolist() == [8] * len(shapes)
    flat_m = torch.cat([m.reshape(-1) for m in dm])
    want, _ = engine.texture_features_batch(levels, flat_m, shapes, 8, **kw)
    for f in ("glcm", "glrlm", "glszm", "gldm", "ngtdm"):
        assert _eq(table[f], want[f]), f
    plain, _ = engine.roi_features_batch(di, dm, binWidth=25)
    assert _eq(table["firstorder"], plain["firstorder"]) and not _eq(table["glcm"], plain["glcm"])
    # the host-array twins
    named = cm.calculate_roi_features_batch(raws, masks, binWidth=25, **kw)
    for f in ("glcm", "glrlm"):
        cols = [k for k, n in enumerate(cm.batch_feature_names(f)) if n]
        assert _eq(np.stack([named[f][n] for n in named[f]], axis=1), table[f][:, cols]), f
    lv = [_host(engine.bin_batch([i], [m], binWidth=25)[0]).reshape(s) for i, m, s in zip(di, dm, shapes)]
    named = cm.calculate_features_batch(lv, masks, 8, **kw)
    for f in ("glcm", "glrlm", "gldm"):
        cols = [k for k, n in enumerate(cm.batch_feature_names(f)) if n]
        assert _eq(np.stack([named[f][n] for n in named[f]], axis=1), want[f][:, cols]), f


# ---- the defaults are the old entry points ----------------------------------------------------------------------------------------
def test_defaults_reproduce_the_old_entry_points():
    import torch
    from pyradiomics_amd import _lib, engine
    lib = _lib.load()
    Ng = 8
    shapes, imgs, masks, bad = _ragged(Ng, 3)
    dl, dm = _dev(imgs, masks)
    B = len(shapes)
    sizes = np.ascontiguousarray(np.array(shapes, dtype=np.intc))
    nvox = sizes.astype(np.int64).prod(1)
    off = np.concatenate([[0], np.cumsum(nvox)[:-1]]).astype(np.int64)
    flat_l, flat_m = torch.cat([t.reshape(-1) for t in dl]), torch.cat([t.reshape(-1) for t in dm]).view(torch.uint8)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    vp = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dist = np.array([1], dtype=np.intc)
    # prad_batch_plan + prad_calculate_batch_dev
    poff, Na = np.zeros((4, B + 1), dtype=np.int64), np.zeros((2, B), dtype=np.intc)
    assert lib.prad_batch_plan(sizes.ctypes.data_as(ip), B, Ng, 15, dist.ctypes.data_as(ip), 1, poff.ctypes.data_as(lp),
                               Na.ctypes.data_as(ip)) == _lib.PRAD_OK
    old = [torch.empty(int(poff[f, B]), dtype=torch.float64, device="cuda:0") for f in range(4)]
    st = torch.empty(B, dtype=torch.int32, device="cuda:0")
    rc = lib.prad_calculate_batch_dev(vp(flat_l), vp(flat_m), sizes.ctypes.data_as(ip), off.ctypes.data_as(lp), B, Ng, 15,
                                      dist.ctypes.data_as(ip), 1, 0, *[vp(o) for o in old], vp(st), stream)
    assert rc == _lib.PRAD_OK and _lib.last_variant() == "batch-lds"
    flat, status = engine.texture_matrices_batch_flat(flat_l, flat_m, sizes, Ng)
    assert _lib.last_variant() == "batch-lds" and status == st.tolist() and set(flat) == set(FAMILIES)
    for f, o in zip(FAMILIES, old):
        assert torch.equal(flat[f], o), f
    mats, status2 = engine.texture_matrices_batch(dl, dm, None, Ng)
    explicit, _ = engine.texture_matrices_batch(dl, dm, None, Ng, force2D=False, force2Ddimension=2, weightingNorm=None,
                                                spacing=SPACINGS[0])
    assert status2 == status and set(mats) == set(FAMILIES) == set(explicit)
    for k, f in enumerate(FAMILIES):
        assert torch.equal(torch.cat([m.reshape(-1) for m in mats[f]]), old[k])
        assert torch.equal(torch.cat([m.reshape(-1) for m in explicit[f]]), old[k])
    # prad_batch_glszm_dev
    zones_old = torch.zeros(2 * flat_l.numel(), dtype=torch.int32, device="cuda:0")
    meta = torch.empty(4 * B, dtype=torch.int32, device="cuda:0")
    rc = lib.prad_batch_glszm_dev(vp(flat_l), vp(flat_m), sizes.ctypes.data_as(ip), off.ctypes.data_as(lp), B, Ng, vp(zones_old),
                                  vp(meta), C.c_void_p(meta.data_ptr() + 12 * B), stream)
    assert rc == _lib.PRAD_OK and _lib.last_variant() == "batch-glszm-lds"
    summary_old = meta.cpu().numpy()[:3 * B].reshape(B, 3)
    zones, summary, zst = engine.glszm_batch_zones(dl, dm, None, Ng)
    assert _lib.last_variant() == "batch-glszm-lds" and np.array_equal(summary, summary_old)
    assert np.array_equal(zst, meta.cpu().numpy()[3 * B:])
    for b in range(B):
        n = int(summary[b, 0])
        assert torch.equal(zones[b].reshape(-1), zones_old[2 * int(off[b]):2 * int(off[b]) + 2 * n])
    # the feature layers: defaults equal the explicit "off" settings, and the unweighted table of the parent's signature
    t0, s0 = engine.texture_features_batch(dl, dm, None, Ng)
    t1, s1 = engine.texture_features_batch(dl, dm, None, Ng, ("glcm", "glrlm", "glszm", "gldm", "ngtdm"), (1,), 0, True, True, False,
                                           False, 0, None, (1.0, 1.0, 1.0))
    assert s0 == s1 and all(_eq(t0[f], t1[f]) for f in t0)
    for res in (engine.glszm_batch(dl, dm, None, Ng), engine.glszm_batch(dl, dm, None, Ng, True, False, 1, None)):
        for b in range(B):
            if b != bad:
                z = gr.zones(imgs[b], masks[b])
                P, sz = gr.compact(z, Ng)
                assert np.array_equal(_host(res[0][b][0]), P) and np.array_equal(res[0][b][1], sz)

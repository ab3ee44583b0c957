"""GPU: the batched front end -- engine.firstorder_batch, engine.bin_batch, engine.roi_features_batch and the host-list calls of
cmatrices (prad_batch_firstorder_dev, prad_batch_digitize_dev; csrc/kernels_batch_firstorder.h) -- at the smallest shapes at which
its two kernels can go wrong, with two witnesses for every ROI of every batch.

Witness 1, the precise reference: all 15 fields of every ROI against firstorder_reference.segment_reference (long double) with
firstorder_reference.compare under seg_bounds(ref, K, K).  Np, Minimum, Maximum, the percentiles and Median must be equal (the
sign of a zero included); rMAD is NaN exactly where the reference's is; a summed field obeys |got - ref| <= K 2^-53 abs_sum (+
the terms of the mean's own rounding, see firstorder_reference).  K is the longest chain of float64 additions a term passes
through in batch_firstorder_kernel: the workgroup of a ROI with m voxels has 256 threads, thread t adds the elements t, t + 256,
... of the SORTED array in index order (ceil(m / 256) additions), then fo_block_sum: 6 __shfl_xor steps and the 3 additions of
sh[0] + sh[1] + sh[2] + sh[3]:
    K = ceil(m / 256) + 6 + 3, never below 11 (the rule of tests/test_gpu_firstorder_limits.py; its helpers are used here).
A ROI the launch hands to the single call (verdict 8) is bounded by that call's geometry, firstorder_reference.k_reduction.

Witness 2, the single calls: the equal fields are also bit-equal to engine.firstorder_stats of the same ROI (only where a ROI
holds both -0.0 and +0.0 is the sign of a zero left open, as in firstorder_reference.compare); bin_batch's levels, Ng, edges and
counts are array_equal to engine.bin_image(with_counts=True); roi_features_batch's texture columns are bit-equal to
texture_features_batch on those levels and its first-order columns to features_from_stats of firstorder_batch's rows, and lie
within firstorder_reference.derived_bounds of the reference.

Measured worst error / bound per field over all cases of this module on an MI355X (every comparison records its ratio;
test_zz_report prints this table and fails on any ratio above 1):
    route                    Energy   Mean     MAD      rMAD     m2       m3       m4
    batch-firstorder         0.182    0.101    0.077    0.0869   0.0808   0.0923   0.0853
    batch-firstorder-single  0.00919  0.00633  0.0129   0.0181   0        0.00772  0.00706      (the capacity + 1 ROIs)
    batch-firstorder-class   Energy 0   TotalEnergy 0   Mean 0   MeanAbsoluteDeviation 0.0362   RobustMeanAbsoluteDeviation 0.0375
                             RootMeanSquared 0   StandardDeviation 0   Variance 0.0402   Skewness 0.0499   Kurtosis 0.0365
The class rows come from int16 ROIs of a few hundred voxels, whose sums of x and (x + c)^2 are exact in float64.

Notes.  With binWidth the edges of a constant ROI are [0, 25, 50] for the value 7 (anchored at 0), not a single-bin pair: the pair
[v - 0.5, v + 0.5] of getBinEdges belongs to an edge list of length 1, which np.arange does not produce for these arguments; the
constant ROI is asserted to be ONE grey level with bin_image's edges.  The single MCC call declines more than 64 occurring
levels, so roi_features_batch leaves MCC NaN for such a ROI and the comparison call is made with mcc=False there.
"""
import math

import numpy as np
import pytest

import firstorder_reference as fr
import test_gpu_firstorder_limits as lim
from test_gpu_batch_rois import RAGGED

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int32, np.int16]
ROUTE, ROUTE_SINGLE, ROUTE_CLASS = "batch-firstorder", "batch-firstorder-single", "batch-firstorder-class"
FIELDS = fr.FIELDS


def _k(m):
    """K of the module docstring"""
    return max(11, -(-m // 256) + 6 + 3)


def _values(dtype, n, rng, lo=-900, hi=15000):
    if np.issubdtype(dtype, np.integer):
        return rng.integers(lo, hi, n).astype(dtype)
    return (rng.standard_normal(n) * 37.5 + 11).astype(dtype)


def _roi(dtype, shape, seed, fill=0.6, count=None):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    img = _values(dtype, n, rng).reshape(shape)
    mask = fr.mask_with_count(shape, count, seed + 3) if count is not None else rng.random(shape) < fill
    return img, mask


def _dev(imgs, masks):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs], [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in masks]


def _bits(x):
    return np.float64(x).tobytes()


def _check_rows(label, imgs, masks, rows, status, shift=0.0, single=()):
    """witness 1 and, for the equal fields, witness 2 on every ROI of a batch"""
    from pyradiomics_amd import engine
    assert rows.shape == (len(imgs), 15) and rows.dtype == np.float64 and len(status) == len(imgs)
    I, M = _dev(imgs, masks)
    for b, (img, mask) in enumerate(zip(imgs, masks)):
        if not mask.any():
            assert status[b] == 1 and np.isnan(rows[b]).all(), (label, b, status[b], rows[b])
            continue
        assert status[b] == (8 if b in single else 0), (label, b, status[b])
        ref = fr.segment_reference(img, mask != 0, shift)
        got = dict(zip(FIELDS, (float(v) for v in rows[b])))
        k = fr.k_reduction(img.size, img.dtype.itemsize) if b in single else _k(ref["m"])
        lim._check(ROUTE_SINGLE if b in single else ROUTE, (label, b, ref["m"]), got, ref, k, k)
        st = engine.firstorder_stats(I[b], M[b], shift)
        for f in fr.EXACT:
            same = got[f] == st[f] if len(ref["zero_signs"]) == 2 else _bits(got[f]) == _bits(st[f])
            assert same, (label, b, f, got[f], st[f])


def _check_bins(label, imgs, masks, **binning):
    from pyradiomics_amd import engine
    I, M = _dev(imgs, masks)
    levels, Ng, edges, counts = engine.bin_batch(I, M, **binning)
    route = engine.last_batch_route()
    import torch
    assert levels.dtype == torch.int32 and levels.numel() == sum(i.size for i in imgs)
    host = levels.cpu().numpy()
    start = 0
    for b, (img, mask) in enumerate(zip(imgs, masks)):
        mine = host[start:start + img.size].reshape(img.shape)
        start += img.size
        if not mask.any():
            assert Ng[b] == 0 and len(edges[b]) == 0 and counts[b].tolist() == [0] and not mine.any(), (label, b)
            continue
        lv, ng, e, c = engine.bin_image(I[b], M[b], with_counts=True, **binning)
        assert Ng[b] == ng, (label, b, Ng[b], ng)
        assert edges[b].dtype == np.float64 and np.array_equal(edges[b], e), (label, b)
        assert counts[b].dtype == np.int64 and np.array_equal(counts[b], c), (label, b, counts[b], c)
        assert np.array_equal(mine, lv.cpu().numpy()), (label, b)
        assert int(c.sum()) == int((mask != 0).sum()) and c[0] == 0
    return route, Ng, edges, counts


def _run(label, imgs, masks, shift=0.0, single=(), route="batch", **binning):
    from pyradiomics_amd import engine
    I, M = _dev(imgs, masks)
    rows, status = engine.firstorder_batch(I, M, voxelArrayShift=shift)
    assert engine.last_batch_route() == route, (label, engine.last_batch_route())
    _check_rows(label, imgs, masks, rows, status, shift, single)
    if binning:
        broute, _, _, _ = _check_bins(label, imgs, masks, **binning)
        assert broute == route, (label, broute)
    return rows, status


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batch_with_a_shift(dtype):
    """unaligned offsets for every dtype (boxes of 1, 9, 8, 8, 255 voxels precede the larger ones), axes of 1 and 2, 1 x 1 x 1"""
    from pyradiomics_amd import _lib
    big = 0.2 if dtype == np.float64 else 0.4          # the 65280-voxel box stays below the key capacity (16384 / 32768)
    rois = [_roi(dtype, s, 100 + k, big if np.prod(s) > 16384 else 0.6) for k, s in enumerate(RAGGED)]
    imgs, masks = [r[0] for r in rois], [r[1] for r in rois]
    masks[0] = np.ones((1, 1, 1), dtype=bool)
    offs = np.cumsum([0] + [i.size for i in imgs[:-1]])
    assert any(int(o) * np.dtype(dtype).itemsize % 16 for o in offs)
    _run(("ragged", dtype.__name__), imgs, masks, shift=2.5, binWidth=25)
    assert _lib.last_path() is not None


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_and_power_of_two_counts(dtype):
    """m = 1 .. 11: quantile ranks clamped, gamma 0 and fractional; 63 .. 1025: the sort's padding and the thread striding"""
    ms = (1, 2, 3, 4, 5, 10, 11, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
    rois = [_roi(dtype, (1, 3, (m + 9) // 3 + 1), 200 + m, count=m) for m in ms]
    assert [int(r[1].sum()) for r in rois] == list(ms)
    gam = {m: [fr.quantile_pos(m, q)[2] for _, q in fr.QUANTILES] for m in ms}
    assert 0.0 in gam[11] and any(0 < g < 1 and g != 0.5 for g in gam[10])
    _run(("counts", dtype.__name__), [r[0] for r in rois], [r[1] for r in rois], binWidth=25)


@pytest.mark.parametrize("dtype", DTYPES)
def test_key_capacity(dtype):
    """capacity - 1 and capacity ROI voxels in a box larger than the capacity: batched; capacity + 1: verdict 8, the single call
    serves that ROI, its neighbours keep their rows"""
    import torch
    from pyradiomics_amd import engine
    cap = engine.batch_firstorder_max_roi(torch.from_numpy(np.zeros(1, dtype=dtype)).dtype)
    assert cap == (16384 if dtype == np.float64 else 32768)
    shape = (cap // 1024 + 1, 32, 32)
    assert int(np.prod(shape)) > cap + 1
    under, at, over = (_roi(dtype, shape, 300 + k, count=cap - 1 + k) for k in range(3))
    small = [_roi(dtype, (3, 4, 5), 310), _roi(dtype, (2, 7, 3), 311)]
    _run(("capacity", dtype.__name__), [under[0], at[0]], [under[1], at[1]])
    imgs, masks = [small[0][0], over[0], small[1][0]], [small[0][1], over[1], small[1][1]]
    rows, status = _run(("capacity + 1", dtype.__name__), imgs, masks, single=(1,), route="mixed", binWidth=25)
    assert status.tolist() == [0, 8, 0]
    alone, _ = engine.firstorder_batch(*_dev([imgs[0], imgs[2]], [masks[0], masks[2]]))
    assert engine.last_batch_route() == "batch"
    assert np.array_equal(rows[[0, 2]], alone, equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_adversarial_values(dtype):
    """constant ROI; two values with the tie run across the P10 rank; values on bin edges; negative intensities"""
    from pyradiomics_amd import engine
    rng = np.random.default_rng(41)
    const = (np.full((3, 4, 5), 7, dtype=dtype), rng.random((3, 4, 5)) < 0.7)
    two = fr._fill((4, 5, 6), 97, np.where(np.arange(97) < 40, 3, 11).astype(dtype), 42, outside=5)
    assert len(set(two[0][two[1]].tolist())) == 2
    xs = np.sort(two[0][two[1]])
    p = fr.quantile_pos(97, 0.1)
    assert xs[p[0]] == 3 and xs[p[1]] == 11                      # the tie run is cut exactly between P10's two ranks
    on_edges = ((rng.integers(-6, 9, (5, 5, 5)) * 25).astype(dtype), rng.random((5, 5, 5)) < 0.6)
    negative = ((-rng.integers(130, 977, (4, 4, 7))).astype(dtype), rng.random((4, 4, 7)) < 0.6)
    rois = [const, two, on_edges, negative]
    imgs, masks = [r[0] for r in rois], [r[1] for r in rois]
    rows, _ = _run(("adversarial", dtype.__name__), imgs, masks, binWidth=25)
    ref = fr.segment_reference(*const)
    for k, f in enumerate(FIELDS):
        assert rows[0, k] == ref["values"][f], (f, rows[0, k], ref["values"][f])          # every field exact
    _, Ng, edges, counts = _check_bins("adversarial", imgs, masks, binWidth=25)
    # (binWidth edges are anchored at 0 -- [0, 25, 50] here; the constant ROI still is ONE grey level.  The single-bin pair
    # [v - 0.5, v + 0.5] of getBinEdges belongs to an edge list of length 1, which np.arange never returns for these arguments.)
    assert Ng[0] == 1 and edges[0].tolist() == [0.0, 25.0, 50.0] and counts[0].tolist() == [0, int(const[1].sum())]
    assert edges[3][0] <= negative[0][negative[1]].min() < 0 and edges[3][0] % 25 == 0
    assert set(np.unique(on_edges[0][on_edges[1]]).tolist()) <= set(edges[2].tolist())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signed_zeros(dtype):
    both = np.array([-0.0, 4, 0.0, -3, -0.0, 5, 0.0, -2, -0.0, 0.0, 0.0], dtype=dtype).reshape(1, 1, -1)
    neg = np.array([-0.0, 4, -0.0, -3, -0.0, 5, -0.0, -2, -0.0], dtype=dtype).reshape(1, 1, -1)
    assert fr.segment_reference(both, np.ones(both.shape, bool))["zero_signs"] == {-1, 1}
    rows, _ = _run(("zeros", dtype.__name__), [both, neg], [np.ones(both.shape, bool), np.ones(neg.shape, bool)], binWidth=25)
    assert np.signbit(rows[1, FIELDS.index("Median")])            # a -0.0 comes back as -0.0


def test_bin_count_and_the_edge_cap():
    """float32 with binCount 16, float64 with binCount 64; int16 with binWidth 1 and a range above the edge cap: that ROI goes
    through bin_image"""
    from pyradiomics_amd import engine
    for dtype, nb in ((np.float32, 16), (np.float64, 64)):
        rois = [_roi(dtype, s, 500 + k) for k, s in enumerate([(4, 5, 6), (1, 1, 3), (7, 8, 9)])]
        masks = [rois[0][1], np.array([[[True, False, True]]]), rois[2][1]]
        route, Ng, edges, _ = _check_bins(("binCount", nb), [r[0] for r in rois], masks, binCount=nb)
        assert route == "batch" and all(len(e) == nb + 1 for e in edges) and Ng.max() == nb
    cap = engine.batch_digitize_max_edges()
    rng = np.random.default_rng(51)
    narrow = (rng.integers(-40, 90, (4, 5, 6)).astype(np.int16), rng.random((4, 5, 6)) < 0.6)
    at_cap = (rng.integers(0, cap - 1, (6, 6, 6)).astype(np.int16), np.ones((6, 6, 6), dtype=bool))
    at_cap[0].flat[0], at_cap[0].flat[1] = 0, cap - 2                # arange(0, cap - 2 + 2, 1): exactly `cap` edges
    wide = (rng.integers(-5000, 5000, (6, 6, 6)).astype(np.int16), rng.random((6, 6, 6)) < 0.6)
    wide[0].flat[0], wide[0].flat[1] = -5000, 4999
    wide[1].flat[0] = wide[1].flat[1] = True
    imgs, masks = [narrow[0], at_cap[0], wide[0]], [narrow[1], at_cap[1], wide[1]]
    route, Ng, edges, _ = _check_bins("edge cap", imgs, masks, binWidth=1)
    assert len(edges[1]) == cap and len(edges[2]) > cap and Ng[2] == 10000 and route == "mixed"
    route, _, _, _ = _check_bins("edge cap", imgs[:2], masks[:2], binWidth=1)
    assert route == "batch"


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_and_full_masks(dtype):
    from pyradiomics_amd import engine
    a, b, c = _roi(dtype, (4, 5, 6), 600), _roi(dtype, (3, 3, 3), 601), _roi(dtype, (5, 4, 3), 602)
    imgs = [a[0], b[0], c[0]]
    masks = [a[1], np.zeros((3, 3, 3), dtype=bool), np.ones((5, 4, 3), dtype=bool)]
    rows, status = _run(("empty / full", dtype.__name__), imgs, masks, binWidth=25)
    assert status.tolist() == [0, 1, 0] and np.isnan(rows[1]).all()
    alone, _ = engine.firstorder_batch(*_dev([imgs[0], imgs[2]], [masks[0], masks[2]]))
    assert np.array_equal(rows[[0, 2]], alone, equal_nan=True)            # the others are unaffected
    table, st = engine.roi_features_batch(*_dev(imgs, masks), binCount=16)
    assert st == [1, 0, 1]
    for cls, t in table.items():
        assert np.isnan(t[1]).all() and not np.isnan(t[[0, 2]]).all(), cls


def test_more_rois_than_compute_units():
    """B = 600 ROIs of 3 x 3 x 3: every row equals the row of the same ROI computed alone"""
    from pyradiomics_amd import engine
    rois = [_roi(np.float32, (3, 3, 3), 700 + k) for k in range(600)]
    I, M = _dev([r[0] for r in rois], [r[1] for r in rois])
    rows, status = engine.firstorder_batch(I, M)
    assert engine.last_batch_route() == "batch" and rows.shape == (600, 15)
    levels, Ng, edges, counts = engine.bin_batch(I, M, stats=(rows, status), binWidth=25)
    lv = levels.cpu().numpy().reshape(600, 27)
    for b in range(600):
        one, st1 = engine.firstorder_batch([I[b]], [M[b]])
        assert st1[0] == status[b] and np.array_equal(one[0], rows[b], equal_nan=True), b
        l1, n1, e1, c1 = engine.bin_batch([I[b]], [M[b]], stats=(one, st1), binWidth=25)
        assert n1[0] == Ng[b] and np.array_equal(e1[0], edges[b]) and np.array_equal(c1[0], counts[b]), b
        assert np.array_equal(l1.cpu().numpy(), lv[b]), b
    for b in range(0, 600, 97):                                            # and the reference, on a sample
        if rois[b][1].any():
            ref = fr.segment_reference(*rois[b])
            lim._check(ROUTE, ("600", b), dict(zip(FIELDS, rows[b].tolist())), ref, _k(ref["m"]), _k(ref["m"]))


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_rows_do_not_depend_on_the_run_or_the_order(dtype):
    """the same batch twice, then with its ROIs in reversed order: bit-identical rows (the sums run over the sorted values in a
    fixed order; where the compaction's atomics land does not matter)"""
    from pyradiomics_amd import engine
    shapes = [(9, 10, 11), (16, 16, 16), (3, 17, 5), (12, 13, 14), (1, 1, 9)]
    rois = [_roi(dtype, s, 800 + k) for k, s in enumerate(shapes)]
    I, M = _dev([r[0] for r in rois], [r[1] for r in rois])
    first, _ = engine.firstorder_batch(I, M, voxelArrayShift=1.5)
    again, _ = engine.firstorder_batch(I, M, voxelArrayShift=1.5)
    back, _ = engine.firstorder_batch(I[::-1], M[::-1], voxelArrayShift=1.5)
    assert first.tobytes() == again.tobytes()
    assert first.tobytes() == np.ascontiguousarray(back[::-1]).tobytes()


def _feature_bounds(ref, k, vol):
    v, b = ref["values"], fr.seg_bounds(ref, k, k)
    d = fr.derived_bounds(v, b)
    m2s = v["m2"] if v["m2"] else 1.0
    return {"Energy": (v["Energy"], b["Energy"]), "TotalEnergy": (v["Energy"] * vol, b["Energy"] * vol + fr.U * abs(v["Energy"] * vol)),
            "Minimum": (v["Minimum"], 0.0), "10Percentile": (v["P10"], 0.0), "90Percentile": (v["P90"], 0.0),
            "Maximum": (v["Maximum"], 0.0), "Mean": (v["Mean"], b["Mean"]), "Median": (v["Median"], 0.0),
            "InterquartileRange": (v["P75"] - v["P25"], 0.0), "Range": (v["Maximum"] - v["Minimum"], 0.0),
            "MeanAbsoluteDeviation": (v["MAD"], b["MAD"]), "RobustMeanAbsoluteDeviation": (v["rMAD"], b["rMAD"]),
            "RootMeanSquared": (math.sqrt(v["Energy"] / v["Np"]), d["RootMeanSquared"]),
            "StandardDeviation": (math.sqrt(v["m2"]), d["StandardDeviation"]), "Variance": (v["m2"], d["Variance"]),
            "Skewness": (v["m3"] / m2s ** 1.5, d["Skewness"]), "Kurtosis": (v["m4"] / m2s ** 2, d["Kurtosis"])}


def test_feature_table_with_three_level_counts():
    """binWidth 25 on ROIs of three intensity ranges: three different Ng, one above 64 (texture_features_batch loops the single
    calls there): every row equals the row of a one-ROI call; texture columns = texture_features_batch on bin_batch's levels;
    first-order columns = features_from_stats of firstorder_batch's rows, inside derived_bounds of the reference"""
    from pyradiomics_amd import cmatrices, engine, firstorder, imageoperations
    rng = np.random.default_rng(91)
    spans = [(0, 200), (-300, 700), (0, 200), (-1000, 2000), (-300, 700)]
    shapes = [(5, 6, 7), (6, 6, 6), (4, 7, 5), (6, 5, 6), (3, 8, 6)]
    imgs = [rng.integers(lo, hi, s).astype(np.int16) for (lo, hi), s in zip(spans, shapes)]
    masks = [rng.random(s) < 0.7 for s in shapes]
    for (lo, hi), i, m in zip(spans, imgs, masks):
        i.flat[0], i.flat[1], m.flat[0], m.flat[1] = lo, hi - 1, True, True
    I, M = _dev(imgs, masks)
    vol = 0.75
    table, status = engine.roi_features_batch(I, M, binWidth=25, voxelArrayShift=3.0, voxelVolume=vol)
    assert engine.last_batch_route() == "mixed" and status == [1] * 5
    assert list(table) == list(engine.ROI_FEATURE_CLASSES)
    rows, verdict = engine.firstorder_batch(I, M, voxelArrayShift=3.0)
    levels, Ng, edges, counts = engine.bin_batch(I, M, stats=(rows, verdict), binWidth=25)
    assert sorted(set(Ng.tolist())) == [8, 40, 120]
    want_fo = firstorder.features_from_stats(rows, [c[1:] for c in counts], vol)
    assert table["firstorder"].tobytes() == want_fo.tobytes()
    names = cmatrices.FIRSTORDER_FEATURES
    start = 0
    for b in range(5):
        one, st1 = engine.roi_features_batch([I[b]], [M[b]], binWidth=25, voxelArrayShift=3.0, voxelVolume=vol)
        assert st1 == [1]
        n = imgs[b].size
        tex, _ = engine.texture_features_batch(levels[start:start + n], M[b].reshape(-1), np.array([shapes[b]]), int(Ng[b]),
                                               mcc=Ng[b] <= 64)       # (the single MCC call declines more than 64 levels)
        start += n
        for cls in table:
            assert np.array_equal(table[cls][b], one[cls][0], equal_nan=True), (b, cls)
            if cls != "firstorder":
                assert np.array_equal(table[cls][b], tex[cls][0], equal_nan=True), (b, cls)
                assert np.array_equal(np.isnan(table[cls][b]), np.isnan(tex[cls][0])), (b, cls)
        ref = fr.segment_reference(imgs[b], masks[b], 3.0)
        got = dict(zip(names, table["firstorder"][b].tolist()))
        for f, (w, bd) in _feature_bounds(ref, _k(ref["m"]), vol).items():
            err = abs(got[f] - w)
            if bd > 0:
                lim._note(ROUTE_CLASS, {f: err / bd})
            assert err <= bd, (b, f, got[f], w, err, bd)
        host_levels, _ = imageoperations.binImage(imgs[b], masks[b], binWidth=25)
        c = np.bincount(host_levels[masks[b]])
        hist = firstorder.features_from_stats(rows[b], c[c > 0], vol, ["Entropy", "Uniformity"])
        assert got["Entropy"] == hist[0, 0] and got["Uniformity"] == hist[0, 1], b


def test_side_queue_mask_types_and_flat_input():
    """one call on engine.side_queue; masks as bool and as uint8 / int32 with values other than 1; flat tensors + sizes"""
    import torch
    from pyradiomics_amd import engine
    rois = [_roi(np.float32, s, 950 + k) for k, s in enumerate([(4, 5, 6), (1, 1, 9), (7, 3, 2)])]
    imgs, masks = [r[0] for r in rois], [r[1] for r in rois]
    I, M = _dev(imgs, masks)
    assert M[0].dtype == torch.bool
    rows, status = engine.firstorder_batch(I, M, voxelArrayShift=0.5)
    binned = engine.bin_batch(I, M, binCount=8)
    with engine.side_queue(0):
        srows, sstatus = engine.firstorder_batch(I, M, voxelArrayShift=0.5)
        sbinned = engine.bin_batch(I, M, binCount=8)
    torch.cuda.synchronize()
    assert np.array_equal(rows, srows, equal_nan=True) and np.array_equal(status, sstatus)
    assert torch.equal(binned[0], sbinned[0]) and np.array_equal(binned[1], sbinned[1])
    u8 = [torch.from_numpy(m.astype(np.uint8) * v).cuda() for m, v in zip(masks, (255, 7, 2))]
    i32 = [torch.from_numpy(m.astype(np.int32) * -3).cuda() for m in masks]
    sizes = np.array([i.shape for i in imgs])
    flat = (torch.cat([i.reshape(-1) for i in I]), torch.cat([m.reshape(-1) for m in u8]))
    for variant in ((I, u8, None), (I, i32, None), (flat[0], flat[1], sizes)):
        r, s = engine.firstorder_batch(variant[0], variant[1], variant[2], voxelArrayShift=0.5)
        assert np.array_equal(rows, r, equal_nan=True) and np.array_equal(status, s)
        lv, ng, _, _ = engine.bin_batch(variant[0], variant[1], variant[2], binCount=8)
        assert torch.equal(binned[0], lv) and np.array_equal(binned[1], ng)
    _check_rows("side queue", imgs, masks, srows, sstatus, 0.5)


def test_host_lists_through_cmatrices():
    from pyradiomics_amd import cmatrices, engine
    rois = [_roi(np.int16, s, 970 + k) for k, s in enumerate([(5, 5, 5), (4, 6, 3)])]
    imgs, masks = [r[0] for r in rois], [r[1] for r in rois]
    table, _ = engine.roi_features_batch(*_dev(imgs, masks), binCount=16, voxelArrayShift=1.0, voxelVolume=2.0)
    got = cmatrices.calculate_roi_features_batch(imgs, masks, binCount=16, voxelArrayShift=1.0, voxelVolume=2.0)
    assert cmatrices.last_batch_route() == "batch"
    assert set(got) == set(engine.ROI_FEATURE_CLASSES) and list(got["firstorder"]) == cmatrices.FIRSTORDER_FEATURES
    for k, name in enumerate(cmatrices.FIRSTORDER_FEATURES):
        assert np.array_equal(got["firstorder"][name], table["firstorder"][:, k]), name
    for k, name in enumerate(cmatrices.batch_feature_names("glcm")):
        assert name and np.array_equal(got["glcm"][name], table["glcm"][:, k], equal_nan=True), name
    fo = cmatrices.calculate_firstorder_batch(imgs, masks, voxelArrayShift=1.0, voxelVolume=2.0, binCount=16)
    assert list(fo) == ["firstorder"]
    for name in cmatrices.FIRSTORDER_FEATURES:
        assert np.array_equal(fo["firstorder"][name], got["firstorder"][name]), name


def _same_bits(a, b, what):
    """bit for bit, NaNs equal to one another"""
    if a is None or b is None:
        assert a is None and b is None, what
        return
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        assert np.array_equal(nan, np.isnan(b)), what
        a, b = a[~nan], b[~nan]
    assert a.tobytes() == b.tobytes(), what


def _same_tables(got, want, what):
    (tg, sg), (tw, sw) = got, want
    assert sg == sw and list(tg) == list(tw), what
    for key in tw:
        if key == "glcm_mcc_angles":
            assert len(tg[key]) == len(tw[key]), what
            for b, (x, y) in enumerate(zip(tg[key], tw[key])):
                _same_bits(x, y, (what, key, b))
        else:
            _same_bits(tg[key], tw[key], (what, key))


def test_three_ways_to_hand_over_a_batch():
    """the same three boxes as lists of non-contiguous views with int64 masks, as lists of contiguous tensors with bool masks and
    as flat tensors plus `sizes`: roi_features_batch (all six classes, extras) and texture_features_batch (int64 levels, Ng = 8)
    answer the three bit for bit -- tables, gray_levels, glcm_mcc_angles and status"""
    import torch
    from pyradiomics_amd import engine
    rng = np.random.default_rng(4242)
    shapes = [(2, 3, 5), (7, 4, 3), (1, 1, 4)]
    imgs = [rng.uniform(0.0, 199.0, s).astype(np.float32) for s in shapes]         # about eight bins of width 25
    masks = [rng.random(s) < 0.8 for s in shapes]
    for i, m in zip(imgs, masks):
        m.flat[0], m.flat[1], m.flat[-1] = True, True, False                       # at least two voxels in, at least one out
        i.flat[0], i.flat[1] = 1.0, 198.0
    lvls = [(np.floor(i / 25.0) + 1).astype(np.int64) for i in imgs]
    assert all(l.min() >= 1 and l.max() <= 8 for l in lvls)
    sizes = np.array(shapes)

    def strided(a):
        wide = np.zeros(a.shape[:2] + (2 * a.shape[2],), dtype=a.dtype)
        wide[:, :, ::2] = a
        view = torch.from_numpy(wide).cuda()[:, :, ::2]
        assert not view.is_contiguous() and np.array_equal(view.cpu().numpy(), a)
        return view

    def ways(arrays):
        cont = [torch.from_numpy(a).cuda() for a in arrays]
        return [strided(a) for a in arrays], cont, torch.cat([c.reshape(-1) for c in cont])
    m64 = [torch.from_numpy(m.astype(np.int64) * 5).cuda() for m in masks]
    mbool = [torch.from_numpy(m).cuda() for m in masks]
    mflat = torch.cat([m.reshape(-1) for m in mbool]).view(torch.uint8)
    a, b, c = ways(imgs)
    kw = dict(binWidth=25, voxelArrayShift=2.0, voxelVolume=0.5, extras=True)
    want = engine.roi_features_batch(b, mbool, **kw)
    assert list(want[0]) == list(engine.ROI_FEATURE_CLASSES) + ["gray_levels", "glcm_mcc_angles"] and want[1] == [1, 1, 1]
    _same_tables(engine.roi_features_batch(a, m64, **kw), want, "strided views, int64 masks")
    _same_tables(engine.roi_features_batch(c, mflat, sizes, **kw), want, "flat tensors")
    a, b, c = ways(lvls)
    assert a[0].dtype == torch.int64
    want = engine.texture_features_batch(b, mbool, None, 8, mcc_angles=True)
    assert want[1] == [1, 1, 1] and "glcm_mcc_angles" in want[0]
    _same_tables(engine.texture_features_batch(a, m64, None, 8, mcc_angles=True), want, "strided levels, int64 masks")
    _same_tables(engine.texture_features_batch(c, mflat, sizes, 8, mcc_angles=True), want, "flat levels")


def test_zz_report():
    print()
    mine = {k: r for k, r in lim.RATIOS.items() if k[0] in (ROUTE, ROUTE_SINGLE, ROUTE_CLASS)}
    for (route, f), r in sorted(mine.items()):
        print("    %-24s %-28s %.3g" % (route, f, r))
    assert mine and all(r <= 1 for r in mine.values())

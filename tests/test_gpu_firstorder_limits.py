"""GPU: the first-order statistic kernels (csrc/kernels_firstorder.h, prad_firstorder.hip) at the limits of their routes --
firstorder-sort, firstorder-select, firstorder-exact, firstorder-queue and the voxel-mode wave kernel -- against
tests/firstorder_reference.py (long double; pinned by tests/test_firstorder_reference.py, which also shows that the
comparison used here rejects a dropped voxel, a rank off by one, a float32 mean and a swapped voxel on every case family).
Every case asserts the route it took and compares ALL fields.

Tolerances (firstorder_reference.seg_bounds / voxel_bounds).  Np, Minimum, Maximum, the percentiles and Median must be
equal; rMAD is NaN exactly where the reference's is.  A summed field obeys |got - ref| <= K 2^-53 abs_sum, abs_sum = the
long-double sum of the absolute terms.  K is the longest chain of float64 additions a term passes through:
  * fo_sums_kernel, fo_central_kernel, fo_band_kernel (routes sort, select, queue; Energy and Mean of the exact route)
    run blocks = min(ceil(n / 256), 1024) workgroups of 256 threads over the n voxels of the ARRAY.  Thread t of the
    T = 256 blocks takes the 16-byte pieces t, t + T, ... (E = 16 / sizeof(T) voxels each, added in index order) and at
    most one voxel of the tail: E ceil(floor(n / E) / T) + [n mod E > 0] additions.  Then 6 __shfl_xor steps, the 3
    additions of sh[0] + sh[1] + sh[2] + sh[3], and the host's (or, on the queue route, a glue kernel's) serial sum
    over the blocks.  K = that sum (firstorder_reference.k_reduction): 11 for one voxel, 1039 for float64 at 2^20 voxels.
  * exact-histogram route: MAD, rMAD and the moments are summed on the host over the distinct values, ascending (in long
    double, so far inside the bound): K = the number of distinct values.
  * a final division (Mean, MAD, rMAD, the moments) counts as one more rounding.
  * the central moments add k |dmu| A_(k-1) (the first-order effect of the mean's own rounding |dmu| <= (K + 1) 2^-53
    sum |x| / m on a moment about it; A_j the j-th absolute central moment), rMAD the same with the band's mean.
  * voxel mode: one wave per centre, lane l adds the window slots l, l + 64, ...: K = ceil(Nk / 64) + 6 shuffle steps;
    the derived features (RootMeanSquared, StandardDeviation, Variance, Skewness, Kurtosis, TotalEnergy) propagate their
    components' bounds to first order plus 4 roundings of the formula (firstorder_reference.derived_bounds).
The roundings inside one term (at most 7 for d^4) are not part of K; K is never below 11 (segment) or 7 (voxel).

Measured worst error / bound per (route, field) over all cases of this module on an MI355X (every comparison records its
ratio; test_zz_report prints this table and fails on any ratio above 1):
    route              Energy   Mean     MAD      rMAD     m2       m3       m4
    firstorder-sort    0.142    0.1      0.0865   0.0745   0.217    0.47     0.102
    firstorder-select  0.289    0.00962  0.0455   0.00634  0.128    0.465    0.0162
    firstorder-exact   0.156    0        0        1.32e-05 5.12e-05 3.94e-07 0
    firstorder-queue   0.00515  0.00962  0.00352  0.00353  0.0042   0.00769  0.00391
    class              Energy 0.0683   Mean 0.064   MeanAbsoluteDeviation 0.000187   RobustMeanAbsoluteDeviation 0.000187
                       RootMeanSquared 0.117   Variance 0   Skewness 0.062   Kurtosis 0.000618
    voxel              Energy 0.505   TotalEnergy 0.442   Entropy 0.469   Uniformity 0.446   Mean 0.248
                       MeanAbsoluteDeviation 0.16   RobustMeanAbsoluteDeviation 0.151   RootMeanSquared 0.265
                       StandardDeviation 0.174   Variance 0.194   Skewness 0.164   Kurtosis 0.118
On the exact route the sum of x is an integer below 2^53, so Mean is exact; so is Energy, except on can-i32-max / -min, whose
squares near 2^62 are rounded one by one (the 0.156).  The bound is met everywhere with a margin of at least 2
and is not vacuous: the comparator tests reject single-voxel defects under it.
The voxel kernel's smallest padded window is P = 2 (prad_voxel_firstorder_dev starts at 2), which serves the window of 1.

Out of scope: non-finite ROI values (NaN, +-inf); ROIs above 2^31 - 1 voxels (declined by the entry point); the Entropy /
Uniformity of segment mode (numpy on the host from the level census, tests/test_firstorder.py).

Defect found by reading fo_scan while deriving K, fixed in the same change and kept covered by
test_misaligned_views_give_the_bits_of_an_aligned_copy: the scalar branch (misaligned image or mask pointer) dealt the
voxels to the threads one by one where the wide-load branch deals them in 16-byte pieces, so the partial sums -- and the
last bits of Energy, Mean and the moments -- depended on the alignment of the view.
"""
import math

import numpy as np
import pytest

import firstorder_reference as fr

pytestmark = pytest.mark.gpu

RATIOS = {}            # (route, field) -> worst error / bound
_dev = {}              # case name -> (image tensor, mask tensor) on the device


def _note(route, ratios):
    for f, r in ratios.items():
        RATIOS[(route, f)] = max(RATIOS.get((route, f), 0.0), r)


def _check(route, label, got, ref, k_sum, k_cen):
    bad, ratios = fr.compare(got, ref, fr.seg_bounds(ref, k_sum, k_cen))
    _note(route, ratios)
    assert not bad, (label, route, bad)


def _tensors(name):
    import torch
    if name not in _dev:
        img, mask, _, _ = fr.case(name)
        _dev[name] = (torch.from_numpy(img).cuda(), torch.from_numpy(mask.view(np.uint8)).cuda())
    return _dev[name]


def _run_case(name, route=None):
    from pyradiomics_amd import _lib, engine
    _, _, shift, want_route = fr.case(name)
    I, M = _tensors(name)
    got = engine.firstorder_stats(I, M, shift)
    assert _lib.last_path() == (route or want_route), (name, _lib.last_path())
    _check(_lib.last_path(), name, got, fr.case_reference(name), *fr.case_k(name, route or want_route))
    return got


# ---- segment mode: route boundaries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fr.BOUNDARY)
def test_route_boundaries(name):
    from pyradiomics_amd import cmatrices, _lib
    img, mask, shift, route = fr.case(name)
    ref = fr.case_reference(name)
    if name.startswith("b16"):
        assert ref["m"] == 65535 + ("exact" in name)
    if name.startswith("b20"):
        assert ref["m"] == (1 << 20) - 1 + ("select" in name)
    if name.startswith("range"):
        assert ref["m"] >= 1 << 16 and ref["values"]["Maximum"] - ref["values"]["Minimum"] == int(name[-5:])
    got = _run_case(name)
    if name == "range-32768":
        assert _lib.last_path() != "firstorder-exact"
    if name.startswith("const"):
        for f, w in ref["values"].items():
            assert got[f] == w, (name, f, got[f], w)              # every field exact
    # the host-array entry point takes the same route to the same bits
    host = cmatrices.firstorder_stats(img, mask, shift)
    assert _lib.last_path() == route
    assert host == got or all(np.array_equal(host[f], got[f], equal_nan=True) for f in got)


# ---- segment mode: rank placement ----------------------------------------------------------------------------------------
def _placements(n, m):
    """ROI index sets of m voxels in an array of n: first voxel only, last voxel only, inside the last block, spread"""
    out = {}
    if m == 1:
        out["first"] = [0]
        out["last"] = [n - 1]
    start = ((n - 1) // 256) * 256
    if n - start >= m:
        out["last-block"] = list(range(n - m, n))
    if n >= m:
        out["spread"] = sorted(set(np.linspace(0, n - 1, m).astype(int).tolist()))
    return {k: v for k, v in out.items() if len(v) == m}


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
def test_rank_placement(dtype):
    """gamma = 0 and 0.5, prev == next clamped, in arrays of one voxel, around one block, with a vector tail"""
    import torch
    from pyradiomics_amd import _lib, engine
    from test_firstorder import _volume
    seen = set()
    for n in (1, 255, 256, 257, 259, 1029):
        assert n in (1, 256) or n % (16 // np.dtype(dtype).itemsize) != 0          # 255, 257, 259, 1029 leave a vector tail
        img = _volume(dtype, (n,), n)[0]
        I = torch.from_numpy(img).cuda()
        for m in (1, 2, 3, 4, 5, 9, 10, 11, 21):
            for place, idx in _placements(n, m).items():
                mask = np.zeros(n, dtype=np.uint8)
                mask[idx] = 1
                for shift in (0.0, 2.5):
                    got = engine.firstorder_stats(I, torch.from_numpy(mask).cuda(), shift)
                    assert _lib.last_path() == "firstorder-sort"
                    ref = fr.stats_of_values(img[idx], shift, np.issubdtype(dtype, np.integer))
                    k = fr.k_reduction(n, img.dtype.itemsize)
                    _check("firstorder-sort", (n, m, place, shift), got, ref, k, k)
                seen.add((m, place))
                gam = [fr.quantile_pos(m, q)[2] for _, q in fr.QUANTILES]
                if m in (1, 2, 3, 5, 9, 11, 21):
                    assert 0.0 in gam or 0.5 in gam
    assert {(1, "first"), (1, "last"), (21, "last-block"), (21, "spread"), (2, "spread")} <= seen


def test_negative_zero_keeps_its_sign():
    """order statistics are elements of the image: a -0.0 comes back as -0.0 (the comparison checks the sign of a zero)"""
    import torch
    from pyradiomics_amd import _lib, engine
    for dtype in (np.float32, np.float64):
        for x in (np.array([-0.0, 4, -0.0, -3, -0.0, 5, -0.0, -2, -0.0], dtype=dtype), np.array([-0.0] * 3, dtype=dtype)):
            ref = fr.stats_of_values(x, 0.0)
            assert np.signbit(ref["values"]["Median"]) and ref["zero_signs"] == {-1}
            got = engine.firstorder_stats(torch.from_numpy(x).cuda(), torch.ones(len(x), dtype=torch.uint8, device="cuda"), 0.0)
            assert _lib.last_path() == "firstorder-sort"
            k = fr.k_reduction(len(x), x.dtype.itemsize)
            _check("firstorder-sort", ("negative zero", dtype.__name__, len(x)), got, ref, k, k)


# ---- segment mode: alignment ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5003, (1 << 20) + 4101])
@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
def test_misaligned_views_give_the_bits_of_an_aligned_copy(dtype, n):
    """engine.firstorder_stats hands a contiguous view to the kernels where it lies (no copy): a misaligned image and / or
    mask pointer takes the scalar branch of fo_scan, which must add the same voxels in the same order"""
    import torch
    from pyradiomics_amd import _lib, engine
    from test_firstorder import _volume
    img, roi = _volume(dtype, (n,), 17, 0.6 if n < 10000 else 0.9999)
    E = 16 // img.dtype.itemsize
    big = n > 1 << 20
    route = ("firstorder-exact" if np.issubdtype(dtype, np.integer) else "firstorder-select") if big else "firstorder-sort"
    ref = fr.stats_of_values(img[roi], 3.0, np.issubdtype(dtype, np.integer))
    assert ref["m"] >= 1 << 20 if big else ref["m"] < 1 << 16
    k = fr.k_reduction(n, img.dtype.itemsize)
    k_cen = ref["distinct"] if route == "firstorder-exact" else k
    ibuf = torch.zeros(n + 16, dtype=torch.from_numpy(img).dtype, device="cuda")
    mbuf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    assert ibuf.data_ptr() % 16 == 0 and mbuf.data_ptr() % 16 == 0
    results = {}
    for io, mo in ((0, 0), (1, 0), (0, 1), (1, 1)):
        I, M = ibuf[io:io + n], mbuf[mo:mo + n]
        I.copy_(torch.from_numpy(img))
        M.copy_(torch.from_numpy(roi.view(np.uint8)))
        assert I.is_contiguous() and M.is_contiguous()
        assert (I.data_ptr() % 16 != 0) == bool(io) and (M.data_ptr() % E != 0) == bool(mo)     # which branch of fo_scan runs
        got = engine.firstorder_stats(I, M, 3.0)
        assert _lib.last_path() == route
        _check(route, (dtype.__name__, n, io, mo), got, ref, k, k_cen)
        results[(io, mo)] = got
        if route == "firstorder-select":              # the queue's scans and glue kernels on the same misaligned pointers
            q = engine.firstorder_stats_queue(I, M, ref["m"], 3.0)
            assert _lib.last_path() == "firstorder-queue" and q[15] == 0
            for j, f in enumerate(engine.FIRSTORDER_FIELDS):
                assert np.array_equal(q[j], got[f], equal_nan=True), ((io, mo), f, q[j], got[f])
            qd = engine.firstorder_stats_queue(I, M, ref["m"], 3.0, deferred=True)
            engine.deferred_status()
            assert np.array_equal(qd, q, equal_nan=True)
    for key, got in results.items():
        for f in got:
            assert np.array_equal(got[f], results[(0, 0)][f], equal_nan=True), (key, f, got[f], results[(0, 0)][f])


# ---- segment mode: selection and cancellation ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", fr.SELECTION)
def test_selection_adversarial(name):
    img, mask, _, _ = fr.case(name)
    ref = fr.case_reference(name)
    assert ref["m"] >= 1 << 20
    xs, m = ref["sorted"], ref["m"]
    vmin, vmax = xs[0], xs[-1]
    scale = fr.BINS / (vmax - vmin)
    bins = np.minimum(((xs[fr.order_ranks(m)] - vmin) * scale).astype(np.int64), fr.BINS - 1)     # fo_bin
    if name == "sel-ten-bins":
        assert len(set(bins.tolist())) == 10 and all(bins[2 * k + 1] == bins[2 * k] + 1 for k in range(5))
    if name == "sel-one-bin":
        assert len(set(bins.tolist())) == 1
    if name == "sel-vmax":
        assert bins[-1] == fr.BINS - 1 and xs[fr.order_ranks(m)[-1]] == vmax
    if name == "sel-ties":
        r = fr.order_ranks(m)
        assert all(xs[r[2 * k]] != xs[r[2 * k + 1]] and xs[r[2 * k] - 1] == xs[r[2 * k]] for k in range(5))
    if name.startswith("sel-outlier"):
        assert int(np.sum(bins == 0)) == 10 and int(np.sum(xs < xs[0] + 1 / scale)) > 1 << 22     # bin 0 exceeds the gather
    if name == "sel-zeros-subnormals":
        assert np.signbit(img[mask][img[mask] == 0]).any() and (~np.signbit(img[mask][img[mask] == 0])).any()
        assert (np.abs(img[mask][img[mask] != 0]) < np.finfo(np.float32).tiny).any()
    _run_case(name)


@pytest.mark.parametrize("name", fr.CANCELLATION)
def test_cancellation(name, monkeypatch):
    _run_case(name)
    if name.startswith("can-i32"):
        monkeypatch.setenv("PRAD_FO_NO_EXACT", "1")
        _run_case(name, "firstorder-select")


# ---- queue route ---------------------------------------------------------------------------------------------------------
FLOAT_CASES = ["b20-sort-f64", "b20-select-f64", "b20-sort-f32", "b20-select-f32", "const-f64", "const-f32", "sel-edges",
               "sel-ulp", "sel-vmax", "sel-ten-bins", "sel-one-bin", "sel-ties", "sel-outlier-many", "sel-outlier-single",
               "sel-zeros-subnormals", "can-f64-1e8", "can-f32-2p24", "can-shift", "can-two-valued-f64"]


def _queue_verdict(ref):
    """what fo_glue_sums_kernel / fo_glue_select_kernel decide: 2 constant ROI, 8 the selected bins exceed the gather
    capacity max(PRAD_FO_QUEUE_CAP = 2^18, roi_count / 2) of prad_firstorder_queue_dev (prad_firstorder.hip)"""
    xs, m = ref["sorted"], ref["m"]
    if not xs[-1] > xs[0]:
        return 2
    scale = fr.BINS / (xs[-1] - xs[0])
    allb = np.minimum(((xs - xs[0]) * scale).astype(np.int64), fr.BINS - 1)
    sel = np.unique(allb[fr.order_ranks(m)])
    total = int(np.isin(allb, sel).sum())
    return 8 if total > max(1 << 18, m // 2) else 0


@pytest.mark.parametrize("name", FLOAT_CASES)
def test_queue_route_equals_the_synchronous_one(name):
    from pyradiomics_amd import _lib, engine
    assert fr.case(name)[0].dtype.kind == "f"
    _, _, shift, _ = fr.case(name)
    ref = fr.case_reference(name)
    I, M = _tensors(name)
    m = ref["m"]
    if m < 1 << 20:                                  # declined up front
        with pytest.raises(NotImplementedError):
            engine.firstorder_stats_queue(I, M, m, shift)
        return
    verdict = _queue_verdict(ref)
    if verdict:
        with pytest.raises(NotImplementedError):
            engine.firstorder_stats_queue(I, M, m, shift)
        v = engine.firstorder_stats_queue(I, M, m, shift, deferred=True)
        engine.deferred_status()
        assert int(v[15]) & verdict, (name, v[15])
        return
    want = engine.firstorder_stats(I, M, shift)
    got = engine.firstorder_stats_queue(I, M, m, shift)
    assert _lib.last_path() == "firstorder-queue"
    assert got[15] == 0
    for k, f in enumerate(engine.FIRSTORDER_FIELDS):
        assert np.array_equal(got[k], want[f], equal_nan=True), (name, f, got[k], want[f])
    q = engine.firstorder_stats_queue(I, M, m, shift, deferred=True)
    engine.deferred_status()
    assert np.array_equal(q, got, equal_nan=True)
    _check("firstorder-queue", name, dict(zip(engine.FIRSTORDER_FIELDS, (float(x) for x in got[:15]))), ref, *fr.case_k(name))


def test_queue_accepts_some_and_declines_some():
    verdicts = {n: _queue_verdict(fr.case_reference(n)) for n in FLOAT_CASES if fr.case_reference(n)["m"] >= 1 << 20}
    assert sum(v == 0 for v in verdicts.values()) >= 5 and 2 in verdicts.values() and 8 in verdicts.values(), verdicts


# ---- through the class ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("name", ["can-f64-1e8", "can-f32-2p24", "can-shift"])
def test_through_the_class(name, resident):
    from pyradiomics_amd import _lib, backend, cmatrices, firstorder
    backend.set(cmatrices)
    img, mask, shift, _ = fr.case(name)
    ref = fr.case_reference(name)
    v = ref["values"]
    b = fr.seg_bounds(ref, *fr.case_k(name))
    got = firstorder.RadiomicsFirstOrder(np.array(img), mask.astype(np.int32), binWidth=25, voxelArrayShift=shift,
                                         deviceResident=resident).execute()
    assert _lib.last_path() == "firstorder-sort"
    d = fr.derived_bounds(v, b)
    m2s = v["m2"] if v["m2"] else 1.0
    want = {"Skewness": (v["m3"] / m2s ** 1.5, d["Skewness"]), "Kurtosis": (v["m4"] / m2s ** 2, d["Kurtosis"]),
            "Variance": (v["m2"], d["Variance"]), "RootMeanSquared": (math.sqrt(v["Energy"] / v["Np"]), d["RootMeanSquared"]),
            "RobustMeanAbsoluteDeviation": (v["rMAD"], b["rMAD"]), "Mean": (v["Mean"], b["Mean"]),
            "Energy": (v["Energy"], b["Energy"]), "MeanAbsoluteDeviation": (v["MAD"], b["MAD"]),
            "Minimum": (v["Minimum"], 0.0), "Maximum": (v["Maximum"], 0.0), "Median": (v["Median"], 0.0),
            "10Percentile": (v["P10"], 0.0), "90Percentile": (v["P90"], 0.0),
            "InterquartileRange": (v["P75"] - v["P25"], 0.0), "Range": (v["Maximum"] - v["Minimum"], 0.0)}
    for f, (w, bd) in want.items():
        g = float(np.asarray(got[f]).ravel()[0])
        err = abs(g - w)
        if bd > 0:
            _note("class", {f: err / bd})
        assert err <= bd, (name, resident, f, g, w, err, bd)


# ---- voxel mode ----------------------------------------------------------------------------------------------------------
def _roi_all(shape, rng):
    return rng.random(shape) < 0.75


def _roi_plane(shape, rng):
    m = np.zeros(shape, dtype=bool)
    m[shape[0] // 2] = rng.random(shape[1:]) < 0.8
    return m


def _roi_line(shape, rng):
    m = np.zeros(shape, dtype=bool)
    m[shape[0] // 2, shape[1] // 2] = True
    return m


def _roi_one(shape, rng):
    m = np.zeros(shape, dtype=bool)
    m[tuple(s // 2 for s in shape)] = True
    return m


def _roi_sparse(shape, rng):
    return rng.random(shape) < 0.06


# (label, shape, ROI, radius, force2D, maskedKernel, window voxels, P)
VOXEL_CONFIGS = [
    ("w1", (3, 4, 5), _roi_one, 1, False, True, 1, 2),
    ("w3", (3, 4, 7), _roi_line, 1, False, True, 3, 4),
    ("w3-unmasked", (1, 1, 13), _roi_all, 1, False, False, 3, 4),
    ("w9", (4, 6, 7), _roi_plane, 1, False, True, 9, 16),
    ("w25-unmasked", (1, 6, 7), _roi_all, 2, False, False, 25, 32),
    ("w25", (3, 7, 8), _roi_all, 2, True, True, 25, 32),
    ("w27", (5, 6, 7), _roi_all, 1, False, True, 27, 32),
    ("w27-unmasked", (5, 6, 7), _roi_all, 1, False, False, 27, 32),
    ("w27-sparse", (6, 7, 8), _roi_sparse, 1, False, True, 27, 32),
    ("w49", (2, 9, 10), _roi_all, 3, True, True, 49, 64),
    ("w125", (6, 7, 8), _roi_all, 2, False, True, 125, 128),
    ("w343", (9, 11, 13), _roi_all, 3, False, True, 343, 512),
]
CONTENTS = ("i16-own", "i16-one", "f64-own", "f64-one", "ties", "equal")


def _content(kind, shape, rng):
    """(image, binWidth): -own puts every voxel into its own grey level, -one the whole image into one level"""
    n = int(np.prod(shape))
    if kind.startswith("i16"):
        return (rng.permutation(n) * 3 + 3).astype(np.int16).reshape(shape), 3 if kind.endswith("own") else 8000
    if kind == "f64-own":
        return (rng.permutation(n) * 0.5 + 0.25 - 0.25 * n).reshape(shape), 0.5
    if kind == "f64-one":
        return rng.standard_normal(shape) * 37.5 + 11, 10 ** 6
    if kind == "ties":
        return (rng.integers(-2, 3, shape) * 7).astype(np.int16), 1
    return np.full(shape, 7.5), 25


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("cfg", VOXEL_CONFIGS, ids=[c[0] for c in VOXEL_CONFIGS])
def test_voxel_mode(cfg, kind):
    from pyradiomics_amd import _lib, backend, cmatrices, firstorder, imageoperations
    label, shape, roi_fn, radius, force2D, masked, nk_want, P_want = cfg
    rng = np.random.default_rng(sum(map(ord, label + kind)))
    img, bw = _content(kind, shape, rng)
    roi = roi_fn(shape, rng)
    shift = 17.0
    batch = next(b for b in (7, 5, 3, 11) if roi.sum() % b)            # does not divide the number of centres
    backend.set(cmatrices)
    fc = firstorder.RadiomicsFirstOrder(img, roi.astype(np.int32), binWidth=bw, voxelBased=True, kernelRadius=radius,
                                        force2D=force2D, force2Ddimension=0, maskedKernel=masked, voxelArrayShift=shift,
                                        voxelBatch=batch, initValue=np.nan)
    fc.enableAllFeatures()
    fc.enableFeatureByName("StandardDeviation")
    res = {k: np.asarray(v.array) for k, v in fc.execute().items()}
    assert _lib.last_path() == "voxel-firstorder"
    assert set(res) == set(fr.VOXEL_FEATURES)
    spacing_volume = float(np.multiply.reduce(fc.pixelSpacing))
    bb = (np.array([np.ptp(c) + 1 for c in np.nonzero(roi)]) if masked else np.array(shape))
    half = fr.window_half(shape, np.minimum(bb, 2 * radius + 1), radius, force2D, 0)
    nk = int(np.prod([2 * h + 1 for h in half]))
    assert nk == nk_want and max(2, 1 << (nk - 1).bit_length()) == P_want
    seen = roi if masked else np.ones(shape, dtype=bool)          # unmasked kernels bin and count over the whole image
    levels, _ = imageoperations.binImage(img, seen, binWidth=bw)
    k = math.ceil(nk / 64) + 6
    for f in fr.VOXEL_FEATURES:
        assert np.array_equal(np.isnan(res[f][~roi]), np.ones(int((~roi).sum()), dtype=bool)), f
    sizes = set()
    for c in zip(*np.nonzero(roi)):
        want, st = fr.voxel_reference(img, seen, levels, c, half, shift, spacing_volume)
        got = {f: float(res[f][c]) for f in fr.VOXEL_FEATURES}
        bad, ratios = fr.compare(got, want, fr.voxel_bounds(want, st, k, spacing_volume), exact=fr.VOXEL_EXACT)
        _note("voxel", ratios)
        assert not bad, (label, kind, c, st["m"], bad)
        sizes.add(st["m"])
        if st["m"] == 1:
            x = float(img[c])
            assert got["Range"] == 0 and got["Skewness"] == 0 and got["Kurtosis"] == 0
            assert got["10Percentile"] == got["90Percentile"] == got["Median"] == got["Minimum"] == got["Maximum"] == x
        if kind == "equal":
            assert got["Skewness"] == 0 and got["Kurtosis"] == 0 and got["Variance"] == 0 and got["Range"] == 0
    if label == "w27-sparse":
        assert {1, 2} <= sizes
    if label == "w27-unmasked":
        assert {8, 12, 18, 27} <= sizes                # windows cut at a corner, an edge, a face, and whole ones


def test_zz_report():
    print()
    for (route, f), r in sorted(RATIOS.items()):
        print("    %-18s %-28s %.3g" % (route, f, r))
    assert all(r <= 1 for r in RATIOS.values())

"""GPU: the segment-mode formula kernels (glcm_matrix_features_kernel, zone_matrix_features_kernel,
ngtdm_matrix_features_kernel, the segment MCC, glszm_rank_kernel + the one-queue GLSZM route) at the limits of what their
entry points accept, against tests/feature_reference.py (long double, pinned to the reference's recorded values by
tests/test_feature_reference.py).  Everything goes through pyradiomics_amd.engine on synthetic device matrices / constructed
volumes, so the expected value depends on the restatement alone; route equalities (strided = contiguous, deferred =
synchronous, one queue = three calls) are additional, bit-exact checks.

Tolerances.  A plain sum F = sum t must satisfy |F_gpu - F_ref| <= c * 2^-53 * A, A = sum |t| from the restatement.  c is the
number of roundings one value can pass through in the kernel (derivations next to the c_* functions below):
  * the longest chain of additions of one lane, ceil(n_terms / 256) (PRAD_FEAT_THREADS lanes stride over the terms),
  * 6 + 2 steps of the shuffle and wave trees (TREE),
  * at most 8 roundings inside one term (TERM: the division by the total, up to four products / powers, log2 and its argument),
  * for sums over a GLCM marginal, the serial build of that marginal: one division and one addition per element of the
    row / column / diagonal, at most Ng + 1 of them.
The zone-matrix marginals are sums of integer counts below 2^53 and therefore exact.  Moments about a mean add
D * bound(mean) (D = sum |dt / d mean|), derived features propagate their components' bounds to first order
(feature_reference.glcm_bounds / zone_bounds / ngtdm_bounds) and the tests assert in long double that their divisors are
at least COND = 1000 times their own error bound.  Imc2 on an exactly independent matrix is rounding noise in any float64
evaluation (HXY2 - HXY is 0 in exact arithmetic): only NaN or |value| <= sqrt(2 bound(HXY2 - HXY)) is asserted there.
Flags, NaN placement, accepted / declined, verdict bits, the special-case values and the route equalities are exact.

Fairness of the bound: every comparison also evaluates the same restatement in float64 numpy and records
err_numpy / bound next to err_gpu / bound; test_zz_report prints the worst ratios of the run.

Worst err / bound over all cases of this module (kernel figures measured on an MI355X with the kernels of commit 9062245,
which this module leaves unchanged; the float64-numpy figures are the same on any x86 host):
    kernel family   GPU kernel (feature)                  float64 numpy (feature)
    glcm            0.25   (Imc2)                         0.25  (Imc2)
    zone            0.174  (SmallEmphasis)                0.297 (SmallEmphasis)
    ngtdm           0.084  (Complexity)                   0.086 (Coarseness)
    glszm routes    0.100  (SmallLowGrayLevelEmphasis)    -
    mcc             0.0011 (MCC)                          -
So the kernels meet the derived c everywhere, 1535 levels, 6000 columns and 4096 large zones included, and the bound is
neither vacuous (ratios within a factor 4 to 10 of it) nor unfair to float64.

Sharpness: one-line mutations of a scratch copy of the kernels, loaded through PRAD_LIB, and the tests that failed on them:
    stride 255 in the loop over p_{x-y} (DifferenceAverage .. InverseVariance)
        test_glcm_features_over_matrix_sizes[Ng >= 256], test_glcm_features_over_contents[300-*], test_glcm_special_cases_are_exact
    `k >= 1` dropped from InverseVariance
        every test_glcm_features_over_* case, test_glcm_special_cases_are_exact
    p_{x+y} loop one term short (i < min(k, Ng - 1))
        every test_glcm_features_over_* case, test_glcm_special_cases_are_exact
    sj used for si in P(i, j)
        test_zone_features_over_shapes_and_size_tables (33 of 36), test_zone_features_over_contents,
        test_zone_features_on_strided_views_equal_the_contiguous_copy
    jvals[j] replaced by j + 1
        test_zone_features_over_shapes_and_size_tables[*-gaps / *-sizes], test_zone_features_over_contents,
        test_zone_features_on_strided_views_equal_the_contiguous_copy
    size value of the large columns written as key[i] + 1 in glszm_rank_kernel
        test_glszm_sizes_at_the_bitmap_boundary, test_glszm_large_zone_deduplication_in_chunks[1023 / 1024 / 1025 / 2500],
        test_glszm_large_zone_list_at_its_capacity[4096]
"""
import math

import numpy as np
import pytest

import feature_reference as fr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
THREADS = 256          # PRAD_FEAT_THREADS
TREE = 6 + 2           # __shfl_xor tree of a wave (6 steps) + pairwise tree over the 4 wave results (2 steps)
TERM = 8               # roundings inside one term, see the module docstring
COND = 1000.0          # a divisor of a derived feature is at least this many times its own error bound

RATIOS = {}            # (kernel, feature) -> [worst err_gpu / bound, worst err_numpy / bound]


def c_glcm_entry(Ng):
    """sums over the Ng^2 entries: lane t adds entries t, t + 256, ...: ceil(Ng^2 / 256) additions, then the trees"""
    return math.ceil(Ng * Ng / THREADS) + TREE + TERM


def c_glcm_marginal(Ng):
    """sums over a marginal (at most 2 Ng - 1 values of k): every marginal value was itself built serially from at most Ng
    quotients C / tot (Ng divisions and additions: relative error (Ng + 1) u), then ceil((2 Ng - 1) / 256) additions, trees"""
    return (Ng + 1) + math.ceil((2 * Ng - 1) / THREADS) + TREE + TERM


def c_zone_marginal(Ni, Nj):
    """sums over the (exact) row / column sums: ceil(max(Ni, Nj) / 256) additions of one lane, trees, term"""
    return math.ceil(max(Ni, Nj) / THREADS) + TREE + TERM


def c_zone_entry(Ni, Nj):
    return math.ceil(Ni * Nj / THREADS) + TREE + TERM


def c_ngtdm(n_terms):
    return math.ceil(n_terms / THREADS) + TREE + TERM


def _note(kernel, name, err_gpu, err_np, bound):
    if bound > 0:
        r = RATIOS.setdefault((kernel, name), [0.0, 0.0])
        r[0], r[1] = max(r[0], err_gpu / bound), max(r[1], err_np / bound)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def _to(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


# ---- GLCM ---------------------------------------------------------------------------------------------------------------
def _check_glcm(dev, counts, symmetric, label, independent=()):
    """counts [Ng, Ng, Na] (integers): every value of every angle against the restatement within the derived bound"""
    from pyradiomics_amd import engine
    Ng, _, Na = counts.shape
    assert counts.sum(axis=(0, 1)).max() * 2 < 2.0 ** 53          # the total is exact in float64
    got, empty = engine.glcm_features(_to(dev, counts), symmetric)
    assert got.shape == (Na, 23) and empty.shape == (Na,)
    ce, cm = c_glcm_entry(Ng), c_glcm_marginal(Ng)
    for a in range(Na):
        ref = fr.glcm_angle(counts[:, :, a], symmetric)
        assert bool(empty[a]) == ref["empty"], (label, a)
        if ref["empty"]:
            assert np.isnan(got[a]).all(), (label, a)
            continue
        lo = fr.glcm_angle(counts[:, :, a], symmetric, dtype=np.float64)
        B, cond = fr.glcm_bounds(ref, ce, cm)
        single = np.count_nonzero(ref["p"]) == 1          # one level pair (i, i): the reference's special values, exactly
        for k, n in enumerate(fr.GLCM_NAMES):
            want = float(ref["values"][n])
            if single and n in fr.GLCM_DERIVED:
                assert got[a, k] == want == {"Correlation": 1, "Imc1": 0, "Imc2": 0}[n], (label, a, n, got[a, k], want)
                continue
            if n == "Imc2" and a in independent:
                lim = math.sqrt(2 * B["HXY2-HXY"])
                assert np.isnan(got[a, k]) or abs(got[a, k]) <= lim, (label, a, n, got[a, k], lim)
                continue
            if n in cond:
                assert cond[n] >= COND, (label, a, n, "ill conditioned input: fix the test case", cond[n])
            err = abs(got[a, k] - want)
            _note("glcm", n, err, abs(float(lo["values"][n]) - want), B[n])
            assert err <= B[n], (label, "angle %d" % a, n, got[a, k], want, err, B[n])
    return got, empty


def _dense(rng, Ng, hi=1000):
    return rng.integers(1, hi, size=(Ng, Ng)).astype(np.float64)


def _sparse(rng, Ng, frac=0.01):
    m = rng.random((Ng, Ng)) < frac
    m[rng.integers(0, Ng), rng.integers(0, Ng)] = True
    if Ng > 1:
        m[0, Ng - 1] = m[Ng - 1, 0] = True          # keeps sigma and the entropies away from zero
    return m * rng.integers(1, 50, size=(Ng, Ng)).astype(np.float64)


def _band(rng, Ng):
    i, j = np.indices((Ng, Ng))
    return (np.abs(i - j) <= 1) * rng.integers(1, 1000, size=(Ng, Ng)).astype(np.float64)


GLCM_SIZES = [1, 2, 3, 63, 64, 65, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1024, 1535]


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "nonsym"])
@pytest.mark.parametrize("Ng", GLCM_SIZES)
def test_glcm_features_over_matrix_sizes(dev, Ng, symmetric):
    """dense / all-zero / sparse / band angles at every size from 1 to the LDS bound (1535): second trips of the strided
    loops (Ng > 256, 2 Ng - 1 > 256 from 129), the diagonal loop bounds, the empty angle in the middle"""
    rng = np.random.default_rng(1000 + Ng)
    C = np.zeros((Ng, Ng, 4))
    C[:, :, 0] = _dense(rng, Ng)
    C[:, :, 2] = _sparse(rng, Ng)
    C[:, :, 3] = _band(rng, Ng)
    if Ng == 1:
        got, empty = _check_glcm(dev, C, symmetric, "Ng=1")
        for a in (0, 2, 3):       # a single level: the special cases, exactly
            assert got[a, 6] == 1 and got[a, 12] == 0 and got[a, 13] == 0 and got[a, 19] == 1
        return
    if Ng == 2:
        C[:, :, 2] = [[3, 1], [2, 5]]
    _check_glcm(dev, C, symmetric, "Ng=%d" % Ng)


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "nonsym"])
@pytest.mark.parametrize("Ng", [129, 300])
def test_glcm_features_over_contents(dev, Ng, symmetric):
    rng = np.random.default_rng(7 + Ng)
    i, j = np.indices((Ng, Ng))
    mats = {}
    mats["diagonal"] = (i == j) * rng.integers(1, 100, size=(Ng, Ng))
    mats["antidiagonal"] = (i + j == Ng - 1) * rng.integers(1, 100, size=(Ng, Ng))
    corners = np.zeros((Ng, Ng))
    corners[0, 0], corners[0, Ng - 1], corners[Ng - 1, 0], corners[Ng - 1, Ng - 1] = 3, 5, 7, 11
    mats["corners"] = corners
    row = np.zeros((Ng, Ng))
    row[Ng // 3, :2 ** int(math.log2(Ng))] = 1        # (a power of two of equal counts: p, ux and sigma_x = 0 are exact in any order)
    mats["one_row"] = row
    mats["band"] = _band(rng, Ng)
    gaps = _dense(rng, Ng)
    absent = np.r_[0:5, Ng // 2 - 10:Ng // 2 + 10, Ng - 7:Ng]
    gaps[absent, :] = 0
    gaps[:, absent] = 0
    mats["absent_levels"] = gaps
    mats["ones"] = (rng.random((Ng, Ng)) < 0.3) * 1.0 + corners.clip(0, 1)
    mats["near_1e9"] = rng.integers(999_000_000, 1_000_000_000, size=(Ng, Ng))
    asym = _dense(rng, Ng) * (j > 2 * i) + (rng.random((Ng, Ng)) < 0.02) * 3.0
    mats["asymmetric"] = asym
    mats["zero_a"] = np.zeros((Ng, Ng))
    names = ["zero_a"] + [n for n in mats if n != "zero_a"] + ["zero_a"]        # an empty angle first and last
    if symmetric:
        names.remove("one_row")          # symmetrised it is a row and a column: covered by the non-symmetric run
    C = np.stack([np.asarray(mats[n], dtype=np.float64) for n in names], axis=2)
    if not symmetric:
        assert not np.allclose(asym.sum(0), asym.sum(1))          # px != py
        C = C[:, :, [k for k, n in enumerate(names) if n != "one_row"]]
    got, empty = _check_glcm(dev, C, symmetric, "contents Ng=%d" % Ng)
    assert empty[0] and empty[-1] and not empty[1:-1].any()


def test_glcm_special_cases_are_exact(dev):
    from pyradiomics_amd import engine
    Ng = 300
    rng = np.random.default_rng(3)
    C = np.zeros((Ng, Ng, 4))
    C[200, 200, 0] = 9                                   # a single level
    C[Ng // 3, :256, 1] = 1                              # one row, not symmetrised: sigma_x = 0 (256 equal counts: exactly)
    px, py = rng.integers(1, 20, size=Ng).astype(np.float64), rng.integers(1, 20, size=Ng).astype(np.float64)
    C[:, :, 2] = np.outer(px, py)                        # exactly independent
    C[:, :, 3] = _dense(rng, Ng)
    got, empty = engine.glcm_features(_to(dev, C), False)
    N = fr.GLCM_NAMES.index
    assert not empty.any()
    assert got[0, N("Correlation")] == 1 and got[0, N("Imc1")] == 0 and got[0, N("Imc2")] == 0
    assert got[0, N("MaximumProbability")] == 1 and got[0, N("JointAverage")] == 201 and got[0, N("Contrast")] == 0
    assert got[1, N("Correlation")] == 1 and got[1, N("SumSquares")] == 0          # sigma_x = 0 -> 1 (the reference's rule)
    ref = fr.glcm_angle(C[:, :, 1], False)
    assert ref["values"]["Correlation"] == 1
    # independent matrix: Correlation and Imc1 are 0 up to their bounds, Imc2 is NaN or noise below sqrt(2 bound(HXY2 - HXY))
    _check_glcm(dev, C[:, :, 1:], False, "special", independent=(1,))
    assert abs(got[2, N("Correlation")]) < 1e-9 and abs(got[2, N("Imc1")]) < 1e-9


@pytest.mark.parametrize("Na,zero", [(1, ()), (4, (0,)), (13, (12,)), (13, (5, 6)), (62, (0, 30, 61))])
def test_glcm_features_over_angle_counts_with_empty_angles(dev, Na, zero):
    """62 angles = distances [1, 2]; all-zero angles first / last / in the middle are NaN with their flag set and leave
    their neighbours alone"""
    Ng = 65
    rng = np.random.default_rng(Na)
    C = rng.integers(0, 30, size=(Ng, Ng, Na)).astype(np.float64)
    C[:, :, list(zero)] = 0
    got, empty = _check_glcm(dev, C, True, "Na=%d" % Na)
    assert sorted(np.where(empty)[0]) == sorted(zero)
    full = rng.integers(0, 30, size=(Ng, Ng, Na)).astype(np.float64)
    full[:, :, [a for a in range(Na) if a not in zero]] = C[:, :, [a for a in range(Na) if a not in zero]]
    from pyradiomics_amd import engine
    got2, _ = engine.glcm_features(_to(dev, full), True)
    keep = ~empty
    assert np.array_equal(got[keep], got2[keep])


def _line_image(n_levels, rng):
    """a 1 x 1 x n image holding every level 1 .. n once, permuted: (Image, mask Image, level array)"""
    from pyradiomics_amd.image import Image
    lev = rng.permutation(n_levels) + 1
    arr = lev.astype(np.float64).reshape(1, 1, -1) - 0.5          # binWidth 1 from a minimum of 0.5: level = value + 0.5
    return Image(arr, spacing=(1.0, 1.0, 1.0)), Image(np.ones(arr.shape, dtype=np.int32), spacing=(1.0, 1.0, 1.0)), lev


@pytest.mark.parametrize("Ng", [1535, 1536])
def test_glcm_one_past_the_lds_bound_is_declined_and_the_host_route_answers(dev, Ng):
    from pyradiomics_amd import backend, cmatrices, engine
    rng = np.random.default_rng(Ng)
    C = np.zeros((Ng, Ng, 1))
    C[:, :, 0] = _sparse(rng, Ng, 0.002)
    if Ng == 1535:
        _check_glcm(dev, C, True, "Ng=1535 accepted")
        return
    with pytest.raises(NotImplementedError):
        engine.glcm_features(_to(dev, C), True)
    # the class on an image of 1536 levels, fusedSegment left on: the host route answers with the values of the restatement
    from pyradiomics_amd.glcm import RadiomicsGLCM
    image, mask, lev = _line_image(Ng, rng)
    calls = []
    real = engine.glcm_features
    backend.set(cmatrices)
    try:
        engine.glcm_features = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        fc = RadiomicsGLCM(image, mask, binWidth=1)
        for n in ("Contrast", "JointEntropy", "Correlation", "Idm", "SumAverage", "ClusterShade"):
            fc.enableFeatureByName(n)
        vals = fc.execute()
    finally:
        engine.glcm_features = real
        backend.set(None)
    assert fc.coefficients["Ng"] == Ng and calls, "the fused route was tried and declined"
    raw = np.zeros((Ng, Ng, 1))
    np.add.at(raw[:, :, 0], (lev[:-1] - 1, lev[1:] - 1), 1)
    ref = fr.glcm_angle(raw[:, :, 0], True)
    B, _ = fr.glcm_bounds(ref, Ng + 34, Ng + 34)          # (numpy on the host: c_ref of tests/test_feature_reference.py)
    for n, v in vals.items():
        assert abs(float(v) - float(ref["values"][n])) <= B[n], (n, v, ref["values"][n], B[n])


# ---- zone matrices (GLRLM / GLSZM / GLDM formulas) ------------------------------------------------------------------------
def _check_zone(dev, P, jvals, label, P_dev=None):
    """P numpy [Ni, Nj(, Na)] integer counts; P_dev: the (possibly strided) device view holding the same values"""
    from pyradiomics_amd import engine
    P3 = P if P.ndim == 3 else P[:, :, None]
    Ni, Nj, Na = P3.shape
    assert P3.sum() < 2.0 ** 53
    got, empty = engine.zone_matrix_features(_to(dev, P) if P_dev is None else P_dev, jvals)
    assert got.shape == (Na, 16)
    cm, ce = c_zone_marginal(Ni, Nj), c_zone_entry(Ni, Nj)
    for a in range(Na):
        ref = fr.zone_angle(P3[:, :, a], jvals)
        assert bool(empty[a]) == ref["empty"], (label, a)
        if ref["empty"]:
            assert np.isnan(got[a]).all(), (label, a)
            continue
        lo = fr.zone_angle(P3[:, :, a], jvals, dtype=np.float64)
        B = fr.zone_bounds(ref, cm, ce)
        for k, n in enumerate(fr.ZONE_NAMES):
            want = float(ref["values"][n])
            err = abs(got[a, k] - want)
            _note("zone", n, err, abs(float(lo["values"][n]) - want), B[n])
            assert err <= B[n], (label, "angle %d" % a, n, got[a, k], want, err, B[n])
    return got, empty


def _jvals(kind, Nj, rng):
    if kind == "index":
        return np.arange(1, Nj + 1, dtype=np.float64)
    if kind == "gaps":
        return np.cumsum(rng.integers(1, 4, size=Nj)).astype(np.float64)
    v = np.unique(np.r_[np.arange(1, Nj // 2 + 1), rng.integers(Nj, 130_000_000, size=Nj)])[:Nj - 1]
    return np.r_[v, 130_000_001].astype(np.float64)[:Nj] if len(v) >= Nj - 1 else None       # GLSZM-like, up to 1.3e8


@pytest.mark.parametrize("kind", ["index", "gaps", "sizes"])
@pytest.mark.parametrize("Ni,Nj,Na", [(1, 1, 1), (2, 63, 1), (7, 64, 13), (8, 65, 1), (9, 255, 13), (33, 256, 62), (255, 257, 1),
                                      (300, 1000, 13), (2000, 63, 1), (9, 6000, 1), (300, 6000, 1), (2000, 1000, 1)])
def test_zone_features_over_shapes_and_size_tables(dev, Ni, Nj, Na, kind):
    rng = np.random.default_rng(Ni * 7 + Nj)
    jv = _jvals(kind, Nj, rng)
    if jv is None or len(jv) != Nj:
        jv = np.r_[np.arange(1, Nj), 130_000_001].astype(np.float64)
    assert len(jv) == Nj and (np.diff(jv) > 0).all()
    P = rng.integers(0, 40, size=(Ni, Nj, Na)).astype(np.float64)
    if Na >= 4:
        P[:, :, 0] = 0
        P[:, :, Na - 1] = 0
        P[:, :, Na // 2] = 0
        P[:, :, 1] *= rng.random((Ni, Nj)) < 0.01           # sparse
        P[Ni // 2, Nj // 2, 1] += 1
    got, empty = _check_zone(dev, P, jv, "zone %dx%dx%d %s" % (Ni, Nj, Na, kind))
    if Na >= 4:
        assert sorted(np.where(empty)[0]) == sorted({0, Na // 2, Na - 1})


def test_zone_features_over_contents(dev):
    rng = np.random.default_rng(21)
    Ni, Nj = 33, 300
    jv = _jvals("gaps", Nj, rng)
    mats = []
    one = np.zeros((Ni, Nj))
    one[4, 17] = 6
    mats.append(one)                                           # a single non-zero entry
    gaps = rng.integers(0, 9, size=(Ni, Nj)).astype(np.float64)
    gaps[[0, 5, 6, Ni - 1]] = 0
    gaps[:, [0, 1, 100, Nj - 1]] = 0
    mats.append(gaps)                                          # empty rows and columns
    col = np.zeros((Ni, Nj))
    col[:, 257] = rng.integers(1, 9, size=Ni)
    mats.append(col)                                           # one column only
    row = np.zeros((Ni, Nj))
    row[8] = rng.integers(1, 9, size=Nj)
    mats.append(row)                                           # one row only
    P = np.stack(mats, axis=2)
    got, _ = _check_zone(dev, P, jv, "zone contents")
    N = fr.ZONE_NAMES.index
    j = jv[17]
    assert got[0, N("SmallEmphasis")] == 1 / (j * j) and got[0, N("LargeEmphasis")] == j * j
    assert got[0, N("Percentage")] == 1 / j and got[0, N("GrayLevelVariance")] == 0 and got[0, N("SizeVariance")] == 0
    assert got[0, N("HighGrayLevelEmphasis")] == 25 and got[0, N("LargeHighGrayLevelEmphasis")] == 25 * j * j
    assert got[0, N("GrayLevelNonUniformityNormalized")] == 1 and abs(got[0, N("Entropy")]) < 1e-15


def test_zone_features_on_strided_views_equal_the_contiguous_copy(dev):
    from pyradiomics_amd import engine
    rng = np.random.default_rng(33)
    Ni, Nj, Na = 34, 520, 16
    jv_all = _jvals("gaps", Nj, rng)
    base = rng.integers(0, 40, size=(Ni, Nj, Na)).astype(np.float64)
    T = _to(dev, base)
    views = {
        "2d": (T[:, :, 0], base[:, :, 0], jv_all),
        "angle_major": (_to(dev, base.transpose(2, 0, 1)).permute(1, 2, 0), base, jv_all),
        "every_other_column": (T[:, ::2, :], base[:, ::2, :], jv_all[::2]),
        "offset_rows_angles": (T[1:, :, 3:], base[1:, :, 3:], jv_all),
        "all_three": (T[::3, 5::7, 1::2], base[::3, 5::7, 1::2], jv_all[5::7]),
    }
    for name, (view, arr, jv) in views.items():
        if name != "2d":
            assert not view.is_contiguous()
        got, empty = _check_zone(dev, np.ascontiguousarray(arr), jv, "view " + name, P_dev=view)
        want, wempty = engine.zone_matrix_features(view.contiguous(), jv)
        assert np.array_equal(got, want) and np.array_equal(empty, wempty), name


def test_deferred_results_equal_the_synchronous_ones_bit_for_bit(dev):
    from pyradiomics_amd import engine
    rng = np.random.default_rng(41)
    G = _to(dev, rng.integers(0, 30, size=(300, 300, 13)))
    Z = _to(dev, rng.integers(0, 30, size=(33, 700, 13)))
    jv = _jvals("gaps", 700, rng)
    N = np.c_[rng.integers(0, 50, size=300), rng.random(300) * 40, np.arange(1, 301)].astype(np.float64)
    Nd = _to(dev, N)
    a1, a2, a3 = engine.glcm_features(G, True), engine.zone_matrix_features(Z, jv), engine.ngtdm_features(Nd)
    b1, b2, b3 = (engine.glcm_features(G, True, deferred=True), engine.zone_matrix_features(Z, jv, deferred=True),
                  engine.ngtdm_features(Nd, deferred=True))
    engine.deferred_status()
    assert np.array_equal(a1[0], b1[0], equal_nan=True) and np.array_equal(a1[1], b1[1] != 0)
    assert np.array_equal(a2[0], b2[0], equal_nan=True) and np.array_equal(a2[1], b2[1] != 0)
    assert np.array_equal(a3, b3)


# ---- NGTDM ------------------------------------------------------------------------------------------------------------------
def _check_ngtdm(dev, N, label):
    from pyradiomics_amd import engine
    got = engine.ngtdm_features(_to(dev, N))
    ref, lo = fr.ngtdm_reference(N), fr.ngtdm_reference(N, dtype=np.float64)
    ngp = ref["parts"]["ngp"]
    B, cond = fr.ngtdm_bounds(ref, c_ngtdm(ngp), c_ngtdm(ngp * ngp))
    for n, v in cond.items():
        assert v >= COND, (label, n, v)
    for k, n in enumerate(fr.NGTDM_NAMES):
        want = float(ref["values"][n])
        err = abs(got[k] - want)
        _note("ngtdm", n, err, abs(float(lo["values"][n]) - want), B[n])
        assert err <= B[n], (label, n, got[k], want, err, B[n])
    return got


@pytest.mark.parametrize("present", ["all", "every_third", "one", "two"])
@pytest.mark.parametrize("Ng", [1, 2, 255, 257, 300, 1024, 2558])
def test_ngtdm_features_over_sizes_and_present_levels(dev, Ng, present):
    rng = np.random.default_rng(Ng)
    N = np.zeros((Ng, 3))
    # the level VALUES are not the row index + 1: the kernel has to read the third column
    N[:, 2] = 3 + 2 * np.arange(Ng)
    keep = {"all": np.arange(Ng), "every_third": np.arange(0, Ng, 3), "one": np.array([Ng // 2]),
            "two": np.unique([Ng // 3, Ng - 1])}[present]
    N[keep, 0] = rng.integers(1, 5000, size=len(keep))
    N[:, 1] = rng.random(Ng) * 100          # s_i of absent levels is garbage the kernel must ignore
    got = _check_ngtdm(dev, N, "ngtdm Ng=%d %s" % (Ng, present))
    if len(keep) == 1:
        assert got[1] == 0 and got[2] == 0 and got[4] == 0          # Contrast (one level), Busyness (absdiff = 0), Strength


def test_ngtdm_special_cases_are_exact(dev):
    N = np.zeros((300, 3))
    N[:, 2] = np.arange(1, 301)
    N[::2, 0] = 7                                                      # s_i all zero: a completely homogeneous neighbourhood
    got = _check_ngtdm(dev, N, "s_i = 0")
    assert got[0] == 1e6 and got[2] == 0 and got[4] == 0 and got[1] == 0 and got[3] == 0


@pytest.mark.parametrize("Ng", [2558, 2559])
def test_ngtdm_one_past_the_lds_bound_is_declined_and_the_host_route_answers(dev, Ng):
    from pyradiomics_amd import backend, cmatrices, engine
    rng = np.random.default_rng(Ng)
    N = np.c_[rng.integers(1, 100, size=Ng), rng.random(Ng) * 10, np.arange(1, Ng + 1)].astype(np.float64)
    if Ng == 2558:
        _check_ngtdm(dev, N, "Ng=2558 accepted")
        return
    with pytest.raises(NotImplementedError):
        engine.ngtdm_features(_to(dev, N))
    from pyradiomics_amd.ngtdm import RadiomicsNGTDM
    image, mask, lev = _line_image(Ng, rng)
    calls = []
    real = engine.ngtdm_features
    backend.set(cmatrices)
    try:
        engine.ngtdm_features = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        vals = RadiomicsNGTDM(image, mask, binWidth=1).execute()
    finally:
        engine.ngtdm_features = real
        backend.set(None)
    assert calls, "the fused route was tried and declined"
    # the NGTDM of a line: every voxel has its one or two neighbours along x
    nb = np.zeros(Ng)
    lf = lev.astype(np.float64)
    nb[1:-1] = (lf[:-2] + lf[2:]) / 2
    nb[0], nb[-1] = lf[1], lf[-2]
    M = np.zeros((Ng, 3))
    M[:, 2] = np.arange(1, Ng + 1)
    M[lev - 1, 0] = 1
    M[lev - 1, 1] = np.abs(lf - nb)
    ref = fr.ngtdm_reference(M)
    B, _ = fr.ngtdm_bounds(ref, Ng + 34, Ng + 34)
    for n in fr.NGTDM_NAMES:
        assert abs(float(vals[n]) - float(ref["values"][n])) <= B[n], (n, vals[n], ref["values"][n], B[n])


# ---- segment MCC ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ng", [300, 1024])
@pytest.mark.parametrize("nocc", [64, 65])
def test_segment_mcc_at_64_and_65_occurring_levels(dev, Ng, nocc):
    """64 occurring levels spread over a 300 / 1024-level matrix are accepted and equal the singular-value reference; 65 are
    declined (deferred: the last entry is non-zero); an empty and a single-level angle sit beside them"""
    from pyradiomics_amd import engine
    rng = np.random.default_rng(Ng + nocc)
    occ = np.unique(np.r_[0, Ng - 1, rng.choice(np.arange(1, Ng - 1), size=nocc - 2, replace=False)])
    assert len(occ) == nocc
    C = np.zeros((Ng, Ng, 3))
    # a diagonally dominant matrix: the second singular value is well away from 0
    blk = rng.integers(1, 20, size=(nocc, nocc)).astype(np.float64) + np.diag(rng.integers(200, 400, size=nocc))
    C[np.ix_(occ, occ, [0])] = blk[:, :, None]
    C[occ[3], occ[3], 2] = 5
    G = _to(dev, C)
    if nocc == 65:
        with pytest.raises(NotImplementedError):
            engine.glcm_mcc(G, True)
        out = engine.glcm_mcc(G, True, deferred=True)
        engine.deferred_status()
        assert out[-1] != 0
        return
    for symmetric in (True, False):
        got = engine.glcm_mcc(G, symmetric)
        ref = fr.mcc_reference(C, symmetric)
        assert np.isnan(got[1]) and np.isnan(ref[1][0]) and got[2] == 0 and ref[2][0] == 0
        s2 = ref[0][0]
        assert s2 > 0.1
        # Jacobi on the symmetric M = A A^T (|M| = sigma_1^2 = 1): every eigenvalue to n TERM u |M|; the square root divides
        # by 2 sigma_2; the reference's own singular value carries the same n TERM u
        bound = 2 * nocc * TERM * U * (1 / (2 * s2) + 1)
        _note("mcc", "MCC", abs(got[0] - s2), 0.0, bound)
        assert abs(got[0] - s2) <= bound, (got[0], s2, bound)
        d = engine.glcm_mcc(G, symmetric, deferred=True)
        engine.deferred_status()
        assert d[-1] == 0 and np.array_equal(d[:3], got, equal_nan=True)


# ---- GLSZM: sizes ranked on the device, one queue ---------------------------------------------------------------------------
def _rows_volume(lengths, W):
    """a 1 x R x W image: row y holds one run of lengths[y] voxels of level 2 + y % 2 followed by W - lengths[y] voxels of level
    4 + y % 2.  Rows of equal parity never touch and neighbouring rows share no level, so every run is a zone of its own:
    -> (levels int32 [1, R, W], {(level, size): count})"""
    lengths = np.asarray(lengths)
    R = len(lengths)
    par = (np.arange(R) % 2)[:, None]
    lev = np.where(np.arange(W)[None, :] < lengths[:, None], 2 + par, 4 + par).astype(np.int32)
    zones = {}
    for y_par in (0, 1):
        ls = lengths[y_par::2]
        for size, cnt in zip(*np.unique(ls, return_counts=True)):
            zones[(2 + y_par, int(size))] = zones.get((2 + y_par, int(size)), 0) + int(cnt)
        for size, cnt in zip(*np.unique(W - ls, return_counts=True)):
            if size > 0:
                zones[(4 + y_par, int(size))] = zones.get((4 + y_par, int(size)), 0) + int(cnt)
    return lev[None], zones


def _expected_matrix(zones, Ng):
    sizes = np.array(sorted({s for _, s in zones}))
    P = np.zeros((Ng, len(sizes)))
    for (level, s), cnt in zones.items():
        P[level - 1, np.searchsorted(sizes, s)] = cnt
    return P, sizes


def _check_glszm(dev, lev, zones, Ng, label, accepted=True):
    import torch
    from pyradiomics_amd import cmatrices, engine
    L = torch.from_numpy(lev).to(dev)
    M = torch.ones(lev.shape, dtype=torch.uint8, device=dev)
    Ns = int(lev.size)
    P, sizes = _expected_matrix(zones, Ng)
    assert (P * sizes[None, :]).sum() == Ns                  # the constructed zones tile the volume
    ref = fr.zone_angle(P, sizes)
    B = fr.zone_bounds(ref, c_zone_marginal(Ng, len(sizes)), c_zone_entry(Ng, len(sizes)))
    # the three-call route: compact matrix and sizes are what the construction says
    Pc, sc = engine.glszm_compact(L, M, Ng, Ns)
    assert np.array_equal(sc, sizes) and np.array_equal(Pc.cpu().numpy(), P), label
    three, none3 = engine.zone_matrix_features(Pc, sc)
    assert not none3[0]

    def compare(vals, what):
        for k, n in enumerate(fr.ZONE_NAMES):
            want = float(ref["values"][n])
            _note("glszm", n, abs(vals[k] - want), 0.0, B[n])
            assert abs(vals[k] - want) <= B[n], (label, what, n, vals[k], want, B[n])
    compare(three[0], "three calls")
    d, dflag = engine.glszm_features(L, M, Ng, Ns, deferred=True)
    engine.deferred_status()
    if accepted:
        got, flag = engine.glszm_features(L, M, Ng, Ns)
        assert got[16] == 0 and flag[0] == 0
        compare(got[:16], "one queue")
        assert np.array_equal(d, got) and dflag[0] == 0
    else:
        assert int(d[16]) & 4, d[16]
        with pytest.raises(NotImplementedError):
            engine.glszm_features(L, M, Ng, Ns)
    # segment_features_enqueue answers on either route (the declined one falls to the three calls)
    names = fr.ZONE_CLASS_NAMES["glszm"]
    for deferred in (False, True):
        fin = cmatrices.segment_features_enqueue("glszm", L, M, Ng, names, Ns=Ns, deferred=deferred)
        if deferred:
            engine.deferred_status()
        vals = fin()
        compare([vals[n] for n in names], "segment_features_enqueue deferred=%s" % deferred)


@pytest.mark.parametrize("sizes", [(8191, 8192, 8193)], ids=["8191-8192-8193"])
def test_glszm_sizes_at_the_bitmap_boundary(dev, sizes):
    """zones of exactly 8191 (bitmap), 8192 and 8193 (sorted list) voxels side by side, repeated, at both row levels"""
    lengths = [8191, 8192, 8193, 8192, 8191, 8193, 8193, 8191, 8192, 8192, 8200, 8191, 1, 8199]
    lev, zones = _rows_volume(lengths, 8200)
    assert {s for _, s in zones} >= set(sizes)
    _check_glszm(dev, lev, zones, 5, "boundary 8191/8192/8193")


@pytest.mark.parametrize("nlarge", [1023, 1024, 1025, 2500])
def test_glszm_large_zone_deduplication_in_chunks(dev, nlarge):
    """more than 1024 zones of 8192+ voxels with many duplicates among their sizes: the de-duplication scan carries its
    running count across chunks of 1024"""
    y = np.arange(nlarge)
    lengths = 8192 + (y * 37) % 101                 # 101 distinct large sizes, each many times, unsorted
    lev, zones = _rows_volume(lengths, 8300)
    assert sum(c for (l, s), c in zones.items() if s >= 8192) == nlarge
    _check_glszm(dev, lev, zones, 5, "nlarge=%d" % nlarge)


@pytest.mark.parametrize("nlarge", [4096, 4097])
def test_glszm_large_zone_list_at_its_capacity(dev, nlarge):
    """exactly PRAD_RANK_LARGE = 4096 large zones are ranked on the device; 4097 set verdict bit 4 and the caller's three-call
    route returns the same values"""
    y = np.arange(nlarge)
    lengths = 8192 + (y * 7) % 9
    lev, zones = _rows_volume(lengths, 8200)
    _check_glszm(dev, lev, zones, 5, "nlarge=%d" % nlarge, accepted=nlarge <= 4096)


def test_glszm_distinct_sizes_at_the_kcap_bound(dev):
    """row r holds runs of r + 1 and k - r voxels: every size 1 .. k occurs once, n = k (k + 1) / 2, so the k distinct sizes
    sit at kcap = sqrt(2 n) + 2 = k + 2 as closely as a volume can"""
    k = 2000
    a = np.arange(1, k // 2 + 1)
    lev, zones = _rows_volume(a, k + 1)
    assert len({s for _, s in zones}) == k and lev.size == k * (k + 1) // 2
    assert int(math.sqrt(2.0 * lev.size)) + 2 == k + 2
    _check_glszm(dev, lev, zones, 5, "kcap")


def test_glszm_single_zone_and_no_zone(dev):
    import torch
    from pyradiomics_amd import engine
    lev = np.ones((4, 16, 64), dtype=np.int32)
    _check_glszm(dev, lev, {(1, lev.size): 1}, 1, "Ng=1 one zone")
    L = torch.from_numpy(lev).to(dev)
    M = torch.zeros(lev.shape, dtype=torch.uint8, device=dev)
    got, flag = engine.glszm_features(L, M, 1, 1)
    assert flag[0] != 0 and got[16] == 0 and np.isnan(got[:16]).all()


def test_zz_report():
    """prints the worst err / bound ratios of this run (kernel against the restatement, float64 numpy against it)"""
    worst = {}
    for (kern, name), (g, n) in RATIOS.items():
        w = worst.setdefault(kern, [0.0, "", 0.0, ""])
        if g > w[0]:
            w[0], w[1] = g, name
        if n > w[2]:
            w[2], w[3] = n, name
    for kern, (g, gn, n, nn) in sorted(worst.items()):
        print("RATIO %-6s kernel worst err/bound = %.3g (%s); float64 numpy worst err/bound = %.3g (%s)" % (kern, g, gn, n, nn))
    assert all(w[0] <= 1 for w in worst.values())

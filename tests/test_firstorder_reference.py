"""CPU tier of the first-order limits suite: tests/firstorder_reference.py (long double) against
oracle/firstorder_oracle.py (float64 numpy, pinned to the reference's recorded values) and against exact
fractions.Fraction arithmetic, and the comparison helper of tests/test_gpu_firstorder_limits.py against subtly wrong
results: for every segment-mode case family the reference result with ONE defect applied must be rejected under the very
bounds the GPU test uses for that case.  A defect that cannot change anything on a family (a rank +- 1 inside a run of
ties, the float32 rounding of a mean that float32 holds) is listed in VACUOUS and asserted to be exactly that."""
import math
from fractions import Fraction

import numpy as np
import pytest

import firstorder_reference as fr
from test_firstorder import _volume

LD = np.longdouble


def test_long_double_has_a_64_bit_significand():
    assert np.finfo(LD).nmant >= 63


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
@pytest.mark.parametrize("shape,frac", [((9, 30, 41), 0.6), ((1, 1, 7), 1.0), ((64, 64, 65), 0.05)])
def test_reference_agrees_with_the_oracle(dtype, shape, frac):
    """order statistics equal; sums within float64 pairwise-summation error of the oracle: numpy adds n terms in blocks of
    128 serial additions (8 accumulators of 16) and a tree above them, (16 + log2 n) roundings, plus 3 inside a term"""
    from oracle import firstorder_oracle
    img, mask = _volume(dtype, shape, 3, frac)
    mask.flat[0] = True
    for shift in (0.0, 2000.0):
        ref = fr.segment_reference(img, mask, shift)
        want = firstorder_oracle.firstorder_stats(img, mask, shift)
        k = 16 + math.ceil(math.log2(ref["m"])) + 3
        bad, _ = fr.compare(want, ref, fr.seg_bounds(ref, k))
        assert not bad, bad


def _fraction_stats(x, shift):
    """every summed field in exact rational arithmetic (about the same float64 means)"""
    xs = sorted(Fraction(float(v)) for v in x)
    m = len(xs)
    q = fr.quantiles_of_sorted(np.array([float(v) for v in xs]))
    mean = float(sum(xs) / m)                   # (Fraction -> float rounds correctly)
    d = [v - Fraction(mean) for v in xs]
    out = {"Energy": sum((v + Fraction(float(shift))) ** 2 for v in xs), "Mean": sum(xs) / m,
           "MAD": sum(abs(t) for t in d) / m, "m2": sum(t ** 2 for t in d) / m, "m3": sum(t ** 3 for t in d) / m,
           "m4": sum(t ** 4 for t in d) / m}
    band = [v for v in xs if q["P10"] <= v <= q["P90"]]
    if band:                                    # (two voxels: nothing lies between P10 and P90, rMAD is NaN)
        mub = float(sum(band) / len(band))
        out["rMAD"] = sum(abs(v - Fraction(mub)) for v in band) / len(band)
    return out, mean


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32, np.float64])
@pytest.mark.parametrize("m", [1, 2, 3, 10, 57, 200])
def test_reference_agrees_with_exact_fractions(dtype, m):
    rng = np.random.default_rng(m)
    kinds = [_volume(dtype, (m,), m)[0]]
    if np.issubdtype(dtype, np.floating):
        kinds.append((1e8 + rng.standard_normal(m) * 1e-3).astype(dtype))
    else:
        kinds.append((np.iinfo(dtype).max - rng.integers(0, 1000, m)).astype(dtype))
    for x in kinds:
        for shift in (0.0, -3.0, 0.1):
            ref = fr.stats_of_values(x, shift, np.issubdtype(dtype, np.integer))
            exact, mean = _fraction_stats(x, shift)
            v = ref["values"]
            assert v["Mean"] == mean and v["Np"] == m
            assert math.isnan(v["rMAD"]) == ("rMAD" not in exact)
            assert v["Minimum"] == float(x.min()) and v["Maximum"] == float(x.max())
            for name, q in zip(("P10", "P25", "Median", "P75", "P90"), (10, 25, 50, 75, 90)):
                assert v[name] == float(np.percentile(x.astype(np.float64), q)), name
            for f, e in exact.items():
                if f == "Mean":
                    continue
                # the long-double value itself: (log2 m + 3) roundings of 2^-64 relative to the sum of |terms|
                tol = Fraction(math.ceil(math.log2(m + 1)) + 4, 2 ** 64) * Fraction(float(ref["abs_sum"][f])) \
                    + abs(e) / 2 ** 53                              # + its rounding to the float64 it is returned as
                assert abs(Fraction(v[f]) - e) <= tol, (f, v[f], float(e))
            # abs_sum is what it says: the sum of the absolute terms
            d = [Fraction(float(t)) - Fraction(mean) for t in x]
            assert abs(Fraction(float(ref["abs_sum"]["m3"])) - sum(abs(t) ** 3 for t in d) / m) \
                <= Fraction(float(ref["abs_sum"]["m3"])) / 2 ** 50
            assert abs(Fraction(float(ref["abs_sum"]["Mean"])) - sum(abs(Fraction(float(t))) for t in x) / m) \
                <= Fraction(float(ref["abs_sum"]["Mean"])) / 2 ** 50


# ---- the comparator against subtly wrong results -------------------------------------------------------------------------
FAMILIES = fr.BOUNDARY + fr.SELECTION + fr.CANCELLATION + fr.SMALL
DEFECTS = ("dropped-voxel", "rank", "mean-float32", "neighbour-value")
# (family, defect) pairs on which the defect changes no field at all: constant ROIs; two-valued ROIs whose ten ranks lie
# inside one run of ties; means that float32 holds exactly
VACUOUS = {("const-f64", "rank"), ("const-f64", "mean-float32"), ("const-f64", "neighbour-value"),
           ("const-f32", "rank"), ("const-f32", "mean-float32"), ("const-f32", "neighbour-value"),
           ("const-i16", "rank"), ("const-i16", "mean-float32"), ("const-i16", "neighbour-value"),
           ("sel-outlier-single", "rank"),
           ("can-two-valued-f64", "rank"), ("can-two-valued-i16", "rank")}


def _defective(name, defect):
    """the reference's values with one defect, or None when no such defect exists on this input"""
    img, mask, shift, _ = fr.case(name)
    ref = fr.case_reference(name)
    if defect == "dropped-voxel":
        idx = np.flatnonzero(mask.ravel())
        keep = np.delete(idx, len(idx) // 2)
        return fr.stats_of_values(img.ravel()[keep], shift, np.issubdtype(img.dtype, np.integer))["values"]
    if defect == "rank":
        xs, m = ref["sorted"], ref["m"]
        for k, r in enumerate(fr.order_ranks(m)):
            for s in (1, -1):
                if 0 <= r + s < m and xs[r + s] != xs[r]:
                    out = dict(ref["values"])
                    out.update(fr.quantiles_of_sorted(xs, (k, s)))
                    if out != ref["values"]:
                        return out
        return None
    if defect == "mean-float32":
        out = dict(ref["values"])
        out["Mean"] = float(np.float32(out["Mean"]))
        return None if out["Mean"] == ref["values"]["Mean"] else out
    x = img.ravel()[np.flatnonzero(mask.ravel())].copy()          # ROI values in raster order
    differ = np.flatnonzero(x[1:] != x[:-1])
    if not len(differ):
        return None
    i = int(differ[len(differ) // 2])
    x[i] = x[i + 1]
    return fr.stats_of_values(x, shift, np.issubdtype(img.dtype, np.integer))["values"]


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("name", FAMILIES)
def test_comparator_rejects_a_defect(name, defect):
    ref = fr.case_reference(name)
    bounds = fr.seg_bounds(ref, *fr.case_k(name))
    bad, _ = fr.compare(dict(ref["values"]), ref, bounds)
    assert not bad, bad                                            # the reference itself passes
    got = _defective(name, defect)
    if (name, defect) in VACUOUS:
        assert got is None or got == ref["values"], "the defect is visible here: take the pair off VACUOUS"
        return
    assert got is not None, "no such defect on this input: change the family's inputs"
    bad, _ = fr.compare(got, ref, bounds)
    assert bad, "the bounds of this family are too loose to see the defect: change the family's inputs"


def test_every_route_bound_is_tighter_than_a_float32_accumulator():
    """k 2^-53 stays below 2^-24 / 1000 at the deepest geometry (1024 blocks, 2^31 - 1 voxels): no float32 step hides"""
    assert (fr.k_reduction(2 ** 31 - 1, 2) + fr.DIV) * fr.U < 2.0 ** -24 / 1000

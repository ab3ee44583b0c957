"""CPU tier: pins tests/feature_reference.py (the long-double restatement the GPU limit tests measure the kernels with)
to what the reference itself recorded, to exact rationals on hand-computable matrices, and shows by mutation that the pin
is sharp.  No GPU.

Tolerance of the golden pin.  The recorded feature values are float64 results of the reference's numpy code, so the rule is
|recorded - restated| <= c_ref * 2^-53 * A per angle (A = sum of the absolute terms, feature_reference.py), propagated to
first order through the derived features, then averaged over the angles (+ Na roundings of the mean).  c_ref follows numpy's
arithmetic, not the observed error: a reduction along a non-contiguous axis (the marginals, the boolean-mask sums of the
diagonals) adds serially, at most Ng terms; the contiguous reductions are pairwise (blocks of 128 summed in 8 lanes: 16
additions, then log2(n / 128) <= 10 levels); a term takes at most 8 roundings (normalisation, products, powers, log2):
c_ref = Ng + 16 + 10 + 8.  For Ng = 33 that is 7.4e-15 relative to A: far inside the 1e-10 the suite uses between routes.
"""
from fractions import Fraction

import numpy as np
import pytest

import feature_reference as fr
from helpers import GOLDEN, load_baseline_features

CASES = ["brain1", "brain2", "breast1"]
U = 2.0 ** -53


def c_ref(Ng):
    return Ng + 16 + 10 + 8


def _case_matrices(case, oracle_port):
    """golden matrices of `case` put back on the full level / size grid: the level and size values are those of the
    discretised image (fixed bin width 25 as in the configuration); the compacted oracle matrix must equal the golden one"""
    import os
    d = np.load(os.path.join(GOLDEN, case + ".npz"))
    img, m = d["image"].astype(np.float64), d["mask"] > 0
    lev = (np.floor(img / 25) - np.floor(img[m].min() / 25) + 1).astype(np.int32)
    gl = np.unique(lev[m])
    Ng = int(gl.max())
    out = {"Ng": Ng, "levels": gl}
    g = np.zeros((Ng, Ng, d["P_glcm"].shape[2]))
    g[np.ix_(gl - 1, gl - 1)] = d["P_glcm"]
    out["glcm"] = g
    r = np.asarray(oracle_port.calculate_glrlm(lev, m, Ng, max(lev.shape), False, 0)[0])
    r = r.reshape(r.shape[-3:])
    z = np.asarray(oracle_port.calculate_glszm(lev, m, Ng, int(m.sum()), False, 0))
    z = z.reshape(z.shape[-2:])
    dm = np.asarray(oracle_port.calculate_gldm(lev, m, [1], Ng, 0, False, 0))
    dm = dm.reshape(dm.shape[-2:])
    for cls, raw in (("glrlm", r), ("glszm", z), ("gldm", dm)):
        cols = np.where(raw.sum(axis=(0, 2) if raw.ndim == 3 else 0) > 0)[0]
        assert np.array_equal(raw[gl - 1][:, cols], d["P_" + cls]), (case, cls)
        full = np.zeros((Ng,) + d["P_" + cls].shape[1:])
        full[gl - 1] = d["P_" + cls]
        out[cls] = (full, cols + 1)
    assert np.array_equal(d["P_ngtdm"][:, 2], gl)
    n = np.zeros((Ng, 3))
    n[:, 2] = np.arange(1, Ng + 1)
    n[gl - 1] = d["P_ngtdm"]
    out["ngtdm"] = n
    return out


def _mean_bound(vals, bounds, empty):
    """bound of the nanmean over the kept angles: mean of the per-angle bounds + one rounding per addition and the division"""
    keep = ~np.asarray(empty)
    vals, bounds = np.asarray(vals, dtype=np.float64)[keep], np.asarray(bounds, dtype=np.float64)[keep]
    return np.nanmean(bounds, 0) + (len(vals) + 1) * U * np.nanmean(np.abs(vals), 0)


def _golden_differences(case, oracle_port, mutate=None):
    """-> list of (class, feature, recorded, restated, bound)"""
    M = _case_matrices(case, oracle_port)
    want = load_baseline_features()[case]["features"]
    Ng, c = M["Ng"], c_ref(M["Ng"])
    rows = []
    ref = fr.glcm_reference(M["glcm"], symmetric=False, mutate=mutate)        # (the golden matrix is symmetrised and normalised)
    empty = [r["empty"] for r in ref]
    vals = np.array([[float(r["values"][n]) for n in fr.GLCM_NAMES] for r in ref])
    bnds = np.array([[fr.glcm_bounds(r, c, c)[0][n] for n in fr.GLCM_NAMES] for r in ref])
    mean, mb = fr.angle_mean(vals, empty), _mean_bound(vals, bnds, empty)
    for k, n in enumerate(fr.GLCM_NAMES):
        rows.append(("glcm", n, want["glcm"][n], mean[k], mb[k]))
    mcc = fr.mcc_reference(M["glcm"], symmetric=False)
    # eigenvalues of the non-symmetric Q in float64: Q = S M S^-1 with M symmetric and S = diag(sqrt(px)), so the error of an
    # eigenvalue is at most cond(S) n u |Q| (Bauer-Fike), and that of its square root is divided by 2 sigma_2
    px = np.array([np.asarray(r["px"], dtype=np.float64) for r in ref])
    conds = [np.sqrt(p[p > 0].max() / p[p > 0].min()) for p in px]
    mb_mcc = np.mean([8 * n_occ * U * cs / (2 * v) for (v, n_occ), cs in zip(mcc, conds)])
    rows.append(("glcm", "MCC", want["glcm"]["MCC"], np.mean([v for v, _ in mcc]), mb_mcc))
    for cls in ("glrlm", "glszm", "gldm"):
        P, jv = M[cls]
        ref = fr.zone_reference(P, jv, mutate=mutate)
        empty = [r["empty"] for r in ref]
        vals = np.array([[float(r["values"][n]) for n in fr.ZONE_NAMES] for r in ref])
        bnds = np.array([[fr.zone_bounds(r, c, c)[n] for n in fr.ZONE_NAMES] for r in ref])
        mean, mb = fr.angle_mean(vals, empty), _mean_bound(vals, bnds, empty)
        for k, n in enumerate(fr.ZONE_CLASS_NAMES[cls]):
            if n is not None:
                rows.append((cls, n, want[cls][n], mean[k], mb[k]))
        assert set(want[cls]) == {n for n in fr.ZONE_CLASS_NAMES[cls] if n}
    r = fr.ngtdm_reference(M["ngtdm"])
    B, cond = fr.ngtdm_bounds(r, c, c)
    for n in fr.NGTDM_NAMES:
        rows.append(("ngtdm", n, want["ngtdm"][n], float(r["values"][n]), B[n]))
    assert set(want["glcm"]) == set(fr.GLCM_NAMES) | {"MCC"} and set(want["ngtdm"]) == set(fr.NGTDM_NAMES)
    return rows


def test_long_double_is_the_yardstick():
    assert fr.HAVE_LONGDOUBLE and np.finfo(np.longdouble).eps < 2e-19


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_recorded_reference_values(case, oracle_port):
    rows = _golden_differences(case, oracle_port)
    assert len(rows) == 24 + 16 + 16 + 14 + 5
    worst = max(rows, key=lambda r: abs(r[2] - r[3]) / r[4] if r[4] > 0 else 0.0)
    print("%s: worst |recorded - restated| / bound = %.3g (%s %s)" % (case, abs(worst[2] - worst[3]) / worst[4], worst[0], worst[1]))
    for cls, n, rec, got, bound in rows:
        assert np.isfinite(got) and abs(rec - got) <= bound, (cls, n, rec, got, abs(rec - got), bound)
        # the bound is never looser than what the suite uses between routes
        assert bound <= 1e-10 * max(abs(rec), 1e-300) or n in ("ClusterShade", "MCC", "Imc1", "Imc2", "Correlation"), (cls, n, bound, rec)
        assert bound <= 1e-9 * max(abs(rec), 1.0), (cls, n, bound, rec)


@pytest.mark.parametrize("mutate,hit", [("contrast_abs", ("glcm", "Contrast")), ("iv_no_guard", ("glcm", "InverseVariance")),
                                        ("size_index", ("glszm", "LargeAreaEmphasis"))])
def test_golden_pin_fails_on_a_mutated_restatement(mutate, hit, oracle_port):
    """(i - j)^2 -> |i - j|; the k >= 1 guard of InverseVariance dropped; the size VALUE replaced by the column index + 1:
    each must break the comparison above, on the feature it touches and on no feature of another class"""
    rows = _golden_differences("brain1", oracle_port, mutate=mutate)
    bad = [(cls, n) for cls, n, rec, got, bound in rows if not (np.isfinite(got) and abs(rec - got) <= bound)]
    assert hit in bad
    # (brain1's run lengths have a gap as well: the size mutation shows in both classes that carry a size table)
    assert {cls for cls, _ in bad} <= ({"glrlm", "glszm"} if mutate == "size_index" else {"glcm"})


# ---- hand-computable matrices, exact rationals ------------------------------------------------------------------------
def _exact_glcm(C):
    """the features without logarithms (and without square roots) of a count matrix, in exact rationals"""
    n = len(C)
    tot = sum(sum(Fraction(x) for x in row) for row in C)
    p = [[Fraction(C[i][j]) / tot for j in range(n)] for i in range(n)]
    E = lambda f: sum(p[i][j] * f(i + 1, j + 1) for i in range(n) for j in range(n))
    ux, uy = E(lambda i, j: i), E(lambda i, j: j)
    pd = [sum(p[i][j] for i in range(n) for j in range(n) if abs(i - j) == k) for k in range(n)]
    da = sum(k * pd[k] for k in range(n))
    return {
        "Autocorrelation": E(lambda i, j: i * j), "JointAverage": ux, "Contrast": E(lambda i, j: (i - j) ** 2),
        "ClusterTendency": E(lambda i, j: (i + j - ux - uy) ** 2), "ClusterShade": E(lambda i, j: (i + j - ux - uy) ** 3),
        "ClusterProminence": E(lambda i, j: (i + j - ux - uy) ** 4), "JointEnergy": E(lambda i, j: p[i - 1][j - 1]),
        "SumSquares": E(lambda i, j: (i - ux) ** 2), "SumAverage": E(lambda i, j: i + j), "DifferenceAverage": da,
        "DifferenceVariance": sum(pd[k] * (k - da) ** 2 for k in range(n)),
        "Idm": sum(pd[k] / (1 + k * k) for k in range(n)), "Id": sum(pd[k] / (1 + k) for k in range(n)),
        "Idmn": sum(pd[k] / (1 + Fraction(k * k, n * n)) for k in range(n)),
        "Idn": sum(pd[k] / (1 + Fraction(k, n)) for k in range(n)),
        "InverseVariance": sum(pd[k] / (k * k) for k in range(1, n)),
        "MaximumProbability": max(max(r) for r in p),
    }


HAND = {
    "1x1": [[7]],
    "2x2": [[1, 2], [3, 4]],
    "off_diagonal_pair": [[0, 0, 0, 0], [0, 0, 0, 5], [0, 0, 0, 0], [0, 0, 0, 0]],
    "diagonal": [[3, 0, 0], [0, 1, 0], [0, 0, 6]],
    "independent": [[2 * 1, 2 * 3, 2 * 5], [7 * 1, 7 * 3, 7 * 5], [4 * 1, 4 * 3, 4 * 5]],
}


@pytest.mark.parametrize("name", sorted(HAND))
@pytest.mark.parametrize("symmetric", [False, True])
def test_glcm_restatement_on_hand_matrices_in_exact_rationals(name, symmetric):
    C = np.array(HAND[name], dtype=np.float64)
    S = C + C.T if symmetric else C
    want = _exact_glcm([[int(x) for x in row] for row in S])
    r = fr.glcm_angle(C, symmetric)
    for n, w in want.items():
        got, w = r["values"][n], np.longdouble(w.numerator) / np.longdouble(w.denominator)
        assert abs(got - w) <= 32 * float(np.finfo(np.longdouble).eps) * max(abs(w), 1e-30) + (1e-17 if w == 0 else 0), (n, got, w)
    V = r["values"]
    if name == "1x1":
        assert V["Correlation"] == 1 and V["Imc1"] == 0 and V["Imc2"] == 0 and V["MaximumProbability"] == 1
        assert abs(V["JointEntropy"]) < 1e-15
    if name == "off_diagonal_pair" and not symmetric:        # one entry: sigma_x = sigma_y = 0
        assert V["Correlation"] == 1 and V["Imc1"] == 0 and V["Contrast"] == 4
    if name == "diagonal":
        assert abs(V["Correlation"] - 1) < 1e-14 and V["Contrast"] == 0 and V["Idm"] == 1
    if name == "independent" and not symmetric:
        # p = px py exactly: HXY2 - HXY is 0 in exact arithmetic, Imc2 is rounding noise or an exact 0 / NaN
        x = r["parts"]["HXY2"][0] - r["parts"]["HXY"][0]
        assert abs(x) < 1e-17 and abs(V["Correlation"]) < 1e-17 and abs(V["Imc1"]) < 1e-17
        assert np.isnan(V["Imc2"]) or abs(V["Imc2"]) < 1e-8


def test_zone_and_ngtdm_restatements_on_hand_matrices():
    P = np.zeros((4, 6))
    P[1, 2] = 5                                         # one entry: level 2, size value 9
    jv = [1, 2, 9, 11, 12, 40]
    V = fr.zone_angle(P, jv)["values"]
    L = np.longdouble
    want = {"SmallEmphasis": L(1) / 81, "LargeEmphasis": 81, "GrayLevelNonUniformity": 5, "GrayLevelNonUniformityNormalized": 1,
            "SizeNonUniformity": 5, "SizeNonUniformityNormalized": 1, "Percentage": L(1) / 9, "GrayLevelVariance": 0,
            "SizeVariance": 0, "LowGrayLevelEmphasis": L(1) / 4, "HighGrayLevelEmphasis": 4,
            "SmallLowGrayLevelEmphasis": L(1) / 324, "SmallHighGrayLevelEmphasis": L(4) / 81,
            "LargeLowGrayLevelEmphasis": L(81) / 4, "LargeHighGrayLevelEmphasis": 324}
    for n, w in want.items():
        assert abs(V[n] - w) <= 4 * float(np.finfo(L).eps) * abs(w), (n, V[n], w)
    assert abs(V["Entropy"]) < 1e-15
    assert fr.zone_angle(np.zeros((3, 3)), [1, 2, 3])["empty"]
    # two zones of level 1 (size 1, size 3) and one of level 3 (size 3): exact rationals
    P = np.array([[1, 1], [0, 0], [0, 1]], dtype=np.float64)
    V = fr.zone_angle(P, [1, 3])["values"]
    F = Fraction
    want = {"SmallEmphasis": (1 + F(2, 9)) / 3, "LargeEmphasis": F(19, 3), "GrayLevelNonUniformity": F(5, 3),
            "SizeNonUniformity": F(5, 3), "Percentage": F(3, 7), "GrayLevelVariance": F(2, 3) * F(4, 9) + F(1, 3) * F(16, 9),
            "SizeVariance": F(1, 3) * F(16, 9) + F(2, 3) * F(4, 9), "LowGrayLevelEmphasis": (2 + F(1, 9)) / 3,
            "HighGrayLevelEmphasis": F(11, 3), "SmallLowGrayLevelEmphasis": (1 + F(1, 9) + F(1, 81)) / 3,
            "LargeHighGrayLevelEmphasis": F(1 + 9 + 81, 3)}
    for n, w in want.items():
        w = L(w.numerator) / L(w.denominator)
        assert abs(V[n] - w) <= 8 * float(np.finfo(L).eps) * abs(w), (n, V[n], w)
    # NGTDM: two levels (values 2 and 5), n = (3, 1), s = (1/2, 3/2)
    N = np.array([[0, 0, 1], [3, 0.5, 2], [0, 0, 3], [0, 7.0, 4], [1, 1.5, 5]])
    V = fr.ngtdm_reference(N)["values"]
    coarse = F(3, 4) * F(1, 2) + F(1, 4) * F(3, 2)
    want = {"Coarseness": 1 / coarse, "Contrast": 2 * F(3, 16) * 9 * 2 / 4 / 2,
            "Busyness": coarse / (2 * abs(2 * F(3, 4) - 5 * F(1, 4))), "Complexity": 2 * 3 * coarse / 4,
            "Strength": F(2 * 9, 2)}
    for n, w in want.items():
        w = L(w.numerator) / L(w.denominator)
        assert abs(V[n] - w) <= 8 * float(np.finfo(L).eps) * abs(w), (n, V[n], w)
    flat = fr.ngtdm_reference(np.array([[9, 0.0, 1]]))["values"]
    assert flat["Coarseness"] == 1e6 and flat["Contrast"] == 0 and flat["Busyness"] == 0 and flat["Strength"] == 0


def test_float64_evaluation_of_the_restatement_meets_its_own_bound():
    """the same expressions in float64 numpy (the reference's arithmetic) stay inside the bound with c_ref: the bound is fair"""
    rng = np.random.default_rng(5)
    Ng = 150
    C = rng.integers(0, 50, size=(Ng, Ng)).astype(np.float64)
    hi, lo = fr.glcm_angle(C, True), fr.glcm_angle(C, True, dtype=np.float64)
    B, cond = fr.glcm_bounds(hi, c_ref(Ng), c_ref(Ng))
    for n in fr.GLCM_NAMES:
        assert abs(float(hi["values"][n]) - float(lo["values"][n])) <= B[n], (n, hi["values"][n], lo["values"][n], B[n])
    assert min(cond.values()) > 100

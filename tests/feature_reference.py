"""High-precision restatement of the segment-mode feature formulas (test helper, not a test).

Plain numpy in np.longdouble (64-bit mantissa on x86: 11 bits more than the float64 the kernels and the reference carry),
written from the definitions the reference documents for its GLCM, GLRLM / GLSZM / GLDM and NGTDM classes; nothing here
imports the product's formula modules.  Every function takes `dtype`: np.longdouble is the yardstick, np.float64 evaluates
the very same expressions with numpy's float64 sums (the reference's arithmetic), which is how a test finds out whether a
bound is fair to float64 at all.

For every feature that is a plain sum F = sum t the functions also return A = sum |t| (for an entropy term p * log2(p + eps)
the |t| is p * (|log2(p + eps)| + 2): the logarithm of a rounded argument is off by up to 2^-53 / ln 2 whatever its own
size), for the moments about a mean the sensitivity D = sum |dt / d mean|, and for the derived features the component sums,
so a bound can follow the conditioning: see glcm_bounds / zone_bounds / ngtdm_bounds, which take the chain-length
constants `c` (derived by the caller from the arithmetic under test) and propagate them to first order.

Matrices are indexed by level: row i stands for grey level i + 1 (absent levels are all-zero rows and columns, which is
what the reference's deletion of absent levels amounts to, its Ng being the largest level).
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
if not np.finfo(LD).eps < 2e-19:      # (a platform whose long double is float64: no yardstick; mpmath covers small sizes)
    import mpmath  # noqa: F401
    HAVE_LONGDOUBLE = False
else:
    HAVE_LONGDOUBLE = True
U = 2.0 ** -53                        # unit roundoff of float64
LN2INV = 1.0 / math.log(2.0)

GLCM_NAMES = ["Autocorrelation", "JointAverage", "ClusterProminence", "ClusterShade", "ClusterTendency", "Contrast",
              "Correlation", "DifferenceAverage", "DifferenceEntropy", "DifferenceVariance", "JointEnergy", "JointEntropy",
              "Imc1", "Imc2", "Idm", "Idmn", "Id", "Idn", "InverseVariance", "MaximumProbability", "SumAverage",
              "SumEntropy", "SumSquares"]
# how each GLCM value is obtained: a sum over the Ng^2 entries, over a marginal (k values), about a mean, or derived
GLCM_ENTRY_SUMS = ["Autocorrelation", "JointAverage", "Contrast", "JointEnergy", "JointEntropy"]
GLCM_MARGINAL_SUMS = ["DifferenceAverage", "DifferenceEntropy", "Idm", "Idmn", "Id", "Idn", "InverseVariance", "SumAverage",
                      "SumEntropy"]
GLCM_CENTRED = ["ClusterProminence", "ClusterShade", "ClusterTendency", "SumSquares", "DifferenceVariance"]
GLCM_DERIVED = ["Correlation", "Imc1", "Imc2"]

ZONE_NAMES = ["SmallEmphasis", "LargeEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized",
              "SizeNonUniformity", "SizeNonUniformityNormalized", "Percentage", "GrayLevelVariance", "SizeVariance", "Entropy",
              "LowGrayLevelEmphasis", "HighGrayLevelEmphasis", "SmallLowGrayLevelEmphasis", "SmallHighGrayLevelEmphasis",
              "LargeLowGrayLevelEmphasis", "LargeHighGrayLevelEmphasis"]
ZONE_ENTRY_SUMS = ["Entropy", "SmallLowGrayLevelEmphasis", "SmallHighGrayLevelEmphasis", "LargeLowGrayLevelEmphasis",
                   "LargeHighGrayLevelEmphasis"]
ZONE_CLASS_NAMES = {
    "glrlm": ["ShortRunEmphasis", "LongRunEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized",
              "RunLengthNonUniformity", "RunLengthNonUniformityNormalized", "RunPercentage", "GrayLevelVariance", "RunVariance",
              "RunEntropy", "LowGrayLevelRunEmphasis", "HighGrayLevelRunEmphasis", "ShortRunLowGrayLevelEmphasis",
              "ShortRunHighGrayLevelEmphasis", "LongRunLowGrayLevelEmphasis", "LongRunHighGrayLevelEmphasis"],
    "glszm": ["SmallAreaEmphasis", "LargeAreaEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized",
              "SizeZoneNonUniformity", "SizeZoneNonUniformityNormalized", "ZonePercentage", "GrayLevelVariance", "ZoneVariance",
              "ZoneEntropy", "LowGrayLevelZoneEmphasis", "HighGrayLevelZoneEmphasis", "SmallAreaLowGrayLevelEmphasis",
              "SmallAreaHighGrayLevelEmphasis", "LargeAreaLowGrayLevelEmphasis", "LargeAreaHighGrayLevelEmphasis"],
    # (the GLDM class has no normalised grey-level non-uniformity and no percentage)
    "gldm": ["SmallDependenceEmphasis", "LargeDependenceEmphasis", "GrayLevelNonUniformity", None, "DependenceNonUniformity",
             "DependenceNonUniformityNormalized", None, "GrayLevelVariance", "DependenceVariance", "DependenceEntropy",
             "LowGrayLevelEmphasis", "HighGrayLevelEmphasis", "SmallDependenceLowGrayLevelEmphasis",
             "SmallDependenceHighGrayLevelEmphasis", "LargeDependenceLowGrayLevelEmphasis",
             "LargeDependenceHighGrayLevelEmphasis"],
}
NGTDM_NAMES = ["Coarseness", "Contrast", "Busyness", "Complexity", "Strength"]


def _eps(dtype):
    return dtype(np.spacing(1))


def _ent(p, eps, dtype):
    """-> (sum p log2(p + eps), sum p (|log2(p + eps)| + 2))"""
    lg = np.log2(p + eps)
    return (p * lg).sum(dtype=dtype), (p * (np.abs(lg) + 2)).sum(dtype=dtype)


def _diag_sums(p, anti):
    """sums of the diagonals |.. i - j = d ..| (anti=False: index d + n - 1) or of the anti-diagonals i + j = k"""
    n = p.shape[0]
    q = p[::-1] if anti else p
    # np.trace keeps the dtype; offsets -(n-1) .. n-1.  flipped rows: anti-diagonal k = i + j  <->  offset k - (n - 1)
    return np.array([np.trace(q, offset=o, dtype=p.dtype) for o in range(-(n - 1), n)], dtype=p.dtype)


def glcm_angle(C, symmetric=True, dtype=LD, mutate=None):
    """one angle: C [Ng, Ng] raw counts (or probabilities) -> dict(empty, values, A, D, parts); level of row i is i + 1.
    `mutate` deliberately breaks one term (tests of the tests): "contrast_abs" | "iv_no_guard"."""
    C = np.asarray(C).astype(dtype)
    if symmetric:
        C = C + C.T
    Ng = C.shape[0]
    tot = C.sum(dtype=dtype)
    nan = dtype(np.nan)
    if tot == 0:
        return {"empty": True, "values": {n: nan for n in GLCM_NAMES}, "A": {}, "D": {}, "parts": {}}
    eps = _eps(dtype)
    p = C / tot
    lev = np.arange(1, Ng + 1).astype(dtype)
    i, j = lev[:, None], lev[None, :]
    px, py = p.sum(1, dtype=dtype), p.sum(0, dtype=dtype)
    ad = _diag_sums(p, True)                       # p_{x+y}(k), k = i + j = 2 .. 2 Ng
    dg = _diag_sums(p, False)
    pdif = dg[Ng - 1:].copy()                      # p_{x-y}(k), k = |i - j| = 0 .. Ng - 1
    pdif[1:] += dg[:Ng - 1][::-1]
    ksum = np.arange(2, 2 * Ng + 1).astype(dtype)
    kdif = np.arange(0, Ng).astype(dtype)
    V, A, D, parts = {}, {}, {}, {}

    def plain(name, terms):
        V[name], A[name] = terms.sum(dtype=dtype), np.abs(terms).sum(dtype=dtype)

    ux, uy = (i * p).sum(dtype=dtype), (j * p).sum(dtype=dtype)
    parts["ux"], parts["uy"] = (ux, ux), (uy, uy)
    plain("Autocorrelation", p * (i * j))
    plain("JointAverage", i * p)
    plain("Contrast", p * (np.abs(i - j) if mutate == "contrast_abs" else (i - j) ** 2))
    plain("JointEnergy", p * p)
    h, ha = _ent(p, eps, dtype)
    V["JointEntropy"], A["JointEntropy"] = -h, ha
    V["MaximumProbability"] = p.max()
    s = (i + j) - ux - uy
    plain("ClusterTendency", p * s ** 2)
    plain("ClusterShade", p * s ** 3)
    plain("ClusterProminence", p * s ** 4)
    D["ClusterTendency"] = (2 * p * np.abs(s)).sum(dtype=dtype)
    D["ClusterShade"] = (3 * p * s ** 2).sum(dtype=dtype)
    D["ClusterProminence"] = (4 * p * np.abs(s) ** 3).sum(dtype=dtype)
    di, dj = i - ux, j - uy
    plain("SumSquares", p * di ** 2)
    D["SumSquares"] = (2 * p * np.abs(di)).sum(dtype=dtype)
    vx = V["SumSquares"]
    vy = (p * dj ** 2).sum(dtype=dtype)
    cov_t = p * di * dj
    cov, cov_A = cov_t.sum(dtype=dtype), np.abs(cov_t).sum(dtype=dtype)
    parts["vx"] = (vx, vx, D["SumSquares"])
    parts["vy"] = (vy, vy, (2 * p * np.abs(dj)).sum(dtype=dtype))
    parts["cov"] = (cov, cov_A, (p * (np.abs(di) + np.abs(dj))).sum(dtype=dtype))
    sx, sy = np.sqrt(vx), np.sqrt(vy)
    V["Correlation"] = dtype(1) if sx * sy == 0 else cov / (sx * sy + eps)
    # differences and sums
    plain("DifferenceAverage", kdif * pdif)
    h, ha = _ent(pdif, eps, dtype)
    V["DifferenceEntropy"], A["DifferenceEntropy"] = -h, ha
    da = V["DifferenceAverage"]
    plain("DifferenceVariance", pdif * (kdif - da) ** 2)
    D["DifferenceVariance"] = (2 * pdif * np.abs(kdif - da)).sum(dtype=dtype)
    plain("Idm", pdif / (1 + kdif ** 2))
    plain("Idmn", pdif / (1 + kdif ** 2 / dtype(Ng) ** 2))
    plain("Id", pdif / (1 + kdif))
    plain("Idn", pdif / (1 + kdif / dtype(Ng)))
    plain("InverseVariance", pdif[1:] / kdif[1:] ** 2)
    if mutate == "iv_no_guard":
        with np.errstate(divide="ignore", invalid="ignore"):
            V["InverseVariance"] = (pdif / kdif ** 2).sum(dtype=dtype)
    plain("SumAverage", ksum * ad)
    h, ha = _ent(ad, eps, dtype)
    V["SumEntropy"], A["SumEntropy"] = -h, ha
    # information measures of correlation
    q = px[:, None] * py[None, :]
    lq = np.log2(q + eps)
    hxy = V["JointEntropy"]
    hxy1, hxy1_A = -(p * lq).sum(dtype=dtype), (p * (np.abs(lq) + 2)).sum(dtype=dtype)
    hxy2, hxy2_A = -(q * lq).sum(dtype=dtype), (q * (np.abs(lq) + 2)).sum(dtype=dtype)
    hx, hx_A = _ent(px, eps, dtype)
    hy, hy_A = _ent(py, eps, dtype)
    hx, hy = -hx, -hy
    parts.update(HXY=(hxy, A["JointEntropy"]), HXY1=(hxy1, hxy1_A), HXY2=(hxy2, hxy2_A), HX=(hx, hx_A), HY=(hy, hy_A))
    div = max(hx, hy)
    V["Imc1"] = (hxy - hxy1) / div if div != 0 else dtype(0)
    if hxy2 == hxy:
        V["Imc2"] = dtype(0)
    else:
        with np.errstate(invalid="ignore"):
            V["Imc2"] = np.sqrt(1 - np.exp(-2 * (hxy2 - hxy)))
    return {"empty": False, "values": V, "A": A, "D": D, "parts": parts, "Ng": Ng, "px": px, "py": py, "p": p}


def glcm_reference(counts, symmetric=True, dtype=LD, mutate=None):
    """counts [Ng, Ng, Na] -> list of glcm_angle results"""
    counts = np.asarray(counts)
    return [glcm_angle(counts[:, :, a], symmetric, dtype, mutate) for a in range(counts.shape[2])]


def glcm_bounds(r, c_entry, c_marg, u=U):
    """first-order error bounds of one angle's values for an evaluation in float64 whose sums over the entries have the
    chain constant c_entry and whose marginal-based sums have c_marg (marginal build + sum over k): {name: bound}.
    Imc2 / Correlation / Imc1 come with their condition numbers in "cond" (the caller asserts them)."""
    V, A, D, P = r["values"], r["A"], r["D"], r["parts"]
    Ng = r["Ng"]
    f = lambda x: float(abs(x))
    B = {}
    for n in GLCM_ENTRY_SUMS:
        B[n] = c_entry * u * f(A[n])
    for n in GLCM_MARGINAL_SUMS:
        B[n] = c_marg * u * f(A[n])
    B["MaximumProbability"] = 2 * u * f(V["MaximumProbability"])
    b_u = c_entry * u * f(P["ux"][1]) + c_entry * u * f(P["uy"][1]) + 3 * u * 2 * Ng      # means + the roundings of (i + j) - ux - uy
    # a deviation d known to within delta: |(d + e)^m - d^m| <= (|d| + delta)^m - |d|^m for |e| <= delta, summed with the weights
    # (to first order this is D * delta; the higher orders matter where every deviation is 0, e.g. one anti-diagonal)
    lev = np.arange(1, Ng + 1).astype(LD)
    p, ux, uy = r["p"], P["ux"][0], P["uy"][0]

    def moved(w, dev, m, delta):
        a = np.abs(dev)
        return float((w * ((a + LD(delta)) ** m - a ** m)).sum(dtype=LD))
    s_abs = (lev[:, None] + lev[None, :]) - ux - uy
    for n, m in (("ClusterProminence", 4), ("ClusterShade", 3), ("ClusterTendency", 2)):
        B[n] = c_entry * u * f(A[n]) + moved(p, s_abs, m, b_u)
    B["SumSquares"] = c_entry * u * f(A["SumSquares"]) + moved(r["px"], lev - ux, 2, b_u)
    b_da = B["DifferenceAverage"] + 2 * u * Ng
    B["DifferenceVariance"] = c_marg * u * f(A["DifferenceVariance"]) + f(D["DifferenceVariance"]) * b_da + b_da ** 2
    cond = {}
    # Correlation = cov / (sx sy + eps)
    vx, vy, cov = P["vx"], P["vy"], P["cov"]
    b_vx = B["SumSquares"]
    b_vy = c_entry * u * f(vy[1]) + moved(r["py"], lev - uy, 2, b_u)
    b_cov = c_entry * u * f(cov[1]) + f(cov[2]) * b_u + b_u ** 2          # |(di + e)(dj + e') - di dj| <= delta (|di| + |dj|) + delta^2
    sx, sy = math.sqrt(f(vx[0])), math.sqrt(f(vy[0]))
    d = sx * sy
    if d == 0:
        B["Correlation"] = 0.0
    else:
        b_sx, b_sy = b_vx / (2 * sx) + u * sx, b_vy / (2 * sy) + u * sy
        b_d = sx * b_sy + sy * b_sx + 2 * u * d
        cond["Correlation"] = d / b_d
        B["Correlation"] = b_cov / d + f(cov[0]) * b_d / d ** 2 + 3 * u * f(V["Correlation"])
    # entropies: the marginals px, py enter a logarithm with their own relative error (c_marg u each)
    b_hxy = c_entry * u * f(P["HXY"][1])
    b_hxy1 = c_entry * u * f(P["HXY1"][1]) + 2 * c_marg * u * LN2INV
    b_hxy2 = (c_entry + 2 * c_marg) * u * f(P["HXY2"][1])
    b_hx, b_hy = 2 * c_marg * u * f(P["HX"][1]), 2 * c_marg * u * f(P["HY"][1])
    div = max(f(P["HX"][0]), f(P["HY"][0]))
    if div == 0:
        B["Imc1"] = 0.0
    else:
        b_div = max(b_hx, b_hy)
        cond["Imc1"] = div / b_div
        num = f(P["HXY"][0] - P["HXY1"][0])
        B["Imc1"] = (b_hxy + b_hxy1) / div + num * b_div / div ** 2 + 2 * u * f(V["Imc1"])
    x, b_x = float(P["HXY2"][0] - P["HXY"][0]), b_hxy + b_hxy2
    B["HXY2-HXY"] = b_x
    if x == 0:
        B["Imc2"] = 0.0
    else:
        cond["Imc2"] = x / b_x
        v = f(V["Imc2"]) if x > 0 else float("nan")
        B["Imc2"] = b_x * math.exp(-2 * x) / v + 4 * u * v if x > 0 else float("nan")
    return B, cond


def mcc_reference(counts, symmetric=True):
    """per angle: (MCC, sigma_2 / conditioning info): second largest singular value of A(i, k) = p(i, k) / sqrt(px(i) py(k) + eps)
    on the occurring levels (the matrix Q of the definition is similar to A A^T); NaN for an angle without pairs, 0 when
    fewer than two levels occur.  A is formed in long double; the singular values are float64 (LAPACK), whose absolute
    error is a small multiple of n 2^-53 sigma_1 with sigma_1 <= 1."""
    counts = np.asarray(counts)
    out = []
    for a in range(counts.shape[2]):
        C = counts[:, :, a].astype(LD)
        if symmetric:
            C = C + C.T
        tot = C.sum(dtype=LD)
        if tot == 0:
            out.append((float("nan"), 0))
            continue
        p = C / tot
        px, py = p.sum(1, dtype=LD), p.sum(0, dtype=LD)
        occ = np.where((px > 0) | (py > 0))[0]
        if len(occ) < 2:
            out.append((0.0, len(occ)))
            continue
        Am = p[np.ix_(occ, occ)] / np.sqrt(px[occ][:, None] * py[occ][None, :] + _eps(LD))
        sv = np.linalg.svd(Am.astype(np.float64), compute_uv=False)
        out.append((float(sv[1]), len(occ)))
    return out


# ---- GLRLM / GLSZM / GLDM ----------------------------------------------------------------------------------------
def zone_angle(P, jvals, ivals=None, dtype=LD, mutate=None):
    """P [Ni, Nj] counts, size values jvals [Nj], level values ivals (default 1 .. Ni) -> dict(empty, values, A, D, parts)"""
    P = np.asarray(P).astype(dtype)
    Ni, Nj = P.shape
    nan = dtype(np.nan)
    n = P.sum(dtype=dtype)
    if n == 0:
        return {"empty": True, "values": {k: nan for k in ZONE_NAMES}, "A": {}, "D": {}, "parts": {}}
    iv = (np.arange(1, Ni + 1) if ivals is None else np.asarray(ivals)).astype(dtype)
    jv = np.asarray(jvals).astype(dtype)
    if mutate == "size_index":
        jv = np.arange(1, Nj + 1).astype(dtype)
    eps = _eps(dtype)
    pg, pj = P.sum(1, dtype=dtype), P.sum(0, dtype=dtype)
    V, A, D = {}, {}, {}
    V["SmallEmphasis"] = (pj / jv ** 2).sum(dtype=dtype) / n
    V["LargeEmphasis"] = (pj * jv ** 2).sum(dtype=dtype) / n
    V["GrayLevelNonUniformity"] = (pg ** 2).sum(dtype=dtype) / n
    V["GrayLevelNonUniformityNormalized"] = (pg ** 2).sum(dtype=dtype) / n ** 2
    V["SizeNonUniformity"] = (pj ** 2).sum(dtype=dtype) / n
    V["SizeNonUniformityNormalized"] = (pj ** 2).sum(dtype=dtype) / n ** 2
    j1 = (pj * jv).sum(dtype=dtype)
    V["Percentage"] = n / j1
    ui, uj = (pg * iv).sum(dtype=dtype) / n, j1 / n
    V["GrayLevelVariance"] = ((pg / n) * (iv - ui) ** 2).sum(dtype=dtype)
    V["SizeVariance"] = ((pj / n) * (jv - uj) ** 2).sum(dtype=dtype)
    D["GrayLevelVariance"] = (2 * (pg / n) * np.abs(iv - ui)).sum(dtype=dtype)
    D["SizeVariance"] = (2 * (pj / n) * np.abs(jv - uj)).sum(dtype=dtype)
    p = P / n
    h, ha = _ent(p, eps, dtype)
    V["Entropy"], A["Entropy"] = -h, ha
    V["LowGrayLevelEmphasis"] = (pg / iv ** 2).sum(dtype=dtype) / n
    V["HighGrayLevelEmphasis"] = (pg * iv ** 2).sum(dtype=dtype) / n
    i2, j2 = (iv ** 2)[:, None], (jv ** 2)[None, :]
    V["SmallLowGrayLevelEmphasis"] = (P / (i2 * j2)).sum(dtype=dtype) / n
    V["SmallHighGrayLevelEmphasis"] = (P * i2 / j2).sum(dtype=dtype) / n
    V["LargeLowGrayLevelEmphasis"] = (P * j2 / i2).sum(dtype=dtype) / n
    V["LargeHighGrayLevelEmphasis"] = (P * i2 * j2).sum(dtype=dtype) / n
    for k in ZONE_NAMES:      # every sum but the entropy has non-negative terms: A is the value itself
        A.setdefault(k, abs(V[k]))
    parts = {"ui": ui, "uj": uj, "n": n, "Ni": Ni, "Nj": Nj, "maxj": jv.max(), "maxi": iv.max()}
    return {"empty": False, "values": V, "A": A, "D": D, "parts": parts}


def zone_reference(P, jvals, ivals=None, dtype=LD, mutate=None):
    P = np.asarray(P)
    if P.ndim == 2:
        P = P[:, :, None]
    return [zone_angle(P[:, :, a], jvals, ivals, dtype, mutate) for a in range(P.shape[2])]


def zone_bounds(r, c_marg, c_entry, u=U):
    """{name: bound}: c_marg for the sums over the (exact, integer) marginals, c_entry for the sums over the entries"""
    V, A, D, P = r["values"], r["A"], r["D"], r["parts"]
    f = lambda x: float(abs(x))
    B = {n: (c_entry if n in ZONE_ENTRY_SUMS else c_marg) * u * f(A[n]) for n in ZONE_NAMES}
    # the means carry c_marg u relative error, the difference (value - mean) one rounding of its larger operand
    # (D * delta to first order + delta^2: the weights sum to 1)
    di, dj = c_marg * u * f(P["ui"]) + u * f(P["maxi"]), c_marg * u * f(P["uj"]) + u * f(P["maxj"])
    B["GrayLevelVariance"] += f(D["GrayLevelVariance"]) * di + di ** 2
    B["SizeVariance"] += f(D["SizeVariance"]) * dj + dj ** 2
    return B


# ---- NGTDM ------------------------------------------------------------------------------------------------------------
def ngtdm_reference(P, dtype=LD, chunk=256):
    """P [Ng, 3] = (n_i, s_i, level value) -> dict(values, A, parts); the sums run over the levels with n_i > 0 only"""
    P = np.asarray(P).astype(dtype)
    keep = P[:, 0] > 0
    n_i, s_i, lv = P[keep, 0], P[keep, 1], P[keep, 2]
    ngp = int(keep.sum())
    nvp = n_i.sum(dtype=dtype)
    V, A = {}, {}
    if ngp == 0:
        return {"values": {k: dtype(np.nan) for k in NGTDM_NAMES}, "A": {}, "parts": {"ngp": 0}}
    p = n_i / nvp
    stot = s_i.sum(dtype=dtype)
    coarse = (p * s_i).sum(dtype=dtype)
    z = dtype(0)
    contrast = absdiff = absdiff_A = complexity = strength = z
    for a0 in range(0, ngp, chunk):
        pa, sa, la = p[a0:a0 + chunk, None], s_i[a0:a0 + chunk, None], lv[a0:a0 + chunk, None]
        pb, sb, lb = p[None, :], s_i[None, :], lv[None, :]
        d = la - lb
        contrast = contrast + (pa * pb * d ** 2).sum(dtype=dtype)
        absdiff = absdiff + np.abs(la * pa - lb * pb).sum(dtype=dtype)
        absdiff_A = absdiff_A + (np.abs(la * pa) + np.abs(lb * pb)).sum(dtype=dtype)
        complexity = complexity + (np.abs(d) * (pa * sa + pb * sb) / (pa + pb)).sum(dtype=dtype)
        strength = strength + ((pa + pb) * d ** 2).sum(dtype=dtype)
    div = dtype(ngp) * dtype(ngp - 1)
    V["Coarseness"] = 1 / coarse if coarse != 0 else dtype(1e6)
    V["Contrast"] = contrast * stot / nvp / div if div != 0 else z
    V["Busyness"] = coarse / absdiff if absdiff != 0 else z
    V["Complexity"] = complexity / nvp
    V["Strength"] = strength / stot if stot != 0 else z
    parts = {"ngp": ngp, "nvp": nvp, "stot": stot, "coarse": coarse, "contrast": contrast, "absdiff": absdiff,
             "absdiff_A": absdiff_A, "complexity": complexity, "strength": strength}
    return {"values": V, "A": A, "parts": parts}


def ngtdm_bounds(r, c_lin, c_pair, u=U):
    """{name: bound}.  All component sums have non-negative terms when s_i >= 0 (A = value) except the |i p_i - j p_j| of
    Busyness, whose terms cancel inside (A = sum (i p_i + j p_j)); c_lin for the sums over the levels, c_pair for those over
    the level pairs.  "cond" = value / bound of the divisors (coarse, absdiff, stot)."""
    V, P = r["values"], r["parts"]
    f = lambda x: float(abs(x))
    rel_coarse, rel_stot = c_lin * u, c_lin * u
    b_abs = c_pair * u * f(P["absdiff_A"])
    B, cond = {}, {}
    B["Coarseness"] = 0.0 if P["coarse"] == 0 else (rel_coarse + 2 * u) * f(V["Coarseness"])
    B["Contrast"] = (c_pair * u + rel_stot + 4 * u) * f(V["Contrast"])
    if P["absdiff"] == 0:
        B["Busyness"] = 0.0
    else:
        cond["absdiff"] = f(P["absdiff"]) / b_abs if b_abs else float("inf")
        B["Busyness"] = (rel_coarse + b_abs / f(P["absdiff"]) + 2 * u) * f(V["Busyness"])
    B["Complexity"] = (c_pair * u + 2 * u) * f(V["Complexity"])
    B["Strength"] = 0.0 if P["stot"] == 0 else (c_pair * u + rel_stot + 2 * u) * f(V["Strength"])
    return B, cond


def angle_mean(rows, empty):
    """what the reference reports: the empty angles deleted, nanmean over the rest (rows: [Na, F] array)"""
    rows = np.asarray(rows)
    kept = rows[~np.asarray(empty)]
    if kept.shape[0] == 0:
        return np.full(rows.shape[1], np.nan)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(kept, 0)

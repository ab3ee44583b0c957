"""TEST INFRASTRUCTURE ONLY -- the precise reference of the first-order statistics: a plain numpy restatement of what
prad_firstorder_dev returns (the 15 fields of engine.FIRSTORDER_FIELDS) and of the 19 voxel-mode features of
voxel_firstorder_kernel, with every sum in np.longdouble (64-bit significand on x86-64; integer images additionally
get their sum and their Energy from exact Python integers), and the comparison helper the GPU tests use.
oracle/firstorder_oracle.py stays the restatement that is pinned to the reference's recorded feature values;
tests/test_firstorder_reference.py pins this module to it, to exact fractions.Fraction arithmetic, and shows that the
comparison helper rejects subtly wrong results.

Definitions (x = the ROI intensities as float64, exact for int16 / int32 / float32 / float64 images; m = their number):
  * order statistics: np.sort and numpy's linear-interpolation rule -- virtual index (m - 1) q, prev = floor, next =
    prev + 1 (both clamped to [0, m - 1]), gamma = the fractional part, and numpy's _lerp in its `t >= 0.5` form;
    Median is the middle element or the mean of the middle pair.  All in float64, as numpy does it.
  * Mean is the float64 rounding of the long-double sum / m; MAD and the central moments m2, m3, m4 are taken about THAT
    float64 value (the reference package computes x - np.mean(x) with a float64 mean), not about the exact mean.
  * rMAD: the voxels with P10 <= x <= P90, mean absolute deviation from the float64 rounding of their own mean; NaN when
    no voxel lies in the band.
  * every summed field F = sum t comes with abs_sum[F] = sum |t| in long double, the terms being those of the field as
    returned (so the terms of Mean are x_i / m, those of m3 are (x_i - Mean)^3 / m, ...).

Error of the reference itself: np.sum of a long-double array is pairwise, so a sum of n terms is within
(log2 n + 3) * 2^-64 * abs_sum of the exact sum (test_firstorder_reference.py checks that against Fractions): 2^-11
times the unit 2^-53 * abs_sum the bounds below are written in, times at most 26.

Error bounds (seg_bounds / voxel_bounds), U = 2^-53.  k_sum is the longest chain of float64 additions a term of the
route's reductions passes through (the GPU test module derives it from the launch geometry), DIV = 1 the final division:
    Np, Minimum, Maximum, P10 .. P90, Median        0: they must be equal
    Energy                                          k_sum U abs_sum
    Mean                                            (k_sum + DIV) U abs_sum                          =: dmu
    MAD                                             (k_cen + DIV) U abs_sum + 1 dmu
    m_k (k = 2, 3, 4)                               (k_cen + DIV) U abs_sum + k dmu A_(k-1)
    rMAD                                            (k_cen + DIV) U abs_sum + 1 dmu_band
where A_j = sum |x_i - Mean|^j / m is the j-th absolute central moment (the first-order effect of the mean's own
rounding on a moment about it) and dmu_band = (k_cen + DIV) U sum_band |x_i| / m_band bounds the band mean.
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
DIV = 1
FIELDS = ("Np", "Energy", "Minimum", "P10", "P25", "Median", "P75", "P90", "Maximum", "Mean", "MAD", "rMAD",
          "m2", "m3", "m4")
EXACT = ("Np", "Minimum", "P10", "P25", "Median", "P75", "P90", "Maximum")
SUMMED = ("Energy", "Mean", "MAD", "rMAD", "m2", "m3", "m4")
QUANTILES = (("P10", 0.1), ("P25", 0.25), ("Median", 0.5), ("P75", 0.75), ("P90", 0.9))
VOXEL_EXACT = ("Minimum", "Maximum", "Median", "10Percentile", "90Percentile", "InterquartileRange", "Range")
VOXEL_FEATURES = ("Energy", "TotalEnergy", "Entropy", "Minimum", "10Percentile", "90Percentile", "Maximum", "Mean",
                  "Median", "InterquartileRange", "Range", "MeanAbsoluteDeviation", "RobustMeanAbsoluteDeviation",
                  "RootMeanSquared", "StandardDeviation", "Skewness", "Kurtosis", "Variance", "Uniformity")


def quantile_pos(m, q):
    """numpy's virtual index of quantile q among m sorted values -> (prev, next, gamma)"""
    virt = float(m - 1) * q
    prev = int(math.floor(virt))
    gamma = virt - float(prev)
    prev = min(max(prev, 0), m - 1)
    return prev, min(prev + 1, m - 1), gamma


def lerp_np(a, b, t):
    a, b = np.float64(a), np.float64(b)
    d = b - a
    return float(b - d * (1 - t)) if t >= 0.5 else float(a + d * t)


def order_ranks(m):
    """the ten ranks behind the five quantiles, ascending"""
    out = []
    for _, q in QUANTILES:
        p, n, _ = quantile_pos(m, q)
        out += [p, n]
    return out


def quantiles_of_sorted(xs, rank_shift=None):
    """{P10, P25, Median, P75, P90} of the sorted float64 array xs; rank_shift = (k, s) reads the k-th of the ten order
    statistics at its rank + s instead (the defect of tests/test_firstorder_reference.py)"""
    m = len(xs)
    out = {}
    for k, (name, q) in enumerate(QUANTILES):
        p, n, g = quantile_pos(m, q)
        r = [p, n]
        if rank_shift is not None and rank_shift[0] // 2 == k:
            r[rank_shift[0] % 2] = min(max(r[rank_shift[0] % 2] + rank_shift[1], 0), m - 1)
        a, b = xs[r[0]], xs[r[1]]
        if name == "Median":
            out[name] = float(a) if m % 2 else float((np.float64(a) + np.float64(b)) / 2.0)
        else:
            out[name] = lerp_np(a, b, g)
    return out


def _ld_sum(a):
    return LD(np.sum(np.asarray(a, dtype=LD))) if len(a) else LD(0)


def stats_of_values(x, shift=0.0, integer=False):
    """The reference of one set of ROI intensities x (1-D, any of the four dtypes): a dict with
    values {field: float}, abs_sum {summed field: long double}, absmom {j: long double A_j, j = 0..3},
    band_abs_mean (sum_band |x| / m_band), m, distinct (number of distinct values), sorted (float64), zero_signs.
    Sums run over the distinct values times their exact counts (a count times a term is one more long-double rounding)."""
    x = np.asarray(x).ravel()
    m = int(x.size)
    assert m >= 1
    xs = np.sort(x.astype(np.float64))
    zeros = np.flatnonzero(xs == 0)                   # -0.0 sorts before +0.0 (np.sort leaves them in input order)
    if len(zeros):
        neg = int(np.signbit(xs[zeros]).sum())
        xs[zeros[:neg]], xs[zeros[neg:]] = -0.0, 0.0
        zero_signs = ({-1} if neg else set()) | ({1} if len(zeros) > neg else set())
    else:
        zero_signs = set()
    first = np.concatenate(([True], xs[1:] != xs[:-1]))
    v = xs[first].astype(LD)
    w = np.diff(np.concatenate((np.flatnonzero(first), [m]))).astype(LD)
    sh = LD(shift)
    if integer and float(shift).is_integer():
        vi, wi = [int(a) for a in xs[first].tolist()], [int(c) for c in w.tolist()]
        sum_x = LD(sum(a * c for a, c in zip(vi, wi)))                      # exact Python integers, rounded once
        energy = LD(sum((a + int(shift)) ** 2 * c for a, c in zip(vi, wi)))
    else:
        y = v + sh
        sum_x, energy = _ld_sum(w * v), _ld_sum(w * (y * y))
    mean = float(sum_x / LD(m))
    d = v - LD(mean)
    ad, d2 = np.abs(d), d * d
    a3 = _ld_sum(w * (d2 * ad)) / m
    m4 = _ld_sum(w * (d2 * d2)) / m
    absmom = {0: LD(1), 1: _ld_sum(w * ad) / m, 2: _ld_sum(w * d2) / m, 3: a3}
    vals = {"Np": float(m), "Energy": float(energy), "Minimum": float(xs[0]), "Maximum": float(xs[-1]), "Mean": mean,
            "MAD": float(absmom[1]), "m2": float(absmom[2]), "m3": float(_ld_sum(w * (d2 * d)) / m), "m4": float(m4)}
    vals.update(quantiles_of_sorted(xs))
    abs_sum = {"Energy": energy, "Mean": _ld_sum(w * np.abs(v)) / m, "MAD": absmom[1], "m2": absmom[2], "m3": a3, "m4": m4}
    inb = (xs[first] >= vals["P10"]) & (xs[first] <= vals["P90"])
    vb, wb = v[inb], w[inb]
    band_abs_mean = LD(0)
    if len(vb):
        mb = _ld_sum(wb)
        mub = float(_ld_sum(wb * vb) / mb)
        r = _ld_sum(wb * np.abs(vb - LD(mub))) / mb
        vals["rMAD"], abs_sum["rMAD"] = float(r), r
        band_abs_mean = _ld_sum(wb * np.abs(vb)) / mb
    else:
        vals["rMAD"], abs_sum["rMAD"] = float("nan"), LD(0)
    return {"values": vals, "abs_sum": abs_sum, "absmom": absmom, "band_abs_mean": band_abs_mean, "m": m,
            "distinct": int(len(v)), "sorted": xs, "zero_signs": zero_signs}


def segment_reference(image, mask, shift=0.0):
    image = np.asarray(image)
    return stats_of_values(image[np.asarray(mask).astype(bool)], shift, np.issubdtype(image.dtype, np.integer))


def seg_bounds(ref, k_sum, k_cen=None):
    """{field: bound on |got - ref|} by the rules of the module docstring (0 for the fields that must be equal)"""
    k_cen = k_sum if k_cen is None else k_cen
    A, M = ref["abs_sum"], ref["absmom"]
    dmu = (k_sum + DIV) * U * float(A["Mean"])
    dmub = (k_cen + DIV) * U * float(ref["band_abs_mean"])
    c = (k_cen + DIV) * U
    b = {f: 0.0 for f in EXACT}
    b["Energy"] = k_sum * U * float(A["Energy"])
    b["Mean"] = dmu
    b["MAD"] = c * float(A["MAD"]) + dmu
    b["rMAD"] = c * float(A["rMAD"]) + dmub
    for k in (2, 3, 4):
        b["m%d" % k] = c * float(A["m%d" % k]) + k * dmu * float(M[k - 1])
    return b


def compare(got, ref, bounds, exact=EXACT):
    """-> (violations, ratios): violations = [(field, got, want, error, bound)] of the fields outside their bound (equal
    fields: any difference, the sign of a zero included; a NaN must sit exactly where the reference's is), ratios =
    {field: error / bound} of the bounded fields.  Only where the ROI holds BOTH -0.0 and +0.0 is the sign of a zero order
    statistic left open: numpy's own sort leaves the two in input order, so the reference package does not define it."""
    want = ref["values"] if "values" in ref else ref
    open_sign = "values" in ref and len(ref.get("zero_signs", ())) == 2
    bad, ratios = [], {}
    if set(got) != set(want):
        return [("fields", sorted(got), sorted(want), None, None)], ratios
    for f, w in want.items():
        g = float(got[f])
        if math.isnan(w) or math.isnan(g):
            if math.isnan(w) != math.isnan(g):
                bad.append((f, g, w, float("nan"), 0.0))
            continue
        err = abs(float(LD(g) - LD(w)))
        if f in exact:
            if g != w or (not open_sign and math.copysign(1.0, g) != math.copysign(1.0, w)):
                bad.append((f, g, w, err, 0.0))
            continue
        bd = bounds[f]
        if err > bd:
            bad.append((f, g, w, err, bd))
        if bd > 0:
            ratios[f] = err / bd
        elif err > 0:
            ratios[f] = float("inf")
    return bad, ratios


# ---- voxel mode --------------------------------------------------------------------------------------------------------
def window_half(shape, bbsize, kernelRadius, force2D=False, force2Ddimension=0):
    """per-dimension half width of the kernel window (prad_voxel_firstorder_dev)"""
    half = []
    for d, n in enumerate(shape):
        h = min(kernelRadius, max(int(bbsize[d]) - 1, 0), n - 1)
        half.append(0 if force2D and d == force2Ddimension else h)
    return half


def voxel_reference(image, mask, levels, centre, half, shift=0.0, voxel_volume=1.0):
    """The 19 features of the window around `centre` -> (values {name: float}, parts): the ROI voxels of the window in
    raster order of the offsets, statistics as in stats_of_values, Entropy / Uniformity from the level multiplicities.
    parts carries what voxel_bounds needs."""
    image, mask = np.asarray(image), np.asarray(mask).astype(bool)
    sl = tuple(slice(max(c - h, 0), min(c + h + 1, n)) for c, h, n in zip(centre, half, image.shape))
    sel = mask[sl]
    x = image[sl][sel]
    st = stats_of_values(x, shift, np.issubdtype(image.dtype, np.integer))
    v, m = st["values"], st["m"]
    lev = np.asarray(levels)[sl][sel]
    _, inv, cnt = np.unique(lev, return_inverse=True, return_counts=True)
    p = (cnt.astype(LD) / LD(m))
    eps = LD(np.spacing(1.0))
    lg = np.log2(p + eps)
    ent_terms = (p * lg)
    m2 = LD(st["absmom"][2])
    m2s = LD(1) if v["m2"] == 0 else LD(v["m2"])
    out = {"Energy": v["Energy"], "TotalEnergy": float(LD(v["Energy"]) * LD(voxel_volume)),
           "Entropy": float(-_ld_sum(ent_terms)), "Minimum": v["Minimum"], "10Percentile": v["P10"],
           "90Percentile": v["P90"], "Maximum": v["Maximum"], "Mean": v["Mean"], "Median": v["Median"],
           "InterquartileRange": float(np.float64(v["P75"]) - np.float64(v["P25"])),
           "Range": float(np.float64(v["Maximum"]) - np.float64(v["Minimum"])), "MeanAbsoluteDeviation": v["MAD"],
           "RobustMeanAbsoluteDeviation": v["rMAD"], "RootMeanSquared": float(np.sqrt(LD(v["Energy"]) / m)),
           "StandardDeviation": float(np.sqrt(m2)), "Variance": float(m2),
           "Skewness": float(LD(v["m3"]) / m2s ** LD(1.5)), "Kurtosis": float(LD(v["m4"]) / (m2s * m2s)),
           "Uniformity": float(_ld_sum(p * p))}
    st["entropy_abs"] = _ld_sum(np.abs(ent_terms))
    st["uniformity_abs"] = _ld_sum(p * p)
    return out, st


def derived_bounds(v, b, extra_u=4):
    """bounds of the class's derived features from the bounds b of the fields v they are formed from, to first order, plus
    extra_u U relative for the roundings of the formula itself (sqrt / pow / product / quotient: at most 4)"""
    out = {}
    m2 = v["m2"]
    e, npx = v["Energy"], v["Np"]
    rms = math.sqrt(e / npx) if npx else 0.0
    out["RootMeanSquared"] = (0.5 * rms * b["Energy"] / e if e > 0 else 0.0) + extra_u * U * rms
    out["Variance"] = b["m2"] + extra_u * U * m2
    sd = math.sqrt(m2)
    out["StandardDeviation"] = (0.5 * b["m2"] / sd if sd > 0 else 0.0) + extra_u * U * sd
    if m2 == 0:
        out["Skewness"] = out["Kurtosis"] = 0.0           # flat region: both are 0 by rule
    else:
        sk, ku = v["m3"] / m2 ** 1.5, v["m4"] / m2 ** 2
        out["Skewness"] = b["m3"] / m2 ** 1.5 + 1.5 * abs(sk) * b["m2"] / m2 + extra_u * U * abs(sk)
        out["Kurtosis"] = b["m4"] / m2 ** 2 + 2.0 * abs(ku) * b["m2"] / m2 + extra_u * U * abs(ku)
    return out


def voxel_bounds(values, st, k, voxel_volume=1.0):
    """{feature: bound} of one centre; k = the per-lane serial length + the 6 shuffle steps"""
    b = seg_bounds(st, k, k)
    v = st["values"]
    out = {f: 0.0 for f in VOXEL_EXACT}
    out.update(derived_bounds(v, b))
    out["Energy"] = b["Energy"]
    out["TotalEnergy"] = b["Energy"] * voxel_volume + U * abs(values["TotalEnergy"])
    out["Mean"], out["MeanAbsoluteDeviation"], out["RobustMeanAbsoluteDeviation"] = b["Mean"], b["MAD"], b["rMAD"]
    out["Entropy"] = (k + DIV) * U * float(st["entropy_abs"])
    out["Uniformity"] = (k + DIV) * U * float(st["uniformity_abs"])
    return out


# ---- launch geometry of prad_firstorder_dev -> k_sum ---------------------------------------------------------------------
def k_reduction(n, itemsize):
    """Longest chain of float64 additions one term passes through in fo_sums_kernel / fo_central_kernel / fo_band_kernel
    over an array of n voxels (prad_firstorder.hip): blocks = min(ceil(n / 256), PRAD_FO_BLOCKS = 1024) workgroups of 256
    threads; thread t of the T = 256 blocks takes the 16-byte pieces t, t + T, ... (E = 16 / itemsize voxels each, added one
    after the other) and at most one voxel of the tail; then 6 __shfl_xor steps, the 3 additions of
    sh[0] + sh[1] + sh[2] + sh[3], and the host's serial sum over the blocks."""
    E = 16 // itemsize
    blocks = max(1, min((n + 255) // 256, 1024))
    T = 256 * blocks
    serial = E * -(-(n // E) // T) + (1 if n % E else 0)
    return serial + 6 + 3 + blocks


# ---- the segment-mode case families (shared by the CPU comparator tests and the GPU tests) --------------------------------
BINS = 16384                   # PRAD_FO_BINS
BIG = (64, 128, 129)           # 1 056 768 voxels: the smallest volume here that holds 2^20 ROI voxels
MID = (16, 64, 65)             # 66 560 voxels: holds 2^16
_cache = {}


def mask_with_count(shape, count, seed):
    n = int(np.prod(shape))
    m = np.zeros(n, dtype=bool)
    m[np.random.default_rng(seed).permutation(n)[:count]] = True
    return m.reshape(shape)


def _fill(shape, count, values, seed, outside=0):
    """volume whose `count` ROI voxels (random positions) hold `values` in random order; a run of ties across the ranks of
    P10 is cut between them (the values after the prev rank move up to the next distinct value), so that an order statistic
    read one rank off is a different number"""
    mask = mask_with_count(shape, count, seed)
    values = np.sort(np.asarray(values))
    p = quantile_pos(count, 0.1)[0]
    hi = int(np.searchsorted(values, values[p], "right"))
    if p + 1 < hi < count:
        values[p + 1:hi] = values[hi]
    img = np.full(shape, outside, dtype=values.dtype)
    img[mask] = np.random.default_rng(seed + 1).permutation(values)
    return img, mask


def _ints(dtype, shape, count, seed, lo=-900, hi=15000):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi, int(np.prod(shape))).astype(dtype).reshape(shape), mask_with_count(shape, count, seed + 7)


def _floats(dtype, shape, count, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 37.5 + 11).astype(dtype), mask_with_count(shape, count, seed + 7)


def _ten_bins():
    """sorted values r / (m - 1) on [0, 1] (scale = 16384 exactly); at every quantile the prev rank is moved to just below
    the next bin edge and the ranks after it up to that edge onto the edge: prev and next lie in adjacent bins, the ten ranks
    in ten different bins"""
    m = 1 << 20
    xs = np.arange(m, dtype=np.float64) / (m - 1)
    for _, q in QUANTILES:
        p, _, _ = quantile_pos(m, q)
        edge = (math.floor(xs[p] * BINS) + 1) / BINS
        hi = int(np.searchsorted(xs, edge, "left"))
        xs[p] = np.nextafter(edge, 0.0)
        xs[p + 1:hi] = edge
    assert np.all(np.diff(xs) >= 0)
    return xs


def _ties_at_ranks():
    """piecewise constant: every tie group ends on a prev rank, the next rank opens the next group"""
    m = 1 << 20
    xs = np.empty(m, dtype=np.float64)
    start = 0
    for k, (_, q) in enumerate(QUANTILES):
        p, _, _ = quantile_pos(m, q)
        xs[start:p + 1] = 3.0 * k + 1.25
        start = p + 1
    xs[start:] = 40.5
    return xs


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    f64, f32, i16, i32 = np.float64, np.float32, np.int16, np.int32
    S, X, Q, E = "firstorder-sort", "firstorder-exact", "firstorder-select", None
    two20 = 1 << 20
    # -- route boundaries
    if name in ("b16-sort-i16", "b16-exact-i16", "b16-sort-i32", "b16-exact-i32"):
        img, mask = _ints(i16 if name.endswith("i16") else i32, MID, 65535 + ("exact" in name), 11)
        return img, mask, 0.0, X if "exact" in name else S
    if name in ("range-32767", "range-32768"):
        R = int(name[-5:])
        vals = rng.integers(-1000, -1000 + R + 1, 1 << 16).astype(i32)
        vals[0], vals[1] = -1000, -1000 + R
        img, mask = _fill(MID, 1 << 16, vals, 12, outside=10 ** 6)
        return img, mask, 3.0, X if R == 32767 else S
    if name in ("b20-sort-f64", "b20-select-f64", "b20-sort-f32", "b20-select-f32"):
        img, mask = _floats(f64 if name.endswith("f64") else f32, BIG, two20 - 1 + ("select" in name), 13)
        return img, mask, 0.0, Q if "select" in name else S
    if name in ("const-f64", "const-f32"):
        img = np.full(BIG, 7.5, dtype=f64 if name.endswith("f64") else f32)
        return img, np.ones(BIG, dtype=bool), 2.0, S
    if name == "const-i16":
        return np.full(MID, -3, dtype=i16), np.ones(MID, dtype=bool), 0.0, X
    # -- selection, adversarial
    if name == "sel-edges":             # every value on a bin edge vmin + k (vmax - vmin) / 16384, both extremes present
        k = rng.integers(0, BINS + 1, two20)
        k[0], k[1] = 0, BINS
        img, mask = _fill(BIG, two20, -3.0 + k * (1638.4 / BINS), 21, outside=1e30)
        return img, mask, 0.0, Q
    if name == "sel-ulp":               # one ulp either side of an edge, and on it
        k = rng.integers(1, BINS, two20).astype(f64)
        v = k * (1.0 / BINS) * 5.0
        side = rng.integers(0, 3, two20)
        v = np.where(side == 0, np.nextafter(v, -np.inf), np.where(side == 1, np.nextafter(v, np.inf), v))
        v[0], v[1] = 0.0, 5.0
        img, mask = _fill(BIG, two20, v, 22, outside=-1e30)
        return img, mask, 0.0, Q
    if name == "sel-vmax":              # a fifth of the ROI equals vmax: P90's ranks lie in the last bin
        v = rng.random(two20) * 10.0
        v[: two20 // 5] = 10.0
        img, mask = _fill(BIG, two20, v, 23)
        return img, mask, 1.0, Q
    if name == "sel-ten-bins":
        img, mask = _fill(BIG, two20, _ten_bins(), 24, outside=5.0)
        return img, mask, 0.0, Q
    if name == "sel-one-bin":           # all ten ranks in ONE bin of many distinct values (gathered and sorted whole)
        v = 0.5 + rng.random(two20) * (0.9 / BINS)
        v[0], v[1] = 0.0, 1.0
        img, mask = _fill(BIG, two20, v, 25)
        return img, mask, 0.0, Q
    if name == "sel-ties":
        img, mask = _fill(BIG, two20, _ties_at_ranks(), 26, outside=-7.0)
        return img, mask, 0.0, Q
    if name == "sel-outlier-many":      # more than 2^22 distinct values share bin 0: no selection, the sort takes over
        n = (1 << 22) + 16384
        v = rng.standard_normal(n) + 50.0
        v[12345] = 1e9
        mask = np.ones(n, dtype=bool)
        mask[::1000] = False
        mask[12345] = True
        return v, mask, 0.0, S
    if name == "sel-outlier-single":    # more than 2^22 voxels in bin 0, all equal: no gather, still the selection
        n = (1 << 22) + 16384
        v = np.full(n, 2.5, dtype=f32)
        v[777] = 1e9
        mask = np.ones(n, dtype=bool)
        mask[::777] = False
        mask[777] = True
        return v, mask, 0.0, Q
    if name == "sel-zeros-subnormals":  # float32: signed zeros, subnormals and small normals
        tiny = np.float32(1e-45)
        pool = np.array([-0.0, 0.0, tiny, -tiny, 3 * tiny, 1e-40, -2e-40, 1.5e-38, 4e-38], dtype=f32)
        v = pool[rng.integers(0, len(pool), two20)]
        img, mask = _fill(BIG, two20, v, 27)
        return img, mask, 0.0, Q
    # -- cancellation
    if name == "can-f64-1e8":
        shape = (9, 10, 11)
        return 1e8 + rng.standard_normal(shape) * 1e-3, mask_with_count(shape, 900, 31), 0.0, S
    if name == "can-f32-2p24":
        img, mask = _fill((9, 10, 11), 901, (16777216.0 + rng.integers(0, 3, 901)).astype(f32), 32, outside=16777216.0)
        return img, mask, 0.0, S
    if name in ("can-i32-max", "can-i32-min"):
        sgn = 1 if name.endswith("max") else -1
        v = (sgn * (2 ** 31 - 1 - rng.integers(0, 1001, two20))).astype(i32)
        img, mask = _fill(BIG, two20, v, 33)
        return img, mask, 0.0, X
    if name == "can-shift":             # voxelArrayShift = -mean: Energy is a sum of small squares
        shape = (9, 10, 11)
        img, mask = 1000.0 + rng.standard_normal(shape), mask_with_count(shape, 800, 34)
        return img, mask, -float(np.mean(img[mask])), S
    if name in ("can-two-valued-f64", "can-two-valued-i16"):      # 1 : 10^6 split
        n = 10 ** 6 + 1
        v = np.zeros(n, dtype=f64 if name.endswith("f64") else i16)
        v[n // 3] = 3
        return v, np.ones(n, dtype=bool), 0.0, S if name.endswith("f64") else X
    # -- rank placement / alignment representatives for the comparator tests
    if name == "rank-21":
        n = 1027
        img = (rng.standard_normal(n) * 37.5 + 11)
        mask = np.zeros(n, dtype=bool)
        mask[np.linspace(0, n - 1, 21).astype(int)] = True
        return img, mask, 0.0, S
    if name == "align-f32":
        n = 5003
        return (rng.standard_normal(n) * 37.5 + 11).astype(f32), rng.random(n) < 0.6, 1.0, S
    raise KeyError(name)


BOUNDARY = ("b16-sort-i16", "b16-exact-i16", "b16-sort-i32", "b16-exact-i32", "range-32767", "range-32768",
            "b20-sort-f64", "b20-select-f64", "b20-sort-f32", "b20-select-f32", "const-f64", "const-f32", "const-i16")
SELECTION = ("sel-edges", "sel-ulp", "sel-vmax", "sel-ten-bins", "sel-one-bin", "sel-ties", "sel-outlier-many",
             "sel-outlier-single", "sel-zeros-subnormals")
CANCELLATION = ("can-f64-1e8", "can-f32-2p24", "can-i32-max", "can-i32-min", "can-shift", "can-two-valued-f64",
                "can-two-valued-i16")
SMALL = ("rank-21", "align-f32")


def case(name):
    """(image, mask, shift, route) of a named case, built once per process and never modified"""
    if name not in _cache:
        img, mask, shift, route = _build(name)
        img.setflags(write=False)
        mask.setflags(write=False)
        _cache[name] = (img, mask, shift, route)
    return _cache[name]


def case_reference(name):
    key = ("ref", name)
    if key not in _cache:
        img, mask, shift, _ = case(name)
        _cache[key] = segment_reference(img, mask, shift)
    return _cache[key]


def case_k(name, route=None):
    """(k_sum, k_cen) of a case on its route: the exact-histogram route sums over the distinct values"""
    img, _, _, r = case(name)
    k = k_reduction(img.size, img.dtype.itemsize)
    return (k, case_reference(name)["distinct"]) if (route or r) == "firstorder-exact" else (k, k)

"""Independent long-double restatement of the filter stack (test helper, not a test): what the wavelet and Laplacian-of-Gaussian
entry points (engine.swt_level1, engine.wavelet_images, filters.getWaveletImage, engine.log_image(s), filters.getLoGImage,
filters.laplacian_recursive_gaussian) have to return.

Nothing here imports pyradiomics_amd or oracle.  Everything is numpy over whole arrays in np.longdouble, which must have a 64-bit
significand (`AVAILABLE`; the tests skip with `SKIP_REASON` otherwise, there is no fallback).  Wavelet taps are handed in as
float64 arrays (`use_taps`): the same numbers the device gets, so no tap error enters a comparison.

Wavelet (`swt_axis`, `swtn`, `swt3`)
  out[o] = sum_k f[k] x[(o + F/2 - k) mod N] per axis in long double; bands are built axis by axis in the order of `axes`, keys
  as PyWavelets names them ('a' / 'd' appended per axis); swt3 pads odd axes by one wrapped sample, re-applies the transform to
  the approximation per level and crops.
  Bound (`wavelet_bound`), derived, not tuned.  u = 2^-53, g = F u / (1 - F u) (gamma_F).  One float64 pass computes F unfused
  products and F adds from 0.0: its result differs from the exact sum by at most g sum_k |f[k] x[.]| <= g S max|x|, where
  S = max(sum |dec_lo|, sum |dec_hi|) (equal for a quadrature pair).  Let the exact values after j passes be bounded by S^j M
  (M = max |x| of the input) and the computed ones carry the error e_j.  A pass multiplies the incoming error by at most S and
  adds its own rounding of values bounded by (1 + g)^(j-1) S^(j-1) M:
      e_j <= S e_(j-1) + g S (1 + g)^(j-1) S^(j-1) M   =>   e_j <= ((1 + g)^j - 1) S^j M          (induction, e_0 = 0)
  which is j F u S^j M to first order.  A level of p axes is p passes; level l (counting the start levels too) takes the
  approximation of level l - 1 as its input, whose exact values are bounded by S^(p (l-1)) M and which carries e_(p (l-1)):
  the same induction runs on, e = ((1 + g)^(p l) - 1) S^(p l) M for every band of level l.  The long-double reference's own
  rounding is 2^-11 of that and is left out.  Conversions to float64 are exact for every type of the case table.

LoG (`restated`)
  Coefficients N, D, M, BN, BM of orders 0 and 2 from the published ITK formulas (RecursiveGaussianImageFilter::SetUp, Deriche's
  recursion with the constants of Farneback & Westin), with NormalizeAcrossScale, evaluated in long double.  The line recursion
  (RecursiveSeparableImageFilter::FilterDataArray) runs in long double with the edge-replicating start at both ends; each 1-D
  pass is rounded ONCE to float32.  Per dimension in ITK order (x, y, z = array axes nd-1 .. 0) the derivative pass runs first
  on the input widened exactly, then the smoothing passes of the other dimensions in increasing ITK direction.  The accumulation
  step is specified in IEEE terms and performed in exactly those float64 operations, not in long double:
      acc = f32( f64(acc) + f64(term) / f64(sp * sp) )
  (its double rounding is part of what ITK computes).  The result is cast to the output type: float64 for a float64 image,
  float32 for every other one.
  Decision points: a voxel of a pass is FLAGGED when its long-double line value lies within r of a float32 rounding tie (the
  middle of two neighbouring float32 values).  r is measured per case and pass: 16 times the largest distance between the
  long-double line values and those of a float64 evaluation of the same recursion on the same input (`flags` takes that
  evaluation as a callable; tests/test_filters_reference.py hands it oracle/filters_oracle._filter_lines, which is not the code
  under test).  16 allows any other association of a step's sixteen float64 operations.  r is one absolute number per pass, so a
  line value far below the pass's largest is always flagged: pure steps and impulses, whose tails decay exponentially, therefore
  ride on noise of unit scale here.  Condition on the case table, asserted on the CPU: no case has a flagged voxel in any pass
  (`RESEED` holds the cases whose first seed had one), and with it the comparison with the device is plain equality of bits.
  The condition cannot be met everywhere: 29 of the 738 (case, sigma) pairs keep flagged voxels under every seed, because
  there float64 arithmetic itself is up to 0.04 float32 ulp away from long double (`UNDECIDED`, with the reasons).  Those
  pairs are compared bit for bit with the float64 restatement instead; no mutation is shown on them.

`mutate=` reproduces ONE hazard in this model (`WAVELET_MUTATIONS`, `LOG_MUTATIONS`); tests/test_filters_reference.py shows that
the family of cases that exists for it notices (`HAZARDS` there).

The case table (`CASES`, `GROUPS`, `case`, `reference`) is shared by tests/test_filters_reference.py (CPU) and
tests/test_gpu_filter_limits.py; `assert_case` and `report` are at the end.
"""
from __future__ import annotations

import functools
import math
import zlib

import numpy as np

LD = np.longdouble
AVAILABLE = bool(np.finfo(LD).eps <= 2.0 ** -63)
SKIP_REASON = "np.longdouble has no 64-bit significand here (eps %.3g > 2^-63): no reference" % float(np.finfo(LD).eps)

U = 2.0 ** -53
MAX_TAPS = 32
LINE_FOLD = 65535                    # lines per blockIdx.z of the contiguous wavelet pass
GRID_CAP = 8192 * 256                # threads of the general wavelet kernel's capped grid
BLOCK = 16                           # samples per block of the LoG pass kernel

WAVELET_MUTATIONS = ("one-wrap", "centre", "reversed", "swapped", "z-first", "float32-stage", "line-alias", "lost-tail")
LOG_MUTATIONS = ("smooth-first", "float64-between", "float32-input", "single-rounding", "zero-causal-start",
                 "zero-anticausal-start", "second-start", "block-restart", "normalize-flipped", "spacing-xyz")

_TAPS = {"fn": None}


def use_taps(fn):
    """fn(name) -> (dec_lo, dec_hi) float64: the tabulated filters, handed in by the test modules"""
    _TAPS["fn"] = fn


def custom_taps(F, seed=5):
    """a (dec_lo, dec_hi) pair of F arbitrary taps (quadrature rule for dec_hi)"""
    lo = np.random.default_rng(seed).standard_normal(F) / 4.0
    hi = np.array([(-1) ** (k + 1) * lo[F - 1 - k] for k in range(F)])
    return lo, hi


def taps(wavelet):
    if isinstance(wavelet, tuple):
        return np.asarray(wavelet[0], dtype=np.float64), np.asarray(wavelet[1], dtype=np.float64)
    if wavelet.startswith("custom"):
        return custom_taps(int(wavelet[6:]))
    lo, hi = _TAPS["fn"](wavelet)
    return np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)


# ---- wavelet -------------------------------------------------------------------------------------------------------------
def swt_axis(x, f, axis, mutate=None):
    x = np.asarray(x, dtype=LD)
    N, F = x.shape[axis], len(f)
    f = np.asarray(f, dtype=LD)
    if mutate == "reversed":
        f = f[::-1]
    centre = F // 2 - (1 if mutate == "centre" else 0)
    o = np.arange(N)
    out = np.zeros_like(x)
    for k in range(F):
        p = o + centre - k
        if mutate == "one-wrap":
            p = np.where(p < 0, p + N, np.where(p >= N, p - N, p))
            p = np.clip(p, 0, N - 1)
        else:
            p = np.mod(p, N)
        out = out + f[k] * np.take(x, p, axis=axis)
    if mutate == "line-alias" and axis == x.ndim - 1:
        lines = out.reshape(-1, N)
        if lines.shape[0] > LINE_FOLD:
            lines = lines.copy()
            lines[LINE_FOLD:] = lines[:lines.shape[0] - LINE_FOLD]
            out = lines.reshape(out.shape)
    if mutate == "lost-tail" and out.size > GRID_CAP:
        flat = out.reshape(-1).copy()
        flat[GRID_CAP:] = 0
        out = flat.reshape(out.shape)
    return out


def swtn(data, lo, hi, axes, mutate=None):
    """dict key -> long-double array, keys in PyWavelets' insertion order"""
    x = np.asarray(data)
    if mutate == "float32-stage":
        x = x.astype(np.float32)
    if mutate == "swapped":
        lo, hi = hi, lo
    coeffs = {"": x.astype(LD)}
    for ax in axes:
        nxt = {}
        for key, c in coeffs.items():
            a, d = swt_axis(c, lo, ax, mutate), swt_axis(c, hi, ax, mutate)
            if mutate == "z-first":
                nxt["a" + key], nxt["d" + key] = a, d
            else:
                nxt[key + "a"], nxt[key + "d"] = a, d
        coeffs = nxt
    return coeffs


def swt3(array, wavelet, level=1, start_level=0, axes=None, mutate=None):
    """-> (approximation, [dict name -> array per level]) in long double; names with L / H"""
    arr = np.asarray(array)
    if axes is None:
        axes = tuple(range(arr.ndim - 1, -1, -1))
    lo, hi = taps(wavelet)
    data = np.pad(arr, tuple((0, 1 if d % 2 else 0) for d in arr.shape), "wrap")
    crop = tuple(slice(0, d) for d in arr.shape)
    ak = "a" * len(axes)
    for _ in range(start_level):
        data = swtn(data, lo, hi, axes, mutate)[ak]
    ret = []
    for _ in range(level):
        dec = swtn(data, lo, hi, axes, mutate)
        data = dec[ak]
        ret.append({k.replace("a", "L").replace("d", "H"): v[crop] for k, v in dec.items() if k != ak})
    return data[crop], ret


def swt3_fused_float64(name):
    """a small level-1 wavelet case in float64 with ONE rounding per tap (s = fma(f[k], x, s), exact rationals rounded once):
    what a compiler that contracts multiply and add computes.  -> (approximation, [dict]) of float64 arrays"""
    from fractions import Fraction
    s = CASES[name]
    lo, hi = taps(s["wavelet"])
    x = case(name)
    data = np.pad(x, tuple((0, 1 if d % 2 else 0) for d in x.shape), "wrap").astype(np.float64)

    def one(c, f, axis):
        m = np.moveaxis(c, axis, -1)
        out = np.zeros_like(m)
        N, F = m.shape[-1], len(f)
        ff = [Fraction(float(t)) for t in f]
        for idx in np.ndindex(m.shape[:-1]):
            line = [Fraction(float(v)) for v in m[idx]]
            for o in range(N):
                acc = 0.0
                for k in range(F):
                    acc = float(ff[k] * line[(o + F // 2 - k) % N] + Fraction(acc))
                out[idx][o] = acc
        return np.moveaxis(out, -1, axis)
    coeffs = {"": data}
    for ax in s["axes"]:
        coeffs = {k + c: one(v, f, ax) for k, v in coeffs.items() for c, f in (("L", lo), ("H", hi))}
    crop = tuple(slice(0, d) for d in x.shape)
    coeffs = {k: v[crop] for k, v in coeffs.items()}
    approx = coeffs.pop("L" * len(s["axes"]))
    return approx, [coeffs]


def wavelet_bound(lo, hi, passes, M):
    """((1 + gamma_F)^passes - 1) S^passes M: see the module docstring"""
    F = len(lo)
    S = max(float(np.abs(lo).sum()), float(np.abs(hi).sum()))
    g = F * U / (1.0 - F * U)
    return math.expm1(passes * math.log1p(g)) * S ** passes * M


def log_name(sigma):
    return "log-sigma-%s-mm-3D" % str(sigma).replace(".", "-")


def band_names(naxes, level_index, nlevels):
    """names and yield order of getWaveletImage for one level (1-based) -- the approximation is not among them"""
    keys = [""]
    for _ in range(naxes):
        keys = [k + c for k in keys for c in "LH"]
    pre = "wavelet-" if level_index == 1 else "wavelet%d-" % level_index
    return [pre + k for k in keys if k != "L" * naxes]


# ---- LoG -----------------------------------------------------------------------------------------------------------------
_W1, _L1, _W2, _L2 = LD("0.6681"), LD("-1.3932"), LD("2.0787"), LD("-1.3732")
_A1 = (LD("1.3530"), LD("-0.6724"), LD("-1.3563"))
_B1 = (LD("1.8151"), LD("-3.4327"), LD("5.2318"))
_A2 = (LD("-0.3531"), LD("0.6724"), LD("0.3446"))
_B2 = (LD("0.0902"), LD("0.6100"), LD("-2.2355"))


def _n_coef(sd, A1, B1, A2, B2):
    s1, s2, c1, c2 = np.sin(_W1 / sd), np.sin(_W2 / sd), np.cos(_W1 / sd), np.cos(_W2 / sd)
    e1, e2 = np.exp(_L1 / sd), np.exp(_L2 / sd)
    N0 = A1 + A2
    N1 = e2 * (B2 * s2 - (A2 + 2 * A1) * c2) + e1 * (B1 * s1 - (A1 + 2 * A2) * c1)
    N2 = 2 * e1 * e2 * ((A1 + A2) * c2 * c1 - (B1 * c2 * s1 + B2 * c1 * s2)) + A2 * e1 * e1 + A1 * e2 * e2
    N3 = e2 * e1 * e1 * (B2 * s2 - A2 * c2) + e1 * e2 * e2 * (B1 * s1 - A1 * c1)
    N = (N0, N1, N2, N3)
    return N, N0 + N1 + N2 + N3, N1 + 2 * N2 + 3 * N3, N1 + 4 * N2 + 9 * N3


@functools.lru_cache(maxsize=None)
def coefficients(sigma, spacing, order, normalize):
    """dict N, D, M, BN, BM (4 long doubles each) of a symmetric filter of order 0 or 2; sigma and spacing are float64 values"""
    sigma, spacing = LD(float(sigma)), LD(abs(float(spacing)))
    sd = sigma / spacing
    c1, c2, e1, e2 = np.cos(_W1 / sd), np.cos(_W2 / sd), np.exp(_L1 / sd), np.exp(_L2 / sd)
    D = (-2 * (e2 * c2 + e1 * c1), 4 * c2 * c1 * e1 * e2 + e1 * e1 + e2 * e2,
         -2 * c1 * e1 * e2 * e2 - 2 * c2 * e2 * e1 * e1, e1 * e1 * e2 * e2)
    SD = 1 + D[0] + D[1] + D[2] + D[3]
    DD = D[0] + 2 * D[1] + 3 * D[2] + 4 * D[3]
    ED = D[0] + 4 * D[1] + 9 * D[2] + 16 * D[3]
    if order == 0:
        N, SN, _, _ = _n_coef(sd, _A1[0], _B1[0], _A2[0], _B2[0])
        alpha0 = 2 * SN / SD - N[0]
        N = tuple(n / alpha0 for n in N)
    elif order == 2:
        N0s, SN0, DN0, EN0 = _n_coef(sd, _A1[0], _B1[0], _A2[0], _B2[0])
        N2s, SN2, DN2, EN2 = _n_coef(sd, _A1[2], _B1[2], _A2[2], _B2[2])
        beta = -(2 * SN2 - SD * N2s[0]) / (2 * SN0 - SD * N0s[0])
        N = tuple(n2 + beta * n0 for n2, n0 in zip(N2s, N0s))
        SN, DN, EN = SN2 + beta * SN0, DN2 + beta * DN0, EN2 + beta * EN0
        alpha2 = (EN * SD * SD - ED * SN * SD - 2 * DN * DD * SD + 2 * DD * DD * SN) / (SD * SD * SD)
        scale = sigma * sigma if normalize else LD(1)
        N = tuple(n * scale / alpha2 for n in N)
    else:
        raise ValueError("order must be 0 or 2")
    M = (N[1] - D[0] * N[0], N[2] - D[1] * N[0], N[3] - D[2] * N[0], -D[3] * N[0])
    SN, SM = N[0] + N[1] + N[2] + N[3], M[0] + M[1] + M[2] + M[3]
    return {"N": N, "D": D, "M": M, "BN": tuple(d * SN / SD for d in D), "BM": tuple(d * SM / SD for d in D)}


def filter_lines(d, c, mutate=None):
    """the causal + anti-causal recursion along the LAST axis of the long-double array d (length >= 4)"""
    N0, N1, N2, N3 = c["N"]
    D1, D2, D3, D4 = c["D"]
    M1, M2, M3, M4 = c["M"]
    BN1, BN2, BN3, BN4 = c["BN"]
    BM1, BM2, BM3, BM4 = c["BM"]
    ln = d.shape[-1]
    assert ln >= 4 and d.dtype == LD
    x = [d[..., i] for i in range(ln)]
    v1 = x[0] * 0 if mutate == "zero-causal-start" else x[0]
    s = [None] * ln
    s[0] = x[0] * N0 + v1 * N1 + v1 * N2 + v1 * N3
    s[1] = x[1] * N0 + x[0] * N1 + v1 * N2 + v1 * N3
    s[2] = x[2] * N0 + x[1] * N1 + x[0] * N2 + v1 * N3
    s[3] = x[3] * N0 + x[2] * N1 + x[1] * N2 + x[0] * N3
    s[0] = s[0] - (v1 * BN1 + v1 * BN2 + v1 * BN3 + v1 * BN4)
    s[1] = s[1] - (s[0] * D1 + v1 * BN2 + v1 * BN3 + v1 * BN4)
    s[2] = s[2] - (s[1] * D1 + s[0] * D2 + v1 * BN3 + v1 * BN4)
    s[3] = s[3] - (s[2] * D1 + s[1] * D2 + s[0] * D3 + v1 * BN4)
    for i in range(4, ln):
        s[i] = (x[i] * N0 + x[i - 1] * N1 + x[i - 2] * N2 + x[i - 3] * N3) - \
               (s[i - 1] * D1 + s[i - 2] * D2 + s[i - 3] * D3 + s[i - 4] * D4)
    e = x[ln - 1]
    v2 = e * 0 if mutate == "zero-anticausal-start" else e
    e1 = x[ln - 2] if mutate == "second-start" else e
    a = [None] * ln
    a[ln - 1] = v2 * M1 + v2 * M2 + v2 * M3 + v2 * M4
    a[ln - 2] = e1 * M1 + v2 * M2 + v2 * M3 + v2 * M4
    a[ln - 3] = x[ln - 2] * M1 + e * M2 + v2 * M3 + v2 * M4
    a[ln - 4] = x[ln - 3] * M1 + x[ln - 2] * M2 + e * M3 + v2 * M4
    a[ln - 1] = a[ln - 1] - (v2 * BM1 + v2 * BM2 + v2 * BM3 + v2 * BM4)
    a[ln - 2] = a[ln - 2] - (a[ln - 1] * D1 + v2 * BM2 + v2 * BM3 + v2 * BM4)
    a[ln - 3] = a[ln - 3] - (a[ln - 2] * D1 + a[ln - 1] * D2 + v2 * BM3 + v2 * BM4)
    a[ln - 4] = a[ln - 4] - (a[ln - 3] * D1 + a[ln - 2] * D2 + a[ln - 1] * D3 + v2 * BM4)
    nb = (ln - 4) // BLOCK + 1
    for i in range(ln - 5, -1, -1):
        q = [a[i + 1], a[i + 2], a[i + 3], a[i + 4]]
        if mutate == "block-restart":                 # the state saved at a block boundary is lost: the block starts from 0
            b = ((i // BLOCK) + 1) * BLOCK            # first sample of the block above sample i
            if b // BLOCK < nb:
                q = [qq if i + 1 + j < b else qq * 0 for j, qq in enumerate(q)]
        a[i] = (x[i + 1] * M1 + x[i + 2] * M2 + x[i + 3] * M3 + x[i + 4] * M4) - \
               (q[0] * D1 + q[1] * D2 + q[2] * D3 + q[3] * D4)
    return np.stack([s[i] + a[i] for i in range(ln)], axis=-1)


def restated(array_zyx, spacing_xyz, sigma, normalize=True, mutate=None, on_pass=None):
    """ITK's LaplacianRecursiveGaussianImageFilter on a numpy array whose LAST axis is x, spacing in (x, y, z, ...) order.
    on_pass(order, spacing, normalize, input moved to the last axis [long double], line values [long double]) sees every pass"""
    arr = np.asarray(array_zyx)
    out_type = np.float64 if arr.dtype == np.float64 else np.float32
    nd = arr.ndim
    sp = [float(s) for s in spacing_xyz]
    if mutate != "spacing-xyz":
        sp = sp[::-1]
    if mutate == "normalize-flipped":
        normalize = not normalize
    between = np.float64 if mutate == "float64-between" else np.float32
    src = arr.astype(np.float32) if mutate == "float32-input" else arr
    src = src.astype(LD)

    def one(img, axis, order):
        norm = bool(normalize) if order == 2 else False
        c = coefficients(float(sigma), sp[axis], order, norm)
        moved = np.moveaxis(img, axis, -1)
        lines = filter_lines(moved, c, mutate)
        if on_pass is not None:
            on_pass(order, sp[axis], norm, moved, lines)
        return np.moveaxis(lines, -1, axis).astype(between)

    acc = np.zeros(arr.shape, dtype=np.float32)
    for dim in range(nd - 1, -1, -1):
        others = [o for o in range(nd - 1, -1, -1) if o != dim]
        if mutate == "smooth-first":
            cur = src
            for o in others:
                cur = one(cur, o, 0).astype(LD)
            cur = one(cur, dim, 2)
        else:
            cur = one(src, dim, 2)
            for o in others:
                cur = one(cur.astype(LD), o, 0)
        sp2 = np.float64(sp[dim]) * np.float64(sp[dim])
        if mutate == "single-rounding":
            acc = (acc.astype(LD) + cur.astype(LD) / LD(sp2)).astype(np.float32)
        else:
            acc = (acc.astype(np.float64) + cur.astype(np.float64) / sp2).astype(np.float32)
    return acc.astype(out_type)


def _f32_ties(v):
    """the two float32 rounding ties around the long-double values v"""
    g = v.astype(np.float32)
    up = np.nextafter(g, np.float32(np.inf)).astype(LD)
    dn = np.nextafter(g, np.float32(-np.inf)).astype(LD)
    gl = g.astype(LD)
    return (gl + up) / 2, (gl + dn) / 2


def flag_counter(sigma, other_lines, stats):
    """an on_pass hook: adds the flagged voxels of every pass to stats["flagged"] and keeps the worst line distance, in float32
    ulps of the pass's largest output, in stats["distance"].
    other_lines(sigma, spacing, order, normalize, float64 input moved to the last axis) -> float64 line values"""
    def hook(order, spc, norm, moved, lines):
        other = other_lines(float(sigma), spc, order, norm, moved.astype(np.float64))
        dist = np.abs(other.astype(LD) - lines).max()
        t1, t2 = _f32_ties(lines)
        stats["flagged"] = stats.get("flagged", 0) + int((np.minimum(np.abs(lines - t1), np.abs(lines - t2)) <= 16 * dist).sum())
        ulp = float(np.spacing(np.float32(np.abs(lines).max())))
        stats["distance"] = max(stats.get("distance", 0.0), float(dist) / ulp)
    return hook


# ---- contents ------------------------------------------------------------------------------------------------------------
def content(kind, shape, dtype, seed):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if kind == "normal":
        if dtype == np.bool_:
            return rng.integers(0, 2, shape).astype(dtype)
        if np.issubdtype(dtype, np.integer):
            return rng.integers(max(np.iinfo(dtype).min, -500), min(np.iinfo(dtype).max, 1500), shape).astype(dtype)
        return (rng.standard_normal(shape) * 300 + 500).astype(dtype)
    if kind == "full":                                               # the whole range of an integer type (int64: +-2^40)
        if dtype == np.bool_:
            return rng.integers(0, 2, shape).astype(dtype)
        if dtype == np.int64:
            return rng.integers(-2 ** 40, 2 ** 40, shape)
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)
    if kind == "big":                                                # float64 at 1e12 with random low bits
        return (1e12 * (1 + rng.random(shape))).astype(dtype)
    if kind == "above24":                                            # |values| in [2^24, 2^31): float32 cannot hold them
        a = rng.integers(2 ** 24, 2 ** 31 - 1, shape) * rng.choice(np.array([-1, 1]), size=shape)
        return a.astype(dtype)
    if kind == "bits":                                               # float64 with all 53 significant bits in use
        return (rng.random(shape) * 1000 + 1 / 3).astype(dtype)
    if kind == "offset":                                             # 30 000 +- 3
        return (30000 + rng.integers(-3, 4, shape)).astype(dtype)
    if kind == "step":                                               # a unit step along the last axis, on unit noise
        a = 1 + rng.random(shape)
        a[..., shape[-1] // 2:] += 1
        return a.astype(dtype)
    if kind.startswith("impulse"):                                   # impulse:<axis>:<index> (negative from the end)
        _, ax, idx = kind.split(":")
        a = 1 + rng.random(shape)
        sl = [s // 2 for s in shape]
        sl[int(ax)] = int(idx) % shape[int(ax)]
        a[tuple(sl)] += 8
        return a.astype(dtype)
    if kind == "nonfinite":
        a = rng.standard_normal(shape) * 300 + 500
        a.flat[a.size // 3] = np.nan
        a.flat[(2 * a.size) // 3] = np.inf
        return a.astype(dtype)
    raise KeyError(kind)


# ---- the case table ------------------------------------------------------------------------------------------------------
CASES = {}
GROUPS = {}
# name -> increment of the seed: cases whose first seed(s) had a flagged voxel
RESEED = {'l-len-a0-14x4x6-float32': 1,
 'l-len-a0-27x4x6-float32': 2,
 'l-len-a0-30x4x6-float32': 1,
 'l-len-a0-32x4x6-float32': 1,
 'l-len-a0-34x4x6-float32': 1,
 'l-len-a0-39x4x6-float32': 1,
 'l-len-a0-41x4x6-float32': 1,
 'l-len-a0-42x4x6-float32': 1,
 'l-len-a0-44x4x6-float32': 1,
 'l-len-a0-46x4x6-float32': 1,
 'l-len-a0-48x4x6-float32': 2,
 'l-len-a0-52x4x6-float32': 1,
 'l-len-a1-4x4x6-float32': 1,
 'l-len-a1-4x11x6-float32': 1,
 'l-len-a1-4x20x6-float32': 2,
 'l-len-a1-4x22x6-float32': 1,
 'l-len-a1-4x24x6-float32': 1,
 'l-len-a1-4x26x6-float32': 1,
 'l-len-a1-4x27x6-float32': 1,
 'l-len-a1-4x29x6-float32': 1,
 'l-len-a1-4x32x6-float32': 3,
 'l-len-a1-4x35x6-float32': 1,
 'l-len-a1-4x43x6-float32': 2,
 'l-len-a1-4x47x6-float32': 2,
 'l-len-a1-4x50x6-float32': 1,
 'l-len-a1-4x51x6-float32': 2,
 'l-len-a1-4x52x6-float32': 4,
 'l-len-a1-4x53x6-float32': 2,
 'l-len-a2-4x6x11-float32': 1,
 'l-len-a2-4x6x22-float32': 1,
 'l-len-a2-4x6x28-float32': 1,
 'l-len-a2-4x6x30-float32': 1,
 'l-len-a2-4x6x33-float32': 1,
 'l-len-a2-4x6x38-float32': 1,
 'l-len-a2-4x6x41-float32': 1,
 'l-len-a2-4x6x44-float32': 1,
 'l-len-a2-4x6x45-float32': 1,
 'l-len-a2-4x6x46-float32': 6,
 'l-len-a2-4x6x47-float32': 1,
 'l-len-a2-4x6x52-float32': 1,
 'l-len-a2-4x6x53-float32': 1,
 'l-len-a0-16x4x6-float64': 1,
 'l-len-a0-35x4x6-float64': 1,
 'l-len-a0-41x4x6-float64': 1,
 'l-len-a0-43x4x6-float64': 1,
 'l-len-a0-46x4x6-float64': 1,
 'l-len-a1-4x43x6-float64': 1,
 'l-len-a1-4x48x6-float64': 1,
 'l-len-a2-4x6x30-float64': 1,
 'l-len-a2-4x6x41-float64': 1,
 'l-len-a2-4x6x52-float64': 1,
 'l-content-impulse-a0--2': 3,
 'l-content-impulse-a0--1': 2,
 'l-content-impulse-a1--1': 1,
 'l-content-impulse-a2--2': 4,
 'l-dims-4x5x6x7-float32': 1,
 'l-dims-4x5x6x7-float64': 1,
 'l-len-many-20x9x30-float32': 1,
 'l-len-many-36x9x30-float32': 1,
 'l-len-many-9x30x52-float32': 1,
 'l-len-long-4x4x520-float32': 13,
 'l-len-long-600x4x4-float32': 7,
 'l-sigmad-0.8-1.1-2.5-float32': 4,
 'l-len-many-9x30x19-float64': 2,
 'l-len-many-9x30x20-float64': 1,
 'l-len-many-20x9x30-float64': 1,
 'l-len-many-36x9x30-float64': 2,
 'l-len-many-9x30x52-float64': 8,
 'l-len-many-52x9x30-float64': 1,
 'l-len-long-4x4x520-float64': 1,
 'l-sigmad-0.8-1.1-2.5-float64': 9,
 'l-options-ten': 1}
# name -> the sigmas of the case that NO seed clears (up to 16 were tried): the float64 recursion itself lies too far from the long-double
# one there (a large sigma / spacing puts the poles next to 1 and the coefficient formulas cancel: up to 0.04 float32 ulp at
# sigma / spacing = 10; an offset of 30 000 under +-3 of noise: 7e-4 ulp of a pass whose values are ~1e-4 of its largest), so
# the long-double reference cannot decide their bits.  These are held bit for bit to the float64 restatement instead, which
# the decided cases -- every other one -- pin to this reference; the CPU file asserts that each entry here does have a flag.
UNDECIDED = {'l-sigmad-0.78125-0.78125-6.5-float32': (0.5, 3.0, 8.0),
 'l-sigmad-0.5-1-2-float32': (0.5, 2.0, 8.0),
 'l-sigmad-0.78125-0.78125-6.5-float64': (0.5, 3.0, 8.0),
 'l-sigmad-0.5-1-2-float64': (0.5, 2.0, 8.0),
 'l-content-offset-int16': (0.7, 1.0, 2.5),
 'l-content-offset-float32': (0.7, 1.0, 2.5),
 'l-len-long-4x4x520-float32': (2.5,),
 'l-len-long-600x4x4-float32': (0.7,),
 'l-sigmad-0.8-1.1-2.5-float32': (3.0, 5.0),
 'l-len-long-4x4x520-float64': (0.7,),
 'l-len-long-600x4x4-float64': (0.7, 2.5),
 'l-sigmad-0.8-1.1-2.5-float64': (3.0, 5.0),
 'l-options-ten': (4.0, 5.0)}
WAVELETS = {2: "haar", 4: "db2", 6: "coif1", 8: "db4", 10: "db5", 12: "coif2"}
LOG_LENGTHS = tuple(range(4, 54))
LOG_SIGMAS = (0.7, 1.0, 2.5)
LOG_SPACING = (0.8, 1.1, 2.5)


def _add(group, name, **spec):
    assert name not in CASES, name
    spec.setdefault("content", "normal")
    spec["group"] = group
    CASES[name] = spec
    GROUPS.setdefault(group, []).append(name)


def _axis_shape(axis, N, others):
    s = list(others)
    s.insert(axis, N)
    return tuple(s)


def _tag(shape):
    return "x".join(map(str, shape))


def _build():
    # ---- wavelet
    for F, w in WAVELETS.items():
        for axis in range(3):
            for N in sorted({2, 4, F - 2, F, F + 2, 34} - {0}):
                shape = _axis_shape(axis, N, (4, 6))
                _add("w:taps", "w-taps-%s-a%d-%s" % (w, axis, _tag(shape)), kind="w", shape=shape, dtype="int16", wavelet=w,
                     axes=(2, 1, 0))
    _add("w:taps", "w-taps-custom32-8", kind="w", shape=(4, 8), dtype="float64", wavelet="custom32", axes=(1,))
    for F in (2, 4, 6):
        shapes = [(8, 8, Nx) for Nx in (30, 32, 34, 64, 66)] + [(8, Ny, 32) for Ny in (6, 10, 16, 18)] + \
                 [(Nz, 8, 32) for Nz in sorted({F, 62, 64, 66, 96})]
        for shape in shapes:
            _add("w:tiles", "w-tiles-%s-%s" % (WAVELETS[F], _tag(shape)), kind="w", shape=shape, dtype="int16",
                 wavelet=WAVELETS[F], axes=(2, 1, 0))
    for dt, cont in (("int16", "full"), ("int32", "full"), ("float32", "normal"), ("float64", "big"), ("uint8", "full"),
                     ("uint16", "full"), ("int64", "full"), ("bool", "full")):
        _add("w:dtypes", "w-dtypes-%s" % dt, kind="w", shape=(6, 9, 10), dtype=dt, content=cont, wavelet="coif1", axes=(2, 1, 0))
    for shape, axes in (((12,), (0,)), ((10, 14), (1, 0)), ((10, 14), (0,)), ((10, 14), (1,)), ((9, 13), (1, 0)),
                        ((6, 7, 10), (0,)), ((6, 7, 10), (2, 0)), ((6, 7, 10), (0, 1, 2)), ((5, 8, 10), (1, 2)),
                        ((4, 6, 4, 8), (3, 2, 1, 0)), ((3, 6, 5, 8), (3, 2, 1, 0)),
                        ((5, 8, 10), (2, 1)), ((6, 8, 9), (1, 0))):
        _add("w:dims", "w-dims-%s-axes%s" % (_tag(shape), "".join(map(str, axes))), kind="w", shape=shape, dtype="float64",
             wavelet="db2", axes=axes)
    for level, start in ((1, 0), (2, 0), (3, 0), (1, 1), (1, 2), (2, 1)):
        _add("w:levels", "w-levels-l%d-s%d" % (level, start), kind="w", shape=(8, 9, 12), dtype="int16", content="full",
             wavelet="coif1", axes=(2, 1, 0), level=level, start_level=start)
    _add("w:grid", "w-grid-lines", kind="w", shape=(65538, 4), dtype="float64", wavelet="haar", axes=(1, 0))
    _add("w:grid", "w-grid-stride", kind="w", shape=(2, 1048580), dtype="float64", wavelet="coif1", axes=(0,))
    _add("w:grid", "w-grid-stride-old", kind="w", shape=(2, 1048580), dtype="float64", wavelet="haar", axes=(0,))
    _add("w:nonfinite", "w-nonfinite", kind="w", shape=(6, 8, 10), dtype="float64", content="nonfinite", wavelet="coif1",
         axes=(2, 1, 0))
    # ---- LoG
    for dt in ("float32", "float64"):
        for axis in range(3):
            for ln in LOG_LENGTHS:
                shape = _axis_shape(axis, ln, (4, 6))
                _add("l:lengths:%s:axis%d" % (dt, axis), "l-len-a%d-%s-%s" % (axis, _tag(shape), dt), kind="l", shape=shape,
                     dtype=dt, spacing=LOG_SPACING, sigmas=LOG_SIGMAS if dt == "float32" else LOG_SIGMAS[1:2])
        for ln in (19, 20, 36, 52):
            for shape in ((9, 30, ln), (ln, 9, 30)):
                _add("l:lengths:%s:many" % dt, "l-len-many-%s-%s" % (_tag(shape), dt), kind="l", shape=shape, dtype=dt,
                     spacing=LOG_SPACING, sigmas=LOG_SIGMAS[1:2])
        for shape in ((4, 4, 520), (600, 4, 4)):
            _add("l:lengths:%s:many" % dt, "l-len-long-%s-%s" % (_tag(shape), dt), kind="l", shape=shape, dtype=dt,
                 spacing=LOG_SPACING, sigmas=LOG_SIGMAS)
        for spacing, sigmas in (((0.78125, 0.78125, 6.5), (0.5, 3.0, 8.0)), ((0.5, 1.0, 2.0), (0.5, 2.0, 8.0)),
                                ((0.8, 1.1, 2.5), (1.0, 3.0, 5.0))):
            _add("l:sigmad", "l-sigmad-%s-%s" % ("-".join("%g" % s for s in spacing), dt), kind="l", shape=(12, 20, 40), dtype=dt,
                 spacing=spacing, sigmas=sigmas)
    shape = (5, 6, 9)
    for dt, cont in (("int16", "full"), ("int16", "offset"), ("float32", "offset"), ("float32", "step"), ("float64", "bits"),
                     ("int32", "above24")):
        _add("l:content", "l-content-%s-%s" % (cont, dt), kind="l", shape=shape, dtype=dt, content=cont, spacing=LOG_SPACING,
             sigmas=LOG_SIGMAS)
    for axis in range(3):
        for idx in (0, 1, -2, -1):
            _add("l:content", "l-content-impulse-a%d-%d" % (axis, idx), kind="l", shape=shape, dtype="float32",
                 content="impulse:%d:%d" % (axis, idx), spacing=LOG_SPACING, sigmas=LOG_SIGMAS)
    _add("l:options", "l-options-raw", kind="l", shape=(6, 7, 21), dtype="float32", spacing=LOG_SPACING, sigmas=LOG_SIGMAS,
         normalize=False)
    _add("l:options", "l-options-raw-f64", kind="l", shape=(6, 7, 21), dtype="float64", spacing=LOG_SPACING, sigmas=LOG_SIGMAS,
         normalize=False)
    _add("l:options", "l-options-ten", kind="l", shape=(6, 7, 21), dtype="int16", spacing=LOG_SPACING,
         sigmas=(0.6, 0.8, 1.0, 1.2, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0))
    _add("l:options", "l-options-repeat", kind="l", shape=(6, 7, 21), dtype="float32", spacing=LOG_SPACING, sigmas=(1.0, 2.0, 1.0))
    for shape, spacing in (((23,), (1.1,)), ((9, 21), (0.8, 1.1)), ((4, 5, 6, 7), (0.8, 1.1, 2.5, 1.3))):
        for dt in ("float32", "float64"):
            _add("l:dims", "l-dims-%s-%s" % (_tag(shape), dt), kind="l", shape=shape, dtype=dt, spacing=spacing, sigmas=LOG_SIGMAS)
    # the admissibility rule of getLoGImage, size >= ceil(sigma / spacing) + 1, met with equality on z by sigma 3 (3.5 fails it)
    _add("l:entry", "l-entry-admissible", kind="l", shape=(4, 6, 8), dtype="int16", spacing=(1.0, 1.0, 1.0), sigmas=(3.0,))


_build()


def spec(name):
    return CASES[name]


def seed_of(name):
    return zlib.crc32(name.encode()) + RESEED.get(name, 0)


@functools.lru_cache(maxsize=None)
def case(name):
    """the image of a case, read-only"""
    s = CASES[name]
    x = content(s["content"], s["shape"], s["dtype"], seed_of(name))
    assert x.shape == tuple(s["shape"]) and x.dtype == np.dtype(s["dtype"])
    x.setflags(write=False)
    return x


_REF = {}


def reference(name, mutate=None, other_lines=None):
    """wavelet case -> (approximation, [dict per level]) in long double; LoG case -> [array per sigma] in the output type.
    With other_lines (see flag_counter) a LoG case returns (arrays, flagged voxels per sigma, worst line distance per sigma)."""
    s = CASES[name]
    x = case(name)
    if other_lines is not None:
        stats = [{} for _ in s["sigmas"]]
        outs = [restated(x, s["spacing"], sg, s.get("normalize", True), on_pass=flag_counter(sg, other_lines, st))
                for sg, st in zip(s["sigmas"], stats)]
        _REF[(name, None)] = outs
        return outs, [st["flagged"] for st in stats], [st["distance"] for st in stats]
    if (name, mutate) not in _REF:
        if s["kind"] == "w":
            val = swt3(x, s["wavelet"], s.get("level", 1), s.get("start_level", 0), s["axes"], mutate)
        else:
            val = [restated(x, s["spacing"], sg, s.get("normalize", True), mutate) for sg in s["sigmas"]]
        if mutate is not None:
            return val
        _REF[(name, mutate)] = val
    return _REF[(name, mutate)]


def magnitude(x):
    x = np.asarray(x)
    return float(np.abs(x[np.isfinite(x)].astype(LD)).max())


def level_bounds(name):
    """the bound of every level a wavelet case returns (and of its approximation: the last one)"""
    s = CASES[name]
    lo, hi = taps(s["wavelet"])
    M, p = magnitude(case(name)), len(s["axes"])
    return [wavelet_bound(lo, hi, p * (s.get("start_level", 0) + l), M) for l in range(1, s.get("level", 1) + 1)]


def wavelet_ratio(name, approx, levels):
    """max |got - reference| / bound over every band of a wavelet case; got as (approximation, [dict per level]); inf when the
    names or their order differ, or the sets of non-finite voxels"""
    ref_ap, ref_levels = reference(name)
    bounds = level_bounds(name)
    assert len(levels) == len(ref_levels)
    worst = 0.0
    with np.errstate(invalid="ignore"):
        for got, want, b in zip(levels, ref_levels, bounds):
            if list(got) != list(want):
                return float("inf")
            for k in want:
                worst = max(worst, _distance(got[k], want[k]) / b)
        worst = max(worst, _distance(approx, ref_ap) / bounds[-1])
    return worst


def _distance(got, want):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    if not np.array_equal(fin, np.isfinite(got)) or not np.array_equal(np.isnan(want), np.isnan(np.asarray(got, dtype=LD))):
        return float("inf")
    if not fin.any():
        return 0.0
    return float(np.abs(got.astype(LD)[fin] - want[fin]).max())


def undecided(name):
    return UNDECIDED.get(name, ())


def assert_case(name, got, ratios, family, who="device", restatement=None):
    """wavelet: got = (approximation, [dict per level]) of float64 arrays, held to the bound; LoG: got = [array per sigma],
    held to equality of bits -- with this reference, or for the sigmas of `UNDECIDED` with restatement(image, spacing, sigma,
    normalize), the float64 restatement.  The worst ratio goes to ratios[family] (LoG: the count of differing voxels)."""
    s = CASES[name]
    if s["kind"] == "w":
        approx, levels = got
        for v in [approx] + [b for lv in levels for b in lv.values()]:
            assert v.dtype == np.float64 and v.shape == tuple(s["shape"]), (name, v.dtype, v.shape)
        r = wavelet_ratio(name, approx, levels)
        print("%-44s %-7s distance / bound %.3g" % (name, who, r))
        ratios[family] = max(ratios.get(family, 0.0), r)
        assert r <= 1.0, (name, who, r)
        return
    want = reference(name)
    assert len(got) == len(want), name
    differ = {"": 0, " (float64 restatement)": 0}
    for sg, g, w in zip(s["sigmas"], got, want):
        g = np.asarray(g)
        key = ""
        if sg in undecided(name):
            key = " (float64 restatement)"
            w = restatement(case(name), s["spacing"], sg, s.get("normalize", True))
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape)
        bits = np.uint32 if g.dtype == np.float32 else np.uint64
        differ[key] += int((g.view(bits) != w.view(bits)).sum())
    print("%-44s %-7s voxels whose bits differ from the reference: %d, from the restatement on undecided sigmas %s: %d"
          % (name, who, differ[""], list(undecided(name)), differ[" (float64 restatement)"]))
    for key, d in differ.items():
        if key == "" or undecided(name):
            ratios[family + key] = max(ratios.get(family + key, 0.0), float(d))
    assert not any(differ.values()), (name, who, differ)


def report(title, ratios):
    print("\n%s: wavelet families (w:) worst distance / bound, LoG families (l:) voxels whose bits differ" % title)
    for key in sorted(ratios):
        print("    %-28s %.3g" % (key, ratios[key]))
    bad = {k: v for k, v in ratios.items() if (not v <= 1.0 if k.startswith("w:") else v != 0)}
    assert not bad, bad

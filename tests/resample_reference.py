"""Independent long-double restatement of the resampling step (test helper, not a test): what engine.resample(image, start,
step, newsize, interpolator) has to return for 1, 2 or 3 dimensions, the four pixel types and the three interpolators.

Nothing here imports pyradiomics_amd for its arithmetic.  Everything is numpy over whole arrays in np.longdouble, which must
have a 64-bit significand (`AVAILABLE`; the tests skip with `SKIP_REASON` otherwise, there is no fallback).

Two references for the cubic B-spline:
  exact      the mathematical object: per axis the coefficients solve (c[k-1] + 4 c[k] + c[k+1]) / 6 = x[k] with the whole-sample
             mirror c[-1] = c[1], c[N] = c[N-2] (Thomas elimination; N == 1 leaves the line alone), evaluated with the closed-form
             cubic B-spline weights on the 4-tap support mirrored with period 2N - 2.  No recursion, no pole, no horizon.
  restated   ITK's published algorithm as the header of csrc/kernels_resample.h documents it: gain, causal start over the 1e-10
             horizon (18 taps) or the exact mirror sum when the horizon reaches N, the causal and anti-causal recursions with the
             float64 value of sqrt(3) - 2 as the pole, the same weight formulas -- all in long double.
linear reads the two neighbours with the index clamped to [0, N-1]; nearest reads floor(p + 0.5), clamped.

Shared steps (the API's contract):
  positions    p = start + o * step in float64, the product rounded before the sum (numpy), then widened
  inside test  -0.5 <= p < N - 0.5 on every axis, 0 outside
  integers     clamp to the type's range, then truncate toward zero
  float32      one rounding of the long-double value

`mutate=` reproduces ONE hazard in this model, so that tests/test_resample_reference.py can show that the family of cases that
exists to catch it moves by more than its tolerance (`MUTATIONS`).

Bounds (u = 2^-53, M = max |x| of the case, z = |sqrt(3) - 2|):
  rounding_bound  8 u 27 M.  The inverse of [1, 4, 1] / 6 has l1 norm 6 z (1 + z) / ((1 - z^2)(1 - z)) = 3 per axis, so the
                  coefficients are bounded by 27 M in 3-D; the weights are non-negative and sum to 1.  float64 arithmetic of this
                  algorithm reaches 0.27 to 0.42 of u 27 M against `exact` on the CPU; 8 is the margin over that.
  horizon_bound   27 e M + rounding_bound with e = 6 z^18 / (1 - z) = 4.16e-10: the truncated tail of the causal start relative to
                  the line's magnitude, carried through the later axes with the factor 3.  Loose on purpose: the tight witness of
                  a line longer than 18 is `restated`.
  linear_bound    16 u M.  f = p - floor(p) is exact in float64.  Each of the three levels a (1 - f) + b f rounds four times
                  (1 - f, the two products, the sum), each by at most u times a magnitude that the convex combination keeps at or
                  below M, and hands its error on with the weights (1 - f) + f = 1: 12 u M to first order, 16 u M with the rest.
  nearest, and every inside / outside decision: equality.
  integer and float32 outputs: equal to the cast of the reference, except where the long-double value lies within the bound of
                  a decision point of the cast (an integer, the middle of two neighbouring float32): one unit / one float32 ulp.
                  `needed` measures it: the distance from the reference value to the set of values that cast to what was got.
                  At most 1 % of a case may lie that close (`flagged`; a condition on the inputs, asserted on the CPU).

The case table (`CASES`, `GROUPS`, `case`, `reference`) is shared by tests/test_resample_reference.py (CPU) and
tests/test_gpu_resample_limits.py; the comparison helpers (`compare`, `assert_case`, `report`) are at the end.
"""
from __future__ import annotations

import functools
import math
import zlib
from fractions import Fraction

import numpy as np

LD = np.longdouble
AVAILABLE = bool(np.finfo(LD).eps <= 2.0 ** -63)
SKIP_REASON = "np.longdouble has no 64-bit significand here (eps %.3g > 2^-63): no reference" % float(np.finfo(LD).eps)

U = 2.0 ** -53
Z = abs(math.sqrt(3.0) - 2.0)
HORIZON = int(math.ceil(math.log(1e-10) / math.log(Z)))          # 18: the last line length with the exact mirror sum
E_TAIL = 6.0 * Z ** HORIZON / (1.0 - Z)
CAP = 0.01

MUTATIONS = ("half-mirror", "clamp-support", "truncated-short", "exact-long", "floor-cast", "half-even", "upper-inclusive",
             "lower-exclusive", "fused", "linear-mirror", "lost-tail")
TO_F64_CAP, RESAMPLE_CAP = 8192 * 256, 16384 * 256                   # threads of the two capped grids


def rounding_bound(M):
    return 8.0 * U * 27.0 * M


def horizon_bound(M):
    return 27.0 * E_TAIL * M + rounding_bound(M)


def linear_bound(M):
    return 16.0 * U * M


# ---- the model ---------------------------------------------------------------------------------------------------------
def positions(start, step, n, fused=False):
    """continuous input index of the n output voxels of one axis, float64; fused=True rounds start + o * step once"""
    if fused:
        s, t = Fraction(float(start)), Fraction(float(step))
        return np.array([float(s + o * t) for o in range(n)], dtype=np.float64)
    return np.float64(start) + np.arange(n, dtype=np.float64) * np.float64(step)


def inside_axis(p, N, mutate=None):
    lo = (p > -0.5) if mutate == "lower-exclusive" else (p >= -0.5)
    hi = (p <= N - 0.5) if mutate == "upper-inclusive" else (p < N - 0.5)
    return lo & hi


def mirror(idx, N, mode="whole"):
    idx = np.asarray(idx, dtype=np.int64)
    if N == 1:
        return np.zeros_like(idx)
    if mode == "clamp":
        return np.clip(idx, 0, N - 1)
    if mode == "half":                                               # ... 1 0 | 0 1 .. N-1 | N-1 ..: period 2N
        m = np.mod(idx, 2 * N)
        return np.where(m >= N, 2 * N - 1 - m, m)
    m = np.mod(idx, 2 * N - 2)                                       # ... 1 | 0 1 .. N-1 | N-2 ..: period 2N - 2
    return np.where(m >= N, 2 * N - 2 - m, m)


def _thomas_axis(x, axis):
    """c with (c[k-1] + 4 c[k] + c[k+1]) / 6 = x[k], c[-1] = c[1], c[N] = c[N-2], along `axis`"""
    d = np.moveaxis(x, axis, 0).astype(LD) * LD(6)
    N = d.shape[0]
    if N == 1:
        return np.moveaxis(d / LD(6), 0, axis)
    sub, sup = np.ones(N, dtype=LD), np.ones(N, dtype=LD)
    sub[N - 1] = 2
    sup[0] = 2
    cp = np.zeros(N, dtype=LD)
    cp[0] = sup[0] / LD(4)
    d[0] = d[0] / LD(4)
    for k in range(1, N):
        den = LD(4) - sub[k] * cp[k - 1]
        cp[k] = sup[k] / den
        d[k] = (d[k] - sub[k] * d[k - 1]) / den
    for k in range(N - 2, -1, -1):
        d[k] = d[k] - cp[k] * d[k + 1]
    return np.moveaxis(d, 0, axis)


def exact_coefficients(x):
    c = np.asarray(x).astype(LD)
    for ax in range(c.ndim):
        c = _thomas_axis(c, ax)
    return c


def _restated_axis(x, axis, mutate=None):
    c = np.moveaxis(x, axis, 0).astype(LD)
    N = c.shape[0]
    if N == 1:
        return np.moveaxis(c, 0, axis)
    z = LD(np.float64(np.sqrt(3.0) - 2.0))
    c = c * ((LD(1) - z) * (LD(1) - LD(1) / z))
    truncated = HORIZON < N
    if mutate == "truncated-short":
        truncated = True
    if mutate == "exact-long":
        truncated = False
    if truncated:
        zn, acc = z, c[0].copy()
        for n in range(1, min(HORIZON, N)):
            acc = acc + zn * c[n]
            zn = zn * z
        c[0] = acc
    else:
        iz, zn = LD(1) / z, z
        z2n = LD(1)
        for _ in range(N - 1):
            z2n = z2n * z
        acc = c[0] + z2n * c[N - 1]
        z2n = z2n * z2n * iz
        for n in range(1, N - 1):
            acc = acc + (zn + z2n) * c[n]
            zn = zn * z
            z2n = z2n * iz
        c[0] = acc / (LD(1) - zn * zn)
    for n in range(1, N):
        c[n] = c[n] + z * c[n - 1]
    c[N - 1] = (z / (z * z - LD(1))) * (z * c[N - 2] + c[N - 1])
    for n in range(N - 2, -1, -1):
        c[n] = z * (c[n + 1] - c[n])
    return np.moveaxis(c, 0, axis)


def restated_coefficients(x, mutate=None):
    c = np.asarray(x).astype(LD)
    for ax in range(c.ndim - 1, -1, -1):                             # ITK filters x first
        c = _restated_axis(c, ax, mutate)
    return c


def _weights_exact(t):
    return ((LD(1) - t) ** 3 / LD(6), (LD(3) * t ** 3 - LD(6) * t ** 2 + LD(4)) / LD(6),
            (LD(-3) * t ** 3 + LD(3) * t ** 2 + LD(3) * t + LD(1)) / LD(6), t ** 3 / LD(6))


def _weights_restated(t):
    w3 = (LD(1) / LD(6)) * t * t * t
    w0 = (LD(1) / LD(6)) + LD(0.5) * t * (t - LD(1)) - w3
    w2 = t + w0 - LD(2) * w3
    w1 = LD(1) - w0 - w2 - w3
    return w0, w1, w2, w3


def _shape1(nd, ax, n):
    s = [1] * nd
    s[ax] = n
    return s


def spline_eval(coef, pos, weights, mode="whole"):
    val = coef
    nd = coef.ndim
    for ax in range(nd - 1, -1, -1):
        p = pos[ax].astype(LD)
        N = coef.shape[ax]
        fl = np.floor(p)
        w = weights(p - fl)
        base = fl.astype(np.int64) - 1
        acc = None
        for k in range(4):
            term = np.take(val, mirror(base + k, N, mode), axis=ax) * w[k].reshape(_shape1(nd, ax, len(p)))
            acc = term if acc is None else acc + term
        val = acc
    return val


def linear_eval(x, pos, mutate=None):
    val = np.asarray(x).astype(LD)
    nd = val.ndim
    for ax in range(nd - 1, -1, -1):
        p = pos[ax].astype(LD)
        N = x.shape[ax]
        fl = np.floor(p)
        f = (p - fl).reshape(_shape1(nd, ax, len(p)))
        b = fl.astype(np.int64)
        if mutate == "linear-mirror":
            i0, i1 = mirror(b, N), mirror(b + 1, N)
        else:
            i0, i1 = np.clip(b, 0, N - 1), np.clip(b + 1, 0, N - 1)
        val = np.take(val, i0, axis=ax) * (LD(1) - f) + np.take(val, i1, axis=ax) * f
    return val


def nearest_eval(x, pos, mutate=None):
    idx = []
    for ax in range(x.ndim):
        p = pos[ax].astype(LD)
        i = np.rint(p) if mutate == "half-even" else np.floor(p + LD(0.5))
        idx.append(np.clip(i.astype(np.int64), 0, x.shape[ax] - 1))
    return np.asarray(x)[np.ix_(*idx)].astype(LD)


def resample(x, start, step, newsize, interp, kind="restated", mutate=None):
    """-> (long-double values before the cast, 0 outside; inside [newsize] bool)"""
    x = np.asarray(x)
    nd = x.ndim
    if mutate == "lost-tail" and interp == 3:                       # the conversion stops after one trip of its grid
        x = np.where(np.arange(x.size).reshape(x.shape) < TO_F64_CAP, x, 0).astype(x.dtype)
    pos = [positions(start[d], step[d], int(newsize[d]), fused=(mutate == "fused")) for d in range(nd)]
    inside = np.ones((), dtype=bool)
    for d in range(nd):
        inside = inside & inside_axis(pos[d], x.shape[d], mutate).reshape(_shape1(nd, d, len(pos[d])))
    if interp == 0:
        val = nearest_eval(x, pos, mutate)
    elif interp == 1:
        val = linear_eval(x, pos, mutate)
    elif interp == 3:
        mode = {"half-mirror": "half", "clamp-support": "clamp"}.get(mutate, "whole")
        if kind == "exact":
            val = spline_eval(exact_coefficients(x), pos, _weights_exact, mode)
        else:
            val = spline_eval(restated_coefficients(x, mutate), pos, _weights_restated, mode)
    else:
        raise ValueError("interpolator %r" % (interp,))
    inside = np.broadcast_to(inside, val.shape)
    if mutate == "lost-tail" and interp != 3:                       # so does the evaluation
        inside = inside & (np.arange(val.size).reshape(val.shape) < RESAMPLE_CAP)
    return np.where(inside, val, LD(0)), inside


def cast(val, dtype, mutate=None):
    dtype = np.dtype(dtype)
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        v = np.clip(val, LD(info.min), LD(info.max))
        v = np.floor(v) if mutate == "floor-cast" else np.trunc(v)
        return v.astype(np.int64).astype(dtype)
    return val.astype(dtype)


# ---- contents ------------------------------------------------------------------------------------------------------------
def content(kind, shape, dtype, seed=0):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == "normal":                                             # what tests/test_gpu_filters.py resamples
        a = rng.standard_normal(shape) * 300 + 500
    elif kind == "ramp":                                             # every voxel its own value, none 0
        a = (np.arange(n, dtype=np.float64) + 1).reshape(shape) * 3
    elif kind in ("checker", "blocks"):
        info = np.iinfo(dtype)
        g = np.indices(shape)
        par = (g // 2 if kind == "blocks" else g).sum(axis=0) % 2
        return np.where(par == 0, info.min, info.max).astype(dtype)
    elif kind == "small":
        a = rng.integers(-2, 3, shape)                               # five values: eight equal neighbours are rare
    elif kind == "labels":
        a = rng.choice(np.array([0, 1, 2, 3, 255, 256, 4095, 32766, 32767]), size=shape)
    else:
        raise KeyError(kind)
    return a.astype(dtype)


# ---- the case table ------------------------------------------------------------------------------------------------------
PREFILTER_N = (1, 2, 3, 4, 17, 18, 19, 20, 40)
GEOMETRY_N = (1, 2, 3, 5)
MANY_LINES = (3, 90, 19)                                             # 270 lines of length 19: a ragged second block
INTERPS = {0: "nearest", 1: "linear", 3: "bspline"}
# Found with exact rationals (fractions.Fraction over the float64 start and step, rounded once = a fused multiply-add):
# (start, step, o, N): float64 start + o * step is 7.5 - 2^-50 (inside N = 8); fused, it is 7.5 = N - 0.5 (outside)
UNFUSED_EDGE = (0.3, 0.3, 24, 8)
# (start, step, o, k): unfused 1.5 - 2^-52 (nearest -> k = 1); fused, exactly the tie 1.5 (-> k + 1)
UNFUSED_TIE = (-0.3, 0.15, 12, 1)

CASES = {}
GROUPS = {}


def _add(group, name, **spec):
    assert name not in CASES, name
    spec.setdefault("content", "normal")
    spec.setdefault("seed", zlib.crc32(name.encode()))
    CASES[name] = spec
    GROUPS.setdefault(group, []).append(name)


def _axis_shape(axis, N, others):
    s = list(others)
    s.insert(axis, N)
    return tuple(s)


def _cover(N, start, step):
    """outputs needed for start + o * step to pass N - 0.5 once"""
    return int(math.floor((N - 0.5 - start) / step)) + 2


def _build():
    for dt in ("float64", "float32"):
        for axis in range(3):
            shapes = [_axis_shape(axis, N, (3, 5)) for N in PREFILTER_N] + ([MANY_LINES] if axis == 2 else [])
            for shape in shapes:
                tag = "x".join(map(str, shape))
                _add("prefilter:%s:axis%d" % (dt, axis), "pre-id-a%d-%s-%s" % (axis, tag, dt), shape=shape, dtype=dt, interp=3,
                     start=(0.0,) * 3, step=(1.0,) * 3, newsize=shape)
                _add("prefilter:%s:axis%d" % (dt, axis), "pre-half-a%d-%s-%s" % (axis, tag, dt), shape=shape, dtype=dt, interp=3,
                     start=(-0.25,) * 3, step=(0.5,) * 3, newsize=tuple(2 * s for s in shape))
        for axis in range(3):
            for N in GEOMETRY_N:
                shape = _axis_shape(axis, N, (3, 4))
                tag = "x".join(map(str, shape))

                def grid(s0, st, n):
                    # the other two axes at 0.3, 0.95, 1.6: not dyadic, or the linear float32 values would be float32 ties
                    start, step, new = [0.3] * 3, [0.65] * 3, [3] * 3
                    start[axis], step[axis], new[axis] = s0, st, n
                    return dict(start=tuple(start), step=tuple(step), newsize=tuple(new))
                for interp in (0, 1, 3):
                    g = "geometry:%s:%s" % (dt, INTERPS[interp])
                    _add(g, "geo-edge-%s-a%d-%s-%s" % (tag, axis, INTERPS[interp], dt), shape=shape, dtype=dt, interp=interp,
                         **grid(-0.5, 0.25, 4 * N + 1))                  # -0.5 (inside) ... N - 0.5 (outside), every quarter
                    _add(g, "geo-far-%s-a%d-%s-%s" % (tag, axis, INTERPS[interp], dt), shape=shape, dtype=dt, interp=interp,
                         **grid(-4.3, 0.7, _cover(N, -4.3, 0.7) + 6))   # four voxels before the buffer to four behind it
                if N in (2, 3):                                       # support -2 .. N + 1 wraps the period 2N - 2 twice
                    _add("mirror:%s" % dt, "geo-mirror-%s-a%d-%s" % (tag, axis, dt), shape=shape, dtype=dt, interp=3,
                         **grid(-0.5, 0.125, 8 * N + 1))
    for dt, cont in (("int16", "normal"), ("int32", "normal"), ("float32", "normal"), ("float64", "normal"), ("int16", "labels")):
        shape = (3, 4, 5)
        _add("ties", "ties-%s-%s" % (dt, cont), shape=shape, dtype=dt, content=cont, interp=0, start=(-0.5,) * 3,
             step=(0.25,) * 3, newsize=tuple(4 * s + 1 for s in shape))
    s, t, o, N = UNFUSED_EDGE
    for interp in (0, 1, 3):
        _add("unfused", "unfused-edge-%s" % INTERPS[interp], shape=(N,), dtype="float64", content="ramp", interp=interp,
             start=(s,), step=(t,), newsize=(o + 1,))
    s, t, o, k = UNFUSED_TIE
    _add("unfused", "unfused-tie", shape=(k + 3,), dtype="float64", content="ramp", interp=0, start=(s,), step=(t,),
         newsize=(o + 1,))
    for dt in ("int16", "int32"):
        for cont, shape in (("checker", (5, 6, 8)), ("blocks", (6, 7, 9)), ("small", (5, 7, 18))):
            for interp in ((3,) if cont == "blocks" else (1, 3)):     # linear between two equal samples is that sample
                _add("integer:%s" % INTERPS[interp], "int-%s-%s-%s" % (cont, dt, INTERPS[interp]), shape=shape, dtype=dt,
                     content=cont, interp=interp, start=(-0.3,) * 3, step=(0.37,) * 3,
                     newsize=tuple(_cover(s, -0.3, 0.37) for s in shape))     # few outputs in the clamped half voxels, where
                #                                                               linear returns a sample (an integer) exactly
    for shape in ((1,), (2,), (7,), (19,), (1, 6), (4, 1), (5, 19)):
        for interp in (0, 1, 3):
            _add("dims:%s" % INTERPS[interp], "dims-%s-%s" % ("x".join(map(str, shape)), INTERPS[interp]), shape=shape,
                 dtype="float64", interp=interp, start=(-0.5,) * len(shape), step=(0.45,) * len(shape),
                 newsize=tuple(_cover(s, -0.5, 0.45) for s in shape))
    # more than 16384 * 256 outputs (resample_kernel's grid cap); more than 8192 * 256 input voxels (to_f64_kernel's)
    shape, new = (20, 24, 28), (164, 160, 161)
    step = tuple(s / n for s, n in zip(shape, new))
    _add("stride", "stride-nearest-int16", shape=shape, dtype="int16", interp=0, start=tuple(0.5 * (t - 1) for t in step),
         step=step, newsize=new)
    shape, new = (130, 128, 127), (6, 7, 8)
    _add("stride", "stride-bspline-float32", shape=shape, dtype="float32", interp=3, start=(-0.45, -0.4, -0.35),
         step=(25.95, 21.2, 18.1), newsize=new)


_build()


def spec(name):
    return CASES[name]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (image, start, step, newsize, interpolator); the image is read-only"""
    s = CASES[name]
    x = content(s["content"], s["shape"], s["dtype"], s["seed"])
    x.setflags(write=False)
    return x, np.array(s["start"], dtype=np.float64), np.array(s["step"], dtype=np.float64), tuple(s["newsize"]), s["interp"]


@functools.lru_cache(maxsize=None)
def reference(name, kind="restated", mutate=None):
    x, start, step, newsize, interp = case(name)
    val, inside = resample(x, start, step, newsize, interp, kind, mutate)
    val.setflags(write=False)
    return val, inside


def magnitude(x):
    return float(np.abs(np.asarray(x).astype(LD)).max())


def is_long(shape):
    return max(shape) > HORIZON


def bound_for(interp, kind, shape, M):
    """the tolerance of one comparison in the units of the image"""
    if interp == 0:
        return 0.0
    if interp == 1:
        return linear_bound(M)
    return horizon_bound(M) if (kind == "exact" and is_long(shape)) else rounding_bound(M)


def kinds_for(name):
    """the references a case is held to.  A float32 or integer output cannot be held to `exact` on a long line: the horizon
    bound (1.1e-8 M) is a sixth of a float32 ulp, so a fifth of the voxels would lie within it of a rounding boundary, against
    the 1 % cap; `restated` is the tight witness there"""
    s = CASES[name]
    if s["interp"] != 3:
        return ("restated",)
    if s["dtype"] != "float64" and is_long(s["shape"]):
        return ("restated",)
    return ("restated", "exact")


# ---- comparison ----------------------------------------------------------------------------------------------------------
def preimage(got):
    """[lo, hi] in long double: the values whose cast is `got` (float64: the value itself, the bound carries its rounding)"""
    got = np.asarray(got)
    g = got.astype(LD)
    if np.issubdtype(got.dtype, np.integer):
        info = np.iinfo(got.dtype)
        lo = np.where(got > 0, g, g - LD(1))
        hi = np.where(got < 0, g, g + LD(1))
        return np.where(got == info.min, -np.inf, lo), np.where(got == info.max, np.inf, hi)
    if got.dtype == np.float32:
        dn = np.nextafter(got, np.float32(-np.inf)).astype(LD)
        up = np.nextafter(got, np.float32(np.inf)).astype(LD)
        return (dn + g) / LD(2), (g + up) / LD(2)
    return g, g


def needed(got, val):
    """how far the device's value must have been from the reference value to give `got`"""
    lo, hi = preimage(got)
    return np.maximum(np.maximum(lo - val, val - hi), LD(0))


def units_apart(got, want):
    """|got - want| in units of the type: integers, float32 ulps; float64 is compared by `needed` alone"""
    if np.issubdtype(got.dtype, np.integer):
        return np.abs(got.astype(np.int64) - want.astype(np.int64))
    if got.dtype == np.float32:
        def key(a):
            i = a.view(np.int32).astype(np.int64)
            return np.where(i < 0, -(i & 0x7FFFFFFF), i)
        return np.abs(key(got) - key(want))
    return np.zeros(got.shape, dtype=np.int64)


def flagged(val, dtype, bound):
    """voxels whose reference value lies within `bound` of a decision point of the cast"""
    return cast(val - LD(bound), dtype) != cast(val + LD(bound), dtype)


def compare(got, x, val, inside, interp, kind):
    """-> dict(ratio, mismatches, apart, outside_ok, bound): no assertion.  ratio is max `needed` / bound over the inside voxels
    (for nearest: 0 when equal, inf otherwise)."""
    got = np.asarray(got)
    assert got.shape == val.shape and got.dtype == x.dtype, (got.shape, val.shape, got.dtype, x.dtype)
    bound = bound_for(interp, kind, x.shape, magnitude(x))
    want = cast(val, x.dtype)
    outside_ok = bool(np.all(got[~inside] == 0))
    nd = needed(got, val)[inside]
    worst = float(nd.max()) if nd.size else 0.0
    if bound > 0:
        ratio = worst / bound
    else:
        ratio = 0.0 if np.array_equal(got[inside], want[inside]) else float("inf")
    differ = (got != want) & inside
    if got.dtype == np.float64:                                      # compared by distance alone: no cast to disagree about
        differ = np.zeros(got.shape, dtype=bool)
    return dict(ratio=ratio, mismatches=float(differ.sum()) / max(1, got.size),
                apart=int(units_apart(got, want)[inside].max()) if inside.any() else 0, outside_ok=outside_ok, bound=bound)


def passes(r):
    return r["outside_ok"] and r["ratio"] <= 1.0 and r["apart"] <= 1 and r["mismatches"] <= CAP


def assert_case(name, got, ratios, family, who="device", kinds=None):
    """`got` against the references of the case (kinds_for); the worst ratio goes to ratios[(family, interpolator, kind)]"""
    x, _start, _step, _newsize, interp = case(name)
    for kind in (kinds or kinds_for(name)):
        val, inside = reference(name, kind if interp == 3 else "restated")
        r = compare(got, x, val, inside, interp, kind)
        key = (family, INTERPS[interp], kind if interp == 3 else "-")
        ratios[key] = max(ratios.get(key, 0.0), r["ratio"])
        print("%-52s %-8s vs %-8s ratio %.3g  differ %.2g  apart %d" % (name, who, kind, r["ratio"], r["mismatches"], r["apart"]))
        assert passes(r), (name, who, kind, r)


def report(title, ratios):
    print("\n%s: worst distance to the reference / bound per family, interpolator and reference" % title)
    for key in sorted(ratios):
        print("    %-22s %-8s %-9s %.3g" % (key + (ratios[key],)))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad

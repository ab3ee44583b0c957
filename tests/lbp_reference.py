"""Reference for the LBP2D image type, written independently of pyradiomics_amd.filters: the arithmetic of scikit-image's
local_binary_pattern as the reference's getLBP2DImage applies it (imageoperations.py:1094-1166), restated from its published
algorithm -- scikit-image itself is optional here (tests/test_lbp_reference.py compares against it when it is installed).

Three forms of the same contract:
  lbp_plane          vectorised numpy, one ufunc per operation: every product and every sum is rounded to float64
  lbp_plane_scalar   a per-pixel loop of Python floats, statement by statement as the contract reads
  lbp_plane_fused    the three interpolation sums (top, bottom, t) evaluated EXACTLY (fractions.Fraction) and rounded once each,
                     what a compiler that contracts a*b + c*d into fused multiply-adds approaches.  It is NOT the contract: it
                     exists to prove that a fixture tells the two apart (finite values only).
lbp_volume applies a plane function to arr.swapaxes(0, axis)[idx] and writes the codes back in the input's dtype."""
import math
from fractions import Fraction

import numpy as np

METHODS = ("uniform", "default", "ror")


def sample_offsets(P, R):
    """(rp, cp): row and column offset of the P samples on the circle of radius R, rounded to 5 decimals, float64"""
    i = np.arange(P, dtype=np.float64)
    rp = np.round(-R * np.sin(2 * np.pi * i / P), 5)
    cp = np.round(R * np.cos(2 * np.pi * i / P), 5)
    return rp, cp


def _code(s, P, method):
    """s: the P signs of one pixel (0 / 1) -> the code"""
    if method == "uniform":
        changes = sum(1 for i in range(P - 1) if s[i] != s[i + 1])
        return sum(s) if changes <= 2 else P + 1
    word = sum(int(s[i]) << i for i in range(P))
    if method == "default":
        return word
    if method == "ror":
        full = (1 << P) - 1
        return min(((word >> k) | (word << (P - k))) & full for k in range(P))
    raise NotImplementedError(method)


def lbp_plane_scalar(plane, P, R, method="uniform"):
    img = np.asarray(plane, dtype=np.float64)
    rows, cols = img.shape
    rp, cp = sample_offsets(P, R)
    out = np.zeros((rows, cols), dtype=np.float64)

    def pixel(r, c):
        if r < 0 or r >= rows or c < 0 or c >= cols:
            return 0.0
        return float(img[r, c])

    for r in range(rows):
        for c in range(cols):
            centre = float(img[r, c])
            s = []
            for i in range(P):
                y = float(r) + float(rp[i])
                x = float(c) + float(cp[i])
                minr, maxr = math.floor(y), math.ceil(y)
                minc, maxc = math.floor(x), math.ceil(x)
                dr = y - float(minr)
                dc = x - float(minc)
                tl, tr = pixel(minr, minc), pixel(minr, maxc)
                bl, br = pixel(maxr, minc), pixel(maxr, maxc)
                a = (1.0 - dc) * tl
                b = dc * tr
                top = a + b
                a = (1.0 - dc) * bl
                b = dc * br
                bottom = a + b
                a = (1.0 - dr) * top
                b = dr * bottom
                t = a + b
                s.append(1 if t - centre >= 0 else 0)
            out[r, c] = _code(s, P, method)
    return out


def lbp_plane_fused(plane, P, R, method="uniform"):
    img = np.asarray(plane, dtype=np.float64)
    if not np.isfinite(img).all():
        raise ValueError("the fused variant takes finite planes only")
    rows, cols = img.shape
    rp, cp = sample_offsets(P, R)
    out = np.zeros((rows, cols), dtype=np.float64)
    F = Fraction

    def pixel(r, c):
        if r < 0 or r >= rows or c < 0 or c >= cols:
            return 0.0
        return float(img[r, c])

    def once(w0, v0, w1, v1):      # w0 v0 + w1 v1, exact, rounded once (float() of a Fraction is correctly rounded)
        return float(F(w0) * F(v0) + F(w1) * F(v1))

    for r in range(rows):
        for c in range(cols):
            centre = float(img[r, c])
            s = []
            for i in range(P):
                y = float(r) + float(rp[i])
                x = float(c) + float(cp[i])
                minr, maxr = math.floor(y), math.ceil(y)
                minc, maxc = math.floor(x), math.ceil(x)
                dr = y - float(minr)
                dc = x - float(minc)
                top = once(1.0 - dc, pixel(minr, minc), dc, pixel(minr, maxc))
                bottom = once(1.0 - dc, pixel(maxr, minc), dc, pixel(maxr, maxc))
                t = once(1.0 - dr, top, dr, bottom)
                s.append(1 if t - centre >= 0 else 0)
            out[r, c] = _code(s, P, method)
    return out


def lbp_plane(plane, P, R, method="uniform"):
    img = np.asarray(plane, dtype=np.float64)
    rows, cols = img.shape
    rp, cp = sample_offsets(P, R)
    r = np.arange(rows, dtype=np.float64)[:, None]
    c = np.arange(cols, dtype=np.float64)[None, :]

    def pixel(ri, ci):
        ri, ci = np.broadcast_arrays(ri.astype(np.int64), ci.astype(np.int64))
        inside = (ri >= 0) & (ri < rows) & (ci >= 0) & (ci < cols)
        return np.where(inside, img[np.clip(ri, 0, rows - 1), np.clip(ci, 0, cols - 1)], 0.0)

    signs = np.zeros((P, rows, cols), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(P):
            y, x = r + rp[i], c + cp[i]
            minr, maxr, minc, maxc = np.floor(y), np.ceil(y), np.floor(x), np.ceil(x)
            dr, dc = y - minr, x - minc
            top = (1.0 - dc) * pixel(minr, minc) + dc * pixel(minr, maxc)
            bottom = (1.0 - dc) * pixel(maxr, minc) + dc * pixel(maxr, maxc)
            t = (1.0 - dr) * top + dr * bottom
            signs[i] = (t - img) >= 0
    if method == "uniform":
        changes = (signs[:-1] != signs[1:]).sum(0)
        return np.where(changes <= 2, signs.sum(0), P + 1).astype(np.float64)
    word = np.zeros((rows, cols), dtype=np.int64)
    for i in range(P):
        word |= signs[i] << i
    if method == "default":
        return word.astype(np.float64)
    if method == "ror":
        full = (1 << P) - 1
        best = word.copy()
        for k in range(1, P):
            best = np.minimum(best, ((word >> k) | (word << (P - k))) & full)
        return best.astype(np.float64)
    raise NotImplementedError(method)


def lbp_volume(array, P=8, R=1, method="uniform", axis=0, plane_fn=lbp_plane):
    """the reference's loop: 3-D arrays plane by plane along `axis`, codes written back in the input's dtype; a 2-D array is one
    plane and comes back as float64"""
    a = np.asarray(array)
    if a.ndim == 2:
        return plane_fn(a, P, R, method)
    out = a.copy().swapaxes(0, axis)
    src = a.swapaxes(0, axis)
    for idx in range(src.shape[0]):
        out[idx, ...] = plane_fn(src[idx], P, R, method)
    return np.ascontiguousarray(out.swapaxes(0, axis))


def plateau_plane(seed=20240611, levels=300, mean=100.0, sigma=30.0, across=20):
    """a float64 plane of 3 x 3 plateaus, `levels` draws of N(mean, sigma): a flat neighbourhood of a level that is no small
    integer interpolates to one ulp beside the centre, and the sign of that ulp changes under contraction"""
    v = np.random.default_rng(seed).normal(mean, sigma, levels)
    grid = v.reshape(levels // across, across)
    return np.kron(grid, np.ones((3, 3))).astype(np.float64)

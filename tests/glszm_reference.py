"""Independent restatement of the grey level size zone matrix (test helper, not a test).

Written from the definition of a zone: a maximal set of ROI voxels of one grey level that is connected under the full
neighbourhood (26 neighbours in 3-D, 3^N - 1 in N-D; with force2D the 8 in-plane neighbours perpendicular to the forced
axis).  For every grey level the voxels of that level are labelled by scipy.ndimage.label with the matching structuring
element and the zone sizes come from np.bincount.  Nothing here shares code or an algorithm with the HIP kernels (tile
labelling + union-find) or with oracle/texture_oracle.c (a flood fill with an explicit stack).

`drop` removes structure elements (offsets such as (-1, -1, -1)); scipy needs a symmetric structure, so the mirrored
element goes with it.  tests/test_glszm_reference.py uses it to show that the pin against the C checker is sharp.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage


def structure(ndim, force2Ddim=None, drop=()):
    """bool [3] * ndim: the neighbours that tie two voxels of one level into one zone"""
    s = np.ones((3,) * ndim, dtype=bool)
    if force2Ddim is not None:
        keep = [slice(None)] * ndim
        for k in (0, 2):
            keep[force2Ddim] = k
            s[tuple(keep)] = False
    for off in drop:
        off = np.asarray(off)
        s[tuple(1 + off)] = False
        s[tuple(1 - off)] = False
    return s


def zones(img, mask, force2D=False, force2Ddimension=0, drop=()):
    """-> int64 [nzones, 3] rows (level, size, first linear index), in the order of the first linear index: the order in
    which a raster scan of the volume discovers the zones"""
    img = np.asarray(img)
    mask = np.asarray(mask).astype(bool)
    st = structure(img.ndim, force2Ddimension if force2D else None, drop)
    rows = []
    for g in np.unique(img[mask]):
        lab, n = ndimage.label((img == g) & mask, structure=st)
        if n == 0:
            continue
        flat = lab.ravel()
        idx = np.flatnonzero(flat)                      # ascending: the first hit of a label is its smallest index
        ids, first = np.unique(flat[idx], return_index=True)
        assert len(ids) == n
        sizes = np.bincount(flat, minlength=n + 1)[1:]
        rows.append(np.stack([np.full(n, int(g), dtype=np.int64), sizes.astype(np.int64), idx[first].astype(np.int64)], 1))
    if not rows:
        return np.zeros((0, 3), dtype=np.int64)
    z = np.concatenate(rows)
    return z[np.argsort(z[:, 2], kind="stable")]


def census(z):
    """{(level, size): number of zones}"""
    if not len(z):
        return {}
    pairs, counts = np.unique(z[:, :2], axis=0, return_counts=True)
    return {(int(g), int(s)): int(c) for (g, s), c in zip(pairs, counts)}


def matrix(z, Ng):
    """the dense layout of the reference's operator: float64 [1, Ng, maxRegion], maxRegion >= 1"""
    maxRegion = max(int(z[:, 1].max()) if len(z) else 0, 1)
    P = np.zeros((1, Ng, maxRegion), dtype=np.float64)
    if len(z):
        if z[:, 0].min() < 1 or z[:, 0].max() > Ng:
            raise IndexError("a zone of a level outside 1..Ng")
        np.add.at(P[0], (z[:, 0] - 1, z[:, 1] - 1), 1.0)
    return P


def compact(z, Ng):
    """(P float64 [Ng, k], sizes int32 [k] ascending): the dense matrix without its empty size columns"""
    sizes = np.unique(z[:, 1]) if len(z) else np.zeros(0, dtype=np.int64)
    P = np.zeros((Ng, len(sizes)), dtype=np.float64)
    if len(z):
        np.add.at(P, (z[:, 0] - 1, np.searchsorted(sizes, z[:, 1])), 1.0)
    return P, sizes.astype(np.int32)


def zone_list(z):
    """int32 [2 * nzones + 1]: (level, size) pairs in discovery order, closed by -1 (the zone list of the operator)"""
    return np.concatenate([z[:, :2].reshape(-1), [-1]]).astype(np.intc)


def census_matrix(cen, Ng):
    """compact (P, sizes) of a census {(level, size): count}"""
    sizes = np.array(sorted({s for _, s in cen}), dtype=np.int64)
    P = np.zeros((Ng, len(sizes)), dtype=np.float64)
    for (g, s), c in cen.items():
        P[g - 1, np.searchsorted(sizes, s)] += c
    return P, sizes.astype(np.int32)

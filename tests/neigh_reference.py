"""Independent restatement of the neighbourhood matrices of segment mode (test helper, not a test): GLDM and NGTDM for
Nd = 2 and 3, any `distances`, force2D and any alpha (a negative alpha puts every voxel in dependence column 0, as the
reference C does), plus the plain GLCM pair count the pairs-tier cases need.

Everything is numpy over whole arrays and Python ints: one shifted copy of the level volume per angle, integer counts
and sums, no atomics, no tiles, no packed bytes.  Nothing here shares code or an algorithm with csrc/kernels_neigh.h,
csrc/kernels_pairs.h or oracle/texture_oracle.c (a raster scan with a float64 running sum).  The angle list is an
argument: the tests hand in what the checker's own generator builds.

`accumulators` returns the integer tables [Ng, Na + 1] in the layout documented at the top of kernels_neigh.h:
  GLDM   [g][k]  = ROI voxels of level g + 1 with k dependent neighbours
  NGTDM  [g][0]  = ROI voxels of level g + 1;  [g][c] = sum over those with c valid neighbours of |c * level - sum(neigh)|
The GLDM matrix and NGTDM columns 0 and 2 follow exactly; NGTDM's s_i is the rational sum_c S_c / c, formed with
fractions.Fraction over Python ints and rounded once (`ngtdm_s`).

`defect=` reproduces ONE kernel hazard in this model, so that tests/test_neigh_reference.py can show that the case table
below notices it:
  left-edge   the dx = -1 neighbour is lost where x % 4 == 0        (neigh4_kernel: byte x0 - 1 from the lower lane)
  right-edge  the dx = +1 neighbour is lost where x % 4 == 3        (byte x0 + 4 from the upper lane)
  wave-edge   the same where the flattened index % 256 is 0 / 255   (lanes 0 and 63 load their own edge bytes)
  row-wrap    x = Nx - 1 -> x = 0 of the next row count as neighbours (the x bound is not applied)
  plane-wrap  the same across planes                                 (the y bound is not applied)
  tail8       the last n % 8 centre voxels are ignored               (pairs_glcm_kernel's tail loop)
  last-tile   centre levels of the last GLCM row tile are ignored    (RT = 38400 / Ng rows per tile)
  slot0       NGTDM level counts come from the GLDM row of the neighbouring level (neigh4_kernel MODE 2's flush)
  slab-halo   neighbours outside the centre planes [zlo, zhi) read as zero (the packed planes [plo, phi))

The case table (`NAMES`, `case`, `GROUPS`) is shared by tests/test_neigh_reference.py (CPU) and the two GPU limit modules.
The GPU modules' comparison helpers (`run_case`, `check_route`, `check_s`, `report`) are at the end.
"""
from __future__ import annotations

import functools
import itertools
from fractions import Fraction

import numpy as np

DEFECTS = ("left-edge", "right-edge", "wave-edge", "row-wrap", "plane-wrap", "tail8", "last-tile", "slot0", "slab-halo")
PAIR_LDS_WORDS = 150 * 256            # kernels_pairs.h: 150 KB of u32


# ---- the model ---------------------------------------------------------------------------------------------------------
def embed3(a):
    a = np.asarray(a)
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def angles3(angles):
    a = np.asarray(angles, dtype=np.int64)
    return np.concatenate([np.zeros((len(a), 3 - a.shape[1]), dtype=np.int64), a], axis=1)


@functools.lru_cache(maxsize=64)
def _geometry(shape3):
    Nz, Ny, Nx = shape3
    flat = np.arange(Nz * Ny * Nx, dtype=np.int64)
    return flat // (Ny * Nx), (flat // Nx) % Ny, flat % Nx, flat


def _packed(levels, mask, Ng):
    lv = embed3(levels).astype(np.int64)
    mk = embed3(mask).astype(bool)
    if lv.shape != mk.shape:
        raise ValueError("image and mask differ in shape")
    if mk.any() and (lv[mk].min() < 1 or lv[mk].max() > Ng):
        raise IndexError("a masked level outside 1..Ng")             # what the reference raises (cmatrices.c:647, :744)
    return np.where(mk, lv, 0).ravel(), tuple(int(s) for s in lv.shape)


def _neighbour(L, shape3, off, defect, zrange):
    """levels of the voxels at +off (0: outside the volume or the ROI), one per voxel of the flattened volume"""
    Nz, Ny, Nx = shape3
    z, y, x, flat = _geometry(shape3)
    dz, dy, dx = (int(o) for o in off)
    zz, yy, xx = z + dz, y + dy, x + dx
    inz, iny, inx = (zz >= 0) & (zz < Nz), (yy >= 0) & (yy < Ny), (xx >= 0) & (xx < Nx)
    j = flat + (dz * Ny + dy) * Nx + dx
    inside = (j >= 0) & (j < L.size)
    if defect == "row-wrap":
        ok = inz & iny & inside
    elif defect == "plane-wrap":
        ok = inz & inx & inside
    else:
        ok = inz & iny & inx
    if defect == "left-edge" and dx == -1:
        ok = ok & (x % 4 != 0)
    if defect == "right-edge" and dx == 1:
        ok = ok & (x % 4 != 3)
    if defect == "wave-edge" and dx == -1:
        ok = ok & (flat % 256 != 0)
    if defect == "wave-edge" and dx == 1:
        ok = ok & (flat % 256 != 255)
    if defect == "slab-halo" and zrange is not None:
        ok = ok & (zz >= zrange[0]) & (zz < zrange[1])
    return np.where(ok, L[np.clip(j, 0, L.size - 1)], 0)


def _centres(L, shape3, Ng, defect, zrange):
    z, _, _, flat = _geometry(shape3)
    c = L != 0
    if zrange is not None:
        c = c & (z >= zrange[0]) & (z < zrange[1])
    if defect == "tail8":
        c = c & (flat < L.size - L.size % 8)
    if defect == "last-tile" and Ng * Ng > PAIR_LDS_WORDS:
        rt = PAIR_LDS_WORDS // Ng
        c = c & (L - 1 < ((Ng - 1) // rt) * rt)
    return c


def accumulators(levels, mask, Ng, angles, alpha=0, defect=None, zrange=None):
    """-> (GLDM int64 [Ng, Na + 1], NGTDM int64 [Ng, Na + 1]) of the centre voxels in planes zrange (default: all)"""
    assert defect is None or defect in DEFECTS, defect
    L, shape3 = _packed(levels, mask, Ng)
    A = angles3(angles)
    Na = len(A)
    cnt = np.zeros(L.size, dtype=np.int64)
    tot = np.zeros(L.size, dtype=np.int64)
    dep = np.zeros(L.size, dtype=np.int64)
    for off in A:
        V = _neighbour(L, shape3, off, defect, zrange)
        nz = V != 0
        cnt += nz
        tot += V
        dep += nz & (np.abs(L - V) <= alpha)
    idx = np.flatnonzero(_centres(L, shape3, Ng, defect, zrange))
    c = L[idx] - 1
    gldm = np.zeros((Ng, Na + 1), dtype=np.int64)
    np.add.at(gldm, (c, dep[idx]), 1)
    ngtdm = np.zeros((Ng, Na + 1), dtype=np.int64)
    np.add.at(ngtdm, (c, 0), 1)
    n = cnt[idx]
    d = np.abs(n * L[idx] - tot[idx])
    has = n > 0
    np.add.at(ngtdm, (c[has], n[has]), d[has])
    if defect == "slot0":
        ngtdm[:, 0] = np.roll(gldm.sum(axis=1), 1)
    return gldm, ngtdm


def gldm_matrix(acc):
    """float64 [Ng, 2 Na + 1]: the reference's row stride, columns beyond Na stay zero (cmatrices.c:660-754)"""
    Ng, W = acc.shape
    out = np.zeros((Ng, 2 * (W - 1) + 1), dtype=np.float64)
    out[:, :W] = acc
    return out


def ngtdm_s_exact(acc):
    """[Ng] Fractions: s_i = sum_c S_c / c over Python ints"""
    s = [Fraction(0)] * acc.shape[0]
    for g, c in zip(*np.nonzero(acc[:, 1:])):
        s[g] += Fraction(int(acc[g, c + 1]), int(c) + 1)
    return s


def ngtdm_s(acc):
    """float64 [Ng]: the correctly rounded s_i (float() of a Fraction rounds the exact quotient once)"""
    return np.array([float(f) for f in ngtdm_s_exact(acc)], dtype=np.float64)


def ngtdm_matrix(acc):
    """float64 [Ng, 3]: n_i, the correctly rounded s_i, the level (cmatrices.c:543-658)"""
    out = np.zeros((acc.shape[0], 3), dtype=np.float64)
    out[:, 0] = acc[:, 0]
    out[:, 1] = ngtdm_s(acc)
    out[:, 2] = np.arange(1, acc.shape[0] + 1)
    return out


def s_bound(exact, Na):
    """|got - exact| allowed for NGTDM column 1: ngtdm_finalize_kernel does Na divisions of exact integers below 2^53 and
    Na additions of non-negative terms in float64 -- (Na + 1) 2^-53 relative to first order; the bound is twice that"""
    return (Na + 2) * 2.0 ** -52 * np.asarray(exact, dtype=np.float64)


def glcm_counts(levels, mask, Ng, angles, defect=None):
    """int64 [Ng, Ng, Na]: ordered pairs (p, p + angle) with both voxels in the ROI (cmatrices.c:4-92)"""
    assert defect is None or defect in DEFECTS, defect
    L, shape3 = _packed(levels, mask, Ng)
    A = angles3(angles)
    centre = _centres(L, shape3, Ng, defect, None)
    out = np.zeros((Ng, Ng, len(A)), dtype=np.int64)
    for a, off in enumerate(A):
        V = _neighbour(L, shape3, off, defect, None)
        sel = centre & (V != 0)
        np.add.at(out[:, :, a], (L[sel] - 1, V[sel] - 1), 1)
    return out


# ---- deterministic contents and masks ----------------------------------------------------------------------------------
CONTENTS = ("checker3", "lattice", "stripes4", "stripes256", "ramp", "equal", "iid")
MASKS = ("full", "faces", "corners", "quad-edges", "wave-edges", "holes4", "empty") + tuple("one%d" % k for k in range(9))
STRUCTURED_MASKS = ("full", "faces", "quad-edges", "wave-edges", "holes4")
# (`cover`, below, is a content of the level-count cases only: not part of the content x mask product of the edge groups)


def _coords(shape):
    shape3 = (1,) * (3 - len(shape)) + tuple(shape)
    z, y, x, flat = _geometry(shape3)
    return shape3, z, y, x, flat


def content(name, shape, Ng, seed=1):
    """int32 levels in 1..Ng"""
    shape3, z, y, x, flat = _coords(shape)
    if name == "checker3":
        v = np.where((x + y + z) % 2 == 0, 1, Ng)
    elif name == "lattice":
        v = np.where((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0), Ng, 1)
    elif name == "stripes4":
        v = 1 + (flat // 4) % Ng
    elif name == "stripes256":
        v = 1 + (flat // 256) % Ng
    elif name == "ramp":
        v = 1 + (x + 3 * y + 7 * z) % Ng
    elif name == "equal":
        v = np.full(flat.size, Ng)
    elif name == "cover":                    # every level 1..min(Ng, n), each at positions Ng apart: unlike `ramp`, whose
        v = 1 + flat % Ng                    # x + 3y + 7z stays below Ng on small volumes, it reaches the last levels
    elif name == "iid":
        v = np.random.default_rng(seed).integers(1, Ng + 1, size=flat.size)
    else:
        raise KeyError(name)
    return v.astype(np.int32).reshape(shape)


def roi(name, shape):
    """bool mask"""
    shape3, z, y, x, flat = _coords(shape)
    Nz, Ny, Nx = shape3
    if name == "full":
        m = np.ones(flat.size, bool)
    elif name == "faces":                    # the boundary faces of the array (of its own dimensions: not the padded ones)
        m = (x == 0) | (x == Nx - 1) | (y == 0) | (y == Ny - 1)
        if len(shape) == 3:
            m = m | (z == 0) | (z == Nz - 1)
    elif name == "corners":
        m = ((x == 0) | (x == Nx - 1)) & ((y == 0) | (y == Ny - 1)) & ((z == 0) | (z == Nz - 1))
    elif name == "quad-edges":
        m = (x % 4 == 0) | (x % 4 == 3)
    elif name == "wave-edges":
        m = (flat % 256 == 0) | (flat % 256 == 255)
    elif name == "holes4":
        m = x % 4 != 0
    elif name == "empty":
        m = np.zeros(flat.size, bool)
    elif name.startswith("one"):             # one voxel: corner k of the eight (bits z, y, x), or the centre for k = 8
        k = int(name[3:])
        p = (Nz // 2, Ny // 2, Nx // 2) if k == 8 else ((Nz - 1) * (k >> 2 & 1), (Ny - 1) * (k >> 1 & 1), (Nx - 1) * (k & 1))
        m = (z == p[0]) & (y == p[1]) & (x == p[2])
    else:
        raise KeyError(name)
    return m.reshape(shape)


# ---- which kernel answers (the plans of kernels_neigh.h and prad_api.hip, restated from their documented limits) -------
def _cube(angles):
    A = angles3(angles)
    r = np.abs(A).max(axis=0)
    return int(np.prod(2 * r + 1)), r


def expected_route(family, shape, Ng, angles, alpha=0, no_box=False, no_pairs=False):
    """the label prad_last_variant() must show for a synchronous segment-mode call: "neigh4-full26", "neigh4-rows", "neigh1",
    "pairs-lds64|lds32|global[+box32|+box64]", "pairs" (GLCM / GLRLM in the tier) or "generic" (last_path, variant "none")"""
    if family in ("glcm", "glrlm"):
        return "generic" if no_pairs else "pairs"
    A = angles3(angles)
    Na = len(A)
    Nx = shape[-1]
    ngtdm = family == "ngtdm"
    cube, _ = _cube(angles)
    box = ngtdm and not no_box and not no_pairs and cube - 1 == Na and cube <= 4096 and cube * Ng < 2 ** 40 and Ng <= 65535
    if not (ngtdm and Na > 26 and box):
        if Ng <= 255 and Na <= 128 and Ng * (Na + 1) * (8 if ngtdm else 4) <= 64 * 1024:
            unit = np.abs(A).max() <= 1
            if (ngtdm or alpha == 0) and Nx % 4 == 0 and unit:
                return "neigh4-full26" if Na == 26 else "neigh4-rows"
            return "neigh1"
    if Ng > 65535 or no_pairs or (not box and Na > 128):
        return "generic"
    nacc = Ng * (Na + 1)
    if not ngtdm:
        return "pairs-lds32" if nacc <= PAIR_LDS_WORDS else "pairs-global"
    place = "lds64" if 2 * nacc <= PAIR_LDS_WORDS else ("lds32" if nacc <= PAIR_LDS_WORDS else "global")
    if not box:
        return "pairs-" + place
    return "pairs-%s+box%d" % (place, 32 if cube <= 127 and cube * Ng < 2 ** 24 else 64)


def path_of(route):
    """prad_last_path() for a label of expected_route"""
    return route.split("-")[0].replace("neigh4", "neigh").replace("neigh1", "neigh")


# ---- the case table ----------------------------------------------------------------------------------------------------
# name -> dict(family, shape, content, mask, Ng, distances, alpha, force2D, dim, group, no_box, no_pairs)
_TABLE = {}
GROUPS = {}           # group -> [names]


def _add(group, family, shape, cont, mask, Ng, distances=(1,), alpha=0, f2d=None, no_box=False, no_pairs=False):
    name = "%s|%s|%s|%s|Ng%d|d%s|a%d|f%s%s%s" % (family, "x".join(map(str, shape)), cont, mask, Ng, "".join(map(str, distances)),
                                                  alpha, "-" if f2d is None else f2d, "|nobox" if no_box else "",
                                                  "|nopairs" if no_pairs else "")
    if name in _TABLE:
        return name
    _TABLE[name] = dict(family=family, shape=tuple(shape), content=cont, mask=mask, Ng=Ng, distances=list(distances), alpha=alpha,
                        force2D=f2d is not None, dim=f2d or 0, group=group, no_box=no_box, no_pairs=no_pairs)
    GROUPS.setdefault(group, []).append(name)
    return name


QUAD_SHAPES = [(3, 3, 4), (3, 5, 8), (2, 7, 12), (3, 3, 252), (3, 3, 256), (3, 3, 260), (1, 9, 16), (9, 16), (5, 1, 16), (2, 2, 1028)]
SCALAR_SHAPES = [(3, 3, 5), (3, 3, 7), (3, 3, 255), (3, 3, 257)]
BIG_SHAPE = (9, 240, 260)
EDGE_DEFECTS = ("left-edge", "right-edge", "wave-edge", "row-wrap", "plane-wrap")


def possible_edge_defects(shape):
    """the edge defects that can change anything on a volume of this shape at all (pure geometry, distance 1)"""
    shape3, z, y, x, flat = _coords(shape)
    Nz, Ny, Nx = shape3
    out = []
    if Nx >= 5:
        out += ["left-edge", "right-edge"]
    if ((flat % 256 == 255) & (x < Nx - 1)).any() or ((flat % 256 == 0) & (x > 0)).any():
        out.append("wave-edge")
    if Nx >= 2 and Ny * Nz > 1:
        out.append("row-wrap")               # the last voxel of a row and the first of the next one
    if Nz > 1 and Ny >= 2:
        out.append("plane-wrap")             # the last row of a plane and the first of the next one
    return out


# (shape, content, mask) combinations of the structured masks on which NO edge defect of the model changes GLDM (alpha 0)
# or NGTDM at 32 levels: they cannot tell a wrong kernel from a right one and are left out of the "edges" groups.
# tests/test_neigh_reference.py recomputes this rule for every combination.
def edge_combo_listed(shape, cont, mask):
    shape3, z, y, x, flat = _coords(shape)
    if mask == "wave-edges":                 # fewer than 257 voxels: voxel 0 alone, or voxels 0 and 255 with no pair between them
        return flat.size > 256
    if mask == "holes4" and shape3[2] % 4 == 0:   # x % 4 == 0 is outside the ROI: every lost or wrapped x neighbour is a hole
        return "plane-wrap" in possible_edge_defects(shape)
    return True


def _build():
    for shape in QUAD_SHAPES + SCALAR_SHAPES:
        tag = "x".join(map(str, shape))
        for cont, mask in itertools.product(CONTENTS, STRUCTURED_MASKS):
            if not edge_combo_listed(shape, cont, mask):
                continue
            for fam in ("gldm", "ngtdm"):
                _add("edges:" + tag, fam, shape, cont, mask, 32)
        for cont in ("checker3", "iid"):                 # the largest per-voxel sums: 255 levels
            for fam in ("gldm", "ngtdm"):
                _add("edges:" + tag, fam, shape, cont, "full", 255)
        for mask in ("empty", "corners") + tuple("one%d" % k for k in range(9)):
            for fam in ("gldm", "ngtdm"):
                _add("degenerate:" + tag, fam, shape, "iid", mask, 32)
        for cont in ("iid", "ramp"):
            for Ng in (1, 2, 32, 255):
                for alpha in (0, 1, Ng - 1, Ng + 5, -1):
                    _add("alpha:" + tag, "gldm", shape, cont, "full", Ng, alpha=alpha)
                _add("alpha:" + tag, "ngtdm", shape, cont, "full", Ng)
    for cont in ("iid", "checker3"):
        for fam in ("gldm", "ngtdm"):
            _add("big", fam, BIG_SHAPE, cont, "full", 32)
    for dim in (0, 1, 2):
        for cont, mask in itertools.product(("iid", "checker3", "ramp", "stripes4"), ("full", "faces", "quad-edges")):
            for fam in ("gldm", "ngtdm"):
                _add("force2d", fam, (6, 8, 12), cont, mask, 32, f2d=dim)
    # plan_neigh's limits: 255 levels, 64 KiB of bins (125 x 4, 99 x 4 and 99 x 8 bytes per level)
    for cont, mask in (("iid", "full"), ("checker3", "faces"), ("ramp", "full")):
        for Ng in (255, 256):
            for fam in ("gldm", "ngtdm"):
                _add("route-edges", fam, (7, 6, 12), cont, mask, Ng)
        for Ng in (131, 132):
            _add("route-edges", "gldm", (7, 6, 12), cont, mask, Ng, (1, 2))
        for Ng in (165, 166):
            _add("route-edges", "gldm", (7, 6, 12), cont, mask, Ng, (2,))
        for Ng in (82, 83):
            _add("route-edges", "ngtdm", (7, 6, 12), cont, mask, Ng, (2,))
    # ---- pairs tier: GLDM / NGTDM ----
    P = (8, 12, 16)
    # `ramp` holds levels 1..98 on this shape and checker3 / lattice only 1 and Ng; `cover` holds every level up to 1536, so the
    # whole bin table is written up to 1423 levels (at 65 535 / 65 536 levels the high bins are reached through level Ng alone)
    for cont, mask in (("ramp", "full"), ("cover", "full"), ("checker3", "faces"), ("lattice", "holes4")):
        for Ng in (256, 711, 712, 1422, 1423, 65535, 65536):
            for fam in ("gldm", "ngtdm"):
                _add("pairs-levels", fam, P, cont, mask, Ng)
        for Ng in (307, 308):
            _add("pairs-levels", "gldm", P, cont, mask, Ng, (1, 2))
        for Ng in (387, 388):
            _add("pairs-levels", "gldm", P, cont, mask, Ng, (2,))
        for Ng in (193, 194, 387, 388):
            _add("pairs-nobox", "ngtdm", P, cont, mask, Ng, (2,))
        for Ng in (153, 154, 307, 308):
            _add("pairs-nobox", "ngtdm", P, cont, mask, Ng, (1, 2), no_box=True)
        for dist in ((1,), (1, 2)):
            for Ng in (153, 154, 307, 308, 65535):
                _add("pairs-box", "ngtdm", P, cont, mask, Ng, dist)
        for Ng in (55, 56, 111, 112, 300):
            _add("pairs-box", "ngtdm", P, cont, mask, Ng, (1, 2, 3))
        for shape in ((2, 9, 9), (9, 2, 2), (2, 2, 2)):
            for dist in ((1, 2), (1, 2, 3)):
                _add("pairs-box", "ngtdm", shape, cont, mask, 300, dist)
        for dim in (0, 1, 2):
            _add("pairs-box", "ngtdm", P, cont, mask, 300, (1, 2), f2d=dim)
    _add("pairs-off", "gldm", P, "ramp", "full", 300, no_pairs=True)
    _add("pairs-off", "ngtdm", P, "checker3", "faces", 300, (1, 2), no_pairs=True)
    # ---- pairs tier: GLCM ----
    for r in range(8):
        for cont in ("ramp", "iid"):
            _add("glcm-tail", "glcm", (3, 5, 7 + r), cont, "full", 161)
            _add("glcm-tail", "glcm", (3, 5, 7 + r), cont, "holes4", 8, (1, 2))
    for shape in ((1, 2, 3), (4, 3, 1), (5, 4, 2), (3, 6, 3), (3, 3, 5)):
        for cont in ("ramp", "iid"):
            _add("glcm-narrow", "glcm", shape, cont, "full", 161)
            _add("glcm-narrow", "glcm", shape, cont, "full", 8, (1, 2))
    for cont, mask in (("ramp", "full"), ("iid", "faces")):
        _add("glcm-groups", "glcm", (5, 6, 7), cont, mask, 32, (1, 2))        # 62 angles as 37 + 25
        _add("glcm-groups", "glcm", (5, 6, 7), cont, mask, 138, (2,))         # 49 angles in groups of two, one left over
        _add("glcm-groups", "glcm", (30, 33), cont, mask, 161)
        _add("glcm-groups", "glcm", (30, 33), cont, mask, 16, (1, 2))
    for shape in ((9, 10, 11), (6, 20, 21)):
        for Ng in (195, 196, 197, 240):
            # `cover`: every level of every row tile, the lone level 196 of the last tile included, has pairs in every angle
            # (`ramp` holds only levels 1..94 / 1..113 on these shapes); `lattice`: most tiles see no voxel
            for cont, mask in (("cover", "full"), ("lattice", "full"), ("cover", "faces")):
                _add("glcm-tiles", "glcm", shape, cont, mask, Ng)


_build()
NAMES = tuple(_TABLE)

# inputs of the GPU-only families (no route of their own in the table): the one-pass GLDM + NGTDM call at 202 / 203 levels and
# the plane ranges of the z-slab split
BOTH_INPUTS = [(shape, cont, mask) for shape in QUAD_SHAPES + SCALAR_SHAPES for cont, mask in (("iid", "full"), ("checker3", "faces"))]
SLAB_SHAPES = ((7, 6, 12), (7, 5, 9))


def slab_partitions(Nz):
    """lists of plane ranges, each list a partition of [0, Nz): every split point, single planes, empty ranges, a three-way split"""
    parts = [[(0, z), (z, Nz)] for z in range(Nz + 1)]
    parts.append([(z, z + 1) for z in range(Nz)])
    parts.append([(0, 0), (0, Nz), (Nz, Nz)])
    parts.append([(0, 2), (2, 5), (5, Nz)])
    return parts

# the defects each group of cases exists to catch (tests/test_neigh_reference.py asserts that it does); the "edges:" groups
# answer for possible_edge_defects(shape).  The "degenerate:" groups (one voxel, no voxel, eight far corners: there for the
# empty table, the dead lanes and the route) and "pairs-off" (the PRAD_NO_PAIRS route switch) answer for NO defect: the
# sharpness assertion is vacuous for them on purpose.  The assertion is per group ("some case notices"), except where a
# case must notice on its own: every "edges:" combination (an edge defect) and every "glcm-tiles" case above 195 levels
# (last-tile) -- tests/test_neigh_reference.py checks those one by one.
GROUP_DEFECTS = {
    "big": ("left-edge", "right-edge", "wave-edge", "row-wrap", "plane-wrap"),
    "force2d": ("left-edge", "right-edge", "row-wrap", "plane-wrap"),
    "route-edges": ("row-wrap", "plane-wrap"),
    "pairs-levels": ("row-wrap", "plane-wrap"),
    "pairs-nobox": ("row-wrap", "plane-wrap"),
    "pairs-box": ("row-wrap", "plane-wrap"),
    "pairs-off": (),
    "glcm-tail": ("tail8", "row-wrap", "plane-wrap"),
    "glcm-narrow": ("tail8", "row-wrap", "plane-wrap"),
    "glcm-groups": ("row-wrap",),
    "glcm-tiles": ("last-tile", "row-wrap", "plane-wrap"),
}


def group_defects(group):
    if group.startswith("edges:") or group.startswith("alpha:"):
        return tuple(possible_edge_defects(tuple(int(s) for s in group.split(":")[1].split("x"))))
    if group.startswith("degenerate:"):
        return ()
    return GROUP_DEFECTS[group]


def spec(name):
    return _TABLE[name]


def neighbour_offsets(shape, distances, force2Ddim=None):
    """int64 [Na, Nd]: the bidirectional neighbour set of GLDM / NGTDM as a SET (no particular order) -- every offset whose
    infinity norm is one of `distances`, that stays inside the array in each dimension and does not move along the forced one.
    Only the route labels use it; the matrices are compared under the checker's own list (tests/test_neigh_reference.py
    asserts that the two hold the same offsets)"""
    m = max(distances)
    axes = [[o for o in range(-m, m + 1) if abs(o) < n and (d != force2Ddim or o == 0)] for d, n in enumerate(shape)]
    offs = [o for o in itertools.product(*axes) if max(abs(v) for v in o) in distances]
    return np.array(offs, dtype=np.int64).reshape(len(offs), len(shape))


def case_angles(name, checker):
    """the checker's own angle list of the case (bidirectional for GLDM / NGTDM)"""
    s = _TABLE[name]
    return checker.generate_angles(s["shape"], s["distances"], s["family"] in ("gldm", "ngtdm"), s["force2D"], s["dim"])


@functools.lru_cache(maxsize=8)
def _arrays(shape, cont, mask, Ng):
    return content(cont, shape, Ng), roi(mask, shape)


def case(name):
    """-> (levels int32, mask bool, Ng, distances, alpha, force2D, force2Ddimension, expected route label)"""
    s = _TABLE[name]
    levels, mask = _arrays(s["shape"], s["content"], s["mask"], s["Ng"])
    offs = None
    if s["family"] in ("gldm", "ngtdm"):
        offs = neighbour_offsets(s["shape"], s["distances"], s["dim"] if s["force2D"] else None)
    route = expected_route(s["family"], s["shape"], s["Ng"], offs, s["alpha"], s["no_box"], s["no_pairs"])
    return levels, mask, s["Ng"], s["distances"], s["alpha"], s["force2D"], s["dim"], route


def case_env(name):
    """environment switches of the case (read per call by the library)"""
    s = _TABLE[name]
    env = {}
    if s["no_box"]:
        env["PRAD_NGTDM_NO_BOX"] = "1"
    if s["no_pairs"]:
        env["PRAD_NO_PAIRS"] = "1"
    return env


# ---- comparison helpers of the GPU limit modules (they import the product lazily: this module stays importable without it) --
def check_route(name, route):
    from pyradiomics_amd import _lib
    assert _lib.last_path() == path_of(route), (name, route, _lib.last_path(), _lib.last_variant())
    assert _lib.last_variant() == ("none" if route == "generic" else route), (name, route, _lib.last_variant())


def check_s(name, route, got, acc, Na, ratios):
    """NGTDM column 1 against the correctly rounded s_i under s_bound; records the worst error / bound of the route"""
    exact = ngtdm_s(acc)
    bound = s_bound(exact, Na)
    err = np.abs(got - exact)
    assert np.all(err <= bound), (name, route, float((err / np.where(bound > 0, bound, 1)).max()))
    pos = bound > 0
    if pos.any():
        ratios[route] = max(ratios.get(route, 0.0), float((err[pos] / bound[pos]).max()))
    else:
        ratios.setdefault(route, 0.0)


def run_case(name, checker, ratios, monkeypatch=None):
    """one table case through pyradiomics_amd.cmatrices (host arrays): route, then all outputs"""
    from pyradiomics_amd import cmatrices as cm
    s = spec(name)
    ang = case_angles(name, checker)
    levels, mask, Ng, dist, alpha, f2d, dim, route = case(name)
    env = case_env(name)
    assert not env or monkeypatch is not None
    for k in ("PRAD_NGTDM_NO_BOX", "PRAD_NO_PAIRS"):
        if k in env:
            monkeypatch.setenv(k, env[k])
        elif monkeypatch is not None:
            monkeypatch.delenv(k, raising=False)
    if s["family"] == "glcm":
        got, gang = cm.calculate_glcm(levels, mask, dist, Ng, f2d, dim)
        check_route(name, route)
        want, wang = checker.calculate_glcm(levels, mask, dist, Ng, f2d, dim)
        assert np.array_equal(gang, wang) and np.array_equal(got, want), name
    elif s["family"] == "gldm":
        got = cm.calculate_gldm(levels, mask, dist, Ng, alpha, f2d, dim)
        check_route(name, route)
        assert np.array_equal(got, checker.calculate_gldm(levels, mask, dist, Ng, alpha, f2d, dim)), name
    else:
        got = cm.calculate_ngtdm(levels, mask, dist, Ng, f2d, dim)
        check_route(name, route)
        want = checker.calculate_ngtdm(levels, mask, dist, Ng, f2d, dim)
        assert got.shape == want.shape and np.array_equal(got[..., 0], want[..., 0]) and np.array_equal(got[..., 2], want[..., 2]), name
        check_s(name, route, got[0, :, 1], accumulators(levels, mask, Ng, ang)[1], len(ang), ratios)
    return route


def report(title, ratios):
    print("\n%s: worst |got - exact| / bound of NGTDM column 1 per route" % title)
    for route in sorted(ratios):
        print("    %-28s %.3g" % (route, ratios[route]))
    bad = {r: v for r, v in ratios.items() if not v <= 1.0}
    assert not bad, bad

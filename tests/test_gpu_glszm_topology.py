"""GLSZM zone labelling on adversarial topologies and tile seams.

Every other GLSZM test feeds the kernels noise, which makes compact blobs.  The volumes here are constructed: one-voxel-wide
paths through every tile, zones held together by corner contacts only, every two-level pattern on the eight voxels around a
tile corner, combs that enter and leave a tile many times, tiles of 4096 single-voxel zones, masks that cut a zone or leave
only tile faces.  Each generator returns, next to the volume, the zone census {(level, size): count} it was built to have,
derived from its parameters (tests/test_glszm_reference.py checks those closed forms on the CPU against
tests/glszm_reference.py -- scipy.ndimage.label per grey level -- and against the C checker).  A test here has up to three
witnesses: the closed form, the scipy restatement and the C checker.  All comparisons are integer and exact, except the
feature values of test_one_queue_features, which inherit the bounds of tests/feature_reference.py
(zone_bounds with the chain-length constants of test_gpu_segment_feature_limits.py) unchanged.

What `_check` asserts for a volume and a neighbourhood: compact (P, sizes) == reference; zone count and largest zone == closed
form; the ordered zone list (prad_glszm_zones) == the reference's raster discovery order, asked twice (the first call turns
the dense path's id volume into the published label view, the second reads that view); a second labelling on the same
workspace gives the same bits; the dense matrix == reference == C checker where it fits; the zone list once more after the
dense call.  On a mismatch of the zone list the message names the first wrong zone, its first voxel, the nearest tile corner
and prints the levels around it.

Tile grid: 8 (z) x 8 (y) x 64 (x).  Routes and the cases that reach them are listed at each test, and each test asserts the
route its calls took: prad_last_variant() names the host's choice (csrc/prad_glszm_plan.h), after the retry of an irregular
level; whether the work list overflowed is decided on the device and is not in the name.

One kernel bug was found and fixed, in the ordered zone list only (matrices, zone counts and sizes were right throughout):
glszm_zmin_kernel took parent[id] for the zone root, but glszm_rootsum_dense_kernel leaves parent[] only nearly flat -- see
test_zone_order_when_the_parent_chains_are_not_flat.  On the kernels before the fix 9 of the 562 cases of this module failed,
all on the order of two zones; with the fix all 563 pass (18 s on an MI355X).

Sharpness.  One-line mutations of the kernels (csrc/kernels_glszm_dense.h, kernels_glszm_labels.h) in scratch builds (loaded
through PRAD_LIB, never committed), each run once against this module on an MI355X, and the tests that failed (number of
failing cases in brackets):
    N2 grown without the `S2 &` restriction (pairs pruned through voxels of another level)                       [136]
        test_default_route (71), test_work_list_capacities, test_serpentine_and_combs_along_every_axis, test_random_blocks_on_seams,
        test_int32_route_by_irregular_level, test_level_shards, test_one_queue_features, test_pairs_kernel_grid,
        test_large_volume_compact, test_2d_input
    PRAD_T8_JUMPS 3 -> 0, PRAD_T8_FLOOD 2 -> 1, PRAD_T8_FLOOD 2 -> 4                                                  [0, 0, 0]
        must pass -- optimisations by the kernel's own comments -- and do: all 563 cases each
    one bit of rowcross dropped (0xe00 -> 0xc00 in the ly == PRAD_TY - 1 term)                                         [11]
        test_random_blocks_on_seams (4), test_default_route[stairs-+1-1+1-*] (3), test_work_list_capacities[stairs-+1-1+1-*],
        test_work_list_capacities_on_random_blocks
    the `k == 3 && lx4 == 15` term of cross dropped                                                                    [112]
        test_default_route (50), test_work_list_capacities, test_random_blocks_on_seams, test_level_shards,
        test_one_queue_features, test_int32_route_by_irregular_level, test_pairs_kernel_grid, test_2d_input,
        test_large_volume_compact
    `a < b` -> `a > b` in dn_union (the union is lost)                                                                  [470]
        every test that labels more than one tile
    `parent[j] = r` (the flatten) skipped in glszm_rootsum_dense_kernel                                                 [0]
        passes, and must since the fix: no kernel relies on a flat parent[] any more, the store only shortens later walks.
        The kernels before the fix relied on it in glszm_zmin_kernel; that is the mutation below.
    glszm_zmin_kernel takes parent[id] for the root again (the fix reverted)                                            [7]
        test_zone_order_when_the_parent_chains_are_not_flat, test_serpentine_and_combs_along_every_axis (3),
        test_work_list_capacities, test_work_list_capacities_on_random_blocks, test_random_blocks_on_seams
    tile origin off by one in the border scans (z % PRAD_TZ == 1 in row_edge of glszm_border8d_kernel and                [5]
    glszm_border_full_kernel)
        test_work_list_capacities[stairs-+1-1+1-+1+0+0-3d-1 / -37], test_work_list_capacities_on_random_blocks,
        test_int32_route_by_level_count[stairs-+1-1+1-+1+0+0-3d-256 / -300]
    one corrupted entry of t8_sel13 (entry 5 answers 1: the second of two unconnected neighbours is dropped)            [41]
        test_random_blocks_on_seams (12), test_default_route (12), test_work_list_capacities, test_2d_input,
        test_int32_route_by_irregular_level, test_pairs_kernel_grid, test_one_queue_features, test_large_volume_compact
None timed out.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import glszm_reference as gr

pytestmark = pytest.mark.gpu

TZ, TY, TX = 8, 8, 64                      # PRAD_TZ, PRAD_TY, PRAD_TX
DENSE_MAX = 1 << 22                        # entries of a dense matrix a test still asks for (32 MB)
CHECKER_MAX = 3 << 20                      # voxels the C flood fill is asked to label


class Vol:
    """a constructed volume: img int32, mask bool, Ng, and the closed-form censuses {(level, size): count} under the full
    neighbourhood (`cen`) and under the in-plane 8-neighbourhood of force2D along axis 0 (`cen2`); None = no closed form"""

    def __init__(self, name, img, mask, Ng, cen, cen2=None):
        self.name, self.img, self.Ng, self.cen, self.cen2 = name, np.ascontiguousarray(img, dtype=np.int32), Ng, cen, cen2
        self.mask = np.ones(self.img.shape, bool) if mask is None else np.ascontiguousarray(mask, dtype=bool)
        self._zones = {}

    def zones(self, force2D=False, f2d=0):
        key = (bool(force2D), f2d if force2D else 0)
        if key not in self._zones:
            self._zones[key] = gr.zones(self.img, self.mask, force2D, f2d)
        return self._zones[key]

    def closed(self, force2D=False, f2d=0):
        if not force2D:
            return self.cen
        return self.cen2 if f2d == 0 else None

    def transposed(self, axes):
        """the same volume with its axes permuted: the full neighbourhood does not care, the in-plane one does"""
        return Vol("%s.T%s" % (self.name, "".join(map(str, axes))), self.img.transpose(axes), self.mask.transpose(axes),
                   self.Ng, self.cen, None)


def _add(cen, level, size, count=1):
    if size > 0 and count > 0:
        cen[(level, size)] = cen.get((level, size), 0) + count
    return cen


# ---- serpentines and spirals ------------------------------------------------------------------------------------------
def serp_plane(Ny, Nx, x_lo=0, x_hi=None, y_off=0):
    """one plane of the serpentine: lanes of level 1 along x in the rows y_off, y_off + 2, ... over x_lo..x_hi, joined at
    alternating ends through the wall rows of level 2 between them.  -> plane, start, end, path length, in-plane census"""
    x_hi = Nx - 1 if x_hi is None else x_hi
    ys = list(range(y_off, Ny, 2))
    nl, W = len(ys), x_hi - x_lo + 1
    plane = np.full((Ny, Nx), 2, dtype=np.int32)
    for i, y in enumerate(ys):
        plane[y, x_lo:x_hi + 1] = 1
        if i + 1 < nl:
            plane[y + 1, x_hi if i % 2 == 0 else x_lo] = 1
    start, end = (ys[0], x_lo), (ys[-1], x_hi if nl % 2 else x_lo)
    per = nl * W + nl - 1
    cen2 = _add({}, 1, per)
    if x_lo == 0 and x_hi == Nx - 1:
        _add(cen2, 2, Nx - 1, nl - 1)                      # the wall rows between two lanes, minus the joint
        _add(cen2, 2, Nx, y_off + (Ny - 1 - ys[-1]))        # whole wall rows before the first and after the last lane
    else:
        # a wall row between two lanes is shut in when the end opposite its joint meets the volume's border; every other
        # wall voxel reaches the columns outside the lanes
        shut = sum(1 for i in range(nl - 1) if (x_lo == 0 if i % 2 == 0 else x_hi == Nx - 1))
        _add(cen2, 2, W - 1, shut)
        _add(cen2, 2, Ny * Nx - per - shut * (W - 1))
    return plane, start, end, per, cen2


@functools.lru_cache(maxsize=None)
def serpentine(shape, x_lo=0, x_hi=None, y_off=0, z_off=0, cut=None):
    """A one-voxel-wide path of level 1 through walls of level 2: the planes z_off, z_off + 2, ... hold serp_plane, every
    other plane is wall except for ONE voxel that joins the end of the plane below to the plane above (which the path then
    walks backwards).  Under the full neighbourhood the path is one zone of known length and the walls are one zone.
    cut = z of a joining plane: the mask removes its joint and the path falls into two zones of known lengths."""
    Nz, Ny, Nx = shape
    plane, S, E, per, pcen2 = serp_plane(Ny, Nx, x_lo, x_hi, y_off)
    img = np.full(shape, 2, dtype=np.int32)
    mask = np.ones(shape, bool)
    pieces, ones = [0], 0
    cen2 = {} if pcen2 is not None else None
    for z in range(Nz):
        if (z - z_off) % 2 == 0:
            img[z] = plane
            pieces[-1] += per
            ones += per
            if cen2 is not None:
                for (g, s), c in pcen2.items():
                    _add(cen2, g, s, c)
        else:
            k = (z - z_off - 1) // 2
            c = E if k % 2 == 0 else S
            img[z][c] = 1
            ones += 1
            if cut == z:
                mask[z][c] = False
                pieces.append(0)
            else:
                pieces[-1] += 1
            if cen2 is not None:
                _add(cen2, 1, 1, 0 if cut == z else 1)
                _add(cen2, 2, Ny * Nx - 1)
    cen = {}
    for p in pieces:
        _add(cen, 1, p)
    _add(cen, 2, Nz * Ny * Nx - ones)
    name = "serpentine%s[x%d..%s,y%d,z%d%s]" % (shape, x_lo, x_hi, y_off, z_off, "" if cut is None else ",cut%d" % cut)
    return Vol(name, img, mask, 2, cen, cen2)


@functools.lru_cache(maxsize=None)
def helix(shape):
    """a 3-D spiral: plane 2k holds side k mod 4 of the rectangle's perimeter, plane 2k + 1 the one voxel at the corner where
    that side ends and the next begins.  One zone of level 1, the rest (level 2) one zone."""
    Nz, Ny, Nx = shape
    img = np.full(shape, 2, dtype=np.int32)
    corners = [(0, 0), (0, Nx - 1), (Ny - 1, Nx - 1), (Ny - 1, 0)]
    L, cen2 = 0, {}
    for z in range(Nz):
        if z % 2 == 0:
            side = (z // 2) % 4
            if side == 0:
                img[z, 0, :] = 1
            elif side == 1:
                img[z, :, Nx - 1] = 1
            elif side == 2:
                img[z, Ny - 1, :] = 1
            else:
                img[z, :, 0] = 1
            n = Nx if side % 2 == 0 else Ny
        else:
            img[z][corners[((z - 1) // 2 + 1) % 4]] = 1
            n = 1
        L += n
        _add(cen2, 1, n)
        _add(cen2, 2, Ny * Nx - n)
    cen = _add(_add({}, 1, L), 2, Nz * Ny * Nx - L)
    return Vol("helix%s" % (shape,), img, None, 2, cen, cen2)


# ---- corner-only and edge-only contacts ---------------------------------------------------------------------------------
def _residues(n, m):
    return [n // m + (1 if r < n % m else 0) for r in range(m)]


@functools.lru_cache(maxsize=None)
def checkerboard(shape, m=2):
    """level 1 + (sum of the coordinates) mod m, any rank.  Under the full neighbourhood every colour is ONE zone held together
    by diagonal contacts only (m = 2: across the body and face diagonals; m = 3: along the anti-diagonals of every plane and
    across the (1, 1, 1) diagonal).  In-plane (force2D axis 0, 3-D only): m = 2 one zone per colour and slice, m = 3 every
    anti-diagonal of a slice is a zone of its own."""
    idx = sum(np.arange(n, dtype=np.int32).reshape([-1 if d == a else 1 for d in range(len(shape))]) for a, n in enumerate(shape))
    img = (1 + idx % m).astype(np.int32)
    tot = [1] + [0] * (m - 1)
    for n in shape:                                        # voxels per residue of the coordinate sum: a cyclic convolution
        r = _residues(n, m)
        tot = [sum(tot[a] * r[(k - a) % m] for a in range(m)) for k in range(m)]
    cen = {}
    for k in range(m):
        _add(cen, 1 + k, tot[k])
    cen2 = None
    if len(shape) == 3:
        Nz, Ny, Nx = shape
        cen2 = {}
        for z in range(Nz):
            if m == 2:
                e0 = (Ny * Nx + (Ny % 2) * (Nx % 2)) // 2
                _add(cen2, 1 + z % 2, e0)
                _add(cen2, 1 + (z + 1) % 2, Ny * Nx - e0)
            else:
                for d in range(Ny + Nx - 1):
                    _add(cen2, 1 + (z + d) % m, min(d, Ny - 1, Nx - 1, Ny + Nx - 2 - d) + 1)
    return Vol("checkerboard%s/%d" % (shape, m), img, None, m, cen, cen2)


DIAGONALS = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]


@functools.lru_cache(maxsize=None)
def staircases(shape, step, base):
    """parallel diagonal lines of level 1 with direction `step` through base + (0, 0, 3 i), every i that meets the volume, on
    level 2: each line is one zone (its voxels touch by the diagonal only), its length the number of t with base + t step
    inside the volume.  base = the tile corner (8, 8, 64) sends line 0 through a tile corner and the others through tile
    edges and faces; shifting the base by one voxel along an axis changes which step meets which seam."""
    Nz, Ny, Nx = shape
    img = np.full(shape, 2, dtype=np.int32)
    cen, total = {}, 0
    per_plane = [0] * Nz
    lens2 = []
    for i in range(-(Nx + Ny + Nz) // 3 - 1, (Nx + Ny + Nz) // 3 + 2):
        p0 = (base[0], base[1], base[2] + 3 * i)
        lo, hi = -10 ** 9, 10 ** 9
        for p, s, n in zip(p0, step, shape):
            if s == 0:
                if not 0 <= p < n:
                    lo, hi = 1, 0
            else:
                a, b = (-p, n - 1 - p) if s > 0 else (p - (n - 1), p)
                lo, hi = max(lo, a), min(hi, b)
        if hi < lo:
            continue
        T = hi - lo + 1
        for t in range(lo, hi + 1):
            img[p0[0] + t * step[0], p0[1] + t * step[1], p0[2] + t * step[2]] = 1
            per_plane[p0[0] + t * step[0]] += 1
        _add(cen, 1, T)
        lens2.append(T)
        total += T
    _add(cen, 2, Nz * Ny * Nx - total)
    cen2 = {}
    if step[0] != 0:
        _add(cen2, 1, 1, total)                             # one voxel of a line per plane
    else:
        for T in lens2:
            _add(cen2, 1, T)
    for z in range(Nz):
        _add(cen2, 2, Ny * Nx - per_plane[z])
    return Vol("staircases%s step%s base%s" % (shape, step, base), img, None, 2, cen, cen2)


# ---- exhaustive seams ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corner_patterns(shape):
    """Every tile corner inside the volume carries a 2 x 2 x 2 block centred on it -- one voxel in each of the eight tiles that
    meet there -- with the two-level pattern number (corner index mod 256): bit 4a + 2b + c set = level 1 at offset
    (a - 1, b - 1, c - 1), else level 2.  Background level 3; the blocks are a tile apart, so each is isolated.  The voxels
    of a block touch each other, so it holds one zone per level present; in-plane each of its two slices does."""
    Nz, Ny, Nx = shape
    img = np.full(shape, 3, dtype=np.int32)
    cen, cen2 = {}, {}
    in_plane = [0] * Nz
    corners = [(cz, cy, cx) for cz in range(TZ, Nz, TZ) for cy in range(TY, Ny, TY) for cx in range(TX, Nx, TX)]
    for i, (cz, cy, cx) in enumerate(corners):
        p = i % 256
        for a in range(2):
            k2 = 0
            for b in range(2):
                for c in range(2):
                    bit = (p >> (4 * a + 2 * b + c)) & 1
                    img[cz - 1 + a, cy - 1 + b, cx - 1 + c] = 1 if bit else 2
                    k2 += bit
            _add(cen2, 1, k2)
            _add(cen2, 2, 4 - k2)
            in_plane[cz - 1 + a] += 4
        k = bin(p).count("1")
        _add(cen, 1, k)
        _add(cen, 2, 8 - k)
    _add(cen, 3, Nz * Ny * Nx - 8 * len(corners))
    for z in range(Nz):
        _add(cen2, 3, Ny * Nx - in_plane[z])
    v = Vol("corner_patterns%s" % (shape,), img, None, 3, cen, cen2)
    v.corners = corners
    return v


@functools.lru_cache(maxsize=None)
def random_blocks(shape, shift, seed, levels=2):
    """random 4 x 4 x 4 blocks of `levels` levels centred on the points (8 i, 8 j, 8 k) + shift, background level levels + 1,
    a moat of 4 voxels between blocks.  shift (0, 0, 0): the blocks sit on tile corners (x a multiple of 64) and on z-y tile
    edges; (4, 0, 0): on y-x edges and y faces; (4, 4, 0): on x faces or inside a tile.  No closed form: scipy and the C
    checker are the witnesses."""
    Nz, Ny, Nx = shape
    rng = np.random.default_rng(seed)
    img = np.full(shape, levels + 1, dtype=np.int32)
    n = 0
    for cz in range(8 + shift[0], Nz - 2, 8):
        for cy in range(8 + shift[1], Ny - 2, 8):
            for cx in range(8 + shift[2], Nx - 2, 8):
                img[cz - 2:cz + 2, cy - 2:cy + 2, cx - 2:cx + 2] = rng.integers(1, levels + 1, size=(4, 4, 4))
                n += 1
    v = Vol("random_blocks%s shift%s seed%d/%d" % (shape, shift, seed, levels), img, None, levels + 1, None, None)
    v.nblocks = n
    return v


# ---- combs and re-entrant zones ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def combs(shape):
    """two interleaved combs in every even plane: level 1 has its spine in row 0 and teeth down the even columns, level 2 its
    spine in the last row and teeth up the odd columns; the odd planes are level 3.  Each comb is one zone that enters and
    leaves every tile of its plane once per tooth; the census is the same in-plane."""
    Nz, Ny, Nx = shape
    img = np.full(shape, 3, dtype=np.int32)
    plane = np.empty((Ny, Nx), dtype=np.int32)
    plane[:, 0::2] = 1
    plane[:, 1::2] = 2
    plane[0, :] = 1
    plane[Ny - 1, :] = 2
    img[0::2] = plane
    ne, no = (Nz + 1) // 2, Nz // 2
    cen = {}
    _add(cen, 1, Nx + ((Nx + 1) // 2) * (Ny - 2), ne)
    _add(cen, 2, Nx + (Nx // 2) * (Ny - 2), ne)
    _add(cen, 3, Ny * Nx, no)
    return Vol("combs%s" % (shape,), img, None, 3, cen, dict(cen))


# ---- component-count limits ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def singles(shape, Ng, seed=0, drop=0):
    """every voxel a zone of its own: level 1 + 8 k + colour with colour = (x & 1) + 2 (y & 1) + 4 (z & 1), k arbitrary; two
    voxels that touch differ in a coordinate's parity, hence in colour, hence in level -- across tile borders too.  A full
    tile holds 4096 zones, four times PRAD_GZ_TILE_ROOTS.  drop: that many voxels masked out (sets the parity of the count)."""
    assert Ng >= 8
    rng = np.random.default_rng(seed)
    z, y, x = np.indices(shape)
    colour = (x & 1) + 2 * (y & 1) + 4 * (z & 1)
    lvl = 1 + 8 * rng.integers(0, (Ng - 8) // 8 + 2, size=shape) + colour
    lvl = np.where(lvl > Ng, lvl - 8, lvl).astype(np.int32)
    mask = np.ones(shape, bool)
    mask.reshape(-1)[:drop] = False
    cen = {}
    for g, c in enumerate(np.bincount(lvl[mask], minlength=Ng + 1)):
        _add(cen, g, 1, int(c))
    return Vol("singles%s Ng%d drop%d" % (shape, Ng, drop), lvl, mask, Ng, cen, dict(cen))


@functools.lru_cache(maxsize=None)
def uniform(shape, level, Ng):
    n = int(np.prod(shape))
    cen2 = _add({}, level, int(np.prod(shape[1:])), shape[0]) if len(shape) == 3 else None
    return Vol("uniform%s level%d/%d" % (shape, level, Ng), np.full(shape, level, dtype=np.int32), None, Ng, _add({}, level, n), cen2)


# ---- masks that cut --------------------------------------------------------------------------------------------------------
def _tile_extents(n, T):
    """summed extents of the even and of the odd tiles along an axis of n voxels"""
    ext = [min(T, n - t) for t in range(0, n, T)]
    return [sum(ext[0::2]), sum(ext[1::2])]


@functools.lru_cache(maxsize=None)
def tile_checker_mask(shape, level=2, Ng=3):
    """one level everywhere, the mask keeps the tiles of even index sum: whole empty tiles between occupied ones, and the
    occupied tiles touch along tile edges and at tile corners only -- one zone.  In-plane: one zone per slice."""
    Nz, Ny, Nx = shape
    z, y, x = np.indices(shape)
    mask = ((z // TZ + y // TY + x // TX) % 2) == 0
    Z, Y, X = _tile_extents(Nz, TZ), _tile_extents(Ny, TY), _tile_extents(Nx, TX)
    assert Y[1] and X[1], "needs two tiles along y and along x"
    cen = _add({}, level, sum(Z[a] * Y[b] * X[c] for a in range(2) for b in range(2) for c in range(2) if (a + b + c) % 2 == 0))
    cen2 = {}
    for zz in range(Nz):
        a = (zz // TZ) % 2
        _add(cen2, level, sum(Y[b] * X[c] for b in range(2) for c in range(2) if (a + b + c) % 2 == 0))
    return Vol("tile_checker_mask%s" % (shape,), np.full(shape, level, dtype=np.int32), mask, Ng, cen, cen2)


def _interior(n, T):
    """coordinates along an axis that are neither the first nor the last of their tile"""
    return (n // T) * (T - 2) + max(0, n % T - 1)


@functools.lru_cache(maxsize=None)
def tile_face_mask(shape, level=1, Ng=2):
    """one level everywhere, the mask keeps only the voxels on a tile face: a lattice of slabs, one zone"""
    Nz, Ny, Nx = shape
    z, y, x = np.indices(shape)
    fz, fy, fx = (z % TZ == 0) | (z % TZ == TZ - 1), (y % TY == 0) | (y % TY == TY - 1), (x % TX == 0) | (x % TX == TX - 1)
    Iz, Iy, Ix = _interior(Nz, TZ), _interior(Ny, TY), _interior(Nx, TX)
    cen = _add({}, level, Nz * Ny * Nx - Iz * Iy * Ix)
    cen2 = _add(_add({}, level, Ny * Nx, Nz - Iz), level, Ny * Nx - Iy * Ix, Iz)
    return Vol("tile_face_mask%s" % (shape,), np.full(shape, level, dtype=np.int32), fz | fy | fx, Ng, cen, cen2)


# ---- the catalogue -------------------------------------------------------------------------------------------------------------
# shapes straddle the tile grid: Nx 63 / 64 / 65 / 127 / 128 / 130, Ny and Nz 7 / 8 / 9 / 17, rows with and without whole quads
SHAPES = [(7, 9, 63), (8, 8, 64), (9, 17, 65), (17, 8, 127), (17, 9, 130), (8, 7, 128), (17, 17, 64)]
BIG = (24, 33, 196)                        # 3 x 5 x 4 tiles, whole quads
CORNER = (TZ, TY, TX)


def catalogue():
    """(id, constructor) of every constructed volume with a closed form -- the CPU tier checks each census"""
    out = []
    for s in SHAPES + [BIG]:
        out.append(("serp-%dx%dx%d" % s, lambda s=s: serpentine(s)))
        out.append(("helix-%dx%dx%d" % s, lambda s=s: helix(s)))
        out.append(("chk2-%dx%dx%d" % s, lambda s=s: checkerboard(s, 2)))
        out.append(("chk3-%dx%dx%d" % s, lambda s=s: checkerboard(s, 3)))
        out.append(("combs-%dx%dx%d" % s, lambda s=s: combs(s)))
    # the path turns one voxel before a tile face, exactly on it, one voxel after it -- in x, and the planes / rows shifted
    for x_hi in (62, 63, 64):
        out.append(("serp-turn-xhi%d" % x_hi, lambda x_hi=x_hi: serpentine((17, 17, 130), 0, x_hi)))
    for x_lo in (63, 64, 65):
        out.append(("serp-turn-xlo%d" % x_lo, lambda x_lo=x_lo: serpentine((17, 17, 130), x_lo, 129)))
    out.append(("serp-yoff1", lambda: serpentine((17, 17, 130), 0, None, 1, 0)))
    out.append(("serp-zoff1", lambda: serpentine((17, 17, 130), 0, None, 0, 1)))
    out.append(("serp-yzoff1-x5..127", lambda: serpentine((17, 17, 130), 5, 127, 1, 1)))
    for cut in (1, 7, 9):                  # the mask removes the joint below, at and above the first tile face in z
        out.append(("serp-cut%d" % cut, lambda cut=cut: serpentine((17, 17, 130), cut=cut)))
    for step in DIAGONALS:
        for base in (CORNER, (TZ + 1, TY, TX), (TZ, TY + 1, TX)):
            out.append(("stairs-%s-%s" % ("".join("%+d" % v for v in step), "".join("%+d" % (b - c) for b, c in zip(base, CORNER))),
                        lambda step=step, base=base: staircases((17, 17, 130), step, base)))
    out.append(("corners-131", lambda: corner_patterns((100, 92, 131))))
    out.append(("corners-132", lambda: corner_patterns((100, 92, 132))))
    for Ng in (8, 254, 255):
        out.append(("singles-tile-Ng%d" % Ng, lambda Ng=Ng: singles((8, 8, 64), Ng)))
    out.append(("singles-many-Ng255", lambda: singles((17, 17, 130), 255, 1)))
    out.append(("singles-quads-Ng255", lambda: singles((16, 24, 128), 255, 2)))
    out.append(("uniform-big", lambda: uniform(BIG, 3, 5)))
    out.append(("uniform-Ng1", lambda: uniform((17, 9, 130), 1, 1)))
    for s in ((17, 17, 130), (16, 16, 128), BIG):
        out.append(("tilechecker-%dx%dx%d" % s, lambda s=s: tile_checker_mask(s)))
        out.append(("tilefaces-%dx%dx%d" % s, lambda s=s: tile_face_mask(s)))
    return out


CATALOGUE = catalogue()
CATALOGUE_IDS = [k for k, _ in CATALOGUE]
BY_ID = dict(CATALOGUE)
# the volumes with many tiles and many cross-tile ties: the subset the alternative routes are driven with
MULTI_TILE = ["serp-24x33x196", "serp-17x9x130", "serp-turn-xhi63", "serp-cut7", "helix-24x33x196", "chk2-24x33x196",
              "chk2-17x9x130", "chk3-24x33x196", "combs-24x33x196", "corners-131", "corners-132", "singles-many-Ng255",
              "uniform-big", "tilechecker-24x33x196", "tilefaces-17x17x130", "stairs-+1+1+1-+0+0+0", "stairs-+1-1+1-+1+0+0"]


# ---- what a test asserts ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cm():
    from pyradiomics_amd import cmatrices
    return cmatrices


def _gpu_zone_list(cap):
    import ctypes as C
    from pyradiomics_amd import _lib
    buf = np.empty(2 * cap + 1, dtype=np.intc)
    n = _lib.load().prad_glszm_zones(0, buf.ctypes.data_as(C.POINTER(C.c_int)), cap)
    assert n >= 0, "prad_glszm_zones failed: %d" % n
    return buf[:2 * n + 1].copy()


def _explain(vol, z, got):
    """where the zone list first departs from the reference: the zone, its first voxel, the nearest tile corner, the levels"""
    want = gr.zone_list(z)
    n = min(len(want), len(got))
    d = np.flatnonzero(want[:n] != got[:n])
    i = int(d[0]) // 2 if len(d) else n // 2
    msg = "%s: %d zones, reference %d" % (vol.name, (len(got) - 1) // 2, len(z))
    if i < len(z) and vol.img.ndim == 3:
        first = np.unravel_index(int(z[i, 2]), vol.img.shape)
        corner = tuple(int(round(c / t)) * t for c, t in zip(first, (TZ, TY, TX)))
        lo = [max(0, c - 2) for c in corner]
        block = np.where(vol.mask, vol.img, 0)[lo[0]:corner[0] + 2, lo[1]:corner[1] + 2, lo[2]:corner[2] + 2]
        msg += "; zone %d is (level %d, size %d) first voxel %s, got %s; nearest tile corner %s, levels there (0 = masked):\n%s" % (
            i, z[i, 0], z[i, 1], first, tuple(got[2 * i:2 * i + 2]), corner, block)
    return msg


def _variant():
    from pyradiomics_amd import _lib
    return _lib.last_variant()


def _dense(force2D):
    """the name of the dense route (prad_last_variant): 26-neighbourhood, or the in-plane 8 of force2D along axis 0"""
    return "dense8" if force2D else "dense26"


def _int32(force2D):
    return "tiles-full8" if force2D else "tiles-full26"


def _check(cm, checker, vol, force2D=False, f2d=0, Ng=None, dense=True, route=None):
    """everything the module docstring lists, for one volume and one neighbourhood; -> number of GPU labellings made.
    route: the name prad_last_variant() must give after every labelling (the host's choice, after any retry)"""
    Ng = vol.Ng if Ng is None else Ng
    img, mask = vol.img, vol.mask
    Ns = int(mask.sum())
    z = vol.zones(force2D, f2d)
    closed = vol.closed(force2D, f2d)
    if closed is not None:
        assert gr.census(z) == closed, "%s: the scipy reference departs from the closed form" % vol.name
    Pr, sr = gr.compact(z, Ng)
    want_list = gr.zone_list(z)
    P, s = cm.calculate_glszm_compact(img, mask, Ng, Ns, force2D, f2d)
    assert route is None or _variant() == route, "%s: route %s, expected %s" % (vol.name, _variant(), route)
    nz, largest = int(P.sum()), (int(s[-1]) if len(s) else 0)
    assert nz == len(z) and largest == (int(z[:, 1].max()) if len(z) else 0), \
        "%s: %d zones, largest %d; reference %d, %d" % (vol.name, nz, largest, len(z), int(z[:, 1].max()) if len(z) else 0)
    if closed is not None:
        assert nz == sum(closed.values()) and largest == max(sz for _, sz in closed)
    assert np.array_equal(s, sr) and np.array_equal(P[0], Pr), "%s: compact matrix" % vol.name
    for again in range(2):                 # the first call publishes the label view, the second reads it
        got = _gpu_zone_list(Ns)
        assert np.array_equal(got, want_list), "zone list (call %d) " % (again + 1) + _explain(vol, z, got)
    P2, s2 = cm.calculate_glszm_compact(img, mask, Ng, Ns, force2D, f2d)     # same workspace: stale rootctl, bitmaps, lists
    assert np.array_equal(s2, s) and np.array_equal(P2, P), "%s: second call on the same workspace" % vol.name
    assert route is None or _variant() == route
    calls = 2
    if dense and Ng * max(largest, 1) <= DENSE_MAX:
        D = cm.calculate_glszm(img, mask, Ng, Ns, force2D, f2d)
        assert route is None or _variant() == route
        want = gr.matrix(z, Ng)
        assert D.shape == want.shape and np.array_equal(D, want), "%s: dense matrix" % vol.name
        got = _gpu_zone_list(Ns)
        assert np.array_equal(got, want_list), "zone list after the dense call " + _explain(vol, z, got)
        calls += 1
        if checker is not None and img.size <= CHECKER_MAX:
            assert np.array_equal(checker.calculate_glszm(img, mask, Ng, Ns, force2D, f2d), want), "%s: C checker" % vol.name
    return calls


# ---- route 1: the default dense packed-byte route, 26-neighbourhood (mode 1) and force2D along axis 0 (mode 2) -------------
@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
@pytest.mark.parametrize("case", CATALOGUE_IDS)
def test_default_route(cm, checker, case, force2D):
    from pyradiomics_amd import _lib
    _check(cm, checker, BY_ID[case](), force2D, 0, route=_dense(force2D))
    assert _lib.last_path() == "glszm-unionfind"


@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
@pytest.mark.parametrize("axes", [(0, 2, 1), (2, 1, 0), (1, 2, 0)], ids=["lanes-y", "lanes-z", "lanes-y-planes-x"])
@pytest.mark.parametrize("shape", [(17, 9, 130), (9, 66, 17), BIG])
def test_serpentine_and_combs_along_every_axis(cm, checker, shape, axes, force2D):
    """the boustrophedon runs along y and along z, the teeth of the combs likewise: the generators' volumes with their axes
    permuted (the census under the full neighbourhood is that of the original; in-plane scipy and the C checker decide)"""
    for vol in (serpentine(shape), combs(shape), helix(shape)):
        _check(cm, checker, vol.transposed(axes), force2D, 0)


@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
@pytest.mark.parametrize("shift", [(0, 0, 0), (4, 0, 0), (4, 4, 0)], ids=["corners+zy-edges", "yx-edges+y-faces", "x-faces"])
@pytest.mark.parametrize("Nx,levels", [(264, 2), (262, 3)])
def test_random_blocks_on_seams(cm, checker, shift, Nx, levels, force2D):
    """2048 random 4 x 4 x 4 blocks per volume (12288 in all) over tile corners, edges and faces"""
    vol = random_blocks((72, 72, Nx), shift, 7 + Nx, levels)
    assert vol.nblocks >= 1792
    _check(cm, checker, vol, force2D, 0)


def test_zone_order_when_the_parent_chains_are_not_flat(cm):
    """Regression.  glszm_rootsum_dense_kernel leaves parent[] only nearly flat (a path-halving store of one lane's find can
    land after the owner's store and put an entry back on an ancestor short of the root) and glszm_zmin_kernel took parent[id]
    for the zone root: the first voxel of a zone whose tile components form a chain of five or more was then missed, and
    the ordered zone list came out with two zones swapped -- now and then, it is a race (9 of 562 cases of this module on
    the kernels before the fix; matrices, counts and sizes were right throughout).  The smallest volume that showed it: ONE
    2 x 2 x 2 block on the tile corner (8, 8, 64) of a 16 x 16 x 128 volume, pattern 245 -- six voxels of level 1 in six
    tiles, two of level 2 whose first voxel is the very next index.  Asked many times, with the transposed serpentine (two
    zones, the first voxels 0 and 1) that showed it too."""
    img = np.full((16, 16, 128), 3, dtype=np.int32)
    img[7:9, 7:9, 63:65] = np.array([[[1, 2], [1, 2]], [[1, 1], [1, 1]]])
    small = Vol("corner block 245", img, None, 3, _add(_add(_add({}, 1, 6), 2, 2), 3, img.size - 8))
    long = serpentine(BIG).transposed((2, 1, 0))
    for vol, times in ((small, 40), (long, 10)):
        want = gr.zone_list(vol.zones())
        for _ in range(times):
            cm.calculate_glszm_compact(vol.img, vol.mask, vol.Ng, vol.img.size, False, 0)
            got = _gpu_zone_list(vol.img.size)
            assert np.array_equal(got, want), _explain(vol, vol.zones(), got)


# ---- route 2: the work list at 1, 37 and more entries than any volume here needs --------------------------------------------
@pytest.mark.parametrize("workcap", [1, 37, 1 << 24])
@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
@pytest.mark.parametrize("case", MULTI_TILE)
def test_work_list_capacities(cm, checker, case, force2D, workcap, monkeypatch):
    """PRAD_GLSZM_WORKCAP is read on every call.  The overflow is decided per tile on the device: at 37 some tiles have listed
    their pairs before a later one finds the list full, at 1 none has; glszm_border8d_kernel must cope with both, and a list
    that never fills must give what the default capacity gives."""
    monkeypatch.setenv("PRAD_GLSZM_WORKCAP", str(workcap))
    _check(cm, None, BY_ID[case](), force2D, 0, route=_dense(force2D))     # (the overflow is the device's choice: not in the name)


def test_work_list_capacities_on_random_blocks(cm, monkeypatch):
    for workcap in (1, 37, 1 << 24):
        monkeypatch.setenv("PRAD_GLSZM_WORKCAP", str(workcap))
        for force2D in (False, True):
            _check(cm, None, random_blocks((72, 72, 264), (0, 0, 0), 271, 2), force2D, 0, dense=False, route=_dense(force2D))


# ---- route 3: the int32 tile kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ng", [256, 300])
@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
@pytest.mark.parametrize("case", MULTI_TILE)
def test_int32_route_by_level_count(cm, checker, case, force2D, Ng):
    """Ng > 255 does not fit the packed bytes: glszm_tile_kernel + glszm_border_full_kernel<1|2> label the same volumes"""
    _check(cm, checker if Ng == 256 else None, BY_ID[case](), force2D, 0, Ng=Ng, route=_int32(force2D))


@pytest.mark.parametrize("Ng", [256, 300])
def test_int32_route_singles_at_the_level_count(cm, checker, Ng):
    """4096 zones in one tile and zones == voxels in many tiles, with levels up to Ng itself"""
    for vol in (singles((8, 8, 64), Ng), singles((17, 17, 130), Ng, 1)):
        assert vol.img.max() == Ng
        _check(cm, checker, vol, False, 0, route=_int32(False))
        _check(cm, checker, vol, True, 0, route=_int32(True))


@pytest.mark.parametrize("f2d", [1, 2])
@pytest.mark.parametrize("case", MULTI_TILE)
def test_int32_route_by_force2d_dimension(cm, checker, case, f2d):
    """force2Ddimension 1 and 2: four in-plane offsets that are not the x-y ones (mode 0, glszm_border_kernel)"""
    _check(cm, checker, BY_ID[case](), True, f2d, route="tiles-offsets")


@pytest.mark.parametrize("bad", [0, 9])
@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
@pytest.mark.parametrize("case", ["serp-17x9x130", "chk2-24x33x196", "corners-132", "combs-24x33x196"])
def test_int32_route_by_irregular_level(cm, checker, case, force2D, bad):
    """a masked level 0 or > Ng: the packed-byte attempt sets flags[0] and computes nothing, the second attempt labels on the
    int32 kernels.  The matrix cannot be filled (IndexError, as the C checker raises); the zones are all there, the
    irregular one included, in the reference's order -- and the next regular call is not disturbed."""
    base = BY_ID[case]()
    img = base.img.copy()
    at = (img.shape[0] // 2, TY, TX - 1)
    img[at] = bad
    vol = Vol(base.name + " level%d@%s" % (bad, at), img, base.mask, base.Ng, None, None)
    Ns = int(vol.mask.sum())
    with pytest.raises(IndexError):
        checker.calculate_glszm(vol.img, vol.mask, vol.Ng, Ns, force2D, 0)
    with pytest.raises(IndexError):
        cm.calculate_glszm(vol.img, vol.mask, vol.Ng, Ns, force2D, 0)
    assert _variant() == _int32(force2D), "the route after the retry"
    z = vol.zones(force2D, 0)
    assert ((z[:, 0] == bad) & (z[:, 1] == 1)).sum() == 1
    for again in range(2):
        got = _gpu_zone_list(Ns)
        assert np.array_equal(got, gr.zone_list(z)), "zone list (call %d) " % (again + 1) + _explain(vol, z, got)
    _check(cm, checker, base, force2D, 0, route=_dense(force2D))


def test_empty_mask(cm, checker):
    img = serpentine((17, 9, 130)).img
    mask = np.zeros(img.shape, bool)
    for force2D in (False, True):
        with pytest.raises(IndexError):                    # Ns = 0: 0 zones >= 2 Ns
            cm.calculate_glszm(img, mask, 2, 0, force2D, 0)
        with pytest.raises(IndexError):
            checker.calculate_glszm(img, mask, 2, 0, force2D, 0)
        got = cm.calculate_glszm(img, mask, 2, 1, force2D, 0)
        assert got.shape == (1, 2, 1) and not got.any()
        assert np.array_equal(got, checker.calculate_glszm(img, mask, 2, 1, force2D, 0))
        assert np.array_equal(_gpu_zone_list(4), [-1])
        P, s = cm.calculate_glszm_compact(img, mask, 2, 1, force2D, 0)
        assert len(s) == 0 and P.shape == (1, 2, 0)


@pytest.mark.parametrize("Ng", [255, 256])
def test_scratch_exhaustion_rule(cm, Ng):
    """segment mode fails with IndexError when zones >= 2 Ns.  Every voxel a zone, so the count is known exactly:
    zones = 2 Ns - 1 still answers (and answers right), zones = 2 Ns raises.  (Only the kernels and the scipy reference here:
    the C checkers size their zone list by Ns and may not be called with fewer entries than zones.)"""
    for force2D in (False, True):
        odd = singles((17, 17, 130), Ng, 1, drop=1 - (17 * 17 * 130) % 2)
        n = int(odd.mask.sum())
        assert n % 2 == 1
        Ns = (n + 1) // 2                                  # n == 2 Ns - 1
        D = cm.calculate_glszm(odd.img, odd.mask, Ng, Ns, force2D, 0)
        assert np.array_equal(D, gr.matrix(odd.zones(force2D, 0), Ng))
        even = singles((17, 17, 130), Ng, 1, drop=2 - (17 * 17 * 130) % 2)
        n = int(even.mask.sum())
        assert n % 2 == 0
        with pytest.raises(IndexError):                    # n == 2 Ns
            cm.calculate_glszm(even.img, even.mask, Ng, n // 2, force2D, 0)
        P, s = cm.calculate_glszm_compact(even.img, even.mask, Ng, n // 2 + 1, force2D, 0)     # n == 2 Ns - 2
        assert np.array_equal(s, [1]) and P.sum() == n


# ---- route 4: the label-volume kernels (4-D and 2-D input) ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 9, 66), (2, 8, 8, 64), (4, 3, 17, 65)])
def test_label_volume_route_4d(cm, checker, shape):
    """4-D input: glszm_init / merge / flatten_count under the 80-neighbourhood.  Checkerboards (each colour one zone), every
    voxel a zone (16 colours by coordinate parity), one level, and a stack of serpentines whose path and walls each fuse
    across the fourth axis"""
    for m in (2, 3):
        _check(cm, checker, checkerboard(shape, m), route="label-volume")
    idx = np.indices(shape)
    colour = sum((idx[d] & 1) << d for d in range(4))
    rng = np.random.default_rng(4)
    lvl = 1 + 16 * rng.integers(0, 15, size=shape) + colour
    cen = {}
    for g, c in enumerate(np.bincount(lvl.ravel())):
        _add(cen, g, 1, int(c))
    _check(cm, checker, Vol("singles4d%s" % (shape,), lvl, None, 240, cen), route="label-volume")
    _check(cm, checker, uniform(shape, 2, 2), route="label-volume")
    s3 = serpentine(shape[1:])
    n1 = sum(sz * c for (g, sz), c in s3.cen.items() if g == 1)
    cen = _add(_add({}, 1, shape[0] * n1), 2, shape[0] * (s3.img.size - n1))
    _check(cm, checker, Vol("serpentine4d%s" % (shape,), np.broadcast_to(s3.img, shape), None, 2, cen), route="label-volume")


@pytest.mark.parametrize("shape", [(17, 130), (64, 64), (9, 255), (130, 17)])
def test_2d_input(cm, checker, shape):
    """2-D arrays: a serpentine plane (path one zone, every wall row a zone), checkerboards (m = 3: every anti-diagonal a
    zone), combs, every pixel a zone"""
    Ny, Nx = shape
    plane, _, _, _, cen = serp_plane(Ny, Nx)
    _check(cm, checker, Vol("serp2d%s" % (shape,), plane, None, 2, cen), route="dense8")
    for m in (2, 3):
        c3 = checkerboard((1, Ny, Nx), m)
        _check(cm, checker, Vol("chk2d%s/%d" % (shape, m), c3.img[0], None, m, c3.cen2), route="dense8")
    c3 = combs((1, Ny, Nx))
    _check(cm, checker, Vol("combs2d%s" % (shape,), c3.img[0], None, 3, c3.cen), route="dense8")
    s3 = singles((1, Ny, Nx), 255, 2)
    _check(cm, checker, Vol("singles2d%s" % (shape,), s3.img[0], None, 255, s3.cen), route="dense8")


# ---- route 5: the lanes of glszm_pairs_kernel ------------------------------------------------------------------------------------
PGRID_CASES = ["serp-24x33x196", "serp-17x9x130", "chk2-24x33x196", "chk3-24x33x196", "helix-24x33x196", "combs-24x33x196",
               "tilechecker-24x33x196", "corners-132"]


def _pgrid_child():
    """runs in a fresh process with PRAD_GLSZM_PGRID set (the library reads it once): closed form and scipy only"""
    from pyradiomics_amd import cmatrices
    n = 0
    for case in PGRID_CASES:
        for force2D in (False, True):
            n += _check(cmatrices, None, BY_ID[case](), force2D, 0)
    vol = serpentine((64, 64, 256))        # one path of 528 k voxels through 256 tiles
    n += _check(cmatrices, None, vol, False, 0, dense=False)
    print("PGRID_CHILD_OK %d" % n)


@pytest.mark.parametrize("pgrid", [1, 2048])
def test_pairs_kernel_grid(pgrid):
    """PRAD_GLSZM_PGRID = 1: one workgroup's lanes make every union of a tree; 2048: as many lanes as the launch allows
    collide in the one tree of the serpentine / the checkerboard (atomicMin on stale roots, no path halving)"""
    env = dict(os.environ, PRAD_GLSZM_PGRID=str(pgrid))
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_glszm_topology as t; t._pgrid_child()" % (os.path.dirname(here), here)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "PGRID_CHILD_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- a volume of 256^3 and one of 512 x 256 x 256 through the compact API -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["serpentine", "checkerboard", "combs"])
def test_large_volume_compact(cm, kind):
    """>= 256^3: the dense matrix would not fit; (P, sizes), the zone count and the largest zone against scipy and the closed form"""
    shape = (256, 256, 256)
    vol = {"serpentine": serpentine, "checkerboard": checkerboard, "combs": combs}[kind].__wrapped__(shape)     # (not kept)
    Ns = vol.img.size
    P, s = cm.calculate_glszm_compact(vol.img, vol.mask, vol.Ng, Ns, False, 0)
    assert _variant() == "dense26"
    Pc, sc = gr.census_matrix(vol.cen, vol.Ng)
    assert np.array_equal(s, sc) and np.array_equal(P[0], Pc), "closed form"
    z = vol.zones()
    Pr, sr = gr.compact(z, vol.Ng)
    assert np.array_equal(s, sr) and np.array_equal(P[0], Pr), "scipy"
    assert int(P.sum()) == len(z) == sum(vol.cen.values()) and int(s[-1]) == max(sz for _, sz in vol.cen)
    P2, s2 = cm.calculate_glszm_compact(vol.img, vol.mask, vol.Ng, Ns, False, 0)
    assert np.array_equal(P2, P) and np.array_equal(s2, s)


# ---- route 6: zones, ranked sizes, compact matrix and formulas in one queue ----------------------------------------------------------
@pytest.mark.parametrize("case", ["serp-24x33x196", "serp-cut7", "singles-tile-Ng255", "singles-many-Ng255", "chk2-24x33x196",
                                  "chk3-24x33x196", "corners-132", "combs-24x33x196"])
@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
def test_one_queue_features(case, force2D):
    """engine.glszm_features against tests/feature_reference.py evaluated in long double on the REFERENCE matrix, within the
    bounds that module derives (zone_bounds; chain lengths c as test_gpu_segment_feature_limits.py derives them)"""
    import torch
    import feature_reference as fr
    from test_gpu_segment_feature_limits import c_zone_marginal, c_zone_entry
    from pyradiomics_amd import engine
    vol = BY_ID[case]()
    Pr, sr = gr.compact(vol.zones(force2D, 0), vol.Ng)
    ref = fr.zone_angle(Pr, sr)
    B = fr.zone_bounds(ref, c_zone_marginal(vol.Ng, len(sr)), c_zone_entry(vol.Ng, len(sr)))
    dev = torch.device("cuda", 0)
    L, M = torch.from_numpy(vol.img).to(dev), torch.from_numpy(vol.mask.view(np.uint8)).to(dev)
    Ns = int(vol.mask.sum())
    got, flag = engine.glszm_features(L, M, vol.Ng, Ns, force2D, 0)
    assert got[16] == 0 and flag[0] == 0
    assert _variant() == _dense(force2D)
    for k, n in enumerate(fr.ZONE_NAMES):
        want = float(ref["values"][n])
        print("%s %s err %.3g bound %.3g" % (vol.name, n, abs(got[k] - want), B[n]))
        assert abs(got[k] - want) <= B[n], (vol.name, n, got[k], want, B[n])
    d, dflag = engine.glszm_features(L, M, vol.Ng, Ns, force2D, 0, deferred=True)
    engine.deferred_status()
    assert np.array_equal(d, got) and dflag[0] == 0
    P, s = engine.glszm_compact(L, M, vol.Ng, Ns, force2D, 0)      # the three-call route right after, same workspace
    assert np.array_equal(s, sr) and np.array_equal(P.cpu().numpy(), Pr)


# ---- route 7: the level shards ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
@pytest.mark.parametrize("case", ["combs-24x33x196", "chk3-24x33x196", "chk3-17x9x130", "corners-131"])
def test_level_shards(case, force2D, world):
    """every rank labels the zones of its own levels (the others masked out: whole levels vanish from between the teeth of
    the combs); merged table == unsharded == reference.  One GPU plays every rank in turn."""
    import torch
    from pyradiomics_amd import batch, engine
    vol = BY_ID[case]()
    dev = torch.device("cuda", 0)
    L, M = torch.from_numpy(vol.img).to(dev), torch.from_numpy(vol.mask.view(np.uint8)).to(dev)
    Pr, sr = gr.compact(vol.zones(force2D, 0), vol.Ng)
    if world == 1:
        P, s = batch.segment_matrices_sharded(L, M, vol.Ng, classes=("glszm",), force2D=force2D, force2Ddimension=0)["glszm"]
    else:
        tables = [batch.segment_partials(L, M, vol.Ng, rank, world, classes=("glszm",), force2D=force2D,
                                         force2Ddimension=0)["glszm"] for rank in range(world)]
        P, s = batch.merge_zone_tables(tables, vol.Ng)
    assert np.array_equal(s, sr) and np.array_equal(np.asarray(P), Pr), "merged table against the reference"
    Pu, su = engine.glszm_compact(L, M, vol.Ng, None, force2D, 0)
    assert np.array_equal(su, s) and np.array_equal(Pu.cpu().numpy(), np.asarray(P)), "merged table against the unsharded call"


# ---- route 8: voxel mode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["whole", "masked"])
@pytest.mark.parametrize("force2D", [False, True], ids=["3d", "2d0"])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("case", ["chk2-17x17x64", "chk3-24x33x196", "serp-24x33x196", "serp-17x9x130", "combs-24x33x196"])
def test_voxel_mode_on_tile_corners(cm, checker, case, radius, force2D, masked):
    """glszm_voxel_kernel (a flood fill per kernel and lane): kernels centred on the eight voxels around a tile corner, on the
    volume's own corners and on a few voxels between, against the checker's voxel mode"""
    vol = BY_ID[case]()
    Nz, Ny, Nx = vol.img.shape
    mask = vol.mask
    if masked:
        mask = mask & (np.random.default_rng(radius).random(vol.img.shape) < 0.8)
    cz, cy, cx = TZ, TY, TX if Nx > TX else TX // 2
    centres = [(cz - 1 + a, cy - 1 + b, cx - 1 + c) for a in range(2) for b in range(2) for c in range(2)]
    centres += [(0, 0, 0), (Nz - 1, Ny - 1, Nx - 1), (0, Ny - 1, 0), (Nz // 2, Ny // 2, Nx // 2), (cz, cy - 3, cx + 2)]
    vox = np.array(centres, dtype=np.intc).T.copy()
    Ns = int(mask.sum())
    want = checker.calculate_glszm(vol.img, mask, vol.Ng, Ns, force2D, 0, kernelRadius=radius, voxels=vox)
    got = cm.calculate_glszm(vol.img, mask, vol.Ng, Ns, force2D, 0, kernelRadius=radius, voxels=vox)
    assert _variant() == "voxel-flood"
    assert got.shape == want.shape and np.array_equal(got, want), (vol.name, radius, force2D, masked)
    # and the independent reference on the crop of every kernel
    for v, (z, y, x) in enumerate(centres):
        lo = [z if force2D else max(z - radius, 0), max(y - radius, 0), max(x - radius, 0)]
        hi = [z if force2D else min(z + radius, Nz - 1), min(y + radius, Ny - 1), min(x + radius, Nx - 1)]
        sl = tuple(slice(a, b + 1) for a, b in zip(lo, hi))
        zz = gr.zones(vol.img[sl], mask[sl], force2D, 0)
        one = gr.matrix(zz, vol.Ng)[0]
        assert np.array_equal(got[v][:, :one.shape[1]], one) and not got[v][:, one.shape[1]:].any(), (vol.name, centres[v])

"""Many small ROIs in a few launches: the device-tensor API of the batch route (csrc/prad_batch*.hip, their shared host layer
csrc/prad_batch_common.h).  A public function turns its arguments into ONE RoiBatch -- flat buffers holding the boxes back to
back, their sizes and offsets, the library following the tensors' device -- and hands it to the internal function of the same
name with a leading underscore; internal functions call internal functions, so nothing is normalised or checked twice.  ROIs
outside a native call's domain go through the single calls of pyradiomics_amd.engine, which re-exports the public names."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import cmatrices as _cm
from .cmatrices import _iptr

FEATURE_FAMILIES = ("glcm", "glrlm", "gldm", "ngtdm", "glszm")       # bit f of the C `families` argument, row f of its offsets
ROI_FEATURE_CLASSES = ("firstorder", "glcm", "glrlm", "glszm", "gldm", "ngtdm")
_FEATURE_ROW = {"glcm": 24, "glrlm": 16, "gldm": 16, "ngtdm": 5, "glszm": 16}
_NP_DTYPES = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int16: np.int16}


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _offsets(counts):
    """int64 [B]: where each of B pieces of `counts` elements starts when they lie back to back"""
    off = np.zeros(len(counts), dtype=np.int64)
    off[1:] = np.cumsum(counts)[:-1]
    return off


def _set_device(lib, dev):
    """the library context is per thread: follow the tensors' device"""
    _lib.raise_for(lib.prad_set_device(dev.index if dev.index is not None else torch.cuda.current_device()), "set_device")


last_batch_route = _cm.last_batch_route


def _route(single, total):
    """how many of `total` ROIs went through the single calls -> the route's name"""
    return "batch" if not single else ("looped" if single == total else "mixed")


def _joined_route(routes):
    return routes[0] if all(r == routes[0] for r in routes) else "mixed"


class RoiBatch(NamedTuple):
    """B boxes back to back in flat device buffers, as every batched call takes them"""
    lib: object
    data: torch.Tensor       # levels (int32) or raw intensities (float32, float64, int32, int16)
    mask: torch.Tensor       # uint8, non-zero = ROI
    sizes: np.ndarray        # intc [B, 3]
    nvox: np.ndarray         # int64 [B]
    off: np.ndarray          # int64 [B]: first element of every box
    device: torch.device

    @property
    def B(self):
        return int(self.sizes.shape[0])

    def view(self, flat, b):
        """box b of a flat buffer in the batch layout, in its 3-D shape"""
        return flat[int(self.off[b]):int(self.off[b] + self.nvox[b])].view(tuple(int(s) for s in self.sizes[b]))

    def boxes(self, idx):
        """(image, mask) of the ROIs idx, for the single calls"""
        return ((self.view(self.data, b), self.view(self.mask, b)) for b in idx)

    def to_device(self, array):
        """a numpy result of the looped routes, put where the native route's results are"""
        return torch.from_numpy(array).to(self.device)

    def with_data(self, data):
        """the same masks and geometry over another flat buffer"""
        return self._replace(data=data)

    def subset(self, idx):
        """a batch of the ROIs `idx` alone, packed again (the batch itself where idx names every ROI in order)"""
        if len(idx) == self.B and np.array_equal(idx, np.arange(self.B)):
            return self
        sizes, nvox = np.ascontiguousarray(self.sizes[idx]), self.nvox[idx]
        pick = lambda flat: torch.cat([flat[int(self.off[b]):int(self.off[b] + self.nvox[b])] for b in idx])
        return self._replace(data=pick(self.data), mask=pick(self.mask), sizes=sizes, nvox=nvox, off=_offsets(nvox))


def _roi_batch(data, masks, sizes, raw=False) -> RoiBatch:
    """levels / masks as the public functions take them: lists of 3-D device tensors (`sizes` is then ignored), or flat device
    tensors plus sizes int [B, 3].  raw: intensity images instead of levels; they keep their dtype where it is one of the four the
    kernels read (float32, float64, int32, int16; anything else, or a list of mixed dtypes, becomes float64)"""
    def image_dtype(dts):
        if not raw:
            return torch.int32
        return dts[0] if dts[0] in _eng._DTYPE_CODES and all(d == dts[0] for d in dts) else torch.float64
    if isinstance(data, (list, tuple)):
        if len(data) != len(masks):
            raise ValueError("levels and masks differ in number")
        if any(l.dim() != 3 or l.shape != m.shape for l, m in zip(data, masks)):
            raise ValueError("the batched matrices take 3-D ROIs with masks of the same shape")
        sizes = np.array([tuple(l.shape) for l in data], dtype=np.intc).reshape(-1, 3)
        if not len(data):
            raise ValueError("empty batch")
        dt = image_dtype([l.dtype for l in data])
        data = torch.cat([l.reshape(-1).to(dt) for l in data])
        masks = torch.cat([(m if m.dtype in (torch.bool, torch.uint8) else m != 0).reshape(-1).view(torch.uint8) for m in masks])
    elif sizes is None:
        raise ValueError("flat level / mask tensors need `sizes`")
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    data, masks = data.reshape(-1), masks.reshape(-1)
    if not data.is_cuda or not masks.is_cuda:
        raise ValueError("engine.* expects CUDA/HIP tensors; use pyradiomics_amd.cmatrices for numpy input")
    data, masks = data.to(image_dtype([data.dtype])).contiguous(), _eng._mask_u8(masks)
    if data.shape != masks.shape:
        raise ValueError("Dimensions of image and mask do not match.")
    lib = _lib.load()
    _set_device(lib, data.device)
    nvox = sizes.astype(np.int64).prod(1)
    if int(nvox.sum()) != data.numel():
        raise ValueError("sizes describe %d voxels, the buffers hold %d" % (int(nvox.sum()), data.numel()))
    return RoiBatch(lib, data, masks, sizes, nvox, _offsets(nvox), data.device)


# ---- GLCM / GLRLM / GLDM / NGTDM (prad_calculate_batch_dev, csrc/kernels_batch.h) --------------------------------------------
def batch_max_vox() -> int:
    """voxels of the largest ROI box the batched call takes (PRAD_BATCH_MAX_VOX)"""
    return int(_lib.load().prad_batch_max_vox())


class Planar(NamedTuple):
    """the settings the batched route shares with the single calls and the feature classes beyond its own arguments"""
    force2D: bool = False
    force2Ddimension: int = 0
    weightingNorm: Optional[str] = None
    spacing: object = (1.0, 1.0, 1.0)          # (z, y, x): one triple, or float [B, 3]; used only for the weights
    symmetric: bool = True                     # symmetricalGLCM, for the merge

    @property
    def f2d(self):
        return _cm.batch_forced_dim(self.force2D, self.force2Ddimension)

    @property
    def axes(self):
        """(force2D, force2Ddimension) as the single calls take them"""
        return bool(self.force2D), int(self.force2Ddimension)

    def subset(self, idx, B):
        return self._replace(spacing=_cm.batch_spacing(self.spacing, B)[idx])


def _planar(force2D, force2Ddimension, weightingNorm, spacing, symmetric=True):
    p = Planar(bool(force2D), int(force2Ddimension), _cm.batch_weighting_norm(weightingNorm), spacing, bool(symmetric))
    p.f2d          # (raises on a dimension outside 0 .. 2)
    return p


def _merge_flat(rois, Ng, families, dist, flat, status, plan, pl):
    """the weighted angle merge of the flat per-angle buffers (prad_batch_merge_angles_dev) -> ({"glcm_w" / "glrlm_w": flat
    float64 device buffer}, merge offsets int64 [3, B + 1])"""
    fams = tuple(f for f in _cm.MERGE_FAMILIES if f in families)
    _, offsets, Na = plan
    moff = _cm.batch_merge_plan(rois.sizes, Ng, Na, fams)
    w = _cm.batch_weights(rois.sizes, Na, dist, pl.weightingNorm, pl.spacing, *pl.axes)
    out = {f: torch.empty(int(moff[_cm.MERGE_FAMILIES.index(f), rois.B]), dtype=torch.float64, device=rois.device) for f in fams}
    merge, ng = _cm.batch_levels_call(rois.lib, "prad_batch_merge_angles_dev", Ng)
    rc = merge(_iptr(rois.sizes), rois.B, ng, sum(1 << _cm.MERGE_FAMILIES.index(f) for f in fams), _iptr(Na),
               _vp(flat.get("glcm")), _vp(flat.get("glrlm")), _lp(offsets), w.ctypes.data_as(C.POINTER(C.c_double)), _vp(status),
               1 if pl.symmetric else 0, _vp(out.get("glcm")), _vp(out.get("glrlm")), _eng._stream_ptr())
    _lib.raise_for(rc, "batched angle merge")
    return {f + "_w": out[f] for f in fams}, moff


def _matrices_flat(rois, Ng, families, dist, gldm_a, plan=None, pl=Planar()):
    plan = plan if plan is not None else _cm.batch_plan(rois.sizes, Ng, families, dist, *pl.axes)
    covered, offsets, _ = plan
    if not covered:
        return None
    B, dist = rois.B, np.ascontiguousarray(np.asarray(dist, dtype=np.intc).ravel())
    flat = {f: torch.empty(int(offsets[_cm.BATCH_FAMILIES.index(f), B]), dtype=torch.float64, device=rois.device) for f in families}
    status = torch.empty(B, dtype=torch.int32, device=rois.device)
    ptr = [_vp(flat.get(f)) for f in _cm.BATCH_FAMILIES]
    calculate, ng = _cm.batch_levels_call(rois.lib, "prad_calculate_batch_f2d_dev", Ng)
    rc = calculate(_vp(rois.data), _vp(rois.mask), _iptr(rois.sizes), _lp(rois.off), B, ng, _cm.batch_family_bits(families),
                   _iptr(dist), int(dist.shape[0]), int(gldm_a), pl.f2d, ptr[0], ptr[1], ptr[2], ptr[3], _vp(status),
                   _eng._stream_ptr())
    if rc == _lib.PRAD_E_UNSUPPORTED:
        return None
    _lib.raise_for(rc, "batched texture matrices")
    if pl.weightingNorm is not None and any(f in families for f in _cm.MERGE_FAMILIES):
        flat.update(_merge_flat(rois, Ng, families, dist, flat, status, plan, pl)[0])
    _cm._set_batch_route("batch")
    return flat, status.tolist()


def texture_matrices_batch_flat(levels, masks, sizes, Ng, families=_cm.BATCH_FAMILIES, distances=(1,), gldm_a=0, force2D=False,
                                force2Ddimension=0, weightingNorm=None, spacing=(1.0, 1.0, 1.0), symmetricalGLCM=True):
    """the native calls alone: -> ({family: flat float64 device buffer}, status list), or None when they decline the batch.
    force2D / force2Ddimension / weightingNorm / spacing / symmetricalGLCM as texture_matrices_batch: with weightingNorm the
    dict also holds the flat merged buffers "glcm_w" / "glrlm_w" (cmatrices.batch_merge_plan lays them out).  Ng: an int, or an
    int sequence [B] (cmatrices.batch_plan lays the buffers out with every ROI's own count); no partition happens here: one count
    above 64 declines the batch."""
    rois = _roi_batch(levels, masks, sizes)
    return _matrices_flat(rois, _cm.batch_levels(Ng, rois.B), tuple(families), list(distances), gldm_a,
                          pl=_planar(force2D, force2Ddimension, weightingNorm, spacing, symmetricalGLCM))


def _matrices_native(rois, Ng, families, dist, gldm_a, pl, merged):
    """the native calls on the whole batch -> ({family: [B views into the flat buffers]}, status), or None when they decline"""
    plan = _cm.batch_plan(rois.sizes, Ng, families, dist, *pl.axes)
    res = _matrices_flat(rois, Ng, families, dist, gldm_a, plan, pl)
    if res is None:
        return None
    shapes = _cm.batch_shapes(rois.sizes, Ng, plan[2])
    flat, status = res
    mats = {}
    for f in families:
        o = plan[1][_cm.BATCH_FAMILIES.index(f)]
        mats[f] = [flat[f][int(o[b]):int(o[b + 1])].view(shapes[f][b]) for b in range(rois.B)]
    if merged:
        moff = _cm.batch_merge_plan(rois.sizes, Ng, plan[2], merged)
        for f in merged:
            o = moff[_cm.MERGE_FAMILIES.index(f)]
            mats[f + "_w"] = [flat[f + "_w"][int(o[b]):int(o[b + 1])].view(shapes[f][b][:2] + (1,)) for b in range(rois.B)]
    return mats, status


def _matrices_looped(rois, Ng, families, dist, gldm_a, pl, merged):
    """the single calls, ROI by ROI, on a batch of ONE count Ng"""
    Na = _cm.batch_plan(rois.sizes, Ng, families, dist, *pl.axes)[2]
    shapes = _cm.batch_shapes(rois.sizes, Ng, Na)
    f2 = pl.axes
    single = {"glcm": lambda i, m: _eng.glcm(i, m, Ng, dist, *f2)[0],
              "glrlm": lambda i, m: _eng.glcm_glrlm(i, m, Ng, max(i.shape), *f2, want_glcm=False)[1],
              "gldm": lambda i, m: _eng.gldm(i, m, Ng, int(gldm_a), dist, *f2),
              "ngtdm": lambda i, m: _eng.ngtdm(i, m, Ng, dist, *f2)}
    mats, status = _cm._looped_matrices(rois.boxes(range(rois.B)), Ng, families, shapes, single, rois.to_device)
    if merged:
        _cm.merge_looped(mats, rois.sizes, Na, dist, pl.weightingNorm, pl.spacing, *f2, pl.symmetric, rois.to_device)
    return mats, status


def _matrices(rois, Ng, families, distances, gldm_a, pl=Planar()):
    dist = [int(d) for d in distances]
    merged = [f for f in _cm.MERGE_FAMILIES if f in families] if pl.weightingNorm is not None else []
    B = rois.B
    if not isinstance(Ng, np.ndarray):          # one count: the whole batch goes one way
        return (_matrices_native(rois, Ng, families, dist, gldm_a, pl, merged)
                or _matrices_looped(rois, Ng, families, dist, gldm_a, pl, merged))
    # a count per ROI: the ROIs inside the native domain share ONE call, each of the others takes the single calls
    Na = _cm.batch_plan(rois.sizes, Ng, families, dist, *pl.axes)[2]
    inside = np.flatnonzero((Ng <= _cm.BATCH_MAX_NG) & (rois.nvox <= batch_max_vox()) & (Na[0] <= 127))
    keys = list(families) + [f + "_w" for f in merged]
    mats, status = {k: [None] * B for k in keys}, [_lib.PRAD_OK] * B
    res = None
    if len(inside):
        res = _matrices_native(rois.subset(inside), np.ascontiguousarray(Ng[inside]), families, dist, gldm_a,
                               pl.subset(inside, B), merged)
    if res is None:
        inside = inside[:0]
    for k, b in enumerate(inside):
        status[b] = res[1][k]
        for key in keys:
            mats[key][b] = res[0][key][k]
    rest = np.setdiff1d(np.arange(B), inside)
    for b in rest:
        one, st = _matrices_looped(rois.subset(np.array([b])), int(Ng[b]), families, dist, gldm_a, pl.subset(np.array([b]), B), merged)
        status[b] = st[0]
        for key in keys:
            mats[key][b] = one[key][0]
    _cm._set_batch_route(_route(len(rest), B))
    return mats, status


def texture_matrices_batch(levels, masks, sizes, Ng, families=_cm.BATCH_FAMILIES, distances=(1,), gldm_a=0, force2D=False,
                           force2Ddimension=0, weightingNorm=None, spacing=(1.0, 1.0, 1.0), symmetricalGLCM=True):
    """GLCM / GLRLM / GLDM / NGTDM of B small ROIs in ONE launch (segment mode).  levels / masks: lists of 3-D device
    tensors (concatenated here; `sizes` is then ignored), or flat device tensors holding the ROIs back to back plus `sizes`
    (int [B, 3]).  -> ({family: [B float64 device tensors, views into one flat buffer, in the single calls' layouts:
    glcm [Ng, Ng, Na], glrlm [Ng, max(size), Na1], gldm [Ng, 2 * Nb + 1] with Nb = 2 * Na, ngtdm [Ng, 3]]}, status [B]: 1,
    or 0 for a ROI with a masked level outside [1, Ng] -- the single calls' IndexError; its matrices are void).
    Covered: Ng <= 64, boxes of at most batch_max_vox() voxels, at most 127 angles; otherwise the single calls are looped ROI
    by ROI (same results, separate tensors) and last_batch_route() says "looped".  GLSZM: glszm_batch.
    force2D / force2Ddimension: the angle sets of the single calls with the same arguments -- no angle leaves the plane across
    axis force2Ddimension (0 z, 1 y, 2 x).  A ROI that keeps no angle (5 x 1 x 1 with dimension 0, 1 x 1 x 1 always) is legal:
    empty GLCM / GLRLM, GLDM and NGTDM of voxels without neighbours.
    weightingNorm ("euclidean", "manhattan", "infinity", "no_weighting"; anything else: ValueError) adds, in one more launch, the
    entries "glcm_w" [Ng, Ng, 1] and "glrlm_w" [Ng, max(size), 1]: the per-angle matrices -- GLCM plus its transpose when
    symmetricalGLCM -- summed over the angles with the weights glcm._weights gives the feature classes for the ROI's angles and
    `spacing` ((z, y, x): one triple or float [B, 3]; used for nothing else).  The sum adds rounded products over the angles
    ascending (csrc/kernels_batch_merge.h), on every route; a ROI without angles or with status 0 gets zeros.
    Ng: an int as above, or an int sequence [B]: ROI b has Ng[b] levels -- its matrices have Ng[b] rows, its masked levels must
    lie in [1, Ng[b]] -- as a fixed bin width gives a table of lesions.  The ROIs of at most 64 levels inside the box caps then
    share ONE native call, each of the others takes the single calls with its own count, and last_batch_route() says "batch",
    "mixed" or "looped"."""
    rois = _roi_batch(levels, masks, sizes)
    return _matrices(rois, _cm.batch_levels(Ng, rois.B), tuple(families), distances, gldm_a,
                     _planar(force2D, force2Ddimension, weightingNorm, spacing, symmetricalGLCM))


# ---- GLSZM (prad_batch_glszm_dev / prad_batch_glszm_fill_dev, csrc/kernels_batch_glszm.h) ------------------------------------
def batch_glszm_max_vox() -> int:
    """voxels of the largest ROI box the batched GLSZM takes (PRAD_BATCH_GLSZM_MAX_VOX)"""
    return int(_lib.load().prad_batch_glszm_max_vox())


def _glszm_label(rois, sizes, off, Ng, f2d=-1):
    """the labelling launch on the ROIs (sizes[b], off[b]) of the batch's buffers -> (zones int32 device buffer indexed by
    2 * off[b], summary int32 numpy [B, 3], status int32 numpy [B]); summary and status come back in ONE copy"""
    B = int(sizes.shape[0])
    zones = torch.empty(2 * rois.data.numel(), dtype=torch.int32, device=rois.device)
    meta = torch.empty(4 * B, dtype=torch.int32, device=rois.device)
    label, ng = _cm.batch_levels_call(rois.lib, "prad_batch_glszm_f2d_dev", Ng)
    rc = label(_vp(rois.data), _vp(rois.mask), _iptr(sizes), _lp(off), B, ng, int(f2d), _vp(zones), _vp(meta),
               C.c_void_p(meta.data_ptr() + 12 * B), _eng._stream_ptr())
    _lib.raise_for(rc, "batched GLSZM")
    host = meta.cpu().numpy()
    return zones, np.ascontiguousarray(host[:3 * B].reshape(B, 3)), host[3 * B:].copy()


class GlszmFlat(NamedTuple):
    """the device buffers the native route's results of glszm_batch are views of"""
    P: torch.Tensor                      # float64: the matrices of the covered ROIs back to back
    covered: np.ndarray                  # indices of those ROIs in the batch
    out_off: np.ndarray                  # int64 [covered]: first double of each matrix
    cols: np.ndarray                     # int64 [covered]: columns of each matrix
    sizes: Optional[torch.Tensor]        # int32: the zone sizes of the compact matrices' columns back to back; None: dense
    s_off: np.ndarray                    # int64 [covered]: first size of each list, -1 without a zone (one zero column)


class _GlszmBatch(list):
    """the result list of glszm_batch; `flat` (a GlszmFlat, or None) describes the buffers of the native route"""
    flat = None


def glszm_batch_zones(levels, masks, sizes, Ng, force2D=False, force2Ddimension=0, weightingNorm=None, spacing=(1.0, 1.0, 1.0)):
    """the zone lists of B small ROIs from the labelling launch alone -> (list of B int32 device tensors [nzones, 2] of
    (level, size) in raster order of each zone's first voxel -- views into one buffer --, summary int32 numpy [B, 3]: zones,
    largest zone, distinct sizes; status int32 numpy [B]).  Raises NotImplementedError outside the native domain (Ng > 64, a box
    above batch_glszm_max_vox() voxels).  force2D / force2Ddimension: as glszm_batch; weightingNorm / spacing are ignored.  Ng: an
    int, or an int sequence [B] (every ROI's levels are checked against its own count)."""
    rois = _roi_batch(levels, masks, sizes)
    pl = _planar(force2D, force2Ddimension, weightingNorm, spacing)
    zones, summary, status = _glszm_label(rois, rois.sizes, rois.off, _cm.batch_levels(Ng, rois.B), pl.f2d)
    _cm._set_batch_route("batch")
    return [zones[2 * int(o):2 * int(o) + 2 * int(n)].view(-1, 2) for o, n in zip(rois.off, summary[:, 0])], summary, status


def _glszm(rois, Ng, compact, pl=Planar()):
    B, dev = rois.B, rois.device
    ngv = _cm.batch_levels_vector(Ng, B)          # (the counts ROI by ROI, whichever form Ng has)
    covered = np.flatnonzero((rois.nvox <= batch_glszm_max_vox()) & (ngv <= _cm.BATCH_MAX_NG))
    results, status = _GlszmBatch([None] * B), [_lib.PRAD_OK] * B
    if len(covered):
        coff = np.ascontiguousarray(rois.off[covered])
        cng = np.ascontiguousarray(ngv[covered]) if isinstance(Ng, np.ndarray) else Ng
        zones, summary, st = _glszm_label(rois, np.ascontiguousarray(rois.sizes[covered]), coff, cng, pl.f2d)
        cols = np.maximum(summary[:, 2 if compact else 1], 1).astype(np.int64)
        k = summary[:, 2].astype(np.int64)
        out_off = np.append(np.int64(0), np.cumsum(ngv[covered].astype(np.int64) * cols))
        s_off = np.append(np.int64(0), np.cumsum(k))
        flat = torch.empty(int(out_off[-1]), dtype=torch.float64, device=dev)
        sizes_dev = torch.empty(max(int(s_off[-1]), 1), dtype=torch.int32, device=dev)
        fill, ng = _cm.batch_levels_call(rois.lib, "prad_batch_glszm_fill_dev", cng)
        rc = fill(_vp(zones), _iptr(summary), _lp(coff), len(covered), ng, 1 if compact else 0, _vp(flat), _lp(out_off),
                  _vp(sizes_dev), _lp(s_off), _eng._stream_ptr())
        _lib.raise_for(rc, "batched GLSZM fill")
        sizes_host = sizes_dev.cpu().numpy() if compact else None
        for i, b in enumerate(covered):
            P = flat[int(out_off[i]):int(out_off[i + 1])].view(int(ngv[b]), int(cols[i]))
            results[b] = (P[:, :int(k[i])], sizes_host[s_off[i]:s_off[i + 1]].copy()) if compact else P
            status[b] = int(st[i])
        # (batch_features_per_angle evaluates the formulas on these buffers, in place)
        results.flat = GlszmFlat(flat, covered, out_off[:-1], cols, sizes_dev if compact else None, np.where(k > 0, s_off[:-1], -1))
    rest = sorted(set(range(B)) - set(int(b) for b in covered))
    for b in rest:
        ng = int(ngv[b])
        single = lambda i, m, Ns: _eng.glszm_compact(i, m, ng, Ns, *pl.axes) if compact else _eng.glszm(i, m, ng, Ns, *pl.axes)
        one, st = _cm._looped_glszm(rois.boxes([b]), ng, compact, single, rois.to_device, pl.f2d)
        results[b], status[b] = one[0], st[0]
    _cm._set_batch_route("looped" if not len(covered) else _route(len(rest), B))
    return results, status


def glszm_batch(levels, masks, sizes, Ng, compact=True, force2D=False, force2Ddimension=0, weightingNorm=None,
                spacing=(1.0, 1.0, 1.0)):
    """GLSZM of B small ROIs in two launches (segment mode; the full neighbourhood, or with force2D the 8 neighbours in the plane
    across axis force2Ddimension, as the single calls; weightingNorm / spacing are accepted and ignored, as the class ignores
    them): zones labelled in LDS by one workgroup
    per ROI, one read-back of the per-ROI summary, one fill.  Inputs as texture_matrices_batch.  -> (list of B results, status
    [B]: 1, or 0 for a ROI with a masked level outside [1, Ng] -- the single call's IndexError; its result is that of an empty
    mask).  compact=True: a result is (P float64 [Ng, k] device tensor, sizes int32 numpy [k] ascending) as glszm_compact
    returns; compact=False: the dense [Ng, max(maxRegion, 1)] tensor as glszm returns.  The results of the native route are
    views into one flat buffer.  ROIs above batch_glszm_max_vox() voxels, or every ROI when Ng > 64, go through glszm_compact /
    glszm one by one (Ns = max(1, masked voxels)); last_batch_route() says "batch", "mixed" or "looped".  Ng: an int, or an int
    sequence [B]: ROI b has Ng[b] levels and a matrix of Ng[b] rows; the ROIs above 64 levels go one by one, the others share the
    two launches."""
    rois = _roi_batch(levels, masks, sizes)
    return _glszm(rois, _cm.batch_levels(Ng, rois.B), compact, _planar(force2D, force2Ddimension, weightingNorm, spacing))


# ---- feature formulas (prad_batch_features_dev, csrc/kernels_batch_features.h) -----------------------------------------------
def _flat_offsets(tensors):
    """element offsets of the tensors in the ONE storage they all are contiguous views of (-> base pointer, int64 offsets),
    or None when they are separate tensors (the looped routes' results)"""
    if not tensors:
        return None
    base = tensors[0].untyped_storage().data_ptr()
    if any((not t.is_cuda) or t.dtype != torch.float64 or not t.is_contiguous() or t.untyped_storage().data_ptr() != base
           for t in tensors):
        return None
    return base, np.array([t.storage_offset() for t in tensors], dtype=np.int64)


def _single_glszm_features(item, Ng):
    """the single call on one glszm_batch result (compact pair or dense tensor); a ROI without zones is an empty matrix"""
    P, jv = item if isinstance(item, tuple) else (item, np.arange(1, item.shape[1] + 1))
    if P.shape[1] == 0:
        return np.full((1, 16), np.nan), np.ones(1, dtype=bool)
    return _eng.zone_matrix_features(P, jv)


def _single_features(f, M, symmetric, mcc):
    """family f of one ROI through the single calls -> (float64 [rows, nfeat], bool [rows])"""
    if f == "ngtdm":
        return _eng.ngtdm_features(M).reshape(1, 5).copy(), np.array([not bool((M[:, 0] > 0).any().item())])
    if f == "glcm":
        Na = int(M.shape[2])
        vals, empty = (_eng.glcm_features(M, symmetric) if Na else (np.empty((0, 23)), np.zeros(0, dtype=bool)))
        last = _eng.glcm_mcc(M, symmetric) if (mcc and Na) else np.full(Na, np.nan)
        return np.concatenate([vals, last.reshape(Na, 1)], axis=1), empty
    if M.dim() == 3 and M.shape[2] == 0:
        return np.empty((0, 16)), np.zeros(0, dtype=bool)
    return _eng.zone_matrix_features(M, np.arange(1, M.shape[1] + 1))


def batch_features_per_angle(mats, Ng, glszm=None, symmetric=True, mcc=True):
    """The feature formulas on the matrices of a batch: `mats` is the dict of texture_matrices_batch, `glszm` the result list of
    glszm_batch (compact or dense) or None.  -> {family: [B pairs (float64 numpy [rows, nfeat], bool numpy [rows] = matrix
    empty)]}, rows = angles for glcm (24 columns: the 23 of glcm_features, then glcm_mcc; NaN without `mcc`) and glrlm (16),
    one row for gldm (16), ngtdm (5; its flag says that no level occurs) and glszm (16): the arrays the single calls return,
    bit for bit.  Matrices that are views of the flat buffers of the batched calls are evaluated in two launches
    (prad_batch_features_dev: Ng <= 64); anything else goes through the single calls, one by one.  Ng: an int, or an int
    sequence [B] -- the counts the matrices were built with; the ROIs of at most 64 levels then share the two launches and a ROI
    above has no MCC (NaN), as glcm_mcc declines it."""
    lib = _lib.load()
    fams = [f for f in FEATURE_FAMILIES[:4] if f in mats]
    B = len(mats[fams[0]]) if fams else len(glszm or [])
    if any(len(mats[f]) != B for f in fams) or (glszm is not None and len(glszm) != B):
        raise ValueError("the families differ in their number of ROIs")
    Ng = _cm.batch_levels(Ng, B)
    if isinstance(Ng, np.ndarray) and (Ng > _cm.BATCH_MAX_NG).any():
        # the ROIs the launches take, as a batch of their own; each of the others through the single calls
        out = {f: [None] * B for f in fams + (["glszm"] if glszm is not None else [])}
        small = np.flatnonzero(Ng <= _cm.BATCH_MAX_NG)
        if len(small):
            zsub = None
            if glszm is not None:
                zsub = _GlszmBatch(glszm[b] for b in small)
                zf = getattr(glszm, "flat", None)
                if zf is not None:          # (its ROIs all have at most 64 levels: _glszm)
                    zsub.flat = zf._replace(covered=np.searchsorted(small, zf.covered))
            sub = batch_features_per_angle({f: [mats[f][b] for b in small] for f in fams}, np.ascontiguousarray(Ng[small]), zsub,
                                           symmetric, mcc)
            for f in out:
                for k, b in enumerate(small):
                    out[f][b] = sub[f][k]
        for b in np.flatnonzero(Ng > _cm.BATCH_MAX_NG):
            for f in out:
                out[f][b] = _single_glszm_features(glszm[b], int(Ng[b])) if f == "glszm" else _single_features(f, mats[f][b], symmetric, False)
        return out
    out = {f: [None] * B for f in fams}
    if glszm is not None:
        out["glszm"] = [None] * B
    small = isinstance(Ng, np.ndarray) or Ng <= _cm.BATCH_MAX_NG
    views = {f: _flat_offsets(list(mats[f])) for f in fams} if small else {f: None for f in fams}
    zflat = getattr(glszm, "flat", None) if (glszm is not None and small) else None
    native = [f for f in fams if views[f] is not None]
    if (native or zflat is not None) and B:
        dev = (mats[native[0]][0] if native else zflat.P).device
        _set_device(lib, dev)
        # the angle counts and the longest axis as the matrices' shapes give them (the C call takes them as prad_batch_plan does)
        Na = np.zeros((2, B), dtype=np.intc)
        sizes = np.ones((B, 3), dtype=np.intc)
        for b in range(B):
            if "glcm" in native:
                Na[0, b] = mats["glcm"][b].shape[2]
            elif "gldm" in native:
                Na[0, b] = (mats["gldm"][b].shape[1] - 1) // 4
            if "glrlm" in native:
                sizes[b, 0], Na[1, b] = mats["glrlm"][b].shape[1], mats["glrlm"][b].shape[2]
        offsets = np.zeros((4, B + 1), dtype=np.int64)
        ptrs = [None] * 4
        bits = 0
        for f in native:
            i = FEATURE_FAMILIES.index(f)
            ptrs[i], offsets[i, :B] = C.c_void_p(views[f][0]), views[f][1]
            bits |= 1 << i
        cols = np.zeros(B, dtype=np.intc)
        zoff, soff = np.zeros(B, dtype=np.int64), np.full(B, -1, dtype=np.int64)
        zptr = sptr = None
        if zflat is not None:
            bits |= 16
            cols[zflat.covered] = zflat.cols
            zoff[zflat.covered] = zflat.out_off
            zptr, sptr = _vp(zflat.P), _vp(zflat.sizes)
            if zflat.sizes is not None:
                soff[zflat.covered] = zflat.s_off
        lay = np.zeros((2, 5, B + 1), dtype=np.int64)
        nrec = np.zeros(3, dtype=np.int64)
        plan, ng = _cm.batch_levels_call(lib, "prad_batch_features_plan", Ng)
        rc = plan(_iptr(sizes), B, ng, bits, _iptr(Na), _iptr(cols), _lp(lay), _lp(nrec))
        _lib.raise_for(rc, "batched features plan")
        nout, nrows = int(lay[0, 4, B]), int(lay[1, 4, B])
        # values and flags in one device block: one read-back
        block = torch.empty(nout + (nrows + 1) // 2 + 1, dtype=torch.float64, device=dev)
        flags = block[nout:].view(torch.int32)
        features, ng = _cm.batch_levels_call(lib, "prad_batch_features_dev", Ng)
        rc = features(_iptr(sizes), B, ng, bits, _iptr(Na), _iptr(cols), ptrs[0], ptrs[1], ptrs[2], ptrs[3], _lp(offsets), zptr,
                      _lp(zoff), sptr, _lp(soff), 1 if symmetric else 0, 1 if mcc else 0, _vp(block), _vp(flags),
                      _eng._stream_ptr())
        _lib.raise_for(rc, "batched features")
        host = block.cpu().numpy()
        vals, empty = host[:nout], host[nout:].view(np.int32)[:nrows] != 0
        for f in native + (["glszm"] if zflat is not None else []):
            i, w = FEATURE_FAMILIES.index(f), _FEATURE_ROW[f]
            for b in (range(B) if f != "glszm" else zflat.covered):
                e0, e1, r0, r1 = int(lay[0, i, b]), int(lay[0, i, b + 1]), int(lay[1, i, b]), int(lay[1, i, b + 1])
                out[f][b] = (vals[e0:e1].reshape(r1 - r0, w).copy(), empty[r0:r1].copy())
    for f in out:      # whatever the native call did not take
        for b in range(B):
            if out[f][b] is None:
                ng = int(Ng[b]) if isinstance(Ng, np.ndarray) else Ng
                out[f][b] = _single_glszm_features(glszm[b], ng) if f == "glszm" else _single_features(f, mats[f][b], symmetric, mcc)
    return out


def _texture_features(rois, Ng, classes, distances, gldm_a, symmetricalGLCM, mcc, mcc_angles, pl=Planar()):
    B = rois.B
    fams = tuple(f for f in FEATURE_FAMILIES[:4] if f in classes)
    status = np.ones(B, dtype=np.int64)
    routes = []
    mats, zones = {}, None
    pl = pl._replace(symmetric=bool(symmetricalGLCM))
    if fams:
        mats, st = _matrices(rois, Ng, fams, distances, gldm_a, pl)
        routes.append(last_batch_route())
        status &= np.asarray(st, dtype=np.int64) == _lib.PRAD_OK
    if "glszm" in classes:
        zones, st = _glszm(rois, Ng, True, pl)
        routes.append(last_batch_route())
        status &= np.asarray(st, dtype=np.int64) == _lib.PRAD_OK
    weighted = {f: mats[f + "_w"] for f in _cm.MERGE_FAMILIES if f + "_w" in mats}
    if weighted:
        # the ROI's one merged matrix per family, one angle and already symmetrised; the other families are laid out by the
        # true angle counts (the GLDM width), so they take a call of their own
        per = batch_features_per_angle(weighted, Ng, None, False, mcc)
        rest = {f: mats[f] for f in mats if f in FEATURE_FAMILIES and f not in weighted}
        if rest or zones is not None:
            per.update(batch_features_per_angle(rest, Ng, zones, symmetricalGLCM, mcc))
    else:
        per = batch_features_per_angle(mats, Ng, zones, symmetricalGLCM, mcc)
    table = {}
    for f in classes:
        rows = np.full((B, _FEATURE_ROW[f]), np.nan)
        for b in range(B):
            if status[b]:
                vals, empty = per[f][b]
                rows[b] = vals[0] if f == "ngtdm" else _cm._angle_mean(vals, empty)
        table[f] = rows
    if mcc_angles and "glcm" in classes:
        table["glcm_mcc_angles"] = [per["glcm"][b][0][:, 23].copy() if status[b] else None for b in range(B)]
    _cm._set_batch_route(_joined_route(routes))
    return table, status.tolist()


def texture_features_batch(levels, masks, sizes, Ng, classes=("glcm", "glrlm", "glszm", "gldm", "ngtdm"),
                           distances=(1,), gldm_a=0, symmetricalGLCM=True, mcc=True, mcc_angles=False, force2D=False,
                           force2Ddimension=0, weightingNorm=None, spacing=(1.0, 1.0, 1.0)):
    """The texture FEATURES of B small ROIs (segment mode; inputs as texture_matrices_batch): texture_matrices_batch,
    glszm_batch(compact=True), the formulas of all matrices in two launches (batch_features_per_angle) and, per ROI, the mean
    over the angles the reference keeps (cmatrices._angle_mean).  -> ({class: float64 numpy [B, nfeat]}, status [B]): glcm 24
    columns (cmatrices.VOXEL_GLCM_FEATURES, then MCC -- NaN without `mcc`), glrlm / gldm / glszm 16 (the shared zone numbering),
    ngtdm 5.  status 0: a masked level outside [1, Ng]; that ROI's rows are NaN, the others are not affected.
    force2D / force2Ddimension: every class uses the in-plane angle sets (texture_matrices_batch, glszm_batch).  weightingNorm +
    spacing ((z, y, x): one triple or float [B, 3]): the GLCM and GLRLM rows come from the ROI's ONE merged matrix ("glcm_w" /
    "glrlm_w" of texture_matrices_batch; MCC is evaluated on it) as the feature classes form them; GLDM, NGTDM and GLSZM ignore
    the weights, as the classes do.  Outside the native domain (Ng > 64, boxes above the batch caps) the single calls are looped and give the same
    values; last_batch_route() says "batch", "mixed" or "looped".  mcc_angles=True adds the entry "glcm_mcc_angles": per ROI the
    MCC of every angle (float64 [Na], NaN for an empty angle; None with status 0) -- what the feature class averages as a flat
    vector (cmatrices._mcc_angle_mean), in another order of additions than the column mean of the table; with weightingNorm
    it has length 1.
    Ng: an int, or an int sequence [B] that gives ROI b its own count Ng[b] (the discretisation of a fixed bin width): the ROIs
    of at most 64 levels inside the box caps go through the native calls together, whatever their counts; each of the others
    takes the single calls, the route is then "mixed", and a ROI above 64 levels has no MCC (NaN)."""
    rois, classes = _roi_batch(levels, masks, sizes), tuple(classes)
    if not classes or any(c not in FEATURE_FAMILIES for c in classes):
        raise ValueError("classes must be a non-empty subset of %s" % (FEATURE_FAMILIES,))
    return _texture_features(rois, _cm.batch_levels(Ng, rois.B), classes, distances, gldm_a, symmetricalGLCM, mcc, mcc_angles,
                             _planar(force2D, force2Ddimension, weightingNorm, spacing))


# ---- first-order statistics and discretisation (prad_batch_firstorder_dev / prad_batch_digitize_dev, -------------------------
# ---- csrc/kernels_batch_firstorder.h): raw intensity boxes in, the table of all six feature classes out ----------------------
def batch_firstorder_max_roi(dtype) -> int:
    """most ROI voxels (mask != 0) per ROI the batched first-order launch sorts in LDS: 32768, or 16384 for float64"""
    code = _eng._DTYPE_CODES[dtype] if dtype in _eng._DTYPE_CODES else int(dtype)
    return int(_lib.load().prad_batch_firstorder_max_roi(code))


def batch_digitize_max_edges() -> int:
    """most bin edges per ROI the batched discretisation stages in LDS (PRAD_BATCH_DIGITIZE_MAX_EDGES)"""
    return int(_lib.load().prad_batch_digitize_max_edges())


def _firstorder(rois, voxelArrayShift):
    B = rois.B
    table = torch.empty((B, 16), dtype=torch.float64, device=rois.device)
    rc = rois.lib.prad_batch_firstorder_dev(_vp(rois.data), _eng._DTYPE_CODES[rois.data.dtype], _vp(rois.mask), _iptr(rois.sizes),
                                            _lp(rois.off), B, float(voxelArrayShift), _vp(table), _eng._stream_ptr())
    if rc == _lib.PRAD_E_UNSUPPORTED:          # nothing was launched: every ROI takes the single call
        tab = np.full((B, 16), np.nan)
        tab[:, 15] = 8
    else:
        _lib.raise_for(rc, "batched first-order statistics")
        tab = table.cpu().numpy()              # the batch's first read-back
    status = tab[:, 15].astype(np.int64)
    rows = np.ascontiguousarray(tab[:, :15])
    rest = np.flatnonzero((status == 2) | (status == 8))
    for b in rest:
        st = _eng.firstorder_stats(rois.view(rois.data, b), rois.view(rois.mask, b), voxelArrayShift)
        rows[b] = [st[f] for f in _eng.FIRSTORDER_FIELDS]
    _cm._set_batch_route(_route(len(rest), B))
    return rows, status


def firstorder_batch(images, masks, sizes=None, voxelArrayShift=0.0):
    """The first-order statistics of B small ROIs in ONE launch (segment mode, 3-D).  images / masks: lists of 3-D device
    tensors of one dtype (float32, float64, int32, int16; anything else is widened to float64), or flat device tensors holding
    the boxes back to back plus `sizes` (int [B, 3]); masks bool or integer, non-zero = ROI.  -> (float64 numpy [B, 15] in the
    order of FIRSTORDER_FIELDS, status int64 [B] = the launch's verdict per ROI: 0 fine; 1 empty ROI, its row is NaN; 2 a
    non-finite ROI value and 8 more ROI voxels than batch_firstorder_max_roi(): that ROI's row comes from firstorder_stats).
    last_batch_route() says "batch", "mixed" (some ROIs went through firstorder_stats) or "looped" (all did)."""
    return _firstorder(_roi_batch(images, masks, sizes, raw=True), voxelArrayShift)


def _bin(rois, stats, binning):
    from . import imageoperations
    B, dev = rois.B, rois.device
    rows, status = _firstorder(rois, 0.0) if stats is None else stats
    rows, status = np.asarray(rows, dtype=np.float64).reshape(B, -1), np.asarray(status).reshape(B)
    np_dtype = _NP_DTYPES[rois.data.dtype]
    cap = batch_digitize_max_edges()
    edges = [np.zeros(0, dtype=np.float64)] * B
    single = []
    edge_off = np.zeros(B + 1, dtype=np.int64)
    count_off = np.full(B, -1, dtype=np.int64)
    ncounts = 0
    i_min, i_max = _eng.FIRSTORDER_FIELDS.index("Minimum"), _eng.FIRSTORDER_FIELDS.index("Maximum")
    for b in range(B):
        ne = 0
        if status[b] == 0:
            e = np.asarray(imageoperations.getBinEdges(np.array([rows[b, i_min], rows[b, i_max]], dtype=np_dtype), **binning),
                           dtype=np.float64)
            if len(e) <= cap:
                edges[b], ne = e, len(e)
        if status[b] == 1 or ne:
            count_off[b] = ncounts
            ncounts += ne + 1
        else:
            single.append(b)
        edge_off[b + 1] = edge_off[b] + ne
    levels = torch.empty(rois.data.numel(), dtype=torch.int32, device=dev)
    counts = [None] * B
    Ng = np.zeros(B, dtype=np.int64)
    if len(single) < B:
        flat_edges = np.concatenate(edges) if edge_off[B] else np.zeros(1, dtype=np.float64)
        d_edges = torch.from_numpy(flat_edges).to(dev)
        back = torch.empty(ncounts + (B + 1) // 2, dtype=torch.int64, device=dev)      # [counts | top (int32)]: one read-back
        top = back[ncounts:].view(torch.int32)
        rc = rois.lib.prad_batch_digitize_dev(_vp(rois.data), _eng._DTYPE_CODES[rois.data.dtype], _vp(rois.mask),
                                              _iptr(rois.sizes), _lp(rois.off), B, _vp(d_edges), _lp(edge_off), _vp(levels),
                                              _vp(back), _lp(count_off), _vp(top), _eng._stream_ptr())
        _lib.raise_for(rc, "batched discretisation")
        host = back.cpu().numpy()              # the batch's second read-back
        tops = host[ncounts:].view(np.int32)
        for b in range(B):
            if count_off[b] >= 0:
                Ng[b] = int(tops[b])
                counts[b] = host[int(count_off[b]):int(count_off[b]) + int(Ng[b]) + 1].copy()
    for b in single:
        lv, ng, e, c = _eng.bin_image(rois.view(rois.data, b), rois.view(rois.mask, b), with_counts=True, **binning)
        rois.view(levels, b).reshape(-1).copy_(lv.reshape(-1))
        Ng[b], edges[b], counts[b] = ng, e, c
    _cm._set_batch_route(_route(len(single), B))
    return levels, Ng, edges, counts


def bin_batch(images, masks, sizes=None, stats=None, **binning):
    """The discretisation of B small ROIs in ONE launch: every ROI gets its own bin edges -- imageoperations.getBinEdges on its
    (Minimum, Maximum), as bin_image builds them; binWidth and binCount both work -- and is digitised against them by its own
    workgroup.  Inputs as firstorder_batch; stats: the (rows, status) pair of firstorder_batch on the same batch (computed here
    when None).  -> (flat int32 level tensor in the batch layout, Ng int64 [B], list of B float64 edge arrays, list of B int64
    count arrays [Ng + 1]), ROI by ROI what bin_image(..., with_counts=True) returns.  An empty ROI has Ng 0, no edges, counts
    [0] and levels 0.  ROIs whose statistics came from the single call (status 2 / 8) or with more than
    batch_digitize_max_edges() edges go through bin_image; last_batch_route() says "batch", "mixed" or "looped"."""
    return _bin(_roi_batch(images, masks, sizes, raw=True), stats, binning)


def roi_features_batch(images, masks, sizes=None, classes=ROI_FEATURE_CLASSES, binWidth=None, binCount=None, voxelArrayShift=0,
                       voxelVolume=1.0, distances=(1,), gldm_a=0, symmetricalGLCM=True, mcc=True, extras=False, force2D=False,
                       force2Ddimension=0, weightingNorm=None, spacing=(1.0, 1.0, 1.0), resegmentRange=None,
                       resegmentMode="absolute"):
    """The feature table of B small ROIs from their raw intensity boxes and masks (inputs as firstorder_batch): firstorder_batch
    and bin_batch -- two launches and two read-backs for the whole batch (binWidth, default 25, or binCount) -- then
    texture_features_batch ONCE on the non-empty ROIs, every ROI with the Ng the discretisation gave it.  -> ({class: float64 numpy [B, nfeat]},
    status [B]): "firstorder" has the 19 columns of cmatrices.FIRSTORDER_FEATURES (firstorder.features_from_stats on the
    statistics, the level counts and voxelVolume, a number or [B]); the texture classes the columns of texture_features_batch.
    status 0: an empty ROI; its rows are NaN, the others are not affected.  last_batch_route() says "batch", "mixed" or
    "looped" (texture_features_batch loops the single calls above 64 levels; MCC is not evaluated there -- its column is NaN
    for a ROI with more than 64 levels, as without `mcc`).  extras=True adds two entries the label route of the feature extractor
    needs to report what the feature classes report: "gray_levels" int64 [B], the number of grey levels that occur in the ROI, and
    (with glcm) "glcm_mcc_angles", see texture_features_batch.  force2D / force2Ddimension / weightingNorm / spacing: passed
    to texture_features_batch; the first-order columns do not depend on them.  resegmentRange / resegmentMode: the masks are
    resegmented first (resegment_batch: one more launch and read-back), per ROI what execute() does with these settings; a ROI
    that is empty afterwards, or keeps a single voxel, is reported as an empty ROI is."""
    from . import firstorder as _fo
    spec = _resegment_settings({"resegmentRange": resegmentRange, "resegmentMode": resegmentMode})
    rois, reseg_route = _resegmented(_roi_batch(images, masks, sizes, raw=True), spec)
    pl = _planar(force2D, force2Ddimension, weightingNorm, spacing)
    classes = tuple(classes)
    if not classes or any(c not in ROI_FEATURE_CLASSES for c in classes):
        raise ValueError("classes must be a non-empty subset of %s" % (ROI_FEATURE_CLASSES,))
    binning = {"binCount": binCount} if binCount is not None else {"binWidth": 25 if binWidth is None else binWidth}
    B = rois.B
    routes = [] if reseg_route is None else [reseg_route]
    rows, verdict = _firstorder(rois, voxelArrayShift)
    routes.append(last_batch_route())
    levels, Ng, _, counts = _bin(rois, (rows, verdict), binning)
    routes.append(last_batch_route())
    binned = rois.with_data(levels)
    status = (verdict != 1).astype(np.int64)
    table = {}
    if "firstorder" in classes:
        vals = _fo.features_from_stats(rows, [c[1:] for c in counts], voxelVolume)
        vals[status == 0] = np.nan
        table["firstorder"] = vals
    texture = tuple(c for c in classes if c != "firstorder")
    angles = [None] * B
    if texture:
        for c in texture:
            table[c] = np.full((B, _FEATURE_ROW[c]), np.nan)
        idx = np.flatnonzero(status == 1)
        if len(idx):
            ngv = np.ascontiguousarray(Ng[idx].astype(np.intc))
            same = bool((ngv == ngv[0]).all())          # (binCount: one count, the scalar calls)
            few = ngv <= _cm.BATCH_MAX_NG               # (glcm_mcc declines more than 64 occurring levels)
            sub, st = _texture_features(binned.subset(idx), int(ngv[0]) if same else ngv, texture, distances, gldm_a,
                                        symmetricalGLCM, bool(mcc and few.any()), bool(extras and mcc and few.any()),
                                        pl.subset(idx, B))
            routes.append(last_batch_route())
            for k, b in enumerate(idx):
                if "glcm_mcc_angles" in sub and few[k]:
                    angles[b] = sub["glcm_mcc_angles"][k]
            for c in texture:
                table[c][idx] = sub[c]
            status[idx] &= np.asarray(st, dtype=np.int64)
    table = {c: table[c] for c in classes}
    if extras:
        table["gray_levels"] = np.array([int((np.asarray(c[1:]) > 0).sum()) for c in counts], dtype=np.int64)
        if "glcm" in classes:
            table["glcm_mcc_angles"] = angles
    _cm._set_batch_route(_joined_route(routes))
    return table, status.tolist()


# ---- wavelet sub-bands of the boxes (prad_batch_swt_dev, csrc/kernels_batch_swt.h) -------------------------------------------
class BandNames(tuple):
    """the image type names of the sub-bands in the order getWaveletImage yields them; rows[i] = the row of `bands` that
    names[i] refers to (row(name) looks it up)"""
    def __new__(cls, names, rows):
        self = super().__new__(cls, names)
        self.rows = tuple(int(r) for r in rows)
        return self

    def row(self, name):
        return self.rows[self.index(name)]


def wavelet_band_names(level=1, naxes=3) -> BandNames:
    """The names getWaveletImage yields for `level` levels over `naxes` transformed axes (3, or 2 with force2D), in its order:
    the detail bands of every level ("wavelet-LLH" ... "wavelet-HHH", from level 2 on "wavelet2-LLH" ...), then the last
    approximation.  Rows: at level 1 the band index of the kernels, (bx * 2 + by) * 2 + bz with L = 0 and H = 1 -- so the
    approximation, yielded last, is row 0; with more levels the rows follow the names."""
    keys = [""]
    for _ in range(int(naxes)):
        keys = [k + c for k in keys for c in "LH"]
    level = int(level)
    if level < 1:
        raise ValueError("wavelet level %d" % level)
    names = [("wavelet-%s" if idx == 1 else "wavelet%d-%%s" % idx) % k for idx in range(1, level + 1) for k in keys[1:]]
    names.append(("wavelet-%s" if level == 1 else "wavelet%d-%%s" % level) % keys[0])
    rows = list(range(1, len(keys))) + [0] if level == 1 else range(len(names))
    return BandNames(names, rows)


def batch_swt_plan(sizes, flen):
    """Host-side plan of the batched wavelet launch (prad_batch_swt_plan; pure, needs no device).  sizes: int [B, 3]; flen: the
    filter length.  -> (verdict int [B]: 0 native, 8 the single route; items int [n, 8]: per workgroup ROI, z0, z1, y0, y1,
    x0, x1 -- half-open, clipped to the box -- and the tile width TX).  NotImplementedError for a filter length the kernel is
    not built for (everything but 2, 4, 6), ValueError for bad arguments."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    B = int(sizes.shape[0])
    lib = _lib.load()
    verdict = np.zeros(max(B, 1), dtype=np.intc)
    n = C.c_longlong(0)
    _lib.raise_for(lib.prad_batch_swt_plan(_iptr(sizes), B, int(flen), _iptr(verdict), C.byref(n), None), "batch swt plan")
    items = np.zeros((max(int(n.value), 1), 8), dtype=np.intc)
    _lib.raise_for(lib.prad_batch_swt_plan(_iptr(sizes), B, int(flen), _iptr(verdict), C.byref(n), _iptr(items)), "batch swt plan")
    return verdict[:B].copy(), items[:int(n.value)]


def batch_swt_occupancy(sizes, flen):
    """Counts -- not measurements -- of what the plan of a batch leaves idle, from `sizes` alone: {"items", "active_lanes": share
    of the 256 lanes of the workgroups that own an output, "warmup_planes": share of the staged planes that are warm-up (F - 1
    per item) rather than output planes, "native": ROIs}."""
    verdict, items = batch_swt_plan(sizes, flen)
    if not len(items):
        return {"items": 0, "active_lanes": 0.0, "warmup_planes": 0.0, "native": 0}
    it = items.astype(np.int64)
    planes = it[:, 2] - it[:, 1]
    lanes = (it[:, 4] - it[:, 3]) * (it[:, 6] - it[:, 5])
    steps = planes + (int(flen) - 1)
    return {"items": int(len(it)), "active_lanes": float((lanes * steps).sum() / (256.0 * steps.sum())),
            "warmup_planes": float((int(flen) - 1) * len(it) / steps.sum()), "native": int((verdict == 0).sum())}


def _image_batch(images, sizes) -> RoiBatch:
    """raw intensity boxes without masks, as _roi_batch(raw=True) normalises them (the batch's `mask` is None)"""
    if isinstance(images, (list, tuple)):
        if not len(images):
            raise ValueError("empty batch")
        if any(i.dim() != 3 for i in images):
            raise ValueError("the batched wavelet takes 3-D boxes")
        sizes = np.array([tuple(i.shape) for i in images], dtype=np.intc).reshape(-1, 3)
        dts = [i.dtype for i in images]
        dt = dts[0] if dts[0] in _eng._DTYPE_CODES and all(d == dts[0] for d in dts) else torch.float64
        images = torch.cat([i.reshape(-1).to(dt) for i in images])
    elif sizes is None:
        raise ValueError("a flat image tensor needs `sizes`")
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    data = images.reshape(-1)
    if not data.is_cuda:
        raise ValueError("engine.* expects CUDA/HIP tensors; use pyradiomics_amd.cmatrices for numpy input")
    data = (data if data.dtype in _eng._DTYPE_CODES else data.to(torch.float64)).contiguous()
    lib = _lib.load()
    _set_device(lib, data.device)
    nvox = sizes.astype(np.int64).prod(1)
    if not len(nvox) or int(nvox.sum()) != data.numel():
        raise ValueError("sizes describe %d voxels, the buffer holds %d" % (int(nvox.sum()), data.numel()))
    return RoiBatch(lib, data, None, sizes, nvox, _offsets(nvox), data.device)


def _wavelet(rois, wavelet, level, start_level, force2D, force2Ddimension, out):
    from . import filters
    lo, hi = filters.wavelet_filters(wavelet)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    level, start_level = int(level), int(start_level)
    axes = [2, 1, 0]
    if force2D:
        _cm.batch_forced_dim(True, force2Ddimension)          # (raises on a dimension outside 0 .. 2)
        axes.remove(int(force2Ddimension))
    names = wavelet_band_names(level, len(axes))
    B, W = rois.B, rois.data.numel()
    if out is None:
        out = torch.empty((len(names), W), dtype=torch.float64, device=rois.device)
    elif (out.dtype != torch.float64 or out.device != rois.device or out.dim() != 2 or tuple(out.shape) != (len(names), W)
          or (W > 1 and out.stride(1) != 1) or out.stride(0) < W):
        raise ValueError("out must be a float64 [%d, %d] tensor on %s with contiguous rows" % (len(names), W, rois.device))
    verdict = np.full(B, 8, dtype=np.intc)
    if level == 1 and start_level == 0 and not force2D:
        rc = rois.lib.prad_batch_swt_dev(_vp(rois.data), _eng._DTYPE_CODES[rois.data.dtype], _iptr(rois.sizes), _lp(rois.off), B,
                                         C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data), len(lo), _vp(out),
                                         int(out.stride(0)), _iptr(verdict), _eng._stream_ptr())
        if rc == _lib.PRAD_E_UNSUPPORTED:          # a filter length the kernel is not built for: nothing was launched
            verdict[:] = 8
        else:
            _lib.raise_for(rc, "batched wavelet")
    rest = np.flatnonzero(verdict != 0)
    for b in rest:
        approx, ret = filters._swt3_device(rois.view(rois.data, b), tuple(axes), wavelet=(lo, hi), level=level,
                                           start_level=start_level)
        o, n = int(rois.off[b]), int(rois.nvox[b])
        for row, band in zip(names.rows, [t for wl in ret for t in wl.values()] + [approx]):
            out[row, o:o + n] = band.reshape(-1)
    _cm._set_batch_route(_route(len(rest), B))
    return out, names


def wavelet_batch(images, sizes=None, wavelet="coif1", level=1, start_level=0, force2D=False, out=None, force2Ddimension=0):
    """The wavelet sub-bands of B small boxes in ONE launch: per box what getWaveletImage computes on it (one wrapped sample
    appended to every odd axis, the undecimated periodised transform over x, y, z, the pad cropped), bit for bit.  images: a list
    of 3-D device tensors of one dtype (float32, float64, int32, int16; anything else is widened to float64), or a flat device
    tensor holding the boxes back to back plus `sizes` (int [B, 3]).  -> (bands, names, sizes): bands float64 [8, W] on the
    device, W the voxels of the batch -- every row is itself a flat batch tensor that roi_features_batch takes as `images`;
    names a BandNames: the strings getWaveletImage yields, in its order ("wavelet-LLH" ... "wavelet-HHH", "wavelet-LLL"), with
    names.rows[i] the row of `bands` that names[i] refers to; sizes int32 [B, 3].  out: a preallocated float64 [8, W] tensor
    (rows contiguous, row stride >= W) to fill instead.
    Native: filters of 2, 4 or 6 taps (haar / db1, db2 / sym2, coif1 / db3 / sym3) and boxes whose padded extents all hold the
    filter; the other boxes are filled from filters._swt3_device one by one.  Every box goes that way -- into the same layout --
    for a longer filter, for level != 1 or start_level != 0 (bands [7 * level + 1, W], rows in the order of the names) and
    with force2D (the axis force2Ddimension is not transformed: [4, W] at level 1).  last_batch_route() says "batch", "mixed"
    or "looped".  The sub-bands are float64 whatever the input (the single route's stated deviation for float32 images)."""
    rois = _image_batch(images, sizes)
    bands, names = _wavelet(rois, wavelet, level, start_level, force2D, force2Ddimension, out)
    return bands, names, rois.sizes


# ---- LoG images of the boxes (prad_batch_log_dev, csrc/kernels_batch_log.h) --------------------------------------------------
LOG_NO_IMAGE = 16          # verdict of a (ROI, sigma) pair the reference yields no image for (PRAD_BLOG_NO_IMAGE)
_LOG_MAX_SIGMAS = 8        # sigmas per call of prad_batch_log_dev


def batch_log_plan(sizes, sigma, spacing=(1.0, 1.0, 1.0)):
    """Host-side plan of the batched LoG launches (prad_batch_log_plan; pure, needs no device).  sizes: int [B, 3]; sigma: up to 8
    values > 0; spacing: one (z, y, x) triple or [B, 3].  -> (verdict int [S, B]: 0 the kernel computes the pair, 8 the box is
    too large for it (an extent above 64, or more than a compute unit's LDS) and the single route serves it, LOG_NO_IMAGE the
    reference yields no image for the pair -- an extent below 4 or below ceil(sigma / spacing) + 1; lds_class int [B]: 0, 1, 2
    by the LDS footprint of a box the kernel takes, -1 for any other).  ValueError for bad arguments."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    B = int(sizes.shape[0])
    sig = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(-1))
    sp = _cm.batch_spacing(spacing, B)
    verdict = np.zeros((max(len(sig), 1), max(B, 1)), dtype=np.intc)
    cls = np.zeros(max(B, 1), dtype=np.intc)
    n = C.c_longlong(0)
    rc = _lib.load().prad_batch_log_plan(_iptr(sizes), B, C.c_void_p(sp.ctypes.data), C.c_void_p(sig.ctypes.data), len(sig),
                                         _iptr(verdict), _iptr(cls), C.byref(n))
    _lib.raise_for(rc, "batch log plan")
    return verdict[:len(sig), :B].copy(), cls[:B].copy()


def _log_sigmas(sigma):
    """the sigmas getLoGImage filters with, in its order and with its warning for the others; duplicates once -> (values, names)"""
    from . import filters
    good = []
    for s in sigma:
        if s > 0.0:
            good.append(s)
        else:
            filters.logger.warning("applyLoG: sigma must be greater than 0.0: %s", s)
    good = list(dict.fromkeys(good))
    if not good:
        raise ValueError("the batched LoG needs at least one sigma above 0")
    return good, ["log-sigma-%s-mm-3D" % str(s).replace(".", "-") for s in good]


def _log(rois, sigma, spacing, normalize, out):
    sig, names = _log_sigmas(sigma)
    B, S, W = rois.B, len(sig), rois.data.numel()
    sp = _cm.batch_spacing(spacing, B)
    dt = torch.float64 if rois.data.dtype == torch.float64 else torch.float32
    if out is None:
        out = torch.empty((S, W), dtype=dt, device=rois.device)
    elif (out.dtype != dt or out.device != rois.device or out.dim() != 2 or tuple(out.shape) != (S, W)
          or (W > 1 and out.stride(1) != 1) or (S > 1 and out.stride(0) < W)):
        raise ValueError("out must be a %s [%d, %d] tensor on %s with contiguous rows" % (dt, S, W, rois.device))
    stride = int(out.stride(0)) if S > 1 else W
    values = np.ascontiguousarray(sig, dtype=np.float64)
    verdict = np.zeros((S, B), dtype=np.intc)
    for lo in range(0, S, _LOG_MAX_SIGMAS):
        part = np.ascontiguousarray(values[lo:lo + _LOG_MAX_SIGMAS])
        v = np.zeros((len(part), B), dtype=np.intc)
        rc = rois.lib.prad_batch_log_dev(_vp(rois.data), _eng._DTYPE_CODES[rois.data.dtype], _iptr(rois.sizes), _lp(rois.off), B,
                                         C.c_void_p(sp.ctypes.data), C.c_void_p(part.ctypes.data), len(part),
                                         1 if normalize else 0, _vp(out[lo]), stride, _iptr(v), _eng._stream_ptr())
        _lib.raise_for(rc, "batched LoG")
        verdict[lo:lo + len(part)] = v
    # the boxes the kernel does not take: the reference's own question (getLoGImage), then the single route box by box
    valid = verdict == 0
    looped = 0
    for b in np.flatnonzero((verdict == 8).any(0)):
        size = rois.sizes[b].astype(np.float64)
        rows = [s for s in np.flatnonzero(verdict[:, b] == 8)
                if size.min() >= 4 and np.all(size >= np.ceil(values[s] / sp[b]) + 1)]
        if not rows:
            continue
        o, n = int(rois.off[b]), int(rois.nvox[b])
        images = _eng.log_images(rois.view(rois.data, b), sp[b][::-1], [values[s] for s in rows], normalize)
        for s, image in zip(rows, images):
            out[s, o:o + n] = image.reshape(-1).to(dt)
            valid[s, b] = True
        looped += len(rows)
    _cm._set_batch_route(_route(looped, int(valid.sum())))
    return out, names, valid


def log_batch(images, sizes=None, sigma=(1.0, 2.0, 3.0), spacing=(1.0, 1.0, 1.0), normalize=True, out=None):
    """The LoG images of B small boxes for S sigmas in at most three launches: per box and sigma what getLoGImage computes on the
    box alone -- ITK's LaplacianRecursiveGaussianImageFilter with NormalizeAcrossScale, engine.log_images(box, spacing, [sigma]) --
    bit for bit.  images: as wavelet_batch takes them (a list of 3-D device tensors of one dtype -- float32, float64, int32,
    int16; anything else is widened to float64 --, or a flat device tensor plus `sizes` int [B, 3]); spacing: (z, y, x), one triple
    or [B, 3]; sigma: in the units of spacing, values <= 0 are dropped with the reference's warning, duplicates kept once.
    -> (logs, names, sizes, valid): logs [S, W] on the device, W the voxels of the batch, float64 for float64 boxes and float32
    otherwise -- every row is itself a flat batch tensor that roi_features_batch takes as `images`; names: the strings
    getLoGImage yields ("log-sigma-1-0-mm-3D" ...), one per row; sizes int32 [B, 3]; valid bool [S, B]: False where the reference
    yields no image (an extent below 4, or below ceil(sigma / spacing) + 1) -- that slice of `logs` is not written.  out: a
    preallocated [S, W] tensor of that dtype (rows contiguous, row stride >= W) to fill instead.
    Native: boxes whose extents all lie in 4 .. 64 and whose float32 copy, rows padded to an odd length, fits a compute unit's
    LDS (32^3 does, 36^3 does not; batch_log_plan tells); the other boxes are filled from engine.log_images one by one.
    last_batch_route() says "batch", "mixed" or "looped"."""
    rois = _image_batch(images, sizes)
    logs, names, valid = _log(rois, sigma, spacing, normalize, out)
    return logs, names, rois.sizes, valid


# ---- intensity transforms and Gradient of the boxes (prad_batch_intensity_dev, csrc/kernels_batch_intensity.h) ---------------
INTENSITY_TYPES = ("Square", "SquareRoot", "Logarithm", "Exponential")      # bit k of the C `types`, in the order of the rows
_GRADIENT_BIT = 1 << len(INTENSITY_TYPES)
INTENSITY_ZERO = 1         # verdict of a ROI whose box is all zeros: the reference's formulas divide by zero (the single route)
INTENSITY_NONFINITE = 2    # verdict of a float ROI that holds a NaN or an infinity (the single route, Gradient included)


def _intensity_bits(types, what="intensity_batch"):
    """the image type names `types` -> (the C bit mask, the names in the order of the rows); ValueError for any other name"""
    types = (types,) if isinstance(types, str) else tuple(types)
    unknown = [t for t in types if t not in INTENSITY_TYPES]
    if unknown or not types:
        raise ValueError("%s: types must be a non-empty subset of %s, got %r" % (what, INTENSITY_TYPES, types))
    bits = sum(1 << INTENSITY_TYPES.index(t) for t in set(types))
    return bits, tuple(t for t in INTENSITY_TYPES if t in types)


def batch_intensity_plan(sizes, types=INTENSITY_TYPES + ("Gradient",)):
    """Host-side plan of the batched intensity launches (prad_batch_intensity_plan; pure, needs no device).  sizes: int [B, 3] (B = 0
    is a valid, empty plan); types: names out of "Square", "SquareRoot", "Logarithm", "Exponential", "Gradient".  -> (items int64
    [n, 4]: per workgroup of the image launch the half-open range [w0, w1) of the batch's voxels in their packed order and the
    first and last ROI the range touches -- a workgroup writes its voxels of every requested row; grid int64 [2]: the workgroups
    of the constants launch -- one per ROI, 0 for Gradient alone -- and of the image launch).  ValueError for an unknown type
    or a size below 1, NotImplementedError above the grid limit."""
    types = (types,) if isinstance(types, str) else tuple(types)
    bits = _GRADIENT_BIT if "Gradient" in types else 0
    rest = tuple(t for t in types if t != "Gradient")
    if rest or not bits:
        bits |= _intensity_bits(rest, "batch_intensity_plan")[0]
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    B = int(sizes.shape[0])
    lib = _lib.load()
    n = C.c_longlong(0)
    grid = np.zeros(2, dtype=np.int64)
    _lib.raise_for(lib.prad_batch_intensity_plan(_iptr(sizes), B, bits, C.byref(n), None, _lp(grid)), "batch intensity plan")
    items = np.zeros((max(int(n.value), 1), 4), dtype=np.int64)
    _lib.raise_for(lib.prad_batch_intensity_plan(_iptr(sizes), B, bits, C.byref(n), _lp(items), _lp(grid)), "batch intensity plan")
    return items[:int(n.value)], grid


def _flat_voxels(images, sizes, what):
    """the voxels of the batch, from the arguments alone (no device is asked): lists give their own shapes, a flat tensor must
    hold what `sizes` describes"""
    if isinstance(images, (list, tuple)):
        if not len(images):
            raise ValueError("empty batch")
        return int(sum(int(i.numel()) for i in images))
    if sizes is None:
        raise ValueError("a flat image tensor needs `sizes`")
    nvox = np.asarray(sizes, dtype=np.int64).reshape(-1, 3).prod(1)
    if not len(nvox) or int(nvox.sum()) != images.numel():
        raise ValueError("%s: sizes describe %d voxels, the buffer holds %d" % (what, int(nvox.sum()), images.numel()))
    return int(nvox.sum())


def _check_out(out, dtype, shape, what):
    """`out` of the intensity calls: a tensor of `dtype` and `shape` with contiguous rows (row stride >= the row length)"""
    if out is None:
        return
    W = shape[-1]
    ok = (out.dtype == dtype and tuple(out.shape) == tuple(shape) and (W <= 1 or out.stride(-1) == 1)
          and (len(shape) == 1 or shape[0] <= 1 or out.stride(0) >= W))
    if not ok:
        raise ValueError("%s: out must be a %s %s tensor with contiguous rows" % (what, dtype, list(shape)))


def _intensity(rois, bits, spacing, use_spacing, out, out_grad):
    """the C call and the fallback for any subset of the five types; out / out_grad have been checked but for their device.
    -> (rows float64 [T, W] or None, gradient float32 [W] or None, verdict [B])"""
    from . import filters
    from .image import Image
    B, W = rois.B, rois.data.numel()
    names = [t for k, t in enumerate(INTENSITY_TYPES) if bits >> k & 1]
    T, grad = len(names), bool(bits & _GRADIENT_BIT)
    for o in (out, out_grad):
        if o is not None and o.device != rois.device:
            raise ValueError("out must live on %s" % (rois.device,))
    if T and out is None:
        out = torch.empty((T, W), dtype=torch.float64, device=rois.device)
    if grad and out_grad is None:
        out_grad = torch.empty(W, dtype=torch.float32, device=rois.device)
    sp = _cm.batch_spacing(spacing, B)
    if grad and use_spacing and not (np.isfinite(sp).all() and (sp > 0).all()):
        raise ValueError("spacing must be positive and finite")
    stride = int(out.stride(0)) if T > 1 else W
    verdict = np.zeros(B, dtype=np.intc)
    rc = rois.lib.prad_batch_intensity_dev(_vp(rois.data), _eng._DTYPE_CODES[rois.data.dtype], _iptr(rois.sizes), _lp(rois.off), B,
                                           bits, C.c_void_p(sp.ctypes.data), 1 if use_spacing else 0, _vp(out if T else None),
                                           stride, _vp(out_grad if grad else None), _iptr(verdict), _eng._stream_ptr())
    _lib.raise_for(rc, "batched intensity transforms")
    # the ROIs the kernels leave alone: the single route box by box, into the same layout (its NaN / inf are the single route's)
    single = {"Square": filters.getSquareImage, "SquareRoot": filters.getSquareRootImage,
              "Logarithm": filters.getLogarithmImage, "Exponential": filters.getExponentialImage}
    looped = 0
    for b in np.flatnonzero(verdict != 0):
        o, n = int(rois.off[b]), int(rois.nvox[b])
        box = Image(tensor=rois.view(rois.data, b), spacing=tuple(float(s) for s in sp[b][::-1]))
        for row, t in enumerate(names):
            image, _, _ = next(single[t](box, None, deviceResident=True))
            out[row, o:o + n] = image.device_tensor().reshape(-1)
        if grad and verdict[b] == INTENSITY_NONFINITE:
            image, _, _ = next(filters.getGradientImage(box, None, deviceResident=True, gradientUseSpacing=bool(use_spacing)))
            out_grad[o:o + n] = image.device_tensor().reshape(-1)
        looped += 1 if (T or verdict[b] == INTENSITY_NONFINITE) else 0
    _cm._set_batch_route(_route(looped, B))
    return (out if T else None), (out_grad if grad else None), verdict


def intensity_batch(images, sizes=None, types=INTENSITY_TYPES, out=None):
    """The Square, SquareRoot, Logarithm and Exponential images of B small boxes in TWO launches whatever B and the number of types:
    per box what filters.getSquareImage ... getExponentialImage compute on the box alone.  With top = max |x| of the BOX AS HANDED
    OVER -- not of the scan it was cut from: the values are those of `execute` on the box, the reference's with preCrop --
    square (c x)(c x), c = 1 / sqrt(top); squareroot sign(x) sqrt(|x| top); logarithm sign(x) log(|x| + 1) top / log(top + 1);
    exponential exp(log(top) / top x), in float64 with the single route's operations in their order: square and squareroot equal
    it bit for bit, logarithm and exponential to the accuracy of two implementations of log and exp.  images: as wavelet_batch
    takes them (a list of 3-D device tensors of one dtype -- float32, float64, int32, int16; anything else is widened to float64 --,
    or a flat device tensor plus `sizes` int [B, 3]); types: a subset of the four names.  -> (rows, names, sizes): rows float64
    [T, W] on the device, W the voxels of the batch, one row per requested type in the order Square, SquareRoot, Logarithm,
    Exponential -- every row is itself a flat batch tensor that roi_features_batch takes as `images`; names: the strings the
    single functions yield ("square", "squareroot", "logarithm", "exponential"), one per row; sizes int32 [B, 3].  out: a
    preallocated float64 [T, W] tensor (rows contiguous, row stride >= W) to fill instead.
    Native: every box whatever its size.  A box that is all zeros (the formulas divide by zero) or, in a float batch, holds a NaN
    or an infinity is filled from the single functions instead, so its NaN / inf are exactly theirs; last_batch_route() says
    "batch", "mixed" or "looped".  Argument errors (an unknown type, sizes that do not describe the buffer, a bad `out`) are
    raised before any device work."""
    bits, kept = _intensity_bits(types)
    W = _flat_voxels(images, sizes, "intensity_batch")
    _check_out(out, torch.float64, (len(kept), W), "intensity_batch")
    rois = _image_batch(images, sizes)
    rows, _, _ = _intensity(rois, bits, (1.0, 1.0, 1.0), False, out, None)
    return rows, tuple(t.lower() for t in kept), rois.sizes


def gradient_batch(images, sizes=None, spacing=(1.0, 1.0, 1.0), gradientUseSpacing=True, out=None):
    """The Gradient magnitude images of B small boxes in ONE launch: per box what filters.getGradientImage computes on the box
    alone, bit for bit -- per axis z, y, x of extent above 1 the central difference 0.5 (x[i + 1] - x[i - 1]), divided by the
    spacing unless gradientUseSpacing is false, squared and summed in float64, the root rounded once to float32.  The gradient
    replicates the BOX's OWN edge (a voxel on a face of the box sees itself beyond it), not the scan the box was cut from: the
    values are those of `execute` on the box, the reference's with preCrop.  images: as wavelet_batch takes them; spacing: (z, y,
    x), one triple or [B, 3].  -> (image float32 [W] on the device -- a flat batch tensor that roi_features_batch takes as
    `images` --, "gradient", sizes int32 [B, 3]).  out: a preallocated float32 [W] tensor to fill instead.
    Native: every box whatever its size, an all-zero box included (its image is zeros).  A float box that holds a NaN or an
    infinity is filled from the single function instead; last_batch_route() says "batch", "mixed" or "looped".  Argument errors
    are raised before any device work."""
    W = _flat_voxels(images, sizes, "gradient_batch")
    _check_out(out, torch.float32, (W,), "gradient_batch")
    rois = _image_batch(images, sizes)
    _, image, _ = _intensity(rois, _GRADIENT_BIT, spacing, bool(gradientUseSpacing), None, out)
    return image, "gradient", rois.sizes


# ---- LBP2D images of the boxes (prad_batch_lbp2d_dev, csrc/kernels_batch_lbp2d.h) ---------------------------------------------
def batch_lbp2d_plan(sizes, force2Ddimension=0, halo=1):
    """Host-side plan of the batched LBP2D launch (prad_batch_lbp2d_plan; pure, needs no device).  sizes: int [B, 3]; halo =
    ceil(lbp2DRadius).  -> (items int32 [n, 4]: per workgroup the ROI and the first output voxel (z0, y0, x0) of its tile inside
    the box; tile (tz, ty, tx): the one tile shape of the launch, that of the largest extent per axis; lds: the bytes of dynamic
    LDS; verdict: 0 native, 1 halo beyond the domain, 2 too many workgroups -- then no items).  The tiles of a box cover its
    voxels exactly once."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    B = int(sizes.shape[0])
    lib = _lib.load()
    tile = np.zeros(3, dtype=np.intc)
    n, lds, verdict = C.c_longlong(0), C.c_longlong(0), C.c_int(0)
    args = (_iptr(sizes), B, int(force2Ddimension), int(halo), _iptr(tile), C.byref(n))
    _lib.raise_for(lib.prad_batch_lbp2d_plan(*args, None, C.byref(lds), C.byref(verdict)), "batch lbp2d plan")
    items = np.zeros((max(int(n.value), 1), 4), dtype=np.intc)
    if verdict.value == 0:
        _lib.raise_for(lib.prad_batch_lbp2d_plan(*args, _iptr(items), C.byref(lds), C.byref(verdict)), "batch lbp2d plan")
    return (items[:int(n.value) if verdict.value == 0 else 0], tuple(int(t) for t in tile), int(lds.value), int(verdict.value))


def _lbp2d(rois, radius, samples, method, axis, out):
    """the C call, or -- beyond the kernel's domain -- the host route box by box; `out` has been checked but for its device"""
    from . import filters
    W = rois.data.numel()
    axis = int(axis)
    if not 0 <= axis <= 2:
        raise ValueError("force2Ddimension must be 0, 1 or 2")
    rp, cp, P, halo, code = _eng._lbp2d_table(radius, samples, method, None)
    if out is None:
        out = torch.empty(W, dtype=torch.float64, device=rois.device)
    elif out.device != rois.device:
        raise ValueError("out must live on %s" % (rois.device,))
    if _eng.lbp2d_native(rois.data.dtype, radius, samples):
        rc = rois.lib.prad_batch_lbp2d_dev(_vp(rois.data), _eng._DTYPE_CODES[rois.data.dtype], _iptr(rois.sizes), _lp(rois.off),
                                           rois.B, axis, C.c_void_p(rp.ctypes.data), C.c_void_p(cp.ctypes.data), P, halo, code,
                                           _vp(out), _eng._stream_ptr())
        if rc != _lib.PRAD_E_UNSUPPORTED:
            _lib.raise_for(rc, "batched LBP2D")
            _cm._set_batch_route(_route(0, rois.B))
            return out
    host = rois.data.cpu().numpy()
    for b in range(rois.B):
        o, n = int(rois.off[b]), int(rois.nvox[b])
        box = host[o:o + n].reshape(tuple(rois.sizes[b])).astype(np.float64)
        out[o:o + n] = torch.from_numpy(filters.lbp2d_host(box, radius, samples, method, axis).reshape(-1)).to(rois.device)
    _cm._set_batch_route(_route(rois.B, rois.B))
    return out


def lbp2d_batch(images, sizes=None, lbp2DRadius=1, lbp2DSamples=8, lbp2DMethod="uniform", force2Ddimension=0, out=None):
    """The LBP2D images of B boxes in ONE launch, boxes of any size: per box what filters.getLBP2DImage computes on the box ALONE
    -- a sample beyond the box's edge reads 0, not the scan the box was cut from: the values are those of `execute` on the box,
    the reference's with preCrop --, equal to engine.lbp2d on that box bit for bit (the same device function runs both).  images:
    as wavelet_batch takes them (a list of 3-D device tensors of one dtype -- float32, float64, int32, int16; anything else is
    widened to float64 --, or a flat device tensor plus `sizes` int [B, 3]).  -> (image float64 [W] on the device, W the voxels
    of the batch -- a flat batch tensor that roi_features_batch takes as `images` --, "lbp-2D", sizes int32 [B, 3]).  out: a
    preallocated float64 [W] tensor to fill instead.  Work is divided by output tiles from a host-built item table
    (batch_lbp2d_plan).  Native: ceil(lbp2DRadius) <= 8; a wider radius fills every box from filters.lbp2d_host
    (last_batch_route() says "batch" or "looped").  `var` raises NotImplementedError, argument errors are raised before any
    device work."""
    W = _flat_voxels(images, sizes, "lbp2d_batch")
    _check_out(out, torch.float64, (W,), "lbp2d_batch")
    from . import filters
    filters.lbp2d_settings(lbp2DRadius, lbp2DSamples, lbp2DMethod)
    rois = _image_batch(images, sizes)
    image = _lbp2d(rois, lbp2DRadius, lbp2DSamples, lbp2DMethod, force2Ddimension, out)
    return image, "lbp-2D", rois.sizes


def _tight_boxes(rois):
    """The box the feature classes of the reference see -- computeFeatures crops every derived image to the ROI's bounding box
    (featureextractor.py:560-604), here cropToTumorMask(padDistance=0)'s box: the bounding box of the mask with its x extent
    grown to a multiple of four inside the given box (imageoperations.alignedBox) -- for every ROI of the batch, worked out on
    the device, ROIs of one shape together.  -> (int64 device tensor: the elements of the flat buffers that make up the tight
    boxes, back to back in the ROIs' order; sizes intc [B, 3]).  A ROI with an empty mask keeps its whole box."""
    from . import imageoperations
    dev, B = rois.device, rois.B
    tight = rois.sizes.copy()
    picks, owners = [], []
    shapes, inverse = np.unique(rois.sizes, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    for g, shape in enumerate(shapes):
        bs = np.flatnonzero(inverse == g)
        G, n = len(bs), int(np.prod(shape.astype(np.int64)))
        pos = torch.from_numpy(rois.off[bs]).to(dev)[:, None] + torch.arange(n, device=dev)[None, :]
        m = (rois.mask[pos] != 0).view(G, *[int(s) for s in shape])
        ends = []
        for ax in range(3):
            line = m.to(torch.uint8).amax(dim=tuple(d + 1 for d in range(3) if d != ax)).to(torch.int32)
            ends += [line.argmax(1), int(shape[ax]) - 1 - line.flip(1).argmax(1), line.sum(1)]
        ends = torch.stack(ends, 1).cpu().numpy().astype(np.int64)       # one read-back per shape
        lo, hi = ends[:, 0::3].copy(), ends[:, 1::3].copy()
        empty = ends[:, 2] == 0
        lo[empty], hi[empty] = 0, shape.astype(np.int64) - 1
        lo, hi = imageoperations.alignedBox(lo, hi, tuple(int(s) for s in shape))
        tight[bs] = (hi - lo + 1).astype(np.intc)
        d_lo, d_hi = torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
        keep = None
        for ax in range(3):
            i = torch.arange(int(shape[ax]), device=dev).view([1] + [-1 if d == ax else 1 for d in range(3)])
            inside = (i >= d_lo[:, ax].view(G, 1, 1, 1)) & (i <= d_hi[:, ax].view(G, 1, 1, 1))
            keep = inside if keep is None else keep & inside
        keep = keep.reshape(G, n)
        picks.append(pos[keep])
        owners.append(torch.from_numpy(bs).to(dev)[:, None].expand(G, n)[keep])
    idx = torch.cat(picks)
    if len(shapes) > 1:          # (the groups follow one another: back into the ROIs' order, each box keeping its own)
        idx = idx[torch.argsort(torch.cat(owners), stable=True)]
    return idx, np.ascontiguousarray(tight)


_WAVELET_SETTINGS = ("wavelet", "level", "start_level")


_IMAGE_TYPES = ("Original", "Wavelet")                 # what roi_features_batch_images takes
_DERIVED_TYPES = ("Original", "Wavelet", "LoG")        # what roi_features_batch_derived takes


def roi_features_batch_images(images, masks, sizes=None, imageTypes=None, classes=ROI_FEATURE_CLASSES, **settings):
    """roi_features_batch on the boxes themselves ("Original") and on their wavelet sub-bands ("Wavelet": wavelet_batch, one
    launch for all eight), each derived image binned on its own per ROI as the reference bins every derived image.  The
    transform sees the boxes as they are given -- with the margin around the ROI that the filter needs, padDistance in the
    reference --; the feature calls see every image cut to the ROI's bounding box (_tight_boxes: one gather per image), as the
    reference's feature classes do, so a ROI's values do not depend on the margin it was handed over with.  imageTypes:
    {"Original": {}, "Wavelet": {}} by default; the dict of a type holds settings for that type alone (for "Wavelet" also
    wavelet / level / start_level), which override **settings -- the keyword arguments of roi_features_batch; force2D and
    force2Ddimension also steer the transform, as in getWaveletImage.  Any other image type: NotImplementedError ("LoG" is
    batched by roi_features_batch_derived, whose results for a box depend on the box it is handed, not on the ROI alone).
    -> ({image name: {class: float64 numpy [B, nfeat]}}, status [B]): image names "original" and those of wavelet_batch, in
    the reference's order; status[b] is the AND over the images.  last_batch_route() joins the routes of all calls.
    resegmentRange / resegmentMode (settings of the call, not of an image type; also taken by roi_features_batch_derived,
    _types and _resampled -- there after resampling): the masks are resegmented once on the boxes as given (resegment_batch),
    every image type then uses the new masks; a ROI that fails resegmentation has status 0 and NaN rows."""
    imageTypes = {"Original": {}, "Wavelet": {}} if imageTypes is None else dict(imageTypes)
    for t in imageTypes:
        if t not in _IMAGE_TYPES:
            raise NotImplementedError("roi_features_batch_images: image type %r (Original and Wavelet are batched here%s)"
                                      % (t, "; roi_features_batch_derived takes LoG" if t == "LoG" else ""))
    return _roi_features_images(images, masks, sizes, imageTypes, classes, settings)


def roi_features_batch_derived(images, masks, sizes=None, imageTypes=None, classes=ROI_FEATURE_CLASSES, **settings):
    """roi_features_batch_images with the LoG images as a third image type: "LoG": {"sigma": [...]} makes one log_batch call for
    all sigmas and one feature call per sigma; `spacing` (z, y, x; the argument the planar route reads) comes from the
    settings.  The LoG is that of the box ALONE, the reference's with preCrop: a recursive filter has unbounded support, so --
    unlike the wavelet sub-bands -- the LoG of a whole volume does not equal the LoG of a crop on the ROI's voxels, however wide
    the margin, and the values of a ROI depend on the box it is handed over in.  The images go in the reference's order, that of
    imageTypes ({"Original": {}, "Wavelet": {}, "LoG": ...} keys); image names are "original", those of wavelet_batch and those of
    log_batch.  A ROI for which the reference yields no LoG image at some sigma (log_batch's `valid`) has NaN rows in that
    image's tables, and its status is not lowered by them.  "LoG" with force2D and any image type but the three:
    NotImplementedError.  -> as roi_features_batch_images."""
    imageTypes = {"Original": {}, "Wavelet": {}} if imageTypes is None else dict(imageTypes)
    for t in imageTypes:
        if t not in _DERIVED_TYPES:
            raise NotImplementedError("roi_features_batch_derived: image type %r (Original, Wavelet and LoG are batched)" % (t,))
    return _roi_features_images(images, masks, sizes, imageTypes, classes, settings)


_LBP2D_SETTINGS = ("lbp2DRadius", "lbp2DSamples", "lbp2DMethod")
# what roi_features_batch_types takes: every image type
_ALL_TYPES = _DERIVED_TYPES + INTENSITY_TYPES + ("Gradient", "LBP2D")


def roi_features_batch_types(images, masks, sizes=None, imageTypes=None, classes=ROI_FEATURE_CLASSES, **settings):
    """roi_features_batch_derived with the remaining five image types of the extractor: "Square", "SquareRoot", "Logarithm",
    "Exponential" and "Gradient" -- ONE prad_batch_intensity_dev call (two launches) for all of them that are enabled, then one
    feature call per image.  As with the LoG the images are those of the box ALONE, the reference's with preCrop: the
    maximum |x| the four transforms scale with is that of the box as handed over, not of the scan it was cut from, and the
    gradient replicates the box's own edge -- the values of a ROI depend on the box it is handed over in.  `spacing` (z, y, x;
    one triple or [B, 3], the argument the planar route reads) and `gradientUseSpacing` (default True) come
    from the settings; the latter is read here and handed to no feature call.  The images go in the reference's order, that
    of imageTypes' keys, under the reference's image names ("square", "squareroot", "logarithm", "exponential", "gradient").  A ROI
    whose box is all zeros or holds a value that is not finite gets the single route's images (intensity_batch).  Any name
    that is no image type: NotImplementedError.  -> as roi_features_batch_images.
    "LBP2D" is the ninth type: ONE prad_batch_lbp2d_dev launch for all boxes (lbp2d_batch), image name "lbp-2D".  Its settings
    lbp2DRadius, lbp2DSamples and lbp2DMethod are read here and handed to no feature call; force2Ddimension, which the feature
    calls read as well, names the axis the planes are stacked along.  Again the image is that of the box alone: a sample beyond
    the box's edge reads 0."""
    imageTypes = {"Original": {}} if imageTypes is None else dict(imageTypes)
    for t in imageTypes:
        if t not in _ALL_TYPES:
            raise NotImplementedError("roi_features_batch_types: %r is not an image type (%s)" % (t, ", ".join(_ALL_TYPES)))
    return _roi_features_images(images, masks, sizes, imageTypes, classes, settings,
                                own=("gradientUseSpacing",) + _LBP2D_SETTINGS)


def _roi_features_images(images, masks, sizes, imageTypes, classes, settings, own=()):
    """the image types have been checked; own: settings the image types read that no feature call takes"""
    if not imageTypes:
        raise ValueError("roi_features_batch_images: no image type")
    settings = dict(settings)
    # resegmentRange / resegmentMode: the masks are resegmented ONCE, on the boxes as given (the Original image, as execute()
    # orders the steps); every image type then works with the new masks
    spec = _resegment_settings(settings)
    rois, reseg_route = _resegmented(_roi_batch(images, masks, sizes, raw=True), spec)
    tables, routes = {}, ([] if reseg_route is None else [reseg_route])
    made = {}

    def transformed():
        """the images of every enabled type of the five, from one call"""
        if not made:
            bits, merged = 0, dict(settings)
            for t, custom in imageTypes.items():
                if t in INTENSITY_TYPES:
                    bits |= 1 << INTENSITY_TYPES.index(t)
                elif t == "Gradient":
                    bits |= _GRADIENT_BIT
                    merged.update(custom or {})
            rows, grad, _ = _intensity(rois, bits, merged.get("spacing", (1.0, 1.0, 1.0)), merged.get("gradientUseSpacing", True),
                                       None, None)
            routes.append(last_batch_route())
            kept = [t for k, t in enumerate(INTENSITY_TYPES) if bits >> k & 1]
            made.update({t: rows[i] for i, t in enumerate(kept)})
            made["Gradient"] = grad
        return made

    status = np.ones(rois.B, dtype=np.int64)
    pick, tight_sizes = _tight_boxes(rois)
    tight_mask = rois.mask[pick]

    def features(name, data, kw, no_image=None):
        table, st = roi_features_batch(data[pick], tight_mask, tight_sizes, classes, **kw)
        routes.append(last_batch_route())
        st = np.asarray(st, dtype=np.int64)
        if no_image is not None and no_image.any():
            for v in table.values():
                if isinstance(v, np.ndarray) and v.shape[:1] == (rois.B,):
                    v[no_image] = np.nan if v.dtype.kind == "f" else 0
            st = np.where(no_image, 1, st)
        tables[name] = table
        status[:] &= st

    for t, custom in imageTypes.items():
        kw = dict(settings)
        kw.update(custom or {})
        lbp = {k: kw[k] for k in _LBP2D_SETTINGS if k in kw}
        for k in tuple(own) + ("resegmentRange", "resegmentMode"):      # (per call, not per image type: done above)
            kw.pop(k, None)
        if t == "LBP2D":
            image = _lbp2d(rois, lbp.get("lbp2DRadius", 1), lbp.get("lbp2DSamples", 8), lbp.get("lbp2DMethod", "uniform"),
                           kw.get("force2Ddimension", 0), None)
            routes.append(last_batch_route())
            features("lbp-2D", image, kw)
            continue
        if t in INTENSITY_TYPES or t == "Gradient":
            features(t.lower(), transformed()[t], kw)
            continue
        if t == "Original":
            features("original", rois.data, kw)
            continue
        if t == "LoG":
            sigma = kw.pop("sigma", [])
            if kw.get("force2D", False):
                raise NotImplementedError("roi_features_batch_derived: LoG with force2D is not batched")
            logs, names, valid = _log(rois, sigma, kw.get("spacing", (1.0, 1.0, 1.0)), True, None)
            routes.append(last_batch_route())
            for s, name in enumerate(names):
                image, bad = logs[s], ~valid[s]
                for b in np.flatnonzero(bad):      # (a slice nothing wrote: the box itself stands in, its rows become NaN)
                    o, n = int(rois.off[b]), int(rois.nvox[b])
                    image[o:o + n] = rois.data[o:o + n].to(image.dtype)
                features(name, image, kw, bad)
            continue
        wkw = {k: kw.pop(k) for k in _WAVELET_SETTINGS if k in kw}
        bands, names = _wavelet(rois, wkw.get("wavelet", "coif1"), wkw.get("level", 1), wkw.get("start_level", 0),
                                kw.get("force2D", False), kw.get("force2Ddimension", 0), None)
        routes.append(last_batch_route())
        for name, row in zip(names, names.rows):
            features(name, bands[row], kw)
    _cm._set_batch_route(_joined_route(routes))
    return tables, status.tolist()


# ---- resampling the boxes, each onto a grid of its own (prad_batch_resample_dev, csrc/kernels_batch_resample.h) ---------------
RESAMPLE_EMPTY = 1         # status of a ROI with an empty mask: nothing to centre a grid on, the box is kept as it is


class ResamplePlan(NamedTuple):
    """what batch_resample_plan works out per ROI; every [B, 3] array is (z, y, x) but origin_shift"""
    start: np.ndarray            # float64 [B, 3]: continuous input index of output voxel 0
    step: np.ndarray             # float64 [B, 3]: input voxels per output voxel
    newsize: np.ndarray          # intc [B, 3]
    interpolator: np.ndarray     # intc [B]: 0 nearest (also: a plain crop), 1 linear, 3 cubic B-spline
    spacing: np.ndarray          # float64 [B, 3]: the spacing of the new grid
    origin_shift: np.ndarray     # float64 [B, 3], (x, y, z) as an Image's origin is: the new origin minus the box's, along its axes
    status: np.ndarray           # int64 [B]: 0, or RESAMPLE_EMPTY


def batch_resample_max_vox() -> int:
    """voxels of the largest box prad_batch_resample_dev resamples itself (= batch_max_vox(); output voxels are not capped)"""
    return int(_lib.load().prad_batch_resample_max_vox())


def _interpolator_codes(interpolator, B):
    """an interpolator name or code as resampleImage accepts it, or [B] of them -> intc [B]; NotImplementedError for any other"""
    from .imageoperations import INTERPOLATOR_CODES
    one = isinstance(interpolator, (str, int, np.integer))
    items = [interpolator] * B if one else list(interpolator)
    if len(items) != B:
        raise ValueError("interpolator must be one name or code, or one per ROI (%d given for %d ROIs)" % (len(items), B))
    for i in items:
        if str(i) not in INTERPOLATOR_CODES:
            raise NotImplementedError("interpolator %r" % (i,))
    return np.array([INTERPOLATOR_CODES[str(i)] for i in items], dtype=np.intc).reshape(B)


def batch_resample_plan(sizes, lo, hi, spacing, resampledPixelSpacing, padDistance=5, interpolator=3,
                        alignCrop=True) -> ResamplePlan:
    """The grid imageoperations.resampleImage would resample every box onto if the box were the whole image: its expressions in
    float64, elementwise over [B, 3] (pure numpy, needs no device).  sizes int [B, 3]; lo / hi int [B, 3]: the inclusive
    (z, y, x) bounds of the masks (mask_boxes_batch; hi < lo marks an empty mask); spacing (z, y, x), one triple or [B, 3];
    resampledPixelSpacing (x, y, z) as in the parameter file it mirrors, a 0 keeps that axis' spacing, and so does an axis along
    which the bounding box is one voxel thick; interpolator: a name or code resampleImage accepts, or [B] of them.
    Where the spacing does not change (np.allclose, as in the reference) the ROI is a plain crop to cropToTumorMask's device
    box -- the bounding box with its x extent grown to a multiple of four inside the box, imageoperations.alignedBox,
    padDistance 0 -- expressed as nearest with step 1 and an integer start, so the kernel copies bits.  alignCrop=False cuts the
    bounding box itself, the extent resampleImage's own crop has: what a filter applied to the crop must see
    (roi_features_batch_resampled).  An empty mask keeps its whole box the same way and gets status RESAMPLE_EMPTY.
    -> ResamplePlan."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 3)
    B = int(sizes.shape[0])
    lo, hi = np.asarray(lo, dtype=np.int64).reshape(-1, 3), np.asarray(hi, dtype=np.int64).reshape(-1, 3)
    if lo.shape[0] != B or hi.shape[0] != B:
        raise ValueError("batch_resample_plan: %d sizes, %d lower bounds, %d upper bounds" % (B, lo.shape[0], hi.shape[0]))
    if (sizes < 1).any():
        raise ValueError("batch_resample_plan: a size below 1")
    old = _cm.batch_spacing(spacing, B)[:, ::-1]                       # (x, y, z) from here on, like resampleImage
    if not (old > 0).all():
        raise ValueError("batch_resample_plan: spacing must be > 0")
    new = np.asarray(resampledPixelSpacing, dtype=np.float64)
    if new.shape != (3,):
        raise AssertionError("Wrong dimensionality (%d-D) of resampledPixelSpacing!, 3-D required" % new.size)
    if (new < 0).any() or not np.isfinite(new).all():
        raise ValueError("batch_resample_plan: resampledPixelSpacing must be >= 0")
    pad = padDistance
    codes = _interpolator_codes(interpolator, B)
    empty = (hi < lo).any(1)
    if ((lo < 0) | (hi >= sizes))[~empty].any():
        raise ValueError("batch_resample_plan: a bounding box leaves its box")
    lo_z = np.where(empty[:, None], 0, lo)
    hi_z = np.where(empty[:, None], sizes - 1, hi)
    fullsize = sizes[:, ::-1]
    lo_x, size = lo_z[:, ::-1], (hi_z - lo_z + 1)[:, ::-1]
    new = np.where(new == 0, old, np.broadcast_to(new, (B, 3)))
    new = np.where(size != 1, new, old)
    crop = np.isclose(old, new).all(1) | empty                       # (np.allclose(old, new) per ROI)
    new = np.where(crop[:, None], old, new)
    ratio = old / new
    L = np.floor((lo_x - 0.5) * ratio - pad)
    U = np.ceil((lo_x + size - 0.5) * ratio + pad)
    maxU = np.ceil(fullsize * ratio) - 1
    L = np.where(L < 0, 0, L)
    U = np.where(U > maxU, maxU, U)
    newsize = np.array(U - L + 1, dtype=np.int64)
    start = 0.5 * (new - old) / old + L / ratio
    step = new / old
    # the plain crops: alignedBox over the batch (every ROI with the x extent of its own box)
    c_lo, c_hi = lo_z.copy(), hi_z.copy()
    need = (-(c_hi[:, 2] - c_lo[:, 2] + 1)) % 4 if alignCrop else np.zeros(B, dtype=np.int64)
    grow = np.minimum(need, sizes[:, 2] - 1 - c_hi[:, 2])
    c_hi[:, 2] += grow
    c_lo[:, 2] -= np.minimum(need - grow, c_lo[:, 2])
    c_lo, c_size = c_lo[:, ::-1], (c_hi - c_lo + 1)[:, ::-1]
    start = np.where(crop[:, None], c_lo.astype(np.float64), start)
    step = np.where(crop[:, None], 1.0, step)
    newsize = np.where(crop[:, None], c_size, newsize)
    zyx = lambda a, dt: np.ascontiguousarray(a[:, ::-1], dtype=dt)
    return ResamplePlan(zyx(start, np.float64), zyx(step, np.float64), zyx(newsize, np.intc),
                        np.where(crop, 0, codes).astype(np.intc), zyx(new, np.float64),
                        np.ascontiguousarray(old * start), np.where(empty, RESAMPLE_EMPTY, 0).astype(np.int64))


def _mask_boxes(rois):
    boxes = np.zeros((max(rois.B, 1), 7), dtype=np.intc)
    rc = rois.lib.prad_batch_mask_boxes_dev(_vp(rois.mask), _iptr(rois.sizes), _lp(rois.off), rois.B, _iptr(boxes),
                                            _eng._stream_ptr())
    _lib.raise_for(rc, "batched mask boxes")
    boxes = boxes[:rois.B].astype(np.int64)
    return boxes[:, 0:3].copy(), boxes[:, 3:6].copy(), boxes[:, 6].copy()


def mask_boxes_batch(masks, sizes=None):
    """The bounding boxes of B masks in ONE launch and one read-back of 28 B bytes.  masks: a list of 3-D device tensors, or a
    flat device tensor holding the boxes back to back plus `sizes` (int [B, 3]); non-zero = ROI.  -> (lo int64 [B, 3], hi int64
    [B, 3], count int64 [B]): inclusive (z, y, x) bounds and the voxels of every ROI, numpy arrays; an empty mask has count 0,
    lo = its sizes and hi = -1 (what batch_resample_plan reads as empty)."""
    if isinstance(masks, (list, tuple)):
        if not len(masks):
            raise ValueError("empty batch")
        if any(m.dim() != 3 for m in masks):
            raise ValueError("mask_boxes_batch takes 3-D boxes")
        sizes = np.array([tuple(m.shape) for m in masks], dtype=np.intc).reshape(-1, 3)
        masks = torch.cat([(m if m.dtype in (torch.bool, torch.uint8) else m != 0).reshape(-1).view(torch.uint8) for m in masks])
    elif sizes is None:
        raise ValueError("a flat mask tensor needs `sizes`")
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    masks = masks.reshape(-1)
    if not masks.is_cuda:
        raise ValueError("engine.* expects CUDA/HIP tensors; use pyradiomics_amd.cmatrices for numpy input")
    masks = _eng._mask_u8(masks)
    nvox = sizes.astype(np.int64).prod(1)
    if not len(nvox) or int(nvox.sum()) != masks.numel():
        raise ValueError("sizes describe %d voxels, the buffer holds %d" % (int(nvox.sum()), masks.numel()))
    lib = _lib.load()
    _set_device(lib, masks.device)
    return _mask_boxes(RoiBatch(lib, None, masks, sizes, nvox, _offsets(nvox), masks.device))


def _geometry(a, B, dtype, what):
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    if a.shape != (B, 3):
        raise ValueError("%s must be an array [%d, 3]" % (what, B))
    return a


def _resample_boxes(rois, start, step, newsize, codes, out, out_masks):
    """the geometry has been checked; rois.mask may be None -> (images, masks or None, verdict)"""
    B = rois.B
    nout = newsize.astype(np.int64).prod(1)
    out_off, W = _offsets(nout), int(nout.sum())

    def buffer(given, dtype, what):
        if given is None:
            return torch.empty(W, dtype=dtype, device=rois.device)
        if given.dtype != dtype or given.device != rois.device or given.dim() != 1 or given.numel() < W or not given.is_contiguous():
            raise ValueError("%s must be a contiguous flat %s tensor of at least %d elements on %s" % (what, dtype, W, rois.device))
        return given
    out = buffer(out, rois.data.dtype, "out")
    if rois.mask is not None:
        out_masks = buffer(out_masks, torch.uint8, "out_masks")
    elif out_masks is not None:
        raise ValueError("out_masks without masks")
    verdict = np.zeros(max(B, 1), dtype=np.intc)
    dp = lambda a: C.c_void_p(a.ctypes.data)
    rc = rois.lib.prad_batch_resample_dev(_vp(rois.data), _eng._DTYPE_CODES[rois.data.dtype], _vp(rois.mask), _iptr(rois.sizes),
                                          _lp(rois.off), B, dp(start), dp(step), _iptr(newsize), _iptr(codes), _lp(out_off),
                                          _vp(out), _vp(out_masks), _iptr(verdict), _eng._stream_ptr())
    _lib.raise_for(rc, "batched resampling")
    verdict = verdict[:B]
    rest = np.flatnonzero(verdict != 0)
    for b in rest:                # boxes above batch_resample_max_vox(): the single route, into the same layout
        o, n = int(out_off[b]), int(nout[b])
        out[o:o + n] = _eng.resample(rois.view(rois.data, b), start[b], step[b], newsize[b], int(codes[b])).reshape(-1)
        if rois.mask is not None:
            m = _eng.resample(rois.view(rois.mask, b).to(torch.int16), start[b], step[b], newsize[b], 0)
            out_masks[o:o + n] = m.reshape(-1).to(torch.uint8)
    _cm._set_batch_route(_route(len(rest), B))
    return out, out_masks, verdict


def resample_boxes_batch(images, sizes, start, step, newsize, interpolator=3, masks=None, out=None, out_masks=None,
                         return_verdict=False):
    """A batch of engine.resample: box b of the batch is resampled ALONE -- output voxel o along axis d reads the box at the
    continuous index start[b][d] + o * step[b][d] -- bit for bit what engine.resample(box, start[b], step[b], newsize[b],
    interpolator[b]) returns, in at most TWO launches whatever B is (the B-spline prefilter of all boxes, one workgroup per box;
    the evaluation, divided by output voxels).  images: a list of 3-D device tensors of one dtype (float32, float64, int32,
    int16; anything else is widened to float64), or a flat device tensor plus `sizes` int [B, 3]; start / step float [B, 3],
    newsize int [B, 3], all (z, y, x); interpolator: 0 nearest, 1 linear, 3 cubic B-spline, an int or [B]; masks (optional): the
    uint8 masks in the same layout, resampled nearest-neighbour on the same grids in the same launch.  -> (images, masks or None):
    flat device tensors in the batch layout of `newsize`, which every *_batch function takes as they are.  out / out_masks:
    preallocated flat tensors (at least sum(prod(newsize)) elements) to fill instead; elements behind the last ROI are not
    touched.  Native: boxes of at most batch_resample_max_vox() voxels, output voxels uncapped; the others are filled from
    engine.resample one by one (return_verdict=True appends the verdicts, intc [B]: 0 native, 8 single route).
    last_batch_route() says "batch", "mixed" or "looped".  The coefficients of the cubic B-spline
    are those of the box: a recursive prefilter has unbounded support, so a box cut out of a larger scan does not resample to
    the values of the resampled scan."""
    rois = _image_batch(images, sizes) if masks is None else _roi_batch(images, masks, sizes, raw=True)
    B = rois.B
    codes = np.ascontiguousarray(np.broadcast_to(np.asarray(interpolator, dtype=np.intc), (B,)))
    if not np.isin(codes, (0, 1, 3)).all():
        raise NotImplementedError("resample_boxes_batch: interpolator codes are 0 nearest, 1 linear, 3 cubic B-spline")
    start, step = _geometry(start, B, np.float64, "start"), _geometry(step, B, np.float64, "step")
    newsize = _geometry(newsize, B, np.intc, "newsize")
    if (newsize < 1).any():
        raise ValueError("resample_boxes_batch: a newsize below 1")
    res = _resample_boxes(rois, start, step, newsize, codes, out, out_masks)
    return res if return_verdict else res[:2]


def resample_batch(images, masks, sizes=None, spacing=(1.0, 1.0, 1.0), resampledPixelSpacing=None, interpolator="sitkBSpline",
                   padDistance=5, alignCrop=True):
    """imageoperations.resampleImage on each of B boxes as if the box were the whole image -- what
    RadiomicsFeatureExtractor.execute does when it is handed the box as its image --, bit for bit, in THREE launches and one
    read-back whatever B is: mask_boxes_batch (the bounding boxes, the only read-back), batch_resample_plan (host arithmetic),
    resample_boxes_batch (prefilter, evaluation; image and mask together).  images / masks / sizes: as roi_features_batch takes
    them; spacing (z, y, x), one triple or [B, 3]; resampledPixelSpacing (x, y, z) as in a parameter file, 0 keeps an axis;
    interpolator: a name or code resampleImage accepts (NotImplementedError for any other), for the image -- the mask is always
    nearest-neighbour; padDistance: voxels of the new grid kept around the bounding box.
    -> (images, masks, sizes int32 [B, 3], spacing float64 [B, 3] (z, y, x), origin_shift float64 [B, 3] (x, y, z): what to add
    to the box's origin along its axes, status int64 [B]): flat batch tensors on the new grids that every *_batch function
    takes as they are.  A ROI whose spacing does not change is cropped (batch_resample_plan), one with an empty mask keeps its
    box and has status RESAMPLE_EMPTY (resampleImage raises there); the others have status 0.  alignCrop=False: a cropped ROI
    keeps the bounding box's own x extent, as resampleImage's crop does, instead of one grown to a multiple of four.
    The resampled values are those of the box ALONE: the B-spline prefilter has unbounded support, so -- like the LoG of
    roi_features_batch_derived -- they are not those of the resampled scan the box was cut from, however wide its margin.
    Boxes above batch_resample_max_vox() voxels go through engine.resample; last_batch_route() says "batch", "mixed" or
    "looped"."""
    if resampledPixelSpacing is None:
        raise ValueError("resample_batch needs resampledPixelSpacing")
    rois = _roi_batch(images, masks, sizes, raw=True)
    _interpolator_codes(interpolator, rois.B)                    # (raises before anything is launched)
    lo, hi, _ = _mask_boxes(rois)
    plan = batch_resample_plan(rois.sizes, lo, hi, spacing, resampledPixelSpacing, padDistance, interpolator, alignCrop)
    out, out_masks, _ = _resample_boxes(rois, plan.start, plan.step, plan.newsize, plan.interpolator, None, None)
    return out, out_masks, plan.newsize, plan.spacing, plan.origin_shift, plan.status


def roi_features_batch_resampled(images, masks, sizes=None, spacing=(1.0, 1.0, 1.0), resampledPixelSpacing=None,
                                 interpolator="sitkBSpline", padDistance=5, imageTypes=None, classes=ROI_FEATURE_CLASSES,
                                 **settings):
    """resample_batch, then roi_features_batch_derived on the resampled boxes: the feature table of B lesions handed over as raw
    boxes with their own spacing under a parameter file that sets resampledPixelSpacing -- per ROI what
    RadiomicsFeatureExtractor.execute(box, mask) computes with those settings and no preCrop.  The new spacing of every ROI goes
    on as `spacing` (LoG, weightingNorm) and its product as voxelVolume.  As for the LoG, the values are those of the box ALONE
    (resample_batch).  A ROI whose spacing does not change is cut to its bounding box as resampleImage cuts it (alignCrop=False):
    a filter sees the crop's own borders, and on a crop one to three columns wider the LoG of every ROI voxel differs.  A ROI
    whose mask is empty -- before or after resampling -- has status 0 and NaN rows (the extractor raises there).  imageTypes / classes / **settings / -> : as roi_features_batch_derived; last_batch_route() joins all calls."""
    if "voxelVolume" in settings:
        raise ValueError("roi_features_batch_resampled works out voxelVolume itself")
    out, out_masks, newsize, new_spacing, _, _ = resample_batch(images, masks, sizes, spacing, resampledPixelSpacing, interpolator,
                                                                padDistance, alignCrop=False)
    route = last_batch_route()
    tables, status = roi_features_batch_derived(out, out_masks, newsize, imageTypes, classes, spacing=new_spacing,
                                                voxelVolume=new_spacing[:, 2] * new_spacing[:, 1] * new_spacing[:, 0],
                                                **settings)          # ((x * y) * z, the order of the feature class)
    _cm._set_batch_route(_joined_route([route, last_batch_route()]))
    return tables, status


# ---- resegmentation of the boxes, each by its own thresholds (prad_batch_resegment_dev, csrc/kernels_batch_resegment.h) -------
RESEGMENT_EMPTY = 1        # status of a ROI that is empty on entry
RESEGMENT_TOO_FEW = 3      # status of a ROI of which at most one voxel is kept (resegmentMask raises there); boxes holds the count


def _resegment_host(rois, b, rng, modename, out, boxes, thr):
    """ROI b through the host arithmetic (imageoperations.resegmentArrays), into the same layout -> its status"""
    from . import imageoperations
    im = rois.view(rois.data, b).cpu().numpy()
    roi = rois.view(rois.mask, b).cpu().numpy() != 0
    shape = np.array(roi.shape, dtype=np.int64)
    boxes[b] = np.concatenate([shape, [-1, -1, -1, 0]])
    thr[b] = 0.0
    if not roi.any():
        rois.view(out, b).zero_()
        return RESEGMENT_EMPTY
    with np.errstate(all="ignore"):
        kept, t = imageoperations.resegmentArrays(im, roi, rng, modename)
    rois.view(out, b).copy_(torch.from_numpy(kept.astype(np.uint8)).to(rois.device))
    compare = np.float32 if im.dtype == np.float32 else np.float64
    with np.errstate(all="ignore"):
        thr[b] = [float(compare(t[0])), float(compare(t[1])) if len(t) == 2 else np.inf]
    n = int(kept.sum())
    if n:
        idx = np.nonzero(kept)
        boxes[b] = [i.min() for i in idx] + [i.max() for i in idx] + [n]
    return 0 if n > 1 else RESEGMENT_TOO_FEW


def _resegment(rois, resegmentRange, resegmentMode):
    """-> (flat uint8 masks, boxes int64 [B, 7], thresholds float64 [B, 2], status int64 [B])"""
    mode, rng = _eng._resegment_args(resegmentRange, resegmentMode)
    B = rois.B
    out = torch.empty_like(rois.mask)
    boxes = np.zeros((max(B, 1), 7), dtype=np.intc)
    thr = np.zeros((max(B, 1), 2), dtype=np.float64)
    verdict = np.zeros(max(B, 1), dtype=np.intc)
    try:
        t = _eng._resegment_numbers(rng, mode, not rois.data.dtype.is_floating_point)
    except NotImplementedError:      # thresholds whose host arithmetic the kernel does not reproduce: every ROI on the host
        verdict[:] = 8
    else:
        dp = C.POINTER(C.c_double)
        rc = rois.lib.prad_batch_resegment_dev(_vp(rois.data), _eng._DTYPE_CODES[rois.data.dtype], _vp(rois.mask), _iptr(rois.sizes),
                                               _lp(rois.off), B, mode, t.ctypes.data_as(dp), len(t), _vp(out), _iptr(boxes),
                                               thr.ctypes.data_as(dp), _iptr(verdict), _eng._stream_ptr())
        _lib.raise_for(rc, "batched resegmentation")
    boxes, thr, status = boxes[:B].astype(np.int64), thr[:B], verdict[:B].astype(np.int64)
    rest = np.flatnonzero((status == 2) | (status == 8))
    for b in rest:
        status[b] = _resegment_host(rois, b, rng, resegmentMode, out, boxes, thr)
    _cm._set_batch_route(_route(len(rest), B))
    return out, boxes, thr, status


def resegment_batch(images, masks, sizes=None, resegmentRange=None, resegmentMode="absolute"):
    """imageoperations.resegmentMask on each of B boxes in ONE launch and one read-back: every ROI is restricted to its voxels
    inside `resegmentRange` (one threshold: >= t; two: the closed range), taken absolutely, relative to the ROI's own maximum
    or in standard deviations about the ROI's own mean ("absolute", "relative", "sigma").  images / masks / sizes: as
    firstorder_batch takes them.  -> (masks: flat uint8 device tensor in the batch layout, 1 in the kept ROI; boxes int64 [B, 7]:
    lo z / y / x, hi z / y / x and the voxel count of the KEPT ROI, mask_boxes_batch's layout; thresholds float64 [B, 2], [1] =
    inf with one bound; status int64 [B]: 0 fine, RESEGMENT_EMPTY (1) the ROI was empty on entry, RESEGMENT_TOO_FEW (3) at most
    one voxel is kept -- a status where resegmentMask raises, not an exception).  Every mask equals the host function's voxel
    for voxel.  ROIs the launch does not serve -- a non-finite value inside the ROI, a box above batch_max_vox() voxels, sigma
    mode on float32 boxes (numpy's float32 mean) -- go through the host arithmetic one by one, into the same layout;
    last_batch_route() says "batch", "mixed" or "looped".  Raises resegmentMask's ValueErrors for a range of None, of length 0 or
    above 2, and an unknown mode, before any device is asked."""
    _eng._resegment_args(resegmentRange, resegmentMode)
    return _resegment(_roi_batch(images, masks, sizes, raw=True), resegmentRange, resegmentMode)


def _resegment_settings(settings):
    """pops resegmentRange / resegmentMode off `settings` and checks them (resegmentMask's ValueErrors, before any device is
    asked) -> (range, mode), or None without a range"""
    rng, mode = settings.pop("resegmentRange", None), settings.pop("resegmentMode", "absolute")
    if rng is None:
        return None
    _eng._resegment_args(rng, mode)
    return rng, mode


def _resegmented(rois, spec):
    """the composite calls' resegmentation step -> (rois with the new masks -- all zeros for a ROI that fails, which the feature
    calls then report as they report an empty ROI --, the step's route or None)"""
    if spec is None:
        return rois, None
    out, _boxes, _thr, status = _resegment(rois, *spec)
    for b in np.flatnonzero(status == RESEGMENT_TOO_FEW):
        rois.view(out, b).zero_()
    return rois._replace(mask=out), last_batch_route()


# ---- the boxes of many labels of one label map in the batch layout (prad_batch_gather_dev, csrc/kernels_batch_gather.h) -------
def gather_rois_batch(image, labelmap, labels, lo, hi, masks=True, images=True):
    """The boxes of B labels cut out of one 3-D volume in ONE launch, packed the way the *_batch functions take raw images.
    image / labelmap: device tensors of one shape (either may be None when its output is not asked for); labels int [B]; lo / hi
    int [B, 3]: inclusive (z, y, x) bounds, as label_census returns them (boxes may overlap).  -> (flat image tensor, flat uint8
    mask tensor, sizes int32 [B, 3]); the mask of ROI b is labelmap == labels[b] inside its box, the image keeps its dtype where
    it is one of the four the batched kernels read (float32, float64, int32, int16; anything else is widened to float64) and
    its values bit for bit.  masks=False / images=False leave that output None.  The label map is narrowed as label_census
    narrows it.  A box that leaves the volume, hi < lo or tensors on two devices raise ValueError before anything is launched.
    No read-back and no host synchronisation; the table of boxes stays on the device while consecutive calls repeat it."""
    lib = _lib.load()
    if not masks and not images:
        raise ValueError("gather_rois_batch: neither masks nor images asked for")
    ref = image if images else labelmap
    if (images and image is None) or (masks and labelmap is None):
        raise ValueError("gather_rois_batch: the %s is missing" % ("image" if images and image is None else "label map"))
    if not ref.is_cuda:
        raise ValueError("engine.gather_rois_batch expects CUDA/HIP tensors")
    if images and masks and (not labelmap.is_cuda or image.device != labelmap.device):
        raise ValueError("gather_rois_batch: image on %s, label map on %s" % (image.device, labelmap.device))
    if ref.dim() != 3 or (images and masks and image.shape != labelmap.shape):
        raise ValueError("gather_rois_batch takes a 3-D image and a label map of the same shape")
    lo = np.ascontiguousarray(np.asarray(lo, dtype=np.int64).reshape(-1, 3))
    hi = np.ascontiguousarray(np.asarray(hi, dtype=np.int64).reshape(-1, 3))
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    B = int(lo.shape[0])
    if B < 1 or hi.shape[0] != B or labels.shape[0] != B:
        raise ValueError("gather_rois_batch: %d lower bounds, %d upper bounds, %d labels" % (B, hi.shape[0], labels.shape[0]))
    if (hi < lo).any():
        raise ValueError("gather_rois_batch: ROI %d has hi < lo" % int(np.flatnonzero((hi < lo).any(1))[0]))
    if (lo < 0).any() or (hi >= np.asarray(ref.shape, dtype=np.int64)).any():
        raise ValueError("gather_rois_batch: ROI %d leaves the volume %s"
                         % (int(np.flatnonzero(((lo < 0) | (hi >= np.asarray(ref.shape))).any(1))[0]), tuple(ref.shape)))
    if (labels > 2**31 - 1).any() or (labels < -2**31).any():
        raise ValueError("gather_rois_batch: labels outside the int32 range")
    if images:
        image = (image if image.dtype in _eng._DTYPE_CODES else image.to(torch.float64)).contiguous()
    if masks:
        labelmap = _eng._label_tensor(labelmap, "gather rois batch")
    sizes = np.ascontiguousarray((hi - lo + 1).astype(np.intc))
    nvox = sizes.astype(np.int64).prod(1)
    total = int(nvox.sum())
    dev = ref.device
    _set_device(lib, dev)
    out_i = torch.empty(total, dtype=image.dtype, device=dev) if images else None
    out_m = torch.empty(total, dtype=torch.uint8, device=dev) if masks else None
    size = np.array(ref.shape, dtype=np.intc)
    lo32, lab32 = np.ascontiguousarray(lo.astype(np.intc)), np.ascontiguousarray(labels.astype(np.intc))
    rc = lib.prad_batch_gather_dev(_vp(image) if images else None, _eng._DTYPE_CODES[image.dtype] if images else 0,
                                   _vp(labelmap) if masks else None, _eng._LABEL_CODES[labelmap.dtype] if masks else 0,
                                   _iptr(size), B, _iptr(lab32), _iptr(lo32), _iptr(sizes), _lp(_offsets(nvox)), _vp(out_i),
                                   _vp(out_m), _eng._stream_ptr())
    _lib.raise_for(rc, "batched ROI gather")
    return out_i, out_m, sizes


# (last: engine binds the public names above at its own end, so either module may be the first to be imported)
from . import engine as _eng  # noqa: E402  the single calls the looped routes use

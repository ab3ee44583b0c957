"""Drop-in for the reference's native operator module `radiomics._cmatrices`
(bound as `radiomics.cMatrices`, radiomics/__init__.py:343-349).

Same six functions, same positional signatures, same dtype coercions, output shapes/dtypes and exception
types as radiomics/src/_cmatrices.c -- but every matrix is built on the MI355X through the C ABI of
include/pyradiomics_amd.h (ctypes).  A reference checkout switches over with

    import radiomics, pyradiomics_amd.cmatrices
    radiomics.cMatrices = pyradiomics_amd.cmatrices          # the one line at radiomics/__init__.py:348

Inputs are numpy arrays (host) as in the reference.  In segment mode the same functions also accept torch tensors
that already live in HBM (`DEVICE_TENSORS`): nothing is staged through the host and only the finished matrix comes
back as numpy, which is how pyradiomics_amd's own feature classes call them (pyradiomics_amd/base.py).  The
lower-level device-resident entry points live in pyradiomics_amd.engine.
"""
from __future__ import annotations

import sys as _sys

import ctypes as C

import os

import numpy as np

from . import _lib

_ip = C.POINTER(C.c_int)

def _engine():
    """the device engine (imports torch), loaded on first use: a function-level `from . import engine` goes through
    importlib's locked lookup on every call (11 us each, 54 of them per 256^3 case); sys.modules is a dict lookup"""
    m = _sys.modules.get("pyradiomics_amd.engine")
    if m is None:
        from . import engine as m
    return m


DEVICE_TENSORS = True     # calculate_* accept device tensors in segment mode (checked by pyradiomics_amd.base)


def _on_device(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _memo(image, mask):
    """per-levels-tensor memo used to serve GLCM and GLRLM from one fused sweep; only active on tensors that
    pyradiomics_amd.base tagged (`_prad_memo`), keyed by the mask they were tagged with"""
    memo = getattr(image, "_prad_memo", None)
    if memo is None or memo.get("mask") is not mask:
        return None
    return memo


class _PairsRuns(dict):
    """{"glcm_dev", "glrlm_dev", "angles"} + the host copies "glcm" / "glrlm" ([1, Ng, ., Na], the reference's layout),
    made when somebody asks (the fused segment route never does: a 256^3 GLRLM is 0.8 MB per derived image)"""

    def __missing__(self, key):
        if key in ("glcm", "glrlm"):
            dev = self[key + "_dev"]
            val = None if dev is None else dev.cpu().numpy()[None]
            self[key] = val
            return val
        raise KeyError(key)


def _dev_pairs_runs(image, mask, Ng, force2D, force2Ddimension, want, deferred=False):
    """distance-1 GLCM / GLRLM of device tensors through the fused sweep.  deferred=True: the kernels are only enqueued
    on the current stream (engine.glcm_glrlm(deferred=True) + deferred_join); engine.deferred_status() tells afterwards
    whether the levels were inside [1, Ng]"""
    engine = _engine()
    f2d = int(force2Ddimension) if force2D else -1
    Nr = int(max(image.shape))
    memo = _memo(image, mask)
    key = ("pairs_runs", int(Ng), f2d)
    if memo is not None and key in memo:
        return memo[key]
    both = memo is not None
    g, r, angles = engine.glcm_glrlm(image, mask, int(Ng), Nr, force2D, force2Ddimension,
                                     want_glcm=both or want == "glcm", want_glrlm=both or want == "glrlm",
                                     deferred=deferred)
    if deferred:
        engine.deferred_join()          # (pipeline mode: the walk of this volume is launched now, not by the next call)
    res = _PairsRuns({"angles": angles, "glcm_dev": g, "glrlm_dev": r})
    if memo is not None:
        memo[key] = res
    return res


def _dev_gldm_ngtdm(image, mask, Ng, alpha, dist, force2D, force2Ddimension, deferred):
    """(GLDM, NGTDM) device matrices of a segment.  On tensors pyradiomics_amd.base tagged (all feature classes of one
    derived image share them) both come from ONE pass over the neighbourhoods (engine.gldm_ngtdm) and are kept for the
    other class; alpha = None: the caller only wants NGTDM (the fused pass runs with the default alpha 0)"""
    engine = _engine()
    f2d = int(force2Ddimension) if force2D else -1
    memo = _memo(image, mask)
    a = 0 if alpha is None else int(alpha)
    key = ("gldm_ngtdm", int(Ng), f2d, tuple(dist), a)
    if memo is not None and not os.environ.get("PRAD_NO_FUSED_NEIGH"):
        for k, v in memo.items():          # NGTDM does not depend on alpha: any fused result of this geometry serves it
            if isinstance(k, tuple) and k[:4] == key[:4] and (alpha is None or k[4] == a):
                return v
        res = engine.gldm_ngtdm(image, mask, int(Ng), a, dist, force2D, force2Ddimension, deferred=deferred)
        memo[key] = res
        return res
    if alpha is None:
        return None, engine.ngtdm(image, mask, int(Ng), dist, force2D, force2Ddimension, deferred=deferred)
    return engine.gldm(image, mask, int(Ng), a, dist, force2D, force2Ddimension, deferred=deferred), None


def _iptr(a):
    return a.ctypes.data_as(_ip)


def _vptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _parse_arrays(image, mask):
    """_cmatrices.c:1023-1085 (try_parse_arrays): int32 / bool, C-contiguous, equal rank and shape."""
    img = np.ascontiguousarray(np.asarray(image).astype(np.intc, copy=False))
    msk = np.asarray(mask)
    if msk.dtype in (np.uint8, np.int8):
        msk = np.ascontiguousarray(msk).view(np.uint8)     # one byte per voxel already, the kernels test != 0: no copy
    else:
        msk = np.ascontiguousarray(msk.astype(np.bool_, copy=False))
    if img.ndim != msk.ndim:
        raise ValueError("Expected image and mask to have equal number of dimensions.")
    if img.shape != msk.shape:
        raise ValueError("Dimensions of image and mask do not match.")
    size = np.array(img.shape, dtype=np.intc)
    return img, msk, size


def _parse_voxels(voxels, Nd, kernelRadius):
    """_cmatrices.c:1087-1118 (try_parse_voxels_arr)."""
    if voxels is None:
        return None, 1
    if kernelRadius <= 0:
        raise RuntimeError("Expecting kernelRadius > 0")
    v = np.ascontiguousarray(np.asarray(voxels).astype(np.intc, copy=False))
    if v.ndim != 2 or v.shape[0] != Nd:
        raise RuntimeError("Expecting voxel indices array to be 2-dimensional")
    return v, int(v.shape[1])


_angle_memo: dict = {}


def _build_angles(size, distances, bidirectional, force2Ddim):
    """_cmatrices.c:926-1021 (build_angles_arr) on prad_get_angle_count / prad_build_angles."""
    lib = _lib.load()
    if distances is None:
        dist = np.array([1], dtype=np.intc)
    else:
        try:
            dist = np.ascontiguousarray(np.asarray(distances).astype(np.intc, copy=False))
        except (TypeError, ValueError):
            raise RuntimeError("Error parsing distances array.")
        if dist.ndim != 1:
            raise ValueError("Expecting distances array to be 1-dimensional.")
    Nd = int(size.shape[0])
    key = (size.tobytes(), dist.tobytes(), bool(bidirectional), int(force2Ddim))
    hit = _angle_memo.get(key)         # (27 calls per case with 5 distinct answers; the table is never written to)
    if hit is not None:
        return hit
    Na = lib.prad_get_angle_count(_iptr(size), _iptr(dist), Nd, int(dist.shape[0]), int(bool(bidirectional)),
                                  int(force2Ddim)) if dist.shape[0] > 0 else 0
    if Na == 0:
        raise RuntimeError("Error getting angle count.")
    angles = np.empty((Na, Nd), dtype=np.intc)
    if lib.prad_build_angles(_iptr(size), _iptr(dist), Nd, int(dist.shape[0]), int(force2Ddim), Na, _iptr(angles)) > 0:
        raise RuntimeError("Error building angles.")
    angles.setflags(write=False)
    if len(_angle_memo) > 256:
        _angle_memo.clear()
    _angle_memo[key] = angles
    return angles


def _common(image, mask, distances, bidirectional, force2D, force2Ddimension, kernelRadius, voxels):
    img, msk, size = _parse_arrays(image, mask)
    vox, Nvox = _parse_voxels(voxels, img.ndim, kernelRadius)
    f2d = int(force2Ddimension) if force2D else -1
    angles = _build_angles(size, distances, bidirectional, f2d)
    return img, msk, size, vox, Nvox, f2d, angles


def calculate_glcm(image, mask, distances, Ng, force2D, force2Ddimension, kernelRadius=0, voxels=None):
    """-> (P float64 [Nvox, Ng, Ng, Na], angles int32 [Na, Nd]);  _cmatrices.c:84-233"""
    if _on_device(image) and voxels is None:
        engine = _engine()
        dist = [int(d) for d in np.asarray(distances).ravel()]
        if dist == [1]:
            res = _dev_pairs_runs(image, mask, Ng, force2D, force2Ddimension, "glcm")
            return res["glcm"], res["angles"]
        P, angles = engine.glcm(image, mask, int(Ng), dist, force2D, force2Ddimension)
        return P.cpu().numpy()[None], angles
    img, msk, size, vox, Nvox, f2d, angles = _common(image, mask, distances, False, force2D, force2Ddimension,
                                                     kernelRadius, voxels)
    Na, Nd = angles.shape
    out = np.empty((Nvox, Ng, Ng, Na), dtype=np.float64)
    rc = _lib.load().prad_calculate_glcm(_vptr(img), _vptr(msk), _iptr(size), Nd, _iptr(angles), Na, int(Ng),
                                         Nvox, _vptr(vox), int(kernelRadius), f2d, _vptr(out))
    _lib.raise_for(rc, "GLCM")
    return out, angles


def calculate_glrlm(image, mask, Ng, Nr, force2D, force2Ddimension, kernelRadius=0, voxels=None):
    """-> (P float64 [Nvox, Ng, Nr, Na], angles);  _cmatrices.c:432-581 (distances fixed to [1])"""
    if _on_device(image) and voxels is None:
        if int(Nr) == int(max(image.shape)):
            res = _dev_pairs_runs(image, mask, Ng, force2D, force2Ddimension, "glrlm")
            return res["glrlm"], res["angles"]
        engine = _engine()
        _, r, angles = engine.glcm_glrlm(image, mask, int(Ng), int(Nr), force2D, force2Ddimension, want_glcm=False)
        return r.cpu().numpy()[None], angles
    img, msk, size, vox, Nvox, f2d, angles = _common(image, mask, None, False, force2D, force2Ddimension,
                                                     kernelRadius, voxels)
    Na, Nd = angles.shape
    out = np.empty((Nvox, Ng, Nr, Na), dtype=np.float64)
    rc = _lib.load().prad_calculate_glrlm(_vptr(img), _vptr(msk), _iptr(size), Nd, _iptr(angles), Na, int(Ng),
                                          int(Nr), Nvox, _vptr(vox), int(kernelRadius), f2d, _vptr(out))
    _lib.raise_for(rc, "GLRLM")
    return out, angles


def calculate_glcm_glrlm(image, mask, Ng, Nr, force2D, force2Ddimension, kernelRadius=0, voxels=None):
    """Both matrices for distance 1 from one pack + one sweep per angle (no reference analogue; results equal
    calculate_glcm(..., [1], ...) and calculate_glrlm(...)).  -> (P_glcm, P_glrlm, angles)"""
    img, msk, size, vox, Nvox, f2d, angles = _common(image, mask, None, False, force2D, force2Ddimension,
                                                     kernelRadius, voxels)
    Na, Nd = angles.shape
    glcm = np.empty((Nvox, Ng, Ng, Na), dtype=np.float64)
    glrlm = np.empty((Nvox, Ng, Nr, Na), dtype=np.float64)
    rc = _lib.load().prad_calculate_glcm_glrlm(_vptr(img), _vptr(msk), _iptr(size), Nd, _iptr(angles), Na, int(Ng),
                                               int(Nr), Nvox, _vptr(vox), int(kernelRadius), f2d, _vptr(glcm),
                                               _vptr(glrlm))
    _lib.raise_for(rc, "GLCM+GLRLM")
    return glcm, glrlm, angles


def calculate_gldm(image, mask, distances, Ng, alpha, force2D, force2Ddimension, kernelRadius=0, voxels=None):
    """-> P float64 [Nvox, Ng, 2*Na+1] (Na = bidirectional angle count);  _cmatrices.c:731-880"""
    if _on_device(image) and voxels is None:
        engine = _engine()
        return engine.gldm(image, mask, int(Ng), int(alpha), [int(d) for d in np.asarray(distances).ravel()], force2D,
                           force2Ddimension).cpu().numpy()[None]
    img, msk, size, vox, Nvox, f2d, angles = _common(image, mask, distances, True, force2D, force2Ddimension,
                                                     kernelRadius, voxels)
    Na, Nd = angles.shape
    out = np.empty((Nvox, Ng, 2 * Na + 1), dtype=np.float64)
    rc = _lib.load().prad_calculate_gldm(_vptr(img), _vptr(msk), _iptr(size), Nd, _iptr(angles), Na, int(Ng),
                                         int(alpha), Nvox, _vptr(vox), int(kernelRadius), f2d, _vptr(out))
    _lib.raise_for(rc, "GLDM")
    return out


def calculate_ngtdm(image, mask, distances, Ng, force2D, force2Ddimension, kernelRadius=0, voxels=None):
    """-> P float64 [Nvox, Ng, 3];  _cmatrices.c:583-729"""
    if _on_device(image) and voxels is None:
        engine = _engine()
        return engine.ngtdm(image, mask, int(Ng), [int(d) for d in np.asarray(distances).ravel()], force2D,
                            force2Ddimension).cpu().numpy()[None]
    img, msk, size, vox, Nvox, f2d, angles = _common(image, mask, distances, True, force2D, force2Ddimension,
                                                     kernelRadius, voxels)
    Na, Nd = angles.shape
    out = np.empty((Nvox, Ng, 3), dtype=np.float64)
    rc = _lib.load().prad_calculate_ngtdm(_vptr(img), _vptr(msk), _iptr(size), Nd, _iptr(angles), Na, int(Ng),
                                          Nvox, _vptr(vox), int(kernelRadius), f2d, _vptr(out))
    _lib.raise_for(rc, "NGTDM")
    return out


def calculate_glszm(image, mask, Ng, Ns, force2D, force2Ddimension, kernelRadius=0, voxels=None):
    """-> P float64 [Nvox, Ng, maxRegion], last axis cropped to the largest zone found (>= 1);
    _cmatrices.c:235-430.  The input mask is not modified (the reference works on a private copy)."""
    if _on_device(image) and voxels is None:
        engine = _engine()
        return engine.glszm(image, mask, int(Ng), int(Ns), force2D, force2Ddimension).cpu().numpy()[None]
    img, msk, size, vox, Nvox, f2d, angles = _common(image, mask, None, True, force2D, force2Ddimension,
                                                     kernelRadius, voxels)
    Na, Nd = angles.shape
    lib = _lib.load()
    nz = C.c_longlong(0)
    rc = lib.prad_calculate_glszm(_vptr(img), _vptr(msk), _iptr(size), Nd, _iptr(angles), Na, int(Ng), int(Ns),
                                  Nvox, _vptr(vox), int(kernelRadius), f2d, C.byref(nz))
    if rc == _lib.PRAD_E_INDEX:
        raise IndexError("Calculation of GLSZM Failed.")   # _cmatrices.c:372
    if rc < 0:
        _lib.raise_for(rc, "GLSZM")
    maxRegion = max(int(rc), 1)   # _cmatrices.c:390
    out = np.empty((Nvox, Ng, maxRegion), dtype=np.float64)
    rc = lib.prad_fill_glszm(_vptr(out), Nvox, int(Ng), maxRegion)
    if rc == _lib.PRAD_INDEX_ERROR:
        raise IndexError("Error filling GLSZM.")
    _lib.raise_for(rc, "GLSZM")
    return out


def calculate_glszm_compact(image, mask, Ng, Ns, force2D, force2Ddimension):
    """Segment-mode GLSZM with the all-zero size columns left out (no reference analogue at this boundary; it is
    the matrix glszm.py:118-131 ends up with).  -> (P float64 [1, Ng, k], sizes int32 [k] ascending).
    Host arrays are uploaded; device tensors are used in place."""
    import torch
    engine = _engine()
    if not _on_device(image):
        img, msk, _ = _parse_arrays(image, mask)
        dev = torch.device("cuda", torch.cuda.current_device())
        image, mask = torch.from_numpy(img).to(dev), torch.from_numpy(msk).to(dev)
    P, sizes = engine.glszm_compact(image, mask, int(Ng), int(Ns), force2D, force2Ddimension)
    return P.cpu().numpy()[None], sizes


# ---- many small ROIs, one launch (prad_batch_plan / prad_calculate_batch_dev; no reference analogue) --------
BATCH_FAMILIES = ("glcm", "glrlm", "gldm", "ngtdm")      # bit f of the C `families` argument, row f of the offsets
_batch_route = "none"


def last_batch_route() -> str:
    """which route served the last *_batch call: "batch" (the native launch), "looped" (the single calls, ROI by ROI) or, for
    the GLSZM batch, "mixed" (ROIs outside the native domain looped, the others batched)"""
    return _batch_route


def _set_batch_route(route: str) -> None:
    global _batch_route
    _batch_route = route


def batch_family_bits(families) -> int:
    unknown = [f for f in families if f not in BATCH_FAMILIES]
    if unknown or not families:
        raise ValueError("families must be a non-empty subset of %s" % (BATCH_FAMILIES,))
    return sum(1 << BATCH_FAMILIES.index(f) for f in set(families))


def batch_forced_dim(force2D, force2Ddimension) -> int:
    """the C `force2Ddim` of the batched calls: -1 without force2D, else the axis (0 z, 1 y, 2 x) no angle may leave"""
    if not force2D:
        return -1
    d = int(force2Ddimension)
    if not 0 <= d <= 2:
        raise ValueError("force2Ddimension must be 0, 1 or 2 for 3-D ROIs, got %r" % (force2Ddimension,))
    return d


# the entry points that take `int Ng` -> their twins that take a host vector `const int *Ng` [B]
_NG_TWIN = {"prad_batch_plan_f2d": "prad_batch_plan_ng", "prad_calculate_batch_f2d_dev": "prad_calculate_batch_ng_dev",
            "prad_batch_glszm_f2d_dev": "prad_batch_glszm_ng_dev", "prad_batch_glszm_fill_dev": "prad_batch_glszm_fill_ng_dev",
            "prad_batch_merge_plan": "prad_batch_merge_plan_ng", "prad_batch_merge_angles_dev": "prad_batch_merge_angles_ng_dev",
            "prad_batch_features_plan": "prad_batch_features_plan_ng", "prad_batch_features_dev": "prad_batch_features_ng_dev"}
BATCH_MAX_NG = 64          # levels per ROI the batched texture kernels take (PRAD_BATCH_MAX_NG)


def batch_levels(Ng, B):
    """`Ng` of the batched calls, normalised: an int stays an int (one count for the whole batch, the calls as they always
    were); an int sequence becomes an intc array [B], one count per ROI (anything but B entries is a ValueError)"""
    if np.ndim(Ng) == 0:
        return int(Ng)
    v = np.asarray(Ng)
    if v.ndim != 1 or v.shape[0] != int(B) or not np.issubdtype(v.dtype, np.integer):
        raise ValueError("Ng must be an int or an int sequence with one entry per ROI (%d), got shape %s %s"
                         % (int(B), v.shape, v.dtype))
    return np.ascontiguousarray(v.astype(np.intc))


def batch_levels_vector(Ng, B):
    """intc [B] whichever form `Ng` has (for the arithmetic of the Python layer)"""
    Ng = batch_levels(Ng, B)
    return Ng if isinstance(Ng, np.ndarray) else np.full(int(B), Ng, dtype=np.intc)


def batch_levels_call(lib, name, Ng):
    """`Ng` as batch_levels returns it -> (the entry point `name` for an int, its _ng twin for a vector; the C argument)"""
    if isinstance(Ng, np.ndarray):
        return getattr(lib, _NG_TWIN[name]), _iptr(Ng)
    return getattr(lib, name), int(Ng)


def batch_plan(sizes, Ng, families=BATCH_FAMILIES, distances=(1,), force2D=False, force2Ddimension=0):
    """Host-side layout of a batch (prad_batch_plan_f2d, or prad_batch_plan_ng for an int sequence Ng [B]: every ROI laid out
    with its own count; needs no device).  sizes: int [B, 3].  -> (covered, offsets int64
    [4, B + 1], Na int32 [2, B]): covered = the native call takes the batch; offsets[f] = first double of every ROI in the
    flat buffer of family BATCH_FAMILIES[f] (last entry: its length); Na[0] = unidirectional angle count of `distances`
    (GLCM; GLDM rows hold 2 * (2 * Na) + 1 columns), Na[1] = that of distance 1 (GLRLM) -- with force2D the counts of
    generate_angles(size, distances, False, True, force2Ddimension), 0 where no angle is left."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    dist = np.ascontiguousarray(np.asarray(distances, dtype=np.intc).ravel())
    B = int(sizes.shape[0])
    offsets = np.zeros((4, B + 1), dtype=np.int64)
    Na = np.zeros((2, B), dtype=np.intc)
    plan, ng = batch_levels_call(_lib.load(), "prad_batch_plan_f2d", batch_levels(Ng, B))
    rc = plan(_iptr(sizes), B, ng, batch_family_bits(families), _iptr(dist), int(dist.shape[0]),
              batch_forced_dim(force2D, force2Ddimension), offsets.ctypes.data_as(C.POINTER(C.c_longlong)), _iptr(Na))
    if rc != _lib.PRAD_OK and rc != _lib.PRAD_E_UNSUPPORTED:
        _lib.raise_for(rc, "batch plan")
    return rc == _lib.PRAD_OK, offsets, Na


MERGE_FAMILIES = ("glcm", "glrlm")       # the families weightingNorm merges: bit f of the C `families`, row f of the merge plan


def batch_merge_plan(sizes, Ng, Na, families=MERGE_FAMILIES):
    """Host-side layout of the weighted angle merge (prad_batch_merge_plan; needs no device).  Na: the int [2, B] of
    batch_plan; Ng: an int or an int sequence [B].  -> offsets int64 [3, B + 1]: rows 0 / 1 = first double of every ROI's merged GLCM [Ng, Ng, 1] / GLRLM [Ng,
    max(size), 1] in its flat buffer (zeros for a family not asked for), row 2 = first weight of every ROI in the flat weight
    table (Na[0, b] GLCM weights, then Na[1, b] GLRLM weights); last entries: the lengths."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    Na = np.ascontiguousarray(np.asarray(Na, dtype=np.intc).reshape(2, -1))
    B = int(sizes.shape[0])
    if Na.shape[1] != B or not families or any(f not in MERGE_FAMILIES for f in families):
        raise ValueError("batch_merge_plan: Na must be [2, B], families a non-empty subset of %s" % (MERGE_FAMILIES,))
    offsets = np.zeros((3, B + 1), dtype=np.int64)
    plan, ng = batch_levels_call(_lib.load(), "prad_batch_merge_plan", batch_levels(Ng, B))
    rc = plan(_iptr(sizes), B, ng, sum(1 << MERGE_FAMILIES.index(f) for f in set(families)), _iptr(Na),
              offsets.ctypes.data_as(C.POINTER(C.c_longlong)))
    _lib.raise_for(rc, "batch merge plan")
    return offsets


def batch_spacing(spacing, B):
    """`spacing` of the batched calls -- one (z, y, x) triple or a float array [B, 3] -- as float64 [B, 3]"""
    sp = np.asarray(spacing, dtype=np.float64)
    if sp.shape == (3,):
        sp = np.broadcast_to(sp, (B, 3))
    if sp.shape != (B, 3):
        raise ValueError("spacing must be one (z, y, x) triple or an array [B, 3]")
    return np.ascontiguousarray(sp)


def batch_weighting_norm(weightingNorm):
    """None, or one of the names paramcheck accepts; anything else is a ValueError (the classes only warn)"""
    from .paramcheck import _WEIGHTINGS
    if weightingNorm is not None and weightingNorm not in _WEIGHTINGS:
        raise ValueError("weightingNorm must be None or one of %s, got %r" % (_WEIGHTINGS, weightingNorm))
    return weightingNorm


def batch_weights(sizes, Na, distances, weightingNorm, spacing=(1.0, 1.0, 1.0), force2D=False, force2Ddimension=0):
    """The flat weight table of the weighted angle merge, in the layout of batch_merge_plan's row 2: per ROI the GLCM weights of
    its Na[0, b] angles, then the GLRLM weights of its Na[1, b] distance-1 angles, both from glcm._weights -- the one function the
    feature classes use -- on the ROI's own angle rows and spacing.  -> float64 [sum(Na)]."""
    import logging
    from .glcm import _weights
    sizes = np.asarray(sizes, dtype=np.intc).reshape(-1, 3)
    sp = batch_spacing(spacing, len(sizes))
    f2d = batch_forced_dim(force2D, force2Ddimension)
    norm, log = batch_weighting_norm(weightingNorm), logging.getLogger(__name__)
    parts = [np.zeros(0)]
    seen = {}          # (size, spacing) -> the ROI's weights: a table of lesions repeats few box shapes
    for b, size in enumerate(sizes):
        key = (size.tobytes(), sp[b].tobytes())
        if key not in seen:
            size = np.ascontiguousarray(size)
            one = [np.zeros(0)]
            if Na[0][b]:
                one.append(_weights(_build_angles(size, distances, False, f2d), sp[b], norm, "glcm", log))
            if Na[1][b]:
                one.append(_weights(_build_angles(size, None, False, f2d), sp[b], norm, "glrlm", log))
            seen[key] = np.concatenate(one)
        parts.append(seen[key])
    return np.ascontiguousarray(np.concatenate(parts))


def batch_shapes(sizes, Ng, Na):
    """{family: [shape of ROI b]} for the plan's Na; Ng: an int or an int sequence [B]"""
    sizes = np.asarray(sizes).reshape(-1, 3)
    ng = [int(g) for g in batch_levels_vector(Ng, len(sizes))]
    return {"glcm": [(g, g, int(a)) for g, a in zip(ng, Na[0])],
            "glrlm": [(g, int(max(s)), int(a)) for g, s, a in zip(ng, sizes, Na[1])],
            "gldm": [(g, 4 * int(a) + 1) for g, a in zip(ng, Na[0])],
            "ngtdm": [(g, 3) for g in ng]}


def _host_box(image, mask):
    """(levels, mask) of one ROI as numpy arrays, wherever they live"""
    back = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return back(image), back(mask) != 0


def _no_angle_matrices(image, mask, Ng, fam):
    """Family `fam` of a box in which no angle of the family fits -- 1 x 1 x 1, or every angle removed by the forced dimension
    (5 x 1 x 1 with dimension 0): the single calls refuse it, cmatrices.c computes these from an empty angle table.  GLCM and
    GLRLM have no angle; every masked voxel is a voxel without neighbours: dependence 0 (GLDM [Ng, 1] = voxels per level),
    NGTDM (voxels per level, 0, level)."""
    if fam in ("glcm", "glrlm"):
        return np.zeros((Ng, Ng if fam == "glcm" else int(max(image.shape)), 0))
    lv, mk = _host_box(image, mask)
    inside = lv[mk].astype(np.int64)
    if inside.size and (inside.min() < 1 or inside.max() > Ng):
        raise IndexError("level outside [1, Ng]")
    out = np.zeros((Ng, 1 if fam == "gldm" else 3))
    out[:, 0] = np.bincount(inside, minlength=Ng + 1)[1:]
    if fam == "ngtdm":
        out[:, 2] = np.arange(1, Ng + 1)
    return out


def _looped_matrices(rois, Ng, families, shapes, single, wrap=lambda a: a):
    """The looped route: every ROI of `rois`, pairs (image, mask), through the single calls -> ({family: [B matrices]}, status).
    single[f](image, mask) is the call of family f; wrap makes the caller's kind of result of a numpy matrix (the device route
    puts it where its other results are).  A family without an angle in a box (its planned shape says so) is not sent to the
    single call, which would refuse the box."""
    _set_batch_route("looped")
    mats, status = {f: [] for f in families}, []
    for b, (image, mask) in enumerate(rois):
        no_angle = {"glcm": shapes["glcm"][b][2] == 0, "glrlm": shapes["glrlm"][b][2] == 0}
        no_angle["gldm"] = no_angle["ngtdm"] = no_angle["glcm"]
        try:
            one = {f: (wrap(_no_angle_matrices(image, mask, Ng, f)) if no_angle[f] else single[f](image, mask))
                   for f in BATCH_FAMILIES if f in families}
            status.append(_lib.PRAD_OK)
        except IndexError:          # a masked level outside [1, Ng]: as the native route, the matrices of an empty mask
            one = {f: np.zeros(shapes[f][b]) for f in families}
            if "ngtdm" in one:
                one["ngtdm"][:, 2] = np.arange(1, Ng + 1)
            one = {f: wrap(m) for f, m in one.items()}
            status.append(_lib.PRAD_INDEX_ERROR)
        for f in families:
            mats[f].append(one[f])
    return mats, status


def merge_looped(mats, sizes, Na, distances, weightingNorm, spacing, force2D, force2Ddimension, symmetric, wrap=lambda a: a):
    """The weighted angle merge on the host, for the looped routes: adds "glcm_w" / "glrlm_w" to `mats` for the families it
    holds, with the arithmetic of the merge launch (kernels_batch_merge.h) -- transpose added first, then acc = acc + P[..., a] *
    w[a] over a ascending in float64 -- so that "looped", "mixed" and "batch" agree bit for bit."""
    w = batch_weights(sizes, Na, distances, weightingNorm, spacing, force2D, force2Ddimension)
    at = 0
    for f in MERGE_FAMILIES:
        if f in mats:
            mats[f + "_w"] = []
    for b in range(len(sizes)):
        for k, f in enumerate(MERGE_FAMILIES):
            n = int(Na[k][b])
            if f in mats:
                P = mats[f][b].cpu().numpy() if hasattr(mats[f][b], "cpu") else np.asarray(mats[f][b])
                if f == "glcm" and symmetric:
                    P = P + P.transpose(1, 0, 2)
                acc = np.zeros(P.shape[:2] + (1,))
                for a in range(n):
                    acc[..., 0] = acc[..., 0] + P[..., a] * w[at + a]
                mats[f + "_w"].append(wrap(acc))
            at += n
    return mats


def _no_angle_glszm(image, mask, Ng, compact, wrap):
    """the GLSZM of a box without neighbours (1 x 1 x 1, or every neighbour removed by the forced dimension: the single call
    refuses it): every masked voxel is a zone of size 1; dense or as calculate_glszm_compact"""
    lv, mk = _host_box(image, mask)
    inside = lv[mk].astype(np.int64)
    if inside.size and (inside.min() < 1 or inside.max() > Ng):
        raise IndexError("level outside [1, Ng]")
    P = np.zeros((Ng, 1))
    P[:, 0] = np.bincount(inside, minlength=Ng + 1)[1:]
    if not compact:
        return wrap(P)
    return (wrap(P), np.ones(1, dtype=np.intc)) if inside.size else (wrap(P[:, :0]), np.zeros(0, dtype=np.intc))


def _looped_glszm(rois, Ng, compact, single, wrap=lambda a: a, f2d=-1):
    """every ROI of `rois`, pairs (image, mask), through the single call -> (results, status): single(image, mask, Ns) is that
    call, dense or compact as asked for; wrap as in _looped_matrices; f2d: the forced dimension the single call is given"""
    results, status = [], []
    lib, one = _lib.load(), np.ones(1, dtype=np.intc)
    for image, mask in rois:
        try:
            size = np.array(image.shape, dtype=np.intc)
            if lib.prad_get_angle_count(_iptr(size), _iptr(one), 3, 1, 1, int(f2d)) == 0:
                results.append(_no_angle_glszm(image, mask, Ng, compact, wrap))
            else:
                results.append(single(image, mask, max(1, int(mask.sum()))))
            status.append(_lib.PRAD_OK)
        except IndexError:          # as the native route: status 0, the result of an empty mask
            results.append(_no_angle_glszm(np.zeros((1, 1, 1), dtype=np.intc), np.zeros((1, 1, 1), dtype=bool), Ng, compact, wrap))
            status.append(_lib.PRAD_INDEX_ERROR)
    return results, status


def _host_roi_batch(images, masks, noun, raw=False, loops=False):
    """Lists of host arrays -> (images, masks, sizes intc [B, 3], upload).  Levels and bool masks are parsed as the single calls
    parse them (_parse_arrays); raw=True: intensity boxes, which keep their dtype where it is one of the four the kernels read
    and all share it (float64 otherwise), and masks of any dtype, non-zero = ROI.  upload() -> (flat data tensor, flat uint8 mask
    tensor) on the current device, ONE copy each.  loops=True: the caller can loop the single calls, so an empty list is fine
    and so is a machine without a device (upload is None there); otherwise both raise.  `noun` names the batch in the messages."""
    if len(images) != len(masks):
        raise ValueError("images and masks differ in number")
    if raw:
        imgs = [np.ascontiguousarray(np.asarray(i)) for i in images]
        msks = [np.ascontiguousarray(np.asarray(m)) for m in masks]
    else:
        parsed = [_parse_arrays(i, m) for i, m in zip(images, masks)]
        imgs, msks = [p[0] for p in parsed], [p[1] for p in parsed]
    if not (imgs or loops) or any(i.ndim != 3 or i.shape != m.shape for i, m in zip(imgs, msks)):
        raise ValueError("the batched %s %s %s3-D ROIs%s" % (noun, "takes" if noun == "GLSZM" else "take",
                                                             "" if loops else "a non-empty list of ",
                                                             " with masks of the same shape" if raw else ""))
    sizes = np.array([i.shape for i in imgs], dtype=np.intc).reshape(-1, 3)
    if _lib.load().prad_device_count() < 1:
        if not loops:
            raise RuntimeError("no HIP device: the batched %s are evaluated on the device" % noun)
        return imgs, msks, sizes, None

    def upload():
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        dt = np.dtype(np.intc)
        if raw:
            dt = imgs[0].dtype if (imgs[0].dtype in (np.float32, np.float64, np.int32, np.int16)
                                   and all(i.dtype == imgs[0].dtype for i in imgs)) else np.dtype(np.float64)
        if not imgs:
            return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.uint8, device=dev)
        flat_i = torch.from_numpy(np.concatenate([i.ravel().astype(dt, copy=False) for i in imgs])).to(dev)
        flat_m = torch.from_numpy(np.concatenate([(m.ravel() != 0 if raw else m.ravel()).view(np.uint8) for m in msks])).to(dev)
        return flat_i, flat_m
    return imgs, msks, sizes, upload


def calculate_matrices_batch(images, masks, Ng, families=BATCH_FAMILIES, distances=(1,), gldm_a=0, force2D=False,
                             force2Ddimension=0, weightingNorm=None, spacing=(1.0, 1.0, 1.0), symmetricalGLCM=True):
    """GLCM / GLRLM / GLDM / NGTDM of B small 3-D ROIs (lists of host arrays: int levels, bool masks) with one upload, one
    native call and one download per family.  -> ({family: [B numpy matrices in the single calls' layouts]}, status [B]:
    1, or 0 for a ROI with a masked level outside [1, Ng] -- the single calls' IndexError; its matrices are void).
    force2D / force2Ddimension / weightingNorm / spacing / symmetricalGLCM: as engine.texture_matrices_batch (weightingNorm
    adds the merged "glcm_w" [Ng, Ng, 1] / "glrlm_w" [Ng, max(size), 1]).
    Where the native call does not cover the batch (Ng > 64, a box above prad_batch_max_vox() voxels, > 127 angles) or no
    device is visible, the single calls are looped ROI by ROI (and raise as they do without a device); last_batch_route()
    tells which.  GLSZM: calculate_glszm_batch.
    Ng: an int, or an int sequence [B] -- every ROI with its own count, as engine.texture_matrices_batch takes it: the ROIs of
    at most 64 levels inside the box caps share one native call, the others take the single calls ("mixed")."""
    families = tuple(families)
    batch_family_bits(families)
    imgs, msks, sizes, upload = _host_roi_batch(images, masks, "matrices", loops=True)
    dist = [int(d) for d in np.asarray(distances).ravel()]
    f2, fd = bool(force2D), int(force2Ddimension)
    B = len(imgs)
    Ng = batch_levels(Ng, B)
    covered, offsets, Na = batch_plan(sizes, Ng, families, dist, f2, fd)
    shapes = batch_shapes(sizes, Ng, Na)
    batch_weighting_norm(weightingNorm)
    # the merge is a device launch and a batch of mixed counts is partitioned there: the device route serves both
    if (weightingNorm is not None or isinstance(Ng, np.ndarray)) and upload is not None:
        mats, status = _engine().texture_matrices_batch(*upload(), sizes, Ng, families, dist, int(gldm_a), f2, fd,
                                                        weightingNorm, spacing, symmetricalGLCM)
        return {f: [m.cpu().numpy() for m in mats[f]] for f in mats}, status
    if not covered or upload is None:
        def single(ng):
            return {"glcm": lambda i, m: calculate_glcm(i, m, dist, ng, f2, fd)[0][0],
                    "glrlm": lambda i, m: calculate_glrlm(i, m, ng, int(max(i.shape)), f2, fd)[0][0],
                    "gldm": lambda i, m: calculate_gldm(i, m, dist, ng, int(gldm_a), f2, fd)[0],
                    "ngtdm": lambda i, m: calculate_ngtdm(i, m, dist, ng, f2, fd)[0]}
        if isinstance(Ng, np.ndarray):          # (no device: ROI by ROI, each with its own count)
            mats, status = {f: [] for f in families}, []
            for b in range(B):
                one, st = _looped_matrices([(imgs[b], msks[b])], int(Ng[b]), families, {f: [shapes[f][b]] for f in shapes},
                                           single(int(Ng[b])))
                status += st
                for f in families:
                    mats[f] += one[f]
        else:
            mats, status = _looped_matrices(zip(imgs, msks), Ng, families, shapes, single(Ng))
        if weightingNorm is not None:
            merge_looped(mats, sizes, Na, dist, weightingNorm, spacing, f2, fd, symmetricalGLCM)
        return mats, status
    flat_l, flat_m = upload()
    flat, status = _engine().texture_matrices_batch_flat(flat_l, flat_m, sizes, Ng, families, dist, int(gldm_a), f2, fd)
    mats = {}
    for f in families:
        host = flat[f].cpu().numpy()
        o = offsets[BATCH_FAMILIES.index(f)]
        mats[f] = [host[o[b]:o[b + 1]].reshape(shapes[f][b]) for b in range(B)]
    return mats, status


def calculate_glszm_batch(images, masks, Ng, compact=False, force2D=False, force2Ddimension=0, weightingNorm=None,
                          spacing=(1.0, 1.0, 1.0)):
    """GLSZM of B small 3-D ROIs (lists of host arrays: int levels, bool masks) with one upload and the two launches of
    engine.glszm_batch.  -> (list of B results, status [B]: 1, or 0 for a ROI with a masked level outside [1, Ng] -- the
    single call's IndexError; its result is that of an empty mask).  compact=False: a result is the float64 matrix [Ng,
    max(maxRegion, 1)] of calculate_glszm (without its leading axis); compact=True: (P [Ng, k], sizes int32 [k]) as
    calculate_glszm_compact.  With no device visible the single calls are looped ROI by ROI (and raise as they do without a
    device); last_batch_route() tells which route ran.  force2D / force2Ddimension: zones join only in the plane across that
    axis; weightingNorm / spacing are accepted and ignored, as the class ignores them.  Ng: an int, or an int sequence [B]
    (every ROI with its own count, as engine.glszm_batch takes it)."""
    imgs, msks, sizes, upload = _host_roi_batch(images, masks, "GLSZM", loops=True)
    Ng = batch_levels(Ng, len(imgs))
    f2, fd = bool(force2D), int(force2Ddimension)
    f2d = batch_forced_dim(f2, fd)
    batch_weighting_norm(weightingNorm)
    if upload is None:
        def single(ng):
            def one(img, msk, Ns):
                P = calculate_glszm(img, msk, ng, Ns, f2, fd)[0]
                cols = np.flatnonzero(P.any(0))
                return (np.ascontiguousarray(P[:, cols]), (cols + 1).astype(np.intc)) if compact else P
            return one
        _set_batch_route("looped")
        if not isinstance(Ng, np.ndarray):
            return _looped_glszm(zip(imgs, msks), Ng, compact, single(Ng), f2d=f2d)
        results, status = [], []
        for img, msk, ng in zip(imgs, msks, Ng):
            one, st = _looped_glszm([(img, msk)], int(ng), compact, single(int(ng)), f2d=f2d)
            results += one
            status += st
        return results, status
    flat_l, flat_m = upload()
    results, status = _engine().glszm_batch(flat_l, flat_m, sizes, Ng, compact=compact, force2D=f2, force2Ddimension=fd)
    if compact:
        return [(P.cpu().numpy(), s) for P, s in results], status
    return [P.cpu().numpy() for P in results], status


def batch_feature_names(cls):
    """the columns of engine.texture_features_batch for class `cls` (None: a slot that is no feature of the class)"""
    return VOXEL_GLCM_FEATURES + ["MCC"] if cls == "glcm" else list(_ZONE_LIKE[cls][1])


def calculate_features_batch(images, masks, Ng, classes=("glcm", "glrlm", "glszm", "gldm", "ngtdm"), distances=(1,), gldm_a=0,
                             symmetricalGLCM=True, mcc=True, force2D=False, force2Ddimension=0, weightingNorm=None,
                             spacing=(1.0, 1.0, 1.0)):
    """The texture features of B small 3-D ROIs (lists of host arrays: int levels, bool masks): one upload, the batched matrix
    calls and the batched formulas of engine.texture_features_batch.  -> {class: {feature name: float64 [B]}}; a ROI with a masked level
    outside [1, Ng] (the single calls' IndexError) has NaN everywhere, the others are not affected.  The names are those of the feature classes
    (VOXEL_*_FEATURES, plus "MCC").  Needs a device (RuntimeError without one); last_batch_route() tells which route ran.
    force2D / force2Ddimension / weightingNorm / spacing: as engine.texture_features_batch; so is Ng: an int, or an int sequence
    [B] that gives every ROI its own count."""
    _, _, sizes, upload = _host_roi_batch(images, masks, "features")
    table, _ = _engine().texture_features_batch(*upload(), sizes, batch_levels(Ng, len(sizes)), tuple(classes),
                                                [int(d) for d in np.asarray(distances).ravel()], int(gldm_a),
                                                bool(symmetricalGLCM), bool(mcc), False, bool(force2D), int(force2Ddimension),
                                                weightingNorm, spacing)
    return {cls: {name: table[cls][:, i].copy() for i, name in enumerate(batch_feature_names(cls)) if name}
            for cls in table}


def batch_firstorder_plan(sizes, dtype):
    """Host-side plan of the batched first-order launch (prad_batch_firstorder_plan; needs no device).  sizes: int [B, 3]; dtype:
    the image dtype code (0 float32, 1 float64, 2 int32, 3 int16).  -> (covered, lds_bytes, inside bool [B]): the launch takes the
    batch; the dynamic LDS it asks for; per ROI whether the box is certainly within the key capacity."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.intc).reshape(-1, 3))
    B = int(sizes.shape[0])
    lds = C.c_longlong(0)
    inside = np.zeros(max(B, 1), dtype=np.intc)
    rc = _lib.load().prad_batch_firstorder_plan(_iptr(sizes), B, int(dtype), C.byref(lds), _iptr(inside))
    if rc != _lib.PRAD_E_UNSUPPORTED:
        _lib.raise_for(rc, "batch firstorder plan")
    return rc == _lib.PRAD_OK, int(lds.value), inside[:B].astype(bool)


def calculate_firstorder_batch(images, masks, voxelArrayShift=0.0, voxelVolume=1.0, **binning):
    """The first-order features of B small 3-D ROIs (lists of host arrays: raw intensities, masks): one upload, then
    engine.roi_features_batch with the first-order class alone -- two launches and two read-backs for the whole batch.  binning:
    binWidth (default 25) or binCount, for Entropy and Uniformity.  -> {"firstorder": {feature name: float64 [B]}}; an empty ROI
    has NaN everywhere.  Needs a device (RuntimeError without one); last_batch_route() tells which route ran."""
    return calculate_roi_features_batch(images, masks, classes=("firstorder",), voxelArrayShift=voxelArrayShift,
                                        voxelVolume=voxelVolume, **binning)


def calculate_roi_features_batch(images, masks, classes=("firstorder", "glcm", "glrlm", "glszm", "gldm", "ngtdm"), binWidth=None,
                                 binCount=None, voxelArrayShift=0.0, voxelVolume=1.0, distances=(1,), gldm_a=0,
                                 symmetricalGLCM=True, mcc=True, force2D=False, force2Ddimension=0, weightingNorm=None,
                                 spacing=(1.0, 1.0, 1.0)):
    """The features of all six classes of B small 3-D ROIs from raw intensity boxes and masks (lists of host arrays): one upload,
    then engine.roi_features_batch.  -> {class: {feature name: float64 [B]}} (FIRSTORDER_FEATURES / batch_feature_names); an
    empty ROI has NaN everywhere, the others are not affected.  Needs a device (RuntimeError without one); last_batch_route()
    tells which route ran.  force2D / force2Ddimension / weightingNorm / spacing: as engine.roi_features_batch."""
    _, _, sizes, upload = _host_roi_batch(images, masks, "ROI features", raw=True)
    table, _ = _engine().roi_features_batch(*upload(), sizes, tuple(classes), binWidth, binCount, float(voxelArrayShift),
                                            voxelVolume, [int(d) for d in np.asarray(distances).ravel()], int(gldm_a),
                                            bool(symmetricalGLCM), bool(mcc), False, bool(force2D), int(force2Ddimension),
                                            weightingNorm, spacing)
    names = {cls: (FIRSTORDER_FEATURES if cls == "firstorder" else batch_feature_names(cls)) for cls in table}
    return {cls: {name: table[cls][:, i].copy() for i, name in enumerate(names[cls]) if name} for cls in table}


def calculate_wavelet_batch(images, wavelet="coif1", level=1, start_level=0, force2D=False, force2Ddimension=0):
    """The wavelet sub-bands of B small 3-D boxes (a list of host arrays: raw intensities): one upload, engine.wavelet_batch --
    one launch for all boxes and all eight bands inside its native domain -- and one download.  -> ({image type name: [B float64
    numpy arrays in the boxes' shapes]}, names): the names getWaveletImage yields, in its order ("wavelet-LLH" ...
    "wavelet-LLL").  Needs a device (RuntimeError without one); last_batch_route() tells which route ran."""
    ones = [np.ones(np.shape(i), dtype=bool) for i in images]
    _, _, sizes, upload = _host_roi_batch(images, ones, "wavelet sub-bands", raw=True)
    bands, names, _ = _engine().wavelet_batch(upload()[0], sizes, wavelet, level, start_level, force2D,
                                              force2Ddimension=force2Ddimension)
    host = bands.cpu().numpy()
    nvox = sizes.astype(np.int64).prod(1)
    off = np.concatenate([[0], np.cumsum(nvox)])
    return {name: [host[row, off[b]:off[b + 1]].reshape(tuple(sizes[b])).copy() for b in range(len(nvox))]
            for name, row in zip(names, names.rows)}, tuple(names)


def calculate_log_batch(images, sigma, spacing=(1.0, 1.0, 1.0)):
    """The LoG images of B small 3-D boxes (a list of host arrays: raw intensities) for the sigmas `sigma`: one upload,
    engine.log_batch -- at most three launches for all boxes and sigmas inside its native domain -- and one download.  spacing:
    (z, y, x), one triple or [B, 3].  -> ({image type name: [B numpy arrays in the boxes' shapes -- float64 for float64 boxes,
    float32 otherwise --, None where the reference yields no image]}, names): the names getLoGImage yields, in its order.  Needs
    a device (RuntimeError without one); last_batch_route() tells which route ran."""
    ones = [np.ones(np.shape(i), dtype=bool) for i in images]
    _, _, sizes, upload = _host_roi_batch(images, ones, "LoG images", raw=True)
    logs, names, _, valid = _engine().log_batch(upload()[0], sizes, sigma, spacing)
    host = logs.cpu().numpy()
    nvox = sizes.astype(np.int64).prod(1)
    off = np.concatenate([[0], np.cumsum(nvox)])
    return {name: [host[s, off[b]:off[b + 1]].reshape(tuple(sizes[b])).copy() if valid[s, b] else None for b in range(len(nvox))]
            for s, name in enumerate(names)}, tuple(names)


def _host_boxes(flat, sizes):
    """a flat host row in the batch layout -> [B numpy arrays in the boxes' shapes]"""
    off = np.concatenate([[0], np.cumsum(sizes.astype(np.int64).prod(1))])
    return [flat[off[b]:off[b + 1]].reshape(tuple(sizes[b])).copy() for b in range(len(sizes))]


def calculate_intensity_batch(images, types=("Square", "SquareRoot", "Logarithm", "Exponential")):
    """The Square, SquareRoot, Logarithm and Exponential images of B small 3-D boxes (a list of host arrays: raw intensities):
    one upload, engine.intensity_batch -- two launches for all boxes and all types -- and one download.  -> ({image type name:
    [B float64 numpy arrays in the boxes' shapes]}, names): the names the single functions yield ("square", "squareroot",
    "logarithm", "exponential"), in the order of the rows.  Every image is that of the box ALONE (its own max |x|).  Needs a
    device (RuntimeError without one); last_batch_route() tells which route ran."""
    ones = [np.ones(np.shape(i), dtype=bool) for i in images]
    _, _, sizes, upload = _host_roi_batch(images, ones, "intensity transforms", raw=True)
    rows, names, _ = _engine().intensity_batch(upload()[0], sizes, types)
    host = rows.cpu().numpy()
    return {name: _host_boxes(host[r], sizes) for r, name in enumerate(names)}, tuple(names)


def calculate_gradient_batch(images, spacing=(1.0, 1.0, 1.0), gradientUseSpacing=True):
    """The Gradient magnitude images of B small 3-D boxes (a list of host arrays: raw intensities): one upload,
    engine.gradient_batch -- one launch for all boxes -- and one download.  spacing: (z, y, x), one triple or [B, 3].  -> ([B
    float32 numpy arrays in the boxes' shapes], "gradient"); the box's own edge is replicated.  Needs a device (RuntimeError
    without one); last_batch_route() tells which route ran."""
    ones = [np.ones(np.shape(i), dtype=bool) for i in images]
    _, _, sizes, upload = _host_roi_batch(images, ones, "gradient images", raw=True)
    image, name, _ = _engine().gradient_batch(upload()[0], sizes, spacing, gradientUseSpacing)
    return _host_boxes(image.cpu().numpy(), sizes), name


def calculate_lbp2d(array, radius=1, samples=8, method="uniform", force2Ddimension=0):
    """The LBP2D image of a host array (2-D, or 3-D with the planes stacked along force2Ddimension): one upload, engine.lbp2d --
    one launch -- and one download.  -> numpy array of the input's shape: 3-D in the dtype the device holds it in (float32,
    float64, int32, int16; anything else is widened to float64), 2-D as float64.  Needs a device (RuntimeError without one);
    NotImplementedError beyond the kernel's domain (ceil(radius) <= 8): filters.lbp2d_host computes those."""
    from . import filters
    a = np.asarray(array)
    if a.ndim not in (2, 3):
        raise ValueError("LBP2D takes 2-D and 3-D images")
    if a.dtype not in (np.float32, np.float64, np.int32, np.int16):
        a = a.astype(np.float64)
    filters.lbp2d_settings(radius, samples, method, a.dtype if a.ndim == 3 else None)      # (before any device work)
    eng = _engine()
    return eng.lbp2d(_to_device(a), radius, samples, method, force2Ddimension).cpu().numpy()


def calculate_lbp2d_batch(images, lbp2DRadius=1, lbp2DSamples=8, lbp2DMethod="uniform", force2Ddimension=0):
    """The LBP2D images of B 3-D boxes (a list of host arrays: raw intensities): one upload, engine.lbp2d_batch -- one launch for
    all boxes -- and one download.  -> ([B float64 numpy arrays in the boxes' shapes], "lbp-2D"); every image is that of the box
    ALONE (a sample beyond its edge reads 0).  Needs a device (RuntimeError without one); last_batch_route() tells which route
    ran."""
    from . import filters
    filters.lbp2d_settings(lbp2DRadius, lbp2DSamples, lbp2DMethod)
    ones = [np.ones(np.shape(i), dtype=bool) for i in images]
    _, _, sizes, upload = _host_roi_batch(images, ones, "LBP2D images", raw=True)
    image, name, _ = _engine().lbp2d_batch(upload()[0], sizes, lbp2DRadius, lbp2DSamples, lbp2DMethod, force2Ddimension)
    return _host_boxes(image.cpu().numpy(), sizes), name


def calculate_mask_boxes_batch(masks):
    """The bounding boxes of B 3-D masks (a list of host arrays, non-zero = ROI): one upload, engine.mask_boxes_batch -- one
    launch -- and one read-back.  -> (lo int64 [B, 3], hi int64 [B, 3], count int64 [B]), inclusive (z, y, x) bounds; an empty
    mask has count 0, lo = its shape and hi = -1.  Needs a device (RuntimeError without one)."""
    _, _, sizes, upload = _host_roi_batch(masks, masks, "mask boxes", raw=True)
    return _engine().mask_boxes_batch(upload()[1], sizes)


def calculate_resegment_batch(images, masks, resegmentRange=None, resegmentMode="absolute"):
    """resegmentMask on each of B small 3-D boxes (lists of host arrays: raw intensities and masks, non-zero = ROI): one upload,
    engine.resegment_batch -- one launch for all boxes inside its native domain -- and one download.  -> (masks: [B uint8 numpy
    arrays in the boxes' shapes, 1 in the kept ROI], boxes int64 [B, 7]: lo z / y / x, hi z / y / x and count of the kept ROI,
    thresholds float64 [B, 2], status int64 [B]: 0 fine, 1 empty on entry, 3 at most one voxel kept).  Needs a device
    (RuntimeError without one); last_batch_route() tells which route ran."""
    _engine()._resegment_args(resegmentRange, resegmentMode)      # (resegmentMask's ValueErrors, before a device is asked)
    _, _, sizes, upload = _host_roi_batch(images, masks, "resegmentation", raw=True)
    out, boxes, thr, status = _engine().resegment_batch(*upload(), sizes, resegmentRange, resegmentMode)
    return _host_boxes(out.cpu().numpy(), sizes), boxes, thr, status


def calculate_resample_batch(images, masks, spacing=(1.0, 1.0, 1.0), resampledPixelSpacing=None, interpolator="sitkBSpline",
                             padDistance=5):
    """resampleImage on each of B small 3-D boxes as if the box were the whole image (lists of host arrays: raw intensities and
    masks, non-zero = ROI): one upload, engine.resample_batch -- three launches for all boxes inside its native domain -- and
    one download.  spacing (z, y, x), one triple or [B, 3]; resampledPixelSpacing (x, y, z).  -> (images, masks: [B numpy arrays
    on the new grids; uint8 masks], spacing float64 [B, 3] (z, y, x), origin_shift float64 [B, 3] (x, y, z), status int64 [B]:
    1 for an empty mask, whose box is kept).  Needs a device (RuntimeError without one); last_batch_route() tells which route
    ran."""
    _, _, sizes, upload = _host_roi_batch(images, masks, "resampling", raw=True)
    out, out_masks, newsize, new_spacing, shift, status = _engine().resample_batch(*upload(), sizes, spacing, resampledPixelSpacing,
                                                                                   interpolator, padDistance)
    host, host_m = out.cpu().numpy(), out_masks.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(newsize.astype(np.int64).prod(1))])
    cut = lambda flat: [flat[off[b]:off[b + 1]].reshape(tuple(newsize[b])).copy() for b in range(len(newsize))]
    return cut(host), cut(host_m), new_spacing, shift, status


# ---- fused voxel-based features of the other four texture classes (prad_voxel_texture_features_dev) ---------
_ZONE_LIKE = {
    "glrlm": (3, ["ShortRunEmphasis", "LongRunEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized",
                  "RunLengthNonUniformity", "RunLengthNonUniformityNormalized", "RunPercentage", "GrayLevelVariance",
                  "RunVariance", "RunEntropy", "LowGrayLevelRunEmphasis", "HighGrayLevelRunEmphasis",
                  "ShortRunLowGrayLevelEmphasis", "ShortRunHighGrayLevelEmphasis", "LongRunLowGrayLevelEmphasis",
                  "LongRunHighGrayLevelEmphasis"]),
    "glszm": (4, ["SmallAreaEmphasis", "LargeAreaEmphasis", "GrayLevelNonUniformity", "GrayLevelNonUniformityNormalized",
                  "SizeZoneNonUniformity", "SizeZoneNonUniformityNormalized", "ZonePercentage", "GrayLevelVariance",
                  "ZoneVariance", "ZoneEntropy", "LowGrayLevelZoneEmphasis", "HighGrayLevelZoneEmphasis",
                  "SmallAreaLowGrayLevelEmphasis", "SmallAreaHighGrayLevelEmphasis", "LargeAreaLowGrayLevelEmphasis",
                  "LargeAreaHighGrayLevelEmphasis"]),
    # None = slot of the shared numbering that is a deprecated feature in this class (gldm.py:228,311)
    "gldm": (1, ["SmallDependenceEmphasis", "LargeDependenceEmphasis", "GrayLevelNonUniformity", None,
                 "DependenceNonUniformity", "DependenceNonUniformityNormalized", None, "GrayLevelVariance",
                 "DependenceVariance", "DependenceEntropy", "LowGrayLevelEmphasis", "HighGrayLevelEmphasis",
                 "SmallDependenceLowGrayLevelEmphasis", "SmallDependenceHighGrayLevelEmphasis",
                 "LargeDependenceLowGrayLevelEmphasis", "LargeDependenceHighGrayLevelEmphasis"]),
    "ngtdm": (2, ["Coarseness", "Contrast", "Busyness", "Complexity", "Strength"]),
}
VOXEL_GLRLM_FEATURES = _ZONE_LIKE["glrlm"][1]
VOXEL_GLSZM_FEATURES = _ZONE_LIKE["glszm"][1]
VOXEL_GLDM_FEATURES = [f for f in _ZONE_LIKE["gldm"][1] if f]
VOXEL_NGTDM_FEATURES = _ZONE_LIKE["ngtdm"][1]


def voxel_texture_features(cls, image, mask, distances, Ng, force2D, force2Ddimension, kernelRadius, voxels, features,
                           alpha=0):
    """-> {feature name: float64 [Nvox]} of feature class `cls` ("glrlm" | "glszm" | "gldm" | "ngtdm") for the kernels
    centred on `voxels` (int [Nd, Nvox]).  Raises NotImplementedError when the fused kernels do not cover the request
    (unknown / deprecated feature, Ng > 255, more than 32 angles, kernels above 512 voxels): the caller then builds
    the matrices with calculate_* and uses the numpy formulas."""
    engine = _engine()
    family, table = _ZONE_LIKE[cls]
    missing = [f for f in features if f not in table]
    if missing:
        raise NotImplementedError("not available in the fused voxel kernel: %s" % ", ".join(missing))
    ids = [table.index(f) for f in features]
    vox = voxels if _on_device(voxels) else _to_device(np.ascontiguousarray(np.asarray(voxels).astype(np.intc, copy=False)))
    try:
        out = engine.voxel_texture_features(family, _to_device(image, integer=True), _to_device(mask), Ng, vox, ids,
                                            kernelRadius, force2D, force2Ddimension,
                                            [int(d) for d in np.asarray(distances).ravel()], alpha)
    except NotImplementedError:
        raise
    out = out.cpu().numpy()
    return {f: out[i] for i, f in enumerate(features)}


# ---- segment-mode features evaluated on the device matrices (prad_glcm_features_dev / prad_zone_matrix_features_dev)
def _angle_mean(per_angle, empty):
    """np.nanmean over the angles the reference keeps (all-empty angles are deleted, e.g. glcm.py:186-198)"""
    kept = per_angle[~empty] if empty.any() else per_angle
    if kept.shape[0] == 0:
        return np.full(per_angle.shape[1], np.nan)
    if not np.isnan(kept).any():
        return kept.mean(0)          # (what nanmean computes without a NaN: sum over the angles / their number)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(kept, 0)


def _mcc_angle_mean(per_angle):
    """MCC of a segment from its per-angle values, as the feature class reports it: np.nanmean over the flat vector (empty
    angles are NaN and drop out).  The batched label route calls this too: a 1-D mean and the column mean of _angle_mean add
    the angles in different orders, and the two must agree to the last bit."""
    import warnings
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return float(np.nanmean(per_angle))


def segment_features(cls, image, mask, Ng, features, distances=(1,), force2D=False, force2Ddimension=0, alpha=0,
                     symmetrical=True, Ns=None):
    """-> {feature name: float} of feature class `cls` ("glcm" | "glrlm" | "glszm" | "gldm" | "ngtdm") in segment mode with the
    matrix AND the formulas on the device; image / mask are device tensors (discretised levels, ROI).
    Raises NotImplementedError for features outside the fused set (MCC, deprecated ones)."""
    return segment_features_enqueue(cls, image, mask, Ng, features, distances, force2D, force2Ddimension, alpha,
                                    symmetrical, Ns, deferred=False)()


def segment_image_enqueue(levels, mask, Ng, Ns, requests, force2D=False, force2Ddimension=0):
    """The enqueue half of segment_features_enqueue / firstorder_stats_enqueue for SEVERAL classes of one derived image in
    one library call (engine.image_enqueue).  requests: {class key: dict} with "features" (names) and, per class,
    "symmetrical" (glcm), "alpha" (gldm), "raw" + "shift" (firstorder).  Returns (token, {class key: finish}); finish() as
    returned by the per-class functions, to be called after segment_image_wait(token).  Classes whose request the fused
    kernels do not cover are left out of the returned dict (the caller queues them one by one)."""
    engine = _engine()
    bits = {"glcm": engine.IMG_GLCM, "glrlm": engine.IMG_GLRLM, "gldm": engine.IMG_GLDM, "ngtdm": engine.IMG_NGTDM,
            "glszm": engine.IMG_GLSZM, "firstorder": engine.IMG_FIRSTORDER}
    classes, take = 0, {}
    for cls, rq in requests.items():
        if cls == "firstorder":
            take[cls] = rq
            classes |= bits[cls]
            continue
        table = VOXEL_GLCM_FEATURES if cls == "glcm" else _ZONE_LIKE[cls][1]
        feats = [f for f in rq["features"] if not (cls == "glcm" and f == "MCC")]
        if cls not in bits or any(f not in table for f in feats):
            continue
        take[cls] = dict(rq, table=table, feats=feats, mcc=(cls == "glcm" and "MCC" in rq["features"]))
        classes |= bits[cls] | (engine.IMG_MCC if take[cls]["mcc"] else 0)
    if not classes:
        return None, {}
    fo = take.get("firstorder")
    tok = engine.image_enqueue(levels, mask, fo["raw"] if fo else None, int(Ng), int(Ns), classes,
                               symmetric=take.get("glcm", {}).get("symmetrical", True), alpha=int(take.get("gldm", {}).get("alpha", 0)),
                               force2D=force2D, force2Ddimension=force2Ddimension,
                               voxelArrayShift=float(fo["shift"]) if fo else 0.0)
    # (with the image launcher the result block and its layout arrive with segment_image_wait: everything below reads them
    #  from the token when it runs, i.e. after the wait; a class the device route declined -- layout -1 -- then says so)
    def flags(k, count):
        res, lay = tok["res"], tok["layout"]
        return res[lay[k]:lay[k] + (count + 1) // 2 + 1].view(np.int32)[:count]

    def named(rq, vals):
        return dict(zip(rq["feats"], vals[rq["idx"]].tolist()))

    def part(k, count):
        res, lay = tok["res"], tok["layout"]
        if lay[k] < 0:
            raise NotImplementedError("declined by the device route")
        return res[lay[k]:lay[k] + count]

    for rq in take.values():
        if "table" in rq:
            rq["idx"] = np.array([rq["table"].index(f) for f in rq["feats"]], dtype=np.intp)
    out = {}
    if "glcm" in take:
        rq = take["glcm"]

        def fin_glcm(rq=rq):
            res, lay = tok["res"], tok["layout"]
            Na = lay[11]
            vals = part(0, Na * 23).reshape(Na, 23)
            r = named(rq, _angle_mean(vals, flags(1, Na) != 0)) if rq["feats"] else {}
            if rq["mcc"] and lay[2] >= 0 and res[lay[2] + Na] == 0:
                r["MCC"] = _mcc_angle_mean(res[lay[2]:lay[2] + Na])
            return r
        out["glcm"] = fin_glcm
    if "glrlm" in take:
        def fin_glrlm(rq=take["glrlm"]):
            Na = tok["layout"][11]
            return named(rq, _angle_mean(part(3, Na * 16).reshape(Na, 16), flags(4, Na) != 0))
        out["glrlm"] = fin_glrlm
    if "gldm" in take:
        out["gldm"] = lambda rq=take["gldm"]: named(rq, _angle_mean(part(5, 16).reshape(1, 16), flags(6, 1) != 0))
    if "ngtdm" in take:
        out["ngtdm"] = lambda rq=take["ngtdm"]: named(rq, part(7, 5))
    if "glszm" in take:
        def fin_glszm(rq=take["glszm"]):
            vals = part(8, 17) if tok["layout"][8] >= 0 else None
            if vals is None or vals[16] != 0:       # the one-queue route or its device-side ranking declined / the reference's IndexError: the exact route
                P, sizes = engine.glszm_compact(levels, mask, int(Ng), Ns, force2D, force2Ddimension)
                if len(sizes) == 0:
                    raise NotImplementedError("no zones")
                return named(rq, _angle_mean(*engine.zone_matrix_features(P, sizes)))
            if flags(9, 1)[0] != 0:
                raise NotImplementedError("no zones")
            return named(rq, vals[:16])
        out["glszm"] = fin_glszm
    if fo is not None:
        def fin_fo():
            lay = tok["layout"]
            vals = part(10, 16) if lay[10] >= 0 else None
            if vals is None or vals[15] != 0:
                return engine.firstorder_stats(_to_device(fo["raw"]), _to_device(mask), fo["shift"])
            return dict(zip(engine.FIRSTORDER_FIELDS, vals[:15].tolist()))
        out["firstorder"] = fin_fo
    lay = tok.get("layout")
    if lay is not None:
        # issued by this thread (no launcher): what the device route declined is known already -- those classes are left out
        # and the caller queues them on its own; with the launcher the same is found out when the closure runs
        for cls, k in (("glcm", 0), ("glrlm", 3), ("gldm", 5), ("ngtdm", 7), ("glszm", 8), ("firstorder", 10)):
            if lay[k] < 0:
                out.pop(cls, None)
    return tok, out


def segment_image_wait(token):
    engine = _engine()
    return engine.image_wait(token)


SEGMENT_QUEUES = {"glcm": 0, "glrlm": 0, "gldm": 0, "ngtdm": 0, "glszm": 1, "firstorder": 2}


def segment_sync():
    """waits for everything segment_features_enqueue queued (inside segment_queue()); False when a queued call met a level
    outside [1, Ng] under the mask (the values are void: compute synchronously, which raises what the reference raises)"""
    engine = _engine()
    from . import _lib
    ok = True
    for k in sorted(set(SEGMENT_QUEUES.values())):
        try:
            with engine.side_queue(k, wait=False):
                engine.deferred_status()
        except _lib.DeferredLevelsError:
            ok = False
    return ok


def segment_mark(classes=None):
    """token behind everything queued inside segment_queue() so far (engine.deferred_mark on every side stream the
    classes use)"""
    engine = _engine()
    used = sorted(set(SEGMENT_QUEUES.get(c, 0) for c in (classes or SEGMENT_QUEUES)))
    marks = []
    for k in used:
        with engine.side_queue(k, wait=False):
            marks.append((k, engine.deferred_mark()))
    return marks


def segment_wait(token):
    """waits for the work in front of the token; False when its values are void (see segment_sync)"""
    engine = _engine()
    ok = True
    for k, mark in token:
        with engine.side_queue(k, wait=False):
            ok = engine.deferred_wait(mark) and ok
    return ok


def segment_queue(cls=None):
    """context manager around the enqueue calls of one feature class of a derived image: they go to the class's side stream
    (engine.side_queue) so that the classes evaluated synchronously meanwhile do not wait for them"""
    engine = _engine()
    return engine.side_queue(SEGMENT_QUEUES.get(cls, 0))


ENQUEUE_CLASSES = ("glcm", "glrlm", "gldm", "ngtdm", "glszm")


def segment_features_enqueue(cls, image, mask, Ng, features, distances=(1,), force2D=False, force2Ddimension=0, alpha=0,
                             symmetrical=True, Ns=None, deferred=True):
    """segment_features in two halves, for the case pipeline (featureextractor.computeFeatures): with deferred=True the
    matrix and feature kernels of `cls` are only ENQUEUED on the current stream, their values land in the library's
    result arena; the returned finish() -> {feature name: float} may be called once engine.deferred_status() has
    synchronised the stream (and not raised: a level outside [1, Ng] voids the values).  No reference analogue (the reference evaluates class after class on the host, base.py:181-198)."""
    engine = _engine()
    dist = [int(d) for d in np.asarray(distances).ravel()]
    if cls == "glcm":
        table = VOXEL_GLCM_FEATURES
    else:
        table = _ZONE_LIKE[cls][1]
    want_mcc = cls == "glcm" and "MCC" in features
    features = [f for f in features if not (cls == "glcm" and f == "MCC")]
    missing = [f for f in features if f not in table]
    if missing:
        raise NotImplementedError("not available in the fused segment kernels: %s" % ", ".join(missing))
    dfr = bool(deferred) and cls in ENQUEUE_CLASSES

    def named(vals):
        return {f: float(vals[table.index(f)]) for f in features}

    def mean_of(pair):
        return _angle_mean(pair[0], np.asarray(pair[1]) != 0)

    if cls == "glcm":
        if dist == [1]:
            g = _dev_pairs_runs(image, mask, Ng, force2D, force2Ddimension, "glcm", deferred=dfr)["glcm_dev"]
        else:
            g, _ = engine.glcm(image, mask, int(Ng), dist, force2D, force2Ddimension)
        pair = engine.glcm_features(g, symmetrical, deferred=dfr) if features else None
        mcc = None
        if want_mcc:
            try:     # (absent from the result when more than 64 grey levels occur: the caller's host route takes it)
                mcc = engine.glcm_mcc(g, symmetrical, deferred=dfr)
            except NotImplementedError:
                mcc = None

        def finish():
            res = named(mean_of(pair)) if features else {}
            if mcc is not None and not (dfr and mcc[-1] != 0):
                res["MCC"] = _mcc_angle_mean(mcc[:-1] if dfr else mcc)
            return res
        return finish
    if cls == "glrlm":
        r = _dev_pairs_runs(image, mask, Ng, force2D, force2Ddimension, "glrlm", deferred=dfr)["glrlm_dev"]
        pair = engine.zone_matrix_features(r, np.arange(1, r.shape[1] + 1), deferred=dfr)
    elif cls == "gldm":
        P = _dev_gldm_ngtdm(image, mask, Ng, alpha, dist, force2D, force2Ddimension, dfr)[0]
        pair = engine.zone_matrix_features(P, np.arange(1, P.shape[1] + 1), deferred=dfr)
    elif cls == "glszm":
        def three_calls():
            P, sizes = engine.glszm_compact(image, mask, int(Ng), Ns, force2D, force2Ddimension)
            if len(sizes) == 0:
                raise NotImplementedError("no zones")
            return named(mean_of(engine.zone_matrix_features(P, sizes)))
        try:        # zones, ranked sizes, compact matrix and formulas in one queue (no host round trip in between)
            vals, none = engine.glszm_features(image, mask, int(Ng), Ns, force2D, force2Ddimension, deferred=dfr)
        except NotImplementedError:
            return three_calls

        def finish():
            if vals[16] != 0:           # the device-side ranking declined / the reference's IndexError: the exact route
                return three_calls()
            if none[0] != 0:
                raise NotImplementedError("no zones")
            return named(vals[:16])
        return finish
    elif cls == "ngtdm":
        vals = engine.ngtdm_features(_dev_gldm_ngtdm(image, mask, Ng, None, dist, force2D, force2Ddimension, dfr)[1],
                                     deferred=dfr)
        return lambda: named(vals)
    else:
        raise NotImplementedError(cls)
    return lambda: named(mean_of(pair))


# ---- first-order statistics (no native code in the reference: radiomics/firstorder.py is numpy; here the ROI /
# ---- the kernels are reduced on the device, see include/pyradiomics_amd.h) ----------------------------------
FIRSTORDER_FEATURES = ["Energy", "TotalEnergy", "Entropy", "Minimum", "10Percentile", "90Percentile", "Maximum", "Mean",
                       "Median", "InterquartileRange", "Range", "MeanAbsoluteDeviation",
                       "RobustMeanAbsoluteDeviation", "RootMeanSquared", "StandardDeviation", "Skewness", "Kurtosis",
                       "Variance", "Uniformity"]


def _to_device(a, integer=False):
    import torch
    if _on_device(a):
        return a
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    elif integer:
        a = a.astype(np.intc, copy=False)
    elif a.dtype not in (np.float32, np.float64, np.int32, np.int16):
        a = a.astype(np.float64)
    return torch.from_numpy(a).to(torch.device("cuda", torch.cuda.current_device()))


def firstorder_stats(image, mask, voxelArrayShift=0.0):
    """-> {Np, Energy, Minimum, P10, P25, Median, P75, P90, Maximum, Mean, MAD, rMAD, m2, m3, m4} of image[mask]
    (numpy arrays are uploaded, device tensors used in place)"""
    engine = _engine()
    return engine.firstorder_stats(_to_device(image), _to_device(mask), voxelArrayShift)


def firstorder_stats_enqueue(image, mask, roi_count, voxelArrayShift=0.0):
    """firstorder_stats in two halves for the case pipeline: the passes are queued on the current stream (no host round
    trip between them, engine.firstorder_stats_queue); the returned finish() -> dict may be called once the stream has
    been waited for and falls back to firstorder_stats when the queued chain declined (verdict word).
    NotImplementedError: not an image for the queue (integer dtype, small ROI)."""
    engine = _engine()
    img, msk = _to_device(image), _to_device(mask)
    vals = engine.firstorder_stats_queue(img, msk, int(roi_count), voxelArrayShift, deferred=True)

    def finish():
        if vals[15] != 0:
            return engine.firstorder_stats(img, msk, voxelArrayShift)
        return dict(zip(engine.FIRSTORDER_FIELDS, (float(v) for v in vals[:15])))
    return finish


def voxel_firstorder(image, mask, levels, voxels, kernelRadius, bbsize, force2D, force2Ddimension, voxelArrayShift,
                     voxelVolume, features):
    """-> {feature name: float64 [Nvox]} for the kernels centred on `voxels` (int [Nd, Nvox])"""
    engine = _engine()
    ids = [FIRSTORDER_FEATURES.index(f) for f in features]
    vox = _to_device(np.ascontiguousarray(np.asarray(voxels).astype(np.intc, copy=False))) if not _on_device(voxels) else voxels
    out = engine.voxel_firstorder(_to_device(image), _to_device(mask), _to_device(levels, integer=True), vox, ids,
                                  kernelRadius, force2D, force2Ddimension, bbsize, voxelArrayShift, voxelVolume)
    out = out.cpu().numpy()
    return {f: out[i] for i, f in enumerate(features)}


def generate_angles(size, distances, bidirectional, force2D, force2Ddimension):
    """-> int32 [Na, Nd];  _cmatrices.c:882-924"""
    size = np.ascontiguousarray(np.asarray(size).astype(np.intc, copy=False))
    if size.ndim != 1:
        raise ValueError("Expected a 1D array for size")
    return _build_angles(size, distances, bidirectional, int(force2Ddimension) if force2D else -1).copy()


# ---- fused voxel-based GLCM features (no reference analogue: replaces calculate_glcm + numpy feature math in
# ---- voxel mode, see include/pyradiomics_amd.h) -------------------------------------------------------------
VOXEL_GLCM_FEATURES = ["Autocorrelation", "JointAverage", "ClusterProminence", "ClusterShade", "ClusterTendency",
                       "Contrast", "Correlation", "DifferenceAverage", "DifferenceEntropy", "DifferenceVariance",
                       "JointEnergy", "JointEntropy", "Imc1", "Imc2", "Idm", "Idmn", "Id", "Idn", "InverseVariance",
                       "MaximumProbability", "SumAverage", "SumEntropy", "SumSquares"]


def voxel_glcm_features(image, mask, distances, Ng, force2D, force2Ddimension, kernelRadius, voxels, features,
                        symmetrical=True):
    """-> {feature name: float64 [Nvox]} for the kernels centred on `voxels` (int [Nd, Nvox]).
    Raises NotImplementedError when the fused kernel does not cover the request (Ng > 64, MCC, ...): the caller
    then uses calculate_glcm and the numpy feature formulas."""
    want_mcc = "MCC" in features
    all_features, features = features, [f for f in features if f != "MCC"]
    unknown = [f for f in features if f not in VOXEL_GLCM_FEATURES]
    if unknown:
        raise NotImplementedError("not available in the fused voxel kernel: %s" % ", ".join(unknown))
    img, msk, size, vox, Nvox, f2d, angles = _common(image, mask, distances, False, force2D, force2Ddimension,
                                                     kernelRadius, voxels)
    if vox is None:
        raise RuntimeError("voxel_glcm_features needs a voxel list")
    Na, Nd = angles.shape
    mcc = None
    if want_mcc:      # its own kernel (one Jacobi eigenvalue iteration per kernel and angle, csrc/kernels_mcc.h)
        mcc = np.empty(Nvox, dtype=np.float64)
        rc = _lib.load().prad_voxel_glcm_mcc(_vptr(img), _vptr(msk), _iptr(size), Nd, _iptr(angles), Na, int(Ng), Nvox,
                                             _vptr(vox), int(kernelRadius), f2d, 1 if symmetrical else 0, _vptr(mcc))
        _lib.raise_for(rc, "voxel GLCM MCC")
        if not features:
            return {"MCC": mcc}
    ids = np.array([VOXEL_GLCM_FEATURES.index(f) for f in features], dtype=np.intc)
    out = np.empty((len(ids), Nvox), dtype=np.float64)
    empty = np.empty(Nvox, dtype=np.uint32)
    anyne = np.zeros(1, dtype=np.uint32)
    rc = _lib.load().prad_voxel_glcm_features(_vptr(img), _vptr(msk), _iptr(size), Nd, _iptr(angles), Na, int(Ng),
                                              Nvox, _vptr(vox), int(kernelRadius), f2d, 1 if symmetrical else 0,
                                              _iptr(ids), len(ids), _vptr(out), _vptr(empty), _vptr(anyne))
    _lib.raise_for(rc, "voxel GLCM features")
    res = {f: out[i] for i, f in enumerate(features)}
    if "JointAverage" in res:
        # glcm.py:292 takes a plain mean over the angles kept for the batch: NaN wherever a kernel lacks an angle
        # that some other kernel of the batch has
        res["JointAverage"] = np.where((empty & anyne[0]) != 0, np.nan, res["JointAverage"])
    if mcc is not None:
        res["MCC"] = mcc
    return res

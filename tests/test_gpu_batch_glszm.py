"""Batched small-ROI GLSZM (engine.glszm_batch, engine.glszm_batch_zones, cmatrices.calculate_glszm_batch,
prad_batch_glszm_dev + prad_batch_glszm_fill_dev): every ROI of every batch against the reference C, called per ROI through
the oracle binding (checker.calculate_glszm -- the dense matrix), and against the scipy restatement tests/glszm_reference.py for
what the reference's wrapper does not hand out (the ordered zone list, the compact layout) and for the 1 x 1 x 1 box it refuses.
The single device calls are a second witness.  Everything is integer and exact: there is no tolerance in this module.

Shapes are the smallest at which the kernel can still go wrong: a ragged batch with unaligned offsets, axes of length 1 and 2
and one box of exactly PRAD_BATCH_GLSZM_MAX_VOX voxels; the topologies on which the label propagation is slowest (one-voxel
paths along every axis, one of them through a box of exactly the cap: the termination test -- the kernel does not hand out its
sweep count, so none is stated or asserted); more ROIs than compute units; empty / full / one-voxel masks; 1 and 64 levels;
every voxel a zone of its own (the zone list fills its capacity); a bad level; the declined domain and the mixed route."""
import ctypes as C

import numpy as np
import pytest

import glszm_reference as gr
from test_gpu_batch_rois import RAGGED as _RAGGED4
from test_gpu_glszm_topology import checkerboard, combs, helix, serpentine

pytestmark = pytest.mark.gpu

MAX_VOX = (160 * 1024 - 256) // 3          # PRAD_BATCH_GLSZM_MAX_VOX (csrc/kernels_batch_glszm.h)
RAGGED = _RAGGED4[:-1] + [(24, 32, 71)]
assert 24 * 32 * 71 == MAX_VOX == 213 * 256


def _rois(shapes, Ng, seed, fill=0.6):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(1, Ng + 1, size=s).astype(np.int32) for s in shapes]
    masks = [rng.random(s) < fill for s in shapes]
    return imgs, masks


def _dev(imgs, masks):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(i)).to("cuda:0") for i in imgs], [torch.from_numpy(np.ascontiguousarray(m)).to("cuda:0") for m in masks]


def _truth(checker, img, mask, Ng):
    """one ROI: {"zones": int [nzones, 2] in discovery order, "summary", "dense" (the reference C where its wrapper takes the box,
    the restatement for 1 x 1 x 1), "compact": (P, sizes)}, or None where the reference raises IndexError"""
    img, mask = np.ascontiguousarray(img, dtype=np.int32), np.ascontiguousarray(mask, dtype=bool)
    if mask.any() and (img[mask].min() < 1 or img[mask].max() > Ng):
        if img.size > 1:
            with pytest.raises(IndexError):
                checker.calculate_glszm(img, mask, Ng, max(1, int(mask.sum())), False, 0)
        return None
    z = gr.zones(img, mask)
    dense = gr.matrix(z, Ng)[0]
    if img.size > 1:
        ref = checker.calculate_glszm(img, mask, Ng, max(1, int(mask.sum())), False, 0)[0]
        assert np.array_equal(ref, dense), "the restatement and the reference C disagree"
        dense = ref
    sizes = np.unique(z[:, 1]) if len(z) else np.zeros(0, np.int64)
    summary = [len(z), int(z[:, 1].max()) if len(z) else 0, len(sizes)]
    return {"zones": z[:, :2].astype(np.int32).reshape(-1, 2), "summary": summary, "dense": dense, "compact": gr.compact(z, Ng)}


def _assert_batched_route(route="batch"):
    from pyradiomics_amd import _lib, engine
    assert engine.last_batch_route() == route and _lib.last_path() == "batch" and _lib.last_variant() == "batch-glszm-lds"


def _check_results(truths, dense, comp, status, zones=None, summary=None):
    """dense / comp: results of glszm_batch(compact=False / True) (device tensors or numpy), either may be None"""
    def host(t):
        return t.cpu().numpy() if hasattr(t, "cpu") else t
    for b, want in enumerate(truths):
        what = "ROI %d" % b
        if want is None:
            assert status[b] == 0, "%s: the reference raises IndexError" % what
            want = {"zones": np.zeros((0, 2), np.int32), "summary": [0, 0, 0], "dense": np.zeros_like(host(dense[b])) if dense is not None else None,
                    "compact": (np.zeros((host(comp[b][0]).shape[0], 0)), np.zeros(0, np.int32)) if comp is not None else None}
        else:
            assert status[b] == 1, "%s status %d" % (what, status[b])
        if zones is not None:
            assert list(summary[b]) == want["summary"], "%s summary %s != %s" % (what, list(summary[b]), want["summary"])
            got = host(zones[b])
            assert got.shape == want["zones"].shape and np.array_equal(got, want["zones"]), "%s zone list (pairs or order)" % what
        if dense is not None:
            got = host(dense[b])
            assert got.dtype == np.float64 and got.shape == want["dense"].shape, "%s dense shape %s != %s" % (what, got.shape, want["dense"].shape)
            assert np.array_equal(got, want["dense"]), "%s dense matrix" % what
        if comp is not None:
            P, sizes = host(comp[b][0]), comp[b][1]
            assert sizes.dtype == np.int32 and np.array_equal(sizes, want["compact"][1]), "%s sizes" % what
            assert P.shape == want["compact"][0].shape and np.array_equal(P, want["compact"][0]), "%s compact matrix" % what


def _run_and_check(checker, imgs, masks, Ng, route="batch"):
    from pyradiomics_amd import engine
    truths = [_truth(checker, i, m, Ng) for i, m in zip(imgs, masks)]
    dl, dm = _dev(imgs, masks)
    comp, st_c = engine.glszm_batch(dl, dm, None, Ng)
    if route is not None:
        _assert_batched_route(route)
    dense, st_d = engine.glszm_batch(dl, dm, None, Ng, compact=False)
    if route is not None:
        _assert_batched_route(route)
    assert st_c == st_d
    zones = summary = None
    if route == "batch":
        zones, summary, st_z = engine.glszm_batch_zones(dl, dm, None, Ng)
        assert st_z.tolist() == st_c
    _check_results(truths, dense, comp, st_c, zones, summary)
    return {"truths": truths, "dev": (dl, dm), "dense": dense, "comp": comp, "status": st_c, "zones": zones, "summary": summary}


@pytest.fixture(scope="module")
def ragged(checker):
    """the ragged batch, its reference and the batched results of the default stream: computed once"""
    Ng = 16
    imgs, masks = _rois(RAGGED, Ng, seed=20261)
    masks[0][:] = True
    res = _run_and_check(checker, imgs, masks, Ng)
    res.update(Ng=Ng, imgs=imgs, masks=masks)
    return res


def test_ragged_batch(ragged):
    from pyradiomics_amd import engine
    Ng = ragged["Ng"]
    assert engine.batch_glszm_max_vox() == MAX_VOX
    # odd voxel counts: the ROIs after the first start at elements that are no multiple of 4
    starts = np.cumsum([0] + [int(np.prod(s)) for s in RAGGED])[:-1]
    assert any(s % 4 for s in starts[1:])
    assert ragged["status"] == [1] * len(RAGGED)
    assert ragged["dense"][0].shape == (Ng, 1) and ragged["summary"][0].tolist() == [1, 1, 1]
    # second witness: the single device calls on two boxes
    dl, dm = ragged["dev"]
    for b in (4, 6):
        assert np.array_equal(ragged["dense"][b].cpu().numpy(), engine.glszm(dl[b], dm[b], Ng).cpu().numpy())
        P, sizes = engine.glszm_compact(dl[b], dm[b], Ng)
        assert np.array_equal(ragged["comp"][b][0].cpu().numpy(), P.cpu().numpy()) and np.array_equal(ragged["comp"][b][1], sizes)


SLOW_SHAPES = [(6, 10, 12), (3, 40, 40)]


def _slow_volumes():
    vols = []
    for shape in SLOW_SHAPES:
        vols += [serpentine(shape), helix(shape), combs(shape), checkerboard(shape, 2)]
        # the same path along the other two axes: the serpentine of the permuted shape, transposed back onto `shape`
        for axes in ((2, 0, 1), (1, 2, 0)):
            src = tuple(shape[axes.index(d)] for d in range(3))
            vols.append(serpentine(src).transposed(axes))
    return vols


def test_slowest_topologies(checker):
    """one-voxel paths, spirals, combs and corner contacts, all in ONE batch; the closed-form census of every generator is a
    third witness"""
    vols = _slow_volumes()
    assert sorted(set(v.img.shape for v in vols)) == sorted(SLOW_SHAPES)
    Ng = 3
    res = _run_and_check(checker, [v.img for v in vols], [v.mask for v in vols], Ng)
    for v, z in zip(vols, res["zones"]):
        assert gr.census(np.c_[z.cpu().numpy().astype(np.int64), np.zeros(len(z), np.int64)]) == v.cen, v.name


def test_serpentine_through_a_box_of_exactly_the_cap(checker):
    """1 x 213 x 256 = 54528 voxels: 107 lanes of 256 voxels joined at alternating ends are ONE zone whose path visits every
    second row in turn.  The termination and iteration-count test: the sweeps are not handed out by the kernel, so no number is
    stated here; the test passes when the labelling ends in the reference's state."""
    v = serpentine((1, 213, 256))
    assert v.img.size == MAX_VOX and v.cen[(1, 107 * 256 + 106)] == 1
    res = _run_and_check(checker, [v.img], [v.mask], 2)
    assert res["summary"][0].tolist()[:2] == [1 + 106, 107 * 256 + 106]
    assert res["zones"][0][0].tolist() == [1, 107 * 256 + 106]


def test_more_rois_than_compute_units(checker):
    B, Ng = 300, 8
    imgs, masks = _rois([(4, 4, 4)] * B, Ng, seed=3, fill=0.5)
    res = _run_and_check(checker, imgs, masks, Ng)          # all 300: none skipped, none written twice
    assert res["status"] == [1] * B


def test_masks_empty_full_single_voxel(checker):
    Ng = 6
    imgs, masks = _rois([(4, 5, 6)] * 3, Ng, seed=4)
    masks[0][:] = False
    masks[1][:] = True
    imgs[1][:] = 4
    masks[2][:] = False
    masks[2][2, 3, 1] = True
    res = _run_and_check(checker, imgs, masks, Ng)
    assert [tuple(d.shape) for d in res["dense"]] == [(Ng, 1), (Ng, 120), (Ng, 1)]
    assert res["summary"].tolist() == [[0, 0, 0], [1, 120, 1], [1, 1, 1]]
    assert not res["dense"][0].any() and res["dense"][1][3, 119].item() == 1 and res["dense"][1].sum().item() == 1
    assert res["comp"][0][0].shape == (Ng, 0) and res["comp"][1][1].tolist() == [120]


@pytest.mark.parametrize("Ng", [1, 64])
def test_level_extremes(checker, Ng):
    shapes = [(5, 6, 7), (6, 9, 4), (5, 6, 7)]
    imgs, masks = _rois(shapes, Ng, seed=50 + Ng)
    imgs[0].flat[0], imgs[0].flat[-1] = 1, Ng
    masks[0].flat[0] = masks[0].flat[-1] = True
    imgs[2][:] = min(Ng, 3)
    masks[2][:] = True
    res = _run_and_check(checker, imgs, masks, Ng)
    assert res["summary"][2].tolist() == [1, 210, 1]
    if Ng == 64:
        assert res["dense"][0][0].sum().item() >= 1 and res["dense"][0][63].sum().item() >= 1


def test_singles(checker):
    """every masked voxel a zone of its own.  Under the full neighbourhood two levels cannot do that (a 3-D checkerboard of two
    levels joins across its face and body diagonals: it is in the batch, under a random mask, checked against the reference
    only), so the colour is the parity of every coordinate (8 colours, levels 1 .. 8) under the same kind of mask; and a full
    4 x 4 x 4 box with 64 distinct levels, whose zone list fills its capacity of 2 * nvox ints"""
    rng = np.random.default_rng(9)
    shape = (5, 6, 7)
    z, y, x = np.indices(shape)
    img = (1 + (x & 1) + 2 * (y & 1) + 4 * (z & 1)).astype(np.int32)
    two = (1 + ((x + y + z) & 1)).astype(np.int32)
    mask = rng.random(shape) < 0.7
    full = (1 + np.arange(64, dtype=np.int32)).reshape(4, 4, 4)
    res = _run_and_check(checker, [img, full, two], [mask, np.ones((4, 4, 4), bool), mask], 64)
    assert res["summary"][0].tolist() == [int(mask.sum()), 1, 1]
    assert res["summary"][1].tolist() == [64, 1, 1] and res["zones"][1].shape == (64, 2)
    assert res["zones"][1][:, 0].tolist() == list(range(1, 65))


def test_bad_level_voids_one_roi_only(checker):
    Ng = 8
    imgs, masks = _rois([(4, 4, 4), (5, 3, 7), (2, 9, 3), (6, 6, 6)], Ng, seed=7)
    imgs[1][2, 1, 4] = 0
    masks[1][2, 1, 4] = True
    imgs[2][0, 0, 0] = 0          # a level 0 OUTSIDE the mask is no error
    masks[2][0, 0, 0] = False
    imgs[3][1, 1, 1] = Ng + 1
    masks[3][1, 1, 1] = True
    res = _run_and_check(checker, imgs, masks, Ng)
    assert res["status"] == [1, 0, 1, 0]
    assert res["summary"][1].tolist() == [0, 0, 0] and res["dense"][3].shape == (Ng, 1) and not res["dense"][3].any()


def _raw_label(lib, dl, dm, shapes, Ng):
    """prad_batch_glszm_dev on sentinel-filled outputs -> (rc, zones, summary, status)"""
    import torch
    sizes = np.array(shapes, dtype=np.intc)
    off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])[:-1]]).astype(np.int64)
    flat_l, flat_m = torch.cat([t.reshape(-1) for t in dl]), torch.cat([t.reshape(-1) for t in dm]).view(torch.uint8)
    zones = torch.full((2 * flat_l.numel(),), -7, dtype=torch.int32, device="cuda:0")
    summary = torch.full((len(shapes), 3), -7, dtype=torch.int32, device="cuda:0")
    status = torch.full((len(shapes),), -7, dtype=torch.int32, device="cuda:0")
    rc = lib.prad_batch_glszm_dev(C.c_void_p(flat_l.data_ptr()), C.c_void_p(flat_m.data_ptr()), sizes.ctypes.data_as(C.POINTER(C.c_int)),
                                  off.ctypes.data_as(C.POINTER(C.c_longlong)), len(shapes), Ng, C.c_void_p(zones.data_ptr()),
                                  C.c_void_p(summary.data_ptr()), C.c_void_p(status.data_ptr()),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, zones, summary, status


def test_out_of_domain_is_declined(checker):
    from pyradiomics_amd import _lib, engine
    lib = _lib.load()
    n = engine.batch_glszm_max_vox() + 1
    over = next((1, d, n // d) for d in range(2, 400) if n % d == 0)          # cap + 1 voxels in one ROI
    assert int(np.prod(over)) == MAX_VOX + 1
    for shapes, Ng in (([over], 4), ([(3, 4, 5), (2, 2, 2)], 65)):
        imgs, masks = _rois(shapes, Ng, seed=8)
        dl, dm = _dev(imgs, masks)
        engine.glszm(dl[0], dm[0], Ng)
        before = _lib.last_path()
        rc, zones, summary, status = _raw_label(lib, dl, dm, shapes, Ng)
        assert rc == _lib.PRAD_E_UNSUPPORTED and _lib.last_path() == before
        assert (zones == -7).all().item() and (summary == -7).all().item() and (status == -7).all().item()
        with pytest.raises(NotImplementedError):
            engine.glszm_batch_zones(dl, dm, None, Ng)


def test_mixed_and_looped_routes(checker):
    from pyradiomics_amd import engine
    Ng = 5
    imgs, masks = _rois([(3, 4, 5), (40, 40, 40), (6, 2, 7)], Ng, seed=11)
    res = _run_and_check(checker, imgs, masks, Ng, route=None)
    assert engine.last_batch_route() == "mixed" and res["status"] == [1, 1, 1]
    # 65 levels: every ROI through the single calls; the 1 x 1 x 1 box and the bad level are answered as the native route does
    Ng = 65
    imgs, masks = _rois([(3, 4, 5), (1, 1, 1), (4, 2, 6), (2, 3, 2)], Ng, seed=12)
    imgs[0].flat[0], masks[0].flat[0] = Ng, True
    masks[1][:] = True
    imgs[3][1, 1, 1], masks[3][1, 1, 1] = Ng + 1, True
    res = _run_and_check(checker, imgs, masks, Ng, route=None)
    assert engine.last_batch_route() == "looped" and res["status"] == [1, 1, 1, 0]


def test_host_route_equals_device_route(ragged):
    from pyradiomics_amd import cmatrices as cm
    dense, status = cm.calculate_glszm_batch(ragged["imgs"], ragged["masks"], ragged["Ng"])
    assert cm.last_batch_route() == "batch" and status == ragged["status"]
    comp, status = cm.calculate_glszm_batch(ragged["imgs"], ragged["masks"], ragged["Ng"], compact=True)
    _assert_batched_route()
    assert all(isinstance(d, np.ndarray) for d in dense) and all(isinstance(p, np.ndarray) for p, _ in comp)
    for b in range(len(RAGGED)):
        assert np.array_equal(dense[b], ragged["dense"][b].cpu().numpy())
        assert np.array_equal(comp[b][0], ragged["comp"][b][0].cpu().numpy()) and np.array_equal(comp[b][1], ragged["comp"][b][1])
    _check_results(ragged["truths"], dense, comp, status)


def test_side_stream(ragged):
    import torch
    from pyradiomics_amd import engine
    dl, dm = ragged["dev"]
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        comp, status = engine.glszm_batch(dl, dm, None, ragged["Ng"])
        dense, _ = engine.glszm_batch(dl, dm, None, ragged["Ng"], compact=False)
        zones, summary, _ = engine.glszm_batch_zones(dl, dm, None, ragged["Ng"])
    side.synchronize()
    assert engine.last_batch_route() == "batch" and status == ragged["status"]
    assert np.array_equal(summary, ragged["summary"])
    for b in range(len(RAGGED)):
        assert torch.equal(comp[b][0], ragged["comp"][b][0]) and np.array_equal(comp[b][1], ragged["comp"][b][1])
        assert torch.equal(dense[b], ragged["dense"][b]) and torch.equal(zones[b], ragged["zones"][b])

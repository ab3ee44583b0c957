"""Batched small-ROI texture matrices (engine.texture_matrices_batch, cmatrices.calculate_matrices_batch,
prad_calculate_batch_dev): every ROI of every batch against the reference C, called per ROI through the oracle binding, with
the single device calls as a second witness.  Shapes are the smallest at which the batched kernel can still go wrong: a
ragged batch with unaligned offsets, axes of length 1 and 2 and one box of exactly PRAD_BATCH_MAX_VOX voxels; more ROIs than
compute units; empty / full / one-voxel masks; 1 and 64 levels; two distances; a bad level; the declined domain.

Tolerances: GLCM, GLRLM, GLDM and the NGTDM count and level columns are exact; the NGTDM float column carries the bound
tests/test_gpu_parity.py:58 applies to the single NGTDM call against the reference (rtol 1e-12, atol 0)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAMILIES = ("glcm", "glrlm", "gldm", "ngtdm")
NGTDM_RTOL = 1e-12          # tests/test_gpu_parity.py:58
MAX_VOX = 160 * 1024 // 2 - 16384 - 256       # PRAD_BATCH_MAX_VOX (csrc/kernels_batch.h)
RAGGED = [(1, 1, 1), (1, 1, 9), (1, 8, 1), (2, 2, 2), (3, 17, 5), (16, 16, 16), (32, 40, 51)]
assert 32 * 40 * 51 == MAX_VOX


def _rois(shapes, Ng, seed, fill=0.6):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(1, Ng + 1, size=s).astype(np.int32) for s in shapes]
    masks = [rng.random(s) < fill for s in shapes]
    return imgs, masks


def _no_angle_truth(checker, img, mask, Ng, alpha):
    """a box no offset fits (1 x 1 x 1): the wrapper refuses it (no angle), the reference's core takes an empty angle table"""
    img = np.ascontiguousarray(img, dtype=np.intc)
    msk = np.ascontiguousarray(mask, dtype=np.bool_)
    size = np.array(img.shape, dtype=np.intc)
    strides = np.array([s // 4 for s in img.strides], dtype=np.intc)
    bb = np.concatenate([np.zeros(3, np.intc), size - 1]).astype(np.intc)
    ang = np.zeros((1, 3), dtype=np.intc)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    gldm, ngtdm = np.zeros((Ng, 1)), np.zeros((Ng, 3))
    std = (img.ctypes.data_as(ip), msk.ctypes.data_as(C.c_char_p), size.ctypes.data_as(ip), bb.ctypes.data_as(ip),
           strides.ctypes.data_as(ip), ang.ctypes.data_as(ip), 0, 3)
    if not checker.L.calculate_gldm(*std, gldm.ctypes.data_as(dp), Ng, alpha):
        raise IndexError("GLDM")
    if not checker.L.calculate_ngtdm(*std, ngtdm.ctypes.data_as(dp), Ng):
        raise IndexError("NGTDM")
    return {"glcm": np.zeros((Ng, Ng, 0)), "glrlm": np.zeros((Ng, max(img.shape), 0)), "gldm": gldm, "ngtdm": ngtdm}


def _truth(checker, img, mask, Ng, dist=(1,), alpha=0):
    """the reference's matrices of one ROI, or None where it raises IndexError (a masked level outside [1, Ng])"""
    dist = list(dist)
    try:
        try:
            glcm = checker.calculate_glcm(img, mask, dist, Ng, False, 0)[0][0]
        except RuntimeError:          # "Error getting angle count."
            return _no_angle_truth(checker, img, mask, Ng, alpha)
        return {"glcm": glcm,
                "glrlm": checker.calculate_glrlm(img, mask, Ng, max(img.shape), False, 0)[0][0],
                "gldm": checker.calculate_gldm(img, mask, dist, Ng, alpha, False, 0)[0],
                "ngtdm": checker.calculate_ngtdm(img, mask, dist, Ng, False, 0)[0]}
    except IndexError:
        return None


def _dev(imgs, masks):
    import torch
    return [torch.from_numpy(i).to("cuda:0") for i in imgs], [torch.from_numpy(m).to("cuda:0") for m in masks]


def _assert_roi(got, want, what):
    for f in ("glcm", "glrlm", "gldm"):
        assert got[f].shape == want[f].shape, "%s %s shape %s != %s" % (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), "%s %s" % (what, f)
    a, b = got["ngtdm"], want["ngtdm"]
    assert a.shape == b.shape
    assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 2], b[:, 2]), "%s NGTDM counts / levels" % what
    np.testing.assert_allclose(a[:, 1], b[:, 1], rtol=NGTDM_RTOL, atol=0, err_msg="%s NGTDM sums" % what)


def _assert_batched_route():
    from pyradiomics_amd import _lib, engine
    assert engine.last_batch_route() == "batch" and _lib.last_path() == "batch" and _lib.last_variant() == "batch-lds"


def _check(checker, imgs, masks, Ng, mats, status, dist=(1,), alpha=0, truths=None):
    """every ROI of a batch result (device tensors or numpy) against the reference; returns the statuses expected"""
    assert len(status) == len(imgs) and all(len(mats[f]) == len(imgs) for f in FAMILIES)
    for b, (img, msk) in enumerate(zip(imgs, masks)):
        want = truths[b] if truths is not None else _truth(checker, img, msk, Ng, dist, alpha)
        if want is None:
            assert status[b] == 0, "ROI %d: the reference raises IndexError" % b
            continue
        assert status[b] == 1, "ROI %d status %d" % (b, status[b])
        got = {f: (mats[f][b].cpu().numpy() if hasattr(mats[f][b], "cpu") else mats[f][b]) for f in FAMILIES}
        _assert_roi(got, want, "ROI %d %s" % (b, img.shape))


@pytest.fixture(scope="module")
def ragged(checker):
    """the ragged batch, its reference matrices (distance 1) and the batched result of the default stream: computed once"""
    from pyradiomics_amd import engine
    Ng = 16
    imgs, masks = _rois(RAGGED, Ng, seed=20260)
    masks[0][:] = True
    truths = [_truth(checker, i, m, Ng) for i, m in zip(imgs, masks)]
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng)
    route = (engine.last_batch_route(), engine.last_path())
    return {"Ng": Ng, "imgs": imgs, "masks": masks, "truths": truths, "dev": (dl, dm), "mats": mats, "status": status,
            "route": route}


def test_single_roi(checker):
    from pyradiomics_amd import engine
    imgs, masks = _rois([(5, 6, 7)], 8, seed=1)
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, 8)
    _assert_batched_route()
    _check(checker, imgs, masks, 8, mats, status)
    # second witness: the single device calls, bit for bit where the matrices are integers
    assert np.array_equal(mats["glcm"][0].cpu().numpy(), engine.glcm(dl[0], dm[0], 8)[0].cpu().numpy())
    assert np.array_equal(mats["glrlm"][0].cpu().numpy(), engine.glcm_glrlm(dl[0], dm[0], 8, 7, want_glcm=False)[1].cpu().numpy())
    assert np.array_equal(mats["gldm"][0].cpu().numpy(), engine.gldm(dl[0], dm[0], 8).cpu().numpy())
    np.testing.assert_allclose(mats["ngtdm"][0].cpu().numpy(), engine.ngtdm(dl[0], dm[0], 8).cpu().numpy(), rtol=NGTDM_RTOL, atol=0)
    # a subset of the families, flat inputs + sizes
    import torch
    sub, st = engine.texture_matrices_batch(dl[0].reshape(-1), dm[0].reshape(-1), [(5, 6, 7)], 8, families=("ngtdm", "glrlm"))
    _assert_batched_route()
    assert set(sub) == {"ngtdm", "glrlm"} and st == [1]
    assert torch.equal(sub["glrlm"][0], mats["glrlm"][0]) and torch.equal(sub["ngtdm"][0], mats["ngtdm"][0])


def test_ragged_batch(checker, ragged):
    from pyradiomics_amd import engine
    assert ragged["route"] == ("batch", "batch")
    Ng, mats = ragged["Ng"], ragged["mats"]
    _check(checker, ragged["imgs"], ragged["masks"], Ng, mats, ragged["status"], truths=ragged["truths"])
    # odd voxel counts: the ROIs after the first start at elements that are no multiple of 4 (nor their bytes of 16)
    starts = np.cumsum([0] + [int(np.prod(s)) for s in RAGGED])[:-1]
    assert any(s % 4 for s in starts[1:]) and any(s % 16 for s in starts[1:])
    # Na[b], Nr[b] and the GLDM width are what the single calls use
    dl, dm = ragged["dev"]
    for b, shape in enumerate(RAGGED):
        if shape == (1, 1, 1):
            assert mats["glcm"][b].shape == (Ng, Ng, 0) and mats["glrlm"][b].shape == (Ng, 1, 0) and mats["gldm"][b].shape == (Ng, 1)
            continue
        na, nb = len(engine.pair_angles(shape)), len(engine.neigh_angles(shape))
        assert mats["glcm"][b].shape == (Ng, Ng, na) and mats["glrlm"][b].shape == (Ng, max(shape), na)
        assert mats["gldm"][b].shape == (Ng, 2 * nb + 1) and nb == 2 * na
    assert [m.shape[2] for m in mats["glcm"]] == [0, 1, 1, 13, 13, 13, 13]
    # second witness on the two largest boxes
    for b in (4, 6):
        assert np.array_equal(mats["glcm"][b].cpu().numpy(), engine.glcm(dl[b], dm[b], Ng)[0].cpu().numpy())
        assert np.array_equal(mats["gldm"][b].cpu().numpy(), engine.gldm(dl[b], dm[b], Ng).cpu().numpy())


def test_more_rois_than_compute_units(checker):
    from pyradiomics_amd import engine
    B, Ng = 300, 8
    imgs, masks = _rois([(4, 4, 4)] * B, Ng, seed=3, fill=0.5)
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng)
    _assert_batched_route()
    assert status == [1] * B
    _check(checker, imgs, masks, Ng, mats, status)          # all 300: none skipped, none written twice


def test_one_workgroup_per_family(checker):
    """1024 ROIs: the angles of a ROI are no longer split over workgroups, so one workgroup walks all 13 in sub-batches
    (4 GLCM tables of 32 x 32 fit the table region at once, 8 GLRLM tables)"""
    from pyradiomics_amd import engine
    B, Ng = 1024, 32
    imgs, masks = _rois([(2, 2, 2)] * (B - 1) + [(3, 2, 4)], Ng, seed=31, fill=0.8)
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng)
    _assert_batched_route()
    _check(checker, imgs, masks, Ng, mats, status)


def test_tables_built_in_passes(checker):
    """tables above the 16 KiB region: 64 levels x 125 neighbour counts (GLDM / NGTDM in 4 level passes), 64 levels x 130 run
    lengths (GLRLM in 3 column passes, the last two skipped for the angles whose lines are short)"""
    from pyradiomics_amd import engine
    Ng = 64
    imgs, masks = _rois([(5, 6, 7), (2, 3, 130), (1, 2, 70), (3, 3, 3)], Ng, seed=32, fill=0.9)
    imgs[1][1, 1, :] = 17
    masks[1][1, 1, :] = True          # a run of 130
    imgs[2][:] = 64
    masks[2][:] = True                # two runs of 70
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng, distances=(1, 2))
    _assert_batched_route()
    _check(checker, imgs, masks, Ng, mats, status, dist=(1, 2))
    a = engine.pair_angles((2, 3, 130)).tolist().index([0, 0, 1])
    assert mats["glrlm"][1][16, 129, a].item() == 1 and mats["glrlm"][2][63, 69, :].sum().item() == 2


def test_masks_empty_full_single_voxel(checker):
    from pyradiomics_amd import engine
    Ng = 6
    imgs, masks = _rois([(4, 5, 6)] * 3 + [(3, 3, 3)], Ng, seed=4)
    masks[0][:] = False
    masks[1][:] = True
    masks[2][:] = False
    masks[2][2, 3, 1] = True
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng)
    _assert_batched_route()
    _check(checker, imgs, masks, Ng, mats, status)
    assert not mats["glcm"][0].any() and not mats["glrlm"][0].any() and not mats["gldm"][0].any()
    assert mats["ngtdm"][0][:, :2].sum().item() == 0 and mats["ngtdm"][0][:, 2].tolist() == list(range(1, Ng + 1))
    assert mats["gldm"][2].sum().item() == 1 and not mats["glrlm"][2].any()     # one voxel: its run column is cleared


@pytest.mark.parametrize("Ng", [1, 64])
def test_level_extremes(checker, Ng):
    from pyradiomics_amd import engine
    shapes = [(5, 6, 7), (6, 9, 4), (5, 6, 7)]
    imgs, masks = _rois(shapes, Ng, seed=50 + Ng)
    imgs[0].flat[0], imgs[0].flat[-1] = 1, Ng
    masks[0].flat[0] = masks[0].flat[-1] = True
    const = min(Ng, 3)
    imgs[2][:] = const          # one constant level under a full mask: one run of full length on every axis,
    masks[2][:] = True          # dependence 2 * Na = 26 in the interior
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng)
    _assert_batched_route()
    _check(checker, imgs, masks, Ng, mats, status)
    if Ng == 64:
        assert mats["ngtdm"][0][0, 0].item() >= 1 and mats["ngtdm"][0][63, 0].item() >= 1
    gldm, glrlm = mats["gldm"][2].cpu().numpy(), mats["glrlm"][2].cpu().numpy()
    assert gldm[const - 1, 26] == 3 * 4 * 5 and gldm[:, 27:].sum() == 0
    ang = engine.pair_angles((5, 6, 7)).tolist()
    for axis, length in ((0, 5), (1, 6), (2, 7)):
        a = ang.index([int(d == axis) for d in range(3)])
        assert glrlm[const - 1, length - 1, a] == 5 * 6 * 7 // length and glrlm[:, :, a].sum() == 5 * 6 * 7 // length


def test_two_distances_and_alpha(checker, ragged):
    from pyradiomics_amd import engine
    Ng, dist = ragged["Ng"], (1, 2)
    dl, dm = ragged["dev"]
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng, distances=dist, gldm_a=2)
    _assert_batched_route()
    _check(checker, ragged["imgs"], ragged["masks"], Ng, mats, status, dist=dist, alpha=2)
    # boxes with an edge <= 2 lose the distance-2 angles: 1x1x9 keeps (0,0,1) and (0,0,2), 2x2x2 only its 13 of distance 1
    assert [m.shape[2] for m in mats["glcm"]] == [0, 2, 2, 13, len(engine.pair_angles((3, 17, 5), dist)), 62, 62]
    # GLRLM stays at distance 1 (_cmatrices.c:432-581)
    import torch
    assert all(torch.equal(a, b) for a, b in zip(mats["glrlm"], ragged["mats"]["glrlm"]))


def test_bad_level_voids_one_roi_only(checker):
    from pyradiomics_amd import engine
    Ng = 8
    imgs, masks = _rois([(4, 4, 4), (5, 3, 7), (2, 9, 3), (6, 6, 6)], Ng, seed=7)
    imgs[1][2, 1, 4] = 0
    masks[1][2, 1, 4] = True
    imgs[2][0, 0, 0] = 0          # a level 0 OUTSIDE the mask is no error
    masks[2][0, 0, 0] = False
    imgs[3][1, 1, 1] = Ng + 1
    masks[3][1, 1, 1] = True
    dl, dm = _dev(imgs, masks)
    mats, status = engine.texture_matrices_batch(dl, dm, None, Ng)
    _assert_batched_route()
    assert status == [1, 0, 1, 0]
    _check(checker, imgs, masks, Ng, mats, status)


def test_out_of_domain_is_declined_and_looped(checker):
    import torch
    from pyradiomics_amd import _lib, engine
    lib = _lib.load()
    over = (1, 97, 673)
    assert int(np.prod(over)) == MAX_VOX + 1 == engine.batch_max_vox() + 1
    for shapes, Ng in (([(3, 4, 5), (1, 1, 1), (4, 2, 6)], 65), ([(3, 4, 5), over], 4)):
        imgs, masks = _rois(shapes, Ng, seed=8)
        imgs[0].flat[0], masks[0].flat[0] = Ng, True
        dl, dm = _dev(imgs, masks)
        mats, status = engine.texture_matrices_batch(dl, dm, None, Ng)
        assert engine.last_batch_route() == "looped" and _lib.last_path() != "batch"
        _check(checker, imgs, masks, Ng, mats, status)
        # the native call declines the whole batch before it launches anything: status and outputs stay untouched
        sizes = np.array(shapes, dtype=np.intc)
        off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])[:-1]]).astype(np.int64)
        flat_l, flat_m = torch.cat([t.reshape(-1) for t in dl]), torch.cat([t.reshape(-1) for t in dm]).view(torch.uint8)
        st = torch.full((len(shapes),), -7, dtype=torch.int32, device="cuda:0")
        out = torch.full((4, 1 << 16), -7.0, dtype=torch.float64, device="cuda:0")
        before = _lib.last_path()
        dist = np.array([1], dtype=np.intc)
        ip = C.POINTER(C.c_int)
        rc = lib.prad_calculate_batch_dev(C.c_void_p(flat_l.data_ptr()), C.c_void_p(flat_m.data_ptr()), sizes.ctypes.data_as(ip),
                                          off.ctypes.data_as(C.POINTER(C.c_longlong)), len(shapes), Ng, 15, dist.ctypes.data_as(ip),
                                          1, 0, *[C.c_void_p(out[f].data_ptr()) for f in range(4)], C.c_void_p(st.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == _lib.PRAD_E_UNSUPPORTED and _lib.last_path() == before
        assert (st == -7).all().item() and (out == -7.0).all().item()
        assert engine.texture_matrices_batch_flat(flat_l, flat_m, sizes, Ng) is None


def test_host_route_equals_device_route(checker, ragged):
    from pyradiomics_amd import cmatrices as cm
    mats, status = cm.calculate_matrices_batch(ragged["imgs"], ragged["masks"], ragged["Ng"])
    assert cm.last_batch_route() == "batch"
    _assert_batched_route()
    assert status == ragged["status"]
    for f in FAMILIES:
        for a, b in zip(mats[f], ragged["mats"][f]):
            assert isinstance(a, np.ndarray) and np.array_equal(a, b.cpu().numpy())
    _check(checker, ragged["imgs"], ragged["masks"], ragged["Ng"], mats, status, truths=ragged["truths"])


def test_side_stream(ragged):
    import torch
    from pyradiomics_amd import engine
    dl, dm = ragged["dev"]
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mats, status = engine.texture_matrices_batch(dl, dm, None, ragged["Ng"])
    side.synchronize()
    assert engine.last_batch_route() == "batch" and status == ragged["status"]
    for f in FAMILIES:
        assert all(torch.equal(a, b) for a, b in zip(mats[f], ragged["mats"][f]))

"""GPU: engine.roi_features_batch_images (Original + the eight wavelet sub-bands of a batch of boxes) against
RadiomicsFeatureExtractor.execute, lesion by lesion.

Three lesions inside the 40 x 44 x 48 float32 volume of tests/test_gpu_labels_batched.py (_inputs: the image recipe; the label
map here is this file's own).  Each lesion's box is the one imageoperations.cropToTumorMask cuts with the case's padDistance
(5, the default): the box execute() filters under `preCrop`, and -- because every lesion keeps more than padDistance voxels
between itself and the volume's faces, so that the crop is not clipped and no ROI voxel's filter support (coif1: 2 below, 3
above) reaches the crop's border -- the box on whose ROI voxels the sub-bands of the whole volume, which execute() filters
otherwise, have the same bits.  Both settings are compared.  roi_features_batch_images cuts every image to the mask's bounding
box before its feature calls, as the reference's classes do: handed the padded boxes, roi_features_batch itself gives GLRLM
features (RunEntropy, the *RunLowGrayLevelEmphasis, ShortRunHighGrayLevelEmphasis) that differ from execute() in their last one
or two bits -- 3.9526090235197335 against 3.9526090235197326 for original_glrlm_RunEntropy of lesion 1 --, because the GLRLM
is max(size) wide; every other feature agreed even then.

Per lesion and image: every texture feature and the first-order features of EXACT_FO bit for bit; the SUMMED first-order
features against firstorder_reference.segment_reference of the same crop under _feature_bounds, with K as
tests/test_gpu_labels_batched.py takes it (the batched launch's chain length; every ROI here is served by it: route "batch")."""
import math

import numpy as np
import pytest

import firstorder_reference as fr
from test_gpu_batch_firstorder import _feature_bounds, _k
from test_gpu_labels_batched import EXACT_FO, SUMMED, _inputs

pytestmark = pytest.mark.gpu

PAD = 5
TYPES = {"Original": {}, "Wavelet": {}}
LABELS = (1, 2, 3)


def _case():
    img, _ = _inputs()
    z, y, x = np.mgrid[0:40, 0:44, 0:48].astype(np.float64)
    lab = np.zeros(img.shape, dtype=np.int16)
    lab[((z - 12) ** 2 + (y - 14) ** 2 + (x - 15) ** 2) <= 4.5 ** 2] = 1                       # a ball: box 9^3, crop 19^3 (odd)
    lab[(((z - 27) * 1.4) ** 2 + (y - 30) ** 2 + ((x - 34) * 0.8) ** 2) <= 5.0 ** 2] = 2       # an ellipsoid
    lab[9:15, 28:36, 30:40] = 3                                                                # a block with holes
    lab[10:14, 30:34, 32:38][np.random.default_rng(5).random((4, 4, 6)) < 0.3] = 0
    return img, lab


_cache = {}


def _batched():
    if "batched" not in _cache:
        import torch
        from pyradiomics_amd import engine, imageoperations
        img, lab = _case()
        boxes, masks, crops = [], [], []
        for l in LABELS:
            cimg, cmask = imageoperations.cropToTumorMask(img, lab, l, padDistance=PAD, alignRows=False)
            assert all(s >= 2 * PAD + 2 for s in cimg.array.shape), "the crop was clipped by the volume"
            a, m = np.ascontiguousarray(cimg.array), np.ascontiguousarray(cmask.array == l)
            lo = [int(np.flatnonzero(m.any(axis=tuple(d for d in range(3) if d != ax)))[0]) for ax in range(3)]
            hi = [int(np.flatnonzero(m.any(axis=tuple(d for d in range(3) if d != ax)))[-1]) for ax in range(3)]
            assert all(v == PAD for v in lo) and all(h == s - 1 - PAD for h, s in zip(hi, m.shape))
            crops.append((a, m))
            boxes.append(torch.from_numpy(a).cuda())
            masks.append(torch.from_numpy(m).cuda())
        tables, status = engine.roi_features_batch_images(boxes, masks, imageTypes=TYPES, binCount=16, extras=True)
        route = engine.last_batch_route()
        bands, names, _ = engine.wavelet_batch(boxes)
        assert engine.last_batch_route() == "batch"
        _cache["batched"] = (tables, status, route, crops, bands.cpu().numpy(), names)
    return _cache["batched"]


def _bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def test_image_names_and_status():
    tables, status, route, crops, bands, names = _batched()
    assert list(tables) == ["original"] + list(names)
    assert status == [1, 1, 1] and route == "batch"
    for name, table in tables.items():
        for cls in ("firstorder", "glcm", "glrlm", "glszm", "gldm", "ngtdm"):
            assert table[cls].shape[0] == 3 and not np.isnan(table[cls]).any(), (name, cls)       # MCC included: <= 64 levels
        assert (table["gray_levels"] >= 2).all() and (table["gray_levels"] <= 16).all()


@pytest.mark.parametrize("preCrop", [False, True])
@pytest.mark.parametrize("label", LABELS)
def test_features_equal_the_extractor(label, preCrop):
    from pyradiomics_amd import cmatrices, engine
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    import torch
    tables, status, route, crops, bands, names = _batched()
    img, lab = _case()
    setting = {"binCount": 16}
    if preCrop:
        setting["preCrop"] = True
    want = RadiomicsFeatureExtractor({"imageType": TYPES, "setting": setting}).execute(img, lab, label=label)
    b = LABELS.index(label)
    held = {cls: (cmatrices.FIRSTORDER_FEATURES if cls == "firstorder" else cmatrices.batch_feature_names(cls))
            for cls in engine.ROI_FEATURE_CLASSES}
    seen, differ = set(), []
    off = np.concatenate([[0], np.cumsum([a.size for a, _ in crops])])
    for key, w in want.items():
        if key.startswith("diagnostics_"):
            continue
        image, cls, feat = key.rsplit("_", 2)
        table = tables[image]
        value = table[cls][b][held[cls].index(feat)]
        if cls == "glcm" and feat == "MCC":          # as RadiomicsGLCM reports it: the flat mean over the angles
            value = cmatrices._mcc_angle_mean(table["glcm_mcc_angles"][b])
        seen.add(image)
        if cls != "firstorder" or feat in EXACT_FO:
            assert not np.isnan(value)
            if _bits(value) != _bits(w):
                differ.append((key, float(value), float(w)))
        else:
            assert feat in SUMMED, key
    assert seen == set(tables)
    for key, value, w in differ:
        print("label %d %-50s batched %.17g extractor %.17g" % (label, key, value, w))
    assert not differ, (label, len(differ), differ[:8])
    # the summed first-order features: against the long-double reference of the same crop
    worst = 0.0
    for image, table in tables.items():
        a, m = crops[b]
        crop = a if image == "original" else np.ascontiguousarray(bands[names.row(image), off[b]:off[b + 1]].reshape(a.shape))
        ref = fr.segment_reference(crop, m, 0.0)
        cap = engine.batch_firstorder_max_roi(torch.float64 if crop.dtype == np.float64 else torch.float32)
        single = ref["m"] > cap                        # (route "batch": no ROI went to the single call for another reason)
        K = fr.k_reduction(crop.size, crop.dtype.itemsize) if single else _k(ref["m"])
        bounds = _feature_bounds(ref, K, 1.0)
        for feat in SUMMED:
            wv, bd = bounds[feat]
            got = float(table["firstorder"][b][held["firstorder"].index(feat)])
            err = abs(got - wv)
            print("label %d %-12s %-28s err %.3g bound %.3g K %d" % (label, image, feat, err, bd, K))
            worst = max(worst, err / bd if bd > 0 else (0.0 if err == 0 else math.inf))
            assert err <= bd, (label, image, feat, got, wv, err, bd, K)
    print("label %d: worst error / bound of the summed first-order features %.3g" % (label, worst))

"""GPU: engine.roi_features_batch_resampled (resample_batch, then Original + Wavelet + LoG of the resampled boxes) against
RadiomicsFeatureExtractor.execute on each box as the image, with the same settings and no preCrop.

The three lesions, the volume and the boxes of tests/test_gpu_batch_wavelet_features.py (_case; cropToTumorMask with padDistance
5), each box handed over with an anisotropic spacing of its own.  Under resampledPixelSpacing (0.9, 1.1, 1.5) every lesion has
an axis that is up-sampled and one that is down-sampled, each along different axes, so an axis mix-up in the planner, the
kernels or the spacing handed on to the LoG shows; the voxel volume, 1.485, is not 1.  execute() resamples the box it is given
(resampleImage on the whole image: the box), so it filters exactly the arrays the batched call filters.

Per lesion and image: every texture feature and the first-order features of EXACT_FO bit for bit; the SUMMED first-order features
against firstorder_reference.segment_reference of the same resampled box under _feature_bounds, exactly as
tests/test_gpu_batch_log_features.py holds them."""
import math

import numpy as np
import pytest

import firstorder_reference as fr
from test_gpu_batch_firstorder import _feature_bounds, _k
from test_gpu_batch_wavelet_features import LABELS, PAD, _bits, _case
from test_gpu_labels_batched import EXACT_FO, SUMMED

pytestmark = pytest.mark.gpu

SIGMA = [1.0, 2.0]
TYPES = {"Original": {}, "Wavelet": {}, "LoG": {"sigma": SIGMA}}
SPACING = {1: (2.0, 0.5, 1.3), 2: (0.6, 1.6, 0.7), 3: (1.2, 2.4, 0.45)}          # (z, y, x) per lesion
NEW = (0.9, 1.1, 1.5)                                                            # (x, y, z), as in a parameter file
VOLUME = 0.9 * 1.1 * 1.5
SETTINGS = {"binCount": 16, "resampledPixelSpacing": list(NEW), "interpolator": "sitkBSpline", "padDistance": PAD}

_cache = {}


def _boxes():
    if "boxes" not in _cache:
        import torch
        from pyradiomics_amd import imageoperations
        img, lab = _case()
        boxes, masks, crops = [], [], []
        for l in LABELS:
            cimg, cmask = imageoperations.cropToTumorMask(img, lab, l, padDistance=PAD, alignRows=False)
            a, m = np.ascontiguousarray(cimg.array), np.ascontiguousarray(cmask.array == l)
            crops.append((a, m))
            boxes.append(torch.from_numpy(a).cuda())
            masks.append(torch.from_numpy(m).cuda())
        _cache["boxes"] = (boxes, masks, crops)
    return _cache["boxes"]


def _batched():
    if "batched" not in _cache:
        from pyradiomics_amd import engine
        boxes, masks, crops = _boxes()
        spacing = np.array([SPACING[l] for l in LABELS])
        tables, status = engine.roi_features_batch_resampled(boxes, masks, spacing=spacing, resampledPixelSpacing=NEW,
                                                             interpolator="sitkBSpline", padDistance=PAD, imageTypes=TYPES,
                                                             binCount=16, extras=True)
        route = engine.last_batch_route()
        # the images the features were computed on, for the long-double reference of the summed first-order features
        out, out_m, sizes, new_spacing, _, rstatus = engine.resample_batch(boxes, masks, spacing=spacing, resampledPixelSpacing=NEW,
                                                                          padDistance=PAD)
        assert rstatus.tolist() == [0, 0, 0] and engine.last_batch_route() == "batch"
        assert np.array_equal(new_spacing, np.tile(np.array(NEW)[::-1], (3, 1)))
        bands, bnames, _ = engine.wavelet_batch(out, sizes)
        logs, lnames, _, valid = engine.log_batch(out, sizes, sigma=SIGMA, spacing=new_spacing)
        assert valid.all()
        images = {"original": out.cpu().numpy()}
        host = bands.cpu().numpy()
        images.update({n: host[r] for n, r in zip(bnames, bnames.rows)})
        host = logs.cpu().numpy()
        images.update({n: host[s] for s, n in enumerate(lnames)})
        _cache["batched"] = (tables, status, route, images, out_m.cpu().numpy() != 0, sizes)
    return _cache["batched"]


def test_image_names_status_and_grids():
    tables, status, route, images, mask, sizes = _batched()
    assert list(tables) == list(images) and len(tables) == 1 + 8 + 2
    assert status == [1, 1, 1] and route == "batch"
    boxes, _, crops = _boxes()
    for b, l in enumerate(LABELS):
        step = np.array(NEW)[::-1] / np.array(SPACING[l])
        assert (step < 1).any() and (step > 1).any(), "an axis up-sampled and one down-sampled per lesion"
        assert tuple(sizes[b]) != crops[b][0].shape
    for name, table in tables.items():
        for cls in ("firstorder", "glcm", "glrlm", "glszm", "gldm", "ngtdm"):
            assert table[cls].shape[0] == 3 and not np.isnan(table[cls]).any(), (name, cls)


@pytest.mark.parametrize("label", LABELS)
def test_features_equal_the_extractor(label):
    from pyradiomics_amd import cmatrices, engine
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image
    import torch
    tables, status, route, images, mask, sizes = _batched()
    b = LABELS.index(label)
    a, m = _boxes()[2][b]
    sp = SPACING[label][::-1]
    want = RadiomicsFeatureExtractor({"imageType": TYPES, "setting": dict(SETTINGS)}).execute(
        Image(a, sp), Image(m.astype(np.uint8), sp), label=1)
    held = {cls: (cmatrices.FIRSTORDER_FEATURES if cls == "firstorder" else cmatrices.batch_feature_names(cls))
            for cls in engine.ROI_FEATURE_CLASSES}
    seen, differ = set(), []
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
    # the summed first-order features: against the long-double reference of the same resampled box
    off = np.concatenate([[0], np.cumsum(sizes.astype(np.int64).prod(1))])
    shape = tuple(int(s) for s in sizes[b])
    roi = np.ascontiguousarray(mask[off[b]:off[b + 1]].reshape(shape))
    worst = 0.0
    for image, table in tables.items():
        crop = np.ascontiguousarray(images[image][off[b]:off[b + 1]].reshape(shape))
        ref = fr.segment_reference(crop, roi, 0.0)
        cap = engine.batch_firstorder_max_roi(torch.float64 if crop.dtype == np.float64 else torch.float32)
        single = ref["m"] > cap                        # (route "batch": no ROI went to the single call for another reason)
        K = fr.k_reduction(crop.size, crop.dtype.itemsize) if single else _k(ref["m"])
        bounds = _feature_bounds(ref, K, VOLUME)
        for feat in SUMMED:
            wv, bd = bounds[feat]
            got = float(table["firstorder"][b][held["firstorder"].index(feat)])
            err = abs(got - wv)
            print("label %d %-20s %-28s err %.3g bound %.3g K %d" % (label, image, feat, err, bd, K))
            worst = max(worst, err / bd if bd > 0 else (0.0 if err == 0 else math.inf))
            assert err <= bd, (label, image, feat, got, wv, err, bd, K)
    print("label %d: worst error / bound of the summed first-order features %.3g" % (label, worst))


def test_an_empty_roi_has_status_0_and_nan_rows():
    import torch
    from pyradiomics_amd import engine
    boxes, masks, _ = _boxes()
    masks = [masks[0], torch.zeros_like(masks[1]), masks[2]]
    spacing = np.array([SPACING[l] for l in LABELS])
    tables, status = engine.roi_features_batch_resampled(boxes, masks, spacing=spacing, resampledPixelSpacing=NEW, padDistance=PAD,
                                                         imageTypes={"Original": {}}, binCount=16, extras=True)
    first = _batched()[0]
    assert status == [1, 0, 1]
    for cls in engine.ROI_FEATURE_CLASSES:
        assert np.isnan(tables["original"][cls][1]).all(), cls
        assert _bits(tables["original"][cls][[0, 2]]) == _bits(first["original"][cls][[0, 2]]), cls


def test_other_image_types_and_interpolators_are_named():
    from pyradiomics_amd import engine
    boxes, masks, _ = _boxes()
    with pytest.raises(NotImplementedError, match="Square"):
        engine.roi_features_batch_resampled(boxes, masks, resampledPixelSpacing=NEW, imageTypes={"Square": {}}, binCount=16)
    with pytest.raises(NotImplementedError, match="interpolator"):
        engine.roi_features_batch_resampled(boxes, masks, resampledPixelSpacing=NEW, interpolator="sitkGaussian", binCount=16)

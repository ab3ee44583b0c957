"""GPU: engine.roi_features_batch_types (the five image types Square, SquareRoot, Logarithm, Exponential and Gradient) against
RadiomicsFeatureExtractor.execute, lesion by lesion.

The three lesions, the volume and the boxes of tests/test_gpu_batch_log_features.py (_boxes: cropToTumorMask with
padDistance 5).  The extractor runs with preCrop=True ONLY, as for the LoG: the maximum |x| the four transforms scale with is
that of the image they are handed, and the gradient replicates the edge of the image it is handed, so without preCrop execute()
transforms the whole volume and its values differ from the transform of the crop.  With preCrop execute() transforms exactly the
box the batched call is handed.

Square, SquareRoot, Gradient -- whose images equal the single route's bit for bit (tests/test_gpu_batch_intensity.py) --: per
lesion and image every texture feature and the first-order features of EXACT_FO bit for bit; the SUMMED first-order features
against firstorder_reference.segment_reference of the same crop under _feature_bounds, exactly as the wavelet and LoG tests hold
them.
Logarithm, Exponential: log and exp of torch and of this library need not agree in the last bit, and a one-ulp difference of the
image may move a voxel across a bin edge, which changes every feature of the ROI by far more than any rounding bound.  So NO
comparison with execute() is asserted for these two; their tables must equal, bit for bit, roi_features_batch applied to the
rows of intensity_batch (cut to the tight boxes the way the table call cuts them)."""
import math

import numpy as np
import pytest

import firstorder_reference as fr
from test_gpu_batch_firstorder import _feature_bounds, _k
from test_gpu_batch_log_features import _boxes
from test_gpu_batch_wavelet_features import LABELS, _bits, _case
from test_gpu_labels_batched import EXACT_FO, SUMMED

pytestmark = pytest.mark.gpu

EXACT = {"Square": {}, "SquareRoot": {}, "Gradient": {}}
LOOSE = {"Logarithm": {}, "Exponential": {}}
TYPES = {"Square": {}, "SquareRoot": {}, "Logarithm": {}, "Exponential": {}, "Gradient": {}}
NAMES = ["square", "squareroot", "logarithm", "exponential", "gradient"]
SPACING = (1.0, 1.0, 1.0)          # the image's, (z, y, x): a numpy volume has unit spacing

_cache = {}


def _batched():
    if "batched" not in _cache:
        from pyradiomics_amd import engine
        boxes, masks, crops = _boxes()
        tables, status = engine.roi_features_batch_types(boxes, masks, imageTypes=TYPES, binCount=16, spacing=SPACING, extras=True)
        route = engine.last_batch_route()
        rows, names, _ = engine.intensity_batch(boxes)
        grad, _, _ = engine.gradient_batch(boxes, spacing=SPACING)
        images = {n: rows[i] for i, n in enumerate(names)}
        images["gradient"] = grad
        _cache["batched"] = (tables, status, route, crops, images)
    return _cache["batched"]


def test_image_names_and_status():
    tables, status, route, crops, images = _batched()
    assert list(tables) == NAMES
    assert status == [1, 1, 1] and route == "batch"
    for name, table in tables.items():
        for cls in ("firstorder", "glcm", "glrlm", "glszm", "gldm", "ngtdm"):
            assert table[cls].shape[0] == 3 and not np.isnan(table[cls]).any(), (name, cls)
        assert (table["gray_levels"] >= 2).all() and (table["gray_levels"] <= 16).all()


@pytest.mark.parametrize("label", LABELS)
def test_features_equal_the_extractor(label):
    from pyradiomics_amd import cmatrices, engine
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    import torch
    tables, status, route, crops, images = _batched()
    img, lab = _case()
    want = RadiomicsFeatureExtractor({"imageType": EXACT, "setting": {"binCount": 16, "preCrop": True}}).execute(img, lab, label=label)
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
    assert seen == {"square", "squareroot", "gradient"}
    for key, value, w in differ:
        print("label %d %-50s batched %.17g extractor %.17g" % (label, key, value, w))
    assert not differ, (label, len(differ), differ[:8])
    # the summed first-order features: against the long-double reference of the same crop
    worst = 0.0
    for image in sorted(seen):
        a, m = crops[b]
        crop = np.ascontiguousarray(images[image][off[b]:off[b + 1]].cpu().numpy().reshape(a.shape))
        ref = fr.segment_reference(crop, m, 0.0)
        cap = engine.batch_firstorder_max_roi(torch.float64 if crop.dtype == np.float64 else torch.float32)
        single = ref["m"] > cap                        # (route "batch": no ROI went to the single call for another reason)
        K = fr.k_reduction(crop.size, crop.dtype.itemsize) if single else _k(ref["m"])
        bounds = _feature_bounds(ref, K, 1.0)
        for feat in SUMMED:
            wv, bd = bounds[feat]
            got = float(tables[image]["firstorder"][b][held["firstorder"].index(feat)])
            err = abs(got - wv)
            print("label %d %-20s %-28s err %.3g bound %.3g K %d" % (label, image, feat, err, bd, K))
            worst = max(worst, err / bd if bd > 0 else (0.0 if err == 0 else math.inf))
            assert err <= bd, (label, image, feat, got, wv, err, bd, K)
    print("label %d: worst error / bound of the summed first-order features %.3g" % (label, worst))


def test_logarithm_and_exponential_tables_are_those_of_their_rows():
    """no comparison with execute() for these two (module docstring): the table call must be roi_features_batch on the rows"""
    from pyradiomics_amd import engine, roi_batch
    tables, status, route, crops, images = _batched()
    boxes, masks, _ = _boxes()
    rois = roi_batch._roi_batch(boxes, masks, None, raw=True)
    pick, tight = roi_batch._tight_boxes(rois)
    for name in ("logarithm", "exponential"):
        table, st = engine.roi_features_batch(images[name][pick], rois.mask[pick], tight, binCount=16, spacing=SPACING, extras=True)
        assert st == [1, 1, 1]
        for cls in engine.ROI_FEATURE_CLASSES + ("gray_levels",):
            assert _bits(table[cls]) == _bits(tables[name][cls]), (name, cls)
    # and on their own they give what they give next to the other three types
    alone, st = engine.roi_features_batch_types(boxes, masks, imageTypes=LOOSE, binCount=16, spacing=SPACING, extras=True)
    assert list(alone) == ["logarithm", "exponential"] and st == [1, 1, 1] and engine.last_batch_route() == "batch"
    for name in alone:
        for cls in engine.ROI_FEATURE_CLASSES:
            assert _bits(alone[name][cls]) == _bits(tables[name][cls]), (name, cls)


def test_the_older_types_go_through_unchanged():
    from pyradiomics_amd import engine
    boxes, masks, _ = _boxes()
    types = {"Original": {}, "Wavelet": {}, "LoG": {"sigma": [1.0]}}
    new, st_new = engine.roi_features_batch_types(boxes, masks, imageTypes=types, binCount=16, spacing=SPACING)
    route = engine.last_batch_route()
    old, st_old = engine.roi_features_batch_derived(boxes, masks, imageTypes=types, binCount=16, spacing=SPACING)
    assert list(new) == list(old) and st_new == st_old and route == engine.last_batch_route()
    for name in old:
        for cls in engine.ROI_FEATURE_CLASSES:
            assert _bits(new[name][cls]) == _bits(old[name][cls]), (name, cls)


def test_order_and_gradient_settings():
    """the images go in the order of imageTypes' keys; gradientUseSpacing is read by the Gradient image and reaches no feature call"""
    from pyradiomics_amd import engine
    boxes, masks, _ = _boxes()
    sp = (0.7, 1.1, 2.0)
    mixed, _ = engine.roi_features_batch_types(boxes, masks, imageTypes={"Gradient": {}, "Original": {}, "Square": {}}, binCount=16,
                                               spacing=sp, gradientUseSpacing=False, classes=("firstorder",))
    assert list(mixed) == ["gradient", "original", "square"]
    unit, _ = engine.roi_features_batch_types(boxes, masks, imageTypes={"Gradient": {}}, binCount=16, classes=("firstorder",))
    scaled, _ = engine.roi_features_batch_types(boxes, masks, imageTypes={"Gradient": {"gradientUseSpacing": True}}, binCount=16,
                                                spacing=sp, gradientUseSpacing=False, classes=("firstorder",))
    assert _bits(mixed["gradient"]["firstorder"]) == _bits(unit["gradient"]["firstorder"])          # spacing not used
    assert _bits(scaled["gradient"]["firstorder"]) != _bits(unit["gradient"]["firstorder"])         # the type's own setting wins

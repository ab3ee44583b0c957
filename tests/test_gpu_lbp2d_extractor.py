"""GPU: the LBP2D image type through RadiomicsFeatureExtractor and through engine.roi_features_batch_types, on a 24^3 synthetic
case (int16, a smooth field plus noise, two labels) with binWidth = 1 and force2D.

  execute         every lbp-2D_* value equals, bit for bit, the original_* value of the same extractor run on the HOST-route LBP
                  image (filters.lbp2d_host, held to tests/lbp_reference.py) -- the class pipeline on the same image.
  executeLabels   on two labels equals the two execute calls, key for key and bit for bit (the image does not depend on the mask
                  and is shared).
  batched         roi_features_batch_types with "LBP2D" on the whole volume as the box equals execute on it: the image of a box is
                  that of the box alone, and here the box IS the image.  Texture features and order statistics bit for bit; the
                  summed first-order features come from the batched kernel's own summation order and are not compared here
                  (tests/test_gpu_batch_firstorder.py holds them to their bounds)."""
import numpy as np
import pytest

import lbp_reference as lr
from test_gpu_labels_batched import EXACT_FO, SUMMED

pytestmark = pytest.mark.gpu

LBP = {"lbp2DRadius": 1.5, "lbp2DSamples": 8, "lbp2DMethod": "uniform"}
SETTING = {"binWidth": 1, "force2D": True, "force2Ddimension": 0}
_cache = {}


def _bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def _case():
    if "case" not in _cache:
        rng = np.random.default_rng(24)
        z, y, x = np.mgrid[0:24, 0:24, 0:24].astype(np.float64)
        img = (200 * np.sin(z / 3.0) * np.cos(y / 4.0) + 10 * x + rng.normal(0, 25, (24, 24, 24))).astype(np.int16)
        lab = np.zeros(img.shape, dtype=np.int16)
        lab[((z - 8) ** 2 + (y - 9) ** 2 + (x - 10) ** 2) <= 5.5 ** 2] = 1
        lab[14:21, 12:22, 4:19] = 2
        lab[16, 15, 8:12] = 0
        _cache["case"] = (img, lab)
    return _cache["case"]


def _extractor(types):
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    return RadiomicsFeatureExtractor({"imageType": types, "setting": dict(SETTING)})


def _executed(label):
    if ("run", label) not in _cache:
        img, lab = _case()
        _cache[("run", label)] = _extractor({"Original": {}, "LBP2D": dict(LBP)}).execute(img, lab, label=label)
    return _cache[("run", label)]


@pytest.mark.parametrize("label", [1, 2])
def test_execute_equals_the_class_pipeline_on_the_host_route_image(label):
    from pyradiomics_amd import filters
    img, lab = _case()
    got = _executed(label)
    host = filters.lbp2d_host(img, LBP["lbp2DRadius"], LBP["lbp2DSamples"], LBP["lbp2DMethod"], 0)
    assert host.dtype == np.int16 and np.array_equal(host, lr.lbp_volume(img, 8, 1.5, "uniform", 0))
    want = _extractor({"Original": {}}).execute(host, lab, label=label)
    keys = [k for k in got if k.startswith("lbp-2D_")]
    assert len(keys) == len([k for k in want if k.startswith("original_")]) > 80
    for k in keys:
        assert _bits(got[k]) == _bits(want["original_" + k[len("lbp-2D_"):]]), k
    plain = _extractor({"Original": {}}).execute(img, lab, label=label)
    for k in plain:
        if k.startswith("original_"):
            assert _bits(got[k]) == _bits(plain[k]), k


def test_execute_labels_shares_the_image():
    img, lab = _case()
    both = list(_extractor({"Original": {}, "LBP2D": dict(LBP)}).executeLabels(img, lab, labels=[1, 2]))
    assert [l for l, _ in both] == [1, 2]
    for label, res in both:
        want = _executed(label)
        assert list(res) == list(want)
        for k, v in want.items():
            if not k.startswith("diagnostics_"):
                assert _bits(res[k]) == _bits(v), (label, k)


@pytest.mark.parametrize("label", [1, 2])
def test_batched_types_call_equals_execute_on_the_box(label):
    import torch
    from pyradiomics_amd import cmatrices, engine
    img, lab = _case()
    want = _executed(label)
    box, mask = torch.from_numpy(img).cuda(), torch.from_numpy((lab == label).astype(np.uint8)).cuda()
    # (LBP2D alone: with binWidth = 1 the Original image has hundreds of grey levels, beyond the batched texture kernels)
    tables, status = engine.roi_features_batch_types([box], [mask], imageTypes={"LBP2D": dict(LBP)}, extras=True, **SETTING)
    assert status == [1] and list(tables) == ["lbp-2D"] and engine.last_batch_route() == "batch"
    held = {cls: (cmatrices.FIRSTORDER_FEATURES if cls == "firstorder" else cmatrices.batch_feature_names(cls))
            for cls in engine.ROI_FEATURE_CLASSES}
    compared = 0
    for key, w in want.items():
        if not key.startswith("lbp-2D_"):
            continue
        image, cls, feat = key.rsplit("_", 2)
        value = tables[image][cls][0][held[cls].index(feat)]
        if cls == "glcm" and feat == "MCC":          # as RadiomicsGLCM reports it: the flat mean over the angles
            value = cmatrices._mcc_angle_mean(tables[image]["glcm_mcc_angles"][0])
        if cls != "firstorder" or feat in EXACT_FO:
            assert _bits(value) == _bits(w), (key, float(value), float(w))
            compared += 1
        else:
            assert feat in SUMMED, key
    assert compared > 75

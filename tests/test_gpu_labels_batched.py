"""GPU: RadiomicsFeatureExtractor.executeLabels(batched=True) against the default mode of the same build.

Inputs (_inputs): a 40 x 44 x 48 float32 image -- a smooth field of a few grey values of amplitude plus noise of sigma 3, fixed
seed -- and an int16 label map with 14 labels:
    1, 2, 7      balls that touch volume faces (1: z = 0, y = 0, x = 0; 2: z = 39, y = 43; 7: x = 47, z = 39)
    3, 4, 5      blobs inside; 6 a block whose box overlaps the boxes of 3 and 5
    8            flat: extent 1 along z                            -> per-label steps ("single")
    9            three voxels: skipped by minimumROISize 5 in both modes
    10           a block inside the box of 14 (a foreign label there)
    11, 12       interleaved plane by plane: each box contains the other's voxels
    13           a steep ramp under it: 171 grey levels at binWidth 2  -> batched with recomputed pairs ("mixed": MCC is NaN in
                 the batched table above 64 levels)
    14           a box of 30 x 30 x 30 with holes (25 187 voxels)
At binWidth 2 every other label has 9 to 19 grey levels in the original image and at most 38 in a haar sub-band (checked on
the host while this was written; test_partition_follows_from_census_and_bin_edges asserts the original's counts).

Compared per label: the label and key sequences, every diagnostics value, every texture feature and the first-order order
statistics / counts bit for bit.  The SUMMED first-order features (Energy, TotalEnergy, Mean, MeanAbsoluteDeviation,
RobustMeanAbsoluteDeviation, RootMeanSquared, StandardDeviation, Variance, Skewness, Kurtosis) are compared on neither side with
the other: the batched kernel sums the sorted ROI in its own order.  They are checked against the long-double reference
(firstorder_reference.segment_reference on the host copy of the same crop) under the bounds of tests/test_gpu_batch_firstorder.py
(_feature_bounds: seg_bounds + derived_bounds) with the chain length K = max(11, ceil(m / 256) + 9) of the batched launch, and
firstorder_reference.k_reduction of the crop where the ROI went to the single call: the labels routed "single", the recomputed
pairs of a "mixed" label, and a ROI with more voxels than the batched launch sorts (label 14 in the float64 sub-bands)."""
import collections
import math

import numpy as np
import pytest

import firstorder_reference as fr
from test_gpu_batch_firstorder import _feature_bounds, _k

pytestmark = pytest.mark.gpu

FLAT, TINY, STEEP, ABSENT = 8, 9, 13, 99
SUMMED = ("Energy", "TotalEnergy", "Mean", "MeanAbsoluteDeviation", "RobustMeanAbsoluteDeviation", "RootMeanSquared",
          "StandardDeviation", "Variance", "Skewness", "Kurtosis")
EXACT_FO = ("Minimum", "Maximum", "Median", "10Percentile", "90Percentile", "InterquartileRange", "Range", "Entropy", "Uniformity")
TYPES = {"Original": {}, "Wavelet": {"wavelet": "haar"}, "LoG": {"sigma": [1.0]}}
RUN1 = {"binWidth": 2, "minimumROISize": 5}
RUN2 = {"binCount": 16, "voxelArrayShift": 100, "distances": [1, 2], "symmetricalGLCM": False, "minimumROISize": 5}
SUBSET = collections.OrderedDict([("glcm", ["MCC", "Contrast", "JointEntropy"]), ("firstorder", ["Mean", "Median", "Entropy", "StandardDeviation", "Kurtosis"]),
                                  ("glszm", ["ZoneEntropy", "SmallAreaEmphasis"]), ("ngtdm", ["Coarseness"]), ("glrlm", ["RunEntropy"]), ("gldm", [])])


def _inputs():
    rng = np.random.default_rng(2024)
    shape = (40, 44, 48)
    z, y, x = np.mgrid[0:40, 0:44, 0:48].astype(np.float64)
    img = 60.0 + 5.0 * np.sin(z / 9.0) + 4.0 * np.cos(y / 8.0) + 3.0 * np.sin((x + y) / 11.0) + rng.normal(0.0, 3.0, shape)
    lab = np.zeros(shape, dtype=np.int16)

    def ball(label, c, r, squeeze=(1.0, 1.0, 1.0)):
        d = ((z - c[0]) * squeeze[0]) ** 2 + ((y - c[1]) * squeeze[1]) ** 2 + ((x - c[2]) * squeeze[2]) ** 2
        lab[(d <= r * r) & (lab == 0)] = label
    lab[5:35, 6:36, 16:46] = 14
    lab[8:30, 10:30, 20:40][rng.random((22, 20, 20)) < 0.15] = 0
    ball(1, (3, 4, 4), 4.5)
    ball(2, (36, 40, 4), 5.0)
    ball(3, (20, 22, 6), 5.5, (1.0, 0.6, 1.0))
    ball(4, (12, 38, 8), 3.2)
    ball(5, (30, 8, 7), 4.0, (0.7, 1.0, 1.0))
    lab[14:26, 2:12, 2:13][lab[14:26, 2:12, 2:13] == 0] = 6
    ball(7, (37, 20, 44), 3.0)
    lab[2, 38:43, 30:40] = FLAT
    lab[38, 2, 20:23] = TINY
    lab[10:16, 12:18, 22:28] = 10
    lab[20:27, 20:28, 30:37][::2, :, :] = 11
    lab[20:27, 20:28, 30:37][1::2, :, :] = 12
    lab[1:5, 14:30, 1:14] = STEEP
    img[1:5, 14:30, 1:14] += 27.0 * (x[1:5, 14:30, 1:14] - 1.0)
    return img.astype(np.float32), lab


_cache = {}


def _extractor(setting, subset=None, types=TYPES):
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    ex = RadiomicsFeatureExtractor({"imageType": types, "setting": dict(setting)})
    if subset is not None:
        ex.disableAllFeatures()
        ex.enableFeaturesByName(**subset)
    return ex


def _both(name, setting, subset=None, types=TYPES):
    """(default-mode results, batched results, route, recomputed pairs, derived images of the batched run), computed once"""
    if name not in _cache:
        img, lab = _inputs()
        ex = _extractor(setting, subset, types)
        want = list(ex.executeLabels(img, lab))
        plain_route = ex.lastLabelsRoute()
        assert plain_route["batched"] == [] and plain_route["mixed"] == [] and plain_route["single"] == [l for l, _ in want]
        seen = []
        inner = ex._derivedImages

        def spy(image, mask, s):
            items = list(inner(image, mask, s))
            seen[:] = items
            return iter(items)
        ex._derivedImages = spy
        got = list(ex.executeLabels(img, lab, batched=True))
        derived = [(typeName, d.array, d.GetSpacing()) for d, typeName, _kw in seen]
        _cache[name] = (want, got, ex.lastLabelsRoute(), ex.lastLabelsRecomputed(), derived)
    return _cache[name]


def _bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def _compare(name, setting, subset=None):
    from pyradiomics_amd import engine, imageoperations
    import torch
    want, got, route, recomputed, derived = _both(name, setting, subset)
    img, lab = _inputs()
    assert [l for l, _ in got] == [l for l, _ in want]
    labels, counts, lo, hi = imageoperations._censusHost(lab)
    alo, ahi = imageoperations.alignedBox(lo, hi, lab.shape)
    box = {int(l): tuple(slice(int(a), int(b) + 1) for a, b in zip(alo[i], ahi[i])) for i, l in enumerate(labels)}
    shift = float(setting.get("voxelArrayShift", 0))
    worst = 0.0
    for (l, g), (_, w) in zip(got, want):
        assert list(g) == list(w), (l, [k for k in w if k not in g], [k for k in g if k not in w])
        assert type(g) is type(w)
        for k in w:
            cls_feat = k.split("_")[-2:]
            if k.startswith("diagnostics_"):
                assert g[k] == w[k], (l, k, g[k], w[k])
            elif cls_feat[0] != "firstorder" or cls_feat[1] in EXACT_FO:
                assert np.ndim(g[k]) == 0 and np.asarray(g[k]).dtype == np.float64
                assert _bits(g[k]) == _bits(w[k]), (l, k, g[k], w[k])
            else:
                assert cls_feat[1] in SUMMED, k
        # the summed first-order features: against the long-double reference of the same crop
        for typeName, arr, spacing in derived:
            names = [k for k in g if k.startswith(typeName + "_firstorder_") and k.split("_")[-1] in SUMMED]
            if not names:
                continue
            crop, roi = np.ascontiguousarray(arr[box[l]]), lab[box[l]] == l
            ref = fr.segment_reference(crop, roi, shift)
            cap = engine.batch_firstorder_max_roi(torch.float64 if crop.dtype == np.float64 else torch.float32)
            single = l in route["single"] or (l, typeName) in recomputed or ref["m"] > cap
            K = fr.k_reduction(crop.size, crop.dtype.itemsize) if single else _k(ref["m"])
            bounds = _feature_bounds(ref, K, float(np.multiply.reduce(spacing)))
            for k in names:
                wv, bd = bounds[k.split("_")[-1]]
                err = abs(float(g[k]) - wv)
                print("%-10s label %2d %-50s err %.3g bound %.3g K %d%s" % (name, l, k, err, bd, K, " (single)" if single else ""))
                worst = max(worst, err / bd if bd > 0 else (0.0 if err == 0 else math.inf))
                assert err <= bd, (l, k, float(g[k]), wv, err, bd, K)
    print("%s: worst error / bound of the summed first-order features %.3g" % (name, worst))
    return want, got, route, recomputed


def test_partition_follows_from_census_and_bin_edges():
    """what the route assertions below rest on, from the census and getBinEdges alone (no device)"""
    from pyradiomics_amd import imageoperations
    img, lab = _inputs()
    labels, counts, lo, hi = imageoperations._censusHost(lab)
    assert labels.tolist() == list(range(1, 15))
    ext = hi - lo + 1
    by = {int(l): i for i, l in enumerate(labels)}
    assert ext[by[FLAT]].tolist()[0] == 1 and counts[by[TINY]] == 3 and ext[by[14]].tolist() == [30, 30, 30]
    flat = [int(l) for l in labels if (ext[by[int(l)]] == 1).any()]
    assert flat == [FLAT, TINY]
    for l in labels:
        ng = len(imageoperations.getBinEdges(img[lab == l], binWidth=RUN1["binWidth"])) - 1
        if l == STEEP:
            assert ng > 64, ng
        elif l != TINY:
            assert 8 <= ng <= 64 and 30 <= counts[by[int(l)]], (l, ng)
    # two labels with overlapping boxes, each holding voxels of the other
    a, b = by[11], by[12]
    assert (lo[a] <= hi[b]).all() and (lo[b] <= hi[a]).all()
    assert (lab[tuple(slice(int(x), int(y) + 1) for x, y in zip(lo[a], hi[a]))] == 12).any()
    # boxes that touch the volume faces
    assert (lo[by[1]] == 0).all() and hi[by[2]][0] == 39 and hi[by[2]][1] == 43 and hi[by[7]][2] == 47


def test_batched_equals_default_mode():
    want, got, route, recomputed = _compare("run1", RUN1)
    labels = [l for l, _ in want]
    assert labels == [l for l in range(1, 15) if l != TINY]          # (the 3-voxel label is skipped in both modes)
    assert route["single"] == [FLAT]
    assert route["mixed"] == [STEEP]
    assert route["batched"] == [l for l in labels if l not in (FLAT, STEEP)]
    assert (STEEP, "original") in recomputed and all(l == STEEP for l, _ in recomputed)
    # NaN never stands in for a value: MCC of the steep label is the class pipeline's
    g13, w13 = dict(got)[STEEP], dict(want)[STEEP]
    assert not np.isnan(g13["original_glcm_MCC"]) and _bits(g13["original_glcm_MCC"]) == _bits(w13["original_glcm_MCC"])
    assert sum(k.startswith("wavelet-") for k in g13) == 8 * sum(k.startswith("original_") for k in g13)
    assert any(k.startswith("log-sigma-1-0-mm-3D_glszm_") for k in g13)


def test_batched_equals_default_mode_with_other_settings_and_a_feature_subset():
    want, got, route, recomputed = _compare("run2", RUN2, SUBSET)
    assert route["single"] == [FLAT] and TINY not in [l for l, _ in got]
    assert len(route["batched"]) + len(route["mixed"]) == 12 and len(route["batched"]) >= 11
    keys = [k for k in dict(got)[1] if k.startswith("original_")]
    assert keys[:3] == ["original_glcm_MCC", "original_glcm_Contrast", "original_glcm_JointEntropy"]      # the order asked for
    assert keys[3:8] == ["original_firstorder_" + f for f in SUBSET["firstorder"]]
    assert sum(k.startswith("original_gldm_") for k in keys) == 14                                         # [] = every feature not deprecated


def test_absent_label_of_an_explicit_list_fails_at_its_position():
    img, lab = _inputs()
    for batched in (False, True):
        ex = _extractor(RUN1, types={"Original": {}})
        seen = []
        with pytest.raises(ValueError, match="not present"):
            for l, res in ex.executeLabels(img, lab, labels=[4, FLAT, 1, ABSENT, 2], batched=batched):
                seen.append((l, res["diagnostics_Mask-original_VoxelNum"]))
        assert [l for l, _ in seen] == [4, FLAT, 1], (batched, seen)
    # and with an explicit list the order is the list's, a too small label fails where it stands
    ex = _extractor(RUN1, types={"Original": {}})
    seen = []
    with pytest.raises(ValueError, match="too few dimensions|too small"):
        for l, _ in ex.executeLabels(img, lab, labels=[12, 3, TINY, 5], batched=True):
            seen.append(l)
    assert seen == [12, 3]
    ordered = list(ex.executeLabels(img, lab, labels=[12, 3, FLAT, 5], batched=True))
    assert [l for l, _ in ordered] == [12, 3, FLAT, 5]
    assert ex.lastLabelsRoute() == {"batched": [12, 3, 5], "single": [FLAT], "mixed": []}
    assert ordered[0][1]["diagnostics_Configuration_Settings"]["label"] == 12


@pytest.mark.parametrize("extra", [{"weightingNorm": "manhattan"}, {"force2D": True}])
def test_settings_outside_the_batched_kernels_route_every_label_single(extra):
    name = "single-" + next(iter(extra))
    want, got, route, recomputed, _ = _both(name, dict(RUN1, **extra), types={"Original": {}})
    labels = [l for l, _ in want]
    assert route == {"batched": [], "single": labels, "mixed": []} and recomputed == [] and len(labels) >= 12
    assert [l for l, _ in got] == labels
    for (l, g), (_, w) in zip(got, want):
        assert list(g) == list(w)
        for k in w:
            if k.startswith("diagnostics_"):
                assert g[k] == w[k], (l, k)
            else:
                assert _bits(g[k]) == _bits(w[k]), (l, k)

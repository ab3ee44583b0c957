"""GPU: the composite batched extraction calls of pyradiomics_amd.roi_batch -- roi_features_batch, roi_features_batch_images,
_derived, _types and _resampled -- on the ragged, degenerate batch of tests/composite_cases.py: four boxes of one shape
interleaved with others, an empty mask, a one-voxel mask, a constant ROI, a planar box, masks on the x faces, per-ROI spacing,
binWidth (every ROI its own number of levels, several above 64), all four element types.

Witnesses, per ROI b of a batch:
W1, the extractor: RadiomicsFeatureExtractor(...).execute(Image(box_b, spacing_b), Image(mask_b, spacing_b)) with the same
    settings and no preCrop -- the box is the whole image, so execute() filters and resamples exactly the array the batched call is
    handed.  Texture features and the first-order features of EXACT_FO bit for bit (a NaN equals a NaN); the SUMMED first-order
    features against firstorder_reference.segment_reference of the image the features were computed on under _feature_bounds, with
    K = _k(m), or firstorder_reference.k_reduction where the ROI exceeds batch_firstorder_max_roi -- as the four *_features tests do.
W1', where execute() refuses the ROI (the one-voxel ROI: "mask has too few dimensions"): the values of
    RadiomicsFeatureExtractor.computeFeatures on the numpy-cut tight crop, the recompute path of _batchedLabels.  The empty ROI's
    whole expectation is status 0 and NaN rows in every table.
W2, the batch of one: the same composite call on ROI b alone gives ROI b's rows of every table, gray_levels and glcm_mcc_angles
    bit for bit, the summed first-order columns included (one workgroup owns a ROI whatever the batch holds).
Logarithm and Exponential keep the rule of tests/test_gpu_batch_intensity_features.py: no W1, neither its comparison with
    execute() nor its summed columns; their tables are bit-equal to roi_features_batch on intensity_batch's rows cut to the tight
    boxes with numpy (composite_cases.tight_restated); W2 applies.  (Measured once with the summed columns held as for the other
    images: all inside their bounds but those of the constant ROI's Exponential image, 160 voxels that all equal exp(log(7) / 7 * 7)
    = 7.000000000000001: the batched mean is one ulp, 8.9e-16, off that value, so Variance is 7.9e-31 and Skewness and Kurtosis are 1
    where the long-double reference has 0 with a bound of 0 -- seg_bounds is first order in the rounding of the mean and the ratios
    are not continuous at a variance of 0.  The class's expressions do the same on such a ROI.)

Documented behaviour that is asserted as documented:
  * MCC: roi_features_batch leaves the MCC column NaN (and glcm_mcc_angles None) for a ROI whose discretisation has more than 64
    levels (its docstring); the extractor has a value there.  W1 asserts the NaN for exactly the ROIs whose bin_batch count exceeds
    64 and compares every other ROI.  For a ROI of one grey level the class reports 1 (the rule of _batchedLabels).
  * The one-voxel ROI has status 1: status 0 is "an empty ROI" alone.  Its tight box is 1 x 1 x 4 (the voxel lies on the right x
    face, alignedBox grows it left by 3), on which the class pipeline yields values: W1'.  In test_resampled_ragged every axis of
    its bounding box is one voxel thick, so it is a crop of ONE voxel; the class pipeline declines such a crop (NotImplementedError,
    "0 / 0 angles"), which is asserted, and W2 and the summed columns hold the ROI.
  * The planar box (1, 12, 16) is declined by the wavelet planner for coif1, and so are the boxes with an extent below the six
    taps, (4, 5, 8) and (5, 4, 7); the expectation is read from batch_swt_plan, not hard-coded.
  * test_between_the_caps_and_above_64_levels bins with binWidth 50: at that width ROIs 0 and 1 stay at or below 64 levels and
    share the native calls, the many-levels ROI (120 levels) does not.
  * Only the all-zero box takes the single route's intensity images (INTENSITY_ZERO); the constant ROI (7) is native.  The
    Square, Logarithm and Exponential images of an all-zero box are NaN, on which execute() raises ValueError (no bin edges); the
    batched call raises the same error for the whole batch.  test_types_all_zero_box holds the box to W1 on the types whose
    images are finite on it (Original, SquareRoot, Gradient) and asserts the ValueError for Square on both sides.
  * roi_features_batch is handed tight boxes (as the composite calls hand them on): on a wider box its GLRLM is max(size) wide
    and a few GLRLM features differ from execute()'s in the last bit.

Found by this module and fixed with it: roi_features_batch_resampled cut a ROI whose spacing does not change (the added twelfth
ROI of test_resampled_ragged; x extent 7) to resample_batch's aligned crop, x grown to 8, while resampleImage -- execute() -- cuts
the bounding box itself.  The LoG of the wider crop differs on every ROI voxel (log-sigma-1-0-mm-3D_firstorder_Median -13.52
against -13.67, every LoG feature off), and original_glrlm_* differed in the last bit.  It now asks resample_batch for the
exact crop (alignCrop=False)."""
import math

import numpy as np
import pytest

import composite_cases as cc
import firstorder_reference as fr
import test_gpu_firstorder_limits as lim
from test_gpu_batch_firstorder import _feature_bounds, _k
from test_gpu_batch_log import _admitted
from test_gpu_batch_wavelet_features import _bits
from test_gpu_labels_batched import EXACT_FO, SUMMED

pytestmark = pytest.mark.gpu

ROUTE = "composite"
STATUS = [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1]
REFUSED = {cc.EMPTY, cc.ONE_VOXEL}          # execute() raises: label not present / too few dimensions


def _dev(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _volume(sp):
    return sp[:, 2] * sp[:, 1] * sp[:, 0]          # ((x * y) * z, the order of the feature class)


def _held():
    from pyradiomics_amd import cmatrices, engine
    return {cls: (cmatrices.FIRSTORDER_FEATURES if cls == "firstorder" else cmatrices.batch_feature_names(cls))
            for cls in engine.ROI_FEATURE_CLASSES}


def _same(a, b):
    a, b = np.float64(a), np.float64(b)
    return bool(np.isnan(a) and np.isnan(b)) or _bits(a) == _bits(b)


def _same_rows(x, y):
    if x is None or y is None:
        return x is None and y is None
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype.kind == "f":
        nan = np.isnan(x)
        return bool(np.array_equal(nan, np.isnan(y)) and x[~nan].tobytes() == y[~nan].tobytes())
    return x.tobytes() == y.tobytes()


def _split(flat, sizes):
    """a flat batch tensor or array -> the list of its boxes as numpy arrays"""
    host = flat.cpu().numpy() if hasattr(flat, "cpu") else np.asarray(flat)
    off = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64).prod(1))])
    return [np.ascontiguousarray(host[off[b]:off[b + 1]].reshape(tuple(int(s) for s in sizes[b]))) for b in range(len(sizes))]


def _levels(images, masks, binning):
    """bin_batch's level count per ROI of one image (the count roi_features_batch hands to its texture calls)"""
    from pyradiomics_amd import engine
    return engine.bin_batch(_dev(images), _dev(masks), **binning)[1]


def _compare(label, b, tables, want, ng, held, differ):
    """the values `want` ({<image>_<class>_<feature>: value}, as execute() and computeFeatures return them) against ROI b's
    rows; -> the image names seen"""
    from pyradiomics_amd import cmatrices
    seen = set()
    for key, w in want.items():
        if key.startswith("diagnostics_"):
            continue
        image, cls, feat = key.rsplit("_", 2)
        table = tables[image]
        seen.add(image)
        if cls == "firstorder" and feat not in EXACT_FO:
            assert feat in SUMMED, key
            continue
        value = table[cls][b][held[cls].index(feat)]
        if cls == "glcm" and feat == "MCC":
            angles = table["glcm_mcc_angles"][b]
            if ng[image][b] > 64:          # (documented: no MCC above 64 levels)
                if not (np.isnan(value) and angles is None):
                    differ.append((label, b, key, "MCC above 64 levels", float(value)))
                continue
            # as RadiomicsGLCM reports it: 1 for a ROI of one grey level, else the flat mean over the angles
            value = 1.0 if table["gray_levels"][b] < 2 else (np.nan if angles is None else cmatrices._mcc_angle_mean(angles))
        if not _same(value, w):
            differ.append((label, b, key, float(value), float(w)))
    return seen


def _summed(label, route, b, name, table, image, mask, vol, held, differ):
    """the SUMMED first-order columns of ROI b against the long-double reference of the image they were computed on"""
    import torch
    from pyradiomics_amd import engine
    image = np.ascontiguousarray(image)
    ref = fr.segment_reference(image, np.ascontiguousarray(mask), 0.0)
    cap = engine.batch_firstorder_max_roi(torch.float64 if image.dtype == np.float64 else torch.float32)
    K = fr.k_reduction(image.size, image.dtype.itemsize) if ref["m"] > cap else _k(ref["m"])
    bounds = _feature_bounds(ref, K, float(vol))
    for feat in SUMMED:
        wv, bd = bounds[feat]
        got = float(table["firstorder"][b][held["firstorder"].index(feat)])
        if np.isnan(wv) or np.isnan(got):
            ok, ratio = bool(np.isnan(wv) and np.isnan(got)), 0.0
        else:
            err = abs(got - wv)
            ratio = err / bd if bd > 0 else (0.0 if err == 0 else math.inf)
            ok = err <= bd
        lim._note("%s-%s-%s" % (ROUTE, label.split("[")[0], route), {feat: ratio})
        if not ok:
            differ.append((label, b, name, feat, got, wv, bd, K))


def _w2(label, b, tables, status, alone, differ):
    one, st = alone
    if st != [status[b]] or list(one) != list(tables):
        differ.append((label, b, "W2 status / names", st, list(one)))
        return
    for name, table in tables.items():
        if list(one[name]) != list(table):
            differ.append((label, b, name, "W2 keys", list(one[name])))
            continue
        for key, rows in table.items():
            if not _same_rows(rows[b], one[name][key][0]):
                differ.append((label, b, name, key, "W2", rows[b], one[name][key][0]))


def _check(label, call, tables, status, route, expect, images, masks, sp, types, setting, exec_inputs, refused, custom, binning,
           no_image=None, loose=(), w2=True):
    """every ROI of one composite call through W1 / W1' / W2.
    call(idx): the composite call on the ROIs idx alone; expect: the status; images: {image name: [the array the features of ROI
    b were computed on]}, masks: [the mask they saw], sp: their spacing (z, y, x) [B, 3]; types / setting: the extractor's;
    exec_inputs: [(box, mask, spacing)] as execute() is handed them; refused: ROIs execute() must refuse; custom(name): the
    settings of that image's type; binning(name): its binning; no_image: {name: ROIs without that image}; loose: names without W1"""
    from pyradiomics_amd import engine
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image
    B, held, differ = len(masks), _held(), []
    no_image = no_image or {}
    assert status == list(expect), (label, status)
    assert list(tables) == list(images), (label, list(tables), list(images))
    ng = {name: _levels(images[name], masks, binning(name)) for name in tables}
    bounds = cc.tight_restated(masks)[2]
    vol = _volume(sp)
    ex = RadiomicsFeatureExtractor({"imageType": types, "setting": dict(setting)})
    exact = [n for n in tables if n not in loose]
    for b in range(B):
        box, mask, spb = exec_inputs[b]
        xyz = tuple(float(s) for s in spb[::-1])
        args = (Image(box, xyz), Image(np.ascontiguousarray(mask).astype(np.uint8), xyz))
        missing = {n for n in tables if b in no_image.get(n, ())}
        for n in missing:
            for cls in engine.ROI_FEATURE_CLASSES:
                assert np.isnan(tables[n][cls][b]).all(), (label, b, n, cls)
        if not expect[b]:          # the empty ROI: NaN everywhere
            with pytest.raises(ValueError):
                ex.execute(*args, label=1)
            for n, table in tables.items():
                for cls in engine.ROI_FEATURE_CLASSES:
                    assert np.isnan(table[cls][b]).all(), (label, b, n, cls)
        else:
            if b in refused:
                with pytest.raises(ValueError):
                    ex.execute(*args, label=1)
                (lo, hi), seen = bounds[b], set()
                cut = (slice(lo[0], hi[0] + 1), slice(lo[1], hi[1] + 1), slice(lo[2], hi[2] + 1))
                for n in exact:
                    if n in missing:
                        continue
                    xyz_f = tuple(float(s) for s in sp[b][::-1])
                    kw = dict(ex.settings)
                    kw.update(custom(n))
                    kw.update(label=1, deviceResident=True)
                    crop = np.ascontiguousarray(images[n][b][cut])
                    try:
                        want = ex.computeFeatures(Image(crop, xyz_f), Image(np.ascontiguousarray(masks[b][cut]).astype(np.uint8), xyz_f),
                                                  n, **kw)
                    except NotImplementedError:
                        # the class pipeline declines a crop of ONE voxel ("0 / 0 angles"): W2 and the summed columns hold this ROI
                        assert crop.size == 1, (label, b, n, crop.shape)
                        seen.add(n)
                        continue
                    seen |= _compare(label, b, tables, want, ng, held, differ)
            else:
                seen = _compare(label, b, tables, ex.execute(*args, label=1), ng, held, differ)
            assert seen == set(exact) - missing, (label, b, sorted(seen), sorted(set(exact) - missing))
            for n, table in tables.items():
                if n not in missing and n not in loose:
                    _summed(label, route, b, n, table, images[n][b], masks[b], vol[b], held, differ)
        if w2:
            _w2(label, b, tables, status, call([b]), differ)
    for d in differ[:60]:
        print("DIFFER", d)
    assert not differ, (label, len(differ), differ[:6])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16, np.int32])
def test_original_ragged(dtype):
    from pyradiomics_amd import engine
    boxes, masks, sp, _ = cc.ragged_batch(dtype)
    I, M, vol = _dev(boxes), _dev(masks), _volume(sp)

    def call(idx):
        return engine.roi_features_batch_images([I[b] for b in idx], [M[b] for b in idx], imageTypes={"Original": {}}, binWidth=25,
                                                voxelVolume=vol[idx], spacing=sp[idx], extras=True)
    tables, status = call(list(range(len(I))))
    route = engine.last_batch_route()
    print("route %s" % route)
    levels = tables["original"]["gray_levels"]
    assert levels[cc.CONSTANT] == 1 and levels[cc.EMPTY] == 0
    _, Ng, _, counts = engine.bin_batch(I, M, binWidth=25)
    assert levels.tolist() == [int((c[1:] > 0).sum()) for c in counts]
    live = [b for b in range(len(I)) if STATUS[b]]
    assert len({int(levels[b]) for b in live}) > 1 and len({int(Ng[b]) for b in live}) > 1          # `same` is false
    assert (Ng > 64).any() and (Ng[live] <= 64).any() and route == "mixed"                          # `few` is mixed
    _check("original[%s]" % np.dtype(dtype).name, call, tables, status, route, STATUS, {"original": boxes}, masks, sp,
           {"Original": {}}, {"binWidth": 25}, list(zip(boxes, masks, sp)), REFUSED, lambda n: {}, lambda n: {"binWidth": 25})


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _wavelet_images(I, sizes, wavelet):
    from pyradiomics_amd import engine
    bands, names, _ = engine.wavelet_batch(I, wavelet=wavelet)
    route = engine.last_batch_route()
    host = bands.cpu().numpy()
    return {n: _split(host[r], sizes) for n, r in zip(names, names.rows)}, list(names), route


def test_bincount_and_per_type_overrides():
    from pyradiomics_amd import engine
    boxes, masks, sp, _ = cc.ragged_batch(np.float32)
    I, M, vol = _dev(boxes), _dev(masks), _volume(sp)
    types = {"Wavelet": {"binCount": 8, "wavelet": "haar"}, "Original": {"binWidth": 10}}

    def call(idx):
        return engine.roi_features_batch_images([I[b] for b in idx], [M[b] for b in idx], imageTypes=types, binWidth=25,
                                                voxelVolume=vol[idx], spacing=sp[idx], extras=True)
    tables, status = call(list(range(len(I))))
    route = engine.last_batch_route()
    print("route %s" % route)
    images, names, wroute = _wavelet_images(I, np.array(cc.SHAPES), "haar")
    assert wroute == "batch"                                   # haar is native on every box of the catalogue
    assert list(tables) == names + ["original"]                # the order of imageTypes' keys
    images["original"] = boxes
    for n in names:                                            # binCount 8 reached the wavelet tables and them alone
        assert (tables[n]["gray_levels"][[b for b in range(len(I)) if STATUS[b]]] <= 8).all(), n
    assert tables["original"]["gray_levels"].max() > 8
    custom = lambda n: types["Original"] if n == "original" else types["Wavelet"]
    binning = lambda n: {"binWidth": 10} if n == "original" else {"binCount": 8}
    _check("overrides", call, tables, status, route, STATUS, images, masks, sp, types, {"binWidth": 25},
           list(zip(boxes, masks, sp)), REFUSED, custom, binning)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_wavelet_ragged():
    from pyradiomics_amd import engine
    boxes, masks, sp, _ = cc.ragged_batch(np.float32)
    I, M, vol = _dev(boxes), _dev(masks), _volume(sp)
    types = {"Original": {}, "Wavelet": {"wavelet": "coif1"}}

    def call(idx):
        return engine.roi_features_batch_images([I[b] for b in idx], [M[b] for b in idx], imageTypes=types, binWidth=25,
                                                voxelVolume=vol[idx], spacing=sp[idx], extras=True)
    tables, status = call(list(range(len(I))))
    route = engine.last_batch_route()
    print("route %s" % route)
    verdict = engine.batch_swt_plan(np.array(cc.SHAPES), 6)[0]
    declined = int((verdict != 0).sum())
    assert verdict[cc.PLANAR] != 0, "the planner takes the planar box for coif1"
    assert 0 < declined < len(I)
    images, names, wroute = _wavelet_images(I, np.array(cc.SHAPES), "coif1")
    assert wroute == "mixed" and route == "mixed"              # what batch_swt_plan says: some boxes native, some looped
    assert list(tables) == ["original"] + names
    images = dict([("original", boxes)] + [(n, images[n]) for n in names])
    _check("wavelet", call, tables, status, route, STATUS, images, masks, sp, types, {"binWidth": 25},
           list(zip(boxes, masks, sp)), REFUSED, lambda n: types["Original" if n == "original" else "Wavelet"],
           lambda n: {"binWidth": 25})


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_log_partly_valid():
    import torch
    from pyradiomics_amd import engine
    boxes, masks, sp, _ = cc.ragged_batch(np.float32)
    I, M, vol = _dev(boxes), _dev(masks), _volume(sp)
    sigma = [1.0, 3.0]
    types = {"Original": {}, "LoG": {"sigma": sigma}}
    B = len(I)

    def call(idx):
        return engine.roi_features_batch_derived([I[b] for b in idx], [M[b] for b in idx], imageTypes=types, binWidth=25,
                                                 voxelVolume=vol[idx], spacing=sp[idx], extras=True)
    tables, status = call(list(range(B)))
    route = engine.last_batch_route()
    print("route %s" % route)
    admitted = np.array([[_admitted(cc.SHAPES[b], sp[b], s) for b in range(B)] for s in sigma])
    assert admitted[1].any() and not admitted[1].all(), "the catalogue needs a valid and an invalid ROI at sigma 3.0"
    W = sum(int(np.prod(s)) for s in cc.SHAPES)
    out = torch.full((2, W), float("nan"), dtype=torch.float32, device=I[0].device)
    logs, names, sizes, valid = engine.log_batch(I, sigma=sigma, spacing=sp, out=out)
    assert np.array_equal(valid, admitted), (valid, admitted)
    assert list(tables) == ["original"] + list(names)
    images, no_image = {"original": boxes}, {}
    host = logs.cpu().numpy()
    for s, n in enumerate(names):
        images[n] = _split(host[s], sizes)
        no_image[n] = {b for b in range(B) if not admitted[s, b]}
        for b in range(B):          # an invalid slice is not written, a valid one holds no NaN
            assert np.isnan(images[n][b]).all() if b in no_image[n] else not np.isnan(images[n][b]).any(), (n, b)
        for b in no_image[n]:       # (the feature call saw the box itself there; its rows are NaN, see _check)
            images[n][b] = boxes[b]
    assert status == STATUS                                    # an invalid pair does not lower the status
    _check("log", call, tables, status, route, STATUS, images, masks, sp, types, {"binWidth": 25},
           list(zip(boxes, masks, sp)), REFUSED, lambda n: types["Original" if n == "original" else "LoG"],
           lambda n: {"binWidth": 25}, no_image=no_image)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
ALL_TYPES = {"Original": {}, "Square": {}, "SquareRoot": {}, "Logarithm": {}, "Exponential": {}, "Gradient": {}}
LOOSE = ("logarithm", "exponential")


def _types_case(label, boxes, masks, sp, types, use_spacing, expect, intensity_route, refused):
    import torch
    from pyradiomics_amd import engine
    I, M, vol = _dev(boxes), _dev(masks), _volume(sp)

    def call(idx):
        return engine.roi_features_batch_types([I[b] for b in idx], [M[b] for b in idx], imageTypes=types, binWidth=25,
                                               voxelVolume=vol[idx], spacing=sp[idx], gradientUseSpacing=use_spacing, extras=True)
    tables, status = call(list(range(len(I))))
    route = engine.last_batch_route()
    print("route %s" % route)
    assert list(tables) == [t.lower() for t in types]
    sizes = np.array([b.shape for b in boxes])
    kinds = [t for t in engine.INTENSITY_TYPES if t in types]
    rows, names, _ = engine.intensity_batch(I, types=kinds)
    assert engine.last_batch_route() == intensity_route
    assert route == "mixed"          # (ROIs above 64 levels take the single texture calls whatever the images' route is)
    grad, _, _ = engine.gradient_batch(I, spacing=sp, gradientUseSpacing=use_spacing)
    images = {"original": boxes}
    images.update({n: _split(rows[i], sizes) for i, n in enumerate(names)})
    images["gradient"] = _split(grad, sizes)
    images = {n: images[n] for n in tables}
    # Logarithm and Exponential: bit-equal to roi_features_batch on intensity_batch's rows cut to the tight boxes with numpy
    idx, tight, _ = cc.tight_restated(masks)
    pick = torch.from_numpy(idx).to(I[0].device)
    flat_mask = torch.cat([m.reshape(-1) for m in M]).view(torch.uint8)
    loose = tuple(n for n in LOOSE if n in tables)
    for n in loose:
        table, st = engine.roi_features_batch(rows[names.index(n)][pick], flat_mask[pick], tight, binWidth=25, voxelVolume=vol,
                                              spacing=sp, extras=True)
        assert st == status
        for key in table:
            for b in range(len(I)):
                assert _same_rows(table[key][b], tables[n][key][b]), (n, key, b)
    exact = {t: c for t, c in types.items() if t.lower() not in LOOSE}
    _check(label, call, tables, status, route, expect, images, masks, sp, exact,
           {"binWidth": 25, "gradientUseSpacing": use_spacing}, list(zip(boxes, masks, sp)), refused, lambda n: {},
           lambda n: {"binWidth": 25}, loose=loose)


@pytest.mark.parametrize("use_spacing", [True, False])
def test_types_ragged(use_spacing):
    boxes, masks, sp, _ = cc.ragged_batch(np.float32)
    _types_case("types[%s]" % use_spacing, boxes, masks, sp, ALL_TYPES, use_spacing, STATUS, "batch", REFUSED)


def test_types_all_zero_box():
    """An all-zero box beside three ROIs of the catalogue.  Its SquareRoot image comes from the single route (INTENSITY_ZERO:
    route "mixed") and is all zeros, like the box and its Gradient: one grey level, held to W1 like every other ROI.  Its Square,
    Logarithm and Exponential images are NaN (the formulas divide by zero), which no binning takes: execute() raises ValueError
    on that box, and so does the batched call -- for the whole batch, which is asserted here as it stands."""
    from pyradiomics_amd import engine
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image
    ragged, rmasks, rsp, _ = cc.ragged_batch(np.float32)
    keep = [0, cc.CONSTANT, 1]
    boxes, masks = [ragged[b] for b in keep] + [np.zeros((4, 4, 5), dtype=np.float32)], [rmasks[b] for b in keep] + [np.ones((4, 4, 5), dtype=bool)]
    sp = np.concatenate([rsp[keep], [cc.ODD_SPACING]])
    finite = {"Original": {}, "SquareRoot": {}, "Gradient": {}}
    _types_case("types[zero]", boxes, masks, sp, finite, True, [1, 1, 1, 1], "mixed", set())
    outcome = []
    for what in ("batched", "extractor"):
        try:
            if what == "batched":
                engine.roi_features_batch_types(_dev(boxes), _dev(masks), imageTypes={"Square": {}}, binWidth=25)
            else:
                xyz = tuple(float(s) for s in sp[3][::-1])
                RadiomicsFeatureExtractor({"imageType": {"Square": {}}, "setting": {"binWidth": 25}}).execute(
                    Image(boxes[3], xyz), Image(masks[3].astype(np.uint8), xyz), label=1)
            outcome.append((what, "values"))
        except ValueError as e:
            outcome.append((what, "ValueError: %s" % e))
    print("square of an all-zero box:", outcome)
    assert all(o.startswith("ValueError") for _, o in outcome), outcome


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_resampled_ragged(dtype):
    from pyradiomics_amd import engine
    new = (1.4, 0.8, 2.5)                                        # (x, y, z): the odd ROIs keep z and y, the even ones no axis
    boxes, masks, sp, _ = cc.ragged_batch(dtype)
    boxes.append(cc.values(dtype, (7, 9, 11), cc.SEED + 50))     # spacing = target: a pure crop, interpolator code 0
    masks.append(cc._ball((7, 9, 11), (3, 4, 5), 3))
    sp = np.concatenate([sp, [new[::-1]]])
    I, M = _dev(boxes), _dev(masks)
    B = len(I)
    sigma = [1.0]
    types = {"Original": {}, "LoG": {"sigma": sigma}}
    setting = {"binWidth": 25, "resampledPixelSpacing": list(new), "interpolator": "sitkBSpline", "padDistance": 5}

    def call(idx):
        return engine.roi_features_batch_resampled([I[b] for b in idx], [M[b] for b in idx], spacing=sp[idx],
                                                   resampledPixelSpacing=new, interpolator="sitkBSpline", padDistance=5,
                                                   imageTypes=types, binWidth=25, extras=True)
    tables, status = call(list(range(B)))
    route = engine.last_batch_route()
    print("route %s" % route)
    # the images the features were computed on: a ROI whose spacing stays is cut to its bounding box, as resampleImage cuts it
    out, out_m, sizes, new_sp, _, rstatus = engine.resample_batch(I, M, spacing=sp, resampledPixelSpacing=new, padDistance=5,
                                                                  alignCrop=False)
    lo, hi, count = engine.mask_boxes_batch(M)
    assert count.tolist() == [int(m.sum()) for m in masks]
    plan = engine.batch_resample_plan(np.array([b.shape for b in boxes]), lo, hi, sp, new, 5, alignCrop=False)
    assert plan.interpolator[B - 1] == 0 and plan.interpolator[0] == 3          # the pure crop beside resampled ROIs
    assert plan.interpolator[cc.ONE_VOXEL] == 0          # (one voxel: every axis is one voxel thick and keeps its spacing)
    assert tuple(sizes[B - 1]) == (7, 7, 7) and tuple(sizes[cc.ONE_VOXEL]) == (1, 1, 1)   # the bounding boxes, x not grown
    for b in range(B):                                   # the new spacing: the target along every axis the ROI is thick on
        want = np.where(hi[b] - lo[b] + 1 != 1, np.array(new)[::-1], sp[b]) if masks[b].any() else sp[b]
        assert np.array_equal(new_sp[b], want), (b, new_sp[b], want)
    new_masks = [m != 0 for m in _split(out_m, sizes)]
    expect = [int(bool(masks[b].any() and new_masks[b].any())) for b in range(B)]          # the status follows out_masks
    assert expect[cc.EMPTY] == 0 and sum(expect) >= B - 2
    assert rstatus.tolist() == [engine.RESAMPLE_EMPTY if b == cc.EMPTY else 0 for b in range(B)]
    logs, names, _, valid = engine.log_batch(out, sizes, sigma=sigma, spacing=new_sp)
    assert np.array_equal(valid, np.array([[_admitted(sizes[b], new_sp[b], s) for b in range(B)] for s in sigma]))
    images = {"original": _split(out, sizes)}
    no_image = {}
    host = logs.cpu().numpy()
    for s, n in enumerate(names):
        images[n] = _split(host[s], sizes)
        no_image[n] = {b for b in range(B) if not valid[s, b]}
        for b in no_image[n]:
            images[n][b] = images["original"][b]
    assert list(tables) == list(images)
    refused = {b for b in range(B) if expect[b] and int(((np.array([a.max() - a.min() for a in np.nonzero(new_masks[b])]) + 1) > 1).sum()) < 2}
    assert cc.ONE_VOXEL in refused or not expect[cc.ONE_VOXEL]
    _check("resampled[%s]" % np.dtype(dtype).name, call, tables, status, route, expect, images, new_masks, new_sp, types, setting,
           list(zip(boxes, masks, sp)), refused, lambda n: types["Original" if n == "original" else "LoG"],
           lambda n: {"binWidth": 25}, no_image=no_image)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_between_the_caps_and_above_64_levels():
    import torch
    from pyradiomics_amd import engine
    ragged, rmasks, _, _ = cc.ragged_batch(np.float32)
    big, bmask = cc.big_glszm()
    many, mmask = cc.many_levels()
    # roi_features_batch is handed tight boxes, as the composite calls hand them on: on a wider box the GLRLM is max(size) wide and
    # some of its features differ from execute()'s in their last bit (tests/test_gpu_batch_wavelet_features.py)
    tight = cc.tight_restated(rmasks)[2]
    cut = lambda a, b: np.ascontiguousarray(a[tuple(slice(l, h + 1) for l, h in zip(*tight[b]))])
    boxes = [cut(ragged[0], 0), big, many, cut(ragged[1], 1)]
    masks = [cut(rmasks[0], 0), bmask, mmask, cut(rmasks[1], 1)]
    BIG, MANY = 1, 2
    assert engine.batch_glszm_max_vox() < big.size <= engine.batch_max_vox()
    assert big.size > engine.batch_firstorder_max_roi(torch.float32)          # (and above the first-order launch's ROI size)
    sp = np.array([cc.EVEN_SPACING, cc.ODD_SPACING, cc.EVEN_SPACING, cc.ODD_SPACING])
    I, M, vol = _dev(boxes), _dev(masks), _volume(sp)

    def call(idx):
        return engine.roi_features_batch([I[b] for b in idx], [M[b] for b in idx], binWidth=50, voxelVolume=vol[idx],
                                         spacing=sp[idx], extras=True)
    table, status = call([0, 1, 2, 3])
    route = engine.last_batch_route()
    print("route %s" % route)
    assert route == "mixed" and status == [1, 1, 1, 1]
    levels, Ng, _, _ = engine.bin_batch(I, M, binWidth=50)
    assert Ng[MANY] > 64 and (Ng[[0, BIG, 3]] <= 64).all() and len(set(Ng.tolist())) > 1, Ng
    # the big ROI's GLSZM came from the single call (above the batched GLSZM's cap) beside the others' batched one
    lv = _split(levels, np.array([b.shape for b in boxes]))[BIG]
    P, zs = engine.glszm_compact(torch.from_numpy(lv).cuda(), M[BIG], int(Ng[BIG]), int(bmask.sum()))
    vals, empty = engine.zone_matrix_features(P, zs)
    assert not empty[0] and _bits(table["glszm"][BIG]) == _bits(vals[0])
    mcc = table["glcm"][:, 23]
    assert np.isnan(mcc).tolist() == [False, False, True, False]                  # NaN for the many-levels ROI only
    assert table["glcm_mcc_angles"][MANY] is None and all(table["glcm_mcc_angles"][b] is not None for b in (0, BIG, 3))
    def named(idx):
        one, st = call(idx)
        return {"original": one}, st
    _check("caps", named, {"original": table}, status, route, [1, 1, 1, 1],
           {"original": boxes}, masks, sp, {"Original": {}}, {"binWidth": 50}, list(zip(boxes, masks, sp)), set(), lambda n: {},
           lambda n: {"binWidth": 50})


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_zz_report():
    print()
    mine = {k: r for k, r in lim.RATIOS.items() if k[0].startswith(ROUTE + "-")}
    for (route, f), r in sorted(mine.items()):
        print("    %-36s %-28s %.3g" % (route, f, r))
    assert mine and all(r <= 1 for r in mine.values())

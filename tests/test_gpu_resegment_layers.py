"""GPU: resegmentation through the layers above the kernels -- the composite batched calls (roi_features_batch and
roi_features_batch_types with resegmentRange) against execute() on each box, execute() device-resident against its host-array
route in the three modes, and executeLabels with resegmentRange sharing the filter stack.

The composite comparison is that of tests/test_gpu_batch_composite_limits.py, whose helpers are used as they are: texture
features and the order statistics of the first-order class bit for bit against execute() on the box (_compare), the summed
first-order columns against the long-double reference of the image they were computed on, under that module's bounds (_summed),
with the mask the HOST resegmentation leaves.  A ROI that fails resegmentation (one voxel kept; empty on entry) has status 0 and
NaN rows, where execute() raises.

roi_features_batch takes the boxes as they are handed over (its docstring: the composite calls hand it tight boxes), so the boxes
of its test are built to stay tight under resegmentation: opposite corners hold the mean value, which every sigma range keeps,
and the x extent is a multiple of four.  roi_features_batch_types cuts the tight boxes itself, after resegmenting."""
import warnings

import numpy as np
import pytest

from labels_cases import A, B, C_, labels_case
from test_gpu_batch_composite_limits import _compare, _dev, _held, _summed

pytestmark = pytest.mark.gpu

RESEG = {"resegmentRange": [-1, 1], "resegmentMode": "sigma"}
FAILS = {3, 4}          # ROI 3 keeps one voxel, ROI 4 is empty on entry


def _boxes():
    g = np.random.default_rng(77)
    shapes = [(6, 7, 8), (8, 8, 8), (7, 6, 12), (6, 6, 8), (6, 7, 8)]
    boxes = [g.integers(0, 400, s).astype(np.int16) for s in shapes]
    masks = [np.ones(s, np.uint8) for s in shapes]
    for b in boxes[:3]:
        b[0, 0, 0] = b[-1, -1, -1] = 200
    masks[3][:] = 0
    masks[3][2, 3, 4] = 1
    masks[4][:] = 0
    return boxes, masks


def _host_masks(boxes, masks, setting):
    """the masks the host resegmentation leaves (None where it raises)"""
    from pyradiomics_amd import imageoperations
    from pyradiomics_amd.image import Image
    out = []
    for im, m in zip(boxes, masks):
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")          # (numpy's mean of the empty ROI)
                out.append((imageoperations.resegmentMask(Image(im), Image(m), label=1, **setting).array != 0).astype(np.uint8))
        except ValueError:
            out.append(None)
    return out


def _check(tables, status, boxes, masks, images, types, setting):
    """tables / status of a composite call against execute() per box; images: {image name: [array per ROI]}"""
    from pyradiomics_amd import engine
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image
    kept = _host_masks(boxes, masks, setting)
    assert [k is None for k in kept] == [b in FAILS for b in range(len(boxes))]
    assert status == [0 if b in FAILS else 1 for b in range(len(boxes))], status
    ex = RadiomicsFeatureExtractor({"imageType": types, "setting": dict(setting, binWidth=25)})
    held, differ = _held(), []
    ng = {name: np.zeros(len(boxes), dtype=np.int64) for name in tables}          # (no ROI here has more than 64 levels: MCC compared)
    for b in range(len(boxes)):
        args = (Image(boxes[b]), Image(masks[b]))
        if b in FAILS:
            with pytest.raises(ValueError):
                ex.execute(*args, label=1)
            for table in tables.values():
                for cls in engine.ROI_FEATURE_CLASSES:
                    assert np.isnan(table[cls][b]).all(), (b, cls)
            continue
        seen = _compare("resegment", b, tables, ex.execute(*args, label=1), ng, held, differ)
        assert seen == set(tables), (b, sorted(seen))
        for name, table in tables.items():
            _summed("resegment", "batch", b, name, table, images[name][b], kept[b], 1.0, held, differ)
    for d in differ[:40]:
        print("DIFFER", d)
    assert not differ, (len(differ), differ[:6])


def test_roi_features_batch_with_resegmentation_equals_execute():
    from pyradiomics_amd import engine
    boxes, masks = _boxes()
    kept = _host_masks(boxes, masks, RESEG)
    for b in range(3):          # the boxes stay tight: the kept ROI touches all six faces
        idx = np.nonzero(kept[b])
        assert all(i.min() == 0 and i.max() == s - 1 for i, s in zip(idx, boxes[b].shape)) and kept[b].sum() < kept[b].size
    table, status = engine.roi_features_batch(_dev(boxes), _dev(masks), binWidth=25, extras=True, **RESEG)
    assert engine.last_batch_route() == "batch"
    _check({"original": table}, status, boxes, masks, {"original": boxes}, {"Original": {}}, RESEG)
    # without the setting nothing changes: the call equals the one that never heard of it
    plain, st = engine.roi_features_batch(_dev(boxes), _dev(masks), binWidth=25)
    none, st2 = engine.roi_features_batch(_dev(boxes), _dev(masks), binWidth=25, resegmentRange=None, resegmentMode="sigma")
    assert st == st2 == [1, 1, 1, 1, 0]
    for cls in plain:
        assert plain[cls].tobytes() == none[cls].tobytes(), cls


def test_roi_features_batch_types_with_wavelet_and_resegmentation_equals_execute():
    from pyradiomics_amd import cmatrices, engine
    boxes, masks = _boxes()
    boxes[1][:] = np.random.default_rng(5).integers(0, 400, boxes[1].shape)          # (this call cuts its own tight boxes)
    types = {"Original": {}, "Wavelet": {}}
    tables, status = engine.roi_features_batch_types(_dev(boxes), _dev(masks), imageTypes=types, binWidth=25, extras=True,
                                                     **RESEG)
    bands, names = cmatrices.calculate_wavelet_batch(boxes)
    images = dict({"original": boxes}, **{n: bands[n] for n in names})
    assert list(tables) == ["original"] + list(names)
    _check(tables, status, boxes, masks, images, types, RESEG)


def _case():
    from pyradiomics_amd.image import Image
    vol, lab = labels_case()
    return Image(vol), Image(lab)


@pytest.mark.parametrize("setting", [{"resegmentRange": [-150, 420], "resegmentMode": "absolute"},
                                     {"resegmentRange": [0.35, 0.9], "resegmentMode": "relative"},
                                     {"resegmentRange": [-1.25, 1.5], "resegmentMode": "sigma"},
                                     {"resegmentRange": [0.4], "resegmentMode": "relative"}],
                         ids=["absolute", "relative", "sigma", "one-threshold"])
def test_execute_device_resident_equals_the_host_array_route(setting):
    """as test_device_resident_route_equals_host_array_route compares: device-resident matrices with the numpy formulas
    (fusedSegment False) against the host-array route -- every value that is not first order equal, first order within 1e-13
    (the device crop pads its rows: the same terms in another order)"""
    from pyradiomics_amd import _lib, backend, cmatrices
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    backend.set(cmatrices)
    lib = _lib.load()
    host = RadiomicsFeatureExtractor({"setting": dict(setting, binWidth=25, deviceResident=False)}).execute(*_case(), label=A)
    lib.prad_timing_begin()
    try:
        dev = RadiomicsFeatureExtractor({"setting": dict(setting, binWidth=25, fusedSegment=False)}).execute(*_case(), label=A)
        launched = lib.prad_timing_count(b"resegment")
    finally:
        lib.prad_timing_end()
    assert launched >= 1
    keys = [k for k in host if not k.startswith("diagnostics")]
    assert len(keys) > 90 and list(host) == list(dev)
    for k in keys:
        a, b = float(dev[k]), float(host[k])
        if "_firstorder_" in k:
            assert a == b or (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-13 * abs(b), (k, a, b)
        else:
            assert a == b or (np.isnan(a) and np.isnan(b)), (k, a, b)
    for k in ("diagnostics_Mask-resegmented_VoxelNum", "diagnostics_Mask-resegmented_BoundingBox",
              "diagnostics_Mask-original_VoxelNum", "diagnostics_Mask-original_BoundingBox"):
        assert dev[k] == host[k], k
    assert dev["diagnostics_Mask-resegmented_VoxelNum"] < dev["diagnostics_Mask-original_VoxelNum"]


def test_device_resident_execute_does_not_download_for_resegmentation(monkeypatch):
    """resegmentMask no longer calls as_array on a device-resident case"""
    from pyradiomics_amd import backend, cmatrices, imageoperations
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    backend.set(cmatrices)
    calls = []
    real = imageoperations.as_array
    monkeypatch.setattr(imageoperations, "as_array", lambda obj: calls.append(type(obj).__name__) or real(obj))
    ex = RadiomicsFeatureExtractor({"setting": {"binWidth": 25, "resegmentRange": [-1.25, 1.5], "resegmentMode": "sigma"}})
    ex.execute(*_case(), label=A)
    assert calls == []
    ex = RadiomicsFeatureExtractor({"setting": {"binWidth": 25, "resegmentRange": [-1.25, 1.5], "resegmentMode": "sigma",
                                                "deviceResident": False}})
    ex.execute(*_case(), label=A)
    assert len(calls) == 2          # (the host route still does: image and mask)


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, (float, np.floating, np.ndarray)):
            x, y = float(x), float(y)
            assert x == y or (np.isnan(x) and np.isnan(y)), k
        else:
            assert x == y, k


def test_execute_labels_shares_the_filter_stack_under_resegmentation():
    from pyradiomics_amd import _lib
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    lib = _lib.load()
    params = {"setting": {"binWidth": 25, "resegmentRange": [-1.5, 1.5], "resegmentMode": "sigma"},
              "imageType": {"Original": {}, "Wavelet": {}}}
    ex = RadiomicsFeatureExtractor(params)
    lib.prad_timing_begin()
    try:
        one = ex.execute(*_case(), label=A)
        swt_one, reseg_one = lib.prad_timing_count(b"swt"), lib.prad_timing_count(b"resegment")
    finally:
        lib.prad_timing_end()
    for batched in (False, True):
        lib.prad_timing_begin()
        try:
            got = list(ex.executeLabels(*_case(), labels=[A, B, C_], batched=batched))
            swt_all, reseg_all = lib.prad_timing_count(b"swt"), lib.prad_timing_count(b"resegment")
        finally:
            lib.prad_timing_end()
        assert swt_one >= 1 and swt_all == swt_one          # eight bands once, not once per label
        assert reseg_one == 1 and reseg_all == 3
        assert [l for l, _ in got] == [A, B, C_]
        # batched=True is not wired to resegment_batch: with resegmentRange every label takes the per-label steps
        assert ex.lastLabelsRoute() == {"batched": [], "single": [A, B, C_], "mixed": []}
        _same(got[0][1], one)
        for l, res in got[1:]:
            _same(res, ex.execute(*_case(), label=l))

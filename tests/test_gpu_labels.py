"""Multi-label extraction on the GPU: the label census kernel (engine.label_census and the host-pointer ABI call) against a
brute-force census on the shapes that reach each of its paths, and RadiomicsFeatureExtractor.executeLabels against per-label
execute() -- key for key, bit for bit -- on one small four-label case, shared path, fallbacks, errors and command line."""
import csv
import ctypes as C

import numpy as np
import pytest

from labels_cases import A, ABSENT, B, C_, D, assert_census, brute_census, census_cases, labels_case

pytestmark = pytest.mark.gpu

CASES = census_cases()
_CODE = {np.uint8: 4, np.int16: 3, np.int32: 2}
# words of 32 bits a workgroup's table may take in LDS (kernels_labels.h: PRAD_CENSUS_LDS_WORDS)
LDS_WORDS = 12288


def _dev(arr, dt):
    import torch
    return torch.from_numpy(arr.astype(dt)).to("cuda:0")


def _abi_census(arr, dt, max_label):
    from pyradiomics_amd import _lib
    a = np.ascontiguousarray(arr.astype(dt))
    size = np.array(a.shape, dtype=np.intc)
    table = np.full((max_label + 1, 1 + 2 * a.ndim), -12345, dtype=np.int64)
    rc = _lib.load().prad_label_census(C.c_void_p(a.ctypes.data), _CODE[dt], size.ctypes.data_as(C.POINTER(C.c_int)), a.ndim,
                                       int(max_label), C.c_void_p(table.ctypes.data))
    _lib.raise_for(rc, "label census")
    return table


def _from_table(table, nd):
    labels = np.flatnonzero(table[:, 0] > 0).astype(np.int64)
    return labels, table[labels, 0], table[labels, 1:1 + nd], table[labels, 1 + nd:]


@pytest.mark.parametrize("name,arr,dtypes", CASES, ids=[c[0] for c in CASES])
def test_census_equals_brute_force(name, arr, dtypes):
    from pyradiomics_amd import _lib, engine
    want = brute_census(arr)
    top = int(arr.max())
    tier = "census-lds" if (top + 1) * (1 + 2 * arr.ndim) <= LDS_WORDS else "census-global"
    for dt in dtypes:
        got = engine.label_census(_dev(arr, dt))
        assert_census(got, want, "%s %s engine" % (name, np.dtype(dt)))
        assert _lib.last_variant() == tier and _lib.last_path() == "label_census"
        table = _abi_census(arr, dt, top)
        assert_census(_from_table(table, arr.ndim), want, "%s %s abi" % (name, np.dtype(dt)))
        # row 0 stays zero; an absent label reads count 0, lo = size, hi = -1
        assert not table[0].any()
        absent = np.setdiff1d(np.arange(1, top + 1), want[0])
        if len(absent):
            assert not table[absent, 0].any()
            assert np.array_equal(table[absent, 1:1 + arr.ndim], np.broadcast_to(arr.shape, (len(absent), arr.ndim)))
            assert (table[absent, 1 + arr.ndim:] == -1).all()
    if name == "background_3x4x8":
        assert len(want[0]) == 0


def test_census_tiers():
    """which table serves which label range: the 512-label map and {1, 255} fit the workgroup's LDS, {3, 1000, 65535} does not;
    the same 512 one-voxel labels with a table sized for 4096 go through the global tier label by label"""
    from pyradiomics_amd import _lib, engine
    by_name = {c[0]: c[1] for c in CASES}
    engine.label_census(_dev(by_name["distinct_4x8x16"], np.int16))
    assert 513 * 7 <= LDS_WORDS and _lib.last_variant() == "census-lds"
    engine.label_census(_dev(by_name["u8_extremes_4x6x20"], np.uint8))
    assert _lib.last_variant() == "census-lds"
    engine.label_census(_dev(by_name["sparse_4x6x20"], np.int32))
    assert 65536 * 7 > LDS_WORDS and _lib.last_variant() == "census-global"
    arr = by_name["distinct_4x8x16"]
    for dt in (np.int16, np.int32):
        got = engine.label_census(_dev(arr, dt), max_label=4096)
        assert 4097 * 7 > LDS_WORDS and _lib.last_variant() == "census-global"
        assert_census(got, brute_census(arr), "distinct, global tier")
    # the unaligned / odd-row path (one voxel per lane) next to the aligned one (four per lane), both tiers
    import torch
    arr = by_name["row_3x5x130"]
    wide = np.zeros((3, 5, 132), np.int64)
    wide[:, :, :130] = arr
    for m in (None, 4096):
        assert_census(engine.label_census(_dev(wide, np.int16), max_label=m), brute_census(wide), "aligned rows")
        shifted = torch.zeros(wide.size + 1, dtype=torch.int16, device="cuda:0")[1:].view(3, 5, 132)     # 2-byte aligned base
        shifted.copy_(_dev(wide, np.int16))
        assert_census(engine.label_census(shifted, max_label=m), brute_census(wide), "unaligned base")


def test_census_many_rounds_per_wave():
    """maps large enough that a wave works through several rounds of loads (more than 4 items per wave at the capped grid)
    and rows of more than one item: the register run survives from round to round and from row to row, and the item
    coordinates are carried on.  Four voxels per lane (nx = 520, three items per row) and one per lane (nx = 521, nine)."""
    import torch
    from pyradiomics_amd import _lib, engine
    for shape in ((48, 256, 520), (40, 128, 521)):
        arr = np.zeros(shape, np.int64)
        arr[2:30, 10:100, 0:shape[2]] = 1                    # whole rows: one run over many rows and rounds
        arr[5:44, 101:128, 250:519] = 2                      # starts and ends inside items, crosses both item seams
        arr[31:40, 3:90, 255:258] = 3                        # three voxels around the first seam
        arr[shape[0] - 1, 127, shape[2] - 1] = 7             # the last voxel of a row
        arr[0, 0, 0] = 9
        arr[20, 50, 100:300:2] = 11                          # alternating with label 1 inside its block
        want = brute_census(arr)
        items = shape[0] * shape[1] * (-(-shape[2] // (256 if shape[2] % 4 == 0 else 64)))
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert items > cus * 4 * 8 * 4, "the map no longer reaches a second round of loads on this device"
        for dt in (np.uint8, np.int16, np.int32):
            for m, tier in ((None, "census-lds"), (4096, "census-global")):
                got = engine.label_census(_dev(arr, dt), max_label=m)
                assert _lib.last_variant() == tier
                assert_census(got, want, "%s %s %s" % (shape, np.dtype(dt), tier))


def test_label_census_route_errors_and_fallback():
    """imageoperations.labelCensus: a label above 65535 goes to the host census (the only failure that does); an int64 tensor
    whose values do not fit 32 bits is refused instead of wrapping into the label range"""
    import torch
    from pyradiomics_amd import engine, imageoperations as io
    from pyradiomics_amd.image import Image
    arr = np.zeros((3, 4, 8), np.int32)
    arr[1, 1:3, 2:6] = 5
    arr[2, 3, 7] = 70000
    assert_census(io.labelCensus(Image(arr), deviceResident=True), brute_census(arr), "host route behind the device's refusal")
    big = torch.zeros((2, 4, 8), dtype=torch.int64, device="cuda:0")
    big[0, 0, 0] = 2**32 + 3                                  # would read as label 3 after a plain narrowing
    big[1, 1, 1] = 4
    with pytest.raises(engine.LabelRangeError):
        engine.label_census(big)
    with pytest.raises(ValueError, match="integer label map"):
        engine.label_census(torch.zeros((2, 4, 8), device="cuda:0"))
    small = torch.zeros((2, 4, 8), dtype=torch.int64, device="cuda:0")
    small[1, 1, 1:4] = 4
    got = engine.label_census(small)
    assert list(got[0]) == [4] and list(got[1]) == [3]


def test_census_ignores_values_outside_the_table_and_writes_nothing_beyond_it():
    import torch
    from pyradiomics_amd import _lib
    arr = np.zeros((4, 6, 20), np.int64)
    arr[0, 0:3, 0:5] = -1
    arr[1, 1:4, 2:9] = 2
    arr[2, 2:6, 3:20] = 5
    arr[3, :, :] = 6                       # max_label + 1: whole rows of it (the uniform-wave path) ...
    arr[1, 5, 19] = 6                      # ... and a single voxel (the per-lane path)
    M, guard = 5, 0x5A5A5A5A5A5A
    size = np.array(arr.shape, dtype=np.intc)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dt in (np.int16, np.int32):
        mask = _dev(arr, dt)
        table = torch.full((M + 3, 7), guard, dtype=torch.int64, device="cuda:0")       # a guard row on each side
        rc = _lib.load().prad_label_census_dev(C.c_void_p(mask.data_ptr()), _CODE[dt], size.ctypes.data_as(C.POINTER(C.c_int)), 3,
                                               M, C.c_void_p(table[1:].data_ptr()), stream)
        _lib.raise_for(rc, "label census")
        assert _lib.last_variant() == "census-lds"
        t = table.cpu().numpy()
        assert (t[0] == guard).all() and (t[-1] == guard).all()
        assert_census(_from_table(t[1:-1], 3), brute_census(arr, M), "guarded table")
    # the global tier with the same out-of-range values: max_label + 1 = 4097 next to valid labels
    arr2 = arr.copy()
    arr2[arr2 == 6] = 4097
    mask = _dev(arr2, np.int32)
    table = torch.full((4096 + 3, 7), guard, dtype=torch.int64, device="cuda:0")
    rc = _lib.load().prad_label_census_dev(C.c_void_p(mask.data_ptr()), 2, size.ctypes.data_as(C.POINTER(C.c_int)), 3, 4096,
                                           C.c_void_p(table[1:].data_ptr()), stream)
    _lib.raise_for(rc, "label census")
    assert _lib.last_variant() == "census-global"
    t = table.cpu().numpy()
    assert (t[0] == guard).all() and (t[-1] == guard).all()
    assert_census(_from_table(t[1:-1], 3), brute_census(arr2, 4096), "guarded table, global tier")


def test_census_refuses_labels_beyond_65535():
    from pyradiomics_amd import _lib, engine
    arr = np.zeros((2, 4, 8), np.int32)
    arr[0, 0, 0] = 65536
    with pytest.raises(ValueError, match="max_label"):
        engine.label_census(_dev(arr, np.int32))
    with pytest.raises(ValueError, match="max_label"):
        engine.label_census(_dev(arr, np.int32), max_label=65536)
    table = np.zeros((1, 7), np.int64)
    size = np.array(arr.shape, dtype=np.intc)
    rc = _lib.load().prad_label_census(C.c_void_p(arr.ctypes.data), 2, size.ctypes.data_as(C.POINTER(C.c_int)), 3, 65536,
                                       C.c_void_p(table.ctypes.data))
    assert rc == _lib.PRAD_E_ARG
    got = engine.label_census(_dev(arr, np.int32), max_label=65535)        # the admissible limit ignores the value above it
    assert len(got[0]) == 0


# ---- executeLabels ---------------------------------------------------------------------------------------------------
PARAMS = {"setting": {"binWidth": 25}, "imageType": {"Original": {}, "Wavelet": {}, "LoG": {"sigma": [1.0]}}}


def _extractor(**settings):
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    p = {"setting": dict(PARAMS["setting"], **settings), "imageType": PARAMS["imageType"]}
    return RadiomicsFeatureExtractor(p)


def _images():
    from pyradiomics_amd.image import Image
    vol, lab = labels_case()
    return Image(vol), Image(lab)


@pytest.fixture(scope="module")
def per_label():
    """execute(label=l) for the three valid labels, computed once"""
    ex = _extractor()
    return {l: ex.execute(*_images(), label=l) for l in (A, B, C_)}


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, (float, np.floating, np.ndarray)):
            x, y = float(x), float(y)
            assert x == y or (np.isnan(x) and np.isnan(y)), k
        else:
            assert x == y, k


def test_execute_labels_equals_execute(per_label):
    ex = _extractor()
    got = dict(ex.executeLabels(*_images()))
    assert list(got) == [A, B, C_]
    for l in got:
        assert len(got[l]) > 900
        _same(got[l], per_label[l])
    ordered = list(ex.executeLabels(*_images(), labels=[B, A]))
    assert [l for l, _ in ordered] == [B, A]
    for l, res in ordered:
        _same(res, per_label[l])


def test_execute_labels_errors_leave_nothing_in_flight(per_label):
    ex = _extractor()
    with pytest.raises(ValueError) as single:
        ex.execute(*_images(), label=D)
    seen = []
    with pytest.raises(ValueError) as multi:
        for l, res in ex.executeLabels(*_images(), labels=[A, D]):
            seen.append(l)
            _same(res, per_label[A])
    assert seen == [A] and str(multi.value) == str(single.value)
    with pytest.raises(ValueError, match=r"Label \(9\) not present in mask"):
        list(ex.executeLabels(*_images(), labels=[ABSENT]))
    # a label that fails BEHIND one whose last image is still queued, then a fresh call on this thread
    with pytest.raises(ValueError):
        list(ex.executeLabels(*_images(), labels=[A, B, ABSENT, C_]))
    # a consumer that stops after the first result: label B's first image is queued behind it and has to be abandoned
    g = ex.executeLabels(*_images(), labels=[A, B, C_])
    assert next(g)[0] == A
    g.close()
    for l, res in ex.executeLabels(*_images()):
        _same(res, per_label[l])


def test_execute_labels_shares_census_and_filters():
    from pyradiomics_amd import _lib
    lib = _lib.load()
    ex = _extractor()
    ex.execute(*_images(), label=A)                     # (warm: workspaces, streams)
    lib.prad_timing_begin()
    try:
        ex.execute(*_images(), label=A)
        swt_one, census_one = lib.prad_timing_count(b"swt"), lib.prad_timing_count(b"label_census")
    finally:
        lib.prad_timing_end()
    lib.prad_timing_begin()
    try:
        n = len(list(ex.executeLabels(*_images(), labels=[A, B, C_])))
        swt_all, census_all = lib.prad_timing_count(b"swt"), lib.prad_timing_count(b"label_census")
    finally:
        lib.prad_timing_end()
    assert n == 3 and swt_one >= 1 and census_one == 0
    assert census_all == 1
    assert swt_all == swt_one


@pytest.mark.parametrize("extra", [{"preCrop": True}, {"resegmentRange": [-3, 3], "resegmentMode": "sigma"},
                                   {"deviceResident": False}], ids=["preCrop", "resegment", "host"])
def test_execute_labels_fallbacks_equal_execute(extra):
    ex = _extractor(**extra)
    got = list(ex.executeLabels(*_images(), labels=[A, B]))
    assert [l for l, _ in got] == [A, B]
    for l, res in got:
        _same(res, ex.execute(*_images(), label=l))


def test_cli_all_labels(tmp_path):
    from pyradiomics_amd import scripts
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image, write_nrrd
    vol, lab = labels_case()
    ip, mp = str(tmp_path / "img.nrrd"), str(tmp_path / "lab.nrrd")
    write_nrrd(ip, Image(vol, (1.0, 1.0, 2.0)))
    write_nrrd(mp, Image(lab, (1.0, 1.0, 2.0)))
    out = tmp_path / "out.csv"
    assert scripts.main([ip, mp, "-s", "binWidth:25", "--all-labels", "-f", "csv", "-o", str(out)]) == 0
    rows = list(csv.DictReader(open(out)))
    assert [r["Label"] for r in rows] == [str(A), str(B), str(C_)]
    ex = RadiomicsFeatureExtractor(binWidth=25.0)
    for r in rows:
        want = ex.execute(ip, mp, label=int(r["Label"]))
        feats = [k for k in want if not k.startswith("diagnostics_")]
        assert len(feats) > 90
        for k in feats:
            x, y = float(r[k]), float(want[k])
            assert x == y or (np.isnan(x) and np.isnan(y)), k

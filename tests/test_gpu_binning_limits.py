"""GPU: the binning kernels (csrc/kernels_binning.h: roi_minmax_kernel, digitize_kernel, bincount_edges_kernel,
level_counts_kernel) and their host side (csrc/prad_binning.hip) at the limits of their routes, against
tests/binning_reference.py (exact; pinned by tests/test_binning_reference.py).  Discretisation is exact arithmetic, so every
assertion is an equality: levels over the whole array (0 outside the ROI), Ng, the edges bit for bit, the level census
(counts[0] == 0, sum == ROI size), on engine.bin_image with and without counts, engine.level_counts, the ticket pair
engine.bin_image_enqueue / bin_image_collect and prad_roi_minmax_dev.

Sizes.  The scans deal 16-byte vectors (E = 16 / sizeof(T) elements) to nthreads = 256 * min(ceil(n / 256), cap) threads, cap =
1024 (digitize, level counts) or 512 (min / max).  Their four-deep loop `for (; v + 3 * nthreads < nvec; ...)` starts at nvec >
3 * cap * 256; n = E (3 * 262144 + 1000) + E - 1 -- 1 574 865 (float64), 3 149 731 (float32, int32), 6 299 463 (int16) -- is
where 1000 digitize threads run it, the others the one-vector loop, and E - 1 elements are left to the scalar tail; the min / max
kernel, with half the threads, runs the four-deep loop in every thread there.  n = 5003 is below every cap.

Tiers.  The thresholds come from the expressions of launch_digitize and prad_level_counts_dev quoted in SOURCE_QUOTES;
test_thresholds_follow_the_source fails when the source no longer holds them.

Out of scope: NaN and infinite voxels (the reference has no defined answer for them).
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import binning_reference as br

pytestmark = pytest.mark.gpu

# expression in the source -> the largest nedges (Ng for the last) it admits
SOURCE_QUOTES = {
    "nedges <= 48": 48,                                                          # a count table per thread
    "edge_b + cnt_b <= 64 * 1024": (64 * 1024 - 16) // (8 + 16),                 # 8 nedges + 16 (nedges + 1): per-wave LDS tables
    "edge_b <= 60 * 1024": 60 * 1024 // 8,                                       # the edges in LDS
    "4 * nb * sizeof(unsigned) <= 48 * 1024": 48 * 1024 // 16 - 1,               # level_counts_kernel: 16 (Ng + 1)
}
SOURCE_DEFINITIONS = ("edge_b = sizeof(double) * (size_t)nedges", "cnt_b = 4 * sizeof(unsigned) * ((size_t)nedges + 1)",
                      "nb = (size_t)Ng + 1", ": 1024;", ": 512;")
LEVEL_COUNTS_NG = (3071, 3072)
SMALL_N = 5003


def test_thresholds_follow_the_source():
    import pyradiomics_amd
    path = os.path.join(os.path.dirname(pyradiomics_amd.__file__), "csrc", "prad_binning.hip")
    with open(path) as f:
        src = f.read()
    for quote in tuple(SOURCE_QUOTES) + SOURCE_DEFINITIONS:
        assert quote in src, quote
    t = list(SOURCE_QUOTES.values())
    assert br.TIER_EDGES == (t[0], t[0] + 1, t[1], t[1] + 1, t[2], t[2] + 1) == (48, 49, 2730, 2731, 7680, 7681)
    assert br.TIER_COUNTS == (t[0] - 1, t[0], t[1] - 1, t[1]) and LEVEL_COUNTS_NG == (t[3], t[3] + 1)
    assert (br.DIGITIZE_CAP, br.MINMAX_CAP, br.BLOCK) == (1024, 512, 256)


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poison(like):
    """bin_image allocates its level tensor uninitialised; the block it gets is most likely the one freed last, so leave
    a block of that size full of a value no level has: a vector the kernel skips is then seen, not papered over"""
    import torch
    t = torch.full(tuple(like.shape), -7, dtype=torch.int32, device=like.device)
    torch.cuda.synchronize()
    del t


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_result(out, want, mask, label, with_counts):
    levels, Ng, edges, counts = want
    got = out[0].cpu().numpy()
    assert got.dtype == np.int32 and got.shape == levels.shape, label
    assert np.array_equal(got, levels), (label, "levels", int((got != levels).sum()), np.flatnonzero((got != levels).ravel())[:8])
    assert out[1] == Ng, (label, "Ng", out[1], Ng)
    assert _same_bits(out[2], edges), (label, "edges")
    if with_counts:
        assert out[3].dtype == np.int64 and np.array_equal(out[3], counts), (label, "counts")
        assert out[3][0] == 0 and int(out[3].sum()) == int(np.asarray(mask).sum()), (label, "census")


def _check(x, mask, kw, X=None, M=None, want=None, label=None, census=True):
    """bin_image with and without counts and level_counts on (x, mask) against the reference; returns (want, levels tensor)"""
    from pyradiomics_amd import engine
    want = br.expected(x, mask, kw) if want is None else want
    X = _cuda(x) if X is None else X
    M = _cuda(mask) if M is None else M
    out = None
    for with_counts in (True, False):
        _poison(X)
        out = engine.bin_image(X, M, with_counts=with_counts, **kw)
        assert len(out) == (4 if with_counts else 3)
        _assert_result(out, want, mask, (label, kw, with_counts), with_counts)
    if census:
        assert np.array_equal(engine.level_counts(out[0], M, want[1]), want[3]), (label, "level_counts")
    return want, out[0]


def _minmax_dev(X, M):
    from pyradiomics_amd import _lib, engine
    lib = _lib.load()
    lib.prad_set_device(X.device.index or 0)
    mm = (C.c_double * 2)()
    rc = lib.prad_roi_minmax_dev(C.c_void_p(X.data_ptr()), engine._DTYPE_CODES[X.dtype], C.c_void_p(M.data_ptr()), X.numel(), mm,
                                 engine._stream_ptr())
    _lib.raise_for(rc, "roi_minmax")
    return float(mm[0]), float(mm[1])


def _bits(v):
    return struct.pack("<d", v)


_scan = {}


def _scan_tensors(dtype):
    """(case, image tensor, mask tensor, reference) of the large flat array of a type, built once"""
    if dtype not in _scan:
        c = br.scan_case(dtype)
        _scan[dtype] = (c, _cuda(c["x"]), _cuda(c["mask"]), br.expected(c["x"], c["mask"], c["kw"]))
    return _scan[dtype]


# ---- scan paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", br.DTYPES)
def test_scan_paths_levels_and_census(dtype):
    """four-deep loop, one-vector loop and scalar tail in one launch: fixed width (two calls) and fixed count (one call)"""
    c, X, M, want = _scan_tensors(dtype)
    assert X.numel() == br.scan_n(dtype) and X.data_ptr() % 16 == 0 and M.data_ptr() % 16 == 0
    _check(c["x"], c["mask"], c["kw"], X, M, want, label=dtype)
    _check(c["x"], c["mask"], dict(binCount=64), X, M, label=dtype)


@pytest.mark.parametrize("dtype", br.DTYPES)
def test_scan_paths_image_off_alignment_at_the_large_size(dtype):
    """the scalar fallback over a grid at its cap: the levels and counts of the aligned copy"""
    import torch
    c, X, M, want = _scan_tensors(dtype)
    buf = torch.empty(X.numel() + 1, dtype=X.dtype, device=X.device)
    buf[1:].copy_(X)
    assert buf[1:].data_ptr() % 16 != 0 and buf[1:].is_contiguous()
    _check(c["x"], c["mask"], c["kw"], buf[1:], M, want, label=dtype)


@pytest.mark.parametrize("dtype", br.DTYPES)
def test_scan_paths_extremes_planted_in_one_place(dtype):
    """the unique minimum, then the unique maximum, in exactly one of: element 0, the last lane of the fourth load of the
    four-deep loop (of digitize_kernel's grid and of roi_minmax_kernel's), a vector of the one-vector loop, the scalar tail"""
    c, X, M, _ = _scan_tensors(dtype)
    pos = br.scan_positions(dtype)
    mask = c["mask"].copy()
    mask[list(pos.values())] = True
    M2 = _cuda(mask)
    X2 = X.clone()
    lo, hi = br.minmax_exact(c["x"], mask)
    assert _minmax_dev(X2, M2) == (lo, hi)
    big = 30000 if np.dtype(dtype).kind == "i" else 30000.5
    assert -big < lo and hi < big
    for name, p in pos.items():
        keep = X2[p].clone()
        X2[p] = big
        assert _minmax_dev(X2, M2) == (lo, float(big)), (dtype, name, "max")
        X2[p] = -big
        assert _minmax_dev(X2, M2) == (float(-big), hi), (dtype, name, "min")
        X2[p] = keep
    # through the one-call route: the maximum only in the scalar tail, the minimum only in the four-deep loop
    x = c["x"].copy()
    x[pos["tail"]], x[pos["digitize-fourth-load"]] = big, -big
    X2[pos["tail"]], X2[pos["digitize-fourth-load"]] = big, -big
    _check(x, mask, dict(binCount=16), X2, M2, label=dtype, census=False)
    # ... and outside the ROI they count for nothing
    mask[pos["tail"]] = mask[pos["digitize-fourth-load"]] = False
    assert _minmax_dev(X2, _cuda(mask)) == br.minmax_exact(x, mask)


@pytest.mark.parametrize("off", ["image", "mask", "both"])
@pytest.mark.parametrize("dtype", br.DTYPES)
def test_views_off_alignment_below_the_caps(dtype, off):
    """n = 5003: the image one element off a 16-byte boundary, the mask one byte off, both"""
    import torch
    c = br.scan_case(dtype, SMALL_N)
    x, mask = c["x"], c["mask"]
    X, M = _cuda(x), _cuda(mask)
    if off in ("image", "both"):
        buf = torch.empty(SMALL_N + 1, dtype=X.dtype, device=M.device)
        buf[1:].copy_(X)
        X = buf[1:]
        assert X.data_ptr() % 16 == X.element_size()
    if off in ("mask", "both"):
        buf8 = torch.empty(SMALL_N + 1, dtype=torch.uint8, device=M.device)
        buf8[1:].copy_(M)
        M = buf8[1:]
        assert M.data_ptr() % 16 == 1
    want, _ = _check(x, mask, c["kw"], X, M, label=(dtype, off))
    _check(x, mask, dict(binCount=32), X, M, label=(dtype, off))
    aligned = _check(x, mask, c["kw"], label=(dtype, "aligned"))[0]
    assert all(np.array_equal(a, b) for a, b in zip(want, aligned))
    assert _minmax_dev(X, M) == br.minmax_exact(x, mask)


@pytest.mark.parametrize("dtype", br.DTYPES)
def test_one_voxel_rois_and_an_empty_roi(dtype):
    from pyradiomics_amd import engine
    c = br.scan_case(dtype, SMALL_N)
    x = c["x"]
    X = _cuda(x)
    for index in (0, SMALL_N - 1):
        mask = np.zeros(SMALL_N, dtype=bool)
        mask[index] = True
        M = _cuda(mask)
        want, _ = _check(x, mask, dict(binWidth=25), X, M, label=(dtype, index))
        assert want[1] == 1 and want[3].tolist() == [0, 1]
        assert _minmax_dev(X, M) == (float(x[index]), float(x[index]))
        # fixed count on one voxel: a constant ROI, np.histogram widens the range (host-built edges)
        edges = np.asarray(br.constant_count_edges(x[index], 8, x.dtype), dtype=np.float64)
        levels = br.levels_exact(x, mask, edges)
        Ng = int(levels.max())
        _check(x, mask, dict(binCount=8), X, M, want=(levels, Ng, edges, br.counts_exact(levels, mask, Ng + 1)), label=(dtype, index))
    empty = _cuda(np.zeros(SMALL_N, dtype=bool))
    for kw in (dict(binWidth=25), dict(binCount=8), dict(binCount=5000)):
        with pytest.raises(ValueError, match="empty ROI"):
            engine.bin_image(X, empty, with_counts=True, **kw)
    assert engine.bin_image_collect(engine.bin_image_enqueue(X, _cuda(np.ones(SMALL_N, dtype=bool)), binCount=8))[1] >= 1
    with pytest.raises(ValueError, match="empty ROI"):
        engine.bin_image_collect(engine.bin_image_enqueue(X, empty, binCount=8))


# ---- tiers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int16", "int32"])
@pytest.mark.parametrize("nedges", br.TIER_EDGES)
def test_digitize_tiers_fixed_width(nedges, dtype):
    c = br.tier_case(nedges, dtype)
    want, _ = _check(c["x"], c["mask"], c["kw"], label=(nedges, dtype))
    assert len(want[2]) == nedges and want[1] == nedges - 1 and want[3][1:].min() >= 1          # every level occupied


@pytest.mark.parametrize("dtype", ["int32", "float32"])
@pytest.mark.parametrize("count", br.TIER_COUNTS)
def test_digitize_tiers_fixed_count(count, dtype):
    c = br.tier_case(count + 1, dtype, count=count)
    want, _ = _check(c["x"], c["mask"], c["kw"], label=(count, dtype))
    assert len(want[2]) == count + 1 and want[1] == count and want[3][1:].min() >= 1


@pytest.mark.parametrize("n", [SMALL_N, br.scan_n("int32")])
@pytest.mark.parametrize("Ng", LEVEL_COUNTS_NG)
def test_level_counts_tiers_and_foreign_levels(Ng, n):
    """LDS tables up to Ng = 3071, global atomics from 3072; levels of 0, below 0 and above Ng under the mask land in [0];
    a view off alignment gives the same"""
    import torch
    from pyradiomics_amd import engine
    rng = np.random.default_rng(Ng + n % 7)
    levels = rng.integers(1, Ng + 1, size=n).astype(np.int32)
    levels[:Ng] = np.arange(1, Ng + 1)
    foreign = rng.random(n) < 0.01
    foreign[:Ng] = False
    levels[foreign] = rng.choice(np.array([0, -1, -2 ** 31, Ng + 1, Ng + 2, 2 ** 31 - 1], dtype=np.int64), size=int(foreign.sum()))
    mask = rng.random(n) < 0.8
    mask[:Ng] = True
    want = np.bincount(np.where((levels >= 1) & (levels <= Ng), levels, 0)[mask], minlength=Ng + 1).astype(np.int64)
    assert want[0] == int((foreign & mask).sum()) > 0 and want[1:].min() >= 1 and want.sum() == mask.sum()
    L, M = _cuda(levels), _cuda(mask)
    got = engine.level_counts(L, M, Ng)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    bufl = torch.empty(n + 1, dtype=torch.int32, device=M.device)
    bufl[1:].copy_(L)
    bufm = torch.empty(n + 1, dtype=torch.uint8, device=M.device)
    bufm[1:].copy_(M)
    assert bufl[1:].data_ptr() % 16 == 4 and bufm[1:].data_ptr() % 4 == 1
    assert np.array_equal(engine.level_counts(bufl[1:], M, Ng), want)
    assert np.array_equal(engine.level_counts(L, bufm[1:], Ng), want)
    assert np.array_equal(engine.level_counts(bufl[1:], bufm[1:], Ng), want)


# ---- values -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.VALUES + br.COUNTS)
def test_adversarial_values(name):
    c = br.case(name)
    want, _ = _check(c["x"], c["mask"], c["kw"], label=name)
    if "Ng" in c:
        assert want[1] == c["Ng"]
    if "nedges" in c:
        assert len(want[2]) == c["nedges"]


@pytest.mark.parametrize("name", br.RAISING)
def test_ranges_without_edges_raise_the_host_routes_error(name):
    from pyradiomics_amd import engine, imageoperations
    c = br.case(name)
    with pytest.raises(ValueError, match="Too many bins") as host:
        with np.errstate(all="ignore"):
            imageoperations.binImage(c["x"], c["mask"], **c["kw"])
    for with_counts in (False, True):
        with pytest.raises(ValueError) as dev, np.errstate(all="ignore"):
            engine.bin_image(_cuda(c["x"]), _cuda(c["mask"]), with_counts=with_counts, **c["kw"])
        assert str(dev.value) == str(host.value)


@pytest.mark.parametrize("name", br.DUPLICATE)
def test_edges_that_are_not_strictly_ascending_follow_the_host_route(name):
    """64 ulps cut into 4096 bins: linspace's edges repeat.  NumPy >= 2.1 raises for them -- then so does the device route, with
    the same error; a NumPy that answers gets the levels of those edges"""
    from pyradiomics_amd import engine, imageoperations
    c = br.case(name)
    try:
        imageoperations.binImage(c["x"], c["mask"], **c["kw"])
    except ValueError as e:
        for with_counts in (False, True):
            with pytest.raises(ValueError) as dev:
                engine.bin_image(_cuda(c["x"]), _cuda(c["mask"]), with_counts=with_counts, **c["kw"])
            assert str(dev.value) == str(e)
        return
    _check(c["x"], c["mask"], c["kw"], label=name)


def test_signed_zeros_and_denormals_keep_their_bits_through_min_max():
    for dt in ("float64", "float32"):
        tiny = float(np.nextafter(np.dtype(dt).type(0), np.dtype(dt).type(1)))
        for values, roi in (([0.0, -0.0, 1.0], [1, 1, 0]), ([-0.0, -0.0, 1.0], [1, 1, 0]), ([0.0, 0.0, -1.0], [1, 1, 0]),
                            ([tiny, -tiny, 9.0], [1, 1, 0]), ([tiny, 2 * tiny, 0.0], [1, 1, 0]), ([-tiny, -0.0, 5.0], [1, 1, 0]),
                            ([0.0, tiny, -0.0, 3.0, -7.0], [1, 1, 1, 0, 0])):
            x, mask = np.array(values, dtype=dt), np.array(roi, dtype=bool)
            lo, hi = _minmax_dev(_cuda(x), _cuda(mask))
            wlo, whi = br.minmax_exact(x, mask)
            assert (_bits(lo), _bits(hi)) == (_bits(wlo), _bits(whi)), (dt, values, lo, hi)
    for dt in ("int16", "int32"):
        info = np.iinfo(dt)
        x, mask = np.array([info.min, info.max, 0, -1], dtype=dt), np.array([1, 1, 1, 0], dtype=bool)
        assert _minmax_dev(_cuda(x), _cuda(mask)) == (float(info.min), float(info.max))


# ---- tickets ----------------------------------------------------------------------------------------------------------------
def test_four_tickets_of_mixed_types_collected_in_reverse():
    from pyradiomics_amd import engine
    rng = np.random.default_rng(41)
    shape = (5, 11, 23)
    jobs = [((rng.standard_normal(shape) * 300).astype(np.int16), 16), ((rng.standard_normal(shape) * 1e6).astype(np.int32), 4096),
            (np.full(shape, 3.25, dtype=np.float32), 8), (rng.standard_normal(shape), 33)]
    mask = rng.random(shape) < 0.7
    mask[0, 0, 0] = True
    M = _cuda(mask)
    for round_ in range(2):                                        # after the four are collected, four more work
        tensors = [_cuda(x) for x, _ in jobs]
        tokens = [engine.bin_image_enqueue(X, M, binCount=N) for X, (_, N) in zip(tensors, jobs)]
        assert all(t is not None for t in tokens) and sorted(t["ticket"] for t in tokens) == [0, 1, 2, 3]
        assert engine.bin_image_enqueue(tensors[0], M, binCount=5) is None          # a fifth in flight
        for k in (3, 2, 1, 0):
            x, N = jobs[k]
            got = engine.bin_image_collect(tokens[k], with_counts=True)
            if k == 2:                                             # the constant ROI falls back inside collect
                edges = np.asarray(br.constant_count_edges(3.25, N, x.dtype), dtype=np.float64)
                levels = br.levels_exact(x, mask, edges)
                want = (levels, int(levels.max()), edges, br.counts_exact(levels, mask, int(levels.max()) + 1))
            else:
                want = br.expected(x, mask, dict(binCount=N))
            _assert_result(got, want, mask, (round_, k), True)
            direct = engine.bin_image(tensors[k], M, with_counts=True, binCount=N)
            assert np.array_equal(direct[0].cpu().numpy(), got[0].cpu().numpy()) and direct[1] == got[1]
            assert _same_bits(direct[2], got[2]) and np.array_equal(direct[3], got[3])


# ---- pixel types ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int8", "int64", "bool"])
def test_other_pixel_types_straight_into_bin_image(dtype):
    rng = np.random.default_rng(7)
    dt = np.dtype(dtype)
    n = 1001
    if dt.kind == "b":
        x = rng.random(n) < 0.5
    else:
        info = np.iinfo(dt)
        x = rng.integers(max(info.min, -40000), min(info.max, 70000), size=n, endpoint=True).astype(dt)
        x[:2] = max(info.min, -40000), min(info.max, 70000)
    mask = rng.random(n) < 0.8
    mask[:2] = True
    for kw in (dict(binWidth=25), dict(binWidth=1), dict(binCount=16)):
        _check(x, mask, kw, label=(dtype, kw))


@pytest.mark.parametrize("name", ["u8-range", "i16-saturated", "i16-lowest"])
def test_integer_images_near_the_ends_of_their_type_through_the_classes(name):
    """a first-order and a GLCM class on Image(uint8 with maximum 250) / a saturated int16 image: the host route and the device
    route see the same levels -- those of the reference -- and return the same values"""
    from pyradiomics_amd import backend, cmatrices, firstorder, glcm
    from pyradiomics_amd.image import Image
    backend.set(cmatrices)
    c = br.case(name)
    x = np.resize(c["x"], (4, 9, 11))
    if name == "i16-saturated":                       # (a narrow range below 32767: a GLCM of some thirty levels)
        x = np.random.default_rng(5).integers(32000, 32768, size=x.shape).astype(np.int16)
        x[1, 1, 1], x[1, 1, 2] = 32767, 32000
    mask = np.ones(x.shape, dtype=np.uint8)
    mask[0, 0, :3] = 0
    roi = mask == 1
    assert x[roi].max() == c["x"].max() and (name == "i16-saturated" or x[roi].min() == c["x"].min())
    levels, Ng, edges, counts = br.expected(x, roi, c["kw"])
    seen = {}
    for cls, names, extra in ((firstorder.RadiomicsFirstOrder, ("Entropy", "Uniformity", "Minimum", "Maximum", "Range", "Median"), {}),
                              (glcm.RadiomicsGLCM, None, dict(fusedSegment=False))):
        for resident in (True, False):
            fc = cls(Image(x.copy()), Image(mask.copy()), deviceResident=resident, **c["kw"], **extra)
            assert fc.deviceResident == resident
            if names is None:
                fc.enableAllFeatures()
            else:
                for f in names:
                    fc.enableFeatureByName(f)
            values = {k: float(v) for k, v in fc.execute().items()}
            assert fc.coefficients["Ng"] == Ng
            assert np.array_equal(fc.coefficients["grayLevels"], np.flatnonzero(counts))
            assert np.array_equal(fc.coefficients["levelCounts"], counts[counts > 0])
            seen[(cls.__name__, resident)] = values
        a, b = seen[(cls.__name__, True)], seen[(cls.__name__, False)]
        assert list(a) == list(b) and len(a) >= 6
        for k in a:
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (cls.__name__, k, a[k], b[k])
    assert seen[("RadiomicsFirstOrder", True)]["Minimum"] == float(x[roi].min())
    assert seen[("RadiomicsFirstOrder", True)]["Maximum"] == float(x[roi].max())

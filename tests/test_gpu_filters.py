"""GPU: wavelet / LoG kernels against the CPU restatement (oracle/filters_oracle.py; parity with PyWavelets / ITK
itself is pinned by tests/test_notebook_pin.py), plus properties that hold for any correct implementation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(6, 8, 10), (5, 7, 9), (16, 12, 20), (1, 16, 16)])
@pytest.mark.parametrize("wavelet", ["coif1", "haar", "db2"])
def test_wavelet_matches_restatement(shape, wavelet):
    from oracle import filters_oracle as fo
    from pyradiomics_amd import filters
    rng = np.random.default_rng(1)
    x = rng.integers(-500, 1500, size=shape).astype(np.int16)
    kw = dict(wavelet=wavelet)
    if shape[0] == 1:
        kw.update(force2D=True, force2Ddimension=0)
    got = {name: im.array for im, name, _ in filters.getWaveletImage(x, None, **kw)}
    axes = tuple(a for a in range(x.ndim - 1, -1, -1) if not (kw.get("force2D") and a == 0))
    ap, ret = fo.swt3(x, wavelet, axes=axes)
    want = {"wavelet-" + k: v for k, v in ret[0].items()}
    want["wavelet-" + "L" * len(axes)] = ap
    assert list(got) == list(want)                      # names AND yield order (LLH ... HHH, then LLL)
    # held to the long-double reference within the derived rounding bound of the float64 passes (tests/filters_reference.py:
    # 1.6e-11 for coif1 here, where 1e-10 was allowed)
    import filters_reference as fr
    assert fr.AVAILABLE, fr.SKIP_REASON
    lo, hi = fo.wavelet_filters(wavelet)
    ref_ap, ref_ret = fr.swt3(x, (lo, hi), axes=axes)
    ref = {"wavelet-" + k: v for k, v in ref_ret[0].items()}
    ref["wavelet-" + "L" * len(axes)] = ref_ap
    bound = fr.wavelet_bound(lo, hi, len(axes), float(np.abs(x.astype(np.float64)).max()))
    assert bound < 2e-11
    for k in want:
        assert got[k].dtype == np.float64 and got[k].shape == x.shape
        assert np.abs(got[k] - ref[k]).max() <= bound, (k, float(np.abs(got[k] - ref[k]).max()), bound)
        assert np.abs(want[k] - ref[k]).max() <= bound
    # energy identity of an orthogonal undecimated transform: sum of sub-band energies = 2^naxes * ||x||^2
    if all(s % 2 == 0 for s in np.array(shape)[list(axes)]):
        e = sum(float((v.astype(np.float64) ** 2).sum()) for v in got.values())
        assert abs(e / ((x.astype(np.float64) ** 2).sum() * 2 ** len(axes)) - 1) < 1e-9


def test_wavelet_two_levels():
    from oracle import filters_oracle as fo
    from pyradiomics_amd import filters
    x = np.random.default_rng(2).standard_normal((8, 10, 12))
    got = {n: im.array for im, n, _ in filters.getWaveletImage(x, None, level=2)}
    ap, ret = fo.swt3(x, "coif1", level=2)
    assert "wavelet2-HHL" in got and "wavelet-HHL" in got and "wavelet2-LLL" in got and len(got) == 15
    np.testing.assert_allclose(got["wavelet2-LLL"], ap, rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(got["wavelet2-LHL"], ret[1]["LHL"], rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (0.78125, 0.78125, 6.5), (0.5, 1.0, 2.0)])
@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_log_matches_restatement(spacing, sigma):
    from oracle import filters_oracle as fo
    from pyradiomics_amd import filters
    from pyradiomics_amd.image import Image
    rng = np.random.default_rng(3)
    x = rng.integers(0, 800, size=(12, 40, 36)).astype(np.int16)
    out = list(filters.getLoGImage(Image(x, spacing), None, sigma=[sigma]))
    want = fo.laplacian_recursive_gaussian(x, spacing, sigma)
    if not out:      # the reference skips sigmas that do not fit the image (imageoperations.py:823)
        assert not np.all(np.array(x.shape[::-1]) >= np.ceil(sigma / np.array(spacing)) + 1)
        return
    im, name, _ = out[0]
    assert name == "log-sigma-%s-mm-3D" % str(sigma).replace(".", "-") and im.array.dtype == np.float32
    assert np.array_equal(im.array, want)                    # float32 images, identical operation order: the same bits


def test_log_properties():
    from pyradiomics_amd import filters
    z, y, x = np.meshgrid(np.arange(24.0), np.arange(28.0), np.arange(32.0), indexing="ij")
    const = filters.laplacian_recursive_gaussian(np.full((8, 9, 10), 7.0), (1, 1, 1), 1.5)
    assert np.abs(const).max() < 1e-4
    quad = filters.laplacian_recursive_gaussian(0.5 * (x - 16) ** 2, (1, 1, 1), 2.0)      # Laplacian 1 -> sigma^2
    assert abs(quad[8:-8, 8:-8, 10:-10].mean() - 4.0) < 0.05
    lin = filters.laplacian_recursive_gaussian(3 * x + 2 * y - z, (1, 1, 1), 2.0)
    assert np.abs(lin[8:-8, 8:-8, 8:-8]).max() < 5e-2      # |ramp| ~ 100: the edge-replicating start decays inwards
    a = np.random.default_rng(0).standard_normal((16, 16, 16)).astype(np.float32)
    two = filters.laplacian_recursive_gaussian(2 * a, (1, 1, 1), 1.0)
    np.testing.assert_allclose(two, 2 * filters.laplacian_recursive_gaussian(a, (1, 1, 1), 1.0), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kw", [dict(binWidth=25), dict(binCount=16), dict(binWidth=0.37)])
@pytest.mark.parametrize("dtype", ["int16", "float32", "float64"])
def test_device_binning_equals_host(kw, dtype):
    """engine.bin_image (ROI min/max + digitize on the device) == imageoperations.binImage (numpy), level for level"""
    import torch
    from pyradiomics_amd import engine, imageoperations
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((9, 20, 33)) * 300).astype(dtype)
    if "binWidth" in kw and kw["binWidth"] < 1 and dtype == "int16":
        pytest.skip("fractional width on an integer image is not a reference use case")
    m = rng.random(x.shape) < 0.7
    want, edges = imageoperations.binImage(x, m, **kw)
    got, Ng, e2 = engine.bin_image(torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda(), **kw)
    assert np.array_equal(got.cpu().numpy(), want) and Ng == int(want[m].max())
    assert np.array_equal(np.asarray(edges, dtype=np.float64), e2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["few", "lds_counts_limit", "global_counts", "global_edges"])
def test_device_binning_counts_and_any_number_of_edges(case):
    """prad_digitize_counts_dev: levels and the ROI voxels per level from ONE pass, for every size class of the edge list --
    LDS edges + LDS counts (<= 2 700 edges), LDS edges + global counts (<= 7 680), edges searched in global memory beyond
    (binWidth 1 on a 0..30 000 int16 image: 30 000 edges raised NotImplementedError before round 3) -- against
    imageoperations.binImage + np.unique (the reference's own route, base.py:119-125)"""
    import torch
    from pyradiomics_amd import engine, imageoperations
    rng = np.random.default_rng(11)
    hi, kw = {"few": (800, dict(binWidth=25)), "lds_counts_limit": (2600, dict(binWidth=1)),
              "global_counts": (7000, dict(binWidth=1)), "global_edges": (30000, dict(binWidth=1))}[case]
    x = rng.integers(0, hi + 1, size=(24, 40, 64)).astype(np.int16)
    x.flat[0], x.flat[1] = 0, hi
    m = rng.random(x.shape) < 0.8
    m.flat[0] = m.flat[1] = True
    want, edges = imageoperations.binImage(x, m, **kw)
    got, Ng, e2, counts = engine.bin_image(torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda(), with_counts=True, **kw)
    assert np.array_equal(got.cpu().numpy(), want) and Ng == int(want[m].max())
    assert np.array_equal(np.asarray(edges, dtype=np.float64), e2)
    lv, n = np.unique(want[m], return_counts=True)
    ref = np.zeros(Ng + 1, dtype=np.int64)
    ref[lv] = n
    assert np.array_equal(counts, ref)
    assert np.array_equal(engine.level_counts(got, torch.from_numpy(m).cuda(), Ng), ref)
    # the plain entry point still answers without the census
    got2, Ng2, _ = engine.bin_image(torch.from_numpy(x).cuda(), torch.from_numpy(m).cuda(), **kw)
    assert Ng2 == Ng and torch.equal(got2, got)


def test_device_resident_filters_equal_host_route():
    import torch
    from pyradiomics_amd import engine, filters
    x = np.random.default_rng(6).integers(0, 900, size=(9, 14, 16)).astype(np.int16)
    host = {n: im.array for im, n, _ in filters.getWaveletImage(x, None)}
    dev = engine.wavelet_images(torch.from_numpy(x).cuda())
    assert list(dev) == list(host)
    for k in host:
        assert np.array_equal(dev[k].cpu().numpy(), host[k])
    a = engine.log_image(torch.from_numpy(x).cuda(), (1.0, 1.0, 2.5), 2.0).cpu().numpy()
    assert np.array_equal(a, filters.laplacian_recursive_gaussian(x, (1.0, 1.0, 2.5), 2.0))


@pytest.mark.gpu
def test_intensity_transform_image_types_follow_the_reference_formulas():
    """Square / SquareRoot / Logarithm / Exponential (imageoperations.py:973-1073) on the device against the
    reference's numpy expressions written out literally"""
    from pyradiomics_amd import filters
    from pyradiomics_amd.image import Image
    rng = np.random.default_rng(2)
    arr = rng.integers(-300, 1200, (6, 9, 11)).astype(np.int16)
    im = arr.astype("float64")
    want = {}
    want["square"] = ((1 / np.sqrt(np.max(np.abs(im)))) * im) ** 2
    t = im.copy(); c = np.max(np.abs(t)); t[t > 0] = np.sqrt(t[t > 0] * c); t[t < 0] = -np.sqrt(-t[t < 0] * c)
    want["squareroot"] = t
    t = im.copy(); top = np.max(np.abs(t)); t[t > 0] = np.log(t[t > 0] + 1); t[t < 0] = -np.log(-(t[t < 0] - 1))
    want["logarithm"] = t * (top / np.max(np.abs(t)))
    top = np.max(np.abs(im))
    want["exponential"] = np.exp((np.log(top) / top) * im)
    for fn in (filters.getSquareImage, filters.getSquareRootImage, filters.getLogarithmImage, filters.getExponentialImage):
        for dev in (True, False):
            (out, name, _kw), = list(fn(Image(arr), None, deviceResident=dev))
            np.testing.assert_allclose(out.array, want[name], rtol=1e-14, atol=1e-12, err_msg=name)
            assert out.on_device == dev


@pytest.mark.gpu
@pytest.mark.parametrize("interp", ["sitkBSpline", "sitkLinear", "sitkNearestNeighbor"])
@pytest.mark.parametrize("dtype", [np.int16, np.float64, np.float32])
def test_device_resampling_is_bit_identical_to_the_pinned_numpy_route(interp, dtype):
    """prad_resample_dev performs the arithmetic of imageoperations.resampleImage's numpy route (which the reference's
    `_resampling` golden vectors pin) in the same order: identical bits, short lines (exact mirror sums) included"""
    from pyradiomics_amd import imageoperations
    from pyradiomics_amd.image import Image
    rng = np.random.default_rng(9)
    for shape, spacing, new, pad in (((9, 40, 37), (0.8, 0.8, 5.0), [2, 2, 2], 5), ((30, 21, 64), (1.0, 1.0, 1.0), [1.5, 0.7, 0], 3),
                                     ((1, 33, 30), (0.5, 0.5, 1.0), [1.3, 1.3, 1.3], 4)):
        arr = (rng.standard_normal(shape) * 300 + 500).astype(dtype)
        msk = np.zeros(shape, dtype=np.int16)
        msk[shape[0] // 4: shape[0] // 4 + max(1, shape[0] // 2), 5:-6, 7:-5] = 1
        kw = dict(resampledPixelSpacing=new, interpolator=interp, padDistance=pad)
        hi, hm = imageoperations.resampleImage(Image(arr, spacing), Image(msk, spacing), **kw)
        di, dm = imageoperations.resampleImage(Image(arr, spacing), Image(msk, spacing), deviceResident=True, **kw)
        assert di.on_device and di.array.dtype == hi.array.dtype and di.array.shape == hi.array.shape
        assert np.array_equal(dm.array, hm.array) and np.allclose(di.origin, hi.origin) and di.spacing == hi.spacing
        # float32 and the (1, 33, 30) slab included: an axis of length 1 is not filtered at all (no pow()), and float32 is one
        # rounding of the same float64 value on both routes.  tests/test_gpu_resample_limits.py holds both routes to a
        # long-double reference on these shapes.
        assert np.array_equal(di.array, hi.array), (interp, shape, np.abs(di.array.astype(float) - hi.array).max())


@pytest.mark.gpu
def test_gradient_image_type():
    from pyradiomics_amd import filters
    from pyradiomics_amd.image import Image
    z, y, x = np.meshgrid(np.arange(5.0), np.arange(7.0), np.arange(9.0), indexing="ij")
    ramp = 2 * x - 3 * y + 0.5 * z                            # constant gradient (2, -3, 0.5) in index units
    for dev in (True, False):
        (g, name, _), = list(filters.getGradientImage(Image(ramp, (1.0, 1.0, 1.0)), None, deviceResident=dev))
        assert name == "gradient" and g.array.dtype == np.float32
        inner = g.array[1:-1, 1:-1, 1:-1]
        np.testing.assert_allclose(inner, np.sqrt(4 + 9 + 0.25), rtol=1e-6)
        assert g.array[0, 3, 4] == pytest.approx(np.sqrt(4 + 9 + 0.0625), rel=1e-6)      # replicated edge halves dz
        (gs, _, _), = list(filters.getGradientImage(Image(ramp, (2.0, 1.0, 1.0)), None, deviceResident=dev))
        np.testing.assert_allclose(gs.array[1:-1, 1:-1, 1:-1], np.sqrt(1 + 9 + 0.25), rtol=1e-6)   # x spacing 2 mm
    rng = np.random.default_rng(0)
    a = rng.standard_normal((4, 6, 8))
    (d1, _, _), = list(filters.getGradientImage(Image(a, (0.7, 1.1, 2.0)), None, deviceResident=True))
    (d2, _, _), = list(filters.getGradientImage(Image(a, (0.7, 1.1, 2.0)), None, deviceResident=False))
    np.testing.assert_allclose(d1.array, d2.array, rtol=1e-6)


def _filter_golden():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filters_golden.npz")
    if not os.path.exists(path):
        pytest.skip("optional volume-level pin: tests/golden/filters_golden.npz has not been generated "
                    "(tests/golden/make_filter_golden.py needs PyWavelets + SimpleITK, absent from this image)")
    return np.load(path)


def test_filters_match_wheel_golden():
    """HIP wavelet / LoG kernels against outputs of the wheels the reference calls (pywt.swtn, SimpleITK's
    LaplacianRecursiveGaussian) -- runs as soon as the golden file exists"""
    from pyradiomics_amd import filters
    from pyradiomics_amd.image import Image
    g = _filter_golden()
    for name in ("brain1", "seeded"):
        x, spacing = g[name + "__input"], tuple(g[name + "__spacing"])
        got = {n: im.array for im, n, _ in filters.getWaveletImage(Image(x, spacing), None, wavelet="coif1")}
        for band in ("LLH", "LHL", "LHH", "HLL", "HLH", "HHL", "HHH", "LLL"):
            want = g["%s__wavelet_coif1_level1_%s" % (name, band)]
            np.testing.assert_allclose(got["wavelet-" + band], want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
        for sigma in (1.0, 2.0, 3.0, 5.0):
            want = g["%s__log_sigma_%g" % (name, sigma)]
            out = list(filters.getLoGImage(Image(x, spacing), None, sigma=[sigma]))
            if out:
                assert np.abs(out[0][0].array - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "int16"])
def test_bspline_resample_device_route_clamps_to_the_original_pixel_type(dtype):
    """narrow unsigned images are widened for the upload; B-spline overshoot must still be clamped to the ORIGINAL
    range (ITK's CastPixelWithBoundsChecking), as the host route does"""
    from pyradiomics_amd import imageoperations
    from pyradiomics_amd.image import Image
    rng = np.random.default_rng(5)
    hi = np.iinfo(dtype).max
    a = np.where(rng.random((12, 14, 16)) < 0.5, np.iinfo(dtype).min, hi).astype(dtype)     # maximal ringing
    m = np.zeros(a.shape, np.uint8)
    m[2:10, 3:11, 3:13] = 1
    kw = dict(resampledPixelSpacing=[0.7, 0.7, 0.7], interpolator="sitkBSpline", padDistance=2)
    host_i, host_m = imageoperations.resampleImage(Image(a.copy()), Image(m.copy()), deviceResident=False, **kw)
    dev_i, dev_m = imageoperations.resampleImage(Image(a.copy()), Image(m.copy()), deviceResident=True, **kw)
    got = dev_i.array.astype(np.int64)
    assert got.min() >= np.iinfo(dtype).min and got.max() <= hi
    assert np.array_equal(got, host_i.array.astype(np.int64)) and np.array_equal(dev_m.array, host_m.array)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,spacing", [((70, 66, 130), (1.0, 1.0, 1.0)), ((9, 14, 16), (1.0, 1.0, 2.5)),
                                           ((37, 53, 70), (0.7, 0.9, 3.0)), ((5, 4, 9), (1.0, 1.0, 1.0)), ((40, 72), (1.0, 1.5))])
def test_log_of_several_sigmas_in_one_launch_sequence_equals_one_at_a_time(shape, spacing):
    """prad_log_multi_dev (blockIdx.y = sigma) leaves the bits of prad_log_dev per sigma; more than 8 sigmas are split
    (imageoperations.py:806-836 loops over the sigma list one filter run at a time)"""
    import torch
    from pyradiomics_amd import engine
    x = torch.from_numpy(np.random.default_rng(8).integers(-200, 1500, size=shape).astype(np.int16)).cuda()
    sig = [0.5, 1.0, 1.7, 2.0, 3.0, 4.0, 5.0, 6.5, 2.5, 1.0]
    many = engine.log_images(x, spacing, sig)
    assert len(many) == len(sig)
    for s, got in zip(sig, many):
        assert torch.equal(got, engine.log_image(x, spacing, s)), s


@pytest.mark.gpu
def test_bincount_edges_built_on_the_device_are_numpys(monkeypatch):
    """prad_bincount_dev (one host synchronisation: min / max -> np.linspace's arithmetic on the device -> levels + census)
    against the two-call route with numpy-built edges (np.histogram(x, N)[1], last edge + 1: imageoperations.py:122-126):
    edges bit for bit, levels, counts; constant ROIs go back to the host route"""
    import torch
    from pyradiomics_amd import engine, imageoperations
    rng = np.random.default_rng(17)
    for trial in range(40):
        shape = (int(rng.integers(3, 20)), int(rng.integers(3, 30)), int(rng.integers(4, 70)))
        scale = 10.0 ** rng.uniform(-6, 9)
        x = (rng.standard_normal(shape) * scale + rng.uniform(-1, 1) * scale * 3).astype(np.float64)
        if trial % 7 == 0:
            x = np.round(x)                      # integer-valued doubles: ties exactly on edges
        if trial % 4 == 1:
            x = x.astype(np.float32)             # numpy builds float32 edges for float32 data
        elif trial % 4 == 2:
            x = np.clip(np.round(x / scale * 300), -30000, 30000).astype(np.int16)
        elif trial % 4 == 3 and scale < 1e6:
            x = np.round(x).astype(np.int32)
        m = rng.random(shape) < 0.7
        m[0, 0, 0] = True
        N = int(rng.choice([1, 2, 7, 16, 32, 33, 47, 48, 64, 100, 255, 1000]))
        X, M = torch.from_numpy(x).cuda(), torch.from_numpy(m.astype(np.uint8)).cuda()
        monkeypatch.delenv("PRAD_BIN_TWO_CALLS", raising=False)
        lv, Ng, edges, cnt = engine.bin_image(X, M, with_counts=True, binCount=N)
        want_edges = np.asarray(imageoperations.getBinEdges(x[m], binCount=N), dtype=np.float64)
        assert np.array_equal(edges, want_edges), (trial, N)
        monkeypatch.setenv("PRAD_BIN_TWO_CALLS", "1")
        lv2, Ng2, edges2, cnt2 = engine.bin_image(X, M, with_counts=True, binCount=N)
        assert Ng == Ng2 and torch.equal(lv, lv2) and np.array_equal(cnt, cnt2) and np.array_equal(edges, edges2)
        want = np.zeros(shape, dtype=np.int64)
        want[m] = np.digitize(x[m], want_edges)
        assert np.array_equal(lv.cpu().numpy(), want)
    monkeypatch.delenv("PRAD_BIN_TWO_CALLS", raising=False)
    flat = torch.full((6, 8, 12), 3.25, dtype=torch.float64).cuda()
    ones = torch.ones((6, 8, 12), dtype=torch.uint8).cuda()
    lv, Ng, edges = engine.bin_image(flat, ones, binCount=8)        # np.histogram widens a constant range: host-built edges
    assert np.array_equal(edges, np.asarray(imageoperations.getBinEdges(np.full(5, 3.25), binCount=8), dtype=np.float64))
    assert int(lv.max()) == Ng


# ---- round 4: one pass kernel for every axis (rgauss_pass_kernel), the Laplacian sum as its own kernel, float64 filter ----
def _log_old_route(fn):
    """runs fn() with the reference kernel of the library: one lane per line, the causal recursion parked in a float64
    scratch image (rgauss_line_kernel) -- the plainest statement of ITK's FilterDataArray on the device"""
    import os
    os.environ["PRAD_LOG_OLDLINE"] = "1"
    try:
        return fn()
    finally:
        del os.environ["PRAD_LOG_OLDLINE"]


@pytest.mark.parametrize("shape,spacing", [((256, 64, 256), (1.0, 1.0, 1.0)),      # 256-sample lines on the contiguous and a strided axis
                                           ((37, 53, 70), (0.8, 1.1, 2.5)),       # nothing a multiple of 4: scalar tile moves, ragged chunks
                                           ((25, 256, 256), (0.78125, 0.78125, 6.5)),   # brain1's grid
                                           ((5, 4, 9), (1.0, 1.0, 1.0)), ((12, 20, 19), (1.0, 2.0, 0.5)),
                                           ((4, 4, 520), (1.0, 1.0, 1.0)), ((600, 8, 4), (1.0, 1.0, 1.0)),
                                           ((3 * 16 + 4, 70, 2 * 16 + 19), (1.0, 1.0, 1.0)), ((20, 5, 23), (1.0, 1.0, 1.0))])   # block-edge cases
def test_log_pass_kernel_equals_the_reference_kernel_bit_for_bit(shape, spacing):
    import torch
    from pyradiomics_amd import engine, _lib
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-300, 1500, size=shape).astype(np.int16)).cuda()
    sig = [1.0, 2.5, 4.0]
    new = [t.cpu().numpy() for t in engine.log_images(x, spacing, sig)]
    assert _lib.last_path() == "log"
    old = _log_old_route(lambda: [t.cpu().numpy() for t in engine.log_images(x, spacing, sig)])
    assert _lib.last_path() == "log-reference"
    for a, b in zip(new, old):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    one = engine.log_image(x, spacing, 2.5).cpu().numpy()
    assert np.array_equal(one, new[1])


@pytest.mark.parametrize("shape,spacing", [((12, 40, 36), (1.0, 1.0, 1.0)), ((25, 64, 72), (0.78125, 0.78125, 6.5)),
                                           ((7, 9, 530), (1.0, 1.0, 1.0))])
@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_log_float64_matches_restatement(shape, spacing, sigma):
    """A float64 image (e.g. after `normalize: true`) comes back as float64 (sitk keeps the input's pixel type,
    imageoperations.py:824-830) but is filtered the way ITK does it: the derivative pass reads the float64 input itself,
    every image between the passes and the cumulative image are float (InternalRealType = float,
    itkLaplacianRecursiveGaussianImageFilter.h) -- ADVICE r4 medium; rounds 3-4 kept float64 images between the passes."""
    import torch
    from oracle import filters_oracle as fo
    from pyradiomics_amd import engine, filters
    from pyradiomics_amd.image import Image
    rng = np.random.default_rng(9)
    x = rng.standard_normal(shape) * 100.0
    want = fo.laplacian_recursive_gaussian(x, spacing, sigma)
    assert want.dtype == np.float64 and np.array_equal(want, want.astype(np.float32))
    got = engine.log_image(torch.from_numpy(x).cuda(), spacing, sigma).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, got.astype(np.float32))      # float32 values in a float64 image
    assert np.array_equal(got, want)
    host = filters.laplacian_recursive_gaussian(x, spacing, sigma)
    assert host.dtype == np.float64 and np.array_equal(host, got)
    multi = engine.log_images(torch.from_numpy(x).cuda(), spacing, [sigma, 2.0])
    assert np.array_equal(multi[0].cpu().numpy(), got)
    old = _log_old_route(lambda: engine.log_image(torch.from_numpy(x).cuda(), spacing, sigma).cpu().numpy())
    assert np.array_equal(old, got)                                   # reference kernel: the same bits
    # the first pass reads the float64 samples, not their float32 roundings: the two differ somewhere
    f32 = engine.log_image(torch.from_numpy(x.astype(np.float32)).cuda(), spacing, sigma).cpu().numpy()
    assert f32.dtype == np.float32 and np.any(f32.astype(np.float64) != got)
    for on_dev in (True, False):
        out = list(filters.getLoGImage(Image(x, spacing), None, sigma=[sigma], deviceResident=on_dev))
        if out:
            assert out[0][0].array.dtype == np.float64 and np.array_equal(out[0][0].array, got)


def test_log_after_normalize_is_float64_through_the_extractor():
    """normalize + LoG, the common MR recipe: normalizeImage returns float64, so must the LoG image"""
    import os
    from helpers import GOLDEN
    from pyradiomics_amd import filters, imageoperations
    from pyradiomics_amd.image import read_nrrd
    from oracle import filters_oracle as fo
    image = read_nrrd(os.path.join(GOLDEN, "data", "brain1_image.nrrd"))
    norm = imageoperations.normalizeImage(image, normalizeScale=100)
    assert norm.array.dtype == np.float64
    (derived, name, _), = list(filters.getLoGImage(norm, None, sigma=[3.0]))
    assert derived.array.dtype == np.float64 and name == "log-sigma-3-0-mm-3D"
    want = fo.laplacian_recursive_gaussian(norm.array, image.GetSpacing(), 3.0)
    assert np.array_equal(derived.array, want)


@pytest.mark.parametrize("shape", [(64, 64, 64), (18, 40, 44), (6, 8, 10), (70, 12, 130), (8, 6, 34)])
@pytest.mark.parametrize("wavelet", ["coif1", "db2", "haar"])
def test_fused_swt_kernel_equals_the_axis_passes_bit_for_bit(shape, wavelet, monkeypatch):
    """the 3-D transform as one kernel (x pass through LDS, y pass per lane, z pass from a register ring) against the three
    separate axis passes: the same float64 bits in all eight sub-bands, ragged tiles and short axes included"""
    import torch
    from pyradiomics_amd import engine, _lib
    from pyradiomics_amd.filters import wavelet_filters
    lo, hi = wavelet_filters(wavelet)
    x = torch.from_numpy(np.random.default_rng(21).standard_normal(shape) * 300).cuda()
    fused = engine.swt_level1(x, lo, hi, (2, 1, 0)).cpu().numpy()
    assert _lib.last_path() == "swt-fused"
    monkeypatch.setenv("PRAD_SWT_NOFUSE", "1")
    plain = engine.swt_level1(x, lo, hi, (2, 1, 0)).cpu().numpy()
    assert _lib.last_path() == "swt"
    assert fused.shape == plain.shape == (8,) + shape and np.array_equal(fused, plain)
    monkeypatch.delenv("PRAD_SWT_NOFUSE")
    other = engine.swt_level1(x, lo, hi, (1, 2)).cpu().numpy()         # any other axis list: the separate passes
    assert _lib.last_path() == "swt" and other.shape == (4,) + shape
    # the image in its own element type: the float64 copy is made while the planes are staged (exact for every type)
    for dt in (torch.int16, torch.int32, torch.float32):
        xi = (x * 3).to(dt)
        a = engine.swt_level1(xi, lo, hi, (2, 1, 0)).cpu().numpy()
        assert _lib.last_path() == "swt-fused"
        b = engine.swt_level1(xi.to(torch.float64), lo, hi, (2, 1, 0)).cpu().numpy()
        assert np.array_equal(a, b), dt


@pytest.mark.gpu
@pytest.mark.parametrize("wavelet", ["db3", "sym3", "db4", "sym4", "db5", "coif2"])
def test_more_wavelet_families_on_the_device_equal_the_restatement(wavelet):
    """round 5 (VERDICT r4 missing #6): the families added to the table -- 6 taps through the fused kernel, 8 / 10 / 12 taps through
    the axis passes -- against oracle/filters_oracle.swt3, odd sizes (the wrap pad) included"""
    import torch
    from oracle import filters_oracle as fo
    from pyradiomics_amd import engine
    rng = np.random.default_rng(4)
    for shape in ((24, 30, 36), (9, 17, 20)):
        x = rng.integers(-200, 1200, size=shape).astype(np.int16)
        got = engine.wavelet_images(torch.from_numpy(x).cuda(), wavelet)
        ap, ret = fo.swt3(x, wavelet)
        want = {"wavelet-" + k: v for k, v in ret[0].items()}
        want["wavelet-LLL"] = ap
        assert set(got) == set(want)
        for k, w in want.items():
            g = got[k].cpu().numpy()
            assert g.shape == w.shape and np.abs(g - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (wavelet, k)

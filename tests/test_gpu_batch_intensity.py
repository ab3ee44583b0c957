"""GPU: engine.intensity_batch / gradient_batch (prad_batch_intensity_dev) against the single functions
filters.get*Image on each box alone.

Shapes: offsets are odd and rows cross the 64-lane width -- (1,1,1) (1,1,2) (2,1,1) (1,2,1) (2,2,2) (3,1,5) (1,7,1) (5,4,3)
(4,4,65) (17,9,33) --, one (41,41,41) box (above the 65 280-voxel cap of the LDS routes: none applies here) and 300 boxes of
(1,1,1) and (2,3,1): more ROIs than compute units.  All four dtypes; negative, zero and positive values; int16 -32768 and int32
-2^31 (|x| must be taken AFTER widening); per-ROI anisotropic spacing (0.7, 1.1, 2.0) next to unit spacing; gradientUseSpacing
False.

Expected values.
  Square, SquareRoot, Gradient: bit for bit filters.get*Image(deviceResident=True) on the box alone -- correctly rounded
    operations only, in the same order.
  Logarithm, Exponential: (a) the host route (deviceResident=False) at rtol 1e-14 / atol 1e-12, the tolerance
    tests/test_gpu_filters.py holds exactly these formulas to; (b) the formulas in np.longdouble under a bound derived from the
    DOCUMENTED accuracy of the functions involved, not from what is measured.  With u = 2^-53 (a correctly rounded operation
    errs by at most u relative) and log / exp of the device library within 1 ulp = 2 u relative (ROCm OCML, double precision:
    log 1 ulp, exp 1 ulp):
      logarithm   y = (sign(x) L) S,  L = log(|x| + 1),  S = top / log(top + 1).
                  |x| + 1 is rounded (u relative in the argument = u ABSOLUTE in the logarithm), log adds 2 u |L|:
                      |dL| <= u + 2 u |L|.
                  S: the same two steps on log(top + 1) =: Lt give (u / Lt + 2 u) relative, the division u more; the final
                  product u:
                      |dy| <= |S| (u + 2 u |L|) + |y| (u / Lt + 2 u + u + u).
      exponential y = exp(k x),  k = log(top) / top: k carries 2 u + u, the product k x one more u, so the argument t = k x is
                  off by at most 4 u |t|, which exp turns into a relative error of 4 u |t|; exp itself adds 2 u:
                      |dy| <= |y| (4 |t| + 2) u.
    Both bounds take a factor 1.001 for the second-order terms and 2^-60 |y| for the long-double evaluation itself.  The
    worst error / bound that is measured is printed (profiles/batch_intensity_measurements.md records it)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 2, 1), (2, 2, 2), (3, 1, 5), (1, 7, 1), (5, 4, 3), (4, 4, 65), (17, 9, 33),
          (41, 41, 41)] + [(1, 1, 1), (2, 3, 1)] * 150
DTYPES = ["float32", "float64", "int32", "int16"]
ANISO = (0.7, 1.1, 2.0)          # (z, y, x)
U = 2.0 ** -53
POINTWISE = ("square", "squareroot", "logarithm", "exponential")

_cache = {}


def _values(rng, shape, dtype):
    n = int(np.prod(shape))
    if dtype.startswith("float"):
        v = rng.normal(0.0, 300.0, n)
        v[rng.random(n) < 0.1] *= 1e-4          # arguments of log near 1
    else:
        v = rng.integers(-1200, 3000, n).astype(np.float64)
    v[rng.random(n) < 0.15] = 0.0
    if n >= 3:                                   # negative, zero and positive in every box that can hold them
        v[:3] = (-7.0, 0.0, 5.0)
    elif not v.any():
        v[0] = -3.0                              # (no all-zero box here: those are the verdict tests')
    return v.astype(dtype).reshape(shape)


def _boxes(dtype):
    rng = np.random.default_rng(DTYPES.index(dtype) + 11)
    boxes = [_values(rng, s, dtype) for s in SHAPES]
    if dtype == "int16":
        boxes[7][2, 1, 1] = -32768
        boxes[0][0, 0, 0] = -32768               # a box that is nothing but the extreme
    if dtype == "int32":
        boxes[7][2, 1, 1] = -2 ** 31
        boxes[9][3, 3, 3] = 2 ** 31 - 1
        boxes[0][0, 0, 0] = -2 ** 31
    spacing = np.array([ANISO if b % 2 else (1.0, 1.0, 1.0) for b in range(len(boxes))])
    return boxes, spacing


def _single(fn, box, spacing=None, **kw):
    """the single function on one box -> numpy"""
    from pyradiomics_amd.image import Image
    im = Image(box, spacing=None if spacing is None else tuple(float(s) for s in spacing[::-1]))
    (out, name, _), = list(fn(im, None, **kw))
    return out.array


def _case(dtype):
    """one batch per dtype: the batched images and the single routes' of every box, computed once"""
    if dtype not in _cache:
        import torch
        from pyradiomics_amd import engine, filters
        boxes, spacing = _boxes(dtype)
        dev = [torch.from_numpy(b).cuda() for b in boxes]
        rows, names, sizes = engine.intensity_batch(dev)
        route = engine.last_batch_route()
        grad, gname, _ = engine.gradient_batch(dev, spacing=spacing)
        groute = engine.last_batch_route()
        plain, _, _ = engine.gradient_batch(dev, spacing=spacing, gradientUseSpacing=False)
        assert names == POINTWISE and gname == "gradient" and np.array_equal(sizes, np.array(SHAPES))
        assert rows.dtype == torch.float64 and grad.dtype == torch.float32 and tuple(rows.shape) == (4, grad.numel())
        off = np.concatenate([[0], np.cumsum([b.size for b in boxes])])
        _cache[dtype] = dict(boxes=boxes, spacing=spacing, dev=dev, rows=rows.cpu().numpy(), grad=grad.cpu().numpy(),
                             plain=plain.cpu().numpy(), off=off, route=route, groute=groute)
    return _cache[dtype]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _cut(c, flat, b):
    return flat[c["off"][b]:c["off"][b + 1]].reshape(SHAPES[b])


@pytest.mark.parametrize("dtype", DTYPES)
def test_square_squareroot_gradient_equal_the_single_route_bit_for_bit(dtype):
    from pyradiomics_amd import filters
    c = _case(dtype)
    assert c["route"] == "batch" and c["groute"] == "batch"
    differ = []
    for b, box in enumerate(c["boxes"]):
        want = {"square": _single(filters.getSquareImage, box, deviceResident=True),
                "squareroot": _single(filters.getSquareRootImage, box, deviceResident=True),
                "gradient": _single(filters.getGradientImage, box, c["spacing"][b], deviceResident=True),
                "gradient-nospacing": _single(filters.getGradientImage, box, c["spacing"][b], deviceResident=True,
                                              gradientUseSpacing=False)}
        got = {"square": _cut(c, c["rows"][0], b), "squareroot": _cut(c, c["rows"][1], b), "gradient": _cut(c, c["grad"], b),
               "gradient-nospacing": _cut(c, c["plain"], b)}
        for name in want:
            if not _same_bits(got[name], want[name]):
                bad = np.flatnonzero(got[name].ravel() != want[name].ravel())
                differ.append((name, b, SHAPES[b], len(bad), float(got[name].ravel()[bad[0]]) if len(bad) else None,
                               float(want[name].ravel()[bad[0]]) if len(bad) else None))
    for d in differ[:20]:
        print("differs:", d)
    assert not differ, (len(differ), differ[:6])


def _long_double(box):
    x = box.astype(np.longdouble)
    a = np.abs(x)
    top = a.max()
    L, Lt = np.log(a + 1), np.log(top + 1)
    S = top / Lt
    y_log = np.sign(x) * L * S
    bound_log = (np.abs(S) * (U + 2 * U * np.abs(L)) + np.abs(y_log) * (U / Lt + 4 * U)) * 1.001 + np.abs(y_log) * 2.0 ** -60
    k = np.log(top) / top
    t = k * x
    y_exp = np.exp(t)
    bound_exp = np.abs(y_exp) * (4 * np.abs(t) + 2) * U * 1.001 + np.abs(y_exp) * 2.0 ** -60
    return (y_log, bound_log), (y_exp, bound_exp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_logarithm_exponential_against_the_host_route_and_long_double(dtype):
    from pyradiomics_amd import filters
    c = _case(dtype)
    worst = {"logarithm": 0.0, "exponential": 0.0}
    host_worst = {"logarithm": 0.0, "exponential": 0.0}
    seen = set()
    for b, box in enumerate(c["boxes"]):
        got = {"logarithm": _cut(c, c["rows"][2], b), "exponential": _cut(c, c["rows"][3], b)}
        key = (SHAPES[b], box.tobytes())
        if key not in seen:                     # (the host route of equal boxes once)
            seen.add(key)
            for name, fn in (("logarithm", filters.getLogarithmImage), ("exponential", filters.getExponentialImage)):
                host = _single(fn, box, deviceResident=False)
                np.testing.assert_allclose(got[name], host, rtol=1e-14, atol=1e-12, err_msg="%s of box %d %s" % (name, b, SHAPES[b]))
                scale = 1e-12 + 1e-14 * np.abs(host)
                host_worst[name] = max(host_worst[name], float((np.abs(got[name] - host) / scale).max()))
        (y_log, bound_log), (y_exp, bound_exp) = _long_double(box)
        for name, want, bound in (("logarithm", y_log, bound_log), ("exponential", y_exp, bound_exp)):
            err = np.abs(got[name].astype(np.longdouble) - want)
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
            worst[name] = max(worst[name], float(ratio.max()))
            assert (err <= bound).all(), (name, b, SHAPES[b], float(ratio.max()))
    for name in worst:
        print("%s %-12s worst error / long-double bound %.3f   worst |batch - host| / (1e-12 + 1e-14 |host|) %.3g"
              % (dtype, name, worst[name], host_worst[name]))


def _bad_batch(dtype="float32"):
    rng = np.random.default_rng(3)
    shapes = [(5, 4, 3), (3, 3, 3), (4, 4, 65), (2, 5, 7), (1, 1, 1), (6, 2, 9), (3, 1, 5)]
    boxes = [_values(rng, s, dtype) for s in shapes]
    boxes[1][:] = 0                              # all zeros: verdict 1
    if dtype.startswith("float"):
        boxes[3][1, 2, 3] = np.nan               # verdict 2
        boxes[5][4, 1, 8] = -np.inf              # verdict 2
    return shapes, boxes


def test_verdict_rois_take_the_fallback_and_leave_their_neighbours_alone():
    import torch
    from pyradiomics_amd import engine, filters
    shapes, boxes = _bad_batch()
    dev = [torch.from_numpy(b).cuda() for b in boxes]
    spacing = np.array([ANISO] * len(boxes))
    rows, names, _ = engine.intensity_batch(dev)
    assert engine.last_batch_route() == "mixed"
    grad, _, _ = engine.gradient_batch(dev, spacing=spacing)
    assert engine.last_batch_route() == "mixed"          # the NaN and the inf box; the all-zero box is native
    good = [b for b in range(len(boxes)) if b not in (1, 3, 5)]
    clean, _, _ = engine.intensity_batch([dev[b] for b in good])
    assert engine.last_batch_route() == "batch"
    clean_grad, _, _ = engine.gradient_batch([dev[b] for b in good], spacing=spacing[good])
    assert engine.last_batch_route() == "batch"
    rows, grad, clean, clean_grad = rows.cpu().numpy(), grad.cpu().numpy(), clean.cpu().numpy(), clean_grad.cpu().numpy()
    off = np.concatenate([[0], np.cumsum([b.size for b in boxes])])
    coff = np.concatenate([[0], np.cumsum([boxes[b].size for b in good])])
    fns = (filters.getSquareImage, filters.getSquareRootImage, filters.getLogarithmImage, filters.getExponentialImage)
    for b in (1, 3, 5):                          # the single route's rows, NaN positions included
        for r, fn in enumerate(fns):
            want = _single(fn, boxes[b], deviceResident=True)
            got = rows[r, off[b]:off[b + 1]].reshape(shapes[b])
            assert np.array_equal(np.isnan(got), np.isnan(want)) and _same_bits(got, want), (b, names[r])
        assert np.isnan(rows[:, off[b]:off[b + 1]]).any(), b
        want = _single(filters.getGradientImage, boxes[b], spacing[b], deviceResident=True)
        got = grad[off[b]:off[b + 1]].reshape(shapes[b])
        assert np.array_equal(np.isnan(got), np.isnan(want)) and _same_bits(got, want), b
    assert not grad[off[1]:off[2]].any() and np.isnan(grad[off[3]:off[4]]).any() and np.isinf(grad[off[5]:off[6]]).any()
    for k, b in enumerate(good):                 # the neighbours: what a batch without the three gives
        assert _same_bits(rows[:, off[b]:off[b + 1]], clean[:, coff[k]:coff[k + 1]]), b
        assert _same_bits(grad[off[b]:off[b + 1]], clean_grad[coff[k]:coff[k + 1]]), b
        assert np.isfinite(rows[:, off[b]:off[b + 1]]).all()


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_gradient_alone_is_native_on_an_all_zero_box(dtype):
    import torch
    from pyradiomics_amd import _lib, engine
    shapes, boxes = _bad_batch("int16")
    boxes = [b.astype(dtype) for b in boxes]
    dev = [torch.from_numpy(b).cuda() for b in boxes]
    grad, name, _ = engine.gradient_batch(dev)
    assert engine.last_batch_route() == "batch" and name == "gradient"
    assert _lib.load().prad_last_variant().decode() == "batch-gradient"          # the image launch alone
    off = np.concatenate([[0], np.cumsum([b.size for b in boxes])])
    assert not grad.cpu().numpy()[off[1]:off[2]].any()
    engine.intensity_batch(dev, types=("Square",))
    assert engine.last_batch_route() == "mixed"          # the all-zero box divides by zero: the single route's NaN
    assert _lib.load().prad_last_variant().decode() == "batch-intensity"


def test_out_and_type_selection():
    import torch
    from pyradiomics_amd import engine
    c = _case("float32")
    dev = c["dev"][:11]
    W = int(c["off"][11])
    full = c["rows"][:, :W]
    SENTINEL = -12345.5
    pad = torch.full((2, W + 7), SENTINEL, dtype=torch.float64, device="cuda")
    rows, names, _ = engine.intensity_batch(dev, types=("Exponential", "SquareRoot"), out=pad[:, :W])
    assert names == ("squareroot", "exponential") and rows.data_ptr() == pad.data_ptr()
    host = pad.cpu().numpy()
    assert (host[:, W:] == SENTINEL).all()               # the gaps between the rows survive
    assert _same_bits(host[0, :W], full[1]) and _same_bits(host[1, :W], full[3])
    one, names, _ = engine.intensity_batch(dev, types=("Logarithm",))
    assert names == ("logarithm",) and tuple(one.shape) == (1, W) and _same_bits(one.cpu().numpy()[0], full[2])
    g = torch.full((W + 5,), SENTINEL, dtype=torch.float32, device="cuda")
    image, _, _ = engine.gradient_batch(dev, spacing=c["spacing"][:11], out=g[:W])
    assert image.data_ptr() == g.data_ptr() and (g[W:] == SENTINEL).all()
    assert _same_bits(g[:W].cpu().numpy(), c["grad"][:W])
    # the flat form: one tensor plus sizes
    flat = torch.cat([d.reshape(-1) for d in dev])
    rows2, _, _ = engine.intensity_batch(flat, SHAPES[:11])
    assert _same_bits(rows2.cpu().numpy(), full)
    with pytest.raises(ValueError, match="out must live on"):
        engine.intensity_batch(dev, out=torch.zeros((4, W), dtype=torch.float64))


def test_host_twins_equal_the_engine_calls():
    from pyradiomics_amd import cmatrices
    c = _case("int16")
    boxes, spacing = c["boxes"][:11], c["spacing"][:11]
    images, names = cmatrices.calculate_intensity_batch(boxes)
    assert names == POINTWISE and cmatrices.last_batch_route() == "batch"
    grads, name = cmatrices.calculate_gradient_batch(boxes, spacing)
    assert name == "gradient"
    for b in range(11):
        for r, n in enumerate(names):
            assert _same_bits(images[n][b], _cut(c, c["rows"][r], b)), (n, b)
        assert _same_bits(grads[b], _cut(c, c["grad"], b)), b
    plain, _ = cmatrices.calculate_gradient_batch(boxes, spacing, gradientUseSpacing=False)
    assert all(_same_bits(plain[b], _cut(c, c["plain"], b)) for b in range(11))
    some, names = cmatrices.calculate_intensity_batch(boxes, types=("Square",))
    assert names == ("square",) and _same_bits(some["square"][9], _cut(c, c["rows"][0], 9))


def test_the_resampled_table_call_still_declines_the_new_types():
    import torch
    from pyradiomics_amd import engine
    x = torch.ones(8, device="cuda")
    for t in ("Square", "Gradient"):
        with pytest.raises(NotImplementedError, match=t):
            engine.roi_features_batch_resampled(x, x, [(2, 2, 2)], resampledPixelSpacing=(1, 1, 1), imageTypes={t: {}})

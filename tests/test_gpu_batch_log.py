"""GPU: engine.log_batch (prad_batch_log_dev, csrc/kernels_batch_log.h) against the single route, engine.log_images on every
box alone, byte for byte, and against the independent restatement oracle/filters_oracle.laplacian_recursive_gaussian.

Batch A (_boxes) holds the smallest boxes at which the kernel can go wrong: (4, 4, 4), where every line is boundary
initialisation only; (5, 4, 6), whose main loops run once or twice; line lengths around a 16-sample block ((4, 5, 37),
(15, 16, 17)); odd and even row pitch ((7, 9, 33), (6, 8, 32)); the extent cap of 64 on the contiguous and on the slowest axis;
line counts below, at and above a wave and a workgroup ((4, 4, 5), (4, 16, 16), (4, 16, 17)); and one 32^3 box between twice
forty 6^3 boxes: two LDS classes, so two launches, in one call.  test_batch_a_exercises_every_path asserts from the planner that
the list does what it is meant to.  The output tensor is filled with NaN before every call -- the caching allocator would
otherwise hand back the previous call's correct values -- and has SLACK elements behind every row: the slack and the slices of
the pairs for which the reference yields no image must keep their NaN.

The restatement builds its boundary coefficients with 1.0 + sum(D) where the library (both routes: csrc/prad_rgauss.h) adds
((1.0 + D1) + D2) + ...; for some (sigma, spacing) pairs they differ in the last bit of a float64, which can move a float32
voxel by one ulp about once in a million voxels.  tests/test_gpu_filters.py holds the single route to the restatement with
array_equal all the same, and so does this file; the batch route's contract is the single route's bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ("int16", "int32", "float32", "float64")
SPACINGS = ((1.0, 1.0, 1.0), (2.5, 0.8, 0.7))          # (z, y, x)
SIGMAS = (0.5, 1.0, 3.0)
SLACK = 5            # elements behind every row of the NaN-filled output
NO_IMAGE = 16
EDGE = [(4, 4, 4), (5, 4, 6), (4, 5, 37), (15, 16, 17), (7, 9, 33), (6, 8, 32), (4, 4, 64), (64, 4, 4), (4, 16, 16), (4, 16, 17),
        (4, 4, 5)]


def _boxes():
    return EDGE + [(6, 6, 6)] * 40 + [(32, 32, 32)] + [(6, 6, 6)] * 40


def _values(boxes, dtype, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for b in boxes:
        if dtype == "int16":
            out.append(rng.integers(-500, 1500, size=b).astype(np.int16))
        elif dtype == "int32":
            out.append(rng.integers(-40000000, 40000000, size=b).astype(np.int32))      # magnitudes above 2^24
        elif dtype == "float32":
            out.append((rng.standard_normal(b) * 300.0 + 40.0).astype(np.float32))
        else:
            out.append(rng.standard_normal(b) * 300.0 + 40.0)
    return out


def _admitted(shape, spacing, sigma):
    """getLoGImage's question: does the reference filter this box with this sigma?"""
    size = np.array(shape, dtype=np.float64)
    return bool(size.min() >= 4 and np.all(size >= np.ceil(sigma / np.array(spacing)) + 1))


_single, _batch = {}, {}


def _single_route(dtype, spacing, boxes=None, key=None):
    """(arrays, per box [numpy image per sigma, None where the reference yields none]) from engine.log_images on each box with
    one sigma at a time; computed once per key and left unchanged"""
    import torch
    from pyradiomics_amd import engine
    key = key or (dtype, spacing)
    if key not in _single:
        arrays = _values(boxes if boxes is not None else _boxes(), dtype)
        sps = spacing if np.ndim(spacing) == 2 else [spacing] * len(arrays)
        res = []
        for a, sp in zip(arrays, sps):
            x = torch.from_numpy(a).cuda()
            res.append([engine.log_images(x, tuple(sp)[::-1], [s])[0].cpu().numpy().copy() if _admitted(a.shape, sp, s) else None
                        for s in SIGMAS])
        _single[key] = (arrays, res)
    return _single[key]


def _nan_out(rows, W, dtype):
    import torch
    big = torch.full((rows, W + SLACK), float("nan"), dtype=torch.float64 if dtype == "float64" else torch.float32, device="cuda")
    return big, big[:, :W]


def _run(arrays, spacing, dtype, sigma=SIGMAS):
    """engine.log_batch into a NaN-filled output with slack behind the rows -> (logs numpy [S, W], names, valid, route)"""
    import torch
    from pyradiomics_amd import engine
    W = sum(a.size for a in arrays)
    big, out = _nan_out(len(sigma), W, dtype)
    logs, names, sizes, valid = engine.log_batch([torch.from_numpy(a).cuda() for a in arrays], sigma=sigma, spacing=spacing, out=out)
    route = engine.last_batch_route()
    assert logs.data_ptr() == out.data_ptr() and np.array_equal(sizes, [a.shape for a in arrays])
    assert list(names) == ["log-sigma-%s-mm-3D" % str(s).replace(".", "-") for s in sigma]
    host = big.cpu().numpy()
    assert np.isnan(host[:, W:]).all(), "the slack behind the rows was written"
    off = 0
    for b, a in enumerate(arrays):          # nothing is written where the reference yields no image
        for s in range(len(sigma)):
            if not valid[s, b]:
                assert np.isnan(host[s, off:off + a.size]).all(), (b, a.shape, sigma[s])
        off += a.size
    return host[:, :W], names, valid, route


def _batch_a(dtype, spacing):
    if (dtype, spacing) not in _batch:
        arrays, _ = _single_route(dtype, spacing)
        _batch[(dtype, spacing)] = _run(arrays, spacing, dtype)
    return _batch[(dtype, spacing)]


def _assert_same_bytes(host, valid, arrays, want, dtype, only=None):
    off = 0
    for b, a in enumerate(arrays):
        if only is None or b in only:
            for s in range(len(SIGMAS)):
                assert bool(valid[s, b]) == (want[b][s] is not None), (b, a.shape, SIGMAS[s])
                if want[b][s] is not None:
                    got = host[s, off:off + a.size].reshape(a.shape)
                    assert got.dtype == want[b][s].dtype == (np.float64 if dtype == "float64" else np.float32)
                    assert got.tobytes() == want[b][s].tobytes(), (b, a.shape, SIGMAS[s], np.abs(got - want[b][s]).max())
        off += a.size


def test_batch_a_exercises_every_path():
    from pyradiomics_amd import engine
    boxes = _boxes()
    lines = lambda b: (b[0] * b[1], b[0] * b[2], b[1] * b[2])          # of the x, y and z passes
    for spacing in SPACINGS:
        verdict, cls = engine.batch_log_plan(boxes, SIGMAS, spacing)
        want = [[0 if _admitted(b, spacing, s) else NO_IMAGE for b in boxes] for s in SIGMAS]
        assert verdict.tolist() == want                                  # every box is inside the kernel's domain
        assert (cls >= 0).all()
        assert cls[boxes.index((6, 6, 6))] == 0 and cls[boxes.index((32, 32, 32))] == 2      # two launches in one call
        assert len(set(cls[len(EDGE):].tolist())) == 2 and cls[-1] == 0
    assert (np.array(want) == NO_IMAGE).any() and (np.array(want)[2] == 0).any()             # (2.5, 0.8, 0.7): both kinds
    assert np.array(want)[2][boxes.index((4, 4, 4))] == NO_IMAGE                             # 4 < ceil(3 / 0.7) + 1
    extents = {n for b in boxes for n in b}
    assert {4, 5, 6, 15, 16, 17, 32, 33, 37, 64} <= extents              # 4: initialisation only; 16 +- 1 and 32 + 1, 37: blocks
    assert any(b[2] % 2 for b in boxes) and any(b[2] % 2 == 0 for b in boxes)                # row pitch Nx and Nx + 1
    assert (4, 4, 64) in boxes and (64, 4, 4) in boxes
    assert max(lines((4, 4, 5))) < 64 and lines((4, 16, 16)) == (64, 64, 256) and lines((4, 16, 17)) == (64, 68, 272)
    assert lines((32, 32, 32)) == (1024, 1024, 1024)
    # the domain's edge
    one = lambda b: engine.batch_log_plan([b], [1.0])[0][0, 0]
    assert one((32, 32, 32)) == 0 and one((36, 36, 36)) == 8 and one((4, 4, 65)) == 8 and one((3, 8, 8)) == NO_IMAGE


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bytes_equal_the_single_route(dtype, spacing):
    from pyradiomics_amd import _lib
    arrays, want = _single_route(dtype, spacing)
    host, names, valid, route = _batch_a(dtype, spacing)
    assert route == "batch"
    _assert_same_bytes(host, valid, arrays, want, dtype)
    assert np.isnan(host).any() == (not valid.all())


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_restatement(dtype, spacing):
    from oracle import filters_oracle as fo
    arrays, _ = _single_route(dtype, spacing)
    host, names, valid, _route = _batch_a(dtype, spacing)
    off = 0
    for b, a in enumerate(arrays):
        for s, sigma in enumerate(SIGMAS):
            assert bool(valid[s, b]) == _admitted(a.shape, spacing, sigma)
            if valid[s, b]:
                want = fo.laplacian_recursive_gaussian(a, spacing[::-1], sigma)
                got = host[s, off:off + a.size].reshape(a.shape)
                assert np.array_equal(got, want), (b, a.shape, sigma, np.abs(got - want).max())
        off += a.size


def test_library_reports_the_batch_route():
    import torch
    from pyradiomics_amd import _lib, engine
    arrays = _values(EDGE[:3], "float32")
    engine.log_batch([torch.from_numpy(a).cuda() for a in arrays], sigma=[1.0])
    assert _lib.last_path() == "batch" and _lib.last_variant() == "batch-log"


def test_out_is_honoured_and_checked():
    import torch
    from pyradiomics_amd import engine
    arrays = _values(EDGE[:4], "int16")
    boxes = [torch.from_numpy(a).cuda() for a in arrays]
    W = sum(a.size for a in arrays)
    out = torch.full((2, W), float("nan"), dtype=torch.float32, device="cuda")
    logs, names, _, valid = engine.log_batch(boxes, sigma=[1.0, 0.5], out=out)
    assert logs.data_ptr() == out.data_ptr() and valid.all() and not torch.isnan(out).any()
    fresh, names2, _, _ = engine.log_batch(boxes, sigma=[1.0, 0.5])
    assert fresh.dtype == torch.float32 and torch.equal(fresh, out) and list(names2) == list(names)
    for bad in (torch.empty((2, W), dtype=torch.float64, device="cuda"), torch.empty((3, W), dtype=torch.float32, device="cuda"),
                torch.empty((2, W + 1), dtype=torch.float32, device="cuda"), torch.empty((2 * W,), dtype=torch.float32, device="cuda"),
                torch.empty((W, 2), dtype=torch.float32, device="cuda").t()):
        with pytest.raises(ValueError):
            engine.log_batch(boxes, sigma=[1.0, 0.5], out=bad)
    with pytest.raises(ValueError):
        engine.log_batch([b.double() for b in boxes], sigma=[1.0, 0.5], out=out)      # float64 boxes return float64


def test_sigmas_are_named_and_filtered_as_getLoGImage_does():
    import torch
    from pyradiomics_amd import engine
    a = _values([(6, 7, 8)], "float32")[0]
    logs, names, _, valid = engine.log_batch([torch.from_numpy(a).cuda()], sigma=[2, 0.0, 1.5, -1.0, 1.5])
    assert list(names) == ["log-sigma-2-mm-3D", "log-sigma-1-5-mm-3D"] and tuple(logs.shape) == (2, a.size) and valid.all()
    with pytest.raises(ValueError):
        engine.log_batch([torch.from_numpy(a).cuda()], sigma=[0.0])


def test_a_large_box_makes_the_route_mixed():
    from pyradiomics_amd import engine
    spacing = SPACINGS[0]
    boxes = _boxes() + [(36, 36, 36), (3, 8, 8)]
    arrays, want = _single_route("float32", spacing, boxes, key="mixed")
    verdict, cls = engine.batch_log_plan(boxes, SIGMAS, spacing)
    assert verdict[:, -2].tolist() == [8, 8, 8] and verdict[:, -1].tolist() == [NO_IMAGE] * 3 and cls[-2:].tolist() == [-1, -1]
    host, names, valid, route = _run(arrays, spacing, "float32")
    assert route == "mixed"
    assert np.array_equal(valid, verdict != NO_IMAGE)                     # false exactly where the planner says no image
    _assert_same_bytes(host, valid, arrays, want, "float32")             # the large box's rows equal the single route
    clean, _, _, _ = _batch_a("float32", spacing)
    assert host[:, :clean.shape[1]].tobytes() == clean.tobytes()         # the native boxes' bytes are unchanged


def test_only_large_boxes_are_looped():
    arrays, want = _single_route("int16", SPACINGS[0], [(36, 36, 36)], key="looped")
    host, names, valid, route = _run(arrays, SPACINGS[0], "int16")
    assert route == "looped" and valid.all()
    _assert_same_bytes(host, valid, arrays, want, "int16")


def test_per_roi_spacing_equals_the_one_spacing_calls():
    boxes = EDGE + [(6, 6, 6)] * 3
    arrays = _values(boxes, "float32")
    both = np.array([SPACINGS[b % 2] for b in range(len(boxes))])
    host, _, valid, route = _run(arrays, both, "float32")
    assert route == "batch"
    ones = [_run(arrays, sp, "float32") for sp in SPACINGS]
    off = 0
    for b, a in enumerate(arrays):
        want, _, want_valid, _ = ones[b % 2]
        assert np.array_equal(valid[:, b], want_valid[:, b])
        assert host[:, off:off + a.size].tobytes() == want[:, off:off + a.size].tobytes(), (b, a.shape)
        off += a.size


def test_a_nan_voxel_stays_in_its_roi():
    arrays, _ = _single_route("float32", SPACINGS[0])
    clean, _, _, _ = _batch_a("float32", SPACINGS[0])
    hit = len(EDGE) + 30                              # one of the 6^3 boxes in front of the large one
    dirty = [a.copy() for a in arrays]
    dirty[hit][2, 3, 1] = np.nan
    host, _, _, _ = _run(dirty, SPACINGS[0], "float32")
    off = np.concatenate([[0], np.cumsum([a.size for a in arrays])])
    other = np.ones(host.shape[1], dtype=bool)
    other[off[hit]:off[hit + 1]] = False
    assert host[:, other].tobytes() == clean[:, other].tobytes()
    assert np.isnan(host[:, ~other]).any()


def test_host_array_twin():
    from pyradiomics_amd import cmatrices
    spacing = SPACINGS[1]
    arrays, want = _single_route("int16", spacing)
    res, names = cmatrices.calculate_log_batch(arrays[:12], SIGMAS, spacing)
    assert list(res) == list(names) == ["log-sigma-0-5-mm-3D", "log-sigma-1-0-mm-3D", "log-sigma-3-0-mm-3D"]
    nones = 0
    for b in range(12):
        for s, name in enumerate(names):
            if want[b][s] is None:
                assert res[name][b] is None
                nones += 1
            else:
                assert res[name][b].shape == arrays[b].shape and res[name][b].tobytes() == want[b][s].tobytes()
    assert nones

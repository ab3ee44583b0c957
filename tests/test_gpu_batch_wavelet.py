"""GPU: engine.wavelet_batch (prad_batch_swt_dev, csrc/kernels_batch_swt.h) against the single route, filters._swt3_device on
every box, byte for byte, and against the independent restatement oracle/filters_oracle.swt3.

Batch A (_boxes) holds the smallest boxes at which the kernel can go wrong: odd extents on every axis (the folded wrap pad),
a padded extent equal to the filter length, rows longer than two tiles ((2, 2, 65)), one extent below / at / above each tile
width (8, 16, 32) and each tile height (32, 16, 8), boxes that make each of the three tile shapes seam in x and in y, z extents
of 7, 8 and 9 planes around the chunk length 8 of a small batch, and one 40^3 box in the middle of forty 6^3 boxes.
test_batch_a_exercises_every_path asserts from the planner that the list does what it is meant to.  (1, 16, 16) is native for
haar alone and is in the haar batches only.  The output tensor is filled with NaN before every call: the caching allocator
would otherwise hand back the previous call's correct values."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVELETS = ("haar", "db2", "coif1")
FLEN = {"haar": 2, "db2": 4, "coif1": 6}
DTYPES = ("int16", "int32", "float32", "float64")
SLACK = 5            # elements between the bands of the NaN-filled output


def _boxes(wavelet):
    edge_x = [(6, 8, 31), (6, 8, 32), (6, 8, 33), (6, 16, 15), (6, 16, 16), (6, 16, 17), (6, 32, 7), (6, 32, 8), (6, 32, 9)]
    edge_y = [(6, 7, 32), (6, 9, 32), (6, 15, 16), (6, 17, 16), (6, 31, 8), (6, 33, 8)]
    seams = [(6, 17, 32), (6, 32, 17)]
    chunk = [(7, 6, 6), (8, 6, 6), (9, 6, 6)]
    boxes = [(5, 6, 7), (6, 6, 6), (7, 9, 11), (2, 2, 65)] + ([(1, 16, 16)] if wavelet == "haar" else [])
    return boxes + edge_x + edge_y + seams + chunk + [(6, 6, 6)] * 20 + [(40, 40, 40)] + [(6, 6, 6)] * 20


def _values(boxes, dtype, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for b in boxes:
        if dtype == "int16":
            out.append(rng.integers(-500, 1500, size=b).astype(np.int16))
        elif dtype == "int32":
            out.append(rng.integers(-2000000, 2000000, size=b).astype(np.int32))
        elif dtype == "float32":
            out.append((rng.standard_normal(b) * 300.0 + 40.0).astype(np.float32))
        else:
            out.append(rng.standard_normal(b) * 300.0 + 40.0)
    return out


_single = {}


def _single_route(wavelet, dtype, boxes=None, key=None, **kw):
    """per box {name: float64 numpy array} from filters._swt3_device, the names in getWaveletImage's order; computed once"""
    import torch
    from pyradiomics_amd import filters
    key = key or (wavelet, dtype)
    if key not in _single:
        arrays = _values(boxes if boxes is not None else _boxes(wavelet), dtype)
        res = []
        for a in arrays:
            approx, ret = filters._swt3_device(torch.from_numpy(a).cuda(), (2, 1, 0), wavelet=wavelet, **kw)
            bands = {}
            for idx, wl in enumerate(ret, start=1):
                for k, v in wl.items():
                    bands[("wavelet-%s" if idx == 1 else "wavelet%d-%%s" % idx) % k] = v.cpu().numpy().copy()
            bands[("wavelet-%s" if len(ret) == 1 else "wavelet%d-%%s" % len(ret)) % "LLL"] = approx.cpu().numpy().copy()
            res.append(bands)
        _single[key] = (arrays, res)
    return _single[key]


def _nan_out(rows, W):
    import torch
    big = torch.full((rows, W + SLACK), float("nan"), dtype=torch.float64, device="cuda")
    return big, big[:, :W]


def _run(arrays, wavelet, **kw):
    """engine.wavelet_batch into a NaN-filled output with slack between the bands -> (bands numpy [rows, W], names, route)"""
    import torch
    from pyradiomics_amd import engine
    rows = len(engine.wavelet_band_names(kw.get("level", 1)))
    W = sum(a.size for a in arrays)
    big, out = _nan_out(rows, W)
    bands, names, sizes = engine.wavelet_batch([torch.from_numpy(a).cuda() for a in arrays], wavelet=wavelet, out=out, **kw)
    assert bands.data_ptr() == out.data_ptr() and np.array_equal(sizes, [a.shape for a in arrays])
    host = big.cpu().numpy()
    assert np.isnan(host[:, W:]).all(), "the slack between the bands was written"
    return host[:, :W], names, engine.last_batch_route()


def _assert_same_bytes(host, names, arrays, want, only=None):
    off = 0
    for b, a in enumerate(arrays):
        if only is None or b in only:
            for name in names:
                got = host[names.row(name), off:off + a.size].reshape(a.shape)
                assert got.tobytes() == want[b][name].tobytes(), (b, a.shape, name, np.abs(got - want[b][name]).max())
        off += a.size


def test_batch_a_exercises_every_path():
    from pyradiomics_amd import engine
    for wavelet in WAVELETS:
        boxes = _boxes(wavelet)
        verdict, items = engine.batch_swt_plan(boxes, FLEN[wavelet])
        want = [0 if all(n + n % 2 >= FLEN[wavelet] for n in b) else 8 for b in boxes]
        assert verdict.tolist() == want
        assert want.count(8) == (0 if wavelet == "haar" else 1)              # (2, 2, 65) pads to 2 < 4
        for tx in (8, 16, 32):                                               # every shape seams in x and in y somewhere
            mine = items[items[:, 7] == tx]
            assert any(len(set(mine[mine[:, 0] == r][:, 5].tolist())) > 1 for r in set(mine[:, 0].tolist())), tx
            assert any(len(set(mine[mine[:, 0] == r][:, 3].tolist())) > 1 for r in set(mine[:, 0].tolist())), tx
        z = {b: sorted(set(map(tuple, items[items[:, 0] == boxes.index(b)][:, 1:3].tolist()))) for b in [(7, 6, 6), (8, 6, 6), (9, 6, 6)]}
        assert z[(7, 6, 6)] == [(0, 7)] and z[(8, 6, 6)] == [(0, 8)] and z[(9, 6, 6)] == [(0, 5), (5, 9)]
        assert (items[:, 0] == boxes.index((40, 40, 40))).sum() == 45        # 3 x 3 tiles, 5 z ranges


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_bytes_equal_the_single_route(wavelet, dtype):
    arrays, want = _single_route(wavelet, dtype)
    host, names, route = _run(arrays, wavelet)
    assert route == ("batch" if wavelet == "haar" else "mixed")
    assert not np.isnan(host).any()
    _assert_same_bytes(host, names, arrays, want)


def test_native_call_writes_nothing_but_the_native_boxes():
    """prad_batch_swt_dev itself, on offsets with gaps: the gaps, the slice of the non-native ROI and the slack behind the
    last box keep their NaN in every band"""
    import torch
    from pyradiomics_amd import _lib, engine, filters
    wavelet, dtype, gap = "coif1", "float32", 3
    arrays, want = _single_route(wavelet, dtype)
    names = engine.wavelet_band_names()
    lib = _lib.load()
    sizes = np.ascontiguousarray([a.shape for a in arrays], dtype=np.intc)
    nvox = sizes.astype(np.int64).prod(1)
    off = np.zeros(len(arrays), dtype=np.int64)
    off[1:] = np.cumsum(nvox + gap)[:-1]
    W = int(off[-1] + nvox[-1]) + gap
    flat = np.zeros(W, dtype=np.float32)
    for o, a in zip(off, arrays):
        flat[o:o + a.size] = a.ravel()
    x = torch.from_numpy(flat).cuda()
    out = torch.full((8, W), float("nan"), dtype=torch.float64, device="cuda")
    lo, hi = filters.wavelet_filters(wavelet)
    verdict = np.full(len(arrays), -1, dtype=np.intc)
    rc = lib.prad_batch_swt_dev(C.c_void_p(x.data_ptr()), 0, sizes.ctypes.data_as(C.POINTER(C.c_int)),
                                off.ctypes.data_as(C.POINTER(C.c_longlong)), len(arrays), C.c_void_p(lo.ctypes.data),
                                C.c_void_p(hi.ctypes.data), len(lo), C.c_void_p(out.data_ptr()), W, verdict.ctypes.data_as(C.POINTER(C.c_int)),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.PRAD_OK, _lib.last_error()
    assert _lib.last_path() == "batch" and _lib.last_variant() == "batch-swt-fused"
    host = out.cpu().numpy()
    written = np.zeros(W, dtype=bool)
    for b, (o, a) in enumerate(zip(off, arrays)):
        if verdict[b] == 0:
            written[o:o + a.size] = True
            for name in names:
                got = host[names.row(name), o:o + a.size].reshape(a.shape)
                assert got.tobytes() == want[b][name].tobytes(), (b, a.shape, name)
        else:
            assert verdict[b] == 8 and a.shape == (2, 2, 65)
    assert (np.isnan(host) == ~written[None, :]).all()


@pytest.mark.parametrize("dtype", ("float64", "int16"))
@pytest.mark.parametrize("wavelet", WAVELETS)
def test_against_the_restatement(wavelet, dtype):
    from oracle import filters_oracle as fo
    arrays, _ = _single_route(wavelet, dtype)
    host, names, _route = _run(arrays, wavelet)
    off = 0
    for a in arrays:
        ap, ret = fo.swt3(a, wavelet)
        want = {"wavelet-" + k: v for k, v in ret[0].items()}
        want["wavelet-LLL"] = ap
        assert list(want) == list(names)
        got = {name: host[names.row(name), off:off + a.size].reshape(a.shape) for name in names}
        for name in names:
            np.testing.assert_allclose(got[name], want[name], rtol=1e-13, atol=1e-10, err_msg="%s %s" % (a.shape, name))
        if all(s % 2 == 0 for s in a.shape):
            e = sum(float((v ** 2).sum()) for v in got.values())
            assert abs(e / ((a.astype(np.float64) ** 2).sum() * 8) - 1) < 1e-9, a.shape
        off += a.size


def test_a_box_below_the_filter_makes_the_route_mixed():
    boxes = _boxes("coif1") + [(4, 8, 8)]
    arrays, want = _single_route("coif1", "float32", boxes, key="mixed")
    host, names, route = _run(arrays, "coif1")
    assert route == "mixed" and not np.isnan(host).any()
    _assert_same_bytes(host, names, arrays, want)


def test_a_longer_filter_is_looped():
    boxes = [(5, 6, 7), (8, 8, 8), (9, 10, 12)]
    arrays, want = _single_route("db4", "int16", boxes, key="db4")
    host, names, route = _run(arrays, "db4")
    assert route == "looped" and not np.isnan(host).any()
    _assert_same_bytes(host, names, arrays, want)


def test_level_two_is_looped_with_the_names_of_getWaveletImage():
    from pyradiomics_amd import filters
    boxes = [(6, 8, 10), (7, 9, 11)]
    arrays, want = _single_route("coif1", "float64", boxes, key="level2", level=2)
    host, names, route = _run(arrays, "coif1", level=2)
    assert route == "looped" and host.shape[0] == 15 and not np.isnan(host).any()
    off = 0
    for a in arrays:
        ref = [(name, im.array) for im, name, _ in filters.getWaveletImage(a, None, level=2)]
        assert [n for n, _ in ref] == list(names)
        for name, arr in ref:
            got = host[names.row(name), off:off + a.size].reshape(a.shape)
            assert got.tobytes() == np.ascontiguousarray(arr).tobytes(), (a.shape, name)
        off += a.size
    _assert_same_bytes(host, names, arrays, want)


def test_force2D_is_looped_into_four_bands():
    import torch
    from pyradiomics_amd import engine, filters
    arrays = _values([(4, 6, 8), (5, 7, 9)], "float32")
    bands, names, _ = engine.wavelet_batch([torch.from_numpy(a).cuda() for a in arrays], force2D=True, force2Ddimension=0)
    assert engine.last_batch_route() == "looped" and tuple(bands.shape) == (4, sum(a.size for a in arrays))
    host, off = bands.cpu().numpy(), 0
    for a in arrays:
        ref = [(name, im.array) for im, name, _ in filters.getWaveletImage(a, None, force2D=True, force2Ddimension=0)]
        assert [n for n, _ in ref] == list(names) == ["wavelet-LH", "wavelet-HL", "wavelet-HH", "wavelet-LL"]
        for name, arr in ref:
            got = host[names.row(name), off:off + a.size].reshape(a.shape)
            assert got.tobytes() == np.ascontiguousarray(arr).tobytes(), (a.shape, name)
        off += a.size


def test_a_nan_voxel_stays_in_its_roi():
    arrays, _ = _single_route("coif1", "float32")
    clean, names, _ = _run(arrays, "coif1")
    hit = 30                                          # one of the 6^3 boxes in front of the large one
    dirty = [a.copy() for a in arrays]
    dirty[hit][2, 3, 1] = np.nan
    host, _, _ = _run(dirty, "coif1")
    off = np.concatenate([[0], np.cumsum([a.size for a in arrays])])
    other = np.ones(host.shape[1], dtype=bool)
    other[off[hit]:off[hit + 1]] = False
    assert host[:, other].tobytes() == clean[:, other].tobytes()
    assert np.isnan(host[:, ~other]).any()


def test_host_array_twin():
    from pyradiomics_amd import cmatrices
    arrays, want = _single_route("db2", "int16")
    res, names = cmatrices.calculate_wavelet_batch(arrays[:6], wavelet="db2")
    assert list(res) == list(names) == list(want[0])
    for b in range(6):
        for name in names:
            assert res[name][b].shape == arrays[b].shape and res[name][b].tobytes() == want[b][name].tobytes()

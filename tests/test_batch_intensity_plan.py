"""The planner and the argument checks of the batched intensity transforms and Gradient (prad_batch_intensity_plan,
prad_batch_intensity_dev, roi_batch.batch_intensity_plan / intensity_batch / gradient_batch / roi_features_batch_types) --
everything that is answered without a device.  Host buffers stand in for the device pointers; no call of
prad_batch_intensity_dev here gets as far as a launch (never add an all-valid call with B > 0: with a GPU it would run on host
memory)."""
import ctypes as C

import numpy as np
import pytest

IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
OK, ARG, UNSUPPORTED = 1, -1, -4
CHUNK = 1024
# the shapes of tests/test_gpu_batch_intensity.py: odd offsets, rows across the 64-lane width, one box above every LDS cap
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 2, 1), (2, 2, 2), (3, 1, 5), (1, 7, 1), (5, 4, 3), (4, 4, 65), (17, 9, 33),
          (41, 41, 41)]
MANY = [(1, 1, 1), (2, 3, 1)] * 150
ALL = ("Square", "SquareRoot", "Logarithm", "Exponential", "Gradient")
TWO = [(6, 6, 6), (4, 4, 5)]
ZERO = [(6, 6, 6), (4, 0, 5)]


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


def _ip(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.intc).ctypes.data_as(IP)


def _lp(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(LP)


_BUF = np.zeros(4096, dtype=np.float64)      # stands in for every device pointer


def _vp(null, name):
    return None if name in null else C.c_void_p(_BUF.ctypes.data)


def _check(got, want):
    from pyradiomics_amd import _lib
    code, text = want if isinstance(want, tuple) else (want, None)
    assert got == code, (got, _lib.last_error())
    if text is not None:
        assert text in _lib.last_error(), _lib.last_error()
    assert (_BUF == 0).all(), "a buffer was written"


def _coverage(sizes, items):
    """how often the items name every voxel of every box: int [W] (element e of box b is voxel off[b] + e of the batch)"""
    nvox = np.asarray(sizes, dtype=np.int64).reshape(-1, 3).prod(1)
    W = int(nvox.sum())
    start = np.concatenate([[0], np.cumsum(nvox)])
    hits = np.zeros(W, dtype=np.int64)
    for w0, w1, first, last in items:
        assert 0 <= w0 < w1 <= W and w1 - w0 <= CHUNK
        hits[w0:w1] += 1
        # the ROIs of the range's ends, as a lane's bisection between them finds every voxel's box
        assert start[first] <= w0 < start[first + 1], (w0, first)
        assert start[last] <= w1 - 1 < start[last + 1], (w1, last)
    return hits


@pytest.mark.parametrize("sizes", [SHAPES, MANY, SHAPES + MANY, [(41, 41, 41)], [(1, 1, 1)]], ids=["shapes", "many", "both", "one41", "one1"])
@pytest.mark.parametrize("types", [ALL, ("Square", "Exponential"), ("Gradient",), ("Logarithm", "Gradient")],
                         ids=["all", "subset", "gradient", "log+gradient"])
def test_items_cover_every_output_element_once(sizes, types):
    from pyradiomics_amd import roi_batch
    items, grid = roi_batch.batch_intensity_plan(sizes, types)
    hits = _coverage(sizes, items)
    # a workgroup writes its voxels of EVERY requested row: once per voxel is once per output element of every row
    assert (hits == 1).all()
    assert items.shape == ((len(hits) + CHUNK - 1) // CHUNK, 4)
    assert (items[1:, 0] == items[:-1, 1]).all() and items[0, 0] == 0 and items[-1, 1] == len(hits)
    pointwise = any(t != "Gradient" for t in types)
    assert grid.tolist() == [len(sizes) if pointwise else 0, len(items)]          # Gradient alone: ONE launch
    # a plan is a function of its arguments alone
    again, grid2 = roi_batch.batch_intensity_plan(sizes, types)
    assert np.array_equal(again, items) and np.array_equal(grid, grid2)


def test_an_empty_batch_is_an_empty_plan():
    from pyradiomics_amd import roi_batch
    for types in (ALL, ("Gradient",), ("Square",)):
        items, grid = roi_batch.batch_intensity_plan(np.zeros((0, 3), dtype=np.intc), types)
        assert items.shape == (0, 4) and grid.tolist() == [0, 0]


def test_grids_stay_within_the_hip_limits_for_a_billion_voxels(lib):
    """1 000 boxes of 100^3: the grid of either launch stays below 2^31 - 1 workgroups AND below 2^32 lanes of 256"""
    sizes = np.full((1000, 3), 100, dtype=np.intc)
    n = C.c_longlong(-1)
    grid = np.zeros(2, dtype=np.int64)
    assert lib.prad_batch_intensity_plan(_ip(sizes), 1000, 31, C.byref(n), None, grid.ctypes.data_as(LP)) == OK
    assert n.value == (10 ** 9 + CHUNK - 1) // CHUNK == grid[1] and grid[0] == 1000
    for g in grid:
        assert 0 < g <= 2 ** 31 - 1 and g * 256 < 2 ** 32
    # above the limit the planner declines instead of wrapping a grid dimension: 20 boxes of 1024^3 are 2.1e10 voxels
    big = np.full((20, 3), 1024, dtype=np.intc)
    _check(lib.prad_batch_intensity_plan(_ip(big), 20, 31, C.byref(n), None, grid.ctypes.data_as(LP)), (UNSUPPORTED, "workgroups"))


def _plan(lib, sizes=TWO, B=2, types=31, null=()):
    n = C.c_longlong(0)
    grid = np.zeros(2, dtype=np.int64)
    return lib.prad_batch_intensity_plan(None if "sizes" in null else _ip(sizes), B, types, None if "n_items" in null else C.byref(n),
                                         None, None if "grid" in null else grid.ctypes.data_as(LP))


def test_plan_errors(lib):
    _check(_plan(lib, B=-1), (ARG, "B=-1"))
    _check(_plan(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_plan(lib, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    _check(_plan(lib, types=0), (ARG, "types=0"))
    _check(_plan(lib, types=32), (ARG, "types=32"))
    for name in ("n_items", "grid"):
        _check(_plan(lib, null=(name,)), (ARG, "NULL output"))
    _check(_plan(lib), OK)
    _check(_plan(lib, B=0), OK)


def _call(lib, sizes=TWO, B=2, dtype=0, off=(0, 216), types=31, spacing=None, use=1, row_stride=296, null=()):
    sp = np.ascontiguousarray(np.ones((2, 3)) if spacing is None else spacing, dtype=np.float64)
    v = np.zeros(32, dtype=np.intc)
    return lib.prad_batch_intensity_dev(_vp(null, "in"), dtype, None if "sizes" in null else _ip(sizes),
                                        None if "off" in null else _lp(off), B, types,
                                        None if "spacing" in null else C.c_void_p(sp.ctypes.data), use, _vp(null, "out64"), row_stride,
                                        _vp(null, "out_grad"), None if "verdict" in null else v.ctypes.data_as(IP), None)


def test_entry_errors(lib):
    _check(_call(lib, B=-1), (ARG, "B=-1"))
    _check(_call(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_call(lib, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    for name in ("in", "off", "out64", "out_grad", "verdict"):
        _check(_call(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_call(lib, types=0), (ARG, "types=0"))
    _check(_call(lib, types=64), (ARG, "types=64"))
    _check(_call(lib, spacing=[(1, 1, 1), (0, 1, 1)]), (ARG, "ROI 1 has spacing[0]"))
    _check(_call(lib, spacing=[(1, 1, np.inf), (1, 1, 1)]), (ARG, "ROI 0 has spacing[2]"))
    _check(_call(lib, off=(0, -216)), (ARG, "off[1]=-216"))
    _check(_call(lib, off=(0, 215)), (ARG, "off[1]=215 lies before the end of ROI 0 (216)"))      # sizes / buffer mismatch
    _check(_call(lib, off=(300, 0), row_stride=600), (ARG, "off[1]=0"))
    _check(_call(lib, row_stride=295), (ARG, "row_stride=295"))                                   # a row too short for the boxes
    _check(_call(lib, dtype=4), (ARG, "dtype 4"))
    _check(_call(lib, dtype=-1), (ARG, "dtype -1"))
    _check(_call(lib, dtype=7, B=-1), (ARG, "dtype 7"))
    # what a call does not ask for may be NULL -- and B = 0 is a valid call that launches nothing
    _check(_call(lib, B=0, types=16, null=("out64", "spacing")), OK)
    _check(_call(lib, B=0, types=15, null=("out_grad", "spacing")), OK)
    _check(_call(lib, B=0), OK)


def test_python_argument_errors_come_before_any_device_work():
    """host tensors: a call that got as far as the device layer would complain about them instead"""
    import torch
    from pyradiomics_amd import roi_batch
    x = torch.zeros(8)
    with pytest.raises(ValueError, match="types must be a non-empty subset"):
        roi_batch.intensity_batch(x, [(2, 2, 2)], types=("Square", "Cube"))
    with pytest.raises(ValueError, match="types must be a non-empty subset"):
        roi_batch.intensity_batch(x, [(2, 2, 2)], types=())
    with pytest.raises(ValueError, match="types must be a non-empty subset"):
        roi_batch.intensity_batch(x, [(2, 2, 2)], types=("Gradient",))          # (gradient_batch is its own call)
    with pytest.raises(ValueError, match="types must be a non-empty subset"):
        roi_batch.batch_intensity_plan([(2, 2, 2)], ("Sqare",))
    with pytest.raises(ValueError, match="sizes describe 12 voxels, the buffer holds 8"):
        roi_batch.intensity_batch(x, [(2, 2, 3)])
    with pytest.raises(ValueError, match="sizes describe 12 voxels, the buffer holds 8"):
        roi_batch.gradient_batch(x, [(2, 2, 3)])
    with pytest.raises(ValueError, match="needs `sizes`"):
        roi_batch.gradient_batch(x)
    for bad in (torch.zeros((4, 8), dtype=torch.float32), torch.zeros((3, 8), dtype=torch.float64),
                torch.zeros((4, 7), dtype=torch.float64), torch.zeros(32, dtype=torch.float64),
                torch.zeros((4, 16), dtype=torch.float64)[:, ::2], torch.zeros((8, 4), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match="out must be a torch.float64"):
            roi_batch.intensity_batch(x, [(2, 2, 2)], out=bad)
    with pytest.raises(ValueError, match="out must be a torch.float64"):
        roi_batch.intensity_batch(x, [(2, 2, 2)], types=("Square",), out=torch.zeros((2, 8), dtype=torch.float64))
    for bad in (torch.zeros(8, dtype=torch.float64), torch.zeros(9, dtype=torch.float32), torch.zeros((1, 8), dtype=torch.float32),
                torch.zeros(16, dtype=torch.float32)[::2]):
        with pytest.raises(ValueError, match="out must be a torch.float32"):
            roi_batch.gradient_batch(x, [(2, 2, 2)], out=bad)
    with pytest.raises(ValueError):
        roi_batch.batch_intensity_plan([(2, 0, 2)])
    # a good `out` passes these checks: the call gets as far as asking for device tensors
    with pytest.raises(ValueError, match="expects CUDA/HIP tensors"):
        roi_batch.intensity_batch(x, [(2, 2, 2)], out=torch.zeros((4, 8), dtype=torch.float64))


def test_image_types_of_the_table_calls():
    """roi_features_batch_types takes all eight image types and rejects any other name; the three older functions keep raising
    for the five new ones (before anything touches a device)"""
    import torch
    from pyradiomics_amd import engine, roi_batch
    assert engine.roi_features_batch_types is roi_batch.roi_features_batch_types
    assert engine.intensity_batch is roi_batch.intensity_batch and engine.gradient_batch is roi_batch.gradient_batch
    x = torch.zeros(8)
    with pytest.raises(NotImplementedError, match="'Cube' is not an image type"):
        roi_batch.roi_features_batch_types(x, x, [(2, 2, 2)], imageTypes={"Square": {}, "Cube": {}})
    every = {"Original": {}, "Wavelet": {}, "LoG": {"sigma": [1.0]}, "Square": {}, "SquareRoot": {}, "Logarithm": {},
             "Exponential": {}, "Gradient": {}}
    with pytest.raises(ValueError, match="expects CUDA/HIP tensors"):          # accepted: the call gets as far as the device layer
        roi_batch.roi_features_batch_types(x, x, [(2, 2, 2)], imageTypes=every)
    for t in ("Square", "SquareRoot", "Logarithm", "Exponential", "Gradient"):
        with pytest.raises(NotImplementedError, match=t):
            roi_batch.roi_features_batch_images(x, x, [(2, 2, 2)], imageTypes={"Original": {}, t: {}})
        with pytest.raises(NotImplementedError, match=t):
            roi_batch.roi_features_batch_derived(x, x, [(2, 2, 2)], imageTypes={"Original": {}, t: {}})
    # (roi_features_batch_resampled resamples on the device before it looks at the types: tests/test_gpu_batch_intensity.py)

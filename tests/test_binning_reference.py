"""CPU: pins tests/binning_reference.py -- its two level counters to each other and to np.digitize, its restated fixed-count
edges to np.histogram bit for bit, its fixed-width edges to imageoperations.getBinEdges -- and checks the host route
(getBinEdges / binImage) where NumPy scalars of an integer pixel type used to wrap.  Every comparison is an equality."""
import warnings

import numpy as np
import pytest

import binning_reference as br
from pyradiomics_amd import imageoperations

SMALL = br.VALUES + br.COUNTS


def _edges_of(c):
    lo, hi = br.minmax_exact(c["x"], c["mask"])
    if c["kw"].get("binCount") is not None:
        return np.asarray(br.edges_count_restated(lo, hi, c["kw"]["binCount"], c["x"].dtype), dtype=np.float64)
    return np.asarray(br.edges_width_exact(lo, hi, c["kw"]["binWidth"], c["x"].dtype), dtype=np.float64)


def _all_small():
    for name in SMALL:
        yield name, br.case(name)
    for ne in br.TIER_EDGES:
        yield "tier-%d" % ne, br.tier_case(ne, "int16")
    for N in br.TIER_COUNTS:
        yield "tier-count-%d" % N, br.tier_case(N + 1, "float32", count=N)


def test_scan_sizes_are_those_of_the_launch_geometry():
    assert br.NTHREADS == 262144
    assert [br.scan_n(d) for d in ("float64", "float32", "int32", "int16")] == [1574865, 3149731, 3149731, 6299463]
    for d in br.DTYPES:
        E, n = br.vector_elems(d), br.scan_n(d)
        nvec = n // E
        assert nvec > 3 * br.NTHREADS and nvec - 3 * br.NTHREADS == 1000 and n % E == E - 1 and n % 8 != 0
        pos = br.scan_positions(d)
        assert len(set(pos.values())) == 5 and pos["tail"] >= nvec * E


def test_brute_force_searchsorted_and_digitize_agree():
    seen = 0
    for name, c in _all_small():
        edges = _edges_of(c)
        v = c["x"][c["mask"]].astype(np.float64)
        fast = br.levels_sorted(v, edges)
        assert np.array_equal(fast, np.digitize(v, edges)), name
        if len(v) * len(edges) <= br.BRUTE_LIMIT:
            assert np.array_equal(br.levels_brute(v, edges), fast), name
            seen += 1
        lv = br.levels_exact(c["x"], c["mask"], edges)
        assert lv.shape == c["x"].shape and not lv[~c["mask"]].any() and lv[c["mask"]].min() >= 1, name
        cnt = br.counts_exact(lv, c["mask"], int(lv.max()) + 1)
        assert cnt[0] == 0 and cnt.sum() == int(c["mask"].sum()), name
    assert seen >= len(SMALL) - 2                  # (only the 10^6-edge cases are beyond the brute-force limit)
    # both counters on either side of the switch
    rng = np.random.default_rng(3)
    e = np.sort(rng.standard_normal(1000))
    v = np.concatenate((e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), rng.standard_normal(5000)))
    assert np.array_equal(br.levels_brute(v, e), br.levels_sorted(v, e))


def test_cases_hold_what_their_names_say():
    c = br.case("w25-i16-neg")
    lo, hi = br.minmax_exact(c["x"], c["mask"])
    assert (lo, hi) == (-1013.0, 1207.0) and _edges_of(c)[0] == -1025.0
    for name in ("w0.1-f64", "w0.1-f32", "w1/3-f64", "w0.37-f32", "w2^-20-f64", "onedge-f64", "outlier-f32"):
        c = br.case(name)
        edges, v = _edges_of(c), c["x"][c["mask"]].astype(np.float64)
        inner = edges[(edges > v.min()) & (edges < v.max())]
        on = np.isin(inner, v).mean()
        below = np.array([(v < e).any() and v[v < e].max() >= np.nextafter(np.float32(e), np.float32(-np.inf)) for e in inner])
        above = np.array([v[v > e].min() <= np.nextafter(np.float32(e), np.float32(np.inf)) for e in inner])
        assert below.all() and above.all(), name
        if c["x"].dtype == np.float64:
            assert on == 1.0, name
    assert br.case("edges1e6-f64")["nedges"] == 2 ** 20 + 2 and br.case("edges1e6-f32")["nedges"] >= 10 ** 6
    assert br.minmax_exact(np.array([0.0, -0.0, 0.0]), np.ones(3, bool)) == (0.0, 0.0)
    lo, hi = br.minmax_exact(np.array([0.0, -0.0, 7.0]), np.array([1, 1, 0]))
    assert np.signbit(lo) and not np.signbit(hi) and (lo, hi) == (0.0, 0.0)
    lo, hi = br.minmax_exact(np.array([-0.0, -0.0, -1.0]), np.array([1, 1, 0]))
    assert np.signbit(lo) and np.signbit(hi)
    for name in ("f32-2^24", "f32-2^24-odd"):
        c = br.case(name)
        assert br.expected(c["x"], c["mask"], c["kw"])[1] == c["kw"]["binCount"] + 1 == c["Ng"]


def _numpy_count_edges(v, N):
    e = np.histogram(v, N)[1]
    e[-1] += 1
    return e


def test_restated_fixed_count_edges_are_np_histograms_bit_for_bit():
    for name, c in _all_small():
        N = c["kw"].get("binCount")
        if N is None:
            continue
        v = c["x"][c["mask"]]
        lo, hi = br.minmax_exact(c["x"], c["mask"])
        want = _numpy_count_edges(v, N)
        got = br.edges_count_restated(lo, hi, N, v.dtype)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), name
        assert br.strictly_ascending_before_shift(lo, hi, N, v.dtype), name
    rng = np.random.default_rng(23)
    for trial in range(300):
        dt = np.dtype(("float32", "float64", "int16", "int32")[trial % 4])
        scale = 10.0 ** rng.uniform(-5, 8)
        lo, hi = np.sort(rng.standard_normal(2) * scale + rng.uniform(-3, 3) * scale)
        if dt.kind == "i":
            lo, hi = np.clip([np.round(lo), np.round(hi)], np.iinfo(dt).min, np.iinfo(dt).max)
        lo, hi = dt.type(lo), dt.type(hi)
        N = int(rng.choice([1, 2, 3, 7, 32, 100, 255, 1000, 4096]))
        if not hi > lo:
            continue
        try:
            want = _numpy_count_edges(np.array([lo, hi, lo]), N)
        except ValueError:
            assert not br.strictly_ascending_before_shift(lo, hi, N, dt), trial
            continue
        got = br.edges_count_restated(lo, hi, N, dt)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (trial, dt, N)


@pytest.mark.parametrize("name", br.DUPLICATE)
def test_edges_that_are_not_strictly_ascending(name):
    """64 ulps cut into 4096 bins: linspace's edges repeat.  NumPy >= 2.1 raises for them; where it answers, the answer is the
    restated one"""
    c = br.case(name)
    v = c["x"][c["mask"]]
    lo, hi = br.minmax_exact(c["x"], c["mask"])
    got = br.edges_count_restated(lo, hi, 4096, v.dtype)
    assert len(np.unique(got[:-1])) < 4096 and not br.strictly_ascending_before_shift(lo, hi, 4096, v.dtype)
    try:
        want = _numpy_count_edges(v, 4096)
    except ValueError:
        return
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", br.RAISING)
def test_ranges_np_histogram_declines(name):
    c = br.case(name)
    lo, hi = br.minmax_exact(c["x"], c["mask"])
    assert br.edges_count_restated(lo, hi, c["kw"]["binCount"], c["x"].dtype) is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError):
            imageoperations.getBinEdges(c["x"][c["mask"]], **c["kw"])


@pytest.mark.parametrize("dtype", ["int16", "int32", "float32", "float64"])
def test_constant_roi_fixed_count_edges(dtype):
    for value, N in ((3, 8), (-70, 1), (0, 20)):
        want = _numpy_count_edges(np.full(5, value, dtype=dtype), N)
        got = br.constant_count_edges(value, N, dtype)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- getBinEdges: integer pixel types --------------------------------------------------------------------------------------
def _parent_width_edges(values, binWidth):
    """the fixed-width branch as it stood before the extremes of integer images became Python integers: NumPy scalars of the
    pixel type throughout.  Raises where that arithmetic wraps."""
    with warnings.catch_warnings(), np.errstate(over="raise"):
        warnings.simplefilter("error")
        lo = min(values)
        hi = max(values)
        first = lo - (lo % binWidth)
        edges = np.arange(first, hi + 2 * binWidth, binWidth)
        if len(edges) == 1:
            edges = [edges[0] - 0.5, edges[0] + 0.5]
        return edges


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


OVERFLOW_POINTS = [
    ("uint8", 3, 250, 25), ("uint8", 0, 255, 25), ("uint8", 200, 231, 13), ("uint8", 255, 255, 1),
    ("int8", -128, 127, 25), ("int8", -128, -128, 25), ("int8", 100, 127, 16), ("int8", -127, 3, 5),
    ("uint16", 0, 65535, 25), ("uint16", 65500, 65501, 25), ("uint16", 7, 65486, 25),
    ("int16", -5, 32760, 25), ("int16", -32768, 0, 25), ("int16", -32768, 32767, 25), ("int16", 32767, 32767, 25),
    ("int16", -32768, -32768, 25), ("int16", 32718, 32718, 25), ("int16", 0, 32767, 1000),
    ("int32", -2 ** 31, 2 ** 31 - 1, 2 ** 24), ("int32", 2 ** 31 - 60, 2 ** 31 - 1, 25), ("int32", -2 ** 31, -2 ** 31 + 90, 25),
]


@pytest.mark.parametrize("dtype,lo,hi,w", OVERFLOW_POINTS)
def test_fixed_width_edges_where_the_pixel_type_would_wrap(dtype, lo, hi, w):
    values = np.array([lo, hi, lo], dtype=dtype)
    got = imageoperations.getBinEdges(values, binWidth=w)
    want = br.edges_width_exact(lo, hi, w, dtype)
    assert _same(got, want), (got, want)
    e = np.asarray(got, dtype=np.float64)
    assert len(e) >= 2 and e[0] <= lo < e[0] + w and e[-1] > hi and e[-2] <= hi + w and np.all(np.diff(e) == w)
    assert np.digitize(values, e).min() == 1


def test_fixed_width_edges_sweep_equals_the_former_arithmetic_where_it_did_not_wrap():
    rng = np.random.default_rng(1709)
    same = wrapped = 0
    for trial in range(3000):
        dt = np.dtype(("uint8", "int8", "uint16", "int16", "int32", "bool", "int64", "float32", "float64")[trial % 9])
        w = (25, 1, 7, 0.37, 2.5, 1000, np.float64(0.1), np.int64(3), 16)[int(rng.integers(0, 9))]
        if dt.kind == "f":
            scale = 10.0 ** rng.uniform(-2, 4)
            lo, hi = np.sort((rng.standard_normal(2) * scale).astype(dt))
            w = float(w) * 10.0 ** int(rng.integers(-2, 2)) if rng.random() < 0.5 else w
        elif dt.kind == "b":
            lo, hi = np.sort(rng.integers(0, 2, size=2).astype(bool))
        else:
            info = np.iinfo(dt)
            if rng.random() < 0.5:                           # anywhere in the type's range, the ends included
                lo, hi = sorted(int(v) for v in rng.integers(info.min, info.max, size=2, endpoint=True, dtype=np.int64))
            else:
                lo = int(rng.integers(max(info.min, -3000), min(info.max, 3000), endpoint=True))
                hi = min(info.max, lo + int(rng.integers(0, 4000)))
            if (hi - lo) / float(w) > 2e5:                   # keep the edge arrays small
                hi = lo + int(float(w) * int(rng.integers(0, 2000)))
                hi = min(hi, info.max)
        values = np.array([lo, hi], dtype=dt)
        got = imageoperations.getBinEdges(values, binWidth=w)
        assert _same(got, br.edges_width_exact(values[0], values[1], w, dt)), (trial, dt, lo, hi, w)
        try:
            parent = _parent_width_edges(values, w)
        except (FloatingPointError, RuntimeWarning, OverflowError):
            wrapped += 1
            assert dt.kind in br.INT_KINDS
            continue
        assert _same(got, parent), (trial, dt, lo, hi, w, got, parent)
        same += 1
    assert same >= 1709 and wrapped >= 20, (same, wrapped)


@pytest.mark.parametrize("name", ["u8-range", "i16-saturated", "i16-lowest", "w25-i32-neg", "w25-i16-neg"])
def test_bin_image_on_integer_images_near_the_ends_of_their_type(name):
    c = br.case(name)
    x, mask = c["x"].reshape(1, -1), c["mask"].reshape(1, -1)
    levels, Ng, edges, counts = br.expected(x, mask, c["kw"])
    got, got_edges = imageoperations.binImage(x, mask, **c["kw"])
    assert np.array_equal(got, levels) and np.array_equal(np.asarray(got_edges, dtype=np.float64), edges)
    assert got[mask].min() == 1 and int(got.max()) == Ng and counts[0] == 0 and counts.sum() == mask.sum()
    whole, _ = imageoperations.binImage(np.where(mask, x, x[mask][0]), **c["kw"])           # no coordinates: the whole array
    assert np.array_equal(whole[mask], levels[mask])
    if name == "u8-range":
        assert len(edges) == 12 and Ng == 11
    if name == "i16-saturated":
        assert edges[0] == -1000 and edges[-1] == 32800 and Ng == len(edges) - 2 == 1351

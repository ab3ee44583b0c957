"""TEST INFRASTRUCTURE ONLY -- the exact reference of grey-level discretisation (csrc/kernels_binning.h, prad_binning.hip,
imageoperations.getBinEdges / binImage), plain numpy and Python, its own code, no device.

Discretisation is exact arithmetic: the level of a voxel is the number of float64 edges <= its value widened to float64
(np.digitize with ascending edges), 0 outside the ROI.  int16, int32, float32 and float64 widen to float64 without rounding, so
the reference is exact, not merely precise, and every comparison made with it is an equality.

  levels_exact(x, mask, edges)        brute force (#edges <= v, counted) up to BRUTE_LIMIT comparisons, np.searchsorted beyond;
                                      tests/test_binning_reference.py pins the two to each other and to np.digitize
  counts_exact(levels, mask, nbins)   ROI voxels per level, int64 [nbins]
  minmax_exact(x, mask)               ROI extremes as float64; -0.0 orders below +0.0 (the kernel orders by a bit key)
  edges_width_exact(lo, hi, w, dtype) the intended fixed-width edges: first = lo - lo % w, arange(first, hi + 2 w, w), in Python
                                      integers for integer (and bool) pixel types -- nothing can wrap --, in NumPy scalars of
                                      the pixel type for float types, as the reference package does; a single edge e becomes
                                      [e - 0.5, e + 0.5]
  edges_count_restated(lo, hi, N, dtype)
                                      np.histogram(x, N)[1] with its last edge moved up by 1, written out: np.linspace's two
                                      roundings i * step, then + lo, the last edge = hi, then + 1 -- all in float32 for a float32
                                      image (NumPy >= 2), in float64 otherwise.  None where np.linspace takes another branch
                                      (constant or non-finite range, step == 0).

Case tables (names; case(name) builds the arrays, deterministic): VALUES, COUNTS, RAISING, TIERS_WIDTH, TIERS_COUNT.
A case is a dict: x (array), mask (bool array), kw (binWidth / binCount), plus what its family needs.
"""
import numpy as np

BRUTE_LIMIT = 10 ** 8
INT_KINDS = "biu"

# launch geometry of the scans (prad_binning.hip): 256 threads, grids of min(ceil(n / 256), cap) blocks
DIGITIZE_CAP, MINMAX_CAP, BLOCK = 1024, 512, 256
NTHREADS = DIGITIZE_CAP * BLOCK                      # 262144: digitize_kernel and level_counts_kernel at their cap
NTHREADS_MINMAX = MINMAX_CAP * BLOCK                 # 131072: roi_minmax_kernel at its cap
DTYPES = ("int16", "int32", "float32", "float64")


def vector_elems(dtype):
    """E: elements per 16-byte load"""
    return 16 // np.dtype(dtype).itemsize


def scan_n(dtype):
    """the smallest-style size at which some digitize threads run the four-deep loop (vectors t, t + T, t + 2T, t + 3T for
    t < 1000; it starts at nvec > 3 T), the others the one-vector loop, and E - 1 elements stay for the scalar tail"""
    E = vector_elems(dtype)
    return E * (3 * NTHREADS + 1000) + (E - 1)


# ---- the reference proper -----------------------------------------------------------------------------------------------
def levels_brute(v, edges):
    """#{edges <= v} per value, counted; v and edges float64 1-D"""
    out = np.empty(len(v), dtype=np.int64)
    chunk = max(1, (1 << 22) // max(1, len(edges)))
    for a in range(0, len(v), chunk):
        out[a:a + chunk] = (edges[None, :] <= v[a:a + chunk, None]).sum(1)
    return out


def levels_sorted(v, edges):
    return np.searchsorted(edges, v, side="right").astype(np.int64)


def levels_exact(x, mask, edges):
    x = np.asarray(x)
    mask = np.asarray(mask).astype(bool)
    edges = np.asarray(edges, dtype=np.float64)
    assert np.all(edges[1:] >= edges[:-1]) and not np.isnan(edges).any()
    v = x[mask].astype(np.float64)
    assert not np.isnan(v).any()
    out = np.zeros(x.shape, dtype=np.int64)
    out[mask] = levels_brute(v, edges) if len(v) * len(edges) <= BRUTE_LIMIT else levels_sorted(v, edges)
    return out


def counts_exact(levels, mask, nbins):
    lv = np.asarray(levels)[np.asarray(mask).astype(bool)]
    assert lv.size == 0 or (lv.min() >= 0 and lv.max() < nbins)
    return np.bincount(lv, minlength=nbins).astype(np.int64)


def minmax_exact(x, mask):
    v = np.asarray(x)[np.asarray(mask).astype(bool)].astype(np.float64)
    assert v.size and not np.isnan(v).any()
    lo, hi = float(v.min()), float(v.max())
    zeros = v[v == 0]
    if lo == 0:
        lo = -0.0 if np.signbit(zeros).any() else 0.0
    if hi == 0:
        hi = 0.0 if (~np.signbit(zeros)).any() else -0.0
    return lo, hi


def edges_width_exact(lo, hi, binWidth, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind in INT_KINDS:
        lo, hi = int(lo), int(hi)
    else:
        lo, hi = dtype.type(lo), dtype.type(hi)
    first = lo - (lo % binWidth)
    edges = np.arange(first, hi + 2 * binWidth, binWidth)
    if len(edges) == 1:
        edges = [edges[0] - 0.5, edges[0] + 0.5]
    return edges


def edges_count_restated(lo, hi, N, dtype):
    ft = np.float32 if np.dtype(dtype) == np.float32 else np.float64
    lo, hi = ft(lo), ft(hi)
    with np.errstate(all="ignore"):
        delta = hi - lo
        step = delta / ft(N)
    if not (hi > lo) or not np.isfinite(delta) or step == 0:
        return None
    i = np.arange(N + 1).astype(ft)
    e = i * step                                   # one rounding
    e = e + lo                                     # the second
    e[N] = hi
    e[N] = e[N] + ft(1)
    assert e.dtype == ft
    return e


def strictly_ascending_before_shift(lo, hi, N, dtype):
    """np.histogram (NumPy >= 2.1) refuses edges that are not strictly ascending, before getBinEdges moves the last one"""
    e = edges_count_restated(lo, hi, N, dtype).copy()
    e[N] = (np.float32 if e.dtype == np.float32 else np.float64)(hi)
    return bool(np.all(e[:-1] < e[1:]))


def expected(x, mask, kw):
    """(levels int64, Ng, edges float64, counts int64 [Ng + 1]) of binImage on the ROI, from the functions above alone"""
    x = np.asarray(x)
    lo, hi = minmax_exact(x, mask)
    if kw.get("binCount") is not None:
        edges = edges_count_restated(lo, hi, int(kw["binCount"]), x.dtype)
        assert edges is not None, "constant ROI: np.histogram widens the range, see expected_constant_count"
    else:
        edges = edges_width_exact(lo, hi, kw.get("binWidth", 25), x.dtype)
    edges = np.asarray(edges, dtype=np.float64)
    levels = levels_exact(x, mask, edges)
    Ng = int(levels.max())
    return levels, Ng, edges, counts_exact(levels, mask, Ng + 1)


def constant_count_edges(value, N, dtype):
    """np.histogram on a constant ROI widens the range to value -+ 0.5 (its _get_outer_edges), then linspace and the +1"""
    ft = np.float32 if np.dtype(dtype) == np.float32 else np.float64
    e = edges_count_restated(ft(value) - ft(0.5), ft(value) + ft(0.5), N, ft)
    return e


# ---- case tables ----------------------------------------------------------------------------------------------------------
def _neighbours(edges, dtype, lo, hi):
    """every edge and its two neighbours in the image's own type, kept inside [lo, hi]; for float32 the roundings on both sides
    of each float64 edge (the nearest float32 and ITS two neighbours cover them)"""
    dtype = np.dtype(dtype)
    e = np.asarray(edges, dtype=np.float64)
    if dtype.kind in INT_KINDS:
        c = np.round(e).astype(np.int64)
        v = np.concatenate((c - 1, c, c + 1))
    else:
        c = e.astype(dtype)
        v = np.concatenate((np.nextafter(c, dtype.type(-np.inf)), c, np.nextafter(c, dtype.type(np.inf))))
    v = v[(v >= lo) & (v <= hi)]
    return np.concatenate(([lo, hi], v)).astype(dtype)


def _width_case(lo, hi, w, dtype, every=1, seed=0):
    dtype = np.dtype(dtype)
    lo, hi = dtype.type(lo), dtype.type(hi)
    edges = np.asarray(edges_width_exact(lo, hi, w, dtype), dtype=np.float64)
    x = _neighbours(edges[::every], dtype, lo, hi)
    rng = np.random.default_rng(seed)
    x = x[rng.permutation(len(x))]
    mask = np.ones(len(x), dtype=bool)
    # a few voxels outside the ROI holding values beyond both ends: they must not move the extremes nor get a level
    out = np.array([lo, hi, lo, hi], dtype=dtype)
    if dtype.kind == "f":
        out = (out.astype(np.float64) + np.array([-7.5, 7.5, -1e3, 1e3])).astype(dtype)
    else:
        out = np.clip(out.astype(np.int64) + np.array([-3, 3, -100, 100]), np.iinfo(dtype).min, np.iinfo(dtype).max).astype(dtype)
    x = np.concatenate((x[:5], out[:2], x[5:], out[2:]))
    mask = np.concatenate((mask[:5], [False, False], mask[5:], [False, False]))
    return dict(x=x, mask=mask, kw=dict(binWidth=w), nedges=len(edges))


VALUES = ("w0.1-f64", "w0.1-f32", "w1/3-f64", "w1/3-f32", "w0.37-f64", "w0.37-f32", "w25-i16-neg", "w25-i32-neg",
          "w2^-20-f64", "edges1e6-f64", "edges1e6-f32", "negzero-f64", "negzero-f32", "const-on-i16", "const-off-i16",
          "const-on-f64", "const-off-f32", "u8-range", "i16-saturated", "i16-lowest")

COUNTS = ("n1-f64", "n1-i16", "n4096-f64", "n4096-i32", "n4097-f64", "n4097-i16", "outlier-f64", "outlier-f32", "f32-2^24",
          "f32-2^24-odd", "onedge-f64", "onedge-i16", "negzero-count-f64", "tiny-f64")

# fixed-count requests np.histogram answers with a ValueError on every NumPy (the host route's error, whichever route is asked)
RAISING = ("denormal-step", "overflowing-range")

# requests whose linspace edges are not strictly ascending: NumPy >= 2.1 raises, earlier ones return the duplicate edges
DUPLICATE = ("dup-f32-64ulp", "dup-f64-64ulp")

# nedges thresholds of launch_digitize (quoted in tests/test_gpu_binning_limits.py)
TIER_EDGES = (48, 49, 2730, 2731, 7680, 7681)
TIER_COUNTS = (47, 48, 2729, 2730)                   # binCount N gives N + 1 edges; 4096 is the most the device builds
TIER_SHAPE = (7, 19, 61)                             # 8113 voxels, no multiple of 8 (nor of 2)

_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("w0.1"):
        return _width_case(0.05, 40.05, 0.1, "float64" if name.endswith("f64") else "float32")
    if name.startswith("w1/3"):
        return _width_case(-7.25, 21.0, 1.0 / 3.0, "float64" if name.endswith("f64") else "float32")
    if name.startswith("w0.37"):
        return _width_case(-100.3, 117.77, 0.37, "float64" if name.endswith("f64") else "float32")
    if name == "w25-i16-neg":
        return _width_case(-1013, 1207, 25, "int16")              # Python modulo: -1013 % 25 == 12, first edge -1025
    if name == "w25-i32-neg":
        return _width_case(-2 ** 31 + 7, -2 ** 31 + 4000, 25, "int32")
    if name == "w2^-20-f64":
        return _width_case(1e6, 1e6 + 300 * 2.0 ** -20, 2.0 ** -20, "float64")
    if name == "edges1e6-f64":                                    # 1 048 578 edges, searched in global memory
        return _width_case(1e6, 1e6 + 1, 2.0 ** -20, "float64", every=997)
    if name == "edges1e6-f32":                                    # the 17 float32 values of [1e6, 1e6 + 1] against them
        return _width_case(1e6, 1e6 + 1, 2.0 ** -20, "float32", every=4099)
    if name.startswith("negzero") and "count" not in name:       # an edge at 0.0; -0.0 == 0.0 belongs to the bin above it
        dt = np.dtype("float64" if name.endswith("f64") else "float32")
        tiny = np.nextafter(dt.type(0), dt.type(1))
        x = np.array([-0.0, 0.0, -tiny, tiny, -1.5, 1.5, -0.0, 0.5, -0.5, 0.0, -0.0], dtype=dt)
        mask = np.ones(len(x), dtype=bool)
        mask[-1] = False
        return dict(x=x, mask=mask, kw=dict(binWidth=0.5))
    if name.startswith("const"):
        dt = np.dtype({"i16": "int16", "f64": "float64", "f32": "float32"}[name[-3:]])
        value = {"const-on-i16": 50, "const-off-i16": -51, "const-on-f64": 0.74, "const-off-f32": 0.5}[name]
        w = 25 if dt.kind == "i" else 0.37
        x = np.full(37, value, dtype=dt)
        mask = rng.random(37) < 0.7
        mask[0] = True
        x[~mask] = dt.type(3)
        return dict(x=x, mask=mask, kw=dict(binWidth=w))
    if name == "u8-range":                                        # 250 + 2 * 25 wraps in uint8
        x = rng.integers(3, 251, size=301).astype(np.uint8)
        x[:2] = 3, 250
        return dict(x=x, mask=np.ones(301, dtype=bool), kw=dict(binWidth=25))
    if name == "i16-saturated":                                   # 32767 + 50 wraps in int16 (CT with metal)
        x = rng.integers(-1000, 3000, size=301).astype(np.int16)
        x[:3] = -5, 32760, 32767
        return dict(x=x, mask=np.ones(301, dtype=bool), kw=dict(binWidth=25))
    if name == "i16-lowest":                                      # -32768 - (-32768 % 25) wraps in int16
        x = rng.integers(-32768, -32000, size=301).astype(np.int16)
        x[:2] = -32768, -32001
        return dict(x=x, mask=np.ones(301, dtype=bool), kw=dict(binWidth=25))
    # ---- fixed count ----
    if name in ("n1-f64", "n4096-f64", "n4097-f64"):
        x = rng.standard_normal(3001) * 37.0 + 5.0
        return dict(x=x, mask=rng.random(3001) < 0.8, kw=dict(binCount=int(name[1:-4])))
    if name in ("n1-i16", "n4097-i16"):
        x = rng.integers(-900, 2500, size=3001).astype(np.int16)
        return dict(x=x, mask=rng.random(3001) < 0.8, kw=dict(binCount=int(name[1:-4])))
    if name == "n4096-i32":
        x = rng.integers(-2 ** 31, 2 ** 31 - 1, size=3001).astype(np.int32)
        x[:2] = -2 ** 31, 2 ** 31 - 1
        return dict(x=x, mask=np.ones(3001, dtype=bool), kw=dict(binCount=4096))
    if name.startswith("outlier"):
        # a range far below 1: the last edge hi + 1 is an outlier among the others, the arithmetic first guess of the kernel
        # (level ~ (v - e0) (nedges - 1) / (elast - e0)) says level 1 for every voxel and the comparisons have to walk
        dt = np.dtype("float64" if name.endswith("f64") else "float32")
        N = 200
        lo, hi = dt.type(0.25), dt.type(0.25 + 1.0 / 1024)
        e = edges_count_restated(lo, hi, N, dt)
        x = _neighbours(e[:-1], dt, lo, hi)
        return dict(x=x, mask=np.ones(len(x), dtype=bool), kw=dict(binCount=N))
    if name == "f32-2^24":                                        # hi + 1 == hi in float32: the maximum lands in level N + 1
        x = (np.float32(2 ** 24) + 2 * rng.integers(0, 33, size=500)).astype(np.float32)
        x[:2] = 2.0 ** 24, 2.0 ** 24 + 64
        return dict(x=x, mask=np.ones(500, dtype=bool), kw=dict(binCount=4), Ng=5)
    if name == "f32-2^24-odd":
        x = (np.float32(-2 ** 25) + 4 * rng.integers(0, 1000, size=500)).astype(np.float32)
        x[:2] = -2.0 ** 25, 2.0 ** 25
        return dict(x=x, mask=np.ones(500, dtype=bool), kw=dict(binCount=7), Ng=8)
    if name == "onedge-f64":                                      # edges i / 8 exactly; voxels on them and one ulp beside
        e = edges_count_restated(-2.0, 2.0, 32, np.float64)
        x = _neighbours(e[:-1], np.float64, -2.0, 2.0)
        return dict(x=x, mask=np.ones(len(x), dtype=bool), kw=dict(binCount=32))
    if name == "onedge-i16":
        x = np.arange(-160, 161, dtype=np.int16)
        return dict(x=x, mask=np.ones(len(x), dtype=bool), kw=dict(binCount=32))
    if name == "negzero-count-f64":
        x = np.array([-0.0, 0.0, -1.0, 1.0, 0.0, -0.0, 0.5, -0.5])
        return dict(x=x, mask=np.ones(8, dtype=bool), kw=dict(binCount=2))
    if name == "tiny-f64":                                        # denormal extremes with a step that does not underflow
        x = np.array([0.0, 5e-324 * 64, 5e-324 * 3, 5e-324 * 32, 5e-324 * 33])
        return dict(x=x, mask=np.ones(5, dtype=bool), kw=dict(binCount=2))
    if name == "denormal-step":
        return dict(x=np.array([0.0, 5e-324, 0.0]), mask=np.ones(3, dtype=bool), kw=dict(binCount=4))
    if name == "overflowing-range":
        return dict(x=np.array([-1e308, 1e308, 0.0]), mask=np.ones(3, dtype=bool), kw=dict(binCount=4))
    if name.startswith("dup"):                                    # 64 ulps cut into 4096 bins
        dt = np.dtype("float32" if "f32" in name else "float64")
        lo = dt.type(1.0)
        x = lo + np.arange(65).astype(dt) * np.spacing(lo)
        assert x[-1] > x[0] and len(np.unique(x)) == 65
        return dict(x=x, mask=np.ones(65, dtype=bool), kw=dict(binCount=4096))
    raise KeyError(name)


def tier_case(nedges, dtype, count=None):
    """a 7 x 19 x 61 image with every level occupied.  binWidth 1 on a ramp 0..M gives M + 2 edges (count None); with
    `count` = N the request is binCount=N on 0..8 N, whose N + 1 edges are the multiples of 8 (and 8 N + 1)"""
    key = ("tier", nedges, dtype, count)
    if key not in _cache:
        rng = np.random.default_rng(nedges + (count or 0))
        n = int(np.prod(TIER_SHAPE))
        if count is None:
            M = nedges - 2
            x = rng.integers(0, M + 1, size=n)
            x[:M + 1] = np.arange(M + 1)
            kw = dict(binWidth=1)
        else:
            assert nedges == count + 1
            M = count
            x = rng.integers(0, 8 * M + 1, size=n)
            x[:M] = 8 * np.arange(M) + rng.integers(0, 8, size=M)
            x[M], x[M + 1] = 0, 8 * M
            kw = dict(binCount=count)
        assert M + 2 <= n
        mask = rng.random(n) < 0.8
        mask[:M + 2] = True
        p = rng.permutation(n)
        _cache[key] = dict(x=x[p].astype(dtype).reshape(TIER_SHAPE), mask=mask[p].reshape(TIER_SHAPE), kw=kw, nedges=nedges)
    return _cache[key]


def scan_case(dtype, n=None):
    """a flat array of scan_n(dtype) values (or n) with a mask of about 0.8.  Voxels 25 apart around +-1200, so binWidth 25 gives
    about a hundred levels; the first and the last element are in the ROI"""
    n = scan_n(dtype) if n is None else n
    key = ("scan", np.dtype(dtype).name, n)
    if key not in _cache:
        rng = np.random.default_rng(n % 100003)
        dt = np.dtype(dtype)
        if dt.kind == "f":
            x = (rng.standard_normal(n) * 400.0).astype(dt)
            x = np.clip(x, -1200, 1200).astype(dt)
        else:
            x = rng.integers(-1200, 1201, size=n).astype(dt)
        mask = rng.random(n) < 0.8
        mask[0] = mask[-1] = True
        _cache[key] = dict(x=x, mask=mask, kw=dict(binWidth=25))
    return _cache[key]


def scan_positions(dtype):
    """where the min/max tests plant an extreme at n = scan_n(dtype): name -> flat index"""
    E, n = vector_elems(dtype), scan_n(dtype)
    nvec = n // E
    assert nvec == 3 * NTHREADS + 1000 and n % E == E - 1
    pos = {
        "first": 0,
        # digitize: threads t < 1000 run the four-deep loop once; the last lane of their fourth load
        "digitize-fourth-load": (999 + 3 * NTHREADS) * E + E - 1,
        # roi_minmax (half the threads): every thread runs the four-deep loop once over vectors t + u * 131072, u < 4
        "minmax-fourth-load": (7 + 3 * NTHREADS_MINMAX) * E + E - 1,
        # a vector of the one-vector loop of both kernels (minmax: t + 5 * 131072; digitize: t + 2 * 262144)
        "remainder-loop": (5 * NTHREADS_MINMAX + 12345) * E + (3 % E),
        "tail": n - 1,
    }
    assert all(0 <= p < n for p in pos.values()) and pos["remainder-loop"] // E < nvec
    return pos

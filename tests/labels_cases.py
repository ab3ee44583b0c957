"""Label maps shared by tests/test_labels.py (host census) and tests/test_gpu_labels.py (device census, executeLabels): the
smallest shapes that reach each path of the census kernel (pyradiomics_amd/csrc/kernels_labels.h), the brute-force census
they are checked against, and the small multi-label case of the executeLabels tests."""
import numpy as np


def census_cases():
    """-> [(name, int64 array, dtypes whose range holds every value)]"""
    rng = np.random.default_rng(11)
    all3 = (np.uint8, np.int16, np.int32)
    cases = []
    # odd extents, rows shorter than a wave, labels 1..7 in random blobs over background
    a = np.zeros((5, 7, 9), np.int64)
    for l in range(1, 8):
        z, y, x = rng.integers(0, 5), rng.integers(0, 7), rng.integers(0, 9)
        a[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 2, 0):x + 2] = l
    for l in range(1, 8):                       # (a blob painted over entirely would drop a label: keep one voxel of each)
        a[l % 5, l % 7, l] = l
    cases.append(("blobs_5x7x9", a, all3))
    # a row spans three waves with a ragged tail; one label covers a whole row, another only x = 129
    a = np.zeros((3, 5, 130), np.int64)
    a[1, 2, :] = 4
    a[2, 4, 129] = 6
    a[0, 0, 60:70] = 2                          # crosses the seam between the first two waves of a row
    cases.append(("row_3x5x130", a, all3))
    # 512 distinct labels, one per voxel: nothing to aggregate
    cases.append(("distinct_4x8x16", np.arange(1, 513, dtype=np.int64).reshape(4, 8, 16), (np.int16, np.int32)))
    # labels alternating per lane: never one value per wave
    a = np.tile(np.array([1, 2], np.int64), 64)[None, None, :].repeat(2, 0).repeat(6, 1)
    cases.append(("alternating_2x6x128", np.ascontiguousarray(a), all3))
    # sparse large values: the table does not fit the workgroup's LDS
    a = np.zeros((4, 6, 20), np.int64)
    a[0, 1, 2:9] = 3
    a[1:3, 2:5, 4:16] = 1000
    a[3, 5, 19] = 65535
    cases.append(("sparse_4x6x20", a, (np.int32,)))
    # the extremes of uint8
    a = np.zeros((4, 6, 20), np.int64)
    a[0:2, 0:3, 0:8] = 1
    a[2:4, 3:6, 9:20] = 255
    cases.append(("u8_extremes_4x6x20", a, all3))
    # eight single-voxel labels at the eight corners: bounds at 0 and size - 1 on every axis
    a = np.zeros((6, 5, 12), np.int64)
    l = 1
    for z in (0, 5):
        for y in (0, 4):
            for x in (0, 11):
                a[z, y, x] = l
                l += 1
    cases.append(("corners_6x5x12", a, all3))
    # 2-D maps
    a = np.zeros((17, 130), np.int64)
    a[3:9, 10:100] = 5
    a[16, 129] = 2
    a[0, :] = 7
    cases.append(("flat_17x130", a, all3))
    a = np.zeros((1, 64), np.int64)
    a[0, 10:20] = 3
    a[0, 63] = 1
    cases.append(("flat_1x64", a, all3))
    # nothing segmented
    cases.append(("background_3x4x8", np.zeros((3, 4, 8), np.int64), all3))
    return cases


def brute_census(arr, max_label=None):
    """np.unique with counts and np.argwhere min / max per label, labels 1..max_label"""
    vals, counts = np.unique(arr, return_counts=True)
    keep = vals >= 1
    if max_label is not None:
        keep &= vals <= max_label
    vals, counts = vals[keep].astype(np.int64), counts[keep].astype(np.int64)
    lo = np.zeros((len(vals), arr.ndim), np.int64)
    hi = np.zeros((len(vals), arr.ndim), np.int64)
    for i, v in enumerate(vals):
        idx = np.argwhere(arr == v)
        lo[i], hi[i] = idx.min(0), idx.max(0)
    return vals, counts, lo, hi


def assert_census(got, want, what=""):
    for g, w, name in zip(got, want, ("labels", "counts", "lo", "hi")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differ\n%s\n%s" % (what, name, g, w)


A, B, C_, D, ABSENT = 1, 2, 3, 4, 9


def labels_case():
    """(volume int16 (12, 20, 38), label map int16): a smooth ramp plus seeded noise; the x extent is no multiple of 4.
    Labels: A an interior box, B an L-shaped region touching the x = 37 and z = 0 faces, C a one-slice-thick plate, D a single
    line of voxels (fails minimumROIDimensions: 2); ABSENT does not occur."""
    rng = np.random.default_rng(7)
    zz, yy, xx = np.meshgrid(np.arange(12), np.arange(20), np.arange(38), indexing="ij")
    vol = (40.0 * zz + 17.0 * yy + 9.0 * xx + rng.normal(0.0, 60.0, zz.shape)).astype(np.int16)
    lab = np.zeros(vol.shape, np.int16)
    lab[3:9, 5:14, 8:21] = A
    lab[0:4, 2:11, 30:38] = B
    lab[0:4, 11:17, 34:38] = B
    lab[10, 3:17, 4:26] = C_
    lab[6, 17, 2:13] = D
    return vol, lab

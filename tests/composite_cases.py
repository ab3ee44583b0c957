"""The catalogue of ROIs the composite batched calls of pyradiomics_amd.roi_batch are tested on (tests/test_batch_tight_boxes.py,
tests/test_gpu_batch_composite_limits.py): deterministic generators, no device.

ragged_batch(dtype) -> (boxes, masks, spacing float64 [B, 3] (z, y, x), tags), the ROIs in this order, so that boxes of one shape
interleave with others:

     #  box (z, y, x)   mask                                     why
     0  12, 13, 14      ball, r = 4, centre (6, 6, 7)            ordinary; first of a group of four; x 3 .. 11 grows by 2 right, 1 left
     1   9, 10, 16      block x 11 .. 15, y 2 .. 7, z 1 .. 6     touches the right x face: extent 5 grows left by 3
     2  12, 13, 14      ball, r = 3, centre (4, 8, 5)            the shape of 0, another tight box
     3  12, 13, 14      empty                                    keeps its box; status 0 downstream
     4   9, 10, 16      block x 0 .. 4, y 2 .. 7, z 1 .. 6       touches the left x face: grows right by 3
     5   9, 10, 16      full                                     tight = box; the mask on every face
     6   6,  6,  6      one voxel at (4, 5, 5)                   on the right x face: tight 1 x 1 x 4 (alignedBox grows the one
                                                                 voxel left by 3); execute() refuses it
     7   4,  5,  8      full, image constant 7                   one grey level
     8   1, 12, 16      disc, r = 4, centre (0, 6, 8)            a planar box
     9  12, 13, 14      random, fill 0.5                         fourth of the group
    10   5,  4,  7      full                                     x extent 7 stays short at both faces

Values: floats standard_normal * 300 + 40, integers integers(-500, 1500), every ROI from a seed of its own, so boxes of one shape
do not hold the same data.  Spacing (z, y, x): (1, 1, 1) for even indices, (2.5, 0.8, 0.7) for odd ones.

big_glszm() and many_levels() are handed out separately because only one test uses them."""
import numpy as np

SHAPES = [(12, 13, 14), (9, 10, 16), (12, 13, 14), (12, 13, 14), (9, 10, 16), (9, 10, 16), (6, 6, 6), (4, 5, 8), (1, 12, 16),
          (12, 13, 14), (5, 4, 7)]
TAGS = ["ball4", "right-face", "ball3", "empty", "left-face", "full", "one-voxel", "constant", "planar", "random", "short-x"]
EVEN_SPACING, ODD_SPACING = (1.0, 1.0, 1.0), (2.5, 0.8, 0.7)
EMPTY, ONE_VOXEL, CONSTANT, PLANAR = 3, 6, 7, 8
SEED = 7100


def _ball(shape, centre, r):
    z, y, x = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    return ((z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2) <= r * r


def ragged_masks():
    """the eleven masks (bool arrays) of the table above"""
    masks = [np.zeros(s, dtype=bool) for s in SHAPES]
    masks[0] = _ball(SHAPES[0], (6, 6, 7), 4)
    masks[1][1:7, 2:8, 11:16] = True
    masks[2] = _ball(SHAPES[2], (4, 8, 5), 3)
    masks[4][1:7, 2:8, 0:5] = True
    masks[5][:] = True
    masks[6][4, 5, 5] = True
    masks[7][:] = True
    masks[8] = _ball(SHAPES[8], (0, 6, 8), 4)
    masks[9] = np.random.default_rng(SEED + 99).random(SHAPES[9]) < 0.5
    masks[10][:] = True
    return masks


def values(dtype, shape, seed):
    """the catalogue's intensities of one box"""
    rng = np.random.default_rng(seed)
    if np.issubdtype(np.dtype(dtype), np.integer):
        return rng.integers(-500, 1500, shape).astype(dtype)
    return (rng.standard_normal(shape) * 300 + 40).astype(dtype)


def ragged_batch(dtype):
    """-> (boxes: list of arrays of `dtype`, masks: list of bool arrays, spacing float64 [B, 3] (z, y, x), tags)"""
    boxes = [values(dtype, s, SEED + b) for b, s in enumerate(SHAPES)]
    boxes[CONSTANT][:] = 7
    spacing = np.array([EVEN_SPACING if b % 2 == 0 else ODD_SPACING for b in range(len(SHAPES))], dtype=np.float64)
    return boxes, ragged_masks(), spacing, list(TAGS)


def big_glszm():
    """a (38, 38, 39) float32 box, 56 316 voxels, full mask: above the batched GLSZM's cap and inside that of the batched
    matrices.  Smooth with noise over 0 .. 2000, so that its zones are of many sizes -> (box, mask)"""
    shape = (38, 38, 39)
    z, y, x = np.mgrid[0:38, 0:38, 0:39].astype(np.float64)
    rng = np.random.default_rng(SEED + 500)
    img = 1000.0 + 500.0 * np.sin(z / 5.0) * np.cos(y / 6.0) + 400.0 * np.sin((x + y) / 7.0) + rng.normal(0.0, 30.0, shape)
    return img.astype(np.float32), np.ones(shape, dtype=bool)


def many_levels():
    """a (10, 10, 12) float32 box, full mask, uniform over 0 .. 6000: 1200 bins of width 5, 120 of width 50 -- above the 64
    levels of the native texture calls at either -> (box, mask)"""
    shape = (10, 10, 12)
    img = np.random.default_rng(SEED + 501).uniform(0.0, 6000.0, shape).astype(np.float32)
    img.flat[0], img.flat[1] = 0.0, 6000.0
    return img, np.ones(shape, dtype=bool)


# ---- the numpy restatement of roi_batch._tight_boxes -------------------------------------------------------------------------
def aligned_box(lo, hi, shape):
    """imageoperations.alignedBox restated for one ROI: the x extent grown to a multiple of four, to the right as far as the box
    reaches, to the left for the rest, short where both faces are reached"""
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    need = (-(hi[2] - lo[2] + 1)) % 4
    right = min(need, shape[2] - 1 - hi[2])
    hi[2] += right
    lo[2] -= min(need - right, lo[2])
    return lo, hi


def tight_restated(masks):
    """per ROI the bounding box of the mask (the whole box for an empty one), aligned_box, then the raster indices of that
    sub-box plus the ROI's offset in the flat buffers -> (idx int64, tight int [B, 3], [(lo, hi)] per ROI)"""
    off, idx, tight, bounds = 0, [], [], []
    for m in masks:
        shape = m.shape
        if m.any():
            nz = np.nonzero(m)
            lo, hi = [int(a.min()) for a in nz], [int(a.max()) for a in nz]
        else:
            lo, hi = [0, 0, 0], [s - 1 for s in shape]
        lo, hi = aligned_box(lo, hi, shape)
        raster = np.arange(m.size, dtype=np.int64).reshape(shape)
        idx.append(raster[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1].reshape(-1) + off)
        tight.append([h - l + 1 for l, h in zip(lo, hi)])
        bounds.append((lo, hi))
        off += m.size
    return np.concatenate(idx), np.array(tight), bounds

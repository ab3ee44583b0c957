"""The sliding-window GLCM kernel (pyradiomics_amd/csrc/kernels_voxslide.h) keeps per angle a byte count per level pair and
reads a LUT entry indexed by that count.  Its ranges follow from the window geometry alone, so they are checked here, on the
CPU, by enumerating the voxel pairs of the windows in plain Python: for every angle of the kernel's angle sets (13 in 3-D, the
4 with dz = 0 of a force2D window), radius 1 and 2, the pairs of a window at a centre, the pairs one step along x brings in
and takes out, and the largest count an entry goes through within the step in the order the kernel applies the two planes.
Every index the kernel forms must then have a real LUT entry below the absent pair's, the byte counters must not wrap and the
2^-40 fixed-point sum S of n log2 n must stay below the nnz bits."""
import itertools
import math
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyradiomics_amd", "csrc", "kernels_voxslide.h")


def _macros():
    with open(HEADER) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*#define\s+(PRAD_VS_\w+)\s+(\d+)\b", f.read(), re.M)}


def _angles(two_d):
    """one offset per undirected angle of distance 1 (the sign does not change how many pairs a window holds)"""
    out = []
    for o in itertools.product((-1, 0, 1), repeat=3):
        if o == (0, 0, 0) or (two_d and o[0] != 0):
            continue
        if tuple(-c for c in o) not in out:
            out.append(o)
    return out


def _pairs(voxels, o):
    """the unordered pairs (v, v + o) with both voxels in the set"""
    return {(v, (v[0] + o[0], v[1] + o[1], v[2] + o[2])) for v in voxels
            if (v[0] + o[0], v[1] + o[1], v[2] + o[2]) in voxels}


def _window(radius, two_d, x0):
    d = 2 * radius + 1
    return {(z, y, x) for z in range(1 if two_d else d) for y in range(d) for x in range(x0, x0 + d)}


def _step(radius, two_d, o):
    """(pairs at a centre, pairs entering, pairs leaving) of angle o when the window moves by one voxel along x"""
    before, after = _pairs(_window(radius, two_d, 0), o), _pairs(_window(radius, two_d, 1), o)
    return len(before), len(after - before), len(before - after)


def test_angle_sets():
    assert len(_angles(False)) == 13 and len(_angles(True)) == 4


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("two_d", [False, True], ids=["3d", "2d"])
def test_slide_lut_covers_every_count_of_a_step(radius, two_d):
    m = _macros()
    lut, fix, nnz_shift = m["PRAD_VS_LUT"], m["PRAD_VS_FIX"], m["PRAD_VS_NNZ_SHIFT"]
    leave_first = m.get("PRAD_VS_LEAVE_FIRST", 0)           # (a kernel without the setting applies the entering plane first)
    absent = lut - 1                                         # the all-zero entry an absent pair reads
    d = 2 * radius + 1
    steady_max = transient_max = 0
    for o in _angles(two_d):
        steady, entering, leaving = _step(radius, two_d, o)
        assert entering == leaving > 0                        # (a step keeps the window's shape)
        # an entry counts at most all pairs of its angle (a uniform window); within the step it goes through
        # steady - leaving (leaving plane first) or steady + entering (entering plane first)
        peak = steady if leave_first else steady + entering
        steady_max, transient_max = max(steady_max, steady), max(transient_max, peak)
    pz = 1 if two_d else d
    assert steady_max == pz * d * (d - 1)                    # the angle along x
    # a pair leaving (entering) an entry of count c + 1 (c) reads LUT entry c <= transient_max - 1; a centre reads pt[P],
    # P <= steady_max pairs
    top = max(transient_max - 1, steady_max)
    assert top < absent, "a count of %d pairs per entry within a sliding step: LUT index %d >= %d, the absent-pair entry " \
                         "(radius %d, %s)" % (transient_max, top, absent, radius, "2-D" if two_d else "3-D")
    assert transient_max <= 255, "the byte counters wrap"
    # S = sum n log2 n over the entries, sum n = 2 pairs; largest when every pair lies on one diagonal entry: n = 2 pairs
    n = 2 * transient_max
    s_fixed = round(n * math.log2(n) * 2 ** fix)
    assert s_fixed < 2 ** (nnz_shift - 1), "S reaches the nnz bits: %d log2 %d = %.1f" % (n, n, n * math.log2(n))
    assert n * n < 2 ** 20, "sum n^2 reaches the pair count of EP"

"""GPU: the tier between the sweeps / byte kernels and the exact generic kernels (csrc/kernels_pairs.h, host plans
pairs_glcm_glrlm and pairs_neigh in prad_api.hip) at the limits of its routes, against the C checker (integer outputs,
np.array_equal) and tests/neigh_reference.py (NGTDM's s_i, correctly rounded from the rational).  tests/test_neigh_reference.py
pins the reference to the checker on every GLCM / GLDM / NGTDM case used here and shows that each group changes under the
hazards it exists to catch (the n % 8 tail ignored, the last level-row tile ignored, neighbours wrapped across rows / planes).
Every case asserts the route it took: prad_last_path() and, for GLDM / NGTDM, the bin placement of prad_last_variant()
("pairs-lds64", "pairs-lds32", "pairs-global", with "+box32" / "+box64" on the box-sum path; the label names the LDS bin
width, so GLDM's u32 bins read "pairs-lds32"), restated from the documented thresholds in neigh_reference.expected_route.

Case families (deterministic contents and masks of neigh_reference):
  glcm-tail      (3,5,7+r), r = 0..7: every n % 8; 161 levels with [1] and 8 levels with [1,2]
  glcm-narrow    n < 8 with (1,2,3); Nx in {1,2,3,5} -- (4,3,1) (5,4,2) (3,6,3) (3,3,5) -- so a group of eight spans rows and planes
  glcm-groups    32 levels x [1,2]: 62 angles as 37 + 25; 138 levels x [2]: groups of two, one left over; 2-D (30,33)
  glcm-tiles     Ng in {195, 196, 197, 240} on (9,10,11) and (6,20,21): one tile, 195 + 1 rows, 194 + 3, 160 + 80.  Content
                 `cover` (1 + flat index mod Ng) instead of the issue's `ramp`, whose x + 3y + 7z stays below 94 / 113 on these
                 shapes and never reaches the last tile: with `cover` every level of every tile, the lone level 196 included,
                 has pairs in every angle as centre and as neighbour (asserted on the CPU side, case by case, together with
                 "a lost last tile changes this case"); lattice: most tiles see no voxel
  glrlm          equal content at 161 / 256 / 300 levels (one run of the full extent per line, length == Nr), stripes4, Nr =
                 max(shape) taken and max(shape) - 1 declined, 8 192 / 8 193 levels (level counts in LDS / global), the
                 multi-element rule on corners, one voxel and a single plane; calculate_glrlm alone and calculate_glcm_glrlm
                 (GLRLM alone is a sweep call up to 255 levels -- asserted as such at 161 -- and the tier's from 256)
  pairs-levels   GLDM / NGTDM [1] at Ng in {256, 711, 712, 1422, 1423, 65535} on (8,12,16): both LDS thresholds of the 27-column
                 table; 65 536 leaves the tier (generic); GLDM [1,2] at 307 / 308, GLDM [2] at 387 / 388.  Contents: ramp
                 (levels 1..98 only on this shape), checker3 and lattice (levels 1 and Ng), and cover, which holds every
                 level up to 1 536 -- the whole bin table is written up to 1 423 levels; at 65 535 the high bins are reached
                 through level Ng alone, which is enough for a threshold test
  pairs-nobox    NGTDM without box sums: [2] at {193, 194, 387, 388} (99 columns), PRAD_NGTDM_NO_BOX=1 with [1,2] at
                 {153, 154, 307, 308} (125 columns)
  pairs-box      32-bit words: [1], [1,2] at {153, 154, 307, 308, 65535}; 64-bit words: [1,2,3] at {55, 56, 111, 112, 300};
                 volumes smaller than the box in one, two and all three axes; force2D in each dimension
  pairs-off      PRAD_NO_PAIRS=1: route generic, the same answer

Tolerance.  GLCM, GLRLM, the angle arrays, GLDM and NGTDM columns 0 and 2 must be equal.  NGTDM column 1: |got - exact| <=
(Na + 2) 2^-52 exact (ngtdm_finalize_kernel: Na divisions of exact integers below 2^53, Na additions of non-negative terms in
float64 -- (Na + 1) 2^-53 relative to first order; the bound is twice that).

Measured worst error / bound per route over all cases of this module on an MI355X (test_zz_report prints it and fails above 1):
    pairs-lds64    0.00936    pairs-lds64+box32    0.0377    pairs-lds64+box64    0.0045
    pairs-lds32    0.00988    pairs-lds32+box32    0.0355    pairs-lds32+box64    0.00469
    pairs-global   0.00941    pairs-global+box32   0.0306    pairs-global+box64   0.00627
    generic        0.0306     neigh4-full26        0.0329    ([1] at 153 / 154 levels stays with the byte kernel)

No defect was found: every case passed against the kernels as they were.
"""
import numpy as np
import pytest

import neigh_reference as nr

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.mark.parametrize("group", ["pairs-levels", "pairs-nobox", "pairs-box", "pairs-off"])
def test_gldm_ngtdm_bin_placements(group, checker, monkeypatch):
    seen = {}
    for name in nr.GROUPS[group]:
        s = nr.spec(name)
        route = nr.run_case(name, checker, RATIOS, monkeypatch)
        seen.setdefault((s["family"], tuple(s["distances"]), s["Ng"], s["force2D"], s["shape"]), route)
    P = (8, 12, 16)
    want = {
        "pairs-levels": {("gldm", (1,), 256): "pairs-lds32", ("gldm", (1,), 1422): "pairs-lds32", ("gldm", (1,), 1423): "pairs-global",
                         ("gldm", (1,), 65535): "pairs-global", ("gldm", (1,), 65536): "generic",
                         ("ngtdm", (1,), 256): "pairs-lds64+box32", ("ngtdm", (1,), 711): "pairs-lds64+box32", ("ngtdm", (1,), 712): "pairs-lds32+box32",
                         ("ngtdm", (1,), 1422): "pairs-lds32+box32", ("ngtdm", (1,), 1423): "pairs-global+box32",
                         ("ngtdm", (1,), 65535): "pairs-global+box32", ("ngtdm", (1,), 65536): "generic",
                         ("gldm", (1, 2), 307): "pairs-lds32", ("gldm", (1, 2), 308): "pairs-global",
                         ("gldm", (2,), 387): "pairs-lds32", ("gldm", (2,), 388): "pairs-global"},
        "pairs-nobox": {("ngtdm", (2,), 193): "pairs-lds64", ("ngtdm", (2,), 194): "pairs-lds32", ("ngtdm", (2,), 387): "pairs-lds32",
                        ("ngtdm", (2,), 388): "pairs-global", ("ngtdm", (1, 2), 153): "pairs-lds64", ("ngtdm", (1, 2), 154): "pairs-lds32",
                        ("ngtdm", (1, 2), 307): "pairs-lds32", ("ngtdm", (1, 2), 308): "pairs-global"},
        "pairs-box": {("ngtdm", (1,), 153): "neigh4-full26", ("ngtdm", (1,), 308): "pairs-lds64+box32",
                      ("ngtdm", (1, 2), 153): "pairs-lds64+box32", ("ngtdm", (1, 2), 154): "pairs-lds32+box32",
                      ("ngtdm", (1, 2), 307): "pairs-lds32+box32", ("ngtdm", (1, 2), 308): "pairs-global+box32",
                      ("ngtdm", (1, 2), 65535): "pairs-global+box32",
                      ("ngtdm", (1, 2, 3), 55): "pairs-lds64+box64", ("ngtdm", (1, 2, 3), 56): "pairs-lds32+box64",
                      ("ngtdm", (1, 2, 3), 111): "pairs-lds32+box64", ("ngtdm", (1, 2, 3), 112): "pairs-global+box64",
                      ("ngtdm", (1, 2, 3), 300): "pairs-global+box64"},
        "pairs-off": {("gldm", (1,), 300): "generic", ("ngtdm", (1, 2), 300): "generic"},
    }[group]
    for (fam, dist, Ng), route in want.items():
        assert seen[(fam, dist, Ng, False, P)] == route, (fam, dist, Ng, seen[(fam, dist, Ng, False, P)])
    if group == "pairs-box":
        small = {k: v for k, v in seen.items() if k[4] != P}
        assert len(small) == 6 and all(v.startswith("pairs-") and "+box" in v for v in small.values()), small
        f2d = {k: v for k, v in seen.items() if k[3]}
        assert f2d and all(v == "pairs-lds64+box32" for v in f2d.values()), f2d


@pytest.mark.parametrize("group", ["glcm-tail", "glcm-narrow", "glcm-groups", "glcm-tiles"])
def test_glcm_visits_of_eight_angle_groups_and_row_tiles(group, checker):
    if group == "glcm-tail":
        assert sorted({int(np.prod(nr.spec(n)["shape"])) % 8 for n in nr.GROUPS[group]}) == list(range(8))
    if group == "glcm-tiles":
        W = nr.PAIR_LDS_WORDS
        assert 195 * 195 <= W < 196 * 196 and W // 196 == 195 and W // 197 == 194 and W // 240 == 160
    for name in nr.GROUPS[group]:
        assert nr.run_case(name, checker, RATIOS) == "pairs"


def _same(ours, theirs, label):
    """both raise IndexError, or both return equal arrays"""
    try:
        want = theirs()
    except IndexError:
        with pytest.raises(IndexError):
            ours()
        return None
    got = ours()
    for g, w in zip(got, want):
        assert np.array_equal(g, w), label
    return got


def _glrlm_all(levels, mask, Ng, Nr, checker, label, f2d=False, dim=0, path="pairs"):
    """calculate_glrlm alone, then calculate_glcm_glrlm.  Up to 255 levels the run-length table alone fits the sweeps' LDS
    budget, so GLRLM on its own is a sweep call ("lines") there: the tier takes it from 256 levels, or together with a GLCM
    whose Ng x Ng table the sweeps cannot hold (161 levels on these narrow volumes)"""
    from pyradiomics_amd import cmatrices as cm, _lib
    wr = lambda: checker.calculate_glrlm(levels, mask, Ng, Nr, f2d, dim)
    out = _same(lambda: cm.calculate_glrlm(levels, mask, Ng, Nr, f2d, dim), wr, label)
    alone = "sweep" if path == "pairs" and Ng <= 255 else path
    assert _lib.last_path() == alone, (label, _lib.last_path())
    assert out is not None or path == "generic"
    if alone != "generic":
        assert _lib.last_variant() == {"pairs": "pairs", "sweep": "lines"}[alone], (label, _lib.last_variant())
    both = _same(lambda: cm.calculate_glcm_glrlm(levels, mask, Ng, Nr, f2d, dim),
                 lambda: (checker.calculate_glcm(levels, mask, [1], Ng, f2d, dim)[0],) + tuple(wr()), label)
    assert _lib.last_path() == path, (label, _lib.last_path())
    assert path == "generic" or (both is not None and _lib.last_variant() == "pairs")
    return out, both


@pytest.mark.parametrize("Ng", [161, 256, 300])
def test_glrlm_full_extent_runs_and_the_run_length_bound(Ng, checker):
    for shape in ((5, 6, 7), (7, 7, 7), (9, 12)):
        for cont in ("equal", "stripes4", "ramp"):
            for mask in ("full", "holes4"):
                levels, m = nr.content(cont, shape, Ng), nr.roi(mask, shape)
                Nr = max(shape)
                out, _ = _glrlm_all(levels, m, Ng, Nr, checker, (shape, cont, mask, Ng))
                if cont == "equal" and mask == "full":
                    assert out[0][0, Ng - 1, Nr - 1].sum() >= 1            # a run of exactly Nr voxels
                # one bin short: the tier declines, the exact kernels say what the reference says (an IndexError for a run
                # of max(shape) voxels)
                _glrlm_all(levels, m, Ng, Nr - 1, checker, (shape, cont, mask, Ng, "Nr - 1"), path="generic")
    for dim in (0, 1, 2):
        levels, m = nr.content("equal", (5, 6, 7), Ng), nr.roi("full", (5, 6, 7))
        _glrlm_all(levels, m, Ng, 7, checker, ("force2D", dim, Ng), f2d=True, dim=dim)


@pytest.mark.parametrize("Ng", [8192, 8193])
def test_glrlm_level_counts_in_lds_and_in_global_memory(Ng, checker):
    from pyradiomics_amd import cmatrices as cm, _lib
    shape = (9, 10, 16)
    for cont, mask in (("ramp", "full"), ("stripes4", "faces")):
        levels, m = nr.content(cont, shape, Ng), nr.roi(mask, shape)
        levels[0, 0, 0] = Ng                                              # the last level is present
        got, ang = cm.calculate_glrlm(levels, m, Ng, 16, False, 0)
        assert _lib.last_path() == "pairs" and _lib.last_variant() == "pairs"
        want, wang = checker.calculate_glrlm(levels, m, Ng, 16, False, 0)
        assert np.array_equal(ang, wang) and np.array_equal(got, want), (Ng, cont)
        assert got[0, Ng - 1].sum() > 0


def test_glrlm_multi_element_rule(checker):
    """cmatrices.c:524-534: an angle none of whose lines holds two ROI voxels loses its run-length-1 column"""
    Ng, shape = 300, (4, 5, 6)
    levels = nr.content("iid", shape, Ng)
    plane = np.zeros(shape, bool)
    plane[2] = True
    masks = {m: nr.roi(m, shape) for m in ("corners", "one0", "one7", "one8", "empty")}
    masks["plane"] = plane
    for tag, m in masks.items():
        for f2d in (False, True):
            _glrlm_all(levels, m, Ng, 6, checker, (tag, f2d), f2d=f2d, dim=0)


def test_zz_report():
    assert RATIOS, "no NGTDM comparison ran before the report"
    nr.report("pairs limits", RATIOS)

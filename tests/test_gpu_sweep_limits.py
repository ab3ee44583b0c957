"""GPU: the GLCM / GLRLM sweep kernels (csrc/kernels_sweep.h, kernels_sweepfw.h, kernels_sweepfw2.h) at the limits of their
tables, bit-exact against the `checker` fixture (the reference's own cmatrices.c when oracle/_ref travelled, else the pinned
restatement).  Every assertion is exact equality of integer-valued matrices.  The constructions are those of
tests/sweep_limits_cases.py, which tests/test_sweep_limits_cases.py checks on the host.

1. Regime changes.  The planner (prad_debug_sweep_plan, asked for the device that runs the test) is scanned over Ng = 1 .. 256
   for one shape per row class; wherever (ok, fused, fw, fw2, fw2_rows, fw2_copies, fw2r_copies, fw2r_waves) changes, both
   neighbours run: GLCM + GLRLM together, each alone (the separate-table layouts differ then), on uniform noise that holds
   every level under a 70 % mask and on a smooth volume under a full mask, with last_path / last_variant held to the plan.
   The scan has to find 36|37, 39|40, 125|126, 157|158, 170|171 at rows of 300 voxels and 36|37, 95|96 at rows of 64 and 600:
   a retuned planner fails these tests (the message lists the changes it found) instead of leaving them without a subject.
2. Planted runs at the edges of the length slots, along every angle each kernel walks (sweep_limits_cases.PLANTED): lengths
   RS - 1 .. RS + 2 of each table that has a long-run path, RS + 63 .. RS + 66 around the last bin of the fused long table G, a run
   that ends at the volume's edge, one that ends at a masked-out voxel, one that starts at march step 7 (a piece boundary under
   PRAD_FW_CL=8, with which the fixed-window cases run a second time), the top level among them.  RS comes from the plan.
   First the CHECKER's GLRLM must hold every planted (level, length, angle): a clipped or merged construction fails as
   "construction broken", not as a kernel failure.  Separate tables hold so many lengths that their line walk reaches its
   long-run path only on long lines: three volumes cover the angles that do not move in x, those that march z and those that
   march y while drifting in x (lines that wrap and break at the slot edge); the four space diagonals are left out there for
   their size (about 6 M voxels) and have the slot edge on the fused table only.
3. Runs of length 1 under skip1: planted levels as isolated voxels on every corner, edge and face and next to masked-out
   voxels; PRAD_FW2_NOSKIP1=1 must be bit-equal, and a call without the x angle (the plan clears skip1) exact.
4. Ranks and Nr: 1-D and 2-D calls (single-row line roles), force2D over each dimension, Nr = the longest edge and + 5 (the
   extra columns are zero), Nr = the longest edge - 1 (declined by the planner; noise whose longest run a host walk bounds).

Sharpness.  One-line mutations of a scratch copy of the kernels, loaded through PRAD_LIB and never committed, each run once
against this module (as it was before the two separate_ng95_* cases joined it: 71 cases), and the tests that failed:
  * the long-run comparison of the fused Walker off by one (kernels_sweep.h Walker::step, `lb > lenmax`: a run of RS + 1 is no
    long run): test_both_sides_of_a_required_regime_change[nx64-36_37], test_planted_runs_at_the_slot_edges[fused_lines_rows-None],
    test_one_dimensional_calls[300-32 / 1025-32], test_two_dimensional_calls[257-1-32 / 513-1-32]
  * the same comparison in the fixed-window step (kernels_sweepfw.h fw_checked, `lb > T.lenlim`):
    test_both_sides_of_a_required_regime_change[nx300-36_37 / nx600-36_37], test_planted_runs_at_the_slot_edges[fused_fw-* /
    fused_fw_rows_launch-*], test_two_dimensional_calls[513-9-32], test_force2d_over_each_dimension[*-32],
    test_nr_beyond_the_longest_edge_in_three_dimensions[32]
  * the last bin of G off by one (`idx <= RS + RL`: a run of RS + 65 lands in the next level's first bin), in Walker::long_event:
    test_planted_runs_at_the_slot_edges[fused_lines_rows-None] ALONE; in fw_long_event:
    test_planted_runs_at_the_slot_edges[fused_fw-* / fused_fw_rows_launch-*] alone.  Off by one the other way (`idx < RS + RL - 1`) is
    an equivalent mutation: the run of RS + 64 takes the wave-aggregated global atomic, which adds to the same accumulator word
    the flush of G would have added to
  * fw2_long_event called with the length instead of the length index (`lb >> 2`):
    test_both_sides_of_the_other_regime_changes[nx300], every fw2_* case of test_planted_runs_at_the_slot_edges
  * the copy index of the fw2 length slots fixed to copy 0 in fw2_flush: 24 cases -- every case that runs the two-table
    kernels: test_both_sides_of_a_required_regime_change[nx300-39_40 / 125_126 / 157_158 / 170_171],
    test_both_sides_of_the_other_regime_changes[nx300], the fw2_* planted cases, test_isolated_voxels_of_planted_levels_under_skip1[*],
    test_two_dimensional_calls[65|257-2|9-64], test_force2d_over_each_dimension[*-64],
    test_nr_beyond_the_longest_edge_in_three_dimensions[64]
  * the skip1 restore skipped for level Ng (finalize_angle_work, `restore && i != Ng - 1`): the same cases but
    test_force2d_over_each_dimension[2-64], whose angle list has no x angle and so no restore (23 cases)
  * the x role flushing its table with the line roles' layout (RSfw in place of RSfw_rows, in sweep_fw_kernel):
    test_both_sides_of_a_required_regime_change[nx300-36_37 / nx600-36_37], test_planted_runs_at_the_slot_edges[fused_fw-*],
    test_two_dimensional_calls[*-2-32 / *-9-32], test_force2d_over_each_dimension[0-32 / 1-32],
    test_nr_beyond_the_longest_edge_in_three_dimensions[32].  (RSfw in the role's WALK was not run: its staging tiles would then
    lie behind a table that fills the workgroup's LDS, outside the allocation.)
"""
import os

import numpy as np
import pytest

import sweep_limits_cases as slc
import sweep_plan_cases as spc

pytestmark = pytest.mark.gpu

_CACHE = {}            # construction and reference of a case, computed once and left unchanged


@pytest.fixture(scope="module")
def cm():
    from pyradiomics_amd import cmatrices
    return cmatrices


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """plans and calls see only the switches a test sets itself"""
    for name in list(os.environ):
        if name.startswith("PRAD_") and name != "PRAD_LIB":
            monkeypatch.delenv(name)


def _reference(checker, key, img, mask, Ng, Nr, force2D=False, dim=0):
    key = ("ref",) + tuple(key) + (Nr, force2D, dim)
    if key not in _CACHE:
        eg, eang = checker.calculate_glcm(img, mask, [1], Ng, force2D, dim)
        er, _ = checker.calculate_glrlm(img, mask, Ng, Nr, force2D, dim)
        for a in (eg, er, eang):
            a.setflags(write=False)
        _CACHE[key] = (eg, er, eang)
    return _CACHE[key]


def _same(what, got, want, ang):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s differs at %d entries, first (voxel, i, j, angle) = %s: %s vs %s; angle %s" % (
        what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])], ang[bad[0][-1]])


def _run(cm, lib, checker, key, img, mask, Ng, nr_delta=0, force2D=False, dim=0, alone=False, route=True):
    """calculate_glcm_glrlm (and each matrix alone) against the checker, route held to the plan; -> (glcm, glrlm, plan).
    The route assertion asks the planner the library itself calls, so it catches a quiet fall-back to the pairs tier or the
    exact kernels, not a wrong plan; the planted cases pin the plan's flags and the variant to fixed values (REACHES)"""
    from pyradiomics_amd import _lib
    Nr = int(max(img.shape)) + nr_delta
    eg, er, eang = _reference(checker, key, img, mask, Ng, Nr, force2D, dim)
    angles = np.ascontiguousarray(eang, dtype=np.int32)
    g, r, ang = cm.calculate_glcm_glrlm(img, mask, Ng, Nr, force2D, dim)
    f = slc.plan_fields(lib, img.shape, Ng, nr_delta, 3, 0, angles)
    if route:
        assert (_lib.last_path(), _lib.last_variant()) == slc.expected_variant(f, 3), f
    assert np.array_equal(ang, eang)
    _same("GLCM", g, eg, ang)
    _same("GLRLM", r, er, ang)
    if alone:
        g1, _ = cm.calculate_glcm(img, mask, [1], Ng, force2D, dim)
        f1 = slc.plan_fields(lib, img.shape, Ng, nr_delta, 1, 0, angles)
        assert (_lib.last_path(), _lib.last_variant()) == slc.expected_variant(f1, 1), f1
        _same("GLCM alone", g1, eg, ang)
        r1, _ = cm.calculate_glrlm(img, mask, Ng, Nr, force2D, dim)
        f2 = slc.plan_fields(lib, img.shape, Ng, nr_delta, 2, 0, angles)
        assert (_lib.last_path(), _lib.last_variant()) == slc.expected_variant(f2, 2), f2
        _same("GLRLM alone", r1, er, ang)
    return g, r, f


# ---- 1. both sides of every regime change -------------------------------------------------------------------------------------
def _changes(lib, shape):
    key = ("changes", shape)
    if key not in _CACHE:
        _CACHE[key] = slc.regime_changes(lib, shape, cus=0)
        print("regime changes of %s on this device: %s" % (shape, " ".join("%d|%d" % c for c in _CACHE[key])))
    return _CACHE[key]


def _regime_case(cm, lib, checker, shape, Ng):
    for kind in ("noise", "smooth"):
        key = (kind, shape, Ng)
        if key not in _CACHE:
            _CACHE[key] = slc.noise(shape, Ng, seed=Ng) if kind == "noise" else slc.smooth(shape, Ng, seed=Ng)
        img, mask = _CACHE[key]
        _run(cm, lib, checker, key, img, mask, Ng, alone=True)


@pytest.mark.parametrize("shape,lo", [(s, lo) for s in slc.SCAN_SHAPES for lo, _hi in slc.REQUIRED[s]],
                         ids=["nx%d-%d_%d" % (s[2], lo, hi) for s in slc.SCAN_SHAPES for lo, hi in slc.REQUIRED[s]])
def test_both_sides_of_a_required_regime_change(cm, lib, checker, shape, lo):
    found = _changes(lib, shape)
    assert (lo, lo + 1) in found, "the planner no longer changes its regime at %d|%d for %s; it does at %s" % (lo, lo + 1, shape, found)
    for Ng in (lo, lo + 1):
        _regime_case(cm, lib, checker, shape, Ng)


@pytest.mark.parametrize("shape", slc.SCAN_SHAPES, ids=["nx%d" % s[2] for s in slc.SCAN_SHAPES])
def test_both_sides_of_the_other_regime_changes(cm, lib, checker, shape):
    """whatever else this device's planner changes inside the scan (fw2_copies, the x-angle kernel's waves and copies)"""
    found = _changes(lib, shape)
    assert set(slc.REQUIRED[shape]) <= set(found), "regime changes of %s: %s" % (shape, found)
    for lo, hi in found:
        if (lo, hi) not in slc.REQUIRED[shape]:
            _regime_case(cm, lib, checker, shape, lo)
            _regime_case(cm, lib, checker, shape, hi)


@pytest.mark.parametrize("Ng", [255, 256])
@pytest.mark.parametrize("shape", [(12, 10, 300), (12, 10, 64)], ids=["nx300", "nx64"])
def test_upper_end_of_the_levels(cm, lib, checker, shape, Ng):
    _regime_case(cm, lib, checker, shape, Ng)


# ---- 2. planted runs at the edges of the length slots --------------------------------------------------------------------------
def _planted(lib, name):
    key = ("planted", name)
    if key not in _CACHE:
        c = slc.planted_case(lib, name, cus=0)
        c["img"].setflags(write=False)
        c["mask"].setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


FIXED_WINDOW = [n for n, r in slc.REACHES.items() if r[1] or r[2]]


@pytest.mark.parametrize("name,cl", [(n, None) for n in slc.PLANTED] + [(n, "8") for n in FIXED_WINDOW])
def test_planted_runs_at_the_slot_edges(cm, lib, checker, name, cl, monkeypatch):
    from pyradiomics_amd import _lib
    c = _planted(lib, name)
    f = c["plan"]
    fused, fw, fw2, fw2_rows, xrole = slc.REACHES[name]
    assert (f["ok"], f["fused"], f["fw"], f["fw2"], f["fw2_rows"], f["fw_xblocks"] > 0) == (1, fused, fw, fw2, fw2_rows, xrole), f
    assert c["tables"] and c["reqs"] and not c["missing"], "construction broken: not placed %s" % c["missing"]
    eg, er, eang = _reference(checker, ("planted", name), c["img"], c["mask"], c["Ng"], c["Nr"])
    assert np.array_equal(eang, c["angles"])
    broken = slc.construction_errors(er[0], c["placed"], c["Ng"])
    assert not broken, "construction broken: %s" % broken[:5]
    assert any(lv == c["Ng"] for *_r, lv, _s in c["placed"])
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    if cl is not None:
        monkeypatch.setenv("PRAD_FW_CL", cl)
    g, r, f_now = _run(cm, lib, checker, ("planted", name), c["img"], c["mask"], c["Ng"])
    assert {k: f_now[k] for k in ("RS", "RSr", "RSfw", "RSfw_rows", "RS2", "RS2r")} == {k: f[k] for k in ("RS", "RSr", "RSfw", "RSfw_rows", "RS2", "RS2r")}
    assert _lib.last_variant() == ("fw2" if fw2 else ("fw" if fw else "lines"))
    for (level, L, ai), n in slc.expected_counts(c["placed"]).items():      # (implied by the equality above; names the run that is lost)
        if L >= 2:
            assert r[0, level - 1, L - 1, ai] == n, "planted run (level %d, length %d, angle %s)" % (level, L, c["angles"][ai])


# ---- 3. runs of length 1 under skip1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ng", [64, 126, 170])
def test_isolated_voxels_of_planted_levels_under_skip1(cm, lib, checker, Ng, monkeypatch):
    from pyradiomics_amd import _lib
    shape = (9, 11, 130)
    key = ("isolated", shape, Ng)
    if key not in _CACHE:
        _CACHE[key] = slc.isolated(shape, Ng, seed=Ng)
    img, mask, planted = _CACHE[key]
    eg, er, eang = _reference(checker, key, img, mask, Ng, 130)
    assert er[0][Ng // 2:, 1:, :].sum() == 0 and (er[0][Ng // 2:, 0, :].sum(axis=0) == len(planted)).all(), "construction broken"
    assert er[0][Ng - 1, 0, :].min() >= 1, "construction broken: level Ng not planted"
    g, r, f = _run(cm, lib, checker, key, img, mask, Ng)
    assert f["fw2"] == 1 and f["skip1"] == 1 and _lib.last_variant() == "fw2"
    # a call without the x angle: nothing to restore the runs of length 1 from, the plan clears skip1 and the walk records them
    g2, r2, f2 = _run(cm, lib, checker, key, img, mask, Ng, force2D=True, dim=2)
    assert f2["fw2"] == 1 and f2["skip1"] == 0 and f2["row_slot"] == -1 and _lib.last_variant() == "fw2"
    monkeypatch.setenv("PRAD_FW2_NOSKIP1", "1")
    g1, r1, f1 = _run(cm, lib, checker, key, img, mask, Ng)
    assert f1["fw2"] == 1 and f1["skip1"] == 0
    assert np.array_equal(g1, g) and np.array_equal(r1, r)


# ---- 4. ranks and Nr ---------------------------------------------------------------------------------------------------------------
def _ranked(cm, lib, checker, shape, Ng, force2D=False, dim=0):
    longest = max(shape)
    for kind in ("noise", "smooth"):
        key = (kind, shape, Ng)
        if key not in _CACHE:
            _CACHE[key] = slc.noise(shape, Ng, seed=Ng + len(shape)) if kind == "noise" else slc.smooth(shape, Ng, seed=Ng + len(shape))
        img, mask = _CACHE[key]
        _run(cm, lib, checker, key, img, mask, Ng, 0, force2D, dim)
        g, r, f = _run(cm, lib, checker, key, img, mask, Ng, 5, force2D, dim)
        assert r.shape[2] == longest + 5 and not r[:, :, longest:, :].any()


@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("Nx", [65, 300, 1025])
def test_one_dimensional_calls(cm, lib, checker, Nx, Ng):
    _ranked(cm, lib, checker, (Nx,), Ng)


@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("Ny", [1, 2, 9])
@pytest.mark.parametrize("Nx", [65, 257, 513])
def test_two_dimensional_calls(cm, lib, checker, Nx, Ny, Ng):
    """[Ny, Nx]: every line role has a single row"""
    _ranked(cm, lib, checker, (Ny, Nx), Ng)


@pytest.mark.parametrize("Ng", [32, 64])
@pytest.mark.parametrize("dim", [0, 1, 2])
def test_force2d_over_each_dimension(cm, lib, checker, dim, Ng):
    _ranked(cm, lib, checker, (9, 70, 130), Ng, True, dim)


@pytest.mark.parametrize("Ng", [32, 38, 64])
def test_nr_beyond_the_longest_edge_in_three_dimensions(cm, lib, checker, Ng):
    _ranked(cm, lib, checker, (9, 70, 130), Ng)


@pytest.mark.parametrize("shape,Ng", [((12, 10, 300), 32), ((9, 70, 130), 64), ((300,), 32), ((9, 257), 38)],
                         ids=["12x10x300-32", "9x70x130-64", "300-32", "9x257-38"])
def test_nr_one_short_of_the_longest_edge_is_declined_and_exact(cm, lib, checker, shape, Ng):
    """Nr = the longest edge - 1: a run could overflow the matrix, so the planner declines and the exact kernels take the call.
    Noise only, and first a host walk shows that no run reaches Nr (the reference writes past its array otherwise)"""
    from pyradiomics_amd import _lib
    key = ("noise", shape, Ng)
    if key not in _CACHE:
        _CACHE[key] = slc.noise(shape, Ng, seed=Ng + len(shape))
    img, mask = _CACHE[key]
    angles = spc.angle_list(lib, list(shape), 0)
    assert slc.longest_run(img, mask, angles) < max(shape) - 1
    g, r, f = _run(cm, lib, checker, key, img, mask, Ng, -1, route=False)
    assert f == {"ok": 0} and _lib.last_path() != "sweep"
    assert r.shape[2] == max(shape) - 1

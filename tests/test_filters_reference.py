"""CPU: tests/filters_reference.py (numpy long double, its own code) pinned to itself, the float64 restatement
oracle/filters_oracle.py held to it, the condition on the LoG cases (no voxel within the measured radius of a float32 rounding
tie) and proof that every family of cases moves under the hazard it exists to catch.  tests/test_gpu_filter_limits.py runs the
same cases on the device.  `test_zz_report` prints the figures of profiles/filter_limits_measurements.md."""
import numpy as np
import pytest

import filters_reference as fr
from oracle import filters_oracle as fo

pytestmark = pytest.mark.skipif(not fr.AVAILABLE, reason=fr.SKIP_REASON)

fr.use_taps(fo.wavelet_filters)
LD = fr.LD
WAVELET_CASES = [n for n, s in fr.CASES.items() if s["kind"] == "w"]
LOG_GROUPS = [g for g in fr.GROUPS if g.startswith("l:")]
RATIOS = {}         # wavelet: oracle distance / bound per family
DISTANCES = {}      # LoG: worst float64-to-long-double line distance per family, in float32 ulps of the pass's largest output
FLAGGED = {}
UNDECIDED_DIFFER = {}   # voxels of the float64 restatement that differ from the reference on the undecided pairs (measured only)

# (mutation, family): the mutation must move at least one case of the family beyond its bound (LoG: change a bit)
HAZARDS = [("one-wrap", "w:taps"), ("reversed", "w:taps"), ("centre", "w:tiles"), ("swapped", "w:dims"), ("z-first", "w:dims"),
           ("float32-stage", "w:dtypes"), ("centre", "w:levels"), ("line-alias", "w:grid"), ("lost-tail", "w:grid"),
           ("centre", "w:nonfinite"),
           ("smooth-first", "l:lengths:float32:axis2"), ("smooth-first", "l:lengths:float64:axis1"),
           ("float64-between", "l:sigmad"), ("single-rounding", "l:sigmad"), ("float32-input", "l:content"),
           ("zero-causal-start", "l:content"), ("zero-anticausal-start", "l:content"), ("second-start", "l:content"),
           ("zero-causal-start", "l:dims"), ("second-start", "l:dims"), ("normalize-flipped", "l:options"), ("smooth-first", "l:entry"),
           ("spacing-xyz", "l:lengths:float64:axis0"), ("spacing-xyz", "l:lengths:float32:axis1")] + \
          [("block-restart", "l:lengths:%s:%s" % (dt, k)) for dt in ("float32", "float64") for k in ("axis0", "axis1", "axis2", "many")]


def _oracle_lines(sigma, spacing, order, normalize, moved):
    return fo._filter_lines(moved, fo.recursive_gaussian_coefficients(sigma, spacing, order, normalize))


def test_case_table_covers_what_the_families_promise():
    assert set(fr.WAVELET_MUTATIONS) | set(fr.LOG_MUTATIONS) == {m for m, _ in HAZARDS}
    assert set(fr.GROUPS) == {g for _, g in HAZARDS}
    for dt in ("float32", "float64"):
        for axis in range(3):
            assert [fr.spec(n)["shape"][axis] for n in fr.GROUPS["l:lengths:%s:axis%d" % (dt, axis)]] == list(range(4, 54))
    for F, w in fr.WAVELETS.items():
        assert len(fo.wavelet_filters(w)[0]) == F
        for axis in range(3):
            have = {fr.spec(n)["shape"][axis] for n in fr.GROUPS["w:taps"] if ("-%s-a%d-" % (w, axis)) in n}
            assert have == {2, 4, F - 2, F, F + 2, 34} - {0}, (w, axis, have)
    assert len(fr.taps("custom32")[0]) == fr.MAX_TAPS
    x = fr.case("w-grid-lines")
    assert x.shape[0] > fr.LINE_FOLD and fr.case("w-grid-stride").size > fr.GRID_CAP
    seeds = [fr.seed_of(n) for n in fr.CASES]
    assert len(set(seeds)) == len(seeds)                             # no case repeats another's image
    big = [n for n in fr.CASES if fr.case(n).size > 30000]
    assert sorted(big) == ["w-grid-lines", "w-grid-stride", "w-grid-stride-old"], big
    a = fr.case("l-content-above24-int32")
    assert np.abs(a.astype(np.int64)).min() >= 2 ** 24 and not np.array_equal(a.astype(np.float32).astype(np.int64), a)
    b = fr.case("l-content-bits-float64")
    assert not np.array_equal(b.astype(np.float32).astype(np.float64), b)


@pytest.mark.parametrize("wavelet", ["haar", "db2", "coif1", "db4", "coif2"])
def test_wavelet_bands_of_an_even_image_carry_2_to_the_p_times_its_energy(wavelet):
    x = np.random.default_rng(11).standard_normal((6, 8, 10))
    for axes in ((2, 1, 0), (1, 2), (0,)):
        ap, lev = fr.swt3(x, wavelet, axes=axes)
        e = (ap ** 2).sum() + sum((v ** 2).sum() for v in lev[0].values())
        want = LD(2) ** len(axes) * (x.astype(LD) ** 2).sum()
        assert abs(e / want - 1) < 1e-10, (wavelet, axes, float(e / want - 1))      # (the tables hold ~1e-12)


@pytest.mark.parametrize("sigmad", [0.3, 1.0, 4.0])
def test_recursion_on_a_constant_and_on_a_parabola(sigmad):
    eps = float(np.finfo(LD).eps)
    const = np.full((2, 40), LD(7))
    c0 = fr.coefficients(sigmad, 1.0, 0, False)
    c2 = fr.coefficients(sigmad, 1.0, 2, True)
    assert np.abs(fr.filter_lines(const, c0) - 7).max() <= 64 * eps * 7
    assert np.abs(fr.filter_lines(const, c2)).max() <= 64 * eps * 7 * max(1.0, sigmad ** 2) * 16
    ln = 400
    t = np.arange(ln, dtype=LD) - ln // 2
    quad = (t * t / 2)[None, :]
    mid = fr.filter_lines(quad, c2)[0, ln // 2 - 20: ln // 2 + 20]
    assert np.abs(mid / LD(sigmad) ** 2 - 1).max() < 1e-9, float(np.abs(mid / LD(sigmad) ** 2 - 1).max())
    raw = fr.filter_lines(quad, fr.coefficients(sigmad, 1.0, 2, False))[0, ln // 2 - 20: ln // 2 + 20]
    assert np.abs(raw - 1).max() < 1e-9


def test_bound_is_the_first_order_formula():
    lo, hi = fo.wavelet_filters("coif1")
    S = np.abs(lo).sum()
    for p in (1, 3, 9):
        assert abs(fr.wavelet_bound(lo, hi, p, 1000.0) / (p * 6 * fr.U * S ** p * 1000.0) - 1) < 1e-13


def test_a_pair_of_34_taps_is_beyond_the_model_too():
    assert len(fr.custom_taps(34)[0]) > fr.MAX_TAPS


@pytest.mark.parametrize("group", [g for g in fr.GROUPS if g.startswith("w:")])
def test_float64_restatement_meets_the_wavelet_bound(group):
    for name in fr.GROUPS[group]:
        s = fr.spec(name)
        wav = s["wavelet"] if not s["wavelet"].startswith("custom") else fr.taps(s["wavelet"])
        ap, lev = fo.swt3(fr.case(name), wav, s.get("level", 1), s.get("start_level", 0), s["axes"])
        r = fr.wavelet_ratio(name, ap, lev)
        RATIOS[group] = max(RATIOS.get(group, 0.0), r)
        assert r <= 1.0, (name, r)


@pytest.mark.parametrize("name", ["w-taps-haar-a0-2x4x6", "w-taps-coif1-a1-4x8x6", "w-dims-9x13-axes10"])
def test_fused_multiply_add_sums_meet_the_wavelet_bound_too(name):
    """one rounding per tap instead of two (what the device computes: tests/test_gpu_filter_limits.py compares) is another
    float64 evaluation inside the same bound, and not the unfused restatement's bits"""
    s = fr.spec(name)
    fused = fr.swt3_fused_float64(name)
    r = fr.wavelet_ratio(name, *fused)
    ap, lev = fo.swt3(fr.case(name), s["wavelet"], axes=s["axes"])
    print("%s: fused / bound %.3g, unfused / bound %.3g" % (name, r, fr.wavelet_ratio(name, ap, lev)))
    assert r <= 1.0
    assert any(not np.array_equal(fused[1][0][k], lev[0][k]) for k in lev[0])


@pytest.mark.parametrize("group", LOG_GROUPS)
def test_float64_restatement_equals_the_log_reference_and_no_voxel_is_flagged(group):
    for name in fr.GROUPS[group]:
        s = fr.spec(name)
        want, nflag, dist = fr.reference(name, other_lines=_oracle_lines)
        for sg, w, nf, d in zip(s["sigmas"], want, nflag, dist):
            got = fo.laplacian_recursive_gaussian(fr.case(name), s["spacing"], sg, s.get("normalize", True))
            assert got.dtype == w.dtype and got.shape == w.shape
            differ = int((got != w).sum())
            if sg in fr.undecided(name):        # the list may not hide a pair that the reference can decide
                key = group + " (undecided)"
                assert nf > 0, (name, sg, "has no flagged voxel: take it out of filters_reference.UNDECIDED")
                UNDECIDED_DIFFER[key] = UNDECIDED_DIFFER.get(key, 0) + differ
            else:
                key = group
                FLAGGED[key] = FLAGGED.get(key, 0) + nf
                assert nf == 0, (name, sg, nf, "re-seed this case (filters_reference.RESEED)")
                assert differ == 0 and np.array_equal(got.view(np.uint8), w.view(np.uint8)), (name, sg, differ)
            DISTANCES[key] = max(DISTANCES.get(key, 0.0), d)


def _moved(name, mutation):
    s = fr.spec(name)
    if s["kind"] == "w":
        return not fr.wavelet_ratio(name, *fr.reference(name, mutation)) <= 1.0
    return any(not np.array_equal(a.view(np.uint8), b.view(np.uint8))              # (decided sigmas only: the others are not
               for sg, a, b in zip(s["sigmas"], fr.reference(name, mutation), fr.reference(name))    # held to this reference)
               if sg not in fr.undecided(name))


@pytest.mark.parametrize("mutation,group", HAZARDS)
def test_every_family_moves_under_its_hazard(mutation, group):
    for name in reversed(fr.GROUPS[group]):
        if _moved(name, mutation):
            print("%s: %s caught by %s" % (group, mutation, name))
            return
    raise AssertionError("no case of %s notices %s" % (group, mutation))


def test_zz_report():
    assert RATIOS and DISTANCES
    print("\nfloat64 restatement / wavelet bound per family:")
    for k in sorted(RATIOS):
        print("    %-28s %.3g" % (k, RATIOS[k]))
    print("LoG: worst float64-to-long-double line distance (float32 ulps of the pass's largest output), flagged voxels:")
    for k in sorted(DISTANCES):
        print("    %-40s %.3g   %s" % (k, DISTANCES[k], FLAGGED[k] if k in FLAGGED else
                                       "(restatement differs from the reference on %d voxels)" % UNDECIDED_DIFFER[k]))
    pairs = sum(len(fr.spec(n)["sigmas"]) for n in fr.CASES if fr.spec(n)["kind"] == "l")
    print("    (case, sigma) pairs: %d, undecided: %d" % (pairs, sum(len(v) for v in fr.UNDECIDED.values())))
    assert max(RATIOS.values()) <= 1.0 and not any(FLAGGED.values())

"""The constructions of tests/sweep_limits_cases.py, checked on the host: every planted run the GPU module asks for is placed,
the reference's GLRLM finds each of them where it was planted, and the planner replayed for 256 compute units changes its table
regime where the GPU module expects it to.  No device call is made."""
import os

import numpy as np
import pytest

import sweep_limits_cases as slc
import sweep_plan_cases as spc


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PRAD_"):
            monkeypatch.delenv(name)


@pytest.mark.parametrize("shape", slc.SCAN_SHAPES)
def test_regime_changes_include_the_required_ones(lib, shape):
    found = slc.regime_changes(lib, shape, cus=256)
    assert set(slc.REQUIRED[shape]) <= set(found), "regime changes of %s at 256 CUs: %s" % (shape, found)
    assert found == slc.SCAN_256[shape]                # the recorded lists (a device with 256 compute units reports the same)
    for lo, hi in found:                               # a change is a change of the key, and only of the key
        assert slc.regime_key(slc.plan_fields(lib, shape, lo, cus=256)) != slc.regime_key(slc.plan_fields(lib, shape, hi, cus=256))
    assert slc.plan_fields(lib, shape, 256, cus=256) == {"ok": 0}


def test_fields_name_the_record(lib):
    """the field names against a record whose values are known from the fixture of tests/test_sweep_plan.py"""
    f = slc.plan_fields(lib, (130, 64, 512), 64, cus=256)
    rec = spc.plan(lib, np.array(spc.NAMED["fw2_512_ng64"], np.int32))
    assert f == slc.fields(rec)
    assert (f["Nz"], f["Ny"], f["Nx"], f["fw2"], f["fused"], f["skip1"], f["lines_count"]) == (130, 64, 512, 1, 0, 1, 12)
    assert rec[len(slc.FIELDS) - 1] == 12 and slc.is_x(spc.angle_list(lib, [130, 64, 512], 0)[f["row_slot"]])
    assert slc.expected_variant(f) == ("sweep", "fw2") and slc.expected_variant({"ok": 0}) == ("pairs", "pairs")


@pytest.mark.parametrize("name", list(slc.PLANTED))
def test_every_requested_run_is_placed_and_found_by_the_reference(lib, oracle_port, name):
    c = slc.planted_case(lib, name, cus=256)
    f = c["plan"]
    fused, fw, fw2, fw2_rows, xrole = slc.REACHES[name]
    assert (f["ok"], f["fused"], f["fw"], f["fw2"], f["fw2_rows"], f["fw_xblocks"] > 0) == (1, fused, fw, fw2, fw2_rows, xrole), f
    assert c["tables"], "no table of this plan has a long-run path"
    assert c["reqs"] and not c["missing"], "not placed: %s" % c["missing"]
    assert len(c["placed"]) == len(c["reqs"])
    # every table's every angle has all of its lengths and kinds ...
    only = c["only"]
    for tname, role, rs, fused_t in c["tables"]:
        ais = [i for i, a in enumerate(c["angles"]) if slc.is_x(a) == (role == "x")]
        if only and tname in only:
            ais = only[tname]
            assert sorted(tuple(int(v) for v in c["angles"][i]) for i in ais) == sorted(slc.ONLY_ANGLES[name])
            assert all(c["shape"][d] >= rs + 2 + 7 for i in ais for d in range(2) if c["angles"][i][d])      # lines that long
        else:
            assert len(ais) == (1 if role == "x" else 12)
        for ai in ais:
            got = {(L, k) for t, a, L, k, _lv, _s in c["placed"] if t == tname and a == ai}
            want = {(L, "free") for L in range(rs - 1, rs + 3) if L >= 1} | {(rs + 1, "edge"), (max(rs, 2), "masked"), (rs + 2, "step7")}
            if fused_t:
                want |= {(L, "free") for L in range(rs + 63, rs + 67)}
            assert got == want, (tname, ai)
    # ... the top level is planted, planted levels are of the upper half, the background of the lower
    levels = {lv for *_r, lv, _s in c["placed"]}
    assert c["Ng"] in levels and min(levels) > c["Ng"] // 2
    # ... and each run is what it claims to be, voxel by voxel
    img, mask, shape = c["img"], c["mask"], c["shape"]
    for _t, ai, L, kind, lv, s in c["placed"]:
        a = [int(v) for v in c["angles"][ai]]
        line = [tuple(s[d] + k * a[d] for d in range(3)) for k in range(-1, L + 1)]
        assert all(img[p] == lv and mask[p] for p in line[1:-1])
        for p in (line[0], line[-1]):
            inside = all(0 <= v < n for v, n in zip(p, shape))
            assert not inside or not mask[p] or img[p] <= c["Ng"] // 2
        after_inside = all(0 <= v < n for v, n in zip(line[-1], shape))
        if kind == "edge":
            assert not after_inside
        if kind == "masked":
            assert after_inside and not mask[line[-1]]
        if kind == "step7":
            assert s[next(d for d in range(3) if a[d])] == 7 and L >= 2
    glrlm, ang = oracle_port.calculate_glrlm(img, mask, c["Ng"], c["Nr"], False, 0)
    assert np.array_equal(ang, c["angles"])
    assert slc.construction_errors(glrlm[0], c["placed"], c["Ng"]) == []
    assert slc.longest_run(img, mask, c["angles"]) == max(L for _t, _a, L, *_r in c["placed"])


def test_a_clipped_or_merged_construction_is_reported(lib, oracle_port):
    """the check that guards the GPU tests against a broken construction does fire: a run cut in two, two runs merged"""
    shape, Ng = (20, 22, 70), 36
    angles = spc.angle_list(lib, list(shape), 0)
    reqs = [("T", ai, L, "free") for ai in range(13) for L in (5, 6)]
    img, mask, placed, missing = slc.plant(shape, Ng, angles, reqs, seed=3)
    assert not missing
    g = oracle_port.calculate_glrlm(img, mask, Ng, 70, False, 0)[0][0]
    assert slc.construction_errors(g, placed, Ng) == []
    _t, ai, L, _k, lv, s = placed[4]
    cut = img.copy()
    a = [int(v) for v in angles[ai]]
    cut[tuple(s[d] + 2 * a[d] for d in range(3))] = 1
    assert slc.construction_errors(oracle_port.calculate_glrlm(cut, mask, Ng, 70, False, 0)[0][0], placed, Ng)
    merged = img.copy()
    merged[tuple(s[d] - a[d] for d in range(3))] = lv       # one voxel longer
    merged_mask = mask.copy()
    merged_mask[tuple(s[d] - a[d] for d in range(3))] = True
    assert slc.construction_errors(oracle_port.calculate_glrlm(merged, merged_mask, Ng, 70, False, 0)[0][0], placed, Ng)


@pytest.mark.parametrize("Ng", [64, 126, 170])
def test_isolated_voxels_have_runs_of_length_one_only(lib, oracle_port, Ng):
    shape = (9, 11, 130)
    img, mask, planted = slc.isolated(shape, Ng, seed=Ng)
    spots = {p for _lv, p in planted}
    for z in (0, 4, 8):
        for y in (0, 5, 10):
            for x in (0, 65, 129):
                assert (z, y, x) in spots
    assert len(planted) > 60 and Ng in {lv for lv, _p in planted}
    g, ang = oracle_port.calculate_glrlm(img, mask, Ng, 130, False, 0)
    assert g[0][Ng // 2:, 1:, :].sum() == 0
    assert (g[0][Ng // 2:, 0, :].sum(axis=0) == len(planted)).all()
    near_masked = sum(1 for _lv, p in planted if not mask[max(0, p[0] - 1):p[0] + 2, max(0, p[1] - 1):p[1] + 2, max(0, p[2] - 1):p[2] + 2].all())
    assert near_masked >= len(planted) // 3


def test_longest_run_and_noise(lib):
    shape = (7, 9, 40)
    angles = spc.angle_list(lib, list(shape), 0)
    img = np.arange(7 * 9 * 40, dtype=np.int32).reshape(shape) % 5 + 1          # x runs of 1; (z, y) steps repeat 40 = 0 mod 5
    mask = np.ones(shape, bool)
    assert slc.longest_run(img, mask, angles) == 9                              # along y (and z: 7): whole lines
    mask[:, 4, :] = False
    assert slc.longest_run(img, mask, angles) == 7
    for Ng in (1, 2, 37, 256):
        im, mk = slc.noise((12, 10, 64), Ng, seed=Ng)
        assert set(np.unique(im[mk])) == set(range(1, Ng + 1))
    im, mk = slc.smooth((12, 10, 64), 40, seed=1)
    assert mk.all() and im.min() >= 1 and im.max() <= 40 and slc.longest_run(im, mk, angles) >= 4

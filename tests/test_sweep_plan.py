"""The sweep planner (csrc/prad_sweep_plan.h plan_sweep) against the plans recorded in tests/golden/sweep_plans.npz: table choice,
LDS bytes, workgroups per role, piece lengths and the rest of the plan record (include/pyradiomics_amd.h,
prad_debug_sweep_plan) for a grid that has both sides of every threshold of the planner.  Host only: no device call is made."""
import os

import numpy as np
import pytest

import sweep_plan_cases as spc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "sweep_plans.npz")


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PRAD_"):
            monkeypatch.delenv(name)


def _named(golden, i):
    names = list(spc.NAMED)
    j = i - (len(golden["cases"]) - len(names))
    return golden["record_" + names[j]] if j >= 0 else None


def test_grid_is_the_recorded_one(lib, golden):
    """the fixture holds every case of the grid, in order, and the switches it names; only a shape that has no such angle
    list (an edge of one voxel has no x angle, a 1-D call no other) is left out"""
    assert list(golden["switches"]) == spc.SWITCHES
    grid = spc.grid()
    cases = golden["cases"]
    assert len(golden["digests"]) == len(cases)
    have = {tuple(c) for c in cases.tolist()}
    missing = [c for c in grid if tuple(c.tolist()) not in have]
    assert len(cases) + len(missing) == len(grid)
    assert all(len(spc.angle_list(lib, spc.size_of(c), int(c[6]))) == 0 for c in missing)


def test_plans_match_the_recorded_ones(lib, golden):
    cases, digests = golden["cases"], golden["digests"]
    switches = list(golden["switches"])
    records = spc.replay(lib, cases, switches)
    assert all(r is not None for r in records)          # no golden case is skipped
    bad = [i for i, r in enumerate(records) if spc.digest(r) != digests[i]]
    for i in bad[:10]:
        sw = switches[cases[i][8]] if cases[i][8] >= 0 else "-"
        print("case %d %s (Nz Ny Nx Ng nr_delta wants alist cus switch) list=%s switch=%s" % (
            i, cases[i].tolist(), spc.ANGLE_LISTS[cases[i][6]], sw))
        print("  new record:", records[i].tolist())
        if _named(golden, i) is not None:
            print("  recorded:  ", _named(golden, i).tolist())
    assert not bad, "%d of %d plans differ from the recorded ones" % (len(bad), len(cases))


def test_named_records(lib, golden):
    """the named cases record for record (the digests of the other test, readable)"""
    n = len(golden["cases"]) - len(spc.NAMED)
    for j, name in enumerate(spc.NAMED):
        got = spc.plan(lib, golden["cases"][n + j], list(golden["switches"]))
        assert got.tolist() == golden["record_" + name].tolist(), name


def test_refused_calls(lib, golden):
    """ok == 0 for lists the sweeps do not take and for Nr below the longest edge (GLRLM wanted)"""
    cases = golden["cases"]
    refused = [c for c in cases if c[6] in spc.REFUSED_LISTS or (c[4] < 0 and c[5] & 2)]
    assert len(refused) > 400
    for lst in spc.REFUSED_LISTS:
        assert any(c[6] == lst for c in refused)
    for r, c in zip(spc.replay(lib, refused), refused):
        assert r.tolist() == [0], c.tolist()
    # ... and the same shapes plan with Nr = the longest edge and the unit list
    fine = [c for c in cases if c[6] == 0 and c[4] == 0 and c[3] == 32 and c[8] < 0]
    assert fine and all(r[0] == 1 for r in spc.replay(lib, fine))


# switches of experiments that were measured and not adopted: the library no longer reads them (scripts/README.md)
RETIRED = ["PRAD_FINALIZE_STREAM", "PRAD_FIN_PLACE", "PRAD_FORCE_FW2", "PRAD_FW_EXTRA_FIRST", "PRAD_FW2_KEEP8", "PRAD_FW2_LANES",
           "PRAD_FW_MINVOX", "PRAD_NO_FW16"]


@pytest.mark.parametrize("name", RETIRED)
def test_retired_switches_change_nothing(lib, golden, monkeypatch, name):
    """a retired variable, set, leaves the default record of every named case and of every case the switches are flipped on
    unchanged (PRAD_FW_MINVOX gets a voxel count above all of them, the others 1).  This sees the planner only, so it can fail
    for PRAD_FORCE_FW2, PRAD_FW_EXTRA_FIRST, PRAD_FW_MINVOX and PRAD_NO_FW16; the other four never entered a plan (they acted in
    the pipeline and the finalize), and what holds for them is that their names no longer occur under pyradiomics_amd/"""
    n = len(golden["cases"]) - len(spc.NAMED)
    cases = [np.array(shp + (0, 3, 0, 256, -1), np.int32) for shp in spc.SWITCH_SHAPES] + list(golden["cases"][n:])
    before = spc.replay(lib, cases)
    monkeypatch.setenv(name, "1000000000" if name == "PRAD_FW_MINVOX" else "1")
    after = spc.replay(lib, cases)
    for c, a, b in zip(cases, before, after):
        assert a.tolist() == b.tolist(), c.tolist()


def test_record_capacity(lib):
    """a record that does not fit is not written: the count needed comes back negative"""
    case = np.array(spc.NAMED["fw_256_ng32"], np.int32)
    full = spc.plan(lib, case)
    import ctypes as C
    size = spc.size_of(case)
    angles = np.ascontiguousarray(spc.angle_list(lib, size, 0))
    out = np.full(8, -7, np.int32)
    n = lib.prad_debug_sweep_plan((C.c_int * 3)(*size), 3, angles.ctypes.data_as(C.POINTER(C.c_int)), len(angles), 32, max(size),
                                  1, 1, 256, out.ctypes.data_as(C.POINTER(C.c_int)), 8)
    assert n == -len(full) and (out == -7).all()

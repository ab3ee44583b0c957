"""Records tests/golden/sweep_plans.npz: what the sweep planner decides for the grid of tests/sweep_plan_cases.py.

    python tests/golden/make_sweep_plans.py

Host only (prad_debug_sweep_plan makes no device call).  Per case the fixture keeps the case and an 8-byte digest of its record;
for the named cases the whole record.

The committed fixture has two origins, and tests/test_sweep_plan.py holds every later planner to both.  The 14 890 cases whose Ng
is not one of those named below are the planner's behaviour BEFORE it was taken apart into csrc/prad_sweep_plan.h: they were
recorded from the commit before that change (b5d5949, "Finalize and zero inside the next walk launch: one launch per volume"),
whose plan_sweep was left untouched, plus tests/golden/sweep_plan_recorder.patch: the patch adds prad_debug_sweep_plan there (with
a thread-local override of cu_count() for `cus`) and nothing else.  The cases with Ng = 36, 37, 95, 96, 125, 126, 157, 158, 170 and
171 (the counts at which the planner changes its table regime) were added later and come from the CURRENT planner: the whole file
was recorded again here, every one of the older cases kept its digest, and the switch list and the named records stayed equal
(profiles/sweep_limits_measurements.md).  To record the grid from the old planner, from the repository root:

    git worktree add ../prad_parent b5d5949
    git -C ../prad_parent apply "$PWD/tests/golden/sweep_plan_recorder.patch"
    cp tests/sweep_plan_cases.py ../prad_parent/tests/
    cp tests/golden/make_sweep_plans.py ../prad_parent/tests/golden/
    python ../prad_parent/tests/golden/make_sweep_plans.py      # builds that tree, writes its tests/golden/sweep_plans.npz
    cp ../prad_parent/tests/golden/sweep_plans.npz tests/golden/ && python -m pytest tests/test_sweep_plan.py

Run here instead, it records what the CURRENT planner decides: do that only for a change that is meant to alter plans."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import sweep_plan_cases as spc  # noqa: E402


def main():
    for name in list(os.environ):
        if name.startswith("PRAD_"):
            del os.environ[name]
    from pyradiomics_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    cases = spc.grid()
    records = spc.replay(lib, cases)
    keep = np.array([r is not None for r in records])
    cases = cases[keep]
    records = [r for r in records if r is not None]
    out = {"cases": cases, "switches": np.array(spc.SWITCHES), "digests": np.array([spc.digest(r) for r in records], dtype="<u8")}
    names = list(spc.NAMED)
    first_named = len(cases) - len(names)
    for i, name in enumerate(names):
        assert tuple(cases[first_named + i]) == spc.NAMED[name]
        out["record_" + name] = records[first_named + i]
    path = os.path.join(HERE, "sweep_plans.npz")
    np.savez_compressed(path, **out)
    ok = sum(int(r[0]) for r in records)
    print("%d cases (%d planned, %d refused), %d bytes" % (len(cases), ok, len(cases) - ok, os.path.getsize(path)))


if __name__ == "__main__":
    main()

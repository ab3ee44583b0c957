"""Does the GLSZM cost the same from a unit of its own (csrc/prad_glszm.hip) as it did inside prad_api.hip?
(profiles/glszm_unit_measurements.md)  With --set neigh: do GLDM / NGTDM cost the same through their planner (neigh_rows below)?

Measured per process, on the volumes of bench.py's config 2 (make_volume, 32 levels, full mask):
  glszm-<size>-<dist>   engine.glszm_compact at 256^3 and 512^3, uniform and smooth levels: device ms of the call
                        (HIP events, engine.last_device_ms) -- median of --reps after a warm-up -- and the wall ms beside it
  case-1thread          wall ms of one case of the product route on ONE host thread (bench.py's batch case: 256^3, ball ROI,
                        Original + Wavelet, RadiomicsFeatureExtractor.execute); the GLSZM is its critical stream
The library is chosen when a process starts, so the two libraries ALTERNATE as child processes of one run, parent library first:

    python scripts/glszm_unit_probe.py --parent-lib /path/to/parent/libpyradiomics_amd.so --alternations 5 --out glszm_unit.json
    python scripts/glszm_unit_probe.py --out glszm_unit.json            # this tree alone (no comparison is made)
    PRAD_LIB=/path/to/libpyradiomics_amd.so python scripts/glszm_unit_probe.py --child      # one process, one JSON line

Every value of every process is reported.  The verdict per row: the median of this tree's values lies inside the spread
(min .. max) of the parent library's values from the same run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES, DISTS, LEVELS = (256, 512), ("uniform", "smooth"), 32
NEW_SYMBOLS = ("prad_debug_glszm_route", "prad_debug_neigh_plan")      # what a library built from an earlier commit may not have


def timed(call, reps):
    """-> (median device ms, median wall ms) of `call` after one warm-up"""
    import torch
    from pyradiomics_amd import engine
    call()
    dev, wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(engine.last_device_ms())
    return float(np.median(dev)), float(np.median(wall))


def glszm_rows(row, device, reps):
    import bench
    from pyradiomics_amd import engine
    for size in SIZES:
        for dist in DISTS:
            img, msk = bench.make_volume(size, LEVELS, dist, 0, device)
            n = img.numel()
            row["glszm-%d-%s" % (size, dist)], row["glszm-%d-%s wall" % (size, dist)] = timed(lambda: engine.glszm_compact(img, msk, LEVELS, n), reps)
            del img, msk


def neigh_rows(row, device, reps):
    """GLDM / NGTDM (profiles/neigh_route_measurements.md): the byte tier at 256^3 and 32 levels, the pairs tier at 300 levels and
    distances (1, 2) -- NGTDM through the box sums and, with PRAD_NGTDM_NO_BOX=1 for those calls, without -- and the three calls at
    32^3, wall ms only: host-bound, a planner's cost would show there"""
    import bench
    from pyradiomics_amd import engine
    img, msk = bench.make_volume(256, LEVELS, "uniform", 0, device)
    for name, call in (("gldm", engine.gldm), ("ngtdm", engine.ngtdm), ("gldm_ngtdm", engine.gldm_ngtdm)):
        row["%s-256" % name], row["%s-256 wall" % name] = timed(lambda: call(img, msk, LEVELS), reps)
    img, msk = bench.make_volume(256, 300, "uniform", 0, device)
    row["gldm-256-300-d12"], row["gldm-256-300-d12 wall"] = timed(lambda: engine.gldm(img, msk, 300, distances=(1, 2)), reps)
    row["ngtdm-256-300-d12-box"], row["ngtdm-256-300-d12-box wall"] = timed(lambda: engine.ngtdm(img, msk, 300, distances=(1, 2)), reps)
    os.environ["PRAD_NGTDM_NO_BOX"] = "1"
    row["ngtdm-256-300-d12-nobox"], row["ngtdm-256-300-d12-nobox wall"] = timed(lambda: engine.ngtdm(img, msk, 300, distances=(1, 2)), reps)
    del os.environ["PRAD_NGTDM_NO_BOX"]
    img, msk = bench.make_volume(32, LEVELS, "uniform", 0, device)
    for name, call in (("gldm", engine.gldm), ("ngtdm", engine.ngtdm), ("gldm_ngtdm", engine.gldm_ngtdm)):
        row["%s-32 wall" % name] = timed(lambda: call(img, msk, LEVELS), 20 * reps)[1]


SETS = {"glszm": glszm_rows, "neigh": neigh_rows}


def child(reps, cases, rows):
    from pyradiomics_amd import _lib
    if os.environ.get("PRAD_LIB"):
        for name in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(name, None)
    import torch
    import bench
    from pyradiomics_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    device = torch.device("cuda", 0)
    row = {"library": _lib.LIB_PATH}
    SETS[rows](row, device, reps)
    engine.release_workspace()             # (the 512^3 workspace: the case below runs in what a case needs)
    _, _, one = bench._batch_case_setup(device, 7000, 2)
    one(0)
    one(0)
    torch.cuda.synchronize()
    ms = []
    for _ in range(cases):
        t0 = time.perf_counter()
        one(1)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    row["case-1thread"] = float(np.median(ms))
    print("PROBE " + json.dumps(row), flush=True)


def run_child(lib, reps, cases, rows):
    env = dict(os.environ)
    env.pop("PRAD_LIB", None)
    if lib:
        env["PRAD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--cases", str(cases), "--set", rows]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in out.stdout.splitlines() if l.startswith("PROBE ")]
    if out.returncode != 0 or not lines:
        raise SystemExit("the child on %s failed (%d):\n%s\n%s" % (lib or "this tree", out.returncode, out.stdout[-2000:], out.stderr[-4000:]))
    return json.loads(lines[-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="measure in this process with the library PRAD_LIB names (default: the tree's)")
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit: alternate with it")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", type=int, default=3)
    ap.add_argument("--set", choices=sorted(SETS), default="glszm", help="which rows to measure in front of case-1thread")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.cases, args.set)
    if args.parent_lib and not os.path.exists(args.parent_lib):
        raise SystemExit("no library at %s: build the parent commit first" % args.parent_lib)
    runs = {"parent": [], "new": []}
    for i in range(args.alternations):          # a failing child ends the run: nothing more is started behind it
        if args.parent_lib:
            runs["parent"].append(run_child(args.parent_lib, args.reps, args.cases, args.set))
            print("alternation %d parent %s" % (i, json.dumps(runs["parent"][-1])), flush=True)
        runs["new"].append(run_child(None, args.reps, args.cases, args.set))
        print("alternation %d new    %s" % (i, json.dumps(runs["new"][-1])), flush=True)
    keys = [k for k in runs["new"][0] if k != "library"]
    table = []
    print("\n| measurement (ms) | parent: every value | parent min .. max | new: every value | new median | inside the parent's spread |")
    print("|---|---|---|---|---|---|")
    for k in keys:
        new = [r[k] for r in runs["new"]]
        old = [r[k] for r in runs["parent"]]
        med = float(np.median(new))
        inside = (min(old) <= med <= max(old)) if old else None
        table.append({"measurement": k, "parent": old, "new": new, "new_median": med, "inside_parent_spread": inside})
        fmt = lambda v: " ".join("%.3f" % x for x in v)        # noqa: E731
        print("| %s | %s | %s | %s | %.3f | %s |" % (k, fmt(old) or "—", ("%.3f .. %.3f" % (min(old), max(old))) if old else "—", fmt(new), med,
                                                  {True: "yes", False: "NO", None: "not compared"}[inside]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"runs": runs, "table": table}, f, indent=1)


if __name__ == "__main__":
    main()

"""Measurements of the LBP2D kernels (profiles/lbp2d_measurements.md).  Needs an MI355X; there is no fallback.

  single   256^3 int16 and float32, P = 8, R = 1, uniform, force2Ddimension 0, 1, 2: engine.lbp2d into a preallocated `out`,
           device events around a warm loop of `--loop` calls (time per call), the library's own events around the last launch
           (prad_last_kernel_ms), algorithmic bytes -- one read and one write per voxel -- over that time against the 8 TB/s
           peak; filters.lbp2d_host (numpy) on the same volume in the same process, once, after its result has been compared
           with the device's.
  batch    256 boxes of 32^3 and 1 024 boxes of 16^3, float32: (a) engine.lbp2d_batch into a preallocated `out`, (b) the loop of
           engine.lbp2d over the boxes and one synchronise; (a) and (b) alternate, wall time around a device synchronise, 2
           warm-up repetitions, median and min .. max of `--reps`.  Equal tensors are asserted before anything is timed.

    python scripts/lbp2d_probe.py [--out lbp2d_probe.json] [--reps 7] [--loop 20] [--no-host]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12


def _stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def single(engine, torch, dtype, axis, loop, host):
    rng = np.random.default_rng(1)
    vol = (rng.normal(300.0, 200.0, (256, 256, 256))).astype(dtype)
    x = torch.from_numpy(vol).cuda()
    out = torch.empty_like(x)
    for _ in range(3):
        engine.lbp2d(x, 1, 8, "uniform", axis, out=out)
    torch.cuda.synchronize()
    per_call = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(loop):
            engine.lbp2d(x, 1, 8, "uniform", axis, out=out)
        b.record()
        torch.cuda.synchronize()
        per_call.append(a.elapsed_time(b) / loop)
    kernel = engine.last_kernel_ms("lbp2d")
    bytes_ = 2 * vol.size * vol.itemsize
    rec = {"dtype": dtype, "axis": axis, "per_call_ms": _stats(per_call), "kernel_ms": kernel,
           "plan": engine.lbp2d_plan(vol.shape, axis, 1), "algorithmic_bytes": bytes_,
           "TBps": bytes_ / (min(per_call) * 1e-3) / 1e12, "share_of_peak": bytes_ / (min(per_call) * 1e-3) / PEAK}
    if host:
        from pyradiomics_amd import filters
        t0 = time.perf_counter()
        want = filters.lbp2d_host(vol, 1, 8, "uniform", axis)
        rec["host_ms"] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(out.cpu().numpy(), want), "device and host route differ"
        rec["equal_to_host"] = True
    return rec


def batch(engine, torch, B, n, reps):
    rng = np.random.default_rng(2)
    flat = torch.from_numpy(rng.normal(300.0, 200.0, B * n ** 3).astype(np.float32)).cuda()
    sizes = np.full((B, 3), n, dtype=np.intc)
    boxes = [flat[b * n ** 3:(b + 1) * n ** 3].view(n, n, n) for b in range(B)]
    out = torch.empty(B * n ** 3, dtype=torch.float64, device="cuda")
    outs = [torch.empty_like(b) for b in boxes]

    def a():
        engine.lbp2d_batch(flat, sizes, 1, 8, "uniform", 0, out=out)
        torch.cuda.synchronize()

    def b():
        for box, o in zip(boxes, outs):
            engine.lbp2d(box, 1, 8, "uniform", 0, out=o)
        torch.cuda.synchronize()

    a()
    b()
    assert torch.equal(out, torch.cat([o.reshape(-1) for o in outs]).to(torch.float64)), "batch and loop differ"
    ta, tb, ka = [], [], []
    for r in range(reps + 2):
        for fn, acc in ((a, ta), (b, tb)):
            t0 = time.perf_counter()
            fn()
            if r >= 2:
                acc.append((time.perf_counter() - t0) * 1e3)
            if fn is a and r >= 2:
                ka.append(engine.last_kernel_ms("batch_lbp2d"))
    bytes_ = B * n ** 3 * (4 + 8)
    return {"B": B, "box": n, "batch_ms": _stats(ta), "loop_ms": _stats(tb), "ratio": statistics.median(tb) / statistics.median(ta),
            "kernel_ms": _stats(ka), "algorithmic_bytes": bytes_, "TBps": bytes_ / (min(ka) * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="lbp2d_probe.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    from pyradiomics_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    res = {"single": [], "batch": []}
    for dtype in ("int16", "float32"):
        for axis in (0, 1, 2):
            rec = single(engine, torch, dtype, axis, args.loop, host=not args.no_host and axis == 0)
            print(json.dumps(rec), flush=True)
            res["single"].append(rec)
    for B, n in ((256, 32), (1024, 16)):
        rec = batch(engine, torch, B, n, args.reps)
        print(json.dumps(rec), flush=True)
        res["batch"].append(rec)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

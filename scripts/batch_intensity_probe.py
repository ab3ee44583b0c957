"""Times the intensity transforms and the Gradient image of many small boxes (profiles/batch_intensity_measurements.md):
  (a) engine.intensity_batch (Square, SquareRoot, Logarithm, Exponential) and engine.gradient_batch on the flat batch, into
      preallocated outputs,
  (b) the loops of filters.getSquareImage ... getExponentialImage and of filters.getGradientImage (deviceResident=True) over the
      same boxes (what a lesion table paid per ROI before).
Workloads: 256 boxes of 32^3 and 1024 boxes of 16^3, float32 and int16, unit spacing.  (a) and (b) alternate in ONE process; wall
time around a device synchronise, warm-up first, median and spread (min .. max) of --reps repetitions.  The probe asserts that
(a) and (b) give equal square, squareroot and gradient tensors before it times anything.  The kernel time of (a)
(prad_last_kernel_ms "batch_intensity": both launches) gives the achieved bytes/s over the algorithmic bytes -- the input read
once, 8 B written per voxel and pointwise row, 4 B per voxel for Gradient -- and their share of the 8 TB/s peak.

    python scripts/batch_intensity_probe.py --out batch_intensity.json                          # (a), (b), kernel time
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/batch_intensity_probe.py --trace    # (a) alone, for kernel times
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [(256, (32, 32, 32)), (1024, (16, 16, 16))]
DTYPES = ("float32", "int16")
SPACING = (1.0, 1.0, 1.0)
PEAK_BYTES_PER_S = 8.0e12


def _wall(fns, reps, warmup):
    """the callables of `fns` alternated: per name the wall ms of each repetition, around a device synchronise"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": reps} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", action="store_true", help="(a) alone, a few times: for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pyradiomics_amd import _lib, engine, filters
    from pyradiomics_amd.image import Image
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    lib = _lib.load()
    result = {"library": _lib.LIB_PATH, "version": lib.prad_version().decode(), "workloads": []}
    pointwise = (filters.getSquareImage, filters.getSquareRootImage, filters.getLogarithmImage, filters.getExponentialImage)
    for dtype in DTYPES:
        for B, shape in WORKLOADS:
            rng = np.random.default_rng(B)
            n = int(np.prod(shape))
            flat = torch.from_numpy((rng.standard_normal(B * n) * 300.0 + 40.0).astype(dtype)).cuda()
            size = flat.element_size()
            sizes = np.tile(np.array(shape, dtype=np.intc), (B, 1))
            boxes = [flat[b * n:(b + 1) * n].view(shape) for b in range(B)]
            out = torch.empty((4, B * n), dtype=torch.float64, device="cuda")
            out_grad = torch.empty(B * n, dtype=torch.float32, device="cuda")
            row = {"dtype": dtype, "B": B, "shape": list(shape), "voxels": B * n,
                   "algorithmic_bytes": {"intensity": B * n * (size + 4 * 8), "gradient": B * n * (size + 4)}}

            def intensity():
                return engine.intensity_batch(flat, sizes, out=out)

            def gradient():
                return engine.gradient_batch(flat, sizes, SPACING, out=out_grad)

            def intensity_loop():
                return [next(fn(Image(tensor=x), None, deviceResident=True))[0].device_tensor() for x in boxes for fn in pointwise]

            def gradient_loop():
                return [next(filters.getGradientImage(Image(tensor=x), None, deviceResident=True))[0].device_tensor() for x in boxes]

            if args.trace:
                for _ in range(3):
                    intensity()
                    gradient()
                torch.cuda.synchronize()
                continue
            out.fill_(float("nan"))
            out_grad.fill_(float("nan"))
            intensity()
            assert engine.last_batch_route() == "batch"
            gradient()
            assert engine.last_batch_route() == "batch"
            single = intensity_loop()
            for r in (0, 1):
                assert torch.equal(out[r], torch.cat([im.reshape(-1) for im in single[r::4]])), "row %d differs from the loop's" % r
            for r in (2, 3):
                assert torch.allclose(out[r], torch.cat([im.reshape(-1) for im in single[r::4]]), rtol=1e-14, atol=1e-12)
            assert torch.equal(out_grad, torch.cat([im.reshape(-1) for im in gradient_loop()])), "the gradient differs from the loop's"
            t = _wall({"intensity": intensity, "intensity_loop": intensity_loop, "gradient": gradient, "gradient_loop": gradient_loop},
                      args.reps, args.warmup)
            row["wall"] = t
            row["loop_over_batched"] = {"intensity": t["intensity_loop"]["median_ms"] / t["intensity"]["median_ms"],
                                        "gradient": t["gradient_loop"]["median_ms"] / t["gradient"]["median_ms"]}
            row["kernel_ms"], row["bytes_per_s"], row["share_of_peak"] = {}, {}, {}
            for name, fn in (("intensity", intensity), ("gradient", gradient)):
                ks = []
                for _ in range(args.reps):
                    fn()
                    ks.append(engine.last_kernel_ms("batch_intensity"))
                row["kernel_ms"][name] = {"median_ms": float(np.median(ks)), "min_ms": float(min(ks)), "max_ms": float(max(ks))}
                rate = row["algorithmic_bytes"][name] / (float(np.median(ks)) * 1e-3)
                row["bytes_per_s"][name], row["share_of_peak"][name] = rate, rate / PEAK_BYTES_PER_S
            result["workloads"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""Times the resampling of many small boxes (profiles/batch_resample_measurements.md):
  raw      (a) engine.resample_boxes_batch on the flat batch, image and mask together, into preallocated outputs,
           (b) the loop of engine.resample(box, ...) for the image (cubic B-spline) and the mask (nearest) over the same boxes;
  planned  (a) engine.resample_batch (mask boxes, plan, prefilter, evaluation),
           (b) the loop of imageoperations.resampleImage(deviceResident=True) on every box as an Image (what a lesion table paid
               per ROI before).
Workloads: 256 boxes of 32^3 and 1024 boxes of 16^3; float32 and int16; cubic B-spline; spacing 1 -> 2 (down-sampling) and
2 -> 1 (up-sampling), the raw call on the grid resampleImage makes for a mask that fills the box.  (a) and (b) alternate in ONE
process; wall time around a device synchronise, warm-up first, median and spread (min .. max) of --reps repetitions.  The probe
asserts that (a) and (b) give equal tensors before it times anything.  The kernel time of the raw (a) (prad_last_kernel_ms
"batch_resample") gives the achieved bytes/s over the algorithmic bytes -- per input voxel the image element and the mask byte
read once and the float64 coefficient written once and read once, per output voxel the image element and the mask byte
written -- and their share of the 8 TB/s peak.

    python scripts/batch_resample_probe.py --out batch_resample.json                     # this tree
    PRAD_LIB=/path/to/parent/libpyradiomics_amd.so python scripts/batch_resample_probe.py --single-only --out parent.json
                                                     # the loops on a library built from the parent commit (no batched symbols)
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/batch_resample_probe.py --trace      # raw (a) alone
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
GRIDS = (("1to2", 1.0, 2.0), ("2to1", 2.0, 1.0))
PAD = 5
PEAK_BYTES_PER_S = 8.0e12
NEW_SYMBOLS = ("prad_batch_mask_boxes_dev", "prad_batch_resample_dev", "prad_batch_resample_max_vox")


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--single-only", action="store_true", help="the loops alone: the library has no batched resampling entry points")
    ap.add_argument("--trace", action="store_true", help="the raw batched call alone, a few times: for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pyradiomics_amd import _lib
    if args.single_only:
        for name in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(name, None)
    import torch
    from pyradiomics_amd import engine, imageoperations
    from pyradiomics_amd.image import Image
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    lib = _lib.load()
    result = {"library": _lib.LIB_PATH, "version": lib.prad_version().decode(), "workloads": []}
    for B, shape in WORKLOADS:
        n = int(np.prod(shape))
        sizes = np.tile(np.array(shape, dtype=np.intc), (B, 1))
        m = np.zeros(shape, dtype=np.uint8)
        m[tuple(slice(s // 4, s - s // 4) for s in shape)] = 1                      # the middle half of every axis
        fmask = torch.from_numpy(np.tile(m.reshape(-1), B)).cuda()
        for dtype in DTYPES:
            rng = np.random.default_rng(B)
            flat = torch.from_numpy((rng.standard_normal(B * n) * 300.0 + 500.0).astype(dtype)).cuda()
            boxes = [flat[b * n:(b + 1) * n].view(shape) for b in range(B)]
            masks = [fmask[b * n:(b + 1) * n].view(shape) for b in range(B)]
            for grid, old, new in GRIDS:
                ratio = old / new
                newsize = np.tile(np.array([int(np.ceil(s * ratio)) for s in shape], dtype=np.intc), (B, 1))
                start = np.full((B, 3), 0.5 * (new - old) / old)
                step = np.full((B, 3), new / old)
                nout = int(newsize[0].astype(np.int64).prod())
                esize = np.dtype(dtype).itemsize
                row = {"B": B, "shape": list(shape), "dtype": dtype, "grid": grid, "newsize": newsize[0].tolist(),
                       "algorithmic_bytes": B * (n * (esize + 1 + 16) + nout * (esize + 1))}
                out = torch.empty(B * nout, dtype=flat.dtype, device="cuda")
                out_m = torch.empty(B * nout, dtype=torch.uint8, device="cuda")

                def raw_batched():
                    return engine.resample_boxes_batch(flat, sizes, start, step, newsize, 3, masks=fmask, out=out, out_masks=out_m)

                def raw_loop():
                    return [(engine.resample(x, start[0], step[0], newsize[0], 3), engine.resample(k, start[0], step[0], newsize[0], 0))
                            for x, k in zip(boxes, masks)]

                def planned_batched():
                    return engine.resample_batch(flat, fmask, sizes, (old,) * 3, (new,) * 3, "sitkBSpline", PAD)

                def planned_loop():
                    return [imageoperations.resampleImage(Image(None, (old,) * 3, tensor=x), Image(None, (old,) * 3, tensor=k),
                                                          resampledPixelSpacing=(new,) * 3, padDistance=PAD, deviceResident=True)
                            for x, k in zip(boxes, masks)]

                if args.trace:
                    for _ in range(3):
                        raw_batched()
                    torch.cuda.synchronize()
                    continue
                if args.single_only:
                    t = _wall({"raw": raw_loop, "planned": planned_loop}, args.reps, args.warmup)
                    row["raw_b_loop"], row["planned_b_loop"] = t["raw"], t["planned"]
                else:
                    out.fill_(0)
                    raw_batched()
                    assert engine.last_batch_route() == "batch"
                    want = raw_loop()
                    assert torch.equal(out, torch.cat([i.reshape(-1) for i, _ in want])), "batched images differ from the loop's"
                    assert torch.equal(out_m, torch.cat([k.reshape(-1) for _, k in want])), "batched masks differ from the loop's"
                    got = planned_batched()
                    assert engine.last_batch_route() == "batch"
                    want = planned_loop()
                    assert torch.equal(got[0], torch.cat([i.device_tensor().reshape(-1) for i, _ in want])), "resample_batch differs"
                    assert torch.equal(got[1], torch.cat([k.device_tensor().reshape(-1).to(torch.uint8) for _, k in want]))
                    t = _wall({"ra": raw_batched, "rb": raw_loop, "pa": planned_batched, "pb": planned_loop}, args.reps, args.warmup)
                    row["raw_a_batched"], row["raw_b_loop"] = t["ra"], t["rb"]
                    row["planned_a_batched"], row["planned_b_loop"] = t["pa"], t["pb"]
                    row["raw_loop_over_batched"] = t["rb"]["median_ms"] / t["ra"]["median_ms"]
                    row["planned_loop_over_batched"] = t["pb"]["median_ms"] / t["pa"]["median_ms"]
                    ks = []
                    for _ in range(args.reps):
                        raw_batched()
                        ks.append(engine.last_kernel_ms("batch_resample"))
                    row["kernel_ms"] = {"median_ms": float(np.median(ks)), "min_ms": float(min(ks)), "max_ms": float(max(ks))}
                    rate = row["algorithmic_bytes"] / (float(np.median(ks)) * 1e-3)
                    row["bytes_per_s"], row["share_of_peak"] = rate, rate / PEAK_BYTES_PER_S
                result["workloads"].append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

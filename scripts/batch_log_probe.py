"""Times the LoG images of many small boxes (profiles/batch_log_measurements.md):
  (a) engine.log_batch on the flat batch, into a preallocated output,
  (b) the loop of engine.log_images(box, spacing, sigmas) over the same boxes (what a lesion table paid per ROI before).
Workloads: 256 boxes of 32^3 and 1024 boxes of 16^3, float32, spacing (1, 1, 1), sigmas (1, 2, 3).  (a) and (b) alternate in
ONE process; wall time around a device synchronise, warm-up first, median and spread (min .. max) of --reps repetitions.  The
probe asserts that (a) and (b) give equal tensors before it times anything.  The kernel time of (a) (prad_last_kernel_ms
"batch_log") gives the achieved bytes/s over the algorithmic bytes -- per voxel and sigma three reads of the input element and
one write of the result -- and their share of the 8 TB/s peak.

    python scripts/batch_log_probe.py --out batch_log.json                     # this tree: (a), (b), kernel time
    PRAD_LIB=/path/to/parent/libpyradiomics_amd.so python scripts/batch_log_probe.py --single-only --out parent.json
                                                     # (b) on a library built from the parent commit (no batched LoG symbols)
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/batch_log_probe.py --trace          # (a) alone, for kernel times
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [(256, (32, 32, 32)), (1024, (16, 16, 16))]
SIGMAS = (1.0, 2.0, 3.0)
SPACING = (1.0, 1.0, 1.0)
PEAK_BYTES_PER_S = 8.0e12
NEW_SYMBOLS = ("prad_batch_log_plan", "prad_batch_log_dev")


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
    ap.add_argument("--single-only", action="store_true", help="(b) alone: the library has no batched LoG entry points")
    ap.add_argument("--trace", action="store_true", help="(a) alone, a few times: for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pyradiomics_amd import _lib
    if args.single_only:
        for name in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(name, None)
    import torch
    from pyradiomics_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    lib = _lib.load()
    result = {"library": _lib.LIB_PATH, "version": lib.prad_version().decode(), "sigmas": list(SIGMAS), "workloads": []}
    for B, shape in WORKLOADS:
        rng = np.random.default_rng(B)
        n = int(np.prod(shape))
        flat = torch.from_numpy((rng.standard_normal(B * n) * 300.0 + 40.0).astype(np.float32)).cuda()
        sizes = np.tile(np.array(shape, dtype=np.intc), (B, 1))
        boxes = [flat[b * n:(b + 1) * n].view(shape) for b in range(B)]
        out = torch.empty((len(SIGMAS), B * n), dtype=torch.float32, device="cuda")
        row = {"B": B, "shape": list(shape), "voxels": B * n, "algorithmic_bytes": B * n * len(SIGMAS) * (3 * 4 + 4)}

        def batched():
            return engine.log_batch(flat, sizes, SIGMAS, SPACING, out=out)

        def loop():
            keep = []
            for x in boxes:
                keep.append(engine.log_images(x, SPACING[::-1], SIGMAS))
            return keep

        if args.trace:
            for _ in range(3):
                batched()
            torch.cuda.synchronize()
            continue
        if args.single_only:
            row.update({"b_loop": _wall({"b": loop}, args.reps, args.warmup)["b"]})
        else:
            out.fill_(float("nan"))
            _, _, _, valid = batched()
            assert engine.last_batch_route() == "batch" and valid.all()
            want = torch.stack([torch.cat([im.reshape(-1) for im in per_sigma]) for per_sigma in zip(*loop())])
            assert torch.equal(out, want), "the batched LoG images differ from the loop's"
            t = _wall({"a": batched, "b": loop}, args.reps, args.warmup)
            row["a_batched"], row["b_loop"] = t["a"], t["b"]
            row["loop_over_batched"] = t["b"]["median_ms"] / t["a"]["median_ms"]
            ks = []
            for _ in range(args.reps):
                batched()
                ks.append(engine.last_kernel_ms("batch_log"))
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

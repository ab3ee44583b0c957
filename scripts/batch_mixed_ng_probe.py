"""Times engine.roi_features_batch with a fixed bin width on a table of lesions whose ROIs differ in their grey-level counts
(profiles/batch_mixed_ng_measurements.md).  The call under test is
    engine.roi_features_batch(images, masks, sizes, binWidth=25)          # all six classes
on 256 boxes of 32^3 and 1 024 boxes of 16^3 (float32, integer-valued, masks ~60 % full, fixed seed) whose intensity ranges
give ROI b the count 25 + b % 40: 40 distinct Ng, all at most 64.  The number of distinct counts bin_batch finds is printed.
Wall time around a device synchronise, warm-up first, median and spread (min .. max) of --reps repetitions.

The yardstick is THIS FILE, unchanged, run in a checkout of the parent commit with its own build: the call exists there (it
evaluates the texture classes once per distinct count), so the probe needs no flag for the old route and imports whatever
tree it lies in.

Beside it, the no-regression check of the uniform path: the kernel time of the matrix launch (prad_last_kernel_ms "batch")
of engine.texture_matrices_batch with ONE count, Ng = 32, on boxes of the same shapes -- the scalar call of both trees.

    python scripts/batch_mixed_ng_probe.py --out batch_mixed_ng.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [(256, (32, 32, 32)), (1024, (16, 16, 16))]
BIN_WIDTH = 25
FIRST_COUNT, COUNTS = 25, 40          # ROI b gets FIRST_COUNT + b % COUNTS levels: 25 .. 64
UNIFORM_NG = 32


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pyradiomics_amd import _lib, engine
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    lib = _lib.load()
    result = {"library": _lib.LIB_PATH, "version": lib.prad_version().decode(), "binWidth": BIN_WIDTH, "workloads": []}
    for B, shape in WORKLOADS:
        rng = np.random.default_rng(B)
        n = int(np.prod(shape))
        want = FIRST_COUNT + np.arange(B) % COUNTS
        img = np.floor(rng.random((B, n)) * (BIN_WIDTH * want)[:, None]).astype(np.float32)
        msk = rng.random((B, n)) < 0.6
        img[:, 0], img[:, 1], msk[:, :2] = 0.0, BIN_WIDTH * want - 1.0, True          # the whole range occurs in every ROI
        flat, mask = torch.from_numpy(img.reshape(-1)).cuda(), torch.from_numpy(msk.reshape(-1).view(np.uint8)).cuda()
        sizes = np.tile(np.array(shape, dtype=np.intc), (B, 1))
        _, Ng, _, _ = engine.bin_batch(flat, mask, sizes, binWidth=BIN_WIDTH)
        row = {"B": B, "shape": list(shape), "distinct_Ng": int(len(set(Ng.tolist()))), "min_Ng": int(Ng.min()), "max_Ng": int(Ng.max())}
        assert np.array_equal(Ng, want), "the intensity ranges do not give the counts they were chosen for"

        def call():
            return engine.roi_features_batch(flat, mask, sizes, binWidth=BIN_WIDTH)

        table, status = call()
        row["route"] = engine.last_batch_route()
        assert status == [1] * B and sorted(table) == sorted(engine.ROI_FEATURE_CLASSES)
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        row["roi_features_batch"] = _stats(ms)

        # the uniform path: the matrix launch of one count on boxes of the same shapes
        levels = torch.from_numpy(rng.integers(1, UNIFORM_NG + 1, B * n).astype(np.int32)).cuda()
        ks = []
        for k in range(args.warmup + args.reps):
            _, st = engine.texture_matrices_batch(levels, mask, sizes, UNIFORM_NG)
            assert engine.last_batch_route() == "batch" and st == [1] * B
            if k >= args.warmup:
                ks.append(engine.last_kernel_ms("batch"))
        row["uniform_ng32_kernel"] = _stats(ks)
        result["workloads"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""Timing probe of the batched first-order statistics and discretisation (profiles/batch_firstorder_measurements.md).

    python scripts/batch_firstorder_probe.py --side batch                          # this tree's library
    PRAD_LIB=<library built from the parent commit> python scripts/batch_firstorder_probe.py --side single

Workloads: 256 ROIs of 32^3 and 1024 ROIs of 16^3, float32 and int16 images, mask fill 0.6, binWidth 25, fixed seed.  HIP events
around each repetition, 3 warm-up repetitions and 20 timed ones; median, minimum and maximum in ms, one JSON line per workload.
  --side batch    engine.firstorder_batch + engine.bin_batch end to end (two launches, two read-backs, the host edges), plus the
                  device time of the "batch_firstorder" kernel family of one more repetition
  --side single   the loop of engine.firstorder_stats + engine.bin_image(with_counts=True) over the same ROIs; uses only calls
                  the parent commit has, so PRAD_LIB can point at a build of it: the new code is never its own yardstick
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyradiomics_amd import _lib  # noqa: E402

# a library of an earlier commit lacks the newest entry points: drop them from the ctypes table before it is loaded
_probe = ctypes.CDLL(_lib.LIB_PATH)
for _name in [n for n in _lib.SYMBOLS if not hasattr(_probe, n)]:
    del _lib.SYMBOLS[_name]

from pyradiomics_amd import engine  # noqa: E402

WORKLOADS = [(256, 32, np.float32), (1024, 16, np.float32), (256, 32, np.int16), (1024, 16, np.int16)]
WARMUP, REPS, BIN_WIDTH = 3, 20, 25


def _batch(B, n, dtype, seed=1):
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    vals = rng.standard_normal(B * n ** 3) * 150 + 300          # ~ 40 bins of width 25 per ROI
    images = torch.from_numpy(vals.astype(dtype)).to(dev)
    masks = torch.from_numpy((rng.random(B * n ** 3) < 0.6).view(np.uint8)).to(dev)
    return images, masks, np.array([(n, n, n)] * B, dtype=np.intc)


def _timed(fn):
    times = []
    for rep in range(WARMUP + REPS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if rep >= WARMUP:
            times.append(t0.elapsed_time(t1))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def _batched(images, masks, sizes):
    stats = engine.firstorder_batch(images, masks, sizes)
    return engine.bin_batch(images, masks, sizes, stats=stats, binWidth=BIN_WIDTH)


def _single_loop(rois):
    for img, msk in rois:
        engine.firstorder_stats(img, msk)
        engine.bin_image(img, msk, with_counts=True, binWidth=BIN_WIDTH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("batch", "single"), required=True)
    args = ap.parse_args()
    for B, n, dtype in WORKLOADS:
        images, masks, sizes = _batch(B, n, dtype)
        line = {"side": args.side, "B": B, "box": n, "dtype": np.dtype(dtype).name, "lib": os.path.basename(_lib.LIB_PATH)}
        if args.side == "batch":
            line.update(_timed(lambda: _batched(images, masks, sizes)))
            line["route"] = engine.last_batch_route()
            engine.timing_begin("batch_firstorder")
            _batched(images, masks, sizes)
            line["batch_firstorder_kernel_ms"] = engine.timing_ms("batch_firstorder")
            engine.timing_end()
        else:
            v = n ** 3
            rois = [(images[b * v:(b + 1) * v].view(n, n, n), masks[b * v:(b + 1) * v].view(n, n, n)) for b in range(B)]
            line.update(_timed(lambda: _single_loop(rois)))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

"""Timing probe of the batched feature formulas (profiles/batch_features_measurements.md).

    python scripts/batch_features_probe.py --side batch                          # this tree's library
    PRAD_LIB=<library built from the parent commit> python scripts/batch_features_probe.py --side single

Workloads: 256 ROIs of 32^3 and 1024 ROIs of 16^3 at Ng = 32, mask fill 0.6, fixed seed.  HIP events around the region, 3
warm-up repetitions and 20 timed ones; median, minimum and maximum in ms, one JSON line per workload.
  --side batch    engine.texture_features_batch end to end (matrices, GLSZM, formulas, angle means), plus the device time of
                  the "batch_features" kernel family of its last repetition
  --side single   the loop of the single feature calls (glcm_features, glcm_mcc, zone_matrix_features x 3, ngtdm_features)
                  over the same batch's matrices, which are built once outside the timed region; runs on any library that has
                  the batched MATRIX calls, so PRAD_LIB can point at a build of the parent commit: the new code is never
                  compared against itself.  --with-matrices adds the matrix calls to the timed region (the end-to-end analogue).
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

WORKLOADS = [(256, 32), (1024, 16)]
NG, WARMUP, REPS = 32, 3, 20


def _batch(B, n, seed=1):
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    levels = torch.from_numpy(rng.integers(1, NG + 1, size=B * n ** 3).astype(np.int32)).to(dev)
    masks = torch.from_numpy((rng.random(B * n ** 3) < 0.6).view(np.uint8)).to(dev)
    return levels, masks, np.array([(n, n, n)] * B, dtype=np.intc)


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


def _single_loop(mats, zones):
    for b in range(len(zones)):
        G = mats["glcm"][b]
        engine.glcm_features(G, True)
        engine.glcm_mcc(G, True)
        R, D = mats["glrlm"][b], mats["gldm"][b]
        engine.zone_matrix_features(R, np.arange(1, R.shape[1] + 1))
        engine.zone_matrix_features(D, np.arange(1, D.shape[1] + 1))
        P, sizes = zones[b]
        if len(sizes):
            engine.zone_matrix_features(P, sizes)
        engine.ngtdm_features(mats["ngtdm"][b])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("batch", "single"), required=True)
    ap.add_argument("--with-matrices", action="store_true")
    args = ap.parse_args()
    for B, n in WORKLOADS:
        levels, masks, sizes = _batch(B, n)
        line = {"side": args.side, "B": B, "box": n, "Ng": NG, "lib": os.path.basename(_lib.LIB_PATH)}
        if args.side == "batch":
            line.update(_timed(lambda: engine.texture_features_batch(levels, masks, sizes, NG)))
            engine.timing_begin("batch_features")
            engine.texture_features_batch(levels, masks, sizes, NG)
            line["batch_features_kernel_ms"] = engine.timing_ms("batch_features")
            engine.timing_end()
            line["route"] = engine.last_batch_route()
        else:
            def matrices():
                return (engine.texture_matrices_batch(levels, masks, sizes, NG)[0],
                        engine.glszm_batch(levels, masks, sizes, NG, compact=True)[0])
            mats, zones = matrices()
            line["with_matrices"] = bool(args.with_matrices)
            line.update(_timed((lambda: _single_loop(*matrices())) if args.with_matrices else (lambda: _single_loop(mats, zones))))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

"""Times the wavelet sub-bands of many small boxes (profiles/batch_wavelet_measurements.md):
  (a) engine.wavelet_batch on the flat batch, into a preallocated output,
  (b) the loop of filters._swt3_device over the same boxes (what a lesion table paid per ROI before),
  (c) engine.roi_features_batch_images (Original + Wavelet, binCount 16) end to end,
  (d) the per-ROI filter loop of (b) writing the batch layout, then engine.roi_features_batch on the original boxes and on
      every sub-band.
Workloads: 256 boxes of 32^3 and 1024 boxes of 16^3, float32, coif1, masks ~60 % full.  (a) and (b), and (c) and (d), alternate
in ONE process; wall time around a device synchronise, warm-up first, median and spread (min .. max) of --reps repetitions.
The kernel time of (a) (prad_last_kernel_ms "batch_swt") gives the achieved bytes/s over the algorithmic bytes -- the input
element plus 64 B of sub-bands per voxel -- and their share of the 8 TB/s peak.  The counts of batch_swt_occupancy (share of
active lanes, share of warm-up planes: functions of the sizes alone, not measurements) are printed beside them.

    python scripts/batch_wavelet_probe.py --out batch_wavelet.json             # this tree: (a) .. (d), counts, kernel time
    PRAD_LIB=/path/to/parent/libpyradiomics_amd.so python scripts/batch_wavelet_probe.py --single-only --out parent.json
                                                     # (b) on a library built from the parent commit (no batched wavelet symbols)
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/batch_wavelet_probe.py --trace      # (a) alone, for kernel times
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [(256, (32, 32, 32)), (1024, (16, 16, 16))]
WAVELET = "coif1"
PEAK_BYTES_PER_S = 8.0e12
NEW_SYMBOLS = ("prad_batch_swt_plan", "prad_batch_swt_dev")


def occupancy(sizes, flen):
    """share of active lanes and of warm-up planes of the batched launch on these boxes, from the sizes alone (the planner's
    item table: engine.batch_swt_occupancy)"""
    from pyradiomics_amd import engine
    return engine.batch_swt_occupancy(sizes, flen)


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
    ap.add_argument("--single-only", action="store_true", help="(b) alone: the library has no batched wavelet entry points")
    ap.add_argument("--trace", action="store_true", help="(a) alone, a few times: for a kernel trace")
    ap.add_argument("--no-features", action="store_true", help="skip (c) and (d)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pyradiomics_amd import _lib
    if args.single_only:
        for name in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(name, None)
    import torch
    from pyradiomics_amd import engine, filters
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    lib = _lib.load()
    flen = len(filters.wavelet_filters(WAVELET)[0])
    result = {"library": _lib.LIB_PATH, "version": lib.prad_version().decode(), "wavelet": WAVELET, "workloads": []}
    for B, shape in WORKLOADS:
        rng = np.random.default_rng(B)
        n = int(np.prod(shape))
        flat = torch.from_numpy((rng.standard_normal(B * n) * 300.0 + 40.0).astype(np.float32)).cuda()
        mask = torch.from_numpy((rng.random(B * n) < 0.6).astype(np.uint8)).cuda()
        sizes = np.tile(np.array(shape, dtype=np.intc), (B, 1))
        boxes = [flat[b * n:(b + 1) * n].view(shape) for b in range(B)]
        out = torch.empty((8, B * n), dtype=torch.float64, device="cuda")
        loop_out = torch.empty((8, B * n), dtype=torch.float64, device="cuda")
        row = {"B": B, "shape": list(shape), "voxels": B * n, "algorithmic_bytes": B * n * (4 + 64)}
        names = engine.wavelet_band_names() if not args.single_only else None

        def batched():
            return engine.wavelet_batch(flat, sizes, WAVELET, out=out)

        def loop():
            keep = []
            for x in boxes:
                keep.append(filters._swt3_device(x, (2, 1, 0), wavelet=WAVELET))
            return keep

        def loop_into_batch():
            for b, x in enumerate(boxes):
                approx, ret = filters._swt3_device(x, (2, 1, 0), wavelet=WAVELET)
                for r, band in zip(range(1, 8), ret[0].values()):
                    loop_out[r, b * n:(b + 1) * n] = band.reshape(-1)
                loop_out[0, b * n:(b + 1) * n] = approx.reshape(-1)

        if args.trace:
            for _ in range(3):
                batched()
            torch.cuda.synchronize()
            continue
        if args.single_only:
            row.update({"b_loop": _wall({"b": loop}, args.reps, args.warmup)["b"]})
        else:
            row["counts"] = occupancy(sizes, flen)
            batched()
            assert engine.last_batch_route() == "batch"
            loop_into_batch()
            assert torch.equal(out, loop_out), "the batched sub-bands differ from the loop's"
            t = _wall({"a": batched, "b": loop}, args.reps, args.warmup)
            row["a_batched"], row["b_loop"] = t["a"], t["b"]
            row["loop_over_batched"] = t["b"]["median_ms"] / t["a"]["median_ms"]
            ks = []
            for _ in range(args.reps):
                batched()
                ks.append(engine.last_kernel_ms("batch_swt"))
            row["kernel_ms"] = {"median_ms": float(np.median(ks)), "min_ms": float(min(ks)), "max_ms": float(max(ks))}
            rate = row["algorithmic_bytes"] / (float(np.median(ks)) * 1e-3)
            row["bytes_per_s"], row["share_of_peak"] = rate, rate / PEAK_BYTES_PER_S
            if not args.no_features:
                def images():
                    return engine.roi_features_batch_images(flat, mask, sizes, binCount=16)

                def images_loop():
                    loop_into_batch()
                    tables = {"original": engine.roi_features_batch(flat, mask, sizes, binCount=16)[0]}
                    for name in names:
                        tables[name] = engine.roi_features_batch(loop_out[names.row(name)], mask, sizes, binCount=16)[0]
                    return tables
                t = _wall({"c": images, "d": images_loop}, max(3, args.reps // 2), 1)
                row["c_images_batched"], row["d_images_loop"] = t["c"], t["d"]
                row["images_loop_over_batched"] = t["d"]["median_ms"] / t["c"]["median_ms"]
        result["workloads"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""Times resegmentation on the device (profiles/resegment_measurements.md).  Three parts, each a run of its own:

  --part execute   execute() of a 256^3 int16 case with resegmentRange [-3, 3], sigma mode, Original only: the whole case and
                   the resegmentation step in it (imageoperations.resegmentMask wrapped in a timer around a device synchronise).
  --part labels    executeLabels on 8 labels of a 256^3 case with Wavelet and resegmentRange: the whole call.
  --part batch     engine.resegment_batch against the loop of the host resegmentMask over the same boxes, 256 boxes of 32^3 and
                   1 024 of 16^3, int16 and float64, the three modes; the kernel time of the call (prad_last_kernel_ms
                   "batch_resegment") and of the single call on a 256^3 volume ("resegment") give the achieved bytes/s over the
                   ALGORITHMIC bytes -- image and mask read once per pass, the mask written once -- against the 8 TB/s peak.
                   The probe asserts that batch and loop give equal masks before it times anything.

`execute` and `labels` use nothing this feature adds, so they also run on another checkout: --tree DIR puts DIR in front of
sys.path (the baseline is the PARENT commit in a checkout of its own, built there; run both trees one after the other on the
same machine).  Wall time around a device synchronise, warm-up first, median and spread (min .. max) of --reps repetitions.

    python scripts/resegment_probe.py --part execute --out new_execute.json
    python scripts/resegment_probe.py --part execute --tree ../parent --out parent_execute.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

PEAK_BYTES_PER_S = 8.0e12
WORKLOADS = [(256, (32, 32, 32)), (1024, (16, 16, 16))]
RANGES = {"absolute": [-200.0, 350.0], "relative": [0.2, 0.9], "sigma": [-1.5, 1.5]}


def _stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": len(v)}


def _case(labels):
    """(volume int16 256^3, label map int16): `labels` boxes of 96 x 96 x 64 voxels, each with its own label"""
    rng = np.random.default_rng(3)
    zz, yy, xx = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij", sparse=True)
    vol = (2.0 * zz + 1.5 * yy + xx + rng.normal(0.0, 120.0, (256, 256, 256))).astype(np.int16)
    lab = np.zeros(vol.shape, np.int16)
    k = 0
    for z in (16, 144):
        for y in (16, 144):
            for x in (16, 96, 176):
                if k < labels:
                    k += 1
                    lab[z:z + 96, y:y + 96, x:x + 64] = k
    return vol, lab


def part_execute(args, labels=False):
    import torch
    from pyradiomics_amd import imageoperations
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image
    vol, lab = _case(8 if labels else 1)
    setting = {"binWidth": 25, "resegmentRange": [-3, 3], "resegmentMode": "sigma"}
    types = {"Original": {}, "Wavelet": {}} if labels else {"Original": {}}
    ex = RadiomicsFeatureExtractor({"setting": setting, "imageType": types})
    step = []
    real = imageoperations.resegmentMask

    def timed(image, mask, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = real(image, mask, **kw)
        torch.cuda.synchronize()
        step.append((time.perf_counter() - t0) * 1e3)
        return out
    imageoperations.resegmentMask = timed

    def run():
        image, mask = Image(vol), Image(lab)
        image.device_tensor(), mask.device_tensor()          # (the upload is not what is measured)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = list(ex.executeLabels(image, mask)) if labels else ex.execute(image, mask, label=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res
    for _ in range(args.warmup):
        run()
    del step[:]
    whole, first = [], None
    for _ in range(args.reps):
        ms, res = run()
        whole.append(ms)
        first = first or res
    row = {"part": "labels" if labels else "execute", "whole": _stat(whole), "resegment_step": _stat(step),
           "steps_per_run": len(step) // args.reps}
    one = first[0][1] if labels else first
    row["kept_voxels"] = int(one["diagnostics_Mask-resegmented_VoxelNum"])
    row["check"] = float(one["original_firstorder_Mean"])          # (the two trees must print the same value)
    return [row]


def part_batch(args):
    import torch
    from pyradiomics_amd import engine, imageoperations
    from pyradiomics_amd.image import Image
    rows = []
    for dtype in ("int16", "float64"):
        for B, shape in WORKLOADS:
            rng = np.random.default_rng(B)
            n = int(np.prod(shape))
            host = rng.integers(-400, 600, B * n).astype(dtype)
            hmask = (rng.random(B * n) < 0.7).astype(np.uint8)
            flat, fmask = torch.from_numpy(host).cuda(), torch.from_numpy(hmask).cuda()
            sizes = np.tile(np.array(shape, dtype=np.intc), (B, 1))
            size = flat.element_size()
            for mode, rng_ in RANGES.items():
                passes = {"absolute": 2, "relative": 2, "sigma": 3}[mode]          # (the statistics pass always runs: verdicts)
                row = {"part": "batch", "dtype": dtype, "B": B, "shape": list(shape), "mode": mode,
                       "algorithmic_bytes": B * n * (passes * (size + 1) + 1)}

                def batch():
                    return engine.resegment_batch(flat, fmask, sizes, rng_, mode)

                def loop():
                    out = []
                    for b in range(B):
                        im, m = host[b * n:(b + 1) * n].reshape(shape), hmask[b * n:(b + 1) * n].reshape(shape)
                        out.append(imageoperations.resegmentMask(Image(im), Image(m), resegmentRange=rng_, resegmentMode=mode,
                                                                 label=1).array)
                    return out
                got = batch()[0].cpu().numpy()
                assert engine.last_batch_route() == "batch"
                assert np.array_equal(got, np.concatenate([m.reshape(-1) for m in loop()]).astype(np.uint8)), "masks differ"
                for _ in range(args.warmup):
                    batch()
                ms = {"batch": [], "loop": [], "kernel": []}
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    batch()
                    torch.cuda.synchronize()
                    ms["batch"].append((time.perf_counter() - t0) * 1e3)
                    ms["kernel"].append(engine.last_kernel_ms("batch_resegment"))
                for _ in range(max(1, args.reps // 3)):
                    t0 = time.perf_counter()
                    loop()
                    ms["loop"].append((time.perf_counter() - t0) * 1e3)
                row.update({k: _stat(v) for k, v in ms.items()})
                row["loop_over_batch"] = row["loop"]["median_ms"] / row["batch"]["median_ms"]
                row["bytes_per_s"] = row["algorithmic_bytes"] / (row["kernel"]["median_ms"] * 1e-3)
                row["share_of_peak"] = row["bytes_per_s"] / PEAK_BYTES_PER_S
                rows.append(row)
    # the single call on a 256^3 int16 volume
    vol, lab = _case(1)
    d_vol, d_lab = torch.from_numpy(vol).cuda(), torch.from_numpy(lab).cuda()
    for mode, rng_ in RANGES.items():
        launches = {"absolute": 1, "relative": 2, "sigma": 3}[mode]
        row = {"part": "single", "dtype": "int16", "shape": [256, 256, 256], "mode": mode,
               "algorithmic_bytes": vol.size * (launches * 4 + 2)}
        call, kernel = [], []
        for k in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engine.resegment(d_vol, d_lab, 1, rng_, mode)
            torch.cuda.synchronize()
            if k >= args.warmup:
                call.append((time.perf_counter() - t0) * 1e3)
                kernel.append(engine.last_kernel_ms("resegment"))
        row.update({"call": _stat(call), "kernel": _stat(kernel)})
        row["bytes_per_s"] = row["algorithmic_bytes"] / (row["kernel"]["median_ms"] * 1e-3)
        row["share_of_peak"] = row["bytes_per_s"] / PEAK_BYTES_PER_S
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("execute", "labels", "batch"), required=True)
    ap.add_argument("--tree", default=None, help="the checkout to import pyradiomics_amd from (default: this one)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    import torch
    from pyradiomics_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    assert os.path.abspath(_lib.LIB_PATH).startswith(tree), (_lib.LIB_PATH, tree)
    rows = {"execute": part_execute, "labels": lambda a: part_execute(a, labels=True), "batch": part_batch}[args.part](args)
    result = {"tree": tree, "library": _lib.LIB_PATH, "version": _lib.load().prad_version().decode(), "rows": rows}
    for row in rows:
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

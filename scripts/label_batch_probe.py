"""Timing probe of executeLabels(batched=True) and of the ROI gather kernel (profiles/label_batch_measurements.md).

    python scripts/label_batch_probe.py --side batched                       # this tree's library
    PRAD_LIB=<library built from the parent commit> python scripts/label_batch_probe.py --side single
    python scripts/label_batch_probe.py --side gather

Cases: one 256^3 float32 volume (a smooth field plus noise, fixed seed) with an int16 label map of 200 blobs in boxes of about
12^3, and the same volume with 1 000 blobs in boxes of about 6^3.  Settings: Original + Wavelet, six classes, binWidth 25.
One process per side; every timed call ends in a device synchronise and is preceded by a call on the case's first 8 labels
(loads every code object) and by --warmup whole calls;
median, minimum and maximum in ms over --reps repetitions, one JSON line per case.
  --side batched   list(executeLabels(image, labelmap, batched=True)), plus lastLabelsRoute() as counts
  --side single    list(executeLabels(image, labelmap)); uses only calls the parent commit has, so PRAD_LIB can point at a
                   build of it: the new code is never its own yardstick.  One repetition of the 1 000-label case is a minute
                   and a half of GPU time: give that side few repetitions (--reps 1 is allowed and is then said so in the line)
  --side gather    engine.gather_rois_batch (image and masks, one launch) against the torch loop it replaces -- per label a
                   slice, .contiguous() and == label -- with HIP events; plus the device time of the "batch_gather" kernel and
                   the bytes it moves (image element in and out, label in, mask byte out) over that time, as a share of 8 TB/s
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyradiomics_amd import _lib  # noqa: E402

# a library of an earlier commit lacks the newest entry points: drop them from the ctypes table before it is loaded
_probe = ctypes.CDLL(_lib.LIB_PATH)
for _name in [n for n in _lib.SYMBOLS if not hasattr(_probe, n)]:
    del _lib.SYMBOLS[_name]

from pyradiomics_amd import engine, imageoperations  # noqa: E402
from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor  # noqa: E402

CASES = [(200, 12), (1000, 6)]          # (labels, box edge)
N = 256
PARAMS = {"imageType": {"Original": {}, "Wavelet": {}}, "setting": {"binWidth": 25}}


def _volume(seed=3):
    rng = np.random.default_rng(seed)
    z, y, x = np.mgrid[0:N, 0:N, 0:N].astype(np.float32)
    img = 300.0 + 120.0 * np.sin(z / 23.0) + 90.0 * np.cos(y / 17.0) + 60.0 * np.sin((x + y) / 29.0)
    return (img + rng.standard_normal((N, N, N), dtype=np.float32) * 40.0).astype(np.float32)


def _labelmap(count, edge, seed=5):
    """`count` ellipsoids, one per cell of a regular grid, jittered inside their cells; semi-axes edge/2 - 1 .. edge/2"""
    rng = np.random.default_rng(seed)
    per = int(np.ceil(count ** (1.0 / 3.0)))
    cell = N // per
    assert cell >= edge + 2
    lab = np.zeros((N, N, N), dtype=np.int16)
    g = np.mgrid[0:edge, 0:edge, 0:edge].astype(np.float64) - (edge - 1) / 2.0
    cells = rng.permutation(per ** 3)[:count]
    for k, c in enumerate(cells):
        cz, cy, cx = c // (per * per), (c // per) % per, c % per
        o = [int(i * cell + rng.integers(0, cell - edge + 1)) for i in (cz, cy, cx)]
        r = edge / 2.0 - rng.random(3)
        blob = (g[0] / r[0]) ** 2 + (g[1] / r[1]) ** 2 + (g[2] / r[2]) ** 2 <= 1.0
        lab[o[0]:o[0] + edge, o[1]:o[1] + edge, o[2]:o[2] + edge][blob] = k + 1
    return lab


def _summary(times, reps):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "reps": reps}


def _wall(fn, warmup, reps):
    times = []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return _summary(times, reps)


def _events(fn, warmup, reps):
    times = []
    for rep in range(warmup + reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if rep >= warmup:
            times.append(t0.elapsed_time(t1))
    return _summary(times, reps)


def _torch_loop(image, labelmap, labels, lo, hi):
    out = []
    for l, a, b in zip(labels, lo, hi):
        sl = tuple(slice(int(x), int(y) + 1) for x, y in zip(a, b))
        out.append((image[sl].contiguous(), labelmap[sl].contiguous() == l))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=("batched", "single", "gather"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", type=int, nargs="*", default=None, help="label counts to run (default: 200 and 1000)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_batch_probe: no GPU -- a timing taken anywhere else says nothing")
    img = _volume()
    for count, edge in CASES:
        if args.cases and count not in args.cases:
            continue
        lab = _labelmap(count, edge)
        line = {"side": args.side, "labels": count, "box": edge, "lib": os.path.basename(_lib.LIB_PATH), "warmup": args.warmup}
        if args.side == "gather":
            present, _, lo, hi = imageoperations._censusHost(lab)
            lo, hi = imageoperations.alignedBox(lo, hi, lab.shape)
            d_img, d_lab = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
            line["kernel"] = _events(lambda: engine.gather_rois_batch(d_img, d_lab, present, lo, hi), 3, max(args.reps, 20))
            line["torch_loop"] = _events(lambda: _torch_loop(d_img, d_lab, present, lo, hi), 3, max(args.reps, 20))
            engine.timing_begin("batch_gather")
            engine.gather_rois_batch(d_img, d_lab, present, lo, hi)
            torch.cuda.synchronize()
            ms = engine.timing_ms("batch_gather")
            engine.timing_end()
            vox = int((hi - lo + 1).prod(1).sum())
            line.update(voxels=vox, batch_gather_kernel_ms=ms, bytes=vox * (4 + 4 + 2 + 1),
                        share_of_8TBs=(vox * 11 / (ms * 1e-3) / 8e12) if ms > 0 else None)
        else:
            ex = RadiomicsFeatureExtractor(PARAMS)
            kw = {"batched": True} if args.side == "batched" else {}
            got = []
            list(ex.executeLabels(img, lab, labels=list(range(1, 9)), **kw))      # loads every code object before the first timed call
            line.update(_wall(lambda: got.append(len(list(ex.executeLabels(img, lab, **kw)))), args.warmup, args.reps))
            line["results"] = got[-1]
            if args.side == "batched":
                line["route"] = {k: len(v) for k, v in ex.lastLabelsRoute().items()}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

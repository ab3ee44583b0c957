"""Times the texture features of many small ROIs with force2D, and with force2D + weightingNorm
(profiles/batch_planar_measurements.md):
  (a) engine.texture_features_batch(force2D=True, force2Ddimension=0[, weightingNorm="euclidean", spacing=...]) end to end,
  (b) the loop of the single device calls over the same ROIs with the same settings: glcm, glcm_glrlm, gldm, ngtdm and
      glszm_compact with the forced dimension, then glcm_features, glcm_mcc, zone_matrix_features (three times) and
      ngtdm_features; with weightingNorm the GLCM and GLRLM are first merged with torch on the device, (P * w).sum(2).
Workloads: 256 ROIs of 16 x 32 x 32 and 1024 ROIs of 8 x 16 x 16 (thick slices: the forced dimension is z), 32 levels, masks
~60 % full.  HIP events around each repetition, warm-up first, median and spread (min .. max) of --reps repetitions.
Kernel times (prad_last_kernel_ms) of the merge launch ("batch_merge") and of the GLSZM labelling launch ("batch_glszm") for the
unforced kernel and the three forced variants are recorded beside them.

    python scripts/batch_planar_probe.py --out batch_planar.json                     # this tree: (a), (b) and the kernel times
    PRAD_LIB=/path/to/parent/libpyradiomics_amd.so python scripts/batch_planar_probe.py --single-only --out parent.json
                                                     # (b) on a library built from the parent commit (no forced batch symbols)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [(256, (16, 32, 32)), (1024, (8, 16, 16))]
NG = 32
SPACING = (2.5, 0.7, 1.3)
NEW_SYMBOLS = ("prad_batch_plan_f2d", "prad_calculate_batch_f2d_dev", "prad_batch_glszm_f2d_dev", "prad_batch_merge_plan",
               "prad_batch_merge_angles_dev")


def _events(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": reps}


def _stat(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--single-only", action="store_true", help="skip (a): the library has no forced batch entry points")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pyradiomics_amd import _lib
    if args.single_only:
        for name in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(name, None)
    import logging
    import torch
    from pyradiomics_amd import engine
    from pyradiomics_amd.glcm import _weights
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    lib = _lib.load()
    log = logging.getLogger("probe")
    result = {"library": _lib.LIB_PATH, "version": lib.prad_version().decode(), "Ng": NG, "workloads": []}
    for B, shape in WORKLOADS:
        rng = np.random.default_rng(B)
        n = int(np.prod(shape))
        levels = torch.from_numpy(rng.integers(1, NG + 1, size=B * n).astype(np.int32)).cuda()
        mask = torch.from_numpy((rng.random(B * n) < 0.6).astype(np.uint8)).cuda()
        sizes = np.tile(np.array(shape, dtype=np.intc), (B, 1))
        rois = [(levels[b * n:(b + 1) * n].view(shape), mask[b * n:(b + 1) * n].view(shape)) for b in range(B)]
        Ns = [max(1, int(c)) for c in mask.view(B, n).sum(1).tolist()]
        ang = engine.pair_angles(shape, (1,), True, 0)
        wg = torch.from_numpy(_weights(ang, np.array(SPACING), "euclidean", "glcm", log)).cuda()
        wr = torch.from_numpy(_weights(ang, np.array(SPACING), "euclidean", "glrlm", log)).cuda()
        row = {"B": B, "shape": list(shape)}

        def loop(weighted):
            keep = []
            for (img, msk), ns in zip(rois, Ns):
                g, r, _ = engine.glcm_glrlm(img, msk, NG, max(shape), True, 0)
                d, t = engine.gldm(img, msk, NG, 0, (1,), True, 0), engine.ngtdm(img, msk, NG, (1,), True, 0)
                z, zs = engine.glszm_compact(img, msk, NG, ns, True, 0)
                sym = True
                if weighted:
                    g = ((g + g.transpose(0, 1)) * wg).sum(2, keepdim=True)
                    r = (r * wr).sum(2, keepdim=True)
                    sym = False
                keep.append((engine.glcm_features(g, sym), engine.glcm_mcc(g, sym),
                             engine.zone_matrix_features(r, np.arange(1, r.shape[1] + 1)),
                             engine.zone_matrix_features(d, np.arange(1, d.shape[1] + 1)), engine.ngtdm_features(t),
                             engine.zone_matrix_features(z, zs) if z.shape[1] else None))
            return keep

        for weighted, tag in ((False, "force2D"), (True, "force2D_weighted")):
            kw = dict(force2D=True, force2Ddimension=0)
            if weighted:
                kw.update(weightingNorm="euclidean", spacing=SPACING)
            if not args.single_only:
                def batched():
                    return engine.texture_features_batch(levels, mask, sizes, NG, **kw)
                table, status = batched()
                assert engine.last_batch_route() == "batch" and status == [1] * B
                row["a_batched_" + tag] = _events(batched, args.reps, args.warmup)
                ref = loop(weighted)          # the same numbers as the loop gives, first and last ROI
                for b in (0, B - 1):
                    if not weighted:
                        vals, empty = ref[b][0]
                        assert np.array_equal(table["glcm"][b][:23], vals[~empty].mean(0))
                    assert np.array_equal(table["ngtdm"][b], ref[b][4].reshape(-1))
            row["b_loop_" + tag] = _events(lambda: loop(weighted), max(3, args.reps // 3), 1)
        if not args.single_only:
            merge, lab = [], {d: [] for d in (-1, 0, 1, 2)}
            for _ in range(args.reps):
                engine.texture_matrices_batch_flat(levels, mask, sizes, NG, ("glcm", "glrlm"), (1,), 0, True, 0, "euclidean", SPACING)
                merge.append(engine.last_kernel_ms("batch_merge"))
                for d in lab:
                    engine.glszm_batch_zones(levels, mask, sizes, NG, force2D=d >= 0, force2Ddimension=max(d, 0))
                    lab[d].append(engine.last_kernel_ms("batch_glszm"))
            row["merge_kernel"] = _stat(merge)
            for d, ms in lab.items():
                row["glszm_label_kernel_f2d%s" % ("_none" if d < 0 else d)] = _stat(ms)
        result["workloads"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

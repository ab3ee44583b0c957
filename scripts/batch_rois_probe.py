"""Times the texture matrices of many small ROIs (profiles/batch_rois_measurements.md):
  (a) one batched call (engine.texture_matrices_batch_flat: prad_calculate_batch_dev),
  (b) the loop of the single device calls over the same ROIs, synchronous,
  (c) the same loop in deferred mode (enqueue only, one deferred_status at the end).
Workloads: 256 ROIs of 32^3 and 1024 ROIs of 16^3, 32 levels, masks ~60 % full, GLCM + GLRLM + GLDM + NGTDM.  HIP events
around each repetition, warm-up first, median and spread (min .. max) of --reps repetitions.

--glszm times the GLSZM of the same workloads instead, on random levels ("noise": small zones) and on levels from a blurred
field quantised to 32 ("smooth": zone sizes drive the labelling kernel):
  (a) engine.glszm_batch(compact=True) end to end, plus the "batch_glszm" kernel times of the labelling and the fill launch,
  (b) the loop of engine.glszm_compact over the same ROIs (Ns counted beforehand),
  (c) the loop of engine.glszm_features(deferred=True), one deferred_status at the end.

    python scripts/batch_rois_probe.py [--glszm] --out batch_probe.json             # this tree: (a), (b), (c)
    PRAD_LIB=/path/to/parent/libpyradiomics_amd.so python scripts/batch_rois_probe.py [--glszm] --single-only ...
                                                     # (b), (c) on a library built from another commit (no batch symbols)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = [(256, 32), (1024, 16)]
NG = 32


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


def _smooth_levels(rng, B, edge):
    """levels of a blurred random field (Gaussian, sigma 1.5 voxels, per ROI), quantised to NG equally filled bins"""
    from scipy import ndimage
    out = np.empty((B, edge, edge, edge), dtype=np.int32)
    for b in range(B):
        f = ndimage.gaussian_filter(rng.standard_normal((edge, edge, edge)), 1.5)
        edges = np.quantile(f, np.linspace(0, 1, NG + 1)[1:-1])
        out[b] = 1 + np.searchsorted(edges, f)
    return out.reshape(-1)


def glszm_mode(args, engine, result):
    import torch
    for B, edge in WORKLOADS:
        for kind in ("noise", "smooth"):
            rng = np.random.default_rng(B + (kind == "smooth"))
            n = edge ** 3
            lv = rng.integers(1, NG + 1, size=B * n).astype(np.int32) if kind == "noise" else _smooth_levels(rng, B, edge)
            mk = (rng.random(B * n) < 0.6).astype(np.uint8)
            levels, mask = torch.from_numpy(lv).cuda(), torch.from_numpy(mk).cuda()
            sizes = np.full((B, 3), edge, dtype=np.intc)
            rois = [(levels[b * n:(b + 1) * n].view(edge, edge, edge), mask[b * n:(b + 1) * n].view(edge, edge, edge)) for b in range(B)]
            Ns = [max(1, int(c)) for c in mk.reshape(B, n).sum(1)]
            row = {"family": "glszm", "levels": kind, "B": B, "edge": edge}
            if not args.single_only:
                def batched():
                    return engine.glszm_batch(levels, mask, sizes, NG, compact=True)
                res, status = batched()
                assert engine.last_batch_route() == "batch" and status == [1] * B
                _, summary, _ = engine.glszm_batch_zones(levels, mask, sizes, NG)
                row["zones_per_roi_mean"] = float(summary[:, 0].mean())
                row["largest_zone_max"] = int(summary[:, 1].max())
                row["a_batched"] = _events(batched, args.reps, args.warmup)
                lab, fill = [], []
                for _ in range(args.reps):
                    engine.glszm_batch_zones(levels, mask, sizes, NG)
                    lab.append(engine.last_kernel_ms("batch_glszm"))
                    batched()
                    fill.append(engine.last_kernel_ms("batch_glszm"))
                for name, ms in (("label_kernel", lab), ("fill_kernel", fill)):
                    row[name] = {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}
                for b in (0, B - 1):          # the same numbers as the loop gives
                    P, sz = engine.glszm_compact(*rois[b], NG, Ns[b])
                    assert torch.equal(res[b][0], P) and np.array_equal(res[b][1], sz)

            def loop_compact():
                return [engine.glszm_compact(img, msk, NG, ns) for (img, msk), ns in zip(rois, Ns)]

            def loop_features():
                keep = [engine.glszm_features(img, msk, NG, ns, deferred=True) for (img, msk), ns in zip(rois, Ns)]
                engine.deferred_status()
                return keep
            row["b_loop_compact"] = _events(loop_compact, args.reps, args.warmup)
            try:
                row["c_loop_features_deferred"] = _events(loop_features, args.reps, args.warmup)
            except NotImplementedError as e:
                row["c_loop_features_deferred"] = {"error": str(e)}
            result["workloads"].append(row)
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--single-only", action="store_true", help="skip (a): the library has no batch entry points")
    ap.add_argument("--glszm", action="store_true", help="time the GLSZM of the workloads instead of the four other families")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pyradiomics_amd import _lib
    if args.single_only:
        for name in [n for n in _lib.SYMBOLS if n.startswith("prad_batch") or n == "prad_calculate_batch_dev"]:
            del _lib.SYMBOLS[name]
    import torch
    from pyradiomics_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing is measured without one")
    lib = _lib.load()
    result = {"library": _lib.LIB_PATH, "version": lib.prad_version().decode(), "Ng": NG, "workloads": []}
    for B, edge in ([] if args.glszm else WORKLOADS):
        rng = np.random.default_rng(B)
        n = edge ** 3
        levels = torch.from_numpy(rng.integers(1, NG + 1, size=B * n).astype(np.int32)).cuda()
        mask = torch.from_numpy((rng.random(B * n) < 0.6).astype(np.uint8)).cuda()
        sizes = np.full((B, 3), edge, dtype=np.intc)
        rois = [(levels[b * n:(b + 1) * n].view(edge, edge, edge), mask[b * n:(b + 1) * n].view(edge, edge, edge)) for b in range(B)]
        row = {"B": B, "edge": edge}

        def loop(deferred):
            keep = []
            for img, msk in rois:
                keep.append(engine.glcm_glrlm(img, msk, NG, edge, deferred=deferred))
                keep.append(engine.gldm(img, msk, NG, deferred=deferred))
                keep.append(engine.ngtdm(img, msk, NG, deferred=deferred))
            if deferred:
                engine.deferred_status()
            return keep

        if not args.single_only:
            def batched():
                return engine.texture_matrices_batch_flat(levels, mask, sizes, NG)
            flat, status = batched()
            assert engine.last_batch_route() == "batch" and status == [1] * B
            row["a_batched"] = _events(batched, args.reps, args.warmup)
            batched()
            kern = engine.last_kernel_ms("batch")
            kms = []
            for _ in range(args.reps):
                batched()
                kms.append(engine.last_kernel_ms("batch"))
            out_bytes = sum(int(t.numel()) * 8 for t in flat.values())
            in_bytes = B * n * 5
            row["batch_kernel"] = {"median_ms": float(np.median(kms)), "min_ms": float(min(kms)), "max_ms": float(max(kms)),
                                   "first_ms": float(kern), "bytes_in": in_bytes, "bytes_out": out_bytes,
                                   "fraction_of_8TBs": (in_bytes + out_bytes) / (float(np.median(kms)) * 1e-3) / 8e12}
            # the same numbers as the loop gives (GLCM + GLRLM of the fused sweep, GLDM, NGTDM) on the first and last ROI
            o = 0
            for b in (0, B - 1):
                g, r, _ = engine.glcm_glrlm(*rois[b], NG, edge)
                per = NG * NG * 13
                assert torch.equal(flat["glcm"][b * per:(b + 1) * per].view(NG, NG, 13), g)
                per = NG * edge * 13
                assert torch.equal(flat["glrlm"][b * per:(b + 1) * per].view(NG, edge, 13), r)
                per = NG * 53
                assert torch.equal(flat["gldm"][b * per:(b + 1) * per].view(NG, 53), engine.gldm(*rois[b], NG))
        row["b_loop_sync"] = _events(lambda: loop(False), args.reps, args.warmup)
        row["c_loop_deferred"] = _events(lambda: loop(True), args.reps, args.warmup)
        result["workloads"].append(row)
        print(json.dumps(row), flush=True)
    if args.glszm:
        glszm_mode(args, engine, result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""bench.py's plain run: one JSON line with the headline keys only, and --dump-outputs writes the matrices of the last timed
step -- the same for two runs with the same arguments, and equal to a synchronous call on the bench volume."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "256",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_dumped_outputs(tmp_path):
    import torch
    import bench
    from pyradiomics_amd import engine
    rec = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "Mvoxels/s" and rec["higher_is_better"] is True
    assert not {"roofline", "modes", "cold_ms_per_step", "cpu_baseline", "host_boundary"} & set(rec)   # --full only
    n, Ng = 256, 32
    g = np.load(tmp_path / "a" / "glcm.npy")
    r = np.load(tmp_path / "a" / "glrlm.npy")
    assert g.dtype == np.float64 and g.shape == (Ng, Ng, 13) and r.dtype == np.float64 and r.shape == (Ng, n, 13)
    dev = torch.device("cuda", 0)
    img, msk = bench.make_volume(n, Ng, "uniform", seed=0, device=dev)
    gs, rs, _ = engine.glcm_glrlm(img, msk, Ng, n)
    assert np.array_equal(g, gs.cpu().numpy()) and np.array_equal(r, rs.cpu().numpy())
    _plain_run(tmp_path / "b")                                      # the same arguments: the same inputs, the same outputs
    for name in ("glcm", "glrlm"):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))), name

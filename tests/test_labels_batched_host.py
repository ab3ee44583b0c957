"""executeLabels(batched=True) away from the device: on the CPU oracle backend nothing can be batched and the mode must be the
default one, result for result; the command line's --batch-labels; and the box arithmetic that turns census bounds into the
boxes the gather kernel cuts (imageoperations.alignedBox) against the box cropToTumorMask itself cuts."""
import numpy as np
import pytest


def _case():
    rng = np.random.default_rng(11)
    z, y, x = np.mgrid[0:12, 0:12, 0:12]
    img = (40.0 * np.sin(z / 3.0) + 25.0 * np.cos(y / 2.5) + 3.0 * x + rng.normal(0, 6, (12, 12, 12))).astype(np.float32)
    lab = np.zeros((12, 12, 12), dtype=np.int16)
    lab[1:6, 1:7, 0:5] = 1
    lab[6:11, 2:9, 5:12] = 2
    lab[2:5, 8:11, 7:10] = 4
    return img, lab


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    return a == b


def test_batched_mode_on_host_backend_is_the_default_mode(oracle_port):
    from pyradiomics_amd import backend
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    old = backend._cmatrices
    backend.set(oracle_port)
    try:
        img, lab = _case()
        ex = RadiomicsFeatureExtractor(binWidth=10)
        assert ex.lastLabelsRoute() == {"batched": [], "single": [], "mixed": []}
        want = list(ex.executeLabels(img, lab))
        assert ex.lastLabelsRoute() == {"batched": [], "single": [1, 2, 4], "mixed": []}
        got = list(ex.executeLabels(img, lab, batched=True))
        assert ex.lastLabelsRoute() == {"batched": [], "single": [1, 2, 4], "mixed": []}
        assert [l for l, _ in got] == [l for l, _ in want] == [1, 2, 4]
        for (_, g), (_, w) in zip(got, want):
            assert list(g) == list(w)
            assert any(k.startswith("original_glszm_") for k in g)
            for k in w:
                assert _same(g[k], w[k]), k
        # an absent label of an explicit list still fails at its position, after the results before it
        seen = []
        with pytest.raises(ValueError, match="not present"):
            for l, _ in ex.executeLabels(img, lab, labels=[2, 3, 1], batched=True):
                seen.append(l)
        assert seen == [2]
        assert ex.lastLabelsRoute()["single"] == [1, 2, 4]      # (the failed call did not finish: the record is the last finished one's)
    finally:
        backend.set(old)


def test_batch_labels_option(monkeypatch, tmp_path):
    from pyradiomics_amd import scripts
    args = scripts.get_parser().parse_args(["img.nrrd", "msk.nrrd", "--batch-labels"])
    assert args.batch_labels and args.mode == "segment"
    assert not scripts.get_parser().parse_args(["img.nrrd", "msk.nrrd", "--all-labels"]).batch_labels
    calls = []

    def fake(cases, param, overrides, mode, jobs, gpus, out_dir, unix_path, level, all_labels=False, batch_labels=False):
        calls.append((mode, all_labels, batch_labels))
        return [{"Image": "img.nrrd", "Mask": "msk.nrrd"}]
    monkeypatch.setattr(scripts, "process_cases", fake)
    out = str(tmp_path / "out.txt")
    assert scripts.main(["img.nrrd", "msk.nrrd", "--batch-labels", "-o", out]) == 0
    assert calls == [("segment", True, True)]                      # implies --all-labels
    assert scripts.main(["img.nrrd", "msk.nrrd", "--all-labels", "-o", out]) == 0
    assert calls[-1] == ("segment", True, False)                   # without the flag nothing changes
    assert scripts.main(["img.nrrd", "msk.nrrd", "--batch-labels", "--mode", "voxel", "-o", out]) != 0
    assert len(calls) == 2                                         # refused in voxel mode: nothing was extracted

    # the worker hands `batched=True` to executeLabels, and only then
    class Ex:
        def __init__(self):
            self.kw = []

        def executeLabels(self, image, mask, **kw):
            self.kw.append(kw)
            return iter([(3, {"f": 1.0})])
    ex = Ex()
    monkeypatch.setitem(scripts._WORKER, "extractor", ex)
    case = {"Image": "img.nrrd", "Mask": "msk.nrrd"}
    rows = scripts._run_case((1, case, "segment", None, False, True, True))[1]
    assert rows[0]["Label"] == 3 and ex.kw[-1].get("batched") is True
    scripts._run_case((1, case, "segment", None, False, True))
    assert "batched" not in ex.kw[-1]


@pytest.mark.parametrize("nx", [9, 16, 23])
def test_aligned_box_is_the_box_the_crop_cuts(nx):
    """x extents 1 to 9 at every x position of rows of 9, 16 and 23 voxels -- boxes at the left edge, at the right edge (the
    extension is clipped there and the box grows to the left instead) and at both (it stays short)"""
    import torch
    from pyradiomics_amd import imageoperations
    from pyradiomics_amd.image import Image
    shape = (3, 4, nx)
    los, his = [], []
    for ext in range(1, 10):
        for x0 in range(0, nx - ext + 1):
            los.append((1, 1, x0))
            his.append((2, 3, x0 + ext - 1))
    got_lo, got_hi = imageoperations.alignedBox(np.array(los), np.array(his), shape)
    assert got_lo.shape == (len(los), 3)
    for i, (lo, hi) in enumerate(zip(los, his)):
        # cropToTumorMask's device route on host tensors: the box it cuts shows in the crop's shape and origin
        msk = Image(None, tensor=torch.zeros(shape, dtype=torch.int16))
        img = Image(None, tensor=torch.zeros(shape, dtype=torch.float32))
        msk._derived[("bbox", 1)] = (np.array(lo), np.array(hi))
        cimg, cmsk = imageoperations.cropToTumorMask(img, msk, 1, padDistance=0, deviceResident=True, alignRows=True)
        want_lo = np.array([int(round(v)) for v in cimg.origin[::-1]])
        want_hi = want_lo + np.array(cimg.shape) - 1
        assert cimg.shape == cmsk.shape
        assert np.array_equal(got_lo[i], want_lo) and np.array_equal(got_hi[i], want_hi), (lo, hi)
        one_lo, one_hi = imageoperations.alignedBox(np.array(lo), np.array(hi), shape)      # (the [Nd] form)
        assert np.array_equal(one_lo, want_lo) and np.array_equal(one_hi, want_hi)
        ext = want_hi[2] - want_lo[2] + 1
        assert want_lo[2] <= lo[2] and want_hi[2] >= hi[2] and (ext % 4 == 0 or (want_lo[2] == 0 and want_hi[2] == nx - 1))
        assert np.array_equal(want_lo[:2], lo[:2]) and np.array_equal(want_hi[:2], hi[:2])
        need = (-(hi[2] - lo[2] + 1)) % 4                          # restated: to the right first, the rest to the left
        assert want_hi[2] - hi[2] == min(need, nx - 1 - hi[2])
        assert lo[2] - want_lo[2] == min(need - (want_hi[2] - hi[2]), lo[2])
    # the inputs are not written to
    assert np.array_equal(np.array(los)[:, 2], [l[2] for l in los])

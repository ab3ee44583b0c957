"""Multi-label extraction, host tier: imageoperations.labelCensus on numpy label maps against a brute-force census, the
bounding-box memo it leaves for cropToTumorMask, RadiomicsFeatureExtractor.executeLabels on the host route (CPU oracle
backend, Original image type) against per-label execute(), and the --all-labels flag of the command line."""
import csv
import logging

import numpy as np
import pytest

from labels_cases import A, ABSENT, B, C_, D, assert_census, brute_census, census_cases, labels_case

CASES = census_cases()


@pytest.mark.parametrize("name,arr,dtypes", CASES, ids=[c[0] for c in CASES])
def test_host_census_equals_brute_force(name, arr, dtypes):
    from pyradiomics_amd import imageoperations as io
    from pyradiomics_amd.image import Image
    want = brute_census(arr)
    for dt in dtypes + (np.int64,):
        mask = Image(arr.astype(dt))
        got = io.labelCensus(mask, deviceResident=False)
        assert_census(got, want, "%s %s" % (name, np.dtype(dt)))
        assert all(np.asarray(g).dtype == np.int64 for g in got)
        assert io.labelCensus(mask, deviceResident=False)[0] is got[0]            # memoised on the Image
        for l in want[0]:
            lo, hi = mask._derived[("bbox", int(l))]
            blo, bhi = io.boundingBox(arr == l)
            assert np.array_equal(lo, blo) and np.array_equal(hi, bhi)
            n, clo, chi = io.censusLookup(mask, int(l))
            assert n == int((arr == l).sum()) and np.array_equal(clo, blo) and np.array_equal(chi, bhi)
        assert io.censusLookup(mask, 77777) == (0, None, None)
        assert io.censusLookup(mask, 0) is None and io.censusLookup(mask, -3) is None
        assert io.censusLookup(Image(arr.astype(dt)), 1) is None                  # no census taken: callers scan as before


def test_host_census_ignores_negative_values_and_takes_large_labels():
    from pyradiomics_amd import imageoperations as io
    from pyradiomics_amd.image import Image
    arr = np.zeros((3, 4, 6), np.int32)
    arr[0, 0, 0:3] = -1
    arr[1, 1:3, 2:5] = 7
    arr[2, 3, 5] = 70000                     # beyond the device census' 65535: still counted on the host
    got = io.labelCensus(Image(arr), deviceResident=False)
    assert_census(got, brute_census(arr))
    assert list(got[0]) == [7, 70000]
    with pytest.raises(ValueError):
        io.labelCensus(Image(np.full((2, 2, 2), 0.5)), deviceResident=False)


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, (float, np.floating, np.ndarray)):
            x, y = float(x), float(y)
            assert x == y or (np.isnan(x) and np.isnan(y)), k
        else:
            assert x == y, k


def test_execute_labels_equals_execute_on_host_route(oracle_port, caplog):
    from pyradiomics_amd import backend
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image
    vol, lab = labels_case()
    old = backend._cmatrices
    backend.set(oracle_port)
    try:
        ex = RadiomicsFeatureExtractor(binWidth=25)
        want = {l: ex.execute(Image(vol), Image(lab), label=l) for l in (A, B, C_)}
        with caplog.at_level(logging.WARNING, logger="pyradiomics_amd.featureextractor"):
            got = list(ex.executeLabels(Image(vol), Image(lab)))
        assert [l for l, _ in got] == [A, B, C_]
        assert any("label %d skipped" % D in r.getMessage() for r in caplog.records)
        for l, res in got:
            assert len(res) > 100
            _same(res, want[l])
        assert [l for l, _ in ex.executeLabels(Image(vol), Image(lab), labels=[B, A])] == [B, A]
        # an explicit label that fails: the labels before it arrive, then execute()'s own error
        with pytest.raises(ValueError) as single:
            ex.execute(Image(vol), Image(lab), label=D)
        seen = []
        with pytest.raises(ValueError) as multi:
            for l, res in ex.executeLabels(Image(vol), Image(lab), labels=[A, D]):
                seen.append(l)
        assert seen == [A] and str(multi.value) == str(single.value)
        with pytest.raises(ValueError, match=r"Label \(9\) not present in mask"):
            list(ex.executeLabels(Image(vol), Image(lab), labels=[ABSENT]))
        # settings that make the image depend on the label: the per-label fallback, same results
        for extra in ({"preCrop": True}, {"resegmentRange": [-3, 3], "resegmentMode": "sigma"}, {"normalize": True}):
            ex2 = RadiomicsFeatureExtractor(binWidth=25, **extra)
            for l, res in ex2.executeLabels(Image(vol), Image(lab), labels=[A, B]):
                _same(res, ex2.execute(Image(vol), Image(lab), label=l))
    finally:
        backend.set(old)


def test_execute_labels_discovers_the_labels_of_a_vector_mask_without_label_1(oracle_port):
    """labels=None asks no label of the mask while loading: a channel of a vector mask that holds only labels 2 and 3 is
    extracted label by label (execute() needs its label named), and an explicit list keeps checking its first label"""
    from pyradiomics_amd import backend
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image
    vol, lab = labels_case()
    lab = np.where((lab == B) | (lab == C_), lab, 0).astype(np.int16)
    vec = np.stack([np.zeros_like(lab), lab], axis=-1)           # (z, y, x, c): channel 1 carries the labels
    old = backend._cmatrices
    backend.set(oracle_port)
    try:
        ex = RadiomicsFeatureExtractor(binWidth=25)
        got = list(ex.executeLabels(Image(vol), vec, label_channel=1))
        assert [l for l, _ in got] == [B, C_]
        for l, res in got:
            _same(res, ex.execute(Image(vol), vec, label=l, label_channel=1))
        with pytest.raises(ValueError, match="not present in mask"):
            list(ex.executeLabels(Image(vol), vec, labels=[A], label_channel=1))
        with pytest.raises(ValueError, match="nothing is segmented"):
            list(ex.executeLabels(Image(vol), vec, label_channel=0))
    finally:
        backend.set(old)


def test_cli_all_labels_on_host_route(tmp_path, oracle_port):
    from pyradiomics_amd import backend, scripts
    from pyradiomics_amd.featureextractor import RadiomicsFeatureExtractor
    from pyradiomics_amd.image import Image, write_nrrd
    assert scripts.get_parser().parse_args(["i.nrrd", "m.nrrd", "--all-labels"]).all_labels
    assert not scripts.get_parser().parse_args(["i.nrrd", "m.nrrd"]).all_labels
    vol, lab = labels_case()
    ip, mp = str(tmp_path / "img.nrrd"), str(tmp_path / "lab.nrrd")
    write_nrrd(ip, Image(vol, (1.0, 1.0, 2.0)))
    write_nrrd(mp, Image(lab, (1.0, 1.0, 2.0)))
    old = backend._cmatrices
    backend.set(oracle_port)
    try:
        out = tmp_path / "out.csv"
        assert scripts.main([ip, mp, "-s", "binWidth:25", "--all-labels", "-f", "csv", "-o", str(out)]) == 0
        rows = list(csv.DictReader(open(out)))
        assert [r["Label"] for r in rows] == [str(A), str(B), str(C_)]
        ex = RadiomicsFeatureExtractor(binWidth=25.0)
        for r in rows:
            want = ex.execute(ip, mp, label=int(r["Label"]))
            feats = [k for k in want if not k.startswith("diagnostics_")]
            assert len(feats) > 90
            for k in feats:
                x, y = float(r[k]), float(want[k])
                assert x == y or (np.isnan(x) and np.isnan(y)), k
        # a batch file: one row per label and case, the case's own columns repeated
        batch = tmp_path / "cases.csv"
        with open(batch, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["ID", "Image", "Mask", "Label"])
            w.writerow(["p1", ip, mp, "2"])
            w.writerow(["p2", ip, mp, "2"])
        out2 = tmp_path / "out2.csv"
        assert scripts.main([str(batch), "-s", "binWidth:25", "--all-labels", "-f", "csv", "-o", str(out2)]) == 0
        rows2 = list(csv.DictReader(open(out2)))
        assert [(r["ID"], r["Label"]) for r in rows2] == [(p, str(l)) for p in ("p1", "p2") for l in (A, B, C_)]
        assert rows2[4]["original_glcm_Contrast"] == rows[1]["original_glcm_Contrast"]
        # without the flag nothing changes: the Label column selects one label per row
        out3 = tmp_path / "out3.csv"
        assert scripts.main([str(batch), "-s", "binWidth:25", "-f", "csv", "-o", str(out3)]) == 0
        rows3 = list(csv.DictReader(open(out3)))
        assert [(r["ID"], r["Label"]) for r in rows3] == [("p1", "2"), ("p2", "2")]
        assert rows3[0]["original_glcm_Contrast"] == rows[1]["original_glcm_Contrast"]
    finally:
        backend.set(old)

"""shared test helpers (CPU side)"""
import atexit
import builtins
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# what the reference's own compiled code answered to every call the tests make of it (tests/golden/make_reference_calls.py)
REFERENCE_CALLS = {"cmatrices": os.path.join(GOLDEN, "reference_cmatrices_calls.npz"),    # oracle/_ref/libcmatrices_ref.so
                   "module": os.path.join(GOLDEN, "reference_module_calls.npz")}         # oracle/_ref/_cmatrices.so
RECORD_ENV = "PRAD_RECORD_REFERENCE"


def _call_key(name, args, kwargs):
    """digest of one call: the function name and every argument, arrays by dtype, shape, strides and contents"""
    h = hashlib.sha256(name.encode())

    def feed(x):
        if isinstance(x, np.ndarray):
            h.update(("A%s%r%r;" % (x.dtype.str, x.shape, x.strides)).encode())
            h.update(np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (list, tuple)):
            h.update(("L%d;" % len(x)).encode())
            for y in x:
                feed(y)
        elif isinstance(x, dict):
            h.update(("D%d;" % len(x)).encode())
            for k in sorted(x):
                feed(k)
                feed(x[k])
        else:
            h.update(("%s:%r;" % (type(x).__name__, x)).encode())
    feed(args)
    feed(kwargs)
    return h.hexdigest()[:32]


class RecordedReference:
    """Stands in for one of the reference's compiled CPU oracles: answers each call with what the reference returned
    (or the exception type it raised) for exactly those arguments when the call was recorded."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError(path + " (record it with tests/golden/make_reference_calls.py)")
        with np.load(path, allow_pickle=False) as z:
            self._arrays = {k: z[k] for k in z.files if k != "__index__"}
            self._index = json.loads(str(z["__index__"]))
        self.path = path

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            key = _call_key(name, args, kwargs)
            if key not in self._index:
                raise KeyError("%s%s: call not recorded in %s (re-record with tests/golden/make_reference_calls.py)"
                               % (name, tuple(type(a).__name__ for a in args), os.path.basename(self.path)))
            rec = self._index[key]
            if "raise" in rec:
                raise getattr(builtins, rec["raise"])("the reference raised %s here (recorded)" % rec["raise"])
            items = [self._arrays["%s.%d" % (key, i)] if kind == "array" else kind["json"]
                     for i, kind in enumerate(rec["items"])]
            return items[0] if rec["single"] else tuple(items)
        return call


class ReferenceRecorder:
    """Passes every call through to the live oracle and writes what it answered to `path` when the process ends."""

    def __init__(self, live, path):
        self._live, self._path, self._index, self._arrays = live, path, {}, {}
        atexit.register(self._save)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        fn = getattr(self._live, name)

        def call(*args, **kwargs):
            key = _call_key(name, args, kwargs)
            try:
                out = fn(*args, **kwargs)
            except Exception as e:
                assert getattr(builtins, type(e).__name__, None) is type(e), "not a builtin exception: %r" % e
                self._index[key] = {"name": name, "raise": type(e).__name__}
                raise
            single = not isinstance(out, tuple)
            items = []
            for i, x in enumerate([out] if single else out):
                if isinstance(x, np.ndarray):
                    self._arrays["%s.%d" % (key, i)] = x
                    items.append("array")
                else:
                    items.append({"json": x})
            self._index[key] = {"name": name, "single": single, "items": items}
            return out
        return call

    def _save(self):
        np.savez_compressed(self._path, __index__=np.array(json.dumps(self._index, sort_keys=True)), **self._arrays)


_ORACLES = {}


def reference_oracle(kind):
    """The reference's own compiled code as the tests see it: `kind` "cmatrices" is cmatrices.c behind oracle.binding's
    ctypes driver, "module" the reference's CPython module `_cmatrices`.  Answers come from the recordings under
    tests/golden/; with PRAD_RECORD_REFERENCE=1 (and oracle/_ref built from the reference) the live code answers and the
    recording is rewritten."""
    if kind not in _ORACLES:
        if os.environ.get(RECORD_ENV):
            from oracle import binding
            if not (binding.have_ref() and binding.have_ref_wrapper()):
                binding.build()
            live = binding.ref() if kind == "cmatrices" else binding.ref_wrapper()
            _ORACLES[kind] = ReferenceRecorder(live, REFERENCE_CALLS[kind])
        else:
            _ORACLES[kind] = RecordedReference(REFERENCE_CALLS[kind])
    return _ORACLES[kind]


CLASSES = ["glcm", "glrlm", "glszm", "gldm", "ngtdm"]          # the matrix-building classes
FEATURE_CLASSES = ["firstorder"] + CLASSES                      # everything with golden feature values


def feature_class(name):
    import importlib
    mod = importlib.import_module("pyradiomics_amd." + name)
    return getattr(mod, "RadiomicsFirstOrder" if name == "firstorder" else "Radiomics" + name.upper())


def load_case(case):
    from pyradiomics_amd.image import Image
    d = np.load(os.path.join(GOLDEN, case + ".npz"))
    image = Image(d["image"], spacing=d["spacing"])
    mask = Image(d["mask"].astype(np.int32), spacing=d["spacing"])
    return image, mask, {c: d["P_" + c] for c in CLASSES}


def load_baseline_features():
    with open(os.path.join(GOLDEN, "baseline_features.json")) as f:
        return json.load(f)


def prepared_case(cfg):
    """image / mask of a baseline configuration after the numpy-only preprocessing the reference's test harness
    applies (tests/testUtils.py: resegmentation then crop to the new ROI); returns (image, mask, settings)"""
    from pyradiomics_amd import imageoperations
    settings = {k: v for k, v in cfg["settings"].items() if v is not None}
    if settings.get("resampledPixelSpacing") is not None:
        # needs the whole grid (the B-spline prefilter is global): only the cases whose NRRD pair is kept in the repo
        from pyradiomics_amd.image import read_nrrd
        path = os.path.join(GOLDEN, "data", cfg["case"] + "_%s.nrrd")
        if not os.path.exists(path % "image"):
            import pytest
            pytest.skip("full image of %s is not part of the fixtures" % cfg["case"])
        image, mask = imageoperations.resampleImage(read_nrrd(path % "image"), read_nrrd(path % "label"), **settings)
        image, mask = imageoperations.cropToTumorMask(image, mask, settings.get("label", 1))
        for k in ("resampledPixelSpacing", "interpolator", "padDistance", "normalize", "normalizeScale", "removeOutliers"):
            settings.pop(k, None)
        return image, mask, settings
    image, mask, _ = load_case(cfg["case"])
    if settings.pop("normalize", False):
        # the reference normalises the WHOLE image before cropping (imageoperations.py:615-654); the fixtures hold the
        # ROI crop plus the whole-image mean / sigma, which is all normalizeImage depends on
        d = np.load(os.path.join(GOLDEN, cfg["case"] + ".npz"))
        arr = (image.array.astype(np.float64) - float(d["image_mean"])) / float(d["image_sigma"])
        if settings.get("removeOutliers") is not None:
            arr = np.clip(arr, -settings["removeOutliers"], settings["removeOutliers"])
        image = image.like(arr * float(settings.get("normalizeScale", 1)))
    for k in ("normalizeScale", "removeOutliers", "interpolator", "padDistance"):
        settings.pop(k, None)
    if cfg["settings"].get("resegmentRange") is not None:
        mask = imageoperations.resegmentMask(image, mask, **settings)
        image, mask = imageoperations.cropToTumorMask(image, mask, settings.get("label", 1))
    return image, mask, settings

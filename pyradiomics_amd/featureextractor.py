"""`RadiomicsFeatureExtractor`: the orchestration API of the reference's radiomics/featureextractor.py for the
path this package accelerates -- image types Original / Wavelet / LoG / Square / SquareRoot / Logarithm / Exponential /
Gradient / LBP2D, feature classes firstorder / glcm / glrlm / glszm / gldm / ngtdm, segment-based and voxel-based extraction --
without SimpleITK / pykwalify / scikit-image (not installed on the build and GPU hosts).  Same constructor forms (parameter file, dict, or keyword settings), the same enable*/disable* methods,
the same `execute(image, mask, label=None, voxelBased=False)` returning an OrderedDict keyed
`<imageType>_<featureClass>_<featureName>` (featureextractor.py:241-396, 560-604).

Not provided (out of scope): the shape classes,
the image type LBP3D (and LBP2D's method `var`), parameter-file schema validation.  Enabling them raises/ warns instead of silently
computing something else."""
from __future__ import annotations

import collections
import contextlib
import json
import logging
import os
from itertools import chain

import numpy as np

from . import __version__, backend, filters, imageoperations
from .image import Image, as_array, as_image, read_image

logger = logging.getLogger(__name__)

_FEATURE_CLASSES = ("firstorder", "glcm", "gldm", "glrlm", "glszm", "ngtdm")     # the reference's (alphabetical) order
_IMAGE_TYPES = {"Original": filters.getOriginalImage, "Wavelet": filters.getWaveletImage, "LoG": filters.getLoGImage,
                "Square": filters.getSquareImage, "SquareRoot": filters.getSquareRootImage,
                "Logarithm": filters.getLogarithmImage, "Exponential": filters.getExponentialImage,
                "Gradient": filters.getGradientImage, "LBP2D": filters.getLBP2DImage}


_feature_classes = None


def getFeatureClasses():
    """name -> class (radiomics/__init__.py:64-117), restricted to the classes on the accelerated path.  Built once:
    the reference caches its dictionary too (`_featureClasses`), and six importlib lookups per derived image were 0.6 ms
    of a 10 ms case."""
    global _feature_classes
    if _feature_classes is None:
        import importlib
        names = {"firstorder": "RadiomicsFirstOrder"}
        _feature_classes = {n: getattr(importlib.import_module("pyradiomics_amd." + n), names.get(n, "Radiomics" + n.upper()))
                            for n in _FEATURE_CLASSES}
    return dict(_feature_classes)


def getImageTypes():
    return list(_IMAGE_TYPES)


class RadiomicsFeatureExtractor:
    def __init__(self, *args, **kwargs):
        self.settings = {}
        self.enabledImagetypes = {}
        self.enabledFeatures = {}
        self.featureClassNames = list(_FEATURE_CLASSES)
        if len(args) == 1 and isinstance(args[0], dict):
            self._applyParams(paramsDict=args[0])
            self.settings.update(kwargs)          # keyword settings override the parameter set (featureextractor.py:117-137)
        elif len(args) == 1 and isinstance(args[0], (str, os.PathLike)):
            self._applyParams(paramsFile=args[0])
            self.settings.update(kwargs)
        else:
            self.settings = self._getDefaultSettings()
            self.settings.update(kwargs)
            self.enabledImagetypes = {"Original": {}}
            self.enabledFeatures = {n: [] for n in self.featureClassNames}

    _labelsRoute = None

    def lastLabelsRoute(self):
        """{"batched": [...], "single": [...], "mixed": [...]}: which way the labels of the last FINISHED executeLabels call
        went, each list in the order the results were yielded.  "batched": every value came from the batched small-ROI
        kernels; "mixed": batched, with at least one (label, derived image) pair recomputed by the per-label class pipeline;
        "single": the per-label steps (every label without `batched=True`).  Skipped labels are in no list."""
        route = self._labelsRoute or {}
        return {k: list(route.get(k, ())) for k in ("batched", "single", "mixed")}

    def lastLabelsRecomputed(self):
        """[(label, image type name)] of that call: the pairs of its "mixed" labels the per-label class pipeline recomputed"""
        return list((self._labelsRoute or {}).get("recomputed", ()))

    @staticmethod
    def _getDefaultSettings():
        # featureextractor.py:139-163 (keys that reach the accelerated path keep their defaults)
        return {"minimumROIDimensions": 2, "minimumROISize": None, "normalize": False, "normalizeScale": 1,
                "removeOutliers": None, "resampledPixelSpacing": None, "interpolator": "sitkBSpline", "preCrop": False,
                "padDistance": 5, "distances": [1], "force2D": False, "force2Ddimension": 0, "resegmentRange": None,
                "label": 1, "additionalInfo": True}

    # -- configuration (featureextractor.py:165-239, 606-763) ----------------------------------------------
    def loadParams(self, paramsFile):
        self._applyParams(paramsFile=paramsFile)

    def loadJSONParams(self, jsonString):
        self._applyParams(paramsDict=json.loads(jsonString))

    def _applyParams(self, paramsFile=None, paramsDict=None):
        if paramsFile is not None:
            import yaml
            with open(paramsFile) as f:
                params = yaml.safe_load(f)
        else:
            params = paramsDict
        params = params or {}
        # the reference validates against radiomics/schemas/paramSchema.yaml here (pykwalify)
        from . import paramcheck
        paramcheck.validate(params, list(_IMAGE_TYPES), {n: list(c.getFeatureNames()) for n, c in getFeatureClasses().items()})
        self.settings = self._getDefaultSettings()
        self.settings.update(params.get("setting") or {})
        self.settings.update(params.get("voxelSetting") or {})
        types = params.get("imageType")
        self.enabledImagetypes = {"Original": {}} if not types else {k: (v or {}) for k, v in types.items()}
        for t in self.enabledImagetypes:
            if t not in _IMAGE_TYPES:
                raise NotImplementedError("image type %r is outside the accelerated path (available: %s)"
                                          % (t, ", ".join(_IMAGE_TYPES)))
        classes = params.get("featureClass")
        if not classes:
            self.enabledFeatures = {n: [] for n in self.featureClassNames}
        else:
            self.enabledFeatures = {}
            for k, v in classes.items():
                if k not in self.featureClassNames:
                    logger.warning("feature class %r is outside the accelerated path and is skipped", k)
                    continue
                self.enabledFeatures[k] = list(v) if v else []

    def addProvenance(self, provenance_on=True):
        self.settings["additionalInfo"] = provenance_on

    def enableAllImageTypes(self):
        self.enabledImagetypes = {t: {} for t in _IMAGE_TYPES}

    def disableAllImageTypes(self):
        self.enabledImagetypes = {}

    def enableImageTypeByName(self, imageType, enabled=True, customArgs=None):
        if imageType not in _IMAGE_TYPES:
            raise NotImplementedError("image type %r is outside the accelerated path" % imageType)
        if enabled:
            self.enabledImagetypes[imageType] = customArgs or {}
        else:
            self.enabledImagetypes.pop(imageType, None)

    def enableImageTypes(self, **enabledImagetypes):
        for k, v in enabledImagetypes.items():
            self.enableImageTypeByName(k, True, v)

    def enableAllFeatures(self):
        self.enabledFeatures = {n: [] for n in self.featureClassNames}

    def disableAllFeatures(self):
        self.enabledFeatures = {}

    def enableFeatureClassByName(self, featureClass, enabled=True):
        if featureClass not in self.featureClassNames:
            logger.warning("Feature class %s is not recognized", featureClass)
            return
        if enabled:
            self.enabledFeatures[featureClass] = []
        else:
            self.enabledFeatures.pop(featureClass, None)

    def enableFeaturesByName(self, **enabledFeatures):
        for k, v in enabledFeatures.items():
            if k in self.featureClassNames:
                self.enabledFeatures[k] = list(v) if v else []
            else:
                logger.warning("Feature class %s is not recognized", k)

    # -- execution ---------------------------------------------------------------------------------------
    @staticmethod
    def loadImage(imageFilepath, maskFilepath, **kwargs):
        """paths to NRRD / NIfTI-1 / MetaImage files, pyradiomics_amd.image.Image objects, or numpy arrays (z, y, x)"""
        def load(x):
            if isinstance(x, (str, os.PathLike)):
                return read_image(os.fspath(x))
            return as_image(x)
        image, mask = load(imageFilepath), load(maskFilepath)
        if getattr(mask, "components", None) is None and len(mask.shape) == len(image.shape) + 1:
            # an array with a trailing component axis (a vector mask given without file geometry)
            mask = Image(mask.array, image.GetSpacing(), image.GetOrigin(), image.GetDirection())
        if getattr(mask, "components", None) is not None or len(mask.shape) == len(mask.GetSpacing()) + 1:
            mask = imageoperations.getMask(mask, **kwargs)      # the channel of a vector mask (label_channel)
        # (a scalar mask is not scanned here: execute() finds a missing label when it takes the bounding box, on the
        # device, and raises the same "Label (..) not present in mask")
        if len(image.shape) != len(mask.shape):
            raise ValueError("Image/Mask datatype or size mismatch: %s vs %s" % (image.shape, mask.shape))
        # imageoperations.checkMask step 1 (:241-287): same grid within geometryTolerance, or correctMask resamples
        mask = imageoperations.checkMaskGeometry(image, mask, **kwargs)
        return image, mask

    def execute(self, imageFilepath, maskFilepath, label=None, label_channel=None, voxelBased=False):
        """featureextractor.py:241-343: every enabled feature of every enabled image type for one (image, mask) pair"""
        steps = self._executeSteps(imageFilepath, maskFilepath, label, label_channel, voxelBased)
        try:
            while True:
                next(steps)
        except StopIteration as done:
            return done.value

    def executeMany(self, cases, label=None, label_channel=None, voxelBased=False):
        """Generator over the results of `cases` -- (image, mask) pairs, or (image, mask, label) -- in their order, with ONE CASE OF
        OVERLAP on this thread: case i + 1 is loaded, uploaded, filtered and its first derived images queued before the values of
        case i's last derived image are collected, so the GPU works through case i's tail while the host does case i + 1's head
        (the upload of a 256^3 case alone is 1.3 ms in which nothing else of that case can run).  Results are those of
        execute(), bit for bit (the same calls in the same order per case; only the collection of the last image moves).  The
        reference's batch mode is a process pool over cases (scripts/__init__.py:387-416); this is its one-process form for a
        GPU.  A case that raises is reported by re-raising at its position; the case in flight behind it is abandoned."""
        prev, cur = None, None
        try:
            for case in cases:
                lab = case[2] if len(case) > 2 else label
                steps = self._executeSteps(case[0], case[1], lab, label_channel, voxelBased)
                try:
                    next(steps)                      # head of this case: loaded, uploaded, filtered, its FIRST derived image queued
                    cur = (steps, None)
                except StopIteration as done:        # (nothing was left pending: e.g. no derived image)
                    cur = (None, done.value)
                if prev is not None:
                    last, prev = prev, None
                    yield self._finishSteps(last)    # the previous case's last image: its kernels ran under this case's head
                if cur[0] is not None:
                    try:
                        next(cur[0])                 # the body: every image but the last collected, the last one left queued
                    except StopIteration as done:
                        cur = (None, done.value)
                prev, cur = cur, None
            if prev is not None:
                last, prev = prev, None
                yield self._finishSteps(last)
        finally:
            for state in (prev, cur):
                if state is not None and state[0] is not None:
                    state[0].close()                 # (abandons what the unfinished case queued)

    def executeLabels(self, imageFilepath, maskFilepath, labels=None, label_channel=None, batched=False):
        """Generator of (label, result) over the labels of ONE label map: every label the map holds, ascending, or `labels` in
        their order.  Each result is execute(image, mask, label=l), key for key and bit for bit, diagnostics included; what
        does not depend on the label is done once per call instead of once per label:
          - image and mask are loaded and uploaded once;
          - one census of the map (imageoperations.labelCensus: a single pass) gives every label's voxel count and bounding
            box, so no label scans the map for its ROI;
          - the derived images of the enabled image types (the wavelet's sub-bands, the LoG's sigmas ...) are produced once;
          - each label's crops go through the per-image pipeline of execute() with its one-image look-ahead, and label i + 1's
            first crop is queued before label i's last image is collected (as executeMany overlaps cases).
        When a setting makes the IMAGE depend on the label -- `resampledPixelSpacing` with an interpolator, `preCrop` -- the
        derived images cannot be shared: the call still loads and counts once and then runs execute()'s steps label by label
        (the same results; the filter stack is repeated per label).  `resegmentRange` changes the MASK alone: the derived images
        stay shared and every label is resegmented on the device (imageoperations.resegmentMask) in its own steps.
        Peak memory: the shared path keeps every derived image of the call alive until the last label is done (Wavelet: 8
        full-size float64 sub-bands, LoG: one image per sigma -- 1.2 GB for a 256^3 case with Wavelet and one sigma), where
        execute() holds the ones in flight.
        With labels=None a label that fails an ROI check of execute() (minimumROIDimensions, minimumROISize, absent after
        processing) is skipped with a logged warning; with an explicit list the ValueError of execute() is raised at that
        label's position, after the results of the labels before it.  Segment-based extraction only.
        batched=True: the labels inside the domain of the batched small-ROI kernels (_batchedLabels) are not run one by one:
        their boxes are gathered on the device (one launch for the masks, one per derived image) and every derived image
        costs one engine.roi_features_batch for all of them.  Results, order, failures and warnings are those of the default
        mode -- texture features, order statistics and counts bit for bit; the summed first-order features come from the
        batched kernel's own summation order -- and every other label takes the per-label steps unchanged.
        With `resegmentRange` batched=True is not wired to engine.resegment_batch: every label keeps taking the per-label steps
        (lastLabelsRoute() lists them as "single"), with the shared filter stack and the device resegmentation.
        lastLabelsRoute() tells which label went which way."""
        s = self.settings.copy()
        if labels is not None:
            labels = [l for l in labels]
            if labels:
                s["label"] = labels[0]        # (loadImage checks a vector mask for the label it is given)
        if label_channel is not None:
            s["label_channel"] = label_channel
        # (without a label list no label is asked of the mask while loading: the channel of a vector mask is picked and a
        # `correctMask` geometry check looks at the box of all labelled voxels)
        image, mask = self.loadImage(imageFilepath, maskFilepath, **(dict(s, label=None) if labels is None else s))
        on_dev = bool(s.get("deviceResident", True)) and getattr(backend.get(), "DEVICE_TENSORS", False)
        s["deviceResident"] = on_dev
        present = imageoperations.labelCensus(mask, deviceResident=on_dev)[0]
        discover = labels is None
        if discover:
            labels = [int(l) for l in present]
            if not labels:
                raise ValueError("No labels found in this mask (i.e. nothing is segmented)!")
        per_label_image = ((s.get("resampledPixelSpacing") is not None and s.get("interpolator") is not None)
                           or s.get("preCrop", False))
        shared = None
        if not per_label_image:
            s["label"] = self.settings.get("label", 1)
            base = imageoperations.normalizeImage(image, **s) if s.get("normalize", False) else image
            shared = (base, list(self._derivedImages(base, mask, s)))
        route = {"batched": [], "single": [], "mixed": []}
        ready, mixed = {}, {}
        if batched and shared is not None and on_dev and s.get("resegmentRange") is None:
            ready, mixed = self._batchedLabels(image, mask, labels, shared, s)
        prev, cur = None, None
        try:
            for lab in labels:
                feats = ready.get(self._labelKey(lab)) if ready else None
                if feats is not None:                # (computed with the whole batched set, before the first result)
                    if prev is not None:
                        last, prev = prev, None
                        yield last[0], self._finishSteps(last[1:])
                    prev = (lab, None, self._batchedResult(image, mask, lab, label_channel, on_dev, feats))
                    route["mixed" if self._labelKey(lab) in mixed else "batched"].append(lab)
                    continue
                steps = self._executeSteps(image, mask, lab, label_channel, False, shared=shared)
                failed = None
                try:
                    next(steps)                      # head of this label: ROI checks, its first crop queued
                    cur = (lab, steps, None)
                    route["single"].append(lab)
                except StopIteration as done:
                    cur = (lab, None, done.value)
                    route["single"].append(lab)
                except ValueError as e:
                    if discover:
                        logger.warning("label %s skipped: %s", lab, e)
                        continue
                    failed = e
                if prev is not None:
                    last, prev = prev, None
                    yield last[0], self._finishSteps(last[1:])
                if failed is not None:
                    raise failed
                if cur[1] is not None:
                    try:
                        next(cur[1])                 # the body: every image but the last collected
                    except StopIteration as done:
                        cur = (lab, None, done.value)
                prev, cur = cur, None
            if prev is not None:
                last, prev = prev, None
                yield last[0], self._finishSteps(last[1:])
            route["recomputed"] = [(lab, name) for lab in route["mixed"] for name in mixed[self._labelKey(lab)]]
            self._labelsRoute = route
        finally:
            for state in (prev, cur):
                if state is not None and state[1] is not None:
                    state[1].close()                 # (abandons what the unfinished label queued: _abandonFeatures)

    # -- executeLabels(batched=True): the labels the batched small-ROI kernels take ------------------------------
    @staticmethod
    def _labelKey(label):
        """the census's key of a label (int), None for what the census does not count"""
        try:
            return int(label) if label == int(label) and int(label) >= 1 else None
        except (TypeError, ValueError):
            return None

    def _batchedColumns(self):
        """{class: [(feature name, column of engine.roi_features_batch's table)]} for the enabled features, in the order
        execute() returns them (the names given to enableFeaturesByName, or every feature that is not deprecated), or None
        when a feature is enabled that the batched tables do not hold"""
        from . import cmatrices
        classes = getFeatureClasses()
        cols = {}
        for cname, fnames in self.enabledFeatures.items():
            if cname not in classes:
                continue
            held = cmatrices.FIRSTORDER_FEATURES if cname == "firstorder" else cmatrices.batch_feature_names(cname)
            names = (list(dict.fromkeys(fnames)) if fnames
                     else [n for n, dep in classes[cname].getFeatureNames().items() if not dep])
            if not names or any(n not in held for n in names):
                return None
            cols[cname] = [(n, held.index(n)) for n in names]
        return cols or None

    def _batchedLabels(self, image, mask, labels, shared, s):
        """The feature values of every label of `labels` inside the batched domain: -> ({label: OrderedDict of its
        <imageType>_<class>_<feature> values in execute()'s order}, {label: [image type names]} of the recomputed pairs).
        Domain of the call: 3-D image, no weightingNorm, no force2D, the fused device formulas (`fusedSegment`), every enabled
        feature a column of the batched tables.  Domain of a label: present, no axis of extent 1, passes minimumROISize /
        minimumROIDimensions.  The boxes are those cropToTumorMask(padDistance=0, alignRows=True) cuts, so the batched
        kernels read the very arrays the per-label classes read.  A (label, derived image) pair whose row lacks a value --
        MCC above 64 grey levels, a derived image of an element type the kernels do not read -- is recomputed by the class
        pipeline on that crop: NaN never stands in for a value execute() has."""
        derived = shared[1]
        cols = self._batchedColumns()
        if cols is None or not derived or len(image.shape) != 3 or len(mask.shape) != 3:
            return {}, {}
        for _img, _name, kw in derived:
            if kw.get("weightingNorm") is not None or kw.get("force2D", False) or not kw.get("fusedSegment", True):
                return {}, {}
        if s.get("minimumROIDimensions", 2) > 3:
            return {}, {}
        chosen = {}
        for lab in labels:
            key = self._labelKey(lab)
            known = imageoperations.censusLookup(mask, lab) if key is not None else None
            if known is None or known[0] == 0 or key in chosen:
                continue
            count, lo, hi = known
            if (hi - lo + 1 <= 1).any() or (s.get("minimumROISize") is not None and count <= s["minimumROISize"]):
                continue
            chosen[key] = (lo, hi)
        if not chosen:
            return {}, {}
        from . import cmatrices
        engine = imageoperations._engine()
        keys = list(chosen)
        lo, hi = imageoperations.alignedBox(np.stack([chosen[k][0] for k in keys]), np.stack([chosen[k][1] for k in keys]),
                                            mask.shape)
        labelmap = mask.device_tensor()
        _, flat_m, sizes = engine.gather_rois_batch(None, labelmap, keys, lo, hi, masks=True, images=False)
        feats = {k: collections.OrderedDict() for k in keys}
        mixed = {}
        for dimg, typeName, kw in derived:
            t = dimg.device_tensor()
            table = None
            if t.dtype in engine._DTYPE_CODES and tuple(t.shape) == tuple(labelmap.shape):
                flat_i, _, _ = engine.gather_rois_batch(t, None, keys, lo, hi, masks=False, images=True)
                table, status = engine.roi_features_batch(
                    flat_i, flat_m, sizes, classes=tuple(cols), binWidth=kw.get("binWidth"), binCount=kw.get("binCount"),
                    voxelArrayShift=kw.get("voxelArrayShift", 0), voxelVolume=np.multiply.reduce(dimg.GetSpacing()),
                    distances=[int(d) for d in np.asarray(kw.get("distances", [1])).ravel()], gldm_a=int(kw.get("gldm_a", 0)),
                    symmetricalGLCM=bool(kw.get("symmetricalGLCM", True)), extras=True)
            for b, k in enumerate(keys):
                block = collections.OrderedDict()
                whole = table is not None and bool(status[b])
                if whole:
                    for cname, pairs in cols.items():
                        row = table[cname][b]
                        for fname, col in pairs:
                            value = row[col]
                            if cname == "glcm" and fname == "MCC":
                                # as RadiomicsGLCM reports it: 1 for a ROI of one grey level, else the flat mean over the angles
                                per_angle = table["glcm_mcc_angles"][b]
                                value = (1.0 if table["gray_levels"][b] < 2 else
                                         np.nan if per_angle is None else cmatrices._mcc_angle_mean(per_angle))
                            block["%s_%s_%s" % (typeName, cname, fname)] = np.array(value)
                    whole = not any(np.isnan(v) for v in block.values())
                if not whole:
                    cimg, cmask = imageoperations.cropToTumorMask(dimg, mask, k, padDistance=0, deviceResident=True)
                    block = self.computeFeatures(cimg, cmask, typeName, **dict(kw, label=k))
                    mixed.setdefault(k, []).append(typeName)
                feats[k].update(block)
        return feats, mixed

    def _batchedResult(self, image, mask, label, label_channel, on_dev, feats):
        """the result of one batched label: execute()'s diagnostics, from the census, in front of its feature values"""
        s = self.settings.copy()
        s["label"] = label
        if label_channel is not None:
            s["label_channel"] = label_channel
        s["deviceResident"] = on_dev
        out = collections.OrderedDict()
        if s.get("additionalInfo", True):
            nvox, blo, bhi = imageoperations.censusLookup(mask, label)
            out["diagnostics_Versions_PyRadiomicsAMD"] = __version__
            out["diagnostics_Versions_Numpy"] = np.__version__
            out["diagnostics_Configuration_Settings"] = {k: v for k, v in s.items()}
            out["diagnostics_Configuration_EnabledImageTypes"] = dict(self.enabledImagetypes)
            out["diagnostics_Image-original_Spacing"] = image.GetSpacing()
            out["diagnostics_Image-original_Size"] = image.GetSize()
            out["diagnostics_Mask-original_Spacing"] = mask.GetSpacing()
            out["diagnostics_Mask-original_Size"] = mask.GetSize()
            out["diagnostics_Mask-original_BoundingBox"] = tuple(int(v) for v in blo[::-1]) + \
                tuple(int(v) for v in (bhi - blo + 1)[::-1])
            out["diagnostics_Mask-original_VoxelNum"] = nvox
        out.update(feats)
        return out

    @staticmethod
    def _finishSteps(state):
        steps, value = state
        if steps is None:
            return value
        try:
            while True:
                next(steps)
        except StopIteration as done:
            return done.value

    def _executeSteps(self, imageFilepath, maskFilepath, label=None, label_channel=None, voxelBased=False, shared=None):
        """execute() as a generator that yields TWICE -- when the case's first derived image is queued (executeMany collects the
        previous case's last image there: at most two images of two cases in flight, the library's tickets are a ring of four) and
        when everything is queued or collected except the values of the last derived image -- and returns what execute() returns.
        `shared` (executeLabels): (image, derived) -- the image as it stands after the label-independent steps and the list of
        (derived image, name, kwargs) of the enabled image types, produced once for all labels of the case"""
        s = self.settings.copy()
        if label is not None:
            s["label"] = label
        if label_channel is not None:
            s["label_channel"] = label_channel
        label = s.get("label", 1)

        kernelRadius = 0
        if voxelBased:
            s["voxelBased"] = True
            kernelRadius = s.get("kernelRadius", 1)
        out = collections.OrderedDict()
        image, mask = self.loadImage(imageFilepath, maskFilepath, **s)
        # Segment-based extraction keeps the case in HBM: one upload of image + mask, then filters, crop,
        # discretisation and the matrices all work on device tensors (`deviceResident: False` restores the
        # host-array route of the reference; voxel-based extraction batches host coordinates and uses it too).
        on_dev = (bool(s.get("deviceResident", True)) and not voxelBased
                  and getattr(backend.get(), "DEVICE_TENSORS", False))
        s["deviceResident"] = on_dev
        info = collections.OrderedDict()

        def describe(stage, img, msk):
            """diagnostics_Image-<stage>_* / diagnostics_Mask-<stage>_* (generalinfo.py:97-190, the subset that needs
            no SimpleITK label statistics)"""
            known = imageoperations.censusLookup(msk, label)      # (a census of this mask, when one was taken: no scan)
            if known is not None:
                nvox, blo, bhi = known
                if nvox == 0:
                    raise ValueError("Label (%g) not present in mask" % label)
            else:
                on = msk.on_device or (on_dev and stage != "original")
                r = imageoperations.roiTensor(msk, label) if on else (msk.array == label)
                try:
                    blo, bhi = imageoperations.boundingBox(r)
                except ValueError:
                    raise ValueError("Label (%g) not present in mask" % label)
            info["diagnostics_Image-%s_Spacing" % stage] = img.GetSpacing()
            info["diagnostics_Image-%s_Size" % stage] = img.GetSize()
            info["diagnostics_Mask-%s_Spacing" % stage] = msk.GetSpacing()
            info["diagnostics_Mask-%s_Size" % stage] = msk.GetSize()
            info["diagnostics_Mask-%s_BoundingBox" % stage] = tuple(int(v) for v in blo[::-1]) + \
                tuple(int(v) for v in (bhi - blo + 1)[::-1])
            info["diagnostics_Mask-%s_VoxelNum" % stage] = int(r.sum()) if known is None else nvox

        if s.get("additionalInfo", True):
            describe("original", image, mask)
        if shared is not None:
            image = shared[0]                          # (normalised once for all labels)
        elif s.get("normalize", False):                # featureextractor.py:432-433: before anything else sees the image
            image = imageoperations.normalizeImage(image, **s)
        # :436-440 (the reference's loadImage only resamples when BOTH the spacing and an interpolator are given)
        if s.get("resampledPixelSpacing") is not None and s.get("interpolator") is not None:
            if not np.any(mask.array == label):
                raise ValueError("Label (%g) not present in mask" % label)
            image, mask = imageoperations.resampleImage(image, mask, **s)
            if s.get("additionalInfo", True):
                describe("interpolated", image, mask)
        elif s.get("preCrop", False):
            # featureextractor.py:471-482: work on the ROI's bounding box grown by padDistance from here on (a speed-up
            # the user opts into; filters then see the crop's borders instead of the image's)
            image, mask = imageoperations.cropToTumorMask(image, mask, label, padDistance=s.get("padDistance", 5),
                                                          deviceResident=on_dev, alignRows=False)
        if s.get("resegmentRange") is not None:
            known = imageoperations.censusLookup(mask, label)      # (a census of this mask answers without a scan)
            if (known[0] == 0) if known is not None else not np.any(mask.array == label):
                raise ValueError("Label (%g) not present in mask" % label)
            mask = imageoperations.resegmentMask(image, mask, **s)
            if s.get("additionalInfo", True):
                describe("resegmented", image, mask)
        known = imageoperations.censusLookup(mask, label)
        if known is not None:
            nroi, lo, hi = known
            if nroi == 0:
                raise ValueError("Label (%g) not present in mask" % label)
        else:
            roi = imageoperations.roiTensor(mask, label) if on_dev else (mask.array == label)
            try:
                lo, hi = imageoperations.boundingBox(roi)
            except ValueError:
                raise ValueError("Label (%g) not present in mask" % label)
            nroi = int(roi.sum())
        mask._derived[("bbox", label)] = (lo, hi)
        ndims = int(np.sum(hi - lo + 1 > 1))
        if ndims < s.get("minimumROIDimensions", 2):
            raise ValueError("mask has too few dimensions (number of dimensions %d, minimum required %d)"
                             % (ndims, s.get("minimumROIDimensions", 2)))
        if s.get("minimumROISize") is not None and nroi <= s["minimumROISize"]:
            raise ValueError("Size of the ROI is too small (minimum size: %g)" % s["minimumROISize"])
        if s.get("additionalInfo", True):
            out["diagnostics_Versions_PyRadiomicsAMD"] = __version__
            out["diagnostics_Versions_Numpy"] = np.__version__
            out["diagnostics_Configuration_Settings"] = {k: v for k, v in s.items()}
            out["diagnostics_Configuration_EnabledImageTypes"] = dict(self.enabledImagetypes)
            out.update(info)
        if shared is not None:
            # the derived images do not depend on the label; the keyword set handed on with each does (`label`)
            gens = ((derived, typeName, dict(kw, label=label)) for derived, typeName, kw in shared[1])
        else:
            gens = self._derivedImages(image, mask, s)
        # Look-ahead: image i + 1 is cropped and its discretisation QUEUED (prebinDevice: no round trip) right behind the device
        # classes of image i, and the host collects image i - 1 after that -- the GPU works through a queue while the host does
        # its Python, and the one round trip of a binning (ROI min / max -> number of levels) has passed by the time the classes
        # of image i + 1 are constructed; results keep the reference's order (featureextractor.py:371-396: image after image).
        from .base import RadiomicsFeaturesBase
        bins = on_dev and bool(self.enabledFeatures)      # (every class discretises: first order for its entropy / uniformity)
        it = iter(gens)

        def fetch():
            try:
                derived, typeName, kw = next(it)
            except StopIteration:
                return None
            cimg, cmask = imageoperations.cropToTumorMask(derived, mask, label, padDistance=kernelRadius, deviceResident=on_dev)
            if bins:
                RadiomicsFeaturesBase.prebinDevice(cimg, cmask, **kw)
            return cimg, cmask, typeName, kw

        pending, nxt, head_done = None, None, False
        try:
            nxt = fetch()
            while nxt is not None:
                cur, nxt = nxt, None
                try:
                    started = self._startFeatures(cur[0], cur[1], cur[2], **cur[3])
                except BaseException:
                    RadiomicsFeaturesBase.dropPrebinned(cur[0])
                    raise
                prev, pending = pending, started
                if prev is None and not head_done:
                    head_done = True
                    yield                          # (executeMany: the previous case's last image is collected here)
                try:
                    nxt = fetch()
                except BaseException:
                    if prev is not None:
                        self._abandonFeatures(prev)
                    raise
                if prev is not None:
                    out.update(self._finishFeatures(prev))      # (abandons `prev` itself when it fails)
            if pending is not None:
                yield                              # (executeMany: the next case's head runs here; GeneratorExit abandons `pending`)
                last, pending = pending, None
                out.update(self._finishFeatures(last))
        except BaseException:
            # an exception between "queued" and "collected" (the next image's filter / crop / binning, a host class): the
            # queued image still holds a ticket of the library's in-flight table (4 per thread) and its side streams hold
            # tensors -- retire them, or every later case on this (persistent batch worker) thread fails
            if pending is not None:
                self._abandonFeatures(pending)
            if nxt is not None:
                RadiomicsFeaturesBase.dropPrebinned(nxt[0])
            raise
        return out

    def _derivedImages(self, image, mask, s):
        """(derived image, name, kwargs) of every enabled image type, in their order (featureextractor.py:371-396)"""
        gens = []
        for imageType, custom in self.enabledImagetypes.items():
            args = s.copy()
            args.update(custom)
            gens = chain(gens, _IMAGE_TYPES[imageType](image, mask, **args))
        return gens

    @staticmethod
    def _abandonFeatures(started):
        """waits for and discards everything _startFeatures queued for one derived image (never raises; idempotent: a token
        that was already waited for -- `tokens[i] is None` -- is not waited for a second time)"""
        fcs, queued, tokens, _name = started
        cm = queued[0].cMatrices if queued else (fcs[0][1].cMatrices if fcs else None)
        for i, wait in ((0, "segment_image_wait"), (1, "segment_wait")):
            tok, tokens[i] = tokens[i], None
            if tok is not None and cm is not None:
                try:
                    getattr(cm, wait)(tok)
                except Exception:          # noqa: BLE001 -- the original exception is the one to report
                    pass
        for fc in queued:
            try:
                fc.dropEnqueued()
            except Exception:              # noqa: BLE001
                pass

    def computeFeatures(self, image, mask, imageTypeName, **kwargs):
        """featureextractor.py:560-604"""
        return self._finishFeatures(self._startFeatures(image, mask, imageTypeName, **kwargs))

    def _startFeatures(self, image, mask, imageTypeName, **kwargs):
        """first half of computeFeatures: the feature classes of one derived image constructed (binning), the device
        classes' kernels queued; -> state for _finishFeatures"""
        classes = getFeatureClasses()
        fcs = []
        for cname, fnames in self.enabledFeatures.items():
            if cname not in classes:
                continue
            fc = classes[cname](image, mask, **kwargs)
            for f in fnames or []:
                fc.enableFeatureByName(f)
            fcs.append((cname, fc))
        # Case pipeline: every class whose work runs on the device without a host round trip (GLCM, GLRLM, GLSZM, GLDM, NGTDM,
        # first order of float images) queues all of its kernels first, on side streams; the rest (first order of the
        # int16 original: exact histogram) runs on the main stream while those queues drain; then ONE wait per image.  The reference evaluates class after
        # class (featureextractor.py:560-604), each with its own round trips.
        cm = fcs[0][1].cMatrices if fcs else None
        side = hasattr(cm, "segment_queue") and fcs[0][1].deviceResident
        queued, names, ticket = [], [], [None]
        try:
            return self._queueFeatures(fcs, cm, side, queued, names, ticket, imageTypeName, kwargs)
        except BaseException:
            # a class that fails to queue after the image call went through: retire that call's ticket before re-raising
            self._abandonFeatures((fcs, queued, [ticket[0], None], imageTypeName))
            raise

    def _queueFeatures(self, fcs, cm, side, queued, names, ticket, imageTypeName, kwargs):
        # one library call queues every class the fused kernels cover (cMatrices.segment_image_enqueue) ...
        image_token = None
        if side and hasattr(cm, "segment_image_enqueue"):
            reqs = {}
            for cname, fc in fcs:
                rq = fc.imageRequest() if hasattr(fc, "imageRequest") else None
                if rq is not None and rq[0] not in reqs:
                    reqs[rq[0]] = (fc, rq[1])
            if reqs:
                any_fc = next(iter(reqs.values()))[0]
                levels = getattr(any_fc, "discretizedImageArray", any_fc.imageArray)
                image_token, finishes = cm.segment_image_enqueue(
                    levels, any_fc.maskArray, any_fc.coefficients["Ng"], any_fc.coefficients["Ns"],
                    {k: rq for k, (fc, rq) in reqs.items()}, force2D=kwargs.get("force2D", False),
                    force2Ddimension=kwargs.get("force2Ddimension", 0))
                ticket[0] = image_token
                for k, fin in finishes.items():
                    reqs[k][0].takeEnqueued(fin)
                    queued.append(reqs[k][0])
        # ... the others queue on their own (or compute in _finishFeatures)
        for cname, fc in fcs:
            if fc in queued:
                continue
            with (cm.segment_queue(cname) if side else contextlib.nullcontext()):
                if fc.enqueue():
                    queued.append(fc)
                    names.append(cname)
        token = cm.segment_mark(names) if names else None
        return fcs, queued, [image_token, token], imageTypeName

    def _finishFeatures(self, started):
        """second half of computeFeatures: the host-side classes evaluated, the queued ones waited for and collected"""
        fcs, queued, tokens, imageTypeName = started
        out = collections.OrderedDict()
        try:
            # (everything below runs under the guard: a failing host class, a failing wait -- the library's generation check, a
            # HIP error -- or a failing collect leaves no ticket un-retired and no queued class holding its results: ADVICE r4)
            values = {cname: fc.execute() for cname, fc in fcs if fc not in queued}
            if queued:
                cm = queued[0].cMatrices
                ok = True
                for i, wait in ((0, cm.segment_image_wait), (1, cm.segment_wait)):
                    tok, tokens[i] = tokens[i], None          # (marked as waited first: the abandon path must not wait again)
                    if tok is not None:
                        ok = wait(tok) and ok
                if not ok:
                    for fc in queued:      # a level outside [1, Ng]: the synchronous route raises what the reference raises
                        fc.dropEnqueued()
            for cname, fc in fcs:
                for fname, value in (values[cname] if cname in values else fc.execute()).items():
                    out["%s_%s_%s" % (imageTypeName, cname, fname)] = value
        except BaseException:
            self._abandonFeatures(started)
            raise
        return out

"""GPU: the three resampling kernels (csrc/kernels_resample.h: to_f64_kernel, bspline_prefilter_kernel, resample_kernel) at their
limits, every case through engine.resample itself, against tests/resample_reference.py (numpy long double, its own code).
tests/test_resample_reference.py pins that reference to itself, holds the host numpy route to the same bounds and shows that
each family below moves under the hazard it exists to catch.

Case families (resample_reference.GROUPS):
  prefilter     N in {1, 2, 3, 4, 17, 18, 19, 20, 40} on each axis in turn, the other two 3 and 5 (the three stride cases of the
                prefilter; N = 18 -> 19 is the switch from the exact mirror sum to the 18-tap start; N = 2 and 3 have an empty
                sum), and (3, 90, 19): 270 lines, a ragged second block.  Identity grid (the output reproduces the input) and the
                half-sample grid start -0.25, step 0.5.  float64 and float32.
  geometry      per axis at N in {1, 2, 3, 5}: quarter steps from exactly -0.5 (inside) to exactly N - 0.5 (outside), so also
                [-0.5, 0) and (N - 1, N - 0.5); steps of 0.7 from four voxels before the buffer to four behind it (0 there).
                Nearest, linear and B-spline, float64 and float32.
  mirror        B-spline at N = 2 and 3 in eighths: the support -2 .. N + 1 wraps the period 2N - 2 more than once
  ties          nearest with outputs exactly on k + 0.5 on every axis: int16, int32, float32, float64 and a label map up to 32767
  unfused       (start 0.3, step 0.3, o 24): 7.5 - 2^-50 in float64, inside N = 8; one rounding (a fused multiply-add) gives 7.5,
                outside.  (start -0.3, step 0.15, o 12): 1.5 - 2^-52 -> voxel 1; fused, the tie 1.5 -> voxel 2.
  integer       int16 / int32 checkerboards of the type's two extremes (their spline is a product of cosine-like factors and stays
                inside the range: 0.98 of it off the samples, so the checkerboard alone reaches neither clamp), 2-voxel blocks of
                the extremes (the B-spline reaches 2.7 times the range, a third of the outputs are clamped, both ends), five-valued
                images around 0 (three in ten outputs in (-1, 0), where floor and truncation differ); short lines, start -0.3,
                step 0.37: no output on a sample.  Linear and B-spline.
  dims          (1,) (2,) (7,) (19,) (1, 6) (4, 1) (5, 19): bit for bit the 3-D call with leading 1s, and the reference
  stride        nearest int16 (20, 24, 28) -> (164, 160, 161), 4 224 640 outputs > 16384 * 256: equal to numpy take;
                B-spline float32 (130, 128, 127), 2 113 280 voxels > 8192 * 256, on a sparse 6 x 7 x 8 grid that reaches the last plane
  filters       the shapes on which tests/test_gpu_filters.py used rtol 1e-6 / atol 1e-4 (float32; (1, 33, 30)): device AND host
                route against the reference, on the grid resampleImage hands to engine.resample

Bounds (derived in resample_reference's docstring; u = 2^-53, M = max |x|): B-spline against `restated` 8 u 27 M on every line,
against `exact` the same on lines <= 18 and 27 e M more (e = 4.16e-10) on longer ones; linear 16 u M; nearest and every
inside / outside decision equal.  Integer and float32 outputs equal the cast of the reference except within the bound of a
decision point of the cast, there one unit / one float32 ulp, on at most 1 % of a case (a float32 or integer output on a long
line is held to `restated` alone: the horizon bound is a sixth of a float32 ulp).

Measured worst distance / bound on an MI355X (test_zz_report prints the table and fails above 1):
    family             B-spline / restated   B-spline / exact   linear    nearest, inside / outside
    prefilter float64  0.0405                0.0651             -         -
    prefilter float32  0 (equal)             0 (equal)          -         -
    geometry float64   0.0276                0.0277             0.0943    equal
    geometry float32   0 (equal)             0 (equal)          0         equal
    mirror float64     0.0302                0.0294             -         -
    mirror float32     0 (equal)             0 (equal)          -         -
    unfused            0.0123                0.0123             0.0625    equal
    integer            0 (equal)             0 (equal)          0         -
    dims               0.0202                0.0183             0.0792    equal
    stride             0 (equal)             -                  -         equal
    ties               -                     -                  -         equal
    filters (device)   0.0104                0.000464           -         -
    filters (host)     0.0104                0.000464           -         -
"0 (equal)": every integer and float32 output was the cast of the reference value, no voxel used the one-unit allowance.  The
worst float64 figure, 0.0651 of 8 u 27 M, is 0.52 of u 27 M: the device's rounding IS the float64 rounding of the algorithm
(the host numpy route reaches the same 0.0405 / 0.0651 on the same cases, tests/test_resample_reference.py), pow() included.

The former loose branch: device and host route are bit for bit equal on all of its shapes and types (float32 and the (1, 33, 30)
slab included) and both lie within 0.0104 of the bound, so neither was off; tests/test_gpu_filters.py now asserts equality
there.  An axis of length 1 is never filtered (no pow() runs), and float32 is one rounding of the same float64 value on both
routes: the old comment named causes that do not exist.

No defect was found: every case passed against the kernels as they were.
"""
import numpy as np
import pytest

import resample_reference as rr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not rr.AVAILABLE, reason=rr.SKIP_REASON)]

RATIOS = {}


def _resample(x, start, step, newsize, interp):
    import torch
    from pyradiomics_amd import engine
    out = engine.resample(torch.from_numpy(np.array(x)).cuda(), start, step, newsize, interp)
    assert out.dtype == torch.from_numpy(np.array(x)).dtype and tuple(out.shape) == tuple(newsize)
    return out.cpu().numpy()


def _device(name):
    return _resample(*rr.case(name))


def _run(group, family):
    for name in rr.GROUPS[group]:
        rr.assert_case(name, _device(name), RATIOS, family)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_prefilter_line_lengths(dtype, axis):
    group = "prefilter:%s:axis%d" % (dtype, axis)
    assert {rr.spec(n)["shape"][axis] for n in rr.GROUPS[group]} >= set(rr.PREFILTER_N)
    for name in rr.GROUPS[group]:
        got = _device(name)
        rr.assert_case(name, got, RATIOS, "prefilter:" + dtype)
        if name.startswith("pre-id-"):        # the identity grid reproduces the input: s(k) = x[k] is what `exact` returns
            x = rr.case(name)[0]
            if dtype == "float32":            # either bound is far below half a float32 ulp of a value that IS a float32
                assert np.array_equal(got, x), name
            else:
                assert np.abs(got - x).max() <= rr.bound_for(3, "exact", x.shape, rr.magnitude(x)), name


@pytest.mark.parametrize("interp", ["nearest", "linear", "bspline"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_evaluation_geometry(dtype, interp):
    group = "geometry:%s:%s" % (dtype, interp)
    for name in rr.GROUPS[group]:
        _val, inside = rr.reference(name)
        assert inside.any() and not inside.all(), name                    # both branches of the inside test
    _run(group, "geometry:" + dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mirror_index_more_than_one_period_away(dtype):
    _run("mirror:" + dtype, "mirror:" + dtype)


def test_nearest_ties_round_half_up_in_every_type():
    for name in rr.GROUPS["ties"]:
        got = _device(name)
        val, _inside = rr.reference(name)
        assert np.array_equal(got, rr.cast(val, got.dtype)), name
        rr.assert_case(name, got, RATIOS, "ties")


def test_positions_are_not_fused():
    for name in rr.GROUPS["unfused"]:
        got = _device(name)
        x = rr.case(name)[0]
        if name.startswith("unfused-edge"):
            assert got[-1] != 0, name                                     # 7.5 - 2^-50: inside
        else:
            assert got[-1] == x[1], name                                  # 1.5 - 2^-52: voxel 1, not the tie's voxel 2
        rr.assert_case(name, got, RATIOS, "unfused")


@pytest.mark.parametrize("interp", ["linear", "bspline"])
def test_integer_clamp_and_truncation(interp):
    _run("integer:" + interp, "integer")


@pytest.mark.parametrize("interp", ["nearest", "linear", "bspline"])
def test_one_and_two_dimensions_equal_the_padded_3d_call(interp):
    for name in rr.GROUPS["dims:" + interp]:
        x, start, step, newsize, code = rr.case(name)
        got = _device(name)
        lead = 3 - x.ndim
        got3 = _resample(x.reshape((1,) * lead + x.shape), np.concatenate([np.zeros(lead), start]),
                         np.concatenate([np.ones(lead), step]), (1,) * lead + tuple(newsize), code)
        assert np.array_equal(got3.reshape(got.shape), got), name
        rr.assert_case(name, got, RATIOS, "dims")


def test_grid_stride_loop_of_the_evaluation():
    name = "stride-nearest-int16"
    x, start, step, newsize, _ = rr.case(name)
    assert int(np.prod(newsize)) > rr.RESAMPLE_CAP
    got = _device(name)
    idx = [np.clip(np.floor(start[d] + np.arange(newsize[d]) * step[d] + 0.5).astype(int), 0, x.shape[d] - 1) for d in range(3)]
    assert np.array_equal(got, x[np.ix_(*idx)])                           # every output is inside
    rr.assert_case(name, got, RATIOS, "stride")


def test_grid_stride_loop_of_the_conversion():
    name = "stride-bspline-float32"
    assert rr.case(name)[0].size > rr.TO_F64_CAP
    rr.assert_case(name, _device(name), RATIOS, "stride")


@pytest.mark.parametrize("which,dtype", [(0, np.float32), (1, np.float32), (2, np.float32), (2, np.float64), (2, np.int16)])
def test_shapes_of_the_former_loose_branch(which, dtype, monkeypatch):
    """tests/test_gpu_filters.py compared the device with the host route at rtol 1e-6 / atol 1e-4 on these: here both are held
    to the reference, on the very grid resampleImage computes"""
    import torch
    from pyradiomics_amd import engine, imageoperations
    from pyradiomics_amd.image import Image
    shape, spacing, new, pad = (((9, 40, 37), (0.8, 0.8, 5.0), [2, 2, 2], 5), ((30, 21, 64), (1.0, 1.0, 1.0), [1.5, 0.7, 0], 3),
                                ((1, 33, 30), (0.5, 0.5, 1.0), [1.3, 1.3, 1.3], 4))[which]
    rng = np.random.default_rng(9 + which)
    arr = (rng.standard_normal(shape) * 300 + 500).astype(dtype)
    msk = np.zeros(shape, dtype=np.int16)
    msk[shape[0] // 4: shape[0] // 4 + max(1, shape[0] // 2), 5:-6, 7:-5] = 1
    kw = dict(resampledPixelSpacing=new, interpolator="sitkBSpline", padDistance=pad)
    grids = []
    real = engine.resample

    def spy(image, start, step, newsize, interpolator=3):
        grids.append((np.array(start, dtype=np.float64), np.array(step, dtype=np.float64), tuple(int(n) for n in newsize), interpolator))
        return real(image, start, step, newsize, interpolator)
    monkeypatch.setattr(engine, "resample", spy)
    di, _dm = imageoperations.resampleImage(Image(arr, spacing), Image(msk, spacing), deviceResident=True, **kw)
    hi, _hm = imageoperations.resampleImage(Image(arr, spacing), Image(msk, spacing), **kw)
    assert len(grids) == 2 and grids[0][3] == 3 and grids[1][3] == 0
    start, step, newsize, _ = grids[0]
    kinds = ("restated",) if (dtype != np.float64 and rr.is_long(shape)) else ("restated", "exact")
    tag = "%s-%s" % ("x".join(map(str, shape)), np.dtype(dtype).name)
    print("%s: device == host route bit for bit: %s" % (tag, np.array_equal(di.array, hi.array)))
    for kind in kinds:
        val, inside = rr.resample(arr, start, step, newsize, 3, kind)
        for who, got in (("device", di.array), ("host", hi.array)):
            r = rr.compare(got, arr, val, inside, 3, kind)
            print("%-22s %-6s vs %-8s ratio %.3g  differ %.2g  apart %d" % (tag, who, kind, r["ratio"], r["mismatches"], r["apart"]))
            key = ("filters:" + who, "bspline", kind)
            RATIOS[key] = max(RATIOS.get(key, 0.0), r["ratio"])
            assert rr.passes(r), (tag, who, kind, r)
    assert isinstance(di.device_tensor(), torch.Tensor) and di.on_device


def test_zz_report():
    assert RATIOS, "no comparison ran before the report"
    rr.report("resample limits", RATIOS)

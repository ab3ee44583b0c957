"""The argument checks of the seven batched small-ROI entry points (prad_calculate_batch_dev, prad_batch_glszm_dev,
prad_batch_glszm_fill_dev, prad_batch_firstorder_dev, prad_batch_digitize_dev, prad_batch_features_dev, prad_batch_gather_dev)
that are answered before the device is touched: the return code of every one of them, the words of the message that other
tests and callers look for, and -- with two things wrong at once -- which of the two is reported.  Host buffers stand in for the
device pointers; no case here gets as far as a launch (never add an all-valid call: with a GPU it would run on host memory).
prad_batch_features_dev checks the matrices' pointers and offsets while it fills its record table, after the device has been
selected, so those two errors are not pinned here."""
import ctypes as C

import numpy as np
import pytest

IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
OK, ARG, UNSUPPORTED = 1, -1, -4
TWO = [(2, 3, 4), (1, 1, 5)]                 # two valid boxes
ZERO = [(2, 3, 4), (1, 0, 5)]                # a zero extent in the second
BIG = (2048, 2048, 512)                      # 2^31 voxels: above what the first-order launches index


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


def _ip(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.intc).ctypes.data_as(IP)


def _lp(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(LP)


_BUF = np.zeros(4096, dtype=np.float64)      # stands in for every device pointer


def _vp(null, name):
    return None if name in null else C.c_void_p(_BUF.ctypes.data)


def _check(got, want):
    from pyradiomics_amd import _lib
    code, text = want if isinstance(want, tuple) else (want, None)
    assert got == code, (got, _lib.last_error())
    if text is not None:
        assert text in _lib.last_error(), _lib.last_error()
    assert (_BUF == 0).all(), "a buffer was written"


def _matrices(lib, sizes=TWO, B=2, Ng=8, off=(0, 24), families=15, distances=(1,), alpha=0, null=()):
    sz = np.ascontiguousarray(sizes, dtype=np.intc)
    dist = np.ascontiguousarray(distances, dtype=np.intc)
    return lib.prad_calculate_batch_dev(_vp(null, "levels"), _vp(null, "mask"), None if "sizes" in null else _ip(sz),
                                        None if "off" in null else _lp(off), B, Ng, families,
                                        None if "distances" in null else _ip(dist), len(dist), alpha, _vp(null, "glcm"),
                                        _vp(null, "glrlm"), _vp(null, "gldm"), _vp(null, "ngtdm"), _vp(null, "status"), None)


def test_texture_matrices(lib):
    cap = lib.prad_batch_max_vox()
    above = [(2, 3, 4), (1, 1, cap + 1)]
    _check(_matrices(lib, B=-1), (ARG, "B=-1"))
    _check(_matrices(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_matrices(lib, sizes=ZERO), (ARG, "ROI 1"))
    _check(_matrices(lib, off=(0, -24)), (ARG, "off[1]"))
    for name in ("levels", "mask", "off", "status"):
        _check(_matrices(lib, null=(name,)), (ARG, "NULL pointer"))
    for f, name in enumerate(("glcm", "glrlm", "gldm", "ngtdm")):
        _check(_matrices(lib, null=(name,)), (ARG, "output %d is NULL" % f))
    _check(_matrices(lib, null=("distances",)), (ARG, "no distances"))
    _check(_matrices(lib, families=0), (ARG, "families=0"))
    _check(_matrices(lib, families=16), (ARG, "families=16"))
    _check(_matrices(lib, distances=(1, 0)), (ARG, "distance 0"))
    _check(_matrices(lib, alpha=-1), (ARG, "alpha=-1"))
    _check(_matrices(lib, Ng=0), (ARG, "Ng=0"))
    _check(_matrices(lib, Ng=65), (UNSUPPORTED, "Ng=65"))
    _check(_matrices(lib, sizes=above), (UNSUPPORTED, "ROI 1 holds %d voxels" % (cap + 1)))
    _check(_matrices(lib, sizes=[(1, 1, cap)], B=1, off=(-1,)), (ARG, "off[0]"))       # the cap itself is inside
    _check(_matrices(lib, B=0), OK)
    # two things wrong: the domain is looked at before the pointers and the offsets, after the sizes
    _check(_matrices(lib, Ng=65, null=("levels",)), (UNSUPPORTED, "Ng=65"))
    _check(_matrices(lib, sizes=above, off=(0, -24)), (UNSUPPORTED, "ROI 1"))
    _check(_matrices(lib, Ng=65, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    _check(_matrices(lib, Ng=0, sizes=ZERO), (ARG, "Ng=0"))
    _check(_matrices(lib, B=-1, Ng=0), (ARG, "B=-1"))
    _check(_matrices(lib, null=("glcm", "levels")), (ARG, "output 0 is NULL"))
    _check(_matrices(lib, alpha=-1, off=(-1, 24)), (ARG, "alpha=-1"))


def _label(lib, sizes=TWO, B=2, Ng=8, off=(0, 24), null=()):
    sz = np.ascontiguousarray(sizes, dtype=np.intc)
    return lib.prad_batch_glszm_dev(_vp(null, "levels"), _vp(null, "mask"), None if "sizes" in null else _ip(sz),
                                    None if "off" in null else _lp(off), B, Ng, _vp(null, "zones"), _vp(null, "summary"),
                                    _vp(null, "status"), None)


def test_glszm_labelling(lib):
    cap = lib.prad_batch_glszm_max_vox()
    above = [(2, 3, 4), (1, 1, cap + 1)]
    _check(_label(lib, B=-1), (ARG, "B=-1"))
    _check(_label(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_label(lib, sizes=ZERO), (ARG, "ROI 1"))
    _check(_label(lib, off=(0, -24)), (ARG, "off[1]"))
    for name in ("levels", "mask", "off", "zones", "summary", "status"):
        _check(_label(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_label(lib, Ng=0), (ARG, "Ng=0"))
    _check(_label(lib, Ng=65), (UNSUPPORTED, "Ng=65"))
    _check(_label(lib, sizes=above), (UNSUPPORTED, "ROI 1 holds %d voxels" % (cap + 1)))
    _check(_label(lib, sizes=[(1, 1, cap)], B=1, off=(-1,)), (ARG, "off[0]"))          # the cap itself is inside
    _check(_label(lib, B=0), OK)
    # two things wrong: here the pointers and the offsets are looked at before the domain
    _check(_label(lib, Ng=65, null=("levels",)), (ARG, "NULL pointer"))
    _check(_label(lib, sizes=above, off=(0, -24)), (ARG, "off[1]"))
    _check(_label(lib, Ng=65, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    _check(_label(lib, Ng=0, sizes=ZERO), (ARG, "Ng=0"))
    _check(_label(lib, B=-1, Ng=0), (ARG, "B=-1"))
    _check(_label(lib, Ng=65, sizes=above), (UNSUPPORTED, "Ng=65"))


def _fill(lib, summary=((2, 3, 2), (1, 1, 1)), B=2, Ng=8, compact=1, off=(0, 24), out_off=(0, 16), sizes_off=(0, 2), null=()):
    return lib.prad_batch_glszm_fill_dev(_vp(null, "zones"), None if "summary" in null else _ip(summary),
                                         None if "off" in null else _lp(off), B, Ng, compact, _vp(null, "out"),
                                         None if "out_off" in null else _lp(out_off), _vp(null, "sizes_out"),
                                         None if "sizes_off" in null else _lp(sizes_off), None)


def test_glszm_fill(lib):
    cap = lib.prad_batch_glszm_max_vox()
    _check(_fill(lib, B=-1), (ARG, "B=-1"))
    for name in ("zones", "summary", "off", "out", "out_off", "sizes_out", "sizes_off"):
        _check(_fill(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_fill(lib, off=(0, -24)), (ARG, "negative offset of ROI 1"))
    _check(_fill(lib, out_off=(0, -16)), (ARG, "negative offset of ROI 1"))
    _check(_fill(lib, sizes_off=(0, -2)), (ARG, "negative offset of ROI 1"))
    _check(_fill(lib, summary=((2, 3, 2), (1, cap + 1, 1))), (ARG, "summary of ROI 1"))       # a zone above the cap
    _check(_fill(lib, summary=((2, 3, 2), (1, 1, 2))), (ARG, "summary of ROI 1"))
    _check(_fill(lib, Ng=0), (ARG, "Ng=0"))
    _check(_fill(lib, Ng=65), (UNSUPPORTED, "Ng=65"))
    _check(_fill(lib, B=0), OK)
    # two things wrong: the domain is looked at last
    _check(_fill(lib, Ng=65, off=(0, -24)), (ARG, "negative offset of ROI 1"))
    _check(_fill(lib, Ng=65, null=("out",)), (ARG, "NULL pointer"))
    _check(_fill(lib, B=-1, Ng=0), (ARG, "B=-1"))
    _check(_fill(lib, Ng=0, null=("zones",)), (ARG, "Ng=0"))


def _firstorder(lib, sizes=TWO, B=2, dtype=0, off=(0, 24), null=()):
    sz = np.ascontiguousarray(sizes, dtype=np.intc)
    return lib.prad_batch_firstorder_dev(_vp(null, "image"), dtype, _vp(null, "mask"), None if "sizes" in null else _ip(sz),
                                         None if "off" in null else _lp(off), B, 0.0, _vp(null, "table"), None)


def test_firstorder(lib):
    above = [(2, 3, 4), BIG]
    _check(_firstorder(lib, B=0), (ARG, "B=0"))
    _check(_firstorder(lib, B=-1), (ARG, "B=-1"))
    _check(_firstorder(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_firstorder(lib, sizes=ZERO), (ARG, "ROI 1"))
    _check(_firstorder(lib, off=(0, -24)), (ARG, "off[1]"))
    for name in ("image", "mask", "off", "table"):
        _check(_firstorder(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_firstorder(lib, dtype=4), (ARG, "dtype 4"))
    _check(_firstorder(lib, dtype=-1), (ARG, "dtype -1"))
    _check(_firstorder(lib, sizes=above), (UNSUPPORTED, "ROI 1 holds 2147483648 voxels"))
    # two things wrong: the pointers and the offsets are looked at before the domain, the dtype before everything
    _check(_firstorder(lib, sizes=above, null=("image",)), (ARG, "NULL pointer"))
    _check(_firstorder(lib, sizes=above, off=(0, -24)), (ARG, "off[1]"))
    _check(_firstorder(lib, dtype=7, B=0), (ARG, "dtype 7"))
    _check(_firstorder(lib, sizes=[BIG, (1, 0, 5)]), (ARG, "ROI 1 has size[1]=0"))
    _check(_firstorder(lib, null=("table",), off=(-1, 24)), (ARG, "NULL pointer"))


def _digitize(lib, sizes=TWO, B=2, dtype=0, off=(0, 24), edge_off=(0, 3, 6), count_off=(0, 4), null=()):
    sz = np.ascontiguousarray(sizes, dtype=np.intc)
    return lib.prad_batch_digitize_dev(_vp(null, "image"), dtype, _vp(null, "mask"), None if "sizes" in null else _ip(sz),
                                       None if "off" in null else _lp(off), B, _vp(null, "edges"),
                                       None if "edge_off" in null else _lp(edge_off), _vp(null, "levels"), _vp(null, "counts"),
                                       None if "count_off" in null else _lp(count_off), _vp(null, "top"), None)


def test_digitize(lib):
    cap = lib.prad_batch_digitize_max_edges()
    many = (0, 3, 3 + cap + 1)
    _check(_digitize(lib, B=0), (ARG, "B=0"))
    _check(_digitize(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_digitize(lib, sizes=ZERO), (ARG, "ROI 1"))
    _check(_digitize(lib, off=(0, -24)), (ARG, "bad offsets of ROI 1"))
    _check(_digitize(lib, edge_off=(0, 3, 2)), (ARG, "bad offsets of ROI 1"))
    _check(_digitize(lib, edge_off=(-1, 3, 6)), (ARG, "bad offsets of ROI 0"))
    for name in ("image", "mask", "off", "edge_off", "levels", "counts", "count_off", "top"):
        _check(_digitize(lib, null=(name,)), (ARG, "NULL pointer"))
    _check(_digitize(lib, null=("edges",)), (ARG, "NULL edges"))
    _check(_digitize(lib, dtype=4), (ARG, "dtype 4"))
    _check(_digitize(lib, edge_off=many), (UNSUPPORTED, "ROI 1 has %d edges" % (cap + 1)))
    _check(_digitize(lib, sizes=[(2, 3, 4), BIG]), (UNSUPPORTED, "ROI 1 holds 2147483648 voxels"))
    _check(_digitize(lib, count_off=(-1, -1)), OK)                    # no ROI asks for the launch: nothing to do
    _check(_digitize(lib, count_off=(-1, -1), edge_off=many), OK)     # (nor are its edges counted)
    # two things wrong: an argument error wins over the domain
    _check(_digitize(lib, edge_off=many, null=("edges",)), (ARG, "NULL edges"))
    _check(_digitize(lib, edge_off=(0, cap + 1, cap + 4), off=(0, -24)), (ARG, "bad offsets of ROI 1"))
    _check(_digitize(lib, sizes=[(2, 3, 4), BIG], null=("top",)), (ARG, "NULL pointer"))
    _check(_digitize(lib, dtype=7, B=0), (ARG, "dtype 7"))
    _check(_digitize(lib, sizes=[(2, 3, 4), BIG], edge_off=many), (UNSUPPORTED, "holds 2147483648 voxels"))


def _features(lib, sizes=TWO, B=2, Ng=8, families=31, Na=((13, 4), (13, 4)), cols=(3, 1), null=()):
    sz = np.ascontiguousarray(sizes, dtype=np.intc)
    zero = np.zeros(5 * (max(B, 0) + 1), dtype=np.int64)
    return lib.prad_batch_features_dev(None if "sizes" in null else _ip(sz), B, Ng, families, None if "Na" in null else _ip(Na),
                                       None if "cols" in null else _ip(cols), _vp(null, "glcm"), _vp(null, "glrlm"),
                                       _vp(null, "gldm"), _vp(null, "ngtdm"), None if "offsets" in null else _lp(zero),
                                       _vp(null, "glszm"), None if "glszm_offsets" in null else _lp(zero),
                                       _vp(null, "glszm_sizes"), None if "glszm_sizes_offsets" in null else _lp(zero), 1, 1,
                                       _vp(null, "out"), _vp(null, "empty"), None)


def test_features(lib):
    _check(_features(lib, B=-1), (ARG, "B=-1"))
    _check(_features(lib, null=("sizes",)), (ARG, "sizes="))
    _check(_features(lib, null=("Na",)), (ARG, "Na="))
    _check(_features(lib, sizes=ZERO), (ARG, "ROI 1"))
    _check(_features(lib, Na=((13, 4), (13, -1))), (ARG, "negative angle count of ROI 1"))
    _check(_features(lib, null=("cols",)), (ARG, "GLSZM without its column counts"))
    _check(_features(lib, families=0), (ARG, "families=0"))
    _check(_features(lib, families=32), (ARG, "families=32"))
    for name, text in (("out", "NULL output"), ("empty", "NULL output"), ("offsets", "NULL offsets"),
                       ("glszm_offsets", "NULL GLSZM offsets"), ("glszm_sizes_offsets", "size lists without their offsets")):
        _check(_features(lib, null=(name,)), (ARG, text))
    _check(_features(lib, Ng=0), (ARG, "Ng=0"))
    _check(_features(lib, Ng=65), (UNSUPPORTED, "Ng=65"))
    _check(_features(lib, B=0), OK)
    _check(_features(lib, families=16, cols=(0, 0)), OK)              # no record to evaluate: nothing to do
    # two things wrong: the domain is looked at after the layout's arguments, before the pointers
    _check(_features(lib, Ng=65, null=("out",)), (UNSUPPORTED, "Ng=65"))
    _check(_features(lib, Ng=65, sizes=ZERO), (ARG, "ROI 1 has size[1]=0"))
    _check(_features(lib, B=-1, Ng=0), (ARG, "B=-1"))
    _check(_features(lib, Ng=0, sizes=ZERO), (ARG, "Ng=0"))
    _check(_features(lib, null=("out", "offsets")), (ARG, "NULL output"))


def _gather(lib, size=(4, 5, 6), B=2, lo=((0, 0, 0), (1, 1, 1)), box=((2, 3, 4), (1, 1, 5)), offsets=(0, 24), image_dtype=0,
            label_dtype=2, null=()):
    return lib.prad_batch_gather_dev(_vp(null, "image"), image_dtype, _vp(null, "labelmap"), label_dtype,
                                     None if "size" in null else _ip(size), B, None if "labels" in null else _ip((1, 2)),
                                     None if "lo" in null else _ip(lo), None if "box" in null else _ip(box),
                                     None if "offsets" in null else _lp(offsets), _vp(null, "out_image"), _vp(null, "out_mask"),
                                     None)


def test_gather(lib):
    _check(_gather(lib, B=0), (ARG, "B=0"))
    _check(_gather(lib, B=-1), (ARG, "B=-1"))
    for name in ("size", "lo", "box", "offsets", "labels"):
        _check(_gather(lib, null=(name,)), (ARG, "NULL table"))
    for name in ("image", "out_image", "labelmap", "out_mask"):
        _check(_gather(lib, null=(name,)), (ARG, "an input without its output"))
    _check(_gather(lib, null=("image", "out_image", "labelmap", "out_mask")), (ARG, "neither image nor label map"))
    _check(_gather(lib, image_dtype=4), (ARG, "image dtype code 4"))
    _check(_gather(lib, label_dtype=0), (ARG, "label dtype code 0"))
    _check(_gather(lib, size=(4, 0, 6)), (ARG, "size[1]=0"))
    _check(_gather(lib, box=((2, 3, 4), (1, 0, 5))), (ARG, "ROI 1 has extent[1]=0"))
    _check(_gather(lib, box=((2, 3, 4), (1, 1, 6))), (ARG, "ROI 1 leaves the volume along axis 2"))
    _check(_gather(lib, lo=((0, 0, 0), (1, -1, 1))), (ARG, "ROI 1 leaves the volume along axis 1"))
    _check(_gather(lib, offsets=(-1, 24)), (ARG, "offsets[0]=-1"))
    _check(_gather(lib, offsets=(0, 23)), (ARG, "offsets[1]=23"))
    # two things wrong: dtype codes before the tables, the tables before B, ROI by ROI after that
    _check(_gather(lib, image_dtype=4, B=0), (ARG, "image dtype code 4"))
    _check(_gather(lib, B=0, null=("lo",)), (ARG, "NULL table"))
    _check(_gather(lib, B=0, size=(4, 0, 6)), (ARG, "B=0"))
    _check(_gather(lib, box=((2, 3, 7), (1, 0, 5)), offsets=(-1, 24)), (ARG, "ROI 0 leaves the volume"))

"""The route planner of a segment-mode GLSZM call (csrc/prad_glszm_plan.h) through prad_debug_glszm_route, against a restatement
of its rules written from their wording, not from the C++.  Host only: no device call is made.

The rules.  The volume is embedded in 3-D (leading extents 1).  An offset is backward when its linear index in the embedded volume
is negative.
    tiled   Nd <= 3, Na <= 64, every offset component in {-1, 0, 1}, at most 32 backward offsets
    mode    1 with 13 backward offsets; 2 with 4 backward offsets that all have dz == 0; otherwise 0
    dense   tiled, mode != 0, 1 <= Ng <= 255
    routes  dense 26 / dense 8; int32 tiles with the full-26, full-8 or offset-table border kernel; label volume
    retry   an irregular level found by the pack reruns a dense call as the int32 tiles of the same mode
A table of more than 32 backward UNIT offsets cannot occur in three dimensions (there are 13 distinct ones, and more than 64
angles already leave the tiled routes), so that clause of `tiled` is not driven here.

Angle sets are the real ones of prad_get_angle_count / prad_build_angles (bidirectional, distance 1) unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

DENSE26, DENSE8, TILES26, TILES8, TILES_OFFSETS, LABEL_VOLUME = range(6)
NAMES = ["dense26", "dense8", "tiles-full26", "tiles-full8", "tiles-offsets", "label-volume"]
TZ, TY, TX = 8, 8, 64


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def real_angles(lib, size, f2d=-1):
    size = np.array(size, dtype=np.intc)
    one = np.array([1], dtype=np.intc)
    Na = lib.prad_get_angle_count(_ip(size), _ip(one), len(size), 1, 1, f2d)
    angles = np.zeros((max(Na, 1), len(size)), dtype=np.intc)
    if Na:
        assert lib.prad_build_angles(_ip(size), _ip(one), len(size), 1, f2d, Na, _ip(angles)) == 0
    return angles[:Na]


def route(lib, size, angles, Ng, irregular=0, cap=128):
    size = np.array(size, dtype=np.intc)
    angles = np.ascontiguousarray(angles, dtype=np.intc)
    out = np.zeros(cap, dtype=np.intc)
    n = lib.prad_debug_glszm_route(_ip(size), len(size), _ip(angles), len(angles), Ng, irregular, _ip(out), cap)
    if n <= 0:
        return n
    r = out[:n].tolist()
    assert n == 7 + 3 * r[6]
    return {"route": r[0], "mode": r[1], "dims": tuple(r[2:5]), "tiles": r[5], "back": [tuple(r[7 + 3 * a:10 + 3 * a]) for a in range(r[6])]}


def expected(size, angles, Ng, irregular=0):
    """the rules of the module docstring"""
    Nd, Na = len(size), len(angles)
    if Nd > 3 or Na > 64 or any(abs(int(c)) > 1 for a in angles for c in a):
        return {"route": LABEL_VOLUME, "mode": 0, "tiles": 0, "back": []}
    dims = (1,) * (3 - Nd) + tuple(size)
    emb = [(0,) * (3 - Nd) + tuple(int(c) for c in a) for a in angles]
    back = [o for o in emb if (o[0] * dims[1] + o[1]) * dims[2] + o[2] < 0]
    assert len(back) <= 32
    mode = 1 if len(back) == 13 else 2 if len(back) == 4 and all(o[0] == 0 for o in back) else 0
    dense = mode != 0 and 1 <= Ng <= 255 and not irregular
    r = {1: DENSE26 if dense else TILES26, 2: DENSE8 if dense else TILES8, 0: TILES_OFFSETS}[mode]
    tiles = -(-dims[0] // TZ) * -(-dims[1] // TY) * -(-dims[2] // TX)
    return {"route": r, "mode": mode, "dims": dims, "tiles": tiles, "back": back}


def agree(lib, size, angles, Ng, irregular=0):
    got, want = route(lib, size, angles, Ng, irregular), expected(size, angles, Ng, irregular)
    assert isinstance(got, dict), got
    for k, v in want.items():
        assert got[k] == v, (k, got, want)
    return got


# (size, force2Ddimension) -> route at Ng = 32, backward offsets
REAL = [
    ((3, 3, 3), -1, DENSE26, 13),
    ((17, 9, 130), -1, DENSE26, 13),
    ((1, 3, 3), -1, DENSE8, 4),
    ((3, 3), -1, DENSE8, 4),
    ((3, 3, 3), 0, DENSE8, 4),
    ((3, 1, 3), -1, TILES_OFFSETS, 4),
    ((3, 3, 1), -1, TILES_OFFSETS, 4),
    ((3, 3, 3), 1, TILES_OFFSETS, 4),
    ((3, 3, 3), 2, TILES_OFFSETS, 4),
    ((5,), -1, TILES_OFFSETS, 1),
]


@pytest.mark.parametrize("size,f2d,want,nback", REAL, ids=["%s-f2d%d" % ("x".join(map(str, s)), f) for s, f, _, _ in REAL])
def test_real_angle_sets(lib, size, f2d, want, nback):
    angles = real_angles(lib, size, f2d)
    got = agree(lib, size, angles, 32)
    assert got["route"] == want and len(got["back"]) == nback, (NAMES[got["route"]], got)
    # an irregular level found by the pack: the int32 tiles of the same mode; the other routes have no pack and no retry
    again = agree(lib, size, angles, 32, irregular=1)
    assert again["route"] == {DENSE26: TILES26, DENSE8: TILES8}.get(want, want)
    assert (again["mode"], again["tiles"], again["back"]) == (got["mode"], got["tiles"], got["back"])


@pytest.mark.parametrize("size,f2d,dense,int32", [((3, 3, 3), -1, DENSE26, TILES26), ((1, 3, 3), -1, DENSE8, TILES8),
                                                  ((3, 3), -1, DENSE8, TILES8), ((3, 3, 3), 0, DENSE8, TILES8)])
def test_level_count_at_the_byte_limit(lib, size, f2d, dense, int32):
    angles = real_angles(lib, size, f2d)
    for Ng in (1, 254, 255):
        assert agree(lib, size, angles, Ng)["route"] == dense
    for Ng in (256, 300, 65536):
        got = agree(lib, size, angles, Ng)
        assert got["route"] == int32 and got["mode"] == (1 if int32 == TILES26 else 2)


def test_tile_counts(lib):
    for size, tiles in (((8, 8, 64), 1), ((9, 8, 64), 2), ((8, 9, 64), 2), ((8, 8, 65), 2), ((24, 33, 196), 3 * 5 * 4),
                        ((256, 256, 256), 32 * 32 * 4), ((64, 64), 8), ((130,), 3)):
        assert agree(lib, size, real_angles(lib, size), 32)["tiles"] == tiles


def test_label_volume(lib):
    size = (2, 3, 3, 3)                                                  # 4-D: 80 neighbours
    got = agree(lib, size, real_angles(lib, size), 32)
    assert got["route"] == LABEL_VOLUME and got["tiles"] == 0 and got["back"] == []
    full = real_angles(lib, (3, 3, 3))
    far = full.copy()
    far[5, 2] = 2                                                        # a component of 2
    assert agree(lib, (5, 5, 5), far, 32)["route"] == LABEL_VOLUME
    fwd = np.array([a for a in full.tolist() if (a[0] * 5 + a[1]) * 5 + a[2] > 0], dtype=np.intc)
    many = np.concatenate([full, full, fwd])                             # 65 angles, all of them unit offsets, 26 backward
    assert len(many) == 65 and agree(lib, (5, 5, 5), many, 32)["route"] == LABEL_VOLUME
    assert agree(lib, (5, 5, 5), many[:64], 32)["route"] == TILES_OFFSETS      # 64 angles: tiled, but no full neighbourhood
    assert agree(lib, (5, 5, 5), far, 32, irregular=1)["route"] == LABEL_VOLUME


def test_partial_neighbourhoods_take_the_offset_table(lib):
    full = real_angles(lib, (3, 3, 3))
    back = [a for a in full.tolist() if (a[0] * 5 + a[1]) * 5 + a[2] < 0]
    assert len(back) == 13
    got = agree(lib, (5, 5, 5), np.array(back[:12], dtype=np.intc), 32)      # twelve of the thirteen
    assert got["route"] == TILES_OFFSETS and got["mode"] == 0
    four = [a for a in back if a[1] == 0][:4]                                # four backward offsets, not all in the plane
    assert len(four) == 4 and any(a[0] for a in four)
    assert agree(lib, (5, 5, 5), np.array(four, dtype=np.intc), 32)["route"] == TILES_OFFSETS
    forward = [[-a[0], -a[1], -a[2]] for a in back]                           # forward offsets only: nothing backward
    got = agree(lib, (5, 5, 5), np.array(forward, dtype=np.intc), 32)
    assert got["route"] == TILES_OFFSETS and got["back"] == []


def test_arguments_no_call_accepts(lib):
    """(1, 1, 1) has no angle: prad_calculate_glszm_dev answers Na < 1 with its argument error, the planner with 0"""
    assert len(real_angles(lib, (1, 1, 1))) == 0
    one = np.zeros((1, 3), dtype=np.intc)
    size = np.array([1, 1, 1], dtype=np.intc)
    out = np.zeros(16, dtype=np.intc)
    assert lib.prad_debug_glszm_route(_ip(size), 3, _ip(one), 0, 32, 0, _ip(out), 16) == 0
    assert lib.prad_debug_glszm_route(_ip(size), 3, _ip(one), 1, 0, 0, _ip(out), 16) == 0      # Ng < 1
    assert lib.prad_debug_glszm_route(_ip(size), 0, _ip(one), 1, 32, 0, _ip(out), 16) == 0     # Nd < 1
    assert lib.prad_debug_glszm_route(None, 3, _ip(one), 1, 32, 0, _ip(out), 16) == 0
    full = real_angles(lib, (3, 3, 3))
    assert route(lib, (3, 3, 3), full, 32, cap=8) == -(7 + 3 * 13)            # too small a buffer: the count it needs

"""The planner of the pairs tier of a GLDM / NGTDM call (csrc/prad_neigh_plan.h, executed by pairs_neigh in prad_api.hip) through
prad_debug_neigh_plan.  Host only: no device call is made.  The oracle for the route label is
tests/neigh_reference.expected_route, written from the documented limits and used as it is; the launch geometry is held to the
u32 overflow rule of the bins by arithmetic on the record alone.

expected_route names the FIRST tier that takes a synchronous call; the byte tier in front of this one is not planned here.  So a
case is held to the oracle where the oracle names this tier ("pairs-..."): the plan applies, with that variant; and where it says
"generic": the plan does not apply.  Where the byte tier answers, nothing is asserted about the tier behind it.

Angle lists are the real ones of prad_get_angle_count / prad_build_angles (bidirectional) unless a case builds its own.

Two caps of the documented limits cannot be reached and have no boundary pair: a box needs cube <= 4096 and the tier Ng <= 65535,
which keeps cube * Ng below 2^28 (the cap was 2^40); narrow box words need cube <= 127, which keeps cube * Ng below 2^23 (the cap
was 2^24).  The planner says so where it leaves the two comparisons out; the largest products the other limits admit are driven."""
import ctypes as C
import itertools

import numpy as np
import pytest

import neigh_reference as nr

VARIANTS = ["none"] + ["pairs-%s%s" % (place, word) for place in ("global", "lds64", "lds32") for word in ("", "+box32", "+box64")]
FIELDS = "applies variant box narrow mode lds threads grid box_grid Nz Ny Nx rz ry rx".split()
CUS = 256


@pytest.fixture(scope="module")
def lib():
    from pyradiomics_amd import _build, _lib
    _build.build()          # no-op when the in-tree .so is current
    return _lib.load()


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


_ANGLES = {}


def real_angles(lib, shape, distances=(1,), f2d=-1):
    key = (tuple(shape), tuple(distances), f2d)
    if key not in _ANGLES:
        size, dist = np.array(shape, dtype=np.intc), np.array(distances, dtype=np.intc)
        Na = lib.prad_get_angle_count(_ip(size), _ip(dist), len(size), len(dist), 1, f2d)
        angles = np.zeros((max(Na, 1), len(size)), dtype=np.intc)
        assert Na > 0 and lib.prad_build_angles(_ip(size), _ip(dist), len(size), len(dist), f2d, Na, _ip(angles)) == 0
        _ANGLES[key] = angles[:Na]
    return _ANGLES[key]


def box_angles(radii):
    """every non-zero offset of the box with these radii, one per row"""
    offs = [o for o in itertools.product(*[range(-r, r + 1) for r in radii]) if any(o)]
    return np.array(offs, dtype=np.intc)


def plan(lib, family, shape, angles, Ng, no_pairs=False, no_box=False, cus=CUS, cap=64):
    size = np.array(shape, dtype=np.intc)
    angles = np.ascontiguousarray(angles, dtype=np.intc)
    out = np.zeros(cap, dtype=np.intc)
    n = lib.prad_debug_neigh_plan(_ip(size), len(size), _ip(angles), len(angles), Ng, int(family == "ngtdm"),
                                  int(no_pairs) | int(no_box) << 1, cus, _ip(out), cap)
    if n <= 0:
        return n
    assert n == len(FIELDS)
    p = dict(zip(FIELDS, out[:n].tolist()))
    assert (p["variant"] >= 1) == bool(p["applies"]) and (p["box"] or not p["narrow"]), p
    if not p["applies"]:
        assert p["grid"] == p["threads"] == p["lds"] == p["box"] == 0, p
    return p


def label(p):
    return VARIANTS[p["variant"]]


def agree(lib, family, shape, angles, Ng, alpha=0, no_box=False, no_pairs=False):
    """-> (plan, the oracle's label); asserts what the module docstring says"""
    p = plan(lib, family, shape, angles, Ng, no_pairs, no_box)
    want = nr.expected_route(family, tuple(shape), Ng, np.asarray(angles, dtype=np.int64), alpha, no_box, no_pairs)
    if want.startswith("pairs-"):
        assert label(p) == want, (family, shape, Ng, len(angles), no_box, no_pairs, label(p), want, p)
    elif want == "generic":
        assert not p["applies"], (family, shape, Ng, len(angles), no_box, no_pairs, p)
    else:
        assert want.startswith("neigh"), want
    return p, want


# ---- 1. every case of the catalogue -----------------------------------------------------------------------------------------
NEIGH_GROUPS = sorted(g for g, names in nr.GROUPS.items() if nr.spec(names[0])["family"] in ("gldm", "ngtdm"))


def test_the_catalogue_holds_the_pairs_limit_groups():
    """the GLDM / NGTDM groups of tests/test_gpu_pairs_limits.py are groups of the case table"""
    assert {"pairs-levels", "pairs-nobox", "pairs-box", "pairs-off", "route-edges", "big", "force2d"} <= set(NEIGH_GROUPS)
    assert sum(len(nr.GROUPS[g]) for g in NEIGH_GROUPS) == sum(nr.spec(n)["family"] in ("gldm", "ngtdm") for n in nr.NAMES)


@pytest.mark.parametrize("group", NEIGH_GROUPS)
def test_every_case_of_the_catalogue(lib, group):
    held = 0
    for name in nr.GROUPS[group]:
        s = nr.spec(name)
        angles = real_angles(lib, s["shape"], s["distances"], s["dim"] if s["force2D"] else -1)
        held += not agree(lib, s["family"], s["shape"], angles, s["Ng"], s["alpha"], s["no_box"], s["no_pairs"])[1].startswith("neigh")
    if group.startswith("pairs-"):          # the groups that exist for this tier: (nearly) every case names it or the exact kernels
        assert held >= len(nr.GROUPS[group]) - 8, (group, held)


# ---- 2. one case on each side of every limit of the tier ------------------------------------------------------------------
Q = (7, 6, 12)


def _first(lib, family, shape, angles, Ng, **kw):
    p, want = agree(lib, family, shape, angles, Ng, **kw)
    assert not want.startswith("neigh"), (want, "the case is meant for this tier")
    return label(p) if p["applies"] else "generic"


def test_levels_and_bins_where_the_byte_tier_ends(lib):
    a1, a12, a2 = real_angles(lib, Q), real_angles(lib, Q, (1, 2)), real_angles(lib, Q, (2,))
    assert (len(a1), len(a12), len(a2)) == (26, 124, 98)
    assert _first(lib, "gldm", Q, a1, 256) == "pairs-lds32" and _first(lib, "ngtdm", Q, a1, 256) == "pairs-lds64+box32"
    assert _first(lib, "gldm", Q, a12, 132) == "pairs-lds32" and _first(lib, "gldm", Q, a2, 166) == "pairs-lds32"
    assert _first(lib, "ngtdm", Q, a2, 83) == "pairs-lds64"
    for fam, a, Ng in (("gldm", a1, 255), ("gldm", a12, 131), ("gldm", a2, 165), ("ngtdm", a2, 82)):      # the byte tier's side
        assert agree(lib, fam, Q, a, Ng)[1].startswith("neigh")


def test_angle_table_of_128(lib):
    many = real_angles(lib, (9, 9, 12), (1, 2, 3))
    assert len(many) == 342
    for fam in ("gldm", "ngtdm"):
        assert _first(lib, fam, (9, 9, 12), many[:128], 300).startswith("pairs-") and _first(lib, fam, (9, 9, 12), many[:129], 300) == "generic"
        assert _first(lib, fam, (9, 9, 12), many[:129], 32) == "generic"
    assert _first(lib, "ngtdm", (9, 9, 12), many, 300) == "pairs-global+box64"          # a whole box needs no table
    assert _first(lib, "ngtdm", (9, 9, 12), many, 300, no_box=True) == "generic"
    far = real_angles(lib, Q).copy()
    far[3, 2] = 128                                                                     # an offset no signed char holds
    assert not plan(lib, "gldm", (7, 6, 300), far, 300)["applies"]
    far[3, 2] = 127
    assert plan(lib, "gldm", (7, 6, 300), far, 300)["applies"]


def test_box_cube_and_word(lib):
    shape = (100, 100)
    for radii, cube in (((31, 31), 3969), ((31, 32), 4095)):
        p, _ = agree(lib, "ngtdm", shape, box_angles(radii), 300)
        assert label(p) == "pairs-global+box64" and (p["ry"], p["rx"]) == radii and len(box_angles(radii)) == cube - 1
    p, want = agree(lib, "ngtdm", shape, box_angles((32, 32)), 300)                      # cube 4225
    assert want == "generic" and not p["applies"]
    p, _ = agree(lib, "ngtdm", shape, box_angles((31, 32)), 32768)                       # the largest cube * Ng within 1 GiB of bins
    assert p["box"] and not p["narrow"]
    assert not plan(lib, "ngtdm", shape, box_angles((31, 32)), 32777)["applies"]         # 4095 x 32777 x 8 bytes > 1 GiB
    hole = box_angles((5, 5))
    hole[7] = hole[8]                                                                    # cube - 1 offsets, but not the whole cube
    p = plan(lib, "ngtdm", shape, hole, 100)
    assert p["applies"] and not p["box"] and label(p) == "pairs-lds64"
    # 32-bit box words up to a cube of 127
    assert _first(lib, "ngtdm", shape, box_angles((5, 5)), 100) == "pairs-lds64+box32"   # 121
    assert _first(lib, "ngtdm", shape, box_angles((5, 6)), 100) == "pairs-lds64+box64"   # 143
    p, _ = agree(lib, "ngtdm", (8, 12, 16), real_angles(lib, (8, 12, 16), (1, 2)), 65535)   # 125 x 65535: the largest narrow product
    assert label(p) == "pairs-global+box32" and p["narrow"]


def test_levels_of_the_pairs_tier(lib):
    P = (8, 12, 16)
    a = real_angles(lib, P)
    assert _first(lib, "gldm", P, a, 65535) == "pairs-global" and _first(lib, "gldm", P, a, 65536) == "generic"
    assert _first(lib, "ngtdm", P, a, 65535) == "pairs-global+box32" and _first(lib, "ngtdm", P, a, 65536) == "generic"
    assert _first(lib, "gldm", P, a, 300, no_pairs=True) == "generic"


def test_bin_placement_at_150_kb(lib):
    P = (8, 12, 16)
    a = real_angles(lib, P)
    for Ng, mode, lds in ((711, 1, 711 * 27 * 8), (712, 2, 712 * 27 * 4), (1422, 2, 1422 * 27 * 4), (1423, 0, 0)):
        p, _ = agree(lib, "ngtdm", P, a, Ng, no_box=True)
        assert (p["mode"], p["lds"]) == (mode, lds) and label(p) == "pairs-" + ("global", "lds64", "lds32")[mode]
    for Ng, mode, lds in ((1422, 1, 1422 * 27 * 4), (1423, 0, 0)):
        p, _ = agree(lib, "gldm", P, a, Ng)
        assert (p["mode"], p["lds"]) == (mode, lds) and label(p) == ("pairs-global", "pairs-lds32")[mode]


def test_sixteen_waves_beyond_40_kib(lib):
    shape = (64, 64, 64)
    a = real_angles(lib, shape)
    p, _ = agree(lib, "gldm", shape, a, 379)                                             # 379 x 27 x 4 = 40 932 bytes
    assert (p["lds"], p["threads"], p["grid"]) == (40932, 256, 64 ** 3 // 256)
    assert plan(lib, "gldm", shape, a, 379, cus=8)["grid"] == 8 * 16
    p, _ = agree(lib, "gldm", shape, a, 380)                                             # 41 040
    assert (p["lds"], p["threads"], p["grid"]) == (41040, 1024, CUS)
    p, _ = agree(lib, "ngtdm", shape, a, 380)
    assert p["box"] and p["box_grid"] == min(64 ** 3 // 256, CUS * 32)


# ---- 3. the overflow rule of the u32 bins, on the plan alone -----------------------------------------------------------------
BIG = [(2048, 2048, 2048), (1024, 1024, 2044), (1290, 1290, 1292), (2048, 2048, 4), (512, 512, 512), (1, 1, 2 ** 30), (300, 300, 300),
       (1024, 1024, 2047), (2048, 2048, 511)]


def test_a_workgroup_of_the_u32_bins_stays_below_2_to_31(lib):
    seen = 0
    for shape in BIG:
        n = int(np.prod(shape, dtype=np.int64))
        for dist, no_box in (((1,), True), ((1, 2), True), ((1, 2), False), ((1, 2, 3), False), ((1, 2, 3), True)):
            a = real_angles(lib, shape, dist)
            for Ng in (56, 111, 154, 255, 307, 1422):
                for cus in (1, CUS):
                    p = plan(lib, "ngtdm", shape, a, Ng, no_box=no_box, cus=cus)
                    if n >= 2 ** 31 - 1 or (len(a) > 128 and no_box):
                        assert not p["applies"], (shape, dist, Ng, p)
                    elif p["mode"] == 2:
                        assert -(-n // p["grid"]) * len(a) * Ng <= 2 ** 31, (shape, dist, Ng, cus, p)
                        assert p["grid"] <= -(-n // p["threads"])
                        seen += 1
    assert seen >= 100          # Na 26 at 1422 levels, 124 at 154 / 255 / 307, 342 at 56 / 111


def test_arguments_no_call_accepts(lib):
    size, one, out = np.array([3, 3, 4], dtype=np.intc), np.zeros((1, 3), dtype=np.intc), np.zeros(64, dtype=np.intc)
    call = lambda *a: lib.prad_debug_neigh_plan(*a)      # noqa: E731
    assert call(_ip(size), 3, _ip(one), 0, 32, 0, 0, CUS, _ip(out), 64) == 0        # Na < 1
    assert call(_ip(size), 3, _ip(one), 1, 0, 0, 0, CUS, _ip(out), 64) == 0         # Ng < 1
    assert call(_ip(size), 0, _ip(one), 1, 32, 0, 0, CUS, _ip(out), 64) == 0        # Nd < 1
    assert call(None, 3, _ip(one), 1, 32, 0, 0, CUS, _ip(out), 64) == 0
    assert call(_ip(size), 3, _ip(real_angles(lib, (3, 3, 4))), 26, 32, 0, 0, CUS, _ip(out), 8) == -len(FIELDS)
    four = (2, 3, 3, 4)                                                              # 4-D: the exact kernels
    assert not plan(lib, "gldm", four, real_angles(lib, four), 300)["applies"]
    # cus <= 0: the device's compute units, 256 without one -- either way a plan, and the same placement
    p = plan(lib, "gldm", (64, 64, 64), real_angles(lib, (64, 64, 64)), 380, cus=0)
    assert p["applies"] and p["threads"] == 1024 and 1 <= p["grid"] <= 64 ** 3 // 1024

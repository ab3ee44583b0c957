"""The grid of sweep-plan cases behind tests/golden/sweep_plans.npz, and how one case is replayed through
prad_debug_sweep_plan.  Shared by the recorder (tests/golden/make_sweep_plans.py) and tests/test_sweep_plan.py; host only.

A case is nine ints: Nz Ny Nx Ng nr_delta wants alist cus switch.
  (Nz, Ny) = (1, 1): a 1-D call of size [Nx]; Nz = 1: a 2-D call [Ny, Nx]; else 3-D.
  Nr = longest edge + nr_delta.  wants: 1 GLCM, 2 GLRLM, 3 both.  alist: index into ANGLE_LISTS.  cus: compute units.
  switch: index into the fixture's `switches` (one "NAME=value" set for the case), or -1."""
import ctypes as C
import hashlib
import os

import numpy as np

NX = [1, 2, 47, 48, 64, 65, 95, 96, 191, 192, 256, 257, 512, 513, 1024, 1025]
ZY = [(1, 1), (1, 5), (3, 3), (40, 9), (130, 64)]
# (36|37, 39|40, 95|96, 125|126, 157|158 and 170|171 are where the planner changes its table regime: tests/sweep_limits_cases.py)
NG = [1, 7, 8, 32, 36, 37, 39, 40, 44, 45, 63, 64, 95, 96, 100, 125, 126, 157, 158, 160, 161, 170, 171, 255, 256]
WANTS = [3, 1, 2]
CUS = [256, 250, 12]
ANGLE_LISTS = ["unit", "unit_no_x", "x_only", "bidirectional", "distance2", "two_x", "too_many"]
REFUSED_LISTS = [3, 4, 5, 6]
MAX_SWEEP = 16          # PRAD_MAX_SWEEP (csrc/kernels_sweep.h)
RECORD_CAP = 1024

# every switch the planner reads, with one value that is not its default
SWITCHES = ["PRAD_NO_FW2=1", "PRAD_FW2_COPIES=2", "PRAD_FW2_RS=16", "PRAD_FW2_NOSKIP1=1", "PRAD_NO_FW2_ROWS=1",
            "PRAD_FW2_ROWS_WAVES=8", "PRAD_THREADS=512", "PRAD_LPL=2", "PRAD_NO_FW=1", "PRAD_FW_BUDGET_KB=64", "PRAD_FW_RS=12",
            "PRAD_FW_ROWS_THREADS=256", "PRAD_FW_BLOCKS=100", "PRAD_FW_THREADS=512", "PRAD_FW_XROLE=0", "PRAD_FW_XBLOCKS=40",
            "PRAD_FW_XGPD=4", "PRAD_FW_PER_WAVE=3", "PRAD_FW_XCD=1", "PRAD_FW_CL=24"]
# (Nz, Ny, Nx, Ng) of the cases every switch is flipped on: fused-table and two-table fixed-window volumes at each window
# width, a volume of the wrapped-lines kernels, one whose rows are too long for the two-table kernel, and the 512^3 headline
# (marches long enough for the piece length to follow PRAD_FW_PER_WAVE)
SWITCH_SHAPES = [(512, 512, 512, 32), (130, 64, 256, 32), (130, 64, 512, 32), (130, 64, 513, 32), (130, 64, 1024, 8), (40, 9, 192, 32),
                 (40, 9, 96, 44), (130, 64, 256, 64), (130, 64, 512, 100), (40, 9, 257, 160), (130, 64, 65, 45)]
# cases whose whole record is kept in the fixture, so that a mismatch can be read: name -> case
NAMED = {
    "headline_512_ng32": (512, 512, 512, 32, 0, 3, 0, 256, -1),
    "fw_256_ng32": (130, 64, 256, 32, 0, 3, 0, 256, -1),
    "fw_65_ng44": (130, 64, 65, 44, 0, 3, 0, 256, -1),
    "fw_513_ng32": (130, 64, 513, 32, 0, 3, 0, 256, -1),
    "fw_1024_ng8": (40, 9, 1024, 8, 0, 3, 0, 256, -1),
    "fw_512_cus250": (130, 64, 512, 32, 0, 3, 0, 250, -1),
    "fw_512_cus12": (130, 64, 512, 32, 0, 3, 0, 12, -1),
    "fw_512_no_x": (130, 64, 512, 32, 0, 3, 1, 256, -1),
    "fw2_512_ng64": (130, 64, 512, 64, 0, 3, 0, 256, -1),
    "fw2_257_ng160": (130, 64, 257, 160, 0, 3, 0, 256, -1),
    "fw2_192_ng45_no_x": (40, 9, 192, 45, 0, 3, 1, 256, -1),
    "lines_1025_ng32": (40, 9, 1025, 32, 0, 3, 0, 256, -1),
    "lines_64_ng32": (130, 64, 64, 32, 0, 3, 0, 256, -1),
    "lines_512_ng161": (130, 64, 512, 161, 0, 3, 0, 256, -1),
    "lines_192_ng255": (40, 9, 192, 255, 0, 3, 0, 256, -1),
    "glcm_only_512_ng64": (130, 64, 512, 64, 0, 1, 0, 256, -1),
    "glrlm_only_512_ng64": (130, 64, 512, 64, 0, 2, 0, 256, -1),
    "x_only_512_ng32": (130, 64, 512, 32, 0, 3, 2, 256, -1),
    "two_d_5x192_ng32": (1, 5, 192, 32, 0, 3, 0, 256, -1),
    "one_d_96_ng7": (1, 1, 96, 7, 0, 3, 0, 256, -1),
    "short_nr_refused": (130, 64, 512, 32, -1, 3, 0, 256, -1),
    "ng256_refused": (130, 64, 512, 256, 0, 3, 0, 256, -1),
}


def grid():
    """the cases, in the fixture's order"""
    cases = []
    for zy in ZY:
        for nx in NX:
            for ng in NG:
                for w in WANTS:                      # every table choice under the three lists a call can plan for
                    for al in (0, 1, 2):
                        cases.append(zy + (nx, ng, 0, w, al, 256, -1))
                for cus in CUS[1:]:                  # the remainder of the workgroups over the roles
                    for al in (0, 1):
                        cases.append(zy + (nx, ng, 0, 3, al, cus, -1))
            for w in WANTS:                          # Nr one short of the longest edge
                cases.append(zy + (nx, 32, -1, w, 0, 256, -1))
            for al in REFUSED_LISTS:
                cases.append(zy + (nx, 32, 0, 3, al, 256, -1))
    for si in range(len(SWITCHES)):
        for shp in SWITCH_SHAPES:
            cases.append(shp + (0, 3, 0, 256, si))
    cases.extend(NAMED.values())
    return np.array(cases, dtype=np.int32)


def size_of(case):
    nz, ny, nx = (int(v) for v in case[:3])
    if nz == 1 and ny == 1:
        return [nx]
    return [ny, nx] if nz == 1 else [nz, ny, nx]


def _built(lib, size, dist, bidirectional):
    nd = len(size)
    sz = (C.c_int * nd)(*size)
    ds = (C.c_int * 1)(dist)
    na = lib.prad_get_angle_count(sz, ds, nd, 1, bidirectional, -1)
    out = np.zeros((na, nd), np.int32)
    if na >= 1:
        assert lib.prad_build_angles(sz, ds, nd, 1, -1, na, out.ctypes.data_as(C.POINTER(C.c_int))) == 0
    return out


def angle_list(lib, size, alist):
    """int32 [Na][Nd] (Na may be 0: the shape has no such list, the case is left out)"""
    nd = len(size)
    unit = _built(lib, size, 1, 0)
    is_x = (unit[:, :-1] == 0).all(axis=1) if len(unit) else np.zeros(0, bool)
    name = ANGLE_LISTS[alist]
    if name == "unit":
        return unit
    if name == "unit_no_x":
        return unit[~is_x]
    if name == "x_only":
        return unit[is_x]
    if name == "bidirectional":
        return _built(lib, size, 1, 1)
    if name == "distance2":
        return _built(lib, size, 2, 0)
    if name == "two_x":
        return np.concatenate([unit, unit[is_x]]) if is_x.any() else unit[:0]
    if name == "too_many":
        return np.concatenate([unit] + [unit[:1]] * (MAX_SWEEP + 1 - len(unit))) if len(unit) else unit
    raise ValueError(alist)


def plan(lib, case, switches=SWITCHES, angles=None):
    """the record of one case (int32 array), or None when the shape has no such angle list"""
    size = size_of(case)
    if angles is None:
        angles = angle_list(lib, size, int(case[6]))
    if len(angles) == 0:
        return None
    angles = np.ascontiguousarray(angles, dtype=np.int32)
    nr = max(size) + int(case[4])
    if nr < 1:
        return None
    out = np.zeros(RECORD_CAP, np.int32)
    sw = int(case[8])
    name = None
    if sw >= 0:
        name, value = switches[sw].split("=")
        os.environ[name] = value
    try:
        n = lib.prad_debug_sweep_plan((C.c_int * len(size))(*size), len(size), angles.ctypes.data_as(C.POINTER(C.c_int)),
                                      len(angles), int(case[3]), nr, int(case[5]) & 1, (int(case[5]) >> 1) & 1, int(case[7]),
                                      out.ctypes.data_as(C.POINTER(C.c_int)), RECORD_CAP)
    finally:
        if name is not None:
            del os.environ[name]
    assert n >= 1, "prad_debug_sweep_plan returned %d for case %s" % (n, list(case))
    return out[:n].copy()


def digest(record):
    return np.frombuffer(hashlib.blake2b(record.astype("<i4").tobytes(), digest_size=8).digest(), dtype="<u8")[0]


def replay(lib, cases, switches=SWITCHES):
    """records of all cases (None where a shape has no such list); the angle lists are built once per shape"""
    lists = {}
    out = []
    for case in cases:
        key = (tuple(size_of(case)), int(case[6]))
        if key not in lists:
            lists[key] = angle_list(lib, list(key[0]), key[1])
        out.append(plan(lib, case, switches, lists[key]))
    return out

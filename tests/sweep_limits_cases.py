"""Host-side constructions behind tests/test_gpu_sweep_limits.py: the plan record of prad_debug_sweep_plan by field name, the
scan for the grey-level counts at which the planner changes its table regime, and volumes with PLANTED runs -- runs of a known
level, length and angle that sit on the edges of a kernel's run-length slots.  Host only (numpy + the planner, which makes no
device call); tests/test_sweep_limits_cases.py checks the constructions themselves.

Planted runs.  The background is noise from the lower half of the levels (1 .. Ng // 2), planted runs carry levels of the upper
half, so a planted level occurs nowhere else.  A run of length L along angle a is the voxels s + k a, k < L; the voxels s - a and
s + L a are background, masked out or outside the volume.  `occ` marks every planted voxel and its 26 neighbours, and a new run
takes only voxels outside it: two planted runs never touch along any of the 13 angles, so along every angle but its own a
planted run falls into isolated voxels, and along its own it is one run of exactly L.  The reference's GLRLM of such a volume
therefore holds, at [level - 1, L - 1, angle] for L >= 2, exactly the number of runs planted with that key (expected_counts)."""
import os

import numpy as np

import sweep_plan_cases as spc

# the head of the plan record (include/pyradiomics_amd.h, prad_debug_sweep_plan)
FIELDS = ["ok", "Nz", "Ny", "Nx", "fused", "fw", "fw2", "fw2_rows", "RS", "RSr", "RSfw", "RSfw_rows", "RS2", "RS2r", "LONG", "LONGr",
          "LONGfw", "LONGfw2", "LONGfw2r", "lds_bytes", "lds_bytes_rows", "lds_fw", "lds_fw_rows", "lds_fw2", "lds_fw2_rows", "threads",
          "fw_threads", "fw_rows_threads", "fwK", "fw_blocks", "fw2_copies", "fw2r_copies", "fw2r_waves", "LPL", "pitch", "padw",
          "pitch16", "vec_rows", "skip1", "row_slot", "fw_xblocks", "lines_count"]
KEY = ["ok", "fused", "fw", "fw2", "fw2_rows", "fw2_copies", "fw2r_copies", "fw2r_waves"]
SCAN_SHAPES = [(12, 10, 300), (12, 10, 64), (6, 5, 600)]          # one per row class: 65..512, <= 64, 513..1024
# regime changes (Ng below | Ng above) that the scan of each shape has to find: a retuned planner fails the tests loudly
REQUIRED = {(12, 10, 300): [(36, 37), (39, 40), (125, 126), (157, 158), (170, 171)],
            (12, 10, 64): [(36, 37), (95, 96)],
            (6, 5, 600): [(36, 37), (95, 96)]}
# the changes a scan for 256 compute units finds (recorded; profiles/sweep_limits_measurements.md has what they change)
SCAN_256 = {(12, 10, 300): [(36, 37), (39, 40), (90, 91), (109, 110), (111, 112), (125, 126), (143, 144), (146, 147), (157, 158), (170, 171)],
            (12, 10, 64): [(36, 37), (95, 96)],
            (6, 5, 600): [(36, 37), (95, 96)]}
LONG_BINS = 64            # PRAD_LONG_BINS (csrc/kernels_sweep.h): lengths RS + 1 .. RS + 64 of a fused table stay in LDS


def fields(record):
    """the head of a plan record as a dict (a declined plan: {"ok": 0})"""
    if record is None or int(record[0]) == 0:
        return {"ok": 0}
    return {name: int(v) for name, v in zip(FIELDS, record)}


def plan_fields(lib, size, Ng, nr_delta=0, wants=3, cus=0, angles=None):
    """the plan of a call of this size ([Nx], [Ny, Nx] or [Nz, Ny, Nx]) under the environment's switches; cus = 0: the device's"""
    size = [int(v) for v in size]
    if angles is None:
        angles = spc.angle_list(lib, size, 0)
    return fields(_plan_of_size(lib, size, angles, Ng, max(size) + nr_delta, wants, cus))


def _plan_of_size(lib, size, angles, Ng, Nr, wants, cus):
    import ctypes as C
    angles = np.ascontiguousarray(angles, dtype=np.int32)
    out = np.zeros(spc.RECORD_CAP, np.int32)
    n = lib.prad_debug_sweep_plan((C.c_int * len(size))(*size), len(size), angles.ctypes.data_as(C.POINTER(C.c_int)), len(angles), int(Ng),
                                  int(Nr), wants & 1, (wants >> 1) & 1, int(cus), out.ctypes.data_as(C.POINTER(C.c_int)), spc.RECORD_CAP)
    assert n >= 1
    return out[:n].copy()


def regime_key(f):
    return tuple(f.get(k, 0) for k in KEY) if f["ok"] else (0,)


def regime_changes(lib, shape, cus=0):
    """[(Ng, Ng + 1)] wherever the key changes between the plans of Ng and Ng + 1, Ng = 1 .. 255, GLCM and GLRLM both wanted"""
    angles = spc.angle_list(lib, list(shape), 0)
    keys = [regime_key(plan_fields(lib, shape, ng, cus=cus, angles=angles)) for ng in range(1, 257)]
    return [(ng, ng + 1) for ng in range(1, 256) if keys[ng - 1] != keys[ng]]


def expected_variant(f, wants=3):
    """(last_path, last_variant) of a synchronous call with this plan on regular levels: a declined call ends on the pairs tier"""
    if not f["ok"]:
        return "pairs", "pairs"
    return "sweep", "fw2" if f["fw2"] else ("fw" if f["fw"] and wants == 3 else "lines")


def tables(f, Nr):
    """the run-length tables of a plan that have a long-run path: [(name, "lines" | "x", RS, fused)].  "lines": the table of
    the kernel that walks the twelve angles with a z or y component, "x": of the one that walks the x angle"""
    if f["fw"]:
        t = [("RSfw", "lines", f["RSfw"], True), ("RSfw_rows", "x", f["RSfw_rows"], True)]
    elif f["fw2"]:
        t = [("RS2", "lines", f["RS2"], False), ("RS2r", "x", f["RS2r"], False) if f["fw2_rows"] else ("RSr", "x", f["RSr"], False)]
    else:
        t = [("RS", "lines", f["RS"], bool(f["fused"])), ("RSr", "x", f["RSr"], bool(f["fused"]))]
    return [e for e in t if 1 <= e[2] < Nr]


def is_x(angle):
    return not any(int(v) for v in angle[:-1])


def requests(tabs, angles, only=None):
    """what to plant for these tables: [(table name, angle index, length, kind)].  Per table and per angle its kernel walks:
    the lengths RS - 1 .. RS + 2 around the last LDS slot, for a fused table RS + 63 .. RS + 66 around the last bin of the long
    table G as well (kind "free"); a run that ends at the volume's edge, one that ends at a masked-out voxel, one that starts
    at march step 7.  only: {table name: [angle indices]} restricts a table to the angles whose lines are long enough"""
    out = []
    for name, role, rs, fused in tabs:
        for ai, a in enumerate(angles):
            if is_x(a) != (role == "x") or (only is not None and ai not in only.get(name, range(len(angles)))):
                continue
            lengths = [rs - 1, rs, rs + 1, rs + 2]
            if fused:
                lengths += [rs + LONG_BINS - 1, rs + LONG_BINS, rs + LONG_BINS + 1, rs + LONG_BINS + 2]
            out += [(name, ai, L, "free") for L in lengths if L >= 1]
            out += [(name, ai, rs + 1, "edge"), (name, ai, max(rs, 2), "masked"), (name, ai, rs + 2, "step7")]
    return out


def _march_dim(a):
    return next(d for d in range(len(a)) if a[d])


def _find_start(shape, a, L, kind, occ, rng, tries=4000):
    nd = len(shape)
    span = L + 1 if kind == "masked" else L           # the masked-out voxel behind the run lies inside the volume
    lo, hi = [0] * nd, [0] * nd
    for d in range(nd):
        lo[d] = span - 1 if a[d] < 0 else 0
        hi[d] = shape[d] - span if a[d] > 0 else shape[d] - 1
        if hi[d] < lo[d]:
            return None
    m = _march_dim(a)
    if kind == "edge":
        lo[m] = hi[m] = shape[m] - L
    if kind == "step7":
        if not lo[m] <= 7 <= hi[m]:
            return None
        lo[m] = hi[m] = 7
    k = np.arange(L)
    for _ in range(tries):
        s = [int(rng.integers(lo[d], hi[d] + 1)) for d in range(nd)]
        idx = tuple(s[d] + k * int(a[d]) for d in range(nd))
        if not occ[idx].any():
            return s
    return None


def plant(shape, Ng, angles, reqs, seed, keep=0.9):
    """-> img int32, mask bool, placed [(table, angle index, L, kind, level, start)], missing [requests that found no place]"""
    rng = np.random.default_rng(seed)
    shape = tuple(int(v) for v in shape)
    half = max(1, Ng // 2)
    assert Ng >= 2 and half < Ng
    img = rng.integers(1, half + 1, size=shape).astype(np.int32)
    mask = rng.random(shape) < keep
    occ = np.zeros(shape, bool)
    upper = list(range(Ng, half, -1))                  # Ng first: the top level is always planted
    placed, missing = [], []
    for i in sorted(range(len(reqs)), key=lambda j: -reqs[j][2]):      # the longest first: they have the fewest places
        name, ai, L, kind = reqs[i]
        a = [int(v) for v in angles[ai]]
        s = _find_start(shape, a, L, kind, occ, rng)
        if s is None:
            missing.append((name, ai, L, kind))
            continue
        level = upper[i % len(upper)]
        for k in range(L):
            p = tuple(s[d] + k * a[d] for d in range(3))
            img[p] = level
            mask[p] = True
            occ[tuple(slice(max(0, c - 1), c + 2) for c in p)] = True
        if kind == "masked":
            mask[tuple(s[d] + L * a[d] for d in range(3))] = False
        placed.append((name, ai, L, kind, level, tuple(s)))
    return img, mask, placed, missing


def expected_counts(placed):
    """{(level, L, angle index): runs planted with that key}"""
    out = {}
    for _name, ai, L, _kind, level, _s in placed:
        out[(level, L, ai)] = out.get((level, L, ai), 0) + 1
    return out


def construction_errors(glrlm, placed, Ng):
    """what the REFERENCE's GLRLM ([Ng, Nr, Na]) says about a planted volume: [] when every planted (level, L >= 2, angle) has
    exactly its planted count and no other run of two or more voxels carries an upper-half level"""
    want = expected_counts(placed)
    bad = []
    for (level, L, ai), n in want.items():
        if L >= 2 and glrlm[level - 1, L - 1, ai] != n:
            bad.append(("count", level, L, ai, float(glrlm[level - 1, L - 1, ai]), n))
        if L == 1 and glrlm[level - 1, 0, ai] < n:
            bad.append(("count", level, L, ai, float(glrlm[level - 1, 0, ai]), n))
    longer = glrlm[max(1, Ng // 2):, 1:, :]
    if longer.sum() != sum(n for (_lv, L, _a), n in want.items() if L >= 2):
        bad.append(("stray runs of planted levels", float(longer.sum())))
    return bad


def isolated(shape, Ng, seed, keep=0.8, extra=60):
    """a volume whose upper-half levels occur only as voxels without an equal (or any planted) neighbour: on all corners, on the
    middle of every edge and face, at random places inside, some of them next to a masked-out voxel.  Every run of a planted
    level has length 1 along all 13 angles.  -> img, mask, planted [(level, position)]"""
    rng = np.random.default_rng(seed)
    shape = tuple(int(v) for v in shape)
    half = max(1, Ng // 2)
    img = rng.integers(1, half + 1, size=shape).astype(np.int32)
    mask = rng.random(shape) < keep
    occ = np.zeros(shape, bool)
    spots = []
    for z in (0, shape[0] // 2, shape[0] - 1):         # corners (8), edge middles (12), face middles (6), and the centre
        for y in (0, shape[1] // 2, shape[1] - 1):
            for x in (0, shape[2] // 2, shape[2] - 1):
                spots.append((z, y, x))
    for _ in range(extra * 50):
        if len(spots) >= 27 + extra:
            break
        spots.append(tuple(int(rng.integers(0, n)) for n in shape))
    upper = list(range(Ng, half, -1))
    planted = []
    for p in spots:
        if occ[p]:
            continue
        level = upper[len(planted) % len(upper)]
        img[p] = level
        mask[p] = True
        occ[tuple(slice(max(0, c - 1), c + 2) for c in p)] = True
        if len(planted) % 3 == 0:                      # a masked-out voxel next to it, in a direction that varies
            step = [(0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 1, 1), (0, 1, -1), (1, -1, 0)][(len(planted) // 3) % 6]
            q = tuple(c + d if c + d < n else c - d for c, d, n in zip(p, step, shape))
            if all(0 <= c < n for c, n in zip(q, shape)):
                mask[q] = False
        planted.append((level, p))
    return img, mask, planted


def longest_run(img, mask, angles):
    """the longest run of equal levels under the mask along any of the angles (a plain numpy walk, no checker involved)"""
    img = np.asarray(img)
    mask = np.asarray(mask, bool)
    lev = np.where(mask, img, 0)
    best = 1 if mask.any() else 0
    for a in angles:
        a = [int(v) for v in a]
        alive = lev != 0
        n = 1
        while True:
            src = tuple(slice(max(0, -n * d), s - max(0, n * d)) for d, s in zip(a, lev.shape))
            dst = tuple(slice(max(0, n * d), s - max(0, -n * d)) for d, s in zip(a, lev.shape))
            if any(s.stop <= s.start for s in src):
                break
            nxt = np.zeros_like(alive)
            nxt[src] = alive[src] & (lev[src] == lev[dst])          # the run from this voxel reaches n steps further
            alive = nxt
            if not alive.any():
                break
            n += 1
            best = max(best, n)
    return best


def noise(shape, Ng, seed, keep=0.7):
    """uniform levels under a random mask that keeps `keep` of the voxels; every level 1 .. Ng occurs under the mask"""
    rng = np.random.default_rng(seed)
    img = rng.integers(1, Ng + 1, size=shape).astype(np.int32)
    mask = rng.random(shape) < keep
    inside = np.flatnonzero(mask.ravel())
    if len(inside) < Ng:                               # (tiny shapes: keep everything)
        mask[...] = True
        inside = np.arange(mask.size)
    assert len(inside) >= Ng, "shape %s has no room for %d levels" % (shape, Ng)
    img.ravel()[rng.choice(inside, size=Ng, replace=False)] = np.arange(1, Ng + 1)
    return img, mask


def smooth(shape, Ng, seed):
    """slowly varying levels (runs of several voxels along every angle) under a full mask"""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    f = np.zeros(shape)
    for _ in range(4):
        w = rng.uniform(0.02, 0.12, size=len(shape))
        f += np.sin(sum(wi * g for wi, g in zip(w, grids)) + rng.uniform(0, 6.28))
    f = (f - f.min()) / (f.max() - f.min() + 1e-12)
    return np.minimum((f * Ng).astype(np.int32) + 1, Ng).astype(np.int32), np.ones(shape, bool)


class switches:
    """PRAD_* switches in the environment for the length of a with-block (host-side tests; the GPU tests use monkeypatch)"""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---- the planted-run cases: name -> (switches, Ng, shape, {table: the dimension its angles must not move in} or None) ---------
# The shape of the fused and two-table cases holds RSfw + 66 voxels along the space diagonals (RSfw = 23 at 36 levels).
# Separate tables hold many more lengths, so their long-run path needs long lines, and such volumes get large.  At 38 levels only
# rows of more than 202 voxels have one (the x angle; 445 slots serve the line angles).  The line angles are reached at 90 and 95
# levels (114 and 98 slots), three volumes for three groups of angles, each restricted to the angles whose lines are long enough
# in it (the host test asserts which):
#   rows of 64 voxels, 126 x 125 of them: the four angles that do not move in x -- (1,0,0), (0,1,0), (1,1,0), (1,-1,0);
#   rows of 520 voxels (separate tables again from 513 on), 108 planes of 3 rows: (1,0,0) and the two that drift in x while they
#   march z, (1,0,1) and (1,0,-1) -- their lines wrap in x and break, Walker::step_brk under risky() and the checked step;
#   the same with 3 planes of 108 rows: (0,1,0), (0,1,1), (0,1,-1).
# LEFT OUT for its size: the four space diagonals (1,+-1,+-1) at the slot edge of separate tables.  They need 100 voxels along z
# AND y in rows of more than 512, about 6 M voxels, six times the largest volume here; the fused table has them (fused_lines_rows).
PLANTED = {
    "fused_fw": ({}, 36, (100, 99, 104), None),
    "fused_fw_rows_launch": ({"PRAD_FW_XROLE": "0"}, 36, (100, 99, 104), None),
    "fused_lines_rows": ({"PRAD_NO_FW": "1"}, 36, (100, 99, 104), None),
    "separate_ng38_x": ({}, 38, (12, 10, 300), None),
    "separate_ng90": ({}, 90, (126, 125, 64), {"RS": 2}),
    "separate_ng95_zx": ({}, 95, (108, 3, 520), {"RS": 1}),
    "separate_ng95_yx": ({}, 95, (3, 108, 520), {"RS": 0}),
    "fw2_ng64": ({}, 64, (100, 99, 104), None),
    "fw2_ng126": ({}, 126, (100, 99, 104), None),
    "fw2_ng170": ({}, 170, (100, 99, 104), None),
    "fw2_rows8_ng170": ({"PRAD_NO_FW2_ROWS": "1"}, 170, (100, 99, 104), None),
}
# the line angles each restricted case plants on
ONLY_ANGLES = {"separate_ng90": [(1, 0, 0), (0, 1, 0), (1, 1, 0), (1, -1, 0)], "separate_ng95_zx": [(1, 0, 0), (1, 0, 1), (1, 0, -1)],
               "separate_ng95_yx": [(0, 1, 0), (0, 1, 1), (0, 1, -1)]}
# the kernels each case has to reach: (fused, fw, fw2, fw2_rows, x as trailing role) of its plan
REACHES = {
    "fused_fw": (1, 1, 0, 0, True), "fused_fw_rows_launch": (1, 1, 0, 0, False), "fused_lines_rows": (1, 0, 0, 0, False),
    "separate_ng38_x": (0, 0, 0, 0, False), "separate_ng90": (0, 0, 0, 0, False), "separate_ng95_zx": (0, 0, 0, 0, False),
    "separate_ng95_yx": (0, 0, 0, 0, False), "fw2_ng64": (0, 0, 1, 1, False),
    "fw2_ng126": (0, 0, 1, 1, False), "fw2_ng170": (0, 0, 1, 1, False), "fw2_rows8_ng170": (0, 0, 1, 0, False),
}


def planted_case(lib, name, cus=0):
    """-> dict(env, Ng, shape, Nr, angles, plan, tables, reqs, img, mask, placed, missing) of one PLANTED case, planned under
    its switches for `cus` compute units (0: the device's)"""
    env, Ng, shape, only = PLANTED[name]
    angles = spc.angle_list(lib, list(shape), 0)
    Nr = max(shape)
    with switches(**env):
        f = plan_fields(lib, shape, Ng, cus=cus)
    tabs = tables(f, Nr)
    if only is not None:
        only = {t: [i for i, a in enumerate(angles) if int(a[still]) == 0 and not is_x(a)] for t, still in only.items()}
    reqs = requests(tabs, angles, only)
    img, mask, placed, missing = plant(shape, Ng, angles, reqs, seed=sum(name.encode()))
    return dict(env=env, Ng=Ng, shape=shape, Nr=Nr, angles=angles, plan=f, tables=tabs, reqs=reqs, img=img, mask=mask, placed=placed,
                missing=missing, only=only)

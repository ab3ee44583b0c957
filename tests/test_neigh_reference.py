"""CPU: pins tests/neigh_reference.py -- the numpy / Python-int restatement of GLDM, NGTDM and the GLCM pair count that the GPU
limit modules (test_gpu_neigh_limits.py, test_gpu_pairs_limits.py) compare against -- to the C checker on every case of the
shared table, and shows that the table is sharp: every group of cases changes its matrices under each kernel hazard it exists
to catch (neigh_reference's `defect=` models).  A case table that a mutant passes is a failure of the table, not of the
assertion."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import neigh_reference as nr


def _reference(name, checker, defect=None):
    """the matrices of the case's family from the numpy model: (integer matrix as float64, s_i or None)"""
    s = nr.spec(name)
    ang = nr.case_angles(name, checker)
    levels, mask, Ng, dist, alpha, f2d, dim, _ = nr.case(name)
    if s["family"] == "glcm":
        return nr.glcm_counts(levels, mask, Ng, ang, defect).astype(np.float64), None
    g, n = nr.accumulators(levels, mask, Ng, ang, alpha, defect)
    if s["family"] == "gldm":
        return nr.gldm_matrix(g), None
    return nr.ngtdm_matrix(n)[:, (0, 2)], nr.ngtdm_s(n)


def _changed(a, b):
    return not np.array_equal(a[0], b[0]) or (a[1] is not None and not np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("group", sorted(nr.GROUPS))
def test_reference_equals_the_checker(group, checker):
    """integer parts bit for bit; s_i (correctly rounded) within 1e-10 relative of the checker's raster-order float64 sum"""
    for name in nr.GROUPS[group]:
        s = nr.spec(name)
        levels, mask, Ng, dist, alpha, f2d, dim, _ = nr.case(name)
        ref, s_i = _reference(name, checker)
        if s["family"] == "glcm":
            want, wang = checker.calculate_glcm(levels, mask, dist, Ng, f2d, dim)
            assert np.array_equal(wang, nr.case_angles(name, checker))
            assert np.array_equal(ref, want[0]), name
        elif s["family"] == "gldm":
            assert np.array_equal(ref, checker.calculate_gldm(levels, mask, dist, Ng, alpha, f2d, dim)[0]), name
            if alpha < 0:
                assert not ref[:, 1:].any(), name              # every voxel in column 0
        else:
            want = checker.calculate_ngtdm(levels, mask, dist, Ng, f2d, dim)[0]
            assert np.array_equal(ref, want[:, (0, 2)]), name
            assert np.all(np.abs(s_i - want[:, 1]) <= 1e-10 * np.abs(s_i)), name


@pytest.mark.parametrize("group", sorted(g for g in nr.GROUPS if not g.startswith("edges:")))
def test_every_group_catches_its_defects(group, checker):
    names = nr.GROUPS[group]
    if group == "big":
        names = names[:1]                                       # (561 600 voxels: one case answers for all five)
    base = {}
    for defect in nr.group_defects(group):
        for name in names:
            if name not in base:
                base[name] = _reference(name, checker)
            if _changed(base[name], _reference(name, checker, defect)):
                break
        else:
            pytest.fail("no case of %s notices the defect %s" % (group, defect))


@pytest.mark.parametrize("shape", nr.QUAD_SHAPES + nr.SCALAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_cases_are_the_sensitive_combinations(shape, checker):
    """a content x mask combination is in the shape's "edges" group exactly when an edge defect changes its GLDM or NGTDM
    accumulators; together the group notices every edge defect that the shape's geometry allows"""
    ang = checker.generate_angles(shape, [1], True, False, 0)
    caught = set()
    for cont, mask in itertools.product(nr.CONTENTS, nr.STRUCTURED_MASKS):
        levels, m = nr.content(cont, shape, 32), nr.roi(mask, shape)
        g0, n0 = nr.accumulators(levels, m, 32, ang)
        hit = set()
        for d in nr.EDGE_DEFECTS:
            g, n = nr.accumulators(levels, m, 32, ang, defect=d)
            if not (np.array_equal(g, g0) and np.array_equal(n, n0)):
                hit.add(d)
        assert bool(hit) == nr.edge_combo_listed(shape, cont, mask), (shape, cont, mask, hit)
        listed = any(nr.spec(n)["content"] == cont and nr.spec(n)["mask"] == mask and nr.spec(n)["Ng"] == 32
                     for n in nr.GROUPS["edges:" + "x".join(map(str, shape))])
        assert listed == bool(hit), (shape, cont, mask)
        caught |= hit
    assert caught == set(nr.possible_edge_defects(shape)), (shape, caught)


def test_slot0_defect_changes_the_one_pass_inputs(checker):
    for shape, cont, mask in nr.BOTH_INPUTS:
        ang = checker.generate_angles(shape, [1], True, False, 0)
        levels, m = nr.content(cont, shape, 202), nr.roi(mask, shape)
        g, n = nr.accumulators(levels, m, 202, ang)
        assert np.array_equal(n[:, 0], g.sum(axis=1))                 # what neigh4_kernel MODE 2 relies on
        assert not np.array_equal(n, nr.accumulators(levels, m, 202, ang, defect="slot0")[1]), (shape, cont, mask)


@pytest.mark.parametrize("shape", nr.SLAB_SHAPES)
def test_plane_ranges_add_up_and_need_their_halo(shape, checker):
    Ng = 32
    ang = checker.generate_angles(shape, [1], True, False, 0)
    levels, m = nr.content("checker3", shape, Ng), nr.roi("full", shape)
    whole = nr.accumulators(levels, m, Ng, ang)
    assert np.array_equal(nr.gldm_matrix(whole[0]), checker.calculate_gldm(levels, m, [1], Ng, 0, False, 0)[0])
    for part in nr.slab_partitions(shape[0]):
        for defect, same in ((None, True), ("slab-halo", len([r for r in part if r[1] > r[0]]) == 1)):
            acc = [nr.accumulators(levels, m, Ng, ang, defect=defect, zrange=r) for r in part]
            for k in (0, 1):
                assert np.array_equal(sum(a[k] for a in acc), whole[k]) == same, (shape, part, defect, k)
    for r in ((3, 3), (7, 7)):
        assert not nr.accumulators(levels, m, Ng, ang, zrange=r)[0].any()


def test_s_is_the_correctly_rounded_rational():
    acc = np.zeros((3, 27), dtype=np.int64)
    acc[0, 1], acc[0, 3], acc[0, 26] = 1, 1, 5
    acc[2, 7] = 2 ** 52 + 1
    s = nr.ngtdm_s_exact(acc)
    assert s == [Fraction(1) + Fraction(1, 3) + Fraction(5, 26), Fraction(0), Fraction(2 ** 52 + 1, 7)]
    got = nr.ngtdm_s(acc)
    for f, v in zip(s, got):
        v = float(v)
        lo, hi = np.nextafter(v, -np.inf), np.nextafter(v, np.inf)
        assert abs(Fraction(v) - f) <= min(abs(Fraction(float(lo)) - f), abs(Fraction(float(hi)) - f))
    assert np.array_equal(nr.s_bound(got, 26), 28 * 2.0 ** -52 * got)


def test_irregular_levels_raise_what_the_checker_raises(checker):
    levels, m = nr.content("iid", (3, 3, 4), 32), nr.roi("full", (3, 3, 4))
    ang = checker.generate_angles((3, 3, 4), [1], True, False, 0)
    for bad in (0, 33, -1):
        lv = levels.copy()
        lv[1, 1, 1] = bad
        with pytest.raises(IndexError):
            nr.accumulators(lv, m, 32, ang)
        with pytest.raises(IndexError):
            checker.calculate_gldm(lv, m, [1], 32, 0, False, 0)
    lv[1, 1, 1] = 77
    m = m.copy()
    m[1, 1, 1] = False                                          # outside the ROI anything goes
    assert np.array_equal(nr.gldm_matrix(nr.accumulators(lv, m, 32, ang)[0]), checker.calculate_gldm(lv, m, [1], 32, 0, False, 0)[0])


def test_case_names_are_unique_and_cheap_to_list():
    assert len(set(nr.NAMES)) == len(nr.NAMES) == sum(len(v) for v in nr.GROUPS.values())
    for name in nr.NAMES[:5]:
        levels, mask, Ng, dist, alpha, f2d, dim, route = nr.case(name)
        assert levels.dtype == np.int32 and mask.dtype == bool and isinstance(route, str)


def test_route_labels_rest_on_the_checkers_neighbour_set(checker):
    """case() derives its route label from neigh_reference.neighbour_offsets: the same offsets as the checker's list"""
    seen = set()
    for name in nr.NAMES:
        s = nr.spec(name)
        key = (s["shape"], tuple(s["distances"]), s["dim"] if s["force2D"] else None)
        if s["family"] not in ("gldm", "ngtdm") or key in seen:
            continue
        seen.add(key)
        own = nr.neighbour_offsets(*key)
        theirs = nr.case_angles(name, checker)
        assert len(own) == len(theirs) and {tuple(o) for o in own.tolist()} == {tuple(o) for o in theirs.tolist()}, key
    assert len(seen) > 30


@pytest.mark.parametrize("name", nr.GROUPS["glcm-tiles"])
def test_every_row_tile_case_reaches_its_last_tile(name, checker):
    """above 195 levels the GLCM is built in level-row tiles of 38400 / Ng rows: each case must notice a lost last tile by
    itself, and the `cover` cases hold every level of that tile -- with the full mask, with pairs in every angle"""
    s = nr.spec(name)
    levels, mask, Ng = nr.case(name)[:3]
    tiled = Ng * Ng > nr.PAIR_LDS_WORDS
    assert tiled == (Ng > 195)
    ang = nr.case_angles(name, checker)
    base = nr.glcm_counts(levels, mask, Ng, ang)
    assert np.array_equal(base, nr.glcm_counts(levels, mask, Ng, ang, defect="last-tile")) == (not tiled), name
    if not tiled:
        return
    rt = nr.PAIR_LDS_WORDS // Ng
    r0 = ((Ng - 1) // rt) * rt                                   # first level row of the last tile
    assert 0 < r0 < Ng and Ng - r0 == {196: 1, 197: 3, 240: 80}[Ng]
    present = np.unique(levels[mask])
    if s["content"] == "cover":
        assert set(range(r0 + 1, Ng + 1)) <= set(present.tolist()), name
        rows, cols = base[r0:].sum(axis=1), base[:, r0:].sum(axis=0)             # [levels of the tile, Na]
        if s["mask"] == "full":
            assert (rows > 0).all() and (cols > 0).all(), name                  # every level, as centre and as neighbour, in every angle
        else:
            assert (rows.sum(axis=1) > 0).all() and (cols.sum(axis=1) > 0).all(), name
    else:
        assert Ng in present and base[Ng - 1].sum() > 0, name

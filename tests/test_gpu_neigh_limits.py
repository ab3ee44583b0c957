"""GPU: the neighbourhood matrices of segment mode (csrc/kernels_neigh.h: neigh_kernel, neigh4_kernel<MODE, FULL26>) at the
limits of their routes, against the C checker (integer outputs, np.array_equal) and tests/neigh_reference.py (NGTDM's s_i,
correctly rounded from the rational).  tests/test_neigh_reference.py pins that reference to the checker on every case used
here and shows that each group of cases changes under the kernel hazards it exists to catch (a lost x0 - 1 / x0 + 4 edge
byte, a lost lane 0 / lane 63 byte, neighbours wrapped across rows or planes, a slot 0 taken from the wrong GLDM row, a
halo plane read as zero).  Every case asserts the route it took: prad_last_path() and the kernel label of
prad_last_variant() ("neigh4-full26", "neigh4-rows", "neigh1", "pairs-...", or path "generic"), restated from the plans'
documented limits in neigh_reference.expected_route.

Case families (all deterministic; contents checker3, lattice, stripes4, stripes256, ramp, equal, iid; masks full, faces,
quad-edges, wave-edges, holes4 where an edge defect can change the matrices, plus corners, one voxel at each corner and the
centre, and the empty mask):
  edges / degenerate   (3,3,4) (3,5,8) (2,7,12) (3,3,252) (3,3,256) (3,3,260) (1,9,16) (9,16) (5,1,16) (2,2,1028) for the packed
                       kernel -- one quad per row, waves that start mid-row, the lane 63 -> lane 0 hand-over inside a row, Nz == 1,
                       Ny == 1 -- and Nx in {5, 7, 255, 257} for neigh_kernel; 32 levels, and 255 levels on checker3 / iid
  alpha                GLDM with alpha in {0, 1, Ng - 1, Ng + 5, -1} at Ng in {1, 2, 32, 255}, NGTDM at the same Ng, every shape
  big                  (9,240,260): 140 400 quads, a second trip of the grid-stride loop, a ragged last wave
  force2d              (6,8,12) with force2Ddimension 0, 1, 2: row masks without the dz / dy / dx rows (neigh4-rows)
  route-edges          255 -> 256 levels; GLDM [1,2] 131 -> 132, GLDM [2] 165 -> 166, NGTDM [2] 82 -> 83 (plan_neigh's 64 KiB)
  one pass             engine.gldm_ngtdm at 202 levels (one neigh launch) and 203 (two): bit for bit the separate calls
  plane ranges         engine.neigh_accumulate on (7,6,12) and (7,5,9): every split point, single planes, empty ranges, a
                       three-way split; an irregular level in the halo raises what the whole volume raises
  deferred             deferred=True of gldm / ngtdm / gldm_ngtdm: the same bits, irregular levels via deferred_status()

Tolerance.  GLDM, NGTDM columns 0 and 2 and the accumulators must be equal.  NGTDM column 1: |got - exact| <= (Na + 2) 2^-52
exact, exact = the correctly rounded rational sum_c S_c / c.  ngtdm_finalize_kernel does Na divisions of exact integers below
2^53 and Na additions of non-negative terms in float64: (Na + 1) 2^-53 relative to first order; the bound is twice that.

Measured worst error / bound per route over all cases of this module on an MI355X (test_zz_report prints it and fails above 1):
    neigh1                0.037      neigh4-full26       0.0393     neigh4-rows         0.0995
    neigh4-full26+gldm    0.0353     neigh4-rows+gldm    0.0891     ("+gldm": the one-pass GLDM + NGTDM launch)
    pairs-lds64           0.0115     pairs-lds64+box32   0.0357     (the far side of the route edges)
The errors are a rounding or two of the last division and addition: most levels have one or two non-empty slots.

No defect was found: every case passed against the kernels as they were.
"""
import numpy as np
import pytest

import neigh_reference as nr

pytestmark = pytest.mark.gpu

RATIOS = {}            # route -> worst error / bound of NGTDM column 1


def _tag(shape):
    return "x".join(map(str, shape))


_SHAPES = nr.QUAD_SHAPES + nr.SCALAR_SHAPES


@pytest.mark.parametrize("shape", _SHAPES, ids=_tag)
def test_edge_bytes_and_degenerate_masks(shape, checker):
    routes = set()
    for name in nr.GROUPS["edges:" + _tag(shape)] + nr.GROUPS["degenerate:" + _tag(shape)]:
        routes.add(nr.run_case(name, checker, RATIOS))
    want = "neigh1" if shape[-1] % 4 else ("neigh4-full26" if len(shape) == 3 and min(shape) > 1 else "neigh4-rows")
    assert routes == {want}, routes


@pytest.mark.parametrize("shape", _SHAPES, ids=_tag)
def test_alpha_and_level_counts(shape, checker):
    routes = set()
    for name in nr.GROUPS["alpha:" + _tag(shape)]:
        routes.add(nr.run_case(name, checker, RATIOS))
    assert "neigh1" in routes                                            # alpha != 0 has no packed-byte form
    assert shape[-1] % 4 != 0 or len(routes) == 2


def test_grid_stride_second_trip_and_ragged_last_wave(checker):
    assert 9 * 240 * 260 // 4 > 256 * 512
    for name in nr.GROUPS["big"]:
        assert nr.run_case(name, checker, RATIOS) == "neigh4-full26"


def test_force2d_row_masks(checker):
    for name in nr.GROUPS["force2d"]:
        assert nr.run_case(name, checker, RATIOS) == "neigh4-rows"


def test_route_edges_of_the_byte_kernels(checker):
    seen = {}
    for name in nr.GROUPS["route-edges"]:
        s = nr.spec(name)
        seen[(s["family"], tuple(s["distances"]), s["Ng"])] = nr.run_case(name, checker, RATIOS)
    assert seen == {("gldm", (1,), 255): "neigh4-full26", ("ngtdm", (1,), 255): "neigh4-full26",
                    ("gldm", (1,), 256): "pairs-lds32", ("ngtdm", (1,), 256): "pairs-lds64+box32",
                    ("gldm", (1, 2), 131): "neigh1", ("gldm", (1, 2), 132): "pairs-lds32",
                    ("gldm", (2,), 165): "neigh1", ("gldm", (2,), 166): "pairs-lds32",
                    ("ngtdm", (2,), 82): "neigh1", ("ngtdm", (2,), 83): "pairs-lds64"}, seen


def _dev(levels, mask):
    import torch
    return torch.from_numpy(levels).cuda(), torch.from_numpy(mask.view(np.uint8)).cuda()


@pytest.mark.parametrize("Ng", [202, 203])
def test_one_pass_gldm_ngtdm_equals_the_separate_calls(Ng, checker):
    """27 * 12 * 202 <= 65 536 < 27 * 12 * 203: the last level count at which GLDM and NGTDM share one launch (MODE 2: slot 0
    formed from the GLDM row in the flush)"""
    import torch
    from pyradiomics_amd import engine
    assert 27 * 12 * 202 <= 65536 < 27 * 12 * 203
    for shape, cont, mask in nr.BOTH_INPUTS:
        levels, m = nr.content(cont, shape, Ng), nr.roi(mask, shape)
        ang = checker.generate_angles(shape, [1], True, False, 0)
        L, M = _dev(levels, m)
        engine.timing_begin()
        try:
            g, n = engine.gldm_ngtdm(L, M, Ng)
            launches = engine.timing_count("neigh")
        finally:
            engine.timing_end()
        route = nr.expected_route("gldm", shape, Ng, ang)
        nr.check_route((shape, cont, mask), route)
        one = shape[-1] % 4 == 0 and Ng * (len(ang) + 1) * 12 <= 65536
        assert launches == (1 if one else 2), (shape, Ng, launches)
        g1, n1 = engine.gldm(L, M, Ng), engine.ngtdm(L, M, Ng)
        assert torch.equal(g, g1) and torch.equal(n, n1), (shape, cont, mask)
        assert np.array_equal(g.cpu().numpy(), checker.calculate_gldm(levels, m, [1], Ng, 0, False, 0)[0])
        want = checker.calculate_ngtdm(levels, m, [1], Ng, False, 0)[0]
        n = n.cpu().numpy()
        assert np.array_equal(n[:, (0, 2)], want[:, (0, 2)]), (shape, cont, mask)
        nr.check_s((shape, cont, mask), route + ("+gldm" if one else ""), n[:, 1], nr.accumulators(levels, m, Ng, ang)[1], len(ang), RATIOS)


@pytest.mark.parametrize("family", [0, 1], ids=["gldm", "ngtdm"])
@pytest.mark.parametrize("shape", nr.SLAB_SHAPES, ids=_tag)
def test_plane_ranges_sum_to_the_whole_volume(shape, family, checker):
    from pyradiomics_amd import engine, _lib
    Ng = 32
    ang = checker.generate_angles(shape, [1], True, False, 0)
    levels, m = nr.content("checker3", shape, Ng), nr.roi("full", shape)
    L, M = _dev(levels, m)
    variant = "neigh4-full26" if shape[-1] % 4 == 0 else "neigh1"
    ref = nr.accumulators(levels, m, Ng, ang)[family]
    whole = engine.neigh_accumulate(family, L, M, Ng, 0, shape[0]).cpu().numpy()
    assert _lib.last_variant() == variant
    assert np.array_equal(whole, ref)
    for part in nr.slab_partitions(shape[0]):
        total = np.zeros_like(ref)
        for lo, hi in part:
            acc = engine.neigh_accumulate(family, L, M, Ng, lo, hi).cpu().numpy()
            assert _lib.last_variant() == (variant if hi > lo else "none"), (part, lo, hi)
            assert np.array_equal(acc, nr.accumulators(levels, m, Ng, ang, zrange=(lo, hi))[family]), (shape, lo, hi)
            total += acc
        assert np.array_equal(total, whole), (shape, part)
    fin = engine.neigh_finalize(family, engine.neigh_accumulate(family, L, M, Ng, 0, shape[0])).cpu().numpy()
    if family == 0:
        assert np.array_equal(fin, checker.calculate_gldm(levels, m, [1], Ng, 0, False, 0)[0])
    else:
        assert np.array_equal(fin[:, (0, 2)], checker.calculate_ngtdm(levels, m, [1], Ng, False, 0)[0][:, (0, 2)])
        nr.check_s(shape, variant, fin[:, 1], ref, len(ang), RATIOS)
    # an irregular level in the halo of the range raises what the whole-volume call raises
    bad = levels.copy()
    bad[2, 1, 1] = Ng + 1
    B, _ = _dev(bad, m)
    with pytest.raises(IndexError):
        engine.neigh_accumulate(family, B, M, Ng, 0, shape[0])
    with pytest.raises(IndexError):
        engine.neigh_accumulate(family, B, M, Ng, 3, 5)          # plane 2 is halo only
    with pytest.raises(IndexError):
        (checker.calculate_ngtdm if family else checker.calculate_gldm)(bad, m, [1], Ng, *((False, 0) if family else (0, False, 0)))


@pytest.mark.parametrize("shape", [(3, 3, 260), (2, 7, 12)], ids=_tag)
def test_deferred_form_gives_the_same_bits(shape):
    import torch
    from pyradiomics_amd import engine
    Ng = 32
    levels, m = nr.content("iid", shape, Ng), nr.roi("faces", shape)
    L, M = _dev(levels, m)
    g, n = engine.gldm(L, M, Ng), engine.ngtdm(L, M, Ng)
    gd, nd = engine.gldm(L, M, Ng, deferred=True), engine.ngtdm(L, M, Ng, deferred=True)
    gb, nb = engine.gldm_ngtdm(L, M, Ng, deferred=True)
    assert engine.last_path() == "neigh" and engine.last_variant() == "neigh4-full26"
    engine.deferred_status()
    assert torch.equal(gd, g) and torch.equal(nd, n) and torch.equal(gb, g) and torch.equal(nb, n)
    bad = levels.copy()
    bad[tuple(np.argwhere(m)[-1])] = Ng + 1
    B, _ = _dev(bad, m)
    for call in (lambda: engine.gldm(B, M, Ng, deferred=True), lambda: engine.ngtdm(B, M, Ng, deferred=True),
                 lambda: engine.gldm_ngtdm(B, M, Ng, deferred=True)):
        call()
        with pytest.raises(RuntimeError):
            engine.deferred_status()
        engine.deferred_status()                                  # (reported once)
    with pytest.raises(IndexError):
        engine.gldm(B, M, Ng)


def test_zz_report():
    assert RATIOS, "no NGTDM comparison ran before the report"
    nr.report("neigh limits", RATIOS)

"""CPU: the pure planners of the LBP2D launches (csrc/prad_lbp2d_plan.h through prad_lbp2d_plan / prad_batch_lbp2d_plan): every
output voxel of every plane belongs to exactly one workgroup, for all three axes; the tile extents are powers of two (the
kernel splits a lane's output index with shifts); the staged block -- the tile plus the halo on both sides of the two in-plane
axes, float64 cells -- is what the plan reports as LDS bytes and stays within 40 KiB up to ceil(R) = 8; beyond the domain the
verdict declines.  The workgroups are decoded here as kernels_lbp2d.h decodes them: block b is tile (b / (nty ntx),
b / ntx % nty, b % ntx)."""
import numpy as np
import pytest

LDS_BUDGET = 40 * 1024


@pytest.fixture(scope="module")
def eng():
    from pyradiomics_amd import _build, engine
    _build.build()
    return engine


def _coverage(shape, plan):
    tz, ty, tx = plan["tile"]
    gz, gy, gx = plan["grid"]
    assert gz * gy * gx == plan["groups"]
    count = np.zeros(shape, dtype=np.int32)
    for b in range(plan["groups"]):
        q, ix = divmod(b, gx)
        iz, iy = divmod(q, gy)
        assert iz * tz < shape[0] and iy * ty < shape[1] and ix * tx < shape[2], "an empty workgroup"
        count[iz * tz:(iz + 1) * tz, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx] += 1
    return count


def _check_plan(plan, axis, halo):
    assert plan["verdict"] == 0
    staged = [t + (2 * halo if d != axis else 0) for d, t in enumerate(plan["tile"])]
    assert plan["lds"] == 8 * staged[0] * staged[1] * staged[2] <= LDS_BUDGET
    assert all(t >= 1 and t & (t - 1) == 0 for t in plan["tile"])


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("halo", [1, 3, 8])
def test_every_voxel_once_at_the_tile_seams(eng, axis, halo):
    """extents T - 1, T and T + 1 of the tile a large volume gets, in both plane axes, with a ragged third axis"""
    big = eng.lbp2d_plan((300, 300, 300), axis, halo)
    _check_plan(big, axis, halo)
    in_plane = [d for d in range(3) if d != axis]
    for da in (-1, 0, 1):
        for db in (-1, 0, 1):
            shape = [5, 5, 5]
            shape[in_plane[0]] = big["tile"][in_plane[0]] + da
            shape[in_plane[1]] = big["tile"][in_plane[1]] + db
            if min(shape) < 1:
                continue
            plan = eng.lbp2d_plan(shape, axis, halo)
            _check_plan(plan, axis, halo)
            assert (_coverage(tuple(shape), plan) == 1).all(), (shape, plan)
            # two tiles and a remainder along each plane axis of the tile this shape itself gets
            own = [plan["tile"][d] * 2 + 1 if d != axis else 3 for d in range(3)]
            again = eng.lbp2d_plan(own, axis, halo)
            _check_plan(again, axis, halo)
            assert (_coverage(tuple(own), again) == 1).all(), (own, again)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_extent_one_on_any_axis(eng, axis):
    for shape in [(1, 1, 1), (1, 9, 70), (9, 1, 70), (9, 70, 1), (1, 1, 130), (40, 1, 1), (1, 40, 1)]:
        for halo in (1, 8):
            plan = eng.lbp2d_plan(shape, axis, halo)
            _check_plan(plan, axis, halo)
            assert (_coverage(shape, plan) == 1).all(), (shape, plan)


def test_two_dimensional_shape_is_one_plane(eng):
    assert eng.lbp2d_plan((33, 70), 0, 1) == eng.lbp2d_plan((1, 33, 70), 0, 1)


def test_lanes_run_over_x_for_every_axis(eng):
    """a large volume gets the full 64-lane x extent within the default halo, also where x is the plane axis"""
    for axis in (0, 1, 2):
        assert eng.lbp2d_plan((256, 256, 256), axis, 1)["tile"][2] == 64


def test_declines_beyond_the_domain(eng):
    for axis in (0, 1, 2):
        assert eng.lbp2d_plan((8, 8, 8), axis, 9)["verdict"] == 1
        assert eng.lbp2d_plan((8, 8, 8), axis, -1)["verdict"] == 1
    assert eng.lbp2d_plan((2 ** 20, 2 ** 20, 1), 2, 1)["verdict"] == 2          # 2^34 tiles
    with pytest.raises(ValueError):
        eng.lbp2d_plan((8, 0, 8), 0, 1)
    with pytest.raises(ValueError):
        eng.lbp2d_plan((8, 8, 8), 3, 1)
    items, tile, lds, verdict = eng.batch_lbp2d_plan([(4, 4, 4)], 0, 9)
    assert verdict == 1 and len(items) == 0


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("halo", [1, 8])
def test_batch_items_cover_every_box_once(eng, axis, halo):
    rng = np.random.default_rng(7 + axis)
    sizes = [(1, 1, 1), (1, 1, 5), (7, 1, 1), (1, 9, 1), (3, 2, 2), (17, 33, 65), (41, 41, 41)]
    sizes += [tuple(int(v) for v in rng.integers(1, 20, 3)) for _ in range(12)]
    items, tile, lds, verdict = eng.batch_lbp2d_plan(sizes, axis, halo)
    _check_plan({"tile": tile, "lds": lds, "verdict": verdict}, axis, halo)
    counts = [np.zeros(s, dtype=np.int32) for s in sizes]
    for b, z0, y0, x0 in items:
        assert z0 % tile[0] == 0 and y0 % tile[1] == 0 and x0 % tile[2] == 0
        assert z0 < sizes[b][0] and y0 < sizes[b][1] and x0 < sizes[b][2], "an empty workgroup"
        counts[b][z0:z0 + tile[0], y0:y0 + tile[1], x0:x0 + tile[2]] += 1
    assert all((c == 1).all() for c in counts)
    assert list(items[:, 0]) == sorted(items[:, 0])          # boxes in their order


def test_batch_of_one_small_box_gets_a_small_tile(eng):
    items, tile, lds, verdict = eng.batch_lbp2d_plan([(16, 16, 16)], 0, 1)
    assert verdict == 0 and tile == (4, 16, 16) and len(items) == 4

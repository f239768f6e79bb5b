"""GPU parity at non-default map parameters and at the ray-length limit.

Every other GPU test integrates with make_params' constants (thresholds 0,
clamp [-2, 3.5], ranges [0.02, 12]).  Here the named sets of
cases.PARAM_SETS run against four shapes, one per apply path of
k_tile_accum (csrc/dm_integrate.hip): the scalar path (state_of), the
vector path (state_bits, v_med3 clamp), a heavy tile (heavy_quarter) and
sparse items.  Everything is compared exactly against the CPU oracle, and
each case asserts, on the oracle's arrays, that the state it is about
exists (a floor), so a case cannot pass for lack of it.
"""
import numpy as np
import pytest

import cases
import dm
import np_oracle
from test_gpu_parity import assert_frontiers_equal, assert_map_equal

pytestmark = pytest.mark.gpu

# W, H, resolution, S, N, colocate, last_stats key that must be non-zero
SHAPES = {
    "scalar": (130, 70, 0.05, 4, 90, 0, None),        # W % 4 != 0, ragged tiles
    "vector": (256, 192, 0.05, 6, 180, 0, None),      # whole tiles only
    "heavy": (320, 256, 0.02, 5, 720, 3, "heavy_tiles"),   # 3 x 720 co-located beams
    "sparse": (1000, 900, 0.01, 16, 12, 0, "sparse_items"),
}
N_BATCHES = 5


def batch(k, p, S, N, colocate):
    """Batches 0 and 1 come back after 2: cells cross thresholds both ways."""
    return cases.mixed_scans(70 + k % 3, p, S, N, colocate)


def touched_params(p):
    """The case's geometry and range gates with make_params' log-odds
    constants: L != 0 in a map integrated with these marks the touched cells."""
    return cases.make_params(p.width, p.height, resolution=p.resolution,
                             origin=(p.origin_x, p.origin_y), range_min=p.range_min,
                             range_max=p.range_max, band_row0=p.band_row0, band_rows=p.band_rows)


def check_floor(name, shape, om, touched, back, clusters):
    """The state each set is about, counted on the oracle's arrays."""
    L, st = om.L, om.state
    if name == "deadband":
        assert (touched & (st == -1)).sum() >= 1000 and back >= 10
    elif name == "asym":
        assert (touched & (st == -1)).sum() >= 100
    elif name == "cancel":
        if shape != "sparse":
            assert (touched & (L == 0)).sum() >= 100
    elif name == "upper_zero":
        assert (touched & (L == 0)).sum() >= 100
    elif name in ("inverted", "short"):
        assert (st == 100).sum() >= 100
    elif name == "zero_clamp":
        assert touched.sum() >= 100
        assert (L[touched] == 0).all() and (st[touched] == -1).all() and len(clusters) == 0
    elif name == "never_occ":
        assert (st == 100).sum() == 0 and (st == 0).sum() >= 100
    else:
        raise AssertionError(name)


def oracle_floor_run(oracle_lib, name, shape):
    """The five batches on the oracle alone: (om, touched, back, clusters)."""
    W, H, res, S, N, colocate, _ = SHAPES[shape]
    p = cases.set_params(name, W, H, res)
    om, tm = oracle_lib.OracleMap(p), oracle_lib.OracleMap(touched_params(p))
    back = 0
    for k in range(N_BATCHES):
        poses, ranges, amin, inc = batch(k, p, S, N, colocate)
        before = om.state.copy()
        om.integrate(poses, ranges, amin, inc)
        tm.integrate(poses, ranges, amin, inc)
        back += int(((before != -1) & (om.state == -1)).sum())
    return om, tm.L != 0, back, om.frontiers(want_mask=False, want_labels=False)[2]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", list(cases.PARAM_SETS))
def test_param_sets_vs_oracle(oracle_lib, name, shape):
    W, H, res, S, N, colocate, stat = SHAPES[shape]
    p = cases.set_params(name, W, H, res)
    om, tm = oracle_lib.OracleMap(p), oracle_lib.OracleMap(touched_params(p))
    back = 0
    with dm.OccupancyMapper(p) as m:
        for k in range(N_BATCHES):
            poses, ranges, amin, inc = batch(k, p, S, N, colocate)
            before = om.state.copy()
            exp = om.integrate(poses, ranges, amin, inc)
            tm.integrate(poses, ranges, amin, inc)
            back += int(((before != -1) & (om.state == -1)).sum())
            assert m.integrate(poses, ranges, amin, inc) == exp
            if stat:
                assert m.last_stats()[stat] >= 1
            if k == 2:  # a pass in the middle: free cells vanish after it
                np.testing.assert_array_equal(
                    m.frontiers().clusters, om.frontiers(want_mask=False, want_labels=False)[2])
        assert_map_equal(m, om)
        mask, labels, clusters = om.frontiers()
        assert_frontiers_equal(m.frontiers(want_mask=True, want_labels=True), mask, labels, clusters)
    check_floor(name, shape, om, tm.L != 0, back, clusters)


def import_image(seed, p, R, W):
    """Arbitrary floats for dm_set_logodds: normal(0, 1.5), then scattered
    cells exactly at the thresholds, at +-0, one ulp either side of each
    threshold, and outside [l_min, l_max]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = rng.normal(0.0, 1.5, (R, W)).astype(np.float32)
    f32 = np.float32
    occ_t, free_t = f32(p.occ_thresh), f32(p.free_thresh)
    special = [occ_t, free_t, f32(0.0), f32(-0.0),
               np.nextafter(occ_t, f32(np.inf)), np.nextafter(occ_t, f32(-np.inf)),
               np.nextafter(free_t, f32(np.inf)), np.nextafter(free_t, f32(-np.inf)),
               f32(p.l_max) + f32(3.75), f32(p.l_min) - f32(7.5),
               np.nextafter(f32(p.l_max), f32(np.inf)), np.nextafter(f32(p.l_min), f32(-np.inf))]
    which = rng.integers(0, 4 * len(special), (R, W))  # a quarter of the cells are special
    for i, v in enumerate(special):
        img[which == i] = v
    return img, special


@pytest.mark.parametrize("W,H", [(257, 130), (256, 128)])  # scalar / vector apply
def test_import_logodds_then_integrate(oracle_lib, W, H):
    p = cases.set_params("deadband", W, H)
    img, special = import_image(5, p, H, W)
    expect = np_oracle.state_of(p, img)
    om, tm = oracle_lib.OracleMap(p), oracle_lib.OracleMap(touched_params(p))
    om.set_logodds(img)
    np.testing.assert_array_equal(om.state, expect)  # both oracles' state-from-L
    for v in special:  # every special value is present, in each of its states
        assert (img.view(np.uint32) == v.view(np.uint32)).sum() >= 100
    assert {-1, 0, 100} == set(np.unique(expect).tolist())
    with dm.OccupancyMapper(p) as m:
        m.set_logodds(img)
        np.testing.assert_array_equal(m.state(), expect)
        np.testing.assert_array_equal(m.logodds().view(np.uint32), img.view(np.uint32))
        assert_frontiers_equal(m.frontiers(want_mask=True, want_labels=True), *om.frontiers())
        for k in range(2):
            poses, ranges, amin, inc = cases.mixed_scans(90 + k, p, 4, 90)
            tm.integrate(poses, ranges, amin, inc)
            assert m.integrate(poses, ranges, amin, inc) == om.integrate(poses, ranges, amin, inc)
        assert_map_equal(m, om)
        assert_frontiers_equal(m.frontiers(want_mask=True, want_labels=True), *om.frontiers())
        # untouched cells keep their imported bits, -0.0 and out-of-clamp values included
        un = tm.L == 0
        got = m.logodds().view(np.uint32)
        np.testing.assert_array_equal(got[un], img.view(np.uint32)[un])
        assert (un & (img.view(np.uint32) == 0x80000000)).sum() >= 10
        assert (un & ((img > np.float32(p.l_max)) | (img < np.float32(p.l_min)))).sum() >= 10
        assert 1000 <= (~un).sum()  # and the scans did touch a good part of the map


def test_sharded_handle_takes_the_parameters(oracle_lib):
    """The overrides reach the band handles of dm_create_sharded."""
    W, H, res, S, N, colocate, _ = SHAPES["vector"]
    p = cases.set_params("deadband", W, H, res)
    om, tm = oracle_lib.OracleMap(p), oracle_lib.OracleMap(touched_params(p))
    back = 0
    with dm.OccupancyMapper(p) as single, dm.OccupancyMapper(p, devices=[0, 0]) as sh:
        for k in range(N_BATCHES):
            poses, ranges, amin, inc = batch(k, p, S, N, colocate)
            before = om.state.copy()
            exp = om.integrate(poses, ranges, amin, inc)
            tm.integrate(poses, ranges, amin, inc)
            back += int(((before != -1) & (om.state == -1)).sum())
            assert single.integrate(poses, ranges, amin, inc) == exp
            assert sh.integrate(poses, ranges, amin, inc) == exp
            if k == 2:
                exp_c = om.frontiers(want_mask=False, want_labels=False)[2]
                np.testing.assert_array_equal(sh.frontiers().clusters, exp_c)
                np.testing.assert_array_equal(single.frontiers().clusters, exp_c)
        mask, labels, clusters = om.frontiers()
        for m in (single, sh):
            assert_map_equal(m, om)
            assert_frontiers_equal(m.frontiers(want_mask=True, want_labels=True), mask, labels, clusters)
    check_floor("deadband", "vector", om, tm.L != 0, back, clusters)


@pytest.mark.parametrize("major", ["x", "y"])
def test_rays_at_the_length_limit(oracle_lib, major):
    """range_max / resolution == 16384, the most validate_params admits: the
    16-bit piece packing (dm_pack_piece), the < 2^31 products of
    dm_for_each_piece and dm_udiv_small's bound at their limits; then 8 beams
    alone, which are enumerated in many k-chunks (dm_integrate_chunks)."""
    p = cases.limit_params(major)
    om = oracle_lib.OracleMap(p)
    poses, ranges, amin, inc = cases.limit_scans(p)
    cells, flags = oracle_lib.endpoints(p, poses, ranges, amin, inc)
    ok = (flags & 1) != 0
    n = np.maximum(np.abs(cells[:, 2] - cells[:, 0]), np.abs(cells[:, 3] - cells[:, 1]))[ok]
    assert n.max() == 16384  # at the limit, not near it
    with dm.OccupancyMapper(p) as m:
        for args in ((poses, ranges, amin, inc), cases.limit_chunk_scan(p)):
            exp = om.integrate(*args)
            assert exp[1] > 1000
            assert m.integrate(*args) == exp
        assert_map_equal(m, om)
        np.testing.assert_array_equal(m.frontiers().clusters,
                                      om.frontiers(want_mask=False, want_labels=False)[2])


def test_infinite_thresholds_are_accepted(oracle_lib):
    """+-inf thresholds are legal (NaN is not: tests/test_abi.py): never
    occupied, never free, always occupied."""
    for kw in (dict(occ_thresh=np.inf), dict(free_thresh=-np.inf),
               dict(occ_thresh=-np.inf, free_thresh=np.inf)):
        p = cases.make_params(128, 64, **kw)
        om = oracle_lib.OracleMap(p)
        poses, ranges, amin, inc = cases.mixed_scans(7, p, 3, 60)
        with dm.OccupancyMapper(p) as m:
            assert m.integrate(poses, ranges, amin, inc) == om.integrate(poses, ranges, amin, inc)
            assert_map_equal(m, om)
        assert len(np.unique(om.state)) == 2  # unknown and one other state

"""GPU: clearance-aware planning (dm_plan_clearance, dm_plan_field_cost and
dm_plan_path on a weighted field; csrc/dm_plan.h k_plan_clear, k_plan_relax_w)
against the host restatement dm.plan, bit for bit: no tolerances anywhere.
Maps are the smallest at which each mechanism can go wrong: a ragged last tile
row and column, discs that reach the diagonal neighbour tile and the grid's
edge, tiles no scan touched beside obstacle tiles, a field over several tiles
from sources in three of them, and a 64-cell row run whose penalties alternate
between 0 and 255 (the weighted row scan's hard case)."""
import ctypes
import os

import numpy as np
import pytest

import cases
import dm
from dm import _ffi, plan
from test_plan_cost_host import l_corridor, l_corridor_paths, least_d2_inside

pytestmark = pytest.mark.gpu

U = plan.UNREACHABLE
RADII = (1, 7, 32)


def _mapper(st):
    H, W = st.shape
    m = dm.OccupancyMapper(cases.make_params(W, H))
    m.set_state(st)
    return m


def _centre(m, cx, cy):
    p = m.params
    return (p.origin_x + (cx + 0.5) * p.resolution, p.origin_y + (cy + 0.5) * p.resolution)


def _check_field(m, st, sources, r, R, pen, max_cost=0):
    """dm_plan_field_cost against host Dijkstra; returns (field, statistics)."""
    stats = m.plan_field_cost([_centre(m, *s) for s in sources], r, R, pen, max_cost=max_cost)
    exp = plan.field_cost(st, sources, r, R, pen, max_cost)
    got = m.plan_cost_field()
    np.testing.assert_array_equal(got, exp)
    assert stats["reached"] == int((exp != U).sum())
    assert stats["traversable"] == int(plan.traversable(st, r).sum())
    return got, stats


def test_clearance_on_a_ragged_random_map():
    """136 x 200: a ragged last tile column and row; 2 % obstacles."""
    rng = np.random.default_rng(41)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(200, 136), p=[0.68, 0.30, 0.02])
    m = _mapper(st)
    try:
        for R in RADII:
            got = m.plan_clearance(R)
            assert got.dtype == np.uint16
            np.testing.assert_array_equal(got, plan.clearance(st, R))
    finally:
        m.close()


@pytest.mark.parametrize("R", RADII)
def test_clearance_of_single_obstacles(R):
    """One obstacle per case on a 192 x 192 map; the probed cell's nearest
    obstacle lies in the diagonal neighbour tile, exactly at distance R
    (d2 == R * R), one cell past it (far), and on the map's edge."""
    far = R * R + 1
    cases_ = [
        # obstacle (x, y), probe (x, y), expected d2
        ((63, 63), (64, 64), 2),             # across the junction of four tiles
        ((127, 128), (128, 127), 2),         # the other diagonal
        ((64, 100), (64 - R, 100), R * R),   # exactly R to the left, in the neighbour tile
        ((64, 100), (63 - R, 100), far),     # one cell past it
        ((100, 127), (100, 127 + R), R * R),  # exactly R below, across a tile border
        ((100, 127), (100, 128 + R), far),
        ((0, 0), (min(R, 5), 0), min(R, 5) ** 2),        # on the map's corner
        ((191, 130), (191, 130 - R), R * R),             # on the right edge
        ((70, 191), (70 + R, 191), R * R),               # on the bottom edge
    ]
    m = _mapper(np.zeros((192, 192), np.int8))
    try:
        for (ox, oy), (px, py), d2 in cases_:
            st = np.zeros((192, 192), np.int8)
            st[oy, ox] = 100
            m.set_state(st)
            got = m.plan_clearance(R)
            assert got[py, px] == d2, ((ox, oy), (px, py))
            assert got[oy, ox] == 0
            np.testing.assert_array_equal(got, plan.clearance(st, R))
    finally:
        m.close()


def test_clearance_beside_tiles_no_scan_touched():
    """One scan from the middle of tile (2, 2) of a 320 x 320 map, every range
    under 32 cells: its hits lie within a few cells of the tile's borders, and
    the eight tiles around were never touched (tile_seen == 0).  Their cells
    get their clearance from the obstacles next door all the same."""
    p = cases.make_params(320, 320)
    rng = np.random.default_rng(43)
    sx = p.origin_x + 160.5 * p.resolution
    sy = p.origin_y + 160.5 * p.resolution
    ranges = rng.uniform(1.3, 1.54, size=(1, 360)).astype(np.float32)
    m = dm.OccupancyMapper(p)
    try:
        for _ in range(3):  # enough evidence for occupied cells
            m.integrate(np.array([[sx, sy, 0.0]]), ranges, 0.0, 2 * np.pi / 360)
        st = m.state()
        inside = np.zeros(st.shape, bool)
        inside[128:192, 128:192] = True
        assert (st[~inside] == -1).all() and (st[inside] == 100).sum() > 50
        for R in RADII:
            got = m.plan_clearance(R)
            np.testing.assert_array_equal(got, plan.clearance(st, R))
        assert (got[~inside] <= 32 * 32).sum() > 1000  # R = 32 reaches well into the untouched tiles
        # and the penalty form of the kernel on the same map, through the weighted field
        pen = rng.integers(0, 256, 7 * 7 + 2).astype(np.uint8)
        src = plan.cell_of(sx, sy, p.origin_x, p.origin_y, p.resolution, 320, 320)
        m.plan_field_cost([(sx, sy)], 1, 7, pen)
        np.testing.assert_array_equal(m.plan_cost_field(), plan.field_cost(st, [src], 1, 7, pen))
    finally:
        m.close()


def test_traversable_is_a_threshold_of_the_clearance():
    rng = np.random.default_rng(47)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(200, 136), p=[0.7, 0.27, 0.03])
    m = _mapper(st)
    try:
        d2 = m.plan_clearance(32)
        for r in (0, 1, 5, 32):
            np.testing.assert_array_equal((d2 > r * r) & (st == 0), m.plan_traversable(r))
    finally:
        m.close()


def test_zero_table_is_the_unweighted_field():
    rng = np.random.default_rng(53)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(200, 136), p=[0.9, 0.05, 0.05])
    st[20, 20] = st[150, 100] = 0
    m = _mapper(st)
    try:
        srcs = [_centre(m, 20, 20), _centre(m, 100, 150)]
        for r, R in ((0, 1), (1, 9)):
            s0 = m.plan_field(srcs, inflate_cells=r)
            f0 = m.plan_cost_field()
            s1 = m.plan_field_cost(srcs, r, R, np.zeros(R * R + 2, np.uint8))
            np.testing.assert_array_equal(m.plan_cost_field(), f0)
            assert (s1["reached"], s1["traversable"]) == (s0["reached"], s0["traversable"])
            assert s0["reached"] > 10000
    finally:
        m.close()


def test_weighted_field_random_map_three_sources():
    """192 x 192, random obstacles, a random non-monotone table, sources in
    three different tiles (one on an occupied cell)."""
    rng = np.random.default_rng(59)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(192, 192), p=[0.93, 0.03, 0.04])
    sources = [(10, 12), (100, 70), (180, 170)]
    st[12, 10] = st[70, 100] = 0
    st[170, 180] = 100
    R = 5
    pen = rng.integers(0, 256, R * R + 2).astype(np.uint8)
    assert (np.diff(pen.astype(int)) > 0).any() and (np.diff(pen.astype(int)) < 0).any()
    m = _mapper(st)
    try:
        f, stats = _check_field(m, st, sources, 1, R, pen)
        assert stats["reached"] > 20000 and stats["rounds"] >= 2
        assert f[12, 10] == 0 and f[170, 180] == 0
        # the reached set is dm_plan_field's: every weight is finite
        m.plan_field([_centre(m, *s) for s in sources], inflate_cells=1)
        np.testing.assert_array_equal(m.plan_cost_field() != U, f != U)
    finally:
        m.close()


def _alternating_row():
    """A free 192 x 192 map with one 64-cell row run, y = 100, x = 64..127 (one
    tile's full width), between two combs: obstacles one cell above and below
    at even x, two cells away at odd x, so d2 alternates 1, 2, 1, 2 along the
    run and the table makes that 0, 255, 0, 255."""
    st = np.zeros((192, 192), np.int8)
    for x in range(64, 128):
        k = 1 if x % 2 == 0 else 2
        st[100 - k, x] = st[100 + k, x] = 100
    pen = np.array([0, 0, 255, 3, 9, 1], np.uint8)  # R = 2: d2 in 0, 1, 2, 4 and far = 5
    return st, pen


def test_weighted_row_scan_alternating_penalties():
    st, pen = _alternating_row()
    cp = plan.penalty(st, 2, pen)
    assert cp[100, 64:128].tolist() == [0, 255] * 32
    assert (plan.traversable(st, 0)[100, 64:128]).all()
    m = _mapper(st)
    try:
        for src in ((64, 100), (127, 100), (90, 100), (5, 5)):  # from either end, from inside, from far away
            f, _ = _check_field(m, st, [src], 0, 2, pen)
        f, _ = _check_field(m, st, [(64, 100)], 0, 2, pen)
        assert f[100, 65] == 5 * 256 and f[100, 66] == 5 * 256 + 5
    finally:
        m.close()


def test_max_cost_cuts_the_weighted_field():
    st, src, dst = l_corridor()
    pen = plan.inflation_table(0.05, 8, 0.05, 10.0)
    m = _mapper(st)
    try:
        full, _ = _check_field(m, st, [src], 1, 8, pen)
        cut = int(full[full != U].max()) // 2
        got, _ = _check_field(m, st, [src], 1, 8, pen, max_cost=cut)
        np.testing.assert_array_equal(got, np.where(full <= cut, full, U))
        assert got[got != U].max() <= cut and 0 < (got != U).sum() < (full != U).sum()
        # the cap's own bound: anything above DM_PLAN_COST_MAX means DM_PLAN_COST_MAX
        m.plan_field_cost([_centre(m, *src)], 1, 8, pen, max_cost=0xFFFFFFFF)
        np.testing.assert_array_equal(m.plan_cost_field(), full)
    finally:
        m.close()


def test_l_corridor_field_paths_and_clearance():
    """The L-shaped corridor: the weighted field, both paths against the host
    walk, and the clearance the paths keep: 6 cells (d2 36) weighted, 2 cells
    (d2 4) shortest, first and last 12 cells aside."""
    st, src, dst = l_corridor()
    t = plan.with_sources(plan.traversable(st, 1), [src])
    pen = plan.inflation_table(0.05, 8, 0.05, 10.0)
    m = _mapper(st)
    try:
        def field_of(cp):
            if cp is None:
                m.plan_field([_centre(m, *src)], inflate_cells=1)
            else:
                _check_field(m, st, [src], 1, 8, pen)
            return m.plan_cost_field()

        def path_of(f, cp):
            got = m.plan_path(_centre(m, *dst), snap_cells=0)
            assert got.tolist() == plan.path(f, t, dst[1] * 192 + dst[0], cp)
            return got

        weighted, shortest = l_corridor_paths(st, src, dst, field_of, path_of)
        assert least_d2_inside(st, weighted) == 36
        assert least_d2_inside(st, shortest) == 4
        assert (len(weighted), len(shortest)) == (272, 266)
    finally:
        m.close()


def test_weighted_paths_on_a_random_map():
    rng = np.random.default_rng(61)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(70, 130), p=[0.9, 0.03, 0.07])
    st[30, 21] = 0
    R = 4
    pen = rng.integers(0, 256, R * R + 2).astype(np.uint8)
    cp = plan.penalty(st, R, pen)
    m = _mapper(st)
    try:
        f, _ = _check_field(m, st, [(21, 30)], 1, R, pen)
        t = plan.with_sources(plan.traversable(st, 1), [(21, 30)])
        reached = np.argwhere(f != U)
        far = reached[np.argmax(f[f != U])]
        checked = 0
        for cy, cx in (far, reached[len(reached) // 2], reached[len(reached) // 3], reached[-1]):
            for snap in (0, 3):
                got = m.plan_path(_centre(m, cx, cy), snap_cells=snap)
                _, ecell = plan.snap(f, (int(cx), int(cy)), snap)
                assert got.tolist() == plan.path(f, t, ecell, cp)
                ys, xs = got // 130, got % 130
                d = np.diff(f[ys, xs].astype(np.int64))
                step = np.abs(np.diff(ys)) + np.abs(np.diff(xs))
                w = 1 + cp[ys[1:], xs[1:]].astype(np.int64)
                assert ((d == 5 * w) & (step == 1) | (d == 7 * w) & (step == 2)).all()
                checked += len(got)
        assert checked > 100
    finally:
        m.close()


def test_state_of_the_handles_field():
    """A map write makes the weighted field stale like any field; dm_plan_field
    after a weighted call brings the 5 / 7 path rule back; dm_plan_clearance
    does not touch the field."""
    st, src, dst = l_corridor()
    pen = plan.inflation_table(0.05, 8, 0.05, 10.0)
    t = plan.with_sources(plan.traversable(st, 1), [src])
    m = _mapper(st)
    try:
        m.plan_field_cost([_centre(m, *src)], 1, 8, pen)
        weighted = m.plan_path(_centre(m, *dst), snap_cells=0)
        m.plan_clearance(3)
        assert m.plan_path(_centre(m, *dst), snap_cells=0).tolist() == weighted.tolist()
        m.set_state(st)
        for call in (lambda: m.plan_query([_centre(m, *dst)]), lambda: m.plan_path(_centre(m, *dst)),
                     m.plan_cost_field):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_STATE
        m.plan_field_cost([_centre(m, *src)], 1, 8, pen)
        assert m.plan_path(_centre(m, *dst), snap_cells=0).tolist() == weighted.tolist()
        m.plan_field([_centre(m, *src)], inflate_cells=1)
        f = m.plan_cost_field()
        np.testing.assert_array_equal(f, plan.field(st, [src], 1))
        shortest = m.plan_path(_centre(m, *dst), snap_cells=0)
        assert shortest.tolist() == plan.path(f, t, dst[1] * 192 + dst[0])
        assert len(shortest) < len(weighted)
    finally:
        m.close()


def test_assign_goals_path_is_the_same_around_a_weighted_call():
    """dm_assign_goals_path before and after dm_plan_field_cost: the same
    goals bit for bit, and the field it leaves is unweighted again."""
    p, batches, amin, inc = cases.world_case(3, 400, 400, 0.05, 2, 360, 4)
    m = dm.OccupancyMapper(p)
    try:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        st = m.state()
        cl = m.frontiers().clusters
        robots = [tuple(batches[-1][0][i][:2]) for i in range(2)]
        kw = dict(min_size=4, inflate_cells=2, snap_cells=5)
        before = m.assign_goals_path(robots, **kw)
        assert any(g is not None for g in before)
        f_before = m.plan_cost_field()
        m.plan_field_cost(robots[:1], 2, 8, plan.inflation_table(p.resolution, 8, 0.05, 10.0))
        assert not np.array_equal(m.plan_cost_field(), f_before)
        after = m.assign_goals_path(robots, **kw)
        assert after == before
        assert after == plan.assign_goals_path(st, cl, robots, p.origin_x, p.origin_y, p.resolution, **kw)
        f = m.plan_cost_field()
        np.testing.assert_array_equal(f, f_before)
        goal = next(g for g in after if g is not None)
        src = plan.cell_of(*robots[-1], p.origin_x, p.origin_y, p.resolution, 400, 400)
        if f.reshape(-1)[goal[2]] != U:
            t = plan.with_sources(plan.traversable(st, 2), [src])
            assert m.plan_path(goal[1], snap_cells=0).tolist() == plan.path(f, t, goal[2])
        m.profile(True)
        m.plan_clearance(8)
        m.plan_field_cost(robots[:1], 2, 8, plan.inflation_table(p.resolution, 8, 0.05, 10.0))
        prof = m.profile_read()
        for name in ("plan_clear", "plan_travers", "plan_relax_w"):
            assert name in prof, prof
        assert "plan_relax" not in prof
    finally:
        m.close()


def test_errors():
    st = np.zeros((96, 96), np.int8)
    m = _mapper(st)
    try:
        src = [_centre(m, 10, 10)]
        m.plan_field(src, inflate_cells=0)
        for R in (0, 33, -1):
            with pytest.raises(dm.DmError) as e:
                m.plan_clearance(R)
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "clear_cells" in str(e.value)
            with pytest.raises(dm.DmError) as e:
                m.plan_field_cost(src, 0, R, np.zeros(max(R, 0) ** 2 + 2, np.uint8))
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "clear_cells" in str(e.value)
        with pytest.raises(dm.DmError) as e:
            m.plan_field_cost(src, 0, 2, None)  # a NULL table
        assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "pen" in str(e.value)
        with pytest.raises(dm.DmError) as e:
            m.plan_field_cost(src, 0, 2, np.zeros(5, np.uint8))
        assert e.value.code == _ffi.DM_ERR_INVALID_ARG
        lib = dm.load_library()
        assert lib.dm_plan_clearance(m._handle(), 2, None) == _ffi.DM_ERR_INVALID_ARG
        tab = (ctypes.c_uint8 * 6)()
        assert lib.dm_plan_field_cost(m._handle(), None, 1, 0, 2, tab, 0, None) == _ffi.DM_ERR_INVALID_ARG
        for bad in ((1e6, 0.0), (float("nan"), 0.0)):
            with pytest.raises(dm.DmError) as e:
                m.plan_field_cost([bad], 0, 2, np.zeros(6, np.uint8))
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG
        with pytest.raises(dm.DmError) as e:
            m.plan_field_cost(src, 33, 2, np.zeros(6, np.uint8))
        assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "inflate_cells" in str(e.value)
        for n in (0, 257):
            with pytest.raises(dm.DmError):
                m.plan_field_cost(np.zeros((n, 2)), 0, 2, np.zeros(6, np.uint8))
    finally:
        m.close()


def test_band_and_sharded_handles_are_refused():
    tab = np.zeros(6, np.uint8)
    m = dm.OccupancyMapper(cases.make_params(128, 128, band_row0=0, band_rows=64))
    try:
        for call in (lambda: m.plan_clearance(2), lambda: m.plan_field_cost([(0.0, 0.0)], 0, 2, tab)):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "whole map" in str(e.value)
    finally:
        m.close()
    m = dm.OccupancyMapper(cases.make_params(128, 128), devices=[0, 0])
    try:
        for call in (lambda: m.plan_clearance(2), lambda: m.plan_field_cost([(0.0, 0.0)], 0, 2, tab)):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "sharded" in str(e.value)
    finally:
        m.close()


def test_round_bound_leaves_no_field():
    """DM_PLAN_MAX_ROUNDS = 2 (read at dm_create): the corridor's weighted
    field needs more rounds, so the call ends with DM_ERR_INCOMPLETE and the
    handle has no field."""
    st, src, dst = l_corridor()
    pen = plan.inflation_table(0.05, 8, 0.05, 10.0)
    os.environ["DM_PLAN_MAX_ROUNDS"] = "2"
    try:
        m = _mapper(st)
    finally:
        del os.environ["DM_PLAN_MAX_ROUNDS"]
    try:
        with pytest.raises(dm.DmError) as e:
            m.plan_field_cost([_centre(m, *src)], 1, 8, pen)
        assert e.value.code == _ffi.DM_ERR_INCOMPLETE
        for call in (m.plan_cost_field, lambda: m.plan_path(_centre(m, *dst))):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_STATE
    finally:
        m.close()

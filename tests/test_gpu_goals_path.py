"""GPU: frontier goals scored by path length (dm_assign_goals_path) against
the host restatement dm.plan.assign_goals_path on the same map and cluster
list: chosen indices, snapped cells and goal coordinates equal, bit for bit;
and the two situations the straight-line policy gets wrong, a nearer cluster
behind a wall and a cluster that cannot be reached at all."""
import numpy as np
import pytest

import cases
import dm
from dm import _ffi, plan
from dm.goals import assign_goals

pytestmark = pytest.mark.gpu


def _check(m, st, clusters, robots, cache, **kw):
    p = m.params
    got = m.assign_goals_path(robots, **kw)
    exp = plan.assign_goals_path(st, clusters, robots, p.origin_x, p.origin_y, p.resolution, cache=cache, **kw)
    assert len(got) == len(exp) == len(robots)
    for g, e in zip(got, exp):
        if e is None:
            assert g is None
        else:
            assert g is not None and g[0] == e[0] and g[2] == e[2]
            assert g[1] == e[1]  # the same doubles
    return got


def test_goals_by_path_on_mapped_world():
    p, batches, amin, inc = cases.world_case(51, 512, 512, 0.05, 4, 720, 3, region_frac=0.7)
    m = dm.OccupancyMapper(p)
    try:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        cl = m.frontiers().clusters
        st = m.state()
        assert len(cl) > 10
        # the robots' own poses: 8 places inside the mapped region
        robots = np.concatenate([batches[-1][0][:, :2], batches[0][0][:, :2]])[:8]
        cache = {}
        some = 0
        for R in (1, 8):
            for kw in (dict(min_size=8), dict(min_size=1, distance_weight=0.25, min_distance=1.0)):
                got = _check(m, st, cl, robots[:R], cache, inflate_cells=2, snap_cells=5, **kw)
                some += sum(g is not None for g in got)
        assert some > 0
        # the field left behind is the last robot's
        last = plan.cell_of(robots[7][0], robots[7][1], p.origin_x, p.origin_y, p.resolution, 512, 512)
        np.testing.assert_array_equal(m.plan_cost_field(), cache[last])
        # dm_assign_goals itself is unchanged by all this
        eu = m.assign_goals(robots, min_size=8)
        assert [g and g[0] for g in eu] == [g and g[0] for g in assign_goals(cl, robots, min_size=8)]
    finally:
        m.close()


def _walled_map(gap: bool):
    """A walled room (free x, y in [10, 60) x [10, 100), occupied ring) with
    the robot inside; a free pocket behind its right wall whose outer cells
    are the near frontier; with `gap`, an opening in the left wall whose
    cells are the far frontier."""
    st = np.full((128, 128), -1, np.int8)
    st[9:101, 9:61] = 100
    st[10:100, 10:60] = 0
    st[45:55, 61:66] = 0       # the pocket behind the wall at x = 60
    if gap:
        st[80:90, 9] = 0       # the opening: free cells facing unknown at x = 8
    return st


def test_cluster_behind_a_wall_loses_to_a_reachable_one():
    st = _walled_map(gap=True)
    m = dm.OccupancyMapper(cases.make_params(128, 128))
    try:
        m.set_state(st)
        cl = m.frontiers().clusters
        p = m.params
        robot = (p.origin_x + 55.5 * p.resolution, p.origin_y + 50.5 * p.resolution)
        cx = np.floor((cl["cx_m"] - p.origin_x) / p.resolution)
        assert (cx > 60).sum() >= 1 and (cx < 12).sum() >= 1
        eu = m.assign_goals([robot], min_size=1)[0]
        assert cx[eu[0]] > 60  # straight-line: the pocket just behind the wall
        got = _check(m, st, cl, [robot], {}, min_size=1, inflate_cells=1, snap_cells=3)[0]
        assert got is not None and cx[got[0]] < 12  # by path: the opening
        assert plan.traversable(st, 1).reshape(-1)[got[2]]
        path = m.plan_path(got[1], snap_cells=0)
        assert path[0] == 50 * 128 + 55 and path[-1] == got[2]
    finally:
        m.close()


def test_sealed_off_cluster_is_no_goal():
    st = _walled_map(gap=False)
    m = dm.OccupancyMapper(cases.make_params(128, 128))
    try:
        m.set_state(st)
        cl = m.frontiers().clusters
        p = m.params
        robot = (p.origin_x + 55.5 * p.resolution, p.origin_y + 50.5 * p.resolution)
        assert len(cl) >= 1
        assert m.assign_goals([robot], min_size=1)[0] is not None
        assert _check(m, st, cl, [robot], {}, min_size=1, inflate_cells=1, snap_cells=3) == [None]
    finally:
        m.close()


def test_goals_by_path_errors():
    m = dm.OccupancyMapper(cases.make_params(128, 128))
    try:
        with pytest.raises(dm.DmError):  # no collected result, as dm_assign_goals
            m.assign_goals_path([(0.0, 0.0)])
        m.frontiers()
        assert m.assign_goals_path([(0.0, 0.0), (1.0, 1.0)]) == [None, None]
        for bad in (dict(distance_weight=-1.0), dict(inflate_cells=33), dict(snap_cells=17)):
            with pytest.raises(dm.DmError) as e:
                m.assign_goals_path([(0.0, 0.0)], **bad)
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG
        with pytest.raises(dm.DmError):
            m.assign_goals_path(np.zeros((257, 2)))
        with pytest.raises(dm.DmError):
            m.assign_goals_path([(0.0, 0.0), (1e6, 0.0)])  # a robot outside the grid
    finally:
        m.close()

"""CPU: the host restatement of the overlap-aware gain calls (dm/gain.py:
visible_set, gain_views_joint, assign_goals_coord; include/dm.h, DESIGN.md
§9.4): the visible set against a scalar, set-based loop written from the dm.h
definition, the properties of the joint marginals, the policy case the calls
are for with its exact numbers, the errors, and the node's two settings."""
import numpy as np
import pytest

import cases
import dm
import np_oracle
from dm import gain
from dm.ros_node import SlamParams


def _scalar_visible(st, vx, vy, R):
    """The marked cells of dm.h's definition: one ray and one step at a time."""
    H, W = st.shape
    marked = set()
    offsets = [(ex, ey) for ex in range(-R, R + 1) for ey in range(-R, R + 1) if max(abs(ex), abs(ey)) == R]
    assert len(offsets) == 8 * R
    for ex, ey in offsets:
        xmajor = abs(ex) >= abs(ey)
        adb = min(abs(ex), abs(ey))
        sa = (ex > 0) - (ex < 0) if xmajor else (ey > 0) - (ey < 0)   # sign of the major offset
        sb = (ey > 0) - (ey < 0) if xmajor else (ex > 0) - (ex < 0)   # and of the minor one
        for k in range(R + 1):
            major, minor = k * sa, sb * ((2 * k * adb + R) // (2 * R))
            dx, dy = (major, minor) if xmajor else (minor, major)
            x, y = vx + dx, vy + dy
            if not (0 <= x < W and 0 <= y < H) or dx * dx + dy * dy > R * R or st[y, x] == 100:
                break
            if st[y, x] != 0:
                marked.add((x, y))
    return marked


def test_visible_set_against_the_scalar_definition():
    st = cases.random_state(4, 80, 96, p_free=0.5, p_occ=0.04)
    H, W = st.shape
    assert (H, W) == (80, 96)
    occ = np.argwhere(st == 100)[3]
    views = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (0, 41), (W - 1, 17), (50, 0), (33, H - 1), (48, 40),
             (int(occ[1]), int(occ[0]))]
    for R in (1, 7, 16):
        for vx, vy in views:
            V = gain.visible_set(st, (vx, vy), R)
            assert V.shape == st.shape and V.dtype == bool
            exp = _scalar_visible(st, vx, vy, R)
            assert {(int(x), int(y)) for y, x in np.argwhere(V)} == exp, (R, vx, vy)
            assert gain.visible_unknown(st, (vx, vy), R) == len(exp) == int(V.sum())
        assert not gain.visible_set(st, (int(occ[1]), int(occ[0])), R).any()  # k = 0 is the occupied view cell
    assert sum(len(_scalar_visible(st, vx, vy, 16)) for vx, vy in views) > 1000


def _centre(x, y, res=0.05, o=0.0):
    return (o + (x + 0.5) * res, o + (y + 0.5) * res)


def test_joint_properties():
    st = cases.random_state(9, 90, 120, p_free=0.5, p_occ=0.03)
    H, W = st.shape
    a = (0.0, 0.0, 0.05)
    cells = [(20, 20), (28, 24), (60, 50), (20, 20), (100, 80), (64, 52), (0, 0)]
    views = [_centre(x, y) for x, y in cells] + [(1e9, 0.0), (float("nan"), 1.0), (1.0, float("inf"))]
    m, c, claimed = gain.gain_views_joint(st, views, *a, 12)
    assert m.dtype == np.uint32 and c.dtype == np.int64 and claimed.dtype == bool and claimed.shape == st.shape
    assert m[3] == 0 and m[0] > 0                         # a repeated view adds nothing
    assert list(c[-3:]) == [-1, -1, -1] and list(m[-3:]) == [0, 0, 0]
    assert [int(v) for v in c[:7]] == [y * W + x for x, y in cells]
    assert int(m.sum()) == int(claimed.sum()) > 500
    # the first view's marginal is its gain; a later overlapping one is below its gain
    g, _ = gain.gain_views(st, views, *a, 12)
    assert m[0] == g[0] and m[1] < g[1] and np.all(m <= g)
    union = np.zeros_like(claimed)
    for x, y in cells:
        union |= gain.visible_set(st, (x, y), 12)
    np.testing.assert_array_equal(claimed, union)
    # another order: other marginals, the same claimed set
    perm = [5, 2, 9, 1, 0, 7, 4, 3, 6, 8]
    m2, c2, claimed2 = gain.gain_views_joint(st, [views[i] for i in perm], *a, 12)
    np.testing.assert_array_equal(claimed2, claimed)
    np.testing.assert_array_equal(c2, c[perm])
    assert int(m2.sum()) == int(m.sum()) and not np.array_equal(m2, m[perm])
    # no views: an empty claimed set
    m0, c0, cl0 = gain.gain_views_joint(st, np.zeros((0, 2)), *a, 12)
    assert m0.shape == (0,) and c0.shape == (0,) and not cl0.any()


def policy_case():
    """Two doorways (A, B) onto one unknown hall and a third (C) elsewhere."""
    st = np.full((128, 128), -1, np.int8)
    st[9:101, 9:61] = 100
    st[10:100, 10:60] = 0
    st[30:34, 60] = 0     # doorway A, right wall
    st[40:44, 60] = 0     # doorway B, right wall, same unknown hall as A
    st[84:88, 9] = 0      # doorway C, left wall
    return st


POLICY_KW = dict(min_size=1, inflate_cells=1, snap_cells=3, radius_cells=40)


def test_policy_case_exact_numbers():
    st = policy_case()
    p = cases.make_params(128, 128, min_frontier_size=1)
    cl = np.array(np_oracle.frontiers(p, st)[2], dtype=np.dtype(dm.CLUSTER_DTYPE))
    assert len(cl) == 3 and list(cl["size"]) == [4, 4, 4]
    a = (p.origin_x, p.origin_y, p.resolution)
    ctr = lambda x, y: (p.origin_x + (x + 0.5) * p.resolution, p.origin_y + (y + 0.5) * p.resolution)
    robots = [ctr(35, 50), ctr(35, 52)]
    cache = {}
    unc = gain.assign_goals_gain(st, cl, robots, *a, cache=cache, **POLICY_KW)
    assert [g[0] for g in unc] == [1, 0] and [g[3] for g in unc] == [2211, 2134]
    assert [g[2] for g in unc] == [42 * 128 + 60, 32 * 128 + 60]
    both = gain.visible_set(st, (60, 42), 40) | gain.visible_set(st, (60, 32), 40)
    assert int(both.sum()) == 2525 and 2134 - (2211 + 2134 - 2525) == 314
    co, claimed = gain.assign_goals_coord(st, cl, robots, *a, cache=cache, return_claimed=True, **POLICY_KW)
    assert [g[0] for g in co] == [1, 2] and [g[3] for g in co] == [2211, 448]
    assert [g[2] for g in co] == [42 * 128 + 60, 85 * 128 + 9]
    assert co[0] == unc[0] and co[1][1] == ctr(9, 85)
    assert int(claimed.sum()) == 2659
    # robot 1 alone, robot 0's goal held by a teammate
    alone, cl1 = gain.assign_goals_coord(st, cl, robots[1:], *a, held_xy=[ctr(60, 42)], cache=cache,
                                         return_claimed=True, **POLICY_KW)
    assert alone[0][0] == 2 and alone[0][3] == 448 and alone[0][2] == 85 * 128 + 9
    np.testing.assert_array_equal(cl1, claimed)
    # one robot, nothing held: assign_goals_gain
    for r in robots:
        assert gain.assign_goals_coord(st, cl, [r], *a, **POLICY_KW) == gain.assign_goals_gain(st, cl, [r], *a,
                                                                                             **POLICY_KW)
    # without return_claimed: the list alone; a held view outside the grid or non-finite adds nothing
    assert gain.assign_goals_coord(st, cl, robots, *a, held_xy=[(1e9, 0.0), (float("nan"), 0.0)], **POLICY_KW) == co
    # no clusters: nobody gets a goal, the held views are claimed
    none, cl2 = gain.assign_goals_coord(st, cl[:0], robots, *a, held_xy=[ctr(60, 42)], return_claimed=True,
                                        **POLICY_KW)
    assert none == [None, None] and int(cl2.sum()) == 2211


def test_errors():
    st = np.full((32, 32), -1, np.int8)
    a = (0.0, 0.0, 0.05)
    cl = np.zeros(0, dtype=np.dtype(dm.CLUSTER_DTYPE))
    ok = [(0.1, 0.1)]
    with pytest.raises(ValueError):
        gain.assign_goals_coord(st, cl, ok, *a, min_gain=-1)
    with pytest.raises(ValueError):
        gain.assign_goals_coord(st, cl, ok, *a, distance_weight=-0.5)
    with pytest.raises(ValueError):
        gain.assign_goals_coord(st, cl, ok, *a, distance_weight=float("nan"))
    for R in (0, 512):
        with pytest.raises(ValueError):
            gain.assign_goals_coord(st, cl, ok, *a, radius_cells=R)
        with pytest.raises(ValueError):
            gain.gain_views_joint(st, ok, *a, R)
        with pytest.raises(ValueError):
            gain.visible_set(st, (3, 3), R)
    with pytest.raises(ValueError):
        gain.assign_goals_coord(st, cl, [(0.1, 0.1), (99.0, 0.1)], *a, radius_cells=4)
    with pytest.raises(ValueError):
        gain.gain_views_joint(st, np.zeros((1025, 2)), *a, 4)
    with pytest.raises(ValueError):
        gain.assign_goals_coord(st, cl, ok, *a, radius_cells=4, held_xy=np.zeros((1025, 2)))
    m, _, claimed = gain.gain_views_joint(st, np.full((1024, 2), 0.8), *a, 4)  # the limit itself is admitted
    assert m[0] == 49 and not m[1:].any() and int(claimed.sum()) == 49  # the disc of radius 4
    assert gain.assign_goals_coord(st, cl, ok, *a, radius_cells=4, held_xy=np.zeros((1024, 2))) == [None]


def test_node_settings():
    d = SlamParams()
    assert d.dm_goal_coordinate is False and d.dm_peer_goals_topic == "/peer_goals"
    s = SlamParams.from_dict({"dm_goal_coordinate": True, "dm_peer_goals_topic": "/team/goals", "unknown_key": 1})
    assert s.dm_goal_coordinate is True and s.dm_peer_goals_topic == "/team/goals"
    assert s.dm_goal_information_gain is False  # implied by the node, not rewritten in the settings

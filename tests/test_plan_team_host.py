"""CPU: the host restatement of team planning (dm.plan.team_fields,
global_greedy, assign_goals_team; include/dm.h): the fields are
plan.field per robot, one robot is assign_goals_path, the global-greedy pick
equals a literal sort of all pairs, and the two fixtures of
tests/team_cases.py have the properties the GPU test relies on."""
import numpy as np
import pytest

import cases
import dm
import team_cases
from dm import gain, plan

U = plan.UNREACHABLE


def test_library_exports_the_team_entry_points():
    lib = dm.load_library()
    for name in ("dm_plan_team", "dm_plan_team_get_field", "dm_plan_team_query", "dm_plan_team_path",
                 "dm_assign_goals_team"):
        assert hasattr(lib, name), name
    assert dm._ffi.DM_PLAN_TEAM_MAX == plan.TEAM_MAX == 64


def test_team_fields_are_single_fields():
    rng = np.random.default_rng(5)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(40, 70), p=[0.7, 0.1, 0.2])
    st[20, 30] = -1   # a robot on an unknown cell
    st[10, 10] = 100  # and one on an occupied cell
    cells = [(30, 20), (10, 10), (5, 33), (30, 20)]
    st[33, 5] = 0
    for r, max_cost in ((0, 0), (1, 0), (1, 120)):
        got = plan.team_fields(st, cells, r, max_cost)
        assert len(got) == 4
        for f, c in zip(got, cells):
            np.testing.assert_array_equal(f, plan.field(st, [c], r, max_cost))
            assert f[c[1], c[0]] == 0
        # a robot's cell is a source in its own field only
        assert got[2][20, 30] == U and got[2][10, 10] == U
    with pytest.raises(ValueError):
        plan.team_fields(st, [], 0)
    with pytest.raises(ValueError):
        plan.team_fields(st, [(1, 1)] * 65, 0)


def _sort_all_pairs(util, labels):
    """The definition, literally: every eligible pair sorted by (util
    descending, label, robot), taken in that order when both are still free."""
    R, K = util.shape
    pairs = sorted((-util[r, c], labels[c], r, c) for r in range(R) for c in range(K) if np.isfinite(util[r, c]))
    out = [-1] * R
    taken = set()
    for _, _, r, c in pairs:
        if out[r] < 0 and c not in taken:
            out[r] = c
            taken.add(c)
    return out


@pytest.mark.parametrize("seed", range(12))
def test_global_greedy_equals_sorting_all_pairs(seed):
    rng = np.random.default_rng(seed)
    R, K = int(rng.integers(1, 7)), int(rng.integers(1, 9))
    util = rng.integers(1, 5, size=(R, K)).astype(np.float64)  # few values: many ties
    util[rng.random((R, K)) < 0.3] = -np.inf
    labels = np.sort(rng.choice(1000, size=K, replace=False))
    got = plan.global_greedy(util, labels)
    assert got == _sort_all_pairs(util, labels)
    done = [c for c in got if c >= 0]
    assert len(set(done)) == len(done)
    assert plan.global_greedy(np.full((2, 3), -np.inf), np.arange(3)) == [-1, -1]


def _world_clusters():
    rng = np.random.default_rng(7)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(70, 130), p=[0.9, 0.07, 0.03])
    p = cases.make_params(130, 70)
    return p, st, team_cases.clusters_of(p, st)


def test_one_robot_is_assign_goals_path_and_gain():
    p, st, cl = _world_clusters()
    assert len(cl) > 5
    free = np.argwhere(st == 0)
    args = (p.origin_x, p.origin_y, p.resolution)
    some = 0
    for k in (3, 40, 200):
        robot = [team_cases.centre(p, int(free[k][1]), int(free[k][0]))]
        kw = dict(min_size=2, distance_weight=0.5, min_distance=0.2, inflate_cells=1, snap_cells=3)
        got = plan.assign_goals_team(st, cl, robot, *args, **kw)
        assert got == plan.assign_goals_path(st, cl, robot, *args, **kw)
        gg = plan.assign_goals_team(st, cl, robot, *args, min_gain=2, radius_cells=12, **kw)
        assert gg == gain.assign_goals_gain(st, cl, robot, *args, min_gain=2, radius_cells=12, **kw)
        some += (got[0] is not None) + (gg[0] is not None)
    assert some > 0
    assert plan.assign_goals_team(st, cl, [], *args) == []
    assert plan.assign_goals_team(st, cl[:0], [team_cases.centre(p, 1, 1)], *args) == [None]


def test_order_matters_fixture():
    """Robots in order: 0 takes A and 1 is sent to B.  The best pair first:
    1 takes A, which it stands beside, and 0 goes to B."""
    st, robots, A, B = team_cases.order_matters()
    p = cases.make_params(192, 64)
    cl = team_cases.clusters_of(p, st)
    assert len(cl) == 2 and cl["size"].tolist() == [10, 10]
    assert (cl["sum_x"][A], cl["sum_x"][B]) == (sum(range(95, 105)), sum(range(15, 25)))
    xy = [team_cases.centre(p, *c) for c in robots]
    args = (p.origin_x, p.origin_y, p.resolution)
    by_path = plan.assign_goals_path(st, cl, xy, *args, **team_cases.KW)
    team = plan.assign_goals_team(st, cl, xy, *args, **team_cases.KW)
    assert [g[0] for g in by_path] == [A, B]
    assert [g[0] for g in team] == [B, A]
    assert team != by_path
    # swapping the robots swaps the team's result and nothing else
    swapped = plan.assign_goals_team(st, cl, xy[::-1], *args, **team_cases.KW)
    assert swapped == team[::-1]
    f = plan.team_fields(st, robots, 0)
    cost = lambda r, g: int(f[r].reshape(-1)[g[2]])
    # 1 is beside A, 0 a little farther from A and much farther from B
    assert cost(1, team[1]) < cost(0, by_path[0]) < cost(1, by_path[1]) < cost(0, team[0])


def test_tie_fixture():
    """Equal utils: the smaller label first, then the smaller robot."""
    st, P, Q, X, Y = team_cases.ties()
    p = cases.make_params(192, 64)
    cl = team_cases.clusters_of(p, st)
    assert len(cl) == 2 and cl["size"].tolist() == [9, 9] and cl["label"][X] < cl["label"][Y]
    f = plan.team_fields(st, [P, Q], 0)
    assert f[0][28, 96] == f[0][36, 56] == f[1][28, 96] == 4 * 7 + 16 * 5
    args = (p.origin_x, p.origin_y, p.resolution)
    for robots, exp in (([P, Q], [X, Y]), ([Q, P], [X, Y])):
        got = plan.assign_goals_team(st, cl, [team_cases.centre(p, *c) for c in robots], *args, **team_cases.KW)
        assert [g[0] for g in got] == exp
        assert got[0][2] == 28 * 192 + 96 and got[1][2] == 36 * 192 + 56

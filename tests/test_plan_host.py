"""CPU: the host restatement of the path planner (dm/plan.py, the reference
of the GPU tests) checked against independent brute-force forms, and the
library's six planning entry points are exported."""
import numpy as np
import pytest

import dm
from dm import plan

U = plan.UNREACHABLE


def _random_state(seed, H, W):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, -1, 100], np.int8), size=(H, W), p=[0.7, 0.1, 0.2])


def _sweep_field(trav, sources, max_cost=plan.MAX_COST):
    """Min-relaxation over the whole array, repeated until stable: no graph,
    no priority queue, nothing shared with dm.plan.field."""
    H, W = trav.shape
    cost = np.full((H, W), U, np.uint64)
    for cx, cy in sources:
        cost[cy, cx] = 0
    changed = True
    while changed:
        changed = False
        for y in range(H):
            for x in range(W):
                if not trav[y, x]:
                    continue
                best = cost[y, x]
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ny, nx = y + dy, x + dx
                        if (dy == 0 and dx == 0) or not (0 <= ny < H and 0 <= nx < W):
                            continue
                        if cost[ny, nx] == U:
                            continue
                        if dy and dx and not (trav[ny, x] and trav[y, nx]):
                            continue
                        c = cost[ny, nx] + (7 if dy and dx else 5)
                        if c < best and c <= max_cost:
                            best = c
                if best < cost[y, x]:
                    cost[y, x] = best
                    changed = True
    return cost.astype(np.uint32)


@pytest.mark.parametrize("seed,H,W,r", [(1, 24, 31, 0), (2, 33, 20, 1), (3, 48, 48, 2)])
def test_field_matches_fixed_point_sweep(seed, H, W, r):
    st = _random_state(seed, H, W)
    rng = np.random.default_rng(seed + 100)
    sources = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(3)]
    trav = plan.with_sources(plan.traversable(st, r), sources)
    got = plan.field(st, sources, r)
    np.testing.assert_array_equal(got, _sweep_field(trav, sources))
    assert (got != U).sum() >= len(set(sources))
    # max_cost: exactly the cells within it stay
    capped = plan.field(st, sources, r, max_cost=40)
    np.testing.assert_array_equal(capped, np.where(got <= 40, got, U))


@pytest.mark.parametrize("r", [0, 1, 3, 5])
def test_traversable_matches_disc_test(r):
    st = _random_state(7 + r, 29, 37)
    H, W = st.shape
    exp = np.zeros((H, W), bool)
    occ = [(x, y) for y in range(H) for x in range(W) if st[y, x] == 100]
    for y in range(H):
        for x in range(W):
            exp[y, x] = st[y, x] == 0 and not any((x - ox) ** 2 + (y - oy) ** 2 <= r * r for ox, oy in occ)
    np.testing.assert_array_equal(plan.traversable(st, r), exp)


@pytest.mark.parametrize("sx,sy", [(1, 1), (-1, 1), (1, -1), (-1, -1)])
def test_no_corner_cutting(sx, sy):
    """Source at the centre, one occupied cell beside it: the diagonal past
    that cell costs two orthogonal moves (10), the free diagonal 7."""
    st = np.zeros((5, 5), np.int8)
    st[2, 2 + sx] = 100  # blocks the diagonals (sx, +-1)
    f = plan.field(st, [(2, 2)], 0)
    assert f[2, 2] == 0 and f[2, 2 + sx] == U
    assert f[2 + sy, 2 + sx] == 10   # around: (0, sy) then (sx, 0)
    assert f[2 - sy, 2 + sx] == 10
    assert f[2 + sy, 2 - sx] == 7    # the other side is open
    assert f[2 + sy, 2] == 5
    # the cell behind the obstacle: both diagonals next to it pass the
    # obstacle's corner, so the way round is four orthogonal moves
    assert f[2, 2 + 2 * sx] == 20


def test_sources_are_traversable_whatever_their_state():
    st = np.zeros((6, 6), np.int8)
    st[1, 1] = -1
    st[4, 4] = 100
    f = plan.field(st, [(1, 1), (4, 4)], 1)
    assert f[1, 1] == 0 and f[4, 4] == 0
    assert f[1, 2] == 5      # out of the unknown source
    assert f[4, 3] == U      # inflated by the occupied source cell itself
    with pytest.raises(ValueError):
        plan.field(st, [(6, 0)], 0)


def test_snap_tie_breaks():
    f = np.full((7, 7), U, np.uint32)
    f[3, 1] = 50  # distance^2 4, index 22
    f[1, 3] = 60  # distance^2 4, index 10: the smaller index wins
    f[5, 5] = 1   # distance^2 8: farther, whatever its cost
    assert plan.snap(f, (3, 3), 2) == (60, 10)
    assert plan.snap(f, (3, 3), 1) == (U, -1)
    assert plan.snap(f, None, 5) == (U, -1)
    f[3, 3] = 9
    assert plan.snap(f, (3, 3), 2) == (9, 24)
    assert plan.snap(f, (0, 0), 1) == (U, -1)  # the window is clipped to the grid


def test_path_predecessor_order():
    """Open 3x3, source in the middle of the top row: the corner (2, 2) has
    cost 12 over two predecessors, (1, 1) by a diagonal (5 + 7) and (2, 1) by
    an orthogonal move (7 + 5); (dy, dx) = (-1, -1) comes first."""
    st = np.zeros((3, 3), np.int8)
    f = plan.field(st, [(1, 0)], 0)
    assert f[2, 2] == 12 and f[1, 1] == 5 and f[1, 2] == 7
    t = plan.with_sources(plan.traversable(st, 0), [(1, 0)])
    assert plan.path(f, t, 8) == [1, 4, 8]
    assert plan.path(f, t, 1) == [1]
    assert plan.path(f, t, -1) == []
    # occupy (2, 0): the diagonal (1, 0) -> (2, 1) would cut its corner, so
    # (2, 1) is reached over (1, 1) with two orthogonal moves
    st[0, 2] = 100
    f = plan.field(st, [(1, 0)], 0)
    t = plan.with_sources(plan.traversable(st, 0), [(1, 0)])
    assert f[1, 2] == 10
    assert plan.path(f, t, 5) == [1, 4, 5]


def test_assign_goals_path_prefers_the_reachable_cluster():
    st = np.zeros((20, 20), np.int8)
    st[:, 10] = 100  # a wall: the right half is sealed off
    cl = np.zeros(2, dtype=np.dtype(dm._ffi.CLUSTER_DTYPE))
    cl["label"], cl["size"] = [5, 9], [10, 10]
    cl["cx_m"], cl["cy_m"] = [12.5, 2.5], [5.5, 5.5]  # resolution 1, origin 0
    got = plan.assign_goals_path(st, cl, [(8.5, 5.5)], 0.0, 0.0, 1.0, min_size=1, inflate_cells=0, snap_cells=1)
    assert got[0][0] == 1 and got[0][2] == 5 * 20 + 2 and got[0][1] == (2.5, 5.5)
    from dm.goals import assign_goals
    assert assign_goals(cl, [(8.5, 5.5)], min_size=1)[0][0] == 0  # straight-line: through the wall


def test_library_exports_the_planning_entry_points():
    lib = dm.load_library()
    for name in ("dm_plan_traversable", "dm_plan_field", "dm_plan_get_field", "dm_plan_query", "dm_plan_path",
                 "dm_assign_goals_path"):
        assert hasattr(lib, name), name


def test_ros_goal_settings_in_cells():
    from dm.ros_node import SlamParams

    s = SlamParams()
    assert s.dm_goal_path_distance is False
    assert s.goal_cells() == (2, 5)  # ceil(0.10 / 0.05), ceil(0.25 / 0.05)
    s = SlamParams(resolution=0.01, dm_goal_inflate_m=1.0, dm_goal_snap_m=1.0)
    assert s.goal_cells() == (32, 16)  # clamped to the C-ABI's limits
    s = SlamParams.from_dict({"dm_goal_path_distance": True, "dm_goal_inflate_m": 0.12})
    assert s.dm_goal_path_distance is True and s.goal_cells() == (3, 5)

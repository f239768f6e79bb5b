"""GPU: team planning (dm_plan_team*, dm_assign_goals_team; csrc/dm_plan.h §4)
against the host restatement dm.plan, bit for bit: every robot's layer is the
single field from that robot alone, a robot's own cell is a source in its own
layer only (inside a tile, in the middle of a row scan, and seen through the
ring of the neighbouring tiles), fields that settle at different times, the
limits, the robot x target matrix and the paths, the lifetime rules beside the
single field, and the global-greedy goals on the fixtures of team_cases.py."""
import os

import numpy as np
import pytest

import cases
import dm
import team_cases
from dm import _ffi, gain, plan

pytestmark = pytest.mark.gpu

U = plan.UNREACHABLE


def _mapper(st):
    H, W = st.shape
    m = dm.OccupancyMapper(cases.make_params(W, H))
    m.set_state(st)
    return m


def _centre(m, cx, cy):
    return team_cases.centre(m.params, cx, cy)


def _random_state(seed, H, W):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, -1, 100], np.int8), size=(H, W), p=[0.65, 0.10, 0.25])


def _code(fn):
    with pytest.raises(dm.DmError) as e:
        fn()
    return e.value.code


def _check_layers(m, st, cells, r, max_cost=0):
    """plan_team of the cells; every layer against plan.field.  Returns (stats, expected layers)."""
    stats = m.plan_team([_centre(m, *c) for c in cells], inflate_cells=r, max_cost=max_cost)
    exp = plan.team_fields(st, cells, r, max_cost)
    for k, e in enumerate(exp):
        np.testing.assert_array_equal(m.plan_team_field(k), e, err_msg=f"layer {k} of {cells}")
    assert stats["reached"] == [int((e != U).sum()) for e in exp]
    assert stats["traversable"] == int(plan.traversable(st, r).sum())
    return stats, exp


# ---- 1. random maps ---------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (70, 130)])
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_maps(H, W, seed):
    """One tile, and 130 x 70: a ragged last tile column and row."""
    st = _random_state(seed, H, W)
    rng = np.random.default_rng(seed + 50)
    free = np.argwhere(st == 0)
    m = _mapper(st)
    try:
        for r in (0, 1, 3):
            cells = [(int(cx), int(cy)) for cy, cx in free[rng.choice(len(free), 3, replace=False)]]
            _, exp = _check_layers(m, st, cells, r)
            for k, c in enumerate(cells):  # and the single field of that robot alone, on the device
                m.plan_field([_centre(m, *c)], inflate_cells=r)
                np.testing.assert_array_equal(m.plan_cost_field(), exp[k])
                np.testing.assert_array_equal(m.plan_team_field(k), exp[k])
    finally:
        m.close()


# ---- 2. the source bit is per field -------------------------------------------------
def _gap_map(H, W, wall_x, gap_y):
    """All free but an unknown column; A stands in it at gap_y, on an unknown cell."""
    st = np.zeros((H, W), np.int8)
    st[:, wall_x] = -1
    return st, (wall_x, gap_y)


@pytest.mark.parametrize("H,W,wall_x,gap_y", [(64, 64, 32, 20), (128, 128, 64, 63), (128, 128, 63, 64)])
def test_a_robot_in_the_gap_opens_it_for_itself_only(H, W, wall_x, gap_y):
    """A's own cell is the only passage through an unknown column: field A
    crosses it, field B (a robot on the left) reaches nothing on the right.
    On 128 x 128 the gap is a corner cell of its tile: the tiles around the
    junction see A's source only through their ring."""
    st, A = _gap_map(H, W, wall_x, gap_y)
    B = (5, 7)
    m = _mapper(st)
    try:
        for cells in ([A, B], [B, A]):
            _, exp = _check_layers(m, st, cells, 0)
            fa, fb = exp[cells.index(A)], exp[cells.index(B)]
            assert (fa[:, wall_x + 1:] != U).all() and (fa[:, :wall_x] != U).all()
            assert (fb[:, wall_x:] == U).all() and (fb[:, :wall_x] != U).all()
            assert fa[gap_y, wall_x + 1] == 5 and fa[gap_y + 1, wall_x + 1] == 10  # no diagonal out of the gap
    finally:
        m.close()


@pytest.mark.parametrize("H,W,A", [(64, 64, (30, 20)), (128, 128, (64, 63)), (128, 128, (63, 64))])
def test_the_row_scan_runs_through_the_robots_own_cell(H, W, A):
    """A stands on an unknown cell in the middle of a free row: in field A
    the row's costs continue through it, in field B the cell is a hole."""
    st = np.zeros((H, W), np.int8)
    st[A[1], A[0]] = -1
    B = (2, A[1])
    m = _mapper(st)
    try:
        _, exp = _check_layers(m, st, [A, B], 0)
        assert exp[0][A[1], A[0] + 9] == 45 and exp[0][A[1], A[0] - 9] == 45
        assert exp[1][A[1], A[0]] == U and exp[1][A[1], A[0] + 1] > 5 * (A[0] + 1 - B[0])  # round the hole
    finally:
        m.close()


# ---- 3. shared tile, shared cell, a robot inside an inflation disc ---------------------
def test_shared_tile_shared_cell_and_inflated_cell():
    st = _random_state(21, 130, 140)
    st[60:80, 60:80] = 0
    st[70, 70] = 100  # (71, 70) is inside its inflation disc
    st[30:40, 30:40] = 0
    cells = [(33, 33), (38, 36), (71, 70), (33, 33)]  # 0, 1, 3: one tile; 0 and 3: one cell
    m = _mapper(st)
    try:
        assert not plan.traversable(st, 1)[70, 71]
        _, exp = _check_layers(m, st, cells, 1)
        np.testing.assert_array_equal(m.plan_team_field(0), m.plan_team_field(3))
        assert exp[2][70, 71] == 0 and exp[0][70, 71] == U  # traversable for robot 2 alone
    finally:
        m.close()


# ---- 4. different settling times --------------------------------------------------------
def _serpentine_and_room():
    """192 x 192: a wall every 4th row with alternating end gaps, and at the
    left end of the last corridor a sealed 3 x 3 room."""
    st = np.zeros((192, 192), np.int8)
    for k, y in enumerate(range(3, 192, 4)):
        st[y, :] = 100
        if k % 2 == 0:
            st[y, 188:] = 0  # gap at the right end
        else:
            st[y, :4] = 0    # gap at the left end
    st[191, :] = 100
    st[188:191, 3] = 100     # the room: x 0..2, y 188..190
    return st


def test_fields_that_settle_at_different_times():
    st = _serpentine_and_room()
    cells = [(1, 1), (1, 189)]
    m = _mapper(st)
    try:
        stats, exp = _check_layers(m, st, cells, 0)
        assert stats["reached"] == [int((st == 0).sum()) - 9, 9]
        single = m.plan_field([_centre(m, 1, 1)], inflate_cells=0)
        room = m.plan_field([_centre(m, 1, 189)], inflate_cells=0)
        assert single["rounds"] > 4 * room["rounds"]
        assert stats["rounds"] == single["rounds"]  # the maximum over the fields, not their sum
        assert stats["tile_relaxations"] == single["tile_relaxations"] + room["tile_relaxations"]
    finally:
        m.close()


# ---- 5. limits -----------------------------------------------------------------------------
def test_limits():
    st = _random_state(14, 64, 64)
    st[20:44, 20:44] = 0
    free = np.argwhere(st == 0)
    rng = np.random.default_rng(3)
    cells = [(int(cx), int(cy)) for cy, cx in free[rng.choice(len(free), 64, replace=False)]]
    m = _mapper(st)
    try:
        _check_layers(m, st, cells, 0)
        assert _code(lambda: m.plan_team_field(64)) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.plan_team_field(-1)) == _ffi.DM_ERR_INVALID_ARG
        _, exp = _check_layers(m, st, [(30, 30), (25, 40)], 0, max_cost=60)
        full = plan.team_fields(st, [(30, 30), (25, 40)], 0)
        for e, f in zip(exp, full):
            np.testing.assert_array_equal(e, np.where(f <= 60, f, U))
            assert (e != U).sum() < (f != U).sum()
        assert _code(lambda: m.plan_team_field(2)) == _ffi.DM_ERR_INVALID_ARG  # two fields now
        for n in (0, 65):
            assert _code(lambda: m.plan_team(np.zeros((n, 2)))) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.plan_team([_centre(m, 5, 5), (1e6, 0.0)])) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.plan_team([_centre(m, 5, 5)], inflate_cells=33)) == _ffi.DM_ERR_INVALID_ARG
        np.testing.assert_array_equal(m.plan_team_field(1), exp[1])  # a refused call leaves the fields
    finally:
        m.close()


# ---- 6. query and path -----------------------------------------------------------------------
def test_query_matrix_and_paths():
    st = _random_state(31, 70, 130)
    st[10:60, 20:24] = 0
    st[8:12, 20:110] = 0
    st[30, 21] = -1  # robot 0 stands on an unknown cell
    st[62:67, 100:105] = 100
    st[63:66, 101:104] = 0  # a sealed room: robot 2 reaches nothing else, the others not this
    cells = [(21, 30), (100, 9), (102, 64)]
    r = 1
    m = _mapper(st)
    try:
        _, exp = _check_layers(m, st, cells, r)
        p = m.params
        targets = [_centre(m, 22, 50), _centre(m, 60, 9), _centre(m, 102, 64), (1e9, 0.0), (float("nan"), 0.0),
                   _centre(m, 0, 69), _centre(m, 129, 0)]
        tcells = [plan.cell_of(x, y, p.origin_x, p.origin_y, p.resolution, 130, 70) for x, y in targets]
        for snap in (0, 3, 16):
            cost, cell = m.plan_team_query(targets, snap_cells=snap)
            assert cost.shape == cell.shape == (3, len(targets))
            for k in range(3):
                for i, t in enumerate(tcells):
                    assert (int(cost[k, i]), int(cell[k, i])) == plan.snap(exp[k], t, snap), (k, i, snap)
        cost, cell = m.plan_team_query(targets, snap_cells=0)
        assert cost[0, 2] == U and cell[0, 2] == -1 and cost[2, 2] == 0  # the room: robot 2 alone
        assert cost[:, 3].tolist() == [U] * 3 and cell[:, 4].tolist() == [-1] * 3  # out of the grid
        trav = plan.traversable(st, r)
        for k, c in enumerate(cells):
            t = plan.with_sources(trav, [c])
            reached = np.argwhere(exp[k] != U)
            far = reached[np.argmax(exp[k][exp[k] != U])]
            for cy, cx in (far, reached[len(reached) // 2]):
                for snap in (0, 3):
                    got = m.plan_team_path(k, _centre(m, cx, cy), snap_cells=snap)
                    _, ecell = plan.snap(exp[k], (int(cx), int(cy)), snap)
                    assert got.tolist() == plan.path(exp[k], t, ecell)
                    assert got[0] == c[1] * 130 + c[0] and got[-1] == ecell
        # a path that ends on another robot's non-free cell: robot 1's path to robot 0's cell
        # stops beside it (snapped), robot 0's own path to it is the cell alone
        assert m.plan_team_path(0, _centre(m, 21, 30), snap_cells=0).tolist() == [30 * 130 + 21]
        assert m.plan_team_path(1, _centre(m, 21, 30), snap_cells=0).size == 0
        got = m.plan_team_path(1, _centre(m, 21, 30), snap_cells=1)
        _, ecell = plan.snap(exp[1], (21, 30), 1)
        assert ecell != 30 * 130 + 21 and got.tolist() == plan.path(exp[1], plan.with_sources(trav, [cells[1]]), ecell)
        # and the reverse walk from a cell next to robot 0's source ends on that non-free cell
        back = m.plan_team_path(0, _centre(m, 22, 31), snap_cells=0)
        assert back[0] == 30 * 130 + 21 and st[30, 21] == -1 and len(back) == 2
        full = m.plan_team_path(0, _centre(m, 100, 9), snap_cells=0)
        assert len(full) > 50
        with pytest.raises(dm.DmError) as e:
            m.plan_team_path(0, _centre(m, 100, 9), snap_cells=0, cap=1)
        assert e.value.code == _ffi.DM_ERR_CAPACITY and f"{len(full)} cells" in str(e.value)
        assert m.plan_team_path(0, (1e9, 1e9)).size == 0
        assert _code(lambda: m.plan_team_path(3, _centre(m, 22, 31))) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.plan_team_query(targets, snap_cells=17)) == _ffi.DM_ERR_INVALID_ARG
        m.profile(True)
        m.plan_team([_centre(m, *c) for c in cells], inflate_cells=r)
        m.plan_team_query(targets)
        m.plan_team_path(0, _centre(m, 100, 9))
        prof = m.profile_read()
        for name in ("plan_team_travers", "plan_team_seed", "plan_team_relax", "plan_team_count", "plan_team_query",
                     "plan_team_path"):
            assert name in prof, prof
    finally:
        m.close()


# ---- 7. lifetime ---------------------------------------------------------------------------------
def test_single_field_and_team_fields_do_not_disturb_each_other():
    st = _random_state(41, 96, 96)
    st[40:60, 10:90] = 0
    st[50, 50] = -1
    single_src, cells = (50, 50), [(12, 45), (85, 55)]
    m = _mapper(st)
    try:
        m.plan_field([_centre(m, *single_src)], inflate_cells=1)
        f1 = m.plan_cost_field()
        p1 = m.plan_path(_centre(m, 12, 45), snap_cells=2)
        np.testing.assert_array_equal(f1, plan.field(st, [single_src], 1))
        _, exp = _check_layers(m, st, cells, 2)
        np.testing.assert_array_equal(m.plan_cost_field(), f1)  # plan_field, plan_team, plan_cost_field
        assert m.plan_path(_centre(m, 12, 45), snap_cells=2).tolist() == p1.tolist()  # over its own bit rows
        tp = m.plan_team_path(1, _centre(m, 12, 45), snap_cells=2)
        m.plan_field([_centre(m, *single_src)], inflate_cells=0)  # another inflation: plan_trav is overwritten
        np.testing.assert_array_equal(m.plan_team_field(0), exp[0])
        np.testing.assert_array_equal(m.plan_team_field(1), exp[1])
        assert m.plan_team_path(1, _centre(m, 12, 45), snap_cells=2).tolist() == tp.tolist()
        t = plan.with_sources(plan.traversable(st, 2), [cells[1]])
        assert tp.tolist() == plan.path(exp[1], t, plan.snap(exp[1], (12, 45), 2)[1]) and len(tp) > 20
    finally:
        m.close()


def test_team_fields_are_stale_after_any_map_write():
    st = np.zeros((96, 96), np.int8)
    m = _mapper(st)
    a, b = _centre(m, 10, 10), _centre(m, 80, 70)

    def stale():
        for call in (lambda: m.plan_team_query([a]), lambda: m.plan_team_path(0, a), lambda: m.plan_team_field(0)):
            assert _code(call) == _ffi.DM_ERR_STATE

    try:
        stale()  # no fields yet
        writers = (lambda: m.integrate(np.zeros((1, 3)), np.full((1, 8), 1.0, np.float32), 0.0, 0.5),
                   lambda: m.set_state(st), m.reset)
        for write in writers:
            m.plan_team([a, b], inflate_cells=0)
            assert m.plan_team_query([a])[0][:, 0].tolist()[0] == 0
            write()
            stale()
        m.plan_team([a, b], inflate_cells=0)  # new fields clear it (a reset map: the sources alone)
        assert m.plan_team_path(1, b).tolist() == [70 * 96 + 80]
    finally:
        m.close()


def test_round_bound_leaves_no_team_fields():
    st = np.zeros((128, 128), np.int8)
    os.environ["DM_PLAN_MAX_ROUNDS"] = "1"
    try:
        m = _mapper(st)
    finally:
        del os.environ["DM_PLAN_MAX_ROUNDS"]
    try:
        a = _centre(m, 10, 10)
        assert _code(lambda: m.plan_team([a, _centre(m, 100, 100)], inflate_cells=0)) == _ffi.DM_ERR_INCOMPLETE
        for call in (lambda: m.plan_team_query([a]), lambda: m.plan_team_path(0, a), lambda: m.plan_team_field(0)):
            assert _code(call) == _ffi.DM_ERR_STATE
    finally:
        m.close()


def test_band_and_sharded_handles_are_refused():
    calls = (lambda m: m.plan_team([(0.0, 0.0)]), lambda m: m.plan_team_field(0),
             lambda m: m.plan_team_query([(0.0, 0.0)]), lambda m: m.plan_team_path(0, (0.0, 0.0)),
             lambda m: m.assign_goals_team([(0.0, 0.0)]))
    m = dm.OccupancyMapper(cases.make_params(128, 128, band_row0=0, band_rows=64))
    try:
        for call in calls:
            with pytest.raises(dm.DmError) as e:
                call(m)
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "whole map" in str(e.value)
    finally:
        m.close()
    m = dm.OccupancyMapper(cases.make_params(128, 128), devices=[0, 0])
    try:
        for call in calls:
            with pytest.raises(dm.DmError) as e:
                call(m)
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "sharded" in str(e.value)
    finally:
        m.close()


# ---- 8. goals ---------------------------------------------------------------------------------------
def _same_goals(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        if e is None:
            assert g is None
        else:
            assert g is not None and tuple(g) == tuple(e)  # index, the same doubles, cell (, gain)


def _goal_map(st):
    m = _mapper(st)
    cl = m.frontiers().clusters
    np.testing.assert_array_equal(cl, team_cases.clusters_of(m.params, st))
    return m, cl


def test_order_matters_fixture():
    """Robots in order (dm_assign_goals_path): 0 takes A, 1 is left with B.
    The best pair first: 1 takes A, 0 takes B."""
    st, robots, A, B = team_cases.order_matters()
    m, cl = _goal_map(st)
    try:
        p = m.params
        xy = [_centre(m, *c) for c in robots]
        args = (p.origin_x, p.origin_y, p.resolution)
        by_path = m.assign_goals_path(xy, **team_cases.KW)
        _same_goals(by_path, plan.assign_goals_path(st, cl, xy, *args, **team_cases.KW))
        assert [g[0] for g in by_path] == [A, B]
        team = m.assign_goals_team(xy, **team_cases.KW)
        _same_goals(team, plan.assign_goals_team(st, cl, xy, *args, **team_cases.KW))
        assert [g[0] for g in team] == [B, A]
        _same_goals(m.assign_goals_team(xy[::-1], **team_cases.KW), team[::-1])
    finally:
        m.close()


def test_tie_fixture():
    st, P, Q, X, Y = team_cases.ties()
    m, cl = _goal_map(st)
    try:
        p = m.params
        for robots in ([P, Q], [Q, P]):
            xy = [_centre(m, *c) for c in robots]
            got = m.assign_goals_team(xy, **team_cases.KW)
            _same_goals(got, plan.assign_goals_team(st, cl, xy, p.origin_x, p.origin_y, p.resolution,
                                                    **team_cases.KW))
            assert [g[0] for g in got] == [X, Y]  # the smaller label first, then the smaller robot
    finally:
        m.close()


def _open_state(seed, H, W):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, -1, 100], np.int8), size=(H, W), p=[0.9, 0.07, 0.03])


def test_one_robot_is_assign_goals_path_and_gain():
    st = _open_state(7, 70, 130)
    m, cl = _goal_map(st)
    try:
        free = np.argwhere(st == 0)
        kw = dict(min_size=2, distance_weight=0.5, min_distance=0.2, inflate_cells=1, snap_cells=3)
        some = 0
        for k in (3, 40, 200):
            robot = [_centre(m, int(free[k][1]), int(free[k][0]))]
            got = m.assign_goals_team(robot, **kw)
            _same_goals(got, m.assign_goals_path(robot, **kw))
            gg = m.assign_goals_team(robot, min_gain=2, radius_cells=12, **kw)
            _same_goals(gg, m.assign_goals_gain(robot, min_gain=2, radius_cells=12, **kw))
            some += (got[0] is not None) + (gg[0] is not None)
        assert some >= 2
    finally:
        m.close()


def test_gain_mode_and_the_fields_left_behind():
    st = _open_state(8, 70, 130)
    m, cl = _goal_map(st)
    try:
        p = m.params
        free = np.argwhere(st == 0)
        cells = [(int(free[k][1]), int(free[k][0])) for k in (10, 2500, 5000)]
        xy = [_centre(m, *c) for c in cells]
        args = (p.origin_x, p.origin_y, p.resolution)
        m.plan_field([xy[0]], inflate_cells=0)
        single = m.plan_cost_field()
        for kw in (dict(min_size=2, min_gain=3, distance_weight=0.5, inflate_cells=1, snap_cells=3, radius_cells=12),
                   dict(min_size=1, min_gain=0, distance_weight=2.0, min_distance=0.5, inflate_cells=1, snap_cells=2,
                        radius_cells=5),
                   dict(min_size=2, distance_weight=0.5, inflate_cells=1, snap_cells=3)):
            got = m.assign_goals_team(xy, **kw)
            _same_goals(got, plan.assign_goals_team(st, cl, xy, *args, **kw))
            assert sum(g is not None for g in got) >= 2
            if "radius_cells" in kw:
                for g in got:
                    if g is not None:
                        assert g[3] == gain.visible_unknown(st, (g[2] % 130, g[2] // 130), kw["radius_cells"])
            # the call leaves these robots' fields: the path to a goal ends in its cell
            exp = plan.team_fields(st, cells, 1)
            for r, g in enumerate(got):
                np.testing.assert_array_equal(m.plan_team_field(r), exp[r])
                if g is not None:
                    path = m.plan_team_path(r, g[1], snap_cells=0)
                    assert path[0] == cells[r][1] * 130 + cells[r][0] and path[-1] == g[2]
        np.testing.assert_array_equal(m.plan_cost_field(), single)  # the single field is untouched
        assert m.assign_goals_team(np.zeros((0, 2))) == []
        for bad in (dict(distance_weight=-1.0), dict(inflate_cells=33), dict(snap_cells=17), dict(radius_cells=512),
                    dict(radius_cells=-1), dict(radius_cells=5, min_gain=-1)):
            assert _code(lambda: m.assign_goals_team(xy, **bad)) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.assign_goals_team(np.zeros((65, 2)))) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.assign_goals_team([xy[0], (1e6, 0.0)])) == _ffi.DM_ERR_INVALID_ARG
    finally:
        m.close()

"""GPU: the device path planner (dm_plan_*, csrc/dm_plan.h) against its host
restatement dm.plan, bit for bit: traversability masks, distance fields,
snapped queries and paths, on the smallest maps at which each mechanism can go
wrong (one tile, ragged last tiles, discs and diagonals across tile junctions,
a serpentine that crosses every tile border many times), plus the field's
lifetime rules and error paths."""
import os

import numpy as np
import pytest

import cases
import dm
from dm import _ffi, plan

pytestmark = pytest.mark.gpu

U = plan.UNREACHABLE


def _mapper(st):
    H, W = st.shape
    m = dm.OccupancyMapper(cases.make_params(W, H))
    m.set_state(st)
    return m


def _centre(m, cx, cy):
    p = m.params
    return (p.origin_x + (cx + 0.5) * p.resolution, p.origin_y + (cy + 0.5) * p.resolution)


def _random_state(seed, H, W):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, -1, 100], np.int8), size=(H, W), p=[0.65, 0.10, 0.25])


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
            np.testing.assert_array_equal(m.plan_traversable(r), plan.traversable(st, r))
            cy, cx = free[rng.integers(len(free))]
            stats = m.plan_field([_centre(m, cx, cy)], inflate_cells=r)
            exp = plan.field(st, [(cx, cy)], r)
            np.testing.assert_array_equal(m.plan_cost_field(), exp)
            assert stats["reached"] == int((exp != U).sum())
            assert stats["traversable"] == int(plan.traversable(st, r).sum())
    finally:
        m.close()


def test_discs_across_tiles_and_the_grid_edge():
    """r = 32 around single occupied cells at tile corners: the discs span up
    to four tiles and are cut by the grid edge."""
    st = np.zeros((192, 192), np.int8)
    for x, y in ((63, 63), (64, 0), (127, 128), (0, 191)):
        st[y, x] = 100
    m = _mapper(st)
    try:
        np.testing.assert_array_equal(m.plan_traversable(32), plan.traversable(st, 32))
        np.testing.assert_array_equal(m.plan_traversable(31), plan.traversable(st, 31))
    finally:
        m.close()


@pytest.mark.parametrize("src,blk,dst", [((63, 63), (64, 63), (64, 64)), ((64, 63), (63, 63), (63, 64)),
                                         ((63, 64), (64, 64), (64, 63)), ((64, 64), (63, 64), (63, 63))])
def test_no_corner_cutting_across_the_tile_junction(src, blk, dst):
    """The four cells around the junction of four tiles: with one of them
    occupied the diagonal between two others is refused, whichever tiles hold
    the move's ends and the corner."""
    st = np.zeros((128, 128), np.int8)
    st[blk[1], blk[0]] = 100
    m = _mapper(st)
    try:
        m.plan_field([_centre(m, *src)], inflate_cells=0)
        f = m.plan_cost_field()
        assert f[dst[1], dst[0]] == 10
        np.testing.assert_array_equal(f, plan.field(st, [src], 0))
    finally:
        m.close()


def _serpentine():
    st = np.zeros((256, 256), np.int8)
    for k, y in enumerate(range(3, 256, 4)):
        st[y, :] = 100
        if k % 2 == 0:
            st[y, 252:] = 0  # gap at the right end
        else:
            st[y, :4] = 0    # gap at the left end
    return st


def test_serpentine_rounds_and_round_bound():
    """A wall every 4th row with alternating end gaps: the shortest path
    crosses every tile border many times, so the field takes many rounds; a
    round bound of 3 (DM_PLAN_MAX_ROUNDS, read at dm_create) ends it with
    DM_ERR_INCOMPLETE and leaves no field."""
    st = _serpentine()
    exp = plan.field(st, [(1, 1)], 0)
    assert (exp != U).sum() == (st == 0).sum()
    m = _mapper(st)
    try:
        stats = m.plan_field([_centre(m, 1, 1)], inflate_cells=0)
        np.testing.assert_array_equal(m.plan_cost_field(), exp)
        assert stats["rounds"] > 4 and stats["tile_relaxations"] >= stats["rounds"]
    finally:
        m.close()
    os.environ["DM_PLAN_MAX_ROUNDS"] = "3"
    try:
        m = _mapper(st)
    finally:
        del os.environ["DM_PLAN_MAX_ROUNDS"]
    try:
        with pytest.raises(dm.DmError) as e:
            m.plan_field([_centre(m, 1, 1)], inflate_cells=0)
        assert e.value.code == _ffi.DM_ERR_INCOMPLETE
        with pytest.raises(dm.DmError) as e:
            m.plan_cost_field()
        assert e.value.code == _ffi.DM_ERR_STATE
    finally:
        m.close()
    m = _mapper(st)  # a fresh handle without the override
    try:
        m.plan_field([_centre(m, 1, 1)], inflate_cells=0)
        np.testing.assert_array_equal(m.plan_cost_field(), exp)
    finally:
        m.close()


def test_closed_room_and_max_cost():
    st = np.zeros((128, 128), np.int8)
    st[40:90, 40] = st[40:90, 89] = 100
    st[40, 40:90] = st[89, 40:90] = 100
    m = _mapper(st)
    try:
        m.plan_field([_centre(m, 5, 5)], inflate_cells=1)
        f = m.plan_cost_field()
        exp = plan.field(st, [(5, 5)], 1)
        np.testing.assert_array_equal(f, exp)
        assert (f[42:88, 42:88] == U).all() and f[5, 100] != U
        cost, cell = m.plan_query([_centre(m, 64, 64), _centre(m, 100, 5), (1e9, 0.0), (float("nan"), 0.0)],
                                  snap_cells=16)
        assert cost.tolist()[0] == U and cell.tolist()[0] == -1
        assert (int(cost[1]), int(cell[1])) == (int(exp[5, 100]), 5 * 128 + 100)
        assert cost.tolist()[2:] == [U, U] and cell.tolist()[2:] == [-1, -1]  # out of the grid
        m.plan_field([_centre(m, 5, 5)], inflate_cells=1, max_cost=200)
        capped = m.plan_cost_field()
        np.testing.assert_array_equal(capped, np.where(exp <= 200, exp, U))
        assert (capped != U).sum() < (exp != U).sum()
    finally:
        m.close()


def test_multiple_sources_and_source_cells():
    st = _random_state(21, 130, 140)
    st[30:40, 30:40] = 0
    st[35, 35] = -1   # a source on an unknown cell
    st[60:80, 60:80] = 0
    st[70, 70] = 100  # (71, 70) is inside its inflation disc
    sources = [(35, 35), (71, 70), (100, 20)]
    st[20, 100] = 0
    m = _mapper(st)
    try:
        singles = []
        for s in sources:
            m.plan_field([_centre(m, *s)], inflate_cells=1)
            singles.append(m.plan_cost_field())
        m.plan_field([_centre(m, *s) for s in sources], inflate_cells=1)
        f = m.plan_cost_field()
        np.testing.assert_array_equal(f, np.minimum(np.minimum(singles[0], singles[1]), singles[2]))
        np.testing.assert_array_equal(f, plan.field(st, sources, 1))
        assert not plan.traversable(st, 1)[35, 35] and not plan.traversable(st, 1)[70, 71]
        assert f[35, 35] == 0 and f[70, 71] == 0 and f[20, 100] == 0
        for bad in ((1e6, 0.0), (float("nan"), 0.0), (m.params.origin_x - 0.01, 0.0)):
            with pytest.raises(dm.DmError) as e:
                m.plan_field([_centre(m, 5, 5), bad])
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG
        for n in (0, 257):
            with pytest.raises(dm.DmError):
                m.plan_field(np.zeros((n, 2)))
        with pytest.raises(dm.DmError):
            m.plan_field([_centre(m, 5, 5)], inflate_cells=33)
    finally:
        m.close()


def test_field_is_stale_after_any_map_write():
    st = np.zeros((96, 96), np.int8)
    m = _mapper(st)
    src = _centre(m, 10, 10)

    def stale():
        for call in (lambda: m.plan_query([src]), lambda: m.plan_path(src), m.plan_cost_field):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_STATE

    try:
        stale()  # no field yet
        writers = (lambda: m.integrate(np.zeros((1, 3)), np.full((1, 8), 1.0, np.float32), 0.0, 0.5),
                   lambda: m.set_state(st), m.reset)
        for write in writers:
            m.plan_field([src], inflate_cells=0)
            assert m.plan_query([src])[0][0] == 0
            write()
            stale()
        m.plan_field([src], inflate_cells=0)  # a new field clears it (a reset map: the source alone)
        assert m.plan_path(src).tolist() == [10 * 96 + 10]
        m.plan_traversable(1)  # does not touch the field
        assert m.plan_cost_field()[10, 10] == 0
    finally:
        m.close()


def test_paths():
    st = _random_state(31, 70, 130)
    st[10:60, 20:24] = 0
    st[8:12, 20:110] = 0
    m = _mapper(st)
    try:
        r = 1
        m.plan_field([_centre(m, 21, 30)], inflate_cells=r)
        f = m.plan_cost_field()
        t = plan.with_sources(plan.traversable(st, r), [(21, 30)])
        np.testing.assert_array_equal(f, plan.field(st, [(21, 30)], r))
        reached = np.argwhere(f != U)
        far = reached[np.argmax(f[f != U])]
        checked = 0
        for cy, cx in (far, reached[len(reached) // 2], reached[len(reached) // 3]):
            for snap in (0, 3):
                got = m.plan_path(_centre(m, cx, cy), snap_cells=snap)
                ecost, ecell = plan.snap(f, (int(cx), int(cy)), snap)
                assert got.tolist() == plan.path(f, t, ecell)
                assert got[0] == 30 * 130 + 21 and got[-1] == ecell
                ys, xs = got // 130, got % 130
                d = np.diff(f[ys, xs].astype(np.int64))
                step = np.abs(np.diff(ys)) + np.abs(np.diff(xs))
                assert ((d == 5) & (step == 1) | (d == 7) & (step == 2)).all()
                diag = np.flatnonzero(step == 2)  # no corner cutting
                assert t[ys[diag], xs[diag + 1]].all() and t[ys[diag + 1], xs[diag]].all()
                assert t[ys, xs].all()
                checked += len(got)
        assert checked > 100
        full = m.plan_path(_centre(m, far[1], far[0]), snap_cells=0)
        with pytest.raises(dm.DmError) as e:
            m.plan_path(_centre(m, far[1], far[0]), snap_cells=0, cap=1)
        assert e.value.code == _ffi.DM_ERR_CAPACITY and f"{len(full)} cells" in str(e.value)
        unreached = np.argwhere(f == U)[0]
        assert m.plan_path(_centre(m, unreached[1], unreached[0]), snap_cells=0).size == 0
        assert m.plan_path((1e9, 1e9)).size == 0
    finally:
        m.close()


def test_field_on_an_integrated_map():
    p, batches, amin, inc = cases.world_case(3, 400, 400, 0.05, 2, 360, 4)
    m = dm.OccupancyMapper(p)
    try:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        st = m.state()
        x, y = batches[0][0][0][:2]
        stats = m.plan_field([(x, y)], inflate_cells=2)
        src = plan.cell_of(x, y, p.origin_x, p.origin_y, p.resolution, 400, 400)
        exp = plan.field(st, [src], 2)
        np.testing.assert_array_equal(m.plan_cost_field(), exp)
        np.testing.assert_array_equal(m.plan_traversable(2), plan.traversable(st, 2))
        assert stats["reached"] == int((exp != U).sum()) > 100
        m.profile(True)
        m.plan_field([(x, y)], inflate_cells=2)
        m.plan_query([(x, y)])
        m.plan_path((x, y))
        prof = m.profile_read()
        for name in ("plan_travers", "plan_relax", "plan_query", "plan_path"):
            assert name in prof, prof
    finally:
        m.close()


def test_band_and_sharded_handles_are_refused():
    p = cases.make_params(128, 128, band_row0=0, band_rows=64)
    m = dm.OccupancyMapper(p)
    try:
        with pytest.raises(dm.DmError) as e:
            m.plan_field([(0.0, 0.0)])
        assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "whole map" in str(e.value)
    finally:
        m.close()
    m = dm.OccupancyMapper(cases.make_params(128, 128), devices=[0, 0])
    try:
        for call in (lambda: m.plan_field([(0.0, 0.0)]), lambda: m.plan_traversable(1),
                     lambda: m.assign_goals_path([(0.0, 0.0)])):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "sharded" in str(e.value)
    finally:
        m.close()

"""GPU: the overlap-aware gain calls (dm_gain_views_joint,
dm_assign_goals_coord, dm_gain_claimed; csrc/dm_gain.h) against
the host restatement dm.gain on the same map, bit for bit: every radius at which
the bitmap's row changes its word count on a map whose last claimed word of a
row is partial, views within R of every edge and several residues of
(vx - R) mod 32, held views committed by many workgroups at once, both forms of
the kernel, the goal assignment with and without held views, the policy case the
calls are for, and the errors."""
import ctypes

import numpy as np
import pytest

import cases
import dm
from dm import _ffi, gain, match, plan

pytestmark = pytest.mark.gpu


def _centre(p, cx, cy):
    return (p.origin_x + (cx + 0.5) * p.resolution, p.origin_y + (cy + 0.5) * p.resolution)


def _mapper(st, **kw):
    H, W = st.shape
    m = dm.OccupancyMapper(cases.make_params(W, H, **kw))
    m.set_state(st)
    return m


def _host_joint(m, st, views, R):
    p = m.params
    return gain.gain_views_joint(st, views, p.origin_x, p.origin_y, p.resolution, R)


def _check_joint(m, st, views, R):
    got_m, got_c = m.gain_views_joint(views, R)
    exp_m, exp_c, exp_claimed = _host_joint(m, st, views, R)
    claimed = m.gain_claimed()
    assert got_m.dtype == np.uint32 and got_c.dtype == np.int64 and claimed.dtype == bool
    np.testing.assert_array_equal(got_c, exp_c)
    np.testing.assert_array_equal(got_m, exp_m)
    np.testing.assert_array_equal(claimed, exp_claimed)
    assert int(got_m.sum()) == int(claimed.sum())
    return got_m, got_c, claimed


def test_joint_parity():
    st = cases.random_state(11, 136, 200, p_free=0.55, p_occ=0.03)  # W = 200: the last claimed word is partial
    H, W = st.shape
    assert (H, W) == (136, 200)
    m = _mapper(st)
    try:
        p = m.params
        occ = np.argwhere(st == 100)[7]
        unk = np.argwhere(st == -1)[11]
        cells = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1),                      # corners
                 (0, 70), (W - 1, 33), (101, 0), (64, H - 1), (5, 100), (W - 3, 90),    # edges: vx - R < 0, vx + R >= W
                 (60, 70), (61, 70), (62, 70), (63, 70), (64, 70), (65, 70), (66, 70), (67, 70),  # residues
                 (int(occ[1]), int(occ[0])), (int(unk[1]), int(unk[0]))]
        views = [_centre(p, x, y) for x, y in cells]
        views += [views[10], (1e9, 0.0), (float("nan"), 0.0), (0.0, float("inf"))]  # a duplicate, outside, non-finite
        total = 0
        for R in (1, 15, 16, 31, 32, 40):
            g, c, claimed = _check_joint(m, st, views, R)
            assert list(c[-3:]) == [-1, -1, -1] and list(g[-3:]) == [0, 0, 0]
            assert g[18] == 0 and g[20] == 0  # the occupied cell sees nothing, the duplicate nothing new
            assert not claimed[st == 0].any() and not claimed[st == 100].any()
            total += int(g.sum())
        assert total > 5000
        # no views: an empty claimed set
        g, c = m.gain_views_joint(np.zeros((0, 2)), 8)
        assert g.shape == (0,) and c.shape == (0,) and not m.gain_claimed().any()
    finally:
        m.close()


def _check_goals(m, st, clusters, robots, held, cache, **kw):
    p = m.params
    got = m.assign_goals_coord(robots, held_xy=held, **kw)
    claimed = m.gain_claimed()
    exp, exp_claimed = gain.assign_goals_coord(st, clusters, robots, p.origin_x, p.origin_y, p.resolution,
                                               held_xy=held, cache=cache, return_claimed=True, **kw)
    assert len(got) == len(exp) == len(robots)
    for g, e in zip(got, exp):
        if e is None:
            assert g is None
        else:
            assert g is not None and g[0] == e[0] and g[2] == e[2] and g[3] == e[3]
            assert g[1] == e[1]  # the same doubles
    np.testing.assert_array_equal(claimed, exp_claimed)
    return got


def test_held_views_seeded_by_many_workgroups():
    st = cases.blob_state(5, 256, 256)
    m = _mapper(st)
    try:
        p = m.params
        cl = m.frontiers().clusters
        assert len(cl) > 2
        rng = np.random.default_rng(21)
        # 64 held views in a 64-cell square: every one overlaps its neighbours (R = 8)
        held = np.stack([p.origin_x + rng.uniform(96, 160, 64) * p.resolution,
                         p.origin_y + rng.uniform(96, 160, 64) * p.resolution], axis=1)
        free = np.argwhere(st == 0)
        robots = [_centre(p, int(free[i][1]), int(free[i][0])) for i in (len(free) // 3, 2 * len(free) // 3)]
        _check_goals(m, st, cl, robots, held, {}, min_size=1, inflate_cells=1, snap_cells=5, radius_cells=8)
        claimed = m.gain_claimed()
        hm, _, hcl = gain.gain_views_joint(st, held, p.origin_x, p.origin_y, p.resolution, 8)
        assert int(hm.sum()) > 300 and int((hm == 0).sum()) < 64  # the views see something, and overlap
        assert (claimed & hcl).sum() == hcl.sum()
    finally:
        m.close()


def test_both_kernel_forms():
    """R = 240 runs the dynamically sized bitmap, R = 511 the static one."""
    N = 1100
    m = dm.OccupancyMapper(cases.make_params(N, N))
    try:
        p = m.params
        unknown = np.full((N, N), -1, np.int8)
        mid, off = _centre(p, N // 2, N // 2), _centre(p, N // 2 + 100, N // 2)
        for R, disc in ((240, 180917), (511, 820249)):
            g, c = m.gain_views_joint([mid, off], R)
            eg, ec, ecl = _host_joint(m, unknown, [mid, off], R)
            assert g[0] == disc
            assert g[1] == eg[1] and 0 < g[1] < disc
            np.testing.assert_array_equal(c, ec)
            claimed = m.gain_claimed()
            assert int(g.sum()) == int(claimed.sum())
            np.testing.assert_array_equal(claimed, ecl)
        st = cases.random_state(23, N, N, p_free=0.6, p_occ=0.002)
        m.set_state(st)
        views = [mid, _centre(p, 3, 700), _centre(p, 830, 260)]
        for R in (240, 511):
            g, _, _ = _check_joint(m, st, views, R)
            assert g.min() > 1000
    finally:
        m.close()


def test_goals_on_mapped_world():
    p, batches, amin, inc = cases.world_case(51, 512, 512, 0.05, 4, 720, 3, region_frac=0.7)
    m = dm.OccupancyMapper(p)
    try:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        cl = m.frontiers().clusters
        st = m.state()
        assert len(cl) > 10
        robots = np.concatenate([batches[-1][0][:, :2], batches[0][0][:, :2]])[:8]
        held3 = [(float(c["cx_m"]), float(c["cy_m"])) for c in cl[:3]]
        cache = {}
        some = 0
        common = dict(inflate_cells=2, snap_cells=5, radius_cells=40)
        sets = (dict(min_size=8, min_gain=0), dict(min_size=1, min_gain=30, distance_weight=0.25, min_distance=1.0))
        for R in (1, 8):
            for kw in sets:
                for held in ((), held3):
                    got = _check_goals(m, st, cl, robots[:R], held, cache, **common, **kw)
                    some += sum(g is not None for g in got)
                    idx = [g[0] for g in got if g is not None]
                    assert len(set(idx)) == len(idx)  # no cluster twice
                # nothing held: robot 0 is dm_assign_goals_gain's robot 0
                first = m.assign_goals_coord(robots[:R], **common, **kw)[0]
                assert first == m.assign_goals_gain(robots[:R], **common, **kw)[0]
        assert some > 4
        # two robots at one pose get different clusters
        same = np.array([robots[0], robots[0], robots[5]])
        got = _check_goals(m, st, cl, same, (), cache, **common, **sets[0])
        assert got[0] is not None and got[1] is not None and got[0][0] != got[1][0]
        # the field left behind is the last robot's
        last = plan.cell_of(same[2][0], same[2][1], p.origin_x, p.origin_y, p.resolution, 512, 512)
        np.testing.assert_array_equal(m.plan_cost_field(), cache[last])
    finally:
        m.close()


def test_policy_case_two_doorways_onto_one_hall():
    st = np.full((128, 128), -1, np.int8)
    st[9:101, 9:61] = 100
    st[10:100, 10:60] = 0
    st[30:34, 60] = 0     # doorway A, right wall
    st[40:44, 60] = 0     # doorway B, right wall, same unknown hall as A
    st[84:88, 9] = 0      # doorway C, left wall
    m = _mapper(st, min_frontier_size=1)
    try:
        p = m.params
        cl = m.frontiers().clusters
        assert len(cl) == 3 and list(cl["size"]) == [4, 4, 4]
        robots = [_centre(p, 35, 50), _centre(p, 35, 52)]
        kw = dict(min_size=1, inflate_cells=1, snap_cells=3, radius_cells=40)
        unc = m.assign_goals_gain(robots, **kw)
        assert [g[0] for g in unc] == [1, 0] and [g[3] for g in unc] == [2211, 2134]
        co = _check_goals(m, st, cl, robots, (), {}, **kw)
        assert [g[0] for g in co] == [1, 2] and [g[3] for g in co] == [2211, 448]
        assert [g[2] for g in co] == [42 * 128 + 60, 85 * 128 + 9]
        assert co[0][1] == _centre(p, 60, 42) and co[1][1] == _centre(p, 9, 85)
        assert int(m.gain_claimed().sum()) == 2659
        alone = _check_goals(m, st, cl, robots[1:], [_centre(p, 60, 42)], {}, **kw)[0]
        assert alone[0] == 2 and alone[3] == 448
        assert int(m.gain_claimed().sum()) == 2659
        g, _ = m.gain_views_joint([_centre(p, 60, 42), _centre(p, 60, 32)], 40)
        assert list(g) == [2211, 314]
    finally:
        m.close()


def test_the_calls_write_nothing():
    p, batches, amin, inc = cases.world_case(3, 128, 128, 0.05, 2, 90, 2)
    m = dm.OccupancyMapper(p)
    try:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        st, L = m.state(), m.logodds()
        cl = m.frontiers().clusters
        x, y = batches[0][0][0][:2]
        kern = match.kernel_table(0.1, 0.05, 4)
        poses, ranges = batches[-1]
        first = m.match_scans(poses, ranges, amin, inc, [0.0], 0, 5, 2, 1, 4, kern)
        m.plan_field([(x, y)], inflate_cells=1)
        field = m.plan_cost_field()
        m.profile(True)
        m.profile_reset()
        views = [(x, y), tuple(batches[-1][0][0][:2])]
        g, _, _ = _check_joint(m, st, views, 40)
        assert g.sum() > 0
        np.testing.assert_array_equal(m.state(), st)
        assert m.logodds().tobytes() == L.tobytes()
        np.testing.assert_array_equal(m.plan_cost_field(), field)  # no DM_ERR_STATE: the map version did not move
        # the assignment leaves its own field, the last robot's (here the same source and inflation)
        _check_goals(m, st, cl, [(x, y)], views[1:], {}, min_size=1, inflate_cells=1, snap_cells=5, radius_cells=40)
        np.testing.assert_array_equal(m.state(), st)
        assert m.logodds().tobytes() == L.tobytes()
        np.testing.assert_array_equal(m.plan_cost_field(), field)
        again = m.match_scans(poses, ranges, amin, inc, [0.0], 0, 5, 2, 1, 4, kern)
        np.testing.assert_array_equal(again["score"], first["score"])
        prof = m.profile_read()
        assert prof["gain_joint"][0] == 1 and prof["gain_commit"][0] >= 1
        assert prof.get("gain_views", (0, 0.0))[0] == 0  # the uncoordinated kernel did not run
        assert prof.get("match_field", (0, 0.0))[0] == 0  # the matcher's field was kept
    finally:
        m.close()


def _code(fn):
    with pytest.raises(dm.DmError) as e:
        fn()
    return e.value.code


def test_errors():
    m = dm.OccupancyMapper(cases.make_params(128, 128))
    try:
        lib, xy = dm.load_library(), np.zeros(2)
        g, c = np.zeros(1, np.uint32), np.zeros(1, np.int64)
        img = np.zeros((128, 128), np.uint8)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert lib.dm_gain_claimed(m._handle(), vp(img)) == _ffi.DM_ERR_STATE  # neither call has run
        assert _code(m.gain_claimed) == _ffi.DM_ERR_STATE
        for R in (0, 512, -3):
            assert _code(lambda: m.gain_views_joint([(0.0, 0.0)], R)) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_gain_views_joint(m._handle(), vp(xy), -1, 8, vp(g), vp(c)) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_gain_views_joint(m._handle(), vp(xy), 1025, 8, vp(g), vp(c)) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_gain_views_joint(m._handle(), None, 1, 8, vp(g), vp(c)) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_gain_views_joint(m._handle(), vp(xy), 1, 8, None, vp(c)) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_gain_views_joint(m._handle(), vp(xy), 1, 8, vp(g), None) == _ffi.DM_ERR_INVALID_ARG
        assert _code(m.gain_claimed) == _ffi.DM_ERR_STATE  # a rejected call leaves no claimed set
        # no collected result, as dm_assign_goals_gain
        assert _code(lambda: m.assign_goals_coord([(0.0, 0.0)])) == _ffi.DM_ERR_INVALID_ARG
        m.frontiers()
        assert m.assign_goals_coord([(0.0, 0.0), (1.0, 1.0)], held_xy=[(0.5, 0.5)], radius_cells=8) == [None, None]
        assert int(m.gain_claimed().sum()) == 197  # the held view's disc of radius 8
        for bad in (dict(min_gain=-1), dict(radius_cells=0), dict(radius_cells=512), dict(distance_weight=-1.0),
                    dict(inflate_cells=33), dict(snap_cells=17), dict(held_xy=np.zeros((1025, 2)))):
            assert _code(lambda: m.assign_goals_coord([(0.0, 0.0)], **bad)) == _ffi.DM_ERR_INVALID_ARG, bad
        assert _code(lambda: m.assign_goals_coord(np.zeros((257, 2)))) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.assign_goals_coord([(0.0, 0.0), (1e6, 0.0)])) == _ffi.DM_ERR_INVALID_ARG  # outside
        i64, f64, u32 = np.zeros(1, np.int64), np.zeros(2), np.zeros(1, np.uint32)
        args = (8, 0, 1.0, 0.0, 2, 0, 5, 8, vp(i64), vp(f64), vp(c), vp(u32))
        assert lib.dm_assign_goals_coord(m._handle(), vp(xy), 1, None, -1, *args) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_assign_goals_coord(m._handle(), vp(xy), 1, None, 1, *args) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_assign_goals_coord(m._handle(), None, 1, None, 0, *args) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_assign_goals_coord(m._handle(), vp(xy), -1, None, 0, *args) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_assign_goals_coord(m._handle(), vp(xy), 1, None, 0, *args) == 0  # held_xy may be NULL with 0
        assert lib.dm_gain_claimed(m._handle(), None) == _ffi.DM_ERR_INVALID_ARG
        # the handle is still good: the disc of radius 8, then nothing new from the same cell
        assert list(m.gain_views_joint([(0.0, 0.0), (0.0, 0.0)], 8)[0]) == [197, 0]
        assert int(m.gain_claimed().sum()) == 197
    finally:
        m.close()
    band = dm.OccupancyMapper(cases.make_params(128, 128, band_row0=0, band_rows=64))
    try:
        assert _code(lambda: band.gain_views_joint([(0.0, 0.0)], 8)) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: band.assign_goals_coord([(0.0, 0.0)])) == _ffi.DM_ERR_INVALID_ARG
        assert _code(band.gain_claimed) == _ffi.DM_ERR_INVALID_ARG
    finally:
        band.close()
    sharded = dm.OccupancyMapper(cases.make_params(128, 128), devices=[0, 0])
    try:
        for call in (lambda: sharded.gain_views_joint([(0.0, 0.0)], 8), lambda: sharded.assign_goals_coord([(0.0, 0.0)]),
                     sharded.gain_claimed):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "sharded" in str(e.value)
    finally:
        sharded.close()

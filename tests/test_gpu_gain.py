"""GPU: the information-gain calls (dm_gain_views, dm_assign_goals_gain;
csrc/dm_gain.h) against the host restatement dm.gain on the same map, bit for
bit: every radius at which the bitmap's row changes its word count, views on
the grid's edges and outside it, the default and the limit radius (the two
forms of the kernel), the goal assignment with its memo hit and missed, and
the policy case the feature is for."""
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


def _host(m, st, views, R):
    p = m.params
    return gain.gain_views(st, views, p.origin_x, p.origin_y, p.resolution, R)


def test_gain_views_parity():
    st = cases.random_state(11, 136, 200, p_free=0.55, p_occ=0.03)  # 200 x 136: edge tiles
    H, W = st.shape
    m = _mapper(st)
    try:
        p = m.params
        occ = np.argwhere(st == 100)[7]
        unk = np.argwhere(st == -1)[11]
        cells = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (0, 70), (W - 1, 33), (101, 0), (64, H - 1),
                 (int(occ[1]), int(occ[0])), (int(unk[1]), int(unk[0])), (63, 63), (64, 64), (150, 100), (31, 97)]
        views = [_centre(p, x, y) for x, y in cells]
        views += [(1e9, 0.0), (float("nan"), 0.0), (0.0, float("-inf")), views[10]]  # outside, non-finite, a duplicate
        np.testing.assert_array_equal(m.state(), st)
        total = 0
        for R in (1, 15, 16, 31, 32, 40):
            g, c = m.gain_views(views, R)
            eg, ec = _host(m, st, views, R)
            np.testing.assert_array_equal(c, ec)
            np.testing.assert_array_equal(g, eg)
            assert g.dtype == np.uint32 and c.dtype == np.int64
            assert list(c[-4:-1]) == [-1, -1, -1] and list(g[-4:-1]) == [0, 0, 0]
            assert g[8] == 0 and g[-1] == g[10]
            total += int(g.sum())
        assert total > 1000
        assert m.gain_views(np.zeros((0, 2)), 8)[0].shape == (0,)
    finally:
        m.close()


def test_many_views_index_every_workgroup():
    st = cases.blob_state(5, 256, 256)
    m = _mapper(st)
    try:
        p = m.params
        rng = np.random.default_rng(8)
        views = np.stack([p.origin_x + rng.uniform(-0.2, 256 * p.resolution + 0.2, 5000),
                          p.origin_y + rng.uniform(-0.2, 256 * p.resolution + 0.2, 5000)], axis=1)
        g, c = m.gain_views(views, 8)
        eg, ec = _host(m, st, views, 8)
        np.testing.assert_array_equal(c, ec)
        np.testing.assert_array_equal(g, eg)
        assert (c < 0).sum() > 0 and (g > 0).sum() > 500
    finally:
        m.close()


def test_default_and_limit_radius():
    """R = 240 runs the dynamically sized bitmap, R = 511 the static one."""
    N = 1100
    m = dm.OccupancyMapper(cases.make_params(N, N))
    try:
        p = m.params
        assert m.default_gain_radius() == 240
        mid, corner = _centre(p, N // 2, N // 2), _centre(p, 0, N - 1)
        # all unknown: the disc's lattice points, and a quarter of them (axes included) from a corner
        unknown = np.full((N, N), -1, np.int8)
        for R, disc in ((240, 180917), (511, 820249)):
            g, c = m.gain_views([mid, corner], R)
            assert c[0] == (N // 2) * N + N // 2 and c[1] == (N - 1) * N
            assert g[0] == disc
            assert g[1] == gain.visible_unknown(unknown, (0, N - 1), R) == (disc - 1 - 4 * R) // 4 + 2 * R + 1
        assert m.gain_views([mid])[0][0] == 180917  # the default radius
        st = cases.random_state(23, N, N, p_free=0.6, p_occ=0.002)
        m.set_state(st)
        views = [mid, _centre(p, 3, 700), _centre(p, 830, 260)]
        for R in (240, 511):
            g, c = m.gain_views(views, R)
            eg, ec = _host(m, st, views, R)
            np.testing.assert_array_equal(c, ec)
            np.testing.assert_array_equal(g, eg)
            assert g.min() > 1000
    finally:
        m.close()


def test_the_call_writes_nothing():
    p, batches, amin, inc = cases.world_case(3, 128, 128, 0.05, 2, 90, 2)
    m = dm.OccupancyMapper(p)
    try:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        st, L = m.state(), m.logodds()
        x, y = batches[0][0][0][:2]
        m.plan_field([(x, y)], inflate_cells=1)
        field = m.plan_cost_field()
        kern = match.kernel_table(0.1, 0.05, 4)
        poses, ranges = batches[-1]
        first = m.match_scans(poses, ranges, amin, inc, [0.0], 0, 5, 2, 1, 4, kern)
        m.profile(True)
        m.profile_reset()
        views = [(x, y), tuple(batches[-1][0][0][:2])]
        g, c = m.gain_views(views, 40)
        np.testing.assert_array_equal(g, _host(m, st, views, 40)[0])
        assert g.sum() > 0
        np.testing.assert_array_equal(m.state(), st)
        assert m.logodds().tobytes() == L.tobytes()
        np.testing.assert_array_equal(m.plan_cost_field(), field)  # no DM_ERR_STATE: the map version did not move
        again = m.match_scans(poses, ranges, amin, inc, [0.0], 0, 5, 2, 1, 4, kern)
        np.testing.assert_array_equal(again["score"], first["score"])
        prof = m.profile_read()
        assert prof["gain_views"][0] == 1
        assert prof.get("match_field", (0, 0.0))[0] == 0  # the matcher's field was kept
    finally:
        m.close()


def _check_goals(m, st, clusters, robots, cache, **kw):
    p = m.params
    got = m.assign_goals_gain(robots, **kw)
    exp = gain.assign_goals_gain(st, clusters, robots, p.origin_x, p.origin_y, p.resolution, cache=cache, **kw)
    assert len(got) == len(exp) == len(robots)
    for g, e in zip(got, exp):
        if e is None:
            assert g is None
        else:
            assert g is not None and g[0] == e[0] and g[2] == e[2] and g[3] == e[3]
            assert g[1] == e[1]  # the same doubles
    return got


def test_goals_by_gain_on_mapped_world():
    p, batches, amin, inc = cases.world_case(51, 512, 512, 0.05, 4, 720, 3, region_frac=0.7)
    m = dm.OccupancyMapper(p)
    try:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        cl = m.frontiers().clusters
        st = m.state()
        assert len(cl) > 10
        robots = np.concatenate([batches[-1][0][:, :2], batches[0][0][:, :2]])[:8]
        cache = {}
        some = 0
        sets = (dict(min_size=8, min_gain=0), dict(min_size=1, min_gain=30, distance_weight=0.25, min_distance=1.0))
        for R in (1, 8):
            for kw in sets:
                got = _check_goals(m, st, cl, robots[:R], cache, inflate_cells=2, snap_cells=5, radius_cells=40, **kw)
                some += sum(g is not None for g in got)
        assert some > 0
        # the memo's hit path (two robots at one pose snap every centroid alike)
        # and its miss path (robots far apart snap some centroids differently,
        # or reach different clusters)
        same = np.array([robots[0], robots[0], robots[5]])
        got = _check_goals(m, st, cl, same, cache, inflate_cells=2, snap_cells=5, radius_cells=40, **sets[0])
        if got[0] is not None and got[1] is not None:
            assert got[0][0] != got[1][0]
        apart = np.array([robots[7], robots[2], robots[4]])
        _check_goals(m, st, cl, apart, cache, inflate_cells=2, snap_cells=5, radius_cells=40, **sets[1])
        # the field left behind is the last robot's
        last = plan.cell_of(apart[2][0], apart[2][1], p.origin_x, p.origin_y, p.resolution, 512, 512)
        np.testing.assert_array_equal(m.plan_cost_field(), cache[last])
    finally:
        m.close()


def test_policy_case_sliver_against_doorway():
    st = np.full((128, 128), -1, np.int8)
    st[9:101, 9:61] = 100
    st[10:100, 10:60] = 0
    st[20:80, 60] = -1      # the sliver
    st[19:81, 61] = 100     # backed by a wall
    st[84:88, 9] = 0        # the four-cell doorway
    m = _mapper(st, min_frontier_size=1)
    try:
        p = m.params
        g, _ = m.gain_views([_centre(p, 59, 50), _centre(p, 10, 86)], 40)
        assert list(g) == [60, 189]
        cl = m.frontiers().clusters
        cx = np.floor((cl["cx_m"] - p.origin_x) / p.resolution)
        robot = [_centre(p, 35, 50)]
        kw = dict(min_size=1, inflate_cells=1, snap_cells=3)
        by_path = m.assign_goals_path(robot, **kw)[0]
        exp_path = plan.assign_goals_path(st, cl, robot, p.origin_x, p.origin_y, p.resolution, **kw)[0]
        assert by_path[0] == exp_path[0] and cx[by_path[0]] == 59 and cl["size"][by_path[0]] >= 60
        by_gain = _check_goals(m, st, cl, robot, {}, radius_cells=40, **kw)[0]
        assert cx[by_gain[0]] == 9 and cl["size"][by_gain[0]] == 4 and by_gain[3] > 60
    finally:
        m.close()


def _code(fn):
    with pytest.raises(dm.DmError) as e:
        fn()
    return e.value.code


def test_errors():
    m = dm.OccupancyMapper(cases.make_params(128, 128))
    try:
        for R in (0, 512, -3):
            assert _code(lambda: m.gain_views([(0.0, 0.0)], R)) == _ffi.DM_ERR_INVALID_ARG
        lib, xy = dm.load_library(), np.zeros(2)
        g, c = np.zeros(1, np.uint32), np.zeros(1, np.int64)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert lib.dm_gain_views(m._handle(), vp(xy), -1, 8, vp(g), vp(c)) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_gain_views(m._handle(), vp(xy), (1 << 20) + 1, 8, vp(g), vp(c)) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_gain_views(m._handle(), None, 1, 8, vp(g), vp(c)) == _ffi.DM_ERR_INVALID_ARG
        assert lib.dm_gain_views(m._handle(), vp(xy), 1, 8, None, vp(c)) == _ffi.DM_ERR_INVALID_ARG
        # no collected result, as dm_assign_goals
        assert _code(lambda: m.assign_goals_gain([(0.0, 0.0)])) == _ffi.DM_ERR_INVALID_ARG
        m.frontiers()
        assert m.assign_goals_gain([(0.0, 0.0), (1.0, 1.0)]) == [None, None]
        for bad in (dict(min_gain=-1), dict(radius_cells=0), dict(radius_cells=512), dict(distance_weight=-1.0),
                    dict(inflate_cells=33), dict(snap_cells=17)):
            assert _code(lambda: m.assign_goals_gain([(0.0, 0.0)], **bad)) == _ffi.DM_ERR_INVALID_ARG, bad
        assert _code(lambda: m.assign_goals_gain(np.zeros((257, 2)))) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.assign_goals_gain([(0.0, 0.0), (1e6, 0.0)])) == _ffi.DM_ERR_INVALID_ARG  # outside
        assert m.gain_views([(0.0, 0.0)], 8)[0][0] == 197  # the handle is still good: the disc of radius 8
    finally:
        m.close()
    band = dm.OccupancyMapper(cases.make_params(128, 128, band_row0=0, band_rows=64))
    try:
        assert _code(lambda: band.gain_views([(0.0, 0.0)], 8)) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: band.assign_goals_gain([(0.0, 0.0)])) == _ffi.DM_ERR_INVALID_ARG
    finally:
        band.close()
    sharded = dm.OccupancyMapper(cases.make_params(128, 128), devices=[0, 0])
    try:
        for call in (lambda: sharded.gain_views([(0.0, 0.0)], 8), lambda: sharded.assign_goals_gain([(0.0, 0.0)])):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG and "sharded" in str(e.value)
    finally:
        sharded.close()

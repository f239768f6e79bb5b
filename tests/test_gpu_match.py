"""GPU: the device scan matcher (dm_match_field, dm_match_scans,
csrc/dm_match.h) against its host restatement dm.match, bit for bit: response
fields on one tile, ragged tiles and across tile corners, score volumes with
negative fine coordinates, unused beams and a NaN pose, beams spread over
several tiles and beam chunks, ties, the absence of side effects, the error
paths, and the two-stage wrapper."""
import numpy as np
import pytest

import cases
import dm
import match_cases
from dm import _ffi, match
from dm.ros_node import LaserScan

pytestmark = pytest.mark.gpu

GAUSS = {r: match.kernel_table(0.1, 0.05, r) for r in (0, 1, 4, 8, 15, 16)}


def _mapper(st, **kw):
    H, W = st.shape
    m = dm.OccupancyMapper(cases.make_params(W, H, **kw))
    m.set_state(st)
    return m


def _random_state(seed, H, W, p_occ=0.05):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, -1, 100], np.int8), size=(H, W), p=[0.75 - p_occ, 0.25, p_occ])


def _wild_table(r, seed=1):
    k = np.random.default_rng(seed).integers(0, 256, r * r + 1).astype(np.uint8)
    assert r == 0 or np.any(np.diff(k.astype(int)) > 0)  # not monotone
    return k


@pytest.mark.parametrize("H,W", [(64, 64), (70, 130)])
def test_field_random_maps(H, W):
    """One tile, and 130 x 70: a ragged last tile column and row."""
    st = _random_state(21, H, W)
    m = _mapper(st)
    try:
        for r in (0, 1, 8, 16):
            np.testing.assert_array_equal(m.match_field(r, GAUSS[r]), match.response_field(st, r, GAUSS[r]))
    finally:
        m.close()


def test_field_discs_across_tiles_and_the_grid_edge():
    """Single occupied cells at tile corners: the discs span up to four tiles
    and are cut by the grid edge."""
    st = np.zeros((192, 192), np.int8)
    for x, y in ((63, 63), (64, 0), (127, 128), (0, 191)):
        st[y, x] = 100
    m = _mapper(st)
    try:
        for r in (16, 15):
            got = m.match_field(r, GAUSS[r])
            np.testing.assert_array_equal(got, match.response_field(st, r, GAUSS[r]))
            assert got[63 + r, 63] == GAUSS[r][r * r] and got[63, 63] == 255
    finally:
        m.close()


@pytest.mark.parametrize("r", [3, 16])
def test_field_non_monotone_table(r):
    """The maximum over the disc, not the value at the nearest occupied cell."""
    st = _random_state(22, 70, 130, p_occ=0.02)
    kern = _wild_table(r)
    m = _mapper(st)
    try:
        np.testing.assert_array_equal(m.match_field(r, kern), match.response_field(st, r, kern))
        # and the table is part of the field's identity: the next one is not served from the last
        gauss = match.kernel_table(0.1, 0.05, r)
        np.testing.assert_array_equal(m.match_field(r, gauss), match.response_field(st, r, gauss))
    finally:
        m.close()


def test_field_with_untouched_tiles():
    """Only one tile was ever written (set_state of a map unknown elsewhere):
    the other tiles are never read, yet the smear of the cells at that tile's
    edges reaches into them."""
    st = np.full((192, 192), -1, np.int8)
    st[64:128, 64:128] = _random_state(23, 64, 64, p_occ=0.03)
    st[64, 64] = st[127, 127] = st[64, 127] = st[100, 64] = 100
    m = _mapper(st)
    try:
        got = m.match_field(8, GAUSS[8])
        np.testing.assert_array_equal(got, match.response_field(st, 8, GAUSS[8]))
        assert got[60, 60] > 0 and got[130, 130] > 0  # in tiles nothing touched
    finally:
        m.close()


def _scans(p, seed, N=37, reach=2.0):
    """Three scans: one from the grid's lower-left corner cell (negative fine
    coordinates, cells out of the grid), one with NaNs and ranges below
    range_min and above range_max, one with a NaN pose."""
    rng = np.random.default_rng(seed)
    poses = np.array([[p.origin_x + 0.031, p.origin_y + 0.017, 0.7],
                      [p.origin_x + 0.5 * p.width * p.resolution + 0.013,
                       p.origin_y + 0.5 * p.height * p.resolution - 0.021, -2.1],
                      [np.nan, 0.0, 0.1]])
    ranges = rng.uniform(0.05, reach, (3, N)).astype(np.float32)
    ranges[1, ::5] = np.nan
    ranges[1, 1::7] = 0.01
    ranges[1, 2::6] = 12.5
    ranges[1, 3] = np.float32(p.range_min)  # the gates are inclusive
    ranges[1, 4] = np.float32(p.range_max)
    return poses, ranges, 0.0, float(np.float32(2 * np.pi / (N - 1)))


def _assert_same(got, exp, volume=True):
    if volume:
        np.testing.assert_array_equal(got["volume"], exp["volume"])
    np.testing.assert_array_equal(got["best"], exp["best"])
    np.testing.assert_array_equal(got["score"], exp["score"])
    np.testing.assert_array_equal(got["n_used"], exp["n_used"])
    assert got["pose"].tobytes() == exp["pose"].tobytes()  # NaNs included


@pytest.mark.parametrize("H,W", [(64, 64), (70, 130)])
@pytest.mark.parametrize("half", [0, 3, 32])
def test_full_volume(H, W, half):
    st = _random_state(31, H, W, p_occ=0.08)
    m = _mapper(st)
    p = m.params
    poses, ranges, amin, inc = _scans(p, 32)
    off = np.array([-0.07, -0.03, 0.0, 0.02, 0.09])
    r, kern = 4, GAUSS[4]
    V = match.response_field(st, r, kern)
    try:
        for sub in (1, 5, 16):
            for stride in (1, 2):
                got = m.match_scans(poses, ranges, amin, inc, off, 2, sub, half, stride, r, kern, want_volume=True)
                exp = match.match_scans(st, p, poses, ranges, amin, inc, off, 2, sub, half, stride, r, kern, field=V)
                _assert_same(got, exp)
                assert exp["n_used"][0] == 37 and 0 < exp["n_used"][1] < 37 and exp["volume"][0].max() > 0
                assert got["n_used"][2] == 0 and got["best"][2].tolist() == [2, 0, 0] and got["score"][2] == 0
                if half:
                    qx, _, used = match.fine_coords(p, poses, ranges, amin, inc, off, sub)
                    assert (qx[0][used[0]] - half * stride).min() < 0
    finally:
        m.close()


def test_beams_over_several_tiles_and_chunks():
    """256 x 256, one scan of 1024 beams up to 5 m long: several beam chunks
    per candidate yaw, endpoints in many tiles."""
    st = _random_state(41, 256, 256, p_occ=0.06)
    m = _mapper(st)
    p = m.params
    rng = np.random.default_rng(42)
    N = 1024
    ranges = rng.uniform(0.05, 5.0, (1, N)).astype(np.float32)
    ranges[0, ::97] = np.nan
    poses = [(0.4, -0.3, 1.1)]
    inc = float(np.float32(2 * np.pi / (N - 1)))
    off = np.array([-0.02, 0.0, 0.02])
    try:
        got = m.match_scans(poses, ranges, 0.0, inc, off, 1, 5, 4, 2, 4, GAUSS[4], want_volume=True)
        exp = match.match_scans(st, p, poses, ranges, 0.0, inc, off, 1, 5, 4, 2, 4, GAUSS[4])
        _assert_same(got, exp)
        qx, qy, used = match.fine_coords(p, poses, ranges, 0.0, inc, off, 5)
        tiles = set(zip((qx[0, 1][used[0, 1]] // 5 // 64).tolist(), (qy[0, 1][used[0, 1]] // 5 // 64).tolist()))
        assert len(tiles) >= 9
        # without the volume the same best candidate comes back
        _assert_same(m.match_scans(poses, ranges, 0.0, inc, off, 1, 5, 4, 2, 4, GAUSS[4]), exp, volume=False)
    finally:
        m.close()


def test_ties():
    """An empty map scores 0 everywhere: (k0, 0, 0).  A map symmetric about
    the pose, and one occupied everywhere, give several candidates the maximum;
    the tie rule picks one."""
    p = cases.make_params(64, 64)
    N = 36
    inc = float(np.float32(2 * np.pi / N))
    ranges = np.full((1, N), 1.0, np.float32)
    off = np.array([-inc, 0.0, inc])  # rotations by one beam: the ring below looks the same
    ring = np.zeros((64, 64), np.int8)
    yy, xx = np.mgrid[0:64, 0:64]
    d2 = (xx - 31.5) ** 2 + (yy - 31.5) ** 2
    ring[(d2 >= 19.0 ** 2) & (d2 <= 21.0 ** 2)] = 100
    kern = match.kernel_table(0.1, 0.05, 2)
    for st in (np.full((64, 64), -1, np.int8), ring, np.full((64, 64), 100, np.int8)):
        m = _mapper(st)
        try:
            got = m.match_scans([(0.0, 0.0, 0.0)], ranges, 0.0, inc, off, 1, 5, 3, 1, 2, kern, want_volume=True)
            exp = match.match_scans(st, p, [(0.0, 0.0, 0.0)], ranges, 0.0, inc, off, 1, 5, 3, 1, 2, kern)
            _assert_same(got, exp)
            assert (exp["volume"] == exp["volume"].max()).sum() > 1  # a real tie
            if not (st == 100).any():
                assert got["best"][0].tolist() == [1, 0, 0] and got["score"][0] == 0 and got["n_used"][0] == N
        finally:
            m.close()


def test_no_side_effects():
    world = cases.world_case(3, 128, 128, 0.05, 2, 90, 2)
    p, batches, amin, inc = world
    m = dm.OccupancyMapper(p)
    try:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        st, L = m.state(), m.logodds()
        x, y = batches[0][0][0][:2]
        m.plan_field([(x, y)], inflate_cells=1)
        field = m.plan_cost_field()
        m.match_field(4, GAUSS[4])
        poses, ranges = batches[-1]
        got = m.match_scans(poses, ranges, amin, inc, [-0.05, 0.0, 0.05], 1, 5, 6, 2, 4, GAUSS[4], want_volume=True)
        _assert_same(got, match.match_scans(st, p, poses, ranges, amin, inc, [-0.05, 0.0, 0.05], 1, 5, 6, 2, 4,
                                            GAUSS[4]))
        assert got["score"].min() > 0
        np.testing.assert_array_equal(m.state(), st)
        assert m.logodds().tobytes() == L.tobytes()
        np.testing.assert_array_equal(m.plan_cost_field(), field)  # still valid: the map version did not move
        # a changed map is matched as it is now, not from the kept field
        m.integrate(*batches[0], amin, inc)
        st2 = m.state()
        got = m.match_scans(poses, ranges, amin, inc, [0.0], 0, 5, 2, 1, 4, GAUSS[4], want_volume=True)
        _assert_same(got, match.match_scans(st2, p, poses, ranges, amin, inc, [0.0], 0, 5, 2, 1, 4, GAUSS[4]))
    finally:
        m.close()


def _code(fn):
    with pytest.raises(dm.DmError) as e:
        fn()
    return e.value.code


def test_errors():
    st = _random_state(51, 64, 64)
    ranges = np.full((1, 8), 1.0, np.float32)
    ok = dict(poses=[(0.0, 0.0, 0.0)], ranges=ranges, angle_min=0.0, angle_increment=0.7, yaw_offsets=[-0.1, 0.0, 0.1],
              k0=1, sub=5, half=2, stride=1, smear_cells=4, kern=GAUSS[4])
    m = _mapper(st)
    try:
        m.match_scans(**ok)
        big = np.zeros(17 * 17 + 1, np.uint8)
        for bad in (dict(smear_cells=17, kern=big), dict(smear_cells=-1), dict(sub=0), dict(sub=17), dict(half=33),
                    dict(half=-1), dict(stride=0), dict(stride=17), dict(yaw_offsets=[], k0=0),
                    dict(yaw_offsets=np.zeros(65)), dict(k0=3), dict(k0=-1), dict(kern=None)):
            assert _code(lambda: m.match_scans(**{**ok, **bad})) == _ffi.DM_ERR_INVALID_ARG, bad
        assert _code(lambda: m.match_field(17, big)) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: m.match_field(4, None)) == _ffi.DM_ERR_INVALID_ARG
        m.match_scans(**ok)  # the handle is still good
    finally:
        m.close()
    band = dm.OccupancyMapper(cases.make_params(64, 128, band_row0=0, band_rows=64))
    try:
        assert _code(lambda: band.match_scans(**ok)) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: band.match_field(4, GAUSS[4])) == _ffi.DM_ERR_INVALID_ARG
    finally:
        band.close()
    sharded = dm.OccupancyMapper(cases.make_params(64, 128), devices=[0, 0])
    try:
        assert _code(lambda: sharded.match_scans(**ok)) == _ffi.DM_ERR_INVALID_ARG
        assert _code(lambda: sharded.match_field(4, GAUSS[4])) == _ffi.DM_ERR_INVALID_ARG
    finally:
        sharded.close()


def test_two_stage_wrapper_on_the_recovery_case():
    p, st, ranges, amin, inc, true, prior = match_cases.recovery_case()
    exp = match.two_stage(st, p, ranges, amin, inc, prior)
    m = dm.OccupancyMapper(p)
    try:
        m.set_state(st)
        got = m.match_scan(LaserScan(angle_min=amin, angle_increment=inc, ranges=ranges), prior)
    finally:
        m.close()
    assert got["pose"] == exp["pose"] and got["response"] == exp["response"]
    assert (got["score"], got["n_used"]) == (exp["score"], exp["n_used"])
    assert got["coarse"] == {k: exp["coarse"][k] for k in got["coarse"]}
    assert got["fine"] == {k: exp["fine"][k] for k in got["fine"]}

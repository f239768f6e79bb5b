"""GPU: dm_match_global (csrc/dm_match_global.h) against its host restatement
dm.match.match_global, bit for bit in best, score, n_used and pose, and the
pruned search against the device's exhaustive one: a small ragged map with
ties at every block size and with many rounds, windows and pooled cells at
negative coordinates, the shape limits, the recovery case, the matcher as a
cross-check, field and pool rebuilds, and the error paths."""
import math

import numpy as np
import pytest

import cases
import dm
import match_cases
import match_global_cases as mgc
from dm import _ffi, match

pytestmark = pytest.mark.gpu

BLOCKS = (4, 8, 16, 32)


def _mapper(st, **kw):
    H, W = st.shape
    m = dm.OccupancyMapper(cases.make_params(W, H, **kw))
    m.set_state(st)
    return m


def _assert_same(got, exp):
    np.testing.assert_array_equal(got["best"], exp["best"])
    np.testing.assert_array_equal(got["score"], exp["score"])
    np.testing.assert_array_equal(got["n_used"], exp["n_used"])
    assert got["pose"].tobytes() == exp["pose"].tobytes()  # NaNs included


def _n_blocks(A, half_x, half_y, block):
    return A * (-(-(2 * half_x + 1) // block)) * (-(-(2 * half_y + 1) // block))


def _check_both(m, exp, args, kw, block):
    """Pruned and exhaustive at one block size against the host result `exp`;
    returns the pruned run's stats [S, 4]."""
    pruned = m.match_global(*args, **kw, block=block)
    full = m.match_global(*args, **kw, block=block, exhaustive=True)
    _assert_same(pruned, exp)
    _assert_same(full, exp)
    n = _n_blocks(len(args[4]), kw["half_x"], kw["half_y"], block)
    for s in range(exp["best"].shape[0]):
        assert pruned["stats"][s, 0] == n and full["stats"][s].tolist()[:3] == [n, 0, n]
        assert pruned["stats"][s, 1] in (0, n) and pruned["stats"][s, 2] <= n
    return pruned["stats"]


@pytest.fixture(scope="module")
def ragged():
    st = mgc.ragged_map()
    ranges, amin, inc = mgc.ragged_scans()
    args = ([mgc.RAGGED_PRIOR], ranges, amin, inc, mgc.RAGGED_OFFSETS)
    exp = match.match_global(st, cases.make_params(96, 128), *args, **mgc.RAGGED)
    return st, args, exp


@pytest.mark.parametrize("block", BLOCKS)
def test_small_ragged_map_with_ties(ragged, block):
    st, args, exp = ragged
    m = _mapper(st)
    try:
        stats = _check_both(m, exp, args, mgc.RAGGED, block)
        print(f"block {block}: stats {stats[0].tolist()}, best {exp['best'][0].tolist()}, score {exp['score'][0]}")
        assert exp["score"][0] > 0 and stats[0, 2] > 0 and stats[0, 3] >= 1
    finally:
        m.close()


@pytest.mark.parametrize("block", BLOCKS)
def test_small_ragged_map_in_many_rounds(ragged, block, monkeypatch):
    """DM_MATCH_GLOBAL_BATCH=16 on a fresh handle: the same result in more than one round."""
    st, args, exp = ragged
    monkeypatch.setenv("DM_MATCH_GLOBAL_BATCH", "16")
    m = _mapper(st)
    try:
        stats = _check_both(m, exp, args, mgc.RAGGED, block)
        print(f"block {block}: stats {stats[0].tolist()}")
        assert stats[0, 3] > 1
    finally:
        m.close()


@pytest.mark.parametrize("block", BLOCKS)
def test_corner_prior(block):
    """The prior 3 cells from the lower-left corner, half 40: windows and pooled
    cells at negative coordinates, endpoints out of the grid."""
    st = mgc.ragged_map()
    p = cases.make_params(96, 128)
    ranges, amin, inc = mgc.ragged_scans()
    prior = (p.origin_x + 3.5 * p.resolution, p.origin_y + 3.5 * p.resolution, 0.2)
    args = ([prior], ranges, amin, inc, mgc.RAGGED_OFFSETS)
    kw = dict(mgc.RAGGED, half_x=40, half_y=40)
    exp = match.match_global(st, p, *args, **kw)
    qx, qy, used = match.fine_coords(p, *args, 1)
    assert (qx[0][used[0]] - 40).min() < -31 and (qx[0][used[0]] < 0).any() and exp["score"][0] > 0
    m = _mapper(st)
    try:
        _check_both(m, exp, args, kw, block)
    finally:
        m.close()


def test_shape_limits():
    st = mgc.ragged_map()
    p = cases.make_params(96, 128)
    ranges, amin, inc = mgc.ragged_scans(S=2)
    poses = [mgc.RAGGED_PRIOR, (-0.9, 1.1, -2.0)]
    m = _mapper(st)
    try:
        # A = 1
        args = (poses[:1], ranges[:1], amin, inc, [0.1])
        kw = dict(mgc.RAGGED, k0=0)
        _check_both(m, match.match_global(st, p, *args, **kw), args, kw, 8)
        # a window of one translation
        args = (poses[:1], ranges[:1], amin, inc, mgc.RAGGED_OFFSETS)
        kw = dict(mgc.RAGGED, half_x=0, half_y=0)
        exp = match.match_global(st, p, *args, **kw)
        assert exp["best"][0, 1:].tolist() == [0, 0]
        for block in BLOCKS:
            _check_both(m, exp, args, kw, block)
        # one translation along y only, and S = 2 with different results, smeared
        kern = match.kernel_table(0.1, 0.05, 4)
        args = (poses, ranges, amin, inc, mgc.RAGGED_OFFSETS)
        kw = dict(mgc.RAGGED, half_y=0, smear_cells=4, kern=kern)
        exp = match.match_global(st, p, *args, **kw)
        assert exp["best"][0].tolist() != exp["best"][1].tolist()
        _check_both(m, exp, args, kw, 4)
        _check_both(m, exp, args, kw, 16)
    finally:
        m.close()
    # an all-unknown map, and one nothing was ever written to
    for fresh in (False, True):
        m = dm.OccupancyMapper(p)
        try:
            if not fresh:
                m.set_state(np.full((128, 96), -1, np.int8))
            args = (poses[:1], ranges[:1], amin, inc, mgc.RAGGED_OFFSETS)
            for ex in (False, True):
                got = m.match_global(*args, **mgc.RAGGED, block=8, exhaustive=ex)
                assert got["best"][0].tolist() == [4, 0, 0] and got["score"][0] == 0 and got["n_used"][0] == 22
                assert got["pose"][0].tolist() == [0.3, -0.4, 0.2 + 0.0]
            assert got["stats"][0, 2] == got["stats"][0, 0]
            assert m.match_global(*args, **mgc.RAGGED, block=8)["stats"][0].tolist()[2:] == [0, 0]
        finally:
            m.close()


@pytest.fixture(scope="module")
def recovery_mapper():
    c = mgc.recovery()
    m = dm.OccupancyMapper(c["p"])
    m.set_state(c["st"])
    yield m
    m.close()


@pytest.mark.parametrize("block", [8, 16])
def test_recovery_case(recovery_mapper, block):
    """A = 64, half 100, a prior off by (2.3, -1.7, 0.9): the host's result, and
    the pruned run refines at most 1 % of its blocks (2 of 43,264 are needed at
    block 8: the cap only rules out pruning that does nothing)."""
    c = mgc.recovery()
    exp = mgc.recovery_host(100)
    args = ([c["prior"]], c["ranges"], c["amin"], c["inc"], c["off"])
    kw = dict(k0=c["k0"], half_x=100, half_y=100, smear_cells=4, kern=c["kern"])
    stats = _check_both(recovery_mapper, exp, args, kw, block)
    print(f"block {block}: stats {stats[0].tolist()}")
    assert exp["best"][0, 1:].tolist() == [-46, 34]
    assert stats[0, 1] == stats[0, 0] and 100 * int(stats[0, 2]) <= int(stats[0, 0])


def test_recovery_case_whole_map(recovery_mapper):
    """The whole 400^2 map from its centre, A = 180: pruned against exhaustive, on the device only."""
    c = mgc.recovery()
    gp = match.global_params(None, 0.05, 400, 400)
    assert len(gp["yaw_offsets"]) == 180
    args = ([(0.0, 0.0, 0.0)], c["ranges"], c["amin"], c["inc"], gp["yaw_offsets"])
    kw = dict(k0=gp["k0"], half_x=200, half_y=200, smear_cells=4, kern=c["kern"])
    full = recovery_mapper.match_global(*args, **kw, block=16, exhaustive=True)
    for block in (8, 16):
        pruned = recovery_mapper.match_global(*args, **kw, block=block)
        _assert_same(pruned, full)
        print(f"block {block}: stats {pruned['stats'][0].tolist()}, best {pruned['best'][0].tolist()}")
        assert 100 * int(pruned["stats"][0, 2]) <= int(pruned["stats"][0, 0])
    res = 0.05
    assert abs(full["pose"][0, 0] - c["true"][0]) <= res and abs(full["pose"][0, 1] - c["true"][1]) <= res
    assert match_cases.yaw_error(full["pose"][0, 2], c["true"][2]) <= 0.5 * 0.0349


def test_equals_the_matcher(recovery_mapper):
    """dm_match_scans(sub = 1, stride = 1, half = 16) is the same search."""
    c = mgc.recovery()
    _, _, _, _, _, _, prior = match_cases.recovery_case()
    args = ([prior], c["ranges"], c["amin"], c["inc"], c["off"])
    exp = recovery_mapper.match_scans(*args, c["k0"], 1, 16, 1, 4, c["kern"])
    for block, ex in ((8, False), (32, False), (16, True)):
        got = recovery_mapper.match_global(*args, k0=c["k0"], half_x=16, half_y=16, smear_cells=4, kern=c["kern"],
                                           block=block, exhaustive=ex)
        _assert_same(got, exp)
    assert exp["score"][0] > 0


def test_field_and_version():
    """A changed map is searched as it is now (field and pool are rebuilt), and
    the call leaves the map, its version and a dm_plan_field result alone."""
    p, batches, amin, inc = cases.world_case(3, 128, 128, 0.05, 2, 90, 2)
    m = dm.OccupancyMapper(p)
    kern = match.kernel_table(0.1, 0.05, 4)
    off, k0 = mgc.full_circle(16)
    kw = dict(k0=k0, half_x=30, half_y=25, smear_cells=4, kern=kern)
    try:
        m.integrate(*batches[0], amin, inc)
        poses, ranges = batches[-1]
        x, y = batches[0][0][0][:2]
        m.plan_field([(x, y)], inflate_cells=1)
        field = m.plan_cost_field()
        st, L = m.state(), m.logodds()
        args = (poses, ranges, amin, inc, off)
        exp = match.match_global(st, p, *args, **kw)
        _check_both(m, exp, args, kw, 8)
        np.testing.assert_array_equal(m.state(), st)
        assert m.logodds().tobytes() == L.tobytes()
        np.testing.assert_array_equal(m.plan_cost_field(), field)  # still valid: the map version did not move
        m.integrate(*batches[1], amin, inc)
        st2 = m.state()
        assert (st2 != st).any()
        exp2 = match.match_global(st2, p, *args, **kw)
        _check_both(m, exp2, args, kw, 8)
        assert exp2["score"].min() > 0
    finally:
        m.close()


def _code(fn):
    with pytest.raises(dm.DmError) as e:
        fn()
    return e.value.code


def test_errors():
    st = mgc.ragged_map()
    ranges, amin, inc = mgc.ragged_scans()
    kern4 = match.kernel_table(0.1, 0.05, 4)
    ok = dict(poses=[mgc.RAGGED_PRIOR], ranges=ranges, angle_min=amin, angle_increment=inc,
              yaw_offsets=mgc.RAGGED_OFFSETS, k0=4, half_x=5, half_y=5, smear_cells=4, kern=kern4, block=8)
    m = _mapper(st)
    try:
        m.match_global(**ok)
        for bad in (dict(block=5), dict(block=0), dict(block=64), dict(half_x=4097), dict(half_y=4097),
                    dict(half_x=-1), dict(yaw_offsets=np.zeros(1025)), dict(yaw_offsets=[], k0=0), dict(k0=8),
                    dict(k0=-1), dict(kern=None), dict(smear_cells=17, kern=np.zeros(17 * 17 + 1, np.uint8))):
            assert _code(lambda: m.match_global(**{**ok, **bad})) == _ffi.DM_ERR_INVALID_ARG, bad
        with pytest.raises(dm.DmError) as e:
            m.match_global(**{**ok, "yaw_offsets": np.zeros(1024), "half_x": 4096, "half_y": 4096, "block": 4})
        assert e.value.code == _ffi.DM_ERR_CAPACITY and str(1024 * 2049 * 2049) in str(e.value)
        assert "block" in str(e.value)
        m.match_global(**ok)  # the handle is still good
    finally:
        m.close()
    band = dm.OccupancyMapper(cases.make_params(64, 128, band_row0=0, band_rows=64))
    try:
        assert _code(lambda: band.match_global(**ok)) == _ffi.DM_ERR_INVALID_ARG
    finally:
        band.close()
    sharded = dm.OccupancyMapper(cases.make_params(64, 128), devices=[0, 0])
    try:
        assert _code(lambda: sharded.match_global(**ok)) == _ffi.DM_ERR_INVALID_ARG
    finally:
        sharded.close()

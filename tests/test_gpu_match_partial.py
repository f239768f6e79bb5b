"""GPU: the matchers on a partially built response field.  dm_match_scans and
dm_match_global build only the 64 x 64 tiles their search windows can reach
and keep host flags of what the field and the pooled field hold; a tile a
window reads but the host did not list would be read stale, silently.  On
tests/match_partial_cases.py's 500 x 390 map (56 tiles) with range_max = 1.6 m
a window reaches a handful of tiles, so every case here checks three things:

  (a) the results equal dm.match's on the full host field of the state the
      mapper reports, bit for bit (volume, best, score, n_used, pose bytes);
  (b) the built flags (dm_match_built) cover match_partial_cases.tiles_read;
  (c) the flags stay under a cap, which proves the partial path ran: 14 of 56
      tiles for one pose of dm_match_scans, 28 of 56 for dm_match_global and
      for calls with several poses that reach the map.

The cases: a field poisoned by another table first, windows that end on a
tile's first or last column or row, incremental builds, table changes, every
map writer, poses over the map's edges and off it, and dm_match_global's pool
across blocks, scans, calls, tables and map writes."""
import ctypes

import numpy as np
import pytest

import cases
import dm
import match_partial_cases as mpc
from dm import _ffi, match

pytestmark = pytest.mark.gpu

NT = mpc.TX * mpc.TY
CAP_ONE, CAP_WIDE = 14, 28


def _mapper(poisoned=False, st=None):
    m = dm.OccupancyMapper(mpc.params())
    m.set_state(mpc.state() if st is None else st)
    if poisoned:  # every tile holds the response of another table
        m.match_field(mpc.SMEAR, mpc.POISON)
        assert m.match_built()[0].all()
    return m


def _assert_same(got, exp, volume=True):
    if volume:
        np.testing.assert_array_equal(got["volume"], exp["volume"])
    np.testing.assert_array_equal(got["best"], exp["best"])
    np.testing.assert_array_equal(got["score"], exp["score"])
    np.testing.assert_array_equal(got["n_used"], exp["n_used"])
    assert got["pose"].tobytes() == exp["pose"].tobytes()


def _assert_covers(flags, need, cap):
    print(f"built {int(flags.sum())} of {NT} tiles, read {int(need.sum())}, cap {cap}")
    assert not (need & ~flags).any(), np.argwhere(need & ~flags).tolist()  # (b)
    assert flags.sum() <= cap, int(flags.sum())                           # (c)


def _check_scans(m, poses, cap, search=mpc.SEARCHES[0], kern=mpc.GAUSS4, smear=mpc.SMEAR, rng=None):
    """One dm_match_scans call checked for (a), (b), (c); returns (result, flags)."""
    args = mpc.scan_args(poses, search, kern, smear, rng)
    exp = mpc.host_scans(m.state(), args)
    got = m.match_scans(*args, want_volume=True)
    _assert_same(got, exp)  # (a)
    flags, _ = m.match_built()
    _assert_covers(flags, mpc.tiles_read_scans(poses, search, rng=args[1]), cap)
    return got, flags


def _n_blocks(block, half_x=mpc.G_HALF_X, half_y=mpc.G_HALF_Y):
    return len(mpc.G_OFFSETS) * (-(-(2 * half_x + 1) // block)) * (-(-(2 * half_y + 1) // block))


def _check_global(m, poses, block, exhaustive, cap=CAP_WIDE, kw=None, rng=None):
    """One dm_match_global call checked for (a), (b), (c); returns (result, flags, n_pool)."""
    kw = mpc.global_kw() if kw is None else kw
    args = mpc.global_args(poses, rng)
    exp = mpc.host_global(m.state(), args, kw)
    got = m.match_global(*args, **kw, block=block, exhaustive=exhaustive)
    _assert_same(got, exp, volume=False)  # (a)
    flags, n_pool = m.match_built()
    _assert_covers(flags, mpc.tiles_read_global(poses, kw["half_x"], kw["half_y"], rng=args[1]), cap)
    assert (got["stats"][:, 0] == _n_blocks(block, kw["half_x"], kw["half_y"])).all()
    return got, flags, n_pool


def _check_both(m, poses, block, **kw):
    """Pruned, then exhaustive, as test_gpu_match_global's _check_both; the two agree."""
    pruned, _, n_pool = _check_global(m, poses, block, False, **kw)
    full, flags, _ = _check_global(m, poses, block, True, **kw)
    _assert_same(pruned, full, volume=False)
    n = pruned["stats"][0, 0]
    for s in range(pruned["best"].shape[0]):
        assert full["stats"][s].tolist()[:3] in ([n, 0, n], [n, 0, 0])  # [n, 0, 0]: the window misses the map
        assert pruned["stats"][s, 1] in (0, n) and pruned["stats"][s, 2] <= n
    return pruned, flags, n_pool


# ---- dm_match_built itself ---------------------------------------------------------
def test_built_entry():
    m = _mapper()
    lib = m._lib
    nf, npool = ctypes.c_int64(-1), ctypes.c_int64(-1)
    try:
        flags, n_pool = m.match_built()
        assert flags.shape == (mpc.TY, mpc.TX) and flags.dtype == bool and not flags.any() and n_pool == 0
        m.match_scans(*mpc.scan_args([mpc.POSE_A]))
        flags, n_pool = m.match_built()
        assert 0 < flags.sum() < NT and n_pool == 0
        # NULL flags: the counts alone
        assert lib.dm_match_built(m._handle(), None, 0, ctypes.byref(nf), ctypes.byref(npool)) == 0
        assert (nf.value, npool.value) == (int(flags.sum()), 0)
        buf = np.full(NT + 1, 7, np.uint8)
        rc = lib.dm_match_built(m._handle(), buf.ctypes.data_as(ctypes.c_void_p), NT - 1, ctypes.byref(nf),
                                ctypes.byref(npool))
        assert rc == _ffi.DM_ERR_CAPACITY and (buf == 7).all()
        assert lib.dm_match_built(m._handle(), buf.ctypes.data_as(ctypes.c_void_p), NT, ctypes.byref(nf),
                                  ctypes.byref(npool)) == 0
        assert (buf[:NT].reshape(mpc.TY, mpc.TX) == flags).all() and buf[NT] == 7
        assert lib.dm_match_built(m._handle(), None, 0, None, ctypes.byref(npool)) == _ffi.DM_ERR_INVALID_ARG
    finally:
        m.close()
    for kw in (dict(params=cases.make_params(64, 128, band_row0=0, band_rows=64)),
               dict(params=cases.make_params(64, 128), devices=[0, 0])):
        h = dm.OccupancyMapper(**kw)
        try:
            with pytest.raises(dm.DmError) as e:
                h.match_built()
            assert e.value.code == _ffi.DM_ERR_INVALID_ARG
        finally:
            h.close()


# ---- dm_match_scans ------------------------------------------------------------------
def test_poison_then_partial():
    """All 56 tiles hold another table's response; the call rebuilds what it
    reads, or (a) sees the poison.  The unchanged call again builds nothing."""
    m = _mapper(poisoned=True)
    try:
        got, flags = _check_scans(m, [mpc.POSE_A], CAP_ONE)
        assert got["score"][0] > 0
        again, flags2 = _check_scans(m, [mpc.POSE_A], CAP_ONE)
        _assert_same(again, got)
        assert (flags2 == flags).all()
    finally:
        m.close()


@pytest.mark.parametrize("poisoned", [False, True], ids=["fresh", "poisoned"])
@pytest.mark.parametrize("search", mpc.SEARCHES, ids=lambda s: "sub%d_half%d_stride%d" % s)
@pytest.mark.parametrize("direction", mpc.DIRECTIONS)
def test_tile_edge_reach(direction, search, poisoned):
    """The extreme translation alone reads a tile's first / last column or row
    (pinned in test_match_partial_host.py): a reach one cell short leaves that
    tile unbuilt, and the volume's outermost line differs."""
    pose, _, cell, axis, _ = mpc.edge_pose(direction, search)
    m = _mapper(poisoned)
    try:
        got, flags = _check_scans(m, [pose], CAP_ONE, search)
        line = flags[:, cell // 64] if axis == 0 else flags[cell // 64, :]
        assert line.any() and got["volume"].max() > 0
    finally:
        m.close()


def test_incremental_builds():
    """A, then B, then both in one call, then the whole field: the flags only grow."""
    m = _mapper()
    try:
        _, fa = _check_scans(m, [mpc.POSE_A], CAP_ONE)
        _, fb = _check_scans(m, [mpc.POSE_B], CAP_WIDE, rng=mpc.ranges(2)[1:])
        assert not (fa & ~fb).any() and fb.sum() > fa.sum()
        _, fab = _check_scans(m, [mpc.POSE_A, mpc.POSE_B], CAP_WIDE)
        assert (fab == fb).all()  # both windows were there already
        V = m.match_field(mpc.SMEAR, mpc.GAUSS4)
        flags, _ = m.match_built()
        assert flags.all() and flags.sum() == NT
        np.testing.assert_array_equal(V, match.response_field(mpc.state(), mpc.SMEAR, mpc.GAUSS4))
        _check_scans(m, [mpc.POSE_A, mpc.POSE_B], NT)
    finally:
        m.close()


def test_table_identity_under_partial_builds():
    """Another table of the same radius, then another radius, then back: each
    switch drops every flag, so what is built afterwards is the new window's
    tiles alone (A's and B's windows share no tile)."""
    m = _mapper()
    rb = mpc.ranges(2)[1:]
    try:
        _, fa = _check_scans(m, [mpc.POSE_A], CAP_ONE)
        _, fb = _check_scans(m, [mpc.POSE_B], CAP_ONE, kern=mpc.OTHER4, rng=rb)
        assert not (fa & fb).any()
        _, f6 = _check_scans(m, [mpc.POSE_A], CAP_ONE, kern=mpc.GAUSS6, smear=6)
        assert (f6 == fa).all()
        _, f4 = _check_scans(m, [mpc.POSE_B], CAP_ONE, rng=rb)
        assert (f4 == fb).all()
        # a radius-1 table whose two entries are GAUSS4's first two: the radius is part of the identity
        assert (mpc.GAUSS6[:2] == mpc.GAUSS4[:2]).all()
        _, f = _check_scans(m, [mpc.POSE_B], CAP_ONE, kern=mpc.GAUSS6[:2], smear=1, rng=rb)
        assert (f == fb).all()
    finally:
        m.close()


def _other_state():
    return np.random.default_rng(8).choice(np.array([0, -1, 100], np.int8), size=(mpc.H, mpc.W), p=[0.6, 0.3, 0.1])


def _write_integrate(m, tmp_path):
    m.integrate(np.array([mpc.POSE_A]), mpc.ranges(1, seed=9), mpc.AMIN, mpc.INC)  # a scan inside A's window


def _write_set_state(m, tmp_path):
    m.set_state(_other_state())


def _write_set_logodds(m, tmp_path):
    m.set_logodds(np.random.default_rng(10).uniform(-2.0, 3.5, (mpc.H, mpc.W)).astype(np.float32))


def _write_reset(m, tmp_path):
    m.reset()


def _write_fuse_state(m, tmp_path):
    peer = np.random.default_rng(11).choice(np.array([-1, 0, 100], np.int8), size=(90, 120), p=[0.2, 0.3, 0.5])
    geom = {"width": 120, "height": 90, "resolution": 0.05, "origin_x": mpc.POSE_A[0] - 3.0,
            "origin_y": mpc.POSE_A[1] - 2.25}
    assert m.fuse_state(peer, geom, (0.0, 0.0, 0.0), "add")["changed"] > 0


def _write_load(m, tmp_path):
    other = _mapper(st=_other_state())
    try:
        other.save(str(tmp_path / "other.dm"))
    finally:
        other.close()
    m.load(str(tmp_path / "other.dm"))


WRITERS = {"integrate": _write_integrate, "set_state": _write_set_state, "set_logodds": _write_set_logodds,
           "reset": _write_reset, "fuse_state": _write_fuse_state, "load": _write_load}


@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_every_map_writer_after_a_partial_build(writer, tmp_path):
    """A partial field and a partial pool, then a map write: nothing is built
    any more, and the next matches are the host's on the new state although
    the buffers still hold the old bytes."""
    m = _mapper()
    try:
        before, fa = _check_scans(m, [mpc.POSE_A], CAP_ONE)
        _, _, n_pool = _check_global(m, [mpc.POSE_A], 8, False)
        assert n_pool > 0
        st = m.state()
        WRITERS[writer](m, tmp_path)
        flags, n_pool = m.match_built()
        assert not flags.any() and n_pool == 0
        st2 = m.state()
        assert (st2 != st).any()
        after, _ = _check_scans(m, [mpc.POSE_A], CAP_ONE)
        _, flags, n_pool = _check_global(m, [mpc.POSE_A], 8, False)
        if writer == "reset":
            assert not (st2 == 100).any()
            assert after["best"][0].tolist() == [mpc.K0, 0, 0] and after["score"][0] == 0
            assert after["n_used"][0] == mpc.N and not after["volume"].any()
        else:
            assert n_pool > 0 and (after["volume"] != before["volume"]).any()
    finally:
        m.close()


def test_poses_over_the_edges_and_off_the_map():
    """C in the upper-right corner, D outside the left edge (a negative pose
    cell), E far away with used beams, F with none; then all four and A in one call."""
    r5 = mpc.ranges(5)
    for pose, rng in ((mpc.POSE_C, r5[0:1]), (mpc.POSE_D, r5[1:2])):
        m = _mapper(poisoned=True)
        try:
            got, flags = _check_scans(m, [pose], CAP_ONE, rng=rng)
            assert got["score"][0] > 0 and flags.any()
        finally:
            m.close()
    m = _mapper()
    try:
        # E and F build nothing for themselves
        for search in mpc.SEARCHES:
            got, flags = _check_scans(m, [mpc.POSE_E, mpc.POSE_F], 0, search, rng=r5[2:4])
            assert got["best"].tolist() == [[mpc.K0, 0, 0]] * 2 and got["score"].tolist() == [0, 0]
            assert got["n_used"][1] == 0 and not flags.any()
        assert _check_scans(m, [mpc.POSE_E, mpc.POSE_F], 0, rng=r5[2:4])[0]["n_used"][0] == mpc.N
        poses = [mpc.POSE_C, mpc.POSE_D, mpc.POSE_E, mpc.POSE_F, mpc.POSE_A]
        got, flags = _check_scans(m, poses, CAP_WIDE, rng=r5)
        assert (got["score"][[0, 1, 4]] > 0).all() and got["score"][[2, 3]].tolist() == [0, 0]
    finally:
        m.close()


# ---- dm_match_global --------------------------------------------------------------------
@pytest.mark.parametrize("block", mpc.BLOCKS)
def test_global_pruned_and_exhaustive_at_every_block(block):
    m = _mapper()
    try:
        got, flags, n_pool = _check_both(m, [mpc.POSE_A], block)
        print(f"block {block}: stats {got['stats'][0].tolist()}, pool tiles {n_pool}")
        assert n_pool > 0 and got["score"][0] > 0 and got["stats"][0, 1] == got["stats"][0, 0]
    finally:
        m.close()


def test_global_two_scans_in_one_call_and_in_two():
    """The second scan of one call lands elsewhere: its tiles and pool tiles
    are built between the scans."""
    rb = mpc.ranges(2)[1:]
    m = _mapper(poisoned=True)
    try:
        got2, f2, p2 = _check_both(m, [mpc.POSE_A, mpc.POSE_B], 8)
        assert got2["best"][0].tolist() != got2["best"][1].tolist()
    finally:
        m.close()
    m = _mapper()
    try:
        ga, fa, pa = _check_global(m, [mpc.POSE_A], 8, False)
        gb, fb, pb = _check_global(m, [mpc.POSE_B], 8, False, rng=rb)
        assert not (fa & ~fb).any() and fb.sum() > fa.sum() and pb > pa > 0
        assert (fb == f2).all() and pb == p2  # the same tiles either way
        for k in ("best", "score", "n_used", "pose"):
            assert np.concatenate([ga[k], gb[k]]).tobytes() == got2[k].tobytes()
    finally:
        m.close()


def test_global_block_switches_keep_the_field_and_restart_the_pool():
    m = _mapper()
    try:
        _, f8, p8 = _check_global(m, [mpc.POSE_A], 8, False)
        _, f16, p16 = _check_global(m, [mpc.POSE_A], 16, False)
        assert not (f8 & ~f16).any() and p16 > 0  # the field's flags are kept
        _, f8b, p8b = _check_global(m, [mpc.POSE_A], 8, False)  # mg_pool holds block 16's bytes now
        assert (f8b == f16).all() and p8b == p8
        # B at block 16 after a block-8 pool that never held B's tiles
        _, f, p = _check_global(m, [mpc.POSE_B], 16, False, rng=mpc.ranges(2)[1:])
        assert not (f8b & ~f).any() and p > 0
    finally:
        m.close()


def test_global_exhaustive_first_then_pruned():
    """After the exhaustive call the field tiles are there and the pool is not."""
    m = _mapper()
    try:
        full, ff, p0 = _check_global(m, [mpc.POSE_A], 16, True)
        assert p0 == 0 and ff.any()
        pruned, fp, p1 = _check_global(m, [mpc.POSE_A], 16, False)
        assert p1 > 0 and not (ff & ~fp).any()
        _assert_same(pruned, full, volume=False)
    finally:
        m.close()


def test_global_on_a_poisoned_handle_and_after_a_table_change():
    m = _mapper(poisoned=True)
    try:
        _, _, p = _check_both(m, [mpc.POSE_A], 16)
        assert p > 0
        # the same call under another table: field and pool start over
        kw = mpc.global_kw(kern=mpc.OTHER4)
        _, f, p2 = _check_both(m, [mpc.POSE_B], 16, kw=kw, rng=mpc.ranges(2)[1:])
        assert p2 > 0 and not f[:, :4].any()  # A's tiles were dropped with the table
    finally:
        m.close()


@pytest.mark.parametrize("name", ["C", "D"])
def test_global_over_the_edges(name):
    pose = {"C": mpc.POSE_C, "D": mpc.POSE_D}[name]
    m = _mapper(poisoned=True)
    try:
        for block in (8, 32):
            got, flags, n_pool = _check_both(m, [pose], block)
            assert got["score"][0] > 0 and n_pool > 0
    finally:
        m.close()


def test_global_off_the_map():
    """E has used beams and a window that reaches no tile: nothing is built,
    bounded or scored.  F uses no beam."""
    r = mpc.ranges(2)
    m = _mapper()
    try:
        for ex in (False, True):
            got, flags, n_pool = _check_global(m, [mpc.POSE_E, mpc.POSE_F], 16, ex, cap=0, rng=r)
            n = _n_blocks(16)
            assert got["stats"][0].tolist() == [n, 0, 0, 0] and got["stats"][1].tolist() == [n, 0, 0, 0]
            assert got["best"].tolist() == [[mpc.G_K0, 0, 0]] * 2 and got["score"].tolist() == [0, 0]
            assert got["n_used"].tolist() == [mpc.N, 0]
            assert not flags.any() and n_pool == 0
        # and between two scans that do reach the map
        poses = [mpc.POSE_A, mpc.POSE_E, mpc.POSE_B]
        got, _, _ = _check_both(m, poses, 16, rng=mpc.ranges(3))
        assert got["stats"][1].tolist() == [n, 0, 0, 0] and got["stats"][0, 2] > 0 and got["stats"][2, 2] > 0
    finally:
        m.close()


def test_global_map_write_between_two_pruned_calls():
    m = _mapper()
    try:
        before, _, p = _check_global(m, [mpc.POSE_A], 8, False)
        assert p > 0
        m.set_state(_other_state())
        flags, n_pool = m.match_built()
        assert not flags.any() and n_pool == 0
        after, _, p = _check_global(m, [mpc.POSE_A], 8, False)
        assert p > 0 and after["score"][0] != before["score"][0]
        _check_global(m, [mpc.POSE_A], 8, True)
    finally:
        m.close()


def test_global_half_16_equals_the_matcher_on_a_partial_field():
    """half_x == half_y == 16: the four outputs are dm_match_scans(sub = 1,
    stride = 1, half = 16)'s, here on the tiles the global call built."""
    m = _mapper(poisoned=True)
    kw = mpc.global_kw(half_x=16, half_y=16)
    r = mpc.ranges(1)
    try:
        glob, fg, _ = _check_global(m, [mpc.POSE_A], 8, False, kw=kw)
        args = (np.array([mpc.POSE_A]), r, mpc.AMIN, mpc.INC, mpc.G_OFFSETS, mpc.G_K0, 1, 16, 1, mpc.SMEAR, mpc.GAUSS4)
        got = m.match_scans(*args, want_volume=True)
        _assert_same(got, mpc.host_scans(m.state(), args))
        _assert_same(glob, got, volume=False)
        flags, _ = m.match_built()
        _assert_covers(flags, mpc.tiles_read(args[0], r, mpc.G_OFFSETS, 1, 1, 16), CAP_WIDE)
        assert not (fg & ~flags).any() and got["score"][0] > 0
        _assert_same(m.match_global(*mpc.global_args([mpc.POSE_A]), **kw, block=32, exhaustive=True), got, volume=False)
    finally:
        m.close()

"""CPU: the preconditions of tests/test_gpu_match_partial.py, pinned on the
host restatement so that the GPU cases cannot go vacuous: a search on
match_partial_cases' map reads few of its 56 tiles, the four edge poses read
their outermost tile through the extreme translation alone, the poses A and B
read disjoint tiles, E reads none, F uses no beam, and the expected scores are
above 0."""
import numpy as np
import pytest

import match_partial_cases as mpc
from dm import match


def test_map_and_tables():
    st = mpc.state()
    assert st.shape == (mpc.H, mpc.W) and (mpc.TX, mpc.TY) == (8, 7)
    assert mpc.W % 64 and mpc.H % 64  # ragged last tile column and row
    V = mpc.field(st)
    assert (V > 0).mean() > 0.97
    assert (mpc.field(st, mpc.SMEAR, mpc.POISON) != V).mean() > 0.9  # a tile left from the poison table shows
    assert (mpc.field(st, mpc.SMEAR, mpc.OTHER4) != V).mean() > 0.5
    r = mpc.ranges(3)
    p = mpc.params()
    assert (r[:, sorted(mpc.FULL_BEAMS.values())] == np.float32(p.range_max)).all()
    assert r.min() >= 0.3 and r.max() == np.float32(p.range_max) and (r[0] != r[1]).any()
    assert mpc.RANGE_CELLS * p.resolution == pytest.approx(p.range_max)


def test_pose_a_reads_few_tiles():
    read = mpc.tiles_read_scans([mpc.POSE_A])
    print("pose A reads", int(read.sum()), "tiles:", np.argwhere(read).tolist())
    assert 1 <= read.sum() <= 14
    assert read.sum() == 4  # today's count, far inside the GPU test's cap
    for search in mpc.SEARCHES:
        for d in mpc.DIRECTIONS:
            assert mpc.tiles_read_scans([mpc.edge_pose(d, search)[0]], search).sum() <= 14, (search, d)
    assert mpc.tiles_read_global([mpc.POSE_A]).sum() <= 28
    assert mpc.tiles_read_global([mpc.POSE_A, mpc.POSE_B]).sum() <= 28


@pytest.mark.parametrize("search", mpc.SEARCHES)
@pytest.mark.parametrize("direction", mpc.DIRECTIONS)
def test_edge_pose_reads_its_outermost_tile_by_the_extreme_translation_alone(direction, search):
    sub, half, stride = search
    pose, beam, cell, axis, sign = mpc.edge_pose(direction, search)
    qx, qy, used = match.fine_coords(mpc.params(), [pose], mpc.ranges(1), mpc.AMIN, mpc.INC, mpc.OFFSETS, sub)
    assert used[0, mpc.K0, beam]
    q = (qx, qy)[axis][0, mpc.K0, beam]
    assert (q + sign * half * stride) // sub == cell          # the extreme translation ends in `cell`
    assert (q + sign * (half - 1) * stride) // sub == cell - sign  # the one before it does not
    assert cell % 64 == (0 if sign > 0 else 63)               # a tile's first / last column or row
    other = (qy, qx)[axis][0, mpc.K0, beam] // sub // 64      # the tile index along the other axis
    tile = (other, cell // 64) if axis == 0 else (cell // 64, other)
    read = mpc.tiles_read_scans([pose], search)
    assert read[tile]
    inner = np.arange(-half + 1, half)
    kw = {"i_values": inner} if axis == 0 else {"j_values": inner}
    without = mpc.tiles_read_scans([pose], search, **kw)
    assert not without[tile]
    # nothing but that extreme translation reads the tile column / row at all
    line = without[:, cell // 64] if axis == 0 else without[cell // 64, :]
    assert not line.any()
    assert (read & ~without).any() and not (without & ~read).any()


def test_a_and_b_read_disjoint_tiles():
    a, b = mpc.tiles_read_scans([mpc.POSE_A]), mpc.tiles_read_scans([mpc.POSE_B])
    assert a.any() and b.any() and not (a & b).any()
    ga, gb = mpc.tiles_read_global([mpc.POSE_A]), mpc.tiles_read_global([mpc.POSE_B])
    assert ga.any() and gb.any() and not (ga & gb).any()
    assert gb[:, mpc.TX - 1].any() and not b[:, mpc.TX - 1].any()  # the whole-window search reaches the ragged column
    both = mpc.tiles_read_scans([mpc.POSE_A, mpc.POSE_B])
    assert (both == (a | mpc.tiles_read_scans([mpc.POSE_B], rng=mpc.ranges(2)[1:]))).all()


def test_edge_poses_hang_over_the_map():
    p = mpc.params()
    c = mpc.tiles_read_scans([mpc.POSE_C])
    assert c[mpc.TY - 1, mpc.TX - 1] and c.sum() <= 4
    qx, qy, used = match.fine_coords(p, [mpc.POSE_C], mpc.ranges(1), mpc.AMIN, mpc.INC, mpc.OFFSETS, 1)
    off_map = (qx[used] >= mpc.W) | (qy[used] >= mpc.H)
    assert off_map.mean() > 0.5  # mostly off the map
    d = mpc.tiles_read_scans([mpc.POSE_D])
    assert d[:, 0].any() and not d[:, 1:].any()
    assert np.floor((mpc.POSE_D[0] - p.origin_x) / p.resolution) == -20


def test_e_reads_no_tile_and_f_uses_no_beam():
    p = mpc.params()
    for search in mpc.SEARCHES:
        assert not mpc.tiles_read_scans([mpc.POSE_E], search).any()
        assert not mpc.tiles_read_scans([mpc.POSE_F], search).any()
    assert not mpc.tiles_read_global([mpc.POSE_E, mpc.POSE_F]).any()
    for sub in (1, 5):
        _, _, used = match.fine_coords(p, [mpc.POSE_E, mpc.POSE_F], mpc.ranges(2), mpc.AMIN, mpc.INC, mpc.OFFSETS, sub)
        assert used[0].all() and not used[1].any()
    assert mpc.POSE_F[0] == p.origin_x + 1.5 * 2 ** 30 * p.resolution


def test_expected_scores():
    st = mpc.state()
    poses = [mpc.POSE_A, mpc.POSE_B, mpc.POSE_C, mpc.POSE_D, mpc.POSE_E, mpc.POSE_F]
    exp = mpc.host_scans(st, mpc.scan_args(poses))
    print("match_scans", exp["best"].tolist(), exp["score"].tolist(), exp["n_used"].tolist())
    assert (exp["score"][:4] > 0).all()
    assert exp["score"][4] == 0 and exp["best"][4].tolist() == [mpc.K0, 0, 0] and exp["n_used"][4] == mpc.N
    assert exp["score"][5] == 0 and exp["best"][5].tolist() == [mpc.K0, 0, 0] and exp["n_used"][5] == 0
    glob = mpc.host_global(st, mpc.global_args(poses), mpc.global_kw())
    print("match_global", glob["best"].tolist(), glob["score"].tolist(), glob["n_used"].tolist())
    assert (glob["score"][:4] > 0).all()
    assert glob["score"][4] == 0 and glob["best"][4].tolist() == [mpc.G_K0, 0, 0] and glob["n_used"][4] == mpc.N
    assert glob["n_used"][5] == 0
    # A and B find different poses, so S = 2 in one call has two results to mix up
    assert glob["best"][0].tolist() != glob["best"][1].tolist()
    # a result from the poison table's field is another one
    bad = mpc.host_scans(st, mpc.scan_args([mpc.POSE_A], kern=mpc.POISON))
    assert (bad["volume"] != exp["volume"][:1]).mean() > 0.9

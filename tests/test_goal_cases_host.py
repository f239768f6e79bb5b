"""CPU: the cases of goal_cases.py exercise what they claim (cluster counts on
both sides of the 4096-record chunk and of the 16-chunk merge group, the size
mix, winners that straddle the boundaries, sealed and gain-filtered clusters),
by the restatements and the numpy oracle alone; and the straight-line policy of
dm.goals, the reference of the GPU tests, against an independent replay in
extended precision."""
import numpy as np
import pytest

import goal_cases as gc
from dm import gain, plan
from dm.goals import assign_goals

# the replay below needs a format wider than double: x87 extended or better
assert np.finfo(np.longdouble).nmant >= 63

K_BIG = gc.TWO_LEVELS + 100


def _indices(got):
    return np.array([g[0] if g is not None else -1 for g in got], np.int64)


@pytest.mark.parametrize("K", gc.LATTICE_KS)
def test_lattice_counts_and_sizes(K):
    st, k = gc.lattice_state(K)
    assert k == K and st.shape == (gc.LAT_H, gc.LAT_W)
    cl = gc.lattice_clusters(K)
    assert len(cl) == K
    size = gc.lattice_sizes(K)
    np.testing.assert_array_equal(cl["size"], size)
    assert (np.diff(cl["label"]) > 0).all()
    assert set(np.unique(size)) == {1, 2, 3}
    three = np.flatnonzero(size == 3)
    assert 0 < len(three) < 256
    assert (three < gc.CHUNK).sum() >= 8 and (three >= K - 100).sum() >= 8
    # the list count the device sees: 16 lists end the merge after one level, 17 need a second
    assert -(-K // gc.CHUNK) == (16 if K == gc.TWO_LEVELS else 17)


def test_lattice_winners_straddle_the_boundaries():
    cl = gc.lattice_clusters(K_BIG)
    size = cl["size"]
    n3 = int((size == 3).sum())
    by = {}
    for name, kind, kw in gc.LATTICE_SETTINGS:
        by[name] = _indices(assign_goals(cl, gc.lattice_robots(kind, K_BIG, 256), **kw))
    for name in ("random", "stacked_last", "stacked_first", "all_ties"):
        assert (by[name] >= 0).all() and len(set(by[name])) == 256
    a = by["random"]
    assert (a < gc.CHUNK).any() and (a >= gc.CHUNK).any() and (a >= gc.TWO_LEVELS).any()
    a = by["stacked_last"]
    assert (a >= gc.TWO_LEVELS).any() and (a < gc.TWO_LEVELS).any()
    a = by["stacked_first"]
    assert (a < gc.CHUNK).any() and (a >= gc.CHUNK).any()
    # no distance term: util = size, so the classes go out largest first, each in index order
    order = np.lexsort((np.arange(K_BIG), -size))
    np.testing.assert_array_equal(by["all_ties"], order[:256])
    assert (by["all_ties"][:n3] >= gc.TWO_LEVELS).any() and (by["all_ties"][:n3] < gc.CHUNK).any()
    a = by["size3_only"]
    assert (a < 0).sum() == 256 - n3
    assert (a[a >= 0] < gc.CHUNK).any() and (a >= gc.TWO_LEVELS).any()
    # the stacked robots reach past the boundary with 3 robots too, and with one record behind it
    a = _indices(assign_goals(cl, gc.lattice_robots("last", K_BIG, 3), min_size=1))
    assert (a >= gc.TWO_LEVELS).any() and (a < gc.TWO_LEVELS).any()
    K1 = gc.TWO_LEVELS + 1
    a = _indices(assign_goals(gc.lattice_clusters(K1), gc.lattice_robots("last", K1, 256), min_size=1))
    assert gc.TWO_LEVELS in a and (a < gc.TWO_LEVELS).sum() == 255


def test_straight_line_policy_in_extended_precision():
    """dm.goals.assign_goals against a replay of the greedy order with every
    utility recomputed in long double.  The margin: the double chain dx,
    dx^2, dy^2, +, sqrt, w*, 1+, / adds positive quantities only and the sqrt
    halves the error before it, so a utility carries at most about 6 relative
    roundings of 2^-53, below 2^-50; two of them compared, 2^-49.  The chosen
    cluster's utility is within that band of the best one left, and of the
    clusters within the band it has the smallest label."""
    ld = np.longdouble
    cl = gc.lattice_clusters(K_BIG)
    robots = gc.lattice_robots("random", K_BIG, 256)
    w = 1.0
    got = assign_goals(cl, robots, min_size=1, distance_weight=w, min_distance=0.0)
    band = ld(1) - ld(2) ** -49
    cx, cy, size = cl["cx_m"].astype(ld), cl["cy_m"].astype(ld), cl["size"].astype(ld)
    label = cl["label"]
    taken = np.zeros(len(cl), bool)
    for (rx, ry), g in zip(robots, got):
        dx, dy = cx - ld(rx), cy - ld(ry)
        util = size / (ld(1) + ld(w) * np.sqrt(dx * dx + dy * dy))
        util[taken] = -1
        assert g is not None
        c = g[0]
        assert not taken[c]
        best = util.max()
        assert util[c] >= band * best
        near = np.flatnonzero(util >= band * best)
        assert label[c] == label[near].min()
        assert g[1] == (float(cl["cx_m"][c]), float(cl["cy_m"][c]))
        taken[c] = True


@pytest.fixture(scope="module")
def room_cache():
    return {}


def _room_call(fn, kind, cache, **kw):
    p = gc.room_params()
    return fn(gc.room_state(), gc.room_clusters(), gc.room_robots(kind), p.origin_x, p.origin_y, p.resolution,
              cache=cache, **kw)


def test_room_shape(room_cache):
    st, cl = gc.room_state(), gc.room_clusters()
    assert st.shape == (gc.ROOM_N, gc.ROOM_N) and gc.ROOM_N % 64 == 16
    assert gc.CHUNK < len(cl) < 2 * gc.CHUNK
    cells = gc.ROOM_SPREAD_CELLS
    assert len(set(cells)) == 8 and all(st[y, x] == 0 for x, y in cells + (gc.ROOM_STACKED_CELL,))
    trav = plan.traversable(st, gc.ROOM_KW["inflate_cells"])
    assert all(trav[y, x] for x, y in cells + (gc.ROOM_STACKED_CELL,))
    # the stacked cell is beside the row where record 4096 lies
    assert abs(int(cl["label"][gc.CHUNK]) // gc.ROOM_N - gc.ROOM_STACKED_CELL[1]) <= 4
    # a whole ring's centroid is its unknown cell: the query has to snap; the rings the wall cuts
    # have theirs on a traversable cell (snap distance 0)
    p = gc.room_params()
    tx = np.floor((cl["cx_m"] - p.origin_x) / p.resolution).astype(int)
    ty = np.floor((cl["cy_m"] - p.origin_y) / p.resolution).astype(int)
    ring = cl["size"] == 8
    assert ring.sum() > gc.CHUNK and (st[ty[ring], tx[ring]] == -1).all() and not trav[ty[ring], tx[ring]].any()
    assert trav[ty, tx].sum() >= 40
    # the sealed box: its clusters are not reached, every ring outside it is
    f = plan.field(st, [gc.ROOM_STACKED_CELL], gc.ROOM_KW["inflate_cells"])
    room_cache[gc.ROOM_STACKED_CELL] = f
    cost = np.array([plan.snap(f, (x, y), gc.ROOM_KW["snap_cells"])[0] for x, y in zip(tx, ty)], np.uint64)
    lo, hi = gc.ROOM_BOX
    inside = (tx > lo) & (tx < hi) & (ty > lo) & (ty < hi)
    assert inside.sum() > 100
    assert (cost[inside] == plan.UNREACHABLE).all() and (cost[ring & ~inside] != plan.UNREACHABLE).all()
    assert (cost[~inside] == plan.UNREACHABLE).sum() <= 2  # a patch wider than the snap distance round its centroid
    # the wall: a path round it is longer than the straight line by more than a metre somewhere
    wx, wy = 60, 104  # below the wall; the stacked cell is far above its level, the detour is from (60, 96)
    g = plan.field(st, [(60, 96)], gc.ROOM_KW["inflate_cells"])
    room_cache[(60, 96)] = g
    assert g[wy, wx] * p.resolution / 5.0 > 1.0 + np.hypot(0, 8) * p.resolution


def test_room_gains_and_the_gain_filter(room_cache):
    cl = gc.room_clusters()
    g = gc.room_gains(room_cache)
    mg = gc.room_min_gain(room_cache)
    reached = g > 0
    assert mg == int(np.median(g[reached])) and mg > 0
    assert len(np.unique(g[g >= mg])) >= 4
    low = reached & (g < mg)
    assert low[:gc.CHUNK].any() and low[gc.CHUNK:].any()
    assert (g >= mg)[:gc.CHUNK].any() and (g >= mg)[gc.CHUNK:].any()
    assert len(cl) == len(g)


def test_room_winners_straddle_the_chunk(room_cache):
    kw = {k: v for k, v in gc.ROOM_KW.items() if k != "radius_cells"}
    for s in gc.ROOM_SETTINGS:
        a = _indices(_room_call(plan.assign_goals_path, "spread", room_cache, **kw, **s))
        assert (a >= 0).all() and a.min() < gc.CHUNK <= a.max()
        a = _indices(_room_call(plan.assign_goals_path, "stacked", room_cache, **kw, **s))
        assert (a >= 0).all() and len(set(a)) == 8 and a.min() < gc.CHUNK <= a.max()
    # each spread robot alone: its own best cluster, some in each chunk
    p = gc.room_params()
    alone = [plan.assign_goals_path(gc.room_state(), gc.room_clusters(), gc.room_robots("spread")[r:r + 1],
                                    p.origin_x, p.origin_y, p.resolution, cache=room_cache, **kw, min_size=1)[0][0]
             for r in range(8)]
    assert min(alone) < gc.CHUNK <= max(alone)
    mg = gc.room_min_gain(room_cache)
    for s in gc.ROOM_SETTINGS + (dict(min_size=1, min_gain=mg),):
        a = _indices(_room_call(gain.assign_goals_gain, "stacked", room_cache, **gc.ROOM_KW, **s))
        assert (a >= 0).all() and len(set(a)) == 8 and a.min() < gc.CHUNK <= a.max()
    # the gain filter decides: in each chunk a spread robot's goal without it has a gain below it
    free = _room_call(gain.assign_goals_gain, "spread", room_cache, **gc.ROOM_KW, min_size=1)
    kept = _room_call(gain.assign_goals_gain, "spread", room_cache, **gc.ROOM_KW, min_size=1, min_gain=mg)
    low = [f[0] for f, k in zip(free, kept) if f[3] < mg and k[0] != f[0]]
    assert min(low) < gc.CHUNK <= max(low)
    assert all(k[3] >= mg for k in kept)

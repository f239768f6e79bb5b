"""GPU: goal selection past one 4096-record sort chunk and through two merge
levels (csrc/dm_goals.hip: k_goal_topk, k_goal_merge, dm_launch_goal_topk)
against the host restatements, bit for bit, on the cases of goal_cases.py
(tests/test_goal_cases_host.py checks on the CPU that those cases reach what
they claim).

Straight-line form: more than 16 * 4096 clusters, so 256 robots (16 chunk
lists per merge workgroup) need a merge of merged lists; the calls run on one
handle in an order that grows the list workspace and then asks for less.
Field-scored forms (path, gain, coord): a 272 x 272 room with a little more
than 4096 clusters, so the chunk offset into the cost and gain rows, the merge,
the skip flags and the memo run past chunk 0."""
import numpy as np
import pytest

import dm
import goal_cases as gc
from dm import gain, plan
from dm.goals import assign_goals

pytestmark = pytest.mark.gpu

K_BIG = gc.TWO_LEVELS + 100
# (K, R) in the order they run on the one handle; lists -> merge levels
LATTICE_CALLS = (
    (K_BIG, 1),                 # 4096 lists per workgroup: one group
    (K_BIG, 256),               # 17 lists -> 2 -> 1; the second group is one ragged list of 100 < T records
    (K_BIG, 255),               # 16 * 255 = 4080: padding inside a full group
    (K_BIG, 200),               # 20 lists per workgroup: one level
    (K_BIG, 3),                 # after the large calls: the workspace is larger than needed
    (gc.TWO_LEVELS + 1, 256),   # a list with one real record through level 2
    (gc.TWO_LEVELS, 256),       # exactly one full group: one level
)


@pytest.fixture(scope="module")
def lattice():
    box = {"m": dm.OccupancyMapper(gc.lattice_params()), "K": None, "clusters": None}
    yield box
    box["m"].close()


def _lattice_at(box, K):
    if box["K"] != K:
        m = box["m"]
        m.set_state(gc.lattice_state(K)[0])
        cl = m.frontiers().clusters.copy()
        assert len(cl) == K
        np.testing.assert_array_equal(cl["size"], gc.lattice_sizes(K))
        np.testing.assert_array_equal(cl["label"], gc.lattice_clusters(K)["label"])
        box["K"], box["clusters"] = K, cl
    return box["m"], box["clusters"]


def _check(m, clusters, robots, **kw):
    got = m.assign_goals(robots, **kw)
    exp = assign_goals(clusters, robots, **kw)
    assert len(got) == len(exp) == len(robots)
    for g, e in zip(got, exp):
        if e is None:
            assert g is None
        else:
            assert g is not None and g[0] == e[0]
            assert g[1] == e[1]  # same record: the same doubles
    return got


@pytest.mark.parametrize("K,R", LATTICE_CALLS)
def test_straight_line_goals_through_two_merge_levels(lattice, K, R):
    m, cl = _lattice_at(lattice, K)
    size = cl["size"]
    n3 = int((size == 3).sum())
    assert 0 < n3 < 256
    for name, kind, kw in gc.LATTICE_SETTINGS:
        got = _check(m, cl, gc.lattice_robots(kind, K, R), **kw)
        idx = np.array([g[0] if g is not None else -1 for g in got], np.int64)
        if name == "stacked_last" and K > gc.TWO_LEVELS and R >= 3:
            # identical robots: robot r gets the r-th best; the winners lie on both sides of list 16
            assert (idx >= gc.TWO_LEVELS).any() and ((idx >= 0) & (idx < gc.TWO_LEVELS)).any()
        if name == "stacked_first" and R >= 200:
            assert (idx >= gc.CHUNK).any() and ((idx >= 0) & (idx < gc.CHUNK)).any()
        if name == "all_ties":
            # util = size: the classes largest first, each in index order, whichever group holds the record
            np.testing.assert_array_equal(idx, np.lexsort((np.arange(K), -size))[:R])
        if name == "size3_only":
            assert (idx < 0).sum() == max(R - n3, 0)
            assert (size[idx[idx >= 0]] == 3).all()
            if R > n3:
                assert (idx[idx >= 0] < gc.CHUNK).any() and (idx >= K - 100).any()


# ---- the field-scored forms on the room ----------------------------------------

_CACHE: dict = {}  # the restatements' per-robot fields, gains and views, shared by the tests below


@pytest.fixture(scope="module")
def room():
    st = gc.room_state()
    m = dm.OccupancyMapper(gc.room_params())
    m.set_state(st)
    cl = m.frontiers().clusters.copy()
    exp = gc.room_clusters()
    assert gc.CHUNK < len(cl) < 2 * gc.CHUNK and len(cl) == len(exp)
    np.testing.assert_array_equal(cl["label"], exp["label"])
    np.testing.assert_array_equal(cl["size"], exp["size"])
    yield m, st, cl
    m.close()


def _same(got, exp, n):
    assert len(got) == len(exp) == n
    for g, e in zip(got, exp):
        if e is None:
            assert g is None
        else:
            assert g is not None and g[0] == e[0] and g[2:] == e[2:]  # index, snapped cell, gain
            assert g[1] == e[1]  # the same doubles
    return np.array([g[0] if g is not None else -1 for g in got], np.int64)


def _straddles(idx):
    return (idx >= 0).all() and len(set(idx)) == len(idx) and idx.min() < gc.CHUNK <= idx.max()


@pytest.mark.parametrize("kind", ("spread", "stacked"))
def test_goals_by_path_past_one_chunk(room, kind):
    m, st, cl = room
    p = m.params
    robots = gc.room_robots(kind)
    kw = {k: v for k, v in gc.ROOM_KW.items() if k != "radius_cells"}
    for s in gc.ROOM_SETTINGS:
        got = m.assign_goals_path(robots, **kw, **s)
        exp = plan.assign_goals_path(st, cl, robots, p.origin_x, p.origin_y, p.resolution, cache=_CACHE, **kw, **s)
        idx = _same(got, exp, 8)
        assert (idx >= 0).all() and idx.min() < gc.CHUNK <= idx.max()
        if kind == "stacked":
            assert _straddles(idx)  # robot r's goal is the r-th best
    # the field left behind is the last robot's
    last = plan.cell_of(robots[7][0], robots[7][1], p.origin_x, p.origin_y, p.resolution, gc.ROOM_N, gc.ROOM_N)
    np.testing.assert_array_equal(m.plan_cost_field(), _CACHE[last])


@pytest.mark.parametrize("kind", ("spread", "stacked"))
def test_goals_by_gain_past_one_chunk(room, kind):
    m, st, cl = room
    p = m.params
    robots = gc.room_robots(kind)
    for s in gc.ROOM_SETTINGS + (dict(min_size=1, min_gain=gc.room_min_gain(_CACHE)),):
        got = m.assign_goals_gain(robots, **gc.ROOM_KW, **s)
        exp = gain.assign_goals_gain(st, cl, robots, p.origin_x, p.origin_y, p.resolution, cache=_CACHE,
                                     **gc.ROOM_KW, **s)
        idx = _same(got, exp, 8)
        if kind == "stacked":
            assert _straddles(idx)


@pytest.mark.parametrize("kind", ("spread", "stacked"))
def test_goals_by_marginal_gain_past_one_chunk(room, kind):
    m, st, cl = room
    p = m.params
    robots = gc.room_robots(kind)
    held = gc.room_held()
    for s in gc.ROOM_SETTINGS:
        got = m.assign_goals_coord(robots, held_xy=held, **gc.ROOM_KW, **s)
        claimed = m.gain_claimed()
        exp, exp_claimed = gain.assign_goals_coord(st, cl, robots, p.origin_x, p.origin_y, p.resolution,
                                                   held_xy=held, cache=_CACHE, return_claimed=True,
                                                   **gc.ROOM_KW, **s)
        idx = _same(got, exp, 8)
        assert (idx >= 0).all() and len(set(idx)) == 8
        np.testing.assert_array_equal(claimed, exp_claimed)

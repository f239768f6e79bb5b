"""CPU: the host restatement of the information-gain calls (dm/gain.py, the
reference of the GPU tests in test_gpu_gain.py) against closed forms, a scalar
per-ray loop written straight from the definition, and the policy case the
feature is for: a long frontier along a sliver of unknown against a short one
that opens onto unmapped space."""
import numpy as np
import pytest

import cases
import dm
import np_oracle
from dm import gain, plan

# lattice points with dx^2 + dy^2 <= R^2
DISC = {1: 5, 2: 13, 3: 29, 7: 149, 15: 709, 16: 797, 31: 3001, 32: 3209, 40: 5025}


def scalar_visible_unknown(st, cell, R):
    """One ray at a time, one step at a time, from the formula of include/dm.h."""
    H, W = st.shape
    vx, vy = cell
    marked = set()
    for ex in range(-R, R + 1):
        for ey in range(-R, R + 1):
            if max(abs(ex), abs(ey)) != R:
                continue
            xmajor = abs(ex) >= abs(ey)
            n, adb = R, min(abs(ex), abs(ey))
            ia = (1 if ex > 0 else -1) if xmajor else (1 if ey > 0 else -1)
            minor_off = ey if xmajor else ex
            ib = (minor_off > 0) - (minor_off < 0)
            for k in range(R + 1):
                major, minor = k * ia, ib * ((2 * k * adb + n) // (2 * n))
                dx, dy = (major, minor) if xmajor else (minor, major)
                x, y = vx + dx, vy + dy
                if not (0 <= x < W and 0 <= y < H) or dx * dx + dy * dy > R * R or st[y, x] == 100:
                    break
                if st[y, x] != 0:
                    marked.add((x, y))
    return len(marked)


def clusters_of(p, st):
    rec = np_oracle.frontiers(p, st)[2]
    return np.array(rec, dtype=np.dtype(dm.CLUSTER_DTYPE))


def policy_map():
    st = np.full((128, 128), -1, np.int8)
    st[9:101, 9:61] = 100
    st[10:100, 10:60] = 0
    st[20:80, 60] = -1      # the sliver
    st[19:81, 61] = 100     # backed by a wall
    st[84:88, 9] = 0        # the four-cell doorway
    return st


def centre(p, cx, cy):
    return (p.origin_x + (cx + 0.5) * p.resolution, p.origin_y + (cy + 0.5) * p.resolution)


@pytest.mark.parametrize("R", sorted(DISC))
def test_disc_invariant(R):
    n = 2 * R + 5
    st = np.full((n, n), -1, np.int8)
    assert gain.visible_unknown(st, (n // 2, n // 2), R) == DISC[R]
    exact = sum(1 for dx in range(-R, R + 1) for dy in range(-R, R + 1) if dx * dx + dy * dy <= R * R)
    assert exact == DISC[R]


@pytest.mark.parametrize("seed,R", [(1, 1), (2, 2), (3, 5), (4, 13), (5, 20)])
def test_vectorised_equals_scalar_loop(seed, R):
    st = cases.random_state(seed, 80, 96)
    H, W = st.shape
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    views = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (0, 37), (W - 1, 41), (50, 0), (23, H - 1)]
    views += [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(6)]
    some = 0
    for v in views:
        g = gain.visible_unknown(st, v, R)
        assert g == scalar_visible_unknown(st, v, R), v
        some += g
    assert some > 0


def test_occlusion():
    st = np.zeros((64, 64), np.int8)
    st[40:, :] = -1
    open_gain = gain.visible_unknown(st, (32, 20), 30)
    assert open_gain > 0
    st[39, :] = 100  # a full occupied row between the view and the unknown half
    assert gain.visible_unknown(st, (32, 20), 30) == 0
    st[:] = -1
    st[30, 30] = 100
    assert gain.visible_unknown(st, (30, 30), 10) == 0  # a view on an occupied cell
    assert gain.visible_unknown(st, (31, 30), 10) > 0


def test_gain_views_cells_and_outside():
    p = cases.make_params(96, 80)
    st = cases.random_state(9, 80, 96)
    views = [centre(p, 5, 7), centre(p, 95, 79), (1e9, 0.0), (float("nan"), 0.0), (0.0, float("inf")), centre(p, 5, 7)]
    g, c = gain.gain_views(st, views, p.origin_x, p.origin_y, p.resolution, 12)
    assert list(c) == [7 * 96 + 5, 79 * 96 + 95, -1, -1, -1, 7 * 96 + 5]
    assert list(g[2:5]) == [0, 0, 0] and g[0] == g[5] == gain.visible_unknown(st, (5, 7), 12)
    for bad in (0, 512):
        with pytest.raises(ValueError):
            gain.gain_views(st, views, p.origin_x, p.origin_y, p.resolution, bad)
    assert gain.default_radius(12.0, 0.05) == 240 and gain.default_radius(100.0, 0.05) == 511


def test_policy_case_sliver_against_doorway():
    st = policy_map()
    assert gain.visible_unknown(st, (59, 50), 40) == 60
    assert gain.visible_unknown(st, (10, 86), 40) == 189
    p = cases.make_params(128, 128, min_frontier_size=1)
    cl = clusters_of(p, st)
    cx = np.floor((cl["cx_m"] - p.origin_x) / p.resolution)
    sliver, door = int(np.flatnonzero(cx == 59)[0]), int(np.flatnonzero(cx == 9)[0])
    assert cl["size"][sliver] >= 60 and cl["size"][door] == 4
    robot = [centre(p, 35, 50)]
    kw = dict(min_size=1, inflate_cells=1, snap_cells=3)
    by_path = plan.assign_goals_path(st, cl, robot, p.origin_x, p.origin_y, p.resolution, **kw)[0]
    by_gain = gain.assign_goals_gain(st, cl, robot, p.origin_x, p.origin_y, p.resolution, radius_cells=40, **kw)[0]
    assert by_path[0] == sliver and by_gain[0] == door
    # each confirmed by the restatement: the gain reported is the chosen cell's
    assert by_gain[3] == gain.visible_unknown(st, (by_gain[2] % 128, by_gain[2] // 128), 40) > 60
    assert by_gain[1] == centre(p, by_gain[2] % 128, by_gain[2] // 128)


def walled_map(gap: bool):
    """The walled room of test_gpu_goals_path.py: free x, y in [10, 60) x
    [10, 100), an occupied ring, a free pocket behind the right wall; with
    `gap`, an opening in the left wall."""
    st = np.full((128, 128), -1, np.int8)
    st[9:101, 9:61] = 100
    st[10:100, 10:60] = 0
    st[45:55, 61:66] = 0
    if gap:
        st[80:90, 9] = 0
    return st


def test_assign_goals_gain_filters_and_ties():
    p = cases.make_params(128, 128, min_frontier_size=1)
    args = (p.origin_x, p.origin_y, p.resolution)
    kw = dict(min_size=1, inflate_cells=1, snap_cells=3, radius_cells=40)
    robot = centre(p, 55, 50)
    # a sealed-off cluster is no goal
    st = walled_map(gap=False)
    cl = clusters_of(p, st)
    assert len(cl) >= 1
    assert gain.assign_goals_gain(st, cl, [robot], *args, **kw) == [None]
    # the opening is; min_gain filters it
    st = walled_map(gap=True)
    cl = clusters_of(p, st)
    got = gain.assign_goals_gain(st, cl, [robot], *args, **kw)[0]
    assert got is not None and got[3] > 0
    assert gain.assign_goals_gain(st, cl, [robot], *args, min_gain=got[3], **kw)[0] == got
    assert gain.assign_goals_gain(st, cl, [robot], *args, min_gain=got[3] + 1, **kw) == [None]
    # two robots do not take the same cluster
    st = policy_map()
    cl = clusters_of(p, st)
    two = gain.assign_goals_gain(st, cl, [centre(p, 35, 50), centre(p, 35, 50)], *args, **kw)
    assert two[0] is not None and two[1] is not None and two[0][0] != two[1][0]
    with pytest.raises(ValueError):
        gain.assign_goals_gain(st, cl, [robot], *args, distance_weight=-1.0, **kw)
    with pytest.raises(ValueError):
        gain.assign_goals_gain(st, cl, [robot], *args, min_gain=-1, **kw)
    with pytest.raises(ValueError):
        gain.assign_goals_gain(st, cl, [(1e6, 0.0)], *args, **kw)


def test_zero_gain_is_never_a_goal():
    """gain == 0 gives util 0, which reads as "not eligible" even with
    min_gain = 0; the same cluster is a goal by path length."""
    st = np.zeros((20, 20), np.int8)
    cl = np.zeros(1, dtype=np.dtype(dm.CLUSTER_DTYPE))
    cl["label"], cl["size"], cl["cx_m"], cl["cy_m"] = 5, 10, 12.5, 5.5  # an all-free map: nothing to see
    got = gain.assign_goals_gain(st, cl, [(3.5, 5.5)], 0.0, 0.0, 1.0, min_size=1, min_gain=0, inflate_cells=0,
                                 snap_cells=1, radius_cells=5)
    assert got == [None]
    assert plan.assign_goals_path(st, cl, [(3.5, 5.5)], 0.0, 0.0, 1.0, min_size=1, inflate_cells=0,
                                  snap_cells=1)[0] is not None


def test_library_exports_the_gain_entry_points():
    lib = dm.load_library()
    for name in ("dm_gain_views", "dm_assign_goals_gain"):
        assert hasattr(lib, name), name

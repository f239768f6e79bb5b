"""Information gain of a viewpoint on the occupancy grid: host restatement and
test reference of dm_gain_views and dm_assign_goals_gain (csrc/dm_gain.h), as
dm/plan.py is for the planner.

The reference explores reactively (server/thymio_project/thymio_project/
main.py:123-188) and has no next-best-view step, so there is no reference
behaviour to match; the definitions are this build's SPEC (include/dm.h,
DESIGN.md §9).  They use integers only, so the results are unique.

Visible-unknown count of a view cell (vx, vy) for radius_cells = R in [1, 511]:

* one ray to each of the 8R offsets (ex, ey) with max(|ex|, |ey|) == R;
* each ray is the SPEC a5 line of csrc/dm_ray.h: the major axis is x iff
  |ex| >= |ey|, n = R, adb = min(|ex|, |ey|), and step k (0..R) is at
  major = k * ia, minor = ib * floor((2 * k * adb + n) / (2 * n));
* a ray is walked from k = 0 and ends before the first cell that is out of
  the grid, has dx*dx + dy*dy > R*R, or has state 100; every cell it visits
  before that whose state is unknown (neither 0 nor 100) is marked;
* the gain is the number of distinct marked cells.

The overlap-aware calls (dm_gain_views_joint, dm_assign_goals_coord; DESIGN.md
§9.4) are restated here too.  The visible set V(cell, R) is the set of marked
cells above; a claimed set C is a set of map cells; the marginal gain of a view
is |V - C| (the cells of V not in C) and its commit is C := C | V.
"""
from __future__ import annotations

import math

import numpy as np

from . import plan

MAX_RADIUS = 511
MAX_VIEWS = 1 << 20
MAX_JOINT_VIEWS = 1024


def check_radius(R: int) -> int:
    R = int(R)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"radius_cells must be in [1, {MAX_RADIUS}]")
    return R


def ray_offsets(R: int):
    """(ex, ey) int64 [8R]: the offsets with max(|ex|, |ey|) == R."""
    a = np.arange(-R, R + 1, dtype=np.int64)
    b = np.arange(-R + 1, R, dtype=np.int64)
    ex = np.concatenate([a, a, np.full(b.shape, -R), np.full(b.shape, R)])
    ey = np.concatenate([np.full(a.shape, -R), np.full(a.shape, R), b, b])
    return ex, ey


def visible_window(state, cell, R: int):
    """The visible set of the view cell (vx, vy), cut to the grid: (y0, x0,
    bool [y1 - y0, x1 - x0]) with the window [vy - R, vy + R] x [vx - R, vx + R]
    clipped to the map.  Vectorised over the 8R rays, a loop over k with an
    alive mask."""
    st = np.asarray(state)
    H, W = st.shape
    R = check_radius(R)
    vx, vy = int(cell[0]), int(cell[1])
    x0, y0 = max(vx - R, 0), max(vy - R, 0)
    x1, y1 = min(vx + R + 1, W), min(vy + R + 1, H)
    marked = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0)), bool)
    ex, ey = ray_offsets(R)
    xmajor = np.abs(ex) >= np.abs(ey)
    adb = np.minimum(np.abs(ex), np.abs(ey))
    sx, sy = np.sign(ex), np.sign(ey)
    alive = np.ones(ex.shape, bool)
    for k in range(R + 1):
        q = (2 * k * adb + R) // (2 * R)
        dx = np.where(xmajor, k * sx, q * sx)
        dy = np.where(xmajor, q * sy, k * sy)
        x, y = vx + dx, vy + dy
        alive &= (x >= 0) & (x < W) & (y >= 0) & (y < H) & (dx * dx + dy * dy <= R * R)
        if not alive.any():
            break
        xa, ya = x[alive], y[alive]
        s = st[ya, xa]
        blocked = s == 100
        unknown = (s != 100) & (s != 0)
        marked[ya[unknown] - y0, xa[unknown] - x0] = True
        alive[np.flatnonzero(alive)[blocked]] = False
    return y0, x0, marked


def visible_set(state, cell, R: int) -> np.ndarray:
    """V(cell, R): bool [H, W], the marked cells of the view cell (vx, vy)."""
    st = np.asarray(state)
    y0, x0, sub = visible_window(st, cell, R)
    out = np.zeros(st.shape, bool)
    out[y0:y0 + sub.shape[0], x0:x0 + sub.shape[1]] = sub
    return out


def visible_unknown(state, cell, R: int) -> int:
    """The visible-unknown count of the view cell (vx, vy): |V(cell, R)|."""
    return int(visible_window(state, cell, R)[2].sum())


def _marginal(claimed: np.ndarray, win) -> int:
    y0, x0, sub = win
    return int((sub & ~claimed[y0:y0 + sub.shape[0], x0:x0 + sub.shape[1]]).sum())


def _commit(claimed: np.ndarray, win) -> None:
    y0, x0, sub = win
    claimed[y0:y0 + sub.shape[0], x0:x0 + sub.shape[1]] |= sub


def gain_views(state, views_xy, origin_x: float, origin_y: float, resolution: float, radius_cells: int):
    """dm_gain_views: (gain uint32 [n], cell int64 [n]); a view outside the
    grid, or a non-finite one, has cell -1 and gain 0."""
    st = np.asarray(state)
    H, W = st.shape
    R = check_radius(radius_cells)
    xy = np.asarray(views_xy, np.float64).reshape(-1, 2)
    if xy.shape[0] > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views")
    gain = np.zeros(xy.shape[0], np.uint32)
    cells = np.full(xy.shape[0], -1, np.int64)
    memo: dict = {}
    for i, (x, y) in enumerate(xy):
        c = plan.cell_of(float(x), float(y), origin_x, origin_y, resolution, W, H)
        if c is None:
            continue
        cells[i] = c[1] * W + c[0]
        if c not in memo:
            memo[c] = visible_unknown(st, c, R)
        gain[i] = memo[c]
    return gain, cells


def gain_views_joint(state, views_xy, origin_x: float, origin_y: float, resolution: float, radius_cells: int):
    """dm_gain_views_joint: (marginal uint32 [n], cell int64 [n], claimed bool
    [H, W]).  The claimed set starts empty; view i's marginal gain is what it
    sees that the views before it do not, then its visible set is committed.
    A view outside the grid, or a non-finite one, has cell -1 and marginal 0
    and commits nothing."""
    st = np.asarray(state)
    H, W = st.shape
    R = check_radius(radius_cells)
    xy = np.asarray(views_xy, np.float64).reshape(-1, 2)
    if xy.shape[0] > MAX_JOINT_VIEWS:
        raise ValueError(f"at most {MAX_JOINT_VIEWS} views")
    marginal = np.zeros(xy.shape[0], np.uint32)
    cells = np.full(xy.shape[0], -1, np.int64)
    claimed = np.zeros((H, W), bool)
    wins: dict = {}
    for i, (x, y) in enumerate(xy):
        c = plan.cell_of(float(x), float(y), origin_x, origin_y, resolution, W, H)
        if c is None:
            continue
        cells[i] = c[1] * W + c[0]
        if c not in wins:
            wins[c] = visible_window(st, c, R)
        marginal[i] = _marginal(claimed, wins[c])
        _commit(claimed, wins[c])
    return marginal, cells, claimed


def default_radius(range_max: float, resolution: float) -> int:
    """ceil(range_max / resolution), capped at the limit."""
    return max(1, min(MAX_RADIUS, int(math.ceil(float(range_max) / float(resolution)))))


def assign_goals_gain(state, clusters: np.ndarray, robots_xy, origin_x: float, origin_y: float, resolution: float,
                      min_size: int = 8, min_gain: int = 0, distance_weight: float = 1.0, min_distance: float = 0.0,
                      inflate_cells: int = 2, max_cost: int = 0, snap_cells: int = 5, radius_cells: int = 240,
                      cache: dict | None = None):
    """dm.plan.assign_goals_path with the visible-unknown count of the snapped
    cell as the numerator of the utility: per robot, in order, (cluster index,
    (x, y) centre of the snapped cell, snapped cell, gain) or None.  A cluster
    is eligible iff size >= min_size, it is reached, dist >= min_distance and
    gain >= min_gain; util = gain / (1 + distance_weight * dist), and a gain of
    0 is never a goal.  `cache`: as for assign_goals_path (the per-robot
    fields, keyed by the robot's cell); the gains of the view cells are kept in
    it too, under ("gain", radius, cell)."""
    if not float(distance_weight) >= 0.0:
        raise ValueError("distance_weight must be >= 0 (dm_assign_goals_gain rejects it too)")
    if int(min_gain) < 0:
        raise ValueError("min_gain must be >= 0")
    R = check_radius(radius_cells)
    st = np.asarray(state)
    H, W = st.shape
    cells = plan._robot_cells(robots_xy, origin_x, origin_y, resolution, W, H)
    if clusters is None or len(clusters) == 0:
        return [None] * len(cells)
    gains: dict = cache if cache is not None else {}

    def numerator(i, cell):
        key = ("gain", R, cell)
        if key not in gains:
            gains[key] = visible_unknown(st, (cell % W, cell // W), R)
        return gains[key]

    return plan._greedy_goals(st, clusters, cells, origin_x, origin_y, resolution, min_size, distance_weight,
                              min_distance, inflate_cells, max_cost, snap_cells, cache, numerator, min_gain)


def assign_goals_coord(state, clusters: np.ndarray, robots_xy, origin_x: float, origin_y: float, resolution: float,
                       min_size: int = 8, min_gain: int = 0, distance_weight: float = 1.0, min_distance: float = 0.0,
                       inflate_cells: int = 2, max_cost: int = 0, snap_cells: int = 5, radius_cells: int = 240,
                       held_xy=(), cache: dict | None = None, return_claimed: bool = False):
    """dm_assign_goals_coord: assign_goals_gain with the marginal gain as the
    numerator.  The claimed set starts as the union of the visible sets of the
    held views (a held view outside the grid or non-finite adds nothing); robot
    r scores cluster c by what the snapped cell of c under r's field sees that
    is not claimed, and the view of the goal r gets is committed before robot
    r + 1 chooses.  Returns assign_goals_gain's tuples with the marginal gain
    in place of the gain; with `return_claimed`, (those, claimed bool [H, W]).
    `cache`: the per-robot fields as for assign_goals_path, and the visible
    sets of the view cells under ("view", radius, cell); gains are not kept,
    they depend on the claimed set."""
    if not float(distance_weight) >= 0.0:
        raise ValueError("distance_weight must be >= 0 (dm_assign_goals_coord rejects it too)")
    if int(min_gain) < 0:
        raise ValueError("min_gain must be >= 0")
    R = check_radius(radius_cells)
    st = np.asarray(state)
    H, W = st.shape
    held = np.asarray(held_xy, np.float64).reshape(-1, 2)
    if held.shape[0] > MAX_JOINT_VIEWS:
        raise ValueError(f"at most {MAX_JOINT_VIEWS} held views")
    cells = plan._robot_cells(robots_xy, origin_x, origin_y, resolution, W, H)
    views: dict = cache if cache is not None else {}

    def window(cell):
        key = ("view", R, cell)
        if key not in views:
            views[key] = visible_window(st, (cell % W, cell // W), R)
        return views[key]

    claimed = np.zeros((H, W), bool)
    for x, y in held:
        c = plan.cell_of(float(x), float(y), origin_x, origin_y, resolution, W, H)
        if c is not None:
            _commit(claimed, window(c[1] * W + c[0]))
    done = lambda out: (out, claimed) if return_claimed else out
    if clusters is None or len(clusters) == 0:
        return done([None] * len(cells))
    return done(plan._greedy_goals(st, clusters, cells, origin_x, origin_y, resolution, min_size, distance_weight,
                                   min_distance, inflate_cells, max_cost, snap_cells, cache,
                                   lambda i, cell: _marginal(claimed, window(cell)), min_gain,
                                   on_pick=lambda cell: _commit(claimed, window(cell))))

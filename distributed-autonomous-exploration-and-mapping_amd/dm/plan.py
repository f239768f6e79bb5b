"""Path planning on the occupancy grid: host restatement and test reference
of dm_plan_* and dm_assign_goals_path (csrc/dm_plan.h), as dm/goals.py is for
dm_assign_goals.

The reference explores reactively (server/thymio_project/thymio_project/
main.py:123-188) and names map-based navigation (Nav2) as future work
(report.pdf p.5 §VI-2), so there is no reference behaviour to match; the
definitions are this build's SPEC (include/dm.h).  They use
integers only, so the results are unique:

* a cell is traversable iff its state is 0 and no in-grid occupied cell (100)
  lies within ``dx*dx + dy*dy <= r*r``; source cells are traversable whatever
  their state;
* moves are 8-connected, cost 5 orthogonal and 7 diagonal; a diagonal move
  needs both cells it passes between traversable (no corner cutting);
* ``cost`` is the least total move cost from any source, ``UNREACHABLE`` where
  there is no path of cost <= max_cost.

The device computes the field by tile-wise min-relaxation; here it is
Dijkstra (scipy) over the legal-move graph.  The fixpoint of min-relaxation is
unique, so both give the same bits.

Clearance-aware planning (dm_plan_clearance, dm_plan_field_cost):

* ``d2[c]`` is the least ``dx*dx + dy*dy <= R*R`` to an in-grid occupied cell,
  ``R*R + 1`` ("far") if there is none;
* entering cell c by a legal move costs ``b * (1 + pen[d2[c]])``, b = 5 / 7,
  for a caller-supplied uint8 table ``pen[R*R + 2]``;
* the weighted field and its paths are defined as above with that move cost.

Team planning (dm_plan_team, dm_assign_goals_team):

* ``team_fields`` is ``field`` per robot, a robot's own cell being a source in
  its own field only;
* ``assign_goals_team`` scores like ``assign_goals_path`` (or, with a view
  radius, ``dm.gain.assign_goals_gain``) and assigns the best (robot, cluster)
  pair first, ties to the smaller label, then the smaller robot
  (``global_greedy``).
"""
from __future__ import annotations

import math

import numpy as np

UNREACHABLE = 0xFFFFFFFF
MAX_COST = 0xFFFFFFEF  # what max_cost == 0 means: a stored cost plus a move never wraps
COST_MAX_WEIGHTED = 0xFFFFF7FF  # the same for a weighted field (DM_PLAN_COST_MAX): a move costs up to 1792
ORTHOGONAL, DIAGONAL = 5, 7
# predecessor order of a path, (dy, dx)
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def _shifted(a: np.ndarray, dy: int, dx: int) -> np.ndarray:
    """out[y, x] = a[y + dy, x + dx], False outside the grid."""
    H, W = a.shape
    out = np.zeros_like(a)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def traversable(state, r: int) -> np.ndarray:
    """bool [H, W]: free and no occupied cell within the disc of radius r."""
    st = np.asarray(state)
    r = int(r)
    if not 0 <= r <= 32:
        raise ValueError("inflate_cells must be in [0, 32]")
    occ = st == 100
    blocked = np.zeros(st.shape, bool)
    if occ.any():
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx * dx + dy * dy <= r * r:
                    blocked |= _shifted(occ, dy, dx)
    return (st == 0) & ~blocked


def _check_clear(R: int) -> int:
    R = int(R)
    if not 1 <= R <= 32:
        raise ValueError("clear_cells must be in [1, 32]")
    return R


def clearance(state, R: int) -> np.ndarray:
    """uint16 [H, W]: the capped squared distance d2 to the nearest occupied
    cell, R*R + 1 where none lies within R.  The Euclidean distance transform
    returns the nearest obstacle's indices, so d2 is exact integer arithmetic."""
    from scipy.ndimage import distance_transform_edt

    st = np.asarray(state)
    R = _check_clear(R)
    far = R * R + 1
    occ = st == 100
    if not occ.any():
        return np.full(st.shape, far, np.uint16)
    idx = distance_transform_edt(~occ, return_distances=False, return_indices=True)
    yy, xx = np.indices(st.shape)
    d2 = (idx[0] - yy).astype(np.int64) ** 2 + (idx[1] - xx).astype(np.int64) ** 2
    return np.where(d2 <= R * R, d2, far).astype(np.uint16)


def penalty(state, R: int, pen) -> np.ndarray:
    """uint8 [H, W]: pen[d2] per cell, for a table uint8 [R*R + 2]."""
    R = _check_clear(R)
    tab = np.asarray(pen)
    if tab.shape != (R * R + 2,):
        raise ValueError(f"pen must have R*R + 2 = {R * R + 2} entries")
    if tab.dtype != np.uint8 and (tab.min() < 0 or tab.max() > 255):
        raise ValueError("pen entries must be in [0, 255]")
    return tab.astype(np.uint8)[clearance(state, R)]


def inflation_table(resolution: float, clear_cells: int, inscribed_m: float, cost_scaling: float) -> np.ndarray:
    """Nav2's inflation curve as a penalty table uint8 [R*R + 2]: 252 within
    the inscribed radius (d = sqrt(d2) * resolution <= inscribed_m), else
    floor(252 * exp(-cost_scaling * (d - inscribed_m))); far = 0."""
    R = _check_clear(clear_cells)
    out = np.zeros(R * R + 2, np.uint8)
    for d2 in range(R * R + 1):
        d = math.sqrt(d2) * float(resolution)
        if d <= inscribed_m:
            out[d2] = 252
        else:
            out[d2] = int(math.floor(252.0 * math.exp(-float(cost_scaling) * (d - inscribed_m))))
    return out


def cell_of(x: float, y: float, origin_x: float, origin_y: float, resolution: float, width: int, height: int):
    """(cx, cy) of a point in metres (floor((x - origin) / resolution), as
    the integration's endpoints), or None outside the grid."""
    fx = math.floor((float(x) - origin_x) / resolution) if math.isfinite(x) else -1
    fy = math.floor((float(y) - origin_y) / resolution) if math.isfinite(y) else -1
    if not (0 <= fx < width and 0 <= fy < height):
        return None
    return int(fx), int(fy)


def with_sources(trav: np.ndarray, sources_cells) -> np.ndarray:
    t = np.array(trav, bool)
    H, W = t.shape
    for cx, cy in sources_cells:
        if not (0 <= cx < W and 0 <= cy < H):
            raise ValueError(f"source cell ({cx}, {cy}) is outside the grid")
        t[cy, cx] = True
    return t


def legal_moves(trav: np.ndarray):
    """For each (dy, dx) of NEIGHBOURS: bool [H, W], the move c -> c + (dy, dx)
    is legal (c itself traversable included)."""
    out = []
    for dy, dx in NEIGHBOURS:
        ok = trav & _shifted(trav, dy, dx)
        if dy != 0 and dx != 0:
            ok &= _shifted(trav, dy, 0) & _shifted(trav, 0, dx)
        out.append(ok)
    return out


def field(state, sources_cells, r: int, max_cost: int = 0, trav: np.ndarray | None = None,
          cell_pen: np.ndarray | None = None) -> np.ndarray:
    """uint32 [H, W] distance field from the source cells [(cx, cy), ...].
    `trav`: a traversable mask to use instead of traversable(state, r).
    `cell_pen`: uint8 [H, W]; entering cell c costs b * (1 + cell_pen[c]) and
    the cap of max_cost is the weighted field's (field_cost)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    sources = [(int(cx), int(cy)) for cx, cy in sources_cells]
    if not sources:
        raise ValueError("need at least one source")
    t = with_sources(traversable(state, r) if trav is None else trav, sources)
    H, W = t.shape
    cap = MAX_COST if cell_pen is None else COST_MAX_WEIGHTED
    max_cost = cap if int(max_cost) == 0 or int(max_cost) > cap else int(max_cost)
    mult = None if cell_pen is None else 1.0 + np.asarray(cell_pen, np.float64).reshape(-1)
    src, dst, wgt = [], [], []
    for (dy, dx), ok in zip(NEIGHBOURS, legal_moves(t)):
        c = np.flatnonzero(ok)
        src.append(c)
        dst.append(c + dy * W + dx)
        b = float(DIAGONAL if dy and dx else ORTHOGONAL)
        wgt.append(np.full(c.shape, b) if mult is None else b * mult[c + dy * W + dx])
    g = csr_matrix((np.concatenate(wgt), (np.concatenate(src), np.concatenate(dst))), shape=(H * W, H * W))
    idx = sorted({cy * W + cx for cx, cy in sources})
    d = dijkstra(g, directed=True, indices=idx, min_only=True, limit=float(max_cost))
    out = np.full(H * W, UNREACHABLE, np.uint32)
    ok = np.isfinite(d) & (d <= max_cost)
    out[ok] = d[ok].astype(np.uint32)  # integer costs are exact in float64
    return out.reshape(H, W)


def field_cost(state, sources_cells, r: int, R: int, pen, max_cost: int = 0) -> np.ndarray:
    """uint32 [H, W]: the penalty-weighted field (dm_plan_field_cost): Dijkstra
    with the move into cell c costing b * (1 + pen[d2[c]])."""
    return field(state, sources_cells, r, max_cost, cell_pen=penalty(state, R, pen))


def snap(cost: np.ndarray, cell, s: int):
    """(cost, linear cell) of the reached cell within Chebyshev distance s of
    `cell` = (cx, cy) that minimises (dx*dx + dy*dy, linear index);
    (UNREACHABLE, -1) if none or cell is None."""
    if cell is None:
        return UNREACHABLE, -1
    H, W = cost.shape
    cx, cy = cell
    best = None
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            x, y = cx + dx, cy + dy
            if not (0 <= x < W and 0 <= y < H) or cost[y, x] == UNREACHABLE:
                continue
            key = (dx * dx + dy * dy, y * W + x)
            if best is None or key < best:
                best = key
    if best is None:
        return UNREACHABLE, -1
    return int(cost.reshape(-1)[best[1]]), int(best[1])


def path(cost: np.ndarray, trav: np.ndarray, cell: int, cell_pen: np.ndarray | None = None) -> list[int]:
    """Linear indices from a source to `cell` (a reached cell; -1: empty
    path).  `trav` includes the sources (with_sources).  The predecessor of c
    is the first neighbour in NEIGHBOURS order that is reached, moves legally
    to c and has cost + w == cost[c]; with `cell_pen` (uint8 [H, W], the
    field being field_cost's) w is b * (1 + cell_pen[c])."""
    if cell < 0:
        return []
    H, W = cost.shape
    out = [int(cell)]
    x, y = cell % W, cell // W
    if cost[y, x] == UNREACHABLE:
        return []
    while cost[y, x] != 0:
        for dy, dx in NEIGHBOURS:
            nx, ny = x + dx, y + dy
            if not (0 <= nx < W and 0 <= ny < H) or cost[ny, nx] == UNREACHABLE:
                continue
            w = DIAGONAL if dy and dx else ORTHOGONAL
            if cell_pen is not None:
                w *= 1 + int(cell_pen[y, x])
            if int(cost[ny, nx]) + w != int(cost[y, x]):
                continue
            if dy and dx and not (trav[ny, x] and trav[y, nx]):
                continue
            x, y = nx, ny
            break
        else:
            raise AssertionError("the field is not a fixpoint: no predecessor")
        out.append(y * W + x)
    return out[::-1]


def _greedy_goals(st, clusters: np.ndarray, robot_cells, origin_x: float, origin_y: float, resolution: float,
                  min_size: int, distance_weight: float, min_distance: float, inflate_cells: int, max_cost: int,
                  snap_cells: int, cache: dict | None, numerator, min_numerator: int = 0, on_pick=None):
    """The one greedy loop of assign_goals_path, dm.gain.assign_goals_gain and
    dm.gain.assign_goals_coord (device: assign_goals_field, csrc/dm_goals.hip).
    Robots choose in order.  Each gets its own field (kept in `cache` under
    its cell (cx, cy) when a dict is given) and the snapped cell of every
    cluster centroid under it; cluster i scores
        util = numerator(i, cell) / (1 + distance_weight * dist),
        dist = cost * resolution / 5,
    where `numerator` is asked for every cluster that snapped somewhere and
    returns an integer.  A cluster is eligible iff size >= min_size, it is
    reached, dist >= min_distance, numerator >= min_numerator, numerator > 0
    (util 0 is the device's key of "not eligible") and no earlier robot took
    it.  The best util wins, ties go to the smaller label; `on_pick(cell)`
    runs before the next robot is scored.  Returns, per robot, (cluster index,
    (x, y) centre of the snapped cell, snapped cell, numerator) or None."""
    H, W = st.shape
    trav = traversable(st, inflate_cells)
    targets = [cell_of(float(c["cx_m"]), float(c["cy_m"]), origin_x, origin_y, resolution, W, H) for c in clusters]
    taken = np.zeros(len(clusters), bool)
    out = []
    for rc in robot_cells:
        f = cache.get(rc) if cache is not None else None
        if f is None:
            f = field(st, [rc], inflate_cells, max_cost, trav=trav)
            if cache is not None:
                cache[rc] = f
        snapped = [snap(f, t, snap_cells) for t in targets]
        cost = np.array([s[0] for s in snapped], np.uint32)
        dist = cost.astype(np.float64) * float(resolution) / 5.0
        num = np.zeros(len(clusters), np.int64)
        for i, (_, cell) in enumerate(snapped):
            if cell >= 0:
                num[i] = numerator(i, cell)
        ok = ((clusters["size"] >= min_size) & (cost != UNREACHABLE) & (dist >= min_distance)
              & (num >= int(min_numerator)) & (num > 0) & ~taken)
        util = np.where(ok, num.astype(np.float64) / (1.0 + float(distance_weight) * dist), -np.inf)
        m = util.max()
        if not np.isfinite(m):
            out.append(None)
            continue
        best = np.flatnonzero(util == m)
        i = int(best[np.argmin(clusters["label"][best])])  # ties: the smaller label
        taken[i] = True
        cell = snapped[i][1]
        if on_pick is not None:
            on_pick(cell)
        xy = (origin_x + ((cell % W) + 0.5) * resolution, origin_y + ((cell // W) + 0.5) * resolution)
        out.append((i, xy, cell, int(num[i])))
    return out


def _robot_cells(robots_xy, origin_x: float, origin_y: float, resolution: float, width: int, height: int):
    cells = [cell_of(float(x), float(y), origin_x, origin_y, resolution, width, height) for x, y in robots_xy]
    if any(c is None for c in cells):
        raise ValueError("a robot is outside the grid")
    return cells


def assign_goals_path(state, clusters: np.ndarray, robots_xy, origin_x: float, origin_y: float, resolution: float,
                      min_size: int = 8, distance_weight: float = 1.0, min_distance: float = 0.0,
                      inflate_cells: int = 2, max_cost: int = 0, snap_cells: int = 5, cache: dict | None = None):
    """dm.goals.assign_goals scored by path length: per robot, in order,
    (cluster index, (x, y) centre of the snapped cell, snapped cell) or None.
    dist = cost * resolution / 5 from the robot's own field to the cluster
    centroid's snapped cell; clusters that are not reached are not eligible.
    `cache`: a dict the per-robot fields are kept in (keyed by the robot's
    cell) for further calls on the same state, inflation and max_cost."""
    if not float(distance_weight) >= 0.0:
        raise ValueError("distance_weight must be >= 0 (dm_assign_goals_path rejects it too)")
    st = np.asarray(state)
    H, W = st.shape
    cells = _robot_cells(robots_xy, origin_x, origin_y, resolution, W, H)
    if clusters is None or len(clusters) == 0:
        return [None] * len(cells)
    got = _greedy_goals(st, clusters, cells, origin_x, origin_y, resolution, min_size, distance_weight, min_distance,
                        inflate_cells, max_cost, snap_cells, cache, lambda i, cell: int(clusters["size"][i]))
    return [g and g[:3] for g in got]


# ---- team planning (dm_plan_team, dm_assign_goals_team) ----------------------
TEAM_MAX = 64


def team_fields(state, robot_cells, r: int, max_cost: int = 0) -> list[np.ndarray]:
    """dm_plan_team: one field per robot cell (cx, cy), each `field` from that
    cell alone.  A robot's own cell is traversable (with_sources) in its own
    field only; the traversable mask is shared."""
    cells = [(int(cx), int(cy)) for cx, cy in robot_cells]
    if not 1 <= len(cells) <= TEAM_MAX:
        raise ValueError(f"n_robots must be in [1, {TEAM_MAX}]")
    trav = traversable(state, r)
    return [field(state, [c], r, max_cost, trav=trav) for c in cells]


def global_greedy(util: np.ndarray, labels) -> list[int]:
    """The pick of dm_assign_goals_team over util [R, K] (-inf: not eligible):
    among the pairs (r, c) with r unassigned and c untaken take the greatest
    util, ties to the smaller label, then the smaller r; until no pair is
    left.  Per robot the cluster index, or -1."""
    u = np.array(util, np.float64)
    R, K = u.shape
    labels = np.asarray(labels)
    out = [-1] * R
    while True:
        m = u.max() if u.size else -np.inf
        if not np.isfinite(m):
            return out
        rs, cs = np.nonzero(u == m)
        j = np.lexsort((rs, labels[cs]))[0]  # by label, then by robot
        r, c = int(rs[j]), int(cs[j])
        out[r] = c
        u[r, :] = -np.inf
        u[:, c] = -np.inf


def assign_goals_team(state, clusters: np.ndarray, robots_xy, origin_x: float, origin_y: float, resolution: float,
                      min_size: int = 8, min_gain: int = 0, distance_weight: float = 1.0, min_distance: float = 0.0,
                      inflate_cells: int = 2, max_cost: int = 0, snap_cells: int = 5, radius_cells: int = 0):
    """dm_assign_goals_team: the global-greedy assignment over the robots'
    team fields.  radius_cells == 0: dist, eligibility and util of
    assign_goals_path (numerator: the cluster's size), per robot (cluster
    index, (x, y) centre of the snapped cell, snapped cell) or None;
    radius_cells >= 1: those of dm.gain.assign_goals_gain (numerator: the
    visible-unknown count of the snapped cell under that robot's field,
    >= min_gain and > 0), per robot (index, (x, y), cell, gain) or None."""
    if not float(distance_weight) >= 0.0:
        raise ValueError("distance_weight must be >= 0 (dm_assign_goals_team rejects it too)")
    gain_mode = int(radius_cells) != 0
    if gain_mode:
        from . import gain as _gain

        R_view = _gain.check_radius(radius_cells)
        if int(min_gain) < 0:
            raise ValueError("min_gain must be >= 0")
    st = np.asarray(state)
    H, W = st.shape
    cells = _robot_cells(robots_xy, origin_x, origin_y, resolution, W, H)
    if len(cells) > TEAM_MAX:
        raise ValueError(f"n_robots must be in [0, {TEAM_MAX}]")
    if not cells or clusters is None or len(clusters) == 0:
        return [None] * len(cells)
    fields = team_fields(st, cells, inflate_cells, max_cost)
    targets = [cell_of(float(c["cx_m"]), float(c["cy_m"]), origin_x, origin_y, resolution, W, H) for c in clusters]
    K = len(clusters)
    util = np.full((len(cells), K), -np.inf)
    snapped = np.full((len(cells), K), -1, np.int64)
    num = np.zeros((len(cells), K), np.int64)
    gains: dict = {}
    for r, f in enumerate(fields):
        got = [snap(f, t, snap_cells) for t in targets]
        cost = np.array([s[0] for s in got], np.uint32)
        snapped[r] = [s[1] for s in got]
        dist = cost.astype(np.float64) * float(resolution) / 5.0
        if gain_mode:
            for i, cell in enumerate(snapped[r]):
                if cell >= 0:
                    if cell not in gains:
                        gains[cell] = _gain.visible_unknown(st, (int(cell % W), int(cell // W)), R_view)
                    num[r, i] = gains[cell]
        else:
            num[r] = clusters["size"]
        ok = (clusters["size"] >= min_size) & (cost != UNREACHABLE) & (dist >= min_distance) & (num[r] > 0)
        if gain_mode:
            ok &= num[r] >= int(min_gain)
        util[r] = np.where(ok, num[r].astype(np.float64) / (1.0 + float(distance_weight) * dist), -np.inf)
    out = []
    for r, i in enumerate(global_greedy(util, clusters["label"])):
        if i < 0:
            out.append(None)
            continue
        cell = int(snapped[r, i])
        xy = (origin_x + ((cell % W) + 0.5) * resolution, origin_y + ((cell // W) + 0.5) * resolution)
        out.append((i, xy, cell, int(num[r, i])) if gain_mode else (i, xy, cell))
    return out

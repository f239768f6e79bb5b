"""Seeded inputs shared by the partial-build matcher tests (CPU:
test_match_partial_host.py, GPU: test_gpu_match_partial.py): one 500 x 390 map
(8 x 7 tiles, the last tile column and row ragged) with range_max = 1.6 m, so a
search window reaches a few of its 56 tiles, and poses whose windows end
exactly on a tile's first or last column or row, lie apart, hang over the
map's edges, or miss the map.

tiles_read states from dm.match.fine_coords which tiles a search reads; it
knows nothing of how the library bounds a window."""
from __future__ import annotations

import functools
import math

import numpy as np

import cases
from dm import match

W, H = 500, 390
TILE = 64
TX, TY = -(-W // TILE), -(-H // TILE)  # 8, 7
RANGE_MAX = 1.6
RANGE_CELLS = 32                       # range_max / resolution
N = 48
AMIN, INC = 0.0, float(np.float32(2.0 * math.pi / N))
FULL_BEAMS = {"+x": 0, "+y": 12, "-x": 24, "-y": 36}  # at exactly float32(range_max): the gate is inclusive

SMEAR = 4
GAUSS4 = match.kernel_table(0.1, 0.05, SMEAR)
OFFSETS = np.array([-0.05, 0.0, 0.05])
K0 = 1
SEARCHES = ((5, 10, 2), (1, 32, 1), (16, 32, 16))  # sub, half, stride: 4, 32 and 32 cells of translation

# dm_match_global
G_OFFSETS = np.array([-0.3, -0.2, -0.1, -0.05, 0.0, 0.1, 0.2, 0.3])
G_K0, G_HALF_X, G_HALF_Y = 4, 40, 30
BLOCKS = (4, 8, 16, 32)


def params():
    return cases.make_params(W, H, range_max=RANGE_MAX)


@functools.lru_cache(maxsize=None)
def state() -> np.ndarray:
    """67 % free, 25 % unknown, 8 % occupied: GAUSS4's response is non-zero on
    98 % of the cells, so a tile that was not built shows in a score.  Shared
    and never modified."""
    st = np.random.default_rng(5).choice(np.array([0, -1, 100], np.int8), size=(H, W), p=[0.67, 0.25, 0.08])
    st.setflags(write=False)
    return st


def poison_table(r=SMEAR, seed=1) -> np.ndarray:
    """A non-monotone table of the same radius: a tile left over from it gives other scores."""
    k = np.random.default_rng(seed).integers(0, 256, r * r + 1).astype(np.uint8)
    assert np.any(np.diff(k.astype(int)) > 0)
    return k


POISON = poison_table()
OTHER4 = match.kernel_table(0.07, 0.05, SMEAR)  # the same radius, another table
GAUSS6 = match.kernel_table(0.1, 0.05, 6)       # another radius


def ranges(S=1, seed=6) -> np.ndarray:
    """float32 [S, N] uniform in [0.3, 1.6], the four axis beams at exactly float32(1.6)."""
    r = np.random.default_rng(seed).uniform(0.3, RANGE_MAX, (S, N)).astype(np.float32)
    r[:, sorted(FULL_BEAMS.values())] = np.float32(RANGE_MAX)
    return r


def at_cell(cx: float, cy: float, yaw: float = 0.0):
    """The pose at cell coordinates (cx, cy), fractions included, e.g. (156.5, 100.5) for a cell's centre."""
    p = params()
    return (p.origin_x + cx * p.resolution, p.origin_y + cy * p.resolution, yaw)


def translation_cells(search) -> int:
    sub, half, stride = search
    assert (half * stride) % sub == 0
    return half * stride // sub


def edge_pose(direction: str, search=SEARCHES[0]):
    """(pose, beam, cell, axis, sign): yaw 0, the full-range beam along
    `direction` ends RANGE_CELLS cells from the pose's cell, and only the
    extreme translation (i or j = sign * half) moves it into `cell`, which is
    the first column / row of a tile for "+x" / "+y" (192, 128) and the last
    one for "-x" / "-y" (127).

    The pose sits 0.3 of a cell (0.7 for the negative directions) into its
    cell along that axis, not at the centre: at sub = 5, stride = 2 the
    endpoint of a centred pose is fine step 2 of 5 in its cell, and the
    translation half - 1 (18 fine steps) would then reach the same cell as
    half (20 fine steps).  At 0.3 the endpoint is fine step 1: 18 steps end one
    cell short."""
    T = translation_cells(search)
    if direction == "+x":
        cell = 192
        return at_cell(cell - RANGE_CELLS - T + 0.3, 100.5), FULL_BEAMS[direction], cell, 0, +1
    if direction == "-x":
        cell = 127
        return at_cell(cell + RANGE_CELLS + T + 0.7, 100.5), FULL_BEAMS[direction], cell, 0, -1
    if direction == "+y":
        cell = 128
        return at_cell(156.5, cell - RANGE_CELLS - T + 0.3), FULL_BEAMS[direction], cell, 1, +1
    if direction == "-y":
        cell = 127
        return at_cell(156.5, cell + RANGE_CELLS + T + 0.7), FULL_BEAMS[direction], cell, 1, -1
    raise ValueError(direction)


DIRECTIONS = ("+x", "-x", "+y", "-y")

POSE_A = edge_pose("+x")[0]                  # cell (156, 100): the window ends on column 192
POSE_B = at_cell(400.5, 300.5, 1.0)          # apart from A; dm_match_global's window reaches the ragged tile column
POSE_C = at_cell(W - 3.5, H - 3.5, 0.4)      # 3 cells inside the upper-right corner: mostly off the map
POSE_D = at_cell(-19.5, 200.5, 0.1)          # 20 cells outside the left edge: a negative pose cell
POSE_E = (1.0e7, 0.0, 0.3)                   # used beams, but no tile within reach
POSE_F = at_cell(1.5 * 2.0 ** 30, 195.5, 0.0)  # every beam fails |q| < 2^30


def scan_args(poses, search=SEARCHES[0], kern=GAUSS4, smear=SMEAR, rng=None):
    """Positional arguments of match_scans behind the state / mapper: S = len(poses) scans."""
    sub, half, stride = search
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    r = ranges(poses.shape[0]) if rng is None else rng
    return (poses, r, AMIN, INC, OFFSETS, K0, sub, half, stride, smear, kern)


def global_args(poses, rng=None):
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    r = ranges(poses.shape[0]) if rng is None else rng
    return (poses, r, AMIN, INC, G_OFFSETS)


def global_kw(kern=GAUSS4, smear=SMEAR, half_x=G_HALF_X, half_y=G_HALF_Y):
    return dict(k0=G_K0, half_x=half_x, half_y=half_y, smear_cells=smear, kern=kern)


def tiles_read(poses, rng, offsets, sub, stride, half_x, half_y=None, i_values=None, j_values=None) -> np.ndarray:
    """bool [TY, TX]: the tiles that hold an in-grid cell some candidate (k, i,
    j) of some scan reads: the cell (floordiv(qx + i*stride, sub), floordiv(qy +
    j*stride, sub)) of every used beam of every candidate yaw, for i in
    [-half_x, half_x] and j in [-half_y, half_y] (or the given i_values /
    j_values).  The definition of the score, restated; no window arithmetic."""
    half_y = half_x if half_y is None else half_y
    qx, qy, used = match.fine_coords(params(), poses, rng, AMIN, INC, offsets, sub)
    i = np.arange(-half_x, half_x + 1) if i_values is None else np.asarray(i_values, np.int64)
    j = np.arange(-half_y, half_y + 1) if j_values is None else np.asarray(j_values, np.int64)
    cx = (qx[used][:, None] + i[None, :] * stride) // sub  # [beams, translations]
    cy = (qy[used][:, None] + j[None, :] * stride) // sub
    cols = np.zeros((cx.shape[0], TX), np.int64)
    rows = np.zeros((cy.shape[0], TY), np.int64)
    for t in range(TX):
        cols[:, t] = ((cx >= 0) & (cx < W) & (cx // TILE == t)).any(axis=1)
    for t in range(TY):
        rows[:, t] = ((cy >= 0) & (cy < H) & (cy // TILE == t)).any(axis=1)
    return (rows.T @ cols) > 0  # a beam reads every (row tile, column tile) pair of its own


def tiles_read_scans(poses, search=SEARCHES[0], rng=None, **kw) -> np.ndarray:
    sub, half, stride = search
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    return tiles_read(poses, ranges(poses.shape[0]) if rng is None else rng, OFFSETS, sub, stride, half, **kw)


def tiles_read_global(poses, half_x=G_HALF_X, half_y=G_HALF_Y, rng=None) -> np.ndarray:
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    return tiles_read(poses, ranges(poses.shape[0]) if rng is None else rng, G_OFFSETS, 1, 1, half_x, half_y)


_fields: dict = {}


def field(st, smear=SMEAR, kern=GAUSS4) -> np.ndarray:
    """dm.match.response_field of the whole state image, kept per (state, table)."""
    st = np.ascontiguousarray(st, np.int8)
    key = (hash(st.tobytes()), int(smear), bytes(np.asarray(kern, np.uint8).tobytes()))
    if key not in _fields:
        _fields[key] = match.response_field(st, smear, kern)
    return _fields[key]


def host_scans(st, args) -> dict:
    """dm.match.match_scans on the full host field of `st`."""
    return match.match_scans(st, params(), *args, field=field(st, args[-2], args[-1]))


def host_global(st, args, kw) -> dict:
    return match.match_global(st, params(), *args, **kw, field=field(st, kw["smear_cells"], kw["kern"]))

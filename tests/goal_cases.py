"""Deterministic cases shared by the goal-selection tests past one sort chunk
(CPU: test_goal_cases_host.py, GPU: test_gpu_goals_chunks.py).

csrc/dm_goals.hip ranks clusters in chunks of CHUNK = 4096 records and folds
`per = CHUNK // T` chunk lists per merge workgroup (T = n_robots), level after
level.  With 256 robots per = 16, so a second merge level needs more than
16 * 4096 records: `lattice_state` builds maps with exactly that many clusters.
The field-scored calls (path, gain, coord) compute one field per robot on the
host reference, so their case (`room_state`) is a small map with a little more
than one chunk of clusters.
"""
from __future__ import annotations

import functools

import numpy as np

import cases
import dm
import np_oracle

CHUNK = 4096                      # kGoalN of csrc/dm_goals.hip
TWO_LEVELS = 16 * CHUNK           # 16 lists: the most one merge workgroup folds for 256 robots

# ---- the straight-line form: a lattice of isolated runs -----------------------

# Horizontal runs of 1 to 3 free cells in unknown space at pitch 4 in x and 2
# in y: no two runs are 8-adjacent, so each is one frontier cluster of its
# length, and the label order (smallest linear index) is the site order, row
# after row.  275 * 239 = 65725 sites hold the largest case.
LAT_W, LAT_H = 1100, 477
LAT_PER_ROW, LAT_ROWS = LAT_W // 4, (LAT_H + 1) // 2
LATTICE_KS = (TWO_LEVELS + 100, TWO_LEVELS + 1, TWO_LEVELS)


def lattice_params():
    return cases.make_params(LAT_W, LAT_H)


def lattice_sizes(K: int) -> np.ndarray:
    """The run length of record i, int64 [K].  Size 3 is rare (fewer than 256
    records in all) and lies in three places: the first chunk, the middle, and
    the last 100 records; the rest alternate 1 and 2 without a period that
    divides the row length."""
    i = np.arange(K, dtype=np.int64)
    size = 1 + ((i * 7 + i // LAT_PER_ROW) % 3 == 0).astype(np.int64)
    three = ((i < CHUNK) & (i % 97 == 5)) | (i % 1021 == 3) | ((i >= K - 100) & ((K - 1 - i) % 7 == 0))
    size[three] = 3
    return size


def lattice_state(K: int, sizes=None):
    """(state int8 [LAT_H, LAT_W], K): the first K lattice sites hold a run
    (the sites behind them are knocked out), site i one of length sizes[i]
    (default lattice_sizes(K))."""
    K = int(K)
    if not 0 <= K <= LAT_PER_ROW * LAT_ROWS:
        raise ValueError("K does not fit the lattice")
    size = lattice_sizes(K) if sizes is None else np.asarray(sizes, np.int64)
    if size.shape != (K,) or size.min(initial=1) < 1 or size.max(initial=1) > 3:
        raise ValueError("sizes: K run lengths in 1..3")
    st = np.full((LAT_H, LAT_W), -1, np.int8)
    i = np.arange(K, dtype=np.int64)
    y, x = 2 * (i // LAT_PER_ROW), 4 * (i % LAT_PER_ROW)
    for d in range(3):
        on = size > d
        st[y[on], x[on] + d] = 0
    return st, K


def lattice_site_xy(p, i: int):
    """The centre (metres) of the first cell of site i."""
    return (p.origin_x + (4 * (i % LAT_PER_ROW) + 0.5) * p.resolution,
            p.origin_y + (2 * (i // LAT_PER_ROW) + 0.5) * p.resolution)


def lattice_robots(kind: str, K: int, R: int) -> np.ndarray:
    """float64 [R, 2].  "random": anywhere on the map and a little outside it;
    "last": all at one point a cell below the last record's row, so the best
    clusters are the highest labels; "first": all at one point beside record
    0's row."""
    p = lattice_params()
    if kind == "random":
        rng = np.random.Generator(np.random.PCG64(1000 * R + K % 1000))
        return np.stack([p.origin_x + rng.uniform(-0.05, 1.05, R) * LAT_W * p.resolution,
                         p.origin_y + rng.uniform(-0.05, 1.05, R) * LAT_H * p.resolution], axis=1)
    if kind == "last":
        x, y = lattice_site_xy(p, K - 1)
        return np.tile([x + 0.013, y + p.resolution + 0.007], (R, 1))
    if kind == "first":
        x, y = lattice_site_xy(p, 0)
        return np.tile([x + 0.021, y + p.resolution - 0.004], (R, 1))
    raise ValueError(kind)


# what test_gpu_goals_chunks.py runs per (K, R): (name, robot kind, keywords)
LATTICE_SETTINGS = (
    ("random", "random", dict(min_size=1)),
    ("stacked_last", "last", dict(min_size=1)),
    ("stacked_first", "first", dict(min_size=1)),
    ("all_ties", "random", dict(min_size=1, distance_weight=0.0)),
    ("size3_only", "random", dict(min_size=3)),
)


def clusters_of(p, st) -> np.ndarray:
    """The label-sorted cluster records of a state image, by the numpy oracle."""
    return np.array(np_oracle.frontiers(p, st)[2], dtype=np.dtype(dm.CLUSTER_DTYPE))


@functools.lru_cache(maxsize=None)
def lattice_clusters(K: int) -> np.ndarray:
    a = clusters_of(lattice_params(), lattice_state(K)[0])
    a.setflags(write=False)
    return a


# ---- the field-scored forms: a room with a little more than one chunk ---------

ROOM_N = 272                      # 4 * 64 + 16: the last tile is ragged
ROOM_KW = dict(inflate_cells=1, snap_cells=2, radius_cells=6)
ROOM_SETTINGS = (dict(min_size=1), dict(min_size=1, distance_weight=0.25, min_distance=1.0))
# (y0, y1, x0, x1) of the unknown patches
ROOM_PATCHES = ((30, 33, 200, 203), (61, 66, 41, 46), (141, 143, 121, 123), (213, 217, 149, 153), (250, 257, 90, 97),
                (257, 261, 221, 225))
ROOM_BOX = (180, 230)             # the sealed box: occupied border rows / columns


def room_params():
    return cases.make_params(ROOM_N, ROOM_N)


@functools.lru_cache(maxsize=None)
def _room():
    st = np.zeros((ROOM_N, ROOM_N), np.int8)
    st[2::4, 2::4] = -1                           # 68 x 68 single unknown cells, each ringed by 8 frontier cells
    for y0, y1, x0, x1 in ROOM_PATCHES:
        st[y0:y1, x0:x1] = -1
    st[100:102, 0:200] = 100                      # the wall: a detour round its right end
    lo, hi = ROOM_BOX
    st[lo:hi + 1, lo] = st[lo:hi + 1, hi] = 100   # the sealed box
    st[lo, lo:hi + 1] = st[hi, lo:hi + 1] = 100
    st.setflags(write=False)
    cl = clusters_of(room_params(), st)
    cl.setflags(write=False)
    return st, cl


def room_state() -> np.ndarray:
    """int8 [272, 272], read-only."""
    return _room()[0]


def room_clusters() -> np.ndarray:
    return _room()[1]


def room_centre(cx: int, cy: int):
    p = room_params()
    return (p.origin_x + (cx + 0.5) * p.resolution, p.origin_y + (cy + 0.5) * p.resolution)


# free cells (cx, cy): x, y = 0 mod 4 lies between the rings.  The first stands on a ring the wall
# shadows, the sixth on a ring the map's edge cuts: their nearest cluster has a gain below the median.
ROOM_SPREAD_CELLS = ((138, 97), (240, 20), (60, 96), (60, 104), (140, 140), (18, 269), (200, 264), (260, 244))
ROOM_STACKED_CELL = (136, 244)


def room_robots(kind: str) -> np.ndarray:
    """float64 [8, 2].  "spread": 8 distinct free cells on both sides of the
    wall and of the row where record 4096 lies; "stacked": one free cell beside
    that row, 8 times."""
    if kind == "spread":
        return np.array([room_centre(x, y) for x, y in ROOM_SPREAD_CELLS])
    if kind == "stacked":
        return np.array([room_centre(*ROOM_STACKED_CELL)] * 8)
    raise ValueError(kind)


def room_held():
    """The one held view of the coord calls: beside the stacked robots, so it
    takes gain from clusters on both sides of record 4096."""
    return [room_centre(ROOM_STACKED_CELL[0] + 4, ROOM_STACKED_CELL[1])]


def room_gains(cache: dict) -> np.ndarray:
    """The gain (radius ROOM_KW) of every room cluster whose centroid snaps under
    the field of the stacked robots' cell, 0 elsewhere; uint32 [K].  `cache`:
    the dict of the restatements (fields and gains are kept in it)."""
    from dm import gain, plan

    st, cl = _room()
    p = room_params()
    f = cache.get(ROOM_STACKED_CELL)
    if f is None:
        f = cache[ROOM_STACKED_CELL] = plan.field(st, [ROOM_STACKED_CELL], ROOM_KW["inflate_cells"])
    out = np.zeros(len(cl), np.uint32)
    for i, c in enumerate(cl):
        t = plan.cell_of(float(c["cx_m"]), float(c["cy_m"]), p.origin_x, p.origin_y, p.resolution, ROOM_N, ROOM_N)
        _, cell = plan.snap(f, t, ROOM_KW["snap_cells"])
        if cell >= 0:
            key = ("gain", ROOM_KW["radius_cells"], cell)
            if key not in cache:
                cache[key] = gain.visible_unknown(st, (cell % ROOM_N, cell // ROOM_N), ROOM_KW["radius_cells"])
            out[i] = cache[key]
    return out


def room_min_gain(cache: dict) -> int:
    """The median gain of the reached clusters: a min_gain that leaves clusters
    on both of its sides in both chunks."""
    g = room_gains(cache)
    return int(np.median(g[g > 0]))

"""Maps shared by tests/test_plan_team_host.py (CPU) and
tests/test_gpu_plan_team.py: the corridor on which the order of the robots
decides what dm_assign_goals_path assigns, and the corridor of ties.  All
cells are occupied except a corridor; a frontier cluster is a row of the
corridor's cells under a notch of unknown cells cut into its wall.  Used with
inflate_cells = 0."""
import numpy as np

import np_oracle
from dm import _ffi

KW = dict(min_size=1, distance_weight=1.0, min_distance=0.0, inflate_cells=0, snap_cells=2)


def clusters_of(p, st):
    """The frontier clusters of a state image as the device reports them
    (label-sorted records), from the numpy oracle."""
    return np.array(np_oracle.frontiers(p, st)[2], dtype=np.dtype(_ffi.CLUSTER_DTYPE))


def centre(p, cx, cy):
    return (p.origin_x + (cx + 0.5) * p.resolution, p.origin_y + (cy + 0.5) * p.resolution)


def order_matters():
    """64 x 192, a corridor of rows 28..35.  Cluster B (index 0) is the ten
    cells (15..24, 28), cluster A (index 1) the ten cells (95..104, 28).
    Robot 1 stands beside A; robot 0 is a little farther from A and much
    farther from B.  Robots choosing in order: 0 takes A, 1 is left with B,
    80 cells away.  The best pair first: 1 takes A, 0 takes B.
    Returns (state, robot cells [(cx, cy)], index of A, index of B)."""
    st = np.full((64, 192), 100, np.int8)
    st[28:36, 8:184] = 0
    st[27, 16:24] = -1
    st[27, 96:104] = -1
    return st, [(112, 30), (100, 30)], 1, 0


def ties():
    """64 x 192, a corridor of rows 28..36.  Cluster X (index 0: the smaller
    label) is the nine cells (92..100, 28) under a notch in the upper wall,
    cluster Y (index 1) the nine cells (52..60, 36) over a notch in the lower
    wall; their centroids are the cells (96, 28) and (56, 36).  P = (76, 32)
    is 20 columns and 4 rows from both: X and Y have equal util for P.
    Q = (116, 32) is as far from X as P is: X is equally good for P and Q.
    Returns (state, P, Q, index of X, index of Y)."""
    st = np.full((64, 192), 100, np.int8)
    st[28:37, 8:184] = 0
    st[27, 93:100] = -1
    st[37, 53:60] = -1
    return st, (76, 32), (116, 32), 0, 1

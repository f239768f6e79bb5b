"""Seeded cases shared by the map-fusion tests (CPU and GPU): one destination
map, the source maps and the table of transforms.

Destination: 200 x 136 cells (ragged tiles on both axes) at 0.05 m, pre-filled
by a few dm.synth scans of 2.5 m range in its lower left part, so most tiles
stay unseen and some cells sit at l_max / l_min.  Sources: 96 x 70 log-odds
maps integrated from scans (exact zeros outside the scans' reach, values at the
clamps) with one NaN and one inf cell, and their state images with a stray 50.
Every case but "outside" must contribute and change states in both modes and
cover fewer cells than the destination has (tests/test_fuse_host.py checks it
with the restatement); "outside" covers nothing.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import cases
from dm import fuse, synth

DST_W, DST_H = 200, 136
SRC_W, SRC_H = 96, 70
MODES = ("add", "fill")
KINDS = ("logodds", "state")


def dst_params(**kw):
    return cases.make_params(DST_W, DST_H, 0.05, range_max=2.5, **kw)


@functools.lru_cache(maxsize=None)
def dst_batches():
    """The scans that pre-fill the destination: 2 robots, 6 steps, 90 beams,
    in the lower left 6 m x 4.4 m of the 10 m x 6.8 m map."""
    p = dst_params()
    world = synth.make_world(11, -5.0, -3.4, 5.0, 3.4)
    stream = synth.ScanStream(world, 2, 90, 12, step=0.05, region=(-5.0, -3.4, 1.0, 1.0))
    batches = [stream.next_batch() for _ in range(6)]
    return p, batches, float(synth.LD06_ANGLE_MIN), float(synth.ld06_angle_increment(90))


@functools.lru_cache(maxsize=None)
def more_batches():
    """Further scans integrated after a fusion (the derived-structure test)."""
    world = synth.make_world(11, -5.0, -3.4, 5.0, 3.4)
    stream = synth.ScanStream(world, 2, 90, 13, step=0.05, region=(-3.0, -3.0, 4.0, 3.0))
    return [stream.next_batch() for _ in range(3)]


@functools.lru_cache(maxsize=None)
def dst_logodds():
    """The pre-filled destination's log-odds by the CPU oracle (bit-equal to
    the device's after the same scans).  Shared and never modified."""
    import oracle

    p, batches, amin, inc = dst_batches()
    om = oracle.OracleMap(p)
    for poses, ranges in batches:
        om.integrate(poses, ranges, amin, inc)
    L = om.L.copy()
    L.setflags(write=False)
    return L


def prefill(mapper):
    """Integrate the destination's scans into a device mapper."""
    _, batches, amin, inc = dst_batches()
    for poses, ranges in batches:
        mapper.integrate(poses, ranges, amin, inc)


@functools.lru_cache(maxsize=None)
def source(res=0.05):
    """(geometry dict, log-odds float32 [70, 96], state int8 [70, 96]) of the
    source map at resolution `res`, centred on its frame's origin: scans of a
    world of its own by the CPU oracle, then one NaN and one inf cell; the
    state image is a7 of the log-odds with a stray 50.  Shared, never modified."""
    import oracle

    w, h = SRC_W * res, SRC_H * res
    p = cases.make_params(SRC_W, SRC_H, res, range_max=30 * res)
    # the walls lie 0.3 m outside the map; the robots start at least 0.3 m inside it
    world = synth.make_world(21, -0.5 * w - 0.5, -0.5 * h - 0.5, 0.5 * w + 0.5, 0.5 * h + 0.5, density=0.05,
                             size_lo=4 * res, size_hi=12 * res)
    stream = synth.ScanStream(world, 2, 90, 22, step=res, region=(-0.5 * w - 0.7, -0.5 * h - 0.7, 0.5 * w + 0.7,
                                                                   0.5 * h + 0.7))
    om = oracle.OracleMap(p)
    inc = float(synth.ld06_angle_increment(90))
    for _ in range(6):
        poses, ranges = stream.next_batch()
        om.integrate(poses, ranges, float(synth.LD06_ANGLE_MIN), inc)
    L = om.L.copy()
    st = om.state.copy()
    known = np.argwhere(L != 0)
    ny, nx = known[len(known) // 3]
    iy, ix = known[2 * len(known) // 3]
    L[ny, nx] = np.nan
    L[iy, ix] = np.inf
    st[ny, nx] = 50
    L.setflags(write=False)
    st.setflags(write=False)
    return fuse.geom_of(p), L, st


# name, source resolution, transform (tx, ty, yaw), source origin override
CASES = [
    ("identity_origin", 0.05, (0.0, 0.0, 0.0), (-4.0, -3.0)),
    ("shift_cells", 0.05, (-1.85, -1.2, 0.0), None),
    ("shift_half_cell", 0.05, (-1.825, -1.175, 0.0), None),
    ("quarter_turn", 0.05, (-1.5, -1.0, math.pi / 2), None),
    ("yaw_0.3", 0.05, (-1.0, -0.7, 0.3), None),
    ("yaw_-2.5_coarse", 0.1, (-0.2, 0.1, -2.5), None),
    ("yaw_-2.5_fine", 0.025, (-0.6, 0.5, -2.5), None),
    ("over_left", 0.05, (-5.0, 2.3, 0.1), None),
    ("over_right", 0.05, (5.0, 0.5, -0.2), None),
    ("over_bottom", 0.05, (-1.0, -3.4, 0.2), None),
    ("over_top", 0.05, (0.5, 3.4, 0.15), None),
    ("outside", 0.05, (50.0, 50.0, 0.3), None),
]
CASE_NAMES = [c[0] for c in CASES]


def case(name):
    """(geometry, log-odds, state, transform) of a named case."""
    _, res, transform, origin = CASES[CASE_NAMES.index(name)]
    geom, L, st = source(res)
    if origin is not None:
        geom = dict(geom, origin_x=origin[0], origin_y=origin[1])
    return geom, L, st, transform


def expected(L_dst, p, name, mode, kind):
    """dm.fuse.fuse_map of a named case on destination log-odds L_dst."""
    geom, L, st, transform = case(name)
    if kind == "state":
        return fuse.fuse_map(L_dst, p, st, geom, transform, mode, src_is_state=True)
    return fuse.fuse_map(L_dst, p, L, geom, transform, mode)


def check_stats(name, stats, n_cells=DST_W * DST_H):
    """What every case asserts of its stats."""
    if name == "outside":
        assert stats == {"covered": 0, "contributing": 0, "changed": 0}
        return
    assert stats["contributing"] > 0 and stats["changed"] > 0, (name, stats)
    assert stats["covered"] < n_cells, (name, stats)

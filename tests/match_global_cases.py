"""Seeded cases shared by the relocalisation tests (CPU and GPU): the small
ragged tie map, the recovery case with a far prior, and the relocalising ROS
node's stand-in mapper and run."""
from __future__ import annotations

import functools
import math

import numpy as np

import cases
import match_cases
from dm import match

FAR = (2.3, -1.7, 0.9)  # the recovery case's prior error, and the node's odometry frame offset


def full_circle(A):
    """A yaw offsets over the full circle, index A // 2 the zero offset."""
    return np.array([(m - A // 2) * (2.0 * math.pi / A) for m in range(A)], np.float64), A // 2


def ragged_map(H=128, W=96):
    """96 wide (no multiple of 64) x 128, 3 % occupied cells (PCG64 seed 7), the rest free."""
    rng = np.random.Generator(np.random.PCG64(7))
    return np.where(rng.random((H, W)) < 0.03, 100, 0).astype(np.int8)


def ragged_scans(S=1, N=24, seed=6):
    """S scans of N beams up to 2 m with two NaN beams each."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ranges = rng.uniform(0.1, 2.0, (S, N)).astype(np.float32)
    ranges[:, 5] = np.nan
    ranges[:, 17] = np.nan
    return ranges, 0.0, float(np.float32(2.0 * math.pi / N))


RAGGED = dict(k0=4, half_x=20, half_y=13, smear_cells=0, kern=np.array([255], np.uint8))
RAGGED_OFFSETS = np.array([-0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3])
RAGGED_PRIOR = (0.3, -0.4, 0.2)


@functools.lru_cache(maxsize=None)
def recovery():
    """match_cases.recovery_case with the prior off by FAR, its response field
    at sigma = 0.1, r = 4, and 64 yaws over the full circle.  Shared and never
    modified."""
    p, st, ranges, amin, inc, true, _ = match_cases.recovery_case()
    prior = (true[0] + FAR[0], true[1] + FAR[1], true[2] + FAR[2])
    kern = match.kernel_table(0.1, 0.05, 4)
    V = match.response_field(st, 4, kern)
    off, k0 = full_circle(64)
    return dict(p=p, st=st, ranges=ranges, amin=amin, inc=inc, true=true, prior=prior, kern=kern, V=V, off=off, k0=k0)


@functools.lru_cache(maxsize=None)
def recovery_host(half=100):
    """dm.match.match_global on the recovery case: A = 64, the given half."""
    c = recovery()
    return match.match_global(c["st"], c["p"], [c["prior"]], c["ranges"], c["amin"], c["inc"], c["off"], c["k0"], half,
                              half, 4, c["kern"], field=c["V"])


# -- the relocalising node ----------------------------------------------------------
# the node tests search a 200^2 map: the host restatement of the whole-map
# search (A = 89; a coarser yaw step finds the room's half-turn twin) takes a second there
NODE_SLAM = dict(coarse_angle_resolution=0.07, loop_search_space_smear_deviation=0.1,
                 loop_match_minimum_response_coarse=0.35, loop_match_minimum_response_fine=0.45)


def node_case(n_steps=4, size=200):
    """A drive (match_cases.drive) on a size^2 map whose first scans are already
    in the map; the odometry frame is the map frame moved by FAR."""
    from dm.ros_node import se2_compose, se2_inverse

    p, amin, inc, true, _, scans = match_cases.drive(n_steps=n_steps, size=size, bias=(0.0, 0.0, 0.0))
    # odom = FAR^-1 o true: map_to_odom must come out as FAR
    odom = [se2_compose(se2_inverse(FAR), q) for q in true]
    return p, amin, inc, true, odom, scans


def built_map(p, true, scans, amin, inc):
    """The state image of the map the node loads: the drive's scan endpoints."""
    return match_cases.endpoint_map(p, true, scans, amin, inc)

"""Seeded cases shared by the scan matcher's tests (CPU and GPU): the
recovery case and the biased-odometry drive of the ROS node tests."""
from __future__ import annotations

import math

import numpy as np

import cases
from dm import synth


def endpoint_map(p, poses, scans, amin, inc) -> np.ndarray:
    """An int8 state image with the endpoints of the scans' in-range beams
    occupied and everything else unknown."""
    H, W = int(p.height), int(p.width)
    st = np.full((H, W), -1, np.int8)
    for (x, y, yaw), r in zip(poses, scans):
        r = np.asarray(r, np.float64)
        phi = float(amin) + np.arange(r.shape[0]) * float(inc)
        ok = np.isfinite(r) & (r >= p.range_min) & (r <= p.range_max)
        cx = np.floor((x + r[ok] * np.cos(yaw + phi[ok]) - p.origin_x) / p.resolution).astype(np.int64)
        cy = np.floor((y + r[ok] * np.sin(yaw + phi[ok]) - p.origin_y) / p.resolution).astype(np.int64)
        inside = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        st[cy[inside], cx[inside]] = 100
    return st


def free_pose(world, rng, lo, hi, margin=0.4):
    while True:
        x, y = rng.uniform(lo, hi), rng.uniform(lo, hi)
        if not world.occupied(x, y, margin=margin):
            return x, y


def recovery_case(seed=3, n_beams=450, offset=(0.07, -0.04, 0.05)):
    """A 20 m room (synth.make_world) on a 400^2 map of 5 cm cells; the map
    holds the scan endpoints of five true poses around a centre pose; the scan
    to match is taken from the centre pose and its prior is off by `offset`.
    Returns (params, state, ranges [N], angle_min, angle_increment, true pose,
    prior pose)."""
    p = cases.make_params(400, 400, 0.05)
    world = synth.make_world(seed, -10.0, -10.0, 10.0, 10.0)
    rng = np.random.Generator(np.random.PCG64(seed + 100))
    amin, inc = float(synth.LD06_ANGLE_MIN), float(synth.ld06_angle_increment(n_beams))
    x, y = free_pose(world, rng, -4.0, 4.0)
    true = (x, y, 0.3)
    poses = [true]
    for dx, dy, dyaw in ((0.1, 0.0, 0.02), (-0.1, 0.05, -0.03), (0.0, -0.1, 0.05), (0.05, 0.1, -0.06)):
        if not world.occupied(x + dx, y + dy, margin=0.2):
            poses.append((x + dx, y + dy, 0.3 + dyaw))
    scans = [synth.ld06_scan(world, q[0], q[1], q[2], n_beams, rng) for q in poses]
    st = endpoint_map(p, poses, scans, amin, inc)
    ranges = synth.ld06_scan(world, true[0], true[1], true[2], n_beams, rng)
    prior = (true[0] + offset[0], true[1] + offset[1], true[2] + offset[2])
    return p, st, ranges, amin, inc, true, prior


def yaw_error(a: float, b: float) -> float:
    return abs(math.remainder(a - b, 2.0 * math.pi))


def drive(n_steps=12, seed=5, n_beams=450, bias=(0.012, -0.008, 0.004), size=400):
    """A robot driving a gentle arc through a synth room with a constant
    per-step odometry bias.  Returns (params, amin, inc, true poses, odometry
    poses, scans): odom[t] = true[t] + t * bias in (x, y, yaw); step 0 agrees."""
    p = cases.make_params(size, size, 0.05)
    half = size * 0.05 / 2.0
    world = synth.make_world(seed, -half, -half, half, half)
    rng = np.random.Generator(np.random.PCG64(seed + 200))
    amin, inc = float(synth.LD06_ANGLE_MIN), float(synth.ld06_angle_increment(n_beams))
    while True:
        x, y = free_pose(world, rng, -0.3 * half, 0.3 * half, margin=0.6)
        yaw = rng.uniform(-math.pi, math.pi)
        true = []
        ok = True
        cx, cy, cyaw = x, y, yaw
        for _ in range(n_steps):
            true.append((cx, cy, cyaw))
            cyaw += 0.03
            cx += 0.12 * math.cos(cyaw)
            cy += 0.12 * math.sin(cyaw)
            ok = ok and not world.occupied(cx, cy, margin=0.3)
        if ok:
            break
    odom = [(q[0] + t * bias[0], q[1] + t * bias[1], q[2] + t * bias[2]) for t, q in enumerate(true)]
    scans = [synth.ld06_scan(world, q[0], q[1], q[2], n_beams, rng) for q in true]
    return p, amin, inc, true, odom, scans


def run_drive(make_node, odom, scans, amin, inc):
    """Feed the drive's scans (one per second) to the node make_node(pose
    provider) returns.  Returns (node, [(step, integrated pose)])."""
    from dm.ros_node import Header, LaserScan

    cur = [0]
    node = make_node(lambda msg: odom[cur[0]])
    integrated = []
    for t in range(len(odom)):
        cur[0] = t
        before = node.scans_integrated
        node.scan_cb(LaserScan(header=Header(stamp=float(t), frame_id="base_laser"), angle_min=amin,
                               angle_increment=inc, ranges=scans[t]))
        if node.scans_integrated > before:
            integrated.append((t, node.last_integrated_pose))
    return node, integrated

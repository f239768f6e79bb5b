"""GPU, end to end: two MappingNodes map overlapping parts of one dm.synth
room, the second in a map frame shifted and turned against the first.
align_peer finds the second's frame from one of its scans (dm_match_global in
the first's map), peer_map_cb folds the second's /map into the first's on the
device, and the result equals dm/fuse.py applied with that transform."""
import functools

import numpy as np
import pytest

import match_cases
import match_global_cases as mgc
from dm import fuse
from dm.ros_node import Header, LaserScan, MappingNode, se2_compose, se2_inverse

pytestmark = pytest.mark.gpu

FRAME = (0.8, -0.5, 0.4)  # the second node's map frame in the first's: p_first = FRAME o p_second
RANGE = 12.0              # max_laser_range (slam_config.yaml:27)
SPLIT = (14, 10)          # the first node takes scans [0, 14), the second [10, 24)
YAW_STEP = 0.00349        # the matcher's fine angle step (fine_search_angle_offset)


@functools.lru_cache(maxsize=None)
def scenario():
    """A 24-step drive through a 400^2 room (no odometry bias); the second
    robot's poses in its own frame are FRAME^-1 o true."""
    p, amin, inc, true, _, scans = match_cases.drive(n_steps=24, bias=(0.0, 0.0, 0.0))
    second = [se2_compose(se2_inverse(FRAME), q) for q in true]
    return p, amin, inc, true, second, scans


def _scan(t, amin, inc, ranges):
    return LaserScan(header=Header(stamp=float(t), frame_id="base_laser"), angle_min=amin, angle_increment=inc,
                     ranges=ranges)


def build_nodes(make_mapper):
    """The two nodes after their drives (make_mapper() -> a stand-in mapper; None: the device's)."""
    p, amin, inc, true, second, scans = scenario()
    kw = dict(dm_width=400, dm_height=400, resolution=0.05, max_laser_range=RANGE, gate=False, **mgc.NODE_SLAM)
    poses = {}
    mk = (lambda: None) if make_mapper is None else make_mapper
    a = MappingNode(pose_provider=lambda msg: poses["a"], mapper=mk(), **kw)
    b = MappingNode(pose_provider=lambda msg: poses["b"], mapper=mk(), **kw)
    for t in range(SPLIT[0]):
        poses["a"] = true[t]
        a.scan_cb(_scan(t, amin, inc, scans[t]))
    for t in range(SPLIT[1], len(true)):
        poses["b"] = second[t]
        b.scan_cb(_scan(t, amin, inc, scans[t]))
    return a, b


def test_two_nodes_align_and_fuse():
    p, amin, inc, true, second, scans = scenario()
    a, b = build_nodes(None)
    try:
        assert a.scans_integrated == SPLIT[0] and b.scans_integrated == len(true) - SPLIT[1]
        res = float(a.params.resolution)
        # a peer map before any transform is known is dropped
        a.peer_map_cb(b.occupancy_grid())
        assert a.peer_maps_dropped == 1 and a.peer_transform is None
        # the second robot's first scan, taken at second[t] in its frame, found in the first's map
        t = SPLIT[1]
        assert a.align_peer(_scan(t, amin, inc, scans[t]), second[t]) is True
        T = a.peer_transform
        at = se2_compose(T, second[t])  # where the transform puts the peer's pose: the matched pose
        print(f"transform {T} (frame {FRAME}); peer pose lands at {at}, true {true[t]}")
        assert abs(at[0] - true[t][0]) <= res and abs(at[1] - true[t][1]) <= res
        assert match_cases.yaw_error(at[2], true[t][2]) <= YAW_STEP
        assert match_cases.yaw_error(T[2], FRAME[2]) <= YAW_STEP
        assert abs(T[0] - FRAME[0]) <= res and abs(T[1] - FRAME[1]) <= res
        # the peer's /map folded in: equal to the restatement with that transform, mode fill
        L0, st0 = a.mapper.logodds(), a.mapper.state()
        msg = b.occupancy_grid()
        stats = a.peer_map_cb(msg)
        src = np.asarray(msg.data, np.int8)
        exp_L, exp_st, exp_stats = fuse.fuse_map(L0, a.params, src, fuse.geom_of(b.params), T, "fill",
                                                 src_is_state=True)
        print(f"fused: {stats}; known before {(st0 != -1).sum()}, after {(exp_st != -1).sum()}")
        assert stats == exp_stats and stats["contributing"] > 0 and stats["changed"] > 0
        L1, st1 = a.mapper.logodds(), a.mapper.state()
        assert np.array_equal(L1.view(np.uint32), exp_L.view(np.uint32)) and np.array_equal(st1, exp_st)
        assert (st1 != -1).sum() > (st0 != -1).sum()
        assert np.array_equal(L1[L0 != 0].view(np.uint32), L0[L0 != 0].view(np.uint32))  # fill keeps what was known
        # the peer republishes the same map: nothing changes
        again = a.peer_map_cb(msg)
        assert again == {"covered": stats["covered"], "contributing": 0, "changed": 0}
        assert np.array_equal(a.mapper.logodds().view(np.uint32), L1.view(np.uint32))
        assert np.array_equal(a.mapper.state(), st1) and a.peer_maps_fused == 2
    finally:
        a.destroy_node()
        b.destroy_node()

"""CPU: the node's scan-matching switch (dm_scan_matching) on an oracle-backed
stand-in mapper whose match_scan is the host restatement dm.match."""
import math

import numpy as np

import match_cases
from dm import match
from dm.ros_node import Header, LaserScan, MappingNode, SlamParams, se2_compose, se2_inverse
from oracle_mapper import OracleMapper


class MatchingOracleMapper(OracleMapper):
    """OracleMapper plus OccupancyMapper.match_scan, computed by dm.match on
    the oracle's state."""

    def __init__(self, params, **kw):
        super().__init__(params, **kw)
        self.match_calls = 0

    def match_scan(self, scan, pose, slam=None):
        self.match_calls += 1
        return match.two_stage(self.state(), self.params, np.asarray(scan.ranges, np.float32),
                               np.float32(scan.angle_min), np.float32(scan.angle_increment), pose, slam)


def make_node(p, mapper, **kw):
    def build(pose_provider):
        return MappingNode(dm_width=int(p.width), dm_height=int(p.height), resolution=float(p.resolution),
                           pose_provider=pose_provider, mapper=mapper, **kw)
    return build


def test_matcher_settings_come_from_the_yaml_names():
    s = SlamParams.from_dict({"use_scan_matching": True, "correlation_search_space_dimension": 0.3,
                              "coarse_angle_resolution": 0.02, "link_match_minimum_response_fine": 0.4,
                              "dm_scan_matching": True, "loop_search_maximum_distance": 3.0})
    assert (s.correlation_search_space_dimension, s.coarse_angle_resolution) == (0.3, 0.02)
    assert s.link_match_minimum_response_fine == 0.4 and s.dm_scan_matching is True
    d = SlamParams()
    assert (d.use_scan_matching, d.dm_scan_matching) == (True, False)
    assert (d.correlation_search_space_dimension, d.correlation_search_space_resolution,
            d.correlation_search_space_smear_deviation) == (0.5, 0.01, 0.1)
    assert (d.coarse_search_angle_offset, d.coarse_angle_resolution, d.fine_search_angle_offset,
            d.link_match_minimum_response_fine) == (0.349, 0.0349, 0.00349, 0.1)
    sp = match.search_params(s, 0.05)
    assert sp["coarse"]["half"] == 7 and len(sp["coarse"]["yaw_offsets"]) == 2 * 17 + 1


def test_se2_helpers():
    a, b = (1.0, -2.0, 0.7), (0.3, 0.4, -1.9)
    c = se2_compose(a, b)
    back = se2_compose(se2_inverse(a), c)
    assert max(abs(u - v) for u, v in zip(back, b)) < 1e-12
    assert se2_compose((0.0, 0.0, 0.0), b) == b  # the identity correction changes no bit


def test_sharded_map_refuses_the_switch():
    import pytest

    with pytest.raises(ValueError, match="dm_scan_matching"):
        MappingNode(dm_width=128, dm_height=256, dm_devices="0,0", dm_scan_matching=True)


def test_switch_off_changes_nothing(oracle_lib):
    p, amin, inc, true, odom, scans = match_cases.drive()
    plain = OracleMapper(p)
    node0, int0 = match_cases.run_drive(make_node(p, plain), odom, scans, amin, inc)
    standin = MatchingOracleMapper(p)
    node1, int1 = match_cases.run_drive(make_node(p, standin), odom, scans, amin, inc)
    assert standin.match_calls == 0 and not node1.matching
    assert int0 == int1 and len(int1) >= 5
    assert [q for _, q in int1] == [tuple(odom[t]) for t, _ in int1]  # integrated at the provider's pose
    np.testing.assert_array_equal(plain.state(), standin.state())
    assert node1.map_to_odom == (0.0, 0.0, 0.0) and (node1.scans_matched, node1.scans_rejected) == (0, 0)
    # the reference's own switch off keeps it off too
    node2, _ = match_cases.run_drive(make_node(p, MatchingOracleMapper(p), dm_scan_matching=True,
                                               use_scan_matching=False), odom, scans, amin, inc)
    assert not node2.matching and node2.mapper.match_calls == 0


def test_switch_on_corrects_biased_odometry(oracle_lib):
    """A constant per-step odometry bias: the correction becomes non-identity
    and the last integrated scan's pose is nearer the truth than its odometry
    pose, in translation and in yaw."""
    p, amin, inc, true, odom, scans = match_cases.drive()
    mapper = MatchingOracleMapper(p)
    node, integrated = match_cases.run_drive(make_node(p, mapper, dm_scan_matching=True), odom, scans, amin, inc)
    assert node.matching and mapper.match_calls == len(integrated) - 1  # every accepted scan but the first
    assert node.scans_matched + node.scans_rejected == mapper.match_calls and node.scans_matched >= 3
    assert node.map_to_odom != (0.0, 0.0, 0.0)
    t, pose = integrated[-1]
    assert t >= 8
    e_odom = math.hypot(odom[t][0] - true[t][0], odom[t][1] - true[t][1])
    e_corr = math.hypot(pose[0] - true[t][0], pose[1] - true[t][1])
    y_odom, y_corr = match_cases.yaw_error(odom[t][2], true[t][2]), match_cases.yaw_error(pose[2], true[t][2])
    print(f"step {t}: translation error {e_odom:.4f} -> {e_corr:.4f} m, yaw error {y_odom:.4f} -> {y_corr:.4f} rad, "
          f"matched {node.scans_matched}, rejected {node.scans_rejected}")
    assert e_corr < e_odom and y_corr < y_odom
    # map_to_odom is matched o odom^-1: it carries the odometry pose to the integrated one
    back = se2_compose(node.map_to_odom, odom[t])
    assert max(abs(u - v) for u, v in zip(back, pose)) < 1e-9
    assert node.latest_pose == pose


def test_rejected_matches_are_integrated_at_the_prior(oracle_lib):
    p, amin, inc, true, odom, scans = match_cases.drive(n_steps=7)
    # (a) against a still-empty map: the first scan has no return at all
    mapper = MatchingOracleMapper(p)
    node = make_node(p, mapper, dm_scan_matching=True, gate=False)(lambda msg: odom[int(msg.header.stamp)])
    nothing = np.full_like(scans[0], np.nan)
    node.scan_cb(LaserScan(header=Header(stamp=0.0), angle_min=amin, angle_increment=inc, ranges=nothing))
    assert node.scans_integrated == 1 and mapper.match_calls == 0 and (mapper.state() == 100).sum() == 0
    node.scan_cb(LaserScan(header=Header(stamp=1.0), angle_min=amin, angle_increment=inc, ranges=scans[1]))
    assert mapper.match_calls == 1 and node.last_match["response"] == 0.0 and node.last_match["n_used"] > 0
    assert (node.scans_matched, node.scans_rejected, node.scans_integrated) == (0, 1, 2)
    assert node.map_to_odom == (0.0, 0.0, 0.0) and node.last_integrated_pose == tuple(odom[1])
    assert (mapper.state() == 100).sum() > 0
    # (b) a threshold no response reaches
    mapper = MatchingOracleMapper(p)
    node, integrated = match_cases.run_drive(make_node(p, mapper, dm_scan_matching=True, gate=False,
                                                       link_match_minimum_response_fine=1.5),
                                             odom, scans, amin, inc)
    assert (node.scans_matched, node.scans_rejected) == (0, len(odom) - 1) and mapper.match_calls == len(odom) - 1
    assert node.last_match["response"] > 0.1
    assert [q for _, q in integrated] == [tuple(o) for o in odom] and node.map_to_odom == (0.0, 0.0, 0.0)

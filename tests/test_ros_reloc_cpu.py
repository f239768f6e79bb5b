"""CPU: the node's relocalisation switches (dm_map_file, dm_relocalize) on an
oracle-backed stand-in mapper whose relocalize is the host restatement
dm.match.relocalize."""
import functools
import os
import tempfile

import numpy as np
import pytest

import match_cases
import match_global_cases as mgc
import oracle
from dm import match
from dm.ros_node import Header, LaserScan, MappingNode, se2_compose
from test_ros_match_cpu import MatchingOracleMapper, make_node


class RelocOracleMapper(MatchingOracleMapper):
    """MatchingOracleMapper plus OccupancyMapper.load (here: a .npy of the
    log-odds) and relocalize, computed by dm.match on the oracle's state."""

    def __init__(self, params, **kw):
        super().__init__(params, **kw)
        self.loads = 0
        self.relocalize_calls = 0

    def load(self, path):
        self.loads += 1
        self.om.set_logodds(np.load(path))

    def relocalize(self, scan, prior=None, slam=None):
        self.relocalize_calls += 1
        return match.relocalize(self.state(), self.params, np.asarray(scan.ranges, np.float32),
                                np.float32(scan.angle_min), np.float32(scan.angle_increment), prior, slam)


def saved_map_logodds(p, true, scans, amin, inc):
    """The map the node starts on: the drive's first three scans at their true poses."""
    om = oracle.OracleMap(p)
    for q, r in list(zip(true, scans))[:3]:
        om.integrate(np.asarray([q], np.float64), np.asarray(r, np.float32)[None, :], np.float32(amin), np.float32(inc))
    return om.L.copy()


def run_reloc(mapper, map_file, p, amin, inc, odom, scans):
    """The node on a loaded map: a scan without a return, then the drive."""
    node = make_node(p, mapper, dm_scan_matching=True, dm_relocalize=True, dm_map_file=map_file, gate=False,
                     **mgc.NODE_SLAM)(lambda msg: odom[int(msg.header.stamp)])
    log = []
    nothing = np.full_like(np.asarray(scans[0], np.float32), np.nan)
    for t, r in [(0, nothing)] + list(enumerate(scans)):
        node.scan_cb(LaserScan(header=Header(stamp=float(t), frame_id="base_laser"), angle_min=amin,
                               angle_increment=inc, ranges=r))
        log.append((node.scans_integrated, node.relocalize_rejected, node.relocalizing, node.map_to_odom,
                    node.last_integrated_pose))
    return node, log


@functools.lru_cache(maxsize=None)
def standin_run():
    """The stand-in's run, shared with the GPU test; oracle.build() must have run."""
    p, amin, inc, true, odom, scans = mgc.node_case()
    L = saved_map_logodds(p, true, scans, amin, inc)
    path = os.path.join(tempfile.mkdtemp(prefix="dm_reloc_"), "map.npy")
    np.save(path, L)
    mapper = RelocOracleMapper(p)
    node, log = run_reloc(mapper, path, p, amin, inc, odom, scans)
    return dict(p=p, amin=amin, inc=inc, true=true, odom=odom, scans=scans, L=L, mapper=mapper, node=node, log=log)


def test_nothing_is_integrated_before_the_accepted_relocalisation(oracle_lib):
    r = standin_run()
    node, log, mapper, p = r["node"], r["log"], r["mapper"], r["p"]
    assert mapper.loads == 1 and node.map_loaded
    # the scan without a return: rejected, nothing integrated, still relocalising
    assert log[0] == (0, 1, True, (0.0, 0.0, 0.0), None)
    # the drive's first scan is found in the map and integrated at the pose found
    n_int, n_rej, relocalizing, m2o, pose = log[1]
    assert (n_int, n_rej, relocalizing) == (1, 1, False) and mapper.relocalize_calls == 2
    res = float(p.resolution)
    print(f"map_to_odom {m2o} (offset {mgc.FAR}), pose {pose}, true {r['true'][0]}")
    assert abs(pose[0] - r["true"][0][0]) <= res and abs(pose[1] - r["true"][0][1]) <= res
    assert match_cases.yaw_error(pose[2], r["true"][0][2]) <= 0.00349
    # map_to_odom carries the odometry frame's offset, to within a cell at the robot
    back = se2_compose(m2o, r["odom"][0])
    assert max(abs(back[0] - pose[0]), abs(back[1] - pose[1]), abs(back[2] - pose[2])) < 1e-9
    assert abs(m2o[0] - mgc.FAR[0]) <= res and abs(m2o[1] - mgc.FAR[1]) <= res and abs(m2o[2] - mgc.FAR[2]) <= 0.00349
    # then the node goes on as the matching node does
    assert [e[0] for e in log[1:]] == list(range(1, len(r["scans"]) + 1))
    assert mapper.match_calls >= len(r["scans"]) - 1 and node.scans_matched >= 1
    assert node.relocalize_rejected == 1 and mapper.relocalize_calls == 2
    last = node.last_relocalize
    assert last["accepted"] and last["global_response"] >= 0.35 and last["response"] >= 0.45
    t = len(r["scans"]) - 1
    final = log[-1][4]
    assert abs(final[0] - r["true"][t][0]) <= res and abs(final[1] - r["true"][t][1]) <= res


def test_a_rejected_relocalisation_leaves_the_map_alone(oracle_lib):
    r = standin_run()
    p = r["p"]
    path = os.path.join(tempfile.mkdtemp(prefix="dm_reloc_"), "map.npy")
    np.save(path, r["L"])
    mapper = RelocOracleMapper(p)
    slam = dict(mgc.NODE_SLAM, loop_match_minimum_response_fine=1.5)  # a threshold no response reaches
    node = make_node(p, mapper, dm_scan_matching=True, dm_relocalize=True, dm_map_file=path, gate=False,
                     **slam)(lambda msg: r["odom"][0])
    st = mapper.state()
    node.scan_cb(LaserScan(header=Header(stamp=0.0), angle_min=r["amin"], angle_increment=r["inc"],
                           ranges=r["scans"][0]))
    assert (node.scans_integrated, node.relocalize_rejected, node.relocalizing) == (0, 1, True)
    assert not node.last_relocalize["accepted"] and node.last_relocalize["global_response"] >= 0.35
    assert node.map_to_odom == (0.0, 0.0, 0.0) and node.last_integrated_pose is None
    np.testing.assert_array_equal(mapper.state(), st)


def test_switches_off_change_nothing(oracle_lib):
    p, amin, inc, true, odom, scans = match_cases.drive(n_steps=6)
    kw = dict(dm_scan_matching=True)
    base = MatchingOracleMapper(p)
    node0, int0 = match_cases.run_drive(make_node(p, base, **kw), odom, scans, amin, inc)
    # the defaults spelled out, and dm_relocalize without a map to load: as before
    for extra in (dict(dm_map_file="", dm_relocalize=False), dict(dm_relocalize=True)):
        mapper = RelocOracleMapper(p)
        node1, int1 = match_cases.run_drive(make_node(p, mapper, **kw, **extra), odom, scans, amin, inc)
        assert int1 == int0 and node1.map_to_odom == node0.map_to_odom
        assert (node1.scans_matched, node1.scans_rejected) == (node0.scans_matched, node0.scans_rejected)
        assert (mapper.loads, mapper.relocalize_calls, mapper.match_calls) == (0, 0, base.match_calls)
        assert not node1.relocalizing and not node1.map_loaded and node1.last_relocalize is None
        np.testing.assert_array_equal(mapper.state(), base.state())
    # and without matching the node is the plain one
    plain = RelocOracleMapper(p)
    node2, _ = match_cases.run_drive(make_node(p, plain), odom, scans, amin, inc)
    assert not node2.matching and not node2.relocalizing and plain.match_calls == 0


def test_the_switch_needs_matching_and_one_handle():
    with pytest.raises(ValueError, match="dm_relocalize needs dm_scan_matching"):
        MappingNode(dm_width=128, dm_height=128, dm_relocalize=True, mapper=object())
    with pytest.raises(ValueError, match="dm_scan_matching needs the whole map in one handle"):
        MappingNode(dm_width=128, dm_height=256, dm_devices="0,0", dm_scan_matching=True, dm_relocalize=True)
    with pytest.raises(ValueError, match="dm_scan_matching needs the whole map in one handle"):
        MappingNode(dm_width=128, dm_height=256, dm_devices="0,0", dm_relocalize=True)

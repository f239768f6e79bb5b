"""GPU: the node's scan-matching drive (tests/test_ros_match_cpu.py) with the
real OccupancyMapper on a 400^2 map: the device matcher must lead the node to
exactly the poses and the correction the host stand-in run arrives at."""
import numpy as np
import pytest

import dm
import match_cases
from test_ros_match_cpu import MatchingOracleMapper, make_node

pytestmark = pytest.mark.gpu


def test_drive_equals_the_stand_in_run(oracle_lib):
    p, amin, inc, true, odom, scans = match_cases.drive(n_steps=9)
    kw = dict(dm_scan_matching=True, gate=False)
    standin = MatchingOracleMapper(p)
    node0, int0 = match_cases.run_drive(make_node(p, standin, **kw), odom, scans, amin, inc)
    mapper = dm.OccupancyMapper(p)
    try:
        node1, int1 = match_cases.run_drive(make_node(p, mapper, **kw), odom, scans, amin, inc)
        assert int1 == int0 and len(int1) == len(odom)
        assert node1.map_to_odom == node0.map_to_odom != (0.0, 0.0, 0.0)
        assert (node1.scans_matched, node1.scans_rejected) == (node0.scans_matched, node0.scans_rejected)
        assert node1.scans_matched >= 6
        assert node1.last_match["response"] == node0.last_match["response"]
        np.testing.assert_array_equal(mapper.state(), standin.state())
    finally:
        mapper.close()

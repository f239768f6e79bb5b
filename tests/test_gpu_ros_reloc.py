"""GPU: the relocalising node (tests/test_ros_reloc_cpu.py) with the real
OccupancyMapper on a dm_save checkpoint of the same map: dm_match_global and
the device matcher must lead the node to exactly the poses and the correction
the host stand-in run arrives at."""
import os

import numpy as np
import pytest

import dm
from test_ros_reloc_cpu import run_reloc, standin_run

pytestmark = pytest.mark.gpu


def test_relocalising_node_equals_the_stand_in_run(oracle_lib, tmp_path):
    r = standin_run()
    p = r["p"]
    path = os.path.join(str(tmp_path), "map.dm")
    with dm.OccupancyMapper(p) as saved:
        saved.set_logodds(r["L"])
        saved.save(path)
    mapper = dm.OccupancyMapper(p)
    try:
        node1, log1 = run_reloc(mapper, path, p, r["amin"], r["inc"], r["odom"], r["scans"])
        node0 = r["node"]
        assert log1 == r["log"]  # integrated counts, rejections, map_to_odom and the integrated poses, bit for bit
        assert node1.map_to_odom == node0.map_to_odom != (0.0, 0.0, 0.0)
        a, b = node1.last_relocalize, node0.last_relocalize
        assert a["accepted"] and a["pose"] == b["pose"]
        assert (a["global_response"], a["response"]) == (b["global_response"], b["response"])
        assert a["global"]["best"] == b["global"]["best"] and a["global"]["pose"] == b["global"]["pose"]
        stats = a["stats"]
        print(f"stats {stats}")
        assert stats[1] == stats[0] and 0 < stats[2] <= stats[0] // 100
        assert (node1.scans_matched, node1.scans_rejected) == (node0.scans_matched, node0.scans_rejected)
        np.testing.assert_array_equal(mapper.state(), r["mapper"].state())
    finally:
        mapper.close()

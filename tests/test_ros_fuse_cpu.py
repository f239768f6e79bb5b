"""CPU: the node's peer-map fusion (dm_peer_map_topic, peer_map_cb, align_peer)
on a stand-in mapper that records its calls."""
import array
import math

import numpy as np
import pytest

from dm import fuse
from dm.ros_node import (Header, LaserScan, MapMetaData, MappingNode, OccupancyGrid, Point, Pose, SlamParams,
                         parse_transform, quaternion_from_yaw, se2_compose, se2_inverse)


class RecordingMapper:
    """OccupancyMapper's fuse_state and relocalize, recorded; relocalize
    answers with the pose and verdict it was given."""

    def __init__(self, pose=(0.0, 0.0, 0.0), accepted=True):
        self.pose, self.accepted = pose, accepted
        self.fused = []
        self.relocalized = []

    def fuse_state(self, st, geom, transform, mode="add"):
        self.fused.append((np.array(st, np.int8), dict(geom), tuple(transform), mode))
        return {"covered": 12, "contributing": 5, "changed": 3}

    def relocalize(self, scan, prior=None, slam=None):
        self.relocalized.append((scan, prior, slam))
        return {"accepted": self.accepted, "pose": self.pose, "global_response": 0.5, "response": 0.6}


def _node(mapper, **kw):
    return MappingNode(dm_width=128, dm_height=128, mapper=mapper, **kw)


def _grid(w=6, h=4, res=0.1, origin=(1.5, -2.0), yaw=0.0):
    data = array.array("b", [(-1, 0, 100)[i % 3] for i in range(w * h)])
    info = MapMetaData(resolution=res, width=w, height=h,
                       origin=Pose(position=Point(origin[0], origin[1], 0.0), orientation=quaternion_from_yaw(yaw)))
    return OccupancyGrid(header=Header(frame_id="peer_map"), info=info, data=data)


def test_defaults_are_off_and_fill():
    d = SlamParams()
    assert (d.dm_peer_map_topic, d.dm_peer_map_mode, d.dm_peer_map_transform) == ("", "fill", "")
    s = SlamParams.from_dict({"dm_peer_map_topic": "/robot2/map", "dm_peer_map_mode": "add",
                              "dm_peer_map_transform": "1.5, -2, 0.25"})
    assert (s.dm_peer_map_topic, s.dm_peer_map_mode) == ("/robot2/map", "add")
    assert parse_transform(s.dm_peer_map_transform) == (1.5, -2.0, 0.25)
    with pytest.raises(ValueError, match="dm_peer_map_mode"):
        _node(RecordingMapper(), dm_peer_map_mode="max")


def test_transform_parsing():
    assert parse_transform("") is None and parse_transform("  ") is None
    assert parse_transform("0,0,0") == (0.0, 0.0, 0.0)
    assert parse_transform([1, 2, 3]) == (1.0, 2.0, 3.0)
    for bad in ("1,2", "1,2,3,4", "1,2,nan", "inf,0,0"):
        with pytest.raises(ValueError):
            parse_transform(bad)
    with pytest.raises(ValueError):
        parse_transform("a,b,c")
    assert _node(RecordingMapper(), dm_peer_map_transform="0.5,-1,0.1").peer_transform == (0.5, -1.0, 0.1)


def test_peer_map_is_dropped_without_a_transform():
    m = RecordingMapper()
    node = _node(m)
    assert node.peer_transform is None
    assert node.peer_map_cb(_grid()) is None
    assert node.peer_map_cb(_grid()) is None
    assert node.peer_maps_dropped == 2 and node.peer_maps_fused == 0 and m.fused == []


def test_peer_map_geometry_comes_from_the_message_and_the_mode_defaults_to_fill():
    m = RecordingMapper()
    node = _node(m, dm_peer_map_transform="0.5,-1,0.1")
    msg = _grid()
    stats = node.peer_map_cb(msg)
    assert stats == {"covered": 12, "contributing": 5, "changed": 3} == node.last_peer_fuse
    assert node.peer_maps_fused == 1 and node.peer_maps_dropped == 0
    st, geom, transform, mode = m.fused[0]
    assert mode == "fill"
    assert geom == {"width": 6, "height": 4, "resolution": 0.1, "origin_x": 1.5, "origin_y": -2.0}
    assert transform == (0.5, -1.0, 0.1)  # an unturned origin changes no bit of the transform
    assert st.dtype == np.int8 and st.tolist() == list(msg.data)
    node2 = _node(m, dm_peer_map_transform="0,0,0", dm_peer_map_mode="add")
    node2.peer_map_cb(msg)
    assert m.fused[1][3] == "add"


def test_a_turned_origin_is_composed_into_the_transform():
    m = RecordingMapper()
    T = (0.5, -1.0, 0.1)
    node = _node(m, dm_peer_map_transform="0.5,-1,0.1")
    yaw = 0.4
    node.peer_map_cb(_grid(origin=(1.5, -2.0), yaw=yaw))
    _, geom, transform, _ = m.fused[0]
    assert (geom["origin_x"], geom["origin_y"]) == (1.5, -2.0)
    # a point u of the unturned grid (geometry origin O) lies at O + R(yaw)(u - O) in the peer's frame
    for u in ((1.5, -2.0), (2.1, -1.6), (1.5, -1.7)):
        c, s = math.cos(yaw), math.sin(yaw)
        in_peer = (1.5 + c * (u[0] - 1.5) - s * (u[1] + 2.0), -2.0 + s * (u[0] - 1.5) + c * (u[1] + 2.0), 0.0)
        want = se2_compose(T, in_peer)
        got = se2_compose(transform, (u[0], u[1], 0.0))
        assert abs(got[0] - want[0]) < 1e-12 and abs(got[1] - want[1]) < 1e-12
    assert abs(transform[2] - (0.1 + yaw)) < 1e-12


def test_align_peer_accepts_and_rejects():
    scan = LaserScan(angle_increment=0.01, ranges=np.ones(8, np.float32))
    matched, peer_pose = (2.0, -1.0, 0.7), (0.4, 0.3, -0.2)
    m = RecordingMapper(pose=matched, accepted=True)
    node = _node(m)
    assert node.align_peer(scan, peer_pose) is True
    assert m.relocalized[0][0] is scan and m.relocalized[0][1] is None and m.relocalized[0][2] is node.slam
    assert node.peer_transform == fuse.peer_transform(matched, peer_pose) == se2_compose(matched, se2_inverse(peer_pose))
    back = se2_compose(node.peer_transform, peer_pose)  # the peer's pose lands on the matched pose
    assert max(abs(a - b) for a, b in zip(back, matched)) < 1e-12
    node.peer_map_cb(_grid())
    assert m.fused[0][2] == node.peer_transform and node.peer_maps_fused == 1
    # a rejected match leaves the transform as it was: none, or the configured one
    m2 = RecordingMapper(pose=matched, accepted=False)
    node2 = _node(m2)
    assert node2.align_peer(scan, peer_pose) is False
    assert node2.peer_transform is None and node2.peer_align_rejected == 1 and not node2.last_peer_align["accepted"]
    node2.peer_map_cb(_grid())
    assert node2.peer_maps_dropped == 1 and m2.fused == []
    node3 = _node(m2, dm_peer_map_transform="1,2,3")
    assert node3.align_peer(scan, peer_pose) is False and node3.peer_transform == (1.0, 2.0, 3.0)

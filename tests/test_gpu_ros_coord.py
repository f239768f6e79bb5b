"""GPU: the ROS 2 drop-in's coordinated goals (dm/ros_node.py,
dm_goal_coordinate): with one peer goal held, the goal on /goal_pose is the one
dm_assign_goals_coord returns, the host restatement's too, and /plan ends at
it."""
import pytest

import cases
from dm import gain
from dm.ros_node import LaserScan, MappingNode, Point, Pose, PoseArray

pytestmark = pytest.mark.gpu


def _drive(node, batches, inc):
    poses_by_scan = {}
    node.pose_provider = lambda m: poses_by_scan[id(m)]
    msgs = []
    for poses, ranges in batches:
        msg = LaserScan(angle_increment=inc, ranges=ranges[0])
        msgs.append(msg)  # keep the ids unique
        poses_by_scan[id(msg)] = tuple(poses[0])
        node.scan_cb(msg)
    node.publish_map(stamp=1.0)
    assert node.poll_frontiers(wait=True)


def test_coordinated_goal_and_plan_topics():
    p, batches, amin, inc = cases.world_case(7, 400, 400, 0.05, 1, 450, 12)
    node = MappingNode(dm_width=400, dm_height=400, clock=lambda: 0.0, gate=False, dm_explore=True,
                       dm_goal_min_size=4, dm_goal_coordinate=True, dm_goal_gain_radius_m=3.0, dm_goal_min_gain=10)
    try:
        _drive(node, batches, inc)
        st = node.mapper.state()
        cl = node.last_frontiers
        x, y, _ = batches[-1][0][0]
        a = (p.origin_x, p.origin_y, p.resolution)
        kw = dict(min_size=4, min_gain=10, distance_weight=1.0, min_distance=0.3, inflate_cells=2, snap_cells=5,
                  radius_cells=60)
        # no peer goal yet: the uncoordinated goal
        alone = gain.assign_goals_gain(st, cl, [(x, y)], *a, **kw)[0]
        assert alone is not None and len(node.goal_pub.messages) == 1 and node.last_gain == alone[3]
        goal = node.goal_pub.messages[-1]
        assert (goal.pose.position.x, goal.pose.position.y) == alone[1]
        # a peer holds that goal: the next choice discounts what it sees
        node.peer_goals_cb(PoseArray(poses=[Pose(position=Point(alone[1][0], alone[1][1], 0.0))]))
        node.publish_map(stamp=2.0)
        assert node.poll_frontiers(wait=True)
        exp = gain.assign_goals_coord(st, cl, [(x, y)], *a, held_xy=[alone[1]], **kw)[0]
        assert exp is not None and exp[0] != alone[0] and exp[3] >= 10
        assert node.mapper.assign_goals_coord([(x, y)], held_xy=[alone[1]], **kw)[0] == exp
        assert len(node.goal_pub.messages) == 2 and node.last_gain == exp[3]
        goal = node.goal_pub.messages[-1]
        assert (goal.pose.position.x, goal.pose.position.y) == exp[1]
        path = node.plan_pub.messages[-1]
        assert path.header.frame_id == "map" and len(path.poses) >= 2
        last = path.poses[-1].pose.position
        assert (last.x, last.y) == exp[1]
    finally:
        node.destroy_node()

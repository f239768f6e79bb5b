"""GPU: the ROS 2 drop-in's path-length goals (dm/ros_node.py,
dm_goal_path_distance): the goal on /goal_pose is the centre of a traversable
cell chosen by dm_assign_goals_path and /plan carries the path to it; with the
default settings the node publishes what it always did and nothing on /plan."""
import numpy as np
import pytest

import cases
from dm import plan
from dm.goals import select_goal
from dm.ros_node import LaserScan, MappingNode

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


def test_path_goal_and_plan_topics():
    p, batches, amin, inc = cases.world_case(7, 400, 400, 0.05, 1, 450, 12)
    node = MappingNode(dm_width=400, dm_height=400, clock=lambda: 0.0, gate=False, dm_explore=True,
                       dm_goal_min_size=4, dm_goal_path_distance=True)
    try:
        _drive(node, batches, inc)
        st = node.mapper.state()
        cl = node.last_frontiers
        x, y, _ = batches[-1][0][0]
        exp = plan.assign_goals_path(st, cl, [(x, y)], p.origin_x, p.origin_y, p.resolution, min_size=4,
                                     distance_weight=1.0, min_distance=0.3, inflate_cells=2, snap_cells=5)[0]
        assert exp is not None
        goal = node.goal_pub.messages[-1]
        assert (goal.pose.position.x, goal.pose.position.y) == exp[1]
        trav = plan.traversable(st, 2)
        assert trav.reshape(-1)[exp[2]]  # a cell the robot can stand on
        path = node.plan_pub.messages[-1]
        assert path.header.frame_id == "map" and len(path.poses) >= 2
        src = plan.cell_of(x, y, p.origin_x, p.origin_y, p.resolution, 400, 400)
        f = plan.field(st, [src], 2)
        cells = plan.path(f, plan.with_sources(trav, [src]), exp[2])
        xs = [p.origin_x + ((c % 400) + 0.5) * p.resolution for c in cells]
        ys = [p.origin_y + ((c // 400) + 0.5) * p.resolution for c in cells]
        assert [q.pose.position.x for q in path.poses] == xs
        assert [q.pose.position.y for q in path.poses] == ys
        last = path.poses[-1].pose.position
        assert (last.x, last.y) == exp[1]
    finally:
        node.destroy_node()


def test_default_settings_publish_what_they_did():
    p, batches, amin, inc = cases.world_case(7, 400, 400, 0.05, 1, 450, 12)
    node = MappingNode(dm_width=400, dm_height=400, clock=lambda: 0.0, gate=False, dm_explore=True,
                       dm_goal_min_size=4)
    try:
        _drive(node, batches, inc)
        x, y, _ = batches[-1][0][0]
        exp = select_goal(node.last_frontiers, (x, y), min_size=4, min_distance=0.3)
        assert exp is not None
        assert len(node.goal_pub.messages) == 1
        goal = node.goal_pub.messages[-1]
        assert (goal.pose.position.x, goal.pose.position.y) == exp[1]  # the centroid, as before
        assert node.plan_pub.messages == [] and node.last_plan is None
    finally:
        node.destroy_node()

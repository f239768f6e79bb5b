"""GPU: the ROS 2 drop-in's information-gain goals (dm/ros_node.py,
dm_goal_information_gain): the goal on /goal_pose is the one
dm_assign_goals_gain returns, the host restatement's too, and /plan carries
the path that ends in its cell."""
import pytest

import cases
from dm import gain, plan
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


def test_gain_goal_and_plan_topics():
    p, batches, amin, inc = cases.world_case(7, 400, 400, 0.05, 1, 450, 12)
    node = MappingNode(dm_width=400, dm_height=400, clock=lambda: 0.0, gate=False, dm_explore=True,
                       dm_goal_min_size=4, dm_goal_information_gain=True, dm_goal_gain_radius_m=3.0,
                       dm_goal_min_gain=10)
    try:
        _drive(node, batches, inc)
        st = node.mapper.state()
        cl = node.last_frontiers
        x, y, _ = batches[-1][0][0]
        kw = dict(min_size=4, min_gain=10, distance_weight=1.0, min_distance=0.3, inflate_cells=2, snap_cells=5,
                  radius_cells=60)
        exp = gain.assign_goals_gain(st, cl, [(x, y)], p.origin_x, p.origin_y, p.resolution, **kw)[0]
        assert exp is not None and exp[3] >= 10
        assert node.mapper.assign_goals_gain([(x, y)], **kw)[0] == exp
        assert len(node.goal_pub.messages) == 1 and node.last_gain == exp[3]
        goal = node.goal_pub.messages[-1]
        assert (goal.pose.position.x, goal.pose.position.y) == exp[1]
        path = node.plan_pub.messages[-1]
        assert path.header.frame_id == "map" and len(path.poses) >= 2
        trav = plan.traversable(st, 2)
        src = plan.cell_of(x, y, p.origin_x, p.origin_y, p.resolution, 400, 400)
        cells = plan.path(plan.field(st, [src], 2), plan.with_sources(trav, [src]), exp[2])
        assert [q.pose.position.x for q in path.poses] == [p.origin_x + ((c % 400) + 0.5) * p.resolution for c in cells]
        assert [q.pose.position.y for q in path.poses] == [p.origin_y + ((c // 400) + 0.5) * p.resolution for c in cells]
        last = path.poses[-1].pose.position
        assert (last.x, last.y) == exp[1]
    finally:
        node.destroy_node()

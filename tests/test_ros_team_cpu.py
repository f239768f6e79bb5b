"""CPU: the node's team switch (dm_team_poses_topic) on the oracle-backed
stand-in mapper of test_ros_gain_cpu.py, whose team call is the host
restatement dm.plan.assign_goals_team: unset, the node makes no team call and
publishes what it did; set, choose_team_goals passes the own pose first and
returns one pose per robot."""
import math

import cases
from dm import plan
from dm.ros_node import LaserScan, MappingNode, Point, Pose, PoseArray, SlamParams
from test_ros_gain_cpu import PlanningOracleMapper


class TeamOracleMapper(PlanningOracleMapper):
    """PlanningOracleMapper plus OccupancyMapper's assign_goals_team."""

    def assign_goals_team(self, robots_xy, **kw):
        self.calls.append(("team", dict(robots_xy=list(robots_xy), **kw)))
        return plan.assign_goals_team(self.state(), self._last, robots_xy, *self._args(), **kw)


def _node(world, **kw):
    p, batches, amin, inc = world
    mapper = TeamOracleMapper(p)
    k = [0]
    node = MappingNode(dm_width=int(p.width), dm_height=int(p.height), resolution=float(p.resolution),
                       pose_provider=lambda m: tuple(batches[k[0]][0][0]), clock=lambda: 0.0, mapper=mapper,
                       gate=False, dm_explore=True, dm_goal_min_size=2, **kw)
    for j in range(len(batches)):
        k[0] = j
        node.scan_cb(LaserScan(angle_min=amin, angle_increment=inc, ranges=batches[j][1][0]))
    return node, mapper


def _publish(node):
    node.publish_map(stamp=1.0)
    assert node.poll_frontiers(wait=True)


def test_team_setting_defaults_to_off():
    assert SlamParams().dm_team_poses_topic == ""
    assert SlamParams.from_dict({"dm_team_poses_topic": "/team_poses"}).dm_team_poses_topic == "/team_poses"


def test_topic_unset_makes_no_team_call(oracle_lib):
    world = cases.world_case(13, 160, 160, 0.05, 1, 180, 3)
    node, mapper = _node(world)
    node.team_poses_cb(PoseArray(poses=[Pose(position=Point(0.5, 0.5, 0.0))]))  # kept, but nothing asks for it
    _publish(node)
    assert mapper.calls == [] and node.team_goals_pub.messages == []
    assert node.choose_team_goals() is None
    assert len(node.goal_pub.messages) == 1  # /goal_pose as before


def test_topic_set_assigns_own_pose_first_and_one_goal_per_robot(oracle_lib):
    world = cases.world_case(13, 160, 160, 0.05, 1, 180, 3)
    p = world[0]
    node, mapper = _node(world, dm_team_poses_topic="/team_poses")
    x, y, _ = world[1][-1][0][0]
    mates = [(x + 0.4, y), (x, y + 0.4)]
    node.team_poses_cb(PoseArray(poses=[Pose(position=Point(mx, my, 0.0)) for mx, my in mates]))
    assert node.team_poses == mates
    _publish(node)
    assert [c[0] for c in mapper.calls] == ["team"]
    call = mapper.calls[0][1]
    assert call["robots_xy"] == [(x, y)] + mates  # own pose first
    assert {k: v for k, v in call.items() if k != "robots_xy"} == dict(
        min_size=2, min_gain=1, distance_weight=1.0, min_distance=0.3, inflate_cells=2, snap_cells=5, radius_cells=0)
    exp = plan.assign_goals_team(mapper.state(), node.last_frontiers, [(x, y)] + mates, p.origin_x, p.origin_y,
                                 p.resolution, min_size=2, distance_weight=1.0, min_distance=0.3, inflate_cells=2,
                                 snap_cells=5)
    assert len(node.team_goals_pub.messages) == 1
    msg = node.team_goals_pub.messages[0]
    assert len(msg.poses) == 3 and msg.header.frame_id == node.slam.map_frame
    assert any(e is not None for e in exp)
    for pose, e in zip(msg.poses, exp):
        if e is None:
            assert math.isnan(pose.position.x) and math.isnan(pose.position.y)
        else:
            assert (pose.position.x, pose.position.y) == e[1]
    taken = [e[0] for e in exp if e is not None]
    assert len(set(taken)) == len(taken)  # no cluster twice
    assert len(node.goal_pub.messages) == 1  # /goal_pose is still published
    # with the information-gain switch the team call scores by gain, with the node's radius
    node, mapper = _node(world, dm_team_poses_topic="/team_poses", dm_goal_information_gain=True,
                         dm_goal_gain_radius_m=2.0, dm_goal_min_gain=5)
    _publish(node)
    team = [c for c in mapper.calls if c[0] == "team"]
    assert len(team) == 1 and team[0][1]["radius_cells"] == 40 and team[0][1]["min_gain"] == 5
    assert team[0][1]["robots_xy"] == [(x, y)]  # no teammates heard yet: the own pose alone
    assert len(node.team_goals_pub.messages[0].poses) == 1

"""CPU: the node's information-gain switch (dm_goal_information_gain) on an
oracle-backed stand-in mapper whose planning and gain calls are the host
restatements dm.plan and dm.gain: the parameters reach the call, and with the
switch off the node does what it did."""
import numpy as np

import cases
from dm import gain, plan
from dm.ros_node import LaserScan, MappingNode, SlamParams
from oracle_mapper import OracleMapper


class PlanningOracleMapper(OracleMapper):
    """OracleMapper plus OccupancyMapper's assign_goals_path, assign_goals_gain
    and plan_path, computed on the oracle's state."""

    def __init__(self, params, **kw):
        super().__init__(params, **kw)
        self.calls = []
        self._field = None

    def _args(self):
        p = self.params
        return p.origin_x, p.origin_y, p.resolution

    def _keep_field(self, robots_xy, inflate_cells):
        p, st = self.params, self.state()
        src = plan.cell_of(robots_xy[-1][0], robots_xy[-1][1], *self._args(), int(p.width), int(p.height))
        trav = plan.traversable(st, inflate_cells)
        self._field = (plan.field(st, [src], inflate_cells, trav=trav), plan.with_sources(trav, [src]))

    def assign_goals_path(self, robots_xy, **kw):
        self.calls.append(("path", kw))
        self._keep_field(robots_xy, kw["inflate_cells"])
        return plan.assign_goals_path(self.state(), self._last, robots_xy, *self._args(), **kw)

    def assign_goals_gain(self, robots_xy, **kw):
        self.calls.append(("gain", kw))
        self._keep_field(robots_xy, kw["inflate_cells"])
        return gain.assign_goals_gain(self.state(), self._last, robots_xy, *self._args(), **kw)

    def plan_path(self, target_xy, snap_cells=5):
        p = self.params
        f, trav = self._field
        _, cell = plan.snap(f, plan.cell_of(target_xy[0], target_xy[1], *self._args(), int(p.width), int(p.height)),
                            snap_cells)
        return np.array(plan.path(f, trav, cell), np.int64)


def test_gain_settings():
    d = SlamParams()
    assert d.dm_goal_information_gain is False and d.dm_goal_min_gain == 1
    assert d.gain_radius_cells() == 240  # the map's range_max: ceil(12 / 0.05)
    assert SlamParams(max_laser_range=8.0).gain_radius_cells() == 160
    assert SlamParams(resolution=0.01).gain_radius_cells() == 511  # clamped to the C-ABI's limit
    assert SlamParams(dm_goal_gain_radius_m=0.0).gain_radius_cells() == 1
    s = SlamParams.from_dict({"dm_goal_information_gain": True, "dm_goal_gain_radius_m": 2.0, "dm_goal_min_gain": 25})
    assert s.dm_goal_information_gain is True and s.gain_radius_cells() == 40 and s.dm_goal_min_gain == 25
    assert s.dm_goal_path_distance is False  # implied by the node, not rewritten in the settings


def _drive(world, **kw):
    p, batches, amin, inc = world
    mapper = PlanningOracleMapper(p)
    k = [0]
    node = MappingNode(dm_width=int(p.width), dm_height=int(p.height), resolution=float(p.resolution),
                       pose_provider=lambda m: tuple(batches[k[0]][0][0]), clock=lambda: 0.0, mapper=mapper,
                       gate=False, dm_explore=True, dm_goal_min_size=2, **kw)
    for j in range(len(batches)):
        k[0] = j
        node.scan_cb(LaserScan(angle_min=amin, angle_increment=inc, ranges=batches[j][1][0]))
    node.publish_map(stamp=1.0)
    assert node.poll_frontiers(wait=True)
    return node, mapper


def test_switch_off_changes_nothing(oracle_lib):
    world = cases.world_case(13, 160, 160, 0.05, 1, 180, 3)
    node, mapper = _drive(world)
    assert mapper.calls == [] and node.last_gain is None and node.plan_pub.messages == []
    x, y, _ = world[1][-1][0][0]
    exp = mapper.assign_goals([(x, y)], min_size=2, distance_weight=1.0, min_distance=0.3)[0]
    assert exp is not None and len(node.goal_pub.messages) == 1
    goal = node.goal_pub.messages[0].pose.position
    assert (goal.x, goal.y) == exp[1]
    # the path-length switch alone takes the path-length call, as before
    node, mapper = _drive(world, dm_goal_path_distance=True)
    assert [c[0] for c in mapper.calls] == ["path"] and node.last_gain is None
    assert set(mapper.calls[0][1]) == {"min_size", "distance_weight", "min_distance", "inflate_cells", "snap_cells"}


def test_switch_on_publishes_the_gain_goal_and_its_plan(oracle_lib):
    world = cases.world_case(13, 160, 160, 0.05, 1, 180, 3)
    p = world[0]
    node, mapper = _drive(world, dm_goal_information_gain=True, dm_goal_gain_radius_m=2.0, dm_goal_min_gain=5)
    assert [c[0] for c in mapper.calls] == ["gain"]
    assert mapper.calls[0][1] == dict(min_size=2, min_gain=5, distance_weight=1.0, min_distance=0.3, inflate_cells=2,
                                      snap_cells=5, radius_cells=40)
    x, y, _ = world[1][-1][0][0]
    exp = gain.assign_goals_gain(mapper.state(), node.last_frontiers, [(x, y)], p.origin_x, p.origin_y, p.resolution,
                                 **mapper.calls[0][1])[0]
    assert exp is not None and exp[3] >= 5 and node.last_gain == exp[3]
    goal = node.goal_pub.messages[-1].pose.position
    assert (goal.x, goal.y) == exp[1]
    path = node.plan_pub.messages[-1]
    assert len(path.poses) >= 2
    last = path.poses[-1].pose.position
    assert (last.x, last.y) == exp[1]  # /plan ends in the goal's cell
    # both switches on: the gain call, once
    node, mapper = _drive(world, dm_goal_information_gain=True, dm_goal_path_distance=True,
                          dm_goal_gain_radius_m=2.0)
    assert [c[0] for c in mapper.calls] == ["gain"] and mapper.calls[0][1]["min_gain"] == 1

"""CPU: the node's coordination switch (dm_goal_coordinate) on an oracle-backed
stand-in mapper whose planning and gain calls are the host restatements dm.plan
and dm.gain: the peers' goals reach the call as held views and the published
goal is the host restatement's; with the switch off the node does what it did."""
import numpy as np

import cases
from dm import gain, plan
from dm.ros_node import LaserScan, MappingNode, Point, Pose, PoseArray
from oracle_mapper import OracleMapper


class CoordOracleMapper(OracleMapper):
    """OracleMapper plus OccupancyMapper's assign_goals_gain, assign_goals_coord
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

    def assign_goals_gain(self, robots_xy, **kw):
        self.calls.append(("gain", kw))
        self._keep_field(robots_xy, kw["inflate_cells"])
        return gain.assign_goals_gain(self.state(), self._last, robots_xy, *self._args(), **kw)

    def assign_goals_coord(self, robots_xy, **kw):
        self.calls.append(("coord", kw))
        self._keep_field(robots_xy, kw["inflate_cells"])
        return gain.assign_goals_coord(self.state(), self._last, robots_xy, *self._args(), **kw)

    def plan_path(self, target_xy, snap_cells=5):
        p = self.params
        f, trav = self._field
        _, cell = plan.snap(f, plan.cell_of(target_xy[0], target_xy[1], *self._args(), int(p.width), int(p.height)),
                            snap_cells)
        return np.array(plan.path(f, trav, cell), np.int64)


KW = dict(min_size=2, min_gain=5, distance_weight=1.0, min_distance=0.3, inflate_cells=2, snap_cells=5,
          radius_cells=40)


def _drive(world, peers=None, **kw):
    p, batches, amin, inc = world
    mapper = CoordOracleMapper(p)
    k = [0]
    node = MappingNode(dm_width=int(p.width), dm_height=int(p.height), resolution=float(p.resolution),
                       pose_provider=lambda m: tuple(batches[k[0]][0][0]), clock=lambda: 0.0, mapper=mapper,
                       gate=False, dm_explore=True, dm_goal_min_size=2, **kw)
    if peers is not None:
        node.peer_goals_cb(PoseArray(poses=[Pose(position=Point(x, y, 0.0)) for x, y in peers]))
    for j in range(len(batches)):
        k[0] = j
        node.scan_cb(LaserScan(angle_min=amin, angle_increment=inc, ranges=batches[j][1][0]))
    node.publish_map(stamp=1.0)
    assert node.poll_frontiers(wait=True)
    return node, mapper


def test_switch_off_is_the_old_node(oracle_lib):
    world = cases.world_case(13, 160, 160, 0.05, 1, 180, 3)
    peers = [(0.5, 0.5)]
    node, mapper = _drive(world, peers=peers)  # peers' goals are stored, and not used
    assert mapper.calls == [] and node.peer_goals == peers and len(node.goal_pub.messages) == 1
    node, mapper = _drive(world, peers=peers, dm_goal_information_gain=True, dm_goal_gain_radius_m=2.0,
                          dm_goal_min_gain=5)
    assert [c[0] for c in mapper.calls] == ["gain"] and mapper.calls[0][1] == KW


def test_switch_on_holds_the_peers_goals(oracle_lib):
    world = cases.world_case(13, 160, 160, 0.05, 1, 180, 3)
    p = world[0]
    a = (p.origin_x, p.origin_y, p.resolution)
    x, y, _ = world[1][-1][0][0]
    # no peers: the goal the gain switch gives
    node, mapper = _drive(world, dm_goal_coordinate=True, dm_goal_gain_radius_m=2.0, dm_goal_min_gain=5)
    assert [c[0] for c in mapper.calls] == ["coord"]
    assert mapper.calls[0][1] == dict(held_xy=[], **KW)
    st, cl = mapper.state(), node.last_frontiers
    alone = gain.assign_goals_gain(st, cl, [(x, y)], *a, **KW)[0]
    assert alone is not None and node.last_gain == alone[3]
    goal = node.goal_pub.messages[-1].pose.position
    assert (goal.x, goal.y) == alone[1]
    # a peer holds that very goal: what it sees is claimed, the robot goes elsewhere
    node, mapper = _drive(world, peers=[alone[1]], dm_goal_coordinate=True, dm_goal_gain_radius_m=2.0,
                          dm_goal_min_gain=5)
    assert [c[0] for c in mapper.calls] == ["coord"] and mapper.calls[0][1]["held_xy"] == [alone[1]]
    exp = gain.assign_goals_coord(st, cl, [(x, y)], *a, held_xy=[alone[1]], **KW)[0]
    assert exp is not None and exp[0] != alone[0] and 5 <= exp[3] == node.last_gain
    goal = node.goal_pub.messages[-1].pose.position
    assert (goal.x, goal.y) == exp[1]
    last = node.plan_pub.messages[-1].poses[-1].pose.position
    assert (last.x, last.y) == exp[1]  # /plan ends in the goal's cell
    # a later message replaces the peers' goals
    node.peer_goals_cb(PoseArray())
    assert node.peer_goals == []

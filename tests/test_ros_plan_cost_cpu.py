"""CPU: the node's clearance switch (dm_plan_clearance_m) on the oracle-backed
stand-in mapper of test_ros_gain_cpu.py, whose planning calls are the host
restatements in dm.plan: off, /plan is what it was; on, /goal_pose is
unchanged and /plan is the path over the penalty-weighted field."""
import numpy as np

import cases
from dm import plan
from dm.ros_node import LaserScan, MappingNode, SlamParams
from test_ros_gain_cpu import PlanningOracleMapper


class CostOracleMapper(PlanningOracleMapper):
    """PlanningOracleMapper plus OccupancyMapper's plan_field_cost; plan_path
    follows the kind of field held, as dm_plan_path does."""

    def __init__(self, params, **kw):
        super().__init__(params, **kw)
        self._cell_pen = None

    def _keep_field(self, robots_xy, inflate_cells):
        super()._keep_field(robots_xy, inflate_cells)
        self._cell_pen = None  # an assign_goals_* call leaves an unweighted field

    def plan_field_cost(self, sources_xy, inflate_cells, clear_cells, pen, max_cost=0):
        self.calls.append(("field_cost", dict(sources_xy=list(sources_xy), inflate_cells=inflate_cells,
                                              clear_cells=clear_cells, pen=np.array(pen))))
        p, st = self.params, self.state()
        srcs = [plan.cell_of(x, y, *self._args(), int(p.width), int(p.height)) for x, y in sources_xy]
        self._cell_pen = plan.penalty(st, clear_cells, pen)
        self._field = (plan.field_cost(st, srcs, inflate_cells, clear_cells, pen, max_cost),
                       plan.with_sources(plan.traversable(st, inflate_cells), srcs))

    def plan_path(self, target_xy, snap_cells=5):
        p = self.params
        f, trav = self._field
        _, cell = plan.snap(f, plan.cell_of(target_xy[0], target_xy[1], *self._args(), int(p.width), int(p.height)),
                            snap_cells)
        return np.array(plan.path(f, trav, cell, self._cell_pen), np.int64)


def _drive(world, **kw):
    p, batches, amin, inc = world
    mapper = CostOracleMapper(p)
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


def _xy(path):
    return [(ps.pose.position.x, ps.pose.position.y) for ps in path.poses]


def test_clearance_settings():
    d = SlamParams()
    assert d.dm_plan_clearance_m == 0.0 and d.dm_plan_cost_scaling == 10.0 and d.clearance_cells() == 0
    assert SlamParams(dm_plan_clearance_m=0.4).clearance_cells() == 8
    assert SlamParams(dm_plan_clearance_m=0.41).clearance_cells() == 9      # ceil
    assert SlamParams(dm_plan_clearance_m=0.001).clearance_cells() == 1
    assert SlamParams(dm_plan_clearance_m=5.0).clearance_cells() == 32      # clamped to the C-ABI's limit
    assert SlamParams(dm_plan_clearance_m=-1.0).clearance_cells() == 0
    s = SlamParams.from_dict({"dm_plan_clearance_m": 0.3, "dm_plan_cost_scaling": 3.0})
    assert s.clearance_cells() == 6 and s.dm_plan_cost_scaling == 3.0


def test_clearance_off_and_on(oracle_lib):
    world = cases.world_case(21, 160, 160, 0.05, 1, 180, 6)
    p = world[0]
    off, mapper_off = _drive(world, dm_goal_path_distance=True)
    assert [c[0] for c in mapper_off.calls] == ["path"]  # no weighted field: /plan as before
    st = mapper_off.state()
    x, y, _ = world[1][-1][0][0]
    src = plan.cell_of(x, y, p.origin_x, p.origin_y, p.resolution, 160, 160)
    goal = off.goal_pub.messages[-1].pose.position
    gcell = plan.cell_of(goal.x, goal.y, p.origin_x, p.origin_y, p.resolution, 160, 160)
    trav = plan.with_sources(plan.traversable(st, 2), [src])

    def centres(cells):
        cells = np.asarray(cells)
        return [(float(p.origin_x) + ((c % 160) + 0.5) * float(p.resolution),
                 float(p.origin_y) + ((c // 160) + 0.5) * float(p.resolution)) for c in cells]

    shortest = plan.path(plan.field(st, [src], 2), trav, gcell[1] * 160 + gcell[0])
    assert len(shortest) >= 2 and _xy(off.plan_pub.messages[-1]) == centres(shortest)

    on, mapper = _drive(world, dm_goal_path_distance=True, dm_plan_clearance_m=1.6, dm_plan_cost_scaling=1.0)
    assert [c[0] for c in mapper.calls] == ["path", "field_cost"]
    call = mapper.calls[1][1]
    assert call["sources_xy"] == [(x, y)] and call["inflate_cells"] == 2 and call["clear_cells"] == 32
    pen = plan.inflation_table(0.05, 32, 0.10, 1.0)
    np.testing.assert_array_equal(call["pen"], pen)
    g_on = on.goal_pub.messages[-1]
    g_off = off.goal_pub.messages[-1]
    assert (g_on.pose.position.x, g_on.pose.position.y) == (goal.x, goal.y)  # /goal_pose is unchanged
    assert g_on.pose.orientation == g_off.pose.orientation
    cp = plan.penalty(st, 32, pen)
    weighted = plan.path(plan.field_cost(st, [src], 2, 32, pen), trav, gcell[1] * 160 + gcell[0], cp)
    got = _xy(on.plan_pub.messages[-1])
    assert got == centres(weighted) and got[-1] == (goal.x, goal.y)
    assert weighted != shortest  # the world's walls are near enough to matter
    d2 = plan.clearance(st, 32).reshape(-1)
    assert d2[weighted].astype(int).sum() / len(weighted) > d2[shortest].astype(int).sum() / len(shortest)

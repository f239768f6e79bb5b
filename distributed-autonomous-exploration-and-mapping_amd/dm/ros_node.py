"""ROS 2 drop-in for the mapping stage.

The reference gets its ``/map`` from slam_toolbox (server/thymio_project/
launch/pc_server.launch.py:12-19, parameters server/thymio_project/config/
slam_config.yaml) and consumes it in ``ThymioBrain.map_cb``
(server/thymio_project/thymio_project/main.py:46,80-81) and ``get_map_image``
(main.py:241-279).  ``MappingNode`` keeps those topics, message types and
callback signatures:

* subscribes ``/scan`` (``sensor_msgs/LaserScan``; ``scan_cb(self, msg)`` as
  main.py:77-78 — every scan is cached as ``latest_scan``) and looks up the
  laser pose ``map -> base_laser`` through a pose provider (tf2 in ROS; any
  callable in tests);
* gates scans the way the stage it replaces does (``ScanGate``: slam_toolbox's
  ``shouldProcessScan`` front gate, then Karto's ``HasMovedEnough``;
  slam_config.yaml:23,28,37-38) and integrates the accepted ones with libdm on
  the GPU (``dm_integrate``);
* on a timer of ``map_update_interval`` seconds (slam_config.yaml:25) —
  like slam_toolbox's map-publishing loop, whether or not scans were accepted
  in between, so a robot that stopped moving still republishes and a late
  subscriber gets a map — publishes ``/map`` as ``nav_msgs/OccupancyGrid``
  (frame ``map_frame``, ``header.stamp`` and ``info.map_load_time`` = the
  tick's time, resolution and origin from the grid, int8 -1/0/100 row-major,
  ``data`` handed over as an ``array('b')`` built from the device copy's bytes
  — no per-cell Python objects) and starts a frontier pass on the GPU
  (``dm_frontiers_begin``).  The pass is collected without blocking the
  callback thread (``dm_frontiers_poll`` from the scan / timer callbacks) and
  then published: the clusters on ``/frontiers`` (``geometry_msgs/PoseArray``
  of centroids) and, with exploration enabled, the chosen frontier goal on
  ``/goal_pose`` (``geometry_msgs/PoseStamped``, the topic Nav2's navigator
  and RViz's "2D Goal Pose" use) — the map-based replacement of the reactive
  IR/LiDAR policy (main.py:123-188) that the report lists as future work
  (report.pdf p.5 §VI-2);
* with ``dm_scan_matching`` (default off), takes the pose provider's pose as the
  odometry pose (``odom -> base_laser``) and corrects every accepted scan
  against the map with the device's correlative matcher (``dm_match_scans``;
  slam_toolbox's, slam_config.yaml:35,50-53,64-66) before integrating it; the
  correction is kept as ``map_to_odom`` and, under ROS, broadcast as
  ``map -> odom``: the part of the TF chain slam_toolbox published;
* with ``dm_map_file`` loads a ``dm_save`` checkpoint at start, and with
  ``dm_relocalize`` (default off; needs ``dm_scan_matching``) integrates no
  scan into it until one has been found in the map (``dm_match_global`` over
  the whole map, then the matcher; slam_toolbox's localization mode,
  slam_config.yaml:20, 47-48, 56-58); the pose found becomes ``map_to_odom``;
* with ``dm_goal_coordinate`` (default off), subscribes ``dm_peer_goals_topic``
  (``geometry_msgs/PoseArray``: the goals the other robots hold) and scores its
  own goal by what it would see that those goals do not
  (``dm_assign_goals_coord``);
* with ``dm_team_poses_topic`` set (default off), subscribes the teammates'
  poses (``geometry_msgs/PoseArray``) and publishes on ``/team_goals`` one goal
  per robot, own pose first, from the global-greedy assignment over all of them
  (``dm_assign_goals_team``);
* with ``dm_peer_map_topic`` set (default off), subscribes a peer's
  ``nav_msgs/OccupancyGrid`` in the peer's own map frame and folds it into this
  map on the device (``dm_fuse_state``; the merge step of a multi-robot stack,
  multirobot_map_merge) under the frame transform given as
  ``dm_peer_map_transform`` or found by ``align_peer`` (a peer's scan
  relocalised in this map, ``dm_match_global``);
* with ``dm_devices`` naming several GPUs, the map is one sharded handle
  (``dm_create_sharded``: row bands over those devices, the exchange inside
  libdm) behind the same calls.

All parameters come from the slam_toolbox parameter file the reference
launches (``SlamParams.from_yaml``), plus the fixed grid size this build needs
(slam_toolbox grows its map from the scans' bounding box; a device-resident
grid is allocated once).  Without rclpy (this container and the GPU box) the
same class runs on duck-typed messages: tests drive ``scan_cb`` directly and
read what was "published" from the publisher stubs.
"""
from __future__ import annotations

import array
import io
import math
import time
from dataclasses import dataclass, field, fields

import numpy as np

from .grid import OccupancyMapper, default_params

try:  # pragma: no cover - ROS is absent in CI and on the GPU box
    import rclpy  # noqa: F401
    from nav_msgs.msg import OccupancyGrid as _RosOccupancyGrid
    HAVE_ROS = True
except Exception:  # ModuleNotFoundError or a broken ROS env
    HAVE_ROS = False


# -- duck-typed message stand-ins (same field names as the ROS messages) -------
@dataclass
class Header:
    stamp: float = 0.0
    frame_id: str = "map"


@dataclass
class Point:
    x: float = 0.0
    y: float = 0.0
    z: float = 0.0


@dataclass
class Quaternion:
    x: float = 0.0
    y: float = 0.0
    z: float = 0.0
    w: float = 1.0


@dataclass
class Pose:
    position: Point = field(default_factory=Point)
    orientation: Quaternion = field(default_factory=Quaternion)


@dataclass
class PoseStamped:
    header: Header = field(default_factory=Header)
    pose: Pose = field(default_factory=Pose)


@dataclass
class Path:
    """nav_msgs/Path: the poses of a plan, start first."""
    header: Header = field(default_factory=Header)
    poses: list = field(default_factory=list)


@dataclass
class PoseArray:
    """geometry_msgs/PoseArray: the goals the peers hold (dm_peer_goals_topic)."""
    header: Header = field(default_factory=Header)
    poses: list = field(default_factory=list)


@dataclass
class MapMetaData:
    map_load_time: float = 0.0
    resolution: float = 0.05
    width: int = 0
    height: int = 0
    origin: Pose = field(default_factory=Pose)


@dataclass
class OccupancyGrid:
    header: Header = field(default_factory=Header)
    info: MapMetaData = field(default_factory=MapMetaData)
    data: array.array = field(default_factory=lambda: array.array("b"))


@dataclass
class LaserScan:
    header: Header = field(default_factory=lambda: Header(frame_id="base_laser"))
    angle_min: float = 0.0
    angle_max: float = 6.2831855
    angle_increment: float = 0.0
    time_increment: float = 0.0
    scan_time: float = 0.1
    range_min: float = 0.02
    range_max: float = 25.0
    ranges: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float32))
    intensities: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float32))


@dataclass
class FrontierCluster:
    label: int
    size: int
    x: float
    y: float


class ListPublisher:
    """Publisher stub: keeps what was published."""

    def __init__(self, topic: str):
        self.topic = topic
        self.messages: list = []

    def publish(self, msg):
        self.messages.append(msg)


def yaw_from_quaternion(q) -> float:
    """Planar yaw of a quaternion (inverse of main.py:31-36 for roll=pitch=0)."""
    return math.atan2(2.0 * (q.w * q.z + q.x * q.y), 1.0 - 2.0 * (q.y * q.y + q.z * q.z))


def quaternion_from_yaw(yaw: float) -> Quaternion:
    """main.py:31-36's euler_to_quaternion(0, 0, yaw)."""
    return Quaternion(0.0, 0.0, math.sin(yaw / 2.0), math.cos(yaw / 2.0))


def stamp_seconds(stamp) -> float:
    """builtin_interfaces/Time (sec, nanosec) or plain seconds."""
    if hasattr(stamp, "sec"):
        return float(stamp.sec) + 1e-9 * float(stamp.nanosec)
    return float(stamp)


@dataclass
class SlamParams:
    """The slam_toolbox parameters the mapping stage uses, with the values of
    server/thymio_project/config/slam_config.yaml as defaults (line numbers
    there), plus this build's fixed grid size and exploration switches."""

    odom_frame: str = "odom"              # :16 (parent of the pose with dm_scan_matching)
    map_frame: str = "map"                # :17
    base_frame: str = "base_link"         # :18
    scan_topic: str = "/scan"             # :19
    throttle_scans: int = 1               # :23
    map_update_interval: float = 5.0      # :25
    resolution: float = 0.05              # :26
    max_laser_range: float = 12.0         # :27
    minimum_time_interval: float = 0.5    # :28
    minimum_travel_distance: float = 0.1  # :37
    minimum_travel_heading: float = 0.1   # :38
    # the correlative scan matcher's settings (used with dm_scan_matching)
    use_scan_matching: bool = True                          # :35
    link_match_minimum_response_fine: float = 0.1           # :41
    correlation_search_space_dimension: float = 0.5         # :51
    correlation_search_space_resolution: float = 0.01       # :52
    correlation_search_space_smear_deviation: float = 0.1   # :53
    fine_search_angle_offset: float = 0.00349               # :64
    coarse_search_angle_offset: float = 0.349               # :65
    coarse_angle_resolution: float = 0.0349                 # :66
    # its wide search's settings (used with dm_relocalize)
    loop_match_minimum_response_coarse: float = 0.35        # :47
    loop_match_minimum_response_fine: float = 0.45          # :48
    loop_search_space_dimension: float = 8.0                # :56
    loop_search_space_smear_deviation: float = 0.03         # :58
    # this build (not slam_toolbox parameters)
    dm_width: int = 4096                  # cells; a 204.8 m square at 5 cm
    dm_height: int = 4096
    dm_origin_x: float = float("nan")     # NaN: map centred on the world origin
    dm_origin_y: float = float("nan")
    dm_device: int = 0
    dm_devices: str = ""                  # e.g. "0,1,2,3": one map sharded in row bands over these GPUs
    dm_explore: bool = False              # publish /goal_pose after each map update
    dm_goal_min_size: int = 8
    dm_goal_distance_weight: float = 1.0
    dm_goal_min_distance: float = 0.3
    # score goals by path length over the inflated map (dm_assign_goals_path)
    # and publish the path on /plan; off: straight-line distance, as before
    dm_goal_path_distance: bool = False
    dm_goal_inflate_m: float = 0.10       # obstacle inflation radius (the robot's)
    dm_goal_snap_m: float = 0.25          # how far a goal may move to reach a traversable cell
    # keep /plan away from walls: the path comes from a field whose moves cost
    # more within this distance of an obstacle (dm_plan_field_cost with Nav2's
    # inflation curve, inscribed radius dm_goal_inflate_m); the goal itself is
    # chosen as before.  0: off, /plan is the shortest path, as before
    dm_plan_clearance_m: float = 0.0
    dm_plan_cost_scaling: float = 10.0    # Nav2's cost_scaling_factor (its default)
    # score goals by what the sensor would see from them, the unknown cells its
    # rays reach on the current map (dm_assign_goals_gain), in place of the
    # frontier's size; implies dm_goal_path_distance; off: as before
    dm_goal_information_gain: bool = False
    dm_goal_gain_radius_m: float = float("nan")   # NaN: the map's range_max (max_laser_range)
    dm_goal_min_gain: int = 1
    # discount a goal's gain by what the goals the peers already hold will see
    # (dm_assign_goals_coord; the peers' goals arrive on dm_peer_goals_topic as
    # a geometry_msgs/PoseArray in the map frame); implies
    # dm_goal_information_gain; off: as before
    dm_goal_coordinate: bool = False
    dm_peer_goals_topic: str = "/peer_goals"
    # the teammates' poses (geometry_msgs/PoseArray in the map frame); when set,
    # the node also publishes on /team_goals one goal per robot, own pose first,
    # from the global-greedy assignment over all of them (dm_assign_goals_team:
    # the best robot-frontier pair first, so no robot takes the frontier next to
    # a teammate).  Uses the goal settings above; "": off, nothing changes.
    dm_team_poses_topic: str = ""
    # a peer's map (nav_msgs/OccupancyGrid in the peer's map frame) folded into
    # this one on the device (dm_fuse_state); "": off.  Mode "fill" writes only
    # cells this map does not know yet, so a peer republishing its map every
    # map_update_interval does not count its evidence twice; "add" adds log-odds.
    # dm_peer_map_transform: "x,y,yaw" of the peer's frame in ours; "": unknown
    # until MappingNode.align_peer finds it, peer maps are dropped meanwhile.
    dm_peer_map_topic: str = ""
    dm_peer_map_mode: str = "fill"
    dm_peer_map_transform: str = ""
    # correct every accepted scan's pose against the map on the device
    # (dm_match_scans) and keep the correction as map -> odom; off: the pose
    # provider's pose is taken as it is, as before.  Needs use_scan_matching
    # too (the reference's own switch, true in its yaml).
    dm_scan_matching: bool = False
    # a dm_save checkpoint loaded into the mapper at start ("": none), the
    # reference's "localization to use a existing map" (slam_config.yaml:20)
    dm_map_file: str = ""
    # with a loaded map: integrate nothing until a scan has been found in it
    # (OccupancyMapper.relocalize over the whole map, dm_match_global); the
    # pose found becomes map -> odom.  Needs dm_scan_matching.
    dm_relocalize: bool = False

    @classmethod
    def from_dict(cls, d: dict) -> "SlamParams":
        """Known keys of a ros__parameters mapping; others are ignored
        (slam_toolbox's loop-closure and variance-penalty settings are not
        this stage's; its correlative matcher's are, see dm_scan_matching)."""
        p = cls()
        for f in fields(cls):
            if f.name in d:
                setattr(p, f.name, type(getattr(p, f.name))(d[f.name]))
        return p

    @classmethod
    def from_yaml(cls, path: str, node_name: str = "slam_toolbox") -> "SlamParams":
        import yaml

        with open(path) as fh:
            doc = yaml.safe_load(fh) or {}
        section = doc.get(node_name, doc.get("/**", {}))
        return cls.from_dict(section.get("ros__parameters", {}))

    def goal_cells(self) -> tuple[int, int]:
        """(inflate_cells, snap_cells): the two lengths in cells,
        ceil(x / resolution), clamped to the C-ABI's limits (32, 16)."""
        res = float(self.resolution)
        inflate = int(math.ceil(float(self.dm_goal_inflate_m) / res))
        snap = int(math.ceil(float(self.dm_goal_snap_m) / res))
        return min(max(inflate, 0), 32), min(max(snap, 0), 16)

    def clearance_cells(self) -> int:
        """dm_plan_clearance_m in cells, ceil(x / resolution), clamped to the
        C-ABI's limits [1, 32]; 0: off."""
        m = float(self.dm_plan_clearance_m)
        if not m > 0.0:
            return 0
        return min(max(int(math.ceil(m / float(self.resolution))), 1), 32)

    def gain_radius_cells(self) -> int:
        """dm_goal_gain_radius_m in cells, ceil(x / resolution), clamped to the
        C-ABI's limits [1, 511]; NaN: the map's range_max."""
        m = float(self.dm_goal_gain_radius_m)
        if math.isnan(m):
            m = float(self.max_laser_range)
        return min(max(int(math.ceil(m / float(self.resolution))), 1), 511)

    def grid_params(self):
        kw = dict(resolution=float(self.resolution), range_max=float(self.max_laser_range))
        if not math.isnan(self.dm_origin_x):
            kw["origin_x"] = float(self.dm_origin_x)
        if not math.isnan(self.dm_origin_y):
            kw["origin_y"] = float(self.dm_origin_y)
        return default_params(int(self.dm_width), int(self.dm_height), **kw)


class ScanGate:
    """Which scans the mapping stage integrates, as slam_toolbox decides it.
    slam_toolbox is not vendored and its version is not pinned (README.md:28
    names the apt package ros-jazzy-slam-toolbox), so this restates its
    published sources (SlamToolbox::shouldProcessScan in
    slam_toolbox_common.cpp, then the Karto mapper's Mapper::HasMovedEnough in
    lib/karto_sdk/src/Mapper.cpp); parity with them is unpinned (SURVEY.md
    §8(c)).  Two layers, in this order:

    1. slam_toolbox's front gate (``shouldProcessScan``; its scan counter counts
       every scan offered, the first included):
       * the first scan is always processed;
       * ``throttle_scans``: dropped unless counter % throttle_scans == 0;
       * ``minimum_time_interval``: dropped if closer in time than this to the
         last scan that passed this gate;
       * dropped if it moved less than ``0.8 * minimum_travel_distance²``
         (squared, "within 10 % for correction error") from that scan's
         pose, or while the counter is below 5 (warm-up).  A robot turning
         in place is therefore never integrated, whatever it turned.
    2. Karto's ``HasMovedEnough`` against the last *processed* scan: processed
       if ``minimum_time_interval`` has passed, or the laser turned by
       ``minimum_travel_heading`` (normalised angle), or moved
       ``minimum_travel_distance`` (squared, less Karto's KT_TOLERANCE 1e-9).
       After layer 1 the time test already holds, so this layer only matters
       when the thresholds are configured differently for the two.

    The values of the reference's slam_config.yaml (lines 23, 28, 37, 38) are
    ``SlamParams``' defaults."""

    KT_TOLERANCE = 1e-9

    def __init__(self, throttle_scans=1, minimum_time_interval=0.5, minimum_travel_distance=0.1,
                 minimum_travel_heading=0.1):
        self.throttle = max(1, int(throttle_scans))
        self.min_dt = float(minimum_time_interval)
        self.min_d2 = float(minimum_travel_distance) ** 2
        self.min_heading = float(minimum_travel_heading)
        self.counter = 0
        self.front = None  # (stamp, x, y) of the last scan past slam_toolbox's gate
        self.last = None   # (stamp, x, y, yaw) of the last processed scan (Karto)

    @classmethod
    def from_params(cls, p: SlamParams) -> "ScanGate":
        return cls(p.throttle_scans, p.minimum_time_interval, p.minimum_travel_distance,
                   p.minimum_travel_heading)

    def _front(self, stamp: float, x: float, y: float) -> bool:
        self.counter += 1
        if self.front is None:
            self.front = (stamp, x, y)
            return True
        if self.counter % self.throttle != 0:
            return False
        t0, x0, y0 = self.front
        if stamp - t0 < self.min_dt:
            return False
        if (x - x0) ** 2 + (y - y0) ** 2 < 0.8 * self.min_d2 or self.counter < 5:
            return False
        self.front = (stamp, x, y)
        return True

    def _moved_enough(self, stamp: float, x: float, y: float, yaw: float) -> bool:
        if self.last is None:
            return True
        t0, x0, y0, yaw0 = self.last
        if stamp - t0 >= self.min_dt:
            return True
        if abs(math.remainder(yaw - yaw0, 2.0 * math.pi)) >= self.min_heading:
            return True
        return (x - x0) ** 2 + (y - y0) ** 2 >= self.min_d2 - self.KT_TOLERANCE

    def accept(self, stamp: float, pose) -> bool:
        x, y, yaw = (float(v) for v in pose)
        if not self._front(stamp, x, y):
            return False
        if not self._moved_enough(stamp, x, y, yaw):
            return False
        self.last = (stamp, x, y, yaw)
        return True


def se2_compose(a, b):
    """a o b for planar poses (x, y, yaw): b expressed in a's frame, in a's parent."""
    ax, ay, at = (float(v) for v in a)
    bx, by, bt = (float(v) for v in b)
    c, s = math.cos(at), math.sin(at)
    return (ax + (c * bx - s * by), ay + (s * bx + c * by), at + bt)


def se2_inverse(a):
    ax, ay, at = (float(v) for v in a)
    c, s = math.cos(at), math.sin(at)
    return (-(c * ax + s * ay), -(c * ay - s * ax), -at)


def parse_devices(spec) -> list[int]:
    """dm_devices: "0,1,2,3" (or a list) -> [0, 1, 2, 3]; "" -> []."""
    if isinstance(spec, (list, tuple)):
        return [int(d) for d in spec]
    return [int(d) for d in str(spec).replace(" ", "").split(",") if d != ""]


def parse_transform(spec):
    """dm_peer_map_transform: "x,y,yaw" (or three numbers) -> (x, y, yaw); "" -> None."""
    if isinstance(spec, (list, tuple)):
        parts = list(spec)
    else:
        parts = [v for v in str(spec).replace(" ", "").split(",") if v != ""]
    if not parts:
        return None
    if len(parts) != 3:
        raise ValueError(f"dm_peer_map_transform needs x,y,yaw, got {spec!r}")
    x, y, yaw = (float(v) for v in parts)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(yaw)):
        raise ValueError(f"dm_peer_map_transform must be finite, got {spec!r}")
    return (x, y, yaw)


class MappingNode:
    """GPU mapping stage: /scan (+TF) -> /map + /frontiers (+ /goal_pose).

    Callbacks (all non-blocking on the GPU except the /map readback itself):
    ``scan_cb`` per LaserScan, ``timer_cb`` every ``map_update_interval``
    seconds, ``poll_frontiers`` whenever convenient (the rclpy wiring in
    ``main`` runs it on a short timer)."""

    def __init__(self, params: SlamParams | None = None, pose_provider=None, map_publisher=None,
                 frontier_publisher=None, goal_publisher=None, clock=time.monotonic, gate: bool = True,
                 mapper=None, plan_publisher=None, team_goals_publisher=None, **overrides):
        """`overrides` set SlamParams fields (tests: dm_width=..., ...).
        `mapper`: an object with OccupancyMapper's interface to use instead of
        creating one (tests inject CPU stand-ins)."""
        p = params or SlamParams()
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown parameter {k!r}")
            setattr(p, k, v)
        self.slam = p
        self.params = p.grid_params()
        if mapper is None:
            devices = parse_devices(p.dm_devices)
            if len(devices) > 1 and ((p.dm_scan_matching and p.use_scan_matching) or p.dm_relocalize):
                raise ValueError("dm_scan_matching needs the whole map in one handle: it is not available "
                                 "with a map sharded over dm_devices")
            if len(devices) > 1:
                mapper = OccupancyMapper(self.params, devices=devices)
            else:
                mapper = OccupancyMapper(self.params, device=devices[0] if devices else int(p.dm_device))
        self.mapper = mapper
        self.map_update_interval = float(p.map_update_interval)
        self.gate = ScanGate.from_params(p) if gate else None
        self.pose_provider = pose_provider
        self.map_pub = map_publisher or ListPublisher("/map")
        self.frontier_pub = frontier_publisher or ListPublisher("/frontiers")
        self.goal_pub = goal_publisher or ListPublisher("/goal_pose")
        self.plan_pub = plan_publisher or ListPublisher("/plan")
        self.last_plan = None  # the Path of the last goal chosen by path length
        self.last_gain = None  # the gain of the last goal chosen with dm_goal_information_gain
        self.peer_goals = []   # (x, y) of the goals the peers hold (dm_goal_coordinate)
        self.team_poses = []   # (x, y) of the teammates (dm_team_poses_topic)
        self.team_goals_pub = team_goals_publisher or ListPublisher("/team_goals")
        self.clock = clock
        self._last_publish = -math.inf
        self._pass_stamp = None  # stamp of the frontier pass in flight (None: none)
        self.latest_scan = None
        self.latest_pose = None
        self.scans_seen = 0
        self.scans_integrated = 0
        self.updates = 0
        self.last_frontiers = None
        # dm_scan_matching: the pose provider's pose is the odometry pose and
        # map_to_odom the correction C (x, y, yaw), identity until a match is
        # accepted; every scan's prior is C o odom
        self.matching = bool(p.dm_scan_matching) and bool(p.use_scan_matching)
        self.map_to_odom = (0.0, 0.0, 0.0)
        self.scans_matched = 0
        self.scans_rejected = 0
        self.last_match = None             # mapper.match_scan's result for the last matched scan
        self.last_integrated_pose = None   # the pose the last scan was integrated at
        # dm_map_file / dm_relocalize: while `relocalizing`, no scan is integrated
        if p.dm_relocalize and not self.matching:
            raise ValueError("dm_relocalize needs dm_scan_matching (and use_scan_matching)")
        self.map_loaded = bool(p.dm_map_file)
        if self.map_loaded:
            self.mapper.load(str(p.dm_map_file))
        self.relocalizing = bool(p.dm_relocalize) and self.map_loaded
        self.relocalize_rejected = 0
        self.last_relocalize = None        # mapper.relocalize's result of the last attempt
        # dm_peer_map_topic: the peer's frame in ours (x, y, yaw), None until
        # configured or found by align_peer
        if str(p.dm_peer_map_mode) not in ("fill", "add"):
            raise ValueError(f"dm_peer_map_mode must be 'fill' or 'add', got {p.dm_peer_map_mode!r}")
        self.peer_transform = parse_transform(p.dm_peer_map_transform)
        self.peer_maps_fused = 0
        self.peer_maps_dropped = 0
        self.peer_align_rejected = 0
        self.last_peer_align = None        # mapper.relocalize's result of the last align_peer
        self.last_peer_fuse = None         # the stats of the last fused peer map

    # main.py:77-78 keeps the signature scan_cb(self, msg)
    def scan_cb(self, msg):
        self.latest_scan = msg
        self.scans_seen += 1
        self.poll_frontiers()
        pose = self.pose_provider(msg) if self.pose_provider is not None else None
        if pose is None:
            return  # no transform yet: slam_toolbox drops such scans too
        odom = tuple(float(v) for v in pose)
        if self.matching:
            pose = se2_compose(self.map_to_odom, odom)  # the prior
        self.latest_pose = tuple(float(v) for v in pose)
        stamp = stamp_seconds(msg.header.stamp)
        if self.gate is not None and not self.gate.accept(stamp, pose):
            return
        if self.relocalizing:
            pose = self._relocalize(msg, odom)
            if pose is None:
                return
            self.latest_pose = pose
        elif self.matching and (self.scans_integrated > 0 or self.map_loaded):
            pose = self._match(msg, odom, pose)
            self.latest_pose = pose
        u, _ = self.mapper.integrate_scan(msg, pose)
        self.last_integrated_pose = tuple(float(v) for v in pose)
        self.updates += u
        self.scans_integrated += 1

    def peer_goals_cb(self, msg):
        """dm_peer_goals_topic: the goals the other robots hold now; the next
        choose_goal with dm_goal_coordinate discounts what they will see."""
        self.peer_goals = [(float(p.position.x), float(p.position.y)) for p in msg.poses]

    def team_poses_cb(self, msg):
        """dm_team_poses_topic: where the teammates are now; the next
        choose_team_goals assigns goals to this robot and to them together."""
        self.team_poses = [(float(p.position.x), float(p.position.y)) for p in msg.poses]

    def choose_team_goals(self, stamp: float | None = None):
        """dm_team_poses_topic: the goals of this robot (first) and of its
        teammates, in the order of the last team_poses message, from the
        global-greedy assignment over the last published frontier clusters
        (dm_assign_goals_team), with the node's goal settings; scored by
        information gain with dm_goal_information_gain, else by size.  A
        PoseArray in the map frame with one pose per robot, NaN position for a
        robot without a goal; None when the topic is not set or there is no
        pose or frontier result yet."""
        s = self.slam
        if not s.dm_team_poses_topic or self.last_frontiers is None or self.latest_pose is None:
            return None
        x, y, _ = self.latest_pose
        robots = [(x, y)] + list(self.team_poses)
        inflate, snap = s.goal_cells()
        gain = s.dm_goal_information_gain or s.dm_goal_coordinate
        goals = self.mapper.assign_goals_team(robots, min_size=s.dm_goal_min_size, min_gain=s.dm_goal_min_gain,
                                              distance_weight=s.dm_goal_distance_weight,
                                              min_distance=s.dm_goal_min_distance, inflate_cells=inflate,
                                              snap_cells=snap, radius_cells=s.gain_radius_cells() if gain else 0)
        msg = PoseArray(header=Header(stamp=self._last_publish if stamp is None else stamp, frame_id=s.map_frame))
        for (rx, ry), g in zip(robots, goals):
            if g is None:
                msg.poses.append(Pose(position=Point(math.nan, math.nan, 0.0)))
            else:
                gx, gy = g[1]
                msg.poses.append(Pose(position=Point(gx, gy, 0.0),
                                      orientation=quaternion_from_yaw(math.atan2(gy - ry, gx - rx))))
        return msg

    def align_peer(self, scan_msg, peer_pose) -> bool:
        """Find the peer's frame in ours from one of its scans: `scan_msg` was
        taken at `peer_pose` (x, y, yaw) in the peer's map frame; relocalised in
        this map (OccupancyMapper.relocalize, the whole map) it gives the
        transform matched o peer_pose^-1 that peer_map_cb then uses.  A rejected
        match is counted and leaves the transform as it was."""
        from . import fuse

        res = self.mapper.relocalize(scan_msg, None, self.slam)
        self.last_peer_align = res
        if not res["accepted"]:
            self.peer_align_rejected += 1
            return False
        self.peer_transform = fuse.peer_transform(tuple(float(v) for v in res["pose"]),
                                                  tuple(float(v) for v in peer_pose))
        return True

    def peer_map_cb(self, msg):
        """dm_peer_map_topic: a peer's nav_msgs/OccupancyGrid in its own frame,
        folded into this map on the device (OccupancyMapper.fuse_state,
        dm_fuse_state) in mode dm_peer_map_mode.  The geometry is msg.info's;
        a turned origin is composed into the transform (the grid turns about
        its origin corner).  Without a known transform the message is counted
        in peer_maps_dropped and ignored."""
        if self.peer_transform is None:
            self.peer_maps_dropped += 1
            return None
        info = msg.info
        ox, oy = float(info.origin.position.x), float(info.origin.position.y)
        geom = {"width": int(info.width), "height": int(info.height), "resolution": float(info.resolution),
                "origin_x": ox, "origin_y": oy}
        transform = self.peer_transform
        oyaw = yaw_from_quaternion(info.origin.orientation)
        if oyaw != 0.0:
            # p_frame = O + R(oyaw) (p - O) for a point p of the unturned grid
            c, s = math.cos(oyaw), math.sin(oyaw)
            transform = se2_compose(transform, (ox - (c * ox - s * oy), oy - (s * ox + c * oy), oyaw))
        data = np.asarray(msg.data, dtype=np.int8)
        stats = self.mapper.fuse_state(data, geom, transform, str(self.slam.dm_peer_map_mode))
        self.last_peer_fuse = stats
        self.peer_maps_fused += 1
        return stats

    def _match(self, msg, odom, prior):
        """Correct an accepted scan's prior against the map (the device's
        two-stage correlative search, OccupancyMapper.match_scan; what
        slam_toolbox's matcher does for the reference, slam_config.yaml:35,
        50-53, 64-66).  A response of at least link_match_minimum_response_fine
        (:41) accepts the match: the scan is integrated at the matched pose and
        map_to_odom becomes matched o odom^-1.  Otherwise the prior stands."""
        res = self.mapper.match_scan(msg, prior, self.slam)
        self.last_match = res
        if res["response"] >= float(self.slam.link_match_minimum_response_fine):
            matched = tuple(float(v) for v in res["pose"])
            self.map_to_odom = se2_compose(matched, se2_inverse(odom))
            self.scans_matched += 1
            return matched
        self.scans_rejected += 1
        return tuple(float(v) for v in prior)

    def _relocalize(self, msg, odom):
        """Find an accepted scan in the loaded map (OccupancyMapper.relocalize:
        the whole map, every yaw; what slam_toolbox's localization mode does
        for the reference, slam_config.yaml:20, :47-48, :56-58).  Accepted:
        map_to_odom becomes matched o odom^-1 and the scan is integrated at
        the matched pose; the node then goes on matching.  Rejected: counted,
        and nothing is integrated (None)."""
        res = self.mapper.relocalize(msg, None, self.slam)
        self.last_relocalize = res
        if not res["accepted"]:
            self.relocalize_rejected += 1
            return None
        matched = tuple(float(v) for v in res["pose"])
        self.map_to_odom = se2_compose(matched, se2_inverse(odom))
        self.relocalizing = False
        return matched

    def timer_cb(self):
        """The map_update_interval timer: publish /map and start a frontier
        pass, independent of scan gating.  Before the first integrated scan
        there is no map (slam_toolbox has no grid before its first processed
        scan either)."""
        self.poll_frontiers()
        if self.scans_integrated == 0:
            return
        self.publish_map(stamp=self.clock())

    def occupancy_grid(self, stamp: float = 0.0):
        st = self.mapper.state()
        p = self.params
        data = array.array("b")
        data.frombytes(st.tobytes())  # one copy of the device readback, no per-cell objects
        if HAVE_ROS:  # pragma: no cover
            msg = _RosOccupancyGrid()
            msg.header.frame_id = self.slam.map_frame
            msg.header.stamp = time_msg(stamp)
            msg.info.map_load_time = time_msg(stamp)
            msg.info.resolution = float(p.resolution)
            msg.info.width = int(p.width)
            msg.info.height = int(p.height)
            msg.info.origin.position.x = float(p.origin_x)
            msg.info.origin.position.y = float(p.origin_y)
            msg.info.origin.orientation.w = 1.0
            msg.data = data
            return msg
        return OccupancyGrid(
            header=Header(stamp=stamp, frame_id=self.slam.map_frame),
            info=MapMetaData(map_load_time=stamp, resolution=float(p.resolution), width=int(p.width),
                             height=int(p.height),
                             origin=Pose(position=Point(float(p.origin_x), float(p.origin_y), 0.0))),
            data=data)

    def frontier_clusters(self) -> list:
        """Synchronous frontier extraction of the map as it is now."""
        fr = self.mapper.frontiers()
        self.last_frontiers = fr.clusters
        return self._cluster_msgs(fr.clusters)

    @staticmethod
    def _cluster_msgs(clusters) -> list:
        return [FrontierCluster(int(c["label"]), int(c["size"]), float(c["cx_m"]), float(c["cy_m"]))
                for c in clusters]

    def choose_goal(self, stamp: float | None = None):
        """The frontier goal for the robot at its latest pose, chosen on the
        device over the last published frontier clusters (dm_assign_goals;
        policy: dm.goals): PoseStamped in the map frame facing the goal, or
        None."""
        if self.last_frontiers is None or self.latest_pose is None:
            return None
        x, y, _ = self.latest_pose
        s = self.slam
        self.last_plan = None
        if s.dm_goal_path_distance or s.dm_goal_information_gain or s.dm_goal_coordinate:
            return self._choose_goal_by_path(x, y, self._last_publish if stamp is None else stamp)
        g = self.mapper.assign_goals([(x, y)], min_size=s.dm_goal_min_size,
                                     distance_weight=s.dm_goal_distance_weight,
                                     min_distance=s.dm_goal_min_distance)[0]
        if g is None:
            return None
        gx, gy = g[1]
        msg = PoseStamped(header=Header(stamp=self._last_publish if stamp is None else stamp,
                                        frame_id=s.map_frame))
        msg.pose.position = Point(gx, gy, 0.0)
        msg.pose.orientation = quaternion_from_yaw(math.atan2(gy - y, gx - x))
        return msg

    def _choose_goal_by_path(self, x: float, y: float, stamp: float):
        """dm_goal_path_distance: the goal is the centre of a reachable cell,
        scored by the path length from the robot (dm_assign_goals_path), and
        the path to it (dm_plan_path over the field that call left) becomes
        ``last_plan``, a nav_msgs/Path whose poses face along the path.  With
        dm_goal_information_gain the score's numerator is the unknown area
        visible from that cell (dm_assign_goals_gain), kept in ``last_gain``;
        with dm_goal_coordinate it is what of that the peers' goals do not
        already see (dm_assign_goals_coord with ``peer_goals`` held).  With
        dm_plan_clearance_m the goal is chosen the same way and the path is
        taken from the penalty-weighted field from the robot instead
        (dm_plan_field_cost), so it keeps its distance from walls."""
        s = self.slam
        inflate, snap = s.goal_cells()
        if s.dm_goal_coordinate:
            g = self.mapper.assign_goals_coord([(x, y)], held_xy=self.peer_goals, min_size=s.dm_goal_min_size,
                                               min_gain=s.dm_goal_min_gain,
                                               distance_weight=s.dm_goal_distance_weight,
                                               min_distance=s.dm_goal_min_distance, inflate_cells=inflate,
                                               snap_cells=snap, radius_cells=s.gain_radius_cells())[0]
            self.last_gain = None if g is None else int(g[3])
        elif s.dm_goal_information_gain:
            g = self.mapper.assign_goals_gain([(x, y)], min_size=s.dm_goal_min_size,
                                              min_gain=s.dm_goal_min_gain,
                                              distance_weight=s.dm_goal_distance_weight,
                                              min_distance=s.dm_goal_min_distance, inflate_cells=inflate,
                                              snap_cells=snap, radius_cells=s.gain_radius_cells())[0]
            self.last_gain = None if g is None else int(g[3])
        else:
            g = self.mapper.assign_goals_path([(x, y)], min_size=s.dm_goal_min_size,
                                              distance_weight=s.dm_goal_distance_weight,
                                              min_distance=s.dm_goal_min_distance, inflate_cells=inflate,
                                              snap_cells=snap)[0]
        if g is None:
            return None
        gx, gy = g[1]
        header = Header(stamp=stamp, frame_id=s.map_frame)
        p = self.params
        R = s.clearance_cells()
        if R:
            from .plan import inflation_table

            pen = inflation_table(float(p.resolution), R, float(s.dm_goal_inflate_m), float(s.dm_plan_cost_scaling))
            self.mapper.plan_field_cost([(x, y)], inflate, R, pen)
        cells = self.mapper.plan_path((gx, gy), snap_cells=0)
        px = float(p.origin_x) + ((cells % int(p.width)) + 0.5) * float(p.resolution)
        py = float(p.origin_y) + ((cells // int(p.width)) + 0.5) * float(p.resolution)
        plan = Path(header=header)
        for i in range(len(cells)):
            j = min(i + 1, len(cells) - 1)
            yaw = math.atan2(py[j] - py[j - 1], px[j] - px[j - 1]) if len(cells) > 1 else 0.0
            plan.poses.append(PoseStamped(header=header, pose=Pose(position=Point(float(px[i]), float(py[i]), 0.0),
                                                                   orientation=quaternion_from_yaw(yaw))))
        self.last_plan = plan
        msg = PoseStamped(header=header)
        msg.pose.position = Point(gx, gy, 0.0)
        msg.pose.orientation = quaternion_from_yaw(math.atan2(gy - y, gx - x))
        return msg

    def publish_map(self, stamp: float = 0.0):
        """Publish /map now and start the frontier pass of this map (its
        clusters are published by poll_frontiers once the GPU is done)."""
        self._last_publish = stamp
        self.map_pub.publish(self.occupancy_grid(stamp))
        if self._pass_stamp is not None:
            self.poll_frontiers(wait=True)  # the previous tick's pass (long done by now)
        self.mapper.frontiers_begin()
        self._pass_stamp = stamp

    def poll_frontiers(self, wait: bool = False) -> bool:
        """Publish the frontier pass in flight if the GPU has finished it
        (never blocks unless `wait`).  Returns True if it published."""
        if self._pass_stamp is None:
            return False
        if not wait and not self.mapper.frontiers_ready():
            return False
        stamp, self._pass_stamp = self._pass_stamp, None
        fr = self.mapper.frontiers_end()
        clusters = fr.clusters if fr is not None else self.mapper.frontiers().clusters  # overflowed: rerun
        self.last_frontiers = clusters
        self.frontier_pub.publish(self._cluster_msgs(clusters))
        if self.slam.dm_explore:
            goal = self.choose_goal(stamp)
            if goal is not None:
                self.goal_pub.publish(goal)
                if self.last_plan is not None:
                    self.plan_pub.publish(self.last_plan)
            if self.slam.dm_team_poses_topic:
                team = self.choose_team_goals(stamp)
                if team is not None:
                    self.team_goals_pub.publish(team)
        return True

    def map_image_png(self) -> bytes:
        """What get_map_image serves (main.py:256-273), rendered on the GPU
        (dm_map_image) and PNG-encoded with PIL."""
        from PIL import Image

        img = Image.fromarray(self.mapper.map_image(), mode="L")
        buf = io.BytesIO()
        img.save(buf, "PNG")
        return buf.getvalue()

    def destroy_node(self):
        self.mapper.close()


def time_msg(t: float):  # pragma: no cover - needs ROS 2
    """Seconds -> builtin_interfaces/Time."""
    from builtin_interfaces.msg import Time

    sec = int(math.floor(t))
    return Time(sec=sec, nanosec=int(round((t - sec) * 1e9)) % 1_000_000_000)


def main(args=None):  # pragma: no cover - needs ROS 2
    """ros2 run entry point: wires MappingNode into rclpy (tf2 pose lookup).
    Parameters are declared with SlamParams' defaults, so the node takes the
    reference's slam_config.yaml (launch/dm_pc_server.launch.py passes it)."""
    if not HAVE_ROS:
        raise SystemExit("rclpy is not available; MappingNode can still be used as a library")
    import rclpy
    from rclpy.node import Node
    from sensor_msgs.msg import LaserScan as RosLaserScan
    from nav_msgs.msg import OccupancyGrid as RosGrid, Path as RosPath
    from geometry_msgs.msg import PoseArray as RosPoseArray, Pose as RosPose, PoseStamped as RosPoseStamped
    import tf2_ros

    rclpy.init(args=args)
    node = Node("dm_mapper")
    defaults = SlamParams()
    values = {}
    for f in fields(SlamParams):
        node.declare_parameter(f.name, getattr(defaults, f.name))
        values[f.name] = node.get_parameter(f.name).value
    sp = SlamParams.from_dict(values)
    tf_buffer = tf2_ros.Buffer()
    tf2_ros.TransformListener(tf_buffer, node)

    def lookup(msg):
        try:
            # with dm_scan_matching this node publishes map -> odom itself: the
            # pose it corrects is the laser's in the odometry frame
            parent = sp.odom_frame if (sp.dm_scan_matching and sp.use_scan_matching) else sp.map_frame
            t = tf_buffer.lookup_transform(parent, msg.header.frame_id, msg.header.stamp)
        except Exception:
            return None
        tr = t.transform
        return (tr.translation.x, tr.translation.y, yaw_from_quaternion(tr.rotation))

    map_pub = node.create_publisher(RosGrid, "/map", 10)
    fr_pub = node.create_publisher(RosPoseArray, "/frontiers", 10)
    goal_pub = node.create_publisher(RosPoseStamped, "/goal_pose", 10)

    class _FrontierAdapter:
        def publish(self, clusters):
            pa = RosPoseArray()
            pa.header.frame_id = sp.map_frame
            pa.header.stamp = node.get_clock().now().to_msg()
            for c in clusters:
                ps = RosPose()
                ps.position.x, ps.position.y = c.x, c.y
                pa.poses.append(ps)
            fr_pub.publish(pa)

    class _GoalAdapter:
        def publish(self, g):
            m = RosPoseStamped()
            m.header.frame_id = g.header.frame_id
            m.header.stamp = node.get_clock().now().to_msg()
            m.pose.position.x, m.pose.position.y = g.pose.position.x, g.pose.position.y
            q = g.pose.orientation
            m.pose.orientation.z, m.pose.orientation.w = q.z, q.w
            goal_pub.publish(m)

    plan_pub = node.create_publisher(RosPath, "/plan", 10)

    class _PlanAdapter:
        def publish(self, plan):
            m = RosPath()
            m.header.frame_id = plan.header.frame_id
            m.header.stamp = node.get_clock().now().to_msg()
            for ps in plan.poses:
                q = RosPoseStamped()
                q.header = m.header
                q.pose.position.x, q.pose.position.y = ps.pose.position.x, ps.pose.position.y
                q.pose.orientation.z, q.pose.orientation.w = ps.pose.orientation.z, ps.pose.orientation.w
                m.poses.append(q)
            plan_pub.publish(m)

    team_pub = node.create_publisher(RosPoseArray, "/team_goals", 10) if sp.dm_team_poses_topic else None

    class _TeamGoalsAdapter:
        def publish(self, goals):
            pa = RosPoseArray()
            pa.header.frame_id = goals.header.frame_id
            pa.header.stamp = node.get_clock().now().to_msg()
            for g in goals.poses:
                ps = RosPose()
                ps.position.x, ps.position.y = g.position.x, g.position.y
                ps.orientation.z, ps.orientation.w = g.orientation.z, g.orientation.w
                pa.poses.append(ps)
            team_pub.publish(pa)

    mn = MappingNode(sp, pose_provider=lookup, map_publisher=map_pub, frontier_publisher=_FrontierAdapter(),
                     goal_publisher=_GoalAdapter(), plan_publisher=_PlanAdapter(),
                     team_goals_publisher=_TeamGoalsAdapter() if team_pub is not None else None,
                     clock=lambda: node.get_clock().now().nanoseconds * 1e-9)
    node.create_subscription(RosLaserScan, sp.scan_topic, mn.scan_cb, 10)
    if sp.dm_goal_coordinate:
        node.create_subscription(RosPoseArray, sp.dm_peer_goals_topic, mn.peer_goals_cb, 10)
    if sp.dm_team_poses_topic:
        node.create_subscription(RosPoseArray, sp.dm_team_poses_topic, mn.team_poses_cb, 10)
    if sp.dm_peer_map_topic:
        node.create_subscription(RosGrid, sp.dm_peer_map_topic, mn.peer_map_cb, 10)
    # slam_toolbox publishes the map on its own period, not per scan
    node.create_timer(sp.map_update_interval, mn.timer_cb)
    node.create_timer(0.01, mn.poll_frontiers)  # frontiers go out as soon as the GPU pass is done
    if mn.matching:
        # slam_toolbox's part of the TF chain map -> odom -> base_link -> base_laser
        # (slam_config.yaml:24 transform_publish_period)
        from geometry_msgs.msg import TransformStamped

        broadcaster = tf2_ros.TransformBroadcaster(node)

        def broadcast_map_to_odom():
            x, y, yaw = mn.map_to_odom
            t = TransformStamped()
            t.header.stamp = node.get_clock().now().to_msg()
            t.header.frame_id = sp.map_frame
            t.child_frame_id = sp.odom_frame
            t.transform.translation.x, t.transform.translation.y = x, y
            q = quaternion_from_yaw(yaw)
            t.transform.rotation.z, t.transform.rotation.w = q.z, q.w
            broadcaster.sendTransform(t)

        node.create_timer(0.1, broadcast_map_to_odom)
    try:
        rclpy.spin(node)
    finally:
        mn.destroy_node()
        node.destroy_node()
        rclpy.shutdown()


if __name__ == "__main__":  # pragma: no cover
    main()

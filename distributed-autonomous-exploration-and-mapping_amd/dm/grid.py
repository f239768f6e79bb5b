"""Python host side of the hot path: a locked handle over libdm.so.

``OccupancyMapper`` is what a ROS 2 node calls (dm/ros_node.py): it takes the
same data a ``sensor_msgs/LaserScan`` carries (ranges, angle_min,
angle_increment) plus the laser pose, and yields what ``nav_msgs/OccupancyGrid``
carries (int8 row-major -1/0/100, origin bottom-left), i.e. the data
``ThymioBrain.map_cb`` caches and ``get_map_image`` renders
(server/thymio_project/thymio_project/main.py:80-81, 241-279).

Threading: the reference writes ``latest_map`` on the
rclpy spin thread and reads it on the Flask thread (main.py:80-81 vs
:244-256); a libdm handle is not thread-safe, so every call here holds a
per-handle lock and every array returned is a fresh copy.
"""
from __future__ import annotations

import ctypes
import threading
from dataclasses import dataclass

import numpy as np

from . import _ffi
from ._ffi import CLUSTER_DTYPE, DmError, DmParams, check, load_library


def default_params(width: int, height: int, **overrides) -> DmParams:
    """dm_default_params + keyword overrides (resolution 0.05 and max range
    12.0 from slam_config.yaml:26-27)."""
    lib = load_library()
    p = DmParams()
    check(lib.dm_default_params(ctypes.byref(p), int(width), int(height)))
    res_given = "resolution" in overrides
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise DmError(_ffi.DM_ERR_INVALID_ARG, f"unknown parameter {k!r}")
        setattr(p, k, v)
    if res_given and "origin_x" not in overrides:
        p.origin_x = -0.5 * p.width * p.resolution
    if res_given and "origin_y" not in overrides:
        p.origin_y = -0.5 * p.height * p.resolution
    return p


def params_from_dict(d: dict) -> DmParams:
    p = DmParams()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def atomic_peak(device: int = 0) -> dict:
    """Measured uncontended atomic throughput of the device (dm_atomic_peak):
    LDS ds_add_u32 and global no-return atomicAdd u32, operations per second."""
    lib = load_library()
    out = (ctypes.c_double * 2)()
    n = ctypes.c_int32(0)
    check(lib.dm_atomic_peak(int(device), out, 2, ctypes.byref(n)))
    return {"lds_add_u32_per_s": float(out[0]), "global_add_u32_per_s": float(out[1])}


@dataclass
class Frontiers:
    """Result of one frontier extraction."""

    clusters: np.ndarray            # structured CLUSTER_DTYPE, sorted by label
    mask: np.ndarray | None = None  # uint8 [rows, W]
    labels: np.ndarray | None = None  # int64 [rows, W], -1 off-frontier

    def __len__(self) -> int:
        return int(self.clusters.shape[0])


def _vp(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class OccupancyMapper:
    """One device-resident map (or one row band of a sharded map)."""

    def __init__(self, params: DmParams, device: int = 0, devices=None):
        """`devices`: a list of HIP devices to shard the map over in row bands
        (dm_create_sharded; a device may repeat); the handle then takes the
        same calls, with results identical to one handle."""
        self._lib = load_library()
        self._lock = threading.RLock()
        self._h = ctypes.c_void_p()
        if devices is not None:
            devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
            check(self._lib.dm_create_sharded(ctypes.byref(self._h), ctypes.byref(params), len(devices), devs))
            device = int(devices[0])
        else:
            check(self._lib.dm_create(ctypes.byref(self._h), ctypes.byref(params), int(device)))
        self.devices = list(devices) if devices is not None else [int(device)]
        out = DmParams()
        check(self._lib.dm_get_params(self._h, ctypes.byref(out)))
        self.params = out
        self.device = device
        self.width = int(out.width)
        self.rows = int(out.band_rows)
        self.row0 = int(out.band_row0)
        self._cap = 1 << 12  # cluster records per frontiers() buffer (grown on demand)
        self.last_incomplete = None  # dm_last_error() of the last pass that returned no result
        self._team_n = 0  # fields of the last plan_team / assign_goals_team: the rows of plan_team_query's matrix

    # -- lifetime ---------------------------------------------------------
    def close(self):
        with self._lock:
            if self._h:
                self._lib.dm_destroy(self._h)
                self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if not self._h:
            raise DmError(_ffi.DM_ERR_STATE, "mapper is closed")
        return self._h

    # -- integration ------------------------------------------------------
    def integrate(self, poses, ranges, angle_min, angle_increment):
        """Integrate S scans: poses [S,3] (x, y, yaw), ranges [S,N] float32.
        Returns (updates U, touched cells T)."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        ranges = np.ascontiguousarray(ranges, dtype=np.float32)
        if ranges.ndim != 2:
            ranges = ranges.reshape(poses.shape[0], -1)
        S, N = ranges.shape
        U = ctypes.c_uint64(0)
        T = ctypes.c_uint64(0)
        with self._lock:
            check(self._lib.dm_integrate(self._handle(), S, _vp(poses), N, _vp(ranges),
                                         float(angle_min), float(angle_increment),
                                         ctypes.byref(U), ctypes.byref(T)))
        return int(U.value), int(T.value)

    def integrate_scan(self, scan, pose):
        """One LaserScan-like message (attributes ranges, angle_min,
        angle_increment) at laser pose (x, y, yaw) in the map frame."""
        ranges = np.asarray(scan.ranges, dtype=np.float32)[None, :]
        return self.integrate(np.asarray(pose, np.float64)[None, :], ranges,
                              np.float32(scan.angle_min), np.float32(scan.angle_increment))

    def integrate_async(self, poses, ranges_ptr: int, S: int, N: int, angle_min, angle_increment):
        """dm_integrate_async: poses [S,3] (read now), ranges a host pointer to
        float32 [S,N] — pinned memory for a truly asynchronous upload — that
        must stay valid until the second integrate_async call after this one
        (or synchronize()).  Returns at once; U/T via last_counts()."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        if poses.shape[0] != S:
            raise DmError(_ffi.DM_ERR_SHAPE, f"poses has {poses.shape[0]} rows, S = {S}")
        with self._lock:
            check(self._lib.dm_integrate_async(self._handle(), int(S), _vp(poses), int(N),
                                               ctypes.c_void_p(ranges_ptr), float(angle_min),
                                               float(angle_increment)))

    def integrate_device(self, d_pose4_ptr: int, S: int, d_ranges_ptr: int, N: int,
                         angle_min, angle_increment):
        """Asynchronous integrate from device pointers (pose4 = x, y, cos yaw,
        sin yaw as float64 [S,4]; ranges float32 [S,N])."""
        with self._lock:
            check(self._lib.dm_integrate_device(self._handle(), int(S), ctypes.c_void_p(d_pose4_ptr),
                                                int(N), ctypes.c_void_p(d_ranges_ptr),
                                                float(angle_min), float(angle_increment)))

    def last_counts(self):
        U = ctypes.c_uint64(0)
        T = ctypes.c_uint64(0)
        with self._lock:
            check(self._lib.dm_last_counts(self._handle(), ctypes.byref(U), ctypes.byref(T)))
        return int(U.value), int(T.value)

    STAT_NAMES = ("updates", "touched", "touched_heavy", "pieces", "active_tiles", "work_items",
                  "heavy_tiles", "frontier_tiles", "frontier_slots", "frontier_clusters", "sparse_items")

    def last_stats(self) -> dict:
        """Diagnostics of the most recent integrate call (dm_last_stats)."""
        k = len(self.STAT_NAMES)
        out = (ctypes.c_uint64 * k)()
        n = ctypes.c_int32(0)
        with self._lock:
            check(self._lib.dm_last_stats(self._handle(), out, k, ctypes.byref(n)))
        return {k: int(out[i]) for i, k in enumerate(self.STAT_NAMES)}

    def frontier_cache_stats(self) -> tuple[int, int]:
        """(hits, misses) of the last collected frontier pass's label cache
        (dm_frontier_cache_stats): tiles labelled from their cached entry /
        labelled in full by the workgroup tile kernel."""
        h, m = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with self._lock:
            check(self._lib.dm_frontier_cache_stats(self._handle(), ctypes.byref(h), ctypes.byref(m)))
        return int(h.value), int(m.value)

    def ld06_to_scans(self, points, offsets, n_beams: int, laser_scan_dir: bool = True,
                      want_intensities: bool = False):
        """LD06 PointData -> LaserScan ranges on the GPU, as the driver's
        ToLaserscanMessagePublish (dm_ld06_to_scans).  points: structured
        array of LD06_POINT_DTYPE; offsets: int64 [S+1].  Returns ranges
        float32 [S, N] (and intensities)."""
        pts = np.ascontiguousarray(points, dtype=np.dtype(_ffi.LD06_POINT_DTYPE))
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        S = off.shape[0] - 1
        ranges = np.empty((S, n_beams), np.float32)
        inten = np.empty((S, n_beams), np.float32) if want_intensities else None
        with self._lock:
            check(self._lib.dm_ld06_to_scans(self._handle(), S, _vp(pts), _vp(off), int(n_beams),
                                             1 if laser_scan_dir else 0, _vp(ranges), _vp(inten)))
        return (ranges, inten) if want_intensities else ranges

    # -- map access -------------------------------------------------------
    def state(self) -> np.ndarray:
        out = np.empty((self.rows, self.width), np.int8)
        with self._lock:
            check(self._lib.dm_get_state(self._handle(), _vp(out)))
        return out

    def logodds(self) -> np.ndarray:
        out = np.empty((self.rows, self.width), np.float32)
        with self._lock:
            check(self._lib.dm_get_logodds(self._handle(), _vp(out)))
        return out

    def set_logodds(self, L):
        L = np.ascontiguousarray(L, dtype=np.float32).reshape(self.rows, self.width)
        with self._lock:
            check(self._lib.dm_set_logodds(self._handle(), _vp(L)))

    def set_state(self, st):
        st = np.ascontiguousarray(st, dtype=np.int8).reshape(self.rows, self.width)
        with self._lock:
            check(self._lib.dm_set_state(self._handle(), _vp(st)))

    # -- map fusion -------------------------------------------------------
    FUSE_STAT_NAMES = ("covered", "contributing", "changed")

    def _fuse(self, fn, values, dtype, geom, transform, mode):
        from . import fuse

        g = geom if isinstance(geom, dict) else fuse.geom_of(geom)
        src = _ffi.DmFuseSource(int(g["width"]), int(g["height"]), float(g["resolution"]), float(g["origin_x"]),
                                float(g["origin_y"]))
        values = np.ascontiguousarray(values, dtype=dtype)
        if values.size != src.width * src.height:
            raise DmError(_ffi.DM_ERR_SHAPE, f"source has {values.size} cells, geometry {src.width} x {src.height}")
        tx, ty, yaw = (float(v) for v in transform)
        out = (ctypes.c_uint64 * 3)()
        with self._lock:
            check(fn(self._handle(), ctypes.byref(src), _vp(values), tx, ty, yaw, fuse.mode_code(mode), out))
        return {k: int(out[i]) for i, k in enumerate(self.FUSE_STAT_NAMES)}

    def fuse_logodds(self, L, geom, transform, mode="add") -> dict:
        """Fold a peer's log-odds map (float32 [h, w], geometry `geom`: a dict
        width / height / resolution / origin_x / origin_y or dm_params, in the
        peer's frame) into this map under transform = (tx, ty, yaw), peer frame
        -> ours (dm_fuse_logodds).  mode "add": log-odds add; "fill": only cells
        this map does not know yet.  Returns {"covered", "contributing",
        "changed"}.  Same result as dm.fuse.fuse_map, bit for bit."""
        return self._fuse(self._lib.dm_fuse_logodds, L, np.float32, geom, transform, mode)

    def fuse_state(self, st, geom, transform, mode="add") -> dict:
        """The same from an OccupancyGrid.data image (int8 -1 / 0 / 100):
        100 adds l_occ, 0 adds l_free (dm_fuse_state)."""
        return self._fuse(self._lib.dm_fuse_state, st, np.int8, geom, transform, mode)

    def fuse_from(self, other_mapper, transform, mode="add") -> dict:
        """The same from another mapper's log-odds, device to device
        (dm_fuse_grid): `other_mapper` is a whole-map mapper on this device."""
        from . import fuse

        tx, ty, yaw = (float(v) for v in transform)
        out = (ctypes.c_uint64 * 3)()
        first, second = sorted((self, other_mapper), key=id)  # one lock order for a pair of mappers
        with first._lock, second._lock:
            check(self._lib.dm_fuse_grid(self._handle(), other_mapper._handle(), tx, ty, yaw, fuse.mode_code(mode),
                                         out))
        return {k: int(out[i]) for i, k in enumerate(self.FUSE_STAT_NAMES)}

    def reset(self):
        with self._lock:
            check(self._lib.dm_reset(self._handle()))

    def map_image(self) -> np.ndarray:
        """get_map_image's grayscale pixels (main.py:256-266), rendered on
        the GPU: uint8 [rows, W], already flipped."""
        out = np.empty((self.rows, self.width), np.uint8)
        with self._lock:
            check(self._lib.dm_map_image(self._handle(), _vp(out)))
        return out

    def _assign(self, fn, robots_xy, args, extra=()):
        """One goal call: fn(handle, robots, R, *args, out_index, out_xy,
        *extra outputs).  `extra`: the dtypes of the int64 / uint32 [R]
        outputs behind out_xy.  Per robot (index, (x, y), *extra) or None."""
        xy = np.ascontiguousarray(np.asarray(robots_xy, np.float64).reshape(-1, 2))
        R = xy.shape[0]
        idx = np.empty(R, np.int64)
        out = np.empty((R, 2), np.float64)
        more = [np.empty(R, dt) for dt in extra]
        with self._lock:
            check(fn(self._handle(), _vp(xy), R, *args, _vp(idx), _vp(out), *[_vp(a) for a in more]))
        return [(int(i), (float(p[0]), float(p[1])), *(int(a[r]) for a in more)) if i >= 0 else None
                for r, (i, p) in enumerate(zip(idx, out))]

    def assign_goals(self, robots_xy, min_size: int = 8, distance_weight: float = 1.0,
                     min_distance: float = 0.0):
        """Frontier goals on the device (dm_assign_goals) over the clusters of
        the last collected frontier result: per robot, in order, (index into
        that result's cluster list, (x, y)) or None.  Same policy as
        dm.goals.assign_goals (the host restatement the tests compare with)."""
        return self._assign(self._lib.dm_assign_goals, robots_xy,
                            (int(min_size), float(distance_weight), float(min_distance)))

    # -- path planning (csrc/dm_plan.h; host restatement: dm/plan.py) ------
    PLAN_STAT_NAMES = ("reached", "traversable", "rounds", "tile_relaxations")

    def plan_traversable(self, inflate_cells: int = 2) -> np.ndarray:
        """The obstacle-inflated traversability mask (dm_plan_traversable):
        bool [rows, W]."""
        out = np.empty((self.rows, self.width), np.uint8)
        with self._lock:
            check(self._lib.dm_plan_traversable(self._handle(), int(inflate_cells), _vp(out)))
        return out.astype(bool)

    def plan_field(self, sources_xy, inflate_cells: int = 2, max_cost: int = 0) -> dict:
        """Compute the shortest-path distance field from the source points
        (metres) on the device (dm_plan_field); it stays in the handle for
        plan_cost_field / plan_query / plan_path until the map changes.
        Returns the call's statistics (PLAN_STAT_NAMES)."""
        xy = np.ascontiguousarray(np.asarray(sources_xy, np.float64).reshape(-1, 2))
        st = (ctypes.c_uint64 * 4)()
        with self._lock:
            check(self._lib.dm_plan_field(self._handle(), _vp(xy), xy.shape[0], int(inflate_cells), int(max_cost), st))
        return {k: int(st[i]) for i, k in enumerate(self.PLAN_STAT_NAMES)}

    def plan_clearance(self, clear_cells: int) -> np.ndarray:
        """The capped squared obstacle distance (dm_plan_clearance): uint16
        [rows, W], clear_cells**2 + 1 where no occupied cell lies within
        clear_cells.  Same values as dm.plan.clearance."""
        out = np.empty((self.rows, self.width), np.uint16)
        with self._lock:
            check(self._lib.dm_plan_clearance(self._handle(), int(clear_cells), _vp(out)))
        return out

    def plan_field_cost(self, sources_xy, inflate_cells: int, clear_cells: int, pen, max_cost: int = 0) -> dict:
        """plan_field with a penalty on cells near obstacles
        (dm_plan_field_cost): entering a cell costs 5 or 7 times
        1 + pen[its clearance], for a uint8 table of clear_cells**2 + 2 entries
        (dm.plan.inflation_table builds Nav2's).  The weighted field stays in
        the handle like plan_field's, and plan_path follows it.  Returns the
        call's statistics (PLAN_STAT_NAMES)."""
        xy = np.ascontiguousarray(np.asarray(sources_xy, np.float64).reshape(-1, 2))
        tab = None
        if pen is not None:
            tab = np.ascontiguousarray(pen, np.uint8)
            if 1 <= int(clear_cells) <= 32 and tab.shape != (int(clear_cells) ** 2 + 2,):
                raise DmError(_ffi.DM_ERR_INVALID_ARG, f"pen must have clear_cells**2 + 2 entries (got {tab.shape})")
        st = (ctypes.c_uint64 * 4)()
        with self._lock:
            check(self._lib.dm_plan_field_cost(self._handle(), _vp(xy), xy.shape[0], int(inflate_cells),
                                               int(clear_cells), None if tab is None else _vp(tab), int(max_cost), st))
        return {k: int(st[i]) for i, k in enumerate(self.PLAN_STAT_NAMES)}

    def plan_cost_field(self) -> np.ndarray:
        """The field (dm_plan_get_field): uint32 [rows, W], costs in fifths of
        a cell (orthogonal move 5, diagonal 7), dm.plan.UNREACHABLE where no
        path leads."""
        out = np.empty((self.rows, self.width), np.uint32)
        with self._lock:
            check(self._lib.dm_plan_get_field(self._handle(), _vp(out)))
        return out

    def plan_query(self, targets_xy, snap_cells: int = 5):
        """Snap target points (metres) to the field (dm_plan_query): (cost
        uint32 [n], cell int64 [n]); (UNREACHABLE, -1) where nothing within
        snap_cells of the target is reached."""
        xy = np.ascontiguousarray(np.asarray(targets_xy, np.float64).reshape(-1, 2))
        n = xy.shape[0]
        cost = np.empty(n, np.uint32)
        cell = np.empty(n, np.int64)
        with self._lock:
            check(self._lib.dm_plan_query(self._handle(), _vp(xy), n, int(snap_cells), _vp(cost), _vp(cell)))
        return cost, cell

    def plan_path(self, target_xy, snap_cells: int = 5, cap: int | None = None) -> np.ndarray:
        """The path to the target's snapped cell, source first, as linear cell
        indices int64 [n] (dm_plan_path); empty if the target is not reached.
        `cap`: the buffer size to use; by default it is grown to the length
        the library reports."""
        n = ctypes.c_int64(0)
        size = 4096 if cap is None else int(cap)
        with self._lock:
            while True:
                buf = np.empty(max(size, 1), np.int64)
                rc = self._lib.dm_plan_path(self._handle(), float(target_xy[0]), float(target_xy[1]),
                                            int(snap_cells), _vp(buf), size, ctypes.byref(n))
                if rc == _ffi.DM_ERR_CAPACITY and cap is None and n.value > size:
                    size = int(n.value)
                    continue
                check(rc)
                return buf[: int(n.value)].copy()

    def assign_goals_path(self, robots_xy, min_size: int = 8, distance_weight: float = 1.0,
                          min_distance: float = 0.0, inflate_cells: int = 2, max_cost: int = 0,
                          snap_cells: int = 5):
        """assign_goals scored by path length (dm_assign_goals_path): per
        robot, in order, (cluster index, (x, y), cell) or None, where (x, y) is
        the centre of the reachable cell the cluster's centroid snaps to.
        Same policy as dm.plan.assign_goals_path."""
        return self._assign(self._lib.dm_assign_goals_path, robots_xy,
                            (int(min_size), float(distance_weight), float(min_distance), int(inflate_cells),
                             int(max_cost), int(snap_cells)), (np.int64,))

    # -- information gain (csrc/dm_gain.h; host restatement: dm/gain.py) ----
    def default_gain_radius(self) -> int:
        """ceil(range_max / resolution) cells, capped at the limit of 511."""
        from .gain import default_radius

        return default_radius(self.params.range_max, self.params.resolution)

    def gain_views(self, views_xy, radius_cells: int | None = None):
        """The visible-unknown count of view points (metres) on the device
        (dm_gain_views): (gain uint32 [n], cell int64 [n]); a view outside the
        grid, or a non-finite one, has cell -1 and gain 0.  `radius_cells`
        defaults to the sensor's range, default_gain_radius()."""
        xy = np.ascontiguousarray(np.asarray(views_xy, np.float64).reshape(-1, 2))
        n = xy.shape[0]
        R = self.default_gain_radius() if radius_cells is None else int(radius_cells)
        gain = np.zeros(n, np.uint32)
        cell = np.full(n, -1, np.int64)
        with self._lock:
            check(self._lib.dm_gain_views(self._handle(), _vp(xy), n, R, _vp(gain), _vp(cell)))
        return gain, cell

    def assign_goals_gain(self, robots_xy, min_size: int = 8, min_gain: int = 0, distance_weight: float = 1.0,
                          min_distance: float = 0.0, inflate_cells: int = 2, max_cost: int = 0,
                          snap_cells: int = 5, radius_cells: int | None = None):
        """assign_goals_path scored by information gain (dm_assign_goals_gain):
        per robot, in order, (cluster index, (x, y), cell, gain) or None, where
        gain is the visible-unknown count of the reachable cell the cluster's
        centroid snaps to.  Same policy as dm.gain.assign_goals_gain."""
        rad = self.default_gain_radius() if radius_cells is None else int(radius_cells)
        return self._assign(self._lib.dm_assign_goals_gain, robots_xy,
                            (int(min_size), int(min_gain), float(distance_weight), float(min_distance),
                             int(inflate_cells), int(max_cost), int(snap_cells), rad), (np.int64, np.uint32))

    def gain_views_joint(self, views_xy, radius_cells: int | None = None):
        """The marginal gains of view points (metres) taken in order
        (dm_gain_views_joint): (marginal uint32 [n], cell int64 [n]); view i
        counts what it sees that the views before it do not.  The claimed set
        it leaves is gain_claimed().  Same as dm.gain.gain_views_joint."""
        xy = np.ascontiguousarray(np.asarray(views_xy, np.float64).reshape(-1, 2))
        n = xy.shape[0]
        R = self.default_gain_radius() if radius_cells is None else int(radius_cells)
        marginal = np.zeros(n, np.uint32)
        cell = np.full(n, -1, np.int64)
        with self._lock:
            check(self._lib.dm_gain_views_joint(self._handle(), _vp(xy), n, R, _vp(marginal), _vp(cell)))
        return marginal, cell

    def assign_goals_coord(self, robots_xy, held_xy=(), min_size: int = 8, min_gain: int = 0,
                           distance_weight: float = 1.0, min_distance: float = 0.0, inflate_cells: int = 2,
                           max_cost: int = 0, snap_cells: int = 5, radius_cells: int | None = None):
        """assign_goals_gain scored by the marginal gain (dm_assign_goals_coord):
        what a goal sees that neither the held views `held_xy` (the goals the
        teammates already hold, metres) nor the goals of the robots before it
        in this call see.  Per robot, in order, (cluster index, (x, y), cell,
        marginal gain) or None; the claimed set it leaves is gain_claimed().
        Same policy as dm.gain.assign_goals_coord."""
        held = np.ascontiguousarray(np.asarray(held_xy, np.float64).reshape(-1, 2))
        rad = self.default_gain_radius() if radius_cells is None else int(radius_cells)
        return self._assign(self._lib.dm_assign_goals_coord, robots_xy,
                            (_vp(held) if held.shape[0] else None, held.shape[0], int(min_size), int(min_gain),
                             float(distance_weight), float(min_distance), int(inflate_cells), int(max_cost),
                             int(snap_cells), rad), (np.int64, np.uint32))

    def gain_claimed(self) -> np.ndarray:
        """The claimed set left by the last gain_views_joint or
        assign_goals_coord (dm_gain_claimed): bool [rows, W]."""
        out = np.empty((self.rows, self.width), np.uint8)
        with self._lock:
            check(self._lib.dm_gain_claimed(self._handle(), _vp(out)))
        return out.astype(bool)

    # -- team planning (csrc/dm_plan.h §4; host restatement: dm/plan.py) ----
    def plan_team(self, robots_xy, inflate_cells: int = 2, max_cost: int = 0) -> dict:
        """One distance field per robot (metres), relaxed together on the
        device (dm_plan_team): field k is plan_field([robots_xy[k]]) bit for
        bit.  The fields stay in the handle beside plan_field's, for
        plan_team_field / plan_team_query / plan_team_path, until the map
        changes.  Returns {"traversable", "rounds", "tile_relaxations",
        "reached": [per robot]}."""
        xy = np.ascontiguousarray(np.asarray(robots_xy, np.float64).reshape(-1, 2))
        n = xy.shape[0]
        st = (ctypes.c_uint64 * (3 + max(n, 1)))()
        with self._lock:
            check(self._lib.dm_plan_team(self._handle(), _vp(xy), n, int(inflate_cells), int(max_cost), st))
            self._team_n = n
        return {"traversable": int(st[0]), "rounds": int(st[1]), "tile_relaxations": int(st[2]),
                "reached": [int(st[3 + k]) for k in range(n)]}

    def plan_team_field(self, k: int) -> np.ndarray:
        """Robot k's field of the last plan_team (dm_plan_team_get_field):
        uint32 [rows, W], as plan_cost_field."""
        out = np.empty((self.rows, self.width), np.uint32)
        with self._lock:
            check(self._lib.dm_plan_team_get_field(self._handle(), int(k), _vp(out)))
        return out

    def plan_team_query(self, targets_xy, snap_cells: int = 5):
        """The robot x target matrix (dm_plan_team_query): (cost uint32
        [n_robots, n], cell int64 [n_robots, n]), plan_query's snap of every
        target under every robot's field."""
        xy = np.ascontiguousarray(np.asarray(targets_xy, np.float64).reshape(-1, 2))
        n = xy.shape[0]
        # the library knows how many fields it holds; its limit bounds the buffers
        cost = np.empty((_ffi.DM_PLAN_TEAM_MAX, n), np.uint32)
        cell = np.empty((_ffi.DM_PLAN_TEAM_MAX, n), np.int64)
        with self._lock:
            check(self._lib.dm_plan_team_query(self._handle(), _vp(xy), n, int(snap_cells), _vp(cost), _vp(cell)))
            R = self._team_n
        return cost.reshape(-1)[: R * n].reshape(R, n).copy(), cell.reshape(-1)[: R * n].reshape(R, n).copy()

    def plan_team_path(self, k: int, target_xy, snap_cells: int = 5, cap: int | None = None) -> np.ndarray:
        """plan_path on robot k's field (dm_plan_team_path)."""
        n = ctypes.c_int64(0)
        size = 4096 if cap is None else int(cap)
        with self._lock:
            while True:
                buf = np.empty(max(size, 1), np.int64)
                rc = self._lib.dm_plan_team_path(self._handle(), int(k), float(target_xy[0]), float(target_xy[1]),
                                                 int(snap_cells), _vp(buf), size, ctypes.byref(n))
                if rc == _ffi.DM_ERR_CAPACITY and cap is None and n.value > size:
                    size = int(n.value)
                    continue
                check(rc)
                return buf[: int(n.value)].copy()

    def assign_goals_team(self, robots_xy, min_size: int = 8, min_gain: int = 0, distance_weight: float = 1.0,
                          min_distance: float = 0.0, inflate_cells: int = 2, max_cost: int = 0,
                          snap_cells: int = 5, radius_cells: int = 0):
        """Global-greedy goals (dm_assign_goals_team): the best (robot,
        cluster) pair is assigned first, so the result does not depend on the
        order of the robots.  radius_cells == 0 scores by cluster size as
        assign_goals_path and returns, per robot, (cluster index, (x, y), cell)
        or None; radius_cells >= 1 scores by information gain as
        assign_goals_gain and returns (cluster index, (x, y), cell, gain).
        Leaves the robots' team fields in the handle (plan_team_path).  Same
        policy as dm.plan.assign_goals_team."""
        rad = int(radius_cells)
        got = self._assign(self._lib.dm_assign_goals_team, robots_xy,
                           (int(min_size), int(min_gain), float(distance_weight), float(min_distance),
                            int(inflate_cells), int(max_cost), int(snap_cells), rad), (np.int64, np.uint32))
        self._team_n = len(got)
        return got if rad != 0 else [g and g[:3] for g in got]

    # -- scan matching (csrc/dm_match.h; host restatement: dm/match.py) ----
    def match_field(self, smear_cells: int, kern) -> np.ndarray:
        """The matcher's response field (dm_match_field): uint8 [rows, W], per
        cell the largest kern[d2] over the occupied cells within smear_cells
        of it.  kern: uint8 [smear_cells**2 + 1] (dm.match.kernel_table)."""
        kern = None if kern is None else np.ascontiguousarray(kern, dtype=np.uint8).reshape(-1)
        if kern is not None and 0 <= int(smear_cells) <= 16 and kern.shape[0] < int(smear_cells) ** 2 + 1:
            raise DmError(_ffi.DM_ERR_INVALID_ARG, "kern needs smear_cells**2 + 1 entries")
        out = np.empty((self.rows, self.width), np.uint8)
        with self._lock:
            check(self._lib.dm_match_field(self._handle(), int(smear_cells), _vp(kern), _vp(out)))
        return out

    def match_scans(self, poses, ranges, angle_min, angle_increment, yaw_offsets, k0: int, sub: int, half: int,
                    stride: int, smear_cells: int, kern, want_volume: bool = False) -> dict:
        """One stage of the correlative matcher on the device (dm_match_scans)
        for S scans: every candidate (yaw + yaw_offsets[k], i * stride, j *
        stride fine steps of resolution / sub) is scored against the response
        field of the map as it is now.  Returns best int32 [S, 3] = (k, i, j),
        score uint32 [S], n_used int32 [S], pose float64 [S, 3] and, with
        want_volume, volume uint32 [S, A, 2*half+1, 2*half+1] (k, j, i).
        Same results as dm.match.match_scans, bit for bit."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        ranges = np.ascontiguousarray(ranges, dtype=np.float32)
        if ranges.ndim != 2:
            ranges = ranges.reshape(poses.shape[0], -1)
        S, N = ranges.shape
        off = np.ascontiguousarray(yaw_offsets, dtype=np.float64).reshape(-1)
        A = off.shape[0]
        kern = None if kern is None else np.ascontiguousarray(kern, dtype=np.uint8).reshape(-1)
        if kern is not None and 0 <= int(smear_cells) <= 16 and kern.shape[0] < int(smear_cells) ** 2 + 1:
            raise DmError(_ffi.DM_ERR_INVALID_ARG, "kern needs smear_cells**2 + 1 entries")
        T1 = 2 * min(max(int(half), 0), 32) + 1
        best = np.zeros((S, 3), np.int32)
        score = np.zeros(S, np.uint32)
        n_used = np.zeros(S, np.int32)
        pose = np.zeros((S, 3), np.float64)
        vol = np.zeros((S, max(A, 1), T1, T1), np.uint32) if want_volume else None
        with self._lock:
            check(self._lib.dm_match_scans(self._handle(), S, _vp(poses), N, _vp(ranges), float(angle_min),
                                           float(angle_increment), A, _vp(off), int(k0), int(sub), int(half),
                                           int(stride), int(smear_cells), _vp(kern), _vp(best), _vp(score),
                                           _vp(n_used), _vp(pose), _vp(vol)))
        out = {"best": best, "score": score, "n_used": n_used, "pose": pose}
        if want_volume:
            out["volume"] = vol
        return out

    def match_scan(self, scan, pose, slam=None) -> dict:
        """Correct the prior pose (x, y, yaw) of one LaserScan-like message
        against the map: the two-stage search this build derives from
        slam_toolbox's matcher settings (dm.match.search_params documents the
        mapping; `slam`: a SlamParams or None for slam_config.yaml's values),
        each stage one dm_match_scans call.  Returns dm.match.two_stage's
        dict: pose, response = score / (255 * n_used), score, n_used, coarse,
        fine."""
        from . import match

        ranges = np.asarray(scan.ranges, dtype=np.float32)[None, :]
        amin, inc = np.float32(scan.angle_min), np.float32(scan.angle_increment)

        def match_one(p, yaw_offsets, k0, sub, half, stride, smear_cells, kern):
            return match.first_scan(self.match_scans([p], ranges, amin, inc, yaw_offsets, k0, sub, half, stride,
                                                     smear_cells, kern))

        with self._lock:  # both stages against one map
            return match.two_stage_with(match_one, pose, slam, float(self.params.resolution))

    def match_global(self, poses, ranges, angle_min, angle_increment, yaw_offsets, k0: int, half_x: int,
                     half_y: int, smear_cells: int, kern, block: int = 16, exhaustive: bool = False) -> dict:
        """The best pose of S scans over a whole window on the device
        (dm_match_global): dm_match_scans' candidates at sub = 1, stride = 1
        for i in [-half_x, half_x], j in [-half_y, half_y] (up to 4096 each) and
        up to 1024 yaws, found exactly by block bounds (`block` in {4, 8, 16,
        32}) or, with `exhaustive`, by scoring everything.  Returns best int32
        [S, 3] = (k, i, j), score uint32 [S], n_used int32 [S], pose float64
        [S, 3] and stats uint64 [S, 4] = blocks, blocks bounded, blocks
        refined, rounds.  Same results as dm.match.match_global, bit for bit."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        ranges = np.ascontiguousarray(ranges, dtype=np.float32)
        if ranges.ndim != 2:
            ranges = ranges.reshape(poses.shape[0], -1)
        S, N = ranges.shape
        off = np.ascontiguousarray(yaw_offsets, dtype=np.float64).reshape(-1)
        kern = None if kern is None else np.ascontiguousarray(kern, dtype=np.uint8).reshape(-1)
        if kern is not None and 0 <= int(smear_cells) <= 16 and kern.shape[0] < int(smear_cells) ** 2 + 1:
            raise DmError(_ffi.DM_ERR_INVALID_ARG, "kern needs smear_cells**2 + 1 entries")
        best = np.zeros((S, 3), np.int32)
        score = np.zeros(S, np.uint32)
        n_used = np.zeros(S, np.int32)
        pose = np.zeros((S, 3), np.float64)
        stats = np.zeros((S, 4), np.uint64)
        with self._lock:
            check(self._lib.dm_match_global(self._handle(), S, _vp(poses), N, _vp(ranges), float(angle_min),
                                            float(angle_increment), off.shape[0], _vp(off), int(k0), int(half_x),
                                            int(half_y), int(block), int(exhaustive), int(smear_cells), _vp(kern),
                                            _vp(best), _vp(score), _vp(n_used), _vp(pose), _vp(stats)))
        return {"best": best, "score": score, "n_used": n_used, "pose": pose, "stats": stats}

    def match_built(self) -> tuple[np.ndarray, int]:
        """What the matcher's kept fields hold for the map as it is now
        (dm_match_built, a diagnostic): (flags bool [tile rows, tile columns]
        of the response field's built 64 x 64 tiles, the pooled field's built
        tiles).  All zero before the first match and after any map write."""
        TY, TX = -(-self.rows // 64), -(-self.width // 64)
        flags = np.zeros((TY, TX), np.uint8)
        n_field, n_pool = ctypes.c_int64(0), ctypes.c_int64(0)
        with self._lock:
            check(self._lib.dm_match_built(self._handle(), _vp(flags), flags.size, ctypes.byref(n_field),
                                           ctypes.byref(n_pool)))
        return flags.astype(bool), int(n_pool.value)

    def relocalize(self, scan, prior=None, slam=None) -> dict:
        """Find the pose of one LaserScan-like message in the map without a good
        prior: the global stage (dm_match_global with dm.match.global_params'
        reading of slam_toolbox's wide search; the whole map from its centre
        when `prior` is None, +-loop_search_space_dimension / 2 around it
        otherwise), then match_scan's two-stage search from its pose.  Returns
        dm.match.relocalize's dict: pose, global_response and response (score
        / (255 * n_used) of the global and the fine stage), accepted (both reach
        loop_match_minimum_response_coarse / _fine), global, fine, stats."""
        from . import match

        ranges = np.asarray(scan.ranges, dtype=np.float32)[None, :]
        amin, inc = np.float32(scan.angle_min), np.float32(scan.angle_increment)

        def global_one(p, **kw):
            res = self.match_global([p], ranges, amin, inc, **kw)
            one = match.first_scan(res)
            one["stats"] = tuple(int(v) for v in res["stats"][0])
            return one

        with self._lock:  # all stages against one map
            return match.relocalize_with(global_one, lambda p: self.match_scan(scan, p, slam), self.params, prior,
                                         slam)

    # -- frontiers --------------------------------------------------------
    def frontiers(self, want_mask=False, want_labels=False, cap=None) -> Frontiers:
        """Frontier mask / labels (optional dense copies) and the cluster
        list sorted by label.  The cluster buffer is reused across calls and
        grown when the library reports more clusters than it holds."""
        mask = np.empty((self.rows, self.width), np.uint8) if want_mask else None
        labels = np.empty((self.rows, self.width), np.int64) if want_labels else None
        n = ctypes.c_int64(0)
        with self._lock:
            if cap is not None and self._cap < cap:
                self._cap = max(1, int(cap))
            while True:
                # a fresh array per call: the library writes the records straight
                # into it and the caller owns the result (no second copy)
                buf = np.empty(self._cap, dtype=np.dtype(CLUSTER_DTYPE))
                rc = self._lib.dm_frontiers(self._handle(), _vp(mask), _vp(labels), _vp(buf),
                                            buf.shape[0], ctypes.byref(n))
                if rc == _ffi.DM_ERR_CAPACITY and n.value > buf.shape[0]:
                    self._cap = int(n.value) * 2
                    continue
                check(rc)
                break
            clusters = buf[: int(n.value)]
        return Frontiers(clusters=clusters, mask=mask, labels=labels)

    def frontiers_begin(self):
        """Enqueue a clusters-only frontier pass and return at once
        (dm_frontiers_begin); collect it with frontiers_end()."""
        with self._lock:
            check(self._lib.dm_frontiers_begin(self._handle()))

    def frontiers_ready(self) -> bool:
        """True when the oldest frontiers_begin() pass has completed, so
        frontiers_end() returns without waiting (dm_frontiers_poll; never
        blocks)."""
        r = ctypes.c_int32(0)
        with self._lock:
            check(self._lib.dm_frontiers_poll(self._handle(), ctypes.byref(r)))
        return bool(r.value)

    def frontiers_end(self) -> Frontiers | None:
        """Clusters of the pass started by frontiers_begin(), as frontiers()
        would have returned them on the map at that time; None if the pass
        overflowed the library's slot arrays (grown now: call frontiers())."""
        n = ctypes.c_int64(0)
        with self._lock:
            while True:
                buf = np.empty(self._cap, dtype=np.dtype(CLUSTER_DTYPE))
                rc = self._lib.dm_frontiers_end(self._handle(), _vp(buf), buf.shape[0], ctypes.byref(n))
                if rc == _ffi.DM_ERR_CAPACITY and n.value > buf.shape[0]:
                    self._cap = int(n.value) * 2  # the pass stays pending: read it again
                    continue
                if rc == _ffi.DM_ERR_INCOMPLETE:
                    self.last_incomplete = _ffi.last_error()
                    return None
                check(rc)
                return Frontiers(clusters=buf[: int(n.value)])

    def set_overlap(self, on: bool = True):
        """dm_set_overlap: run the integrate front-end beside an in-flight
        frontier pass (results unchanged)."""
        with self._lock:
            check(self._lib.dm_set_overlap(self._handle(), 1 if on else 0))

    # -- sharding support -------------------------------------------------
    def set_halo(self, before=None, after=None):
        b = None if before is None else np.ascontiguousarray(before, np.int8)
        a = None if after is None else np.ascontiguousarray(after, np.int8)
        with self._lock:
            check(self._lib.dm_set_halo(self._handle(), _vp(b), _vp(a)))

    def set_halo_device(self, before_ptr: int | None, after_ptr: int | None):
        with self._lock:
            check(self._lib.dm_set_halo_device(self._handle(),
                                               None if before_ptr is None else ctypes.c_void_p(before_ptr),
                                               None if after_ptr is None else ctypes.c_void_p(after_ptr)))

    def edge_rows(self):
        first = np.empty(self.width, np.int8)
        last = np.empty(self.width, np.int8)
        with self._lock:
            check(self._lib.dm_get_edge_rows(self._handle(), _vp(first), _vp(last)))
        return first, last

    def edge_rows_device(self, first_ptr: int, last_ptr: int):
        with self._lock:
            check(self._lib.dm_get_edge_rows_device(self._handle(), ctypes.c_void_p(first_ptr),
                                                    ctypes.c_void_p(last_ptr)))

    def edge_labels(self):
        first = np.empty(self.width, np.int64)
        last = np.empty(self.width, np.int64)
        with self._lock:
            check(self._lib.dm_get_edge_labels(self._handle(), _vp(first), _vp(last)))
        return first, last

    # -- cross-band exchange (device-resident; dm/sharded.py) --------------
    def export_bytes(self, rec_cap: int) -> int:
        n = ctypes.c_int64(0)
        check(self._lib.dm_export_bytes(self._handle(), int(rec_cap), ctypes.byref(n)))
        return int(n.value)

    def frontiers_export_device(self, d_export_ptr: int, rec_cap: int):
        """Band frontiers + export record into a device buffer of
        export_bytes(rec_cap) bytes; asynchronous, complete on
        exchange_stream() (the pass stream with overlap on)."""
        with self._lock:
            check(self._lib.dm_frontiers_export_device(self._handle(), ctypes.c_void_p(d_export_ptr),
                                                       int(rec_cap)))

    def exchange_stream(self) -> int:
        """hipStream_t (as an int) on which exports are complete and merges
        run (dm_exchange_stream): order the records' all-gather on it."""
        s = ctypes.c_void_p(0)
        with self._lock:
            check(self._lib.dm_exchange_stream(self._handle(), ctypes.byref(s)))
        return int(s.value or 0)

    def merge_bands(self, d_gathered_ptr: int, nranks: int, rec_cap: int, min_size: int):
        """Merge all-gathered export records on the device.  Returns
        (clusters, None) or (None, largest band K) when a band's record was
        incomplete (DM_ERR_INCOMPLETE: rerun with more capacity)."""
        n = ctypes.c_int64(0)
        with self._lock:
            while True:
                buf = self._mbuf if getattr(self, "_mbuf", None) is not None else \
                    np.empty(1 << 14, dtype=np.dtype(CLUSTER_DTYPE))
                rc = self._lib.dm_merge_bands(self._handle(), ctypes.c_void_p(d_gathered_ptr), int(nranks),
                                              int(rec_cap), int(min_size), _vp(buf), buf.shape[0],
                                              ctypes.byref(n))
                self._mbuf = buf
                if rc == _ffi.DM_ERR_INCOMPLETE:
                    self.last_incomplete = _ffi.last_error()
                    return None, int(n.value)
                if rc == _ffi.DM_ERR_CAPACITY and n.value > buf.shape[0]:
                    self._mbuf = np.empty(int(n.value) * 2, dtype=np.dtype(CLUSTER_DTYPE))
                    continue
                check(rc)
                return buf[: int(n.value)].copy(), None

    def merge_max_band_k(self) -> int:
        """Largest band cluster count of the last collected merge."""
        k = ctypes.c_int64(0)
        with self._lock:
            check(self._lib.dm_merge_max_band_k(self._handle(), ctypes.byref(k)))
        return int(k.value)

    def merge_bands_begin(self, d_gathered_ptr: int, nranks: int, rec_cap: int, min_size: int):
        """Enqueue the device merge of gathered export records and return
        (dm_merge_bands_begin); collect it with merge_bands_end()."""
        with self._lock:
            check(self._lib.dm_merge_bands_begin(self._handle(), ctypes.c_void_p(d_gathered_ptr), int(nranks),
                                                 int(rec_cap), int(min_size)))

    def merge_bands_end(self):
        """merge_bands()'s result for the pass started by merge_bands_begin()."""
        n = ctypes.c_int64(0)
        with self._lock:
            while True:
                buf = self._mbuf if getattr(self, "_mbuf", None) is not None else \
                    np.empty(1 << 14, dtype=np.dtype(CLUSTER_DTYPE))
                rc = self._lib.dm_merge_bands_end(self._handle(), _vp(buf), buf.shape[0], ctypes.byref(n))
                self._mbuf = buf
                if rc == _ffi.DM_ERR_INCOMPLETE:
                    self.last_incomplete = _ffi.last_error()
                    return None, int(n.value)
                if rc == _ffi.DM_ERR_CAPACITY and n.value > buf.shape[0]:
                    self._mbuf = np.empty(int(n.value) * 2, dtype=np.dtype(CLUSTER_DTYPE))
                    continue  # the pass stays pending: read it again
                check(rc)
                return buf[: int(n.value)].copy(), None

    # -- checkpoint / streams / profiling ----------------------------------
    def save(self, path: str):
        with self._lock:
            check(self._lib.dm_save(self._handle(), str(path).encode()))

    def load(self, path: str):
        with self._lock:
            check(self._lib.dm_load(self._handle(), str(path).encode()))

    def set_stream(self, stream_ptr: int | None):
        with self._lock:
            check(self._lib.dm_set_stream(self._handle(),
                                          None if not stream_ptr else ctypes.c_void_p(stream_ptr)))

    def synchronize(self):
        with self._lock:
            check(self._lib.dm_synchronize(self._handle()))

    def profile(self, enable: bool = True):
        with self._lock:
            check(self._lib.dm_profile_enable(self._handle(), 1 if enable else 0))

    def profile_read(self) -> dict:
        cap = 64
        arr = (_ffi.DmKernelStat * cap)()
        n = ctypes.c_int32(0)
        with self._lock:
            check(self._lib.dm_profile_read(self._handle(), arr, cap, ctypes.byref(n)))
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms))
                for i in range(min(n.value, cap))}

    def profile_reset(self):
        with self._lock:
            check(self._lib.dm_profile_reset(self._handle()))

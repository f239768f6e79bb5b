#!/usr/bin/env python3
"""Timing of the device path planner (dm_plan_field) on two maps: the
integrated 400^2 world of config C1's size (the smoke world) and a 4096^2
world.  One JSON line per map: the call's statistics, the per-kernel times
(dm_profile_read, over the timed calls), the wall time of plan_field (median
of 20 after 3 warm-ups) and the wall time of the host restatement
dm.plan.field on the same map, the only baseline there is.

With --cost the same two maps also go through dm_plan_clearance and
dm_plan_field_cost (R = 8, Nav2's curve: inflation_table(resolution, 8, 0.05,
10.0)), one more JSON line per map, with k_plan_clear's time beside its byte
model; --parent-lib PATH adds dm_plan_field's times from that build of libdm
(the parent commit's), measured by a child process of this tool on the same
box before this process opens the GPU.

    python tools/plan_timing.py [--out profiles/plan_timing.jsonl] [--cost [--parent-lib PATH]]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "distributed-autonomous-exploration-and-mapping_amd"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import cases  # noqa: E402
import dm  # noqa: E402
from dm import plan  # noqa: E402


def measure(name, p, batches, amin, inc, inflate, n_sources, reps=20, warmup=3, host=True):
    W, H = int(p.width), int(p.height)
    with dm.OccupancyMapper(p) as m:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        sources = [(float(q[0]), float(q[1])) for q in batches[0][0][:n_sources]]  # the robots' first poses
        for _ in range(warmup):
            stats = m.plan_field(sources, inflate_cells=inflate)
        m.profile(True)
        m.profile_reset()
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            stats = m.plan_field(sources, inflate_cells=inflate)
            wall.append(time.perf_counter() - t0)
        prof = m.profile_read()
        m.profile(False)
        st = m.state()
        field = m.plan_cost_field()
    out = {
        "map": name, "width": W, "height": H, "inflate_cells": inflate, "sources": len(sources), "stats": stats,
        "plan_field_wall_ms_median": 1e3 * statistics.median(wall),
        "plan_field_wall_ms_min": 1e3 * min(wall),
        "kernel_ms_per_call": {k: v[1] / reps for k, v in prof.items() if k.startswith("plan_")},
        "kernel_launch_groups_per_call": {k: v[0] / reps for k, v in prof.items() if k.startswith("plan_")},
        # one tile visit moves the tile's costs in, a one-cell ring of costs,
        # 66 x 3 traversable words, and the changed costs out (all 4096 at most)
        "bytes_per_tile_visit_max": 4096 * 4 + (66 * 66 - 4096) * 4 + 66 * 3 * 8 + 4096 * 4,
    }
    k = out["kernel_ms_per_call"]
    out["host_share_of_wall"] = 1.0 - sum(k.values()) / out["plan_field_wall_ms_median"]
    if host:
        src = [plan.cell_of(x, y, p.origin_x, p.origin_y, p.resolution, W, H) for x, y in sources]
        t0 = time.perf_counter()
        ref = plan.field(st, src, inflate)
        out["host_dijkstra_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["equal_to_host"] = bool(np.array_equal(ref, field))
    return out


CLEAR_CELLS = 8


def _timed(call, reps, warmup):
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        wall.append(time.perf_counter() - t0)
    return out, 1e3 * statistics.median(wall), 1e3 * min(wall)


def measure_cost(name, p, batches, amin, inc, inflate, n_sources, reps=20, warmup=3, host=True):
    """dm_plan_field, dm_plan_clearance and dm_plan_field_cost on one map:
    medians as in measure(), kernel times per call from dm_profile_read."""
    W, H = int(p.width), int(p.height)
    pen = plan.inflation_table(float(p.resolution), CLEAR_CELLS, 0.05, 10.0)
    out = {"map": name, "width": W, "height": H, "inflate_cells": inflate, "clear_cells": CLEAR_CELLS,
           "sources": n_sources}
    with dm.OccupancyMapper(p) as m:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        sources = [(float(q[0]), float(q[1])) for q in batches[0][0][:n_sources]]
        m.profile(True)
        for key, call in (("plan_field", lambda: m.plan_field(sources, inflate_cells=inflate)),
                          ("plan_clearance", lambda: m.plan_clearance(CLEAR_CELLS)),
                          ("plan_field_cost", lambda: m.plan_field_cost(sources, inflate, CLEAR_CELLS, pen))):
            for _ in range(warmup):
                call()
            m.profile_reset()
            res, med, lo = _timed(call, reps, 0)
            prof = m.profile_read()
            out[key] = {"wall_ms_median": med, "wall_ms_min": lo,
                        "kernel_ms_per_call": {k: v[1] / reps for k, v in prof.items() if k.startswith("plan_")}}
            if isinstance(res, dict):
                out[key]["stats"] = res
        m.profile(False)
        st = m.state()
        field = m.plan_cost_field()
    # k_plan_clear's byte model: every cell's state once, the halo rows and
    # columns of the 8 neighbour tiles again (a tile reads (64 + 2R)^2 cells),
    # and 2 bytes (dm_plan_clearance) or 1 byte (the penalty form) per cell out
    tiles = -(-W // 64) * -(-H // 64)
    bytes_in = tiles * (64 + 2 * CLEAR_CELLS) ** 2
    for key, per_cell in (("plan_clearance", 2), ("plan_field_cost", 1)):
        ms = out[key]["kernel_ms_per_call"]["plan_clear"]
        nbytes = bytes_in + per_cell * W * H
        out[key]["plan_clear_model_bytes"] = nbytes
        out[key]["plan_clear_GBps_of_model"] = nbytes / (ms * 1e-3) / 1e9
    a, b = out["plan_field"], out["plan_field_cost"]
    out["relax_ms_per_round"] = {"plan_relax": a["kernel_ms_per_call"]["plan_relax"] / a["stats"]["rounds"],
                                 "plan_relax_w": b["kernel_ms_per_call"]["plan_relax_w"] / b["stats"]["rounds"]}
    if host:
        src = [plan.cell_of(x, y, p.origin_x, p.origin_y, p.resolution, W, H) for x, y in sources]
        t0 = time.perf_counter()
        ref = plan.field_cost(st, src, inflate, CLEAR_CELLS, pen)
        out["host_dijkstra_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["equal_to_host"] = bool(np.array_equal(ref, field))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--no-host", action="store_true", help="skip the host Dijkstra baseline")
    ap.add_argument("--cost", action="store_true", help="measure dm_plan_clearance and dm_plan_field_cost too")
    ap.add_argument("--parent-lib", default=None, help="with --cost: a libdm.so of the parent commit to time "
                    "dm_plan_field with, beside this build's")
    ap.add_argument("--field-only", action="store_true", help=argparse.SUPPRESS)  # the --parent-lib child
    args = ap.parse_args()
    if args.field_only:  # an older libdm: bind only what it exports
        from dm import _ffi

        for name in ("dm_plan_clearance", "dm_plan_field_cost"):
            _ffi.SIGNATURES.pop(name, None)
    parent = {}
    if args.cost and args.parent_lib:
        got = subprocess.run([sys.executable, os.path.abspath(__file__), "--field-only", "--no-host"],
                             env={**os.environ, "DM_LIB": os.path.abspath(args.parent_lib)}, check=True,
                             capture_output=True, text=True, timeout=600).stdout
        for ln in got.splitlines():
            rec = json.loads(ln)
            parent[rec["map"]] = {k: rec[k] for k in ("stats", "plan_field_wall_ms_median", "plan_field_wall_ms_min",
                                                      "kernel_ms_per_call")}
    for name, world, n_sources in (("world 400^2 (4 batches of 2 scans)", (3, 400, 400, 0.05, 2, 360, 4), 1),
                                   ("world 4096^2 (4 batches of 16 scans)", (11, 4096, 4096, 0.05, 16, 1440, 4), 16)):
        p, batches, amin, inc = cases.world_case(*world)
        if args.cost:
            rec = measure_cost(name, p, batches, amin, inc, 2, n_sources, host=not args.no_host)
            if name in parent:
                rec["parent_plan_field"] = parent[name]
        else:
            rec = measure(name, p, batches, amin, inc, 2, n_sources, host=not args.no_host)
        ln = json.dumps(rec)
        print(ln, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(ln + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the device scan matcher (dm_match_scans) at the reference's
matcher settings (slam_config.yaml:50-53, 64-66): the two-stage match of
450-beam scans against an integrated 400^2 map, for S = 1 and S = 32 scans per
call.  One JSON line per S: the device wall time of both stages (median of 30
after 5 warm-ups; the first timed call of each repetition follows a map
touch, so the response field is rebuilt every time, as after an integrate),
the per-kernel times (dm_profile_read over the timed calls, a separate pass
so the events do not sit in the wall time), and the wall time of the host
restatement dm.match on the same inputs: the only baseline there is.

    python tools/match_timing.py [--out profiles/match_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "distributed-autonomous-exploration-and-mapping_amd"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import cases  # noqa: E402
import dm  # noqa: E402
from dm import match  # noqa: E402


def two_stage_batch(m, sp, poses, ranges, amin, inc):
    """Both stages for S scans in two dm_match_scans calls."""
    common = dict(sub=sp["sub"], smear_cells=sp["smear_cells"], kern=sp["kern"])
    c = m.match_scans(poses, ranges, amin, inc, **sp["coarse"], **common)
    return m.match_scans(c["pose"], ranges, amin, inc, **sp["fine"], **common)


def host_two_stage_batch(st, p, sp, poses, ranges, amin, inc):
    V = match.response_field(st, sp["smear_cells"], sp["kern"])
    common = dict(sub=sp["sub"], smear_cells=sp["smear_cells"], kern=sp["kern"], field=V)
    c = match.match_scans(st, p, poses, ranges, amin, inc, **sp["coarse"], **common)
    return match.match_scans(st, p, c["pose"], ranges, amin, inc, **sp["fine"], **common)


def measure(S, reps=30, warmup=5, host=True):
    p, batches, amin, inc = cases.world_case(3, 400, 400, 0.05, S, 450, 3)
    sp = match.search_params(None, float(p.resolution))
    rng = np.random.default_rng(S)
    with dm.OccupancyMapper(p) as m:
        for poses, ranges in batches:
            m.integrate(poses, ranges, amin, inc)
        st = m.state()
        poses, ranges = batches[-1]
        prior = poses + np.stack([rng.uniform(-0.08, 0.08, S), rng.uniform(-0.08, 0.08, S),
                                  rng.uniform(-0.05, 0.05, S)], axis=1)

        def touch():  # a new map version without a new map: the field is dropped
            m.set_state(st)

        for _ in range(warmup):
            touch()
            got = two_stage_batch(m, sp, prior, ranges, amin, inc)
        wall, wall_kept = [], []
        for _ in range(reps):
            touch()
            m.synchronize()
            t0 = time.perf_counter()
            got = two_stage_batch(m, sp, prior, ranges, amin, inc)
            wall.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            two_stage_batch(m, sp, prior, ranges, amin, inc)  # same map: the kept field
            wall_kept.append(time.perf_counter() - t0)
        m.profile(True)
        m.profile_reset()
        for _ in range(reps):
            touch()
            two_stage_batch(m, sp, prior, ranges, amin, inc)
        prof = m.profile_read()
        m.profile(False)
    err0 = np.hypot(*(prior[:, :2] - poses[:, :2]).T)
    err1 = np.hypot(*(got["pose"][:, :2] - poses[:, :2]).T)
    out = {
        "what": "two-stage match, reference settings", "S": S, "beams": 450, "width": 400, "height": 400,
        "sub": sp["sub"], "smear_cells": sp["smear_cells"],
        "coarse": {k: (len(v) if k == "yaw_offsets" else v) for k, v in sp["coarse"].items()},
        "fine": {k: (len(v) if k == "yaw_offsets" else v) for k, v in sp["fine"].items()},
        "device_wall_ms_median": 1e3 * statistics.median(wall),
        "device_wall_ms_min": 1e3 * min(wall),
        "device_wall_ms_median_field_kept": 1e3 * statistics.median(wall_kept),
        "kernel_ms_per_match": {k: v[1] / reps for k, v in prof.items() if k.startswith("match_")},
        "kernel_launches_per_match": {k: v[0] / reps for k, v in prof.items() if k.startswith("match_")},
        "median_translation_error_m": {"prior": float(np.median(err0)), "matched": float(np.median(err1))},
    }
    if host:
        t0 = time.perf_counter()
        exp = host_two_stage_batch(st, p, sp, prior, ranges, amin, inc)
        out["host_restatement_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["equal_to_host"] = bool(np.array_equal(exp["best"], got["best"]) and
                                    exp["pose"].tobytes() == got["pose"].tobytes() and
                                    np.array_equal(exp["score"], got["score"]))
        out["speedup_over_host"] = out["host_restatement_wall_ms"] / out["device_wall_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement baseline")
    args = ap.parse_args()
    for S in (1, 32):
        ln = json.dumps(measure(S, host=not args.no_host))
        print(ln, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(ln + "\n")


if __name__ == "__main__":
    main()

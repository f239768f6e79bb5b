"""Correlative scan matching on the occupancy grid: host restatement and test
reference of dm_match_field and dm_match_scans (csrc/dm_match.h), as
dm/plan.py is for dm_plan_*.

In the reference the pose of every scan comes from slam_toolbox, whose
correlative scan matcher corrects odometry (server/thymio_project/config/
slam_config.yaml:35 ``use_scan_matching``, :50-53 and :64-66 its settings).
slam_toolbox is not vendored, so there is no reference behaviour to pin: the
definitions are this build's SPEC (include/dm.h).  They use
integers and separately rounded doubles only, so the results are unique:

* response field ``V[c]``: the maximum of ``kern[d2]`` over the in-grid
  occupied cells within ``d2 = dx*dx + dy*dy <= r*r`` of ``c``, 0 if none;
* fine coordinates ``(qx, qy) = floor((endpoint - origin) / step)`` with
  ``step = resolution / sub`` of every used beam (``range_min <= r <=
  range_max``) for every candidate yaw ``yaw + yaw_offsets[k]``;
* ``score[s][k][j][i]``: the sum over used beams of ``V`` at the cell
  ``(floordiv(qx + i*stride, sub), floordiv(qy + j*stride, sub))``;
* best candidate: maximal score, ties to the least
  ``(i*i + j*j, |k - k0|, k, j, i)``.

The trigonometry is ``math.cos`` / ``math.sin`` per value (the C library, as
``synth.pose4``), everything else NumPy float64 / int64 element-wise, which
rounds every operation separately like the device code compiled without FMA
contraction.

``match_global`` restates dm_match_global (csrc/dm_match_global.h): the same
score at sub = 1, stride = 1 over a window of up to 8193 x 8193 translations
and 1024 yaws, as the exhaustive search that defines its result;
``global_params`` and ``relocalize`` are this build's reading of
slam_toolbox's wide search (slam_config.yaml:47-48, 56-58).

``two_stage`` is the coarse-then-fine search this build derives from the
reference's slam_config.yaml; the wrapper (``OccupancyMapper.match_scan``)
runs the same driver over the device calls.
"""
from __future__ import annotations

import math

import numpy as np

MAX_SMEAR = 16
MAX_ANGLES = 64
MAX_HALF = 32
LIMIT = 2 ** 30

# slam_config.yaml's matcher settings (line numbers there); SlamParams
# (dm/ros_node.py) carries the same names and defaults
MATCHER_DEFAULTS = {
    "correlation_search_space_dimension": 0.5,         # :51
    "correlation_search_space_resolution": 0.01,       # :52
    "correlation_search_space_smear_deviation": 0.1,   # :53
    "fine_search_angle_offset": 0.00349,               # :64
    "coarse_search_angle_offset": 0.349,               # :65
    "coarse_angle_resolution": 0.0349,                 # :66
}


def kernel_table(sigma_m: float, resolution: float, r: int) -> np.ndarray:
    """uint8 [r*r + 1]: kern[d2] = floor(255 * exp(-0.5 * d2 * res^2 / sigma^2) + 0.5),
    a Gaussian smear of deviation sigma_m metres sampled at squared cell
    distances.  The library computes no exp: its callers pass this table."""
    r = int(r)
    if not 0 <= r <= MAX_SMEAR:
        raise ValueError("smear_cells must be in [0, 16]")
    res, sigma = float(resolution), float(sigma_m)
    out = np.empty(r * r + 1, np.uint8)
    for d2 in range(r * r + 1):
        out[d2] = int(math.floor(255.0 * math.exp(-0.5 * d2 * res * res / (sigma * sigma)) + 0.5))
    return out


def _check_table(r: int, kern) -> np.ndarray:
    r = int(r)
    if not 0 <= r <= MAX_SMEAR:
        raise ValueError("smear_cells must be in [0, 16]")
    kern = np.ascontiguousarray(kern, dtype=np.uint8).reshape(-1)
    if kern.shape[0] < r * r + 1:
        raise ValueError("kern must have r*r + 1 entries")
    return kern


def _shifted(a: np.ndarray, dy: int, dx: int) -> np.ndarray:
    """out[y, x] = a[y + dy, x + dx], False outside the grid."""
    H, W = a.shape
    out = np.zeros_like(a)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def response_field(state, r: int, kern) -> np.ndarray:
    """uint8 [H, W]: V[c] = max of kern[d2] over the occupied cells within the
    disc of radius r around c (any table, monotone or not)."""
    kern = _check_table(r, kern)
    r = int(r)
    occ = np.asarray(state) == 100
    V = np.zeros(occ.shape, np.uint8)
    if occ.any():
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                d2 = dx * dx + dy * dy
                if d2 <= r * r and kern[d2]:
                    np.maximum(V, np.where(_shifted(occ, dy, dx), kern[d2], np.uint8(0)), out=V)
    return V


def _cos_sin(a: float):
    """The C library's cos / sin; NaN for a non-finite angle, as C gives."""
    if not math.isfinite(a):
        return math.nan, math.nan
    return math.cos(a), math.sin(a)


def fine_coords(params, poses, ranges, angle_min, angle_increment, yaw_offsets, sub: int):
    """(qx, qy, used): int64, int64, bool [S, A, N].  params: resolution,
    origin_x, origin_y, range_min, range_max (a DmParams)."""
    sub = int(sub)
    if not 1 <= sub <= 16:
        raise ValueError("sub must be in [1, 16]")
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    S = poses.shape[0]
    r32 = np.asarray(ranges, np.float32).reshape(S, -1)
    N = r32.shape[1]
    off = np.asarray(yaw_offsets, np.float64).reshape(-1)
    A = off.shape[0]
    ox, oy = float(params.origin_x), float(params.origin_y)
    step = float(params.resolution) / float(sub)
    amin, inc = float(np.float32(angle_min)), float(np.float32(angle_increment))
    phi = [amin + float(i) * inc for i in range(N)]
    cphi = np.array([math.cos(v) for v in phi], np.float64)
    sphi = np.array([math.sin(v) for v in phi], np.float64)
    with np.errstate(invalid="ignore"):
        in_range = (r32 >= np.float32(params.range_min)) & (r32 <= np.float32(params.range_max))
    rr = r32.astype(np.float64)
    qx = np.zeros((S, A, N), np.int64)
    qy = np.zeros((S, A, N), np.int64)
    used = np.zeros((S, A, N), bool)
    for s in range(S):
        x, y, yaw = (float(v) for v in poses[s])
        for k in range(A):
            cyaw, syaw = _cos_sin(yaw + float(off[k]))
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(cyaw) and math.isfinite(syaw)):
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                a1 = cyaw * cphi
                a2 = syaw * sphi
                dcx = a1 - a2
                b1 = syaw * cphi
                b2 = cyaw * sphi
                dcy = b1 + b2
                t1 = rr[s] * dcx
                ex = x + t1
                t2 = rr[s] * dcy
                ey = y + t2
                fx = np.floor((ex - ox) / step)
                fy = np.floor((ey - oy) / step)
                ok = in_range[s] & (np.abs(fx) < float(LIMIT)) & (np.abs(fy) < float(LIMIT))
            used[s, k] = ok
            qx[s, k] = np.where(ok, fx, 0.0).astype(np.int64)
            qy[s, k] = np.where(ok, fy, 0.0).astype(np.int64)
    return qx, qy, used


def score_volume(V, qx, qy, used, sub: int, half: int, stride: int) -> np.ndarray:
    """uint32 [S, A, 2*half + 1, 2*half + 1], index order k, j, i."""
    sub, half, stride = int(sub), int(half), int(stride)
    if not 1 <= sub <= 16:
        raise ValueError("sub must be in [1, 16]")
    if not 0 <= half <= MAX_HALF:
        raise ValueError("half must be in [0, 32]")
    if not 1 <= stride <= 16:
        raise ValueError("stride must be in [1, 16]")
    V = np.asarray(V, np.uint8)
    H, W = V.shape
    S, A, _ = qx.shape
    T1 = 2 * half + 1
    d = np.arange(-half, half + 1, dtype=np.int64) * stride
    vol = np.zeros((S, A, T1, T1), np.uint32)
    for s in range(S):
        for k in range(A):
            u = used[s, k]
            x, y = qx[s, k][u], qy[s, k][u]
            acc = np.zeros((T1, T1), np.uint64)
            for b0 in range(0, x.shape[0], 256):
                cx = (x[b0:b0 + 256, None] + d[None, :]) // sub  # floor division
                cy = (y[b0:b0 + 256, None] + d[None, :]) // sub
                okx = (cx >= 0) & (cx < W)
                oky = (cy >= 0) & (cy < H)
                vals = V[np.clip(cy, 0, H - 1)[:, :, None], np.clip(cx, 0, W - 1)[:, None, :]]
                vals = np.where(oky[:, :, None] & okx[:, None, :], vals, np.uint8(0))
                acc += vals.sum(axis=0, dtype=np.uint64)
            vol[s, k] = acc.astype(np.uint32)
    return vol


def best(volume_s, k0: int, half: int):
    """(k, i, j, score) of one scan's volume [A, T1, T1]: the maximal score,
    ties to the least (i*i + j*j, |k - k0|, k, j, i)."""
    vol = np.asarray(volume_s)
    mx = vol.max()
    ks, js, is_ = np.nonzero(vol == mx)
    i, j = is_.astype(np.int64) - half, js.astype(np.int64) - half
    order = np.lexsort((i, j, ks, np.abs(ks - int(k0)), i * i + j * j))  # last key first
    n = order[0]
    return int(ks[n]), int(i[n]), int(j[n]), int(mx)


def match_scans(state, params, poses, ranges, angle_min, angle_increment, yaw_offsets, k0: int, sub: int,
                half: int, stride: int, smear_cells: int, kern, field=None) -> dict:
    """dm_match_scans restated: best int32 [S, 3] = (k, i, j), score uint32
    [S], n_used int32 [S], pose float64 [S, 3], volume uint32 [S, A, T1, T1].
    `field`: the response field of (state, smear_cells, kern) if the caller
    has it already."""
    off = np.asarray(yaw_offsets, np.float64).reshape(-1)
    A = off.shape[0]
    if not 1 <= A <= MAX_ANGLES:
        raise ValueError("A must be in [1, 64]")
    if not 0 <= int(k0) < A:
        raise ValueError("k0 must be in [0, A)")
    V = response_field(state, smear_cells, kern) if field is None else np.asarray(field, np.uint8)
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    S = poses.shape[0]
    qx, qy, used = fine_coords(params, poses, ranges, angle_min, angle_increment, off, sub)
    vol = score_volume(V, qx, qy, used, sub, half, stride)
    step = float(params.resolution) / float(int(sub))
    out_best = np.zeros((S, 3), np.int32)
    out_score = np.zeros(S, np.uint32)
    out_pose = np.zeros((S, 3), np.float64)
    for s in range(S):
        k, i, j, sc = best(vol[s], k0, int(half))
        out_best[s] = (k, i, j)
        out_score[s] = sc
        out_pose[s] = (poses[s, 0] + float(i * int(stride)) * step, poses[s, 1] + float(j * int(stride)) * step,
                       poses[s, 2] + off[k])
    return {"best": out_best, "score": out_score, "n_used": used[:, int(k0), :].sum(axis=1).astype(np.int32),
            "pose": out_pose, "volume": vol}


# -- whole-window relocalisation (dm_match_global) ---------------------------------
MAX_GLOBAL_ANGLES = 1024
MAX_GLOBAL_HALF = 4096

# slam_config.yaml's wide-search settings (line numbers there)
GLOBAL_DEFAULTS = {
    "loop_search_space_dimension": 8.0,            # :56
    "loop_search_space_smear_deviation": 0.03,     # :58
    "loop_match_minimum_response_coarse": 0.35,    # :47
    "loop_match_minimum_response_fine": 0.45,      # :48
    "coarse_angle_resolution": 0.0349,             # :66
}


def match_global(state, params, poses, ranges, angle_min, angle_increment, yaw_offsets, k0: int, half_x: int,
                 half_y: int, smear_cells: int, kern, field=None) -> dict:
    """dm_match_global restated as the exhaustive search: dm_match_scans'
    definition at sub = 1, stride = 1 over i in [-half_x, half_x], j in
    [-half_y, half_y].  best int32 [S, 3] = (k, i, j), score uint32 [S], n_used
    int32 [S], pose float64 [S, 3].  Per yaw and used beam the window
    V[qy - half_y : qy + half_y + 1, qx - half_x : qx + half_x + 1] (0 out of the
    grid) is added to the yaw's score plane; no volume is kept."""
    off = np.asarray(yaw_offsets, np.float64).reshape(-1)
    A = off.shape[0]
    k0, hx, hy = int(k0), int(half_x), int(half_y)
    if not 1 <= A <= MAX_GLOBAL_ANGLES:
        raise ValueError("A must be in [1, 1024]")
    if not 0 <= k0 < A:
        raise ValueError("k0 must be in [0, A)")
    if not (0 <= hx <= MAX_GLOBAL_HALF and 0 <= hy <= MAX_GLOBAL_HALF):
        raise ValueError("half_x and half_y must be in [0, 4096]")
    V = response_field(state, smear_cells, kern) if field is None else np.asarray(field, np.uint8)
    H, W = V.shape
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    S = poses.shape[0]
    qx, qy, used = fine_coords(params, poses, ranges, angle_min, angle_increment, off, 1)
    res = float(params.resolution)
    jj, ii = np.mgrid[-hy:hy + 1, -hx:hx + 1].astype(np.int64)
    # the tie tuple's (i*i + j*j, j, i) of one yaw as one integer
    key = ((ii * ii + jj * jj) << 28) | ((jj + hy) << 14) | (ii + hx)
    far = np.int64(2 ** 62)
    out_best = np.zeros((S, 3), np.int32)
    out_score = np.zeros(S, np.uint32)
    out_pose = np.zeros((S, 3), np.float64)
    empty = not V.any()
    for s in range(S):
        top = (0, (0, 0, k0, 0, 0))  # score, tie tuple: stands when nothing scores above 0
        for k in range(A if not empty else 0):
            u = used[s, k]
            if not u.any():
                continue
            acc = np.zeros((2 * hy + 1, 2 * hx + 1), np.uint32)
            for x, y in zip(qx[s, k][u].tolist(), qy[s, k][u].tolist()):
                x0, x1 = max(x - hx, 0), min(x + hx + 1, W)
                y0, y1 = max(y - hy, 0), min(y + hy + 1, H)
                if x0 < x1 and y0 < y1:
                    acc[y0 - (y - hy):y1 - (y - hy), x0 - (x - hx):x1 - (x - hx)] += V[y0:y1, x0:x1]
            mx = int(acc.max())
            if mx == 0 or mx < top[0]:
                continue
            kk = int(np.where(acc == mx, key, far).min())
            i, j = (kk & 0x3FFF) - hx, ((kk >> 14) & 0x3FFF) - hy
            cand = (i * i + j * j, abs(k - k0), k, j, i)
            if mx > top[0] or cand < top[1]:
                top = (mx, cand)
        sc, (_, _, k, j, i) = top
        out_best[s] = (k, i, j)
        out_score[s] = sc
        out_pose[s] = (poses[s, 0] + float(i) * res, poses[s, 1] + float(j) * res, poses[s, 2] + off[k])
    return {"best": out_best, "score": out_score, "n_used": used[:, k0, :].sum(axis=1).astype(np.int32),
            "pose": out_pose}


def global_params(slam, resolution: float, width: int, height: int, prior=None) -> dict:
    """This build's reading of slam_toolbox's wide search (`slam` as for
    search_params; missing names take the yaml's values):

    * yaw candidates over the full circle in steps of coarse_angle_resolution:
      n = floor(2 pi / step) of them (the 1e-9 tolerance of _symmetric_offsets
      on the count; 180 at 0.0349), offsets (m - n // 2) * step, k0 = n // 2 the
      zero offset; at most 1024;
    * sigma = loop_search_space_smear_deviation, smear_cells = min(16,
      ceil(2 sigma / resolution));
    * without a prior the window is the whole map from its centre: half_x =
      ceil(width / 2), half_y = ceil(height / 2); with one it is
      +-loop_search_space_dimension / 2 in cells;
    * block 16."""
    g = {k: float(getattr(slam, k, v)) for k, v in GLOBAL_DEFAULTS.items()}
    res = float(resolution)
    step = g["coarse_angle_resolution"]
    n = int(math.floor(2.0 * math.pi / step + 1e-9)) if step > 0.0 else 1
    n = min(max(n, 1), MAX_GLOBAL_ANGLES)
    k0 = n // 2
    sigma = g["loop_search_space_smear_deviation"]
    r = min(MAX_SMEAR, max(0, int(math.ceil(2.0 * sigma / res))))
    if prior is None:
        hx, hy = (int(width) + 1) // 2, (int(height) + 1) // 2
    else:
        hx = hy = int(math.ceil(g["loop_search_space_dimension"] / 2.0 / res - 1e-9))
    return {"yaw_offsets": np.array([(m - k0) * step for m in range(n)], np.float64), "k0": k0,
            "half_x": min(max(hx, 0), MAX_GLOBAL_HALF), "half_y": min(max(hy, 0), MAX_GLOBAL_HALF),
            "smear_cells": r, "kern": kernel_table(sigma, res, r) if sigma > 0.0 else np.array([255], np.uint8),
            "block": 16}


def relocalize_with(global_one, fine_two_stage, params, prior, slam) -> dict:
    """The relocalisation driver over any global matcher and two-stage matcher:
    global_one(pose, **global search) -> one scan's {"best", "score", "n_used",
    "pose"[, "stats"]}; fine_two_stage(pose) -> two_stage's dict.  The global
    stage runs from `prior` (None: the map's centre, yaw 0, the whole map),
    the two-stage search from its pose.  accepted: the global response >=
    loop_match_minimum_response_coarse and the fine one >=
    loop_match_minimum_response_fine."""
    gp = global_params(slam, float(params.resolution), int(params.width), int(params.height), prior)
    if prior is None:
        res = float(params.resolution)
        start = (float(params.origin_x) + 0.5 * float(int(params.width)) * res,
                 float(params.origin_y) + 0.5 * float(int(params.height)) * res, 0.0)
    else:
        start = tuple(float(v) for v in prior)
    glob = global_one(start, **gp)
    n, score = int(glob["n_used"]), int(glob["score"])
    g_resp = score / (255.0 * n) if n > 0 else 0.0
    fine = fine_two_stage(tuple(float(v) for v in glob["pose"]))
    lo_c = float(getattr(slam, "loop_match_minimum_response_coarse", GLOBAL_DEFAULTS["loop_match_minimum_response_coarse"]))
    lo_f = float(getattr(slam, "loop_match_minimum_response_fine", GLOBAL_DEFAULTS["loop_match_minimum_response_fine"]))
    return {"pose": tuple(float(v) for v in fine["pose"]), "global_response": g_resp,
            "response": float(fine["response"]), "accepted": bool(g_resp >= lo_c and fine["response"] >= lo_f),
            "global": glob, "fine": fine, "stats": glob.get("stats")}


def relocalize(state, params, ranges, angle_min, angle_increment, prior=None, slam=None) -> dict:
    """relocalize_with over the host restatement (OccupancyMapper.relocalize's
    reference)."""
    r1 = np.asarray(ranges, np.float32).reshape(1, -1)

    def global_one(p, yaw_offsets, k0, half_x, half_y, smear_cells, kern, block):
        return first_scan(match_global(state, params, [p], r1, angle_min, angle_increment, yaw_offsets, k0, half_x,
                                       half_y, smear_cells, kern))

    return relocalize_with(global_one, lambda p: two_stage(state, params, r1[0], angle_min, angle_increment, p, slam),
                           params, prior, slam)


# -- the two-stage search of this build --------------------------------------------
def _symmetric_offsets(step: float, limit: float) -> tuple[np.ndarray, int]:
    """m * step for |m * step| <= limit (a 1e-9 tolerance on the count: 0.349 /
    0.0349 must give 10, not 9), at most 63 of them; and the index of 0."""
    m = int(math.floor(limit / step + 1e-9)) if step > 0.0 and limit > 0.0 else 0
    m = min(max(m, 0), (MAX_ANGLES - 1) // 2)
    return np.array([i * step for i in range(-m, m + 1)], np.float64), m


def search_params(slam, resolution: float) -> dict:
    """The two one-stage searches derived from slam_toolbox's settings (`slam`:
    any object with the names of MATCHER_DEFAULTS, e.g. SlamParams; missing
    ones take the yaml's values).  This mapping is this build's choice:

    * sub = round(resolution / correlation_search_space_resolution) in [1, 16];
    * sigma = correlation_search_space_smear_deviation,
      smear_cells = min(16, ceil(2 sigma / resolution));
    * coarse: angles m * coarse_angle_resolution within
      +-coarse_search_angle_offset, stride 2,
      half = floor((correlation_search_space_dimension / 2 / step) / 2);
    * fine, around the coarse result: angles m * fine_search_angle_offset within
      +-coarse_angle_resolution / 2, stride 1, half 2."""
    g = {k: float(getattr(slam, k, v)) for k, v in MATCHER_DEFAULTS.items()}
    res = float(resolution)
    sub = min(max(int(round(res / g["correlation_search_space_resolution"])), 1), 16)
    step = res / float(sub)
    sigma = g["correlation_search_space_smear_deviation"]
    r = min(MAX_SMEAR, max(0, int(math.ceil(2.0 * sigma / res))))
    c_off, c_k0 = _symmetric_offsets(g["coarse_angle_resolution"], g["coarse_search_angle_offset"])
    f_off, f_k0 = _symmetric_offsets(g["fine_search_angle_offset"], g["coarse_angle_resolution"] / 2.0)
    c_half = int(math.floor((g["correlation_search_space_dimension"] / 2.0 / step) / 2.0 + 1e-9))
    return {
        "sub": sub, "step": step, "smear_cells": r, "kern": kernel_table(sigma, res, r),
        "coarse": {"yaw_offsets": c_off, "k0": c_k0, "half": min(max(c_half, 0), MAX_HALF), "stride": 2},
        "fine": {"yaw_offsets": f_off, "k0": f_k0, "half": 2, "stride": 1},
    }


def two_stage_with(match_one, pose, slam, resolution: float) -> dict:
    """The coarse-then-fine driver over any one-stage matcher:
    match_one(pose, yaw_offsets, k0, sub, half, stride, smear_cells, kern) ->
    {"best": (k, i, j), "score", "n_used", "pose": (x, y, yaw)} of one scan.
    Returns pose (x, y, yaw), response = score / (255 * n_used) of the fine
    stage (0 if no beam was used), score, n_used and both stages' results."""
    sp = search_params(slam, resolution)
    common = {"sub": sp["sub"], "smear_cells": sp["smear_cells"], "kern": sp["kern"]}
    coarse = match_one(tuple(float(v) for v in pose), **sp["coarse"], **common)
    fine = match_one(tuple(float(v) for v in coarse["pose"]), **sp["fine"], **common)
    n, score = int(fine["n_used"]), int(fine["score"])
    return {"pose": tuple(float(v) for v in fine["pose"]), "response": score / (255.0 * n) if n > 0 else 0.0,
            "score": score, "n_used": n, "coarse": coarse, "fine": fine}


def first_scan(res: dict) -> dict:
    """One scan's entries of a match_scans result with S = 1."""
    return {"best": tuple(int(v) for v in res["best"][0]), "score": int(res["score"][0]),
            "n_used": int(res["n_used"][0]), "pose": tuple(float(v) for v in res["pose"][0])}


def two_stage(state, params, ranges, angle_min, angle_increment, pose, slam=None) -> dict:
    """two_stage_with over the host restatement: match one scan (ranges [N])
    at the prior `pose` against the map `state`."""
    sp = search_params(slam, float(params.resolution))
    V = response_field(state, sp["smear_cells"], sp["kern"])
    r1 = np.asarray(ranges, np.float32).reshape(1, -1)

    def match_one(p, yaw_offsets, k0, sub, half, stride, smear_cells, kern):
        return first_scan(match_scans(state, params, [p], r1, angle_min, angle_increment, yaw_offsets, k0, sub, half,
                                      stride, smear_cells, kern, field=V))

    return two_stage_with(match_one, pose, slam, float(params.resolution))

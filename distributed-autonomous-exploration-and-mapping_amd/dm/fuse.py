"""Host restatement of map fusion (include/dm.h: dm_fuse_logodds,
dm_fuse_state, dm_fuse_grid) in NumPy: the same operations in the same order,
float64 geometry and a float32 add, so the device results equal these bit for
bit.  This is the definition the GPU tests compare against; the product path
is the HIP kernel (csrc/dm_fuse.hip), never this module.
"""
from __future__ import annotations

import math

import numpy as np

FUSE_ADD = 0
FUSE_FILL = 1
MODES = {"add": FUSE_ADD, "fill": FUSE_FILL}


def mode_code(mode) -> int:
    """"add" / "fill" (or DM_FUSE_ADD / DM_FUSE_FILL) -> the C constant."""
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"unknown fuse mode {mode!r}")
        return MODES[mode]
    return int(mode)


def geom_of(params) -> dict:
    """The dm_fuse_source geometry of a map with these dm_params."""
    return {"width": int(params.width), "height": int(params.height), "resolution": float(params.resolution),
            "origin_x": float(params.origin_x), "origin_y": float(params.origin_y)}


def _geom(src_geom) -> dict:
    if isinstance(src_geom, dict):
        return src_geom
    return geom_of(src_geom)


def _pz(v) -> np.float32:
    """A zero bound or threshold reads as +0 (include/dm.h, dm_params)."""
    v = np.float32(v)
    return np.float32(0.0) if v == 0 else v


def state_of(L, params) -> np.ndarray:
    """SPEC a7: L == 0 -> -1, else L >= occ_thresh -> 100, else L <= free_thresh -> 0, else -1."""
    L = np.asarray(L, np.float32)
    st = np.full(L.shape, -1, np.int8)
    st[L <= _pz(params.free_thresh)] = 0
    st[L >= _pz(params.occ_thresh)] = 100
    st[L == 0] = -1
    return st


def source_cells(dst_params, rows: int, src_geom, transform, cs=None):
    """(covered bool [rows, W], qx int64, qy int64): the source cell under the
    centre of every destination cell of the handle's rows (band_row0 on)."""
    g = _geom(src_geom)
    tx, ty, yaw = (float(v) for v in transform)
    c, s = (math.cos(yaw), math.sin(yaw)) if cs is None else (float(cs[0]), float(cs[1]))
    W = int(dst_params.width)
    res = float(dst_params.resolution)
    cx = np.arange(W, dtype=np.float64)[None, :]
    cy = (np.arange(rows, dtype=np.float64) + float(int(dst_params.band_row0)))[:, None]
    wx = float(dst_params.origin_x) + (cx + 0.5) * res
    wy = float(dst_params.origin_y) + (cy + 0.5) * res
    dx = wx - tx
    dy = wy - ty
    with np.errstate(all="ignore"):
        sx = c * dx + s * dy
        sy = c * dy - s * dx
        qx = np.floor((sx - float(g["origin_x"])) / float(g["resolution"]))
        qy = np.floor((sy - float(g["origin_y"])) / float(g["resolution"]))
        cov = (np.isfinite(sx) & np.isfinite(sy) & (qx >= 0.0) & (qx < float(int(g["width"])))
               & (qy >= 0.0) & (qy < float(int(g["height"]))))
    qxi = np.where(cov, qx, 0.0).astype(np.int64)
    qyi = np.where(cov, qy, 0.0).astype(np.int64)
    return cov, qxi, qyi


def fuse_map(L_dst, dst_params, src_values, src_geom, transform, mode, *, src_is_state=False, cs=None):
    """Fuse a source map into the destination log-odds `L_dst` (float32
    [rows, W], the rows of dst_params' band).  src_values: the source's
    log-odds (float32 [h, w]) or, with src_is_state, its int8 state image;
    src_geom: a dict width / height / resolution / origin_x / origin_y (or
    dm_params); transform: (tx, ty, yaw), source frame -> destination frame;
    mode: "add" / "fill".  cs = (c, s) overrides cos / sin of the yaw (exact
    quarter turns).  Returns (L', state', stats) with stats = {"covered",
    "contributing", "changed"}."""
    g = _geom(src_geom)
    fill = mode_code(mode) == FUSE_FILL
    if mode_code(mode) not in (FUSE_ADD, FUSE_FILL):
        raise ValueError(f"unknown fuse mode {mode!r}")
    L = np.array(L_dst, dtype=np.float32, copy=True)
    rows, W = L.shape
    sh, sw = int(g["height"]), int(g["width"])
    if src_is_state:
        sv = np.asarray(src_values, np.int8).reshape(sh, sw)
        lsrc = np.zeros((sh, sw), np.float32)
        lsrc[sv == 100] = np.float32(dst_params.l_occ)
        lsrc[sv == 0] = np.float32(dst_params.l_free)
    else:
        lsrc = np.array(src_values, dtype=np.float32, copy=True).reshape(sh, sw)
        lsrc[~np.isfinite(lsrc)] = np.float32(0.0)
    cov, qx, qy = source_cells(dst_params, rows, g, transform, cs)
    l = np.where(cov, lsrc[qy, qx], np.float32(0.0)).astype(np.float32)
    con = cov & (l != 0)
    if fill:
        con &= L == 0
    with np.errstate(all="ignore"):
        v = l if fill else (L + l).astype(np.float32)
    l_min, l_max = _pz(dst_params.l_min), _pz(dst_params.l_max)
    v = np.where(v < l_min, l_min, v)
    v = np.where(v > l_max, l_max, v).astype(np.float32)
    old_state = state_of(L, dst_params)
    out = np.where(con, v, L).astype(np.float32)
    state = np.where(con, state_of(v, dst_params), old_state).astype(np.int8)
    stats = {"covered": int(cov.sum()), "contributing": int(con.sum()), "changed": int((state != old_state).sum())}
    return out, state, stats


def peer_transform(matched_pose, peer_pose):
    """The source -> destination transform (tx, ty, yaw) when a scan taken at
    `peer_pose` in the peer's frame was found at `matched_pose` in ours:
    se2_compose(matched, se2_inverse(peer_pose))."""
    from .ros_node import se2_compose, se2_inverse

    return se2_compose(matched_pose, se2_inverse(peer_pose))

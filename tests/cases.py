"""Seeded parity cases shared by the CPU oracle tests and the GPU parity tests."""
from __future__ import annotations

import numpy as np

from dm._ffi import DmParams
from dm import synth


def make_params(width, height, resolution=0.05, origin=None, **kw) -> DmParams:
    """Same defaults as dm_default_params (include/dm.h), without the library."""
    p = DmParams()
    p.width, p.height, p.resolution = width, height, resolution
    ox, oy = origin if origin is not None else (-0.5 * width * resolution, -0.5 * height * resolution)
    p.origin_x, p.origin_y = ox, oy
    p.range_min, p.range_max = np.float32(0.02), 12.0
    p.l_occ, p.l_free, p.l_min, p.l_max = 0.85, -0.4, -2.0, 3.5
    p.occ_thresh = p.free_thresh = 0.0
    p.min_frontier_size = 1
    p.band_row0 = 0
    p.band_rows = 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def world_case(seed, width, height, resolution, n_robots, n_beams, n_batches, region_frac=0.9):
    """A synthetic world covering the map, robots random-walking inside it.
    Returns (params, list of (poses[S,3], ranges[S,N])), angle_min, angle_inc."""
    p = make_params(width, height, resolution)
    half_w, half_h = width * resolution / 2, height * resolution / 2
    world = synth.make_world(seed, -half_w, -half_h, half_w, half_h)
    f = region_frac
    stream = synth.ScanStream(world, n_robots, n_beams, seed + 1,
                              region=(-half_w * f, -half_h * f, half_w * f, half_h * f))
    batches = [stream.next_batch() for _ in range(n_batches)]
    return p, batches, float(synth.LD06_ANGLE_MIN), float(synth.ld06_angle_increment(n_beams))


def random_scans(seed, p, S, N, spread=1.0, nan_frac=0.05, far_frac=0.1):
    """Unstructured scans: poses anywhere around the map (also outside it),
    ranges uniform in [0, 1.3*range_max] with NaNs, zeros and infinities."""
    rng = np.random.Generator(np.random.PCG64(seed))
    wx, wy = p.width * p.resolution, p.height * p.resolution
    x = p.origin_x + rng.uniform(-0.2 * spread, 1 + 0.2 * spread, S) * wx
    y = p.origin_y + rng.uniform(-0.2 * spread, 1 + 0.2 * spread, S) * wy
    yaw = rng.uniform(-np.pi, np.pi, S)
    poses = np.stack([x, y, yaw], 1)
    r = rng.uniform(0.0, 1.3 * p.range_max, (S, N)).astype(np.float32)
    r = (np.round(r * 1000) / 1000).astype(np.float32)
    m = rng.random((S, N))
    r[m < nan_frac] = np.nan
    r[(m >= nan_frac) & (m < nan_frac + 0.01)] = 0.0
    r[(m >= nan_frac + 0.01) & (m < nan_frac + 0.02)] = np.inf
    r[(m >= 1 - far_frac)] = np.float32(p.range_max + 1.0)
    inc = float(np.float32(2 * np.pi / max(N - 1, 1)))
    return poses, r, 0.0, inc


def mixed_scans(seed, p, S, N, colocate=0):
    """Scans that reach every state: sensors inside the map, ranges short
    enough that most beams end inside it (hits, so occupied and dead-band
    cells, not only free ones), 5 % NaN and 7 % beyond range_max.  The first
    `colocate` scans share scan 0's position (many pieces on one tile)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    wx, wy = p.width * p.resolution, p.height * p.resolution
    x = p.origin_x + rng.uniform(0.05, 0.95, S) * wx
    y = p.origin_y + rng.uniform(0.05, 0.95, S) * wy
    yaw = rng.uniform(-np.pi, np.pi, S)
    x[:colocate] = x[0]
    y[:colocate] = y[0]
    poses = np.stack([x, y, yaw], 1)
    r = rng.uniform(p.range_min, min(0.45 * min(wx, wy), 1.2 * p.range_max), (S, N))
    r = (np.round(r * 1000) / 1000).astype(np.float32)
    u = rng.random((S, N))
    r[u < 0.05] = np.nan
    r[u > 0.93] = np.float32(1.5 * p.range_max)
    inc = float(np.float32(2 * np.pi / max(N - 1, 1)))
    return poses, r, 0.0, inc


# Named overrides of make_params' map constants (tests/test_gpu_params.py,
# test_oracle.py, test_emulated_kernels.py) and what each one reaches.
PARAM_SETS = {
    # touched cells that stay unknown; free -> unknown by one hit
    "deadband": dict(occ_thresh=0.6, free_thresh=-0.7),
    # overlapping thresholds: occupied wins
    "inverted": dict(occ_thresh=-0.3, free_thresh=0.5),
    # thresholds equal to the clamp bounds (>= / <= at equality)
    "asym": dict(l_occ=0.3, l_free=-0.85, l_min=-0.85, l_max=0.6, occ_thresh=0.6, free_thresh=-0.85),
    # clamp to a zero bound given as -0.0: clamped cells become unknown again
    "upper_zero": dict(l_min=-2.0, l_max=-0.0, occ_thresh=0.0, free_thresh=-0.4),
    # l_min == l_max: every touched cell keeps L == 0, state -1, no frontier
    "zero_clamp": dict(l_min=0.0, l_max=0.0),
    # exact cancellation: 1 hit + 2 misses gives L == 0 on a touched cell
    "cancel": dict(l_occ=0.5, l_free=-0.25, occ_thresh=0.25, free_thresh=-0.25),
    # non-default range gates; most beams truncated
    "short": dict(range_min=0.5, range_max=1.7, l_occ=2.0, l_free=-1.0, l_min=-4.0, l_max=4.0),
    # infinite threshold: never occupied
    "never_occ": dict(occ_thresh=float("inf"), free_thresh=-0.5),
}


def set_params(name, width, height, resolution=0.05, **kw) -> DmParams:
    """make_params with the named set's overrides and a slightly off-grid origin."""
    origin = (-width * resolution / 2 + 0.0137, -height * resolution / 2 - 0.0071)
    return make_params(width, height, resolution=resolution, origin=origin, **{**PARAM_SETS[name], **kw})


def limit_params(major) -> DmParams:
    """range_max / resolution == 16384 cells exactly, the longest ray
    validate_params admits.  "x": a 192-row band in the middle of a 32768^2
    map (6.3 M cells; steep rays cross it with large k); "y": a 192-column
    map, 32768 rows."""
    if major == "x":
        return make_params(32768, 32768, resolution=2.0 ** -10, range_max=16.0,
                           band_row0=16320, band_rows=192)
    return make_params(192, 32768, resolution=2.0 ** -10, range_max=16.0)


def limit_scans(p, S=4, N=720):
    """Scan 0 near the map's centre with beam 0 along the map's long axis
    (16384 major steps); the others anywhere within +-15.9 m (x inside the
    map where it is narrow).  A third of the beams hit at exactly range_max,
    a third at 15.99, a third are +inf (truncated at range_max)."""
    rng = np.random.Generator(np.random.PCG64(16384))
    x = rng.uniform(-15.9, 15.9, S)
    y = rng.uniform(-15.9, 15.9, S)
    yaw = rng.uniform(-np.pi, np.pi, S)
    wx = p.width * p.resolution
    narrow = p.width < p.height
    if narrow:
        x = p.origin_x + (x + 15.9) / 31.8 * wx
    x[0], y[0], yaw[0] = 0.0003, 0.0004, (np.pi / 2 if narrow else 0.0)
    r = np.empty((S, N), np.float32)
    r[:, 0::3] = 16.0
    r[:, 1::3] = 15.99
    r[:, 2::3] = np.inf
    return np.stack([x, y, yaw], 1), r, 0.0, float(np.float32(2 * np.pi / (N - 1)))


def limit_chunk_scan(p):
    """One scan of 8 beams at the limit: so few beams are enumerated in many
    k-chunks (dm_integrate_chunks)."""
    r = np.array([[16.0, 15.99, np.inf, 16.0, 15.99, np.inf, 16.0, 15.99]], np.float32)
    return np.array([[0.0003, 0.0004, 0.1]]), r, 0.0, float(np.float32(2 * np.pi / 8))


def random_state(seed, R, W, p_free=0.5, p_occ=0.1):
    rng = np.random.Generator(np.random.PCG64(seed))
    u = rng.random((R, W))
    st = np.full((R, W), -1, np.int8)
    st[u < p_free] = 0
    st[(u >= p_free) & (u < p_free + p_occ)] = 100
    return st


def blob_state(seed, R, W, n_blobs=20):
    """Unknown background with free discs (explored areas) and occupied specks:
    long, winding frontier components that cross many 64x64 tiles."""
    rng = np.random.Generator(np.random.PCG64(seed))
    st = np.full((R, W), -1, np.int8)
    yy, xx = np.mgrid[0:R, 0:W]
    for _ in range(n_blobs):
        cy, cx = rng.uniform(0, R), rng.uniform(0, W)
        rad = rng.uniform(3, max(4, min(R, W) / 4))
        st[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = 0
    occ = rng.random((R, W)) < 0.03
    st[occ & (st == 0)] = 100
    return st


def sparse_state(seed, R, W, step=3, p_free=0.9):
    """Isolated free cells in unknown space: about R*W/step^2 clusters."""
    rng = np.random.Generator(np.random.PCG64(seed))
    st = np.full((R, W), -1, np.int8)
    st[::step, ::step] = np.where(rng.random(st[::step, ::step].shape) < p_free, 0, -1)
    return st


def tiles_with_free(st):
    """bool [tile rows, tile columns]: the 64 x 64 tiles that hold a free cell."""
    H, W = st.shape
    TY, TX = -(-H // 64), -(-W // 64)
    pad = np.full((TY * 64, TX * 64), 1, np.int8)
    pad[:H, :W] = st
    return (pad.reshape(TY, 64, TX, 64) == 0).any(axis=(1, 3))

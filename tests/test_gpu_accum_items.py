"""k_tile_accum's item loop, branch by branch, bit-exact against the CPU oracle.

Every kind of work item (csrc/dm_integrate.hip: k_plan sorts a call's tiles
by their piece count c) on small maps, each call's U / T statistics and the
final map compared with the oracle, with dm_set_overlap on and off:

  heavy   c > 1024: 256-piece chunks added to the tile's slab, the last one
          applies it; packed slab (c < 65536) and wide slab (c >= 65536)
  medium  257..1024 pieces: one item walked in rounds
  light   16..256 pieces: split walks (c < 256), c = 256, and c just above
  sparse  <= 15 pieces: one item per wave, <= 256 touched 4-cell groups
          (listed) and more (four row passes)

A sensor in the middle of a tile with every beam valid and longer than the
tile's diagonal puts exactly one piece per beam on that tile (a ray leaves a
convex tile once, within 46 steps, and k-chunks are at least 64 steps long),
so c of the sensor's tile is the beam count N.

test_many_items_per_workgroup covers the loop-carried state (the next item's
descriptor and pieces, prefetched across iterations): after a tiny call the
next call's grid is sized from the tiny call's hint, so its workgroups stride
over many dense and many sparse items.
"""
import numpy as np
import pytest

import cases
import dm
from test_gpu_parity import assert_map_equal

pytestmark = pytest.mark.gpu

TS = 64  # tile side (DM_TS)

# name -> (W, H, band_row0, band_rows, sensor cell, second sensor cell); cells
# are (column, global row) of tile centres inside the band
MAPS = {
    "3x3": (192, 192, 0, 0, (96, 96), (32, 160)),
    "ragged": (200, 136, 0, 0, (96, 32), (160, 96)),       # last tile column 8 cells, last tile row 8 rows
    "ragged_odd": (198, 134, 0, 0, (96, 32), (160, 96)),   # W % 4 != 0: the cell-by-cell apply
    "band0": (256, 256, 0, 128, (96, 32), (224, 96)),      # a 256 x 256 map as two bands of 128 rows
    "band1": (256, 256, 128, 128, (160, 224), (32, 160)),
}


def _params(name):
    W, H, r0, rows, a, b = MAPS[name]
    return cases.make_params(W, H, band_row0=r0, band_rows=rows), a, b


def _scan(p, cell, N, seed, S=1, rmin=2.6, rmax=8.0):
    """S scans of N valid beams from the middle of `cell` (a little off the
    cell's centre), every range beyond the tile's diagonal (64 * sqrt 2 cells
    = 4.53 m from a corner, 2.3 m from the middle)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = p.origin_x + (cell[0] + 0.31) * p.resolution
    y = p.origin_y + (cell[1] + 0.27) * p.resolution
    poses = np.tile(np.array([[x, y, 0.3]]), (S, 1))
    poses[:, 2] += rng.uniform(-0.01, 0.01, S)
    ranges = (np.round(rng.uniform(rmin, rmax, (S, N)) * 1000) / 1000).astype(np.float32)
    return poses, ranges, 0.0, float(np.float32(2 * np.pi / max(N - 1, 1)))


def _touched_groups(om_L, p, cell):
    """4-cell groups with a touched cell in the tile around `cell` (on a fresh
    map: every touched cell has L != 0 with the default l_occ / l_free)."""
    r0 = int(p.band_row0)
    ty, tx = (cell[1] - r0) // TS * TS, cell[0] // TS * TS
    t = om_L[ty:ty + TS, tx:tx + TS] != 0
    pad = (-t.shape[1]) % 4
    t = np.pad(t, ((0, 0), (0, pad)))
    return int(t.reshape(t.shape[0], -1, 4).any(axis=2).sum())


def _step(m, om, scan, overlap):
    got = m.integrate(*scan)
    exp = om.integrate(*scan)
    assert got == exp, (got, exp)
    if overlap:  # a frontier pass in flight beside the next call's front-end
        m.frontiers()
    return m.last_stats()


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("name", list(MAPS))
def test_item_kinds(oracle_lib, name, overlap):
    p, a, b = _params(name)
    om = oracle_lib.OracleMap(p)
    with dm.OccupancyMapper(p) as m:
        m.set_overlap(overlap)
        # sparse: 3 beams touch few groups of the sensor's tile, 15 beams many
        st = _step(m, om, _scan(p, b, 3, 1), overlap)
        assert st["sparse_items"] == st["work_items"] >= 1
        assert _touched_groups(om.L, p, b) <= 256
        m.reset()
        om.L[:] = 0.0
        om.state[:] = -1
        st = _step(m, om, _scan(p, a, 15, 2), overlap)
        assert st["sparse_items"] == st["work_items"] >= 1
        assert _touched_groups(om.L, p, a) > 256
        # heavy, packed slab: 2048 pieces = 8 chunks; twice over the same
        # tiles (tile_count, the slab and the ticket are reset by the first)
        for k in range(2):
            st = _step(m, om, _scan(p, a, 2048, 3 + k), overlap)
            assert st["heavy_tiles"] == 1 and st["work_items"] >= 8
        # medium, and light around c = 256
        for N in (600, 1024, 100, 17, 255, 256, 257, 300):
            st = _step(m, om, _scan(p, a, N, 10 + N), overlap)
            assert st["heavy_tiles"] == 0 and st["work_items"] > st["sparse_items"]
        st = _step(m, om, _scan(p, a, 1025, 5), overlap)
        assert st["heavy_tiles"] == 1
        # heavy, wide slab: 17 x 4096 = 69632 pieces on the sensor's tile
        st = _step(m, om, _scan(p, b, 4096, 6, S=17), overlap)
        assert st["heavy_tiles"] >= 1 and st["work_items"] >= 272
        st = _step(m, om, _scan(p, b, 4096, 7, S=17), overlap)
        assert st["heavy_tiles"] >= 1
        # sparse items over applied tiles
        _step(m, om, _scan(p, b, 12, 8), overlap)
        m.set_overlap(False)
        assert_map_equal(m, om)


def _quantize_up(n):  # dm_quantize_up (csrc/dm_internal.h)
    if n <= 8:
        return n
    sh = 0
    while (n >> sh) >= 8:
        sh += 1
    step = 1 << sh
    return (n + step - 1) // step * step


@pytest.mark.parametrize("overlap", [False, True])
def test_many_items_per_workgroup(oracle_lib, overlap):
    """A one-scan, 12-beam call, then a call with hundreds of dense and
    sparse items on the same handle: the second call's grid comes from the
    first call's hint (hw + hw / 16 + 64 workgroups, quantized), so every
    workgroup runs several dense items and every wave several sparse ones."""
    W = H = 3072
    p = cases.make_params(W, H)
    rng = np.random.Generator(np.random.PCG64(77))
    om = oracle_lib.OracleMap(p)
    N = 2048
    inc = float(np.float32(2 * np.pi / (N - 1)))
    # 8 dense sensors (heavy tile, medium ring, light tiles further out) and
    # 300 scans of 12 beams (every 170th beam valid) all over the map: about
    # 600 dense and 1300 sparse items
    S = 308
    cx = rng.integers(4, 44, S) * TS + 32
    cy = rng.integers(4, 44, S) * TS + 32
    poses = np.stack([p.origin_x + (cx + 0.31) * p.resolution, p.origin_y + (cy + 0.27) * p.resolution,
                      rng.uniform(-np.pi, np.pi, S)], 1)
    ranges = (np.round(rng.uniform(2.6, 11.5, (S, N)) * 1000) / 1000).astype(np.float32)
    thin = np.ones(N, bool)
    thin[::170] = False
    ranges[8:, thin] = np.nan
    with dm.OccupancyMapper(p) as m:
        m.set_overlap(overlap)
        for k in range(2):
            tiny = _scan(p, (1568, 1568 + 64 * k), 12, 20 + k, rmin=6.0, rmax=11.0)
            st = _step(m, om, tiny, overlap)
            dense0 = st["work_items"] - st["sparse_items"]
            hw = dense0 + (st["sparse_items"] + 3) // 4
            grid = _quantize_up(hw + hw // 16 + 64)
            st = _step(m, om, (poses, ranges, 0.0, inc), overlap)
            dense = st["work_items"] - st["sparse_items"]
            print(f"grid {grid}: {dense} dense items, {st['sparse_items']} sparse items, "
                  f"{st['heavy_tiles']} heavy tiles")
            assert st["heavy_tiles"] >= 4
            assert dense >= 3 * grid, (dense, grid)
            assert st["sparse_items"] >= 3 * 4 * grid, (st["sparse_items"], grid)
        m.set_overlap(False)
        assert_map_equal(m, om)

"""k_tile_accum's tile totals (touched cells, free-cell change, updates) at
the ends of their ranges, against the CPU oracle.

The apply sums each wave's totals with one packed DPP reduction (wave_totals,
csrc/dm_integrate.hip): touched cells in the low half, the free-cell change,
biased per thread, in the high half, and the updates of edge and heavy tiles
in a reduction of their own.  A tile's free count decides whether it is on
the frontier tile list, and a periodic rebuild (the passes 1, 3, 7, ... after
a bulk write) lists exactly the tiles whose count is above zero: a count that
drifted keeps or drops a tile there, and `frontier_tiles` shows it.

Every case states on the oracle's arrays what it needs the call to do (all
of a tile's cells touched and freed; a tile that both gains and loses free
cells under one wave; a tile whose last free cells go), so that a case which
stops exercising its branch fails instead of passing idly.

Pieces per tile: a ray leaves a convex tile once, so a beam puts one piece
on a tile it crosses, or two where one of the call's k-chunk boundaries falls
inside the tile (a call of few beams splits every beam at multiples of
ceil((nmax + 1) / chunks) steps, chunks <= 3 at 240 steps; dm_integrate_chunks).
"""
import numpy as np
import pytest

import cases
import dm
from cases import tiles_with_free
from test_gpu_accum_items import MAPS, _quantize_up
from test_gpu_parity import assert_map_equal

pytestmark = pytest.mark.gpu

TS = 64
NMAX = 240  # range_max / resolution of cases.make_params
CHUNK_LENS = [(NMAX + c) // c for c in (1, 2, 3)]


def _pose(p, cell, yaw=0.3):
    return np.array([[p.origin_x + (cell[0] + 0.31) * p.resolution, p.origin_y + (cell[1] + 0.27) * p.resolution, yaw]])


def _inc(N):
    return float(np.float32(2 * np.pi / (N - 1)))


def _tile(a, tx, ty):
    return a[ty * TS:(ty + 1) * TS, tx * TS:(tx + 1) * TS]


def _beams_on_tile(oracle_lib, p, scan, tx, ty):
    """(beams with a cell in tile (tx, ty), beams whose cells there straddle a
    possible k-chunk boundary), from the oracle's ray cells."""
    cells, flags = oracle_lib.endpoints(p, *scan)
    n = both = 0
    for (sx, sy, ex, ey), f in zip(cells.tolist(), flags.tolist()):
        if not f:
            continue
        lc = oracle_lib.line_cells(sx, sy, ex, ey)
        k = np.nonzero((lc[:, 0] // TS == tx) & (lc[:, 1] // TS == ty))[0]
        if len(k):
            n += 1
            both += any(k[0] // cl != k[-1] // cl for cl in CHUNK_LENS)
    return n, both


def _passes(m, om, checks=(1, 3, 7)):
    """Frontier passes from a fresh list: pass 1, 3, 7 bring a rebuild, whose
    list holds exactly the tiles with a free cell; every pass's clusters are
    the oracle's."""
    exp = om.frontiers(want_mask=False, want_labels=False)[2]
    for k in range(1, max(checks) + 1):
        fr = m.frontiers()
        np.testing.assert_array_equal(fr.clusters, exp)
        if k in checks:
            assert m.last_stats()["frontier_tiles"] == int(tiles_with_free(om.state).sum()), k


# ---- every lane at the maximum -------------------------------------------------

FULL_SENSOR = (30, 224)   # tile (0, 3) of a 640 x 448 map
FULL_LIGHT = (3, 3)       # columns 192..255: steps 162..225 from the sensor (one k-chunk)
FULL_MEDIUM = (2, 3)      # columns 128..191


def _full_scan(p, cell):
    N = 4096
    return _pose(p, cell), np.full((1, N), np.float32(p.range_max), np.float32), 0.0, _inc(N)


def test_every_cell_of_a_tile_freed(oracle_lib):
    """One 4096-beam scan at maximum range on a fresh map: a light and a
    medium tile some 200 cells away have all 4096 cells touched and turned
    free, so every thread of their applies adds 16 touched and 16 freed cells
    and every wave's packed sum is 1024 in both fields."""
    p = cases.make_params(640, 448)
    scan = _full_scan(p, FULL_SENSOR)
    om = oracle_lib.OracleMap(p)
    exp = om.integrate(*scan)
    for t in (FULL_LIGHT, FULL_MEDIUM):
        assert (_tile(om.state, *t) == 0).all(), t
    n, both = _beams_on_tile(oracle_lib, p, scan, *FULL_LIGHT)
    assert 15 < n <= 256 and both == 0, (n, both)          # <= 256 pieces: one split walk
    n, both = _beams_on_tile(oracle_lib, p, scan, *FULL_MEDIUM)
    assert 257 <= n and n + both <= 1024, (n, both)        # 257..1024 pieces: walked in rounds
    with dm.OccupancyMapper(p) as m:
        got = m.integrate(*scan)
        assert got == exp, (got, exp)
        st = m.last_stats()
        assert st["heavy_tiles"] >= 1 and st["touched"] == exp[1]
        _passes(m, om, checks=(1,))
        # the same scan again: every cell touched, no free count changes
        assert m.integrate(*scan) == om.integrate(*scan)
        _passes(m, om, checks=(2, 6))  # the handle's passes 3 and 7
        assert_map_equal(m, om)


@pytest.mark.parametrize("name", ["ragged", "ragged_odd"])
def test_edge_tiles_freed(oracle_lib, name):
    """The same scan on maps whose last tile column and row are 8 (6) cells
    wide: the edge tiles count their updates in the apply (cells past the
    map's edge are no updates), and W % 4 != 0 applies cell by cell."""
    W, H = MAPS[name][:2]
    p = cases.make_params(W, H)
    scan = _full_scan(p, (100, 70))  # (from here the scan reaches every cell of both maps)
    om = oracle_lib.OracleMap(p)
    exp = om.integrate(*scan)
    TX, TY = -(-W // TS), -(-H // TS)
    # every in-map cell of the last tile column and of the last tile row is
    # touched, and none stays unknown
    assert (om.L[:, (TX - 1) * TS:] != 0).all() and (om.L[(TY - 1) * TS:, :] != 0).all()
    assert (om.state[:, (TX - 1) * TS:] == 0).sum() > 0 and (om.state[(TY - 1) * TS:, :] == 0).sum() > 0
    with dm.OccupancyMapper(p) as m:
        got = m.integrate(*scan)
        assert got == exp, (got, exp)
        _passes(m, om, checks=(1,))
        assert m.integrate(*scan) == om.integrate(*scan)
        _passes(m, om, checks=(2,))
        assert_map_equal(m, om)


# ---- gains and losses under one wave, and a count that reaches zero -------------

X = (2, 1)  # the tile under test of a 384 x 256 map: columns 128..191, rows 64..127


def _light_wave(r):   # k_tile_accum's dense apply: thread tid takes rows tid / 16 + 16 rr
    return (r % 16) // 4


def _heavy_wave(r):   # heavy_quarter: thread tid takes rows 16 q + 4 k + tid / 64
    return r % 4


def _prepared(oracle_lib, p, scan, spots, patch):
    """The map before the call: unknown, tile X saturated occupied except the
    cells under the `spots` beams' end points (free) and the `patch` rows x
    columns of X (unknown).  Returns (L, the spots' cells)."""
    L = np.zeros((int(p.height), int(p.width)), np.float32)
    _tile(L, *X)[...] = np.float32(p.l_max)
    if patch:
        (r0, r1), (c0, c1) = patch
        _tile(L, *X)[r0:r1, c0:c1] = 0.0
    cells, flags = oracle_lib.endpoints(p, *scan)
    ends = []
    for b in spots:
        ex, ey = int(cells[b, 2]), int(cells[b, 3])
        assert flags[b] and (ex // TS, ey // TS) == X, (b, ex, ey)
        L[ey, ex] = -1.0
        ends.append((ex, ey))
    return L, ends


def _light_case(p):
    """From a tile 100 cells to the left: five beams that end in X on rows
    32..35 (wave 0's), and forty that cross X's rows 16..19, also wave 0's
    (45 pieces: a dense light item); both kinds cross the unknown tile in
    between."""
    N = 2048
    ranges = np.full((1, N), np.nan, np.float32)
    spots = [0, 2, 4, 6, 8]
    ranges[0, spots] = np.float32(5.6) + np.float32(0.3) * np.arange(5, dtype=np.float32)  # columns 152..176, rows 96..99
    ranges[0, N - 60:N - 20] = np.float32(11.0)        # angles -0.18 .. -0.06: through rows 80..83 of X and on
    return (_pose(p, (40, 96), yaw=0.0), ranges, 0.0, _inc(N)), spots, ((16, 20), (0, 64))


def _heavy_case(p):
    """2048 beams of 20 cells from the middle of X: a heavy item whose last
    chunk applies the slab in four quarters.  Every 128th beam ends on a free
    cell; the beams towards +x cross the block that some_left leaves unknown."""
    N = 2048
    ranges = np.full((1, N), np.float32(1.0), np.float32)
    spots = list(range(0, N, 128))
    return (_pose(p, (X[0] * TS + 32, X[1] * TS + 32), yaw=0.0), ranges, 0.0, _inc(N)), spots, ((30, 34), (40, 48))


@pytest.mark.parametrize("with_gains", [True, False], ids=["some_left", "none_left"])
@pytest.mark.parametrize("kind", ["light", "heavy"])
def test_gains_and_losses_under_one_wave(oracle_lib, kind, with_gains):
    """One hit turns a free cell occupied (l_occ = 3), one miss frees an
    unknown cell and leaves a saturated one occupied.  some_left: X loses its
    prepared free cells and gains others in the same call, under the same
    wave, so that wave's free-cell sum mixes signs.  none_left: no unknown
    cell of X is crossed, and X's free count must come down to exactly zero:
    the rebuild at the next pass then drops the tile."""
    # (a miss takes 2^-10: the cells around the heavy case's sensor take 2048
    # of them and must stay occupied)
    p = cases.make_params(384, 256, l_occ=3.0, l_free=-(2.0 ** -10))
    scan, spots, patch = (_light_case if kind == "light" else _heavy_case)(p)
    L, ends = _prepared(oracle_lib, p, scan, spots, patch if with_gains else None)
    om = oracle_lib.OracleMap(p)
    om.set_logodds(L)
    before = _tile(om.state, *X).copy()
    assert (before == 0).sum() == len(set(ends)) >= 4
    exp = om.integrate(*scan)
    after = _tile(om.state, *X)
    lost = (before == 0) & (after != 0)
    gained = (before != 0) & (after == 0)
    wave = _light_wave if kind == "light" else _heavy_wave
    rows = np.arange(TS)
    assert lost.sum() == (before == 0).sum()             # every prepared free cell was hit
    if with_gains:
        both = [w for w in range(4) if lost[wave(rows) == w].any() and gained[wave(rows) == w].any()]
        assert both and (after == 0).sum() == gained.sum() > 0, both
        # and a neighbouring tile's unknown cells were freed by the same call
        assert kind == "heavy" or (_tile(om.state, X[0] - 1, X[1]) == 0).any()
    else:
        assert not gained.any() and not (after == 0).any()
        assert tiles_with_free(om.state)[X[1], X[0]] == 0
    with dm.OccupancyMapper(p) as m:
        m.set_logodds(L)
        got = m.integrate(*scan)
        assert got == exp, (got, exp)
        st = m.last_stats()
        assert st["heavy_tiles"] == (1 if kind == "heavy" else 0)
        _passes(m, om, checks=(1,))
        assert_map_equal(m, om)


# ---- the skipped trailing clear ---------------------------------------------------


def _stack_and_spray(p, rng, n_stack, n_spray):
    """n_stack scans of 2048 short beams from the middle of one tile (all their
    cells in that tile: 8 heavy items per scan and nothing else) and n_spray
    scans of 12 long beams from the middles of n_spray other tiles (sparse
    items, and the odd light one where sprays meet)."""
    N = 2048
    S = n_stack + n_spray
    poses = np.zeros((S, 3))
    poses[:n_stack] = _pose(p, (5 * TS + 32, 5 * TS + 32))
    poses[:n_stack, 2] += rng.uniform(-0.01, 0.01, n_stack)
    ranges = (np.round(rng.uniform(0.3, 1.0, (S, N)) * 1000) / 1000).astype(np.float32)
    thin = np.ones(N, bool)
    thin[::170] = False
    others = rng.permutation([t for t in range(100) if t != 55])[:n_spray]
    for k in range(n_spray):
        tx, ty = int(others[k]) % 10, int(others[k]) // 10
        poses[n_stack + k] = _pose(p, (tx * TS + 32, ty * TS + 32), yaw=rng.uniform(-np.pi, np.pi))[0]
        ranges[n_stack + k] = (np.round(rng.uniform(6.0, 11.5, N) * 1000) / 1000).astype(np.float32)
        ranges[n_stack + k, thin] = np.nan
    return poses, ranges, 0.0, _inc(N)


def _items(m):
    st = m.last_stats()
    return st["work_items"] - st["sparse_items"], st["sparse_items"]


def test_one_dense_item_then_sparse_items(oracle_lib):
    """A workgroup whose only dense item is its last clears the count tile
    after it only if it goes on to sparse items.  A tiny call; a call whose
    grid (from the tiny call's hint) gives every workgroup several dense items
    and some of them sparse ones after; then a call sized to its own grid
    (from the second call's hint): as many dense items as workgroups, fewer by
    at most 7, so the sparse items wrap around to workgroups that ran exactly
    one dense item."""
    p = cases.make_params(640, 640)
    rng = np.random.Generator(np.random.PCG64(31))
    om = oracle_lib.OracleMap(p)

    def grid_after(dense, sparse):
        hw = dense + (sparse + 3) // 4
        return min(_quantize_up(hw + hw // 16 + 64), 16384)

    with dm.OccupancyMapper(p) as m:
        def step(scan):
            got, exp = m.integrate(*scan), om.integrate(*scan)
            assert got == exp, (got, exp)
            return _items(m)

        dense, sparse = step(_stack_and_spray(p, rng, 0, 1))
        assert dense == 0 and sparse >= 1
        grid = grid_after(dense, sparse)
        dense, sparse = step(_stack_and_spray(p, rng, 40, 12))
        print(f"call 2: grid {grid}, {dense} dense items, {sparse} sparse items")
        assert dense >= 3 * grid and sparse >= 8, (grid, dense, sparse)
        grid = grid_after(dense, sparse)
        dense, sparse = step(_stack_and_spray(p, rng, grid // 8, 12))
        print(f"call 3: grid {grid}, {dense} dense items, {sparse} sparse items")
        # the sparse items go to the workgroups from dense % grid on, four per
        # workgroup, wrapping around; workgroup b ran exactly one dense item
        # if b < dense <= b + grid
        takers = {(dense % grid + r) % grid for r in range(min((sparse + 3) // 4, grid))}
        assert any(b < dense <= b + grid for b in takers), (grid, dense, sparse)
        assert m.last_stats()["heavy_tiles"] == 1
        assert_map_equal(m, om)

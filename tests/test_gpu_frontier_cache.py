"""GPU: the label cache of the workgroup tile kernel (DESIGN.md §3.2,
dm_frontier_cache_stats).  A tile whose 64 frontier bit rows equal the ones
its cache entry was computed from is labelled from the entry (a hit); every
other tile with frontier cells is labelled in full (a miss) and stores its
entry.  Every pass must equal the CPU oracle's, and the hit / miss counts of
every pass must equal those of the host model below, so that no test passes
with one of the two paths never taken.

The model restates the rules: an entry is keyed by the tile's 64x64 frontier
block alone; tiles in a band's first and last tile row (they write band-edge
rows) and passes with dense outputs never hit; a tile with more than 62
tile-local components invalidates its entry; a tile without frontier cells
neither reads nor writes it.  With DM_FRONTIER_KERNEL=wave only tiles with
more runs than a tile-wave holds (384) reach the workgroup kernel."""
import numpy as np
import pytest

import cases
import dm
from test_gpu_parity import assert_frontiers_equal, assert_map_equal

pytestmark = pytest.mark.gpu

TS = 64
CACHE_ROOTS = 62   # components an entry holds (kCacheRoots)
WAVE_RUNS = 384    # runs a tile-wave holds (kRunsFast)


def _components(block):
    """8-connected components of a 64x64 0/1 block."""
    cells = {(int(y), int(x)) for y, x in zip(*np.nonzero(block))}
    n = 0
    while cells:
        n += 1
        todo = [cells.pop()]
        while todo:
            y, x = todo.pop()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    c = (y + dy, x + dx)
                    if c in cells:
                        cells.remove(c)
                        todo.append(c)
    return n


def _runs(block):
    b = np.zeros((block.shape[0], TS + 1), np.int8)
    b[:, 1:block.shape[1] + 1] = block
    return int(np.count_nonzero(np.diff(b, axis=1) == 1))


class CacheModel:
    """Host model of the cache of one map (bands: `band_rows` rows each)."""

    def __init__(self, H, W, band_rows=None, wave=False, enabled=True):
        self.H, self.W = H, W
        self.R = band_rows or H
        self.wave = wave
        self.enabled = enabled
        self.entries = {}
        self.last = {}

    def tiles(self):
        return [(ty, tx) for ty in range((self.H + TS - 1) // TS) for tx in range((self.W + TS - 1) // TS)]

    def block(self, mask, t):
        blk = np.zeros((TS, TS), np.uint8)
        part = mask[t[0] * TS:(t[0] + 1) * TS, t[1] * TS:(t[1] + 1) * TS]
        blk[:part.shape[0], :part.shape[1]] = part
        return blk

    def band_edge(self, t):
        y0 = (t[0] * TS) % self.R          # band-local first row of the tile
        rows = min(self.R, self.H - (t[0] * TS - y0))  # rows of the tile's band
        return y0 == 0 or y0 + TS >= rows

    def step(self, mask, dense=False):
        """Feeds one pass's frontier mask; returns (hits, misses)."""
        hits = misses = 0
        self.last = {}
        if not self.enabled:
            return 0, 0
        for t in self.tiles():
            blk = self.block(mask, t)
            if not blk.any():
                continue
            if self.wave and _runs(blk) <= WAVE_RUNS:
                continue
            key = blk.tobytes()
            match = not self.band_edge(t) and self.entries.get(t) == key
            if match and not dense:
                hits += 1
                self.last[t] = "hit"
                continue
            misses += 1
            self.last[t] = "miss"
            if not match and not self.band_edge(t):
                if _components(blk) <= CACHE_ROOTS:
                    self.entries[t] = key
                else:
                    self.entries.pop(t, None)
        return hits, misses


def _logodds(p, st):
    return np.where(st == 100, np.float32(p.l_occ), np.where(st == 0, np.float32(p.l_free), np.float32(0)))


def _base_state(H, W):
    """Free regions whose frontiers cross tile edges and corners of the
    interior tile row (tile rows 64..127), in unknown space."""
    st = np.full((H, W), -1, np.int8)
    st[40:min(H, 150), 30:min(W, 236)] = 0          # a free room over every tile column
    st[70:75, 100:140] = 100                        # a wall inside it
    st[90:110, 56:72] = -1                          # unknown pockets over the tile edges x = 64, 128, 192
    st[80:100, 120:136] = -1
    st[100:120, 186:198] = -1
    st[56:72, 150:170] = -1                         # ... and over y = 64, y = 128
    st[120:min(H, 136), 20:40] = -1
    st[120:min(H, 136), 120:136] = -1               # over the corner (128, 128)
    st[60:68, 60:68] = -1                           # over the corner (64, 64)
    return st


def _diag_state(H, W):
    """_base_state plus a one-cell diagonal corridor of free cells in the
    unknown pocket over the corner (128, 128): a component that crosses the
    corner between tile (1, 1) and tile (2, 2) diagonally."""
    st = _base_state(H, W)
    for i in range(121, min(H, 135)):
        st[i, i] = 0
    return st


def _check_pass(m, om, model, want_labels=False, want_mask=False):
    fr = m.frontiers(want_mask=want_mask, want_labels=want_labels)
    mask, labels, clusters = om.frontiers()
    assert_frontiers_equal(fr, mask, labels, clusters)
    expect = model.step(mask, dense=want_labels or want_mask)
    assert m.frontier_cache_stats() == expect, (m.frontier_cache_stats(), expect)
    return fr, expect


def _set(m, om, p, st):
    om.L[...] = _logodds(p, st)
    om.state[...] = st
    m.set_state(st)


MAPS = [(256, 192), (200, 136)]


@pytest.mark.parametrize("W,H", MAPS)
def test_same_state_twice_hits_every_interior_tile(oracle_lib, monkeypatch, W, H):
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    p = cases.make_params(W, H)
    st = _diag_state(H, W)
    om = oracle_lib.OracleMap(p)
    model = CacheModel(H, W)
    with dm.OccupancyMapper(p) as m:
        _set(m, om, p, st)
        fr1, (h1, m1) = _check_pass(m, om, model)
        assert h1 == 0 and m1 > 0
        fr2, (h2, m2) = _check_pass(m, om, model)
        np.testing.assert_array_equal(fr1.clusters, fr2.clusters)
        interior = [t for t, v in model.last.items() if not model.band_edge(t)]
        assert len(interior) == (W + TS - 1) // TS            # every tile of the interior row has frontier cells
        assert all(model.last[t] == "hit" for t in interior)
        assert h2 == len(interior) and h2 + m2 == m1
        # the bulk write of an equal state touches no entry
        m.set_state(st)
        _, (h3, _) = _check_pass(m, om, model)
        assert h3 == h2


@pytest.mark.parametrize("W,H", MAPS)
def test_one_cell_changes_one_tile(oracle_lib, monkeypatch, W, H):
    """A cell flipped deep inside tile (1, 1): that tile misses, its
    neighbours (whose components continue into it across the edges x = 64 and
    x = 128, and across the corner (128, 128) on the tall map) hit."""
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    p = cases.make_params(W, H)
    st = _diag_state(H, W)
    om = oracle_lib.OracleMap(p)
    model = CacheModel(H, W)
    with dm.OccupancyMapper(p) as m:
        _set(m, om, p, st)
        _check_pass(m, om, model)
        _check_pass(m, om, model)
        before = om.frontiers()[0].copy()
        st2 = st.copy()
        st2[90, 128 - 3] = 0          # the unknown pocket at rows 80..99, columns 120..135
        _set(m, om, p, st2)
        after = om.frontiers()[0]
        changed = {t for t in model.tiles() if not np.array_equal(model.block(before, t), model.block(after, t))}
        assert changed == {(1, 1)}
        _, (h, ms) = _check_pass(m, om, model)
        assert model.last[(1, 1)] == "miss"
        assert model.last[(1, 0)] == "hit" and model.last[(1, 2)] == "hit"
        assert h == (W + TS - 1) // TS - 1
        # components of the missed tile continue into hit tiles: over both of its vertical edges
        lab = om.frontiers()[1]
        assert len(set(lab[64:128, 63][lab[64:128, 63] >= 0]) & set(lab[64:128, 64][lab[64:128, 64] >= 0])) > 0
        assert len(set(lab[64:128, 127][lab[64:128, 127] >= 0]) & set(lab[64:128, 128][lab[64:128, 128] >= 0])) > 0
        if H > 129:  # ... and diagonally over the corner (128, 128)
            assert lab[127, 127] >= 0 and lab[127, 127] == lab[128, 128]
        _, (h, ms) = _check_pass(m, om, model)
        assert h == (W + TS - 1) // TS


def test_emptied_tile_hits_on_its_old_entry(oracle_lib, monkeypatch):
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    W, H = 256, 192
    p = cases.make_params(W, H)
    st = _diag_state(H, W)
    om = oracle_lib.OracleMap(p)
    model = CacheModel(H, W)
    with dm.OccupancyMapper(p) as m:
        _set(m, om, p, st)
        _check_pass(m, om, model)
        stB = st.copy()
        stB[64:128, 128:192] = 100    # tile (1, 2): no free cell, so no frontier cell
        _set(m, om, p, stB)
        _check_pass(m, om, model)
        assert (1, 2) not in model.last
        _set(m, om, p, st)
        _, (h, _) = _check_pass(m, om, model)
        assert model.last[(1, 2)] == "hit" and h >= 1


def test_reset_then_same_scans(oracle_lib, monkeypatch):
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    W, H = 256, 192
    p, batches, amin, inc = cases.world_case(81, W, H, 0.05, 3, 360, 3, region_frac=0.8)
    model = CacheModel(H, W)
    with dm.OccupancyMapper(p) as m:
        total_hits = []
        for rnd in range(2):
            om = oracle_lib.OracleMap(p)
            hits = 0
            for poses, ranges in batches:
                assert m.integrate(poses, ranges, amin, inc) == om.integrate(poses, ranges, amin, inc)
                hits += _check_pass(m, om, model)[1][0]
            _, (h, _) = _check_pass(m, om, model)   # the unchanged map once more
            assert h == sum(1 for t in model.last if not model.band_edge(t)) > 0
            assert_map_equal(m, om)
            total_hits.append(hits)
            m.reset()
        # the replay ends on the entries of the first round's last pass
        assert total_hits[1] >= total_hits[0]


@pytest.mark.parametrize("n,cached", [(CACHE_ROOTS, True), (CACHE_ROOTS + 1, False)])
def test_entry_capacity(oracle_lib, monkeypatch, n, cached):
    """Isolated free cells in unknown space, n of them in tile (1, 1): n
    tile-local components."""
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    W, H = 256, 192
    p = cases.make_params(W, H)
    st = np.full((H, W), -1, np.int8)
    st[70:100, 10:40] = 0             # something in tile (1, 0) too
    for i in range(n):
        st[66 + 2 * (i // 16), 66 + 2 * (i % 16)] = 0
    om = oracle_lib.OracleMap(p)
    model = CacheModel(H, W)
    with dm.OccupancyMapper(p) as m:
        _set(m, om, p, st)
        fr, _ = _check_pass(m, om, model)
        assert len(fr.clusters) == n + 1
        for _ in range(2):
            _check_pass(m, om, model)
            assert model.last[(1, 0)] == "hit"
            assert model.last[(1, 1)] == ("hit" if cached else "miss")
        # a valid entry is invalidated by an overfull pass and rebuilt afterwards
        st2 = st.copy()
        st2[120, 70] = 0
        _set(m, om, p, st2)
        _check_pass(m, om, model)
        assert model.last[(1, 1)] == "miss"
        _set(m, om, p, st)
        _check_pass(m, om, model)
        assert model.last[(1, 1)] == "miss"
        _check_pass(m, om, model)
        assert model.last[(1, 1)] == ("hit" if cached else "miss")


def test_dense_outputs_after_cached_passes(oracle_lib, monkeypatch):
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    W, H = 200, 136
    p = cases.make_params(W, H)
    st = _diag_state(H, W)
    om = oracle_lib.OracleMap(p)
    model = CacheModel(H, W)
    with dm.OccupancyMapper(p) as m:
        _set(m, om, p, st)
        _check_pass(m, om, model)
        _, (h, _) = _check_pass(m, om, model)
        assert h > 0
        _, (hd, md) = _check_pass(m, om, model, want_labels=True)
        assert hd == 0 and md == len(model.last)
        _, (hd, md) = _check_pass(m, om, model, want_mask=True, want_labels=True)
        assert hd == 0
        _, (h2, _) = _check_pass(m, om, model)   # the entries survived the dense passes
        assert h2 == h
        # a dense pass on changed rows stores the entries the next pass hits
        st2 = st.copy()
        st2[90, 128 - 3] = 0
        _set(m, om, p, st2)
        _check_pass(m, om, model, want_labels=True)
        _, (h3, _) = _check_pass(m, om, model)
        assert h3 == h


def _comb_state(H, W):
    """Run-rich tiles with one component each (a comb: one free row, every
    other column free below it, in unknown space), more than a tile-wave's
    384 runs, so that DM_FRONTIER_KERNEL=wave sends them to the workgroup
    kernel too; few clusters, many listed tiles."""
    st = np.full((H, W), -1, np.int8)
    for ty, tx in [(1, 1), (1, 2), (0, 1)]:
        y0, x0 = ty * TS, tx * TS
        st[y0 + 2, x0:x0 + TS] = 0
        st[y0 + 3:y0 + 60, x0:x0 + TS:2] = 0
    for y0, x0 in [(70, 8), (10, 200), (10, 8), (140, 8), (140, 140), (140, 200), (70, 200)]:
        st[y0:y0 + 40, x0:x0 + 30] = 0   # plain tiles, listed as well: one cluster each
    return st


@pytest.mark.parametrize("kernel", ["wave", "wg"])
def test_both_edge_kinds(oracle_lib, monkeypatch, kernel):
    """The tile-edge unions in the tile kernel (wg) and in k_frontier_edges
    after publish-only tile kernels (wave: only the run-rich comb tiles reach
    the workgroup kernel), hit tiles publishing their edges from the entry."""
    monkeypatch.setenv("DM_FRONTIER_KERNEL", kernel)
    W, H = 256, 192
    p = cases.make_params(W, H)
    st = _comb_state(H, W)
    om = oracle_lib.OracleMap(p)
    model = CacheModel(H, W, wave=kernel == "wave")
    with dm.OccupancyMapper(p) as m:
        _set(m, om, p, st)
        _check_pass(m, om, model)
        for k in range(3):
            fr, (h, ms) = _check_pass(m, om, model, want_labels=k == 1)
            if k != 1:
                assert model.last[(1, 1)] == "hit" and model.last[(1, 2)] == "hit" and model.last[(0, 1)] == "miss"
            if kernel == "wave":
                assert h + ms == 3
                listed = sum(1 for t in model.tiles() if (model.block(st == 0, t)).any())
                assert len(fr.clusters) <= listed   # no more clusters than listed tiles: the edge kernel's passes
        st2 = st.copy()
        st2[100, 128 + 1] = 0       # joins two teeth of tile (1, 2)'s comb
        _set(m, om, p, st2)
        _check_pass(m, om, model)
        assert model.last[(1, 1)] == "hit" and model.last[(1, 2)] == "miss"
        _check_pass(m, om, model)


def test_banded_handle(oracle_lib, monkeypatch):
    """Three bands of three tile rows each (halo rows between them): the
    counts are the bands' sums, the interior tile row of every band hits."""
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    W, H = 256, 576
    p = cases.make_params(W, H)
    st = np.full((H, W), -1, np.int8)
    for b in range(3):
        st[b * 192:(b + 1) * 192] = _diag_state(192, W)
    st[150:240, 100:110] = 0          # free corridors across the band edges
    st[340:420, 30:40] = 0
    om = oracle_lib.OracleMap(p)
    model = CacheModel(H, W, band_rows=192)
    import ctypes

    for r in range(3):
        row0, rows = ctypes.c_int64(0), ctypes.c_int64(0)
        assert dm.load_library().dm_sharded_band_rows(H, 3, r, ctypes.byref(row0), ctypes.byref(rows)) == 0
        assert (row0.value, rows.value) == (192 * r, 192)
    with dm.OccupancyMapper(p, devices=[0, 0, 0]) as sh:
        _set(sh, om, p, st)
        _check_pass(sh, om, model)
        _, (h, ms) = _check_pass(sh, om, model)
        assert h == 3 * 4 and ms > 0
        st2 = st.copy()
        st2[192 + 90, 128 - 3] = 0
        _set(sh, om, p, st2)
        _, (h, ms) = _check_pass(sh, om, model)
        assert h == 3 * 4 - 1 and model.last[(4, 1)] == "miss"
        # the bands' own dense passes (per-cell labels) are misses and keep the entries
        assert_frontiers_equal(sh.frontiers(want_mask=True, want_labels=True), *om.frontiers())
        _, (h, ms) = _check_pass(sh, om, model)
        assert h == 3 * 4


def test_pipelined_depth_two(oracle_lib, monkeypatch):
    """Two passes in flight with integrate calls in between: every collected
    pass equals the oracle's, and its counts the model's, in order."""
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    W, H = 256, 192
    p, batches, amin, inc = cases.world_case(83, W, H, 0.05, 3, 360, 6, region_frac=0.8)
    batches = batches + batches[-1:] * 2       # the last scans again: little changes, many hits
    om = oracle_lib.OracleMap(p)
    expect = []
    for poses, ranges in batches:
        om.integrate(poses, ranges, amin, inc)
        expect.append(om.frontiers(want_labels=False))
    model = CacheModel(H, W)
    with dm.OccupancyMapper(p) as m:
        m.set_overlap(True)
        got = []

        def collect():
            got.append((m.frontiers_end(), m.frontier_cache_stats()))

        for k, (poses, ranges) in enumerate(batches):
            m.integrate(poses, ranges, amin, inc)
            if k > 1:
                collect()
            m.frontiers_begin()
        collect()
        collect()
        assert len(got) == len(expect)
        hits = 0
        for (fr, stats), (mask, _, clusters) in zip(got, expect):
            assert fr is not None
            np.testing.assert_array_equal(fr.clusters, clusters)
            assert stats == model.step(mask)
            hits += stats[0]
        assert hits > 0
        assert_map_equal(m, om)


def test_cache_off(oracle_lib, monkeypatch):
    monkeypatch.setenv("DM_FRONTIER_KERNEL", "wg")
    monkeypatch.setenv("DM_FRONTIER_CACHE", "off")
    W, H = 256, 192
    p = cases.make_params(W, H)
    st = _diag_state(H, W)
    om = oracle_lib.OracleMap(p)
    model = CacheModel(H, W, enabled=False)
    with dm.OccupancyMapper(p) as m:
        _set(m, om, p, st)
        for k in range(3):
            _, (h, ms) = _check_pass(m, om, model, want_labels=k == 2)
            assert m.frontier_cache_stats()[0] == 0

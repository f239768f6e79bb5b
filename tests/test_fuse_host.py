"""CPU: the host restatement of map fusion (dm/fuse.py) against independent
NumPy, and the shared case table's inputs against the conditions every case
asserts (tests/fuse_cases.py)."""
import math

import numpy as np
import pytest

import cases
import fuse_cases as fc
from dm import fuse
from dm.ros_node import se2_compose


def _random_L(seed, shape, p, zero_frac=0.4):
    rng = np.random.Generator(np.random.PCG64(seed))
    L = rng.uniform(float(p.l_min), float(p.l_max), shape).astype(np.float32)
    L[rng.random(shape) < zero_frac] = 0.0
    return L


def _state(L, p):
    st = np.full(L.shape, -1, np.int8)
    st[(L != 0) & (L <= p.free_thresh)] = 0
    st[(L != 0) & (L >= p.occ_thresh)] = 100
    return st


def test_identity_add_is_clipped_sum():
    p = cases.make_params(200, 136)
    L1, L2 = _random_L(1, (136, 200), p), _random_L(2, (136, 200), p)
    out, st, stats = fuse.fuse_map(L1, p, L2, fuse.geom_of(p), (0.0, 0.0, 0.0), "add")
    exp = np.where(L2 != 0, np.clip(L1 + L2, np.float32(p.l_min), np.float32(p.l_max)), L1).astype(np.float32)
    assert np.array_equal(out.view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(st, _state(exp, p))
    assert stats["covered"] == 200 * 136 and stats["contributing"] == int((L2 != 0).sum())
    assert stats["changed"] == int((_state(exp, p) != _state(L1, p)).sum())


def test_whole_cell_shift_is_slicing():
    p = cases.make_params(200, 136)
    L1 = np.zeros((136, 200), np.float32)
    src_p = cases.make_params(96, 70, origin=(float(p.origin_x), float(p.origin_y)))
    L2 = _random_L(3, (70, 96), p, zero_frac=0.0)
    # the source's cell (0, 0) lands on destination cell (30, 20); its top rows hang over the edge at (150, 100)
    for (i, j) in ((30, 20), (150, 100), (-10, -7)):
        out, _, stats = fuse.fuse_map(L1, p, L2, fuse.geom_of(src_p), (i * 0.05, j * 0.05, 0.0), "add")
        exp = np.zeros_like(L1)
        y0, x0 = max(j, 0), max(i, 0)
        y1, x1 = min(j + 70, 136), min(i + 96, 200)
        exp[y0:y1, x0:x1] = L2[y0 - j:y1 - j, x0 - i:x1 - i]
        assert np.array_equal(out, exp), (i, j)
        assert stats["covered"] == (y1 - y0) * (x1 - x0) == stats["contributing"]


def test_exact_quarter_turn_is_rot90():
    n = 64
    p = cases.make_params(n, n)
    L2 = _random_L(4, (n, n), p, zero_frac=0.0)
    out, _, stats = fuse.fuse_map(np.zeros((n, n), np.float32), p, L2, fuse.geom_of(p), (0.0, 0.0, math.pi / 2),
                                  "add", cs=(0.0, 1.0))
    # p_dst = R(pi/2) p_src: destination (cx, cy) reads source (cy, n - 1 - cx)
    assert np.array_equal(out, np.rot90(L2, -1))
    assert stats["covered"] == n * n
    # and the half turn reads (n - 1 - cx, n - 1 - cy)
    out, _, _ = fuse.fuse_map(np.zeros((n, n), np.float32), p, L2, fuse.geom_of(p), (0.0, 0.0, math.pi), "add",
                              cs=(-1.0, 0.0))
    assert np.array_equal(out, np.rot90(L2, 2))


def test_non_finite_source_values_read_as_zero_and_states_map_to_log_odds():
    p = cases.make_params(64, 64)
    L2 = np.zeros((64, 64), np.float32)
    L2[3, 4], L2[5, 6], L2[7, 8], L2[9, 10] = np.nan, np.inf, -np.inf, 1.0
    out, _, stats = fuse.fuse_map(np.zeros((64, 64), np.float32), p, L2, fuse.geom_of(p), (0.0, 0.0, 0.0), "add")
    assert stats["contributing"] == 1 and out[9, 10] == 1.0 and np.count_nonzero(out) == 1
    st = np.full((64, 64), -1, np.int8)
    st[1, 1], st[2, 2], st[3, 3] = 100, 0, 50
    out, state, stats = fuse.fuse_map(np.zeros((64, 64), np.float32), p, st, fuse.geom_of(p), (0.0, 0.0, 0.0), "add",
                                      src_is_state=True)
    assert out[1, 1] == np.float32(p.l_occ) and out[2, 2] == np.float32(p.l_free) and out[3, 3] == 0
    assert state[1, 1] == 100 and state[2, 2] == 0 and stats == {"covered": 4096, "contributing": 2, "changed": 2}


@pytest.mark.parametrize("name", [n for n in fc.CASE_NAMES if n != "outside"])
def test_fill_is_idempotent_and_keeps_known_cells(name):
    p = fc.dst_params()
    L0 = fc.dst_logodds()
    out, st, stats = fc.expected(L0, p, name, "fill", "logodds")
    known = L0 != 0
    assert np.array_equal(out[known].view(np.uint32), L0[known].view(np.uint32))
    again, st2, stats2 = fc.expected(out, p, name, "fill", "logodds")
    assert np.array_equal(again.view(np.uint32), out.view(np.uint32)) and np.array_equal(st2, st)
    assert stats2["contributing"] == 0 and stats2["changed"] == 0 and stats2["covered"] == stats["covered"]


@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_case_table_meets_its_conditions(name, mode, kind):
    """The conditions the GPU tests assert hold for the chosen inputs, and the
    stats agree with the arrays."""
    p = fc.dst_params()
    L0 = fc.dst_logodds()
    out, st, stats = fc.expected(L0, p, name, mode, kind)
    fc.check_stats(name, stats)
    assert np.array_equal(st, _state(out, p))
    changed_L = out.view(np.uint32) != L0.view(np.uint32)
    assert changed_L.sum() <= stats["contributing"] <= stats["covered"]
    assert stats["changed"] == int((st != _state(L0, p)).sum())
    assert out.min() >= np.float32(p.l_min) and out.max() <= np.float32(p.l_max)


def test_case_inputs_have_the_edge_values():
    p = fc.dst_params()
    L0 = fc.dst_logodds()
    assert (L0 == np.float32(p.l_max)).any() and (L0 == np.float32(p.l_min)).any()
    # tile_seen is mixed: some 64 x 64 tiles are untouched, some are not
    seen = [bool((L0[y:y + 64, x:x + 64] != 0).any()) for y in range(0, 136, 64) for x in range(0, 200, 64)]
    assert any(seen) and not all(seen)
    for res in (0.05, 0.1, 0.025):
        geom, L, st = fc.source(res)
        assert L.shape == (fc.SRC_H, fc.SRC_W) and geom["resolution"] == res
        assert np.isnan(L).sum() == 1 and np.isinf(L).sum() == 1 and (L == 0).any()
        fin = L[np.isfinite(L)]
        assert (fin == np.float32(3.5)).any() and (fin == np.float32(-2.0)).any()
        assert set(np.unique(st)) == {-1, 0, 50, 100}
    # ADD clamps somewhere: a sum leaves [l_min, l_max] before the clamp
    geom, L, _, transform = fc.case("yaw_0.3")
    cov, qx, qy = fuse.source_cells(p, fc.DST_H, geom, transform)
    l = np.where(cov & np.isfinite(L[qy, qx]), L[qy, qx], 0).astype(np.float32)
    raw = L0 + l
    assert (raw > np.float32(p.l_max)).any() or (raw < np.float32(p.l_min)).any()


def test_mode_names():
    assert fuse.mode_code("add") == fuse.FUSE_ADD == 0 and fuse.mode_code("fill") == fuse.FUSE_FILL == 1
    with pytest.raises(ValueError):
        fuse.mode_code("max")


def test_peer_transform_round_trips_with_se2_compose():
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(20):
        T = tuple(rng.uniform(-3, 3, 3))
        q = tuple(rng.uniform(-3, 3, 3))
        got = fuse.peer_transform(se2_compose(T, q), q)
        assert np.allclose(got[:2], T[:2], atol=1e-12)
        assert abs(math.remainder(got[2] - T[2], 2 * math.pi)) < 1e-12

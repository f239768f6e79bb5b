"""CPU: the host restatement of clearance-aware planning (dm.plan.clearance,
penalty, inflation_table, field_cost, path with a penalty), which the GPU
tests (test_gpu_plan_cost.py) compare dm_plan_clearance and dm_plan_field_cost
with: checked here against brute force, against the unweighted restatement,
and on the L-shaped corridor the feature is for."""
import math

import numpy as np
import pytest

from dm import plan

U = plan.UNREACHABLE


def brute_clearance(st, R):
    """The definition, literally: the disc minimum around every cell."""
    H, W = st.shape
    far = R * R + 1
    out = np.full((H, W), far, np.int64)
    occ = st == 100
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d = dx * dx + dy * dy
            if d <= R * R:
                out = np.where(plan._shifted(occ, dy, dx), np.minimum(out, d), out)
    return out.astype(np.uint16)


def l_corridor():
    """192 x 192, all occupied but an 11-cell-wide L: along y = 20..30 from
    x = 20 to 167, then along x = 157..167 down to y = 167.  Returns the state,
    the source and the target cell (cx, cy), on the centre line 5 cells from
    either end."""
    st = np.full((192, 192), 100, np.int8)
    st[20:31, 20:168] = 0
    st[20:168, 157:168] = 0
    return st, (25, 25), (162, 162)


def l_corridor_paths(st, src, dst, field_of, path_of):
    """(weighted, unweighted) paths source -> target for inflate_cells = 1,
    R = 8 and Nav2's curve at 5 cm; field_of(cell_pen or None) -> uint32 field,
    path_of(field, cell_pen or None) -> linear indices."""
    pen = plan.inflation_table(0.05, 8, 0.05, 10.0)
    cp = plan.penalty(st, 8, pen)
    return [np.asarray(path_of(field_of(c), c)) for c in (cp, None)]


def least_d2_inside(st, cells, skip=12):
    return int(plan.clearance(st, 8).reshape(-1)[cells[skip:-skip]].min())


@pytest.mark.parametrize("R", [1, 7, 32])
def test_clearance_is_the_disc_minimum(R):
    rng = np.random.default_rng(5 + R)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(75, 100), p=[0.68, 0.30, 0.02])
    got = plan.clearance(st, R)
    assert got.dtype == np.uint16
    np.testing.assert_array_equal(got, brute_clearance(st, R))
    assert (got[st == 100] == 0).all() and got.max() <= R * R + 1
    np.testing.assert_array_equal(plan.clearance(np.zeros((9, 9), np.int8), R), np.full((9, 9), R * R + 1))
    for bad in (0, 33):
        with pytest.raises(ValueError):
            plan.clearance(st, bad)


@pytest.mark.parametrize("r", [0, 1, 5, 32])
def test_traversable_is_a_threshold_of_the_clearance(r):
    rng = np.random.default_rng(17)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(90, 110), p=[0.7, 0.27, 0.03])
    np.testing.assert_array_equal((plan.clearance(st, 32) > r * r) & (st == 0), plan.traversable(st, r))


def test_zero_table_is_the_unweighted_field():
    rng = np.random.default_rng(23)
    st = rng.choice(np.array([0, -1, 100], np.int8), size=(70, 90), p=[0.92, 0.05, 0.03])
    st[10, 10] = st[50, 70] = 0
    srcs = [(10, 10), (70, 50)]
    for r, R in ((0, 1), (1, 6)):
        exp = plan.field(st, srcs, r)
        np.testing.assert_array_equal(plan.field_cost(st, srcs, r, R, np.zeros(R * R + 2, np.uint8)), exp)
        np.testing.assert_array_equal(plan.field_cost(st, srcs, r, R, np.zeros(R * R + 2, np.uint8), max_cost=150),
                                      np.where(exp <= 150, exp, U))
    assert (exp != U).sum() > 500


def test_weighted_field_is_a_fixpoint_of_the_weighted_move():
    """Every reached cell but the sources has a predecessor by the weighted
    rule (path finds one from every cell), and no legal move undercuts a cost."""
    rng = np.random.default_rng(29)
    st = rng.choice(np.array([0, 100], np.int8), size=(40, 50), p=[0.9, 0.1])
    st[5, 5] = 0
    R = 3
    pen = rng.integers(0, 256, R * R + 2).astype(np.uint8)
    cp = plan.penalty(st, R, pen)
    f = plan.field_cost(st, [(5, 5)], 0, R, pen)
    t = plan.with_sources(plan.traversable(st, 0), [(5, 5)])
    reached = np.flatnonzero(f.reshape(-1) != U)
    assert len(reached) > 1000
    for c in reached[:: 37]:
        p = plan.path(f, t, int(c), cp)
        assert p[0] == 5 * 50 + 5 and p[-1] == c and len(p) <= f.reshape(-1)[c] // 5 + 1
    fi = f.astype(np.int64)
    for (dy, dx), ok in zip(plan.NEIGHBOURS, plan.legal_moves(t)):
        b = 7 if dy and dx else 5
        ys, xs = np.nonzero(ok & (f != U))
        assert (fi[ys + dy, xs + dx] <= fi[ys, xs] + b * (1 + cp[ys + dy, xs + dx].astype(np.int64))).all()


def test_inflation_table_end_points():
    tab = plan.inflation_table(0.05, 8, 0.05, 10.0)
    assert tab.dtype == np.uint8 and tab.shape == (66,)
    assert tab[0] == 252 and tab[1] == 252            # 0 m and 0.05 m: within the inscribed radius
    assert tab[2] == math.floor(252 * math.exp(-10.0 * (math.sqrt(2) * 0.05 - 0.05)))
    assert tab[64] == math.floor(252 * math.exp(-10.0 * 0.35)) == 7
    assert tab[65] == 0                               # far
    assert (np.diff(tab[:65].astype(int)) <= 0).all()
    assert plan.inflation_table(0.05, 1, 0.0, 10.0).tolist() == [252, math.floor(252 * math.exp(-0.5)), 0]
    for bad in (0, 33):
        with pytest.raises(ValueError):
            plan.inflation_table(0.05, bad, 0.05, 10.0)
    with pytest.raises(ValueError):
        plan.penalty(np.zeros((4, 4), np.int8), 2, np.zeros(5, np.uint8))  # needs 6 entries


def test_l_corridor_keeps_its_clearance():
    """The weighted path keeps to the corridor's centre line (6 cells from
    either wall) round the corner, the shortest path shaves the inside corner
    at 2 cells; six path cells more."""
    st, src, dst = l_corridor()
    t = plan.with_sources(plan.traversable(st, 1), [src])
    weighted, shortest = l_corridor_paths(
        st, src, dst, lambda cp: plan.field(st, [src], 1, cell_pen=cp),
        lambda f, cp: plan.path(f, t, dst[1] * 192 + dst[0], cp))
    assert least_d2_inside(st, weighted) == 36
    assert least_d2_inside(st, shortest) == 4
    assert (len(weighted), len(shortest)) == (272, 266)

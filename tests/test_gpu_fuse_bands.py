"""GPU: map fusion on row bands.  A band handle fuses its own rows of the same
global picture, and a dm_create_sharded handle forwards to its bands and sums
their stats: both equal one whole-map handle bit for bit."""
import numpy as np
import pytest

import cases
import dm
import fuse_cases as fc
from dm import fuse

pytestmark = pytest.mark.gpu

W, H = 200, 192
# the 4.8 m x 3.5 m source turned about the map's centre: it reaches over both edges of rows 64..127
TRANSFORMS = [(0.1, -0.05, 0.3), (-3.0, 1.2, -2.5), (0.0, 0.0, 0.0)]


def _dst_logodds(p):
    """Log-odds with unknown regions, both clamps and every state."""
    rng = np.random.Generator(np.random.PCG64(31))
    L = rng.choice(np.array([0.0, -0.4, 0.85, -2.0, 3.5, 1.7], np.float32), size=(H, W),
                   p=[0.5, 0.2, 0.1, 0.1, 0.05, 0.05]).astype(np.float32)
    L[:, 120:] = 0.0  # whole tiles unknown
    return L


@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("mode", fc.MODES)
def test_band_handle_equals_its_rows_of_the_whole_map(mode, kind):
    p = cases.make_params(W, H)
    pb = cases.make_params(W, H, band_row0=64, band_rows=64)
    geom, Ls, sts, _ = fc.case("yaw_0.3")
    L0 = _dst_logodds(p)
    with dm.OccupancyMapper(p) as whole, dm.OccupancyMapper(pb) as band:
        whole.set_logodds(L0)
        band.set_logodds(L0[64:128])
        for t in TRANSFORMS:
            call = (lambda m: m.fuse_state(sts, geom, t, mode)) if kind == "state" else \
                (lambda m: m.fuse_logodds(Ls, geom, t, mode))
            before = band.logodds()
            sw, sb = call(whole), call(band)
            Lw, Lb = whole.logodds(), band.logodds()
            assert np.array_equal(Lb.view(np.uint32), Lw[64:128].view(np.uint32))
            assert np.array_equal(band.state(), whole.state()[64:128])
            # the band's stats are those of the restatement on its rows
            src = sts if kind == "state" else Ls
            exp = fuse.fuse_map(before, pb, src, geom, t, mode, src_is_state=kind == "state")
            assert sb == exp[2] and np.array_equal(Lb.view(np.uint32), exp[0].view(np.uint32))
            assert 0 < sb["covered"] < sw["covered"]
        assert sb["covered"] < 64 * W


@pytest.mark.parametrize("mode", fc.MODES)
def test_sharded_handle_equals_one_handle(mode):
    p = cases.make_params(W, H)
    geom, Ls, sts, _ = fc.case("yaw_0.3")
    L0 = _dst_logodds(p)
    sp = cases.make_params(fc.SRC_W, fc.SRC_H, geom["resolution"], origin=(geom["origin_x"], geom["origin_y"]))
    with dm.OccupancyMapper(p) as one, dm.OccupancyMapper(p, devices=[0, 0, 0]) as sh, \
            dm.OccupancyMapper(sp) as s:
        one.set_logodds(L0)
        sh.set_logodds(L0)
        s.set_logodds(Ls)
        for k, t in enumerate(TRANSFORMS):
            if k == 0:
                a, b = one.fuse_logodds(Ls, geom, t, mode), sh.fuse_logodds(Ls, geom, t, mode)
            elif k == 1:
                a, b = one.fuse_state(sts, geom, t, mode), sh.fuse_state(sts, geom, t, mode)
            else:
                a, b = one.fuse_from(s, t, mode), sh.fuse_from(s, t, mode)
            assert a == b and a["covered"] > 0
            assert np.array_equal(sh.logodds().view(np.uint32), one.logodds().view(np.uint32))
            assert np.array_equal(sh.state(), one.state())
            fa = one.frontiers(want_mask=True, want_labels=True)
            fb = sh.frontiers(want_mask=True, want_labels=True)
            assert np.array_equal(fa.mask, fb.mask) and np.array_equal(fa.labels, fb.labels)
            assert np.array_equal(fa.clusters, fb.clusters)

"""GPU: a fusion keeps every derived structure of the handle right (state,
tile_free, the tile list, fmask, fedge, tile_seen; csrc/dm_internal.h's
INVARIANT): after dm_fuse_* the frontiers, further integrate calls, the planner
and the matcher behave exactly as on a fresh handle given the fused log-odds
with dm_set_logodds."""
import numpy as np
import pytest

import dm
import fuse_cases as fc
from dm import _ffi, match

pytestmark = pytest.mark.gpu


def _fuse(m, name, mode):
    geom, L, _, transform = fc.case(name)
    return m.fuse_logodds(L, geom, transform, mode)


def _assert_same_frontiers(a, b):
    fa = a.frontiers(want_mask=True, want_labels=True)
    fb = b.frontiers(want_mask=True, want_labels=True)
    np.testing.assert_array_equal(fa.mask, fb.mask)
    np.testing.assert_array_equal(fa.labels, fb.labels)
    np.testing.assert_array_equal(fa.clusters, fb.clusters)
    return fa


@pytest.mark.parametrize("fmask", ["on", "off"])
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("name", ["yaw_0.3", "over_top", "yaw_-2.5_coarse"])
def test_frontiers_and_later_scans_match_a_fresh_handle(monkeypatch, name, mode, fmask):
    """over_top writes only tiles no scan has touched (tile_seen 0 before);
    yaw_-2.5_coarse nearly the whole map; yaw_0.3 the explored part's border."""
    monkeypatch.setenv("DM_FMASK", fmask)
    p = fc.dst_params()
    _, _, amin, inc = fc.dst_batches()
    with dm.OccupancyMapper(p) as a, dm.OccupancyMapper(p) as b:
        fc.prefill(a)
        before = a.frontiers(want_mask=True)  # a pass before the fusion: tile list, bit rows and label cache exist
        stats = _fuse(a, name, mode)
        fc.check_stats(name, stats)
        b.set_logodds(a.logodds())
        np.testing.assert_array_equal(a.state(), b.state())
        fr = _assert_same_frontiers(a, b)
        assert len(fr) > 0 and not np.array_equal(fr.mask, before.mask)
        for poses, ranges in fc.more_batches():
            assert a.integrate(poses, ranges, amin, inc) == b.integrate(poses, ranges, amin, inc)
            _assert_same_frontiers(a, b)
        np.testing.assert_array_equal(a.logodds().view(np.uint32), b.logodds().view(np.uint32))
        np.testing.assert_array_equal(a.state(), b.state())


def test_plan_readers_are_stale_after_a_fuse():
    p = fc.dst_params()
    at = tuple(fc.dst_batches()[1][0][0][0][:2])
    with dm.OccupancyMapper(p) as m:
        fc.prefill(m)
        m.plan_field([at], inflate_cells=1)
        m.plan_query([at])
        _fuse(m, "yaw_0.3", "fill")
        for call in (lambda: m.plan_query([at]), m.plan_cost_field):
            with pytest.raises(dm.DmError) as e:
                call()
            assert e.value.code == _ffi.DM_ERR_STATE
        m.plan_field([at], inflate_cells=1)
        m.plan_query([at])


def test_match_scans_after_a_fuse_equals_a_fresh_handle():
    p = fc.dst_params()
    _, batches, amin, inc = fc.dst_batches()
    poses, ranges = batches[-1]
    kern = match.kernel_table(0.1, float(p.resolution), 4)
    args = (poses, ranges, amin, inc, [-0.03, 0.0, 0.03], 1, 2, 4, 2, 4, kern)
    with dm.OccupancyMapper(p) as a, dm.OccupancyMapper(p) as b:
        fc.prefill(a)
        first = a.match_scans(*args, want_volume=True)  # the response field of the map before the fusion
        _fuse(a, "yaw_-2.5_coarse", "add")
        b.set_logodds(a.logodds())
        ga = a.match_scans(*args, want_volume=True)
        gb = b.match_scans(*args, want_volume=True)
        assert np.array_equal(ga["volume"], gb["volume"]) and np.array_equal(ga["best"], gb["best"])
        assert np.array_equal(ga["score"], gb["score"]) and ga["pose"].tobytes() == gb["pose"].tobytes()
        assert not np.array_equal(ga["volume"], first["volume"])  # the field was rebuilt for the fused map

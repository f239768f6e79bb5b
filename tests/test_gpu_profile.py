"""GPU: the profile calls (dm_profile_enable / _read / _reset).  The timers
are recorded on all four streams of a handle (with overlap on, the integrate
front-end on the front-end stream and a begin / end pass's labelling on the
pass stream), read by dm_profile_read and dropped with the handle."""
import math

import pytest

import cases
import dm

pytestmark = pytest.mark.gpu

# one launch per integrate call / frontier pass of this size
KERNELS = ("beam_prep", "plan", "scatter", "tile_accum", "frontier_bits", "frontier_tile", "frontier_resolve",
           "sort_clusters")


def test_profile_counts_every_stream():
    p = cases.make_params(128, 128)
    m = dm.OccupancyMapper(p)
    m.set_overlap(True)
    m.profile(True)
    for k, split in enumerate((True, False)):
        poses, ranges, amin, inc = cases.random_scans(40 + k, p, 2, 64, spread=0.3)
        m.integrate(poses, ranges, amin, inc)
        if split:
            m.frontiers_begin()
            assert m.frontiers_end() is not None
        else:
            m.frontiers()
    stats = m.profile_read()
    print(stats)
    for name in KERNELS:
        assert name in stats, (name, sorted(stats))
        assert stats[name][0] == 2, (name, stats[name])
    for name, (launches, total_ms) in stats.items():
        assert launches > 0 and math.isfinite(total_ms) and total_ms > 0.0, (name, launches, total_ms)
    assert m.profile_read() == stats  # nothing new: the same numbers
    m.profile_reset()
    assert m.profile_read() == {}
    # timers still pending when the handle goes: nothing raised
    poses, ranges, amin, inc = cases.random_scans(42, p, 2, 64, spread=0.3)
    m.integrate(poses, ranges, amin, inc)
    m.close()

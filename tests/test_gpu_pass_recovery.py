"""GPU: the recovery paths of pipelined frontier passes (include/dm.h,
dm_frontiers_end): a pass that overflows the slot arrays has no result
(DM_ERR_INCOMPLETE, *n_out == 0; frontiers_end() returns None and sets
last_incomplete) and the arrays are grown at once, while a second pass may
still be in the ring; a result is "lost to a reallocation or a later pass"
when its device records were reallocated or, unsorted, overwritten.  A pass
is either exactly the oracle's cluster list or None, never anything else, and
the handle recovers: the next synchronous pass and the next pipelined pass
are exact.

`big`: isolated free cells in unknown space on every second row and column of
a 576 x 576 map, one cluster each: 74 583 clusters by the oracle, above the
create-time slot capacity max(65536, 4 * tiles) = 65536, so by pigeonhole the
first pass over it overflows whichever shard region a tile's slots land in.
576 is the smallest multiple of 64 that does it: a lattice cannot be denser
than every second cell without merging clusters, and 512 x 512 holds 65 536
lattice cells, 58 982 of them free.  The floor is asserted on the oracle's count."""
import functools

import numpy as np
import pytest

import cases
import dm
from dm import _ffi
from dm.goals import assign_goals

pytestmark = pytest.mark.gpu

N = 576
SLOT_CAPACITY = max(65536, 4 * (N // 64) ** 2)  # dm_create: max(1 << 16, kSlotsPerTile * tiles)
ROBOTS = ((-10.0, -4.0), (0.0, 0.0), (9.0, 12.0))


def _params():
    return cases.make_params(N, N)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(state, the oracle's clusters of it): computed once, shared, never modified."""
    import oracle

    if name == "big":
        st = cases.sparse_state(1, N, N, step=2)
    elif name == "small":
        st = cases.blob_state(3, N, N, n_blobs=10)
    elif name == "blob":
        st = cases.blob_state(4, N, N, n_blobs=30)
    else:
        st = np.full((N, N), -1, np.int8)
    om = oracle.OracleMap(_params())
    om.state[...] = st
    clusters = om.frontiers(want_mask=False, want_labels=False, cap=1 << 17)[2]
    st.setflags(write=False)
    clusters.setflags(write=False)
    return st, clusters


def test_the_big_state_exceeds_the_slot_capacity(oracle_lib):
    assert len(_case("big")[1]) > SLOT_CAPACITY
    assert 0 < len(_case("small")[1]) < 4096 and 0 < len(_case("blob")[1]) < 4096


def _exact(fr, exp):
    assert fr is not None
    np.testing.assert_array_equal(fr.clusters, exp)


def _exact_or_none(fr, exp):
    if fr is not None:
        np.testing.assert_array_equal(fr.clusters, exp)
    return fr is not None


def _ring_is_empty(m):
    with pytest.raises(dm.DmError) as e:
        m.frontiers_end()
    assert e.value.code == _ffi.DM_ERR_INVALID_ARG


def _recovers(m, exp):
    """After a pass without a result: the synchronous pass is exact, then a
    pipelined one (the arrays have grown), and the ring is empty."""
    _exact(m.frontiers(), exp)
    m.frontiers_begin()
    _exact(m.frontiers_end(), exp)
    _ring_is_empty(m)


def _end_raw(m):
    """dm_frontiers_end through the C ABI: (return code, *n_out)."""
    import ctypes

    buf = np.empty(1 << 17, dtype=np.dtype(_ffi.CLUSTER_DTYPE))
    n = ctypes.c_int64(-1)
    rc = m._lib.dm_frontiers_end(m._handle(), buf.ctypes.data_as(ctypes.c_void_p), buf.shape[0], ctypes.byref(n))
    return rc, int(n.value)


def test_cold_overflow_one_pass(oracle_lib):
    big, exp = _case("big")
    with dm.OccupancyMapper(_params()) as m:
        m.set_state(big)
        m.frontiers_begin()
        assert _end_raw(m) == (_ffi.DM_ERR_INCOMPLETE, 0)
        _recovers(m, exp)
        # ... and through the wrapper, on a fresh handle
    with dm.OccupancyMapper(_params()) as m:
        m.set_state(big)
        m.frontiers_begin()
        assert m.last_incomplete is None
        assert m.frontiers_end() is None
        assert m.last_incomplete
        _recovers(m, exp)


def test_cold_overflow_two_passes(oracle_lib):
    """The first end grows the arrays while the second pass is in the ring:
    the second end must notice (None) or be exact."""
    big, exp = _case("big")
    with dm.OccupancyMapper(_params()) as m:
        m.set_state(big)
        m.frontiers_begin()
        m.frontiers_begin()
        got = [_exact_or_none(m.frontiers_end(), exp) for _ in range(2)]
        assert got[0] is False  # the cold pass overflows for certain
        _ring_is_empty(m)
        m.frontiers_begin()
        _exact(m.frontiers_end(), exp)


@pytest.mark.parametrize("overlap", [False, True])
def test_overflow_behind_a_good_pass_across_a_bulk_write(oracle_lib, overlap):
    """The write must not reach the pass that began before it."""
    big, exp = _case("big")
    small, exp_small = _case("small")
    with dm.OccupancyMapper(_params()) as m:
        m.set_overlap(overlap)
        m.set_state(small)
        m.frontiers_begin()
        m.set_state(big)
        m.frontiers_begin()
        _exact(m.frontiers_end(), exp_small)
        assert m.frontiers_end() is None and m.last_incomplete
        _recovers(m, exp)


def test_unsorted_result_overwritten(oracle_lib):
    """A grown handle whose last collected pass was small sorts the next pass
    with the rank sort (cap 65536): the big passes come back unsorted, as raw
    records shared by every pass, so the first of two is lost to the second
    (None) unless the library can still give it exactly; the last one is
    exact, and the pass after it takes the row sort."""
    big, exp = _case("big")
    small, exp_small = _case("small")
    with dm.OccupancyMapper(_params()) as m:
        m.set_state(big)
        m.frontiers_begin()
        assert m.frontiers_end() is None
        _exact(m.frontiers(), exp)  # grown
        m.set_state(small)
        _exact(m.frontiers(), exp_small)  # the hint is small now
        m.set_state(big)
        m.frontiers_begin()
        m.frontiers_begin()
        _exact_or_none(m.frontiers_end(), exp)
        _exact(m.frontiers_end(), exp)
        _ring_is_empty(m)
        m.frontiers_begin()
        _exact(m.frontiers_end(), exp)


def test_goals_after_a_failed_pass(oracle_lib):
    """dm_assign_goals after a pass without a result raises
    DM_ERR_INVALID_ARG: growing the slot arrays reallocates the device records
    of every readback slot, the list collected before included, so there is no
    collected result on the device any more (it does not fall back to the
    earlier list).  Once a pass is collected again it equals
    dm.goals.assign_goals on that pass's list."""
    big, exp = _case("big")
    small, exp_small = _case("small")
    with dm.OccupancyMapper(_params()) as m:
        m.set_state(small)
        _exact(m.frontiers(), exp_small)
        assert m.assign_goals(ROBOTS, min_size=2) == assign_goals(exp_small, ROBOTS, min_size=2)
        m.set_state(big)
        m.frontiers_begin()
        assert m.frontiers_end() is None
        with pytest.raises(dm.DmError) as e:
            m.assign_goals(ROBOTS, min_size=2)
        assert e.value.code == _ffi.DM_ERR_INVALID_ARG
        _exact(m.frontiers(), exp)
        _exact(m.frontiers(), exp)  # sorted on the device (the row sort, by the hint of the pass before)
        assert m.assign_goals(ROBOTS, min_size=1) == assign_goals(exp, ROBOTS, min_size=1)


@pytest.mark.parametrize("cap", [None, 1 << 17])
def test_goals_after_a_synchronous_overflow_sorted_on_the_device(oracle_lib, monkeypatch, cap):
    """dm_frontiers overflows the slot arrays, grows them and retries inside
    one call, and the retry is sorted on the device (DM_SORT_MIN=8: the small
    pass before it hints the row sort).  cap 1 << 17: the caller's buffer holds
    the result, so that call's device records are the goal source and
    dm_assign_goals must read what the retry wrote, in the synchronous call's
    own readback slot, not in a slot of the ring.  cap None: the wrapper's
    4096-record buffer does not, it calls dm_frontiers again with a larger one,
    and the goals read that second pass, which ran on the grown arrays."""
    monkeypatch.setenv("DM_SORT_MIN", "8")  # read at dm_create
    big, exp = _case("big")
    small, exp_small = _case("small")
    assert len(exp_small) > 8
    with dm.OccupancyMapper(_params()) as m:
        m.set_state(small)
        _exact(m.frontiers(), exp_small)
        m.set_state(big)
        _exact(m.frontiers(cap=cap), exp)
        assert m.assign_goals(ROBOTS, min_size=1) == assign_goals(exp, ROBOTS, min_size=1)
        m.frontiers_begin()
        _exact(m.frontiers_end(), exp)
        _ring_is_empty(m)


def test_hint_cliffs_pipelined(oracle_lib):
    """One handle, overlap on, every pass a begin / end pair, through maps
    whose cluster and tile counts jump both ways: the grids, kernels and sorts
    of each pass follow the hints of the map before it.  Every pass is exact or
    None; after a None one synchronous pass is exact; after each bulk write the
    tile list holds exactly the tiles with a free cell."""
    import oracle

    p, batches, amin, inc = cases.world_case(7, N, N, 0.05, 2, 90, 1)
    om = oracle.OracleMap(p)
    counts = om.integrate(*batches[0], amin, inc)
    exp_scan = om.frontiers(want_mask=False, want_labels=False, cap=1 << 17)[2]
    assert len(exp_scan) > 0
    nones = 0
    with dm.OccupancyMapper(p) as m:
        m.set_overlap(True)

        def one_pass(exp, st=None):
            nonlocal nones
            m.frontiers_begin()
            if not _exact_or_none(m.frontiers_end(), exp):
                nones += 1
                _exact(m.frontiers(), exp)
            if st is not None:
                assert m.last_stats()["frontier_tiles"] == int(cases.tiles_with_free(st).sum())

        for name in ("unknown", "big"):
            m.set_state(_case(name)[0])
            one_pass(_case(name)[1], _case(name)[0])
        m.reset()
        one_pass(_case("unknown")[1], _case("unknown")[0])
        assert m.integrate(*batches[0], amin, inc) == counts
        one_pass(exp_scan)
        for name in ("big", "blob"):
            m.set_state(_case(name)[0])
            one_pass(_case(name)[1], _case(name)[0])
        _ring_is_empty(m)
    assert nones >= 1  # the first pass over `big` overflows the create-time arrays

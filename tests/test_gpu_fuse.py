"""GPU: map fusion (dm_fuse_logodds, dm_fuse_state, dm_fuse_grid) against the
host restatement dm/fuse.py, bit for bit: every case of tests/fuse_cases.py in
both modes from log-odds and from state images, device-to-device fusion, FILL's
idempotence, and the error codes (which leave the map and its version alone)."""
import ctypes

import numpy as np
import pytest

import cases
import dm
import fuse_cases as fc
from dm import _ffi, fuse

pytestmark = pytest.mark.gpu


def _bits(L):
    return np.ascontiguousarray(L, np.float32).view(np.uint32)


def _fuse_case(m, name, mode, kind):
    geom, L, st, transform = fc.case(name)
    if kind == "state":
        return m.fuse_state(st, geom, transform, mode)
    return m.fuse_logodds(L, geom, transform, mode)


@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_fuse_equals_host_restatement(name, mode, kind):
    p = fc.dst_params()
    with dm.OccupancyMapper(p) as m:
        fc.prefill(m)
        L0, st0 = m.logodds(), m.state()
        exp_L, exp_st, exp_stats = fc.expected(L0, p, name, mode, kind)
        stats = _fuse_case(m, name, mode, kind)
        L1, st1 = m.logodds(), m.state()
        print(name, mode, kind, stats)
        assert stats == exp_stats
        assert np.array_equal(_bits(L1), _bits(exp_L))
        assert np.array_equal(st1, exp_st)
        fc.check_stats(name, stats)
        if name == "outside":
            assert np.array_equal(_bits(L1), _bits(L0)) and np.array_equal(st1, st0)
        if mode == "fill":  # idempotent on the device
            again = _fuse_case(m, name, mode, kind)
            assert again == {"covered": stats["covered"], "contributing": 0, "changed": 0}
            assert np.array_equal(_bits(m.logodds()), _bits(L1)) and np.array_equal(m.state(), st1)


@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("name", ["yaw_0.3", "yaw_-2.5_coarse", "over_bottom"])
def test_fuse_grid_equals_fuse_logodds_of_its_logodds(name, mode):
    p = fc.dst_params()
    geom, L, _, transform = fc.case(name)
    sp = cases.make_params(fc.SRC_W, fc.SRC_H, geom["resolution"], origin=(geom["origin_x"], geom["origin_y"]))
    with dm.OccupancyMapper(p) as a, dm.OccupancyMapper(p) as b, dm.OccupancyMapper(sp) as s:
        fc.prefill(a)
        fc.prefill(b)
        s.set_logodds(L)  # its NaN and inf cell included: they read as 0
        got = a.fuse_from(s, transform, mode)
        exp = b.fuse_logodds(s.logodds(), fuse.geom_of(s.params), transform, mode)
        assert got == exp
        fc.check_stats(name, got)
        assert np.array_equal(_bits(a.logodds()), _bits(b.logodds()))
        assert np.array_equal(a.state(), b.state())
        assert np.array_equal(_bits(s.logodds()), _bits(L))  # the source is only read


def _raw(m, fn, src, values, t=(0.0, 0.0, 0.0), mode=0, stats=True):
    out = (ctypes.c_uint64 * 3)()
    return fn(m._handle(), None if src is None else ctypes.byref(src), None if values is None else
              values.ctypes.data_as(ctypes.c_void_p), t[0], t[1], t[2], mode, out if stats else None)


def test_errors_return_codes_and_leave_the_map_alone():
    p = fc.dst_params()
    lib = dm.load_library()
    L = np.ones((fc.SRC_H, fc.SRC_W), np.float32)
    st = np.zeros((fc.SRC_H, fc.SRC_W), np.int8)
    nan, inf = float("nan"), float("inf")

    def src(**kw):
        g = dict(width=fc.SRC_W, height=fc.SRC_H, resolution=0.05, origin_x=-1.0, origin_y=-1.0)
        g.update(kw)
        return _ffi.DmFuseSource(g["width"], g["height"], g["resolution"], g["origin_x"], g["origin_y"])

    with dm.OccupancyMapper(p) as m, dm.OccupancyMapper(p, devices=[0, 0]) as sh, \
            dm.OccupancyMapper(cases.make_params(128, 128, band_row0=64, band_rows=64)) as band:
        fc.prefill(m)
        at = tuple(fc.dst_batches()[1][0][0][0][:2])  # a robot's position: a free cell
        m.plan_field([at], inflate_cells=0)  # valid for this map version only
        L0, st0 = m.logodds(), m.state()
        bad = _ffi.DM_ERR_INVALID_ARG
        for fn, values in ((lib.dm_fuse_logodds, L), (lib.dm_fuse_state, st)):
            assert fn(None, ctypes.byref(src()), values.ctypes.data_as(ctypes.c_void_p), 0.0, 0.0, 0.0, 0, None) == bad
            assert _raw(m, fn, None, values) == bad
            assert _raw(m, fn, src(), None) == bad
            for kw in (dict(width=0), dict(width=32769), dict(height=0), dict(height=32769), dict(resolution=0.0),
                       dict(resolution=-0.05), dict(resolution=nan), dict(resolution=inf), dict(origin_x=nan),
                       dict(origin_y=-inf)):
                assert _raw(m, fn, src(**kw), values) == bad, kw
            for t in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, nan), (0.0, 0.0, -inf)):
                assert _raw(m, fn, src(), values, t=t) == bad, t
            for mode in (-1, 2):
                assert _raw(m, fn, src(), values, mode=mode) == bad
                assert _raw(sh, fn, src(), values, mode=mode) == bad
        out = (ctypes.c_uint64 * 3)()
        for other in (None, m._handle(), sh._handle(), band._handle()):
            assert lib.dm_fuse_grid(m._handle(), other, 0.0, 0.0, 0.0, 0, out) == bad
        assert lib.dm_fuse_grid(None, m._handle(), 0.0, 0.0, 0.0, 0, out) == bad
        assert lib.dm_fuse_grid(m._handle(), band._handle(), 0.0, 0.0, nan, 0, out) == bad
        assert np.array_equal(_bits(m.logodds()), _bits(L0)) and np.array_equal(m.state(), st0)
        m.plan_query([at])  # the map version did not move: the field is still valid
        # and a successful call with no stats buffer works, moving the version
        assert _raw(m, lib.dm_fuse_logodds, src(), L, stats=False) == 0
        with pytest.raises(dm.DmError) as e:
            m.plan_query([at])
        assert e.value.code == _ffi.DM_ERR_STATE

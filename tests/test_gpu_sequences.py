"""GPU: whole call sequences against the host model (tests/seq_model.py).

The other GPU tests pin one derived structure of a handle each, with one map
writer on a quiescent handle and a synchronous pass behind it.  Here the bulk
writers (set_state, set_logodds, reset, load, the three fusions) run while
pipelined frontier passes are pending, with the overlapped front-end on and
off, between integrate calls, synchronous passes and readers: the
stream ordering of each writer, the tile list's rebuilds, the frontier bit
records, the label cache and the grids and kernels chosen from the hints of
a map that no longer exists are checked composed.

Each committed sequence is replayed on the device and on the model, and after
every op what the device returns must equal the model's, bit for bit: U / T
and the fusion statistics, every collected pipelined pass (the oracle's
clusters of the map as it was at that pass's begin), every synchronous pass
(mask, labels, clusters), every reader (its host restatement on the model's
map), plan_query's DM_ERR_STATE after a map change if a field existed, and at
the end the log-odds (as uint32) and the state.

The label cache's counters: a tile with frontier cells that the workgroup
tile kernel labels is a hit or a miss, so with DM_FRONTIER_KERNEL=wg every
collected pass with clusters must report hits + misses > 0 (a pass cannot
skip the workgroup kernel unnoticed).  With the wave kernel (forced, or
chosen by auto for sparse passes) only run-rich tiles reach the workgroup
kernel (tests/test_gpu_frontier_cache.py), so no count is asserted there.
A sharded handle reports the sum over its bands' last passes, which belong to
the collected pass only when that pass was synchronous.

For the sharded handle the replay skips the readers that need one handle over
the whole map; the sequence itself is the same for both handle kinds."""
import numpy as np
import pytest

import dm
import seq_model as sm
from dm import _ffi

pytestmark = pytest.mark.gpu

_DEVICE_BATCHES = {}


def _device_batch(i):
    """(pose4, ranges) of integrate batch i on the device: made once, complete
    before any call uses them (overlap mode reads them on another stream)."""
    if i not in _DEVICE_BATCHES:
        import torch
        from dm import synth

        poses, ranges, _, _ = sm.batch(i)
        _DEVICE_BATCHES[i] = (torch.from_numpy(synth.pose4(poses)).cuda(),
                              torch.from_numpy(np.ascontiguousarray(ranges)).cuda())
        torch.cuda.synchronize()
    return _DEVICE_BATCHES[i]


def _eq(got, exp, where):
    np.testing.assert_array_equal(got, exp, err_msg=where)


def replay(m, src, seed, tmp_path, sharded, check_cache):
    ops, exps, L_end, st_end, _ = sm.expectations(seed)
    assert dm.load_library().dm_max_passes_in_flight() == sm.default_max_pending()
    kern = sm.match_kernel()

    def collected(fr, exp, where, pipelined=False):
        assert fr is not None, where + f": no result ({m.last_incomplete})"
        _eq(fr.clusters, exp["clusters"], where)
        # a sharded handle reports its bands' last passes (include/dm.h), which
        # are this pass only if it was a synchronous one
        if check_cache and len(exp["clusters"]) and not (sharded and pipelined):
            hits, misses = m.frontier_cache_stats()
            assert hits + misses > 0, where + f": label cache hits {hits}, misses {misses}"

    for i, (op, exp) in enumerate(zip(ops, exps)):
        kind = op[0]
        where = f"seed {seed} op {i} {op}, after {ops[max(0, i - 4):i]}"
        if kind == "integrate":
            assert m.integrate(*sm.batch(op[1])) == exp["counts"], where
        elif kind == "integrate_device":
            pose4, rng = _device_batch(op[1])
            _, ranges, amin, inc = sm.batch(op[1])
            m.integrate_device(pose4.data_ptr(), pose4.shape[0], rng.data_ptr(), ranges.shape[1], amin, inc)
            assert m.last_counts() == exp["counts"], where
        elif kind == "set_state":
            m.set_state(sm.state_image(*op[1:]))
        elif kind == "set_logodds":
            m.set_logodds(sm.logodds_image(*op[1:]))
        elif kind == "reset":
            m.reset()
        elif kind == "save":
            m.save(str(tmp_path / f"ck{exp['slot']}.dmap"))
        elif kind == "load":
            m.load(str(tmp_path / f"ck{op[1]}.dmap"))
        elif kind in ("fuse_logodds", "fuse_state", "fuse_from"):
            geom, L, st, transform = sm.fc.case(op[1])
            if kind == "fuse_logodds":
                stats = m.fuse_logodds(L, geom, transform, op[2])
            elif kind == "fuse_state":
                stats = m.fuse_state(st, geom, transform, op[2])
            else:
                stats = m.fuse_from(src, transform, op[2])
            assert stats == exp["stats"], where
        elif kind == "frontiers":
            fr = m.frontiers(want_mask=bool(op[1]), want_labels=bool(op[1]))
            if op[1]:
                _eq(fr.mask, exp["mask"], where)
                _eq(fr.labels, exp["labels"], where)
            collected(fr, exp, where)
        elif kind == "begin":
            m.frontiers_begin()
        elif kind == "end":
            collected(m.frontiers_end(), exp, where, pipelined=True)
        elif kind == "set_overlap":
            m.set_overlap(bool(op[1]))
        elif kind == "map_image":
            _eq(m.map_image(), exp["image"], where)
        elif kind == "assign_goals":
            assert m.assign_goals(sm.ROBOTS, min_size=sm.GOAL_MIN_SIZE) == exp["goals"], where
        elif sharded:
            assert kind in sm.WHOLE_MAP_READERS, where
        elif kind == "match_field":
            _eq(m.match_field(sm.SMEAR, kern), exp["field"], where)
        elif kind == "plan_traversable":
            _eq(m.plan_traversable(sm.INFLATE), exp["trav"], where)
        elif kind == "plan_field":
            m.plan_field([sm.PLAN_AT], inflate_cells=sm.INFLATE)
            _eq(m.plan_cost_field(), exp["cost"], where)
            m.plan_query([sm.PLAN_AT])
        else:
            raise AssertionError(where)
        if exp.get("field_stale") and not sharded:
            with pytest.raises(dm.DmError) as e:
                m.plan_query([sm.PLAN_AT])
            assert e.value.code == _ffi.DM_ERR_STATE, where
    _eq(m.logodds().view(np.uint32), L_end.view(np.uint32), f"seed {seed}: final log-odds")
    _eq(m.state(), st_end, f"seed {seed}: final state")


def _run(monkeypatch, tmp_path, seed, kind, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = sm.fc.dst_params()
    devices = [0, 0] if kind == "sharded" else None
    check_cache = env.get("DM_FRONTIER_KERNEL") == "wg" and env.get("DM_FRONTIER_CACHE", "on") == "on"
    with dm.OccupancyMapper(p, devices=devices) as m, dm.OccupancyMapper(sm.source_params()) as src:
        src.set_logodds(sm.fc.source(0.05)[1])
        replay(m, src, seed, tmp_path, kind == "sharded", check_cache)


@pytest.mark.parametrize("kind", ["single", "sharded"])
@pytest.mark.parametrize("kernel", ["auto", "wg", "wave"])
@pytest.mark.parametrize("fmask", ["on", "off"])
@pytest.mark.parametrize("seed", sm.SEEDS)
def test_sequence(oracle_lib, monkeypatch, tmp_path, seed, fmask, kernel, kind):
    _run(monkeypatch, tmp_path, seed, kind, {"DM_FMASK": fmask, "DM_FRONTIER_KERNEL": kernel})


@pytest.mark.parametrize("kind", ["single", "sharded"])
@pytest.mark.parametrize("kernel", ["auto", "wg", "wave"])
@pytest.mark.parametrize("fmask", ["on", "off"])
def test_sequence_without_the_label_cache(oracle_lib, monkeypatch, tmp_path, fmask, kernel, kind):
    _run(monkeypatch, tmp_path, sm.SEEDS[0], kind,
         {"DM_FMASK": fmask, "DM_FRONTIER_KERNEL": kernel, "DM_FRONTIER_CACHE": "off"})


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_sequence_through_both_sorts(oracle_lib, monkeypatch, tmp_path, seed):
    """DM_SORT_MIN=8: the passes with more than 8 clusters hint the row sort
    for the next one, the others the rank sort, so both sorts see the same
    small passes alternately."""
    _run(monkeypatch, tmp_path, seed, "single", {"DM_SORT_MIN": "8"})

"""CPU: the sequence generator of tests/seq_model.py meets its coverage
floors for every committed seed, on the model alone (no device).  The floors
are what makes the replay on the device (tests/test_gpu_sequences.py) worth
its time: a sequence that misses one is repaired by changing the generator's
weights, never the floor."""
import numpy as np
import pytest

import seq_model as sm


@pytest.fixture(scope="module", params=sm.SEEDS)
def run(request, oracle_lib):
    seed = request.param
    ops, exps, L, st, log = sm.expectations(seed)
    return seed, ops, exps, log


def test_sequences_are_reproducible_and_distinct(oracle_lib):
    seqs = [sm.sequence(s) for s in sm.SEEDS]
    assert len(set(seqs)) == len(seqs)
    for s, ops in zip(sm.SEEDS, seqs):
        assert len(ops) == sm.N_OPS
        sm.sequence.cache_clear()
        assert sm.sequence(s) == ops


def test_every_bulk_kind_with_one_and_with_two_passes_pending(run):
    _, _, _, log = run
    for kind in sm.BULK:
        seen = {r["pending"] for r in log if r["kind"] == kind}
        assert {1, 2} <= seen, (kind, seen)


def test_every_bulk_kind_with_overlap_on_and_off(run):
    _, _, _, log = run
    for kind in sm.BULK:
        seen = {r["overlap"] for r in log if r["kind"] == kind}
        assert seen == {True, False}, (kind, seen)


def test_every_writer_changes_the_frontier_mask(run):
    _, ops, _, log = run
    for op, r in zip(ops, log):
        if r["kind"] in sm.WRITERS:
            assert r["mask_changed"], op


def test_collected_passes(run):
    """At least half of the collected passes (pipelined, and pipelined and
    synchronous together) have clusters; one pipelined pass at least is
    collected after two or more writers; begin never exceeds the ring."""
    _, ops, _, log = run
    ends = [r for r in log if r["kind"] == "end"]
    both = ends + [r for r in log if r["kind"] == "frontiers"]
    assert len(ends) >= 4
    assert 2 * sum(r["clusters"] > 0 for r in ends) >= len(ends)
    assert 2 * sum(r["clusters"] > 0 for r in both) >= len(both)
    assert any(r["writers"] >= 2 for r in ends)
    assert max(r["pending"] for r in log) <= sm.default_max_pending()
    assert all(r["pending"] < sm.default_max_pending() for r in log if r["kind"] == "begin")
    assert all(r["pending"] > 0 for r in log if r["kind"] == "end")


def test_an_integrate_directly_follows_every_writer_kind(run):
    _, ops, _, _ = run
    followed = {a[0] for a, b in zip(ops, ops[1:]) if b[0] in ("integrate", "integrate_device")}
    assert set(sm.WRITERS) <= followed, set(sm.WRITERS) - followed


def test_the_other_ops_occur(run):
    """Both integrate entry points, both synchronous pass forms, overlap
    toggled with a pass pending, every reader, the three named fusion cases in
    both modes across the seeds' writers, a set_logodds image with cells at
    both clamps, and a field made stale by a writer."""
    _, ops, exps, log = run
    kinds = {op[0] for op in ops}
    assert {"integrate", "integrate_device", "begin", "end", "set_overlap"} <= kinds
    assert set(sm.READERS) <= kinds
    assert {op[1] for op in ops if op[0] == "frontiers"} == {0, 1}
    assert any(r["kind"] == "set_overlap" and r["pending"] > 0 for r in log)
    assert any(e.get("field_stale") for e in exps)


def test_fusion_cases_and_images_across_the_seeds(oracle_lib):
    ops = [op for s in sm.SEEDS for op in sm.sequence(s)]
    fused = {(op[1], op[2]) for op in ops if op[0] in ("fuse_logodds", "fuse_state")}
    for name in ("yaw_0.3", "over_top", "yaw_-2.5_coarse"):
        assert {(name, "add"), (name, "fill")} <= fused, (name, fused)
    assert {op[1] for op in ops if op[0] == "set_state"} == {"blob", "random", "unknown"}
    assert "clamps" in {op[1] for op in ops if op[0] == "set_logodds"}
    p = sm.fc.dst_params()
    L = sm.logodds_image("clamps", 6)
    assert (L == np.float32(p.l_min)).any() and (L == np.float32(p.l_max)).any()

"""Host model of one map handle under a sequence of calls, and the seeded
generator of such sequences (tests/test_seq_model.py checks the generator on
the CPU, tests/test_gpu_sequences.py replays the sequences on the device).

A sequence interleaves the bulk map writers (set_state, set_logodds, reset,
load, the three fusions) and checkpoint saves with integrate calls,
synchronous frontier passes, pipelined passes (begin / end, up to
dm_max_passes_in_flight() pending), overlap toggles and readers.  The model
holds the CPU oracle's map, a FIFO with the clusters each pending pass must
return (the oracle's at the moment of its begin), the saved checkpoints, and
what the library documents about two pieces of handle state:

* the distance field is stale after any map change (plan_query: DM_ERR_STATE);
* assign_goals reads the last collected cluster list while its readback slot
  still holds it: the synchronous passes have a slot of their own, pipelined
  pass k uses ring slot k mod dm_max_passes_in_flight(), and a begin into
  the slot of the last collected list drops it.  The generator emits
  assign_goals only while the list is held.

An op is a tuple (kind, *args) of names and small integers; the arrays behind
the names come from the functions below (shared, never modified), so a
sequence is plain data and is the same for every handle kind.

The map is fuse_cases.dst_params(): 200 x 136 cells, 4 x 3 tiles, ragged on
both axes.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import cases
import fuse_cases as fc
from dm import fuse, goals, match, plan

SEEDS = (101, 202, 303)
N_OPS = 64

# the calls that replace or fold into the whole map
WRITERS = ("set_state", "set_logodds", "reset", "load", "fuse_logodds", "fuse_state", "fuse_from")
# ... and save, a bulk read of the map with passes in flight: it has the
# pending / overlap floors of a writer, but cannot change the frontier mask
BULK = WRITERS + ("save",)
READERS = ("map_image", "match_field", "plan_traversable", "assign_goals", "plan_field")
# readers that need one handle covering the whole map (a sharded handle refuses them)
WHOLE_MAP_READERS = ("match_field", "plan_traversable", "plan_field")

FUSE_NAMES = ("yaw_0.3", "over_top", "yaw_-2.5_coarse")
FUSE_FROM_NAMES = ("yaw_0.3", "over_top", "quarter_turn")  # sources at the second handle's resolution, 0.05
STATE_IMAGES = tuple([("blob", s) for s in (1, 2, 3)] + [("random", s) for s in (4, 5)] + [("unknown", 0)])
LOGODDS_IMAGES = (("scans", 0), ("clamps", 6), ("clamps", 7))

ROBOTS = ((-3.0, -2.0), (0.0, 0.0), (2.5, 1.5))
GOAL_MIN_SIZE = 2
SMEAR = 4
INFLATE = 2
PLAN_AT = (-3.0, -2.0)
CLUSTER_CAP = 1 << 13  # the oracle's record buffer: a 200 x 136 map has at most 6800 clusters


def n_batches():
    return len(fc.dst_batches()[1]) + len(fc.more_batches())


def batch(i):
    """(poses, ranges, angle_min, angle_increment) of integrate batch i."""
    _, first, amin, inc = fc.dst_batches()
    poses, ranges = (first + fc.more_batches())[i]
    return poses, ranges, amin, inc


@functools.lru_cache(maxsize=None)
def state_image(kind, seed):
    if kind == "blob":
        st = cases.blob_state(seed, fc.DST_H, fc.DST_W, n_blobs=6)
    elif kind == "random":
        st = cases.random_state(seed, fc.DST_H, fc.DST_W)
    else:
        st = np.full((fc.DST_H, fc.DST_W), -1, np.int8)
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def logodds_image(kind, seed):
    """"scans": the pre-filled destination of the fusion tests; "clamps": a
    blocky random image of the values 0, l_free, l_occ, l_min and l_max."""
    if kind == "scans":
        return fc.dst_logodds()
    p = fc.dst_params()
    rng = np.random.Generator(np.random.PCG64(seed))
    values = np.array([0.0, 0.0, p.l_free, p.l_free, p.l_occ, p.l_min, p.l_max], np.float32)
    coarse = rng.integers(0, len(values), (-(-fc.DST_H // 8), -(-fc.DST_W // 8)))
    L = np.ascontiguousarray(values[np.kron(coarse, np.ones((8, 8), np.int64))][:fc.DST_H, :fc.DST_W])
    assert (L == np.float32(p.l_min)).any() and (L == np.float32(p.l_max)).any()
    L.setflags(write=False)
    return L


def source_params():
    """The second handle (fuse_from's source): fuse_cases.source(0.05)'s map."""
    geom, _, _ = fc.source(0.05)
    return cases.make_params(fc.SRC_W, fc.SRC_H, geom["resolution"], origin=(geom["origin_x"], geom["origin_y"]))


def match_kernel():
    return match.kernel_table(0.1, float(fc.dst_params().resolution), SMEAR)


class Model:
    """The expected behaviour of one handle.  apply(op) advances the model and
    returns what the device must return for that op; `log` keeps one record
    per op for the coverage floors."""

    def __init__(self, max_pending):
        import oracle

        self.p = fc.dst_params()
        self.om = oracle.OracleMap(self.p)
        self._scratch = oracle.OracleMap(self.p)
        self.max_pending = int(max_pending)
        self.pending = collections.deque()  # dicts: clusters, writers since the begin
        self.checkpoints = []
        self.overlap = False
        self.collected = None    # the last collected cluster list
        self.goal_slot = None    # the readback slot that holds it, None: dropped
        self.ring_head = 0
        self.field_valid = False
        self.log = []

    # -- helpers ----------------------------------------------------------
    def mask(self):
        return self.om.frontiers(want_labels=False, cap=CLUSTER_CAP)[0]

    def mask_of(self, L):
        self._scratch.set_logodds(L)
        return self._scratch.frontiers(want_labels=False, cap=CLUSTER_CAP)[0]

    def clusters(self):
        clusters = self.om.frontiers(want_mask=False, want_labels=False, cap=CLUSTER_CAP)[2]
        assert len(clusters) < CLUSTER_CAP
        return clusters

    def goal_held(self):
        return self.goal_slot is not None

    def written(self, op):
        """(L', stats or None): the map a bulk writer leaves."""
        kind = op[0]
        p = self.p
        if kind == "set_state":
            st = state_image(*op[1:])
            L = np.where(st == 100, np.float32(p.l_occ), np.where(st == 0, np.float32(p.l_free), np.float32(0)))
            return L.astype(np.float32), None
        if kind == "set_logodds":
            return logodds_image(*op[1:]), None
        if kind == "reset":
            return np.zeros_like(self.om.L), None
        if kind == "load":
            return self.checkpoints[op[1]], None
        name, mode = op[1:]
        geom, Ls, sts, transform = fc.case(name)
        if kind == "fuse_state":
            L, _, stats = fuse.fuse_map(self.om.L, p, sts, geom, transform, mode, src_is_state=True)
        else:  # fuse_logodds, and fuse_from a handle that holds the same log-odds
            L, _, stats = fuse.fuse_map(self.om.L, p, Ls, geom, transform, mode)
        return L, stats

    # -- one op -----------------------------------------------------------
    def apply(self, op):
        kind = op[0]
        rec = {"kind": kind, "pending": len(self.pending), "overlap": self.overlap}
        exp = {}
        changes_map = kind in WRITERS or kind in ("integrate", "integrate_device")
        if changes_map:
            # plan_query must now refuse a field computed before this op
            exp["field_stale"] = self.field_valid
            self.field_valid = False
        if kind in ("integrate", "integrate_device"):
            exp["counts"] = self.om.integrate(*batch(op[1]))
        elif kind in WRITERS:
            before = self.mask()
            L, stats = self.written(op)
            self.om.set_logodds(L)
            if kind == "set_state":
                assert np.array_equal(self.om.state, state_image(*op[1:]))
            if stats is not None:
                exp["stats"] = stats
            rec["mask_changed"] = not np.array_equal(before, self.mask())
            for q in self.pending:
                q["writers"] += 1
        elif kind == "save":
            exp["slot"] = len(self.checkpoints)
            self.checkpoints.append(self.om.L.copy())
        elif kind == "frontiers":
            dense = bool(op[1])
            mask, labels, clusters = self.om.frontiers(want_mask=dense, want_labels=dense, cap=CLUSTER_CAP)
            exp.update(mask=mask, labels=labels, clusters=clusters)
            self.collected, self.goal_slot = clusters, "sync"
            rec["clusters"] = len(clusters)
        elif kind == "begin":
            assert len(self.pending) < self.max_pending
            slot = (self.ring_head + len(self.pending)) % self.max_pending
            if self.goal_slot == slot:
                self.goal_slot = None  # the pass rewrites the slot's records
            self.pending.append({"clusters": self.clusters(), "writers": 0})
        elif kind == "end":
            q = self.pending.popleft()
            exp["clusters"] = q["clusters"]
            self.collected, self.goal_slot = q["clusters"], self.ring_head
            self.ring_head = (self.ring_head + 1) % self.max_pending
            rec["clusters"] = len(q["clusters"])
            rec["writers"] = q["writers"]
        elif kind == "set_overlap":
            self.overlap = bool(op[1])
        elif kind == "map_image":
            exp["image"] = self.om.map_image()
        elif kind == "match_field":
            exp["field"] = match.response_field(self.om.state, SMEAR, match_kernel())
        elif kind == "plan_traversable":
            exp["trav"] = plan.traversable(self.om.state, INFLATE)
        elif kind == "plan_field":
            p = self.p
            src = plan.cell_of(*PLAN_AT, p.origin_x, p.origin_y, p.resolution, int(p.width), int(p.height))
            exp["cost"] = plan.field(self.om.state, [src], INFLATE)
            self.field_valid = True
        elif kind == "assign_goals":
            assert self.goal_held()
            exp["goals"] = goals.assign_goals(self.collected, ROBOTS, min_size=GOAL_MIN_SIZE)
        else:
            raise ValueError(f"unknown op {op!r}")
        self.log.append(rec)
        return exp


def default_max_pending():
    import dm

    return int(dm.load_library().dm_max_passes_in_flight())


def _least_used(rng, used, items):
    """`items` in random order, those the sequence has used least first."""
    items = [items[i] for i in rng.permutation(len(items))]
    return sorted(items, key=lambda it: used[it])


def _bulk_candidates(rng, kind, m, used):
    if kind == "set_state":
        return [(kind, *im) for im in _least_used(rng, used, STATE_IMAGES)]
    if kind == "set_logodds":
        return [(kind, *im) for im in _least_used(rng, used, LOGODDS_IMAGES)]
    if kind == "load":
        return [(kind, int(i)) for i in rng.permutation(len(m.checkpoints))]
    if kind in ("reset", "save"):
        return [(kind,)]
    # the two host fusions share their count: every named case in both modes between them
    names = FUSE_FROM_NAMES if kind == "fuse_from" else FUSE_NAMES
    tag = "from" if kind == "fuse_from" else "host"
    combos = [(tag, n, mode) for n in names for mode in fc.MODES]
    return [(kind, n, mode) for _, n, mode in _least_used(rng, used, combos)]


def _pick_bulk(rng, m, kind, used):
    """An op of this bulk kind for the model's present map, or None: a writer
    must change the oracle's frontier mask, a checkpoint must hold a map."""
    if kind == "save":
        return (kind,) if (m.om.L != 0).any() else None
    before = m.mask()
    for op in _bulk_candidates(rng, kind, m, used):
        if not np.array_equal(m.mask_of(m.written(op)[0]), before):
            return op
    return None


@functools.lru_cache(maxsize=None)
def sequence(seed, n_ops=N_OPS, max_pending=None):
    """The op list of a seed (a tuple of tuples), drawn from PCG64(seed).

    The floors of tests/test_seq_model.py are met by construction: every bulk
    kind has two obligations, one with one pass pending and one with two, one
    of them with overlap on and the other with it off (which way round is
    drawn per kind), and the first occurrence of every writer kind is followed
    by an integrate call.  The obligations are taken in random order, those
    of the present overlap mode first; begin / end / set_overlap ops bring the
    handle into an obligation's situation, and ops drawn by weight (readers,
    synchronous passes, integrate calls, further begins, ends, toggles and
    bulk ops) fill the rest of the sequence around them."""
    if max_pending is None:
        max_pending = default_max_pending()
    assert max_pending >= 2
    rng = np.random.Generator(np.random.PCG64(seed))
    m = Model(max_pending)
    ops = []
    used = collections.Counter()  # images, fusion cases, readers and pass forms so far
    int_owed = set(WRITERS)

    def emit(op):
        kind = op[0]
        if kind in ("set_state", "set_logodds"):
            used[op[1:]] += 1
        elif kind in ("fuse_logodds", "fuse_state", "fuse_from"):
            used[("from" if kind == "fuse_from" else "host", *op[1:])] += 1
        m.apply(op)
        ops.append(op)
        if kind in int_owed:
            int_owed.discard(kind)
            emit(integrate_op())

    def integrate_op():
        return ("integrate" if rng.random() < 0.5 else "integrate_device", int(rng.integers(n_batches())))

    def filler():
        npend = len(m.pending)
        weights = {"reader": 2.2, "frontiers": 0.8, "integrate": 0.5, "set_overlap": 0.25, "bulk": 0.4,
                   "begin": 0.6 if npend < max_pending else 0.0, "end": 0.6 if npend else 0.0}
        names = list(weights)
        w = np.array([weights[k] for k in names])
        cat = names[rng.choice(len(names), p=w / w.sum())]
        if cat == "reader":
            kind = _least_used(rng, used, [k for k in READERS if k != "assign_goals" or m.goal_held()])[0]
            used[kind] += 1
            emit((kind,))
        elif cat == "frontiers":
            dense = _least_used(rng, used, [("frontiers", 0), ("frontiers", 1)])[0]
            used[dense] += 1
            emit(dense)
        elif cat == "integrate":
            emit(integrate_op())
        elif cat == "set_overlap":
            emit(("set_overlap", int(not m.overlap)))
        elif cat == "bulk":
            op = _pick_bulk(rng, m, BULK[rng.integers(len(BULK))], used)
            if op is not None:
                emit(op)
        else:
            emit((cat,))

    todo = []
    for kind in BULK:
        first_on = bool(rng.integers(2))
        todo += [(kind, 1, first_on), (kind, 2, not first_on)]
    todo = [todo[i] for i in rng.permutation(len(todo))]
    emit(("integrate", 0))
    emit(("integrate_device", 1))
    deferred = 0
    while todo and len(ops) < n_ops:
        # room for fillers: an obligation takes up to four ops (toggle, begin or end, the op, an integrate)
        while len(ops) + 4 * len(todo) + 2 < n_ops and rng.random() < 0.55:
            filler()
        todo.sort(key=lambda t: t[2] != m.overlap)  # stable: this overlap mode's first
        kind, npend, overlap = todo[0]
        if overlap != m.overlap:
            emit(("set_overlap", int(overlap)))
        while len(m.pending) < npend:
            emit(("begin",))
        while len(m.pending) > npend:
            emit(("end",))
        op = _pick_bulk(rng, m, kind, used)
        if op is None:  # e.g. a load before the first save: later
            todo.append(todo.pop(0))
            deferred += 1
            assert deferred < 64, todo
            if len(todo) == 1 or deferred % 4 == 0:
                filler()
            continue
        todo.pop(0)
        emit(op)
    while len(ops) < n_ops:
        filler()
    assert not todo and not int_owed, (todo, int_owed)
    return tuple(ops[:n_ops])


@functools.lru_cache(maxsize=None)
def expectations(seed, n_ops=N_OPS, max_pending=None):
    """(ops, what the device must return for each op, the final log-odds and
    state, the model's log): computed once per seed, shared and never modified."""
    if max_pending is None:
        max_pending = default_max_pending()
    ops = sequence(seed, n_ops, max_pending)
    m = Model(max_pending)
    exps = tuple(m.apply(op) for op in ops)
    L, st = m.om.L.copy(), m.om.state.copy()
    L.setflags(write=False)
    st.setflags(write=False)
    return ops, exps, L, st, tuple(m.log)


def histogram(seed):
    return dict(sorted(collections.Counter(op[0] for op in sequence(seed)).items()))

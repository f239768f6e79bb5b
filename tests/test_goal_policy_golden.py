"""CPU: the host restatements of the four goal policies (dm.goals, dm.plan,
dm.gain: what the GPU tests compare the device with) against results recorded
before the policies were folded into one loop
(tests/golden/goal_policy_golden.npz, written by make_goal_policy_golden.py).
Exact: indices, cells and gains as integers, goals by their bytes, claimed sets
as packed bitmaps."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_goal_policy_golden",
                                                  os.path.join(GOLDEN_DIR, "make_goal_policy_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN_DIR, "goal_policy_golden.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_file_covers_what_the_issue_lists(golden):
    keys = set(golden)
    for world in gen.WORLDS:
        assert any(k.startswith(world + "/") for k in keys), world
    for k in ("doorways/coord/none/claimed", "doorways/coord/held/idx", "doorways/coord/alone/gain",
              "sliver/path/cell", "sliver/gain/gain", "world/path/set0/idx", "world/gain/set1/gain",
              "world/coord/set1/held/claimed", "world/coord/one_robot/none/idx",
              "world/coord/no_clusters/held/claimed", "world/euclid/set0/idx", "ties/euclid/idx"):
        assert k in keys, k
    assert list(golden["doorways/coord/none/idx"]) == [1, 2] and list(golden["doorways/coord/none/gain"]) == [2211, 448]
    assert int(np.unpackbits(golden["doorways/coord/none/claimed"]).sum()) == 2659
    # no clusters: no goals, and the claimed set is the held views'
    assert (golden["world/coord/no_clusters/held/idx"] == -1).all()
    assert np.unpackbits(golden["world/coord/no_clusters/held/claimed"]).sum() > 0
    assert np.unpackbits(golden["world/coord/no_clusters/none/claimed"]).sum() == 0


@pytest.mark.parametrize("world", gen.WORLDS)
def test_current_code_reproduces_the_record(golden, world):
    now = gen.compute(world)
    want = {k: v for k, v in golden.items() if k.startswith(world + "/")}
    assert sorted(now) == sorted(want)
    for k, w in want.items():
        g = np.asarray(now[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if k.endswith("/xy"):
            assert g.tobytes() == w.tobytes(), k  # the same doubles, NaN for "no goal" included
        elif k.endswith("/kw"):
            assert str(g) == str(w), k
        else:  # idx, cell, gain: int64; claimed: np.packbits
            assert g.dtype in (np.int64, np.uint8), k
            np.testing.assert_array_equal(g, w, err_msg=k)

"""CPU: the host restatement of the whole-window relocalisation
(dm.match.match_global, global_params) against the matcher's restatement and
on the recovery case with a prior 2.9 m and 0.9 rad off."""
import math

import numpy as np

import cases
import match_cases
import match_global_cases as mgc
from dm import match


def test_recovery_case_far_prior():
    """A = 64 over the full circle, half 100, r = 4, sigma = 0.1: the true pose
    is found to the cell from a prior off by (2.3, -1.7, 0.9)."""
    c = mgc.recovery()
    got = mgc.recovery_host(100)
    k, i, j = (int(v) for v in got["best"][0])
    pose = got["pose"][0]
    resp = int(got["score"][0]) / (255.0 * int(got["n_used"][0]))
    print(f"best (k, i, j) = {(k, i, j)}, pose {pose.tolist()}, true {c['true']}, response {resp:.3f}")
    assert (i, j) == (-46, 34)
    res = float(c["p"].resolution)
    assert abs(pose[0] - c["true"][0]) <= res and abs(pose[1] - c["true"][1]) <= res
    assert match_cases.yaw_error(pose[2], c["true"][2]) <= 0.5 * (2.0 * math.pi / 64)
    assert resp >= 0.8


def test_equals_match_scans_on_a_small_window():
    p, st, ranges, amin, inc, true, prior = match_cases.recovery_case()
    kern = match.kernel_table(0.1, 0.05, 4)
    V = match.response_field(st, 4, kern)
    off = np.array([-0.07, -0.03, 0.0, 0.02, 0.09])
    exp = match.match_scans(st, p, [prior], ranges, amin, inc, off, 2, 1, 7, 1, 4, kern, field=V)
    got = match.match_global(st, p, [prior], ranges, amin, inc, off, 2, 7, 7, 4, kern, field=V)
    for name in ("best", "score", "n_used"):
        np.testing.assert_array_equal(got[name], exp[name])
    assert got["pose"].tobytes() == exp["pose"].tobytes()
    assert got["score"][0] > 0


def test_ragged_window_equals_the_cropped_volume_with_ties():
    """half_x != half_y, endpoints out of the grid, a real tie: the volume of
    the square window cropped to the rows of the ragged one, reduced by the
    SPEC's tuple."""
    st = mgc.ragged_map()
    p = cases.make_params(96, 128)
    ranges, amin, inc = mgc.ragged_scans()
    kw = mgc.RAGGED
    got = match.match_global(st, p, [mgc.RAGGED_PRIOR], ranges, amin, inc, mgc.RAGGED_OFFSETS, **kw)
    sq = match.match_scans(st, p, [mgc.RAGGED_PRIOR], ranges, amin, inc, mgc.RAGGED_OFFSETS, kw["k0"], 1, 20, 1, 0,
                           kw["kern"])
    vol = sq["volume"][0][:, 20 - 13:20 + 13 + 1, :]
    mx = vol.max()
    ks, js, is_ = np.nonzero(vol == mx)
    i, j = is_.astype(np.int64) - 20, js.astype(np.int64) - 13
    n = np.lexsort((i, j, ks, np.abs(ks - kw["k0"]), i * i + j * j))[0]
    assert got["best"][0].tolist() == [int(ks[n]), int(i[n]), int(j[n])] and got["score"][0] == mx > 0
    assert got["n_used"][0] == 22 and ks.shape[0] > 1


def test_empty_map():
    p = cases.make_params(96, 128)
    ranges, amin, inc = mgc.ragged_scans()
    for fill in (-1, 0):
        st = np.full((128, 96), fill, np.int8)
        got = match.match_global(st, p, [mgc.RAGGED_PRIOR], ranges, amin, inc, mgc.RAGGED_OFFSETS, **mgc.RAGGED)
        assert got["best"][0].tolist() == [4, 0, 0] and got["score"][0] == 0 and got["n_used"][0] == 22
        assert got["pose"][0].tolist() == [0.3, -0.4, 0.2 + 0.0]


def test_global_params_reads_the_yaml():
    gp = match.global_params(None, 0.05, 400, 401)
    assert len(gp["yaw_offsets"]) == 180 and gp["k0"] == 90 and gp["yaw_offsets"][90] == 0.0
    assert abs(gp["yaw_offsets"][0] + 90 * 0.0349) < 1e-12
    assert (gp["half_x"], gp["half_y"]) == (200, 201)
    assert gp["smear_cells"] == 2 and gp["kern"].tolist() == match.kernel_table(0.03, 0.05, 2).tolist()
    near = match.global_params(None, 0.05, 4096, 4096, prior=(1.0, 2.0, 0.3))
    assert (near["half_x"], near["half_y"]) == (80, 80)

    class S:
        coarse_angle_resolution = 2.0 * math.pi / 90  # an exact divisor: 90, not 89
        loop_search_space_smear_deviation = 0.1
        loop_search_space_dimension = 3.0

    own = match.global_params(S, 0.05, 100, 100, prior=(0.0, 0.0, 0.0))
    assert len(own["yaw_offsets"]) == 90 and own["smear_cells"] == 4 and own["half_x"] == 30


def test_slam_params_carry_the_wide_search():
    from dm.ros_node import SlamParams

    d = SlamParams()
    assert (d.loop_search_space_dimension, d.loop_search_space_smear_deviation,
            d.loop_match_minimum_response_coarse, d.loop_match_minimum_response_fine) == (8.0, 0.03, 0.35, 0.45)
    assert (d.dm_map_file, d.dm_relocalize) == ("", False)
    s = SlamParams.from_dict({"loop_search_space_dimension": 4.0, "dm_relocalize": True, "dm_map_file": "a.dm"})
    assert (s.loop_search_space_dimension, s.dm_relocalize, s.dm_map_file) == (4.0, True, "a.dm")

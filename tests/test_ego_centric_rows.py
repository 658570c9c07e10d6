"""``smarts_amd.env.ego_centric_rows`` — the ego-centric adapters over host copies of the dense rows — against the
outputs of the reference's own adapter module (``tests/golden/ego_centric_cases.npz`` / ``ego_centric_actions.npz``,
written by ``tests/golden/gen_golden_ego_centric.py``).

Float64 outputs are asserted BIT-EQUAL (it holds: same libm, same operations in the same order; the issue's bound
was 1e-12 absolute); float32 outputs equal after rounding the reference's float64 to float32."""
import math
import os

import numpy as np
import pytest

from smarts_amd import _native as nat
from smarts_amd.env.ego_centric_rows import actions_to_world_rows, ego_centric_rows, wrap_value

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLDEN, "ego_centric_cases.npz"))
    groups = {}
    for name in z["groups"]:
        name = str(name)
        rows = {k[len(name) + 4:]: z[k] for k in z.files if k.startswith(name + "_in_")}
        ref = {k[len(name) + 5:]: z[k] for k in z.files if k.startswith(name + "_ref_")}
        groups[name] = (rows, ref, ego_centric_rows(rows))
    return groups


@pytest.fixture(scope="module")
def actions():
    return dict(np.load(os.path.join(GOLDEN, "ego_centric_actions.npz")))


def test_the_fixture_holds_what_it_should(cases):
    assert sum(rows["ego_pos"].shape[0] for name, (rows, _, _) in cases.items() if name != "hand") == 64
    rows = cases["4lane"][0]
    assert (rows["wp_count"][:, 0] > 1).any()  # junction poses: several paths
    assert (rows["lidar_hit"] == 0).any() and (rows["lidar_hit"] != 0).any()
    assert (rows["rw_count"] > 0).any()
    nb = np.arange(rows["nb_heading"].shape[1])[None, :] < rows["nb_count"][:, None]
    d = np.abs(rows["nb_heading"].astype(np.float64) - rows["ego_frame"][:, 3:4])
    assert (nb & (np.minimum(d, 2 * math.pi - d) > 3.0)).any()  # a neighbour on an oncoming lane


def test_positions_are_bit_equal_to_the_reference(cases):
    for name, (rows, ref, got) in cases.items():
        assert got["ec_flags"].all()
        assert np.array_equal(got["ego_frame"], rows["ego_frame"])
        assert not ref["ec_ego_pos"].any() and not ref["ec_ego_heading"].any()  # the origin
        for k in ("ec_wp_pos", "ec_nb_pos", "ec_rw_pos", "ec_lidar_point"):
            if k in ref:
                assert np.array_equal(got[k], ref[k], equal_nan=True), (name, k, np.nanmax(np.abs(got[k] - ref[k])))
    rows, ref, got = cases["4lane"]
    miss = rows["lidar_hit"] == 0
    assert np.isnan(got["ec_lidar_point"][miss]).all() and np.isfinite(got["ec_lidar_point"][~miss]).all()


def test_float32_rows_equal_the_reference_after_rounding(cases):
    E = nat.EGO
    for name, (rows, ref, got) in cases.items():
        for k in ("ec_wp_heading", "ec_nb_heading", "ec_rw_heading"):
            if k in ref:
                assert got[k].dtype == np.float32
                assert np.array_equal(got[k], ref[k].astype(np.float32)), (name, k)
        f = got["ec_ego_f32"]
        assert not f[:, E["HEADING"]].any()
        for j, key in enumerate(("LIN_VEL", "LIN_ACC", "LIN_JERK")):
            assert np.array_equal(f[:, E[key]:E[key] + 3], ref["ec_ego_lin"][:, j].astype(np.float32)), (name, key)
            assert not f[:, E[key] + 1].any()
        same = np.ones(nat.EGO_F32_COUNT, dtype=bool)
        same[[E["HEADING"], *[E[key] + i for key in ("LIN_VEL", "LIN_ACC", "LIN_JERK") for i in range(2)]]] = False
        assert np.array_equal(f[:, same], rows["ego_f32"][:, same])  # every other column copied


def test_every_branch_of_wrap_value_is_in_the_file(cases):
    d = []
    for rows, _, _ in cases.values():
        H = rows["ego_frame"][:, 3]
        nb = np.arange(rows["nb_heading"].shape[1])[None, :] < rows["nb_count"][:, None]
        d.append((rows["nb_heading"].astype(np.float64) - H[:, None])[nb])
        P, W = rows["wp_heading"].shape[1:]
        wp = (np.arange(P)[None, :, None] < rows["wp_count"][:, :1, None]) & (np.arange(W)[None, None, :] < rows["wp_count"][:, 1:, None])
        d.append((rows["wp_heading"].astype(np.float64) - H[:, None, None])[wp])
    d = np.concatenate(d)
    counts = {"<= -pi": int((d <= -math.pi).sum()), "> pi": int((d > math.pi).sum()), "== -pi": int((d == -math.pi).sum()),
              "> 2 pi": int((d > 2 * math.pi).sum()), "< -2 pi": int((d < -2 * math.pi).sum()), "== 0": int((d == 0.0).sum()),
              "inside": int(((d > -math.pi) & (d <= math.pi)).sum())}
    assert all(n >= 1 for n in counts.values()), counts
    assert counts["== -pi"] == 2 and counts["> 2 pi"] == 2 and counts["< -2 pi"] == 2, counts  # (the hand-made rows: wp + nb each)
    assert wrap_value(-math.pi, -math.pi, math.pi) == math.pi and wrap_value(0.0, -math.pi, math.pi) == 0.0
    for v in d:
        assert -math.pi < wrap_value(float(v), -math.pi, math.pi) <= math.pi


def _rows(actions):
    return {"ego_frame": actions["frame"], "ec_flags": actions["flags"]}


@pytest.mark.parametrize("space,key,has_counts", [("Trajectory", "traj", True), ("TargetPose", "pose", False),
                                                  ("TrajectoryWithTime", "twt", True)])
def test_actions_to_world_is_bit_equal_to_the_reference(space, key, has_counts, actions):
    a, counts = actions[key + "_in"], actions[key + "_counts"] if has_counts else None
    got = actions_to_world_rows(space, a, counts, _rows(actions))
    assert np.array_equal(got, actions[key + "_ref"], equal_nan=True)
    assert np.array_equal(got[3], a[3])  # flags 0: the reference's last_obs is None
    if has_counts:
        assert np.array_equal(got[4], a[4]) and counts[4] == 0  # no action
        assert (got[counts > 0] != a[counts > 0]).any()
    else:
        assert np.array_equal(got[5], a[5], equal_nan=True) and np.isnan(a[5, 0])


def test_the_reference_tests_known_answers(actions):
    rows = _rows(actions)
    got = actions_to_world_rows("Trajectory", actions["traj_in"], actions["traj_counts"], rows)[0]
    assert np.allclose(got[:, :2], actions["kat_traj"])
    got = actions_to_world_rows("TargetPose", actions["pose_in"], None, rows)[0]
    assert np.allclose(got, actions["kat_pose"]) and np.allclose(actions["kat_pose"], (165.23485529, 1.2, 1.81238898, 20.0))
    got = actions_to_world_rows("TrajectoryWithTime", actions["twt_in"], actions["twt_counts"], rows)[0]
    assert np.allclose(got[1:, :2], actions["kat_traj"]) and np.array_equal(got[0, :2], [0.1, 0.2])  # time is not rotated

"""The kinematic action spaces (TargetPose, TrajectoryWithTime) without a GPU: the restatement in tests/kinematic_ref.py
against the reference's own outputs (tests/golden/kinematic_*.npz, written by tests/golden/gen_golden_kinematic.py), what
the fixtures cover, the Python surface, and the launch plan.

Bounds: bit-exact where only + - * / sqrt and the float modulo are involved; 4e-15 relative where libm sin / cos /
atan2 enter (the bound of the controller fixtures) — relative to the size of the operands the libm value
is multiplied into, since several of these quantities are differences that cancel (a speed of 0 from a control
polygon metres long, an "angular velocity" that is a difference of unit vectors over dt)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import kinematic_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIBM = 4e-15


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _target(row):
    return None if np.isnan(row[0]) else tuple(float(v) for v in row)


@pytest.mark.parametrize("tag", ["dt100", "dt010"])
def test_target_pose_fixture_covers_the_cases(tag):
    g = _load(f"kinematic_target_pose_{tag}.npz")
    dt, tg, raw = float(g["dt"]), g["targets"], g["raw"]
    T, V = tg.shape[:2]
    assert V >= 64 and T >= 40 and sorted(set(g["map"].tolist())) == [0, 1, 2]
    given = ~np.isnan(tg[..., 0])
    sec = tg[..., 3][given]
    assert (sec < dt).any() and (sec == dt).any() and (sec > dt).any()
    assert (~given).any() and (~given).sum() > T  # ticks without an action
    same = given & (tg[..., 0] == raw[:-1, :, 0]) & (tg[..., 1] == raw[:-1, :, 1])
    assert same.any()  # target = current position: extension 0
    diff = (tg[..., 2] - raw[:-1, :, 2])[given]
    assert (diff > math.pi).any() and (diff < -math.pi).any() and (np.abs(diff) < math.pi).any()
    assert (raw[..., 2] >= math.pi).any() or (raw[..., 2] < -math.pi).any()  # the provider's heading leaves [-pi, pi)
    assert (np.abs(g["veh"][..., 2]) <= math.pi).all()


@pytest.mark.parametrize("tag", ["dt100", "dt010"])
def test_target_pose_restatement_matches_the_provider(tag):
    g = _load(f"kinematic_target_pose_{tag}.npz")
    dt, tg, raw, veh, speed = float(g["dt"]), g["targets"], g["raw"], g["veh"], g["speed"]
    worst = 0.0
    for t in range(tg.shape[0]):
        for v in range(tg.shape[1]):
            x, y, h = (float(c) for c in raw[t, v])
            target = _target(tg[t, v])
            nx, ny, nh, ns = kr.bezier_first_point(x, y, h, target, dt)
            assert nh == raw[t + 1, v, 2], (t, v)  # + - * and the float modulo only
            assert kr.heading_of(nh) == veh[t + 1, v, 2], (t, v)
            reach = 0.0 if target is None else math.hypot(target[0] - x, target[1] - y)
            for got, want, scale in ((nx, raw[t + 1, v, 0], abs(x) + reach), (ny, raw[t + 1, v, 1], abs(y) + reach),
                                     (ns, speed[t + 1, v], 6.0 * reach)):
                err = abs(got - want) / max(abs(want), scale, 1e-300)
                worst = max(worst, err)
                assert err <= LIBM, (t, v, got, want)
            assert veh[t + 1, v, 0] == raw[t + 1, v, 0] and veh[t + 1, v, 1] == raw[t + 1, v, 1]
    print(f"target pose {tag}: worst relative error {worst:.3g}")


@pytest.mark.parametrize("tag", ["dt100", "dt010"])
def test_box_chassis_restatement_matches_the_reference(tag):
    g = _load(f"kinematic_target_pose_{tag}.npz")
    dt, veh, speed = float(g["dt"]), g["veh"], g["speed"]
    T1, V = speed.shape
    assert np.isnan(g["box_yaw_rate"][0]).all() and not np.isnan(g["box_yaw_rate"][1:]).any()  # None until control(dt)
    assert np.isnan(g["box_steering"]).all() and (g["box_ang_vel"][0] == 0).all()
    for v in range(V):
        box = kr.BoxChassisRef(float(veh[0, v, 2]), float(speed[0, v]))
        for t in range(T1):
            if t:
                box.control(float(veh[t, v, 2]), float(speed[t, v]), dt)
            sp, lin, ang, yaw, steer = box.read_back()
            assert sp == g["box_speed"][t, v] and math.isnan(steer)
            assert (math.isnan(yaw) and np.isnan(g["box_yaw_rate"][t, v])) or yaw == g["box_yaw_rate"][t, v], (t, v)
            for q in range(3):
                assert abs(lin[q] - g["box_lin_vel"][t, v, q]) <= LIBM * max(abs(sp), 1e-300), (t, v, q)
                # a difference of two unit-vector components over dt
                assert abs(ang[q] - g["box_ang_vel"][t, v, q]) <= LIBM * 2.0 / dt, (t, v, q)


def test_trajectory_with_time_restatement_matches_the_provider():
    g = _load("kinematic_trajectory_with_time.npz")
    trajs, counts = g["trajs"], g["counts"]
    assert len(trajs) >= 256 and counts.min() == 2 and counts.max() == 32
    first = trajs[:, 0, 0]
    assert (first < g["dt"]).any() and (first == g["dt"]).any()  # (a first time above dt is among the illegal ones)
    for k in range(len(trajs)):
        got = kr.interpolate_trajectory(trajs[k], int(counts[k]), float(g["dt"][k]))
        assert got is not None, k
        assert got[0] == g["pose"][k, 0] and got[1] == g["pose"][k, 1] and got[3] == g["speed"][k], k
        assert abs(got[2] - g["pose"][k, 2]) <= LIBM * math.pi, k
    reasons = set(g["illegal_reason"].tolist())
    assert reasons == {"less than 2", "nan, positive inf or negative inf", "not strictly increasing", "can not be located"}
    for k in range(len(g["illegal"])):
        assert kr.interpolate_trajectory(g["illegal"][k], int(g["illegal_counts"][k]), float(g["illegal_dt"][k])) is None, \
            (k, g["illegal_reason"][k])
    # a heading pair across +-pi is among the blended columns
    crossing = 0
    for k in range(len(trajs)):
        j = int(np.argmax(trajs[k, 0, :counts[k]] > g["dt"][k]))
        crossing += abs(trajs[k, 3, j] - trajs[k, 3, j - 1]) > math.pi
    assert crossing >= 10


def test_python_surface_lets_the_kinematic_spaces_through():
    from smarts_amd import _native as nat
    from smarts_amd.env.agent_interface import DEVICE_ACTION_SPACES, ActionSpaceType, AgentInterface

    assert nat.ACTION_SPACES["TargetPose"] == 5 and nat.ACTION_SPACES["TrajectoryWithTime"] == 6
    assert {"smx_step_target_pose", "smx_step_trajectory_with_time"} <= set(nat.EXPORTS)
    for space in (ActionSpaceType.TargetPose, ActionSpaceType.TrajectoryWithTime):
        assert space in DEVICE_ACTION_SPACES
        AgentInterface(waypoints=True, action=space).validate_for_device()
    for space in (ActionSpaceType.MPC, ActionSpaceType.MultiTargetPose, ActionSpaceType.Imitation):
        with pytest.raises(NotImplementedError):
            AgentInterface(waypoints=True, action=space).validate_for_device()
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "SMX_ACTION_SPACE_TARGET_POSE = 5" in header and "SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME = 6" in header


def test_launch_plan_of_the_kinematic_spaces(tmp_path):
    """smx_plan.h, host-compiled (tests/native/host_plan.cpp): a kinematic space plans the kinematic control kernel in a
    step of either form and nothing in a reset, and every other decision of the plan is the one Continuous gets."""
    import ctypes as C
    import itertools

    from smarts_amd import _native as nat

    lib_path = str(tmp_path / "libhost_plan.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "host_plan.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    CONTROL, CONTROL_NONE, CONTROL_KINEMATIC = 8, 0, 6  # index in the output; enum class Control by value
    arg, out = (C.c_int * 16)(), (C.c_int * 16)()
    checked = 0
    for (total, strategy, junctions, routed, lidar, timing, is_step, blobs, side_ready, idm) in itertools.product(
            (64, 16384, 16416, 131072), range(5), (0, 1), (0, 1), (0, 1), (0, 2), (0, 1), (31, 0, 15), (0, 1), (0, 1)):
        sensors = nat.SENSOR_WAYPOINTS | nat.SENSOR_OGM | (nat.SENSOR_LIDAR if lidar else 0)
        plans = {}
        for space in (1, 5, 6):
            arg[:] = [total // 32, 32, strategy, junctions, routed, sensors, 4, 64, 64, timing, is_step, blobs, side_ready, 0, idm, space]
            n = lib.host_plan(arg, out)
            plans[space] = list(out[:n])
        for space in (5, 6):
            assert plans[space][CONTROL] == (CONTROL_KINEMATIC if is_step else CONTROL_NONE), list(arg)
            rest = [v for i, v in enumerate(plans[space]) if i != CONTROL]
            assert rest == [v for i, v in enumerate(plans[1]) if i != CONTROL], list(arg)
        checked += 1
    assert checked > 5000


def test_launch_plan_gives_the_kinematic_spaces_no_control_slow_list(tmp_path):
    """tests/native/host_plan_control_slow.cpp: in the one-lane cut the Lane controller gets its slow list and the
    kinematic kernel gets none, while the sensor side's slow lists stay; outside that cut nobody has one."""
    import ctypes as C

    lib_path = str(tmp_path / "libhost_plan_control_slow.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "host_plan_control_slow.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_control_slow.argtypes = [C.POINTER(C.c_int)]
    one_lane_seen = 0
    for total in (64, 32768, 131072):
        for strategy in range(5):
            for junctions in (0, 1):
                got = {space: lib.host_plan_control_slow((C.c_int * 5)(total // 32, 32, strategy, junctions, space)) for space in (0, 1, 5, 6)}
                one_lane = bool(got[0] & 1)
                assert all(bool(g & 1) == one_lane for g in got.values())
                assert got[0] == (15 if one_lane else 0), (total, strategy, junctions, got)
                for space in (5, 6):
                    assert got[space] == (9 if one_lane else 0), (total, strategy, junctions, space, got)
                one_lane_seen += one_lane
    assert one_lane_seen >= 4

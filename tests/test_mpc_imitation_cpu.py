"""The MPC and Imitation action spaces without a GPU: the plain-float restatement of the two device paths
(tests/mpc_imitation_ref.py) against the reference's own outputs (tests/golden/mpc_cases.npz, imitation_cases.npz,
written by tests/golden/gen_golden_mpc_imitation.py), the enum values of the public surface, and the launch plan."""
import math
import os
import subprocess

import numpy as np

import kinematic_ref as kr
import mpc_imitation_ref as mr
from conftest import GOLDEN, ROOT

TOL = 1e-9  # the project's per-tick float64 bound


def mpc_reference_step(g, i):
    """The restatement on case i of mpc_cases.npz: (throttle, brake, steering, MpcState after)."""
    from oracle import controller as octl

    fields = list(g["state_fields"])
    ins = dict(zip(fields, g["in_state"][i]))
    st = mr.MpcState(float(ins["velocity_error"]), float(ins["integral_windup_error"]), float(ins["throttle_state"]),
                     float(ins["steering_state"]))
    tr = octl.unpack_trajectory(g["traj"][i], int(g["n"][i]))
    out = mr.trajectory_tracking_mpc(tr, float(g["x"][i]), float(g["y"][i]), float(g["heading"][i]), float(g["speed"][i]),
                                     float(g["lng_speed"][i]), float(g["lat_speed"][i]), st, float(g["dt"][i]))
    return out + (st,)


def test_mpc_restatement_equals_the_reference():
    """perform_trajectory_tracking_MPC on 378 mock vehicles + 8 ticks without an action: throttle, brake, steering and
    the three state fields the law updates within 1e-9.  Measured: throttle, brake and the state fields equal to the
    last bit; steering differs by at most 9.6e-14 (the reference inverts 2H, the restatement eliminates)."""
    g = np.load(os.path.join(GOLDEN, "mpc_cases.npz"))
    fields = list(g["state_fields"])
    worst = {}
    acted = 0
    for i in range(len(g["n"])):
        if g["n"][i] == 0:
            assert np.array_equal(g["in_state"][i], g["out_state"][i])
            continue
        acted += 1
        thr, brk, steer, st = mpc_reference_step(g, i)
        want = dict(zip(fields, g["out_state"][i]))
        for name, got, ref in (("throttle", thr, g["throttle"][i]), ("brake", brk, g["brake"][i]), ("steering", steer, g["steering"][i]),
                               ("velocity_error", st.velocity_error, want["velocity_error"]),
                               ("integral_windup_error", st.integral_windup_error, want["integral_windup_error"]),
                               ("throttle_state", st.throttle_state, want["throttle_state"])):
            worst[name] = max(worst.get(name, 0.0), abs(float(got) - float(ref)))
            assert abs(float(got) - float(ref)) <= TOL, (i, name, got, ref)
        # the reference's law leaves these four alone
        for name in ("heading_error", "lateral_error", "integral_velocity_error", "steering_state"):
            assert g["in_state"][i][fields.index(name)] == want[name]
    print("worst differences:", worst)
    assert acted > 300
    # the classes the generator insisted on are in the file
    classes = dict(c.rsplit(": ", 1) for c in g["mpc_classes"])
    assert all(int(v) >= 8 for v in classes.values()), classes
    assert {"length 1..5", "length 10", "length 11", "length > 11", "straight (heading sum exactly 0)", "ahead curvature < 30",
            "ahead curvature 30..100", "longitudinal speed 0", "longitudinal speed below 0.1", "brake", "dt 0.01",
            "no action", "steering clipped at +1", "steering clipped at -1"} <= set(classes)


def imitation_reference_rollout(g):
    """The restatement over every vehicle and tick of imitation_cases.npz: pose [T+1, V, 3], speed, last_heading, last_dt,
    yaw_rate, lin_vel, ang_vel as the fixture lays them out."""
    T, V = g["actions"].shape[:2]
    out = {k: np.full((T + 1, V) + s, np.nan) for k, s in (("pose", (3,)), ("speed", ()), ("last_heading", ()), ("last_dt", ()),
                                                           ("yaw_rate", ()), ("lin_vel", (3,)), ("ang_vel", (3,)))}
    for v in range(V):
        x, y, h, sp = (float(c) for c in g["start"][v])
        box = kr.BoxChassisRef(h, sp)
        box.last_heading = math.nan  # (no _last_heading before the second control())
        dt = float(g["dt"][v])
        for t in range(T + 1):
            if t > 0:
                a0, a1 = (float(c) for c in g["actions"][t - 1, v])
                step = mr.imitation_step(x, y, box.heading, box.speed, a0, a1, dt)
                if step is not None:
                    x, y = step[0], step[1]
                    box.control(step[2], step[3], dt)
            speed, lin, ang, yaw_rate, _ = box.read_back()
            out["pose"][t, v], out["speed"][t, v] = (x, y, box.heading), speed
            out["last_heading"][t, v], out["last_dt"][t, v], out["yaw_rate"][t, v] = box.last_heading, box.last_dt, yaw_rate
            out["lin_vel"][t, v], out["ang_vel"][t, v] = lin, ang
    return out


def test_imitation_restatement_equals_the_reference():
    """ImitationController.perform_action on a BoxChassis, 192 vehicles x 3 ticks: pose, speed and the BoxChassis
    read-back within 1e-9, NaN placement (no _last_heading yet, yaw rate None) exact.  Measured worst differences: pose
    3.6e-15, speed 0, _last_heading 8.9e-16, yaw rate 8.9e-14 and angular velocity 8.4e-14 (a last-bit heading difference
    over dt = 0.01)."""
    g = np.load(os.path.join(GOLDEN, "imitation_cases.npz"))
    assert g["actions"].dtype == np.float32
    got = imitation_reference_rollout(g)
    worst = 0.0
    for k, a in got.items():
        assert np.array_equal(np.isnan(a), np.isnan(g[k])), k
        err = np.nanmax(np.abs(a - g[k]))
        worst = max(worst, float(err))
        assert err <= TOL, (k, err)
    print("worst difference:", worst)
    # control() was called exactly where an action was sent, and never otherwise
    assert np.array_equal(g["called"] != 0, ~np.isnan(g["actions"][..., 0]))
    assert np.array_equal(g["last_dt"][1:] > 0, np.cumsum(g["called"], axis=0) > 0)
    classes = dict(c.rsplit(": ", 1) for c in g["imitation_classes"])
    assert all(int(v) >= 8 for v in classes.values()), classes
    assert {"two-float form", "scalar form", "no action", "crosses +pi", "crosses -pi", "crosses 2 pi upwards",
            "crosses 2 pi downwards", "speed below 0", "two consecutive actions", "yaw rate None"} <= set(classes)
    # what the device reports instead of carrying on is "not stepped" here
    assert mr.imitation_step(1.0, 2.0, 0.3, 4.0, 1.0, math.inf, 0.1) is None
    assert mr.imitation_step(1.0, 2.0, 0.3, 4.0, math.inf, math.nan, 0.1) is None
    assert mr.imitation_step(1.0, 2.0, 0.3, 4.0, math.nan, 1.0, 0.1) is None


def test_public_surface_names_the_two_spaces():
    from smarts_amd import _native as nat
    from smarts_amd.env.agent_interface import DEVICE_ACTION_SPACES, ActionSpaceType

    assert nat.ACTION_SPACES["MPC"] == 7 and nat.ACTION_SPACES["Imitation"] == 8
    assert 9 not in nat.ACTION_SPACES.values()
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "SMX_ACTION_SPACE_MPC = 7" in header and "SMX_ACTION_SPACE_IMITATION = 8" in header
    # the env-level gate stays shut in this change (the C-ABI and BatchedSim are the surface)
    assert ActionSpaceType.MPC not in DEVICE_ACTION_SPACES and ActionSpaceType.Imitation not in DEVICE_ACTION_SPACES


def test_launch_plan_of_mpc_and_imitation(tmp_path):
    """smx_plan.h, host-compiled (tests/native/host_plan.cpp): Imitation plans the kinematic control kernel in a step of
    either form and nothing in a reset, with every other decision Continuous's; MPC plans launch for launch what
    Trajectory plans."""
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
        for space in (1, 4, nat.ACTION_SPACES["MPC"], nat.ACTION_SPACES["Imitation"]):
            arg[:] = [total // 32, 32, strategy, junctions, routed, sensors, 4, 64, 64, timing, is_step, blobs, side_ready, 0, idm, space]
            n = lib.host_plan(arg, out)
            plans[space] = list(out[:n])
        assert plans[7] == plans[4], list(arg)
        assert plans[8][CONTROL] == (CONTROL_KINEMATIC if is_step else CONTROL_NONE), list(arg)
        assert [v for i, v in enumerate(plans[8]) if i != CONTROL] == [v for i, v in enumerate(plans[1]) if i != CONTROL], list(arg)
        checked += 1
    assert checked > 5000

    # the control slow list (tests/native/host_plan_control_slow.cpp): MPC as Trajectory, Imitation none, as TargetPose
    lib_path = str(tmp_path / "libhost_plan_control_slow.so")
    cmd[-3], cmd[-1] = os.path.join(ROOT, "tests", "native", "host_plan_control_slow.cpp"), lib_path
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_control_slow.argtypes = [C.POINTER(C.c_int)]
    for total, strategy, junctions in itertools.product((64, 32768, 131072), range(5), (0, 1)):
        got = {space: lib.host_plan_control_slow((C.c_int * 5)(total // 32, 32, strategy, junctions, space)) for space in (4, 5, 7, 8)}
        assert got[7] == got[4] and got[8] == got[5], (total, strategy, junctions, got)

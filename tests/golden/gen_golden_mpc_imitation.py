#!/usr/bin/env python3
"""Golden vectors of the MPC and Imitation action spaces, from the reference's OWN classes.

Same import shim as ``gen_golden.py`` (which see): runs only where the reference tree is; the suite consumes the
committed ``tests/golden/mpc_cases.npz`` and ``tests/golden/imitation_cases.npz`` (arrays only).

* ``TrajectoryTrackingController.perform_trajectory_tracking_MPC`` on mock vehicles, as ``gen_golden.py::
  dump_trajectory_pd`` drives the PD law: an ``AckermannChassis`` made with ``__new__`` that carries the sedan's chassis
  mass and yaw inertia, the tyre model's cornering stiffnesses (models/tire_parameters.yaml) and the given body speeds.
  One tick per case; the classes of cases the generator insists on are counted in ``mpc_classes`` / asserted below.
* ``ImitationController.perform_action`` on a ``BoxChassis`` (bullet body / constraint stubbed) whose ``control``
  records its arguments: three consecutive ticks per vehicle, with both action forms, ticks without an action, headings
  whose update crosses +-pi and 2 pi, and decelerations through speed 0.  The action floats are float32 values, as they
  travel in the action buffer.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mpc_imitation.py
"""
import math
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402

TMAX = 11
STATE_FIELDS = ("heading_error", "lateral_error", "velocity_error", "integral_velocity_error", "integral_windup_error",
                "steering_state", "throttle_state")
SEDAN_LENGTH = 3.68  # VEHICLE_CONFIGS["passenger"].dimensions.length (vehicle.py:101)
IMITATION_TICKS = 3


def _trajectory(rng, x, y, h, n, shape, v_last, aside):
    """`n` points ahead of (x, y, h), `aside` metres to its right: "straight" (every heading the same float), an arc of
    radius `shape` otherwise."""
    xs, ys, hs = [], [], []
    px, py = x + rng.normal(0, 0.3) + aside * math.cos(h), y + rng.normal(0, 0.3) + aside * math.sin(h)
    ph = h + (0.0 if shape == "straight" else rng.normal(0, 0.05))
    step = float(rng.uniform(0.7, 1.3))
    for _ in range(n):
        xs.append(float(px)), ys.append(float(py)), hs.append(float(ph))
        px, py = px - math.sin(ph) * step, py + math.cos(ph) * step
        if shape != "straight":
            ph = ph + step / shape
    speeds = [max(0.0, float(v_last + rng.normal(0, 0.5))) for _ in range(n - 1)] + [float(v_last)]
    return [xs, ys, hs, speeds]


def dump_mpc(seed=7301):
    import yaml

    from smarts.core.chassis import AckermannChassis
    from smarts.core.controllers.trajectory_tracking_controller import (
        TrajectoryTrackingController as TTC,
        TrajectoryTrackingControllerState,
    )
    from smarts.core.coordinates import Heading, Pose
    from smarts.core.utils.math import fast_quaternion_from_angle

    with open(os.path.join(gg.REF, "smarts", "core", "models", "tire_parameters.yaml")) as f:
        tire = yaml.safe_load(f)
    assert (tire["C_alpha_front"], tire["C_alpha_rear"]) == (25000, 25000)
    rng = np.random.default_rng(seed)
    # length classes: 1..5 (every curvature the sentinel), 6..9 (some offsets only), 10, 11, beyond
    lengths = [1, 3, 5, 6, 9, 10, 11, 12, 25]
    # arc radii: |curvature(trajectory, 4)| equals the radius: the bands < 30, 30..100, >= 100, both turning senses
    shapes = ["straight", 12.0, -20.0, 45.0, -80.0, 150.0, -400.0]
    cols = {k: [] for k in ["x", "y", "heading", "speed", "lng_speed", "lat_speed", "n", "traj", "dt", "in_state", "out_state",
                            "throttle", "brake", "steering", "ahead_curvature", "curvature0"]}
    k = 0
    for n in lengths:
        for shape in shapes:
            for lng_kind in ("zero", "crawl", "drive"):
                for dt in (0.1, 0.01):
                    k += 1
                    x, y, h = float(rng.uniform(-50, 50)), float(rng.uniform(-50, 50)), float(rng.uniform(-math.pi, math.pi))
                    lng = {"zero": 0.0, "crawl": float(rng.uniform(0.005, 0.095)), "drive": float(rng.uniform(0.2, 25.0))}[lng_kind]
                    lat = float(rng.normal(0, 0.05)) if k % 3 else 0.0
                    speed = math.sqrt(lng * lng + lat * lat)
                    # the wanted speed below and above the vehicle's, so that the filtered throttle takes both signs
                    v_last = float(rng.uniform(0.0, 4.0)) if k % 2 else float(rng.uniform(speed + 2.0, speed + 12.0))
                    # every seventh case far off its trajectory, to either side: the steering reaches the clip
                    aside = 0.0 if k % 7 else float(rng.uniform(15.0, 40.0)) * (1 if k % 14 else -1)
                    trajectory = _trajectory(rng, x, y, h, n, shape, v_last, aside)
                    hd = Heading(h)
                    pose = Pose(position=np.array([x, y, 0.01265]), orientation=fast_quaternion_from_angle(hd), heading_=hd)
                    chassis = AckermannChassis.__new__(AckermannChassis)
                    chassis.__dict__["longitudinal_lateral_speed"] = (lng, lat)
                    chassis.__dict__["mass_and_inertia"] = (2356.0, 2681.95008628)
                    chassis._tire_parameters = tire
                    assert chassis.front_rear_stiffness == (25000, 25000)
                    captured = {}

                    def control(throttle=0, brake=0, steering=0, captured=captured):
                        captured.update(throttle=float(throttle), brake=float(brake), steering=float(steering))

                    vehicle = types.SimpleNamespace(chassis=chassis, pose=pose, position=pose.position, heading=hd, speed=speed,
                                                    length=SEDAN_LENGTH, control=control)
                    st = TrajectoryTrackingControllerState()
                    if k % 5:
                        st.heading_error = float(rng.normal(0, 0.1))
                        st.lateral_error = float(rng.normal(0, 0.3))
                        st.velocity_error = float(rng.normal(0, 1.0))
                        st.integral_velocity_error = float(rng.normal(0, 2.0))
                        st.integral_windup_error = float(rng.normal(0, 0.2))
                        st.steering_state = float(np.clip(rng.normal(0, 0.3), -1, 1))
                        st.throttle_state = float(rng.uniform(-1, 1))
                    in_state = [float(getattr(st, f)) for f in STATE_FIELDS]
                    TTC.perform_trajectory_tracking_MPC(trajectory, vehicle, st, dt)
                    packed = np.zeros((4, TMAX))
                    for r in range(4):
                        head = trajectory[r][:10]
                        packed[r, :len(head)] = head
                        packed[r, 10] = trajectory[r][-1]
                    row = dict(x=x, y=y, heading=h, speed=speed, lng_speed=lng, lat_speed=lat, n=n, traj=packed, dt=dt,
                               in_state=in_state, out_state=[float(getattr(st, f)) for f in STATE_FIELDS],
                               throttle=captured["throttle"], brake=captured["brake"], steering=captured["steering"],
                               ahead_curvature=abs(TTC.curvature_calculation(trajectory, 4)),
                               curvature0=TTC.curvature_calculation(trajectory, 0))
                    for key, val in row.items():
                        cols[key].append(val)
    # count 0: no action this tick (nothing is called; the state stays)
    for dt in (0.1, 0.01):
        for _ in range(4):
            st_in = [float(v) for v in rng.normal(0, 0.3, len(STATE_FIELDS))]
            row = dict(x=float(rng.uniform(-50, 50)), y=float(rng.uniform(-50, 50)), heading=float(rng.uniform(-3, 3)),
                       speed=5.0, lng_speed=5.0, lat_speed=0.0, n=0, traj=np.zeros((4, TMAX)), dt=dt, in_state=st_in,
                       out_state=st_in, throttle=0.0, brake=0.0, steering=math.nan, ahead_curvature=1e20, curvature0=1e20)
            for key, val in row.items():
                cols[key].append(val)
    out = {key: np.array(val) for key, val in cols.items()}
    out["n"] = out["n"].astype(np.int32)
    out["state_fields"] = np.array(STATE_FIELDS)

    # ---- the classes of cases the fixture must hold
    n, ahead, act = out["n"], out["ahead_curvature"], out["n"] > 0
    need = {
        "length 1..5": ((n >= 1) & (n <= 5)).sum(), "length 6..9": ((n >= 6) & (n <= 9)).sum(), "length 10": (n == 10).sum(),
        "length 11": (n == 11).sum(), "length > 11": (n > 11).sum(),
        "straight (heading sum exactly 0)": (act & (n > 5) & (out["curvature0"] == 1e20)).sum(),
        "ahead curvature < 30": (act & (ahead < 30)).sum(), "ahead curvature 30..100": (act & (ahead >= 30) & (ahead < 100)).sum(),
        "ahead curvature >= 100": (act & (ahead >= 100)).sum(),
        "longitudinal speed 0": (act & (out["lng_speed"] == 0)).sum(),
        "longitudinal speed below 0.1": (act & (out["lng_speed"] > 0) & (out["lng_speed"] < 0.1)).sum(),
        "longitudinal speed above 0.1": (act & (out["lng_speed"] > 0.1)).sum(),
        "throttle": (act & (out["throttle"] > 0)).sum(), "brake": (act & (out["brake"] > 0)).sum(),
        "dt 0.1": (act & (out["dt"] == 0.1)).sum(), "dt 0.01": (act & (out["dt"] == 0.01)).sum(),
        "no action": (~act).sum(), "steering inside the clip": (act & (np.abs(out["steering"]) < 1)).sum(),
        "steering clipped at +1": (act & (out["steering"] == 1)).sum(), "steering clipped at -1": (act & (out["steering"] == -1)).sum(),
    }
    minimum = {key: 8 for key in need}
    minimum.update({"length 10": 20, "length 11": 20, "steering inside the clip": 100})
    for key, cnt in need.items():
        assert cnt >= minimum[key], (key, int(cnt))
    out["mpc_classes"] = np.array([f"{key}: {int(cnt)}" for key, cnt in need.items()])
    return out


def dump_imitation(seed=7302, vehicles=192):
    import smarts.core.chassis as chassis_mod
    from smarts.core.controllers.imitation_controller import ImitationController
    from smarts.core.coordinates import Heading, Pose
    from smarts.core.vehicle import VEHICLE_CONFIGS

    class RecordingBox(chassis_mod.BoxChassis):
        """BoxChassis whose control() keeps what it was called with."""

        calls = None

        def control(self, pose, speed, dt=0):
            if self.calls is not None:
                self.calls.append((float(pose.position[0]), float(pose.position[1]), float(pose.heading), float(speed), float(dt)))
            super().control(pose, speed, dt)

    rng = np.random.default_rng(seed)
    dims = VEHICLE_CONFIGS["passenger"].dimensions
    T, V = IMITATION_TICKS, vehicles
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    start = np.zeros((V, 4))
    dts = np.where(np.arange(V) % 2 == 0, 0.1, 0.01)
    actions = np.full((T, V, 2), np.nan, dtype=np.float32)
    pose = np.zeros((T + 1, V, 3))
    speed = np.zeros((T + 1, V))
    last_heading = np.full((T + 1, V), np.nan)
    last_dt = np.zeros((T + 1, V))
    yaw_rate = np.full((T + 1, V), np.nan)
    lin_vel = np.zeros((T + 1, V, 3))
    ang_vel = np.zeros((T + 1, V, 3))
    called = np.zeros((T, V), dtype=np.uint8)
    kind = (np.arange(V) // 2) % 8
    for v in range(V):
        dt = float(dts[v])
        h = float(rng.uniform(-math.pi, math.pi))
        sp = float(rng.uniform(0.0, 15.0))
        acts = [(f32(rng.normal(0, 2.0)), f32(rng.normal(0, 0.5))) for _ in range(T)]
        if kind[v] == 1:  # the update crosses +pi: every tick turns left from just below it
            h = math.pi - 0.3 * dt
            acts = [(a, f32(rng.uniform(0.5, 2.0))) for a, _ in acts]
        elif kind[v] == 2:  # ... -pi, turning right
            h = -math.pi + 0.3 * dt
            acts = [(a, f32(-rng.uniform(0.5, 2.0))) for a, _ in acts]
        elif kind[v] == 3:  # (heading + w dt) % 2 pi goes from just below 2 pi to just above 0, and back
            h = -0.4 * dt
            acts = [(acts[0][0], f32(1.0)), (acts[1][0], f32(-2.5)), (acts[2][0], f32(3.0))]
        elif kind[v] == 4:  # braking through speed 0
            sp = float(rng.uniform(0.0, 2.0)) * dt * 10
            acts = [(f32(-rng.uniform(3.0, 8.0)), w) for _, w in acts]
        elif kind[v] == 5:  # the scalar form first ("setting the initial speed"), also last
            acts = [(f32(rng.uniform(0.0, 20.0)), math.nan), acts[1], (f32(rng.uniform(-2.0, 20.0)), math.nan)]
        elif kind[v] == 6:  # a tick without an action between two with one
            acts[1] = None
        elif kind[v] == 7:  # no action at first: no control() with a dt yet, so no yaw rate
            acts[0] = None
            if v % 4 < 2:
                acts[1] = None
        start[v] = (float(rng.uniform(-50, 50)), float(rng.uniform(-50, 50)), h, sp)
        p0 = Pose.from_center([start[v, 0], start[v, 1], 0], Heading(h))
        box = RecordingBox(p0, sp, dims, gg._Anything())
        vehicle = types.SimpleNamespace(chassis=box)

        def control(pose, speed, dt=0, box=box):
            box.control(pose=pose, speed=speed, dt=dt)  # Vehicle.control (vehicle.py:578)

        vehicle.control = control

        def read(t):
            vehicle.pose, vehicle.position, vehicle.heading, vehicle.speed = box.pose, box.pose.position, box.pose.heading, box.speed
            pose[t, v] = (*box.pose.position[:2], float(box.pose.heading))
            speed[t, v] = box.speed
            last_heading[t, v] = getattr(box, "_last_heading", math.nan)
            last_dt[t, v] = box._last_dt
            yaw_rate[t, v] = math.nan if box.yaw_rate is None else box.yaw_rate
            lin_vel[t, v], ang_vel[t, v] = box.velocity_vectors

        read(0)
        start[v, 2] = pose[0, v, 2]
        for t in range(T):
            box.calls = []
            a = acts[t]
            if a is not None:
                actions[t, v] = a
                if a[1] != a[1]:
                    ImitationController.perform_action(dt, vehicle, float(a[0]))
                else:
                    ImitationController.perform_action(dt, vehicle, (float(a[0]), float(a[1])))
                assert len(box.calls) == 1 and box.calls[0][4] == dt
            assert len(box.calls) == (a is not None)
            called[t, v] = len(box.calls)
            read(t + 1)
    out = dict(dt=dts, start=start, actions=actions, pose=pose, speed=speed, last_heading=last_heading, last_dt=last_dt,
               yaw_rate=yaw_rate, lin_vel=lin_vel, ang_vel=ang_vel, called=called, kind=kind.astype(np.int32))
    # ---- the classes of cases the fixture must hold
    a0, a1 = actions[..., 0].astype(np.float64), actions[..., 1].astype(np.float64)
    two = ~np.isnan(a0) & ~np.isnan(a1)
    raw = pose[:-1, :, 2] + a1 * dts[None, :]  # heading + w dt before the modulo
    need = {
        "two-float form": two.sum(), "scalar form": (~np.isnan(a0) & np.isnan(a1)).sum(), "no action": np.isnan(a0).sum(),
        "crosses +pi": (two & (raw > math.pi)).sum(), "crosses -pi": (two & (raw < -math.pi)).sum(),
        "crosses 2 pi upwards": (two & (pose[:-1, :, 2] < 0) & (raw >= 0)).sum(),
        "crosses 2 pi downwards": (two & (pose[:-1, :, 2] >= 0) & (raw < 0)).sum(),
        "speed below 0": (speed[1:] < 0).sum(), "action after a tick without one": (np.isnan(a0[:-1]) & ~np.isnan(a0[1:])).sum(),
        "two consecutive actions": (~np.isnan(a0[:-1]) & ~np.isnan(a0[1:])).sum(),
        "yaw rate None": np.isnan(yaw_rate[1:]).sum(),
    }
    for key, cnt in need.items():
        assert cnt >= 8, (key, int(cnt))
    out["imitation_classes"] = np.array([f"{key}: {int(cnt)}" for key, cnt in need.items()])
    return out


def main():
    gg.install_reference()
    import smarts.core.chassis as chassis_mod

    # BoxChassis' bullet body and constraint, stubbed as gen_golden.py stubs pybullet: names only, nothing computed
    chassis_mod.BulletBoxShape = gg._Anything
    chassis_mod.BulletPositionConstraint = gg._Anything
    mpc = dump_mpc()
    np.savez_compressed(os.path.join(gg.OUT, "mpc_cases.npz"), **mpc)
    imi = dump_imitation()
    np.savez_compressed(os.path.join(gg.OUT, "imitation_cases.npz"), **imi)
    print("\n".join(mpc["mpc_classes"]))
    print("\n".join(imi["imitation_classes"]))
    print(f"mpc cases: {len(mpc['n'])}; imitation vehicles: {imi['start'].shape[0]} x {IMITATION_TICKS} ticks")


if __name__ == "__main__":
    main()

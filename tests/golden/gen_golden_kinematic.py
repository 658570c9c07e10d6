#!/usr/bin/env python3
"""Golden vectors of the kinematic action spaces (TargetPose, TrajectoryWithTime), from the reference's OWN classes.

Same import shim as ``gen_golden.py`` (which see): runs only where the reference tree is; the suite consumes the
committed ``tests/golden/kinematic_*.npz`` (data only).

* ``MotionPlannerProvider.step`` — 72 vehicles (24 on each of the three maps) x 40 ticks, at dt 0.1 and 0.01: the
  provider's own pose rows (``_poses``) and the ``VehicleState`` pose / speed it hands out, tick by tick.
* ``BoxChassis`` (bullet body / constraint stubbed) fed those ``VehicleState`` sequences: speed, velocity vectors,
  yaw rate, steering per tick, the tick before the first ``control(..., dt)`` included.
* ``TrajectoryInterpolationProvider.perform_trajectory_interpolation`` — 320 legal trajectories and a list of
  illegal ones with the reason the reference gives.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_kinematic.py
"""
import math
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402

VEH_PER_MAP, TICKS, MAX_POINTS = 24, 40, 32


def start_poses(nets, rng):
    poses, maps = [], []
    for k, (name, net) in enumerate(nets.items()):
        for x, y, h in gg.sample_poses(net, rng, VEH_PER_MAP, lateral=0.5, heading_noise=0.2, far_fraction=0.0):
            poses.append((x, y, h, float(rng.uniform(0.0, 15.0))))
            maps.append(k)
    return np.array(poses), np.array(maps, dtype=np.int32)


def target_for(rng, v, t, raw, dt):
    """One TargetPose action for vehicle v at tick t (None = no action), by the vehicle's kind (v % 6) and the tick."""
    x, y, h = raw
    kind = v % 6
    if rng.random() < (0.5 if kind == 5 else 0.12):
        return None
    seconds = [0.5 * dt, dt, 3.0 * dt, 1.0, 0.0][int(rng.integers(5))]
    if kind == 1 and t % 5 == 0:
        return np.array([x, y, h + rng.uniform(-1.0, 1.0), seconds])  # target = current position: extension 0
    ahead = rng.uniform(0.0, 3.0) * (10.0 * dt)
    side = rng.normal(0.0, 0.2) * (10.0 * dt)
    tx = x - math.sin(h) * ahead + math.cos(h) * side
    ty = y + math.cos(h) * ahead + math.sin(h) * side
    if kind == 2:
        th = h + 2.5  # keeps turning one way, a whole tick's worth: the provider's heading leaves [-pi, pi)
        seconds = dt
    elif kind == 3:
        th = h - 2.9 if t % 2 else h + 3.1  # corrections on both sides of +-pi
    elif kind == 4:
        th = rng.uniform(-4.0 * math.pi, 4.0 * math.pi)  # target headings far outside one turn
    else:
        th = h + rng.normal(0.0, 0.3)
    return np.array([tx, ty, th, seconds])


def dump_target_pose(nets, dt, seed):
    from smarts.core.chassis import BoxChassis
    from smarts.core.coordinates import Heading, Pose
    from smarts.core.motion_planner_provider import MotionPlannerProvider
    from smarts.core.vehicle import VEHICLE_CONFIGS, VehicleState

    rng = np.random.default_rng(seed)
    start, maps = start_poses(nets, rng)
    V = len(start)
    dims = VEHICLE_CONFIGS["passenger"].dimensions
    provider = MotionPlannerProvider()
    provider.setup(None)
    ids = [f"v{v:03d}" for v in range(V)]
    chassis = []
    for v, vid in enumerate(ids):
        pose = Pose.from_center([start[v, 0], start[v, 1], 0], Heading(start[v, 2]))
        provider.create_vehicle(VehicleState(vehicle_id=vid, vehicle_config_type="passenger", pose=pose, dimensions=dims,
                                             speed=start[v, 3]))
        chassis.append(BoxChassis(pose, start[v, 3], dims, gg._Anything()))

    raw = np.zeros((TICKS + 1, V, 3))
    veh = np.zeros((TICKS + 1, V, 3))
    speed = np.zeros((TICKS + 1, V))
    targets = np.full((TICKS, V, 4), np.nan)
    box = {k: np.zeros((TICKS + 1, V) + s) for k, s in
           (("speed", ()), ("lin_vel", (3,)), ("ang_vel", (3,)), ("yaw_rate", ()), ("steering", ()))}

    def read_back(t):
        for v, ch in enumerate(chassis):
            lin, ang = ch.velocity_vectors
            box["speed"][t, v] = ch.speed
            box["lin_vel"][t, v] = lin
            box["ang_vel"][t, v] = ang
            box["yaw_rate"][t, v] = np.nan if ch.yaw_rate is None else ch.yaw_rate
            box["steering"][t, v] = np.nan if ch.steering is None else ch.steering

    raw[0] = provider._poses
    veh[0] = [(*c.pose.position[:2], float(c.pose.heading)) for c in chassis]
    speed[0] = start[:, 3]
    read_back(0)
    for t in range(TICKS):
        acts = {}
        for v, vid in enumerate(ids):
            a = target_for(rng, v, t, provider._poses[v], dt)
            acts[vid] = a
            if a is not None:
                targets[t, v] = a
        state = provider.step(acts, dt, (t + 1) * dt)
        assert [s.vehicle_id for s in state.vehicles] == ids
        raw[t + 1] = provider._poses
        for v, s in enumerate(state.vehicles):
            veh[t + 1, v] = (*s.pose.position[:2], float(s.pose.heading))
            speed[t + 1, v] = s.speed
            chassis[v].control(pose=s.pose, speed=s.speed, dt=dt)  # Vehicle.control (vehicle.py:578)
        read_back(t + 1)
    out = dict(dt=np.float64(dt), map=maps, map_names=np.array(list(nets)), start=start, targets=targets, raw=raw, veh=veh,
               speed=speed)
    out.update({"box_" + k: a for k, a in box.items()})
    return out


def dump_trajectory_with_time(net, seed, n_legal=320):
    """(Trajectories start near the lanes of `net`, so that a batch placed on them stays on its map.)"""
    from smarts.core.trajectory_interpolation_provider import TrajectoryInterpolationProvider as TIP

    rng = np.random.default_rng(seed)
    bases = gg.sample_poses(net, rng, 64, lateral=0.5, heading_noise=0.2, far_fraction=0.0)

    def make(n, dt, first):
        bx, by, _ = bases[int(rng.integers(len(bases)))]
        times = first + np.concatenate([[0.0], np.cumsum(rng.uniform(0.2 * dt, 1.5 * dt, n - 1))])
        if times[-1] <= dt:
            times[-1] = dt * (1.0 + rng.uniform(0.01, 2.0))
        h0 = rng.uniform(-math.pi, math.pi)
        heads = h0 + np.cumsum(rng.normal(0.0, 0.4, n))
        tr = np.stack([times, bx + np.cumsum(rng.normal(0.0, 0.5, n)), by + np.cumsum(rng.normal(0.0, 0.5, n)), heads,
                       rng.uniform(0.0, 20.0, n)])
        return tr

    trajs = np.zeros((n_legal, 5, MAX_POINTS))
    counts = np.zeros(n_legal, dtype=np.int32)
    dts = np.zeros(n_legal)
    pose = np.zeros((n_legal, 3))
    speed = np.zeros(n_legal)
    for k in range(n_legal):
        n = [2, 3, MAX_POINTS][k] if k < 3 else int(rng.integers(2, MAX_POINTS + 1))
        dt = (0.1, 0.01)[k % 2]
        first = [0.0, 0.5 * dt, dt, -dt][k % 4]  # the first time below or equal to dt
        tr = make(n, dt, first)
        if k % 5 == 0:  # a heading pair across +-pi around the blended columns
            j = int(np.argmax(tr[0] > dt))
            tr[3, j - 1], tr[3, j] = math.pi - rng.uniform(0.0, 0.3), -math.pi + rng.uniform(0.0, 0.3)
        if k % 7 == 0:
            tr[3] += 5.0 * math.pi  # headings outside one turn
        p, s = TIP.perform_trajectory_interpolation(dt, tr)
        trajs[k, :, :n], counts[k], dts[k] = tr, n, dt
        pose[k] = (*p.position[:2], float(p.heading))
        speed[k] = s

    illegal, reasons, ill_counts, ill_dt = [], [], [], []

    def refuse(tr, dt, why):
        try:
            TIP.perform_trajectory_interpolation(dt, tr)
        except AssertionError as e:
            assert why in str(e), (why, str(e))
        else:
            raise RuntimeError("the reference accepts a trajectory meant to be illegal: " + why)
        n = tr.shape[1]
        pad = np.zeros((5, MAX_POINTS))
        pad[:, :n] = tr
        illegal.append(pad)
        ill_counts.append(n)
        ill_dt.append(dt)
        reasons.append(why)

    for dt in (0.1, 0.01):
        refuse(make(2, dt, 0.0)[:, :1], dt, "less than 2")
        for bad in (np.nan, np.inf, -np.inf):
            for row in range(5):
                tr = make(6, dt, 0.0)
                tr[row, 3 if row else 5] = bad
                refuse(tr, dt, "nan, positive inf or negative inf")
        tr = make(6, dt, 0.0)
        tr[0, 3] = tr[0, 2]
        refuse(tr, dt, "not strictly increasing")
        tr = make(6, dt, 0.0)
        tr[0, 4] = tr[0, 2] - 0.001 * dt
        refuse(tr, dt, "not strictly increasing")
        refuse(make(6, dt, 1.5 * dt), dt, "can not be located")  # the first time above dt
        tr = make(6, dt, 0.0)
        tr[0] = np.linspace(0.0, dt, 6)  # no column later than dt
        refuse(tr, dt, "can not be located")
    return dict(trajs=trajs, counts=counts, dt=dts, pose=pose, speed=speed, illegal=np.array(illegal),
                illegal_counts=np.array(ill_counts, dtype=np.int32), illegal_dt=np.array(ill_dt),
                illegal_reason=np.array(reasons))


def main():
    gg.install_reference()
    import smarts.core.chassis as chassis_mod
    from smarts_amd.sumo_map import load_net

    # BoxChassis' bullet body and constraint, stubbed as gen_golden.py stubs pybullet: names only, nothing computed
    chassis_mod.BulletBoxShape = gg._Anything
    chassis_mod.BulletPositionConstraint = gg._Anything
    nets = {n: load_net(os.path.join(gg.REF, rel)) for n, rel in gg.SCENARIOS.items()}
    for tag, dt, seed in (("dt100", 0.1, 5101), ("dt010", 0.01, 5102)):
        np.savez_compressed(os.path.join(gg.OUT, f"kinematic_target_pose_{tag}.npz"), **dump_target_pose(nets, dt, seed))
    np.savez_compressed(os.path.join(gg.OUT, "kinematic_trajectory_with_time.npz"), **dump_trajectory_with_time(nets["loop"], 5103))
    print("kinematic goldens written")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors of the ego-centric adapters, from the reference's OWN module
(``smarts/core/utils/adapters/ego_centric_adapters.py``), imported under the shim of ``gen_golden.py`` (which see):
runs only where the reference tree is; the suite consumes the committed ``tests/golden/ego_centric_cases.npz`` and
``tests/golden/ego_centric_actions.npz`` (arrays only).

Observations: dense rows (include/smx.h) of oracle rollouts — loop (waypoints, neighbours), 4lane (waypoints with
junction paths, neighbours on oncoming lanes, road waypoints, a small lidar with hits and misses), minicity — and rows
made by hand whose heading differences reach every branch of ``wrap_value`` (exactly -pi, just above pi, beyond
+-2 pi, 0).  The reference's ``Observation`` is filled field by field from the rows (headings as plain floats: the
adapter only subtracts them), ``ego_centric_observation_adapter`` runs on it, and the fixture keeps per group ``g``
the rows (``g_in_*``, with ``g_in_ego_frame`` = px, py, pz, H the frame given to the reference) and the adapter's
output in the layout of ``smarts_amd.env.ego_centric_rows`` (``g_ref_*``; headings and the linear triples float64 as
the reference returns them).

Actions: Trajectory, TargetPose and TrajectoryWithTime buffers in the layouts of ``BatchedSim.step_*`` through the
reference's ``_trajectory_adaption`` / ``_egocentric_target_pose_adapter`` (TrajectoryWithTime: on rows 1-3,
reassembled), with random frames, and the vectors of the reference's own test
(``smarts/core/utils/adapters/tests/test_egocentric_adapters.py:328-386``, that file's fixture pose).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ego_centric.py
"""
import math
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402

SMALL_LIDAR = dict(start_angle=0.0, end_angle=2 * math.pi, laser_angles=(0.0, 0.05), angle_resolution=2 * math.pi / 12,
                   max_distance=20.0)
GROUPS = {  # name: (map, scenario dir, E, N, seed, ticks, quota, SimConfig keywords)
    "loop": ("loop", 1, 16, 3, 3, 16, dict()),
    "4lane": ("intersections/4lane", 2, 16, 11, 2, 32, dict(road_waypoints=True, rw_horizon=4, rw_lanes=4, rw_paths=2, lidar="small")),
    "minicity": ("minicity", 1, 16, 5, 2, 16, dict()),
}


def project_heading(v):
    from smarts_amd.env.observations import Heading

    return float(Heading(float(v)))


def hand_rows():
    """Seven agents, one waypoint and one neighbour each, heading difference d = h - H."""
    from smarts_amd import _native as nat

    cases = [(0.0, math.pi), (float(np.float32(math.pi - 1.0 + 1e-6)), -1.0), (7.0, -0.5), (-7.0, 0.5), (0.25, 0.25),
             (-3.0, 1.0), (1.0, 0.5)]
    T, P, W, K = len(cases), 4, 20, 10
    r = dict(ego_pos=np.zeros((T, 3)), ego_f32=np.zeros((T, nat.EGO_F32_COUNT), np.float32), ego_frame=np.zeros((T, 4)),
             wp_pos=np.zeros((T, P, W, 3)), wp_heading=np.zeros((T, P, W), np.float32), wp_count=np.zeros((T, P + 1), np.uint8),
             nb_pos=np.zeros((T, K, 3)), nb_heading=np.zeros((T, K), np.float32), nb_count=np.zeros(T, np.uint8))
    for g, (h, H) in enumerate(cases):
        r["ego_pos"][g] = (10.0 + g, -3.0 * g, 0.5)
        r["ego_frame"][g] = (*r["ego_pos"][g], H)
        r["ego_f32"][g, nat.EGO["HEADING"]] = H
        r["ego_f32"][g, nat.EGO["LIN_VEL"]:nat.EGO["LIN_VEL"] + 3] = (3.0, -4.0, 0.5)
        r["ego_f32"][g, nat.EGO["LIN_ACC"]:nat.EGO["LIN_ACC"] + 3] = (0.1 * g, 0.2, 0.0)
        r["ego_f32"][g, nat.EGO["LIN_JERK"]:nat.EGO["LIN_JERK"] + 3] = (-1.0, 0.0, 0.0)
        r["wp_count"][g, :2] = (1, 1)
        r["wp_pos"][g, 0, 0] = (12.0 + g, 4.0, 0.0)
        r["wp_heading"][g, 0, 0] = h
        r["nb_count"][g] = 1
        r["nb_pos"][g, 0] = (7.5, 1.0 - g, 0.25)
        r["nb_heading"][g, 0] = h
    return r


def rollout_rows(name, spec):
    sys.path.insert(0, os.path.join(gg.REPO, "tests"))
    import parity
    from smarts_amd.engine import SimConfig, make_spawns
    from smarts_amd.lidar import SensorParams
    from smarts_amd.map_compiler import compile_map
    from smarts_amd.sumo_map import load_net

    scen, E, N, seed, ticks, quota, kw = spec
    kw = dict(kw)
    if kw.get("lidar") == "small":
        kw["lidar"] = SensorParams(**SMALL_LIDAR)
    net = load_net(os.path.join(gg.REPO, "smarts_amd", "scenarios", scen))
    cm = compile_map(net)
    cfg = SimConfig(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, **kw)
    spawns = make_spawns(cm, E, N, episodes=1, seed=seed)
    ob = parity.OracleBatch(net, cm, cfg, spawns[0])
    rng = np.random.default_rng(seed)
    rows = ob.reset_observe()
    for _ in range(ticks):
        rows = ob.step(parity.lane_actions(rng, E, N))
    keep = np.flatnonzero(rows["active"] != 0)[:quota]
    keys = ["ego_pos", "ego_f32", "wp_pos", "wp_heading", "wp_count", "nb_pos", "nb_heading", "nb_count", "lidar_hit",
            "lidar_point", "rw_lane", "rw_path_count", "rw_count", "rw_pos", "rw_heading"]
    r = {k: np.ascontiguousarray(rows[k][keep]) for k in keys if k in rows}
    from smarts_amd import _native as nat

    r["ego_frame"] = np.concatenate([r["ego_pos"], np.array([[project_heading(h)] for h in r["ego_f32"][:, nat.EGO["HEADING"]]])], axis=1)
    return r


def reference_outputs(rad, r):
    """Run the reference's observation adapter on every agent of rows `r`; pack its output densely."""
    from smarts.core.coordinates import Dimensions as RDimensions
    from smarts.core.events import Events as REvents
    from smarts.core.plan import EndlessGoal, Mission, Start
    from smarts.core.road_map import Waypoint as RWaypoint
    from smarts.core.sensors import DrivableAreaGridMap, GridMapMetadata, OccupancyGridMap, RoadWaypoints, TopDownRGB
    from smarts.core.sensors import EgoVehicleObservation as REgo
    from smarts.core.sensors import Observation as RObservation
    from smarts.core.sensors import VehicleObservation as RVehicle
    from smarts.core.sensors import Vias as RVias

    from smarts_amd import _native as nat

    E_ = nat.EGO
    T = r["ego_pos"].shape[0]
    out = {"ec_ego_lin": np.zeros((T, 3, 3)), "ec_ego_pos": np.zeros((T, 3)), "ec_ego_heading": np.zeros(T)}
    for k in ("wp_pos", "nb_pos", "lidar_point", "rw_pos"):
        if k in r:
            out["ec_" + k] = np.zeros_like(r[k])
    for k in ("wp_heading", "nb_heading", "rw_heading"):
        if k in r:
            out["ec_" + k] = np.zeros(r[k].shape, np.float64)
    meta = GridMapMetadata(created_at=0, resolution=0.2, width=2, height=2, camera_pos=(1.0, 2.0, 3.0), camera_heading_in_degrees=30.0)
    wpt = lambda xy, h: RWaypoint(pos=np.array(xy, dtype=np.float64), heading=float(h), lane_id="l", lane_width=3.2,  # noqa: E731
                                  speed_limit=13.89, lane_index=0)
    for g in range(T):
        f = r["ego_f32"][g]
        v3 = lambda k: np.array(f[E_[k]:E_[k] + 3], dtype=np.float64)  # noqa: E731
        pos, H = np.array(r["ego_frame"][g, :3]), float(r["ego_frame"][g, 3])
        mission = Mission(start=Start(position=np.array([1.0, 2.0]), heading=0.3), goal=EndlessGoal())
        ego = REgo(id="a", position=pos, bounding_box=RDimensions(3.68, 1.47, 1.0), heading=H, speed=float(f[E_["SPEED"]]),
                   steering=0.0, yaw_rate=0.0, road_id="r", lane_id="l", lane_index=0, mission=mission,
                   linear_velocity=v3("LIN_VEL"), angular_velocity=v3("ANG_VEL"), linear_acceleration=v3("LIN_ACC"),
                   angular_acceleration=v3("ANG_ACC"), linear_jerk=v3("LIN_JERK"), angular_jerk=v3("ANG_JERK"))
        nbs = [RVehicle(id=f"n{k}", position=tuple(float(x) for x in r["nb_pos"][g, k]), bounding_box=RDimensions(3.68, 1.47, 1.0),
                        heading=float(r["nb_heading"][g, k]), speed=1.0, road_id="r", lane_id="l", lane_index=0)
               for k in range(min(int(r["nb_count"][g]), r["nb_heading"].shape[1]))]
        P, W = r["wp_heading"].shape[1:3]
        paths = [[wpt(r["wp_pos"][g, p, w, :2], r["wp_heading"][g, p, w]) for w in range(min(int(r["wp_count"][g, 1 + p]), W))]
                 for p in range(min(int(r["wp_count"][g, 0]), P))]
        lidar = []
        if "lidar_point" in r:
            pts = [np.array(p) for p in r["lidar_point"][g]]
            lidar = (pts, [bool(h) for h in r["lidar_hit"][g]], [(pos.copy(), pos + 1.0) for _ in pts])
        rw = None
        if "rw_pos" in r:
            lanes = {}
            for l in range(r["rw_lane"].shape[1]):
                if r["rw_lane"][g, l] < 0:
                    continue
                lanes[l] = [[wpt(r["rw_pos"][g, l, p, w, :2], r["rw_heading"][g, l, p, w]) for w in range(int(r["rw_count"][g, l, p]))]
                            for p in range(min(int(r["rw_path_count"][g, l]), r["rw_count"].shape[2]))]
            rw = RoadWaypoints(lanes=lanes)
        ev = REvents(collisions=[], off_road=False, off_route=False, on_shoulder=False, wrong_way=False, not_moving=False,
                     reached_goal=False, reached_max_episode_steps=False, agents_alive_done=False)
        grid = np.zeros((2, 2, 1), np.uint8)
        obs = RObservation(dt=0.1, step_count=1, elapsed_sim_time=0.1, events=ev, ego_vehicle_state=ego,
                           neighborhood_vehicle_states=nbs, waypoint_paths=paths, distance_travelled=0.0,
                           lidar_point_cloud=lidar, drivable_area_grid_map=DrivableAreaGridMap(meta, grid),
                           occupancy_grid_map=OccupancyGridMap(meta, grid), top_down_rgb=TopDownRGB(meta, grid),
                           road_waypoints=rw, via_data=RVias(near_via_points=[], hit_via_points=[]))
        with np.errstate(invalid="ignore"):
            new = rad.ego_centric_observation_adapter(obs)
        e = new.ego_vehicle_state
        out["ec_ego_pos"][g], out["ec_ego_heading"][g] = e.position, float(e.heading)
        out["ec_ego_lin"][g] = (e.linear_velocity, e.linear_acceleration, e.linear_jerk)
        for k, nv in enumerate(new.neighborhood_vehicle_states):
            out["ec_nb_pos"][g, k], out["ec_nb_heading"][g, k] = nv.position, float(nv.heading)
        for p, path in enumerate(new.waypoint_paths):
            for w, wp in enumerate(path):
                out["ec_wp_pos"][g, p, w, :2], out["ec_wp_heading"][g, p, w] = wp.pos, float(wp.heading)
        if "lidar_point" in r:
            out["ec_lidar_point"][g] = np.array(new.lidar_point_cloud[0])
        if rw is not None:
            for l, lane_paths in new.road_waypoints.lanes.items():
                for p, path in enumerate(lane_paths):
                    for w, wp in enumerate(path):
                        out["ec_rw_pos"][g, l, p, w, :2], out["ec_rw_heading"][g, l, p, w] = wp.pos, float(wp.heading)
    return out


class _Obs:  # what the action adapters read of last_obs
    def __init__(self, pos, H):
        self.ego_vehicle_state = type("E", (), dict(position=np.array(pos), heading=float(H)))()


def action_cases(rad):
    rng = np.random.default_rng(17)
    T, M = 12, 6
    frame = np.column_stack([rng.uniform(-200, 200, T), rng.uniform(-200, 200, T), np.zeros(T), rng.uniform(-math.pi, math.pi, T)])
    frame[0] = (161.23485529, 3.2, 0.0, -1.5707963267948966)  # the reference test's fixture pose
    frame[1, 3], frame[2, 3] = math.pi, 0.0
    flags = np.ones(T, np.uint8)
    flags[3] = 0  # last_obs is None
    out = {"frame": frame, "flags": flags}
    # ---- Trajectory [T, 4, 11]
    traj = np.zeros((T, 4, 11))
    counts = rng.integers(1, 14, T).astype(np.int32)
    counts[4] = 0
    traj[:, 0], traj[:, 1] = rng.uniform(-30, 30, (T, 11)), rng.uniform(-30, 30, (T, 11))
    traj[:, 2], traj[:, 3] = rng.uniform(-7, 7, (T, 11)), rng.uniform(0, 20, (T, 11))
    traj[0, :, :2], traj[0, :, 10], counts[0] = [[1, 2], [5, 6], [0.3, 3.14], [20.0, 21.0]], [2, 6, 3.14, 21.0], 2
    want = traj.copy()
    for g in range(T):
        if not flags[g] or counts[g] == 0:
            continue
        cols = list(range(min(int(counts[g]), 10))) + [10]
        res = rad._trajectory_adaption(tuple(traj[g][:, cols]), _Obs(frame[g, :3], frame[g, 3]))
        for k in range(4):
            want[g, k, cols] = res[k]
    out.update(traj_in=traj, traj_counts=counts, traj_ref=want)
    # ---- TargetPose [T, 4]
    pose = np.column_stack([rng.uniform(-30, 30, T), rng.uniform(-30, 30, T), rng.uniform(-7, 7, T), rng.uniform(0.1, 2, T)])
    pose[0] = (2, 4, -2.9, 20)
    pose[5, 0] = np.nan
    want = pose.copy()
    for g in range(T):
        if flags[g] and not np.isnan(pose[g, 0]):
            want[g] = rad._egocentric_target_pose_adapter(tuple(pose[g]), _Obs(frame[g, :3], frame[g, 3]))
    out.update(pose_in=pose, pose_ref=want)
    # ---- TrajectoryWithTime [T, 5, M]: time, x, y, heading, speed; the adapter on rows 1-3, reassembled
    twt = np.zeros((T, 5, M))
    tcounts = rng.integers(2, M + 1, T).astype(np.int32)
    tcounts[4] = 0
    twt[:, 0] = np.cumsum(rng.uniform(0.05, 0.3, (T, M)), axis=1)
    twt[:, 1], twt[:, 2] = rng.uniform(-30, 30, (T, M)), rng.uniform(-30, 30, (T, M))
    twt[:, 3], twt[:, 4] = rng.uniform(-7, 7, (T, M)), rng.uniform(0, 20, (T, M))
    twt[0, :, :2], tcounts[0] = [[0.1, 0.2], [1, 2], [5, 6], [0.3, 3.14], [20.0, 21.0]], 2
    want = twt.copy()
    for g in range(T):
        n = int(tcounts[g])
        if not flags[g] or n == 0:
            continue
        res = rad._trajectory_adaption(tuple(twt[g, 1:4, :n]), _Obs(frame[g, :3], frame[g, 3]))
        for k in range(3):
            want[g, 1 + k, :n] = res[k]
    out.update(twt_in=twt, twt_counts=tcounts, twt_ref=want)
    # the reference test's expected values (to its own np.allclose)
    out["kat_traj"] = np.array([[166.23485529, 167.23485529], [2.2, 1.2], [-1.27079633, 1.56920367], [20.0, 21.0]])
    out["kat_pose"] = np.array([165.23485529, 1.2, 1.81238898, 20.0])
    return out


def main():
    gg.install_reference()
    for name in ("gym.envs", "gym.envs.registration", "gym.wrappers"):
        gg._stub(name)
    from smarts.core.utils.adapters import ego_centric_adapters as rad

    out = {}
    groups = {name: rollout_rows(name, spec) for name, spec in GROUPS.items()}
    groups["hand"] = hand_rows()
    for name, r in groups.items():
        for k, v in r.items():
            out[f"{name}_in_{k}"] = v
        for k, v in reference_outputs(rad, r).items():
            out[f"{name}_ref_{k}"] = v
    out["groups"] = np.array(sorted(groups))
    np.savez_compressed(os.path.join(HERE, "ego_centric_cases.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "ego_centric_actions.npz"), **action_cases(rad))
    print({k: v["ego_pos"].shape[0] for k, v in groups.items()})


if __name__ == "__main__":
    main()

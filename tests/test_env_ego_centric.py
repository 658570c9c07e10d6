"""The ego-centric adapters of the object path (``smarts_amd.env.ego_centric_adapters``) and ``FormatObs.from_rows(...,
ego_centric=True)`` against the reference's outputs (``tests/golden/ego_centric_cases.npz`` / ``ego_centric_actions.npz``),
and the checks of the new ABI that need no device: ``smx_check_buffers``, ``smx_struct_size``, the sensor mask and the
launch plan with and without the bit.  CPU only."""
import ctypes as C
import dataclasses
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from smarts_amd import _native as nat
from smarts_amd.engine import SimConfig
from smarts_amd.env import ActionSpaceType, FormatObs, ego_centric_observation_adapter, get_egocentric_adapters
from smarts_amd.env.ego_centric_rows import ego_centric_rows
from smarts_amd.env.format_obs import std_obs
from smarts_amd.env.observations import (
    FixedRouteMission, GridMapMetadata, Heading, ObservationBuilder, OccupancyGridMap, PositionalGoal, ViaPoint, Vias,
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ROLLOUTS = ("loop", "4lane", "minicity")


@pytest.fixture(scope="module")
def cases():
    """Per rollout group: the rows (with the columns an ``Observation`` also needs), the reference's outputs, and the
    ``Observation`` of every agent built from those rows."""
    z = np.load(os.path.join(GOLDEN, "ego_centric_cases.npz"))
    groups = {}
    for name in ROLLOUTS:
        rows = {k[len(name) + 4:]: z[k] for k in z.files if k.startswith(name + "_in_")}
        ref = {k[len(name) + 5:]: z[k] for k in z.files if k.startswith(name + "_ref_")}
        T = rows["ego_pos"].shape[0]
        rows.update(ego_lane=np.zeros((T, 2), np.int16), events=np.zeros((T, nat.EV_COUNT), np.uint8), dist=np.arange(T, dtype=np.float64),
                    nb_box=np.ones(rows["nb_pos"].shape, np.float32), nb_speed=np.ones(rows["nb_heading"].shape, np.float32),
                    nb_slot=np.zeros(rows["nb_heading"].shape, np.int8))
        for k, dt in (("lane_index", np.int8), ("lane_id", np.int16)):
            rows["nb_" + k] = np.zeros(rows["nb_heading"].shape, dt)
        for pre in ("wp", "rw"):
            if pre + "_heading" in rows:
                shape = rows[pre + "_heading"].shape
                rows.update({f"{pre}_lane_width": np.full(shape, 3.2, np.float32), f"{pre}_speed_limit": np.full(shape, 13.89, np.float32),
                             f"{pre}_lane_index": np.zeros(shape, np.int8), f"{pre}_lane_id": np.zeros(shape, np.int16)})
        # (rows beyond the counts are zero, as the world rows have them)
        nb = np.arange(rows["nb_heading"].shape[1])[None, :] < rows["nb_count"][:, None]
        rows["nb_box"], rows["nb_speed"] = rows["nb_box"] * nb[..., None], rows["nb_speed"] * nb
        P, W = rows["wp_heading"].shape[1:]
        wp = (np.arange(P)[None, :, None] < rows["wp_count"][:, :1, None]) & (np.arange(W)[None, None, :] < rows["wp_count"][:, 1:, None])
        rows["wp_lane_width"], rows["wp_speed_limit"] = rows["wp_lane_width"] * wp, rows["wp_speed_limit"] * wp
        lidar = "lidar_point" in rows
        builder = ObservationBuilder([f"lane_{i}" for i in range(512)], ["road"] * 512, [f"a{i}" for i in range(T)], waypoints=True,
                                     neighbors=True, accelerometer=True, road_waypoints="rw_pos" in rows,
                                     lidar_rays=np.ones((rows["lidar_point"].shape[1], 3)) if lidar else None)
        groups[name] = (rows, ref, [builder.build(rows, g, 1, 0.1) for g in range(T)])
    return groups


def test_object_adapter_matches_the_reference(cases):
    for name, (rows, ref, observations) in cases.items():
        for g, obs in enumerate(observations):
            assert float(obs.ego_vehicle_state.heading) == rows["ego_frame"][g, 3]  # the frame the reference was given
            new = ego_centric_observation_adapter(obs)
            e = new.ego_vehicle_state
            assert not np.asarray(e.position).any() and e.heading == 0 and isinstance(e.heading, Heading)
            got = np.array([e.linear_velocity, e.linear_acceleration, e.linear_jerk])
            assert np.array_equal(got, ref["ec_ego_lin"][g]), (name, g)
            assert np.array_equal(e.angular_velocity, obs.ego_vehicle_state.angular_velocity)
            for k, nv in enumerate(new.neighborhood_vehicle_states):
                assert np.array_equal(nv.position, ref["ec_nb_pos"][g, k]), (name, g, k)
                assert np.float32(nv.heading) == np.float32(ref["ec_nb_heading"][g, k]), (name, g, k)
            assert len(new.waypoint_paths) == min(int(rows["wp_count"][g, 0]), 4)
            for p, path in enumerate(new.waypoint_paths):
                for w, wp in enumerate(path):
                    assert np.array_equal(wp.pos, ref["ec_wp_pos"][g, p, w, :2]), (name, g, p, w)
                    assert np.float32(wp.heading) == np.float32(ref["ec_wp_heading"][g, p, w])
                    assert wp.lane_width == obs.waypoint_paths[p][w].lane_width
            if "ec_lidar_point" in ref:
                assert np.array_equal(np.array(new.lidar_point_cloud[0]), ref["ec_lidar_point"][g], equal_nan=True)
                assert new.lidar_point_cloud[1] == obs.lidar_point_cloud[1]
            if "ec_rw_pos" in ref:
                lanes = [l for l in range(rows["rw_lane"].shape[1]) if rows["rw_lane"][g, l] >= 0]
                assert len(new.road_waypoints.lanes) == len(set(int(rows["rw_lane"][g, l]) for l in lanes))
                for l, lane_paths in zip(lanes, new.road_waypoints.lanes.values()):
                    for p, path in enumerate(lane_paths):
                        for w, wp in enumerate(path):
                            assert np.array_equal(wp.pos, ref["ec_rw_pos"][g, l, p, w, :2]), (name, g, l, p, w)
                            assert np.float32(wp.heading) == np.float32(ref["ec_rw_heading"][g, l, p, w])
            assert obs.ego_vehicle_state.position.any()  # the input is not modified


def test_from_rows_ego_centric_equals_format_obs_of_the_adapted_observation(cases):
    for name, (rows, _, observations) in cases.items():
        world = {k: v for k, v in rows.items() if k != "ego_frame"}  # the frame an Observation of these rows has
        both = dict(world, **ego_centric_rows(world))
        shaped = {k: v[None] for k, v in both.items()}
        for g, obs in enumerate(observations):
            adapted = ego_centric_observation_adapter(obs)
            cloud = adapted.lidar_point_cloud  # (StdObs' lidar block has the default sensor's 300 rays: compared below)
            want = std_obs(dataclasses.replace(adapted, lidar_point_cloud=None))
            got = FormatObs.from_rows(shaped, 0, g, ego_centric=True)
            assert got.dist == want.dist
            for k, v in want.ego.items():
                assert np.array_equal(got.ego[k], v, equal_nan=True), (name, g, k)
            assert got.events == want.events
            for block in ("neighbors", "waypoints"):
                a, b = getattr(got, block), getattr(want, block)
                assert (a is None) == (b is None), (name, g, block)
                for k, v in (b or {}).items():
                    assert a[k].dtype == v.dtype and np.array_equal(a[k], v), (name, g, block, k)
            if cloud is not None:
                assert np.array_equal(got.lidar["hit"], np.array(cloud[1], dtype=np.int8))
                assert np.array_equal(got.lidar["point_cloud"], np.nan_to_num(np.array(cloud[0]), nan=0.0))  # misses: 0 (format_obs.py:452-489)
            # (ttc: lane_ttc of the observation, invariant under the frame; from_rows keeps the world rows' block)
        with pytest.raises(ValueError):
            FormatObs.from_rows({k: v[None] for k, v in world.items()}, 0, 0, ego_centric=True)


def test_missions_vias_and_camera_metadata(cases):
    obs = cases["loop"][2][0]
    ego = obs.ego_vehicle_state
    pos, H = ego.position, float(ego.heading)
    ahead = pos[:2] + 10.0 * np.array([-math.sin(H), math.cos(H)])  # ten metres along the heading (0 = +y)
    mission = FixedRouteMission(tuple(pos[:2]), H, PositionalGoal(tuple(ahead), 2.0), ("r0",))
    via = ViaPoint(position=tuple(ahead), lane_index=0, road_id="r0", required_speed=5.0)
    meta = GridMapMetadata(created_at=0, resolution=0.2, width=2, height=2, camera_pos=tuple(pos), camera_heading_in_degrees=30.0)
    obs = dataclasses.replace(obs, ego_vehicle_state=ego._replace(mission=mission), via_data=Vias([via], [via]),
                              occupancy_grid_map=OccupancyGridMap(meta, np.zeros((2, 2, 1), np.uint8)))
    new = ego_centric_observation_adapter(obs)
    m = new.ego_vehicle_state.mission
    assert np.allclose(m.start_position, (0, 0), atol=1e-12) and abs(m.start_heading) < 1e-12
    assert np.allclose(m.goal.position, (0.0, 10.0), atol=1e-9) and m.goal.radius == 2.0  # ahead is +y: a heading of 0 points along +y
    for v in new.via_data.near_via_points + new.via_data.hit_via_points:
        assert len(v.position) == 2 and np.allclose(v.position, (0.0, 10.0), atol=1e-9) and v.required_speed == 5.0
    assert new.occupancy_grid_map.metadata.camera_pos == (0, 0, 0) and new.occupancy_grid_map.metadata.camera_heading_in_degrees == 0
    assert new.drivable_area_grid_map is None and new.top_down_rgb is None


def test_paired_action_adapter_uses_the_unmodified_last_observation(cases):
    acts = dict(np.load(os.path.join(GOLDEN, "ego_centric_actions.npz")))
    obs0 = cases["loop"][2][0]
    frame = acts["frame"]

    def at(g):
        e = obs0.ego_vehicle_state._replace(position=np.array(frame[g, :3]), heading=float(frame[g, 3]))
        return dataclasses.replace(obs0, ego_vehicle_state=e)

    for space, key, first in ((ActionSpaceType.Trajectory, "traj", 0), (ActionSpaceType.TrajectoryWithTime, "twt", 1)):
        oa, aa = get_egocentric_adapters(space)
        g, n = 0, int(acts[key + "_counts"][0])
        act = tuple(acts[key + "_in"][g][:, :n])
        assert all(np.array_equal(a, b) for a, b in zip(aa(act), act))  # before any observation: passed through
        adapted = oa(at(g))
        assert adapted.ego_vehicle_state.heading == 0  # (the adapter returned the ego-frame observation ...)
        got = np.array(aa(act))  # (... and kept the unmodified one for the action)
        assert np.array_equal(got, acts[key + "_ref"][g][:, :n]), space
        assert np.allclose(got[first:first + 4], acts["kat_traj"])
    oa, aa = get_egocentric_adapters(ActionSpaceType.TargetPose)
    assert aa((2, 4, -2.9, 20)) == (2, 4, -2.9, 20)
    for g in (0, 1, 2, 6):
        oa(at(g))
        assert np.array_equal(aa(tuple(acts["pose_in"][g])), acts["pose_ref"][g]), g
    oa(at(0))
    assert np.allclose(aa((2, 4, -2.9, 20)), (165.23485529, 1.2, 1.81238898, 20.0))
    oa, aa = get_egocentric_adapters(ActionSpaceType.MPC)
    oa(at(0))
    assert np.allclose(np.array(aa(tuple(acts["traj_in"][0][:, :2]))), acts["kat_traj"])


def test_frame_free_actions_come_back_untouched(cases):
    obs = cases["loop"][2][0]
    for space, act in ((ActionSpaceType.Lane, "keep_lane"), (ActionSpaceType.Continuous, [0.9, 0.8, 0.7]),
                       (ActionSpaceType.ActuatorDynamic, [1.0, 1.0, 1.0]), (ActionSpaceType.LaneWithContinuousSpeed, [0, 20.2]),
                       (ActionSpaceType.Imitation, (2, 2))):
        oa, aa = get_egocentric_adapters(space)
        assert aa(act) is act
        oa(obs)
        assert aa(act) is act
    oa, aa = get_egocentric_adapters(ActionSpaceType.MultiTargetPose)
    with pytest.raises(ValueError):
        aa({"v": (1, 2, 3, 4)})


# ---- the ABI, no device ----
def _declared(sensors, E=3, N=4, rays=7):
    """An smx_config and structs with fake pointers (never dereferenced by smx_check_buffers) of exactly the extents
    the configuration needs."""
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.dt, c.sensors = E, N, 0.1, sensors
    c.wp_lookahead, c.wp_paths, c.wp_len, c.nb_max, c.nb_radius = 32, 4, 20, 10, 50.0
    c.lidar_rays, c.lidar_max_distance, c.rw_horizon, c.rw_lanes, c.rw_paths = rays, 20.0, 4, 4, 2
    n, PW, K, RW = E * N, 4 * 20, 10, 4 * 2 * 9
    st, sp, out = nat.SmxState(), nat.SmxSpawns(), nat.SmxOutputs()
    state = dict(f64=(nat.S_COUNT * n, nat.DT_F64), flags=(n, nat.DT_I32), steps=(n, nat.DT_I32), env_ticks=(E, nat.DT_I32),
                 env_done_count=(E, nat.DT_I32), env_episode=(E, nat.DT_I32), driven_path=(n * 500, nat.DT_F64),
                 seed_cache=(nat.SEED_COUNT * n, nat.DT_I32), facts_i32=(nat.FACT_I_COUNT * n, nat.DT_I32),
                 facts_f64=(nat.FACT_F_COUNT * n, nat.DT_F64), env_reset_pending=(E, nat.DT_I32))
    for k, name in enumerate(nat.STATE_BUFFERS):
        setattr(st, name, 0x1000 + k)
        st.count[k], st.dtype[k] = state[name]
    sp.episodes, sp.pose, sp.pose_count = 2, 0x2000, 2 * n * 4
    outs = dict(ego_pos=(3 * n, nat.DT_F64), ego_f32=(nat.EGO_F32_COUNT * n, nat.DT_F32), ego_lane=(2 * n, nat.DT_I16),
                events=(9 * n, nat.DT_U8), reward=(n, nat.DT_F64), dist=(n, nat.DT_F64), done=(n, nat.DT_U8),
                active=(n, nat.DT_U8), env_done=(E, nat.DT_U8),
                ego_frame=(4 * n, nat.DT_F64), ec_flags=(n, nat.DT_U8), ec_ego_f32=(nat.EGO_F32_COUNT * n, nat.DT_F32))
    if sensors & nat.SENSOR_WAYPOINTS:
        outs.update(wp_pos=(n * PW * 3, nat.DT_F64), wp_heading=(n * PW, nat.DT_F32), wp_lane_width=(n * PW, nat.DT_F32),
                    wp_speed_limit=(n * PW, nat.DT_F32), wp_lane_index=(n * PW, nat.DT_I8), wp_lane_id=(n * PW, nat.DT_I16),
                    wp_count=(n * 5, nat.DT_U8), ec_wp_pos=(n * PW * 3, nat.DT_F64), ec_wp_heading=(n * PW, nat.DT_F32))
    if sensors & nat.SENSOR_NEIGHBORS:
        outs.update(nb_pos=(n * K * 3, nat.DT_F64), nb_box=(n * K * 3, nat.DT_F32), nb_heading=(n * K, nat.DT_F32),
                    nb_speed=(n * K, nat.DT_F32), nb_lane_index=(n * K, nat.DT_I8), nb_lane_id=(n * K, nat.DT_I16),
                    nb_slot=(n * K, nat.DT_I8), nb_count=(n, nat.DT_U8), ec_nb_pos=(n * K * 3, nat.DT_F64),
                    ec_nb_heading=(n * K, nat.DT_F32))
    if sensors & nat.SENSOR_LIDAR:
        outs.update(lidar_hit=(n * rays, nat.DT_U8), lidar_point=(n * rays * 3, nat.DT_F64), ec_lidar_point=(n * rays * 3, nat.DT_F64))
    if sensors & nat.SENSOR_ROAD_WAYPOINTS:
        outs.update(rw_lane_count=(n, nat.DT_U8), rw_lane=(n * 4, nat.DT_I16), rw_path_count=(n * 4, nat.DT_I16), rw_count=(n * 8, nat.DT_U8),
                    rw_pos=(n * RW * 3, nat.DT_F64), rw_heading=(n * RW, nat.DT_F32), rw_lane_width=(n * RW, nat.DT_F32),
                    rw_speed_limit=(n * RW, nat.DT_F32), rw_lane_index=(n * RW, nat.DT_I8), rw_lane_id=(n * RW, nat.DT_I16),
                    ec_rw_pos=(n * RW * 3, nat.DT_F64), ec_rw_heading=(n * RW, nat.DT_F32))
    for k, name in enumerate(nat.OUTPUT_BUFFERS):
        if name in outs:
            setattr(out, name, 0x3000 + k)
            out.count[k], out.dtype[k] = outs[name]
    return c, st, sp, out


def _check(c, st, sp, out):
    err = C.create_string_buffer(512)
    rc = nat.load_library().smx_check_buffers(C.byref(c), 0, C.byref(st), C.byref(sp), C.byref(out), err, 512)
    return rc, err.value.decode()


ALL = (nat.SENSOR_WAYPOINTS | nat.SENSOR_NEIGHBORS | nat.SENSOR_LIDAR | nat.SENSOR_ROAD_WAYPOINTS | nat.SENSOR_EGO_CENTRIC)


def test_entry_check_of_the_ego_centric_buffers():
    c, st, sp, out = _declared(ALL)
    assert _check(c, st, sp, out) == (0, "")
    wrong = {nat.DT_F64: nat.DT_F32, nat.DT_F32: nat.DT_F64, nat.DT_U8: nat.DT_I8}
    for name in nat.EC_OUTPUT_FIELDS:
        k = nat.OUTPUT_BUFFERS.index(name)
        keep = getattr(out, name)
        setattr(out, name, None)
        rc, msg = _check(c, st, sp, out)
        assert rc == -1 and f"out.{name} is NULL" in msg, (name, rc, msg)
        setattr(out, name, keep)
        out.count[k] -= 1
        rc, msg = _check(c, st, sp, out)
        assert rc == -1 and f"out.{name}:" in msg and "elements declared" in msg, (name, rc, msg)
        out.count[k] += 1
        right = out.dtype[k]
        out.dtype[k] = wrong[right]
        rc, msg = _check(c, st, sp, out)
        assert rc == -1 and f"out.{name}:" in msg and "dtype" in msg, (name, rc, msg)
        out.dtype[k] = right
    assert _check(c, st, sp, out) == (0, "")


def test_entry_check_accepts_null_rows_of_disabled_sensors_and_of_a_config_without_the_bit():
    c, st, sp, out = _declared(nat.SENSOR_NEIGHBORS | nat.SENSOR_EGO_CENTRIC)  # no waypoints, lidar, road waypoints
    for name in ("ec_wp_pos", "ec_wp_heading", "ec_lidar_point", "ec_rw_pos", "ec_rw_heading"):
        assert not getattr(out, name)
    assert _check(c, st, sp, out) == (0, "")
    c, st, sp, out = _declared(ALL)
    c.sensors &= ~nat.SENSOR_EGO_CENTRIC
    for name in nat.EC_OUTPUT_FIELDS:
        setattr(out, name, None)
    assert _check(c, st, sp, out) == (0, "")


def test_struct_sizes_indices_and_the_sensor_mask():
    lib = nat.load_library()
    assert lib.smx_struct_size(4) == C.sizeof(nat.SmxOutputs) and lib.smx_struct_size(0) == C.sizeof(nat.SmxConfig)
    # appended: every index before the new pointers keeps its value
    assert nat.OUTPUT_BUFFERS[:len(nat.OUTPUT_FIELDS)] == nat.OUTPUT_FIELDS and nat.OUTPUT_BUFFERS.index("lane_ttc_flags") == 49
    assert nat.OUTPUT_BUFFERS[50:] == nat.EC_OUTPUT_FIELDS and nat.SENSOR_EGO_CENTRIC == 1 << 8
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "SMX_SENSOR_EGO_CENTRIC = 1 << 8" in header and "int smx_actions_to_world(" in header
    order = header[header.index("SMX_OUT_LANE_TTC_FLAGS,"):header.index("SMX_OUT_BUFFERS")]
    assert [s.strip()[8:].lower() for s in order.replace("\n", " ").split(",")[1:-1]] == nat.EC_OUTPUT_FIELDS
    assert SimConfig().sensors_mask() == nat.SENSOR_WAYPOINTS | nat.SENSOR_ACCELEROMETER  # the default is unchanged
    assert SimConfig(ego_centric=True).sensors_mask() == SimConfig().sensors_mask() | nat.SENSOR_EGO_CENTRIC
    assert "smx_actions_to_world" in nat.EXPORTS


def test_launch_plan_is_the_parents_without_the_bit_and_gains_one_launch_with_it(tmp_path):
    lib_path = str(tmp_path / "libhost_plan_ego.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "host_plan_ego.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_ego.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    arg, out = (C.c_int * 16)(), (C.c_longlong * 64)()

    def plan(*values):
        arg[:] = values
        n = lib.host_plan_ego(arg, out)
        return list(out[:n])

    base = nat.SENSOR_WAYPOINTS | nat.SENSOR_NEIGHBORS
    checked = 0
    for (envs, nv), strategy, junctions, lidar, ttc, timing, is_step, blobs in itertools.product(
            [(2, 4), (3, 5), (512, 32), (513, 32), (2049, 64)], range(5), (0, 1), (0, 1), (0, 1), (0, 2), (0, 1), (31, 0)):
        sensors = base | (nat.SENSOR_LIDAR if lidar else 0) | (nat.SENSOR_LANE_TTC if ttc else 0)
        rest = (strategy, junctions, 0, sensors, 4, 0, 0, timing, is_step, blobs, 1, 0, 0, 0)
        off = plan(envs, nv, *rest)
        on = plan(envs, nv, *rest[:3], sensors | nat.SENSOR_EGO_CENTRIC, *rest[4:])
        assert off[-3:] == [0, 0, 0], (envs, nv, rest)  # no flag, no grid: the parent's launches
        assert on[:-3] == off[:-3], (envs, nv, rest)  # every other decision is untouched by the bit
        total, apb = envs * nv, 64 // 16
        obs_blocks, reset_pass = off[29], off[24]
        assert on[-3:] == [1, -(-total // apb), obs_blocks * 16 if reset_pass else 0], (envs, nv, rest, on[-3:])
        checked += 1
    assert checked == 5 * 5 * 2 * 2 * 2 * 2 * 2 * 2

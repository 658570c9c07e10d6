"""Record what the device-free half of the C-ABI answers, message for message (tests/golden/host_checks.json).

    python tests/golden/gen_golden_host_checks.py          # rewrites the fixture from the built library

`sweep(lib)` drives smx_check_buffers, smx_check_frame_stack, smx_check_rgb_output, smx_check_guard,
smx_check_mission_goals and the validation of smx_create through ctypes with fake non-NULL pointers (none of them is
dereferenced: no device is needed) and yields (label, return code, message) for every case, in a fixed order.
tests/test_host_checks.py replays the same sweep against the built library and compares both fields with the fixture,
case by case.  The fixture keeps every distinct message once and the cases as [return code, message index].

The extents below are this file's own statement of include/smx.h (the element count of every caller buffer), not a
copy of the library's table: a case "one element short" is one short of THESE numbers.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "host_checks.json")
E, N = 3, 4
DT_SIZE = {1: 8, 2: 4, 3: 4, 4: 2, 5: 1, 6: 1, 7: 8}  # SMX_DT_* -> bytes
ALL_SENSORS = (1 << 10) - 1


def _nat():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from smarts_amd import _native as nat

    return nat


def config(nat, **over):
    """The shape numbers every configuration of the sweep shares; `sensors` and the switches come from `over`."""
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.dt = E, N, 0.1
    c.wp_lookahead, c.wp_paths, c.wp_len, c.nb_max, c.nb_radius = 32, 4, 20, 10, 50.0
    c.ogm_width, c.ogm_height, c.ogm_resolution, c.lidar_rays, c.lidar_max_distance = 64, 64, 0.5, 100, 20.0
    c.dagm_width, c.dagm_height, c.dagm_resolution = 32, 32, 0.5
    c.rw_horizon, c.rw_lanes, c.rw_paths = 2, 3, 2
    c.rgb_width, c.rgb_height, c.rgb_resolution = 16, 8, 0.5
    for k, v in over.items():
        setattr(c, k, v)
    return c


def extents(nat, c, episodes=2):
    """name -> (elements, SMX_DT_*) of every state / spawn / output buffer as the entry check sizes a non-NULL one: from
    the shape numbers whether or not the sensor is on, except the road-waypoint rows (0 with the sensor off)."""
    T, Ev = c.num_envs * c.num_vehicles, c.num_envs
    PW, K, R, V = c.wp_paths * c.wp_len, c.nb_max, c.lidar_rays, max(c.via_max, 0)
    rw = bool(c.sensors & nat.SENSOR_ROAD_WAYPOINTS)
    L = c.rw_lanes if rw else 0
    LP = L * (c.rw_paths if rw else 0)
    LPR = LP * ((2 * c.rw_horizon + 1) if rw else 0)
    F64, F32, I32, I16, I8, U8, U64 = nat.DT_F64, nat.DT_F32, nat.DT_I32, nat.DT_I16, nat.DT_I8, nat.DT_U8, nat.DT_U64
    state = dict(f64=(nat.S_COUNT * T, F64), flags=(T, I32), steps=(T, I32), env_ticks=(Ev, I32), env_done_count=(Ev, I32),
                 env_episode=(Ev, I32), driven_path=(T * 500, F64), seed_cache=(nat.SEED_COUNT * T, I32),
                 facts_i32=(nat.FACT_I_COUNT * T, I32), facts_f64=(nat.FACT_F_COUNT * T, F64), env_reset_pending=(Ev, I32))
    spawns = dict(pose=(episodes * T * 4, F64), social=(episodes * T * 2, F64))
    ego = dict(ego_pos=(3 * T, F64), ego_f32=(nat.EGO_F32_COUNT * T, F32), ego_lane=(2 * T, I16), events=(9 * T, U8), dist=(T, F64))
    out = dict(ego, reward=(T, F64), done=(T, U8), active=(T, U8), env_done=(Ev, U8),
               via_near=(T * V, I8), via_near_count=(T, U8), via_hit=(T, I32), learner=(2 * T, F32),
               wp_pos=(T * PW * 3, F64), wp_heading=(T * PW, F32), wp_lane_width=(T * PW, F32), wp_speed_limit=(T * PW, F32),
               wp_lane_index=(T * PW, I8), wp_lane_id=(T * PW, I16), wp_count=(T * (c.wp_paths + 1), U8),
               nb_pos=(T * K * 3, F64), nb_box=(T * K * 3, F32), nb_heading=(T * K, F32), nb_speed=(T * K, F32),
               nb_lane_index=(T * K, I8), nb_lane_id=(T * K, I16), nb_slot=(T * K, I8), nb_count=(T, U8),
               ogm=(T * c.ogm_width * c.ogm_height, U8), lidar_hit=(T * R, U8), lidar_point=(T * R * 3, F64),
               dagm=(T * c.dagm_width * c.dagm_height, U8), collidees=(T, U64),
               rw_lane_count=(T, U8), rw_lane=(T * L, I16), rw_path_count=(T * L, I16), rw_count=(T * LP, U8),
               rw_pos=(T * LPR * 3, F64), rw_heading=(T * LPR, F32), rw_lane_width=(T * LPR, F32),
               rw_speed_limit=(T * LPR, F32), rw_lane_index=(T * LPR, I8), rw_lane_id=(T * LPR, I16),
               lane_ttc=(nat.TTC_COUNT * T, F64), lane_ttc_flags=(T, U8),
               ego_frame=(4 * T, F64), ec_flags=(T, U8), ec_ego_f32=(nat.EGO_F32_COUNT * T, F32),
               ec_wp_pos=(T * PW * 3, F64), ec_wp_heading=(T * PW, F32), ec_nb_pos=(T * K * 3, F64), ec_nb_heading=(T * K, F32),
               ec_lidar_point=(T * R * 3, F64), ec_rw_pos=(T * LPR * 3, F64), ec_rw_heading=(T * LPR, F32))
    for name, ext in ego.items():
        out["final_" + name] = ext
    assert set(out) == set(nat.OUTPUT_BUFFERS) and set(state) == set(nat.STATE_BUFFERS)
    return state, spawns, out


FINALS = ["final_ego_pos", "final_ego_f32", "final_ego_lane", "final_events", "final_dist"]
REQUIRED_OUT = ["ego_pos", "ego_f32", "ego_lane", "events", "reward", "dist", "done", "active", "env_done"]
DECLARED_OUT = REQUIRED_OUT + ["learner", "wp_pos", "wp_heading", "wp_lane_width", "wp_speed_limit", "wp_lane_index",
                               "wp_lane_id", "wp_count", "nb_pos", "nb_box", "nb_heading", "nb_speed", "nb_lane_index",
                               "nb_lane_id", "nb_slot", "nb_count", "ogm", "lidar_hit", "lidar_point", "collidees"]


def configurations(nat):
    """(label, config, extents the buffers are sized by, names of the buffers given)."""
    everything = config(nat, sensors=ALL_SENSORS, via_max=4, num_social=1, social_speed_factor=1.0,
                        done_criteria=nat.DONE_NOT_MOVING, frame_stack=4)
    declared = config(nat, sensors=nat.SENSOR_WAYPOINTS | nat.SENSOR_NEIGHBORS | nat.SENSOR_OGM | nat.SENSOR_LIDAR,
                      dagm_width=0, dagm_height=0, dagm_resolution=0.0, rw_horizon=0, rw_lanes=0, rw_paths=0,
                      rgb_width=0, rgb_height=0, rgb_resolution=0.0)
    bare = config(nat, sensors=0, wp_lookahead=0, wp_paths=0, wp_len=0, nb_max=0, ogm_width=0, ogm_height=0, lidar_rays=0,
                  dagm_width=0, dagm_height=0, rw_horizon=0, rw_lanes=0, rw_paths=0, rgb_width=0, rgb_height=0)
    oversized = config(nat, sensors=0, via_max=4, frame_stack=4)
    every = set(nat.STATE_BUFFERS) | {"pose", "social"} | set(nat.OUTPUT_BUFFERS)
    basic = set(nat.STATE_BUFFERS) | {"pose"}
    return [
        ("everything", everything, extents(nat, everything), every),
        ("declared", declared, extents(nat, declared), basic | set(DECLARED_OUT)),
        ("bare", bare, extents(nat, bare), (basic - {"driven_path"}) | set(REQUIRED_OUT)),
        ("oversized", oversized, extents(nat, everything), every),
    ]


def structs(nat, ext, given, episodes=2, change=None):
    """The three structs with fake pointers for the buffers in `given`.  change = (name, kind): that one buffer NULL
    ("null"), one element short ("short") or declared with another dtype ("dtype")."""
    state, spawns, out = ext
    st, sp, o = nat.SmxState(), nat.SmxSpawns(), nat.SmxOutputs()

    def one(name, extent, fake):
        count, dtype = extent
        ptr = fake if name in given else None
        if change and change[0] == name:
            ptr = None if change[1] == "null" else fake
            count = max(count - 1, 0) if change[1] == "short" else count
            dtype = dtype % 7 + 1 if change[1] == "dtype" else dtype
        return (ptr, count, dtype) if ptr else (None, 0, nat.DT_NONE)

    for k, name in enumerate(nat.STATE_BUFFERS):
        ptr, st.count[k], st.dtype[k] = one(name, state[name], 0x1000 + 16 * k)
        setattr(st, name, ptr)
    for k, name in enumerate(nat.OUTPUT_BUFFERS):
        ptr, o.count[k], o.dtype[k] = one(name, out[name], 0x3000 + 16 * k)
        setattr(o, name, ptr)
    sp.episodes = episodes
    sp.pose, sp.pose_count, _ = one("pose", spawns["pose"], 0x2000)
    sp.social, sp.social_count, _ = one("social", spawns["social"], 0x2100)
    return st, sp, o


def _buffers(lib, c, has_vias, st, sp, o):
    err = C.create_string_buffer(512)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    rc = lib.smx_check_buffers(ref(c), has_vias, ref(st), ref(sp), ref(o), err, len(err))
    return rc, err.value.decode()


def sweep_buffers(lib, nat):
    for label, c, ext, given in configurations(nat):
        for has_vias in (0, 1):
            tag = f"buffers/{label}/vias{has_vias}"
            yield (tag + "/exact",) + _buffers(lib, c, has_vias, *structs(nat, ext, given))
            for name in nat.STATE_BUFFERS + ["pose", "social"] + nat.OUTPUT_BUFFERS:
                for kind in ("null", "short", "dtype"):
                    if kind == "dtype" and name in ("pose", "social"):
                        continue  # (the spawn tables carry no dtype)
                    yield (f"{tag}/{name}/{kind}",) + _buffers(lib, c, has_vias, *structs(nat, ext, given, change=(name, kind)))
        yield (f"buffers/{label}/no_episodes",) + _buffers(lib, c, 0, *structs(nat, ext, given, episodes=0))
        for n in range(1, 5):  # one to four of the five final_* rows
            some = (given - set(FINALS)) | set(FINALS[:n])
            yield (f"buffers/{label}/finals{n}",) + _buffers(lib, c, 0, *structs(nat, ext, some))
        st, sp, o = structs(nat, ext, given)
        yield (f"buffers/{label}/null_config",) + _buffers(lib, None, 0, st, sp, o)
        yield (f"buffers/{label}/null_state",) + _buffers(lib, c, 0, None, sp, o)
        yield (f"buffers/{label}/null_spawns",) + _buffers(lib, c, 0, st, None, o)
        yield (f"buffers/{label}/null_outputs",) + _buffers(lib, c, 0, st, sp, None)
    # lane_ttc without the rows it reads: the one configuration error the entry check reports itself
    label, c, ext, given = configurations(nat)[0]
    c.sensors = ALL_SENSORS & ~nat.SENSOR_NEIGHBORS
    yield ("buffers/lane_ttc_without_neighbours",) + _buffers(lib, c, 0, *structs(nat, ext, given))
    c.sensors, c.wp_paths, c.wp_len = ALL_SENSORS, 19, 27
    yield ("buffers/lane_ttc_513_waypoints",) + _buffers(lib, c, 0, *structs(nat, extents(nat, c), given))


def sweep_frame_stack(lib, nat):
    err = C.create_string_buffer(512)
    for label, c, _, _ in configurations(nat):
        _, _, out = extents(nat, c)
        for frames in (0, 1, 2, 8, 9):
            c.frame_stack = frames
            for source in list(range(-1, len(nat.OUTPUT_BUFFERS) + 1)) + [nat.STACK_SOURCE_RGB]:
                if source == nat.STACK_SOURCE_RGB:
                    row = c.rgb_width * c.rgb_height * 3
                elif 0 <= source < len(nat.OUTPUT_BUFFERS):
                    count, dtype = out[nat.OUTPUT_BUFFERS[source]]
                    row = count // (E * N) * DT_SIZE[dtype]  # (what a per-agent row holds; the others are refused anyway)
                else:
                    row = 0
                need = E * N * frames * row
                for layout in (nat.STACK_FRAMES, nat.STACK_DSTACK):
                    for tag, nbytes in (("exact", need), ("short", max(need - 1, 0))):
                        rc = lib.smx_check_frame_stack(C.byref(c), source, layout, nbytes, err, len(err))
                        yield f"stack/{label}/k{frames}/src{source}/layout{layout}/{tag}", rc, err.value.decode()
    c = configurations(nat)[0][1]
    c.frame_stack = 4
    yield "stack/unknown_layout", lib.smx_check_frame_stack(C.byref(c), 0, 2, 1 << 20, err, len(err)), err.value.decode()
    c.num_envs = 0
    yield "stack/no_envs", lib.smx_check_frame_stack(C.byref(c), 0, 0, 1 << 20, err, len(err)), err.value.decode()
    yield "stack/null_config", lib.smx_check_frame_stack(None, 0, 0, 0, err, len(err)), err.value.decode()


def sweep_rgb_and_guard(lib, nat):
    err = C.create_string_buffer(512)
    need = E * N * 16 * 8 * 3
    cases = [("exact", {}, need), ("short", {}, need - 1), ("no_envs", dict(num_envs=0), need),
             ("no_vehicles", dict(num_vehicles=0), need), ("grid_not_16", dict(rgb_width=15, rgb_height=3), need),
             ("grid_zero", dict(rgb_width=0), need), ("grid_65536", dict(rgb_width=256, rgb_height=256), E * N * 65536 * 3),
             ("grid_65552", dict(rgb_width=4097, rgb_height=16), 1 << 40), ("resolution_zero", dict(rgb_resolution=0.0), need),
             ("resolution_nan", dict(rgb_resolution=float("nan")), need), ("bit_off", dict(sensors=0, rgb_width=0), 0)]
    for tag, over, count in cases:
        c = config(nat, **dict(dict(sensors=nat.SENSOR_RGB), **over))
        yield f"rgb/{tag}", lib.smx_check_rgb_output(C.byref(c), count, err, len(err)), err.value.decode()
    yield "rgb/null_config", lib.smx_check_rgb_output(None, 0, err, len(err)), err.value.decode()
    inf = float("inf")
    cases = [("exact", {}, E * N, 1000.0), ("short", {}, E * N - 1, 1000.0), ("no_envs", dict(num_envs=0), 16, 1000.0),
             ("no_vehicles", dict(num_vehicles=0), 16, 1000.0), ("margin_0", {}, E * N, 0.0), ("margin_max", {}, E * N, 1.0e6),
             ("margin_negative", {}, E * N, -1.0), ("margin_nan", {}, E * N, float("nan")), ("margin_inf", {}, E * N, inf),
             ("margin_large", {}, E * N, 1.0e6 + 1.0)]
    for tag, over, count, margin in cases:
        c = config(nat, **over)
        yield f"guard/{tag}", lib.smx_check_guard(C.byref(c), count, margin, err, len(err)), err.value.decode()
    yield "guard/null_config", lib.smx_check_guard(None, 0, 0.0, err, len(err)), err.value.decode()


def sweep_mission_goals(lib, nat):
    err = C.create_string_buffer(512)
    nan = float("nan")
    headings, dead = (C.c_double * 3)(0.1, 0.2, 0.3), (C.c_int32 * 3)(0, 1, 0)
    bad_headings = (C.c_double * 3)(0.1, nan, 0.3)
    P, LAP, TRAVERSE = nat.GOAL_POSITIONAL, nat.GOAL_LAP, nat.GOAL_TRAVERSE
    cases = [("positional", [(P, 0, 0.0)] * 4, 4, None, None, 0, 3), ("clear", [], 4, None, None, 0, 3),
             ("lap", [(LAP, 2, 50.0)] + [(P, 0, 0.0)] * 3, 4, None, None, 0, 3),
             ("lap_no_laps", [(P, 0, 0.0), (LAP, 0, 50.0)] + [(P, 0, 0.0)] * 2, 4, None, None, 0, 3),
             ("lap_length_nan", [(LAP, 1, nan)] + [(P, 0, 0.0)] * 3, 4, None, None, 0, 3),
             ("lap_length_negative", [(LAP, 1, -1.0)] + [(P, 0, 0.0)] * 3, 4, None, None, 0, 3),
             ("unknown_kind", [(P, 0, 0.0)] * 3 + [(7, 0, 0.0)], 4, None, None, 0, 3),
             ("slots_mismatch", [(P, 0, 0.0)] * 3, 4, None, None, 0, 3),
             ("traverse", [(TRAVERSE, 0, 0.0)] * 4, 4, headings, dead, 3, 3),
             ("traverse_no_tables", [(TRAVERSE, 0, 0.0)] * 4, 4, None, None, 0, 3),
             ("traverse_lane_count", [(TRAVERSE, 0, 0.0)] * 4, 4, headings, dead, 3, 5),
             ("traverse_heading_nan", [(TRAVERSE, 0, 0.0)] * 4, 4, bad_headings, dead, 3, 3)]
    for tag, goals, nv, head, dead_end, n_lanes, map_lanes in cases:
        table = (nat.SmxMissionGoal * max(len(goals), 1))(*[nat.SmxMissionGoal(*g) for g in goals])
        rc = lib.smx_check_mission_goals(table, len(goals), nv, head, dead_end, n_lanes, map_lanes, err, len(err))
        yield f"goals/{tag}", rc, err.value.decode()
    yield "goals/null_table", lib.smx_check_mission_goals(None, 4, 4, None, None, 0, 3, err, len(err)), err.value.decode()
    yield "goals/negative_slots", lib.smx_check_mission_goals(None, -1, 4, None, None, 0, 3, err, len(err)), err.value.decode()
    small = C.create_string_buffer(16)  # a short err buffer: the message is cut, the terminator kept
    yield "goals/short_err", lib.smx_check_mission_goals(None, 4, 4, None, None, 0, 3, small, len(small)), small.value.decode()
    c = config(nat)
    yield "guard/short_err", lib.smx_check_guard(C.byref(c), 0, 0.0, small, len(small)), small.value.decode()
    yield "guard/no_err", lib.smx_check_guard(C.byref(c), 0, 0.0, None, 0), ""


def sweep_create(lib, nat):
    """smx_create's validation.  A configuration that passes it goes on to hipSetDevice: SMX_OK with a device (the handle
    is destroyed again), SMX_ERR_HIP without one — both are recorded as (0, ""): "the validation let it through"."""
    S = nat
    wpnb = S.SENSOR_WAYPOINTS | S.SENSOR_NEIGHBORS
    ogm = dict(sensors=S.SENSOR_OGM, ogm_width=64, ogm_height=64, ogm_resolution=0.2)
    dagm = dict(sensors=S.SENSOR_DAGM, dagm_width=64, dagm_height=64, dagm_resolution=0.2)
    rgb = dict(sensors=S.SENSOR_RGB, rgb_width=64, rgb_height=64, rgb_resolution=0.2)
    rw = dict(sensors=S.SENSOR_ROAD_WAYPOINTS, rw_horizon=4, rw_lanes=2, rw_paths=2)
    ttc = dict(sensors=wpnb | S.SENSOR_LANE_TTC)
    nan = float("nan")
    cases = [
        # every refusal of test_c_abi_rejects_invalid_configs_before_touching_the_device
        dict(num_vehicles=65), dict(num_envs=0), dict(dt=0.0), dict(wp_len=34), dict(wp_lookahead=40), dict(wp_paths=65),
        dict(via_max=33), dict(num_social=4), dict(action_space=9), dict(social_model=7), dict(nb_max=200),
        dict(sensors=S.SENSOR_OGM, ogm_width=300, ogm_height=300, ogm_resolution=0.2),
        dict(sensors=S.SENSOR_OGM, ogm_width=64, ogm_height=64, ogm_resolution=0.0),
        dict(sensors=S.SENSOR_DAGM, dagm_width=10, dagm_height=10, dagm_resolution=1.0),
        dict(sensors=S.SENSOR_LIDAR, lidar_rays=0), dict(alive_lists=5),
        # each limit's last good and first bad value
        {}, dict(num_envs=1), dict(num_envs=-1), dict(num_vehicles=1), dict(num_vehicles=0), dict(num_vehicles=64),
        dict(dt=1e-300), dict(dt=-0.1), dict(dt=nan),
        dict(rw), dict(rw, rw_horizon=0), dict(rw, rw_horizon=1), dict(rw, rw_horizon=64), dict(rw, rw_horizon=65),
        dict(rw, rw_lanes=0), dict(rw, rw_lanes=1), dict(rw, rw_lanes=8), dict(rw, rw_lanes=9),
        dict(rw, rw_paths=0), dict(rw, rw_paths=1), dict(rw, rw_paths=64), dict(rw, rw_paths=65),
        dict(sensors=0, rw_horizon=0), dict(sensors=0, wp_paths=0, wp_len=0, wp_lookahead=0),
        dict(wp_lookahead=0), dict(wp_lookahead=1, wp_len=1), dict(wp_lookahead=34), dict(wp_lookahead=35),
        dict(wp_paths=0), dict(wp_paths=1), dict(wp_paths=64), dict(wp_len=0), dict(wp_len=1), dict(wp_len=33),
        dict(via_max=-1), dict(via_max=0), dict(via_max=32),
        dict(alive_lists=-1), dict(alive_lists=0), dict(alive_lists=4), dict(alive_min_ego=-1), dict(alive_min_ego=0),
        dict(alive_min_total=-1), dict(alive_min_total=0),
        dict(num_social=-1), dict(num_social=0), dict(num_social=3, social_speed_factor=0.0),
        dict(num_social=1, social_speed_factor=-0.5), dict(num_social=1, social_speed_factor=nan),
        dict(num_social=0, social_speed_factor=-0.5),
        dict(social_model=-1), dict(social_model=0), dict(social_model=1), dict(social_model=2),
        dict(action_space=-1), dict(action_space=0), dict(action_space=8),
        dict(ogm), dict(ogm, ogm_width=0), dict(ogm, ogm_height=0), dict(ogm, ogm_width=1, ogm_height=16),
        dict(ogm, ogm_width=1, ogm_height=15), dict(ogm, ogm_width=256, ogm_height=256), dict(ogm, ogm_width=4097, ogm_height=16),
        dict(ogm, ogm_resolution=nan), dict(ogm, ogm_resolution=-1.0), dict(sensors=0, ogm_width=0),
        dict(dagm), dict(dagm, dagm_width=0), dict(dagm, dagm_height=0), dict(dagm, dagm_width=1, dagm_height=16),
        dict(dagm, dagm_width=1, dagm_height=15), dict(dagm, dagm_width=256, dagm_height=256),
        dict(dagm, dagm_width=4097, dagm_height=16), dict(dagm, dagm_resolution=nan), dict(dagm, dagm_resolution=0.0),
        dict(sensors=S.SENSOR_LIDAR, lidar_rays=1), dict(sensors=S.SENSOR_LIDAR, lidar_rays=65536),
        dict(sensors=S.SENSOR_LIDAR, lidar_rays=65537), dict(sensors=0, lidar_rays=0),
        dict(nb_max=0), dict(nb_max=1), dict(nb_max=127), dict(nb_max=128), dict(sensors=S.SENSOR_WAYPOINTS, nb_max=0),
        dict(ttc), dict(sensors=S.SENSOR_WAYPOINTS | S.SENSOR_LANE_TTC), dict(sensors=S.SENSOR_NEIGHBORS | S.SENSOR_LANE_TTC),
        dict(ttc, wp_paths=16, wp_len=32), dict(ttc, wp_paths=19, wp_len=27),
        dict(rgb), dict(rgb, rgb_width=0), dict(rgb, rgb_height=0), dict(rgb, rgb_width=1, rgb_height=15),
        dict(rgb, rgb_width=256, rgb_height=256), dict(rgb, rgb_width=4097, rgb_height=16), dict(rgb, rgb_resolution=0.0),
        dict(frame_stack=-1), dict(frame_stack=0), dict(frame_stack=1), dict(frame_stack=2), dict(frame_stack=8),
        dict(frame_stack=9),
    ]
    for over in cases:
        c = nat.SmxConfig()
        c.num_envs, c.num_vehicles, c.dt = 2, 4, 0.1
        c.sensors = wpnb
        c.wp_lookahead, c.wp_paths, c.wp_len, c.nb_max, c.nb_radius = 32, 4, 20, 10, 50.0
        for k, v in over.items():
            setattr(c, k, v)
        h = C.c_void_p(0xDEAD)
        rc = lib.smx_create(C.byref(c), 0, C.byref(h))
        msg = lib.smx_last_error(None).decode() if rc != 0 else ""
        if rc == 0:
            lib.smx_destroy(h)
        elif rc == -2:  # SMX_ERR_HIP: validated, no device here
            assert not h.value
            rc, msg = 0, ""
        label = "create/" + (",".join(f"{k}={v}" for k, v in over.items()) or "base")
        yield label, rc, msg
    h = C.c_void_p(0xDEAD)
    yield "create/null_config", lib.smx_create(None, 0, C.byref(h)), lib.smx_last_error(None).decode()


def sweep(lib):
    nat = _nat()
    for part in (sweep_buffers, sweep_frame_stack, sweep_rgb_and_guard, sweep_mission_goals, sweep_create):
        yield from part(lib, nat)


def main():
    lib = _nat().load_library()
    messages, cases = {}, []
    for _, rc, msg in sweep(lib):
        cases.append([rc, messages.setdefault(msg, len(messages))])
    with open(FIXTURE, "w") as f:
        json.dump({"messages": list(messages), "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {len(messages)} distinct messages, {os.path.getsize(FIXTURE)} bytes -> {FIXTURE}")


if __name__ == "__main__":
    main()

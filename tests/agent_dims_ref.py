"""Per-agent vehicle dimensions for the oracle and the tests (tests/test_agent_dims_cpu.py, tests/test_gpu_agent_dims.py):
the scene, the oracle's agent bodies with a box each, and an observe-only oracle tick for kinematic agents.

``oracle/`` already reads ``body.length / .width / .height`` in its collision test, its corners, its lane lookups, its
``off_route`` radius and its box rows; what it lacks is the kinematic chassis.  So the device moves the agents (an
Imitation sim) and the oracle observes: ``observe_tick`` copies the device's poses onto the oracle's bodies and runs the
part of ``OracleEnv.step`` that follows the physics — collisions, sensors, events — over them.

The scene, on ``loop`` and ``4lane``: E = 4 envs of 3 agents and 2 replayed slots.  Agent 0 is a 10 x 2.5 x 4 trailer,
agent 1 a 2.5 x 1 x 1.4 motorcycle, agent 2 a sedan — in envs 0 and 1; envs 2 and 3 repeat their poses with every agent a
sedan.  Every agent drives straight on at the speed of its spawn row (the Imitation action 0, 0).
 - envs 0 / 2: agent 0 starts on a lane, OFFSET m to the side of its centre line: a trailer corner is off the road, the
   sedan's four are on it (premise b).  STANDING (a replayed vehicle, the sedan's box) stands parallel to agent 0's line,
   SIDE m beside it and AHEAD m ahead: the trailer's box hits it in passing, the sedan's clears it (premise a).  FAR (the
   other replayed vehicle) stands between 3.68 m and 10 m from the nearest lane: the trailer reports that lane for it, a
   sedan none (premise d).
 - envs 1 / 3: agent 0 stands OFF_ROUTE m from the nearest lane, between the sedan's off_route radius (6.98 m) and the
   trailer's (10.15 m) — and beyond the 10 m the road-facts search reaches without dimensions (premise c)."""
import math

import numpy as np

import traffic_history_dims_ref as sized_ref
import traffic_history_ref as base
from oracle.dynamics import CHASSIS_HEIGHT, CHASSIS_LENGTH, CHASSIS_WIDTH, VehicleBody
from oracle.sim import COLLISION_LEEWAY, boxes_within
from smarts_amd.traffic_history import TrafficHistoryTable

SEDAN = (CHASSIS_LENGTH, CHASSIS_WIDTH, CHASSIS_HEIGHT)
TRAILER = (10.0, 2.5, 4.0)
MOTORCYCLE = (2.5, 1.0, 1.4)
E, AGENTS, SLOTS, DT, FRAMES = 4, 3, 2, 0.1, 40
N = AGENTS + SLOTS
STANDING, FAR = 5, 9  # the history's vehicle ids
VEHICLE_ROWS = [(STANDING, 2, CHASSIS_LENGTH, CHASSIS_WIDTH, CHASSIS_HEIGHT), (FAR, 2, CHASSIS_LENGTH, CHASSIS_WIDTH, CHASSIS_HEIGHT)]
SIDE, AHEAD = 1.9, 9.5  # the standing vehicle's centre from agent 0's spawn: across and along its heading
SPEED = 5.0
OFF_ROUTE = 10.07       # metres from the nearest lane: sedan radius 6.98 < 10 < OFF_ROUTE < trailer radius 10.15
SEDAN_RADIUS = 0.5 * math.hypot(CHASSIS_LENGTH, CHASSIS_WIDTH) + 5.0
TRAILER_RADIUS = 0.5 * math.hypot(TRAILER[0], TRAILER[1]) + 5.0
beside, ahead, sized = sized_ref.beside, sized_ref.ahead, sized_ref.sized


def dims_table():
    """float64 (1, E, A, 3): envs 0 and 1 trailer, motorcycle, NaN (the sedan's box); envs 2 and 3 all NaN."""
    d = np.full((1, E, AGENTS, 3), np.nan)
    d[0, :2, 0] = TRAILER
    d[0, :2, 1] = MOTORCYCLE
    return d


def box_of(dims, e, i, episode=0):
    """The box agent ``i`` of env ``e`` has under the table ``dims`` (None: nothing bound)."""
    if dims is None:
        return SEDAN
    t = dims[episode % dims.shape[0], e, i]
    return SEDAN if np.isnan(t[0]) else tuple(float(v) for v in t)


def body_at(pose, box=SEDAN, speed=0.0):
    return sized(VehicleBody(pose[0], pose[1], pose[2], speed), box)


def corners_on_road(road_map, body):
    return [bool(road_map.road_with_point((c[0], c[1], 0))) for c in body.bounding_box]


def _lane_dist_between(road_map, p, lo, hi):
    """The nearest lane of point ``p`` lies farther than ``lo`` and nearer than ``hi``."""
    q = np.array([p[0], p[1], 0.0])
    return road_map.nearest_lane(q, radius=lo) is None and road_map.nearest_lane(q, radius=hi) is not None


def scene(cm, road_map):
    """dict(table, spawns [1, E * N, 4], social_spawns [1, E * N, 2], dims, starts, lane, offset, side, far_pose,
    standing_pose, off_route_pose); ``ValueError`` names the premise the map cannot give."""
    lanes = sorted((i for i in range(cm.n_lanes) if not cm.lane_in_junction[i]), key=lambda i: -float(cm.lane_length[i]))
    found = None
    for a in lanes:  # premise (b): a lane, a place on it and a lateral offset
        for at in (5.0, 15.0, 30.0):
            if at + 60.0 > float(cm.lane_length[a]):
                continue
            for off in (0.5, -0.5, 0.7, -0.7, 0.3, -0.3, 0.9, -0.9):
                pose = beside(base.lane_pose(cm, a, at), off)
                if all(corners_on_road(road_map, body_at(pose, SEDAN))) and not all(corners_on_road(road_map, body_at(pose, TRAILER))):
                    found = (a, at, off, pose)
                    break
            if found:
                break
        if found:
            break
    if not found:
        raise ValueError("premise (b): no lane where an offset puts a trailer corner off the road and keeps the sedan's on it")
    a, at, off, spawn0 = found
    standing_pose = beside(ahead(spawn0, AHEAD), (-1.0 if off > 0 else 1.0) * SIDE)
    # premise (d): FAR beside the road, between a sedan's length and the trailer's from the nearest lane
    far_pose = side = None
    for t in np.arange(4.5, 9.0, 0.25):
        for sg in (1.0, -1.0):
            p = beside(ahead(spawn0, -2.0), sg * float(t))
            if far_pose is None and _lane_dist_between(road_map, p, CHASSIS_LENGTH + 0.3, TRAILER[0] - 0.3):
                far_pose, side = p, sg  # (the road's edge is on this side of the lane)
    if far_pose is None:
        raise ValueError("premise (d): no place beside the lane between 3.68 m and 10 m from every lane")
    # premise (c): agent 0 of envs 1 / 3, OFF_ROUTE m from the nearest lane
    off_route_pose = None
    for t in np.arange(9.0, 16.0, 0.01):
        p = beside(base.lane_pose(cm, a, at + 30.0), side * float(t))
        if _lane_dist_between(road_map, p, OFF_ROUTE - 0.03, OFF_ROUTE + 0.03):
            off_route_pose = p
            break
    if off_route_pose is None:
        raise ValueError("premise (c): no place 10.07 m from the nearest lane")
    b = next(i for i in lanes if cm.lane_road[i] != cm.lane_road[a])
    t_ = lambda k: round(k * DT, 6)  # noqa: E731
    traj = [(STANDING, t_(k), *standing_pose, 0.0) for k in range(FRAMES)] + [(FAR, t_(k), *far_pose, 0.0) for k in range(FRAMES)]
    table = TrafficHistoryTable.from_rows(VEHICLE_ROWS, traj, DT, SLOTS)
    spawns = np.zeros((1, E * N, 4))
    social = np.zeros((1, E * N, 2))
    social[..., 0] = a
    for e in range(E):
        rows = spawns[0, e * N:(e + 1) * N]
        rows[0] = (spawn0 + (SPEED,)) if e % 2 == 0 else (off_route_pose + (0.0,))
        rows[1] = base.lane_pose(cm, b, 25.0) + (SPEED,)
        rows[2] = base.lane_pose(cm, a, at + 40.0) + (SPEED,)
        rows[AGENTS:] = rows[2]  # (never read while the history is bound)
    return dict(table=table, spawns=spawns, social_spawns=social, dims=dims_table(), starts=np.zeros((1, E), dtype=np.int32),
                lane=a, offset=off, side=side, far_pose=far_pose, standing_pose=standing_pose, off_route_pose=off_route_pose,
                spawn0=spawn0)


def slot_of(table, vid):
    return sized_ref.slot_of(table, vid)


# ---------------------------------------------------------------------------------------------------------------------
def install(ob, sc, dims):
    """The scene's history into ``ob`` (a ``parity.OracleBatch``), and the box ``dims`` gives every agent (None: sedans),
    with what ``_Agent.__init__`` derived from the box redone: the trip meter's first waypoint (sensors.py:885-898)."""
    base.install(ob, sc["table"], sc["starts"][0])
    for e, env in enumerate(ob.envs):
        for i, ag in enumerate(env.agents):
            sized(ag.body, box_of(dims, e, i))
            ag.wps_for_distance = []
            wps = ob.road_map.waypoint_paths(ag.body.position, ag.body.heading, lookahead=1, within_radius=ag.body.length)
            if wps:
                ag.wps_for_distance.append(wps[0][0])


def copy_poses(ob, sim):
    """The device's pose and speed words onto the oracle's agent bodies (a kinematic agent: no lateral speed, no yaw rate)."""
    import torch

    from smarts_amd import _native as nat

    torch.cuda.synchronize()
    st = sim.state.cpu().numpy().reshape(nat.S_COUNT, -1)
    S = nat.S
    for e, env in enumerate(ob.envs):
        for i, ag in enumerate(env.agents):
            g = e * ob.N + i
            b = ag.body
            b.x, b.y, b.heading, b.u = st[S["X"], g], st[S["Y"], g], st[S["HEADING"], g], st[S["U"], g]
            b.v = b.yaw_rate_z = b.delta = 0.0


def observe_only(env):
    """``OracleEnv.step`` from its collision test on (smarts.py:1270-1291, 287-314), for bodies something else has moved:
    the clock, the replayed slots' frame, collisions, sensors and events, teardown."""
    env.elapsed_sim_time = round(env.elapsed_sim_time + env.dt, env._round)
    for sv in env.social:
        sv.body.step(env.dt)
    everyone = env._vehicles()
    for i, ag in enumerate(env.agents):
        ag.collisions = []
        if ag.alive:
            ag.collisions = [j for j, other in everyone if j != i and boxes_within(ag.body, other, COLLISION_LEEWAY)]
    obs, rewards, dones = {}, {}, {}
    for i, ag in enumerate(env.agents):
        if not ag.alive:
            continue
        ag.steps += 1
        obs[i], dones[i] = env._observe(i, ag, everyone)
        rewards[i] = ag.dist_travelled - ag.last_dist_travelled
    for i, d in dones.items():
        if d:
            env.agents[i].alive = False
    env.step_count += 1
    return obs, rewards, dones


def observe_tick(ob, sim):
    """The oracle's dense rows of the tick the device has just run."""
    import parity

    copy_poses(ob, sim)
    parts = []
    for env in ob.envs:
        obs, rew, dones = observe_only(env)
        parts.append(parity.pack(ob.cfg, ob.lane_no, ob.N, obs, rew, dones))
    return ob._stack(parts)


def kinematic_columns(dev, ora):
    """``ora`` with the ego columns a kinematic chassis defines its own way — steering None, the yaw rate and the velocity
    vectors of ``BoxChassis`` (chassis.py:275-308), which the oracle's dynamic body does not model — taken from ``dev``:
    heading, speed and the box words stay the oracle's."""
    from smarts_amd import _native as nat

    G = nat.EGO
    keep = np.zeros(nat.EGO_F32_COUNT, dtype=bool)
    keep[G["HEADING"]] = keep[G["SPEED"]] = True
    keep[G["BOX"]:G["BOX"] + 3] = True
    out = dict(ora)
    out["ego_f32"] = np.where(keep[None, :], ora["ego_f32"], np.where(np.isnan(dev["ego_f32"]), 0, dev["ego_f32"]))
    return out

"""Lap and traverse goals, endless missions with a chosen start — on the device, in the small launch form and both
forced cuts of the large one:

* the reference-generated rows of tests/golden/mission_goals_lap.npz / mission_goals_traverse.npz placed into the
  caller-owned state rows: first observation (the reset pass) and one tick, ``events[REACHED_GOAL]`` and ``done``;
* closed loops: laps on ``loop``, driving off a dead-end edge of ``4lane``, ``HiWayEnv`` with an ``EndlessMission``,
  and every goal kind in one env.
"""
import os

import numpy as np
import pytest

import mission_goals_ref as ref
from conftest import GOLDEN
from test_gpu_golden import _host, _sim_at_poses

pytestmark = pytest.mark.gpu

STRATEGIES = ["small", "large_teams", "large_one_lane"]


def _expected_done(ev, nat):
    """sensors.py:465-476 with SimConfig's default done criteria (collision, off_road, off_route)."""
    return (ev[:, nat.EV_REACHED_GOAL] | ev[:, nat.EV_COLLISIONS] | ev[:, nat.EV_OFF_ROAD] | ev[:, nat.EV_OFF_ROUTE] |
            ev[:, nat.EV_REACHED_MAX_EPISODE_STEPS] | ev[:, nat.EV_AGENTS_ALIVE_DONE]).astype(bool)


def _lap_cases(nets):
    from smarts_amd.missions import LapMission, Route, plan_mission

    g = np.load(os.path.join(GOLDEN, "mission_goals_plan.npz"))
    off = lambda t: t if t in ("base", "max") else float(t)  # noqa: E731
    out = []
    for spec, row in zip(g["lap_spec"][:5], g["lap_rows"][:5]):
        s = [str(x) for x in spec]
        out.append(plan_mission(nets("loop"), LapMission(Route((s[0], int(s[1]), off(s[2])), (s[3], int(s[4]), off(s[5]))),
                                                         num_laps=int(row[7]))))
    return out


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_lap_goal_rows_equal_the_reference(strategy, nets, compiled_maps):
    import torch

    from smarts_amd import _native as nat

    cm = compiled_maps("loop")
    g = np.load(os.path.join(GOLDEN, "mission_goals_lap.npz"))
    rows, want = g["rows"], g["is_complete"].astype(bool)
    seen = 0
    for p in _lap_cases(nets):
        sel = np.flatnonzero((rows[:, 5] == p.goal[0]) & (rows[:, 6] == p.goal[1]) & (rows[:, 3] == p.num_laps) &
                             (rows[:, 4] == p.route_length))
        assert len(sel) > 100
        poses = np.concatenate([rows[sel, :2], np.zeros((len(sel), 1))], axis=1)
        sim = _sim_at_poses(cm, poses, launch_strategy=strategy)
        sim.set_missions([p])
        out = sim.reset()
        ev = _host(out["events"])[:, 0]
        # first observation: the trip meter reads 0, no lap is complete (and a reset observation never ends an agent)
        assert not ev[:, nat.EV_REACHED_GOAL].any() and not _host(out["done"]).any()
        sim.state[nat.S["DIST"], :, 0] = torch.from_numpy(rows[sel, 2]).to(sim.state.device)
        out = sim.step(torch.full((len(sel), 1), -1, dtype=torch.int8, device="cuda"))
        ev, done, active = _host(out["events"])[:, 0], _host(out["done"])[:, 0], _host(out["active"])[:, 0]
        assert np.array_equal(_host(out["dist"])[:, 0], rows[sel, 2])  # standing still: the total is the one placed
        assert np.array_equal(_host(out["ego_pos"])[:, 0, :2], rows[sel, :2])
        bad = np.flatnonzero(ev[:, nat.EV_REACHED_GOAL].astype(bool) != want[sel])
        assert len(bad) == 0, (strategy, sel[bad][:10])
        assert np.array_equal(done.astype(bool), _expected_done(ev, nat)) and np.array_equal(active, 1 - done)
        assert np.array_equal(_host(sim.flags)[:, 0] & nat.F_ALIVE != 0, done == 0)
        sim.close()
        seen += len(sel)
    assert seen == len(rows)


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("name", ["4lane", "minicity"])
def test_traverse_goal_rows_equal_the_reference(name, strategy, compiled_maps):
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.missions import GOAL_TRAVERSE, PlannedMission

    cm = compiled_maps(name)
    g = np.load(os.path.join(GOLDEN, "mission_goals_traverse.npz"))
    poses, want = g[f"{name}_poses"], g[f"{name}_reached"].astype(bool)
    sim = _sim_at_poses(cm, poses, launch_strategy=strategy)
    sim.set_missions([PlannedMission((0.0, 0.0), 0.0, (0.0, 0.0, 0.0), (), GOAL_TRAVERSE)])
    out = sim.reset()  # the first observation (reset pass)
    ev = _host(out["events"])[:, 0]
    bad = np.flatnonzero(ev[:, nat.EV_REACHED_GOAL].astype(bool) != want)
    assert len(bad) == 0, ("reset", bad[:10])
    assert not _host(out["done"]).any()
    out = sim.step(torch.full((len(poses), 1), -1, dtype=torch.int8, device="cuda"))
    ev, done = _host(out["events"])[:, 0], _host(out["done"])[:, 0]
    assert np.array_equal(_host(out["ego_pos"])[:, 0, :2], poses[:, :2])
    bad = np.flatnonzero(ev[:, nat.EV_REACHED_GOAL].astype(bool) != want)
    assert len(bad) == 0, ("step", bad[:10])
    assert np.array_equal(done.astype(bool), _expected_done(ev, nat)) and done[want].all()
    sim.close()


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_laps_on_the_loop(strategy, nets, compiled_maps):
    """Two lap missions in one env, keep_lane until done: every tick ``reached_goal`` is the rule — inside the goal
    radius and the trip meter past route_length x num_laps —, each agent passes its goal without the event before
    the pass that ends it, and nobody is off route on the way round."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig
    from smarts_amd.missions import LapMission, Route, plan_mission

    cm, net = compiled_maps("loop"), nets("loop")
    missions = [plan_mission(net, LapMission(Route(("445633931", 0, 10), ("445633932", 0, 30)), num_laps=1)),
                plan_mission(net, LapMission(Route(("445633931", 1, 10), ("445633932", 1, 30)), num_laps=2))]
    spawns = np.zeros((1, 2, 4))
    for i, m in enumerate(missions):
        spawns[0, i] = (*m.spawn_pose(), 10.0)
    sim = BatchedSim(cm, SimConfig(num_envs=1, num_vehicles=2, launch_strategy=strategy), spawns=spawns, missions=missions)
    sim.reset()
    acts = torch.zeros((1, 2), dtype=torch.int8, device="cuda")
    alive, inside_before, passes, finished = [True, True], [False, False], [0, 0], [None, None]
    for t in range(4000):
        out = sim.step(acts)
        ev, done = _host(out["events"])[0], _host(out["done"])[0]
        pos, dist = _host(out["ego_pos"])[0], _host(out["dist"])[0]
        for i, m in enumerate(missions):
            if not alive[i]:
                continue
            inside = (pos[i, 0] - m.goal[0]) ** 2 + (pos[i, 1] - m.goal[1]) ** 2 <= m.goal[2] ** 2
            rule = ref.lap_is_complete(pos[i, 0], pos[i, 1], dist[i], m.num_laps, m.route_length, m.goal)
            assert bool(ev[i, nat.EV_REACHED_GOAL]) == rule, (t, i, dist[i])
            assert not ev[i, nat.EV_OFF_ROUTE] and not ev[i, nat.EV_OFF_ROAD] and not ev[i, nat.EV_COLLISIONS], (t, i, ev[i])
            assert bool(done[i]) == rule
            if inside and not inside_before[i] and not rule:
                passes[i] += 1  # through the goal without the event
            inside_before[i] = inside
            if done[i]:
                alive[i], finished[i] = False, (t, float(dist[i]))
        if not any(alive):
            break
    sim.close()
    assert finished[0] is not None and finished[1] is not None, (finished, passes)
    assert finished[0][1] > missions[0].route_length and finished[1][1] > 2 * missions[1].route_length
    assert passes[0] >= 1 and passes[1] == passes[0] + 1, passes  # one more lap, one more pass
    assert finished[1][0] > finished[0][0]


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_traverse_mission_drives_off_a_dead_end_with_every_kind_beside_it(strategy, nets, compiled_maps):
    """4lane, one env holding all four kinds (one wavefront, every branch): a traverse agent near the end of the
    dead-end edge east, a positional mission, a lap mission and an agent without a mission.  The traverse agent ends
    with reached_goal on the tick tests/mission_goals_ref.py says it has driven off the map — off_road with it."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig
    from smarts_amd.missions import LapMission, Mission, Route, TraverseMission, lane_end_tables, plan_mission

    cm, net = compiled_maps("4lane"), nets("4lane")
    length = net.getEdge("edge-east-WE").getLane(0).getLength()
    missions = [plan_mission(net, TraverseMission(("edge-east-WE", 0, length - 25.0))),
                plan_mission(net, Mission(Route(("edge-west-WE", 1, 40), ("edge-east-WE", 1, 25)))),
                plan_mission(net, LapMission(Route(("edge-south-SN", 1, 10), ("edge-north-SN", 1, 20)), num_laps=1)),
                None]
    spawns = np.zeros((1, 4, 4))
    for i, m in enumerate(missions[:3]):
        spawns[0, i] = (*m.spawn_pose(), 8.0)
    spawns[0, 3] = (*plan_mission(net, TraverseMission(("edge-north-NS", 0, 20))).spawn_pose(), 8.0)
    sim = BatchedSim(cm, SimConfig(num_envs=1, num_vehicles=4, launch_strategy=strategy), spawns=spawns, missions=missions)
    out = sim.reset()
    assert np.allclose(_host(out["ego_pos"])[0, 0, :2], missions[0].spawn_pose()[:2])
    tables = lane_end_tables(cm)
    acts = torch.zeros((1, 4), dtype=torch.int8, device="cuda")
    ended = None
    lap_inside_without_event = False
    for t in range(200):
        out = sim.step(acts)
        ev, done, pos = _host(out["events"])[0], _host(out["done"])[0], _host(out["ego_pos"])[0]
        heading = float(_host(sim.state)[nat.S["HEADING"], 0, 0])
        if ended is None:
            rule = ref.drove_off_map(net, cm, tables, pos[0, 0], pos[0, 1], heading)
            assert bool(ev[0, nat.EV_REACHED_GOAL]) == rule, (t, pos[0])
            if done[0]:
                ended = (t, ev[0].copy())
        m = missions[2]
        if (pos[2, 0] - m.goal[0]) ** 2 + (pos[2, 1] - m.goal[1]) ** 2 <= 4.0 and pos[2].any():
            assert not ev[2, nat.EV_REACHED_GOAL]  # a first pass is never past route_length
            lap_inside_without_event = True
        assert not ev[3, nat.EV_REACHED_GOAL]
    sim.close()
    assert ended is not None
    assert ended[1][nat.EV_REACHED_GOAL] and ended[1][nat.EV_OFF_ROAD] and not ended[1][nat.EV_OFF_ROUTE], ended
    assert lap_inside_without_event


def test_hiway_env_endless_mission_starts_at_its_begin():
    from smarts_amd.env import Agent, AgentInterface, AgentSpec, AgentType, HiWayEnv
    from smarts_amd.missions import EndlessMission

    spec = AgentSpec(interface=AgentInterface.from_type(AgentType.Laner, max_episode_steps=50),
                     agent_builder=lambda: Agent.from_function(lambda _: "keep_lane"))
    # the reference's own 4lane scenario gives its agents this mission
    env = HiWayEnv(scenarios=["scenarios/intersections/4lane"], agent_specs={"A": spec, "B": spec}, seed=3,
                   missions={"A": EndlessMission(begin=("edge-south-SN", 1, 10))})
    obs = env.reset()
    ego = obs["A"].ego_vehicle_state
    g = np.load(os.path.join(GOLDEN, "mission_goals_plan.npz"))
    sx, sy, sh = g["endless_4lane_rows"][0]
    # Pose.from_front_bumper: the centre half a chassis length behind the planned start, northbound (heading 0)
    assert np.allclose(ego.position[:2], (sx, sy - 1.84), atol=1e-9) and abs(float(ego.heading) - sh) < 1e-6
    assert ego.mission.goal == "EndlessGoal" and ego.mission.route_roads == ()
    for _ in range(5):
        obs, rew, done, info = env.step({a: "keep_lane" for a in obs})
        assert not obs["A"].events.reached_goal and not obs["A"].events.off_route
    env.close()


def test_lap_missions_through_parallel_env_auto_reset(nets):
    """ParallelEnv: a lap agent whose episode ends (here by max_episode_steps) starts the next one at the mission's
    start again."""
    from smarts_amd.env import Agent, AgentInterface, AgentSpec, AgentType, HiWayEnv, ParallelEnv
    from smarts_amd.missions import LapMission, Route, plan_mission

    lap = LapMission(Route(("445633931", 0, 10), ("445633932", 0, 30)), num_laps=1)
    spec = AgentSpec(interface=AgentInterface.from_type(AgentType.Laner, max_episode_steps=6),
                     agent_builder=lambda: Agent.from_function(lambda _: "keep_lane"))
    ctor = lambda: HiWayEnv(scenarios=["scenarios/loop"], agent_specs={"A": spec}, missions={"A": lap})  # noqa: E731
    env = ParallelEnv(env_constructors=[ctor, ctor], auto_reset=True, seed=1)
    start = np.array(plan_mission(nets("loop"), lap).spawn_pose()[:2])
    obs = env.reset()
    assert all(np.allclose(o["A"].ego_vehicle_state.position[:2], start, atol=1e-9) for o in obs)
    restarted = False
    for _ in range(8):
        obs, rew, done, info = env.step([{"A": "keep_lane"}] * 2)
        if done[0]["__all__"]:
            assert np.allclose(obs[0]["A"].ego_vehicle_state.position[:2], start, atol=1e-9)
            restarted = True
            break
    assert restarted
    env.close()

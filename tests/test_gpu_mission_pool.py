"""Mission pool on the device (smx_set_mission_pool, BatchedSim.set_mission_pool): missions per env and per episode.

* against the oracle, one OracleEnv per env with that env's missions and vias, teacher-forced, both launch forms;
* bit for bit against the uniform path: every env of a pool-bound batch equals a one-env batch with ``set_missions`` /
  vias of that env's missions, in every output row and in the state; a pool that gives every env slot a's old mission
  equals the per-slot batch;
* a restart inside the launch (``auto_reset``): the finishing tick under the old row, the new episode under the new one;
* lap and traverse goals from the pool; table entries outside -1 .. M - 1; the exclusion of the per-slot calls.
"""
import numpy as np
import pytest

import mission_pool_ref as mp
import parity

pytestmark = pytest.mark.gpu

STRATEGIES = ["small", "large_teams"]
STATE = ("state", "flags", "steps", "env_ticks", "env_done_count", "seed_cache", "facts_i32", "facts_f64")
PER_VEHICLE_3D = ("st_state", "st_seed_cache", "st_facts_i32", "st_facts_f64", "learner")  # [row][E][N]
SEED_FILTER_N, SEED_FILTER_ROAD0, ROUTE_FIXED = 1, 2, 3  # seed_cache rows (store_seeds), SMX_ROUTE_FIXED
FI_VIA_CONSUMED = 6  # SMX_FI_VIA_CONSUMED


def _snap(sim, out):
    """Every output row and every state buffer, on the host."""
    import torch

    torch.cuda.synchronize()
    d = {k: v.cpu().numpy() for k, v in out.items()}
    for name in STATE:
        d["st_" + name] = getattr(sim, name).cpu().numpy()
    return d


def _env(d, e):
    return {k: (a[:, e] if k in PER_VEHICLE_3D else a[e]) for k, a in d.items()}


def _differing(pool_env, twin_env, missions_of_slots, twin_has_vias=True, skip=()):
    """Keys whose bytes differ between one env of a pool-bound batch and its per-slot twin.  Two words are not the
    same by design and are checked for what they must hold instead:
      * seed_cache row 2 of a fixed-route filter is RouteFilter::road[0], the index of the route's table row — the pool
        index in the one batch, the slot in the other;
      * facts_i32 row SMX_FI_VIA_CONSUMED is written by the via sensor, which a twin without any via never runs."""
    bad = []
    for k, a in pool_env.items():
        if k in skip:
            continue
        b = twin_env[k]
        if k == "st_seed_cache":
            a, b = a.copy(), b.copy()
            fixed = a[SEED_FILTER_N] == ROUTE_FIXED
            if not np.array_equal(fixed, b[SEED_FILTER_N] == ROUTE_FIXED):
                bad.append(k + " (filter kind)")
                continue
            for slot in np.flatnonzero(fixed):
                if a[SEED_FILTER_ROAD0, slot] != missions_of_slots[slot] or b[SEED_FILTER_ROAD0, slot] != slot:
                    bad.append(f"{k} (road[0] of slot {slot}: {a[SEED_FILTER_ROAD0, slot]} / {b[SEED_FILTER_ROAD0, slot]})")
            a[SEED_FILTER_ROAD0, fixed] = b[SEED_FILTER_ROAD0, fixed] = 0
        if k == "st_facts_i32" and not twin_has_vias:
            a, b = a.copy(), b.copy()
            a[FI_VIA_CONSUMED] = b[FI_VIA_CONSUMED] = 0
        if a.shape != b.shape or a.dtype != b.dtype or np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes():
            bad.append(k)
    return bad


def _config(strategy, E, **kw):
    from smarts_amd.engine import SimConfig

    base = dict(num_envs=E, num_vehicles=mp.N, num_social=mp.SOCIAL, neighbors=True, nb_radius=50.0, via_max=4,
                launch_strategy=strategy)
    base.update(kw)
    return SimConfig(**base)


def _pool_sim(cm, cfg, spawns, where, missions, vias, table):
    import torch

    from smarts_amd.engine import BatchedSim

    sim = BatchedSim(cm, cfg, spawns=spawns, social_spawns=where)
    rows = torch.from_numpy(np.ascontiguousarray(table)).to(sim.device)
    sim.set_mission_pool(missions, vias, rows)
    return sim, rows


def _twin(cm, cfg, spawns, where, missions, vias, table, k, e, **kw):
    """The one-env batch with per-slot missions: env e of episode row k, its spawn rows as the only ones."""
    import dataclasses

    from smarts_amd.engine import BatchedSim

    n = cfg.num_vehicles
    ms, vs = mp.env_missions(missions, vias, table, k, e)
    has_vias = any(len(v) for v in vs)
    cfg1 = dataclasses.replace(cfg, num_envs=1, **kw)
    sim = BatchedSim(cm, cfg1, spawns=spawns[k:k + 1, e * n:(e + 1) * n], social_spawns=where[k:k + 1, e * n:(e + 1) * n],
                     vias=vs if has_vias else None, missions=ms)
    return sim, has_vias


@pytest.fixture(scope="module")
def scene(nets, compiled_maps):
    cm = compiled_maps("4lane")
    missions, vias = mp.pool_4lane(nets, cm)
    spawns, where = mp.spawn_rows(nets, cm, missions, mp.TABLE)
    return cm, missions, vias, spawns, where


def _actions(rng, t, E):
    acts = parity.lane_actions(rng, E, mp.N)
    acts[:, 1] = 0  # slot 1 keeps its lane: the agent of the single-road route reaches its goal inside the run
    return acts


# ---------------------------------------------------------------------------------------------------------------------
# 1. oracle parity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_pool_rollout_against_one_oracle_per_env(strategy, scene, nets):
    """E = 3, two agents and a social vehicle each, the pool of four, episode row 0 of a table of two rows: slot 1 is
    routed in envs 0 and 1 and endless in env 2; env 1's slot 0 holds a route it does not stand on and is off it from the
    first observation; env 2's slot 0 drives through its vias; env 1's slot 1 reaches its goal."""
    import torch

    from smarts_amd import _native as nat

    cm, missions, vias, spawns, where = scene
    T = 24
    cfg = _config(strategy, mp.E)
    sim, _rows = _pool_sim(cm, cfg, spawns, where, missions, vias, mp.TABLE)
    ob = mp.PoolOracle(nets("4lane"), cm, cfg, spawns[0], where[0], missions, vias, mp.TABLE[0])
    d, o = parity.host(sim.reset()), ob.reset_observe()
    # (the oracle's reset observation carries no reward — parity.pack leaves the row 0 — and the device's is the trip
    # meter's first step: 0 for every agent that starts on its route, which is compared, and the jump to the route's
    # first waypoint for the one misplaced agent, whose entry alone is taken out; the twin tests below pin that one
    # against the per-slot path, bit for bit)
    misplaced = 1 * mp.N + 0
    assert d["reward"][misplaced] > 0.0
    d["reward"][misplaced] = 0.0
    assert parity.compare(d, o, tol64=1e-9, tol32=2e-6, where="reset ") == []
    rng = np.random.default_rng(11)
    reached = off_route = via_hits = 0
    for t in range(T):
        acts = _actions(rng, t, mp.E)
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
        bad = parity.compare(d, o, tol64=1e-9, tol32=2e-6, where=f"t{t} ")
        assert bad == [], "\n".join(bad[:8])
        ev = d["events"].reshape(mp.E, mp.N, -1)
        reached += int(ev[:, :, nat.EV_REACHED_GOAL].sum())
        off_route += int(ev[:, :, nat.EV_OFF_ROUTE].sum())
        via_hits += int(sum(bin(int(x)).count("1") for x in d["via_hit"]))
        if t == 0:
            assert ev[1, 0, nat.EV_OFF_ROUTE] and d["done"].reshape(mp.E, mp.N)[1, 0]
        parity.sync_oracle_from_device(ob, sim)
    sim.sync()
    sim.close()
    # the comparison cannot have passed on idle rows
    assert reached >= 1 and off_route >= 1 and via_hits >= 1, (reached, off_route, via_hits)


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit for bit against the uniform path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_every_env_of_a_pool_equals_its_per_slot_twin(strategy, scene):
    import torch

    cm, missions, vias, spawns, where = scene
    cfg = _config(strategy, mp.E)
    sim, rows = _pool_sim(cm, cfg, spawns, where, missions, vias, mp.TABLE)
    twins = [_twin(cm, cfg, spawns, where, missions, vias, mp.TABLE, 0, e) for e in range(mp.E)]
    slot_missions = [list(mp.TABLE[0, e]) + [len(missions)] * mp.SOCIAL for e in range(mp.E)]
    p = _snap(sim, sim.reset())
    snaps = [_snap(tw, tw.reset()) for tw, _ in twins]
    rng = np.random.default_rng(3)
    for t in range(-1, 22):
        if t >= 0:
            acts = _actions(rng, t, mp.E)
            p = _snap(sim, sim.step(torch.from_numpy(acts).cuda()))
            snaps = [_snap(tw, tw.step(torch.from_numpy(acts[e:e + 1]).cuda())) for e, (tw, _) in enumerate(twins)]
        for e in range(mp.E):
            bad = _differing(_env(p, e), _env(snaps[e], 0), slot_missions[e], twins[e][1])
            assert bad == [], (t, e, bad)
    assert p["dist"].max() > 20.0
    sim.close()
    for tw, _ in twins:
        tw.close()


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_a_pool_of_the_slots_old_missions_equals_the_per_slot_batch(strategy, scene):
    """The table gives slot a of every env and every episode row the mission set_missions gave slot a."""
    import torch

    from smarts_amd.engine import BatchedSim

    cm, missions, vias, spawns, where = scene
    cfg = _config(strategy, mp.E)
    per_slot, per_slot_vias = [missions[2], missions[1], None], [vias[2], [], []]
    table = np.tile(np.array([2, 1], dtype=np.int32), (mp.ROWS, mp.E, 1))
    own = spawns.copy()
    for e in range(mp.E):
        for a, m in enumerate(per_slot[:mp.AGENTS]):
            own[:, e * mp.N + a] = (*m.spawn_pose(), mp.SPEED + e)
    a_sim, _rows = _pool_sim(cm, cfg, own, where, missions, vias, table)
    b_sim = BatchedSim(cm, cfg, spawns=own, social_spawns=where, vias=per_slot_vias, missions=per_slot)
    pa, pb = _snap(a_sim, a_sim.reset()), _snap(b_sim, b_sim.reset())
    rng = np.random.default_rng(4)
    for t in range(-1, 18):
        if t >= 0:
            acts = torch.from_numpy(parity.lane_actions(rng, mp.E, mp.N)).cuda()
            pa, pb = _snap(a_sim, a_sim.step(acts)), _snap(b_sim, b_sim.step(acts))
        for e in range(mp.E):
            bad = _differing(_env(pa, e), _env(pb, e), [2, 1, len(missions)])
            assert bad == [], (t, e, bad)
    a_sim.close(), b_sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. restart inside the launch
# ---------------------------------------------------------------------------------------------------------------------
def _restart_scene(name, nets, compiled_maps):
    """E = 2, one agent and one social vehicle an env, R = 2 and a different mission in every cell.  Env 0's first
    mission is a single-road route whose goal lies 30 m ahead: it ends at tick ~20, when env 1 is far from its goal."""
    from smarts_amd.engine import make_spawns
    from smarts_amd.missions import Mission, Route, plan_mission

    cm, net = compiled_maps(name), nets(name)
    if name == "4lane":
        specs = [Route(begin=("edge-east-EW", 1, 10), end=("edge-east-EW", 1, 40)),
                 Route(begin=("edge-north-NS", 0, 40), end=("edge-east-WE", 0, 30)),
                 Route(begin=("edge-west-WE", 1, 60), end=("edge-east-WE", 1, 12))]
    else:
        specs = [Route(("445633931", 0, 10), ("445633931", 0, 40)),
                 Route(("445633931", 1, 10), ("445633932", 1, 30)),
                 Route(("445633932", 0, 10), ("445633932", 0, 40))]
    missions = [plan_mission(net, Mission(r)) for r in specs]
    table = np.array([[[0], [1]], [[2], [0]]], dtype=np.int32)
    E, N = 2, 2
    spawns, where = make_spawns(cm, E, N, episodes=2, seed=5, return_lanes=True)
    for k in range(2):
        for e in range(E):
            spawns[k, e * N] = (*missions[table[k, e, 0]].spawn_pose(), mp.SPEED)
    return cm, missions, [[] for _ in missions], spawns, where, table


@pytest.mark.parametrize("name,lookahead", [("4lane", 32), ("loop", 16)])
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_restart_inside_the_launch_takes_the_next_row(strategy, name, lookahead, nets, compiled_maps):
    """The second case keeps the controller's knot lists across ticks (wp_lookahead >= 16, the loop's unbranched lanes):
    a list walked under the old mission is not taken for the new one."""
    import torch

    from smarts_amd import _native as nat

    cm, missions, vias, spawns, where, table = _restart_scene(name, nets, compiled_maps)
    E, N = 2, 2
    cfg = _config(strategy, E, num_vehicles=N, num_social=1, via_max=0, auto_reset=True, wp_lookahead=lookahead,
                  wp_len=min(20, lookahead))
    sim, rows = _pool_sim(cm, cfg, spawns, where, missions, None, table)
    # env 1 all along, and env 0's first episode: per-slot twins
    first, _ = _twin(cm, cfg, spawns, where, missions, vias, table, 0, 0, auto_reset=False)
    other, _ = _twin(cm, cfg, spawns, where, missions, vias, table, 0, 1, auto_reset=False)
    # what is excluded from a comparison, and why:
    #   final_* (every comparison): the twins run without auto_reset and have no such rows
    #   env_done, reward, done, learner (the first observation of the new episode only): under auto_reset the restart
    #     keeps the terminal step's reward / done / env_done — the learner block is their copy for the device-side
    #     gather —, where the fresh batch's reset wrote its own; from the next tick on they are compared again
    TWIN_SKIP = ("final_ego_pos", "final_ego_f32", "final_ego_lane", "final_events", "final_dist")
    FRESH_SKIP = TWIN_SKIP + ("env_done", "reward", "done", "learner")
    p = _snap(sim, sim.reset())
    f, o = _snap(first, first.reset()), _snap(other, other.reset())
    acts = torch.zeros((E, N), dtype=torch.int8, device="cuda")
    fresh, restarted_at = None, None
    for t in range(40):
        p = _snap(sim, sim.step(acts))
        o = _snap(other, other.step(acts[1:2]))
        bad = _differing(_env(p, 1), _env(o, 0), [table[0, 1, 0], len(missions)], False, skip=TWIN_SKIP)
        assert bad == [], ("env 1", t, bad)  # untouched by env 0's restart
        assert not p["env_done"][1]
        if fresh is not None:
            q = _snap(fresh, fresh.step(acts[0:1]))
            bad = _differing(_env(p, 0), _env(q, 0), [table[1, 0, 0], len(missions)], False, skip=TWIN_SKIP)
            assert bad == [], ("second episode", t, bad)
            continue
        f = _snap(first, first.step(acts[0:1]))
        if not p["env_done"][0]:
            bad = _differing(_env(p, 0), _env(f, 0), [table[0, 0, 0], len(missions)], False, skip=TWIN_SKIP)
            assert bad == [], ("first episode", t, bad)
            continue
        # the finishing tick: final_* carry the OLD mission's events — the goal of row 0's mission was reached —, equal to
        # what the twin, which does not restart, observed in this tick
        restarted_at = t
        assert p["final_events"][0, 0, nat.EV_REACHED_GOAL] == 1 and f["events"][0, 0, nat.EV_REACHED_GOAL] == 1
        for k in ("ego_pos", "ego_f32", "ego_lane", "events", "dist"):
            assert p["final_" + k][0].tobytes() == f[k][0].tobytes(), k
        # ... and the rows hold the first observation of the new episode: a fresh batch of row 1's mission and spawn row
        fresh, _ = _twin(cm, cfg, spawns, where, missions, vias, table, 1, 0, auto_reset=False)
        q = _snap(fresh, fresh.reset())
        bad = _differing(_env(p, 0), _env(q, 0), [table[1, 0, 0], len(missions)], False, skip=FRESH_SKIP)
        assert bad == [], ("first observation", t, bad)
        assert int(sim.env_episode[0]) == 1 and int(sim.env_episode[1]) == 0
    assert restarted_at is not None and 10 < restarted_at < 30 and t - restarted_at > 8, restarted_at
    sim.sync()
    for s in (sim, first, other, fresh):
        s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. lap and traverse goals from the pool
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["traverse", "lap"])
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_lap_and_traverse_goals_from_the_pool(strategy, kind, nets, compiled_maps):
    """The env of tests/test_gpu_mission_goals.py that holds every goal kind, from a pool (indices permuted) and from
    set_missions: bit for bit.  `traverse`: the traverse agent drives off the dead-end edge and ends with reached_goal.
    `lap`: the lap agent's trip meter is placed past its route length, so that its pass through the goal completes the
    lap."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig
    from smarts_amd.missions import LapMission, Mission, Route, TraverseMission, plan_mission

    cm, net = compiled_maps("4lane"), nets("4lane")
    length = net.getEdge("edge-east-WE").getLane(0).getLength()
    per_slot = [plan_mission(net, TraverseMission(("edge-east-WE", 0, length - 25.0))),
                plan_mission(net, Mission(Route(("edge-west-WE", 1, 40), ("edge-east-WE", 1, 25)))),
                plan_mission(net, LapMission(Route(("edge-south-SN", 1, 10), ("edge-north-SN", 1, 20)), num_laps=1)),
                None]
    spawns = np.zeros((1, 4, 4))
    for i, m in enumerate(per_slot[:3]):
        spawns[0, i] = (*m.spawn_pose(), 8.0)
    spawns[0, 3] = (*plan_mission(net, TraverseMission(("edge-north-NS", 0, 20))).spawn_pose(), 8.0)
    cfg = SimConfig(num_envs=1, num_vehicles=4, launch_strategy=strategy)
    a_sim = BatchedSim(cm, cfg, spawns=spawns)
    pool = [per_slot[2], per_slot[0], per_slot[1]]  # slot -> pool index: 1, 2, 0, -1
    table = torch.tensor([[[1, 2, 0, -1]]], dtype=torch.int32, device=a_sim.device)
    a_sim.set_mission_pool(pool, None, table)
    b_sim = BatchedSim(cm, cfg, spawns=spawns, missions=per_slot)
    pa, pb = _snap(a_sim, a_sim.reset()), _snap(b_sim, b_sim.reset())
    if kind == "lap":
        for s in (a_sim, b_sim):
            s.state[nat.S["DIST"], 0, 2] = per_slot[2].route_length + 1.0
    acts = torch.zeros((1, 4), dtype=torch.int8, device="cuda")
    reached = np.zeros(4, dtype=int)
    for t in range(-1, 220):
        if t >= 0:
            pa, pb = _snap(a_sim, a_sim.step(acts)), _snap(b_sim, b_sim.step(acts))
            reached += pa["events"][0, :, nat.EV_REACHED_GOAL]
        bad = _differing(_env(pa, 0), _env(pb, 0), [1, 2, 0, len(pool)], False)
        assert bad == [], (t, bad)
        if reached[0 if kind == "traverse" else 2]:
            break
    a_sim.close(), b_sim.close()
    assert reached[0 if kind == "traverse" else 2] == 1, reached


# ---------------------------------------------------------------------------------------------------------------------
# 5. bad table entries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_entries_outside_the_pool_read_as_endless_and_are_reported(strategy, scene):
    """An entry of M and an entry of -7 behave as -1, bit for bit, and the next sync reports them — once."""
    import torch

    from smarts_amd._native import SmxError

    cm, missions, vias, spawns, where = scene
    cfg = _config(strategy, mp.E)
    good = mp.TABLE.copy()
    good[0, 1, 0] = -1
    assert good[0, 2, 1] == -1
    bad = good.copy()
    bad[0, 1, 0], bad[0, 2, 1] = len(missions), -7
    a_sim, _a = _pool_sim(cm, cfg, spawns, where, missions, vias, bad)
    b_sim, _b = _pool_sim(cm, cfg, spawns, where, missions, vias, good)
    pa, pb = _snap(a_sim, a_sim.reset()), _snap(b_sim, b_sim.reset())
    with pytest.raises(SmxError, match="mission pool"):
        a_sim.sync()
    b_sim.sync()
    rng = np.random.default_rng(8)
    for t in range(6):
        acts = torch.from_numpy(parity.lane_actions(rng, mp.E, mp.N)).cuda()
        pa, pb = _snap(a_sim, a_sim.step(acts)), _snap(b_sim, b_sim.step(acts))
        for k in pa:
            assert pa[k].tobytes() == pb[k].tobytes(), (t, k)
    with pytest.raises(SmxError, match="-1 .. n_missions - 1"):
        a_sim.sync()
    _a[0, 1, 0], _a[0, 2, 1] = -1, -1  # mended in place: nothing more to report
    a_sim.step(acts)
    a_sim.sync()
    a_sim.close(), b_sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. exclusivity through BatchedSim
# ---------------------------------------------------------------------------------------------------------------------
def test_pool_excludes_the_per_slot_calls_and_unbinds(scene):
    import torch

    from smarts_amd._native import SmxError
    from smarts_amd.engine import BatchedSim

    cm, missions, vias, spawns, where = scene
    cfg = _config("small", mp.E)
    per_slot = [missions[0], missions[1], None]
    sim = BatchedSim(cm, cfg, spawns=spawns, social_spawns=where, missions=per_slot, vias=[vias[2], [], []])
    plain = BatchedSim(cm, cfg, spawns=spawns, social_spawns=where)
    rows = torch.from_numpy(mp.TABLE.copy()).to(sim.device)
    with pytest.raises(ValueError, match="rows"):
        sim.set_mission_pool(missions, vias, rows[:, :2].contiguous())
    with pytest.raises(ValueError, match="rows"):
        sim.set_mission_pool(missions, vias, rows.to(torch.int64))
    sim.set_mission_pool(missions, vias, rows)   # drops the per-slot missions and vias
    assert sim.missions is None and sim.vias is None
    with pytest.raises(SmxError, match="mission pool"):
        sim.set_missions(per_slot)
    with pytest.raises(SmxError, match="mission pool"):
        sim.set_missions(None)
    sim.set_mission_pool(None)                   # every mission endless again, no vias
    pa, pb = _snap(sim, sim.reset()), _snap(plain, plain.reset())
    acts = torch.zeros((mp.E, mp.N), dtype=torch.int8, device="cuda")
    for t in range(4):
        pa, pb = _snap(sim, sim.step(acts)), _snap(plain, plain.step(acts))
    for k in pb:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    sim.set_missions(per_slot)                   # ... and the per-slot call is taken again
    sim.close(), plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. env layer
# ---------------------------------------------------------------------------------------------------------------------
def test_parallel_env_flies_the_variations_in_turn(nets):
    """ParallelEnv, 3 envs, V = 2, shuffle off: every env sees variation 0, then — across an auto-reset — variation 1,
    with the start, the goal and the vias of its Observation to match; with an explicit schedule env 1 differs."""
    from smarts_amd.env import Agent, AgentInterface, AgentSpec, AgentType, HiWayEnv, ParallelEnv
    from smarts_amd.missions import Mission, Route, plan_mission
    from smarts_amd.vias import Via

    variations = [Mission(Route(begin=("edge-east-EW", 1, 10), end=("edge-east-EW", 1, 40))),
                  Mission(Route(begin=("edge-west-WE", 1, 60), end=("edge-east-WE", 1, 12)))]
    planned = [plan_mission(nets("4lane"), m) for m in variations]
    spec = AgentSpec(interface=AgentInterface.from_type(AgentType.Laner, max_episode_steps=8),
                     agent_builder=lambda: Agent.from_function(lambda _: "keep_lane"))

    # B has no mission and vias all over the map, so that one is near wherever its endless mission starts: they are
    # sensed in every variation, as they are without a list of variations
    far_vias = [Via(edge, 0, off, 8) for edge in ("edge-east-EW", "edge-west-WE", "edge-north-NS", "edge-south-SN",
                                                  "edge-east-WE", "edge-west-EW", "edge-north-SN", "edge-south-NS") for off in (10, 28, 46)]

    def make(schedule=None):
        ctor = lambda s: (lambda: HiWayEnv(scenarios=["scenarios/intersections/4lane"], agent_specs={"A": spec, "B": spec},  # noqa: E731
                                           shuffle_scenarios=False, missions={"A": variations}, mission_schedule=s,
                                           vias={"A": [Via("edge-east-EW", 1, 30, 8)], "B": far_vias}))
        return ParallelEnv(env_constructors=[ctor(None if schedule is None else schedule[e]) for e in range(3)], auto_reset=True, seed=1)

    def flies(ob, j):
        ego = ob["A"].ego_vehicle_state
        assert ego.mission.goal.position == tuple(planned[j].goal[:2]) and ego.mission.route_roads == tuple(planned[j].route_roads), j
        assert ob["B"].ego_vehicle_state.mission.goal == "EndlessGoal"
        assert len(ob["B"].via_data.near_via_points) >= 1   # the mission-less agent keeps its vias

    env = make()
    obs = env.reset()
    for e in range(3):
        flies(obs[e], 0)
        assert np.allclose(obs[e]["A"].ego_vehicle_state.position[:2], planned[0].spawn_pose()[:2], atol=1e-9)
        assert len(obs[e]["A"].via_data.near_via_points) == 1   # the via lies 20 m ahead on variation 0's road
    restarted = False
    for _ in range(10):
        obs, rew, done, info = env.step([{a: "keep_lane" for a in ("A", "B")}] * 3)
        if done[0]["__all__"]:
            for e in range(3):
                assert done[e]["__all__"]
                flies(obs[e], 1)     # the first observation of the next episode: variation 1
                assert np.allclose(obs[e]["A"].ego_vehicle_state.position[:2], planned[1].spawn_pose()[:2], atol=1e-9)
                assert len(obs[e]["A"].via_data.near_via_points) == 0   # ... whose start is far from the via
                final = info[e]["A"]["env_obs"].ego_vehicle_state.mission   # the finishing tick's observation: still variation 0
                assert final.goal.position == tuple(planned[0].goal[:2]) and final.route_roads == tuple(planned[0].route_roads)
            restarted = True
            break
        for e in range(3):
            flies(obs[e], 0)
    assert restarted
    env.close()
    env = make(schedule=[[0, 1], [1, 0], [0, 0]])
    obs = env.reset()
    flies(obs[0], 0), flies(obs[1], 1), flies(obs[2], 0)
    assert np.allclose(obs[1]["A"].ego_vehicle_state.position[:2], planned[1].spawn_pose()[:2], atol=1e-9)
    env.close()
    with pytest.raises(ValueError, match="one common length"):
        bad = HiWayEnv(scenarios=["scenarios/intersections/4lane"], agent_specs={"A": spec, "B": spec},
                       missions={"A": variations, "B": variations + variations})
        bad.reset()

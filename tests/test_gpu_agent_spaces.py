"""GPU: per-agent action spaces (include/smx.h smx_set_agent_spaces / smx_step_mixed) — one tick drives a mixed fleet.

Parity with the oracle, which reads the action space per agent (oracle/sim.py), teacher-forced as the uniform parity
tests are; equivalence of every space's slots with the uniform kernels of that space from identical state (which covers
MPC, which the oracle does not have); the tables of one space; a binding that switches the cut mid-episode; bind and
unbind; a restart inside the launch; the env layer."""
import ctypes
import dataclasses

import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

FLOATS = ("Continuous", "ActuatorDynamic", "LaneWithContinuousSpeed")
TRACKING = ("Trajectory", "MPC")
SIX = ("Lane", "Continuous", "LaneWithContinuousSpeed", "ActuatorDynamic", "Trajectory", "MPC")
_host = parity.host


def _fleet_actions(rng, t, spaces, d, E, N, none_at=None):
    """One tick's actions for a fleet whose agent slot i has ``spaces[i]`` (slots past len(spaces) are social): the four
    buffers of step_mixed over (E, N), every slot filled with an action of its own kind, and the same actions as the
    oracle takes them.  ``d``: the last observation's host rows (a tracking agent follows one of its waypoint paths,
    as test_trajectory_action_space has it).  ``none_at``: {space: slot} agents that send no action this tick."""
    from oracle import controller as octl
    from smarts_amd.engine import pack_trajectory

    none_at = none_at or {}
    lane = parity.lane_actions(rng, E, N)
    floats = np.full((E, N, 3), np.nan, dtype=np.float32)
    packed = np.zeros((E, N, 4, 11))
    counts = np.zeros((E, N), dtype=np.int32)
    oracle = [[None] * len(spaces) for _ in range(E)]
    P, W = d["wp_count"].shape[-1] - 1, d["wp_pos"].shape[-2]
    wp_pos, wp_h = d["wp_pos"].reshape(E, N, P, W, 3), d["wp_heading"].reshape(E, N, P, W)
    wp_c, act = d["wp_count"].reshape(E, N, P + 1), d["active"].reshape(E, N)
    for e in range(E):
        for i, space in enumerate(spaces):
            silent = none_at.get(space) == i and e == 0
            if space == "Lane":
                if silent:
                    lane[e, i] = -1
                oracle[e][i] = int(lane[e, i])
            elif space in FLOATS:
                if space == "LaneWithContinuousSpeed":
                    a = [rng.choice([0.0, 2.03, 2.045, 5.0, 9.5, 14.0, 18.0]), rng.choice([0.0, 0.0, 0.0, 1.0, -1.0]), 0.0]
                else:
                    a = [rng.uniform(-0.2, 1.2), rng.uniform(0, 1) if rng.random() < 0.2 else 0.0, rng.uniform(-1.3, 1.3) * 0.3]
                floats[e, i] = a
                if silent:
                    floats[e, i, 0] = np.nan
                oracle[e][i] = floats[e, i].astype(np.float64)
            else:
                oracle[e][i] = ([], [], [], [])
                if not act[e, i] or wp_c[e, i, 0] == 0 or silent:
                    continue  # gone, nothing to track, or a tick without an action (count 0)
                p = int(rng.integers(min(int(wp_c[e, i, 0]), P)))
                n = min(int(rng.choice([3, 7, 10, 11, 20])), int(wp_c[e, i, 1 + p]))
                v0 = float(rng.choice([0.0, 6.0, 11.0, 16.0, 22.0]))
                traj = (wp_pos[e, i, p, :n, 0].tolist(), wp_pos[e, i, p, :n, 1].tolist(), [float(x) for x in wp_h[e, i, p, :n]],
                        [v0 + 0.1 * k for k in range(n)])
                packed[e, i], counts[e, i] = pack_trajectory(traj)
                oracle[e][i] = octl.unpack_trajectory(packed[e, i], n)
    return lane, floats, packed, counts, oracle


def _step_mixed(sim, lane, floats, packed, counts):
    import torch

    return sim.step_mixed(torch.from_numpy(lane), torch.from_numpy(floats), torch.from_numpy(packed), torch.from_numpy(counts))


@pytest.mark.parametrize("strategy", ["small", "large_teams"])
@pytest.mark.parametrize("name,E,spaces,social,T,seed", [
    ("loop", 3, ("Lane", "Continuous", "LaneWithContinuousSpeed", "ActuatorDynamic", "Trajectory", "Lane"), 2, 25, 71),
    ("4lane", 2, ("Lane", "Continuous", "ActuatorDynamic", "LaneWithContinuousSpeed", "Trajectory"), 0, 15, 72)])
def test_mixed_fleet_matches_the_oracle(name, E, spaces, social, T, seed, strategy, nets, compiled_maps):
    """Teacher-forced, as test_float_action_spaces: every agent steps by its own controller from its own kind of action,
    each space's "no action" among them, and the scripted social slots move once a tick."""
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps(name)
    A, N = len(spaces), len(spaces) + social
    cfg = SimConfig(num_envs=E, num_vehicles=N, num_social=social, neighbors=True, nb_radius=50.0, launch_strategy=strategy)
    spawns, where = make_spawns(cm, E, N, episodes=2, seed=seed, return_lanes=True)
    sim = BatchedSim(cm, cfg, spawns=spawns, social_spawns=where if social else None)
    sim.set_agent_spaces(spaces)
    assert sim.launch_form() == strategy
    ob = parity.OracleBatch(nets(name), cm, cfg, spawns[0], where[0] if social else None)
    for env in ob.envs:
        for i, ag in enumerate(env.agents):
            ag.cfg = dataclasses.replace(ag.cfg, action_space=spaces[i])
    d, o = _host(sim.reset()), ob.reset_observe()
    assert parity.compare(d, o, tol64=1e-9, tol32=2e-6, where="reset ") == []
    rng = np.random.default_rng(seed)
    silent = set()
    for t in range(T):
        # every space's "no action" in turn: code -1, a NaN first float, count 0
        none_at = {spaces[i]: i for i in range(A) if t % 3 == 2 and i == (t // 3) % A}
        silent |= set(none_at)
        lane, floats, packed, counts, oracle_actions = _fleet_actions(rng, t, spaces, d, E, N, none_at)
        d = _host(_step_mixed(sim, lane, floats, packed, counts))
        parts = []
        for e, env in enumerate(ob.envs):
            obs, rew, dones = env.step(oracle_actions[e])
            parts.append(parity.pack(cfg, ob.lane_no, N, obs, rew, dones))
        bad = parity.compare(d, ob._stack(parts), tol64=1e-9, tol32=2e-5, where=f"mixed {name} {strategy} t{t} ")
        assert bad == [], "\n".join(bad[:8])
        # the social slots' poses: a social step taken once per launch would show here
        S = sim.state.cpu().numpy()
        for e, env in enumerate(ob.envs):
            for k, sv in enumerate(env.social):
                got = S[0:3, e, A + k]
                assert np.abs(got - [sv.body.x, sv.body.y, sv.body.heading]).max() < 1e-9, (t, e, k, got, sv.body.x, sv.body.y)
        parity.sync_oracle_from_device(ob, sim)
    assert silent == set(spaces)
    sim.sync()
    sim.close()


def _state_tensors(sim):
    from smarts_amd import _native as nat

    return [t for t in (getattr(sim, "state" if name == "f64" else name) for name in nat.STATE_BUFFERS) if t is not None]


def _equivalence(space, strategy, compiled_maps, T, seed, **cfg_kw):
    """A mixed sim that holds `space` and a uniform sim of `space` on the same spawns: before every tick the uniform sim
    takes the mixed sim's state, `space`'s agents get the same actions in both, and afterwards the state columns and flags
    of `space`'s slots are the same bits."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps("loop")
    E, N = 2, 6
    spaces = SIX[SIX.index(space):] + SIX[:SIX.index(space)]  # every space is there; `space` leads once, trails once, ...
    kw = dict(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, launch_strategy=strategy, done_collision=False)
    kw.update(cfg_kw)
    spawns = make_spawns(cm, E, N, episodes=2, seed=seed)
    mixed = BatchedSim(cm, SimConfig(**kw), spawns=spawns)
    mixed.set_agent_spaces(spaces)
    uniform = BatchedSim(cm, SimConfig(action_space=space, **kw), spawns=spawns)
    d = _host(mixed.reset())
    uniform.reset()
    mine = [i for i, s in enumerate(spaces) if s == space]
    rng = np.random.default_rng(seed)
    moved = 0.0
    for t in range(T):
        lane, floats, packed, counts, _ = _fleet_actions(rng, t, spaces, d, E, N, {space: mine[0]} if t == 2 else None)
        for dst, src in zip(_state_tensors(uniform), _state_tensors(mixed)):
            dst.copy_(src)
        before = mixed.state[0:2].clone()
        d = _host(_step_mixed(mixed, lane, floats, packed, counts))
        if space == "Lane":
            uniform.step(torch.from_numpy(lane))
        elif space in FLOATS:
            uniform.step(torch.from_numpy(floats))
        else:
            uniform.step_trajectory(torch.from_numpy(packed), torch.from_numpy(counts))
        torch.cuda.synchronize()
        assert torch.equal(mixed.state[:, :, mine], uniform.state[:, :, mine]), (space, strategy, t)
        assert torch.equal(mixed.flags[:, mine], uniform.flags[:, mine]), (space, strategy, t)
        assert torch.equal(mixed.steps[:, mine], uniform.steps[:, mine]) and torch.equal(mixed.env_episode, uniform.env_episode)
        moved += float((mixed.state[0:2] - before)[:, :, mine].abs().sum())
    assert moved > 1.0  # the slots drove
    episodes = int(mixed.env_episode.max())
    mixed.sync()
    mixed.close()
    uniform.close()
    return episodes


@pytest.mark.parametrize("strategy", ["small", "large_teams"])
@pytest.mark.parametrize("space", SIX)
def test_mixed_slots_equal_the_uniform_kernels(space, strategy, compiled_maps):
    _equivalence(space, strategy, compiled_maps, T=6, seed=81)


@pytest.mark.parametrize("space,strategy", [("Lane", "small"), ("ActuatorDynamic", "small"), ("MPC", "small"),
                                            ("LaneWithContinuousSpeed", "large_teams"), ("Trajectory", "large_teams")])
def test_slots_keep_their_spaces_across_a_restart_inside_the_launch(space, strategy, compiled_maps):
    """auto_reset: every env ends at max_episode_steps and restarts inside the launch, twice in 15 ticks; the equivalence
    with the uniform kernels holds through the restarts, so the new episode's slots have the spaces of the old one."""
    episodes = _equivalence(space, strategy, compiled_maps, T=15, seed=82, auto_reset=True, max_episode_steps=6)
    assert episodes >= 2  # (episode 0 is the reset's)


def _step_uniform(sim, space, lane, floats, packed, counts):
    import torch

    if space == "Lane":
        return sim.step(torch.from_numpy(lane))
    if space in FLOATS:
        return sim.step(torch.from_numpy(floats))
    return sim.step_trajectory(torch.from_numpy(packed), torch.from_numpy(counts))


def _same_bits(a, b, outs_a, outs_b, where):
    import torch

    torch.cuda.synchronize()
    assert torch.equal(a.state, b.state) and torch.equal(a.flags, b.flags) and torch.equal(a.steps, b.steps), where
    for k in ("ego_pos", "ego_f32", "wp_pos", "done", "events", "nb_slot"):
        assert torch.equal(outs_a[k], outs_b[k]), (where, k)


@pytest.mark.parametrize("strategy", ["small", "large_teams"])
@pytest.mark.parametrize("space", ["Lane", "Continuous"])
def test_a_table_of_one_space_is_the_uniform_sim(space, strategy, compiled_maps):
    """The two tables whose entries are all equal, in a Lane configuration: all Lane, which is cfg.action_space, so
    smx_step_mixed launches the uniform kernels; all Continuous, which is not, so it is a mixed tick of one launch.
    Either way the run is, bit for bit, that of a uniform sim of that space, the scripted social slots included."""
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps("loop")
    E, A, social = 2, 5, 2
    N = A + social
    kw = dict(num_envs=E, num_vehicles=N, num_social=social, neighbors=True, nb_radius=50.0, launch_strategy=strategy)
    spawns, where = make_spawns(cm, E, N, episodes=2, seed=83, return_lanes=True)
    tabled = BatchedSim(cm, SimConfig(**kw), spawns=spawns, social_spawns=where)
    tabled.set_agent_spaces([space] * A)
    uniform = BatchedSim(cm, SimConfig(action_space=space, **kw), spawns=spawns, social_spawns=where)
    assert tabled.launch_form() == uniform.launch_form() == strategy
    d = _host(tabled.reset())
    uniform.reset()
    rng = np.random.default_rng(83)
    start = tabled.state[0:2].clone()
    for t in range(6):
        lane, floats, packed, counts, _ = _fleet_actions(rng, t, [space] * A, d, E, N, {space: 1} if t == 2 else None)
        o1 = _step_mixed(tabled, lane, floats, packed, counts)
        o2 = _step_uniform(uniform, space, lane, floats, packed, counts)
        _same_bits(tabled, uniform, o1, o2, (space, strategy, t))
        d = _host(o1)
    assert float((tabled.state[0:2] - start).abs().sum()) > 1.0  # they drove
    tabled.sync()
    tabled.close()
    uniform.close()


def test_binding_mid_episode_switches_the_cut(compiled_maps):
    """A batch in the one-lane cut takes a table in the middle of an episode: the tick's form becomes the teams cut, so
    the slow lists stop and the alive list the one-lane tick carried is read by the team kernels; unbinding switches
    back.  A twin under launch_strategy "large_teams" takes the same bindings and the same actions and never changes its
    cut: the two runs are the same bits at every tick (as the strategies agree bit for bit without a table)."""
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps("loop")
    E, N = 4, 8
    spaces = ("Lane", "Continuous", "LaneWithContinuousSpeed", "Trajectory", "Lane", "ActuatorDynamic", "MPC", "Lane")
    kw = dict(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, done_collision=False)
    spawns = make_spawns(cm, E, N, episodes=2, seed=84)
    sim = BatchedSim(cm, SimConfig(launch_strategy="large_one_lane", **kw), spawns=spawns)
    twin = BatchedSim(cm, SimConfig(launch_strategy="large_teams", **kw), spawns=spawns)
    d = _host(sim.reset())
    twin.reset()
    rng = np.random.default_rng(84)
    t = 0
    for table, form, ticks in ((None, "large_one_lane", 4), (spaces, "large_teams", 5), (None, "large_one_lane", 4)):
        sim.set_agent_spaces(table)
        twin.set_agent_spaces(table)
        assert sim.launch_form() == form and twin.launch_form() == "large_teams"
        for _ in range(ticks):
            lane, floats, packed, counts, _ = _fleet_actions(rng, t, table or ("Lane",) * N, d, E, N)
            if table:
                o1, o2 = _step_mixed(sim, lane, floats, packed, counts), _step_mixed(twin, lane, floats, packed, counts)
            else:
                o1, o2 = (_step_uniform(s, "Lane", lane, floats, packed, counts) for s in (sim, twin))
            _same_bits(sim, twin, o1, o2, (form, t))
            d = _host(o1)
            t += 1
    sim.sync()
    sim.close()
    twin.close()


def test_bind_and_unbind(compiled_maps):
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps("loop")
    E, N = 2, 6
    spawns = make_spawns(cm, E, N, episodes=2, seed=91)
    cfg = SimConfig(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0)
    sim, plain = BatchedSim(cm, cfg, spawns=spawns), BatchedSim(cm, cfg, spawns=spawns)
    sim.reset()
    plain.reset()
    lane = torch.zeros((E, N), dtype=torch.int8, device=sim.device)
    floats = torch.zeros((E, N, 3), dtype=torch.float32, device=sim.device)
    packed = torch.zeros((E, N, 4, nat.TRAJ_COLS), dtype=torch.float64, device=sim.device)
    counts = torch.zeros((E, N), dtype=torch.int32, device=sim.device)
    with pytest.raises(RuntimeError, match="set_agent_spaces"):
        sim.step_mixed(lane=lane)
    no_table = nat.SmxMixedActions()
    no_table.lane_dev = lane.data_ptr()
    with pytest.raises(nat.SmxError, match="no table of agent spaces is bound"):
        sim._tick("smx_step_mixed", ctypes.byref(no_table))
    with pytest.raises(nat.SmxError, match="slot 1.*Imitation"):
        sim.set_agent_spaces(["Lane", "Imitation", "Lane", "Lane", "Lane", "Lane"])
    with pytest.raises(nat.SmxError, match="n_agents is 5"):
        sim.set_agent_spaces(["Lane"] * 5)
    sim.set_agent_spaces(["Lane", "Continuous", "Lane", "Lane", "Trajectory", "Lane"])
    learner = sim.out["learner"]
    with pytest.raises(nat.SmxError, match="smx_step_mixed"):
        sim.step(lane)
    assert sim.out["learner"] is learner  # (a refused call flips nothing)
    for entry, args in (("smx_step_continuous", (floats.data_ptr(),)), ("smx_step_trajectory", (packed.data_ptr(), counts.data_ptr())),
                        ("smx_step_target_pose", (packed.data_ptr(),)), ("smx_step_trajectory_with_time", (packed.data_ptr(), counts.data_ptr(), 2)),
                        ("smx_step_history_agents", ()), ("smx_step_history_handover", (floats.data_ptr(),))):
        with pytest.raises(nat.SmxError, match=f"{entry}: per-agent action spaces are bound.*smx_step_mixed"):
            sim._tick(entry, *args)
    for method, args in ((sim.step_trajectory, (packed, counts)), (sim.step_target_pose, (packed[..., 0],)),
                         (sim.step_trajectory_with_time, (packed, counts)), (sim.step_history_agents, ())):
        with pytest.raises((ValueError, RuntimeError)):
            method(*args)
    with pytest.raises(ValueError, match="needs floats"):
        sim.step_mixed(lane=lane, trajectories=packed, counts=counts)
    with pytest.raises(ValueError, match="needs trajectories and counts"):
        sim.step_mixed(lane=lane, floats=floats, trajectories=packed)
    with pytest.raises(ValueError, match="needs lane"):
        sim.step_mixed(floats=floats, trajectories=packed, counts=counts)
    acts = nat.SmxMixedActions()
    acts.lane_dev, acts.floats_dev = lane.data_ptr(), floats.data_ptr()
    with pytest.raises(nat.SmxError, match="trajectories_dev or counts_dev is NULL"):
        sim._tick("smx_step_mixed", ctypes.byref(acts))
    sim.set_agent_spaces(["Lane", "Lane", "Lane", "Lane", "Lane", "LaneWithContinuousSpeed"])
    sim.step_mixed(lane=lane, floats=floats)  # (no Trajectory slot any more: those buffers may be missing)
    # a Lane code that names no action is reported for Lane slots only: no other slot's byte is read
    odd = lane.clone()
    odd[:, 5] = 77
    sim.step_mixed(lane=odd, floats=floats)
    sim.sync()
    odd[:, 0] = 77
    sim.step_mixed(lane=odd, floats=floats)
    with pytest.raises(nat.SmxError, match="Lane action code"):
        sim.sync()
    sim.set_agent_spaces(None)
    with pytest.raises(RuntimeError, match="set_agent_spaces"):
        sim.step_mixed(lane=lane)
    # unbound: a uniform Lane run is the run of a sim that never had a table, bit for bit
    sim.reset()
    plain.reset()
    rng = np.random.default_rng(91)
    for t in range(10):
        a = torch.from_numpy(parity.lane_actions(rng, E, N))
        o1, o2 = sim.step(a), plain.step(a)
        torch.cuda.synchronize()
        assert torch.equal(sim.state, plain.state) and torch.equal(sim.flags, plain.flags), t
        for k in ("ego_pos", "ego_f32", "wp_pos", "done", "events", "nb_slot"):
            assert torch.equal(o1[k], o2[k]), (t, k)
    sim.close()
    plain.close()


def test_hiway_env_drives_a_mixed_fleet():
    """Four specs that differ in their action space only — Laner, Standard, LanerWithSpeed, Tracker — each stepped with
    its native action type: ego positions and dones are those of BatchedSim.step_mixed on the same spawns and the
    encoded actions."""
    import torch

    from smarts_amd.engine import BatchedSim
    from smarts_amd.env import AgentInterface, AgentSpec, AgentType, HiWayEnv

    types = {"laner": AgentType.Laner, "standard": AgentType.Standard, "speeder": AgentType.LanerWithSpeed, "tracker": AgentType.Tracker}
    specs = {a: AgentSpec(interface=AgentInterface.from_type(t, waypoints=True, neighborhood_vehicles=True, max_episode_steps=8))
             for a, t in types.items()}
    ids = list(specs)
    env = HiWayEnv(scenarios=["scenarios/loop"], agent_specs=specs, seed=7)
    obs = env.reset()
    core = env._core
    assert core.mixed and core.sim.agent_spaces == ("Lane", "ActuatorDynamic", "LaneWithContinuousSpeed", "Trajectory")
    twin = BatchedSim(core.cm, core.cfg, spawns=core.sim.spawns.cpu().numpy())
    twin.set_agent_spaces(core.sim.agent_spaces)
    out = twin.reset()
    lane_script = ["keep_lane", "change_lane_left", "slow_down", "keep_lane"]
    ended = set()
    for t in range(10):
        pos = out["ego_pos"].cpu().numpy()[0]
        for i, a in enumerate(ids):
            if a in obs:
                assert np.array_equal(obs[a].ego_vehicle_state.position, pos[i]), (t, a)
        actions = {}
        if "laner" in obs:
            actions["laner"] = lane_script[t % 4]
        if "standard" in obs:
            actions["standard"] = (0.6, 0.0, 0.1 if t % 2 else -0.1)
        if "speeder" in obs and t != 3:  # (a tick without an action)
            actions["speeder"] = (9.0 + t, [0, 1, 0, -1][t % 4])
        if "tracker" in obs:
            path = obs["tracker"].waypoint_paths[0][:10]
            actions["tracker"] = ([float(w.pos[0]) for w in path], [float(w.pos[1]) for w in path], [float(w.heading) for w in path],
                                  [8.0 + 0.2 * k for k in range(len(path))])
        lane, floats, packed, counts = core.encode_mixed_actions([actions])
        assert (lane[0, 0] >= 0) == ("laner" in actions) and np.isnan(floats[0, 2, 0]) == ("speeder" not in actions)
        obs, rewards, dones, infos = env.step(actions)
        out = twin.step_mixed(torch.from_numpy(lane), torch.from_numpy(floats), torch.from_numpy(packed), torch.from_numpy(counts))
        done = out["done"].cpu().numpy()[0]
        assert {a: bool(done[i]) for i, a in enumerate(ids) if a in dones} == {a: dones[a] for a in ids if a in dones}, t
        ended |= {a for a in ids if dones.get(a)}
        if dones["__all__"]:
            break
    assert ended == set(ids) and dones["__all__"] and t >= 5  # max_episode_steps ends everybody, after the silent tick too
    twin.close()
    env.close()

"""The LARGE launch form (smx_plan.h tick_plan(); AUTO picks it above 16 384 vehicles) with every action space,
social traffic, the grid maps, vias and the config variants, and the OGM kernel forms that only large batches reach.

The large form has kernels and template instantiations of its own (k_control_fast / k_control_paths / k_control_law
per action space, k_social ahead of k_alive_list, k_dagm beside the scan, k_waypoints past SMX_WPT_MAX_PATHS rows,
k_ogm_env<1> / <2> / k_ogm by tile size and env size).  Forced onto oracle-sized batches, every output is held to the
oracle teacher-forced (float64 to 1e-9, float32 to 2e-6 on reset and 2e-5 on ticks, integers, flags, counts and grids
bit-exact); long auto-reset runs are held to the small form bit for bit; a batch at the size where the small form
draws OGM tiles with k_ogm_env<2> is held to an 8-env small batch.  Every test first asserts the form it exercises.
"""
import numpy as np
import pytest

import parity
from test_gpu_parity import VARIANTS

pytestmark = pytest.mark.gpu

CUTS = ("large_one_lane", "large_teams")
FORMS = ("small",) + CUTS
TOL_RESET = dict(tol64=1e-9, tol32=2e-6)
TOL_TICK = dict(tol64=1e-9, tol32=2e-5)
OGM64 = dict(ogm=True, ogm_width=64, ogm_height=64, ogm_resolution=50 / 64)

# LaneWithContinuousSpeed draws: target speeds with the clip window of the heading gain (2.02-2.06 m/s) and 0; lane
# changes that truncate toward zero (+-0.99), that clip at either end of the path list (+-2, +-3) and, for a few
# agents, far outside the int32 range (the reference's int(action[1]) is a Python int: np.clip(current + change, 0,
# n - 1) then picks the first / last path whatever the current one)
SPEEDS = [0.0, 2.03, 2.045, 5.0, 9.5, 14.0, 18.0]
CHANGES = [-3.0, -1.0, -0.99, 0.0, 0.0, 0.0, 0.99, 1.0, 2.0, 3.0]


def _forced(name, E, N, nets, compiled_maps, seed, strategy, **kw):
    sim, ob, cfg = parity.make(name, E, N, nets, compiled_maps, seed, launch_strategy=strategy, **kw)
    assert sim.launch_form() == strategy
    return sim, ob, cfg


def _check_reset(sim, ob):
    d = parity.host(sim.reset())
    bad = parity.compare(d, ob.reset_observe(), where="reset ", **TOL_RESET)
    assert bad == [], "\n".join(bad[:8])
    return d


def _check_tick(sim, ob, d, o, where):
    bad = parity.compare(d, o, where=where, **TOL_TICK)
    assert bad == [], "\n".join(bad[:8])
    parity.sync_oracle_from_device(ob, sim)


def _float_actions(space, rng, E, N, t):
    """float32 [E, N, 3] actions of `space`; NaN in the first component = no action this tick."""
    if space == "LaneWithContinuousSpeed":
        speed = rng.choice(SPEEDS, size=(E, N))
        change = rng.choice(CHANGES, size=(E, N))
        change = np.where(rng.random((E, N)) < 0.1, rng.choice([-3e9, 3e9], size=(E, N)), change)
        acts = np.stack([speed, change, np.zeros((E, N))], axis=-1).astype(np.float32)
    else:
        # test_gpu_parity.test_float_action_spaces' draws, plus hard steering: inside (0.9, 1) and past the clip at +-1
        steer = np.where(rng.random((E, N)) < 0.2, rng.choice([-1.2, -1.0, -0.95, 0.95, 1.0, 1.2], size=(E, N)),
                         rng.uniform(-1.3, 1.3, (E, N)) * 0.3)
        acts = np.stack([rng.uniform(-0.2, 1.2, (E, N)), np.where(rng.random((E, N)) < 0.2, rng.uniform(0, 1, (E, N)), 0.0),
                         steer], axis=-1).astype(np.float32)
    if t % 5 == 2:
        acts[0, 0, 0] = np.nan
        acts[-1, -1, 0] = np.nan
    return acts


def _trajectory_actions(rng, d, cfg, t, with_oracle=True):
    """Every agent tracks one of its own waypoint rows of the last observation `d` (host layout) with a speed profile;
    (packed [E, N, 4, 11], counts [E, N], the oracle's action lists or None)."""
    from oracle import controller as octl
    from smarts_amd.engine import pack_trajectory

    E, N, P, W = cfg.num_envs, cfg.num_vehicles, cfg.wp_paths, cfg.wp_len
    packed = np.zeros((E, N, 4, 11))
    counts = np.zeros((E, N), dtype=np.int32)
    oracle_actions = [[([], [], [], []) for _ in range(N)] for _ in range(E)] if with_oracle else None
    wp_pos = d["wp_pos"].reshape(E, N, P, W, 3)
    wp_h = d["wp_heading"].reshape(E, N, P, W)
    wp_c = d["wp_count"].reshape(E, N, P + 1)
    act = d["active"].reshape(E, N)
    for e in range(E):
        for i in range(N):
            if not act[e, i] or wp_c[e, i, 0] == 0 or (t % 6 == 4 and i == 0):
                continue  # gone, nothing to track, or a tick without an action
            p = int(rng.integers(min(int(wp_c[e, i, 0]), P)))
            n = min(int(rng.choice([3, 7, 10, 11, 20])), int(wp_c[e, i, 1 + p]))
            if n == 0:
                continue
            v0 = float(rng.choice([0.0, 6.0, 11.0, 16.0, 22.0]))
            traj = (wp_pos[e, i, p, :n, 0].tolist(), wp_pos[e, i, p, :n, 1].tolist(),
                    [float(x) for x in wp_h[e, i, p, :n]], [v0 + 0.1 * k for k in range(n)])
            packed[e, i], counts[e, i] = pack_trajectory(traj)
            if with_oracle:
                oracle_actions[e][i] = octl.unpack_trajectory(packed[e, i], n)
    return packed, counts, oracle_actions


def _via_setup(cm, E, N, seed, episodes):
    """test_gpu_parity.test_via_sensor's world: the via points of scenarios/intersections/4lane's mission, slots 0 and 1
    of every env on the approach lanes below the 13 m/s vias at 13 m/s, the last slot without vias."""
    from smarts_amd.engine import lane_heading, make_spawns
    from smarts_amd.vias import Via, _position_at_shape_offset, resolve_vias

    vias = resolve_vias(cm, [Via("edge-south-SN", 1, 30, 4), Via("edge-west-EW", 0, 20, 8), Via("edge-west-EW", 1, 50, 2),
                             Via("edge-west-EW", 0, 55, 5), Via("edge-south-SN", 0, 25, 13, hit_distance=3.0),
                             Via("edge-south-SN", 1, 45, 13, hit_distance=3.0)])
    spawns = make_spawns(cm, E, N, episodes=episodes, seed=seed)
    for slot, (lane_id, off) in enumerate([("edge-south-SN_0", 6.0), ("edge-south-SN_1", 20.0)]):
        shape = cm.lane_shape(cm.lane_ids.index(lane_id))
        x, y = _position_at_shape_offset(shape, off)
        spawns[:, slot::N] = (x, y, lane_heading(shape, 0), 13.0)
    per_slot = [vias if i % 2 == 0 else vias[:2] + vias[4:] for i in range(N - 1)] + [[]]
    return spawns, per_slot


# ---- 1. teacher-forced oracle parity in the forced large form ---------------------------------------------------


@pytest.mark.parametrize("space,name,E,N,T,seed", [("Continuous", "loop", 4, 8, 20, 141),
                                                  ("ActuatorDynamic", "4lane", 2, 16, 20, 142),
                                                  ("LaneWithContinuousSpeed", "loop", 4, 8, 25, 143),
                                                  ("LaneWithContinuousSpeed", "minicity", 2, 16, 20, 144)])
@pytest.mark.parametrize("strategy", CUTS)
def test_float_action_spaces(space, name, E, N, T, seed, strategy, nets, compiled_maps):
    """k_control_law<CONTINUOUS / ACTUATOR_DYNAMIC> and, for LaneWithContinuousSpeed, k_control_fast<3> with its
    listed kernels (one-lane cut) or k_control_paths<3> + k_control_law<3> (team cut) against the oracle.  A NaN lane
    change (or +-inf) with a finite speed makes the reference raise in int(); those inputs are left out."""
    import torch

    sim, ob, cfg = _forced(name, E, N, nets, compiled_maps, seed, strategy, action_space=space)
    _check_reset(sim, ob)
    rng = np.random.default_rng(seed)
    for t in range(T):
        acts = _float_actions(space, rng, E, N, t)
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts.astype(np.float64))
        _check_tick(sim, ob, d, o, f"{space} {name} {strategy} t{t} ")
    sim.close()


@pytest.mark.parametrize("strategy", FORMS)
def test_lane_change_far_outside_the_int32_range(strategy, nets, compiled_maps):
    """LaneWithContinuousSpeed lane changes of +-3e9 on every agent, in all three forms (k_control; k_control_fast and
    its listed kernels; k_control_paths): the reference clips current + change with Python ints, so +3e9 picks the
    last path and -3e9 the first, from whichever path the vehicle is on.  (NaN / +-inf lane changes are left out: the
    reference raises on them.)"""
    import torch

    E, N, T = 2, 16, 12
    sim, ob, cfg = _forced("minicity", E, N, nets, compiled_maps, 145, strategy, action_space="LaneWithContinuousSpeed")
    _check_reset(sim, ob)
    rng = np.random.default_rng(145)
    for t in range(T):
        speed = rng.choice([5.0, 9.5, 14.0], size=(E, N))
        change = rng.choice([-3e9, 3e9], size=(E, N))
        acts = np.stack([speed, change, np.zeros((E, N))], axis=-1).astype(np.float32)
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts.astype(np.float64))
        _check_tick(sim, ob, d, o, f"lane change 3e9 {strategy} t{t} ")
    sim.close()


@pytest.mark.parametrize("name,E,N,T,seed", [("loop", 3, 6, 25, 161), ("minicity", 2, 12, 15, 162)])
@pytest.mark.parametrize("strategy", CUTS)
def test_trajectory_action_space(name, E, N, T, seed, strategy, nets, compiled_maps):
    """k_control_law<TRAJECTORY> (PD tracking) through step_trajectory, rows of the previous tick as targets."""
    import torch

    sim, ob, cfg = _forced(name, E, N, nets, compiled_maps, seed, strategy, action_space="Trajectory")
    d = _check_reset(sim, ob)
    rng = np.random.default_rng(seed)
    for t in range(T):
        packed, counts, oracle_actions = _trajectory_actions(rng, d, cfg, t)
        d = parity.host(sim.step_trajectory(torch.from_numpy(packed), torch.from_numpy(counts)))
        parts = []
        for e, env in enumerate(ob.envs):
            obs, rew, dones = env.step(oracle_actions[e])
            parts.append(parity.pack(cfg, ob.lane_no, N, obs, rew, dones))
        _check_tick(sim, ob, d, ob._stack(parts), f"trajectory {name} {strategy} t{t} ")
    sim.close()


@pytest.mark.parametrize("model,name,E,agents,social,T,seed", [("constant", "loop", 2, 6, 10, 25, 151),
                                                               ("constant", "4lane", 2, 4, 12, 20, 152),
                                                               ("idm", "loop", 2, 4, 12, 30, 154),
                                                               ("idm", "4lane", 2, 4, 12, 20, 155)])
@pytest.mark.parametrize("strategy", CUTS)
def test_social_traffic(model, name, E, agents, social, T, seed, strategy, nets, compiled_maps):
    """Scripted (constant-speed) and IDM social vehicles in the last slots: k_control_fast's / control_law_for's
    social branch, k_scan_fast's social rows, k_social ahead of k_alive_list; OGM 64 x 64 (k_ogm_env<2>) with the
    scripted fleet on loop."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps(name)
    N = agents + social
    if model == "idm":
        kw = dict(social_model="idm", social_speed_factor=1.0, done_collision=False)
    else:
        kw = dict(done_collision=True, **(OGM64 if name == "loop" else {}))
    cfg = SimConfig(num_envs=E, num_vehicles=N, num_social=social, neighbors=True, nb_radius=60.0, launch_strategy=strategy,
                    **kw)
    spawns, where = make_spawns(cm, E, N, episodes=2, seed=seed, return_lanes=True)
    sim = BatchedSim(cm, cfg, spawns=spawns, social_spawns=where)
    assert sim.launch_form() == strategy
    ob = parity.OracleBatch(nets(name), cm, cfg, spawns[0], where[0])
    d = _check_reset(sim, ob)
    assert d["active"].reshape(E, N)[:, agents:].sum() == 0  # social slots never observe
    rng = np.random.default_rng(seed)
    saw_social_neighbour = 0
    pos0 = sim.state[0:2, :, agents:].clone()
    for t in range(T):
        acts = parity.lane_actions(rng, E, N)
        if model == "idm":
            acts[:, 0] = 1  # agent 0 of every env brakes to a stop: a standing obstacle for whoever follows it
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
        _check_tick(sim, ob, d, o, f"{model} {name} {strategy} t{t} ")
        saw_social_neighbour += int((d["nb_slot"] >= agents).sum())
    assert saw_social_neighbour > 0
    moved = (sim.state[0:2, :, agents:] - pos0).norm(dim=0)
    assert float(moved.median()) > 5.0  # the social fleet drove on
    sim.close()


@pytest.mark.parametrize("name,E,N,T,seed,grid", [("loop", 2, 8, 8, 135, (64, 64, 50 / 64)), ("4lane", 1, 12, 6, 136, (64, 32, 0.5))])
@pytest.mark.parametrize("strategy", CUTS)
def test_drivable_area_grid_map(name, E, N, T, seed, grid, strategy, nets, compiled_maps):
    """k_dagm (on side stream 0 beside the scan) and k_grid_first<true> on reset, bit-exact against the oracle's
    raster, square and not."""
    import torch

    kw = dict(dagm=True, dagm_width=grid[0], dagm_height=grid[1], dagm_resolution=grid[2])
    sim, ob, cfg = _forced(name, E, N, nets, compiled_maps, seed, strategy, **kw)
    d = _check_reset(sim, ob)
    assert (d["dagm"] == 255).any()
    rng = np.random.default_rng(seed)
    for t in range(T):
        acts = parity.lane_actions(rng, E, N)
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
        _check_tick(sim, ob, d, o, f"dagm {name} {strategy} t{t} ")
    sim.close()


@pytest.mark.parametrize("strategy", CUTS)
def test_via_sensor(strategy, nets, compiled_maps):
    """Via rows (via_max > 0) in the large form: hits occur, and lists longer than via_max occur."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig

    cm = compiled_maps("4lane")
    E, N = 3, 8
    cfg = SimConfig(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, via_max=4, done_off_route=False,
                    launch_strategy=strategy)
    spawns, per_slot = _via_setup(cm, E, N, 71, episodes=2)
    sim = BatchedSim(cm, cfg, spawns=spawns, vias=per_slot)
    assert sim.launch_form() == strategy
    ob = parity.OracleBatch(nets("4lane"), cm, cfg, spawns[0], vias=per_slot)
    _check_reset(sim, ob)
    rng = np.random.default_rng(71)
    hits = near_rows = 0
    for t in range(30):
        acts = parity.lane_actions(rng, E, N)
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
        _check_tick(sim, ob, d, o, f"vias {strategy} t{t} ")
        hits += int(sum(bin(int(x)).count("1") for x in d["via_hit"]))
        near_rows += int((d["via_near_count"] > cfg.via_max).sum())
    assert hits > 0 and near_rows > 0
    sim.close()


LARGE_VARIANTS = {k: VARIANTS[k] for k in ("no_waypoints_sensor", "short_lookahead_two_paths", "all_done_criteria",
                                           "agents_alive", "half_timestep", "no_neighbours")}
LARGE_VARIANTS["nine_rows"] = dict(wp_paths=9, wp_len=12)  # one row past SMX_WPT_MAX_PATHS: k_waypoints


@pytest.mark.parametrize("variant", sorted(LARGE_VARIANTS))
@pytest.mark.parametrize("strategy", CUTS)
def test_config_variants(variant, strategy, nets, compiled_maps):
    """AgentInterface options in the large form on loop (3 x 7: ragged workgroups): no waypoints sensor (no knot
    lists for k_control_fast), a lookahead under SMX_CTRL_WPS - 1 (every vehicle through the control slow list),
    nine rows (k_waypoints instead of walk + emit), done criteria, agents_alive, dt = 0.05, no neighbours."""
    import torch

    E, N = 3, 7
    kw = dict(LARGE_VARIANTS[variant])
    if kw.get("alive_min_ego") == "N":
        kw["alive_min_ego"] = N
    sim, ob, cfg = _forced("loop", E, N, nets, compiled_maps, 77, strategy, **kw)
    _check_reset(sim, ob)
    rng = np.random.default_rng(77)
    seen_alive_done = 0
    for t in range(18):
        acts = parity.lane_actions(rng, E, N)
        if variant == "all_done_criteria":
            acts[:, ::2] = 1  # slow_down: half of the fleet stops and trips not_moving
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
        _check_tick(sim, ob, d, o, f"{variant} {strategy} t{t} ")
        seen_alive_done += int(d["events"][:, 8].sum())
    if variant == "agents_alive":
        assert seen_alive_done > 0  # the criterion fired
    sim.close()


# ---- 2. the OGM kernel forms ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,E,N,T,seed,grid,strategy", [
    ("minicity", 1, 64, 5, 181, (64, 64, 50 / 64), "large_teams"),         # N > 32: k_ogm_env<1>
    ("loop", 2, 16, 6, 182, (128, 128, 50 / 128), "large_one_lane"),       # 16 KiB tiles: four fit 64 KiB, eight do not
    ("loop", 2, 16, 6, 183, (96, 32, 0.5), "large_one_lane"),              # not square, k_ogm_env<2>
    ("loop", 2, 16, 6, 184, (128, 96, 50 / 128), "large_teams"),           # not square, k_ogm_env<1>
    ("loop", 1, 8, 4, 185, (256, 256, 50 / 256), "large_one_lane"),        # the default grid: k_ogm per observer
])
def test_ogm_kernel_forms(name, E, N, T, seed, grid, strategy, nets, compiled_maps):
    """The large form's OGM tiles (TickPlan::ogm in smx_plan.h) bit-exact against the oracle; every alive agent's own
    footprint fills the 2 x 2 centre of its grid."""
    import torch

    w, h, res = grid
    sim, ob, cfg = _forced(name, E, N, nets, compiled_maps, seed, strategy, ogm=True, ogm_width=w, ogm_height=h,
                           ogm_resolution=res)
    d = _check_reset(sim, ob)
    rng = np.random.default_rng(seed)
    for t in range(T + 1):
        act = d["active"].astype(bool)
        assert act.any()
        g = d["ogm"].reshape(E * N, h, w)[act]
        assert g[:, h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1].min() == 255, t
        if t == T:
            break
        acts = parity.lane_actions(rng, E, N)
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
        _check_tick(sim, ob, d, o, f"ogm {w}x{h} {strategy} t{t} ")
    sim.close()


def test_small_form_per_env_ogm_at_the_threshold(compiled_maps):
    """512 x 32 with OGM 64 x 64 (configs[3]'s 8-GPU shard): AUTO keeps the small form at exactly 16 384 vehicles and
    draws the tiles with k_ogm_env<2> (SMX_OGM_ENV_MIN_VEHICLES).  Eight distinct envs tiled: the first and the last
    slice must equal an 8-env batch, whose tiles k_sensors draws, bit for bit."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    name, E, N, sub, ticks = "loop", 512, 32, 8, 10
    assert E * N == nat.LARGE_BATCH_VEHICLES and E * N >= nat.OGM_ENV_MIN_VEHICLES
    cm = compiled_maps(name)
    spawns = make_spawns(cm, sub, N, episodes=1, seed=19)
    big = np.tile(spawns, (1, E // sub, 1))
    kw = dict(num_vehicles=N, neighbors=True, nb_radius=50.0, **OGM64)
    sim = BatchedSim(cm, SimConfig(num_envs=E, **kw), spawns=big)
    sim2 = BatchedSim(cm, SimConfig(num_envs=sub, launch_strategy="small", **kw), spawns=spawns)
    assert sim.launch_form() == "small" and sim2.launch_form() == "small"
    rng = np.random.default_rng(19)
    sim.reset(), sim2.reset()
    for t in range(ticks):
        a_small = parity.lane_actions(rng, sub, N)
        o1 = sim.step(torch.from_numpy(np.tile(a_small, (E // sub, 1))).cuda())
        o2 = sim2.step(torch.from_numpy(a_small).cuda())
    torch.cuda.synchronize()
    for k in o2:
        a, b = o1[k].cpu().numpy(), o2[k].cpu().numpy()
        first, last = (a[:, :sub], a[:, E - sub:]) if k == "learner" else (a[:sub], a[E - sub:])
        assert np.array_equal(first, b, equal_nan=True) and np.array_equal(last, b, equal_nan=True), k
    act = o2["active"].cpu().numpy().reshape(-1).astype(bool)
    g = o2["ogm"].cpu().numpy().reshape(sub * N, 64, 64)[act]
    assert act.any() and g[:, 31:33, 31:33].min() == 255
    sim.close(), sim2.close()


# ---- 3. small vs large, bit for bit, over long auto-reset runs ---------------------------------------------------

DAGM64 = dict(dagm=True, dagm_width=64, dagm_height=64, dagm_resolution=50 / 64)
LONG_RUNS = {
    "continuous": ("loop", 40, 8, dict(action_space="Continuous")),
    "lane_with_continuous_speed": ("minicity", 20, 16, dict(action_space="LaneWithContinuousSpeed")),
    "trajectory": ("loop", 32, 8, dict(action_space="Trajectory")),
    "idm_social_dagm": ("4lane", 20, 16, dict(num_social=12, social_model="idm", social_speed_factor=1.0, **DAGM64)),
    "vias": ("4lane", 40, 8, dict(via_max=4, done_off_route=False)),
}


@pytest.mark.parametrize("feature", sorted(LONG_RUNS))
def test_forms_agree_bit_for_bit_over_auto_reset_runs(feature, compiled_maps):
    """The small form and both cuts of the large form over 50 auto-reset ticks (episodes of 24 steps: restarts through
    k_first with walk_new, k_grid_first<true>; alive lists that thin out; slow lists under each feature), with a
    masked reset of every third env in mid-run: every output, the state and the flags agree bit for bit."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    name, E, N, extra = LONG_RUNS[feature]
    extra = dict(extra)
    cm = compiled_maps(name)
    seed, T, mask_at = 23, 50, 17
    kw = dict(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, auto_reset=True, max_episode_steps=24, **extra)
    sim_kw = {}
    if feature == "vias":
        spawns, sim_kw["vias"] = _via_setup(cm, E, N, seed, episodes=4)
    elif extra.get("num_social"):
        spawns, sim_kw["social_spawns"] = make_spawns(cm, E, N, episodes=4, seed=seed, return_lanes=True)
    else:
        spawns = make_spawns(cm, E, N, episodes=4, seed=seed)
    sims = [BatchedSim(cm, SimConfig(launch_strategy=s, **kw), spawns=spawns, **sim_kw) for s in FORMS]
    assert [s.launch_form() for s in sims] == list(FORMS)
    space = extra.get("action_space", "Lane")
    rng = np.random.default_rng(seed)
    outs = [s.reset() for s in sims]

    def check(t):
        torch.cuda.synchronize()
        for other in (1, 2):
            for k in outs[0]:
                assert np.array_equal(outs[0][k].cpu().numpy(), outs[other][k].cpu().numpy(), equal_nan=True), (t, k, FORMS[other])
            assert np.array_equal(sims[0].state.cpu().numpy(), sims[other].state.cpu().numpy(), equal_nan=True), (t, FORMS[other])
            assert np.array_equal(sims[0].flags.cpu().numpy(), sims[other].flags.cpu().numpy()), (t, FORMS[other])

    check("reset")
    mask = torch.from_numpy((np.arange(E) % 3 == 1).astype(np.uint8))
    for t in range(T):
        if t == mask_at:
            outs = [s.reset(mask) for s in sims]
            check(f"masked reset at t{t}")
        if space == "Trajectory":
            packed, counts, _ = _trajectory_actions(rng, parity.host(outs[0]), sims[0].cfg, t, with_oracle=False)
            packed, counts = torch.from_numpy(packed), torch.from_numpy(counts)
            outs = [s.step_trajectory(packed, counts) for s in sims]
        else:
            if space == "Lane":
                acts = parity.lane_actions(rng, E, N)
            else:
                acts = _float_actions(space, rng, E, N, t)
            acts = torch.from_numpy(acts).cuda()
            outs = [s.step(acts) for s in sims]
        if t % 5 == 4 or t == T - 1:
            check(f"t{t}")
    episodes = sims[0].env_episode.cpu().numpy()
    assert (episodes[mask.numpy() == 1] >= 2).all() and (episodes >= 1).all()  # masked and auto restarts both happened
    for s in sims:
        s.close()

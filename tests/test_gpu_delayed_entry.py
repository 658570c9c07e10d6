"""Delayed agent entry on the device (include/smx.h smx_set_agent_entry; smarts_amd/csrc/smx_k_entry.h), through
BatchedSim and the env layer.

Every case is decided before it touches the device: a free run of the NumPy model (tests/delayed_entry_ref.py) over the
social slots' poses — the oracle's scripted lane followers, or the rows of a recorded table — asserts that no distance of
the case lies within 1e-6 m of its overlap radius, and that the case shows what it is there to show (no blocking where
timing is tested, blocking followed by entry where the overlap is).  The device's decisions are then compared exactly.
"""
import math

import numpy as np
import pytest

import delayed_entry_ref as ref

pytestmark = pytest.mark.gpu

E, A, S = 4, 4, 4
SEDAN_L = 3.68
CLEARANCE = 1e-6


def _front(row):
    """The front bumper of a spawn row (x, y, heading): PlannedMission.spawn_pose inverted."""
    a = (row[2] + math.pi * 0.5) % (2 * math.pi)
    return row[0] + math.cos(a) * 0.5 * SEDAN_L, row[1] + math.sin(a) * 0.5 * SEDAN_L


def _check_rows(spawns, n, agents, envs, dims=None):
    """check [1, envs, agents, 3]: every agent's start point (front bumper of its spawn row) and its largest plane dimension."""
    chk = np.zeros((1, envs, agents, 3))
    for e in range(envs):
        for a in range(agents):
            chk[0, e, a, :2] = _front(spawns[0, e * n + a])
    chk[..., 2] = SEDAN_L if dims is None else dims
    return chk


def _host(sim):
    import torch

    torch.cuda.synchronize()
    return {"status": sim.out["entry_status"].cpu().numpy(), "entered": sim.out["entered_tick"].cpu().numpy(),
            "flags": sim.flags.cpu().numpy(), "done_count": sim.env_done_count.cpu().numpy(),
            "active": sim.out["active"].cpu().numpy(), "done": sim.out["done"].cpu().numpy(),
            "ego_pos": sim.out["ego_pos"].cpu().numpy(), "events": sim.out["events"].cpu().numpy(),
            "env_done": sim.out["env_done"].cpu().numpy()}


def _expect_tick(d, status, entered, t, done_so_far, agents, what):
    """One pass's rows against the model's status after tick t (row t of its history)."""
    want_entered = np.where(entered <= t, entered, -1)
    want_entered[status[t] != ref.ENTERED] = -1
    assert np.array_equal(d["status"][:, :agents], status[t]), (what, t, d["status"][:, :agents], status[t])
    assert np.array_equal(d["entered"][:, :agents], want_entered), (what, t, d["entered"][:, :agents], want_entered)
    present = status[t] == ref.ENTERED
    alive = (d["flags"][:, :agents] & 1) != 0
    assert np.array_equal(alive, present & ~done_so_far), (what, t, alive, present, done_so_far)
    assert np.array_equal(d["done_count"], done_so_far.sum(axis=1)), (what, t, d["done_count"], done_so_far)
    # a pending agent's rows are an absent agent's
    pending = ~present
    assert not d["active"][:, :agents][pending].any() and not d["done"][:, :agents][pending].any(), (what, t)
    assert d["active"][:, :agents][present & ~done_so_far].all(), (what, t)  # an entrant observes from its entry tick on
    assert not d["ego_pos"][:, :agents][pending].any() and not d["events"][:, :agents][pending].any(), (what, t)


def _scripted_case(compiled_maps, oracle_maps, name, seed, ready_row, T, factor=0.8):
    from smarts_amd.engine import make_spawns

    cm, rm = compiled_maps(name), oracle_maps(name)
    N = A + S
    spawns, where = make_spawns(cm, E, N, episodes=1, seed=seed, return_lanes=True)
    ready = np.broadcast_to(np.asarray(ready_row, dtype=np.int32), (1, E, A)).copy()
    chk = _check_rows(spawns, N, A, E)
    xy = ref.scripted_poses(rm, cm, where[0], A, S, E, T, factor)
    return cm, spawns, where, ready, chk, xy


def _run_ticks(sim, status, entered, T, agents, what, act=None):
    import torch

    N = sim.N
    d = _host(sim)
    done_so_far = np.zeros((sim.E, agents), dtype=bool)
    _expect_tick(d, status, entered, 0, done_so_far, agents, what)
    acts = torch.zeros((sim.E, N), dtype=torch.int8, device=sim.device) if act is None else act
    for t in range(1, T + 1):
        sim.step(acts)
        d = _host(sim)
        done_so_far |= d["done"][:, :agents].astype(bool)
        _expect_tick(d, status, entered, t, done_so_far, agents, what)
    return d


@pytest.mark.parametrize("name,seed,form", [("loop", 16, "small"), ("4lane", 12, "small"), ("loop", 16, "large_one_lane"),
                                            ("4lane", 12, "large_teams")])
def test_timing(name, seed, form, compiled_maps, oracle_maps):
    """Ready ticks 0 / 3 / 3 / 9 and no social vehicle near any start point: every agent enters on its ready tick; status,
    entered tick, SMX_F_ALIVE and env_done_count after every tick equal the model's; a pending agent's rows read as an
    absent agent's, an entrant's are present from its entry tick on; the small form and both forced large ones.  (Without
    the binding — the parent commit — BatchedSim has no set_agent_entry.)"""
    from smarts_amd.engine import BatchedSim, SimConfig

    T = 12
    cm, spawns, where, ready, chk, xy = _scripted_case(compiled_maps, oracle_maps, name, seed, (0, 3, 3, 9), T)
    status, entered, clearance = ref.run(ready[0], chk[0], xy, np.ones(xy.shape[:3], dtype=bool))
    assert clearance >= CLEARANCE, clearance
    assert not (status == ref.BLOCKED).any() and np.array_equal(entered, ready[0]), "the case: nothing blocks"
    cfg = SimConfig(num_envs=E, num_vehicles=A + S, num_social=S, launch_strategy=form, neighbors=True, nb_radius=30.0)
    sim = BatchedSim(cm, cfg, spawns=spawns, social_spawns=where)
    assert sim.launch_form() == form
    sim.set_agent_entry(ready, chk)
    sim.reset()
    _run_ticks(sim, status, entered, T, A, name + " " + form)
    sim.close()


def test_steps_wait_for_a_reset_after_a_bind_or_unbind(compiled_maps):
    """A table bound or unbound in mid-episode would meet status rows that describe no episode: steps are refused until a
    reset of every env (a masked one does not do); then entry runs from that reset.  Nothing was respawned meanwhile."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps("loop")
    spawns = make_spawns(cm, E, A, episodes=1, seed=71)
    sim = BatchedSim(cm, SimConfig(num_envs=E, num_vehicles=A, launch_strategy="small", done_collision=False,
                                   done_off_road=False, done_off_route=False), spawns=spawns)
    acts = torch.zeros((E, A), dtype=torch.int8, device=sim.device)
    sim.reset()
    for _ in range(3):
        sim.step(acts)
    steps = sim.steps.clone()
    ready = np.zeros((1, E, A), dtype=np.int32)
    ready[0, :, 1] = 2
    sim.set_agent_entry(ready, _check_rows(spawns, A, A, E))
    with pytest.raises(nat.SmxError, match="step after one"):
        sim.step(acts)
    sim.reset(torch.tensor([1, 0, 1, 0], dtype=torch.uint8))
    with pytest.raises(nat.SmxError, match="step after one"):
        sim.step(acts)
    assert torch.equal(sim.steps[[1, 3]], steps[[1, 3]]), "no live agent was touched"
    sim.reset()
    for t in range(1, 3):
        sim.step(acts)
        torch.cuda.synchronize()
        assert (sim.out["entered_tick"][:, 1] == (2 if t >= 2 else -1)).all() and (sim.steps[:, 0] == 1 + t).all()
    sim.set_agent_entry(None)  # an unbind in mid-episode: agent 1 would stay out; steps wait for a reset again
    with pytest.raises(nat.SmxError, match="step after one"):
        sim.step(acts)
    sim.reset()
    sim.step(acts)
    torch.cuda.synchronize()
    assert ((sim.flags & 1) == 1).all()
    sim.close()


def _history_over(point, heading, first_frame, frames, speed=10.0, length=None):
    """A TrafficHistoryTable (from_rows) whose one vehicle, id 7, drives straight through `point` along `heading` at
    `speed`, a quarter metre past it in frame `first_frame + 6`; every other slot empty."""
    from smarts_amd.traffic_history import TrafficHistoryTable

    dt = 0.1
    fx, fy = -math.sin(heading), math.cos(heading)  # heading 0 faces +y
    rows = []
    for f in range(first_frame, first_frame + frames):
        s = (f - first_frame - 6) * speed * dt + 0.25  # (a quarter metre off the point: no tick sits on a boundary)
        rows.append((7, round(f * dt, 6), point[0] + fx * s, point[1] + fy * s, heading, speed))
    vehicles = [(7, 2, length, None if length is None else 2.5, None if length is None else 4.0)]
    return TrafficHistoryTable.from_rows(vehicles, rows, dt, S)


def _history_model(table, start, res, T, agents_env, lw=False):
    """Social poses, presence and boxes over ticks 1..T from a table's own rows (frame start + res + t)."""
    xy = np.zeros((T, agents_env, S, 2))
    alive = np.zeros((T, agents_env, S), dtype=bool)
    box = np.tile(np.array(ref.SEDAN), (T, agents_env, S, 1))
    for t in range(1, T + 1):
        f = start + res + t
        if f >= table.num_frames:
            continue
        xy[t - 1, :, :, :] = table.frames[f, :, :2]
        alive[t - 1, :, :] = table.vehicle[f] >= 0
        if lw:
            for s in range(S):
                v = int(table.vehicle[f, s])
                if v >= 0:
                    box[t - 1, :, s] = table.resolved_dimensions(v)[:2]
    return xy, alive, box


@pytest.mark.parametrize("variant,form", [("scripted", "small"), ("history", "small"), ("history_dims", "small"),
                                          ("scripted", "large_one_lane"), ("history", "large_teams")])
def test_blocked_then_clear(variant, form, compiled_maps, oracle_maps):
    """A social vehicle drives over agent 1's start point: agent 1 is BLOCKED for exactly the model's ticks and enters on
    the first clear one — scripted traffic, a recorded table (TrafficHistoryTable.from_rows), and that table with its
    vehicle 12 m long and its dimensions bound, which widens the radius the slot's box gives; the small form and both
    forced large ones."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    T = 30
    cm, rm = compiled_maps("loop"), oracle_maps("loop")
    N = A + S
    spawns, where = make_spawns(cm, E, N, episodes=1, seed=21, return_lanes=True)
    ready = np.zeros((1, E, A), dtype=np.int32)
    ready[0, :, 1] = 3
    cfg = SimConfig(num_envs=E, num_vehicles=N, num_social=S, launch_strategy=form, done_collision=False)
    res = cfg.reset_elapsed_steps()
    if variant == "scripted":
        xy = ref.scripted_poses(rm, cm, where[0], A, S, E, T, 0.8)
        alive, box = np.ones(xy.shape[:3], dtype=bool), None
        # agent 1's start point: where social slot 0 of its env is in tick 5, a quarter metre ahead of it
        for e in range(E):
            p, q = xy[4, e, 0], xy[5, e, 0]
            h = math.atan2(q[1] - p[1], q[0] - p[0]) - 0.5 * math.pi
            front = (p[0] + 0.25 * math.cos(h), p[1] + 0.25 * math.sin(h))
            a = h + 0.5 * math.pi
            spawns[0, e * N + 1, :3] = (front[0] - math.cos(a) * 0.5 * SEDAN_L, front[1] - math.sin(a) * 0.5 * SEDAN_L, h)
        table = None
    else:
        # a start point of agent 1 in every env: the same (the table is every env's), half way along the middle segment
        # of the lane with the most vertices; its spawn row with it
        lane = max(range(cm.n_lanes), key=lambda i: len(cm.lane_shape(i)))
        shape = cm.lane_shape(lane)
        p, q = shape[len(shape) // 2 - 1], shape[len(shape) // 2]
        h = math.atan2(q[1] - p[1], q[0] - p[0]) - 0.5 * math.pi
        front = (0.5 * (p[0] + q[0]), 0.5 * (p[1] + q[1]))
        a = h + 0.5 * math.pi
        for e in range(E):
            spawns[0, e * N + 1, :3] = (front[0] - math.cos(a) * 0.5 * SEDAN_L, front[1] - math.sin(a) * 0.5 * SEDAN_L, h)
        table = _history_over(front, h, 0, res + T + 2, length=12.0 if variant == "history_dims" else None)
        xy, alive, box = _history_model(table, 0, res, T, E, lw=variant == "history_dims")
    chk = _check_rows(spawns, N, A, E)
    status, entered, clearance = ref.run(ready[0], chk[0], xy, alive, box)
    assert clearance >= CLEARANCE, clearance
    blocked = (status[:, :, 1] == ref.BLOCKED).sum(axis=0)
    assert (blocked >= 2).all() and (entered[:, 1] > 3).all() and (entered[:, 1] < T).all(), (blocked, entered)
    if variant == "history_dims":  # the long box blocks longer than a sedan would
        _, sedan_entered, _ = ref.run(ready[0], chk[0], xy, alive, None)
        assert (entered[:, 1] > sedan_entered[:, 1]).all(), (entered, sedan_entered)
    sim = BatchedSim(cm, cfg, spawns=spawns, social_spawns=where)
    assert sim.launch_form() == form
    if table is not None:
        sim.set_traffic_history(table, dims=variant == "history_dims")
    sim.set_agent_entry(ready, chk)
    sim.reset()
    _run_ticks(sim, status, entered, T, A, variant + " " + form, act=torch.full((E, N), -1, dtype=torch.int8, device=sim.device))
    sim.close()


def test_slots_across_the_wavefront(compiled_maps):
    """E = 3, 4 agents + 60 recorded slots — 64 vehicles an env, the most a configuration takes (smx_create refuses more,
    so no env has a social slot at a lane index past the wavefront's 64, and the second turn of k_entry's strided loop over
    the slots cannot be reached from any configuration) — with the one blocker in the last slot, lane 59 of k_entry's
    wavefront: the lanes over the slots and the ballot; the 59 others stand parked far from every start point."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns
    from smarts_amd.traffic_history import TrafficHistoryTable

    envs, social, T = 3, 60, 24
    blocker = social - 1
    N = A + social
    cm = compiled_maps("loop")
    spawns, where = make_spawns(cm, envs, N, episodes=1, seed=31, return_lanes=True)
    ready = np.zeros((1, envs, A), dtype=np.int32)
    ready[0, :, 1] = 2
    # agent 1 of every env starts at the same point (the table is every env's)
    for e in range(envs):
        spawns[0, e * N + 1] = spawns[0, 1]
    chk = _check_rows(spawns, N, A, envs)
    point = chk[0, 0, 1, :2]
    # parked vehicles: lane shape vertices more than 40 m from every agent's start point
    verts = np.concatenate([cm.lane_shape(i) for i in range(cm.n_lanes)])
    starts = chk[0, :, :, :2].reshape(-1, 2)
    far = verts[np.min(np.linalg.norm(verts[:, None, :] - starts[None, :, :], axis=2), axis=1) > 40.0]
    assert len(far) > 0
    res = SimConfig().reset_elapsed_steps()
    F = res + T + 2
    frames = np.zeros((F, social, 4))
    vehicle = np.full((F, social), -1, dtype=np.int32)
    for s in range(social):
        if s == blocker:
            for f in range(F):  # through the point at 6 m/s, there in frame res + 6, a quarter metre aside
                frames[f, s] = (point[0] + 0.25, point[1] + (f - res - 6) * 0.6, 0.0, 6.0)
        else:
            frames[:, s, :2] = far[(s * 7) % len(far)]
        vehicle[:, s] = 100 + s
    table = TrafficHistoryTable(frames, vehicle, 0.1)
    xy = np.broadcast_to(frames[None, res + 1:res + T + 1, :, :2].transpose(1, 0, 2, 3), (T, envs, social, 2))
    alive = np.ones((T, envs, social), dtype=bool)
    status, entered, clearance = ref.run(ready[0], chk[0], xy, alive)
    assert clearance >= CLEARANCE, clearance
    assert ((status[:, :, 1] == ref.BLOCKED).sum(axis=0) >= 2).all() and (entered[:, 1] > 2).all() and (entered[:, 1] < T).all()
    # the case: only the last slot ever comes within reach (the others alone block nobody)
    alone = alive.copy()
    alone[:, :, blocker] = False
    assert not (ref.run(ready[0], chk[0], xy, alone)[0] == ref.BLOCKED).any()
    cfg = SimConfig(num_envs=envs, num_vehicles=N, num_social=social, launch_strategy="small", done_collision=False)
    sim = BatchedSim(cm, cfg, spawns=spawns, social_spawns=where)
    assert sim.launch_form() == "small"
    sim.set_traffic_history(table)
    sim.set_agent_entry(ready, chk)
    sim.reset()
    _run_ticks(sim, status, entered, T, A, "72 slots", act=torch.full((envs, N), -1, dtype=torch.int8, device=sim.device))
    sim.close()


def _far_pair(cm):
    """Two spawn rows on loop more than 100 m apart: agent 1's, and the farthest of sixteen drawn rows from it."""
    from smarts_amd.engine import make_spawns

    rows = make_spawns(cm, 1, 16, episodes=1, seed=41)[0]
    far = max(range(1, 16), key=lambda i: math.hypot(*(rows[i, :2] - rows[0, :2])))
    assert math.hypot(*(rows[far, :2] - np.array(_front(rows[0])))) > 100.0
    return rows[far].copy(), rows[0].copy()


SHIFT_K = 5
SHIFT_J = 15


@pytest.mark.parametrize("space,form", [("Continuous", "small"), ("Lane", "small"), ("TargetPose", "small"),
                                        ("Lane", "large_one_lane"), ("Continuous", "large_teams")])
def test_shifted_episode_identity(space, form, compiled_maps):
    """Agent 1 entering at tick k = 5 (sim A) and at the reset (sim B, nothing bound), with the same actions from its first
    step on: for 15 ticks every output row of agent 1 in A at tick k + j equals B's at tick j bit for bit — the entry
    tick's observation is a first observation (steps 1, distance 0), and the actions A sent it while pending were ignored."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig

    cm = compiled_maps("loop")
    row0, row1 = _far_pair(cm)
    row1[3] = 5.0
    spawns = np.stack([row0, row1])[None]  # one episode, one env
    cfg = SimConfig(num_envs=1, num_vehicles=2, action_space=space, launch_strategy=form, neighbors=True, nb_radius=20.0,
                    ogm=True, ogm_width=64, ogm_height=64, ogm_resolution=50 / 64, lane_ttc=True, done_collision=False,
                    done_off_road=False, done_off_route=False)
    sims = [BatchedSim(cm, cfg, spawns=spawns) for _ in range(2)]
    for s in sims:
        assert s.launch_form() == form
    dev = sims[0].device
    ready = np.array([[[0, SHIFT_K]]], dtype=np.int32)
    chk = np.zeros((1, 1, 2, 3))
    chk[0, 0, 0, :2], chk[0, 0, 1, :2] = _front(row0), _front(row1)
    chk[..., 2] = SEDAN_L
    sims[0].set_agent_entry(ready, chk)
    rng = np.random.default_rng(5)

    def action(j, garbage=False):
        if space == "Lane":
            a = np.array([[int(rng.integers(-1, 4)) if garbage else (0, 1, -1, 0, 2)[j % 5]] * 2], dtype=np.int8)
            return torch.from_numpy(a).to(dev)
        if space == "Continuous":
            a = np.zeros((1, 2, 3), dtype=np.float32)
            a[0, :] = (rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(-1, 1)) if garbage else (0.3, 0.0, 0.1 * math.sin(j))
            return torch.from_numpy(a).to(dev)
        a = np.zeros((1, 2, 4))
        h = row1[2] + 0.02 * j
        for k, r in enumerate((row0, row1)):
            fx, fy = -math.sin(r[2]), math.cos(r[2])
            a[0, k] = (r[0] + fx * (j + 1) * 0.6, r[1] + fy * (j + 1) * 0.6, h, 0.5)
        if garbage:
            a[0, 1] = (1e3, -1e3, 2.0, 0.1)
        return torch.from_numpy(a)

    def step(sim, act):
        return sim.step_target_pose(act) if space == "TargetPose" else sim.step(act)

    def rows(sim):
        torch.cuda.synchronize()
        out = {k: v[:, :, 1].cpu().numpy().copy() if k == "learner" else v[0, 1].cpu().numpy().copy()
               for k, v in sim.out.items() if k not in ("env_done", "entry_status", "entered_tick")}
        out["steps"] = sim.steps[0, 1].item()
        out["state"] = sim.state[:, 0, 1].cpu().numpy().copy()
        return out

    A_, B_ = sims
    A_.reset()
    B_.reset()
    for t in range(1, SHIFT_K):
        step(A_, action(0, garbage=True))  # agent 1 pending: its rows in these ticks are ignored
    step(A_, action(0, garbage=True))  # tick k: agent 1 enters; the action sent for it in this tick is not read
    seen = []
    for j in range(SHIFT_J + 1):
        ra, rb = rows(A_), rows(B_)
        if j == 0:
            assert A_.out["entered_tick"][0, 1].item() == SHIFT_K and ra["steps"] == 1 and ra["dist"] == 0.0
            assert not ra["events"][0] and ra["active"] == 1
        for k in rb:
            assert np.array_equal(ra[k], rb[k], equal_nan=True), (space, form, j, k, ra[k], rb[k])
        seen.append(ra["ego_pos"].copy())
        act = action(j)
        step(A_, act)
        step(B_, act)
    assert np.abs(seen[-1] - seen[0]).max() > 0.5, "agent 1 moved"
    for s in sims:
        s.close()


def _seen_at_entry(cm, parked, form):
    """The scene of test_seen_in_the_entry_tick in one launch form: its checks, and agent 0's neighbour rows, OGM tile,
    events and collidees (and the entrant's) at tick k."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig

    _, row1 = _far_pair(cm)
    row1[3] = 4.25
    front = np.array(_front(row1))
    fx, fy = -math.sin(row1[2]), math.cos(row1[2])
    row0 = row1.copy()
    row0[3] = 0.0
    if not parked:  # 6 m from the start point, straight ahead
        row0[0], row0[1] = front[0] + fx * 6.0, front[1] + fy * 6.0
    spawns = np.stack([row0, row1])[None]
    k = 4
    cfg = SimConfig(num_envs=1, num_vehicles=2, action_space="TargetPose", launch_strategy=form, neighbors=True,
                    nb_radius=20.0, ogm=True, ogm_width=64, ogm_height=64, ogm_resolution=50 / 64, done_collision=False,
                    done_off_road=False, done_off_route=False)
    sim = BatchedSim(cm, cfg, spawns=spawns)
    assert sim.launch_form() == form
    ready = np.array([[[0, k]]], dtype=np.int32)
    chk = np.zeros((1, 1, 2, 3))
    chk[0, 0, 0, :2], chk[0, 0, 1, :2] = _front(row0), front
    chk[..., 2] = SEDAN_L
    sim.set_agent_entry(ready, chk)
    none = torch.full((1, 2, 4), float("nan"), dtype=torch.float64)  # no action: agent 0 stands
    sim.reset()
    ogm = []
    for t in range(1, k + 1):
        sim.step_target_pose(none)
        torch.cuda.synchronize()
        ogm.append(sim.out["ogm"][0, 0].cpu().numpy().copy())
        if t == k - 1:
            assert sim.out["entry_status"][0, 1].item() == nat.ENTRY_PENDING
            assert sim.out["nb_count"][0, 0].item() == 0 and not sim.out["events"][0, 0, nat.EV_COLLISIONS].item()
    assert sim.out["entry_status"][0, 1].item() == nat.ENTRY_ENTERED and sim.out["entered_tick"][0, 1].item() == k
    if parked:
        ev = sim.out["events"][0, :, nat.EV_COLLISIONS].cpu().numpy()
        col = sim.out["collidees"][0].cpu().numpy()
        assert ev.tolist() == [1, 1] and col.tolist() == [2, 1], (form, ev, col)
    else:
        assert sim.out["nb_count"][0, 0].item() == 1 and sim.out["nb_slot"][0, 0, 0].item() == 1
        pos = sim.out["nb_pos"][0, 0, 0].cpu().numpy()
        assert pos[0] == row1[0] and pos[1] == row1[1], (form, pos, row1)
        assert sim.out["nb_speed"][0, 0, 0].item() == np.float32(row1[3])
        assert sim.out["nb_heading"][0, 0, 0].item() == np.float32(row1[2])
        # the entrant's lane as its mate reports it: the entrant stands on a lane centre (its road facts are this tick's)
        assert sim.out["nb_lane_id"][0, 0, 0].item() >= 0 and sim.out["nb_lane_index"][0, 0, 0].item() >= 0, form
        assert np.array_equal(ogm[-2], ogm[-3]), "agent 0 stands: its grid does not change while agent 1 is pending"
        assert (ogm[-1] >= ogm[-2]).all(), "agent 1's arrival only adds cells"
        # the cells whose centres lie inside agent 1's box (a micrometre clear of its edges: the grid draws a cell whose
        # centre lies in the box), in agent 0's frame (ego at the grid's centre, column -> right, row 0 ahead): set at
        # tick k and not at k - 1
        H = W = 64
        res = 50 / 64
        h0, h1 = row0[2], row1[2]
        cols, rows = np.meshgrid(np.arange(W), np.arange(H))
        px, py = (cols + 0.5 - 0.5 * W) * res, (0.5 * H - (rows + 0.5)) * res
        wx = row0[0] + px * math.cos(h0) - py * math.sin(h0)
        wy = row0[1] + px * math.sin(h0) + py * math.cos(h0)
        dx, dy = wx - row1[0], wy - row1[1]
        along, side = -dx * math.sin(h1) + dy * math.cos(h1), dx * math.cos(h1) + dy * math.sin(h1)
        inside = (np.abs(along) <= 0.5 * SEDAN_L - 1e-6) & (np.abs(side) <= 0.5 * 1.47 - 1e-6)
        assert inside.sum() >= 4, inside.sum()
        assert (ogm[-1][inside] > 0).all() and (ogm[-2][inside] == 0).all(), "agent 1's box appears in agent 0's grid"
    torch.cuda.synchronize()
    rows_k = {key: sim.out[key][0, 0].cpu().numpy().copy() for key in sim.out if key.startswith("nb_")}
    rows_k["ogm"] = ogm[-1]
    rows_k["events"] = sim.out["events"][0].cpu().numpy().copy()
    rows_k["collidees"] = sim.out["collidees"][0].cpu().numpy().copy()
    sim.close()
    return rows_k


@pytest.mark.parametrize("parked", [False, True])
def test_seen_in_the_entry_tick(parked, compiled_maps):
    """Agent 0 stands 6 m from agent 1's start point: at tick k - 1 its neighbour row is empty, at tick k it holds agent
    1's spawn pose and speed word for word, its lane, and its OGM has the cells of agent 1's box set that were not.  Parked
    on the start point instead, agent 0 and the entrant both carry the collision event at tick k.  In the small form and
    both forced large ones; the large forms' rows of tick k — agent 0's every neighbour row (nb_lane_id / nb_lane_index
    included), its OGM tile, both agents' events and collidees — equal the small form's bit for bit."""
    cm = compiled_maps("loop")
    small = _seen_at_entry(cm, parked, "small")
    for form in ("large_one_lane", "large_teams"):
        large = _seen_at_entry(cm, parked, form)
        assert set(large) == set(small)
        for key in small:
            assert np.array_equal(large[key], small[key], equal_nan=True), (form, key, large[key], small[key])


def test_episodes(compiled_maps):
    """auto_reset with two spawn / entry rows of different ticks: an env ends only once every agent has entered and
    ended (max_episode_steps counts from each agent's entry), restarts inside the launch with its pending agents pending
    again, and takes the second row's ticks; a masked smx_reset does the same for the envs it names."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps("loop")
    M = 4
    spawns = make_spawns(cm, E, A, episodes=2, seed=51)
    rows = np.array([[0, 2, 2, 5], [0, 1, 4, 0]], dtype=np.int32)
    ready = np.broadcast_to(rows[:, None, :], (2, E, A)).copy()
    chk = np.zeros((2, E, A, 3))
    for r in range(2):
        for e in range(E):
            for a in range(A):
                chk[r, e, a, :2] = _front(spawns[r, e * A + a])
    chk[..., 2] = SEDAN_L
    cfg = SimConfig(num_envs=E, num_vehicles=A, launch_strategy="small", auto_reset=True, max_episode_steps=M,
                    done_collision=False, done_off_road=False, done_off_route=False)
    sim = BatchedSim(cm, cfg, spawns=spawns)
    sim.set_agent_entry(ready, chk)
    sim.reset()
    acts = torch.zeros((E, A), dtype=torch.int8, device=sim.device)
    end1 = int(rows[0].max()) + M - 1  # the last agent enters at 5 and ends M - 1 ticks later
    for t in range(1, end1 + 1):
        sim.step(acts)
        d = _host(sim)
        for a in range(A):
            if t < rows[0, a]:
                assert d["status"][0, a] == nat.ENTRY_PENDING and not d["flags"][0, a] & 1, (t, a)
            elif t == rows[0, a] + M - 1:
                assert d["done"][0, a] == 1, (t, a)  # steps count from the entry
        if t < end1:
            assert not d["env_done"].any(), t  # never ends while an agent is pending (or alive)
    # tick end1 ended every env and restarted it inside the launch: episode 1, row 1
    assert d["env_done"].all() and (sim.env_episode.cpu().numpy() == 1).all()
    want = np.where(rows[1] == 0, nat.ENTRY_ENTERED, nat.ENTRY_PENDING)
    assert (d["status"][:, :A] == want).all() and (d["entered"][:, :A] == np.where(rows[1] == 0, 0, -1)).all(), d["status"]
    for t in range(1, int(rows[1].max()) + 1):
        sim.step(acts)
        d = _host(sim)
        assert (d["entered"][:, :A] == np.where(rows[1] <= t, rows[1], -1)).all(), (t, d["entered"])
    # a masked reset: envs 1 and 3 start episode 2 (row 0 again), envs 0 and 2 keep theirs
    before = _host(sim)
    sim.reset(torch.tensor([0, 1, 0, 1], dtype=torch.uint8))
    d = _host(sim)
    want = np.where(rows[0] == 0, nat.ENTRY_ENTERED, nat.ENTRY_PENDING)
    for e in (1, 3):
        assert (d["status"][e, :A] == want).all() and (d["entered"][e, :A] == np.where(rows[0] == 0, 0, -1)).all()
        assert d["done_count"][e] == 0
    for e in (0, 2):
        assert (d["status"][e] == before["status"][e]).all() and (d["entered"][e] == before["entered"][e]).all()
    sim.close()


def test_guard_parks_an_entrant_with_an_out_of_bounds_spawn(compiled_maps):
    """With the state guard on, an entrant whose spawn row lies out of bounds enters parked, its byte SMX_GUARD_SPAWN, and
    ends (done = 1), as a reset creates such an agent parked and ends it."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cm = compiled_maps("loop")
    spawns = make_spawns(cm, E, A, episodes=1, seed=61)
    edge = max(float(cm.lpg_origin[0]) + float(cm.lpg_cell) * int(cm.lpg_dims[0]),
               float(cm.sg_origin[0]) + float(cm.sg_cell) * int(cm.sg_dims[0]))
    for e in range(E):
        spawns[0, e * A + 2, 0] = edge + 200.0  # 200 m outside the grids, the margin 50 m
    ready = np.zeros((1, E, A), dtype=np.int32)
    ready[0, :, 2] = 3
    chk = _check_rows(spawns, A, A, E)
    cfg = SimConfig(num_envs=E, num_vehicles=A, launch_strategy="small", state_guard=True, state_guard_margin=50.0,
                    done_collision=False, done_off_road=False, done_off_route=False)
    sim = BatchedSim(cm, cfg, spawns=spawns)
    sim.set_agent_entry(ready, chk)
    sim.reset()
    acts = torch.zeros((E, A), dtype=torch.int8, device=sim.device)
    assert (sim.out["guard"][:, 2] == 0).all()  # pending: an absent agent's byte
    for _ in range(3):
        sim.step(acts)
    torch.cuda.synchronize()
    assert (sim.out["entry_status"][:, 2] == nat.ENTRY_ENTERED).all() and (sim.out["entered_tick"][:, 2] == 3).all()
    assert (sim.out["guard"][:, 2] == nat.GUARD_SPAWN).all() and (sim.out["done"][:, 2] == 1).all()
    assert ((sim.flags[:, 2] & 1) == 0).all()
    assert (sim.out["guard"][:, [0, 1, 3]] == 0).all()
    sim.close()


def test_env_layer_delays_agent_b(compiled_maps):
    """HiWayEnv on loop, two agents with start_time 0.1 and 0.7: reset() returns agent A alone; B first appears in step()'s
    dict at the tick entry_ticks gives (8 - 2 = 6); dones["__all__"] waits for both.  Equal start times bind nothing."""
    from smarts_amd.env import Agent, AgentInterface, AgentSpec, AgentType, HiWayEnv
    from smarts_amd.missions import EndlessMission, entry_ticks

    spec = AgentSpec(interface=AgentInterface.from_type(AgentType.Laner, max_episode_steps=9),
                     agent_builder=lambda: Agent.from_function(lambda _: "keep_lane"))
    missions = {"A": EndlessMission(begin=("445633931", 0, 10.0), start_time=0.1),
                "B": EndlessMission(begin=("445633932", 0, 30.0), start_time=0.7)}
    k = entry_ticks(0.7, 0.0, 0.1) - entry_ticks(0.1, 0.0, 0.1)
    assert k == 6
    env = HiWayEnv(scenarios=["scenarios/loop"], agent_specs={"A": spec, "B": spec}, seed=3, missions=missions)
    obs = env.reset()
    assert set(obs) == {"A"}
    assert env._core.sim.agent_entry is not None and env._core.cfg.reset_elapsed_steps() == 2
    seen_b, all_done_at = None, None
    for t in range(1, 30):
        obs, rew, done, info = env.step({a: "keep_lane" for a in obs})
        if "B" in obs and seen_b is None:
            seen_b = t
        if t < k:
            assert "B" not in obs and "B" not in done
        if done["__all__"]:
            all_done_at = t
            break
    assert seen_b == k
    # A ends at tick 8 (max_episode_steps 9, reset observation step 1); B at k + 8: __all__ waits for it
    assert all_done_at == k + 8, all_done_at
    env.close()
    same = HiWayEnv(scenarios=["scenarios/loop"], agent_specs={"A": spec, "B": spec}, seed=3,
                    missions={"A": EndlessMission(begin=("445633931", 0, 10.0), start_time=0.7),
                              "B": EndlessMission(begin=("445633932", 0, 30.0), start_time=0.7)})
    assert set(same.reset()) == {"A", "B"}
    assert same._core.sim.agent_entry is None and "entry_status" not in same._core.sim.out
    same.close()

"""The state guard on the device (include/smx.h smx_set_guard; smarts_amd/csrc/smx_guard.h), through BatchedSim.

Loop map, E = 4 envs x N = 4 agents: two env groups' worth where a kernel packs envs per wavefront, slot 0 and the last
slot among the offenders.  No case hands the device an input that would be dangerous without a guard: the box cases use
margin = 50 m and points 200 m outside the map's grids (an ordinary off-road vehicle when the guard is off), and the one
not-finite case runs last, only after every other case of this file has passed in this process.  The exhaustive per-word
coverage of the test itself is the host program's (tests/test_host_guard.py).

Every comparison is exact (torch.equal, NaNs equal): the guard computes nothing, it only decides what is stored.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, N = 4, 4
MARGIN = 50.0
FORMS = ("small", "large_one_lane", "large_teams")
OUTSIDE = 200.0  # metres beyond the grids' extent
STATE_ROWS = 14  # SMX_S_X .. SMX_S_MCL_Y: the vehicle and controller words a control kernel stores
_passed = set()  # the cases of tests 1-3 that passed in this process (the not-finite case asks)
_EXPECTED = 9 + 3 + 3 + 3


def _require_guard():
    from smarts_amd.engine import BatchedSim

    assert hasattr(BatchedSim, "bind_guard"), "this build has no state guard (smx_set_guard / BatchedSim.bind_guard)"


def _grid_edge_x(cm):
    """The union of the two grids' extents, high x edge (the guard box's before it is grown)."""
    return max(float(cm.lpg_origin[0]) + float(cm.lpg_cell) * int(cm.lpg_dims[0]),
               float(cm.sg_origin[0]) + float(cm.sg_cell) * int(cm.sg_dims[0]))


def _sim(cm, space, guard, form, spawns=None, n=N, auto_reset=False, episodes=1):
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cfg = SimConfig(num_envs=E, num_vehicles=n, action_space=space, launch_strategy=form, neighbors=True,
                    done_collision=False, done_off_road=False, done_off_route=False, auto_reset=auto_reset,
                    state_guard=guard, state_guard_margin=MARGIN)
    if spawns is None:
        spawns = make_spawns(cm, E, n, episodes=episodes, seed=5)
    return BatchedSim(cm, cfg, spawns=spawns)


def _snapshot(sim):
    """Every state buffer and every output of the last pass (but the guard byte itself), cloned."""
    import torch

    torch.cuda.synchronize()
    snap = {"out." + k: v.clone() for k, v in sim.out.items() if k != "guard"}
    for name in ("state", "flags", "steps", "env_ticks", "env_done_count", "env_episode", "driven_path", "seed_cache",
                 "facts_i32", "facts_f64", "env_reset_pending"):
        t = getattr(sim, name)
        if t is not None:
            snap["st." + name] = t.clone()
    return snap


def _env_axis(key, t):
    """The tensor with the env axis first ([E, ...])."""
    if key == "out.learner":  # [2, E, N]
        return t.transpose(0, 1)
    if key in ("st.state", "st.seed_cache", "st.facts_i32", "st.facts_f64"):  # [rows, E, N]
        return t.transpose(0, 1)
    if key == "st.driven_path":  # [E * N, ring]
        return t.reshape(E, -1)
    return t


def _assert_same(a, b, envs=range(E), what=""):
    import torch

    assert sorted(a) == sorted(b)
    idx = torch.tensor(list(envs), device=next(iter(a.values())).device)
    for k in a:
        x, y = _env_axis(k, a[k]).index_select(0, idx), _env_axis(k, b[k]).index_select(0, idx)
        ne = x != y
        if x.is_floating_point():
            ne &= ~(x.isnan() & y.isnan())
        assert not bool(ne.any()), (what, k, "envs", list(envs), int(ne.sum()), "elements differ")


def _actions(sim, space, rng):
    """One tick's actions of a run with nothing out of bounds (the same for the two sims of a pair: same seed)."""
    import torch

    from smarts_amd import _native as nat

    n = sim.N
    if space == "Lane":
        return torch.from_numpy(rng.integers(0, 4, size=(E, n)).astype(np.int8))
    if space == "Continuous":
        a = np.zeros((E, n, 3), dtype=np.float32)
        a[..., 0] = 0.4
        a[..., 2] = rng.uniform(-0.1, 0.1, size=(E, n))
        return torch.from_numpy(a)
    # TargetPose: a metre ahead of where the vehicle stands, one tick from now
    torch.cuda.synchronize()
    x, y, h = (sim.state[nat.S[k]].cpu().numpy() for k in ("X", "Y", "HEADING"))
    t = np.stack([x - np.sin(h), y + np.cos(h), h, np.full_like(x, sim.cfg.dt)], axis=-1)
    return torch.from_numpy(np.ascontiguousarray(t))


def _step(sim, space, actions):
    return sim.step_target_pose(actions) if space == "TargetPose" else sim.step(actions)


def _pair(cm, space, form, **kw):
    on, off = _sim(cm, space, True, form, **kw), _sim(cm, space, False, form, **kw)
    assert "guard" in on.out and "guard" not in off.out
    on.reset(), off.reset()
    return on, off


def _run_pair(on, off, space, ticks, seed=3):
    r1, r2 = np.random.default_rng(seed), np.random.default_rng(seed)
    for _ in range(ticks):
        _step(on, space, _actions(on, space, r1))
        _step(off, space, _actions(off, space, r2))


def _parked(cm):
    return float(cm.lp_x[0]), float(cm.lp_y[0]), float(cm.lp_heading[0])


def _rows(sim, e, i):
    import torch

    torch.cuda.synchronize()
    return sim.state[:STATE_ROWS, e, i].clone()


def _assert_parked(sim, cm, e, i, kinematic=False):
    from smarts_amd import _native as nat

    rows = _rows(sim, e, i).cpu().numpy()
    px, py, ph = _parked(cm)
    want = np.zeros(STATE_ROWS)
    want[nat.S["X"]], want[nat.S["Y"]], want[nat.S["HEADING"]] = px, py, ph
    if kinematic:
        want[nat.S["DELTA"]] = ph  # SMX_S_KIN_RAW_HEADING
    assert np.array_equal(rows, want), (rows, want)
    f = int(sim.flags[e, i])
    assert (f & nat.F_GUARDED) and not (f & nat.F_MCL_SET)


def _finite_where_it_was(before, after, what):
    for k, v in after.items():
        if k.startswith("out.") and v.is_floating_point():
            worse = ~v.isfinite() & before[k].isfinite()
            assert not bool(worse.any()), (what, k, int(worse.sum()), "elements are no longer finite")


# ---------------------------------------------------------------------------------------------- 1. transparent
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("space", ("Lane", "Continuous", "TargetPose"))
def test_guard_on_changes_nothing_while_everything_is_in_bounds(compiled_maps, space, form, request):
    _require_guard()
    cm = compiled_maps("loop")
    on, off = _pair(cm, space, form)
    _assert_same(_snapshot(on), _snapshot(off), what="reset")
    assert int(on.out["guard"].sum()) == 0
    _run_pair(on, off, space, 10)
    _assert_same(_snapshot(on), _snapshot(off), what=f"{space} {form} after 10 ticks")
    assert int(on.out["guard"].sum()) == 0
    assert bool(on.out["active"].any())  # (the run was a run: agents are still driving)
    _passed.add(request.node.name)


# ---------------------------------------------------------------------------------------------- 2. STEP, kinematic
@pytest.mark.parametrize("form", FORMS)
def test_a_target_outside_the_box_holds_the_vehicle_and_ends_the_agent(compiled_maps, form, request):
    import torch

    from smarts_amd import _native as nat

    _require_guard()
    cm = compiled_maps("loop")
    on, off = _pair(cm, "TargetPose", form)
    _run_pair(on, off, "TargetPose", 2)
    before = _snapshot(on)
    held = {(1, 0): _rows(on, 1, 0), (1, 3): _rows(on, 1, 3)}
    acts = []
    for sim in (on, off):
        a = _actions(sim, "TargetPose", np.random.default_rng(0))
        for (e, i) in held:
            a[e, i, 0] = _grid_edge_x(cm) + OUTSIDE  # seconds = dt: the provider would place the vehicle there this tick
        acts.append(a)
    assert torch.equal(acts[0], acts[1])
    on.step_target_pose(acts[0]), off.step_target_pose(acts[1])
    after = _snapshot(on)
    guard = on.out["guard"].cpu().numpy()
    want = np.zeros((E, N), dtype=np.uint8)
    for (e, i), rows in held.items():
        want[e, i] = nat.GUARD_STEP
        assert torch.equal(_rows(on, e, i), rows), ("state rows of a held vehicle", e, i)
        assert int(on.out["done"][e, i]) == 1 and int(on.out["active"][e, i]) == 0
        f = int(on.flags[e, i])
        assert (f & nat.F_GUARDED) and not (f & nat.F_ALIVE)
        # guard off: the ordinary off-road vehicle the same action makes
        assert float(off.state[nat.S["X"], e, i]) == _grid_edge_x(cm) + OUTSIDE
    assert np.array_equal(guard, want), guard
    others = on.out["done"].cpu().numpy().astype(bool)
    others[1, 0] = others[1, 3] = False
    assert not others.any()
    _finite_where_it_was(before, after, form)
    _assert_same(after, _snapshot(off), envs=(0, 2, 3), what=f"TargetPose {form}: the other envs")
    on.sync()  # what smx_sync reports is unchanged: a finite target is no "bad target pose"
    # the next tick: the agents are gone like any done agent, their bytes read 0 again
    _run_pair(on, off, "TargetPose", 1)
    assert int(on.out["guard"].sum()) == 0 and int(on.out["done"][1, 0]) == 0 and int(on.out["active"][1, 0]) == 0
    _assert_same(_snapshot(on), _snapshot(off), envs=(0, 2, 3), what=f"TargetPose {form}: the tick after")
    _passed.add(request.node.name)


# ---------------------------------------------------------------------------------------------- 3. STATE and SPAWN by the box
@pytest.mark.parametrize("form", FORMS)
def test_a_state_written_outside_the_box_is_parked_and_ends_the_agent(compiled_maps, form, request):
    from smarts_amd import _native as nat

    _require_guard()
    cm = compiled_maps("loop")
    on, off = _pair(cm, "Lane", form)
    _run_pair(on, off, "Lane", 2)
    for sim in (on, off):
        sim.state[nat.S["X"], 2, 1] = _grid_edge_x(cm) + OUTSIDE
    before = _snapshot(on)
    _run_pair(on, off, "Lane", 1, seed=8)
    want = np.zeros((E, N), dtype=np.uint8)
    want[2, 1] = nat.GUARD_STATE
    assert np.array_equal(on.out["guard"].cpu().numpy(), want)
    _assert_parked(on, cm, 2, 1)
    assert int(on.out["done"][2, 1]) == 1 and int(on.out["active"][2, 1]) == 0 and not (int(on.flags[2, 1]) & nat.F_ALIVE)
    px, py, _ = _parked(cm)
    pos = on.out["ego_pos"][2, 1].cpu().numpy()
    assert pos[0] == px and pos[1] == py  # the observation is built from the parked pose
    after = _snapshot(on)
    _finite_where_it_was(before, after, form)
    _assert_same(after, _snapshot(off), envs=(0, 1, 3), what=f"Lane {form}: the other envs")
    _passed.add(request.node.name)


@pytest.mark.parametrize("form", FORMS)
def test_a_spawn_row_outside_the_box_creates_the_vehicle_parked(compiled_maps, form, request):
    from smarts_amd import _native as nat
    from smarts_amd.engine import make_spawns

    _require_guard()
    cm = compiled_maps("loop")
    spawns = make_spawns(cm, E, N, episodes=1, seed=5)
    spawns[0, 3 * N + 3, 0] = _grid_edge_x(cm) + OUTSIDE
    on, off = _pair(cm, "Lane", form, spawns=spawns)
    want = np.zeros((E, N), dtype=np.uint8)
    want[3, 3] = nat.GUARD_SPAWN
    assert np.array_equal(on.out["guard"].cpu().numpy(), want)
    _assert_parked(on, cm, 3, 3)
    assert int(on.out["done"][3, 3]) == 0 and int(on.out["active"][3, 3]) == 1  # reset passes report no done
    assert int(on.flags[3, 3]) & nat.F_ALIVE
    _assert_same(_snapshot(on), _snapshot(off), envs=(0, 1, 2), what=f"reset {form}: the other envs")
    _run_pair(on, off, "Lane", 1)
    assert np.array_equal(on.out["guard"].cpu().numpy(), want)  # SPAWN still
    assert int(on.out["done"][3, 3]) == 1 and int(on.out["active"][3, 3]) == 0 and not (int(on.flags[3, 3]) & nat.F_ALIVE)
    _assert_parked(on, cm, 3, 3)  # held where it was parked
    _assert_same(_snapshot(on), _snapshot(off), envs=(0, 1, 2), what=f"first step {form}: the other envs")
    _passed.add(request.node.name)


# ---------------------------------------------------------------------------------------------- 4. auto_reset
def test_an_env_whose_agents_are_all_guarded_restarts_inside_the_launch(compiled_maps):
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import make_spawns

    _require_guard()
    cm = compiled_maps("loop")
    spawns = make_spawns(cm, E, 2, episodes=2, seed=5)
    sim = _sim(cm, "TargetPose", True, "small", spawns=spawns, n=2, auto_reset=True)
    sim.reset()
    rng = np.random.default_rng(1)
    for _ in range(2):
        sim.step_target_pose(_actions(sim, "TargetPose", rng))
    torch.cuda.synchronize()
    episode = sim.env_episode.cpu().numpy().copy()
    held = sim.state[:, 2, :].clone()
    a = _actions(sim, "TargetPose", rng)
    a[2, :, 0] = _grid_edge_x(cm) + OUTSIDE
    out = sim.step_target_pose(a)
    torch.cuda.synchronize()
    assert out["env_done"].cpu().numpy().tolist() == [0, 0, 1, 0]
    assert out["done"][2].cpu().numpy().tolist() == [1, 1]  # the finishing tick's, kept
    now = sim.env_episode.cpu().numpy()
    assert now[2] == episode[2] + 1 and (np.delete(now, 2) == np.delete(episode, 2)).all()
    # the first observation of the new episode
    assert int(out["guard"].sum()) == 0
    flags = sim.flags[2].cpu().numpy()
    assert ((flags & nat.F_ALIVE) != 0).all() and ((flags & nat.F_GUARDED) == 0).all()
    assert out["active"][2].cpu().numpy().tolist() == [1, 1]
    row = spawns[int(now[2]) % 2].reshape(E, 2, 4)[2]
    assert np.array_equal(out["ego_pos"][2, :, :2].cpu().numpy(), row[:, :2])
    # final_*: the finishing tick's rows, built from the held poses
    assert torch.equal(out["final_ego_pos"][2, :, 0], held[nat.S["X"]]) and torch.equal(out["final_ego_pos"][2, :, 1], held[nat.S["Y"]])
    # (finite wherever an undisturbed kinematic agent's row is: steering reads NaN for a BoxChassis, include/smx.h)
    assert bool((out["final_ego_f32"][2].isfinite() | ~out["ego_f32"][0].isfinite()).all())
    assert bool(out["final_dist"][2].isfinite().all())


# ---------------------------------------------------------------------------------------------- 5. not finite (last)
def test_a_nan_in_the_state_is_parked_like_a_pose_outside_the_box(compiled_maps):
    import torch

    from smarts_amd import _native as nat

    _require_guard()
    if len(_passed) < _EXPECTED:
        pytest.skip(f"runs only after the box cases of this file have passed in this process ({len(_passed)} of {_EXPECTED} did)")
    cm = compiled_maps("loop")
    sim = _sim(cm, "Lane", True, "small")
    sim.reset()
    rng = np.random.default_rng(2)
    for _ in range(2):
        sim.step(_actions(sim, "Lane", rng))
    sim.state[nat.S["R"], 1, 2] = float("nan")
    out = sim.step(_actions(sim, "Lane", rng))
    torch.cuda.synchronize()
    want = np.zeros((E, N), dtype=np.uint8)
    want[1, 2] = nat.GUARD_STATE
    assert np.array_equal(out["guard"].cpu().numpy(), want)
    _assert_parked(sim, cm, 1, 2)
    assert int(out["done"][1, 2]) == 1 and int(out["active"][1, 2]) == 0
    for k, v in out.items():
        if v.is_floating_point():
            assert bool(v.isfinite().all()), k
    assert bool(sim.state.isfinite().all())

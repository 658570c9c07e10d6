"""History agents on the device (include/smx.h smx_set_history_agents; BatchedSim.set_history_agents /
step_history_agents): agent slots that follow recorded vehicles of the bound traffic history.

The scene and the rules restated in NumPy are tests/history_agents_ref.py's: E = 4 envs, 3 agent slots and 3 replayed
slots each, 30 ticks, on ``loop`` and ``4lane``, in the small form and in the forced large form."""
import ctypes as C
import math

import numpy as np
import pytest

import history_agents_ref as ref
import mpc_imitation_ref as imit
import parity
from smarts_amd import _native as nat

pytestmark = pytest.mark.gpu

E, A, S, N = ref.E, ref.AGENTS, ref.SLOTS, ref.N
T = 30
DT = ref.DT
S_ = nat.S
FORMS = ("small", "large")
MAPS = ("loop", "4lane")
QUIET = dict(done_collision=False, done_off_road=False, done_off_route=False, done_on_shoulder=False, done_wrong_way=False)


def _sim(cm, sc, action_space="Imitation", spawns=None, **cfg_kw):
    from smarts_amd.engine import BatchedSim, SimConfig

    kw = dict(num_envs=E, num_vehicles=N, num_social=S, dt=DT, action_space=action_space, neighbors=True, nb_radius=60.0)
    kw.update(QUIET)
    kw.update(cfg_kw)
    episodes = 2
    spawns = np.tile(sc["spawns"], (episodes, E, 1)) if spawns is None else spawns
    social = np.tile(sc["social_spawns"], (episodes, E, 1))
    return BatchedSim(cm, SimConfig(**kw), spawns=spawns, social_spawns=social)


def _bound(cm, starts=ref.STARTS, follow=ref.FOLLOW, replaced=ref.REPLACED, expert_actions=True, **cfg_kw):
    """(sim, scene, model): an Imitation sim with the scene's history and the follow table bound."""
    import torch

    sc = ref.scene(cm)
    sim = _sim(cm, sc, **cfg_kw)
    st = torch.from_numpy(np.ascontiguousarray(starts)).cuda()
    rp = torch.from_numpy(np.ascontiguousarray(replaced)).cuda() if replaced is not None else None
    sim.set_traffic_history(sc["table"], st, rp)
    sim.set_history_agents(torch.from_numpy(np.ascontiguousarray(follow)).cuda(), expert_actions=expert_actions)
    return sim, sc, ref.Model(sc["table"], starts, follow, sim.cfg.reset_elapsed_steps())


def _host(sim):
    import torch

    torch.cuda.synchronize()
    st = sim.state.cpu().numpy()
    words = np.stack([st[S_[w]] for w in ("X", "Y", "HEADING", "U")], axis=-1)  # [E, N, 4]
    return st, words, sim.flags.cpu().numpy()


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _check_against_model(sim, m, replaced, where, before=None, left=None):
    """After a pass, everything rule 1-4 fix: the followers' words bit for bit, _last_heading / _last_dt, status,
    SMX_F_ALIVE, the expert action, the done count, and the social slots' presence with the twins hidden."""
    st, words, flags = _host(sim)
    status = sim.out["history_agent_status"].cpu().numpy()
    action = sim.out["expert_action"].cpu().numpy()
    assert np.array_equal(sim.env_episode.cpu().numpy(), m.episode), (where, sim.env_episode, m.episode)
    assert np.array_equal(sim.env_ticks.cpu().numpy(), m.ticks), where
    assert np.array_equal(status[:, :A], m.status), (where, status[:, :A], m.status)
    assert np.array_equal((flags[:, :A] & nat.F_ALIVE) != 0, m.alive), (where, flags[:, :A], m.alive)
    assert not (flags[:, :A] & nat.F_SOCIAL).any()
    assert np.array_equal(sim.env_done_count.cpu().numpy(), m.done_count), (where, sim.env_done_count, m.done_count)
    following = m.status == nat.HA_FOLLOWING
    got, want = words[:, :A][following], m.row[following]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (where, got, want)  # the table, bit for bit
    fresh = m.last_dt == 0.0
    assert np.array_equal(st[S_["SPD_INT"]][:, :A][following], m.last_dt[following]), where  # _last_dt: dt, 0 after a reset
    moved = following & ~fresh
    assert np.array_equal(st[S_["LAT_INT"]][:, :A][moved].view(np.uint64), m.last_heading[moved].view(np.uint64)), where
    assert np.array_equal(st[S_["DELTA"]][:, :A][following & fresh], m.row[..., 2][following & fresh]), where  # KIN_RAW_HEADING at a reset
    # the expert action: NaN exactly where rule 4 says, else the float32 rounding within 1 ulp (+ 4 x 2^-51 / dt on the
    # wrapped heading difference, the bound tests/test_gpu_imitation.py derives); third word 0; social rows never written
    act = action[:, :A]
    assert np.array_equal(np.isnan(act[..., :2]), np.isnan(m.action)), (where, act, m.action)
    assert (act[..., 2] == 0).all() and np.isnan(action[:, A:, :2]).all()
    ok = ~np.isnan(m.action[..., 0])
    w32 = m.action.astype(np.float32).astype(np.float64)
    err = np.abs(act[..., :2].astype(np.float64) - w32)
    tol = _ulp32(w32) + np.array([0.0, 4 * 2.0 ** -51 / DT])
    assert (err[ok] <= tol[ok]).all(), (where, float(err[ok].max()))
    # a follower that left this tick: nothing of its state was stored
    # (the vehicle's own words; the sensors' words — trip meter, accelerometer — go on with the leaving tick's observation)
    if left is not None and left.any():
        for w in ("X", "Y", "HEADING", "U", "DELTA", "LAT_INT", "SPD_INT", "PREV_X", "PREV_Y"):
            assert np.array_equal(st[S_[w]][:, :A][left].view(np.uint64), before[S_[w]][:, :A][left].view(np.uint64)), (where, w)
    # social slots: SMX_F_ALIVE was decided by this pass's commit for the coming frame; present slots hold their rows
    for e in range(E):
        coming = m.social_present(e, replaced, ahead=1)
        assert np.array_equal((flags[e, A:] & nat.F_ALIVE) != 0, coming), (where, e, flags[e, A:], coming)
        now = m.social_present(e, replaced)
        f = m.frame(e)
        for k in np.nonzero(now)[0]:
            assert np.array_equal(words[e, A + k].view(np.uint64), m.table.frames[f, k].view(np.uint64)), (where, e, k)
    return st


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MAPS)
def test_followers_hold_the_table_bit_for_bit(name, form, compiled_maps):
    """Checks 1 and 3 (without auto_reset) and the NaN / ulp half of 4, in every tick of the run: the table's words,
    the twins hidden (`replaced` still hiding its vehicle), leaving — state untouched, done = 1, active = 0, LEFT, the
    done count up by one —, never entering — not alive from the reset, ABSENT, counted — and the env that follows nothing
    done after its first tick."""
    cm = compiled_maps(name)
    sim, sc, m = _bound(cm, launch_strategy=form)
    assert (sim.launch_form() == "small") == (form == "small")
    table = sc["table"]
    out = sim.reset()
    m.reset()
    st = _check_against_model(sim, m, ref.REPLACED, "reset")
    d = parity.host(out)
    act, done = d["active"].reshape(E, N), d["done"].reshape(E, N)
    assert np.array_equal(act[:, :A] != 0, m.alive) and not done.any() and not act[:, A:].any()
    # an agent that did not enter reads as an absent agent: zeros, lane ids -1
    gone = ~m.alive
    assert not d["ego_pos"].reshape(E, N, 3)[:, :A][gone].any() and not d["ego_f32"].reshape(E, N, -1)[:, :A][gone].any()
    assert (d["ego_lane"].reshape(E, N, 2)[:, :A][gone] == -1).all() and (d["nb_count"].reshape(E, N)[:, :A][gone] == 0).all()
    # the slot of a followed id is not alive in the env that follows it and alive in one that does not
    slot = lambda v: int(np.nonzero((table.vehicle == v).any(axis=0))[0][0])  # noqa: E731
    flags = sim.flags.cpu().numpy()
    assert not flags[0, A + slot(ref.LEAVER)] & nat.F_ALIVE and flags[1, A + slot(ref.LEAVER)] & nat.F_ALIVE
    assert not flags[1, A + slot(ref.STANDING)] & nat.F_ALIVE and flags[0, A + slot(ref.STANDING)] & nat.F_ALIVE
    assert not flags[3, A + slot(ref.STANDING)] & nat.F_ALIVE  # ... hidden by `replaced`
    collided = np.zeros((E, A), dtype=bool)
    lefts = 0
    for t in range(T):
        before = st
        was_alive = m.alive.copy()
        count_before = m.done_count.copy()
        out = sim.step_history_agents()
        left, env_done = m.step()
        st = _check_against_model(sim, m, ref.REPLACED, f"{name} {form} t{t}", before, left)
        d = parity.host(out)
        act, done = d["active"].reshape(E, N)[:, :A], d["done"].reshape(E, N)[:, :A]
        assert np.array_equal(done != 0, left), (t, done, left)  # done in the leaving tick, and only there
        assert np.array_equal(act != 0, m.alive), t
        assert np.array_equal(m.done_count - count_before, left.sum(axis=1))
        assert np.array_equal(out["env_done"].cpu().numpy() != 0, env_done), (t, env_done)
        assert env_done.tolist() == [False, False, True, False]  # the env that follows nothing: done from its first tick on
        # the leaving tick's observation is built from the held pose
        ego = d["ego_pos"].reshape(E, N, 3)[:, :A]
        assert np.array_equal(ego[left][:, :2], np.stack([before[S_["X"]][:, :A][left], before[S_["Y"]][:, :A][left]], axis=-1))
        observed = was_alive & ~left
        assert np.array_equal(ego[observed][:, :2], m.row[observed][:, :2])
        collided |= d["events"].reshape(E, N, -1)[:, :A, nat.EV_COLLISIONS].astype(bool)
        lefts += int(left.sum())
        assert not d["active"].reshape(E, N)[:, A:].any() and not d["done"].reshape(E, N)[:, A:].any()
    assert lefts == 2
    # the driver's follower ran into the standing vehicle where that is a social vehicle; not where `replaced` hides it;
    # and where another agent follows it, that agent is what it hits
    assert collided[0].tolist() == [True, False, False] and collided[1].tolist() == [True, True, False] and not collided[3].any()
    sim.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MAPS)
def test_auto_reset_restarts_from_the_next_rows(name, form, compiled_maps):
    """Check 3 under auto_reset: an env restarts once all its present agents are done (the one that follows nothing after
    its first tick) and episode k uses row k mod 2 of start_frames, replaced and the follow table."""
    cm = compiled_maps(name)
    starts = np.array([[24, 33, 1, 31], [3, 0, 5, 30]], dtype=np.int32)  # (windows that run off the table's end within the run)
    sim, sc, m = _bound(cm, starts=starts, launch_strategy=form, auto_reset=True)
    sim.reset()
    m.reset()
    st = _check_against_model(sim, m, ref.REPLACED, "reset")
    restarts = np.zeros(E, dtype=int)
    for t in range(T):
        episode = m.episode.copy()
        out = sim.step_history_agents()
        left, env_done = m.step(auto_reset=True)
        # (a restarted env's rows are its new episode's: the `left` rows of the finishing tick are gone with it)
        st = _check_against_model(sim, m, ref.REPLACED, f"{name} {form} t{t}", st, left & ~env_done[:, None])
        assert np.array_equal(out["env_done"].cpu().numpy() != 0, env_done), (t, env_done)
        restarts += m.episode - episode
    assert (restarts >= 1).all() and restarts[2] >= 1 and restarts[3] >= 2, restarts  # every env went through row 1; env 3 and back
    sim.close()


def _nan_safe(d, o, keep):
    """The rows `keep` of two sims' host outputs with the NaNs both hold in the same places (the BoxChassis' steering, the
    yaw rate of a fresh vehicle) replaced by zeros, for parity.compare."""
    a, b = {}, {}
    for k in o:
        if d[k].shape[0] != keep.shape[0]:
            continue  # (the learner block: not a per-vehicle row)
        x, y = d[k][keep], o[k][keep]
        if x.dtype.kind == "f":
            nx, ny = np.isnan(x), np.isnan(y)
            assert np.array_equal(nx, ny), k
            x, y = np.where(nx, 0, x), np.where(ny, 0, y)
        a[k], b[k] = x, y
    return a, b


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MAPS)
def test_twin_against_trajectory_with_time(name, form, compiled_maps):
    """Check 2, the whole observation: a TrajectoryWithTime sim whose table lacks the followed vehicles, whose agents are
    spawned on their rows and steered on to each next row with a two-column trajectory t = (dt, 2 dt) (interpolation
    ratio exactly 0: x, y, speed land exactly, the heading to an ulp or two of atan2(sin, cos)).  While every follower
    follows, every dense row of every follower agrees at tests/test_gpu_traffic_history.py's tolerances — OGM 64 x 64 and
    the collision with the standing vehicle included.  Agent 2 follows nothing in every env; its twin stands far away
    (the scene's spawn rows: farther than the neighbourhood radius and the grid's reach) without an action."""
    import torch

    cm = compiled_maps(name)
    follow = np.array([[[ref.DRIVER, ref.LEAVER, -1]] * E], dtype=np.int32)
    starts = np.array([[0, 2, 4, 1]], dtype=np.int32)
    replaced = np.array([[-1, -1, -1, ref.STANDING]], dtype=np.int32)
    grid = dict(ogm=True, ogm_width=64, ogm_height=64, ogm_resolution=50 / 64, launch_strategy=form)
    sim, sc, m = _bound(cm, starts=starts, follow=follow, replaced=replaced, **grid)
    table = sc["table"]
    assert sc["far"] > 80.0  # (beyond the neighbourhood radius, 60 m, and the grid's reach, 36 m)
    res = sim.cfg.reset_elapsed_steps()
    spawns = np.tile(sc["spawns"], (2, E, 1))
    for e in range(E):
        for a in range(2):
            spawns[:, e * N + a] = table.spawn_of(int(follow[0, e, a]), int(starts[0, e]) + res)
    twin = _sim(cm, sc, action_space="TrajectoryWithTime", spawns=spawns, **grid)
    twin.set_traffic_history(ref.blanked(table, (ref.DRIVER, ref.LEAVER)), torch.from_numpy(starts).cuda(), torch.from_numpy(replaced).cuda())
    keep = np.zeros((E, N), dtype=bool)
    keep[:, :2] = True
    keep = keep.reshape(-1)
    d, o = parity.host(sim.reset()), parity.host(twin.reset())
    m.reset()
    bad = parity.compare(*_nan_safe(d, o, keep), tol64=1e-9, tol32=2e-6, where="reset ")
    assert bad == [], "\n".join(bad)
    ticks = ref.LEAVER_LAST - (int(starts.max()) + res)  # while the leaver is there in every env
    assert ticks >= 10
    collided = np.zeros(E, dtype=bool)
    for t in range(ticks):
        traj = np.zeros((E, N, 5, 2))
        counts = np.zeros((E, N), dtype=np.int32)
        for e in range(E):
            for a in range(2):
                row = table.spawn_of(int(follow[0, e, a]), m.frame(e) + 1)
                traj[e, a, 0] = (DT, 2 * DT)
                traj[e, a, 1:, 0] = row
                traj[e, a, 1:, 1] = row
                counts[e, a] = 2
        d = parity.host(sim.step_history_agents())
        o = parity.host(twin.step_trajectory_with_time(torch.from_numpy(traj), torch.from_numpy(counts)))
        left, _ = m.step()
        assert not left.any()
        bad = parity.compare(*_nan_safe(d, o, keep), tol64=1e-9, tol32=2e-5, where=f"{name} {form} t{t} ")
        assert bad == [], "\n".join(bad)
        collided |= d["events"].reshape(E, N, -1)[:, 0, nat.EV_COLLISIONS].astype(bool)
    twin.sync()
    assert set(d) >= {"ego_pos", "ego_f32", "wp_pos", "nb_pos", "events", "reward", "ogm"}
    assert d["ogm"].reshape(E, N, -1)[:, 0].any()
    assert collided.tolist() == [True, True, True, False]
    sim.close()
    twin.close()


@pytest.mark.parametrize("name", MAPS)
def test_expert_actions_close_the_loop(name, compiled_maps):
    """Check 4, device to device: a plain Imitation sim (no binding, the same spawn rows) fed out["expert_action"] tick
    by tick keeps the recorded heading and speed.  Bound, from the data: per tick |label| x 2^-24 x dt for the label's
    rounding to float32, plus the project's 1e-9 per tick, summed over the run."""
    import torch

    cm = compiled_maps(name)
    follow = np.array([[[ref.DRIVER, ref.LEAVER, ref.STANDING]] * E], dtype=np.int32)
    starts = np.array([[0, 1, 3, 5]], dtype=np.int32)
    sim, sc, m = _bound(cm, starts=starts, follow=follow, replaced=None)
    table = sc["table"]
    res = sim.cfg.reset_elapsed_steps()
    spawns = np.tile(sc["spawns"], (2, E, 1))
    for e in range(E):
        for a in range(A):
            spawns[:, e * N + a] = table.spawn_of(int(follow[0, e, a]), int(starts[0, e]) + res)
    plain = _sim(cm, sc, spawns=spawns)
    sim.reset()
    plain.reset()
    m.reset()
    bound = np.zeros((E, A, 2))
    ticks = ref.LEAVER_LAST - (int(starts.max()) + res)
    worst = 0.0
    for t in range(ticks):
        label = sim.out["expert_action"].clone()
        assert not torch.isnan(label[:, :A]).any()
        plain.step(label)
        sim.step_history_agents()
        m.step()
        lab = label[:, :A, :2].cpu().numpy().astype(np.float64)
        bound += np.abs(lab[..., ::-1]) * 2.0 ** -24 * DT + 1e-9  # (heading, speed) <- (angular velocity, acceleration)
        st, words, _ = _host(plain)
        got = words[:, :A, 2:4]
        err_h = np.abs((got[..., 0] - m.row[..., 2] + math.pi) % (2 * math.pi) - math.pi)
        err_u = np.abs(got[..., 1] - m.row[..., 3])
        worst = max(worst, float(err_h.max()), float(err_u.max()))
        assert (err_h <= bound[..., 0]).all() and (err_u <= bound[..., 1]).all(), (t, err_h.max(), err_u.max(), bound.min())
    print(f"closed loop {name}: worst heading / speed difference over {ticks} ticks {worst:.3g}, bound {bound.min():.3g}")
    plain.sync()
    sim.close()
    plain.close()


@pytest.mark.parametrize("form", FORMS)
def test_hand_over_and_back(form, compiled_maps):
    """Check 5: five following ticks, five ticks of step(actions), one following tick."""
    import torch

    cm = compiled_maps("loop")
    sim, sc, m = _bound(cm, launch_strategy=form)
    table = sc["table"]
    sim.reset()
    m.reset()
    for t in range(5):
        sim.step_history_agents()
        m.step()
    st0, words0, flags0 = _host(sim)
    status0, action0 = sim.out["history_agent_status"].clone(), sim.out["expert_action"].clone()
    acts = torch.zeros((E, N, 3), dtype=torch.float32)
    acts[..., 0], acts[..., 1] = 0.5, 0.1
    words = words0
    for t in range(5):
        sim.step(acts.cuda())
        _, new, flags = _host(sim)
        for e in range(E):
            for a in range(A):
                if not m.alive[e, a]:
                    continue
                # from the state it holds (the first driven tick: the last recorded pose), ImitationController's step
                x, y, h, u = (float(v) for v in words[e, a])
                want = imit.imitation_step(x, y, h, u, 0.5, float(np.float32(0.1)), DT)
                assert np.abs(new[e, a] - np.array(want)).max() <= 1e-9, (t, e, a, new[e, a], want)
            m.ticks[e] += 1  # (the env's frame goes on: the social slots replay, the twins stay hidden)
            coming = m.social_present(e, ref.REPLACED, ahead=1)
            assert np.array_equal((flags[e, A:] & nat.F_ALIVE) != 0, coming), (t, e)
        words = new
        # status and expert action keep their last values (bytes: the NaNs too)
        assert torch.equal(sim.out["history_agent_status"], status0)
        assert torch.equal(sim.out["expert_action"].view(torch.uint8), action0.view(torch.uint8))
    # (the model's rows are stale after the driven ticks: the following tick is checked by hand)
    before = words
    sim.step_history_agents()
    st, words, flags = _host(sim)
    status = sim.out["history_agent_status"].cpu().numpy()
    back = 0
    for e in range(E):
        f = m.frame(e) + 1
        for a in range(A):
            if not m.alive[e, a]:
                continue
            k = ref.find(table, f, m.followed(e, a))
            assert k >= 0 and status[e, a] == nat.HA_FOLLOWING
            assert np.array_equal(words[e, a].view(np.uint64), table.frames[f, k].view(np.uint64)), (e, a)  # back on the recording
            assert st[S_["LAT_INT"]][e, a] == before[e, a, 2] and st[S_["SPD_INT"]][e, a] == DT
            back += 1
    assert back >= 6
    sim.sync()
    sim.close()


@pytest.mark.parametrize("name,large", [("loop", "large_one_lane"), ("4lane", "large_teams")])
def test_launch_forms_agree_bit_for_bit(name, large, compiled_maps):
    """Check 6: state, flags, status, expert action and every output row, OGM and RGB on, under auto_reset."""
    import torch

    cm = compiled_maps(name)
    kw = dict(ogm=True, ogm_width=32, ogm_height=32, ogm_resolution=50 / 32, rgb=True, rgb_width=32, rgb_height=32,
              rgb_resolution=50 / 32, auto_reset=True)
    starts = np.array([[24, 33, 1, 31], [3, 0, 5, 30]], dtype=np.int32)
    sims = [_bound(cm, starts=starts, launch_strategy=s, **kw)[0] for s in FORMS]
    assert sims[0].launch_form() == "small" and sims[1].launch_form() == large

    def same(where):
        torch.cuda.synchronize()
        assert {"history_agent_status", "expert_action"} <= set(sims[0].out)
        for k in sims[0].out:
            if k == "learner":
                continue
            a, b = sims[0].out[k], sims[1].out[k]
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (where, k)  # (bytes: NaNs compare too)
        assert torch.equal(sims[0].flags, sims[1].flags), where
        a, b = sims[0].state.cpu().numpy(), sims[1].state.cpu().numpy()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), where
        assert torch.equal(sims[0].env_done_count, sims[1].env_done_count) and torch.equal(sims[0].env_episode, sims[1].env_episode)

    for s in sims:
        s.reset()
    same("reset")
    for t in range(T):
        for s in sims:
            s.step_history_agents()
        same(f"t{t}")
    assert (sims[0].flags.cpu().numpy() & nat.F_LEFT).any() or (sims[0].env_episode.cpu().numpy() > 0).all()
    for s in sims:
        s.close()


@pytest.mark.parametrize("form", FORMS)
def test_with_the_state_guard(form, compiled_maps):
    """Check 7: state_guard=True gives the same rows, and the guard byte of every follower reads 0 (the table was checked
    against the grids when it was bound), at the reset — whatever the spawn rows hold — and in every tick."""
    import torch

    cm = compiled_maps("loop")
    plain, sc, m = _bound(cm, launch_strategy=form)
    # spawn rows far outside the grids: a follower never reads them
    spawns = np.tile(sc["spawns"], (2, E, 1))
    spawns[:, :, 0] = 1.0e7
    guarded = _sim(cm, sc, spawns=spawns, launch_strategy=form, state_guard=True)
    guarded.set_traffic_history(sc["table"], torch.from_numpy(ref.STARTS).cuda(), torch.from_numpy(ref.REPLACED).cuda())
    guarded.set_history_agents(torch.from_numpy(ref.FOLLOW).cuda())

    def same(where):
        torch.cuda.synchronize()
        assert not guarded.out["guard"].any(), (where, guarded.out["guard"])
        assert not (guarded.flags & nat.F_GUARDED).any()
        for k in plain.out:
            if k == "learner":
                continue
            assert torch.equal(plain.out[k].view(torch.uint8), guarded.out[k].view(torch.uint8)), (where, k)
        assert torch.equal(plain.flags, guarded.flags), where
        a, b = plain.state.cpu().numpy(), guarded.state.cpu().numpy()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), where

    plain.reset()
    guarded.reset()
    same("reset")
    for t in range(T):
        plain.step_history_agents()
        guarded.step_history_agents()
        same(f"t{t}")
    assert (plain.out["history_agent_status"].cpu().numpy()[:, :A] == nat.HA_LEFT).sum() == 2
    plain.close()
    guarded.close()


def test_refusals(compiled_maps):
    """Check 8: no history bound, a sim that is not Imitation, short buffers, smx_step_history_agents without a binding;
    and smx_set_social_history, with a table or without, drops the binding."""
    import torch

    cm = compiled_maps("loop")
    sc = ref.scene(cm)
    follow = torch.from_numpy(ref.FOLLOW).cuda()
    st, rp = torch.from_numpy(ref.STARTS).cuda(), torch.from_numpy(ref.REPLACED).cuda()
    sim = _sim(cm, sc)
    with pytest.raises(nat.SmxError, match=r"\(-3\).*bound history"):  # SMX_ERR_STATE
        sim.set_history_agents(follow)
    sim.reset()
    with pytest.raises(nat.SmxError, match=r"\(-3\).*no history agents"):
        sim.step_history_agents()
    sim.set_traffic_history(sc["table"], st, rp)
    with pytest.raises(nat.SmxError, match=r"\(-3\).*no history agents"):
        sim.step_history_agents()
    with pytest.raises(ValueError, match="int32"):
        sim.set_history_agents(follow.to(torch.int64))
    with pytest.raises(ValueError, match="rows"):
        sim.set_history_agents(follow[:1].contiguous())

    def raw(vehicle_count, action=None, status=None):
        ha = nat.SmxHistoryAgents()
        ha.vehicle_dev, ha.vehicle_count = follow.data_ptr(), vehicle_count
        if action is not None:
            ha.action_dev, ha.action_count = action.data_ptr(), action.numel()
        if status is not None:
            ha.status_dev, ha.status_count = status.data_ptr(), status.numel()
        nat.check(sim.lib, sim.handle, sim.lib.smx_set_history_agents(sim.handle, C.byref(ha)), "smx_set_history_agents")

    with pytest.raises(nat.SmxError, match=r"\(-1\).*vehicle"):
        raw(follow.numel() - 1)
    with pytest.raises(nat.SmxError, match=r"\(-1\).*action"):
        raw(follow.numel(), action=torch.zeros(3 * E * N - 1, dtype=torch.float32).cuda())
    with pytest.raises(nat.SmxError, match=r"\(-1\).*status"):
        raw(follow.numel(), status=torch.zeros(E * N - 1, dtype=torch.uint8).cuda())
    assert "history_agent_status" not in sim.out
    sim.set_history_agents(follow, expert_actions=False)  # (and the good one binds, without the action row)
    assert "history_agent_status" in sim.out and "expert_action" not in sim.out
    sim.reset()
    sim.step_history_agents()
    sim.set_traffic_history(sc["table"], st, rp)  # binding a history drops the agents, on both sides
    assert "history_agent_status" not in sim.out and sim.history_agents is None
    with pytest.raises(nat.SmxError, match=r"\(-3\).*no history agents"):
        sim.step_history_agents()
    sim.set_history_agents(follow)
    sim.set_traffic_history(None)
    assert "expert_action" not in sim.out
    with pytest.raises(nat.SmxError, match=r"\(-3\)"):
        sim.step_history_agents()
    sim.sync()
    sim.close()
    other = _sim(cm, sc, action_space="TrajectoryWithTime")
    other.set_traffic_history(sc["table"], st, rp)
    with pytest.raises(nat.SmxError, match=r"\(-1\).*action_space.*IMITATION"):
        other.set_history_agents(follow)
    other.close()


def test_history_observer(compiled_maps):
    """Check 9: HistoryObserver hands out, per env, the observation of every followed vehicle under the reference's agent
    id; position, heading and speed are the recording; dones is true in the leaving tick; followers among the neighbours
    carry the provider's vehicle name."""
    from smarts_amd.env import HistoryObserver
    from smarts_amd.env.agent_interface import AgentInterface, AgentType, DoneCriteria, NeighborhoodVehicles

    cm = compiled_maps("loop")
    table = ref.scene(cm)["table"]
    never = DoneCriteria(collision=False, off_road=False, off_route=False, on_shoulder=False, wrong_way=False, not_moving=False)
    itf = AgentInterface.from_type(AgentType.Laner, neighborhood_vehicles=NeighborhoodVehicles(radius=None), done_criteria=never,
                                   max_episode_steps=None)
    watch = [ref.DRIVER, ref.LEAVER]
    ho = HistoryObserver("scenarios/loop", table, itf, vehicle_ids=watch, num_agents=2, dt=DT)
    assert ho.sim.cfg.action_space == "Imitation" and ho.E == 2
    # each env's second agent slot follows the lowest other id of the vehicle's first frame: the standing vehicle
    assert ho.followed[0].tolist() == [[ref.DRIVER, ref.STANDING], [ref.LEAVER, ref.STANDING]]
    name = lambda v: f"Agent-history-vehicle-{v}"  # noqa: E731
    obs, rewards, dones = ho.reset()
    left_tick = None
    for t in range(ref.LEAVER_LAST + 3):
        frame = t  # every env started at its vehicle's first frame, 0
        labels = ho.expert_actions()
        for e, v in enumerate(watch):
            gone = v == ref.LEAVER and frame > ref.LEAVER_LAST
            want_keys = {name(ref.STANDING)} | (set() if gone else {name(v)})
            assert set(obs[e]) == want_keys and set(rewards[e]) == want_keys, (t, e, set(obs[e]))
            for vid in (v, ref.STANDING):
                if name(vid) not in obs[e]:
                    continue
                o = obs[e][name(vid)]
                x, y, h, u = table.spawn_of(vid, frame)
                ego = o.ego_vehicle_state
                assert ego.id == f"history-vehicle-{vid}" and o.step_count == frame + ho.cfg.reset_elapsed_steps()
                assert ego.position[0] == x and ego.position[1] == y  # float64 rows: the recording itself
                assert float(ego.heading) == float(np.float32(h)) and ego.speed == float(np.float32(u))
                assert dones[e][name(vid)] is False
                want = table.expert_actions(vid)[frame].astype(np.float32)
                assert np.allclose(labels[e][name(vid)], want, rtol=0, atol=float(np.nan_to_num(_ulp32(want)).max()) + 4 * 2.0 ** -51 / DT, equal_nan=True)
                # every other vehicle of the frame is a neighbour (no radius), followers and replayed slots named alike
                ids = {nv.id for nv in o.neighborhood_vehicle_states}
                present = {w for w in (ref.STANDING, ref.DRIVER, ref.LEAVER, ref.LATE) if w != vid and ref.find(table, frame, w) >= 0}
                if v == ref.LEAVER and frame == ref.LEAVER_LAST + 1:
                    present.add(ref.LEAVER)  # (in its leaving tick a follower is still there for its env-mates, at the pose it holds)
                assert ids == {f"history-vehicle-{w}" for w in present}, (t, e, vid, ids)
            if v == ref.LEAVER and frame == ref.LEAVER_LAST + 1:
                assert dones[e][name(v)] is True and name(v) not in obs[e]  # done in the leaving tick, without an observation
                left_tick = t
            assert dones[e]["__all__"] is False
        obs, rewards, dones = ho.step()
    assert left_tick == ref.LEAVER_LAST + 1
    ho.close()

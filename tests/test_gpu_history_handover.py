"""Handing history agents over to actions one by one, inside a tick (include/smx.h smx_set_history_handover;
BatchedSim.set_history_handover / step_history_handover).

The scene is tests/history_agents_ref.py's — E = 4 envs, 3 agent slots and 3 replayed slots each, 30 ticks, on ``loop``
and ``4lane``, in the small form and in the forced large form — with the handover table, the actions and the rule in
NumPy of tests/history_handover_ref.py.  A follower is held to everything tests/test_gpu_history_agents.py holds it to
(its ``_check_against_model``); a driven agent to the NumPy Imitation step of tests/mpc_imitation_ref.py from the words
the device held before the tick, within tests/test_gpu_imitation.py's 1e-9 on the float64 state rows."""
import ctypes as C

import numpy as np
import pytest

import history_agents_ref as ref
import history_handover_ref as hand
import mpc_imitation_ref as imit
import parity
import test_gpu_history_agents as base
from smarts_amd import _native as nat

pytestmark = pytest.mark.gpu

E, A, S, N = ref.E, ref.AGENTS, ref.SLOTS, ref.N
T = 30
DT = ref.DT
S_ = nat.S
FORMS = ("small", "large")
MAPS = ("loop", "4lane")
# SMX_S_X .. SMX_S_MCL_Y, the vehicle and controller words a control kernel stores: pose, speed, raw / last heading, last dt
# among them.  (The rows behind them are the sensors' — trip meter, accelerometer, driven path — and the position the
# previous observation recorded, which every Imitation tick stores whatever the action says.)
OWN_WORDS = tuple(nat.STATE_FIELDS[:14])
RUN_OFF = np.array([[24, 33, 1, 31], [3, 0, 5, 30]], dtype=np.int32)  # (windows that run off the table's end within the run)


def _bound(cm, handover=hand.HANDOVER, starts=ref.STARTS, follow=ref.FOLLOW, replaced=ref.REPLACED, bind=True, **cfg_kw):
    """(sim, scene, model, the handover tensor): base._bound with the handover table bound beside the follow table."""
    import torch

    sim, sc, _ = base._bound(cm, starts=starts, follow=follow, replaced=replaced, **cfg_kw)
    ticks = torch.from_numpy(np.ascontiguousarray(handover)).cuda()
    if bind:
        sim.set_history_handover(ticks)
    return sim, sc, hand.Model(sc["table"], starts, follow, np.array(handover), sim.cfg.reset_elapsed_steps()), ticks


def _acts(t):
    import torch

    return torch.from_numpy(hand.actions(t)).cuda()


def _check_driven(sim, m, drive, acts, before, where, kept=None):
    """The agents `drive` [E, A] after a mixed tick, against the words `before` held: status and action row, the
    Imitation step, _last_heading / _last_dt, a NaN action's untouched words, SMX_F_LEFT never set.  `kept`: agents that
    ended while driven (the guard) and keep the byte."""
    st, words, flags = base._host(sim)
    status = sim.out["history_agent_status"].cpu().numpy()[:, :A]
    action = sim.out["expert_action"].cpu().numpy()[:, :A]
    assert ((status == nat.HA_DRIVEN) == (drive if kept is None else drive | kept)).all(), (where, status)
    assert np.isnan(action[drive][:, :2]).all() and (action[drive][:, 2] == 0).all(), where
    assert not (flags[:, :A][drive] & nat.F_LEFT).any(), where
    assert ((flags[:, :A][drive] & nat.F_ALIVE) != 0).all(), where
    worst = 0.0
    for e, a in zip(*np.nonzero(drive)):
        x, y, h, u = (float(before[S_[w]][e, a]) for w in ("X", "Y", "HEADING", "U"))
        want = imit.imitation_step(x, y, h, u, float(acts[e, a, 0]), float(acts[e, a, 1]), DT)
        # (the position recorded by the previous observation is stored whatever the action says, as in every Imitation tick)
        assert st[S_["PREV_X"]][e, a] == x and st[S_["PREV_Y"]][e, a] == y, (where, e, a)
        if want is None:  # no action: no control() call, every word of the vehicle's own bit for bit
            for w in OWN_WORDS:
                assert st[S_[w]][e, a].view(np.uint64) == before[S_[w]][e, a].view(np.uint64), (where, e, a, w)
            continue
        err = float(np.abs(words[e, a] - np.array(want)).max())
        worst = max(worst, err)
        assert err <= 1e-9, (where, e, a, words[e, a], want)
        assert st[S_["LAT_INT"]][e, a] == h and st[S_["SPD_INT"]][e, a] == DT, (where, e, a)  # control(): _last_heading, _last_dt
    m.hold(words[:, :A], drive)
    return worst


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MAPS)
def test_mixed_ticks_follow_the_rule(name, form, compiled_maps):
    """Cases 1-6 of the table, in every tick of the run: followers as in a following tick, driven agents as in a tick of
    step(actions), side by side in one launch."""
    cm = compiled_maps(name)
    sim, sc, m, _ = _bound(cm, launch_strategy=form)
    assert (sim.launch_form() == "small") == (form == "small")
    res = sim.cfg.reset_elapsed_steps()
    hand.assert_driven_in_bounds(cm, hand.driven_poses(sc["table"], ref.STARTS, hand.HANDOVER, res, T))
    sim.reset()
    m.reset()
    st = base._check_against_model(sim, m, ref.REPLACED, "reset")
    assert m.status[1, 2] == nat.HA_ABSENT and m.done_count.tolist() == [1, 1, 3, 1]  # case 3: counted from the start
    driven_ticks = np.zeros((E, A), dtype=int)
    nan_acts = scalar_acts = 0
    lefts = 0
    worst = 0.0
    for t in range(T):
        where = f"{name} {form} t{t}"
        acts = hand.actions(t)
        drive = m.driven_next()
        out = sim.step_history_handover(_acts(t))
        left, env_done = m.step(acts)
        before, st = st, base._check_against_model(sim, m, ref.REPLACED, where, st, left)
        worst = max(worst, _check_driven(sim, m, drive, acts, before, where))
        d = parity.host(out)
        act, done = d["active"].reshape(E, N)[:, :A], d["done"].reshape(E, N)[:, :A]
        assert np.array_equal(done != 0, left) and np.array_equal(act != 0, m.alive), where
        assert not (left & drive).any()
        assert np.array_equal(out["env_done"].cpu().numpy() != 0, env_done), where
        # a driven agent is observed at the pose it was driven to
        ego = d["ego_pos"].reshape(E, N, 3)[:, :A]
        assert np.array_equal(ego[drive][:, :2], np.stack([st[S_["X"]][:, :A][drive], st[S_["Y"]][:, :A][drive]], axis=-1)), where
        driven_ticks += drive
        nan_acts += int(np.isnan(acts[:, :A, 0])[drive].sum())
        scalar_acts += int((np.isnan(acts[:, :A, 1]) & ~np.isnan(acts[:, :A, 0]))[drive].sum())
        lefts += int(left.sum())
        if t == 0:
            assert drive.tolist() == [[False] * 3, [False, True, False], [False] * 3, [False] * 3]  # case 2: H = 0, the first tick
    print(f"{name} {form}: driven words within {worst:.3g} of the NumPy Imitation step (bound 1e-9)")
    # case 1: driven from env_ticks 5 on, beside the follower that left at its frame; case 6: its third slot never entered
    assert driven_ticks[0, 0] == T - (5 - res) and m.status[0].tolist() == [nat.HA_DRIVEN, nat.HA_LEFT, nat.HA_ABSENT]
    assert driven_ticks[1].tolist() == [0, T, 0] and m.status[1, 2] == nat.HA_ABSENT  # cases 2 and 3
    # case 4: its recorded vehicle ended at frame 17; the agent is alive and driven at the end, and never left
    assert driven_ticks[3, 0] == T - (10 - res) and m.alive[3, 0] and m.status[3, 0] == nat.HA_DRIVEN
    assert driven_ticks[3, 1] == 0 and m.status[3, 1] == nat.HA_FOLLOWING  # case 5
    assert driven_ticks[ref.FOLLOW[0] < 0].sum() == 0 and lefts == 1  # case 6; the one leaver that was never handed over
    assert nan_acts >= 4 and scalar_acts == 2
    sim.sync()
    sim.close()


def _same(a, b, where, skip=()):
    """Two sims after a pass: every output row, the state words and the flags, bit for bit."""
    import torch

    torch.cuda.synchronize()
    assert set(a.out) == set(b.out)
    for k in a.out:
        if k == "learner" or k in skip:
            continue
        assert torch.equal(a.out[k].view(torch.uint8), b.out[k].view(torch.uint8)), (where, k)  # (bytes: NaNs compare too)
    assert torch.equal(a.flags, b.flags), where
    x, y = a.state.cpu().numpy(), b.state.cpu().numpy()
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), where
    assert torch.equal(a.env_done_count, b.env_done_count) and torch.equal(a.env_episode, b.env_episode) and torch.equal(a.env_ticks, b.env_ticks)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MAPS)
def test_all_following_equals_the_following_tick(name, form, compiled_maps):
    """Equivalence (a): with every H = -1, step_history_handover is step_history_agents, bit for bit, under auto_reset."""
    cm = compiled_maps(name)
    never = np.full_like(hand.HANDOVER, -1)
    sim, _, _, _ = _bound(cm, handover=never, starts=RUN_OFF, launch_strategy=form, auto_reset=True)
    twin, _, _, _ = _bound(cm, handover=never, starts=RUN_OFF, launch_strategy=form, auto_reset=True, bind=False)
    sim.reset(), twin.reset()
    _same(sim, twin, "reset")
    for t in range(T):
        sim.step_history_handover(_acts(t))
        twin.step_history_agents()
        _same(sim, twin, f"{name} {form} t{t}")
    assert (sim.env_episode.cpu().numpy() >= 1).all()
    sim.close(), twin.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MAPS)
def test_all_driven_equals_the_driving_tick(name, form, compiled_maps):
    """Equivalence (b): with every H = 0 and the same actions, step_history_handover is step(actions) on a twin bound sim,
    bit for bit but for the status and expert-action rows, which step(actions) does not write."""
    cm = compiled_maps(name)
    always = np.zeros_like(hand.HANDOVER)
    sim, _, _, _ = _bound(cm, handover=always, launch_strategy=form)
    twin, _, _, _ = _bound(cm, handover=always, launch_strategy=form, bind=False)
    sim.reset(), twin.reset()
    _same(sim, twin, "reset")
    for t in range(T):
        sim.step_history_handover(_acts(t))
        twin.step(_acts(t))
        _same(sim, twin, f"{name} {form} t{t}", skip=("history_agent_status", "expert_action"))
    status = sim.out["history_agent_status"].cpu().numpy()[:, :A]
    assert np.array_equal(status == nat.HA_DRIVEN, (sim.flags.cpu().numpy()[:, :A] & nat.F_ALIVE) != 0) and (status == nat.HA_DRIVEN).sum() == 6
    assert not (sim.flags.cpu().numpy() & nat.F_LEFT).any()
    # the plain entry points ignore the table: a following tick on the sim with every H = 0 follows
    sim.step_history_agents()
    assert not (sim.out["history_agent_status"].cpu().numpy() == nat.HA_DRIVEN).any()
    sim.sync(), twin.sync()
    sim.close(), twin.close()


@pytest.mark.parametrize("form", FORMS)
def test_rewriting_the_table_in_place_puts_an_agent_back_on_the_recording(form, compiled_maps):
    """Twenty mixed ticks, then every driven agent's H becomes -1 in the bound tensor: at the next tick the driver is on
    its recorded row again (with the heading it drove to as _last_heading), and the agent whose vehicle the frame lacks
    leaves."""
    cm = compiled_maps("loop")
    sim, sc, m, ticks = _bound(cm, launch_strategy=form)
    sim.reset()
    m.reset()
    st = base._check_against_model(sim, m, ref.REPLACED, "reset")
    for t in range(20):
        acts = hand.actions(t)
        drive = m.driven_next()
        sim.step_history_handover(_acts(t))
        left, _ = m.step(acts)
        before, st = st, base._check_against_model(sim, m, ref.REPLACED, f"{form} t{t}", st, left)
        _check_driven(sim, m, drive, acts, before, f"{form} t{t}")
    was = m.driven_next()
    assert was[0, 0] and was[1, 1] and was[3, 0]
    ticks[ticks >= 0] = -1  # in place, on the device: the binding is not renewed
    m.handover[m.handover >= 0] = -1
    sim.step_history_handover(_acts(20))
    left, _ = m.step(hand.actions(20))
    base._check_against_model(sim, m, ref.REPLACED, f"{form} back", st, left)
    assert not m.driven_next().any()
    assert m.status[0, 0] == nat.HA_FOLLOWING and m.status[1, 1] == nat.HA_FOLLOWING  # back on the recording's words
    assert left[3, 0] and m.status[3, 0] == nat.HA_LEFT and left.sum() == 1  # frame 23 lacks the leaver
    assert m.last_heading[0, 0] == st[S_["HEADING"]][0, 0]  # (the heading it had driven to)
    sim.sync()
    sim.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MAPS)
def test_auto_reset_inside_a_handover_tick(name, form, compiled_maps):
    """An env that restarts inside a mixed tick: its agents are FOLLOWING on their spawn rows with _last_dt = 0 (the
    reset pass is unchanged), and the next tick applies episode 1's row of H."""
    cm = compiled_maps(name)
    sim, sc, m, _ = _bound(cm, starts=RUN_OFF, launch_strategy=form, auto_reset=True)
    res = sim.cfg.reset_elapsed_steps()
    hand.assert_driven_in_bounds(cm, hand.driven_poses(sc["table"], RUN_OFF, hand.HANDOVER, res, T, auto_reset=True))
    sim.reset()
    m.reset()
    st = base._check_against_model(sim, m, ref.REPLACED, "reset")
    restarted_at = {}
    first_after = {}
    for t in range(T):
        where = f"{name} {form} t{t}"
        acts = hand.actions(t)
        drive = m.driven_next()
        episode = m.episode.copy()
        out = sim.step_history_handover(_acts(t))
        left, env_done = m.step(acts, auto_reset=True)
        drive &= ~env_done[:, None]  # (a restarted env's rows are its new episode's)
        before, st = st, base._check_against_model(sim, m, ref.REPLACED, where, st, left & ~env_done[:, None])
        _check_driven(sim, m, drive, acts, before, where)
        assert np.array_equal(out["env_done"].cpu().numpy() != 0, env_done), where
        for e in np.nonzero(m.episode != episode)[0]:
            restarted_at[int(e)] = t
            assert (m.status[e][m.alive[e]] == nat.HA_FOLLOWING).all() and (m.last_dt[e] == 0).all()
        for e, at in restarted_at.items():
            if at == t - 1:
                first_after[e] = drive[e].tolist()
    # env 2 follows nothing in episode 0 and restarts after its first tick; env 3's only follower runs off the table
    assert restarted_at[2] == 0 and 3 in restarted_at and set(restarted_at) == {2, 3}, restarted_at
    assert (m.episode == [0, 0, 1, 1]).all()
    # the tick after the restart reads episode 1's row: H = 0 and H = 2 drive at once, H = 3 and H = -1 do not
    assert first_after[2] == [True, False, False] and first_after[3] == [True, False, False], first_after
    sim.sync()
    sim.close()


@pytest.mark.parametrize("form", FORMS)
def test_with_the_state_guard(form, compiled_maps):
    """state_guard=True: a follower's byte reads 0 in every tick; a driven agent whose action takes it outside the
    margin is held with GUARD_STEP and done, as an Imitation agent is.  (The wild action — a speed of 1e7 m/s set by the
    scalar form, then a plain step from it — only ever goes to a guarded sim.)"""
    import torch

    cm = compiled_maps("loop")
    sim, sc, m, _ = _bound(cm, launch_strategy=form, state_guard=True)
    sim.reset()
    m.reset()
    st = base._check_against_model(sim, m, ref.REPLACED, "reset")
    assert not sim.out["guard"].any()
    kept = np.zeros((E, A), dtype=bool)
    for t in range(12):
        where = f"{form} t{t}"
        acts = hand.actions(t)
        if t == 6:
            acts[1, 1, 0], acts[1, 1, 1] = 1.0e7, np.nan  # env 1 / agent 1, driven from the first tick: the speed is set
        if t == 7:
            acts[1, 1, 0], acts[1, 1, 1] = 0.0, 0.0  # ... and the step from it would land 1000 km away
        drive = m.driven_next()
        out = sim.step_history_handover(torch.from_numpy(acts).cuda())
        if t == 7:
            # the placement is refused: nothing of the vehicle is stored, the agent ends with this tick's observation
            # (its status byte says who decided the tick, and stays, as a left agent's does)
            assert drive[1, 1]
            drive[1, 1], kept[1, 1] = False, True
            m.alive[1, 1] = False
            m.done_count[1] += 1
            m.status[1, 1] = nat.HA_DRIVEN
        left, _ = m.step(acts)
        before, st = st, base._check_against_model(sim, m, ref.REPLACED, where, st, left)
        _check_driven(sim, m, drive, acts, before, where, kept)
        want = np.zeros((E, N), dtype=np.uint8)
        if t == 7:
            want[1, 1] = nat.GUARD_STEP
            assert before[S_["U"]][1, 1] == 1.0e7
            for w in OWN_WORDS:
                assert st[S_[w]][1, 1].view(np.uint64) == before[S_[w]][1, 1].view(np.uint64), (where, w)
            assert int(out["done"][1, 1]) == 1 and int(out["active"][1, 1]) == 0
            f = int(sim.flags[1, 1])
            assert (f & nat.F_GUARDED) and not (f & nat.F_ALIVE) and not (f & nat.F_LEFT)
        assert np.array_equal(sim.out["guard"].cpu().numpy(), want), where  # followers, and everybody in bounds: 0
    assert kept[1, 1] and m.driven_next()[0, 0]
    sim.sync()
    sim.close()


def test_refusals(compiled_maps):
    """smx_step_history_handover without a binding and smx_set_history_handover without history agents: SMX_ERR_STATE; a
    short or NULL table, NULL actions: SMX_ERR_INVALID; set_history_agents and set_traffic_history drop the binding."""
    import torch

    cm = compiled_maps("loop")
    sc = ref.scene(cm)
    follow = torch.from_numpy(ref.FOLLOW).cuda()
    ticks = torch.from_numpy(hand.HANDOVER).cuda()
    st, rp = torch.from_numpy(ref.STARTS).cuda(), torch.from_numpy(ref.REPLACED).cuda()
    sim = base._sim(cm, sc)
    sim.reset()
    acts = _acts(0)
    with pytest.raises(nat.SmxError, match=r"\(-3\).*no handover table"):
        sim.step_history_handover(acts)
    with pytest.raises(nat.SmxError, match=r"\(-3\).*bound history agents"):
        sim.set_history_handover(ticks)
    sim.set_traffic_history(sc["table"], st, rp)
    with pytest.raises(nat.SmxError, match=r"\(-3\).*bound history agents"):
        sim.set_history_handover(ticks)
    sim.set_history_agents(follow)
    with pytest.raises(nat.SmxError, match=r"\(-3\).*no handover table"):  # history agents alone are no binding
        sim.step_history_handover(acts)
    with pytest.raises(ValueError, match="int32"):
        sim.set_history_handover(ticks.to(torch.int64))
    with pytest.raises(ValueError, match="rows"):
        sim.set_history_handover(ticks[:1].contiguous())

    def raw(count, table=True):
        ho = nat.SmxHistoryHandover()
        ho.tick_dev, ho.tick_count = (ticks.data_ptr() if table else None), count
        nat.check(sim.lib, sim.handle, sim.lib.smx_set_history_handover(sim.handle, C.byref(ho)), "smx_set_history_handover")

    with pytest.raises(nat.SmxError, match=r"\(-1\).*tick"):
        raw(ticks.numel() - 1)
    with pytest.raises(nat.SmxError, match=r"\(-1\).*tick_dev"):
        raw(ticks.numel(), table=False)
    assert sim.history_handover is None
    sim.set_history_handover(ticks)
    assert sim.history_handover is ticks
    sim.reset()
    sim.step_history_handover(acts)
    with pytest.raises(ValueError, match="shape"):
        sim.step_history_handover(acts[:, :, :2].contiguous())
    rc = sim.lib.smx_step_history_handover(sim.handle, None, C.byref(sim._st), C.byref(sim._sp), C.byref(sim._out), sim._stream_ptr())
    assert rc == -1  # SMX_ERR_INVALID: actions_dev is NULL
    sim.set_history_handover(None)  # unbinds
    assert sim.history_handover is None
    with pytest.raises(nat.SmxError, match=r"\(-3\).*no handover table"):
        sim.step_history_handover(acts)
    sim.set_history_handover(ticks)
    sim.set_history_agents(follow)  # binding a follow table drops the handover, on both sides
    assert sim.history_handover is None
    with pytest.raises(nat.SmxError, match=r"\(-3\).*no handover table"):
        sim.step_history_handover(acts)
    sim.set_history_handover(ticks)
    sim.set_history_agents(None)  # ... and so does unbinding it
    assert sim.history_handover is None
    with pytest.raises(nat.SmxError, match=r"\(-3\)"):
        sim.step_history_handover(acts)
    sim.set_history_agents(follow)
    sim.set_history_handover(ticks)
    sim.set_traffic_history(sc["table"], st, rp)  # ... and a history, with a table or without
    assert sim.history_handover is None and sim.history_agents is None
    with pytest.raises(nat.SmxError, match=r"\(-3\)"):
        sim.step_history_handover(acts)
    sim.set_history_agents(follow)
    sim.set_history_handover(ticks)
    sim.set_traffic_history(None)
    assert sim.history_handover is None
    with pytest.raises(nat.SmxError, match=r"\(-3\)"):
        sim.step_history_handover(acts)
    sim.sync()
    sim.close()


def test_history_observer_with_a_handover(compiled_maps):
    """HistoryObserver(handover=...) end to end on ``loop``: a log-replay warm-up of four ticks for the driver, then the
    policy drives it; the other vehicles keep following.  Ids, driven(), the driven agent's observation keyed as before,
    NaN for its expert action."""
    from smarts_amd.env import HistoryObserver
    from smarts_amd.env.agent_interface import AgentInterface, AgentType, DoneCriteria, NeighborhoodVehicles

    cm = compiled_maps("loop")
    table = ref.scene(cm)["table"]
    never = DoneCriteria(collision=False, off_road=False, off_route=False, on_shoulder=False, wrong_way=False, not_moving=False)
    itf = AgentInterface.from_type(AgentType.Laner, neighborhood_vehicles=NeighborhoodVehicles(radius=None), done_criteria=never,
                                   max_episode_steps=None)
    watch = [ref.DRIVER, ref.LEAVER]
    name = lambda v: f"Agent-history-vehicle-{v}"  # noqa: E731
    res = 2
    ho = HistoryObserver("scenarios/loop", table, itf, vehicle_ids=watch, num_agents=2, dt=DT, handover={ref.DRIVER: res + 4})
    assert ho.handover.tolist() == [[[res + 4, -1], [-1, -1]]] and ho.cfg.reset_elapsed_steps() == res
    obs, rewards, dones = ho.reset()
    assert ho.driven() == [[], []]
    pose = None
    for t in range(10):
        driven = ho.driven()
        assert driven == ([[name(ref.DRIVER)], []] if t >= 4 else [[], []]), (t, driven)
        o = obs[0][name(ref.DRIVER)]
        assert set(obs[0]) == {name(ref.DRIVER), name(ref.STANDING)} and set(obs[1]) == {name(ref.LEAVER), name(ref.STANDING)}
        assert o.ego_vehicle_state.id == f"history-vehicle-{ref.DRIVER}" and o.step_count == t + res
        labels = ho.expert_actions()
        if t <= 4:  # on the recording (the observation after tick 4 is still the last followed one)
            x, y, h, u = table.spawn_of(ref.DRIVER, t)
            assert o.ego_vehicle_state.position[0] == x and o.ego_vehicle_state.position[1] == y
        if t < 5:
            assert not np.isnan(labels[0][name(ref.DRIVER)]).any()
        else:  # driven: no label, and the pose is the Imitation step's from the one before
            assert np.isnan(labels[0][name(ref.DRIVER)]).all()
            want = imit.imitation_step(*pose, 0.5, float(np.float32(0.1)), DT)
            got = o.ego_vehicle_state
            assert abs(got.position[0] - want[0]) <= 1e-9 and abs(got.position[1] - want[1]) <= 1e-9
            assert got.speed == float(np.float32(want[3]))
        assert not np.isnan(labels[0][name(ref.STANDING)]).any() and not np.isnan(labels[1][name(ref.LEAVER)]).any()
        st, words, _ = base._host(ho.sim)
        pose = tuple(float(v) for v in words[0, 0])
        # the same action for every env that has the id: only the driven agent reads it
        obs, rewards, dones = ho.step({name(ref.DRIVER): (0.5, 0.1), name(ref.STANDING): (3.0, 3.0)})
        assert dones[0][name(ref.DRIVER)] is False
    # the standing vehicle and the leaver were never driven: still on their rows
    x, y, h, u = table.spawn_of(ref.STANDING, 10)
    assert obs[0][name(ref.STANDING)].ego_vehicle_state.position[0] == x
    x, y, h, u = table.spawn_of(ref.LEAVER, 10)
    assert obs[1][name(ref.LEAVER)].ego_vehicle_state.position[1] == y
    ho.close()

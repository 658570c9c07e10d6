"""Traffic-history replay on the device (include/smx.h smx_set_social_history; BatchedSim.set_traffic_history).

The scene (tests/traffic_history_ref.py ``scene``): two agents and three replayed slots per env, a synthetic history along
lane centre lines of ``loop`` and ``4lane`` — a vehicle standing in agent 0's lane ahead of its spawn (a collision within
the run), one slot used by two vehicles on opposite sides of the map, a vehicle off the road but inside the grids,
vehicles that appear and leave mid-run — replayed by four envs from their own start frames: 0, a negative one, one whose
window runs past the table's end, and a twin of env 0 that hides the standing vehicle."""
import numpy as np
import pytest

import parity
import traffic_history_ref as ref
from smarts_amd import _native as nat

pytestmark = pytest.mark.gpu

E = 4
STARTS = np.array([[0, -3, 25, 1]], dtype=np.int32)
REPLACED = np.array([[-1, -1, -1, ref.STANDING]], dtype=np.int32)
A, S = ref.AGENTS, ref.SLOTS
N = A + S
T = 30
S_ = nat.S


def _make(cm, starts=STARTS, replaced=REPLACED, bind=True, **cfg_kw):
    """(sim, scene, start tensor, replaced tensor): the scene in every env, the history bound."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig

    sc = ref.scene(cm)
    kw = dict(num_envs=E, num_vehicles=N, num_social=S, neighbors=True, nb_radius=60.0)
    kw.update(cfg_kw)
    cfg = SimConfig(**kw)
    episodes = max(2, starts.shape[0])
    spawns = np.tile(sc["spawns"], (episodes, E, 1))
    social = np.tile(sc["social_spawns"], (episodes, E, 1))
    sim = BatchedSim(cm, cfg, spawns=spawns, social_spawns=social)
    st = torch.from_numpy(starts.copy()).cuda()
    rp = torch.from_numpy(replaced.copy()).cuda() if replaced is not None else None
    if bind:
        sim.set_traffic_history(sc["table"], st, rp)
    return sim, sc, st, rp


def _expected(table, starts_row, replaced_row, ticks, ahead=0):
    """Per env and slot: presence and the row of the frame at tick count `ticks[e]` (+ `ahead`)."""
    present = np.zeros((E, S), dtype=bool)
    rows = np.zeros((E, S, 4))
    for e in range(E):
        frame = int(starts_row[e]) + int(ticks[e]) + ahead
        for k in range(S):
            v = table.vehicle_at(frame, k)
            present[e, k] = v >= 0 and v != int(replaced_row[e])
            if present[e, k]:
                rows[e, k] = table.frames[frame, k]
    return present, rows


def _social_state(sim):
    import torch

    torch.cuda.synchronize()
    st = sim.state.cpu().numpy()
    words = np.stack([st[S_[w]][:, A:] for w in ("X", "Y", "HEADING", "U")], axis=-1)  # [E, S, 4]
    return words, sim.flags.cpu().numpy()[:, A:], st


def _assert_rows_are_the_table(sim, table, starts_row, replaced_row, where):
    """After a pass: the social slots present in the pass's frame hold that frame's rows, and the flags word — which the
    pass's commit has already made the next tick's — says who is present in the next frame."""
    words, flags, st = _social_state(sim)
    ticks = sim.env_ticks.cpu().numpy()
    present, rows = _expected(table, starts_row, replaced_row, ticks)
    coming, _ = _expected(table, starts_row, replaced_row, ticks, ahead=1)
    assert np.array_equal((flags & nat.F_ALIVE) != 0, coming), (where, flags, coming)
    assert np.all(flags & nat.F_SOCIAL), where
    got, want = words[present], rows[present]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (where, got, want)  # bit for bit
    for w in ("MCL_X", "MCL_Y", "SPD_INT"):
        assert not st[S_[w]][:, A:].any(), (where, w)
    return present


def _actions(rng):
    acts = np.where(rng.random((E, N)) < 0.8, 0, 1).astype(np.int8)  # keep_lane, now and then slow_down
    acts[:, 0] = 0  # agent 0 keeps its lane: into the standing vehicle
    return acts


def _slot_of(table, vid):
    return int(np.nonzero((table.vehicle == vid).any(axis=0))[0][0])


@pytest.mark.parametrize("name", ["loop", "4lane"])
def test_against_the_oracle_and_the_table(name, nets, compiled_maps):
    """Every dense row against the oracle with replayed social bodies, teacher forced, at test_gpu_parity's tolerances;
    and in every tick and env the social slots' state rows are the table's rows bit for bit, SMX_F_ALIVE is presence,
    their active / done read 0, and leaving social vehicles never count as finished agents."""
    import torch

    cm = compiled_maps(name)
    sim, sc, st, rp = _make(cm, ogm=True, ogm_width=64, ogm_height=64, ogm_resolution=50 / 64)
    table = sc["table"]
    assert _slot_of(table, ref.FIRST) == _slot_of(table, ref.SECOND)  # the reused slot
    ob = parity.OracleBatch(nets(name), cm, sim.cfg, np.tile(sc["spawns"][0], (E, 1)), np.tile(sc["social_spawns"][0], (E, 1)))
    ref.install(ob, table, STARTS[0], REPLACED[0])
    d, o = parity.host(sim.reset()), ob.reset_observe()
    bad = parity.compare(d, o, tol64=1e-9, tol32=2e-6, where="reset ")
    assert bad == [], "\n".join(bad)
    seen = _assert_rows_are_the_table(sim, table, STARTS[0], REPLACED[0], "reset").astype(int)
    appeared = left = 0
    rng = np.random.default_rng(7)
    collided = np.zeros(E, dtype=bool)
    collidee_bits = np.zeros(E, dtype=np.uint64)
    for t in range(T):
        acts = _actions(rng)
        out = sim.step(torch.from_numpy(acts).cuda())
        d, o = parity.host(out), ob.step(acts)
        bad = parity.compare(d, o, tol64=1e-9, tol32=2e-5, where=f"{name} t{t} ")
        assert bad == [], "\n".join(bad)
        present = _assert_rows_are_the_table(sim, table, STARTS[0], REPLACED[0], f"{name} t{t}").astype(int)
        appeared += int(((present - seen) > 0).sum())
        left += int(((present - seen) < 0).sum())
        seen = present
        act, done = d["active"].reshape(E, N), d["done"].reshape(E, N)
        assert not act[:, A:].any() and not done[:, A:].any()
        ev = d["events"].reshape(E, N, -1)[:, 0, nat.EV_COLLISIONS].astype(bool)
        collidee_bits |= np.where(ev, d["collidees"].reshape(E, N)[:, 0].astype(np.uint64), np.uint64(0))
        collided |= ev
        # env_done_count counts agents only; an env whose social vehicles have all left goes on while an agent lives
        agents_gone = A - ((sim.flags.cpu().numpy()[:, :A] & nat.F_ALIVE) != 0).sum(axis=1)
        assert np.array_equal(sim.env_done_count.cpu().numpy(), agents_gone), (t, sim.env_done_count, agents_gone)
        assert np.array_equal(out["env_done"].cpu().numpy() != 0, agents_gone == A)
        parity.sync_oracle_from_device(ob, sim)
    assert appeared >= 4 and left >= 6, (appeared, left)  # vehicles came and went mid-run, the reused slot among them
    # env 2's window ran past the table's end: every social vehicle gone, the env not done while agent 1 lives
    flags = sim.flags.cpu().numpy()
    assert not (flags[2, A:] & nat.F_ALIVE).any() and (flags[2, 1] & nat.F_ALIVE) and not sim.out["env_done"].cpu().numpy()[2]
    # agent 0 ran into the standing vehicle — bit of its slot — except where that vehicle is hidden (`replaced`)
    standing = np.uint64(1 << (A + _slot_of(table, ref.STANDING)))
    assert collided.tolist() == [True, True, True, False], collided
    assert all(collidee_bits[e] == standing for e in (0, 1, 2)) and collidee_bits[3] == 0
    sim.close()


@pytest.mark.parametrize("name,large", [("loop", "large_one_lane"), ("4lane", "large_teams")])
def test_launch_forms_agree_bit_for_bit(name, large, compiled_maps):
    """The same scene in the small form and in the map's large form (loop: the one-lane cut, 4lane: the teams cut),
    OGM, lidar, neighbours and RGB on: every output and the state bit for bit equal in every tick, the reused slot's
    first tick and every appearing vehicle's included."""
    import torch

    from smarts_amd.lidar import SensorParams

    cm = compiled_maps(name)
    kw = dict(ogm=True, ogm_width=32, ogm_height=32, ogm_resolution=50 / 32, rgb=True, rgb_width=32, rgb_height=32,
              rgb_resolution=50 / 32,
              lidar=SensorParams(start_angle=0.0, end_angle=2 * np.pi, laser_angles=np.linspace(-np.pi / 36, np.pi / 36, 2),
                                 angle_resolution=np.pi / 8, max_distance=20.0, noise_mu=0, noise_sigma=0))
    sims = [_make(cm, launch_strategy=s, **kw)[0] for s in ("small", "large")]
    assert sims[0].launch_form() == "small" and sims[1].launch_form() == large
    table = ref.scene(cm)["table"]

    def same(where):
        torch.cuda.synchronize()
        for k in sims[0].out:
            if k == "learner":
                continue
            assert torch.equal(sims[0].out[k], sims[1].out[k]), (where, k)
        assert torch.equal(sims[0].flags, sims[1].flags), where
        a, b = sims[0].state.cpu().numpy(), sims[1].state.cpu().numpy()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), where

    for s in sims:
        s.reset()
    same("reset")
    rng = np.random.default_rng(11)
    for t in range(T):
        acts = torch.from_numpy(_actions(rng)).cuda()
        for s in sims:
            s.step(acts)
        same(f"t{t}")
        _assert_rows_are_the_table(sims[1], table, STARTS[0], REPLACED[0], f"large t{t}")
    for s in sims:
        s.close()


def test_auto_reset_and_rewritten_start_frames(compiled_maps):
    """R = 2 rows: after an env restarts, its social slots show the table at start_frames[1, e] + reset_elapsed_steps;
    rewriting start_frames in place between ticks moves the next tick's frame."""
    import torch

    cm = compiled_maps("loop")
    starts = np.array([[0, -3, 25, 1], [12, 2, 0, 14]], dtype=np.int32)
    replaced = np.array([[-1, -1, -1, ref.STANDING], [ref.STANDING, -1, -1, -1]], dtype=np.int32)
    sim, sc, st, rp = _make(cm, starts=starts, replaced=replaced, auto_reset=True, max_episode_steps=6)
    table = sc["table"]
    sim.reset()
    rows = np.zeros(E, dtype=np.int64)  # the row of the two tables each env reads: its episode mod 2
    rng = np.random.default_rng(3)
    restarted = np.zeros(E, dtype=bool)
    for t in range(7):  # (every episode is five ticks long: the fifth tick restarts every env, and the tenth would)
        out = sim.step(torch.from_numpy(_actions(rng)).cuda())
        ep = sim.env_episode.cpu().numpy()
        rows = ep % 2
        ticks = sim.env_ticks.cpu().numpy()
        fresh = ticks == sim.cfg.reset_elapsed_steps()
        restarted |= fresh & (ep > 0)
        s_row, r_row = starts[rows, np.arange(E)], replaced[rows, np.arange(E)]
        _assert_rows_are_the_table(sim, table, s_row, r_row, f"t{t}")
        assert not out["active"][:, A:].any()
    assert restarted.all()  # max_episode_steps ended every episode once
    # in place: every env jumps a few frames ahead, to a frame that holds the same vehicles in the same slots as the one
    # it would have shown (the flags word was decided for that one); the next tick shows the new frame's rows
    ticks = sim.env_ticks.cpu().numpy()
    old_frames = starts[rows, np.arange(E)] + ticks + 1
    ids = lambda f: [table.vehicle_at(int(f), k) for k in range(S)]  # noqa: E731
    jump = {e: next((d for d in range(2, 7) if ids(old_frames[e]) == ids(old_frames[e] + d) and any(v >= 0 for v in ids(old_frames[e]))), None)
            for e in range(E)}
    moved = [e for e in range(E) if jump[e] is not None]
    assert moved, (old_frames, jump)
    new = starts.copy()
    for e in moved:
        new[rows[e], e] += jump[e]
    st.copy_(torch.from_numpy(new).cuda())
    sim.step(torch.from_numpy(_actions(rng)).cuda())
    words, flags, _ = _social_state(sim)
    assert np.array_equal(sim.env_episode.cpu().numpy() % 2, rows)  # (no env restarted in this tick)
    checked = 0
    for e in moved:
        target = int(old_frames[e] + jump[e])
        for k in range(S):
            v = table.vehicle_at(target, k)
            if v >= 0 and v != replaced[rows[e], e]:
                assert np.array_equal(words[e, k].view(np.uint64), table.frames[target, k].view(np.uint64)), (e, k, words[e, k])
                checked += 1
    assert checked > 0
    # a vehicle the new frame lacks leaves at once: past the end of the table nothing is alive
    st.fill_(10_000)
    sim.step(torch.from_numpy(_actions(rng)).cuda())
    torch.cuda.synchronize()
    assert not (sim.flags.cpu().numpy()[:, A:] & nat.F_ALIVE).any()
    # ... and at the ends of int32 too (any value is safe)
    for v in (np.iinfo(np.int32).min, np.iinfo(np.int32).max):
        st.fill_(int(v))
        sim.step(torch.from_numpy(_actions(rng)).cuda())
    torch.cuda.synchronize()
    assert not (sim.flags.cpu().numpy()[:, A:] & nat.F_ALIVE).any()
    sim.close()


def test_unbinding_restores_the_scripted_vehicles(compiled_maps):
    """table=None unbinds: after the next reset the social slots are the scripted lane followers again."""
    import torch

    cm = compiled_maps("loop")
    sim, sc, st, rp = _make(cm)
    sim.reset()
    sim.step(torch.zeros((E, N), dtype=torch.int8).cuda())
    sim.set_traffic_history(None)
    sim.reset()
    sim.step(torch.zeros((E, N), dtype=torch.int8).cuda())
    torch.cuda.synchronize()
    flags = sim.flags.cpu().numpy()[:, A:]
    assert ((flags & nat.F_ALIVE) != 0).all()
    assert (sim.state[S_["MCL_Y"]][:, A:] > 0).all()  # arclength along their lane
    sim.close()


def test_refusals(compiled_maps):
    """IDM, a wrong slot count and an out-of-grid row are SMX_ERR_INVALID with the reason."""
    import torch

    from smarts_amd.traffic_history import TrafficHistoryTable

    cm = compiled_maps("loop")
    sim, sc, st, rp = _make(cm, bind=False)
    table = sc["table"]
    wide = TrafficHistoryTable(np.concatenate([table.frames, table.frames[:, :1]], axis=1),
                               np.concatenate([table.vehicle, np.full_like(table.vehicle[:, :1], -1)], axis=1), table.dt)
    with pytest.raises(nat.SmxError, match=r"\(-1\).*num_social"):
        sim.set_traffic_history(wide, st, rp)
    far = TrafficHistoryTable(table.frames.copy(), table.vehicle, table.dt)
    far.frames[7, 0, 0] = 1.0e5
    with pytest.raises(nat.SmxError, match=r"\(-1\).*frame 7, slot 0.*grids"):
        sim.set_traffic_history(far, st, rp)
    far.frames[7, 0, 0] = np.nan
    with pytest.raises(nat.SmxError, match=r"\(-1\).*not finite"):
        sim.set_traffic_history(far, st, rp)
    with pytest.raises(ValueError, match="int32"):
        sim.set_traffic_history(table, st.to(torch.int64), None)
    with pytest.raises(nat.SmxError, match=r"\(-1\).*start_frame"):  # a short table, straight through the C-ABI
        import ctypes as C

        hs = nat.SmxSocialHistory()
        f, v = np.ascontiguousarray(table.frames), np.ascontiguousarray(table.vehicle)
        hs.frames_host, hs.vehicle_host, hs.n_frames, hs.num_social = f.ctypes.data, v.ctypes.data, f.shape[0], f.shape[1]
        hs.start_frame_dev, hs.rows, hs.start_count = st.data_ptr(), 2, st.numel()
        nat.check(sim.lib, sim.handle, sim.lib.smx_set_social_history(sim.handle, C.byref(hs)), "smx_set_social_history")
    sim.set_traffic_history(table, st, rp)  # (and the good one binds)
    sim.close()
    idm, *_ = _make(cm, bind=False, social_model="idm")
    with pytest.raises(nat.SmxError, match=r"\(-1\).*IDM"):
        idm.set_traffic_history(table, st, rp)
    idm.close()


def test_env_layer_names_replayed_neighbours(compiled_maps):
    """HiWayEnv(traffic_history=...): neighbour ids are history-vehicle-<id> of table.vehicle_at(frame, slot)."""
    from smarts_amd.env.agent import AgentSpec
    from smarts_amd.env.agent_interface import AgentInterface, AgentType, NeighborhoodVehicles
    from smarts_amd.env.hiway_env import HiWayEnv

    cm = compiled_maps("loop")
    table = ref.scene(cm)["table"]
    itf = AgentInterface.from_type(AgentType.Laner, max_episode_steps=50, neighborhood_vehicles=NeighborhoodVehicles(radius=None))
    start = 2
    env = HiWayEnv(["scenarios/loop"], {"a": AgentSpec(interface=itf)}, num_social=S, traffic_history=table,
                   history_start_frames=start, spawns="synthetic")
    obs = env.reset()
    names_seen = set()
    for t in range(14):
        o = obs["a"]
        frame = start + int(o.step_count)
        want = {f"history-vehicle-{table.vehicle_at(frame, k)}" for k in range(S) if table.vehicle_at(frame, k) >= 0}
        got = {nv.id for nv in o.neighborhood_vehicle_states}
        assert got == want, (t, frame, got, want)
        names_seen |= got
        obs, _, dones, _ = env.step({"a": "keep_lane"})
        if dones["__all__"]:
            break
    assert {f"history-vehicle-{v}" for v in (ref.STANDING, ref.FIRST, ref.SECOND, ref.OFF_ROAD)} <= names_seen
    env.close()

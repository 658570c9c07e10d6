"""The end of a large-form pass: k_tail (the tick's commit, the new vehicles' OGM / DAGM tiles, the env groups with new
vehicles for k_first, the next tick's alive list in eight segments) and the merged control slow list.

Each test forces the large form onto a small batch and holds it to the small form bit for bit (every output, the
state and the flags), or teacher-forced to the oracle: envs that restart on the same tick as vehicles elsewhere die,
with OGM on; auto_reset=False (k_tail commits, nothing restarts); IDM social traffic (k_social moves vehicles ahead of
the list, so the tick builds its own); the first tick after an explicit smx_reset, full and masked.
"""
import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

CUTS = ("large_one_lane", "large_teams")
FORMS = ("small",) + CUTS
OGM64 = dict(ogm=True, ogm_width=64, ogm_height=64, ogm_resolution=50 / 64)


def _sims(cm, spawns, kw, sim_kw=None):
    from smarts_amd.engine import BatchedSim, SimConfig

    sims = [BatchedSim(cm, SimConfig(launch_strategy=s, **kw), spawns=spawns, **(sim_kw or {})) for s in FORMS]
    assert [s.launch_form() for s in sims] == list(FORMS)
    return sims


def _agree(sims, outs, where):
    import torch

    torch.cuda.synchronize()
    for other in (1, 2):
        for k in outs[0]:
            assert np.array_equal(outs[0][k].cpu().numpy(), outs[other][k].cpu().numpy(), equal_nan=True), (where, k, FORMS[other])
        assert np.array_equal(sims[0].state.cpu().numpy(), sims[other].state.cpu().numpy(), equal_nan=True), (where, FORMS[other])
        assert np.array_equal(sims[0].flags.cpu().numpy(), sims[other].flags.cpu().numpy()), (where, FORMS[other])


def test_restarts_beside_deaths_with_ogm(compiled_maps):
    """Envs on staggered episodes (masked resets on ticks 1-7), two vehicles of every env spawned on the same spot: on
    some tick an env restarts (k_tail respawns it and draws its OGM tiles, k_first runs over the listed groups) while
    the pair of a freshly started env elsewhere collides and dies (k_tail's list leaves it out).  Every tick agrees bit
    for bit with the small form."""
    import torch

    from smarts_amd.engine import make_spawns

    cm = compiled_maps("loop")
    E, N, T = 16, 8, 30
    kw = dict(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, auto_reset=True, max_episode_steps=9,
              done_collision=True, **OGM64)
    spawns = make_spawns(cm, E, N, episodes=8, seed=41)
    spawns[:, 1::N] = spawns[:, 0::N]  # vehicles 0 and 1 of every env collide on their first tick
    sims = _sims(cm, spawns, kw)
    outs = [s.reset() for s in sims]
    _agree(sims, outs, "reset")
    rng = np.random.default_rng(41)
    both = 0
    for t in range(T):
        if 1 <= t <= 7:
            mask = torch.from_numpy((np.arange(E) % 8 == t).astype(np.uint8))
            outs = [s.reset(mask) for s in sims]
            _agree(sims, outs, f"masked reset t{t}")
        before = sims[0].flags.cpu().numpy().reshape(E, N).copy()
        acts = torch.from_numpy(parity.lane_actions(rng, E, N)).cuda()
        outs = [s.step(acts) for s in sims]
        _agree(sims, outs, f"t{t}")
        env_done = outs[0]["env_done"].cpu().numpy().reshape(E).astype(bool)
        died = outs[0]["done"].cpu().numpy().reshape(E, N).astype(bool) & (before & 1).astype(bool)
        if env_done.any() and died[~env_done].any():
            both += 1
    assert both > 0  # restarts and deaths elsewhere on the same tick happened
    assert (outs[0]["ogm"].cpu().numpy() == 255).any()
    for s in sims:
        s.close()


@pytest.mark.parametrize("strategy", CUTS)
def test_restart_tick_matches_oracle_with_ogm(strategy, nets, compiled_maps):
    """The tick on which every env reaches its step limit, with OGM on: the observation handed back is episode 1's
    first one, as an explicit reset of a twin batch builds it (k_reset + k_tail + k_first); the ticks before it are
    held to the oracle teacher-forced."""
    import torch

    from smarts_amd.engine import BatchedSim

    E, N = 4, 8
    sim, ob, cfg = parity.make("loop", E, N, nets, compiled_maps, 57, launch_strategy=strategy, max_episode_steps=5,
                               auto_reset=True, done_collision=False, done_off_road=False, done_off_route=False, **OGM64)
    assert sim.launch_form() == strategy
    d = parity.host(sim.reset())
    bad = parity.compare(d, ob.reset_observe(), where="reset ", tol64=1e-9, tol32=2e-6)
    assert bad == [], "\n".join(bad[:8])
    acts = np.zeros((E, N), dtype=np.int8)
    for t in range(3):
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
        bad = parity.compare(d, o, where=f"t{t} ", tol64=1e-9, tol32=2e-5)
        assert bad == [], "\n".join(bad[:8])
        parity.sync_oracle_from_device(ob, sim)
    out = sim.step(torch.from_numpy(acts).cuda())
    got = parity.host(out)
    assert out["env_done"].cpu().numpy().all()
    twin = BatchedSim(sim.cm, cfg, spawns=sim.spawns.cpu().numpy())
    twin.reset()
    ref = parity.host(twin.reset())
    for k in ref:
        if k in ("reward", "done", "learner") or k.startswith("final_"):
            continue  # the auto-reset tick keeps the finishing tick's reward / done (and its final rows)
        assert np.array_equal(ref[k], got[k], equal_nan=True), k
    assert (got["ogm"] == 255).any()
    twin.close()
    sim.close()


def test_no_auto_reset(compiled_maps):
    """auto_reset=False: k_tail commits, envs that end stay ended, the list thins out to nothing."""
    import torch

    from smarts_amd.engine import make_spawns

    cm = compiled_maps("loop")
    E, N, T = 6, 16, 14
    kw = dict(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, auto_reset=False, max_episode_steps=6,
              done_collision=True)
    sims = _sims(cm, make_spawns(cm, E, N, episodes=2, seed=43), kw)
    outs = [s.reset() for s in sims]
    rng = np.random.default_rng(43)
    for t in range(T):
        acts = torch.from_numpy(parity.lane_actions(rng, E, N)).cuda()
        outs = [s.step(acts) for s in sims]
        _agree(sims, outs, f"t{t}")
    assert (sims[1].flags.cpu().numpy() & 1).sum() == 0  # every agent gone, none respawned
    assert (sims[1].env_episode.cpu().numpy() == 0).all()
    for s in sims:
        s.close()


def test_idm_social_traffic(compiled_maps):
    """IDM social traffic: k_social moves the fleet ahead of the tick's list, which k_alive_list then builds itself;
    auto-reset restarts on the way."""
    import torch

    from smarts_amd.engine import make_spawns

    cm = compiled_maps("loop")
    E, agents, social, T = 4, 4, 12, 24
    N = agents + social
    kw = dict(num_envs=E, num_vehicles=N, num_social=social, social_model="idm", social_speed_factor=1.0,
              neighbors=True, nb_radius=60.0, auto_reset=True, max_episode_steps=10, done_collision=False)
    spawns, where = make_spawns(cm, E, N, episodes=4, seed=45, return_lanes=True)
    sims = _sims(cm, spawns, kw, dict(social_spawns=where))
    outs = [s.reset() for s in sims]
    _agree(sims, outs, "reset")
    rng = np.random.default_rng(45)
    for t in range(T):
        acts = parity.lane_actions(rng, E, N)
        acts[:, 0] = 1
        outs = [s.step(torch.from_numpy(acts).cuda()) for s in sims]
        _agree(sims, outs, f"t{t}")
    assert (sims[0].env_episode.cpu().numpy() >= 1).all()
    for s in sims:
        s.close()


@pytest.mark.parametrize("strategy", CUTS)
def test_first_tick_after_reset_matches_oracle(strategy, nets, compiled_maps):
    """The first tick after smx_reset takes the alive list the reset pass's k_tail built: held to the oracle
    teacher-forced, after the first reset and after a second full reset in mid-run."""
    import torch

    E, N = 3, 8
    sim, ob, cfg = parity.make("loop", E, N, nets, compiled_maps, 59, launch_strategy=strategy, **OGM64)
    assert sim.launch_form() == strategy
    rng = np.random.default_rng(59)
    for rnd in range(2):
        if rnd == 1:  # a reset starts the next spawn row: the oracle of episode 1
            ob = parity.OracleBatch(nets("loop"), compiled_maps("loop"), cfg, sim.spawns[1].cpu().numpy())
        d = parity.host(sim.reset())
        bad = parity.compare(d, ob.reset_observe(), where=f"reset {rnd} ", tol64=1e-9, tol32=2e-6)
        assert bad == [], "\n".join(bad[:8])
        for t in range(3):
            acts = parity.lane_actions(rng, E, N)
            d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
            bad = parity.compare(d, o, where=f"round {rnd} t{t} ", tol64=1e-9, tol32=2e-5)
            assert bad == [], "\n".join(bad[:8])
            parity.sync_oracle_from_device(ob, sim)
    sim.close()


def test_first_tick_after_masked_reset(compiled_maps):
    """A masked smx_reset between ticks: the next tick's list comes from the reset pass's k_tail and must hold the
    respawned envs' vehicles as well as the others'."""
    import torch

    from smarts_amd.engine import make_spawns

    cm = compiled_maps("loop")
    E, N, T = 6, 16, 12
    kw = dict(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, auto_reset=False, max_episode_steps=5,
              done_collision=True)
    sims = _sims(cm, make_spawns(cm, E, N, episodes=4, seed=47), kw)
    outs = [s.reset() for s in sims]
    rng = np.random.default_rng(47)
    mask = torch.from_numpy((np.arange(E) % 2 == 0).astype(np.uint8))
    for t in range(T):
        if t == 6:  # every env has ended (step limit 5, no auto-reset): half of them come back
            assert (sims[1].flags.cpu().numpy() & 1).sum() == 0
            outs = [s.reset(mask) for s in sims]
            _agree(sims, outs, f"masked reset t{t}")
        acts = torch.from_numpy(parity.lane_actions(rng, E, N)).cuda()
        outs = [s.step(acts) for s in sims]
        _agree(sims, outs, f"t{t}")
        if t == 6:
            assert outs[1]["active"].cpu().numpy().reshape(E, N)[::2].any()  # the respawned envs' agents moved on
    for s in sims:
        s.close()

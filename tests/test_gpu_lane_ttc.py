"""SMX_SENSOR_LANE_TTC on the device (k_lane_ttc): ``out["lane_ttc"]`` / ``out["lane_ttc_flags"]`` against
``lane_ttc_rows`` applied to the device's own dense rows of the same tick — no oracle rollout, so closed-loop drift
does not enter.  Flags exact, values within 1e-9 except on margin-sensitive agent-ticks (lane_ttc_check), which are
left out, counted and capped at 1 %.  One case per launch path: the small form, the two cuts of the large form, a map
with junctions, social traffic, truncated rows, the first observation, the reset pass under auto_reset and after a
masked reset, and per-phase timing (the unforked tick)."""
import numpy as np
import pytest
import torch

import lane_ttc_check as chk
import parity
from smarts_amd import _native as nat
from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

pytestmark = pytest.mark.gpu


def _sim(compiled_maps, name, E, N, seed, slow_odd_slots=False, **kw):
    cm = compiled_maps(name)
    base = dict(neighbors=True, nb_radius=50.0, wp_paths=4, wp_len=33, lane_ttc=True)
    base.update(kw)
    cfg = SimConfig(num_envs=E, num_vehicles=N, **base)
    spawns, where = make_spawns(cm, E, N, episodes=2, seed=seed, return_lanes=True)
    if slow_odd_slots:  # every second vehicle starts at 8 m/s instead of the speed limit: closing speeds at the reset already
        spawns[..., 3] = np.where(np.arange(E * N) % 2 == 1, 8.0, spawns[..., 3])
    return BatchedSim(cm, cfg, spawns=spawns, social_spawns=where if cfg.num_social else None), cfg


def _check(rows, cfg, where):
    return chk.compare(rows["lane_ttc"], rows["lane_ttc_flags"], rows, cfg, where=where)


def _assert_counts(totals, where, min_non_default=1):
    """What every case owes: at most 1 % of its valid agent-ticks left out, and a compared row with a real ttc."""
    valid, left_out, non_default = (int(x) for x in totals)
    assert left_out <= chk.MAX_LEFT_OUT * valid, (where, left_out, valid)
    assert non_default >= min_non_default, (where, non_default)  # not vacuous


def _run(sim, cfg, ticks, seed, where, min_non_default=1):
    """Reset + `ticks` ticks of parity.lane_actions, every pass compared; returns the rows of every pass."""
    E, N = cfg.num_envs, cfg.num_vehicles
    rng = np.random.default_rng(seed)
    passes = [parity.host(sim.reset())]
    totals = np.array(_check(passes[0], cfg, f"{where} reset"))
    for t in range(ticks):
        passes.append(parity.host(sim.step(torch.from_numpy(parity.lane_actions(rng, E, N)).cuda())))
        totals += _check(passes[-1], cfg, f"{where} t{t}")
    sim.sync()
    _assert_counts(totals, where, min_non_default)
    return passes


@pytest.mark.parametrize("strategy,form", [("small", "small"), ("large_one_lane", "large_one_lane"), ("large_teams", "large_teams")])
def test_loop_in_every_launch_form(strategy, form, compiled_maps):
    sim, cfg = _sim(compiled_maps, "loop", 2, 32, 3, launch_strategy=strategy)
    assert sim.launch_form() == form
    for rows in _run(sim, cfg, 10, 3, f"loop {form}"):
        # whole paths are kept (33 waypoints, at most four paths on this map): only an eleventh neighbour truncates
        assert np.array_equal((rows["lane_ttc_flags"] & nat.TTC_TRUNCATED) != 0,
                              ((rows["lane_ttc_flags"] & nat.TTC_VALID) != 0) & (rows["nb_count"] > cfg.nb_max))
    sim.close()


def test_4lane_junction_paths(compiled_maps):
    sim, cfg = _sim(compiled_maps, "4lane", 2, 16, 11)
    fanned = 0
    for rows in _run(sim, cfg, 6, 11, "4lane"):
        # several paths per lane index: an agent that holds more paths than its first waypoints have lane indices
        n_paths = np.minimum(rows["wp_count"][:, 0], cfg.wp_paths)
        top = np.where(np.arange(cfg.wp_paths)[None, :] < n_paths[:, None], rows["wp_lane_index"][:, :, 0], -1).max(1)
        fanned += int((n_paths > top + 1).sum())
    assert fanned >= 5, fanned
    sim.close()


def test_slow_social_leaders_give_real_ttc(compiled_maps):
    sim, cfg = _sim(compiled_maps, "loop", 2, 8, 5, num_social=3, social_speed_factor=0.5)
    social = np.tile(np.arange(8) >= 5, 2)
    for rows in _run(sim, cfg, 10, 5, "social", min_non_default=5):
        assert not rows["lane_ttc_flags"][social].any()  # a social vehicle has no observation
    sim.close()


@pytest.mark.parametrize("kw", [dict(wp_paths=2, nb_max=2), dict(wp_len=20, wp_lookahead=32)], ids=["rows", "window"])
def test_truncated_rows_are_flagged_where_the_counts_say(kw, compiled_maps):
    sim, cfg = _sim(compiled_maps, "loop", 2, 32, 3, **kw)
    rng = np.random.default_rng(3)
    rows = parity.host(sim.reset())
    seen = 0
    totals = np.zeros(3, dtype=np.int64)
    for t in range(4):
        valid = (rows["lane_ttc_flags"] & nat.TTC_VALID) != 0
        want = (rows["wp_count"][:, 0] > cfg.wp_paths) | (rows["nb_count"] > cfg.nb_max) | (cfg.wp_len < cfg.wp_lookahead + 1)
        assert np.array_equal((rows["lane_ttc_flags"] & nat.TTC_TRUNCATED) != 0, valid & want), t
        seen += int((valid & want).sum())
        totals += _check(rows, cfg, f"truncated {kw} t{t}")
        rows = parity.host(sim.step(torch.from_numpy(parity.lane_actions(rng, 2, 32)).cuda()))
    assert seen >= 64, seen
    _assert_counts(totals, f"truncated {kw}")
    sim.close()


def test_first_observation_after_reset(compiled_maps):
    sim, cfg = _sim(compiled_maps, "loop", 2, 32, 7, slow_odd_slots=True)
    rows = parity.host(sim.reset())
    assert ((rows["lane_ttc_flags"] & nat.TTC_VALID) != 0).all()
    totals = _check(rows, cfg, "first observation")
    assert totals[0] == 64
    _assert_counts(totals, "first observation")  # (of 64 rows: none left out)
    sim.close()


def test_reset_pass_rewrites_the_rows_of_a_restarted_env(compiled_maps):
    """auto_reset with max_episode_steps=4, and env 0 put out of step with env 1 by a masked reset — the two share an
    env group of the reset pass: on the tick an env restarts its rows are lane_ttc of the new episode's first
    observation, and the env beside it keeps its tick's."""
    sim, cfg = _sim(compiled_maps, "loop", 2, 32, 9, auto_reset=True, max_episode_steps=4)
    E, N = 2, 32
    rng = np.random.default_rng(9)
    parity.host(sim.reset())
    totals = np.zeros(3, dtype=np.int64)
    restarts = np.zeros(E, dtype=np.int64)
    alone = 0
    for t in range(9):
        if t == 2:
            rows = parity.host(sim.reset(torch.tensor([1, 0], dtype=torch.uint8)))
            totals += _check(rows, cfg, "masked reset")
            assert ((rows["lane_ttc_flags"][:N] & nat.TTC_VALID) != 0).all()
        out = sim.step(torch.from_numpy(parity.lane_actions(rng, E, N)).cuda())
        rows = parity.host(out)
        env_done = out["env_done"].cpu().numpy() != 0
        totals += _check(rows, cfg, f"auto_reset t{t} restarted {env_done.tolist()}")
        for e in np.flatnonzero(env_done):
            mine = slice(e * N, (e + 1) * N)
            # the first observation of the next episode: every agent is back, at its spawn pose of that episode
            assert ((rows["lane_ttc_flags"][mine] & nat.TTC_VALID) != 0).all(), (t, e)
            assert rows["active"][mine].all(), (t, e)
        restarts += env_done
        alone += int(env_done.sum() == 1)
    sim.sync()
    assert (restarts >= 1).all() and alone >= 2, (restarts, alone)  # each env restarted, and did so without the other
    _assert_counts(totals, "auto_reset")
    sim.close()


@pytest.mark.parametrize("strategy", ["small", "large_one_lane"])
def test_phase_timing_changes_no_bit(strategy, compiled_maps):
    """smx_set_timing(2): the tick without a fork, a boundary event after every kernel."""
    sims = [_sim(compiled_maps, "loop", 2, 32, 3, launch_strategy=strategy) for _ in range(2)]
    sims[1][0].set_timing(2)
    acts = torch.from_numpy(parity.lane_actions(np.random.default_rng(3), 2, 32)).cuda()
    got = []
    for sim, cfg in sims:
        sim.reset()
        rows = parity.host(sim.step(acts))
        _assert_counts(_check(rows, cfg, f"timing {strategy}"), f"timing {strategy}")
        got.append(rows)
    assert sims[1][0].read_phase_ms().shape == (1, len(nat.PHASES))
    assert np.array_equal(got[0]["lane_ttc_flags"], got[1]["lane_ttc_flags"])
    valid = (got[0]["lane_ttc_flags"] & nat.TTC_VALID) != 0
    assert np.array_equal(got[0]["lane_ttc"][valid], got[1]["lane_ttc"][valid])
    for sim, _ in sims:
        sim.close()

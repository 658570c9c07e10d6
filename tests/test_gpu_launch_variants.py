"""Launch variants of one tick that must not change a bit of it.

The large form (smx_plan.h tick_plan(), issued by smx_kernels.hip enqueue()) picks its launches at run time: the cut (one lane per vehicle or teams),
whether the one-lane path-seeds kernel and its slow seeds chain run, which row kernels run (k_wp_walk ->
k_waypoints_emit up to SMX_WPT_MAX_PATHS = 8 rows, k_waypoints past them) and whether the grid maps, the lidar and the
slow seeds chain leave on side streams or run on the caller's stream, as they do at per-kernel timing
(smx_set_timing(2)).  Here each combination is held to the same batch at timing 0, or to the small form, bit for bit
over auto-reset ticks, on maps where a third of the vehicles goes through the slow lists (4lane, minicity), and the
rows past eight on a split map are held to the oracle teacher-forced.  Every test first asserts the form it runs.
"""
import ctypes as C

import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

FORMS = ("small", "large_one_lane", "large_teams")
OGM64 = dict(ogm=True, ogm_width=64, ogm_height=64, ogm_resolution=50 / 64)
TOL_RESET = dict(tol64=1e-9, tol32=2e-6)
TOL_TICK = dict(tol64=1e-9, tol32=2e-5)


def _sims(name, E, N, strategies, compiled_maps, seed, **extra):
    """One batch per launch strategy, all on the same seeded spawns (three episodes: auto-reset restarts)."""
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns
    from smarts_amd.lidar import Planar100

    extra = dict(extra)
    if extra.get("lidar") == "planar100":
        extra["lidar"] = Planar100
    cm = compiled_maps(name)
    spawns = make_spawns(cm, E, N, episodes=3, seed=seed)
    sims = [BatchedSim(cm, SimConfig(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, auto_reset=True,
                                     launch_strategy=s, **extra), spawns=spawns) for s in strategies]
    assert [s.launch_form() for s in sims] == list(strategies)
    return sims


def _assert_same(sims, outs, where):
    """Every output, the whole state and the flags of sims[1:] equal sims[0]'s, bit for bit."""
    import torch

    torch.cuda.synchronize()
    ref = {k: v.cpu().numpy() for k, v in outs[0].items()}
    st, fl = sims[0].state.cpu().numpy(), sims[0].flags.cpu().numpy()
    for i in range(1, len(sims)):
        for k, a in ref.items():
            assert np.array_equal(a, outs[i][k].cpu().numpy(), equal_nan=True), (where, i, k)
        assert np.array_equal(st, sims[i].state.cpu().numpy(), equal_nan=True), (where, i, "state")
        assert np.array_equal(fl, sims[i].flags.cpu().numpy()), (where, i, "flags")


def _slow_counts(sim):
    """[facts, seeds, control, rows]: the lengths of the last tick's slow lists (developer entry point)."""
    fn = sim.lib.smx_debug_slow_counts
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    buf = (C.c_int32 * 4)()
    assert fn(sim.handle, buf) == 0
    return list(buf)


def _switching(t):
    """The level of the fourth batch at tick t: 0 -> 2 -> 1 -> 0 ..., three ticks each."""
    return (0, 2, 1)[(t // 3) % 3]


BATCHES = {
    # C4's shape: k_ogm_env moves from side stream 0 to the caller's stream
    "loop_ogm": ("loop", 6, 32, OGM64),
    # long slow lists: about a third of the vehicles through the slow seeds chain in the one-lane cut
    "minicity": ("minicity", 12, 16, {}),
    # k_lidar moves stream too
    "minicity_lidar": ("minicity", 8, 16, dict(lidar="planar100")),
}


@pytest.mark.parametrize("batch", sorted(BATCHES))
@pytest.mark.parametrize("form", FORMS)
def test_timing_level_changes_no_bit(batch, form, compiled_maps):
    """The same batch at timing 0, 1, 2 and switched between levels every three ticks: at level 2 the large form runs
    unforked (grids, lidar and the serial slow seeds chain on the caller's stream); no output, state or flag may
    differ.  read_phase_ms / read_step_ms must return one row per tick stepped at level 2 / 1 since the last read,
    which proves the levels were on."""
    import torch

    name, E, N, extra = BATCHES[batch]
    sims = _sims(name, E, N, (form,) * 4, compiled_maps, 41, **extra)
    for s, level in zip(sims, (0, 1, 2, 0)):
        s.set_timing(level)
        s.reset()
    rng = np.random.default_rng(41)
    T = 42
    since = dict(steps=0, switched=0)
    for t in range(T):
        sims[3].set_timing(_switching(t))
        since["switched"] += _switching(t) == 2
        since["steps"] += 1
        acts = torch.from_numpy(parity.lane_actions(rng, E, N)).cuda()
        outs = [s.step(acts) for s in sims]
        if t % 7 == 0 or t == T - 1:
            _assert_same(sims, outs, f"{batch} {form} t{t}")
            assert len(sims[1].read_step_ms()) == since["steps"]
            assert sims[2].read_phase_ms().shape[0] == since["steps"]
            assert sims[3].read_phase_ms().shape[0] == since["switched"]
            since = dict(steps=0, switched=0)
    for s in sims:
        s.close()


ROWS = [(8, 10), (9, 12), (16, 1), (64, 33)]  # the last staged count, the first k_waypoints one, one waypoint, the maximum


@pytest.mark.parametrize("name", ["4lane", "minicity"])
@pytest.mark.parametrize("rows", ROWS, ids=[f"{p}x{w}" for p, w in ROWS])
def test_rows_around_the_staged_limit_agree_with_the_small_form(name, rows, compiled_maps):
    """Both large cuts at timing 0 and 2 against the small form, at row counts on either side of SMX_WPT_MAX_PATHS, on
    maps with branchings and junction roads.  The slow lists must have been populated in the one-lane cut: the facts
    list on most ticks on minicity, and the seeds list on most ticks while the rows are staged (else the slow seeds
    chain was never reached).  Past eight rows the team seeds kernel serves every vehicle."""
    import torch

    P, W = rows
    E, N, T = 12, 16, 30
    strategies = ("small", "large_one_lane", "large_one_lane", "large_teams", "large_teams")
    sims = _sims(name, E, N, strategies, compiled_maps, 43, wp_paths=P, wp_len=W)
    for s, level in zip(sims, (0, 0, 2, 0, 2)):
        s.set_timing(level)
        s.reset()
    rng = np.random.default_rng(43)
    counts = {1: [], 2: []}  # the one-lane sims' slow-list lengths, tick by tick
    for t in range(T):
        acts = torch.from_numpy(parity.lane_actions(rng, E, N)).cuda()
        outs = [s.step(acts) for s in sims]
        for i in counts:
            counts[i].append(_slow_counts(sims[i]))
        if t % 7 == 0 or t == T - 1:
            _assert_same(sims, outs, f"{name} {P}x{W} t{t}")
    # (on 4lane no vehicle reaches a junction road inside the run: its facts list stays empty, and its slow traffic is
    # the seeds list — branchings, new roads)
    for i in counts:
        c = np.array(counts[i])
        if name == "minicity":
            assert (c[:, 0] > 0).sum() >= 0.75 * T, (i, c[:, 0].tolist())
        if P <= 8:
            assert (c[:, 1] > 0).sum() >= 0.75 * T, (i, c[:, 1].tolist())
    for s in sims:
        s.close()


@pytest.mark.parametrize("name,E,N,P,W,T,form,level", [
    ("minicity", 2, 16, 9, 12, 15, "small", 0),
    ("minicity", 2, 16, 9, 12, 15, "small", 2),
    ("minicity", 2, 16, 9, 12, 15, "large_one_lane", 0),
    ("minicity", 2, 16, 9, 12, 15, "large_one_lane", 2),
    ("4lane", 2, 8, 64, 33, 12, "large_one_lane", 0),
    ("4lane", 2, 8, 64, 33, 12, "large_one_lane", 2),
])
def test_rows_past_eight_against_the_oracle(name, E, N, P, W, T, form, level, nets, compiled_maps):
    """Rows past SMX_WPT_MAX_PATHS on split maps, teacher-forced against the oracle: float64 to 1e-9, float32 to 2e-6
    on reset and 2e-5 on ticks, integers, counts and flags exact."""
    import torch

    sim, ob, cfg = parity.make(name, E, N, nets, compiled_maps, 47, launch_strategy=form, wp_paths=P, wp_len=W)
    assert sim.launch_form() == form
    sim.set_timing(level)
    bad = parity.compare(parity.host(sim.reset()), ob.reset_observe(), where="reset ", **TOL_RESET)
    assert bad == [], "\n".join(bad[:8])
    rng = np.random.default_rng(47)
    for t in range(T):
        acts = parity.lane_actions(rng, E, N)
        if t % 5 == 2:
            acts[0, 0] = -1
        d, o = parity.host(sim.step(torch.from_numpy(acts).cuda())), ob.step(acts)
        bad = parity.compare(d, o, where=f"{name} {form} timing {level} t{t} ", **TOL_TICK)
        assert bad == [], "\n".join(bad[:8])
        parity.sync_oracle_from_device(ob, sim)
    sim.close()

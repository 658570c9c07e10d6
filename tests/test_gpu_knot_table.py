"""The one-lane cut's knot lists from the map's knot table (smx_roadmap.h KnotRow, k_knot_table).

k_waypoints_emit and k_control_fast read the row of a start lanepoint instead of the list k_wp_walk walked for the
vehicle; the vehicles no row serves (branchings, a filter other than the row's, fixed routes, more knots than a row
holds) take the slow lists as before.  No bit may change: every case runs the same seeded batch three times — table on,
table off (smx_debug_set_knot_table, the walked lists of before) and the SMALL form — and compares the whole state, the
flags and every output after the reset and after every tick.
"""
import ctypes as C

import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

TICKS = 30


def _switch(sim, mode):
    fn = sim.lib.smx_debug_set_knot_table
    fn.argtypes = [C.c_void_p, C.c_int32]
    assert fn(sim.handle, mode) == 0


def _stats(sim):
    """[rows, rows tabled, tabled rows on one road, path lanes served while the switch was 2]"""
    fn = sim.lib.smx_debug_knot_table_stats
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    buf = (C.c_int64 * 4)()
    assert fn(sim.handle, buf) == 0
    return list(buf)


def _slow_counts(sim):
    fn = sim.lib.smx_debug_slow_counts
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    buf = (C.c_int32 * 4)()
    assert fn(sim.handle, buf) == 0
    return list(buf)


def _fixed_routes(cm, N):
    """every slot a fixed route over every road of the map (a goal nobody reaches): no vehicle is tabled"""
    from smarts_amd.missions import PlannedMission

    return [PlannedMission((0.0, 0.0), 0.0, (1e7, 1e7, 1.0), tuple(cm.road_ids)) for _ in range(N)]


CASES = {
    "loop": ("loop", 4, 8, "large_one_lane", {}, None, False),
    # branchings and junction filters: every fallback
    "minicity": ("minicity", 2, 16, "large_one_lane", {}, None, False),
    "4lane": ("4lane", 3, 7, "large_one_lane", {}, None, False),
    "loop_rows": ("loop", 4, 8, "large_one_lane", dict(wp_paths=8, wp_len=12), None, False),
    "loop_pool": ("loop", 4, 8, "large_one_lane", {}, 40, False),
    "loop_routed": ("loop", 4, 8, "large_one_lane", {}, None, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_table_on_off_and_small_form_agree_bit_for_bit(case, compiled_maps):
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    name, E, N, form, extra, pool, routed = CASES[case]
    cm = compiled_maps(name)
    spawns = make_spawns(cm, E, N, episodes=3, seed=151)
    missions = _fixed_routes(cm, N) if routed else None
    sims = [BatchedSim(cm, SimConfig(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0, auto_reset=True,
                                     launch_strategy=s, **extra), spawns=spawns, missions=missions)
            for s in (form, form, "small")]
    assert [s.launch_form() for s in sims] == [form, form, "small"]
    _switch(sims[0], 2)  # the table, counting the path lanes it serves
    _switch(sims[1], 0)  # the walked lists
    if pool is not None:
        for s in sims[:2]:
            s.lib.smx_debug_set_wp_pool.argtypes = [C.c_void_p, C.c_int32]
            assert s.lib.smx_debug_set_wp_pool(s.handle, pool) == 0

    def same(outs, where):
        torch.cuda.synchronize()
        ref = {k: v.cpu().numpy() for k, v in outs[0].items()}
        st, fl = sims[0].state.cpu().numpy(), sims[0].flags.cpu().numpy()
        for i in (1, 2):
            for k, a in ref.items():
                assert np.array_equal(a, outs[i][k].cpu().numpy(), equal_nan=True), (case, where, i, k)
            assert np.array_equal(st, sims[i].state.cpu().numpy(), equal_nan=True), (case, where, i, "state")
            assert np.array_equal(fl, sims[i].flags.cpu().numpy()), (case, where, i, "flags")

    same([s.reset() for s in sims], "reset")
    rng = np.random.default_rng(151)
    longer = []
    for t in range(TICKS):
        acts = torch.from_numpy(parity.lane_actions(rng, E, N)).cuda()
        same([s.step(acts) for s in sims], f"t{t}")
        on, off = _slow_counts(sims[0]), _slow_counts(sims[1])
        if name == "loop" and (on[2] > off[2] or on[3] > off[3]):  # control, rows
            longer.append((t, on, off))
    rows, tabled, one_road, served = _stats(sims[0])
    assert 0 < tabled <= rows and 0 <= one_road <= tabled
    if name == "loop":
        assert longer == [], longer[:4]
        if routed:
            assert served == 0  # a fixed route is never tabled
        else:
            assert served > 0  # path lanes of vehicle-ticks served from rows
    assert _stats(sims[1])[3] == 0
    for s in sims:
        s.close()

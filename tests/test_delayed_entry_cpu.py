"""Delayed agent entry without a GPU: the trap countdown (``missions.entry_ticks``), the tables ``missions.entry_table``
builds for ``BatchedSim.set_agent_entry``, the mission types' new fields, and the NumPy model the GPU tests decide their
cases with (tests/delayed_entry_ref.py)."""
import math

import numpy as np
import pytest

import delayed_entry_ref as ref
from smarts_amd.missions import (CHASSIS_LENGTH, EndlessMission, LapMission, Mission, Route, TrapEntryTactic, TraverseMission,
                                 entry_table, entry_ticks, load_missions, plan_mission)

# (start_time, wait_to_hijack_limit_s, dt) -> the step the trap fires on, by the repeated float64 subtraction of
# Trap.step_trigger and the tests ready / patience_expired (trap_manager.py:53-65)
PINNED = [((0.3, 0.0, 0.1), 3), ((2.0, 0.0, 0.1), 20), ((0.1, 0.0, 0.1), 2), ((0.7, 0.0, 0.1), 8), ((0.5, 0.2, 0.1), 8),
          ((1.2, 0.3, 0.1), 16), ((0.1, 0.0, 0.01), 11)]


def _closed_form(t, dt):
    """SimConfig.reset_elapsed_steps' formula, floor(t / dt + 1e-9) + 1."""
    return int(math.floor(t / dt + 1e-9)) + 1


@pytest.mark.parametrize("args,want", PINNED)
def test_entry_ticks_pinned(args, want):
    assert entry_ticks(*args) == want


@pytest.mark.parametrize("t,want", [(0.3, 3), (2.0, 20)])
def test_entry_ticks_is_the_subtraction_not_the_closed_form(t, want):
    """0.3 - 0.1 - 0.1 - 0.1 is -2.8e-17 < 0: the trap fires on step 3, where t / dt says 4 (and 21 for 2.0 s)."""
    assert entry_ticks(t, 0.0, 0.1) == want
    assert _closed_form(t, 0.1) == want + 1
    assert entry_ticks(t, 0.0, 0.1) != _closed_form(t, 0.1)


def test_default_start_time_matches_the_reset_steps_of_today():
    """The default mission (0.1 s, no patience) fires on the step SimConfig.reset_elapsed_steps() burns today."""
    from smarts_amd.engine import SimConfig

    for dt in (0.1, 0.05, 0.04, 0.2):
        assert entry_ticks(0.1, 0.0, dt) == SimConfig(num_envs=1, num_vehicles=1, dt=dt).reset_elapsed_steps()
    assert SimConfig(num_envs=1, num_vehicles=1, entry_reset_steps=7).reset_elapsed_steps() == 7


def test_entry_ticks_refuses_a_bad_step():
    with pytest.raises(ValueError):
        entry_ticks(0.1, 0.0, 0.0)
    with pytest.raises(ValueError):
        entry_ticks(float("nan"), 0.0, 0.1)


def test_trap_zone_is_refused():
    with pytest.raises(ValueError, match="zone"):
        TrapEntryTactic(1.0, zone=object())
    with pytest.raises(ValueError):
        TrapEntryTactic(-1.0)
    t = TrapEntryTactic(0.5, default_entry_speed=3.0)
    assert t.zone is None and t.exclusion_prefixes == () and t.default_entry_speed == 3.0


def test_missions_without_the_new_fields_are_todays():
    r = Route(("a", 0, 1.0), ("b", 1, "max"))
    assert Mission(r) == Mission(r, 0.1, None) and Mission(r).start_time == 0.1 and Mission(r).entry_tactic is None
    assert EndlessMission(("a", 0, 1.0)) == EndlessMission(("a", 0, 1.0), (), 0.1, None)
    assert LapMission(r, 2) == LapMission(r, 2, (), 0.1, None)
    assert TraverseMission(("a", 0, 1.0)) == TraverseMission(("a", 0, 1.0), 0.1, None)
    assert Mission(r, start_time=0.7) != Mission(r)
    # the JSON form: without the keys, today's missions; with them, the fields
    spec = {"A": {"begin": ["a", 0, 1.0], "end": ["b", 1, "max"]},
            "B": {"type": "endless", "begin": ["a", 0, 1.0], "start_time": 0.7,
                  "entry_tactic": {"wait_to_hijack_limit_s": 0.2, "default_entry_speed": 4.0}}}
    got = load_missions(spec)
    assert got["A"] == Mission(r)
    assert got["B"] == EndlessMission(("a", 0, 1.0), start_time=0.7, entry_tactic=TrapEntryTactic(0.2, default_entry_speed=4.0))


@pytest.fixture(scope="module")
def loop_scene(nets):
    net = nets("loop")
    missions = [EndlessMission(begin=("445633931", 0, 10.0)),  # start_time 0.1: fires on step 2
                EndlessMission(begin=("445633932", 0, 30.0), start_time=0.7,
                               entry_tactic=TrapEntryTactic(0.2, default_entry_speed=5.0))]  # 0.7 + 0.2: step 10
    planned = [plan_mission(net, m) for m in missions]
    return missions, planned


def test_entry_table_on_loop(loop_scene):
    missions, planned = loop_scene
    E = 3
    dims = np.full((2, E, 2, 3), np.nan)
    dims[1, :, 1] = (10.0, 2.5, 4.0)  # the second episode's agent 1 is a trailer
    dims[0, 1, 0] = (2.0, 3.0, 1.5)   # env 1's agent 0 is wider than long in the first
    t = entry_table(missions, planned, E, 0.1, dims)
    assert t.steps == (2, 10) and t.reset_steps == 2 and t.differs
    assert t.ready.dtype == np.int32 and t.ready.shape == (2, E, 2)
    assert (t.ready[..., 0] == 0).all() and (t.ready[..., 1] == 8).all()
    assert ((t.ready == 0).any(axis=2)).all()  # every (row, env) has an agent at the reset observation
    assert t.entry_speed == (None, 5.0)
    assert t.check.dtype == np.float64 and t.check.shape == (2, E, 2, 3)
    for a in range(2):
        # the check point is the mission's start (the front bumper), half a length ahead of the spawn centre
        assert (t.check[:, :, a, 0] == planned[a].start_position[0]).all()
        assert (t.check[:, :, a, 1] == planned[a].start_position[1]).all()
        cx, cy, _ = planned[a].spawn_pose()
        assert math.hypot(t.check[0, 0, a, 0] - cx, t.check[0, 0, a, 1] - cy) == pytest.approx(0.5 * CHASSIS_LENGTH, abs=1e-9)
    # the largest plane dimension: the agent_dims row where it has one, else the sedan's 3.68 x 1.47
    assert t.check[1, 0, 1, 2] == 10.0 and t.check[0, 0, 1, 2] == 3.68
    assert t.check[0, 1, 0, 2] == 3.0 and t.check[0, 0, 0, 2] == 3.68 and t.check[1, 1, 0, 2] == 3.68
    # equal start times: nothing worth binding
    same = entry_table([missions[0], missions[0]], [planned[0], planned[0]], E, 0.1)
    assert not same.differs and (same.ready == 0).all() and same.reset_steps == 2


def test_entry_table_needs_a_start_point_for_a_late_agent(loop_scene):
    missions, planned = loop_scene
    with pytest.raises(ValueError, match="planned mission"):
        entry_table(missions, [planned[0], None], 1, 0.1)
    t = entry_table(missions, [None, planned[1]], 1, 0.1)  # the early agent is never checked
    assert t.ready[0, 0].tolist() == [0, 8]


def test_check_refuses_what_the_device_cannot_take():
    """``engine.check_agent_entry`` (smx_check_agent_entry): each refusal with its reason."""
    from smarts_amd.engine import check_agent_entry

    ready = np.zeros((1, 2, 2), dtype=np.int32)
    ready[0, :, 1] = 3
    check = np.zeros((1, 2, 2, 3))
    check[..., 2] = 3.68
    check_agent_entry(2, 3, 1, ready, check)
    bad = ready.copy()
    bad[0, 1, 1] = -1
    with pytest.raises(ValueError, match="negative"):
        check_agent_entry(2, 3, 1, bad, check)
    bad = ready.copy()
    bad[0, 1, 0] = 2
    with pytest.raises(ValueError, match="no agent at tick 0"):
        check_agent_entry(2, 3, 1, bad, check)
    c = check.copy()
    c[0, 0, 1, 0] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        check_agent_entry(2, 3, 1, ready, c)
    c = check.copy()
    c[0, 0, 1, 2] = 0.0
    with pytest.raises(ValueError, match="> 0"):
        check_agent_entry(2, 3, 1, ready, c)
    with pytest.raises(ValueError, match="shape"):
        check_agent_entry(2, 3, 1, ready[:0], check[:0])


def test_model_pending_blocked_entered():
    """The NumPy model on a made-up scene: one slot drives over agent 1's start point and on."""
    ready = np.array([[0, 3, 1]])
    check = np.array([[[0.0, 0.0, 3.68], [10.0, 0.0, 3.68], [-50.0, 0.0, 3.68]]])
    T = 8
    xs = np.array([0.0, 4.0, 8.0, 11.0, 14.0, 17.0, 20.0, 23.0])  # the slot's x in ticks 1..8 (y = 0.5)
    xy = np.zeros((T, 1, 1, 2))
    xy[:, 0, 0, 0], xy[:, 0, 0, 1] = xs, 0.5
    alive = np.ones((T, 1, 1), dtype=bool)
    status, entered, clearance = ref.run(ready, check, xy, alive)
    # radius 0.5 * (3.68 + 3.68); distances from (10, 0) in ticks 3, 4, 5: 2.06, 1.12, 4.03 -> blocked twice, enters at 5
    assert status[0].tolist() == [[ref.ENTERED, ref.PENDING, ref.PENDING]]
    assert status[1].tolist() == [[ref.ENTERED, ref.PENDING, ref.ENTERED]]
    assert [int(status[t, 0, 1]) for t in range(T + 1)] == [0, 0, 0, 1, 1, 2, 2, 2, 2]
    assert entered.tolist() == [[0, 5, 1]]
    want = min([abs(math.hypot(x - 10.0, 0.5) - 3.68) for x in xs[2:5]] + [abs(math.hypot(50.0, 0.5) - 3.68)])
    assert clearance == want and clearance > 1e-6
    # a dead slot blocks nobody; a longer box blocks longer (radius 0.5 * (12 + 3.68) = 7.84: 4.03 and 7.02 block)
    status, entered, _ = ref.run(ready, check, xy, np.zeros_like(alive))
    assert entered.tolist() == [[0, 3, 1]]
    status, entered, _ = ref.run(ready, check, xy, alive, np.array([[[12.0, 2.0]]]))
    assert entered.tolist() == [[0, 7, 1]]

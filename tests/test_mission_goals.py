"""EndlessMission, LapMission and TraverseMission on the host: planning (smarts_amd/missions.py) against the
reference's own ``Scenario._extract_mission`` / ``Plan.create_route`` (tests/golden/mission_goals_plan.npz), the
plain-Python restatement of the two goal tests (tests/mission_goals_ref.py) against the reference's
``LapMission.is_complete`` and ``TraverseGoal._drove_off_map`` (mission_goals_lap.npz, mission_goals_traverse.npz,
written by tests/golden/gen_golden_mission_goals.py), and the C-ABI's validation of the goal table."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mission_goals_ref as ref
from conftest import GOLDEN


def _offset(text):
    return text if text in ("base", "max") else float(text)


def test_lap_missions_plan_as_the_reference_does(nets):
    from smarts_amd.missions import GOAL_LAP, LapMission, Route, plan_mission

    g = np.load(os.path.join(GOLDEN, "mission_goals_plan.npz"))
    net = nets("loop")
    shared = 0
    for k, (spec, row) in enumerate(zip(g["lap_spec"], g["lap_rows"])):
        spec = [str(s) for s in spec]
        via = tuple(v for v in spec[6].split(",") if v)
        m = LapMission(Route(begin=(spec[0], int(spec[1]), _offset(spec[2])), end=(spec[3], int(spec[4]), _offset(spec[5])),
                             via=via), num_laps=int(row[7]))
        p = plan_mission(net, m)
        # floats bit for bit: same arithmetic, same libm
        assert np.array_equal(np.array([*p.start_position, p.start_heading, *p.goal, p.route_length]), row[:7]), (k, spec)
        assert p.goal_kind == GOAL_LAP and p.num_laps == int(row[7])
        roads = [str(r) for r in g["lap_route_roads"][g["lap_route_off"][k]:g["lap_route_off"][k + 1]]]
        assert list(p.route_roads) == roads, (k, spec)
        shared += spec[0] == spec[3]
    assert shared >= 3  # begin and end on one road: the lap is measured from the first outgoing road


@pytest.mark.parametrize("name", ["4lane", "minicity"])
def test_endless_and_traverse_missions_start_where_the_reference_starts_them(name, nets):
    from smarts_amd.missions import GOAL_POSITIONAL, GOAL_TRAVERSE, EndlessMission, TraverseMission, plan_mission

    g = np.load(os.path.join(GOLDEN, "mission_goals_plan.npz"))
    for spec, row in zip(g[f"endless_{name}_spec"], g[f"endless_{name}_rows"]):
        begin = (str(spec[0]), int(spec[1]), _offset(str(spec[2])))
        for mission, kind in ((EndlessMission(begin), GOAL_POSITIONAL), (TraverseMission(begin), GOAL_TRAVERSE)):
            p = plan_mission(nets(name), mission)
            assert np.array_equal(np.array([*p.start_position, p.start_heading]), row), begin
            assert p.route_roads == () and p.goal_kind == kind  # is_endless(): an empty route (plan.py:321-323)


def test_planned_mission_defaults_mean_a_positional_goal():
    from smarts_amd.missions import GOAL_POSITIONAL, PlannedMission

    p = PlannedMission((0.0, 0.0), 0.0, (1.0, 2.0, 2.0), ("a",))
    assert (p.goal_kind, p.route_length, p.num_laps) == (GOAL_POSITIONAL, 0.0, 0)


def test_lap_mission_refusals(nets):
    from smarts_amd.missions import EndlessMission, LapMission, Route, plan_mission

    route = Route(begin=("445633931", 0, 10), end=("445633932", 0, 30))
    for laps in (None, 0, -1, 1.5, True):
        with pytest.raises(ValueError, match="num_laps"):
            plan_mission(nets("loop"), LapMission(route, num_laps=laps))
    with pytest.raises(ValueError, match="random"):
        plan_mission(nets("loop"), LapMission(Route(begin=("445633931", 0, "random"), end=route.end), num_laps=1))
    with pytest.raises(ValueError, match="random"):
        plan_mission(nets("loop"), EndlessMission(begin=("445633931", 0, "random")))
    with pytest.raises(TypeError):
        plan_mission(nets("loop"), object())


def test_load_missions_round_trip(tmp_path):
    from smarts_amd.missions import EndlessMission, LapMission, Mission, Route, TraverseMission, load_missions

    spec = {
        "old": {"begin": ["a", 0, 10], "end": ["b", 1, "max"], "via": ["c"]},
        "typed": {"type": "mission", "begin": ["a", 0, 10], "end": ["b", 1, "max"]},
        "lap": {"type": "lap", "begin": ["a", 0, 10], "end": ["a", 0, 5], "num_laps": 3},
        "endless": {"type": "endless", "begin": ["a", 1, "base"]},
        "traverse": {"type": "traverse", "begin": ["a", 1, 2.5]},
    }
    path = tmp_path / "missions.json"
    path.write_text(json.dumps(spec))
    for source in (spec, str(path)):
        ms = load_missions(source)
        assert ms["old"] == Mission(Route(("a", 0, 10), ("b", 1, "max"), ("c",)))  # no "type": today's format
        assert ms["typed"] == Mission(Route(("a", 0, 10), ("b", 1, "max")))
        assert ms["lap"] == LapMission(Route(("a", 0, 10), ("a", 0, 5)), num_laps=3)
        assert ms["endless"] == EndlessMission(("a", 1, "base")) and ms["traverse"] == TraverseMission(("a", 1, 2.5))
    assert load_missions({"x": {"type": "lap", "begin": ["a", 0, 1], "end": ["a", 0, 2]}})["x"].num_laps is None  # refused when planned
    with pytest.raises(ValueError, match="unknown type"):
        load_missions({"x": {"type": "grouped_lap", "begin": ["a", 0, 1]}})


def test_lap_goal_restatement_equals_the_reference_on_every_row():
    g = np.load(os.path.join(GOLDEN, "mission_goals_lap.npz"))
    rows, want = g["rows"], g["is_complete"].astype(bool)
    got = np.array([ref.lap_is_complete(r[0], r[1], r[2], int(r[3]), r[4], (r[5], r[6], r[7])) for r in rows])
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert want.any() and not want.all()


@pytest.mark.parametrize("name", ["4lane", "minicity"])
def test_traverse_goal_restatement_equals_the_reference_on_every_row(name, nets, compiled_maps):
    from smarts_amd.missions import lane_end_tables

    g = np.load(os.path.join(GOLDEN, "mission_goals_traverse.npz"))
    poses, want, branch = g[f"{name}_poses"], g[f"{name}_reached"].astype(bool), g[f"{name}_branch"]
    # the fixture's own conditions: both answers a hundred times, every return of _drove_off_map ten times
    assert want.sum() >= 100 and (~want).sum() >= 100 and (np.bincount(branch, minlength=5) >= 10).all()
    assert ((branch == 4) & ~want).sum() >= 10
    net, cm = nets(name), compiled_maps(name)
    tables = lane_end_tables(cm)
    got = np.array([ref.drove_off_map(net, cm, tables, x, y, h) for x, y, h in poses])
    assert np.array_equal(got, want), np.flatnonzero(got != want)


def test_lane_end_tables_name_the_dead_ends(nets, compiled_maps):
    from smarts_amd.missions import lane_end_tables

    cm = compiled_maps("4lane")
    heading, dead_end = lane_end_tables(cm)
    assert heading.dtype == np.float64 and dead_end.dtype == np.int32 and len(heading) == len(dead_end) == len(cm.lane_ids)
    dead = {cm.lane_ids[k] for k in np.flatnonzero(dead_end)}
    assert dead == {lane.getID() for lane in nets("4lane").all_lanes() if not lane.getOutgoing()} and len(dead) == 8
    assert not lane_end_tables(compiled_maps("loop"))[1].any()  # a closed circuit has none
    k = cm.lane_ids.index("edge-east-WE_0")  # eastbound: heading -pi/2, in vec_to_radians' range [0, 2 pi)
    assert abs(heading[k] - 1.5 * np.pi) < 1e-9


def test_c_abi_rejects_invalid_goal_tables_before_touching_the_device():
    """smx_check_mission_goals is the validation smx_set_mission_goals runs first (include/smx.h): no GPU, no handle."""
    from smarts_amd import _native as nat

    lib = nat.load_library()

    def check(goals, n_vehicles=None, heading=None, dead=None, n_lanes=0, map_lanes=4):
        recs = (nat.SmxMissionGoal * max(len(goals), 1))()
        for r, (kind, laps, length) in zip(recs, goals):
            r.kind, r.num_laps, r.route_length = kind, laps, length
        err = C.create_string_buffer(256)
        h = (C.c_double * len(heading))(*heading) if heading is not None else None
        d = (C.c_int32 * len(dead))(*dead) if dead is not None else None
        rc = lib.smx_check_mission_goals(recs, len(goals), len(goals) if n_vehicles is None else n_vehicles, h, d, n_lanes,
                                         map_lanes, err, 256)
        return rc, err.value.decode()

    assert C.sizeof(nat.SmxMissionGoal) == 16
    assert check([(nat.GOAL_POSITIONAL, 0, 0.0), (nat.GOAL_LAP, 2, 350.5)]) == (0, "")
    assert check([(nat.GOAL_TRAVERSE, 0, 0.0)], heading=[0.0] * 4, dead=[0, 1, 0, 1], n_lanes=4) == (0, "")
    assert check([]) == (0, "")  # n_slots = 0 clears
    bad = [
        (dict(goals=[(3, 1, 1.0)]), "unknown goal kind"), (dict(goals=[(-1, 1, 1.0)]), "unknown goal kind"),
        (dict(goals=[(nat.GOAL_LAP, 0, 10.0)]), "num_laps"), (dict(goals=[(nat.GOAL_LAP, -2, 10.0)]), "num_laps"),
        (dict(goals=[(nat.GOAL_LAP, 1, float("nan"))]), "route_length"), (dict(goals=[(nat.GOAL_LAP, 1, float("inf"))]), "route_length"),
        (dict(goals=[(nat.GOAL_LAP, 1, -1.0)]), "route_length"),
        (dict(goals=[(nat.GOAL_LAP, 1, 1.0)], n_vehicles=2), "one goal per vehicle slot"),
        (dict(goals=[(nat.GOAL_TRAVERSE, 0, 0.0)]), "lane tables"),
        (dict(goals=[(nat.GOAL_TRAVERSE, 0, 0.0)], heading=[0.0] * 3, dead=[0] * 3, n_lanes=3), "lane count"),
        (dict(goals=[(nat.GOAL_TRAVERSE, 0, 0.0)], heading=[0.0, float("nan"), 0.0, 0.0], dead=[0] * 4, n_lanes=4), "not finite"),
    ]
    for kw, word in bad:
        rc, msg = check(**kw)
        assert rc < 0 and word in msg, (kw, rc, msg)

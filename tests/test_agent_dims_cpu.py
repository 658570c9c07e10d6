"""Per-agent vehicle dimensions without a GPU: the host resolver and the start placement against the reference's own
outputs (tests/golden/agent_dims.json; tests/golden/gen_golden_agent_dims.py), ``TrafficHistoryTable.agent_dims``, and the
premises of the scene the GPU tests run (tests/agent_dims_ref.py), asserted on the oracle alone."""
import json
import math
import os

import numpy as np
import pytest

import agent_dims_ref as ref
from oracle.road_network import ORoadNetwork
from oracle.sim import COLLISION_LEEWAY, boxes_within
from smarts_amd.missions import PlannedMission
from smarts_amd.traffic_history import PASSENGER_DIMENSIONS, TrafficHistoryTable, resolve_dimensions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agent_dims.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_resolver_gives_what_agent_vehicle_dims_gives(golden):
    """``resolve_dimensions`` over the passenger type — the rule the env layer's ``agent_dims`` applies — for every spec of
    the fixture: every "no value" spelling per component, nothing given, everything given; no spec: the passenger's."""
    assert golden["passenger"] == list(PASSENGER_DIMENSIONS)
    assert len(golden["specs"]) == len(golden["resolved"]) >= 20
    for spec, want in zip(golden["specs"], golden["resolved"]):
        got = PASSENGER_DIMENSIONS if spec is None else resolve_dimensions(2, *spec)
        assert list(got) == want, (spec, got, want)
    assert [10.0, 2.5, 4.0] in golden["resolved"]


def test_front_bumper_start_is_placed_with_the_agents_own_length(golden):
    """``PlannedMission.spawn_pose(length)`` is ``Pose.from_front_bumper`` at the fixture's three lengths, to the last bit."""
    assert len(golden["bumper"]) == 3 and {b[3] for b in golden["bumper"]} == {3.68, 10.0, 2.5}
    for (x, y, heading, length), want in zip(golden["bumper"], golden["centre"]):
        m = PlannedMission((x, y), heading, (0.0, 0.0, 0.0), ())
        got = m.spawn_pose(length)
        assert list(got) == want, (length, got, want)
    m = PlannedMission((1.0, 2.0), 0.5, (0.0, 0.0, 0.0), ())
    assert m.spawn_pose() == m.spawn_pose(3.68)


def test_table_agent_dims():
    """``TrafficHistoryTable.agent_dims``: (R, E, A) ids -> (R, E, A, 3) through ``resolved_dimensions``; -1 gives NaNs; the
    same helper serves one id (a ``replaced`` stand-in)."""
    rows = [(3, 3, 10.0, 2.5, None), (8, 1, None, None, None), (11, 2, 4.2, 0, -1)]
    traj = [(v, 0.0, 1.0 * v, 2.0, 0.0, 1.0) for v, *_ in rows]
    table = TrafficHistoryTable.from_rows(rows, traj, 0.1, 3)
    follow = np.array([[[3, 8, -1], [11, 11, 3]], [[-1, -1, -1], [8, 3, 11]]], dtype=np.int32)
    out = table.agent_dims(follow)
    assert out.shape == (2, 2, 3, 3) and out.dtype == np.float64
    for idx in np.ndindex(*follow.shape):
        v = int(follow[idx])
        if v < 0:
            assert np.isnan(out[idx]).all(), idx
        else:
            assert tuple(out[idx]) == table.resolved_dimensions(v), idx
    assert tuple(out[0, 0, 0]) == (10.0, 2.5, 1.89) and tuple(out[0, 0, 1]) == (2.5, 1.0, 1.4) and tuple(out[0, 1, 0]) == (4.2, 1.47, 1.4)
    assert tuple(table.agent_dims(np.array(3))) == (10.0, 2.5, 1.89)  # one stand-in
    assert table.agent_dims(np.zeros((1, 2, 0), dtype=np.int32)).shape == (1, 2, 0, 3)


@pytest.mark.parametrize("name", ["loop", "4lane"])
def test_scene_premises(name, nets, compiled_maps):
    """What tests/test_gpu_agent_dims.py rests on, on the oracle alone.  Both maps give all four premises."""
    cm = compiled_maps(name)
    rm = ORoadNetwork(nets(name), lanepoint_spacing=cm.lanepoint_spacing)
    sc = ref.scene(cm, rm)
    assert sc["dims"].shape == (1, ref.E, ref.AGENTS, 3) and np.isnan(sc["dims"][0, 2:]).all() and np.isnan(sc["dims"][0, :2, 2]).all()
    spawn0 = sc["spawn0"]
    # (a) abreast of the standing vehicle — AHEAD m down agent 0's line, parallel to it, SIDE m apart — the trailer's box
    # is within the collision leeway of it and the sedan's is not; at the spawn neither is
    standing = ref.body_at(sc["standing_pose"])
    abreast = ref.ahead(spawn0, ref.AHEAD)
    assert boxes_within(ref.body_at(abreast, ref.TRAILER), standing, COLLISION_LEEWAY)
    assert not boxes_within(ref.body_at(abreast, ref.SEDAN), standing, COLLISION_LEEWAY)
    assert not boxes_within(ref.body_at(spawn0, ref.TRAILER), standing, COLLISION_LEEWAY)
    gap = ref.SIDE - 0.5 * ref.SEDAN[1]
    assert 0.5 * ref.SEDAN[1] + ref.COLLISION_LEEWAY < gap < 0.5 * ref.TRAILER[1] - 0.01
    # (b) at the spawn a trailer corner is off the road, the sedan's four and the motorcycle's are on it
    assert all(ref.corners_on_road(rm, ref.body_at(spawn0, ref.SEDAN))) and all(ref.corners_on_road(rm, ref.body_at(spawn0, ref.MOTORCYCLE)))
    assert not all(ref.corners_on_road(rm, ref.body_at(spawn0, ref.TRAILER)))
    assert rm.road_with_point(np.array([spawn0[0], spawn0[1], 0.0]))  # (the centre is on the road: on_shoulder, not off_road)
    # (c) agent 0 of envs 1 / 3: its nearest lane lies between the two off_route radii — and beyond 10 m
    assert math.isclose(ref.SEDAN_RADIUS, 6.98, abs_tol=0.01) and math.isclose(ref.TRAILER_RADIUS, 10.15, abs_tol=0.01)
    p = np.array([sc["off_route_pose"][0], sc["off_route_pose"][1], 0.0])
    assert rm.nearest_lane(p, radius=ref.SEDAN_RADIUS) is None and rm.nearest_lane(p, radius=10.0) is None
    assert rm.nearest_lane(p, radius=ref.TRAILER_RADIUS) is not None
    sedan, trailer = ref.body_at(sc["off_route_pose"]), ref.body_at(sc["off_route_pose"], ref.TRAILER)
    from oracle.sim import OracleEnv

    env = OracleEnv.__new__(OracleEnv)
    env.road_map = rm
    assert env._off_route_and_wrong_way(sedan)[0] is True and env._off_route_and_wrong_way(trailer)[0] is False
    # (d) FAR's nearest lane lies between a sedan's length and the trailer's: the trailer reports it, a sedan and the
    # motorcycle none
    q = np.array([sc["far_pose"][0], sc["far_pose"][1], 0.0])
    assert rm.nearest_lane(q, radius=ref.SEDAN[0]) is None and rm.nearest_lane(q, radius=ref.MOTORCYCLE[0]) is None
    assert rm.nearest_lane(q, radius=ref.TRAILER[0]) is not None
    # the table holds both vehicles in every frame, standing
    table = sc["table"]
    assert table.num_slots == ref.SLOTS and (table.vehicle >= 0).all() and table.num_frames == ref.FRAMES
    assert (table.frames[..., 3] == 0).all()

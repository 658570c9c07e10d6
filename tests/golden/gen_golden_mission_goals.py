#!/usr/bin/env python3
"""Golden vectors of the mission kinds beyond ``Mission(Route)``: EndlessMission, LapMission and TraverseGoal, from
the reference's OWN classes.

Same import shim as ``gen_golden.py`` (which see): runs only where the reference tree is; the suite consumes the
committed ``tests/golden/mission_goals_*.npz`` (arrays only).

* ``mission_goals_plan.npz`` — ``Scenario._extract_mission`` (scenario.py:625-750) of sstudio ``LapMission`` objects on
  ``loop`` (begin / end on different roads and on the same road, with and without ``via``): start, goal,
  ``route_length``; and the road list of ``Plan.create_route`` (plan.py:316-354) for the same mission.  Of sstudio
  ``EndlessMission`` objects — the one the reference's 4lane ``scenario.py`` gives its agents, more on 4lane and
  minicity — start position and heading.
* ``mission_goals_lap.npz`` — rows ``(x, y, distance_travelled, num_laps, route_length, goal) -> LapMission.is_complete``
  (plan.py:272-277): inside the goal radius with too little distance, at ``distance == route_length * num_laps``
  (strict ``>``) and one ulp on either side of it, on the radius and one ulp on either side of it.
* ``mission_goals_traverse.npz`` — poses on 4lane and minicity -> ``TraverseGoal._drove_off_map`` (plan.py:147-166)
  through the reference's ``SumoRoadNetwork`` (``gen_golden.make_reference_road_network``), and which of its returns
  each row took (``branch``: 0 no lane near, 1 the lane leads on, 2 still inside the lane, 3 not near the lane's end,
  4 the heading test).  The candidate set behind ``nearest_lanes`` is this project's ``getNeighboringLanes`` stand-in
  (``SumoNet.neighboring_lanes``), as for ``nearest_*.npz``: sumolib's rtree is not on this path.
  Asserted here: per map at least 100 rows true and 100 false, every branch at least 10 times.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mission_goals.py
"""
import math
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402

LAP_CASES = [  # (begin, end, via, num_laps) on loop
    (("445633931", 0, 10), ("445633932", 0, 30), (), 1),
    (("445633931", 1, 25.5), ("445633932", 1, "max"), (), 2),
    (("445633932", 0, "base"), ("445633931", 2, 40), (), 3),
    (("445633931", 0, 10), ("445633931", 0, 5), (), 1),       # begin and end on one road, the end behind the begin
    (("445633931", 2, 10), ("445633931", 0, 60), (), 2),      # ... and ahead of it
    (("445633932", 1, 50), ("445633932", 1, 20), (), 1),
    # (a via that is the end road itself has no route in the reference: generate_routes asks for a path from it to it)
    (("445633931", 0, 10), ("445633931", 0, 5), ("445633932",), 2),
    (("445633932", 1, 50), ("445633932", 1, 20), ("445633931",), 1),
]
ENDLESS_CASES = {
    "4lane": [("edge-south-SN", 1, 10),  # the reference's scenarios/intersections/4lane/scenario.py
              ("edge-west-WE", 0, "base"), ("edge-north-NS", 1, "max"), ("edge-east-EW", 0, 33.25)],
    "minicity": [("-10334990#0", 0, 5), ("-10390225#1", 0, "max"), ("-110128151", 0, "base"), ("-126742589#0", 0, 12.5)],
}


def dump_plan(nets):
    from smarts.core.plan import Plan
    from smarts.core.scenario import Scenario
    from smarts.sstudio import types as ss

    out = {}
    rn = gg.make_reference_road_network(nets["loop"])
    rows, roads, road_off, spec = [], [], [0], []
    for begin, end, via, laps in LAP_CASES:
        m = Scenario._extract_mission(ss.LapMission(route=ss.Route(begin=begin, end=end, via=via), num_laps=laps), rn)
        plan = Plan(rn, m)
        assert m.has_fixed_route and m.num_laps == laps
        rows.append([m.start.position[0], m.start.position[1], float(m.start.heading), m.goal.position[0],
                     m.goal.position[1], m.goal.radius, m.route_length, laps])
        roads += [r.road_id for r in plan.route.roads]
        road_off.append(len(roads))
        spec.append([begin[0], str(begin[1]), str(begin[2]), end[0], str(end[1]), str(end[2]), ",".join(via)])
    out["lap_spec"] = np.array(spec)            # begin road, lane, offset, end road, lane, offset, vias
    out["lap_rows"] = np.array(rows, dtype=np.float64)  # start x, y, heading, goal x, y, radius, route_length, num_laps
    out["lap_route_off"] = np.array(road_off, dtype=np.int32)
    out["lap_route_roads"] = np.array(roads)
    for name, cases in ENDLESS_CASES.items():
        rn = gg.make_reference_road_network(nets[name])
        rows = []
        for begin in cases:
            m = Scenario._extract_mission(ss.EndlessMission(begin=begin), rn)
            assert m.goal.is_endless() and not m.has_fixed_route
            assert len(Plan(rn, m).route.roads) == 0
            rows.append([m.start.position[0], m.start.position[1], float(m.start.heading)])
        out[f"endless_{name}_spec"] = np.array([[b[0], str(b[1]), str(b[2])] for b in cases])
        out[f"endless_{name}_rows"] = np.array(rows, dtype=np.float64)
    return out


def dump_lap(nets):
    from smarts.core.scenario import Scenario
    from smarts.sstudio import types as ss

    rn = gg.make_reference_road_network(nets["loop"])
    rng = np.random.default_rng(7007)
    rows, complete = [], []
    for begin, end, via, laps in LAP_CASES[:5]:
        m = Scenario._extract_mission(ss.LapMission(route=ss.Route(begin=begin, end=end, via=via), num_laps=laps), rn)
        gx, gy, r, need = m.goal.position[0], m.goal.position[1], m.goal.radius, m.route_length * laps
        up, down = math.nextafter(need, math.inf), math.nextafter(need, -math.inf)
        spots = [(0.0, 0.0), (1.0, -1.0), (r, 0.0), (0.0, -r), (math.nextafter(r, math.inf), 0.0),
                 (math.nextafter(r, 0.0), 0.0), (1.2, 1.6), (-1.6, 1.2), (2.5, 0.0), (0.0, 40.0)]
        spots += [tuple(rng.uniform(-2.5, 2.5, size=2)) for _ in range(10)]
        dists = [0.0, 0.5 * need, down, need, up, need + 0.25, m.route_length * (laps + 1), need - 1.0]
        dists += list(rng.uniform(0.0, 2.0 * need, size=4))
        for dx, dy in spots:
            for d in dists:
                veh = types.SimpleNamespace(position=np.array([gx + dx, gy + dy, 0.0]))
                rows.append([gx + dx, gy + dy, d, laps, m.route_length, gx, gy, r])
                complete.append(bool(m.is_complete(veh, d)))
    rows = np.array(rows, dtype=np.float64)
    complete = np.array(complete, dtype=np.uint8)
    inside = (rows[:, 0] - rows[:, 5]) ** 2 + (rows[:, 1] - rows[:, 6]) ** 2 <= rows[:, 7] ** 2
    assert (inside & (complete == 0)).sum() >= 50 and complete.sum() >= 50
    assert (complete[rows[:, 2] == rows[:, 3] * rows[:, 4]] == 0).all()  # strict >
    return dict(rows=rows, is_complete=complete)  # x, y, distance_travelled, num_laps, route_length, goal x, y, radius


def traverse_branch(rn, x, y, h):
    """_drove_off_map's returns, told apart with the reference's own objects (plan.py:147-166)."""
    from smarts.core.coordinates import Point
    from smarts.core.utils.math import min_angles_difference_signed, vec_to_radians

    pos = Point(x, y, 0.0)
    nearest = rn.nearest_lanes(pos)
    if not nearest:
        return 0
    nl, dist = nearest[0]
    offset = nl.to_lane_coord(pos).s
    width = nl.width_at_offset(offset)
    if nl.outgoing_lanes:
        return 1
    if dist < 0.5 * width + 1e-1:
        return 2
    if offset < nl.length - 2 * width:
        return 3
    end_heading = vec_to_radians(nl.vector_at_offset(nl.length - 0.1)[:2])
    assert isinstance(min_angles_difference_signed(end_heading, h), float)
    return 4


def dump_traverse(nets):
    from smarts.core.plan import TraverseGoal
    from smarts.core.utils.math import vec_to_radians

    out = {}
    for name in ("4lane", "minicity"):
        net = nets[name]
        rn = gg.make_reference_road_network(net)
        goal = TraverseGoal(rn)
        rng = np.random.default_rng(9100 + len(name))
        lanes = net.all_lanes()
        dead = [l for l in lanes if not l.getOutgoing()]
        live = [l for l in lanes if l.getOutgoing() and not l.getEdge().isSpecial()]
        pick = lambda ls, n: [ls[i] for i in rng.choice(len(ls), size=min(n, len(ls)), replace=False)]  # noqa: E731
        poses = []
        for lane, is_dead in [(l, True) for l in pick(dead, 12)] + [(l, False) for l in pick(live, 6)]:
            rl = rn.lane_by_id(lane.getID())
            length, width = rl.length, rl._width
            vec = rl.vector_at_offset(length - 0.1)
            end_heading = vec_to_radians(vec[:2])
            d = np.asarray(vec[:2]) / np.linalg.norm(vec[:2])
            n = np.array([-d[1], d[0]])
            end = np.asarray(lane.getShape(False)[-1], dtype=np.float64)
            headings = [0.0, math.pi / 6 - 0.02, math.pi / 6 + 0.02, -math.pi / 6 + 0.02, -math.pi / 6 - 0.02, math.pi,
                        0.3, -0.4, 1.2]
            side = [0.5 * width - 0.2, 0.5 * width + 0.2, 0.5 * width + 0.1, -(0.5 * width - 0.2), -(0.5 * width + 0.2), 0.0]
            # beyond the end, beside the end, around length - 2 x width, far out
            along = [0.6, 1.7, 2.5, 6.0, 9.5, 11.0, 15.0, -0.5, -(2 * width) + 0.3, -(2 * width) - 0.3, -(2 * width), -12.0]
            for k in range(130 if is_dead else 14):
                a = along[rng.integers(len(along))] + rng.normal(0.0, 0.05)
                s = side[rng.integers(len(side))] + rng.normal(0.0, 0.02)
                if rng.random() < 0.3:
                    s *= 3.0
                if k % 5 == 0:  # outside the lane's edge, short of its last 2 x width
                    a = [-(2 * width) - 0.3, -(2 * width) - 1.5, -12.0][rng.integers(3)] + rng.normal(0.0, 0.05)
                    s = (0.5 * width + rng.uniform(0.15, 1.5)) * (1 if rng.random() < 0.5 else -1)
                h = end_heading + headings[rng.integers(len(headings) if k % 2 else 5)] + rng.normal(0.0, 0.005)
                if rng.random() < 0.5:
                    h = (h + math.pi) % (2 * math.pi) - math.pi  # Heading's range, as a vehicle's is
                p = end + d * a + n * s
                poses.append((float(p[0]), float(p[1]), float(h)))
        poses = np.array(poses, dtype=np.float64)
        reached = np.array([bool(goal._drove_off_map((x, y, 0.0), h)) for x, y, h in poses], dtype=np.uint8)
        branch = np.array([traverse_branch(rn, x, y, h) for x, y, h in poses], dtype=np.uint8)
        assert (reached[branch != 4] == 0).all()
        counts = np.bincount(branch, minlength=5)
        print(name, "traverse rows", len(poses), "true", int(reached.sum()), "branches", counts.tolist(),
              "heading test false", int(((branch == 4) & (reached == 0)).sum()))
        assert reached.sum() >= 100 and (reached == 0).sum() >= 100, name
        assert (counts >= 10).all() and ((branch == 4) & (reached == 0)).sum() >= 10, (name, counts)
        out[f"{name}_poses"] = poses
        out[f"{name}_reached"] = reached
        out[f"{name}_branch"] = branch
    return out


def main():
    gg.install_reference()
    from smarts_amd.sumo_map import load_net

    nets = {n: load_net(os.path.join(gg.REF, rel)) for n, rel in gg.SCENARIOS.items()}
    for stem, dump in (("plan", dump_plan), ("lap", dump_lap), ("traverse", dump_traverse)):
        data = dump(nets)
        assert all(isinstance(v, np.ndarray) and v.dtype.kind in "fiuU" for v in data.values()), stem  # arrays only
        path = os.path.join(gg.OUT, f"mission_goals_{stem}.npz")
        np.savez_compressed(path, **data)
        print(f"mission_goals_{stem}.npz written:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors of ``lane_ttc`` (reference ``smarts/env/custom_observations.py:148-280``) for the cases the rollout
fixture ``std_obs.npz`` does not reach, from the reference's OWN function.

Same import shim as ``gen_golden.py`` (which see): runs only where the reference tree is; the suite consumes the
committed ``tests/golden/lane_ttc_cases.npz`` (arrays only).

Every case is one agent built by hand as dense rows (include/smx.h): straight paths along +y, one lane per path
unless the case says otherwise.  The reference's ``Observation`` is filled field by field from those rows (through
``ObservationBuilder``, as ``gen_golden.dump_std_obs`` does), ``lane_ttc`` runs on it, and the fixture keeps the rows
(``in_*``), the outputs (``ref``: distance_from_center, angle_error, ego_ttc x 3, ego_lane_dist x 3), whether the
reference raised ``IndexError`` (``raised``) and the case names.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lane_ttc.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402

P, W, K, LOOKAHEAD = 4, 6, 4, 5
LANE_WIDTH, SPEED_LIMIT = 3.2, 13.89
N_LANES = 8  # lane ids 0..7 ("lane_0" ...)


def path(lane, lane_index, x, y0=0.0, n=W, spacing=1.0, lanes=None):
    """Waypoints (x, y0 + w * spacing), heading 0; `lanes`: a lane id per waypoint instead of one for the path."""
    return dict(lane=lanes if lanes is not None else [lane] * n, lane_index=lane_index, x=x, y0=y0, n=n, spacing=spacing)


def case(name, paths, ego, nbs, n_total=None, nb_total=None):
    """ego = (x, y, heading, speed); nbs = [(x, y, lane id | None, speed)]."""
    return dict(name=name, paths=paths, ego=ego, nbs=nbs, n_total=n_total, nb_total=nb_total)


def cases():
    up, dn = np.nextafter(2.0, 3.0), np.nextafter(2.0, 1.0)
    three = [path(0, 0, 0.0), path(1, 1, 3.2), path(2, 2, 6.4)]
    out = [
        # two waypoints of one path exactly 0.5 from the neighbour: the first (arclength 1) wins over the second (2)
        case("equidistant_on_one_path", three, (3.2, 0.25, 0.0, 10.0), [(3.2, 1.5, 1, 5.0)]),
        # the same lane's waypoints in two paths, at the same coordinates: the first path wins
        case("equidistant_across_paths", [path(0, 0, 0.0), path(1, 1, 3.2), path(1, 1, 3.2, y0=0.0, spacing=1.0)],
             (3.2, 0.25, 0.0, 10.0), [(3.2, 2.0, 1, 5.0)]),
        # ... and at different coordinates, the same distance: path 1's waypoints 2 and 3 and path 2's waypoint 0
        case("equidistant_across_paths_shifted", [path(0, 0, 0.0), path(1, 1, 3.2), path(1, 1, 3.2, y0=2.0, spacing=2.0)],
             (3.2, 0.25, 0.0, 10.0), [(3.2, 2.5, 1, 5.0)]),
        case("gap_exactly_2", three, (3.2, 0.25, 0.0, 10.0), [(3.2 + 2.0, 3.0, 1, 5.0)]),
        case("gap_one_ulp_above_2", three, (0.0, 0.25, 0.0, 10.0), [(up, 3.0, 0, 5.0)]),
        case("gap_one_ulp_below_2", three, (0.0, 0.25, 0.0, 10.0), [(dn, 3.0, 0, 5.0)]),
        case("gap_exactly_2_from_zero", three, (0.0, 0.25, 0.0, 10.0), [(2.0, 3.0, 0, 5.0)]),
        case("equal_speeds_clamp", three, (3.2, 0.25, 0.0, 7.5), [(3.2, 3.0, 1, 7.5)]),
        case("nearly_equal_speeds_negative", three, (3.2, 0.25, 0.0, 7.5), [(3.2, 3.0, 1, float(np.nextafter(np.float32(7.5), np.float32(8))))]),
        case("faster_neighbour_ahead_discarded", three, (3.2, 0.25, 0.0, 5.0), [(3.2, 3.0, 1, 10.0)]),
        case("neighbour_at_first_waypoint_ttc_zero", three, (3.2, 0.25, 0.0, 10.0), [(3.2, 0.1, 1, 5.0)]),
        case("neighbour_without_lane", three, (3.2, 0.25, 0.0, 10.0), [(3.2, 3.0, None, 5.0)]),
        case("neighbour_on_unlisted_lane", three, (3.2, 0.25, 0.0, 10.0), [(3.2, 3.0, 7, 5.0)]),
        case("two_neighbours_one_path_min", three, (3.2, 0.25, 0.0, 10.0), [(3.2, 4.0, 1, 5.0), (3.2, 2.0, 1, 9.0), (3.2, 3.0, 1, 2.5)]),
        case("neighbours_on_three_paths", three, (3.2, 0.25, 0.0, 10.0), [(0.0, 4.0, 0, 5.0), (3.2, 2.0, 1, 9.0), (6.4, 3.0, 2, 2.5)]),
        case("lane_index_0_right_is_zero", three, (0.1, 0.25, 0.1, 10.0), [(0.0, 4.0, 0, 5.0), (3.2, 2.0, 1, 9.0)]),
        case("top_lane_left_is_zero", three, (6.3, 0.25, -0.2, 10.0), [(6.4, 4.0, 2, 5.0), (3.2, 2.0, 1, 9.0)]),
        # a junction: four paths over two lane indices (each lane fans out), the lists are indexed by lane index
        case("junction_paths_share_lane_index",
             [path(0, 0, 0.0, lanes=[0, 0, 3, 3, 3, 3]), path(0, 0, 0.0, lanes=[0, 0, 4, 4, 4, 4]),
              path(1, 1, 3.2, lanes=[1, 1, 5, 5, 5, 5]), path(1, 1, 3.2, lanes=[1, 1, 6, 6, 6, 6])],
             (3.2, 0.25, 0.0, 10.0), [(0.0, 3.0, 3, 5.0), (0.0, 4.0, 4, 4.0), (3.2, 3.0, 5, 5.0), (3.2, 5.0, 6, 2.5)]),
        case("junction_more_paths_than_rows",
             [path(0, 0, 0.0, lanes=[0, 0, 3, 3, 3, 3]), path(0, 0, 0.0, lanes=[0, 0, 4, 4, 4, 4]),
              path(1, 1, 3.2, lanes=[1, 1, 5, 5, 5, 5]), path(1, 1, 3.2, lanes=[1, 1, 6, 6, 6, 6])],
             (0.0, 0.25, 0.0, 10.0), [(0.0, 3.0, 3, 5.0), (0.0, 4.0, 4, 4.0)], n_total=6, nb_total=9),
        # the closest first waypoint's lane index is past the per-path list: the reference raises IndexError
        case("lane_index_past_the_paths", [path(2, 2, 6.4)], (6.4, 0.25, 0.0, 10.0), [(6.4, 3.0, 2, 5.0)]),
        case("lane_index_equal_to_len_paths", [path(1, 1, 3.2), path(2, 2, 6.4)], (6.4, 0.25, 0.0, 10.0), [(6.4, 3.0, 2, 5.0)]),
        case("no_neighbours", three, (3.3, 0.25, 0.3, 10.0), []),
        case("short_paths", [path(0, 0, 0.0, n=1), path(1, 1, 3.2, n=3)], (3.2, 0.25, 3.0, 10.0), [(3.2, 2.0, 1, 5.0), (0.0, 0.0, 0, 5.0)]),
        # two first waypoints at the same distance from the ego: the first path's wins
        case("equidistant_first_waypoints", three, (1.6, 0.0, 0.0, 10.0), [(0.0, 3.0, 0, 5.0), (3.2, 3.0, 1, 2.5)]),
    ]
    return out


def rows_of(cs):
    sys.path.insert(0, os.path.join(gg.REPO, "tests"))
    import parity
    from smarts_amd import _native as nat
    from smarts_amd.engine import SimConfig

    n = len(cs)
    cfg = SimConfig(num_envs=1, num_vehicles=n, neighbors=True, wp_paths=P, wp_len=W, nb_max=K, wp_lookahead=LOOKAHEAD)
    d = parity.empty_dense(cfg, n)
    for i, c in enumerate(cs):
        x, y, heading, speed = c["ego"]
        d["ego_pos"][i, :2] = (x, y)
        d["ego_f32"][i, nat.EGO["HEADING"]], d["ego_f32"][i, nat.EGO["SPEED"]] = heading, speed
        d["active"][i] = 1
        d["wp_count"][i, 0] = c["n_total"] or len(c["paths"])
        for p, pa in enumerate(c["paths"]):
            d["wp_count"][i, 1 + p] = pa["n"]
            for w in range(pa["n"]):
                d["wp_pos"][i, p, w, :2] = (pa["x"], pa["y0"] + w * pa["spacing"])
                d["wp_lane_width"][i, p, w], d["wp_speed_limit"][i, p, w] = LANE_WIDTH, SPEED_LIMIT
                d["wp_lane_index"][i, p, w], d["wp_lane_id"][i, p, w] = pa["lane_index"], pa["lane"][w]
        d["nb_count"][i] = c["nb_total"] or len(c["nbs"])
        for k, (vx, vy, lane, vs) in enumerate(c["nbs"]):
            d["nb_pos"][i, k, :2] = (vx, vy)
            d["nb_speed"][i, k] = vs
            d["nb_lane_id"][i, k] = -1 if lane is None else lane
            d["nb_lane_index"][i, k] = -1 if lane is None else 0
            d["nb_slot"][i, k] = (i + 1 + k) % n
    return cfg, d


def dump():
    from smarts.core.coordinates import Dimensions as RDimensions
    from smarts.core.coordinates import Heading as RHeading
    from smarts.core.events import Events as REvents
    from smarts.core.road_map import Waypoint as RWaypoint
    from smarts.core.sensors import EgoVehicleObservation as REgo
    from smarts.core.sensors import Observation as RObservation
    from smarts.core.sensors import VehicleObservation as RVehicle
    from smarts.core.sensors import Vias as RVias
    from smarts.env import custom_observations as rco

    from smarts_amd.env.observations import ObservationBuilder

    cs = cases()
    cfg, rows = rows_of(cs)
    n = len(cs)
    lane_ids = [f"lane_{i}" for i in range(N_LANES)]
    builder = ObservationBuilder(lane_ids, [f"road_{i}" for i in range(N_LANES)], [f"agent_{i}" for i in range(n)],
                                 waypoints=True, neighbors=True, accelerometer=True, dt=0.1)

    def to_ref(o):
        e = o.ego_vehicle_state
        ego = REgo(id=e.id, position=e.position, bounding_box=RDimensions(*e.bounding_box.as_lwh),
                   heading=RHeading(float(e.heading)), speed=e.speed, steering=e.steering, yaw_rate=e.yaw_rate,
                   road_id=e.road_id, lane_id=e.lane_id, lane_index=e.lane_index, mission=None,
                   linear_velocity=e.linear_velocity, angular_velocity=e.angular_velocity,
                   linear_acceleration=e.linear_acceleration, angular_acceleration=e.angular_acceleration,
                   linear_jerk=e.linear_jerk, angular_jerk=e.angular_jerk)
        nbs = [RVehicle(id=v.id, position=v.position, bounding_box=RDimensions(*v.bounding_box.as_lwh),
                        heading=RHeading(float(v.heading)), speed=v.speed, road_id=v.road_id, lane_id=v.lane_id,
                        lane_index=v.lane_index) for v in o.neighborhood_vehicle_states]
        paths = [[RWaypoint(pos=w.pos, heading=RHeading(float(w.heading)), lane_id=w.lane_id, lane_width=w.lane_width,
                            speed_limit=w.speed_limit, lane_index=w.lane_index) for w in p] for p in o.waypoint_paths]
        return RObservation(dt=o.dt, step_count=o.step_count, elapsed_sim_time=o.elapsed_sim_time,
                            events=REvents(**o.events._asdict()), ego_vehicle_state=ego, neighborhood_vehicle_states=nbs,
                            waypoint_paths=paths, distance_travelled=o.distance_travelled, lidar_point_cloud=None,
                            drivable_area_grid_map=None, occupancy_grid_map=None, top_down_rgb=None,
                            road_waypoints=None, via_data=RVias(near_via_points=[], hit_via_points=[]))

    ref = np.zeros((n, 8), dtype=np.float64)
    raised = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        ro = to_ref(builder.build(rows, i, 1, 0.1))
        try:
            val = rco.lane_ttc(ro)
        except IndexError:
            raised[i] = 1
            continue
        ref[i] = np.concatenate([np.asarray(val[k], dtype=np.float64).reshape(-1)
                                 for k in ("distance_from_center", "angle_error", "ego_ttc", "ego_lane_dist")])
    assert raised.sum() == 2, raised
    keep = ("ego_pos", "ego_f32", "wp_pos", "wp_heading", "wp_lane_width", "wp_speed_limit", "wp_lane_index", "wp_lane_id",
            "wp_count", "nb_pos", "nb_box", "nb_heading", "nb_speed", "nb_lane_index", "nb_lane_id", "nb_slot", "nb_count",
            "ego_lane", "events", "dist", "active", "done", "reward")
    out = {f"in_{k}": rows[k] for k in keep}
    out.update(ref=ref, raised=raised, names=np.array([c["name"] for c in cs]), wp_lookahead=np.array(LOOKAHEAD))
    return out


def main():
    gg.install_reference()
    for name in ("gym.envs", "gym.envs.registration", "gym.wrappers"):
        gg._stub(name)
    data = dump()
    assert all(isinstance(v, np.ndarray) and v.dtype.kind in "fiuU" for v in data.values())  # arrays only
    np.savez_compressed(os.path.join(gg.OUT, "lane_ttc_cases.npz"), **data)
    for name, r, bad in zip(data["names"], data["ref"], data["raised"]):
        print(f"{name:40s} {'IndexError' if bad else np.array2string(r, precision=6)}")


if __name__ == "__main__":
    main()

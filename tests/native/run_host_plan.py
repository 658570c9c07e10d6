"""Child process of tests/test_host_plan.py (sanitizer runtime preloaded): asks the host-compiled launch plan
(smarts_amd/csrc/smx_plan.h) for every configuration of the grid and checks the boundaries, the coupling invariants and
the reported form.  Prints one JSON line: the number of plans checked and the first failures."""
import ctypes as C
import itertools
import json
import sys

lib = C.CDLL(sys.argv[1])
lib.host_plan.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
FIELDS = ["form", "seeds", "facts", "facts_start", "rows", "chain", "ogm", "lidar", "control", "alive", "fork", "social",
          "tail_builds_list", "seed_pending", "slow_lists", "phased"]
# the enums of smx_plan.h and include/smx.h, by value
AUTO, SMALL, LARGE, LARGE_ONE_LANE, LARGE_TEAMS = range(5)
FORM_SMALL, FORM_TEAMS, FORM_ONE_LANE = range(3)
SEEDS_SCAN, SEEDS_ONE_LANE, SEEDS_ROUTED, SEEDS_WIDE, SEEDS_FOUR = range(5)
FACTS_SCAN, FACTS_ONE_LANE, FACTS_WIDE, FACTS_FOUR = range(4)
START_CALLER, START_WITH_GRIDS, START_AFTER_SEEDS = range(3)
ROWS_SENSORS, ROWS_UNSTAGED, ROWS_TABLES, ROWS_EMIT, ROWS_EMIT_CHAIN_SIDE, ROWS_EMIT_CHAIN_AFTER = range(6)
CHAIN_NONE, CHAIN_SIDE, CHAIN_AFTER_ROWS = range(3)
OGM_NONE, OGM_IN_SENSORS, OGM_ENV2, OGM_ENV1, OGM_PER_OBSERVER = range(5)
LIDAR_NONE, LIDAR_IN_SENSORS, LIDAR_SIDE, LIDAR_CALLER = range(4)
CONTROL_NONE = 0
ALIVE_NONE = 0
SENSOR_WAYPOINTS, SENSOR_OGM, SENSOR_LIDAR = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
ALIVE, SLOW, PENDING, KNOTS, CTRL = 1, 2, 4, 8, 16

# The boundaries as the parent commit's smx_kernels.hip has them (1cab73e), each by the name it has there.
LARGE_BATCH_VEHICLES = 16384       # SMX_LARGE_BATCH_VEHICLES: AUTO is SMALL up to and including this many
ONE_LANE_MIN_VEHICLES = 114688     # SMX_ONE_LANE_MIN_VEHICLES: the one-lane seeds kernel from here on
SCAN_WIDE_MAX_VEHICLES = 65536     # SMX_SCAN_WIDE_MAX_VEHICLES: eight-lane team halves on split maps up to and including
FACTS_EARLY_MAX = 32768            # SMX_FACTS_EARLY_MAX: the facts half released with the grid kernels up to and including
OGM_ENV_MIN_VEHICLES = 8192        # SMX_OGM_ENV_MIN_VEHICLES: per-env OGM in the small form from here on ...
OGM_ENV_MAX_PER_ENV = 32           # ... with at most 32 vehicles an env
OGM_ENV_LDS = 64 * 1024            # ... and eight tiles (SMX_OGM_WAVES * 2) that fit a workgroup's LDS
OGM_INLINE_MAX = 16 * 1024         # inline OGM (inside k_sensors) only in the small form, up to 16 KiB
WPT_MAX_PATHS = 8                  # SMX_WPT_MAX_PATHS: rows the staged form handles

# (envs, vehicles per env): 32 a env on both sides of every threshold, 64 a env around the small form's OGM choice
BATCHES = [(t // 32, 32) for b in (OGM_ENV_MIN_VEHICLES, LARGE_BATCH_VEHICLES, FACTS_EARLY_MAX, SCAN_WIDE_MAX_VEHICLES,
                                    ONE_LANE_MIN_VEHICLES) for t in (b - 32, b, b + 32)] + [(128, 64), (256, 64), (257, 64)]
OGM_TILES = [(0, 0), (64, 64), (128, 128), (144, 128)]  # off, 4 KiB, 16 KiB, 18 KiB
BLOBS = [31, 0, 31 & ~ALIVE, 31 & ~SLOW, 31 & ~PENDING, 31 & ~KNOTS, 31 & ~CTRL]

failures, checked = [], 0
arg, out = (C.c_int * 16)(), (C.c_int * 16)()


def check(ok, what, case, p):
    if not ok and len(failures) < 20:
        failures.append([what, case, p])


for ((envs, nv), strategy, junctions, routed, wp_paths, waypoints, (ow, oh), lidar, timing, is_step, blobs, side_ready,
     idm) in itertools.product(BATCHES, range(5), (0, 1), (0, 1), (WPT_MAX_PATHS, WPT_MAX_PATHS + 1), (0, 1), OGM_TILES, (0, 1),
                               (0, 2), (0, 1), BLOBS, (0, 1), (0, 1)):
    sensors = (SENSOR_WAYPOINTS if waypoints else 0) | (SENSOR_OGM if ow else 0) | (SENSOR_LIDAR if lidar else 0)
    carried = (envs + strategy + blobs) & 1
    space = (0, 3, 1, 4)[(envs + wp_paths + timing) % 4]
    arg[:] = [envs, nv, strategy, junctions, routed, sensors, wp_paths, ow, oh, timing, is_step, blobs, side_ready, carried, idm, space]
    assert lib.host_plan(arg, out) == len(FIELDS)
    p = dict(zip(FIELDS, out))
    case = list(arg)
    total, tile = envs * nv, ow * oh
    checked += 1
    small = p["form"] == FORM_SMALL
    # (c) the form smx_launch_form reported at the parent: SMALL by strategy or, under AUTO, by size; else the one-lane
    # cut where the alive and slow blobs exist and the strategy forces it or (unforced) the map has no splits
    parent_small = strategy == SMALL or (strategy == AUTO and total <= LARGE_BATCH_VEHICLES)
    parent_cut = strategy == LARGE_ONE_LANE or (strategy != LARGE_TEAMS and not junctions)
    parent_form = FORM_SMALL if parent_small else FORM_ONE_LANE if (blobs & ALIVE and blobs & SLOW and parent_cut) else FORM_TEAMS
    check(p["form"] == parent_form, "form", case, p)
    # (a) boundaries
    if strategy == AUTO:
        check(small == (total <= LARGE_BATCH_VEHICLES), "AUTO: SMALL up to 16 384", case, p)
    one_lane_seeds = p["seeds"] == SEEDS_ONE_LANE
    if one_lane_seeds:
        check(strategy == LARGE_ONE_LANE or total >= ONE_LANE_MIN_VEHICLES, "one-lane seeds below 114 688", case, p)
    if is_step and p["form"] == FORM_ONE_LANE and not routed and waypoints and wp_paths <= WPT_MAX_PATHS and blobs == 31:
        check(one_lane_seeds == (strategy == LARGE_ONE_LANE or total >= ONE_LANE_MIN_VEHICLES), "one-lane seeds from 114 688 on", case, p)
    wide_ok = junctions and not small and total <= SCAN_WIDE_MAX_VEHICLES
    check((p["seeds"] == SEEDS_WIDE) <= wide_ok and (p["facts"] == FACTS_WIDE) <= wide_ok, "eight-lane halves past 65 536 or off split maps", case, p)
    if p["form"] == FORM_TEAMS and junctions:
        check((p["facts"] == FACTS_WIDE) == (total <= SCAN_WIDE_MAX_VEHICLES), "eight-lane facts half up to 65 536", case, p)
        if not routed:
            check((p["seeds"] == SEEDS_WIDE) == (total <= SCAN_WIDE_MAX_VEHICLES), "eight-lane seeds half up to 65 536", case, p)
    if p["fork"]:
        check((p["facts_start"] == START_WITH_GRIDS) == (total <= FACTS_EARLY_MAX) and p["facts_start"] != START_CALLER,
              "facts half with the grid kernels up to 32 768", case, p)
    else:
        check(p["facts_start"] == START_CALLER, "facts half on a side stream without a fork", case, p)
    check((p["ogm"] == OGM_NONE) == (tile == 0), "OGM kernel without / no kernel with the sensor", case, p)
    if tile and small:
        env_ogm = total >= OGM_ENV_MIN_VEHICLES and nv <= OGM_ENV_MAX_PER_ENV and tile * 8 <= OGM_ENV_LDS
        check((p["ogm"] == OGM_ENV2) == env_ogm, "small form: per-env OGM from 8 192 on, <= 32 vehicles, tiles that fit", case, p)
        check(p["ogm"] != OGM_ENV1, "small form: four-tile per-env OGM", case, p)
        if not env_ogm:
            check((p["ogm"] == OGM_IN_SENSORS) == (tile <= OGM_INLINE_MAX), "small form: inline OGM up to 16 KiB", case, p)
    if not small:
        check(p["ogm"] != OGM_IN_SENSORS and p["lidar"] != LIDAR_IN_SENSORS and p["rows"] != ROWS_SENSORS, "k_sensors roles in the large form", case, p)
    # (b) coupling
    chained = p["chain"] != CHAIN_NONE
    check(one_lane_seeds == chained == bool(p["seed_pending"]) == (p["rows"] in (ROWS_EMIT_CHAIN_SIDE, ROWS_EMIT_CHAIN_AFTER)),
          "seed_pending: seeds kernel <=> walk / emit <=> one slow chain", case, p)
    check((p["rows"] == ROWS_EMIT_CHAIN_SIDE) == (p["chain"] == CHAIN_SIDE) and (p["rows"] == ROWS_EMIT_CHAIN_AFTER) == (p["chain"] == CHAIN_AFTER_ROWS),
          "the slow chain runs once, where the rows say", case, p)
    if one_lane_seeds:
        check(not routed and waypoints and wp_paths <= WPT_MAX_PATHS, "one-lane seeds with routed missions or past 8 rows", case, p)
        check(blobs & PENDING and blobs & SLOW and blobs & KNOTS and p["slow_lists"], "one-lane seeds without the pending / slow / knots blobs", case, p)
        check(is_step and p["form"] == FORM_ONE_LANE and p["facts"] == FACTS_ONE_LANE, "one-lane seeds outside the one-lane cut's tick", case, p)
    side = p["fork"] or p["chain"] == CHAIN_SIDE or p["lidar"] == LIDAR_SIDE or p["facts_start"] != START_CALLER
    if timing == 2 or small or not side_ready or not is_step:
        check(not side, "work on a side stream at timing level 2 / in the small form / without side streams / in a reset", case, p)
    check(p["fork"] == bool(is_step and not small and timing != 2 and side_ready), "fork", case, p)
    check(p["phased"] == bool(is_step and timing == 2), "phase events", case, p)
    if not is_step:
        check(p["control"] == CONTROL_NONE and p["alive"] == ALIVE_NONE and not p["fork"] and not p["social"] and not chained,
              "a reset call plans control, an alive list, a fork, social traffic or a chain", case, p)
    else:
        check(p["control"] != CONTROL_NONE, "a step without a controller", case, p)
        check((p["alive"] != ALIVE_NONE) == bool(not small and blobs & ALIVE), "alive list: large form with the blob", case, p)
        check(p["social"] == bool(idm), "k_social", case, p)
    if idm:
        check(not p["tail_builds_list"], "k_tail builds the next list with IDM social traffic", case, p)
    if p["tail_builds_list"]:
        check(not small and blobs & ALIVE and blobs & SLOW, "k_tail builds a list in the small form or without blobs", case, p)

print(json.dumps({"checked": checked, "failures": failures}))

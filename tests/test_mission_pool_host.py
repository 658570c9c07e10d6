"""The mission pool without a device (include/smx.h smx_set_mission_pool / smx_check_mission_pool).

tests/native/host_mission_pool.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over the
shim hip_runtime.h and the HIP memory stand-in shim/hip_memory.h — drives the check over every refusal and the handle's
bind / rebind / unbind, its exclusion of the per-slot calls and what a new map drops, with every HIP call failing in turn.
The rest is the entry point on the built library, the declarations, and the env layer's schedule and spawn rows."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "smarts_amd", "csrc")


def test_mission_pool_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_mission_pool")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", CSRC,
           os.path.join(NATIVE, "host_mission_pool.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    # the environment is inherited as it is; the sanitizer runtime is linked into the program itself, so its check of
    # the library order (which a preload of the caller's would trip) has nothing to protect here
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert proc.returncode == 0 and "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, \
        (proc.stdout[-3000:], proc.stderr[-3000:])
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    assert res["sweep_points"] == res["hip_calls"] > 80 and res["skipped"] == 0, res
    assert res["refused"] + res["release_points"] == res["sweep_points"] and res["refused"] > 50, res
    assert res["mallocs"] == res["frees"] and res["steps"] >= 24 and res["checks"] > 5000, res


def test_header_declares_the_entry_points_and_the_cap():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_mission_pool(smx_handle h, const smx_mission_pool* pool);" in header
    assert "int smx_check_mission_pool(const smx_config* cfg, const smx_map_tables* map, const smx_mission_pool* pool, char* err," in header
    assert "#define SMX_MISSION_POOL_MAX 4096" in header
    from smarts_amd import _native as nat

    assert "smx_set_mission_pool" in nat.EXPORTS and "smx_check_mission_pool" in nat.EXPORTS
    assert C.sizeof(nat.SmxMissionPool) == 96 and nat.MISSION_POOL_MAX == 4096
    assert C.sizeof(nat.SmxMission) == 32 and C.sizeof(nat.SmxMissionGoal) == 16 and C.sizeof(nat.SmxVia) == 40  # the neighbours keep their layout
    lib = nat.load_library()
    assert lib.smx_struct_size(0) == C.sizeof(nat.SmxConfig)


def _pool_4lane(nets, compiled_maps):
    import mission_pool_ref as mp

    cm = compiled_maps("4lane")
    missions, vias = mp.pool_4lane(nets, cm)
    return cm, missions, vias, mp


def test_smx_check_mission_pool_needs_no_device(nets, compiled_maps):
    import dataclasses

    from smarts_amd import _native as nat
    from smarts_amd.engine import check_mission_pool
    from smarts_amd.missions import GOAL_LAP, PlannedMission

    cm, missions, vias, mp = _pool_4lane(nets, compiled_maps)
    check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, missions, vias, mp.TABLE, via_max=4)
    check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, missions + [None], None)   # no vias, one row of -1
    with pytest.raises(ValueError, match="via_max"):
        check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, missions, vias, mp.TABLE, via_max=0)
    with pytest.raises(ValueError, match="shape"):
        check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, missions, vias, mp.TABLE[:, :2], via_max=4)
    with pytest.raises(ValueError, match="one via list per pool entry"):
        check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, missions, vias[:2], mp.TABLE, via_max=4)
    for bad in (len(missions), -7):
        table = mp.TABLE.copy()
        table[1, 2, 0] = bad
        with pytest.raises(ValueError, match=r"-1 \.\. 3"):
            check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, missions, vias, table, via_max=4)
    with pytest.raises(ValueError, match="SMX_MISSION_POOL_MAX"):
        check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, [None] * (nat.MISSION_POOL_MAX + 1), None)
    check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, [None] * nat.MISSION_POOL_MAX, None)
    with pytest.raises(ValueError, match="at most 32 vias"):
        check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, missions, [vias[2] * 11, [], [], []], mp.TABLE, via_max=4)
    with pytest.raises(ValueError, match="lap goal"):   # a lap goal on an empty route
        check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, [PlannedMission((0.0, 0.0), 0.0, (0.0, 0.0, 0.0), (), GOAL_LAP, 10.0, 1)], None)
    with pytest.raises(KeyError):                        # a road the map does not have
        check_mission_pool(cm, mp.E, mp.N, mp.SOCIAL, [dataclasses.replace(missions[0], route_roads=("no-such-road",))], None)
    # ... and an index outside the road table, through the C-ABI
    lib = nat.load_library()
    from smarts_amd.engine import _mission_pool_struct, map_tables_struct

    mpool, keep = _mission_pool_struct(cm, missions, vias)
    table = mp.TABLE.copy()
    mpool.rows_dev, mpool.rows_count, mpool.rows = table.ctypes.data, table.size, table.shape[0]
    cfg = nat.SmxConfig()
    cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.via_max = mp.E, mp.N, mp.SOCIAL, 4
    tables, keep_map = map_tables_struct(cm)
    err = C.create_string_buffer(512)
    assert lib.smx_check_mission_pool(C.byref(cfg), C.byref(tables), C.byref(mpool), err, len(err)) == 0, err.value
    roads = C.cast(mpool.route_roads_host, C.POINTER(C.c_int32))
    roads[1] = len(cm.road_ids)
    assert lib.smx_check_mission_pool(C.byref(cfg), C.byref(tables), C.byref(mpool), err, len(err)) == -1
    assert b"road index out of range" in err.value and b"smx_set_mission_pool" in err.value
    roads[1] = 0
    mpool.rows_dev = None
    assert lib.smx_check_mission_pool(C.byref(cfg), C.byref(tables), C.byref(mpool), err, len(err)) == -1 and b"rows_dev" in err.value
    assert lib.smx_check_mission_pool(None, None, None, None, 0) == -1
    del keep, keep_map


# ---- the env layer's device-free half (smarts_amd.missions)
def test_mission_variations_and_their_errors():
    from smarts_amd.missions import mission_variations

    v = mission_variations({"A": ["a0", "a1", "a2"], "B": "b", "D": ("d0", "d1", "d2")}, ["A", "B", "C", "D"])
    assert v == [["a0", "b", None, "d0"], ["a1", "b", None, "d1"], ["a2", "b", None, "d2"]]
    assert mission_variations({"A": "a"}, ["A", "B"]) == [["a", None]]   # no list: one variation
    with pytest.raises(ValueError, match="one common length"):
        mission_variations({"A": ["a0", "a1"], "B": ["b0", "b1", "b2"]}, ["A", "B"])
    with pytest.raises(ValueError, match="empty list"):
        mission_variations({"A": []}, ["A"])
    with pytest.raises(ValueError, match="unknown agents"):
        mission_variations({"Z": ["z"]}, ["A"])


def test_mission_schedule_defaults():
    from smarts_amd.missions import mission_schedule

    # shuffle off: R = V, episode k runs variation k mod V in every env — the reference's cycle
    s = mission_schedule(3, 4, seed=9, shuffle_scenarios=False)
    assert s.dtype == np.int32 and s.shape == (3, 4) and np.array_equal(s, np.repeat(np.arange(3)[:, None], 4, axis=1))
    # shuffle on: every env's cycle is the same cycle rolled by an offset drawn from seed + e
    r = mission_schedule(5, 6, seed=9, shuffle_scenarios=True)
    assert r.shape == (5, 6)
    for e in range(6):
        offset = int(np.random.Generator(np.random.PCG64(9 + e)).integers(5))
        assert np.array_equal(r[:, e], (np.arange(5) + offset) % 5), e
    assert len({tuple(r[:, e]) for e in range(6)}) > 1                       # the envs do not all start alike
    assert np.array_equal(r, mission_schedule(5, 6, seed=9, shuffle_scenarios=True))
    # env e of a batch seeded s is env 0 of a batch seeded s + e (ParallelEnv.seed: env i gets seed + i)
    assert np.array_equal(r[:, 4], mission_schedule(5, 1, seed=13, shuffle_scenarios=True)[:, 0])
    # an explicit schedule
    assert np.array_equal(mission_schedule(2, 3, schedule=[1, 0, 0]), [[1, 1, 1], [0, 0, 0], [0, 0, 0]])
    assert np.array_equal(mission_schedule(2, 2, schedule=[[1, 0], [0, 0]]), [[1, 0], [0, 0]])
    for bad, why in (([[2, 0]], "0 .. 1"), ([[-1, 0]], "0 .. 1"), ([[0, 0, 0]], "shape"), ([[0.5, 0.0]], "integer")):
        with pytest.raises(ValueError, match=why):
            mission_schedule(2, 2, schedule=bad)


def test_pool_rows_and_spawn_rows_follow_the_schedule(nets, compiled_maps):
    from smarts_amd.missions import mission_pool_rows, mission_schedule, mission_spawn_poses

    cm, missions, vias, mp = _pool_4lane(nets, compiled_maps)
    planned = [[missions[0], None], [missions[1], missions[3]], [None, missions[2]]]   # V = 3 variations of two agents
    sched = mission_schedule(3, 2, schedule=[[0, 2], [1, 1], [2, 0]])
    rows = mission_pool_rows(planned, sched)
    assert rows.dtype == np.int32 and rows.shape == (3, 2, 2)
    assert np.array_equal(rows, [[[0, -1], [-1, 5]], [[2, 3], [2, 3]], [[-1, 5], [0, -1]]])   # j * A + a, -1: no mission
    # an agent with vias and no mission points at its own (endless) pool entry, which carries the vias; -1 has none
    with_vias = mission_pool_rows(planned, sched, has_vias=[False, True])
    assert np.array_equal(with_vias, [[[0, 1], [-1, 5]], [[2, 3], [2, 3]], [[-1, 5], [0, 1]]])
    poses = mission_spawn_poses(planned, sched, 6)
    assert poses.shape == (6, 2, 2, 3)
    for s in range(6):
        for e in range(2):
            for a in range(2):
                m = planned[sched[s % 3, e]][a]
                if m is None:
                    assert np.isnan(poses[s, e, a]).all()
                else:
                    assert np.array_equal(poses[s, e, a], m.spawn_pose()), (s, e, a)
    with pytest.raises(ValueError, match="multiple"):
        mission_spawn_poses(planned, sched, 4)
    longer = mission_spawn_poses(planned, sched, 3, lengths=[5.0, None])
    assert not np.array_equal(longer[0, 0, 0], poses[0, 0, 0]) and np.array_equal(longer[1, 0, 1], poses[1, 0, 1])

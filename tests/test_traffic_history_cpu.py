"""Traffic-history replay, host side (smarts_amd/traffic_history.py), without a device.

tests/golden/traffic_history_*.npz (gen_golden_traffic_history.py) hold small synthetic histories and what the
reference's own TrafficHistoryProvider.step returned for them, tick by tick.  The table built from the same input rows
must hand out the same vehicles with the same four numbers, exactly: they are copies, and the heading wrap is
Heading.__new__'s to the bit."""
import glob
import os

import numpy as np
import pytest

from smarts_amd.traffic_history import (TrafficHistoryTable, read_spec, read_sqlite, slots_needed, wrap_heading,
                                        write_sqlite)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("traffic_history_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "traffic_history_*.npz")))


def _load(name):
    g = np.load(os.path.join(GOLDEN, f"traffic_history_{name}.npz"))
    veh = [(int(r[0]), int(r[1])) + tuple(None if np.isnan(v) else float(v) for v in r[2:5]) for r in g["vehicle_rows"]]
    traj = [(int(r[0]),) + tuple(float(v) for v in r[1:6]) for r in g["trajectory_rows"]]
    return g, veh, traj


def test_the_golden_cases_are_the_ones_the_issue_names():
    assert set(CASES) >= {"period_dt", "period_2dt", "start_offset", "off_grid", "coarse_dt"}


@pytest.mark.parametrize("name", CASES)
def test_table_reproduces_the_provider_exactly(name):
    g, veh, traj = _load(name)
    dt, start, ticks = float(g["dt"]), int(g["start_frame"]), int(g["ticks"])
    S = slots_needed(veh, traj, dt)
    table = TrafficHistoryTable.from_rows(veh, traj, dt, S + 1)
    off = g["tick_off"]
    for k in range(ticks):
        want = {int(i): g["out_row"][j] for j, i in zip(range(off[k], off[k + 1]), g["out_id"][off[k]:off[k + 1]])}
        assert len(want) == off[k + 1] - off[k]  # (the provider hands a vehicle out once per tick)
        frame = start + k
        got = {}
        if 0 <= frame < table.num_frames:
            for s in range(table.num_slots):
                v = table.vehicle_at(frame, s)
                if v >= 0:
                    assert v not in got
                    got[v] = table.frames[frame, s]
        assert set(got) == set(want), (name, k, sorted(got), sorted(want))
        for v, row in want.items():
            # bit for bit (array_equal on the raw words: -0.0 and 0.0 would differ, NaNs would compare equal)
            assert np.array_equal(got[v].view(np.uint64), np.asarray(row, dtype=np.float64).view(np.uint64)), (name, k, v, got[v], row)
            assert table.spawn_of(v, frame) == tuple(float(x) for x in row)
    # beyond the data every frame is empty
    assert table.vehicle_at(table.num_frames, 0) == -1 and table.vehicle_at(-1, 0) == -1


def test_flicker_of_data_coarser_than_dt_is_kept():
    g, veh, traj = _load("period_2dt")
    table = TrafficHistoryTable.from_rows(veh, traj, 0.1, 2)
    present5 = [(table.vehicle[k] == 5).any() for k in range(10)]
    assert present5 == [True, False] * 5  # samples at 0.0, 0.2, ...: absent in the frames between, as in the reference
    present2 = [(table.vehicle[k] == 2).any() for k in range(10)]
    assert present2 == [False, True] * 5


def test_heading_wrap_is_headings():
    import math

    for h in (0.0, math.pi, -math.pi, math.nextafter(math.pi, 4.0), 3.5, -4.0, 7.0, 100.0, -100.0, 2 * math.pi, -0.0):
        v = h % (2 * math.pi)  # coordinates.py:175-184
        if v > math.pi:
            v -= 2 * math.pi
        assert wrap_heading(h) == v and -math.pi <= wrap_heading(h) <= math.pi
    assert wrap_heading(-math.pi) == math.pi  # (the half-open end)


def _history(n_vehicles=6, overlap=3):
    """Vehicle v lives in frames [2 v, 2 v + 2 overlap): `overlap` at once."""
    veh = [(100 - v, 2, None, None, None) for v in range(n_vehicles)]  # ids descending in order of appearance
    traj = []
    for v in range(n_vehicles):
        for k in range(2 * v, 2 * v + 2 * overlap):
            traj.append((100 - v, round(k * 0.1, 6), float(v), float(k), 0.0, 1.0))
    return veh, traj


def test_slot_assignment_properties():
    veh, traj = _history()
    need = slots_needed(veh, traj, 0.1)
    table = TrafficHistoryTable.from_rows(veh, traj, 0.1, need)
    F, S = table.vehicle.shape
    where = {}
    for k in range(F):
        ids = [int(v) for v in table.vehicle[k] if v >= 0]
        assert len(ids) == len(set(ids))  # one slot per vehicle and frame
        for s in range(S):
            v = int(table.vehicle[k, s])
            if v < 0:
                continue
            if k > 0 and (table.vehicle[k - 1] == v).any():
                assert table.vehicle[k - 1, s] == v  # a stable slot while present in consecutive frames
            else:
                assert k == 0 or table.vehicle[k - 1, s] < 0  # a new vehicle takes a slot that stood empty for a frame
            where.setdefault(v, set()).add(s)
    assert all(len(s) == 1 for s in where.values())
    assert need == 4  # three at once, and the slot of a vehicle that left is not reused in the very next frame
    # deterministic: the same rows in another order give the same table
    again = TrafficHistoryTable.from_rows(veh[::-1], traj[::-1], 0.1, need)
    assert np.array_equal(again.vehicle, table.vehicle) and np.array_equal(again.frames, table.frames)
    # vehicles appearing in one frame take the lowest free slots in ascending id order
    both = TrafficHistoryTable.from_rows([(9, 2, None, None, None), (4, 2, None, None, None)],
                                         [(9, 0.0, 0, 0, 0, 0), (4, 0.0, 1, 1, 0, 0)], 0.1, 3)
    assert both.vehicle[0].tolist() == [4, 9, -1]


def test_too_few_slots_names_the_number_needed():
    veh, traj = _history()
    with pytest.raises(ValueError, match=r"needs 4 slots"):
        TrafficHistoryTable.from_rows(veh, traj, 0.1, 3)
    assert slots_needed(veh, traj, 0.1) == 4
    assert slots_needed(veh, [], 0.1) == 0


def test_exclude_ids():
    veh, traj = _history()
    table = TrafficHistoryTable.from_rows(veh, traj, 0.1, 4, exclude_ids=(100, 98))
    assert 100 not in table.vehicle_ids() and 98 not in table.vehicle_ids() and 99 in table.vehicle_ids()
    assert slots_needed(veh, traj, 0.1, exclude_ids=(100, 98, 96)) < 4
    # a trajectory without its Vehicle row is dropped (the provider's INNER JOIN)
    t2 = TrafficHistoryTable.from_rows(veh[1:], traj, 0.1, 4)
    assert 100 not in t2.vehicle_ids()


def test_helpers():
    veh, traj = _history()
    table = TrafficHistoryTable.from_rows(veh, traj, 0.1, 5)
    assert table.frame_of(0.0) == 0 and table.frame_of(0.3) == 3 and table.frame_of(1.2) == 12
    assert table.frame_of(0.1 + 0.2) == 3  # (0.30000000000000004: on the grid)
    for bad in (0.05, 0.31, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="multiple of dt"):
            table.frame_of(bad)
    assert table.vehicle_at(0, 0) == 100
    with pytest.raises(IndexError):
        table.vehicle_at(0, 5)
    with pytest.raises(KeyError):
        table.spawn_of(100, 10)  # gone by then
    assert table.dimensions(100) == (None, None, None)
    assert table.frames.dtype == np.float64 and table.vehicle.dtype == np.int32
    assert table.frames.flags["C_CONTIGUOUS"] and table.vehicle.flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("name", ["period_dt", "off_grid"])
def test_from_sqlite(tmp_path, name):
    g, veh, traj = _load(name)
    path = str(tmp_path / "history.shf")
    write_sqlite(path, veh, traj, spec={"source": "synthetic", "speed_limit_mps": 13.89})
    dt = float(g["dt"])
    S = slots_needed(veh, traj, dt)
    a = TrafficHistoryTable.from_rows(veh, traj, dt, S)
    b = TrafficHistoryTable.from_sqlite(path, dt, S)
    assert np.array_equal(a.vehicle, b.vehicle) and np.array_equal(a.frames.view(np.uint64), b.frames.view(np.uint64))
    assert a.dims == b.dims
    rows = read_sqlite(path)
    assert len(rows[0]) == len(veh) and len(rows[1]) == len(traj)
    assert read_spec(path)["source"] == "synthetic"
    with pytest.raises(ValueError, match="slots"):
        TrafficHistoryTable.from_sqlite(path, dt, S - 1)


def test_env_keywords_without_a_device(monkeypatch):
    """HiWayEnv / ParallelEnv / BatchCore hand the table and the start frames to BatchedSim.set_traffic_history."""
    import smarts_amd.engine as engine
    from smarts_amd.env.agent import AgentSpec
    from smarts_amd.env.agent_interface import AgentInterface, AgentType
    from smarts_amd.env.hiway_env import HiWayEnv
    from smarts_amd.env.parallel_env import ParallelEnv

    seen = []

    class Recorder:
        def __init__(self, cm, cfg, **kw):
            self.device = "cpu"
            self.cfg = cfg

        def set_traffic_history(self, table, start_frames=None, replaced=None):
            seen.append((table, start_frames.numpy().copy(), self.cfg.num_social))

        def close(self):
            pass

    monkeypatch.setattr(engine, "BatchedSim", Recorder)
    veh, traj = _history()
    table = TrafficHistoryTable.from_rows(veh, traj, 0.1, 4)
    specs = {"a": AgentSpec(interface=AgentInterface.from_type(AgentType.Laner, max_episode_steps=10))}
    env = HiWayEnv(["scenarios/loop"], specs, num_social=4, traffic_history=table, history_start_frames=3)
    env._ensure_core()
    assert seen[-1][0] is table and seen[-1][1].tolist() == [[3]] and seen[-1][2] == 4
    env._core = None
    par = ParallelEnv([lambda k=k: HiWayEnv(["scenarios/loop"], specs, num_social=4, traffic_history=table,
                                            history_start_frames=[k, -k]) for k in range(3)], auto_reset=True)
    assert seen[-1][1].tolist() == [[0, 1, 2], [0, -1, -2]] and seen[-1][1].dtype == np.int32
    par._core = None
    with pytest.raises(ValueError, match="traffic_history"):
        HiWayEnv(["scenarios/loop"], specs, num_social=4, history_start_frames=3)
    assert HiWayEnv(["scenarios/loop"], specs, num_social=4).signature() != env.signature()

#!/usr/bin/env python3
"""Golden vectors of traffic-history replay, from the reference's OWN ``TrafficHistory`` and
``TrafficHistoryProvider.step`` (smarts/core/traffic_history.py, traffic_history_provider.py:96-136).

Same import shim as ``gen_golden.py`` (which see; ``cached_property`` is stubbed there): runs only where the reference
tree is; the suite consumes the committed ``tests/golden/traffic_history_*.npz`` (arrays only).

Each case is a small synthetic history written into a temporary SQLite file with the three tables of the converter's
layout (smarts/sstudio/genhistories.py:105-137).  The reference's provider is set up on it and stepped with
``elapsed_sim_time = rounder(k * dt)``, k = 0 .. ticks - 1, as ``SMARTS._step`` advances it (smarts.py:262), from
``start_time = start_frame * dt``.  Stored per case:

  vehicle_rows     [V, 5]  id, type, length, width, height (NaN where the dataset has NULL)
  trajectory_rows  [T, 6]  vehicle_id, sim_time, position_x, position_y, heading_rad, speed — in the file's order
  dt, start_frame, ticks
  tick_off         [ticks + 1]  rows of tick k are out_*[tick_off[k] : tick_off[k + 1]], in the provider's order
  out_id           [R] int64    the id behind "history-vehicle-<id>"
  out_row          [R, 4]       pose.position x, y; float(pose.heading); speed

Cases: data period = dt (0.1 / 0.1); data period = 2 dt (a vehicle is present in every second tick: the flicker); a
non-zero start offset; vehicles entering and leaving; ids out of order; samples off the dt grid; headings outside
(-pi, pi] (Heading.__new__ wraps them).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_traffic_history.py
"""
import math
import os
import sqlite3
import sys
import tempfile
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402


def write_db(path, vehicle_rows, trajectory_rows):
    db = sqlite3.connect(path)
    db.execute("CREATE TABLE Spec (key TEXT PRIMARY KEY, value TEXT) WITHOUT ROWID")
    db.execute("CREATE TABLE Vehicle (id INTEGER PRIMARY KEY, type INTEGER NOT NULL, length REAL, width REAL, height REAL, "
               "is_ego_vehicle INTEGER DEFAULT 0) WITHOUT ROWID")
    db.execute("CREATE TABLE Trajectory (vehicle_id INTEGER NOT NULL, sim_time REAL NOT NULL, position_x REAL NOT NULL, "
               "position_y REAL NOT NULL, heading_rad REAL NOT NULL, speed REAL DEFAULT 0.0, lane_id INTEGER DEFAULT 0, "
               "PRIMARY KEY (vehicle_id, sim_time), FOREIGN KEY (vehicle_id) REFERENCES Vehicles(id)) WITHOUT ROWID")
    db.execute("INSERT INTO Spec VALUES ('source', 'synthetic')")
    db.executemany("INSERT INTO Vehicle VALUES (?, ?, ?, ?, ?, 0)", vehicle_rows)
    db.executemany("INSERT INTO Trajectory VALUES (?, ?, ?, ?, ?, ?, 0)", trajectory_rows)
    db.commit()
    db.close()


def track(vid, t0, n, period, x0, y0, heading, speed, jitter=0.0):
    """n samples of a vehicle moving along its heading (0 = +y, counter-clockwise) from (x0, y0)."""
    rows = []
    for i in range(n):
        t = round(t0 + i * period + jitter, 6)
        d = speed * i * period
        rows.append((vid, t, x0 - math.sin(heading) * d, y0 + math.cos(heading) * d, heading + 0.01 * i, speed + 0.1 * i))
    return rows


def cases():
    sedan = (2, 3.68, 1.47, 1.4)
    out = {}
    # data period = dt; vehicles enter and leave; ids out of order; a slot's worth of vehicles at once
    veh = [(41, *sedan), (7, 2, None, None, None), (19, 3, 8.0, 2.5, None), (3, *sedan), (1000, *sedan)]
    traj = (track(41, 0.0, 12, 0.1, 10.0, 5.0, 0.3, 8.0) + track(7, 0.3, 6, 0.1, -20.0, 2.0, -2.0, 4.0) +
            track(19, 0.5, 15, 0.1, 0.0, 0.0, 3.5, 10.0) + track(3, 1.4, 5, 0.1, 100.0, -50.0, -4.0, 0.0) +
            track(1000, 0.1, 3, 0.1, 1.0, 1.0, 7.0, 2.0))
    out["period_dt"] = (veh, traj, 0.1, 0, 24)
    # data period = 2 dt: present in every second tick
    veh = [(5, *sedan), (2, *sedan)]
    traj = track(5, 0.0, 8, 0.2, 0.0, 0.0, 0.0, 5.0) + track(2, 0.1, 6, 0.2, 3.2, 0.0, math.pi, 5.0)
    out["period_2dt"] = (veh, traj, 0.1, 0, 20)
    # a non-zero start offset into the first history (and past its end)
    veh, traj = out["period_dt"][0], out["period_dt"][1]
    out["start_offset"] = (veh, traj, 0.1, 7, 22)
    # samples off the dt grid (the window's ends decide), two samples of one vehicle in one window (the later wins),
    # a coarser dt
    veh = [(8, *sedan), (9, *sedan)]
    traj = (track(8, 0.0, 20, 0.05, 0.0, 0.0, 1.0, 3.0) + track(9, 0.0, 9, 0.1, 5.0, 5.0, -1.0, 3.0, jitter=0.04))
    out["off_grid"] = (veh, traj, 0.1, 0, 14)
    out["coarse_dt"] = (veh, traj, 0.25, 1, 6)
    return out


def run_case(veh, traj, dt, start_frame, ticks):
    from smarts.core.traffic_history import TrafficHistory
    from smarts.core.traffic_history_provider import TrafficHistoryProvider
    from smarts.core.utils.math import rounder_for_dt

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "history.shf")
        write_db(path, veh, traj)
        history = TrafficHistory(types.SimpleNamespace(path=path, name="history.shf"))
        provider = TrafficHistoryProvider()
        provider.setup(types.SimpleNamespace(traffic_history=history))
        rounder = rounder_for_dt(dt)
        provider.start_time = rounder(start_frame * dt)
        tick_off, ids, rows = [0], [], []
        for k in range(ticks):
            state = provider.step({}, dt, rounder(k * dt))
            for vs in state.vehicles:
                assert vs.vehicle_id.startswith("history-vehicle-") and vs.source == "HISTORY"
                ids.append(int(vs.vehicle_id[len("history-vehicle-"):]))
                rows.append((float(vs.pose.position[0]), float(vs.pose.position[1]), float(vs.pose.heading), float(vs.speed)))
            tick_off.append(len(ids))
        provider.teardown()
    nan = float("nan")
    return dict(
        vehicle_rows=np.array([[nan if v is None else float(v) for v in r] for r in veh], dtype=np.float64),
        trajectory_rows=np.array(traj, dtype=np.float64), dt=np.float64(dt), start_frame=np.int64(start_frame),
        ticks=np.int64(ticks), tick_off=np.array(tick_off, dtype=np.int64), out_id=np.array(ids, dtype=np.int64),
        out_row=np.array(rows, dtype=np.float64).reshape(-1, 4))


def main():
    gg.install_reference()
    for name, case in cases().items():
        data = run_case(*case)
        per_tick = np.diff(data["tick_off"])
        assert per_tick.max() >= 2 and per_tick.min() == 0 or name in ("period_2dt", "off_grid", "coarse_dt"), (name, per_tick)
        path = os.path.join(gg.OUT, f"traffic_history_{name}.npz")
        np.savez_compressed(path, **data)
        print(name, "ticks", int(data["ticks"]), "rows", len(data["out_id"]), "per tick", per_tick.tolist(),
              os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Traffic-history replay, host side: a recorded dataset resampled into the dense table the device replays.

The reference replays a converted dataset (NGSIM, INTERACTION: ``smarts/sstudio/genhistories.py`` writes the SQLite
file) tick by tick through ``TrafficHistoryProvider.step`` (``smarts/core/traffic_history_provider.py:96-136`` over
``TrafficHistory.vehicles_active_between``, ``traffic_history.py:221-231``).  ``TrafficHistoryTable`` holds what that
provider would hand out at every tick of a run that starts at history time 0, in ``num_slots`` vehicle slots: the table
``smx_set_social_history`` (include/smx.h) copies to the device, where every env replays its own window of it
(``BatchedSim.set_traffic_history``).

Frame ``k`` is history time ``k * dt``.  Per vehicle it holds the latest sample with
``rounder(rounder(k * dt) - dt) < sim_time <= rounder(k * dt)`` — the provider's ``ORDER BY sim_time DESC``, first row per
id, ``rounder_for_dt(dt)`` — as a copy: x, y, speed untouched, the heading wrapped as ``Heading.__new__`` wraps it
(``coordinates.py:175-184``).  A vehicle without a sample in a window is absent from that frame, exactly as in the
reference: data recorded at a period longer than ``dt`` flickers (present in the frames that hold a sample, absent in
between), here as there.

Deviations from the reference, all stated in DESIGN.md section 5:
 - a window starts at a frame, i.e. at a multiple of ``dt`` (``frame_of`` raises otherwise); the reference's
   ``start_time`` is any non-negative float;
 - the per-vehicle dimensions are opt-in (``BatchedSim.set_traffic_history(..., dims=True)``): ``device_dims()`` applies
   the provider's rule — the dataset's ``length, width, height``, or where it has none (``None``, 0, -1) the default of
   the vehicle's type (``traffic_history_provider.py:112-126``) — and the device then replays every vehicle at its own
   size; without them every replayed vehicle has the sedan's box.  An agent that stands in for a recorded vehicle
   (``replaced``) is a sedan whatever that vehicle was, and the lidar stands every box on the ground instead of centring
   it on z = 0;
 - ``Trajectory`` rows of a vehicle type other than the passenger car are replayed too (the provider does the same; only
   the reference's mission discovery filters on the type).
"""
from __future__ import annotations

import math
import sqlite3
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

HISTORY_VEHICLE_PREFIX = "history-vehicle-"  # TrafficHistoryProvider._vehicle_id_prefix

# The default (length, width, height) of a dataset type: TrafficHistory.decode_vehicle_type (traffic_history.py:127-146:
# 1 motorcycle, 2 passenger, 3 truck, 4 pedestrian, anything else passenger) into VEHICLE_CONFIGS (vehicle.py:97-140).
PASSENGER_DIMENSIONS = (3.68, 1.47, 1.4)
TYPE_DIMENSIONS = {1: (2.5, 1.0, 1.4), 2: PASSENGER_DIMENSIONS, 3: (5.0, 1.91, 1.89), 4: (0.5, 0.5, 1.6)}
MAX_DEVICE_ID = 1 << 20  # device_dims() holds a row per id up to the largest


def resolve_dimensions(vehicle_type, length, width, height) -> Tuple[float, float, float]:
    """``Dimensions.init_with_defaults`` (coordinates.py:55-66) over the type's default: a value that is ``None``, 0 or
    -1 takes the default's."""
    defaults = TYPE_DIMENSIONS.get(vehicle_type, PASSENGER_DIMENSIONS)
    return tuple(float(d) if (not v or v == -1) else float(v) for v, d in zip((length, width, height), defaults))


def round_param_for_dt(dt: float) -> int:
    """The digits ``round()`` keeps for a time step (smarts/core/utils/math.py:553-563)."""
    strep = np.format_float_positional(dt)
    decimal = strep.find(".")
    if decimal >= len(strep) - 1:
        return 1 - decimal
    return len(strep) - decimal - 1


def wrap_heading(value: float) -> float:
    """``Heading.__new__`` (coordinates.py:175-184): into (-pi, pi], with Python's float modulo."""
    value = float(value) % (2 * math.pi)
    if value > math.pi:
        value -= 2 * math.pi
    return value


def _window_samples(vehicle_rows, trajectory_rows, dt: float, exclude_ids: Iterable[int]):
    """Per frame, ``{vehicle id: (x, y, heading, speed)}`` of what the provider returns at that frame's tick."""
    if not dt > 0.0:
        raise ValueError("dt must be > 0")
    known = {int(r[0]) for r in vehicle_rows}  # (the provider's INNER JOIN: a trajectory needs its Vehicle row)
    hidden = {int(v) for v in exclude_ids}
    rp = round_param_for_dt(dt)
    traj = sorted(((float(r[1]), int(r[0]), float(r[2]), float(r[3]), float(r[4]), float(r[5] if r[5] is not None else 0.0))
                   for r in trajectory_rows if int(r[0]) in known and int(r[0]) not in hidden))
    if not traj:
        return [dict()]
    if any(not math.isfinite(t[0]) for t in traj):
        raise ValueError("trajectory times must be finite")
    last = traj[-1][0]
    frames: List[Dict[int, Tuple[float, float, float, float]]] = []
    i, k = 0, 0
    while True:
        hi = round(k * dt, rp)
        lo = round(hi - dt, rp)
        while i < len(traj) and traj[i][0] <= lo:  # (samples at or before the window's open end: never shown by this or a later frame)
            i += 1
        cur: Dict[int, Tuple[float, float, float, float]] = {}
        j = i
        while j < len(traj) and traj[j][0] <= hi:  # ascending time: a later sample of the same vehicle replaces the earlier
            _, vid, x, y, h, s = traj[j]
            cur[vid] = (x, y, wrap_heading(h), s)
            j += 1
        frames.append(cur)
        if hi >= last:
            break
        k += 1
    return frames


def _assign_slots(frames) -> Tuple[List[Dict[int, int]], int]:
    """Slot of every vehicle in every frame, and the slots needed.  A vehicle keeps its slot while it is present in
    consecutive frames; a slot is free for another vehicle only once it has stood empty for a frame; vehicles that
    appear in the same frame take the lowest free slots in ascending id order."""
    prev: Dict[int, int] = {}
    out: List[Dict[int, int]] = []
    needed = 0
    for cur in frames:
        held = {vid: prev[vid] for vid in cur if vid in prev}
        blocked = set(prev.values())  # occupied in the frame before: kept by its vehicle, or cooling off for one frame
        now = dict(held)
        slot = 0
        for vid in sorted(v for v in cur if v not in prev):
            while slot in blocked:
                slot += 1
            now[vid] = slot
            blocked.add(slot)
        needed = max(needed, max(now.values()) + 1 if now else 0)
        out.append(now)
        prev = now
    return out, needed


def slots_needed(vehicle_rows, trajectory_rows, dt: float, exclude_ids: Iterable[int] = ()) -> int:
    """The smallest ``num_slots`` ``TrafficHistoryTable.from_rows`` accepts for these rows (nothing is built)."""
    return _assign_slots(_window_samples(vehicle_rows, trajectory_rows, dt, exclude_ids))[1]


class TrafficHistoryTable:
    """``frames`` [F, S, 4] float64 (x, y, heading, speed: the vehicle centre, the reference's heading convention,
    wrapped), ``vehicle`` [F, S] int32 (the history's vehicle id, < 0 = the slot is empty), ``dims`` {id: (length, width,
    height)} with ``None`` where the dataset has none, ``types`` {id: the dataset's type} (both as the dataset has
    them; ``device_dims`` / ``resolved_dimensions`` apply the provider's rule)."""

    def __init__(self, frames: np.ndarray, vehicle: np.ndarray, dt: float, dims: Optional[Dict[int, Tuple]] = None,
                 types: Optional[Dict[int, int]] = None):
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        vehicle = np.ascontiguousarray(vehicle, dtype=np.int32)
        if frames.ndim != 3 or frames.shape[2] != 4 or vehicle.shape != frames.shape[:2] or frames.shape[0] < 1:
            raise ValueError(f"frames must be [F >= 1, S, 4] and vehicle [F, S], got {frames.shape} and {vehicle.shape}")
        self.frames, self.vehicle, self.dt = frames, vehicle, float(dt)
        self.dims = dict(dims or {})
        self.types = dict(types or {})
        self._rp = round_param_for_dt(self.dt)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_rows(cls, vehicle_rows: Sequence[Sequence], trajectory_rows: Sequence[Sequence], dt: float, num_slots: int,
                  exclude_ids: Iterable[int] = ()) -> "TrafficHistoryTable":
        """``vehicle_rows``: (id, type, length, width, height[, is_ego_vehicle]) as in the ``Vehicle`` table;
        ``trajectory_rows``: (vehicle_id, sim_time, position_x, position_y, heading_rad, speed[, lane_id]) as in
        ``Trajectory``.  ``exclude_ids`` never enter the table (for a vehicle an agent replaces in every env; to hide one
        per env, keep it and use ``replaced`` of ``BatchedSim.set_traffic_history``).  More vehicles at once than
        ``num_slots`` holds raises ``ValueError`` naming the number needed."""
        samples = _window_samples(vehicle_rows, trajectory_rows, dt, exclude_ids)
        slots, needed = _assign_slots(samples)
        if needed > num_slots:
            raise ValueError(f"the history needs {needed} slots (vehicles present at once, and a free frame before a slot "
                             f"is reused), num_slots is {num_slots}")
        frames = np.zeros((len(samples), num_slots, 4), dtype=np.float64)
        vehicle = np.full((len(samples), num_slots), -1, dtype=np.int32)
        for k, (cur, where) in enumerate(zip(samples, slots)):
            for vid, row in cur.items():
                if not 0 <= vid <= 0x7FFFFFFF:
                    raise ValueError(f"vehicle id {vid} does not fit the table's int32 ids (>= 0)")
                frames[k, where[vid]] = row
                vehicle[k, where[vid]] = vid
        dims = {int(r[0]): tuple(None if v is None else float(v) for v in r[2:5]) for r in vehicle_rows}
        types = {int(r[0]): (None if r[1] is None else int(r[1])) for r in vehicle_rows}
        return cls(frames, vehicle, dt, dims, types)

    @classmethod
    def from_sqlite(cls, path: str, dt: float, num_slots: int, exclude_ids: Iterable[int] = ()) -> "TrafficHistoryTable":
        """From a converted dataset: the ``Vehicle`` and ``Trajectory`` tables ``genhistories.py`` writes."""
        vehicle_rows, trajectory_rows = read_sqlite(path)
        return cls.from_rows(vehicle_rows, trajectory_rows, dt, num_slots, exclude_ids)

    # ------------------------------------------------------------------ helpers
    @property
    def num_frames(self) -> int:
        return int(self.frames.shape[0])

    @property
    def num_slots(self) -> int:
        return int(self.frames.shape[1])

    def frame_of(self, time: float) -> int:
        """The frame of history time ``time``, which must be a multiple of ``dt`` (a deviation: the reference's
        ``start_time`` may be any non-negative time; a window here starts at a frame)."""
        time = float(time)
        k = int(round(time / self.dt)) if math.isfinite(time) else 0
        if not math.isfinite(time) or abs(k * self.dt - time) > 1e-9 * max(1.0, abs(time)):
            raise ValueError(f"history time {time!r} is not a multiple of dt = {self.dt}")
        return k

    def vehicle_at(self, frame: int, slot: int) -> int:
        """The vehicle id in ``slot`` at ``frame``; -1 for an empty slot and for a frame outside the table."""
        if not 0 <= slot < self.num_slots:
            raise IndexError(f"slot {slot} of {self.num_slots}")
        if not 0 <= frame < self.num_frames:
            return -1
        return int(self.vehicle[frame, slot])

    def spawn_of(self, vehicle_id: int, frame: int) -> Tuple[float, float, float, float]:
        """(x, y, heading, speed) of ``vehicle_id`` at ``frame``: the spawn row of an agent that replaces it."""
        if 0 <= frame < self.num_frames:
            hit = np.nonzero(self.vehicle[frame] == int(vehicle_id))[0]
            if len(hit):
                return tuple(float(v) for v in self.frames[frame, hit[0]])
        raise KeyError(f"vehicle {vehicle_id} is not present in frame {frame}")

    def dimensions(self, vehicle_id: int) -> Tuple:
        """(length, width, height) of the dataset, ``None`` where it has none (``resolved_dimensions``: the rule applied)."""
        return self.dims[int(vehicle_id)]

    def resolved_dimensions(self, vehicle_id: int) -> Tuple[float, float, float]:
        """(length, width, height) the reference's provider gives ``vehicle_id``: the dataset's values over the default
        of its type.  An id without a ``Vehicle`` row (a table from the plain constructor): the passenger default."""
        vid = int(vehicle_id)
        return resolve_dimensions(self.types.get(vid, 2), *self.dims.get(vid, (None, None, None)))

    def device_dims(self) -> np.ndarray:
        """float64 ``[max id + 1, 3]``: ``resolved_dimensions`` by vehicle id, the table ``smx_set_social_history_dims``
        takes.  Ids that never occur in ``vehicle`` hold the passenger default."""
        ids = self.vehicle_ids()
        top = ids[-1] if ids else 0
        if top > MAX_DEVICE_ID:
            raise ValueError(f"vehicle id {top} is above {MAX_DEVICE_ID} (2^20): the device table holds a row per id up "
                             f"to the largest; renumber the dataset's vehicles")
        out = np.tile(np.asarray(PASSENGER_DIMENSIONS, dtype=np.float64), (top + 1, 1))
        for vid in ids:
            out[vid] = self.resolved_dimensions(vid)
        return out

    def agent_dims(self, vehicle) -> np.ndarray:
        """The table ``BatchedSim.set_agent_dims`` takes for agents that stand for recorded vehicles — followers
        (``set_history_agents``' follow table) and ``replaced`` stand-ins alike: ``vehicle`` is an integer array of
        vehicle ids, ``(R, E, A)`` for a follow table, and the result float64 ``vehicle.shape + (3,)`` holds each id's
        ``resolved_dimensions`` (a recorded vehicle keeps its dimensions when an agent takes it over, vehicle_index.py:
        439, 489).  An id < 0 (the slot follows nothing) gives three NaNs: the sedan's box."""
        ids = np.asarray(vehicle.cpu() if hasattr(vehicle, "cpu") else vehicle, dtype=np.int64)
        out = np.full(ids.shape + (3,), np.nan, dtype=np.float64)
        for vid in np.unique(ids[ids >= 0]):
            out[ids == vid] = self.resolved_dimensions(int(vid))
        return out

    def vehicle_ids(self) -> List[int]:
        return sorted(int(v) for v in np.unique(self.vehicle) if v >= 0)

    # ------------------------------------------------------------------ history agents (BatchedSim.set_history_agents)
    def frames_of(self, vehicle_id: int) -> np.ndarray:
        """The frames that hold ``vehicle_id``, ascending (empty for an id the table lacks)."""
        return np.nonzero((self.vehicle == int(vehicle_id)).any(axis=1))[0] if int(vehicle_id) >= 0 else np.zeros(0, dtype=np.int64)

    def first_seen_frames(self) -> Dict[int, int]:
        """``{vehicle id: the first frame that holds it}``: ``TrafficHistory.first_seen_times`` (traffic_history.py:
        148-155) on the table's frame grid."""
        out: Dict[int, int] = {}
        for k in range(self.num_frames):
            for vid in self.vehicle[k]:
                if vid >= 0:
                    out.setdefault(int(vid), k)
        return dict(sorted(out.items()))

    def last_seen_frame(self, vehicle_id: int) -> int:
        """The last frame that holds ``vehicle_id`` (``KeyError`` for an id the table lacks)."""
        held = self.frames_of(vehicle_id)
        if not len(held):
            raise KeyError(f"vehicle {vehicle_id} is not in the table")
        return int(held[-1])

    def expert_actions(self, vehicle_id: int) -> np.ndarray:
        """float64 ``[frames present, 2]``: per frame ``f`` that holds the vehicle, the Imitation action that takes its
        recorded heading and speed to frame ``f + 1``'s — the exact inverse of ``ImitationController``
        (imitation_controller.py:61-78): ``acceleration = (speed[f+1] - speed[f]) / dt``, ``angular_velocity =
        min_angles_difference_signed(heading[f+1], heading[f]) / dt`` — and NaN, NaN ("no action") where frame ``f + 1``
        lacks the vehicle.  What the device writes to ``out["expert_action"]`` (rounded once to float32)."""
        held = self.frames_of(vehicle_id)
        out = np.full((len(held), 2), np.nan, dtype=np.float64)
        for i, f in enumerate(held):
            if f + 1 >= self.num_frames:
                continue
            nxt = np.nonzero(self.vehicle[f + 1] == int(vehicle_id))[0]
            if not len(nxt):
                continue
            h0, s0 = self.frames[f, np.nonzero(self.vehicle[f] == int(vehicle_id))[0][0], 2:4]
            h1, s1 = self.frames[f + 1, nxt[0], 2:4]
            out[i, 0] = (float(s1) - float(s0)) / self.dt
            out[i, 1] = ((((float(h1) - float(h0)) + math.pi) % (2 * math.pi)) - math.pi) / self.dt
        return out

    def history_agent_windows(self, ids: Sequence[int], num_envs: int, num_agents: int,
                              reset_elapsed_steps: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """``(start_frames [1, E] int32, vehicle [1, E, A] int32)`` for one env per recorded vehicle: env ``k`` follows
        ``ids[k]`` in agent slot 0 from that vehicle's first frame (``start = first_seen - reset_elapsed_steps``, so the
        reset observation is its first frame; a negative start is fine), its other agent slots follow the further
        vehicles present in that frame in ascending id order, and ``-1`` fills what is left (and every env past
        ``len(ids)``, which starts at frame 0)."""
        ids = [int(v) for v in ids]
        if len(ids) > num_envs:
            raise ValueError(f"{len(ids)} vehicles for {num_envs} envs")
        if num_agents < 1:
            raise ValueError("num_agents must be >= 1")
        first = self.first_seen_frames()
        start = np.zeros((1, num_envs), dtype=np.int32)
        vehicle = np.full((1, num_envs, num_agents), -1, dtype=np.int32)
        for k, vid in enumerate(ids):
            if vid not in first:
                raise KeyError(f"vehicle {vid} is not in the table")
            start[0, k] = first[vid] - int(reset_elapsed_steps)
            others = sorted(int(v) for v in self.vehicle[first[vid]] if v >= 0 and v != vid)
            vehicle[0, k, :] = ([vid] + others + [-1] * num_agents)[:num_agents]
        return start, vehicle

    # ------------------------------------------------------------------ handover (BatchedSim.set_history_handover)
    def zone_entry_frames(self, pos: Sequence[float], size: Sequence[float]) -> Dict[int, int]:
        """``{vehicle id: the first frame whose recorded position lies strictly inside the zone}``: the axis-aligned
        rectangle of the reference's ``PositionalZone(pos, size)`` (sstudio/types.py:686-700) — centre ``pos``, extent
        ``size[0]`` along x and ``size[1]`` along y.  A point on the boundary is outside, as ``Point.within`` has it; a
        vehicle that never enters is absent from the result.  With ``handover_ticks`` a bubble over a replayed history
        is one host pass: no polygon test on the device."""
        x0, x1 = float(pos[0]) - float(size[0]) / 2, float(pos[0]) + float(size[0]) / 2
        y0, y1 = float(pos[1]) - float(size[1]) / 2, float(pos[1]) + float(size[1]) / 2
        x, y = self.frames[..., 0], self.frames[..., 1]
        inside = (self.vehicle >= 0) & (x > x0) & (x < x1) & (y > y0) & (y < y1)
        out: Dict[int, int] = {}
        for k, s in zip(*np.nonzero(inside)):  # (row-major: ascending frames)
            out.setdefault(int(self.vehicle[k, s]), int(k))
        return dict(sorted(out.items()))

    @staticmethod
    def handover_ticks(vehicle: np.ndarray, start_frames: np.ndarray, frame_of: Dict[int, int]) -> np.ndarray:
        """The handover table of ``BatchedSim.set_history_handover``, int32 ``[R, E, A]``, for the follow table
        ``vehicle`` ``[R, E, A]`` and ``start_frames`` ``[R, E]``: agent ``a`` of env ``e`` is driven from the tick at
        which its env shows frame ``frame_of[v]`` of its vehicle ``v`` — ``max(frame_of[v] - start_frames[r, e], 0)`` —
        and never (``-1``) where ``v < 0`` or ``v`` has no entry in ``frame_of``."""
        vehicle, start_frames = np.asarray(vehicle), np.asarray(start_frames)
        if vehicle.ndim != 3 or start_frames.shape != vehicle.shape[:2]:
            raise ValueError(f"vehicle must be [R, E, A] and start_frames [R, E], got {vehicle.shape} and {start_frames.shape}")
        out = np.full(vehicle.shape, -1, dtype=np.int32)
        for idx in np.ndindex(*vehicle.shape):
            v = int(vehicle[idx])
            if v >= 0 and v in frame_of:
                out[idx] = min(max(int(frame_of[v]) - int(start_frames[idx[:2]]), 0), np.iinfo(np.int32).max)
        return out


def read_sqlite(path: str):
    """(vehicle_rows, trajectory_rows) of a converted dataset, in the column order ``from_rows`` takes."""
    with sqlite3.connect(f"file:{path}?mode=ro", uri=True) as db:
        vehicle_rows = db.execute("SELECT id, type, length, width, height, is_ego_vehicle FROM Vehicle ORDER BY id").fetchall()
        trajectory_rows = db.execute("SELECT vehicle_id, sim_time, position_x, position_y, heading_rad, speed, lane_id "
                                     "FROM Trajectory ORDER BY vehicle_id, sim_time").fetchall()
    return vehicle_rows, trajectory_rows


def read_spec(path: str) -> Dict[str, str]:
    """The ``Spec`` table of a converted dataset (source, lane width, speed limit, ...) as a dict."""
    with sqlite3.connect(f"file:{path}?mode=ro", uri=True) as db:
        return {str(k): v for k, v in db.execute("SELECT key, value FROM Spec").fetchall()}


def write_sqlite(path: str, vehicle_rows: Sequence[Sequence], trajectory_rows: Sequence[Sequence], spec: Optional[Dict] = None):
    """A dataset file with the three tables of the converter's layout (for tests and small synthetic histories)."""
    with sqlite3.connect(path) as db:
        db.execute("CREATE TABLE Spec (key TEXT PRIMARY KEY, value TEXT) WITHOUT ROWID")
        db.execute("CREATE TABLE Vehicle (id INTEGER PRIMARY KEY, type INTEGER NOT NULL, length REAL, width REAL, height REAL, "
                   "is_ego_vehicle INTEGER DEFAULT 0) WITHOUT ROWID")
        db.execute("CREATE TABLE Trajectory (vehicle_id INTEGER NOT NULL, sim_time REAL NOT NULL, position_x REAL NOT NULL, "
                   "position_y REAL NOT NULL, heading_rad REAL NOT NULL, speed REAL DEFAULT 0.0, lane_id INTEGER DEFAULT 0, "
                   "PRIMARY KEY (vehicle_id, sim_time)) WITHOUT ROWID")
        db.executemany("INSERT INTO Spec VALUES (?, ?)", [(str(k), str(v)) for k, v in (spec or {}).items()])
        db.executemany("INSERT INTO Vehicle VALUES (?, ?, ?, ?, ?, ?)", [(tuple(r) + (0,))[:6] for r in vehicle_rows])
        db.executemany("INSERT INTO Trajectory VALUES (?, ?, ?, ?, ?, ?, ?)", [(tuple(r) + (0,))[:7] for r in trajectory_rows])

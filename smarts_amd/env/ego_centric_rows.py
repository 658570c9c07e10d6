"""The ego-centric adapters (reference ``smarts/core/utils/adapters/ego_centric_adapters.py:60-266``) over host copies
of the dense rows (include/smx.h ``smx_outputs``): what ``k_ego_frame`` and ``k_actions_to_world`` compute on the device
(``SimConfig(ego_centric=True)``), restated with the reference's own operations so that the result is comparable with
the reference bit for bit — ``np.matmul`` on the 3 x 3 of ``_gen_ego_frame_matrix`` (``smarts/core/utils/math.py:464-487``),
``np.linalg.inv`` for the way back (:490-505), Python's ``%`` in ``wrap_value`` (:452-461) and ``Heading``
(``coordinates.py:175-184``).  One point at a time, as the adapter does: written for checking, not for speed.

Frame of an agent: ``rows["ego_frame"]`` (px, py, pz, H) where the rows hold it (the device keeps the float64 heading
there); else its ``ego_pos`` row and ``Heading()`` of the float32 heading of ``ego_f32`` widened, which is the frame
of an ``Observation`` built from the same rows.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from .. import _native as nat

LINEAR_TRIPLES = ("LIN_VEL", "LIN_ACC", "LIN_JERK")


def wrap_value(value: float, _min: float, _max: float) -> float:
    """math.py:452-461."""
    v = value
    diff = _max - _min
    if value <= _min:
        v = _max - (_min - value) % diff
    if value > _max:
        v = _min + (value - _max) % diff
    return v


def heading(value: float) -> float:
    """Heading.__new__ (coordinates.py:175-184)."""
    value = value % (2 * math.pi)
    if value > math.pi:
        value -= 2 * math.pi
    return value


def frame_matrix(ego_heading: float) -> np.ndarray:
    """_gen_ego_frame_matrix (math.py:464-470)."""
    m = np.eye(3)
    m[0, 0] = np.cos(-ego_heading)
    m[0, 1] = -np.sin(-ego_heading)
    m[1, 0] = np.sin(-ego_heading)
    m[1, 1] = np.cos(-ego_heading)
    return m


def position_to_ego_frame(position, ego_position, ego_heading) -> list:
    """math.py:473-487."""
    m = frame_matrix(ego_heading)
    rel = np.asarray(position) - np.asarray(ego_position)
    with np.errstate(invalid="ignore"):  # a lidar miss: 0 * inf
        return np.matmul(m, rel.T).T.tolist()


def world_position_from_ego_frame(position, ego_world_position, ego_world_heading) -> list:
    """math.py:490-505."""
    m = np.linalg.inv(frame_matrix(ego_world_heading))
    rot = np.matmul(m, np.asarray(position).T).T
    return (np.asarray(rot) + np.asarray(ego_world_position)).tolist()


def relative_heading(h: float, ego_heading: float) -> float:
    """Heading(adjust_heading(h)) (adapter :72-73, :94)."""
    return heading(wrap_value(h - ego_heading, -math.pi, math.pi))


def ego_frame_dynamics(v) -> np.ndarray:
    """adapter :66-67."""
    return np.array([np.linalg.norm(v[:2]), 0, *v[2:]])


def frames(rows: Dict[str, np.ndarray]):
    """(positions [T, 3], headings [T]) of every agent's frame (module docstring)."""
    if "ego_frame" in rows:
        f = np.asarray(rows["ego_frame"], dtype=np.float64)
        return f[:, :3], f[:, 3]
    # (Heading() of the widened float32, as ObservationBuilder forms EgoVehicleObservation.heading: one float64 ulp
    # from the widened value for some negative headings)
    return (np.asarray(rows["ego_pos"], dtype=np.float64),
            np.array([heading(float(h)) for h in rows["ego_f32"][:, nat.EGO["HEADING"]]], dtype=np.float64))


def ego_centric_rows(rows: Dict[str, np.ndarray], cfg=None, valid: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """``rows``: host arrays with the env and vehicle axes flattened into one.  Returns ``ego_frame``, ``ec_flags``,
    ``ec_ego_f32`` and an ``ec_*`` twin of every position / heading row present (waypoints, neighbours, lidar, road
    waypoints; ``cfg``, a ``SimConfig``, may switch a sensor's rows off).  ``valid``: the agents with an observation
    (default: ``rows["ec_flags"]`` where the rows hold it, else all); the others read flags 0 and zero rows.  Entries
    beyond the rows' counts stay zero."""
    T = rows["ego_pos"].shape[0]
    if valid is None:
        valid = (np.asarray(rows["ec_flags"]) & nat.EC_VALID) != 0 if "ec_flags" in rows else np.ones(T, dtype=bool)
    on = lambda name, key: key in rows and (cfg is None or bool(getattr(cfg, name)))  # noqa: E731
    wp, nb = on("waypoints", "wp_pos"), on("neighbors", "nb_pos")
    lidar = "lidar_point" in rows and (cfg is None or cfg.lidar is not None)
    rw = on("road_waypoints", "rw_pos")
    pos, hd = frames(rows)
    out = {"ego_frame": np.zeros((T, 4)), "ec_flags": np.zeros(T, np.uint8), "ec_ego_f32": np.zeros_like(rows["ego_f32"])}
    for name, have in (("wp_pos", wp), ("wp_heading", wp), ("nb_pos", nb), ("nb_heading", nb), ("lidar_point", lidar),
                       ("rw_pos", rw), ("rw_heading", rw)):
        if have:
            out["ec_" + name] = np.zeros_like(rows[name])
    E = nat.EGO
    for g in np.flatnonzero(valid):
        p, H = pos[g], float(hd[g])
        out["ego_frame"][g] = (*p, H)
        out["ec_flags"][g] = nat.EC_VALID
        f = np.array(rows["ego_f32"][g])
        f[E["HEADING"]] = 0.0
        for k in LINEAR_TRIPLES:
            f[E[k]:E[k] + 3] = ego_frame_dynamics(np.asarray(rows["ego_f32"][g, E[k]:E[k] + 3], dtype=np.float64))
        out["ec_ego_f32"][g] = f
        if wp:
            counts = rows["wp_count"][g]
            P, W = rows["wp_heading"].shape[1:3]
            for q in range(min(int(counts[0]), P)):
                for w in range(min(int(counts[1 + q]), W)):
                    xy = position_to_ego_frame(np.append(rows["wp_pos"][g, q, w, :2], [0]), p, H)[:2]
                    out["ec_wp_pos"][g, q, w] = (*xy, 0.0)
                    out["ec_wp_heading"][g, q, w] = relative_heading(float(rows["wp_heading"][g, q, w]), H)
        if nb:
            for k in range(min(int(rows["nb_count"][g]), rows["nb_heading"].shape[1])):
                out["ec_nb_pos"][g, k] = position_to_ego_frame(rows["nb_pos"][g, k], p, H)
                out["ec_nb_heading"][g, k] = relative_heading(float(rows["nb_heading"][g, k]), H)
        if lidar:
            for k in range(rows["lidar_point"].shape[1]):
                # (a miss is (inf, inf, inf) in the world row: the reference's product yields NaN, written as such)
                out["ec_lidar_point"][g, k] = (position_to_ego_frame(rows["lidar_point"][g, k], p, H)
                                               if rows["lidar_hit"][g, k] else (np.nan, np.nan, np.nan))
        if rw:
            L, Q, R = rows["rw_heading"].shape[1:4]
            for l in range(L):
                if rows["rw_lane"][g, l] < 0:
                    continue
                for q in range(min(int(rows["rw_path_count"][g, l]), Q)):
                    for w in range(min(int(rows["rw_count"][g, l, q]), R)):
                        xy = position_to_ego_frame(np.append(rows["rw_pos"][g, l, q, w, :2], [0]), p, H)[:2]
                        out["ec_rw_pos"][g, l, q, w] = (*xy, 0.0)
                        out["ec_rw_heading"][g, l, q, w] = relative_heading(float(rows["rw_heading"][g, l, q, w]), H)
    return out


def actions_to_world_rows(space: str, actions: np.ndarray, counts: Optional[np.ndarray], rows: Dict[str, np.ndarray]) -> np.ndarray:
    """The action adapters (:195-266) over a flattened action buffer in the layout of ``BatchedSim.step_trajectory``
    ([T, 4, 11], with ``counts``), ``step_target_pose`` ([T, 4]) or ``step_trajectory_with_time`` ([T, 5, M], with
    ``counts``): x, y through ``world_position_from_ego_frame``, headings through ``wrap_value(h + H)``, with the frames
    of ``rows`` (``ego_frame`` / ``ec_flags``, as ``ego_centric_rows`` or the device return them).  Agents with flags 0
    or without an action are copied through.  TrajectoryWithTime converts rows 1, 2, 3 — x, y, heading in the
    provider's layout (trajectory_interpolation_provider.py:31-38); the reference's adapter reads rows 0, 1, 2."""
    a = np.asarray(actions, dtype=np.float64)
    out = a.copy()
    pos, hd = np.asarray(rows["ego_frame"])[:, :3], np.asarray(rows["ego_frame"])[:, 3]
    flags = (np.asarray(rows["ec_flags"]) & nat.EC_VALID) != 0
    for g in np.flatnonzero(flags):
        p, H = pos[g], float(hd[g])
        if space == "TargetPose":
            if np.isnan(a[g, 0]):
                continue
            xy = world_position_from_ego_frame(np.append(a[g, :2], [0]), p, H)[:2]
            out[g, :3] = (*xy, wrap_value(H + float(a[g, 2]), -math.pi, math.pi))
            continue
        n = int(counts[g])
        if n <= 0:
            continue
        if space == "Trajectory":
            cols, rx = list(range(min(n, nat.TRAJ_COLS - 1))) + [nat.TRAJ_COLS - 1], 0
        elif space == "TrajectoryWithTime":
            cols, rx = list(range(min(n, a.shape[2]))), 1
        else:
            raise ValueError(f"{space} actions hold no position or heading")
        for c in cols:
            xy = world_position_from_ego_frame([a[g, rx, c], a[g, rx + 1, c], 0], p, H)[:2]
            out[g, rx, c], out[g, rx + 1, c] = xy
            out[g, rx + 2, c] = wrap_value(float(a[g, rx + 2, c]) + H, -math.pi, math.pi)
    return out

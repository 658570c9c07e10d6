"""``lane_ttc`` (reference ``smarts/env/custom_observations.py:148-280``) over the dense rows of include/smx.h, for
every agent at once: a vectorised NumPy restatement with no ``Observation`` objects.

It is the CPU twin of the device's ``k_lane_ttc`` (``SMX_SENSOR_LANE_TTC``: ``out["lane_ttc"]``,
``out["lane_ttc_flags"]``) — the tests compare the two on the same rows — and what a caller without a GPU uses.  The
function is the one ``custom_observations.lane_ttc(ObservationBuilder.build(rows_of_env, slot, ...))`` computes:
speeds and headings are the float32 values of ``ego_f32``, ``nb_speed`` and ``wp_heading``, positions are float64,
lane identity is ``wp_lane_id`` / ``nb_lane_id`` and ``-1`` never matches.

An agent has a row (``TTC_VALID``) when its observation holds at least one path, ``wp_count[0] > 0``: the rows of
an agent without an observation read zero (include/smx.h).  A kept path without waypoints (``path[0]`` raises in the
reference) leaves the agent without a row too.  ``TTC_INDEX_ERROR`` is set where the closest first waypoint's lane
index is negative or not below the number of kept paths: the reference indexes the per-path lists with it and raises
(lane indices are never negative on a map, so Python's wrap-around of a negative index does not arise).
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np

from .. import _native as nat

_TWO_PI = 2 * math.pi
_CHUNK = 2048  # agents per pass: bounds the [agents, neighbours, paths, waypoints] distance block


def _heading(x: np.ndarray) -> np.ndarray:
    """Heading.__new__ (coordinates.py:175-184) of float64 values."""
    v = np.mod(x, _TWO_PI)
    return np.where(v > math.pi, v - _TWO_PI, v)


def _norm2(dx, dy):
    return np.sqrt(dx * dx + dy * dy)


def _rel_gap(a, b):
    """|a - b| relative to the larger magnitude (0 / 0 -> inf: equal zeros are not a close call)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.maximum(np.abs(a), np.abs(b))
        return np.where((m > 0) & np.isfinite(m), np.abs(a - b) / m, np.inf)


def _runner_up(dist, pos_x, pos_y, best):
    """Along the last axis: the smallest entry of ``dist`` whose position differs from the best entry's (inf if
    none).  Candidates at the very same coordinates tie exactly in any arithmetic — the first one wins everywhere —
    so only a different point can make the choice depend on the last place."""
    bx = np.take_along_axis(pos_x, best[..., None], -1)
    by = np.take_along_axis(pos_y, best[..., None], -1)
    other = (pos_x != bx) | (pos_y != by)
    return np.where(other, dist, np.inf).min(-1)


def _chunk(rows: Dict[str, np.ndarray], lookahead: int, want_margins: bool):
    cnt_all = rows["wp_count"].astype(np.int64)
    n, P, W = rows["wp_heading"].shape
    K = rows["nb_speed"].shape[1]
    values = np.zeros((n, nat.TTC_COUNT), dtype=np.float64)
    flags = np.zeros(n, dtype=np.uint8)
    margin = np.full(n, np.inf)
    n_total = cnt_all[:, 0]
    n_paths = np.minimum(n_total, P)
    cnt = np.minimum(cnt_all[:, 1:], W)
    kept = np.arange(P)[None, :] < n_paths[:, None]                      # [n, P]
    ok = (n_paths > 0) & np.all(~kept | (cnt > 0), axis=1)
    if not ok.any():
        return values, flags, margin
    held = kept[:, :, None] & (np.arange(W)[None, None, :] < cnt[:, :, None]) & ok[:, None, None]  # [n, P, W]
    x, y = rows["wp_pos"][..., 0].astype(np.float64), rows["wp_pos"][..., 1].astype(np.float64)
    # ---- arclength (:205-212): sequential float64 sums in waypoint order (np.cumsum accumulates left to right)
    seg = _norm2(x[..., 1:] - x[..., :-1], y[..., 1:] - y[..., :-1])
    seg = np.where(held[..., 1:], seg, 0.0)
    cum = np.concatenate([np.zeros((n, P, 1)), np.cumsum(seg, axis=-1)], axis=-1)
    # ---- neighbours (:217-254)
    nb_total = rows["nb_count"].astype(np.int64)
    nb_kept = np.minimum(nb_total, K)
    v_lane = rows["nb_lane_id"].astype(np.int64)                          # [n, K]
    live = (np.arange(K)[None, :] < nb_kept[:, None]) & (v_lane >= 0) & ok[:, None]
    lid = rows["wp_lane_id"].astype(np.int64).reshape(n, 1, P * W)
    cand = held.reshape(n, 1, P * W) & (lid == v_lane[:, :, None]) & live[:, :, None]  # [n, K, P*W]
    fx, fy = x.reshape(n, 1, P * W), y.reshape(n, 1, P * W)
    vx, vy = rows["nb_pos"][..., 0].astype(np.float64), rows["nb_pos"][..., 1].astype(np.float64)
    gap = np.where(cand, _norm2(fx - vx[:, :, None], fy - vy[:, :, None]), np.inf)
    best = gap.argmin(-1)                                                 # first of equal distances (min(), :230-232)
    best_gap = np.take_along_axis(gap, best[..., None], -1)[..., 0]
    near = cand.any(-1) & ~(best_gap > 2)
    lane_dist = np.take_along_axis(cum.reshape(n, 1, P * W), best[..., None], -1)[..., 0]
    path = best // W
    ego_speed = rows["ego_f32"][:, nat.EGO["SPEED"]].astype(np.float64)
    rel_raw = (ego_speed[:, None] - rows["nb_speed"].astype(np.float64)) * 1000 / 3600
    rel = np.where(np.abs(rel_raw) < 1e-5, 1e-5, rel_raw)
    ttc = lane_dist / rel / 10
    counts = near & ~(ttc <= 0)
    ttc_by_path = np.full((n, P), 1000.0)
    dtc_by_path = np.full((n, P), 1.0)
    who = np.arange(n)
    for k in range(K):  # (one neighbour of every agent at a time: an agent's entries never collide inside a step)
        m = counts[:, k]
        i, p = who[m], path[m, k]
        ttc_by_path[i, p] = np.minimum(ttc_by_path[i, p], ttc[m, k])
        dtc_by_path[i, p] = np.minimum(dtc_by_path[i, p], lane_dist[m, k] / 100)
    # ---- the closest first waypoint (:164-176)
    ex, ey = rows["ego_pos"][:, 0].astype(np.float64), rows["ego_pos"][:, 1].astype(np.float64)
    first_d = np.where(kept & ok[:, None], _norm2(x[:, :, 0] - ex[:, None], y[:, :, 0] - ey[:, None]), np.inf)
    first = first_d.argmin(-1)
    pick = lambda a: a[who, first, 0]  # noqa: E731
    wp_heading = _heading(pick(rows["wp_heading"]).astype(np.float64))
    ego_heading = _heading(rows["ego_f32"][:, nat.EGO["HEADING"]].astype(np.float64))
    # Heading.direction_vector (coordinates.py:241-243) through the host's libm, as the object route takes it
    angle = np.mod(wp_heading + math.pi * 0.5, _TWO_PI)
    d0 = np.array([math.cos(v) for v in angle])
    d1 = np.array([math.sin(v) for v in angle])
    p1x, p1y = pick(x), pick(y)
    p2x, p2y = p1x + d0, p1y + d1
    # Waypoint.signed_lateral_error (road_map.py:608-614) over signed_dist_to_line (utils/math.py:163-185)
    u = np.abs(d1 * ex - d0 * ey + p2x * p1y - p2y * p1x)
    side = np.sign((ex - p1x) * -d1 + (ey - p1y) * d0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lateral = u / _norm2(d0, d1) * side
        values[:, nat.TTC["DIST_FROM_CENTER"]] = lateral / (pick(rows["wp_lane_width"]).astype(np.float64) * 0.5)
    values[:, nat.TTC["ANGLE_ERROR"]] = _heading(_heading(wp_heading - ego_heading))  # Heading.relative_to
    # ---- _ego_ttc_calc (:259-280): the per-path lists indexed by LANE index
    li = pick(rows["wp_lane_index"]).astype(np.int64)
    index_error = (li < 0) | (li >= n_paths)
    for j in range(3):  # right, current, left
        p = li - 1 + j
        have = ~index_error & (p >= 0) & (p < n_paths)
        q = np.where(have, p, 0)
        values[:, nat.TTC["TTC"] + j] = np.where(have, ttc_by_path[who, q], 0.0)
        values[:, nat.TTC["DTC"] + j] = np.where(have, dtc_by_path[who, q], 0.0)
    truncated = (n_total > P) | (nb_total > K) | (W < lookahead + 1)
    flags[:] = (nat.TTC_VALID | np.where(nb_total > 0, nat.TTC_STD, 0) | np.where(truncated, nat.TTC_TRUNCATED, 0)
                | np.where(index_error, nat.TTC_INDEX_ERROR, 0))
    values[~ok] = 0.0
    flags[~ok] = 0
    if want_margins:
        has = cand.any(-1)
        second = _runner_up(gap, np.broadcast_to(fx, gap.shape), np.broadcast_to(fy, gap.shape), best)
        parts = [
            np.where(has, _rel_gap(best_gap, second), np.inf).min(-1, initial=np.inf),            # best two candidates
            np.where(has, np.abs(best_gap - 2) / 2, np.inf).min(-1, initial=np.inf),               # |gap - 2|
            # (ttc = 0 where the nearest waypoint is a path's first one: an exact zero in any arithmetic)
            np.where(near & (lane_dist != 0), np.abs(ttc), np.inf).min(-1, initial=np.inf),        # |ttc|
            np.where(near, np.abs(np.abs(rel_raw) - 1e-5) / 1e-5, np.inf).min(-1, initial=np.inf),  # ||rel| - 1e-5|
            _rel_gap(first_d.min(-1), _runner_up(first_d, x[:, :, 0], y[:, :, 0], first)),         # best two first waypoints
        ]
        margin = np.where(ok, np.min(parts, axis=0), np.inf)
    return values, flags, margin


def lane_ttc_rows(rows: Dict[str, np.ndarray], cfg, margins: bool = False):
    """``rows``: host copies of the dense rows, every array with the same leading agent axes (``[n, ...]`` or
    ``[E, N, ...]``); ``cfg``: the ``SimConfig`` they were written under (its ``wp_lookahead`` decides
    ``TTC_TRUNCATED``; the row lengths are the arrays' own).  Returns ``(values[..., 8], flags[...])``: the columns
    ``_native.TTC`` and the ``TTC_*`` bits of include/smx.h; rows without ``TTC_VALID`` are zero.

    ``margins=True`` adds a third array: per agent the smallest relative margin of the decisions that hang on the
    last place of a distance — the two best candidate waypoints of a neighbour, ``|gap - 2|``, ``|ttc|``,
    ``||rel| - 1e-5|`` and the two best first waypoints (inf where no such decision was taken).  Two implementations
    that round a distance differently may disagree on an agent whose margin is of the order of a float64 epsilon."""
    lead = rows["wp_count"].shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    keys = ("wp_count", "wp_pos", "wp_heading", "wp_lane_width", "wp_lane_index", "wp_lane_id", "nb_count", "nb_pos",
            "nb_speed", "nb_lane_id", "ego_pos", "ego_f32")
    flat = {k: np.asarray(rows[k]).reshape((n,) + tuple(np.shape(rows[k])[len(lead):])) for k in keys}
    values = np.zeros((n, nat.TTC_COUNT), dtype=np.float64)
    flags = np.zeros(n, dtype=np.uint8)
    margin = np.full(n, np.inf)
    for a in range(0, n, _CHUNK):
        sl = slice(a, min(n, a + _CHUNK))
        values[sl], flags[sl], margin[sl] = _chunk({k: v[sl] for k, v in flat.items()}, int(cfg.wp_lookahead), margins)
    out = (values.reshape(lead + (nat.TTC_COUNT,)), flags.reshape(lead))
    return out + (margin.reshape(lead),) if margins else out

"""A NumPy model of delayed agent entry (include/smx.h smx_set_agent_entry; trap_manager.py:121-241 without a capture
zone), shared by the CPU and GPU tests.

Given the ready ticks and check rows of one episode and, per tick, the poses, presence and boxes of every social slot as
the control phase leaves them, ``run`` plays the rule tick by tick: agents in slot order, a pending agent whose ready
tick has come is BLOCKED when an alive social slot lies at ``dx*dx + dy*dy <= (0.5 * (max(l, w) + dim)) ** 2`` from its
check point, else it ENTERS at that tick.  It also reports the smallest ``|distance - radius|`` it met over every
(tick, agent, slot) it evaluated, so a test can assert that no decision of its case sits on the boundary, where the
device's and the model's pose arithmetic could part.

``scripted_poses`` gives the poses of the scripted lane followers from the oracle's own ``SocialBody`` (the model the
parity tests hold the device to), so a case can be decided before it touches the device.
"""
import math

import numpy as np

PENDING, BLOCKED, ENTERED = 0, 1, 2  # SMX_ENTRY_*
SEDAN = (3.68, 1.47)


def run(ready, check, social_xy, social_alive, social_lw=None):
    """``ready`` int (E, A); ``check`` float64 (E, A, 3); ``social_xy`` float64 (T, E, S, 2): the slots' positions in tick
    1..T (index t - 1); ``social_alive`` bool (T, E, S); ``social_lw`` float64 (E, S, 2) or (T, E, S, 2) (None: sedans).
    Returns ``status`` uint8 (T + 1, E, A) — row 0 after the reset, row t after tick t —, ``entered`` int32 (E, A) and
    the smallest clearance met (inf when no slot was ever evaluated)."""
    ready = np.asarray(ready)
    E, A = ready.shape
    T = social_xy.shape[0]
    S = social_xy.shape[2]
    if social_lw is None:
        social_lw = np.broadcast_to(np.array(SEDAN, dtype=np.float64), (E, S, 2))
    if social_lw.ndim == 3:
        social_lw = np.broadcast_to(social_lw, (T,) + social_lw.shape)
    status = np.where(ready == 0, ENTERED, PENDING).astype(np.uint8)
    entered = np.where(ready == 0, 0, -1).astype(np.int32)
    history = [status.copy()]
    clearance = math.inf
    for t in range(1, T + 1):
        for e in range(E):
            for a in range(A):
                if status[e, a] == ENTERED or t < ready[e, a]:
                    continue
                cx, cy, dim = (float(v) for v in check[e, a])
                hit = False
                for s in range(S):
                    if not social_alive[t - 1, e, s]:
                        continue
                    l, w = (float(v) for v in social_lw[t - 1, e, s])
                    dx = float(social_xy[t - 1, e, s, 0]) - cx
                    dy = float(social_xy[t - 1, e, s, 1]) - cy
                    r = 0.5 * (max(l, w) + dim)
                    d2 = dx * dx + dy * dy
                    clearance = min(clearance, abs(math.sqrt(d2) - r))
                    hit = hit or d2 <= r ** 2
                if hit:
                    status[e, a] = BLOCKED
                else:
                    status[e, a] = ENTERED
                    entered[e, a] = t
        history.append(status.copy())
    return np.stack(history), entered, clearance


def scripted_poses(road_map, cm, where, num_agents, num_social, E, T, factor, dt=0.1):
    """Positions (T, E, S, 2) of the scripted social slots over ticks 1..T, from their spawn rows ``where`` (one episode,
    ``[E * N, 2]`` lane index, arclength as ``make_spawns(return_lanes=True)`` gives them), through the oracle's
    ``SocialBody`` (constant fraction ``factor`` of the limit)."""
    from oracle.sim import SocialBody

    N = num_agents + num_social
    out = np.zeros((T, E, num_social, 2), dtype=np.float64)
    for e in range(E):
        for s in range(num_social):
            lane, off = where[e * N + num_agents + s]
            body = SocialBody(0.0, 0.0, 0.0, 0.0, road_map.lane_by_id(cm.lane_ids[int(lane)]), float(off), num_agents + s, factor)
            for t in range(T):
                body.step(dt)
                out[t, e, s] = (body.x, body.y)
    return out

"""History agents (include/smx.h smx_set_history_agents): the synthetic scene the tests follow, and the rules restated in
NumPy — which agent follows, has left or never entered at every tick, the row it stands on, its expert action and the
env's done count — for tests/test_gpu_history_agents.py to hold the device to.

The scene extends ``traffic_history_ref.scene``: vehicles along lane centre lines, in ``SLOTS`` slots.
 - STANDING stands still in the longest lane A in every frame;
 - DRIVER drives down lane A at 8 m/s from GAP metres behind it, speeding up a little and its heading wobbling by a few
   milliradians frame by frame (so that both words of the expert action are non-zero): a follower of it runs into
   STANDING within the run;
 - LEAVER (frames 0 .. LEAVER_LAST) drives down a lane B of another road and leaves mid-run; LATE (from LATE_FIRST on)
   takes its slot once that has stood empty, on a lane far away.
"""
import math

import numpy as np

from smarts_amd import _native as nat
from smarts_amd.traffic_history import TrafficHistoryTable
from traffic_history_ref import lane_pose

STANDING, DRIVER, LEAVER, LATE = 11, 22, 33, 44
FRAMES, AGENTS, SLOTS, DT = 40, 3, 3, 0.1
GAP = 9.0
LEAVER_LAST, LATE_FIRST = 17, 20
E = 4
N = AGENTS + SLOTS

# The follow table of the rule tests, one row per episode.  Episode 0: env 0 follows the driver and the leaver, its agent 2
# nothing; env 1's agent 2 follows LATE, which its reset frame lacks; env 2 follows nothing at all; env 3 also hides
# STANDING through `replaced`.  Episode 1 moves everybody.
FOLLOW = np.array([[[DRIVER, LEAVER, -1], [DRIVER, STANDING, LATE], [-1, -1, -1], [LEAVER, DRIVER, -1]],
                   [[LEAVER, -1, DRIVER], [-1, DRIVER, -1], [STANDING, DRIVER, LEAVER], [DRIVER, -1, -1]]], dtype=np.int32)
STARTS = np.array([[0, 2, 1, 0], [3, 0, 5, 30]], dtype=np.int32)
REPLACED = np.array([[-1, -1, -1, STANDING], [-1, STANDING, -1, -1]], dtype=np.int32)


def scene(cm):
    """dict(table, spawns [1, N, 4] for one env — what a sim without the binding spawns its agents at: one point far from
    the scene —, social_spawns [1, N, 2], far (its distance in metres from the nearest recorded pose of STANDING, DRIVER
    and LEAVER))."""
    lanes = [i for i in range(cm.n_lanes) if not cm.lane_in_junction[i]]
    a = max(lanes, key=lambda i: cm.lane_length[i])
    b = next(i for i in sorted(lanes, key=lambda i: -cm.lane_length[i]) if cm.lane_road[i] != cm.lane_road[a])
    at_a = np.array(lane_pose(cm, a, 5.0 + GAP)[:2])
    c = max((i for i in lanes if i not in (a, b)), key=lambda i: float(np.hypot(*(cm.lane_shape(i)[0] - at_a))))
    veh = [(v, 2, None, None, None) for v in (STANDING, DRIVER, LEAVER, LATE)]
    t = lambda k: round(k * DT, 6)  # noqa: E731
    traj = []
    x, y, h = lane_pose(cm, a, 5.0 + GAP)
    traj += [(STANDING, t(k), x, y, h, 0.0) for k in range(FRAMES)]
    for k in range(FRAMES):
        x, y, h = lane_pose(cm, a, 5.0 + 0.8 * k)
        traj.append((DRIVER, t(k), x, y, h + 0.004 * math.sin(1.3 * k), 8.0 + 0.05 * k))
    for k in range(LEAVER_LAST + 1):
        x, y, h = lane_pose(cm, b, 5.0 + 0.5 * k)
        traj.append((LEAVER, t(k), x, y, h + 2 * math.pi * (k % 2) - 0.003 * k, 5.0 - 0.02 * k))  # (the table wraps the turn)
    for k in range(LATE_FIRST, FRAMES):
        x, y, h = lane_pose(cm, c, 2.0 + 0.3 * (k - LATE_FIRST))
        traj.append((LATE, t(k), x, y, h, 3.0))
    table = TrafficHistoryTable.from_rows(veh, traj, DT, SLOTS)
    # the spawn rows: the lane point (2 m grid) farthest from every recorded pose of the three vehicles an agent may follow
    scene_xy = table.frames[(table.vehicle >= 0) & (table.vehicle != LATE)][:, :2]
    far, where = max((float(np.hypot(*(scene_xy - np.array(lane_pose(cm, i, off)[:2])).T).min()), (i, off))
                     for i in lanes for off in np.arange(1.0, float(cm.lane_length[i]) - 1.0, 2.0))
    spawns = np.zeros((1, N, 4))
    spawns[0, :] = lane_pose(cm, *where) + (0.0,)
    social = np.zeros((1, N, 2))
    social[0, :, 0] = a
    return dict(table=table, spawns=spawns, social_spawns=social, far=far, lanes=(a, b, c))


def blanked(table, ids):
    """The table without the vehicles ``ids``, every other vehicle in the slot it had (the plain constructor)."""
    vehicle = np.where(np.isin(table.vehicle, list(ids)), -1, table.vehicle).astype(np.int32)
    return TrafficHistoryTable(table.frames.copy(), vehicle, table.dt)


def find(table, frame, vid):
    """The slot of ``vid`` in ``frame``, -1 where the frame lacks it (or lies outside the table, or vid < 0)."""
    if vid < 0 or not 0 <= frame < table.num_frames:
        return -1
    hit = np.nonzero(table.vehicle[frame] == vid)[0]
    return int(hit[0]) if len(hit) else -1


def expert_action(table, frame, vid):
    """Rule 4 for one (frame, vehicle), float64: NaN, NaN where frame + 1 lacks the vehicle."""
    s0, s1 = find(table, frame, vid), find(table, frame + 1, vid)
    if s0 < 0 or s1 < 0:
        return np.array([np.nan, np.nan])
    held = table.frames_of(vid)
    return table.expert_actions(vid)[int(np.nonzero(held == frame)[0][0])]


class Model:
    """The rules for one batch: call ``reset(episodes)`` / ``step()`` beside the sim; read ``status`` [E, A] (SMX_HA_*),
    ``row`` [E, A, 4] (the words a following agent holds; NaN elsewhere), ``last_heading`` / ``last_dt`` [E, A],
    ``action`` [E, A, 2] float64, ``done_count`` [E], ``alive`` [E, A]."""

    def __init__(self, table, starts, follow, reset_elapsed_steps, envs=E, agents=AGENTS):
        self.table, self.starts, self.follow, self.res = table, np.asarray(starts), np.asarray(follow), int(reset_elapsed_steps)
        self.E, self.A = envs, agents
        self.episode = np.full(envs, -1)
        self.ticks = np.zeros(envs, dtype=np.int64)
        self.status = np.full((envs, agents), nat.HA_ABSENT)
        self.alive = np.zeros((envs, agents), dtype=bool)
        self.row = np.full((envs, agents, 4), np.nan)
        self.last_heading = np.zeros((envs, agents))
        self.last_dt = np.zeros((envs, agents))
        self.action = np.full((envs, agents, 2), np.nan)
        self.done_count = np.zeros(envs, dtype=np.int64)

    def table_row(self, e):
        return int(self.episode[e]) % self.starts.shape[0]

    def frame(self, e):
        return int(self.starts[self.table_row(e), e]) + int(self.ticks[e])

    def followed(self, e, a):
        return int(self.follow[self.table_row(e), e, a])

    def reset_env(self, e):
        self.episode[e] += 1
        self.ticks[e] = self.res
        f = self.frame(e)
        for a in range(self.A):
            v = self.followed(e, a)
            s = find(self.table, f, v)
            self.alive[e, a] = s >= 0
            self.status[e, a] = nat.HA_FOLLOWING if s >= 0 else nat.HA_ABSENT
            self.row[e, a] = self.table.frames[f, s] if s >= 0 else np.nan
            self.last_heading[e, a] = 0.0
            self.last_dt[e, a] = 0.0
            self.action[e, a] = expert_action(self.table, f, v) if s >= 0 else np.nan
        self.done_count[e] = int((~self.alive[e]).sum())

    def reset(self):
        for e in range(self.E):
            self.reset_env(e)

    def step(self, auto_reset=False):
        """One following tick.  Returns (left [E, A], env_done [E]) of the tick; under auto_reset the envs that ended are
        restarted afterwards, as the device's reset pass does."""
        left = np.zeros((self.E, self.A), dtype=bool)
        for e in range(self.E):
            f = self.frame(e) + 1
            for a in range(self.A):
                if not self.alive[e, a]:
                    continue
                v = self.followed(e, a)
                s = find(self.table, f, v)
                if s < 0:
                    left[e, a] = True
                    self.alive[e, a] = False
                    self.status[e, a] = nat.HA_LEFT
                    self.action[e, a] = np.nan
                    self.done_count[e] += 1
                    continue
                self.last_heading[e, a] = self.row[e, a, 2]
                self.last_dt[e, a] = self.table.dt
                self.row[e, a] = self.table.frames[f, s]
                self.action[e, a] = expert_action(self.table, f, v)
            self.ticks[e] += 1
        env_done = self.done_count >= self.A
        if auto_reset:
            for e in np.nonzero(env_done)[0]:
                self.reset_env(e)
        return left, env_done

    def social_present(self, e, replaced, ahead=0):
        """Presence of every social slot of env ``e`` in its current frame (+ ``ahead``): the table's, less ``replaced``
        and every followed id of the env."""
        f = self.frame(e) + ahead
        out = np.zeros(self.table.num_slots, dtype=bool)
        gone = {self.followed(e, a) for a in range(self.A)} | ({int(replaced[self.table_row(e), e])} if replaced is not None else set())
        for k in range(self.table.num_slots):
            v = self.table.vehicle_at(f, k)
            out[k] = v >= 0 and v not in gone
        return out

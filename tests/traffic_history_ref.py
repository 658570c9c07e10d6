"""Traffic-history replay for the oracle, and the synthetic scene the GPU tests replay (tests/test_gpu_traffic_history.py).

``oracle/`` knows scripted social vehicles only.  A replayed one is a body whose ``step()`` copies the table's row of
the frame the coming observation belongs to, owned by an object whose ``alive`` follows the table's presence rule;
``install`` puts them into ``OracleEnv.social`` after construction (``OracleEnv._vehicles`` filters on ``alive``, and
``OracleEnv.step`` steps every social body before collisions and sensors: the place the device gives the replay)."""
import math

import numpy as np

from oracle.dynamics import VehicleBody
from smarts_amd.engine import lane_heading
from smarts_amd.traffic_history import TrafficHistoryTable


class HistoryBody(VehicleBody):
    """The vehicle in social slot ``slot`` of ``env``: frame = start_frame + the tick count the observation reports."""

    def __init__(self, env, table, slot, start_frame, replaced=-1):
        super().__init__(0.0, 0.0, 0.0, 0.0)
        self.env, self.table, self.slot, self.start_frame, self.replaced = env, table, slot, int(start_frame), int(replaced)
        self.present = False
        self._copy(self.start_frame + env.step_count + 1)  # the reset observation (OracleEnv counts it after observing)

    def _copy(self, frame):
        vid = self.table.vehicle_at(frame, self.slot)
        self.present = vid >= 0 and vid != self.replaced
        if self.present:
            self.x, self.y, self.heading, self.u = (float(v) for v in self.table.frames[frame, self.slot])
            self.v = self.yaw_rate_z = 0.0

    def control(self, *a, **k):
        pass

    def step(self, dt):
        self._copy(self.start_frame + self.env.step_count + 1)


class HistorySocial:
    collisions = ()

    def __init__(self, body):
        self.body = body

    @property
    def alive(self):
        return self.body.present


def install(oracle_batch, table, start_frames, replaced=None):
    """Replace the social vehicles of every env of a ``parity.OracleBatch`` (``start_frames`` / ``replaced``: per env)."""
    for e, env in enumerate(oracle_batch.envs):
        hidden = -1 if replaced is None else int(replaced[e])
        env.social = [HistorySocial(HistoryBody(env, table, k, start_frames[e], hidden)) for k in range(table.num_slots)]


# ---------------------------------------------------------------------------------------------------------------------
def lane_pose(cm, lane, offset):
    """(x, y, heading) at arclength ``offset`` of a lane's centre line."""
    sh = cm.lane_shape(lane)
    acc, cum = 0.0, [0.0]
    for a, b in zip(sh[:-1], sh[1:]):
        acc += math.hypot(float(a[0] - b[0]), float(a[1] - b[1]))
        cum.append(acc)
    seg = min(max(int(np.searchsorted(cum, offset, side="right") - 1), 0), len(cum) - 2)
    f = (offset - cum[seg]) / (cum[seg + 1] - cum[seg])
    return (float(sh[seg, 0] + (sh[seg + 1, 0] - sh[seg, 0]) * f), float(sh[seg, 1] + (sh[seg + 1, 1] - sh[seg, 1]) * f),
            lane_heading(sh, seg))


STANDING, FIRST, SECOND, OFF_ROAD = 11, 22, 33, 44  # the history's vehicle ids
FRAMES, AGENTS, SLOTS, DT = 40, 2, 3, 0.1
GAP = 14.0  # metres from agent 0's spawn to the standing vehicle, centre to centre


def scene(cm):
    """A synthetic history along lane centre lines and the spawn rows that go with it, the same in every env:
     - agent 0 starts 5 m into the longest lane A at its speed limit, agent 1 on a lane of another road;
     - vehicle STANDING stands still in lane A, GAP metres ahead of agent 0's spawn, in every frame: agent 0 runs into it;
     - FIRST (frames 0..9, at the start of its lane) and SECOND (frames 11..30, half way down its lane) share one slot, on
       the two lanes whose starts lie farthest apart: opposite sides of the map;
     - OFF_ROAD (frames 4..20) creeps along off the road, 3 m inside the corner of the lanepoint grid.
    Returns dict(table, spawns [1, N, 4] for one env, social_spawns [1, N, 2], lanes)."""
    lanes = [i for i in range(cm.n_lanes) if not cm.lane_in_junction[i]]
    a = max(lanes, key=lambda i: cm.lane_length[i])
    b = next(i for i in sorted(lanes, key=lambda i: -cm.lane_length[i]) if cm.lane_road[i] != cm.lane_road[a])
    start = {i: cm.lane_shape(i)[0] for i in lanes if i not in (a, b)}
    far1, far2 = max(((i, j) for i in start for j in start if i < j),
                     key=lambda ij: float(np.hypot(*(start[ij[0]] - start[ij[1]]))))
    veh = [(v, 2, None, None, None) for v in (STANDING, FIRST, SECOND, OFF_ROAD)]
    traj = []
    t = lambda k: round(k * DT, 6)  # noqa: E731
    x, y, h = lane_pose(cm, a, 5.0 + GAP)
    traj += [(STANDING, t(k), x, y, h, 0.0) for k in range(FRAMES)]
    for vid, lane, k0, k1, at in ((FIRST, far1, 0, 10, 5.0), (SECOND, far2, 11, 31, 0.5 * float(cm.lane_length[far2]))):
        for k in range(k0, k1):
            x, y, h = lane_pose(cm, lane, at + 0.5 * (k - k0))  # 5 m/s
            traj.append((vid, t(k), x, y, h + 2 * math.pi * (k % 2), 5.0))  # (every second heading a turn off: the table wraps it)
    cx, cy = float(cm.lpg_origin[0]) + 3.0, float(cm.lpg_origin[1]) + 3.0
    traj += [(OFF_ROAD, t(k), cx + 0.05 * (k - 4), cy, -0.5 * math.pi, 0.5) for k in range(4, 21)]
    table = TrafficHistoryTable.from_rows(veh, traj, DT, SLOTS)
    N = AGENTS + SLOTS
    spawns = np.zeros((1, N, 4))
    spawns[0, 0] = lane_pose(cm, a, 5.0) + (cm.lane_speed[a],)
    spawns[0, 1] = lane_pose(cm, b, 5.0) + (cm.lane_speed[b],)
    spawns[0, AGENTS:] = spawns[0, 0]  # (never read while the history is bound)
    social = np.zeros((1, N, 2))
    social[0, :, 0] = a
    return dict(table=table, spawns=spawns, social_spawns=social, lanes=(a, b, far1, far2))

"""Per-vehicle dimensions of a replayed history for the oracle and the tests (tests/test_gpu_traffic_history_dims.py):
the scene, ``HistoryBody`` with the box of the vehicle its frame holds, and the test-side lidar reference.

``oracle/`` already takes ``body.length / .width / .height`` per body in ``boxes_within``, ``ogm`` and the neighbour rows;
its lidar (``sensors_extra._ray_box``) has the sedan's box built in, so ``lidar_ref`` restates it here with the box per
body and the device's vertical rule: the box keeps the sedan's underside, BASE_HEIGHT + 0.1, and rises by the vehicle's
height (the reference centres a BoxChassis box on z = 0; this path stands every vehicle on the ground)."""
import math

import numpy as np

import traffic_history_ref as base
from oracle.dynamics import CHASSIS_HEIGHT, CHASSIS_LENGTH, CHASSIS_WIDTH, VehicleBody
from oracle.sensors_extra import BASE_HEIGHT, CHASSIS_BOX_Z
from smarts_amd.traffic_history import TrafficHistoryTable

SEDAN = (CHASSIS_LENGTH, CHASSIS_WIDTH, CHASSIS_HEIGHT)

# the history's vehicle ids; (type, length, width, height) as a dataset would hold them
TRUCK, TRAILER, MOTORCYCLE, LATE_TRAILER, PEDESTRIAN = 7, 12, 21, 35, 44
VEHICLE_ROWS = [
    (TRAILER, 3, 10.0, 2.5, 4.0),        # a trailer-sized truck with every value given
    (MOTORCYCLE, 1, None, None, None),   # the type's default: 2.5 x 1.0 x 1.4
    (LATE_TRAILER, 3, 10.0, 2.5, None),  # length and width as NGSIM gives them, the truck's default height 1.89
    (PEDESTRIAN, 4, None, 0, -1),        # each "no value" spelling: 0.5 x 0.5 x 1.6
    (TRUCK, 3, -1, None, 0),             # 5 x 1.91 x 1.89
]
FRAMES, AGENTS, SLOTS, DT = 40, 2, 4, 0.1
SIDE = 1.9    # metres from agent 0's spawn to the standing trailer's centre, across the spawn's heading
AHEAD = 7.5   # ... and along it: the agent's nose is 0.66 m short of the trailer's rear at the spawn, 1 m past it a tick later
LEEWAY = 0.05  # oracle.sim.COLLISION_LEEWAY


def beside(pose, right):
    """(x, y, heading) moved `right` metres along the pose's right axis (cos h, sin h)."""
    x, y, h = pose
    return (x + right * math.cos(h), y + right * math.sin(h), h)


def ahead(pose, forward):
    """... moved `forward` metres along its forward axis (-sin h, cos h)."""
    x, y, h = pose
    return (x - forward * math.sin(h), y + forward * math.cos(h), h)


def scene(cm):
    """``traffic_history_ref.scene``'s lanes and agents with vehicles of mixed types and sizes, the same in every env:
     - agent 0 starts 5 m into the longest lane A at its speed limit; agent 1 25 m into a lane B of another road;
     - TRAILER (10 x 2.5 x 4) stands parallel to lane A at the spawn, its centre SIDE m to the side of the spawn and
       AHEAD m ahead of it, in every frame: a sedan's box passes it 0.43 m clear, the trailer's overlaps the agent's by
       0.085 m.  So near the spawn the agent has not left the line it started on; where the lane bends within the next
       metres the trailer stands on the outside of the bend (on a straight lane: to the right);
     - PEDESTRIAN (0.5 x 0.5 x 1.6) stands 8 m ahead of the spawn, 3 m to the other side;
     - TRUCK (5 x 1.91 x 1.89) follows agent 1 down lane B at 5 m/s from the lane's 5 m mark;
     - MOTORCYCLE (frames 0..9) and LATE_TRAILER (frames 11..30) share one slot, on the two lanes whose starts lie
       farthest apart.
    Returns dict(table, spawns [1, N, 4] for one env, social_spawns [1, N, 2], lanes, trailer_pose)."""
    lanes = [i for i in range(cm.n_lanes) if not cm.lane_in_junction[i]]
    a = max(lanes, key=lambda i: cm.lane_length[i])
    b = next(i for i in sorted(lanes, key=lambda i: -cm.lane_length[i]) if cm.lane_road[i] != cm.lane_road[a])
    start = {i: cm.lane_shape(i)[0] for i in lanes if i not in (a, b)}
    far1, far2 = max(((i, j) for i in start for j in start if i < j),
                     key=lambda ij: float(np.hypot(*(start[ij[0]] - start[ij[1]]))))
    t = lambda k: round(k * DT, 6)  # noqa: E731
    traj = []
    spawn = base.lane_pose(cm, a, 5.0)
    bend = base.lane_pose(cm, a, 5.0 + 2 * AHEAD)[2] - spawn[2]
    bend = (bend + math.pi) % (2 * math.pi) - math.pi  # > 0: the lane turns left (headings count counter-clockwise)
    side = -1.0 if bend < 0.0 else 1.0                 # the trailer's side: right, unless the lane turns right
    trailer_pose = beside(ahead(spawn, AHEAD), side * SIDE)
    traj += [(TRAILER, t(k), *trailer_pose, 0.0) for k in range(FRAMES)]
    traj += [(PEDESTRIAN, t(k), *beside(ahead(spawn, 8.0), -side * 3.0), 0.0) for k in range(FRAMES)]
    traj += [(TRUCK, t(k), *base.lane_pose(cm, b, 5.0 + 0.5 * k), 5.0) for k in range(FRAMES)]
    for vid, lane, k0, k1, at in ((MOTORCYCLE, far1, 0, 10, 5.0), (LATE_TRAILER, far2, 11, 31, 0.5 * float(cm.lane_length[far2]))):
        for k in range(k0, k1):
            traj.append((vid, t(k), *base.lane_pose(cm, lane, at + 0.5 * (k - k0)), 5.0))
    table = TrafficHistoryTable.from_rows(VEHICLE_ROWS, traj, DT, SLOTS)
    N = AGENTS + SLOTS
    spawns = np.zeros((1, N, 4))
    spawns[0, 0] = spawn + (cm.lane_speed[a],)
    spawns[0, 1] = base.lane_pose(cm, b, 25.0) + (cm.lane_speed[b],)
    spawns[0, AGENTS:] = spawns[0, 0]  # (never read while the history is bound)
    social = np.zeros((1, N, 2))
    social[0, :, 0] = a
    return dict(table=table, spawns=spawns, social_spawns=social, lanes=(a, b, far1, far2), trailer_pose=trailer_pose)


def slot_of(table, vid):
    return int(np.nonzero((table.vehicle == vid).any(axis=0))[0][0])


def box_of(table, frame, slot, dims=True):
    """(length, width, height) of what social slot ``slot`` holds in ``frame``: the table's rule, or the sedan's box."""
    vid = table.vehicle_at(frame, slot)
    return tuple(table.resolved_dimensions(vid)) if dims and vid >= 0 else SEDAN


def sized(body, box):
    body.length, body.width, body.height = (float(v) for v in box)
    return body


def closest_pass(cm, sc):
    """Agent 0 abreast of the standing trailer — AHEAD m down the line it starts on, both parallel to the lane — and the
    trailer, as oracle bodies ((agent, trailer with its own box, trailer with the sedan's box)): what the scene
    promises, checked on the CPU with ``oracle.sim.boxes_within`` before any device run."""
    tx, ty, th = sc["trailer_pose"]
    best = ahead(tuple(sc["spawns"][0, 0, :3]), AHEAD)
    agent = VehicleBody(best[0], best[1], best[2], 0.0)
    table = sc["table"]
    own = sized(VehicleBody(tx, ty, th, 0.0), table.resolved_dimensions(TRAILER))
    return agent, own, sized(VehicleBody(tx, ty, th, 0.0), SEDAN)


# ---------------------------------------------------------------------------------------------------------------------
class SizedHistoryBody(base.HistoryBody):
    """``HistoryBody`` whose box is that of the vehicle its frame holds (``dims`` off: the sedan's, as before)."""

    def __init__(self, env, table, slot, start_frame, replaced=-1, dims=True):
        self.dims = dims
        super().__init__(env, table, slot, start_frame, replaced)

    def _copy(self, frame):
        super()._copy(frame)
        if self.present:
            sized(self, box_of(self.table, frame, self.slot, self.dims))


def install(oracle_batch, table, start_frames, replaced=None, dims=True):
    """``traffic_history_ref.install`` with per-vehicle boxes."""
    for e, env in enumerate(oracle_batch.envs):
        hidden = -1 if replaced is None else int(replaced[e])
        env.social = [base.HistorySocial(SizedHistoryBody(env, table, k, start_frames[e], hidden, dims)) for k in range(table.num_slots)]


# ---------------------------------------------------------------------------------------------------------------------
def _ray_box(origin, direction, body):
    """``oracle.sensors_extra._ray_box`` with the body's own half extents and the vertical rule of the module docstring;
    a sedan-high body's centre is the oracle's, BASE_HEIGHT + CHASSIS_BOX_Z."""
    h = body.heading
    f = np.array([-math.sin(h), math.cos(h), 0.0])
    r = np.array([math.cos(h), math.sin(h), 0.0])
    u = np.array([0.0, 0.0, 1.0])
    cz = (BASE_HEIGHT + CHASSIS_BOX_Z) + (0.5 * body.height - 0.5 * CHASSIS_HEIGHT)
    c = np.array([body.x, body.y, cz])
    half = (0.5 * body.length, 0.5 * body.width, 0.5 * body.height)
    rel = origin - c
    tmin, tmax = 0.0, 1.0
    for axis, hw in zip((f, r, u), half):
        o = float(rel @ axis)
        d = float(direction @ axis)
        if d == 0.0:
            if abs(o) > hw:
                return None
            continue
        t1, t2 = (-hw - o) / d, (hw - o) / d
        if t1 > t2:
            t1, t2 = t2, t1
        tmin, tmax = max(tmin, t1), min(tmax, t2)
        if tmin > tmax:
            return None
    return tmin


def lidar_ref(ego, others, rays):
    """``oracle.sensors_extra.lidar`` over sized bodies: (points [R, 3] with inf on a miss, hits [R] bool, the index into
    ``others`` of the body each ray hit first, -1 for the ground or a miss)."""
    origin = np.array([ego.x, ego.y, BASE_HEIGHT]) + np.array([0.0, 0.0, 1.0])
    pts = np.full((len(rays), 3), np.inf)
    hits = np.zeros(len(rays), dtype=bool)
    who = np.full(len(rays), -1, dtype=np.int64)
    for i, d in enumerate(rays):
        best = None
        if d[2] < 0.0:  # ground plane z = 0
            t = -origin[2] / d[2]
            if 0.0 <= t <= 1.0:
                best = t
        for k, b in enumerate(others):
            t = _ray_box(origin, d, b)
            if t is not None and (best is None or t < best):
                best, who[i] = t, k
        if best is not None:
            hits[i] = True
            pts[i] = origin + best * d
    return pts, hits, who

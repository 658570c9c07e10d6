"""Bubbles over a replayed history (include/smx.h smx_set_history_bubbles): the rule restated in
NumPy, the scene and the cases the tests use, for tests/test_history_bubbles_cpu.py to hold to the golden fixture and
tests/test_gpu_history_bubbles.py to hold the device to.

The pass is written the way the reference's ``_sync_cursors`` runs — agents outside, bubbles inside, Python sets — while
the device runs bubbles outside and the agents as a loop over 64-bit masks: the two only agree if the rule is the same.

The scene is one straight line: through the start of the map's longest lane, along that lane's heading there.  Recorded
vehicle ``IDS[i]`` is at arclength ``S0[i] + 0.8 * frame`` of the line in every frame (8 m/s at dt 0.1), so a fixed
bubble ``on_line(centre, length)`` — axis-aligned, as every fixed bubble is — is crossed through its x faces on both maps
(``loop``'s line is 7.6 degrees off the x axis, ``4lane``'s lies on it)."""
import math
from dataclasses import dataclass, field
from typing import Callable, Optional, Tuple

import numpy as np

import history_handover_ref as hand
import history_agents_ref as agents_ref
import mpc_imitation_ref as imit
from smarts_amd import _native as nat
from smarts_amd.traffic_history import TrafficHistoryTable
from traffic_history_ref import lane_pose

SOCIAL, SHADOWED, HIJACKED, RELEASED = nat.BUBBLE_SOCIAL, nat.BUBBLE_SHADOWED, nat.BUBBLE_HIJACKED, nat.BUBBLE_RELEASED
EGO = 4  # an agent the handover table drives in the tick: none of the four
T_NONE, T_AIRLOCK_ENTERED, T_ENTERED, T_EXITED, T_AIRLOCK_EXITED = 0, 1, 2, 3, 4
C_NONE, C_IN_BUBBLE, C_IN_AIRLOCK = 0, 1, 2
CLEARANCE = 1e-6  # metres every (tick, agent, bubble) keeps from both rectangles' edges: a thousand times the 1e-9 poses are held to


@dataclass
class B:
    """One bubble, include/smx.h's smx_bubble."""
    x: float = 0.0
    y: float = 0.0
    size_x: float = 1.0
    size_y: float = 1.0
    margin: float = 2.0
    offset: Tuple[float, float] = (0.0, 0.0)
    follow: int = -1
    hijack_limit: int = 0
    shadow_limit: int = 0

    def native(self):
        return nat.SmxBubble(self.x, self.y, self.size_x, self.size_y, self.margin, self.offset[0], self.offset[1], self.follow,
                             self.hijack_limit, self.shadow_limit)


def zone(b, p, fpos=None, fheading=0.0, rotate=True):
    """(in_bubble, in_airlock, clearance) of point ``p`` at bubble ``b``; ``fpos`` / ``fheading``: the followed agent's
    position and heading (a travelling bubble).  clearance: the least distance of the point, in the bubble's frame, from
    the lines the two rectangles' edges lie on.  ``rotate=False`` leaves the heading out (test case 7's foil)."""
    if b.follow < 0:
        qx, qy = p[0] - b.x, p[1] - b.y
    else:
        h = fheading if rotate else 0.0
        s, c = math.sin(h), math.cos(h)
        dx, dy = p[0] - fpos[0], p[1] - fpos[1]
        qx, qy = c * dx + s * dy - b.offset[0], -s * dx + c * dy - b.offset[1]
    ax, ay, hx, hy = abs(qx), abs(qy), 0.5 * b.size_x, 0.5 * b.size_y
    inner = ax < hx and ay < hy
    outer = ax < hx + b.margin and ay < hy + b.margin
    clearance = min(abs(ax - hx), abs(ay - hy), abs(ax - hx - b.margin), abs(ay - hy - b.margin))
    return inner, outer and not inner, clearance


def transition(state, was_in, in_bubble, in_airlock, hijackable, shadowable):
    """Cursor.from_pos (bubble_manager.py:313-327): the first that holds."""
    if state == SOCIAL and shadowable and in_airlock:
        return T_AIRLOCK_ENTERED
    if state == SHADOWED and hijackable and in_bubble:
        return T_ENTERED
    if state == HIJACKED and in_airlock:
        return T_EXITED
    if was_in and state in (SHADOWED, HIJACKED) and not in_airlock and not in_bubble:
        return T_AIRLOCK_EXITED
    return T_NONE


def cursor_state(in_bubble, in_airlock, hijackable, shadowable):
    if hijackable and in_bubble:
        return C_IN_BUBBLE
    if shadowable and in_airlock:
        return C_IN_AIRLOCK
    return C_NONE


def apply_transition(state, t):
    if t == T_AIRLOCK_ENTERED and state == SOCIAL:
        return SHADOWED
    if t == T_ENTERED and state == SHADOWED:
        return HIJACKED
    if t == T_AIRLOCK_EXITED and state == HIJACKED:
        return RELEASED
    if t == T_AIRLOCK_EXITED and state == SHADOWED:
        return SOCIAL
    return state


def pass_zones(zones, active, alive, ego, state, mask, limits):
    """One env's pass on zone decisions already made.  zones [A, B, 2] bool (in_bubble, in_airlock); active [B]; alive,
    ego [A] bool; state, mask [A] as the pass found them; limits [B, 2] (hijack, shadow; 0 = none).  Returns (state, mask,
    transitions [A, B], cursors [A, B]) after it."""
    A, nb = len(state), len(active)
    seen = [EGO if ego[a] else int(state[a]) for a in range(A)]
    cur = np.zeros((A, nb), dtype=np.int64)
    trans = np.zeros((A, nb), dtype=np.int64)
    for a in range(A):
        if not alive[a]:
            continue
        for j in range(nb):
            if not active[j]:
                continue
            # (a vehicle that is gone is neither hijacked nor shadowed for the index, vehicle_index.py:189-201)
            all_hij = {u for u in range(A) if alive[u] and (int(mask[u]) >> j) & 1 and seen[u] == HIJACKED} | {u for u in range(a) if cur[u, j] == C_IN_AIRLOCK}
            all_shd = {u for u in range(A) if alive[u] and (int(mask[u]) >> j) & 1 and seen[u] == SHADOWED} | {u for u in range(a) if cur[u, j] == C_IN_BUBBLE}
            all_hij -= {a}
            all_shd -= {a}
            hl, sl = int(limits[j][0]), int(limits[j][1])
            hijackable = hl == 0 or len(all_hij) < hl
            shadowable = sl == 0 or len(all_shd) + len(all_hij) < sl
            inb, ina = bool(zones[a, j, 0]), bool(zones[a, j, 1])
            trans[a, j] = transition(seen[a], bool((int(mask[a]) >> j) & 1), inb, ina, hijackable, shadowable)
            cur[a, j] = cursor_state(inb, ina, hijackable, shadowable)
    new_state = np.array(state, dtype=np.int64).copy()
    new_mask = np.zeros(A, dtype=np.int64)
    for a in range(A):
        for j in range(nb):
            new_state[a] = apply_transition(int(new_state[a]), int(trans[a, j]))
            if cur[a, j] != C_NONE:
                new_mask[a] |= 1 << j
    return new_state, new_mask, trans, cur


def bubble_pass(bubbles, pos, heading, alive, ego, state, mask, rotate=True):
    """One env's pass from poses.  Returns pass_zones' four, the least clearance met and the zone decisions [A, B, 2]."""
    A = len(state)
    active = [b.follow < 0 or bool(alive[b.follow]) for b in bubbles]
    zones = np.zeros((A, len(bubbles), 2), dtype=bool)
    least = math.inf
    for a in range(A):
        if not alive[a]:
            continue
        for j, b in enumerate(bubbles):
            if not active[j]:
                continue
            f = b.follow
            inb, ina, c = zone(b, pos[a], pos[f] if f >= 0 else None, float(heading[f]) if f >= 0 else 0.0, rotate)
            zones[a, j] = inb, ina
            least = min(least, c)
    limits = [(b.hijack_limit, b.shadow_limit) for b in bubbles]
    return pass_zones(zones, active, alive, ego, state, mask, limits) + (least, zones)


class Model(hand.Model):
    """history_handover_ref.Model with bubbles: ``step(actions)`` is a tick of smx_step_history_handover with bubbles
    bound (``handover`` may be None: no table).  ``bstate`` / ``bmask`` [E, A] are the two bytes, ``clearance`` the least
    distance any zone test of the run kept from an edge, ``transitions`` the last pass's [E, A, B]."""

    def __init__(self, table, starts, follow, handover, reset_elapsed_steps, bubbles, envs, agents, rotate=True, max_steps=0):
        never = np.full(np.asarray(follow).shape, -1, dtype=np.int32)
        super().__init__(table, starts, follow, never if handover is None else handover, reset_elapsed_steps, envs, agents)
        self.bubbles, self.rotate = list(bubbles), rotate
        self.bstate = np.zeros((envs, agents), dtype=np.int64)
        self.bmask = np.zeros((envs, agents), dtype=np.int64)
        self.transitions = np.zeros((envs, agents, len(self.bubbles)), dtype=np.int64)
        self.zones = np.zeros((envs, agents, len(self.bubbles), 2), dtype=bool)  # the last pass's (in_bubble, in_airlock)
        self.clearance = math.inf
        # SensorState._step per agent and cfg.max_episode_steps (0: none): an alive agent whose count reaches it is done
        # with the tick's observation, whatever it did in the tick.  A test may write ``steps`` (and the device's row).
        self.steps = np.zeros((envs, agents), dtype=np.int64)
        self.max_steps = int(max_steps)

    def reset_env(self, e):
        super().reset_env(e)
        self.bstate[e] = 0
        self.bmask[e] = 0
        self.steps[e] = 1

    def table_driven(self):
        """[E, A]: the agents the handover table drives in the coming tick, alive or not (the pass reads the table alone)."""
        out = np.zeros((self.E, self.A), dtype=bool)
        for e in range(self.E):
            for a in range(self.A):
                out[e, a] = 0 <= self.H(e, a) <= self.ticks[e]
        return out

    def step(self, acts, auto_reset=False):
        """One tick.  Returns (ended [E, A]: left or released — nothing of the state stored —, env_done [E], drive [E, A],
        maxed [E, A]: ended by max_episode_steps after its tick)."""
        ended = np.zeros((self.E, self.A), dtype=bool)
        maxed = np.zeros((self.E, self.A), dtype=bool)
        ego = self.table_driven()
        drive = np.zeros((self.E, self.A), dtype=bool)
        dt = self.table.dt
        for e in range(self.E):
            self.bstate[e], self.bmask[e], self.transitions[e], _, least, self.zones[e] = bubble_pass(
                self.bubbles, self.held[e, :, :2], self.held[e, :, 2], self.alive[e], ego[e], self.bstate[e], self.bmask[e], self.rotate)
            self.clearance = min(self.clearance, least)
            f = self.frame(e) + 1
            for a in range(self.A):
                if not self.alive[e, a]:
                    continue
                self.steps[e, a] += 1
                if self.max_steps > 0 and self.steps[e, a] >= self.max_steps:
                    maxed[e, a] = True
                if ego[e, a] or self.bstate[e, a] == HIJACKED:
                    drive[e, a] = True
                    self.status[e, a] = nat.HA_DRIVEN
                    self.action[e, a] = np.nan
                    self.row[e, a] = np.nan
                    x, y, h, u = (float(v) for v in self.held[e, a])
                    out = imit.imitation_step(x, y, h, u, float(acts[e, a, 0]), float(acts[e, a, 1]), dt)
                    if out is not None:
                        self.last_heading[e, a] = h
                        self.last_dt[e, a] = dt
                        self.held[e, a] = out
                    continue
                v = self.followed(e, a)
                s = agents_ref.find(self.table, f, v)
                if self.bstate[e, a] == RELEASED or s < 0:
                    ended[e, a] = True
                    maxed[e, a] = False
                    self.alive[e, a] = False
                    self.status[e, a] = nat.HA_RELEASED if self.bstate[e, a] == RELEASED else nat.HA_LEFT
                    self.action[e, a] = np.nan
                    self.row[e, a] = np.nan
                    self.done_count[e] += 1
                    continue
                self.status[e, a] = nat.HA_SHADOWED if self.bstate[e, a] == SHADOWED else nat.HA_FOLLOWING
                self.last_heading[e, a] = self.held[e, a, 2]
                self.last_dt[e, a] = dt
                self.row[e, a] = self.held[e, a] = self.table.frames[f, s]
                self.action[e, a] = agents_ref.expert_action(self.table, f, v)
            self.ticks[e] += 1
            self.alive[e] &= ~maxed[e]
            self.done_count[e] += int(maxed[e].sum())
        env_done = self.done_count >= self.A
        if auto_reset:
            for e in np.nonzero(env_done)[0]:
                self.reset_env(e)
        return ended, env_done, drive, maxed


# ---------------------------------------------------------------------------------------------------------------------
# the scene
IDS = (11, 22, 33, 44)
S0 = (0.0, -6.0, -12.0, -18.0)  # arclength of each vehicle in frame 0: 6 m apart
STEP = 0.8                      # metres a frame: 8 m/s at dt 0.1
DT = 0.1
FRAMES = 70
E, AGENTS, SLOTS = 4, 4, 4
N = AGENTS + SLOTS


class Line:
    """The scene's straight line: ``at(s)`` = (x, y) at arclength s, ``heading`` the lane's at its start."""

    def __init__(self, cm, origin=0.0):
        lanes = [i for i in range(cm.n_lanes) if not cm.lane_in_junction[i]]
        self.lane = max(lanes, key=lambda i: cm.lane_length[i])
        self.x0, self.y0, self.heading = lane_pose(cm, self.lane, origin)
        self.dx, self.dy = -math.sin(self.heading), math.cos(self.heading)  # (heading 0 = +y, counter-clockwise)

    def at(self, s, side=0.0):
        """``side``: metres to the left of the line."""
        return self.x0 + self.dx * s - self.dy * side, self.y0 + self.dy * s + self.dx * side

    def on_line(self, centre, length, width=12.0, **kw):
        """A fixed bubble centred at arclength ``centre``, ``length`` along x (the line's axis, nearly), ``width`` along y."""
        x, y = self.at(centre)
        return B(x=x, y=y, size_x=length, size_y=width, **kw)


def scene(cm, ids=IDS, s0=S0, frames=FRAMES, slots=SLOTS, origin=0.0):
    """dict(table, line, spawns [1, slots + agents, 4], social_spawns): the column of vehicles on the line through the
    point ``origin`` metres down the lane, along the lane's heading there."""
    line = Line(cm, origin)
    veh = [(v, 2, None, None, None) for v in ids]
    traj = []
    for v, s in zip(ids, s0):
        for k in range(frames):
            x, y = line.at(s + STEP * k)
            traj.append((v, round(k * DT, 6), x, y, line.heading, STEP / DT))
    table = TrafficHistoryTable.from_rows(veh, traj, DT, slots)
    n = 2 * slots
    spawns = np.zeros((1, n, 4))
    spawns[0, :] = line.at(0.0) + (line.heading, 0.0)
    social = np.zeros((1, n, 2))
    social[0, :, 0] = line.lane
    return dict(table=table, line=line, spawns=spawns, social_spawns=social)


def zero_actions(tick, envs=E, n=N):
    """Zero acceleration and angular velocity for every agent slot (social rows NaN: nobody reads them)."""
    a = np.full((envs, n, 3), np.nan, dtype=np.float32)
    a[:, : n // 2, :] = 0.0
    a[..., 2] = 0.0
    return a


@dataclass
class Case:
    """One test case: what is bound, how long it runs, and what the model must show before the device is touched."""
    name: str
    bubbles: Callable  # line -> [B]
    follow: np.ndarray  # [R, E, A]
    starts: np.ndarray  # [R, E]
    ticks: int
    expect: Callable  # (history: list of per-tick dicts, model) -> None, asserts
    handover: Optional[np.ndarray] = None
    actions: Callable = zero_actions
    cfg: dict = field(default_factory=dict)
    auto_reset: bool = False
    max_steps: int = 0
    steps_at_reset: dict = field(default_factory=dict)  # {(env, agent): SensorState._step written after the reset}


def run_model(case, sc, reset_elapsed_steps, rotate=True, envs=E, agents=AGENTS):
    """A free run of the model over the case.  Returns (model, history): per tick dict(state, mask, status, ended, drive,
    alive, transitions, episode)."""
    m = new_model(case, sc, reset_elapsed_steps, rotate, envs, agents)
    hist = []
    for t in range(case.ticks):
        ended, env_done, drive, maxed = m.step(case.actions(t, envs, 2 * agents), auto_reset=case.auto_reset)
        hist.append(dict(state=m.bstate.copy(), mask=m.bmask.copy(), status=m.status.copy(), ended=ended, drive=drive, alive=m.alive.copy(),
                         transitions=m.transitions.copy(), episode=m.episode.copy(), env_done=env_done, maxed=maxed, held=m.held.copy(),
                         zones=m.zones.copy()))
    return m, hist


def new_model(case, sc, reset_elapsed_steps, rotate=True, envs=E, agents=AGENTS):
    """The case's model after its reset."""
    m = Model(sc["table"], case.starts, case.follow, case.handover, reset_elapsed_steps, case.bubbles(sc["line"]), envs, agents, rotate,
              case.max_steps)
    m.reset()
    for (e, a), v in case.steps_at_reset.items():
        m.steps[e, a] = v
    return m


def states_of(hist, e, a):
    """The run of distinct state bytes agent (e, a) went through, e.g. [0, 1, 2, 3]."""
    out = [0]
    for h in hist:
        s = int(h["state"][e, a])
        if s != out[-1]:
            out.append(s)
    return out


def _follow(rows):
    return np.array(rows, dtype=np.int32)


NOBODY = [-1, -1, -1, -1]


def _case_1_2(hist, m):
    # case 1, env 0 / agent 0 (and every agent of env 1): the through drive
    for e, a in [(0, 0), (1, 0), (1, 1), (1, 2)]:
        assert states_of(hist, e, a) == [SOCIAL, SHADOWED, HIJACKED, RELEASED], (e, a, states_of(hist, e, a))
    assert states_of(hist, 1, 3) == [SOCIAL, SHADOWED, HIJACKED]  # (no limits: the four ride through one behind the other)
    first = lambda e, a, s: next(t for t, h in enumerate(hist) if h["state"][e, a] == s)  # noqa: E731
    t_rel = first(0, 0, RELEASED)
    assert hist[t_rel]["ended"][0, 0] and hist[t_rel]["status"][0, 0] == nat.HA_RELEASED and not hist[t_rel]["alive"][0, 0]
    # released by the first pass that finds it outside both zones: the tick before, that pass found it in the far ring
    assert hist[t_rel - 1]["drive"][0, 0] and hist[t_rel - 1]["zones"][0, 0, 0, 1] and not hist[t_rel]["zones"][0, 0, 0].any()
    assert hist[first(0, 0, SHADOWED)]["status"][0, 0] == nat.HA_SHADOWED
    driven = [t for t, h in enumerate(hist) if h["drive"][0, 0]]
    assert driven == list(range(first(0, 0, HIJACKED), t_rel)) and len(driven) >= 10
    assert any(h["transitions"][0, 0, 0] == T_EXITED for h in hist)  # driven in the far ring too
    # case 2, env 3: the reset frame lies inside the inner zone — never captured, although the cursor has a state
    # (the far ring shadows it on its way out, as the rule has it; it is never hijacked and never driven)
    assert states_of(hist, 3, 0) == [SOCIAL, SHADOWED, SOCIAL] and hist[0]["mask"][3, 0] == 1 and not any(h["drive"][3].any() for h in hist)
    assert m.done_count.tolist()[0] == 4 and m.done_count.tolist()[1] == 3


def case_through_drive():
    """Cases 1 and 2: B0 = 8 m long around arclength 20.  Env 0 follows vehicle 11 alone, env 1 all four, env 2 vehicle
    22 from frame 5, env 3 vehicle 11 from frame 25, where it stands at arclength 20: inside the inner zone."""
    return Case("through_drive", lambda ln: [ln.on_line(20.3, 8.0)],
                _follow([[[11, -1, -1, -1], [11, 22, 33, 44], [22, -1, -1, -1], [11, -1, -1, -1]]]), np.array([[0, 0, 5, 25]], dtype=np.int32), 50,
                _case_1_2)


def _case_3_4(hist, m):
    for e in (0, 1):
        # case 3: a ring of 0.5 m is jumped at 0.8 m a tick — bubble 0 never captures, though the vehicle is inside for ticks
        inside = [t for t, h in enumerate(hist) if h["mask"][e, 0] & 1]
        assert len(inside) >= 3 and all(hist[t]["state"][e, 0] == SOCIAL for t in range(inside[-1] + 2)), (e, inside)
        assert all((h["transitions"][e, 0, 0] == T_NONE) for h in hist)
        # case 4: clips bubble 1's ring only — SHADOWED, FOLLOWING again —, then bubble 2 further on captures it
        assert states_of(hist, e, 0) == [SOCIAL, SHADOWED, SOCIAL, SHADOWED, HIJACKED, RELEASED], (e, states_of(hist, e, 0))
        back = next(t for t, h in enumerate(hist) if h["transitions"][e, 0, 1] == T_AIRLOCK_EXITED)
        assert hist[back]["status"][e, 0] == nat.HA_FOLLOWING and hist[back - 1]["status"][e, 0] == nat.HA_SHADOWED
        assert all(h["transitions"][e, 0, 1] in (T_NONE, T_AIRLOCK_ENTERED, T_AIRLOCK_EXITED) for h in hist)
        assert any(h["transitions"][e, 0, 2] == T_ENTERED for h in hist[back:])


def case_ring_only():
    """Cases 3 and 4, one vehicle (11) per env, env 1 three frames ahead of env 0.  Bubble 0: margin 0.5, on the line.
    Bubble 1 lies beside the line so that only its ring reaches it.  Bubble 2 sits on the line further on."""
    def bubbles(ln):
        x, y = ln.at(17.0, side=6.0)  # inner zone 3 m wide: its near face is 4.5 m from the line, its 5 m ring reaches past it
        # (bubble 0's two rings, [4.1, 4.6] and [8.9, 9.4] along x, lie between the vehicle's positions, multiples of 0.8)
        return [ln.on_line(6.75, 4.3, margin=0.5), B(x=x, y=y, size_x=3.0, size_y=3.0, margin=5.0), ln.on_line(34.4, 5.0)]
    return Case("ring_only", bubbles, _follow([[[11, -1, -1, -1], [11, -1, -1, -1], NOBODY, NOBODY]]), np.array([[0, 3, 0, 0]], dtype=np.int32), 56,
                _case_3_4)


def _brake_first(tick, envs=E, n=N):
    """Zero actions, but env 1's agent 0 is braked to rest by one tick of -80 m/s^2 (8 m/s at dt 0.1) once it is inside."""
    a = zero_actions(tick, envs, n)
    if tick == 24:
        a[1, 0, 0] = -80.0
    return a


def _case_5(hist, m):
    # env 0: the second rides SHADOWED while the first is HIJACKED, and is driven once the first is released
    assert states_of(hist, 0, 0) == [SOCIAL, SHADOWED, HIJACKED, RELEASED] and states_of(hist, 0, 1) == [SOCIAL, SHADOWED, HIJACKED, RELEASED]
    both = [t for t, h in enumerate(hist) if h["state"][0, 0] == HIJACKED and h["state"][0, 1] == SHADOWED]
    assert len(both) >= 6 and sum(bool(hist[t]["zones"][0, 1, 0, 0]) for t in both) >= 4  # ... through the inner zone
    t_rel = next(t for t, h in enumerate(hist) if h["state"][0, 0] == RELEASED)
    assert hist[t_rel]["state"][0, 1] == SHADOWED and hist[t_rel + 1]["state"][0, 1] == HIJACKED and hist[t_rel + 1]["drive"][0, 1]
    # env 1: the first stands inside to the end; the second rides through SHADOWED and is let go, SHADOWED -> SOCIAL
    assert states_of(hist, 1, 0) == [SOCIAL, SHADOWED, HIJACKED] and hist[-1]["drive"][1, 0]
    assert states_of(hist, 1, 1) == [SOCIAL, SHADOWED, SOCIAL] and not any(h["drive"][1, 1] for h in hist)
    assert abs(hist[-1]["held"][1, 0, 3]) < 1e-9  # at rest


def case_hijack_limit():
    """Case 5: hijack_limit = 1, vehicles 11 and 22, 6 m apart, in envs 0 and 1.  At equal speeds the second cannot be
    outside both zones while the first is still hijacked (it is behind it), so no zone length gives the second branch:
    in env 1 the first is braked to rest inside by its action instead, and the second rides through."""
    return Case("hijack_limit", lambda ln: [ln.on_line(20.3, 8.0, hijack_limit=1)],
                _follow([[[11, 22, -1, -1], [11, 22, -1, -1], NOBODY, NOBODY]]), np.array([[0, 0, 0, 0]], dtype=np.int32), 56, _case_5,
                actions=_brake_first)


def _case_6(hist, m):
    # slots 2, 1, 0 follow the first, second and third vehicle: the first two are shadowed and hijacked in turn, the third
    # meets a bubble that holds two and is not shadowed
    assert states_of(hist, 0, 2)[:3] == [SOCIAL, SHADOWED, HIJACKED] and states_of(hist, 0, 1)[:3] == [SOCIAL, SHADOWED, HIJACKED]
    full = [t for t, h in enumerate(hist) if h["state"][0, 1] == HIJACKED and h["state"][0, 2] == HIJACKED]
    turned = [t for t in full if hist[t]["zones"][0, 0, 0, 1] and hist[t]["state"][0, 0] == SOCIAL and hist[t]["mask"][0, 0] == 0]
    assert len(turned) >= 2 and all(hist[t]["state"][0, 0] == SOCIAL for t in range(full[-1] + 1))  # in the ring, and not shadowed
    # env 1, slots in the vehicles' order: the quirk of the running sets — the first counts twice, the second is turned away
    assert states_of(hist, 1, 0)[:3] == [SOCIAL, SHADOWED, HIJACKED]
    assert sum(1 for h in hist if h["zones"][1, 1, 0, 1] and h["state"][1, 1] == SOCIAL and h["mask"][1, 1] == 0 and h["state"][1, 0] == HIJACKED) >= 2


def case_shadow_limit():
    """Case 6: shadow_limit = 2, three vehicles, one bubble 16 m long."""
    return Case("shadow_limit", lambda ln: [ln.on_line(22.3, 16.0, shadow_limit=2)],
                _follow([[[33, 22, 11, -1], [11, 22, 33, -1], NOBODY, NOBODY]]), np.array([[8, 8, 0, 0]], dtype=np.int32), 50, _case_6)


def _turning(tick, envs=E, n=N):
    """Agent 0 of every env speeds up to 12 m/s in the first tick and turns at 0.03 rad/s; the others send zeros."""
    a = zero_actions(tick, envs, n)
    a[:, 0, 0] = 40.0 if tick == 0 else 0.0
    a[:, 0, 1] = 0.03
    return a


TRAVEL_END = 24  # the tick in which env 1's agent 0 ends by max_episode_steps (its own step count is set ahead)
TRAVEL_MAX = 100


def _case_7(hist, m):
    # env 0: the bubble ahead of agent 0 (table-driven from the first tick, never in a state) overtakes vehicle 11
    assert states_of(hist, 0, 0) == [SOCIAL] and all(h["drive"][0, 0] for h in hist)
    assert states_of(hist, 0, 1) == [SOCIAL, SHADOWED, HIJACKED, RELEASED], states_of(hist, 0, 1)
    # env 1: agent 0 ends in tick TRAVEL_END — the bubble is inactive from the next pass on, the bits clear, states freeze
    assert hist[TRAVEL_END]["maxed"][1, 0] and not hist[TRAVEL_END]["alive"][1, 0]
    assert hist[TRAVEL_END]["state"][1, 1] == HIJACKED and hist[TRAVEL_END]["mask"][1, 1] == 1
    assert all(h["state"][1, 1] == HIJACKED and h["mask"][1, 1] == 0 and h["drive"][1, 1] for h in hist[TRAVEL_END + 1:])


def case_travelling():
    """Case 7: one bubble pinned to agent 0, 8 m ahead of it (offset (0, 8): y is ahead), 6 m wide and 4.2 m long.  Agent 0
    follows the rear-most vehicle, 44, and is handed over at tick 0; agent 1 follows vehicle 11, 18 m ahead."""
    handover = np.full((1, E, AGENTS), -1, dtype=np.int32)
    handover[0, :, 0] = 0
    return Case("travelling", lambda ln: [B(size_x=6.0, size_y=4.2, offset=(0.0, 8.0), follow=0)],
                _follow([[[44, 11, -1, -1], [44, 11, -1, -1], NOBODY, NOBODY]]), np.array([[0, 0, 0, 0]], dtype=np.int32), 52, _case_7,
                handover=handover, actions=_turning, max_steps=TRAVEL_MAX, steps_at_reset={(1, 0): TRAVEL_MAX - (TRAVEL_END + 1)},
                cfg=dict(max_episode_steps=TRAVEL_MAX))


RESTART_MAX = 26  # every agent ends in tick RESTART_MAX - 2


def _case_8(hist, m):
    t_end = RESTART_MAX - 2
    assert hist[t_end - 1]["state"][0, 0] == HIJACKED and hist[t_end - 1]["episode"][0] == 0
    # the env restarted inside the tick: the new episode starts from SOCIAL with a zero mask and follows row 1
    assert hist[t_end]["episode"][0] == 1 and hist[t_end]["state"][0].tolist() == [0] * 4 and hist[t_end]["mask"][0].tolist() == [0] * 4
    assert hist[t_end]["status"][0, 1] == nat.HA_FOLLOWING and hist[t_end]["status"][0, 0] == nat.HA_ABSENT
    assert states_of(hist[t_end:], 0, 1)[:3] == [SOCIAL, SHADOWED, HIJACKED]  # row 1's follower is captured in its turn
    assert m.episode.tolist()[0] >= 2  # ... and a second restart


def case_auto_reset():
    """Case 8: auto_reset, two rows.  Episode 0: env 0's agent 0 follows vehicle 11 and is HIJACKED when every agent ends by
    max_episode_steps; episode 1: its agent 1 follows vehicle 22 from frame 10."""
    return Case("auto_reset", lambda ln: [ln.on_line(18.3, 8.0)],
                _follow([[[11, -1, -1, -1], [11, 22, -1, -1], NOBODY, [33, -1, -1, -1]], [[-1, 22, -1, -1], [22, -1, 11, -1], NOBODY, [-1, -1, -1, 44]]]),
                np.array([[0, 2, 0, 4], [10, 8, 0, 30]], dtype=np.int32), 56, _case_8, auto_reset=True, max_steps=RESTART_MAX,
                cfg=dict(max_episode_steps=RESTART_MAX, auto_reset=True))


CASES = {c.name: c for c in (case_through_drive(), case_ring_only(), case_hijack_limit(), case_shadow_limit(), case_travelling(),
                             case_auto_reset())}

# ---- case 9, the width: E = 3, 32 agent slots + 32 replayed slots, a column of 32 vehicles 4 m apart
WIDE_E, WIDE_AGENTS = 3, 32
WIDE_IDS = tuple(100 + i for i in range(WIDE_AGENTS))
WIDE_S0 = tuple(-4.0 * i for i in range(WIDE_AGENTS))


def wide_scene(cm):
    # (the column is 124 m long: the line starts 40 m down the lane so that its tail lies inside the map's grids)
    return scene(cm, WIDE_IDS, WIDE_S0, frames=60, slots=WIDE_AGENTS, origin=40.0)


def _case_9(hist, m):
    peak_h = max(int((h["state"][e] == HIJACKED).sum()) for h in hist for e in range(WIDE_E))
    peak_s = max(int(((h["state"][e] == HIJACKED) | (h["state"][e] == SHADOWED)).sum()) for h in hist for e in range(WIDE_E))
    assert peak_h >= 5 and peak_s > 5, (peak_h, peak_s)  # the hijack limit is reached
    refused = sum(int((h["zones"][..., 0, 0] & (h["state"] == SHADOWED) & (h["transitions"][..., 0] == T_NONE)).sum()) for h in hist)
    assert refused >= 6  # shadowed vehicles inside a full bubble ride on, not driven
    assert sum(int(h["ended"].sum()) for h in hist) >= 4  # releases: the count comes down and lets the next ones in
    turned_away = [(e, a) for e in range(WIDE_E) for a in range(WIDE_AGENTS) if any(h["mask"][e, a] == 0 and h["state"][e, a] == SOCIAL and
                   h["alive"][e, a] for h in hist)]
    assert len(turned_away) > 10


def case_wide():
    """Case 9: one fixed bubble 22 m long with hijack_limit = 5, shadow_limit = 9, 40 ticks.  Env 0 follows the column in
    slot order, env 1 in reverse, env 2 interleaved and from frame 10."""
    order = np.array(WIDE_IDS, dtype=np.int32)
    mixed = np.concatenate([order[::2], order[1::2]])
    follow = np.stack([order, order[::-1], mixed])[None]
    return Case("wide", lambda ln: [ln.on_line(13.3, 22.0, hijack_limit=5, shadow_limit=9)], follow.astype(np.int32),
                np.array([[0, 0, 10]], dtype=np.int32), 40, _case_9)

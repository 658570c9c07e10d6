"""Handing history agents over to actions inside a tick (include/smx.h smx_set_history_handover): the handover table and
the actions the tests use on tests/history_agents_ref.py's scene, and the rule restated in NumPy — who follows and who is
driven at every tick, the words each holds, status, expert action and done count — for
tests/test_gpu_history_handover.py to hold the device to.

Episode 0 (FOLLOW[0], STARTS[0]):
  case 1  env 0 / agent 0  DRIVER    H = 5     a driven lane beside a follower that leaves at its frame, in one wavefront
          env 0 / agent 1  LEAVER    H = -1    the follower that leaves
  case 2  env 1 / agent 1  STANDING  H = 0     driven from the first tick
  case 3  env 1 / agent 2  LATE      H = 3     absent at the reset: stays ABSENT and counted in the done count
  case 4  env 3 / agent 0  LEAVER    H = 10    driven before its last frame, 17: alive and DRIVEN at tick 30, never LEFT
  case 5  env 3 / agent 1  DRIVER    H = 1000  a follower throughout
  case 6  every slot that follows nothing      H = 7: ignored
Episode 1 uses another assignment, so that a run under auto_reset exercises the row switch: env 2's agent 0 and env 3's
agent 0 are driven in the first tick after their restart.
"""
import math

import numpy as np

import history_agents_ref as ref
import mpc_imitation_ref as imit
from smarts_amd import _native as nat

HANDOVER = np.array([[[5, -1, 7], [-1, 0, 3], [7, 7, 7], [10, 1000, 7]],
                     [[-1, 7, 4], [7, 0, 7], [0, -1, 3], [2, 7, 7]]], dtype=np.int32)
assert HANDOVER.shape == ref.FOLLOW.shape


def actions(tick, envs=ref.E, n=ref.N):
    """float32 [E, N, 3], a fixed function of (tick, env, agent): small accelerations and angular velocities; agent 0
    sends nothing (NaN, NaN) in the ticks 3, 10, 17, 24; agent 1 of env 1 at tick 12 and agent 0 of env 3 at tick 20 send
    the scalar form (a speed to set).  Social rows are NaN: nobody reads them."""
    a = np.full((envs, n, 3), np.nan, dtype=np.float32)
    a[..., 2] = 0.0
    for e in range(envs):
        for k in range(ref.AGENTS):
            a[e, k, 0] = 0.3 * math.sin(0.7 * tick + e + 2 * k)
            a[e, k, 1] = 0.05 * math.cos(0.4 * tick + 2 * e + k)
        if tick % 7 == 3:
            a[e, 0, :2] = np.nan
    if tick == 12 and envs > 1:
        a[1, 1, 0], a[1, 1, 1] = 2.0, np.nan
    if tick == 20 and envs > 3:
        a[3, 0, 0], a[3, 0, 1] = 4.5, np.nan
    return a


class Model(ref.Model):
    """history_agents_ref.Model with the handover rule: ``step(actions)`` is a tick of smx_step_history_handover.
    ``held`` [E, A, 4] are the words every alive agent holds (a follower's: its row); a driven agent's ``status`` is
    HA_DRIVEN, its ``row`` and ``action`` NaN.  The driven agents' words free-run in float64 unless the test writes the
    device's into ``held`` after a tick (``hold``), which makes the next tick's ``last_heading`` the device's own."""

    def __init__(self, table, starts, follow, handover, reset_elapsed_steps, envs=ref.E, agents=ref.AGENTS):
        super().__init__(table, starts, follow, reset_elapsed_steps, envs, agents)
        self.handover = np.asarray(handover)
        self.held = np.full((envs, agents, 4), np.nan)

    def reset_env(self, e):
        super().reset_env(e)
        self.held[e] = self.row[e]

    def H(self, e, a):
        return int(self.handover[self.table_row(e), e, a])

    def driven_next(self):
        """[E, A]: the agents the next tick drives."""
        out = np.zeros((self.E, self.A), dtype=bool)
        for e in range(self.E):
            for a in range(self.A):
                h = self.H(e, a)
                out[e, a] = self.alive[e, a] and h >= 0 and self.ticks[e] >= h
        return out

    def hold(self, words, which):
        """Take the device's words [E, A, 4] for the agents ``which`` (teacher forcing of the driven agents)."""
        self.held[which] = words[which]

    def step(self, acts, auto_reset=False):
        """One mixed tick.  Returns (left [E, A], env_done [E])."""
        left = np.zeros((self.E, self.A), dtype=bool)
        drive = self.driven_next()
        dt = self.table.dt
        for e in range(self.E):
            f = self.frame(e) + 1
            for a in range(self.A):
                if not self.alive[e, a]:
                    continue
                if drive[e, a]:
                    self.status[e, a] = nat.HA_DRIVEN
                    self.action[e, a] = np.nan
                    self.row[e, a] = np.nan
                    x, y, h, u = (float(v) for v in self.held[e, a])
                    out = imit.imitation_step(x, y, h, u, float(acts[e, a, 0]), float(acts[e, a, 1]), dt)
                    if out is not None:  # a control() call
                        self.last_heading[e, a] = h
                        self.last_dt[e, a] = dt
                        self.held[e, a] = out
                    continue
                v = self.followed(e, a)
                s = ref.find(self.table, f, v)
                if s < 0:
                    left[e, a] = True
                    self.alive[e, a] = False
                    self.status[e, a] = nat.HA_LEFT
                    self.action[e, a] = np.nan
                    self.done_count[e] += 1
                    continue
                self.status[e, a] = nat.HA_FOLLOWING
                self.last_heading[e, a] = self.held[e, a, 2]
                self.last_dt[e, a] = dt
                self.row[e, a] = self.held[e, a] = self.table.frames[f, s]
                self.action[e, a] = ref.expert_action(self.table, f, v)
            self.ticks[e] += 1
        env_done = self.done_count >= self.A
        if auto_reset:
            for e in np.nonzero(env_done)[0]:
                self.reset_env(e)
        return left, env_done


def grid_box(cm):
    """(x0, y0, x1, y1): the union of the map's two grids' extents — the box the state guard grows by its margin."""
    lx0, ly0 = float(cm.lpg_origin[0]), float(cm.lpg_origin[1])
    sx0, sy0 = float(cm.sg_origin[0]), float(cm.sg_origin[1])
    lx1, ly1 = lx0 + float(cm.lpg_cell) * int(cm.lpg_dims[0]), ly0 + float(cm.lpg_cell) * int(cm.lpg_dims[1])
    sx1, sy1 = sx0 + float(cm.sg_cell) * int(cm.sg_dims[0]), sy0 + float(cm.sg_cell) * int(cm.sg_dims[1])
    return min(lx0, sx0), min(ly0, sy0), max(lx1, sx1), max(ly1, sy1)


def driven_poses(table, starts, handover, res, ticks, follow=ref.FOLLOW, auto_reset=False):
    """Every pose [k, 4] a driven agent holds in a free run of ``ticks`` ticks of ``actions``."""
    m = Model(table, starts, follow, handover, res)
    m.reset()
    poses = []
    for t in range(ticks):
        drive = m.driven_next()
        m.step(actions(t), auto_reset=auto_reset)
        poses.append(m.held[drive & m.alive])
    return np.concatenate(poses) if poses else np.zeros((0, 4))


def assert_driven_in_bounds(cm, poses, margin=0.0):
    """Every driven pose is finite and inside the map's grids (no out-of-range cell index can be formed from it)."""
    x0, y0, x1, y1 = grid_box(cm)
    assert len(poses) > 0 and np.isfinite(poses).all()
    assert (poses[:, 0] >= x0 - margin).all() and (poses[:, 0] <= x1 + margin).all(), (poses[:, 0].min(), poses[:, 0].max(), x0, x1)
    assert (poses[:, 1] >= y0 - margin).all() and (poses[:, 1] <= y1 + margin).all(), (poses[:, 1].min(), poses[:, 1].max(), y0, y1)
    assert np.abs(poses[:, 3]).max() < 50.0

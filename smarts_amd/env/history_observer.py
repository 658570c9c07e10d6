"""Observe recorded vehicles' drives on the device: the reference's ``SMARTS.attach_sensors_to_vehicles`` +
``observe_from`` over a traffic history (``examples/observation_collection_for_imitation_learning.py``).

``HistoryObserver`` runs one env per recorded vehicle, each starting at that vehicle's first frame: agent slot 0 of env
``k`` follows ``vehicle_ids[k]`` (``BatchedSim.set_history_agents``), the further agent slots the other vehicles present
in that frame, and the social slots replay the rest of the history.  ``reset()`` / ``step()`` return, per env, the
``Observation`` of every followed vehicle under the reference's agent id ``Agent-history-vehicle-<id>``, built from the
interface's sensors like any agent's, and ``expert_actions()`` the Imitation action that takes each vehicle to its next
recorded frame: a behaviour-cloning dataset is the two side by side.

With ``handover`` the followers are handed over to actions one by one (``BatchedSim.set_history_handover``, the
reference's ``SMARTS.switch_control_to_agent``): a log-replay warm-up, then ``step(actions)`` drives the agents whose
handover tick has come while every other vehicle keeps replaying.

With ``bubbles`` the device decides that itself, tick by tick (``BatchedSim.set_history_bubbles``, the reference's
``BubbleManager.step``): a follower is shadowed in a bubble's airlock, driven inside, and released — it ends — once it is
outside again; a bubble may travel with an agent that is itself driven.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _native as nat
from ..lidar import base_rays
from ..traffic_history import HISTORY_VEHICLE_PREFIX, TrafficHistoryTable, read_sqlite, slots_needed
from .agent_interface import ActionSpaceType, AgentInterface
from .core import resolve_scenario, sim_config_from_interface
from .observations import Observation, ObservationBuilder

AGENT_PREFIX = "Agent-"  # smarts.py attach_sensors_to_vehicles: agent_id = f"Agent-{vehicle_id}"


class _FollowerNames(ObservationBuilder):
    """The builder with the followers named after their recorded vehicles (``rows["followed"]``: the id per agent slot)."""

    num_agents = 0
    _rows = None

    def actor_id(self, slot: int, rows=None) -> str:
        rows = self._rows if rows is None else rows
        if slot < self.num_agents and rows is not None and "followed" in rows:
            return f"{AGENT_PREFIX}{HISTORY_VEHICLE_PREFIX}{int(rows['followed'][slot])}"
        return super().actor_id(slot, rows)

    def vehicle_id(self, slot: int, rows=None) -> str:
        rows = self._rows if rows is None else rows
        if slot < self.num_agents and rows is not None and "followed" in rows:
            return f"{HISTORY_VEHICLE_PREFIX}{int(rows['followed'][slot])}"  # the vehicle keeps the provider's name
        return super().vehicle_id(slot, rows)

    def build(self, rows, slot, step_count, elapsed_sim_time, low_dimensional=False):
        self._rows = rows
        try:
            return super().build(rows, slot, step_count, elapsed_sim_time, low_dimensional)
        finally:
            self._rows = None


class HistoryObserver:
    """``scenario``: a scenario directory (as ``HiWayEnv`` takes it); ``table_or_path``: a ``TrafficHistoryTable`` or the
    path of a converted dataset (SQLite); ``agent_interface``: its sensors and done criteria are used, its ``action`` is
    ignored (the reference's collection example passes a Laner: nobody acts); ``vehicle_ids``: the recorded vehicles to
    observe, one env each (``None``: every vehicle of the table); ``num_envs``: at least ``len(vehicle_ids)`` (the
    default); ``num_agents``: agent slots per env — 1 observes the env's own vehicle alone, more also the other
    vehicles present in its first frame.  An env ends when every followed vehicle has left the recording (or ended by
    the interface's done criteria); nothing restarts.  ``handover`` (default ``None``: nobody is ever driven, every method
    behaves as without it): an int — the recorded ticks before every agent drives —, a mapping ``{vehicle id: ticks}``
    (vehicles it lacks are never driven), or a ready int32 table ``[1, E, A]`` (``TrafficHistoryTable.handover_ticks``
    makes one from zone entry frames: a bubble).  ``bubbles`` (default ``None``), alone or beside ``handover``: a sequence
    of ``smarts_amd.env.Bubble`` with ``PositionalZone`` zones, evaluated on the device at the start of every tick;
    ``follow_actor_id`` is an agent id of this observer (``agent_id``) and names the same agent slot in every env that has
    it.  ``bubble_states()`` reads what they decided.  (``bubbles`` stands before ``handover`` in the signature: pass both
    by keyword.)  ``dims`` (by keyword too; default ``False``: every vehicle has the sedan's box): the replayed vehicles at their own
    dimensions (``set_traffic_history(dims=True)``) and every follower at those of the vehicle it follows
    (``BatchedSim.set_agent_dims`` over ``table.agent_dims``), through a handover and a bubble alike — the boxes, events
    and lane ids beside every expert action are then the recorded vehicle's.  A followed vehicle longer than 10 m is refused
    (``SmxError``: the cap of ``set_agent_dims``); it can be replayed at its size, not followed at it."""

    bubbles = None

    def __init__(self, scenario: str, table_or_path, agent_interface: AgentInterface, vehicle_ids: Optional[Sequence[int]] = None,
                 num_envs: Optional[int] = None, dt: float = 0.1, num_agents: int = 1, device: str = "cuda:0",
                 waypoint_window: Optional[Tuple[int, int]] = (4, 20), seed: int = 0, bubbles=None, dims: bool = False,
                 handover=None):
        import torch

        from ..engine import BatchedSim, make_spawns
        from ..scenario_build import load_compiled_map

        table = table_or_path
        if not isinstance(table, TrafficHistoryTable):
            path = os.fspath(table_or_path)
            table = TrafficHistoryTable.from_sqlite(path, dt, max(1, slots_needed(*read_sqlite(path), dt)))
        if abs(table.dt - dt) > 1e-12:
            raise ValueError(f"the table was resampled at dt = {table.dt}, the observer runs at dt = {dt}")
        self.table = table
        self.vehicle_ids = table.vehicle_ids() if vehicle_ids is None else [int(v) for v in vehicle_ids]
        if not self.vehicle_ids:
            raise ValueError("no vehicle to observe")
        self.E = len(self.vehicle_ids) if num_envs is None else int(num_envs)
        self.A, self.S, self.dt = int(num_agents), table.num_slots, float(dt)
        itf = agent_interface.replace(action=ActionSpaceType.Lane)  # (ignored; the sim below is an Imitation sim)
        self.interface = itf
        self.scenario_dir = resolve_scenario(scenario)
        self.cm = load_compiled_map(self.scenario_dir)
        self.cfg = sim_config_from_interface(itf, self.E, self.A, dt, False, waypoint_window, self.S)
        self.cfg.action_space = "Imitation"
        start, vehicle = table.history_agent_windows(self.vehicle_ids, self.E, self.A, self.cfg.reset_elapsed_steps())
        spawns, where = make_spawns(self.cm, self.E, self.A + self.S, episodes=1, seed=seed, return_lanes=True)  # (never read)
        self.sim = BatchedSim(self.cm, self.cfg, device=device, spawns=spawns, seed=seed, social_spawns=where)
        self.start_frames, self.followed = start, vehicle
        self.dims = bool(dims)
        self.sim.set_traffic_history(table, torch.from_numpy(start).to(self.sim.device), dims=self.dims)
        self.sim.set_history_agents(torch.from_numpy(vehicle).to(self.sim.device))
        if self.dims:
            self.sim.set_agent_dims(table.agent_dims(vehicle))
        self.handover = None if handover is None else self._handover_table(handover)
        if self.handover is not None:
            self.sim.set_history_handover(torch.from_numpy(self.handover).to(self.sim.device))
        self.bubbles = None if bubbles is None else list(bubbles)
        if self.bubbles is not None:
            self.sim.set_history_bubbles([b.to_native(self._slot_of) for b in self.bubbles])
        road_ids = [self.cm.road_ids[r] for r in self.cm.lane_road]
        names = [f"follower-{a}" for a in range(self.A)] + [f"social-{k}" for k in range(self.S)]
        self.builder = _FollowerNames(
            self.cm.lane_ids, road_ids, names, waypoints=self.cfg.waypoints, neighbors=self.cfg.neighbors,
            accelerometer=self.cfg.accelerometer, ogm=itf.ogm or None, dagm=itf.drivable_area_grid_map or None,
            lidar_rays=base_rays(itf.lidar.sensor_params) if itf.lidar else None, dt=dt,
            road_waypoints=bool(itf.road_waypoints), history=table)
        self.builder.num_agents = self.A
        self._was_reset = False

    def agent_id(self, env: int, agent: int = 0) -> Optional[str]:
        """``Agent-history-vehicle-<id>`` of the vehicle agent slot ``agent`` of env ``env`` follows, ``None`` for none."""
        v = int(self.followed[0, env, agent])
        return f"{AGENT_PREFIX}{HISTORY_VEHICLE_PREFIX}{v}" if v >= 0 else None

    def _slot_of(self, agent_id: str) -> int:
        """The agent slot that carries ``agent_id`` (a bubble's ``follow_actor_id``): one slot, in every env that has it."""
        slots = {a for e in range(self.E) for a in range(self.A) if self.agent_id(e, a) == agent_id}
        if len(slots) != 1:
            raise ValueError(f"follow_actor_id {agent_id!r} names {'no agent' if not slots else 'different agent slots in different envs'}")
        return slots.pop()

    def bubble_states(self) -> List[Dict[str, int]]:
        """Per env ``{agent id: BUBBLE_SOCIAL | BUBBLE_SHADOWED | BUBBLE_HIJACKED | BUBBLE_RELEASED}`` (``bubbles`` only)."""
        if self.bubbles is None:
            return [{} for _ in range(self.E)]
        import torch

        torch.cuda.synchronize(self.sim.device)
        state = self.sim.out["bubble_state"].cpu().numpy()
        return [{self.agent_id(e, a): int(state[e, a]) for a in range(self.A) if self.followed[0, e, a] >= 0} for e in range(self.E)]

    def _handover_table(self, handover) -> np.ndarray:
        """int32 ``[1, E, A]`` from an int, a mapping vehicle id -> ticks, or a ready table."""
        if isinstance(handover, (int, np.integer)):
            return np.where(self.followed >= 0, int(handover), -1).astype(np.int32)
        if hasattr(handover, "keys"):
            table = np.full(self.followed.shape, -1, dtype=np.int32)
            for idx in np.ndindex(*self.followed.shape):
                v = int(self.followed[idx])
                if v >= 0 and v in handover:
                    table[idx] = int(handover[v])
            return table
        table = np.ascontiguousarray(handover, dtype=np.int32)
        if table.shape != self.followed.shape:
            raise ValueError(f"a handover table must have shape {self.followed.shape}, got {table.shape}")
        return table

    def driven(self) -> List[List[str]]:
        """Per env, the ids of the agents the last tick drove or whose handover tick has come: alive, and either the
        handover table drives them in the next ``step`` or a bubble holds them (its state row reads HIJACKED; the bubble
        pass of the next ``step`` may add to these, or release one)."""
        if self.handover is None and self.bubbles is None:
            return [[] for _ in range(self.E)]
        import torch

        torch.cuda.synchronize(self.sim.device)
        ticks = self.sim.env_ticks.cpu().numpy()
        alive = (self.sim.flags[:, :self.A].cpu().numpy() & nat.F_ALIVE) != 0
        by_table = np.zeros((self.E, self.A), dtype=bool)
        if self.handover is not None:
            by_table = (self.handover[0] >= 0) & (self.handover[0] <= ticks[:, None])
        held = np.zeros((self.E, self.A), dtype=bool)
        if self.bubbles is not None:
            held = self.sim.out["bubble_state"][:, :self.A].cpu().numpy() == nat.BUBBLE_HIJACKED
        return [[self.agent_id(e, a) for a in range(self.A)
                 if alive[e, a] and self.followed[0, e, a] >= 0 and (by_table[e, a] or held[e, a])] for e in range(self.E)]

    def _action_rows(self, actions) -> np.ndarray:
        """float32 ``(E, N, 3)`` in ``BatchedSim.step``'s Imitation layout from ``{agent id: (acceleration,
        angular_velocity) | speed}`` — one mapping for every env, or a sequence of one per env; a missing id = no action."""
        rows = np.full((self.E, self.A + self.S, 3), np.nan, dtype=np.float32)
        rows[..., 2] = 0.0
        if actions is None:
            return rows
        per_env = [actions] * self.E if hasattr(actions, "keys") else list(actions)
        if len(per_env) != self.E:
            raise ValueError(f"{len(per_env)} action mappings for {self.E} envs")
        for e, given in enumerate(per_env):
            for a in range(self.A):
                act = given.get(self.agent_id(e, a)) if given else None
                if act is None:
                    continue
                if np.ndim(act) == 0:
                    rows[e, a, 0] = float(act)  # the scalar form: a speed to set (the second word stays NaN)
                else:
                    rows[e, a, 0], rows[e, a, 1] = float(act[0]), float(act[1])
        return rows

    def reset(self):
        out = self.sim.reset()
        self._was_reset = True
        return self._collect(out)

    def step(self, actions=None):
        """One tick.  ``actions`` (only with ``handover`` or ``bubbles``): ``{agent id: (acceleration, angular_velocity) | speed}`` for
        the agents ``driven()`` names — one mapping for every env or a sequence of one per env; a missing id means no
        action, and what is given for a follower is ignored."""
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        if self.handover is None and self.bubbles is None:
            if actions is not None:
                raise ValueError("actions need a handover or bubbles: without either every agent follows its recorded vehicle")
            return self._collect(self.sim.step_history_agents())
        import torch

        return self._collect(self.sim.step_history_handover(torch.from_numpy(self._action_rows(actions)).to(self.sim.device)))

    def expert_actions(self) -> List[Dict[str, np.ndarray]]:
        """Per env ``{agent id: float32 (acceleration, angular_velocity)}`` of the followers still on the recording: the
        action that takes the vehicle from the frame just observed to the next (NaN, NaN where that frame lacks it, and
        for an agent the last tick drove: nobody labels a driven agent)."""
        import torch

        torch.cuda.synchronize(self.sim.device)
        act = self.sim.out["expert_action"].cpu().numpy()
        status = self.sim.out["history_agent_status"].cpu().numpy()
        return [{self.agent_id(e, a): act[e, a, :2].copy() for a in range(self.A)
                 if self.followed[0, e, a] >= 0 and status[e, a] in (nat.HA_FOLLOWING, nat.HA_SHADOWED, nat.HA_DRIVEN)} for e in range(self.E)]

    def _collect(self, out):
        import torch

        torch.cuda.synchronize(self.sim.device)
        rows = {k: v.cpu().numpy() for k, v in out.items() if k != "learner"}
        ticks = self.sim.env_ticks.cpu().numpy()
        observations: List[Dict[str, Observation]] = []
        rewards: List[Dict[str, float]] = []
        dones: List[Dict[str, bool]] = []
        for e in range(self.E):
            er = {k: v[e] for k, v in rows.items() if k != "env_done"}
            er["history_frame"] = int(self.start_frames[0, e]) + int(ticks[e])
            er["followed"] = self.followed[0, e]
            t = int(ticks[e])
            obs, rew, done = {}, {}, {}
            for a in range(self.A):
                name = self.agent_id(e, a)
                active, ended = bool(rows["active"][e, a]), bool(rows["done"][e, a])
                if name is None or not (active or ended):
                    continue
                # (a vehicle that left the recording this tick is done without an observation, agent_manager.py:153-157)
                # (... and so is one its bubble released)
                left = rows["history_agent_status"][e, a] in (nat.HA_LEFT, nat.HA_RELEASED)
                if not left:
                    obs[name] = self.builder.build(er, a, t, round(t * self.dt, 6))
                    rew[name] = float(rows["reward"][e, a])
                done[name] = ended
            done["__all__"] = bool(rows["env_done"][e])
            observations.append(obs)
            rewards.append(rew)
            dones.append(done)
        return observations, rewards, dones

    def close(self):
        self.sim.close()

"""Shared engine behind ``HiWayEnv`` and ``ParallelEnv``: E identical env instances x N agents on
one GPU (``BatchedSim``), with the reference's dict-of-agent-id surface on top.

Plays the role of ``SMARTS`` + ``AgentManager`` (reference ``smarts/core/smarts.py:187-227, 365-460``,
``agent_manager.py:161-240``) for the whole batch.
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _native as nat
from ..lidar import base_rays
from .agent import AgentSpec
from .agent_interface import ActionSpaceType, AgentInterface
from .observations import Observation, ObservationBuilder

# Controllers.perform_action, Lane space (controllers/__init__.py:125-144)
LANE_ACTIONS = {"keep_lane": 0, "slow_down": 1, "change_lane_left": 2, "change_lane_right": 3}
NO_ACTION = -1

PKG_SCENARIOS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenarios")


class SMARTSNotSetupError(Exception):
    """smarts.py:73-76: stepping before reset."""


class SMARTSDestroyedError(Exception):
    """smarts.py:79-82: use after destroy."""


def resolve_scenario(path: str) -> str:
    """A scenario directory holding ``map.net.xml`` (the reference's layout, scenario.py:109-121) or
    the compact ``map.smxnet.json.gz``; a bare reference-style name (``scenarios/loop``) falls back
    to the maps shipped with the package."""
    cands = [path]
    parts = os.path.normpath(path).split(os.sep)
    if "scenarios" in parts:
        tail = parts[parts.index("scenarios") + 1:]
        cands.append(os.path.join(PKG_SCENARIOS, *tail))
    cands.append(os.path.join(PKG_SCENARIOS, os.path.basename(os.path.normpath(path))))
    for c in cands:
        if os.path.isdir(c) and any(os.path.exists(os.path.join(c, f)) for f in ("map.net.xml", "map.smxnet.json.gz")):
            return c
    raise FileNotFoundError(f"scenario {path!r}: no map.net.xml / map.smxnet.json.gz found (looked in {cands})")


def encode_lane_action(action: Any) -> int:
    """Lane action string -> device code; anything else is an error, as in the reference
    (controllers/__init__.py:137-144 looks the string up in a dict)."""
    if isinstance(action, str):
        if action not in LANE_ACTIONS:
            raise KeyError(f"unknown Lane action {action!r}; expected one of {sorted(LANE_ACTIONS)}")
        return LANE_ACTIONS[action]
    raise TypeError(f"ActionSpaceType.Lane expects a string action, got {type(action).__name__}")


def encode_float_action(space: ActionSpaceType, action: Any):
    """Continuous / ActuatorDynamic: (throttle, brake, steering[-rate]); LaneWithContinuousSpeed:
    (target_speed, lane_change) (controllers/__init__.py:94-124) -> three float32."""
    vals = [float(x) for x in action]
    if space is ActionSpaceType.LaneWithContinuousSpeed:
        if len(vals) != 2:
            raise ValueError("LaneWithContinuousSpeed expects (target_speed, lane_change)")
        vals.append(0.0)
    elif len(vals) != 3:
        raise ValueError(f"{space.name} expects three floats")
    return vals


# the action spaces whose agents may share one env (BatchedSim.set_agent_spaces; MPC is on the device too, but
# AgentInterface.validate_for_device keeps it off the env layer)
MIXED_ENV_SPACES = (ActionSpaceType.Lane, ActionSpaceType.Continuous, ActionSpaceType.ActuatorDynamic,
                    ActionSpaceType.LaneWithContinuousSpeed, ActionSpaceType.Trajectory)


def encode_mixed_actions(agent_ids: Sequence[str], agent_specs: Dict[str, AgentSpec], spaces: Sequence[ActionSpaceType],
                         num_envs: int, slots: int, per_env_actions: Sequence[Dict[str, Any]]):
    """Per-env ``{agent_id: action}`` dicts of a mixed fleet -> the buffers of ``BatchedSim.step_mixed``: every agent's
    action goes through its own adapter and is encoded by its own space (``spaces[i]`` for ``agent_ids[i]``) into the
    buffer of that space's kind.  Returns ``(lane, floats, trajectories, counts)`` over ``(num_envs, slots)``; an agent
    without an action — absent from the dict, or adapted to ``None`` — keeps its space's "no action": code -1, NaN,
    count 0.  Host code only."""
    from ..engine import pack_trajectory

    lane = np.full((num_envs, slots), NO_ACTION, dtype=np.int8)
    floats = np.full((num_envs, slots, 3), np.nan, dtype=np.float32)
    packed = np.zeros((num_envs, slots, 4, nat.TRAJ_COLS), dtype=np.float64)
    counts = np.zeros((num_envs, slots), dtype=np.int32)
    for e, agent_actions in enumerate(per_env_actions):
        assert isinstance(agent_actions, dict) and all(isinstance(k, str) for k in agent_actions), \
            "Expected Dict[str, any]"  # hiway_env.py:232-234
        for agent_id, action in agent_actions.items():
            adapted = agent_specs[agent_id].action_adapter(action)
            i = agent_ids.index(agent_id)
            if adapted is None:
                continue
            space = spaces[i]
            if space is ActionSpaceType.Lane:
                lane[e, i] = encode_lane_action(adapted)
            elif space is ActionSpaceType.Trajectory or space is ActionSpaceType.MPC:
                packed[e, i], counts[e, i] = pack_trajectory(adapted)
            elif space in (ActionSpaceType.Continuous, ActionSpaceType.ActuatorDynamic, ActionSpaceType.LaneWithContinuousSpeed):
                floats[e, i] = encode_float_action(space, adapted)
            else:
                raise ValueError(f"{space} agents cannot be part of a mixed fleet")
    return lane, floats, packed, counts


# paths kept per agent when the caller asks for the reference's full ``waypoint_paths`` (one path per
# lane of the ego's road, plus junction branches; the shipped maps have at most 4 lanes per road)
FULL_WINDOW_PATHS = 8


def sim_config_from_interface(itf: AgentInterface, num_envs: int, num_agents: int, dt: float, auto_reset: bool,
                              waypoint_window: Optional[Tuple[int, int]] = (4, 20), num_social: int = 0,
                              agent_ids: Optional[Sequence[str]] = None):
    """AgentInterface -> SimConfig (one interface for every agent, as FormatObs also requires,
    format_obs.py:207-210).  ``waypoint_window`` = (paths, waypoints per path) kept in the dense
    rows; ``None`` keeps what the reference's ``Observation`` holds: every waypoint of a path
    (``lookahead + 1``) for up to ``FULL_WINDOW_PATHS`` paths."""
    from ..engine import SimConfig

    itf.validate_for_device()
    dc, evc = itf.done_criteria, itf.event_configuration
    kw: Dict[str, Any] = dict(
        num_envs=num_envs, num_vehicles=num_agents + num_social, num_social=num_social, dt=dt,
        waypoints=bool(itf.waypoints), wp_lookahead=itf.waypoints.lookahead if itf.waypoints else 32,
        neighbors=bool(itf.neighborhood_vehicles),
        nb_radius=itf.neighborhood_vehicles.radius if itf.neighborhood_vehicles else None,
        accelerometer=bool(itf.accelerometer), max_episode_steps=itf.max_episode_steps,
        done_collision=dc.collision, done_off_road=dc.off_road, done_off_route=dc.off_route,
        done_on_shoulder=dc.on_shoulder, done_wrong_way=dc.wrong_way, done_not_moving=dc.not_moving,
        not_moving_time=evc.not_moving_time, not_moving_distance=evc.not_moving_distance, auto_reset=auto_reset,
        action_space=itf.action.name if itf.action is not None else "Lane",  # None: every action is "no action"
    )
    alive = dc.agents_alive
    if alive is not None:
        kw.update(alive_min_ego=alive.minimum_ego_agents_alive, alive_min_total=alive.minimum_total_agents_alive)
        lists = []
        for lst in alive.agent_lists_alive or ():
            if agent_ids is None:
                raise ValueError("agents_alive lists need the agent ids")
            # ids that are not agents of this env are never alive (sensors.py:432-435)
            lists.append(([agent_ids.index(a) for a in lst.agents_list if a in agent_ids], lst.minimum_agents_alive_in_list))
        kw["alive_lists"] = tuple(lists)
    if itf.waypoints:
        # (4, 20) is the StdObs window (format_obs.py:42); rows are never longer than the lookahead
        if waypoint_window is None:
            waypoint_window = (FULL_WINDOW_PATHS, itf.waypoints.lookahead + 1)
        kw["wp_paths"] = waypoint_window[0]
        kw["wp_len"] = min(waypoint_window[1], itf.waypoints.lookahead + 1)
    if itf.ogm:
        kw.update(ogm=True, ogm_width=itf.ogm.width, ogm_height=itf.ogm.height, ogm_resolution=itf.ogm.resolution)
    if itf.drivable_area_grid_map:
        g = itf.drivable_area_grid_map
        kw.update(dagm=True, dagm_width=g.width, dagm_height=g.height, dagm_resolution=g.resolution)
    if itf.rgb:  # (validate_for_device refuses it today: DESIGN.md §9)
        kw.update(rgb=True, rgb_width=itf.rgb.width, rgb_height=itf.rgb.height, rgb_resolution=itf.rgb.resolution)
    if itf.lidar:
        kw.update(lidar=itf.lidar.sensor_params)
    if itf.road_waypoints:
        kw.update(road_waypoints=True, rw_horizon=itf.road_waypoints.horizon)
    return SimConfig(**kw)


class BatchCore:
    """E env instances of one scenario x the agents of ``agent_specs`` on one device."""

    def __init__(self, scenario_dir: str, agent_specs: Dict[str, AgentSpec], num_envs: int, dt: float, seed: int,
                 auto_reset: bool, device: str = "cuda:0", waypoint_window: Optional[Tuple[int, int]] = (4, 20),
                 num_social: int = 0, vias: Optional[Dict[str, Sequence]] = None, social_model: str = "constant",
                 missions: Optional[Dict[str, Any]] = None, spawns: str = "reference", shuffle_scenarios: bool = True,
                 ego_centric: bool = False, state_guard: bool = False,
                 state_guard_margin: float = nat.GUARD_MARGIN_DEFAULT, traffic_history=None, history_start_frames=None,
                 history_dims: bool = False, agent_dims: Optional[Dict[str, Sequence]] = None, mission_schedule=None):
        """``missions``: ``{agent id: mission}`` — or ``{agent id: [mission, ...]}``: the scenario's variations
        (scenario.py:206-227, 292-294).  All lists have one common length V, a single mission is repeated, and variation
        ``j`` gives every agent of an env its ``j``-th mission.  ``mission_schedule``: int ``(R, E)`` (or ``(R,)``) of
        variation numbers, episode ``k`` of env ``e`` runs ``schedule[k mod R, e]``; ``None``: every env cycles through
        the variations, rolled per env when ``shuffle_scenarios`` is set (``missions.mission_schedule``).  With a list
        anywhere the missions go to the device as a pool (``BatchedSim.set_mission_pool``): the agents' spawn rows,
        routes, goals and the ``mission`` of their observations are the variation's, also across an auto-reset.
        Variations of one agent that differ in ``start_time`` or ``entry_tactic`` are refused.  With no list nothing
        changes and no pool is bound.
        ``agent_dims``: ``{agent id: (length, width, height)}``, the agent's own vehicle dimensions
        (``BatchedSim.set_agent_dims``; the reference's ``Vehicle.agent_vehicle_dims``): a component that is ``None``, 0
        or -1 takes the passenger default (``Dimensions.copy_with_defaults``), agents it lacks stay sedans.  The agent's
        start is placed from the front bumper with its own length, its events, ``ego_vehicle_state.bounding_box`` and
        the box its env-mates see are its own.  ``ValueError`` for an action space that is not kinematic (TargetPose,
        TrajectoryWithTime, Imitation): the dynamic chassis is the sedan.
        ``traffic_history``: a ``smarts_amd.traffic_history.TrafficHistoryTable`` or the path of a converted dataset
        (SQLite): the ``num_social`` slots replay it (``BatchedSim.set_traffic_history``) and are named
        ``history-vehicle-<id>`` in the observations, the reference provider's prefix.  ``history_start_frames``: int
        ``[R, E]`` (or ``[E]``), the table frame at which episode ``k`` of env ``e`` starts (row ``k mod R``); ``None`` =
        every env replays from frame 0.  ``history_dims``: replay every vehicle at its own dimensions
        (``BatchedSim.set_traffic_history(dims=True)``): a neighbour's ``bounding_box`` is then the table's
        ``resolved_dimensions``; off, the sedan's box.
        ``state_guard`` / ``state_guard_margin``: ``SimConfig``'s (the state guard, include/smx.h smx_set_guard):
        ``info[agent]["guard"]`` then holds the agent's guard byte whenever it is non-zero.  One exception: the infos
        ``ParallelEnv.step`` returns for an env that restarted inside the launch (``auto_reset``) describe the finishing
        tick, whose bytes the new episode's have replaced already, so they carry no ``"guard"``.
        ``ego_centric``: the dense rows carry their ego-frame twins (``SimConfig(ego_centric=True)``) and the
        agents' Trajectory / TargetPose / TrajectoryWithTime actions are given in the frame of their last
        observation: ``step_actions`` converts them on the device (the reference's ``get_egocentric_adapters``)."""
        from ..engine import BatchedSim, checked_guard_margin, make_spawns
        from ..scenario_build import load_compiled_map

        self.agent_ids: List[str] = list(agent_specs.keys())
        self.agent_specs = agent_specs
        interfaces = [spec.interface for spec in agent_specs.values()]
        if any(i is None for i in interfaces):
            raise ValueError("every AgentSpec needs an interface")
        first = interfaces[0]
        # The agents may differ in their action space — a mixed fleet (BatchedSim.set_agent_spaces) — and in nothing else:
        # sensors and done criteria are the shared part's.
        if any(i.replace(action=first.action) != first for i in interfaces[1:]):
            raise NotImplementedError("all agents of an accelerated env must share one AgentInterface (only the action "
                                      "space may differ from agent to agent)")
        self.agent_spaces: List[Optional[ActionSpaceType]] = [i.action for i in interfaces]
        self.mixed = any(a is not first.action for a in self.agent_spaces[1:])
        if self.mixed:
            for agent_id, itf in zip(self.agent_ids, interfaces):
                itf.validate_for_device()
                if itf.action not in MIXED_ENV_SPACES:
                    raise NotImplementedError(f"agent {agent_id!r}: {itf.action} cannot share an env with other action spaces "
                                              f"(a mixed fleet takes {[a.name for a in MIXED_ENV_SPACES]})")
            if ego_centric:
                raise NotImplementedError("ego_centric=True with differing action spaces: ego-frame actions of a mixed fleet "
                                          "are not built")
        self.interface: AgentInterface = first
        self.E, self.N, self.dt, self.seed = num_envs, len(self.agent_ids), dt, seed
        self.scenario_dir = resolve_scenario(scenario_dir)
        self.cm = load_compiled_map(self.scenario_dir)  # compiled-map cache next to the map (scenario build)
        self.cfg = sim_config_from_interface(first, num_envs, self.N, dt, auto_reset, waypoint_window, num_social,
                                             self.agent_ids)
        self.num_social = num_social
        self.cfg.social_model = social_model
        self.ego_centric = self.cfg.ego_centric = bool(ego_centric)
        self.cfg.state_guard, self.cfg.state_guard_margin = bool(state_guard), checked_guard_margin(state_guard_margin)
        # Start poses.  "reference": what hiway-v0 gives agents of a scenario without missions.pkl — a random endless
        # mission each, from CPython's random stream (missions.reference_spawn_table); "synthetic": the benchmark's
        # spawn table (PCG64(seed + env), 8 m apart on a lane, at the speed limit).  Scripted social
        # vehicles (the stand-in for the scenario's SUMO flows) always start from the synthetic table.
        if spawns not in ("reference", "synthetic"):
            raise ValueError('spawns must be "reference" or "synthetic"')
        spawn_mode = spawns
        # the agents' own dimensions (resolved here: the start poses below are placed with the agent's own length)
        self.agent_dims = None
        own_length: List[Optional[float]] = [None] * self.N
        if agent_dims:
            from ..traffic_history import resolve_dimensions

            unknown = set(agent_dims) - set(self.agent_ids)
            if unknown:
                raise ValueError(f"agent_dims for unknown agents: {sorted(unknown)}")
            if self.cfg.action_space not in ("TargetPose", "TrajectoryWithTime", "Imitation"):
                raise ValueError(f"agent_dims needs a kinematic action space (TargetPose, TrajectoryWithTime, Imitation): "
                                 f"an agent of ActionSpaceType.{self.cfg.action_space} drives the sedan its dynamics model describes")
            self.agent_dims = {a: resolve_dimensions(2, *agent_dims[a]) for a in agent_dims}  # 2: passenger
            own_length = [self.agent_dims[a][0] if a in self.agent_dims else None for a in self.agent_ids]
        # mission variations (missions.mission_variations): the schedule first — spawn row (episode mod S) must be the
        # start of the mission of table row (episode mod R), so the spawn table gets a multiple of R rows
        self.mission_variations = self.mission_schedule = None
        if missions and any(isinstance(m, (list, tuple)) for m in missions.values()):
            from ..missions import _entry_of, mission_schedule as default_schedule, mission_variations

            self.mission_variations = mission_variations(missions, self.agent_ids)
            self.mission_schedule = default_schedule(len(self.mission_variations), num_envs, seed, shuffle_scenarios, mission_schedule)
            for i, a in enumerate(self.agent_ids):
                if len({_entry_of(v[i]) for v in self.mission_variations}) > 1:
                    raise NotImplementedError(f"agent {a!r}: its mission variations differ in start_time / entry_tactic; the "
                                              "delayed-entry table is built for one entry per agent")
        elif mission_schedule is not None:
            raise ValueError("mission_schedule needs missions with a list of variations")
        spawn_rows = 4
        if self.mission_schedule is not None:
            R = self.mission_schedule.shape[0]
            spawn_rows = R * -(-4 // R)
        spawns, where = make_spawns(self.cm, num_envs, self.N + num_social, episodes=spawn_rows, seed=seed, return_lanes=True)
        if spawn_mode == "reference":
            from ..missions import reference_spawn_table
            from ..sumo_map import load_net

            ref = reference_spawn_table(load_net(self.scenario_dir), num_envs, self.N, seed, episodes=spawns.shape[0],
                                        shuffle_scenarios=shuffle_scenarios, lengths=own_length if self.agent_dims else None)
            slots = self.N + num_social
            spawns.reshape(spawns.shape[0], num_envs, slots, 4)[:, :, :self.N] = ref.reshape(spawns.shape[0], num_envs, self.N, 4)
        # mission vias (sstudio Via per agent id) -> resolved lists per vehicle slot
        self.vias = None
        if vias:
            from ..vias import resolve_vias

            unknown = set(vias) - set(self.agent_ids)
            if unknown:
                raise ValueError(f"vias for unknown agents: {sorted(unknown)}")
            self.vias = [resolve_vias(self.cm, vias.get(a, ())) for a in self.agent_ids] + [[] for _ in range(num_social)]
            self.cfg.via_max = 8
        # missions (sstudio Mission / EndlessMission / LapMission, or TraverseMission, per agent id): planned once
        # (Scenario._extract_mission + Plan.create_route), the agent's spawn rows become the mission's start in every
        # env and episode — for every kind, the ones with an empty route included
        self.missions = None
        self.planned_variations = None
        if self.mission_variations is not None:
            from ..missions import plan_mission
            from ..sumo_map import load_net

            net = load_net(self.scenario_dir)
            self.planned_variations = [[plan_mission(net, m) if m is not None else None for m in v] for v in self.mission_variations]
            from ..missions import mission_spawn_poses

            slots = self.N + num_social
            poses = mission_spawn_poses(self.planned_variations, self.mission_schedule, spawns.shape[0], own_length)
            table = spawns.reshape(spawns.shape[0], num_envs, slots, 4)[:, :, :self.N]
            given = ~np.isnan(poses[..., 0])
            table[given, :3], table[given, 3] = poses[given], 0.0
        elif missions:
            from ..missions import plan_mission
            from ..sumo_map import load_net

            unknown = set(missions) - set(self.agent_ids)
            if unknown:
                raise ValueError(f"missions for unknown agents: {sorted(unknown)}")
            net = load_net(self.scenario_dir)
            self.missions = [plan_mission(net, missions[a]) if a in missions else None for a in self.agent_ids]
            self.missions += [None] * num_social
            slots = self.N + num_social
            for i, m in enumerate(self.missions):
                if m is not None:
                    own = own_length[i] if i < self.N else None
                    x, y, h = m.spawn_pose() if own is None else m.spawn_pose(own)
                    spawns.reshape(spawns.shape[0], num_envs, slots, 4)[:, :, i] = (x, y, h, 0.0)
        # delayed entry (Mission.start_time / entry_tactic, smarts_amd.missions.entry_table): bound only when the agents'
        # fire steps differ; then the reset observation is the earliest agent's and the others enter inside a tick
        self.entry = None
        if self.mission_variations is not None:
            # one entry per agent (checked above), the start point it keeps clear per row: the variation's
            from ..missions import EntryTable, entry_table

            dims_rows = None
            if self.agent_dims:
                dims_rows = np.full((1, num_envs, self.N, 3), np.nan, dtype=np.float64)
                for i, a in enumerate(self.agent_ids):
                    if a in self.agent_dims:
                        dims_rows[0, :, i] = self.agent_dims[a]
            per = [entry_table(v, p, num_envs, dt, dims_rows) for v, p in zip(self.mission_variations, self.planned_variations)]
            if per[0].differs:
                sched = self.mission_schedule
                ready = np.repeat(per[0].ready, sched.shape[0], axis=0)
                check = np.stack([np.stack([per[sched[k, e]].check[0, e] for e in range(num_envs)]) for k in range(sched.shape[0])])
                self.entry = EntryTable(np.ascontiguousarray(ready), np.ascontiguousarray(check), per[0].reset_steps, per[0].steps,
                                        per[0].entry_speed)
                self.cfg.entry_reset_steps = per[0].reset_steps
                slots = self.N + num_social
                for i, speed in enumerate(per[0].entry_speed):
                    if speed is not None:
                        spawns.reshape(spawns.shape[0], num_envs, slots, 4)[:, :, i, 3] = speed
        elif missions:
            from ..missions import entry_table

            dims_rows = None
            if self.agent_dims:
                dims_rows = np.full((1, num_envs, self.N, 3), np.nan, dtype=np.float64)
                for i, a in enumerate(self.agent_ids):
                    if a in self.agent_dims:
                        dims_rows[0, :, i] = self.agent_dims[a]
            table = entry_table([missions.get(a) for a in self.agent_ids], self.missions[:self.N], num_envs, dt, dims_rows)
            if table.differs:
                self.entry = table
                self.cfg.entry_reset_steps = table.reset_steps
                slots = self.N + num_social
                for i, speed in enumerate(table.entry_speed):
                    if speed is not None:  # TrapEntryTactic.default_entry_speed: the new vehicle's speed
                        spawns.reshape(spawns.shape[0], num_envs, slots, 4)[:, :, i, 3] = speed
        pooled = self.planned_variations is not None
        self.sim = BatchedSim(self.cm, self.cfg, device=device, spawns=spawns, seed=seed, social_spawns=where,
                              vias=None if pooled else self.vias, missions=self.missions)
        if pooled:
            import torch

            from ..missions import mission_pool_rows

            # the pool variation by variation: entry j * N + a is agent a's mission in variation j, with the agent's vias
            pool = [m for v in self.planned_variations for m in v]
            pool_vias = [list(self.vias[i]) for _ in self.planned_variations for i in range(self.N)] if self.vias else None
            rows = mission_pool_rows(self.planned_variations, self.mission_schedule,
                                     [bool(self.vias[i]) for i in range(self.N)] if self.vias else None)
            self.sim.set_mission_pool(pool, pool_vias, torch.from_numpy(rows).to(self.sim.device))
        if self.agent_dims:
            table = np.full((1, num_envs, self.N, 3), np.nan, dtype=np.float64)
            for i, a in enumerate(self.agent_ids):
                if a in self.agent_dims:
                    table[0, :, i] = self.agent_dims[a]
            self.sim.set_agent_dims(table)
        if self.mixed:
            self.sim.set_agent_spaces([a.name for a in self.agent_spaces])
        if self.entry is not None:  # (the agent slots: the table's A is this core's N)
            self.sim.set_agent_entry(self.entry.ready, self.entry.check)
        self.traffic_history = None
        if traffic_history is not None:
            import torch

            from ..traffic_history import TrafficHistoryTable

            if num_social < 1:
                raise ValueError("traffic_history needs num_social >= 1 (the slots that replay it)")
            table = traffic_history
            if not isinstance(table, TrafficHistoryTable):
                table = TrafficHistoryTable.from_sqlite(os.fspath(traffic_history), dt, num_social)
            start = np.zeros((1, num_envs), dtype=np.int32) if history_start_frames is None else \
                np.atleast_2d(np.asarray(history_start_frames)).astype(np.int32)
            if start.shape[1:] != (num_envs,):
                raise ValueError(f"history_start_frames must have shape [R, {num_envs}] or [{num_envs}]")
            self.sim.set_traffic_history(table, torch.from_numpy(np.ascontiguousarray(start)).to(self.sim.device))
            if history_dims:
                self.sim.set_history_dims(True)
            self.traffic_history = table
        elif history_start_frames is not None:
            raise ValueError("history_start_frames needs traffic_history")
        elif history_dims:
            raise ValueError("history_dims needs traffic_history")
        road_ids = [self.cm.road_ids[r] for r in self.cm.lane_road]
        vehicle_names = self.agent_ids + [f"social-{k}" for k in range(num_social)]
        self.builder = ObservationBuilder(
            self.cm.lane_ids, road_ids, vehicle_names, waypoints=self.cfg.waypoints, neighbors=self.cfg.neighbors,
            accelerometer=self.cfg.accelerometer, ogm=first.ogm or None, dagm=first.drivable_area_grid_map or None,
            lidar_rays=base_rays(first.lidar.sensor_params) if first.lidar else None, dt=dt, vias=self.vias,
            road_waypoints=bool(first.road_waypoints), missions=self.missions, rgb=first.rgb or None,
            history=self.traffic_history)
        # one name table per variation: the `mission` of an observation is the one its env flies in that episode
        self.builders = None
        if pooled:
            self.builders = [ObservationBuilder(
                self.cm.lane_ids, road_ids, vehicle_names, waypoints=self.cfg.waypoints, neighbors=self.cfg.neighbors,
                accelerometer=self.cfg.accelerometer, ogm=first.ogm or None, dagm=first.drivable_area_grid_map or None,
                lidar_rays=self.builder.lidar_rays, dt=dt, vias=self.vias, road_waypoints=bool(first.road_waypoints),
                missions=list(v) + [None] * num_social, rgb=first.rgb or None, history=self.traffic_history)
                for v in self.planned_variations]
        self._was_reset = False
        self._destroyed = False

    @property
    def step_count(self) -> np.ndarray:
        """Ticks since each env's last reset, read from the device (``smx_state.env_ticks``): the one clock
        of the batch, also across ``reset_dense(env_mask)`` and the in-launch auto-reset."""
        return self.sim.env_ticks.cpu().numpy().astype(np.int64)

    # ------------------------------------------------------------------ dense (fast) path
    def reset_dense(self, env_mask=None):
        self._check_alive()
        out = self.sim.reset(env_mask)
        self._was_reset = True
        return out

    def step_dense(self, actions):
        """``actions``: int8 tensor [E, N] of lane-action codes (NO_ACTION = -1)."""
        self._check_alive()
        if not self._was_reset:
            raise SMARTSNotSetupError("Must call reset() or setup() before stepping.")
        return self.sim.step(actions)

    # ------------------------------------------------------------------ object path
    def step_actions(self, per_env_actions: Sequence[Dict[str, Any]]):
        """Per-env ``{agent_id: action}`` dicts -> one device tick (the reference's
        ``SMARTS.step(agent_actions)``); returns the dict of output tensors."""
        import torch

        from ..engine import pack_trajectory

        if self.mixed:
            lane, floats, packed, counts = self.encode_mixed_actions(per_env_actions)
            self._check_alive()
            if not self._was_reset:
                raise SMARTSNotSetupError("Must call reset() or setup() before stepping.")
            return self.sim.step_mixed(torch.from_numpy(lane), torch.from_numpy(floats), torch.from_numpy(packed),
                                       torch.from_numpy(counts))
        space = self.interface.action
        if space is ActionSpaceType.TargetPose or space is ActionSpaceType.TrajectoryWithTime:
            return self._step_kinematic(per_env_actions)
        if space is not ActionSpaceType.Trajectory:
            acts = self.encode_actions(per_env_actions)
            return self.step_dense(torch.from_numpy(acts).to(self.sim.device))
        # ActionSpaceType.Trajectory: (xs, ys, headings, speeds) per agent (controllers/__init__.py:104-110)
        slots = self.N + self.num_social
        packed = np.zeros((self.E, slots, 4, nat.TRAJ_COLS), dtype=np.float64)
        counts = np.zeros((self.E, slots), dtype=np.int32)
        for e, agent_actions in enumerate(per_env_actions):
            assert isinstance(agent_actions, dict) and all(isinstance(k, str) for k in agent_actions), \
                "Expected Dict[str, any]"  # hiway_env.py:232-234
            for agent_id, action in agent_actions.items():
                adapted = self.agent_specs[agent_id].action_adapter(action)
                i = self.agent_ids.index(agent_id)
                if adapted is None:
                    continue  # count 0 = no action
                packed[e, i], counts[e, i] = pack_trajectory(adapted)
        self._check_alive()
        if not self._was_reset:
            raise SMARTSNotSetupError("Must call reset() or setup() before stepping.")
        return self.sim.step_trajectory(torch.from_numpy(packed), torch.from_numpy(counts), ego_centric=self.ego_centric)

    def _step_kinematic(self, per_env_actions: Sequence[Dict[str, Any]]):
        """TargetPose: ``[x, y, heading, seconds into the future]`` per agent (motion_planner_provider.py:65-78);
        TrajectoryWithTime: a ``5 x T`` array of rows time, x, y, heading, speed
        (trajectory_interpolation_provider.py:31-38).  ``None`` = no action this tick."""
        import torch

        slots = self.N + self.num_social
        adapted: Dict[Tuple[int, int], np.ndarray] = {}
        for e, agent_actions in enumerate(per_env_actions):
            assert isinstance(agent_actions, dict) and all(isinstance(k, str) for k in agent_actions), \
                "Expected Dict[str, any]"  # hiway_env.py:232-234
            for agent_id, action in agent_actions.items():
                a = self.agent_specs[agent_id].action_adapter(action)
                if a is not None:
                    adapted[e, self.agent_ids.index(agent_id)] = np.asarray(a, dtype=np.float64)
        self._check_alive()
        if not self._was_reset:
            raise SMARTSNotSetupError("Must call reset() or setup() before stepping.")
        if self.interface.action is ActionSpaceType.TargetPose:
            targets = np.full((self.E, slots, 4), np.nan, dtype=np.float64)  # NaN x = no action
            for (e, i), a in adapted.items():
                if a.shape != (4,):
                    raise ValueError(f"TargetPose expects [x, y, heading, seconds_into_future], got shape {a.shape}")
                targets[e, i] = a
            return self.sim.step_target_pose(torch.from_numpy(targets), ego_centric=self.ego_centric)
        for a in adapted.values():
            if a.ndim != 2 or a.shape[0] != 5:
                raise ValueError(f"TrajectoryWithTime expects a 5 x T array (time, x, y, heading, speed), got shape {a.shape}")
        # (a trajectory of one point is handed on as it is: the device refuses it as the reference does, at the next sync)
        width = max([2] + [a.shape[1] for a in adapted.values()])
        trajs = np.zeros((self.E, slots, 5, width), dtype=np.float64)
        counts = np.zeros((self.E, slots), dtype=np.int32)  # 0 = no action
        for (e, i), a in adapted.items():
            trajs[e, i, :, :a.shape[1]], counts[e, i] = a, a.shape[1]
        return self.sim.step_trajectory_with_time(torch.from_numpy(trajs), torch.from_numpy(counts), ego_centric=self.ego_centric)

    def encode_mixed_actions(self, per_env_actions: Sequence[Dict[str, Any]]):
        """The buffers of ``BatchedSim.step_mixed`` for a mixed fleet's actions (``encode_mixed_actions`` above)."""
        return encode_mixed_actions(self.agent_ids, self.agent_specs, self.agent_spaces, self.E, self.N + self.num_social,
                                    per_env_actions)

    def encode_actions(self, per_env_actions: Sequence[Dict[str, Any]]) -> np.ndarray:
        space = self.interface.action
        lane = space is ActionSpaceType.Lane or space is None
        slots = self.N + self.num_social
        if lane:
            acts = np.full((self.E, slots), NO_ACTION, dtype=np.int8)
        else:
            acts = np.full((self.E, slots, 3), np.nan, dtype=np.float32)  # NaN = no action
        for e, agent_actions in enumerate(per_env_actions):
            assert isinstance(agent_actions, dict) and all(isinstance(k, str) for k in agent_actions), \
                "Expected Dict[str, any]"  # hiway_env.py:232-234
            for agent_id, action in agent_actions.items():
                adapted = self.agent_specs[agent_id].action_adapter(action)
                i = self.agent_ids.index(agent_id)
                if adapted is None:
                    continue  # controllers/__init__.py:90-91: no action, no control call this tick
                if space is None:
                    raise ValueError("perform_action(action_space=None, ...) has failed: the interface has no action space")
                if lane:
                    acts[e, i] = encode_lane_action(adapted)
                else:
                    acts[e, i] = encode_float_action(space, adapted)
        return acts

    def host_rows(self, out) -> Dict[str, np.ndarray]:
        import torch

        torch.cuda.synchronize(self.sim.device)
        # the learner block is [2, E, N] (reward / done axis first) and exists for the device-side gather only
        rows = {k: v.cpu().numpy() for k, v in out.items() if k != "learner"}
        rows["env_ticks"] = self.sim.env_ticks.cpu().numpy()
        if self.traffic_history is not None:
            # the table frame every env's observation shows (include/smx.h smx_set_social_history): names the neighbours
            start = self.sim.history_start_frames.cpu().numpy().astype(np.int64)
            episode = self.sim.env_episode.cpu().numpy().astype(np.int64)
            rows["history_frame"] = start[episode % start.shape[0], np.arange(self.E)] + rows["env_ticks"]
        if self.builders is not None:
            # the variation every env flies now, and the one of the episode before (the finishing tick of a restart)
            episode = self.sim.env_episode.cpu().numpy().astype(np.int64)
            sched, envs = self.mission_schedule, np.arange(self.E)
            rows["mission_variation"] = sched[episode % sched.shape[0], envs]
            rows["mission_variation_before"] = sched[(episode - 1) % sched.shape[0], envs]
        return rows

    PER_ENV_ROWS = ("env_done", "env_ticks", "history_frame", "mission_variation", "mission_variation_before")  # [E]; every other row is [E, N, ...]

    def _builder(self, rows, env: int, before: bool = False):
        if self.builders is None:
            return self.builder
        return self.builders[int(rows["mission_variation_before" if before else "mission_variation"][env])]

    def observations(self, rows: Dict[str, np.ndarray], env: int, present: np.ndarray) -> Dict[str, Observation]:
        er = {k: v[env] for k, v in rows.items() if k not in self.PER_ENV_ROWS}
        if "history_frame" in rows:
            er["history_frame"] = int(rows["history_frame"][env])
        t = int(rows["env_ticks"][env])  # device clock: already that of the new episode after an auto-reset
        elapsed = round(t * self.dt, 6)
        builder = self._builder(rows, env)
        return {self.agent_ids[i]: builder.build(er, i, t, elapsed) for i in range(self.N) if present[i]}

    def final_observations(self, rows: Dict[str, np.ndarray], env: int, present: np.ndarray, step_count: int) -> Dict[str, Observation]:
        """The finishing tick's observation of the agents of an env that restarted inside the launch
        (``smx_outputs.final_*``: ego block, events, distance travelled — the low-dimensional part; the sensor rows of
        that tick are gone): what the reference hands back as ``info[agent]["env_obs"]`` (parallel_env.py:303-309)."""
        er = {k: v[env] for k, v in rows.items() if k not in self.PER_ENV_ROWS}
        for k in ("ego_pos", "ego_f32", "ego_lane", "events", "dist"):
            er[k] = rows["final_" + k][env]
        elapsed = round(step_count * self.dt, 6)
        builder = self._builder(rows, env, before=True)
        return {self.agent_ids[i]: builder.build(er, i, step_count, elapsed, low_dimensional=True)
                for i in range(self.N) if present[i]}

    def close(self):
        if not self._destroyed:
            self.sim.close()
            self._destroyed = True

    def _check_alive(self):
        if self._destroyed:
            raise SMARTSDestroyedError("BUG: SMARTS was destroyed and is no longer usable")

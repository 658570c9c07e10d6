"""Batched simulation engine: E environment instances x N vehicle slots on one GPU.

Host-side owner of the device buffers (PyTorch-ROCm tensors, used purely as the
zero-copy buffer type) and thin caller of the C-ABI (include/smx.h).  It plays the
role of ``SMARTS`` (reference ``smarts/core/smarts.py``) for a whole shard:
``reset`` ~ ``SMARTS.reset`` (:365-460), ``step`` ~ ``SMARTS.step`` (:187-227).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as nat
from .lidar import SensorParams, base_rays, ray_count
from .map_compiler import CompiledMap


def checked_guard_margin(margin):
    """``margin`` if it is a valid state-guard margin (include/smx.h smx_set_guard: a finite number of metres,
    0 <= margin <= SMX_GUARD_MARGIN_MAX), else ValueError.  SimConfig and the env layer validate with this."""
    m = margin
    if isinstance(m, bool) or not isinstance(m, (int, float)) or not math.isfinite(m) or not 0.0 <= m <= nat.GUARD_MARGIN_MAX:
        raise ValueError(f"state_guard_margin must be a finite number of metres in [0, {nat.GUARD_MARGIN_MAX:g}], got {m!r}")
    return m


@dataclass
class SimConfig:
    """Mirror of ``smx_config``; defaults follow the reference's AgentInterface / HiWayEnv."""

    num_envs: int = 1
    num_vehicles: int = 1
    dt: float = 0.1  # hiway_env.py:113
    waypoints: bool = True
    neighbors: bool = False
    accelerometer: bool = True  # agent_interface.py:291
    wp_lookahead: int = 32  # agent_interface.py:78
    wp_paths: int = 4  # format_obs.py:42
    wp_len: int = 20
    nb_max: int = 10  # format_obs.py:41
    nb_radius: Optional[float] = None  # agent_interface.py:98
    max_episode_steps: Optional[int] = None
    done_collision: bool = True  # agent_interface.py:186-206
    done_off_road: bool = True
    done_off_route: bool = True
    done_on_shoulder: bool = False
    done_wrong_way: bool = False
    done_not_moving: bool = False
    not_moving_time: float = 60.0
    not_moving_distance: float = 1.0
    auto_reset: bool = False  # parallel_env.py:62
    track_driven_path: bool = True
    ogm: bool = False  # agent_interface.py:42-51 (OGM defaults 256 x 256 @ 50/256)
    ogm_width: int = 256
    ogm_height: int = 256
    ogm_resolution: float = 50 / 256
    dagm: bool = False  # agent_interface.py:29-38 (DrivableAreaGridMap defaults 256 x 256 @ 50/256)
    dagm_width: int = 256
    dagm_height: int = 256
    dagm_resolution: float = 50 / 256
    lidar: Optional[SensorParams] = None  # agent_interface.py:132-135
    # the top-down RGB camera (agent_interface.py:54-64, RGB defaults 256 x 256 @ 50/256): out["rgb"], [E, N, H, W, 3]
    # uint8 (include/smx.h SMX_SENSOR_RGB); the sim owns the image buffer and binds it with smx_set_rgb_output
    rgb: bool = False
    rgb_width: int = 256
    rgb_height: int = 256
    rgb_resolution: float = 50 / 256
    # DoneCriteria.agents_alive (agent_interface.py:155-176): minima (None = unset) and up to four
    # (agent slots, minimum alive) lists
    alive_min_ego: Optional[int] = None
    alive_min_total: Optional[int] = None
    alive_lists: Sequence = ()
    via_max: int = 0  # near-via rows per agent (the via sensor runs when BatchedSim gets vias)
    num_social: int = 0  # scripted social vehicles: the last num_social slots of every env (include/smx.h)
    social_speed_factor: float = 0.8
    social_model: str = "constant"  # "constant" | "idm" (include/smx.h SMX_SOCIAL_*)
    # ActionSpaceType name: Lane | Continuous | ActuatorDynamic | LaneWithContinuousSpeed | Trajectory | TargetPose |
    # TrajectoryWithTime | MPC | Imitation (TargetPose, TrajectoryWithTime and Imitation: kinematic agents, placed by a
    # provider or by the Imitation controller instead of driven through a control law and the dynamics model)
    action_space: str = "Lane"
    launch_strategy: str = "auto"  # "auto" | "small" | "large": how a tick is cut into launches (include/smx.h)
    # RoadWaypoints (agent_interface.py RoadWaypoints.horizon = 32; sensors.py:991-1040): dense rows keep the first
    # rw_lanes lanes and the first rw_paths paths of each, 2 x horizon + 1 waypoints per path
    road_waypoints: bool = False
    rw_horizon: int = 32
    rw_lanes: int = 8
    rw_paths: int = 4
    # lane_ttc (custom_observations.py:148-280) of every agent on the device: out["lane_ttc"], out["lane_ttc_flags"]
    # (include/smx.h SMX_SENSOR_LANE_TTC); needs waypoints and neighbors
    lane_ttc: bool = False
    # the ego-centric adapters (smarts/core/utils/adapters/ego_centric_adapters.py) on the device: out["ego_frame"],
    # out["ec_flags"], out["ec_ego_f32"] and an out["ec_*"] twin of every position / heading row whose sensor is on
    # (include/smx.h SMX_SENSOR_EGO_CENTRIC); actions_to_world turns ego-frame actions back
    ego_centric: bool = False
    # FrameStack (smarts/env/wrappers/frame_stack.py) on the device: 0 = off, 2..8 = frames kept, newest first, of every
    # row named in frame_stack_rows — out["stack_<row>"], [E, N, k, ...row shape]; frame_stack_rgb_dstack adds
    # out["rgb_dstack"], [E, N, H, W, 3k]: the array RGBImage returns (include/smx.h smx_bind_frame_stack)
    frame_stack: int = 0
    frame_stack_rows: Sequence[str] = ()
    frame_stack_rgb_dstack: bool = False
    # the state guard (include/smx.h smx_set_guard), off by default: an agent whose state or spawn row is not finite or
    # lies more than state_guard_margin metres outside the map's grids ends (done = 1) instead of reaching a map search;
    # out["guard"], [E, N] uint8, holds the reason (nat.GUARD_STEP / GUARD_STATE / GUARD_SPAWN)
    state_guard: bool = False
    state_guard_margin: float = nat.GUARD_MARGIN_DEFAULT
    # delayed agent entry (smarts_amd.missions.entry_table): the steps reset() burns before the first agent enters,
    # min over the agents of missions.entry_ticks; None = the 0.1 s default start time of every mission
    entry_reset_steps: Optional[int] = None

    def __post_init__(self):
        checked_guard_margin(self.state_guard_margin)

    def sensors_mask(self) -> int:
        m = 0
        if self.waypoints:
            m |= nat.SENSOR_WAYPOINTS
        if self.neighbors:
            m |= nat.SENSOR_NEIGHBORS
        if self.accelerometer:
            m |= nat.SENSOR_ACCELEROMETER
        if self.ogm:
            m |= nat.SENSOR_OGM
        if self.lidar is not None:
            m |= nat.SENSOR_LIDAR
        if self.dagm:
            m |= nat.SENSOR_DAGM
        if self.road_waypoints:
            m |= nat.SENSOR_ROAD_WAYPOINTS
        if self.lane_ttc:
            m |= nat.SENSOR_LANE_TTC
        if self.ego_centric:
            m |= nat.SENSOR_EGO_CENTRIC
        if self.rgb:
            m |= nat.SENSOR_RGB
        return m

    def done_mask(self) -> int:
        m = 0
        for bit, on in (
            (nat.DONE_COLLISION, self.done_collision), (nat.DONE_OFF_ROAD, self.done_off_road),
            (nat.DONE_OFF_ROUTE, self.done_off_route), (nat.DONE_ON_SHOULDER, self.done_on_shoulder),
            (nat.DONE_WRONG_WAY, self.done_wrong_way), (nat.DONE_NOT_MOVING, self.done_not_moving),
        ):
            if on:
                m |= bit
        return m

    def reset_elapsed_steps(self) -> int:
        """Ticks the reference burns in ``reset()`` before the first ego observation exists:
        the trap fires once ``mission.start_time`` (0.1 s, plan.py:209) has *passed*
        (trap_manager.py:53-65), and ``reset`` spins ``step({})`` until then (smarts.py:426-434)."""
        if self.entry_reset_steps is not None:
            return int(self.entry_reset_steps)
        return int(math.floor(0.1 / self.dt + 1e-9)) + 1


def pack_trajectory(trajectory) -> Tuple[np.ndarray, int]:
    """(xs, ys, headings, speeds) of any length -> ([4, 11] float64, length): the first ten points and,
    in column 10, the last one — everything ``perform_trajectory_tracking_PD`` reads
    (trajectory_tracking_controller.py:176-473)."""
    n = len(trajectory[0])
    if n < 1 or any(len(r) != n for r in trajectory):
        raise ValueError("a trajectory is four equally long sequences (x, y, heading, speed)")
    out = np.zeros((4, nat.TRAJ_COLS), dtype=np.float64)
    for r in range(4):
        head = np.asarray(trajectory[r][:10], dtype=np.float64)
        out[r, :len(head)] = head
        out[r, 10] = float(trajectory[r][n - 1])
    return out, n


def lane_heading(shape: np.ndarray, seg: int) -> float:
    vx, vy = shape[seg + 1] - shape[seg]
    # heading convention of the reference (0 = +y, counter-clockwise)
    h = math.atan2(vy, vx) - math.pi / 2
    return (h + math.pi) % (2 * math.pi) - math.pi


def make_spawns(cm: CompiledMap, num_envs: int, num_vehicles: int, episodes: int = 1, seed: int = 42,
                first_env: int = 0, min_gap: float = 8.0, return_lanes: bool = False):
    """Synthetic spawn table: vehicle k of env e starts on lane (k mod L) of the
    map's normal lanes at an arclength drawn U(0.05, 0.95)*lane_length from
    ``numpy.random.Generator(PCG64(seed + e))``, re-drawn while within ``min_gap`` metres of an
    earlier vehicle on that lane; heading = lane heading, speed = lane speed limit.
    Returns ``[episodes, num_envs * num_vehicles, 4]`` (x, y, heading, speed); with
    ``return_lanes`` also ``[episodes, num_envs * num_vehicles, 2]`` (lane index, arclength), which
    is what scripted social vehicles start from."""
    lanes = [i for i in range(cm.n_lanes) if not cm.lane_in_junction[i]]
    shapes = [cm.lane_shape(i) for i in lanes]
    cums = []
    for sh in shapes:
        acc, cum = 0.0, [0.0]
        for a, b in zip(sh[:-1], sh[1:]):  # vertex by vertex, like smx_shape_rec.cum
            ex, ey = float(a[0] - b[0]), float(a[1] - b[1])
            acc = acc + math.sqrt(ex * ex + ey * ey)
            cum.append(acc)
        cums.append(np.array(cum))
    out = np.zeros((episodes, num_envs * num_vehicles, 4), dtype=np.float64)
    where = np.zeros((episodes, num_envs * num_vehicles, 2), dtype=np.float64)
    L = len(lanes)
    for e in range(num_envs):
        rng = np.random.Generator(np.random.PCG64(seed + first_env + e))
        for ep in range(episodes):
            taken: Dict[int, list] = {}
            for k in range(num_vehicles):
                li = k % L
                cum = cums[li]
                total = cum[-1]
                for _ in range(1000):
                    off = rng.uniform(0.05, 0.95) * total
                    if all(abs(off - o) >= min_gap for o in taken.get(li, ())):
                        break
                taken.setdefault(li, []).append(off)
                seg = int(np.searchsorted(cum, off, side="right") - 1)
                seg = min(max(seg, 0), len(cum) - 2)
                f = (off - cum[seg]) / (cum[seg + 1] - cum[seg]) if cum[seg + 1] > cum[seg] else 0.0
                sh = shapes[li]
                x = sh[seg, 0] + (sh[seg + 1, 0] - sh[seg, 0]) * f
                y = sh[seg, 1] + (sh[seg + 1, 1] - sh[seg, 1]) * f
                out[ep, e * num_vehicles + k] = (x, y, lane_heading(sh, seg), cm.lane_speed[lanes[li]])
                where[ep, e * num_vehicles + k] = (lanes[li], off)
    return (out, where) if return_lanes else out


from .map_compiler import map_tables_struct  # noqa: E402,F401  (torch-free; also used by tests/native)


def check_guard(num_envs: int, num_vehicles: int, count: int, margin: float = nat.GUARD_MARGIN_DEFAULT) -> None:
    """``smx_check_guard``: would ``smx_set_guard`` take a byte buffer of ``count`` elements and this margin for a
    shard of ``num_envs`` x ``num_vehicles``?  Needs the built library, no device and no handle; raises ``ValueError``
    with the library's reason when not.  (The margin against a map's cell sizes is checked where the map is known:
    ``smx_set_guard`` / ``smx_load_map``.)"""
    lib = nat.load_library()
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles = int(num_envs), int(num_vehicles)
    err = C.create_string_buffer(512)
    if lib.smx_check_guard(C.byref(c), int(count), float(margin), err, len(err)) != 0:
        raise ValueError(err.value.decode())


def check_agent_dims(action_space: str, num_envs: int, num_vehicles: int, num_social: int, dims: np.ndarray) -> None:
    """``smx_check_agent_dims``: would ``smx_set_agent_dims`` take the float64 table ``dims`` ``(R, E, A, 3)`` for a shard
    of this shape and action space?  Needs the built library, no device and no handle; raises ``ValueError`` with the
    library's reason when not."""
    lib = nat.load_library()
    dims = _agent_dims_table(dims, int(num_envs), int(num_vehicles) - int(num_social))
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.num_social = int(num_envs), int(num_vehicles), int(num_social)
    if action_space not in nat.ACTION_SPACES:
        raise ValueError(f"action space {action_space!r} is not on the accelerated path")
    c.action_space = nat.ACTION_SPACES[action_space]
    ad = nat.SmxAgentDims()
    ad.dims_host, ad.rows = dims.ctypes.data, int(dims.shape[0])
    err = C.create_string_buffer(512)
    if lib.smx_check_agent_dims(C.byref(c), C.byref(ad), err, len(err)) != 0:
        raise ValueError(err.value.decode())


def _agent_space_codes(spaces: Sequence[str]) -> np.ndarray:
    unknown = [s for s in spaces if s not in nat.ACTION_SPACES]
    if unknown:
        raise ValueError(f"action space {unknown[0]!r} is not on the accelerated path (supported: {sorted(nat.ACTION_SPACES)})")
    return np.ascontiguousarray([nat.ACTION_SPACES[s] for s in spaces], dtype=np.int32)


def check_agent_spaces(action_space: str, num_vehicles: int, num_social: int, spaces: Sequence[str]) -> None:
    """``smx_check_agent_spaces``: would ``smx_set_agent_spaces`` take ``spaces`` — one action space name per agent slot —
    for a shard of this shape whose ``SimConfig.action_space`` is ``action_space``?  Needs the built library, no device
    and no handle; raises ``ValueError`` with the library's reason when not."""
    lib = nat.load_library()
    codes = _agent_space_codes(list(spaces) + [action_space])
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.num_social, c.action_space = 1, int(num_vehicles), int(num_social), int(codes[-1])
    sp = nat.SmxAgentSpaces()
    sp.space_host, sp.n_agents = codes.ctypes.data, len(codes) - 1
    err = C.create_string_buffer(512)
    if lib.smx_check_agent_spaces(C.byref(c), C.byref(sp), err, len(err)) != 0:
        raise ValueError(err.value.decode())


def check_agent_entry(num_envs: int, num_vehicles: int, num_social: int, ready_ticks: np.ndarray, check: np.ndarray) -> None:
    """``smx_check_agent_entry``: would ``smx_set_agent_entry`` take the int32 table ``ready_ticks`` ``(R, E, A)`` and the
    float64 table ``check`` ``(R, E, A, 3)`` for a shard of this shape?  Needs the built library, no device and no handle;
    raises ``ValueError`` with the library's reason when not."""
    lib = nat.load_library()
    ready, chk = _agent_entry_tables(ready_ticks, check, int(num_envs), int(num_vehicles) - int(num_social))
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.num_social = int(num_envs), int(num_vehicles), int(num_social)
    en = nat.SmxAgentEntry()
    en.ready_host, en.check_host, en.rows = ready.ctypes.data, chk.ctypes.data, int(ready.shape[0])
    # (the rows' extents are what the check reads of them; no device buffer is touched)
    en.status_dev, en.entered_dev = 1, 1
    en.status_count = en.entered_count = int(num_envs) * int(num_vehicles)
    err = C.create_string_buffer(512)
    if lib.smx_check_agent_entry(C.byref(c), C.byref(en), err, len(err)) != 0:
        raise ValueError(err.value.decode())


def _mission_pool_struct(cm: CompiledMap, missions: Sequence, vias: Optional[Sequence[Sequence]]):
    """``smx_mission_pool`` of a pool of ``PlannedMission | None`` and the via list of each (host side; the caller adds the
    table of rows), with the arrays it points into."""
    M = len(missions)
    if vias is not None and len(vias) != M:
        raise ValueError("mission pool: one via list per pool entry")
    road_no = {rid: i for i, rid in enumerate(cm.road_ids)}
    recs = (nat.SmxMission * max(M, 1))()
    goals = (nat.SmxMissionGoal * max(M, 1))()
    roads = []
    for s, m in enumerate(missions):
        if m is None:
            continue
        recs[s].goal_x, recs[s].goal_y, recs[s].goal_radius = m.goal
        recs[s].route_off, recs[s].route_len = len(roads), len(m.route_roads)
        roads += [road_no[r] for r in m.route_roads]
        kind = getattr(m, "goal_kind", nat.GOAL_POSITIONAL)
        goals[s].kind, goals[s].num_laps, goals[s].route_length = kind, int(m.num_laps), float(m.route_length)
    road_arr = (C.c_int32 * max(len(roads), 1))(*roads)
    keep = [recs, goals, road_arr]
    mp = nat.SmxMissionPool()
    mp.missions_host, mp.n_missions = C.addressof(recs), M
    mp.route_roads_host, mp.n_route_roads = C.addressof(road_arr), len(roads)
    if any(goals[s].kind != nat.GOAL_POSITIONAL for s in range(M)):
        mp.goals_host = C.addressof(goals)
        if any(goals[s].kind == nat.GOAL_TRAVERSE for s in range(M)):
            from .missions import lane_end_tables

            h, d = lane_end_tables(cm)  # the two lane facts of TraverseGoal: host libm
            h, d = np.ascontiguousarray(h, dtype=np.float64), np.ascontiguousarray(d, dtype=np.int32)
            mp.lane_end_heading_host, mp.lane_dead_end_host, mp.n_lanes = h.ctypes.data, d.ctypes.data, len(h)
            keep += [h, d]
    flat = [v for lst in (vias or []) for v in lst]
    if flat:
        vrecs = (nat.SmxVia * len(flat))()
        for i, v in enumerate(flat):
            vrecs[i].x, vrecs[i].y = v.position
            vrecs[i].hit_distance, vrecs[i].required_speed, vrecs[i].lane = v.hit_distance, v.required_speed, v.lane
        offs = (C.c_int32 * (M + 1))(*np.concatenate([[0], np.cumsum([len(lst) for lst in vias])]).astype(int).tolist())
        mp.vias_host, mp.via_off_host, mp.n_vias = C.addressof(vrecs), C.addressof(offs), len(flat)
        keep += [vrecs, offs]
    return mp, keep


def check_mission_pool(cm: CompiledMap, num_envs: int, num_vehicles: int, num_social: int, missions: Sequence,
                       vias: Optional[Sequence[Sequence]] = None, rows: Optional[np.ndarray] = None, via_max: int = 0) -> None:
    """``smx_check_mission_pool``: would ``smx_set_mission_pool`` take this pool — ``PlannedMission | None`` entries, a via
    list per entry — and a table of rows of the shape of ``rows`` (host int32 ``(R, E, A)``; ``None``: one row) for a
    shard of this shape on map ``cm``?  The host copy of the table is checked here as well: every entry in -1 .. M - 1
    (on the device such an entry is read as -1 and reported by the next ``sync``).  Needs the built library, no device
    and no handle; raises ``ValueError`` with the reason when not."""
    lib = nat.load_library()
    E, A = int(num_envs), int(num_vehicles) - int(num_social)
    table = np.full((1, E, max(A, 0)), -1, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    if table.ndim != 3 or table.shape[0] < 1 or tuple(table.shape[1:]) != (E, A):
        raise ValueError(f"mission rows must be int32 of shape (R, {E}, {A}), got {tuple(table.shape)}")
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.num_social, c.via_max = E, int(num_vehicles), int(num_social), int(via_max)
    mp, keep = _mission_pool_struct(cm, missions, vias)
    mp.rows_dev, mp.rows_count, mp.rows = table.ctypes.data, int(table.size), int(table.shape[0])  # (only tested for NULL)
    tables, keep_map = map_tables_struct(cm)
    err = C.create_string_buffer(512)
    rc = lib.smx_check_mission_pool(C.byref(c), C.byref(tables), C.byref(mp), err, len(err))
    del keep, keep_map
    if rc != 0:
        raise ValueError(err.value.decode())
    if table.size and (table.min() < -1 or table.max() >= len(missions)):
        raise ValueError(f"mission rows: entries must lie in -1 .. {len(missions) - 1}")


def _agent_entry_tables(ready_ticks, check, num_envs: int, num_agents: int) -> Tuple[np.ndarray, np.ndarray]:
    ready = np.ascontiguousarray(ready_ticks, dtype=np.int32)
    chk = np.ascontiguousarray(check, dtype=np.float64)
    if ready.ndim != 3 or ready.shape[0] < 1 or tuple(ready.shape[1:]) != (num_envs, num_agents):
        raise ValueError(f"ready ticks must be int32 of shape (R, {num_envs}, {num_agents}), got {tuple(ready.shape)}")
    if tuple(chk.shape) != tuple(ready.shape) + (3,):
        raise ValueError(f"check must be float64 of shape {tuple(ready.shape) + (3,)}, got {tuple(chk.shape)}")
    return ready, chk


def _agent_dims_table(dims, num_envs: int, num_agents: int) -> np.ndarray:
    dims = np.ascontiguousarray(dims, dtype=np.float64)
    if dims.ndim != 4 or dims.shape[0] < 1 or tuple(dims.shape[1:]) != (num_envs, num_agents, 3):
        raise ValueError(f"agent dims must be float64 of shape (R, {num_envs}, {num_agents}, 3), got {tuple(dims.shape)}")
    return dims


class BatchedSim:
    """One shard of environment instances resident on one GPU."""

    def __init__(self, cm: CompiledMap, cfg: SimConfig, device: str = "cuda:0", spawns: Optional[np.ndarray] = None,
                 spawn_episodes: int = 2, seed: int = 42, first_env: int = 0, social_spawns: Optional[np.ndarray] = None,
                 vias: Optional[Sequence[Sequence]] = None, missions: Optional[Sequence] = None):
        """``vias``: per agent slot, a list of ``vias.ResolvedVia`` (the missions' via points).
        ``missions``: per vehicle slot ``None`` (endless mission, empty route) or a
        ``missions.PlannedMission`` (fixed route + PositionalGoal, a lap goal, or an empty route with an endless or
        a traverse goal); see ``set_missions``."""
        self.lib = nat.load_library()
        if not torch.cuda.is_available():
            raise nat.NativeLibraryError("no ROCm device visible: the smarts_amd hot path runs on the GPU only")
        self.cm = cm
        self.cfg = cfg
        self.device = torch.device(device)
        E, N = cfg.num_envs, cfg.num_vehicles
        self.E, self.N = E, N
        dev = self.device
        idx = self.device.index if self.device.index is not None else 0

        c = nat.SmxConfig()
        c.num_envs, c.num_vehicles, c.dt = E, N, cfg.dt
        c.sensors, c.done_criteria = cfg.sensors_mask(), cfg.done_mask()
        c.wp_lookahead, c.wp_paths, c.wp_len = cfg.wp_lookahead, cfg.wp_paths, cfg.wp_len
        c.nb_max = cfg.nb_max
        c.nb_radius = -1.0 if cfg.nb_radius is None else float(cfg.nb_radius)
        c.max_episode_steps = cfg.max_episode_steps or 0
        c.not_moving_time, c.not_moving_distance = cfg.not_moving_time, cfg.not_moving_distance
        c.auto_reset = 1 if cfg.auto_reset else 0
        c.reset_elapsed_steps = cfg.reset_elapsed_steps()
        if cfg.action_space not in nat.ACTION_SPACES:
            raise ValueError(f"action space {cfg.action_space!r} is not on the accelerated path "
                             f"(supported: {sorted(nat.ACTION_SPACES)})")
        c.action_space = nat.ACTION_SPACES[cfg.action_space]
        c.num_social, c.social_speed_factor = int(cfg.num_social), float(cfg.social_speed_factor)
        c.social_model = nat.SOCIAL_MODELS[cfg.social_model]
        self.vias = [list(v) for v in vias] if vias is not None else None
        if self.vias is not None and cfg.via_max <= 0:
            raise ValueError("vias need SimConfig(via_max > 0)")
        c.via_max = int(cfg.via_max)
        c.alive_min_ego, c.alive_min_total = int(cfg.alive_min_ego or 0), int(cfg.alive_min_total or 0)
        if len(cfg.alive_lists) > 4:
            raise ValueError("DoneCriteria.agents_alive: at most four agent lists on the accelerated path")
        c.alive_lists = len(cfg.alive_lists)
        for k, (slots, minimum) in enumerate(cfg.alive_lists):
            mask = 0
            for i in slots:
                if not 0 <= int(i) < N - cfg.num_social:
                    raise ValueError(f"agents_alive list {k}: slot {i} is not an agent slot")
                mask |= 1 << int(i)
            c.alive_list_mask[k], c.alive_list_min[k] = mask, int(minimum)
        if cfg.ogm:
            c.ogm_width, c.ogm_height, c.ogm_resolution = cfg.ogm_width, cfg.ogm_height, cfg.ogm_resolution
        if cfg.lidar is not None:
            c.lidar_rays, c.lidar_max_distance = ray_count(cfg.lidar), cfg.lidar.max_distance
        if cfg.dagm:
            c.dagm_width, c.dagm_height, c.dagm_resolution = cfg.dagm_width, cfg.dagm_height, cfg.dagm_resolution
        if cfg.road_waypoints:
            c.rw_horizon, c.rw_lanes, c.rw_paths = int(cfg.rw_horizon), int(cfg.rw_lanes), int(cfg.rw_paths)
        if cfg.rgb:
            c.rgb_width, c.rgb_height, c.rgb_resolution = int(cfg.rgb_width), int(cfg.rgb_height), float(cfg.rgb_resolution)
        if cfg.frame_stack == 1 or not 0 <= cfg.frame_stack <= nat.STACK_MAX_FRAMES:
            raise ValueError(f"frame_stack must be 0 (off) or 2..{nat.STACK_MAX_FRAMES} (the reference asserts num_stack > 1)")
        if (cfg.frame_stack_rows or cfg.frame_stack_rgb_dstack) and not cfg.frame_stack:
            raise ValueError("frame_stack_rows / frame_stack_rgb_dstack need SimConfig(frame_stack >= 2)")
        c.frame_stack = int(cfg.frame_stack)
        self._c = c
        self.handle = C.c_void_p()
        rc = self.lib.smx_create(C.byref(c), idx, C.byref(self.handle))
        nat.check(self.lib, self.handle, rc, "smx_create")
        rc = self.lib.smx_set_launch_strategy(self.handle, nat.LAUNCH_STRATEGIES[cfg.launch_strategy])
        nat.check(self.lib, self.handle, rc, "smx_set_launch_strategy")
        tables, keep = map_tables_struct(cm)
        nat.check(self.lib, self.handle, self.lib.smx_load_map(self.handle, C.byref(tables)), "smx_load_map")
        del keep
        if self.vias is not None:
            if len(self.vias) != N:
                raise ValueError("vias: one list per vehicle slot")
            flat = [v for lst in self.vias for v in lst]
            recs = (nat.SmxVia * max(len(flat), 1))()
            for i, v in enumerate(flat):
                recs[i].x, recs[i].y = v.position
                recs[i].hit_distance, recs[i].required_speed, recs[i].lane = v.hit_distance, v.required_speed, v.lane
            offs = (C.c_int32 * (N + 1))(*np.concatenate([[0], np.cumsum([len(lst) for lst in self.vias])]).astype(int).tolist())
            nat.check(self.lib, self.handle, self.lib.smx_set_vias(self.handle, recs, len(flat), offs), "smx_set_vias")
        self.missions = None
        self.mission_pool = self.mission_rows = None  # set_mission_pool
        if missions is not None:
            self.set_missions(missions)
        if cfg.lidar is not None:
            self.lidar_rays = torch.from_numpy(base_rays(cfg.lidar)).to(dev)
            rc = self.lib.smx_set_lidar_rays(self.handle, self.lidar_rays.data_ptr(), int(self.lidar_rays.shape[0]))
            nat.check(self.lib, self.handle, rc, "smx_set_lidar_rays")

        # ---- state ----
        T = E * N
        self.state = torch.zeros((nat.S_COUNT, E, N), dtype=torch.float64, device=dev)
        self.flags = torch.zeros((E, N), dtype=torch.int32, device=dev)
        self.steps = torch.zeros((E, N), dtype=torch.int32, device=dev)
        self.env_ticks = torch.zeros((E,), dtype=torch.int32, device=dev)
        self.env_done_count = torch.zeros((E,), dtype=torch.int32, device=dev)
        self.env_episode = torch.full((E,), -1, dtype=torch.int32, device=dev)
        need_ring = cfg.track_driven_path or cfg.done_not_moving
        self.driven_path = torch.zeros((T, nat.DRIVEN_PATH_LEN), dtype=torch.float64, device=dev) if need_ring else None
        self.seed_cache = torch.full((nat.SEED_COUNT, E, N), -1, dtype=torch.int32, device=dev)
        self.facts_i32 = torch.full((nat.FACT_I_COUNT, E, N), -1, dtype=torch.int32, device=dev)
        self.facts_f64 = torch.zeros((nat.FACT_F_COUNT, E, N), dtype=torch.float64, device=dev)
        self.env_reset_pending = torch.zeros((E,), dtype=torch.int32, device=dev)
        st = nat.SmxState()
        for name, t in (("f64", self.state), ("flags", self.flags), ("steps", self.steps), ("env_ticks", self.env_ticks),
                        ("env_done_count", self.env_done_count), ("env_episode", self.env_episode),
                        ("driven_path", self.driven_path), ("seed_cache", self.seed_cache),
                        ("facts_i32", self.facts_i32), ("facts_f64", self.facts_f64),
                        ("env_reset_pending", self.env_reset_pending)):
            nat.bind_buffer(st, nat.STATE_BUFFERS, name, t)  # pointer + element count + dtype (checked on entry)
        self._st = st

        # ---- spawns ----
        if spawns is None:
            spawns, where = make_spawns(cm, E, N, episodes=spawn_episodes, seed=seed, first_env=first_env,
                                        return_lanes=True)
            if social_spawns is None:
                social_spawns = where
        spawns = np.ascontiguousarray(spawns, dtype=np.float64)
        assert spawns.ndim == 3 and spawns.shape[1:] == (T, 4), spawns.shape
        self.spawns = torch.from_numpy(spawns).to(dev)
        sp = nat.SmxSpawns()
        sp.episodes, sp.pose, sp.pose_count = int(spawns.shape[0]), self.spawns.data_ptr(), self.spawns.numel()
        self.social_spawns = None
        if cfg.num_social > 0:
            if social_spawns is None:
                raise ValueError("num_social > 0 with an explicit spawn table needs social_spawns "
                                 "(make_spawns(..., return_lanes=True))")
            social_spawns = np.ascontiguousarray(social_spawns, dtype=np.float64)
            assert social_spawns.shape == (spawns.shape[0], T, 2), social_spawns.shape
            self.social_spawns = torch.from_numpy(social_spawns).to(dev)
            sp.social, sp.social_count = self.social_spawns.data_ptr(), self.social_spawns.numel()
        self._sp = sp

        # ---- outputs (dense StdObs layout, format_obs.py:313-373) ----
        o: Dict[str, torch.Tensor] = {}
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        o["ego_pos"] = z((E, N, 3), torch.float64)
        o["ego_f32"] = z((E, N, nat.EGO_F32_COUNT), torch.float32)
        o["ego_lane"] = z((E, N, 2), torch.int16)
        o["events"] = z((E, N, nat.EV_COUNT), torch.uint8)
        o["reward"] = z((E, N), torch.float64)
        o["dist"] = z((E, N), torch.float64)
        o["done"] = z((E, N), torch.uint8)
        o["active"] = z((E, N), torch.uint8)
        o["env_done"] = z((E,), torch.uint8)
        if cfg.waypoints:
            P, W = cfg.wp_paths, cfg.wp_len
            o["wp_pos"] = z((E, N, P, W, 3), torch.float64)
            o["wp_heading"] = z((E, N, P, W), torch.float32)
            o["wp_lane_width"] = z((E, N, P, W), torch.float32)
            o["wp_speed_limit"] = z((E, N, P, W), torch.float32)
            o["wp_lane_index"] = z((E, N, P, W), torch.int8)
            o["wp_lane_id"] = z((E, N, P, W), torch.int16)
            o["wp_count"] = z((E, N, P + 1), torch.uint8)
        if cfg.neighbors:
            K = cfg.nb_max
            o["nb_pos"] = z((E, N, K, 3), torch.float64)
            o["nb_box"] = z((E, N, K, 3), torch.float32)
            o["nb_heading"] = z((E, N, K), torch.float32)
            o["nb_speed"] = z((E, N, K), torch.float32)
            o["nb_lane_index"] = z((E, N, K), torch.int8)
            o["nb_lane_id"] = z((E, N, K), torch.int16)
            o["nb_slot"] = z((E, N, K), torch.int8)
            o["nb_count"] = z((E, N), torch.uint8)
        if cfg.via_max > 0:
            o["via_near"] = torch.full((E, N, cfg.via_max), -1, dtype=torch.int8, device=dev)
            o["via_near_count"] = z((E, N), torch.uint8)
            o["via_hit"] = z((E, N), torch.int32)
        if cfg.ogm:
            o["ogm"] = z((E, N, cfg.ogm_height, cfg.ogm_width), torch.uint8)
        if cfg.dagm:
            o["dagm"] = z((E, N, cfg.dagm_height, cfg.dagm_width), torch.uint8)
        if cfg.road_waypoints:
            L, Q, R = cfg.rw_lanes, cfg.rw_paths, 2 * cfg.rw_horizon + 1
            o["rw_lane_count"] = z((E, N), torch.uint8)
            o["rw_lane"] = torch.full((E, N, L), -1, dtype=torch.int16, device=dev)
            o["rw_path_count"] = z((E, N, L), torch.int16)
            o["rw_count"] = z((E, N, L, Q), torch.uint8)
            o["rw_pos"] = z((E, N, L, Q, R, 3), torch.float64)
            o["rw_heading"] = z((E, N, L, Q, R), torch.float32)
            o["rw_lane_width"] = z((E, N, L, Q, R), torch.float32)
            o["rw_speed_limit"] = z((E, N, L, Q, R), torch.float32)
            o["rw_lane_index"] = z((E, N, L, Q, R), torch.int8)
            o["rw_lane_id"] = z((E, N, L, Q, R), torch.int16)
        if cfg.lane_ttc:
            o["lane_ttc"] = z((E, N, nat.TTC_COUNT), torch.float64)
            o["lane_ttc_flags"] = z((E, N), torch.uint8)
        if cfg.lidar is not None:
            R = ray_count(cfg.lidar)
            o["lidar_hit"] = z((E, N, R), torch.uint8)
            o["lidar_point"] = z((E, N, R, 3), torch.float64)
        if cfg.ego_centric:
            o["ego_frame"] = z((E, N, 4), torch.float64)
            o["ec_flags"] = z((E, N), torch.uint8)
            o["ec_ego_f32"] = z((E, N, nat.EGO_F32_COUNT), torch.float32)
            for name in ("wp_pos", "wp_heading", "nb_pos", "nb_heading", "lidar_point", "rw_pos", "rw_heading"):
                if name in o:  # a twin of every position / heading row whose sensor is on
                    o["ec_" + name] = torch.zeros_like(o[name])
        # learner-facing block (reward, done) as float32, two buffers used on alternate ticks so that
        # one can be in flight in a collective while the next tick writes the other
        self._learner = [z((2, E, N), torch.float32), z((2, E, N), torch.float32)]
        self._learner_k = 0
        o["learner"] = self._learner[0]
        self.out = o
        o["collidees"] = z((E, N), torch.int64)  # bit j: touching the vehicle in slot j (read as unsigned)
        if cfg.auto_reset:
            # the finishing tick's low-dimensional rows of an env that restarts inside the launch (include/smx.h)
            o["final_ego_pos"] = z((E, N, 3), torch.float64)
            o["final_ego_f32"] = z((E, N, nat.EGO_F32_COUNT), torch.float32)
            o["final_ego_lane"] = z((E, N, 2), torch.int16)
            o["final_events"] = z((E, N, nat.EV_COUNT), torch.uint8)
            o["final_dist"] = z((E, N), torch.float64)
        so = nat.SmxOutputs()
        for name in nat.OUTPUT_BUFFERS:
            nat.bind_buffer(so, nat.OUTPUT_BUFFERS, name, o.get(name))
        self._out = so
        if cfg.rgb:
            # not a member of smx_outputs (its pointer list is closed): a buffer of its own, bound to the handle
            o["rgb"] = z((E, N, cfg.rgb_height, cfg.rgb_width, 3), torch.uint8)
            self.bind_rgb(o["rgb"])
        if cfg.state_guard:
            # like the image: a buffer of its own, bound to the handle
            self.bind_guard(z((E, N), torch.uint8))
        if cfg.frame_stack:
            if cfg.frame_stack_rgb_dstack and not cfg.rgb:
                raise ValueError("frame_stack_rgb_dstack needs SimConfig(rgb=True)")
            for row in cfg.frame_stack_rows:
                nat.stack_source(row)  # (a row that cannot be stacked: ValueError)
                if row not in o:
                    raise ValueError(f"frame_stack_rows: {row!r} is not a row of this configuration (its sensor is off)")
            for row in cfg.frame_stack_rows:
                self.bind_frame_stack(row, z((E, N, cfg.frame_stack) + tuple(o[row].shape[2:]), o[row].dtype))
            if cfg.frame_stack_rgb_dstack:
                self.bind_frame_stack("rgb", z((E, N, cfg.rgb_height, cfg.rgb_width, 3 * cfg.frame_stack), torch.uint8),
                                      layout="dstack")
        self._stream = None
        self._was_reset = False

    # ------------------------------------------------------------------
    def _stream_ptr(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def output_bytes_per_agent_step(self) -> int:
        """Bytes of observation/reward/done written per agent-step (dense layout); with frame stacking on, the k
        frames of every stack the pass rewrites among them."""
        per = 0
        for name, t in self.out.items():
            if name in ("env_done", "learner") or name.startswith("final_"):
                continue
            per += t[0, 0].numel() * t.element_size()
        return per

    def state_bytes_per_agent_step(self) -> int:
        return nat.S_COUNT * 8 + 4 + 4 + nat.SEED_COUNT * 4

    def kernel_bytes_per_agent_step(self) -> Dict[str, Tuple[int, int]]:
        """Algorithmic HBM bytes of one agent-step as (read, write) per timing phase — SURVEY.md §8(d)'s
        accounting on this layout: compulsory reads of the vehicle's own state and action, the state written
        back, and every observation / reward / done byte of the dense rows.  NOT counted: the map tables
        (L2 / Infinity-Cache resident) and the hand-off buffers between the kernels of a tick (path seeds,
        road facts: ``handoff_bytes_per_agent_step``) — traffic this design adds, not traffic the path needs."""
        o = {k: (t[0, 0].numel() * t.element_size()) for k, t in self.out.items()
             if k not in ("env_done", "learner", "rgb_dstack")
             and not k.startswith(("final_", "stack_"))}  # (final_*: copied for restarting envs only; the stacks: below)
        pose = 3 * 8 + 4  # x, y, heading + flags: what every sensor kernel reads of a vehicle
        ctrl_state = 14 * 8 + 4  # SMX_S_X .. SMX_S_MCL_Y + flags: read and written back by k_control
        obs_state_r, obs_state_w = 16 * 8 + 4 + 4, 12 * 8 + 4  # trip meter / accelerometer / driven-path fields, steps
        wp = sum(v for k, v in o.items() if k.startswith("wp_")) if self.cfg.waypoints else 0
        rows = sum(v for k, v in o.items() if not k.startswith(("wp_", "ogm", "lidar", "dagm", "rw_", "rgb"))) + 8  # + learner block
        kb = {
            "control": (ctrl_state + (12 if self.cfg.action_space != "Lane" else 1), ctrl_state + 2 * 8),
            "scan": (pose, 0),
            "sensors": ((pose if self.cfg.waypoints else 0) + obs_state_r, wp + rows + obs_state_w),
            "commit": (4, 4),
        }
        ogm = (pose, o["ogm"]) if self.cfg.ogm else (0, 0)
        dagm = (pose, o["dagm"]) if self.cfg.dagm else (0, 0)
        rgb = (pose, o["rgb"]) if self.cfg.rgb else (0, 0)
        tile = self.cfg.ogm_width * self.cfg.ogm_height
        ogm_env_small = (self.small_form() and self.E * self.N >= nat.OGM_ENV_MIN_VEHICLES and self.N <= 32
                         and tile * 8 <= 64 * 1024)  # smx_plan.h tick_plan(): k_ogm_env on small batches too
        ogm_inline = (self.cfg.ogm and tile <= 16 * 1024
                      and self.small_form() and not ogm_env_small)  # smx_plan.h tick_plan(): small batches only
        add = lambda a, b: (a[0] + b[0], a[1] + b[1])  # noqa: E731
        if (self.cfg.ogm and not ogm_inline) or self.cfg.dagm or self.cfg.rgb:
            kb["ogm"] = add(add((0, 0) if ogm_inline else ogm, dagm), rgb)  # their own launches (one timing phase)
        if ogm_inline:
            kb["sensors"] = add(kb["sensors"], ogm)
        if self.cfg.lidar is not None:
            kb["sensors"] = add(kb["sensors"], (pose, o["lidar_hit"] + o["lidar_point"]))
        stacks = sum(t[0, 0].numel() * t.element_size() for k, t in self.out.items() if k.startswith("stack_") or k == "rgb_dstack")
        if stacks:  # k_frame_push / k_frame_dstack shift in place: k frames read (k - 1 old, one new), k written
            kb["frame_stack"] = (stacks + 4 + 1, stacks)
        return kb

    def set_missions(self, missions: Optional[Sequence]):
        """Missions per vehicle slot, shared by every env (``smx_set_missions``, and ``smx_set_mission_goals`` when
        a slot has a lap or a traverse goal): ``None`` entries (or ``missions=None``) are endless missions with an
        empty route."""
        N = self.N
        if missions is None or all(m is None for m in missions):
            nat.check(self.lib, self.handle, self.lib.smx_set_missions(self.handle, None, 0, None, 0), "smx_set_missions")
            self.missions = None
            return
        if len(missions) != N:
            raise ValueError("missions: one entry per vehicle slot")
        road_no = {rid: i for i, rid in enumerate(self.cm.road_ids)}
        recs = (nat.SmxMission * N)()
        roads = []
        for s, m in enumerate(missions):
            if m is None:
                continue
            recs[s].goal_x, recs[s].goal_y, recs[s].goal_radius = m.goal
            recs[s].route_off, recs[s].route_len = len(roads), len(m.route_roads)
            roads += [road_no[r] for r in m.route_roads]
        arr = (C.c_int32 * max(len(roads), 1))(*roads)
        nat.check(self.lib, self.handle, self.lib.smx_set_missions(self.handle, recs, N, arr, len(roads)), "smx_set_missions")
        self.missions = list(missions)
        # goal kinds beyond the positional one (smx_set_mission_goals; smx_set_missions left every slot positional)
        kinds = [getattr(m, "goal_kind", nat.GOAL_POSITIONAL) if m is not None else nat.GOAL_POSITIONAL for m in missions]
        if any(k != nat.GOAL_POSITIONAL for k in kinds):
            goals = (nat.SmxMissionGoal * N)()
            for s, m in enumerate(missions):
                if m is not None:
                    goals[s].kind, goals[s].num_laps, goals[s].route_length = kinds[s], int(m.num_laps), float(m.route_length)
            heading = dead_end = None
            n_lanes = 0
            if nat.GOAL_TRAVERSE in kinds:
                from .missions import lane_end_tables

                h, d = lane_end_tables(self.cm)  # the two lane facts of TraverseGoal: host libm, owned by the handle
                n_lanes = len(h)
                heading = np.ascontiguousarray(h, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
                dead_end = np.ascontiguousarray(d, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
                keep = (h, d)  # noqa: F841 (alive across the call)
            nat.check(self.lib, self.handle, self.lib.smx_set_mission_goals(self.handle, goals, N, heading, dead_end, n_lanes),
                      "smx_set_mission_goals")

    def set_mission_pool(self, missions: Optional[Sequence], vias: Optional[Sequence[Sequence]] = None,
                         rows: Optional[torch.Tensor] = None):
        """Bind a mission pool (``smx_set_mission_pool``): missions per env and per episode.  ``missions``: a sequence of
        ``PlannedMission | None`` (``None``: an endless mission), at most ``MISSION_POOL_MAX``; ``vias``: per pool entry a
        list of ``vias.ResolvedVia`` (needs ``SimConfig(via_max > 0)``); ``rows``: int32 ``(R, E, A)`` on the sim's device,
        ``A = N - num_social`` — agent ``a`` of env ``e`` has mission ``rows[k mod R, e, a]`` in episode ``k``, ``-1`` = an
        endless mission without vias.  The tensor stays the caller's and is read by every pass wherever a mission is
        needed: rewriting the row of a running episode changes that agent's mission in the middle of the episode; rows of
        episodes that have not started may be rewritten freely (a curriculum sampled on the device).  An entry outside
        ``-1 .. len(missions) - 1`` is read as ``-1`` and makes the next ``sync()`` raise.  The finishing tick of an
        episode reads the old episode's row, the first observation of the next one — a restart under ``auto_reset``
        included — the new one's.  Binding drops what ``set_missions`` and the constructor's ``vias`` bound, and while a
        pool is bound ``set_missions`` raises; ``set_mission_pool(None)`` unbinds (every mission endless again).  A shard
        of a larger batch binds its own slice ``rows[:, first_env:first_env + E]`` (contiguous), like every per-env
        table."""
        if missions is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_mission_pool(self.handle, None), "smx_set_mission_pool")
            self.mission_pool = self.mission_rows = None
            return
        want = (self.E, self.N - self.cfg.num_social)
        if (rows is None or rows.dtype != torch.int32 or rows.device != self.device or not rows.is_contiguous() or rows.ndim != 3
                or rows.shape[0] < 1 or tuple(rows.shape[1:]) != want):
            raise ValueError(f"rows must be a contiguous int32 tensor of shape [R, {want[0]}, {want[1]}] on {self.device}")
        mp, keep = _mission_pool_struct(self.cm, missions, vias)
        mp.rows_dev, mp.rows_count, mp.rows = rows.data_ptr(), int(rows.numel()), int(rows.shape[0])
        nat.check(self.lib, self.handle, self.lib.smx_set_mission_pool(self.handle, C.byref(mp)), "smx_set_mission_pool")
        del keep
        # (the library reads the tensor in every pass: it lives as long as the binding)
        self.mission_pool, self.mission_rows = (list(missions), [list(v) for v in vias] if vias is not None else None), rows
        self.missions = self.vias = None

    def bind_rgb(self, images: Optional[torch.Tensor]):
        """Bind the image buffer of the RGB sensor (``smx_set_rgb_output``): uint8 [E, N, rgb_height, rgb_width, 3] on
        the sim's device, or ``None`` to unbind.  ``out["rgb"]`` follows; a caller may alternate two buffers between
        ticks, as with the learner block."""
        if images is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_rgb_output(self.handle, None, 0), "smx_set_rgb_output")
            self.out.pop("rgb", None)
            return
        want = (self.E, self.N, self.cfg.rgb_height, self.cfg.rgb_width, 3)
        if images.dtype != torch.uint8 or not images.is_cuda or not images.is_contiguous() or tuple(images.shape) != want:
            raise ValueError(f"the rgb buffer must be a contiguous uint8 device tensor of shape {want}")
        rc = self.lib.smx_set_rgb_output(self.handle, images.data_ptr(), int(images.numel()))
        nat.check(self.lib, self.handle, rc, "smx_set_rgb_output")
        self.out["rgb"] = images

    def invalidate_outputs(self):
        """Tell the library that the caller wrote into ``out["ogm"]`` itself (``smx_invalidate_outputs``): the next call
        stores whole tiles.  The library stores only the pieces of an OGM tile that changed since its last call, so
        reading the rows is free, writing into them needs this call, and binding another tensor (``bind_ogm``) is
        noticed by itself."""
        nat.check(self.lib, self.handle, self.lib.smx_invalidate_outputs(self.handle), "smx_invalidate_outputs")

    def set_ogm_delta(self, on: bool):
        """OGM tiles stored as the pieces that changed (True, the default) or whole in every call (False:
        ``smx_set_ogm_delta``).  The rows read the same either way."""
        nat.check(self.lib, self.handle, self.lib.smx_set_ogm_delta(self.handle, 1 if on else 0), "smx_set_ogm_delta")

    def bind_ogm(self, tiles: torch.Tensor):
        """Point ``out["ogm"]`` at another tensor of the same shape; the next call stores whole tiles into it."""
        want = (self.E, self.N, self.cfg.ogm_height, self.cfg.ogm_width)
        if not self.cfg.ogm or tiles.dtype != torch.uint8 or tiles.device != self.device or not tiles.is_contiguous() or tuple(tiles.shape) != want:
            raise ValueError(f"the OGM rows must be a contiguous uint8 device tensor of shape {want} (SimConfig(ogm=True))")
        nat.bind_buffer(self._out, nat.OUTPUT_BUFFERS, "ogm", tiles)
        self.out["ogm"] = tiles

    def bind_guard(self, guard: Optional[torch.Tensor], margin: Optional[float] = None):
        """Bind the byte buffer of the state guard (``smx_set_guard``): uint8 [E, N] on the sim's device — which switches
        the guard on — or ``None`` to switch it off.  ``margin`` defaults to ``SimConfig.state_guard_margin``.
        ``out["guard"]`` follows."""
        if guard is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_guard(self.handle, None, 0, 0.0), "smx_set_guard")
            self.out.pop("guard", None)
            return
        if guard.dtype != torch.uint8 or tuple(guard.shape) != (self.E, self.N) or guard.device != self.device or not guard.is_contiguous():
            raise ValueError(f"the guard buffer must be a contiguous uint8 device tensor of shape {(self.E, self.N)}")
        margin = float(self.cfg.state_guard_margin if margin is None else margin)
        rc = self.lib.smx_set_guard(self.handle, guard.data_ptr(), int(guard.numel()), margin)
        nat.check(self.lib, self.handle, rc, "smx_set_guard")
        self.out["guard"] = guard

    def set_traffic_history(self, table, start_frames: Optional[torch.Tensor] = None, replaced: Optional[torch.Tensor] = None,
                            dims: bool = False):
        """Bind a recorded traffic history (``smx_set_social_history``; ``smarts_amd.traffic_history``): from the next
        pass on the social slots take pose, speed and presence from ``table`` (a ``TrafficHistoryTable`` with
        ``num_social`` slots) instead of the scripted lane follower.  ``start_frames``: int32 ``[R, E]`` on the sim's
        device, the table frame at which episode ``k`` of env ``e`` has tick count 0 (row ``k mod R``; any value is
        safe, frames outside the table are empty); ``None`` = one row of zeros.  ``replaced``: int32 ``[R, E]``, the
        vehicle id hidden in that env (an agent stands in for it; see ``table.spawn_of``), -1 for none; ``None`` = nothing
        hidden.  Both tensors stay the caller's and are read by every pass: rewriting them in place takes effect with
        the next tick (``include/smx.h`` says how presence follows).  ``dims=True`` also binds ``table.device_dims()``
        (``smx_set_social_history_dims``): collisions, ``nb_box``, OGM, RGB and lidar then see every replayed vehicle at
        its own size — the dataset's, or its type's default; off, every one has the sedan's box.  ``set_history_dims``
        switches that while the history stays bound.  ``table=None`` unbinds.  Refused with the
        library's reason (``SmxError``): a slot count other than ``num_social``, ``social_model="idm"``, a row of a
        present vehicle that is not finite or lies outside the map's grids."""
        if table is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_social_history(self.handle, None), "smx_set_social_history")
            self.traffic_history = self.history_start_frames = self.history_replaced = None
            self.history_dims = False
            self._drop_history_agents()
            return
        E = self.E
        if start_frames is None:
            start_frames = torch.zeros((1, E), dtype=torch.int32, device=self.device)
        for name, t in (("start_frames", start_frames), ("replaced", replaced)):
            if t is None:
                continue
            if t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or t.ndim != 2 or t.shape[1] != E or t.shape[0] < 1:
                raise ValueError(f"{name} must be a contiguous int32 tensor of shape [R, {E}] on {self.device}")
        if replaced is not None and replaced.shape != start_frames.shape:
            raise ValueError("start_frames and replaced must have the same shape [R, E]")
        frames = np.ascontiguousarray(table.frames, dtype=np.float64)
        vehicle = np.ascontiguousarray(table.vehicle, dtype=np.int32)
        hs = nat.SmxSocialHistory()
        hs.frames_host, hs.vehicle_host = frames.ctypes.data, vehicle.ctypes.data
        hs.n_frames, hs.num_social = int(frames.shape[0]), int(frames.shape[1])
        hs.start_frame_dev, hs.start_count, hs.rows = start_frames.data_ptr(), int(start_frames.numel()), int(start_frames.shape[0])
        if replaced is not None:
            hs.replaced_dev, hs.replaced_count = replaced.data_ptr(), int(replaced.numel())
        nat.check(self.lib, self.handle, self.lib.smx_set_social_history(self.handle, C.byref(hs)), "smx_set_social_history")
        # (the library reads the two tensors in every pass: they live as long as the binding)
        self.traffic_history, self.history_start_frames, self.history_replaced = table, start_frames, replaced
        self.history_dims = False  # (binding a history drops the dimensions of the one before)
        self._drop_history_agents()  # (... and its history agents)
        if dims:
            self.set_history_dims(True)

    def set_history_dims(self, on: bool):
        """Bind (``True``) the bound history's ``device_dims()`` or unbind them (``False``: the sedan's box again from the
        next tick), ``smx_set_social_history_dims``."""
        if not on:
            nat.check(self.lib, self.handle, self.lib.smx_set_social_history_dims(self.handle, None), "smx_set_social_history_dims")
            self.history_dims = False
            return
        if self.traffic_history is None:
            raise ValueError("set_history_dims needs a bound traffic history")
        table = np.ascontiguousarray(self.traffic_history.device_dims(), dtype=np.float64)
        sd = nat.SmxSocialDims()
        sd.dims_host, sd.n_ids = table.ctypes.data, int(table.shape[0])
        nat.check(self.lib, self.handle, self.lib.smx_set_social_history_dims(self.handle, C.byref(sd)), "smx_set_social_history_dims")
        self.history_dims = True

    def set_agent_dims(self, dims: Optional[np.ndarray]):
        """Bind per-agent vehicle dimensions (``smx_set_agent_dims``; the kinematic action spaces TargetPose,
        TrajectoryWithTime and Imitation only): host float64 ``(R, E, A, 3)`` — length, width, height of agent ``a`` of
        env ``e`` in episode ``k`` (row ``k mod R``), three NaNs = the sedan's box; ``A = N - num_social``.  The library
        copies the table.  An agent takes its triple where it is (re)spawned — the next ``reset``, a restart under
        ``auto_reset``, a history agent's placement — and keeps it until the next one; from then on its collisions, its
        ``on_shoulder`` / ``off_road`` corners, its ``off_route`` radius, its ego box row and its neighbours' lane ids are
        its own box's, and its env-mates see it in ``nb_box``, OGM, RGB and lidar.  ``None`` unbinds: sedans again from
        the next (re)spawn.  ``set_traffic_history`` keeps the binding.  Refused with the library's reason
        (``SmxError``): a dynamic action space, a component that is not finite, <= 0 or above its cap (length 10 m —
        the radius at which a neighbour's lane is searched, which answers the lookup within the observer's length —, width
        25 m, height 10 m), a triple that is partly NaN."""
        if dims is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_agent_dims(self.handle, None), "smx_set_agent_dims")
            self.agent_dims = None
            return
        table = _agent_dims_table(dims, self.E, self.N - self.cfg.num_social)
        ad = nat.SmxAgentDims()
        ad.dims_host, ad.rows = table.ctypes.data, int(table.shape[0])
        nat.check(self.lib, self.handle, self.lib.smx_set_agent_dims(self.handle, C.byref(ad)), "smx_set_agent_dims")
        self.agent_dims = table.copy()

    def set_agent_entry(self, ready_ticks: Optional[np.ndarray], check: Optional[np.ndarray] = None):
        """Bind delayed agent entry (``smx_set_agent_entry``; ``smarts_amd.missions.entry_table`` builds both tables):
        ``ready_ticks`` int32 ``(R, E, A)`` — the tick, counted from the reset observation, from which agent ``a`` of env
        ``e`` may enter in episode ``k`` (row ``k mod R``), at least one 0 per (row, env) — and ``check`` float64
        ``(R, E, A, 3)`` — the mission's start point (front bumper) and the new vehicle's largest plane dimension.  From
        the next ``reset`` on an agent at tick 0 enters with the reset; any other is pending (its rows an absent agent's)
        and enters in the first tick from its ready tick on in which no alive social vehicle overlaps its start point,
        with a first observation its env-mates see in that tick.  ``out["entry_status"]`` ``(E, N)`` uint8 holds
        ``ENTRY_PENDING / ENTRY_BLOCKED / ENTRY_ENTERED`` per agent and ``out["entered_tick"]`` ``(E, N)`` int32 the tick
        of its entry observation (-1 before).  Every launch form.  After a bind or unbind ``step`` is refused until a
        ``reset()`` of every env (no mask).  ``None`` unbinds (every agent enters at its
        next reset); so does a new map.  Refused with the library's reason (``SmxError``): a negative tick, a (row, env)
        without an agent at tick 0, a check row that is not finite or a dimension <= 0, history agents or a frame stack
        bound."""
        if ready_ticks is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_agent_entry(self.handle, None), "smx_set_agent_entry")
            self.agent_entry = None
            self.out.pop("entry_status", None)
            self.out.pop("entered_tick", None)
            return
        if check is None:
            raise ValueError("set_agent_entry needs the check table beside the ready ticks")
        ready, chk = _agent_entry_tables(ready_ticks, check, self.E, self.N - self.cfg.num_social)
        status = torch.full((self.E, self.N), nat.ENTRY_PENDING, dtype=torch.uint8, device=self.device)
        entered = torch.full((self.E, self.N), -1, dtype=torch.int32, device=self.device)
        en = nat.SmxAgentEntry()
        en.ready_host, en.check_host, en.rows = ready.ctypes.data, chk.ctypes.data, int(ready.shape[0])
        en.status_dev, en.status_count = status.data_ptr(), int(status.numel())
        en.entered_dev, en.entered_count = entered.data_ptr(), int(entered.numel())
        nat.check(self.lib, self.handle, self.lib.smx_set_agent_entry(self.handle, C.byref(en)), "smx_set_agent_entry")
        self.agent_entry = (ready.copy(), chk.copy())
        self.out["entry_status"] = status  # (written by every pass: they live as long as the binding)
        self.out["entered_tick"] = entered

    def set_agent_spaces(self, spaces: Optional[Sequence[str]]):
        """Bind per-agent action spaces (``smx_set_agent_spaces``): ``spaces[a]`` is the action space of agent slot ``a``
        in every env — any of Lane, Continuous, ActuatorDynamic, LaneWithContinuousSpeed, Trajectory and MPC, mixed
        freely.  While bound the tick is ``step_mixed``; ``step``, ``step_trajectory`` and the other uniform entries,
        ``actions_to_world`` and the kinematic bindings (history agents, handover, bubbles, agent dimensions) raise, and a
        large batch runs the teams cut.  No reset is needed; a slot that changes its space in the middle of an episode
        keeps controller state of its previous space's meaning, so a ``reset()`` after rebinding is recommended.
        ``None`` unbinds.  Refused with the library's reason (``SmxError``): a wrong length, a kinematic or unknown
        entry, a kinematic ``SimConfig.action_space``."""
        if spaces is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_agent_spaces(self.handle, None), "smx_set_agent_spaces")
            self.agent_spaces = None
            return
        codes = _agent_space_codes(list(spaces))
        sp = nat.SmxAgentSpaces()
        sp.space_host, sp.n_agents = codes.ctypes.data, len(codes)
        nat.check(self.lib, self.handle, self.lib.smx_set_agent_spaces(self.handle, C.byref(sp)), "smx_set_agent_spaces")
        self.agent_spaces = tuple(spaces)

    def step_mixed(self, lane: Optional[torch.Tensor] = None, floats: Optional[torch.Tensor] = None,
                   trajectories: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """One tick of a mixed fleet (``smx_step_mixed``; ``set_agent_spaces`` first).  Each buffer is laid out over all
        ``(E, N)`` vehicles as its uniform entry takes it, and a slot reads the buffer of its own space only: ``lane``
        int8 ``(E, N)`` codes for Lane slots (-1 = no action), ``floats`` float32 ``(E, N, 3)`` for Continuous /
        ActuatorDynamic / LaneWithContinuousSpeed slots (NaN first float = no action), ``trajectories`` float64
        ``(E, N, 4, 11)`` with ``counts`` int32 ``(E, N)`` for Trajectory / MPC slots (count 0 = no action).  The buffer
        of a space no slot has may be omitted; a missing buffer of a present space is a ``ValueError``."""
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        if self.agent_spaces is None:
            raise RuntimeError("step_mixed() without a table of agent spaces (set_agent_spaces)")
        present = set(self.agent_spaces)
        if "Lane" in present and lane is None:
            raise ValueError("the fleet holds Lane agents: step_mixed needs lane")
        if present & set(nat.FLOAT_SPACES) and floats is None:
            raise ValueError(f"the fleet holds {sorted(present & set(nat.FLOAT_SPACES))} agents: step_mixed needs floats")
        if present & {"Trajectory", "MPC"} and (trajectories is None or counts is None):
            raise ValueError("the fleet holds Trajectory / MPC agents: step_mixed needs trajectories and counts")
        acts = nat.SmxMixedActions()
        keep = []  # (the converted tensors live until the call is issued)
        for field, t, dtype, shape in (("lane_dev", lane, torch.int8, (self.E, self.N)),
                                       ("floats_dev", floats, torch.float32, (self.E, self.N, 3)),
                                       ("trajectories_dev", trajectories, torch.float64, (self.E, self.N, 4, nat.TRAJ_COLS)),
                                       ("counts_dev", counts, torch.int32, (self.E, self.N))):
            if t is None:
                continue
            if t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                t = t.to(device=self.device, dtype=dtype).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"step_mixed: {field[:-4]} must have shape {shape}, got {tuple(t.shape)}")
            keep.append(t)
            setattr(acts, field, t.data_ptr())
        return self._tick("smx_step_mixed", C.byref(acts))

    def set_history_agents(self, vehicle: Optional[torch.Tensor], expert_actions: bool = True):
        """Bind the history agents (``smx_set_history_agents``; needs ``action_space="Imitation"`` and a bound traffic
        history): agent slot ``a`` of env ``e`` follows recorded vehicle ``vehicle[k mod R, e, a]`` in episode ``k`` —
        int32 ``[R, E, A]`` on the sim's device, ``R`` the rows of the bound ``start_frames``, ``A = N - num_social``,
        < 0 = follows nothing; the tensor stays the caller's and is read by every pass (any value is safe).  From the
        next ``reset`` on a follower starts on its vehicle's row of the reset observation's frame, that vehicle is
        hidden from the env's social slots, and ``step_history_agents()`` moves every follower along the recording
        (``include/smx.h`` has the rules: leaving, never entering, the hand-over to ``step(actions)``).
        ``out["history_agent_status"]`` ``(E, N)`` uint8 holds ``HA_FOLLOWING / HA_LEFT / HA_ABSENT`` per agent and,
        with ``expert_actions``, ``out["expert_action"]`` ``(E, N, 3)`` float32 the Imitation action that takes the
        vehicle to its next recorded frame (NaN, NaN, 0: none), in the layout ``step`` takes.  ``vehicle=None``
        unbinds; so do ``set_traffic_history`` and a new map."""
        if vehicle is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_history_agents(self.handle, None), "smx_set_history_agents")
            self._drop_history_agents()
            return
        A = self.N - self.cfg.num_social
        if (vehicle.dtype != torch.int32 or vehicle.device != self.device or not vehicle.is_contiguous() or vehicle.ndim != 3
                or tuple(vehicle.shape[1:]) != (self.E, A) or vehicle.shape[0] < 1):
            raise ValueError(f"vehicle must be a contiguous int32 tensor of shape [R, {self.E}, {A}] on {self.device}")
        if self.history_start_frames is not None and vehicle.shape[0] != self.history_start_frames.shape[0]:
            raise ValueError(f"vehicle has {vehicle.shape[0]} rows, the bound start_frames {self.history_start_frames.shape[0]}")
        status = torch.full((self.E, self.N), nat.HA_ABSENT, dtype=torch.uint8, device=self.device)
        action = None
        if expert_actions:
            action = torch.full((self.E, self.N, 3), float("nan"), dtype=torch.float32, device=self.device)
            action[..., 2] = 0.0
        ha = nat.SmxHistoryAgents()
        ha.vehicle_dev, ha.vehicle_count = vehicle.data_ptr(), int(vehicle.numel())
        ha.status_dev, ha.status_count = status.data_ptr(), int(status.numel())
        if action is not None:
            ha.action_dev, ha.action_count = action.data_ptr(), int(action.numel())
        nat.check(self.lib, self.handle, self.lib.smx_set_history_agents(self.handle, C.byref(ha)), "smx_set_history_agents")
        self._drop_history_agents()
        self.history_agents = vehicle  # (read by every pass: lives as long as the binding)
        self.out["history_agent_status"] = status
        if action is not None:
            self.out["expert_action"] = action

    def _drop_history_agents(self):
        self.history_agents = None
        self.history_handover = None  # (the library drops the handover table with the follow table)
        self._drop_history_bubbles()  # (... and the bubbles)
        self.out.pop("history_agent_status", None)
        self.out.pop("expert_action", None)

    def step_history_agents(self) -> Dict[str, torch.Tensor]:
        """One tick in which every agent follows its recorded vehicle (``smx_step_history_agents``; no actions)."""
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        return self._tick("smx_step_history_agents")

    def set_history_handover(self, ticks: Optional[torch.Tensor]):
        """Bind the handover table (``smx_set_history_handover``; needs bound history agents): int32 ``[R, E, A]`` on the
        sim's device, indexed exactly as ``set_history_agents``' ``vehicle``.  In a ``step_history_handover(actions)``
        tick that starts with ``env_ticks[e] = t``, agent ``a`` of env ``e`` is driven by its action iff
        ``H = ticks[k mod R, e, a]`` has ``H >= 0 and t >= H``; otherwise it follows its recorded vehicle.  The tensor
        stays the caller's and is read by every such tick: rewriting it in place takes effect with the next one, and any
        value is safe.  ``step_history_agents()`` and ``step(actions)`` ignore it.  ``ticks=None`` unbinds; so does
        everything that drops the history agents."""
        if ticks is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_history_handover(self.handle, None), "smx_set_history_handover")
            self.history_handover = None
            return
        A = self.N - self.cfg.num_social
        if (ticks.dtype != torch.int32 or ticks.device != self.device or not ticks.is_contiguous() or ticks.ndim != 3
                or tuple(ticks.shape[1:]) != (self.E, A) or ticks.shape[0] < 1):
            raise ValueError(f"ticks must be a contiguous int32 tensor of shape [R, {self.E}, {A}] on {self.device}")
        if self.history_agents is not None and ticks.shape[0] != self.history_agents.shape[0]:
            raise ValueError(f"ticks has {ticks.shape[0]} rows, the bound follow table {self.history_agents.shape[0]}")
        ho = nat.SmxHistoryHandover()
        ho.tick_dev, ho.tick_count = ticks.data_ptr(), int(ticks.numel())
        nat.check(self.lib, self.handle, self.lib.smx_set_history_handover(self.handle, C.byref(ho)), "smx_set_history_handover")
        self.history_handover = ticks  # (read by every mixed tick: lives as long as the binding)

    def set_history_bubbles(self, bubbles):
        """Bind bubbles (``smx_set_history_bubbles``; needs bound history agents): a sequence of 1 .. ``MAX_BUBBLES``
        ``nat.SmxBubble`` — a rectangle ``size_x`` x ``size_y`` with an airlock ``margin`` around it, fixed at ``(x, y)``
        or travelling with agent slot ``follow_agent`` at ``(offset_x, offset_y)`` in its frame, ``hijack_limit`` /
        ``shadow_limit`` (0 = none).  Every ``step_history_handover(actions)`` tick then starts with the bubble pass
        (``include/smx.h`` has the rule): ``out["bubble_state"]`` ``(E, N)`` uint8 holds ``BUBBLE_SOCIAL / SHADOWED /
        HIJACKED / RELEASED`` per agent, ``out["bubble_cursor"]`` the per-bubble cursor bits.  A HIJACKED agent is driven
        by its action, a RELEASED one ends; no handover table is needed.  ``step_history_agents()`` and ``step(actions)``
        ignore the bubbles.  ``bubbles=None`` unbinds; so does everything that drops the history agents."""
        if bubbles is None:
            nat.check(self.lib, self.handle, self.lib.smx_set_history_bubbles(self.handle, None), "smx_set_history_bubbles")
            self._drop_history_bubbles()
            return
        bubbles = list(bubbles)
        state = torch.zeros((self.E, self.N), dtype=torch.uint8, device=self.device)
        cursor = torch.zeros((self.E, self.N), dtype=torch.uint8, device=self.device)
        hb = nat.SmxHistoryBubbles()
        host = (nat.SmxBubble * max(len(bubbles), 1))(*bubbles)
        hb.bubbles_host, hb.n_bubbles = host, len(bubbles)
        hb.state_dev, hb.state_count = state.data_ptr(), int(state.numel())
        hb.cursor_dev, hb.cursor_count = cursor.data_ptr(), int(cursor.numel())
        nat.check(self.lib, self.handle, self.lib.smx_set_history_bubbles(self.handle, C.byref(hb)), "smx_set_history_bubbles")
        self.history_bubbles = bubbles
        self.out["bubble_state"] = state  # (written by every mixed tick: they live as long as the binding)
        self.out["bubble_cursor"] = cursor

    def _drop_history_bubbles(self):
        self.history_bubbles = None
        self.out.pop("bubble_state", None)
        self.out.pop("bubble_cursor", None)

    def step_history_handover(self, actions: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One tick in which every agent follows its recorded vehicle or is driven by its row of ``actions`` — float32
        ``(E, N, 3)`` in ``step``'s Imitation layout — as the handover table and the bound bubbles say (``smx_step_history_handover``).
        Followers' and social rows of ``actions`` are ignored.  ``out["history_agent_status"]`` reads ``HA_DRIVEN`` for a
        driven agent and its ``out["expert_action"]`` row NaN, NaN, 0."""
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        if actions.dtype != torch.float32 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(actions.shape) != (self.E, self.N, 3):
            raise ValueError(f"actions must have shape {(self.E, self.N, 3)}, got {tuple(actions.shape)}")
        return self._tick("smx_step_history_handover", actions.data_ptr())

    history_agents = None
    history_handover = None
    history_bubbles = None
    history_dims = False
    agent_dims = None  # the bound (R, E, A, 3) table of set_agent_dims (a host copy), or None
    agent_entry = None  # the bound (ready ticks, check) tables of set_agent_entry (host copies), or None
    agent_spaces = None  # the bound per-slot action space names of set_agent_spaces, or None
    traffic_history = None
    history_start_frames = None
    history_replaced = None

    def bind_frame_stack(self, row: str, stack: Optional[torch.Tensor], layout: str = "frames"):
        """Bind the frame stack of ``out[row]`` (``smx_bind_frame_stack``; needs ``SimConfig(frame_stack=k)``): a
        contiguous device tensor of the row's dtype, ``[E, N, k, ...row shape]`` for ``layout="frames"`` or, for the
        image alone, ``[E, N, H, W, 3k]`` uint8 for ``layout="dstack"``; ``None`` unbinds.  The device keeps the last k
        frames of the row in it, newest first; ``out["stack_<row>"]`` (``out["rgb_dstack"]``) follows."""
        key = "rgb_dstack" if layout == "dstack" else "stack_" + row
        if layout not in nat.STACK_LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(nat.STACK_LAYOUTS)}")
        source, code = nat.stack_source(row), nat.STACK_LAYOUTS[layout]
        if stack is None:
            nat.check(self.lib, self.handle, self.lib.smx_bind_frame_stack(self.handle, source, code, None, 0), "smx_bind_frame_stack")
            self.out.pop(key, None)
            return
        if row not in self.out:
            raise ValueError(f"{row!r} is not a row of this configuration (its sensor is off)")
        if layout == "dstack" and row != "rgb":
            raise ValueError("layout='dstack' is the image's alone (row 'rgb')")
        k, src = self.cfg.frame_stack, self.out[row]
        want = (tuple(src.shape[:4]) + (3 * k,)) if layout == "dstack" else (self.E, self.N, k) + tuple(src.shape[2:])
        if not self.cfg.frame_stack:
            want = tuple(stack.shape)  # (the library refuses the bind: SMX_ERR_STATE)
        if stack.dtype != src.dtype or not stack.is_cuda or not stack.is_contiguous() or tuple(stack.shape) != want:
            raise ValueError(f"the {key} buffer must be a contiguous {src.dtype} device tensor of shape {want}")
        rc = self.lib.smx_bind_frame_stack(self.handle, source, code, stack.data_ptr(), int(stack.numel() * stack.element_size()))
        nat.check(self.lib, self.handle, rc, "smx_bind_frame_stack")
        self.out[key] = stack

    def small_form(self) -> bool:
        """Whether a tick runs in the SMALL launch form (smx_plan.h: SMX_LARGE_BATCH_VEHICLES)."""
        s = self.cfg.launch_strategy
        return s == "small" or (s == "auto" and self.E * self.N <= nat.LARGE_BATCH_VEHICLES)  # ("large*": never)

    def launch_form(self) -> str:
        """The form the library runs a tick in: "small", "large_teams" or "large_one_lane" (smx_launch_form)."""
        rc = self.lib.smx_launch_form(self.handle)
        if rc < 0:
            nat.check(self.lib, self.handle, rc, "smx_launch_form")
        return nat.LAUNCH_FORMS[rc]

    def handoff_bytes_per_agent_step(self) -> int:
        """Bytes written by one kernel of the tick and read by a later one (path seeds, road facts, next flags):
        reported beside the algorithmic bytes, never inside them."""
        return 2 * (nat.SEED_COUNT * 4 + nat.FACT_I_COUNT * 4 + nat.FACT_F_COUNT * 8) + nat.SEED_COUNT * 4

    def reset(self, env_mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        mask_ptr = None
        if env_mask is not None:
            env_mask = env_mask.to(device=self.device, dtype=torch.uint8).contiguous()
            assert env_mask.shape == (self.E,)
            mask_ptr = env_mask.data_ptr()
        rc = self.lib.smx_reset(self.handle, mask_ptr, C.byref(self._st), C.byref(self._sp), C.byref(self._out),
                                self._stream_ptr())
        nat.check(self.lib, self.handle, rc, "smx_reset")
        self._was_reset = True
        return self.out

    def step(self, actions: torch.Tensor) -> Dict[str, torch.Tensor]:
        if not self._was_reset:
            raise RuntimeError("step() before reset()")  # SMARTSNotSetupError (smarts.py:207-208)
        if self.cfg.action_space in ("Trajectory", "MPC"):
            raise ValueError(f"ActionSpaceType.{self.cfg.action_space} steps through step_trajectory(trajectories, counts)")
        if self.cfg.action_space == "TargetPose":
            raise ValueError("ActionSpaceType.TargetPose steps through step_target_pose(targets)")
        if self.cfg.action_space == "TrajectoryWithTime":
            raise ValueError("ActionSpaceType.TrajectoryWithTime steps through step_trajectory_with_time(trajectories, counts)")
        lane = self.cfg.action_space == "Lane"
        want_dtype, want_shape = (torch.int8, (self.E, self.N)) if lane else (torch.float32, (self.E, self.N, 3))
        if actions.dtype != want_dtype or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=want_dtype).contiguous()
        if tuple(actions.shape) != want_shape:
            raise ValueError(f"{self.cfg.action_space} actions must have shape {want_shape}, got {tuple(actions.shape)}")
        # Lane: codes outside -1..3 cannot be seen from here without a device round trip: the kernel treats them as
        # "no action" and smx_sync / BatchedSim.sync() reports them.  The float spaces: three floats per agent; NaN in
        # the first one = no action this tick (Imitation: acceleration, angular velocity, -; a NaN angular velocity =
        # the scalar form, the first float a speed to set)
        return self._tick("smx_step" if lane else "smx_step_continuous", actions.data_ptr())

    def _tick(self, entry: str, *args) -> Dict[str, torch.Tensor]:
        """Issue one step entry point of the library (``args``: what it takes between the handle and the state block).
        The call writes the next learner block (same extent and dtype as the other one); the blocks flip only when the
        library took the call: a refusal raises and leaves ``out["learner"]`` and ``next_learner_block`` as they were."""
        self._out.learner = self.next_learner_block.data_ptr()
        rc = getattr(self.lib, entry)(self.handle, *args, C.byref(self._st), C.byref(self._sp), C.byref(self._out),
                                      self._stream_ptr())
        if rc != 0:
            self._out.learner = self.out["learner"].data_ptr()
            nat.check(self.lib, self.handle, rc, entry)
        self._learner_k ^= 1
        self.out["learner"] = self._learner[self._learner_k]
        return self.out

    @property
    def next_learner_block(self) -> torch.Tensor:
        """The learner block the NEXT ``step`` will write (see ``RewardDoneGather.release``)."""
        return self._learner[self._learner_k ^ 1]

    def actions_to_world(self, space: str, actions: torch.Tensor, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Ego-frame actions -> world-frame actions on the device (``smx_actions_to_world``; the action half of the
        reference's ``get_egocentric_adapters``): ``actions`` in the layout ``step_trajectory`` / ``step_target_pose``
        / ``step_trajectory_with_time`` take, given in the frame of each agent's last observation
        (``out["ego_frame"]``).  Returns a new tensor of the same layout; agents without an observation yet
        (``out["ec_flags"] == 0``), without an action and social slots are copied through."""
        if not self.cfg.ego_centric:
            raise ValueError("actions_to_world needs SimConfig(ego_centric=True)")
        if space not in ("Trajectory", "MPC", "TargetPose", "TrajectoryWithTime"):
            raise ValueError(f"{space} actions hold no position or heading: they are the same in either frame")
        if space != self.cfg.action_space:
            raise ValueError(f"actions_to_world({space!r}) on a {self.cfg.action_space} batch")
        actions = actions.to(device=self.device, dtype=torch.float64).contiguous()
        want = {"Trajectory": (self.E, self.N, 4, nat.TRAJ_COLS), "MPC": (self.E, self.N, 4, nat.TRAJ_COLS),
                "TargetPose": (self.E, self.N, 4),
                "TrajectoryWithTime": (self.E, self.N, 5) + tuple(actions.shape[3:4])}[space]
        if tuple(actions.shape) != want or (space == "TrajectoryWithTime" and (actions.ndim != 4 or actions.shape[3] < 2)):
            raise ValueError(f"{space} actions must have shape {want}, got {tuple(actions.shape)}")
        counts_ptr = None
        if space != "TargetPose":
            if counts is None:
                raise ValueError(f"{space} actions come with counts")
            counts = counts.to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(counts.shape) != (self.E, self.N):
                raise ValueError(f"counts must have shape {(self.E, self.N)}, got {tuple(counts.shape)}")
            counts_ptr = counts.data_ptr()
        world = torch.empty_like(actions)
        rc = self.lib.smx_actions_to_world(self.handle, nat.ACTION_SPACES[space], actions.data_ptr(), counts_ptr,
                                           int(actions.shape[3]) if space == "TrajectoryWithTime" else 0, world.data_ptr(),
                                           C.byref(self._out), self._stream_ptr())
        nat.check(self.lib, self.handle, rc, "smx_actions_to_world")
        return world

    def step_trajectory(self, trajectories: torch.Tensor, counts: torch.Tensor,
                        ego_centric: bool = False) -> Dict[str, torch.Tensor]:
        """One tick in ActionSpaceType.Trajectory or ActionSpaceType.MPC: ``trajectories`` float64 [E, N, 4, 11] in the packed
        form of include/smx.h (``pack_trajectory``), ``counts`` int32 [E, N] (0 = no action).  ``ego_centric``: the
        trajectories are in the frame of each agent's last observation (``actions_to_world`` first)."""
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        if self.cfg.action_space not in ("Trajectory", "MPC"):
            raise ValueError("step_trajectory needs SimConfig(action_space='Trajectory') or 'MPC'")
        if ego_centric:
            trajectories = self.actions_to_world(self.cfg.action_space, trajectories, counts)
        trajectories = trajectories.to(device=self.device, dtype=torch.float64).contiguous()
        counts = counts.to(device=self.device, dtype=torch.int32).contiguous()
        assert trajectories.shape == (self.E, self.N, 4, nat.TRAJ_COLS) and counts.shape == (self.E, self.N)
        return self._tick("smx_step_trajectory", trajectories.data_ptr(), counts.data_ptr())

    def step_target_pose(self, targets: torch.Tensor, ego_centric: bool = False) -> Dict[str, torch.Tensor]:
        """One tick in ActionSpaceType.TargetPose: ``targets`` float64 [E, N, 4] = x, y, heading, seconds into the
        future at which the pose is wanted; NaN in x = no action this tick (include/smx.h).  ``ego_centric``: the
        poses are in the frame of each agent's last observation (``actions_to_world`` first)."""
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        if self.cfg.action_space != "TargetPose":
            raise ValueError("step_target_pose needs SimConfig(action_space='TargetPose')")
        if ego_centric:
            targets = self.actions_to_world("TargetPose", targets)
        targets = targets.to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(targets.shape) != (self.E, self.N, 4):
            raise ValueError(f"TargetPose actions must have shape {(self.E, self.N, 4)}, got {tuple(targets.shape)}")
        return self._tick("smx_step_target_pose", targets.data_ptr())

    def step_trajectory_with_time(self, trajectories: torch.Tensor, counts: torch.Tensor,
                                  ego_centric: bool = False) -> Dict[str, torch.Tensor]:
        """One tick in ActionSpaceType.TrajectoryWithTime: ``trajectories`` float64 [E, N, 5, T] with rows time, x,
        y, heading, speed, ``counts`` int32 [E, N] = points given (0 = no action).  A trajectory the reference
        raises on moves nothing and is reported by the next ``sync()``.  ``ego_centric``: rows x, y and heading are
        in the frame of each agent's last observation (``actions_to_world`` first)."""
        if not self._was_reset:
            raise RuntimeError("step() before reset()")
        if self.cfg.action_space != "TrajectoryWithTime":
            raise ValueError("step_trajectory_with_time needs SimConfig(action_space='TrajectoryWithTime')")
        if ego_centric:
            trajectories = self.actions_to_world("TrajectoryWithTime", trajectories, counts)
        trajectories = trajectories.to(device=self.device, dtype=torch.float64).contiguous()
        counts = counts.to(device=self.device, dtype=torch.int32).contiguous()
        if (trajectories.ndim != 4 or tuple(trajectories.shape[:3]) != (self.E, self.N, 5) or trajectories.shape[3] < 2
                or tuple(counts.shape) != (self.E, self.N)):
            raise ValueError(f"TrajectoryWithTime actions must have shapes {(self.E, self.N, 5, 'T >= 2')} and "
                             f"{(self.E, self.N)}, got {tuple(trajectories.shape)} and {tuple(counts.shape)}")
        return self._tick("smx_step_trajectory_with_time", trajectories.data_ptr(), counts.data_ptr(), int(trajectories.shape[3]))

    def set_timing(self, level):
        """0/False = off, 1/True = one event pair per smx_step, 2 = per-kernel phases."""
        nat.check(self.lib, self.handle, self.lib.smx_set_timing(self.handle, int(level)), "smx_set_timing")

    def read_phase_ms(self, max_steps: int = 16384) -> np.ndarray:
        """[steps, len(PHASES)] kernel-phase durations (ms) recorded at timing level 2."""
        k = len(nat.PHASES)
        buf = (C.c_float * (max_steps * k))()
        n = C.c_int32()
        rc = self.lib.smx_read_phase_ms(self.handle, buf, max_steps, C.byref(n))
        nat.check(self.lib, self.handle, rc, "smx_read_phase_ms")
        return np.frombuffer(buf, dtype=np.float32, count=n.value * k).reshape(n.value, k).copy()

    def last_step_ms(self) -> float:
        ms = C.c_float()
        nat.check(self.lib, self.handle, self.lib.smx_last_step_ms(self.handle, C.byref(ms)), "smx_last_step_ms")
        return float(ms.value)

    def read_step_ms(self, max_count: int = 65536) -> np.ndarray:
        """Durations (ms) of the smx_step launches recorded since timing was enabled / last read."""
        buf = (C.c_float * max_count)()
        n = C.c_int32()
        rc = self.lib.smx_read_step_ms(self.handle, buf, max_count, C.byref(n))
        nat.check(self.lib, self.handle, rc, "smx_read_step_ms")
        return np.frombuffer(buf, dtype=np.float32, count=n.value).copy()

    def sync(self):
        nat.check(self.lib, self.handle, self.lib.smx_sync(self.handle, self._stream_ptr()), "smx_sync")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.smx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # smarts.py:711-721
        try:
            self.close()
        except Exception:
            pass

"""The reference's ego-centric adapters (``smarts/core/utils/adapters/ego_centric_adapters.py``) over this package's
``Observation`` types: ``ego_centric_observation_adapter(obs)`` moves every position and heading of an observation into
the frame of the ego vehicle, and ``get_egocentric_adapters(action_space)`` pairs it with the action adapter that turns
Trajectory / TargetPose / TrajectoryWithTime (and MPC-shaped) actions given in that frame back into world coordinates
with the pose of the last UNMODIFIED observation (``_pair_adapters``, :284-303).  The arithmetic is
``ego_centric_rows``'s (the reference's own operations); the dense path computes the same on the device
(``SimConfig(ego_centric=True)``).

Where this differs from the reference, on purpose:
 - a TrajectoryWithTime action is time, x, y, heading, speed (trajectory_interpolation_provider.py:31-38): rows 1, 2, 3
   are converted; the reference's ``_trajectory_adaption`` (:195-212) reads rows 0, 1, 2 of any trajectory;
 - via positions are 2-D: the reference subtracts the 3-D ego position from them and raises; here they are
   transformed as the waypoints are (append 0, take ``[:2]``); a mission's 2-D goal position likewise;
 - a camera observation that is ``None`` stays ``None`` (the reference's ``_replace`` raises on it);
 - MultiTargetPose raises ``ValueError`` (the reference builds the error and never raises it, :269-275).
"""
from __future__ import annotations

import math
from dataclasses import is_dataclass
from dataclasses import replace as dc_replace
from typing import Any, Callable, Optional, Tuple

import numpy as np

from .agent_interface import ActionSpaceType
from .ego_centric_rows import position_to_ego_frame, world_position_from_ego_frame, wrap_value
from .observations import FixedRouteMission, Heading, Observation, PositionalGoal


def _replace(obj: Any, **kwargs):
    """adapter :40-57."""
    if is_dataclass(obj):
        return dc_replace(obj, **kwargs)
    if isinstance(obj, tuple) and hasattr(obj, "_fields"):
        return obj._replace(**kwargs)
    raise ValueError("Must be a namedtuple or dataclass.")


def ego_centric_observation_adapter(obs: Observation, *args: Any, **kwargs: Any) -> Observation:
    """adapter :60-176."""
    ego = obs.ego_vehicle_state
    position, heading = ego.position, ego.heading

    def ego_frame_dynamics(v):
        return None if v is None else np.array([np.linalg.norm(v[:2]), 0, *v[2:]])  # point to X

    def transform(v):
        return position_to_ego_frame(v, position, heading)

    def transform_2d(v):
        return transform(np.append(np.asarray(v, dtype=np.float64)[:2], [0]))[:2]

    def adjust_heading(h):
        return wrap_value(float(h) - heading, -math.pi, math.pi)

    def replace_wps(lwps):
        return [[_replace(wp, pos=np.array(transform_2d(wp.pos)), heading=Heading(adjust_heading(wp.heading)))
                 for wp in wps] for wps in lwps]

    def replace_via(via):
        return _replace(via, position=tuple(transform_2d(via.position)))

    def replace_metadata(cam):
        if cam is None:
            return None
        return _replace(cam, metadata=_replace(cam.metadata, camera_pos=(0, 0, 0), camera_heading_in_degrees=0))

    def replace_lidar(lidar):
        if not lidar:
            return lidar
        return ([np.array(transform(p)) for p in lidar[0]], lidar[1],
                [(np.array(transform(s)), np.array(transform(e))) for s, e in lidar[2]])

    mission = ego.mission
    if isinstance(mission, FixedRouteMission):  # start, goal (adapter :145-158); an endless mission holds neither
        goal = mission.goal
        if isinstance(goal, PositionalGoal):
            goal = _replace(goal, position=tuple(transform_2d(goal.position)))
        mission = _replace(mission, start_position=tuple(transform_2d(mission.start_position)),
                           start_heading=adjust_heading(mission.start_heading), goal=goal)
    vd = obs.via_data
    if vd:
        vd = _replace(vd, near_via_points=[replace_via(v) for v in vd.near_via_points],
                      hit_via_points=[replace_via(v) for v in vd.hit_via_points])
    rwps = obs.road_waypoints
    if rwps:
        rwps = _replace(rwps, lanes={lane_id: replace_wps(wps) for lane_id, wps in rwps.lanes.items()})
    nvs = obs.neighborhood_vehicle_states
    return _replace(
        obs,
        ego_vehicle_state=_replace(
            ego, position=np.array([0, 0, 0]), heading=Heading(0), linear_velocity=ego_frame_dynamics(ego.linear_velocity),
            linear_acceleration=ego_frame_dynamics(ego.linear_acceleration), linear_jerk=ego_frame_dynamics(ego.linear_jerk),
            mission=mission),
        neighborhood_vehicle_states=None if nvs is None else [
            _replace(nv, position=tuple(transform(nv.position)), heading=Heading(adjust_heading(nv.heading))) for nv in nvs],
        lidar_point_cloud=replace_lidar(obs.lidar_point_cloud),
        waypoint_paths=None if obs.waypoint_paths is None else replace_wps(obs.waypoint_paths),
        drivable_area_grid_map=replace_metadata(obs.drivable_area_grid_map),
        occupancy_grid_map=replace_metadata(obs.occupancy_grid_map),
        top_down_rgb=replace_metadata(obs.top_down_rgb),
        road_waypoints=rwps,
        via_data=vd,
    )


def _passthrough(act, _=None):
    """Continuous, ActuatorDynamic, Lane, LaneWithContinuousSpeed, Imitation (adapter :179-192, :278-281)."""
    return act


def _trajectory_adaption(act, last_obs: Observation, first_row: int = 0):
    """adapter :195-212 on rows ``first_row`` .. ``first_row + 2`` (x, y, heading); the other rows are kept."""
    ego = last_obs.ego_vehicle_state
    xs, ys, hs = act[first_row], act[first_row + 1], act[first_row + 2]
    new_pos = np.array([world_position_from_ego_frame([x, y, 0], ego.position, ego.heading)[:2] for x, y in zip(xs, ys)]).T
    new_headings = np.array([wrap_value(float(h) + ego.heading, -math.pi, math.pi) for h in hs])
    return (*act[:first_row], *new_pos, new_headings, *act[first_row + 3:])


def _trajectory_adapter(act, last_obs: Optional[Observation] = None):
    return _trajectory_adaption(act, last_obs) if last_obs else act


def _trajectory_with_time_adapter(act, last_obs: Optional[Observation] = None):
    return _trajectory_adaption(act, last_obs, first_row=1) if last_obs else act


def _target_pose_adapter(act: Tuple[float, float, float, float], last_obs: Optional[Observation] = None):
    """adapter :248-266."""
    if not last_obs:
        return act
    ego = last_obs.ego_vehicle_state
    out_pos = world_position_from_ego_frame(np.append(act[:2], [0]), ego.position, ego.heading)
    return np.array([*out_pos[:2], wrap_value(ego.heading + act[2], -math.pi, math.pi), act[3]])


def _multi_target_pose_adapter(act, last_obs: Optional[Observation] = None):
    raise ValueError("Ego-centric assumes single vehicle and is ambiguous with multi-target-pose.")


def _pair_adapters(observation_adapter: Callable[[Observation], Observation],
                   action_adapter: Callable[[Any, Optional[Observation]], Any]):
    """Wrapper that shares the state between both adapters (adapter :284-303)."""
    last_obs = None

    def oa_wrapper(obs: Observation):
        nonlocal last_obs
        last_obs = obs  # the unmodified observation
        return observation_adapter(obs)

    def aa_wrapper(act: Any):
        return action_adapter(act, last_obs)

    return oa_wrapper, aa_wrapper


def get_egocentric_adapters(action_space: ActionSpaceType):
    """(observation adapter, action adapter) that share the last unmodified observation, so that the action adapter
    converts back to world space (adapter :306-325)."""
    m = {
        ActionSpaceType.Continuous: _passthrough, ActionSpaceType.ActuatorDynamic: _passthrough,
        ActionSpaceType.Lane: _passthrough, ActionSpaceType.LaneWithContinuousSpeed: _passthrough,
        ActionSpaceType.Trajectory: _trajectory_adapter, ActionSpaceType.TrajectoryWithTime: _trajectory_with_time_adapter,
        ActionSpaceType.MPC: _trajectory_adapter, ActionSpaceType.TargetPose: _target_pose_adapter,
        ActionSpaceType.MultiTargetPose: _multi_target_pose_adapter, ActionSpaceType.Imitation: _passthrough,
    }
    return _pair_adapters(ego_centric_observation_adapter, m[action_space])

// smx_kernels.hip — the per-tick kernels of the SMARTS hot path on gfx950, and the C-ABI.
//
// A tick = SMARTS._step (smarts.py:236-327) for every environment instance of the shard, as a short
// sequence of kernels on one stream (each stage has its own natural thread mapping; together
// they stay far below the register pressure of one fused kernel):
//
//   k_control   4 lanes / vehicle       A controllers (_perform_agent_actions, smarts.py:1233-1263):
//                                         the team finds the controller's waypoint path together
//                                       B physics     (_step_pybullet, smarts.py:923-931)
//   k_scan      8 lanes / vehicle       map sweeps at the new pose: nearest lane / road_with_point
//                                       at centre + 4 corners, lane heading (wrong way); 10 nearest
//                                       lanepoints, path seeds
//   k_sensors   workgroup roles         waypoints role  4 lanes / vehicle: waypoint paths streamed
//                                         into the dense rows, trip meter / reward
//                                       observe role    1 lane / vehicle, whole envs / workgroup:
//                                         collisions, neighbours, ego block, accelerometer, driven
//                                         path, events, done
//                                       lidar / OGM roles  1 wavefront / vehicle
//   k_tail      1 lane / vehicle        new flags (teardown), dones["__all__"], auto-reset respawn,
//                                       the new vehicles' grid tiles, the next tick's alive list
//
// followed, for envs whose episode ended under auto_reset (parallel_env.py:303-309), by k_first: scan /
// sensors / commit restricted to the re-created vehicles.  Above 16384 vehicles every role is
// launched on its own (k_waypoints, k_observe, k_lidar, k_ogm; see enqueue()).  Envs are independent
// (reference: one process per env, parallel_env.py:96-122): no inter-workgroup communication.
//
// Three phases are in headers of their own so far, included below: smx_k_scan.h (k_scan and its listed forms),
// smx_k_grids.h (OGM / DAGM / RGB roles, k_ogm, k_dagm, k_rgb) and smx_k_lidar.h (lidar role, k_lidar, k_lidar_first);
// what the phases share is in smx_tick.h.  The other phases follow.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "smx_bubbles.h"
#include "smx_guard.h"
#include "smx_handle.h"
#include "smx_history.h"
#include "smx_host.h"
#include "smx_k_grids.h"
#include "smx_k_lidar.h"
#include "smx_k_scan.h"
#include "smx_k_entry.h"  // (after smx_k_scan.h: its large-form instance runs the facts half for an entrant)
#include "smx_plan.h"
#include "smx_scan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

// =================================================================================
// k_control: controllers (a1-a3) + vehicle dynamics (a4-a6), SMX_WP_LANES lanes per vehicle.
// The controller's waypoint query (lane_following_controller.py:96-98) is the long part: the team
// walks the candidate paths together — lane p synthesises path p, every lane measures the first
// waypoint of the paths it owns (find_current_lane :367-374) — then the wanted path moves to
// lane 0 through shuffles and lane 0 runs the control law and the 24 physics substeps.
// =================================================================================

// ---- the steps every launch form of the controller shares (k_control, k_control_paths / k_control_law,
// k_control_fast / k_control_listed, k_control_kinematic), each written once

// Controllers.perform_action's decoding of a Lane / LaneWithContinuousSpeed action (controllers/__init__.py:113-144),
// on action words its caller has loaded (`action` for Lane, act0 / act1 for the other).  Without an action the other
// fields mean nothing and are not read.  (The Lane fields are selects on the code, outside any branch, so that
// they can sink below k_control's path search: behind the has-action branch k_control<0, true> took 231 registers
// for 225; the other space's are left unset without an action: zero-filled, k_control_law<3> took 188 for 186 —
// profiles/r09_controller_shared_steps.txt.)
struct LaneAction {
  bool has_action;
  double target_speed, hg, lg;
  int lane_change;
};
template <int SPACE>
__device__ __forceinline__ LaneAction decode_lane_action(const KernelArgs& a, int action, float act0, float act1) {
  LaneAction la;
  la.has_action = false;
  if (SPACE == SMX_ACTION_SPACE_LANE) {
    // the reference looks the action string up in a dict and raises (:137-144); a code that names no action is
    // reported at the next smx_sync and moves nothing
    const bool bad_code = action < SMX_ACTION_NONE || action > SMX_ACTION_CHANGE_LANE_RIGHT;
    if (bad_code) atomicOr(a.status, SMX_DEVICE_BAD_LANE_ACTION);
    la.has_action = !bad_code && action >= 0;
    // :125-144
    la.target_speed = action == SMX_ACTION_KEEP_LANE ? 15.0 : (action == SMX_ACTION_SLOW_DOWN ? 0.0 : 12.5);
    la.lane_change = action == SMX_ACTION_CHANGE_LANE_LEFT ? 1 : (action == SMX_ACTION_CHANGE_LANE_RIGHT ? -1 : 0);
    la.hg = la.target_speed > 0.0 ? a.heading_gain_pos : 0.01;
    la.lg = la.target_speed > 0.0 ? a.lateral_gain_pos : 0.36;
  } else if (!(act0 != act0)) {  // NaN = no action
    // :113-124: (target_speed, lane_change)
    la.has_action = true;
    la.target_speed = (double)act0;
    la.lane_change = lane_change_of_action(act1);
    lateral_gains_for_speed(la.target_speed, la.hg, la.lg);
  }
  return la;
}
template <int SPACE>
__device__ __forceinline__ LaneAction load_lane_action(const KernelArgs& a, size_t gid) {
  if (SPACE == SMX_ACTION_SPACE_LANE) return decode_lane_action<SPACE>(a, a.actions[gid], 0.f, 0.f);
  return decode_lane_action<SPACE>(a, SMX_ACTION_NONE, a.actions_f32[gid * 3 + 0], a.actions_f32[gid * 3 + 1]);
}

// No action this tick: wheel torques do not persist, the steer motor target does.
__device__ __forceinline__ ControlOut idle_command(const CtrlState& cs) {
  ControlOut co;
  co.throttle = 0.0;
  co.brake = 0.0;
  co.steering = cs.steer;
  return co;
}
// The reference asserts "no waypoints found"; keep the last command.
__device__ __forceinline__ ControlOut last_command(const CtrlState& cs) {
  ControlOut co;
  co.throttle = cs.throttle;
  co.brake = 0.0;
  co.steering = cs.steer;
  return co;
}

// The Continuous / ActuatorDynamic command (controllers/__init__.py:94-99).
template <int SPACE>
__device__ __forceinline__ ControlOut direct_command(float act0, float act1, float act2, CtrlState& cs, double dt) {
  ControlOut co;
  co.throttle = clip_ref((double)act0, 0.0, 1.0);
  co.brake = clip_ref((double)act1, 0.0, 1.0);
  if (SPACE == SMX_ACTION_SPACE_CONTINUOUS) {
    co.steering = clip_ref((double)act2, -1.0, 1.0);
  } else {
    // ActuatorDynamicController.perform_action (actuator_dynamic_controller.py:47-80): the third
    // component is a steering *rate*; the held angle is the controller state
    const double change = clip_ref((double)act2, -1.0, 1.0);
    co.steering = clip_ref((1.0 - 0.001) * cs.steer + change * dt, -1.0, 1.0);
  }
  cs.steer = co.steering;  // last_steering_angle / the persisting steer target
  return co;
}

// ---- team helpers: SMX_WP_LANES lanes per vehicle
__device__ __forceinline__ int team_or(int v) {
#pragma unroll
  for (int msk = SMX_WP_LANES / 2; msk >= 1; msk >>= 1) v |= __shfl_xor(v, msk, SMX_WP_LANES);
  return v;
}

// exclusive prefix of `cnt` over the team: the sum over the lanes below p0; `total`: the sum over the whole team
__device__ __forceinline__ int team_exclusive_prefix(int cnt, int p0, int& total) {
  int incl = cnt;
  int t = __shfl_up(incl, 1, SMX_WP_LANES);
  if (p0 >= 1) incl += t;
  t = __shfl_up(incl, 2, SMX_WP_LANES);
  if (p0 >= 2) incl += t;
  total = __shfl(incl, SMX_WP_LANES - 1, SMX_WP_LANES);
  return incl - cnt;
}

// nearest path over the team: smallest distance, then smallest number
__device__ __forceinline__ void team_nearest(double& my_d, int& my_idx) {
#pragma unroll
  for (int msk = SMX_WP_LANES / 2; msk >= 1; msk >>= 1) {
    const double od = __shfl_xor(my_d, msk, SMX_WP_LANES);
    const int oi = __shfl_xor(my_idx, msk, SMX_WP_LANES);
    if (od < my_d || (od == my_d && oi < my_idx)) {
      my_d = od;
      my_idx = oi;
    }
  }
}

// wp_paths[clip(current_lane + lane_change)] (lane_following_controller.py:100-103)
__device__ __forceinline__ int wanted_path(int nearest, int lane_change, int n_paths) {
  const int want = nearest + lane_change;
  return want < 0 ? 0 : (want > n_paths - 1 ? n_paths - 1 : want);
}

// The team's search of the candidate paths (find_current_lane, lane_following_controller.py:367-374).
// Paths are numbered in the reference's order: seed lanes by index, branches depth-first.
// Team lane p walks seed lanes p, p + 4, ... on its own (no lane re-walks another lane's
// paths) and measures the first waypoint of every path it meets; counts are exchanged by shuffles
// to turn (lane, branch) into the global number.  FUSED: the first branch of the lane's first seed
// lane is synthesised in full through `put` while it is walked (n_first waypoints).
struct TeamSearch {
  int n_paths;      // of the whole team
  double my_d;      // this lane's nearest first waypoint and its path's number (team_nearest: the team's)
  int my_idx;
  int goff0, cnt0;  // the paths of this lane's first seed lane: number of the first one, how many
  int n_first;
};
template <bool FUSED, class Put>
__device__ __forceinline__ TeamSearch team_path_search(const MapDev& m, const PathSeeds& seed, int p0, double px, double py,
                                                       int* knots, Put&& put) {
  TeamSearch ts;
  ts.n_paths = 0;
  ts.my_d = SMX_INF;
  ts.my_idx = 0x7fffffff;
  ts.goff0 = ts.cnt0 = ts.n_first = 0;
  if (seed.road < 0) return ts;
  for (int r4 = 0; r4 < seed.n_lanes; r4 += SMX_WP_LANES) {  // uniform within a team
    const int li = r4 + p0;
    int cnt = 0, bj = 0x7fffffff;
    double bd = SMX_INF;
    if (li < seed.n_lanes) {
      const int start = seed_start(m, seed, li, px, py);
      if (start >= 0) {
        BranchState bs;
        bs.reset();
        do {
          double fx = 0.0, fy = 0.0;
          if (FUSED && r4 == 0 && cnt == 0) {
            ts.n_first = equally_spaced_path(m, seed.f, bs, start, SMX_CTRL_WPS - 1, px, py, knots, SMX_BLOCK,
                                             SMX_CTRL_WPS, [&](int i, const WaypointOut& w) {
                                               put(i, w);
                                               if (i == 0) {
                                                 fx = w.x;
                                                 fy = w.y;
                                               }
                                             });
          } else {
            equally_spaced_path(m, seed.f, bs, start, SMX_CTRL_WPS - 1, px, py, knots, SMX_BLOCK, 1,
                                [&](int, const WaypointOut& w) {
                                  fx = w.x;
                                  fy = w.y;
                                });
          }
          const double ex = fx - px, ey = fy - py;
          const double d = sqrt(ex * ex + ey * ey);
          if (d < bd) {  // strict: the lowest-numbered path wins ties (np.argmin)
            bd = d;
            bj = cnt;
          }
          ++cnt;
        } while (bs.advance());
      }
    }
    int round_total;
    const int g = ts.n_paths + team_exclusive_prefix(cnt, p0, round_total);
    if (r4 == 0) {
      ts.goff0 = g;
      ts.cnt0 = cnt;
    }
    if (bj != 0x7fffffff && (bd < ts.my_d || (bd == ts.my_d && g + bj < ts.my_idx))) {
      ts.my_d = bd;
      ts.my_idx = g + bj;
    }
    ts.n_paths += round_total;
  }
  return ts;
}

// Branch `branch` of seed lane `li`, walked to again and synthesised through `put` (rare in k_control: branching
// inside 16 hops).  Returns its waypoints.
template <class Put>
__device__ __forceinline__ int rewalk_branch(const MapDev& m, const PathSeeds& seed, int li, double px, double py, int branch,
                                             int* knots, Put&& put) {
  const int start = seed_start(m, seed, li, px, py);
  BranchState bs;
  bs.reset();
  int j = 0;
  do {
    if (j == branch) return equally_spaced_path(m, seed.f, bs, start, SMX_CTRL_WPS - 1, px, py, knots, SMX_BLOCK, SMX_CTRL_WPS, put);
    equally_spaced_path(m, seed.f, bs, start, SMX_CTRL_WPS - 1, px, py, knots, SMX_BLOCK, 0, [&](int, const WaypointOut&) {});
    ++j;
  } while (bs.advance());
  return 0;
}

// ---- reuse of the knot lists the waypoints sensor walked last tick (control_paths_for explains it)

// Is the list walked for this start lanepoint and route filter, without a branching, and not empty?
__device__ __forceinline__ bool knot_list_reusable(int key0, int key1, int key2, int cnt, int n32, int start, const RouteFilter& f) {
  return key0 == start && key1 == (f.n > 0 ? f.road[0] : -1) && key2 == (f.n > 1 ? f.road[1] : -1) && cnt == 1 && n32 > 0;
}

// Distance to the first waypoint of a seed lane's paths: the projection of the vehicle on the start lanepoint's
// heading line (interpolate_knots at t = 0), the lanepoint itself on a path of one lanepoint.
__device__ __forceinline__ double first_waypoint_distance(double rx, double ry, double rdx, double rdy, int n32, double px, double py) {
  const double proj = (px - rx) * rdx + (py - ry) * rdy;
  const double fx = n32 == 1 ? rx : rx + proj * rdx, fy = n32 == 1 ? ry : ry + proj * rdy;
  const double ex = fx - px, ey = fy - py;
  return sqrt(ex * ex + ey * ey);
}

// The controller's n16 waypoints of knot list `pth` (start record r0, nk16 knots, `last` the last knot when it is
// not one of the list's): knots into registers (every load in flight together), their arclength in path order
// (pass 1's additions), then the interpolation through `put`.  ONE_LANE is k_control_fast's form: the knot numbers
// are loaded whatever nk16 is, and lane, width and speed limit of the waypoints (not the controller's business) are
// left 0.
template <bool ONE_LANE, class Put>
__device__ __forceinline__ void ctrl_waypoints_from_knots(const KernelArgs& a, const int32_t* knot1, size_t kstride, const smx_lp_rec& r0,
                                                          int nk16, int last, int n16, double px, double py, Put&& put) {
  // (knot k + 1 of the list is knot1[k * kstride]: a column of KnotLists::idx, or a row of the knot table)
  const MapDev& m = a.map;
  auto fetch = [&](int k) { return (k == nk16 - 1 && last >= 0) ? last : knot1[(size_t)k * kstride]; };
  constexpr int KP = SMX_WPT_PRELOAD;
  double kx[KP], ky[KP], kh[KP], kw[KP], ks_[KP];
  int kl[KP];
  {
    int kid[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (ONE_LANE) {
        const int id = knot1[(size_t)k * kstride];  // (in range whatever nk16 is)
        kid[k] = (k == nk16 - 1 && last >= 0) ? last : id;
      } else {
        kid[k] = k < nk16 ? fetch(k) : 0;
      }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const bool have = k < nk16;
      const smx_lp_rec* r = m.lp_rec + (have ? kid[k] : 0);
      kx[k] = have ? r->x : 0.0;
      ky[k] = have ? r->y : 0.0;
      kh[k] = have ? r->heading : 0.0;
      kl[k] = (have && !ONE_LANE) ? r->lane : 0;
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const bool ask = !ONE_LANE && k < nk16 && kl[k] != (k == 0 ? (int)r0.lane : kl[k > 0 ? k - 1 : 0]);
      kw[k] = ask ? m.lane_width[kl[k]] : 0.0;
      ks_[k] = ask ? m.lane_speed[kl[k]] : 0.0;
    }
  }
  double D = 0.0;
  {
    const double proj = (px - r0.x) * r0.dirx + (py - r0.y) * r0.diry;
    double lastx = r0.x + proj * r0.dirx, lasty = r0.y + proj * r0.diry;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (k < nk16) {
        const double ex = kx[k] - lastx, ey = ky[k] - lasty;
        D += sqrt(ex * ex + ey * ey);
        lastx = kx[k];
        lasty = ky[k];
      }
    }
    for (int k = KP; k < nk16; ++k) {
      const smx_lp_rec* r = m.lp_rec + fetch(k);
      const double qx = r->x, qy = r->y;
      const double ex = qx - lastx, ey = qy - lasty;
      D += sqrt(ex * ex + ey * ey);
      lastx = qx;
      lasty = qy;
    }
  }
  interpolate_knots_preloaded<KP>(m, r0, ONE_LANE ? 0.0 : m.lane_width[r0.lane], ONE_LANE ? 0.0 : m.lane_speed[r0.lane], nk16, n16, D,
                                  px, py, SMX_CTRL_WPS, kx, ky, kh, kl, kw, ks_, fetch, put);
}

// One instantiation per action space: the Lane kernel does not carry the registers of the others.
// waves_per_eu(2): at most 256 registers, so that two wavefronts share a SIMD on large batches.
// LDS_PATH (small batches, lane-following spaces): the candidate path is written to LDS as it is
// synthesised and read back with fixed indices by the lane that runs the control law.  In registers a
// put at a run-time index is a 17-way compare / select chain over every live element (~90
// instructions per waypoint); the LDS copy costs 26 KB per workgroup, which would halve the
// wavefronts per CU on large batches, so those keep the register form.
// GUARD (every control kernel and k_reset / k_tail): the state guard as a compile-time choice — the plan launches the
// GUARD instantiation while a guard buffer is bound, and the other one is the kernel without a guard, word for word.
// (the role: team lane threadIdx.x % SMX_WP_LANES of vehicle `gid`; k_control takes the vehicles in batch order,
// k_control_slots — the tick of a mixed fleet — the slots of one action space)
template <int SPACE, bool LDS_PATH, bool GUARD>
__device__ __forceinline__ void control_one_for(const KernelArgs& a, const size_t gid, int* knots, double* path_lds) {
  // element (waypoint i, component q) of this lane's path: consecutive lanes, consecutive words
  auto path_put = [&](CtrlPath& p, int i, double x, double y, double h) {
    if (LDS_PATH) {
      double* q = path_lds + (size_t)(i * 3) * SMX_BLOCK + threadIdx.x;
      q[0] = x;
      q[SMX_BLOCK] = y;
      q[2 * SMX_BLOCK] = h;
    } else {
      ctrl_path_put(p, i, x, y, h);
    }
  };
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const int p0 = threadIdx.x % SMX_WP_LANES;
  if (gid >= total) return;  // whole teams leave together
  int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE)) return;
  if (flags & SMX_F_SOCIAL) {
    if (p0 == 0)
      social_vehicle_step(a, gid, total, SF(SMX_S_MCL_X), SF(SMX_S_MCL_Y), SF(SMX_S_SPD_INT), SF(SMX_S_THROTTLE), SF(SMX_S_X), SF(SMX_S_Y));
    return;
  }
  SMX_TSTAMP(tc0);
  VehState s = load_vehicle(a, gid, total);
  if constexpr (GUARD) {
    const GuardVerdict gv = guard_at_load(a, flags, s);  // (the same for the team's four lanes)
    if (gv.action != GUARD_STORE) {
      if (p0 == 0) guard_refuse(a, gid, total, flags, gv);
      return;
    }
  }
  CtrlState cs = load_ctrl_state(a, gid, total, flags);
  // ---- Controllers.perform_action (controllers/__init__.py:61-152)
  constexpr int space = SPACE;
  constexpr bool lane_following =
      space == SMX_ACTION_SPACE_LANE || space == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED;
  constexpr bool tracking = space == SMX_ACTION_SPACE_TRAJECTORY || space == SMX_ACTION_SPACE_MPC;  // packed trajectories
  LaneAction la = LaneAction{};
  float act0 = 0.f, act1 = 0.f, act2 = 0.f;
  bool has_action;
  if (lane_following) {
    la = load_lane_action<SPACE>(a, gid);
    has_action = la.has_action;
  } else if (tracking) {
    has_action = a.traj_n[gid] > 0;
  } else {
    act0 = a.actions_f32[gid * 3 + 0];
    act1 = a.actions_f32[gid * 3 + 1];
    act2 = a.actions_f32[gid * 3 + 2];
    has_action = !(act0 != act0);  // NaN = no action
  }
  int act_lane = 0;  // the team lane that runs the control law and the physics (uniform in the team)
  ControlOut co = idle_command(cs);
  if (has_action && tracking) {
    if (p0 == 0) {
      PackedTraj t;
      t.p = a.traj + gid * (size_t)(4 * SMX_TRAJ_COLS);
      t.n = a.traj_n[gid];
      co = space == SMX_ACTION_SPACE_MPC ? trajectory_tracking_mpc(s, cs, c.dt, t) : trajectory_tracking_pd(s, cs, c.dt, t);
    }
  } else if (has_action && !lane_following) {
    co = direct_command<SPACE>(act0, act1, act2, cs, c.dt);
  }
  if (has_action && lane_following && !SMX_SKIP(a, 1)) {  // uniform within a team
    const double target_speed = la.target_speed, hg = la.hg, lg = la.lg;
    const int lane_change = la.lane_change;
    const PathSeeds seed = load_seeds(a, gid, total);  // found by k_scan at this very pose
    const double px = s.x, py = s.y;
    CtrlPath path;
    path.n = 0;
#pragma unroll
    for (int k = 0; k < SMX_CTRL_WPS; ++k) path.x[k] = path.y[k] = path.h[k] = 0.0;
    SMX_TSTAMP(tc1);
    SMX_TACC(15, tc0, tc1);
    TeamSearch ts = team_path_search<true>(m, seed, p0, px, py, knots,
                                           [&](int i, const WaypointOut& w) { path_put(path, i, w.x, w.y, w.heading); });
    path.n = ts.n_first;
    const int n_paths = ts.n_paths, goff0 = ts.goff0, cnt0 = ts.cnt0;
    SMX_TSTAMP(tc2);
    SMX_TACC(16, tc1, tc2);
    team_nearest(ts.my_d, ts.my_idx);
    if (n_paths > 0) {  // uniform within a team
      const int want = wanted_path(ts.my_idx, lane_change, n_paths);
      // the lane whose first seed lane holds path `want`
      const bool own = cnt0 > 0 && want >= goff0 && want < goff0 + cnt0;
      if (own && want > goff0)  // a later branch of this lane's seed lane
        path.n = rewalk_branch(m, seed, p0, px, py, want - goff0, knots,
                               [&](int i, const WaypointOut& w) { path_put(path, i, w.x, w.y, w.heading); });
      const int owners = team_or(own ? (1 << p0) : 0);
      // the lane that holds the wanted path carries on alone (control law, physics, state write):
      // nothing moves between lanes and no second copy of the path is kept in registers
      act_lane = owners ? (__ffs(owners) - 1) : 0;
      SMX_TSTAMP(tc3);
      SMX_TACC(17, tc2, tc3);
      if (p0 == act_lane) {
        if (LDS_PATH) {
#pragma unroll
          for (int k = 0; k < SMX_CTRL_WPS; ++k) {
            const double* q = path_lds + (size_t)(k * 3) * SMX_BLOCK + threadIdx.x;
            const bool held = k < path.n;
            path.x[k] = held ? q[0] : 0.0;
            path.y[k] = held ? q[SMX_BLOCK] : 0.0;
            path.h[k] = held ? q[2 * SMX_BLOCK] : 0.0;
          }
        }
        // beyond the team's first seed lanes (roads with more than 4 lanes): serial search
        if (!owners)
          path.n = ctrl_path_serial(m, seed, px, py, want, knots, SMX_BLOCK,
                                    [&](int i, const WaypointOut& w) { ctrl_path_put(path, i, w.x, w.y, w.heading); });
        if (!SMX_SKIP(a, 1048576)) co = lane_following_from_path(s, cs, c.dt, target_speed, lane_change, hg, lg, path);
      }
      SMX_TSTAMP(tc4);
      SMX_TACC(18, tc3, tc4);
    } else {
      co = last_command(cs);
    }
  }
  if (p0 != act_lane) return;
  SMX_TSTAMP(tc5);
  SF(SMX_S_PREV_X) = s.x;  // the position recorded by the previous observation
  SF(SMX_S_PREV_Y) = s.y;
  if (!SMX_SKIP(a, 2097152)) vehicle_step(s, co, c.dt);
  SMX_TSTAMP(tc6);
  SMX_TACC(19, tc5, tc6);
  if constexpr (GUARD)
    if (!guard_before_store(a, gid, flags, s)) return;
  store_vehicle_state(a, gid, total, s, cs, flags);
  SMX_TSTAMP(tc7);
  SMX_TACC(20, tc0, tc7);
}

template <int SPACE, bool LDS_PATH = false, bool GUARD = false>
__global__ void __attribute__((amdgpu_waves_per_eu(2, 8))) __launch_bounds__(SMX_BLOCK) k_control(const KernelArgs a) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  __shared__ double path_lds[LDS_PATH ? 3 * SMX_CTRL_WPS * SMX_BLOCK : 1];
  control_one_for<SPACE, LDS_PATH, GUARD>(a, ((size_t)blockIdx.x * SMX_BLOCK + threadIdx.x) / SMX_WP_LANES, knot_scratch + threadIdx.x, path_lds);
}

// The slots of ONE action space in a mixed fleet (smx_set_agent_spaces; the small form's tick of smx_step_mixed): team t
// of the launch works on slot slots[t % n_slots] of env t / n_slots, so every wavefront is full of that space's agents
// and an agent of another space costs the launch nothing.  The list of the space that owns the social slots ends with
// them (smx_handle.h AgentSpacesDev): the role steps them as k_control does.
struct SlotList {
  const int32_t* slots;  // [n_slots] ascending slots of an env
  int32_t n_slots;
};
template <int SPACE, bool GUARD = false>
__global__ void __attribute__((amdgpu_waves_per_eu(2, 8))) __launch_bounds__(SMX_BLOCK) k_control_slots(const KernelArgs a, const SlotList sl) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  const size_t total = (size_t)a.cfg.num_envs * a.cfg.num_vehicles;
  const size_t team = ((size_t)blockIdx.x * SMX_BLOCK + threadIdx.x) / SMX_WP_LANES;
  const size_t env = team / (size_t)sl.n_slots;
  // (past the last env: no vehicle — the role's own test; the slot is loaded from inside the list either way)
  const size_t gid = env < (size_t)a.cfg.num_envs ? env * a.cfg.num_vehicles + (size_t)sl.slots[team % (size_t)sl.n_slots] : total;
  control_one_for<SPACE, false, GUARD>(a, gid, knot_scratch + threadIdx.x, nullptr);
}

// =================================================================================
// Large batches: the controller as two launches.  In k_control the control law and the 24 physics substeps
// run on ONE lane of each vehicle's team of four (154 of its 223 us at 131 k vehicles, three quarters of the
// lanes masked off).  Here k_control_paths keeps the team work — candidate paths, nearest path, the wanted
// path written as 17 waypoints to a hand-off in device memory, laid out [waypoint][component][vehicle] —
// and k_control_law runs law + physics with one lane per vehicle: a quarter of the wavefronts, every lane
// busy.  Small batches keep the single launch (one wavefront's latency is what they wait for).
// =================================================================================
template <int SPACE, bool GUARD>
__device__ __forceinline__ void control_paths_for(const KernelArgs& a, const CtrlHandoff& ho, const size_t gid, int* knots) {
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const int p0 = threadIdx.x % SMX_WP_LANES;
  if (gid >= total) return;  // whole teams leave together
  const int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE) || (flags & SMX_F_SOCIAL)) return;
  if constexpr (GUARD)  // no path search for a vehicle the law kernel will park or hold
    if (guard_at_load(a, flags, load_vehicle(a, gid, total)).action != GUARD_STORE) return;
  const LaneAction la = load_lane_action<SPACE>(a, gid);
  if (!la.has_action) return;  // uniform within a team
  const PathSeeds seed = load_seeds(a, gid, total);  // found by k_scan at this very pose
  const double px = SF(SMX_S_X), py = SF(SMX_S_Y);
  auto put = [&](int i, const WaypointOut& w) {
    double* q = ho.path + (size_t)(i * 3) * total + gid;
    q[0] = w.x;
    q[total] = w.y;
    q[2 * total] = w.heading;
  };
  // ---- no walk at all when the waypoints sensor's chain walks of the previous tick can be reused: they started
  // from these very seeds (the controller asks its paths at the pose of the last observation), and a
  // lookahead-16 path is the first 17 lanepoints of the lookahead-32 one: its knots are the longer path's
  // knots less than 16 hops down plus the lanepoint 16 hops down (KnotLists.end16).  The first waypoint of
  // every path of a seed lane is the projection of the vehicle on the start lanepoint's heading line
  // (interpolate_knots at t = 0), so find_current_lane needs the start records only.  Taken when every seed
  // lane of the team has a list for its start and filter and none branches inside the lookahead.
  // (The choice among the seed lanes is written across the team's lanes here and over per-seed-lane arrays in
  // k_control_fast: that piece is left separate.)
  if (a.knots.key != nullptr && c.wp_lookahead >= SMX_CTRL_WPS - 1 && seed.road >= 0 && seed.n_lanes <= SMX_WP_LANES) {
    const size_t paths = total * SMX_WP_LANES, path = gid * SMX_WP_LANES + p0;
    const int start = p0 < seed.n_lanes ? seed_start(m, seed, p0, px, py) : -1;
    bool reusable = true;
    int n32 = 0;
    if (start >= 0) {
      n32 = a.knots.n[path];
      reusable = knot_list_reusable(a.knots.key[path], a.knots.key[paths + path], a.knots.key[2 * paths + path], a.knots.cnt[path],
                                    n32, start, seed.f);
    }
    if (!team_or(reusable ? 0 : 1)) {  // uniform within a team
      const int started = team_or(start >= 0 ? (1 << p0) : 0);
      const int n_paths = __popc(started);
      if (n_paths == 0) {
        if (p0 == 0) ho.n[gid] = 0;
        return;
      }
      const int mine = __popc(started & ((1 << p0) - 1));  // this lane's path number
      double my_d = SMX_INF;
      int my_idx = 0x7fffffff;
      smx_lp_rec r0 = smx_lp_rec{};
      if (start >= 0) {
        r0 = load_lp(m, start, 46);
        my_d = first_waypoint_distance(r0.x, r0.y, r0.dirx, r0.diry, n32, px, py);
        my_idx = mine;
      }
      team_nearest(my_d, my_idx);
      if (start < 0 || mine != wanted_path(my_idx, la.lane_change, n_paths)) return;
      const int n16 = n32 < SMX_CTRL_WPS ? n32 : SMX_CTRL_WPS;
      ctrl_waypoints_from_knots<false>(a, a.knots.idx + paths + path, paths, r0, a.knots.nk16[path], a.knots.end16[path], n16, px, py, put);
      ho.n[gid] = n16;
      return;
    }
  }
  TeamSearch ts = team_path_search<false>(m, seed, p0, px, py, knots, [](int, const WaypointOut&) {});
  team_nearest(ts.my_d, ts.my_idx);
  if (ts.n_paths <= 0) {  // uniform within a team
    if (p0 == 0) ho.n[gid] = 0;
    return;
  }
  const int want = wanted_path(ts.my_idx, la.lane_change, ts.n_paths);
  // the lane whose first seed lane holds path `want` walks to it again and writes its waypoints; a path of a
  // later seed lane (roads with more than four lanes) is found by lane 0 the long way
  const bool own = ts.cnt0 > 0 && want >= ts.goff0 && want < ts.goff0 + ts.cnt0;
  const int owners = team_or(own ? (1 << p0) : 0);
  const int act_lane = owners ? (__ffs(owners) - 1) : 0;
  if (p0 != act_lane) return;
  const int n = owners ? rewalk_branch(m, seed, p0, px, py, want - ts.goff0, knots, put)
                       : ctrl_path_serial(m, seed, px, py, want, knots, SMX_BLOCK, put);
  ho.n[gid] = n < SMX_CTRL_WPS ? n : SMX_CTRL_WPS;
}

// One team of four lanes per vehicle.  With a slow list in the arguments (large batches: the vehicles k_control_fast
// could not serve) a fixed grid strides that list, whose length is only known on the device.
// (the list form is a kernel of its own: with both forms in one kernel the role was inlined twice and the team cut's
// launch paid for it — 111 -> 137 registers here, 168 -> 256 in k_control_law, one wavefront per SIMD: C5's control
// phase 0.169 -> 0.209 ms)
template <int SPACE, bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_control_paths(const KernelArgs a, const CtrlHandoff ho) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  const size_t total = (size_t)a.cfg.num_envs * a.cfg.num_vehicles;
  control_paths_for<SPACE, GUARD>(a, ho, launch_vehicle(a, ((size_t)blockIdx.x * SMX_BLOCK + threadIdx.x) / SMX_WP_LANES, total), knot_scratch + threadIdx.x);
}
// ... of a mixed fleet (smx_step_mixed, large form): the same grid over the alive list, filtered by the table — a team
// whose slot has another space leaves before the role loads anything of the vehicle.  `slot_space`: AgentSpacesDev::space.
template <int SPACE, bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_control_paths_mixed(const KernelArgs a, const CtrlHandoff ho, const int32_t* slot_space) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  const size_t total = (size_t)a.cfg.num_envs * a.cfg.num_vehicles;
  const size_t gid = launch_vehicle(a, ((size_t)blockIdx.x * SMX_BLOCK + threadIdx.x) / SMX_WP_LANES, total);
  if (gid >= total || slot_space[gid % (size_t)a.cfg.num_vehicles] != SPACE) return;  // whole teams leave together
  control_paths_for<SPACE, GUARD>(a, ho, gid, knot_scratch + threadIdx.x);
}

// Control law + vehicle dynamics, one lane per vehicle (see k_control_paths).  Every action space; the
// lane-following ones read the wanted path from the hand-off.
template <int SPACE, bool GUARD>
__device__ __forceinline__ void control_law_for(const KernelArgs& a, const CtrlHandoff& ho, const size_t gid) {
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  if (gid >= total) return;
  int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE)) return;
  if (flags & SMX_F_SOCIAL) {
    social_vehicle_step(a, gid, total, SF(SMX_S_MCL_X), SF(SMX_S_MCL_Y), SF(SMX_S_SPD_INT), SF(SMX_S_THROTTLE), SF(SMX_S_X), SF(SMX_S_Y));
    return;
  }
  VehState s = load_vehicle(a, gid, total);
  if constexpr (GUARD) {
    const GuardVerdict gv = guard_at_load(a, flags, s);
    if (gv.action != GUARD_STORE) {
      guard_refuse(a, gid, total, flags, gv);
      return;
    }
  }
  CtrlState cs = load_ctrl_state(a, gid, total, flags);
  ControlOut co = idle_command(cs);
  constexpr bool lane_following = SPACE == SMX_ACTION_SPACE_LANE || SPACE == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED;
  if (lane_following) {
    const LaneAction la = load_lane_action<SPACE>(a, gid);
    if (la.has_action) {
      const int n = ho.n[gid];
      if (n > 0) {
        CtrlPath path;
        path.n = n;
#pragma unroll
        for (int k = 0; k < SMX_CTRL_WPS; ++k) {
          const double* q = ho.path + (size_t)(k * 3) * total + gid;
          const bool held = k < n;
          path.x[k] = held ? q[0] : 0.0;
          path.y[k] = held ? q[total] : 0.0;
          path.h[k] = held ? q[2 * total] : 0.0;
        }
        co = lane_following_from_path(s, cs, c.dt, la.target_speed, la.lane_change, la.hg, la.lg, path);
      } else {
        co = last_command(cs);
      }
    }
  } else if (SPACE == SMX_ACTION_SPACE_TRAJECTORY || SPACE == SMX_ACTION_SPACE_MPC) {
    if (a.traj_n[gid] > 0) {
      PackedTraj t;
      t.p = a.traj + gid * (size_t)(4 * SMX_TRAJ_COLS);
      t.n = a.traj_n[gid];
      co = SPACE == SMX_ACTION_SPACE_MPC ? trajectory_tracking_mpc(s, cs, c.dt, t) : trajectory_tracking_pd(s, cs, c.dt, t);
    }
  } else {
    const float act0 = a.actions_f32[gid * 3 + 0], act1 = a.actions_f32[gid * 3 + 1], act2 = a.actions_f32[gid * 3 + 2];
    if (!(act0 != act0)) co = direct_command<SPACE>(act0, act1, act2, cs, c.dt);  // NaN = no action
  }
  SF(SMX_S_PREV_X) = s.x;  // the position recorded by the previous observation
  SF(SMX_S_PREV_Y) = s.y;
  vehicle_step(s, co, c.dt);
  if constexpr (GUARD)
    if (!guard_before_store(a, gid, flags, s)) return;
  store_vehicle_state(a, gid, total, s, cs, flags);
}

template <int SPACE, bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_control_law(const KernelArgs a, const CtrlHandoff ho) {
  control_law_for<SPACE, GUARD>(a, ho, (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x);
}
// ... of a mixed fleet (see k_control_paths_mixed): a lane whose slot has another space leaves before the role loads
// anything of the vehicle.  The social slots carry the owner space in the table, so one launch of the tick steps them.
template <int SPACE, bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_control_law_mixed(const KernelArgs a, const CtrlHandoff ho, const int32_t* slot_space) {
  const size_t gid = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  if (slot_space[gid % (size_t)a.cfg.num_vehicles] != SPACE) return;
  control_law_for<SPACE, GUARD>(a, ho, gid);
}
// =================================================================================
// k_control_kinematic: the kinematic action spaces, one lane per vehicle, in the place of controller + vehicle_step.
// The agent's vehicle is a box that a provider places (BoxChassis.control, chassis.py:211-217): the new pose and
// speed go to the state rows, with the heading held before and the dt of the move for the ego read-back
// (include/smx.h lists the rows).  All float64, in the reference's order of operations.
// =================================================================================
struct KinPose {
  double x, y, heading, speed;
};

// MotionPlannerProvider.step -> BezierMotionPlanner.trajectory_batched(pose, target, n = 1, dt)
// (motion_planner_provider.py:92-99, bezier_motion_planner.py:53-121); `heading` in and out is the provider's own
// (_poses[:, 2]: never re-normalised).
__device__ __forceinline__ KinPose bezier_first_point(double x, double y, double heading, double tx, double ty, double th,
                                                      double seconds, double dt) {
  const double extend = 0.9, bias = 0.5;
  const double target_heading = th + SMX_PI * 0.5, current_heading = heading + SMX_PI * 0.5;
  double tsn, tcs, csn, ccs;
  sincos(target_heading, &tsn, &tcs);
  sincos(current_heading, &csn, &ccs);
  const double ex = tx - x, ey = ty - y;
  const double extension = sqrt(ex * ex + ey * ey) * extend;
  const double p0[2] = {x, y};
  const double p1[2] = {x + ccs * extension * bias, y + csn * extension * bias};
  const double p2[2] = {tx - tcs * extension * (1.0 - bias), ty - tsn * extension * (1.0 - bias)};
  const double p3[2] = {tx, ty};
  const double t = (1.0 * dt) / (seconds < dt ? dt : seconds);  // .clip(dt, None): a NaN stays one
  auto linear = [t](double a, double b) { return (1.0 - t) * a + t * b; };
  auto quadratic = [&](double a, double b, double c) { return linear(linear(a, b), linear(b, c)); };
  double pos[2], tan[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    pos[q] = linear(quadratic(p0[q], p1[q], p2[q]), quadratic(p1[q], p2[q], p3[q]));
    const double u = 1.0 - t;
    tan[q] = 3.0 * (u * u) * (p1[q] - p0[q]) + 6.0 * u * t * (p2[q] - p1[q]) + 3.0 * (t * t) * (p3[q] - p2[q]);
  }
  const double correction = py_mod((target_heading - current_heading) + SMX_PI, SMX_TWO_PI) - SMX_PI;
  KinPose o;
  o.x = pos[0];
  o.y = pos[1];
  o.heading = current_heading + (py_mod(t * correction + SMX_PI, SMX_TWO_PI) - SMX_PI) - SMX_PI * 0.5;
  o.speed = sqrt(tan[0] * tan[0] + tan[1] * tan[1]);
  return o;
}

// TrajectoryInterpolationProvider.perform_trajectory_interpolation(dt, trajectory) (trajectory_interpolation_provider.py:
// 96-193) on rows time, x, y, heading, speed of `stride` columns, n of them given.  False: the reference raises
// (is_legal_trajectory :97-109, locate_motion_state :143-145).  (Its "stop here" branch for an infinite time,
// :175-183, lies behind is_legal_trajectory's isfinite and cannot be reached.)
__device__ __forceinline__ bool interpolate_trajectory(const double* tr, int n, int stride, double dt, KinPose& o) {
  if (n < 2 || n > stride) return false;
  bool legal = true;
  int end = -1;  // the first column later than dt
  double prev = 0.0;
  for (int i = 0; i < n; ++i) {
    const double ti = tr[i];
#pragma unroll
    for (int r = 0; r < 5; ++r) legal = legal && isfinite(tr[(size_t)r * stride + i]);
    if (i > 0 && !(ti - prev > 0.0)) legal = false;
    if (end < 0 && ti > dt) end = i;
    prev = ti;
  }
  if (!legal || end < 1) return false;  // (none, or the first one already: no pair to blend)
  const double* m0 = tr + (end - 1);
  const double* m1 = tr + end;
  const double ratio = fabs((dt - m0[0]) / (m1[0] - m0[0]));
  const double u = 1.0 - ratio;
  double s0, c0, s1, c1;
  sincos(m0[(size_t)3 * stride], &s0, &c0);
  sincos(m1[(size_t)3 * stride], &s1, &c1);
  o.x = u * m0[(size_t)1 * stride] + ratio * m1[(size_t)1 * stride];
  o.y = u * m0[(size_t)2 * stride] + ratio * m1[(size_t)2 * stride];
  o.heading = atan2(u * s0 + ratio * s1, u * c0 + ratio * c1);
  o.speed = u * m0[(size_t)4 * stride] + ratio * m1[(size_t)4 * stride];
  return true;
}

// (FOLLOW, Imitation only: the tick of smx_step_history_agents — every agent is placed on the row its recorded vehicle
// has in the frame of the coming observation, Vehicle.update_state -> control(pose, speed, dt), smarts.py:919-921,
// vehicle.py:573-579; no action is read.  HANDOVER, Imitation only, never with FOLLOW: the tick of
// smx_step_history_handover — each lane decides from the handover table whether its agent follows, as above, or is driven
// by its action as in the plain form, switch_control_to_agent's BoxChassis at the held pose and speed, smarts.py:505-561.
// BUBBLES, with HANDOVER only: that tick with bubbles bound (smx_set_history_bubbles) — k_bubbles has left each agent's
// state byte in `bubble_state`; a HIJACKED agent is driven as a table-driven one is, a RELEASED one ends as a leaving
// follower does, a SHADOWED one follows under its own status; the table may be absent.)
template <int SPACE, bool GUARD, bool FOLLOW, bool HANDOVER, bool BUBBLES>
__device__ __forceinline__ void control_kinematic(const KernelArgs& a, const uint8_t* bubble_state) {
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE)) return;
  if (flags & SMX_F_SOCIAL) {
    social_vehicle_step(a, gid, total, SF(SMX_S_MCL_X), SF(SMX_S_MCL_Y), SF(SMX_S_SPD_INT), SF(SMX_S_THROTTLE), SF(SMX_S_X), SF(SMX_S_Y));
    return;
  }
  const double x = SF(SMX_S_X), y = SF(SMX_S_Y);
  if constexpr (GUARD) {
    // the kinematic vehicle's words: x, y, heading, speed
    const GuardVerdict gv = guard_resolve((flags & SMX_F_GUARDED) != 0, guard_in_bounds_kin(a.guard_box, x, y, SF(SMX_S_HEADING), SF(SMX_S_U)), true);
    if (gv.action != GUARD_STORE) {
      guard_refuse(a, gid, total, flags, gv);
      return;
    }
    a.guard[gid] = 0;  // (the tick may end below without a placement: no action, an action the reference raises on)
  }
  if constexpr (FOLLOW || HANDOVER) {
    const int env = (int)(gid / (size_t)c.num_vehicles);
    const int episode = a.st.env_episode[env];
    bool follows = true;
    int follow_status = SMX_HA_FOLLOWING;
    if constexpr (BUBBLES) {
      const int bubble = bubble_state[gid];
      if (a.history.handover != nullptr)
        follows = !history_driven(history_handover(a.history, episode, env, (int)(gid - (size_t)env * c.num_vehicles)), a.st.env_ticks[env]);
      if (bubble == SMX_BUBBLE_HIJACKED) follows = false;
      if (follows && bubble == SMX_BUBBLE_RELEASED) {
        // released by its bubble in this tick: the agent ends as a follower whose vehicle has left the recording ends
        a.st.flags[gid] = flags | SMX_F_LEFT;
        history_agent_report(a, gid, SMX_HA_RELEASED, 0, nullptr, -1);
        return;
      }
      if (bubble == SMX_BUBBLE_SHADOWED) follow_status = SMX_HA_SHADOWED;
    } else if constexpr (HANDOVER) {
      follows = !history_driven(history_handover(a.history, episode, env, (int)(gid - (size_t)env * c.num_vehicles)), a.st.env_ticks[env]);
    }
    if (follows) {
      if constexpr (BUBBLES)
        history_agent_follow(a, gid, total, flags, env, episode, x, y, follow_status);
      else
        history_agent_follow(a, gid, total, flags, env, episode, x, y);
      return;
    }
    // a driven agent: the Imitation branch below from the state it holds — no expert label, and SMX_F_LEFT is never set
    history_agent_report(a, gid, SMX_HA_DRIVEN, 0, nullptr, -1);
  }
  // the placement's test, ahead of its first store: held = nothing of the vehicle is stored
  auto guard_holds = [&](const KinPose& q) {
    const GuardVerdict gv = guard_resolve(false, true, guard_in_bounds_kin(a.guard_box, q.x, q.y, q.heading, q.speed));
    if (gv.action == GUARD_STORE) return false;
    a.guard[gid] = gv.byte;
    a.st.flags[gid] = flags | SMX_F_GUARDED;
    return true;
  };
  SF(SMX_S_PREV_X) = x;  // the position recorded by the previous observation
  SF(SMX_S_PREV_Y) = y;
  KinPose o;
  if (SPACE == SMX_ACTION_SPACE_TARGET_POSE) {
    const double raw = SF(SMX_S_KIN_RAW_HEADING);
    const double* tp = a.traj + gid * 4;
    double tx = tp[0], ty = tp[1], th = tp[2], seconds = tp[3];
    bool given = !(tx != tx);
    if (given) {
      o = bezier_first_point(x, y, raw, tx, ty, th, seconds, c.dt);
      if (!(isfinite(o.x) && isfinite(o.y) && isfinite(o.heading) && isfinite(o.speed))) {
        // (the reference would carry the pose on and fail later; here it is reported at the next smx_sync and the
        // agent is stepped as if it had sent nothing)
        atomicOr(a.status, SMX_DEVICE_BAD_TARGET_POSE);
        given = false;
      }
    }
    // no target pose from the agent: the pose the provider holds, dt ahead (_normalize_target_pose, :119-129) — the
    // vehicle stays, its speed is 0, and control() is still called
    if (!given) o = bezier_first_point(x, y, raw, x, y, raw, c.dt, c.dt);
    if constexpr (GUARD)
      if (guard_holds(o)) return;
    SF(SMX_S_KIN_RAW_HEADING) = o.heading;
  } else if (SPACE == SMX_ACTION_SPACE_IMITATION) {
    // ImitationController.perform_action on a BoxChassis (imitation_controller.py:50-78)
    const float act0 = a.actions_f32[gid * 3 + 0], act1 = a.actions_f32[gid * 3 + 1];
    if (act0 != act0) return;  // no action: no control() call
    const double heading = SF(SMX_S_HEADING), speed = SF(SMX_S_U);
    if (act1 != act1) {
      // a scalar action, "setting the initial speed" (:50-56): vehicle.control(vehicle.pose, action, dt)
      o.x = x;
      o.y = y;
      o.heading = heading;
      o.speed = (double)act0;
    } else {
      // (acceleration, angular_velocity), from the heading and speed held before the tick (:61-78)
      const double acceleration = (double)act0, angular_velocity = (double)act1;
      const double target_heading = py_mod(heading + angular_velocity * c.dt, SMX_TWO_PI);
      double hvx, hvy;
      radians_to_vec(heading, hvx, hvy);
      o.x = x + hvx * speed * c.dt;
      o.y = y + hvy * speed * c.dt;
      // Pose(orientation=fast_quaternion_from_angle(target_heading)).heading: yaw_from_quaternion of (0, 0, sin, cos)
      // of the half angle (math.py:78-106), then Heading() further down
      double qz, qw;
      sincos(target_heading * 0.5, &qz, &qw);
      o.heading = atan2(2.0 * (0.0 * 0.0 + qw * qz), qw * qw + 0.0 * 0.0 - 0.0 * 0.0 - qz * qz);
      o.speed = speed + acceleration * c.dt;
    }
    if (!(isfinite(o.x) && isfinite(o.y) && isfinite(o.heading) && isfinite(o.speed))) {
      // (an infinite component, or a pose or speed that came out not finite: the reference would carry it on; here it is
      // reported at the next smx_sync and the agent is stepped as if it had sent nothing)
      atomicOr(a.status, SMX_DEVICE_BAD_TARGET_POSE);
      return;
    }
  } else {
    const int n = a.traj_n[gid];
    if (n == 0) return;  // no action: the vehicle is not updated (no control() call: _last_heading, _last_dt stay)
    if (!interpolate_trajectory(a.traj + gid * (size_t)5 * a.traj_max, n, a.traj_max, c.dt, o)) {
      atomicOr(a.status, SMX_DEVICE_BAD_TRAJECTORY);  // the reference raises; reported at the next smx_sync
      return;
    }
  }
  if constexpr (GUARD && SPACE != SMX_ACTION_SPACE_TARGET_POSE)
    if (guard_holds(o)) return;
  // Vehicle.control(pose, speed, dt) -> BoxChassis.control (vehicle.py:578, chassis.py:211-217)
  SF(SMX_S_KIN_LAST_HEADING) = SF(SMX_S_HEADING);
  SF(SMX_S_KIN_LAST_DT) = c.dt;
  SF(SMX_S_X) = o.x;
  SF(SMX_S_Y) = o.y;
  // Heading(...) (coordinates.py:175-184); Imitation's scalar form hands the vehicle's own pose back, a Heading already
  const double held_heading = SF(SMX_S_HEADING);
  SF(SMX_S_HEADING) = (SPACE == SMX_ACTION_SPACE_IMITATION && o.heading == held_heading) ? held_heading : wrap_heading(o.heading);
  SF(SMX_S_U) = o.speed;
}
template <int SPACE, bool GUARD = false, bool FOLLOW = false, bool HANDOVER = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_control_kinematic(const KernelArgs a) {
  control_kinematic<SPACE, GUARD, FOLLOW, HANDOVER, false>(a, nullptr);
}
// (the BUBBLES form: the state row is the kernel's own second argument — KernelArgs does not grow for a rare binding)
template <bool GUARD>
__global__ void __launch_bounds__(SMX_BLOCK) k_control_kinematic_bubbles(const KernelArgs a, const uint8_t* bubble_state) {
  control_kinematic<SMX_ACTION_SPACE_IMITATION, GUARD, false, true, true>(a, bubble_state);
}

// =================================================================================
// k_bubbles (smx_set_history_bubbles; smx_bubbles.h holds the rule): the bubble pass ahead of the control kernel of a
// mixed tick, one wavefront per env, one lane per agent slot, on the poses the previous pass left.  The zone tests run
// per lane; ballots turn them and the state bytes into the per-bubble masks of bubble_recurrence, the serial loop over
// the env's agent slots that the limits need, which every lane runs on the same words.  Each lane then applies its own
// transitions in ascending bubble order and stores its two bytes.  An env in the first tick of an episode starts from
// zero bytes whatever the rows hold (k_bubbles_clear zeroes them behind a reset pass of this entry point or of
// smx_reset; a reset inside another entry point's tick leaves them alone).
// =================================================================================
struct BubbleArgs {
  const int32_t* flags;        // [E*N]
  const double* f64;           // [SMX_S_COUNT][E*N]
  const int32_t* env_ticks;    // [E]
  const int32_t* env_episode;  // [E]
  HistoryDev history;          // (the handover table: who is an ego in this tick)
  uint8_t* state;              // [E*N]
  uint8_t* cursor;             // [E*N]
  size_t total;
  int num_envs, num_vehicles, n_agents, reset_elapsed_steps;
};
__global__ void __launch_bounds__(64) k_bubbles(const BubbleArgs g, const BubbleSet bs) {
  const int env = (int)blockIdx.x, k = (int)threadIdx.x;
  if (env >= g.num_envs) return;  // (uniform)
  const bool lane = k < g.n_agents;
  const size_t gid = (size_t)env * g.num_vehicles + (size_t)(lane ? k : 0);
  const int ticks = g.env_ticks[env];
  const bool fresh = ticks == g.reset_elapsed_steps;
  const int flags = g.flags[gid];
  const bool alive = lane && (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL);
  const double x = g.f64[(size_t)SMX_S_X * g.total + gid], y = g.f64[(size_t)SMX_S_Y * g.total + gid];
  const double heading = g.f64[(size_t)SMX_S_HEADING * g.total + gid];
  int state = fresh ? SMX_BUBBLE_SOCIAL : (int)g.state[gid];
  const unsigned was = fresh ? 0u : (unsigned)g.cursor[gid];
  const bool ego = lane && g.history.handover != nullptr && history_driven(history_handover(g.history, g.env_episode[env], env, lane ? k : 0), ticks);
  const int seen = ego ? SMX_BUBBLE_EGO : state;
  const uint64_t alive_m = __ballot(alive);
  // (an agent that is not alive is in none of the three: for the reference's index a vehicle that is gone is neither
  // hijacked nor shadowed, vehicle_index.py:189-201)
  const uint64_t social_m = __ballot(alive && seen == SMX_BUBBLE_SOCIAL), shadowed_m = __ballot(alive && seen == SMX_BUBBLE_SHADOWED),
                 hijacked_m = __ballot(alive && seen == SMX_BUBBLE_HIJACKED);
  unsigned now = 0;
  int applied = state;
  for (int b = 0; b < bs.n && b < SMX_MAX_BUBBLES; ++b) {  // (uniform)
    const smx_bubble& bb = bs.b[b];
    const int f = bb.follow_agent < g.n_agents ? bb.follow_agent : -1;  // (held below the agent count at the bind)
    double fx = 0.0, fy = 0.0, fh = 0.0;
    bool active = true;
    if (f >= 0) {
      fx = __shfl(x, f);
      fy = __shfl(y, f);
      fh = __shfl(heading, f);
      active = ((alive_m >> f) & 1) != 0;
    }
    if (!active) continue;  // no cursors: this bubble's bits clear, states stay
    const BubbleZone z = bubble_zone(bb, x, y, fx, fy, fh);
    BubbleMasks m;
    m.alive = alive_m;
    m.social = social_m;
    m.shadowed = shadowed_m;
    m.hijacked = hijacked_m;
    m.was_in = __ballot(lane && ((was >> b) & 1u));
    m.in_bubble = __ballot(alive && z.in_bubble);
    m.in_airlock = __ballot(alive && z.in_airlock);
    const BubbleResult r = bubble_recurrence(m, g.n_agents, bb.hijack_limit, bb.shadow_limit);
    if (lane) {
      if (((r.cur_bubble | r.cur_airlock) >> k) & 1) now |= 1u << b;
      applied = bubble_apply(applied, bubble_transition_of(r, k));  // (an ego makes none)
    }
  }
  if (lane) {
    g.state[gid] = (uint8_t)applied;
    g.cursor[gid] = (uint8_t)now;
  }
}
// Behind a reset pass: the two bytes of every agent of an env that has just been reset read 0.
__global__ void __launch_bounds__(SMX_BLOCK) k_bubbles_clear(const BubbleArgs g) {
  const size_t gid = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  if (gid >= g.total) return;
  const int env = (int)(gid / (size_t)g.num_vehicles);
  if ((int)(gid - (size_t)env * g.num_vehicles) >= g.n_agents || g.env_ticks[env] != g.reset_elapsed_steps) return;
  g.state[gid] = 0;
  g.cursor[gid] = 0;
}

// The vehicles k_control_fast left on its slow list (large batches), a fixed grid striding the list, whose length is only
// known on the device: sixteen vehicles a round, their candidate paths by teams of four lanes, then, behind a barrier,
// their control law + dynamics on sixteen lanes, the wanted path passed through the hand-off in device memory.  (One
// launch: the list is under 1 % of the vehicles on a map whose lanes do not split, and a second launch over it was
// a launch boundary on the tick's longest chain.)
template <int SPACE, bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_control_listed(const KernelArgs a, const CtrlHandoff ho) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  constexpr int VPB = SMX_BLOCK / SMX_WP_LANES;
  const int count = *a.slow_count;
  for (int i0 = (int)blockIdx.x * VPB; i0 < count; i0 += (int)gridDim.x * VPB) {  // (uniform in the workgroup)
    const int i = i0 + (int)threadIdx.x / SMX_WP_LANES;
    if (i < count) control_paths_for<SPACE, GUARD>(a, ho, (size_t)a.slow_list[i], knot_scratch + threadIdx.x);
    __threadfence_block();
    __syncthreads();
    if ((int)threadIdx.x < VPB && i0 + (int)threadIdx.x < count) control_law_for<SPACE, GUARD>(a, ho, (size_t)a.slow_list[i0 + threadIdx.x]);
  }
}

// =================================================================================
// k_control_fast (large batches, lane-following action spaces): controller + dynamics with ONE lane per vehicle and
// no hand-off.  The controller's candidate paths start on the seeds the waypoints sensor walked last tick
// (k_control_paths explains the reuse): find_current_lane needs the start lanepoints only, and the wanted path's
// 17 waypoints are interpolated from its knot list straight into this lane's LDS column, read back with fixed
// indices by the control law.  k_control_paths wrote them to device memory for k_control_law to read back (115 MB
// each way at 131 k vehicles) with three of its four lanes idle during the interpolation.  A vehicle whose lists
// cannot be reused — a new vehicle, a branching inside the lookahead, a road of more than four lanes — goes to the
// slow list and through k_control_paths / k_control_law as before.
// =================================================================================
template <int SPACE, bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_control_fast(const KernelArgs a) {
  SMX_TSTAMP(span0);
  // the wanted path's waypoints, [element][lane]: 17 headings, then x and y of the first ten (lane_following_from_path
  // reads no position beyond waypoint 9).  19 KB: eight workgroups per CU, every vehicle of 131 k resident at once — at
  // 26 KB (all 51 elements) six fit, and the kernel ran a second round for a quarter of its workgroups.
  constexpr int CTRL_XY = 10;
  __shared__ double path_lds[(SMX_CTRL_WPS + 2 * CTRL_XY) * SMX_BLOCK];
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = launch_vehicle(a, (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x, total);
  bool slow = false;
  // ---- every word whose address only needs the vehicle, loaded together and whatever the flags say (two wavefronts
  // per SIMD hide nothing: flags -> action -> seeds -> list keys -> ... one behind the other was a microsecond each)
  const bool in_range = gid < total;
  const size_t g = in_range ? gid : 0;
  int flags = a.st.flags[g];
  int action = SMX_ACTION_NONE;
  float act0 = 0.f, act1 = 0.f;
  if (SPACE == SMX_ACTION_SPACE_LANE) {
    action = a.actions[g];
  } else {
    act0 = a.actions_f32[g * 3 + 0];
    act1 = a.actions_f32[g * 3 + 1];
  }
  VehState s = load_vehicle(a, g, total);
  CtrlState cs = load_ctrl_state(a, g, total, flags);
  const PathSeeds seed = load_seeds(a, g, total);
  const bool table = a.knot_table != nullptr;
  const bool lists = table || a.knots.key != nullptr;
  const size_t paths = total * SMX_WP_LANES;
  int kn_n[SMX_WP_LANES], kn_key0[SMX_WP_LANES], kn_key1[SMX_WP_LANES], kn_key2[SMX_WP_LANES], kn_cnt[SMX_WP_LANES],
      kn_nk16[SMX_WP_LANES], kn_end16[SMX_WP_LANES];
  // with the knot table: the rows of the four start lanepoints (the seeds hold them: one level behind the seeds' loads);
  // kn_key0 = the row's flags, kn_key1 / kn_key2 = the filter it was walked with, kn_cnt = its road
  int st[SMX_WP_LANES];
#pragma unroll
  for (int q = 0; q < SMX_WP_LANES; ++q) {
    st[q] = (seed.road >= 0 && seed.n_lanes <= SMX_WP_LANES && q < seed.n_lanes) ? seed_start(m, seed, q, s.x, s.y) : -1;
    const size_t pth = g * SMX_WP_LANES + q;
    if (table) {
      // (a dead slot's seeds are words of any age: the row index is held to the table whatever they say)
      const KnotRow* row = a.knot_table + ((unsigned)st[q] < (unsigned)m.n_lanepoints ? st[q] : 0);
      kn_n[q] = row->n;
      kn_key0[q] = row->flags;
      kn_key1[q] = row->f0;
      kn_key2[q] = row->f1;
      kn_cnt[q] = row->road;
      kn_nk16[q] = row->nk16;
      kn_end16[q] = row->end16;
    } else {
      kn_n[q] = lists ? (int)a.knots.n[pth] : 0;
      kn_key0[q] = lists ? a.knots.key[pth] : -1;
      kn_key1[q] = lists ? a.knots.key[paths + pth] : -1;
      kn_key2[q] = lists ? a.knots.key[2 * paths + pth] : -1;
      kn_cnt[q] = lists ? (int)a.knots.cnt[pth] : 0;
      kn_nk16[q] = lists ? (int)a.knots.nk16[pth] : 0;
      kn_end16[q] = lists ? a.knots.end16[pth] : -1;
    }
  }
  if (in_range && (flags & SMX_F_ALIVE)) {
    GuardVerdict gv = {0, GUARD_STORE};
    if constexpr (GUARD) gv = guard_at_load(a, flags, s);
    if (flags & SMX_F_SOCIAL) {
      social_vehicle_step(a, gid, total, cs.mcl_x, cs.mcl_y, cs.spd_int, cs.throttle, s.x, s.y);
    } else if (GUARD && gv.action != GUARD_STORE) {
      guard_refuse(a, gid, total, flags, gv);  // (never on the slow list: no search sees the pose)
    } else {
      const LaneAction la = decode_lane_action<SPACE>(a, action, act0, act1);  // (on the words loaded above)
      const bool has_action = la.has_action;
      CtrlPath path;
      path.n = 0;
      if (has_action && !SMX_SKIP(a, 1 << 26)) {
        // ---- the wanted path from the sensor's knot lists (k_control_paths' reuse, one lane doing the team's part)
        const double px = s.x, py = s.y;
        if (!lists || c.wp_lookahead < SMX_CTRL_WPS - 1 || (seed.road >= 0 && seed.n_lanes > SMX_WP_LANES)) {
          slow = true;
        } else if (seed.road >= 0) {
          int started = 0, qw = 0;
          double my_d = SMX_INF;
          int my_idx = 0;
          // the start lanepoints' records, together
          double rx[SMX_WP_LANES], ry[SMX_WP_LANES], rdx[SMX_WP_LANES], rdy[SMX_WP_LANES], rh[SMX_WP_LANES];
#pragma unroll
          for (int q = 0; q < SMX_WP_LANES; ++q) {
            const smx_lp_rec* r = m.lp_rec + (st[q] >= 0 ? st[q] : 0);
            rx[q] = r->x;
            ry[q] = r->y;
            rdx[q] = r->dirx;
            rdy[q] = r->diry;
            rh[q] = r->heading;
          }
          // every seed lane's list must be this tick's; the nearest first waypoint (find_current_lane,
          // lane_following_controller.py:367-374: np.argmin, the lowest path number wins ties)
#pragma unroll
          for (int q = 0; q < SMX_WP_LANES; ++q) {
            if (st[q] >= 0) {
              const bool usable = table ? knot_row_serves(kn_key0[q], kn_key1[q], kn_key2[q], kn_cnt[q], seed.f)
                                        : knot_list_reusable(kn_key0[q], kn_key1[q], kn_key2[q], kn_cnt[q], kn_n[q], st[q], seed.f);
              SMX_COUNT(57, !usable);
              if (!usable) slow = true;
              const double d = first_waypoint_distance(rx[q], ry[q], rdx[q], rdy[q], kn_n[q], px, py);
              if (d < my_d) {
                my_d = d;
                my_idx = __popc(started);
              }
              started |= 1 << q;
            }
          }
          const int n_paths = __popc(started);
          if (!slow && n_paths > 0) {
            const int want = wanted_path(my_idx, la.lane_change, n_paths);
            // the want-th started seed lane
#pragma unroll
            for (int q = 0; q < SMX_WP_LANES; ++q)
              if ((started >> q) & 1)
                if (__popc(started & ((1 << q) - 1)) == want) qw = q;
            int n32w = 0, nk16 = 0, last = -1, stw = 0;
            smx_lp_rec r0 = smx_lp_rec{};
#pragma unroll
            for (int q = 0; q < SMX_WP_LANES; ++q)
              if (q == qw) {
                stw = st[q];
                n32w = kn_n[q];
                nk16 = kn_nk16[q];
                last = kn_end16[q];  // the last knot when it is not one of the list's
                r0.x = rx[q];
                r0.y = ry[q];
                r0.dirx = rdx[q];
                r0.diry = rdy[q];
                r0.heading = rh[q];
              }
            r0.lane = 0;  // (lane, width and speed limit of the waypoints are not the controller's business)
            const int n16 = n32w < SMX_CTRL_WPS ? n32w : SMX_CTRL_WPS;
            double* col = path_lds + threadIdx.x;
            const int32_t* const knot1 = table ? a.knot_table[stw].idx : a.knots.idx + paths + gid * SMX_WP_LANES + qw;
            ctrl_waypoints_from_knots<true>(a, knot1, table ? (size_t)1 : paths, r0, nk16, last, n16, px, py,
                                            [&](int i, const WaypointOut& w) {
                                              col[(size_t)i * SMX_BLOCK] = w.heading;
                                              if (i < CTRL_XY) {
                                                col[(size_t)(SMX_CTRL_WPS + i) * SMX_BLOCK] = w.x;
                                                col[(size_t)(SMX_CTRL_WPS + CTRL_XY + i) * SMX_BLOCK] = w.y;
                                              }
                                            });
            path.n = n16;
#pragma unroll
            for (int k = 0; k < SMX_CTRL_WPS; ++k) {
              const bool held = k < n16;
              path.h[k] = held ? col[(size_t)k * SMX_BLOCK] : 0.0;
              path.x[k] = (held && k < CTRL_XY) ? col[(size_t)(SMX_CTRL_WPS + (k < CTRL_XY ? k : 0)) * SMX_BLOCK] : 0.0;
              path.y[k] = (held && k < CTRL_XY) ? col[(size_t)(SMX_CTRL_WPS + CTRL_XY + (k < CTRL_XY ? k : 0)) * SMX_BLOCK] : 0.0;
            }
          }
        }
      }
      if (!slow) {
        ControlOut co = idle_command(cs);
        if (has_action) {
          if (path.n > 0 && !SMX_SKIP(a, 1 << 28)) {
            co = lane_following_from_path(s, cs, c.dt, la.target_speed, la.lane_change, la.hg, la.lg, path);
          } else {
            co = last_command(cs);
          }
        }
        SF(SMX_S_PREV_X) = s.x;  // the position recorded by the previous observation
        SF(SMX_S_PREV_Y) = s.y;
        if (!SMX_SKIP(a, 1 << 27)) vehicle_step(s, co, c.dt);
        if (!GUARD || guard_before_store(a, gid, flags, s)) store_vehicle_state(a, gid, total, s, cs, flags);
      }
    }
  }
  // the wavefront's slow vehicles, appended with one atomic
  const unsigned long long mask = __ballot(slow);
  if (mask != 0ull) {
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(a.slow_count, __popcll(mask));
    base = __shfl(base, __ffsll((long long)mask) - 1);
    if (slow) a.slow_list[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)gid;
  }
  SMX_TSTAMP(span1);
  SMX_TSPAN(0, span0, span1);
}

// =================================================================================
// k_social (SMX_SOCIAL_IDM only): car following of the scripted social vehicles, one thread per
// vehicle, before k_control moves anything: every follower reads its env-mates' poses and speeds as
// they stand at the start of the tick and leaves its speed for the tick in SMX_S_THROTTLE (unused by a
// kinematic vehicle).  The arithmetic is oracle/sim.py::SocialBody.idm_speed.
// =================================================================================
__global__ void __launch_bounds__(SMX_BLOCK) k_social(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE) || !(flags & SMX_F_SOCIAL)) return;
  const int n_veh = c.num_vehicles;
  const size_t env0 = (gid / n_veh) * n_veh;
  const int slot = (int)(gid - env0);
  const double x = SF(SMX_S_X), y = SF(SMX_S_Y), h = SF(SMX_S_HEADING), v = SF(SMX_S_U);
  const double v0 = m.lane_speed[(int)SF(SMX_S_MCL_X)] * c.social_speed_factor;
  const double fx = -sin(h), fy = cos(h), rx = cos(h), ry = sin(h);
  double best = 60.0, lead_u = 0.0;
  bool found = false;
  for (int j = 0; j < n_veh; ++j) {
    if (j == slot) continue;
    const size_t og = env0 + j;
    if (!(a.st.flags[og] & SMX_F_ALIVE)) continue;
    const double dx = a.st.f64[(size_t)SMX_S_X * total + og] - x, dy = a.st.f64[(size_t)SMX_S_Y * total + og] - y;
    const double lon = dx * fx + dy * fy, lat = dx * rx + dy * ry;
    if (lon > 0.0 && lon < best && fabs(lat) < 1.6) {
      best = lon;
      lead_u = a.st.f64[(size_t)SMX_S_U * total + og];
      found = true;
    }
  }
  double v_new;
  if (v0 <= 0.0) {
    v_new = fmax(0.0, v - 4.5 * c.dt);
  } else {
    const double ratio = v / v0;
    const double free_term = 1.0 - (ratio * ratio) * (ratio * ratio);
    double inter = 0.0;
    if (found) {
      const double gap = fmax(best - SMX_CHASSIS_LENGTH, 0.1);
      const double dv = v - lead_u;
      const double sstar = 2.5 + fmax(0.0, v * 1.0 + v * dv / (2.0 * sqrt(2.6 * 4.5)));
      const double q = sstar / gap;
      inter = q * q;
    }
    const double acc = 2.6 * (free_term - inter);
    v_new = fmin(fmax(v + acc * c.dt, 0.0), v0);
  }
  SF(SMX_S_THROTTLE) = v_new;
}

// =================================================================================
// waypoints role: waypoint paths (sensors.py:268-275, 972-985) + trip meter (sensors.py:880-947).
// SMX_WP_LANES lanes per vehicle.  Team lane p takes seed lane p and writes its first path straight
// into the dense rows at the slot it would have if no lower seed lane branches (its provisional
// number); the team then exchanges the real counts.  Almost always that guess was right and every
// lane has walked exactly one path.  Otherwise (a branching inside the lookahead, or a road with
// more than four lanes) the team numbers the paths the long way and rewrites the rows.
// Rows are written whole every tick (unused waypoints and paths as zeros, format_obs.py:589-596),
// each lane streaming its own row in order, so L2 assembles full lines before they leave.
// The steps below the row helpers — one path into one row, the branching case, the long way, closing the rows,
// the trip meter — are written once and shared with the staged and the emit-parallel form further down.
// =================================================================================
struct WpRows {
  double* pos;
  float *heading, *width, *speed;
  int16_t* lid;
  int8_t* lidx;
  int cached_lane;  // lane whose index is held in cached_index (-1: none): consecutive waypoints
  int cached_index; // mostly share their lane, and a look-up per waypoint stalls its own store
};

__device__ __forceinline__ WpRows wp_rows(const smx_outputs& o, size_t gid, int P, int W, int slot) {
  const size_t q = (gid * P + slot) * (size_t)W;
  WpRows r;
  r.pos = o.wp_pos + q * 3;
  r.heading = o.wp_heading + q;
  r.width = o.wp_lane_width + q;
  r.speed = o.wp_speed_limit + q;
  r.lid = o.wp_lane_id + q;
  r.lidx = o.wp_lane_index + q;
  r.cached_lane = -1;
  r.cached_index = 0;
  return r;
}

__device__ __forceinline__ void wp_put(const MapDev& m, WpRows& r, int i, const WaypointOut& w) {
  if (r.pos == nullptr) {  // developer switch (SMX_DEBUG_SKIP & 32768): compute, do not store
    if (i == 0x7fffffff) r.cached_index = (int)(w.x + w.y + w.heading + w.width + w.speed) + w.lane;
    return;
  }
  if (w.lane != r.cached_lane) {
    r.cached_lane = w.lane;
    r.cached_index = m.lane_index[w.lane];
  }
  r.pos[i * 3 + 0] = w.x;
  r.pos[i * 3 + 1] = w.y;
  r.pos[i * 3 + 2] = 0.0;
  r.heading[i] = (float)w.heading;
  r.width[i] = (float)w.width;
  r.speed[i] = (float)w.speed;
  r.lid[i] = (int16_t)w.lane;
  r.lidx[i] = (int8_t)r.cached_index;
}

__device__ __forceinline__ void wp_zero(const WpRows& r, int from, int W) {
  if (r.pos == nullptr) return;
  for (int i = from; i < W; ++i) {
    r.pos[i * 3 + 0] = 0.0;
    r.pos[i * 3 + 1] = 0.0;
    r.pos[i * 3 + 2] = 0.0;
    r.heading[i] = 0.0f;
    r.width[i] = 0.0f;
    r.speed[i] = 0.0f;
    r.lid[i] = -1;
    r.lidx[i] = 0;
  }
}

// ---- the steps every emitter shares (waypoints_for, waypoints_tables_role, waypoints_emit_role) ----
// first waypoint of a path (of the vehicle's path 0: what the trip meter reads)
struct WpFirst {
  bool have;
  double x, y, h;
};

// One path into one output row: wp_rows, the interpolation with a wp_put sink, zeros behind the path, the row's wp_count
// byte.  `knots`: this thread's column of a [SMX_MAX_KNOTS][KSTRIDE] LDS scratch owned by the kernel.
// `kept` false: nothing is stored and the path is only walked (the caller enumerates its branchings), as far as its
// first waypoint when that is wanted.  `want_first`: the path's first waypoint goes to `*first` (which call sites name
// directly, or as nullptr: a pointer chosen at run time would keep the caller's WpFirst out of registers).
// `count_byte` false: the caller's row book holds the count.  `store` false: the developer switch SMX_DEBUG_SKIP & 32768,
// compute and do not store.  Returns the number of lanepoints on the path.
template <int KSTRIDE>
__device__ __forceinline__ int wp_emit_path(const KernelArgs& a, const RouteFilter& f, BranchState& bs, int start, size_t gid,
                                            double px, double py, int* knots, int slot, bool kept, bool want_first,
                                            WpFirst* first, bool count_byte = true, bool store = true) {
  const MapDev& m = a.map;
  const int P = a.cfg.wp_paths, W = a.cfg.wp_len, lookahead = a.cfg.wp_lookahead;
  if (!kept && !want_first)
    return equally_spaced_path(m, f, bs, start, lookahead, px, py, knots, KSTRIDE, 0, [&](int, const WaypointOut&) {});
  WpRows rows = wp_rows(a.out, gid, P, W, slot);
  if (!store) rows.pos = nullptr;
  const int n = equally_spaced_path(m, f, bs, start, lookahead, px, py, knots, KSTRIDE, kept ? W : 1,
                                    [&](int i, const WaypointOut& w) {
                                      if (want_first && i == 0) {
                                        first->have = true;
                                        first->x = w.x;
                                        first->y = w.y;
                                        first->h = w.heading;
                                      }
                                      if (kept) wp_put(m, rows, i, w);
                                    });
  if (kept) {
    wp_zero(rows, n < W ? n : W, W);
    if (count_byte) a.out.wp_count[gid * (P + 1) + 1 + slot] = (uint8_t)(n < W ? n : W);
  }
  return n;
}

// Closing a vehicle's rows: the rows of the paths that do not exist, spread over the team, and the path count (lane 0)
__device__ __forceinline__ void wp_close_rows(const KernelArgs& a, size_t gid, int p0, int n_paths_total) {
  const smx_outputs& o = a.out;
  const int P = a.cfg.wp_paths, W = a.cfg.wp_len;
  for (int slot = n_paths_total + ((p0 - n_paths_total) & (SMX_WP_LANES - 1)); slot < P; slot += SMX_WP_LANES) {
    wp_zero(wp_rows(o, gid, P, W, slot), 0, W);
    o.wp_count[gid * (P + 1) + 1 + slot] = 0;
  }
  if (p0 == 0) o.wp_count[gid * (P + 1)] = (uint8_t)(n_paths_total > 255 ? 255 : n_paths_total);
}

// Path 0 is the lowest started lane's first path: its first waypoint (`g`: every lane's own), for the whole team
__device__ __forceinline__ WpFirst team_first_waypoint(int started, const WpFirst& g, bool have) {
  const int src = started ? (__ffs(started) - 1) : 0;
  WpFirst fw;
  fw.have = have;
  fw.x = __shfl(g.x, src, SMX_WP_LANES);
  fw.y = __shfl(g.y, src, SMX_WP_LANES);
  fw.h = __shfl(g.h, src, SMX_WP_LANES);
  return fw;
}

// A lane branches inside the lookahead: paths are numbered lanes by index, branches depth-first, i.e. lane p's paths
// follow those of the lower lanes.  The counts are known (waypoints_for's first pass, k_wp_walk), so an exclusive prefix
// over the team gives every lane the numbers of its own paths, and each lane writes its own branches, with its own
// walks, into the right rows.  `start`: this lane's start lanepoint (< 0: no path starts here).  `in_place`: the row
// this lane's first path already stands in (waypoints_for's provisional one; -1: none).  Only a first path whose row
// was already the right one stays as written and is only walked, to learn the branchings the enumeration continues
// from: provisional rows are distinct (a lane's rank among the started lanes), so nobody else wrote there in the first
// pass, and whoever owns another lane's stale provisional row rewrites it here, later.  `first`: takes the first
// waypoint of path 0 if that path is written here (one in place keeps what the first pass learnt).  Returns the
// team's number of paths.
template <int KSTRIDE>
__device__ __forceinline__ int wp_emit_branches(const KernelArgs& a, const RouteFilter& f, size_t gid, int p0, double px,
                                                double py, int* knots, int start, int cnt, int in_place, WpFirst& first) {
  const int P = a.cfg.wp_paths;
  int n_paths_total;
  const int base = team_exclusive_prefix(cnt, p0, n_paths_total);
  const bool first_in_place = base == in_place;
  if (start >= 0 && base < P && !(cnt == 1 && first_in_place)) {
    BranchState bs;
    bs.reset();
    int idx = base;
    do {
      if (idx >= P) break;
      if (idx == base && first_in_place)
        wp_emit_path<KSTRIDE>(a, f, bs, start, gid, px, py, knots, 0, false, false, nullptr);
      else
        wp_emit_path<KSTRIDE>(a, f, bs, start, gid, px, py, knots, idx, true, idx == 0, &first);
      ++idx;
    } while (bs.advance());
  }
  return n_paths_total;
}

// Roads with more than four lanes: every path of the vehicle the long way (lanes by index, branches depth-first): every
// team lane walks every path to discover the branchings, lane (idx % 4) writes kept path idx.  Returns the number of
// paths; lane 0 of the team learns the first waypoint.
template <int KSTRIDE>
__device__ __forceinline__ int waypoints_long_way(const KernelArgs& a, const PathSeeds& seed, size_t gid, int p0, double px,
                                                  double py, int* knots, WpFirst& fw) {
  const int P = a.cfg.wp_paths;
  int idx = 0;
  for (int li = 0; li < seed.n_lanes; ++li) {
    const int st = seed_start(a.map, seed, li, px, py);
    if (st < 0) continue;
    BranchState bs;
    bs.reset();
    do {
      const bool kept = idx < P && (idx % SMX_WP_LANES) == p0;
      const bool first_path = (idx == 0 && p0 == 0);
      if (kept || first_path)
        wp_emit_path<KSTRIDE>(a, seed.f, bs, st, gid, px, py, knots, kept ? idx : 0, kept, first_path, &fw);
      else if (p0 == 0 || idx < P)
        wp_emit_path<KSTRIDE>(a, seed.f, bs, st, gid, px, py, knots, 0, false, false, nullptr);
      ++idx;
    } while (bs.advance() && (p0 == 0 || idx < P));
  }
  return __shfl(idx, 0, SMX_WP_LANES);  // lane 0 counts them all
}

// Trip meter (sensors.py:880-947) and reward = its increment (agent_manager.py:233-234): lane 0 of the team.
// The meter's words as loaded (the emit-parallel form loads them early, with everything else of the vehicle):
struct TripMeter {
  double dist, last_dist;         // the total, and what it was when this tick began
  double trip_x, trip_y, trip_h;  // the waypoint the meter last advanced to
  bool has_wp;                    // ... if there is one
};

__device__ __forceinline__ TripMeter trip_meter_of(double dist, double trip_x, double trip_y, double trip_h, bool has_wp) {
  TripMeter t;
  t.dist = t.last_dist = dist;
  t.trip_x = trip_x;
  t.trip_y = trip_y;
  t.trip_h = trip_h;
  t.has_wp = has_wp;
  return t;
}

// A new vehicle (TripMeterSensor.__init__): the meter's waypoint is the first one of the lowest lane, lookahead-1 path,
// no route; it goes to the state rows.  Returns whether there is one.
template <int KSTRIDE>
__device__ __forceinline__ bool trip_meter_start(const KernelArgs& a, size_t gid, size_t total, double px, double py, int* knots) {
  bool has_wp = false;
  const int ts = a.st.facts_i32[(size_t)SMX_FI_TRIP_START * total + gid];
  if (ts >= 0) {
    BranchState bs;
    bs.reset();
    RouteFilter nof;
    nof.none();
    equally_spaced_path(a.map, nof, bs, ts, 1, px, py, knots, KSTRIDE, 1, [&](int, const WaypointOut& w) {
      SF(SMX_S_TRIP_X) = w.x;
      SF(SMX_S_TRIP_Y) = w.y;
      SF(SMX_S_TRIP_H) = w.heading;
      has_wp = true;
    });
  }
  return has_wp;
}

// The first waypoint of path 0, when it counts (trip_counts_waypoint), is appended: the meter moves on to it once it
// lies more than half a metre away.  (The new waypoint goes straight to the state rows: held in the struct until
// trip_meter_store it cost k_waypoints_tables two registers.)
__device__ __forceinline__ void trip_meter_advance(const KernelArgs& a, size_t gid, size_t total, TripMeter& t, const WpFirst& fw) {
  if (!t.has_wp) {
    SF(SMX_S_TRIP_X) = fw.x;
    SF(SMX_S_TRIP_Y) = fw.y;
    SF(SMX_S_TRIP_H) = fw.h;
    t.has_wp = true;
  } else {
    double dx = fw.x - t.trip_x, dy = fw.y - t.trip_y;
    double nrm = sqrt(dx * dx + dy * dy);
    if (nrm > 0.5) {
      double hvx, hvy;
      radians_to_vec(t.trip_h, hvx, hvy);
      double dot = hvx * dx + hvy * dy;
      double sgn = dot > 0.0 ? 1.0 : (dot < 0.0 ? -1.0 : 0.0);
      t.dist += sgn * nrm;
      SF(SMX_S_TRIP_X) = fw.x;
      SF(SMX_S_TRIP_Y) = fw.y;
      SF(SMX_S_TRIP_H) = fw.h;
    }
  }
}

__device__ __forceinline__ void trip_meter_store(const KernelArgs& a, size_t gid, size_t total, const TripMeter& t) {
  const smx_outputs& o = a.out;
  SF(SMX_S_DIST) = t.dist;
  o.dist[gid] = t.dist;
  if (!a.keep_reward_done) {
    o.reward[gid] = t.dist - t.last_dist;
    if (o.learner) o.learner[gid] = (float)(t.dist - t.last_dist);
  }
  // the flags word itself is not written here (the observe role owns it)
  a.st.facts_i32[(size_t)SMX_FI_TRIP_HAS_WP * total + gid] = t.has_wp ? 1 : 0;
}

// The three in turn, on the state rows (the serial emitter, the staged form): the meter's waypoint is loaded behind
// the start, which may just have written it, and only when it is needed
template <int KSTRIDE>
__device__ __forceinline__ void trip_meter_update(const KernelArgs& a, size_t gid, size_t total, int flags, double px, double py,
                                                  int* knots, const WpFirst& fw) {
  double dist = SF(SMX_S_DIST);
  bool has_wp = a.st.facts_i32[(size_t)SMX_FI_TRIP_HAS_WP * total + gid] != 0;
  if (flags & SMX_F_FIRST) {
    has_wp = trip_meter_start<KSTRIDE>(a, gid, total, px, py, knots);
    dist = 0.0;
  }
  const bool counts = fw.have && trip_counts_waypoint(a, a.map, gid, total);
  TripMeter t = trip_meter_of(dist, counts ? SF(SMX_S_TRIP_X) : 0.0, counts ? SF(SMX_S_TRIP_Y) : 0.0,
                              counts ? SF(SMX_S_TRIP_H) : 0.0, has_wp);
  if (counts) trip_meter_advance(a, gid, total, t, fw);
  trip_meter_store(a, gid, total, t);
}

// The serial emitter: every row of the vehicle and its trip meter, a team of SMX_WP_LANES lanes
template <int KSTRIDE>
__device__ __forceinline__ void waypoints_for(const KernelArgs& a, const size_t gid, int* knots) {
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const int p0 = threadIdx.x % SMX_WP_LANES;
  if (gid >= total) return;  // whole teams leave together
  if (SMX_SKIP(a, 16384)) return;
  SMX_TSTAMP(tw0);
  int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE) || (flags & SMX_F_SOCIAL) || (a.first_only && !(flags & SMX_F_FIRST))) return;
  const bool wp_on = (c.sensors & SMX_SENSOR_WAYPOINTS) != 0;
  const int P = c.wp_paths;
  const VehState s = load_vehicle(a, gid, total);
  const double px = s.x, py = s.y;

  WpFirst fw = {false, 0.0, 0.0, 0.0};  // first waypoint of path 0 (trip meter), valid on team lane 0
  if (!wp_on) {
    // only the first waypoint of the first path is needed (trip meter)
    const int os = a.st.facts_i32[(size_t)SMX_FI_OBS_START * total + gid];
    if (p0 == 0 && os >= 0) {
      BranchState bs;
      bs.reset();
      RouteFilter nof;
      nof.none();
      equally_spaced_path(m, nof, bs, os, 1, px, py, knots, KSTRIDE, 1, [&](int, const WaypointOut& w) {
        fw.have = true;
        fw.x = w.x;
        fw.y = w.y;
        fw.h = w.heading;
      });
    }
  } else {
    const PathSeeds seed = load_seeds(a, gid, total);
    int n_paths_total = 0;
    SMX_TSTAMP(tw1);
    SMX_TACC(0, tw0, tw1);
    if (seed.road >= 0 && !SMX_SKIP(a, 16)) {
      // ---- the guess: seed lane p holds exactly one path
      const int start = (p0 < seed.n_lanes) ? seed_start(m, seed, p0, px, py) : -1;
      const int started = team_or(start >= 0 ? (1 << p0) : 0);
      const int prov = __popc(started & ((1 << p0) - 1));
      int cnt = 0;
      WpFirst g = {false, 0.0, 0.0, 0.0};  // first waypoint of this lane's first path
      if (start >= 0) {
        BranchState bs;
        bs.reset();
        do {
          if (cnt == 0 && prov < P)
            wp_emit_path<KSTRIDE>(a, seed.f, bs, start, gid, px, py, knots, prov, true, true, &g, true, !SMX_SKIP(a, 32768));
          else
            wp_emit_path<KSTRIDE>(a, seed.f, bs, start, gid, px, py, knots, 0, false, false, nullptr);
          ++cnt;
        } while (bs.advance());
      }
      const bool branching = team_or(cnt > 1 ? 1 : 0) != 0;
      if (seed.n_lanes > SMX_WP_LANES) {
        n_paths_total = waypoints_long_way<KSTRIDE>(a, seed, gid, p0, px, py, knots, fw);
      } else {
        // the guess held (path numbers are the provisional ones) unless a lane branches inside the lookahead
        n_paths_total = branching ? wp_emit_branches<KSTRIDE>(a, seed.f, gid, p0, px, py, knots, start, cnt, prov, g)
                                  : __popc(started);
        fw = team_first_waypoint(started, g, n_paths_total > 0);
      }
    }
    SMX_TSTAMP(tw2);
    SMX_TACC(1, tw1, tw2);
    wp_close_rows(a, gid, p0, n_paths_total);
  }

  if (p0 != 0) return;
  trip_meter_update<KSTRIDE>(a, gid, total, flags, px, py, knots, fw);
  SMX_TSTAMP(tw3);
  SMX_TACC(3, tw0, tw3);
}

__device__ __forceinline__ void waypoints_role(const KernelArgs& a, const int block) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  waypoints_for<SMX_BLOCK>(a, ((size_t)block * SMX_BLOCK + threadIdx.x) / SMX_WP_LANES, knot_scratch + threadIdx.x);
}

// =================================================================================
// waypoints role, staged form (large batches): the same rows as waypoints_for, written as whole
// contiguous pieces.  The chain walks are k_wp_walk's (one lane per path, nothing else, many wavefronts per
// SIMD); this kernel re-reads the knots with independent loads.  A workgroup = one wavefront = 16 vehicles x
// 4 team lanes:
//   1. number — the team exchanges what k_wp_walk found; when no lane branches inside the lookahead (almost
//               always) path numbers are the lanes' ranks among the started lanes, and every output row of
//               the vehicle is bound to a team lane, or to "zeros";
//   2. stage  — every lane interpolates its own path (interpolate_knots: the serial emitter's arithmetic,
//               one path per lane, all lanes busy) into an LDS stage [waypoint][lane] of 16-byte cells;
//   3. copy   — the wavefront's lanes sweep the 16 x P x W waypoint slots of its vehicles in memory order
//               (rows of consecutive vehicles are adjacent in every output array): lane l takes element
//               e = 64 k + l and copies its cell, or zeros.  A store instruction writes 64 consecutive
//               elements.
// Steps 2-3 run twice over the same stage: positions (x, y: 16 bytes), then heading / lane width / speed limit
// / lane id / lane index (packed into 16 bytes); the interpolation is cheap next to a second stage's LDS.
// Teams that need more — a branching inside the lookahead, a road with more than four lanes, a knot list
// cut at SMX_WPK_CAP — write their rows afterwards with the serial emitter's own steps (wp_emit_branches,
// waypoints_long_way, wp_emit_path, wp_close_rows), exactly as waypoints_for does; their rows are skipped in step 3.
// =================================================================================
// floor(e / d) for 0 <= e < 4096, 1 <= d <= 64, rcp = 1.0f / d: (e + 0.5) / d is at least 0.5 / d away from an integer,
// the float32 product is off by less than 4096 / d * 2^-22
__device__ __forceinline__ int small_quotient(int e, float rcp) { return (int)(((float)e + 0.5f) * rcp); }
#define SMX_WPT_VEHICLES (SMX_BLOCK / SMX_WP_LANES)
enum { SMX_ROW_SKIP = -2, SMX_ROW_ZERO = -1 };

struct WpRowBook {  // which table column feeds which output row of the workgroup's vehicles
  short src[SMX_WPT_VEHICLES * SMX_WPT_MAX_PATHS];          // column, SMX_ROW_ZERO or SMX_ROW_SKIP
  unsigned char count[SMX_WPT_VEHICLES * SMX_WPT_MAX_PATHS];  // wp_count of the row
  unsigned char paths[SMX_WPT_VEHICLES];                     // total number of paths of the vehicle
  unsigned char tabled[SMX_WPT_VEHICLES];                    // the vehicle's counts come from this book
  unsigned int veh[SMX_WPT_VEHICLES];                        // the vehicle of team v (launch_vehicle: the alive list)
};

// A team opens its vehicle's part of the book.  `tabled`: the vehicle's rows and counts leave through the book, rows
// without a path as zeros; otherwise (a dead / absent vehicle, a team that goes the serial way) they are not the
// sweep's to write.  The caller's barrier comes before the path lanes bind their rows.
__device__ __forceinline__ void wp_book_open(WpRowBook& book, int v, int p0, int P, size_t gid, size_t total, bool tabled,
                                             int n_paths) {
  if (p0 == 0) {
    book.veh[v] = (unsigned int)(gid < total ? gid : 0);
    book.tabled[v] = tabled ? 1 : 0;
    book.paths[v] = (unsigned char)n_paths;
  }
  for (int slot = p0; slot < P; slot += SMX_WP_LANES) {
    book.src[v * P + slot] = (short)(tabled ? SMX_ROW_ZERO : SMX_ROW_SKIP);
    book.count[v * P + slot] = 0;
  }
}

// wp_count of the tabled vehicles: [vehicle][0] = number of paths, [1 + slot] = waypoints kept of the path in that row
__device__ __forceinline__ void wp_book_store_counts(const WpRowBook& book, uint8_t* wp_count, int P) {
  const int cells = SMX_WPT_VEHICLES * (P + 1);
  for (int e = threadIdx.x; e < cells; e += SMX_BLOCK) {
    const int vv = e / (P + 1), qq = e - vv * (P + 1);
    if (!book.tabled[vv]) continue;
    wp_count[(size_t)book.veh[vv] * (P + 1) + qq] = qq == 0 ? book.paths[vv] : book.count[vv * P + qq - 1];
  }
}

// Element e of the workgroup's rows, advanced by SMX_BLOCK: e = row * W + i, and row = vv * P + slot (team vv's path
// row `slot`) where the rows swept are the book's own (a sweep of a list of rows reads `row` as its place in the list)
struct WpCursor {
  int row, i, vv, slot;
  int W, P, drow, di;
  __device__ __forceinline__ WpCursor(int W_, int P_) : W(W_), P(P_) {
    row = threadIdx.x / W;
    i = threadIdx.x - row * W;
    vv = row / P;
    slot = row - vv * P;
    drow = SMX_BLOCK / W;
    di = SMX_BLOCK - drow * W;
  }
  __device__ __forceinline__ void advance() {
    row += drow;
    slot += drow;
    i += di;
    if (i >= W) {
      i -= W;
      ++row;
      ++slot;
    }
    while (slot >= P) {
      slot -= P;
      ++vv;
    }
  }
};

// How the team numbers its paths from what k_wp_walk found (the staged and the emit-parallel form)
struct WpTeam {
  int started;       // bit p: a path starts on seed lane p
  int prov;          // this lane's path number if nobody branches
  int n_paths;       // ... and the vehicle's number of paths then
  bool branching;    // a lane branches inside the lookahead
  bool long_way;     // a road with more than four lanes
  bool serial_team;  // the team has to number its paths the long way: its rows do not come from the table
  bool staged;       // this lane's path leaves through the table (or the serial emitter alone)
  bool listed;       // ... k_wp_walk's knot list holds all its knots
  bool my_row;       // ... and one of the kept rows holds it
};
// (`seeded`, `n_lanes` and therefore long_way, branching and serial_team are uniform in the team)
__device__ __forceinline__ WpTeam wp_team_number(bool seeded, int n_lanes, int p0, int n_first, int nk, int cnt, int P) {
  WpTeam t;
  t.long_way = seeded && n_lanes > SMX_WP_LANES;
  t.started = team_or(n_first > 0 ? (1 << p0) : 0);
  t.prov = __popc(t.started & ((1 << p0) - 1));
  t.branching = team_or(cnt > 1 ? 1 : 0) != 0;
  t.serial_team = seeded && (t.long_way || t.branching);
  t.n_paths = __popc(t.started);
  t.staged = n_first > 0 && !t.serial_team;
  t.listed = nk <= SMX_WPK_CAP;
  t.my_row = t.staged && t.prov < P;
  return t;
}

// k_alive_list: the alive vehicles of the tick, compacted (large batches).  Late in an episode most agents of an env
// are gone while the env waits for its last one (hiway_env.py:258-261): a per-vehicle team kernel then runs its
// wavefronts a quarter to a half full.  Order within the list is that of the atomics (it varies from run to run;
// every result is indexed by vehicle, never by list position).  The counter of the next tick is zeroed here.
#define SMX_ALIVE_BLOCK 1024
__global__ void __launch_bounds__(SMX_ALIVE_BLOCK) k_alive_list(const KernelArgs a, int32_t* list, int32_t* count, int32_t* count_next,
                                                                  int32_t* slow_next) {
  // one atomic per workgroup of 1024 (a wavefront each was 2 048 atomics on one counter: 28 us at 131 k vehicles)
  __shared__ int wave_base[SMX_ALIVE_BLOCK / 64];
  __shared__ int group_base;
  const size_t total = (size_t)a.cfg.num_envs * a.cfg.num_vehicles;
  const size_t gid = (size_t)blockIdx.x * SMX_ALIVE_BLOCK + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool alive = gid < total && (a.st.flags[gid] & SMX_F_ALIVE);
  const unsigned long long mask = __ballot(alive);
  if (gid == 0) {
    *count_next = 0;
    slow_next[0] = slow_next[1] = slow_next[2] = slow_next[3] = 0;  // the slow lists of the next tick's fast kernels
  }
  if (lane == 0) wave_base[wave] = __popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < SMX_ALIVE_BLOCK / 64; ++w) {
      const int n = wave_base[w];
      wave_base[w] = sum;
      sum += n;
    }
    group_base = sum > 0 ? atomicAdd(count, sum) : 0;
  }
  __syncthreads();
  if (alive) list[group_base + wave_base[wave] + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)gid;
}

// k_wp_walk: the chain walks of the waypoints sensor, one lane per (vehicle, seed lane) and nothing else —
// no LDS, few registers, so that many wavefronts per SIMD hide the dependent loads.  Leaves the knot list of
// the seed lane's first path and the number of paths that start there (KnotLists).
// (`honour_pending`: pass over a vehicle whose seeds the slow chain is still looking for — k_scan_fast; the slow chain's
// own walk and the walk of the reset pass's new vehicles take every vehicle they are given)
__device__ __forceinline__ void wp_walk_for(const KernelArgs& a, const size_t gid, const int p0, const bool honour_pending,
                                            const bool whatever_the_pass = false) {
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t paths = total * SMX_WP_LANES;
  if (gid >= total) return;
  const size_t path = gid * SMX_WP_LANES + p0;
  const int flags = a.st.flags[gid];
  int n = 0, nk = 0, cnt = 0;
  double D = 0.0;
  // (nothing of a pending vehicle's lists is touched here: the slow chain writes them meanwhile, on another stream)
  if (honour_pending && a.seed_pending != nullptr && a.seed_pending[gid]) return;
  if ((flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (!a.first_only || whatever_the_pass || (flags & SMX_F_FIRST))) {
    const PathSeeds seed = load_seeds(a, gid, total);
    if (seed.road >= 0 && seed.n_lanes <= SMX_WP_LANES && p0 < seed.n_lanes) {
      const double px = SF(SMX_S_X), py = SF(SMX_S_Y);
      const int start = seed_start(m, seed, p0, px, py);
      if (start >= 0) {
        a.knots.idx[path] = start;
        const KnotListHead w = walk_knot_list(m, seed.f, start, c.wp_lookahead, SMX_CTRL_WPS, px, py,
                                              [&](int k, int idx, double) { a.knots.idx[(size_t)k * paths + path] = idx; });
        n = w.n;
        nk = w.nk;
        D = w.D;
        cnt = w.cnt;
        a.knots.nk16[path] = (uint8_t)w.nk16;
        a.knots.end16[path] = w.end16;
        a.knots.key[path] = start;
        a.knots.key[paths + path] = seed.f.n > 0 ? seed.f.road[0] : -1;
        a.knots.key[2 * paths + path] = seed.f.n > 1 ? seed.f.road[1] : -1;
      }
    }
  }
  a.knots.n[path] = (int16_t)n;
  a.knots.nk[path] = (int16_t)nk;
  a.knots.cnt[path] = (uint8_t)cnt;
  a.knots.D[path] = D;
  if (n == 0) a.knots.key[path] = -1;  // nothing here for the next tick's controller to reuse
}

// The map's knot table, once per map: one lane per lanepoint walks its row (build_knot_row: wp_walk_for's own walk).
// stats: rows tabled, rows that touch their start road only.
__global__ void __launch_bounds__(SMX_BLOCK) k_knot_table(const MapDev m, const int lookahead, KnotRow* rows, int32_t* stats) {
  const int lp = (int)(blockIdx.x * SMX_BLOCK + threadIdx.x);
  if (lp >= m.n_lanepoints) return;
  KnotRow row;
  build_knot_row(m, lp, lookahead, SMX_CTRL_WPS, row);
  rows[lp] = row;
  if (row.flags & SMX_KROW_TABLED) atomicAdd(stats, 1);
  if (row.flags & SMX_KROW_SINGLE_ROAD) atomicAdd(stats + 1, 1);
}

__global__ void __launch_bounds__(SMX_BLOCK) k_wp_walk(const KernelArgs a) {
  SMX_TSTAMP(span0);
  const size_t total = (size_t)a.cfg.num_envs * a.cfg.num_vehicles;
  const size_t lane_no = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  wp_walk_for(a, launch_vehicle(a, lane_no / SMX_WP_LANES, total), (int)(lane_no % SMX_WP_LANES), true);
  SMX_TSTAMP(span1);
  SMX_TSPAN(3, span0, span1);
}

// the slow chain's vehicles (their seeds come from k_scan_listed): a fixed grid striding the slow list.  Their rows
// leave through k_waypoints_listed; the lists are for the next tick's k_control_fast.
__global__ void __launch_bounds__(SMX_BLOCK) k_wp_walk_listed(const KernelArgs a) {
  const int count = *a.slow_count;
  constexpr int VPB = SMX_BLOCK / SMX_WP_LANES;
  for (int i = (int)blockIdx.x * VPB + (int)threadIdx.x / SMX_WP_LANES; i < count; i += (int)gridDim.x * VPB)
    wp_walk_for(a, (size_t)a.slow_list[i], (int)threadIdx.x % SMX_WP_LANES, false);
}

struct __align__(16) WpStageCell {  // second pass: everything of a waypoint but its position
  float heading, width, speed;
  short lane;
  signed char lane_index;
  signed char pad;
};

__device__ __forceinline__ void waypoints_tables_role(const KernelArgs& a, const int block) {
  extern __shared__ __align__(16) unsigned char stage_raw[];  // [wp_len][SMX_BLOCK] cells of 16 bytes
  __shared__ WpRowBook book;
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const smx_outputs& o = a.out;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const int P = c.wp_paths, W = c.wp_len;
  const int p0 = threadIdx.x % SMX_WP_LANES, v = threadIdx.x / SMX_WP_LANES;
  // team v works on the v-th vehicle of the workgroup's sixteen launch slots (alive vehicles only when the tick
  // has its list): the rows of a vehicle are contiguous in the outputs, the vehicles of a workgroup need not be
  const size_t gid = launch_vehicle(a, (size_t)block * SMX_WPT_VEHICLES + v, total);
  const size_t path = gid * SMX_WP_LANES + p0, paths = total * SMX_WP_LANES;
  const int col = threadIdx.x;
  SMX_TSTAMP(tw0);
  int flags = gid < total ? a.st.flags[gid] : 0;
  const bool live = gid < total && (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (!a.first_only || (flags & SMX_F_FIRST));
  double px = 0.0, py = 0.0;
  PathSeeds seed;
  seed.road = -1;
  seed.n_lanes = 0;
  seed.f.none();
  int n_first = 0, nk = 0, cnt = 0;
  double D = 0.0;
  if (live) {
    px = SF(SMX_S_X);
    py = SF(SMX_S_Y);
    seed = load_seeds(a, gid, total);
    n_first = a.knots.n[path];  // what k_wp_walk found on seed lane p0 (0: no path starts there)
    nk = a.knots.nk[path];
    cnt = a.knots.cnt[path];
    D = a.knots.D[path];
  }
  SMX_TSTAMP(tw1);
  SMX_TACC(0, tw0, tw1);
  // ---- 1. number the paths; the team's rows come from the stage unless it has to number them the long way
  const bool seeded = live && seed.road >= 0;
  const WpTeam tm = wp_team_number(seeded, seed.n_lanes, p0, n_first, nk, cnt, P);
  wp_book_open(book, v, p0, P, gid, total, live && !tm.serial_team, seeded ? tm.n_paths : 0);
  __syncthreads();  // (one wavefront: orders the LDS writes of the team's other lanes)
  if (tm.my_row) {
    book.src[v * P + tm.prov] = (short)(tm.listed ? col : SMX_ROW_SKIP);
    book.count[v * P + tm.prov] = (unsigned char)min(n_first, W);
  }
  // ---- 2 + 3, positions
  const bool pre = tm.staged && tm.listed;
  const smx_lp_rec r0 = pre ? load_lp(m, a.knots.idx[path], 46) : smx_lp_rec{};
  auto fetch = [&](int k) { return a.knots.idx[(size_t)(k + 1) * paths + path]; };
  // the knots of the path into registers, every load issued before anything waits for one (paths of more
  // knots than SMX_WPT_PRELOAD interpolate straight from the list, a dependent load per knot)
  constexpr int KP = SMX_WPT_PRELOAD;
  double kx[KP], ky[KP], kh[KP], kw[KP], ks_[KP];
  int kl[KP];
  double w0 = 0.0, s0 = 0.0;
  {
    int kid[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) kid[k] = (pre && k < nk) ? fetch(k) : 0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const smx_lp_rec* r = m.lp_rec + kid[k];
      const bool have = pre && k < nk;
      kx[k] = have ? r->x : 0.0;
      ky[k] = have ? r->y : 0.0;
      kh[k] = have ? r->heading : 0.0;
      kl[k] = have ? r->lane : 0;
    }
    if (pre) {
      w0 = m.lane_width[r0.lane];
      s0 = m.lane_speed[r0.lane];
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      // the tables are read only where the lane changes (few lanes of the wavefront ask at all)
      const bool ask = pre && k < nk && kl[k] != (k == 0 ? (int)r0.lane : kl[k > 0 ? k - 1 : 0]);
      kw[k] = ask ? m.lane_width[kl[k]] : 0.0;
      ks_[k] = ask ? m.lane_speed[kl[k]] : 0.0;
    }
  }
  const int elems = SMX_WPT_VEHICLES * P * W;
  WpFirst g = {false, 0.0, 0.0, 0.0};  // first waypoint of this lane's path
  {
    double2* stage = reinterpret_cast<double2*>(stage_raw);
    auto put_xy = [&](int i, const WaypointOut& w) {
      if (i == 0) {
        g.x = w.x;
        g.y = w.y;
      }
      stage[i * SMX_BLOCK + col] = make_double2(w.x, w.y);
    };
    if (pre)
      interpolate_knots_preloaded<KP>(m, r0, w0, s0, nk, n_first, D, px, py, tm.my_row ? W : 1, kx, ky, kh, kl, kw, ks_, fetch, put_xy);
    __syncthreads();
    SMX_TSTAMP(tw2);
    SMX_TACC(1, tw1, tw2);
    WpCursor cur(W, P);
    for (int e = threadIdx.x; e < elems; e += SMX_BLOCK, cur.advance()) {
      const int src = book.src[cur.row];
      if (src != SMX_ROW_SKIP) {
        double2 xy = make_double2(0.0, 0.0);
        if (src >= 0 && cur.i < (int)book.count[cur.row]) xy = stage[cur.i * SMX_BLOCK + src];
        double* dst = o.wp_pos + (((size_t)book.veh[cur.vv] * P + cur.slot) * W + cur.i) * 3;
        dst[0] = xy.x;
        dst[1] = xy.y;
        dst[2] = 0.0;
      }
    }
    __syncthreads();  // the stage is reused
    SMX_TSTAMP(tw2b);
    SMX_TACC(24, tw2, tw2b);
  }
  SMX_TSTAMP(tw3);
  // ---- 2 + 3, the other fields
  {
    WpStageCell* stage = reinterpret_cast<WpStageCell*>(stage_raw);
    if (pre) {
      int cached_lane = -1, cached_index = 0;  // consecutive waypoints mostly share their lane
      auto put_rest = [&](int i, const WaypointOut& w) {
        if (i == 0) g.h = w.heading;
        if (w.lane != cached_lane) {
          cached_lane = w.lane;
          cached_index = m.lane_index[w.lane];
        }
        WpStageCell cell;
        cell.heading = (float)w.heading;
        cell.width = (float)w.width;
        cell.speed = (float)w.speed;
        cell.lane = (short)w.lane;
        cell.lane_index = (signed char)cached_index;
        cell.pad = 0;
        stage[i * SMX_BLOCK + col] = cell;
      };
      interpolate_knots_preloaded<KP>(m, r0, w0, s0, nk, n_first, D, px, py, tm.my_row ? W : 1, kx, ky, kh, kl, kw, ks_, fetch, put_rest);
    }
    __syncthreads();
    SMX_TSTAMP(tw3b);
    SMX_TACC(25, tw3, tw3b);
    WpCursor cur(W, P);
    for (int e = threadIdx.x; e < elems; e += SMX_BLOCK, cur.advance()) {
      const int src = book.src[cur.row];
      if (src != SMX_ROW_SKIP) {
        WpStageCell cell;
        cell.heading = 0.0f;
        cell.width = 0.0f;
        cell.speed = 0.0f;
        cell.lane = -1;
        cell.lane_index = 0;
        if (src >= 0 && cur.i < (int)book.count[cur.row]) cell = stage[cur.i * SMX_BLOCK + src];
        const size_t q = ((size_t)book.veh[cur.vv] * P + cur.slot) * W + cur.i;
        o.wp_heading[q] = cell.heading;
        o.wp_lane_width[q] = cell.width;
        o.wp_speed_limit[q] = cell.speed;
        o.wp_lane_id[q] = cell.lane;
        o.wp_lane_index[q] = cell.lane_index;
      }
    }
    wp_book_store_counts(book, o.wp_count, P);
    SMX_TSTAMP(tw3c);
    SMX_TACC(26, tw3b, tw3c);
  }
  __syncthreads();  // the stage is done with: its memory becomes the serial emitter's knot scratch
  SMX_TSTAMP(tw4);
  SMX_TACC(2, tw3, tw4);
  int* knots = reinterpret_cast<int*>(stage_raw) + threadIdx.x;
  WpFirst fw = {false, 0.0, 0.0, 0.0};
  if (live) {
    if (tm.serial_team) {
      // the team's rows with the serial emitter, exactly as waypoints_for writes them (its own walks: the knot list
      // only holds the first path of a lane, whose start k_wp_walk left)
      int n_paths_total;
      if (tm.long_way) {
        n_paths_total = waypoints_long_way<SMX_BLOCK>(a, seed, gid, p0, px, py, knots, fw);
      } else {
        n_paths_total = wp_emit_branches<SMX_BLOCK>(a, seed.f, gid, p0, px, py, knots, cnt > 0 ? a.knots.idx[path] : -1, cnt, -1, g);
        fw = team_first_waypoint(tm.started, g, n_paths_total > 0);
      }
      wp_close_rows(a, gid, p0, n_paths_total);
    } else {
      if (tm.staged && !tm.listed) {
        // more knots than the list holds: this path leaves through the serial emitter (its own walk; the book has its count)
        BranchState bs;
        bs.reset();
        wp_emit_path<SMX_BLOCK>(a, seed.f, bs, a.knots.idx[path], gid, px, py, knots, tm.my_row ? tm.prov : 0, tm.my_row, true, &g, false);
      }
      fw = team_first_waypoint(tm.started, g, tm.n_paths > 0);
    }
  }
  SMX_TSTAMP(tw5);
  SMX_TACC(5, tw4, tw5);
  if (live && p0 == 0) trip_meter_update<SMX_BLOCK>(a, gid, total, flags, px, py, knots, fw);
  SMX_TSTAMP(tw6);
  SMX_TACC(3, tw0, tw6);
}

// =================================================================================
// waypoints role, emit-parallel form (large batches, round 3): the same rows as waypoints_tables_role, one lane per
// WAYPOINT instead of one lane per path.
//   The staged form interpolates one path per lane: 64 paths of a wavefront meet their knots at different
// waypoints, so the wavefront runs every knot's arithmetic and the longest run of waypoints of every knot interval
// (~50 emit rounds for 20 waypoints), twice (two 16-byte stage passes), and then copies the stage out element by
// element: 7.8 k vector instructions per wavefront with 20 KB of LDS (two wavefronts per SIMD).
//   Here a path lane only walks its knots ONCE for what is sequential by nature — the running arclength and the
// running heading unwrap, in the reference's order of additions — and leaves the knots it needs for its W waypoints
// in an LDS pool shared by the workgroup's paths (a path on a straight needs two records, one in a bend ten:
// records are handed out by a prefix sum over the wavefront).  Then the wavefront sweeps its 16 x P x W waypoint
// slots in memory order: a lane finds its waypoint's knot interval in the path's records, takes np.interp's slope
// from the two knots and stores the waypoint straight from registers — every store instruction writes consecutive
// elements, no stage, no divergence between lanes beyond the interval search.
//   Same expressions, same bits: t_i, (q - j) / (cum_q - cum_j), slope * (t - cum_j) + j, the lane rules.
// Vehicles with a path the pool cannot hold (more knots than SMX_WPE_KNOTS inside the kept waypoints, a pool
// overflow) or whose team numbers its paths the long way go to a slow list and through the serial emitter of
// k_waypoints_listed (waypoints_for: its own walks, every row, the trip meter): a serial tail inside this kernel would
// hold its whole wavefront, and its registers would set this kernel's occupancy.
// =================================================================================
#define SMX_WPE_KNOTS 10  // knots after the start a path lane holds in registers
// knot records per workgroup (64 paths; loop: 48 paths of 5.5 records on average, sigma 14).  A workgroup whose paths need
// more sends the teams that do not fit to the slow list, whose kernel is a launch of pure latency at the end of the tick's
// longest chain: at 320 a dozen workgroups of 8 192 overflowed per tick (76 us each tick for 200 vehicles); two sweeps of
// the pool inside the kernel kept the knots in registers across the sweep (256 registers, one wavefront per SIMD).
#ifndef SMX_WPE_POOL  // (a developer build with a small pool drives most paths through the overflow area: tests)
#define SMX_WPE_POOL 352
#endif
struct __align__(8) WpKnot {
  double x, y, h, cum;  // position, unwrapped heading, arclength from the projected start
};
struct WpKnotLanes {
  short lane, strict;   // the knot's lane; lane of the last knot with an arclength strictly below this one's
};
// the overflow area of one workgroup: per column SMX_WPE_KNOTS + 1 records, then as many lane pairs
#define SMX_WPE_SPILL_GROUP_BYTES ((size_t)SMX_BLOCK * (SMX_WPE_KNOTS + 1) * (sizeof(WpKnot) + sizeof(WpKnotLanes)))

__device__ __forceinline__ void waypoints_emit_role(const KernelArgs& a, const int block) {
  // 15.6 KB of LDS in all: ten workgroups per CU (its registers allow twelve: three wavefronts per SIMD)
  __shared__ WpKnot pool[SMX_WPE_POOL];
  __shared__ WpKnotLanes pool_lanes[SMX_WPE_POOL];
  __shared__ WpRowBook book;
  __shared__ double hdr_step[SMX_BLOCK], hdr_D[SMX_BLOCK];
  __shared__ unsigned short hdr_off[SMX_BLOCK];
  __shared__ unsigned char hdr_nrec[SMX_BLOCK], hdr_n[SMX_BLOCK];
  // lane width / speed limit / lane index of the path's start lane, and whether every knot held lies on that lane (almost
  // always): the waypoint lanes then need no table look-up behind their interval search
  __shared__ float hdr_w0[SMX_BLOCK], hdr_s0[SMX_BLOCK];  // (as they leave: the rows hold them as float32)
  __shared__ signed char hdr_li0[SMX_BLOCK];
  __shared__ unsigned char hdr_one_lane[SMX_BLOCK];
  __shared__ double first_wp[SMX_WPT_VEHICLES][3];
  __shared__ unsigned char rows_live[SMX_WPT_VEHICLES * SMX_WPT_MAX_PATHS], rows_zero[SMX_WPT_VEHICLES * SMX_WPT_MAX_PATHS];
  __shared__ unsigned char rows_spill[SMX_WPT_VEHICLES * SMX_WPT_MAX_PATHS];  // rows whose knots lie in the overflow area
  __shared__ unsigned char hdr_spill[SMX_BLOCK];
  static_assert(SMX_WPT_VEHICLES * SMX_WPT_MAX_PATHS <= 256, "row numbers are bytes");
  static_assert(sizeof(WpKnot) == 32 && sizeof(WpKnotLanes) == 4, "WpKnot layout");
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const smx_outputs& o = a.out;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const int P = c.wp_paths, W = c.wp_len;
  const int p0 = threadIdx.x % SMX_WP_LANES, v = threadIdx.x / SMX_WP_LANES;
  const size_t gid = launch_vehicle(a, (size_t)block * SMX_WPT_VEHICLES + v, total);
  const size_t path = gid * SMX_WP_LANES + p0, paths = total * SMX_WP_LANES;
  const int col = threadIdx.x;
  // Every load whose address only needs the vehicle is issued here, together and whatever the flags say (a dead slot's
  // words are loaded and dropped): the kernel runs two wavefronts per SIMD, and flags -> seeds -> knot list -> records
  // -> trip meter taken one after the other was five round trips of 2-4 us each under load (round 3: 85 of its 217 us).
  constexpr int KP = SMX_WPE_KNOTS;
  SMX_TSTAMP(te0);
  const bool in_range = gid < total;
  const size_t g = in_range ? gid : 0, pth = g * SMX_WP_LANES + p0;
  int flags = a.st.flags[g];
  const int pend = a.seed_pending != nullptr ? (int)a.seed_pending[g] : 0;
  double px = a.st.f64[(size_t)SMX_S_X * total + g], py = a.st.f64[(size_t)SMX_S_Y * total + g];
  PathSeeds seed = load_seeds(a, g, total);
  const bool table = a.knot_table != nullptr;
  int n_first, nk, cnt, kid0;  // what the walk found on seed lane p0 (n_first 0: no path starts there)
  double D = 0.0;
  int kid[KP];
  // (table) the terms of D behind the first: those of knots 2 .. KD + 1 from here (a path of more knots is a bend: it reads
  // the rest of its row where it sums D; the whole row in registers cost the kernel its third wavefront per SIMD)
  constexpr int KD = 6;
  double kd[KD];
  bool untabled = false;       // (table) a path starts here and the table does not hold it for this vehicle's filter
  if (table) {
    // the row of the start lanepoint: one level behind the seeds' loads, and D is summed below in walk_knots' order —
    // its first term is the only one the vehicle's position enters
    kid0 = (seed.road >= 0 && seed.n_lanes <= SMX_WP_LANES && p0 < seed.n_lanes) ? seed_start(m, seed, p0, px, py) : -1;
    if ((unsigned)kid0 >= (unsigned)m.n_lanepoints) kid0 = -1;  // (a dead slot's seeds are words of any age)
    const KnotRow* row = a.knot_table + (kid0 >= 0 ? kid0 : 0);
    const bool serves = knot_row_serves(row->flags, row->f0, row->f1, row->road, seed.f);
    untabled = kid0 >= 0 && !serves;
    n_first = (kid0 >= 0 && serves) ? (int)row->n : 0;
    nk = (kid0 >= 0 && serves) ? (int)row->nk : 0;
    cnt = (kid0 >= 0 && serves) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < KP; ++k) kid[k] = row->idx[k];
#pragma unroll
    for (int k = 0; k < KD; ++k) kd[k] = row->d[k];
    if (kid0 < 0) kid0 = 0;
  } else {
    n_first = a.knots.n[pth];
    nk = a.knots.nk[pth];
    cnt = a.knots.cnt[pth];
    D = a.knots.D[pth];
    kid0 = a.knots.idx[pth];
#pragma unroll
    for (int k = 0; k < KP; ++k) kid[k] = a.knots.idx[(size_t)(k + 1) * paths + pth];
#pragma unroll
    for (int k = 0; k < KD; ++k) kd[k] = 0.0;
  }
  // the trip meter's words (lane 0 of the team uses them)
  const double trip_dist = a.st.f64[(size_t)SMX_S_DIST * total + g], trip_x = a.st.f64[(size_t)SMX_S_TRIP_X * total + g],
               trip_y = a.st.f64[(size_t)SMX_S_TRIP_Y * total + g], trip_h = a.st.f64[(size_t)SMX_S_TRIP_H * total + g];
  const int trip_has = a.st.facts_i32[(size_t)SMX_FI_TRIP_HAS_WP * total + g];
  // (the slow chain writes the rows of a vehicle whose seeds it is still looking for: k_scan_fast; uniform in the team)
  const bool live = in_range && (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (!a.first_only || (flags & SMX_F_FIRST)) && !pend;
  if (!live) {
    seed.road = -1;
    seed.n_lanes = 0;
    seed.f.none();
    n_first = nk = cnt = 0;
    D = 0.0;
    untabled = false;
  }
  // ---- 1. number the paths (as the staged form does)
  const bool seeded = live && seed.road >= 0;
  const WpTeam tm = wp_team_number(seeded, seed.n_lanes, p0, n_first, nk, cnt, P);
  // ---- 2. the path lane's walk over its knots: arclength, unwrapped headings, how many it needs
  SMX_TSTAMP(te1);
  SMX_TACC(32, te0, te1);
  bool tabled_path = false;
  int nrec = 0;
  double kx[KP], ky[KP], kh[KP], cum[KP];
  int kl[KP], kstrict[KP];
  double k0x = 0.0, k0y = 0.0, k0h = 0.0;
  int lane0 = 0;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    kx[k] = ky[k] = kh[k] = cum[k] = 0.0;
    kl[k] = kstrict[k] = 0;
  }
  const bool walk = tm.my_row && tm.listed && !SMX_SKIP(a, 1 << 22);
  if (walk) {
    const smx_lp_rec r0 = load_lp(m, kid0, 46);
    lane0 = r0.lane;
    const int nkp = nk < KP ? nk : KP;
    {
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const bool have = k < nkp;
        const smx_lp_rec* r = m.lp_rec + (have ? kid[k] : 0);
        kx[k] = have ? r->x : 0.0;
        ky[k] = have ? r->y : 0.0;
        kh[k] = have ? r->heading : 0.0;
        kl[k] = have ? r->lane : 0;
      }
    }
    const int n = n_first;
    if (n == 1) {
      // :1379-1390 (a one-point path): the lanepoint itself, not the projection; its heading as it is
      k0x = r0.x;
      k0y = r0.y;
      k0h = r0.heading;
      nrec = 1;
      tabled_path = true;
    } else {
      const double proj = (px - r0.x) * r0.dirx + (py - r0.y) * r0.diry;
      k0x = r0.x + proj * r0.dirx;
      k0y = r0.y + proj * r0.diry;
      k0h = r0.heading;
      if (table) {
        // walk_knots' D: the distance from the projected start to knot 1 (cum[0] below), then the row's terms in order
        const double ex = kx[0] - k0x, ey = ky[0] - k0y;
        D = sqrt(ex * ex + ey * ey);
#pragma unroll
        for (int k = 2; k <= KD + 1; ++k)
          if (k <= nk) D += kd[k - 2];
        const double* const rest = a.knot_table[kid0].d;
#pragma unroll 4
        for (int k = KD + 2; k <= nk; ++k) D += rest[k - 2];
      }
      const int n_emit = n < W ? n : W;
      const double step = D / (double)(n - 1);  // np.linspace(0, D, n)
      const double t_last = (n_emit - 1 == n - 1) ? D : (double)(n_emit - 1) * step;
      double jx = k0x, jy = k0y, jcum = 0.0;
      int jlane = lane0, strict_lane = lane0;
      Unwrap uw;
      uw.start(k0h);
      int need = -1;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k < nkp && need < 0) {
          const double ex = kx[k] - jx, ey = ky[k] - jy;
          const double qcum = jcum + sqrt(ex * ex + ey * ey);
          kh[k] = uw.push(kh[k]);
          cum[k] = qcum;
          if (qcum > jcum) strict_lane = jlane;
          kstrict[k] = strict_lane;
          if (t_last < qcum) need = k + 2;  // the last kept waypoint lies inside this interval
          jx = kx[k];
          jy = ky[k];
          jcum = qcum;
          jlane = kl[k];
        }
      }
      if (need < 0 && nkp == nk) need = nk + 1;  // kept waypoints at or beyond the last knot: every knot, the last one as the tail
      if (need > 0) {
        nrec = need;
        tabled_path = true;
      }
    }
  }
  // ---- records handed out by an exclusive prefix sum over the wavefront's paths
  SMX_TSTAMP(te2);
  SMX_TACC(33, te1, te2);
  int incl = tabled_path ? nrec : 0;
  {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
  }
  const int off = incl - (tabled_path ? nrec : 0);
  // The pool is full (a workgroup whose sixteen vehicles all sit in a bend: one or two of 8 192 per tick): the path's
  // records go to the workgroup's overflow area in device memory instead, and its rows are swept after the others by
  // a plain loop that reads them back (L2).  The rows list's serial emitter — 50 us of one team's latency behind this
  // kernel, at the end of the tick's longest chain, on two ticks of three — is left to the teams that need it.
  const bool spilled = tabled_path && off + nrec > a.wp_pool_limit && a.wp_spill != nullptr;
  if (tabled_path && off + nrec > a.wp_pool_limit && !spilled) tabled_path = false;
  WpKnot* const spill_knots = reinterpret_cast<WpKnot*>(a.wp_spill + (size_t)block * SMX_WPE_SPILL_GROUP_BYTES);
  WpKnotLanes* const spill_lanes = reinterpret_cast<WpKnotLanes*>(spill_knots + (size_t)SMX_BLOCK * (SMX_WPE_KNOTS + 1));
  // A team with a row the pool does not hold (more knots than the table form takes, a cut knot list, a full pool), or
  // that has to number its paths the long way (a branching inside the lookahead, a road of more than four lanes),
  // leaves all its rows and its trip meter to k_waypoints_listed: its vehicle goes to the slow list.
  // (so does a new vehicle, whose trip meter starts with a walk of its own: none comes here on a tick, whose new
  // vehicles are the reset pass's)
  // (developer counts of the reasons, per path lane)
  SMX_COUNT(50, live && p0 == 0 && tm.long_way);
  SMX_COUNT(51, live && p0 == 0 && tm.branching);
  SMX_COUNT(52, tm.my_row && !tm.listed);
  SMX_COUNT(53, tm.my_row && tm.listed && nrec == 0);
  SMX_COUNT(54, tm.my_row && tm.listed && nrec > 0 && !tabled_path);
  SMX_COUNT(55, live && p0 == 0 && (flags & SMX_F_FIRST));
  SMX_COUNT(56, live && p0 == 0);
  // (the knot table: path lanes it could not serve, by reason — the row is not tabled, its filter is another)
  SMX_COUNT(58, untabled && !(a.knot_table[kid0].flags & SMX_KROW_TABLED));
  SMX_COUNT(62, untabled && (a.knot_table[kid0].flags & SMX_KROW_TABLED));
  const bool slow_team =  // uniform in the team
      team_or((live && (tm.serial_team || (tm.my_row && !tabled_path) || untabled || (flags & SMX_F_FIRST))) ? 1 : 0) != 0;
  if (slow_team) tabled_path = false;
  if (a.knot_served != nullptr) {  // (developer count, uniform branch)
    const unsigned long long served = __ballot(table && tabled_path);
    if (threadIdx.x == 0 && served != 0ull) atomicAdd(a.knot_served, (unsigned long long)__popcll(served));
  }
  wp_book_open(book, v, p0, P, gid, total, live && !slow_team, seeded ? tm.n_paths : 0);
  {
    // the wavefront's slow vehicles, appended with one atomic
    const bool app = slow_team && p0 == 0;
    const unsigned long long mask = __ballot(app);
    if (mask != 0ull) {
      const int lane = threadIdx.x & 63;
      int base = 0;
      if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(a.slow_count, __popcll(mask));
      base = __shfl(base, __ffsll((long long)mask) - 1);
      if (app) a.slow_list[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)gid;
    }
  }
  __syncthreads();  // (one wavefront: orders the LDS writes of the team's other lanes)
  if (tm.my_row && !slow_team) {
    book.src[v * P + tm.prov] = (short)col;
    book.count[v * P + tm.prov] = (unsigned char)min(n_first, W);
  }
  if (tabled_path) {
    hdr_step[col] = n_first > 1 ? D / (double)(n_first - 1) : 0.0;
    hdr_D[col] = D;
    hdr_off[col] = (unsigned short)off;
    hdr_nrec[col] = (unsigned char)nrec;
    hdr_n[col] = (unsigned char)n_first;
    hdr_w0[col] = (float)m.lane_width[lane0];
    hdr_s0[col] = (float)m.lane_speed[lane0];
    hdr_li0[col] = (signed char)m.lane_index[lane0];
    {
      bool one = true;
#pragma unroll
      for (int k = 0; k < KP; ++k) one = one && (k + 1 >= nrec || kl[k] == lane0);
      hdr_one_lane[col] = one ? 1 : 0;
    }
    // the path's records out of the registers: the projected start, then the knots it needs
    auto put_records = [&](WpKnot* gk, WpKnotLanes* gl) {
      WpKnot r;
      r.x = k0x;
      r.y = k0y;
      r.h = k0h;
      r.cum = 0.0;
      WpKnotLanes rl;
      rl.lane = (short)lane0;
      rl.strict = (short)lane0;
      gk[0] = r;
      gl[0] = rl;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k + 1 < nrec) {
          WpKnot q;
          q.x = kx[k];
          q.y = ky[k];
          q.h = kh[k];
          q.cum = cum[k];
          gk[k + 1] = q;
          WpKnotLanes ql;
          ql.lane = (short)kl[k];
          ql.strict = (short)kstrict[k];
          gl[k + 1] = ql;
        }
      }
    };
    if (!spilled)
      put_records(pool + off, pool_lanes + off);
    else
      put_records(spill_knots + col * (SMX_WPE_KNOTS + 1), spill_lanes + col * (SMX_WPE_KNOTS + 1));
  }
  hdr_spill[col] = spilled ? 1 : 0;
  __threadfence_block();  // (the overflow area is read back by other lanes of the workgroup)
  __syncthreads();
  SMX_TSTAMP(te3);
  SMX_TACC(34, te2, te3);
  // ---- 3. the waypoint slots of the workgroup's rows, a lane per waypoint.  The rows that hold a path first, in memory
  // order (a road of three lanes leaves every fourth row empty, and the slot arithmetic is straight-line code that a lane
  // without a path went through all the same: a fifth round of four for nothing); then the empty rows, zeros only.
  // Four slots per lane
  // and round, their arithmetic written without branches (every read at a clamped index, results selected at the end):
  // the four dependency chains — header, interval search, two knot records, three divisions, the heading wrap — are
  // independent, and straight-line code is what lets the compiler interleave them (a wavefront alone on its SIMD half
  // the time issues one chain's instruction every ten cycles or so).  Only the rare lane look-ups keep their branch.
  int n_rows_live = 0, n_rows_zero = 0, n_rows_spill = 0;  // (uniform: the workgroup is one wavefront)
  {
    static_assert(SMX_BLOCK == 64, "one ballot per 64 rows");
    const int n_rows = SMX_WPT_VEHICLES * P;
    const unsigned long long below = (1ull << threadIdx.x) - 1ull;
    for (int r0 = 0; r0 < n_rows; r0 += SMX_BLOCK) {
      const int r = r0 + (int)threadIdx.x;
      const int src = r < n_rows ? (int)book.src[r] : (int)SMX_ROW_SKIP;
      const bool in_pool = src >= 0 && hdr_spill[src] == 0, in_spill = src >= 0 && hdr_spill[src] != 0;
      const unsigned long long ml = __ballot(in_pool), mz = __ballot(src == SMX_ROW_ZERO), ms = __ballot(in_spill);
      if (in_pool) rows_live[n_rows_live + __popcll(ml & below)] = (unsigned char)r;
      if (src == SMX_ROW_ZERO) rows_zero[n_rows_zero + __popcll(mz & below)] = (unsigned char)r;
      if (in_spill) rows_spill[n_rows_spill + __popcll(ms & below)] = (unsigned char)r;
      n_rows_live += __popcll(ml);
      n_rows_zero += __popcll(mz);
      n_rows_spill += __popcll(ms);
    }
  }
  __syncthreads();
  {
    const float rcp_p = 1.0f / (float)P;  // (row -> vehicle: small_quotient, rows below 128)
    const int drow = SMX_BLOCK / W, di = SMX_BLOCK - drow * W;
    {  // the empty rows of the workgroup's tabled vehicles: zeros, lane ids -1
      WpCursor cur(W, P);
      for (int e = threadIdx.x; e < n_rows_zero * W; e += SMX_BLOCK, cur.advance()) {
        const int row = rows_zero[cur.row];
        const int vq = small_quotient(row, rcp_p);
        const size_t q = ((size_t)book.veh[vq] * P + (row - vq * P)) * W + cur.i;
        double* dst = o.wp_pos + q * 3;
        dst[0] = 0.0;
        dst[1] = 0.0;
        dst[2] = 0.0;
        o.wp_heading[q] = 0.0f;
        o.wp_lane_width[q] = 0.0f;
        o.wp_speed_limit[q] = 0.0f;
        o.wp_lane_id[q] = (int16_t)-1;
        o.wp_lane_index[q] = (int8_t)0;
      }
    }
    const int elems = n_rows_live * W;
    int ridx = threadIdx.x / W, i = threadIdx.x - ridx * W;  // element e = ridx * W + i, advanced by 64 per slot
    constexpr int U = 4;
    for (int e0 = threadIdx.x; e0 < (SMX_SKIP(a, 1 << 21) ? 0 : elems); e0 += U * SMX_BLOCK) {
      int s_row[U], s_i[U], s_vv[U], s_slot[U];
      bool s_in[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s_in[u] = e0 + u * SMX_BLOCK < elems;
        s_row[u] = rows_live[min(ridx, n_rows_live - 1)];
        s_i[u] = i;
        s_vv[u] = small_quotient(s_row[u], rcp_p);
        s_slot[u] = s_row[u] - s_vv[u] * P;
        ridx += drow;
        i += di;
        if (i >= W) {
          i -= W;
          ++ridx;
        }
      }
      SMX_TSTAMP(tr0);
      double ox[U], oy[U], oh[U];
      float ow[U], os[U];
      int oln[U], oli[U], osrc[U], okl[U], oql[U];
      bool owrite[U], ohave[U], oone[U], ointerior[U];
      double oden[U], odt[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int src = s_in[u] ? (int)book.src[s_row[u]] : (int)SMX_ROW_SKIP;
        const bool have = src >= 0 && s_i[u] < (int)book.count[s_row[u]];
        const int sc = have ? src : 0;
        const int n = hdr_n[sc], nr = max((int)hdr_nrec[sc], 1), koff = hdr_off[sc];
        const double t = (s_i[u] == n - 1) ? hdr_D[sc] : (double)s_i[u] * hdr_step[sc];
        // np.interp's interval: the last knot with cum <= t.  Cums do not decrease along the path, so that is the
        // number of knots 1 .. nr-1 with cum <= t (the reads are issued together)
        int j = 0;
#pragma unroll
        for (int k = 1; k <= SMX_WPE_KNOTS; ++k) {
          const double ck = pool[min(koff + k, SMX_WPE_POOL - 1)].cum;
          j += (k < nr && ck <= t) ? 1 : 0;
        }
        const bool interior = j + 1 < nr;
        const int kj = min(koff + j, SMX_WPE_POOL - 1), qj = min(koff + (interior ? j + 1 : j), SMX_WPE_POOL - 1);
        const WpKnot K = pool[kj];
        const WpKnot Q = pool[qj];
        const WpKnotLanes KL = pool_lanes[kj], QL = pool_lanes[qj];
        const double den = interior ? Q.cum - K.cum : 1.0;
        const double dt_ = t - K.cum;
        const double sx = (Q.x - K.x) / den, sy = (Q.y - K.y) / den, sh = (Q.h - K.h) / den;
        // (at or beyond the last knot: the knot itself; t == cum: the lane of the last knot strictly passed)
        double h = interior ? sh * dt_ + K.h : K.h;
        h = (n == 1) ? h : wrap_heading(h);
        ox[u] = have ? (interior ? sx * dt_ + K.x : K.x) : 0.0;
        oy[u] = have ? (interior ? sy * dt_ + K.y : K.y) : 0.0;
        oh[u] = have ? h : 0.0;
        ow[u] = have ? hdr_w0[sc] : 0.0f;
        os[u] = have ? hdr_s0[sc] : 0.0f;
        oln[u] = have ? ((t == K.cum) ? (int)KL.strict : (int)KL.lane) : -1;
        oli[u] = have ? (int)hdr_li0[sc] : 0;
        osrc[u] = src;
        owrite[u] = src != SMX_ROW_SKIP;
        ohave[u] = have;
        oone[u] = hdr_one_lane[sc] != 0;
        ointerior[u] = interior;
        okl[u] = KL.lane;
        oql[u] = QL.lane;
        oden[u] = den;
        odt[u] = dt_;
      }
      SMX_TSTAMP(tr1);
      // a path whose knots do not all lie on its start lane (seldom): lane width / speed limit / index from the tables,
      // interpolated where the interval joins two lanes
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ohave[u] && !oone[u]) {
          double wj = m.lane_width[okl[u]], sj = m.lane_speed[okl[u]];
          if (ointerior[u] && oql[u] != okl[u]) {
            const double sw = (m.lane_width[oql[u]] - wj) / oden[u], ss = (m.lane_speed[oql[u]] - sj) / oden[u];
            wj = sw * odt[u] + wj;
            sj = ss * odt[u] + sj;
          }
          ow[u] = (float)wj;
          os[u] = (float)sj;
          oli[u] = m.lane_index[oln[u]];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ohave[u] && s_i[u] == 0 && s_slot[u] == 0) {  // first waypoint of the vehicle's first path: the trip meter's
          first_wp[s_vv[u]][0] = ox[u];
          first_wp[s_vv[u]][1] = oy[u];
          first_wp[s_vv[u]][2] = oh[u];
        }
        if (owrite[u] && (!SMX_SKIP(a, 1 << 20) || ox[u] == 1.2345e300)) {  // (developer ablation: compute, do not store)
          const size_t q = ((size_t)book.veh[s_vv[u]] * P + s_slot[u]) * W + s_i[u];
          double* dst = o.wp_pos + q * 3;
          dst[0] = ox[u];
          dst[1] = oy[u];
          dst[2] = 0.0;
          o.wp_heading[q] = (float)oh[u];
          o.wp_lane_width[q] = ow[u];
          o.wp_speed_limit[q] = os[u];
          o.wp_lane_id[q] = (int16_t)oln[u];
          o.wp_lane_index[q] = (int8_t)oli[u];
        }
      }
      SMX_TSTAMP(tr2);
      SMX_TACC(38, tr0, tr1);
      SMX_TACC(39, tr1, tr2);
    }
    // the rows whose knots lie in the overflow area (seldom any): the same expressions, one slot at a time, the knot
    // records read back from device memory
    if (n_rows_spill > 0) {
      WpCursor cur(W, P);
      for (int e = threadIdx.x; e < n_rows_spill * W; e += SMX_BLOCK, cur.advance()) {
        const int row = rows_spill[cur.row], i = cur.i;
        const int vq = small_quotient(row, rcp_p), slot_q = row - vq * P;
        const int sc = (int)book.src[row];
        const bool have = i < (int)book.count[row];
        const WpKnot* gk = spill_knots + sc * (SMX_WPE_KNOTS + 1);
        const WpKnotLanes* gl = spill_lanes + sc * (SMX_WPE_KNOTS + 1);
        const int n = hdr_n[sc], nr = max((int)hdr_nrec[sc], 1);
        const double t = (i == n - 1) ? hdr_D[sc] : (double)i * hdr_step[sc];
        int j = 0;
        for (int k = 1; k < nr; ++k) j += (gk[k].cum <= t) ? 1 : 0;
        const bool interior = j + 1 < nr;
        const WpKnot K = gk[j];
        const WpKnot Q = gk[interior ? j + 1 : j];
        const WpKnotLanes KL = gl[j], QL = gl[interior ? j + 1 : j];
        const double den = interior ? Q.cum - K.cum : 1.0;
        const double dt_ = t - K.cum;
        const double sx = (Q.x - K.x) / den, sy = (Q.y - K.y) / den, sh = (Q.h - K.h) / den;
        double h = interior ? sh * dt_ + K.h : K.h;
        h = (n == 1) ? h : wrap_heading(h);
        const double ox = have ? (interior ? sx * dt_ + K.x : K.x) : 0.0;
        const double oy = have ? (interior ? sy * dt_ + K.y : K.y) : 0.0;
        const double oh = have ? h : 0.0;
        float ow = have ? hdr_w0[sc] : 0.0f, os = have ? hdr_s0[sc] : 0.0f;
        const int oln = have ? ((t == K.cum) ? (int)KL.strict : (int)KL.lane) : -1;
        int oli = have ? (int)hdr_li0[sc] : 0;
        if (have && hdr_one_lane[sc] == 0) {
          double wj = m.lane_width[KL.lane], sj = m.lane_speed[KL.lane];
          if (interior && QL.lane != KL.lane) {
            const double sw = (m.lane_width[QL.lane] - wj) / den, ss = (m.lane_speed[QL.lane] - sj) / den;
            wj = sw * dt_ + wj;
            sj = ss * dt_ + sj;
          }
          ow = (float)wj;
          os = (float)sj;
          oli = m.lane_index[oln];
        }
        if (have && i == 0 && slot_q == 0) {
          first_wp[vq][0] = ox;
          first_wp[vq][1] = oy;
          first_wp[vq][2] = oh;
        }
        const size_t q = ((size_t)book.veh[vq] * P + slot_q) * W + i;
        double* dst = o.wp_pos + q * 3;
        dst[0] = ox;
        dst[1] = oy;
        dst[2] = 0.0;
        o.wp_heading[q] = (float)oh;
        o.wp_lane_width[q] = ow;
        o.wp_speed_limit[q] = os;
        o.wp_lane_id[q] = (int16_t)oln;
        o.wp_lane_index[q] = (int8_t)oli;
      }
    }
    SMX_TSTAMP(te4);
    SMX_TACC(35, te3, te4);
    wp_book_store_counts(book, o.wp_count, P);
  }
  __syncthreads();  // first_wp is complete
  SMX_TSTAMP(te5);
  // ---- trip meter + reward (lane 0 of the team): path 0 is the lowest started lane's, row 0 of the vehicle
  if (live && !slow_team && p0 == 0) {
    // the advance and the store, on the words loaded at the top (no new vehicle comes here: nothing to start)
    TripMeter t = trip_meter_of(trip_dist, trip_x, trip_y, trip_h, trip_has != 0);
    if (tm.n_paths > 0 && trip_counts_waypoint(a, m, gid, total)) {
      const WpFirst fw = {true, first_wp[v][0], first_wp[v][1], first_wp[v][2]};
      trip_meter_advance(a, gid, total, t, fw);
    }
    trip_meter_store(a, gid, total, t);
  }
  SMX_TSTAMP(te6);
  SMX_TACC(36, te5, te6);
  SMX_TACC(37, te0, te6);
}

// =================================================================================
// observe role: the rest of Sensors.observe (sensors.py:238-396) and the events / done logic
// (sensors.py:443-594), one thread per vehicle, whole envs per workgroup (env-mates' poses in LDS)
// =================================================================================
// The rows of several elements per agent (ego block, events, neighbour rows) go through LDS: every lane fills
// its own vehicle's cells, then the workgroup sweeps each output array in memory order — the rows of its
// vehicles are adjacent — so a store instruction writes consecutive elements instead of one element of 64 rows.
// (Scalars per agent — done, active, reward, counts — are consecutive across lanes as they are.)
#define SMX_NB_STAGE 16  // neighbour rows per agent the staged form handles (nb_max; StdObs keeps 10)
static_assert(SMX_BLOCK * SMX_NB_STAGE * 3 < 4096, "small_quotient's range");
struct ObsStage {
  float ego_f32[SMX_BLOCK][SMX_EGO_F32_COUNT];
  short ego_lane[SMX_BLOCK][2];
  unsigned char events[SMX_BLOCK][SMX_EV_COUNT + 1];
  signed char nb_list[SMX_BLOCK][SMX_NB_STAGE];  // env-mate slot of every neighbour row kept
  unsigned char nb_kept[SMX_BLOCK];
  unsigned char mode[SMX_BLOCK];                 // 1: this vehicle's rows are written this pass
};

// TraverseGoal._drove_off_map (plan.py:147-166): the vehicle has left the map beyond the end of a dead-end lane,
// going roughly the lane's way.  `lane`, `dist`: the scan's nearest lane — the same query as nearest_lanes(pos)[0]
// (radius max(10, 2 x default lane width), junction lanes included, dist < radius, ties to the lower lane id).
__device__ inline bool drove_off_map(const MissionsDev& ms, const MapDev& m, int n_slots, int lane, double dist, double px,
                                     double py, double heading) {
  if (lane < 0) return false;  // "we can't tell anything here"
  const double offset = lane_offset_along(m, lane, px, py);
  const double width = m.lane_width[lane];  // width_at_offset (sumo_road_network.py:493-494)
  if (!ms.lane_dead_end(n_slots, m.n_lanes)[lane] || dist < 0.5 * width + 1e-1) return false;
  if (offset < m.lane_length[lane] - 2 * width) return false;
  const double heading_err = min_angles_difference_signed(ms.lane_end_heading(n_slots)[lane], heading);
  return fabs(heading_err) < SMX_PI / 6;
}

// LapMission.is_complete (plan.py:272-277), second half: reached_goal also needs distance_travelled >
// route_length * num_laps, where distance_travelled is the trip meter's total with this tick's waypoint counted
// (sensors.py:349-351, 491-496).  The observe role runs beside the waypoints role that writes that total, so it
// decides a lap slot as a positional one and the commit role — after both, in every launch form and in the reset
// pass — takes the event back while the distance is short: reached_goal off, done from the other events of the
// row (sensors.py:465-476), and the flags / active / done / learner words the observe role derived from done.
// (`tick`: the tick's commit, whose observe role saw every agent and wrote reward / done; k_tail's argument block is
// the reset pass's, so first_only / keep_reward_done are read only for the reset pass's own commit)
__device__ inline void lap_goal_gate(const KernelArgs& a, size_t gid, size_t total, int slot, bool tick) {
  const smx_mission_goal g = a.missions.goal_kind[slot];
  if (g.kind != SMX_GOAL_LAP) return;
  const smx_config& c = a.cfg;
  const smx_outputs& o = a.out;
  const int flags = a.st.flags[gid];
  const bool observed = (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (tick || !a.first_only || (flags & SMX_F_FIRST));
  uint8_t* ev = o.events + gid * SMX_EV_COUNT;
  if (!observed || !ev[SMX_EV_REACHED_GOAL]) return;
  if (o.dist[gid] > g.route_length * g.num_laps) return;
  ev[SMX_EV_REACHED_GOAL] = 0;
  const uint32_t dc = c.done_criteria;
  bool done = (ev[SMX_EV_OFF_ROAD] && (dc & SMX_DONE_OFF_ROAD)) || ev[SMX_EV_REACHED_MAX_EPISODE_STEPS] ||
              (ev[SMX_EV_ON_SHOULDER] && (dc & SMX_DONE_ON_SHOULDER)) || (ev[SMX_EV_COLLISIONS] && (dc & SMX_DONE_COLLISION)) ||
              (ev[SMX_EV_NOT_MOVING] && (dc & SMX_DONE_NOT_MOVING)) || (ev[SMX_EV_OFF_ROUTE] && (dc & SMX_DONE_OFF_ROUTE)) ||
              (ev[SMX_EV_WRONG_WAY] && (dc & SMX_DONE_WRONG_WAY)) || ev[SMX_EV_AGENTS_ALIVE_DONE];
  if (flags & SMX_F_FIRST) done = false;
  if (done) return;  // ended by another event: every derived word stands
  a.st.facts_i32[(size_t)SMX_FI_FLAGS_NEXT * total + gid] |= SMX_F_ALIVE;
  o.active[gid] = 1;
  if (tick || !a.keep_reward_done) {
    o.done[gid] = 0;
    if (o.learner) o.learner[total + gid] = 0.0f;
  }
}

// (own_box: a triple block is bound, TickPlan::sized — the caller's literal; the copy without it keeps the observer's box
// a constant.  A function argument and not a template argument: as a template the role's kernels without dimensions
// took 27 registers more and spilled, profiles/r24_agent_dims_resources.txt)
__device__ __forceinline__ void observe_role(const KernelArgs& a, const int block, const bool own_box) {
  const bool OWN_BOX = own_box;
  __shared__ SharedPose pose[SMX_BLOCK];
  __shared__ ObsStage stage;
  __shared__ unsigned long long zero_mask;  // vehicles of the workgroup whose rows are to read as an absent agent's
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const smx_outputs& o = a.out;
  const int n_veh = c.num_vehicles;
  const int epb = SMX_BLOCK / n_veh;
  const int local = threadIdx.x;
  if (local == 0) zero_mask = 0ull;
  const int env_local = local / n_veh;
  const int slot = local - env_local * n_veh;
  const int env = block * epb + env_local;
  const bool valid = (env_local < epb) && (env < c.num_envs);
  const size_t total = (size_t)c.num_envs * n_veh;
  const size_t gid = valid ? ((size_t)env * n_veh + slot) : 0;
  const SharedPose* env_pose = pose + env_local * n_veh;

  if (SMX_SKIP(a, 8192)) return;
  SMX_TSTAMP(to0);
  VehState s = {0, 0, 0, 0, 0, 0, 0};
  int flags = 0;
  bool alive = false;
  int my_lane = -1, my_facts = 0;
  double my_lane_dist = SMX_INF;
  if (valid) {
    flags = a.st.flags[gid];
    alive = (flags & SMX_F_ALIVE) != 0;
    s = load_vehicle(a, gid, total);
    if (alive) {
      my_lane = a.st.facts_i32[(size_t)SMX_FI_LANE * total + gid];
      my_facts = a.st.facts_i32[(size_t)SMX_FI_FLAGS * total + gid];
      my_lane_dist = a.st.facts_f64[(size_t)SMX_FF_LANE_DIST * total + gid];
    }
  }
  const HeadingTrig trig = heading_trig(s.heading);
  // an agent of the kinematic spaces (uniform over the launch) reports the provider's speed (BoxChassis.speed)
  const bool kinematic = smx_kinematic_space(c.action_space) && !(flags & SMX_F_SOCIAL);
  const double speed = kinematic ? s.u : vehicle_speed(s, trig);
  if (local < SMX_BLOCK) {  // k_first runs this role in a wider workgroup: the extra threads hold nothing
    SharedPose& p = pose[local];
    p.x = s.x;
    p.y = s.y;
    p.heading = wrap_heading(s.heading);
    p.speed = speed;
    p.lane = my_lane;
    p.lane_dist = my_lane_dist;
    p.alive = (valid && alive) ? 1 : 0;
    // what an observer reports as this vehicle's lane: nearest_lane(nv.pose.point, radius=vehicle.length)
    // (sensors.py:244-246: the OBSERVER's length — the sedan's here; with dimensions bound the readers of nl / nlidx
    // take the lane and its distance and ask with their own length instead)
    const int nl = (my_lane >= 0 && my_lane_dist < SMX_CHASSIS_LENGTH) ? my_lane : -1;
    p.nl = (short)nl;
    p.nlidx = (short)(nl >= 0 ? m.lane_index[nl] : -1);
    stage.mode[local] = 0;
  }
  __syncthreads();
  SMX_TSTAMP(to1);
  SMX_TACC(7, to0, to1);

  const bool first = (flags & SMX_F_FIRST) != 0;
  const bool social = (flags & SMX_F_SOCIAL) != 0;
  const bool mine = valid && alive && !social && (!a.first_only || first);
  bool done = false;
  int new_flags = flags;  // what the commit kernel makes the vehicle's flags word after this pass
  if (valid && first && (social || !alive)) {
    // nothing to observe: its rows read as an absent agent's (a scripted vehicle is alive here; a replayed slot that is
    // empty in the reset observation's frame carries SMX_F_FIRST without SMX_F_ALIVE for the same treatment, and so
    // does a history agent that did not enter, the one agent that is created not alive)
    atomicOr(&zero_mask, 1ull << local);
    o.active[gid] = 0;
    o.done[gid] = 0;
    new_flags = flags & ~SMX_F_FIRST;
  }
  const bool nb_staged = c.nb_max <= SMX_NB_STAGE;
  if (mine) {
    stage.mode[local] = 1;
    const double px = s.x, py = s.y;
    int steps = a.st.steps[gid];
    // (a reset pass runs after its commit: a new vehicle's tick is env_ticks; in a tick's own pass — a new vehicle there is
    // an entrant of smx_set_agent_entry — the commit comes later)
    const int env_ticks = (first && a.first_only) ? a.st.env_ticks[env] : a.st.env_ticks[env] + 1;  // smarts.py:261-262
    if (!first) ++steps;  // SensorState.step (agent_manager.py:250-258); a new vehicle starts at 1

    // ---- collisions (smarts.py:1270-1291): a new vehicle has not been through a physics step
    bool collided = false;
    unsigned long long collidee_mask = 0ull;
    // One pass over the env-mates serves the collisions' broad phase (circumscribed circles; the narrow phase then
    // runs over the survivors only: a wavefront pays for max-over-lanes(candidates) box tests, not for n_veh) and
    // the neighbourhood (sensors.py:241-266, smarts.py:1191-1208: every other vehicle of the instance within
    // `radius`, in slot order, first nb_max kept) — both look at the same squared distance.
    // (an entrant of smx_set_agent_entry, SMX_F_ENTERING, is tested: its mates see it in their collisions this tick, and
    // so does it — include/smx.h)
    const bool want_col = (!first || (flags & SMX_F_ENTERING)) && !SMX_SKIP(a, 4);
    const bool want_nb = (c.sensors & SMX_SENSOR_NEIGHBORS) && !SMX_SKIP(a, 8);
    const bool nb_in_pass = want_nb && nb_staged;  // (more rows than the staged form holds: the loop further down)
    int nb_cnt = 0;
    {
      unsigned long long cand = 0ull;
      const double reach = sqrt(SMX_CHASSIS_LENGTH * SMX_CHASSIS_LENGTH + SMX_CHASSIS_WIDTH * SMX_CHASSIS_WIDTH) +
                           SMX_COLLISION_LEEWAY;
      const double reach2 = reach * reach;
      const bool nb_all = !(c.nb_radius >= 0.0);
      for (int j = 0; j < n_veh; ++j) {
        if (j == slot) continue;
        const SharedPose& q = env_pose[j];
        if (!q.alive) continue;
        const double dx = px - q.x, dy = py - q.y;
        const double d2 = dx * dx + dy * dy;
        if (want_col && !(d2 > reach2)) cand |= 1ull << j;
        // sqrt(dx^2 + dy^2 + 0^2) <= radius, as a threshold on the squared distance (radius_threshold)
        if (nb_in_pass && (nb_all || d2 <= a.nb_d2_max)) {
          if (nb_cnt < c.nb_max) stage.nb_list[local][nb_cnt] = (signed char)j;
          ++nb_cnt;
        }
      }
      const double my_h = wrap_heading(s.heading);
      const bool sized = dims_sized(a);
      double my_len = SMX_CHASSIS_LENGTH, my_wid = SMX_CHASSIS_WIDTH;
      if (sized && want_col) {
        // Dimensions bound (smx_set_social_history_dims, smx_set_agent_dims): the candidates again, in a pass of its own
        // so that the loop above stays what it is without them.  The reach is the observer's half diagonal plus the
        // mate's plus the leeway — boxes_within's own broad phase; between two sedans the one full diagonal.
        double my_half_diag = 0.5 * sqrt(SMX_CHASSIS_LENGTH * SMX_CHASSIS_LENGTH + SMX_CHASSIS_WIDTH * SMX_CHASSIS_WIDTH);
        if (OWN_BOX) {
          const VehBox my = vehicle_box(a, gid, true);
          my_len = my.length, my_wid = my.width;
          my_half_diag = 0.5 * sqrt(my_len * my_len + my_wid * my_wid);
        }
        cand = 0ull;
        for (int j = 0; j < n_veh; ++j) {
          if (j == slot) continue;
          const SharedPose& q = env_pose[j];
          if (!q.alive) continue;
          const VehBox mb = vehicle_box(a, gid - slot + j, true);
          const double dx = px - q.x, dy = py - q.y;
          const double r = my_half_diag + 0.5 * sqrt(mb.length * mb.length + mb.width * mb.width) + SMX_COLLISION_LEEWAY;
          if (!(dx * dx + dy * dy > r * r)) cand |= 1ull << j;
        }
      }
      // one Collision per collidee (smarts.py:1270-1291): every survivor is tested, not just the first hit
      // (one call site for both: a second inlined copy of the box test made the kernel spill)
      while (cand != 0ull) {
        const int j = __ffsll((long long)cand) - 1;
        cand &= cand - 1ull;
        const SharedPose& q = env_pose[j];
        const VehBox mb = vehicle_box(a, gid - slot + j, sized);
        if (boxes_within(px, py, my_h, q.x, q.y, q.heading, OWN_BOX ? my_len : SMX_CHASSIS_LENGTH, OWN_BOX ? my_wid : SMX_CHASSIS_WIDTH, mb.length,
                         mb.width, SMX_COLLISION_LEEWAY))
          collidee_mask |= 1ull << j;
      }
      collided = collidee_mask != 0ull;
    }
    if (o.collidees) o.collidees[gid] = collidee_mask;

    double lng, lat;
    long_lat_speed(s, trig, lng, lat);
    double kin_av[2] = {0.0, 0.0}, kin_yaw_rate = 0.0;
    if (kinematic) {
      // BoxChassis.velocity_vectors / .yaw_rate (chassis.py:275-308): the linear velocity is the heading vector x speed;
      // the "angular velocity" is the difference of the heading vectors over dt, as the reference has it; no yaw rate
      // (None -> NaN) until control() has been called with a dt
      double vhx, vhy;
      radians_to_vec(s.heading, vhx, vhy);
      lng = vhx * speed;
      lat = vhy * speed;
      const double last_dt = SF(SMX_S_KIN_LAST_DT), last_heading = SF(SMX_S_KIN_LAST_HEADING);
      if (last_dt > 0.0) {
        double lhx, lhy;
        radians_to_vec(last_heading, lhx, lhy);
        kin_av[0] = (vhx - lhx) / last_dt;
        kin_av[1] = (vhy - lhy) / last_dt;
        kin_yaw_rate = min_angles_difference_signed(s.heading, last_heading) / last_dt;
      } else {
        kin_yaw_rate = __builtin_nan("");
      }
    }
    // ---- ego lane (sensors.py:277-285): nearest lane within max(10, 2 * default lane width)
    const int ego_lane = (my_lane >= 0 && my_lane_dist < fmax(10.0, 2.0 * m.default_lane_width)) ? my_lane : -1;
    // ---- ego vehicle state (sensors.py:314-329; read-back of chassis.py:493-566)
    float* ef = stage.ego_f32[local];  // (ego_pos comes from the pose block)
    ef[SMX_EGO_HEADING] = (float)wrap_heading(s.heading);
    ef[SMX_EGO_SPEED] = (float)speed;
    // (BoxChassis.steering is None: np.float32(None) = NaN, format_obs.py:432)
    ef[SMX_EGO_STEERING] = kinematic ? __builtin_nanf("") : (float)(-s.delta);
    ef[SMX_EGO_YAW_RATE] = kinematic ? (float)kin_yaw_rate : (float)vec_to_radians(0.0, 0.0);  // chassis.py:552-556 on a planar body
    ef[SMX_EGO_LIN_VEL + 0] = (float)lng;
    ef[SMX_EGO_LIN_VEL + 1] = (float)lat;
    ef[SMX_EGO_LIN_VEL + 2] = 0.0f;
    ef[SMX_EGO_ANG_VEL + 0] = (float)kin_av[0];
    ef[SMX_EGO_ANG_VEL + 1] = (float)kin_av[1];
    ef[SMX_EGO_ANG_VEL + 2] = (float)s.r;
    ef[SMX_EGO_BOX + 0] = (float)SMX_CHASSIS_LENGTH;
    ef[SMX_EGO_BOX + 1] = (float)SMX_CHASSIS_WIDTH;
    ef[SMX_EGO_BOX + 2] = (float)SMX_CHASSIS_HEIGHT;
    if (OWN_BOX) {  // (sensors.py:317: the agent's own box)
      const VehBox my = vehicle_box(a, gid, true);
      ef[SMX_EGO_BOX + 0] = (float)my.length;
      ef[SMX_EGO_BOX + 1] = (float)my.width;
      ef[SMX_EGO_BOX + 2] = (float)my.height;
    }
    stage.ego_lane[local][0] = (short)ego_lane;
    stage.ego_lane[local][1] = (short)(ego_lane >= 0 ? m.lane_index[ego_lane] : -1);

    // ---- accelerometer (sensors.py:1053-1084): finite differences over a 3-deep history
    {
      double la[3] = {0, 0, 0}, aa[3] = {0, 0, 0}, lj[3] = {0, 0, 0}, aj[3] = {0, 0, 0};
      if (c.sensors & SMX_SENSOR_ACCELEROMETER) {
        int hist = first ? 0 : ((flags >> SMX_F_HIST_SHIFT) & 3);  // samples held before this one
        double l0x = SF(SMX_S_LV0_LONG), l0y = SF(SMX_S_LV0_LAT), a0z = SF(SMX_S_AV0_Z);
        double l1x = SF(SMX_S_LV1_LONG), l1y = SF(SMX_S_LV1_LAT), a1z = SF(SMX_S_AV1_Z);
        if (hist >= 1) {
          la[0] = (lng - l0x) / c.dt;
          la[1] = (lat - l0y) / c.dt;
          aa[2] = (s.r - a0z) / c.dt;
          if (hist >= 2) {
            lj[0] = la[0] - (l0x - l1x) / c.dt;
            lj[1] = la[1] - (l0y - l1y) / c.dt;
            aj[2] = aa[2] - (a0z - a1z) / c.dt;
          }
        }
        SF(SMX_S_LV1_LONG) = l0x;
        SF(SMX_S_LV1_LAT) = l0y;
        SF(SMX_S_AV1_Z) = a0z;
        SF(SMX_S_LV0_LONG) = lng;
        SF(SMX_S_LV0_LAT) = lat;
        SF(SMX_S_AV0_Z) = s.r;
        hist = hist < 2 ? hist + 1 : 2;
        flags = (flags & ~(3 << SMX_F_HIST_SHIFT)) | (hist << SMX_F_HIST_SHIFT);
      }
      for (int q = 0; q < 3; ++q) {
        ef[SMX_EGO_LIN_ACC + q] = (float)la[q];
        ef[SMX_EGO_ANG_ACC + q] = (float)aa[q];
        ef[SMX_EGO_LIN_JERK + q] = (float)lj[q];
        ef[SMX_EGO_ANG_JERK + q] = (float)aj[q];
      }
    }

    // ---- neighbourhood: the staged form's rows were listed above; more rows than it holds leave from here
    if (want_nb) {
      int cnt = nb_cnt;
      for (int j = 0; j < n_veh && !nb_staged; ++j) {
        if (j == slot) continue;
        const SharedPose& q = env_pose[j];
        if (!q.alive) continue;
        if (c.nb_radius >= 0.0) {
          double dx = q.x - px, dy = q.y - py, dz = SMX_BASE_HEIGHT - SMX_BASE_HEIGHT;
          double d = sqrt(dx * dx + dy * dy + dz * dz);
          if (!(d <= c.nb_radius)) continue;
        }
        if (cnt < c.nb_max) {
          size_t w = gid * c.nb_max + cnt;
          o.nb_pos[w * 3 + 0] = q.x;
          o.nb_pos[w * 3 + 1] = q.y;
          o.nb_pos[w * 3 + 2] = SMX_BASE_HEIGHT;
          const VehBox mb = vehicle_box(a, gid - slot + j);
          o.nb_box[w * 3 + 0] = (float)mb.length;
          o.nb_box[w * 3 + 1] = (float)mb.width;
          o.nb_box[w * 3 + 2] = (float)mb.height;
          o.nb_heading[w] = (float)q.heading;
          o.nb_speed[w] = (float)q.speed;
          // nearest_lane(nv.pose.point, radius=vehicle.length) (sensors.py:244-246: the EGO's length)
          int nl = (q.lane >= 0 && q.lane_dist < vehicle_box(a, gid, OWN_BOX).length) ? q.lane : -1;
          o.nb_lane_id[w] = (int16_t)nl;
          o.nb_lane_index[w] = (int8_t)(nl >= 0 ? m.lane_index[nl] : -1);
          o.nb_slot[w] = (int8_t)j;
        }
        ++cnt;
      }
      stage.nb_kept[local] = (unsigned char)(cnt < c.nb_max ? cnt : c.nb_max);
      for (int q0 = cnt; q0 < c.nb_max && !nb_staged; ++q0) {
        size_t w = gid * c.nb_max + q0;
        o.nb_pos[w * 3] = o.nb_pos[w * 3 + 1] = o.nb_pos[w * 3 + 2] = 0.0;
        o.nb_box[w * 3] = o.nb_box[w * 3 + 1] = o.nb_box[w * 3 + 2] = 0.0f;
        o.nb_heading[w] = 0.0f;
        o.nb_speed[w] = 0.0f;
        o.nb_lane_index[w] = 0;
        o.nb_lane_id[w] = -1;
        o.nb_slot[w] = -1;
      }
      o.nb_count[gid] = (uint8_t)(cnt > 255 ? 255 : cnt);
    }

    SMX_TSTAMP(to2);
    SMX_TACC(8, to1, to2);
    // ---- driven path (sensors.py:842-877): running length of the last window
    bool is_not_moving = false;
    if (a.st.driven_path != nullptr) {
      double* ring = a.st.driven_path + gid * (size_t)SMX_DRIVEN_PATH_LEN;
      double sum = SF(SMX_S_PATH_SUM);
      int window_pts = (int)floor(c.not_moving_time / c.dt + 1e-9) + 1;
      if (window_pts > SMX_DRIVEN_PATH_LEN) window_pts = SMX_DRIVEN_PATH_LEN;
      const int K = window_pts - 1;  // segments in a full window
      if (first) {
        sum = 0.0;  // a reset records a point but no segment
      } else {
        double dx = SF(SMX_S_PREV_X) - px, dy = SF(SMX_S_PREV_Y) - py;
        double seg = sqrt(dx * dx + dy * dy);
        int nseg = steps - 1;  // segments recorded so far, this one included
        ring[(nseg - 1) % SMX_DRIVEN_PATH_LEN] = seg;
        sum += seg;
        if (nseg > K) sum -= ring[(nseg - 1 - K) % SMX_DRIVEN_PATH_LEN];
      }
      SF(SMX_S_PATH_SUM) = sum;
      double elapsed = (double)env_ticks * c.dt;
      if (!(elapsed < c.not_moving_time)) is_not_moving = sum < c.not_moving_distance;
    }

    // ---- via sensor (ViaSensor.__call__, sensors.py:1103-1146; acquisition range 40 m and speed
    //      tolerance 1.5 m/s from vehicle.py:553-557)
    if (c.via_max > 0 && a.vias != nullptr) {
      const int v_a = a.via_slot_off[slot], v_b = a.via_slot_off[slot + 1];
      int32_t* consumed_p = a.st.facts_i32 + (size_t)SMX_FI_VIA_CONSUMED * total + gid;
      unsigned consumed = first ? 0u : (unsigned)*consumed_p;
      int hit = 0, cnt = 0;
      int8_t* near = o.via_near + gid * (size_t)c.via_max;
      for (int v = v_a; v < v_b; ++v) {
        const smx_via via = a.vias[v];
        double qx, qy;
        lane_center_at_point(m, via.lane, px, py, qx, qy);
        const double lx = qx - px, ly = qy - py;
        if (lx * lx + ly * ly > 40.0 * 40.0) continue;
        const double dx = via.x - px, dy = via.y - py;
        const double d2 = dx * dx + dy * dy;
        // sorted(near_points, key=squared distance): stable insertion keeps list order among equals
        // (the kept rows live in the output itself; a row's distance is recomputed from the table)
        int pos = cnt < c.via_max ? cnt : c.via_max;
        while (pos > 0) {
          const smx_via prev = a.vias[v_a + near[pos - 1]];
          const double ex = prev.x - px, ey = prev.y - py;
          if (ex * ex + ey * ey > d2)
            --pos;
          else
            break;
        }
        if (pos < c.via_max) {
          const int last = (cnt < c.via_max ? cnt : c.via_max - 1);
          for (int k = last; k > pos; --k) near[k] = near[k - 1];
          near[pos] = (int8_t)(v - v_a);
        }
        ++cnt;
        const int bit = 1 << (v - v_a);
        // np.isclose(speed, required_speed, atol=1.5) with the default rtol = 1e-5
        const bool speed_ok = fabs(speed - via.required_speed) <= 1.5 + 1e-5 * fabs(via.required_speed);
        if (d2 <= via.hit_distance * via.hit_distance && !(consumed & bit) && speed_ok) {
          consumed |= bit;
          hit |= bit;
        }
      }
      for (int k = (cnt < c.via_max ? cnt : c.via_max); k < c.via_max; ++k) near[k] = -1;
      o.via_near_count[gid] = (uint8_t)(cnt > 255 ? 255 : cnt);
      o.via_hit[gid] = hit;
      *consumed_p = (int32_t)consumed;
    }

    // ---- events + done (sensors.py:443-489)
    // Mission.is_complete -> PositionalGoal.is_reached (plan.py:116-120, 220-222); EndlessGoal never (:76-84)
    RouteFilter route;
    const bool fixed_route = route.fixed_route(a.missions, slot, m.n_roads);
    bool reached_goal = false;
    if (fixed_route) {
      const double gx = a.missions.goal[3 * slot], gy = a.missions.goal[3 * slot + 1], gr = a.missions.goal[3 * slot + 2];
      const double sqr_dist = (s.x - gx) * (s.x - gx) + (s.y - gy) * (s.y - gy);
      reached_goal = sqr_dist <= gr * gr;
    }
    // (a lap goal's distance condition waits for this tick's trip meter, which the waypoints role is still writing:
    // the commit role applies it, lap_goal_gate)
    if (__builtin_expect(a.missions.goal_kind != nullptr, 0) && a.missions.goal_kind[slot].kind == SMX_GOAL_TRAVERSE)
      reached_goal = drove_off_map(a.missions, m, n_veh, OWN_BOX ? ego_lane : my_lane, my_lane_dist, s.x, s.y, wrap_heading(s.heading));
    const bool is_off_road = !(my_facts & SMX_FACT_ON_ROAD);           // sensors.py:498-500
    const bool is_on_shoulder = ((my_facts >> SMX_FACT_CORNER_SHIFT) & 15) != 15;  // sensors.py:502-509
    const bool reached_max = c.max_episode_steps > 0 && steps >= c.max_episode_steps;
    bool is_off_route, is_wrong_way;
    {
      // sensors.py:527-594
      double radius = sqrt(SMX_CHASSIS_LENGTH * SMX_CHASSIS_LENGTH + SMX_CHASSIS_WIDTH * SMX_CHASSIS_WIDTH) * 0.5 + 5.0;
      if (OWN_BOX) {  // (sensors.py:548: the agent's own half diagonal)
        const VehBox my = vehicle_box(a, gid, true);
        radius = sqrt(my.length * my.length + my.width * my.width) * 0.5 + 5.0;
      }
      int nl = (my_lane >= 0 && my_lane_dist < radius) ? my_lane : -1;
      if (nl < 0) {
        is_off_route = true;
        is_wrong_way = false;
      } else {
        is_off_route = false;
        is_wrong_way = false;
        if (!m.lane_in_junction[nl] && !SMX_SKIP(a, 64)) {
          const double target = a.st.facts_f64[(size_t)SMX_FF_LANE_HEADING * total + gid];  // k_scan
          is_wrong_way = fabs(heading_relative_to(s.heading, target)) > 0.5 * SMX_PI;
        }
        // an endless mission has no route roads: on route (:556-561); else the nearest lane's road must be
        // one of them, or a junction, or the lane has an oncoming neighbour that is (:563-574)
        if (fixed_route && !route.has(m, m.lane_road[nl]) && !m.lane_in_junction[nl])
          is_off_route = !oncoming_lane_on_route(m, route, nl, lane_offset_along(m, nl, s.x, s.y));
      }
    }
    unsigned char* ev = stage.events[local];
    ev[SMX_EV_COLLISIONS] = collided ? 1 : 0;
    ev[SMX_EV_OFF_ROAD] = is_off_road ? 1 : 0;
    ev[SMX_EV_OFF_ROUTE] = is_off_route ? 1 : 0;
    ev[SMX_EV_ON_SHOULDER] = is_on_shoulder ? 1 : 0;
    ev[SMX_EV_WRONG_WAY] = is_wrong_way ? 1 : 0;
    ev[SMX_EV_NOT_MOVING] = is_not_moving ? 1 : 0;
    ev[SMX_EV_REACHED_GOAL] = reached_goal ? 1 : 0;
    ev[SMX_EV_REACHED_MAX_EPISODE_STEPS] = reached_max ? 1 : 0;
    // ---- DoneCriteria.agents_alive (sensors.py:404-441): agents registered at the start of the tick
    bool agents_alive_done = false;
    if (c.alive_min_ego > 0 || c.alive_min_total > 0 || c.alive_lists > 0) {
      unsigned long long alive_mask = 0ull;
      const int n_agents = n_veh - c.num_social;
      for (int j = 0; j < n_agents; ++j)
        if (env_pose[j].alive) alive_mask |= 1ull << j;
      const int n_alive = __popcll(alive_mask);
      // no social *agents* exist on this path, so every registered agent is an ego agent
      if (c.alive_min_ego > 0 && n_alive < c.alive_min_ego) agents_alive_done = true;
      if (c.alive_min_total > 0 && n_alive < c.alive_min_total) agents_alive_done = true;
      for (int k = 0; k < c.alive_lists && k < SMX_MAX_ALIVE_LISTS; ++k)
        if (__popcll(alive_mask & c.alive_list_mask[k]) < c.alive_list_min[k]) agents_alive_done = true;
    }
    ev[SMX_EV_AGENTS_ALIVE_DONE] = agents_alive_done ? 1 : 0;
    const uint32_t dc = c.done_criteria;
    done = (is_off_road && (dc & SMX_DONE_OFF_ROAD)) || reached_goal || reached_max ||
           (is_on_shoulder && (dc & SMX_DONE_ON_SHOULDER)) || (collided && (dc & SMX_DONE_COLLISION)) ||
           (is_not_moving && (dc & SMX_DONE_NOT_MOVING)) || (is_off_route && (dc & SMX_DONE_OFF_ROUTE)) ||
           (is_wrong_way && (dc & SMX_DONE_WRONG_WAY)) || agents_alive_done;
    if (first) done = false;  // sensors.py:465: `not sim.resetting and (...)`: reset observations never end an agent

    // ---- teardown (smarts.py:314, 329-363)
    flags &= ~(SMX_F_FIRST | SMX_F_ENTERING);
    if (done) flags &= ~SMX_F_ALIVE;
    a.st.steps[gid] = steps;
    new_flags = flags;  // applied by k_tail's commit: the waypoints role of this launch still reads the old word
    o.active[gid] = done ? 0 : 1;
    if (!a.keep_reward_done) {
      o.done[gid] = done ? 1 : 0;
      if (o.learner) o.learner[total + gid] = done ? 1.0f : 0.0f;
    }
  } else if (valid && !a.first_only) {
    if (o.learner && (!alive || social)) {
      o.learner[gid] = 0.0f;  // no agent in this slot: absent from the learner block
      o.learner[total + gid] = 0.0f;
    }
    // an agent whose vehicle is gone: absent from the observations (zeros), done stays 0
    if (!alive && (o.active[gid] != 0 || o.done[gid] != 0)) {
      atomicOr(&zero_mask, 1ull << local);
      o.done[gid] = 0;
      o.active[gid] = 0;
    }
  }
  if (valid) a.st.facts_i32[(size_t)SMX_FI_FLAGS_NEXT * total + gid] = new_flags;
  // ---- copy-out of the staged rows, every array in memory order over the workgroup's vehicles
  __syncthreads();
  SMX_TSTAMP(to2c);
  {
    const int nth = (int)blockDim.x;
    for (unsigned long long zm = zero_mask; zm != 0ull; zm &= zm - 1ull)  // (uniform in the workgroup)
      zero_dense_rows(a, (size_t)block * epb * n_veh + (__ffsll((long long)zm) - 1), local, nth);
    // (element -> vehicle, row: quotients by the run-time row lengths, below 4096 / by at most 64 — exact in float32
    // with half a unit added; an integer division is some forty instructions, and these sweeps were half the kernel)
    const float rcp_veh = 1.0f / (float)n_veh;
    const int wg_veh = epb * n_veh;                           // vehicles of this workgroup (<= 64), gids g0 ...
    const size_t g0 = (size_t)block * epb * n_veh;
    for (int e = local; e < wg_veh * 3; e += nth) {           // ego_pos
      const int v = e / 3, q = e - v * 3;
      if (!stage.mode[v]) continue;
      o.ego_pos[g0 * 3 + e] = q == 0 ? pose[v].x : (q == 1 ? pose[v].y : SMX_BASE_HEIGHT);
    }
    for (int e = local; e < wg_veh * SMX_EGO_F32_COUNT; e += nth) {
      const int v = e / SMX_EGO_F32_COUNT;
      if (stage.mode[v]) o.ego_f32[g0 * SMX_EGO_F32_COUNT + e] = stage.ego_f32[v][e - v * SMX_EGO_F32_COUNT];
    }
    for (int e = local; e < wg_veh * 2; e += nth)
      if (stage.mode[e >> 1]) o.ego_lane[g0 * 2 + e] = stage.ego_lane[e >> 1][e & 1];
    for (int e = local; e < wg_veh * SMX_EV_COUNT; e += nth) {
      const int v = e / SMX_EV_COUNT;
      if (stage.mode[v]) o.events[g0 * SMX_EV_COUNT + e] = stage.events[v][e - v * SMX_EV_COUNT];
    }
    if ((c.sensors & SMX_SENSOR_NEIGHBORS) && nb_staged && !SMX_SKIP(a, 8)) {
      const int K = c.nb_max;
      const float rcp_k3 = 1.0f / (float)(K * 3), rcp_k = 1.0f / (float)K;
      for (int e = local; e < wg_veh * K * 3; e += nth) {     // nb_pos, nb_box
        const int v = small_quotient(e, rcp_k3), r = e - v * (K * 3), k = r / 3, q = r - k * 3;
        if (!stage.mode[v]) continue;
        const bool held = k < (int)stage.nb_kept[v];
        const int mate = small_quotient(v, rcp_veh) * n_veh + (held ? (int)stage.nb_list[v][k] : 0);
        const SharedPose& P = pose[mate];
        o.nb_pos[g0 * K * 3 + e] = held ? (q == 0 ? P.x : (q == 1 ? P.y : SMX_BASE_HEIGHT)) : 0.0;
        float box = held ? (float)(q == 0 ? SMX_CHASSIS_LENGTH : (q == 1 ? SMX_CHASSIS_WIDTH : SMX_CHASSIS_HEIGHT)) : 0.0f;
        if (dims_sized(a) && held) box = (float)a.dims.slot[(g0 + mate) * 3 + q];
        o.nb_box[g0 * K * 3 + e] = box;
      }
      for (int e = local; e < wg_veh * K; e += nth) {         // the scalar neighbour rows
        const int v = small_quotient(e, rcp_k), k = e - v * K;
        if (!stage.mode[v]) continue;
        const bool held = k < (int)stage.nb_kept[v];
        const int j = held ? (int)stage.nb_list[v][k] : 0;
        const SharedPose& P = pose[small_quotient(v, rcp_veh) * n_veh + j];
        const size_t w = g0 * K + e;
        o.nb_heading[w] = held ? (float)P.heading : 0.0f;
        o.nb_speed[w] = held ? (float)P.speed : 0.0f;
        int nl = held ? P.nl : -1, nlidx = held ? P.nlidx : 0;
        if (OWN_BOX && held) {  // nearest_lane(nv.pose.point, radius = the observer's own length)
          nl = (P.lane >= 0 && P.lane_dist < a.dims.slot[(g0 + v) * 3]) ? P.lane : -1;
          nlidx = nl >= 0 ? m.lane_index[nl] : -1;
        }
        o.nb_lane_id[w] = (int16_t)nl;
        o.nb_lane_index[w] = (int8_t)nlidx;
        o.nb_slot[w] = (int8_t)(held ? j : -1);
      }
    }
  }
  SMX_TSTAMP(to3);
  SMX_TACC(6, to0, to3);
  SMX_TACC(45, to2c, to3);
}

// =================================================================================
// commit role (k_tail, k_first): the end of a pass, after every sensor role has read the old flags: apply the flags the
// observe role decided (teardown of done agents, smarts.py:314, 329-363), per-env done count and
// dones["__all__"] (hiway_env.py:258-261), and the auto-reset respawn (parallel_env.py:303-309) —
// the reset pass that follows builds the first observations of the restarted envs.
// One thread per vehicle, whole envs per workgroup.
// =================================================================================
// (`tick`: the tick's commit — every agent's teardown, done counts, auto-reset respawn; else the reset pass's, which
// only applies the new vehicles' flags)
// (GUARD, the tick's commit only: an agent that carries SMX_F_GUARDED ends with this tick's observation — done = 1, not
// active, its vehicle gone —, applied here as lap_goal_gate applies its correction: the observe role is the kernel
// without a guard; and the byte of every slot without an agent in the tick reads 0)
// A replayed social slot at the end of a pass (smx_set_social_history): SMX_F_ALIVE for the next tick is the slot's
// presence in the next tick's frame — the env's tick count after this pass (the tick's commit has not incremented it
// yet) plus one.  The same rule in the tick's commit and in the reset pass's, whose env groups also hold envs that were
// not reset: for those it finds what the tick's commit found.  An env that restarts is respawned after this, from its
// next episode's window.
// A vehicle that appears may be anywhere on the map, far from where the slot's last occupant left: its road facts must
// not be searched for from that occupant's carry.  The appearing vehicle's carry is invalidated (SMX_FI_LANE = -1 is "no
// usable carry" to both scan forms: scan_role starts from scratch, k_scan_fast hands the vehicle to its slow list); the
// path seeds are never asked of a social slot.
__device__ __forceinline__ int history_commit(const KernelArgs& a, size_t gid, size_t total, int env, int slot_in_env, int old_flags,
                                           int new_flags, bool tick) {
  const int slot = slot_in_env - (a.cfg.num_vehicles - a.cfg.num_social);
  int64_t frame;
  const bool present = history_slot_present(a, env, slot, a.st.env_episode[env], a.st.env_ticks[env] + (tick ? 2 : 1), frame);
  if (present && !(old_flags & SMX_F_ALIVE)) a.st.facts_i32[(size_t)SMX_FI_LANE * total + gid] = -1;
  return present ? (new_flags | SMX_F_ALIVE) : (new_flags & ~SMX_F_ALIVE);
}

template <bool GUARD>
__device__ __forceinline__ void commit_role(const KernelArgs& a, const int block, const bool tick) {
  __shared__ int env_new_done[SMX_BLOCK];
  __shared__ int env_respawn[SMX_BLOCK];
  __shared__ int env_first_alive[SMX_BLOCK];
  const smx_config& c = a.cfg;
  const smx_outputs& o = a.out;
  const int n_veh = c.num_vehicles;
  const int epb = SMX_BLOCK / n_veh;
  const int local = threadIdx.x;
  const int env_local = local / n_veh;
  const int slot = local - env_local * n_veh;
  const int env = block * epb + env_local;
  const bool valid = (env_local < epb) && (env < c.num_envs);
  const size_t total = (size_t)c.num_envs * n_veh;
  const size_t gid = valid ? ((size_t)env * n_veh + slot) : 0;
  if (local < SMX_BLOCK) {
    env_new_done[local] = 0;
    env_respawn[local] = 0;
  }
  __syncthreads();
  if (valid) {
    if (__builtin_expect(a.missions.goal_kind != nullptr, 0)) lap_goal_gate(a, gid, total, slot, tick);
    const int old_flags = a.st.flags[gid];
    int new_flags = a.st.facts_i32[(size_t)SMX_FI_FLAGS_NEXT * total + gid];
    if constexpr (GUARD) {
      if (tick) {
        const bool agent = (old_flags & SMX_F_ALIVE) && !(old_flags & SMX_F_SOCIAL);
        if (!agent) {
          a.guard[gid] = 0;
        } else if (old_flags & SMX_F_GUARDED) {  // (set by the control phase, or by the reset that created it parked)
          // The observe role's done path writes four words per agent — SMX_F_ALIVE off in the next flags, active,
          // done, the learner block's done — and these are the four: no other per-agent row depends on done (events,
          // reward and the learner's reward are what the held / parked pose yields, as for any agent), and what reads
          // done afterwards (the env's done count below, the frame pushes that end the pass) reads it as set here.
          new_flags &= ~SMX_F_ALIVE;
          o.active[gid] = 0;
          o.done[gid] = 1;
          if (o.learner) o.learner[total + gid] = 1.0f;
        }
      }
    }
    if (__builtin_expect(a.history.vehicle != nullptr, 0) && (old_flags & SMX_F_SOCIAL))
      new_flags = history_commit(a, gid, total, env, slot, old_flags, new_flags, tick);
    // A history agent whose vehicle left the recording in this tick (SMX_F_LEFT, k_control_kinematic's FOLLOW form) ends
    // with this tick's observation, applied as the guard's done above is: the same four words.
    if (__builtin_expect(a.history.follow != nullptr, 0) && tick && (old_flags & (SMX_F_ALIVE | SMX_F_LEFT | SMX_F_SOCIAL)) == (SMX_F_ALIVE | SMX_F_LEFT)) {
      new_flags &= ~SMX_F_ALIVE;
      o.active[gid] = 0;
      o.done[gid] = 1;
      if (o.learner) o.learner[total + gid] = 1.0f;
    }
    a.st.flags[gid] = new_flags;
    // (agents only: a replayed social vehicle that leaves its history is not a finished agent; a scripted one never ends)
    if ((old_flags & SMX_F_ALIVE) && !(new_flags & SMX_F_ALIVE) && !(old_flags & SMX_F_SOCIAL)) atomicAdd(&env_new_done[env_local], 1);
    if (slot == 0) env_first_alive[env_local] = (new_flags & SMX_F_ALIVE) ? 1 : 0;
  }
  __syncthreads();
  if (valid && slot == 0) {
    if (tick) {
      int dcnt = a.st.env_done_count[env] + env_new_done[env_local];
      a.st.env_done_count[env] = dcnt;
      a.st.env_ticks[env] = a.st.env_ticks[env] + 1;
      bool all_done = dcnt >= n_veh - c.num_social;  // every agent (hiway_env.py:258-261)
      o.env_done[env] = all_done ? 1 : 0;
      a.st.env_reset_pending[env] = 0;
      env_respawn[env_local] = (all_done && c.auto_reset) ? 1 : 0;
    } else if (!a.keep_reward_done) {
      if (a.st.env_done_count[env] == 0 && env_first_alive[env_local]) o.env_done[env] = 0;
    }
  }
  __syncthreads();
  const bool respawn = valid && env_respawn[valid ? env_local : 0] != 0;
  int next_episode = 0;
  if (respawn && o.final_ego_pos != nullptr) {
    // the finishing tick's rows, before the reset pass writes the next episode's first observation over them
    // (parallel_env.py:303-309: what info[agent]["env_obs"] holds for the agents that ended with their env)
    for (int k = 0; k < 3; ++k) o.final_ego_pos[gid * 3 + k] = o.ego_pos[gid * 3 + k];
    for (int k = 0; k < SMX_EGO_F32_COUNT; ++k) o.final_ego_f32[gid * SMX_EGO_F32_COUNT + k] = o.ego_f32[gid * SMX_EGO_F32_COUNT + k];
    o.final_ego_lane[gid * 2] = o.ego_lane[gid * 2];
    o.final_ego_lane[gid * 2 + 1] = o.ego_lane[gid * 2 + 1];
    for (int k = 0; k < SMX_EV_COUNT; ++k) o.final_events[gid * SMX_EV_COUNT + k] = o.events[gid * SMX_EV_COUNT + k];
    o.final_dist[gid] = o.dist[gid];
  }
  if (respawn) {
    next_episode = a.st.env_episode[env] + 1;
    respawn_vehicle<GUARD>(a, gid, total, next_episode);
  }
  __syncthreads();  // every thread of the env has read env_episode
  if (respawn && slot == 0) {
    a.st.env_episode[env] = next_episode;
    // (history agents that do not enter count as finished from the start; the barrier above has the env's new flags)
    a.st.env_done_count[env] = __builtin_expect(a.history.follow != nullptr, 0) ? history_agents_absent(a, env) : 0;
    a.st.env_ticks[env] = c.reset_elapsed_steps;
  }
}


// =================================================================================
// k_sensors: the observation of a pass as ONE launch whose workgroups take different roles —
// waypoint paths + trip meter (4 lanes / vehicle), the rest of Sensors.observe (1 lane / vehicle,
// whole envs per workgroup) and, if enabled, lidar and OGM (1 wavefront / vehicle each).  The roles read the
// same pose / flags / facts and write disjoint outputs, so they overlap in time; the flags word
// itself only changes in the commit role.
// =================================================================================
// (SIZED: a triple block is bound, TickPlan::sized — the observe role with the agent's own box)
template <int SIZED>
__device__ __forceinline__ void sensors_roles(const KernelArgs& a) {
  const int b = (int)blockIdx.x;
  if (b < a.wp_blocks) {
    waypoints_role(a, b);
  } else if (b < a.wp_blocks + a.obs_blocks) {
    observe_role(a, b - a.wp_blocks, SIZED != 0);
  } else if (b < a.wp_blocks + a.obs_blocks + a.lidar_blocks) {
    lidar_role<-1>(a, b - a.wp_blocks - a.obs_blocks);
  } else {
    ogm_role(a, b - a.wp_blocks - a.obs_blocks - a.lidar_blocks);
  }
}
__global__ void __launch_bounds__(SMX_BLOCK) k_sensors(const KernelArgs a) { sensors_roles<0>(a); }
__global__ void __launch_bounds__(SMX_BLOCK) k_sensors_sized(const KernelArgs a) { sensors_roles<1>(a); }

// =================================================================================
// k_first: the reset pass (first observations of re-created vehicles) as ONE launch.  A workgroup
// owns the envs of one observe-role group and runs scan -> sensors -> commit for their new vehicles
// itself, phase after phase; results pass between phases through global memory behind a fence and a
// barrier.  It runs over the env groups k_tail listed (new vehicles in them); OGM / DAGM tiles need
// dynamic LDS and come from k_tail.
// =================================================================================
// (eight wavefronts: the (vehicle, scan half) pairs of a restarted 64-vehicle env are 128 teams of eight lanes — four
// rounds of ~55 us each in a workgroup of 256, the largest piece of C5's reset pass; the waypoint teams, four lanes a
// vehicle, fit the first 256 threads, whose knot scratch is all the LDS the workgroup may have)
#define SMX_FIRST_BLOCK 512
#define SMX_FIRST_WP_THREADS 256
template <int SIZED>
__device__ __forceinline__ void first_role(const KernelArgs& a, const int block) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_FIRST_WP_THREADS];
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const int n_veh = c.num_vehicles;
  const int epb = SMX_BLOCK / n_veh;  // the env groups are those of the observe / commit roles
  const size_t total = (size_t)c.num_envs * n_veh;
  const size_t g0 = (size_t)block * epb * n_veh;
  const size_t g1 = min(total, g0 + (size_t)epb * n_veh);
  int mine_first = 0;
  if (g0 + threadIdx.x < g1) {
    const int f = a.st.flags[g0 + threadIdx.x];
    mine_first = (f & SMX_F_ALIVE) && (f & SMX_F_FIRST);
  }
  const int n_new = __syncthreads_count(mine_first);
  if (n_new == 0) return;
  SMX_TSTAMP(tk0);
  // More new vehicles than one round of (vehicle, scan half) teams holds (a 64-vehicle env of C5: 128 pairs for 64
  // teams): the seeds halves take the round — the waypoint rows wait for nothing else —, and the facts halves
  // then run BESIDE the rows' serial emitter (minicity: 220 us of a restarted env's 410) on the
  // workgroup's other four wavefronts; observe needs both.  Fewer: one round serves both halves as before.
  const bool split = 2 * n_new > SMX_FIRST_BLOCK / SMX_TEAM;
  // The workgroup is four wavefronts wide: a restarted env's chain scan -> sensors -> commit is
  // pure latency, so its independent pieces run side by side — (vehicle, scan half) pairs over the
  // teams of all four wavefronts, then the vehicles' waypoint teams — instead of one after the
  // other in a single wavefront (an env of 16 vehicles: 4 scan rounds of ~40 us became 1).
  // ---- scan: one team per (vehicle, half)
  // (one scan call site inside a two-turn loop: inlined three times the kernel spilled 2 KB per lane)
#pragma nounroll
  for (int turn = 0; turn < 2; ++turn) {
    SMX_TSTAMP(tt0);
    // turn 0: every team scans — both halves of a vehicle (pair = 2 x vehicle + half), or the seeds halves only;
    // turn 1: the first 256 threads emit the rows, and the other 32 teams take the facts halves left over
    const bool scans = turn == 0 || (split && threadIdx.x >= SMX_FIRST_WP_THREADS);
    if (scans) {
      const int teams = turn == 0 ? SMX_FIRST_BLOCK / SMX_TEAM : (SMX_FIRST_BLOCK - SMX_FIRST_WP_THREADS) / SMX_TEAM;
      const int team = ((int)threadIdx.x - (turn == 0 ? 0 : SMX_FIRST_WP_THREADS)) / SMX_TEAM;
      const bool both = turn == 0 && !split;
      const size_t units = both ? (g1 - g0) * 2 : (g1 - g0);
      for (size_t u0 = 0; u0 < units; u0 += teams) {
        const size_t u = u0 + team;
        if (u < units) {
          const size_t gid = g0 + (both ? (u >> 1) : u);
          const int half = both ? (int)(u & 1) : (turn == 0 ? 1 : 0);
          const int flags = a.st.flags[gid];
          if ((flags & SMX_F_ALIVE) && (flags & SMX_F_FIRST)) scan_role<SMX_TEAM, true, SIZED>(a, m, c, gid, total, team_rank<SMX_TEAM>(), flags, half);
        }
      }
    } else if (turn == 1 && threadIdx.x < SMX_FIRST_WP_THREADS) {  // (whole wavefronts; waypoints_for holds no barrier)
      for (size_t base = g0; base < g1; base += SMX_FIRST_WP_THREADS / SMX_WP_LANES) {
        const size_t gid = base + threadIdx.x / SMX_WP_LANES;
        if (gid < g1) waypoints_for<SMX_FIRST_WP_THREADS>(a, gid, knot_scratch + threadIdx.x);
      }
    }
    __threadfence();
    __syncthreads();
    SMX_TSTAMP(tt1);
    SMX_TACC_ALL(turn == 0 ? 57 : 58, tt0, tt1);
  }
  SMX_TSTAMP(tk2);
  observe_role(a, block, SIZED != 0);
  SMX_TSTAMP(tk3);
  SMX_TACC_ALL(59, tk2, tk3);
  if ((c.sensors & SMX_SENSOR_LIDAR) && a.lidar_blocks != 0)  // (0: the reset pass launched k_lidar for the new vehicles)
    for (size_t gid = g0; gid < g1; ++gid) {
      lidar_role<-1>(a, (int)gid);
      __syncthreads();  // the role's LDS block is reused by the next vehicle
    }
  __threadfence();
  __syncthreads();
  // ---- commit
  SMX_TSTAMP(tk4);
  commit_role<false>(a, block, false);  // (the reset pass's commit has no guard work: respawn_vehicle wrote the bytes)
  SMX_TSTAMP(tk5);
  SMX_TACC_ALL(60, tk4, tk5);
  SMX_TACC_ALL(61, tk0, tk5);
  // ---- large batches: the new vehicles' knot lists, so that the next tick's k_control_fast serves them too (a new
  // vehicle without lists went through the slow controller, two launches of pure latency in front of everything else
  // of the tick).  New here: alive, SMX_F_FIRST just cleared by the commit, one step old.
  if (a.walk_new) {
    __threadfence();
    __syncthreads();
    for (size_t base = g0; base < g1; base += SMX_FIRST_BLOCK / SMX_WP_LANES) {
      const size_t gid = base + threadIdx.x / SMX_WP_LANES;
      if (gid >= g1) continue;
      const int f = a.st.flags[gid];
      if ((f & SMX_F_ALIVE) && !(f & SMX_F_SOCIAL) && !(f & SMX_F_FIRST) && a.st.steps[gid] == 1) {
        wp_walk_for(a, gid, (int)threadIdx.x % SMX_WP_LANES, false, true);  // (the reset pass's flag word says "new vehicles only")
      }
    }
  }
}

// The reset pass over the env groups k_tail found new vehicles in (`groups`, `*n_groups` of them): workgroup i takes
// entry i, and the rest leave after one scalar load instead of a flags load and a barrier count.  (A fixed grid
// striding the list would launch eight times fewer workgroups, but the loop around the role spilled 112 registers of
// its 256: 436 bytes of scratch a lane.)
__global__ void __launch_bounds__(SMX_FIRST_BLOCK) k_first(const KernelArgs a, const int32_t* groups, const int32_t* n_groups) {
  if ((int)blockIdx.x >= *n_groups) return;
  first_role<0>(a, groups[blockIdx.x]);
}
// (... with a triple block bound, TickPlan::sized: the scan and observe roles with the agent's own box)
__global__ void __launch_bounds__(SMX_FIRST_BLOCK) k_first_sized(const KernelArgs a, const int32_t* groups, const int32_t* n_groups) {
  if ((int)blockIdx.x >= *n_groups) return;
  first_role<1>(a, groups[blockIdx.x]);
}

// =================================================================================
// k_road_waypoints: RoadWaypointsSensor (sensors.py:991-1040).  SMX_RW_LANE_CAP lanes of a wavefront share a
// vehicle: every lane of the team builds the sensor's lane list for itself (the same serial steps, so the
// team does not diverge), then team lane l follows road lane l: start `horizon` metres behind the vehicle
// along the lane (through its incoming lanes, depth first in their order, where the lane is shorter), and from
// each start every lanepoint path of lookahead 2 x horizon, interpolated like the waypoints sensor's
// (equally_spaced_path, its knots in private memory: up to 2 x horizon + 2 of them).  An optional sensor off
// the headline configurations: written for parity, not for throughput.
// Where the reference cannot answer — the nearest lane is junction-internal: Road.parallel_roads asks sumolib
// for the internal edge's from-node, which is None, and raises — the road has no parallel roads here.
// =================================================================================
#define SMX_RW_MAX_KNOTS (2 * SMX_RW_HORIZON_MAX + 4)
#define SMX_RW_STACK 24
struct RwLanes {
  int n;  // lanes the sensor reports (the list keeps the first SMX_RW_LANE_CAP)
  int lane[SMX_RW_LANE_CAP];
  // lane_paths[lane.lane_id] = ...: a lane met again keeps its first place in the dict
  __device__ __forceinline__ void add_road(const MapDev& m, int road) {
    for (int k = m.road_lane_off[road]; k < m.road_lane_off[road + 1]; ++k) {
      const int ln = m.road_lanes[k];
      bool seen = false;
      for (int q = 0; q < min(n, SMX_RW_LANE_CAP); ++q) seen = seen || lane[q] == ln;
      if (seen) continue;
      if (n < SMX_RW_LANE_CAP) lane[n] = ln;
      ++n;
    }
  }
};

__global__ void __launch_bounds__(SMX_BLOCK) k_road_waypoints(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const smx_outputs& o = a.out;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t tid = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  const size_t gid = tid / SMX_RW_LANE_CAP;
  const int l = (int)(tid % SMX_RW_LANE_CAP);
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE) || (flags & SMX_F_SOCIAL) || (a.first_only && !(flags & SMX_F_FIRST))) return;
  const int L = c.rw_lanes, P = c.rw_paths, H = c.rw_horizon, R = 2 * H + 1;
  const double px = SF(SMX_S_X), py = SF(SMX_S_Y);
  // ---- the sensor's lanes: nearest lane's road, its parallel roads, the roads oncoming at the point
  RwLanes lanes;
  lanes.n = 0;
  // road_map.nearest_lane(point) (road_map.py:91-96, the default radius); asked here rather than taken from
  // k_scan so that the kernel also serves the reset pass, whose scan runs inside k_first
  // In a tick the scan's facts half has just answered it (the nearest lane and its distance: the observe role reads
  // its ego lane the same way); only the reset pass, whose scan runs inside k_first after this kernel, asks here —
  // every lane of the team repeating a one-lane ring search was the longest piece of the kernel.
  int near_lane = -1;
  if (!a.first_only) {
    const int ln = a.st.facts_i32[(size_t)SMX_FI_LANE * total + gid];
    const double dd = a.st.facts_f64[(size_t)SMX_FF_LANE_DIST * total + gid];
    near_lane = (ln >= 0 && dd < fmax(10.0, 2.0 * m.default_lane_width)) ? ln : -1;
  } else {
    near_lane = road_facts_scan(m, px, py, fmax(10.0, 2.0 * m.default_lane_width), 0, nullptr, nullptr).lane;
  }
  if (near_lane >= 0) {
    const int road = m.lane_road[near_lane];
    lanes.add_road(m, road);
    for (int k = m.road_par_off[road]; k < m.road_par_off[road + 1]; ++k) lanes.add_road(m, m.road_par_idx[k]);
    // Road.oncoming_roads_at_point (sumo_road_network.py:596-605)
    for (int k = m.road_lane_off[road]; k < m.road_lane_off[road + 1]; ++k) {
      const int ln = m.road_lanes[k];
      const double off = lane_offset_along(m, ln, px, py);
      oncoming_lanes_at_offset(m, ln, off, [&](int other) {
        if (m.lane_road[other] != road) lanes.add_road(m, m.lane_road[other]);
      });
    }
  }
  if (l == 0) o.rw_lane_count[gid] = (uint8_t)min(lanes.n, 255);
  if (l >= L) return;
  const size_t lane_row = gid * (size_t)L + l;
  const bool mine = l < min(lanes.n, SMX_RW_LANE_CAP);
  int my_lane = -1;
#pragma unroll
  for (int q = 0; q < SMX_RW_LANE_CAP; ++q)
    if (q == l && mine) my_lane = lanes.lane[q];
  o.rw_lane[lane_row] = (int16_t)my_lane;
  int n_paths = 0;
  if (my_lane >= 0) {
    RouteFilter f;  // route = plan.route: a fixed route filters, the endless mission's empty route does not
    f.fixed_route(a.missions, (int)(gid % (size_t)c.num_vehicles), m.n_roads);
    // ---- paths_for_lane (sensors.py:1014-1040): depth first through the incoming lanes
    int st_lane[SMX_RW_STACK];
    double st_start[SMX_RW_STACK];
    int sp = 0;
    st_lane[sp] = my_lane;
    st_start[sp] = lane_offset_along(m, my_lane, px, py) - (double)H;
    ++sp;
    int knots[SMX_RW_MAX_KNOTS];
    while (sp > 0) {
      --sp;
      const int ln = st_lane[sp];
      double start_offset = st_start[sp];
      const int ia = m.lane_in_off[ln], ib = m.lane_in_off[ln + 1];
      if (start_offset < 0.0 && ib > ia) {
        // children in reverse so that the first incoming lane is taken up first (a full stack drops the rest:
        // rows of at most rw_paths paths are kept anyway, the count then reads low)
        for (int k = ib - 1; k >= ia; --k) {
          if (sp >= SMX_RW_STACK) break;
          const int child = m.lane_in_idx[k];
          st_lane[sp] = child;
          st_start[sp] = m.lane_length[child] + start_offset;
          ++sp;
        }
        continue;
      }
      start_offset = fmax(0.0, start_offset);
      double wx, wy;
      lane_point_at_offset(m, ln, start_offset, wx, wy);
      int key[4] = {ln, -9, -9, -9};
      int idx4[4];
      closest_filtered4(m, wx, wy, key, 1, false, idx4, nullptr);
      const int start = idx4[0];
      if (start < 0) continue;
      BranchState bs;
      bs.reset();
      do {
        const bool kept = n_paths < P;
        const size_t row = (lane_row * (size_t)P + (size_t)(kept ? n_paths : 0)) * (size_t)R;
        const int n = equally_spaced_path<SMX_RW_MAX_KNOTS>(m, f, bs, start, 2 * H, wx, wy, knots, 1, kept ? R : 0,
                                                            [&](int i, const WaypointOut& w) {
                                                              double* d = o.rw_pos + (row + i) * 3;
                                                              d[0] = w.x;
                                                              d[1] = w.y;
                                                              d[2] = 0.0;
                                                              o.rw_heading[row + i] = (float)w.heading;
                                                              o.rw_lane_width[row + i] = (float)w.width;
                                                              o.rw_speed_limit[row + i] = (float)w.speed;
                                                              o.rw_lane_index[row + i] = (int8_t)m.lane_index[w.lane];
                                                              o.rw_lane_id[row + i] = (int16_t)w.lane;
                                                            });
        if (kept) o.rw_count[lane_row * (size_t)P + n_paths] = (uint8_t)min(n, R);
        if (n_paths < 32767) ++n_paths;
      } while (bs.advance());
    }
  }
  o.rw_path_count[lane_row] = (int16_t)n_paths;
  for (int p = min(n_paths, P); p < P; ++p) o.rw_count[lane_row * (size_t)P + p] = 0;
}

// =================================================================================
// k_lane_ttc: lane_ttc (custom_observations.py:148-280) of every agent with an observation, from the dense rows this
// pass has just written (wp_*, nb_*, ego_*) — the function smarts_amd/env/lane_ttc_rows.py restates on the host.
// SMX_TTC_TEAM lanes of a wavefront share an agent:
//  - the team stages the agent's waypoints (x, y, lane id, per-path counts) in LDS, one coalesced sweep of the rows;
//  - segment lengths in parallel, then lane p sums path p's in waypoint order: the reference's arclength is a
//    sequential float64 sum (:206-211) and is not re-associated;
//  - lane k takes neighbour k and walks the flat (path, waypoint) order itself, so min()'s "first of equal distances"
//    (:230-232) is the loop's own strict `<` (every lane of the team reads the same LDS word: a broadcast, no bank
//    conflict); the distances compared are the square roots, as in the reference — two different squares can round
//    to one root — but a root is only taken of a square smaller than the best one so far;
//  - the per-path minima (:251-254) are LDS atomic minima over the bit patterns: every value is positive (ttc <= 0 is
//    discarded, the defaults are 1000 and 1), so the unsigned order is the numeric one and the result exact whatever
//    the order of arrival;
//  - lane 0 picks the closest first waypoint, indexes the per-path lists by its lane index (_ego_ttc_calc, :259-280,
//    the quirk included) and writes the row.
// In a tick the grid covers every vehicle and flags are still those of the tick's start (k_tail commits later): an
// agent alive then has an observation.  In the reset pass (`groups` set) it covers the env groups k_tail listed, after
// k_first has written the new vehicles' first observations and committed their flags: an alive agent's rows are its
// first observation (a restarted env) or this tick's (the env beside it in the group: the same row again).
// Its cost per tick and what bounds it have not been measured; it re-reads up to 3.4 KB of rows per agent
// at 4 x 33 waypoints and ten neighbours.
// =================================================================================
__global__ void __launch_bounds__(SMX_BLOCK) k_lane_ttc(const KernelArgs a, const int32_t* groups, const int32_t* n_groups) {
  extern __shared__ __align__(16) unsigned char ttc_lds[];
  constexpr int T = SMX_TTC_TEAM, APB = SMX_BLOCK / T;
  const smx_config& c = a.cfg;
  const smx_outputs& o = a.out;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const int team = (int)threadIdx.x / T, r = (int)threadIdx.x % T;
  size_t gid;
  bool in_range;
  if (groups) {
    constexpr int BPG = SMX_BLOCK / APB;  // workgroups per env group (up to SMX_BLOCK vehicles)
    const int entry = (int)blockIdx.x / BPG;
    if (entry >= *n_groups) return;  // (uniform in the workgroup)
    const int n_veh = c.num_vehicles, epb = SMX_BLOCK / n_veh;
    const size_t g0 = (size_t)groups[entry] * epb * n_veh;
    gid = g0 + (size_t)((int)blockIdx.x % BPG) * APB + team;
    in_range = gid < min(total, g0 + (size_t)epb * n_veh);
  } else {
    gid = (size_t)blockIdx.x * APB + team;
    in_range = gid < total;
  }
  const int P = c.wp_paths, W = c.wp_len, K = c.nb_max, PW = P * W;
  unsigned char* base = ttc_lds + (size_t)team * smx_ttc_lds_per_agent(P, W);
  double* wx = reinterpret_cast<double*>(base);
  double* wy = wx + PW;
  double* cum = wy + PW;
  unsigned long long* ttc_min = reinterpret_cast<unsigned long long*>(cum + PW);
  unsigned long long* dtc_min = ttc_min + P;
  int* cnt = reinterpret_cast<int*>(dtc_min + P);
  short* lid = reinterpret_cast<short*>(cnt + P);

  const int flags = in_range ? a.st.flags[gid] : 0;
  const bool agent = in_range && (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL);
  const int n_total = agent ? (int)o.wp_count[gid * (P + 1)] : 0;  // paths the sensor found
  const int n_paths = min(n_total, P);                             // ... and the rows kept
  for (int p = r; p < n_paths; p += T) {
    cnt[p] = min((int)o.wp_count[gid * (P + 1) + 1 + p], W);
    ttc_min[p] = (unsigned long long)__double_as_longlong(1000.0);
    dtc_min[p] = (unsigned long long)__double_as_longlong(1.0);
  }
  __syncthreads();
  bool ok = n_paths > 0;  // an observation with at least one path, none of them empty (path[0], :164)
  for (int p = 0; p < n_paths; ++p) ok = ok && cnt[p] > 0;
  const int np = ok ? n_paths : 0;
  // ---- stage the waypoints
  for (int p = 0; p < np; ++p) {
    const int n = cnt[p];
    const size_t row = (gid * P + p) * W;
    for (int w = r; w < n; w += T) {
      wx[p * W + w] = o.wp_pos[(row + w) * 3];
      wy[p * W + w] = o.wp_pos[(row + w) * 3 + 1];
      lid[p * W + w] = o.wp_lane_id[row + w];
    }
  }
  __syncthreads();
  // ---- arclength (:206-211): the segment lengths side by side, then one lane per path adds them in order
  for (int p = 0; p < np; ++p) {
    const int n = cnt[p];
    for (int w = r; w + 1 < n; w += T) {
      const int i = p * W + w;
      const double dx = wx[i + 1] - wx[i], dy = wy[i + 1] - wy[i];
      cum[i + 1] = sqrt(dx * dx + dy * dy);
    }
  }
  __syncthreads();
  for (int p = r; p < np; p += T) {
    const int n = cnt[p];
    double acc = 0.0;
    cum[p * W] = 0.0;
    for (int w = 1; w < n; ++w) {
      acc += cum[p * W + w];
      cum[p * W + w] = acc;
    }
  }
  __syncthreads();
  // ---- neighbours (:217-254): lane k takes neighbour k
  const int nb_total = ok ? (int)o.nb_count[gid] : 0;
  const int nb_kept = min(nb_total, K);
  const double ego_speed = ok ? (double)o.ego_f32[gid * SMX_EGO_F32_COUNT + SMX_EGO_SPEED] : 0.0;
  for (int k = r; k < nb_kept; k += T) {
    const size_t q = gid * K + k;
    const int v_lane = o.nb_lane_id[q];
    if (v_lane < 0) continue;  // no lane: never the lane of a waypoint
    const double vx = o.nb_pos[q * 3], vy = o.nb_pos[q * 3 + 1];
    double best_gap = SMX_INF, best_sq = SMX_INF;
    int best_i = -1, best_p = 0;
    for (int p = 0; p < np; ++p) {
      const int n = cnt[p];
      for (int w = 0; w < n; ++w) {
        const int i = p * W + w;
        if (lid[i] != v_lane) continue;
        const double dx = wx[i] - vx, dy = wy[i] - vy;
        const double sq = dx * dx + dy * dy;
        if (sq < best_sq) {
          const double gap = sqrt(sq);
          if (gap < best_gap) {  // (an equal root keeps the earlier waypoint)
            best_gap = gap;
            best_sq = sq;
            best_i = i;
            best_p = p;
          }
        }
      }
    }
    if (best_i < 0 || best_gap > 2.0) continue;
    const double lane_dist = cum[best_i];
    double rel = (ego_speed - (double)o.nb_speed[q]) * 1000.0 / 3600.0;
    if (fabs(rel) < 1e-5) rel = 1e-5;
    const double ttc = lane_dist / rel / 10.0;
    if (ttc <= 0.0) continue;
    atomicMin(&ttc_min[best_p], (unsigned long long)__double_as_longlong(ttc));
    atomicMin(&dtc_min[best_p], (unsigned long long)__double_as_longlong(lane_dist / 100.0));
  }
  __syncthreads();
  if (r != 0 || !in_range) return;
  if (!ok) {
    // no observation, or one without paths: flags 0, the row untouched (reset pass: a vehicle that ended in this
    // tick keeps the tick's row)
    if (!groups || (flags & SMX_F_ALIVE)) o.lane_ttc_flags[gid] = 0;
    return;
  }
  // ---- the closest first waypoint (:164-170), first of equals
  const double ex = o.ego_pos[gid * 3], ey = o.ego_pos[gid * 3 + 1];
  int first = 0;
  double first_d = SMX_INF;
  for (int p = 0; p < np; ++p) {
    const double dx = wx[p * W] - ex, dy = wy[p * W] - ey;
    const double d = sqrt(dx * dx + dy * dy);
    if (d < first_d) {
      first_d = d;
      first = p;
    }
  }
  const size_t fq = (gid * P + first) * W;
  const double wp_heading = wrap_heading((double)o.wp_heading[fq]);
  const double ego_heading = wrap_heading((double)o.ego_f32[gid * SMX_EGO_F32_COUNT + SMX_EGO_HEADING]);
  double dvx, dvy;
  radians_to_vec(wp_heading, dvx, dvy);  // Heading.direction_vector (coordinates.py:241-243)
  const double lateral = signed_dist_to_line(ex, ey, wx[first * W], wy[first * W], dvx, dvy);  // road_map.py:608-614
  double* row = o.lane_ttc + gid * SMX_TTC_COUNT;
  row[SMX_TTC_DIST_FROM_CENTER] = lateral / ((double)o.wp_lane_width[fq] * 0.5);
  row[SMX_TTC_ANGLE_ERROR] = heading_relative_to(wp_heading, ego_heading);
  // ---- _ego_ttc_calc (:259-280): the per-path lists indexed by LANE index
  const int li = (int)o.wp_lane_index[fq];
  const bool index_error = li < 0 || li >= np;
  for (int j = 0; j < 3; ++j) {
    const int p = li - 1 + j;  // right, current, left
    const bool have = !index_error && p >= 0 && p < np;
    row[SMX_TTC_TTC + j] = have ? __longlong_as_double((long long)ttc_min[p]) : 0.0;
    row[SMX_TTC_DTC + j] = have ? __longlong_as_double((long long)dtc_min[p]) : 0.0;
  }
  const bool truncated = n_total > P || nb_total > K || W < c.wp_lookahead + 1;
  o.lane_ttc_flags[gid] = (uint8_t)(SMX_TTC_VALID | (nb_total > 0 ? SMX_TTC_STD : 0) | (truncated ? SMX_TTC_TRUNCATED : 0) |
                                    (index_error ? SMX_TTC_INDEX_ERROR : 0));
}

// =================================================================================
// k_ego_frame (SMX_SENSOR_EGO_CENTRIC): the reference's ego_centric_observation_adapter
// (smarts/core/utils/adapters/ego_centric_adapters.py:60-176) over the dense rows this pass has just written — the
// function smarts_amd/env/ego_centric_rows.py restates on the host.  A pure streaming transform: every position and
// heading of the waypoint, neighbour, lidar and road-waypoint rows is read once and written once into its ec_* twin.
// SMX_EC_TEAM lanes of a wavefront share an agent:
//  - lane 0 of the team reads the float64 heading H the observe role rounded into ego_f32 (wrap_heading of the state's)
//    and takes cos(-H), sin(-H) once (_gen_ego_frame_matrix, math.py:464-470: a float64 sincos is some hundred
//    instructions on this chip, a point's transform four); the team gets them by a cross-lane read;
//  - the team walks each [..][3] float64 row element by element in memory order, lane r element r, r + 16, ...: a store
//    instruction of the team writes one 128-byte line, and the x and y an element needs are in the lines its
//    neighbours read;
//  - the per-path counts bound the loops (a path is skipped or walked whole; no lane-dependent branch inside a row
//    beyond the select of the component).
// The launch sites and the meaning of `groups` are k_lane_ttc's: in a tick every vehicle (flags are those of the tick's
// start: an agent alive then has an observation), in the reset pass the env groups k_tail listed, after k_first.
// =================================================================================
// wrap_value(value, -pi, pi) (math.py:452-461): (-pi, pi], both branches tested on the value that came in
__device__ __forceinline__ double wrap_value_pi(double value) {
  double v = value;
  if (value <= -SMX_PI) v = SMX_PI - py_mod(-SMX_PI - value, SMX_TWO_PI);
  if (value > SMX_PI) v = -SMX_PI + py_mod(value - SMX_PI, SMX_TWO_PI);
  return v;
}

struct EgoFrame {
  double px, py, pz, H, cs, sn;  // cs = cos(-H), sn = sin(-H)
};

// position_to_ego_frame (math.py:473-487) over `n` points of a [..][3] row; `flat`: the row's z is written as 0 (a
// waypoint: transform(np.append(wp.pos, [0]))[:2], adapter :93); `hit`: per point, 0 = write three NaNs (a lidar miss)
__device__ __forceinline__ void ec_points(const EgoFrame& f, const double* __restrict__ src, double* __restrict__ dst, int n, int r,
                                          bool flat, const uint8_t* hit) {
  for (int i = r; i < 3 * n; i += SMX_EC_TEAM) {
    const int q = i / 3, comp = i - 3 * q;
    const double dx = src[3 * q] - f.px, dy = src[3 * q + 1] - f.py;
    double v = comp == 0 ? f.cs * dx - f.sn * dy : comp == 1 ? f.sn * dx + f.cs * dy : (flat ? 0.0 : src[i] - f.pz);
    if (hit && !hit[q]) v = __builtin_nan("");
    dst[i] = v;
  }
}
// Heading(wrap_value(h - H, -pi, pi)) (adapter :72-73, :94) over `n` float32 headings
__device__ __forceinline__ void ec_headings(const EgoFrame& f, const float* __restrict__ src, float* __restrict__ dst, int n, int r) {
  for (int i = r; i < n; i += SMX_EC_TEAM) dst[i] = (float)wrap_heading(wrap_value_pi((double)src[i] - f.H));
}

__global__ void __launch_bounds__(SMX_BLOCK) k_ego_frame(const KernelArgs a, const int32_t* groups, const int32_t* n_groups) {
  constexpr int T = SMX_EC_TEAM, APB = SMX_BLOCK / T;
  const smx_config& c = a.cfg;
  const smx_outputs& o = a.out;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const int team = (int)threadIdx.x / T, r = (int)threadIdx.x % T;
  size_t gid;
  bool in_range;
  if (groups) {
    constexpr int BPG = SMX_BLOCK / APB;  // workgroups per env group (up to SMX_BLOCK vehicles)
    const int entry = (int)blockIdx.x / BPG;
    if (entry >= *n_groups) return;  // (uniform in the workgroup)
    const int n_veh = c.num_vehicles, epb = SMX_BLOCK / n_veh;
    const size_t g0 = (size_t)groups[entry] * epb * n_veh;
    gid = g0 + (size_t)((int)blockIdx.x % BPG) * APB + team;
    in_range = gid < min(total, g0 + (size_t)epb * n_veh);
  } else {
    gid = (size_t)blockIdx.x * APB + team;
    in_range = gid < total;
  }
  const int flags = in_range ? a.st.flags[gid] : 0;
  const bool agent = in_range && (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL);
  EgoFrame f{0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  if (agent && r == 0) {
    f.H = wrap_heading(SF(SMX_S_HEADING));  // what k_observe rounds into ego_f32[SMX_EGO_HEADING]
    sincos(-f.H, &f.sn, &f.cs);
  }
  f.H = __shfl(f.H, 0, T);  // (every lane of the wavefront is still here)
  f.cs = __shfl(f.cs, 0, T);
  f.sn = __shfl(f.sn, 0, T);
  if (!agent) {
    // no observation in this pass: flags 0, the rows untouched (reset pass: a vehicle that ended in this tick keeps
    // the tick's rows)
    if (r == 0 && in_range && (!groups || (flags & SMX_F_ALIVE))) o.ec_flags[gid] = 0;
    return;
  }
  f.px = o.ego_pos[gid * 3];
  f.py = o.ego_pos[gid * 3 + 1];
  f.pz = o.ego_pos[gid * 3 + 2];
  if (r < 4) o.ego_frame[gid * 4 + r] = r == 0 ? f.px : r == 1 ? f.py : r == 2 ? f.pz : f.H;
  // ---- the ego block (adapter :134-144): position and heading are the origin, the linear triples point along x
  const float* ef = o.ego_f32 + gid * SMX_EGO_F32_COUNT;
  for (int k = r; k < SMX_EGO_F32_COUNT; k += T) {
    float v = ef[k];
    if (k == SMX_EGO_HEADING) v = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int base = j == 0 ? SMX_EGO_LIN_VEL : j == 1 ? SMX_EGO_LIN_ACC : SMX_EGO_LIN_JERK;
      if (k == base) {
        const double x = (double)ef[base], y = (double)ef[base + 1];
        v = (float)sqrt(x * x + y * y);  // np.linalg.norm(v[:2])
      } else if (k == base + 1) {
        v = 0.0f;
      }
    }
    o.ec_ego_f32[gid * SMX_EGO_F32_COUNT + k] = v;
  }
  if (c.sensors & SMX_SENSOR_WAYPOINTS) {
    const int P = c.wp_paths, W = c.wp_len;
    const int n_paths = min((int)o.wp_count[gid * (P + 1)], P);
    for (int p = 0; p < n_paths; ++p) {
      const int n = min((int)o.wp_count[gid * (P + 1) + 1 + p], W);
      const size_t row = (gid * P + p) * W;
      ec_points(f, o.wp_pos + row * 3, o.ec_wp_pos + row * 3, n, r, true, nullptr);
      ec_headings(f, o.wp_heading + row, o.ec_wp_heading + row, n, r);
    }
  }
  if (c.sensors & SMX_SENSOR_NEIGHBORS) {
    const int K = c.nb_max, n = min((int)o.nb_count[gid], K);
    ec_points(f, o.nb_pos + gid * K * 3, o.ec_nb_pos + gid * K * 3, n, r, false, nullptr);
    ec_headings(f, o.nb_heading + gid * K, o.ec_nb_heading + gid * K, n, r);
  }
  if (c.sensors & SMX_SENSOR_LIDAR) {
    const size_t row = gid * (size_t)c.lidar_rays;
    ec_points(f, o.lidar_point + row * 3, o.ec_lidar_point + row * 3, c.lidar_rays, r, false, o.lidar_hit + row);
  }
  if (c.sensors & SMX_SENSOR_ROAD_WAYPOINTS) {
    const int L = c.rw_lanes, P = c.rw_paths, R = 2 * c.rw_horizon + 1;
    for (int l = 0; l < L; ++l) {
      const size_t lane_row = gid * (size_t)L + l;
      if (o.rw_lane[lane_row] < 0) continue;  // (uniform in the team)
      const int n_paths = min((int)o.rw_path_count[lane_row], P);
      for (int p = 0; p < n_paths; ++p) {
        const int n = min((int)o.rw_count[lane_row * P + p], R);
        const size_t row = (lane_row * P + p) * (size_t)R;
        ec_points(f, o.rw_pos + row * 3, o.ec_rw_pos + row * 3, n, r, true, nullptr);
        ec_headings(f, o.rw_heading + row, o.ec_rw_heading + row, n, r);
      }
    }
  }
  if (r == 0) o.ec_flags[gid] = 1;
}

// =================================================================================
// k_actions_to_world: the action half of the ego-centric adapters (ego_centric_adapters.py:195-266) — an action buffer
// given in the frame of each agent's last observation (ego_frame / ec_flags of the last pass) rewritten into a second
// buffer of the same layout in world coordinates.  One lane per (agent, point); the lanes of an agent are adjacent in
// the wavefront, the first of them takes cos(-H), sin(-H) and the others read them across lanes.  A lane writes every
// row of its column, converted or copied, so the output is complete whatever the agents sent.
//   to_world(q) = inv(M) q + (px, py, pz) (world_position_from_ego_frame, math.py:490-505; inv(M) = M transposed)
//   heading     = wrap_value(h + H, -pi, pi) (adapter :206-211, :260-262)
// =================================================================================
template <int SPACE>
__global__ void __launch_bounds__(SMX_BLOCK) k_actions_to_world(const double* __restrict__ in, const int32_t* __restrict__ counts,
                                                                double* __restrict__ out, const double* __restrict__ frame,
                                                                const uint8_t* __restrict__ ec_flags, const size_t total,
                                                                const int n_veh, const int n_social, const int cols) {
  // (SMX_ACTION_SPACE_MPC takes the Trajectory instance: both are _trajectory_adapter, ego_centric_adapters.py:316-322)
  constexpr bool POSE = SPACE == SMX_ACTION_SPACE_TARGET_POSE, TIMED = SPACE == SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME;
  constexpr int ROWS = POSE ? 4 : TIMED ? 5 : 4;
  constexpr int RX = TIMED ? 1 : 0;  // rows x, y, heading are RX, RX + 1, RX + 2
  const int t = (int)threadIdx.x;
  const size_t tid = (size_t)blockIdx.x * SMX_BLOCK + t;
  const size_t gid = tid / (size_t)cols;
  const int col = (int)(tid - gid * (size_t)cols);
  const bool valid = gid < total;
  const int leader = max(0, t - col);  // the agent's first lane in this wavefront
  const bool framed = valid && (ec_flags[gid] & 1) && (int)(gid % (size_t)n_veh) < n_veh - n_social;
  double H = 0.0, cs = 1.0, sn = 0.0;
  if (framed && t == leader) {
    H = frame[gid * 4 + 3];
    sincos(-H, &sn, &cs);
  }
  H = __shfl(H, leader);
  cs = __shfl(cs, leader);
  sn = __shfl(sn, leader);
  if (!valid) return;
  // POSE: [E*N][4], one column; else [E*N][ROWS][cols]
  const size_t base = POSE ? gid * 4 : gid * (size_t)ROWS * cols + col, stride = POSE ? 1 : (size_t)cols;
  double v[ROWS];
#pragma unroll
  for (int k = 0; k < ROWS; ++k) v[k] = in[base + k * stride];
  bool convert = framed;
  if (POSE) {
    convert = convert && !(v[0] != v[0]);  // a NaN x: no action this tick
  } else {
    const int n = counts[gid];  // 0: no action this tick
    convert = convert && n > 0 && (TIMED ? col < min(n, cols) : (col < min(n, SMX_TRAJ_COLS - 1) || col == SMX_TRAJ_COLS - 1));
  }
  if (convert) {
    const double qx = v[RX], qy = v[RX + 1];
    v[RX] = (cs * qx + sn * qy) + frame[gid * 4];
    v[RX + 1] = (cs * qy - sn * qx) + frame[gid * 4 + 1];
    v[RX + 2] = wrap_value_pi(v[RX + 2] + H);
  }
#pragma unroll
  for (int k = 0; k < ROWS; ++k) out[base + k * stride] = v[k];
}

// =================================================================================
// k_frame_push / k_frame_dstack (smx_config.frame_stack; include/smx.h smx_bind_frame_stack): FrameStack of
// smarts/env/wrappers/frame_stack.py over (env, slot) rows — per agent the last k frames of every bound row, newest
// first, kept in place in the caller's buffers.  The last launches of a pass: every row is complete, the flags are the
// ones the pass leaves, `done` is this tick's and env_done says which envs restarted inside the launch.  Per agent:
//   smx_reset            FILL when its env is selected (mask / all) and it is an alive agent, else HOLD
//   tick, env restarted  FILL (auto_reset and env_done raised: the rows hold the next episode's first observation)
//   tick, otherwise      PUSH when it was alive at the tick's start — still alive, or done in this tick — else HOLD
// and HOLD for every social slot.  No per-agent state beyond what the pass already keeps.
// A thread owns one column of bytes (16, 4 or 1 wide) at a fixed offset of the agent's row: it loads the k - 1 frames
// that stay and the new one into registers, then stores k — the shift in place has no hazard, a fill is the same thread
// storing its new value k times.  Pure streaming: 16-byte accesses wherever the row's size and both pointers allow.
// =================================================================================
#define SMX_STACK_BLOCK 256
enum { SMX_STACK_HOLD = 0, SMX_STACK_PUSH = 1, SMX_STACK_FILL = 2 };
struct FrameStackBinding {
  const uint8_t* src;  // the row: [total][bytes]
  uint8_t* dst;        // the stack: [total][k][bytes] (FRAMES) / [total][pixels][3k] (DSTACK)
  uint32_t bytes;      // per agent and frame
  uint32_t unit;       // FRAMES: bytes a thread moves per frame (16, 4 or 1), chosen on the host from the alignments
  uint32_t block0;     // FRAMES: the binding's first workgroup of the launch
  uint32_t pad;
};
struct FrameStackArgs {
  FrameStackBinding b[SMX_STACK_MAX_BINDINGS];
  int n;  // bindings of this launch (their workgroups follow one another: block0 ascends)
  int k;  // frames
  uint32_t total, n_veh;
  const int32_t* flags;     // after the pass
  const uint8_t* done;      // out.done of this tick
  const uint8_t* env_done;  // out.env_done
  const uint8_t* env_mask;  // smx_reset's mask (null: every env)
  int is_step, auto_reset;
};

__device__ __forceinline__ int frame_stack_action(const FrameStackArgs& f, const uint32_t agent) {
  const int flags = f.flags[agent];
  if (flags & SMX_F_SOCIAL) return SMX_STACK_HOLD;
  const uint32_t env = agent / f.n_veh;
  const bool alive = (flags & SMX_F_ALIVE) != 0;
  if (!f.is_step) return (alive && (!f.env_mask || f.env_mask[env])) ? SMX_STACK_FILL : SMX_STACK_HOLD;
  if (f.auto_reset && f.env_done[env]) return alive ? SMX_STACK_FILL : SMX_STACK_HOLD;
  return (alive || f.done[agent]) ? SMX_STACK_PUSH : SMX_STACK_HOLD;
}

// thread `t` of a workgroup whose first unit is u0, `per` units an agent: its agent and its unit inside the agent
// (one 64-bit division, uniform in the workgroup; the per-thread one is 32-bit: rem + t < per + SMX_STACK_BLOCK)
__device__ __forceinline__ void frame_stack_split(const uint64_t u0, const uint32_t per, const uint32_t t, uint64_t& agent, uint32_t& col) {
  const uint64_t a0 = u0 / per;
  const uint32_t local = (uint32_t)(u0 - a0 * per) + t, q = local / per;
  agent = a0 + q;
  col = local - q * per;
}

template <typename U>
__device__ __forceinline__ void frame_push_columns(const FrameStackArgs& f, const FrameStackBinding& b, const uint32_t block) {
  const uint32_t per = b.bytes / (uint32_t)sizeof(U);
  uint64_t agent;
  uint32_t col;
  frame_stack_split((uint64_t)block * SMX_STACK_BLOCK, per, threadIdx.x, agent, col);
  if (agent >= f.total) return;
  const int action = frame_stack_action(f, (uint32_t)agent);
  if (action == SMX_STACK_HOLD) return;
  const U fresh = reinterpret_cast<const U*>(b.src + agent * b.bytes)[col];
  U* frame = reinterpret_cast<U*>(b.dst + agent * (uint64_t)f.k * b.bytes) + col;  // frame j: frame[j * per]
  U v[SMX_STACK_MAX_FRAMES];
  v[0] = fresh;
#pragma unroll
  for (int j = 1; j < SMX_STACK_MAX_FRAMES; ++j) {
    v[j] = fresh;
    if (j < f.k && action == SMX_STACK_PUSH) v[j] = frame[(size_t)(j - 1) * per];
  }
#pragma unroll
  for (int j = 0; j < SMX_STACK_MAX_FRAMES; ++j)
    if (j < f.k) frame[(size_t)j * per] = v[j];
}

__global__ void __launch_bounds__(SMX_STACK_BLOCK) k_frame_push(const FrameStackArgs f) {
  int i = 0;  // the binding of this workgroup (uniform)
  while (i + 1 < f.n && blockIdx.x >= f.b[i + 1].block0) ++i;
  const FrameStackBinding& b = f.b[i];
  const uint32_t block = blockIdx.x - b.block0;
  if (b.unit == 16)
    frame_push_columns<uint4>(f, b, block);
  else if (b.unit == 4)
    frame_push_columns<uint32_t>(f, b, block);
  else
    frame_push_columns<uint8_t>(f, b, block);
}

// The interleaved image, [total][pixels][3K] with channel 3j + c = frame j's channel c (np.dstack, rgb_image.py:93-99).
// A thread takes four pixels: 12 source bytes, and the 12K contiguous bytes of the stack they own — three dwords in,
// 3K dwords in and out (16-byte accesses when 12K is a multiple of 16: K = 4, 8).  Pixel p's new 3K bytes are its three
// new bytes followed by the first 3(K - 1) of its old ones; every index below is a constant once the loops unroll.
// An image whose pixel count is no multiple of four takes the byte path, a pixel after the other.
template <int K>
__global__ void __launch_bounds__(SMX_STACK_BLOCK) k_frame_dstack(const FrameStackArgs f) {
  constexpr int NW = 3 * K, PB = 3 * K;  // dwords per thread, bytes per pixel
  const FrameStackBinding& b = f.b[0];
  const uint32_t pixels = b.bytes / 3, groups = (pixels + 3) / 4;
  uint64_t agent;
  uint32_t g;
  frame_stack_split((uint64_t)blockIdx.x * SMX_STACK_BLOCK, groups, threadIdx.x, agent, g);
  if (agent >= f.total) return;
  const int action = frame_stack_action(f, (uint32_t)agent);
  if (action == SMX_STACK_HOLD) return;
  const uint8_t* src = b.src + agent * b.bytes + (size_t)12 * g;
  uint8_t* dst = b.dst + agent * (uint64_t)K * b.bytes + (size_t)4 * PB * g;
  if ((pixels & 3u) != 0) {  // (uniform over the launch)
    const int n = (int)min(4u, pixels - 4 * g);
    for (int p = 0; p < n; ++p)
      for (int c = 0; c < 3; ++c) {
        const uint8_t fresh = src[3 * p + c];
        uint8_t* px = dst + p * PB + c;
        for (int j = K - 1; j >= 1; --j) px[3 * j] = action == SMX_STACK_PUSH ? px[3 * (j - 1)] : fresh;
        px[0] = fresh;
      }
    return;
  }
  uint32_t nw[3], ow[NW], out[NW];
#pragma unroll
  for (int w = 0; w < 3; ++w) nw[w] = reinterpret_cast<const uint32_t*>(src)[w];
  if (action == SMX_STACK_PUSH) {
    if constexpr (NW % 4 == 0) {
#pragma unroll
      for (int q = 0; q < NW / 4; ++q) {
        const uint4 v = reinterpret_cast<const uint4*>(dst)[q];
        ow[4 * q] = v.x, ow[4 * q + 1] = v.y, ow[4 * q + 2] = v.z, ow[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int w = 0; w < NW; ++w) ow[w] = reinterpret_cast<const uint32_t*>(dst)[w];
    }
  } else {
#pragma unroll
    for (int w = 0; w < NW; ++w) ow[w] = 0u;
  }
  const bool push = action == SMX_STACK_PUSH;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    uint32_t word = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * w + q, p = i / PB, r = i % PB;  // byte i: pixel p, channel r of its 3K
      const int ni = 3 * p + r % 3;                     // the new byte of that colour
      const int oi = p * PB + (r >= 3 ? r - 3 : 0);     // the old byte that moves here (r >= 3)
      const uint32_t fresh = (nw[ni >> 2] >> (8 * (ni & 3))) & 255u;
      const uint32_t old = (ow[oi >> 2] >> (8 * (oi & 3))) & 255u;
      word |= ((r < 3 || !push) ? fresh : old) << (8 * q);
    }
    out[w] = word;
  }
  if constexpr (NW % 4 == 0) {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) reinterpret_cast<uint4*>(dst)[q] = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
  } else {
#pragma unroll
    for (int w = 0; w < NW; ++w) reinterpret_cast<uint32_t*>(dst)[w] = out[w];
  }
}

// =================================================================================
// k_tail: the end of every pass, one wavefront per env group (those of the observe role), in one launch:
//  - the tick's commit (commit_role: teardown, done counts, auto-reset respawn);
//  - the OGM / DAGM / RGB tiles of the group's new vehicles (respawned just now, or by k_reset), one after the other — almost
//    no group has any, and a group looks at its flags with one load and a ballot;
//  - the env groups with new vehicles, listed for k_first (the reset pass), one atomic per such group;
//  - large batches: the next tick's alive list (seg_position), built here instead of by a k_alive_list launch at the
//    head of that tick.  The reset pass does not change SMX_F_ALIVE (a new vehicle is never done on its first
//    observation), so the flags are final here; the next tick's list counter, slow-list counters and reset-group
//    counter are zeroed by workgroup 0.
// (k_first stays a launch of its own: its 512 threads at 256 registers run one workgroup per CU, and the commit of
// every group would wait behind that occupancy — round 2 measured the commit inside the reset pass: no gain)
// =================================================================================
struct TailArgs {
  int commit;              // the tick's commit (0: smx_reset, which has no tick)
  int grids;               // OGM / DAGM / RGB tiles of the new vehicles
  int32_t* groups;         // env groups with new vehicles (for k_first)
  int32_t* n_groups;
  int32_t* n_groups_next;  // zeroed: the next pass's counter
  int32_t* list;           // the next tick's alive list (null: not built here)
  int32_t* seg_count;      // its eight counters, SMX_SEG_STRIDE apart
  int32_t* seg_next;       // zeroed: the eight counters the list after it is built with
  int32_t* flat_next;      // zeroed: k_alive_list's counter of the next tick (should that tick build its list itself)
  int32_t* slow_next;      // zeroed: the next tick's four slow-list counters
};

template <bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_tail(const KernelArgs a, const TailArgs t) {
  const smx_config& c = a.cfg;
  const int block = (int)blockIdx.x;
  const int n_veh = c.num_vehicles;
  const int epb = SMX_BLOCK / n_veh;
  const size_t total = (size_t)c.num_envs * n_veh;
  const size_t g0 = (size_t)block * epb * n_veh;
  const size_t g1 = min(total, g0 + (size_t)epb * n_veh);
  const int lane = (int)threadIdx.x;
  const size_t gid = g0 + lane;
  if (t.commit) commit_role<GUARD>(a, block, true);  // (lane l commits vehicle g0 + l: its flags word is read back below)
  if (block == 0 && lane == 0) {
    *t.n_groups_next = 0;
    if (t.list) {
      for (int k = 0; k < 8; ++k) t.seg_next[SMX_SEG_STRIDE * k] = 0;
      *t.flat_next = 0;
      for (int k = 0; k < 4; ++k) t.slow_next[k] = 0;
    }
  }
  const int f = gid < g1 ? a.st.flags[gid] : 0;
  const bool alive = (f & SMX_F_ALIVE) != 0;
  if (__ballot(alive && (f & SMX_F_FIRST)) != 0ull) {  // (uniform)
    if (lane == 0) t.groups[atomicAdd(t.n_groups, 1)] = block;
    if (t.grids) {
      unsigned long long fresh = __ballot(alive && (f & SMX_F_FIRST) && !(f & SMX_F_SOCIAL));
      while (fresh != 0ull) {
        const int j = __ffsll((long long)fresh) - 1;
        fresh &= fresh - 1ull;
        if (c.sensors & SMX_SENSOR_OGM) {
          ogm_role(a, (int)(g0 + j));
          __syncthreads();  // the tile is reused
        }
        if (c.sensors & SMX_SENSOR_DAGM) {
          dagm_role(a, (int)(g0 + j));
          __syncthreads();
        }
        if (c.sensors & SMX_SENSOR_RGB) {
          rgb_role(a, (int)(g0 + j));
          __syncthreads();
        }
      }
    }
  }
  if (t.list) {
    // the group's vehicles lie in at most two segments (of 64 vehicles: one)
    const size_t s0 = (g0 >> 6) & 7;
    const size_t seg = (gid >> 6) & 7;
    const unsigned long long m0 = __ballot(alive && seg == s0), m1 = __ballot(alive && seg != s0);
    int b0 = 0, b1 = 0;
    if (lane == 0) {
      if (m0) b0 = atomicAdd(t.seg_count + SMX_SEG_STRIDE * s0, __popcll(m0));
      if (m1) b1 = atomicAdd(t.seg_count + SMX_SEG_STRIDE * (((g1 - 1) >> 6) & 7), __popcll(m1));
    }
    b0 = __shfl(b0, 0);
    b1 = __shfl(b1, 0);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (alive) {
      const bool first_seg = seg == s0;
      const size_t off = (size_t)(first_seg ? b0 : b1) + __popcll((first_seg ? m0 : m1) & below);
      t.list[seg_position(seg, off)] = (int32_t)gid;
    }
  }
}
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints(const KernelArgs a) { waypoints_role(a, (int)blockIdx.x); }
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_tables(const KernelArgs a) { waypoints_tables_role(a, (int)blockIdx.x); }
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_emit(const KernelArgs a) {
  SMX_TSTAMP(span0);
  waypoints_emit_role(a, (int)blockIdx.x);
  SMX_TSTAMP(span1);
  SMX_TSPAN(4, span0, span1);
}
// the vehicles k_waypoints_emit left on the slow list: waypoints_for (a team of four lanes per vehicle), a fixed grid
// striding the list, whose length is only known on the device
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_listed(const KernelArgs a) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  const int count = *a.slow_count;
  constexpr int VPB = SMX_BLOCK / SMX_WP_LANES;
  for (int i = (int)blockIdx.x * VPB + (int)threadIdx.x / SMX_WP_LANES; i < count; i += (int)gridDim.x * VPB)
    waypoints_for<SMX_BLOCK>(a, (size_t)a.slow_list[i], knot_scratch + threadIdx.x);
}
// the slow chain's form (short lists: its latency ends the chain): eight lanes a vehicle — four emit the rows
// (waypoints_for), four walk the knot lists for the next tick's controller (k_wp_walk_listed's work) beside them
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_walk_listed(const KernelArgs a) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  const int count = *a.slow_count;
  constexpr int VPB = SMX_BLOCK / (2 * SMX_WP_LANES);
  const bool walker = ((threadIdx.x / SMX_WP_LANES) & 1) != 0;  // (uniform in an aligned group of four lanes)
  for (int i = (int)blockIdx.x * VPB + (int)threadIdx.x / (2 * SMX_WP_LANES); i < count; i += (int)gridDim.x * VPB) {
    const size_t gid = (size_t)a.slow_list[i];
    if (walker)
      wp_walk_for(a, gid, (int)threadIdx.x % SMX_WP_LANES, false);
    else
      waypoints_for<SMX_BLOCK>(a, gid, knot_scratch + threadIdx.x);
  }
}
// (capped at 168 registers for a third wavefront per SIMD beside the waypoint kernels it spills 52 of them: 0.796 -> 0.806 ms)
__global__ void __launch_bounds__(SMX_BLOCK) k_observe(const KernelArgs a) {
  SMX_TSTAMP(span0);
  observe_role(a, (int)blockIdx.x, false);
  SMX_TSTAMP(span1);
  SMX_TSPAN(5, span0, span1);
}
// (... with a triple block bound, TickPlan::sized)
__global__ void __launch_bounds__(SMX_BLOCK) k_observe_sized(const KernelArgs a) {
  SMX_TSTAMP(span0);
  observe_role(a, (int)blockIdx.x, true);
  SMX_TSTAMP(span1);
  SMX_TSPAN(5, span0, span1);
}

// =================================================================================
// k_reset: SMARTS.reset (smarts.py:365-460) for the selected envs — vehicles re-created at their
// spawn poses (AckermannChassis._initialize_speed, chassis.py:668-671); the observation kernels
// that follow produce their first observations.
// =================================================================================
// (SIZED: a triple block is bound, TickPlan::sized — the agents' triples are written beside their spawn poses; ENTRY: an
// entry table is bound, TickPlan::entry — agents whose ready tick is not 0 are created pending)
template <bool GUARD = false, bool SIZED = false, bool ENTRY = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_reset(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  if (gid >= total) return;
  const int env = (int)(gid / c.num_vehicles);
  const int slot = (int)(gid - (size_t)env * c.num_vehicles);
  bool sel;
  if (a.reset_all)
    sel = true;
  else if (a.env_mask)
    sel = a.env_mask[env] != 0;
  else
    sel = a.st.env_reset_pending[env] != 0;
  if (!sel) {
    if constexpr (GUARD) a.guard[gid] = 0;  // (an agent absent from the pass)
    return;
  }
  respawn_vehicle<GUARD, SIZED ? 1 : 0, ENTRY ? 1 : 0>(a, gid, total, a.st.env_episode[env] + 1);  // every reset starts the next spawn row
  // per-env words are written by every thread of the env with the same values (no ordering needed
  // inside this kernel; the env's own threads never read them here)
  (void)slot;
}

// per-env bookkeeping of a reset, after k_reset (separate launch: k_reset's threads read env_episode)
__global__ void __launch_bounds__(SMX_BLOCK) k_reset_env(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const int env = blockIdx.x * SMX_BLOCK + threadIdx.x;
  if (env >= c.num_envs) return;
  bool sel;
  if (a.reset_all)
    sel = true;
  else if (a.env_mask)
    sel = a.env_mask[env] != 0;
  else
    sel = a.st.env_reset_pending[env] != 0;
  if (!sel) return;
  a.st.env_episode[env] = a.st.env_episode[env] + 1;
  a.st.env_done_count[env] = __builtin_expect(a.history.follow != nullptr, 0) ? history_agents_absent(a, env) : 0;
  a.st.env_ticks[env] = c.reset_elapsed_steps;
  a.st.env_reset_pending[env] = 0;
  if (!a.keep_reward_done) a.out.env_done[env] = 0;
}

// =================================================================================
// C-ABI (include/smx.h)
// =================================================================================
extern "C" const char* smx_version(void) { return "smarts-mi355x 0.2 (gfx950)"; }

#ifdef SMX_DEBUG_TIMING
extern "C" int smx_span_read(unsigned int* out) {  // developer: [kernel][wavefront] spans of the last launches, 10 ns units
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(smx_span), sizeof(unsigned int) * SMX_SPAN_KERNELS * SMX_SPAN_WAVES) != hipSuccess) return -2;
  return 0;
}

extern "C" int smx_prof_read(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(smx_prof), 128 * sizeof(unsigned long long)) != hipSuccess) return -2;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(smx_prof), z, sizeof(z)) != hipSuccess) return -2;
  }
  return 0;
}
#endif
#ifdef SMX_DEBUG_BOUNDS
extern "C" int smx_debug_read(int* site, long long* value) {
  if (hipMemcpyFromSymbol(site, HIP_SYMBOL(smx_dbg_site), sizeof(int)) != hipSuccess) return -2;
  if (hipMemcpyFromSymbol(value, HIP_SYMBOL(smx_dbg_value), sizeof(long long)) != hipSuccess) return -2;
  int aux[8];
  if (hipMemcpyFromSymbol(aux, HIP_SYMBOL(smx_dbg_aux), sizeof(aux)) != hipSuccess) return -2;
  double f[64];
  if (hipMemcpyFromSymbol(f, HIP_SYMBOL(smx_dbg_f), sizeof(f)) != hipSuccess) return -2;
  printf("dbg ctrl: wp_n=%g la_num=%g lax=%.6f lay=%.6f lah=%.6f n_paths=%g want=%g curv=%g\n", f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]);
  for (int k = 0; k < 17; ++k) printf("  wp%d %.6f %.6f %.6f\n", k, f[8 + 3 * k], f[9 + 3 * k], f[10 + 3 * k]);
  printf("dbg aux: first=%d remaining=%d hops=%d n_next=%d lane=%d next0=%d cur_idx=%d mem_next0=%d\n", aux[0], aux[1], aux[2], aux[3], aux[4], aux[5], aux[6], aux[7]);
  return 0;
}
#endif

extern "C" uint64_t smx_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(smx_config);
    case 1: return sizeof(smx_map_tables);
    case 2: return sizeof(smx_state);
    case 3: return sizeof(smx_spawns);
    case 4: return sizeof(smx_outputs);
    default: return 0;
  }
}

// the constants smx_host.h decides with are the device side's
static_assert(SMX_HOST_BLOCK == SMX_BLOCK && SMX_HOST_WP_LANES == SMX_WP_LANES && SMX_HOST_MAX_KNOTS == SMX_MAX_KNOTS &&
                  SMX_HOST_SLOW_BLOCKS == SMX_SLOW_BLOCKS && SMX_HOST_STACK_BLOCK == SMX_STACK_BLOCK,
              "smx_host.h mirrors these");

// the map's knot table, for load_map_impl (smx_handle.h)
// The agents' triples of one triple block into another (smx_handle.h build_dims_blob: the block moves when the social
// table beside it is bound or dropped while smx_set_agent_dims' table stays), then a synchronisation.
__global__ void __launch_bounds__(SMX_BLOCK) k_copy_agent_dims(const double* from, double* to, int n_veh, int n_agents, size_t total) {
  const size_t g = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  if (g >= total || (int)(g % (size_t)n_veh) >= n_agents) return;
  for (int q = 0; q < 3; ++q) to[g * 3 + q] = from[g * 3 + q];
}
static int copy_agent_dims(smx_handle h, const double* from, double* to) {
  const size_t total = (size_t)h->cfg.num_envs * (size_t)h->cfg.num_vehicles;
  hipLaunchKernelGGL(k_copy_agent_dims, dim3((unsigned)((total + SMX_BLOCK - 1) / SMX_BLOCK)), dim3(SMX_BLOCK), 0, 0, from, to,
                     h->cfg.num_vehicles, h->cfg.num_vehicles - h->cfg.num_social, total);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}

static int build_knot_table(smx_handle h, KnotRow* table) {
  hipLaunchKernelGGL(k_knot_table, dim3(smx_blocks((size_t)h->map.n_lanepoints)), dim3(SMX_BLOCK), 0, 0, h->map, (int)h->cfg.wp_lookahead,
                     table, h->knot_stats.get<int32_t>());
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}

extern "C" int smx_create(const smx_config* cfg, int device, smx_handle* out) {
  const int rc = create_impl(cfg, device, out, KernelSide{SMX_WPE_POOL, SMX_WPE_SPILL_GROUP_BYTES, SMX_SIDE_PRIO, build_knot_table, copy_agent_dims});
#ifdef SMX_DEBUG_TIMING
  if (const char* dbg = getenv("SMX_DEBUG_SKIP"))
    if (rc == SMX_OK) (*out)->debug_skip = atoi(dbg);
#endif
  return rc;
}

extern "C" int smx_set_launch_strategy(smx_handle h, int strategy) {
  if (!h) return SMX_ERR_INVALID;
  if (strategy < SMX_LAUNCH_AUTO || strategy > SMX_LAUNCH_LARGE_TEAMS) return fail(h, SMX_ERR_INVALID, "unknown launch strategy");
  h->launch_strategy = strategy;
  return SMX_OK;
}

// What a call's plan (smx_plan.h) may depend on, read off the handle.  `st`: the caller's state block, for the carried
// alive list (null: no tick is planned, only the form is asked for).
// `follow`: the call is smx_step_history_agents; `handover`: smx_step_history_handover; `mixed`: smx_step_mixed.
static PlanInputs plan_inputs(const smx_handle_s* h, bool is_step, const smx_state* st, bool follow = false, bool handover = false,
                              bool mixed = false) {
  PlanInputs in{};
  in.cfg = &h->cfg;
  in.launch_strategy = h->launch_strategy;
  in.map_junctions = h->map_junctions;
  in.slow_blocks = h->slow_blocks;
  in.routed = h->missions.route_last != nullptr;
  in.is_step = is_step;
  in.phase_timing = h->phase_timing && h->ph_used < 16384;
  in.side_ready = h->streams.ready;
  in.list_carried = st && h->list_ready && std::memcmp(&h->list_state, st, sizeof(smx_state)) == 0;
  in.debug_skip = (SMX_SKIP(*h, SMX_SKIP_FORCE_SMALL) ? SMX_SKIP_FORCE_SMALL : 0) |
                  (SMX_SKIP(*h, SMX_SKIP_FORCE_SCAN_SPLIT) ? SMX_SKIP_FORCE_SCAN_SPLIT : 0);
  in.alive_blob = (bool)h->alive_blob;
  in.knots_blob = (bool)h->knots_blob;
  in.knot_table = h->knot_table && h->knot_table_mode != 0;
  in.ctrl_blob = (bool)h->ctrl_blob;
  in.pending_blob = h->pending_blob.get<uint8_t>();
  in.slow = SlowLists{h->slow_blob.get<int32_t>(), (size_t)h->cfg.num_envs * h->cfg.num_vehicles};
  in.slow_parity = h->alive_parity;
  in.frame_stack_bound = !h->stacks.empty();
  in.guard_bound = h->guard_out != nullptr;
  in.dims_bound = h->dims.table != nullptr;
  in.agent_dims_bound = h->dims.agent != nullptr;
  in.history_bound = h->history.vehicle != nullptr;
  in.follow_entry = follow;
  in.ogm_mask = h->ogm_mask && h->ogm_delta;
  in.handover_entry = handover;
  in.bubbles_bound = h->bubble_state != nullptr;
  in.entry_bound = h->entry.ready != nullptr;
  in.agent_spaces = h->spaces.space != nullptr ? h->spaces.mask : 0u;
  in.mixed_entry = mixed;
  return in;
}

extern "C" int smx_launch_form(smx_handle h) {
  if (!h) return SMX_ERR_INVALID;
  if (!h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_launch_form needs the map (the form depends on it)");
  return tick_plan(plan_inputs(h, false, nullptr)).form;
}

extern "C" int smx_set_controller_gains(smx_handle h, double heading_gain, double lateral_gain) {
  if (!h) return SMX_ERR_INVALID;
  h->heading_gain_pos = heading_gain;
  h->lateral_gain_pos = lateral_gain;
  return SMX_OK;
}

extern "C" int smx_load_map(smx_handle h, const smx_map_tables* t) { return load_map_impl(h, t); }

extern "C" int smx_set_vias(smx_handle h, const smx_via* vias_host, int32_t n, const int32_t* slot_off_host) {
  return set_vias_impl(h, vias_host, n, slot_off_host);
}

extern "C" int smx_set_missions(smx_handle h, const smx_mission* missions_host, int32_t n_slots,
                                const int32_t* route_roads_host, int32_t n_route_roads) {
  return set_missions_impl(h, missions_host, n_slots, route_roads_host, n_route_roads);
}

extern "C" int smx_check_mission_goals(const smx_mission_goal* goals, int32_t n_slots, int32_t num_vehicles,
                                       const double* lane_end_heading, const int32_t* lane_dead_end, int32_t n_lanes,
                                       int32_t map_lanes, char* err, uint64_t err_len) {
  const std::string msg = mission_goals_error(goals, n_slots, num_vehicles, lane_end_heading, lane_dead_end, n_lanes, map_lanes);
  return report(msg.empty() ? SMX_OK : SMX_ERR_INVALID, msg, err, err_len);
}

extern "C" int smx_set_mission_goals(smx_handle h, const smx_mission_goal* goals_host, int32_t n_slots,
                                     const double* lane_end_heading_host, const int32_t* lane_dead_end_host, int32_t n_lanes) {
  return set_mission_goals_impl(h, goals_host, n_slots, lane_end_heading_host, lane_dead_end_host, n_lanes);
}

extern "C" int smx_set_lidar_rays(smx_handle h, const double* rays_dev, int32_t n_rays) { return set_lidar_rays_impl(h, rays_dev, n_rays); }

// ---- the smx_check_* entry points: smx_host.h's checks, callable without a device or a handle ----
extern "C" int smx_check_buffers(const smx_config* cfg, int has_vias, const smx_state* st, const smx_spawns* sp,
                                 const smx_outputs* out, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = cfg ? check_buffers_impl(*cfg, has_vias != 0, st, sp, out, msg) : refuse(msg, "null config");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_check_rgb_output(const smx_config* cfg, uint64_t count, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = cfg ? check_rgb_output_impl(*cfg, count, msg) : refuse(msg, "null config");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_check_guard(const smx_config* cfg, uint64_t count, double margin, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = cfg ? check_guard_impl(*cfg, count, margin, msg) : refuse(msg, "null config");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_check_frame_stack(const smx_config* cfg, int32_t source, int32_t layout, uint64_t bytes, char* err, uint64_t err_len) {
  std::string msg;
  uint64_t row;
  const int rc = cfg ? check_frame_stack_impl(*cfg, source, layout, bytes, row, msg) : refuse(msg, "null config");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_rgb_output(smx_handle h, uint8_t* rgb_dev, uint64_t count) { return set_rgb_output_impl(h, rgb_dev, count); }

extern "C" int smx_set_guard(smx_handle h, uint8_t* guard_dev, uint64_t count, double margin) {
  return set_guard_impl(h, guard_dev, count, margin);
}

extern "C" int smx_check_social_history(const smx_config* cfg, const smx_map_tables* map, const smx_social_history* hist, char* err,
                                        uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && map && hist) ? check_social_history_impl(*cfg, *map, *hist, msg) : refuse(msg, "null config / map / history");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_social_history(smx_handle h, const smx_social_history* hist) { return set_social_history_impl(h, hist); }

extern "C" int smx_check_social_history_dims(const smx_config* cfg, const smx_social_history* hist, const smx_social_dims* dims,
                                             char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && hist && dims) ? check_social_history_dims_impl(*cfg, *hist, *dims, msg) : refuse(msg, "null config / history / dims");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_social_history_dims(smx_handle h, const smx_social_dims* dims) { return set_social_history_dims_impl(h, dims); }

extern "C" int smx_check_agent_dims(const smx_config* cfg, const smx_agent_dims* dims, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && dims) ? check_agent_dims_impl(*cfg, *dims, msg) : refuse(msg, "null config / dims");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_agent_dims(smx_handle h, const smx_agent_dims* dims) { return set_agent_dims_impl(h, dims); }

extern "C" int smx_check_agent_entry(const smx_config* cfg, const smx_agent_entry* entry, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && entry) ? check_agent_entry_impl(*cfg, *entry, msg) : refuse(msg, "null config / entry");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_agent_entry(smx_handle h, const smx_agent_entry* entry) { return set_agent_entry_impl(h, entry); }

extern "C" int smx_check_agent_spaces(const smx_config* cfg, const smx_agent_spaces* spaces, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && spaces) ? check_agent_spaces_impl(*cfg, *spaces, msg) : refuse(msg, "agent spaces: null config / table");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_agent_spaces(smx_handle h, const smx_agent_spaces* spaces) { return set_agent_spaces_impl(h, spaces); }

extern "C" int smx_check_history_agents(const smx_config* cfg, const smx_social_history* hist, const smx_history_agents* ha, char* err,
                                        uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && hist && ha) ? check_history_agents_impl(*cfg, hist->rows, *ha, msg) : refuse(msg, "null config / history / history agents");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_history_agents(smx_handle h, const smx_history_agents* ha) { return set_history_agents_impl(h, ha); }

extern "C" int smx_check_history_handover(const smx_config* cfg, const smx_social_history* hist, const smx_history_handover* ho, char* err,
                                          uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && hist && ho) ? check_history_handover_impl(*cfg, hist->rows, *ho, msg) : refuse(msg, "null config / history / history handover");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_history_handover(smx_handle h, const smx_history_handover* ho) { return set_history_handover_impl(h, ho); }

extern "C" int smx_check_history_bubbles(const smx_config* cfg, const smx_history_bubbles* hb, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && hb) ? check_history_bubbles_impl(*cfg, *hb, msg) : refuse(msg, "null config / history bubbles");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_history_bubbles(smx_handle h, const smx_history_bubbles* hb) { return set_history_bubbles_impl(h, hb); }

extern "C" int smx_bind_frame_stack(smx_handle h, int32_t source, int32_t layout, void* stack_dev, uint64_t bytes) {
  return bind_frame_stack_impl(h, source, layout, stack_dev, bytes);
}

// the pass's last launches: every FRAMES binding in one k_frame_push, the interleaved image in one k_frame_dstack
static int launch_frame_stacks(smx_handle h, const bool is_step, const uint8_t* mask, const smx_state* st, const smx_outputs* out,
                               hipStream_t stream) {
  const smx_config& c = h->cfg;
  FrameStackArgs f{};
  f.k = c.frame_stack;
  f.total = (uint32_t)((size_t)c.num_envs * c.num_vehicles);
  f.n_veh = (uint32_t)c.num_vehicles;
  f.flags = st->flags;
  f.done = out->done;
  f.env_done = out->env_done;
  f.env_mask = is_step ? nullptr : mask;
  f.is_step = is_step ? 1 : 0;
  f.auto_reset = c.auto_reset ? 1 : 0;
  FrameStackArgs d = f;
  uint64_t blocks = 0, dstack_blocks = 0;
  for (const smx_handle_s::StackBinding& s : h->stacks) {
    const uint8_t* src = s.source == SMX_STACK_SOURCE_RGB ? h->rgb_out : (const uint8_t*)buffer_ptr(*out, s.source);
    if (!src || !s.row)
      return fail(h, SMX_ERR_STATE, "frame stack: source " + std::to_string(s.source) + " is bound but its row is NULL in this call");
    FrameStackBinding b{src, s.dst, s.row, 0, 0, 0};
    if (s.layout == SMX_STACK_DSTACK) {
      d.b[0] = b;
      d.n = 1;
      dstack_blocks = stack_dstack_blocks(s.row, f.total);
      continue;
    }
    const StackColumns at = stack_push_place(s.row, reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(s.dst), f.total, blocks);
    b.unit = at.unit;
    b.block0 = at.block0;
    f.b[f.n++] = b;
  }
  if (blocks >= STACK_BLOCKS_CAP || dstack_blocks >= STACK_BLOCKS_CAP) return fail(h, SMX_ERR_INVALID, "frame stack: the bound rows need more workgroups than a launch has");
  if (f.n) hipLaunchKernelGGL(k_frame_push, dim3((unsigned)blocks), dim3(SMX_STACK_BLOCK), 0, stream, f);
  if (d.n) {
    void (*const dstack[])(FrameStackArgs) = {k_frame_dstack<2>, k_frame_dstack<3>, k_frame_dstack<4>, k_frame_dstack<5>,
                                              k_frame_dstack<6>, k_frame_dstack<7>, k_frame_dstack<8>};
    hipLaunchKernelGGL(dstack[c.frame_stack - 2], dim3((unsigned)dstack_blocks), dim3(SMX_STACK_BLOCK), 0, stream, d);
  }
  return SMX_OK;
}

static int check_buffers(smx_handle h, const smx_state* st, const smx_spawns* sp, const smx_outputs* o) {
  std::string msg;
  const int rc = check_buffers_impl(h->cfg, h->n_vias > 0, st, sp, o, msg);
  if (rc != SMX_OK) return fail(h, rc, msg);
  if ((h->cfg.sensors & SMX_SENSOR_LIDAR) && !h->lidar_rays)
    return fail(h, SMX_ERR_STATE, "lidar sensor enabled but smx_set_lidar_rays has not been called");
  if ((h->cfg.sensors & SMX_SENSOR_RGB) && !h->rgb_out)
    return fail(h, SMX_ERR_STATE, "rgb sensor enabled but no image buffer is bound (smx_set_rgb_output)");
  for (const smx_handle_s::StackBinding& s : h->stacks)  // (an optional row the caller left NULL: nothing is launched)
    if (s.source != SMX_STACK_SOURCE_RGB && !buffer_ptr(*o, s.source))
      return fail(h, SMX_ERR_STATE, "frame stack: source " + std::to_string(s.source) + " is bound but its row is NULL in smx_outputs");
  return SMX_OK;
}

// enqueue() issues a call's TickPlan (smx_plan.h) step by step; the steps launch what the plan names and decide nothing.
using Kernel = void (*)(KernelArgs);
using HandoffKernel = void (*)(KernelArgs, CtrlHandoff);
static void launch(Kernel k, unsigned blocks, size_t lds, hipStream_t s, const KernelArgs& a) {
  hipLaunchKernelGGL(k, dim3(blocks), dim3(SMX_BLOCK), lds, s, a);
}
static void launch(HandoffKernel k, unsigned blocks, hipStream_t s, const KernelArgs& a, const CtrlHandoff& ho) {
  hipLaunchKernelGGL(k, dim3(blocks), dim3(SMX_BLOCK), 0, s, a, ho);
}
static KernelArgs with_slow(KernelArgs a, const SlowRef& slow) {
  a.slow_list = slow.list;
  a.slow_count = slow.count;
  return a;
}

// the controller kernels of one action space (the lane-following forms exist for the two lane spaces only)
struct ControlKernels {
  Kernel one, one_lds, fast;
  HandoffKernel listed, paths, law;
  Kernel kinematic;  // (the kinematic spaces have this one alone)
};
template <int SPACE, bool GUARD>
static ControlKernels control_kernels_of() {
  if constexpr (smx_kinematic_space(SPACE)) {
    return ControlKernels{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, k_control_kinematic<SPACE, GUARD>};
  } else {
    ControlKernels k{k_control<SPACE, false, GUARD>, nullptr, nullptr, nullptr, nullptr, k_control_law<SPACE, GUARD>, nullptr};
    if constexpr (SPACE == SMX_ACTION_SPACE_LANE || SPACE == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED) {
      k.one_lds = k_control<SPACE, true, GUARD>;
      k.fast = k_control_fast<SPACE, GUARD>;
      k.listed = k_control_listed<SPACE, GUARD>;
      k.paths = k_control_paths<SPACE, GUARD>;
    }
    return k;
  }
}
// (`guard`: TickPlan::guard — the instantiations with the state guard)
template <bool GUARD>
static ControlKernels control_kernels(int action_space) {
  switch (action_space) {
    case SMX_ACTION_SPACE_LANE: return control_kernels_of<SMX_ACTION_SPACE_LANE, GUARD>();
    case SMX_ACTION_SPACE_CONTINUOUS: return control_kernels_of<SMX_ACTION_SPACE_CONTINUOUS, GUARD>();
    case SMX_ACTION_SPACE_ACTUATOR_DYNAMIC: return control_kernels_of<SMX_ACTION_SPACE_ACTUATOR_DYNAMIC, GUARD>();
    case SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED: return control_kernels_of<SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED, GUARD>();
    case SMX_ACTION_SPACE_TRAJECTORY: return control_kernels_of<SMX_ACTION_SPACE_TRAJECTORY, GUARD>();
    case SMX_ACTION_SPACE_MPC: return control_kernels_of<SMX_ACTION_SPACE_MPC, GUARD>();
    case SMX_ACTION_SPACE_TARGET_POSE: return control_kernels_of<SMX_ACTION_SPACE_TARGET_POSE, GUARD>();
    case SMX_ACTION_SPACE_IMITATION: return control_kernels_of<SMX_ACTION_SPACE_IMITATION, GUARD>();
    default: return control_kernels_of<SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME, GUARD>();
  }
}

// the controller kernels of one action space in a mixed fleet (smx_step_mixed; the six spaces of the Ackermann chassis)
using SlotKernel = void (*)(KernelArgs, SlotList);
using MixedKernel = void (*)(KernelArgs, CtrlHandoff, const int32_t*);
struct MixedKernels {
  SlotKernel one;
  MixedKernel paths, law;  // (paths: the two lane spaces only)
};
template <int SPACE, bool GUARD>
static MixedKernels mixed_kernels_of() {
  MixedKernels k{k_control_slots<SPACE, GUARD>, nullptr, k_control_law_mixed<SPACE, GUARD>};
  if constexpr (SPACE == SMX_ACTION_SPACE_LANE || SPACE == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED)
    k.paths = k_control_paths_mixed<SPACE, GUARD>;
  return k;
}
template <bool GUARD>
static MixedKernels mixed_kernels(int action_space) {
  switch (action_space) {
    case SMX_ACTION_SPACE_LANE: return mixed_kernels_of<SMX_ACTION_SPACE_LANE, GUARD>();
    case SMX_ACTION_SPACE_CONTINUOUS: return mixed_kernels_of<SMX_ACTION_SPACE_CONTINUOUS, GUARD>();
    case SMX_ACTION_SPACE_ACTUATOR_DYNAMIC: return mixed_kernels_of<SMX_ACTION_SPACE_ACTUATOR_DYNAMIC, GUARD>();
    case SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED: return mixed_kernels_of<SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED, GUARD>();
    case SMX_ACTION_SPACE_TRAJECTORY: return mixed_kernels_of<SMX_ACTION_SPACE_TRAJECTORY, GUARD>();
    default: return mixed_kernels_of<SMX_ACTION_SPACE_MPC, GUARD>();
  }
}
// One launch, or pair of launches, per space present, all on the caller's stream; they touch disjoint vehicles, so their
// order is free (ascending space numbers here).
static void launch_control_mixed(smx_handle h, const TickPlan& p, const KernelArgs& a, hipStream_t stream) {
  const AgentSpacesDev& sd = h->spaces;
  for (int s = 0; s <= SMX_ACTION_SPACE_IMITATION; ++s) {
    if (!((p.mixed_spaces >> s) & 1u)) continue;
    const MixedKernels k = p.guard ? mixed_kernels<true>(s) : mixed_kernels<false>(s);
    switch (p.control_of[s]) {
      case Control::ONE: {
        const SlotList sl{sd.slots + (size_t)s * h->cfg.num_vehicles, sd.count[s]};
        const unsigned blocks = smx_blocks((size_t)h->cfg.num_envs * sd.count[s], SMX_BLOCK / SMX_WP_LANES);
        hipLaunchKernelGGL(k.one, dim3(blocks), dim3(SMX_BLOCK), 0, stream, a, sl);
        break;
      }
      case Control::PATHS_LAW:
        hipLaunchKernelGGL(k.paths, dim3(p.wp_blocks), dim3(SMX_BLOCK), 0, stream, a, h->ctrl, sd.space);
        hipLaunchKernelGGL(k.law, dim3(p.veh_blocks), dim3(SMX_BLOCK), 0, stream, a, h->ctrl, sd.space);
        break;
      case Control::LAW: hipLaunchKernelGGL(k.law, dim3(p.veh_blocks), dim3(SMX_BLOCK), 0, stream, a, h->ctrl, sd.space); break;
      default: break;
    }
  }
}

// what k_bubbles / k_bubbles_clear get of a call (only built with bubbles bound)
static BubbleArgs bubble_args(const smx_handle_s* h, const KernelArgs& a) {
  BubbleArgs g{};
  g.flags = a.st.flags;
  g.f64 = a.st.f64;
  g.env_ticks = a.st.env_ticks;
  g.env_episode = a.st.env_episode;
  g.history = h->history;
  g.state = h->bubble_state;
  g.cursor = h->bubble_cursor;
  g.total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  g.num_envs = h->cfg.num_envs;
  g.num_vehicles = h->cfg.num_vehicles;
  g.n_agents = h->cfg.num_vehicles - h->cfg.num_social;
  g.reset_elapsed_steps = h->cfg.reset_elapsed_steps;
  return g;
}

static void launch_control(smx_handle h, const TickPlan& p, const KernelArgs& a, hipStream_t stream) {
  const ControlKernels k = p.guard ? control_kernels<true>(h->cfg.action_space) : control_kernels<false>(h->cfg.action_space);
  switch (p.control) {
    case Control::NONE: break;
    case Control::MIXED: launch_control_mixed(h, p, a, stream); break;
    case Control::ONE: launch(k.one, p.wp_blocks, 0, stream, a); break;
    case Control::ONE_LDS: launch(k.one_lds, p.wp_blocks, 0, stream, a); break;
    case Control::LAW: launch(k.law, p.veh_blocks, stream, a, h->ctrl); break;
    case Control::PATHS_LAW:
      launch(k.paths, p.wp_blocks, stream, a, h->ctrl);
      launch(k.law, p.veh_blocks, stream, a, h->ctrl);
      break;
    case Control::FAST_LISTED: {
      const KernelArgs ac = with_slow(a, p.control_slow);  // the controller's slow list
      launch(k.fast, p.veh_blocks, 0, stream, ac);
      launch(k.listed, p.slow_blocks, stream, ac, h->ctrl);
      break;
    }
    case Control::KINEMATIC: launch(k.kinematic, p.veh_blocks, 0, stream, a); break;
    case Control::KINEMATIC_FOLLOW:  // (smx_set_history_agents holds the binding to Imitation)
      launch(p.guard ? k_control_kinematic<SMX_ACTION_SPACE_IMITATION, true, true> : k_control_kinematic<SMX_ACTION_SPACE_IMITATION, false, true>,
             p.veh_blocks, 0, stream, a);
      break;
    case Control::KINEMATIC_HANDOVER:  // (the binding again; smx_step_history_handover holds actions_f32 to non-null)
      launch(p.guard ? k_control_kinematic<SMX_ACTION_SPACE_IMITATION, true, false, true> : k_control_kinematic<SMX_ACTION_SPACE_IMITATION, false, false, true>,
             p.veh_blocks, 0, stream, a);
      break;
    case Control::KINEMATIC_BUBBLES:  // (the bubble pass, then the mixed tick that reads its state row; both on the caller's stream)
      hipLaunchKernelGGL(k_bubbles, dim3((unsigned)h->cfg.num_envs), dim3(64), 0, stream, bubble_args(h, a), h->bubbles);
      hipLaunchKernelGGL(p.guard ? k_control_kinematic_bubbles<true> : k_control_kinematic_bubbles<false>, dim3(p.veh_blocks), dim3(SMX_BLOCK), 0,
                         stream, a, (const uint8_t*)h->bubble_state);
      break;
  }
}

// the tick's alive list: the one the last pass's k_tail built from these flags (it zeroed this tick's slow-list
// counters too), or k_alive_list now
static void alive_list(smx_handle h, const TickPlan& p, KernelArgs& a, hipStream_t stream) {
  if (p.alive == AliveList::NONE) return;
  const AliveLayout al = alive_layout(h->cfg);
  int32_t* counters = h->alive_blob.get<int32_t>() + al.flat;
  a.alive_list = h->alive_blob.get<int32_t>();
  if (p.alive == AliveList::CARRIED) {
    a.alive_count = h->alive_blob.get<int32_t>() + al.seg + (size_t)8 * SMX_SEG_STRIDE * (h->seg_parity ^ 1);
    a.alive_segmented = 1;
  } else {
    const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
    a.alive_count = counters + h->alive_parity;
    hipLaunchKernelGGL(k_alive_list, dim3(smx_blocks(total, SMX_ALIVE_BLOCK)), dim3(SMX_ALIVE_BLOCK), 0, stream, a, h->alive_blob.get<int32_t>(),
                       counters + h->alive_parity, counters + (h->alive_parity ^ 1), p.alive_zero);
  }
  h->alive_parity ^= 1;
}

static void launch_grids(smx_handle h, const TickPlan& p, const KernelArgs& k, hipStream_t s) {
  const unsigned total = (unsigned)(h->cfg.num_envs * h->cfg.num_vehicles);
  switch (p.ogm) {
    case Ogm::NONE:
    case Ogm::IN_SENSORS: break;
    case Ogm::ENV2: hipLaunchKernelGGL((p.sized ? k_ogm_env<2, true> : k_ogm_env<2, false>), dim3((unsigned)h->cfg.num_envs), dim3(SMX_OGM_WAVES * 64), p.ogm_lds, s, k); break;
    case Ogm::ENV1: hipLaunchKernelGGL((p.sized ? k_ogm_env<1, true> : k_ogm_env<1, false>), dim3((unsigned)h->cfg.num_envs), dim3(SMX_OGM_WAVES * 64), p.ogm_lds, s, k); break;
    case Ogm::PER_OBSERVER: launch(k_ogm, total, p.ogm_lds, s, k); break;
  }
  if (p.dagm) launch(k_dagm, total, p.dagm_bytes, s, k);
  if (p.rgb) launch(k_rgb, total, p.rgb_lds, s, k);
}

// the slow seeds chain over the vehicles the one-lane seeds kernel left seed_pending: searches from scratch, then their
// walks and rows by the serial emitter
static void launch_slow_chain(const TickPlan& p, const KernelArgs& ks, hipStream_t s) {
  if (p.chain_fused) {
    launch(p.sized ? k_scan_listed<1, false, SMX_TEAM, true> : k_scan_listed<1, false, SMX_TEAM>, p.slow_blocks, 0, s, ks);
    launch(k_waypoints_walk_listed, p.slow_blocks, 0, s, ks);
  } else {
    launch(p.sized ? k_scan_listed<1, false, SMX_TEAM_LARGE, true> : k_scan_listed<1>, p.slow_blocks, 0, s, ks);
    launch(k_waypoints_listed, p.slow_blocks, 0, s, ks);
    launch(k_wp_walk_listed, p.slow_blocks, 0, s, ks);
  }
}

// one tick's observations: grid kernels, the scan's halves, the slow seeds chain, rows, observe, lidar, joins, road
// waypoints (`ph`: the call's phase events, null unless the plan is phased)
static void observation_pass(smx_handle h, const TickPlan& p, const KernelArgs& k, hipStream_t stream, hipEvent_t* ph) {
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  const hipStream_t s_grid = p.fork ? h->streams.side[0] : stream, s_obs = p.fork ? h->streams.side[1] : stream;
  if (p.fork) {
    (void)hipEventRecord(h->streams.ev_fork_grid, stream);
    (void)hipStreamWaitEvent(s_grid, h->streams.ev_fork_grid, 0);
    launch_grids(h, p, k, s_grid);
    if (p.lidar == Lidar::SIDE) launch(p.sized ? k_lidar<true> : k_lidar<false>, p.lidar_blocks, 0, s_grid, k);
  }
  // the scan's halves as two launches in the large form, on two streams when forked: path seeds (-> waypoint kernels) on
  // the caller's, road facts (-> observe) on side 1; each half appends to its own slow list
  KernelArgs ks = with_slow(k, p.seeds_slow);
  ks.seed_pending = p.seed_pending();
  switch (p.seeds()) {
    case Seeds::SCAN: {
      const Kernel scan = p.scan_split ? (p.routed ? k_scan<true, true> : k_scan<true>) : (p.routed ? k_scan<false, true> : k_scan<false>);
      launch(scan, p.seeds_blocks, 0, stream, k);
      break;
    }
    case Seeds::ONE_LANE: launch(k_scan_fast<1>, p.seeds_blocks, 0, stream, ks); break;
    case Seeds::ROUTED: launch(p.sized ? k_scan_half<1, true, SMX_TEAM_LARGE, true> : k_scan_half<1, true>, p.seeds_blocks, 0, stream, k); break;
    case Seeds::WIDE: launch(p.sized ? k_scan_half<1, false, SMX_TEAM, true> : k_scan_half<1, false, SMX_TEAM>, p.seeds_blocks, 0, stream, k); break;
    case Seeds::FOUR: launch(p.sized ? k_scan_half<1, false, SMX_TEAM_LARGE, true> : k_scan_half<1>, p.seeds_blocks, 0, stream, k); break;
  }
  if (p.chain() == SlowChain::SIDE) {
    // the slow chain runs beside the main chain (k_wp_walk -> k_waypoints_emit pass over its vehicles)
    // (one event after the seeds half serves this fork and the facts half's below: every record on the caller's
    // stream is a packet its next kernel waits behind, ten microseconds of the tick's longest chain)
    (void)hipEventRecord(h->streams.ev_fork, stream);
    (void)hipStreamWaitEvent(h->streams.side[2], h->streams.ev_fork, 0);
    launch_slow_chain(p, ks, h->streams.side[2]);
  }
  if (p.facts_start == FactsStart::WITH_GRIDS) {
    (void)hipStreamWaitEvent(s_obs, h->streams.ev_fork_grid, 0);
  } else if (p.facts_start == FactsStart::AFTER_SEEDS) {
    if (p.chain() != SlowChain::SIDE) (void)hipEventRecord(h->streams.ev_fork, stream);
    (void)hipStreamWaitEvent(s_obs, h->streams.ev_fork, 0);
  }
  const KernelArgs kf = with_slow(k, p.facts_slow);
  switch (p.facts) {
    case Facts::SCAN: break;
    case Facts::ONE_LANE:
      launch(k_scan_fast<0>, p.facts_blocks, 0, s_obs, kf);
      launch(p.sized ? k_scan_listed<0, false, SMX_TEAM_LARGE, true> : k_scan_listed<0>, p.slow_blocks, 0, s_obs, kf);
      break;
    case Facts::WIDE: launch(p.sized ? k_scan_half<0, false, SMX_TEAM, true> : k_scan_half<0, false, SMX_TEAM>, p.facts_blocks, 0, s_obs, kf); break;
    case Facts::FOUR: launch(p.sized ? k_scan_half<0, false, SMX_TEAM_LARGE, true> : k_scan_half<0>, p.facts_blocks, 0, s_obs, kf); break;  // (the facts half seeds no path)
  }
  if (ph) (void)hipEventRecord(ph[SMX_PHASE_SCAN + 1], stream);
  if (!p.fork) launch_grids(h, p, k, stream);
  if (ph) (void)hipEventRecord(ph[SMX_PHASE_OGM + 1], stream);
  KernelArgs kw = k;  // the waypoint kernels, which pass over the slow chain's vehicles
  kw.seed_pending = p.seed_pending();
  const unsigned walk_blocks = smx_blocks(total * SMX_WP_LANES);
  switch (p.rows) {
    case Rows::SENSORS: launch(p.sized ? k_sensors_sized : k_sensors, p.sensor_blocks, p.sensor_lds, stream, k); break;
    case Rows::UNSTAGED: launch(k_waypoints, p.wp_blocks, 0, stream, k); break;
    case Rows::TABLES:
      launch(k_wp_walk, walk_blocks, 0, stream, kw);
      launch(k_waypoints_tables, p.wp_blocks, std::max((size_t)h->cfg.wp_len * SMX_BLOCK * 16, (size_t)SMX_MAX_KNOTS * SMX_BLOCK * sizeof(int)),
             stream, k);
      break;
    case Rows::EMIT:
    case Rows::EMIT_CHAIN_SIDE:
    case Rows::EMIT_CHAIN_AFTER:
      if (!p.knot_table) launch(k_wp_walk, walk_blocks, 0, stream, kw);  // (the table: k_waypoints_emit reads the rows)
      kw = with_slow(kw, p.rows_slow);
      launch(k_waypoints_emit, p.wp_blocks, 0, stream, kw);
      launch(k_waypoints_listed, p.slow_blocks, 0, stream, kw);
      if (p.rows == Rows::EMIT_CHAIN_AFTER) launch_slow_chain(p, ks, stream);  // (one stream: after the main waypoint kernels)
      break;
  }
  if (!p.small()) launch(p.sized ? k_observe_sized : k_observe, p.obs_blocks, 0, s_obs, k);
  if (p.lidar == Lidar::CALLER) launch(p.sized ? k_lidar<true> : k_lidar<false>, p.lidar_blocks, 0, stream, k);
  if (p.fork) {
    // (each side stream joins the caller's directly: chaining side 0 through side 1 puts one more hop behind the
    // last kernel when k_observe ends the tick — 1 % late in a run)
    for (int i = 0; i < (p.chain() == SlowChain::SIDE ? 3 : 2); ++i) {
      (void)hipEventRecord(h->streams.ev_join[i], h->streams.side[i]);
      (void)hipStreamWaitEvent(stream, h->streams.ev_join[i], 0);
    }
  }
  if (p.road_waypoints)  // (poses are the tick's new ones; flags still those of its start)
    launch(k_road_waypoints, smx_blocks(total * SMX_RW_LANE_CAP), 0, stream, k);
  if (p.lane_ttc)  // (the waypoint, neighbour and ego rows are complete here in every form: the side streams have joined)
    hipLaunchKernelGGL(k_lane_ttc, dim3(p.ttc_blocks), dim3(SMX_BLOCK), p.ttc_lds, stream, k, (const int32_t*)nullptr, (const int32_t*)nullptr);
  if (p.ego_centric)  // (the same site: every world row it reads, the lidar's and the road waypoints' included, is complete)
    hipLaunchKernelGGL(k_ego_frame, dim3(p.ec_blocks), dim3(SMX_BLOCK), 0, stream, k, (const int32_t*)nullptr, (const int32_t*)nullptr);
  if (ph) (void)hipEventRecord(ph[SMX_PHASE_SENSORS + 1], stream);
}

// the end of the pass: k_tail (the tick's commit, the new vehicles' grid tiles, the env groups with new vehicles,
// the next tick's alive list), then the reset pass over those groups (first observations of the new vehicles)
static int tail_and_reset_pass(smx_handle h, const TickPlan& p, const KernelArgs& a, const uint8_t* mask, const smx_state* st,
                               hipStream_t stream, hipEvent_t* ph) {
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  const AliveLayout al = alive_layout(h->cfg);
  KernelArgs r = a;
  r.alive_list = nullptr;
  r.alive_count = nullptr;
  r.alive_segmented = 0;
  r.first_only = 1;
  r.keep_reward_done = p.is_step ? 1 : 0;
  r.reset_all = (!p.is_step && mask == nullptr) ? 1 : 0;
  r.env_mask = p.is_step ? nullptr : mask;
  if (!p.is_step) {
    if (p.entry)  // (the ENTRY instantiations: pending agents; the plain ones hold nothing of it)
      launch(p.guard ? (p.sized ? k_reset<true, true, true> : k_reset<true, false, true>)
                     : (p.sized ? k_reset<false, true, true> : k_reset<false, false, true>), p.veh_blocks, 0, stream, r);
    else
      launch(p.guard ? (p.sized ? k_reset<true, true> : k_reset<true>) : (p.sized ? k_reset<false, true> : k_reset<false>), p.veh_blocks, 0, stream, r);
    launch(k_reset_env, p.env_blocks, 0, stream, r);
  }
  TailArgs t{};
  t.commit = p.is_step ? 1 : 0;
  t.grids = p.tail_grids ? 1 : 0;
  t.groups = h->alive_blob.get<int32_t>() + al.groups;
  t.n_groups = h->alive_blob.get<int32_t>() + al.group_count + SMX_SEG_STRIDE * h->group_parity;
  t.n_groups_next = h->alive_blob.get<int32_t>() + al.group_count + SMX_SEG_STRIDE * (h->group_parity ^ 1);
  if (p.tail_builds_list) {  // (the next tick's parity is h->alive_parity now)
    t.list = h->alive_blob.get<int32_t>();
    t.seg_count = h->alive_blob.get<int32_t>() + al.seg + (size_t)8 * SMX_SEG_STRIDE * h->seg_parity;
    t.seg_next = h->alive_blob.get<int32_t>() + al.seg + (size_t)8 * SMX_SEG_STRIDE * (h->seg_parity ^ 1);
    t.flat_next = h->alive_blob.get<int32_t>() + al.flat + h->alive_parity;
    t.slow_next = SlowLists{h->slow_blob.get<int32_t>(), total}.counters(h->alive_parity);
  }
  hipLaunchKernelGGL(p.guard ? k_tail<true> : k_tail<false>, dim3(p.obs_blocks), dim3(SMX_BLOCK), p.tail_grids ? std::max({p.ogm_bytes, p.dagm_bytes, p.rgb_lds}) : 0, stream, r, t);
  if (p.entry_first)  // (a large form's tick: this tick's entrants into the reset pass's groups, smx_k_entry.h)
    hipLaunchKernelGGL(k_entry_first, dim3(p.obs_blocks), dim3(SMX_BLOCK), 0, stream, r, t.groups, t.n_groups);
  if (ph) SMX_HIP(hipEventRecord(ph[SMX_PHASE_COMMIT + 1], stream));
  h->group_parity ^= 1;
  h->list_ready = p.tail_builds_list;
  if (p.tail_builds_list) {
    h->seg_parity ^= 1;
    h->list_state = *st;
  }
  if (p.reset_pass) {
    if (p.road_waypoints)  // before k_first clears SMX_F_FIRST
      launch(k_road_waypoints, smx_blocks(total * SMX_RW_LANE_CAP), 0, stream, r);
    if (p.lidar_first) {
      launch(p.sized ? k_lidar_first<true> : k_lidar_first<false>, (unsigned)std::min<size_t>(SMX_LIDAR_FIRST_BLOCKS, total), 0, stream, r);
      r.lidar_blocks = 0;
    }
    r.walk_new = p.first_walks_new ? 1 : 0;
    hipLaunchKernelGGL((p.sized ? k_first_sized : k_first), dim3(p.obs_blocks), dim3(SMX_FIRST_BLOCK), 0, stream, r, t.groups, t.n_groups);
    if (p.lane_ttc)  // after k_first: it reads the first observations' rows, not SMX_F_FIRST
      hipLaunchKernelGGL(k_lane_ttc, dim3(p.ttc_first_blocks), dim3(SMX_BLOCK), p.ttc_lds, stream, r, (const int32_t*)t.groups, (const int32_t*)t.n_groups);
    if (p.ego_centric)
      hipLaunchKernelGGL(k_ego_frame, dim3(p.ec_first_blocks), dim3(SMX_BLOCK), 0, stream, r, (const int32_t*)t.groups, (const int32_t*)t.n_groups);
  }
  return SMX_OK;
}

// the argument block every kernel of the call starts from
static KernelArgs kernel_args(smx_handle h, const TickPlan& p, const int8_t* actions, const float* actions_f32, const double* traj,
                              const int32_t* traj_n, int32_t traj_max, const uint8_t* mask, const smx_state* st, const smx_spawns* sp,
                              const smx_outputs* out) {
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  KernelArgs a;
  a.cfg = h->cfg;
  a.map = h->map;
  a.st = *st;
  a.sp = *sp;
  a.out = *out;
  a.actions = actions;
  a.actions_f32 = actions_f32;
  a.traj = traj;
  a.traj_n = traj_n;
  a.traj_max = traj_max;
  a.env_mask = mask;
  a.lidar_rays = h->lidar_rays;
  a.vias = h->n_vias > 0 ? h->vias_dev.get<smx_via>() : nullptr;
  a.missions = h->missions;
  a.via_slot_off = h->via_off_dev.get<int32_t>();
  a.first_only = 0;
  a.keep_reward_done = 0;
  a.reset_all = 0;
  a.heading_gain_pos = h->heading_gain_pos;
  a.nb_d2_max = h->nb_d2_max;
  a.walk_new = 0;
  a.wp_spill = h->spill_blob.get<char>();
  a.wp_pool_limit = h->wp_pool_limit;
  a.lateral_gain_pos = h->lateral_gain_pos;
  a.debug_skip = h->debug_skip;
  a.knots = h->knots;
  a.knot_table = p.knot_table ? h->knot_table.get<KnotRow>() : nullptr;
  a.knot_served = (p.knot_table && h->knot_table_mode == 2) ? (unsigned long long*)(h->knot_stats.get<int32_t>() + 2) : nullptr;
  a.status = h->status_dev.get<int32_t>();
  a.alive_list = nullptr;
  a.alive_count = nullptr;
  a.alive_segmented = 0;
  a.slow_list = nullptr;
  a.slow_count = nullptr;
  a.seed_pending = nullptr;
  a.seeds_carry = h->scan_carry.get<double>();
  a.facts_carry = h->scan_carry ? h->scan_carry.get<double>() + 4 * total : nullptr;
  a.dagm_reach = h->dagm_reach;
  a.rgb = h->rgb_out;
  a.guard = h->guard_out;
  a.guard_box = h->guard_box;
  a.history = h->history;
  a.dims = h->dims;
  a.ha_action = h->ha_action;
  a.ha_status = h->ha_status;
  a.ogm_mask = (p.ogm_delta && out->ogm) ? h->ogm_mask.get<unsigned long long>() : nullptr;
  a.entry = h->entry;
  a.wp_blocks = (int)p.wp_blocks;
  a.obs_blocks = (int)p.obs_blocks;
  a.lidar_blocks = (int)p.lidar_blocks;
  return a;
}

// which entry point a call came through (each hands over its own pointers and leaves the others null)
enum class Entry { RESET, LANE, FLOATS, TRAJECTORY, TARGET_POSE, TRAJECTORY_WITH_TIME, HISTORY_AGENTS, HISTORY_HANDOVER, MIXED };
static const char* entry_name(Entry e) {
  static const char* const names[] = {"smx_reset", "smx_step", "smx_step_continuous", "smx_step_trajectory", "smx_step_target_pose",
                                      "smx_step_trajectory_with_time", "smx_step_history_agents", "smx_step_history_handover", "smx_step_mixed"};
  return names[(int)e];
}
// (traj_max: columns per row of a TrajectoryWithTime action)
static int enqueue(smx_handle h, const Entry entry, const int8_t* actions, const float* actions_f32, const double* traj,
                   const int32_t* traj_n, int32_t traj_max, const uint8_t* mask, const smx_state* st,
                   const smx_spawns* sp, const smx_outputs* out, void* stream_) {
  if (!h) return SMX_ERR_INVALID;
  if (!h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_load_map has not been called");
  int rc = check_buffers(h, st, sp, out);
  if (rc != SMX_OK) return rc;
  const bool is_step = entry != Entry::RESET;
  const bool follow = entry == Entry::HISTORY_AGENTS, handover = entry == Entry::HISTORY_HANDOVER, mixed = entry == Entry::MIXED;
  if (is_step) {  // (smx_step_mixed with a table bound, the others without one; its buffers: smx_handle.h check_step_entry)
    const smx_mixed_actions acts{actions, actions_f32, traj, traj_n};
    rc = check_step_entry(h, entry_name(entry), mixed ? &acts : nullptr, mixed);
    if (rc != SMX_OK) return rc;
  }
  if (follow) {  // (the binding holds cfg.action_space to Imitation; the tick reads no action)
    if (h->history.follow == nullptr) return fail(h, SMX_ERR_STATE, "smx_step_history_agents: no history agents are bound (smx_set_history_agents)");
  } else if (handover) {  // (the binding holds cfg.action_space to Imitation; the driven agents' rows are read)
    if (h->history.follow == nullptr || (h->history.handover == nullptr && h->bubble_state == nullptr))
      return fail(h, SMX_ERR_STATE, "smx_step_history_handover: no handover table is bound (smx_set_history_handover)");
    if (actions_f32 == nullptr) return fail(h, SMX_ERR_INVALID, "smx_step_history_handover: actions_dev is NULL");
  } else if (is_step && !mixed) {  // (smx_step_mixed's buffers were checked against the table above)
    const int sp_ = h->cfg.action_space;
    const bool ok = sp_ == SMX_ACTION_SPACE_LANE ? (entry == Entry::LANE && actions != nullptr)
                    : (sp_ == SMX_ACTION_SPACE_TRAJECTORY || sp_ == SMX_ACTION_SPACE_MPC)
                        ? (entry == Entry::TRAJECTORY && traj != nullptr && traj_n != nullptr)
                    : sp_ == SMX_ACTION_SPACE_TARGET_POSE ? (entry == Entry::TARGET_POSE && traj != nullptr)
                    : sp_ == SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME
                        ? (entry == Entry::TRAJECTORY_WITH_TIME && traj != nullptr && traj_n != nullptr)
                        : (entry == Entry::FLOATS && actions_f32 != nullptr);
    if (!ok)
      return fail(h, SMX_ERR_INVALID,
                  "actions do not match cfg.action_space (smx_step: Lane, smx_step_trajectory: Trajectory and MPC, "
                  "smx_step_continuous: the float spaces and Imitation, smx_step_target_pose: TargetPose, "
                  "smx_step_trajectory_with_time: TrajectoryWithTime)");
  }
  hipStream_t stream = (hipStream_t)stream_;
  const TickPlan p = tick_plan(plan_inputs(h, is_step, st, follow, handover, mixed));
  if (is_step && h->entry_reset_needed)
    return fail(h, SMX_ERR_STATE, "agent entry: smx_set_agent_entry bound or unbound a table since the last smx_reset of every "
                                  "env (env_mask NULL); step after one");
  if (!is_step && mask == nullptr) h->entry_reset_needed = false;
  KernelArgs a = kernel_args(h, p, actions, actions_f32, traj, traj_n, traj_max, mask, st, sp, out);
  const bool timed = h->timing && is_step && h->ev_used < 65536;
  if (timed) {
    if (h->ev_pool.ev.size() < 2 * (h->ev_used + 1)) {
      hipEvent_t e0, e1;
      SMX_HIP(hipEventCreate(&e0));
      SMX_HIP(hipEventCreate(&e1));
      h->ev_pool.ev.push_back(e0);
      h->ev_pool.ev.push_back(e1);
    }
    SMX_HIP(hipEventRecord(h->ev_pool.ev[2 * h->ev_used], stream));
  }
  // phase timing (smx_set_timing level 2): one boundary event after every kernel of the tick
  hipEvent_t* ph = nullptr;
  if (p.phased) {
    const size_t need = (h->ph_used + 1) * (SMX_PHASE_COUNT + 1);
    while (h->ph_pool.ev.size() < need) {
      hipEvent_t e;
      SMX_HIP(hipEventCreate(&e));
      h->ph_pool.ev.push_back(e);
    }
    ph = &h->ph_pool.ev[h->ph_used * (SMX_PHASE_COUNT + 1)];
    SMX_HIP(hipEventRecord(ph[0], stream));
  }
  if (a.ogm_mask && !(h->ogm_known && h->ogm_rows == out->ogm)) {
    // the masks do not describe these rows (KernelArgs::ogm_mask): every piece may be non-zero, this pass stores whole tiles
    SMX_HIP(hipMemsetAsync(h->ogm_mask.get<unsigned long long>(), 0xff, h->ogm_mask_bytes, stream));
    h->ogm_rows = out->ogm;
    h->ogm_known = true;
  }
  if (!a.ogm_mask) h->ogm_known = false;  // a pass that stores without the masks leaves them stale
  if (p.social) launch(k_social, p.veh_blocks, 0, stream, a);
  alive_list(h, p, a, stream);
  if (is_step) {
    launch_control(h, p, a, stream);
    if (p.entry)  // (after the control phase has moved the social slots, ahead of every sensor: smx_k_entry.h)
      hipLaunchKernelGGL(p.small() ? (p.guard ? k_entry<true, false> : k_entry<false, false>)
                                   : (p.guard ? k_entry<true, true> : k_entry<false, true>),
                         dim3((unsigned)h->cfg.num_envs), dim3(64), 0, stream, a);
    if (ph) SMX_HIP(hipEventRecord(ph[SMX_PHASE_CONTROL + 1], stream));
    observation_pass(h, p, a, stream, ph);
  }
  rc = tail_and_reset_pass(h, p, a, mask, st, stream, ph);
  if (rc != SMX_OK) return rc;
  // bubbles: an env that this pass has reset (smx_reset, or auto_reset inside a mixed tick) starts from zero bytes
  if (h->bubble_state != nullptr && (!is_step || (handover && p.reset_pass)))
    hipLaunchKernelGGL(k_bubbles_clear, dim3(p.veh_blocks), dim3(SMX_BLOCK), 0, stream, bubble_args(h, a));
  if (p.frame_stack) {  // (after the reset pass: a restarted env's rows hold its first observation)
    rc = launch_frame_stacks(h, is_step, mask, st, out, stream);
    if (rc != SMX_OK) return rc;
  }
  SMX_HIP(hipGetLastError());
  if (ph) {
    SMX_HIP(hipEventRecord(ph[SMX_PHASE_RESET + 1], stream));
    h->ph_used += 1;
  }
  if (timed) {
    SMX_HIP(hipEventRecord(h->ev_pool.ev[2 * h->ev_used + 1], stream));
    h->ev_used += 1;
  }
  return SMX_OK;
}

extern "C" int smx_reset(smx_handle h, const uint8_t* env_mask_dev, const smx_state* st, const smx_spawns* sp,
                         const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::RESET, nullptr, nullptr, nullptr, nullptr, 0, env_mask_dev, st, sp, out, hip_stream);
}

extern "C" int smx_step(smx_handle h, const int8_t* actions_dev, const smx_state* st, const smx_spawns* sp,
                        const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::LANE, actions_dev, nullptr, nullptr, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_continuous(smx_handle h, const float* actions_dev, const smx_state* st, const smx_spawns* sp,
                                   const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::FLOATS, nullptr, actions_dev, nullptr, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_history_agents(smx_handle h, const smx_state* st, const smx_spawns* sp, const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::HISTORY_AGENTS, nullptr, nullptr, nullptr, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_history_handover(smx_handle h, const float* actions_dev, const smx_state* st, const smx_spawns* sp,
                                         const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::HISTORY_HANDOVER, nullptr, actions_dev, nullptr, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_trajectory(smx_handle h, const double* trajectories_dev, const int32_t* counts_dev,
                                   const smx_state* st, const smx_spawns* sp, const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::TRAJECTORY, nullptr, nullptr, trajectories_dev, counts_dev, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_target_pose(smx_handle h, const double* targets_dev, const smx_state* st, const smx_spawns* sp,
                                    const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::TARGET_POSE, nullptr, nullptr, targets_dev, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_trajectory_with_time(smx_handle h, const double* trajectories_dev, const int32_t* counts_dev,
                                             int32_t max_points, const smx_state* st, const smx_spawns* sp,
                                             const smx_outputs* out, void* hip_stream) {
  if (h && max_points < 2) return fail(h, SMX_ERR_INVALID, "smx_step_trajectory_with_time: max_points < 2");
  return enqueue(h, Entry::TRAJECTORY_WITH_TIME, nullptr, nullptr, trajectories_dev, counts_dev, max_points, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_mixed(smx_handle h, const smx_mixed_actions* acts, const smx_state* st, const smx_spawns* sp,
                              const smx_outputs* out, void* hip_stream) {
  if (!h) return SMX_ERR_INVALID;
  if (!acts) return check_step_entry(h, "smx_step_mixed", nullptr, true);  // (no table: SMX_ERR_STATE; else the null argument)
  return enqueue(h, Entry::MIXED, acts->lane_dev, acts->floats_dev, acts->trajectories_dev, acts->counts_dev, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_actions_to_world(smx_handle h, int32_t action_space, const double* in_dev, const int32_t* counts_dev,
                                    int32_t max_points, double* out_dev, const smx_outputs* out, void* hip_stream) {
  if (!h) return SMX_ERR_INVALID;
  const smx_config& c = h->cfg;
  if (h->spaces.space != nullptr)
    return fail(h, SMX_ERR_STATE, "smx_actions_to_world: per-agent action spaces are bound (smx_set_agent_spaces); ego-frame actions of a "
                                  "mixed fleet are not built");
  if (!(c.sensors & SMX_SENSOR_EGO_CENTRIC))
    return fail(h, SMX_ERR_STATE, "smx_actions_to_world: the configuration has no SMX_SENSOR_EGO_CENTRIC (no frame is kept)");
  const bool traj = action_space == SMX_ACTION_SPACE_TRAJECTORY || action_space == SMX_ACTION_SPACE_MPC;
  const bool pose = action_space == SMX_ACTION_SPACE_TARGET_POSE;
  const bool timed = action_space == SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME;
  if (!traj && !pose && !timed)
    return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: only Trajectory, MPC, TargetPose and TrajectoryWithTime actions have a frame");
  if (action_space != c.action_space) return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: action_space is not cfg.action_space");
  if (!in_dev || !out_dev || in_dev == out_dev || (!pose && !counts_dev))
    return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: null action buffer or counts, or the output is the input");
  if (timed && max_points < 2) return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: max_points < 2");
  const uint64_t total = (uint64_t)c.num_envs * c.num_vehicles;
  if (!out || !out->ego_frame || !out->ec_flags || out->dtype[SMX_OUT_EGO_FRAME] != SMX_DT_F64 ||
      out->dtype[SMX_OUT_EC_FLAGS] != SMX_DT_U8 || out->count[SMX_OUT_EGO_FRAME] < 4 * total || out->count[SMX_OUT_EC_FLAGS] < total)
    return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: out.ego_frame / out.ec_flags missing, short or mistyped");
  const int cols = traj ? SMX_TRAJ_COLS : pose ? 1 : max_points;
  const unsigned blocks = smx_blocks((size_t)total * cols);
  hipStream_t s = (hipStream_t)hip_stream;
#define SMX_A2W(SPACE)                                                                                                  \
  hipLaunchKernelGGL(k_actions_to_world<SPACE>, dim3(blocks), dim3(SMX_BLOCK), 0, s, in_dev, counts_dev, out_dev,        \
                     (const double*)out->ego_frame, (const uint8_t*)out->ec_flags, (size_t)total, (int)c.num_vehicles, \
                     (int)c.num_social, cols)
  if (traj) SMX_A2W(SMX_ACTION_SPACE_TRAJECTORY);
  else if (pose) SMX_A2W(SMX_ACTION_SPACE_TARGET_POSE);
  else SMX_A2W(SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME);
#undef SMX_A2W
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

extern "C" int smx_sync(smx_handle h, void* hip_stream) {
  if (!h) return SMX_ERR_INVALID;
  SMX_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
  if (h->status_dev) {  // what the kernels could not report themselves
    int32_t bits = 0;
    SMX_HIP(hipMemcpy(&bits, h->status_dev.get<int32_t>(), sizeof(bits), hipMemcpyDeviceToHost));
    if (bits) {
      SMX_HIP(hipMemset(h->status_dev.get<int32_t>(), 0, sizeof(int32_t)));
      if (bits & SMX_DEVICE_BAD_LANE_ACTION)
        return fail(h, SMX_ERR_INVALID,
                    "a Lane action code outside -1..3 reached smx_step since the last smx_sync; the agents that sent one "
                    "were stepped as if they had sent no action");
      if (bits & SMX_DEVICE_BAD_TRAJECTORY)
        return fail(h, SMX_ERR_INVALID,
                    "an illegal TrajectoryWithTime action reached smx_step_trajectory_with_time since the last smx_sync (fewer "
                    "than two points or more than max_points, a value that is not finite, times not strictly increasing, no "
                    "point later than dt or the first one already later); the agents that sent one were not moved");
      if (bits & SMX_DEVICE_BAD_TARGET_POSE)
        return fail(h, SMX_ERR_INVALID,
                    "a TargetPose action whose pose is not finite reached smx_step_target_pose, or an Imitation action "
                    "with an infinite component or a pose or speed that is not finite reached smx_step_continuous, since the "
                    "last smx_sync; the agents that sent one were stepped as if they had sent no action");
    }
  }
  return SMX_OK;
}

// Developer diagnostics (not part of include/smx.h): the lengths of the last large-form tick's slow lists
// (scan facts, scan seeds, control, waypoint rows), after a synchronisation of the device.
extern "C" int smx_debug_slow_counts(smx_handle h, int32_t* out4) {
  if (!h || !out4) return SMX_ERR_INVALID;
  if (!h->slow_blob) return fail(h, SMX_ERR_STATE, "no slow lists (the map is not loaded)");
  SMX_HIP(hipDeviceSynchronize());
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  SMX_HIP(hipMemcpy(out4, SlowLists{h->slow_blob.get<int32_t>(), total}.counters(h->alive_parity ^ 1), 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SMX_OK;
}

// developer / tests: use only `records` of k_waypoints_emit's LDS knot pool (0 < records <= SMX_WPE_POOL), so that
// small batches reach its overflow area too (a full pool needs sixteen vehicles in a bend in one workgroup)
extern "C" int smx_debug_set_wp_pool(smx_handle h, int32_t records) {
  if (!h) return SMX_ERR_INVALID;
  if (records < 1 || records > SMX_WPE_POOL) return fail(h, SMX_ERR_INVALID, "smx_debug_set_wp_pool: 1 .. SMX_WPE_POOL records");
  h->wp_pool_limit = records;
  return SMX_OK;
}

// developer / tests: the one-lane cut's knot lists from the map's knot table (1, the default), from the walks of
// k_wp_walk as before the table (0), or from the table with a count of the path lanes it serves (2)
extern "C" int smx_debug_set_knot_table(smx_handle h, int32_t mode) {
  if (!h) return SMX_ERR_INVALID;
  if (mode < 0 || mode > 2) return fail(h, SMX_ERR_INVALID, "smx_debug_set_knot_table: 0 (walked lists), 1 (table), 2 (table, counting)");
  h->knot_table_mode = mode;
  return SMX_OK;
}

// the loaded map's knot table after a synchronisation of the device: rows in all, rows tabled, tabled rows that stay on
// their start road, path lanes served from a row while the switch above was 2
extern "C" int smx_debug_knot_table_stats(smx_handle h, int64_t* out4) {
  if (!h || !out4) return SMX_ERR_INVALID;
  if (!h->knot_table) return fail(h, SMX_ERR_STATE, "no knot table (no map loaded, or no waypoints sensor)");
  SMX_HIP(hipDeviceSynchronize());
  int32_t st[4];
  SMX_HIP(hipMemcpy(st, h->knot_stats.get<int32_t>(), sizeof(st), hipMemcpyDeviceToHost));
  unsigned long long served;
  std::memcpy(&served, st + 2, sizeof(served));
  out4[0] = h->map.n_lanepoints;
  out4[1] = st[0];
  out4[2] = st[1];
  out4[3] = (int64_t)served;
  return SMX_OK;
}

// The caller wrote into the OGM rows itself: the next call stores whole tiles (the masks describe what the library stored).
extern "C" int smx_invalidate_outputs(smx_handle h) {
  if (!h) return SMX_ERR_INVALID;
  h->ogm_known = false;
  return SMX_OK;
}

// OGM delta stores on (the default) or off: off passes the kernels the null mask and every call stores every piece.
extern "C" int smx_set_ogm_delta(smx_handle h, int on) {
  if (!h) return SMX_ERR_INVALID;
  h->ogm_delta = on != 0;
  h->ogm_known = false;
  return SMX_OK;
}

extern "C" int smx_set_timing(smx_handle h, int level) {
  if (!h) return SMX_ERR_INVALID;
  h->timing = level == 1;
  h->phase_timing = level == 2;
  return SMX_OK;
}

extern "C" int smx_read_phase_ms(smx_handle h, float* ms, int32_t max_steps, int32_t* n) {
  if (!h || !ms || !n || max_steps < 0) return SMX_ERR_INVALID;
  int32_t count = 0;
  for (size_t i = 0; i < h->ph_used; ++i) {
    hipEvent_t* ph = &h->ph_pool.ev[i * (SMX_PHASE_COUNT + 1)];
    SMX_HIP(hipEventSynchronize(ph[SMX_PHASE_COUNT]));
    if (count >= max_steps) continue;
    for (int p = 0; p < SMX_PHASE_COUNT; ++p) {
      float t = 0.f;
      SMX_HIP(hipEventElapsedTime(&t, ph[p], ph[p + 1]));
      ms[(size_t)count * SMX_PHASE_COUNT + p] = t;
    }
    ++count;
  }
  h->ph_used = 0;
  *n = count;
  return SMX_OK;
}

extern "C" int smx_read_step_ms(smx_handle h, float* ms, int32_t max, int32_t* n) {
  if (!h || !ms || !n || max < 0) return SMX_ERR_INVALID;
  int32_t count = 0;
  for (size_t i = 0; i < h->ev_used; ++i) {
    SMX_HIP(hipEventSynchronize(h->ev_pool.ev[2 * i + 1]));
    float t = 0.f;
    SMX_HIP(hipEventElapsedTime(&t, h->ev_pool.ev[2 * i], h->ev_pool.ev[2 * i + 1]));
    if (count < max) ms[count++] = t;
  }
  h->ev_used = 0;
  *n = count;
  return SMX_OK;
}

extern "C" int smx_last_step_ms(smx_handle h, float* ms) {
  if (!h || !ms) return SMX_ERR_INVALID;
  if (h->ev_used == 0) return fail(h, SMX_ERR_STATE, "no timed step recorded (smx_set_timing(1) then smx_step)");
  const size_t i = h->ev_used - 1;
  SMX_HIP(hipEventSynchronize(h->ev_pool.ev[2 * i + 1]));
  SMX_HIP(hipEventElapsedTime(ms, h->ev_pool.ev[2 * i], h->ev_pool.ev[2 * i + 1]));
  return SMX_OK;
}

extern "C" const char* smx_last_error(smx_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" void smx_destroy(smx_handle h) { destroy_impl(h); }

// smx_k_control.h — the control phase: every launch form of the controller, the kinematic forms, the bubble pass and k_social.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_bubbles.h"
#include "smx_guard.h"
#include "smx_handle.h"
#include "smx_history.h"
#include "smx_plan.h"
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

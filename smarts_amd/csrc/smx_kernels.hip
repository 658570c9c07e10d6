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
// Five phases are in headers of their own so far, included below: smx_k_control.h (every k_control form, the kinematic
// forms, k_bubbles, k_social), smx_k_scan.h (k_scan and its listed forms), smx_k_waypoints.h (the waypoints role's three
// forms, k_wp_walk, k_knot_table, k_waypoints and its listed forms), smx_k_grids.h (OGM / DAGM / RGB roles, k_ogm, k_dagm,
// k_rgb) and smx_k_lidar.h (lidar role, k_lidar, k_lidar_first); what the phases share is in smx_tick.h.  Left here: the
// observe role, the pass glue with k_alive_list, the row kernels and the host code.
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
#include "smx_k_control.h"
#include "smx_k_grids.h"
#include "smx_k_lidar.h"
#include "smx_k_scan.h"
#include "smx_k_entry.h"  // (after smx_k_scan.h: its large-form instance runs the facts half for an entrant)
#include "smx_k_waypoints.h"
#include "smx_plan.h"
#include "smx_scan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

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
// (`mission`: the slot's mission_row)
__device__ inline void lap_goal_gate(const KernelArgs& a, size_t gid, size_t total, int mission, bool tick) {
  const smx_mission_goal g = a.missions.goal_kind[mission];
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
// (pooled: the kernel is a pool instance, TickPlan::pool — a literal too; mission_row, smx_tick.h)
__device__ __forceinline__ void observe_role(const KernelArgs& a, const int block, const bool own_box, const bool pooled = false) {
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
    const int mission = mission_row(a, env, slot, pooled);
    if (c.via_max > 0 && a.vias != nullptr) {
      const int via_row = mission;
      const int v_a = a.via_slot_off[via_row], v_b = a.via_slot_off[via_row + 1];
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
    const bool fixed_route = route.fixed_route(a.missions, mission, m.n_roads);
    bool reached_goal = false;
    if (fixed_route) {
      const double gx = a.missions.goal[3 * mission], gy = a.missions.goal[3 * mission + 1], gr = a.missions.goal[3 * mission + 2];
      const double sqr_dist = (s.x - gx) * (s.x - gx) + (s.y - gy) * (s.y - gy);
      reached_goal = sqr_dist <= gr * gr;
    }
    // (a lap goal's distance condition waits for this tick's trip meter, which the waypoints role is still writing:
    // the commit role applies it, lap_goal_gate)
    if (__builtin_expect(a.missions.goal_kind != nullptr, 0) && a.missions.goal_kind[mission].kind == SMX_GOAL_TRAVERSE)
      reached_goal = drove_off_map(a.missions, m, pooled ? a.missions.n + 1 : n_veh, OWN_BOX ? ego_lane : my_lane, my_lane_dist, s.x, s.y, wrap_heading(s.heading));
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
__device__ __forceinline__ void commit_role(const KernelArgs& a, const int block, const bool tick, const bool pooled = false) {
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
    if (__builtin_expect(a.missions.goal_kind != nullptr, 0)) lap_goal_gate(a, gid, total, mission_row(a, env, slot, pooled), tick);
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
__device__ __forceinline__ void sensors_roles(const KernelArgs& a, const bool pooled = false) {
  const int b = (int)blockIdx.x;
  if (b < a.wp_blocks) {
    waypoints_role(a, b, pooled);
  } else if (b < a.wp_blocks + a.obs_blocks) {
    observe_role(a, b - a.wp_blocks, SIZED != 0, pooled);
  } else if (b < a.wp_blocks + a.obs_blocks + a.lidar_blocks) {
    lidar_role<-1>(a, b - a.wp_blocks - a.obs_blocks);
  } else {
    ogm_role(a, b - a.wp_blocks - a.obs_blocks - a.lidar_blocks);
  }
}
__global__ void __launch_bounds__(SMX_BLOCK) k_sensors(const KernelArgs a) { sensors_roles<0>(a); }
__global__ void __launch_bounds__(SMX_BLOCK) k_sensors_sized(const KernelArgs a) { sensors_roles<1>(a); }
// (... their pool instances, TickPlan::pool)
__global__ void __launch_bounds__(SMX_BLOCK) k_sensors_pool(const KernelArgs a) { sensors_roles<0>(a, true); }
__global__ void __launch_bounds__(SMX_BLOCK) k_sensors_sized_pool(const KernelArgs a) { sensors_roles<1>(a, true); }

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
__device__ __forceinline__ void first_role(const KernelArgs& a, const int block, const bool pooled = false) {
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
          if ((flags & SMX_F_ALIVE) && (flags & SMX_F_FIRST)) scan_role<SMX_TEAM, true, SIZED>(a, m, c, gid, total, team_rank<SMX_TEAM>(), flags, half, pooled);
        }
      }
    } else if (turn == 1 && threadIdx.x < SMX_FIRST_WP_THREADS) {  // (whole wavefronts; waypoints_for holds no barrier)
      for (size_t base = g0; base < g1; base += SMX_FIRST_WP_THREADS / SMX_WP_LANES) {
        const size_t gid = base + threadIdx.x / SMX_WP_LANES;
        if (gid < g1) waypoints_for<SMX_FIRST_WP_THREADS>(a, gid, knot_scratch + threadIdx.x, pooled);
      }
    }
    __threadfence();
    __syncthreads();
    SMX_TSTAMP(tt1);
    SMX_TACC_ALL(turn == 0 ? 57 : 58, tt0, tt1);
  }
  SMX_TSTAMP(tk2);
  observe_role(a, block, SIZED != 0, pooled);
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
  commit_role<false>(a, block, false, pooled);  // (the reset pass's commit has no guard work: respawn_vehicle wrote the bytes)
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
// (... their pool instances, TickPlan::pool)
__global__ void __launch_bounds__(SMX_FIRST_BLOCK) k_first_pool(const KernelArgs a, const int32_t* groups, const int32_t* n_groups) {
  if ((int)blockIdx.x >= *n_groups) return;
  first_role<0>(a, groups[blockIdx.x], true);
}
__global__ void __launch_bounds__(SMX_FIRST_BLOCK) k_first_sized_pool(const KernelArgs a, const int32_t* groups, const int32_t* n_groups) {
  if ((int)blockIdx.x >= *n_groups) return;
  first_role<1>(a, groups[blockIdx.x], true);
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

__device__ __forceinline__ void road_waypoints_role(const KernelArgs& a, const bool pooled) {
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
    f.fixed_route(a.missions, mission_row(a, gid, pooled), m.n_roads);
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
__global__ void __launch_bounds__(SMX_BLOCK) k_road_waypoints(const KernelArgs a) { road_waypoints_role(a, false); }
// (... its pool instance, TickPlan::pool)
__global__ void __launch_bounds__(SMX_BLOCK) k_road_waypoints_pool(const KernelArgs a) { road_waypoints_role(a, true); }

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

template <bool GUARD>
__device__ __forceinline__ void tail_role(const KernelArgs& a, const TailArgs& t, const bool pooled) {
  const smx_config& c = a.cfg;
  const int block = (int)blockIdx.x;
  const int n_veh = c.num_vehicles;
  const int epb = SMX_BLOCK / n_veh;
  const size_t total = (size_t)c.num_envs * n_veh;
  const size_t g0 = (size_t)block * epb * n_veh;
  const size_t g1 = min(total, g0 + (size_t)epb * n_veh);
  const int lane = (int)threadIdx.x;
  const size_t gid = g0 + lane;
  if (t.commit) commit_role<GUARD>(a, block, true, pooled);  // (lane l commits vehicle g0 + l: its flags word is read back below)
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
template <bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_tail(const KernelArgs a, const TailArgs t) { tail_role<GUARD>(a, t, false); }
// (... its pool instance, TickPlan::pool: the lap gate of the tick's commit reads the mission through the pool's table)
template <bool GUARD = false>
__global__ void __launch_bounds__(SMX_BLOCK) k_tail_pool(const KernelArgs a, const TailArgs t) { tail_role<GUARD>(a, t, true); }
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
// (... their pool instances, TickPlan::pool)
__global__ void __launch_bounds__(SMX_BLOCK) k_observe_pool(const KernelArgs a) { observe_role(a, (int)blockIdx.x, false, true); }
__global__ void __launch_bounds__(SMX_BLOCK) k_observe_sized_pool(const KernelArgs a) { observe_role(a, (int)blockIdx.x, true, true); }

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
  in.routed = h->missions.route_last != nullptr;  // (a mission pool: some pool entry has a fixed route)
  in.pool_bound = h->missions.rows != nullptr;
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

extern "C" int smx_set_mission_pool(smx_handle h, const smx_mission_pool* pool) { return set_mission_pool_impl(h, pool); }

extern "C" int smx_check_mission_pool(const smx_config* cfg, const smx_map_tables* map, const smx_mission_pool* pool, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && map && pool) ? check_mission_pool_impl(*cfg, *map, *pool, msg) : refuse(msg, "null config, map or pool");
  return report(rc, msg, err, err_len);
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
// A kernel that reads a per-mission table has a pool instance (TickPlan::pool): the steps below name the kernel as they
// always have, and while a pool is bound — a.missions.rows, which is what PlanInputs::pool_bound was read from — its
// instance is launched in its place.  Kernels without such a site have none and are launched as they are.
static Kernel pool_instance(Kernel k) {
  static const struct { Kernel plain, pool; } twins[] = {
      {k_scan<true, true>, k_scan_pool<true>}, {k_scan<false, true>, k_scan_pool<false>},
      {k_scan_half<1, true>, k_scan_half_pool<false>}, {k_scan_half<1, true, SMX_TEAM_LARGE, true>, k_scan_half_pool<true>},
      {k_sensors, k_sensors_pool}, {k_sensors_sized, k_sensors_sized_pool}, {k_observe, k_observe_pool}, {k_observe_sized, k_observe_sized_pool},
      {k_waypoints, k_waypoints_pool}, {k_waypoints_tables, k_waypoints_tables_pool}, {k_waypoints_emit, k_waypoints_emit_pool},
      {k_waypoints_listed, k_waypoints_listed_pool}, {k_waypoints_walk_listed, k_waypoints_walk_listed_pool},
      {k_road_waypoints, k_road_waypoints_pool}};
  for (const auto& t : twins)
    if (t.plain == k) return t.pool;
  return k;
}
static void launch(Kernel k, unsigned blocks, size_t lds, hipStream_t s, const KernelArgs& a) {
  hipLaunchKernelGGL(a.missions.rows != nullptr ? pool_instance(k) : k, dim3(blocks), dim3(SMX_BLOCK), lds, s, a);
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
  hipLaunchKernelGGL(p.pool ? (p.guard ? k_tail_pool<true> : k_tail_pool<false>) : (p.guard ? k_tail<true> : k_tail<false>), dim3(p.obs_blocks), dim3(SMX_BLOCK), p.tail_grids ? std::max({p.ogm_bytes, p.dagm_bytes, p.rgb_lds}) : 0, stream, r, t);
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
    hipLaunchKernelGGL(p.pool ? (p.sized ? k_first_sized_pool : k_first_pool) : (p.sized ? k_first_sized : k_first), dim3(p.obs_blocks), dim3(SMX_FIRST_BLOCK), 0, stream, r, t.groups, t.n_groups);
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
      if (bits & SMX_DEVICE_BAD_MISSION_ROW)
        return fail(h, SMX_ERR_INVALID,
                    "an entry outside -1 .. n_missions - 1 was read from the table of the mission pool (smx_set_mission_pool) "
                    "since the last smx_sync; the agents it stood for had an endless mission, as for -1");
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

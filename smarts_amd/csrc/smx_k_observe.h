// smx_k_observe.h — the observe role and its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_device.h"
#include "smx_plan.h"
#include "smx_roadmap.h"
#include "smx_scan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

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

// smx_k_pass.h — what strings a pass together: the alive list, the commit role, k_sensors, k_first, k_tail and k_reset.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_device.h"
#include "smx_handle.h"
#include "smx_k_grids.h"
#include "smx_k_lidar.h"
#include "smx_k_observe.h"
#include "smx_k_scan.h"
#include "smx_k_waypoints.h"
#include "smx_plan.h"
#include "smx_roadmap.h"
#include "smx_scan.h"
#include "smx_tick.h"

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

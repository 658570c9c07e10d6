// smx_k_entry.h — delayed agent entry (smx_set_agent_entry): the pass that lets pending agents enter, k_entry.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_k_scan.h"
#include "smx_plan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

// =================================================================================
// k_entry: TrapManager.step for traps without a capture zone (trap_manager.py:121-241), in the tick's place of it —
// after the providers stepped (the control phase has moved every social slot) and before the sensors observe
// (smarts.py:259-301).  One wavefront per env; the plan launches it only while a table is bound, after the control
// phase and ahead of the observation pass.
// For each pending agent of the env, in slot order, whose ready tick has come (the tick this pass produces, counted from
// the reset observation, is at least its row of the table): the patience has expired (the host folded the countdown into
// the ready tick, smarts_amd.missions.entry_ticks), so the agent is blocked when any alive social slot of the env lies
// within (0.5 * (largest plane dimension of the slot + that of the new vehicle)) of the mission's start point
// (:212-226: squared_dist against the squared half-sum, float64; agents are not checked, so two entrants may overlap),
// else it enters — respawn_vehicle for that agent alone, exactly as a reset creates it, SMX_F_ALIVE | SMX_F_FIRST, so
// that this tick's observation pass gives it a first observation and its mates see it.  A blocked agent tries again in
// the next tick.  The lanes stride over the env's social slots (their state words are SoA: the loads of a step
// coalesce) and a ballot decides; no LDS, no atomics.
// FACTS (the large forms): the tick's facts half runs over the alive list built a tick ahead, which does not hold the
// entrant, and its mates' observe role reads the entrant's nearest lane and distance (nb_lane_id / nb_lane_index) from
// its road facts.  So the first team of the wavefront runs the facts half for the entrant here, from scratch (its
// SMX_F_FIRST), as the small form's k_scan does with a team of the same width.
// =================================================================================
template <bool GUARD, bool FACTS>
__global__ void __launch_bounds__(64) k_entry(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const int env = (int)blockIdx.x;
  const int lane = (int)threadIdx.x;
  if (env >= c.num_envs) return;
  const int n_veh = c.num_vehicles, n_agents = n_veh - c.num_social, rows = a.entry.rows;
  const size_t total = (size_t)c.num_envs * n_veh;
  const size_t g0 = (size_t)env * n_veh;
  const int episode = a.st.env_episode[env];
  const size_t row = (size_t)(((episode % rows) + rows) % rows);
  const size_t cell0 = (row * (size_t)c.num_envs + (size_t)env) * (size_t)n_agents;
  // the tick this pass produces: the commit that ends it makes env_ticks reset_elapsed_steps + tick
  const int tick = a.st.env_ticks[env] + 1 - c.reset_elapsed_steps;
  const bool sized = dims_sized(a);
  for (int k = 0; k < n_agents; ++k) {  // (uniform)
    const size_t gid = g0 + (size_t)k;
    // (pending: not ENTERED by this episode's respawn, and no vehicle — the binding holds steps until a reset has written
    // every status byte, smx_handle.h entry_reset_needed)
    if (a.entry.status[gid] == SMX_ENTRY_ENTERED || (a.st.flags[gid] & SMX_F_ALIVE)) continue;
    if (tick < a.entry.ready[cell0 + (size_t)k]) continue;
    const double* q = a.entry.check + (cell0 + (size_t)k) * 3;
    const double cx = q[0], cy = q[1], own = q[2];
    bool hit = false;
    for (int s = lane; s < c.num_social; s += 64) {
      const size_t g = g0 + (size_t)(n_agents + s);
      if (!(a.st.flags[g] & SMX_F_ALIVE)) continue;
      const VehBox b = vehicle_box(a, g, sized);
      const double largest = fmax(b.length, b.width);
      const double dx = a.st.f64[(size_t)SMX_S_X * total + g] - cx;
      const double dy = a.st.f64[(size_t)SMX_S_Y * total + g] - cy;
      const double r = 0.5 * (largest + own);
      if (dx * dx + dy * dy <= r * r) hit = true;
    }
    if (__ballot(hit) != 0ull) {
      if (lane == 0) a.entry.status[gid] = (uint8_t)SMX_ENTRY_BLOCKED;
      continue;
    }
    if (lane == 0) {
      respawn_vehicle<GUARD, -1, 0>(a, gid, total, episode);  // (a reset's, without the branch that makes it pending)
      a.st.flags[gid] = a.st.flags[gid] | SMX_F_ENTERING;  // (its first observation runs its collision test)
      a.entry.status[gid] = (uint8_t)SMX_ENTRY_ENTERED;
      a.entry.entered[gid] = tick;
    }
    if constexpr (FACTS) {
      __syncthreads();  // (the respawned state, written by lane 0, for the team's loads; the loop is uniform)
      const int f = a.st.flags[gid];
      if (lane < SMX_TEAM) scan_role<SMX_TEAM, false>(a, a.map, c, gid, total, lane, f, 0);
    }
  }
}

// =================================================================================
// k_entry_first: the large forms' half of an entrant's first observation.  Their tick runs the scan, waypoint and
// control kernels over the alive list built a tick ahead, which does not hold this tick's entrants: the tick's pass lets
// the mates see an entrant (the per-env and per-vehicle grid, lidar and observe launches read every slot's pose) but
// cannot observe it.  After the tick's commit this kernel gives each agent that entered in this tick (ENTERED, its tick
// the env's, still alive) SMX_F_FIRST | SMX_F_ENTERING again and lists its env group for the reset pass — the same
// first_only pass a restart inside the tick uses (k_first, k_lidar_first, the first lane-TTC and ego-frame passes) —
// unless k_tail listed the group already (it has a new vehicle of a restart).  That pass observes the entrant from
// scratch and its commit counts it.  One workgroup per env group of the observe / commit roles (<= 64 vehicles: one
// wavefront), the tail's list counter; the plan launches it in a large form's tick with a table bound.
// =================================================================================
__global__ void __launch_bounds__(SMX_BLOCK) k_entry_first(const KernelArgs a, int32_t* groups, int32_t* n_groups) {
  const smx_config& c = a.cfg;
  const int block = (int)blockIdx.x;
  const int n_veh = c.num_vehicles, n_agents = n_veh - c.num_social;
  const int epb = SMX_BLOCK / n_veh;
  const size_t total = (size_t)c.num_envs * n_veh;
  const size_t g0 = (size_t)block * epb * n_veh;
  const size_t g1 = min(total, g0 + (size_t)epb * n_veh);
  const size_t gid = g0 + threadIdx.x;
  int f = 0;
  bool entrant = false;
  if (gid < g1) {
    f = a.st.flags[gid];
    const int env = (int)(gid / (size_t)n_veh);
    const int slot = (int)(gid - (size_t)env * n_veh);
    const int tick = a.st.env_ticks[env] - c.reset_elapsed_steps;  // (after the commit: this tick's number)
    entrant = slot < n_agents && tick > 0 && (f & SMX_F_ALIVE) && a.entry.status[gid] == SMX_ENTRY_ENTERED &&
              a.entry.entered[gid] == tick;
  }
  const bool listed = __ballot((f & SMX_F_ALIVE) && (f & SMX_F_FIRST)) != 0ull;  // (k_tail's rule: uniform)
  const unsigned long long mark = __ballot(entrant);
  if (entrant) {
    a.st.flags[gid] = f | SMX_F_FIRST | SMX_F_ENTERING;
    // the tick's pass pushed one accelerometer sample (observe role: LV1 <- LV0, LV0 <- this one); the reset pass pushes
    // the first observation's again, so the sample before it goes back to what the respawn left, as after a reset
    if (c.sensors & SMX_SENSOR_ACCELEROMETER)
      for (int w = 0; w < 3; ++w) a.st.f64[(size_t)(SMX_S_LV0_LONG + w) * total + gid] = a.st.f64[(size_t)(SMX_S_LV1_LONG + w) * total + gid];
  }
  if (mark != 0ull && !listed && threadIdx.x == 0) groups[atomicAdd(n_groups, 1)] = block;
}

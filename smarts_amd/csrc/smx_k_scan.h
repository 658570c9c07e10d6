// smx_k_scan.h — the scan phase: k_scan's map sweeps at the new pose and its listed forms.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_plan.h"
#include "smx_scan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

// =================================================================================
// k_scan: map sweeps at the vehicle's pose, SMX_TEAM lanes per vehicle.
//   facts: nearest lane + distance (nearest_lane with any radius up to 10 m is "that lane if
//          closer than r": ego lane sensors.py:277, neighbour lanes :244, off-route :552),
//          road_with_point at the centre (:498-500) and at the four bounding-box corners
//          (:502-509; Vehicle.bounding_box vehicle.py:315-332, rotate_around_point math.py:436-444)
//   seeds: start road / route filter / start lanepoints of waypoint_paths(pose, route)
//          (sumo_road_network.py:815-882), used by the waypoints role now and by k_control next tick
// =================================================================================
// one half of k_scan for one vehicle team (see k_scan)
template <int TEAM, bool ROUTED, int SIZED = -1>
__device__ __forceinline__ void scan_role(const KernelArgs& a, const MapDev& m, const smx_config& c, size_t gid,
                                          size_t total, int rank, int flags, int role, const bool pooled = false) {
  SMX_TSTAMP(ts0);
  const VehState s = load_vehicle(a, gid, total);
  int32_t* fi = a.st.facts_i32;
  if (SMX_SKIP(a, 512) && role == 1) return;
  if (SMX_SKIP(a, 1024) && role == 0) return;
  if (role == 0) {
    // ---- road facts
    const double cxs[4] = {-0.5, 0.5, 0.5, -0.5};
    const double cys[4] = {0.5, 0.5, -0.5, -0.5};
    double cx[4], cy[4];
    const double ch = cos(s.heading), sh = sin(s.heading);
    const bool social = (flags & SMX_F_SOCIAL) != 0;  // only its nearest lane is ever asked for (neighbour rows)
    // the observer's own box (sensors.py:506): the sedan's, or with dimensions bound an agent's triple and its reaches
    ObserverBox ob = {SMX_CHASSIS_LENGTH, SMX_CHASSIS_WIDTH, 2.0, SMX_POSE_SCAN_RADIUS};
    if (own_box_sized<SIZED>(a) && !social) ob = observer_box(a, gid, a.dagm_reach + 0.1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double qx = s.x + cxs[q] * ob.width;
      double qy = s.y + cys[q] * ob.length;
      cx[q] = s.x + ch * (qx - s.x) + sh * (qy - s.y);
      cy[q] = s.y + -sh * (qx - s.x) + ch * (qy - s.y);
    }
    FactsCarry fc;
    fc.valid = false;
    if (a.facts_carry != nullptr && !(flags & SMX_F_FIRST)) {
      fc.qx = a.facts_carry[gid];
      fc.qy = a.facts_carry[total + gid];
      fc.prev_dist = a.st.facts_f64[(size_t)SMX_FF_LANE_DIST * total + gid];
      fc.valid = fi[(size_t)SMX_FI_LANE * total + gid] >= 0;
    }
    RoadFacts h = team_road_facts_seeded<TEAM>(m, s.x, s.y, ob.scan_radius, social ? 0 : 4, cx, cy, fc, a.dagm_reach + 0.1, ob.corner_reach);
    if (a.facts_carry != nullptr && rank == 0) {
      a.facts_carry[gid] = s.x;
      a.facts_carry[total + gid] = s.y;
    }
    SMX_TSTAMP(ts1);
    SMX_TACC(10, ts0, ts1);
    // wrong-way test input (sensors.py:556-562, 581-586): the lane heading at the point of the
    // nearest lane closest to the vehicle; junction lanes are exempt (:548-551)
    double lane_heading = 0.0;
    if (SMX_SKIP(a, 2048)) return;
    const bool want_heading = !social && h.lane >= 0 && !m.lane_in_junction[h.lane] && !SMX_SKIP(a, 64);  // uniform in the team
    if (want_heading) lane_heading = team_lane_heading_at_point<TEAM>(m, h.lane, s.x, s.y, h.dist);
    SMX_TSTAMP(ts2);
    SMX_TACC(11, ts1, ts2);
    if (rank == 0) {
      fi[(size_t)SMX_FI_LANE * total + gid] = h.lane;
      fi[(size_t)SMX_FI_FLAGS * total + gid] =
          (h.on_road ? SMX_FACT_ON_ROAD : 0) | ((h.corner_mask & 15) << SMX_FACT_CORNER_SHIFT);
      a.st.facts_f64[(size_t)SMX_FF_LANE_DIST * total + gid] = h.dist;
      a.st.facts_f64[(size_t)SMX_FF_LANE_HEADING * total + gid] = lane_heading;
    }
    return;
  }
  // ---- path seeds
  if (flags & SMX_F_SOCIAL) return;
  SMX_TSTAMP(ts3);
  Top10 t;
  LaneGuess guess;
  SeedsCarry scy;
  scy.valid = false;
  if (a.seeds_carry != nullptr && !(flags & SMX_F_FIRST)) {
    const int32_t* sc_ = a.st.seed_cache;
    scy.qx = a.seeds_carry[gid];
    scy.qy = a.seeds_carry[total + gid];
    scy.d10 = a.seeds_carry[2 * total + gid];
    scy.d1 = a.seeds_carry[3 * total + gid];
    scy.prev_road = sc_[0 * total + gid];
    scy.prev_lanes = sc_[4 * total + gid];
#pragma unroll
    for (int q = 0; q < SMX_SEED_LANES; ++q) scy.prev_start[q] = sc_[(size_t)(5 + q) * total + gid];
    scy.valid = true;
  }
  const bool wp_on = (c.sensors & SMX_SENSOR_WAYPOINTS) != 0;
  team_nearest10_carried<TEAM>(m, s.x, s.y, scy, t, guess);
  if (a.seeds_carry != nullptr && rank == 0) {
    a.seeds_carry[gid] = s.x;
    a.seeds_carry[total + gid] = s.y;
    a.seeds_carry[2 * total + gid] = t.idx[9] >= 0 ? t.d2[9] : -1.0;
    a.seeds_carry[3 * total + gid] = t.idx[0] >= 0 ? t.d2[0] : -1.0;
  }
  SMX_TSTAMP(ts4);
  SMX_TACC(12, ts3, ts4);
  // what the controller (and the waypoints sensor) ask: paths at this pose with the agent's route
  if (SMX_SKIP(a, 4096)) return;
  Top10Scores sc;
  if (SMX_SKIP(a, 256)) {
#pragma unroll
    for (int k = 0; k < 10; ++k) sc.rel[k] = 0.0;
  } else {
    sc = team_top10_heading_terms<TEAM>(m, t, s.heading);
  }
  SMX_TSTAMP(ts4b);
  SMX_TACC(9, ts4, ts4b);
  const PathSeeds seed = team_compute_path_seeds<TEAM, ROUTED>(m, s.x, s.y, s.heading, 5.0, true, t, sc, a.missions, ROUTED ? mission_row(a, gid, pooled) : 0, &guess);
  // without the waypoints sensor the observation still takes the first waypoint of
  // waypoint_paths(pose, lookahead=1, within_radius=length) for the trip meter (sensors.py:270-275,
  // 349-351); TripMeterSensor.__init__ (sensors.py:885-898) asks the same on a new vehicle
  int obs_start = -1, trip_start = -1;
  if (!wp_on || (flags & SMX_F_FIRST)) {
    // (within_radius = the vehicle's length, sensors.py:895: with dimensions bound the agent's own)
    const double own_length = own_box_sized<SIZED>(a) ? vehicle_box(a, gid, true).length : SMX_CHASSIS_LENGTH;
    const PathSeeds ts = team_compute_path_seeds<TEAM, false>(m, s.x, s.y, s.heading, own_length, false, t, sc, a.missions, 0, &guess);
    trip_start = (ts.road >= 0) ? ts.start[0] : -1;
    obs_start = trip_start;
  }
  SMX_TSTAMP(ts5);
  SMX_TACC(13, ts4, ts5);
  if (rank == 0) {
    store_seeds(a, gid, total, seed);
    fi[(size_t)SMX_FI_TRIP_START * total + gid] = (flags & SMX_F_FIRST) ? trip_start : -1;
    fi[(size_t)SMX_FI_OBS_START * total + gid] = obs_start;
  }
  SMX_TSTAMP(ts6);
  SMX_TACC(14, ts0, ts6);
}

// Register budgets (amdgpu_waves_per_eu): the split form runs on small batches, where at most two or
// three wavefronts per SIMD exist anyway, and takes the ~160 registers it wants — capped at 128 it
// spilled 136 B per lane and cost 10 us of 48 at 8 k vehicles, plus 9 MB of scratch write-back per
// tick.  The back-to-back form (large batches) is capped at 128 registers: four wavefronts per
// SIMD; five (96 registers, 276 B of spills) was 1.5x slower at 131 k vehicles.
#ifndef SMX_SCAN_WAVES
#define SMX_SCAN_WAVES 3
#endif
// ROUTED: the instance that knows fixed routes (smx_set_missions); batches without missions run the other one
template <bool SPLIT, bool ROUTED = false>
__global__ void __attribute__((amdgpu_waves_per_eu(SPLIT ? 2 : SMX_SCAN_WAVES, 8))) __launch_bounds__(SMX_BLOCK) k_scan(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  // the two halves of the scan are independent: on small batches they run as different workgroups
  // of one launch (even: road facts + lane heading, odd: lanepoint search + path seeds) and
  // overlap in time; on large ones every workgroup does both, one after the other
  const size_t gid = ((size_t)(SPLIT ? (blockIdx.x >> 1) : blockIdx.x) * SMX_BLOCK + threadIdx.x) / SMX_TEAM;
  const int rank = team_rank<SMX_TEAM>();
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE)) return;
  if (a.first_only && !(flags & SMX_F_FIRST)) return;
  if (SPLIT) {
    if (blockIdx.x & 1)
      scan_role<SMX_TEAM, ROUTED>(a, m, c, gid, total, rank, flags, 1);
    else
      scan_role<SMX_TEAM, ROUTED>(a, m, c, gid, total, rank, flags, 0);
  } else {
    scan_role<SMX_TEAM, ROUTED>(a, m, c, gid, total, rank, flags, 0);
    scan_role<SMX_TEAM, ROUTED>(a, m, c, gid, total, rank, flags, 1);
  }
}

// (... its pool instances, TickPlan::pool: the routed scan with the mission read through the pool's table)
template <bool SPLIT>
__global__ void __attribute__((amdgpu_waves_per_eu(SPLIT ? 2 : SMX_SCAN_WAVES, 8))) __launch_bounds__(SMX_BLOCK) k_scan_pool(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = ((size_t)(SPLIT ? (blockIdx.x >> 1) : blockIdx.x) * SMX_BLOCK + threadIdx.x) / SMX_TEAM;
  const int rank = team_rank<SMX_TEAM>();
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE)) return;
  if (a.first_only && !(flags & SMX_F_FIRST)) return;
  if (SPLIT) {
    scan_role<SMX_TEAM, true>(a, m, c, gid, total, rank, flags, (blockIdx.x & 1) ? 1 : 0, true);
  } else {
    scan_role<SMX_TEAM, true>(a, m, c, gid, total, rank, flags, 0, true);
    scan_role<SMX_TEAM, true>(a, m, c, gid, total, rank, flags, 1, true);
  }
}

// One half of the scan as a launch of its own (large batches): the road facts feed the observe role only and
// the path seeds the waypoint kernels only, so the two go to different streams and each keeps the registers
// it needs (the facts half alone fits more wavefronts per SIMD than the pair).
// (TEAM: four lanes a vehicle when the batch fills the chip, eight up to SMX_SCAN_WIDE_MAX_VEHICLES on maps whose lanes
// split: a quarter-full chip is bound by one team's latency, and the wider team's is the shorter)
// (SIZED: per-agent dimensions, TickPlan::sized — the agent's own box in the corners, the reaches and the trip meter's lookup)
template <int ROLE, bool ROUTED = false, int TEAM = SMX_TEAM_LARGE, bool SIZED = false>
__global__ void __attribute__((amdgpu_waves_per_eu(ROLE == 0 ? 4 : 3, 8))) __launch_bounds__(SMX_BLOCK) k_scan_half(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = launch_vehicle(a, ((size_t)blockIdx.x * SMX_BLOCK + threadIdx.x) / TEAM, total);
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE)) return;
  if (a.first_only && !(flags & SMX_F_FIRST)) return;
  scan_role<TEAM, ROUTED, SIZED ? 1 : 0>(a, a.map, c, gid, total, team_rank<TEAM>(), flags, ROLE);
}
// (... the seeds half's pool instance, TickPlan::pool)
template <bool SIZED = false>
__global__ void __attribute__((amdgpu_waves_per_eu(3, 8))) __launch_bounds__(SMX_BLOCK) k_scan_half_pool(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = launch_vehicle(a, ((size_t)blockIdx.x * SMX_BLOCK + threadIdx.x) / SMX_TEAM_LARGE, total);
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  if (!(flags & SMX_F_ALIVE)) return;
  if (a.first_only && !(flags & SMX_F_FIRST)) return;
  scan_role<SMX_TEAM_LARGE, true, SIZED ? 1 : 0>(a, a.map, c, gid, total, team_rank<SMX_TEAM_LARGE>(), flags, 1, true);
}

// k_scan_fast (large batches): one half of the scan with ONE lane per vehicle (smx_scan.h facts_one_lane /
// seeds_one_lane: searches seeded from last tick's answers, two passes over per-lane candidate lists).  A vehicle it
// cannot serve — no usable carry, a list overflow, the in-junction rule, stacked lanes — is appended to the slow list
// and served by k_scan_half's teams afterwards: one such vehicle would otherwise hold its whole wavefront for the
// length of the searches from scratch.
template <int ROLE>
__global__ void __launch_bounds__(SMX_BLOCK) k_scan_fast(const KernelArgs a) {
  SMX_TSTAMP(span0);
  __shared__ int cand_lds[(ROLE == 0 ? SMX_FACTS_CAND : SMX_SEEDS_CAND) * SMX_BLOCK];
  const smx_config& c = a.cfg;
  const MapDev& m = a.map;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = launch_vehicle(a, (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x, total);
  bool slow = false;
  // every word whose address only needs the vehicle is loaded here, together and whatever the flags say (one round
  // trip instead of flags -> pose -> carry one behind the other: two wavefronts per SIMD hide nothing)
  const bool in_range = gid < total;
  const size_t g = in_range ? gid : 0;
  const int flags = a.st.flags[g];
  const double sx_ = a.st.f64[(size_t)SMX_S_X * total + g], sy_ = a.st.f64[(size_t)SMX_S_Y * total + g],
               sh_ = a.st.f64[(size_t)SMX_S_HEADING * total + g];
  int32_t* fi = a.st.facts_i32;
  FactsCarry fc;
  SeedsCarry scy;
  fc.valid = false;
  scy.valid = false;
  int prev_lane = -1;
  if (ROLE == 0) {
    fc.qx = a.facts_carry[g];
    fc.qy = a.facts_carry[total + g];
    fc.prev_dist = a.st.facts_f64[(size_t)SMX_FF_LANE_DIST * total + g];
    prev_lane = fi[(size_t)SMX_FI_LANE * total + g];
  } else {
    const int32_t* sc_ = a.st.seed_cache;
    scy.qx = a.seeds_carry[g];
    scy.qy = a.seeds_carry[total + g];
    scy.d10 = a.seeds_carry[2 * total + g];
    scy.d1 = a.seeds_carry[3 * total + g];
    scy.prev_road = sc_[0 * total + g];
    scy.prev_lanes = sc_[4 * total + g];
#pragma unroll
    for (int q = 0; q < SMX_SEED_LANES; ++q) scy.prev_start[q] = sc_[(size_t)(5 + q) * total + g];
  }
  if (in_range && (flags & SMX_F_ALIVE) && (!a.first_only || (flags & SMX_F_FIRST))) {
    int* cand = cand_lds + threadIdx.x;
    const bool seeded = !(flags & SMX_F_FIRST);
    if (ROLE == 0) {
      const double cxs[4] = {-0.5, 0.5, 0.5, -0.5};
      const double cys[4] = {0.5, 0.5, -0.5, -0.5};
      double cx[4], cy[4];
      const double ch = cos(sh_), sh = sin(sh_);
      const bool social = (flags & SMX_F_SOCIAL) != 0;
      // (the observer's own box: as in scan_role)
      ObserverBox ob = {SMX_CHASSIS_LENGTH, SMX_CHASSIS_WIDTH, 2.0, SMX_POSE_SCAN_RADIUS};
      if (dims_sized(a) && !social) ob = observer_box(a, gid, a.dagm_reach + 0.1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double qx = sx_ + cxs[q] * ob.width;
        double qy = sy_ + cys[q] * ob.length;
        cx[q] = sx_ + ch * (qx - sx_) + sh * (qy - sy_);
        cy[q] = sy_ + -sh * (qx - sx_) + ch * (qy - sy_);
      }
      fc.valid = seeded && prev_lane >= 0;
      RoadFacts h;
      double lane_heading = 0.0;
      bool served;
      if (SMX_SKIP(a, 1 << 23)) {  // (developer ablation: the prologue and the stores only)
        h.lane = prev_lane;
        h.dist = fc.prev_dist + cx[0] * 1e-30;
        h.on_road = true;
        h.corner_mask = 15;
        served = true;
      } else {
        served = facts_one_lane(m, sx_, sy_, ob.scan_radius, social ? 0 : 4, cx, cy, fc, a.dagm_reach + 0.1, cand, SMX_BLOCK,
                                !social, h, lane_heading, ob.corner_reach);
      }
      if (served) {
        a.facts_carry[gid] = sx_;
        a.facts_carry[total + gid] = sy_;
        fi[(size_t)SMX_FI_LANE * total + gid] = h.lane;
        fi[(size_t)SMX_FI_FLAGS * total + gid] =
            (h.on_road ? SMX_FACT_ON_ROAD : 0) | ((h.corner_mask & 15) << SMX_FACT_CORNER_SHIFT);
        a.st.facts_f64[(size_t)SMX_FF_LANE_DIST * total + gid] = h.dist;
        a.st.facts_f64[(size_t)SMX_FF_LANE_HEADING * total + gid] = lane_heading;
      } else {
        slow = true;
      }
    } else if (!(flags & SMX_F_SOCIAL)) {
      scy.valid = seeded;
      PathSeeds one;
      double d1sq = -1.0;
      if (seeds_one_lane(m, sx_, sy_, sh_, 5.0, scy, cand, SMX_BLOCK, one, d1sq)) {
        a.seeds_carry[gid] = sx_;
        a.seeds_carry[total + gid] = sy_;
        a.seeds_carry[2 * total + gid] = -1.0;  // (the tenth nearest was not looked for)
        a.seeds_carry[3 * total + gid] = d1sq;
        store_seeds(a, gid, total, one);
        fi[(size_t)SMX_FI_TRIP_START * total + gid] = -1;  // (only a new vehicle or a batch without the waypoints
        fi[(size_t)SMX_FI_OBS_START * total + gid] = -1;   //  sensor asks these: neither comes here)
      } else {
        // its seeds, walks and rows are the slow chain's (k_scan_listed -> k_waypoints_listed, beside the tick's main
        // chain): k_wp_walk and k_waypoints_emit pass over the vehicle
        slow = true;
      }
      if (a.seed_pending != nullptr) a.seed_pending[gid] = slow ? 1 : 0;
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
  SMX_TSPAN(ROLE == 1 ? 1 : 2, span0, span1);
}

// k_scan_half over a list whose length is only known on the device (the slow list): a fixed grid, teams striding it
// (TEAM: four lanes a vehicle where the lists are long — maps whose lanes split —, eight where they hold a few
// hundred vehicles and the kernel is one team's latency at the end of the slow chain: 70 against 55 us)
template <int ROLE, bool ROUTED = false, int TEAM = SMX_TEAM_LARGE, bool SIZED = false>
__global__ void __attribute__((amdgpu_waves_per_eu(ROLE == 0 ? 4 : 3, 8))) __launch_bounds__(SMX_BLOCK) k_scan_listed(const KernelArgs a) {
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const int count = *a.slow_count;
  constexpr int VPB = SMX_BLOCK / TEAM;
  for (int i = (int)blockIdx.x * VPB + (int)threadIdx.x / TEAM; i < count; i += (int)gridDim.x * VPB) {
    const size_t gid = (size_t)a.slow_list[i];
    const int flags = a.st.flags[gid];
    scan_role<TEAM, ROUTED, SIZED ? 1 : 0>(a, a.map, c, gid, total, team_rank<TEAM>(), flags, ROLE);
  }
}


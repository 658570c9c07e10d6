// smx_tick.h — what every phase of a tick shares: the kernels' argument block, vehicle load / store, replay, guard and respawn steps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_guard.h"
#include "smx_handle.h"
#include "smx_history.h"
#include "smx_scan.h"
#include "smx_vehicle.h"

#define SMX_COLLISION_LEEWAY 0.05  // chassis.py:75-78
#define SMX_POSE_SCAN_RADIUS 10.0
#define SMX_WPT_PRELOAD 8           // knots of a path held in registers while it is interpolated
#define SMX_SLOW_BLOCKS 512          // workgroups of the slow lists' kernels on a map without junctions (smx_load_map: slow_blocks)

struct KernelArgs {
  smx_config cfg;
  MapDev map;
  smx_state st;
  smx_spawns sp;
  smx_outputs out;
  const int8_t* actions;
  const float* actions_f32;  // float action spaces: [E*N][3]
  const double* traj;        // Trajectory space: [E*N][4][SMX_TRAJ_COLS]
  const int32_t* traj_n;     // ... true lengths, 0 = no action
  // the kinematic spaces use the same two: TargetPose traj = [E*N][4] targets (traj_n null); TrajectoryWithTime
  // traj = [E*N][5][traj_max], traj_n = points given
  int traj_max;
  const uint8_t* env_mask;  // k_reset: explicit mask (NULL = use env_reset_pending / all)
  const double* lidar_rays;
  const smx_via* vias;          // device copy of smx_set_vias, or of the vias of smx_set_mission_pool
  const int32_t* via_slot_off;  // [num_vehicles + 1]; a pool: [missions + 2], read through mission_row
  int first_only;           // restrict to vehicles carrying SMX_F_FIRST (reset observations)
  int keep_reward_done;     // auto-reset: the terminal step's reward / done / env_done stay
  int reset_all;            // k_reset: every env (explicit reset with NULL mask)
  double heading_gain_pos, lateral_gain_pos;  // lateral gains for target_speed > 0
  int wp_pool_limit;        // k_waypoints_emit: records of its LDS pool in use (SMX_WPE_POOL; less: developer / tests)
  char* wp_spill;           // k_waypoints_emit: knot records of the paths its LDS pool has no room for, [workgroup][column][11] + lanes
  int walk_new;             // k_first: also walk the new vehicles' knot lists (large batches: for the next tick's k_control_fast)
  double nb_d2_max;         // the largest squared distance whose rounded square root is <= cfg.nb_radius (radius_threshold)
  int debug_skip;
  int wp_blocks, obs_blocks, lidar_blocks;  // k_sensors: workgroups per role (OGM takes the rest)
  double dagm_reach;        // widest lane's half width (which segments can touch a DAGM view)
  uint8_t* rgb;             // SMX_SENSOR_RGB: the image buffer bound by smx_set_rgb_output, [E*N][rgb_height][rgb_width][3]
  KnotLists knots;          // library-owned hand-off: k_wp_walk -> k_waypoints_tables
  // the map's knot table (smx_roadmap.h KnotRow), [n_lanepoints]; set in the one-lane cut's tick only: k_waypoints_emit
  // and k_control_fast take their knot lists from it and k_wp_walk is not launched (null: the walked lists)
  const KnotRow* knot_table;
  unsigned long long* knot_served;  // developer (smx_debug_set_knot_table(h, 2)): path lanes k_waypoints_emit served from a row
  MissionsDev missions;     // device copy of smx_set_missions or smx_set_mission_pool (null pointers: every mission endless)
  // large batches: the tick's alive vehicles, compacted by k_alive_list at the start of the tick (null: launch
  // index = vehicle).  The per-vehicle team kernels then run over full wavefronts however many agents are gone.
  const int32_t* alive_list;
  const int32_t* alive_count;
  int alive_segmented;      // 1: the list k_tail built at the end of the last tick (eight segments, launch_vehicle)
  int32_t* status;          // library-owned device word of SMX_DEVICE_* bits, read and cleared by smx_sync
  // library-owned, kept from tick to tick: what the scan's seeded searches start from (smx_scan.h).  Null: unseeded.
  double* seeds_carry;      // [4][E*N]: pose (x, y) the seeds half last ran at, d2 of its 10th nearest and of its nearest lanepoint (< 0: none)
  double* facts_carry;      // [2][E*N]: pose (x, y) the facts half last ran at (its answers are facts_i32 / facts_f64)
  // large batches: vehicles the one-lane scan kernels could not serve (k_scan_fast -> k_scan_half over this list)
  int32_t* slow_list;
  int32_t* slow_count;
  // [E*N], 1: the vehicle's path seeds, walks and rows are the slow chain's this tick (k_scan_fast<1> decides; null: none)
  uint8_t* seed_pending;
  // the state guard (smx_set_guard; smx_guard.h): the per-agent byte and the box a vehicle state has to lie in.  Read by
  // the GUARD instantiations of the control, reset and tail kernels only (null: the plan launches the others).
  uint8_t* guard;
  GuardBox guard_box;
  // traffic-history replay (smx_set_social_history; smx_history.h): history.vehicle null = none bound, the social slots are
  // the scripted lane followers.  Every branch on it is marked as the rare side.
  HistoryDev history;
  // ... at each vehicle's own dimensions (smx_set_social_history_dims, smx_set_agent_dims): dims.slot null = neither bound,
  // every box is the sedan's.  dims.slot holds a triple per vehicle of the batch, written beside a replayed slot's pose
  // (dims.table) and beside an agent's spawn pose (dims.agent).
  HistoryDimsDev dims;
  // history agents (smx_set_history_agents; the table itself is history.follow): the caller's optional expert-action and
  // status rows, written where a follower's pose is (respawn_vehicle, k_control_kinematic's FOLLOW form); null: not wanted
  float* ha_action;
  uint8_t* ha_status;
  // OGM delta stores (TickPlan::ogm_delta), library-owned, [E*N][smx_ogm_mask_words(tile)]: bit p of an agent's words = piece
  // p (SMX_OGM_PIECE bytes) of its tile in the caller's out.ogm may be non-zero; a clear bit says the piece IS zero there.
  // A kernel stores a piece iff it is non-zero now or its bit was set, and leaves the bit = non-zero now (ogm_store_tile;
  // zero_dense_rows zeroes the tile and clears the words).  Null: every piece is stored.  No two kernels of a tick that can
  // run beside each other touch the same agent's words: k_ogm_env / the OGM role draw for the agents alive at the tick's
  // start, zero_dense_rows runs for agents that were not, and k_tail's tiles of new vehicles come after both have joined.
  unsigned long long* ogm_mask;
  // delayed agent entry (smx_set_agent_entry; smx_k_entry.h): entry.ready null = none bound, every agent enters at its
  // reset.  Read by respawn_vehicle on the rare side of a branch, and by k_entry.
  EntryDev entry;
};
enum {
  SMX_DEVICE_BAD_LANE_ACTION = 1,  // a Lane action code outside -1..3 was met (and treated as "no action")
  SMX_DEVICE_BAD_TRAJECTORY = 2,   // a TrajectoryWithTime action the reference raises on (it moved nothing)
  SMX_DEVICE_BAD_TARGET_POSE = 4,  // a TargetPose / Imitation action whose pose or speed came out not finite (it moved nothing)
  SMX_DEVICE_BAD_MISSION_ROW = 8   // an entry outside -1 .. M - 1 in the table of a mission pool was met (and read as -1)
};

#define SF(field) a.st.f64[(size_t)(field) * total + gid]

// The alive list k_tail builds for the next tick is eight segments, one counter each (2 048 workgroups adding to one
// counter would queue behind each other: 28 us for 2 048 atomics on one word at 131 k vehicles).  Vehicle g belongs to
// segment (g / 64) % 8 — the workgroups of 64-vehicle env groups then add to their own XCD's counter — and list
// position i holds entry ((i / 512) * 64 + i % 64) of segment (i / 64) % 8: a wavefront's 64 positions are 64
// consecutive entries of one segment, and a segment has exactly as many positions below E*N as it can have entries.
__device__ __forceinline__ size_t seg_position(const size_t seg, const size_t off) {
  return ((off >> 6) << 9) | (seg << 6) | (off & 63);
}

// The vehicle that team (or lane) i of a per-vehicle launch works on; `total` = none (i is past the last one).
__device__ __forceinline__ size_t launch_vehicle(const KernelArgs& a, size_t i, size_t total) {
  if (a.alive_list == nullptr) return i < total ? i : total;
  // (the entry is loaded beside the count, not behind it: one round trip; entries past the count are old vehicle
  // numbers or zeros, in range either way)
  const int32_t entry = a.alive_list[i < total ? i : total - 1];
  if (a.alive_segmented) {
    const size_t off = ((i >> 9) << 6) | (i & 63);
    return (i < total && off < (size_t)a.alive_count[SMX_SEG_STRIDE * ((i >> 6) & 7)]) ? (size_t)entry : total;
  }
  return i < (size_t)*a.alive_count ? (size_t)entry : total;
}

// Developer timing switches ("switch a piece off and see what the tick costs without it"): they exist
// only in the -DSMX_DEBUG_TIMING variant of the library (smarts_amd/build.py --prof); in the shipped
// library the test is the constant false and nothing, environment included, can drop work from a tick.
#if defined(SMX_ABLATE)  // developer variant without the stamps: the pieces named by a compile-time mask are off
#define SMX_SKIP(args, bit) (((SMX_ABLATE) & (bit)) != 0)
#elif defined(SMX_DEBUG_TIMING)
#define SMX_SKIP(args, bit) (((args).debug_skip & (bit)) != 0)
#else
#define SMX_SKIP(args, bit) false
#endif

// ---------------------------------------------------------------------------------
// oriented-box proximity (substitution for pybullet getClosestPoints)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void box_corners(double x, double y, double sh, double ch, double len, double wid,
                                            double* cx, double* cy) {
  double fx = -sh, fy = ch, rx = ch, ry = sh;
  double hl = 0.5 * len, hw = 0.5 * wid;
  cx[0] = x + fx * hl + rx * hw;
  cy[0] = y + fy * hl + ry * hw;
  cx[1] = x + fx * hl - rx * hw;
  cy[1] = y + fy * hl - ry * hw;
  cx[2] = x - fx * hl - rx * hw;
  cy[2] = y - fy * hl - ry * hw;
  cx[3] = x - fx * hl + rx * hw;
  cy[3] = y - fy * hl + ry * hw;
}

__device__ __forceinline__ bool point_in_box(double px, double py, double x, double y, double sh, double ch,
                                             double len, double wid) {
  double fx = -sh, fy = ch, rx = ch, ry = sh;
  double dx = px - x, dy = py - y;
  return fabs(dx * fx + dy * fy) <= 0.5 * len && fabs(dx * rx + dy * ry) <= 0.5 * wid;
}

__device__ __forceinline__ double seg_point_dist2(double px, double py, double ax, double ay, double bx, double by) {
  double dx = bx - ax, dy = by - ay;
  double ll = dx * dx + dy * dy;
  double t = (ll == 0.0) ? 0.0 : ((px - ax) * dx + (py - ay) * dy) / ll;
  t = fmin(1.0, fmax(0.0, t));
  double ex = ax + t * dx - px, ey = ay + t * dy - py;
  return ex * ex + ey * ey;
}

// (box a: len x wid, box b: blen x bwid.  Two equal boxes: 0.5 d + 0.5 d is d exactly, the reach of one full diagonal.)
__device__ inline bool boxes_within(double ax, double ay, double ah, double bx, double by, double bh, double len,
                                    double wid, double blen, double bwid, double leeway) {
  // broad phase: circumscribed circles
  double dx = ax - bx, dy = ay - by;
  double reach = 0.5 * sqrt(len * len + wid * wid) + 0.5 * sqrt(blen * blen + bwid * bwid) + leeway;
  if (dx * dx + dy * dy > reach * reach) return false;
  double cax[4], cay[4], cbx[4], cby[4];
  double sa, ca, sb, cb;
  sincos(ah, &sa, &ca);
  sincos(bh, &sb, &cb);
  box_corners(ax, ay, sa, ca, len, wid, cax, cay);
  box_corners(bx, by, sb, cb, blen, bwid, cbx, cby);
  double best = SMX_INF;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (point_in_box(cax[i], cay[i], bx, by, sb, cb, blen, bwid)) return true;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      best = fmin(best, seg_point_dist2(cax[i], cay[i], cbx[k], cby[k], cbx[(k + 1) & 3], cby[(k + 1) & 3]));
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (point_in_box(cbx[i], cby[i], ax, ay, sa, ca, len, wid)) return true;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      best = fmin(best, seg_point_dist2(cbx[i], cby[i], cax[k], cay[k], cax[(k + 1) & 3], cay[(k + 1) & 3]));
  }
  if (best <= leeway * leeway) return true;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double a0x = cax[i], a0y = cay[i], a1x = cax[(i + 1) & 3], a1y = cay[(i + 1) & 3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double b0x = cbx[k], b0y = cby[k], b1x = cbx[(k + 1) & 3], b1y = cby[(k + 1) & 3];
      double d1 = (a1x - a0x) * (b0y - a0y) - (a1y - a0y) * (b0x - a0x);
      double d2 = (a1x - a0x) * (b1y - a0y) - (a1y - a0y) * (b1x - a0x);
      double d3 = (b1x - b0x) * (a0y - b0y) - (b1y - b0y) * (a0x - b0x);
      double d4 = (b1x - b0x) * (a1y - b0y) - (b1y - b0y) * (a1x - b0x);
      if (((d1 > 0) != (d2 > 0)) && ((d3 > 0) != (d4 > 0))) return true;
    }
  }
  return false;
}

__device__ __forceinline__ void store_seeds(const KernelArgs& a, size_t gid, size_t total, const PathSeeds& s) {
  int32_t* c = a.st.seed_cache;
  c[0 * total + gid] = s.road;
  c[1 * total + gid] = s.f.n;
  c[2 * total + gid] = s.f.n > 0 ? s.f.road[0] : -1;
  c[3 * total + gid] = s.f.n > 1 ? s.f.road[1] : -1;
  c[4 * total + gid] = s.n_lanes;
  c[5 * total + gid] = s.start[0];
  c[6 * total + gid] = s.start[1];
  c[7 * total + gid] = s.start[2];
  c[8 * total + gid] = s.start[3];
}

__device__ __forceinline__ PathSeeds load_seeds(const KernelArgs& a, size_t gid, size_t total) {
  const int32_t* c = a.st.seed_cache;
  PathSeeds s;
  s.road = c[0 * total + gid];
  s.f.n = c[1 * total + gid];
  s.f.road[0] = c[2 * total + gid];
  s.f.road[1] = c[3 * total + gid];
  s.n_lanes = c[4 * total + gid];
  s.start[0] = c[5 * total + gid];
  s.start[1] = c[6 * total + gid];
  s.start[2] = c[7 * total + gid];
  s.start[3] = c[8 * total + gid];
  return s;
}

// The mission of vehicle slot `slot` of env `env`, as the index every per-mission table is read with (MissionsDev's
// tables, RouteFilter::road[0], the via offsets).  No pool bound: the slot itself.  A pool (smx_set_mission_pool): entry
// [env_episode[env] mod n_rows][env][slot] of the caller's table when it lies in 0 .. n - 1, else n — the endless mission
// the tables hold behind the pool's — for -1, for a social slot (it has no entry) and for any other value, which is
// reported by the next smx_sync and never used as an index.  env_episode is read as it stands: every kernel of a tick
// runs before the tick's commit advances it, every kernel of a reset pass after.  The table is the
// caller's and may change under a running episode; each site takes what it reads.
// `pooled` is a literal of the kernel that holds the site: the plan launches the kernels' pool instances (k_*_pool,
// TickPlan::pool) while a pool is bound and the others otherwise, and in those `pooled` is false and the lookup is not
// there — every kernel without a pool is the code it was before pools existed, as with ROUTED, SIZED, ENTRY and GUARD.
// 32-bit index arithmetic: the bind-time check keeps n_rows x E x A below 2^31.  The row of the episode is taken as the
// spawn, dimension and entry tables take theirs: ((k mod R) + R) mod R.
__device__ __forceinline__ int mission_row(const KernelArgs& a, int env, int slot, const bool pooled) {
  if (!pooled) return slot;
  const MissionsDev& ms = a.missions;
  const uint32_t n_agents = (uint32_t)(a.cfg.num_vehicles - a.cfg.num_social);
  if ((uint32_t)slot >= n_agents) return ms.n;
  const int rows = ms.n_rows;
  const uint32_t row = (uint32_t)(((a.st.env_episode[env] % rows) + rows) % rows);
  const int32_t entry = ms.rows[(row * (uint32_t)a.cfg.num_envs + (uint32_t)env) * n_agents + (uint32_t)slot];
  if ((uint32_t)entry < (uint32_t)ms.n) return entry;
  if (entry != -1) atomicOr(a.status, SMX_DEVICE_BAD_MISSION_ROW);
  return ms.n;
}
__device__ __forceinline__ int mission_row(const KernelArgs& a, size_t gid, const bool pooled) {
  const size_t n_veh = (size_t)a.cfg.num_vehicles;
  if (!pooled) return (int)(gid % n_veh);
  const uint32_t env = (uint32_t)gid / (uint32_t)n_veh;
  return mission_row(a, (int)env, (int)((uint32_t)gid - env * (uint32_t)n_veh), true);
}

// TripMeterSensor.append_waypoint_if_new's should_count_wp (sensors.py:908-913): with a fixed route only waypoints
// on the route's roads count.  The first waypoint of the first path lies on the seed road: with the waypoints
// sensor that is one of the route's roads by construction (_waypoint_paths_along_route); without it the path
// comes from the unrouted lookahead-1 query (sensors.py:271-275), whose start lanepoint is SMX_FI_OBS_START.
__device__ __forceinline__ bool trip_counts_waypoint(const KernelArgs& a, const MapDev& m, size_t gid, size_t total, const bool pooled) {
  RouteFilter f;
  if (!f.fixed_route(a.missions, mission_row(a, gid, pooled), m.n_roads)) return true;
  if (a.cfg.sensors & SMX_SENSOR_WAYPOINTS) return true;
  const int os = a.st.facts_i32[(size_t)SMX_FI_OBS_START * total + gid];
  if (os < 0) return true;  // no waypoint this tick anyway
  return f.has(m, m.lane_road[m.lp_rec[os].lane]);
}

__device__ __forceinline__ VehState load_vehicle(const KernelArgs& a, size_t gid, size_t total) {
  VehState s;
  s.x = SF(SMX_S_X);
  s.y = SF(SMX_S_Y);
  s.heading = SF(SMX_S_HEADING);
  s.u = SF(SMX_S_U);
  s.v = SF(SMX_S_V);
  s.r = SF(SMX_S_R);
  s.delta = SF(SMX_S_DELTA);
  return s;
}

// ---- traffic-history replay (smx_set_social_history; smx_history.h holds the frame arithmetic and the presence rule).
// The three callers are on the rare side of a branch on the bound pointer.  Inlined on purpose: out of line, with the
// argument block by reference, the compiler spills the whole block to scratch in every kernel that holds a call
// (profiles/r16_traffic_history_resources.txt).
// Is social slot `slot` of `env` present when the env's observation reports `env_ticks` ticks, and in which frame.
__device__ __forceinline__ bool history_slot_present(const KernelArgs& a, int env, int slot, int episode, int env_ticks, int64_t& frame) {
  frame = history_frame(a.history, episode, env, env_ticks);
  return history_present(a.history, episode, env, frame, slot);
}
// The dimensions of the vehicle a present slot holds in `frame` (smx_set_social_history_dims), written wherever the
// slot's pose is: a sensor sees the size of the vehicle whose pose it sees.  Nothing bound: nothing written.
__device__ __forceinline__ void history_store_dims(const KernelArgs& a, size_t gid, int64_t frame, int slot) {
  if (a.dims.table == nullptr) return;
  const double* d = history_dims_row(a.history, a.dims, frame, slot);
  double* w = a.dims.slot + gid * 3;
  w[0] = d[0];
  w[1] = d[1];
  w[2] = d[2];
}
// Vehicle `gid`'s box as every consumer reads it: the slot's triple with dimensions bound, else the sedan's.
struct VehBox {
  double length, width, height;
};
// (`sized`: dimensions are bound.  The kernels the launch plan instantiates with and without them — smx_plan.h,
// TickPlan::sized — pass their template argument; the others ask the argument block, marked as the rare side.)
__device__ __forceinline__ VehBox vehicle_box(const KernelArgs& a, size_t gid, bool sized) {
  VehBox b = {SMX_CHASSIS_LENGTH, SMX_CHASSIS_WIDTH, SMX_CHASSIS_HEIGHT};
  if (sized) {
    const double* d = a.dims.slot + gid * 3;
    b.length = d[0];
    b.width = d[1];
    b.height = d[2];
  }
  return b;
}
__device__ __forceinline__ bool dims_sized(const KernelArgs& a) { return __builtin_expect(a.dims.slot != nullptr, 0); }
__device__ __forceinline__ VehBox vehicle_box(const KernelArgs& a, size_t gid) { return vehicle_box(a, gid, dims_sized(a)); }
// SIZED, an int template argument of the roles that read an agent's OWN box (scan, observe, respawn): 1 / 0 — the launch
// plan chose the instantiation (TickPlan::sized), and the one without dimensions holds nothing of that work —, -1: the
// role asks the argument block, the rare side of a branch.
template <int SIZED>
__device__ __forceinline__ bool own_box_sized(const KernelArgs& a) {
  return SIZED < 0 ? dims_sized(a) : SIZED != 0;
}
// An agent's triple (smx_set_agent_dims), written by respawn_vehicle beside the spawn pose and by nobody else: row
// (episode mod agent_rows) of the bound table, the sedan's for an all-NaN triple (the bind-time check lets NaN through
// for whole triples only) and with no table bound (social dimensions alone: an unbind shows at the next respawn).
// Only called with a triple block (dims.slot): with nothing bound nothing is written.
__device__ __forceinline__ void agent_store_dims(const KernelArgs& a, size_t gid, int episode) {
  VehBox b = {SMX_CHASSIS_LENGTH, SMX_CHASSIS_WIDTH, SMX_CHASSIS_HEIGHT};
  if (a.dims.agent != nullptr) {
    const int n_veh = a.cfg.num_vehicles, n_agents = n_veh - a.cfg.num_social, rows = a.dims.agent_rows;
    const size_t env = gid / (size_t)n_veh, k = gid - env * (size_t)n_veh;
    const size_t row = (size_t)(((episode % rows) + rows) % rows);
    const double* d = a.dims.agent + ((row * (size_t)a.cfg.num_envs + env) * (size_t)n_agents + k) * 3;
    if (d[0] == d[0]) b = VehBox{d[0], d[1], d[2]};
  }
  double* w = a.dims.slot + gid * 3;
  w[0] = b.length;
  w[1] = b.width;
  w[2] = b.height;
}
// The observer's own box on the sized path, with the reaches the road-facts search takes from it (smx_scan.h): the
// corners lie half a diagonal from the centre, and the search radius covers the lookups that are answered from its
// own nearest lane — off_route's half diagonal + 5 (sensors.py:548); within_radius = length (sensors.py:274) is covered
// by the length's cap, SMX_AGENT_DIMS_MAX_LENGTH = SMX_POSE_SCAN_RADIUS — and every segment a corner's road_with_point
// can see (`thr_max`: the widest threshold of the map).  The sedan: 2 m and
// SMX_POSE_SCAN_RADIUS, the constants of the path without dimensions.
static_assert(SMX_AGENT_DIMS_MAX_LENGTH == SMX_POSE_SCAN_RADIUS, "an agent's length is capped at the radius of its mates' road-facts search");
struct ObserverBox {
  double length, width, corner_reach, scan_radius;
};
__device__ __forceinline__ ObserverBox observer_box(const KernelArgs& a, size_t gid, double thr_max) {
  const VehBox b = vehicle_box(a, gid, true);
  const double half_diag = 0.5 * sqrt(b.length * b.length + b.width * b.width);
  ObserverBox o;
  o.length = b.length;
  o.width = b.width;
  o.corner_reach = fmax(2.0, half_diag + 1e-6);
  o.scan_radius = fmax(SMX_POSE_SCAN_RADIUS, half_diag + fmax(5.0, thr_max) + 1e-6);
  return o;
}
// The replayed vehicle's step, in the scripted step's place in the tick (before collisions and sensors): the pose and
// speed of the frame this tick's observation belongs to — env_ticks + 1, smarts.py:261-262 —, copied word for word.
// SMX_S_PREV_X / _Y as for the scripted vehicle.  The slot is alive because the last commit found it in this frame; if
// the caller has rewritten its tables since and the frame lacks it now, it leaves here, ahead of every sensor.
__device__ __forceinline__ void history_vehicle_step(const KernelArgs& a, size_t gid, size_t total, double prev_x, double prev_y) {
  const int n_veh = a.cfg.num_vehicles;
  const int env = (int)(gid / (size_t)n_veh);
  const int slot = (int)(gid - (size_t)env * n_veh) - (n_veh - a.cfg.num_social);
  int64_t frame;
  if (!history_slot_present(a, env, slot, a.st.env_episode[env], a.st.env_ticks[env] + 1, frame)) {
    a.st.flags[gid] = a.st.flags[gid] & ~SMX_F_ALIVE;
    return;
  }
  const double* row = history_row(a.history, frame, slot);
  SF(SMX_S_PREV_X) = prev_x;
  SF(SMX_S_PREV_Y) = prev_y;
  SF(SMX_S_X) = row[0];
  SF(SMX_S_Y) = row[1];
  SF(SMX_S_HEADING) = row[2];
  SF(SMX_S_U) = row[3];
  history_store_dims(a, gid, frame, slot);
}

// ---- history agents (smx_set_history_agents): an agent slot placed on a recorded vehicle's rows.  Called on the rare
// side of a branch on history.follow (respawn_vehicle) or from the FOLLOW form of k_control_kinematic, which the plan
// launches for smx_step_history_agents alone; inlined for the reason above.
// The follower's status byte and its expert action, wherever its pose is written: the inverse of ImitationController
// (imitation_controller.py:61-78) between `frame`, whose row of the followed vehicle `v` is `row`, and the next frame —
// float64, rounded once; NaN, NaN where the next frame lacks the vehicle and for a follower that is absent or has left.
__device__ __forceinline__ void history_agent_report(const KernelArgs& a, size_t gid, int status, int64_t frame, const double* row, int32_t v) {
  if (a.ha_status != nullptr) a.ha_status[gid] = (uint8_t)status;
  if (a.ha_action == nullptr) return;
  float acceleration = __builtin_nanf(""), angular_velocity = __builtin_nanf("");
  if (status == SMX_HA_FOLLOWING || status == SMX_HA_SHADOWED) {  // (a shadowed agent follows: its label is the follower's)
    const int next = history_find(a.history, frame + 1, v);
    if (next >= 0) {
      const double* to = history_row(a.history, frame + 1, next);
      acceleration = (float)((to[3] - row[3]) / a.cfg.dt);
      angular_velocity = (float)(min_angles_difference_signed(to[2], row[2]) / a.cfg.dt);
    }
  }
  a.ha_action[gid * 3 + 0] = acceleration;
  a.ha_action[gid * 3 + 1] = angular_velocity;
  a.ha_action[gid * 3 + 2] = 0.0f;
}
// A follower of a freshly reset env: its vehicle's row of the reset observation's frame in the place of the spawn row
// (every other state word is 0 already; SMX_S_KIN_LAST_DT = 0 is "no control() call yet").  Returns the flags word: a
// follower of nothing, or of a vehicle that frame lacks, does not enter — not alive, SMX_F_FIRST all the same so that
// the reset pass's observe role makes its rows an absent agent's, as for an empty replayed slot.
__device__ __forceinline__ int history_agent_respawn(const KernelArgs& a, size_t gid, size_t total, int episode) {
  const int n_veh = a.cfg.num_vehicles;
  const int env = (int)(gid / (size_t)n_veh);
  const int32_t v = history_followed(a.history, episode, env, (int)(gid - (size_t)env * n_veh));
  const int64_t frame = history_frame(a.history, episode, env, a.cfg.reset_elapsed_steps);
  const int at = history_find(a.history, frame, v);
  double x = 0.0, y = 0.0, heading = 0.0, speed = 0.0;
  if (at >= 0) {
    const double* row = history_row(a.history, frame, at);
    x = row[0], y = row[1], heading = row[2], speed = row[3];
    history_agent_report(a, gid, SMX_HA_FOLLOWING, frame, row, v);
  } else {
    history_agent_report(a, gid, SMX_HA_ABSENT, frame, nullptr, v);
  }
  SF(SMX_S_X) = x;
  SF(SMX_S_Y) = y;
  SF(SMX_S_HEADING) = heading;
  SF(SMX_S_U) = speed;
  SF(SMX_S_KIN_RAW_HEADING) = heading;
  SF(SMX_S_PREV_X) = x;
  SF(SMX_S_PREV_Y) = y;
  return SMX_F_FIRST | (at >= 0 ? SMX_F_ALIVE : 0);
}
// The agents of env `env` that did not enter at its reset (read after the env's respawn_vehicle calls are complete): what
// the env's done count starts at, so that the env ends when its present agents have ended.
__device__ __forceinline__ int history_agents_absent(const KernelArgs& a, int env) {
  const int n_veh = a.cfg.num_vehicles;
  int absent = 0;
  for (int k = 0; k < n_veh - a.cfg.num_social; ++k)
    if (!(a.st.flags[(size_t)env * n_veh + k] & SMX_F_ALIVE)) ++absent;
  return absent;
}

// A follower's tick (k_control_kinematic's FOLLOW form for every agent, its HANDOVER form for the agents the table does
// not drive), on the flags word and position its caller has loaded: the agent is placed on the row its recorded vehicle
// has in the frame of the coming observation, or leaves.  `status`: what a placed follower reports — SMX_HA_FOLLOWING, or
// SMX_HA_SHADOWED from the BUBBLES form.
__device__ __forceinline__ void history_agent_follow(const KernelArgs& a, size_t gid, size_t total, int flags, int env, int episode, double x,
                                                     double y, int status = SMX_HA_FOLLOWING) {
  const smx_config& c = a.cfg;
  // (no placement test under the guard: every row of the table was checked against the grids when it was bound, and a
  // follower's byte reads 0 — also in a mixed tick, and for an agent that was driven a tick ago: it lands on a row too)
  const int32_t v = history_followed(a.history, episode, env, (int)(gid - (size_t)env * c.num_vehicles));
  const int64_t frame = history_frame(a.history, episode, env, a.st.env_ticks[env] + 1);
  const int at = history_find(a.history, frame, v);
  if (at < 0) {
    // The vehicle has left the recording: the agent's done_this_step (agent_manager.py:153-157).  Nothing of its state
    // is stored; the observation is built from the held pose and the tick's commit ends the agent.
    a.st.flags[gid] = flags | SMX_F_LEFT;
    history_agent_report(a, gid, SMX_HA_LEFT, frame, nullptr, v);
    return;
  }
  const double* row = history_row(a.history, frame, at);
  SF(SMX_S_PREV_X) = x;  // the position recorded by the previous observation
  SF(SMX_S_PREV_Y) = y;
  SF(SMX_S_KIN_LAST_HEADING) = SF(SMX_S_HEADING);
  SF(SMX_S_KIN_LAST_DT) = c.dt;
  SF(SMX_S_X) = row[0];
  SF(SMX_S_Y) = row[1];
  SF(SMX_S_HEADING) = row[2];  // (wrapped already, as Heading.__new__ wraps it: include/smx.h, frames_host)
  SF(SMX_S_U) = row[3];
  history_agent_report(a, gid, status, frame, row, v);
}

// Scripted social vehicle (lane follower: no controller, no dynamics), on state words its caller has loaded:
// lane, offset and crossed flag (SMX_S_MCL_X / MCL_Y / SPD_INT), SMX_S_THROTTLE and the pose's x / y.
__device__ __forceinline__ void social_vehicle_step(const KernelArgs& a, size_t gid, size_t total, double mcl_x, double mcl_y,
                                                    double spd_int, double throttle, double prev_x, double prev_y) {
  const smx_config& c = a.cfg;
  if (__builtin_expect(a.history.vehicle != nullptr, 0)) {
    history_vehicle_step(a, gid, total, prev_x, prev_y);
    return;
  }
  int lane = (int)mcl_x, crossed = (int)spd_int;
  double offset = mcl_y, speed, x, y, heading;
  SF(SMX_S_PREV_X) = prev_x;
  SF(SMX_S_PREV_Y) = prev_y;
  // SMX_SOCIAL_IDM: k_social decided this tick's speed from the state at the start of the tick
  const double cmd = c.social_model == SMX_SOCIAL_IDM ? throttle : -1.0;
  social_step(a.map, (int)(gid % c.num_vehicles), c.social_speed_factor, c.dt, lane, offset, crossed, speed, cmd);
  social_pose(a.map, lane, offset, x, y, heading);
  SF(SMX_S_X) = x;
  SF(SMX_S_Y) = y;
  SF(SMX_S_HEADING) = heading;
  SF(SMX_S_U) = speed;
  SF(SMX_S_MCL_X) = (double)lane;
  SF(SMX_S_MCL_Y) = offset;
  SF(SMX_S_SPD_INT) = (double)crossed;
}

// (loads that need the vehicle number only: k_control_fast issues them before it has looked at the flags)
__device__ __forceinline__ CtrlState load_ctrl_state(const KernelArgs& a, size_t gid, size_t total, int flags) {
  CtrlState cs;
  cs.lat_int = SF(SMX_S_LAT_INT);
  cs.spd_int = SF(SMX_S_SPD_INT);
  cs.steer = SF(SMX_S_STEER);
  cs.throttle = SF(SMX_S_THROTTLE);
  cs.spd_err = SF(SMX_S_SPD_ERR);
  cs.mcl_x = SF(SMX_S_MCL_X);
  cs.mcl_y = SF(SMX_S_MCL_Y);
  cs.mcl_set = (flags & SMX_F_MCL_SET) != 0;
  return cs;
}

// The state rows after vehicle_step.
__device__ __forceinline__ void store_vehicle_state(const KernelArgs& a, size_t gid, size_t total, const VehState& s,
                                                    const CtrlState& cs, int flags) {
  SF(SMX_S_X) = s.x;
  SF(SMX_S_Y) = s.y;
  SF(SMX_S_HEADING) = s.heading;
  SF(SMX_S_U) = s.u;
  SF(SMX_S_V) = s.v;
  SF(SMX_S_R) = s.r;
  SF(SMX_S_DELTA) = s.delta;
  SF(SMX_S_LAT_INT) = cs.lat_int;
  SF(SMX_S_SPD_INT) = cs.spd_int;
  SF(SMX_S_STEER) = cs.steer;
  SF(SMX_S_THROTTLE) = cs.throttle;
  SF(SMX_S_SPD_ERR) = cs.spd_err;
  SF(SMX_S_MCL_X) = cs.mcl_x;
  SF(SMX_S_MCL_Y) = cs.mcl_y;
  a.st.flags[gid] = cs.mcl_set ? (flags | SMX_F_MCL_SET) : (flags & ~SMX_F_MCL_SET);
}

// ---- the state guard's steps in the control phase (GUARD instantiations only; smx_guard.h holds the test and the table)
// The parked vehicle: lanepoint 0's pose at rest, state and controller words as after a reset (respawn_vehicle), the
// previous-observation position at the same place (the driven path then sees a step of length 0, not the bad pose).
__device__ __forceinline__ void guard_park(const KernelArgs& a, size_t gid, size_t total, int flags, uint8_t byte) {
  const GuardParked p = guard_parked_pose(a.map.lp_rec[0]);
  for (int f = SMX_S_X; f <= SMX_S_MCL_Y; ++f) SF(f) = 0.0;
  SF(SMX_S_X) = p.x;
  SF(SMX_S_Y) = p.y;
  SF(SMX_S_HEADING) = p.heading;
  if (smx_kinematic_space(a.cfg.action_space)) SF(SMX_S_KIN_RAW_HEADING) = p.heading;
  SF(SMX_S_PREV_X) = p.x;
  SF(SMX_S_PREV_Y) = p.y;
  a.st.flags[gid] = (flags & ~SMX_F_MCL_SET) | SMX_F_GUARDED;
  a.guard[gid] = byte;
}
// The verdict at the load: may the controller, its path search and the dynamics run for this vehicle?  (No writes: the
// teams of k_control and k_control_paths ask with every lane.)
__device__ __forceinline__ GuardVerdict guard_at_load(const KernelArgs& a, int flags, const VehState& s) {
  return guard_resolve((flags & SMX_F_GUARDED) != 0, guard_in_bounds(a.guard_box, s), true);
}
// ... carried out by the one lane that owns the vehicle's words when the answer is no: parked, or held (a parked spawn
// waiting for its first observation with done: nothing moves).
__device__ __forceinline__ void guard_refuse(const KernelArgs& a, size_t gid, size_t total, int flags, const GuardVerdict v) {
  if (v.action == GUARD_PARK) {
    guard_park(a, gid, total, flags, v.byte);
  } else {
    a.guard[gid] = v.byte;
    a.st.flags[gid] = flags | SMX_F_GUARDED;
  }
}
// The verdict on the stepped state, ahead of store_vehicle_state: true = store it.  Held: the state rows, the controller
// rows and the flags word keep what they held at the start of the tick, but for SMX_F_GUARDED.
__device__ __forceinline__ bool guard_before_store(const KernelArgs& a, size_t gid, int flags, const VehState& s) {
  const GuardVerdict v = guard_resolve(false, true, guard_in_bounds(a.guard_box, s));
  a.guard[gid] = v.byte;
  if (v.action == GUARD_STORE) return true;
  a.st.flags[gid] = flags | SMX_F_GUARDED;
  return false;
}

// A vehicle of a freshly reset env: state from the spawn table row of `episode`
// (SMARTS.reset / TrapManager, smarts.py:365-460, trap_manager.py:212-230).
// (GUARD: an agent's spawn row that is out of bounds — smx_guard.h — creates the vehicle parked at lanepoint 0 at rest,
// flagged SMX_F_GUARDED, its byte SMX_GUARD_SPAWN; a social slot's pose comes from the library's own tables)
// A replayed social slot of a freshly reset env (smx_set_social_history): its first pose and SMX_F_ALIVE come from the
// frame of the reset observation, cfg.reset_elapsed_steps ticks into `episode`'s window; every other state word is 0.
// Returns the flags word.  An empty slot is not alive; it carries SMX_F_FIRST all the same, so that the reset pass's
// observe role makes its rows an absent agent's (every other reader of SMX_F_FIRST asks for SMX_F_ALIVE first).
__device__ __forceinline__ int history_respawn(const KernelArgs& a, size_t gid, size_t total, int episode) {
  const int n_veh = a.cfg.num_vehicles;
  const int env = (int)(gid / (size_t)n_veh);
  const int slot = (int)(gid - (size_t)env * n_veh) - (n_veh - a.cfg.num_social);
  int64_t frame;
  const bool present = history_slot_present(a, env, slot, episode, a.cfg.reset_elapsed_steps, frame);
  double x = 0.0, y = 0.0, heading = 0.0, speed = 0.0;
  if (present) {
    const double* row = history_row(a.history, frame, slot);
    x = row[0], y = row[1], heading = row[2], speed = row[3];
    history_store_dims(a, gid, frame, slot);
  }
  SF(SMX_S_X) = x;
  SF(SMX_S_Y) = y;
  SF(SMX_S_HEADING) = heading;
  SF(SMX_S_U) = speed;
  SF(SMX_S_KIN_RAW_HEADING) = 0.0;
  SF(SMX_S_PREV_X) = x;
  SF(SMX_S_PREV_Y) = y;
  return SMX_F_SOCIAL | SMX_F_FIRST | (present ? SMX_F_ALIVE : 0);
}

// An agent of a freshly reset env under delayed entry (smx_set_agent_entry), on the flags word respawn_vehicle made: ready
// tick 0 enters with the reset as before — status ENTERED at tick 0 —; any other is PENDING: not alive, SMX_F_FIRST all
// the same so that the reset pass's observe role makes its rows an absent agent's, as for an empty replayed slot.
__device__ __forceinline__ int entry_respawn(const KernelArgs& a, size_t gid, int episode, int fl) {
  const int n_veh = a.cfg.num_vehicles, n_agents = n_veh - a.cfg.num_social, rows = a.entry.rows;
  const size_t env = gid / (size_t)n_veh, k = gid - env * (size_t)n_veh;
  const size_t row = (size_t)(((episode % rows) + rows) % rows);
  const bool now = a.entry.ready[(row * (size_t)a.cfg.num_envs + env) * (size_t)n_agents + k] <= 0;
  a.entry.status[gid] = (uint8_t)(now ? SMX_ENTRY_ENTERED : SMX_ENTRY_PENDING);
  a.entry.entered[gid] = now ? 0 : -1;
  return now ? fl : SMX_F_FIRST;
}

// (ENTRY, as SIZED: 1 / 0 — the plan chose the instantiation of k_reset (TickPlan::entry), and the one without a table
// holds nothing of the entry branch —, -1: the caller asks the argument block, the rare side of a branch)
template <bool GUARD, int SIZED = -1, int ENTRY = -1>
__device__ __forceinline__ void respawn_vehicle(const KernelArgs& a, size_t gid, size_t total, int episode) {
  const int row = a.sp.episodes > 0 ? (((episode % a.sp.episodes) + a.sp.episodes) % a.sp.episodes) : 0;
  const double* sp = a.sp.pose + ((size_t)row * total + gid) * 4;
  for (int f = 0; f < SMX_S_COUNT; ++f) SF(f) = 0.0;
  int fl = SMX_F_ALIVE | SMX_F_FIRST;
  const int n_veh = a.cfg.num_vehicles;
  bool parked = false;
  if constexpr (GUARD) {
    const bool agent = (int)(gid % n_veh) < n_veh - a.cfg.num_social;
    const GuardVerdict gv = guard_resolve_spawn(!agent || guard_in_bounds_kin(a.guard_box, sp[0], sp[1], sp[2], sp[3]));
    a.guard[gid] = gv.byte;
    parked = gv.action == GUARD_PARK;
  }
  if (GUARD && parked) {
    const GuardParked p = guard_parked_pose(a.map.lp_rec[0]);
    SF(SMX_S_X) = p.x;
    SF(SMX_S_Y) = p.y;
    SF(SMX_S_HEADING) = p.heading;
    if (smx_kinematic_space(a.cfg.action_space)) SF(SMX_S_KIN_RAW_HEADING) = p.heading;
    SF(SMX_S_PREV_X) = p.x;
    SF(SMX_S_PREV_Y) = p.y;
    fl |= SMX_F_GUARDED;
  } else {
    SF(SMX_S_X) = sp[0];
    SF(SMX_S_Y) = sp[1];
    SF(SMX_S_HEADING) = wrap_heading(sp[2]);
    SF(SMX_S_U) = sp[3];
    // kinematic spaces: MotionPlannerProvider.create_vehicle takes pose.heading (:164-168); _last_dt is 0
    if (smx_kinematic_space(a.cfg.action_space)) SF(SMX_S_KIN_RAW_HEADING) = SF(SMX_S_HEADING);
    SF(SMX_S_PREV_X) = sp[0];
    SF(SMX_S_PREV_Y) = sp[1];
  }
  if ((int)(gid % n_veh) >= n_veh - a.cfg.num_social) {
    if (__builtin_expect(a.history.vehicle != nullptr, 0)) {
      fl = history_respawn(a, gid, total, episode);  // (the spawn rows written above are overwritten or unused: not alive)
    } else {
      const double* so = a.sp.social + ((size_t)row * total + gid) * 2;
      SF(SMX_S_MCL_X) = so[0];  // lane
      SF(SMX_S_MCL_Y) = so[1];  // arclength offset
      fl |= SMX_F_SOCIAL;
    }
  } else {
    if (__builtin_expect(a.history.follow != nullptr, 0)) {
      // a history agent (smx_set_history_agents): the recording's row, not the spawn row (whose guard verdict goes with it)
      fl = history_agent_respawn(a, gid, total, episode);
      if constexpr (GUARD) a.guard[gid] = 0;
    }
    // the agent's own dimensions (smx_set_agent_dims), beside its pose: a follower keeps them through whatever comes
    if (own_box_sized<SIZED>(a)) agent_store_dims(a, gid, episode);
    // delayed entry (smx_set_agent_entry): an agent whose ready tick is not the reset observation's waits for k_entry
    if (ENTRY < 0 ? __builtin_expect(a.entry.ready != nullptr, 0) : ENTRY != 0) {
      fl = entry_respawn(a, gid, episode, fl);
      if constexpr (GUARD) {
        if (!(fl & SMX_F_ALIVE)) a.guard[gid] = 0;  // (an absent agent's byte: its spawn row is tested when it enters)
      }
    }
  }
  a.st.flags[gid] = fl;
  // the slot's knot lists belong to the vehicle that is gone (k_wp_walk only visits alive vehicles)
  if (a.knots.key != nullptr)
    for (int p = 0; p < SMX_WP_LANES; ++p) a.knots.key[gid * SMX_WP_LANES + p] = -1;
  a.st.facts_i32[(size_t)SMX_FI_TRIP_HAS_WP * total + gid] = 0;
  a.st.steps[gid] = 1;  // SensorState.step runs in the tick that creates the vehicle (agent_manager.py:250-258)
}

struct __align__(16) SharedPose {
  double x, y, heading, speed;
  double lane_dist;
  int lane;
  int alive;
  short nl, nlidx;  // lane and lane index an observer reports for this vehicle (-1: none within its length)
  int pad;
};

// OGM delta stores (KernelArgs::ogm_mask).  A step of a wavefront's copy-out is 64 int4: SMX_OGM_PIECE / 16 lanes share a
// piece, so a step covers 64 or 16 pieces and a mask word one step or four.
#define SMX_OGM_LPP (SMX_OGM_PIECE / 16)  // lanes per piece
#define SMX_OGM_PPS (64 / SMX_OGM_LPP)    // pieces per step
// the lanes' ballot -> a bit per piece of the step (a piece is non-zero when one of its lanes is)
__device__ __forceinline__ unsigned long long ogm_pieces_of_lanes(unsigned long long b) {
  if constexpr (SMX_OGM_LPP == 1) return b;
  b |= b >> 1;
  b |= b >> 2;
  b &= 0x1111111111111111ull;  // piece j at bit 4 j; packed below
  b = (b | (b >> 3)) & 0x0303030303030303ull;
  b = (b | (b >> 6)) & 0x000f000f000f000full;
  b = (b | (b >> 12)) & 0x000000ff000000ffull;
  return (b | (b >> 24)) & 0xffffull;
}
// ... and back: a bit per piece of the step -> the lanes of those pieces
__device__ __forceinline__ unsigned long long ogm_lanes_of_pieces(unsigned long long q) {
  if constexpr (SMX_OGM_LPP == 1) return q;
  q &= 0xffffull;
  q = (q | (q << 24)) & 0x000000ff000000ffull;
  q = (q | (q << 12)) & 0x000f000f000f000full;
  q = (q | (q << 6)) & 0x0303030303030303ull;
  q = (q | (q << 3)) & 0x1111111111111111ull;
  return q * 0xfull;
}
// One wavefront (every lane calls) copies a finished tile of n16 int4 from LDS to the agent's row `dst` of out.ogm under
// the agent's mask words: a piece leaves iff it is non-zero or its bit was set, and its bit becomes "non-zero".  The ballot
// and the words are uniform in the wavefront; lane 0 writes a word back once its pieces are through.  mask null: the plain
// copy.  (The words fetched once per tile into lanes and written back in one store took eight registers more and
// k_ogm_env a wavefront per SIMD: 70 -> 78 VGPRs.)
__device__ __forceinline__ void ogm_store_tile(const int4* src, int4* dst, unsigned long long* mask, const int n16, const int lane) {
  if (mask == nullptr) {
    for (int k = lane; k < n16; k += 64) dst[k] = src[k];
    return;
  }
  const int steps = (n16 + 63) >> 6;
  unsigned long long old_word = 0ull, new_word = 0ull;
#pragma nounroll
  for (int i = 0; i < steps; ++i) {
    const int k = i * 64 + lane;
    const bool mine = k < n16;
    int4 v = make_int4(0, 0, 0, 0);
    if (mine) v = src[k];
    const unsigned long long nz = ogm_pieces_of_lanes(__ballot((v.x | v.y | v.z | v.w) != 0));
    const int sub = i % SMX_OGM_LPP, shift = sub * SMX_OGM_PPS;  // the step's place in its mask word
    if (sub == 0) {
      old_word = mask[i / SMX_OGM_LPP];
      new_word = 0ull;
    }
    const unsigned long long leaving = ogm_lanes_of_pieces(nz | (old_word >> shift));
    if (mine && ((leaving >> lane) & 1ull)) dst[k] = v;
    new_word |= nz << shift;
    if ((sub == SMX_OGM_LPP - 1 || i == steps - 1) && lane == 0) mask[i / SMX_OGM_LPP] = new_word;
  }
}

// The rows of an agent that is gone read as an absent agent's: zeros (lane ids and slots -1).  Written by the whole
// workgroup, thread t of nth striding each array — one lane on its own took 4 096 byte stores for an OGM tile and
// 640 for the waypoint rows, one after the other, and the wavefront that held such a lane ended the kernel (C4: 380
// agents go per tick, one in six wavefronts of k_observe held one: 98 us for a kernel whose wavefronts take 43).
__device__ __forceinline__ void zero_dense_rows(const KernelArgs& a, size_t gid, int t, int nth) {
  const smx_config& c = a.cfg;
  const smx_outputs& o = a.out;
  for (int k = t; k < 3; k += nth) o.ego_pos[gid * 3 + k] = 0.0;
  for (int k = t; k < SMX_EGO_F32_COUNT; k += nth) o.ego_f32[gid * SMX_EGO_F32_COUNT + k] = 0.0f;
  for (int k = t; k < 2; k += nth) o.ego_lane[gid * 2 + k] = -1;
  for (int k = t; k < SMX_EV_COUNT; k += nth) o.events[gid * SMX_EV_COUNT + k] = 0;
  if (t == 0) {
    if (o.collidees) o.collidees[gid] = 0ull;
    o.reward[gid] = 0.0;
    o.dist[gid] = 0.0;
  }
  if (c.sensors & SMX_SENSOR_WAYPOINTS) {
    const int per = c.wp_paths * c.wp_len;
    for (int k = t; k < per * 3; k += nth) o.wp_pos[gid * per * 3 + k] = 0.0;
    for (int k = t; k < per; k += nth) {
      const size_t q = gid * per + k;
      o.wp_heading[q] = 0.0f;
      o.wp_lane_width[q] = 0.0f;
      o.wp_speed_limit[q] = 0.0f;
      o.wp_lane_index[q] = 0;
      o.wp_lane_id[q] = -1;
    }
    for (int k = t; k <= c.wp_paths; k += nth) o.wp_count[gid * (c.wp_paths + 1) + k] = 0;
  }
  if (c.sensors & SMX_SENSOR_NEIGHBORS) {
    for (int k = t; k < c.nb_max * 3; k += nth) {
      o.nb_pos[gid * c.nb_max * 3 + k] = 0.0;
      o.nb_box[gid * c.nb_max * 3 + k] = 0.0f;
    }
    for (int k = t; k < c.nb_max; k += nth) {
      const size_t q = gid * c.nb_max + k;
      o.nb_heading[q] = 0.0f;
      o.nb_speed[q] = 0.0f;
      o.nb_lane_index[q] = 0;
      o.nb_lane_id[q] = -1;
      o.nb_slot[q] = -1;
    }
    if (t == 0) o.nb_count[gid] = 0;
  }
  if ((c.sensors & SMX_SENSOR_LANE_TTC) && t == 0) o.lane_ttc_flags[gid] = 0;  // (the row itself stays: flags 0 say so)
  if (c.via_max > 0 && o.via_near) {
    for (int k = t; k < c.via_max; k += nth) o.via_near[gid * (size_t)c.via_max + k] = -1;
    if (t == 0) {
      o.via_near_count[gid] = 0;
      o.via_hit[gid] = 0;
    }
  }
  auto zero_bytes = [&](uint8_t* base, size_t n) {
    uint8_t* p = base + gid * n;
    if (n % 16 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      for (size_t k = t; k < n / 16; k += nth) reinterpret_cast<int4*>(p)[k] = make_int4(0, 0, 0, 0);
    } else {
      for (size_t k = t; k < n; k += nth) p[k] = 0;
    }
  };
  if ((c.sensors & SMX_SENSOR_OGM) && o.ogm) {
    zero_bytes(o.ogm, (size_t)c.ogm_width * c.ogm_height);
    if (a.ogm_mask) {  // the whole tile is zero now (nobody else holds this agent's words in this tick: KernelArgs::ogm_mask)
      const size_t words = smx_ogm_mask_words((size_t)c.ogm_width * c.ogm_height);
      for (size_t k = t; k < words; k += nth) a.ogm_mask[gid * words + k] = 0ull;
    }
  }
  if ((c.sensors & SMX_SENSOR_DAGM) && o.dagm) zero_bytes(o.dagm, (size_t)c.dagm_width * c.dagm_height);
  if ((c.sensors & SMX_SENSOR_LIDAR) && o.lidar_hit) {
    for (int k = t; k < c.lidar_rays; k += nth) o.lidar_hit[gid * (size_t)c.lidar_rays + k] = 0;
    for (int k = t; k < c.lidar_rays * 3; k += nth) o.lidar_point[gid * (size_t)c.lidar_rays * 3 + k] = 0.0;
  }
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

// floor(e / d) for 0 <= e < 4096, 1 <= d <= 64, rcp = 1.0f / d: (e + 0.5) / d is at least 0.5 / d away from an integer,
// the float32 product is off by less than 4096 / d * 2^-22
__device__ __forceinline__ int small_quotient(int e, float rcp) { return (int)(((float)e + 0.5f) * rcp); }

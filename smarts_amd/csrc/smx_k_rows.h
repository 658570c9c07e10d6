// smx_k_rows.h — the kernels that only transform rows and belong to no pass: road waypoints, lane TTC, the ego frame,
// the frame stacks and the copy of the agents' dimension triples.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_device.h"
#include "smx_plan.h"
#include "smx_roadmap.h"
#include "smx_scan.h"
#include "smx_tick.h"

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

// The agents' triples of one triple block into another (smx_handle.h build_dims_blob: the block moves when the social
// table beside it is bound or dropped while smx_set_agent_dims' table stays), then a synchronisation.
__global__ void __launch_bounds__(SMX_BLOCK) k_copy_agent_dims(const double* from, double* to, int n_veh, int n_agents, size_t total) {
  const size_t g = (size_t)blockIdx.x * SMX_BLOCK + threadIdx.x;
  if (g >= total || (int)(g % (size_t)n_veh) >= n_agents) return;
  for (int q = 0; q < 3; ++q) to[g * 3 + q] = from[g * 3 + q];
}

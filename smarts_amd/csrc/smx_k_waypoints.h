// smx_k_waypoints.h — the waypoints role: its serial, staged and emit-parallel forms, the knot walks, and their kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_plan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

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
                                                  int* knots, const WpFirst& fw, const bool pooled) {
  double dist = SF(SMX_S_DIST);
  bool has_wp = a.st.facts_i32[(size_t)SMX_FI_TRIP_HAS_WP * total + gid] != 0;
  if (flags & SMX_F_FIRST) {
    has_wp = trip_meter_start<KSTRIDE>(a, gid, total, px, py, knots);
    dist = 0.0;
  }
  const bool counts = fw.have && trip_counts_waypoint(a, a.map, gid, total, pooled);
  TripMeter t = trip_meter_of(dist, counts ? SF(SMX_S_TRIP_X) : 0.0, counts ? SF(SMX_S_TRIP_Y) : 0.0,
                              counts ? SF(SMX_S_TRIP_H) : 0.0, has_wp);
  if (counts) trip_meter_advance(a, gid, total, t, fw);
  trip_meter_store(a, gid, total, t);
}

// The serial emitter: every row of the vehicle and its trip meter, a team of SMX_WP_LANES lanes
template <int KSTRIDE>
__device__ __forceinline__ void waypoints_for(const KernelArgs& a, const size_t gid, int* knots, const bool pooled = false) {
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
  trip_meter_update<KSTRIDE>(a, gid, total, flags, px, py, knots, fw, pooled);
  SMX_TSTAMP(tw3);
  SMX_TACC(3, tw0, tw3);
}

__device__ __forceinline__ void waypoints_role(const KernelArgs& a, const int block, const bool pooled = false) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  waypoints_for<SMX_BLOCK>(a, ((size_t)block * SMX_BLOCK + threadIdx.x) / SMX_WP_LANES, knot_scratch + threadIdx.x, pooled);
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

__device__ __forceinline__ void waypoints_tables_role(const KernelArgs& a, const int block, const bool pooled = false) {
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
  if (live && p0 == 0) trip_meter_update<SMX_BLOCK>(a, gid, total, flags, px, py, knots, fw, pooled);
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

__device__ __forceinline__ void waypoints_emit_role(const KernelArgs& a, const int block, const bool pooled = false) {
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
    if (tm.n_paths > 0 && trip_counts_waypoint(a, m, gid, total, pooled)) {
      const WpFirst fw = {true, first_wp[v][0], first_wp[v][1], first_wp[v][2]};
      trip_meter_advance(a, gid, total, t, fw);
    }
    trip_meter_store(a, gid, total, t);
  }
  SMX_TSTAMP(te6);
  SMX_TACC(36, te5, te6);
  SMX_TACC(37, te0, te6);
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

// ---- the pool instances of the kernels above (TickPlan::pool; mission_row, smx_tick.h): the same roles with the trip
// meter's on-route rule read through the pool's table
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_pool(const KernelArgs a) { waypoints_role(a, (int)blockIdx.x, true); }
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_tables_pool(const KernelArgs a) { waypoints_tables_role(a, (int)blockIdx.x, true); }
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_emit_pool(const KernelArgs a) { waypoints_emit_role(a, (int)blockIdx.x, true); }
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_listed_pool(const KernelArgs a) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  const int count = *a.slow_count;
  constexpr int VPB = SMX_BLOCK / SMX_WP_LANES;
  for (int i = (int)blockIdx.x * VPB + (int)threadIdx.x / SMX_WP_LANES; i < count; i += (int)gridDim.x * VPB)
    waypoints_for<SMX_BLOCK>(a, (size_t)a.slow_list[i], knot_scratch + threadIdx.x, true);
}
__global__ void __launch_bounds__(SMX_BLOCK) k_waypoints_walk_listed_pool(const KernelArgs a) {
  __shared__ int knot_scratch[SMX_MAX_KNOTS * SMX_BLOCK];
  const int count = *a.slow_count;
  constexpr int VPB = SMX_BLOCK / (2 * SMX_WP_LANES);
  const bool walker = ((threadIdx.x / SMX_WP_LANES) & 1) != 0;
  for (int i = (int)blockIdx.x * VPB + (int)threadIdx.x / (2 * SMX_WP_LANES); i < count; i += (int)gridDim.x * VPB) {
    const size_t gid = (size_t)a.slow_list[i];
    if (walker)
      wp_walk_for(a, gid, (int)threadIdx.x % SMX_WP_LANES, false);
    else
      waypoints_for<SMX_BLOCK>(a, gid, knot_scratch + threadIdx.x, true);
  }
}

// Stand-alone host program over the device-free side of the mission pool (tests/test_mission_pool_host.py builds it with
// -fsanitize=address,undefined and runs it), over shim/hip_memory.h as tests/native/host_agent_dims.cpp is:
//   (a) smx_check_mission_pool's rule (smarts_amd/csrc/smx_host.h mission_pool_error / check_mission_pool_impl) over every
//       refusal, on heap tables of exactly the stated sizes;
//   (b) the handle (smarts_amd/csrc/smx_handle.h): smx_set_mission_pool bind / rebind / unbind, the tables it leaves on the
//       device — every one with the endless mission behind the pool's —, the SMX_ERR_STATE pairs with smx_set_missions /
//       smx_set_mission_goals / smx_set_vias, what a new map drops — field by field after each call, then the same
//       sequence once for every HIP call of the clean run with that call failing: the call returns SMX_ERR_HIP, every
//       pointer a kernel would get is null or inside a live allocation of its size, the call succeeds when repeated, and
//       nothing is live after smx_destroy.
// Prints one JSON line and returns 0 when every check held, else prints the failed checks and returns 1.
#include <hip_memory.h>  // the stand-in (and through it the shim <hip/hip_runtime.h>): plain C++

#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "smx_handle.h"
#include "tiny_map.h"

static int failures = 0, checks = 0;
static std::string context;
static void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    std::printf("FAILED [%s]: %s\n", context.c_str(), what.c_str());
  }
}
static bool contains(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }

enum { E = 2, N = 3, SOCIAL = 1, AGENTS = N - SOCIAL, TOTAL = E * N, ROWS = 2, M = 3 };

static smx_config config() {
  smx_config c{};
  c.num_envs = E, c.num_vehicles = N, c.dt = 0.1, c.num_social = SOCIAL, c.social_speed_factor = 1.0;
  c.action_space = SMX_ACTION_SPACE_LANE;
  c.sensors = SMX_SENSOR_WAYPOINTS;
  c.wp_lookahead = 32, c.wp_paths = 4, c.wp_len = 20, c.nb_radius = 50.0, c.via_max = 4;
  return c;
}

// A pool on the tiny map (roads 0 -> 1, lanes 0, 1 -> 2), every table on the heap at exactly its stated size:
// mission 0 the route 0 -> 1 with two vias, mission 1 the road 1 alone (a lap goal), mission 2 endless (a traverse goal).
struct Pool {
  smx_mission* missions = new smx_mission[M];
  int32_t* roads = new int32_t[3]{0, 1, 1};
  smx_mission_goal* goals = new smx_mission_goal[M];
  double* end_heading = new double[3]{0.0, 0.0, 0.5};
  int32_t* dead_end = new int32_t[3]{0, 0, 1};
  smx_via* vias = new smx_via[2];
  int32_t* via_off = new int32_t[M + 1]{0, 2, 2, 2};
  int32_t* rows = new int32_t[ROWS * E * AGENTS];  // (the caller's device table: the library never reads it on the host)
  smx_mission_pool p{};
  Pool() {
    missions[0] = smx_mission{50.0, 1.0, 2.0, 0, 2};
    missions[1] = smx_mission{55.0, 1.0, 2.0, 2, 1};
    missions[2] = smx_mission{0.0, 0.0, 0.0, 0, 0};
    goals[0] = smx_mission_goal{SMX_GOAL_POSITIONAL, 0, 0.0};
    goals[1] = smx_mission_goal{SMX_GOAL_LAP, 2, 30.0};
    goals[2] = smx_mission_goal{SMX_GOAL_TRAVERSE, 0, 0.0};
    vias[0] = smx_via{10.0, 0.0, 2.0, 5.0, 0, 0};
    vias[1] = smx_via{40.0, 1.0, 2.0, 5.0, 2, 0};
    for (int i = 0; i < ROWS * E * AGENTS; ++i) rows[i] = i % (M + 1) - 1;
    p.missions_host = missions, p.route_roads_host = roads, p.goals_host = goals, p.lane_end_heading_host = end_heading;
    p.lane_dead_end_host = dead_end, p.vias_host = vias, p.via_off_host = via_off, p.rows_dev = rows;
    p.rows_count = ROWS * E * AGENTS, p.n_missions = M, p.n_route_roads = 3, p.n_lanes = 3, p.n_vias = 2, p.rows = ROWS;
  }
  Pool(const Pool&) = delete;
  ~Pool() {
    delete[] missions, delete[] roads, delete[] goals, delete[] end_heading, delete[] dead_end, delete[] vias, delete[] via_off, delete[] rows;
  }
};

// ---- (a) the check
static void check_refusals() {
  context = "check";
  Map map;
  std::string why;
  auto run = [&](const smx_config& c, const smx_mission_pool& p) {
    why.clear();
    return check_mission_pool_impl(c, map.t, p, why);
  };
  {
    Pool g;
    expect(run(config(), g.p) == SMX_OK, "the pool is taken: " + why);
    smx_mission_pool q = g.p;
    q.goals_host = nullptr, q.lane_end_heading_host = nullptr, q.lane_dead_end_host = nullptr, q.n_lanes = 0;
    expect(run(config(), q) == SMX_OK, "without goal kinds: " + why);
    q = g.p, q.vias_host = nullptr, q.via_off_host = nullptr, q.n_vias = 0;
    expect(run(config(), q) == SMX_OK, "without vias: " + why);
    q = g.p, q.rows_count += 5;
    expect(run(config(), q) == SMX_OK, "a longer table of rows");
  }
  auto refused = [&](const char* what, const char* part, std::function<void(Pool&, smx_config&)> spoil) {
    Pool g;
    smx_config c = config();
    spoil(g, c);
    const int rc = run(c, g.p);
    expect(rc == SMX_ERR_INVALID && contains(why, part) && contains(why, "smx_set_mission_pool"), std::string(what) + " is refused with the reason: " + why);
  };
  refused("a null missions table", "null table", [](Pool& g, smx_config&) { g.p.missions_host = nullptr; });
  refused("a null road list", "null table", [](Pool& g, smx_config&) { g.p.route_roads_host = nullptr; });
  refused("a null table of rows", "rows_dev", [](Pool& g, smx_config&) { g.p.rows_dev = nullptr; });
  refused("null vias", "null table", [](Pool& g, smx_config&) { g.p.vias_host = nullptr; });
  refused("null via offsets", "null table", [](Pool& g, smx_config&) { g.p.via_off_host = nullptr; });
  refused("n_missions = 0", "SMX_MISSION_POOL_MAX", [](Pool& g, smx_config&) { g.p.n_missions = 0; });
  refused("n_missions over the cap", "4096", [](Pool& g, smx_config&) { g.p.n_missions = SMX_MISSION_POOL_MAX + 1; });
  refused("rows = 0", "rows must be", [](Pool& g, smx_config&) { g.p.rows = 0; });
  refused("a short table of rows", "needs 8", [](Pool& g, smx_config&) { g.p.rows_count = ROWS * E * AGENTS - 1; });
  refused("a table beyond 32-bit indices", "too large", [](Pool& g, smx_config& c) { g.p.rows = 1 << 30, c.num_envs = 4; });
  refused("a configuration without agents", "no agent slot", [](Pool&, smx_config& c) { c.num_social = N; });
  refused("a road outside the map", "road index out of range", [](Pool& g, smx_config&) { g.roads[1] = 2; });
  refused("a negative road", "road index out of range", [](Pool& g, smx_config&) { g.roads[2] = -1; });
  refused("a route range outside the list", "route range", [](Pool& g, smx_config&) { g.missions[1].route_off = 3; });
  refused("a fixed route without a goal", "PositionalGoal", [](Pool& g, smx_config&) { g.missions[0].goal_radius = -1.0; });
  refused("a lap goal on an empty route", "lap goal", [](Pool& g, smx_config&) { g.goals[2].kind = SMX_GOAL_LAP, g.goals[2].num_laps = 1; });
  refused("a traverse goal on a fixed route", "traverse goal", [](Pool& g, smx_config&) { g.goals[0].kind = SMX_GOAL_TRAVERSE; });
  refused("num_laps = 0", "num_laps", [](Pool& g, smx_config&) { g.goals[1].num_laps = 0; });
  refused("an unknown goal kind", "unknown goal kind", [](Pool& g, smx_config&) { g.goals[0].kind = 7; });
  refused("a traverse goal without the lane tables", "lane tables", [](Pool& g, smx_config&) { g.p.lane_dead_end_host = nullptr; });
  refused("lane tables of another map", "lane count", [](Pool& g, smx_config&) { g.p.n_lanes = 2; });
  refused("vias without via_max", "via_max", [](Pool&, smx_config& c) { c.via_max = 0; });
  refused("via offsets that do not end at n_vias", "offsets", [](Pool& g, smx_config&) { g.via_off[M] = 1; });
  refused("via offsets that descend", "offsets ascending", [](Pool& g, smx_config&) { g.via_off[1] = 2, g.via_off[2] = 1; });
  refused("a via on a lane outside the map", "lane index", [](Pool& g, smx_config&) { g.vias[1].lane = 3; });
  {  // more than 32 vias in one mission: a table of exactly 33
    Pool g;
    smx_via* many = new smx_via[33];
    for (int i = 0; i < 33; ++i) many[i] = g.vias[0];
    g.via_off[1] = g.via_off[2] = g.via_off[3] = 33;
    g.p.vias_host = many, g.p.n_vias = 33;
    expect(run(config(), g.p) == SMX_ERR_INVALID && contains(why, "at most 32 vias") && contains(why, "mission 0"), "33 vias in one mission: " + why);
    g.via_off[1] = 32;
    expect(run(config(), g.p) == SMX_OK, "32 and 1 are taken: " + why);
    delete[] many;
  }
  {  // the map tables themselves
    Pool g;
    Map bad;
    bad.t.lane_out_idx = nullptr;
    why.clear();
    expect(check_mission_pool_impl(config(), bad.t, g.p, why) == SMX_ERR_INVALID && contains(why, "map tables"), "a map without lane_out_idx");
  }
}

// ---- (b) the handle
static int fake_knot_table(smx_handle_s* h, KnotRow* table) {
  std::memset(table, 0, (size_t)h->map.n_lanepoints * sizeof(KnotRow));
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}
static int fake_copy_agent_dims(smx_handle_s*, const double*, double*) { return SMX_OK; }
static const KernelSide KERNELS = {352, 64 * 11 * 36, 0, fake_knot_table, fake_copy_agent_dims};

struct World {
  smx_handle h = nullptr;
  smx_config cfg = config();
  Map map_a, map_b;
  Pool pool;
  std::vector<smx_mission> slots{smx_mission{50.0, 1.0, 2.0, 0, 2}, smx_mission{0, 0, 0, 0, 0}, smx_mission{0, 0, 0, 0, 0}};
  std::vector<smx_mission_goal> slot_goals{smx_mission_goal{SMX_GOAL_LAP, 1, 30.0}, smx_mission_goal{}, smx_mission_goal{}};
  std::vector<int32_t> slot_via_off{0, 1, 2, 2};
};

static bool live_or_null(const void* p, size_t bytes) { return p == nullptr || shim_hip.inside(p, bytes); }
static bool bound(const smx_handle_s* h) { return h->missions.rows != nullptr; }
// what holds after every call, failed or not
static void check_handle(const smx_handle_s* h) {
  if (!h) return;
  const MissionsDev& ms = h->missions;
  const size_t slots = bound(h) ? (size_t)ms.n + 1 : (size_t)N;
  const size_t lanes = h->map_loaded ? (size_t)h->map.n_lanes : 0, roads = h->map_loaded ? (size_t)h->map.n_roads : 0;
  expect(live_or_null(ms.goal, slots * 3 * sizeof(double)) && live_or_null(ms.route_last, slots * sizeof(int32_t)) &&
             live_or_null(h->map.route_pos, slots * roads * sizeof(int16_t)) && live_or_null(h->map.route_lane_ok, slots * lanes),
         "the route tables are null or live allocations of their size");
  expect(live_or_null(ms.goal_kind, slots * sizeof(smx_mission_goal)), "the goal kinds are null or a live allocation of their size");
  // (a load that failed after it released the old map leaves no map — ticks are refused — and the old missions in their
  // blob, out of reach, for the next load to drop: the map's two route pointers are null then)
  expect((ms.route_last != nullptr) == (bool)h->missions_blob && (ms.goal != nullptr) == (bool)h->missions_blob, "the route tables with their blob");
  expect(h->map_loaded ? (h->map.route_pos != nullptr) == (bool)h->missions_blob && (h->map.route_lane_ok != nullptr) == (bool)h->missions_blob
                       : !h->map.route_pos && !h->map.route_lane_ok,
         "the map's route pointers with the blob, or null without a map");
  expect((ms.goal_kind != nullptr) == (bool)h->goals_blob, "the goal kinds with their blob");
  expect((h->n_vias > 0) == (bool)h->vias_dev && (bool)h->vias_dev == (bool)h->via_off_dev, "the vias with their blobs");
  if (h->n_vias > 0) {
    const int32_t* off = h->via_off_dev.get<int32_t>();
    expect(shim_hip.inside(off, (slots + 1) * sizeof(int32_t)) && shim_hip.inside(h->vias_dev.get<smx_via>(), (size_t)h->n_vias * sizeof(smx_via)),
           "the via tables are live allocations of their size");
    expect(off[0] == 0 && off[slots] == h->n_vias, "the via offsets run from 0 to n_vias over every entry");
  }
  if (bound(h)) {
    expect(ms.n >= 1 && ms.n <= SMX_MISSION_POOL_MAX && ms.n_rows >= 1, "a bound pool has its sizes");
    if (ms.route_last) expect(ms.route_last[ms.n] == -1, "the entry behind the pool has no route");
    if (ms.goal_kind) expect(ms.goal_kind[ms.n].kind == SMX_GOAL_POSITIONAL, "the entry behind the pool has no goal kind");
    if (h->n_vias > 0) expect(h->via_off_dev.get<int32_t>()[ms.n] == h->n_vias && h->via_off_dev.get<int32_t>()[ms.n + 1] == h->n_vias, "the entry behind the pool has no vias");
  } else {
    expect(ms.n == 0 && ms.n_rows == 0, "no pool: no sizes");
  }
  const DeviceBlob* blobs[] = {&h->map_blob, &h->knots_blob, &h->spill_blob, &h->knot_table, &h->knot_stats, &h->alive_blob, &h->pending_blob, &h->slow_blob,
                               &h->scan_carry, &h->ctrl_blob, &h->status_dev, &h->vias_dev, &h->via_off_dev, &h->missions_blob, &h->goals_blob,
                               &h->history_blob, &h->ogm_mask, &h->dims_blob, &h->agent_dims_blob, &h->entry_blob, &h->spaces_blob};
  size_t owned = 0;
  for (const DeviceBlob* b : blobs) {
    expect(!*b || shim_hip.live.count(b->get<const char>()) == 1, "every blob of the handle is empty or a live allocation");
    owned += (bool)*b;
  }
  expect(owned == shim_hip.live.size(), "every live allocation has its owner in the handle (" + std::to_string(owned) + " of " + std::to_string(shim_hip.live.size()) + ")");
}

struct Step {
  const char* name;
  std::function<int(World&)> call;
  std::function<void(World&)> after;
  int want = SMX_OK;  // SMX_ERR_STATE: the call is a refusal (it makes no HIP call)
};

static void pool_tables(World& w, bool goals, bool vias) {
  const smx_handle_s* h = w.h;
  const MissionsDev& ms = h->missions;
  expect(bound(h) && ms.rows == w.pool.rows && ms.n_rows == ROWS && ms.n == M, "the pool is bound: the caller's table, its rows, M");
  expect(ms.route_last && ms.route_last[0] == 1 && ms.route_last[1] == 1 && ms.route_last[2] == -1 && ms.route_last[M] == -1, "last roads, the endless entries -1");
  expect(ms.goal[0] == 50.0 && ms.goal[3 + 0] == 55.0 && ms.goal[3 + 2] == 2.0, "the goals");
  const int16_t* pos = h->map.route_pos;
  expect(pos[0 * 2 + 0] == 0 && pos[0 * 2 + 1] == 1 && pos[1 * 2 + 0] == -1 && pos[1 * 2 + 1] == 0 && pos[2 * 2 + 0] == -1 && pos[M * 2 + 1] == -1, "route positions, M + 1 rows");
  const uint8_t* ok = h->map.route_lane_ok;
  expect(ok[0] == 1 && ok[1] == 1 && ok[2] == 1 && ok[3 + 0] == 0 && ok[3 + 2] == 1 && ok[M * 3 + 2] == 0, "the lane table, M + 1 rows");
  expect((ms.goal_kind != nullptr) == goals, "goal kinds bound or not");
  if (goals) {
    expect(ms.goal_kind[1].kind == SMX_GOAL_LAP && ms.goal_kind[1].num_laps == 2 && ms.goal_kind[2].kind == SMX_GOAL_TRAVERSE, "the goal kinds");
    const double* heading = (const double*)(ms.goal_kind + (M + 1));  // MissionsDev::lane_end_heading(slots = M + 1)
    const int32_t* dead = (const int32_t*)(heading + 3);
    expect(shim_hip.inside(heading, 3 * sizeof(double) + 3 * sizeof(int32_t)) && heading[2] == 0.5 && dead[2] == 1 && dead[0] == 0, "the lane tables behind M + 1 goal kinds");
  }
  expect((h->n_vias == 2) == vias && (h->n_vias == 0) == !vias, "vias bound or not");
  if (vias) {
    const int32_t* off = h->via_off_dev.get<int32_t>();
    expect(off[0] == 0 && off[1] == 2 && off[2] == 2 && off[3] == 2 && off[4] == 2 && h->vias_dev.get<smx_via>()[1].lane == 2, "the via tables");
  }
  expect(h->host_route_last.empty(), "nothing is kept for smx_set_mission_goals");
}

static std::vector<Step> sequence() {
  std::vector<Step> s;
  auto nothing = [](World&) {};
  auto bind = [](World& w) { return set_mission_pool_impl(w.h, &w.pool.p); };
  auto unbind = [](World& w) { return set_mission_pool_impl(w.h, nullptr); };
  auto missions = [](World& w) { return set_missions_impl(w.h, w.slots.data(), N, w.pool.roads, 3); };
  auto goals = [](World& w) { return set_mission_goals_impl(w.h, w.slot_goals.data(), N, nullptr, nullptr, 0); };
  auto vias = [](World& w) { return set_vias_impl(w.h, w.pool.vias, 2, w.slot_via_off.data()); };
  auto names_pool = [](World& w) { expect(contains(w.h->err, "mission pool") && bound(w.h), "the refusal names the pool, which stays bound: " + w.h->err); };
  s.push_back({"smx_create", [](World& w) { return create_impl(&w.cfg, 0, &w.h, KERNELS); }, nothing});
  s.push_back({"smx_set_mission_pool before a map", bind, [](World& w) { expect(contains(w.h->err, "needs the map") && !bound(w.h), "refused: " + w.h->err); }, SMX_ERR_STATE});
  s.push_back({"smx_set_mission_pool(NULL) with nothing bound", unbind, nothing});
  s.push_back({"smx_load_map", [](World& w) { return load_map_impl(w.h, &w.map_a.t); }, nothing});
  s.push_back({"smx_set_missions", missions, [](World& w) { expect(!bound(w.h) && w.h->missions.route_last && w.h->host_route_last.size() == N, "per-slot missions"); }});
  s.push_back({"smx_set_mission_goals", goals, [](World& w) { expect(w.h->missions.goal_kind != nullptr, "per-slot goals"); }});
  s.push_back({"smx_set_vias", vias, [](World& w) { expect(w.h->n_vias == 2, "per-slot vias"); }});
  s.push_back({"smx_set_mission_pool", bind, [](World& w) { pool_tables(w, true, true); }});
  s.push_back({"smx_set_missions while bound", missions, names_pool, SMX_ERR_STATE});
  s.push_back({"smx_set_missions(clear) while bound", [](World& w) { return set_missions_impl(w.h, nullptr, 0, nullptr, 0); }, names_pool, SMX_ERR_STATE});
  s.push_back({"smx_set_mission_goals while bound", goals, names_pool, SMX_ERR_STATE});
  s.push_back({"smx_set_vias while bound", vias, names_pool, SMX_ERR_STATE});
  s.push_back({"smx_set_vias(clear) while bound", [](World& w) { return set_vias_impl(w.h, nullptr, 0, nullptr); }, names_pool, SMX_ERR_STATE});
  s.push_back({"smx_set_mission_pool (rebind, no goal kinds, no vias)", [](World& w) {
                 smx_mission_pool q = w.pool.p;
                 q.goals_host = nullptr, q.vias_host = nullptr, q.via_off_host = nullptr, q.n_vias = 0;
                 return set_mission_pool_impl(w.h, &q);
               }, [](World& w) { pool_tables(w, false, false); }});
  s.push_back({"smx_set_mission_pool (rebind, all of it)", bind, [](World& w) { pool_tables(w, true, true); }});
  s.push_back({"smx_set_mission_pool (a refused pool keeps the one in place)", [](World& w) {
                 Pool other;
                 other.roads[0] = 9;
                 const int rc = set_mission_pool_impl(w.h, &other.p);
                 expect(rc == SMX_ERR_INVALID && contains(w.h->err, "road index"), "refused: " + w.h->err);
                 return rc == SMX_ERR_INVALID ? (int)SMX_OK : rc;
               }, [](World& w) { pool_tables(w, true, true); }});
  s.push_back({"smx_set_mission_pool(NULL)", unbind, [](World& w) {
                 const smx_handle_s* h = w.h;
                 expect(!bound(h) && !h->missions.route_last && !h->missions.goal && !h->missions.goal_kind && !h->map.route_pos && !h->map.route_lane_ok &&
                            h->n_vias == 0 && !h->missions_blob && !h->goals_blob && !h->vias_dev && !h->via_off_dev,
                        "unbound: every mission endless, no vias, nothing allocated");
               }});
  s.push_back({"smx_set_missions after the unbind", missions, [](World& w) { expect(!bound(w.h) && w.h->missions.route_last != nullptr, "the per-slot call is taken again"); }});
  s.push_back({"smx_set_vias after the unbind", vias, [](World& w) { expect(w.h->n_vias == 2, "... and the vias"); }});
  s.push_back({"smx_set_mission_pool (over per-slot tables)", bind, [](World& w) { pool_tables(w, true, true); }});
  s.push_back({"smx_load_map (second)", [](World& w) { return load_map_impl(w.h, &w.map_b.t); }, [](World& w) {
                 const smx_handle_s* h = w.h;
                 expect(!bound(h) && !h->missions.route_last && !h->missions.goal_kind && !h->map.route_pos && h->n_vias == 0 && !h->vias_dev && !h->via_off_dev,
                        "a new map drops the pool with its vias");
               }});
  s.push_back({"smx_set_vias after the map", vias, nothing});
  s.push_back({"smx_set_mission_pool (after the map)", bind, [](World& w) { pool_tables(w, true, true); }});
  s.push_back({"smx_destroy", [](World& w) {
                 destroy_impl(w.h);
                 w.h = nullptr;
                 return (int)SMX_OK;
               }, [](World&) { expect(shim_hip.live.empty() && shim_hip.streams.empty() && shim_hip.events.empty(), "after smx_destroy nothing is live"); }});
  return s;
}

struct Tally {
  long refused = 0, release_points = 0, skipped = 0;
};

static void run(const std::vector<Step>& steps, long fail_at, Tally& tally) {
  shim_hip.reset();
  shim_hip.fail_at = fail_at;
  World w;
  for (const Step& s : steps) {
    context = (fail_at ? "call " + std::to_string(fail_at) + " fails" : std::string("clean")) + ", " + s.name;
    const bool armed = !shim_hip.fired;
    int rc = s.call(w);
    if (armed && shim_hip.fired) {
      if (shim_hip.fired_in_release) {
        ++tally.release_points;
        expect(rc == s.want, "a failed release does not fail the call");
      } else {
        ++tally.refused;
        expect(rc == SMX_ERR_HIP, "the call that contained the failed HIP call returns SMX_ERR_HIP, not " + std::to_string(rc));
        check_handle(w.h);
        rc = s.call(w);
        expect(rc == s.want, "repeating the failed call without the fault succeeds (" + std::to_string(rc) + (w.h ? ": " + w.h->err : "") + ")");
      }
    } else {
      expect(rc == s.want, "the call returns " + std::to_string(s.want) + " (" + std::to_string(rc) + (w.h ? ": " + w.h->err : ": " + g_create_err) + ")");
    }
    if (rc != s.want) break;
    check_handle(w.h);
    s.after(w);
  }
  if (w.h) destroy_impl(w.h);
  context = fail_at ? "call " + std::to_string(fail_at) + " fails, at the end" : "clean, at the end";
  if (fail_at && !shim_hip.fired) ++tally.skipped;
  expect(shim_hip.live.empty() && shim_hip.streams.empty() && shim_hip.events.empty(), "nothing is live at the end");
  expect(shim_hip.misuse == 0, "no HIP call was given a pointer that is not live");
}

int main() {
  check_refusals();
  context = "handle";
  expect(set_mission_pool_impl(nullptr, nullptr) == SMX_ERR_INVALID, "a null handle");
  const std::vector<Step> steps = sequence();
  Tally clean_tally, tally;
  run(steps, 0, clean_tally);
  const ShimHip clean = shim_hip;
  long points = 0;
  for (long n = 1; n <= clean.calls; ++n, ++points) run(steps, n, tally);
  context = "sweep";
  expect(points == clean.calls, "one sweep point for every HIP call of the clean run");
  expect(tally.skipped == 0 && tally.refused + tally.release_points == points, "every point's fault fired");
  if (failures) return 1;
  std::printf("{\"checks\": %d, \"steps\": %d, \"hip_calls\": %ld, \"sweep_points\": %ld, \"refused\": %ld, \"release_points\": %ld, \"skipped\": %ld, "
              "\"mallocs\": %ld, \"frees\": %ld}\n",
              checks, (int)steps.size(), clean.calls, points, tally.refused, tally.release_points, tally.skipped, clean.mallocs, clean.frees);
  return 0;
}

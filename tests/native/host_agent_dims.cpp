// Stand-alone host program over the device-free side of the per-agent vehicle dimensions (tests/test_host_agent_dims.py
// builds it with -fsanitize=address,undefined and runs it), over shim/hip_memory.h as tests/native/host_handle.cpp is:
//   (a) smx_check_agent_dims' rule (smarts_amd/csrc/smx_host.h check_agent_dims_impl) over every refusal, on a heap table
//       of exactly the stated size;
//   (b) the handle (smarts_amd/csrc/smx_handle.h): smx_set_agent_dims bind / rebind / unbind and what the other bindings
//       drop — a new history keeps the agents' dimensions and their triples and drops the social ones, a new map drops
//       both — field by field after each call, then the same sequence once for every HIP call of the clean run with that
//       call failing: the call returns SMX_ERR_HIP, every pointer a kernel would get is null or inside a live allocation
//       of its size, the call succeeds when repeated, and nothing is live after smx_destroy;
//   (c) the launch plan (smarts_amd/csrc/smx_plan.h): agent_dims_bound alone makes the plan sized and changes nothing else.
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

enum { E = 2, N = 3, SOCIAL = 1, AGENTS = N - SOCIAL, TOTAL = E * N, ROWS = 2 };
static const double NaN = std::numeric_limits<double>::quiet_NaN();

static smx_config config(int action_space = SMX_ACTION_SPACE_IMITATION) {
  smx_config c{};
  c.num_envs = E, c.num_vehicles = N, c.dt = 0.1, c.num_social = SOCIAL, c.social_speed_factor = 1.0;
  c.action_space = action_space;
  c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_OGM;
  c.wp_lookahead = 32, c.wp_paths = 4, c.wp_len = 20, c.nb_radius = 50.0;
  c.ogm_width = 16, c.ogm_height = 16, c.ogm_resolution = 0.5;
  return c;
}

// ---- (a) the check, over a heap table of exactly rows x E x AGENTS triples
static void check_refusals() {
  context = "check";
  const size_t words = (size_t)ROWS * E * AGENTS * 3;
  double* t = new double[words];
  auto fill = [&] {
    for (size_t i = 0; i < words; i += 3) t[i] = 10.0, t[i + 1] = 2.5, t[i + 2] = 4.0;
  };
  auto run = [&](const smx_config& c, const double* table, int rows, std::string& why) {
    smx_agent_dims d{table, rows};
    why.clear();
    return check_agent_dims_impl(c, d, why);
  };
  std::string why;
  fill();
  expect(run(config(), t, ROWS, why) == SMX_OK, "the trailer in every triple is taken: " + why);
  for (int space : {SMX_ACTION_SPACE_TARGET_POSE, SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME, SMX_ACTION_SPACE_IMITATION})
    expect(run(config(space), t, ROWS, why) == SMX_OK, "kinematic space " + std::to_string(space));
  for (int space : {SMX_ACTION_SPACE_LANE, SMX_ACTION_SPACE_CONTINUOUS, SMX_ACTION_SPACE_ACTUATOR_DYNAMIC, SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED,
                    SMX_ACTION_SPACE_TRAJECTORY, SMX_ACTION_SPACE_MPC})
    expect(run(config(space), t, ROWS, why) == SMX_ERR_INVALID && contains(why, "kinematic"), "dynamic space " + std::to_string(space) + " is refused");
  expect(run(config(), nullptr, ROWS, why) == SMX_ERR_INVALID && contains(why, "null table"), "a null table");
  expect(run(config(), t, 0, why) == SMX_ERR_INVALID && contains(why, "rows"), "rows = 0");
  expect(run(config(), t, -1, why) == SMX_ERR_INVALID, "rows < 0");
  smx_config none = config();
  none.num_social = N;
  expect(run(none, t, ROWS, why) == SMX_ERR_INVALID, "a configuration without agents");
  const double bad[] = {0.0, -1.0, NaN, std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
  for (size_t at : {(size_t)0, words / 2, words - 1})  // the first, a middle and the very last word of the table
    for (double v : bad) {
      fill();
      t[at] = v;
      expect(run(config(), t, ROWS, why) == SMX_ERR_INVALID, "word " + std::to_string(at) + " = " + std::to_string(v) + " is refused");
      expect(contains(why, "triple " + std::to_string(at / 3)), "... naming the triple: " + why);
    }
  fill();
  // the caps: the length's is the radius of the neighbours' lane search (10 m: the trailer exactly), not the 25 m of a
  // replayed vehicle's — an observer longer than that would be told "no lane" for a neighbour 10 m or more from its lane
  expect(SMX_AGENT_DIMS_MAX_LENGTH == 10.0 && SMX_DIMS_MAX_PLANAR == 25.0 && SMX_DIMS_MAX_HEIGHT == 10.0, "the caps");
  const double caps[3] = {SMX_AGENT_DIMS_MAX_LENGTH, SMX_DIMS_MAX_PLANAR, SMX_DIMS_MAX_HEIGHT};
  t[words - 3] = caps[0], t[words - 2] = caps[1], t[words - 1] = caps[2];
  expect(run(config(), t, ROWS, why) == SMX_OK, "the caps themselves are taken");
  for (int q = 0; q < 3; ++q) {
    fill();
    t[words - 3 + q] = std::nextafter(caps[q], 1e9);
    expect(run(config(), t, ROWS, why) == SMX_ERR_INVALID && contains(why, "<="), "a component just above its cap");
  }
  for (double length : {10.01, 16.0, 25.0}) {  // a 16 m truck can be replayed, not followed at its own length
    fill();
    t[0] = length;
    expect(run(config(), t, ROWS, why) == SMX_ERR_INVALID && contains(why, "length") && contains(why, "neighbours' lane search"),
           "a length of " + std::to_string(length) + " m is refused, with the reason");
  }
  fill();
  t[3] = t[4] = t[5] = NaN;
  expect(run(config(), t, ROWS, why) == SMX_OK, "three NaNs: the sedan's box");
  for (int q = 0; q < 3; ++q) {
    fill();
    t[3] = t[4] = t[5] = NaN;
    t[3 + q] = 2.0;
    expect(run(config(), t, ROWS, why) == SMX_ERR_INVALID && contains(why, "partly NaN"), "a triple that is only partly NaN");
  }
  // a table of one row is read to its end and no further (the sanitizer's to see)
  double* one = new double[(size_t)E * AGENTS * 3];
  for (size_t i = 0; i < (size_t)E * AGENTS * 3; ++i) one[i] = 1.0;
  expect(run(config(), one, 1, why) == SMX_OK, "rows = 1");
  delete[] one;
  delete[] t;
}

// ---- (c) the plan
static void check_plan() {
  context = "plan";
  static int32_t slow[64];
  static uint8_t pending[1];
  for (int total : {64, 32768})
    for (int is_step : {0, 1}) {
      smx_config c = config();
      c.num_envs = total / 32, c.num_vehicles = 32, c.num_social = 2;
      c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_NEIGHBORS | SMX_SENSOR_OGM | SMX_SENSOR_LIDAR;
      c.ogm_width = c.ogm_height = 64;
      PlanInputs pi{};
      pi.cfg = &c;
      pi.launch_strategy = SMX_LAUNCH_AUTO;
      pi.slow_blocks = 512;
      pi.is_step = is_step != 0;
      pi.alive_blob = pi.knots_blob = pi.ctrl_blob = pi.side_ready = true;
      pi.slow = SlowLists{slow, 0};
      pi.pending_blob = pending;
      TickPlan without = tick_plan(pi);
      pi.agent_dims_bound = true;
      TickPlan agents = tick_plan(pi);
      pi.dims_bound = true;
      TickPlan both = tick_plan(pi);
      pi.agent_dims_bound = false;
      TickPlan social = tick_plan(pi);
      expect(!without.sized && agents.sized && both.sized && social.sized, "sized is either binding");
      expect(agents.form == without.form && agents.control == without.control && agents.rows == without.rows && agents.facts == without.facts &&
                 agents.ogm == without.ogm && agents.lidar == without.lidar && agents.veh_blocks == without.veh_blocks &&
                 agents.obs_blocks == without.obs_blocks && agents.sensor_blocks == without.sensor_blocks && agents.sensor_lds == without.sensor_lds &&
                 agents.ogm_lds == without.ogm_lds && agents.lidar_blocks == without.lidar_blocks && agents.reset_pass == without.reset_pass &&
                 agents.tail_builds_list == without.tail_builds_list && agents.tail_grids == without.tail_grids,
             "the same launches on the same streams: nothing else of the plan moves");
    }
}

// ---- (b) the handle
static int fake_knot_table(smx_handle_s* h, KnotRow* table) {
  std::memset(table, 0, (size_t)h->map.n_lanepoints * sizeof(KnotRow));
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}
// the kernel of smx_kernels.hip, stood in: both blocks are live and of a block's size; then the synchronisation
static int fake_copy_agent_dims(smx_handle_s* h, const double* from, double* to) {
  expect(shim_hip.inside(from, TOTAL * 3 * sizeof(double)) && shim_hip.inside(to, TOTAL * 3 * sizeof(double)) && from != to,
         "the copy's two blocks are live, of a block's size, and not the same");
  for (int g = 0; g < TOTAL; ++g)
    if (g % N < AGENTS)
      for (int q = 0; q < 3; ++q) to[g * 3 + q] = from[g * 3 + q];
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}
static const KernelSide KERNELS = {352, 64 * 11 * 36, 0, fake_knot_table, fake_copy_agent_dims};

struct World {
  smx_handle h = nullptr;
  smx_config cfg = config();
  Map map_a, map_b;
  std::vector<double> frames{10.0, 1.0, 0.0, 5.0, /**/ 10.5, 1.0, 0.0, 5.0, /**/ 11.0, 1.0, 0.0, 5.0};  // 3 frames x 1 slot
  std::vector<int32_t> frame_vehicle{4, 4, -1}, start_frame = std::vector<int32_t>(ROWS * E, 0);
  std::vector<double> social_dims = std::vector<double>(5 * 3, 2.0);  // ids 0..4
  std::vector<double> agent_dims = std::vector<double>((size_t)ROWS * E * AGENTS * 3, 7.0);
  smx_social_history history() const {
    smx_social_history hs{};
    hs.frames_host = frames.data(), hs.vehicle_host = frame_vehicle.data(), hs.n_frames = 3, hs.num_social = SOCIAL;
    hs.start_frame_dev = start_frame.data(), hs.rows = ROWS, hs.start_count = start_frame.size();
    return hs;
  }
};

static bool live_or_null(const void* p, size_t bytes) { return p == nullptr || shim_hip.inside(p, bytes); }
static bool agents_bound(const smx_handle_s* h, int rows = ROWS) {
  return h->agent_dims_blob && h->dims.agent == h->agent_dims_blob.get<double>() && h->dims.agent_rows == rows && h->dims.slot;
}
static bool social_bound(const smx_handle_s* h) { return h->dims_blob && h->dims.table && h->dims.n_ids == 5 && h->dims.slot; }
// what holds after every call, failed or not
static void check_handle(const smx_handle_s* h) {
  if (!h) return;
  expect(live_or_null(h->dims.table, 5 * 3 * sizeof(double)) && live_or_null(h->dims.slot, TOTAL * 3 * sizeof(double)) &&
             live_or_null(h->dims.agent, (size_t)h->dims.agent_rows * E * AGENTS * 3 * sizeof(double)),
         "dims.table / slot / agent are null or live allocations of their size");
  expect((h->dims.agent != nullptr) == (bool)h->agent_dims_blob, "the agents' table with its blob");
  expect((h->dims.slot != nullptr) == (bool)h->dims_blob, "the triple block with its blob");
  expect((h->dims.slot != nullptr) == (h->dims.table != nullptr || h->dims.agent != nullptr), "a triple block exactly while either binding holds");
  expect(!h->dims.table || h->history.vehicle, "social dimensions only with a history");
  if (h->dims.slot)  // every triple is initialised: a whole box
    for (int g = 0; g < TOTAL; ++g)
      expect(h->dims.slot[g * 3] > 0.0 && h->dims.slot[g * 3 + 1] > 0.0 && h->dims.slot[g * 3 + 2] > 0.0, "triple " + std::to_string(g) + " is a box");
  const DeviceBlob* blobs[] = {&h->map_blob, &h->knots_blob, &h->spill_blob, &h->knot_table, &h->knot_stats, &h->alive_blob, &h->pending_blob, &h->slow_blob,
                               &h->scan_carry, &h->ctrl_blob, &h->status_dev, &h->vias_dev, &h->via_off_dev, &h->missions_blob, &h->goals_blob,
                               &h->history_blob, &h->ogm_mask, &h->dims_blob, &h->agent_dims_blob};
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
};
static bool sedan(const double* t) { return t[0] == SMX_CHASSIS_LENGTH && t[1] == SMX_CHASSIS_WIDTH && t[2] == SMX_CHASSIS_HEIGHT; }
// what respawn_vehicle does for env 0's agent 0: its triple into the block
static void spawn_agent0(World& w, double length) {
  if (w.h->dims.slot) w.h->dims.slot[0] = length, w.h->dims.slot[1] = 2.5, w.h->dims.slot[2] = 4.0;
}

static std::vector<Step> sequence() {
  std::vector<Step> s;
  auto history = [](World& w) {
    const smx_social_history hs = w.history();
    return set_social_history_impl(w.h, &hs);
  };
  auto social = [](World& w) {
    const smx_social_dims d{w.social_dims.data(), 5};
    return set_social_history_dims_impl(w.h, &d);
  };
  auto agents = [](World& w) {
    const smx_agent_dims d{w.agent_dims.data(), ROWS};
    return set_agent_dims_impl(w.h, &d);
  };
  auto nothing = [](World&) {};
  s.push_back({"smx_create", [](World& w) { return create_impl(&w.cfg, 0, &w.h, KERNELS); }, nothing});
  s.push_back({"smx_set_agent_dims before a map", agents, [](World& w) {
                 expect(agents_bound(w.h) && !w.h->dims.table && sedan(w.h->dims.slot) && sedan(w.h->dims.slot + (TOTAL - 1) * 3), "bound without a map or a history: a block of sedans");
                 expect(std::memcmp(w.h->dims.agent, w.agent_dims.data(), w.agent_dims.size() * sizeof(double)) == 0, "the table was copied whole");
               }});
  s.push_back({"smx_load_map", [](World& w) { return load_map_impl(w.h, &w.map_a.t); }, [](World& w) {
                 expect(w.h->map_loaded && !w.h->agent_dims_blob && !w.h->dims.agent && !w.h->dims.slot && !w.h->dims_blob && w.h->dims.agent_rows == 0, "a new map drops the agents' dimensions");
               }});
  s.push_back({"smx_set_agent_dims", agents, [](World& w) {
                 expect(agents_bound(w.h) && !w.h->dims.table, "bound");
                 spawn_agent0(w, 10.0);
               }});
  s.push_back({"smx_set_agent_dims (rebind, one row)", [](World& w) {
                 const smx_agent_dims d{w.agent_dims.data(), 1};
                 return set_agent_dims_impl(w.h, &d);
               }, [](World& w) { expect(agents_bound(w.h, 1) && w.h->dims.slot[0] == 10.0, "a rebind keeps the block: an agent keeps its triple until it is respawned"); }});
  s.push_back({"smx_set_social_history", history, [](World& w) {
                 expect(agents_bound(w.h, 1) && !w.h->dims.table && w.h->history.vehicle, "a history keeps the agents' dimensions");
                 expect(w.h->dims.slot[0] == 10.0 && sedan(w.h->dims.slot + 3) && sedan(w.h->dims.slot + (N - 1) * 3), "... and their triples, in a fresh block");
               }});
  s.push_back({"smx_set_social_history_dims", social, [](World& w) {
                 expect(agents_bound(w.h, 1) && social_bound(w.h), "both bound");
                 expect(w.h->dims.slot[0] == 10.0 && sedan(w.h->dims.slot + (N - 1) * 3) && w.h->dims.table[0] == 2.0, "the agents' triples moved into the block beside the social table");
                 w.h->dims.slot[(N - 1) * 3] = 2.0;  // (a replayed slot's pose was written)
               }});
  s.push_back({"smx_set_social_history (again)", history, [](World& w) {
                 expect(agents_bound(w.h, 1) && !w.h->dims.table && w.h->dims.n_ids == 0, "a new history drops the social dimensions and keeps the agents'");
                 expect(w.h->dims.slot[0] == 10.0 && sedan(w.h->dims.slot + (N - 1) * 3), "... the agent's triple kept, the replayed slot's the sedan's again");
               }});
  s.push_back({"smx_set_social_history_dims (again)", social, [](World& w) { expect(agents_bound(w.h, 1) && social_bound(w.h) && w.h->dims.slot[0] == 10.0, "both bound again"); }});
  s.push_back({"smx_set_social_history_dims (unbind)", [](World& w) { return set_social_history_dims_impl(w.h, nullptr); }, [](World& w) {
                 expect(agents_bound(w.h, 1) && !w.h->dims.table && w.h->dims.slot[0] == 10.0, "unbinding the social dimensions keeps the agents' and their triples");
               }});
  s.push_back({"smx_set_social_history_dims (third)", social, nothing});
  s.push_back({"smx_set_agent_dims (unbind, social bound)", [](World& w) { return set_agent_dims_impl(w.h, nullptr); }, [](World& w) {
                 expect(!w.h->agent_dims_blob && !w.h->dims.agent && social_bound(w.h), "unbinding the agents' keeps the social dimensions and the block");
                 expect(w.h->dims.slot[0] == 10.0, "... in which an agent is a sedan again from its next respawn, not before");
               }});
  s.push_back({"smx_set_agent_dims (bind, social bound)", agents, [](World& w) { expect(agents_bound(w.h) && social_bound(w.h), "both"); }});
  s.push_back({"smx_set_social_history (unbind)", [](World& w) { return set_social_history_impl(w.h, nullptr); }, [](World& w) {
                 expect(agents_bound(w.h) && !w.h->dims.table && !w.h->history.vehicle, "unbinding the history keeps the agents' dimensions");
               }});
  s.push_back({"smx_set_agent_dims (unbind)", [](World& w) { return set_agent_dims_impl(w.h, nullptr); }, [](World& w) {
                 expect(!w.h->agent_dims_blob && !w.h->dims.agent && !w.h->dims.slot && !w.h->dims_blob, "nothing bound: no block");
               }});
  s.push_back({"smx_set_agent_dims (unbind again)", [](World& w) { return set_agent_dims_impl(w.h, nullptr); }, nothing});
  s.push_back({"smx_set_social_history (last)", history, nothing});
  s.push_back({"smx_set_social_history_dims (last)", social, nothing});
  s.push_back({"smx_set_agent_dims (last)", agents, [](World& w) { expect(agents_bound(w.h) && social_bound(w.h), "both"); }});
  s.push_back({"smx_load_map (second)", [](World& w) { return load_map_impl(w.h, &w.map_b.t); }, [](World& w) {
                 expect(!w.h->agent_dims_blob && !w.h->dims.agent && !w.h->dims.slot && !w.h->dims.table && !w.h->dims_blob && !w.h->history_blob, "a new map drops both");
               }});
  s.push_back({"smx_set_agent_dims (after the map)", agents, nothing});
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
        expect(rc == SMX_OK, "a failed release does not fail the call");
      } else {
        ++tally.refused;
        expect(rc == SMX_ERR_HIP, "the call that contained the failed HIP call returns SMX_ERR_HIP, not " + std::to_string(rc));
        check_handle(w.h);
        rc = s.call(w);
        expect(rc == SMX_OK, "repeating the failed call without the fault succeeds (" + std::to_string(rc) + (w.h ? ": " + w.h->err : "") + ")");
      }
    } else {
      expect(rc == SMX_OK, "the call succeeds (" + std::to_string(rc) + (w.h ? ": " + w.h->err : ": " + g_create_err) + ")");
    }
    if (rc != SMX_OK) break;
    check_handle(w.h);
    s.after(w);
  }
  if (w.h) destroy_impl(w.h);
  context = fail_at ? "call " + std::to_string(fail_at) + " fails, at the end" : "clean, at the end";
  if (fail_at && !shim_hip.fired) ++tally.skipped;
  expect(shim_hip.live.empty() && shim_hip.streams.empty() && shim_hip.events.empty(), "nothing is live at the end");
  expect(shim_hip.misuse == 0, "no HIP call was given a pointer that is not live");
}

// the refusals through the handle: nothing of a binding in place is touched
static void handle_refusals() {
  context = "handle refusals";
  shim_hip.reset();
  World w;
  expect(create_impl(&w.cfg, 0, &w.h, KERNELS) == SMX_OK, "create");
  const smx_agent_dims good{w.agent_dims.data(), ROWS};
  expect(set_agent_dims_impl(w.h, &good) == SMX_OK, "bind");
  const double* table = w.h->dims.agent;
  std::vector<double> bad = w.agent_dims;
  bad[4] = 0.0;
  const smx_agent_dims zero{bad.data(), ROWS};
  expect(set_agent_dims_impl(w.h, &zero) == SMX_ERR_INVALID && contains(w.h->err, "agent dimensions"), "a zero is refused with a reason");
  expect(w.h->dims.agent == table && agents_bound(w.h), "... and the binding in place stays");
  expect(set_agent_dims_impl(nullptr, &good) == SMX_ERR_INVALID, "a null handle");
  destroy_impl(w.h);
  World lane;
  lane.cfg = config(SMX_ACTION_SPACE_LANE);
  expect(create_impl(&lane.cfg, 0, &lane.h, KERNELS) == SMX_OK, "create (Lane)");
  expect(set_agent_dims_impl(lane.h, &good) == SMX_ERR_INVALID && !lane.h->dims.agent && !lane.h->dims.slot, "a Lane-space handle refuses");
  expect(set_agent_dims_impl(lane.h, nullptr) == SMX_OK, "... and takes the unbind");
  destroy_impl(lane.h);
  expect(shim_hip.live.empty(), "nothing is live");
}

int main() {
  check_refusals();
  check_plan();
  handle_refusals();
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

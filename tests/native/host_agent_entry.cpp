// Stand-alone host program over the device-free side of delayed agent entry (tests/test_host_agent_entry.py builds it
// with -fsanitize=address,undefined and runs it), over shim/hip_memory.h as tests/native/host_handle.cpp is:
//   (a) smx_check_agent_entry's rule (smarts_amd/csrc/smx_host.h check_agent_entry_impl) over every refusal, each with its
//       message, on heap tables of exactly the stated size;
//   (b) the handle (smarts_amd/csrc/smx_handle.h): smx_set_agent_entry fill, then commit — bind before a map, a new map
//       drops it, rebind, unbind — and the refused combinations in both orders (history agents, a frame stack), field by
//       field after each call; then the same sequence once for every HIP call of the clean run with that call failing:
//       the call returns SMX_ERR_HIP, the binding in place is untouched or none is left, every pointer a kernel would get
//       is null or inside a live allocation of its size, the call succeeds when repeated, and nothing is live after
//       smx_destroy.
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

enum { E = 2, N = 3, SOCIAL = 1, AGENTS = N - SOCIAL, TOTAL = E * N, ROWS = 2, STACK = 2 };
static const double NaN = std::numeric_limits<double>::quiet_NaN();
static const double Inf = std::numeric_limits<double>::infinity();

static smx_config config() {
  smx_config c{};
  c.num_envs = E, c.num_vehicles = N, c.dt = 0.1, c.num_social = SOCIAL, c.social_speed_factor = 1.0;
  c.action_space = SMX_ACTION_SPACE_IMITATION;  // (history agents, for the refused combination)
  c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_OGM | SMX_SENSOR_RGB;
  c.wp_lookahead = 32, c.wp_paths = 4, c.wp_len = 20, c.nb_radius = 50.0;
  c.ogm_width = 16, c.ogm_height = 16, c.ogm_resolution = 0.5;
  c.rgb_width = 16, c.rgb_height = 8, c.rgb_resolution = 0.5;
  c.frame_stack = STACK;
  return c;
}

// ---- (a) the check, over heap tables of exactly rows x E x AGENTS cells
static void check_refusals() {
  context = "check";
  const size_t cells = (size_t)ROWS * E * AGENTS;
  int32_t* ready = new int32_t[cells];
  double* chk = new double[cells * 3];
  uint8_t* status = new uint8_t[TOTAL];
  int32_t* entered = new int32_t[TOTAL];
  auto fill = [&] {
    for (size_t i = 0; i < cells; ++i) {
      ready[i] = (int32_t)(i % AGENTS) * 5;  // agent 0 of every (row, env) at the reset, agent 1 five ticks later
      chk[i * 3] = 10.0 + (double)i, chk[i * 3 + 1] = -3.0, chk[i * 3 + 2] = 3.68;
    }
  };
  auto table = [&](int rows = ROWS) {
    smx_agent_entry d{};
    d.ready_host = ready, d.check_host = chk, d.rows = rows;
    d.status_dev = status, d.entered_dev = entered, d.status_count = TOTAL, d.entered_count = TOTAL;
    return d;
  };
  std::string why;
  auto run = [&](const smx_config& c, const smx_agent_entry& d) {
    why.clear();
    return check_agent_entry_impl(c, d, why);
  };
  fill();
  expect(run(config(), table()) == SMX_OK, "a good table is taken: " + why);
  expect(run(config(), table(1)) == SMX_OK, "rows = 1 (read to its end and no further)");
  expect(run(config(), table(0)) == SMX_ERR_INVALID && contains(why, "rows must be >= 1"), "rows = 0: " + why);
  expect(run(config(), table(-3)) == SMX_ERR_INVALID && contains(why, "rows must be >= 1"), "rows < 0");
  smx_agent_entry d = table();
  d.ready_host = nullptr;
  expect(run(config(), d) == SMX_ERR_INVALID && contains(why, "null table"), "a null ready table");
  d = table();
  d.check_host = nullptr;
  expect(run(config(), d) == SMX_ERR_INVALID && contains(why, "null table"), "a null check table");
  d = table();
  d.status_dev = nullptr;
  expect(run(config(), d) == SMX_ERR_INVALID && contains(why, "status row"), "a null status row");
  d = table();
  d.entered_count = TOTAL - 1;
  expect(run(config(), d) == SMX_ERR_INVALID && contains(why, "entered row") && contains(why, "out-of-bounds"), "a short entered row: " + why);
  smx_config none = config();
  none.num_social = N;
  expect(run(none, table()) == SMX_ERR_INVALID && contains(why, "no agents"), "a configuration without agents");
  for (size_t at : {(size_t)1, cells / 2 + 1, cells - 1}) {  // a late agent: the first, a middle and the very last cell
    fill();
    ready[at] = -1;
    expect(run(config(), table()) == SMX_ERR_INVALID && contains(why, "is negative") && contains(why, "agent 1"), "a negative tick: " + why);
    fill();
    ready[at] = std::numeric_limits<int32_t>::max();
    expect(run(config(), table()) == SMX_OK, "a tick that never comes is taken (the agent keeps its env open)");
    for (int q = 0; q < 3; ++q)
      for (double v : {NaN, Inf, -Inf}) {
        fill();
        chk[at * 3 + q] = v;
        expect(run(config(), table()) == SMX_ERR_INVALID && contains(why, "not finite"), "a check row that is not finite: " + why);
      }
    for (double v : {0.0, -1.0, -0.0}) {
      fill();
      chk[at * 3 + 2] = v;
      expect(run(config(), table()) == SMX_ERR_INVALID && contains(why, "must be > 0"), "a dimension <= 0: " + why);
    }
  }
  // every (row, env) needs an agent at tick 0: the last (row, env) of the table too
  fill();
  ready[cells - AGENTS] = 1;
  expect(run(config(), table()) == SMX_ERR_INVALID && contains(why, "row 1, env 1 has no agent at tick 0"), "no agent at tick 0: " + why);
  fill();
  ready[cells - AGENTS] = 1, ready[cells - 1] = 0;  // ... any agent will do
  expect(run(config(), table()) == SMX_OK, "the other agent at tick 0");
  delete[] ready;
  delete[] chk;
  delete[] status;
  delete[] entered;
}

// ---- (b) the handle
static int fake_knot_table(smx_handle_s* h, KnotRow* table) {
  std::memset(table, 0, (size_t)h->map.n_lanepoints * sizeof(KnotRow));
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}
static const KernelSide KERNELS = {352, 64 * 11 * 36, 0, fake_knot_table, nullptr};

struct World {
  smx_handle h = nullptr;
  smx_config cfg = config();
  Map map_a, map_b;
  std::vector<int32_t> ready = std::vector<int32_t>((size_t)ROWS * E * AGENTS, 0);
  std::vector<double> check = std::vector<double>((size_t)ROWS * E * AGENTS * 3, 3.68);
  std::vector<uint8_t> status = std::vector<uint8_t>(TOTAL);
  std::vector<int32_t> entered = std::vector<int32_t>(TOTAL);
  std::vector<double> frames{10.0, 1.0, 0.0, 5.0, /**/ 10.5, 1.0, 0.0, 5.0, /**/ 11.0, 1.0, 0.0, 5.0};  // 3 frames x 1 slot
  std::vector<int32_t> frame_vehicle{4, 4, -1}, start_frame = std::vector<int32_t>(ROWS * E, 0);
  std::vector<int32_t> follow = std::vector<int32_t>(ROWS * E * AGENTS, 4);
  std::vector<uint8_t> stack = std::vector<uint8_t>((size_t)TOTAL * STACK * 16 * 8 * 3);
  World() {
    for (size_t i = 0; i < ready.size(); ++i) ready[i] = (int32_t)(i % AGENTS) * 7;
  }
  smx_agent_entry entry(int rows = ROWS) {
    smx_agent_entry d{};
    d.ready_host = ready.data(), d.check_host = check.data(), d.rows = rows;
    d.status_dev = status.data(), d.entered_dev = entered.data(), d.status_count = TOTAL, d.entered_count = TOTAL;
    return d;
  }
  smx_social_history history() const {
    smx_social_history hs{};
    hs.frames_host = frames.data(), hs.vehicle_host = frame_vehicle.data(), hs.n_frames = 3, hs.num_social = SOCIAL;
    hs.start_frame_dev = start_frame.data(), hs.rows = ROWS, hs.start_count = start_frame.size();
    return hs;
  }
  smx_history_agents agents() {
    smx_history_agents ha{};
    ha.vehicle_dev = follow.data(), ha.vehicle_count = follow.size();
    return ha;
  }
};

static bool live_or_null(const void* p, size_t bytes) { return p == nullptr || shim_hip.inside(p, bytes); }
// the committed binding: the blob holds the ready ticks, then (8-byte aligned) the check rows, copied whole
static bool entry_bound(const World& w, int rows = ROWS) {
  const smx_handle_s* h = w.h;
  const size_t cells = (size_t)rows * E * AGENTS;
  return h->entry_blob && h->entry.ready == h->entry_blob.get<int32_t>() && h->entry.rows == rows &&
         shim_hip.inside(h->entry.ready, cells * sizeof(int32_t)) && shim_hip.inside(h->entry.check, cells * 3 * sizeof(double)) &&
         ((uintptr_t)h->entry.check & 7) == 0 && (const char*)h->entry.check >= (const char*)h->entry.ready + cells * sizeof(int32_t) &&
         std::memcmp(h->entry.ready, w.ready.data(), cells * sizeof(int32_t)) == 0 &&
         std::memcmp(h->entry.check, w.check.data(), cells * 3 * sizeof(double)) == 0 && h->entry.status == w.status.data() &&
         h->entry.entered == w.entered.data();
}
static bool entry_none(const smx_handle_s* h) {
  return !h->entry_blob && !h->entry.ready && !h->entry.check && h->entry.rows == 0 && !h->entry.status && !h->entry.entered;
}
// what holds after every call, failed or not
static void check_handle(const smx_handle_s* h) {
  if (!h) return;
  expect((h->entry.ready != nullptr) == (bool)h->entry_blob, "the tables with their blob");
  expect(!h->entry.ready || (live_or_null(h->entry.ready, (size_t)h->entry.rows * E * AGENTS * sizeof(int32_t)) &&
                             live_or_null(h->entry.check, (size_t)h->entry.rows * E * AGENTS * 3 * sizeof(double))),
         "entry.ready / check are null or live allocations of their size");
  expect(!(h->entry.ready && h->history.follow), "never entry and history agents at once");
  expect(!(h->entry.ready && !h->stacks.empty()), "never entry and a frame stack at once");
  const DeviceBlob* blobs[] = {&h->map_blob, &h->knots_blob, &h->spill_blob, &h->knot_table, &h->knot_stats, &h->alive_blob, &h->pending_blob, &h->slow_blob,
                               &h->scan_carry, &h->ctrl_blob, &h->status_dev, &h->vias_dev, &h->via_off_dev, &h->missions_blob, &h->goals_blob,
                               &h->history_blob, &h->ogm_mask, &h->dims_blob, &h->agent_dims_blob, &h->entry_blob};
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

static std::vector<Step> sequence() {
  std::vector<Step> s;
  auto bind = [](World& w) {
    const smx_agent_entry d = w.entry();
    return set_agent_entry_impl(w.h, &d);
  };
  auto nothing = [](World&) {};
  s.push_back({"smx_create", [](World& w) { return create_impl(&w.cfg, 0, &w.h, KERNELS); },
               [](World& w) { expect(entry_none(w.h) && !w.h->entry_reset_needed, "nothing bound, nothing to wait for"); }});
  s.push_back({"smx_set_agent_entry before a map", bind, [](World& w) { expect(entry_bound(w), "bound without a map"); }});
  s.push_back({"smx_load_map", [](World& w) { return load_map_impl(w.h, &w.map_a.t); },
               [](World& w) { expect(w.h->map_loaded && entry_none(w.h), "a new map drops the entry table"); }});
  s.push_back({"smx_set_agent_entry", bind, [](World& w) {
                 expect(entry_bound(w) && w.h->entry_reset_needed, "bound: steps wait for a reset of every env");
                 w.h->entry_reset_needed = false;  // (what enqueue does for smx_reset with env_mask NULL)
               }});
  s.push_back({"smx_set_agent_entry (rebind, one row)", [](World& w) {
                 w.ready[1] = 3;  // (the caller's table changes; the copy taken is the new one)
                 const smx_agent_entry d = w.entry(1);
                 return set_agent_entry_impl(w.h, &d);
               }, [](World& w) { expect(entry_bound(w, 1), "rebound with one row, the new ticks"); }});
  s.push_back({"smx_set_social_history", [](World& w) {
                 const smx_social_history hs = w.history();
                 return set_social_history_impl(w.h, &hs);
               }, [](World& w) { expect(entry_bound(w, 1) && w.h->history.vehicle, "a history keeps the entry table"); }});
  s.push_back({"smx_set_history_agents (refused: entry bound)", [](World& w) {
                 const smx_history_agents ha = w.agents();
                 const int rc = set_history_agents_impl(w.h, &ha);
                 expect(rc == SMX_ERR_STATE && contains(w.h->err, "delayed agent entry is bound"), "history agents are refused: " + w.h->err);
                 return rc == SMX_ERR_STATE ? (int)SMX_OK : rc;
               }, [](World& w) { expect(entry_bound(w, 1) && !w.h->history.follow, "... and nothing changed"); }});
  s.push_back({"smx_bind_frame_stack (refused: entry bound)", [](World& w) {
                 const int rc = bind_frame_stack_impl(w.h, SMX_STACK_SOURCE_RGB, SMX_STACK_FRAMES, w.stack.data(), w.stack.size());
                 expect(rc == SMX_ERR_STATE && contains(w.h->err, "delayed agent entry is bound"), "a frame stack is refused: " + w.h->err);
                 return rc == SMX_ERR_STATE ? (int)SMX_OK : rc;
               }, [](World& w) { expect(entry_bound(w, 1) && w.h->stacks.empty(), "... and nothing changed"); }});
  s.push_back({"smx_set_agent_entry (unbind)", [](World& w) { return set_agent_entry_impl(w.h, nullptr); }, [](World& w) {
                 expect(entry_none(w.h) && w.h->entry_reset_needed, "unbound: steps wait for a reset of every env");
                 w.h->entry_reset_needed = false;
               }});
  s.push_back({"smx_set_agent_entry (unbind again)", [](World& w) { return set_agent_entry_impl(w.h, nullptr); },
               [](World& w) { expect(!w.h->entry_reset_needed, "an unbind of nothing changes no episode"); }});
  s.push_back({"smx_set_history_agents", [](World& w) {
                 const smx_history_agents ha = w.agents();
                 return set_history_agents_impl(w.h, &ha);
               }, [](World& w) { expect(w.h->history.follow != nullptr, "history agents bound"); }});
  s.push_back({"smx_set_agent_entry (refused: history agents)", [](World& w) {
                 const smx_agent_entry d = w.entry();
                 const int rc = set_agent_entry_impl(w.h, &d);
                 expect(rc == SMX_ERR_STATE && contains(w.h->err, "history agents are bound"), "entry is refused: " + w.h->err);
                 return rc == SMX_ERR_STATE ? (int)SMX_OK : rc;
               }, [](World& w) { expect(entry_none(w.h) && w.h->history.follow, "... and nothing changed"); }});
  s.push_back({"smx_set_history_agents (unbind)", [](World& w) { return set_history_agents_impl(w.h, nullptr); }, nothing});
  s.push_back({"smx_bind_frame_stack", [](World& w) { return bind_frame_stack_impl(w.h, SMX_STACK_SOURCE_RGB, SMX_STACK_FRAMES, w.stack.data(), w.stack.size()); },
               [](World& w) { expect(w.h->stacks.size() == 1, "a frame stack bound"); }});
  s.push_back({"smx_set_agent_entry (refused: frame stack)", [](World& w) {
                 const smx_agent_entry d = w.entry();
                 const int rc = set_agent_entry_impl(w.h, &d);
                 expect(rc == SMX_ERR_STATE && contains(w.h->err, "frame stack is bound"), "entry is refused: " + w.h->err);
                 return rc == SMX_ERR_STATE ? (int)SMX_OK : rc;
               }, [](World& w) { expect(entry_none(w.h) && w.h->stacks.size() == 1, "... and nothing changed"); }});
  s.push_back({"smx_bind_frame_stack (unbind)", [](World& w) { return bind_frame_stack_impl(w.h, SMX_STACK_SOURCE_RGB, SMX_STACK_FRAMES, nullptr, 0); }, nothing});
  s.push_back({"smx_set_agent_entry (last)", bind, [](World& w) { expect(entry_bound(w), "bound again"); }});
  s.push_back({"smx_load_map (second)", [](World& w) {
                 if (w.h->entry.ready) w.h->entry_reset_needed = false;  // (a retry after a failed call finds it dropped and set)
                 return load_map_impl(w.h, &w.map_b.t);
               }, [](World& w) { expect(entry_none(w.h) && w.h->entry_reset_needed, "a new map drops it; steps wait for a reset"); }});
  s.push_back({"smx_set_agent_entry (after the map)", bind, nothing});
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
    // what a failed bind must leave: the binding that was in place (fill, then commit)
    const bool had = w.h && w.h->entry.ready;
    const int had_rows = had ? w.h->entry.rows : 0;
    const void* had_blob = had ? w.h->entry_blob.p : nullptr;
    int rc = s.call(w);
    if (armed && shim_hip.fired) {
      if (shim_hip.fired_in_release) {
        ++tally.release_points;
        expect(rc == SMX_OK, "a failed release does not fail the call");
      } else {
        ++tally.refused;
        expect(rc == SMX_ERR_HIP, "the call that contained the failed HIP call returns SMX_ERR_HIP, not " + std::to_string(rc));
        check_handle(w.h);
        if (w.h && had && w.h->entry.ready)
          expect(w.h->entry_blob.p == had_blob && w.h->entry.rows == had_rows, "a failed call leaves the binding in place as it was");
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

// a refused table through the handle: the binding in place stays
static void handle_refusals() {
  context = "handle refusals";
  shim_hip.reset();
  World w;
  expect(create_impl(&w.cfg, 0, &w.h, KERNELS) == SMX_OK, "create");
  const smx_agent_entry good = w.entry();
  expect(set_agent_entry_impl(w.h, &good) == SMX_OK && entry_bound(w), "bind");
  const void* blob = w.h->entry_blob.p;
  std::vector<int32_t> bad = w.ready;
  bad[0] = 4;  // (row 0, env 0 has no agent at tick 0 now)
  smx_agent_entry late = good;
  late.ready_host = bad.data();
  expect(set_agent_entry_impl(w.h, &late) == SMX_ERR_INVALID && contains(w.h->err, "no agent at tick 0"), "refused with a reason: " + w.h->err);
  expect(w.h->entry_blob.p == blob && entry_bound(w), "... and the binding in place stays");
  expect(set_agent_entry_impl(nullptr, &good) == SMX_ERR_INVALID, "a null handle");
  destroy_impl(w.h);
  expect(shim_hip.live.empty(), "nothing is live");
}

int main() {
  check_refusals();
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

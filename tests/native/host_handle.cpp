// Stand-alone host program over smarts_amd/csrc/smx_handle.h, the handle of the C-ABI and what it owns
// (tests/test_host_handle.py builds it with -fsanitize=address,undefined and runs it), over shim/hip_memory.h: device
// memory is recorded malloc, and one counter makes the n-th HIP call fail.
//   (a) clean run: create, load the hand-written map twice, bind everything, rebind; after each call the drop rule,
//       field by field; after smx_destroy nothing is live.
//   (b) failure sweep: the same sequence once for every HIP call of the clean run, that call failing.  The ABI call that
//       contained it returns SMX_ERR_HIP, every pointer a kernel would get is null or inside a live allocation,
//       map_loaded is false unless the map blob is whole, the same call succeeds when repeated, and the rest of the
//       sequence and smx_destroy leave nothing live.  (A failing release — hipFree, a destroy, the stream
//       synchronisation of smx_destroy — is ignored by design: the call succeeds and the object is released.)
// Prints one JSON line and returns 0 when every check held, else prints the failed checks and returns 1.
#include <hip_memory.h>  // the stand-in (and through it the shim <hip/hip_runtime.h>): plain C++

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "smx_handle.h"
#include "tiny_map.h"

static int failures = 0, checks = 0;
static std::string context;  // which run, which step
static void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    std::printf("FAILED [%s]: %s\n", context.c_str(), what.c_str());
  }
}

// the launch of smx_load_map, stood in: the table and the counters it is given are live and of the size the kernel
// writes, the map it reads is the new one; then the synchronisation that follows the launch
static int fake_knot_table(smx_handle_s* h, KnotRow* table) {
  expect(shim_hip.inside(table, (size_t)h->map.n_lanepoints * sizeof(KnotRow)) && shim_hip.inside(h->knot_stats.p, 4 * sizeof(int32_t)),
         "k_knot_table's table and counters are live allocations of their size");
  expect(h->map_blob && shim_hip.inside(h->map.lp_rec, (size_t)h->map.n_lanepoints * sizeof(smx_lp_rec)), "... and the map it reads is committed");
  std::memset(table, 0, (size_t)h->map.n_lanepoints * sizeof(KnotRow));
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}
static const KernelSide KERNELS = {352, 64 * 11 * 36, 0, fake_knot_table};

enum { E = 2, N = 3, SOCIAL = 1, AGENTS = N - SOCIAL, TOTAL = E * N, STACK = 2, ROWS = 2 };
static smx_config config() {
  smx_config c{};
  c.num_envs = E, c.num_vehicles = N, c.dt = 0.1, c.num_social = SOCIAL, c.social_speed_factor = 1.0;
  c.action_space = SMX_ACTION_SPACE_IMITATION;  // (history agents)
  c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_OGM | SMX_SENSOR_RGB;
  c.wp_lookahead = 32, c.wp_paths = 4, c.wp_len = 20, c.nb_radius = 50.0;
  c.ogm_width = 16, c.ogm_height = 16, c.ogm_resolution = 0.5;
  c.rgb_width = 16, c.rgb_height = 8, c.rgb_resolution = 0.5;
  c.via_max = 4, c.frame_stack = STACK;
  return c;
}

// everything the calls are given; the "device" buffers of the caller are host memory the handle only keeps pointers to
struct World {
  smx_handle h = nullptr;
  smx_config cfg = config();
  Map map_a, map_b;
  std::vector<smx_via> vias{{10.0, 0.0, 2.0, 5.0, 0, 0}, {40.0, 1.0, 2.0, 5.0, 2, 0}};
  std::vector<int32_t> via_off{0, 1, 2, 2};
  std::vector<smx_mission> missions{{50.0, 1.0, 2.0, 0, 2}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
  std::vector<int32_t> route_roads{0, 1};
  std::vector<smx_mission_goal> goals{{SMX_GOAL_LAP, 2, 60.0}, {SMX_GOAL_TRAVERSE, 0, 0.0}, {SMX_GOAL_POSITIONAL, 0, 0.0}};
  std::vector<double> lane_end_heading{0.0, 0.0, 0.0};
  std::vector<int32_t> lane_dead_end{0, 0, 1};
  std::vector<double> frames{10.0, 1.0, 0.0, 5.0, /**/ 10.5, 1.0, 0.0, 5.0, /**/ 11.0, 1.0, 0.0, 5.0};  // 3 frames x 1 slot
  std::vector<int32_t> frame_vehicle{4, 4, -1}, start_frame = std::vector<int32_t>(ROWS * E, 0);
  std::vector<double> dims = std::vector<double>(5 * 3, 2.0);  // ids 0..4
  std::vector<int32_t> follow = std::vector<int32_t>(ROWS * E * AGENTS, 4), handover = std::vector<int32_t>(ROWS * E * AGENTS, -1);
  std::vector<float> expert = std::vector<float>(3 * TOTAL);
  std::vector<uint8_t> ha_status = std::vector<uint8_t>(TOTAL), guard = std::vector<uint8_t>(TOTAL);
  std::vector<uint8_t> rgb = std::vector<uint8_t>((size_t)TOTAL * 16 * 8 * 3), stack = std::vector<uint8_t>((size_t)TOTAL * STACK * 16 * 8 * 3);
  smx_social_history history() const {
    smx_social_history hs{};
    hs.frames_host = frames.data(), hs.vehicle_host = frame_vehicle.data(), hs.n_frames = 3, hs.num_social = SOCIAL;
    hs.start_frame_dev = start_frame.data(), hs.rows = ROWS, hs.start_count = start_frame.size();
    return hs;
  }
  smx_history_agents agents(bool rows) {
    smx_history_agents ha{};
    ha.vehicle_dev = follow.data(), ha.vehicle_count = follow.size();
    if (rows) ha.action_dev = expert.data(), ha.action_count = expert.size(), ha.status_dev = ha_status.data(), ha.status_count = ha_status.size();
    return ha;
  }
};

// ---- what must hold of a handle after every call, failed or not
static bool live_or_null(const void* p, size_t bytes = 1) { return p == nullptr || shim_hip.inside(p, bytes); }
static void check_handle(const smx_handle_s* h) {
  if (!h) return;
  const size_t paths = (size_t)TOTAL * SMX_WP_LANES;
  // the map: whole in its blob, or absent
  auto whole = shim_hip.live.find(h->map_blob.get<const char>());
  const bool map_whole = h->map_blob && whole != shim_hip.live.end() && whole->second == h->map_bytes;
  expect(!h->map_blob || map_whole, "the map blob is a live allocation of map_bytes");
  expect(!h->map_loaded || map_whole, "map_loaded only with the map blob whole");
  if (map_whole) {
#define IN_BLOB(field, type, count) \
  expect(h->map.field && shim_hip.inside(h->map.field, (size_t)(count) * sizeof(type)) && (const char*)h->map.field >= whole->first && (const char*)h->map.field <= whole->first + whole->second, "map." #field " lies in the map blob");
    SMX_MAP_TABLES(IN_BLOB, h->map)
#undef IN_BLOB
  } else {
#define IS_NULL(field, type, count) expect(h->map.field == nullptr, "map." #field " is null without a map blob");
    SMX_MAP_TABLES(IS_NULL, h->map)
#undef IS_NULL
  }
  if (h->map_loaded)
    expect(h->alive_blob && h->slow_blob && h->pending_blob && h->scan_carry && h->knots_blob && h->knot_table && h->knot_stats && h->spill_blob &&
               h->status_dev && h->ctrl_blob && h->streams.ready && h->knots.idx && h->ctrl.path,
           "a loaded map comes with the batch's storage, the knot table and the side streams");
  expect(live_or_null(h->map.route_pos, (size_t)N * 2 * sizeof(int16_t)) && live_or_null(h->map.route_lane_ok, (size_t)N * 3), "map.route_pos / route_lane_ok");
  // (a load that failed before it reached the drop leaves the old map's missions in their blob, out of reach: every
  // entry point asks map_loaded first and the next load drops them)
  expect((h->missions.route_last != nullptr) == (bool)h->missions_blob && (h->missions.goal != nullptr) == (bool)h->missions_blob &&
             (!map_whole || ((h->map.route_pos != nullptr) == (bool)h->missions_blob && (h->map.route_lane_ok != nullptr) == (bool)h->missions_blob)),
         "the four route pointers are set together, with their blob");
  expect(live_or_null(h->missions.goal, N * 3 * sizeof(double)) && live_or_null(h->missions.route_last, N * sizeof(int32_t)), "missions.goal / route_last");
  expect(live_or_null(h->missions.goal_kind, N * sizeof(smx_mission_goal)) && (h->missions.goal_kind != nullptr) == (bool)h->goals_blob, "missions.goal_kind, with its blob");
  expect(live_or_null(h->knots.idx, (SMX_WPK_CAP + 1) * paths * sizeof(int32_t)) && live_or_null(h->knots.D, paths * sizeof(double)) &&
             live_or_null(h->knots.n, paths * sizeof(int16_t)) && live_or_null(h->knots.nk, paths * sizeof(int16_t)) &&
             live_or_null(h->knots.end16, paths * sizeof(int32_t)) && live_or_null(h->knots.key, 3 * paths * sizeof(int32_t)) &&
             live_or_null(h->knots.cnt, paths) && live_or_null(h->knots.nk16, paths), "knots.*");
  expect((h->knots.idx != nullptr) == (bool)h->knots_blob && (h->knots.key != nullptr) == (bool)h->knots_blob && (h->knots.nk16 != nullptr) == (bool)h->knots_blob,
         "knots.* are set with their blob");
  expect(live_or_null(h->ctrl.path, (size_t)SMX_CTRL_WPS * 3 * TOTAL * sizeof(double)) && live_or_null(h->ctrl.n, TOTAL * sizeof(int32_t)) &&
             (h->ctrl.path != nullptr) == (bool)h->ctrl_blob && (h->ctrl.n != nullptr) == (bool)h->ctrl_blob, "ctrl.*, with their blob");
  expect(live_or_null(h->history.frames, 3 * SOCIAL * 4 * sizeof(double)) && live_or_null(h->history.vehicle, 3 * SOCIAL * sizeof(int32_t)) &&
             (h->history.vehicle != nullptr) == (bool)h->history_blob && (h->history.frames != nullptr) == (bool)h->history_blob, "history.*, with their blob");
  expect(live_or_null(h->dims.table, 5 * 3 * sizeof(double)) && live_or_null(h->dims.slot, TOTAL * 3 * sizeof(double)) &&
             (h->dims.table != nullptr) == (bool)h->dims_blob && (h->dims.slot != nullptr) == (bool)h->dims_blob, "dims.*, with their blob");
  const DeviceBlob* blobs[] = {&h->map_blob, &h->knots_blob, &h->spill_blob, &h->knot_table, &h->knot_stats, &h->alive_blob, &h->pending_blob, &h->slow_blob,
                               &h->scan_carry, &h->ctrl_blob, &h->status_dev, &h->vias_dev, &h->via_off_dev, &h->missions_blob, &h->goals_blob,
                               &h->history_blob, &h->ogm_mask, &h->dims_blob};
  size_t owned = 0;
  for (const DeviceBlob* b : blobs) {
    expect(!*b || shim_hip.live.count(b->get<const char>()) == 1, "every blob of the handle is empty or a live allocation");
    owned += (bool)*b;
  }
  expect(owned == shim_hip.live.size(), "every live allocation has its owner in the handle (" + std::to_string(owned) + " of " + std::to_string(shim_hip.live.size()) + ")");
  expect((h->n_vias > 0) == (bool)h->vias_dev && (bool)h->vias_dev == (bool)h->via_off_dev, "the vias and their offsets come together");
  expect(h->streams.ready ? (shim_hip.streams.size() == 3 && shim_hip.events.size() == 5) : (shim_hip.streams.empty() && shim_hip.events.empty()),
         "three side streams and five events, or none of either");
  // no dependant without what it depends on
  expect(!h->history.follow || h->history.vehicle, "history agents only with a history");
  expect(!h->history.handover || h->history.follow, "a handover table only with history agents");
  expect(!(h->ha_action || h->ha_status) || h->history.follow, "action / status rows only with history agents");
  expect(!h->dims.table || h->history.vehicle, "dimensions only with a history");
  expect(!h->missions.goal_kind || !h->host_route_last.empty(), "goal kinds only after missions");
}

// ---- the sequence: one ABI call a step, and what the drop rule says of the handle after it
struct Step {
  const char* name;
  std::function<int(World&)> call;
  std::function<void(World&)> after;
};
static bool missions_bound(const smx_handle_s* h) { return h->missions_blob && h->missions.goal && h->missions.route_last && h->map.route_pos && h->map.route_lane_ok; }
static bool goals_bound(const smx_handle_s* h) { return h->goals_blob && h->missions.goal_kind; }
static bool history_bound(const smx_handle_s* h) { return h->history_blob && h->history.vehicle && h->history.frames && h->history.rows == ROWS; }
static bool dims_bound(const smx_handle_s* h) { return h->dims_blob && h->dims.table && h->dims.slot && h->dims.n_ids == 5; }
static bool agents_bound(const smx_handle_s* h) { return h->history.follow && h->history.n_agents == AGENTS; }
static bool kept_by_a_new_map(const World& w) {
  const smx_handle_s* h = w.h;
  return h->vias_dev && h->via_off_dev && h->n_vias == 2 && h->rgb_out == w.rgb.data() && h->rgb_count == w.rgb.size() && h->guard_out == w.guard.data() &&
         h->stacks.size() == 1 && h->stacks[0].dst == w.stack.data() && h->lidar_rays == w.frames.data();
}
static bool all_ff(const void* p, size_t bytes) {
  for (size_t i = 0; i < bytes; ++i)
    if (((const uint8_t*)p)[i] != 0xff) return false;
  return true;
}

static std::vector<Step> sequence() {
  std::vector<Step> s;
  auto missions = [](World& w) { return set_missions_impl(w.h, w.missions.data(), N, w.route_roads.data(), (int32_t)w.route_roads.size()); };
  auto goals = [](World& w) { return set_mission_goals_impl(w.h, w.goals.data(), N, w.lane_end_heading.data(), w.lane_dead_end.data(), 3); };
  auto history = [](World& w) {
    const smx_social_history hs = w.history();
    return set_social_history_impl(w.h, &hs);
  };
  auto dims = [](World& w) {
    const smx_social_dims d{w.dims.data(), 5};
    return set_social_history_dims_impl(w.h, &d);
  };
  auto agents = [](World& w) {
    const smx_history_agents ha = w.agents(true);
    return set_history_agents_impl(w.h, &ha);
  };
  auto handover = [](World& w) {
    const smx_history_handover ho{w.handover.data(), w.handover.size()};
    return set_history_handover_impl(w.h, &ho);
  };
  auto nothing = [](World&) {};
  auto all_bound = [](World& w) {
    expect(missions_bound(w.h) && goals_bound(w.h) && history_bound(w.h) && dims_bound(w.h) && agents_bound(w.h) && w.h->history.handover == w.handover.data() &&
               w.h->ha_action == w.expert.data() && w.h->ha_status == w.ha_status.data(), "missions, goals, history, dims, agents and handover are bound");
  };
  auto bind_all = [&](const char* tag) {
    (void)tag;
    s.push_back({"smx_set_missions", missions, [](World& w) { expect(missions_bound(w.h) && !goals_bound(w.h) && w.h->host_route_last == std::vector<int32_t>({1, -1, -1}), "missions bound, no goals yet"); }});
    s.push_back({"smx_set_mission_goals (lap, traverse)", goals, [](World& w) {
                   expect(goals_bound(w.h) && missions_bound(w.h), "goals bound beside the missions");
                   const char* base = w.h->goals_blob.get<const char>();  // all three tables were copied
                   expect(std::memcmp(base, w.goals.data(), N * sizeof(smx_mission_goal)) == 0 &&
                              std::memcmp(base + N * sizeof(smx_mission_goal), w.lane_end_heading.data(), 3 * sizeof(double)) == 0 &&
                              std::memcmp(base + N * sizeof(smx_mission_goal) + 3 * sizeof(double), w.lane_dead_end.data(), 3 * sizeof(int32_t)) == 0,
                          "goal kinds | lane end headings | dead-end lanes, as given");
                 }});
    s.push_back({"smx_set_social_history", history, [](World& w) {
                   expect(history_bound(w.h) && !dims_bound(w.h) && !agents_bound(w.h) && !w.h->history.handover && w.h->history_max_id == 4 && !w.h->list_ready,
                          "history bound, nothing that hangs on it");
                 }});
    s.push_back({"smx_set_social_history_dims", dims, [](World& w) { expect(dims_bound(w.h) && history_bound(w.h) && w.h->dims.slot[0] == SMX_CHASSIS_LENGTH, "dims bound, every slot the sedan's"); }});
    s.push_back({"smx_set_history_agents", agents, [](World& w) {
                   expect(agents_bound(w.h) && w.h->ha_action == w.expert.data() && w.h->ha_status == w.ha_status.data() && !w.h->history.handover && dims_bound(w.h),
                          "agents bound with their rows, no handover yet, dims untouched");
                 }});
    s.push_back({"smx_set_history_handover", handover, all_bound});
  };

  s.push_back({"smx_create", [](World& w) { return create_impl(&w.cfg, 0, &w.h, KERNELS); }, [](World& w) {
                 expect(w.h && w.h->ogm_mask && !w.h->map_loaded && w.h->wp_pool_limit == 352 && shim_hip.live.size() == 1 && shim_hip.live.begin()->second == w.h->ogm_mask_bytes,
                        "a handle with its OGM piece mask and nothing else");
               }});
  s.push_back({"smx_load_map", [](World& w) { return load_map_impl(w.h, &w.map_a.t); }, [](World& w) {
                 expect(w.h->map_loaded && w.h->map.n_lanes == 3 && !w.h->missions_blob && !w.h->history_blob && shim_hip.live.size() == 12, "the map and the batch's storage: twelve allocations");
                 expect(all_ff(w.h->knots.key, 3 * (size_t)TOTAL * SMX_WP_LANES * sizeof(int32_t)) && all_ff(w.h->scan_carry.p, 6 * TOTAL * sizeof(double)) &&
                            w.h->alive_blob.get<int32_t>()[alive_layout(w.cfg).size - 1] == 0, "knot keys and scan carries all ones, the alive list zero");
               }});
  s.push_back({"smx_set_vias", [](World& w) { return set_vias_impl(w.h, w.vias.data(), 2, w.via_off.data()); }, [](World& w) {
                 expect(w.h->n_vias == 2 && std::memcmp(w.h->vias_dev.p, w.vias.data(), 2 * sizeof(smx_via)) == 0 && w.h->via_off_dev.get<int32_t>()[N] == 2, "vias copied");
               }});
  bind_all("first");
  // the caller's buffers: no HIP call in any of them
  s.push_back({"smx_set_lidar_rays", [](World& w) { return set_lidar_rays_impl(w.h, w.frames.data(), 0); }, nothing});
  s.push_back({"smx_set_rgb_output", [](World& w) { return set_rgb_output_impl(w.h, w.rgb.data(), w.rgb.size()); }, nothing});
  s.push_back({"smx_set_guard", [](World& w) { return set_guard_impl(w.h, w.guard.data(), w.guard.size(), 10.0); }, nothing});
  s.push_back({"smx_bind_frame_stack", [](World& w) { return bind_frame_stack_impl(w.h, SMX_STACK_SOURCE_RGB, SMX_STACK_FRAMES, w.stack.data(), w.stack.size()); },
               [](World& w) { expect(kept_by_a_new_map(w), "vias, lidar rays, image, guard and frame stack are bound"); }});
  // a new map drops missions, goals, history, dims, agents and handover; keeps the rest
  s.push_back({"smx_load_map (second)", [](World& w) {
                 w.h->list_ready = true;  // (a new map leaves the carried list's flag alone)
                 return load_map_impl(w.h, &w.map_b.t);
               }, [](World& w) {
                 const smx_handle_s* h = w.h;
                 expect(h->map_loaded && !h->missions_blob && !h->missions.goal && !h->missions.route_last && !h->map.route_pos && !h->map.route_lane_ok && h->host_route_last.empty(), "a new map drops the missions");
                 expect(!h->goals_blob && !h->missions.goal_kind, "... the goals");
                 expect(!h->history_blob && !h->history.vehicle && !h->history.frames && h->history.rows == 0, "... the history");
                 expect(!h->dims_blob && !h->dims.table && !h->dims.slot, "... the dimensions");
                 expect(!h->history.follow && h->history.n_agents == 0 && !h->ha_action && !h->ha_status, "... the history agents and their rows");
                 expect(!h->history.handover, "... the handover table");
                 expect(kept_by_a_new_map(w) && h->guard_margin == 10.0 && h->list_ready, "and keeps vias, lidar rays, image, guard and frame stacks");
                 expect(shim_hip.live.size() == 14, "one map blob, one knot table: fourteen allocations with the vias");
               }});
  bind_all("second");
  // new missions drop the goals and invalidate the knot keys
  s.push_back({"smx_set_missions (again)", [missions](World& w) {
                 std::memset(w.h->knots.key, 0, 8);  // (a walked list)
                 return missions(w);
               }, [](World& w) {
                 expect(missions_bound(w.h) && !w.h->goals_blob && !w.h->missions.goal_kind, "new missions drop the goals");
                 expect(all_ff(w.h->knots.key, 3 * (size_t)TOTAL * SMX_WP_LANES * sizeof(int32_t)), "... and invalidate the knot keys");
                 expect(history_bound(w.h) && dims_bound(w.h) && agents_bound(w.h) && w.h->history.handover, "... and nothing of the history");
               }});
  s.push_back({"smx_set_mission_goals (again)", goals, [](World& w) { expect(goals_bound(w.h), "goals bound again"); }});
  // history agents, bind or unbind, drop the handover table and the rows
  s.push_back({"smx_set_history_agents (again, without rows)", [](World& w) {
                 const smx_history_agents ha = w.agents(false);
                 return set_history_agents_impl(w.h, &ha);
               }, [](World& w) {
                 expect(agents_bound(w.h) && !w.h->history.handover && !w.h->ha_action && !w.h->ha_status, "a new follow table drops the handover table and the rows");
                 expect(history_bound(w.h) && dims_bound(w.h) && missions_bound(w.h) && goals_bound(w.h), "... and nothing else");
               }});
  s.push_back({"smx_set_history_handover (again)", handover, [](World& w) { expect(w.h->history.handover == w.handover.data(), "handover bound again"); }});
  s.push_back({"smx_set_history_agents (unbind)", [](World& w) { return set_history_agents_impl(w.h, nullptr); }, [](World& w) {
                 expect(!w.h->history.follow && w.h->history.n_agents == 0 && !w.h->history.handover && !w.h->ha_action && !w.h->ha_status && history_bound(w.h) && dims_bound(w.h),
                        "unbinding the agents drops the handover table, keeps history and dims");
               }});
  s.push_back({"smx_set_history_agents (third)", agents, nothing});
  s.push_back({"smx_set_history_handover (third)", handover, all_bound});
  // a new history, bind or unbind, drops dims, agents and handover and clears list_ready
  s.push_back({"smx_set_social_history (again)", [history](World& w) {
                 w.h->list_ready = true;
                 return history(w);
               }, [](World& w) {
                 expect(history_bound(w.h) && !w.h->dims_blob && !w.h->dims.table && !w.h->dims.slot, "a new history drops the dimensions");
                 expect(!w.h->history.follow && w.h->history.n_agents == 0 && !w.h->ha_action && !w.h->ha_status && !w.h->history.handover, "... the agents, their rows and the handover table");
                 expect(!w.h->list_ready && missions_bound(w.h) && goals_bound(w.h), "... clears list_ready, keeps the missions");
               }});
  s.push_back({"smx_set_social_history_dims (again)", dims, nothing});
  s.push_back({"smx_set_history_agents (fourth)", agents, nothing});
  s.push_back({"smx_set_history_handover (fourth)", handover, all_bound});
  s.push_back({"smx_set_social_history (unbind)", [](World& w) {
                 w.h->list_ready = true;
                 return set_social_history_impl(w.h, nullptr);
               }, [](World& w) {
                 expect(!w.h->history_blob && !w.h->history.vehicle && !w.h->dims_blob && !w.h->dims.table && !w.h->history.follow && !w.h->history.handover && !w.h->ha_action &&
                            !w.h->ha_status && !w.h->list_ready, "unbinding the history drops everything that hangs on it");
               }});
  s.push_back({"smx_set_social_history (last)", history, nothing});
  s.push_back({"smx_set_social_history_dims (last)", dims, nothing});
  s.push_back({"smx_set_vias (clear)", [](World& w) { return set_vias_impl(w.h, nullptr, 0, nullptr); }, [](World& w) { expect(!w.h->vias_dev && !w.h->via_off_dev && w.h->n_vias == 0, "vias cleared"); }});
  s.push_back({"smx_set_vias (last)", [](World& w) { return set_vias_impl(w.h, w.vias.data(), 2, w.via_off.data()); }, nothing});
  s.push_back({"smx_bind_frame_stack (unbind)", [](World& w) { return bind_frame_stack_impl(w.h, SMX_STACK_SOURCE_RGB, SMX_STACK_FRAMES, nullptr, 0); }, [](World& w) { expect(w.h->stacks.empty(), "stack unbound"); }});
  s.push_back({"smx_destroy", [](World& w) {
                 destroy_impl(w.h);
                 w.h = nullptr;
                 return (int)SMX_OK;
               }, [](World&) { expect(shim_hip.live.empty() && shim_hip.streams.empty() && shim_hip.events.empty(), "after smx_destroy no allocation, stream or event is live"); }});
  return s;
}

struct Tally {
  long refused = 0, release_points = 0, skipped = 0;
};

// the whole sequence with HIP call `fail_at` failing (0: none)
static void run(const std::vector<Step>& steps, long fail_at, Tally& tally) {
  shim_hip.reset();
  shim_hip.fail_at = fail_at;
  World w;
  for (const Step& s : steps) {
    context = (fail_at ? "call " + std::to_string(fail_at) + " fails" : std::string("clean")) + ", " + s.name;
    const bool armed = !shim_hip.fired;
    if (shim_hip.trace) shim_hip.trace = s.name;
    const long first_call = shim_hip.calls + 1;
    int rc = s.call(w);
    if (armed && shim_hip.fired) {
      if (shim_hip.fired_in_release) {  // (ignored by design: nothing to do about a release that fails)
        ++tally.release_points;
        expect(rc == SMX_OK, "a failed release does not fail the call");
      } else {
        ++tally.refused;
        expect(rc == SMX_ERR_HIP, "the call that contained the failed HIP call returns SMX_ERR_HIP, not " + std::to_string(rc));
        expect(w.h ? !w.h->err.empty() : !g_create_err.empty(), "... with a reason");
        check_handle(w.h);
        // (its first call, hipSetDevice, fails before anything of the old map is touched)
        expect(w.h == nullptr || !w.h->map_loaded || std::string(s.name).find("smx_load_map") == std::string::npos || fail_at == first_call,
               "a smx_load_map that failed after releasing the old map leaves no map loaded");
        rc = s.call(w);
        expect(rc == SMX_OK, "repeating the failed call without the fault succeeds (" + std::to_string(rc) + (w.h ? ": " + w.h->err : "") + ")");
      }
    } else {
      expect(rc == SMX_OK, "the call succeeds (" + std::to_string(rc) + (w.h ? ": " + w.h->err : ": " + g_create_err) + ")");
    }
    if (rc != SMX_OK) break;  // (reported above; the steps after it would only repeat it)
    check_handle(w.h);
    s.after(w);
  }
  if (w.h) destroy_impl(w.h);
  context = fail_at ? "call " + std::to_string(fail_at) + " fails, at the end" : "clean, at the end";
  if (fail_at && !shim_hip.fired) ++tally.skipped;
  expect(shim_hip.live.empty() && shim_hip.streams.empty() && shim_hip.events.empty(), "nothing is live at the end");
  expect(shim_hip.misuse == 0, "no HIP call was given a pointer that is not live");
}

// `--trace`: the clean run prints every HIP call with its number (= the sweep point at which it fails) and its step
int main(int argc, char** argv) {
  const std::vector<Step> steps = sequence();
  Tally clean_tally, tally;
  if (argc > 1 && std::string(argv[1]) == "--trace") shim_hip.trace = "";
  run(steps, 0, clean_tally);
  shim_hip.trace = nullptr;
  const ShimHip clean = shim_hip;
  context = "clean";
  expect(clean.mallocs > 0 && clean.memcpys > 0 && clean.memsets > 0 && clean.frees > 0 && clean.stream_creates == 3 && clean.event_creates == 5,
         "the clean run made calls of every kind");
  expect(clean.mallocs == clean.frees, "as many frees as allocations");
  long points = 0;
  for (long n = 1; n <= clean.calls; ++n, ++points) run(steps, n, tally);
  context = "sweep";
  expect(points == clean.calls, "one sweep point for every HIP call of the clean run");
  expect(tally.skipped == 0 && tally.refused + tally.release_points == points, "every point's fault fired");
  if (failures) return 1;
  std::printf("{\"checks\": %d, \"steps\": %d, \"hip_calls\": %ld, \"sweep_points\": %ld, \"refused\": %ld, \"release_points\": %ld, \"skipped\": %ld, "
              "\"mallocs\": %ld, \"memcpys\": %ld, \"memsets\": %ld, \"frees\": %ld, \"stream_creates\": %ld}\n",
              checks, (int)steps.size(), clean.calls, points, tally.refused, tally.release_points, tally.skipped, clean.mallocs, clean.memcpys, clean.memsets,
              clean.frees, clean.stream_creates);
  return 0;
}

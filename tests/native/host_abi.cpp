// Stand-alone host program over smarts_amd/csrc/smx_host.h, the device-free half of the C-ABI (tests/test_host_abi.py
// builds it with -fsanitize=address,undefined and runs it): (a) the caller-buffer table seen by the frame stacks against
// the entry check, (b) the entry check over real heap buffers of exactly the needed size, (c) the frame-stack launch
// geometry, (d) config_error at the ends of int32, (e) map_tables_error and the table list on a hand-written map,
// (f) the route tables on that map.  Prints one JSON line and returns 0 when every check held, else prints the failed
// checks and returns 1.
#include <hip/hip_runtime.h>  // the shim: plain C++

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "smx_host.h"
#include "tiny_map.h"

static int failures = 0, checks = 0;
static volatile uint64_t sink;  // (keeps calls whose only point is to run under the sanitizers)
static void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    std::printf("FAILED: %s\n", what.c_str());
  }
}
static bool starts_with(const std::string& s, const std::string& head) { return s.compare(0, head.size(), head) == 0; }

// ---- the configurations of tests/golden/gen_golden_host_checks.py, 3 envs x 4 vehicles
static const uint32_t ALL_SENSORS = (1u << 10) - 1;
static smx_config shapes() {
  smx_config c{};
  c.num_envs = 3, c.num_vehicles = 4, c.dt = 0.1;
  c.wp_lookahead = 32, c.wp_paths = 4, c.wp_len = 20, c.nb_max = 10, c.nb_radius = 50.0;
  c.ogm_width = 64, c.ogm_height = 64, c.ogm_resolution = 0.5, c.lidar_rays = 100, c.lidar_max_distance = 20.0;
  c.dagm_width = 32, c.dagm_height = 32, c.dagm_resolution = 0.5;
  c.rw_horizon = 2, c.rw_lanes = 3, c.rw_paths = 2;
  c.rgb_width = 16, c.rgb_height = 8, c.rgb_resolution = 0.5;
  return c;
}
enum { EVERYTHING = 0, DECLARED, BARE, OVERSIZED, CONFIGS };
static const char* const CONFIG_NAMES[CONFIGS] = {"everything", "declared", "bare", "oversized"};
static smx_config sweep_config(int which) {
  smx_config c = shapes();
  if (which == EVERYTHING || which == OVERSIZED) c.via_max = 4, c.frame_stack = 4;
  if (which == EVERYTHING) c.sensors = ALL_SENSORS, c.num_social = 1, c.social_speed_factor = 1.0, c.done_criteria = SMX_DONE_NOT_MOVING;
  if (which == DECLARED) {
    c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_NEIGHBORS | SMX_SENSOR_OGM | SMX_SENSOR_LIDAR;
    c.dagm_width = c.dagm_height = c.rw_horizon = c.rw_lanes = c.rw_paths = c.rgb_width = c.rgb_height = 0;
  }
  if (which == BARE) {
    c.wp_lookahead = c.wp_paths = c.wp_len = c.nb_max = c.ogm_width = c.ogm_height = c.lidar_rays = 0;
    c.dagm_width = c.dagm_height = c.rw_horizon = c.rw_lanes = c.rw_paths = c.rgb_width = c.rgb_height = 0;
  }
  return c;
}
// is the output row's buffer given in the configuration (the generator's `given` sets)
static bool out_given(int which, int i) {
  if (which == EVERYTHING || which == OVERSIZED) return true;
  if (i <= SMX_OUT_ENV_DONE) return true;
  if (which == BARE) return false;
  return i == SMX_OUT_LEARNER || (i >= SMX_OUT_WP_POS && i <= SMX_OUT_LIDAR_POINT) || i == SMX_OUT_COLLIDEES;
}

// this file's own statement of include/smx.h: the sensor bits an output row needs (all of them), and the rows no stack takes
static uint32_t sensors_of(int i) {
  const uint32_t wp = SMX_SENSOR_WAYPOINTS, nb = SMX_SENSOR_NEIGHBORS, lidar = SMX_SENSOR_LIDAR, rw = SMX_SENSOR_ROAD_WAYPOINTS;
  const uint32_t ec = SMX_SENSOR_EGO_CENTRIC;
  if (i >= SMX_OUT_WP_POS && i <= SMX_OUT_WP_COUNT) return wp;
  if (i >= SMX_OUT_NB_POS && i <= SMX_OUT_NB_COUNT) return nb;
  if (i == SMX_OUT_OGM) return SMX_SENSOR_OGM;
  if (i == SMX_OUT_LIDAR_HIT || i == SMX_OUT_LIDAR_POINT) return lidar;
  if (i == SMX_OUT_DAGM) return SMX_SENSOR_DAGM;
  if (i >= SMX_OUT_RW_LANE_COUNT && i <= SMX_OUT_RW_LANE_ID) return rw;
  if (i == SMX_OUT_LANE_TTC || i == SMX_OUT_LANE_TTC_FLAGS) return SMX_SENSOR_LANE_TTC;
  if (i >= SMX_OUT_EGO_FRAME && i <= SMX_OUT_EC_EGO_F32) return ec;
  if (i == SMX_OUT_EC_WP_POS || i == SMX_OUT_EC_WP_HEADING) return ec | wp;
  if (i == SMX_OUT_EC_NB_POS || i == SMX_OUT_EC_NB_HEADING) return ec | nb;
  if (i == SMX_OUT_EC_LIDAR_POINT) return ec | lidar;
  if (i == SMX_OUT_EC_RW_POS || i == SMX_OUT_EC_RW_HEADING) return ec | rw;
  return 0;
}
static bool stackable(int i) {
  return i >= 0 && i < SMX_OUT_BUFFERS && i != SMX_OUT_ENV_DONE && i != SMX_OUT_LEARNER && !(i >= SMX_OUT_FINAL_EGO_POS && i <= SMX_OUT_FINAL_DIST);
}
static bool stack_source_on(const smx_config& c, int i) {
  const bool via = i >= SMX_OUT_VIA_NEAR && i <= SMX_OUT_VIA_HIT;
  return stackable(i) && (c.sensors & sensors_of(i)) == sensors_of(i) && (!via || c.via_max > 0);
}

// (a) stack_row_bytes x E*N = the entry check's elements x the size of the dtype, for every stackable source whose sensor is
// on; 0 with a message for every other source
static int case_table() {
  int on = 0;
  for (int which = 0; which < CONFIGS; ++which) {
    const smx_config c = sweep_config(which);
    const uint64_t T = (uint64_t)c.num_envs * c.num_vehicles;
    for (int s = -1; s <= SMX_OUT_BUFFERS; ++s) {
      std::string msg;
      const uint64_t row = stack_row_bytes(c, s, msg);
      const std::string tag = std::string(CONFIG_NAMES[which]) + " source " + std::to_string(s);
      if (stack_source_on(c, s)) {
        ++on;
        expect(row > 0 && msg.empty(), tag + ": a stackable row whose sensor is on has a size and no message");
        expect(row * T == row_elements(OUT_ROWS[s], c, 0) * dtype_size(OUT_ROWS[s].dtype), tag + ": the stack's row x E*N is what the entry check asks");
        expect(OUT_ROWS[s].unit == BUF_PER_AGENT && OUT_ROWS[s].sensors == sensors_of(s), tag + ": a per-agent row with the header's sensor bits");
      } else {
        expect(row == 0 && !msg.empty(), tag + ": refused with a message");
        expect(starts_with(msg, stackable(s) ? "frame stack: the sensor of source" : "frame stack: source"), tag + ": ... that says why");
      }
    }
    std::string msg;
    const uint64_t rgb = stack_row_bytes(c, SMX_STACK_SOURCE_RGB, msg);
    if (c.sensors & SMX_SENSOR_RGB)
      expect(rgb == (uint64_t)c.rgb_width * c.rgb_height * 3 && msg.empty(), "the image's row is width x height x 3");
    else
      expect(rgb == 0 && !msg.empty(), "the image with the sensor off is refused");
  }
  for (int i = 0; i < SMX_OUT_BUFFERS; ++i) expect(OUT_ROWS[i].stackable == stackable(i), "row " + std::to_string(i) + ": stackable as smx.h says");
  return on;
}

// (b) the entry check over heap buffers of exactly the needed size
struct Buffers {
  smx_state st{};
  smx_spawns sp{};
  smx_outputs out{};
  std::vector<void*> owned;
  ~Buffers() {
    for (void* p : owned) std::free(p);
  }
  // `elements` of the row's dtype, the last one touched: a table entry that overstates is an ASan report here
  void* make(const BufRow& r, uint64_t elements) {
    const size_t bytes = (size_t)(elements * dtype_size(r.dtype));
    char* p = (char*)std::malloc(bytes ? bytes : 1);
    if (bytes) p[bytes - dtype_size(r.dtype)] = 1;
    owned.push_back(p);
    return p;
  }
  template <class Struct>
  static void set(Struct& s, int index, void* p) { memcpy(reinterpret_cast<char*>(&s) + (size_t)index * sizeof(void*), &p, sizeof(p)); }
};
static void case_entry_check() {
  for (int which = 0; which < CONFIGS; ++which) {
    const smx_config c = sweep_config(which), sized_by = sweep_config(which == OVERSIZED ? EVERYTHING : which);
    const std::string tag = CONFIG_NAMES[which];
    Buffers b;
    b.sp.episodes = 2;
    for (const BufRow& r : STATE_ROWS) {
      if (r.index == SMX_ST_DRIVEN_PATH && which == BARE) continue;
      Buffers::set(b.st, r.index, b.make(r, row_elements(r, sized_by, 0)));
      b.st.count[r.index] = row_elements(r, sized_by, 0), b.st.dtype[r.index] = r.dtype;
    }
    b.sp.pose_count = row_elements(SPAWN_ROWS[0], sized_by, 2);
    b.sp.pose = (const double*)b.make(SPAWN_ROWS[0], b.sp.pose_count);
    if (which == EVERYTHING || which == OVERSIZED) {
      b.sp.social_count = row_elements(SPAWN_ROWS[1], sized_by, 2);
      b.sp.social = (const double*)b.make(SPAWN_ROWS[1], b.sp.social_count);
    }
    for (const BufRow& r : OUT_ROWS) {
      if (!out_given(which, r.index)) continue;
      Buffers::set(b.out, r.index, b.make(r, row_elements(r, sized_by, 0)));
      b.out.count[r.index] = row_elements(r, sized_by, 0), b.out.dtype[r.index] = r.dtype;
    }
    expect(b.st.f64 && b.st.env_reset_pending && b.out.ego_pos && buffer_ptr(b.out, SMX_OUT_ENV_DONE) == b.out.env_done &&
               buffer_ptr(b.st, SMX_ST_FLAGS) == b.st.flags, tag + ": pointer i of a struct is the member the enum names");
    std::string msg;
    for (const int has_vias : {0, 1}) expect(check_buffers_impl(c, has_vias != 0, &b.st, &b.sp, &b.out, msg) == SMX_OK && msg.empty(), tag + ": exact extents are accepted " + msg);
    // each buffer one element short of what this configuration needs: refused by its name
    auto short_of = [&](const BufRow& r, uint64_t& count, int32_t episodes) {
      const uint64_t need = row_elements(r, c, episodes), keep = count;
      if (need == 0) return;
      count = need - 1;
      msg.clear();
      expect(check_buffers_impl(c, true, &b.st, &b.sp, &b.out, msg) == SMX_ERR_INVALID && starts_with(msg, std::string(r.name) + ": " + std::to_string(need - 1) + " elements declared"),
             tag + ": " + r.name + " one element short is refused by name (" + msg + ")");
      count = keep;
    };
    for (const BufRow& r : STATE_ROWS)
      if (buffer_ptr(b.st, r.index)) short_of(r, b.st.count[r.index], 0);
    short_of(SPAWN_ROWS[0], b.sp.pose_count, 2);
    if (b.sp.social) short_of(SPAWN_ROWS[1], b.sp.social_count, 2);
    for (const BufRow& r : OUT_ROWS)
      if (buffer_ptr(b.out, r.index)) short_of(r, b.out.count[r.index], 0);
    msg.clear();
    expect(check_buffers_impl(c, true, &b.st, &b.sp, &b.out, msg) == SMX_OK, tag + ": and accepted again with the extents restored");
  }
  // the way out of the smx_check_* entry points: the message cut to the caller's buffer, the terminator kept
  char err[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  expect(report(SMX_ERR_INVALID, "null config", err, sizeof(err)) == SMX_ERR_INVALID && std::string(err) == "null co", "report cuts the message to err_len - 1");
  expect(report(SMX_OK, "", err, sizeof(err)) == SMX_OK && err[0] == 0, "report writes the empty message of a success");
  err[0] = 7;
  expect(report(-3, "x", err, 1) == -3 && err[0] == 0 && report(-3, "x", err, 0) == -3 && report(-3, "x", nullptr, 8) == -3, "report with one byte, none, no buffer");
}

// (c) the frame-stack launch geometry
static void case_geometry() {
  const uintptr_t base = 0x10000, offs[3] = {0, 4, 1};
  const uint64_t rows[5] = {16, 12, 4, 3, 1}, total = 1000;
  uint64_t blocks = 0;
  for (const uintptr_t so : offs)
    for (const uintptr_t dof : offs)
      for (const uint64_t row : rows) {
        const uint64_t before = blocks;
        const StackColumns s = stack_push_place(row, base + so, base + 0x4000 + dof, total, blocks);
        const bool by16 = so % 16 == 0 && dof % 16 == 0 && row % 16 == 0, by4 = so % 4 == 0 && dof % 4 == 0 && row % 4 == 0;
        const std::string tag = "src+" + std::to_string(so) + " dst+" + std::to_string(dof) + " row " + std::to_string(row);
        expect(s.unit == (by16 ? 16u : by4 ? 4u : 1u), tag + ": 16 only when both addresses and the row are multiples of 16, 4 likewise, else 1");
        expect(s.block0 == before && blocks > before, tag + ": block0 is where the earlier bindings end, and ascends");
        const uint64_t columns = total * (row / s.unit), mine = blocks - before;
        expect(mine * SMX_HOST_STACK_BLOCK >= columns && (mine - 1) * SMX_HOST_STACK_BLOCK < columns,
               tag + ": the last workgroup covers the last column, and none lies beyond it (the next binding starts there)");
      }
  expect(blocks < STACK_BLOCKS_CAP, "a launch of small rows fits");
  uint64_t at_cap = 0, below = 0;
  stack_push_place(1, 1, 1, (uint64_t)SMX_HOST_STACK_BLOCK << 31, at_cap);
  stack_push_place(1, 1, 1, ((uint64_t)SMX_HOST_STACK_BLOCK << 31) - SMX_HOST_STACK_BLOCK, below);
  expect(at_cap == STACK_BLOCKS_CAP && at_cap >= STACK_BLOCKS_CAP && below == STACK_BLOCKS_CAP - 1 && STACK_BLOCKS_CAP == (1ull << 31),
         "2^31 workgroups reach the cap, one fewer does not");
  // the interleaved image: a thread per four pixels
  expect(stack_dstack_blocks(3 * 128, 12) == (12 * 32 + 255) / 256 && stack_dstack_blocks(3 * 5, 1000) == (1000 * 2 + 255) / 256 &&
             stack_dstack_blocks(3 * 65536, 1ull << 25) >= STACK_BLOCKS_CAP, "k_frame_dstack's workgroups: ceil(pixels / 4) threads an agent");
}

// (d) config_error at the ends of int32: a message or none, never undefined behaviour
static int case_config_extremes() {
  int32_t smx_config::* const fields[] = {
      &smx_config::num_envs, &smx_config::num_vehicles, &smx_config::wp_lookahead, &smx_config::wp_paths, &smx_config::wp_len,
      &smx_config::nb_max, &smx_config::max_episode_steps, &smx_config::frame_stack, &smx_config::auto_reset, &smx_config::reset_elapsed_steps,
      &smx_config::ogm_width, &smx_config::ogm_height, &smx_config::lidar_rays, &smx_config::action_space, &smx_config::num_social,
      &smx_config::via_max, &smx_config::alive_min_ego, &smx_config::alive_min_total, &smx_config::alive_lists, &smx_config::dagm_width,
      &smx_config::dagm_height, &smx_config::social_model, &smx_config::rw_horizon, &smx_config::rw_lanes, &smx_config::rw_paths,
      &smx_config::rgb_width, &smx_config::rgb_height};
  const smx_config good = sweep_config(EVERYTHING);
  expect(config_error(good) == nullptr, "the everything-on configuration is valid");
  int refused = 0;
  const int32_t ends[2] = {std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()};
  auto probe = [&](const smx_config& c) {
    const char* why = config_error(c);
    refused += why != nullptr;
    expect(why == nullptr || why[0] != 0, "a refusal has a text");
    std::string msg;
    uint64_t sum = 0, row = 0;
    for (int s = -1; s <= SMX_OUT_BUFFERS; ++s) sum += stack_row_bytes(c, s, msg);  // (unsigned arithmetic throughout)
    sum += check_frame_stack_impl(c, SMX_STACK_SOURCE_RGB, SMX_STACK_DSTACK, 0, row, msg) + check_rgb_output_impl(c, 0, msg) + check_guard_impl(c, 0, 0.0, msg);
    for (const BufRow& r : OUT_ROWS) sum += row_elements(r, c, 1);
    sink = sink + sum;
  };
  for (auto field : fields)
    for (const int32_t v : ends) {
      smx_config c = good;
      c.*field = v;
      probe(c);
    }
  for (const int32_t v : ends) {  // every field at once: width x height = 2^62, 2^64 - 2^33 + 1 after the cast
    smx_config c = good;
    for (auto field : fields) c.*field = v;
    probe(c);
    for (int k = 0; k < 4; ++k) c.alive_list_min[k] = v;
    probe(c);
  }
  smx_config c = good;
  c.ogm_width = c.ogm_height = 65536;  // 2^32 cells: the int product was 0
  expect(config_error(c) != nullptr && starts_with(config_error(c), "ogm:"), "a grid of 2^32 cells is refused");
  return refused;
}

// (e), (f): the hand-written map of tiny_map.h

static void case_map_tables() {
  {
    Map m;
    expect(map_tables_error(m.t) == nullptr, "the hand-written map is accepted");
    expect(!map_lanes_split(m.t) && slow_list_blocks(false, 262144) == SMX_HOST_SLOW_BLOCKS, "no lanepoint with two successors: the small grid");
    expect(slow_list_blocks(true, 262144) == 8192 && slow_list_blocks(true, 1000) == SMX_HOST_SLOW_BLOCKS && slow_list_blocks(true, 1 << 30) == 8192,
           "where lanes split: a team slot for every second vehicle, between 512 and 8192 workgroups");
    m.lp[3].n_next = 2;
    expect(map_lanes_split(m.t), "a lanepoint with two successors: lanes split");
    expect(map_dagm_reach(m.t) == 1.75, "half the widest lane");
  }
  // each checked index in turn at -1 and at its count
  struct Bad {
    const char* what;
    void (*set)(Map&, int32_t);
    int32_t count;
    const char* message;
  };
  const Bad bad[] = {
      {"lp.lane", [](Map& m, int32_t v) { m.lp[5].lane = v; }, 3, "lanepoint record out of range"},
      {"lp.next0", [](Map& m, int32_t v) { m.lp[5].next0 = v; }, 12, "lanepoint record out of range"},
      {"lp.knot_next", [](Map& m, int32_t v) { m.lp[5].knot_next = v; }, 12, "lanepoint record out of range"},
      {"lp.next_off", [](Map& m, int32_t v) { m.lp[5].next_off = v; }, 11, "lanepoint record out of range"},
      {"succ.idx", [](Map& m, int32_t v) { m.succ[4].idx = v; }, 12, "successor record out of range"},
      {"succ.knot", [](Map& m, int32_t v) { m.succ[4].knot = v; }, 12, "successor record out of range"},
      {"succ.lane", [](Map& m, int32_t v) { m.succ[4].lane = v; }, 3, "successor record out of range"},
      {"sg.lane", [](Map& m, int32_t v) { m.sg[1].lane = v; }, 3, "segment record out of range"},
      {"sg.v0", [](Map& m, int32_t v) { m.sg[1].v0 = v; }, 5, "segment record out of range"},  // (v0 + 1 is a vertex too)
      {"lane_in_idx", [](Map& m, int32_t v) { m.lane_in_idx[1] = v; }, 3, "incoming lane out of range"},
      {"road_par_idx", [](Map& m, int32_t v) { m.road_par_idx[0] = v; }, 2, "parallel road out of range"},
  };
  for (const Bad& b : bad)
    for (const int32_t v : {-1, b.count}) {
      Map m;
      b.set(m, v);
      const char* why = map_tables_error(m.t);
      expect(why && std::string(why) == b.message, std::string(b.what) + " = " + std::to_string(v) + " is refused: " + (why ? why : "accepted"));
      Map ok;
      b.set(ok, b.count - 1);
      if (std::string(b.what) != "lp.next_off") expect(map_tables_error(ok.t) == nullptr, std::string(b.what) + ": the last index is accepted");
    }
  {
    Map m;
    m.succ[4].hops = 0;
    expect(std::string(map_tables_error(m.t)) == "successor record out of range", "a successor zero hops away is refused");
  }
  {
    Map m;
    m.t.n_lanes = 0;
    expect(std::string(map_tables_error(m.t)) == "empty map tables", "no lanes: empty");
    m.t.n_lanes = 32768;  // (refused before any table is read)
    expect(starts_with(map_tables_error(m.t), "lane ids are reported as int16"), "more lanes than an int16 names");
    m.t.n_lanes = 3, m.t.lane_in_off = nullptr;
    expect(std::string(map_tables_error(m.t)) == "map tables: lane_in_* / road_par_* missing", "the newer tables are required");
  }
  {  // the table list: every table lands in the blob whole, at a multiple of 256 bytes, in the list's order
    Map m;
    BlobWriter w;
    int tables = 0;
    size_t end = 0;
#define CHECK_TABLE(field, type, count)                                                                                   \
  {                                                                                                                       \
    const size_t bytes = (size_t)(count) * sizeof(type), off = w.add(m.t.field, bytes);                                   \
    expect(off % 256 == 0 && off >= end && w.host.size() == off + bytes && (bytes == 0 || memcmp(&w.host[off], m.t.field, bytes) == 0), \
           #field ": copied whole to an aligned offset");                                                                 \
    end = off + bytes, ++tables;                                                                                          \
  }
    SMX_MAP_TABLES(CHECK_TABLE, m.t)
#undef CHECK_TABLE
    expect(tables == 26, "26 tables");
  }
}

// (f) the route tables
static std::vector<uint8_t> lane_ok_of(const Map& m, const std::vector<int32_t>& filter_edge_ids) {
  // lanepoints.py:666-683, per lane: skipped unless on a road of the route; skipped when that is not the route's last road
  // and none of its outgoing lanes is on a road of the route
  auto in_filter = [&](int32_t road) { return std::find(filter_edge_ids.begin(), filter_edge_ids.end(), road) != filter_edge_ids.end(); };
  std::vector<uint8_t> ok(m.lane_road.size(), 0);
  for (size_t lane = 0; lane < m.lane_road.size(); ++lane) {
    const int32_t edge_id = m.lane_road[lane];
    if (!in_filter(edge_id)) continue;
    bool all_out_off_route = true;
    for (int k = m.lane_out_off[lane]; k < m.lane_out_off[lane + 1]; ++k) all_out_off_route = all_out_off_route && !in_filter(m.lane_road[m.lane_out_idx[k]]);
    if (edge_id != filter_edge_ids.back() && all_out_off_route) continue;
    ok[lane] = 1;
  }
  return ok;
}

static void case_routes() {
  const Map m;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const std::vector<int32_t> roads{0, 1, /* slot 1: */ 0, 1, 0, /* slot 3: */ 0};  // exactly what the missions name
  const std::vector<smx_mission> missions{{10.0, 1.0, 2.0, 0, 2}, {5.0, 0.0, 0.0, 2, 3}, {nan, nan, -1.0, 0, 0}, {1.0, 2.0, 3.0, 5, 1}};
  auto tables = [&](const std::vector<smx_mission>& ms, const std::vector<int32_t>& rr, RouteTables& rt) {
    return route_tables(ms.data(), (int32_t)ms.size(), rr.data(), (int32_t)rr.size(), 2, 3, m.lane_road, m.lane_out_off, m.lane_out_idx, rt);
  };
  RouteTables rt;
  expect(tables(missions, roads, rt) == nullptr && rt.any, "the four missions are accepted");
  expect(rt.pos.size() == 4 * 2 && rt.lane_ok.size() == 4 * 3 && rt.last.size() == 4 && rt.goal.size() == 4 * 3, "n_slots x n_roads, n_slots x n_lanes");
  expect(rt.pos == std::vector<int16_t>({0, 1, /**/ 0, 1, /**/ -1, -1, /**/ 0, -1}), "positions: a road named twice keeps its first position; an endless slot has none");
  expect(rt.last == std::vector<int32_t>({1, 0, -1, 0}), "last roads, -1 for the empty route");
  expect(rt.goal == std::vector<double>({10, 1, 2, 5, 0, 0, 0, 0, 0, 1, 2, 3}), "goals; an endless slot's is not read");
  const std::vector<std::vector<int32_t>> routes{{0, 1}, {0, 1, 0}, {}, {0}};
  for (size_t s = 0; s < routes.size(); ++s) {
    const std::vector<uint8_t> want = routes[s].empty() ? std::vector<uint8_t>(3, 0) : lane_ok_of(m, routes[s]);
    expect(std::vector<uint8_t>(rt.lane_ok.begin() + 3 * s, rt.lane_ok.begin() + 3 * s + 3) == want, "slot " + std::to_string(s) + ": route_lane_ok is the reference's filter, lane by lane");
  }
  expect(rt.lane_ok == std::vector<uint8_t>({1, 1, 1, /**/ 1, 1, 0, /**/ 0, 0, 0, /**/ 1, 1, 0}), "... spelled out");
  const std::vector<smx_mission> endless(4, smx_mission{0, 0, 0, 0, 0});
  expect(tables(endless, {}, rt) == nullptr && !rt.any && rt.last == std::vector<int32_t>(4, -1), "only endless missions: no table is needed");
  expect(route_tables(nullptr, 0, nullptr, 0, 2, 3, m.lane_road, m.lane_out_off, m.lane_out_idx, rt) == nullptr && !rt.any && rt.pos.empty(), "no slots: cleared");
  // refusals
  auto refused = [&](smx_mission ms, std::vector<int32_t> rr, const char* head, const std::string& what) {
    std::vector<smx_mission> four = endless;
    four[2] = ms;
    RouteTables r;
    const char* why = tables(four, rr, r);
    expect(why && starts_with(why, head), what + ": " + (why ? why : "accepted"));
  };
  const char* range = "smx_set_missions: route range outside route_roads";
  refused({1, 1, 1, 0, 3}, {0, 1}, range, "a route longer than route_roads");
  refused({1, 1, 1, 2, 1}, {0, 1}, range, "a route that starts at the end of route_roads");
  refused({1, 1, 1, -1, 1}, {0, 1}, range, "a negative offset");
  refused({1, 1, 1, 0, -1}, {0, 1}, range, "a negative length");
  refused({1, 1, 1, 2147483647, 2147483647}, {0, 1}, range, "offset + length past int32");
  refused({1, 1, 1, 0, 2}, {0, 2}, "smx_set_missions: road index out of range", "a road index equal to the road count");
  refused({1, 1, 1, 0, 2}, {-1, 1}, "smx_set_missions: road index out of range", "a negative road index");
  const char* goal = "smx_set_missions: a fixed route needs a PositionalGoal";
  refused({nan, 1, 1, 0, 1}, {0}, goal, "a NaN goal");
  refused({1, inf, 1, 0, 1}, {0}, goal, "an infinite goal");
  refused({1, 1, -1.0, 0, 1}, {0}, goal, "a negative radius");
  refused({1, 1, nan, 0, 1}, {0}, goal, "a NaN radius");
  // the goal kinds against the routes
  bool any = true, traverse = true;
  const std::vector<int32_t> last{1, 0, -1, 0};
  std::vector<smx_mission_goal> goals{{SMX_GOAL_LAP, 2, 60.0}, {SMX_GOAL_POSITIONAL, 0, 0.0}, {SMX_GOAL_TRAVERSE, 0, 0.0}, {SMX_GOAL_POSITIONAL, 0, 0.0}};
  expect(mission_goals_route_error(goals.data(), 4, last, any, traverse) == nullptr && any && traverse, "a lap on a routed slot, a traverse goal on an endless one");
  expect(mission_goals_error(goals.data(), 4, 4, nullptr, nullptr, 0, 3).find("needs the lane tables") != std::string::npos, "a traverse goal needs the lane tables");
  goals[2].kind = SMX_GOAL_POSITIONAL;
  expect(mission_goals_error(goals.data(), 4, 4, nullptr, nullptr, 0, 3).empty() && mission_goals_route_error(goals.data(), 4, last, any, traverse) == nullptr && any && !traverse, "without it: a lap alone");
  goals[2].kind = SMX_GOAL_LAP, goals[2].num_laps = 1;
  expect(starts_with(mission_goals_route_error(goals.data(), 4, last, any, traverse), "smx_set_mission_goals: a lap goal needs"), "a lap on an endless slot is refused");
  expect(starts_with(mission_goals_route_error(goals.data(), 4, {}, any, traverse), "smx_set_mission_goals: a lap goal needs"), "... and before any smx_set_missions");
  goals[2].kind = SMX_GOAL_POSITIONAL, goals[1].kind = SMX_GOAL_TRAVERSE;
  expect(starts_with(mission_goals_route_error(goals.data(), 4, last, any, traverse), "smx_set_mission_goals: a traverse goal has an empty route"), "a traverse goal on a routed slot is refused");
  goals[1].kind = SMX_GOAL_POSITIONAL, goals[0].kind = SMX_GOAL_POSITIONAL;
  expect(mission_goals_route_error(goals.data(), 4, last, any, traverse) == nullptr && !any && !traverse, "positional goals alone: nothing to keep");
}

int main() {
  const int on = case_table();
  case_entry_check();
  case_geometry();
  const int refused = case_config_extremes();
  case_map_tables();
  case_routes();
  if (failures) return 1;
  std::printf("{\"checks\": %d, \"configs\": %d, \"stack_sources_on\": %d, \"extremes_refused\": %d}\n", checks, (int)CONFIGS, on, refused);
  return 0;
}

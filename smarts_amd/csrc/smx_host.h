// smx_host.h — the device-free half of the C-ABI (include/smx.h): everything that stands between a caller's pointers
// and kernels that follow indices without bounds tests, and needs no device to decide — the configuration checks, the
// table of caller buffers behind the entry check and the frame stacks, the frame-stack launch geometry, the range checks
// and the field list of the map tables, the route tables of smx_set_missions.  No HIP call, no __device__, no kernel
// type: smx_kernels.hip includes it and keeps the handle, the allocations, the copies and the launches; plain g++
// compiles it too (tests/native/host_abi.cpp drives it under AddressSanitizer + UBSan).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smx.h"
#include "smx_guard.h"

// Constants of the device side that a host decision depends on.  Their owners define the macros (smx_plan.h,
// smx_roadmap.h, the kernels); smx_kernels.hip asserts that the two agree.
constexpr int SMX_HOST_BLOCK = 64;         // SMX_BLOCK
constexpr int SMX_HOST_WP_LANES = 4;       // SMX_WP_LANES
constexpr int SMX_HOST_MAX_KNOTS = 36;     // SMX_MAX_KNOTS
constexpr int SMX_HOST_SLOW_BLOCKS = 512;  // SMX_SLOW_BLOCKS
constexpr int SMX_HOST_STACK_BLOCK = 256;  // SMX_STACK_BLOCK

#define SMX_STR_(x) #x
#define SMX_STR(x) SMX_STR_(x)

// ---- the smx_check_* entry points' way out: the code, and the message cut to the caller's err[err_len] ----
inline int report(int rc, const std::string& msg, char* err, uint64_t err_len) {
  if (err && err_len > 0) {
    const size_t n = std::min<size_t>(msg.size(), (size_t)err_len - 1);
    memcpy(err, msg.data(), n);
    err[n] = 0;
  }
  return rc;
}
// a refusal: the reason into `err`, the code back
inline int refuse(std::string& err, std::string why, int rc = SMX_ERR_INVALID) {
  err = std::move(why);
  return rc;
}

// ---- The configuration (smx_create; the smx_check_* functions ask the three single-feature ones again) ----
// SMX_SENSOR_LANE_TTC reads the waypoint and neighbour rows
inline const char* lane_ttc_config_error(const smx_config& c) {
  if (!(c.sensors & SMX_SENSOR_LANE_TTC)) return nullptr;
  if (!(c.sensors & SMX_SENSOR_WAYPOINTS) || !(c.sensors & SMX_SENSOR_NEIGHBORS))
    return "lane_ttc: SMX_SENSOR_LANE_TTC needs SMX_SENSOR_WAYPOINTS and SMX_SENSOR_NEIGHBORS (it is a function of their rows)";
  if ((int64_t)c.wp_paths * c.wp_len > SMX_TTC_MAX_WAYPOINTS)
    return "lane_ttc: need wp_paths * wp_len <= " SMX_STR(SMX_TTC_MAX_WAYPOINTS) " (an agent's waypoints are staged in LDS)";
  return nullptr;
}

// a sensor grid of the OGM's kind: cells a multiple of 16 and at most 65536 (products in int64_t: defined for every int32)
inline bool grid_ok(int32_t width, int32_t height, double resolution) {
  const int64_t cells = (int64_t)width * height;
  return width >= 1 && height >= 1 && cells % 16 == 0 && cells <= 64 * 1024 && resolution > 0.0;
}

// SMX_SENSOR_RGB's grid: the DAGM's limits
inline const char* rgb_config_error(const smx_config& c) {
  if (!(c.sensors & SMX_SENSOR_RGB) || grid_ok(c.rgb_width, c.rgb_height, c.rgb_resolution)) return nullptr;
  return "rgb: need width*height a multiple of 16 and at most 65536 (the class tile of an image is staged in LDS), resolution > 0";
}

// smx_config.frame_stack: off, or FrameStack's num_stack (frame_stack.py:47 asserts num_stack > 1)
inline const char* frame_stack_config_error(const smx_config& c) {
  if (c.frame_stack == 0 || (c.frame_stack >= 2 && c.frame_stack <= SMX_STACK_MAX_FRAMES)) return nullptr;
  return "frame_stack: need 0 (off) or 2 <= frame_stack <= " SMX_STR(SMX_STACK_MAX_FRAMES) " (the reference asserts num_stack > 1)";
}

// Why smx_create refuses the configuration (null: it does not).
inline const char* config_error(const smx_config& c) {
  if (c.num_envs <= 0 || c.num_vehicles <= 0 || c.num_vehicles > SMX_HOST_BLOCK) return "num_envs must be > 0 and 0 < num_vehicles <= 64";
  if (!(c.dt > 0.0)) return "dt must be > 0";
  if ((c.sensors & SMX_SENSOR_ROAD_WAYPOINTS) &&
      (c.rw_horizon < 1 || c.rw_horizon > SMX_RW_HORIZON_MAX || c.rw_lanes < 1 || c.rw_lanes > SMX_RW_LANE_CAP || c.rw_paths < 1 ||
       c.rw_paths > 64))
    return "road waypoints: need 1 <= rw_horizon <= 64, 1 <= rw_lanes <= 8, 1 <= rw_paths <= 64";
  if ((c.sensors & SMX_SENSOR_WAYPOINTS) &&
      (c.wp_lookahead < 1 || c.wp_lookahead > SMX_HOST_MAX_KNOTS - 2 || c.wp_paths < 1 || c.wp_paths > 64 || c.wp_len < 1 ||
       c.wp_len > c.wp_lookahead + 1))
    return "waypoints: need lookahead >= 1, 1 <= wp_paths <= 64, 1 <= wp_len <= lookahead + 1";
  if (c.via_max < 0 || c.via_max > 32) return "via_max must be in 0..32";
  if (c.alive_lists < 0 || c.alive_lists > SMX_MAX_ALIVE_LISTS || c.alive_min_ego < 0 || c.alive_min_total < 0)
    return "agents_alive: at most 4 lists, non-negative minima";
  if (c.num_social < 0 || c.num_social >= c.num_vehicles) return "num_social must leave at least one agent slot";
  if (c.num_social > 0 && !(c.social_speed_factor >= 0.0)) return "social_speed_factor must be >= 0";
  if (c.social_model != SMX_SOCIAL_CONSTANT && c.social_model != SMX_SOCIAL_IDM) return "unknown social_model";
  if (c.action_space < SMX_ACTION_SPACE_LANE || c.action_space > SMX_ACTION_SPACE_IMITATION) return "unknown action_space";
  if ((c.sensors & SMX_SENSOR_OGM) && !grid_ok(c.ogm_width, c.ogm_height, c.ogm_resolution))
    return "ogm: need width*height a multiple of 16 and at most 65536, resolution > 0";
  if ((c.sensors & SMX_SENSOR_DAGM) && !grid_ok(c.dagm_width, c.dagm_height, c.dagm_resolution))
    return "dagm: need width*height a multiple of 16 and at most 65536, resolution > 0";
  if ((c.sensors & SMX_SENSOR_LIDAR) && (c.lidar_rays < 1 || c.lidar_rays > 65536)) return "lidar: need 1 <= lidar_rays <= 65536";
  if ((c.sensors & SMX_SENSOR_NEIGHBORS) && (c.nb_max < 1 || c.nb_max > 127)) return "neighbours: need 1 <= nb_max <= 127";
  if (const char* why = lane_ttc_config_error(c)) return why;
  if (const char* why = rgb_config_error(c)) return why;
  return frame_stack_config_error(c);
}

// =================================================================================
// The caller's buffers: one row per pointer of smx_state, smx_spawns and smx_outputs.  The entry check of every
// smx_reset / smx_step* (smx_check_buffers) and the frame stacks (smx_check_frame_stack, k_frame_push's row size) both
// read it; a new output row is one entry here.
// =================================================================================
// Both structs open with their pointers in the order of their index enums, then the counts: pointer i by its index.
static_assert(offsetof(smx_outputs, count) == SMX_OUT_BUFFERS * sizeof(void*), "smx_outputs opens with SMX_OUT_BUFFERS pointers");
static_assert(offsetof(smx_outputs, ec_rw_heading) == (SMX_OUT_BUFFERS - 1) * sizeof(void*), "... the last of them ec_rw_heading");
static_assert(offsetof(smx_state, count) == SMX_ST_BUFFERS * sizeof(void*), "smx_state opens with SMX_ST_BUFFERS pointers");
static_assert(offsetof(smx_state, env_reset_pending) == (SMX_ST_BUFFERS - 1) * sizeof(void*), "... the last of them env_reset_pending");
template <class Struct>  // smx_outputs by SMX_OUT_*, smx_state by SMX_ST_*
inline const void* buffer_ptr(const Struct& s, int index) {
  const void* p;
  memcpy(&p, reinterpret_cast<const char*>(&s) + (size_t)index * sizeof(void*), sizeof(p));
  return p;
}

enum BufUnit : uint8_t { BUF_PER_AGENT, BUF_PER_ENV, BUF_LEARNER, BUF_PER_SPAWN };  // [E*N]... | [E] | [2][E*N] | [episodes][E*N]...
// when a NULL pointer is an error: never | always | every bit of `sensors` is set | via_max > 0 and vias were given
// (smx_set_vias) | SMX_DONE_NOT_MOVING is a done criterion | num_social > 0
enum BufNull : uint8_t { NULL_NEVER, NULL_ALWAYS, NULL_WITH_SENSOR, NULL_WITH_VIAS, NULL_WITH_NOT_MOVING, NULL_WITH_SOCIAL };
struct BufRow {
  int index;         // SMX_OUT_* / SMX_ST_* (the spawn tables: 0 pose, 1 social)
  const char* name;  // as the messages print it
  uint8_t dtype;     // SMX_DT_* the ABI writes
  BufUnit unit;
  uint64_t (*per_unit)(const smx_config&);  // elements per unit.  From the shape numbers whether or not the sensor is on
                                            // (a buffer that is given is checked), except the road-waypoint rows: 0 when off
  uint32_t sensors;  // SMX_SENSOR_* bits the row belongs to (0: none)
  BufNull null_error;
  bool stackable;    // smx_bind_frame_stack takes it as a source
};

namespace buf {  // elements per unit
using C = const smx_config&;
template <uint64_t K> constexpr uint64_t fixed(C) { return K; }
constexpr uint64_t wp(C c) { return (uint64_t)c.wp_paths * c.wp_len; }
constexpr uint64_t wp3(C c) { return wp(c) * 3; }
constexpr uint64_t wp_count(C c) { return (uint64_t)((int64_t)c.wp_paths + 1); }
constexpr uint64_t nb(C c) { return (uint64_t)c.nb_max; }
constexpr uint64_t nb3(C c) { return nb(c) * 3; }
constexpr uint64_t rays(C c) { return (uint64_t)c.lidar_rays; }
constexpr uint64_t rays3(C c) { return rays(c) * 3; }
constexpr uint64_t ogm(C c) { return (uint64_t)c.ogm_width * c.ogm_height; }
constexpr uint64_t dagm(C c) { return (uint64_t)c.dagm_width * c.dagm_height; }
constexpr uint64_t vias(C c) { return (uint64_t)(c.via_max > 0 ? c.via_max : 0); }
constexpr bool rw_on(C c) { return (c.sensors & SMX_SENSOR_ROAD_WAYPOINTS) != 0; }
constexpr uint64_t rw_lanes(C c) { return rw_on(c) ? (uint64_t)c.rw_lanes : 0; }
constexpr uint64_t rw_paths(C c) { return rw_on(c) ? rw_lanes(c) * (uint64_t)c.rw_paths : 0; }
constexpr uint64_t rw(C c) { return rw_on(c) ? rw_paths(c) * (2 * (uint64_t)c.rw_horizon + 1) : 0; }
constexpr uint64_t rw3(C c) { return rw(c) * 3; }
}  // namespace buf

constexpr BufRow STATE_ROWS[SMX_ST_BUFFERS] = {
    {SMX_ST_F64, "state.f64", SMX_DT_F64, BUF_PER_AGENT, buf::fixed<SMX_S_COUNT>, 0, NULL_ALWAYS, false},
    {SMX_ST_FLAGS, "state.flags", SMX_DT_I32, BUF_PER_AGENT, buf::fixed<1>, 0, NULL_ALWAYS, false},
    {SMX_ST_STEPS, "state.steps", SMX_DT_I32, BUF_PER_AGENT, buf::fixed<1>, 0, NULL_ALWAYS, false},
    {SMX_ST_ENV_TICKS, "state.env_ticks", SMX_DT_I32, BUF_PER_ENV, buf::fixed<1>, 0, NULL_ALWAYS, false},
    {SMX_ST_ENV_DONE_COUNT, "state.env_done_count", SMX_DT_I32, BUF_PER_ENV, buf::fixed<1>, 0, NULL_ALWAYS, false},
    {SMX_ST_ENV_EPISODE, "state.env_episode", SMX_DT_I32, BUF_PER_ENV, buf::fixed<1>, 0, NULL_ALWAYS, false},
    {SMX_ST_DRIVEN_PATH, "state.driven_path", SMX_DT_F64, BUF_PER_AGENT, buf::fixed<SMX_DRIVEN_PATH_LEN>, 0, NULL_WITH_NOT_MOVING, false},
    {SMX_ST_SEED_CACHE, "state.seed_cache", SMX_DT_I32, BUF_PER_AGENT, buf::fixed<SMX_SEED_COUNT>, 0, NULL_ALWAYS, false},
    {SMX_ST_FACTS_I32, "state.facts_i32", SMX_DT_I32, BUF_PER_AGENT, buf::fixed<SMX_FACT_I_COUNT>, 0, NULL_ALWAYS, false},
    {SMX_ST_FACTS_F64, "state.facts_f64", SMX_DT_F64, BUF_PER_AGENT, buf::fixed<SMX_FACT_F_COUNT>, 0, NULL_ALWAYS, false},
    {SMX_ST_ENV_RESET_PENDING, "state.env_reset_pending", SMX_DT_I32, BUF_PER_ENV, buf::fixed<1>, 0, NULL_ALWAYS, false},
};
constexpr BufRow SPAWN_ROWS[2] = {
    {0, "spawns.pose", SMX_DT_F64, BUF_PER_SPAWN, buf::fixed<4>, 0, NULL_ALWAYS, false},
    {1, "spawns.social", SMX_DT_F64, BUF_PER_SPAWN, buf::fixed<2>, 0, NULL_WITH_SOCIAL, false},
};

#define SMX_OUT_ROW(field, INDEX, dtype, unit, per_unit, sensors, null_error, stackable) \
  {SMX_OUT_##INDEX, "out." #field, SMX_DT_##dtype, unit, per_unit, sensors, null_error, stackable}
#define AGENT_ROW(field, INDEX, dtype, per_unit) SMX_OUT_ROW(field, INDEX, dtype, BUF_PER_AGENT, per_unit, 0, NULL_ALWAYS, true)
#define SENSOR_ROW(field, INDEX, dtype, per_unit, sensors) SMX_OUT_ROW(field, INDEX, dtype, BUF_PER_AGENT, per_unit, sensors, NULL_WITH_SENSOR, true)
#define VIA_ROW(field, INDEX, dtype, per_unit) SMX_OUT_ROW(field, INDEX, dtype, BUF_PER_AGENT, per_unit, 0, NULL_WITH_VIAS, true)
// (not stacked: env_done is per env, learner is [2][E*N], the final_* rows are written for restarting envs only)
#define FINAL_ROW(field, INDEX, dtype, per_unit) SMX_OUT_ROW(field, INDEX, dtype, BUF_PER_AGENT, per_unit, 0, NULL_NEVER, false)
constexpr BufRow OUT_ROWS[SMX_OUT_BUFFERS] = {
    AGENT_ROW(ego_pos, EGO_POS, F64, buf::fixed<3>),
    AGENT_ROW(ego_f32, EGO_F32, F32, buf::fixed<SMX_EGO_F32_COUNT>),
    AGENT_ROW(ego_lane, EGO_LANE, I16, buf::fixed<2>),
    AGENT_ROW(events, EVENTS, U8, buf::fixed<SMX_EV_COUNT>),
    AGENT_ROW(reward, REWARD, F64, buf::fixed<1>),
    AGENT_ROW(dist, DIST, F64, buf::fixed<1>),
    AGENT_ROW(done, DONE, U8, buf::fixed<1>),
    AGENT_ROW(active, ACTIVE, U8, buf::fixed<1>),
    SMX_OUT_ROW(env_done, ENV_DONE, U8, BUF_PER_ENV, buf::fixed<1>, 0, NULL_ALWAYS, false),
    VIA_ROW(via_near, VIA_NEAR, I8, buf::vias),
    VIA_ROW(via_near_count, VIA_NEAR_COUNT, U8, buf::fixed<1>),
    VIA_ROW(via_hit, VIA_HIT, I32, buf::fixed<1>),
    SMX_OUT_ROW(learner, LEARNER, F32, BUF_LEARNER, buf::fixed<1>, 0, NULL_NEVER, false),
    SENSOR_ROW(wp_pos, WP_POS, F64, buf::wp3, SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(wp_heading, WP_HEADING, F32, buf::wp, SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(wp_lane_width, WP_LANE_WIDTH, F32, buf::wp, SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(wp_speed_limit, WP_SPEED_LIMIT, F32, buf::wp, SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(wp_lane_index, WP_LANE_INDEX, I8, buf::wp, SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(wp_lane_id, WP_LANE_ID, I16, buf::wp, SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(wp_count, WP_COUNT, U8, buf::wp_count, SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(nb_pos, NB_POS, F64, buf::nb3, SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(nb_box, NB_BOX, F32, buf::nb3, SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(nb_heading, NB_HEADING, F32, buf::nb, SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(nb_speed, NB_SPEED, F32, buf::nb, SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(nb_lane_index, NB_LANE_INDEX, I8, buf::nb, SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(nb_lane_id, NB_LANE_ID, I16, buf::nb, SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(nb_slot, NB_SLOT, I8, buf::nb, SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(nb_count, NB_COUNT, U8, buf::fixed<1>, SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(ogm, OGM, U8, buf::ogm, SMX_SENSOR_OGM),
    SENSOR_ROW(lidar_hit, LIDAR_HIT, U8, buf::rays, SMX_SENSOR_LIDAR),
    SENSOR_ROW(lidar_point, LIDAR_POINT, F64, buf::rays3, SMX_SENSOR_LIDAR),
    SENSOR_ROW(dagm, DAGM, U8, buf::dagm, SMX_SENSOR_DAGM),
    SMX_OUT_ROW(collidees, COLLIDEES, U64, BUF_PER_AGENT, buf::fixed<1>, 0, NULL_NEVER, true),
    SENSOR_ROW(rw_lane_count, RW_LANE_COUNT, U8, buf::fixed<1>, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_lane, RW_LANE, I16, buf::rw_lanes, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_path_count, RW_PATH_COUNT, I16, buf::rw_lanes, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_count, RW_COUNT, U8, buf::rw_paths, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_pos, RW_POS, F64, buf::rw3, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_heading, RW_HEADING, F32, buf::rw, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_lane_width, RW_LANE_WIDTH, F32, buf::rw, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_speed_limit, RW_SPEED_LIMIT, F32, buf::rw, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_lane_index, RW_LANE_INDEX, I8, buf::rw, SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(rw_lane_id, RW_LANE_ID, I16, buf::rw, SMX_SENSOR_ROAD_WAYPOINTS),
    FINAL_ROW(final_ego_pos, FINAL_EGO_POS, F64, buf::fixed<3>),
    FINAL_ROW(final_ego_f32, FINAL_EGO_F32, F32, buf::fixed<SMX_EGO_F32_COUNT>),
    FINAL_ROW(final_ego_lane, FINAL_EGO_LANE, I16, buf::fixed<2>),
    FINAL_ROW(final_events, FINAL_EVENTS, U8, buf::fixed<SMX_EV_COUNT>),
    FINAL_ROW(final_dist, FINAL_DIST, F64, buf::fixed<1>),
    SENSOR_ROW(lane_ttc, LANE_TTC, F64, buf::fixed<SMX_TTC_COUNT>, SMX_SENSOR_LANE_TTC),
    SENSOR_ROW(lane_ttc_flags, LANE_TTC_FLAGS, U8, buf::fixed<1>, SMX_SENSOR_LANE_TTC),
    SENSOR_ROW(ego_frame, EGO_FRAME, F64, buf::fixed<4>, SMX_SENSOR_EGO_CENTRIC),
    SENSOR_ROW(ec_flags, EC_FLAGS, U8, buf::fixed<1>, SMX_SENSOR_EGO_CENTRIC),
    SENSOR_ROW(ec_ego_f32, EC_EGO_F32, F32, buf::fixed<SMX_EGO_F32_COUNT>, SMX_SENSOR_EGO_CENTRIC),
    SENSOR_ROW(ec_wp_pos, EC_WP_POS, F64, buf::wp3, SMX_SENSOR_EGO_CENTRIC | SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(ec_wp_heading, EC_WP_HEADING, F32, buf::wp, SMX_SENSOR_EGO_CENTRIC | SMX_SENSOR_WAYPOINTS),
    SENSOR_ROW(ec_nb_pos, EC_NB_POS, F64, buf::nb3, SMX_SENSOR_EGO_CENTRIC | SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(ec_nb_heading, EC_NB_HEADING, F32, buf::nb, SMX_SENSOR_EGO_CENTRIC | SMX_SENSOR_NEIGHBORS),
    SENSOR_ROW(ec_lidar_point, EC_LIDAR_POINT, F64, buf::rays3, SMX_SENSOR_EGO_CENTRIC | SMX_SENSOR_LIDAR),
    SENSOR_ROW(ec_rw_pos, EC_RW_POS, F64, buf::rw3, SMX_SENSOR_EGO_CENTRIC | SMX_SENSOR_ROAD_WAYPOINTS),
    SENSOR_ROW(ec_rw_heading, EC_RW_HEADING, F32, buf::rw, SMX_SENSOR_EGO_CENTRIC | SMX_SENSOR_ROAD_WAYPOINTS),
};
#undef SMX_OUT_ROW
#undef AGENT_ROW
#undef SENSOR_ROW
#undef VIA_ROW
#undef FINAL_ROW

template <size_t N>
constexpr bool rows_in_index_order(const BufRow (&rows)[N]) {
  for (size_t i = 0; i < N; ++i)
    if (rows[i].index != (int)i) return false;
  return true;
}
static_assert(rows_in_index_order(STATE_ROWS) && rows_in_index_order(SPAWN_ROWS) && rows_in_index_order(OUT_ROWS),
              "a row per index, in the order of the enum (and of the struct's pointers)");

inline const char* dtype_name(int d) {
  static const char* n[] = {"none", "f64", "f32", "i32", "i16", "i8", "u8", "u64"};
  return (d >= 0 && d <= SMX_DT_U64) ? n[d] : "?";
}
inline uint64_t dtype_size(int d) {
  static const uint8_t bytes[] = {0, 8, 4, 4, 2, 1, 1, 8};
  return (d >= 0 && d <= SMX_DT_U64) ? bytes[d] : 0;
}

// every bit of the row's sensors is set (a row without sensor bits: always)
inline bool row_sensor_on(const BufRow& r, const smx_config& c) { return (c.sensors & r.sensors) == r.sensors; }

// elements a non-NULL buffer must hold
inline uint64_t row_elements(const BufRow& r, const smx_config& c, int32_t episodes) {
  const uint64_t E = (uint64_t)c.num_envs, T = E * (uint64_t)c.num_vehicles;
  const uint64_t units = r.unit == BUF_PER_ENV ? E : r.unit == BUF_LEARNER ? 2 * T : r.unit == BUF_PER_SPAWN ? (uint64_t)(episodes > 0 ? episodes : 0) * T : T;
  return units * r.per_unit(c);
}

inline bool row_null_is_error(const BufRow& r, const smx_config& c, bool has_vias) {
  switch (r.null_error) {
    case NULL_ALWAYS: return true;
    case NULL_WITH_SENSOR: return row_sensor_on(r, c);
    case NULL_WITH_VIAS: return c.via_max > 0 && has_vias;
    case NULL_WITH_NOT_MOVING: return (c.done_criteria & SMX_DONE_NOT_MOVING) != 0;
    case NULL_WITH_SOCIAL: return c.num_social > 0;
    default: return false;
  }
}

// one buffer against its row
inline int check_row(const BufRow& r, const smx_config& c, bool has_vias, int32_t episodes, const void* ptr, uint64_t have, uint8_t dtype,
                     std::string& err) {
  const auto name = [&] { return std::string(r.name); };  // (no string is built unless the buffer is refused)
  if (!ptr) return row_null_is_error(r, c, has_vias) ? refuse(err, name() + " is NULL but the configuration needs it") : SMX_OK;
  if (dtype != r.dtype) return refuse(err, name() + ": declared dtype " + dtype_name(dtype) + ", the ABI says " + dtype_name(r.dtype));
  const uint64_t need = row_elements(r, c, episodes);
  if (have < need)
    return refuse(err, name() + ": " + std::to_string(have) + " elements declared, the configuration needs " + std::to_string(need) +
                           " (a short buffer would be an out-of-bounds device write)");
  return SMX_OK;
}

// The entry check of every smx_reset / smx_step* (and smx_check_buffers, which needs no device).
inline int check_buffers_impl(const smx_config& c, bool has_vias, const smx_state* st, const smx_spawns* sp, const smx_outputs* o,
                              std::string& err) {
  if (!st || !sp || !o) return refuse(err, "null state / spawns / outputs");
  if (const char* why = lane_ttc_config_error(c)) return refuse(err, why);
  if (sp->episodes < 1) return refuse(err, "spawn table is empty (episodes < 1)");
  for (const BufRow& r : STATE_ROWS)
    if (const int rc = check_row(r, c, has_vias, 0, buffer_ptr(*st, r.index), st->count[r.index], st->dtype[r.index], err)) return rc;
  if (const int rc = check_row(SPAWN_ROWS[0], c, has_vias, sp->episodes, sp->pose, sp->pose_count, SMX_DT_F64, err)) return rc;
  if (const int rc = check_row(SPAWN_ROWS[1], c, has_vias, sp->episodes, sp->social, sp->social_count, SMX_DT_F64, err)) return rc;
  for (const BufRow& r : OUT_ROWS)
    if (const int rc = check_row(r, c, has_vias, 0, buffer_ptr(*o, r.index), o->count[r.index], o->dtype[r.index], err)) return rc;
  const int finals = (o->final_ego_pos != nullptr) + (o->final_ego_f32 != nullptr) + (o->final_ego_lane != nullptr) +
                     (o->final_events != nullptr) + (o->final_dist != nullptr);
  if (finals != 0 && finals != 5) return refuse(err, "out.final_*: give all five buffers or none");
  return SMX_OK;
}

inline int check_rgb_output_impl(const smx_config& c, uint64_t count, std::string& err) {
  if (const char* why = rgb_config_error(c)) return refuse(err, why);
  if (!(c.sensors & SMX_SENSOR_RGB)) return SMX_OK;
  if (c.num_envs <= 0 || c.num_vehicles <= 0) return refuse(err, "rgb: num_envs and num_vehicles must be > 0");
  const uint64_t need = (uint64_t)c.num_envs * (uint64_t)c.num_vehicles * (uint64_t)c.rgb_width * (uint64_t)c.rgb_height * 3;
  if (count < need)
    return refuse(err, "rgb output: " + std::to_string(count) + " bytes declared, the configuration needs " + std::to_string(need) +
                           " (a short buffer would be an out-of-bounds device write)");
  return SMX_OK;
}

// ---- the state guard (smx_set_guard / smx_check_guard) ----
inline int check_guard_impl(const smx_config& c, uint64_t count, double margin, std::string& err) {
  if (c.num_envs <= 0 || c.num_vehicles <= 0) return refuse(err, "state guard: num_envs and num_vehicles must be > 0");
  if (!guard_margin_ok(margin))
    return refuse(err, "state guard: the margin must be finite and 0 <= margin <= " + std::to_string((long long)SMX_GUARD_MARGIN_MAX) + " m");
  const uint64_t need = (uint64_t)c.num_envs * (uint64_t)c.num_vehicles;
  if (count < need)
    return refuse(err, "state guard: " + std::to_string(count) + " bytes declared, the configuration needs " + std::to_string(need) +
                           " (a short buffer would be an out-of-bounds device write)");
  return SMX_OK;
}

// ---- Traffic-history replay (smx_set_social_history / smx_check_social_history) ----
// The kernels copy a present slot's row into the state without a test, and the map searches then form cell indices from
// it: every row of a non-empty slot is checked here, once, against the union of the map's two grids (the state guard's
// box with margin 0; the guard itself does not cover social slots).  Rows of empty slots are never read by a kernel and
// may hold anything.  `map`: only its grid extents are read.
inline int check_social_history_impl(const smx_config& c, const smx_map_tables& map, const smx_social_history& hs, std::string& err) {
  if (c.num_envs <= 0 || c.num_vehicles <= 0) return refuse(err, "social history: num_envs and num_vehicles must be > 0");
  if (c.num_social <= 0) return refuse(err, "social history: the configuration has no social slots (num_social is 0)");
  if (hs.num_social != c.num_social)
    return refuse(err, "social history: the table has " + std::to_string(hs.num_social) + " slots, the configuration's num_social is " +
                           std::to_string(c.num_social));
  if (c.social_model == SMX_SOCIAL_IDM)
    return refuse(err, "social history: social_model is SMX_SOCIAL_IDM (the replay replaces the speed model; use SMX_SOCIAL_CONSTANT)");
  if (hs.n_frames < 1) return refuse(err, "social history: n_frames must be >= 1");
  if (hs.rows < 1) return refuse(err, "social history: rows must be >= 1");
  const uint64_t cells = (uint64_t)hs.n_frames * (uint64_t)hs.num_social;
  if (cells > 0x7fffffffull) return refuse(err, "social history: n_frames * num_social must stay below 2^31");
  if (!hs.frames_host || !hs.vehicle_host) return refuse(err, "social history: null table (frames_host / vehicle_host)");
  if (!hs.start_frame_dev) return refuse(err, "social history: start_frame_dev is NULL");
  const uint64_t need = (uint64_t)hs.rows * (uint64_t)c.num_envs;
  if (hs.start_count < need)
    return refuse(err, "social history: start_frame " + std::to_string(hs.start_count) + " elements declared, rows * num_envs is " +
                           std::to_string(need) + " (a short table would be an out-of-bounds device read)");
  if (hs.replaced_dev && hs.replaced_count < need)
    return refuse(err, "social history: replaced " + std::to_string(hs.replaced_count) + " elements declared, rows * num_envs is " +
                           std::to_string(need) + " (a short table would be an out-of-bounds device read)");
  const GuardBox box = guard_box_of(map, 0.0);
  for (uint64_t i = 0; i < cells; ++i) {
    if (hs.vehicle_host[i] < 0) continue;
    const double* r = hs.frames_host + i * 4;
    if (!guard_in_bounds_kin(box, r[0], r[1], r[2], r[3]))
      return refuse(err, "social history: frame " + std::to_string(i / (uint64_t)hs.num_social) + ", slot " +
                             std::to_string(i % (uint64_t)hs.num_social) + " (vehicle " + std::to_string(hs.vehicle_host[i]) +
                             ") is not finite or lies outside the map's grids");
  }
  return SMX_OK;
}

// ---- ... at each vehicle's own dimensions (smx_set_social_history_dims / smx_check_social_history_dims) ----
// The caps bound every reach and pixel rectangle the kernels form from a triple (the largest default, the trailer, is
// 10 x 2.5 x 4); the id check makes every lookup through a cell of the bound table an index inside dims_host.
#define SMX_DIMS_MAX_PLANAR 25.0
#define SMX_DIMS_MAX_HEIGHT 10.0
// the largest vehicle id of a history's table, -1 when every cell is empty
inline int32_t social_history_max_id(const smx_social_history& hs) {
  int32_t max_id = -1;
  const uint64_t cells = (uint64_t)hs.n_frames * (uint64_t)hs.num_social;
  for (uint64_t i = 0; i < cells; ++i) max_id = hs.vehicle_host[i] > max_id ? hs.vehicle_host[i] : max_id;
  return max_id;
}
// `max_id`: of the history the dimensions are bound to
inline int check_social_dims_impl(const smx_social_dims& d, int32_t max_id, std::string& err) {
  if (d.n_ids < 1) return refuse(err, "history dimensions: n_ids must be >= 1");
  if (!d.dims_host) return refuse(err, "history dimensions: null table (dims_host)");
  if (max_id >= d.n_ids)
    return refuse(err, "history dimensions: the bound history holds vehicle id " + std::to_string(max_id) + ", the table has n_ids = " +
                           std::to_string(d.n_ids) + " rows (a short table would be an out-of-bounds device read)");
  for (int32_t id = 0; id < d.n_ids; ++id) {
    const double* r = d.dims_host + (size_t)id * 3;
    for (int q = 0; q < 3; ++q) {
      const double cap = q < 2 ? SMX_DIMS_MAX_PLANAR : SMX_DIMS_MAX_HEIGHT;
      if (!(std::isfinite(r[q]) && r[q] > 0.0 && r[q] <= cap))
        return refuse(err, "history dimensions: vehicle " + std::to_string(id) + (q == 0 ? ", length " : (q == 1 ? ", width " : ", height ")) +
                               std::to_string(r[q]) + " must be finite, > 0 and <= " + std::to_string((int)cap) + " m");
    }
  }
  return SMX_OK;
}
inline int check_social_history_dims_impl(const smx_config& c, const smx_social_history& hs, const smx_social_dims& d, std::string& err) {
  if (hs.num_social != c.num_social || hs.num_social <= 0)
    return refuse(err, "history dimensions: the history has " + std::to_string(hs.num_social) + " slots, the configuration's num_social is " +
                           std::to_string(c.num_social));
  if (hs.n_frames < 1 || !hs.vehicle_host) return refuse(err, "history dimensions: the history has no table (n_frames / vehicle_host)");
  return check_social_dims_impl(d, social_history_max_id(hs), err);
}

// ---- Per-agent dimensions (smx_set_agent_dims / smx_check_agent_dims) ----
// The kinematic spaces only; every triple whole: three values within the caps (include/smx.h has the derivation), or
// three NaNs for the sedan's box.  The length's cap is the radius at which every vehicle's road-facts search runs
// (SMX_POSE_SCAN_RADIUS, smx_tick.h, which asserts the two equal): an observer asks for its neighbours' lanes within its
// own length (sensors.py:245) and is answered from the NEIGHBOUR's search, which finds no lane at that radius or beyond.
#define SMX_AGENT_DIMS_MAX_LENGTH 10.0
inline int check_agent_dims_impl(const smx_config& c, const smx_agent_dims& d, std::string& err) {
  if (c.action_space != SMX_ACTION_SPACE_TARGET_POSE && c.action_space != SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME &&
      c.action_space != SMX_ACTION_SPACE_IMITATION)
    return refuse(err, "agent dimensions: only the kinematic action spaces (TargetPose, TrajectoryWithTime, Imitation) take them; "
                       "a dynamic chassis is the sedan its model constants belong to");
  if (c.num_envs <= 0 || c.num_vehicles <= 0 || c.num_social < 0 || c.num_social >= c.num_vehicles)
    return refuse(err, "agent dimensions: the configuration has no agents");
  if (!d.dims_host) return refuse(err, "agent dimensions: null table (dims_host)");
  if (d.rows < 1) return refuse(err, "agent dimensions: rows must be >= 1");
  const uint64_t triples = (uint64_t)d.rows * (uint64_t)c.num_envs * (uint64_t)(c.num_vehicles - c.num_social);
  for (uint64_t i = 0; i < triples; ++i) {
    const double* r = d.dims_host + i * 3;
    const int nans = (r[0] != r[0]) + (r[1] != r[1]) + (r[2] != r[2]);
    if (nans == 3) continue;
    if (nans != 0)
      return refuse(err, "agent dimensions: triple " + std::to_string(i) + " is partly NaN (three NaNs = the sedan's box, or three values)");
    for (int q = 0; q < 3; ++q) {
      const double cap = q == 0 ? SMX_AGENT_DIMS_MAX_LENGTH : (q == 1 ? SMX_DIMS_MAX_PLANAR : SMX_DIMS_MAX_HEIGHT);
      if (!(std::isfinite(r[q]) && r[q] > 0.0 && r[q] <= cap))
        return refuse(err, "agent dimensions: triple " + std::to_string(i) + (q == 0 ? ", length " : (q == 1 ? ", width " : ", height ")) +
                               std::to_string(r[q]) + " must be finite, > 0 and <= " + std::to_string((int)cap) + " m" +
                               (q == 0 ? " (the radius of the neighbours' lane search, which answers the lookup within the observer's length)" : ""));
    }
  }
  return SMX_OK;
}

// ---- Delayed agent entry (smx_set_agent_entry / smx_check_agent_entry) ----
// k_entry reads the two tables at (episode mod rows, env, agent) and writes the two rows by vehicle: their shapes are
// checked here, and so is what the rule needs — a reset observation holds an agent (smarts.py:426-434 steps until one
// exists), and the overlap radius is a positive length.
inline int check_agent_entry_impl(const smx_config& c, const smx_agent_entry& d, std::string& err) {
  if (c.num_envs <= 0 || c.num_vehicles <= 0 || c.num_social < 0 || c.num_social >= c.num_vehicles)
    return refuse(err, "agent entry: the configuration has no agents");
  if (!d.ready_host || !d.check_host) return refuse(err, "agent entry: null table (ready_host / check_host)");
  if (d.rows < 1) return refuse(err, "agent entry: rows must be >= 1");
  const uint64_t agents = (uint64_t)(c.num_vehicles - c.num_social), total = (uint64_t)c.num_envs * (uint64_t)c.num_vehicles;
  if (!d.status_dev || d.status_count < total)
    return refuse(err, "agent entry: status row missing or short (" + std::to_string(d.status_count) + " elements declared, num_envs * num_vehicles is " +
                           std::to_string(total) + ": a short row would be an out-of-bounds device write)");
  if (!d.entered_dev || d.entered_count < total)
    return refuse(err, "agent entry: entered row missing or short (" + std::to_string(d.entered_count) + " elements declared, num_envs * num_vehicles is " +
                           std::to_string(total) + ": a short row would be an out-of-bounds device write)");
  for (int32_t r = 0; r < d.rows; ++r)
    for (int32_t e = 0; e < c.num_envs; ++e) {
      bool at_reset = false;
      for (uint64_t a = 0; a < agents; ++a) {
        const uint64_t i = ((uint64_t)r * (uint64_t)c.num_envs + (uint64_t)e) * agents + a;
        const int32_t t = d.ready_host[i];
        if (t < 0)
          return refuse(err, "agent entry: row " + std::to_string(r) + ", env " + std::to_string(e) + ", agent " + std::to_string(a) +
                                 ": ready tick " + std::to_string(t) + " is negative (ticks count from the reset observation)");
        at_reset = at_reset || t == 0;
        const double* q = d.check_host + i * 3;
        if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2])))
          return refuse(err, "agent entry: row " + std::to_string(r) + ", env " + std::to_string(e) + ", agent " + std::to_string(a) +
                                 ": check row is not finite");
        if (!(q[2] > 0.0))
          return refuse(err, "agent entry: row " + std::to_string(r) + ", env " + std::to_string(e) + ", agent " + std::to_string(a) +
                                 ": dimension " + std::to_string(q[2]) + " must be > 0");
      }
      if (!at_reset)
        return refuse(err, "agent entry: row " + std::to_string(r) + ", env " + std::to_string(e) +
                               " has no agent at tick 0 (the reset observation is the first that holds an agent)");
    }
  return SMX_OK;
}

// ---- Per-agent action spaces (smx_set_agent_spaces / smx_check_agent_spaces) ----
// The six spaces that drive the Ackermann chassis share the state layout, the reset and the observation pass, so only
// the control phase reads the table; a kinematic agent's slot means something else to respawn_vehicle, the guard and the
// observe role, which all read cfg.action_space: neither a kinematic entry nor a kinematic cfg.action_space is taken.
static constexpr unsigned SMX_MIXABLE_SPACES =
    (1u << SMX_ACTION_SPACE_LANE) | (1u << SMX_ACTION_SPACE_CONTINUOUS) | (1u << SMX_ACTION_SPACE_ACTUATOR_DYNAMIC) |
    (1u << SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED) | (1u << SMX_ACTION_SPACE_TRAJECTORY) | (1u << SMX_ACTION_SPACE_MPC);
inline const char* action_space_name(int32_t s) {
  static const char* const names[] = {"Lane", "Continuous", "ActuatorDynamic", "LaneWithContinuousSpeed", "Trajectory",
                                      "TargetPose", "TrajectoryWithTime", "MPC", "Imitation"};
  return (s >= 0 && s <= SMX_ACTION_SPACE_IMITATION) ? names[s] : "unknown";
}
inline int check_agent_spaces_impl(const smx_config& c, const smx_agent_spaces& d, std::string& err) {
  if (c.num_vehicles <= 0 || c.num_social < 0 || c.num_social >= c.num_vehicles)
    return refuse(err, "agent spaces: the configuration has no agents");
  if (c.action_space < 0 || c.action_space > SMX_ACTION_SPACE_IMITATION || !((SMX_MIXABLE_SPACES >> c.action_space) & 1u))
    return refuse(err, std::string("agent spaces: cfg.action_space is ") + action_space_name(c.action_space) +
                           ": a table is taken beside one of Lane, Continuous, ActuatorDynamic, LaneWithContinuousSpeed, "
                           "Trajectory and MPC only (every slot of a kinematic configuration is a kinematic agent's)");
  if (!d.space_host) return refuse(err, "agent spaces: null table (space_host)");
  const int32_t agents = c.num_vehicles - c.num_social;
  if (d.n_agents != agents)
    return refuse(err, "agent spaces: n_agents is " + std::to_string(d.n_agents) + ", num_vehicles - num_social is " + std::to_string(agents) +
                           " (slot " + std::to_string(d.n_agents < agents ? std::max(d.n_agents, 0) : agents) +
                           (d.n_agents < agents ? " has no entry)" : " is no agent slot)"));
  for (int32_t a = 0; a < agents; ++a) {
    const int32_t s = d.space_host[a];
    if (s < 0 || s > SMX_ACTION_SPACE_IMITATION)
      return refuse(err, "agent spaces: slot " + std::to_string(a) + ": " + std::to_string(s) + " is no SMX_ACTION_SPACE_* value");
    if (!((SMX_MIXABLE_SPACES >> s) & 1u))
      return refuse(err, "agent spaces: slot " + std::to_string(a) + ": " + action_space_name(s) +
                             " is a kinematic space; only Lane, Continuous, ActuatorDynamic, LaneWithContinuousSpeed, Trajectory and "
                             "MPC may be mixed");
  }
  return SMX_OK;
}
// the spaces a table holds, bit s = SMX_ACTION_SPACE_* s (a checked table)
inline unsigned agent_spaces_mask(const int32_t* space, int32_t n) {
  unsigned m = 0;
  for (int32_t a = 0; a < n; ++a) m |= 1u << space[a];
  return m;
}

// ---- History agents (smx_set_history_agents / smx_check_history_agents) ----
// The kernels index vehicle_dev by (episode mod rows, env, agent) and the two optional rows by vehicle: the counts are
// checked against those shapes here; the ids the table holds are only ever compared.  `rows`: the bound history's.
inline int check_history_agents_impl(const smx_config& c, int32_t rows, const smx_history_agents& ha, std::string& err) {
  if (c.num_envs <= 0 || c.num_vehicles <= 0) return refuse(err, "history agents: num_envs and num_vehicles must be > 0");
  if (c.action_space != SMX_ACTION_SPACE_IMITATION)
    return refuse(err, "history agents: cfg.action_space is " + std::to_string(c.action_space) +
                           ", a followed vehicle is the BoxChassis agent of SMX_ACTION_SPACE_IMITATION");
  if (c.num_social <= 0 || c.num_social >= c.num_vehicles)
    return refuse(err, "history agents: the configuration needs social slots (the history's) and at least one agent slot");
  if (rows < 1) return refuse(err, "history agents: the history's rows must be >= 1");
  if (!ha.vehicle_dev) return refuse(err, "history agents: vehicle_dev is NULL");
  const uint64_t agents = (uint64_t)(c.num_vehicles - c.num_social), total = (uint64_t)c.num_envs * (uint64_t)c.num_vehicles;
  const uint64_t need = (uint64_t)rows * (uint64_t)c.num_envs * agents;
  if (ha.vehicle_count < need)
    return refuse(err, "history agents: vehicle " + std::to_string(ha.vehicle_count) + " elements declared, rows * num_envs * agents is " +
                           std::to_string(need) + " (a short table would be an out-of-bounds device read)");
  if (ha.action_dev && ha.action_count < 3 * total)
    return refuse(err, "history agents: action " + std::to_string(ha.action_count) + " elements declared, 3 * num_envs * num_vehicles is " +
                           std::to_string(3 * total) + " (a short row would be an out-of-bounds device write)");
  if (ha.status_dev && ha.status_count < total)
    return refuse(err, "history agents: status " + std::to_string(ha.status_count) + " elements declared, num_envs * num_vehicles is " +
                           std::to_string(total) + " (a short row would be an out-of-bounds device write)");
  return SMX_OK;
}

// ---- The handover table (smx_set_history_handover / smx_check_history_handover) ----
// Indexed exactly as vehicle_dev is, (episode mod rows, env, agent): the same count; the ticks it holds are only compared.
inline int check_history_handover_impl(const smx_config& c, int32_t rows, const smx_history_handover& ho, std::string& err) {
  if (c.num_envs <= 0 || c.num_vehicles <= 0) return refuse(err, "history handover: num_envs and num_vehicles must be > 0");
  if (c.num_social <= 0 || c.num_social >= c.num_vehicles)
    return refuse(err, "history handover: the configuration needs social slots (the history's) and at least one agent slot");
  if (rows < 1) return refuse(err, "history handover: the history's rows must be >= 1");
  if (!ho.tick_dev) return refuse(err, "history handover: tick_dev is NULL");
  const uint64_t need = (uint64_t)rows * (uint64_t)c.num_envs * (uint64_t)(c.num_vehicles - c.num_social);
  if (ho.tick_count < need)
    return refuse(err, "history handover: tick " + std::to_string(ho.tick_count) + " elements declared, rows * num_envs * agents is " +
                           std::to_string(need) + " (a short table would be an out-of-bounds device read)");
  return SMX_OK;
}

// ---- Bubbles (smx_set_history_bubbles / smx_check_history_bubbles) ----
// k_bubbles indexes the two rows by vehicle and reads agent slot follow_agent of the env it works on: the counts and the
// slot are checked against those shapes here; the limits' rule is BubbleLimits.__post_init__'s.
inline int check_history_bubbles_impl(const smx_config& c, const smx_history_bubbles& hb, std::string& err) {
  if (c.num_envs <= 0 || c.num_vehicles <= 0) return refuse(err, "history bubbles: num_envs and num_vehicles must be > 0");
  if (c.num_social <= 0 || c.num_social >= c.num_vehicles)
    return refuse(err, "history bubbles: the configuration needs social slots (the history's) and at least one agent slot");
  if (c.num_vehicles - c.num_social > 64) return refuse(err, "history bubbles: an env's agent slots must fit one wavefront (64)");
  if (hb.n_bubbles < 1 || hb.n_bubbles > SMX_MAX_BUBBLES)
    return refuse(err, "history bubbles: n_bubbles is " + std::to_string(hb.n_bubbles) + ", 1 .. " + std::to_string(SMX_MAX_BUBBLES) + " are held");
  if (!hb.bubbles_host) return refuse(err, "history bubbles: bubbles_host is NULL");
  const int32_t agents = c.num_vehicles - c.num_social;
  for (int32_t i = 0; i < hb.n_bubbles; ++i) {
    const smx_bubble& b = hb.bubbles_host[i];
    const std::string at = "history bubbles: bubble " + std::to_string(i);
    const double fields[7] = {b.x, b.y, b.size_x, b.size_y, b.margin, b.offset_x, b.offset_y};
    for (double f : fields)
      if (!std::isfinite(f)) return refuse(err, at + " has a field that is not finite");
    if (!(b.size_x > 0.0 && b.size_y > 0.0)) return refuse(err, at + ": size_x and size_y must be > 0");
    if (!(b.margin > 0.0)) return refuse(err, at + ": margin must be > 0");
    if (b.follow_agent >= agents)
      return refuse(err, at + ": follow_agent is " + std::to_string(b.follow_agent) + ", an env has " + std::to_string(agents) + " agent slots");
    if (b.hijack_limit < 0 || b.shadow_limit < 0) return refuse(err, at + ": a limit is negative (0 = none)");
    if (b.shadow_limit != 0 && b.shadow_limit < b.hijack_limit)
      return refuse(err, at + ": shadow_limit " + std::to_string(b.shadow_limit) + " is below hijack_limit " + std::to_string(b.hijack_limit));
  }
  const uint64_t total = (uint64_t)c.num_envs * (uint64_t)c.num_vehicles;
  if (!hb.state_dev || !hb.cursor_dev) return refuse(err, "history bubbles: state_dev or cursor_dev is NULL");
  if (hb.state_count < total)
    return refuse(err, "history bubbles: state " + std::to_string(hb.state_count) + " elements declared, num_envs * num_vehicles is " +
                           std::to_string(total) + " (a short row would be an out-of-bounds device write)");
  if (hb.cursor_count < total)
    return refuse(err, "history bubbles: cursor " + std::to_string(hb.cursor_count) + " elements declared, num_envs * num_vehicles is " +
                           std::to_string(total) + " (a short row would be an out-of-bounds device write)");
  return SMX_OK;
}

// ---- Frame stacking (smx_bind_frame_stack / smx_check_frame_stack) ----
// bytes per agent of a stackable source, 0 with the reason in `err`: a row of smx_outputs by its SMX_OUT_* index — stackable,
// its sensor on, its elements times the size of its dtype — or the image by SMX_STACK_SOURCE_RGB
inline uint64_t stack_row_bytes(const smx_config& c, int32_t source, std::string& err) {
  bool on = false;
  uint64_t bytes = 0;
  if (source == SMX_STACK_SOURCE_RGB) {
    on = (c.sensors & SMX_SENSOR_RGB) != 0, bytes = (uint64_t)c.rgb_width * c.rgb_height * 3;
  } else if (source >= 0 && source < SMX_OUT_BUFFERS && OUT_ROWS[source].stackable) {
    const BufRow& r = OUT_ROWS[source];
    on = row_sensor_on(r, c) && (r.null_error != NULL_WITH_VIAS || c.via_max > 0);
    bytes = r.per_unit(c) * dtype_size(r.dtype);
  } else {
    return refuse(err, "frame stack: source " + std::to_string(source) + " is not a per-agent row that can be stacked "
                       "(an SMX_OUT_* index other than env_done, learner and final_*, or SMX_STACK_SOURCE_RGB)", 0);
  }
  if (!on || bytes == 0) return refuse(err, "frame stack: the sensor of source " + std::to_string(source) + " is off in this configuration", 0);
  if (bytes > (1ull << 30)) return refuse(err, "frame stack: a row of more than 2^30 bytes per agent", 0);
  return bytes;
}

// SMX_OK with the bytes per agent and frame in `row`, or the code with the reason in `err`
inline int check_frame_stack_impl(const smx_config& c, int32_t source, int32_t layout, uint64_t bytes, uint64_t& row, std::string& err) {
  row = 0;
  if (const char* why = frame_stack_config_error(c)) return refuse(err, why);
  if (c.frame_stack == 0) return refuse(err, "frame stack: smx_config.frame_stack is 0 (off): nothing can be bound", SMX_ERR_STATE);
  if (c.num_envs <= 0 || c.num_vehicles <= 0) return refuse(err, "frame stack: num_envs and num_vehicles must be > 0");
  if (layout != SMX_STACK_FRAMES && layout != SMX_STACK_DSTACK)
    return refuse(err, "frame stack: unknown layout " + std::to_string(layout) + " (SMX_STACK_FRAMES or SMX_STACK_DSTACK)");
  if (layout == SMX_STACK_DSTACK && source != SMX_STACK_SOURCE_RGB)
    return refuse(err, "frame stack: SMX_STACK_DSTACK is the layout of the RGB image alone (SMX_STACK_SOURCE_RGB); the single-channel "
                       "grids and the rows already have a fixed shape in SMX_STACK_FRAMES");
  row = stack_row_bytes(c, source, err);
  if (!row) return SMX_ERR_INVALID;
  const uint64_t need = (uint64_t)c.num_envs * (uint64_t)c.num_vehicles * (uint64_t)c.frame_stack * row;
  if (bytes < need)
    return refuse(err, "frame stack: " + std::to_string(bytes) + " bytes declared for source " + std::to_string(source) +
                           ", the configuration needs " + std::to_string(need) + " (a short buffer would be an out-of-bounds device write)");
  return SMX_OK;
}

// The launch geometry of a pass's frame-stack kernels.  k_frame_push: a thread owns one column of `unit` bytes of an
// agent's row — 16 where the row's size and both addresses are multiples of 16, 4 likewise, else 1 — and the bindings'
// workgroups follow one another from block0.  k_frame_dstack: a thread owns four pixels of the image.
constexpr uint64_t STACK_BLOCKS_CAP = 1ull << 31;  // workgroups a launch may have: below this
struct StackColumns {
  uint32_t unit, block0;
};
// a SMX_STACK_FRAMES binding behind `blocks` workgroups of earlier ones; `blocks` grows by its own
inline StackColumns stack_push_place(uint64_t row, uintptr_t src, uintptr_t dst, uint64_t total, uint64_t& blocks) {
  const uintptr_t both = src | dst | (uintptr_t)row;
  StackColumns s;
  s.unit = (both & 15) == 0 ? 16 : (both & 3) == 0 ? 4 : 1;
  s.block0 = (uint32_t)blocks;
  blocks += (total * (row / s.unit) + SMX_HOST_STACK_BLOCK - 1) / SMX_HOST_STACK_BLOCK;
  return s;
}
inline uint64_t stack_dstack_blocks(uint64_t row, uint64_t total) {
  return (total * ((row / 3 + 3) / 4) + SMX_HOST_STACK_BLOCK - 1) / SMX_HOST_STACK_BLOCK;
}

// ---- The map tables (smx_load_map) ----
// Every record index stored in the tables is range-checked here, once, so that the kernels can follow them without
// bounds tests.  (Not checked: lane_road, lane_out_idx, road_lanes, lpg_pts, that the offset arrays ascend, and sg_off
// is read before its NULL test — DESIGN.md section 9.)
inline const char* map_tables_error(const smx_map_tables& t) {
  if (t.n_lanes <= 0 || t.n_roads <= 0 || t.n_lanepoints <= 0) return "empty map tables";
  if (t.n_lanes > 32767) return "lane ids are reported as int16: at most 32767 lanes";
  const size_t sg_cells = (size_t)t.sg_nx * t.sg_ny;
  for (int i = 0; i < t.n_lanepoints; ++i) {
    const smx_lp_rec& r = t.lp_rec[i];
    if (r.lane < 0 || r.lane >= t.n_lanes || r.next0 >= t.n_lanepoints || r.knot_next >= t.n_lanepoints ||
        (r.n_next > 0 && (r.next_off < 0 || r.next_off + r.n_next > t.n_succ || r.next0 < 0 || r.knot_next < 0)))
      return "lanepoint record out of range";
  }
  for (int i = 0; i < t.n_succ; ++i) {
    const smx_succ_rec& r = t.succ_rec[i];
    if (r.idx < 0 || r.idx >= t.n_lanepoints || r.knot < 0 || r.knot >= t.n_lanepoints || r.lane < 0 || r.lane >= t.n_lanes || r.hops < 1)
      return "successor record out of range";
  }
  for (int i = 0; i < t.sg_off[sg_cells]; ++i)
    if (t.sg_rec[i].lane < 0 || t.sg_rec[i].lane >= t.n_lanes || t.sg_rec[i].v0 < 0 || t.sg_rec[i].v0 + 1 >= t.n_shape_pts)
      return "segment record out of range";
  if (!t.lane_in_off || !t.lane_in_idx || !t.road_par_off || !t.road_par_idx) return "map tables: lane_in_* / road_par_* missing";
  for (int i = 0; i < t.lane_in_off[t.n_lanes]; ++i)
    if (t.lane_in_idx[i] < 0 || t.lane_in_idx[i] >= t.n_lanes) return "incoming lane out of range";
  for (int i = 0; i < t.road_par_off[t.n_roads]; ++i)
    if (t.road_par_idx[i] < 0 || t.road_par_idx[i] >= t.n_roads) return "parallel road out of range";
  return nullptr;
}

// The 26 tables of smx_map_tables `t`, each once: X(field, element type, elements).  The blob writer and the re-pointing
// into the device blob both expand it.
#define SMX_MAP_TABLES(X, t)                                                    \
  X(lane_road, int32_t, (t).n_lanes)                                            \
  X(lane_index, int32_t, (t).n_lanes)                                           \
  X(lane_width, double, (t).n_lanes)                                            \
  X(lane_speed, double, (t).n_lanes)                                            \
  X(lane_length, double, (t).n_lanes)                                           \
  X(lane_in_junction, uint8_t, (t).n_lanes)                                     \
  X(lane_shape_off, int32_t, (size_t)(t).n_lanes + 1)                           \
  X(shape_x, double, (t).n_shape_pts)                                           \
  X(shape_y, double, (t).n_shape_pts)                                           \
  X(shape_rec, smx_shape_rec, (t).n_shape_pts)                                  \
  X(lane_out_off, int32_t, (size_t)(t).n_lanes + 1)                             \
  X(lane_out_idx, int32_t, (t).lane_out_off[(t).n_lanes])                       \
  X(lane_in_off, int32_t, (size_t)(t).n_lanes + 1)                              \
  X(lane_in_idx, int32_t, (t).lane_in_off[(t).n_lanes])                         \
  X(road_par_off, int32_t, (size_t)(t).n_roads + 1)                             \
  X(road_par_idx, int32_t, (t).road_par_off[(t).n_roads])                       \
  X(road_lane_off, int32_t, (size_t)(t).n_roads + 1)                            \
  X(road_lanes, int32_t, (t).road_lane_off[(t).n_roads])                        \
  X(road_is_junction, uint8_t, (t).n_roads)                                     \
  X(road_out_road, int32_t, (t).n_roads)                                        \
  X(lp_rec, smx_lp_rec, (t).n_lanepoints)                                       \
  X(succ_rec, smx_succ_rec, (t).n_succ)                                         \
  X(lpg_off, int32_t, (size_t)(t).lpg_nx * (t).lpg_ny + 1)                      \
  X(lpg_pts, smx_pt_rec, (t).lpg_off[(size_t)(t).lpg_nx * (t).lpg_ny])          \
  X(sg_off, int32_t, (size_t)(t).sg_nx * (t).sg_ny + 1)                         \
  X(sg_rec, smx_seg_rec, (t).sg_off[(size_t)(t).sg_nx * (t).sg_ny])

// the host image of the one device allocation that holds every table, each at a multiple of 256 bytes
struct BlobWriter {
  std::string host;
  size_t add(const void* p, size_t bytes) {
    size_t off = (host.size() + 255) & ~size_t(255);
    host.resize(off + bytes);
    if (bytes) memcpy(&host[off], p, bytes);
    return off;
  }
};

// Lanes of the map split: some lanepoint has several successors.  (Junction-internal lanes alone do not tell — the loop
// map's two edges are joined by six of them, one successor each.)
inline bool map_lanes_split(const smx_map_tables& t) {
  for (int i = 0; i < t.n_lanepoints; ++i)
    if (t.lp_rec[i].n_next > 1) return true;
  return false;
}

// The slow lists' kernels run a fixed grid that strides a list whose length only the device knows.  On a map whose
// lanes never split the lists hold a few vehicles of a hundred thousand and the grid is an empty launch's latency; where
// lanes branch or cross, a third of the vehicles is on them (minicity, 262 144 vehicles: 77 000 rows through 512
// workgroups were half a wavefront per SIMD for nine passes, 1.4 ms of a 2.8 ms tick) — a team slot for every second
// vehicle then.
inline int slow_list_blocks(bool lanes_split, size_t total_vehicles) {
  const size_t teams_per_block = SMX_HOST_BLOCK / SMX_HOST_WP_LANES;
  if (!lanes_split) return SMX_HOST_SLOW_BLOCKS;
  return (int)std::min<size_t>(8192, std::max<size_t>(SMX_HOST_SLOW_BLOCKS, total_vehicles / (2 * teams_per_block)));
}

// half the widest lane width of the map
inline double map_dagm_reach(const smx_map_tables& t) {
  double reach = 0.0;
  for (int i = 0; i < t.n_lanes; ++i) reach = std::max(reach, 0.5 * t.lane_width[i]);
  return reach;
}

// ---- Missions (smx_set_missions, smx_set_mission_goals) ----
struct RouteTables {
  std::vector<int16_t> pos;      // [n_slots][n_roads] position of the road in the slot's route, -1: not on it
  std::vector<uint8_t> lane_ok;  // [n_slots][n_lanes] the route filter of lanepoints.py:666-683, per lane
  std::vector<int32_t> last;     // [n_slots] the route's last road, -1: empty route
  std::vector<double> goal;      // [n_slots][3] x, y, radius
  bool any = false;              // some slot has a fixed route
};

// The route tables of the slots' missions (null), or why the missions are refused.  lane_road, lane_out_off and
// lane_out_idx: the loaded map's, n_lanes (+ 1) entries.
inline const char* route_tables(const smx_mission* missions, int32_t n_slots, const int32_t* route_roads, int32_t n_route_roads,
                                int32_t n_roads, int32_t n_lanes, const std::vector<int32_t>& lane_road,
                                const std::vector<int32_t>& lane_out_off, const std::vector<int32_t>& lane_out_idx, RouteTables& out) {
  const int nr = n_roads, nl = n_lanes;
  out.pos.assign((size_t)n_slots * nr, (int16_t)-1);
  out.lane_ok.assign((size_t)n_slots * nl, (uint8_t)0);
  out.last.assign((size_t)n_slots, -1);
  out.goal.assign((size_t)n_slots * 3, 0.0);
  out.any = false;
  for (int s = 0; s < n_slots; ++s) {
    const smx_mission& ms = missions[s];
    if (ms.route_len == 0) continue;  // endless mission: empty route (plan.py:321-323)
    if (ms.route_len < 0 || ms.route_len > 32767 || ms.route_off < 0 || (int64_t)ms.route_off + ms.route_len > n_route_roads)
      return "smx_set_missions: route range outside route_roads (at most 32767 roads)";
    if (!(ms.goal_radius >= 0.0) || !std::isfinite(ms.goal_x) || !std::isfinite(ms.goal_y))
      return "smx_set_missions: a fixed route needs a PositionalGoal (finite position, radius >= 0)";
    int16_t* on = &out.pos[(size_t)s * nr];
    for (int k = 0; k < ms.route_len; ++k) {
      const int road = route_roads[ms.route_off + k];
      if (road < 0 || road >= nr) return "smx_set_missions: road index out of range";
      if (on[road] < 0) on[road] = (int16_t)k;  // first occurrence: `min` over the route keeps the first minimum
    }
    out.last[s] = route_roads[ms.route_off + ms.route_len - 1];
    // lanepoints.py:666-683 per lane (the rule lane_allowed evaluates for the short in-junction lists): on a road
    // of the route, and — unless that is the route's last road — leading on to a road of the route
    for (int lane = 0; lane < nl; ++lane) {
      const int road = lane_road[lane];
      bool ok = on[road] >= 0;
      if (ok && road != out.last[s]) {
        bool leads_on = false;
        for (int k = lane_out_off[lane]; k < lane_out_off[lane + 1]; ++k) leads_on = leads_on || on[lane_road[lane_out_idx[k]]] >= 0;
        ok = leads_on;
      }
      out.lane_ok[(size_t)s * nl + lane] = ok ? 1 : 0;
    }
    out.goal[3 * s] = ms.goal_x;
    out.goal[3 * s + 1] = ms.goal_y;
    out.goal[3 * s + 2] = ms.goal_radius;
    out.any = true;
  }
  return nullptr;
}

// smx_check_mission_goals: the table on its own ("" = good)
inline std::string mission_goals_error(const smx_mission_goal* goals, int32_t n_slots, int32_t num_vehicles, const double* lane_end_heading,
                                       const int32_t* lane_dead_end, int32_t n_lanes, int32_t map_lanes) {
  if (n_slots < 0 || (n_slots > 0 && !goals)) return "smx_set_mission_goals: null table";
  if (n_slots != 0 && n_slots != num_vehicles) return "smx_set_mission_goals: one goal per vehicle slot (cfg.num_vehicles)";
  bool traverse = false;
  for (int s = 0; s < n_slots; ++s) {
    const smx_mission_goal& g = goals[s];
    const std::string at = "smx_set_mission_goals: slot " + std::to_string(s);
    if (g.kind == SMX_GOAL_LAP) {
      if (g.num_laps < 1) return at + ": num_laps must be >= 1";
      if (!std::isfinite(g.route_length) || g.route_length < 0.0) return at + ": route_length must be finite and >= 0";
    } else if (g.kind == SMX_GOAL_TRAVERSE) {
      traverse = true;
    } else if (g.kind != SMX_GOAL_POSITIONAL) {
      return at + ": unknown goal kind " + std::to_string(g.kind);
    }
  }
  if (traverse) {
    if (!lane_end_heading || !lane_dead_end) return "smx_set_mission_goals: a traverse goal needs the lane tables (lane_end_heading, lane_dead_end)";
    if (n_lanes != map_lanes) return "smx_set_mission_goals: n_lanes is not the map's lane count";
    for (int l = 0; l < n_lanes; ++l)
      if (!std::isfinite(lane_end_heading[l])) return "smx_set_mission_goals: lane_end_heading not finite";
  }
  return std::string();
}

// ... and against the slots' routes (route_last: smx_set_missions' last roads, -1 or no entry: an empty route).  `any`: some
// goal is not positional; `traverse`: some goal is a traverse goal.
inline const char* mission_goals_route_error(const smx_mission_goal* goals, int32_t n_slots, const std::vector<int32_t>& route_last,
                                             bool& any, bool& traverse) {
  any = traverse = false;
  for (int s = 0; s < n_slots; ++s) {
    const bool routed = s < (int)route_last.size() && route_last[s] >= 0;
    if (goals[s].kind == SMX_GOAL_LAP && !routed)
      return "smx_set_mission_goals: a lap goal needs the slot's fixed route and PositionalGoal (smx_set_missions)";
    if (goals[s].kind == SMX_GOAL_TRAVERSE && routed)
      return "smx_set_mission_goals: a traverse goal has an empty route (smx_mission.route_len = 0)";
    any = any || goals[s].kind != SMX_GOAL_POSITIONAL;
    traverse = traverse || goals[s].kind == SMX_GOAL_TRAVERSE;
  }
  return nullptr;
}

// ---- Mission pool (smx_set_mission_pool) ----
// What the handle copies to the device: every per-mission table with n_missions + 1 entries — the pool's missions and,
// last, the endless mission that a table entry of -1 resolves to (MissionsDev, smx_roadmap.h).
struct MissionPoolTables {
  RouteTables rt;                       // [n_missions + 1] rows
  std::vector<smx_mission_goal> goals;  // [n_missions + 1]; empty: every goal positional
  std::vector<int32_t> via_off;         // [n_missions + 2]
  bool traverse = false;                // some goal is a traverse goal: the two lane tables ride along
};

// The pool against the configuration and the map it is for (n_roads, n_lanes and the three lane tables of route_tables):
// "" and the tables, or why the pool is refused.  The checks of smx_set_missions, smx_set_mission_goals and smx_set_vias
// per pool entry; rows_dev, device memory, is tested for NULL and its declared size only.
inline std::string mission_pool_error(const smx_config& c, const smx_mission_pool& p, int32_t n_roads, int32_t n_lanes,
                                      const std::vector<int32_t>& lane_road, const std::vector<int32_t>& lane_out_off,
                                      const std::vector<int32_t>& lane_out_idx, MissionPoolTables& out) {
  const std::string at = "smx_set_mission_pool: ";
  if (c.num_envs <= 0 || c.num_vehicles <= 0 || c.num_social < 0 || c.num_social >= c.num_vehicles)
    return at + "the configuration has no agent slot";
  const int M = p.n_missions;
  if (M < 1 || M > SMX_MISSION_POOL_MAX) return at + "n_missions must be 1 .. SMX_MISSION_POOL_MAX (" SMX_STR(SMX_MISSION_POOL_MAX) ")";
  if (!p.missions_host || p.n_route_roads < 0 || (p.n_route_roads > 0 && !p.route_roads_host)) return at + "null table (missions_host / route_roads_host)";
  if (!p.rows_dev) return at + "null table (rows_dev)";
  if (p.rows < 1) return at + "rows must be >= 1";
  const uint64_t want = (uint64_t)p.rows * (uint64_t)c.num_envs * (uint64_t)(c.num_vehicles - c.num_social);
  if (want > 0x7fffffffull) return at + "rows x num_envs x agents too large (the table is indexed with 32 bits)";
  if (p.rows_count < want)
    return at + "rows_dev holds " + std::to_string(p.rows_count) + " entries, rows x num_envs x agents needs " + std::to_string(want);
  if (((size_t)M + 1) * (size_t)n_roads > 0x7fffffffull) return at + "missions x roads too large";
  if (((size_t)M + 1) * (size_t)n_lanes > 0x7fffffffull) return at + "missions x lanes too large";  // (route_lane_ok's index)
  std::vector<smx_mission> ms(p.missions_host, p.missions_host + M);
  ms.push_back(smx_mission{});  // (route_len 0: the endless mission)
  if (const char* why = route_tables(ms.data(), M + 1, p.route_roads_host, p.n_route_roads, n_roads, n_lanes, lane_road, lane_out_off, lane_out_idx, out.rt))
    return at + why;
  out.goals.clear();
  out.traverse = false;
  if (p.goals_host) {
    const std::string msg = mission_goals_error(p.goals_host, M, M, p.lane_end_heading_host, p.lane_dead_end_host, p.n_lanes, n_lanes);
    if (!msg.empty()) return at + msg;
    bool any = false;
    if (const char* why = mission_goals_route_error(p.goals_host, M, out.rt.last, any, out.traverse)) return at + why;
    if (any) {
      out.goals.assign(p.goals_host, p.goals_host + M);
      out.goals.push_back(smx_mission_goal{SMX_GOAL_POSITIONAL, 0, 0.0});
    }
  }
  if (p.n_vias < 0 || (p.n_vias > 0 && (!p.vias_host || !p.via_off_host))) return at + "null table (vias_host / via_off_host)";
  if (p.n_vias > 0 && c.via_max <= 0) return at + "vias need cfg.via_max > 0";
  out.via_off.assign((size_t)M + 2, p.n_vias);
  if (p.n_vias > 0) {
    if (p.via_off_host[0] != 0 || p.via_off_host[M] != p.n_vias) return at + "via offsets must run from 0 to n_vias";
    for (int m = 0; m < M; ++m)
      if (p.via_off_host[m + 1] < p.via_off_host[m] || p.via_off_host[m + 1] - p.via_off_host[m] > 32)
        return at + "at most 32 vias per mission, offsets ascending (mission " + std::to_string(m) + ")";
    for (int i = 0; i < p.n_vias; ++i)
      if (p.vias_host[i].lane < 0 || p.vias_host[i].lane >= n_lanes) return at + "via lane index out of range";
    std::copy(p.via_off_host, p.via_off_host + M + 1, out.via_off.begin());
  }
  return std::string();
}

// smx_check_mission_pool: the same against the host tables of the map
inline int check_mission_pool_impl(const smx_config& c, const smx_map_tables& map, const smx_mission_pool& p, std::string& err) {
  if (map.n_lanes <= 0 || map.n_roads <= 0 || !map.lane_road || !map.lane_out_off || !map.lane_out_idx)
    return refuse(err, "smx_check_mission_pool: the map tables lack lane_road / lane_out_off / lane_out_idx");
  const std::vector<int32_t> lane_road(map.lane_road, map.lane_road + map.n_lanes);
  const std::vector<int32_t> lane_out_off(map.lane_out_off, map.lane_out_off + map.n_lanes + 1);
  const std::vector<int32_t> lane_out_idx(map.lane_out_idx, map.lane_out_idx + lane_out_off[map.n_lanes]);
  for (int32_t r : lane_road)
    if (r < 0 || r >= map.n_roads) return refuse(err, "smx_check_mission_pool: lane_road out of range");
  for (int l = 0; l < map.n_lanes; ++l)
    if (lane_out_off[l] < 0 || lane_out_off[l + 1] < lane_out_off[l]) return refuse(err, "smx_check_mission_pool: lane_out_off not ascending");
  for (int32_t l : lane_out_idx)
    if (l < 0 || l >= map.n_lanes) return refuse(err, "smx_check_mission_pool: lane_out_idx out of range");
  MissionPoolTables t;
  const std::string msg = mission_pool_error(c, p, map.n_roads, map.n_lanes, lane_road, lane_out_off, lane_out_idx, t);
  return msg.empty() ? SMX_OK : refuse(err, msg);
}

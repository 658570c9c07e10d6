// smx_kernels.hip — the C-ABI of the SMARTS hot path on gfx950 and the code that launches its per-tick kernels.
//
// A tick = SMARTS._step (smarts.py:236-327) for every environment instance of the shard, as a short
// sequence of kernels on one stream (each stage has its own natural thread mapping; together
// they stay far below the register pressure of one fused kernel):
//
//   k_control   4 lanes / vehicle       A controllers (_perform_agent_actions, smarts.py:1233-1263):
//                                         the team finds the controller's waypoint path together
//                                       B physics     (_step_pybullet, smarts.py:923-931)
//   k_scan      8 lanes / vehicle       map sweeps at the new pose: nearest lane / road_with_point
//                                       at centre + 4 corners, lane heading (wrong way); 10 nearest
//                                       lanepoints, path seeds
//   k_sensors   workgroup roles         waypoints role  4 lanes / vehicle: waypoint paths streamed
//                                         into the dense rows, trip meter / reward
//                                       observe role    1 lane / vehicle, whole envs / workgroup:
//                                         collisions, neighbours, ego block, accelerometer, driven
//                                         path, events, done
//                                       lidar / OGM roles  1 wavefront / vehicle
//   k_tail      1 lane / vehicle        new flags (teardown), dones["__all__"], auto-reset respawn,
//                                       the new vehicles' grid tiles, the next tick's alive list
//
// followed, for envs whose episode ended under auto_reset (parallel_env.py:303-309), by k_first: scan /
// sensors / commit restricted to the re-created vehicles.  Above 16384 vehicles every role is
// launched on its own (k_waypoints, k_observe, k_lidar, k_ogm; see enqueue()).  Envs are independent
// (reference: one process per env, parallel_env.py:96-122): no inter-workgroup communication.
//
// Every kernel is in the header of its phase, included below: smx_k_control.h (every k_control form, the kinematic forms,
// k_bubbles, k_social), smx_k_scan.h (k_scan and its listed forms), smx_k_entry.h (delayed entry), smx_k_waypoints.h (the
// waypoints role's three forms, k_wp_walk, k_knot_table, k_waypoints and its listed forms), smx_k_grids.h (OGM / DAGM / RGB
// roles, k_ogm, k_dagm, k_rgb), smx_k_lidar.h (lidar role, k_lidar, k_lidar_first), smx_k_observe.h (observe role,
// k_observe), smx_k_pass.h (k_alive_list, the commit role, k_sensors, k_first, k_tail, k_reset) and smx_k_rows.h
// (k_road_waypoints, k_lane_ttc, k_ego_frame, k_actions_to_world, the frame stacks, k_copy_agent_dims); what the phases
// share is in smx_tick.h.  This file defines no device code: it names kernels only to launch them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "smx_bubbles.h"
#include "smx_guard.h"
#include "smx_handle.h"
#include "smx_history.h"
#include "smx_host.h"
#include "smx_k_control.h"
#include "smx_k_grids.h"
#include "smx_k_lidar.h"
#include "smx_k_observe.h"
#include "smx_k_pass.h"
#include "smx_k_rows.h"
#include "smx_k_scan.h"
#include "smx_k_entry.h"  // (after smx_k_scan.h: its large-form instance runs the facts half for an entrant)
#include "smx_k_waypoints.h"
#include "smx_plan.h"
#include "smx_scan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

// =================================================================================
// C-ABI (include/smx.h)
// =================================================================================
extern "C" const char* smx_version(void) { return "smarts-mi355x 0.2 (gfx950)"; }

#ifdef SMX_DEBUG_TIMING
extern "C" int smx_span_read(unsigned int* out) {  // developer: [kernel][wavefront] spans of the last launches, 10 ns units
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(smx_span), sizeof(unsigned int) * SMX_SPAN_KERNELS * SMX_SPAN_WAVES) != hipSuccess) return -2;
  return 0;
}

extern "C" int smx_prof_read(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(smx_prof), 128 * sizeof(unsigned long long)) != hipSuccess) return -2;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(smx_prof), z, sizeof(z)) != hipSuccess) return -2;
  }
  return 0;
}
#endif
#ifdef SMX_DEBUG_BOUNDS
extern "C" int smx_debug_read(int* site, long long* value) {
  if (hipMemcpyFromSymbol(site, HIP_SYMBOL(smx_dbg_site), sizeof(int)) != hipSuccess) return -2;
  if (hipMemcpyFromSymbol(value, HIP_SYMBOL(smx_dbg_value), sizeof(long long)) != hipSuccess) return -2;
  int aux[8];
  if (hipMemcpyFromSymbol(aux, HIP_SYMBOL(smx_dbg_aux), sizeof(aux)) != hipSuccess) return -2;
  double f[64];
  if (hipMemcpyFromSymbol(f, HIP_SYMBOL(smx_dbg_f), sizeof(f)) != hipSuccess) return -2;
  printf("dbg ctrl: wp_n=%g la_num=%g lax=%.6f lay=%.6f lah=%.6f n_paths=%g want=%g curv=%g\n", f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]);
  for (int k = 0; k < 17; ++k) printf("  wp%d %.6f %.6f %.6f\n", k, f[8 + 3 * k], f[9 + 3 * k], f[10 + 3 * k]);
  printf("dbg aux: first=%d remaining=%d hops=%d n_next=%d lane=%d next0=%d cur_idx=%d mem_next0=%d\n", aux[0], aux[1], aux[2], aux[3], aux[4], aux[5], aux[6], aux[7]);
  return 0;
}
#endif

extern "C" uint64_t smx_struct_size(int which) {
  switch (which) {
    case 0: return sizeof(smx_config);
    case 1: return sizeof(smx_map_tables);
    case 2: return sizeof(smx_state);
    case 3: return sizeof(smx_spawns);
    case 4: return sizeof(smx_outputs);
    default: return 0;
  }
}

// the constants smx_host.h decides with are the device side's
static_assert(SMX_HOST_BLOCK == SMX_BLOCK && SMX_HOST_WP_LANES == SMX_WP_LANES && SMX_HOST_MAX_KNOTS == SMX_MAX_KNOTS &&
                  SMX_HOST_SLOW_BLOCKS == SMX_SLOW_BLOCKS && SMX_HOST_STACK_BLOCK == SMX_STACK_BLOCK,
              "smx_host.h mirrors these");

static int copy_agent_dims(smx_handle h, const double* from, double* to) {
  const size_t total = (size_t)h->cfg.num_envs * (size_t)h->cfg.num_vehicles;
  hipLaunchKernelGGL(k_copy_agent_dims, dim3((unsigned)((total + SMX_BLOCK - 1) / SMX_BLOCK)), dim3(SMX_BLOCK), 0, 0, from, to,
                     h->cfg.num_vehicles, h->cfg.num_vehicles - h->cfg.num_social, total);
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}

// the map's knot table, for load_map_impl (smx_handle.h)
static int build_knot_table(smx_handle h, KnotRow* table) {
  hipLaunchKernelGGL(k_knot_table, dim3(smx_blocks((size_t)h->map.n_lanepoints)), dim3(SMX_BLOCK), 0, 0, h->map, (int)h->cfg.wp_lookahead,
                     table, h->knot_stats.get<int32_t>());
  SMX_HIP(hipGetLastError());
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}

extern "C" int smx_create(const smx_config* cfg, int device, smx_handle* out) {
  const int rc = create_impl(cfg, device, out, KernelSide{SMX_WPE_POOL, SMX_WPE_SPILL_GROUP_BYTES, SMX_SIDE_PRIO, build_knot_table, copy_agent_dims});
#ifdef SMX_DEBUG_TIMING
  if (const char* dbg = getenv("SMX_DEBUG_SKIP"))
    if (rc == SMX_OK) (*out)->debug_skip = atoi(dbg);
#endif
  return rc;
}

extern "C" int smx_set_launch_strategy(smx_handle h, int strategy) {
  if (!h) return SMX_ERR_INVALID;
  if (strategy < SMX_LAUNCH_AUTO || strategy > SMX_LAUNCH_LARGE_TEAMS) return fail(h, SMX_ERR_INVALID, "unknown launch strategy");
  h->launch_strategy = strategy;
  return SMX_OK;
}

// What a call's plan (smx_plan.h) may depend on, read off the handle.  `st`: the caller's state block, for the carried
// alive list (null: no tick is planned, only the form is asked for).
// `follow`: the call is smx_step_history_agents; `handover`: smx_step_history_handover; `mixed`: smx_step_mixed.
static PlanInputs plan_inputs(const smx_handle_s* h, bool is_step, const smx_state* st, bool follow = false, bool handover = false,
                              bool mixed = false) {
  PlanInputs in{};
  in.cfg = &h->cfg;
  in.launch_strategy = h->launch_strategy;
  in.map_junctions = h->map_junctions;
  in.slow_blocks = h->slow_blocks;
  in.routed = h->missions.route_last != nullptr;  // (a mission pool: some pool entry has a fixed route)
  in.pool_bound = h->missions.rows != nullptr;
  in.is_step = is_step;
  in.phase_timing = h->phase_timing && h->ph_used < 16384;
  in.side_ready = h->streams.ready;
  in.list_carried = st && h->list_ready && std::memcmp(&h->list_state, st, sizeof(smx_state)) == 0;
  in.debug_skip = (SMX_SKIP(*h, SMX_SKIP_FORCE_SMALL) ? SMX_SKIP_FORCE_SMALL : 0) |
                  (SMX_SKIP(*h, SMX_SKIP_FORCE_SCAN_SPLIT) ? SMX_SKIP_FORCE_SCAN_SPLIT : 0);
  in.alive_blob = (bool)h->alive_blob;
  in.knots_blob = (bool)h->knots_blob;
  in.knot_table = h->knot_table && h->knot_table_mode != 0;
  in.ctrl_blob = (bool)h->ctrl_blob;
  in.pending_blob = h->pending_blob.get<uint8_t>();
  in.slow = SlowLists{h->slow_blob.get<int32_t>(), (size_t)h->cfg.num_envs * h->cfg.num_vehicles};
  in.slow_parity = h->alive_parity;
  in.frame_stack_bound = !h->stacks.empty();
  in.guard_bound = h->guard_out != nullptr;
  in.dims_bound = h->dims.table != nullptr;
  in.agent_dims_bound = h->dims.agent != nullptr;
  in.history_bound = h->history.vehicle != nullptr;
  in.follow_entry = follow;
  in.ogm_mask = h->ogm_mask && h->ogm_delta;
  in.handover_entry = handover;
  in.bubbles_bound = h->bubble_state != nullptr;
  in.entry_bound = h->entry.ready != nullptr;
  in.agent_spaces = h->spaces.space != nullptr ? h->spaces.mask : 0u;
  in.mixed_entry = mixed;
  return in;
}

extern "C" int smx_launch_form(smx_handle h) {
  if (!h) return SMX_ERR_INVALID;
  if (!h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_launch_form needs the map (the form depends on it)");
  return tick_plan(plan_inputs(h, false, nullptr)).form;
}

extern "C" int smx_set_controller_gains(smx_handle h, double heading_gain, double lateral_gain) {
  if (!h) return SMX_ERR_INVALID;
  h->heading_gain_pos = heading_gain;
  h->lateral_gain_pos = lateral_gain;
  return SMX_OK;
}

extern "C" int smx_load_map(smx_handle h, const smx_map_tables* t) { return load_map_impl(h, t); }

extern "C" int smx_set_vias(smx_handle h, const smx_via* vias_host, int32_t n, const int32_t* slot_off_host) {
  return set_vias_impl(h, vias_host, n, slot_off_host);
}

extern "C" int smx_set_missions(smx_handle h, const smx_mission* missions_host, int32_t n_slots,
                                const int32_t* route_roads_host, int32_t n_route_roads) {
  return set_missions_impl(h, missions_host, n_slots, route_roads_host, n_route_roads);
}

extern "C" int smx_check_mission_goals(const smx_mission_goal* goals, int32_t n_slots, int32_t num_vehicles,
                                       const double* lane_end_heading, const int32_t* lane_dead_end, int32_t n_lanes,
                                       int32_t map_lanes, char* err, uint64_t err_len) {
  const std::string msg = mission_goals_error(goals, n_slots, num_vehicles, lane_end_heading, lane_dead_end, n_lanes, map_lanes);
  return report(msg.empty() ? SMX_OK : SMX_ERR_INVALID, msg, err, err_len);
}

extern "C" int smx_set_mission_goals(smx_handle h, const smx_mission_goal* goals_host, int32_t n_slots,
                                     const double* lane_end_heading_host, const int32_t* lane_dead_end_host, int32_t n_lanes) {
  return set_mission_goals_impl(h, goals_host, n_slots, lane_end_heading_host, lane_dead_end_host, n_lanes);
}

extern "C" int smx_set_mission_pool(smx_handle h, const smx_mission_pool* pool) { return set_mission_pool_impl(h, pool); }

extern "C" int smx_check_mission_pool(const smx_config* cfg, const smx_map_tables* map, const smx_mission_pool* pool, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && map && pool) ? check_mission_pool_impl(*cfg, *map, *pool, msg) : refuse(msg, "null config, map or pool");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_lidar_rays(smx_handle h, const double* rays_dev, int32_t n_rays) { return set_lidar_rays_impl(h, rays_dev, n_rays); }

// ---- the smx_check_* entry points: smx_host.h's checks, callable without a device or a handle ----
extern "C" int smx_check_buffers(const smx_config* cfg, int has_vias, const smx_state* st, const smx_spawns* sp,
                                 const smx_outputs* out, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = cfg ? check_buffers_impl(*cfg, has_vias != 0, st, sp, out, msg) : refuse(msg, "null config");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_check_rgb_output(const smx_config* cfg, uint64_t count, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = cfg ? check_rgb_output_impl(*cfg, count, msg) : refuse(msg, "null config");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_check_guard(const smx_config* cfg, uint64_t count, double margin, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = cfg ? check_guard_impl(*cfg, count, margin, msg) : refuse(msg, "null config");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_check_frame_stack(const smx_config* cfg, int32_t source, int32_t layout, uint64_t bytes, char* err, uint64_t err_len) {
  std::string msg;
  uint64_t row;
  const int rc = cfg ? check_frame_stack_impl(*cfg, source, layout, bytes, row, msg) : refuse(msg, "null config");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_rgb_output(smx_handle h, uint8_t* rgb_dev, uint64_t count) { return set_rgb_output_impl(h, rgb_dev, count); }

extern "C" int smx_set_guard(smx_handle h, uint8_t* guard_dev, uint64_t count, double margin) {
  return set_guard_impl(h, guard_dev, count, margin);
}

extern "C" int smx_check_social_history(const smx_config* cfg, const smx_map_tables* map, const smx_social_history* hist, char* err,
                                        uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && map && hist) ? check_social_history_impl(*cfg, *map, *hist, msg) : refuse(msg, "null config / map / history");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_social_history(smx_handle h, const smx_social_history* hist) { return set_social_history_impl(h, hist); }

extern "C" int smx_check_social_history_dims(const smx_config* cfg, const smx_social_history* hist, const smx_social_dims* dims,
                                             char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && hist && dims) ? check_social_history_dims_impl(*cfg, *hist, *dims, msg) : refuse(msg, "null config / history / dims");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_social_history_dims(smx_handle h, const smx_social_dims* dims) { return set_social_history_dims_impl(h, dims); }

extern "C" int smx_check_agent_dims(const smx_config* cfg, const smx_agent_dims* dims, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && dims) ? check_agent_dims_impl(*cfg, *dims, msg) : refuse(msg, "null config / dims");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_agent_dims(smx_handle h, const smx_agent_dims* dims) { return set_agent_dims_impl(h, dims); }

extern "C" int smx_check_agent_entry(const smx_config* cfg, const smx_agent_entry* entry, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && entry) ? check_agent_entry_impl(*cfg, *entry, msg) : refuse(msg, "null config / entry");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_agent_entry(smx_handle h, const smx_agent_entry* entry) { return set_agent_entry_impl(h, entry); }

extern "C" int smx_check_agent_spaces(const smx_config* cfg, const smx_agent_spaces* spaces, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && spaces) ? check_agent_spaces_impl(*cfg, *spaces, msg) : refuse(msg, "agent spaces: null config / table");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_agent_spaces(smx_handle h, const smx_agent_spaces* spaces) { return set_agent_spaces_impl(h, spaces); }

extern "C" int smx_check_history_agents(const smx_config* cfg, const smx_social_history* hist, const smx_history_agents* ha, char* err,
                                        uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && hist && ha) ? check_history_agents_impl(*cfg, hist->rows, *ha, msg) : refuse(msg, "null config / history / history agents");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_history_agents(smx_handle h, const smx_history_agents* ha) { return set_history_agents_impl(h, ha); }

extern "C" int smx_check_history_handover(const smx_config* cfg, const smx_social_history* hist, const smx_history_handover* ho, char* err,
                                          uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && hist && ho) ? check_history_handover_impl(*cfg, hist->rows, *ho, msg) : refuse(msg, "null config / history / history handover");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_history_handover(smx_handle h, const smx_history_handover* ho) { return set_history_handover_impl(h, ho); }

extern "C" int smx_check_history_bubbles(const smx_config* cfg, const smx_history_bubbles* hb, char* err, uint64_t err_len) {
  std::string msg;
  const int rc = (cfg && hb) ? check_history_bubbles_impl(*cfg, *hb, msg) : refuse(msg, "null config / history bubbles");
  return report(rc, msg, err, err_len);
}

extern "C" int smx_set_history_bubbles(smx_handle h, const smx_history_bubbles* hb) { return set_history_bubbles_impl(h, hb); }

extern "C" int smx_bind_frame_stack(smx_handle h, int32_t source, int32_t layout, void* stack_dev, uint64_t bytes) {
  return bind_frame_stack_impl(h, source, layout, stack_dev, bytes);
}

// the pass's last launches: every FRAMES binding in one k_frame_push, the interleaved image in one k_frame_dstack
static int launch_frame_stacks(smx_handle h, const bool is_step, const uint8_t* mask, const smx_state* st, const smx_outputs* out,
                               hipStream_t stream) {
  const smx_config& c = h->cfg;
  FrameStackArgs f{};
  f.k = c.frame_stack;
  f.total = (uint32_t)((size_t)c.num_envs * c.num_vehicles);
  f.n_veh = (uint32_t)c.num_vehicles;
  f.flags = st->flags;
  f.done = out->done;
  f.env_done = out->env_done;
  f.env_mask = is_step ? nullptr : mask;
  f.is_step = is_step ? 1 : 0;
  f.auto_reset = c.auto_reset ? 1 : 0;
  FrameStackArgs d = f;
  uint64_t blocks = 0, dstack_blocks = 0;
  for (const smx_handle_s::StackBinding& s : h->stacks) {
    const uint8_t* src = s.source == SMX_STACK_SOURCE_RGB ? h->rgb_out : (const uint8_t*)buffer_ptr(*out, s.source);
    if (!src || !s.row)
      return fail(h, SMX_ERR_STATE, "frame stack: source " + std::to_string(s.source) + " is bound but its row is NULL in this call");
    FrameStackBinding b{src, s.dst, s.row, 0, 0, 0};
    if (s.layout == SMX_STACK_DSTACK) {
      d.b[0] = b;
      d.n = 1;
      dstack_blocks = stack_dstack_blocks(s.row, f.total);
      continue;
    }
    const StackColumns at = stack_push_place(s.row, reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(s.dst), f.total, blocks);
    b.unit = at.unit;
    b.block0 = at.block0;
    f.b[f.n++] = b;
  }
  if (blocks >= STACK_BLOCKS_CAP || dstack_blocks >= STACK_BLOCKS_CAP) return fail(h, SMX_ERR_INVALID, "frame stack: the bound rows need more workgroups than a launch has");
  if (f.n) hipLaunchKernelGGL(k_frame_push, dim3((unsigned)blocks), dim3(SMX_STACK_BLOCK), 0, stream, f);
  if (d.n) {
    void (*const dstack[])(FrameStackArgs) = {k_frame_dstack<2>, k_frame_dstack<3>, k_frame_dstack<4>, k_frame_dstack<5>,
                                              k_frame_dstack<6>, k_frame_dstack<7>, k_frame_dstack<8>};
    hipLaunchKernelGGL(dstack[c.frame_stack - 2], dim3((unsigned)dstack_blocks), dim3(SMX_STACK_BLOCK), 0, stream, d);
  }
  return SMX_OK;
}

static int check_buffers(smx_handle h, const smx_state* st, const smx_spawns* sp, const smx_outputs* o) {
  std::string msg;
  const int rc = check_buffers_impl(h->cfg, h->n_vias > 0, st, sp, o, msg);
  if (rc != SMX_OK) return fail(h, rc, msg);
  if ((h->cfg.sensors & SMX_SENSOR_LIDAR) && !h->lidar_rays)
    return fail(h, SMX_ERR_STATE, "lidar sensor enabled but smx_set_lidar_rays has not been called");
  if ((h->cfg.sensors & SMX_SENSOR_RGB) && !h->rgb_out)
    return fail(h, SMX_ERR_STATE, "rgb sensor enabled but no image buffer is bound (smx_set_rgb_output)");
  for (const smx_handle_s::StackBinding& s : h->stacks)  // (an optional row the caller left NULL: nothing is launched)
    if (s.source != SMX_STACK_SOURCE_RGB && !buffer_ptr(*o, s.source))
      return fail(h, SMX_ERR_STATE, "frame stack: source " + std::to_string(s.source) + " is bound but its row is NULL in smx_outputs");
  return SMX_OK;
}

// enqueue() issues a call's TickPlan (smx_plan.h) step by step; the steps launch what the plan names and decide nothing.
using Kernel = void (*)(KernelArgs);
using HandoffKernel = void (*)(KernelArgs, CtrlHandoff);
// A kernel that reads a per-mission table has a pool instance (TickPlan::pool): the steps below name the kernel as they
// always have, and while a pool is bound — a.missions.rows, which is what PlanInputs::pool_bound was read from — its
// instance is launched in its place.  Kernels without such a site have none and are launched as they are.
static Kernel pool_instance(Kernel k) {
  static const struct { Kernel plain, pool; } twins[] = {
      {k_scan<true, true>, k_scan_pool<true>}, {k_scan<false, true>, k_scan_pool<false>},
      {k_scan_half<1, true>, k_scan_half_pool<false>}, {k_scan_half<1, true, SMX_TEAM_LARGE, true>, k_scan_half_pool<true>},
      {k_sensors, k_sensors_pool}, {k_sensors_sized, k_sensors_sized_pool}, {k_observe, k_observe_pool}, {k_observe_sized, k_observe_sized_pool},
      {k_waypoints, k_waypoints_pool}, {k_waypoints_tables, k_waypoints_tables_pool}, {k_waypoints_emit, k_waypoints_emit_pool},
      {k_waypoints_listed, k_waypoints_listed_pool}, {k_waypoints_walk_listed, k_waypoints_walk_listed_pool},
      {k_road_waypoints, k_road_waypoints_pool}};
  for (const auto& t : twins)
    if (t.plain == k) return t.pool;
  return k;
}
static void launch(Kernel k, unsigned blocks, size_t lds, hipStream_t s, const KernelArgs& a) {
  hipLaunchKernelGGL(a.missions.rows != nullptr ? pool_instance(k) : k, dim3(blocks), dim3(SMX_BLOCK), lds, s, a);
}
static void launch(HandoffKernel k, unsigned blocks, hipStream_t s, const KernelArgs& a, const CtrlHandoff& ho) {
  hipLaunchKernelGGL(k, dim3(blocks), dim3(SMX_BLOCK), 0, s, a, ho);
}
static KernelArgs with_slow(KernelArgs a, const SlowRef& slow) {
  a.slow_list = slow.list;
  a.slow_count = slow.count;
  return a;
}

// the controller kernels of one action space (the lane-following forms exist for the two lane spaces only)
struct ControlKernels {
  Kernel one, one_lds, fast;
  HandoffKernel listed, paths, law;
  Kernel kinematic;  // (the kinematic spaces have this one alone)
};
template <int SPACE, bool GUARD>
static ControlKernels control_kernels_of() {
  if constexpr (smx_kinematic_space(SPACE)) {
    return ControlKernels{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, k_control_kinematic<SPACE, GUARD>};
  } else {
    ControlKernels k{k_control<SPACE, false, GUARD>, nullptr, nullptr, nullptr, nullptr, k_control_law<SPACE, GUARD>, nullptr};
    if constexpr (SPACE == SMX_ACTION_SPACE_LANE || SPACE == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED) {
      k.one_lds = k_control<SPACE, true, GUARD>;
      k.fast = k_control_fast<SPACE, GUARD>;
      k.listed = k_control_listed<SPACE, GUARD>;
      k.paths = k_control_paths<SPACE, GUARD>;
    }
    return k;
  }
}
// (`guard`: TickPlan::guard — the instantiations with the state guard)
template <bool GUARD>
static ControlKernels control_kernels(int action_space) {
  switch (action_space) {
    case SMX_ACTION_SPACE_LANE: return control_kernels_of<SMX_ACTION_SPACE_LANE, GUARD>();
    case SMX_ACTION_SPACE_CONTINUOUS: return control_kernels_of<SMX_ACTION_SPACE_CONTINUOUS, GUARD>();
    case SMX_ACTION_SPACE_ACTUATOR_DYNAMIC: return control_kernels_of<SMX_ACTION_SPACE_ACTUATOR_DYNAMIC, GUARD>();
    case SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED: return control_kernels_of<SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED, GUARD>();
    case SMX_ACTION_SPACE_TRAJECTORY: return control_kernels_of<SMX_ACTION_SPACE_TRAJECTORY, GUARD>();
    case SMX_ACTION_SPACE_MPC: return control_kernels_of<SMX_ACTION_SPACE_MPC, GUARD>();
    case SMX_ACTION_SPACE_TARGET_POSE: return control_kernels_of<SMX_ACTION_SPACE_TARGET_POSE, GUARD>();
    case SMX_ACTION_SPACE_IMITATION: return control_kernels_of<SMX_ACTION_SPACE_IMITATION, GUARD>();
    default: return control_kernels_of<SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME, GUARD>();
  }
}

// the controller kernels of one action space in a mixed fleet (smx_step_mixed; the six spaces of the Ackermann chassis)
using SlotKernel = void (*)(KernelArgs, SlotList);
using MixedKernel = void (*)(KernelArgs, CtrlHandoff, const int32_t*);
struct MixedKernels {
  SlotKernel one;
  MixedKernel paths, law;  // (paths: the two lane spaces only)
};
template <int SPACE, bool GUARD>
static MixedKernels mixed_kernels_of() {
  MixedKernels k{k_control_slots<SPACE, GUARD>, nullptr, k_control_law_mixed<SPACE, GUARD>};
  if constexpr (SPACE == SMX_ACTION_SPACE_LANE || SPACE == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED)
    k.paths = k_control_paths_mixed<SPACE, GUARD>;
  return k;
}
template <bool GUARD>
static MixedKernels mixed_kernels(int action_space) {
  switch (action_space) {
    case SMX_ACTION_SPACE_LANE: return mixed_kernels_of<SMX_ACTION_SPACE_LANE, GUARD>();
    case SMX_ACTION_SPACE_CONTINUOUS: return mixed_kernels_of<SMX_ACTION_SPACE_CONTINUOUS, GUARD>();
    case SMX_ACTION_SPACE_ACTUATOR_DYNAMIC: return mixed_kernels_of<SMX_ACTION_SPACE_ACTUATOR_DYNAMIC, GUARD>();
    case SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED: return mixed_kernels_of<SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED, GUARD>();
    case SMX_ACTION_SPACE_TRAJECTORY: return mixed_kernels_of<SMX_ACTION_SPACE_TRAJECTORY, GUARD>();
    default: return mixed_kernels_of<SMX_ACTION_SPACE_MPC, GUARD>();
  }
}
// One launch, or pair of launches, per space present, all on the caller's stream; they touch disjoint vehicles, so their
// order is free (ascending space numbers here).
static void launch_control_mixed(smx_handle h, const TickPlan& p, const KernelArgs& a, hipStream_t stream) {
  const AgentSpacesDev& sd = h->spaces;
  for (int s = 0; s <= SMX_ACTION_SPACE_IMITATION; ++s) {
    if (!((p.mixed_spaces >> s) & 1u)) continue;
    const MixedKernels k = p.guard ? mixed_kernels<true>(s) : mixed_kernels<false>(s);
    switch (p.control_of[s]) {
      case Control::ONE: {
        const SlotList sl{sd.slots + (size_t)s * h->cfg.num_vehicles, sd.count[s]};
        const unsigned blocks = smx_blocks((size_t)h->cfg.num_envs * sd.count[s], SMX_BLOCK / SMX_WP_LANES);
        hipLaunchKernelGGL(k.one, dim3(blocks), dim3(SMX_BLOCK), 0, stream, a, sl);
        break;
      }
      case Control::PATHS_LAW:
        hipLaunchKernelGGL(k.paths, dim3(p.wp_blocks), dim3(SMX_BLOCK), 0, stream, a, h->ctrl, sd.space);
        hipLaunchKernelGGL(k.law, dim3(p.veh_blocks), dim3(SMX_BLOCK), 0, stream, a, h->ctrl, sd.space);
        break;
      case Control::LAW: hipLaunchKernelGGL(k.law, dim3(p.veh_blocks), dim3(SMX_BLOCK), 0, stream, a, h->ctrl, sd.space); break;
      default: break;
    }
  }
}

// what k_bubbles / k_bubbles_clear get of a call (only built with bubbles bound)
static BubbleArgs bubble_args(const smx_handle_s* h, const KernelArgs& a) {
  BubbleArgs g{};
  g.flags = a.st.flags;
  g.f64 = a.st.f64;
  g.env_ticks = a.st.env_ticks;
  g.env_episode = a.st.env_episode;
  g.history = h->history;
  g.state = h->bubble_state;
  g.cursor = h->bubble_cursor;
  g.total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  g.num_envs = h->cfg.num_envs;
  g.num_vehicles = h->cfg.num_vehicles;
  g.n_agents = h->cfg.num_vehicles - h->cfg.num_social;
  g.reset_elapsed_steps = h->cfg.reset_elapsed_steps;
  return g;
}

static void launch_control(smx_handle h, const TickPlan& p, const KernelArgs& a, hipStream_t stream) {
  const ControlKernels k = p.guard ? control_kernels<true>(h->cfg.action_space) : control_kernels<false>(h->cfg.action_space);
  switch (p.control) {
    case Control::NONE: break;
    case Control::MIXED: launch_control_mixed(h, p, a, stream); break;
    case Control::ONE: launch(k.one, p.wp_blocks, 0, stream, a); break;
    case Control::ONE_LDS: launch(k.one_lds, p.wp_blocks, 0, stream, a); break;
    case Control::LAW: launch(k.law, p.veh_blocks, stream, a, h->ctrl); break;
    case Control::PATHS_LAW:
      launch(k.paths, p.wp_blocks, stream, a, h->ctrl);
      launch(k.law, p.veh_blocks, stream, a, h->ctrl);
      break;
    case Control::FAST_LISTED: {
      const KernelArgs ac = with_slow(a, p.control_slow);  // the controller's slow list
      launch(k.fast, p.veh_blocks, 0, stream, ac);
      launch(k.listed, p.slow_blocks, stream, ac, h->ctrl);
      break;
    }
    case Control::KINEMATIC: launch(k.kinematic, p.veh_blocks, 0, stream, a); break;
    case Control::KINEMATIC_FOLLOW:  // (smx_set_history_agents holds the binding to Imitation)
      launch(p.guard ? k_control_kinematic<SMX_ACTION_SPACE_IMITATION, true, true> : k_control_kinematic<SMX_ACTION_SPACE_IMITATION, false, true>,
             p.veh_blocks, 0, stream, a);
      break;
    case Control::KINEMATIC_HANDOVER:  // (the binding again; smx_step_history_handover holds actions_f32 to non-null)
      launch(p.guard ? k_control_kinematic<SMX_ACTION_SPACE_IMITATION, true, false, true> : k_control_kinematic<SMX_ACTION_SPACE_IMITATION, false, false, true>,
             p.veh_blocks, 0, stream, a);
      break;
    case Control::KINEMATIC_BUBBLES:  // (the bubble pass, then the mixed tick that reads its state row; both on the caller's stream)
      hipLaunchKernelGGL(k_bubbles, dim3((unsigned)h->cfg.num_envs), dim3(64), 0, stream, bubble_args(h, a), h->bubbles);
      hipLaunchKernelGGL(p.guard ? k_control_kinematic_bubbles<true> : k_control_kinematic_bubbles<false>, dim3(p.veh_blocks), dim3(SMX_BLOCK), 0,
                         stream, a, (const uint8_t*)h->bubble_state);
      break;
  }
}

// the tick's alive list: the one the last pass's k_tail built from these flags (it zeroed this tick's slow-list
// counters too), or k_alive_list now
static void alive_list(smx_handle h, const TickPlan& p, KernelArgs& a, hipStream_t stream) {
  if (p.alive == AliveList::NONE) return;
  const AliveLayout al = alive_layout(h->cfg);
  int32_t* counters = h->alive_blob.get<int32_t>() + al.flat;
  a.alive_list = h->alive_blob.get<int32_t>();
  if (p.alive == AliveList::CARRIED) {
    a.alive_count = h->alive_blob.get<int32_t>() + al.seg + (size_t)8 * SMX_SEG_STRIDE * (h->seg_parity ^ 1);
    a.alive_segmented = 1;
  } else {
    const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
    a.alive_count = counters + h->alive_parity;
    hipLaunchKernelGGL(k_alive_list, dim3(smx_blocks(total, SMX_ALIVE_BLOCK)), dim3(SMX_ALIVE_BLOCK), 0, stream, a, h->alive_blob.get<int32_t>(),
                       counters + h->alive_parity, counters + (h->alive_parity ^ 1), p.alive_zero);
  }
  h->alive_parity ^= 1;
}

static void launch_grids(smx_handle h, const TickPlan& p, const KernelArgs& k, hipStream_t s) {
  const unsigned total = (unsigned)(h->cfg.num_envs * h->cfg.num_vehicles);
  switch (p.ogm) {
    case Ogm::NONE:
    case Ogm::IN_SENSORS: break;
    case Ogm::ENV2: hipLaunchKernelGGL((p.sized ? k_ogm_env<2, true> : k_ogm_env<2, false>), dim3((unsigned)h->cfg.num_envs), dim3(SMX_OGM_WAVES * 64), p.ogm_lds, s, k); break;
    case Ogm::ENV1: hipLaunchKernelGGL((p.sized ? k_ogm_env<1, true> : k_ogm_env<1, false>), dim3((unsigned)h->cfg.num_envs), dim3(SMX_OGM_WAVES * 64), p.ogm_lds, s, k); break;
    case Ogm::PER_OBSERVER: launch(k_ogm, total, p.ogm_lds, s, k); break;
  }
  if (p.dagm) launch(k_dagm, total, p.dagm_bytes, s, k);
  if (p.rgb) launch(k_rgb, total, p.rgb_lds, s, k);
}

// the slow seeds chain over the vehicles the one-lane seeds kernel left seed_pending: searches from scratch, then their
// walks and rows by the serial emitter
static void launch_slow_chain(const TickPlan& p, const KernelArgs& ks, hipStream_t s) {
  if (p.chain_fused) {
    launch(p.sized ? k_scan_listed<1, false, SMX_TEAM, true> : k_scan_listed<1, false, SMX_TEAM>, p.slow_blocks, 0, s, ks);
    launch(k_waypoints_walk_listed, p.slow_blocks, 0, s, ks);
  } else {
    launch(p.sized ? k_scan_listed<1, false, SMX_TEAM_LARGE, true> : k_scan_listed<1>, p.slow_blocks, 0, s, ks);
    launch(k_waypoints_listed, p.slow_blocks, 0, s, ks);
    launch(k_wp_walk_listed, p.slow_blocks, 0, s, ks);
  }
}

// one tick's observations: grid kernels, the scan's halves, the slow seeds chain, rows, observe, lidar, joins, road
// waypoints (`ph`: the call's phase events, null unless the plan is phased)
static void observation_pass(smx_handle h, const TickPlan& p, const KernelArgs& k, hipStream_t stream, hipEvent_t* ph) {
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  const hipStream_t s_grid = p.fork ? h->streams.side[0] : stream, s_obs = p.fork ? h->streams.side[1] : stream;
  if (p.fork) {
    (void)hipEventRecord(h->streams.ev_fork_grid, stream);
    (void)hipStreamWaitEvent(s_grid, h->streams.ev_fork_grid, 0);
    launch_grids(h, p, k, s_grid);
    if (p.lidar == Lidar::SIDE) launch(p.sized ? k_lidar<true> : k_lidar<false>, p.lidar_blocks, 0, s_grid, k);
  }
  // the scan's halves as two launches in the large form, on two streams when forked: path seeds (-> waypoint kernels) on
  // the caller's, road facts (-> observe) on side 1; each half appends to its own slow list
  KernelArgs ks = with_slow(k, p.seeds_slow);
  ks.seed_pending = p.seed_pending();
  switch (p.seeds()) {
    case Seeds::SCAN: {
      const Kernel scan = p.scan_split ? (p.routed ? k_scan<true, true> : k_scan<true>) : (p.routed ? k_scan<false, true> : k_scan<false>);
      launch(scan, p.seeds_blocks, 0, stream, k);
      break;
    }
    case Seeds::ONE_LANE: launch(k_scan_fast<1>, p.seeds_blocks, 0, stream, ks); break;
    case Seeds::ROUTED: launch(p.sized ? k_scan_half<1, true, SMX_TEAM_LARGE, true> : k_scan_half<1, true>, p.seeds_blocks, 0, stream, k); break;
    case Seeds::WIDE: launch(p.sized ? k_scan_half<1, false, SMX_TEAM, true> : k_scan_half<1, false, SMX_TEAM>, p.seeds_blocks, 0, stream, k); break;
    case Seeds::FOUR: launch(p.sized ? k_scan_half<1, false, SMX_TEAM_LARGE, true> : k_scan_half<1>, p.seeds_blocks, 0, stream, k); break;
  }
  if (p.chain() == SlowChain::SIDE) {
    // the slow chain runs beside the main chain (k_wp_walk -> k_waypoints_emit pass over its vehicles)
    // (one event after the seeds half serves this fork and the facts half's below: every record on the caller's
    // stream is a packet its next kernel waits behind, ten microseconds of the tick's longest chain)
    (void)hipEventRecord(h->streams.ev_fork, stream);
    (void)hipStreamWaitEvent(h->streams.side[2], h->streams.ev_fork, 0);
    launch_slow_chain(p, ks, h->streams.side[2]);
  }
  if (p.facts_start == FactsStart::WITH_GRIDS) {
    (void)hipStreamWaitEvent(s_obs, h->streams.ev_fork_grid, 0);
  } else if (p.facts_start == FactsStart::AFTER_SEEDS) {
    if (p.chain() != SlowChain::SIDE) (void)hipEventRecord(h->streams.ev_fork, stream);
    (void)hipStreamWaitEvent(s_obs, h->streams.ev_fork, 0);
  }
  const KernelArgs kf = with_slow(k, p.facts_slow);
  switch (p.facts) {
    case Facts::SCAN: break;
    case Facts::ONE_LANE:
      launch(k_scan_fast<0>, p.facts_blocks, 0, s_obs, kf);
      launch(p.sized ? k_scan_listed<0, false, SMX_TEAM_LARGE, true> : k_scan_listed<0>, p.slow_blocks, 0, s_obs, kf);
      break;
    case Facts::WIDE: launch(p.sized ? k_scan_half<0, false, SMX_TEAM, true> : k_scan_half<0, false, SMX_TEAM>, p.facts_blocks, 0, s_obs, kf); break;
    case Facts::FOUR: launch(p.sized ? k_scan_half<0, false, SMX_TEAM_LARGE, true> : k_scan_half<0>, p.facts_blocks, 0, s_obs, kf); break;  // (the facts half seeds no path)
  }
  if (ph) (void)hipEventRecord(ph[SMX_PHASE_SCAN + 1], stream);
  if (!p.fork) launch_grids(h, p, k, stream);
  if (ph) (void)hipEventRecord(ph[SMX_PHASE_OGM + 1], stream);
  KernelArgs kw = k;  // the waypoint kernels, which pass over the slow chain's vehicles
  kw.seed_pending = p.seed_pending();
  const unsigned walk_blocks = smx_blocks(total * SMX_WP_LANES);
  switch (p.rows) {
    case Rows::SENSORS: launch(p.sized ? k_sensors_sized : k_sensors, p.sensor_blocks, p.sensor_lds, stream, k); break;
    case Rows::UNSTAGED: launch(k_waypoints, p.wp_blocks, 0, stream, k); break;
    case Rows::TABLES:
      launch(k_wp_walk, walk_blocks, 0, stream, kw);
      launch(k_waypoints_tables, p.wp_blocks, std::max((size_t)h->cfg.wp_len * SMX_BLOCK * 16, (size_t)SMX_MAX_KNOTS * SMX_BLOCK * sizeof(int)),
             stream, k);
      break;
    case Rows::EMIT:
    case Rows::EMIT_CHAIN_SIDE:
    case Rows::EMIT_CHAIN_AFTER:
      if (!p.knot_table) launch(k_wp_walk, walk_blocks, 0, stream, kw);  // (the table: k_waypoints_emit reads the rows)
      kw = with_slow(kw, p.rows_slow);
      launch(k_waypoints_emit, p.wp_blocks, 0, stream, kw);
      launch(k_waypoints_listed, p.slow_blocks, 0, stream, kw);
      if (p.rows == Rows::EMIT_CHAIN_AFTER) launch_slow_chain(p, ks, stream);  // (one stream: after the main waypoint kernels)
      break;
  }
  if (!p.small()) launch(p.sized ? k_observe_sized : k_observe, p.obs_blocks, 0, s_obs, k);
  if (p.lidar == Lidar::CALLER) launch(p.sized ? k_lidar<true> : k_lidar<false>, p.lidar_blocks, 0, stream, k);
  if (p.fork) {
    // (each side stream joins the caller's directly: chaining side 0 through side 1 puts one more hop behind the
    // last kernel when k_observe ends the tick — 1 % late in a run)
    for (int i = 0; i < (p.chain() == SlowChain::SIDE ? 3 : 2); ++i) {
      (void)hipEventRecord(h->streams.ev_join[i], h->streams.side[i]);
      (void)hipStreamWaitEvent(stream, h->streams.ev_join[i], 0);
    }
  }
  if (p.road_waypoints)  // (poses are the tick's new ones; flags still those of its start)
    launch(k_road_waypoints, smx_blocks(total * SMX_RW_LANE_CAP), 0, stream, k);
  if (p.lane_ttc)  // (the waypoint, neighbour and ego rows are complete here in every form: the side streams have joined)
    hipLaunchKernelGGL(k_lane_ttc, dim3(p.ttc_blocks), dim3(SMX_BLOCK), p.ttc_lds, stream, k, (const int32_t*)nullptr, (const int32_t*)nullptr);
  if (p.ego_centric)  // (the same site: every world row it reads, the lidar's and the road waypoints' included, is complete)
    hipLaunchKernelGGL(k_ego_frame, dim3(p.ec_blocks), dim3(SMX_BLOCK), 0, stream, k, (const int32_t*)nullptr, (const int32_t*)nullptr);
  if (ph) (void)hipEventRecord(ph[SMX_PHASE_SENSORS + 1], stream);
}

// the end of the pass: k_tail (the tick's commit, the new vehicles' grid tiles, the env groups with new vehicles,
// the next tick's alive list), then the reset pass over those groups (first observations of the new vehicles)
static int tail_and_reset_pass(smx_handle h, const TickPlan& p, const KernelArgs& a, const uint8_t* mask, const smx_state* st,
                               hipStream_t stream, hipEvent_t* ph) {
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  const AliveLayout al = alive_layout(h->cfg);
  KernelArgs r = a;
  r.alive_list = nullptr;
  r.alive_count = nullptr;
  r.alive_segmented = 0;
  r.first_only = 1;
  r.keep_reward_done = p.is_step ? 1 : 0;
  r.reset_all = (!p.is_step && mask == nullptr) ? 1 : 0;
  r.env_mask = p.is_step ? nullptr : mask;
  if (!p.is_step) {
    if (p.entry)  // (the ENTRY instantiations: pending agents; the plain ones hold nothing of it)
      launch(p.guard ? (p.sized ? k_reset<true, true, true> : k_reset<true, false, true>)
                     : (p.sized ? k_reset<false, true, true> : k_reset<false, false, true>), p.veh_blocks, 0, stream, r);
    else
      launch(p.guard ? (p.sized ? k_reset<true, true> : k_reset<true>) : (p.sized ? k_reset<false, true> : k_reset<false>), p.veh_blocks, 0, stream, r);
    launch(k_reset_env, p.env_blocks, 0, stream, r);
  }
  TailArgs t{};
  t.commit = p.is_step ? 1 : 0;
  t.grids = p.tail_grids ? 1 : 0;
  t.groups = h->alive_blob.get<int32_t>() + al.groups;
  t.n_groups = h->alive_blob.get<int32_t>() + al.group_count + SMX_SEG_STRIDE * h->group_parity;
  t.n_groups_next = h->alive_blob.get<int32_t>() + al.group_count + SMX_SEG_STRIDE * (h->group_parity ^ 1);
  if (p.tail_builds_list) {  // (the next tick's parity is h->alive_parity now)
    t.list = h->alive_blob.get<int32_t>();
    t.seg_count = h->alive_blob.get<int32_t>() + al.seg + (size_t)8 * SMX_SEG_STRIDE * h->seg_parity;
    t.seg_next = h->alive_blob.get<int32_t>() + al.seg + (size_t)8 * SMX_SEG_STRIDE * (h->seg_parity ^ 1);
    t.flat_next = h->alive_blob.get<int32_t>() + al.flat + h->alive_parity;
    t.slow_next = SlowLists{h->slow_blob.get<int32_t>(), total}.counters(h->alive_parity);
  }
  hipLaunchKernelGGL(p.pool ? (p.guard ? k_tail_pool<true> : k_tail_pool<false>) : (p.guard ? k_tail<true> : k_tail<false>), dim3(p.obs_blocks), dim3(SMX_BLOCK), p.tail_grids ? std::max({p.ogm_bytes, p.dagm_bytes, p.rgb_lds}) : 0, stream, r, t);
  if (p.entry_first)  // (a large form's tick: this tick's entrants into the reset pass's groups, smx_k_entry.h)
    hipLaunchKernelGGL(k_entry_first, dim3(p.obs_blocks), dim3(SMX_BLOCK), 0, stream, r, t.groups, t.n_groups);
  if (ph) SMX_HIP(hipEventRecord(ph[SMX_PHASE_COMMIT + 1], stream));
  h->group_parity ^= 1;
  h->list_ready = p.tail_builds_list;
  if (p.tail_builds_list) {
    h->seg_parity ^= 1;
    h->list_state = *st;
  }
  if (p.reset_pass) {
    if (p.road_waypoints)  // before k_first clears SMX_F_FIRST
      launch(k_road_waypoints, smx_blocks(total * SMX_RW_LANE_CAP), 0, stream, r);
    if (p.lidar_first) {
      launch(p.sized ? k_lidar_first<true> : k_lidar_first<false>, (unsigned)std::min<size_t>(SMX_LIDAR_FIRST_BLOCKS, total), 0, stream, r);
      r.lidar_blocks = 0;
    }
    r.walk_new = p.first_walks_new ? 1 : 0;
    hipLaunchKernelGGL(p.pool ? (p.sized ? k_first_sized_pool : k_first_pool) : (p.sized ? k_first_sized : k_first), dim3(p.obs_blocks), dim3(SMX_FIRST_BLOCK), 0, stream, r, t.groups, t.n_groups);
    if (p.lane_ttc)  // after k_first: it reads the first observations' rows, not SMX_F_FIRST
      hipLaunchKernelGGL(k_lane_ttc, dim3(p.ttc_first_blocks), dim3(SMX_BLOCK), p.ttc_lds, stream, r, (const int32_t*)t.groups, (const int32_t*)t.n_groups);
    if (p.ego_centric)
      hipLaunchKernelGGL(k_ego_frame, dim3(p.ec_first_blocks), dim3(SMX_BLOCK), 0, stream, r, (const int32_t*)t.groups, (const int32_t*)t.n_groups);
  }
  return SMX_OK;
}

// the argument block every kernel of the call starts from
static KernelArgs kernel_args(smx_handle h, const TickPlan& p, const int8_t* actions, const float* actions_f32, const double* traj,
                              const int32_t* traj_n, int32_t traj_max, const uint8_t* mask, const smx_state* st, const smx_spawns* sp,
                              const smx_outputs* out) {
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  KernelArgs a;
  a.cfg = h->cfg;
  a.map = h->map;
  a.st = *st;
  a.sp = *sp;
  a.out = *out;
  a.actions = actions;
  a.actions_f32 = actions_f32;
  a.traj = traj;
  a.traj_n = traj_n;
  a.traj_max = traj_max;
  a.env_mask = mask;
  a.lidar_rays = h->lidar_rays;
  a.vias = h->n_vias > 0 ? h->vias_dev.get<smx_via>() : nullptr;
  a.missions = h->missions;
  a.via_slot_off = h->via_off_dev.get<int32_t>();
  a.first_only = 0;
  a.keep_reward_done = 0;
  a.reset_all = 0;
  a.heading_gain_pos = h->heading_gain_pos;
  a.nb_d2_max = h->nb_d2_max;
  a.walk_new = 0;
  a.wp_spill = h->spill_blob.get<char>();
  a.wp_pool_limit = h->wp_pool_limit;
  a.lateral_gain_pos = h->lateral_gain_pos;
  a.debug_skip = h->debug_skip;
  a.knots = h->knots;
  a.knot_table = p.knot_table ? h->knot_table.get<KnotRow>() : nullptr;
  a.knot_served = (p.knot_table && h->knot_table_mode == 2) ? (unsigned long long*)(h->knot_stats.get<int32_t>() + 2) : nullptr;
  a.status = h->status_dev.get<int32_t>();
  a.alive_list = nullptr;
  a.alive_count = nullptr;
  a.alive_segmented = 0;
  a.slow_list = nullptr;
  a.slow_count = nullptr;
  a.seed_pending = nullptr;
  a.seeds_carry = h->scan_carry.get<double>();
  a.facts_carry = h->scan_carry ? h->scan_carry.get<double>() + 4 * total : nullptr;
  a.dagm_reach = h->dagm_reach;
  a.rgb = h->rgb_out;
  a.guard = h->guard_out;
  a.guard_box = h->guard_box;
  a.history = h->history;
  a.dims = h->dims;
  a.ha_action = h->ha_action;
  a.ha_status = h->ha_status;
  a.ogm_mask = (p.ogm_delta && out->ogm) ? h->ogm_mask.get<unsigned long long>() : nullptr;
  a.entry = h->entry;
  a.wp_blocks = (int)p.wp_blocks;
  a.obs_blocks = (int)p.obs_blocks;
  a.lidar_blocks = (int)p.lidar_blocks;
  return a;
}

// which entry point a call came through (each hands over its own pointers and leaves the others null)
enum class Entry { RESET, LANE, FLOATS, TRAJECTORY, TARGET_POSE, TRAJECTORY_WITH_TIME, HISTORY_AGENTS, HISTORY_HANDOVER, MIXED };
static const char* entry_name(Entry e) {
  static const char* const names[] = {"smx_reset", "smx_step", "smx_step_continuous", "smx_step_trajectory", "smx_step_target_pose",
                                      "smx_step_trajectory_with_time", "smx_step_history_agents", "smx_step_history_handover", "smx_step_mixed"};
  return names[(int)e];
}
// (traj_max: columns per row of a TrajectoryWithTime action)
static int enqueue(smx_handle h, const Entry entry, const int8_t* actions, const float* actions_f32, const double* traj,
                   const int32_t* traj_n, int32_t traj_max, const uint8_t* mask, const smx_state* st,
                   const smx_spawns* sp, const smx_outputs* out, void* stream_) {
  if (!h) return SMX_ERR_INVALID;
  if (!h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_load_map has not been called");
  int rc = check_buffers(h, st, sp, out);
  if (rc != SMX_OK) return rc;
  const bool is_step = entry != Entry::RESET;
  const bool follow = entry == Entry::HISTORY_AGENTS, handover = entry == Entry::HISTORY_HANDOVER, mixed = entry == Entry::MIXED;
  if (is_step) {  // (smx_step_mixed with a table bound, the others without one; its buffers: smx_handle.h check_step_entry)
    const smx_mixed_actions acts{actions, actions_f32, traj, traj_n};
    rc = check_step_entry(h, entry_name(entry), mixed ? &acts : nullptr, mixed);
    if (rc != SMX_OK) return rc;
  }
  if (follow) {  // (the binding holds cfg.action_space to Imitation; the tick reads no action)
    if (h->history.follow == nullptr) return fail(h, SMX_ERR_STATE, "smx_step_history_agents: no history agents are bound (smx_set_history_agents)");
  } else if (handover) {  // (the binding holds cfg.action_space to Imitation; the driven agents' rows are read)
    if (h->history.follow == nullptr || (h->history.handover == nullptr && h->bubble_state == nullptr))
      return fail(h, SMX_ERR_STATE, "smx_step_history_handover: no handover table is bound (smx_set_history_handover)");
    if (actions_f32 == nullptr) return fail(h, SMX_ERR_INVALID, "smx_step_history_handover: actions_dev is NULL");
  } else if (is_step && !mixed) {  // (smx_step_mixed's buffers were checked against the table above)
    const int sp_ = h->cfg.action_space;
    const bool ok = sp_ == SMX_ACTION_SPACE_LANE ? (entry == Entry::LANE && actions != nullptr)
                    : (sp_ == SMX_ACTION_SPACE_TRAJECTORY || sp_ == SMX_ACTION_SPACE_MPC)
                        ? (entry == Entry::TRAJECTORY && traj != nullptr && traj_n != nullptr)
                    : sp_ == SMX_ACTION_SPACE_TARGET_POSE ? (entry == Entry::TARGET_POSE && traj != nullptr)
                    : sp_ == SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME
                        ? (entry == Entry::TRAJECTORY_WITH_TIME && traj != nullptr && traj_n != nullptr)
                        : (entry == Entry::FLOATS && actions_f32 != nullptr);
    if (!ok)
      return fail(h, SMX_ERR_INVALID,
                  "actions do not match cfg.action_space (smx_step: Lane, smx_step_trajectory: Trajectory and MPC, "
                  "smx_step_continuous: the float spaces and Imitation, smx_step_target_pose: TargetPose, "
                  "smx_step_trajectory_with_time: TrajectoryWithTime)");
  }
  hipStream_t stream = (hipStream_t)stream_;
  const TickPlan p = tick_plan(plan_inputs(h, is_step, st, follow, handover, mixed));
  if (is_step && h->entry_reset_needed)
    return fail(h, SMX_ERR_STATE, "agent entry: smx_set_agent_entry bound or unbound a table since the last smx_reset of every "
                                  "env (env_mask NULL); step after one");
  if (!is_step && mask == nullptr) h->entry_reset_needed = false;
  KernelArgs a = kernel_args(h, p, actions, actions_f32, traj, traj_n, traj_max, mask, st, sp, out);
  const bool timed = h->timing && is_step && h->ev_used < 65536;
  if (timed) {
    if (h->ev_pool.ev.size() < 2 * (h->ev_used + 1)) {
      hipEvent_t e0, e1;
      SMX_HIP(hipEventCreate(&e0));
      SMX_HIP(hipEventCreate(&e1));
      h->ev_pool.ev.push_back(e0);
      h->ev_pool.ev.push_back(e1);
    }
    SMX_HIP(hipEventRecord(h->ev_pool.ev[2 * h->ev_used], stream));
  }
  // phase timing (smx_set_timing level 2): one boundary event after every kernel of the tick
  hipEvent_t* ph = nullptr;
  if (p.phased) {
    const size_t need = (h->ph_used + 1) * (SMX_PHASE_COUNT + 1);
    while (h->ph_pool.ev.size() < need) {
      hipEvent_t e;
      SMX_HIP(hipEventCreate(&e));
      h->ph_pool.ev.push_back(e);
    }
    ph = &h->ph_pool.ev[h->ph_used * (SMX_PHASE_COUNT + 1)];
    SMX_HIP(hipEventRecord(ph[0], stream));
  }
  if (a.ogm_mask && !(h->ogm_known && h->ogm_rows == out->ogm)) {
    // the masks do not describe these rows (KernelArgs::ogm_mask): every piece may be non-zero, this pass stores whole tiles
    SMX_HIP(hipMemsetAsync(h->ogm_mask.get<unsigned long long>(), 0xff, h->ogm_mask_bytes, stream));
    h->ogm_rows = out->ogm;
    h->ogm_known = true;
  }
  if (!a.ogm_mask) h->ogm_known = false;  // a pass that stores without the masks leaves them stale
  if (p.social) launch(k_social, p.veh_blocks, 0, stream, a);
  alive_list(h, p, a, stream);
  if (is_step) {
    launch_control(h, p, a, stream);
    if (p.entry)  // (after the control phase has moved the social slots, ahead of every sensor: smx_k_entry.h)
      hipLaunchKernelGGL(p.small() ? (p.guard ? k_entry<true, false> : k_entry<false, false>)
                                   : (p.guard ? k_entry<true, true> : k_entry<false, true>),
                         dim3((unsigned)h->cfg.num_envs), dim3(64), 0, stream, a);
    if (ph) SMX_HIP(hipEventRecord(ph[SMX_PHASE_CONTROL + 1], stream));
    observation_pass(h, p, a, stream, ph);
  }
  rc = tail_and_reset_pass(h, p, a, mask, st, stream, ph);
  if (rc != SMX_OK) return rc;
  // bubbles: an env that this pass has reset (smx_reset, or auto_reset inside a mixed tick) starts from zero bytes
  if (h->bubble_state != nullptr && (!is_step || (handover && p.reset_pass)))
    hipLaunchKernelGGL(k_bubbles_clear, dim3(p.veh_blocks), dim3(SMX_BLOCK), 0, stream, bubble_args(h, a));
  if (p.frame_stack) {  // (after the reset pass: a restarted env's rows hold its first observation)
    rc = launch_frame_stacks(h, is_step, mask, st, out, stream);
    if (rc != SMX_OK) return rc;
  }
  SMX_HIP(hipGetLastError());
  if (ph) {
    SMX_HIP(hipEventRecord(ph[SMX_PHASE_RESET + 1], stream));
    h->ph_used += 1;
  }
  if (timed) {
    SMX_HIP(hipEventRecord(h->ev_pool.ev[2 * h->ev_used + 1], stream));
    h->ev_used += 1;
  }
  return SMX_OK;
}

extern "C" int smx_reset(smx_handle h, const uint8_t* env_mask_dev, const smx_state* st, const smx_spawns* sp,
                         const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::RESET, nullptr, nullptr, nullptr, nullptr, 0, env_mask_dev, st, sp, out, hip_stream);
}

extern "C" int smx_step(smx_handle h, const int8_t* actions_dev, const smx_state* st, const smx_spawns* sp,
                        const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::LANE, actions_dev, nullptr, nullptr, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_continuous(smx_handle h, const float* actions_dev, const smx_state* st, const smx_spawns* sp,
                                   const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::FLOATS, nullptr, actions_dev, nullptr, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_history_agents(smx_handle h, const smx_state* st, const smx_spawns* sp, const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::HISTORY_AGENTS, nullptr, nullptr, nullptr, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_history_handover(smx_handle h, const float* actions_dev, const smx_state* st, const smx_spawns* sp,
                                         const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::HISTORY_HANDOVER, nullptr, actions_dev, nullptr, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_trajectory(smx_handle h, const double* trajectories_dev, const int32_t* counts_dev,
                                   const smx_state* st, const smx_spawns* sp, const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::TRAJECTORY, nullptr, nullptr, trajectories_dev, counts_dev, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_target_pose(smx_handle h, const double* targets_dev, const smx_state* st, const smx_spawns* sp,
                                    const smx_outputs* out, void* hip_stream) {
  return enqueue(h, Entry::TARGET_POSE, nullptr, nullptr, targets_dev, nullptr, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_trajectory_with_time(smx_handle h, const double* trajectories_dev, const int32_t* counts_dev,
                                             int32_t max_points, const smx_state* st, const smx_spawns* sp,
                                             const smx_outputs* out, void* hip_stream) {
  if (h && max_points < 2) return fail(h, SMX_ERR_INVALID, "smx_step_trajectory_with_time: max_points < 2");
  return enqueue(h, Entry::TRAJECTORY_WITH_TIME, nullptr, nullptr, trajectories_dev, counts_dev, max_points, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_step_mixed(smx_handle h, const smx_mixed_actions* acts, const smx_state* st, const smx_spawns* sp,
                              const smx_outputs* out, void* hip_stream) {
  if (!h) return SMX_ERR_INVALID;
  if (!acts) return check_step_entry(h, "smx_step_mixed", nullptr, true);  // (no table: SMX_ERR_STATE; else the null argument)
  return enqueue(h, Entry::MIXED, acts->lane_dev, acts->floats_dev, acts->trajectories_dev, acts->counts_dev, 0, nullptr, st, sp, out, hip_stream);
}

extern "C" int smx_actions_to_world(smx_handle h, int32_t action_space, const double* in_dev, const int32_t* counts_dev,
                                    int32_t max_points, double* out_dev, const smx_outputs* out, void* hip_stream) {
  if (!h) return SMX_ERR_INVALID;
  const smx_config& c = h->cfg;
  if (h->spaces.space != nullptr)
    return fail(h, SMX_ERR_STATE, "smx_actions_to_world: per-agent action spaces are bound (smx_set_agent_spaces); ego-frame actions of a "
                                  "mixed fleet are not built");
  if (!(c.sensors & SMX_SENSOR_EGO_CENTRIC))
    return fail(h, SMX_ERR_STATE, "smx_actions_to_world: the configuration has no SMX_SENSOR_EGO_CENTRIC (no frame is kept)");
  const bool traj = action_space == SMX_ACTION_SPACE_TRAJECTORY || action_space == SMX_ACTION_SPACE_MPC;
  const bool pose = action_space == SMX_ACTION_SPACE_TARGET_POSE;
  const bool timed = action_space == SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME;
  if (!traj && !pose && !timed)
    return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: only Trajectory, MPC, TargetPose and TrajectoryWithTime actions have a frame");
  if (action_space != c.action_space) return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: action_space is not cfg.action_space");
  if (!in_dev || !out_dev || in_dev == out_dev || (!pose && !counts_dev))
    return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: null action buffer or counts, or the output is the input");
  if (timed && max_points < 2) return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: max_points < 2");
  const uint64_t total = (uint64_t)c.num_envs * c.num_vehicles;
  if (!out || !out->ego_frame || !out->ec_flags || out->dtype[SMX_OUT_EGO_FRAME] != SMX_DT_F64 ||
      out->dtype[SMX_OUT_EC_FLAGS] != SMX_DT_U8 || out->count[SMX_OUT_EGO_FRAME] < 4 * total || out->count[SMX_OUT_EC_FLAGS] < total)
    return fail(h, SMX_ERR_INVALID, "smx_actions_to_world: out.ego_frame / out.ec_flags missing, short or mistyped");
  const int cols = traj ? SMX_TRAJ_COLS : pose ? 1 : max_points;
  const unsigned blocks = smx_blocks((size_t)total * cols);
  hipStream_t s = (hipStream_t)hip_stream;
#define SMX_A2W(SPACE)                                                                                                  \
  hipLaunchKernelGGL(k_actions_to_world<SPACE>, dim3(blocks), dim3(SMX_BLOCK), 0, s, in_dev, counts_dev, out_dev,        \
                     (const double*)out->ego_frame, (const uint8_t*)out->ec_flags, (size_t)total, (int)c.num_vehicles, \
                     (int)c.num_social, cols)
  if (traj) SMX_A2W(SMX_ACTION_SPACE_TRAJECTORY);
  else if (pose) SMX_A2W(SMX_ACTION_SPACE_TARGET_POSE);
  else SMX_A2W(SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME);
#undef SMX_A2W
  SMX_HIP(hipGetLastError());
  return SMX_OK;
}

extern "C" int smx_sync(smx_handle h, void* hip_stream) {
  if (!h) return SMX_ERR_INVALID;
  SMX_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
  if (h->status_dev) {  // what the kernels could not report themselves
    int32_t bits = 0;
    SMX_HIP(hipMemcpy(&bits, h->status_dev.get<int32_t>(), sizeof(bits), hipMemcpyDeviceToHost));
    if (bits) {
      SMX_HIP(hipMemset(h->status_dev.get<int32_t>(), 0, sizeof(int32_t)));
      if (bits & SMX_DEVICE_BAD_LANE_ACTION)
        return fail(h, SMX_ERR_INVALID,
                    "a Lane action code outside -1..3 reached smx_step since the last smx_sync; the agents that sent one "
                    "were stepped as if they had sent no action");
      if (bits & SMX_DEVICE_BAD_TRAJECTORY)
        return fail(h, SMX_ERR_INVALID,
                    "an illegal TrajectoryWithTime action reached smx_step_trajectory_with_time since the last smx_sync (fewer "
                    "than two points or more than max_points, a value that is not finite, times not strictly increasing, no "
                    "point later than dt or the first one already later); the agents that sent one were not moved");
      if (bits & SMX_DEVICE_BAD_TARGET_POSE)
        return fail(h, SMX_ERR_INVALID,
                    "a TargetPose action whose pose is not finite reached smx_step_target_pose, or an Imitation action "
                    "with an infinite component or a pose or speed that is not finite reached smx_step_continuous, since the "
                    "last smx_sync; the agents that sent one were stepped as if they had sent no action");
      if (bits & SMX_DEVICE_BAD_MISSION_ROW)
        return fail(h, SMX_ERR_INVALID,
                    "an entry outside -1 .. n_missions - 1 was read from the table of the mission pool (smx_set_mission_pool) "
                    "since the last smx_sync; the agents it stood for had an endless mission, as for -1");
    }
  }
  return SMX_OK;
}

// Developer diagnostics (not part of include/smx.h): the lengths of the last large-form tick's slow lists
// (scan facts, scan seeds, control, waypoint rows), after a synchronisation of the device.
extern "C" int smx_debug_slow_counts(smx_handle h, int32_t* out4) {
  if (!h || !out4) return SMX_ERR_INVALID;
  if (!h->slow_blob) return fail(h, SMX_ERR_STATE, "no slow lists (the map is not loaded)");
  SMX_HIP(hipDeviceSynchronize());
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  SMX_HIP(hipMemcpy(out4, SlowLists{h->slow_blob.get<int32_t>(), total}.counters(h->alive_parity ^ 1), 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SMX_OK;
}

// developer / tests: use only `records` of k_waypoints_emit's LDS knot pool (0 < records <= SMX_WPE_POOL), so that
// small batches reach its overflow area too (a full pool needs sixteen vehicles in a bend in one workgroup)
extern "C" int smx_debug_set_wp_pool(smx_handle h, int32_t records) {
  if (!h) return SMX_ERR_INVALID;
  if (records < 1 || records > SMX_WPE_POOL) return fail(h, SMX_ERR_INVALID, "smx_debug_set_wp_pool: 1 .. SMX_WPE_POOL records");
  h->wp_pool_limit = records;
  return SMX_OK;
}

// developer / tests: the one-lane cut's knot lists from the map's knot table (1, the default), from the walks of
// k_wp_walk as before the table (0), or from the table with a count of the path lanes it serves (2)
extern "C" int smx_debug_set_knot_table(smx_handle h, int32_t mode) {
  if (!h) return SMX_ERR_INVALID;
  if (mode < 0 || mode > 2) return fail(h, SMX_ERR_INVALID, "smx_debug_set_knot_table: 0 (walked lists), 1 (table), 2 (table, counting)");
  h->knot_table_mode = mode;
  return SMX_OK;
}

// the loaded map's knot table after a synchronisation of the device: rows in all, rows tabled, tabled rows that stay on
// their start road, path lanes served from a row while the switch above was 2
extern "C" int smx_debug_knot_table_stats(smx_handle h, int64_t* out4) {
  if (!h || !out4) return SMX_ERR_INVALID;
  if (!h->knot_table) return fail(h, SMX_ERR_STATE, "no knot table (no map loaded, or no waypoints sensor)");
  SMX_HIP(hipDeviceSynchronize());
  int32_t st[4];
  SMX_HIP(hipMemcpy(st, h->knot_stats.get<int32_t>(), sizeof(st), hipMemcpyDeviceToHost));
  unsigned long long served;
  std::memcpy(&served, st + 2, sizeof(served));
  out4[0] = h->map.n_lanepoints;
  out4[1] = st[0];
  out4[2] = st[1];
  out4[3] = (int64_t)served;
  return SMX_OK;
}

// The caller wrote into the OGM rows itself: the next call stores whole tiles (the masks describe what the library stored).
extern "C" int smx_invalidate_outputs(smx_handle h) {
  if (!h) return SMX_ERR_INVALID;
  h->ogm_known = false;
  return SMX_OK;
}

// OGM delta stores on (the default) or off: off passes the kernels the null mask and every call stores every piece.
extern "C" int smx_set_ogm_delta(smx_handle h, int on) {
  if (!h) return SMX_ERR_INVALID;
  h->ogm_delta = on != 0;
  h->ogm_known = false;
  return SMX_OK;
}

extern "C" int smx_set_timing(smx_handle h, int level) {
  if (!h) return SMX_ERR_INVALID;
  h->timing = level == 1;
  h->phase_timing = level == 2;
  return SMX_OK;
}

extern "C" int smx_read_phase_ms(smx_handle h, float* ms, int32_t max_steps, int32_t* n) {
  if (!h || !ms || !n || max_steps < 0) return SMX_ERR_INVALID;
  int32_t count = 0;
  for (size_t i = 0; i < h->ph_used; ++i) {
    hipEvent_t* ph = &h->ph_pool.ev[i * (SMX_PHASE_COUNT + 1)];
    SMX_HIP(hipEventSynchronize(ph[SMX_PHASE_COUNT]));
    if (count >= max_steps) continue;
    for (int p = 0; p < SMX_PHASE_COUNT; ++p) {
      float t = 0.f;
      SMX_HIP(hipEventElapsedTime(&t, ph[p], ph[p + 1]));
      ms[(size_t)count * SMX_PHASE_COUNT + p] = t;
    }
    ++count;
  }
  h->ph_used = 0;
  *n = count;
  return SMX_OK;
}

extern "C" int smx_read_step_ms(smx_handle h, float* ms, int32_t max, int32_t* n) {
  if (!h || !ms || !n || max < 0) return SMX_ERR_INVALID;
  int32_t count = 0;
  for (size_t i = 0; i < h->ev_used; ++i) {
    SMX_HIP(hipEventSynchronize(h->ev_pool.ev[2 * i + 1]));
    float t = 0.f;
    SMX_HIP(hipEventElapsedTime(&t, h->ev_pool.ev[2 * i], h->ev_pool.ev[2 * i + 1]));
    if (count < max) ms[count++] = t;
  }
  h->ev_used = 0;
  *n = count;
  return SMX_OK;
}

extern "C" int smx_last_step_ms(smx_handle h, float* ms) {
  if (!h || !ms) return SMX_ERR_INVALID;
  if (h->ev_used == 0) return fail(h, SMX_ERR_STATE, "no timed step recorded (smx_set_timing(1) then smx_step)");
  const size_t i = h->ev_used - 1;
  SMX_HIP(hipEventSynchronize(h->ev_pool.ev[2 * i + 1]));
  SMX_HIP(hipEventElapsedTime(ms, h->ev_pool.ev[2 * i], h->ev_pool.ev[2 * i + 1]));
  return SMX_OK;
}

extern "C" const char* smx_last_error(smx_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" void smx_destroy(smx_handle h) { destroy_impl(h); }

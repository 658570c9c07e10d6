// The tick's launch plan (smarts_amd/csrc/smx_plan.h) with and without SMX_SENSOR_EGO_CENTRIC, host-compiled and driven
// by tests/test_env_ego_centric.py: the configuration is built the way tests/native/host_plan.cpp builds its own, and
// every launch decision is returned beside the new flag and its grid sizes.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

// in: as host_plan.cpp (num_envs, num_vehicles, strategy, junctions, routed, sensors, wp_paths, ogm_width, ogm_height,
// timing level, is_step, blobs, side_ready, list_carried, social IDM, action_space).  Returns the number of values.
int host_plan_ego(const int* in, long long* out) {
  static int32_t slow[64];
  static uint8_t pending[1];
  smx_config c{};
  c.num_envs = in[0];
  c.num_vehicles = in[1];
  c.sensors = (uint32_t)in[5];
  c.wp_paths = in[6];
  c.wp_len = 1;
  c.ogm_width = in[7];
  c.ogm_height = in[8];
  c.num_social = in[14] ? 1 : 0;
  c.social_model = in[14] ? SMX_SOCIAL_IDM : SMX_SOCIAL_CONSTANT;
  c.action_space = in[15];
  c.auto_reset = 1;
  PlanInputs pi{};
  pi.cfg = &c;
  pi.launch_strategy = in[2];
  pi.map_junctions = in[3] != 0;
  pi.slow_blocks = 512;
  pi.routed = in[4] != 0;
  pi.phase_timing = in[9] == 2;
  pi.is_step = in[10] != 0;
  pi.alive_blob = (in[11] & 1) != 0;
  pi.slow = SlowLists{(in[11] & 2) ? slow : nullptr, 0};
  pi.pending_blob = (in[11] & 4) ? pending : nullptr;
  pi.knots_blob = (in[11] & 8) != 0;
  pi.ctrl_blob = (in[11] & 16) != 0;
  pi.side_ready = in[12] != 0;
  pi.list_carried = in[13] != 0;
  const TickPlan p = tick_plan(pi);
  int n = 0;
  // ---- every launch decision the parent's plan holds
  out[n++] = p.form;
  out[n++] = (int)p.seeds();
  out[n++] = (int)p.facts;
  out[n++] = (int)p.facts_start;
  out[n++] = (int)p.rows;
  out[n++] = (int)p.chain();
  out[n++] = (int)p.ogm;
  out[n++] = (int)p.lidar;
  out[n++] = (int)p.control;
  out[n++] = (int)p.alive;
  out[n++] = p.fork;
  out[n++] = p.social;
  out[n++] = p.tail_builds_list;
  out[n++] = p.tail_grids;
  out[n++] = p.seed_pending() != nullptr;
  out[n++] = p.phased;
  out[n++] = p.scan_split;
  out[n++] = p.chain_fused;
  out[n++] = p.dagm;
  out[n++] = p.road_waypoints;
  out[n++] = p.lane_ttc;
  out[n++] = p.ttc_blocks;
  out[n++] = p.ttc_first_blocks;
  out[n++] = (long long)p.ttc_lds;
  out[n++] = p.reset_pass;
  out[n++] = p.lidar_first;
  out[n++] = p.first_walks_new;
  out[n++] = p.veh_blocks;
  out[n++] = p.wp_blocks;
  out[n++] = p.obs_blocks;
  out[n++] = p.env_blocks;
  out[n++] = p.lidar_blocks;
  out[n++] = p.seeds_blocks;
  out[n++] = p.facts_blocks;
  out[n++] = p.slow_blocks;
  out[n++] = p.sensor_blocks;
  out[n++] = (long long)p.ogm_lds;
  out[n++] = (long long)p.sensor_lds;
  // ---- the new flag and its grids (the last three values)
  out[n++] = p.ego_centric;
  out[n++] = p.ec_blocks;
  out[n++] = p.ec_first_blocks;
  return n;
}
}

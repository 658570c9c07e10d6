// The tick's launch plan (smarts_amd/csrc/smx_plan.h) with and without frame stacking, host-compiled and driven by
// tests/test_host_plan_frame_stack.py: the configuration is built the way tests/native/host_plan_rgb.cpp builds its own,
// every value that one reports is returned in its order, and the new flag follows.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

// in[0..18]: as host_plan_rgb.cpp; in[19] = smx_config.frame_stack, in[20] = something is bound.  Returns the number
// of values.
int host_plan_frame_stack(const int* in, long long* out) {
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
  c.auto_reset = in[16];
  c.rgb_width = in[17];
  c.rgb_height = in[18];
  c.frame_stack = in[19];
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
  pi.frame_stack_bound = in[20] != 0;
  const TickPlan p = tick_plan(pi);
  int n = 0;
  // ---- what host_plan_rgb reports, in its order
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
  out[n++] = p.tail_grids;  // index 13 (HOST_PLAN_TAIL_GRIDS in the test)
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
  out[n++] = p.reset_pass;  // index 24 (HOST_PLAN_RESET_PASS)
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
  out[n++] = p.ego_centric;
  out[n++] = p.ec_blocks;
  out[n++] = p.ec_first_blocks;
  out[n++] = p.rgb;
  out[n++] = (long long)p.rgb_lds;
  // ---- the new flag (the last value)
  out[n++] = p.frame_stack;
  return n;
}
}

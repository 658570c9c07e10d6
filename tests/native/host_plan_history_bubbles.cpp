// What the tick's launch plan (smarts_amd/csrc/smx_plan.h) does with bound bubbles (smx_set_history_bubbles), behind one C
// entry point for tests/test_host_history_bubbles.py.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

// in: num_envs, num_vehicles, strategy (SMX_LAUNCH_*), map has junctions, the entry (0: smx_step_continuous, 1:
// smx_step_history_agents, 2: smx_step_history_handover), is_step, auto_reset, the guard is bound, action space (a history
// is bound throughout, OGM on), bubbles are bound.  Returns TickPlan::control as an integer; *same receives 1 when every
// other field of the plan that a launch reads equals the plan's of the same call through smx_step_continuous without bubbles.
int host_plan_history_bubbles(const int* in, int* same) {
  static int32_t slow[64];  // (never dereferenced; total 0 keeps every list and counter inside it)
  static uint8_t pending[1];
  smx_config c{};
  c.num_envs = in[0];
  c.num_vehicles = in[1];
  c.num_social = 2;
  c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_NEIGHBORS | SMX_SENSOR_OGM;
  c.ogm_width = c.ogm_height = 64;
  c.wp_paths = 4;
  c.wp_len = 20;
  c.wp_lookahead = 32;
  c.auto_reset = in[6];
  c.action_space = in[8];
  PlanInputs pi{};
  pi.cfg = &c;
  pi.launch_strategy = in[2];
  pi.map_junctions = in[3] != 0;
  pi.slow_blocks = 512;
  pi.is_step = in[5] != 0;
  pi.guard_bound = in[7] != 0;
  pi.alive_blob = pi.knots_blob = pi.ctrl_blob = pi.side_ready = true;
  pi.slow = SlowLists{slow, 0};
  pi.pending_blob = pending;
  pi.history_bound = true;
  const TickPlan without = tick_plan(pi);
  pi.follow_entry = in[4] == 1;
  pi.handover_entry = in[4] == 2;
  pi.bubbles_bound = in[9] != 0;
  const TickPlan p = tick_plan(pi);
  *same = p.form == without.form && p.is_step == without.is_step && p.phased == without.phased && p.routed == without.routed &&
          p.rows == without.rows && p.facts == without.facts && p.team_seeds == without.team_seeds && p.chain_fused == without.chain_fused &&
          p.alive == without.alive && p.alive_zero == without.alive_zero && p.fork == without.fork && p.scan_split == without.scan_split &&
          p.social == without.social && p.reset_pass == without.reset_pass && p.lidar_first == without.lidar_first &&
          p.knot_table == without.knot_table && p.first_walks_new == without.first_walks_new && p.veh_blocks == without.veh_blocks &&
          p.wp_blocks == without.wp_blocks && p.obs_blocks == without.obs_blocks && p.env_blocks == without.env_blocks &&
          p.lidar_blocks == without.lidar_blocks && p.slow_blocks == without.slow_blocks && p.guard == without.guard &&
          p.sized == without.sized && p.ogm == without.ogm && p.ogm_delta == without.ogm_delta && p.ogm_bytes == without.ogm_bytes &&
          p.ogm_lds == without.ogm_lds && p.lidar == without.lidar && p.dagm == without.dagm && p.rgb == without.rgb &&
          p.sensor_blocks == without.sensor_blocks && p.sensor_lds == without.sensor_lds && p.tail_builds_list == without.tail_builds_list &&
          p.tail_grids == without.tail_grids && p.facts_start == without.facts_start && p.seeds_blocks == without.seeds_blocks &&
          p.facts_blocks == without.facts_blocks && p.frame_stack == without.frame_stack && p.lane_ttc == without.lane_ttc &&
          p.ego_centric == without.ego_centric && p.road_waypoints == without.road_waypoints && p.pending == without.pending &&
          p.control_slow.list == without.control_slow.list && p.control_slow.count == without.control_slow.count &&
          p.facts_slow.list == without.facts_slow.list && p.seeds_slow.list == without.seeds_slow.list && p.rows_slow.list == without.rows_slow.list;
  return (int)p.control;
}
}

// What the tick's launch plan (smarts_amd/csrc/smx_plan.h) does with bound per-vehicle dimensions
// (smx_set_social_history_dims), behind one C entry point for tests/test_host_history_dims.py.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

// in: num_envs, num_vehicles, strategy (SMX_LAUNCH_*), map has junctions, dimensions bound, is_step, auto_reset (a history
// is bound throughout, OGM and lidar on).  Returns TickPlan::sized; *same receives 1 when every other field of the plan that a
// launch reads equals the plan's without the dimensions.
int host_plan_dims(const int* in, int* same) {
  static int32_t slow[64];  // (never dereferenced; total 0 keeps every list and counter inside it)
  static uint8_t pending[1];
  smx_config c{};
  c.num_envs = in[0];
  c.num_vehicles = in[1];
  c.num_social = 2;
  c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_NEIGHBORS | SMX_SENSOR_OGM | SMX_SENSOR_LIDAR;
  c.ogm_width = c.ogm_height = 64;
  c.wp_paths = 4;
  c.wp_len = 20;
  c.wp_lookahead = 32;
  c.auto_reset = in[6];
  c.action_space = SMX_ACTION_SPACE_LANE;
  PlanInputs pi{};
  pi.cfg = &c;
  pi.launch_strategy = in[2];
  pi.map_junctions = in[3] != 0;
  pi.slow_blocks = 512;
  pi.is_step = in[5] != 0;
  pi.alive_blob = pi.knots_blob = pi.ctrl_blob = pi.side_ready = true;
  pi.slow = SlowLists{slow, 0};
  pi.pending_blob = pending;
  pi.history_bound = true;
  TickPlan without = tick_plan(pi);
  pi.dims_bound = in[4] != 0;
  TickPlan p = tick_plan(pi);
  const int sized = p.sized ? 1 : 0;
  *same = without.sized ? 0 : 1;
  p.sized = without.sized = false;
  *same = *same && p.form == without.form && p.control == without.control && p.rows == without.rows && p.facts == without.facts &&
          p.team_seeds == without.team_seeds && p.alive == without.alive && p.fork == without.fork && p.social == without.social &&
          p.reset_pass == without.reset_pass && p.knot_table == without.knot_table && p.first_walks_new == without.first_walks_new &&
          p.veh_blocks == without.veh_blocks && p.obs_blocks == without.obs_blocks && p.guard == without.guard && p.ogm == without.ogm &&
          p.lidar == without.lidar && p.lidar_first == without.lidar_first && p.ogm_lds == without.ogm_lds &&
          p.lidar_blocks == without.lidar_blocks && p.sensor_blocks == without.sensor_blocks && p.sensor_lds == without.sensor_lds &&
          p.tail_builds_list == without.tail_builds_list && p.tail_grids == without.tail_grids && p.facts_start == without.facts_start;
  return sized;
}
}

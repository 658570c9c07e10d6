// What the tick's launch plan (smarts_amd/csrc/smx_plan.h) does with the entry smx_step_history_agents, behind one C
// entry point for tests/test_host_history_agents.py.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

// in: num_envs, num_vehicles, strategy (SMX_LAUNCH_*), map has junctions, the call is smx_step_history_agents, is_step,
// auto_reset, the guard is bound, action space (a history is bound throughout, OGM on).  Returns TickPlan::control as an
// integer; *same receives 1 when every other field of the plan that a launch reads equals the plan's of the same call
// through another entry.
int host_plan_history_agents(const int* in, int* same) {
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
  TickPlan without = tick_plan(pi);
  pi.follow_entry = in[4] != 0;
  TickPlan p = tick_plan(pi);
  const int control = (int)p.control;
  *same = (pi.follow_entry && pi.is_step && smx_kinematic_space(c.action_space)) ? (without.control == Control::KINEMATIC && p.control == Control::KINEMATIC_FOLLOW)
                                                                                   : p.control == without.control;
  *same = *same && p.form == without.form && p.rows == without.rows && p.facts == without.facts && p.team_seeds == without.team_seeds &&
          p.alive == without.alive && p.fork == without.fork && p.social == without.social && p.reset_pass == without.reset_pass &&
          p.knot_table == without.knot_table && p.first_walks_new == without.first_walks_new && p.veh_blocks == without.veh_blocks &&
          p.obs_blocks == without.obs_blocks && p.guard == without.guard && p.sized == without.sized && p.ogm == without.ogm &&
          p.ogm_lds == without.ogm_lds && p.lidar == without.lidar && p.sensor_blocks == without.sensor_blocks && p.sensor_lds == without.sensor_lds &&
          p.tail_builds_list == without.tail_builds_list && p.tail_grids == without.tail_grids && p.facts_start == without.facts_start &&
          p.seeds_blocks == without.seeds_blocks && p.facts_blocks == without.facts_blocks && p.frame_stack == without.frame_stack &&
          p.control_slow.list == without.control_slow.list;
  return control;
}
}

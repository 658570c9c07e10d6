// What the tick's launch plan (smarts_amd/csrc/smx_plan.h) does with a bound traffic history, behind one C entry point
// for tests/test_host_plan_history.py.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

// in: num_envs, num_vehicles, strategy (SMX_LAUNCH_*), map has junctions, history bound, is_step, auto_reset,
// the last pass's list is carried.  Returns bit 0: tail_builds_list, bit 1: the tick's alive list is BUILD (k_alive_list),
// bit 2: it is CARRIED, bit 3: the form is small; *same receives 1 when every other field of the plan that a launch
// reads equals the plan's without the history.
int host_plan_history(const int* in, int* same) {
  static int32_t slow[64];  // (never dereferenced; total 0 keeps every list and counter inside it)
  static uint8_t pending[1];
  smx_config c{};
  c.num_envs = in[0];
  c.num_vehicles = in[1];
  c.num_social = 2;
  c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_NEIGHBORS;
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
  pi.list_carried = in[7] != 0;
  pi.alive_blob = pi.knots_blob = pi.ctrl_blob = pi.side_ready = true;
  pi.slow = SlowLists{slow, 0};
  pi.pending_blob = pending;
  TickPlan without = tick_plan(pi);
  pi.history_bound = in[4] != 0;
  TickPlan p = tick_plan(pi);
  const int bits = (p.tail_builds_list ? 1 : 0) | (p.alive == AliveList::BUILD ? 2 : 0) | (p.alive == AliveList::CARRIED ? 4 : 0) |
                   (p.small() ? 8 : 0);
  without.tail_builds_list = p.tail_builds_list = false;
  *same = p.form == without.form && p.control == without.control && p.rows == without.rows && p.facts == without.facts &&
          p.team_seeds == without.team_seeds && p.alive == without.alive && p.fork == without.fork && p.social == without.social &&
          p.reset_pass == without.reset_pass && p.knot_table == without.knot_table && p.first_walks_new == without.first_walks_new &&
          p.veh_blocks == without.veh_blocks && p.obs_blocks == without.obs_blocks && p.guard == without.guard;
  return bits;
}
}

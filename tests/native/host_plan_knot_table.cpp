// What the tick's launch plan (smarts_amd/csrc/smx_plan.h) does with the map's knot table, behind one C entry point for
// tests/test_host_plan_knot_table.py.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

// in: num_envs, num_vehicles, strategy (SMX_LAUNCH_*), map has junctions, routed, table built and on, is_step,
// auto_reset, wp_lookahead.  Returns bit 0: form is the one-lane cut, bit 1: knot_table, bit 2: first_walks_new,
// bit 3: the rows are the emit form (k_waypoints_emit), bit 4: control is FAST_LISTED.
int host_plan_knot_table(const int* in) {
  static int32_t slow[64];  // (never dereferenced; total 0 keeps every list and counter inside it)
  static uint8_t pending[1];
  smx_config c{};
  c.num_envs = in[0];
  c.num_vehicles = in[1];
  c.sensors = SMX_SENSOR_WAYPOINTS;
  c.wp_paths = 4;
  c.wp_len = 20;
  c.wp_lookahead = in[8];
  c.auto_reset = in[7];
  c.action_space = SMX_ACTION_SPACE_LANE;
  PlanInputs pi{};
  pi.cfg = &c;
  pi.launch_strategy = in[2];
  pi.map_junctions = in[3] != 0;
  pi.routed = in[4] != 0;
  pi.knot_table = in[5] != 0;
  pi.slow_blocks = 512;
  pi.is_step = in[6] != 0;
  pi.alive_blob = pi.knots_blob = pi.ctrl_blob = pi.side_ready = true;
  pi.slow = SlowLists{slow, 0};
  pi.pending_blob = pending;
  const TickPlan p = tick_plan(pi);
  const bool emit = p.rows == Rows::EMIT || p.rows == Rows::EMIT_CHAIN_SIDE || p.rows == Rows::EMIT_CHAIN_AFTER;
  return (p.form == SMX_FORM_LARGE_ONE_LANE ? 1 : 0) | (p.knot_table ? 2 : 0) | (p.first_walks_new ? 4 : 0) | (emit ? 8 : 0) |
         (p.control == Control::FAST_LISTED ? 16 : 0);
}
}

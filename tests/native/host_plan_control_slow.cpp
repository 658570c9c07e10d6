// Whether the tick's launch plan (smarts_amd/csrc/smx_plan.h) hands the controller a slow list, behind one C entry point
// for tests/test_kinematic_cpu.py.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

// in: num_envs, num_vehicles, strategy (SMX_LAUNCH_*), map has junctions, action_space; a step with every blob present.
// Returns bit 0: form is the one-lane cut, bit 1: control_slow.list set, bit 2: control_slow.count set,
// bit 3: the seeds / rows slow lists set.
int host_plan_control_slow(const int* in) {
  static int32_t slow[64];  // (never dereferenced; total 0 keeps every list and counter inside it)
  static uint8_t pending[1];
  smx_config c{};
  c.num_envs = in[0];
  c.num_vehicles = in[1];
  c.sensors = SMX_SENSOR_WAYPOINTS;
  c.wp_paths = 4;
  c.wp_len = 1;
  c.action_space = in[4];
  PlanInputs pi{};
  pi.cfg = &c;
  pi.launch_strategy = in[2];
  pi.map_junctions = in[3] != 0;
  pi.slow_blocks = 512;
  pi.is_step = true;
  pi.alive_blob = pi.knots_blob = pi.ctrl_blob = pi.side_ready = true;
  pi.slow = SlowLists{slow, 0};
  pi.pending_blob = pending;
  const TickPlan p = tick_plan(pi);
  return (p.form == SMX_FORM_LARGE_ONE_LANE ? 1 : 0) | (p.control_slow.list ? 2 : 0) | (p.control_slow.count ? 4 : 0) |
         (p.seeds_slow.list && p.rows_slow.list ? 8 : 0);
}
}

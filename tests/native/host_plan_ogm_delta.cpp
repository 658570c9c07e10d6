// What the tick's launch plan (smarts_amd/csrc/smx_plan.h) decides about the OGM tiles' piece mask, behind one C entry
// point for tests/test_host_ogm_delta.py.  Test infrastructure only.
#include "smx_plan.h"

extern "C" {

int host_ogm_piece(void) { return SMX_OGM_PIECE; }

// in: ogm_width, ogm_height, num_envs, num_vehicles, strategy (SMX_LAUNCH_*), is_step, the handle holds a mask and the
// delta is on.  Returns TickPlan::ogm_delta; *words receives the mask words per agent tile, *same 1 when every other
// field of the plan that a launch reads equals the plan's without the mask.
int host_plan_ogm_delta(const int* in, unsigned long long* words, int* same) {
  static int32_t slow[64];  // (never dereferenced; total 0 keeps every list and counter inside it)
  static uint8_t pending[1];
  smx_config c{};
  c.ogm_width = in[0];
  c.ogm_height = in[1];
  c.num_envs = in[2];
  c.num_vehicles = in[3];
  c.sensors = SMX_SENSOR_WAYPOINTS | SMX_SENSOR_NEIGHBORS | SMX_SENSOR_OGM;
  c.wp_paths = 4;
  c.wp_len = 20;
  c.wp_lookahead = 32;
  c.auto_reset = 1;
  c.action_space = SMX_ACTION_SPACE_LANE;
  PlanInputs pi{};
  pi.cfg = &c;
  pi.launch_strategy = in[4];
  pi.slow_blocks = 512;
  pi.is_step = in[5] != 0;
  pi.alive_blob = pi.knots_blob = pi.ctrl_blob = pi.side_ready = true;
  pi.slow = SlowLists{slow, 0};
  pi.pending_blob = pending;
  TickPlan without = tick_plan(pi);
  pi.ogm_mask = in[6] != 0;
  TickPlan p = tick_plan(pi);
  *words = (unsigned long long)smx_ogm_mask_words((size_t)c.ogm_width * c.ogm_height);
  *same = !without.ogm_delta && p.form == without.form && p.control == without.control && p.rows == without.rows &&
          p.facts == without.facts && p.team_seeds == without.team_seeds && p.alive == without.alive && p.fork == without.fork &&
          p.reset_pass == without.reset_pass && p.ogm == without.ogm && p.ogm_lds == without.ogm_lds && p.ogm_bytes == without.ogm_bytes &&
          p.sensor_blocks == without.sensor_blocks && p.sensor_lds == without.sensor_lds && p.tail_grids == without.tail_grids &&
          p.tail_builds_list == without.tail_builds_list && p.facts_start == without.facts_start && p.obs_blocks == without.obs_blocks;
  return p.ogm_delta ? 1 : 0;
}
}

// What the launch plan (smarts_amd/csrc/smx_plan.h) does with a bound entry table (smx_set_agent_entry), as a stand-alone
// program for tests/test_host_agent_entry.py: over the three launch forms, reset calls and ticks, with and without
// auto_reset, the guard, dimensions, OGM, lidar and IDM traffic, TickPlan::entry is exactly entry_bound; without a table
// entry and entry_first are false; with one, a large form's tick has entry_first and the reset pass (every field the
// plan of the same tick under auto_reset has), and every other plan is the plan without the table, field for field —
// everything enqueue() reads to issue launches.
// Prints one JSON line and returns 0 when every check held.
#include <cstdio>
#include <string>

#include "smx_plan.h"

static int failures = 0, checks = 0;
static void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok && ++failures <= 20) std::printf("FAILED: %s\n", what.c_str());
}

// every field of TickPlan but `entry` and `entry_first`
#define PLAN_FIELDS(X)                                                                                                          \
  X(form) X(is_step) X(phased) X(routed) X(social) X(alive) X(alive_zero) X(control) X(control_slow.list) X(control_slow.count) \
  X(fork) X(scan_split) X(team_seeds) X(facts) X(facts_start) X(rows) X(chain_fused) X(facts_slow.list) X(facts_slow.count)    \
  X(seeds_slow.list) X(seeds_slow.count) X(rows_slow.list) X(rows_slow.count) X(ogm) X(ogm_delta) X(lidar) X(dagm)             \
  X(road_waypoints) X(rgb) X(rgb_lds) X(lane_ttc) X(ttc_blocks) X(ttc_first_blocks) X(ttc_lds) X(ego_centric) X(ec_blocks)     \
  X(ec_first_blocks) X(frame_stack) X(guard) X(sized) X(tail_builds_list) X(tail_grids) X(reset_pass) X(lidar_first)          \
  X(first_walks_new) X(knot_table) X(veh_blocks) X(wp_blocks) X(obs_blocks) X(env_blocks) X(lidar_blocks) X(seeds_blocks)     \
  X(facts_blocks) X(slow_blocks) X(sensor_blocks) X(ogm_bytes) X(dagm_bytes) X(ogm_lds) X(sensor_lds) X(pending)

int main() {
  static int32_t slow[4 * 65536 + 8];
  static uint8_t pending[1];
  int plans = 0, forms[3] = {0, 0, 0};
  for (int envs : {2, 512, 2048})
    for (int strategy : {SMX_LAUNCH_AUTO, SMX_LAUNCH_SMALL, SMX_LAUNCH_LARGE_ONE_LANE, SMX_LAUNCH_LARGE_TEAMS})
      for (int junctions : {0, 1})
        for (int is_step : {0, 1})
          for (int auto_reset : {0, 1})
            for (int guard : {0, 1})
              for (int sized : {0, 1})
                for (int sensors : {0, SMX_SENSOR_WAYPOINTS | SMX_SENSOR_NEIGHBORS | SMX_SENSOR_OGM | SMX_SENSOR_LIDAR})
                  for (int idm : {0, 1}) {
                    smx_config c{};
                    c.num_envs = envs, c.num_vehicles = 32, c.num_social = 8, c.dt = 0.1;
                    c.sensors = (uint32_t)sensors;
                    c.ogm_width = c.ogm_height = 64;
                    c.wp_paths = 4, c.wp_len = 20, c.wp_lookahead = 32, c.nb_max = 10;
                    c.auto_reset = auto_reset;
                    c.social_model = idm ? SMX_SOCIAL_IDM : SMX_SOCIAL_CONSTANT;
                    c.action_space = SMX_ACTION_SPACE_LANE;
                    PlanInputs pi{};
                    pi.cfg = &c;
                    pi.launch_strategy = strategy;
                    pi.map_junctions = junctions != 0;
                    pi.slow_blocks = 512;
                    pi.is_step = is_step != 0;
                    pi.alive_blob = pi.knots_blob = pi.ctrl_blob = pi.side_ready = pi.knot_table = true;
                    pi.slow = SlowLists{slow, (size_t)envs * 32};
                    pi.pending_blob = pending;
                    pi.guard_bound = guard != 0;
                    pi.agent_dims_bound = sized != 0;
                    const TickPlan without = tick_plan(pi);
                    // what the table may move: a large form's tick runs the reset pass, as under auto_reset
                    const bool large_tick = is_step && without.form != SMX_FORM_SMALL;
                    c.auto_reset = auto_reset || large_tick;
                    const TickPlan want = tick_plan(pi);
                    c.auto_reset = auto_reset;
                    pi.entry_bound = true;
                    const TickPlan with = tick_plan(pi);
                    const std::string at = "envs " + std::to_string(envs) + " strategy " + std::to_string(strategy) + " junctions " +
                                           std::to_string(junctions) + " step " + std::to_string(is_step) + " auto_reset " +
                                           std::to_string(auto_reset) + " guard " + std::to_string(guard) + " sized " + std::to_string(sized) +
                                           " sensors " + std::to_string(sensors) + " idm " + std::to_string(idm);
                    expect(!without.entry && !without.entry_first, "no table: no entry launch, " + at);
                    expect(with.entry, "a table: the entry launch (k_entry in a tick, the ENTRY k_reset in a reset), " + at);
                    expect(with.entry_first == large_tick, "k_entry_first in a large form's tick only, " + at);
                    expect(!large_tick || with.reset_pass, "a large form's tick with a table runs the reset pass, " + at);
#define SAME(f) expect(with.f == want.f, "field " #f " is the plan's without the table (large tick: under auto_reset), " + at);
                    PLAN_FIELDS(SAME)
#undef SAME
                    ++plans;
                    ++forms[with.form];
                  }
  expect(forms[SMX_FORM_SMALL] > 0 && forms[SMX_FORM_LARGE_TEAMS] > 0 && forms[SMX_FORM_LARGE_ONE_LANE] > 0, "all three forms were planned");
  if (failures) return 1;
  std::printf("{\"checks\": %d, \"plans\": %d, \"small\": %d, \"large_teams\": %d, \"large_one_lane\": %d}\n", checks, plans,
              forms[SMX_FORM_SMALL], forms[SMX_FORM_LARGE_TEAMS], forms[SMX_FORM_LARGE_ONE_LANE]);
  return 0;
}

// What the launch plan (smarts_amd/csrc/smx_plan.h) does with a bound table of agent spaces (smx_set_agent_spaces), as a
// stand-alone program for tests/test_host_agent_spaces.py, over the input sweep of host_plan_entry.cpp (the three launch
// forms, reset calls and ticks, auto_reset, the guard, dimensions, sensors, IDM traffic) times a few tables:
//   - with a table the form is never the one-lane cut, in a reset call or a tick;
//   - a tick through smx_step_mixed has Control::MIXED and, per space present, that space's form — ONE in the small form,
//     PATHS_LAW for the two lane spaces and LAW for the other four in the large one — and NONE for every other space;
//   - every other field is the plan of the same inputs without a table under the teams cut (a large form: the strategy
//     SMX_LAUNCH_LARGE_TEAMS; the small form: the same strategy) — everything enqueue() reads to issue launches;
//   - a table whose single space is cfg.action_space gives that uniform plan whole, its control form named for the space;
//   - without a table nothing of this is set.
// Prints one JSON line and returns 0 when every check held.
#include <cstdio>
#include <string>

#include "smx_plan.h"

static int failures = 0, checks = 0;
static void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok && ++failures <= 20) std::printf("FAILED: %s\n", what.c_str());
}

// every field of TickPlan but `control`, `mixed_spaces` and `control_of`
#define PLAN_FIELDS(X)                                                                                                          \
  X(form) X(is_step) X(phased) X(routed) X(social) X(alive) X(alive_zero) X(control_slow.list) X(control_slow.count)           \
  X(fork) X(scan_split) X(team_seeds) X(facts) X(facts_start) X(rows) X(chain_fused) X(facts_slow.list) X(facts_slow.count)    \
  X(seeds_slow.list) X(seeds_slow.count) X(rows_slow.list) X(rows_slow.count) X(ogm) X(ogm_delta) X(lidar) X(dagm)             \
  X(road_waypoints) X(rgb) X(rgb_lds) X(lane_ttc) X(ttc_blocks) X(ttc_first_blocks) X(ttc_lds) X(ego_centric) X(ec_blocks)     \
  X(ec_first_blocks) X(frame_stack) X(guard) X(sized) X(entry) X(entry_first) X(tail_builds_list) X(tail_grids) X(reset_pass)  \
  X(lidar_first) X(first_walks_new) X(knot_table) X(veh_blocks) X(wp_blocks) X(obs_blocks) X(env_blocks) X(lidar_blocks)       \
  X(seeds_blocks) X(facts_blocks) X(slow_blocks) X(sensor_blocks) X(ogm_bytes) X(dagm_bytes) X(ogm_lds) X(sensor_lds) X(pending)

static constexpr unsigned bit(int s) { return 1u << s; }

int main() {
  static int32_t slow[4 * 65536 + 8];
  static uint8_t pending[1];
  const unsigned all_six = bit(SMX_ACTION_SPACE_LANE) | bit(SMX_ACTION_SPACE_CONTINUOUS) | bit(SMX_ACTION_SPACE_ACTUATOR_DYNAMIC) |
                           bit(SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED) | bit(SMX_ACTION_SPACE_TRAJECTORY) | bit(SMX_ACTION_SPACE_MPC);
  const unsigned tables[] = {all_six, bit(SMX_ACTION_SPACE_LANE) | bit(SMX_ACTION_SPACE_CONTINUOUS), bit(SMX_ACTION_SPACE_TRAJECTORY) | bit(SMX_ACTION_SPACE_MPC),
                             bit(SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED), bit(SMX_ACTION_SPACE_LANE)};
  int plans = 0, forms[3] = {0, 0, 0}, uniform = 0;
  for (int envs : {2, 512, 2048})
    for (int strategy : {SMX_LAUNCH_AUTO, SMX_LAUNCH_SMALL, SMX_LAUNCH_LARGE_ONE_LANE, SMX_LAUNCH_LARGE_TEAMS})
      for (int junctions : {0, 1})
        for (int is_step : {0, 1})
          for (int auto_reset : {0, 1})
            for (int guard : {0, 1})
              for (int sized : {0, 1})
                for (int sensors : {0, SMX_SENSOR_WAYPOINTS | SMX_SENSOR_NEIGHBORS | SMX_SENSOR_OGM | SMX_SENSOR_LIDAR})
                  for (int idm : {0, 1})
                    for (unsigned table : tables) {
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
                      // the plan to agree with: no table, and a large form under the teams cut
                      if (without.form != SMX_FORM_SMALL) pi.launch_strategy = SMX_LAUNCH_LARGE_TEAMS;
                      const TickPlan want = tick_plan(pi);
                      pi.launch_strategy = strategy;
                      pi.agent_spaces = table;
                      pi.mixed_entry = is_step != 0;
                      const TickPlan with = tick_plan(pi);
                      const std::string at = "envs " + std::to_string(envs) + " strategy " + std::to_string(strategy) + " junctions " +
                                             std::to_string(junctions) + " step " + std::to_string(is_step) + " auto_reset " +
                                             std::to_string(auto_reset) + " guard " + std::to_string(guard) + " sized " + std::to_string(sized) +
                                             " sensors " + std::to_string(sensors) + " idm " + std::to_string(idm) + " table " + std::to_string(table);
                      expect(without.mixed_spaces == 0 && without.control != Control::MIXED, "no table: nothing mixed, " + at);
                      for (int s = 0; s <= SMX_ACTION_SPACE_IMITATION; ++s)
                        expect(without.control_of[s] == Control::NONE, "no table: no per-space form, " + at);
                      expect(with.form != SMX_FORM_LARGE_ONE_LANE, "a table: never the one-lane cut, " + at);
                      expect((with.form == SMX_FORM_SMALL) == (without.form == SMX_FORM_SMALL), "a table moves no batch between small and large, " + at);
                      expect(want.form == with.form, "the form of the plan to agree with, " + at);
#define SAME(f) expect(with.f == want.f, "field " #f " is the plan's without the table under the teams cut, " + at);
                      PLAN_FIELDS(SAME)
#undef SAME
                      const bool single = table == bit(c.action_space);
                      if (!is_step) {
                        expect(with.control == Control::NONE && with.mixed_spaces == 0, "a reset call has no control phase, " + at);
                      } else if (single) {
                        ++uniform;
                        expect(with.control == want.control && with.control != Control::MIXED && with.control != Control::FAST_LISTED,
                               "a table of cfg.action_space alone: the uniform plan's control form, " + at);
                        expect(with.mixed_spaces == table && with.control_of[c.action_space] == want.control, "... named for the space, " + at);
                      } else {
                        expect(with.control == Control::MIXED && with.mixed_spaces == table, "the mixed tick, " + at);
                      }
                      if (is_step && !single)
                        for (int s = 0; s <= SMX_ACTION_SPACE_IMITATION; ++s) {
                          const bool lanes = s == SMX_ACTION_SPACE_LANE || s == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED;
                          const Control form = !((table >> s) & 1u)          ? Control::NONE
                                               : with.form == SMX_FORM_SMALL ? Control::ONE
                                               : lanes                       ? Control::PATHS_LAW
                                                                             : Control::LAW;
                          expect(with.control_of[s] == form, "space " + std::to_string(s) + " has its control form, " + at);
                        }
                      // a uniform call while a table is bound is refused before it is planned; were it planned, it would not be mixed
                      pi.mixed_entry = false;
                      const TickPlan other = tick_plan(pi);
                      expect(other.control != Control::MIXED && other.mixed_spaces == 0 && other.form == with.form, "not the mixed entry: not the mixed tick, " + at);
                      ++plans;
                      ++forms[with.form];
                    }
  expect(forms[SMX_FORM_SMALL] > 0 && forms[SMX_FORM_LARGE_TEAMS] > 0 && forms[SMX_FORM_LARGE_ONE_LANE] == 0, "the small form and the teams cut were planned");
  if (failures) return 1;
  std::printf("{\"checks\": %d, \"plans\": %d, \"small\": %d, \"large_teams\": %d, \"large_one_lane\": %d, \"uniform\": %d}\n", checks, plans,
              forms[SMX_FORM_SMALL], forms[SMX_FORM_LARGE_TEAMS], forms[SMX_FORM_LARGE_ONE_LANE], uniform);
  return 0;
}

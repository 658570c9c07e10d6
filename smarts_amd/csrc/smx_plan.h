// smx_plan.h — what one smx_reset / smx_step* call launches, decided once (tick_plan) from the configuration, the
// launch strategy, the map's facts and what the handle holds; enqueue() in smx_kernels.hip issues the plan and
// smx_launch_form reports its form.  Host code only (no HIP): tests/test_host_plan.py builds it with a host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/smx.h"

#define SMX_BLOCK 64
#define SMX_WP_LANES 4  // lanes of a wavefront that share one vehicle (k_control, waypoints role)
#ifndef SMX_TEAM
#define SMX_TEAM 8  // lanes per vehicle on small batches (one wavefront's latency); large batches: SMX_TEAM_LARGE
#endif
#ifndef SMX_TEAM_LARGE
#define SMX_TEAM_LARGE 4  // fewer lanes repeat the per-vehicle uniform work (cell ranges, merges) at 131 k vehicles
#endif
#define SMX_WPT_MAX_PATHS 8  // dense rows per vehicle (wp_paths) the staged form handles
#define SMX_OGM_WAVES 4
// OGM delta stores: the bytes of a tile's piece the handle keeps one "may be non-zero in device memory" bit for (16: one
// lane's int4 of the copy-out; 64: a whole sector, four lanes').  profiles/r19_ogm_delta.txt has both measured: at 16 a
// tile of the headline workload stores 377 B that reach memory as 753 (partial sectors), at 64 1 120 B as 1 120, and the
// tick is the same or 1 % shorter at 64, with a quarter of the mask.
#ifndef SMX_OGM_PIECE
#define SMX_OGM_PIECE 64
#endif
static_assert(SMX_OGM_PIECE == 16 || SMX_OGM_PIECE == 64, "a piece is one int4 or one 64-byte sector");
// 64-bit mask words per agent tile ([E*N][words], a tile's last word padded)
static constexpr size_t smx_ogm_mask_words(size_t tile_bytes) { return (tile_bytes / SMX_OGM_PIECE + 63) / 64; }
#define SMX_TTC_TEAM 16  // lanes of a wavefront that share one agent in k_lane_ttc
// ... and in k_ego_frame: a team's access to a float64 row is one 128-byte line; the shortest rows (ten neighbours: 30
// float64, one path of 20 waypoints: 60) still fill it, and four agents' rows share a wavefront
#define SMX_EC_TEAM 16
// SMX_LAUNCH_AUTO: the LARGE launch form above this many vehicles.  Measured crossover (round 2, C4's shape:
// 8 192 vehicles 0.165 / 0.216 ms small / large, 32 768: 0.461 / 0.303, 65 536: 0.886 / 0.505; C3 at 32 768:
// 0.514 / 0.504; C2 at 8 192: 0.133 / 0.187).  At 16 384 the two cross: every agent alive 0.258 / 0.226, over
// ticks 50-550 of a run (fewer alive) 0.223 / 0.250 — the longer run decides, 16 384 stays small.
#define SMX_LARGE_BATCH_VEHICLES 16384
#ifndef SMX_SCAN_WIDE_MAX_VEHICLES  // the team scan halves take eight lanes a vehicle up to this many vehicles, four above
#define SMX_SCAN_WIDE_MAX_VEHICLES 65536
#endif
#ifndef SMX_ONE_LANE_ON_SPLIT_MAPS  // developer: the one-lane cut on maps whose lanes split too
#define SMX_ONE_LANE_ON_SPLIT_MAPS 0
#endif
#ifndef SMX_ONE_LANE_MIN_VEHICLES  // the one-lane cut's seeds half is the one-lane kernel + slow chain from this many vehicles on
#define SMX_ONE_LANE_MIN_VEHICLES 114688
#endif
#ifndef SMX_OGM_ENV_MIN_VEHICLES  // small form: OGM tiles by k_ogm_env from this many vehicles on (smarts_amd/engine.py mirrors it)
#define SMX_OGM_ENV_MIN_VEHICLES 8192
#endif
#ifndef SMX_FACTS_EARLY_MAX  // the facts half leaves with the grid kernels up to this many vehicles, else after the seeds half
#define SMX_FACTS_EARLY_MAX 32768
#endif
// developer timing switches (SMX_SKIP in smx_tick.h) that change the plan: the small form / its split scan forced
#define SMX_SKIP_FORCE_SMALL 131072
#define SMX_SKIP_FORCE_SCAN_SPLIT 65536

// slow_blob: [4][total] slow lists of the one-lane kernels + [2][4] counters in list order (ticks alternate)
struct SlowLists {
  enum { FACTS, SEEDS, CONTROL, ROWS, COUNT };
  int32_t* base;
  size_t total;
  static size_t size(size_t total) { return COUNT * total + 2 * COUNT; }
  int32_t* list(int i) const { return base + (size_t)i * total; }
  int32_t* counters(int parity) const { return base + COUNT * total + COUNT * parity; }
};

// one kernel's slow list and the counter it appends to / reads (KernelArgs::slow_list, slow_count)
struct SlowRef {
  int32_t* list;
  int32_t* count;
};

struct PlanInputs {
  const smx_config* cfg;
  int launch_strategy;  // SMX_LAUNCH_*
  bool map_junctions;   // lanes of the map split
  int slow_blocks;      // grid of the slow lists' kernels (smx_load_map)
  bool routed;          // some slot (with a mission pool: some pool entry) has a fixed route: the scan instance that knows them
  bool pool_bound;      // smx_set_mission_pool holds a pool: the kernels' pool instances (mission_row, smx_tick.h)
  bool is_step;
  bool phase_timing;  // smx_set_timing level 2 (and room for this call's events): one boundary event after every kernel
  bool side_ready;
  bool list_carried;  // the last pass's k_tail built this tick's alive list from these flags
  int debug_skip;     // developer timing switches; 0 in the shipped library
  bool alive_blob, knots_blob, ctrl_blob;
  bool knot_table;  // the map's knot table is built and switched on
  uint8_t* pending_blob;  // [total] seed_pending, or null
  SlowLists slow;         // (base null: no slow lists)
  int slow_parity;        // the counters this tick's one-lane kernels use
  bool frame_stack_bound;  // smx_bind_frame_stack holds at least one buffer
  bool guard_bound;        // smx_set_guard holds a buffer: the state guard is on
  bool history_bound;      // smx_set_social_history holds a table: the social slots replay it
  bool dims_bound;         // smx_set_social_history_dims holds a table: ... at each vehicle's own dimensions
  bool agent_dims_bound;   // smx_set_agent_dims holds a table: the agents at their own (either one: a triple block is bound)
  bool follow_entry;       // the call is smx_step_history_agents: the agents are placed on their recorded vehicles' rows
  bool ogm_mask;           // the handle holds the OGM tiles' piece mask and smx_set_ogm_delta has not switched it off
  bool handover_entry;     // the call is smx_step_history_handover: each agent follows or is driven, as its handover tick says
  bool bubbles_bound;      // smx_set_history_bubbles holds bubbles: that call's tick starts with k_bubbles and reads its state row
  bool entry_bound;        // smx_set_agent_entry holds a table: pending agents enter inside a tick (k_entry)
  // smx_set_agent_spaces holds a table: bit s = some agent slot has SMX_ACTION_SPACE_* s (0: none bound) ...
  unsigned agent_spaces;
  bool mixed_entry;        // ... and the call is smx_step_mixed, the only tick there is while one is bound
};

enum class AliveList : uint8_t { NONE, CARRIED, BUILD };  // BUILD: k_alive_list ahead of the tick
// ONE / ONE_LDS: k_control (the LDS-path form fits one wavefront per SIMD: only while the batch needs no more);
// large batches: candidate paths by teams of four, then law + physics with one lane per vehicle (PATHS_LAW), the float
// spaces and Trajectory the law alone (LAW); FAST_LISTED: one lane per vehicle, the rest through the slow list;
// KINEMATIC: the kinematic spaces' k_control_kinematic, one lane per vehicle in either form (no candidate paths, no
// control slow list); KINEMATIC_FOLLOW: its FOLLOW form, the tick of smx_step_history_agents — the same launch;
// KINEMATIC_HANDOVER: its HANDOVER form, the tick of smx_step_history_handover — the same launch again;
// KINEMATIC_BUBBLES: that tick with bubbles bound (smx_set_history_bubbles) — k_bubbles, then the BUBBLES form (it
// stands first with its number: the older values keep theirs, and the line they end, which a test reads);
// MIXED: the tick of smx_step_mixed over a table of several spaces (or one that is not cfg.action_space) — one launch or
// pair of launches per space present, each in the form TickPlan::control_of names for it (it stands first as well)
enum class Control : uint8_t { MIXED = 10, KINEMATIC_BUBBLES = 9, NONE = 0, ONE, ONE_LDS, PATHS_LAW, LAW, FAST_LISTED, KINEMATIC, KINEMATIC_FOLLOW, KINEMATIC_HANDOVER };
static constexpr bool smx_kinematic_space(int action_space) {
  // (one mask test; smx_create holds action_space to 0 .. SMX_ACTION_SPACE_IMITATION)
  constexpr unsigned kinematic = (1u << SMX_ACTION_SPACE_TARGET_POSE) | (1u << SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME) |
                                 (1u << SMX_ACTION_SPACE_IMITATION);
  return ((kinematic >> (action_space & 31)) & 1u) != 0;
}
// SCAN: the small form's k_scan (both halves); large form: the one-lane kernel (+ slow list / chain), k_scan_half with the
// routed instance, with eight lanes a vehicle, with four
enum class Seeds : uint8_t { SCAN, ONE_LANE, ROUTED, WIDE, FOUR };
enum class Facts : uint8_t { SCAN, ONE_LANE, WIDE, FOUR };
enum class FactsStart : uint8_t { CALLER, WITH_GRIDS, AFTER_SEEDS };  // (side stream 1 unless CALLER)
// The waypoint rows, and with them the seeds kernel that may feed them: SENSORS the role inside k_sensors (small form);
// large form: k_wp_walk -> k_waypoints_emit + k_waypoints_listed (EMIT, one-lane cut; without k_wp_walk where the knot
// table serves the tick: TickPlan::knot_table) or -> k_waypoints_tables (TABLES,
// teams cut) while the rows fit the staged form, else k_waypoints (UNSTAGED), which reads every vehicle's seeds (no
// seed_pending) and so cannot run beside or ahead of a slow seeds chain.  Only the two *_CHAIN_* values have the one-lane
// seeds kernel, which leaves the vehicles it cannot serve seed_pending: the walk / emit kernels then pass over those
// vehicles and the slow chain — from-scratch searches, then their walks and rows by the serial emitter — runs once, on
// side stream 2 beside the main chain or on the caller's stream after the rows.
enum class Rows : uint8_t { SENSORS, UNSTAGED, TABLES, EMIT, EMIT_CHAIN_SIDE, EMIT_CHAIN_AFTER };
enum class SlowChain : uint8_t { NONE, SIDE, AFTER_ROWS };
// OGM tiles: inside k_sensors (small form, up to 16 KiB of dynamic LDS), or a launch of their own — per env (four
// wavefronts share the env's poses) while four tiles (ENV1) or eight (ENV2) fit a workgroup's LDS, else per observer
enum class Ogm : uint8_t { NONE, IN_SENSORS, ENV2, ENV1, PER_OBSERVER };
enum class Lidar : uint8_t { NONE, IN_SENSORS, SIDE, CALLER };

struct TickPlan {
  int form;  // SMX_FORM_*
  bool is_step, phased, routed;
  bool pool;  // the pool instances of the kernels that read a per-mission table (k_*_pool); without a pool the others, which hold no lookup
  bool social;  // k_social (IDM) ahead of the tick
  AliveList alive;
  int32_t* alive_zero;  // BUILD: the other parity's slow counters, zeroed by k_alive_list
  Control control;
  // Control::MIXED: the spaces the table holds (PlanInputs::agent_spaces) and, per space present, the form its launches
  // take — ONE in the small form (k_control_slots over the space's slot list), in the large form PATHS_LAW for the two
  // lane spaces and LAW for the other four (the _mixed kernels, which filter by the table); NONE for a space not present.
  // A table whose only space is cfg.action_space needs neither: the tick is the uniform one under the teams cut, `control`
  // is its form and control_of names it too.
  unsigned mixed_spaces;
  Control control_of[SMX_ACTION_SPACE_IMITATION + 1];
  SlowRef control_slow;
  // Large batches, no per-kernel timing asked: the grid maps and the lidar (which read poses only) leave on
  // side stream 0 at once and overlap the scan — kernels bound by their own write stream beside one bound by
  // arithmetic and load latency; observe goes to side stream 1 after the scan, the waypoint kernels stay on
  // the caller's stream; all are joined before k_tail.
  bool fork;
  bool scan_split;  // SCAN: k_scan's halves as separate roles
  Seeds team_seeds;  // the seeds kernel unless the rows have a chain (seeds())
  Facts facts;
  FactsStart facts_start;
  Rows rows;
  bool chain_fused;  // SIDE on a map without splits: eight-lane searches, walk and rows in one kernel
  SlowRef facts_slow, seeds_slow, rows_slow;
  Ogm ogm;
  // the OGM kernels store only the pieces of a tile that are, or a call ago were, non-zero (KernelArgs::ogm_mask); false:
  // the null mask, every piece is stored.  Tiles that are no whole number of pieces keep the null mask.
  bool ogm_delta;
  Lidar lidar;
  bool dagm, road_waypoints;
  bool rgb;  // k_rgb (SMX_SENSOR_RGB): wherever k_dagm is launched; rgb_lds = its class tile, a byte a pixel
  size_t rgb_lds;
  // k_lane_ttc (SMX_SENSOR_LANE_TTC): in a tick over every agent, on the caller's stream once the waypoint, neighbour
  // and ego rows are complete (after the joins); in the reset pass over the env groups k_tail listed, after k_first
  bool lane_ttc;
  unsigned ttc_blocks, ttc_first_blocks;
  size_t ttc_lds;  // per workgroup: SMX_BLOCK / SMX_TTC_TEAM agents' waypoints (x, y, arclength, lane id) and per-path minima
  // k_ego_frame (SMX_SENSOR_EGO_CENTRIC): the same two sites, after k_lane_ttc (both only read the world rows)
  bool ego_centric;
  unsigned ec_blocks, ec_first_blocks;
  // k_frame_push / k_frame_dstack (smx_config.frame_stack with something bound): the last launches of the pass, on the
  // caller's stream, after the observation pass has joined and after k_tail / the reset pass (they read the pass's
  // finished rows, the flags it left, this tick's done row and env_done) — in a tick and in smx_reset, in either form
  bool frame_stack;
  // the state guard (smx_set_guard): the GUARD instantiations of the control kernels, k_reset and k_tail in the places of
  // the plain ones — the same launches on the same streams, no kernel and no edge more
  bool guard;
  // per-vehicle dimensions (smx_set_social_history_dims or smx_set_agent_dims: a triple block is bound): the SIZED instantiations of k_ogm_env, k_lidar and k_lidar_first
  // in the places of the plain ones — the same launches on the same streams; every other reader branches on the pointer
  bool sized;
  // delayed agent entry (smx_set_agent_entry holds a table): the ENTRY instantiations of k_reset in a reset call (the
  // tick's commit, which restarts envs under auto_reset, asks the argument block), and in a tick k_entry after the control
  // phase, ahead of the observation pass, on the caller's stream.  The small form's tick kernels visit every vehicle, so
  // the entrant's first observation is the tick's own; the large forms' tick lists its vehicles a tick ahead (entry_first)
  bool entry;
  // ... in a large form's tick: k_entry_first after k_tail, and the reset pass over the groups it lists (reset_pass)
  bool entry_first;
  bool tail_builds_list;  // k_tail builds the next tick's alive list
  bool tail_grids;        // ... and the new vehicles' grid tiles
  bool reset_pass, lidar_first, first_walks_new;
  // the one-lane cut's tick takes its knot lists from the map's knot table: k_waypoints_emit and k_control_fast read
  // rows, k_wp_walk is not launched, and k_first walks no list for the new vehicles (first_walks_new is then false)
  bool knot_table;
  unsigned veh_blocks, wp_blocks, obs_blocks, env_blocks, lidar_blocks, seeds_blocks, facts_blocks, slow_blocks, sensor_blocks;
  size_t ogm_bytes, dagm_bytes, ogm_lds, sensor_lds;
  uint8_t* pending;  // seed_pending of the one-lane seeds kernel, its chain and the walk / emit kernels; else null

  bool small() const { return form == SMX_FORM_SMALL; }
  SlowChain chain() const {
    return rows == Rows::EMIT_CHAIN_SIDE ? SlowChain::SIDE : rows == Rows::EMIT_CHAIN_AFTER ? SlowChain::AFTER_ROWS : SlowChain::NONE;
  }
  Seeds seeds() const { return chain() != SlowChain::NONE ? Seeds::ONE_LANE : team_seeds; }
  uint8_t* seed_pending() const { return chain() != SlowChain::NONE ? pending : nullptr; }
};

static inline unsigned smx_blocks(size_t threads, size_t block = SMX_BLOCK) { return (unsigned)((threads + block - 1) / block); }

// k_lane_ttc's LDS per agent: x, y, arclength (float64) of wp_paths x wp_len waypoints, per-path ttc / dtc minima
// (float64), waypoint counts (int32), lane ids (int16), rounded up to 8 bytes.  (constexpr: the kernel carves with it too)
static constexpr size_t smx_ttc_lds_per_agent(int wp_paths, int wp_len) {
  return 3 * 8 * ((size_t)wp_paths * wp_len) + 2 * 8 * (size_t)wp_paths +
         ((4 * (size_t)wp_paths + 2 * ((size_t)wp_paths * wp_len) + 7) & ~(size_t)7);
}

static inline TickPlan tick_plan(const PlanInputs& in) {
  const smx_config& c = *in.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  TickPlan p{};
  p.is_step = in.is_step;
  p.phased = in.phase_timing && in.is_step;
  p.routed = in.routed;
  p.pool = in.pool_bound;
  // Small batches are bound by one wavefront's latency, so independent work is spread over more
  // workgroups (k_scan halves as separate roles: 54 vs 70 us at 8 k vehicles; the OGM role inside
  // k_sensors); large batches are bound by throughput, where the same tricks cost occupancy
  // (131 k vehicles: k_scan 0.69 vs 0.52 ms split vs back-to-back, OGM inside k_sensors +6 %).
  const bool small = in.launch_strategy == SMX_LAUNCH_SMALL ||
                     (in.launch_strategy == SMX_LAUNCH_AUTO && total <= SMX_LARGE_BATCH_VEHICLES) ||
                     (in.debug_skip & SMX_SKIP_FORCE_SMALL);
  // Which cut of the LARGE form a batch takes (smx.h, smx_launch_form): one lane per vehicle + slow lists where the lists
  // stay short: a map whose lanes never split (loop: under 1 % of the vehicles).  Where lanes branch and cross, a third
  // of the vehicles would take the lists' serial forms (minicity, 262 144 vehicles: 1.40 ms a tick against 0.9x with
  // round 2's team kernels for everybody), so those maps keep the team kernels.  The strategies LARGE_ONE_LANE /
  // LARGE_TEAMS force a cut.
  // A bound table of agent spaces acts like LARGE_TEAMS: k_control_fast / k_control_listed have no per-space forms.
  const bool one_lane_cut = in.agent_spaces == 0 &&
                            (in.launch_strategy == SMX_LAUNCH_LARGE_ONE_LANE ||
                             (in.launch_strategy != SMX_LAUNCH_LARGE_TEAMS && (!in.map_junctions || SMX_ONE_LANE_ON_SPLIT_MAPS)));
  p.form = small ? SMX_FORM_SMALL : (in.alive_blob && in.slow.base && one_lane_cut) ? SMX_FORM_LARGE_ONE_LANE : SMX_FORM_LARGE_TEAMS;
  // the tick of the one-lane cut (not a reset call): one-lane kernels + teams over their slow lists
  const bool one_lane = in.is_step && p.form == SMX_FORM_LARGE_ONE_LANE;
  const bool idm = c.num_social > 0 && c.social_model == SMX_SOCIAL_IDM;
  const bool staged = (c.sensors & SMX_SENSOR_WAYPOINTS) && c.wp_paths <= SMX_WPT_MAX_PATHS && in.knots_blob;
  const bool lidar = (c.sensors & SMX_SENSOR_LIDAR) != 0;
  p.social = in.is_step && idm;
  p.alive = !(in.is_step && !small && in.alive_blob) ? AliveList::NONE : in.list_carried ? AliveList::CARRIED : AliveList::BUILD;
  p.alive_zero = (p.alive == AliveList::BUILD && in.slow.base) ? in.slow.counters(in.slow_parity ^ 1) : nullptr;
  if (one_lane) {
    int32_t* const counters = in.slow.counters(in.slow_parity);
    p.facts_slow = {in.slow.list(SlowLists::FACTS), counters + SlowLists::FACTS};
    p.seeds_slow = {in.slow.list(SlowLists::SEEDS), counters + SlowLists::SEEDS};
    if (!smx_kinematic_space(c.action_space)) p.control_slow = {in.slow.list(SlowLists::CONTROL), counters + SlowLists::CONTROL};
    p.rows_slow = {in.slow.list(SlowLists::ROWS), counters + SlowLists::ROWS};
  }
  const bool lane_space = c.action_space == SMX_ACTION_SPACE_LANE || c.action_space == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED;
  if (!in.is_step)
    p.control = Control::NONE;
  else if (smx_kinematic_space(c.action_space))
    p.control = in.handover_entry ? (in.bubbles_bound ? Control::KINEMATIC_BUBBLES : Control::KINEMATIC_HANDOVER)
                : in.follow_entry ? Control::KINEMATIC_FOLLOW
                                  : Control::KINEMATIC;
  else if (!small && in.ctrl_blob)
    p.control = !lane_space ? Control::LAW : one_lane ? Control::FAST_LISTED : Control::PATHS_LAW;
  else
    p.control = (lane_space && small && total * SMX_WP_LANES <= (size_t)1024 * 64) ? Control::ONE_LDS : Control::ONE;
  if (in.is_step && in.mixed_entry && in.agent_spaces != 0) {
    p.mixed_spaces = in.agent_spaces;
    if (in.agent_spaces == (1u << c.action_space)) {
      p.control_of[c.action_space] = p.control;
    } else {
      p.control = Control::MIXED;
      for (int s = 0; s <= SMX_ACTION_SPACE_IMITATION; ++s) {
        if (!((in.agent_spaces >> s) & 1u)) continue;
        const bool lanes = s == SMX_ACTION_SPACE_LANE || s == SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED;
        p.control_of[s] = (small || !in.ctrl_blob) ? Control::ONE : lanes ? Control::PATHS_LAW : Control::LAW;
      }
    }
  }

  p.fork = in.is_step && !small && !p.phased && in.side_ready;
  p.scan_split = small || (in.debug_skip & SMX_SKIP_FORCE_SCAN_SPLIT);
  // (where the searches are long — lanes that split and cross: 4lane 2048 x 16 0.430 -> 0.393 ms; on loop the four-lane
  // teams stay: 32 768 vehicles 0.260 either way, 65 536 0.371 against 0.378)
  const bool wide = in.map_junctions && total <= SMX_SCAN_WIDE_MAX_VEHICLES;
  p.team_seeds = small ? Seeds::SCAN : in.routed ? Seeds::ROUTED : wide ? Seeds::WIDE : Seeds::FOUR;
  p.facts = small ? Facts::SCAN : one_lane ? Facts::ONE_LANE : wide ? Facts::WIDE : Facts::FOUR;
  // the facts half (-> observe) has slack, the seeds half heads the tick's longest chain (-> walk -> rows): the
  // facts half starts when the seeds half is done and then fills the chip beside the waypoint kernels, whose two
  // wavefronts per SIMD leave it half empty (C4, ticks 20-220: 0.815 -> 0.792 ms)
  // (late in a run, with 40 % of the agents alive, starting both halves together is 1.5 % faster; with 80 % alive
  // it is 4 % slower)
  // (at 32 768 vehicles — a quarter of the headline batch, one rank's shard at four GPUs — the chains are short and
  // both halves start together: 0.241 against 0.249 ms; at 65 536 the order above wins, 0.294 against 0.300)
  // (holding the grid kernels back as well was slower: 0.81 -> 0.85 ms; they overlap the seeds half.  So was one fork
  // event after the seeds half for the grid kernels too, one record less on the caller's stream: C4 0.556 -> 0.605 ms)
  p.facts_start = !p.fork ? FactsStart::CALLER : total <= SMX_FACTS_EARLY_MAX ? FactsStart::WITH_GRIDS : FactsStart::AFTER_SEEDS;
  // One-lane seeds — path seeds without the ten-nearest list — serve agents with a route object and no fixed route and
  // staged rows (past SMX_WPT_MAX_PATHS rows the team seeds kernel serves everybody, as in the teams cut).  And inside
  // the one-lane cut the seeds half is the one-lane kernel + the slow seeds chain, or the team kernel for everybody:
  // the chain is 110 us of latency behind the seeds kernel whatever the batch, and below SMX_ONE_LANE_MIN_VEHICLES it
  // ends the tick; the team seeds kernel then costs less than it saves (C4's shards, default run / ticks 5-65, ms per
  // tick, team seeds against one-lane seeds: 1024 envs 0.195 / 0.265 against 0.266 / 0.284; 2048: 0.251 / 0.378 against
  // 0.288 / 0.383; 3072: 0.286 / 0.455 against 0.325 / 0.477; 4096: 0.367 / 0.603 against 0.380 / 0.579; the team kernels
  // throughout: 0.227 / 0.287, 0.273 / 0.435, 0.371 / 0.593, 0.440 / 0.768).
  const bool one_lane_seeds = one_lane && !in.routed && staged && in.pending_blob &&
                              (in.launch_strategy == SMX_LAUNCH_LARGE_ONE_LANE || total >= SMX_ONE_LANE_MIN_VEHICLES);
  p.rows = small ? Rows::SENSORS
           : !staged ? Rows::UNSTAGED
           : !one_lane ? Rows::TABLES
           : !one_lane_seeds ? Rows::EMIT
           : p.fork ? Rows::EMIT_CHAIN_SIDE : Rows::EMIT_CHAIN_AFTER;
  p.chain_fused = p.rows == Rows::EMIT_CHAIN_SIDE && !in.map_junctions;
  p.pending = in.pending_blob;

  p.ogm_bytes = (c.sensors & SMX_SENSOR_OGM) ? (size_t)c.ogm_width * c.ogm_height : 0;
  p.dagm_bytes = (c.sensors & SMX_SENSOR_DAGM) ? (size_t)c.dagm_width * c.dagm_height : 0;
  const bool env2_fits = c.num_vehicles <= 32 && p.ogm_bytes * SMX_OGM_WAVES * 2 <= 64 * 1024;
  // (from SMX_OGM_ENV_MIN_VEHICLES on, the per-env kernel of the large form beats the per-observer role inside
  // k_sensors even as a launch of its own on the same stream: a third of the instructions per tile)
  if (!p.ogm_bytes)
    p.ogm = Ogm::NONE;
  else if (env2_fits && (!small || total >= SMX_OGM_ENV_MIN_VEHICLES))
    p.ogm = Ogm::ENV2;
  else if (small)
    p.ogm = p.ogm_bytes <= 16 * 1024 ? Ogm::IN_SENSORS : Ogm::PER_OBSERVER;
  else
    p.ogm = p.ogm_bytes * SMX_OGM_WAVES <= 64 * 1024 ? Ogm::ENV1 : Ogm::PER_OBSERVER;
  p.ogm_lds = p.ogm == Ogm::ENV2 ? p.ogm_bytes * SMX_OGM_WAVES * 2 : p.ogm == Ogm::ENV1 ? p.ogm_bytes * SMX_OGM_WAVES : p.ogm_bytes;
  p.ogm_delta = in.ogm_mask && p.ogm_bytes != 0 && p.ogm_bytes % SMX_OGM_PIECE == 0;
  p.dagm = p.dagm_bytes != 0;
  p.rgb = (c.sensors & SMX_SENSOR_RGB) != 0;
  p.rgb_lds = p.rgb ? (size_t)c.rgb_width * c.rgb_height : 0;
  p.lidar = !lidar ? Lidar::NONE : small ? Lidar::IN_SENSORS : p.fork ? Lidar::SIDE : Lidar::CALLER;
  p.road_waypoints = (c.sensors & SMX_SENSOR_ROAD_WAYPOINTS) != 0;
  p.lane_ttc = (c.sensors & SMX_SENSOR_LANE_TTC) != 0;

  // k_tail builds the next tick's alive list unless k_social moves vehicles (and can end them) ahead of the list, or a
  // traffic history is bound: the reset pass's commit then still changes SMX_F_ALIVE of the new envs' social slots (a
  // slot shows the reset observation's frame in that pass and the next frame in the tick after it), behind k_tail
  p.tail_builds_list = !small && in.alive_blob && in.slow.base && !idm && !in.history_bound;
  // (in a step, k_tail's commit respawns the envs that ended; with an entry table bound, a large form's tick also gives
  // its entrants their first observation there)
  p.entry_first = in.entry_bound && in.is_step && !small;
  p.reset_pass = !in.is_step || c.auto_reset || p.entry_first;
  p.tail_grids = p.reset_pass && (p.ogm_bytes || p.dagm_bytes || p.rgb);
  // large batches: the new vehicles' lidar as a launch of its own instead of one after the other inside
  // k_first — at C5 an env restart brings 64 new vehicles, whose serial lidar roles made the reset pass 0.58 ms
  // of a 1.5 ms tick late in a run (many restarts per tick)
  p.lidar_first = p.reset_pass && lidar && !small;
  // large batches: k_first also walks the new vehicles' knot lists, for the next tick's k_control_fast
  // (only k_control_fast reads them: not on the maps that keep the team kernels)
  // The table serves the lookaheads the controller's reuse is defined for (k_control_fast sends every vehicle to its slow
  // list below that, with or without it), and batches without fixed routes: a route's filter names an agent slot (a pool row with a mission pool bound), which
  // no row is walked for, so with routes set the tick keeps the walked lists and every launch it had.
  const bool table = in.knot_table && !in.routed && staged && c.wp_lookahead >= 16;
  p.knot_table = table && one_lane;
  // (the reset pass of a tick whose form is the one-lane cut: the next tick's k_control_fast reads rows, not lists)
  p.first_walks_new = p.reset_pass && !small && one_lane_cut && staged && !(table && p.form == SMX_FORM_LARGE_ONE_LANE);

  const int vpb = SMX_BLOCK / SMX_WP_LANES, epb = SMX_BLOCK / c.num_vehicles;
  p.veh_blocks = smx_blocks(total);
  p.wp_blocks = smx_blocks(total, vpb);
  p.obs_blocks = (unsigned)((c.num_envs + epb - 1) / epb);
  p.env_blocks = smx_blocks((size_t)c.num_envs);
  p.lidar_blocks = lidar ? (unsigned)total : 0;
  p.slow_blocks = (unsigned)in.slow_blocks;
  p.seeds_blocks = small ? (p.scan_split ? 2 : 1) * smx_blocks(total * SMX_TEAM)
                   : one_lane_seeds ? p.veh_blocks
                   : p.team_seeds == Seeds::WIDE ? smx_blocks(total * SMX_TEAM) : smx_blocks(total * SMX_TEAM_LARGE);
  p.facts_blocks = one_lane ? p.veh_blocks : wide ? smx_blocks(total * SMX_TEAM) : smx_blocks(total * SMX_TEAM_LARGE);
  p.sensor_blocks = p.wp_blocks + p.obs_blocks + p.lidar_blocks + (p.ogm == Ogm::IN_SENSORS ? (unsigned)total : 0);
  p.sensor_lds = p.ogm == Ogm::IN_SENSORS ? p.ogm_bytes : 0;
  if (p.lane_ttc) {
    const size_t apb = SMX_BLOCK / SMX_TTC_TEAM;  // agents per workgroup
    p.ttc_blocks = smx_blocks(total, apb);
    p.ttc_first_blocks = p.reset_pass ? p.obs_blocks * (unsigned)(SMX_BLOCK / apb) : 0;  // an env group holds up to SMX_BLOCK vehicles
    p.ttc_lds = apb * smx_ttc_lds_per_agent(c.wp_paths, c.wp_len);
  }
  p.frame_stack = c.frame_stack > 0 && in.frame_stack_bound;
  p.guard = in.guard_bound;
  p.sized = in.dims_bound || in.agent_dims_bound;
  p.entry = in.entry_bound;
  p.ego_centric = (c.sensors & SMX_SENSOR_EGO_CENTRIC) != 0;
  if (p.ego_centric) {
    const size_t apb = SMX_BLOCK / SMX_EC_TEAM;
    p.ec_blocks = smx_blocks(total, apb);
    p.ec_first_blocks = p.reset_pass ? p.obs_blocks * (unsigned)(SMX_BLOCK / apb) : 0;
  }
  return p;
}

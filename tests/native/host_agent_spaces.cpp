// Stand-alone host program over the device-free side of per-agent action spaces (tests/test_host_agent_spaces.py builds
// it with -fsanitize=address,undefined and runs it), over shim/hip_memory.h as tests/native/host_agent_entry.cpp is:
//   (a) smx_check_agent_spaces' rule (smarts_amd/csrc/smx_host.h check_agent_spaces_impl) over every refusal, each with a
//       message that names the slot, on heap tables of exactly the stated size;
//   (b) the handle (smarts_amd/csrc/smx_handle.h): smx_set_agent_spaces fill, then commit — bind before a map, a new map
//       keeps it, rebind, unbind — the blob's contents (the table with the social slots on the owner space, the slot
//       lists), which tick entry is taken while bound and while not (check_step_entry: the uniform entries, smx_step_mixed
//       and its buffers), and the kinematic bindings refused beside it; then the same sequence once for every HIP call of
//       the clean run with that call failing: the call returns SMX_ERR_HIP, the binding in place is untouched or none is
//       left, every pointer a kernel would get is null or inside a live allocation of its size, the call succeeds when
//       repeated, and nothing is live after smx_destroy.
// Prints one JSON line and returns 0 when every check held, else prints the failed checks and returns 1.
#include <hip_memory.h>  // the stand-in (and through it the shim <hip/hip_runtime.h>): plain C++

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "smx_handle.h"
#include "tiny_map.h"

static int failures = 0, checks = 0;
static std::string context;
static void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    std::printf("FAILED [%s]: %s\n", context.c_str(), what.c_str());
  }
}
static bool contains(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }

enum { E = 2, N = 5, SOCIAL = 2, AGENTS = N - SOCIAL, TOTAL = E * N, SPACES = SMX_ACTION_SPACE_IMITATION + 1 };

static smx_config config(int action_space = SMX_ACTION_SPACE_LANE) {
  smx_config c{};
  c.num_envs = E, c.num_vehicles = N, c.dt = 0.1, c.num_social = SOCIAL, c.social_speed_factor = 1.0;
  c.action_space = action_space;
  c.sensors = SMX_SENSOR_WAYPOINTS;
  c.wp_lookahead = 32, c.wp_paths = 4, c.wp_len = 20, c.nb_radius = 50.0;
  return c;
}

// ---- (a) the check, over a heap table of exactly n entries
static void check_refusals() {
  context = "check";
  std::string why;
  auto run = [&](const smx_config& c, const int32_t* space, int32_t n) {
    smx_agent_spaces d{};
    d.space_host = space, d.n_agents = n;
    why.clear();
    return check_agent_spaces_impl(c, d, why);
  };
  const int mixable[] = {SMX_ACTION_SPACE_LANE, SMX_ACTION_SPACE_CONTINUOUS, SMX_ACTION_SPACE_ACTUATOR_DYNAMIC,
                         SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED, SMX_ACTION_SPACE_TRAJECTORY, SMX_ACTION_SPACE_MPC};
  const int kinematic[] = {SMX_ACTION_SPACE_TARGET_POSE, SMX_ACTION_SPACE_TRAJECTORY_WITH_TIME, SMX_ACTION_SPACE_IMITATION};
  int32_t* t = new int32_t[AGENTS];
  for (int a : mixable)
    for (int b : mixable)
      for (int cfg_space : mixable) {
        t[0] = a, t[1] = b, t[2] = a;
        expect(run(config(cfg_space), t, AGENTS) == SMX_OK, "a table of mixable spaces is taken: " + why);
      }
  t[0] = t[1] = t[2] = SMX_ACTION_SPACE_CONTINUOUS;
  expect(run(config(), t, AGENTS) == SMX_OK, "a table whose entries are all equal is legal (and need not be cfg.action_space)");
  expect(run(config(), nullptr, AGENTS) == SMX_ERR_INVALID && contains(why, "null table"), "a null table: " + why);
  expect(run(config(), t, AGENTS - 1) == SMX_ERR_INVALID && contains(why, "n_agents is 2") && contains(why, "slot 2 has no entry"), "a short table: " + why);
  expect(run(config(), t, AGENTS + 1) == SMX_ERR_INVALID && contains(why, "n_agents is 4") && contains(why, "slot 3 is no agent slot"), "a long table: " + why);
  expect(run(config(), t, N) == SMX_ERR_INVALID && contains(why, "n_agents is 5"), "a table over every slot (the social ones have no space): " + why);
  expect(run(config(), t, 0) == SMX_ERR_INVALID && run(config(), t, -1) == SMX_ERR_INVALID && contains(why, "slot 0"), "n_agents <= 0: " + why);
  for (int at = 0; at < AGENTS; ++at) {
    for (int k : kinematic) {
      t[0] = t[1] = t[2] = SMX_ACTION_SPACE_LANE;
      t[at] = k;
      expect(run(config(), t, AGENTS) == SMX_ERR_INVALID && contains(why, "slot " + std::to_string(at) + ":") && contains(why, "kinematic") &&
                 contains(why, action_space_name(k)),
             "a kinematic entry: " + why);
    }
    for (int bad : {-1, 9, 10, 1 << 20, -2147483647 - 1}) {
      t[0] = t[1] = t[2] = SMX_ACTION_SPACE_TRAJECTORY;
      t[at] = bad;
      expect(run(config(), t, AGENTS) == SMX_ERR_INVALID && contains(why, "slot " + std::to_string(at) + ":") && contains(why, "no SMX_ACTION_SPACE_"),
             "an unknown entry: " + why);
    }
  }
  t[0] = t[1] = t[2] = SMX_ACTION_SPACE_LANE;
  for (int k : kinematic)
    expect(run(config(k), t, AGENTS) == SMX_ERR_INVALID && contains(why, "cfg.action_space is") && contains(why, action_space_name(k)),
           "a kinematic cfg.action_space: " + why);
  smx_config none = config();
  none.num_social = N;
  expect(run(none, t, 0) == SMX_ERR_INVALID && contains(why, "no agents"), "a configuration without agents");
  delete[] t;
}

// ---- (b) the handle
static int fake_knot_table(smx_handle_s* h, KnotRow* table) {
  std::memset(table, 0, (size_t)h->map.n_lanepoints * sizeof(KnotRow));
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}
static const KernelSide KERNELS = {352, 64 * 11 * 36, 0, fake_knot_table, nullptr};

struct World {
  smx_handle h = nullptr;
  smx_config cfg = config();
  Map map_a, map_b;
  std::vector<int32_t> spaces{SMX_ACTION_SPACE_TRAJECTORY, SMX_ACTION_SPACE_CONTINUOUS, SMX_ACTION_SPACE_TRAJECTORY};
  std::vector<double> dims = std::vector<double>((size_t)E * AGENTS * 3, 2.0);
  smx_agent_spaces table() {
    smx_agent_spaces d{};
    d.space_host = spaces.data(), d.n_agents = (int32_t)spaces.size();
    return d;
  }
};

// the committed binding: the table over every slot (the social ones on the owner space), then the slot lists
static bool spaces_bound(const World& w) {
  const smx_handle_s* h = w.h;
  const AgentSpacesDev& d = h->spaces;
  if (!h->spaces_blob || d.space != h->spaces_blob.get<int32_t>() || d.slots != d.space + N) return false;
  if (!shim_hip.inside(d.space, (size_t)(1 + SPACES) * N * sizeof(int32_t))) return false;
  unsigned mask = 0;
  for (int32_t s : w.spaces) mask |= 1u << s;
  const int owner = __builtin_ctz(mask);
  if (d.mask != mask || d.owner != owner) return false;
  int count[SPACES] = {};
  for (int slot = 0; slot < N; ++slot) {
    const int s = slot < AGENTS ? w.spaces[slot] : owner;
    if (d.space[slot] != s) return false;
    if (d.slots[s * N + count[s]++] != slot) return false;  // ascending, the social slots last in the owner's list
  }
  for (int s = 0; s < SPACES; ++s)
    if (d.count[s] != count[s]) return false;
  return true;
}
static bool spaces_none(const smx_handle_s* h) {
  bool zero = !h->spaces_blob && !h->spaces.space && !h->spaces.slots && h->spaces.mask == 0 && h->spaces.owner == 0;
  for (int s = 0; s < SPACES; ++s) zero = zero && h->spaces.count[s] == 0;
  return zero;
}
static bool live_or_null(const void* p, size_t bytes) { return p == nullptr || shim_hip.inside(p, bytes); }
// what holds after every call, failed or not
static void check_handle(const smx_handle_s* h) {
  if (!h) return;
  expect((h->spaces.space != nullptr) == (bool)h->spaces_blob, "the table with its blob");
  expect(live_or_null(h->spaces.space, (size_t)(1 + SPACES) * N * sizeof(int32_t)), "spaces.space is null or a live allocation of its size");
  expect(!(h->spaces.space && (h->history.follow || h->dims.agent)), "never a table beside history agents or agent dimensions");
  const DeviceBlob* blobs[] = {&h->map_blob, &h->knots_blob, &h->spill_blob, &h->knot_table, &h->knot_stats, &h->alive_blob, &h->pending_blob, &h->slow_blob,
                               &h->scan_carry, &h->ctrl_blob, &h->status_dev, &h->vias_dev, &h->via_off_dev, &h->missions_blob, &h->goals_blob,
                               &h->history_blob, &h->ogm_mask, &h->dims_blob, &h->agent_dims_blob, &h->entry_blob, &h->spaces_blob};
  size_t owned = 0;
  for (const DeviceBlob* b : blobs) {
    expect(!*b || shim_hip.live.count(b->get<const char>()) == 1, "every blob of the handle is empty or a live allocation");
    owned += (bool)*b;
  }
  expect(owned == shim_hip.live.size(), "every live allocation has its owner in the handle (" + std::to_string(owned) + " of " + std::to_string(shim_hip.live.size()) + ")");
}

// which tick entry is taken: smx_step_mixed with a table, the uniform ones without (no HIP call in any of it)
static void check_entries(World& w, bool bound) {
  smx_handle h = w.h;
  int8_t lane[1];
  float floats[1];
  double traj[1];
  int32_t counts[1];
  for (const char* name : {"smx_step", "smx_step_continuous", "smx_step_trajectory", "smx_step_target_pose", "smx_step_trajectory_with_time",
                           "smx_step_history_agents", "smx_step_history_handover"}) {
    const int rc = check_step_entry(h, name, nullptr, false);
    if (bound)
      expect(rc == SMX_ERR_STATE && contains(h->err, name) && contains(h->err, "smx_step_mixed"), std::string(name) + " is refused while a table is bound: " + h->err);
    else
      expect(rc == SMX_OK, std::string(name) + " is taken without a table");
  }
  const smx_mixed_actions all{lane, floats, traj, counts};
  if (!bound) {
    expect(check_step_entry(h, "smx_step_mixed", &all, true) == SMX_ERR_STATE && contains(h->err, "no table"), "smx_step_mixed without a table: " + h->err);
    expect(check_step_entry(h, "smx_step_mixed", nullptr, true) == SMX_ERR_STATE, "... whatever its argument");
    return;
  }
  // the world's table holds Trajectory and Continuous: their buffers are needed, the Lane one is not
  expect(check_step_entry(h, "smx_step_mixed", &all, true) == SMX_OK, "every buffer given");
  expect(check_step_entry(h, "smx_step_mixed", nullptr, true) == SMX_ERR_INVALID, "a null argument");
  smx_mixed_actions a = all;
  a.lane_dev = nullptr;
  expect(check_step_entry(h, "smx_step_mixed", &a, true) == SMX_OK, "the buffer of an absent space may be NULL");
  a = all, a.floats_dev = nullptr;
  expect(check_step_entry(h, "smx_step_mixed", &a, true) == SMX_ERR_INVALID && contains(h->err, "floats_dev is NULL"), "a present space's buffer missing: " + h->err);
  a = all, a.trajectories_dev = nullptr;
  expect(check_step_entry(h, "smx_step_mixed", &a, true) == SMX_ERR_INVALID && contains(h->err, "trajectories_dev"), "no trajectories: " + h->err);
  a = all, a.counts_dev = nullptr;
  expect(check_step_entry(h, "smx_step_mixed", &a, true) == SMX_ERR_INVALID && contains(h->err, "counts_dev"), "no counts: " + h->err);
}

struct Step {
  const char* name;
  std::function<int(World&)> call;
  std::function<void(World&)> after;
};

static std::vector<Step> sequence() {
  std::vector<Step> s;
  auto bind = [](World& w) {
    const smx_agent_spaces d = w.table();
    return set_agent_spaces_impl(w.h, &d);
  };
  auto refused = [](World& w, int rc, const char* what) {
    expect(rc == SMX_ERR_STATE && contains(w.h->err, "per-agent action spaces are bound"), std::string(what) + " is refused beside the table: " + w.h->err);
    return rc == SMX_ERR_STATE ? (int)SMX_OK : rc;
  };
  s.push_back({"smx_create", [](World& w) { return create_impl(&w.cfg, 0, &w.h, KERNELS); }, [](World& w) {
                 expect(spaces_none(w.h), "nothing bound");
                 check_entries(w, false);
               }});
  s.push_back({"smx_set_agent_spaces before a map", bind, [](World& w) { expect(spaces_bound(w), "bound without a map"); }});
  s.push_back({"smx_load_map", [](World& w) { return load_map_impl(w.h, &w.map_a.t); }, [](World& w) {
                 expect(w.h->map_loaded && spaces_bound(w), "a new map keeps the table (it names slots, nothing of the map)");
                 check_entries(w, true);
               }});
  s.push_back({"the plan's inputs", [](World&) { return (int)SMX_OK; }, [](World& w) {
                 expect(w.h->spaces.mask == ((1u << SMX_ACTION_SPACE_TRAJECTORY) | (1u << SMX_ACTION_SPACE_CONTINUOUS)) &&
                            w.h->spaces.owner == SMX_ACTION_SPACE_CONTINUOUS,
                        "the mask holds the agents' spaces; the lowest-numbered one owns the social slots");
               }});
  // the kinematic bindings beside the table (each refuses before it reads its argument's tables)
  s.push_back({"smx_set_agent_dims (refused)", [refused](World& w) {
                 smx_agent_dims ad{};
                 ad.dims_host = w.dims.data(), ad.rows = 1;
                 return refused(w, set_agent_dims_impl(w.h, &ad), "smx_set_agent_dims");
               }, [](World& w) { expect(spaces_bound(w) && !w.h->dims.agent, "... and nothing changed"); }});
  s.push_back({"smx_set_history_agents (refused)", [refused](World& w) {
                 smx_history_agents ha{};
                 return refused(w, set_history_agents_impl(w.h, &ha), "smx_set_history_agents");
               }, [](World& w) { expect(spaces_bound(w) && !w.h->history.follow, "... and nothing changed"); }});
  s.push_back({"smx_set_history_handover (refused)", [refused](World& w) {
                 smx_history_handover ho{};
                 return refused(w, set_history_handover_impl(w.h, &ho), "smx_set_history_handover");
               }, [](World& w) { expect(spaces_bound(w) && !w.h->history.handover, "... and nothing changed"); }});
  s.push_back({"smx_set_history_bubbles (refused)", [refused](World& w) {
                 smx_history_bubbles hb{};
                 return refused(w, set_history_bubbles_impl(w.h, &hb), "smx_set_history_bubbles");
               }, [](World& w) { expect(spaces_bound(w) && !w.h->bubble_state, "... and nothing changed"); }});
  s.push_back({"smx_set_agent_spaces (rebind: Lane owns the social slots)", [](World& w) {
                 w.spaces = {SMX_ACTION_SPACE_MPC, SMX_ACTION_SPACE_LANE, SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED};
                 const smx_agent_spaces d = w.table();
                 return set_agent_spaces_impl(w.h, &d);
               }, [](World& w) {
                 expect(spaces_bound(w) && w.h->spaces.owner == SMX_ACTION_SPACE_LANE && w.h->spaces.count[SMX_ACTION_SPACE_LANE] == 1 + SOCIAL,
                        "rebound: the new table, the social slots in the Lane list");
               }});
  s.push_back({"smx_set_agent_spaces (unbind)", [](World& w) { return set_agent_spaces_impl(w.h, nullptr); }, [](World& w) {
                 expect(spaces_none(w.h), "unbound");
                 check_entries(w, false);
               }});
  s.push_back({"smx_set_agent_spaces (unbind again)", [](World& w) { return set_agent_spaces_impl(w.h, nullptr); },
               [](World& w) { expect(spaces_none(w.h), "an unbind of nothing"); }});
  s.push_back({"smx_set_agent_spaces (one space, not cfg's)", [](World& w) {
                 w.spaces = {SMX_ACTION_SPACE_TRAJECTORY, SMX_ACTION_SPACE_TRAJECTORY, SMX_ACTION_SPACE_TRAJECTORY};
                 const smx_agent_spaces d = w.table();
                 return set_agent_spaces_impl(w.h, &d);
               }, [](World& w) { expect(spaces_bound(w) && w.h->spaces.count[SMX_ACTION_SPACE_TRAJECTORY] == N, "every slot in one list"); }});
  s.push_back({"smx_load_map (second)", [](World& w) { return load_map_impl(w.h, &w.map_b.t); },
               [](World& w) { expect(spaces_bound(w), "kept across the second map too"); }});
  s.push_back({"smx_destroy", [](World& w) {
                 destroy_impl(w.h);
                 w.h = nullptr;
                 return (int)SMX_OK;
               }, [](World&) { expect(shim_hip.live.empty() && shim_hip.streams.empty() && shim_hip.events.empty(), "after smx_destroy nothing is live"); }});
  return s;
}

struct Tally {
  long refused = 0, release_points = 0, skipped = 0;
};

static void run(const std::vector<Step>& steps, long fail_at, Tally& tally) {
  shim_hip.reset();
  shim_hip.fail_at = fail_at;
  World w;
  for (const Step& s : steps) {
    context = (fail_at ? "call " + std::to_string(fail_at) + " fails" : std::string("clean")) + ", " + s.name;
    const bool armed = !shim_hip.fired;
    // what a failed bind must leave: the binding that was in place (fill, then commit)
    const void* had_blob = (w.h && w.h->spaces.space) ? w.h->spaces_blob.p : nullptr;
    const std::vector<int32_t> had_spaces = w.spaces;
    int rc = s.call(w);
    if (armed && shim_hip.fired) {
      if (shim_hip.fired_in_release) {
        ++tally.release_points;
        expect(rc == SMX_OK, "a failed release does not fail the call");
      } else {
        ++tally.refused;
        expect(rc == SMX_ERR_HIP, "the call that contained the failed HIP call returns SMX_ERR_HIP, not " + std::to_string(rc));
        check_handle(w.h);
        if (w.h && had_blob && w.h->spaces.space) {
          World before;
          before.h = w.h, before.spaces = had_spaces;
          expect(w.h->spaces_blob.p == had_blob && spaces_bound(before), "a failed call leaves the binding in place as it was");
          before.h = nullptr;
        }
        rc = s.call(w);
        expect(rc == SMX_OK, "repeating the failed call without the fault succeeds (" + std::to_string(rc) + (w.h ? ": " + w.h->err : "") + ")");
      }
    } else {
      expect(rc == SMX_OK, "the call succeeds (" + std::to_string(rc) + (w.h ? ": " + w.h->err : ": " + g_create_err) + ")");
    }
    if (rc != SMX_OK) break;
    check_handle(w.h);
    s.after(w);
  }
  if (w.h) destroy_impl(w.h);
  context = fail_at ? "call " + std::to_string(fail_at) + " fails, at the end" : "clean, at the end";
  if (fail_at && !shim_hip.fired) ++tally.skipped;
  expect(shim_hip.live.empty() && shim_hip.streams.empty() && shim_hip.events.empty(), "nothing is live at the end");
  expect(shim_hip.misuse == 0, "no HIP call was given a pointer that is not live");
}

// a refused table through the handle: the binding in place stays
static void handle_refusals() {
  context = "handle refusals";
  shim_hip.reset();
  World w;
  expect(create_impl(&w.cfg, 0, &w.h, KERNELS) == SMX_OK, "create");
  const smx_agent_spaces good = w.table();
  expect(set_agent_spaces_impl(w.h, &good) == SMX_OK && spaces_bound(w), "bind");
  const void* blob = w.h->spaces_blob.p;
  std::vector<int32_t> bad = w.spaces;
  bad[1] = SMX_ACTION_SPACE_IMITATION;
  smx_agent_spaces kin = good;
  kin.space_host = bad.data();
  expect(set_agent_spaces_impl(w.h, &kin) == SMX_ERR_INVALID && contains(w.h->err, "slot 1") && contains(w.h->err, "Imitation"), "refused with a reason: " + w.h->err);
  expect(w.h->spaces_blob.p == blob && spaces_bound(w), "... and the binding in place stays");
  expect(set_agent_spaces_impl(nullptr, &good) == SMX_ERR_INVALID, "a null handle");
  destroy_impl(w.h);
  // a kinematic configuration takes no table (so the kinematic bindings and a table never meet)
  World k;
  k.cfg = config(SMX_ACTION_SPACE_IMITATION);
  expect(create_impl(&k.cfg, 0, &k.h, KERNELS) == SMX_OK, "create (Imitation)");
  const smx_agent_spaces t = k.table();
  expect(set_agent_spaces_impl(k.h, &t) == SMX_ERR_INVALID && contains(k.h->err, "cfg.action_space is Imitation") && spaces_none(k.h), "refused: " + k.h->err);
  destroy_impl(k.h);
  expect(shim_hip.live.empty(), "nothing is live");
}

int main() {
  check_refusals();
  handle_refusals();
  const std::vector<Step> steps = sequence();
  Tally clean_tally, tally;
  run(steps, 0, clean_tally);
  const ShimHip clean = shim_hip;
  long points = 0;
  for (long n = 1; n <= clean.calls; ++n, ++points) run(steps, n, tally);
  context = "sweep";
  expect(points == clean.calls, "one sweep point for every HIP call of the clean run");
  expect(tally.skipped == 0 && tally.refused + tally.release_points == points, "every point's fault fired");
  if (failures) return 1;
  std::printf("{\"checks\": %d, \"steps\": %d, \"hip_calls\": %ld, \"sweep_points\": %ld, \"refused\": %ld, \"release_points\": %ld, \"skipped\": %ld, "
              "\"mallocs\": %ld, \"frees\": %ld}\n",
              checks, (int)steps.size(), clean.calls, points, tally.refused, tally.release_points, tally.skipped, clean.mallocs, clean.frees);
  return 0;
}

// Stand-alone host program over the device-free pieces of the history agents (tests/test_host_history_agents.py builds it
// with -fsanitize=address,undefined and runs it): the validation behind smx_set_history_agents / smx_check_history_agents
// (smarts_amd/csrc/smx_host.h) and what the kernels ask of the follow table (smarts_amd/csrc/smx_history.h: the followed id,
// its slot in a frame, the hidden twin inside the presence rule), over heap tables of exactly the stated size — an index
// one past any of them is an AddressSanitizer report.  Prints one JSON line and returns 0 when every check held, else
// prints the failed checks and returns 1.
#include <hip/hip_runtime.h>  // the shim: plain C++

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "smx_history.h"
#include "smx_host.h"

static int failures = 0, checks = 0;
static void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    std::printf("FAILED: %s\n", what.c_str());
  }
}
static bool contains(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }

// Heap tables of exactly the stated size.  Slot s holds vehicle 10 s + k / 4 in the frames whose k % 4 != 3.
struct Tables {
  int n_frames, num_social, rows, num_envs, agents;
  int32_t* vehicle;
  int32_t* start;
  int32_t* replaced;
  int32_t* follow;
  Tables(int F, int S, int R, int E, int A) : n_frames(F), num_social(S), rows(R), num_envs(E), agents(A) {
    vehicle = new int32_t[(size_t)F * S];
    start = new int32_t[(size_t)R * E];
    replaced = new int32_t[(size_t)R * E];
    follow = new int32_t[(size_t)R * E * A];
    for (int k = 0; k < F; ++k)
      for (int s = 0; s < S; ++s) vehicle[(size_t)k * S + s] = k % 4 != 3 ? 10 * s + k / 4 : -1;
    for (int i = 0; i < R * E; ++i) start[i] = 0, replaced[i] = -1;
    for (int i = 0; i < R * E * A; ++i) follow[i] = -1;
  }
  ~Tables() {
    delete[] vehicle;
    delete[] start;
    delete[] replaced;
    delete[] follow;
  }
  Tables(const Tables&) = delete;
  int32_t& followed(int row, int env, int agent) { return follow[((size_t)row * num_envs + env) * agents + agent]; }
  HistoryDev dev(bool with_replaced, bool with_follow) const {
    HistoryDev d{};
    d.vehicle = vehicle, d.start_frame = start, d.replaced = with_replaced ? replaced : nullptr;
    d.n_frames = n_frames, d.num_social = num_social, d.rows = rows, d.num_envs = num_envs;
    d.follow = with_follow ? follow : nullptr, d.n_agents = with_follow ? agents : 0;
    return d;
  }
};

static smx_config config(int E, int N, int S, int space = SMX_ACTION_SPACE_IMITATION) {
  smx_config c{};
  c.num_envs = E, c.num_vehicles = N, c.dt = 0.1, c.num_social = S, c.action_space = space;
  return c;
}

static int check(const smx_config& c, int rows, const smx_history_agents& ha, std::string& why) {
  why.clear();
  return check_history_agents_impl(c, rows, ha, why);
}

int main() {
  const int F = 13, S = 3, R = 2, E = 4, A = 2, N = A + S;
  std::string why;

  // ---- the check
  {
    const smx_config c = config(E, N, S);
    int32_t v[1];
    float act[1];
    uint8_t st[1];  // (never dereferenced by the check: only the counts are read)
    smx_history_agents ok{};
    ok.vehicle_dev = v, ok.vehicle_count = (uint64_t)R * E * A;
    expect(check(c, R, ok, why) == SMX_OK && why.empty(), "the table alone passes: " + why);
    smx_history_agents ha = ok;
    ha.action_dev = act, ha.action_count = 3ull * E * N, ha.status_dev = st, ha.status_count = (uint64_t)E * N;
    expect(check(c, R, ha, why) == SMX_OK, "with both rows: " + why);
    ha.vehicle_count = (uint64_t)R * E * A - 1;
    expect(check(c, R, ha, why) == SMX_ERR_INVALID && contains(why, "vehicle") && contains(why, std::to_string(R * E * A)), "a short table: " + why);
    ha.vehicle_count = 0;
    expect(check(c, R, ha, why) == SMX_ERR_INVALID, "an empty table");
    ha = ok, ha.vehicle_dev = nullptr;
    expect(check(c, R, ha, why) == SMX_ERR_INVALID && contains(why, "vehicle_dev"), "no table: " + why);
    ha = ok, ha.action_dev = act, ha.action_count = 3ull * E * N - 1;
    expect(check(c, R, ha, why) == SMX_ERR_INVALID && contains(why, "action"), "a short action row: " + why);
    ha.action_count = 3ull * E * N;
    expect(check(c, R, ha, why) == SMX_OK, "... and the exact one: " + why);
    ha = ok, ha.status_dev = st, ha.status_count = (uint64_t)E * N - 1;
    expect(check(c, R, ha, why) == SMX_ERR_INVALID && contains(why, "status"), "a short status row: " + why);
    ha = ok, ha.action_count = 0, ha.status_count = 0;  // (counts of rows that are not given are not read)
    expect(check(c, R, ha, why) == SMX_OK, "NULL rows need no count: " + why);
    // a table sized for one row of episodes against a history of R
    ha = ok, ha.vehicle_count = (uint64_t)E * A;
    expect(check(c, R, ha, why) == SMX_ERR_INVALID && check(c, 1, ha, why) == SMX_OK, "the history's rows decide the size");
    expect(check(c, 0, ok, why) == SMX_ERR_INVALID && check(c, -3, ok, why) == SMX_ERR_INVALID, "rows < 1");
    // the action space: Imitation alone
    for (int space = 0; space <= SMX_ACTION_SPACE_IMITATION + 1; ++space) {
      const int rc = check(config(E, N, S, space), R, ok, why);
      expect((rc == SMX_OK) == (space == SMX_ACTION_SPACE_IMITATION), "action space " + std::to_string(space) + ": " + why);
      if (rc != SMX_OK) expect(rc == SMX_ERR_INVALID && contains(why, "action_space") && contains(why, "IMITATION"), "... with the reason: " + why);
    }
    expect(check(config(E, N, 0), R, ok, why) == SMX_ERR_INVALID, "no social slots");
    expect(check(config(E, S, S), R, ok, why) == SMX_ERR_INVALID && contains(why, "agent"), "no agent slot: " + why);
    expect(check(config(0, N, S), R, ok, why) == SMX_ERR_INVALID && check(config(E, 0, 0), R, ok, why) == SMX_ERR_INVALID, "an empty batch");
    // sizes near 2^31 elements do not wrap
    smx_config big = config(1 << 20, 64, 1);
    ha = ok, ha.vehicle_count = (uint64_t)R * (1ull << 20) * 63 - 1;
    expect(check(big, R, ha, why) == SMX_ERR_INVALID, "a large batch, one element short");
    ha.vehicle_count += 1;
    expect(check(big, R, ha, why) == SMX_OK, "... and exact: " + why);
  }

  // ---- the follow table on the device's side
  {
    Tables t(F, S, R, E, A);
    t.followed(0, 1, 0) = 10;                 // env 1, episode row 0: agent 0 follows slot 1's first vehicle
    t.followed(0, 1, 1) = 21;                 // ... agent 1 slot 2's second
    t.followed(1, E - 1, A - 1) = 10 * 2 + 3; // the table's last cell
    const HistoryDev d = t.dev(true, true);
    expect(history_followed(d, 0, 1, 0) == 10 && history_followed(d, 0, 1, 1) == 21 && history_followed(d, 0, 0, 0) == -1, "the followed id");
    expect(history_followed(d, 1, E - 1, A - 1) == 23 && history_followed(d, 3, E - 1, A - 1) == 23 && history_followed(d, -1, E - 1, A - 1) == 23,
           "the last cell, through episode mod rows (a negative episode too)");
    // history_find: the slot, or -1 for a frame outside the table, an id that is none, a frame that lacks it
    for (int k = 0; k < F; ++k)
      for (int s = 0; s < S; ++s) {
        const int32_t id = t.vehicle[(size_t)k * S + s];
        if (id >= 0) expect(history_find(d, k, id) == s, "frame " + std::to_string(k) + " holds vehicle " + std::to_string(id));
      }
    expect(history_find(d, 3, 10) == -1 && history_find(d, 4, 10) == -1 && history_find(d, 0, 11) == -1, "frames that lack the vehicle");
    expect(history_find(d, -1, 10) == -1 && history_find(d, F, 10) == -1 && history_find(d, (int64_t)1 << 40, 10) == -1 &&
               history_find(d, std::numeric_limits<int64_t>::min(), 10) == -1,
           "frames outside the table");
    expect(history_find(d, 0, -1) == -1 && history_find(d, 3, -1) == -1 && history_find(d, 0, std::numeric_limits<int32_t>::min()) == -1,
           "no id matches an empty cell");
    expect(history_find(d, F - 1, t.vehicle[(size_t)F * S - 1]) == S - 1, "the table's last cell");

    // the hidden twin: a followed vehicle's slot is absent in its follower's env and episode row, and nowhere else
    int hidden = 0;
    for (int episode = -2; episode < 4; ++episode)
      for (int env = 0; env < E; ++env)
        for (int64_t k = -1; k <= F; ++k)
          for (int s = 0; s < S; ++s) {
            const bool in = k >= 0 && k < F;
            const int32_t id = in ? t.vehicle[(size_t)k * S + s] : -1;
            bool twin = false;
            const int row = ((episode % R) + R) % R;
            for (int a = 0; a < A; ++a) twin = twin || (id >= 0 && t.followed(row, env, a) == id);
            const bool want = id >= 0 && !twin;
            expect(history_present(d, episode, env, k, s) == want,
                   "presence, episode " + std::to_string(episode) + " env " + std::to_string(env) + " frame " + std::to_string((long long)k) + " slot " + std::to_string(s));
            hidden += twin;
            // without the binding the rule is what it was
            expect(history_present(t.dev(true, false), episode, env, k, s) == (id >= 0), "... and unbound");
          }
    expect(hidden >= 9, "some twins were hidden: " + std::to_string(hidden));
    // beside `replaced`, which keeps working, with and without its table
    t.replaced[1] = 0;  // env 1 hides vehicle 0 (slot 0) in episode row 0
    expect(!history_present(t.dev(true, true), 0, 1, 0, 0) && !history_present(t.dev(true, true), 0, 1, 0, 1) && history_present(t.dev(true, true), 0, 1, 0, 2),
           "replaced and followed, both hidden");
    expect(history_present(t.dev(false, true), 0, 1, 0, 0) && !history_present(t.dev(false, true), 0, 1, 0, 1), "followed without a replaced table");
    // any value in the table is safe: ids are only compared
    for (int i = 0; i < R * E * A; ++i) t.follow[i] = (i % 2) ? std::numeric_limits<int32_t>::max() : std::numeric_limits<int32_t>::min();
    expect(history_present(t.dev(true, true), 0, 0, 0, 1) && history_find(t.dev(true, true), 0, history_followed(t.dev(true, true), 0, 0, 1)) == -1,
           "the ends of int32");
  }

  if (failures) return 1;
  std::printf("{\"checks\": %d, \"frames\": 13, \"slots\": 3}\n", checks);
  return 0;
}

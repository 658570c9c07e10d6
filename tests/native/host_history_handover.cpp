// Stand-alone host program over the device-free pieces of the handover of history agents
// (tests/test_host_history_handover.py builds it with -fsanitize=address,undefined and runs it): the validation behind
// smx_set_history_handover / smx_check_history_handover (smarts_amd/csrc/smx_host.h) and what k_control_kinematic's HANDOVER
// form asks of the table (smarts_amd/csrc/smx_history.h: history_handover, indexed as history_followed is, and the
// driven / follow decision), over heap tables of exactly the stated size — an index one past either of them is an
// AddressSanitizer report.  Prints one JSON line and returns 0 when every check held, else prints the failed checks
// and returns 1.
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

static smx_config config(int E, int N, int S) {
  smx_config c{};
  c.num_envs = E, c.num_vehicles = N, c.dt = 0.1, c.num_social = S, c.action_space = SMX_ACTION_SPACE_IMITATION;
  return c;
}

static int check(const smx_config& c, int rows, const smx_history_handover& ho, std::string& why) {
  why.clear();
  return check_history_handover_impl(c, rows, ho, why);
}

// the value cell (row, env, agent) holds: distinct in every cell, both signs, so that a wrong index is a wrong value
static int32_t cell_value(int row, int env, int agent, int E, int A) { return ((row * E + env) * A + agent) * 3 - 7; }

// The two tables of one shape on the heap, exactly rows * E * A elements each, and every question the kernel asks.
static void walk(int R, int E, int A) {
  const std::string shape = std::to_string(R) + " x " + std::to_string(E) + " x " + std::to_string(A);
  int32_t* follow = new int32_t[(size_t)R * E * A];
  int32_t* handover = new int32_t[(size_t)R * E * A];
  for (int r = 0; r < R; ++r)
    for (int e = 0; e < E; ++e)
      for (int a = 0; a < A; ++a) {
        follow[((size_t)r * E + e) * A + a] = 1000 + cell_value(r, e, a, E, A);
        handover[((size_t)r * E + e) * A + a] = cell_value(r, e, a, E, A);
      }
  HistoryDev d{};
  d.rows = R, d.num_envs = E, d.n_agents = A;
  d.follow = follow, d.handover = handover;
  for (int episode = -2 * R - 1; episode <= 2 * R + 1; ++episode) {
    const int row = ((episode % R) + R) % R;
    for (int e = 0; e < E; ++e)
      for (int a = 0; a < A; ++a) {
        const int32_t want = cell_value(row, e, a, E, A);
        const int32_t h = history_handover(d, episode, e, a);
        expect(h == want, shape + ": the handover tick of episode " + std::to_string(episode) + " env " + std::to_string(e) + " agent " + std::to_string(a));
        expect(history_followed(d, episode, e, a) == 1000 + h, shape + ": ... at the follow table's own index");
        for (int t = -1; t <= (want < 0 ? 3 : want + 2); ++t)
          expect(history_driven(h, t) == (want >= 0 && t >= want), shape + ": driven at tick " + std::to_string(t) + " with H = " + std::to_string(want));
      }
  }
  delete[] follow;
  delete[] handover;
}

int main() {
  const int S = 3, R = 2, E = 4, A = 2, N = A + S;
  std::string why;

  // ---- the check
  {
    const smx_config c = config(E, N, S);
    int32_t t[1];  // (never dereferenced by the check: only the count is read)
    smx_history_handover ok{};
    ok.tick_dev = t, ok.tick_count = (uint64_t)R * E * A;
    expect(check(c, R, ok, why) == SMX_OK && why.empty(), "the exact table passes: " + why);
    smx_history_handover ho = ok;
    ho.tick_count = (uint64_t)R * E * A + 5;
    expect(check(c, R, ho, why) == SMX_OK, "a longer one too: " + why);
    ho.tick_count = (uint64_t)R * E * A - 1;
    expect(check(c, R, ho, why) == SMX_ERR_INVALID && contains(why, "tick") && contains(why, std::to_string(R * E * A)), "a short table: " + why);
    ho.tick_count = 0;
    expect(check(c, R, ho, why) == SMX_ERR_INVALID, "an empty table");
    ho = ok, ho.tick_dev = nullptr;
    expect(check(c, R, ho, why) == SMX_ERR_INVALID && contains(why, "tick_dev"), "no table: " + why);
    ho = ok, ho.tick_count = (uint64_t)E * A;
    expect(check(c, R, ho, why) == SMX_ERR_INVALID && check(c, 1, ho, why) == SMX_OK, "the history's rows decide the size");
    expect(check(c, 0, ok, why) == SMX_ERR_INVALID && check(c, -3, ok, why) == SMX_ERR_INVALID, "rows < 1");
    expect(check(config(E, N, 0), R, ok, why) == SMX_ERR_INVALID, "no social slots");
    expect(check(config(E, S, S), R, ok, why) == SMX_ERR_INVALID && contains(why, "agent"), "no agent slot: " + why);
    expect(check(config(0, N, S), R, ok, why) == SMX_ERR_INVALID && check(config(E, 0, 0), R, ok, why) == SMX_ERR_INVALID, "an empty batch");
    // sizes near 2^31 elements do not wrap
    smx_config big = config(1 << 20, 64, 1);
    ho = ok, ho.tick_count = (uint64_t)R * (1ull << 20) * 63 - 1;
    expect(check(big, R, ho, why) == SMX_ERR_INVALID, "a large batch, one element short");
    ho.tick_count += 1;
    expect(check(big, R, ho, why) == SMX_OK, "... and exact: " + why);
  }

  // ---- the table on the device's side: every episode (negative included), env and agent of small shapes
  walk(1, 1, 1);
  walk(1, 3, 2);
  walk(2, 4, 3);
  walk(3, 2, 5);
  walk(5, 1, 1);

  // ---- the decision: stateless, any value is safe
  {
    const int32_t lo = std::numeric_limits<int32_t>::min(), hi = std::numeric_limits<int32_t>::max();
    expect(history_driven(0, 0) && history_driven(0, 1) && history_driven(0, hi), "H = 0 drives from the first tick after the reset");
    expect(!history_driven(-1, 0) && !history_driven(-1, hi) && !history_driven(lo, 0) && !history_driven(lo, hi), "H < 0 never drives");
    expect(!history_driven(5, 4) && history_driven(5, 5) && history_driven(5, 6), "driven from tick H on");
    expect(!history_driven(hi, hi - 1) && history_driven(hi, hi), "the largest tick");
    expect(!history_driven(3, -1) && !history_driven(0, -1) && !history_driven(0, lo), "a negative tick count drives nobody");
  }

  if (failures) return 1;
  std::printf("{\"checks\": %d, \"shapes\": 5}\n", checks);
  return 0;
}

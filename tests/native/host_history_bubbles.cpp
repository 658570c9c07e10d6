// Stand-alone host program over the device-free pieces of the bubbles (tests/test_host_history_bubbles.py builds it with
// -fsanitize=address,undefined and runs it):
//   (a) the rule, smarts_amd/csrc/smx_bubbles.h — bubble_zone, bubble_recurrence (admissibility, transition, cursor state)
//       and bubble_apply — in a serial loop over the cases of tests/golden/bubble_cursors.npz, which the runner hands over
//       as a text file (argv[1]): every state, cursor mask, transition and cursor state the reference's own code gave;
//   (b) the validation behind smx_set_history_bubbles / smx_check_history_bubbles (smx_host.h), refusal by refusal;
//   (c) the handle's bind / unbind / drop paths (smx_handle.h) over shim/hip_memory.h, then the same sequence once for every
//       HIP call of the clean run with that call failing: the ABI call returns SMX_ERR_HIP, the binding it would have
//       replaced is whole or gone — never half —, and repeating the call succeeds.
// Prints one JSON line and returns 0 when every check held, else prints the failed checks and returns 1.
#include <hip_memory.h>  // the stand-in (and through it the shim <hip/hip_runtime.h>): plain C++

#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "smx_bubbles.h"
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

// ---- (a) the fixture ------------------------------------------------------------------------------------------------
static bool read_int(FILE* f, long& v) { return std::fscanf(f, "%ld", &v) == 1; }
static bool read_double(FILE* f, double& v) { return std::fscanf(f, "%lf", &v) == 1; }

static int walk_fixture(const char* path, long& ticks_seen) {
  FILE* f = std::fopen(path, "r");
  if (!f) {
    std::printf("cannot open %s\n", path);
    return -1;
  }
  long n_cases = 0;
  if (!read_int(f, n_cases)) n_cases = 0;
  int cases = 0;
  for (long c = 0; c < n_cases; ++c) {
    char name[128];
    long A = 0, nb = 0, T = 0;
    if (std::fscanf(f, "%127s", name) != 1 || !read_int(f, A) || !read_int(f, nb) || !read_int(f, T)) break;
    expect(A >= 1 && A <= 64 && nb >= 1 && nb <= SMX_MAX_BUBBLES, std::string(name) + ": a case the device could be given");
    if (A < 1 || A > 64 || nb < 1 || nb > SMX_MAX_BUBBLES) break;
    std::vector<smx_bubble> bubbles((size_t)nb);
    for (smx_bubble& b : bubbles) {
      double v[10];
      for (double& x : v) read_double(f, x);
      b = smx_bubble{v[0], v[1], v[2], v[3], v[4], v[5], v[6], (int32_t)v[7], (int32_t)v[8], (int32_t)v[9]};
    }
    // exactly A elements each, on the heap: an index past an env's agents is an AddressSanitizer report
    std::vector<double> px((size_t)A), py((size_t)A), heading((size_t)A);
    std::vector<long> alive((size_t)A), ego((size_t)A), want_state((size_t)A), want_mask((size_t)A), want_trans((size_t)(A * nb)), want_cur((size_t)(A * nb));
    std::vector<int> state((size_t)A, SMX_BUBBLE_SOCIAL);
    std::vector<unsigned> mask((size_t)A, 0u);
    for (long t = 0; t < T; ++t) {
      context = std::string(name) + " tick " + std::to_string(t);
      for (long a = 0; a < A; ++a) read_double(f, px[a]), read_double(f, py[a]);
      for (double& h : heading) read_double(f, h);
      for (long& v : alive) read_int(f, v);
      for (long& v : ego) read_int(f, v);
      for (long& v : want_state) read_int(f, v);
      for (long& v : want_mask) read_int(f, v);
      for (long& v : want_trans) read_int(f, v);
      for (long& v : want_cur) read_int(f, v);
      // k_bubbles, serially: the masks of the state bytes as the pass found them, then bubble by bubble
      uint64_t alive_m = 0, social_m = 0, shadowed_m = 0, hijacked_m = 0;
      for (long a = 0; a < A; ++a) {
        const uint64_t me = (uint64_t)1 << a;
        if (!alive[a]) continue;
        alive_m |= me;
        const int seen = ego[a] ? (int)SMX_BUBBLE_EGO : state[a];
        if (seen == SMX_BUBBLE_SOCIAL) social_m |= me;
        if (seen == SMX_BUBBLE_SHADOWED) shadowed_m |= me;
        if (seen == SMX_BUBBLE_HIJACKED) hijacked_m |= me;
      }
      std::vector<unsigned> now((size_t)A, 0u);
      std::vector<int> applied(state);
      for (long b = 0; b < nb; ++b) {
        const smx_bubble& bb = bubbles[b];
        const int fo = bb.follow_agent;
        const bool active = fo < 0 || ((alive_m >> fo) & 1);
        BubbleResult r = {0, 0, 0, 0, 0};
        if (active) {
          BubbleMasks m = {alive_m, social_m, shadowed_m, hijacked_m, 0, 0, 0};
          for (long a = 0; a < A; ++a) {
            const uint64_t me = (uint64_t)1 << a;
            if ((mask[a] >> b) & 1u) m.was_in |= me;
            if (!alive[a]) continue;
            const BubbleZone z = bubble_zone(bb, px[a], py[a], fo >= 0 ? px[fo] : 0.0, fo >= 0 ? py[fo] : 0.0, fo >= 0 ? heading[fo] : 0.0);
            if (z.in_bubble) m.in_bubble |= me;
            if (z.in_airlock) m.in_airlock |= me;
          }
          r = bubble_recurrence(m, (int)A, bb.hijack_limit, bb.shadow_limit);
        }
        for (long a = 0; a < A; ++a) {
          const long cur = ((r.cur_bubble >> a) & 1) ? SMX_BC_IN_BUBBLE : ((r.cur_airlock >> a) & 1) ? SMX_BC_IN_AIRLOCK : SMX_BC_NONE;
          const BubbleTransition tr = bubble_transition_of(r, (int)a);
          expect(cur == want_cur[a * nb + b], "cursor state of agent " + std::to_string(a) + " at bubble " + std::to_string(b));
          // (Exited changes nothing and is not kept by bubble_transition_of: the fixture's 3 reads as none here)
          const long want = want_trans[a * nb + b] == SMX_BT_EXITED ? (long)SMX_BT_NONE : want_trans[a * nb + b];
          expect((long)tr == want, "transition of agent " + std::to_string(a) + " at bubble " + std::to_string(b));
          if (cur != SMX_BC_NONE) now[a] |= 1u << b;
          applied[a] = bubble_apply(applied[a], tr);
        }
      }
      for (long a = 0; a < A; ++a) {
        state[a] = applied[a];
        mask[a] = now[a];
        expect(state[a] == want_state[a] && (long)mask[a] == want_mask[a], "state and cursor mask of agent " + std::to_string(a));
      }
      ++ticks_seen;
    }
    ++cases;
  }
  std::fclose(f);
  return cases;
}

// the functions one by one, at and around the edges
static void edges() {
  context = "edges";
  const smx_bubble fixed{10.0, 20.0, 8.0, 4.0, 2.0, 0.0, 0.0, -1, 0, 0};
  auto at = [&](double x, double y) { return bubble_zone(fixed, x, y, 0.0, 0.0, 0.0); };
  expect(at(10.0, 20.0).in_bubble && !at(10.0, 20.0).in_airlock, "the centre is inside");
  expect(!at(14.0, 20.0).in_bubble && at(14.0, 20.0).in_airlock, "the inner boundary is outside the inner zone (strict), in the airlock");
  expect(!at(16.0, 20.0).in_bubble && !at(16.0, 20.0).in_airlock, "the airlock's boundary is outside");
  expect(at(std::nextafter(16.0, 0.0), 20.0).in_airlock && at(10.0, std::nextafter(24.0, 0.0)).in_airlock && !at(10.0, 24.0).in_airlock, "... and one ulp inside it is in");
  expect(at(15.9, 23.9).in_airlock, "the airlock is a rectangle: its corner region is in (mitre join)");
  // a travelling bubble 8 m ahead of an agent at (3, 4) facing west (heading pi / 2): its centre is at (-5, 4)
  const smx_bubble moving{1e9, 1e9, 6.0, 4.0, 2.0, 0.0, 8.0, 0, 0, 0};
  const double west = 1.5707963267948966;
  expect(bubble_zone(moving, -5.0, 4.0, 3.0, 4.0, west).in_bubble && bubble_zone(moving, -5.0, 6.9, 3.0, 4.0, west).in_bubble, "ahead of a west-facing agent: its width lies along y");
  expect(bubble_zone(moving, -7.5, 4.0, 3.0, 4.0, west).in_airlock && !bubble_zone(moving, 3.0, 12.0, 3.0, 4.0, west).in_bubble, "x, y of the bubble are not read; the heading is");
  expect(bubble_zone(moving, 3.0, 12.0, 3.0, 4.0, 0.0).in_bubble, "facing north it is at (3, 12)");
  bool h, s;
  bubble_admissible(0, 0, 0, 0, h, s);
  expect(h && s, "no limits");
  bubble_admissible(1000, 1000, 0, 0, h, s);
  expect(h && s, "0 = none, whatever the counts");
  bubble_admissible(1, 0, 1, 2, h, s);
  expect(!h && s, "hijack limit reached, room to shadow");
  bubble_admissible(1, 1, 2, 2, h, s);
  expect(h && !s, "the shadow limit counts both sets");
  const BubbleZone in{true, false}, ring{false, true}, out{false, false};
  expect(bubble_transition(SMX_BUBBLE_SOCIAL, false, ring, true, true) == SMX_BT_AIRLOCK_ENTERED && bubble_transition(SMX_BUBBLE_SOCIAL, false, ring, true, false) == SMX_BT_NONE, "rule 1");
  expect(bubble_transition(SMX_BUBBLE_SOCIAL, false, in, true, true) == SMX_BT_NONE, "a vehicle that appears inside is not captured");
  expect(bubble_transition(SMX_BUBBLE_SHADOWED, true, in, true, true) == SMX_BT_ENTERED && bubble_transition(SMX_BUBBLE_SHADOWED, true, in, false, true) == SMX_BT_NONE, "rule 2");
  expect(bubble_transition(SMX_BUBBLE_HIJACKED, true, ring, false, false) == SMX_BT_EXITED, "rule 3 asks no limit");
  expect(bubble_transition(SMX_BUBBLE_HIJACKED, true, out, true, true) == SMX_BT_AIRLOCK_EXITED && bubble_transition(SMX_BUBBLE_SHADOWED, true, out, true, true) == SMX_BT_AIRLOCK_EXITED &&
             bubble_transition(SMX_BUBBLE_HIJACKED, false, out, true, true) == SMX_BT_NONE, "rule 4 needs the cursor bit");
  for (int st : {(int)SMX_BUBBLE_RELEASED, (int)SMX_BUBBLE_EGO})
    for (const BubbleZone& z : {in, ring, out}) expect(bubble_transition(st, true, z, true, true) == SMX_BT_NONE, "a released agent and an ego make no transition");
  expect(bubble_cursor(in, true, false) == SMX_BC_IN_BUBBLE && bubble_cursor(in, false, true) == SMX_BC_NONE && bubble_cursor(ring, false, true) == SMX_BC_IN_AIRLOCK &&
             bubble_cursor(ring, true, false) == SMX_BC_NONE && bubble_cursor(out, true, true) == SMX_BC_NONE, "the cursor state");
  expect(bubble_apply(SMX_BUBBLE_SOCIAL, SMX_BT_AIRLOCK_ENTERED) == SMX_BUBBLE_SHADOWED && bubble_apply(SMX_BUBBLE_SHADOWED, SMX_BT_ENTERED) == SMX_BUBBLE_HIJACKED &&
             bubble_apply(SMX_BUBBLE_HIJACKED, SMX_BT_AIRLOCK_EXITED) == SMX_BUBBLE_RELEASED && bubble_apply(SMX_BUBBLE_SHADOWED, SMX_BT_AIRLOCK_EXITED) == SMX_BUBBLE_SOCIAL &&
             bubble_apply(SMX_BUBBLE_HIJACKED, SMX_BT_EXITED) == SMX_BUBBLE_HIJACKED && bubble_apply(SMX_BUBBLE_RELEASED, SMX_BT_AIRLOCK_ENTERED) == SMX_BUBBLE_RELEASED, "the four state changes");
  // a full env: 64 agents all in the ring of a bubble that shadows 9 — the first nine by slot, no shift past bit 63
  BubbleMasks m = {~(uint64_t)0, ~(uint64_t)0, 0, 0, 0, 0, ~(uint64_t)0};
  const BubbleResult r = bubble_recurrence(m, 64, 5, 9);
  expect(r.airlock_entered == 0x1ff && r.cur_airlock == 0x1ff && r.cur_bubble == 0 && r.entered == 0 && r.airlock_exited == 0, "64 lanes: the first nine are shadowed");
  expect(bubble_recurrence(m, 64, 0, 0).airlock_entered == ~(uint64_t)0, "64 lanes, no limits: all of them");
}

// ---- (b) the validation ---------------------------------------------------------------------------------------------
enum { E = 2, N = 3, SOCIAL = 1, AGENTS = N - SOCIAL, TOTAL = E * N, ROWS = 2 };
static smx_config config() {
  smx_config c{};
  c.num_envs = E, c.num_vehicles = N, c.dt = 0.1, c.num_social = SOCIAL, c.social_speed_factor = 1.0;
  c.action_space = SMX_ACTION_SPACE_IMITATION;
  c.sensors = SMX_SENSOR_WAYPOINTS;
  c.wp_lookahead = 32, c.wp_paths = 4, c.wp_len = 20, c.nb_radius = 50.0;
  return c;
}
static const smx_bubble GOOD{1.0, 2.0, 8.0, 4.0, 2.0, 0.0, 8.0, 1, 1, 2};

static void validation() {
  context = "validation";
  const smx_config c = config();
  uint8_t rows[TOTAL];
  auto check = [&](std::vector<smx_bubble> b, std::function<void(smx_history_bubbles&)> edit, const char* word) {
    smx_history_bubbles hb{b.data(), (int32_t)b.size(), rows, rows, TOTAL, TOTAL};
    if (edit) edit(hb);
    std::string why;
    const int rc = check_history_bubbles_impl(c, hb, why);
    if (word)
      expect(rc == SMX_ERR_INVALID && contains(why, word), std::string("refused with '") + word + "': " + why);
    else
      expect(rc == SMX_OK && why.empty(), "accepted: " + why);
  };
  auto with = [](std::function<void(smx_bubble&)> edit) {
    smx_bubble b = GOOD;
    edit(b);
    return std::vector<smx_bubble>{GOOD, b};
  };
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  check({GOOD}, nullptr, nullptr);
  check(std::vector<smx_bubble>(SMX_MAX_BUBBLES, GOOD), nullptr, nullptr);
  check(with([](smx_bubble& b) { b.follow_agent = -1, b.hijack_limit = 0, b.shadow_limit = 0; }), nullptr, nullptr);
  check(with([](smx_bubble& b) { b.hijack_limit = 0, b.shadow_limit = 1; }), nullptr, nullptr);
  check({GOOD}, [](smx_history_bubbles& hb) { hb.n_bubbles = 0; }, "n_bubbles");
  check(std::vector<smx_bubble>(SMX_MAX_BUBBLES, GOOD), [](smx_history_bubbles& hb) { hb.n_bubbles = SMX_MAX_BUBBLES + 1; }, "n_bubbles");  // (refused before element 8 is read)
  check({GOOD}, [](smx_history_bubbles& hb) { hb.bubbles_host = nullptr; }, "bubbles_host");
  check(with([&](smx_bubble& b) { b.x = nan; }), nullptr, "not finite");
  check(with([&](smx_bubble& b) { b.offset_y = inf; }), nullptr, "not finite");
  check(with([&](smx_bubble& b) { b.margin = -inf; }), nullptr, "not finite");
  check(with([](smx_bubble& b) { b.size_x = 0.0; }), nullptr, "size");
  check(with([](smx_bubble& b) { b.size_y = -4.0; }), nullptr, "size");
  check(with([](smx_bubble& b) { b.margin = 0.0; }), nullptr, "margin");
  check(with([](smx_bubble& b) { b.follow_agent = AGENTS; }), nullptr, "follow_agent");
  check(with([](smx_bubble& b) { b.hijack_limit = -1; }), nullptr, "negative");
  check(with([](smx_bubble& b) { b.shadow_limit = -1; }), nullptr, "negative");
  check(with([](smx_bubble& b) { b.hijack_limit = 3, b.shadow_limit = 2; }), nullptr, "shadow_limit");
  check({GOOD}, [](smx_history_bubbles& hb) { hb.state_dev = nullptr; }, "NULL");
  check({GOOD}, [](smx_history_bubbles& hb) { hb.cursor_dev = nullptr; }, "NULL");
  check({GOOD}, [](smx_history_bubbles& hb) { hb.state_count = TOTAL - 1; }, "state");
  check({GOOD}, [](smx_history_bubbles& hb) { hb.cursor_count = 0; }, "cursor");
}

// ---- (c) the handle -------------------------------------------------------------------------------------------------
static int fake_knot_table(smx_handle_s* h, KnotRow* table) {
  std::memset(table, 0, (size_t)h->map.n_lanepoints * sizeof(KnotRow));
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}
static const KernelSide KERNELS = {352, 64 * 11 * 36, 0, fake_knot_table};

struct World {
  smx_handle h = nullptr;
  smx_config cfg = config();
  Map map;
  std::vector<double> frames{10.0, 1.0, 0.0, 5.0, /**/ 10.5, 1.0, 0.0, 5.0, /**/ 11.0, 1.0, 0.0, 5.0};  // 3 frames x 1 slot
  std::vector<int32_t> frame_vehicle{4, 4, -1}, start_frame = std::vector<int32_t>(ROWS * E, 0);
  std::vector<int32_t> follow = std::vector<int32_t>(ROWS * E * AGENTS, 4), handover = std::vector<int32_t>(ROWS * E * AGENTS, -1);
  std::vector<uint8_t> state = std::vector<uint8_t>(TOTAL), cursor = std::vector<uint8_t>(TOTAL), state2 = std::vector<uint8_t>(TOTAL);
  std::vector<smx_bubble> bubbles{GOOD, GOOD, GOOD};
};
struct Step {
  const char* name;
  std::function<int(World&)> call;
  std::function<void(World&)> after;
};
static bool bubbles_bound(const World& w, int n, const uint8_t* state) {
  const smx_handle_s* h = w.h;
  bool same = h->bubbles.n == n && h->bubble_state == state && h->bubble_cursor == w.cursor.data();
  for (int i = 0; same && i < n; ++i) same = std::memcmp(&h->bubbles.b[i], &w.bubbles[i], sizeof(smx_bubble)) == 0;
  return same;
}
static bool bubbles_gone(const smx_handle_s* h) { return h->bubbles.n == 0 && !h->bubble_state && !h->bubble_cursor; }
// whole or gone, never half: what every call, failed or not, leaves
static void check_handle(const World& w) {
  if (!w.h) return;
  const smx_handle_s* h = w.h;
  expect(bubbles_gone(h) || (h->bubbles.n >= 1 && h->bubbles.n <= SMX_MAX_BUBBLES && h->bubble_state && h->bubble_cursor), "the bubbles are whole or gone");
  expect(bubbles_gone(h) || h->history.follow, "bubbles only with history agents");
  expect(!h->history.follow || h->history.vehicle, "history agents only with a history");
}

static std::vector<Step> sequence() {
  std::vector<Step> s;
  auto history = [](World& w) {
    smx_social_history hs{};
    hs.frames_host = w.frames.data(), hs.vehicle_host = w.frame_vehicle.data(), hs.n_frames = 3, hs.num_social = SOCIAL;
    hs.start_frame_dev = w.start_frame.data(), hs.rows = ROWS, hs.start_count = w.start_frame.size();
    return set_social_history_impl(w.h, &hs);
  };
  auto agents = [](World& w) {
    smx_history_agents ha{};
    ha.vehicle_dev = w.follow.data(), ha.vehicle_count = w.follow.size();
    return set_history_agents_impl(w.h, &ha);
  };
  auto bind = [](int n, bool second_rows) {
    return [n, second_rows](World& w) {
      smx_history_bubbles hb{w.bubbles.data(), n, second_rows ? w.state2.data() : w.state.data(), w.cursor.data(), TOTAL, TOTAL};
      return set_history_bubbles_impl(w.h, &hb);
    };
  };
  auto bound3 = [](World& w) { expect(bubbles_bound(w, 3, w.state.data()), "three bubbles bound, copied, with the caller's rows"); };
  auto nothing = [](World&) {};
  s.push_back({"smx_create", [](World& w) { return create_impl(&w.cfg, 0, &w.h, KERNELS); }, [](World& w) { expect(w.h && bubbles_gone(w.h), "a new handle has no bubbles"); }});
  s.push_back({"smx_load_map", [](World& w) { return load_map_impl(w.h, &w.map.t); }, nothing});
  s.push_back({"smx_set_history_bubbles (no history)", [bind](World& w) {
                 const int rc = bind(3, false)(w);
                 expect(rc == SMX_ERR_STATE && contains(w.h->err, "needs bound history agents"), "bubbles without history agents: SMX_ERR_STATE");
                 return rc == SMX_ERR_STATE ? (int)SMX_OK : -100;
               }, [](World& w) { expect(bubbles_gone(w.h), "... and nothing bound"); }});
  s.push_back({"smx_set_social_history", history, nothing});
  s.push_back({"smx_set_history_bubbles (no agents)", [bind](World& w) { return bind(3, false)(w) == SMX_ERR_STATE ? (int)SMX_OK : -100; }, [](World& w) { expect(bubbles_gone(w.h), "a history alone does not do"); }});
  s.push_back({"smx_set_history_agents", agents, [](World& w) { expect(bubbles_gone(w.h) && w.h->history.follow, "agents bound, no bubbles yet"); }});
  s.push_back({"smx_set_history_bubbles", bind(3, false), bound3});
  s.push_back({"smx_set_history_bubbles (refused)", [](World& w) {
                 smx_bubble bad = GOOD;
                 bad.margin = 0.0;
                 smx_history_bubbles hb{&bad, 1, w.state2.data(), w.cursor.data(), TOTAL, TOTAL};
                 const int rc = set_history_bubbles_impl(w.h, &hb);
                 expect(rc == SMX_ERR_INVALID && contains(w.h->err, "margin"), "a refused binding says why");
                 return rc == SMX_ERR_INVALID ? (int)SMX_OK : -100;
               }, bound3});  // (... and leaves the binding it would have replaced)
  s.push_back({"smx_set_history_bubbles (again: one bubble, other rows)", bind(1, true), [](World& w) {
                 expect(bubbles_bound(w, 1, w.state2.data()), "a second binding replaces the first");
                 expect(w.h->bubbles.b[1].size_x == 0.0 && w.h->bubbles.b[2].margin == 0.0, "... and nothing of the first is left behind the new count");
               }});
  s.push_back({"smx_set_history_handover", [](World& w) {
                 const smx_history_handover ho{w.handover.data(), w.handover.size()};
                 return set_history_handover_impl(w.h, &ho);
               }, [](World& w) { expect(bubbles_bound(w, 1, w.state2.data()) && w.h->history.handover, "a handover table beside the bubbles: both bound"); }});
  s.push_back({"smx_set_history_handover (unbind)", [](World& w) { return set_history_handover_impl(w.h, nullptr); }, [](World& w) { expect(bubbles_bound(w, 1, w.state2.data()) && !w.h->history.handover, "... and the table goes alone"); }});
  s.push_back({"smx_set_history_bubbles (unbind)", [](World& w) { return set_history_bubbles_impl(w.h, nullptr); }, [](World& w) { expect(bubbles_gone(w.h) && w.h->history.follow, "NULL unbinds the bubbles alone"); }});
  s.push_back({"smx_set_history_bubbles (third)", bind(3, false), bound3});
  s.push_back({"smx_set_history_agents (again)", agents, [](World& w) { expect(bubbles_gone(w.h) && w.h->history.follow, "a new follow table drops the bubbles"); }});
  s.push_back({"smx_set_history_bubbles (fourth)", bind(3, false), bound3});
  s.push_back({"smx_set_history_agents (unbind)", [](World& w) { return set_history_agents_impl(w.h, nullptr); }, [](World& w) { expect(bubbles_gone(w.h) && !w.h->history.follow, "unbinding the agents drops the bubbles"); }});
  s.push_back({"smx_set_history_agents (third)", agents, nothing});
  s.push_back({"smx_set_history_bubbles (fifth)", bind(3, false), bound3});
  s.push_back({"smx_set_social_history (again)", history, [](World& w) { expect(bubbles_gone(w.h) && !w.h->history.follow, "a new history drops the agents and the bubbles"); }});
  s.push_back({"smx_set_history_agents (fourth)", agents, nothing});
  s.push_back({"smx_set_history_bubbles (sixth)", bind(3, false), bound3});
  s.push_back({"smx_set_social_history (unbind)", [](World& w) { return set_social_history_impl(w.h, nullptr); }, [](World& w) { expect(bubbles_gone(w.h), "unbinding the history drops the bubbles"); }});
  s.push_back({"smx_set_social_history (third)", history, nothing});
  s.push_back({"smx_set_history_agents (fifth)", agents, nothing});
  s.push_back({"smx_set_history_bubbles (seventh)", bind(3, false), bound3});
  s.push_back({"smx_load_map (second)", [](World& w) { return load_map_impl(w.h, &w.map.t); }, [](World& w) { expect(bubbles_gone(w.h) && !w.h->history.vehicle, "a new map drops the history and with it the bubbles"); }});
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
    const bool was_bound = w.h && !bubbles_gone(w.h);
    int rc = s.call(w);
    if (armed && shim_hip.fired) {
      if (shim_hip.fired_in_release) {
        ++tally.release_points;
        expect(rc == SMX_OK, "a failed release does not fail the call");
      } else {
        ++tally.refused;
        expect(rc == SMX_ERR_HIP, "the call that contained the failed HIP call returns SMX_ERR_HIP, not " + std::to_string(rc));
        check_handle(w);
        // smx_set_history_bubbles fails before it touches the handle: the old binding, if any, is still whole
        if (w.h && std::string(s.name).find("smx_set_history_bubbles") == 0) expect(was_bound == !bubbles_gone(w.h), "a failed bind leaves the binding as it was");
        rc = s.call(w);
        expect(rc == SMX_OK, "repeating the failed call without the fault succeeds (" + std::to_string(rc) + ")");
      }
    } else {
      expect(rc == SMX_OK, "the call succeeds (" + std::to_string(rc) + (w.h ? ": " + w.h->err : ": " + g_create_err) + ")");
    }
    if (rc != SMX_OK) break;
    check_handle(w);
    s.after(w);
  }
  if (w.h) destroy_impl(w.h);
  context = "at the end";
  if (fail_at && !shim_hip.fired) ++tally.skipped;
  expect(shim_hip.live.empty() && shim_hip.streams.empty() && shim_hip.events.empty(), "nothing is live at the end");
  expect(shim_hip.misuse == 0, "no HIP call was given a pointer that is not live");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: host_history_bubbles <fixture as text>\n");
    return 2;
  }
  long ticks = 0;
  const int cases = walk_fixture(argv[1], ticks);
  edges();
  validation();
  const std::vector<Step> steps = sequence();
  Tally clean_tally, tally;
  run(steps, 0, clean_tally);
  const ShimHip clean = shim_hip;
  long points = 0;
  for (long n = 1; n <= clean.calls; ++n, ++points) run(steps, n, tally);
  context = "sweep";
  expect(tally.skipped == 0 && tally.refused + tally.release_points == points, "every point's fault fired");
  if (failures) return 1;
  std::printf("{\"checks\": %d, \"cases\": %d, \"ticks\": %ld, \"steps\": %d, \"hip_calls\": %ld, \"sweep_points\": %ld, \"refused\": %ld, \"release_points\": %ld, \"skipped\": %ld}\n",
              checks, cases, ticks, (int)steps.size(), clean.calls, points, tally.refused, tally.release_points, tally.skipped);
  return 0;
}

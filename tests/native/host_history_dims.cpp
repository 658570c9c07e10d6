// Stand-alone host program over the two device-free pieces of the per-vehicle dimensions of a replayed history
// (tests/test_host_history_dims.py builds it with -fsanitize=address,undefined and runs it): the validation behind
// smx_set_social_history_dims / smx_check_social_history_dims (smarts_amd/csrc/smx_host.h) and the id -> triple lookup
// the kernels run (smarts_amd/csrc/smx_history.h), over heap tables of exactly the stated size — an index one past any of
// them is an AddressSanitizer report.  Prints one JSON line and returns 0 when every check held, else prints the failed
// checks and returns 1.
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

// Heap tables of exactly the stated size.  Slot s holds vehicle 10 s + k / 4 in frames whose k % 4 != 3; the last frame's
// last slot holds the largest id of the table, TOP.
struct Tables {
  int n_frames, num_social, top;
  int32_t* vehicle;
  double* dims;  // [top + 1][3]
  Tables(int F, int S, int top_id) : n_frames(F), num_social(S), top(top_id) {
    vehicle = new int32_t[(size_t)F * S];
    for (int k = 0; k < F; ++k)
      for (int s = 0; s < S; ++s) vehicle[(size_t)k * S + s] = k % 4 != 3 ? 10 * s + k / 4 : -1;
    vehicle[(size_t)F * S - 1] = top_id;
    dims = new double[((size_t)top_id + 1) * 3];
    for (int id = 0; id <= top_id; ++id) {
      dims[(size_t)id * 3 + 0] = 2.0 + 0.01 * id;
      dims[(size_t)id * 3 + 1] = 1.0 + 0.001 * id;
      dims[(size_t)id * 3 + 2] = 1.5 + 0.0001 * id;
    }
  }
  ~Tables() {
    delete[] vehicle;
    delete[] dims;
  }
  Tables(const Tables&) = delete;
  smx_social_history history() const {
    smx_social_history h{};
    h.vehicle_host = vehicle, h.n_frames = n_frames, h.num_social = num_social;
    return h;
  }
  smx_social_dims abi() const {
    smx_social_dims d{};
    d.dims_host = dims, d.n_ids = top + 1;
    return d;
  }
};

static smx_config config(int S) {
  smx_config c{};
  c.num_envs = 4, c.num_vehicles = S + 2, c.dt = 0.1, c.num_social = S;
  return c;
}

static int check(const smx_config& c, const smx_social_history& h, const smx_social_dims& d, std::string& why) {
  why.clear();
  return check_social_history_dims_impl(c, h, d, why);
}

int main() {
  const int F = 13, S = 3, TOP = 57;
  const smx_config c = config(S);
  std::string why;

  // ---- the check
  {
    Tables t(F, S, TOP);
    expect(social_history_max_id(t.history()) == TOP, "the largest id is found in the last cell");
    expect(check(c, t.history(), t.abi(), why) == SMX_OK && why.empty(), "a good table passes: " + why);
    smx_social_dims d = t.abi();
    for (int bad : {0, -1, std::numeric_limits<int32_t>::min()}) {
      d = t.abi(), d.n_ids = bad;
      expect(check(c, t.history(), d, why) == SMX_ERR_INVALID && contains(why, "n_ids"), "n_ids " + std::to_string(bad) + ": " + why);
    }
    d = t.abi(), d.dims_host = nullptr;
    expect(check(c, t.history(), d, why) == SMX_ERR_INVALID && contains(why, "dims_host"), "no table: " + why);
    // a cell's id at n_ids: refused
    {
      Tables shorter(F, S, TOP);
      d = shorter.abi(), d.n_ids = TOP;  // rows 0 .. TOP - 1
      expect(check(c, shorter.history(), d, why) == SMX_ERR_INVALID && contains(why, "57") && contains(why, "n_ids"), "an id at n_ids: " + why);
      shorter.vehicle[(size_t)F * S - 1] = -1;  // the cell emptied: ids up to 22 remain
      expect(check(c, shorter.history(), d, why) == SMX_OK, "... and with that cell empty the shorter table does: " + why);
      d.n_ids = 23;
      expect(check(c, shorter.history(), d, why) == SMX_OK, "n_ids = max id + 1 is enough: " + why);
      d.n_ids = 22;
      expect(check(c, shorter.history(), d, why) == SMX_ERR_INVALID, "n_ids = max id is not");
    }
    // the history's own shape
    smx_social_history h = t.history();
    h.num_social = S + 1;
    expect(check(c, h, t.abi(), why) == SMX_ERR_INVALID && contains(why, "num_social"), "a wrong slot count: " + why);
    h = t.history(), h.vehicle_host = nullptr;
    expect(check(c, h, t.abi(), why) == SMX_ERR_INVALID, "a history without its id table");
    h = t.history(), h.n_frames = 0;
    expect(check(c, h, t.abi(), why) == SMX_ERR_INVALID, "a history without frames");
  }
  // values: not finite, <= 0, above the caps; the caps themselves are accepted; every row and word is checked
  {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    struct Case {
      int word;
      double value;
      bool ok;
    } cases[] = {{0, nan, false}, {1, nan, false}, {2, nan, false}, {0, inf, false}, {1, -inf, false}, {2, inf, false},
                 {0, 0.0, false}, {1, 0.0, false}, {2, 0.0, false}, {0, -1.0, false}, {1, -0.5, false}, {2, -4.0, false},
                 {0, 25.0, true}, {1, 25.0, true}, {2, 10.0, true}, {0, 25.000001, false}, {1, 25.000001, false},
                 {2, 10.000001, false}, {2, 25.0, false}, {0, 1e-9, true}, {1, 1e-300, true}, {0, 1e300, false}};
    for (int id : {0, 21, TOP})
      for (const Case& k : cases) {
        Tables t(F, S, TOP);
        t.dims[(size_t)id * 3 + k.word] = k.value;
        const int rc = check(c, t.history(), t.abi(), why);
        expect((rc == SMX_OK) == k.ok, "vehicle " + std::to_string(id) + " word " + std::to_string(k.word) + " = " + std::to_string(k.value) + ": " + why);
        if (!k.ok) {
          expect(rc == SMX_ERR_INVALID && contains(why, "vehicle " + std::to_string(id)), "the reason names the vehicle: " + why);
          expect(contains(why, k.word == 0 ? "length" : (k.word == 1 ? "width" : "height")), "... and the word: " + why);
        }
      }
    // an id that never occurs in the history is checked all the same: its row is in the table the device gets
    Tables t(F, S, TOP);
    t.dims[(size_t)40 * 3 + 1] = nan;
    expect(check(c, t.history(), t.abi(), why) == SMX_ERR_INVALID && contains(why, "vehicle 40"), "an unused row: " + why);
    // the handle's own form: the largest id of the bound history, kept from the bind
    expect(check_social_dims_impl(t.abi(), -1, why) == SMX_ERR_INVALID, "(still the NaN)");
    t.dims[(size_t)40 * 3 + 1] = 1.0;
    why.clear();
    expect(check_social_dims_impl(t.abi(), -1, why) == SMX_OK, "a history of empty cells takes any table: " + why);
    expect(check_social_dims_impl(t.abi(), TOP, why) == SMX_OK && check_social_dims_impl(t.abi(), TOP + 1, why) == SMX_ERR_INVALID,
           "max id against n_ids");
  }

  // ---- the lookup: every present cell reads its own vehicle's row, the last frame's last slot the table's last row
  {
    Tables t(F, S, TOP);
    HistoryDev h{};
    h.vehicle = t.vehicle, h.n_frames = F, h.num_social = S, h.rows = 1, h.num_envs = 1;
    HistoryDimsDev d{};
    d.table = t.dims, d.n_ids = TOP + 1;
    int seen = 0;
    for (int64_t k = 0; k < F; ++k)
      for (int s = 0; s < S; ++s) {
        const int32_t id = t.vehicle[(size_t)k * S + s];
        if (id < 0) continue;
        const double* r = history_dims_row(h, d, k, s);
        expect(r == t.dims + (size_t)id * 3 && r[0] == 2.0 + 0.01 * id && r[1] == 1.0 + 0.001 * id && r[2] == 1.5 + 0.0001 * id,
               "the triple of vehicle " + std::to_string(id));
        ++seen;
      }
    expect(seen > 20, "some cells were present");
    const double* last = history_dims_row(h, d, F - 1, S - 1);
    expect(last == t.dims + (size_t)TOP * 3 && last[2] == 1.5 + 0.0001 * TOP, "the largest id reads the last row");
    // an id outside the table (the bind-time check excludes it) reads row 0, never outside
    d.n_ids = 10;
    expect(history_dims_row(h, d, F - 1, S - 1) == t.dims, "an id past n_ids reads row 0");
    expect(history_dims_row(h, d, 3, 0) == t.dims, "an empty cell's id reads row 0");
  }

  if (failures) return 1;
  std::printf("{\"checks\": %d, \"frames\": 13, \"slots\": 3}\n", checks);
  return 0;
}

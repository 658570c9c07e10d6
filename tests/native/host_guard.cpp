// Stand-alone host program over smarts_amd/csrc/smx_guard.h (tests/test_host_guard.py builds it with
// -fsanitize=address,undefined and runs it): the in-bounds test, the guard box, the index bound at the largest margin and
// the resolution table, on the host.  Arguments: one group of ten numbers per map —
//   lpg_x0 lpg_y0 lpg_cell lpg_nx lpg_ny sg_x0 sg_y0 sg_cell sg_nx sg_ny
// (the grids of the packed tables); the first group is the map the word and box cases run on.  Prints one JSON line and
// returns 0 when every check held, else prints the failed checks and returns 1.
#include <hip/hip_runtime.h>  // the shim: plain C++

#include <cfloat>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "smx_guard.h"

struct Vs {  // VehState's members (smx_vehicle.h)
  double x, y, heading, u, v, r, delta;
};
struct Grids {
  double lpg_x0, lpg_y0, lpg_cell;
  int lpg_nx, lpg_ny;
  double sg_x0, sg_y0, sg_cell;
  int sg_nx, sg_ny;
};

static int failures = 0, checks = 0;
static void expect(bool ok, const std::string& what) {
  ++checks;
  if (!ok) {
    ++failures;
    std::printf("FAILED: %s\n", what.c_str());
  }
}

static GuardBox box_of(const Grids& g, double margin) {
  return guard_box_of(g.lpg_x0, g.lpg_y0, g.lpg_cell, g.lpg_nx, g.lpg_ny, g.sg_x0, g.sg_y0, g.sg_cell, g.sg_nx, g.sg_ny, margin);
}

// a model of the state rows of one vehicle and what a control kernel does with a verdict
struct Rows {
  double w[14];  // SMX_S_X .. SMX_S_MCL_Y
  int flags;
  uint8_t byte;
};
static void apply(Rows& rows, const GuardVerdict v, const Rows& stepped, const smx_lp_rec& lp0) {
  rows.byte = v.byte;
  if (v.action == GUARD_STORE) {
    for (int i = 0; i < 14; ++i) rows.w[i] = stepped.w[i];
    rows.flags = stepped.flags;
  } else if (v.action == GUARD_PARK) {
    const GuardParked p = guard_parked_pose(lp0);
    for (int i = 0; i < 14; ++i) rows.w[i] = 0.0;
    rows.w[SMX_S_X] = p.x;
    rows.w[SMX_S_Y] = p.y;
    rows.w[SMX_S_HEADING] = p.heading;
    rows.flags = (rows.flags & ~SMX_F_MCL_SET) | SMX_F_GUARDED;
  } else {
    rows.flags |= SMX_F_GUARDED;
  }
}

int main(int argc, char** argv) {
  if (argc < 11 || (argc - 1) % 10 != 0) {
    std::fprintf(stderr, "usage: host_guard (lpg_x0 lpg_y0 lpg_cell lpg_nx lpg_ny sg_x0 sg_y0 sg_cell sg_nx sg_ny)+\n");
    return 2;
  }
  std::vector<Grids> maps;
  for (int i = 1; i + 9 < argc; i += 10) {
    Grids g;
    g.lpg_x0 = std::atof(argv[i]), g.lpg_y0 = std::atof(argv[i + 1]), g.lpg_cell = std::atof(argv[i + 2]);
    g.lpg_nx = std::atoi(argv[i + 3]), g.lpg_ny = std::atoi(argv[i + 4]);
    g.sg_x0 = std::atof(argv[i + 5]), g.sg_y0 = std::atof(argv[i + 6]), g.sg_cell = std::atof(argv[i + 7]);
    g.sg_nx = std::atoi(argv[i + 8]), g.sg_ny = std::atoi(argv[i + 9]);
    maps.push_back(g);
  }
  const Grids& g = maps[0];
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

  // ---- finiteness: NaN, +inf, -inf in each of the seven words in turn
  {
    const GuardBox b = box_of(g, SMX_GUARD_MARGIN_DEFAULT);
    const Vs good = {0.5 * (b.x0 + b.x1), 0.5 * (b.y0 + b.y1), 0.3, 5.0, 0.1, 0.01, 0.02};
    expect(guard_in_bounds(b, good), "a finite state in the middle of the box is in bounds");
    expect(guard_in_bounds_kin(b, good.x, good.y, good.heading, good.u), "... and as a kinematic state");
    const double bad[3] = {nan, inf, -inf};
    for (int w = 0; w < 7; ++w)
      for (int k = 0; k < 3; ++k) {
        Vs s = good;
        double* words[7] = {&s.x, &s.y, &s.heading, &s.u, &s.v, &s.r, &s.delta};
        *words[w] = bad[k];
        expect(!guard_in_bounds(b, s), "word " + std::to_string(w) + " value " + std::to_string(k) + " is out of bounds");
        expect(!guard_in_bounds(b, s.x, s.y, s.heading, s.u, s.v, s.r, s.delta), "... through the seven-word form");
        if (w < 4) expect(!guard_in_bounds_kin(b, s.x, s.y, s.heading, s.u), "... and as a kinematic state / spawn row");
      }
    expect(guard_in_bounds(b, Vs{good.x, good.y, DBL_MAX, -DBL_MAX, 0, 0, 0}), "the largest finite words are finite");
  }

  // ---- the box: the four edges at +-0, +-1 ulp and +-margin; margin 0
  for (const double margin : {0.0, 50.0, SMX_GUARD_MARGIN_DEFAULT, SMX_GUARD_MARGIN_MAX}) {
    const GuardBox b = box_of(g, margin), raw = box_of(g, 0.0);
    const std::string tag = " (margin " + std::to_string(margin) + ")";
    // the box is the union of both grids, grown
    const double ux0 = std::min(g.lpg_x0, g.sg_x0), uy0 = std::min(g.lpg_y0, g.sg_y0);
    const double ux1 = std::max(g.lpg_x0 + g.lpg_cell * g.lpg_nx, g.sg_x0 + g.sg_cell * g.sg_nx);
    const double uy1 = std::max(g.lpg_y0 + g.lpg_cell * g.lpg_ny, g.sg_y0 + g.sg_cell * g.sg_ny);
    expect(raw.x0 == ux0 && raw.y0 == uy0 && raw.x1 == ux1 && raw.y1 == uy1, "margin 0: the box is the union of the two grids' extents");
    expect(b.x0 == ux0 - margin && b.y0 == uy0 - margin && b.x1 == ux1 + margin && b.y1 == uy1 + margin, "the box is grown by the margin on every side" + tag);
    const double mx = 0.5 * (b.x0 + b.x1), my = 0.5 * (b.y0 + b.y1);
    struct Edge {
      double edge;
      bool is_x, low;
    } edges[4] = {{b.x0, true, true}, {b.x1, true, false}, {b.y0, false, true}, {b.y1, false, false}};
    for (const Edge& e : edges) {
      const double out_dir = e.low ? -inf : inf, in_dir = e.low ? inf : -inf;
      const double on = e.edge, just_out = std::nextafter(e.edge, out_dir), just_in = std::nextafter(e.edge, in_dir);
      auto at = [&](double v) { return e.is_x ? guard_in_box(b, v, my) : guard_in_box(b, mx, v); };
      expect(at(on), "a point on an edge is in the box" + tag);
      expect(at(just_in), "one ulp inside an edge is in the box" + tag);
      expect(!at(just_out), "one ulp outside an edge is out of the box" + tag);
      if (margin > 0.0) {
        // the un-grown grid's edge lies `margin` inside; `margin` beyond the box's edge lies outside
        expect(at(e.low ? e.edge + margin : e.edge - margin), "the grids' own edge is in the box" + tag);
        expect(!at(e.low ? e.edge - margin : e.edge + margin), "a margin beyond the box's edge is out" + tag);
      }
      if (e.edge == 0.0) expect(at(-0.0) && at(0.0), "both zeros lie on an edge at zero" + tag);
    }
    expect(guard_in_box(b, 0.0 + mx, -0.0 + my) && guard_in_box(b, mx, my), "the middle of the box" + tag);
    expect(!guard_in_box(b, nan, my) && !guard_in_box(b, mx, nan), "a NaN coordinate is in no box" + tag);
  }
  // (signed zeros on an edge: a box whose low edges are at 0)
  {
    const GuardBox z = guard_box_of(0.0, 0.0, 4.0, 10, 10, 0.0, 0.0, 8.0, 5, 5, 0.0);
    expect(guard_in_box(z, 0.0, 0.0) && guard_in_box(z, -0.0, -0.0), "+0 and -0 lie on an edge at 0");
    expect(!guard_in_box(z, -DBL_TRUE_MIN, 0.0), "the smallest negative number is outside an edge at 0");
  }

  // ---- the margin's range
  expect(guard_margin_ok(0.0) && guard_margin_ok(SMX_GUARD_MARGIN_DEFAULT) && guard_margin_ok(SMX_GUARD_MARGIN_MAX), "0, the default and the cap are margins");
  expect(!guard_margin_ok(-1e-300) && !guard_margin_ok(std::nextafter(SMX_GUARD_MARGIN_MAX, inf)) && !guard_margin_ok(nan) &&
             !guard_margin_ok(inf) && !guard_margin_ok(-inf),
         "negative, too large, NaN and infinite margins are refused");

  // ---- the largest margin: the cell index of the farthest in-bounds point, in int64, for every map given
  int64_t worst = 0;
  for (const Grids& m : maps) {
    const GuardBox b = box_of(m, SMX_GUARD_MARGIN_MAX);
    const double bound = guard_index_bound(b, m.lpg_cell, m.sg_cell);
    expect(bound < SMX_GUARD_INDEX_MAX, "the index bound of a shipped map at the largest margin stays below 2^30");
    const double xs[2] = {b.x0, b.x1}, ys[2] = {b.y0, b.y1};
    for (int cx = 0; cx < 2; ++cx)
      for (int cy = 0; cy < 2; ++cy)
        for (const double reach : {0.0, SMX_GUARD_REACH_MAX, -SMX_GUARD_REACH_MAX}) {
          const double idx[4] = {std::floor((xs[cx] + reach - m.lpg_x0) / m.lpg_cell), std::floor((ys[cy] + reach - m.lpg_y0) / m.lpg_cell),
                                 std::floor((xs[cx] + reach - m.sg_x0) / m.sg_cell), std::floor((ys[cy] + reach - m.sg_y0) / m.sg_cell)};
          for (int q = 0; q < 4; ++q) {
            const int64_t i = (int64_t)idx[q];
            const int64_t mag = i < 0 ? -i : i;
            if (mag > worst) worst = mag;
            expect(mag < ((int64_t)1 << 31), "a cell index of a corner of the largest box fits int32");
            expect((double)mag <= bound, "... and is within guard_index_bound");
            // the ring loops walk out to lp_max_ring = the farthest grid edge, in cells
            const int64_t n = q == 0 ? m.lpg_nx : q == 1 ? m.lpg_ny : q == 2 ? m.sg_nx : m.sg_ny;
            const int64_t ring = std::max(mag, (i - (n - 1)) < 0 ? -(i - (n - 1)) : (i - (n - 1)));
            expect(ring < ((int64_t)1 << 31), "the farthest ring of a corner of the largest box fits int32");
          }
        }
  }
  {  // a map whose cells are too fine for the largest margin is refused, and passes with a smaller one
    smx_map_tables t{};
    t.lpg_x0 = t.lpg_y0 = t.sg_x0 = t.sg_y0 = 0.0;
    t.lpg_cell = 0.001, t.sg_cell = 4.0;
    t.lpg_nx = t.lpg_ny = 1000, t.sg_nx = t.sg_ny = 1;
    expect(!guard_map_ok(t, SMX_GUARD_MARGIN_MAX), "millimetre cells and the largest margin: refused");
    expect(guard_map_ok(t, 1000.0), "millimetre cells and a kilometre: accepted");
    t.lpg_cell = 0.0;
    expect(!guard_map_ok(t, 0.0), "a grid without a cell size is refused");
  }

  // ---- the resolution table
  {
    smx_lp_rec lp0{};
    lp0.x = 12.5, lp0.y = -3.25, lp0.heading = 0.75;
    Rows start{};
    for (int i = 0; i < 14; ++i) start.w[i] = 1.0 + i;
    start.flags = SMX_F_ALIVE | SMX_F_MCL_SET | (2 << SMX_F_HIST_SHIFT);
    Rows stepped = start;
    for (int i = 0; i < 14; ++i) stepped.w[i] += 0.5;
    // good start, good step: stored, byte 0
    Rows r = start;
    GuardVerdict v = guard_resolve(false, true, true);
    apply(r, v, stepped, lp0);
    expect(v.action == GUARD_STORE && v.byte == 0 && !v.guarded() && std::memcmp(r.w, stepped.w, sizeof r.w) == 0 && r.flags == start.flags,
           "good start, good step: stored, byte 0");
    // good start, bad step: held bit for bit, STEP
    r = start;
    v = guard_resolve(false, true, false);
    apply(r, v, stepped, lp0);
    expect(v.action == GUARD_HOLD && v.byte == SMX_GUARD_STEP && v.guarded() && std::memcmp(r.w, start.w, sizeof r.w) == 0 &&
               r.flags == (start.flags | SMX_F_GUARDED),
           "good start, bad step: held bit for bit, SMX_GUARD_STEP");
    // bad start: parked at lanepoint 0, STATE (whatever the step would have been)
    for (const bool step_ok : {true, false}) {
      r = start;
      r.w[SMX_S_R] = nan;
      v = guard_resolve(false, false, step_ok);
      apply(r, v, stepped, lp0);
      bool rest = true;
      for (int i = SMX_S_U; i < 14; ++i) rest = rest && r.w[i] == 0.0;
      expect(v.action == GUARD_PARK && v.byte == SMX_GUARD_STATE && r.w[SMX_S_X] == lp0.x && r.w[SMX_S_Y] == lp0.y &&
                 r.w[SMX_S_HEADING] == lp0.heading && rest && r.flags == ((start.flags & ~SMX_F_MCL_SET) | SMX_F_GUARDED),
             "bad start: parked at lanepoint 0 at rest, controller state as after a reset, SMX_GUARD_STATE");
    }
    // bad spawn: parked, SPAWN; its first tick holds it and reports SPAWN again
    v = guard_resolve_spawn(false);
    expect(v.action == GUARD_PARK && v.byte == SMX_GUARD_SPAWN && v.guarded(), "bad spawn: parked, SMX_GUARD_SPAWN");
    v = guard_resolve_spawn(true);
    expect(v.action == GUARD_STORE && v.byte == 0, "good spawn: created as given, byte 0");
    v = guard_resolve(true, true, true);
    expect(v.action == GUARD_HOLD && v.byte == SMX_GUARD_SPAWN, "a parked spawn's first tick: held, SMX_GUARD_SPAWN still");
    v = guard_resolve(true, false, true);
    expect(v.action == GUARD_PARK && v.byte == (SMX_GUARD_STATE | SMX_GUARD_SPAWN), "a parked spawn whose state was overwritten: parked again, both bits");
    expect(SMX_GUARD_STEP == 1 && SMX_GUARD_STATE == 2 && SMX_GUARD_SPAWN == 4 && SMX_F_GUARDED == 4, "the header's values");
  }

  if (failures) return 1;
  std::printf("{\"checks\": %d, \"maps\": %zu, \"worst_index\": %" PRId64 "}\n", checks, maps.size(), worst);
  return 0;
}

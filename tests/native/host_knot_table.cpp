// The knot table of smarts_amd/csrc/smx_roadmap.h (KnotRow, build_knot_row, knot_row_serves) compiled for the HOST: a
// stand-alone program, run under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_host_knot_table.py, which
// writes the compiled tables of a map to a file: the raw smx_map_tables struct, then the 26 tables in SMX_MAP_TABLES'
// order, each behind its length in bytes (uint64).
//
//   host_knot_table <tables file>...
//
// For every lanepoint of every map, at lookaheads 16 and 32:
//   1. the row's n, nk, idx[] equal a plain walk_knots from that start with the row's filter, and nk16 / end16 describe the
//      lookahead-16 walk from there (its knots are the row's, its last one end16 when that is no knot of the row);
//   2. D chained as k_waypoints_emit chains it — the first term from the query point, then the row's d[] in order —
//      equals walk_knots' D bit for bit, from three query points (on the lanepoint, 0.4 m along, 0.4 m aside);
//   3. wherever knot_row_serves lets a junction filter take a row walked without one, the filtered walk is the row.
// Prints one JSON line; exit status 1 if anything differed.
#include <hip/hip_runtime.h>  // the shim: plain C++

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "smx_host.h"
#include "smx_roadmap.h"

#define CTRL_WPS 17  // SMX_CTRL_WPS (smx_vehicle.h): the controller's path is 16 hops

struct LoadedMap {
  smx_map_tables t;
  std::vector<std::vector<char>> keep;
};

static bool load(const char* path, LoadedMap& m) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  bool ok = fread(&m.t, sizeof(m.t), 1, f) == 1;
#define READ(field, type, count)                                              \
  if (ok) {                                                                   \
    uint64_t bytes = 0;                                                       \
    ok = fread(&bytes, sizeof(bytes), 1, f) == 1;                             \
    const size_t want = (size_t)(count) * sizeof(type);                       \
    ok = ok && bytes >= want;                                                 \
    m.keep.emplace_back((size_t)bytes + 8);                                   \
    ok = ok && (bytes == 0 || fread(m.keep.back().data(), 1, bytes, f) == bytes); \
    m.t.field = (const type*)m.keep.back().data();                            \
  }
  SMX_MAP_TABLES(READ, m.t)
#undef READ
  fclose(f);
  return ok && map_tables_error(m.t) == nullptr;
}

struct Walked {
  int n, nk;
  double D;
  std::vector<int> idx;
  std::vector<double> term;
  int cnt;
};

static Walked plain_walk(const MapDev& m, const RouteFilter& f, int start, int lookahead, double px, double py) {
  Walked w;
  BranchState bs;
  bs.reset();
  const PathWalk pw = walk_knots_terms(m, f, bs, start, lookahead, px, py, [&](int, int idx, int, double term) {
    w.idx.push_back(idx);
    w.term.push_back(term);
  });
  w.n = pw.n;
  w.nk = pw.nk;
  w.D = pw.D;
  w.cnt = 1;
  while (bs.advance()) {
    walk_knots(m, f, bs, start, lookahead, px, py, [](int, int, int) {});
    ++w.cnt;
  }
  return w;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

int main(int argc, char** argv) {
  long long rows = 0, tabled = 0, single = 0, checks = 0, bad_list = 0, bad_d = 0, bad_rule2 = 0, rule2_rows = 0;
  std::string per_map;
  for (int a = 1; a < argc; ++a) {
    LoadedMap lm;
    if (!load(argv[a], lm)) {
      fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    const MapDev m(lm.t);
    // the junction roads that lead to each road
    std::vector<std::vector<int>> into(m.n_roads);
    for (int r = 0; r < m.n_roads; ++r)
      if (m.road_is_junction[r] && m.road_out_road[r] >= 0) into[m.road_out_road[r]].push_back(r);
    for (const int lookahead : {16, 32}) {
      long long map_tabled = 0, map_single = 0;
      for (int lp = 0; lp < m.n_lanepoints; ++lp) {
        KnotRow row;
        build_knot_row(m, lp, lookahead, CTRL_WPS, row);
        const smx_lp_rec r0 = m.lp_rec[lp];
        const RouteFilter f = knot_row_filter(m, lp);
        const bool is_tabled = (row.flags & SMX_KROW_TABLED) != 0;
        ++rows;
        map_tabled += is_tabled;
        map_single += (row.flags & SMX_KROW_SINGLE_ROAD) != 0;
        // ---- 1. the list
        const Walked w = plain_walk(m, f, lp, lookahead, r0.x, r0.y);
        bool ok = row.n == w.n && row.nk == w.nk && is_tabled == (w.cnt == 1 && w.n > 0 && w.nk <= SMX_WPK_CAP);
        ok = ok && row.f0 == (f.n > 0 ? f.road[0] : -1) && row.f1 == (f.n > 1 ? f.road[1] : -1) && row.road == m.lane_road[r0.lane];
        for (int k = 0; ok && k < w.nk && k < SMX_WPK_CAP; ++k) ok = row.idx[k] == w.idx[k];
        if (ok && is_tabled && lookahead >= CTRL_WPS - 1) {
          const Walked w16 = plain_walk(m, f, lp, CTRL_WPS - 1, r0.x, r0.y);
          ok = row.nk16 == w16.nk && w16.n == (w.n < CTRL_WPS ? w.n : CTRL_WPS);
          for (int k = 0; ok && k < w16.nk; ++k) {
            const int mine = (k == w16.nk - 1 && row.end16 >= 0) ? row.end16 : row.idx[k];
            ok = mine == w16.idx[k];
          }
        }
        ++checks;
        if (!ok) ++bad_list;
        if (!is_tabled) continue;
        // ---- 2. D, chained
        const double q[3][2] = {{r0.x, r0.y}, {r0.x + 0.4 * r0.dirx, r0.y + 0.4 * r0.diry}, {r0.x - 0.4 * r0.diry, r0.y + 0.4 * r0.dirx}};
        for (int i = 0; i < 3; ++i) {
          const double px = q[i][0], py = q[i][1];
          const Walked ref = plain_walk(m, f, lp, lookahead, px, py);
          double D = 0.0;
          if (row.nk >= 1) {
            const double proj = (px - r0.x) * r0.dirx + (py - r0.y) * r0.diry;
            const double k0x = r0.x + proj * r0.dirx, k0y = r0.y + proj * r0.diry;
            const smx_lp_rec k1 = m.lp_rec[row.idx[0]];
            const double ex = k1.x - k0x, ey = k1.y - k0y;
            D = sqrt(ex * ex + ey * ey);
            for (int k = 2; k <= SMX_WPK_CAP; ++k)
              if (k <= row.nk) D += row.d[k - 2];
          }
          ++checks;
          if (!same_bits(D, ref.D) || ref.nk != row.nk) ++bad_d;
        }
        // ---- 3. a junction filter on a row walked without one
        if (row.f0 < 0 && (row.flags & SMX_KROW_SINGLE_ROAD)) {
          for (const int j : into[row.road]) {
            const RouteFilter fj = junction_filter(m, j);
            if (!knot_row_serves(row.flags, row.f0, row.f1, row.road, fj)) {
              ++bad_rule2;  // (the rule is meant to hold here)
              continue;
            }
            ++rule2_rows;
            int idx[SMX_WPK_CAP];
            double d[SMX_WPK_CAP];
            for (int k = 0; k < SMX_WPK_CAP; ++k) idx[k] = -1, d[k] = 0.0;
            const KnotListHead hd = walk_knot_list(m, fj, lp, lookahead, CTRL_WPS, r0.x, r0.y, [&](int k, int id, double term) {
              idx[k - 1] = id;
              d[k - 1] = term;
            });
            bool same = hd.n == row.n && hd.nk == row.nk && hd.cnt == 1 && hd.nk16 == row.nk16 && hd.end16 == row.end16;
            for (int k = 0; same && k < row.nk; ++k) same = idx[k] == row.idx[k] && (k == 0 || same_bits(d[k], row.d[k - 1]));
            ++checks;
            if (!same) ++bad_rule2;
          }
        }
        // (a fixed route is never served)
        RouteFilter fixed;
        fixed.n = SMX_ROUTE_FIXED;
        fixed.road[0] = 0;
        fixed.road[1] = row.road;
        if (knot_row_serves(row.flags, row.f0, row.f1, row.road, fixed)) ++bad_rule2;
      }
      tabled += map_tabled;
      single += map_single;
      char buf[256];
      snprintf(buf, sizeof(buf), "%s{\"file\": %d, \"lookahead\": %d, \"rows\": %d, \"tabled\": %lld, \"single_road\": %lld, \"bytes\": %zu}",
               per_map.empty() ? "" : ", ", a, lookahead, (int)m.n_lanepoints, map_tabled, map_single, (size_t)m.n_lanepoints * sizeof(KnotRow));
      per_map += buf;
    }
  }
  printf("{\"maps\": %d, \"rows\": %lld, \"tabled\": %lld, \"single_road\": %lld, \"checks\": %lld, \"rule2_uses\": %lld, "
         "\"bad_list\": %lld, \"bad_D\": %lld, \"bad_rule2\": %lld, \"per_map\": [%s]}\n",
         argc - 1, rows, tabled, single, checks, rule2_rows, bad_list, bad_d, bad_rule2, per_map.c_str());
  return (bad_list || bad_d || bad_rule2) ? 1 : 0;
}

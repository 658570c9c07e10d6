// smx_guard.h — the state guard (include/smx.h, smx_set_guard): the test "is this vehicle state in bounds" and what
// becomes of a vehicle that fails it, each written once.  Every control form (k_control, k_control_paths / k_control_law,
// k_control_fast / k_control_listed, k_control_kinematic), k_reset and the commit-time respawn call these; the header
// holds no HIP and also compiles for the host (tests/native/host_guard.cpp drives it under AddressSanitizer + UBSan).
//
// In bounds = every word finite AND (x, y) inside the guard box: the union of the lanepoint grid's and the segment grid's
// extents grown by `margin` metres on every side.  Both edges belong to the box.
//
// Why SMX_GUARD_MARGIN_MAX bounds the map searches.  A search turns a coordinate into a cell index with
// (int)floor((p +- reach - x0) / cell), x0 the origin of one of the two grids.  `reach` is a fixed radius of a sensor or
// a query (at most SMX_GUARD_REACH_MAX metres) or, in the seeded searches of smx_scan.h, a distance between the pose and
// a point found at the vehicle's previous pose, which was in bounds too: at most the box's diagonal, under 1.5 x its
// longer side.  For an in-bounds p, |p - x0| <= side, the longer side of the grown box (both grids lie inside it).  So
// |index| <= (2.5 side + SMX_GUARD_REACH_MAX) / cell + 1 for the smaller cell: guard_index_bound().  smx_set_guard /
// smx_load_map refuse a (map, margin) pair whose bound reaches SMX_GUARD_INDEX_MAX = 2^30: half of int32, the room to
// spare (index differences, index + ring).  At the cap of 1.0e6 m a map with cells of a metre may span 4.2e8 m and one
// with cells of 0.01 m 2.2e6 m; the three shipped maps (cells of 4 and 8 m, at most 1 456 m across) reach 1.3e6.  The
// ring loops walk out to lp_max_ring, at most that same bound.
#pragma once
#include <stdint.h>

#include "../../include/smx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMX_GUARD_FN __host__ __device__ __forceinline__
#else
#define SMX_GUARD_FN inline
#endif

#define SMX_GUARD_REACH_MAX 1024.0              // metres: no sensor or query radius is larger
#define SMX_GUARD_INDEX_MAX 1073741824.0        // 2^30

struct GuardBox {
  double x0, y0, x1, y1;  // grown by the margin already; x0 > x1: no box (nothing is in bounds)
};

// (false for a NaN and for both infinities; one v_cmp_class_f64 on the device)
SMX_GUARD_FN bool guard_finite(double v) { return __builtin_isfinite(v); }

// The union of the two grids' extents, grown by margin.
SMX_GUARD_FN GuardBox guard_box_of(double lpg_x0, double lpg_y0, double lpg_cell, int lpg_nx, int lpg_ny, double sg_x0,
                                   double sg_y0, double sg_cell, int sg_nx, int sg_ny, double margin) {
  const double lx1 = lpg_x0 + lpg_cell * (double)lpg_nx, ly1 = lpg_y0 + lpg_cell * (double)lpg_ny;
  const double sx1 = sg_x0 + sg_cell * (double)sg_nx, sy1 = sg_y0 + sg_cell * (double)sg_ny;
  GuardBox b;
  b.x0 = (lpg_x0 < sg_x0 ? lpg_x0 : sg_x0) - margin;
  b.y0 = (lpg_y0 < sg_y0 ? lpg_y0 : sg_y0) - margin;
  b.x1 = (lx1 > sx1 ? lx1 : sx1) + margin;
  b.y1 = (ly1 > sy1 ? ly1 : sy1) + margin;
  return b;
}
SMX_GUARD_FN GuardBox guard_box_of(const smx_map_tables& m, double margin) {
  return guard_box_of(m.lpg_x0, m.lpg_y0, m.lpg_cell, m.lpg_nx, m.lpg_ny, m.sg_x0, m.sg_y0, m.sg_cell, m.sg_nx, m.sg_ny, margin);
}

// The margin on its own: finite and 0 <= margin <= SMX_GUARD_MARGIN_MAX.
SMX_GUARD_FN bool guard_margin_ok(double margin) { return guard_finite(margin) && margin >= 0.0 && margin <= SMX_GUARD_MARGIN_MAX; }

// The largest |cell index| a search can form for an in-bounds point (see the head of the file), as a double.
SMX_GUARD_FN double guard_index_bound(const GuardBox& grown, double lpg_cell, double sg_cell) {
  const double sx = grown.x1 - grown.x0, sy = grown.y1 - grown.y0;
  const double side = sx > sy ? sx : sy;
  const double cell = lpg_cell < sg_cell ? lpg_cell : sg_cell;
  return (2.5 * side + SMX_GUARD_REACH_MAX) / cell + 1.0;
}
SMX_GUARD_FN bool guard_map_ok(const smx_map_tables& m, double margin) {
  if (!(m.lpg_cell > 0.0) || !(m.sg_cell > 0.0)) return false;
  const double bound = guard_index_bound(guard_box_of(m, margin), m.lpg_cell, m.sg_cell);
  return guard_finite(bound) && bound < SMX_GUARD_INDEX_MAX;
}

SMX_GUARD_FN bool guard_in_box(const GuardBox& b, double x, double y) {
  return x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1;  // (false for a NaN)
}

// A dynamic vehicle: the seven words of VehState.
SMX_GUARD_FN bool guard_in_bounds(const GuardBox& b, double x, double y, double heading, double u, double v, double r, double delta) {
  const bool finite = guard_finite(x) & guard_finite(y) & guard_finite(heading) & guard_finite(u) & guard_finite(v) &
                      guard_finite(r) & guard_finite(delta);
  return finite && guard_in_box(b, x, y);
}
template <class State>  // anything with VehState's members
SMX_GUARD_FN bool guard_in_bounds(const GuardBox& b, const State& s) {
  return guard_in_bounds(b, s.x, s.y, s.heading, s.u, s.v, s.r, s.delta);
}
// A kinematic vehicle, and a spawn row: x, y, heading, speed.
SMX_GUARD_FN bool guard_in_bounds_kin(const GuardBox& b, double x, double y, double heading, double speed) {
  const bool finite = guard_finite(x) & guard_finite(y) & guard_finite(heading) & guard_finite(speed);
  return finite && guard_in_box(b, x, y);
}

// What becomes of the vehicle.
enum GuardAction {
  GUARD_STORE = 0,  // in bounds: the tick goes on / the stepped state is stored
  GUARD_HOLD = 1,   // nothing of the vehicle is stored: it keeps the state of the start of the tick
  GUARD_PARK = 2    // the vehicle is put at lanepoint 0 at rest, controller state as after a reset
};
struct GuardVerdict {
  uint8_t byte;    // SMX_GUARD_* bits for guard_dev[gid]
  uint8_t action;  // GuardAction
  bool guarded() const { return byte != 0; }  // the agent carries SMX_F_GUARDED from here on
};

// The control phase.  `flagged`: the vehicle carries SMX_F_GUARDED already (a parked spawn: its first tick; nothing else
// reaches a control phase with the flag, a guarded agent is gone after its next observation).  `start_ok`: its state at
// the start of the tick is in bounds.  `step_ok`: the stepped state is.  The kernels ask twice — at the load with
// step_ok = true ("may the controller, its path search and the dynamics run?": only GUARD_STORE says yes), and with the
// stepped state in hand.
SMX_GUARD_FN GuardVerdict guard_resolve(bool flagged, bool start_ok, bool step_ok) {
  GuardVerdict v;
  if (!start_ok) {
    v.byte = (uint8_t)(SMX_GUARD_STATE | (flagged ? SMX_GUARD_SPAWN : 0));
    v.action = GUARD_PARK;
  } else if (flagged) {
    v.byte = SMX_GUARD_SPAWN;
    v.action = GUARD_HOLD;
  } else if (!step_ok) {
    v.byte = SMX_GUARD_STEP;
    v.action = GUARD_HOLD;
  } else {
    v.byte = 0;
    v.action = GUARD_STORE;
  }
  return v;
}
// The reset pass: a spawn row (x, y, heading, speed).
SMX_GUARD_FN GuardVerdict guard_resolve_spawn(bool spawn_ok) {
  GuardVerdict v;
  v.byte = spawn_ok ? 0 : SMX_GUARD_SPAWN;
  v.action = spawn_ok ? GUARD_STORE : GUARD_PARK;
  return v;
}

// The parked state: lanepoint 0's pose (always on the map), everything else of the state and controller words zero.
struct GuardParked {
  double x, y, heading;
};
SMX_GUARD_FN GuardParked guard_parked_pose(const smx_lp_rec& lp0) {
  GuardParked p;
  p.x = lp0.x;
  p.y = lp0.y;
  p.heading = lp0.heading;
  return p;
}

// smx_k_lidar.h — the lidar role and its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_plan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

// =================================================================================
// lidar role: lidar sensor (LidarSensor sensors.py:797-827, Lidar lidar.py:58-134): one wavefront per
// observing vehicle, lanes over rays.  Ray i = [origin, origin + base_ray[i]], origin = vehicle
// position + (0, 0, 1); base rays come from the host (they do not rotate with the vehicle,
// lidar.py:109-113).  pybullet rayTestBatch is substituted by exact ray / oriented-box and
// ray / ground-plane intersection (DESIGN.md "Substitutions"); a miss reports (inf, inf, inf).
// =================================================================================
struct LidarPose {
  double x, y, fx, fy;  // centre, forward axis
  int slot;             // its slot in the env (the compacted list's order is not the env's)
};

// (SIZED: per-vehicle dimensions, smx_set_social_history_dims — 1 bound, 0 not: the launches of its own, for which the
// launch plan picks the instantiation; -1: the role inside k_sensors / k_first, which asks the argument block)
template <int SIZED>
__device__ __forceinline__ void lidar_role(const KernelArgs& a, const int block) {
  __shared__ LidarPose mates[SMX_BLOCK];
  const bool sized = SIZED < 0 ? dims_sized(a) : SIZED != 0;
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = (size_t)block;
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  const bool live = (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (!a.first_only || (flags & SMX_F_FIRST));
  if (!live) return;
  const int n_veh = c.num_vehicles;
  const int env = (int)(gid / n_veh);
  const int slot = (int)(gid - (size_t)env * n_veh);
  // env-mates that a ray can reach at all (|ray| = max_distance; a chassis box lies within 2.1 m of
  // its centre — with dimensions bound, smx_set_social_history_dims, within the mate's own half diagonal),
  // compacted into LDS by ballot / prefix count — the order does not matter for a min
  __shared__ int n_mates;
  {
    const double ex = SF(SMX_S_X), ey = SF(SMX_S_Y);
    const double reach = c.lidar_max_distance + 2.1;
    bool keep = false;
    LidarPose p;
    p.x = p.y = p.fx = p.fy = 0.0;
    p.slot = (int)threadIdx.x;
    if ((int)threadIdx.x < n_veh && (int)threadIdx.x != slot) {
      const size_t og = (size_t)env * n_veh + threadIdx.x;
      if (a.st.flags[og] & SMX_F_ALIVE) {
        p.x = a.st.f64[(size_t)SMX_S_X * total + og];
        p.y = a.st.f64[(size_t)SMX_S_Y * total + og];
        const double dx = p.x - ex, dy = p.y - ey;
        double mate_reach = reach;
        if (sized) {
          const VehBox mb = vehicle_box(a, og, true);
          // (+ 0.12 m: the slack the sedan's 2.1 has over its 1.98 — a corner exactly at max_distance must not be lost to rounding)
          mate_reach = c.lidar_max_distance + 0.5 * sqrt(mb.length * mb.length + mb.width * mb.width) + 0.12;
        }
        if (dx * dx + dy * dy <= mate_reach * mate_reach) {
          const double h = wrap_heading(a.st.f64[(size_t)SMX_S_HEADING * total + og]);
          p.fx = -sin(h);
          p.fy = cos(h);
          keep = true;
        }
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) mates[__popcll(mask & ((1ull << threadIdx.x) - 1ull))] = p;
    if (threadIdx.x == 0) n_mates = __popcll(mask);
  }
  __syncthreads();
  const int mates_n = n_mates;
  const double ox = SF(SMX_S_X), oy = SF(SMX_S_Y), oz = SMX_BASE_HEIGHT + 1.0;
  const double hl = 0.5 * SMX_CHASSIS_LENGTH, hw = 0.5 * SMX_CHASSIS_WIDTH, hh = 0.5 * SMX_CHASSIS_HEIGHT;
  const double bz = SMX_BASE_HEIGHT + 0.6;  // chassis box centre height (models/vehicle.urdf)
  for (int i = threadIdx.x; i < c.lidar_rays; i += (int)blockDim.x) {
    const double dx = a.lidar_rays[i * 3 + 0], dy = a.lidar_rays[i * 3 + 1], dz = a.lidar_rays[i * 3 + 2];
    double best = SMX_INF;
    if (dz < 0.0) {
      const double t = -oz / dz;
      if (t >= 0.0 && t <= 1.0) best = t;
    }
    for (int j = 0; j < mates_n; ++j) {
      const LidarPose p = mates[j];
      double mhl = hl, mhw = hw, mhh = hh, mbz = bz;
      if (sized) {
        // the mate's own half length and half width; vertically the box keeps the sedan's underside, SMX_BASE_HEIGHT
        // + 0.1, and rises by the vehicle's height (a stated deviation: the reference centres a BoxChassis box on z = 0)
        const VehBox mb = vehicle_box(a, (size_t)env * n_veh + p.slot, true);
        mhl = 0.5 * mb.length, mhw = 0.5 * mb.width, mhh = 0.5 * mb.height;
        mbz = bz + (mhh - hh);  // (a sedan-high mate: bz itself)
      }
      const double relx = ox - p.x, rely = oy - p.y, relz = oz - mbz;
      // slabs along the box axes: forward f, right r = (f.y, -f.x), up
      double tmin = 0.0, tmax = 1.0;
      bool miss = false;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        double o, d, half;
        if (ax == 0) {
          o = relx * p.fx + rely * p.fy;
          d = dx * p.fx + dy * p.fy;
          half = mhl;
        } else if (ax == 1) {
          o = relx * p.fy + rely * (-p.fx);
          d = dx * p.fy + dy * (-p.fx);
          half = mhw;
        } else {
          o = relz;
          d = dz;
          half = mhh;
        }
        if (d == 0.0) {
          if (fabs(o) > half) miss = true;
        } else {
          double t1 = (-half - o) / d, t2 = (half - o) / d;
          if (t1 > t2) {
            double tt = t1;
            t1 = t2;
            t2 = tt;
          }
          tmin = fmax(tmin, t1);
          tmax = fmin(tmax, t2);
          if (tmin > tmax) miss = true;
        }
      }
      if (!miss && tmin < best) best = tmin;
    }
    const size_t q = gid * (size_t)c.lidar_rays + i;
    if (best <= 1.0) {
      a.out.lidar_hit[q] = 1;
      a.out.lidar_point[q * 3 + 0] = ox + best * dx;
      a.out.lidar_point[q * 3 + 1] = oy + best * dy;
      a.out.lidar_point[q * 3 + 2] = oz + best * dz;
    } else {
      a.out.lidar_hit[q] = 0;
      const double inf = __builtin_huge_val();
      a.out.lidar_point[q * 3 + 0] = inf;
      a.out.lidar_point[q * 3 + 1] = inf;
      a.out.lidar_point[q * 3 + 2] = inf;
    }
  }
}

template <bool SIZED>
__global__ void __launch_bounds__(SMX_BLOCK) k_lidar(const KernelArgs a) { lidar_role<SIZED ? 1 : 0>(a, (int)blockIdx.x); }
// The lidar of the reset pass on large batches: almost no vehicle is new in a given tick, and when an env restarts
// all its vehicles are — neighbours in memory.  Workgroup w looks at the vehicles v = w (mod gridDim.x), 64 flags per
// load and ballot, and runs the lidar role for the new ones it finds: an env's 64 new vehicles land in 64 different
// workgroups instead of one after the other in k_first's, and a tick without restarts pays a few microseconds.
#define SMX_LIDAR_FIRST_BLOCKS 1024
template <bool SIZED>
__global__ void __launch_bounds__(SMX_BLOCK) k_lidar_first(const KernelArgs a) {
  const size_t total = (size_t)a.cfg.num_envs * a.cfg.num_vehicles;
  const size_t stride = (size_t)gridDim.x;
  for (size_t base = blockIdx.x; base < total; base += stride * SMX_BLOCK) {
    const size_t v = base + (size_t)threadIdx.x * stride;
    const int f = v < total ? a.st.flags[v] : 0;
    unsigned long long fresh = __ballot((f & SMX_F_ALIVE) && (f & SMX_F_FIRST) && !(f & SMX_F_SOCIAL));
    while (fresh != 0ull) {  // uniform in the (one-wavefront) workgroup
      const int l = __ffsll((long long)fresh) - 1;
      fresh &= fresh - 1ull;
      lidar_role<SIZED ? 1 : 0>(a, (int)(base + (size_t)l * stride));
      __syncthreads();  // the role's LDS block is reused
    }
  }
}

// smx_k_grids.h — the grid roles: OGM, DAGM and top-down RGB tiles, and their kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "smx_plan.h"
#include "smx_tick.h"
#include "smx_vehicle.h"

// =================================================================================
// OGM role: occupancy grid map sensor (OGMSensor, sensors.py:719-758): one wavefront per observing
// vehicle.  The H x W byte tile is built in LDS (lane j rasterises env-mate j's footprint over the
// few pixels its bounding rectangle touches) and leaves as full 16-byte pieces — the kernel is
// bound by its own 4 KiB-per-agent output stream.  Pixel rule (substitution for the Panda3D
// orthographic render, renderer.py:325-395): a pixel is 255 iff its centre lies inside a vehicle's
// oriented chassis rectangle; view centred on the vehicle, +row = behind, row 0 = ahead
// (np.flipud, sensors.py:748), extent width*res x height*res (renderer.py:384-385).
// =================================================================================
struct OgmMate {
  double cx, cy, vfx, vfy, vrx, vry;  // centre and axes of the footprint in the ego frame
  int c0, r0, bw, n_px;               // pixel rectangle: first column / row, width, pixel count
};

// Vehicle `og`'s footprint in the frame of the observer at (ex0, ey0) with right axis (rx, ry) and forward axis
// (fx, fy), and the pixel rectangle of a W x H grid that can hold it; false (q untouched): the rectangle misses the view.
__device__ __forceinline__ bool ogm_mate_footprint(const KernelArgs& a, const size_t og, const size_t total, const int W, const int H,
                                                   const double res, const double ex0, const double ey0, const double rx, const double ry,
                                                   const double fx, const double fy, OgmMate& q) {
  const VehBox box = vehicle_box(a, og);
  const double hl = 0.5 * box.length, hw = 0.5 * box.width;
  const double vx = a.st.f64[(size_t)SMX_S_X * total + og], vy = a.st.f64[(size_t)SMX_S_Y * total + og];
  const double vh = wrap_heading(a.st.f64[(size_t)SMX_S_HEADING * total + og]);
  const double dx = vx - ex0, dy = vy - ey0;
  const double cx = dx * rx + dy * ry, cy = dx * fx + dy * fy;  // centre in the ego frame
  // the mate's axes in the ego frame from each vehicle's own cos / sin (the rule k_ogm_env shares)
  const double cm = cos(vh), sm = sin(vh);
  const double vfx = cm * ry - sm * rx, vfy = sm * ry + cm * rx, vrx = cm * rx + sm * ry, vry = sm * rx - cm * ry;
  const double ext_x = fabs(vfx) * hl + fabs(vrx) * hw, ext_y = fabs(vfy) * hl + fabs(vry) * hw;
  // pixel centre (r, col): x = (col + 0.5 - W/2) res, y = (H/2 - (r + 0.5)) res
  int c0 = (int)floor((cx - ext_x) / res + 0.5 * W - 0.5) - 1, c1 = (int)ceil((cx + ext_x) / res + 0.5 * W - 0.5) + 1;
  int r0 = (int)floor(0.5 * H - 0.5 - (cy + ext_y) / res) - 1, r1 = (int)ceil(0.5 * H - 0.5 - (cy - ext_y) / res) + 1;
  c0 = max(c0, 0);
  r0 = max(r0, 0);
  c1 = min(c1, W - 1);
  r1 = min(r1, H - 1);
  if (c0 > c1 || r0 > r1) return false;
  q.cx = cx;
  q.cy = cy;
  q.vfx = vfx;
  q.vfy = vfy;
  q.vrx = vrx;
  q.vry = vry;
  q.c0 = c0;
  q.r0 = r0;
  q.bw = c1 - c0 + 1;
  q.n_px = (c1 - c0 + 1) * (r1 - r0 + 1);
  return true;
}

// ... drawn by the workgroup's lanes over the rectangle's pixels: VALUE where the pixel centre lies inside the chassis
// of vehicle `og` (the rectangle is clamped to the view and walked whole, whatever the vehicle's size)
template <int VALUE>
__device__ __forceinline__ void ogm_draw_mate(const KernelArgs& a, const size_t og, unsigned char* tile, const OgmMate& q, const int W,
                                              const int H, const double res) {
  const VehBox box = vehicle_box(a, og);
  const double hl = 0.5 * box.length, hw = 0.5 * box.width;
  for (int p = (int)threadIdx.x; p < q.n_px; p += SMX_BLOCK) {
    const int r = q.r0 + p / q.bw, col = q.c0 + p % q.bw;
    const double py = (0.5 * H - (r + 0.5)) * res - q.cy;
    const double px = (col + 0.5 - 0.5 * W) * res - q.cx;
    if (fabs(px * q.vfx + py * q.vfy) <= hl && fabs(px * q.vrx + py * q.vry) <= hw) tile[r * W + col] = VALUE;
  }
}

__device__ __forceinline__ void ogm_role(const KernelArgs& a, const int block) {
  extern __shared__ __align__(16) unsigned char tile[];
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = (size_t)block;
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  const bool live = (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (!a.first_only || (flags & SMX_F_FIRST));
  if (!live) return;  // uniform for the whole workgroup
  const int W = c.ogm_width, H = c.ogm_height;
  const int n_veh = c.num_vehicles;
  const int env = (int)(gid / n_veh);
  const int bytes = W * H;
  for (int k = threadIdx.x; k < bytes / 4; k += SMX_BLOCK) reinterpret_cast<int*>(tile)[k] = 0;
  __syncthreads();
  const double res = c.ogm_resolution;
  const double ex0 = SF(SMX_S_X), ey0 = SF(SMX_S_Y), eh = wrap_heading(SF(SMX_S_HEADING));
  const double rx = cos(eh), ry = sin(eh);    // ego right axis
  const double fx = -sin(eh), fy = cos(eh);   // ego forward axis
  // Pass 1, lane j = env-mate j: its footprint in the ego frame and the pixel rectangle that can hold
  // it.  Pass 2: the mates whose rectangle meets the view (a ballot; typically a handful of the env)
  // are drawn one after the other with the wavefront's lanes over the rectangle's pixels — a lane per
  // mate would make every lane wait for the mate with the most pixels while most lanes draw nothing.
  __shared__ OgmMate mates[SMX_BLOCK];
  for (int base = 0; base < n_veh; base += SMX_BLOCK) {
    const int j = base + (int)threadIdx.x;
    bool in_view = false;
    if (j < n_veh) {
      const size_t og = (size_t)env * n_veh + j;
      if (a.st.flags[og] & SMX_F_ALIVE) in_view = ogm_mate_footprint(a, og, total, W, H, res, ex0, ey0, rx, ry, fx, fy, mates[threadIdx.x]);
    }
    unsigned long long todo = __ballot(in_view);
    __syncthreads();
    while (todo != 0ull) {  // uniform
      const int idx = __ffsll((long long)todo) - 1;
      const OgmMate q = mates[idx];
      todo &= todo - 1ull;
      ogm_draw_mate<255>(a, (size_t)env * n_veh + base + idx, tile, q, W, H, res);
    }
    __syncthreads();  // before the stage is reused (envs of more than 64 vehicles do not exist, but the loop is general)
  }
  __syncthreads();
  static_assert(SMX_BLOCK == 64, "ogm_store_tile: the workgroup is one wavefront");
  int4* dst = reinterpret_cast<int4*>(a.out.ogm + gid * (size_t)bytes);
  ogm_store_tile(reinterpret_cast<const int4*>(tile), dst, a.ogm_mask ? a.ogm_mask + gid * smx_ogm_mask_words((size_t)bytes) : nullptr,
                 bytes / 16, (int)threadIdx.x);
}

// k_ogm_env (large batches): the same tiles, one workgroup of four wavefronts per ENV.  The env's poses are
// loaded once, with one cos / sin pair per vehicle (a workgroup per observer reloads all its mates and takes
// a sine and a cosine per mate: n x n of each per env); every wavefront then builds the tiles of a quarter of
// the observers, one after the other, in its own LDS tile.
struct OgmPose {
  double x, y, ch, sh;  // centre, cos / sin of the wrapped heading
  int alive, observes;
};
#ifndef SMX_SIDE_PRIO  // developer: side streams that get the default priority instead of the lowest (bit i = side i)
#define SMX_SIDE_PRIO 0
#endif
// orders a wavefront's own LDS traffic for the compiler (the hardware keeps a wavefront's LDS operations in order)
#define SMX_WAVE_SYNC()                                   \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                      \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)
// a double of another lane of the wavefront (lane index uniform): two v_readlane_b32
__device__ __forceinline__ double readlane_f64(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// OBS observers per wavefront at a time (two while the env has at most 32 vehicles and eight tiles fit the LDS a
// workgroup may have): lane = (observer, env-mate) for the footprints' rectangles, so that a wavefront of 32-vehicle
// envs is full; the footprints in view are then drawn two at a time, each by a half wavefront of 8 rows x 4 columns
// (a car ahead is 3 x 6 pixels at 0.78 m per pixel: one step), its record fetched from the lane that holds it with
// ds_bpermute.  390 -> 1xx vector instructions per tile (a third of the headline tick's were this kernel's).
// (SIZED: per-vehicle dimensions are bound, smx_set_social_history_dims — a compile-time choice of the launch plan's: as a
// branch on the bound pointer the extents cost the kernel without them ten registers and a wavefront per SIMD,
// profiles/r17_vehicle_dims_resources.txt)
template <int OBS, bool SIZED>
__global__ void __attribute__((amdgpu_waves_per_eu(4, 8))) __launch_bounds__(SMX_OGM_WAVES * 64) k_ogm_env(const KernelArgs a) {
  SMX_TSTAMP(span0);
  extern __shared__ __align__(16) unsigned char tiles[];  // [SMX_OGM_WAVES][OBS][H * W]
  __shared__ OgmPose pose[SMX_BLOCK];
  __shared__ unsigned char observers[SMX_BLOCK];  // the env's observing slots, compacted: the wavefronts share them evenly
  __shared__ int n_observers;                     // however many agents of the env are gone
  const smx_config& c = a.cfg;
  const int n_veh = c.num_vehicles;
  const size_t total = (size_t)c.num_envs * n_veh;
  const int env = (int)blockIdx.x;
  const int W = c.ogm_width, H = c.ogm_height, bytes = W * H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if ((int)threadIdx.x < n_veh) {
    const size_t gid = (size_t)env * n_veh + threadIdx.x;
    const int flags = a.st.flags[gid];
    OgmPose p;
    p.alive = (flags & SMX_F_ALIVE) ? 1 : 0;
    p.observes = ((flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (!a.first_only || (flags & SMX_F_FIRST))) ? 1 : 0;
    p.x = SF(SMX_S_X);
    p.y = SF(SMX_S_Y);
    const double h = wrap_heading(SF(SMX_S_HEADING));
    p.ch = cos(h);
    p.sh = sin(h);
    pose[threadIdx.x] = p;
  }
  if (wave == 0) {  // (n_veh <= 64: the first wavefront sees every slot)
    const bool obs_here = lane < n_veh && pose[lane].observes;
    const unsigned long long om = __ballot(obs_here);
    if (obs_here) observers[__popcll(om & ((1ull << lane) - 1ull))] = (unsigned char)lane;
    if (lane == 0) n_observers = __popcll(om);
  }
  __syncthreads();
  unsigned char* tile = tiles + (size_t)wave * OBS * bytes;
  const double res = c.ogm_resolution;
  const double inv_res = 1.0 / res;  // for the pixel RECTANGLES only (an enumeration bound with a margin on every
                                     // side); the pixel test itself keeps the oracle's arithmetic
  const int half = lane >> 5, in_half = lane & 31;
  const int mate = OBS == 2 ? in_half : lane;
  const int mate_clamped = min(mate, n_veh - 1);  // (every lane computes; lanes past the env's vehicles are masked below)
  // this lane's mate's half extents: the sedan's, or with dimensions bound (smx_set_social_history_dims) its own — a
  // drawing step then fetches them from the lane that holds the footprint, as it fetches the rest of the record
  const VehBox mate_box = vehicle_box(a, (size_t)env * n_veh + mate_clamped, SIZED);
  const double hl = 0.5 * mate_box.length, hw = 0.5 * mate_box.width;
  const int lr = in_half >> 2, lc = in_half & 3;  // this lane's pixel of a drawing step: 8 rows x 4 columns per half
  // pixel centre (r, col): x = (col + 0.5 - W/2) res, y = (H/2 - (r + 0.5)) res; the sums in front of `res` are
  // exact in any order (integers and halves), so the constants are folded
  const double col_bias = 0.5 - 0.5 * W, row_bias = 0.5 * H - 0.5;
  const int n_obs = n_observers;
  const int per_round = SMX_OGM_WAVES * OBS;
  const int rounds = (n_obs + per_round - 1) / per_round;
  const size_t mask_words = smx_ogm_mask_words((size_t)bytes);
  // Each wavefront owns its tiles: inside the loop only lanes of ONE wavefront exchange data through LDS, whose
  // operations a wavefront issues in order — a scheduling fence is all that is needed (four workgroup barriers per
  // round made the four wavefronts wait for the slowest one's rectangles)
#pragma nounroll
  for (int it = 0; it < rounds; ++it) {
    const int turn0 = (it * SMX_OGM_WAVES + wave) * OBS;  // uniform in the wavefront
    const int n_live = min(OBS, n_obs - turn0);
    if (n_live <= 0) break;  // (turns grow with `it`)
    for (int k = lane; k < n_live * (bytes / 16); k += 64) reinterpret_cast<int4*>(tile)[k] = make_int4(0, 0, 0, 0);
    const int my_turn = turn0 + (OBS == 2 ? half : 0);
    const bool live = my_turn < n_obs;
    const int obs = (int)observers[live ? my_turn : turn0];
    // the footprint of vehicle `mate` in this observer's frame stays in this lane's registers (no LDS copy of it)
    const OgmPose e = pose[obs];
    const OgmPose v = pose[mate_clamped];
    const double rx = e.ch, ry = e.sh;   // ego right axis
    const double fx = -e.sh, fy = e.ch;  // ego forward axis
    const double dx = v.x - e.x, dy = v.y - e.y;
    const double cx = dx * rx + dy * ry, cy = dx * fx + dy * fy;  // centre in the ego frame
    const double cm = v.ch, sm = v.sh;
    const double vfx = cm * ry - sm * rx, vfy = sm * ry + cm * rx, vrx = cm * rx + sm * ry, vry = sm * rx - cm * ry;
    const double ext_x = fabs(vfx) * hl + fabs(vrx) * hw, ext_y = fabs(vfy) * hl + fabs(vry) * hw;
    // (a pixel centre inside the footprint lies inside its bounding box: columns ceil(lo) .. floor(hi).  The bounds
    // are rounded — a dozen operations on numbers below 1e3 pixels, errors of 1e-12 — and the pixel test accepts a
    // centre its own rounding puts on the edge: a millionth of a pixel on every side covers both.  A whole pixel of
    // margin made a car ahead, 3 x 6 pixels, a rectangle of 5 x 8.)
    const double slack = 1e-6;
    // (clamped as doubles first: a mate far away must not overflow the conversion)
    const double c_lo = fmax((cx - ext_x) * inv_res + 0.5 * W - 0.5 - slack, -1.0), c_hi = fmin((cx + ext_x) * inv_res + 0.5 * W - 0.5 + slack, (double)W);
    const double r_lo = fmax(0.5 * H - 0.5 - (cy + ext_y) * inv_res - slack, -1.0), r_hi = fmin(0.5 * H - 0.5 - (cy - ext_y) * inv_res + slack, (double)H);
    const int c0 = max((int)ceil(c_lo), 0), c1 = min((int)floor(c_hi), W - 1);
    const int r0 = max((int)ceil(r_lo), 0), r1 = min((int)floor(r_hi), H - 1);
    const int bw = c1 - c0 + 1, bh = r1 - r0 + 1;
    const bool in_view = live && mate < n_veh && v.alive != 0 && bw > 0 && bh > 0;
    unsigned long long todo = __ballot(in_view);
    SMX_WAVE_SYNC();
    while (todo != 0ull) {  // uniform in the wavefront: two footprints per turn, one per half
      const int s0 = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const int s1 = todo != 0ull ? __ffsll((long long)todo) - 1 : s0;
      const bool two = todo != 0ull;
      todo &= todo - 1ull;  // (0 & anything = 0)
      const int src = half ? s1 : s0;
      const bool drawing = half == 0 || two;
      const double qcx = __shfl(cx, src), qcy = __shfl(cy, src);
      const double qvfx = __shfl(vfx, src), qvfy = __shfl(vfy, src), qvrx = __shfl(vrx, src), qvry = __shfl(vry, src);
      const int qc0 = __shfl(c0, src), qr0 = __shfl(r0, src), qbw = __shfl(bw, src), qbh = __shfl(bh, src);
      double qhl = 0.5 * SMX_CHASSIS_LENGTH, qhw = 0.5 * SMX_CHASSIS_WIDTH;
      if constexpr (SIZED) qhl = __shfl(hl, src), qhw = __shfl(hw, src);
      unsigned char* dst_tile = tile + (OBS == 2 ? (src >> 5) * bytes : 0);
      const int bh_max = max(__builtin_amdgcn_readlane(bh, s0), __builtin_amdgcn_readlane(bh, s1));
      const int bw_max = max(__builtin_amdgcn_readlane(bw, s0), __builtin_amdgcn_readlane(bw, s1));
      // (one step nearly always: kept from the loop optimiser, which interleaved four column steps and paid two
      // dozen register copies per footprint for it)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
      for (int rr = 0; rr < bh_max; rr += 8) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int cc = 0; cc < bw_max; cc += 4) {
          const int dr = rr + lr, dc = cc + lc;
          const int r = qr0 + dr, col = qc0 + dc;
          const double py = (row_bias - (double)r) * res - qcy;
          const double px = ((double)col + col_bias) * res - qcx;
          if (drawing && dr < qbh && dc < qbw && fabs(px * qvfx + py * qvfy) <= qhl && fabs(px * qvrx + py * qvry) <= qhw)
            dst_tile[r * W + col] = 255;
        }
      }
    }
    SMX_WAVE_SYNC();
    for (int t = 0; t < n_live; ++t) {
      const int4* src_tile = reinterpret_cast<const int4*>(tile + (size_t)t * bytes);
      const size_t gid = (size_t)env * n_veh + (int)observers[turn0 + t];
      int4* dst = reinterpret_cast<int4*>(a.out.ogm + gid * (size_t)bytes);
      ogm_store_tile(src_tile, dst, a.ogm_mask ? a.ogm_mask + gid * mask_words : nullptr, bytes / 16, lane);
    }
    SMX_WAVE_SYNC();  // the tiles are reused
  }
  SMX_TSTAMP(span1);
  SMX_TSPAN(6, span0, span1);
}

// =================================================================================
// DAGM role: drivable-area grid map (DrivableAreaGridMapSensor, sensors.py:675-716): one workgroup per
// observing vehicle, the tile in LDS.  The reference renders the road mesh (lane centre lines
// buffered by half the lane width) through the OGM's camera; here a pixel is 255 when its centre
// lies within half a lane width of a segment of a lane centre line (DESIGN.md "Substitutions").
// The segment grid only prunes: a segment that can reach the view lies within the view's
// circumscribed circle grown by the widest half width, so its bounding box meets the visited cells.
// Wavefronts take segments, lanes the pixels of a segment's bounding box; a segment listed in
// several cells is drawn again (same value).
// =================================================================================
// The road layer of a W x H tile for the observer at (ex0, ey0): VALUE where the pixel centre lies within half a lane
// width of a segment (wavefronts over the segments of the grid cells the view can reach, lanes over a segment's pixels).
template <int VALUE>
__device__ __forceinline__ void road_layer(const KernelArgs& a, unsigned char* tile, const int W, const int H, const double res,
                                           const double ex0, const double ey0, const double rx, const double ry, const double fx,
                                           const double fy) {
  const MapDev& m = a.map;
  const double vw = 0.5 * W * res, vh = 0.5 * H * res;
  const double reach = sqrt(vw * vw + vh * vh) + a.dagm_reach + 1e-6;
  int cx0 = (int)floor((ex0 - reach - m.sg_x0) / m.sg_cell), cx1 = (int)floor((ex0 + reach - m.sg_x0) / m.sg_cell);
  int cy0 = (int)floor((ey0 - reach - m.sg_y0) / m.sg_cell), cy1 = (int)floor((ey0 + reach - m.sg_y0) / m.sg_cell);
  cx0 = max(cx0, 0);
  cy0 = max(cy0, 0);
  cx1 = min(cx1, m.sg_nx - 1);
  cy1 = min(cy1, m.sg_ny - 1);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = SMX_BLOCK >> 6;
  for (int gy = cy0; gy <= cy1; ++gy) {
    if (cx0 > cx1) break;
    const int row = gy * m.sg_nx;
    // cells of one grid row are contiguous in the member array
    const int m0 = m.sg_off[row + cx0], m1 = m.sg_off[row + cx1 + 1];
    for (int k = m0 + wave; k < m1; k += n_waves) {
      const smx_seg_rec s = m.sg_rec[k];
      const double hw = 0.5 * m.lane_width[s.lane];
      // end points in the ego frame (x to the right, y ahead)
      const double d1x = s.x1 - ex0, d1y = s.y1 - ey0, d2x = s.x2 - ex0, d2y = s.y2 - ey0;
      const double ax = d1x * rx + d1y * ry, ay = d1x * fx + d1y * fy;
      const double bx = d2x * rx + d2y * ry, by = d2x * fx + d2y * fy;
      // pixel centre (r, col): x = (col + 0.5 - W/2) res, y = (H/2 - (r + 0.5)) res
      int c0 = (int)floor((fmin(ax, bx) - hw) / res + 0.5 * W - 0.5) - 1, c1 = (int)ceil((fmax(ax, bx) + hw) / res + 0.5 * W - 0.5) + 1;
      int r0 = (int)floor(0.5 * H - 0.5 - (fmax(ay, by) + hw) / res) - 1, r1 = (int)ceil(0.5 * H - 0.5 - (fmin(ay, by) - hw) / res) + 1;
      c0 = max(c0, 0);
      r0 = max(r0, 0);
      c1 = min(c1, W - 1);
      r1 = min(r1, H - 1);
      if (c0 > c1 || r0 > r1) continue;
      const int bw = c1 - c0 + 1, n_px = bw * (r1 - r0 + 1);
      for (int q = lane; q < n_px; q += 64) {
        const int r = r0 + q / bw, col = c0 + q % bw;
        const double px = (col + 0.5 - 0.5 * W) * res, py = (0.5 * H - (r + 0.5)) * res;
        if (seg_point_dist2(px, py, ax, ay, bx, by) <= hw * hw) tile[r * W + col] = VALUE;
      }
    }
  }
}

__device__ __forceinline__ void dagm_role(const KernelArgs& a, const int block) {
  extern __shared__ __align__(16) unsigned char tile[];
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = (size_t)block;
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  const bool live = (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (!a.first_only || (flags & SMX_F_FIRST));
  if (!live) return;  // uniform for the whole workgroup
  const int W = c.dagm_width, H = c.dagm_height;
  const int bytes = W * H;
  for (int k = threadIdx.x; k < bytes / 4; k += SMX_BLOCK) reinterpret_cast<int*>(tile)[k] = 0;
  __syncthreads();
  const double res = c.dagm_resolution;
  const double ex0 = SF(SMX_S_X), ey0 = SF(SMX_S_Y), eh = wrap_heading(SF(SMX_S_HEADING));
  const double rx = cos(eh), ry = sin(eh);    // ego right axis
  const double fx = -sin(eh), fy = cos(eh);   // ego forward axis
  road_layer<255>(a, tile, W, H, res, ex0, ey0, rx, ry, fx, fy);
  __syncthreads();
  int4* dst = reinterpret_cast<int4*>(a.out.dagm + gid * (size_t)bytes);
  for (int k = threadIdx.x; k < bytes / 16; k += SMX_BLOCK) dst[k] = reinterpret_cast<const int4*>(tile)[k];
}

// =================================================================================
// RGB role: the top-down RGB camera (RGBSensor, sensors.py:761-794; the image is defined in include/smx.h): one
// workgroup per observing vehicle, a tile of one CLASS byte a pixel in LDS — 0 nothing, 1 road, 2 social vehicle,
// 3 agent vehicle, the highest class that holds — built from the DAGM's road layer and the OGM's footprints, the very
// functions those roles call.  The layers are drawn lowest class first with a workgroup barrier between them, so a
// pixel is only ever raised and plain stores do (no read-modify-write, no race that could lose the larger class).
// Copy-out: a thread turns 16 class bytes into the 48 bytes of their pixels and stores them as three 16-byte vectors;
// thread k's 48 bytes follow thread k - 1's, so the workgroup's stores fill one contiguous span of the image, which is
// written exactly once.
// =================================================================================
#define SMX_RGB_LUT_R 0xD2C05000u   // byte c = the red byte of class c:      0, 80, 192, 210 (colors.py:58-62)
#define SMX_RGB_LUT_GB 0x1EC05000u  // ... its green and its blue byte:       0, 80, 192,  30
__device__ __forceinline__ unsigned rgb_of_class(const unsigned cls) {  // R | G << 8 | B << 16
  const unsigned r = (SMX_RGB_LUT_R >> (8u * cls)) & 0xffu, gb = (SMX_RGB_LUT_GB >> (8u * cls)) & 0xffu;
  return r | (gb << 8) | (gb << 16);
}

__device__ __forceinline__ void rgb_role(const KernelArgs& a, const int block) {
  extern __shared__ __align__(16) unsigned char tile[];
  const smx_config& c = a.cfg;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  const size_t gid = (size_t)block;
  if (gid >= total) return;
  const int flags = a.st.flags[gid];
  const bool live = (flags & SMX_F_ALIVE) && !(flags & SMX_F_SOCIAL) && (!a.first_only || (flags & SMX_F_FIRST));
  if (!live) return;  // uniform for the whole workgroup
  const int W = c.rgb_width, H = c.rgb_height;
  const int n_veh = c.num_vehicles;
  const int env = (int)(gid / n_veh);
  const int bytes = W * H;
  for (int k = threadIdx.x; k < bytes / 4; k += SMX_BLOCK) reinterpret_cast<int*>(tile)[k] = 0;
  __syncthreads();
  const double res = c.rgb_resolution;
  const double ex0 = SF(SMX_S_X), ey0 = SF(SMX_S_Y), eh = wrap_heading(SF(SMX_S_HEADING));
  const double rx = cos(eh), ry = sin(eh);    // ego right axis
  const double fx = -sin(eh), fy = cos(eh);   // ego forward axis
  road_layer<1>(a, tile, W, H, res, ex0, ey0, rx, ry, fx, fy);
  __syncthreads();
  // the env's alive vehicles, the observer among them: the social ones (class 2), then the agents (class 3)
  __shared__ OgmMate mates[SMX_BLOCK];
  for (int cls = 2; cls <= 3; ++cls) {
    for (int base = 0; base < n_veh; base += SMX_BLOCK) {
      const int j = base + (int)threadIdx.x;
      bool in_view = false;
      if (j < n_veh) {
        const size_t og = (size_t)env * n_veh + j;
        const int f = a.st.flags[og];
        if ((f & SMX_F_ALIVE) && ((f & SMX_F_SOCIAL) != 0) == (cls == 2))
          in_view = ogm_mate_footprint(a, og, total, W, H, res, ex0, ey0, rx, ry, fx, fy, mates[threadIdx.x]);
      }
      unsigned long long todo = __ballot(in_view);
      __syncthreads();
      while (todo != 0ull) {  // uniform
        const int idx = __ffsll((long long)todo) - 1;
        const OgmMate q = mates[idx];
        todo &= todo - 1ull;
        const size_t og = (size_t)env * n_veh + base + idx;
        if (cls == 2)
          ogm_draw_mate<2>(a, og, tile, q, W, H, res);
        else
          ogm_draw_mate<3>(a, og, tile, q, W, H, res);
      }
      __syncthreads();  // the stage is reused, and the next class goes on top of this one
    }
  }
  uint4* dst = reinterpret_cast<uint4*>(a.rgb + gid * (size_t)bytes * 3);
  for (int k = threadIdx.x; k < bytes / 16; k += SMX_BLOCK) {
    const uint4 cls4 = reinterpret_cast<const uint4*>(tile)[k];
    const unsigned cw[4] = {cls4.x, cls4.y, cls4.z, cls4.w};
    unsigned w[12];
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // four pixels -> twelve bytes: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
      const unsigned p0 = rgb_of_class(cw[g] & 3u), p1 = rgb_of_class((cw[g] >> 8) & 3u);
      const unsigned p2 = rgb_of_class((cw[g] >> 16) & 3u), p3 = rgb_of_class((cw[g] >> 24) & 3u);
      w[3 * g] = p0 | (p1 << 24);
      w[3 * g + 1] = (p1 >> 8) | (p2 << 16);
      w[3 * g + 2] = (p2 >> 16) | (p3 << 8);
    }
    dst[3 * k] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[3 * k + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    dst[3 * k + 2] = make_uint4(w[8], w[9], w[10], w[11]);
  }
}

// single-role launches: large batches (each role then keeps its own register / LDS footprint and
// occupancy; forcing more wavefronts per SIMD onto k_waypoints / k_observe by waves_per_eu cost more
// in spills than it won: +20 % on loop 4096 x 32) and OGM tiles too large to ride along as dynamic LDS of every k_sensors workgroup
__global__ void __launch_bounds__(SMX_BLOCK) k_ogm(const KernelArgs a) { ogm_role(a, (int)blockIdx.x); }
__global__ void __launch_bounds__(SMX_BLOCK) k_dagm(const KernelArgs a) { dagm_role(a, (int)blockIdx.x); }
__global__ void __launch_bounds__(SMX_BLOCK) k_rgb(const KernelArgs a) { rgb_role(a, (int)blockIdx.x); }

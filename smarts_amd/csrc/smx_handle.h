// smx_handle.h — the handle of the C-ABI (include/smx.h) and everything it owns: device allocations, side streams,
// event pools, and the bindings smx_load_map / smx_set_* make.  No kernel, no launch, no __device__: smx_kernels.hip
// includes it (as does smx_tick.h, for CtrlHandoff and SMX_SEG_STRIDE) and forwards its extern "C" entry points here,
// and tests/native/host_handle.cpp compiles it with g++ over a host stand-in of the HIP memory calls, under
// AddressSanitizer and UBSan, with every HIP call failing in turn.
//
// Three rules hold throughout:
//   One owner.  A device allocation is a DeviceBlob member of the handle and is freed by it alone; the side streams and
//     the event pools destroy themselves.  smx_destroy synchronises the side streams and deletes the handle.
//   Fill, then commit.  A table is allocated and filled in a local DeviceBlob; only after the last fill succeeded is it
//     moved into the handle and are the pointers the kernels get (map, knots, ctrl, missions, history, dims) set.  After
//     a failed call every such pointer is null or points into an allocation the handle owns.
//   The drop rule, once.  What a new binding drops is written in the unbind_* functions below and nowhere else:
//       a new map       drops missions (-> goals), the history (-> dims, history agents -> handover) and the agents' dimensions;
//                       keeps vias, lidar rays, the image buffer and the frame stacks; re-checks the guard margin
//       new missions    drop the goals and invalidate the knot keys
//       a mission pool  (smx_set_mission_pool, bind or unbind) drops the per-slot missions, goals and vias and invalidates
//                       the knot keys; while it is bound the three per-slot calls are refused (SMX_ERR_STATE); a new map
//                       drops it with its vias
//       a new history   (bind or unbind) drops dims, history agents and handover, and the carried alive list; it keeps
//                       the agents' dimensions (smx_set_agent_dims: they name no vehicle of the history), whose triples
//                       move into a fresh triple block
//       history agents  (bind or unbind) drop the handover table, the bubbles and the action / status rows
//       a new map       also drops the agents' entry table (smx_set_agent_entry: its check points lie on the old map)
//       agent spaces    (smx_set_agent_spaces, bind or unbind) drop nothing, and a new map keeps the table: it names agent
//                       slots, nothing of the map
//   What does not combine is refused, once, in entry_conflict below: the entry table beside history agents (and so their
//   handover table and bubbles) or a frame stack — whichever is bound second is refused; and in spaces_conflict: the
//   kinematic bindings (history agents, handover, bubbles, agent dimensions) beside a table of agent spaces.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "smx_bubbles.h"
#include "smx_guard.h"
#include "smx_history.h"
#include "smx_host.h"
#include "smx_plan.h"
#include "smx_vehicle.h"  // SMX_CTRL_WPS, SMX_CHASSIS_*; smx_roadmap.h: MissionsDev, KnotLists, KnotRow; smx_device.h: MapDev

// The hand-off of the two-launch controller (k_control_paths -> k_control_law), in the handle's ctrl_blob.
struct CtrlHandoff {
  double* path;  // [SMX_CTRL_WPS][3][E*N]: x, y, heading of the wanted path's waypoints
  int32_t* n;    // [E*N] waypoints held; 0 = no path found (the reference asserts; the last command is kept)
};

// What the kernels get of smx_set_agent_entry (ready null: none bound): the device copy of the two tables and the caller's
// two rows.  ready [rows][E][A] ticks from the reset observation; check [rows][E][A][3] x, y, largest plane dimension.
struct EntryDev {
  const int32_t* ready;
  const double* check;
  int32_t rows;
  uint8_t* status;   // [E*N] SMX_ENTRY_*
  int32_t* entered;  // [E*N]
};

// What the control kernels of smx_step_mixed get of smx_set_agent_spaces (space null: none bound), all in one blob:
//   space [N]      SMX_ACTION_SPACE_* of every slot of an env.  The social slots carry `owner`, the lowest-numbered space
//                  present: that space's launch steps them, so they are stepped once however many launches a tick has.
//   slots [S][N]   per space s (S = SMX_ACTION_SPACE_IMITATION + 1) the slots whose entry in `space` is s, ascending —
//                  the owner's list ends with the social slots — and count[s] how many (the small form's slot lists)
struct AgentSpacesDev {
  const int32_t* space;
  const int32_t* slots;
  int32_t count[SMX_ACTION_SPACE_IMITATION + 1];
  unsigned mask;  // bit s: some AGENT slot has space s
  int32_t owner;
};

// One device allocation: allocates, frees in its destructor, reset() frees now, get<T>() reads the pointer.
struct DeviceBlob {
  void* p = nullptr;
  DeviceBlob() = default;
  DeviceBlob(const DeviceBlob&) = delete;
  DeviceBlob& operator=(const DeviceBlob&) = delete;
  DeviceBlob(DeviceBlob&& o) noexcept : p(o.p) { o.p = nullptr; }
  DeviceBlob& operator=(DeviceBlob&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  ~DeviceBlob() { reset(); }
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  template <class T>
  T* get() const { return static_cast<T*>(p); }
  explicit operator bool() const { return p != nullptr; }
};

// Large batches: the sensor kernels of a tick are independent of each other (they read the pose and write
// disjoint rows) and are bound by different things — waypoint chain walks by load latency, OGM tiles by
// their own write stream — so they are enqueued on side streams between two events and overlap.
struct SideStreams {
  hipStream_t side[3] = {};
  hipEvent_t ev_fork = nullptr, ev_fork_grid = nullptr, ev_join[3] = {};
  bool ready = false;
  SideStreams() = default;
  SideStreams(const SideStreams&) = delete;
  SideStreams& operator=(const SideStreams&) = delete;
  ~SideStreams() { destroy(); }
  // lowest priority (bit i of `prio_mask` set: default priority for stream i): the caller's stream carries the tick's
  // critical chain (control -> seeds -> waypoints); the side kernels fill the chip around it instead of sharing it
  // evenly.  A creation that fails part-way releases what it had made.
  hipError_t create(int prio_mask) {
    int prio_least = 0, prio_greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) {
      e = hipStreamCreateWithPriority(&side[i], hipStreamNonBlocking, ((prio_mask >> i) & 1) ? 0 : prio_least);
      if (e != hipSuccess) side[i] = nullptr;
      else if ((e = hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming)) != hipSuccess) ev_join[i] = nullptr;
    }
    if (e == hipSuccess && (e = hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming)) != hipSuccess) ev_fork = nullptr;
    if (e == hipSuccess && (e = hipEventCreateWithFlags(&ev_fork_grid, hipEventDisableTiming)) != hipSuccess) ev_fork_grid = nullptr;
    if (e == hipSuccess) ready = true;
    else destroy();
    return e;
  }
  void synchronize() {
    for (hipStream_t s : side)
      if (s) (void)hipStreamSynchronize(s);
  }
  void destroy() {
    for (int i = 0; i < 3; ++i) {
      if (side[i]) (void)hipStreamDestroy(side[i]);
      if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
      side[i] = nullptr, ev_join[i] = nullptr;
    }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_fork_grid) (void)hipEventDestroy(ev_fork_grid);
    ev_fork = ev_fork_grid = nullptr;
    ready = false;
  }
};

// The timing events a handle has created so far (enqueue adds to `ev` as ticks are timed).
struct EventPool {
  std::vector<hipEvent_t> ev;
  EventPool() = default;
  EventPool(const EventPool&) = delete;
  EventPool& operator=(const EventPool&) = delete;
  ~EventPool() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

// What this header takes from the kernels' file: the sizes its records fix, and the one launch of smx_load_map.
struct KernelSide {
  int wp_pool;               // SMX_WPE_POOL
  size_t spill_group_bytes;  // SMX_WPE_SPILL_GROUP_BYTES
  int side_prio;             // SMX_SIDE_PRIO
  // k_knot_table over h->map (the map just loaded) into `table`, counting into h->knot_stats, then a synchronisation
  int (*build_knot_table)(smx_handle_s* h, KnotRow* table);
  // the agents' triples of triple block `from` into block `to` (both [num_envs * num_vehicles][3]), then a synchronisation:
  // smx_set_agent_dims' triples outlive the block they were written into (build_dims_blob)
  int (*copy_agent_dims)(smx_handle_s* h, const double* from, double* to);
};

// (created by `new smx_handle_s()`: every member without an initialiser starts as zero)
struct smx_handle_s {
  smx_config cfg;
  int device;
  KernelSide kernels;
  bool map_loaded;
  MapDev map;
  DeviceBlob map_blob;  // one device allocation holding every table
  size_t map_bytes;
  DeviceBlob knots_blob;  // KnotLists of the waypoints sensor (k_wp_walk -> k_waypoints_tables)
  DeviceBlob spill_blob;  // k_waypoints_emit's overflow area (KernelArgs::wp_spill)
  int wp_pool_limit;      // records of k_waypoints_emit's LDS pool in use (smx_debug_set_wp_pool)
  // the map's knot table (k_knot_table, at smx_load_map: the map and cfg.wp_lookahead are what it depends on), its
  // counters — [0] rows tabled, [1] rows on one road, then as 64 bits at [2] the path lanes served
  // (smx_debug_set_knot_table(h, 2)) — and the developer switch
  DeviceBlob knot_table;  // KnotRow [n_lanepoints]
  DeviceBlob knot_stats;  // int32 [4]
  int knot_table_mode = 1;  // 0: the walked lists; 1: the table; 2: the table, counting what it serves
  DeviceBlob alive_blob;    // int32 [total] alive list + two counters (ticks alternate), large batches
  DeviceBlob pending_blob;  // uint8 [total] seed_pending
  DeviceBlob slow_blob;     // int32 [4][total] slow lists of the fast kernels (scan facts, scan seeds, control, waypoint rows) + [2][4] counters (ticks alternate)
  DeviceBlob scan_carry;    // double [6][total]: seeds_carry (x, y, d10^2, d1^2) | facts_carry (x, y) of the seeded scan
  int alive_parity;
  KnotLists knots;
  DeviceBlob ctrl_blob;  // CtrlHandoff of the two-launch controller (k_control_paths -> k_control_law)
  CtrlHandoff ctrl;
  DeviceBlob status_dev;  // int32: SMX_DEVICE_* bits raised by the kernels
  SideStreams streams;
  const double* lidar_rays;
  DeviceBlob vias_dev;     // smx_via [n_vias]
  DeviceBlob via_off_dev;  // int32 [num_vehicles + 1]
  int32_t n_vias;
  DeviceBlob missions_blob;  // device copy of smx_set_missions: goals | last roads | route positions | lane table
  std::vector<int32_t> host_lane_road, host_lane_out_off, host_lane_out_idx;  // kept for smx_set_missions
  DeviceBlob goals_blob;     // device copy of smx_set_mission_goals: goal kinds | lane end headings | dead-end lanes
  std::vector<int32_t> host_route_last;  // smx_set_missions' last roads (-1: empty route), kept for smx_set_mission_goals
  MissionsDev missions;
  // lane_following_controller.py:426-430: place_poles gains clipped to [0.02, 0.04] / [3.4, 4.1];
  // for the sedan they saturate at (0.04, 3.4) for both Lane-space target speeds.
  double heading_gain_pos = 0.04, lateral_gain_pos = 3.4;
  double nb_d2_max;
  int slow_blocks = SMX_HOST_SLOW_BLOCKS;  // grid of the slow lists' kernels (smx_load_map)
  // the alive list k_tail built for the next tick: counters of parity `seg_parity` (the other parity's are zero), built
  // from the flags of `list_state`; the next large-form tick takes it instead of launching k_alive_list
  bool list_ready;
  int seg_parity;
  smx_state list_state;
  int group_parity;  // k_tail's counter of env groups with new vehicles (the other one is zero)
  bool map_junctions;  // lanes of the map split (some lanepoint has several successors)
  double dagm_reach;  // half the widest lane width of the loaded map
  uint8_t* guard_out;  // smx_set_guard: the caller's byte buffer (null: guard off), its margin and the box of the loaded map
  uint64_t guard_count;
  double guard_margin = SMX_GUARD_MARGIN_DEFAULT;
  GuardBox guard_box = {1.0, 1.0, 0.0, 0.0};
  uint8_t* rgb_out;   // smx_set_rgb_output: the caller's image buffer (null: none bound) and the bytes it holds
  uint64_t rgb_count;
  DeviceBlob history_blob;  // smx_set_social_history: device copy of the table, frames | vehicle ids (null: none bound)
  HistoryDev history;  // ... and what the kernels get (vehicle null: none bound; follow: smx_set_history_agents' table)
  float* ha_action;    // smx_set_history_agents: the caller's optional expert-action and status rows
  uint8_t* ha_status;
  int32_t history_max_id;  // the largest vehicle id of the bound table (-1: every cell empty)
  // smx_set_history_bubbles: the bubbles (copied; k_bubbles gets them by value) and the caller's state and cursor rows
  // (bubble_state null: none bound)
  BubbleSet bubbles;
  uint8_t* bubble_state;
  uint8_t* bubble_cursor;
  // OGM delta stores (KernelArgs::ogm_mask): the tiles' piece mask, allocated with the handle when the OGM sensor is on.
  // The caller's out.ogm arrives with every call, so the masks describe the buffer of the last call only: `ogm_rows` is
  // that pointer, and a call that brings another one — or the first call, or the one after smx_invalidate_outputs /
  // smx_set_ogm_delta — sets every bit ahead of its pass (ogm_known false) and so stores whole tiles.
  DeviceBlob ogm_mask;  // unsigned long long
  size_t ogm_mask_bytes;
  const uint8_t* ogm_rows;
  bool ogm_known;
  bool ogm_delta = true;  // smx_set_ogm_delta
  // smx_set_social_history_dims / smx_set_agent_dims.  dims_blob: device copy of the social table (none: zero rows) | the
  // triple per vehicle, which exists while either binding holds; agent_dims_blob: device copy of the agents' table.
  DeviceBlob dims_blob;
  DeviceBlob agent_dims_blob;
  HistoryDimsDev dims;   // ... and what the kernels get (table / agent null: that one not bound; slot null: neither)
  DeviceBlob entry_blob;  // smx_set_agent_entry: device copy of the tables, ready ticks | check rows (null: none bound)
  EntryDev entry;         // ... and what the kernels get (ready null: none bound)
  // a table was bound or unbound since the last smx_reset of every env: the status rows do not describe the episodes yet,
  // so steps are refused until one (enqueue clears it)
  bool entry_reset_needed;
  DeviceBlob spaces_blob;  // smx_set_agent_spaces: device copy of the table and its slot lists (null: none bound)
  AgentSpacesDev spaces;   // ... and what the control kernels of smx_step_mixed get (space null: none bound)
  struct StackBinding {  // smx_bind_frame_stack: one caller-owned stack per (source, layout)
    int32_t source, layout;
    uint8_t* dst;
    uint64_t bytes;
    uint32_t row;  // bytes per agent and frame (the configuration's: it does not change while the handle lives)
  };
  std::vector<StackBinding> stacks;
  int debug_skip;
  int launch_strategy = SMX_LAUNCH_AUTO;  // SMX_LAUNCH_*
  bool timing;
  EventPool ev_pool;  // pairs: [2*i] start, [2*i+1] stop
  size_t ev_used;     // pairs recorded since the last read
  bool phase_timing;
  EventPool ph_pool;  // SMX_PHASE_COUNT + 1 boundary events per step
  size_t ph_used;
  std::string err;
};

static thread_local std::string g_create_err;  // the reason of this thread's last failed smx_create

static int fail(smx_handle h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

#define SMX_HIP(call)                                                                         \
  do {                                                                                        \
    hipError_t e__ = (call);                                                                  \
    if (e__ != hipSuccess) return fail(h, SMX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

// sqrt(d2) <= radius without the square root: the correctly rounded root does not decrease with its argument, so
// the test holds exactly for the squared distances up to a threshold — the largest double whose rounded root is
// still <= radius (found from radius * radius by stepping a few units in the last place).  k_observe takes the
// 32 x 32 distances of an env per tick; the root and its comparison were twenty instructions each.
static double radius_threshold(double radius) {
  if (!(radius >= 0.0)) return -1.0;           // (unlimited: the kernels do not look at it)
  if (std::isinf(radius)) return radius;
  double t = radius * radius;
  if (std::isinf(t)) return t;
  while (t > 0.0 && std::sqrt(t) > radius) t = std::nextafter(t, 0.0);
  for (;;) {
    const double up = std::nextafter(t, INFINITY);
    if (std::isinf(up) || !(std::sqrt(up) <= radius)) break;
    t = up;
  }
  return t;
}

// alive_blob: [E*N] alive list, k_alive_list's two counters, k_tail's [2][8] segment counters and [2] counters of env
// groups with new vehicles (SMX_SEG_STRIDE apart), the list of those groups
#define SMX_SEG_STRIDE 32  // ints between two segment counters (a cache line each)
struct AliveLayout {
  size_t flat, seg, group_count, groups, size;
};
static AliveLayout alive_layout(const smx_config& c) {
  AliveLayout l;
  const size_t total = (size_t)c.num_envs * c.num_vehicles;
  l.flat = total;
  l.seg = (total + 2 + SMX_SEG_STRIDE - 1) / SMX_SEG_STRIDE * SMX_SEG_STRIDE;
  l.group_count = l.seg + 2 * 8 * SMX_SEG_STRIDE;
  l.groups = l.group_count + 2 * SMX_SEG_STRIDE;
  l.size = l.groups + (size_t)c.num_envs;  // (at least one env a group)
  return l;
}

// `bytes` of device memory, every byte `fill`, into `dst` (which stays empty when either step fails)
static hipError_t alloc_filled(DeviceBlob& dst, size_t bytes, int fill) {
  DeviceBlob b;
  hipError_t e = b.alloc(bytes);
  if (e == hipSuccess) e = hipMemset(b.p, fill, bytes);
  if (e == hipSuccess) dst = std::move(b);
  return e;
}

// ---- the drop rule (the caller has waited for the device where launches may still read a table)
static void unbind_goals(smx_handle h) {
  h->goals_blob.reset();
  h->missions.goal_kind = nullptr;
}
static void unbind_vias(smx_handle h) {
  h->vias_dev.reset();
  h->via_off_dev.reset();
  h->n_vias = 0;
}
// (a mission pool — smx_set_mission_pool, missions.rows — lives in the blobs of the per-slot tables it excludes)
static bool pool_bound(const smx_handle_s* h) { return h->missions.rows != nullptr; }
static void unbind_missions(smx_handle h) {
  if (pool_bound(h)) unbind_vias(h);  // a pool's vias are indexed by its missions: they go with it
  h->missions_blob.reset();
  unbind_goals(h);  // goal kinds go with the missions they refine
  h->host_route_last.clear();
  h->missions = MissionsDev{nullptr, nullptr};
  h->map.route_pos = nullptr;
  h->map.route_lane_ok = nullptr;
}
static void unbind_handover(smx_handle h) { h->history.handover = nullptr; }
static void unbind_bubbles(smx_handle h) {
  h->bubbles.n = 0;
  h->bubble_state = nullptr;
  h->bubble_cursor = nullptr;
}
static void unbind_history_agents(smx_handle h) {  // (every buffer is the caller's)
  h->history.follow = nullptr;
  h->history.n_agents = 0;
  unbind_handover(h);  // (the handover table is indexed as the follow table is)
  unbind_bubbles(h);   // (the bubbles' rows and follow_agent are the followers')
  h->ha_action = nullptr;
  h->ha_status = nullptr;
}
// (the social table and the triple block in its blob.  While the agents' dimensions stay bound the caller puts a block
// back at once — install_dims, from a blob it built beforehand: build_dims_blob)
static void unbind_dims(smx_handle h) {
  h->dims_blob.reset();
  h->dims.table = nullptr;
  h->dims.slot = nullptr;
  h->dims.n_ids = 0;
}
static void unbind_agent_dims(smx_handle h) {  // (the caller drops the triple block too when no social table is bound)
  h->agent_dims_blob.reset();
  h->dims.agent = nullptr;
  h->dims.agent_rows = 0;
}
static void unbind_history(smx_handle h) {
  h->history_blob.reset();
  h->history = HistoryDev{};
  unbind_dims(h);  // the per-vehicle dimensions were checked against this history's ids
  unbind_history_agents(h);
}
static void unbind_agent_entry(smx_handle h) {  // (the two rows are the caller's)
  h->entry_blob.reset();
  h->entry = EntryDev{};
}
// The bindings that do not combine with delayed entry (include/smx.h smx_set_agent_entry), asked by whichever is bound
// second: a history agent enters by its recording, not by a ready tick, and the reference hands an entrant a stack shorter
// than the frame stacks here keep.  Empty: no conflict.
enum class Binding { AGENT_ENTRY, HISTORY_AGENTS, FRAME_STACK };
static const char* entry_conflict(const smx_handle_s* h, Binding b) {
  switch (b) {
    case Binding::AGENT_ENTRY:
      if (h->history.follow != nullptr) return "agent entry: history agents are bound (smx_set_history_agents): they enter by their recording";
      if (!h->stacks.empty()) return "agent entry: a frame stack is bound (smx_bind_frame_stack): an entrant's stack is not built";
      return nullptr;
    case Binding::HISTORY_AGENTS:
      return h->entry.ready != nullptr ? "history agents: delayed agent entry is bound (smx_set_agent_entry)" : nullptr;
    case Binding::FRAME_STACK:
      return h->entry.ready != nullptr ? "frame stack: delayed agent entry is bound (smx_set_agent_entry)" : nullptr;
  }
  return nullptr;
}

static void unbind_agent_spaces(smx_handle h) {
  h->spaces_blob.reset();
  h->spaces = AgentSpacesDev{};
}
// The bindings a table of agent spaces is not taken beside (include/smx.h smx_set_agent_spaces): they make some agent a
// kinematic one.  This is the one place the rule stands: the other order, a table bound beside one of them, does not
// occur, since their checks ask for a kinematic cfg.action_space and the table's check refuses one.
static int spaces_conflict(smx_handle h, const char* what) {  // SMX_OK: no conflict
  if (h->spaces.space == nullptr) return SMX_OK;
  return fail(h, SMX_ERR_STATE, std::string(what) + ": per-agent action spaces are bound (smx_set_agent_spaces): every slot of a mixed "
                                                    "fleet drives the Ackermann chassis");
}
// Which tick entry a call may come through: smx_step_mixed with a table bound, the uniform entries without one.
// `acts`: smx_step_mixed's argument (null: a uniform entry, `entry_name` says which).
static int check_step_entry(smx_handle h, const char* entry_name, const smx_mixed_actions* acts, bool mixed_entry) {
  if (!mixed_entry) {
    if (h->spaces.space != nullptr)
      return fail(h, SMX_ERR_STATE, std::string(entry_name) + ": per-agent action spaces are bound (smx_set_agent_spaces); the tick of a "
                                    "mixed fleet is smx_step_mixed");
    return SMX_OK;
  }
  if (h->spaces.space == nullptr) return fail(h, SMX_ERR_STATE, "smx_step_mixed: no table of agent spaces is bound (smx_set_agent_spaces)");
  if (!acts) return fail(h, SMX_ERR_INVALID, "smx_step_mixed: acts is NULL");
  const unsigned m = h->spaces.mask;
  const unsigned floats = (1u << SMX_ACTION_SPACE_CONTINUOUS) | (1u << SMX_ACTION_SPACE_ACTUATOR_DYNAMIC) | (1u << SMX_ACTION_SPACE_LANE_WITH_CONTINUOUS_SPEED);
  const unsigned tracking = (1u << SMX_ACTION_SPACE_TRAJECTORY) | (1u << SMX_ACTION_SPACE_MPC);
  if ((m & (1u << SMX_ACTION_SPACE_LANE)) && !acts->lane_dev)
    return fail(h, SMX_ERR_INVALID, "smx_step_mixed: the table holds Lane slots and lane_dev is NULL");
  if ((m & floats) && !acts->floats_dev)
    return fail(h, SMX_ERR_INVALID, "smx_step_mixed: the table holds Continuous / ActuatorDynamic / LaneWithContinuousSpeed slots and floats_dev is NULL");
  if ((m & tracking) && (!acts->trajectories_dev || !acts->counts_dev))
    return fail(h, SMX_ERR_INVALID, "smx_step_mixed: the table holds Trajectory / MPC slots and trajectories_dev or counts_dev is NULL");
  return SMX_OK;
}

static void destroy_impl(smx_handle h) {
  if (!h) return;
  h->streams.synchronize();
  delete h;
}

// On failure no handle is left behind for the caller to remember to destroy.
static int create_impl(const smx_config* cfg, int device, smx_handle* out, const KernelSide& kernels) {
  if (out) *out = nullptr;
  if (!cfg || !out) return refuse(g_create_err, "smx_create: null config or handle pointer");
  if (const char* why = config_error(*cfg)) return refuse(g_create_err, why);
  const hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return refuse(g_create_err, std::string("hipSetDevice: ") + hipGetErrorString(e), SMX_ERR_HIP);
  smx_handle h = new (std::nothrow) smx_handle_s();
  if (!h) return refuse(g_create_err, "out of memory", SMX_ERR_NOMEM);
  h->cfg = *cfg;
  h->device = device;
  h->kernels = kernels;
  h->wp_pool_limit = kernels.wp_pool;
  h->nb_d2_max = radius_threshold(h->cfg.nb_radius);
  if (h->cfg.sensors & SMX_SENSOR_OGM) {  // the OGM tiles' piece mask; its bits are set by the first call (ogm_known)
    h->ogm_mask_bytes = (size_t)cfg->num_envs * cfg->num_vehicles * smx_ogm_mask_words((size_t)cfg->ogm_width * cfg->ogm_height) * sizeof(unsigned long long);
    const hipError_t em = h->ogm_mask.alloc(h->ogm_mask_bytes);
    if (em != hipSuccess) {
      destroy_impl(h);
      return refuse(g_create_err, std::string("hipMalloc (OGM piece mask): ") + hipGetErrorString(em), SMX_ERR_HIP);
    }
  }
  *out = h;
  return SMX_OK;
}

// From the release of the old map to the last statement the handle has no map (map_loaded false): a failure in between
// leaves it refusing ticks (SMX_ERR_STATE) until a load succeeds (one that fails before it reaches the drop leaves the old
// map's missions and history in their blobs, out of reach, for the next load to drop).  The per-batch storage allocated
// on the first load is kept by later ones.
static int load_map_impl(smx_handle h, const smx_map_tables* t) {
  if (!h || !t) return SMX_ERR_INVALID;
  if (const char* why = map_tables_error(*t)) return fail(h, SMX_ERR_INVALID, why);
  // a bound guard stays bound: its margin against this map's cells (smx_guard.h), its box recomputed below
  if (h->guard_out && !guard_map_ok(*t, h->guard_margin))
    return fail(h, SMX_ERR_INVALID, "state guard: with this margin a cell index of this map's grids would not fit (smx_guard.h, SMX_GUARD_INDEX_MAX)");
  SMX_HIP(hipSetDevice(h->device));
  const size_t total = (size_t)h->cfg.num_envs * h->cfg.num_vehicles;
  const bool waypoints = (h->cfg.sensors & SMX_SENSOR_WAYPOINTS) != 0;
  h->dagm_reach = map_dagm_reach(*t);
  h->map_junctions = map_lanes_split(*t);
  h->slow_blocks = slow_list_blocks(h->map_junctions, total);
  BlobWriter w;
#define ADD(field, type, count) const size_t off_##field = w.add(t->field, (size_t)(count) * sizeof(type));
  SMX_MAP_TABLES(ADD, *t)
#undef ADD
  h->map_loaded = false;
  h->map_blob.reset();
  h->map = MapDev(smx_map_tables{});
  {
    DeviceBlob blob;
    SMX_HIP(blob.alloc(w.host.size()));
    SMX_HIP(hipMemcpy(blob.p, w.host.data(), w.host.size(), hipMemcpyHostToDevice));
    char* base = blob.get<char>();
    MapDev m = *t;  // scalars; every pointer is re-pointed into the device blob
#define PTR(field, type, count) m.field = (const type*)(base + off_##field);
    SMX_MAP_TABLES(PTR, *t)
#undef PTR
    h->map_blob = std::move(blob);
    h->map_bytes = w.host.size();
    h->map = m;
  }
  const size_t nl = t->n_lanes;
  h->host_lane_road.assign(t->lane_road, t->lane_road + nl);
  h->host_lane_out_off.assign(t->lane_out_off, t->lane_out_off + nl + 1);
  h->host_lane_out_idx.assign(t->lane_out_idx, t->lane_out_idx + t->lane_out_off[nl]);
  unbind_missions(h);  // missions name roads of the map they were set for: a new map starts without any
  unbind_history(h);   // a bound traffic history was checked against the old map's grids: a new map starts without one
  unbind_agent_dims(h);  // (the triple block went with the history's dimensions) a new map starts with sedans
  if (h->entry.ready) h->entry_reset_needed = true;
  unbind_agent_entry(h);  // the check points lie on the old map: a new map starts with every agent entering at its reset
  // the tick's alive list (large batches) + its counters, the env groups with new vehicles (alive_layout)
  if (!h->alive_blob) SMX_HIP(alloc_filled(h->alive_blob, alive_layout(h->cfg).size * sizeof(int32_t), 0));
  if (!h->slow_blob) SMX_HIP(alloc_filled(h->slow_blob, SlowLists::size(total) * sizeof(int32_t), 0));
  if (!h->pending_blob) SMX_HIP(alloc_filled(h->pending_blob, total, 0));
  // all ones = NaN: nothing to start a seeded search from yet
  if (!h->scan_carry) SMX_HIP(alloc_filled(h->scan_carry, 6 * total * sizeof(double), 0xff));
  // hand-off storage of the waypoints sensor's chain walks (the library's own: it never leaves the tick)
  if (waypoints && !h->knots_blob) {
    const size_t paths = total * SMX_WP_LANES;
    const size_t off_D = (size_t)(SMX_WPK_CAP + 1) * paths * sizeof(int32_t);
    const size_t off_n = off_D + paths * sizeof(double), off_nk = off_n + paths * sizeof(int16_t);
    const size_t off_end = off_nk + paths * sizeof(int16_t), off_key = off_end + paths * sizeof(int32_t);
    const size_t off_cnt = off_key + 3 * paths * sizeof(int32_t), off_nk16 = off_cnt + paths;
    DeviceBlob blob;
    SMX_HIP(alloc_filled(blob, off_nk16 + paths, 0));
    char* kb = blob.get<char>();
    SMX_HIP(hipMemset(kb + off_key, 0xff, 3 * paths * sizeof(int32_t)));  // no list is valid yet
    h->knots_blob = std::move(blob);
    h->knots.idx = (int32_t*)kb;
    h->knots.D = (double*)(kb + off_D);
    h->knots.n = (int16_t*)(kb + off_n);
    h->knots.nk = (int16_t*)(kb + off_nk);
    h->knots.end16 = (int32_t*)(kb + off_end);
    h->knots.key = (int32_t*)(kb + off_key);
    h->knots.cnt = (uint8_t*)(kb + off_cnt);
    h->knots.nk16 = (uint8_t*)(kb + off_nk16);
  }
  h->knot_table.reset();  // (the rows of the map before)
  if (waypoints) {
    if (!h->knot_stats) SMX_HIP(h->knot_stats.alloc(4 * sizeof(int32_t)));
    SMX_HIP(hipMemset(h->knot_stats.p, 0, 4 * sizeof(int32_t)));
    DeviceBlob table;
    SMX_HIP(table.alloc((size_t)t->n_lanepoints * sizeof(KnotRow)));
    const int rc = h->kernels.build_knot_table(h, table.get<KnotRow>());
    if (rc != SMX_OK) return rc;
    h->knot_table = std::move(table);
  }
  if (waypoints && !h->spill_blob) {
    // a region of (SMX_WPE_KNOTS + 1) knot records + lanes per column of every k_waypoints_emit workgroup: 1.6 KB per
    // vehicle (the outputs are 8 KB), touched only by the few workgroups of a tick whose paths outgrow the LDS pool
    const size_t group_vehicles = SMX_BLOCK / SMX_WP_LANES;  // (SMX_WPT_VEHICLES)
    SMX_HIP(h->spill_blob.alloc((total + group_vehicles - 1) / group_vehicles * h->kernels.spill_group_bytes));
  }
  if (!h->status_dev) SMX_HIP(alloc_filled(h->status_dev, sizeof(int32_t), 0));
  if (!h->ctrl_blob) {
    const size_t path_bytes = (size_t)SMX_CTRL_WPS * 3 * total * sizeof(double);
    SMX_HIP(alloc_filled(h->ctrl_blob, path_bytes + total * sizeof(int32_t), 0));
    h->ctrl.path = h->ctrl_blob.get<double>();
    h->ctrl.n = (int32_t*)(h->ctrl_blob.get<char>() + path_bytes);
  }
  if (!h->streams.ready) SMX_HIP(h->streams.create(h->kernels.side_prio));
  h->guard_box = guard_box_of(*t, h->guard_margin);
  h->map_loaded = true;
  return SMX_OK;
}

static int set_vias_impl(smx_handle h, const smx_via* vias_host, int32_t n, const int32_t* slot_off_host) {
  if (!h) return SMX_ERR_INVALID;
  if (pool_bound(h)) return fail(h, SMX_ERR_STATE, "smx_set_vias: a mission pool is bound (smx_set_mission_pool holds the vias; a NULL pool unbinds it)");
  if (n < 0 || (n > 0 && (!vias_host || !slot_off_host))) return fail(h, SMX_ERR_INVALID, "smx_set_vias: null table");
  if (n > 0 && h->cfg.via_max <= 0) return fail(h, SMX_ERR_INVALID, "smx_set_vias: cfg.via_max is 0");
  if (n > 0 && !h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_set_vias needs the map (lane indices are checked)");
  const int nv = h->cfg.num_vehicles;
  if (n > 0) {
    if (slot_off_host[0] != 0 || slot_off_host[nv] != n) return fail(h, SMX_ERR_INVALID, "smx_set_vias: slot offsets");
    for (int s = 0; s < nv; ++s)
      if (slot_off_host[s + 1] < slot_off_host[s] || slot_off_host[s + 1] - slot_off_host[s] > 32)
        return fail(h, SMX_ERR_INVALID, "smx_set_vias: at most 32 vias per agent, offsets ascending");
    for (int i = 0; i < n; ++i)
      if (vias_host[i].lane < 0 || vias_host[i].lane >= h->map.n_lanes)
        return fail(h, SMX_ERR_INVALID, "smx_set_vias: lane index out of range");
  }
  SMX_HIP(hipSetDevice(h->device));
  unbind_vias(h);
  if (n == 0) return SMX_OK;
  DeviceBlob vias, offs;
  SMX_HIP(vias.alloc((size_t)n * sizeof(smx_via)));
  SMX_HIP(offs.alloc((size_t)(nv + 1) * sizeof(int32_t)));
  SMX_HIP(hipMemcpy(vias.p, vias_host, (size_t)n * sizeof(smx_via), hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(offs.p, slot_off_host, (size_t)(nv + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  h->vias_dev = std::move(vias);
  h->via_off_dev = std::move(offs);
  h->n_vias = n;
  return SMX_OK;
}

static int set_missions_impl(smx_handle h, const smx_mission* missions_host, int32_t n_slots, const int32_t* route_roads_host,
                             int32_t n_route_roads) {
  if (!h) return SMX_ERR_INVALID;
  if (pool_bound(h)) return fail(h, SMX_ERR_STATE, "smx_set_missions: a mission pool is bound (smx_set_mission_pool; a NULL pool unbinds it)");
  if (!h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_set_missions needs the map (road indices are checked)");
  if (n_slots < 0 || n_route_roads < 0 || (n_slots > 0 && !missions_host) || (n_route_roads > 0 && !route_roads_host))
    return fail(h, SMX_ERR_INVALID, "smx_set_missions: null table");
  const int nv = h->cfg.num_vehicles, nr = h->map.n_roads;
  if (n_slots != 0 && n_slots != nv) return fail(h, SMX_ERR_INVALID, "smx_set_missions: one mission per vehicle slot (cfg.num_vehicles)");
  if ((size_t)nv * (size_t)nr > 0x7fffffffull) return fail(h, SMX_ERR_INVALID, "smx_set_missions: slots x roads too large");
  RouteTables rt;
  if (const char* why = route_tables(missions_host, n_slots, route_roads_host, n_route_roads, nr, h->map.n_lanes, h->host_lane_road,
                                     h->host_lane_out_off, h->host_lane_out_idx, rt))
    return fail(h, SMX_ERR_INVALID, why);
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  unbind_missions(h);
  // the knot lists of the previous tick were walked under the old routes
  if (h->knots_blob && h->knots.key)
    SMX_HIP(hipMemset(h->knots.key, 0xff, 3 * (size_t)h->cfg.num_envs * nv * SMX_WP_LANES * sizeof(int32_t)));
  h->host_route_last = rt.last;
  if (!rt.any) return SMX_OK;
  const size_t goal_bytes = rt.goal.size() * sizeof(double), last_bytes = rt.last.size() * sizeof(int32_t),
               pos_bytes = rt.pos.size() * sizeof(int16_t);
  const size_t off_last = goal_bytes, off_pos = (goal_bytes + last_bytes + 7) & ~(size_t)7;
  const size_t off_lane = (off_pos + pos_bytes + 7) & ~(size_t)7;
  DeviceBlob blob;
  SMX_HIP(blob.alloc(off_lane + rt.lane_ok.size()));
  char* base = blob.get<char>();
  SMX_HIP(hipMemcpy(base, rt.goal.data(), goal_bytes, hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(base + off_last, rt.last.data(), last_bytes, hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(base + off_pos, rt.pos.data(), pos_bytes, hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(base + off_lane, rt.lane_ok.data(), rt.lane_ok.size(), hipMemcpyHostToDevice));
  h->missions_blob = std::move(blob);
  h->missions.goal = (const double*)base;
  h->missions.route_last = (const int32_t*)(base + off_last);
  h->map.route_pos = (const int16_t*)(base + off_pos);
  h->map.route_lane_ok = (const uint8_t*)(base + off_lane);
  return SMX_OK;
}

static int set_mission_goals_impl(smx_handle h, const smx_mission_goal* goals_host, int32_t n_slots, const double* lane_end_heading_host,
                                  const int32_t* lane_dead_end_host, int32_t n_lanes) {
  if (!h) return SMX_ERR_INVALID;
  if (pool_bound(h)) return fail(h, SMX_ERR_STATE, "smx_set_mission_goals: a mission pool is bound (smx_set_mission_pool holds the goal kinds; a NULL pool unbinds it)");
  if (!h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_set_mission_goals needs the map (the lane tables are checked against it)");
  const int nv = h->cfg.num_vehicles, nl = h->map.n_lanes;
  const std::string msg = mission_goals_error(goals_host, n_slots, nv, lane_end_heading_host, lane_dead_end_host, n_lanes, nl);
  if (!msg.empty()) return fail(h, SMX_ERR_INVALID, msg);
  bool any = false, traverse = false;
  if (const char* why = mission_goals_route_error(goals_host, n_slots, h->host_route_last, any, traverse)) return fail(h, SMX_ERR_INVALID, why);
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  unbind_goals(h);
  if (!any) return SMX_OK;
  const size_t kind_bytes = (size_t)nv * sizeof(smx_mission_goal);
  const size_t head_bytes = traverse ? (size_t)nl * sizeof(double) : 0, dead_bytes = traverse ? (size_t)nl * sizeof(int32_t) : 0;
  DeviceBlob blob;
  SMX_HIP(blob.alloc(kind_bytes + head_bytes + dead_bytes));
  char* base = blob.get<char>();
  SMX_HIP(hipMemcpy(base, goals_host, kind_bytes, hipMemcpyHostToDevice));
  if (traverse) {
    SMX_HIP(hipMemcpy(base + kind_bytes, lane_end_heading_host, head_bytes, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(base + kind_bytes + head_bytes, lane_dead_end_host, dead_bytes, hipMemcpyHostToDevice));
  }
  h->goals_blob = std::move(blob);
  h->missions.goal_kind = (const smx_mission_goal*)base;
  return SMX_OK;
}

// One table of a pool into a fresh allocation (`bytes` > 0)
static hipError_t upload(DeviceBlob& dst, const void* src, size_t bytes) {
  hipError_t e = dst.alloc(bytes);
  if (e == hipSuccess) e = hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice);
  return e;
}

static int set_mission_pool_impl(smx_handle h, const smx_mission_pool* pool) {
  if (!h) return SMX_ERR_INVALID;
  const size_t key_bytes = 3 * (size_t)h->cfg.num_envs * h->cfg.num_vehicles * SMX_WP_LANES * sizeof(int32_t);
  if (!pool) {  // unbind: every mission endless again, no vias
    if (!pool_bound(h)) return SMX_OK;
    SMX_HIP(hipSetDevice(h->device));
    SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the tables
    unbind_missions(h);
    if (h->knots_blob && h->knots.key) SMX_HIP(hipMemset(h->knots.key, 0xff, key_bytes));
    return SMX_OK;
  }
  if (!h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_set_mission_pool needs the map (road and lane indices are checked)");
  MissionPoolTables t;
  const std::string msg = mission_pool_error(h->cfg, *pool, h->map.n_roads, h->map.n_lanes, h->host_lane_road, h->host_lane_out_off, h->host_lane_out_idx, t);
  if (!msg.empty()) return fail(h, SMX_ERR_INVALID, msg);
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old tables
  // the knot lists of the previous tick were walked under the old routes (harmless should a fill below fail: a list
  // without a key is walked again)
  if (h->knots_blob && h->knots.key) SMX_HIP(hipMemset(h->knots.key, 0xff, key_bytes));
  const int M = pool->n_missions, nl = h->map.n_lanes;
  // fill ...
  DeviceBlob missions, goals, vias, offs;
  size_t off_last = 0, off_pos = 0, off_lane = 0;
  if (t.rt.any) {
    const size_t goal_bytes = t.rt.goal.size() * sizeof(double), last_bytes = t.rt.last.size() * sizeof(int32_t),
                 pos_bytes = t.rt.pos.size() * sizeof(int16_t);
    off_last = goal_bytes, off_pos = (goal_bytes + last_bytes + 7) & ~(size_t)7;
    off_lane = (off_pos + pos_bytes + 7) & ~(size_t)7;
    SMX_HIP(missions.alloc(off_lane + t.rt.lane_ok.size()));
    char* base = missions.get<char>();
    SMX_HIP(hipMemcpy(base, t.rt.goal.data(), goal_bytes, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(base + off_last, t.rt.last.data(), last_bytes, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(base + off_pos, t.rt.pos.data(), pos_bytes, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(base + off_lane, t.rt.lane_ok.data(), t.rt.lane_ok.size(), hipMemcpyHostToDevice));
  }
  if (!t.goals.empty()) {
    const size_t kind_bytes = t.goals.size() * sizeof(smx_mission_goal);
    const size_t head_bytes = t.traverse ? (size_t)nl * sizeof(double) : 0, dead_bytes = t.traverse ? (size_t)nl * sizeof(int32_t) : 0;
    SMX_HIP(goals.alloc(kind_bytes + head_bytes + dead_bytes));
    char* base = goals.get<char>();
    SMX_HIP(hipMemcpy(base, t.goals.data(), kind_bytes, hipMemcpyHostToDevice));
    if (t.traverse) {
      SMX_HIP(hipMemcpy(base + kind_bytes, pool->lane_end_heading_host, head_bytes, hipMemcpyHostToDevice));
      SMX_HIP(hipMemcpy(base + kind_bytes + head_bytes, pool->lane_dead_end_host, dead_bytes, hipMemcpyHostToDevice));
    }
  }
  if (pool->n_vias > 0) {
    SMX_HIP(upload(vias, pool->vias_host, (size_t)pool->n_vias * sizeof(smx_via)));
    SMX_HIP(upload(offs, t.via_off.data(), t.via_off.size() * sizeof(int32_t)));
  }
  // ... then commit: the per-slot tables and vias go, the pool's take their places
  unbind_missions(h);
  unbind_vias(h);
  h->host_route_last.clear();  // (smx_set_mission_goals is refused while the pool is bound)
  if (missions) {
    char* base = missions.get<char>();
    h->missions_blob = std::move(missions);
    h->missions.goal = (const double*)base;
    h->missions.route_last = (const int32_t*)(base + off_last);
    h->map.route_pos = (const int16_t*)(base + off_pos);
    h->map.route_lane_ok = (const uint8_t*)(base + off_lane);
  }
  if (goals) {
    h->missions.goal_kind = goals.get<smx_mission_goal>();
    h->goals_blob = std::move(goals);
  }
  if (vias) {
    h->vias_dev = std::move(vias);
    h->via_off_dev = std::move(offs);
    h->n_vias = pool->n_vias;
  }
  h->missions.rows = pool->rows_dev;
  h->missions.n_rows = pool->rows;
  h->missions.n = M;
  return SMX_OK;
}

static int set_lidar_rays_impl(smx_handle h, const double* rays_dev, int32_t n_rays) {
  if (!h) return SMX_ERR_INVALID;
  if (n_rays != h->cfg.lidar_rays) return fail(h, SMX_ERR_INVALID, "n_rays != cfg.lidar_rays");
  h->lidar_rays = rays_dev;
  return SMX_OK;
}

static int set_rgb_output_impl(smx_handle h, uint8_t* rgb_dev, uint64_t count) {
  if (!h) return SMX_ERR_INVALID;
  if (!rgb_dev) {  // unbind
    h->rgb_out = nullptr;
    h->rgb_count = 0;
    return SMX_OK;
  }
  if (!(h->cfg.sensors & SMX_SENSOR_RGB))
    return fail(h, SMX_ERR_STATE, "smx_set_rgb_output: the configuration has no SMX_SENSOR_RGB");
  if ((reinterpret_cast<uintptr_t>(rgb_dev) & 15) != 0)
    return fail(h, SMX_ERR_INVALID, "rgb output: the buffer must be 16-byte aligned (it is written with 16-byte stores)");
  std::string msg;
  const int rc = check_rgb_output_impl(h->cfg, count, msg);
  if (rc != SMX_OK) return fail(h, rc, msg);
  h->rgb_out = rgb_dev;
  h->rgb_count = count;
  return SMX_OK;
}

static int set_guard_impl(smx_handle h, uint8_t* guard_dev, uint64_t count, double margin) {
  if (!h) return SMX_ERR_INVALID;
  if (!guard_dev) {  // guard off
    h->guard_out = nullptr;
    h->guard_count = 0;
    return SMX_OK;
  }
  std::string msg;
  const int rc = check_guard_impl(h->cfg, count, margin, msg);
  if (rc != SMX_OK) return fail(h, rc, msg);
  // (before a map is loaded, smx_load_map makes this check)
  if (h->map_loaded && !guard_map_ok(h->map, margin))
    return fail(h, SMX_ERR_INVALID, "state guard: with this margin a cell index of the loaded map's grids would not fit (smx_guard.h, SMX_GUARD_INDEX_MAX)");
  h->guard_out = guard_dev;
  h->guard_count = count;
  h->guard_margin = margin;
  if (h->map_loaded) h->guard_box = guard_box_of(h->map, margin);
  return SMX_OK;
}

// The dims blob afresh, filled and not yet committed: `social`'s table (null: zero rows) | a triple per vehicle of the
// batch — the sedan's until a replayed slot's pose or an agent's spawn pose is written, but for the agents' triples of the
// block in place, which are carried over while their table is bound (an agent keeps its size until it is respawned).
static int build_dims_blob(smx_handle h, const smx_social_dims* social, DeviceBlob& out) {
  const size_t table_words = social ? (size_t)social->n_ids * 3 : 0;
  const size_t total = (size_t)h->cfg.num_envs * (size_t)h->cfg.num_vehicles;
  std::vector<double> host(table_words + total * 3);
  if (social) std::copy(social->dims_host, social->dims_host + table_words, host.begin());
  double* slot = host.data() + table_words;
  for (size_t g = 0; g < total; ++g) {
    slot[g * 3 + 0] = SMX_CHASSIS_LENGTH;
    slot[g * 3 + 1] = SMX_CHASSIS_WIDTH;
    slot[g * 3 + 2] = SMX_CHASSIS_HEIGHT;
  }
  DeviceBlob blob;
  SMX_HIP(blob.alloc(host.size() * sizeof(double)));
  SMX_HIP(hipMemcpy(blob.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
  if (h->dims.agent != nullptr && h->dims.slot != nullptr) {
    const int rc = h->kernels.copy_agent_dims(h, h->dims.slot, blob.get<double>() + table_words);
    if (rc != SMX_OK) return rc;
  }
  out = std::move(blob);
  return SMX_OK;
}
// ... committed (after unbind_dims): the blob and the pointers into it
static void install_dims(smx_handle h, DeviceBlob&& blob, const smx_social_dims* social) {
  const size_t table_words = social ? (size_t)social->n_ids * 3 : 0;
  h->dims_blob = std::move(blob);
  h->dims.table = social ? h->dims_blob.get<double>() : nullptr;
  h->dims.slot = h->dims_blob.get<double>() + table_words;
  h->dims.n_ids = social ? social->n_ids : 0;
}

static int set_social_history_impl(smx_handle h, const smx_social_history* hist) {
  if (!h) return SMX_ERR_INVALID;
  if (hist) {
    if (!h->map_loaded) return fail(h, SMX_ERR_STATE, "smx_set_social_history needs the map (the rows are checked against its grids)");
    std::string msg;
    const int rc = check_social_history_impl(h->cfg, h->map, *hist, msg);  // (the grid extents are scalars: the device copy of the tables has them)
    if (rc != SMX_OK) return fail(h, rc, msg);
  }
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  DeviceBlob kept;  // the agents' dimensions outlive the history: their triples, in a block without a social table
  if (h->dims.agent != nullptr) {
    const int rc = build_dims_blob(h, nullptr, kept);
    if (rc != SMX_OK) return rc;
  }
  unbind_history(h);
  if (kept) install_dims(h, std::move(kept), nullptr);
  // the alive list k_tail built for the next tick was built under the other rule (smx_plan.h: tail_builds_list)
  h->list_ready = false;
  if (!hist) return SMX_OK;
  const size_t cells = (size_t)hist->n_frames * (size_t)hist->num_social;
  const size_t frame_bytes = cells * 4 * sizeof(double), id_bytes = cells * sizeof(int32_t);
  DeviceBlob blob;
  SMX_HIP(blob.alloc(frame_bytes + id_bytes));
  char* base = blob.get<char>();
  SMX_HIP(hipMemcpy(base, hist->frames_host, frame_bytes, hipMemcpyHostToDevice));
  SMX_HIP(hipMemcpy(base + frame_bytes, hist->vehicle_host, id_bytes, hipMemcpyHostToDevice));
  HistoryDev d{};
  d.frames = (const double*)base;
  d.vehicle = (const int32_t*)(base + frame_bytes);
  d.start_frame = hist->start_frame_dev;
  d.replaced = hist->replaced_dev;
  d.n_frames = hist->n_frames;
  d.num_social = hist->num_social;
  d.rows = hist->rows;
  d.num_envs = h->cfg.num_envs;
  h->history_blob = std::move(blob);
  h->history = d;
  h->history_max_id = social_history_max_id(*hist);
  return SMX_OK;
}

static int set_social_history_dims_impl(smx_handle h, const smx_social_dims* dims) {
  if (!h) return SMX_ERR_INVALID;
  if (dims) {
    if (h->history.vehicle == nullptr) return fail(h, SMX_ERR_STATE, "smx_set_social_history_dims needs a bound history (smx_set_social_history)");
    std::string msg;
    const int rc = check_social_dims_impl(*dims, h->history_max_id, msg);
    if (rc != SMX_OK) return fail(h, rc, msg);
  }
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  if (!dims && h->dims.agent == nullptr) {
    unbind_dims(h);
    return SMX_OK;
  }
  DeviceBlob blob;  // (with the agents' dimensions bound an unbind leaves a block without a social table)
  const int rc = build_dims_blob(h, dims, blob);
  if (rc != SMX_OK) return rc;
  unbind_dims(h);
  install_dims(h, std::move(blob), dims);
  return SMX_OK;
}

static int set_agent_dims_impl(smx_handle h, const smx_agent_dims* ad) {
  if (!h) return SMX_ERR_INVALID;
  if (ad) {
    if (spaces_conflict(h, "agent dimensions") != SMX_OK) return SMX_ERR_STATE;
    std::string msg;
    const int rc = check_agent_dims_impl(h->cfg, *ad, msg);
    if (rc != SMX_OK) return fail(h, rc, msg);
  }
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  if (!ad) {  // every agent is a sedan again from its next (re)spawn: at once where no block is left to read
    unbind_agent_dims(h);
    if (h->dims.table == nullptr) unbind_dims(h);
    return SMX_OK;
  }
  const size_t words = (size_t)ad->rows * (size_t)h->cfg.num_envs * (size_t)(h->cfg.num_vehicles - h->cfg.num_social) * 3;
  DeviceBlob table, block;
  SMX_HIP(table.alloc(words * sizeof(double)));
  SMX_HIP(hipMemcpy(table.p, ad->dims_host, words * sizeof(double), hipMemcpyHostToDevice));
  if (h->dims.slot == nullptr) {  // (a block in place stays: its agents keep their triples until they are respawned)
    const int rc = build_dims_blob(h, nullptr, block);
    if (rc != SMX_OK) return rc;
  }
  unbind_agent_dims(h);
  h->agent_dims_blob = std::move(table);
  h->dims.agent = h->agent_dims_blob.get<double>();
  h->dims.agent_rows = ad->rows;
  if (block) install_dims(h, std::move(block), nullptr);
  return SMX_OK;
}

static int set_history_agents_impl(smx_handle h, const smx_history_agents* ha) {
  if (!h) return SMX_ERR_INVALID;
  if (ha) {
    if (spaces_conflict(h, "history agents") != SMX_OK) return SMX_ERR_STATE;
    if (h->history.vehicle == nullptr) return fail(h, SMX_ERR_STATE, "smx_set_history_agents needs a bound history (smx_set_social_history)");
    if (const char* why = entry_conflict(h, Binding::HISTORY_AGENTS)) return fail(h, SMX_ERR_STATE, why);
    std::string msg;
    const int rc = check_history_agents_impl(h->cfg, h->history.rows, *ha, msg);
    if (rc != SMX_OK) return fail(h, rc, msg);
  }
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  unbind_history_agents(h);
  if (!ha) return SMX_OK;
  h->history.follow = ha->vehicle_dev;
  h->history.n_agents = h->cfg.num_vehicles - h->cfg.num_social;
  h->ha_action = ha->action_dev;
  h->ha_status = ha->status_dev;
  return SMX_OK;
}

static int set_history_handover_impl(smx_handle h, const smx_history_handover* ho) {
  if (!h) return SMX_ERR_INVALID;
  if (ho) {
    if (spaces_conflict(h, "history handover") != SMX_OK) return SMX_ERR_STATE;
    if (h->history.follow == nullptr) return fail(h, SMX_ERR_STATE, "smx_set_history_handover needs bound history agents (smx_set_history_agents)");
    std::string msg;
    const int rc = check_history_handover_impl(h->cfg, h->history.rows, *ho, msg);
    if (rc != SMX_OK) return fail(h, rc, msg);
  }
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  unbind_handover(h);
  if (ho) h->history.handover = ho->tick_dev;
  return SMX_OK;
}

static int set_history_bubbles_impl(smx_handle h, const smx_history_bubbles* hb) {
  if (!h) return SMX_ERR_INVALID;
  BubbleSet set{};  // filled here, committed after the wait
  if (hb) {
    if (spaces_conflict(h, "history bubbles") != SMX_OK) return SMX_ERR_STATE;
    if (h->history.follow == nullptr) return fail(h, SMX_ERR_STATE, "smx_set_history_bubbles needs bound history agents (smx_set_history_agents)");
    std::string msg;
    const int rc = check_history_bubbles_impl(h->cfg, *hb, msg);
    if (rc != SMX_OK) return fail(h, rc, msg);
    std::copy(hb->bubbles_host, hb->bubbles_host + hb->n_bubbles, set.b);
    set.n = hb->n_bubbles;
  }
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still write the old rows
  unbind_bubbles(h);
  if (!hb) return SMX_OK;
  h->bubbles = set;
  h->bubble_state = hb->state_dev;
  h->bubble_cursor = hb->cursor_dev;
  return SMX_OK;
}

static int set_agent_entry_impl(smx_handle h, const smx_agent_entry* en) {
  if (!h) return SMX_ERR_INVALID;
  DeviceBlob blob;  // ready ticks | check rows, filled here, committed after the wait
  if (en) {
    if (const char* why = entry_conflict(h, Binding::AGENT_ENTRY)) return fail(h, SMX_ERR_STATE, why);
    std::string msg;
    const int rc = check_agent_entry_impl(h->cfg, *en, msg);
    if (rc != SMX_OK) return fail(h, rc, msg);
    const size_t cells = (size_t)en->rows * (size_t)h->cfg.num_envs * (size_t)(h->cfg.num_vehicles - h->cfg.num_social);
    const size_t ready_bytes = (cells * sizeof(int32_t) + 7) / 8 * 8;  // (the check rows start 8-byte aligned)
    SMX_HIP(hipSetDevice(h->device));
    SMX_HIP(blob.alloc(ready_bytes + cells * 3 * sizeof(double)));
    SMX_HIP(hipMemcpy(blob.p, en->ready_host, cells * sizeof(int32_t), hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy((char*)blob.p + ready_bytes, en->check_host, cells * 3 * sizeof(double), hipMemcpyHostToDevice));
  }
  SMX_HIP(hipSetDevice(h->device));
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  if (en || h->entry.ready) h->entry_reset_needed = true;  // (an unbind of nothing changes no episode)
  unbind_agent_entry(h);
  if (!en) return SMX_OK;
  const size_t cells = (size_t)en->rows * (size_t)h->cfg.num_envs * (size_t)(h->cfg.num_vehicles - h->cfg.num_social);
  const size_t ready_bytes = (cells * sizeof(int32_t) + 7) / 8 * 8;
  h->entry_blob = std::move(blob);
  h->entry.ready = h->entry_blob.get<int32_t>();
  h->entry.check = (const double*)((const char*)h->entry_blob.p + ready_bytes);
  h->entry.rows = en->rows;
  h->entry.status = en->status_dev;
  h->entry.entered = en->entered_dev;
  return SMX_OK;
}

// (a new map keeps the table: it names agent slots, nothing of the map.  No reset is needed either way: include/smx.h)
static int set_agent_spaces_impl(smx_handle h, const smx_agent_spaces* as) {
  if (!h) return SMX_ERR_INVALID;
  constexpr int S = SMX_ACTION_SPACE_IMITATION + 1;
  DeviceBlob blob;  // space [N] | slots [S][N], filled here, committed after the wait
  AgentSpacesDev d{};
  if (as) {
    std::string msg;
    const int rc = check_agent_spaces_impl(h->cfg, *as, msg);
    if (rc != SMX_OK) return fail(h, rc, msg);
  }
  SMX_HIP(hipSetDevice(h->device));
  if (as) {
    const int32_t N = h->cfg.num_vehicles, agents = N - h->cfg.num_social;
    d.mask = agent_spaces_mask(as->space_host, agents);
    d.owner = __builtin_ctz(d.mask);
    std::vector<int32_t> host((size_t)(1 + S) * N, -1);
    for (int32_t slot = 0; slot < N; ++slot) {
      const int32_t s = slot < agents ? as->space_host[slot] : d.owner;
      host[slot] = s;
      host[(size_t)(1 + s) * N + d.count[s]++] = slot;
    }
    SMX_HIP(blob.alloc(host.size() * sizeof(int32_t)));
    SMX_HIP(hipMemcpy(blob.p, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  SMX_HIP(hipDeviceSynchronize());  // launches in flight still read the old table
  unbind_agent_spaces(h);
  if (!as) return SMX_OK;
  h->spaces_blob = std::move(blob);
  d.space = h->spaces_blob.get<int32_t>();
  d.slots = d.space + h->cfg.num_vehicles;
  h->spaces = d;
  return SMX_OK;
}

static int bind_frame_stack_impl(smx_handle h, int32_t source, int32_t layout, void* stack_dev, uint64_t bytes) {
  if (!h) return SMX_ERR_INVALID;
  auto at = std::find_if(h->stacks.begin(), h->stacks.end(),
                         [&](const smx_handle_s::StackBinding& b) { return b.source == source && b.layout == layout; });
  if (!stack_dev) {  // unbind
    if (at != h->stacks.end()) h->stacks.erase(at);
    return SMX_OK;
  }
  std::string msg;
  uint64_t row;
  const int rc = check_frame_stack_impl(h->cfg, source, layout, bytes, row, msg);
  if (rc != SMX_OK) return fail(h, rc, msg);
  if (const char* why = entry_conflict(h, Binding::FRAME_STACK)) return fail(h, SMX_ERR_STATE, why);
  if (layout == SMX_STACK_DSTACK && (reinterpret_cast<uintptr_t>(stack_dev) & 15) != 0)
    return fail(h, SMX_ERR_INVALID, "frame stack: an SMX_STACK_DSTACK buffer must be 16-byte aligned (it is moved with up to 16-byte accesses)");
  if (at != h->stacks.end()) {
    at->dst = (uint8_t*)stack_dev;
    at->bytes = bytes;
    return SMX_OK;
  }
  if (h->stacks.size() >= SMX_STACK_MAX_BINDINGS)
    return fail(h, SMX_ERR_STATE, "frame stack: at most " SMX_STR(SMX_STACK_MAX_BINDINGS) " bindings");
  h->stacks.push_back({source, layout, (uint8_t*)stack_dev, bytes, (uint32_t)row});
  return SMX_OK;
}

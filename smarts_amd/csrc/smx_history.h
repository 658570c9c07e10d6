// smx_history.h — traffic-history replay (include/smx.h, smx_set_social_history): which frame of the recorded table an
// env replays in a pass, whether a social slot holds a vehicle there, and the row it takes its pose from, each written
// once.  social_vehicle_step (every control form), respawn_vehicle (k_reset and the commit-time respawn) and commit_role
// call these, and the history agents (smx_set_history_agents: respawn_vehicle, k_control_kinematic's FOLLOW and HANDOVER
// forms); the header holds no HIP and also compiles for the host (tests/native/host_history.cpp, host_history_dims.cpp,
// host_history_agents.cpp and host_history_handover.cpp drive it under AddressSanitizer + UBSan).  The second half is the per-vehicle dimensions
// (smx_set_social_history_dims): the id -> (length, width, height) lookup the same writers use.
//
// Nothing read from the two caller-owned tables can take an index out of a table: the row of start_frame / replaced is
// (episode mod rows) brought into [0, rows), the env is the kernel's own, the frame is formed in 64 bits (an int32 start
// plus an int32 tick count cannot overflow them) and compared against [0, n_frames) before it indexes anything, and a
// replaced id is only ever compared.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/smx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMX_HISTORY_FN __host__ __device__ __forceinline__
#else
#define SMX_HISTORY_FN inline
#endif

// The bound history as the kernels see it (vehicle == null: none bound).  frames / vehicle: the handle's device copy of
// smx_social_history's host tables; start_frame / replaced: the caller's device tables.
struct HistoryDev {
  const double* frames;        // [n_frames][num_social][4] x, y, heading, speed
  const int32_t* vehicle;      // [n_frames][num_social], < 0 = empty
  const int32_t* start_frame;  // [rows][num_envs]
  const int32_t* replaced;     // [rows][num_envs], or null
  int32_t n_frames, num_social, rows, num_envs;
  // history agents (smx_set_history_agents; follow == null: none bound): the caller's table of followed vehicle ids
  const int32_t* follow;  // [rows][num_envs][n_agents], < 0 = the agent follows nothing
  int32_t n_agents;       // agent slots of an env (num_vehicles - num_social)
  // the handover table (smx_set_history_handover; null: none bound), indexed as follow is: the tick from which the agent
  // is driven by its action in a tick of smx_step_history_handover, < 0 = never
  const int32_t* handover;  // [rows][num_envs][n_agents]
};

// the row of the two per-env tables that episode `episode` reads (Python's modulo: a negative episode counts from the end)
SMX_HISTORY_FN int history_table_row(const HistoryDev& h, int episode) {
  const int r = episode % h.rows;
  return r < 0 ? r + h.rows : r;
}

// The frame env `env` replays when its observation reports `env_ticks` ticks.
SMX_HISTORY_FN int64_t history_frame(const HistoryDev& h, int episode, int env, int env_ticks) {
  const size_t at = (size_t)history_table_row(h, episode) * (size_t)h.num_envs + (size_t)env;
  return (int64_t)h.start_frame[at] + (int64_t)env_ticks;
}

// Does social slot `slot` (0 .. num_social - 1) of env `env` hold a vehicle in `frame`?
SMX_HISTORY_FN bool history_present(const HistoryDev& h, int episode, int env, int64_t frame, int slot) {
  if (frame < 0 || frame >= (int64_t)h.n_frames) return false;
  const int32_t id = h.vehicle[(size_t)frame * (size_t)h.num_social + (size_t)slot];
  if (id < 0) return false;
  const size_t cell = (size_t)history_table_row(h, episode) * (size_t)h.num_envs + (size_t)env;
  if (h.replaced != nullptr && id == h.replaced[cell]) return false;
  if (h.follow == nullptr) return true;
  // history agents: the recorded vehicle an agent of this env follows is that agent (any value in the table is safe:
  // ids are only compared)
  const int32_t* v = h.follow + cell * (size_t)h.n_agents;
  for (int k = 0; k < h.n_agents; ++k)
    if (v[k] == id) return false;
  return true;
}

// The four words of a present slot (only called when history_present said yes: the frame is in range).
SMX_HISTORY_FN const double* history_row(const HistoryDev& h, int64_t frame, int slot) {
  return h.frames + ((size_t)frame * (size_t)h.num_social + (size_t)slot) * 4;
}

// ---- history agents (smx_set_history_agents) ----
// The vehicle agent `agent` (0 .. n_agents - 1) of env `env` follows in `episode` (only called with follow bound).
SMX_HISTORY_FN int32_t history_followed(const HistoryDev& h, int episode, int env, int agent) {
  return h.follow[((size_t)history_table_row(h, episode) * (size_t)h.num_envs + (size_t)env) * (size_t)h.n_agents + (size_t)agent];
}

// The handover tick of the same agent (only called with follow and handover bound: one index for both tables).
SMX_HISTORY_FN int32_t history_handover(const HistoryDev& h, int episode, int env, int agent) {
  return h.handover[((size_t)history_table_row(h, episode) * (size_t)h.num_envs + (size_t)env) * (size_t)h.n_agents + (size_t)agent];
}
// Is an agent whose handover tick is `handover` driven in the tick that starts with env_ticks = `env_ticks`?  Stateless:
// the value is only compared, so any value is safe (0: from the first tick after the reset; < 0: never).
SMX_HISTORY_FN bool history_driven(int32_t handover, int env_ticks) { return handover >= 0 && env_ticks >= handover; }

// The slot that holds vehicle `id` in `frame`, -1: the frame is outside the table, the id is none (< 0), or the frame
// lacks it.  (`replaced` is not asked: a followed vehicle is hidden from the social slots by its follower.)
SMX_HISTORY_FN int history_find(const HistoryDev& h, int64_t frame, int32_t id) {
  if (id < 0 || frame < 0 || frame >= (int64_t)h.n_frames) return -1;
  const int32_t* ids = h.vehicle + (size_t)frame * (size_t)h.num_social;
  for (int s = 0; s < h.num_social; ++s)
    if (ids[s] == id) return s;
  return -1;
}

// ---- per-vehicle dimensions (smx_set_social_history_dims) ----
// table: the handle's device copy of smx_social_dims (null: none bound, every vehicle has the sedan's box); slot: the
// handle's triple per (env, vehicle), which the writers of a replayed slot's pose write beside it and every consumer
// reads.  agent: the handle's device copy of smx_agent_dims (smx_set_agent_dims; null: none bound), which respawn_vehicle
// writes an agent's triple from (an all-NaN triple: the sedan's).  slot exists when either binding holds — "sized" is
// `slot != null` —; a vehicle whose binding is absent keeps the sedan's triple there.
struct HistoryDimsDev {
  const double* table;  // [n_ids][3] length, width, height
  double* slot;         // [num_envs * num_vehicles][3]
  int32_t n_ids;
  int32_t agent_rows;   // an episode uses row (episode mod agent_rows), as the spawn tables do
  const double* agent;  // [agent_rows][num_envs][num_agents][3]
};

// The triple of the vehicle in `slot` of `frame` (only called when history_present said yes).  The bind-time check
// found every id of the table below n_ids; an id outside it all the same reads row 0, never outside the table.
SMX_HISTORY_FN const double* history_dims_row(const HistoryDev& h, const HistoryDimsDev& d, int64_t frame, int slot) {
  const int32_t id = h.vehicle[(size_t)frame * (size_t)h.num_social + (size_t)slot];
  return d.table + 3 * (size_t)((id >= 0 && id < d.n_ids) ? id : 0);
}

// smx_bubbles.h — the bubble rule (include/smx.h, smx_set_history_bubbles): the reference's
// Bubble.in_bubble_or_airlock, Bubble.admissibility, Cursor.from_pos and the state changes of
// BubbleManager._handle_transitions (bubble_manager.py:154-218, 275-337, 440-463) for PositionalZone bubbles, each written
// once.  k_bubbles calls these with one wavefront per env; the header holds no HIP and also compiles for the host
// (tests/native/host_history_bubbles.cpp drives it in a serial loop under AddressSanitizer + UBSan).
//
// An env's agents are at most 64 (smx_create holds num_vehicles to 64), so a set of agents is a 64-bit mask, bit k = agent
// slot k.  The limits make the pass serial in the agents — agent k's admissibility counts the cursors agents 0 .. k-1 got
// in this pass — and bubble_recurrence is that loop over masks alone: on the device every lane runs it on the same
// (wavefront-uniform) words, on the host it is called as it stands.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/smx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMX_BUBBLES_FN __host__ __device__ __forceinline__
#else
#define SMX_BUBBLES_FN inline
#endif

// The bound bubbles as k_bubbles gets them: by value, its own kernel argument (584 bytes).
struct BubbleSet {
  smx_bubble b[SMX_MAX_BUBBLES];
  int32_t n;
};

// A state that is none of the four: an agent the handover table drives in this tick ("ego": not social, not shadowed, not
// hijacked — it makes no transition and counts in no set of the last pass's states; its cursor still counts).
enum { SMX_BUBBLE_EGO = 4 };
enum BubbleTransition : uint8_t { SMX_BT_NONE = 0, SMX_BT_AIRLOCK_ENTERED = 1, SMX_BT_ENTERED = 2, SMX_BT_EXITED = 3, SMX_BT_AIRLOCK_EXITED = 4 };
enum BubbleCursor : uint8_t { SMX_BC_NONE = 0, SMX_BC_IN_BUBBLE = 1, SMX_BC_IN_AIRLOCK = 2 };

struct BubbleZone {
  bool in_bubble, in_airlock;  // inside the inner rectangle; inside the grown one and not inside the inner one
};

// Bubble.in_bubble_or_airlock for the point (px, py).  A fixed bubble (follow_agent < 0) is centred at (x, y); a
// travelling one lies in the frame of the followed agent, whose position (fx, fy) and heading fh its state holds:
// q = R(-fh) (p - pf) - follow_offset (move_to_follow_vehicle, :225-249, inverted).  Strict: Point.within puts the
// boundary outside.
SMX_BUBBLES_FN BubbleZone bubble_zone(const smx_bubble& b, double px, double py, double fx, double fy, double fh) {
  double qx, qy;
  if (b.follow_agent < 0) {
    qx = px - b.x;
    qy = py - b.y;
  } else {
    const double s = sin(fh), c = cos(fh), dx = px - fx, dy = py - fy;
    qx = c * dx + s * dy - b.offset_x;
    qy = -s * dx + c * dy - b.offset_y;
  }
  const double ax = fabs(qx), ay = fabs(qy), hx = 0.5 * b.size_x, hy = 0.5 * b.size_y;
  BubbleZone z;
  z.in_bubble = ax < hx && ay < hy;
  z.in_airlock = !z.in_bubble && ax < hx + b.margin && ay < hy + b.margin;
  return z;
}

// Bubble.admissibility's last lines: the sizes of the two sets against the limits (0 = none, `or maxsize`).
SMX_BUBBLES_FN void bubble_admissible(int n_hijacked, int n_shadowed, int32_t hijack_limit, int32_t shadow_limit, bool& hijackable,
                                      bool& shadowable) {
  hijackable = hijack_limit == 0 || n_hijacked < hijack_limit;
  shadowable = shadow_limit == 0 || n_shadowed + n_hijacked < shadow_limit;
}

// Cursor.from_pos' transition (:313-327): the first that holds.  `state`: SMX_BUBBLE_* or SMX_BUBBLE_EGO; `was_in`: the
// agent's cursor at this bubble had a state in the previous pass.
SMX_BUBBLES_FN BubbleTransition bubble_transition(int state, bool was_in, BubbleZone z, bool hijackable, bool shadowable) {
  if (state == SMX_BUBBLE_SOCIAL && shadowable && z.in_airlock) return SMX_BT_AIRLOCK_ENTERED;
  if (state == SMX_BUBBLE_SHADOWED && hijackable && z.in_bubble) return SMX_BT_ENTERED;
  if (state == SMX_BUBBLE_HIJACKED && z.in_airlock) return SMX_BT_EXITED;
  if (was_in && (state == SMX_BUBBLE_SHADOWED || state == SMX_BUBBLE_HIJACKED) && !z.in_airlock && !z.in_bubble) return SMX_BT_AIRLOCK_EXITED;
  return SMX_BT_NONE;
}

// ... and its state (:329-333).
SMX_BUBBLES_FN BubbleCursor bubble_cursor(BubbleZone z, bool hijackable, bool shadowable) {
  if (hijackable && z.in_bubble) return SMX_BC_IN_BUBBLE;
  if (shadowable && z.in_airlock) return SMX_BC_IN_AIRLOCK;
  return SMX_BC_NONE;
}

// _handle_transitions on the state byte: what the airlock / hijack / relinquish / stop-shadowing calls leave the
// vehicle index with.  A transition that does not fit the state it meets changes nothing.
SMX_BUBBLES_FN int bubble_apply(int state, BubbleTransition t) {
  if (t == SMX_BT_AIRLOCK_ENTERED && state == SMX_BUBBLE_SOCIAL) return SMX_BUBBLE_SHADOWED;
  if (t == SMX_BT_ENTERED && state == SMX_BUBBLE_SHADOWED) return SMX_BUBBLE_HIJACKED;
  if (t == SMX_BT_AIRLOCK_EXITED && state == SMX_BUBBLE_HIJACKED) return SMX_BUBBLE_RELEASED;
  if (t == SMX_BT_AIRLOCK_EXITED && state == SMX_BUBBLE_SHADOWED) return SMX_BUBBLE_SOCIAL;
  return state;
}

// One bubble's view of an env at the start of the pass, a bit per agent slot.
struct BubbleMasks {
  uint64_t alive;                       // has a cursor (alive agents; all zero for an inactive bubble)
  uint64_t social, shadowed, hijacked;  // the state byte as the pass found it (an ego, or an agent not alive, is in none)
  uint64_t was_in;                      // the cursor mask's bit of this bubble as the pass found it
  uint64_t in_bubble, in_airlock;       // bubble_zone of the agent's position
};
// ... and what the pass makes of it.
struct BubbleResult {
  uint64_t cur_bubble, cur_airlock;  // cursor state InBubble / InAirlock (the new cursor bit = either)
  uint64_t airlock_entered, entered, airlock_exited;  // the transitions that change a state
};

SMX_BUBBLES_FN int bubble_popcount(uint64_t m) { return __builtin_popcountll((unsigned long long)m); }

// _sync_cursors for one bubble: agents in ascending slot.  For agent k the hijacked set is the agents the last pass left
// at this bubble and hijacked, united with the agents visited earlier in this pass whose cursor is InAirlock, less k;
// the shadowed set likewise with shadowed and InBubble — the pairing is the reference's (:188-196).
SMX_BUBBLES_FN BubbleResult bubble_recurrence(const BubbleMasks& m, int n_agents, int32_t hijack_limit, int32_t shadow_limit) {
  BubbleResult r = {0, 0, 0, 0, 0};
  const uint64_t held_hijacked = m.was_in & m.hijacked, held_shadowed = m.was_in & m.shadowed;
  for (int k = 0; k < n_agents && k < 64; ++k) {
    const uint64_t me = (uint64_t)1 << k;
    if (!(m.alive & me)) continue;
    bool hijackable, shadowable;
    bubble_admissible(bubble_popcount((held_hijacked | r.cur_airlock) & ~me), bubble_popcount((held_shadowed | r.cur_bubble) & ~me),
                      hijack_limit, shadow_limit, hijackable, shadowable);
    const int state = (m.social & me)     ? SMX_BUBBLE_SOCIAL
                      : (m.shadowed & me) ? SMX_BUBBLE_SHADOWED
                      : (m.hijacked & me) ? SMX_BUBBLE_HIJACKED
                                          : SMX_BUBBLE_EGO;  // (an ego or a released agent: no transition either way)
    BubbleZone z;
    z.in_bubble = (m.in_bubble & me) != 0;
    z.in_airlock = (m.in_airlock & me) != 0;
    const BubbleTransition t = bubble_transition(state, (m.was_in & me) != 0, z, hijackable, shadowable);
    const BubbleCursor c = bubble_cursor(z, hijackable, shadowable);
    if (c == SMX_BC_IN_BUBBLE) r.cur_bubble |= me;
    if (c == SMX_BC_IN_AIRLOCK) r.cur_airlock |= me;
    if (t == SMX_BT_AIRLOCK_ENTERED) r.airlock_entered |= me;
    if (t == SMX_BT_ENTERED) r.entered |= me;
    if (t == SMX_BT_AIRLOCK_EXITED) r.airlock_exited |= me;
  }
  return r;
}

// Agent k's transition at the bubble whose result is `r` (SMX_BT_EXITED changes nothing and is not kept).
SMX_BUBBLES_FN BubbleTransition bubble_transition_of(const BubbleResult& r, int k) {
  const uint64_t me = (uint64_t)1 << k;
  return (r.airlock_entered & me) ? SMX_BT_AIRLOCK_ENTERED : (r.entered & me) ? SMX_BT_ENTERED : (r.airlock_exited & me) ? SMX_BT_AIRLOCK_EXITED : SMX_BT_NONE;
}

#!/usr/bin/env python3
"""Generate tests/golden/bubble_cursors.npz by running the reference's OWN bubble code.

Runs only where the reference is (see gen_golden.py, whose import shim this uses).  ``shapely`` is absent there, so the few
shapely calls bubble_manager.py makes are served by the small stand-in below: a convex polygon with a strict ``within``,
``centroid``, a mitre ``buffer`` and ``affinity.translate`` / ``rotate``.  Everything that decides anything is the
reference's: ``PositionalZone.to_geometry``, ``Bubble`` (airlock geometry, ``in_bubble_or_airlock``, ``admissibility``,
``move_to_follow_vehicle``), ``Cursor.from_pos`` and ``BubbleManager._sync_cursors`` / ``_active_bubbles``, driven with a
duck-typed vehicle index.  The generator applies the cursors' transitions to that index as ``_handle_transitions`` would
(airlock: social -> shadowed; hijack: shadowed -> hijacked; relinquish: the vehicle leaves the index's social agents and
is marked released; stop shadowing: -> social).

Vehicles are inserted in slot order, so the index's iteration order is the slot order the device uses; an agent the
handover table drives (an "ego") is a vehicle that is not social, not shadowed and not hijacked.  Transitions are applied
in ascending (slot, bubble) order; no case gives one vehicle two state-changing transitions in a pass.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bubbles.py
"""
import math
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import gen_golden  # noqa: E402

SOCIAL, SHADOWED, HIJACKED, RELEASED = 0, 1, 2, 3


# ---- the stand-in for shapely ----------------------------------------------------------------------------------------
class Point:
    def __init__(self, *a):
        xy = a[0] if len(a) == 1 else a
        self.x, self.y = float(xy[0]), float(xy[1])

    def within(self, poly):
        return poly.contains_strictly(self.x, self.y)


class Polygon:
    """A convex polygon, vertices in either order."""

    def __init__(self, pts):
        self.pts = [(float(x), float(y)) for x, y in pts]

    def _signed_area(self):
        p = self.pts
        return 0.5 * sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p)))

    @property
    def centroid(self):
        p, a = self.pts, self._signed_area()
        cx = sum((p[i][0] + p[(i + 1) % len(p)][0]) * (p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1]) for i in range(len(p)))
        cy = sum((p[i][1] + p[(i + 1) % len(p)][1]) * (p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1]) for i in range(len(p)))
        return Point(cx / (6 * a), cy / (6 * a))

    def contains_strictly(self, x, y):
        p = self.pts
        sign = 1.0 if self._signed_area() > 0 else -1.0
        for i in range(len(p)):
            (x0, y0), (x1, y1) = p[i], p[(i + 1) % len(p)]
            if sign * ((x1 - x0) * (y - y0) - (y1 - y0) * (x - x0)) <= 0.0:
                return False  # on an edge or outside it: the boundary is outside
        return True

    def buffer(self, d, cap_style=None, join_style=None):
        """Mitre join: every edge moves outward by d, neighbours meet where their lines cross."""
        p = self.pts
        n = len(p)
        sign = 1.0 if self._signed_area() > 0 else -1.0
        lines = []
        for i in range(n):
            (x0, y0), (x1, y1) = p[i], p[(i + 1) % n]
            ex, ey = x1 - x0, y1 - y0
            ln = math.hypot(ex, ey)
            nx, ny = sign * ey / ln, -sign * ex / ln  # outward normal
            lines.append((x0 + nx * d, y0 + ny * d, ex, ey))
        out = []
        for i in range(n):
            ax, ay, adx, ady = lines[i - 1]
            bx, by, bdx, bdy = lines[i]
            den = adx * bdy - ady * bdx
            t = ((bx - ax) * bdy - (by - ay) * bdx) / den
            out.append((ax + adx * t, ay + ady * t))
        return Polygon(out)


def translate(geom, xoff=0.0, yoff=0.0):
    return Polygon([(x + xoff, y + yoff) for x, y in geom.pts])


def rotate(geom, angle, origin="center", use_radians=False):
    if not use_radians:
        angle = math.radians(angle)
    if origin == "centroid":
        c = geom.centroid
        ox, oy = c.x, c.y
    else:
        ox, oy = origin
    s, c = math.sin(angle), math.cos(angle)
    return Polygon([(ox + c * (x - ox) - s * (y - oy), oy + s * (x - ox) + c * (y - oy)) for x, y in geom.pts])


class _Style:
    square = 3
    mitre = 2


def install():
    gen_golden.install_reference()
    geo, aff = sys.modules["shapely.geometry"], sys.modules["shapely.affinity"]
    geo.Point, geo.Polygon, geo.CAP_STYLE, geo.JOIN_STYLE = Point, Polygon, _Style, _Style
    aff.rotate, aff.translate = rotate, translate
    import importlib

    return importlib.import_module("smarts.core.bubble_manager"), importlib.import_module("smarts.sstudio.types")


# ---- the duck-typed vehicle index ------------------------------------------------------------------------------------
class _Pose:
    def __init__(self, x, y):
        self.point = type("P", (), {"as_shapely": Point(x, y)})()


class Vehicle:
    def __init__(self, slot, x, y, heading):
        self.id = f"v{slot:02d}"
        self.slot = slot
        self.position = (x, y, 0.0)
        self.heading = heading
        self.pose = _Pose(x, y)


class Index:
    """What Cursor.from_pos, Bubble.admissibility, _sync_cursors and _active_bubbles ask of a VehicleIndex."""

    def __init__(self, vehicles, state, ego):
        self.vehicles = {v.id: v for v in vehicles}  # insertion order = slot order
        self.state, self.ego = state, ego

    def __and__(self, other):
        keep = [v for k, v in self.vehicles.items() if k in other.vehicles]
        return Index(keep, self.state, self.ego)

    def vehicleitems(self):
        return list(self.vehicles.items())

    def social_vehicle_ids(self):
        return {k for k, v in self.vehicles.items() if not self.ego[v.slot] and self.state[v.slot] in (SOCIAL, SHADOWED)}

    def vehicle_is_hijacked(self, vid):  # (a vehicle that is gone is neither, vehicle_index.py:189-201)
        v = self.vehicles.get(vid)
        return v is not None and not self.ego[v.slot] and self.state[v.slot] == HIJACKED

    def vehicle_is_shadowed(self, vid):
        v = self.vehicles.get(vid)
        return v is not None and not self.ego[v.slot] and self.state[v.slot] == SHADOWED

    def vehicle_is_hijacked_or_shadowed(self, vid):
        return self.vehicle_is_hijacked(vid), self.vehicle_is_shadowed(vid)

    def vehicles_by_actor_id(self, actor_id):
        return [v for v in self.vehicles.values() if v.id == actor_id]

    _any = {}  # vehicle id -> slot


def run_case(bm_mod, types, bubbles, ticks):
    """bubbles: [dict(pos, size, margin, follow, offset, hijack, shadow)]; ticks: [dict(pos [A, 2], heading [A], alive [A],
    ego [A])].  Returns per tick (state, mask, transitions, cursors) after the pass."""
    A = len(ticks[0]["alive"])
    ss = []
    for b in bubbles:
        limit = None
        if b["hijack"] or b["shadow"]:
            # (the wrapper takes a BubbleLimits as it is; 0 = none is the wrapper's `or maxsize`.  BubbleLimits itself
            # refuses shadow < hijack, so a lone shadow limit goes in through a plain record of the same two fields.)
            limit = type("Limits", (types.BubbleLimits,), {"__post_init__": lambda self: None})(b["hijack"], b["shadow"])
        ss.append(types.Bubble(zone=types.PositionalZone(pos=tuple(b["pos"]), size=tuple(b["size"])), actor=types.SocialAgentActor(name="a", agent_locator="l"),
                               margin=b["margin"], limit=limit, follow_actor_id=(f"v{b['follow']:02d}" if b["follow"] >= 0 else None),
                               follow_offset=(tuple(b["offset"]) if b["follow"] >= 0 else None)))
    mgr = bm_mod.BubbleManager(ss, None)
    # The one listed deviation: vehicle_ids_per_bubble merges two dicts keyed by bubble (:389-391),
    # so a bubble that has cursors of both states keeps its InAirlock set alone.  The fixture pins the rule with the union
    # of the two sets, which is what the method's name and its callers mean; nothing else of the reference is replaced.
    from collections import defaultdict

    def vehicle_ids_per_bubble(cursors):
        vid = bm_mod.BubbleManager._vehicle_ids_divided_by_bubble_state(cursors)
        both = defaultdict(set)
        for st in (bm_mod.BubbleState.InBubble, bm_mod.BubbleState.InAirlock):
            for bubble, ids in vid[st].items():
                both[bubble] |= ids
        return both

    bm_mod.BubbleManager.vehicle_ids_per_bubble = staticmethod(vehicle_ids_per_bubble)
    order = {id(b): j for j, b in enumerate(mgr._bubbles)}
    state = [SOCIAL] * A
    Index._any = {f"v{a:02d}": a for a in range(A)}
    out = []
    for tk in ticks:
        ego = [bool(e) for e in tk["ego"]]
        vehicles = [Vehicle(a, tk["pos"][a][0], tk["pos"][a][1], tk["heading"][a]) for a in range(A) if tk["alive"][a]]
        index = Index(vehicles, state, ego)
        mgr._last_vehicle_index = index  # (the vehicles of the pass: none is new, none has gone)
        for b in mgr._active_bubbles():
            if b.is_travelling:
                b.move_to_follow_vehicle(index.vehicles_by_actor_id(b.follow_actor_id)[0])
        mgr._cursors = mgr._sync_cursors(index, index)
        nb = len(mgr._bubbles)
        trans = np.zeros((A, nb), dtype=np.int8)
        curs = np.zeros((A, nb), dtype=np.int8)
        for c in mgr._cursors:
            a, j = Index._any[c.vehicle_id], order[id(c.bubble)]
            trans[a, j] = 0 if c.transition is None else c.transition.value + 1
            curs[a, j] = 0 if c.state is None else (1 if c.state == bm_mod.BubbleState.InBubble else 2)
        for a in range(A):  # _handle_transitions on the index
            for j in range(nb):
                t = trans[a, j]
                if t == 1 and state[a] == SOCIAL:
                    state[a] = SHADOWED
                elif t == 2 and state[a] == SHADOWED:
                    state[a] = HIJACKED
                elif t == 4:
                    state[a] = RELEASED if state[a] == HIJACKED else SOCIAL
        mask = [sum(1 << j for j in range(nb) if curs[a, j]) for a in range(A)]
        out.append((list(state), mask, trans, curs))
    return out


def cases(rng):
    """name -> (bubbles, ticks).  Columns of vehicles driving through bubbles at 0.8 m a tick, along x or on a slant."""
    def column(n, gap, ticks, heading=-math.pi / 2, y=0.0, slant=0.0, x0=0.0, order=None, leave=None, ego=None):
        order = list(range(n)) if order is None else order
        out = []
        for t in range(ticks):
            pos = [[x0 - gap * order[a] + 0.8 * t + 0.013, y + slant * (-gap * order[a] + 0.8 * t) + 0.007] for a in range(n)]
            alive = [not (leave and a in leave and t >= leave[a]) for a in range(n)]
            out.append(dict(pos=pos, heading=[heading] * n, alive=alive, ego=[bool(ego and a in ego and t >= ego[a]) for a in range(n)]))
        return out

    fixed = lambda x, length, **kw: dict(dict(pos=(x, 0.0), size=(length, 12.0), margin=2.0, follow=-1, offset=(0, 0), hijack=0, shadow=0), **kw)  # noqa: E731
    c = {}
    c["through"] = ([fixed(20.3, 8.0)], column(4, 6.0, 60))
    c["inside_at_start"] = ([fixed(0.3, 8.0)], column(1, 6.0, 20))
    c["jumped_ring"] = ([fixed(6.75, 4.3, margin=0.5)], column(1, 6.0, 20))
    c["ring_then_second"] = ([dict(fixed(17.0, 3.0, margin=5.0), pos=(17.0, 6.0), size=(3.0, 3.0)), fixed(34.4, 5.0)], column(1, 6.0, 56))
    c["hijack_limit_1"] = ([fixed(20.3, 8.0, hijack=1)], column(2, 6.0, 56))
    c["hijack_limit_1_reverse_slots"] = ([fixed(20.3, 8.0, hijack=1)], column(2, 6.0, 56, order=[1, 0]))
    c["shadow_limit_2"] = ([fixed(22.3, 16.0, shadow=2)], column(3, 6.0, 60, order=[2, 1, 0], x0=6.4))
    c["shadow_limit_2_slot_order"] = ([fixed(22.3, 16.0, shadow=2)], column(3, 6.0, 60, x0=6.4))
    c["column_5_9"] = ([fixed(13.3, 22.0, hijack=5, shadow=9)], column(16, 4.0, 70))
    c["column_5_9_mixed"] = ([fixed(13.3, 22.0, hijack=5, shadow=9)], column(16, 4.0, 70, order=list(range(0, 16, 2)) + list(range(1, 16, 2))))
    c["two_overlapping"] = ([fixed(20.3, 8.0, hijack=2, shadow=3), fixed(26.1, 6.0, hijack=1, shadow=2)], column(5, 5.0, 70, slant=0.1))
    c["leaves_while_hijacked"] = ([fixed(20.3, 8.0, hijack=1)], column(3, 6.0, 60, leave={0: 26}))
    c["ego_rides_through"] = ([fixed(20.3, 8.0, hijack=1, shadow=2)], column(3, 6.0, 60, ego={0: 0, 2: 30}))
    # a travelling bubble: vehicle 0 overtakes the column at 1.2 m a tick, turning slowly; it ends at tick 40
    ticks = column(4, 6.0, 60)
    for t, tk in enumerate(ticks):
        h = -math.pi / 2 + 0.003 * t
        tk["pos"][0] = [-30.0 + 1.2 * t + 0.011, 0.4 * math.sin(0.05 * t)]
        tk["heading"][0] = h
        tk["ego"][0] = True
        tk["alive"][0] = t < 40
    c["travelling"] = ([dict(pos=(0.0, 0.0), size=(6.0, 4.2), margin=2.0, follow=0, offset=(0.0, 8.0), hijack=0, shadow=0)], ticks)
    c["travelling_limits"] = ([dict(pos=(0.0, 0.0), size=(6.0, 9.2), margin=2.0, follow=0, offset=(0.0, 8.0), hijack=1, shadow=2),
                               fixed(20.3, 8.0, hijack=1)], ticks)
    # random walks around three bubbles with limits: every branch of the rule, many times over
    walk = []
    pos = rng.uniform(-14.0, 14.0, size=(8, 2))
    for t in range(160):
        pos = pos + rng.uniform(-1.6, 1.6, size=(8, 2))
        pos = np.clip(pos, -16.0, 16.0)
        walk.append(dict(pos=(np.round(pos, 3) + 0.0004).tolist(), heading=[0.0] * 8, alive=[not (a == 3 and 50 <= t < 70) for a in range(8)],
                         ego=[a == 5 and t >= 100 for a in range(8)]))
    c["random_walk"] = ([dict(pos=(-4.0, 0.0), size=(9.0, 9.0), margin=2.0, follow=-1, offset=(0, 0), hijack=2, shadow=3),
                         dict(pos=(5.0, 2.0), size=(7.0, 11.0), margin=1.5, follow=-1, offset=(0, 0), hijack=1, shadow=0),
                         dict(pos=(0.0, -6.0), size=(14.0, 5.0), margin=3.0, follow=-1, offset=(0, 0), hijack=0, shadow=2)], walk)
    return c


def main():
    bm_mod, types = install()
    rng = np.random.default_rng(20261019)
    out = {}
    names = []
    for name, (bubbles, ticks) in cases(rng).items():
        res = run_case(bm_mod, types, bubbles, ticks)
        names.append(name)
        out[f"{name}/bubbles"] = np.array([[*b["pos"], *b["size"], b["margin"], *b["offset"], b["follow"], b["hijack"], b["shadow"]] for b in bubbles], dtype=np.float64)
        out[f"{name}/pos"] = np.array([tk["pos"] for tk in ticks], dtype=np.float64)
        out[f"{name}/heading"] = np.array([tk["heading"] for tk in ticks], dtype=np.float64)
        out[f"{name}/alive"] = np.array([tk["alive"] for tk in ticks], dtype=np.uint8)
        out[f"{name}/ego"] = np.array([tk["ego"] for tk in ticks], dtype=np.uint8)
        out[f"{name}/state"] = np.array([r[0] for r in res], dtype=np.uint8)
        out[f"{name}/mask"] = np.array([r[1] for r in res], dtype=np.uint8)
        out[f"{name}/transitions"] = np.stack([r[2] for r in res])
        out[f"{name}/cursors"] = np.stack([r[3] for r in res])
        seen = sorted(set(np.stack([r[2] for r in res]).ravel().tolist()))
        print(f"{name}: {len(ticks)} ticks, states {sorted(set(np.array([r[0] for r in res]).ravel().tolist()))}, transitions {seen}")
    out["names"] = np.array(names)
    path = os.path.join(gen_golden.OUT, "bubble_cursors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

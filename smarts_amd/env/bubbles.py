"""The reference's bubble descriptors (``smarts/sstudio/types.py``: ``Bubble``, ``PositionalZone``, ``BubbleLimits``) for
``HistoryObserver(bubbles=...)``: the same field names and the same ``__post_init__`` refusals, turned into the
``smx_bubble`` records of ``BatchedSim.set_history_bubbles`` (``include/smx.h``; DESIGN.md section 5.21 has the rule).

What the device evaluates is a ``PositionalZone`` bubble over a replayed history.  A ``MapZone``, a boid actor and
``keep_alive`` raise ``NotImplementedError``."""
from __future__ import annotations

from dataclasses import dataclass, field
from sys import maxsize
from typing import Any, Callable, Optional, Tuple

from .. import _native as nat


@dataclass(frozen=True)
class Zone:
    """The base of the zone descriptors."""


@dataclass(frozen=True)
class PositionalZone(Zone):
    """A capture area at a specific XY location: ``pos`` its centre, ``size`` its (x, y) extent."""

    pos: Tuple[float, float]
    size: Tuple[float, float]


@dataclass(frozen=True)
class MapZone(Zone):
    """A capture area along lanes of the map (accepted as a descriptor; not evaluated on the device)."""

    start: Tuple[str, int, float]
    length: float
    n_lanes: int = 2


@dataclass(frozen=True)
class BubbleLimits:
    """The capture limits of a bubble."""

    hijack_limit: int = maxsize
    shadow_limit: int = maxsize

    def __post_init__(self):
        if self.shadow_limit is None:
            raise ValueError("Shadow limit must be a non-negative real number")
        if self.hijack_limit is None or self.shadow_limit < self.hijack_limit:
            raise ValueError("Shadow limit must be >= hijack limit")


@dataclass(frozen=True)
class Bubble:
    """A capture bubble.  ``actor``: who takes the captured vehicles over (any value: the caller's policy acts through
    ``HistoryObserver.step``; an object whose class is named ``BoidAgentActor`` is refused).  ``follow_actor_id``: the
    agent id (``HistoryObserver.agent_id``) the bubble travels with, ``follow_offset`` its centre in that vehicle's
    frame, as if the vehicle faced north."""

    zone: Zone
    actor: Any = None
    margin: float = 2
    limit: Optional[BubbleLimits] = None
    exclusion_prefixes: Tuple[str, ...] = field(default_factory=tuple)
    id: str = "bubble"
    follow_actor_id: Optional[str] = None
    follow_offset: Optional[Tuple[float, float]] = None
    keep_alive: bool = False

    def __post_init__(self):
        if self.margin <= 0:
            raise ValueError("Airlocking margin must be greater than 0")
        if self.follow_actor_id is not None and self.follow_offset is None:
            raise ValueError("A follow offset must be set if this is a travelling bubble")
        if self.keep_alive and not self.is_boid:
            raise ValueError("Only boids can have keep_alive enabled (for persistent boids)")

    @property
    def is_boid(self) -> bool:
        return type(self.actor).__name__ == "BoidAgentActor"

    def to_native(self, slot_of: Callable[[str], int]) -> "nat.SmxBubble":
        """The ``smx_bubble`` of this descriptor; ``slot_of`` maps ``follow_actor_id`` to an agent slot."""
        if not isinstance(self.zone, PositionalZone):
            raise NotImplementedError(f"{type(self.zone).__name__} bubbles are not evaluated on the device: only PositionalZone is (a rectangle test)")
        if self.is_boid or self.keep_alive:
            raise NotImplementedError("boid actors and keep_alive need agents that are created at run time; a bubble here captures agent slots")
        if self.exclusion_prefixes:
            raise NotImplementedError("exclusion_prefixes: a recorded vehicle is excluded by not giving it an agent slot")
        # (Bubble.__init__, bubble_manager.py:70-74: no limit = BubbleLimits(); a limit's maxsize is "none", 0 on the device)
        limit = self.limit or BubbleLimits()
        none = lambda v: 0 if v >= maxsize else int(v)  # noqa: E731
        follow = -1 if self.follow_actor_id is None else int(slot_of(self.follow_actor_id))
        ox, oy = self.follow_offset if self.follow_offset is not None else (0.0, 0.0)
        return nat.SmxBubble(float(self.zone.pos[0]), float(self.zone.pos[1]), float(self.zone.size[0]), float(self.zone.size[1]),
                             float(self.margin), float(ox), float(oy), follow, none(limit.hijack_limit), none(limit.shadow_limit))

"""Frame stacking over host copies of the dense rows: what ``k_frame_push`` / ``k_frame_dstack`` do on the device
(``SimConfig(frame_stack=k)``, include/smx.h ``smx_bind_frame_stack``), restated in NumPy the way ``lane_ttc_rows`` and
``ego_centric_rows`` restate their blocks.

The semantics are the reference's ``FrameStack`` (smarts/env/wrappers/frame_stack.py) over ``(env, slot)`` rows: per
agent a ``deque(maxlen=k)`` kept newest first.  An agent with an observation gets its row pushed (``appendleft``,
:69-72); the first observation of an episode fills all k frames (:104-109) — on ``reset`` for the selected envs, and for
an env that restarted inside a step under ``auto_reset`` (``ParallelEnv``'s worker calls the wrapped ``reset()``,
parallel_env.py:303-309: the finishing tick's frame is not pushed); an agent without an observation keeps its stack.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np


def dstack_frames(stack: np.ndarray) -> np.ndarray:
    """``[..., k, H, W, 3]`` frames -> ``[..., H, W, 3k]`` with channel ``3j + c`` = frame j's channel c: ``np.dstack``
    of the frames, the array ``RGBImage.observation`` returns (rgb_image.py:93-99)."""
    k = stack.shape[-4]
    return np.concatenate([stack[..., j, :, :, :] for j in range(k)], axis=-1)


class FrameStackRows:
    """Stacks of the last ``k`` frames of every row given, ``stacks[name]`` of shape ``[E, N, k, ...row shape]``."""

    def __init__(self, k: int):
        assert k > 1, f"Expected num_stack > 1, but got {k}."
        self.k = int(k)
        self.stacks: Dict[str, np.ndarray] = {}

    def _apply(self, rows: Dict[str, np.ndarray], push: np.ndarray, fill: np.ndarray) -> Dict[str, np.ndarray]:
        for name, row in rows.items():
            row = np.asarray(row)
            if name not in self.stacks:
                self.stacks[name] = np.zeros(row.shape[:2] + (self.k,) + row.shape[2:], dtype=row.dtype)
            s = self.stacks[name]
            s[push, 1:] = s[push, :-1].copy()
            s[push, 0] = row[push]
            s[fill] = row[fill][:, None]
        return self.stacks

    def reset(self, rows: Dict[str, np.ndarray], env_mask: Optional[np.ndarray], observing: np.ndarray) -> Dict[str, np.ndarray]:
        """``observing`` [E, N]: the agents with an observation after the reset; ``env_mask`` [E]: the envs that were
        reset (``None``: all).  Their stacks are filled, everybody else's are untouched."""
        observing = np.asarray(observing, dtype=bool)
        sel = np.ones(observing.shape[0], dtype=bool) if env_mask is None else np.asarray(env_mask, dtype=bool)
        fill = observing & sel[:, None]
        return self._apply(rows, np.zeros_like(fill), fill)

    def step(self, rows: Dict[str, np.ndarray], observing: np.ndarray, restarted: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
        """``observing`` [E, N]: the agents with an observation in this step (for a restarted env: in its first
        observation); ``restarted`` [E]: the envs that restarted inside the step (``auto_reset``), whose agents'
        stacks are filled instead of pushed."""
        observing = np.asarray(observing, dtype=bool)
        again = np.zeros(observing.shape[0], dtype=bool) if restarted is None else np.asarray(restarted, dtype=bool)
        return self._apply(rows, observing & ~again[:, None], observing & again[:, None])

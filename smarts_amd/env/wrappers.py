"""The observation wrappers of the reference's ``smarts/env/wrappers`` that this package lacked: ``FrameStack``
(frame_stack.py), ``RGBImage`` (rgb_image.py) and ``SingleAgent`` (single_agent.py), over ``Observation`` objects and
any env with ``agent_specs``, ``reset()`` and ``step(actions)``.  Same assertions and messages, same return types; no
``gym`` dependency, like ``FormatObs``.  The device-side counterpart over dense rows is ``SimConfig(frame_stack=k)``
(``frame_stack_rows`` on the host)."""
from __future__ import annotations

import copy
from collections import deque
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np


class _Wrapper:
    """What the three wrappers need of ``gym.Wrapper``: the wrapped env and attribute pass-through."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.env, name)

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        return self.env.step(actions)

    def close(self):
        return self.env.close()


class FrameStack(_Wrapper):
    """Stacks ``num_stack`` consecutive observations per agent in a moving window, newest first; returns deep copies."""

    def __init__(self, env, num_stack: int = 3):
        assert num_stack > 1, f"Expected num_stack > 1, but got {num_stack}."
        super().__init__(env)
        self._num_stack = num_stack
        self._frames = {agent_id: deque(maxlen=num_stack) for agent_id in env.agent_specs.keys()}

    def _stacked(self, frame: Dict[str, Any]) -> Dict[str, List[Any]]:
        out = {}
        for agent_id, observation in frame.items():
            self._frames[agent_id].appendleft(observation)
            out[agent_id] = copy.deepcopy(list(self._frames[agent_id]))
        return out

    def step(self, agent_actions: Dict) -> Tuple[Dict[str, List[Any]], Dict[str, float], Dict[str, bool], Dict[str, Any]]:
        observations, rewards, dones, infos = self.env.step(agent_actions)
        return self._stacked(observations), rewards, dones, infos

    def reset(self) -> Dict[str, List[Any]]:
        observations = self.env.reset()
        for agent_id, observation in observations.items():  # the first observation fills the window
            self._frames[agent_id].extendleft([observation] * (self._num_stack - 1))
        return self._stacked(observations)


class RGBImage(_Wrapper):
    """Keeps only the top-down RGB image of every observation; over ``FrameStack`` the frames are stacked along the
    channel axis: ``(H, W, 3 * num_stack)`` uint8, newest first."""

    def __init__(self, env, num_stack: int):
        super().__init__(env)
        for agent_id, spec in env.agent_specs.items():
            assert spec.interface.rgb, (
                f"To use RGBImage wrapper, enable RGB "
                f"functionality in {agent_id}'s AgentInterface."
            )
        self._num_stack = num_stack
        assert self._num_stack > 0

    def observation(self, obs: Dict[str, Any]) -> Dict[str, np.ndarray]:
        wrapped = {}
        for agent_id, agent_obs in obs.items():
            if isinstance(agent_obs, Sequence):
                true_num_stack = len(agent_obs)
            else:
                true_num_stack, agent_obs = 1, [agent_obs]
            assert self._num_stack == true_num_stack, (
                f"User supplied `num_stack` (={self._num_stack}) argument to "
                f"`RGBImage` wrapper does not match the number of frames "
                f"stacked (={true_num_stack}) in the underlying base env."
            )
            wrapped[agent_id] = np.dstack([o.top_down_rgb.data.astype(np.uint8) for o in agent_obs])
        return wrapped

    def reset(self):
        return self.observation(self.env.reset())

    def step(self, actions):
        observations, rewards, dones, infos = self.env.step(actions)
        return self.observation(observations), rewards, dones, infos


class SingleAgent(_Wrapper):
    """Unwraps the per-agent dictionaries of an env with exactly one agent."""

    def __init__(self, env):
        super().__init__(env)
        agent_ids = list(env.agent_specs.keys())
        assert (
            len(agent_ids) == 1
        ), f"Expected env to have a single agent, but got {len(agent_ids)} agents."
        self._agent_id = agent_ids[0]

    def step(self, action: Any) -> Tuple[Any, float, bool, Any]:
        obs, reward, done, info = self.env.step({self._agent_id: action})
        return obs[self._agent_id], reward[self._agent_id], done[self._agent_id], info[self._agent_id]

    def reset(self) -> Any:
        return self.env.reset()[self._agent_id]

"""Generates tests/golden/frame_stack_cases.npz: the reference's own FrameStack, RGBImage and SingleAgent
(smarts/env/wrappers/frame_stack.py, rgb_image.py, single_agent.py) run over a scripted two-agent stub env.

Run where the reference checkout is present (SMARTS_REFERENCE, as gen_golden.py):
    python tests/golden/gen_golden_frame_stack.py
The three modules are loaded by path; `gym` and `smarts.core.sensors` are name-only stubs (the wrappers use gym for the
Wrapper base classes and for space objects nobody reads here, and sensors for annotations).  The file holds only the
script, the frame numbers per stack position per tick and the dstacked arrays.
"""
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get("SMARTS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
AGENTS = ("agent_a", "agent_b")
H, W = 4, 3
# (kind, agents present in what the env returns); frame n is the n-th call
SCRIPT = [("reset", (0, 1)), ("step", (0, 1)), ("step", (0,)), ("step", (0, 1)), ("step", (0,)), ("step", (0, 1)),
          ("reset", (0, 1)), ("step", (0, 1)), ("step", (1,)), ("step", (1,)), ("step", (0, 1))]


def image(n: int, agent: int) -> np.ndarray:
    """The 4 x 3 x 3 image agent `agent` sees in frame `n`: every byte differs, and frames and agents differ."""
    return ((np.arange(H * W * 3).reshape(H, W, 3) + 37 * n + 101 * agent) % 256).astype(np.uint8)


def _stub_modules():
    gym = types.ModuleType("gym")

    class Env:
        pass

    class Wrapper(Env):
        observation_space = None

        def __init__(self, env):
            self.env = env

        def __getattr__(self, name):
            if name.startswith("_"):
                raise AttributeError(name)
            return getattr(self.env, name)

        def step(self, action):
            return self.env.step(action)

        def reset(self):
            return self.env.reset()

    class ObservationWrapper(Wrapper):
        def reset(self):
            return self.observation(self.env.reset())

        def step(self, action):
            obs, reward, done, info = self.env.step(action)
            return self.observation(obs), reward, done, info

    class _Space:
        def __init__(self, *args, **kwargs):
            pass

    gym.Env, gym.Wrapper, gym.ObservationWrapper = Env, Wrapper, ObservationWrapper
    gym.spaces = types.ModuleType("gym.spaces")
    gym.spaces.Dict = gym.spaces.Tuple = gym.spaces.Box = _Space
    sys.modules["gym"], sys.modules["gym.spaces"] = gym, gym.spaces
    for name in ("smarts", "smarts.core", "smarts.core.sensors"):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
        sys.modules[name] = m
    sys.modules["smarts"].core = sys.modules["smarts.core"]
    sys.modules["smarts.core"].sensors = sys.modules["smarts.core.sensors"]
    sys.modules["smarts.core.sensors"].Observation = object


def _load(name):
    path = os.path.join(REF, "smarts", "env", "wrappers", name + ".py")
    spec = importlib.util.spec_from_file_location("ref_wrappers_" + name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


class Obs:
    """An observation as far as the wrappers look: frame number and top_down_rgb.data."""

    def __init__(self, n, agent):
        self.n = n
        self.top_down_rgb = types.SimpleNamespace(data=image(n, agent))


class StubEnv:
    def __init__(self, agents):
        self.agents = tuple(agents)
        rgb = types.SimpleNamespace(width=W, height=H)
        self.agent_specs = {AGENTS[i]: types.SimpleNamespace(interface=types.SimpleNamespace(rgb=rgb)) for i in self.agents}
        self.observation_space = None
        self.call = -1

    def _frame(self, kind):
        self.call += 1
        want, present = SCRIPT[self.call]
        assert want == kind, (self.call, kind)
        return {AGENTS[i]: Obs(self.call, i) for i in present if i in self.agents}

    def reset(self):
        return self._frame("reset")

    def step(self, actions):
        obs = self._frame("step")
        return obs, {a: 0.0 for a in obs}, {a: False for a in obs}, {a: {"n": o.n} for a, o in obs.items()}


def main():
    _stub_modules()
    frame_stack, rgb_image, single_agent = _load("frame_stack"), _load("rgb_image"), _load("single_agent")
    T = len(SCRIPT)
    present = np.zeros((T, 2), dtype=bool)
    for t, (_, who) in enumerate(SCRIPT):
        present[t, list(who)] = True
    out = {"is_reset": np.array([kind == "reset" for kind, _ in SCRIPT]), "present": present}
    for k in (2, 3):
        frames = np.full((T, 2, k), -1, dtype=np.int64)
        stacked_env = frame_stack.FrameStack(StubEnv((0, 1)), num_stack=k)
        dstack = np.zeros((T, 2, H, W, 3 * k), dtype=np.uint8)
        image_env = rgb_image.RGBImage(frame_stack.FrameStack(StubEnv((0, 1)), num_stack=k), num_stack=k)
        # SingleAgent over FrameStack, agent_b alone (absent on some ticks of the script: a single-agent env always
        # answers, so its script is the ticks agent_b is present in, in order)
        single = np.full((T, k), -1, dtype=np.int64)
        solo = StubEnv((1,))
        single_env = single_agent.SingleAgent(frame_stack.FrameStack(solo, num_stack=k))
        for t, (kind, who) in enumerate(SCRIPT):
            obs = stacked_env.reset() if kind == "reset" else stacked_env.step({})[0]
            images = image_env.reset() if kind == "reset" else image_env.step({})[0]
            assert set(obs) == set(images) == {AGENTS[i] for i in who}
            for i in who:
                frames[t, i] = [o.n for o in obs[AGENTS[i]]]
                dstack[t, i] = images[AGENTS[i]]
            if 1 in who:
                got = single_env.reset() if kind == "reset" else single_env.step(0)[0]
                single[t] = [o.n for o in got]
            else:
                solo.call += 1  # the tick passes without agent_b
        out[f"frames_k{k}"], out[f"dstack_k{k}"], out[f"single_k{k}"] = frames, dstack, single
    path = os.path.join(HERE, "frame_stack_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in (2, 3):
        print(k, out[f"frames_k{k}"][:, :, :].tolist())


if __name__ == "__main__":
    main()

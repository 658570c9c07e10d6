"""Frame stacking without a GPU: the three wrappers (smarts_amd/env/wrappers.py) and the host restatement of the device
pass (smarts_amd/env/frame_stack_rows.py) against tests/golden/frame_stack_cases.npz — the reference's own FrameStack,
RGBImage and SingleAgent over a scripted two-agent stub env (tests/golden/gen_golden_frame_stack.py) — the reference's
assertion messages, FormatObs.from_rows(frame=j), and the ABI additions with smx_check_frame_stack, which needs neither a
device nor a handle.  The device side is tests/test_gpu_frame_stack.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from smarts_amd import _native as nat
from smarts_amd.engine import SimConfig
from smarts_amd.env import FrameStack, RGBImage, SingleAgent
from smarts_amd.env.frame_stack_rows import FrameStackRows, dstack_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGENTS = ("agent_a", "agent_b")
H, W = 4, 3


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "frame_stack_cases.npz")))


def image(n, agent):  # (the generator's numbering)
    return ((np.arange(H * W * 3).reshape(H, W, 3) + 37 * n + 101 * agent) % 256).astype(np.uint8)


class Obs:
    def __init__(self, n, agent):
        self.n = n
        self.top_down_rgb = types.SimpleNamespace(data=image(n, agent))


class ScriptedEnv:
    """Replays the golden's script: call n returns frame n for the agents present in it."""

    def __init__(self, golden, agents, rgb=True):
        self.golden, self.agents, self.call = golden, tuple(agents), -1
        iface = types.SimpleNamespace(rgb=types.SimpleNamespace(width=W, height=H) if rgb else None)
        self.agent_specs = {AGENTS[i]: types.SimpleNamespace(interface=iface) for i in self.agents}

    def _frame(self, reset):
        self.call += 1
        assert bool(self.golden["is_reset"][self.call]) == reset
        return {AGENTS[i]: Obs(self.call, i) for i in self.agents if self.golden["present"][self.call, i]}

    def reset(self):
        return self._frame(True)

    def step(self, actions):
        obs = self._frame(False)
        return obs, {a: 1.5 for a in obs}, {a: False for a in obs}, {a: {"n": o.n} for a, o in obs.items()}


@pytest.mark.parametrize("k", (2, 3))
def test_wrappers_reproduce_the_reference(golden, k):
    T = len(golden["is_reset"])
    assert golden["is_reset"][0] and golden["is_reset"][1:].any() and not golden["present"].all()  # a reset midway, absences
    stacked = FrameStack(ScriptedEnv(golden, (0, 1)), num_stack=k)
    images = RGBImage(FrameStack(ScriptedEnv(golden, (0, 1)), num_stack=k), num_stack=k)
    solo = ScriptedEnv(golden, (1,))
    single = SingleAgent(FrameStack(solo, num_stack=k))
    for t in range(T):
        reset = bool(golden["is_reset"][t])
        obs = stacked.reset() if reset else stacked.step({})[0]
        img = images.reset() if reset else images.step({})[0]
        who = [i for i in (0, 1) if golden["present"][t, i]]
        assert set(obs) == set(img) == {AGENTS[i] for i in who}
        for i in who:
            frames = obs[AGENTS[i]]
            assert isinstance(frames, list) and [o.n for o in frames] == golden[f"frames_k{k}"][t, i].tolist()
            got = img[AGENTS[i]]
            assert got.dtype == np.uint8 and got.shape == (H, W, 3 * k) and np.array_equal(got, golden[f"dstack_k{k}"][t, i])
        if 1 in who:
            if reset:
                got = single.reset()
            else:
                got, reward, done, info = single.step(0)
                assert reward == 1.5 and done is False and info == {"n": t}
            assert [o.n for o in got] == golden[f"single_k{k}"][t].tolist()
        else:
            solo.call += 1
    # deep copies: what a caller does to a returned frame does not reach the window
    env = FrameStack(ScriptedEnv(golden, (0, 1)), num_stack=k)
    first = env.reset()
    first[AGENTS[0]][0].n = 99
    assert [o.n for o in env.step({})[0][AGENTS[0]]] == golden[f"frames_k{k}"][1, 0].tolist()


@pytest.mark.parametrize("k", (2, 3))
def test_frame_stack_rows_reproduce_the_reference(golden, k):
    """One env of two slots; rows: the frame number (int64, one column), the image, and a 9-byte row."""
    fs = FrameStackRows(k)
    T = len(golden["is_reset"])
    for t in range(T):
        present = golden["present"][t][None, :]  # [E = 1, N = 2]
        rows = {"n": np.full((1, 2, 1), t, dtype=np.int64), "rgb": np.stack([image(t, 0), image(t, 1)])[None],
                "events": (np.arange(18, dtype=np.uint8).reshape(1, 2, 9) + t)}
        stacks = fs.reset(rows, None, present) if golden["is_reset"][t] else fs.step(rows, present)
        assert stacks["rgb"].shape == (1, 2, k, H, W, 3) and stacks["rgb"].dtype == np.uint8
        for i in (0, 1):
            if not present[0, i]:
                continue
            want = golden[f"frames_k{k}"][t, i]
            assert stacks["n"][0, i, :, 0].tolist() == want.tolist()
            assert np.array_equal(dstack_frames(stacks["rgb"])[0, i], golden[f"dstack_k{k}"][t, i])
            assert np.array_equal(stacks["events"][0, i], np.stack([np.arange(9 * i, 9 * i + 9, dtype=np.uint8) + n for n in want]))


def test_frame_stack_rows_masked_reset_and_restart():
    fs = FrameStackRows(3)
    rows = lambda v: {"x": np.full((2, 2), v, dtype=np.float32)}  # noqa: E731
    every = np.ones((2, 2), dtype=bool)
    fs.reset(rows(1), None, every)
    fs.step(rows(2), every)
    s = fs.reset(rows(7), np.array([False, True]), every)  # env 1 alone
    assert s["x"][0].tolist() == [[2, 1, 1]] * 2 and s["x"][1].tolist() == [[7, 7, 7]] * 2
    s = fs.step(rows(8), np.array([[True, False], [True, True]]), restarted=np.array([True, False]))
    assert s["x"][0].tolist() == [[8, 8, 8], [2, 1, 1]]  # restarted: filled; its absent agent: held
    assert s["x"][1].tolist() == [[8, 7, 7]] * 2  # the other env pushed


def test_the_references_assertion_messages(golden):
    env = ScriptedEnv(golden, (0, 1))
    with pytest.raises(AssertionError, match=r"^Expected num_stack > 1, but got 1\.$"):
        FrameStack(env, num_stack=1)
    with pytest.raises(AssertionError, match=r"^Expected num_stack > 1, but got 1\.$"):
        FrameStackRows(1)
    with pytest.raises(AssertionError, match=r"^To use RGBImage wrapper, enable RGB functionality in agent_a's AgentInterface\.$"):
        RGBImage(ScriptedEnv(golden, (0, 1), rgb=False), num_stack=1)
    with pytest.raises(AssertionError):
        RGBImage(env, num_stack=0)
    wrong = RGBImage(FrameStack(ScriptedEnv(golden, (0, 1)), num_stack=2), num_stack=3)
    with pytest.raises(AssertionError, match=r"^User supplied `num_stack` \(=3\) argument to `RGBImage` wrapper does not match "
                                             r"the number of frames stacked \(=2\) in the underlying base env\.$"):
        wrong.reset()
    with pytest.raises(AssertionError, match=r"^Expected env to have a single agent, but got 2 agents\.$"):
        SingleAgent(env)
    unstacked = RGBImage(ScriptedEnv(golden, (0, 1)), num_stack=1)  # a plain observation counts as one frame
    assert np.array_equal(unstacked.reset()[AGENTS[1]], image(0, 1))


def test_format_obs_reads_a_frame_of_the_stacked_rows():
    from smarts_amd.env.format_obs import FormatObs

    rng = np.random.default_rng(11)
    E, N, k = 2, 3, 3
    rows = {
        "ego_pos": rng.normal(size=(E, N, 3)), "ego_f32": rng.normal(size=(E, N, nat.EGO_F32_COUNT)).astype(np.float32),
        "ego_lane": np.zeros((E, N, 2), np.int16), "events": np.zeros((E, N, nat.EV_COUNT), np.uint8),
        "dist": np.zeros((E, N)), "collidees": np.zeros((E, N), np.int64),
        "rgb": rng.integers(0, 256, (E, N, H, W, 3)).astype(np.uint8),
    }
    rows["stack_ego_pos"] = rng.normal(size=(E, N, k, 3))
    rows["stack_rgb"] = rng.integers(0, 256, (E, N, k, H, W, 3)).astype(np.uint8)
    plain = FormatObs.from_rows(rows, 1, 2)
    assert np.array_equal(plain.rgb, rows["rgb"][1, 2]) and np.array_equal(plain.ego["pos"], rows["ego_pos"][1, 2])
    for j in range(k):
        got = FormatObs.from_rows(rows, 1, 2, frame=j)
        assert np.array_equal(got.rgb, rows["stack_rgb"][1, 2, j]) and np.array_equal(got.ego["pos"], rows["stack_ego_pos"][1, 2, j])
        assert np.array_equal(got.ego["heading"], plain.ego["heading"])  # (ego_f32 is not stacked here: the unstacked row)
    with pytest.raises(ValueError, match="frame 3"):
        FormatObs.from_rows(rows, 1, 2, frame=k)


# ------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
    from smarts_amd import build

    if not os.path.exists(build.LIB_PATH):
        build.build()
    return nat.load_library()


def test_abi_additions(lib):
    assert lib.smx_struct_size(0) == C.sizeof(nat.SmxConfig)
    # the new member took padding: no other member moved
    assert nat.SmxConfig.frame_stack.offset == nat.SmxConfig.max_episode_steps.offset + 4
    assert nat.SmxConfig.not_moving_time.offset == nat.SmxConfig.max_episode_steps.offset + 8
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_bind_frame_stack(smx_handle h, int32_t source, int32_t layout, void* stack_dev, uint64_t bytes);" in header
    assert ("int smx_check_frame_stack(const smx_config* cfg, int32_t source, int32_t layout, uint64_t bytes, char* err, "
            "uint64_t err_len);") in header
    assert "SMX_STACK_SOURCE_RGB = 1 << 16" in header and nat.STACK_SOURCE_RGB == 1 << 16
    assert "enum { SMX_STACK_FRAMES = 0, SMX_STACK_DSTACK = 1 };" in header and (nat.STACK_FRAMES, nat.STACK_DSTACK) == (0, 1)
    assert "smx_bind_frame_stack" in nat.EXPORTS and "smx_check_frame_stack" in nat.EXPORTS
    assert nat.stack_source("rgb") == nat.STACK_SOURCE_RGB and nat.stack_source("ego_pos") == 0
    assert nat.stack_source("ec_rw_heading") == len(nat.OUTPUT_BUFFERS) - 1
    for row in ("env_done", "learner", "final_ego_pos", "no_such_row"):
        with pytest.raises(ValueError):
            nat.stack_source(row)
    assert (SimConfig().frame_stack, tuple(SimConfig().frame_stack_rows), SimConfig().frame_stack_rgb_dstack) == (0, (), False)


def _config(k=3, E=3, N=8, sensors=nat.SENSOR_WAYPOINTS | nat.SENSOR_RGB | nat.SENSOR_OGM):
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.dt = E, N, 0.1
    c.sensors, c.frame_stack = sensors, k
    c.wp_paths, c.wp_len = 4, 20
    c.rgb_width, c.rgb_height, c.rgb_resolution = 48, 32, 50 / 32
    c.ogm_width, c.ogm_height, c.ogm_resolution = 16, 16, 1.0
    return c


def _check(lib, c, source, layout, count):
    err = C.create_string_buffer(512)
    rc = lib.smx_check_frame_stack(C.byref(c), source, layout, count, err, len(err))
    return rc, err.value.decode()


def test_check_frame_stack(lib):
    T, k = 3 * 8, 3
    src = nat.stack_source
    per_agent = {"rgb": 32 * 48 * 3, "ogm": 256, "ego_pos": 24, "ego_f32": 100, "ego_lane": 4, "events": 9, "reward": 8, "done": 1,
                 "wp_lane_index": 80, "wp_pos": 80 * 24, "wp_count": 5, "collidees": 8}
    for row, bytes_ in per_agent.items():
        need = T * k * bytes_
        assert _check(lib, _config(), src(row), nat.STACK_FRAMES, need) == (0, ""), row
        rc, why = _check(lib, _config(), src(row), nat.STACK_FRAMES, need - 1)
        assert rc == -1 and str(need) in why and "frame stack" in why, row
    assert _check(lib, _config(k=8), src("events"), nat.STACK_FRAMES, T * 8 * 9)[0] == 0
    assert _check(lib, _config(k=2), src("events"), nat.STACK_FRAMES, T * 2 * 9)[0] == 0
    # the interleaved layout: the image alone
    assert _check(lib, _config(), src("rgb"), nat.STACK_DSTACK, T * k * per_agent["rgb"]) == (0, "")
    assert _check(lib, _config(), src("rgb"), nat.STACK_DSTACK, T * k * per_agent["rgb"] - 1)[0] == -1
    rc, why = _check(lib, _config(), src("ogm"), nat.STACK_DSTACK, 10 ** 9)
    assert rc == -1 and "DSTACK" in why
    assert _check(lib, _config(), src("rgb"), 2, 10 ** 9)[0] == -1  # no such layout
    # frame_stack: 0 is off (nothing can be bound: SMX_ERR_STATE), 1 and 9 are refused
    rc, why = _check(lib, _config(k=0), src("events"), nat.STACK_FRAMES, 10 ** 9)
    assert rc == -3 and "frame_stack" in why
    for bad in (1, 9, -1):
        rc, why = _check(lib, _config(k=bad), src("events"), nat.STACK_FRAMES, 10 ** 9)
        assert rc == -1 and "num_stack > 1" in why, bad
    # refused sources: per-env and learner rows, the final_* twins, indices that are no row, rows of sensors that are off
    for row in ("env_done", "learner", "final_ego_pos", "final_ego_f32", "final_ego_lane", "final_events", "final_dist"):
        rc, why = _check(lib, _config(), nat.OUTPUT_BUFFERS.index(row), nat.STACK_FRAMES, 10 ** 9)
        assert rc == -1 and "not a per-agent row" in why, row
    for bad in (-1, len(nat.OUTPUT_BUFFERS), nat.STACK_SOURCE_RGB + 1):
        assert _check(lib, _config(), bad, nat.STACK_FRAMES, 10 ** 9)[0] == -1
    for row in ("nb_pos", "dagm", "lidar_hit", "rw_pos", "lane_ttc", "ego_frame", "ec_wp_pos", "via_near"):
        rc, why = _check(lib, _config(), src(row), nat.STACK_FRAMES, 10 ** 9)
        assert rc == -1 and "is off" in why, row
    no_rgb = _config(sensors=nat.SENSOR_WAYPOINTS)
    assert _check(lib, no_rgb, src("rgb"), nat.STACK_FRAMES, 10 ** 9)[0] == -1
    assert _check(lib, no_rgb, src("ogm"), nat.STACK_FRAMES, 10 ** 9)[0] == -1
    assert lib.smx_check_frame_stack(None, 0, 0, 0, None, 0) == -1


def test_sim_config_refuses_what_the_library_would(monkeypatch):
    """BatchedSim validates frame_stack before it touches the device: ValueError, whatever the box."""
    from smarts_amd import engine

    monkeypatch.setattr(engine.torch.cuda, "is_available", lambda: True)
    for kw in (dict(frame_stack=1), dict(frame_stack=9), dict(frame_stack=0, frame_stack_rows=("ego_pos",)),
               dict(frame_stack=0, frame_stack_rgb_dstack=True)):
        with pytest.raises(ValueError, match="frame_stack"):
            engine.BatchedSim(None, SimConfig(num_envs=1, num_vehicles=2, **kw))

"""Per-agent action spaces without a device (include/smx.h smx_set_agent_spaces / smx_check_agent_spaces / smx_step_mixed).

tests/native/host_agent_spaces.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over the
shim hip_runtime.h and the HIP memory stand-in shim/hip_memory.h — drives the check over every refusal, the handle's fill
then commit, the blob's contents, which tick entry is taken while a table is bound and the refused kinematic bindings,
with every HIP call failing in turn.  tests/native/host_plan_agent_spaces.cpp drives the launch plan.  The rest is the
entry point on the built library, the declarations, and the env layer's host half: which specs BatchCore takes, and the
encoder of a mixed fleet's actions."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "smarts_amd", "csrc")


def _build_and_run(tmp_path, name):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", CSRC,
           os.path.join(NATIVE, name + ".cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    # the sanitizer runtime is linked into the program itself: its check of the library order has nothing to protect
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert proc.returncode == 0 and "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, \
        (proc.stdout[-3000:], proc.stderr[-3000:])
    return json.loads(proc.stdout.strip().splitlines()[-1])


def test_agent_spaces_on_the_host_under_sanitizers(tmp_path):
    res = _build_and_run(tmp_path, "host_agent_spaces")
    assert res["sweep_points"] == res["hip_calls"] > 60 and res["skipped"] == 0, res
    assert res["refused"] + res["release_points"] == res["sweep_points"] and res["refused"] > 40, res
    assert res["mallocs"] == res["frees"] and res["steps"] >= 14 and res["checks"] > 5000, res


def test_plan_with_a_table_of_agent_spaces(tmp_path):
    res = _build_and_run(tmp_path, "host_plan_agent_spaces")
    assert res["plans"] == 1536 * 5 and res["large_one_lane"] == 0 and min(res["small"], res["large_teams"]) > 1000, res
    assert res["uniform"] == 768, res  # the ticks whose table is cfg.action_space alone


def test_header_declares_the_entry_points_and_keeps_every_struct():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_agent_spaces(smx_handle h, const smx_agent_spaces* spaces);" in header
    assert "int smx_check_agent_spaces(const smx_config* cfg, const smx_agent_spaces* spaces, char* err, uint64_t err_len);" in header
    assert ("int smx_step_mixed(smx_handle h, const smx_mixed_actions* acts, const smx_state* st, const smx_spawns* sp,\n"
            "                   const smx_outputs* out, void* hip_stream);") in header
    assert "previous space" in header and "smx_reset after rebinding is recommended" in header
    from smarts_amd import _native as nat

    for name in ("smx_set_agent_spaces", "smx_check_agent_spaces", "smx_step_mixed"):
        assert name in nat.EXPORTS
    assert C.sizeof(nat.SmxAgentSpaces) == 16 and C.sizeof(nat.SmxMixedActions) == 32
    assert C.sizeof(nat.SmxAgentEntry) == 56 and C.sizeof(nat.SmxAgentDims) == 16  # the neighbours keep their layout
    lib = nat.load_library()
    assert lib.smx_struct_size(0) == C.sizeof(nat.SmxConfig)
    assert len(lib.smx_step_mixed.argtypes) == 6 and len(lib.smx_set_agent_spaces.argtypes) == 2
    assert set(nat.MIXABLE_SPACES) | {"TargetPose", "TrajectoryWithTime", "Imitation"} == set(nat.ACTION_SPACES)
    # the plan header: the value stands first, the older ones keep theirs
    plan = open(os.path.join(CSRC, "smx_plan.h")).read()
    assert "enum class Control : uint8_t { MIXED = 10, KINEMATIC_BUBBLES = 9, NONE = 0," in plan
    assert "FAST_LISTED, KINEMATIC, KINEMATIC_FOLLOW, KINEMATIC_HANDOVER };" in plan


def test_smx_check_agent_spaces_needs_no_device():
    from smarts_amd import _native as nat
    from smarts_amd import engine

    lib = nat.load_library()
    N, S = 6, 2

    def run(spaces, cfg_space="Lane", n=None, null=False):
        cfg = nat.SmxConfig()
        cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.dt = 3, N, S, 0.1
        cfg.action_space = nat.ACTION_SPACES[cfg_space]
        table = np.asarray(spaces, dtype=np.int32)
        sp = nat.SmxAgentSpaces()
        sp.space_host, sp.n_agents = (None if null else table.ctypes.data), (len(table) if n is None else n)
        err = C.create_string_buffer(512)
        return lib.smx_check_agent_spaces(C.byref(cfg), C.byref(sp), err, len(err)), err.value.decode()

    A = nat.ACTION_SPACES
    assert run([A["Lane"], A["Continuous"], A["Trajectory"], A["MPC"]]) == (0, "")
    assert run([A["ActuatorDynamic"]] * 4, cfg_space="LaneWithContinuousSpeed") == (0, "")  # all equal is legal
    rc, why = run([0, 0, 0, 0], null=True)
    assert rc == -1 and "null table" in why
    rc, why = run([0, 0, 0])
    assert rc == -1 and "n_agents is 3" in why and "num_vehicles - num_social is 4" in why and "slot 3 has no entry" in why, why
    rc, why = run([0, 0, 0, 0, 0])
    assert rc == -1 and "n_agents is 5" in why and "slot 4 is no agent slot" in why, why
    rc, why = run([0, 1, A["TargetPose"], 0])
    assert rc == -1 and "slot 2" in why and "TargetPose" in why and "kinematic" in why, why
    rc, why = run([0, 1, 0, A["Imitation"]])
    assert rc == -1 and "slot 3" in why and "Imitation" in why, why
    rc, why = run([A["TrajectoryWithTime"], 1, 0, 0])
    assert rc == -1 and "slot 0" in why and "TrajectoryWithTime" in why, why
    rc, why = run([0, 9, 0, 0])
    assert rc == -1 and "slot 1" in why and "9 is no SMX_ACTION_SPACE_* value" in why, why
    rc, why = run([0, 0, -1, 0])
    assert rc == -1 and "slot 2" in why and "-1 is no SMX_ACTION_SPACE_* value" in why, why
    for kinematic in ("TargetPose", "TrajectoryWithTime", "Imitation"):
        rc, why = run([0, 1, 0, 0], cfg_space=kinematic)
        assert rc == -1 and f"cfg.action_space is {kinematic}" in why, why
    assert lib.smx_check_agent_spaces(None, None, None, 0) == -1
    # the same through the engine's wrapper
    engine.check_agent_spaces("Lane", N, S, ["Lane", "Continuous", "Trajectory", "MPC"])
    with pytest.raises(ValueError, match="slot 1.*Imitation"):
        engine.check_agent_spaces("Lane", N, S, ["Lane", "Imitation", "Trajectory", "MPC"])
    with pytest.raises(ValueError, match="n_agents is 2"):
        engine.check_agent_spaces("Lane", N, S, ["Lane", "Lane"])
    with pytest.raises(ValueError, match="not on the accelerated path"):
        engine.check_agent_spaces("Lane", N, S, ["Lane", "Lane", "Lane", "MultiTargetPose"])


def _specs(types, **kw):
    from smarts_amd.env.agent import AgentSpec
    from smarts_amd.env.agent_interface import AgentInterface

    shared = dict(waypoints=True, neighborhood_vehicles=True, max_episode_steps=20)
    shared.update(kw)
    return {f"agent-{i}": AgentSpec(interface=AgentInterface.from_type(t, **shared)) for i, t in enumerate(types)}


def test_batchcore_takes_specs_that_differ_in_their_action_space_only(monkeypatch):
    """No device: BatchedSim is replaced by a recorder."""
    import smarts_amd.engine as engine
    from smarts_amd.env.agent_interface import AgentType, Waypoints
    from smarts_amd.env.core import BatchCore
    from smarts_amd.env.hiway_env import HiWayEnv
    from smarts_amd.env.parallel_env import ParallelEnv

    seen = []

    class Recorder:
        def __init__(self, cm, cfg, **kw):
            self.cfg, self.device, self.spaces = cfg, "cpu", "never set"
            seen.append(self)

        def set_agent_spaces(self, spaces):
            self.spaces = list(spaces)

        def close(self):
            pass

    monkeypatch.setattr(engine, "BatchedSim", Recorder)
    kw = dict(num_envs=2, dt=0.1, seed=1, auto_reset=False)
    mixed = _specs([AgentType.Laner, AgentType.Standard, AgentType.LanerWithSpeed, AgentType.Tracker, AgentType.StandardWithAbsoluteSteering])
    core = BatchCore("scenarios/loop", mixed, num_social=2, **kw)
    assert core.mixed and seen[-1].spaces == ["Lane", "ActuatorDynamic", "LaneWithContinuousSpeed", "Trajectory", "Continuous"]
    # sensors and done criteria are the shared part's; cfg.action_space is the first agent's
    cfg = seen[-1].cfg
    assert cfg.action_space == "Lane" and cfg.neighbors and cfg.waypoints and cfg.max_episode_steps == 20 and cfg.num_vehicles == 7
    # equal interfaces: no table is bound, nothing changes
    core = BatchCore("scenarios/loop", _specs([AgentType.Tracker] * 3), **kw)
    assert not core.mixed and seen[-1].spaces == "never set" and seen[-1].cfg.action_space == "Trajectory"
    # any other difference stays refused
    differ = _specs([AgentType.Laner, AgentType.Tracker])
    differ["agent-1"].interface = differ["agent-1"].interface.replace(max_episode_steps=21)
    with pytest.raises(NotImplementedError, match="only the action space may differ"):
        BatchCore("scenarios/loop", differ, **kw)
    differ = _specs([AgentType.Laner, AgentType.Laner])
    differ["agent-1"].interface = differ["agent-1"].interface.replace(waypoints=Waypoints(lookahead=16))
    with pytest.raises(NotImplementedError, match="only the action space may differ"):
        BatchCore("scenarios/loop", differ, **kw)
    # the kinematic spaces, MPC and an agent without an action space stay out of a mix
    for other in (AgentType.TrajectoryInterpolator, AgentType.Imitation, AgentType.MPCTracker, AgentType.Buddha):
        with pytest.raises(NotImplementedError):
            BatchCore("scenarios/loop", _specs([AgentType.Laner, other]), **kw)
    with pytest.raises(NotImplementedError, match="ego_centric"):
        BatchCore("scenarios/loop", _specs([AgentType.Laner, AgentType.Tracker]), ego_centric=True, **kw)
    BatchCore("scenarios/loop", _specs([AgentType.Tracker, AgentType.Tracker]), ego_centric=True, **kw)  # (uniform: as before)
    # HiWayEnv needs no new argument; ParallelEnv compares agent by agent
    env = HiWayEnv(["scenarios/loop"], mixed)
    env._ensure_core()
    assert seen[-1].spaces[3] == "Trajectory"
    env._core = None
    swapped = dict(zip(mixed, list(mixed.values())[::-1]))
    assert HiWayEnv(["scenarios/loop"], mixed).signature() == env.signature() != HiWayEnv(["scenarios/loop"], swapped).signature()
    with pytest.raises(ValueError, match="each agent's interface"):
        ParallelEnv([lambda: HiWayEnv(["scenarios/loop"], mixed), lambda: HiWayEnv(["scenarios/loop"], swapped)], auto_reset=False)


def test_mixed_action_encoder():
    from smarts_amd import _native as nat
    from smarts_amd.engine import pack_trajectory
    from smarts_amd.env.agent import AgentSpec
    from smarts_amd.env.agent_interface import ActionSpaceType as A
    from smarts_amd.env.agent_interface import AgentType
    from smarts_amd.env.core import encode_mixed_actions

    specs = _specs([AgentType.Laner, AgentType.Standard, AgentType.LanerWithSpeed, AgentType.Tracker, AgentType.StandardWithAbsoluteSteering])
    ids = list(specs)
    # an adapter of the agent's own: the Tracker's policy hands a dict, its adapter makes the trajectory of it
    specs["agent-3"] = AgentSpec(interface=specs["agent-3"].interface, action_adapter=lambda a: None if a is None else a["trajectory"])
    spaces = [s.interface.action for s in specs.values()]
    assert spaces == [A.Lane, A.ActuatorDynamic, A.LaneWithContinuousSpeed, A.Trajectory, A.Continuous]
    traj = ([0.0, 1.0, 2.0], [5.0, 5.0, 5.5], [0.1, 0.1, 0.2], [3.0, 3.5, 4.0])
    E, slots = 3, 7  # five agents and two social slots
    per_env = [
        {"agent-0": "change_lane_left", "agent-1": (0.5, 0.0, -0.25), "agent-2": (7.5, -1), "agent-3": {"trajectory": traj},
         "agent-4": np.array([1.0, 0.25, 0.5])},
        {"agent-0": None, "agent-1": None, "agent-2": None, "agent-3": None, "agent-4": None},
        {"agent-2": (0.0, 0), "agent-0": "slow_down"},  # agents without an entry send no action
    ]
    lane, floats, packed, counts = encode_mixed_actions(ids, specs, spaces, E, slots, per_env)
    assert lane.dtype == np.int8 and lane.shape == (E, slots) and floats.dtype == np.float32 and floats.shape == (E, slots, 3)
    assert packed.dtype == np.float64 and packed.shape == (E, slots, 4, nat.TRAJ_COLS) and counts.dtype == np.int32
    assert lane.tolist() == [[2, -1, -1, -1, -1, -1, -1], [-1] * 7, [1, -1, -1, -1, -1, -1, -1]]
    assert floats[0, 1].tolist() == [0.5, 0.0, -0.25] and floats[0, 2].tolist() == [7.5, -1.0, 0.0] and floats[0, 4].tolist() == [1.0, 0.25, 0.5]
    assert np.isnan(floats[0, [0, 3, 5, 6]]).all() and np.isnan(floats[1]).all()
    assert floats[2, 2].tolist() == [0.0, 0.0, 0.0] and np.isnan(floats[2, [0, 1, 3, 4, 5, 6]]).all()
    want, n = pack_trajectory(traj)
    assert counts.tolist() == [[0, 0, 0, n, 0, 0, 0], [0] * 7, [0] * 7] and n == 3
    assert np.array_equal(packed[0, 3], want) and not packed[1:].any() and not packed[0, [0, 1, 2, 4, 5, 6]].any()
    # each agent's action is checked as its own space checks it
    with pytest.raises(KeyError):
        encode_mixed_actions(ids, specs, spaces, E, slots, [{"agent-0": "fly"}])
    with pytest.raises(TypeError):
        encode_mixed_actions(ids, specs, spaces, E, slots, [{"agent-0": (1.0, 0.0, 0.0)}])
    with pytest.raises(ValueError, match="LaneWithContinuousSpeed"):
        encode_mixed_actions(ids, specs, spaces, E, slots, [{"agent-2": (1.0, 0.0, 0.0)}])
    with pytest.raises(ValueError, match="three floats"):
        encode_mixed_actions(ids, specs, spaces, E, slots, [{"agent-1": (1.0, 0.0)}])

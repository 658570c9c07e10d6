"""The state guard without a device (include/smx.h smx_set_guard; smarts_amd/csrc/smx_guard.h).

tests/native/host_guard.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over the shim
hip_runtime.h — drives the header's in-bounds test, the guard box, the index bound at the largest margin (for the grids
of the three shipped maps, read from their packed tables) and the resolution table.  The rest is the validation:
smx_check_guard on the built library, SimConfig, and BatchCore's keyword pass-through."""
import ctypes as C
import json
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
MAPS = {"loop": "loop", "4lane": "intersections/4lane", "minicity": "minicity"}


def _grids(name):
    """The ten grid numbers of a shipped map, from the table struct smx_load_map is given."""
    from smarts_amd.map_compiler import compile_map, map_tables_struct
    from smarts_amd.sumo_map import load_net

    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", MAPS[name])))
    t, keep = map_tables_struct(cm)
    return [repr(float(v)) if isinstance(v, float) else str(int(v))
            for v in (t.lpg_x0, t.lpg_y0, t.lpg_cell, t.lpg_nx, t.lpg_ny, t.sg_x0, t.sg_y0, t.sg_cell, t.sg_nx, t.sg_ny)]


def test_guard_header_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_guard")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_guard.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    args = [a for name in ("loop", "4lane", "minicity") for a in _grids(name)]
    # the environment is inherited as it is; the sanitizer runtime is linked into the program itself, so its check of
    # the library order (which a preload of the caller's would trip) has nothing to protect here
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=120)
    assert proc.returncode == 0 and "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, \
        (proc.stdout[-3000:], proc.stderr[-3000:])
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    assert res["maps"] == 3 and res["checks"] > 300, res
    # the farthest cell index of the three maps at SMX_GUARD_MARGIN_MAX, computed there in int64
    assert 0 < res["worst_index"] < 2 ** 30, res


def test_header_declares_the_guard():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_guard(smx_handle h, uint8_t* guard_dev, uint64_t count, double margin);" in header
    assert "int smx_check_guard(const smx_config* cfg, uint64_t count, double margin, char* err, uint64_t err_len);" in header
    assert "SMX_F_GUARDED = 1 << 2" in header and "SMX_F_RESERVED2" not in header
    assert "#define SMX_GUARD_MARGIN_DEFAULT 1000.0" in header and "#define SMX_GUARD_MARGIN_MAX 1.0e6" in header
    from smarts_amd import _native as nat

    assert "smx_set_guard" in nat.EXPORTS and "smx_check_guard" in nat.EXPORTS
    assert (nat.GUARD_STEP, nat.GUARD_STATE, nat.GUARD_SPAWN, nat.F_GUARDED) == (1, 2, 4, 4)
    assert (nat.GUARD_MARGIN_DEFAULT, nat.GUARD_MARGIN_MAX) == (1000.0, 1.0e6)


def _check(lib, nat, E, N, count, margin):
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles = E, N
    err = C.create_string_buffer(512)
    return lib.smx_check_guard(C.byref(c), count, margin, err, len(err)), err.value.decode()


def test_smx_check_guard_needs_no_device():
    from smarts_amd import _native as nat
    from smarts_amd.engine import check_guard

    lib = nat.load_library()
    assert b"0.2" in lib.smx_version()  # bumped with the ABI addition
    assert _check(lib, nat, 4, 4, 16, 1000.0) == (0, "")
    assert _check(lib, nat, 4, 4, 64, 0.0)[0] == 0 and _check(lib, nat, 4, 4, 16, 1.0e6)[0] == 0
    rc, why = _check(lib, nat, 4, 4, 15, 1000.0)  # short count
    assert rc == -1 and "15" in why and "16" in why
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf"), math.nextafter(1.0e6, math.inf)):
        rc, why = _check(lib, nat, 4, 4, 16, bad)
        assert rc == -1 and "margin" in why, (bad, why)
    assert _check(lib, nat, 0, 4, 16, 1000.0)[0] == -1
    assert lib.smx_check_guard(None, 0, 0.0, None, 0) == -1
    # the Python wrapper
    check_guard(4, 4, 16)
    check_guard(4, 4, 16, margin=0.0)
    with pytest.raises(ValueError, match="16"):
        check_guard(4, 4, 3)
    with pytest.raises(ValueError, match="margin"):
        check_guard(4, 4, 16, margin=float("nan"))


def test_simconfig_validates_the_margin():
    from smarts_amd.engine import SimConfig

    c = SimConfig()
    assert c.state_guard is False and c.state_guard_margin == 1000.0
    assert SimConfig(state_guard=True, state_guard_margin=0).state_guard_margin == 0
    SimConfig(state_guard=True, state_guard_margin=1.0e6)
    for bad in (-1.0, float("nan"), float("inf"), 1.0e6 + 1.0, "50", None, True):
        with pytest.raises(ValueError, match="state_guard_margin"):
            SimConfig(state_guard=True, state_guard_margin=bad)


def test_batchcore_passes_the_guard_keywords_through(monkeypatch):
    """No device: BatchedSim is replaced by a recorder."""
    import smarts_amd.engine as engine
    from smarts_amd.env.agent import AgentSpec
    from smarts_amd.env.agent_interface import AgentInterface, AgentType
    from smarts_amd.env.core import BatchCore
    from smarts_amd.env.hiway_env import HiWayEnv

    seen = []

    class Recorder:
        def __init__(self, cm, cfg, **kw):
            seen.append(cfg)
            self.device = "cpu"

        def close(self):
            pass

    monkeypatch.setattr(engine, "BatchedSim", Recorder)
    specs = {"a": AgentSpec(interface=AgentInterface.from_type(AgentType.Laner, max_episode_steps=10))}
    BatchCore("scenarios/loop", specs, num_envs=2, dt=0.1, seed=1, auto_reset=False)
    assert seen[-1].state_guard is False and seen[-1].state_guard_margin == 1000.0
    BatchCore("scenarios/loop", specs, num_envs=2, dt=0.1, seed=1, auto_reset=False, state_guard=True, state_guard_margin=50.0)
    assert seen[-1].state_guard is True and seen[-1].state_guard_margin == 50.0
    with pytest.raises(ValueError, match="state_guard_margin"):
        BatchCore("scenarios/loop", specs, num_envs=2, dt=0.1, seed=1, auto_reset=False, state_guard=True, state_guard_margin=-1.0)
    env = HiWayEnv(["scenarios/loop"], specs, state_guard=True, state_guard_margin=25.0)
    env._ensure_core()
    assert seen[-1].state_guard is True and seen[-1].state_guard_margin == 25.0
    assert HiWayEnv(["scenarios/loop"], specs).signature() != env.signature()
    env._core = None

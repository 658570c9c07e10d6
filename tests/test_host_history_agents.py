"""History agents without a device: the validation behind smx_set_history_agents / smx_check_history_agents
(smarts_amd/csrc/smx_host.h), what the kernels ask of the follow table (smarts_amd/csrc/smx_history.h) and the launch
plan's choice for smx_step_history_agents (smarts_amd/csrc/smx_plan.h).

tests/native/host_history_agents.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over
the shim hip_runtime.h — drives the first two over heap tables of exactly the stated size.  The rest is the entry point on
the built library, the declarations and the plan."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
KINEMATIC, KINEMATIC_FOLLOW = 6, 7  # smx_plan.h: enum class Control


def test_history_agent_headers_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_history_agents")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_history_agents.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    # the environment is inherited as it is; the sanitizer runtime is linked into the program itself, so its check of
    # the library order (which a preload of the caller's would trip) has nothing to protect here
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert proc.returncode == 0 and "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, \
        (proc.stdout[-3000:], proc.stderr[-3000:])
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    assert res["checks"] > 500, res


def test_header_declares_the_history_agents():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_history_agents(smx_handle h, const smx_history_agents* ha);" in header
    assert "int smx_check_history_agents(const smx_config* cfg, const smx_social_history* hist, const smx_history_agents* ha, char* err," in header
    assert "int smx_step_history_agents(smx_handle h, const smx_state* st, const smx_spawns* sp, const smx_outputs* out, void* hip_stream);" in header
    assert "enum { SMX_HA_FOLLOWING = 0, SMX_HA_LEFT = 1, SMX_HA_ABSENT = 2 };" in header
    assert "SMX_F_LEFT = 1 << 7" in header
    from smarts_amd import _native as nat

    for name in ("smx_set_history_agents", "smx_check_history_agents", "smx_step_history_agents"):
        assert name in nat.EXPORTS
    assert C.sizeof(nat.SmxHistoryAgents) == 48
    assert C.sizeof(nat.SmxSocialHistory) == 64  # smx_social_history keeps its layout
    assert (nat.HA_FOLLOWING, nat.HA_LEFT, nat.HA_ABSENT) == (0, 1, 2)
    # no new action space: the Imitation agent is the follower
    assert max(nat.ACTION_SPACES.values()) == 8 and nat.ACTION_SPACES["Imitation"] == 8


def _check(lib, nat, cfg, rows, vehicle_count, action_count=None, status_count=None, vehicle=True):
    hs = nat.SmxSocialHistory()
    hs.rows = rows
    ha = nat.SmxHistoryAgents()
    keep = np.zeros(4, dtype=np.int32)  # (host memory stands in for the device pointers: the check reads no element)
    ha.vehicle_dev, ha.vehicle_count = (keep.ctypes.data if vehicle else None), vehicle_count
    if action_count is not None:
        ha.action_dev, ha.action_count = keep.ctypes.data, action_count
    if status_count is not None:
        ha.status_dev, ha.status_count = keep.ctypes.data, status_count
    err = C.create_string_buffer(512)
    return lib.smx_check_history_agents(C.byref(cfg), C.byref(hs), C.byref(ha), err, len(err)), err.value.decode()


def test_smx_check_history_agents_needs_no_device():
    from smarts_amd import _native as nat

    lib = nat.load_library()
    cfg = nat.SmxConfig()
    cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.dt = 4, 6, 3, 0.1
    cfg.action_space = nat.ACTION_SPACES["Imitation"]
    E, N, A, R = 4, 6, 3, 2
    assert _check(lib, nat, cfg, R, R * E * A) == (0, "")
    assert _check(lib, nat, cfg, R, R * E * A, 3 * E * N, E * N) == (0, "")
    rc, why = _check(lib, nat, cfg, R, R * E * A - 1)
    assert rc == -1 and "vehicle" in why and str(R * E * A) in why
    rc, why = _check(lib, nat, cfg, R, R * E * A, 3 * E * N - 1, E * N)
    assert rc == -1 and "action" in why
    rc, why = _check(lib, nat, cfg, R, R * E * A, 3 * E * N, E * N - 1)
    assert rc == -1 and "status" in why
    rc, why = _check(lib, nat, cfg, R, R * E * A, vehicle=False)
    assert rc == -1 and "vehicle_dev" in why
    assert _check(lib, nat, cfg, 0, R * E * A)[0] == -1
    for name, code in nat.ACTION_SPACES.items():
        cfg.action_space = code
        rc, why = _check(lib, nat, cfg, R, R * E * A)
        assert (rc == 0) == (name == "Imitation"), name
        if rc:
            assert rc == -1 and "action_space" in why and "IMITATION" in why, why
    assert lib.smx_check_history_agents(None, None, None, None, 0) == -1


def test_the_plan_picks_the_follow_form_and_nothing_else(tmp_path):
    """smx_step_history_agents (PlanInputs::follow_entry) turns Control::KINEMATIC into KINEMATIC_FOLLOW in both launch
    forms, with and without the guard, and no other field of the plan moves with it."""
    lib_path = str(tmp_path / "libhost_plan_history_agents.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_plan_history_agents.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_history_agents.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    imitation = 8
    seen = set()
    for total, strategy, junctions, auto_reset, guard in itertools.product((64, 32768, 131072), range(5), (0, 1), (0, 1), (0, 1)):
        for follow in (0, 1):
            same = C.c_int(0)
            control = lib.host_plan_history_agents((C.c_int * 9)(total // 32, 32, strategy, junctions, follow, 1, auto_reset, guard, imitation),
                                                   C.byref(same))
            assert control == (KINEMATIC_FOLLOW if follow else KINEMATIC) and same.value == 1, (total, strategy, junctions, auto_reset, guard, follow)
            seen.add(control)
    assert seen == {KINEMATIC, KINEMATIC_FOLLOW}
    # a reset call launches no controller whatever the entry
    same = C.c_int(0)
    assert lib.host_plan_history_agents((C.c_int * 9)(4, 32, 0, 0, 1, 0, 0, 0, imitation), C.byref(same)) == 0 and same.value == 1

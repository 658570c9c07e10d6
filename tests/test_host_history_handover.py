"""Handing history agents over to actions, without a device: the validation behind smx_set_history_handover /
smx_check_history_handover (smarts_amd/csrc/smx_host.h), what k_control_kinematic's HANDOVER form asks of the table
(smarts_amd/csrc/smx_history.h) and the launch plan's choice for smx_step_history_handover (smarts_amd/csrc/smx_plan.h).

tests/native/host_history_handover.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan
over the shim hip_runtime.h — drives the first two over heap tables of exactly the stated size.  The rest is the entry
point on the built library, the declarations and the plan."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
KINEMATIC, KINEMATIC_FOLLOW, KINEMATIC_HANDOVER = 6, 7, 8  # smx_plan.h: enum class Control


def test_handover_headers_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_history_handover")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_history_handover.cpp"), "-o", exe]
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
    print(res)
    assert res["checks"] > 1000 and res["shapes"] == 5, res


def test_header_declares_the_handover():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_history_handover(smx_handle h, const smx_history_handover* ho);" in header
    assert "int smx_check_history_handover(const smx_config* cfg, const smx_social_history* hist, const smx_history_handover* ho, char* err," in header
    assert ("int smx_step_history_handover(smx_handle h, const float* actions_dev, const smx_state* st, const smx_spawns* sp,\n"
            "                              const smx_outputs* out, void* hip_stream);") in header
    lines = header.splitlines()
    driven = [ln for ln in lines if "SMX_HA_DRIVEN = 3" in ln]
    assert len(driven) == 1 and driven[0].startswith("enum { SMX_HA_DRIVEN = 3 };")
    # ... on a line of its own: the three values before it keep theirs
    assert "enum { SMX_HA_FOLLOWING = 0, SMX_HA_LEFT = 1, SMX_HA_ABSENT = 2 };" in lines
    assert "const int32_t* tick_dev;" in header and "uint64_t tick_count;" in header
    # the rule is written into the header
    for phrase in ("H >= 0 && t >= H", "never sets SMX_F_LEFT", "rewrite it in place", "SMX_HA_DRIVEN"):
        assert phrase in header, phrase
    from smarts_amd import _native as nat

    for name in ("smx_set_history_handover", "smx_check_history_handover", "smx_step_history_handover"):
        assert name in nat.EXPORTS
    assert C.sizeof(nat.SmxHistoryHandover) == 16
    assert C.sizeof(nat.SmxHistoryAgents) == 48 and C.sizeof(nat.SmxSocialHistory) == 64  # the older two keep their layouts
    assert (nat.HA_FOLLOWING, nat.HA_LEFT, nat.HA_ABSENT, nat.HA_DRIVEN) == (0, 1, 2, 3)
    lib = nat.load_library()
    assert lib.smx_step_history_handover.argtypes[1] is C.c_void_p and len(lib.smx_step_history_handover.argtypes) == 6
    assert len(lib.smx_set_history_handover.argtypes) == 2 and len(lib.smx_check_history_handover.argtypes) == 5
    # the plan header: the value is appended, the older ones keep theirs
    plan = open(os.path.join(ROOT, "smarts_amd", "csrc", "smx_plan.h")).read()
    assert "FAST_LISTED, KINEMATIC, KINEMATIC_FOLLOW, KINEMATIC_HANDOVER };" in plan
    assert plan.index("bool ogm_mask;") < plan.index("bool handover_entry;") < plan.index("enum class AliveList")


def _check(lib, nat, cfg, rows, tick_count, table=True):
    hs = nat.SmxSocialHistory()
    hs.rows = rows
    ho = nat.SmxHistoryHandover()
    keep = np.zeros(4, dtype=np.int32)  # (host memory stands in for the device pointer: the check reads no element)
    ho.tick_dev, ho.tick_count = (keep.ctypes.data if table else None), tick_count
    err = C.create_string_buffer(512)
    return lib.smx_check_history_handover(C.byref(cfg), C.byref(hs), C.byref(ho), err, len(err)), err.value.decode()


def _config(nat, E=4, N=6, S=3):
    cfg = nat.SmxConfig()
    cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.dt = E, N, S, 0.1
    cfg.action_space = nat.ACTION_SPACES["Imitation"]
    return cfg


def test_check_accepts_the_exact_table():
    from smarts_amd import _native as nat

    lib = nat.load_library()
    E, A, R = 4, 3, 2
    assert _check(lib, nat, _config(nat), R, R * E * A) == (0, "")
    assert _check(lib, nat, _config(nat), R, R * E * A + 1) == (0, "")
    assert _check(lib, nat, _config(nat), 1, E * A) == (0, "")


def test_check_refuses_a_short_table():
    from smarts_amd import _native as nat

    lib = nat.load_library()
    E, A, R = 4, 3, 2
    rc, why = _check(lib, nat, _config(nat), R, R * E * A - 1)
    assert rc == -1 and "tick" in why and str(R * E * A) in why
    assert _check(lib, nat, _config(nat), R, E * A)[0] == -1  # sized for one row of episodes against a history of two
    assert _check(lib, nat, _config(nat), R, 0)[0] == -1


def test_check_refuses_a_null_table():
    from smarts_amd import _native as nat

    rc, why = _check(nat.load_library(), nat, _config(nat), 2, 24, table=False)
    assert rc == -1 and "tick_dev" in why


def test_check_refuses_a_history_without_rows_and_a_batch_without_agent_slots():
    from smarts_amd import _native as nat

    lib = nat.load_library()
    assert _check(lib, nat, _config(nat), 0, 24)[0] == -1
    rc, why = _check(lib, nat, _config(nat, N=3, S=3), 2, 24)
    assert rc == -1 and "agent" in why
    assert _check(lib, nat, _config(nat, S=0), 2, 48)[0] == -1


def test_check_refuses_null_arguments():
    from smarts_amd import _native as nat

    lib = nat.load_library()
    assert lib.smx_check_history_handover(None, None, None, None, 0) == -1
    err = C.create_string_buffer(64)
    assert lib.smx_check_history_handover(C.byref(_config(nat)), None, None, err, len(err)) == -1 and b"null" in err.value


def test_the_plan_picks_the_handover_form_and_nothing_else(tmp_path):
    """smx_step_history_handover (PlanInputs::handover_entry) turns Control::KINEMATIC into KINEMATIC_HANDOVER in both
    launch forms, with and without the guard, follow_entry alone still gives KINEMATIC_FOLLOW, neither KINEMATIC, and no
    other field of the plan moves with either."""
    lib_path = str(tmp_path / "libhost_plan_history_handover.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_plan_history_handover.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_history_handover.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    imitation = 8
    want = {0: KINEMATIC, 1: KINEMATIC_FOLLOW, 2: KINEMATIC_HANDOVER}
    seen = set()
    for total, strategy, junctions, auto_reset, guard in itertools.product((64, 32768, 131072), range(5), (0, 1), (0, 1), (0, 1)):
        for entry in (0, 1, 2):
            same = C.c_int(0)
            control = lib.host_plan_history_handover((C.c_int * 9)(total // 32, 32, strategy, junctions, entry, 1, auto_reset, guard, imitation),
                                                     C.byref(same))
            assert control == want[entry] and same.value == 1, (total, strategy, junctions, auto_reset, guard, entry, control)
            seen.add(control)
    assert seen == {KINEMATIC, KINEMATIC_FOLLOW, KINEMATIC_HANDOVER}
    # a reset call launches no controller whatever the entry
    for entry in (0, 1, 2):
        same = C.c_int(0)
        assert lib.host_plan_history_handover((C.c_int * 9)(4, 32, 0, 0, entry, 0, 0, 0, imitation), C.byref(same)) == 0 and same.value == 1
    # a space that is not kinematic keeps its controller (the binding never lets the entry reach one; the plan does not care)
    same = C.c_int(0)
    lane = lib.host_plan_history_handover((C.c_int * 9)(4, 32, 0, 0, 0, 1, 0, 0, 0), C.byref(same))
    assert lib.host_plan_history_handover((C.c_int * 9)(4, 32, 0, 0, 2, 1, 0, 0, 0), C.byref(same)) == lane and same.value == 1

"""Delayed agent entry without a device (include/smx.h smx_set_agent_entry / smx_check_agent_entry).

tests/native/host_agent_entry.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over the
shim hip_runtime.h and the HIP memory stand-in shim/hip_memory.h — drives the check over every refusal, the handle's fill
then commit, its drop rule and the refused combinations with every HIP call failing in turn.  tests/native/
host_plan_entry.cpp drives the launch plan: with a table bound it has the entry launch in every form, and every other field
is the plan's without one.  The rest is the entry point on the built library and the declarations."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

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


def test_agent_entry_on_the_host_under_sanitizers(tmp_path):
    res = _build_and_run(tmp_path, "host_agent_entry")
    assert res["sweep_points"] == res["hip_calls"] > 60 and res["skipped"] == 0, res
    assert res["refused"] + res["release_points"] == res["sweep_points"] and res["refused"] > 40, res
    assert res["mallocs"] == res["frees"] and res["steps"] >= 20 and res["checks"] > 5000, res


def test_plan_with_an_entry_table(tmp_path):
    res = _build_and_run(tmp_path, "host_plan_entry")
    assert res["plans"] == 1536 and min(res["small"], res["large_teams"], res["large_one_lane"]) > 100, res


def test_header_declares_the_entry_points_and_keeps_every_struct():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_agent_entry(smx_handle h, const smx_agent_entry* entry);" in header
    assert "int smx_check_agent_entry(const smx_config* cfg, const smx_agent_entry* entry, char* err, uint64_t err_len);" in header
    assert "enum { SMX_ENTRY_PENDING = 0, SMX_ENTRY_BLOCKED = 1, SMX_ENTRY_ENTERED = 2 };" in header
    from smarts_amd import _native as nat

    assert "smx_set_agent_entry" in nat.EXPORTS and "smx_check_agent_entry" in nat.EXPORTS
    assert (nat.ENTRY_PENDING, nat.ENTRY_BLOCKED, nat.ENTRY_ENTERED) == (0, 1, 2)
    assert C.sizeof(nat.SmxAgentEntry) == 56
    assert C.sizeof(nat.SmxAgentDims) == 16  # the neighbours keep their layout
    lib = nat.load_library()
    assert lib.smx_struct_size(0) == C.sizeof(nat.SmxConfig)


def test_smx_check_agent_entry_needs_no_device():
    from smarts_amd import _native as nat

    lib = nat.load_library()
    E, N, S = 3, 4, 1
    ready = np.zeros((2, E, N - S), dtype=np.int32)
    ready[:, :, 1:] = [4, 9]
    check = np.zeros((2, E, N - S, 3))
    check[..., 2] = 3.68
    status, entered = (C.c_uint8 * (E * N))(), (C.c_int32 * (E * N))()

    def run(rdy, chk, rows=2, status_count=E * N):
        cfg = nat.SmxConfig()
        cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.dt = E, N, S, 0.1
        en = nat.SmxAgentEntry()
        en.ready_host, en.check_host, en.rows = rdy.ctypes.data, chk.ctypes.data, rows
        en.status_dev, en.entered_dev = C.addressof(status), C.addressof(entered)
        en.status_count, en.entered_count = status_count, E * N
        err = C.create_string_buffer(512)
        return lib.smx_check_agent_entry(C.byref(cfg), C.byref(en), err, len(err)), err.value.decode()

    assert run(ready, check) == (0, "")
    assert run(ready, check, rows=1) == (0, "")
    rc, why = run(ready, check, rows=0)
    assert rc == -1 and "rows must be >= 1" in why
    rc, why = run(ready, check, status_count=E * N - 1)
    assert rc == -1 and "status row" in why
    bad = ready.copy()
    bad[1, 2, 2] = -5
    rc, why = run(bad, check)
    assert rc == -1 and "row 1, env 2, agent 2" in why and "negative" in why, why
    bad = ready.copy()
    bad[1, 1, 0] = 1
    rc, why = run(bad, check)
    assert rc == -1 and "row 1, env 1 has no agent at tick 0" in why, why
    c = check.copy()
    c[0, 2, 1, 1] = np.nan
    rc, why = run(ready, c)
    assert rc == -1 and "not finite" in why, why
    c = check.copy()
    c[0, 0, 2, 2] = -1.0
    rc, why = run(ready, c)
    assert rc == -1 and "must be > 0" in why, why
    assert lib.smx_check_agent_entry(None, None, None, 0) == -1

"""Traffic-history replay without a device: the validation behind smx_check_social_history (smarts_amd/csrc/smx_host.h)
and the lookup the kernels run (smarts_amd/csrc/smx_history.h).

tests/native/host_history.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over the
shim hip_runtime.h — drives both over heap tables of exactly the stated size: start frames at both ends of int32, frames
just inside and outside the table, a replaced id present and absent, NaN / inf / out-of-grid rows, short counts.  The
rest is the entry point on the built library and the declarations."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def test_history_headers_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_history")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_history.cpp"), "-o", exe]
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
    assert res["checks"] > 10000, res


def test_the_lookup_header_is_host_and_device():
    """smx_history.h holds no HIP call and includes include/smx.h alone; the kernels include it directly, and the check
    lives in smx_host.h itself (whose include set tests/test_host_abi.py pins)."""
    import re

    src = open(os.path.join(ROOT, "smarts_amd", "csrc", "smx_history.h")).read()
    includes = re.findall(r'#include\s+([<"][^>"]+[>"])', src)
    assert {i for i in includes if i.startswith('"')} == {'"../../include/smx.h"'}
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("hipMalloc", "hipMemcpy", "hipLaunchKernelGGL", "__global__"):
        assert word not in code, word
    kernels = open(os.path.join(ROOT, "smarts_amd", "csrc", "smx_kernels.hip")).read()
    assert '#include "smx_history.h"' in kernels
    assert "check_social_history_impl" in open(os.path.join(ROOT, "smarts_amd", "csrc", "smx_host.h")).read()


def test_header_declares_the_history():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_social_history(smx_handle h, const smx_social_history* hist);" in header
    assert "int smx_check_social_history(const smx_config* cfg, const smx_map_tables* map, const smx_social_history* hist, char* err," in header
    assert "enum { SMX_SOCIAL_CONSTANT = 0, SMX_SOCIAL_IDM = 1 };" in header  # no third model: the replay is a binding
    from smarts_amd import _native as nat

    assert "smx_set_social_history" in nat.EXPORTS and "smx_check_social_history" in nat.EXPORTS
    assert C.sizeof(nat.SmxSocialHistory) == 64


def _check(lib, nat, cfg, tables, frames, vehicle, rows=1, start_count=None, num_social=None):
    hs = nat.SmxSocialHistory()
    hs.frames_host, hs.vehicle_host = frames.ctypes.data, vehicle.ctypes.data
    hs.n_frames, hs.num_social = frames.shape[0], frames.shape[1] if num_social is None else num_social
    start = np.zeros((rows, cfg.num_envs), dtype=np.int32)  # (the check reads neither device table: a host array stands in)
    hs.start_frame_dev, hs.rows = start.ctypes.data, rows
    hs.start_count = start.size if start_count is None else start_count
    err = C.create_string_buffer(512)
    return lib.smx_check_social_history(C.byref(cfg), C.byref(tables), C.byref(hs), err, len(err)), err.value.decode()


def test_smx_check_social_history_needs_no_device():
    from smarts_amd import _native as nat
    from smarts_amd.map_compiler import compile_map, map_tables_struct
    from smarts_amd.sumo_map import load_net

    lib = nat.load_library()
    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", "loop")))
    tables, keep = map_tables_struct(cm)
    cfg = nat.SmxConfig()
    cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.dt = 3, 4, 2, 0.1
    x0, y0 = tables.lpg_x0 + 1.0, tables.lpg_y0 + 1.0
    frames = np.zeros((5, 2, 4), dtype=np.float64)
    frames[..., 0], frames[..., 1] = x0, y0
    vehicle = np.full((5, 2), 7, dtype=np.int32)
    assert _check(lib, nat, cfg, tables, frames, vehicle) == (0, "")
    assert _check(lib, nat, cfg, tables, frames, vehicle, rows=4)[0] == 0
    rc, why = _check(lib, nat, cfg, tables, frames, vehicle, num_social=3)
    assert rc == -1 and "num_social" in why
    rc, why = _check(lib, nat, cfg, tables, frames, vehicle, rows=2, start_count=5)
    assert rc == -1 and "5" in why and "6" in why
    cfg.social_model = nat.SOCIAL_MODELS["idm"]
    rc, why = _check(lib, nat, cfg, tables, frames, vehicle)
    assert rc == -1 and "IDM" in why
    cfg.social_model = 0
    bad = frames.copy()
    bad[3, 1, 0] = tables.lpg_x0 - 1.0e4  # far outside both grids
    rc, why = _check(lib, nat, cfg, tables, bad, vehicle)
    assert rc == -1 and "frame 3" in why and "slot 1" in why and "grids" in why
    gone = vehicle.copy()
    gone[3, 1] = -1  # the row of an empty slot is never read
    assert _check(lib, nat, cfg, tables, bad, gone)[0] == 0
    bad[3, 1, 0] = float("nan")
    assert _check(lib, nat, cfg, tables, bad, vehicle)[0] == -1
    assert lib.smx_check_social_history(None, None, None, None, 0) == -1
    del keep

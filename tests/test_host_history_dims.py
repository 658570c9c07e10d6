"""Per-vehicle dimensions of a replayed history without a device: the validation behind smx_set_social_history_dims /
smx_check_social_history_dims (smarts_amd/csrc/smx_host.h) and the id -> triple lookup the kernels run
(smarts_amd/csrc/smx_history.h).

tests/native/host_history_dims.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over
the shim hip_runtime.h — drives both over heap tables of exactly the stated size: every refusal, the accepted edge values
25.0 / 10.0, and the lookup over a table whose last frame and last slot hold the largest id.  The rest is the entry point
on the built library, the declarations and the launch plan's field."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def test_dimension_headers_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_history_dims")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_history_dims.cpp"), "-o", exe]
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
    assert res["checks"] > 150, res


def test_header_declares_the_dimensions():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_social_history_dims(smx_handle h, const smx_social_dims* dims);" in header
    assert ("int smx_check_social_history_dims(const smx_config* cfg, const smx_social_history* hist, const smx_social_dims* dims, "
            "char* err,") in header
    from smarts_amd import _native as nat

    assert "smx_set_social_history_dims" in nat.EXPORTS and "smx_check_social_history_dims" in nat.EXPORTS
    assert C.sizeof(nat.SmxSocialDims) == 16
    assert C.sizeof(nat.SmxSocialHistory) == 64  # smx_social_history keeps its layout


def _check(lib, nat, cfg, vehicle, dims, n_ids=None):
    hs = nat.SmxSocialHistory()
    hs.vehicle_host, hs.n_frames, hs.num_social = vehicle.ctypes.data, vehicle.shape[0], vehicle.shape[1]
    sd = nat.SmxSocialDims()
    sd.dims_host, sd.n_ids = dims.ctypes.data, dims.shape[0] if n_ids is None else n_ids
    err = C.create_string_buffer(512)
    return lib.smx_check_social_history_dims(C.byref(cfg), C.byref(hs), C.byref(sd), err, len(err)), err.value.decode()


def test_smx_check_social_history_dims_needs_no_device():
    from smarts_amd import _native as nat

    lib = nat.load_library()
    cfg = nat.SmxConfig()
    cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.dt = 3, 4, 2, 0.1
    vehicle = np.array([[0, -1], [3, 7], [-1, 7]], dtype=np.int32)
    dims = np.tile(np.array([3.68, 1.47, 1.4]), (8, 1))
    assert _check(lib, nat, cfg, vehicle, dims) == (0, "")
    rc, why = _check(lib, nat, cfg, vehicle, dims, n_ids=7)
    assert rc == -1 and "7" in why and "n_ids" in why
    assert _check(lib, nat, cfg, vehicle, dims, n_ids=0)[0] == -1
    for word, cap, name in ((0, 25.0, "length"), (1, 25.0, "width"), (2, 10.0, "height")):
        edge = dims.copy()
        edge[5, word] = cap
        assert _check(lib, nat, cfg, vehicle, edge)[0] == 0, name
        for bad in (np.nextafter(cap, 100.0), 0.0, -1.0, np.nan, np.inf):
            edge[5, word] = bad
            rc, why = _check(lib, nat, cfg, vehicle, edge)
            assert rc == -1 and "vehicle 5" in why and name in why, (name, bad, why)
    cfg.num_social = 3
    rc, why = _check(lib, nat, cfg, vehicle, dims)
    assert rc == -1 and "num_social" in why
    assert lib.smx_check_social_history_dims(None, None, None, None, 0) == -1


def test_the_plan_picks_the_sized_kernels_and_nothing_else(tmp_path):
    """TickPlan::sized follows PlanInputs::dims_bound in every form, and no other field of the plan moves with it."""
    lib_path = str(tmp_path / "libhost_plan_dims.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_plan_dims.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_dims.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    for total, strategy, junctions, is_step, auto_reset in itertools.product((64, 32768, 131072), range(5), (0, 1), (0, 1), (0, 1)):
        for bound in (0, 1):
            same = C.c_int(0)
            sized = lib.host_plan_dims((C.c_int * 7)(total // 32, 32, strategy, junctions, bound, is_step, auto_reset), C.byref(same))
            assert sized == bound and same.value == 1, (total, strategy, junctions, is_step, auto_reset, bound)

"""Per-agent vehicle dimensions without a device (include/smx.h smx_set_agent_dims / smx_check_agent_dims).

tests/native/host_agent_dims.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over the
shim hip_runtime.h and the HIP memory stand-in shim/hip_memory.h — drives the check over every refusal, the handle's bind /
unbind / drop rules with every HIP call failing in turn, and the launch plan with ``agent_dims_bound``.  The rest is the
entry point on the built library and the declarations."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "smarts_amd", "csrc")


def test_agent_dims_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_agent_dims")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", CSRC,
           os.path.join(NATIVE, "host_agent_dims.cpp"), "-o", exe]
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
    assert res["sweep_points"] == res["hip_calls"] > 60 and res["skipped"] == 0, res
    assert res["refused"] + res["release_points"] == res["sweep_points"] and res["refused"] > 40, res
    assert res["mallocs"] == res["frees"] and res["steps"] >= 20 and res["checks"] > 5000, res


def test_header_declares_the_entry_points_and_keeps_every_struct():
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_agent_dims(smx_handle h, const smx_agent_dims* dims);" in header
    assert "int smx_check_agent_dims(const smx_config* cfg, const smx_agent_dims* dims, char* err, uint64_t err_len);" in header
    from smarts_amd import _native as nat

    assert "smx_set_agent_dims" in nat.EXPORTS and "smx_check_agent_dims" in nat.EXPORTS
    assert C.sizeof(nat.SmxAgentDims) == 16
    assert C.sizeof(nat.SmxSocialDims) == 16 and C.sizeof(nat.SmxSocialHistory) == 64  # the neighbours keep their layout
    lib = nat.load_library()
    assert lib.smx_struct_size(0) == C.sizeof(nat.SmxConfig)  # smx_config as the library was built with


def _check(lib, nat, space, dims, num_social=2, rows=None):
    cfg = nat.SmxConfig()
    cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.dt = dims.shape[1], dims.shape[2] + num_social, num_social, 0.1
    cfg.action_space = nat.ACTION_SPACES[space]
    ad = nat.SmxAgentDims()
    ad.dims_host, ad.rows = dims.ctypes.data, dims.shape[0] if rows is None else rows
    err = C.create_string_buffer(512)
    return lib.smx_check_agent_dims(C.byref(cfg), C.byref(ad), err, len(err)), err.value.decode()


def test_smx_check_agent_dims_needs_no_device():
    from smarts_amd import _native as nat
    from smarts_amd.engine import check_agent_dims

    lib = nat.load_library()
    dims = np.tile(np.array([10.0, 2.5, 4.0]), (2, 3, 2, 1))
    dims[1, 2, 1] = np.nan
    for space in ("TargetPose", "TrajectoryWithTime", "Imitation"):
        assert _check(lib, nat, space, dims) == (0, ""), space
    for space in ("Lane", "Continuous", "ActuatorDynamic", "LaneWithContinuousSpeed", "Trajectory", "MPC"):
        rc, why = _check(lib, nat, space, dims)
        assert rc == -1 and "kinematic" in why, (space, why)
    assert _check(lib, nat, "Imitation", dims, rows=0)[0] == -1
    for word, cap, name in ((0, 10.0, "length"), (1, 25.0, "width"), (2, 10.0, "height")):
        edge = dims.copy()
        edge[1, 2, 0, word] = cap
        assert _check(lib, nat, "Imitation", edge)[0] == 0, name
        for bad in (np.nextafter(cap, 100.0), 0.0, -1.0, np.inf):
            edge[1, 2, 0, word] = bad
            rc, why = _check(lib, nat, "Imitation", edge)
            assert rc == -1 and "triple 10" in why and name in why, (name, bad, why)
        edge[1, 2, 0, word] = np.nan
        rc, why = _check(lib, nat, "Imitation", edge)
        assert rc == -1 and "partly NaN" in why, why
    assert lib.smx_check_agent_dims(None, None, None, 0) == -1
    # engine.check_agent_dims: the same through the Python layer
    check_agent_dims("Imitation", 3, 4, 2, dims)
    with pytest.raises(ValueError, match="kinematic"):
        check_agent_dims("Lane", 3, 4, 2, dims)
    with pytest.raises(ValueError, match="shape"):
        check_agent_dims("Imitation", 3, 5, 2, dims)
    zero = dims.copy()
    zero[0, 0, 0, 1] = 0.0
    with pytest.raises(ValueError, match="width"):
        check_agent_dims("Imitation", 3, 4, 2, zero)

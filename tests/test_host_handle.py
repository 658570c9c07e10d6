"""The handle of the C-ABI and what it owns, on the host (smarts_amd/csrc/smx_handle.h).

tests/native/host_handle.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over the
shim hip_runtime.h and the HIP memory stand-in shim/hip_memory.h — creates a handle, loads the hand-written map twice,
binds and rebinds everything, and checks the drop rule after each call; then it runs the same sequence once for every
HIP call of that clean run with that call failing."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "smarts_amd", "csrc")


def test_handle_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_handle")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", CSRC,
           os.path.join(NATIVE, "host_handle.cpp"), "-o", exe]
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
    # one sweep point for every HIP call of the clean run, none skipped: each either made its ABI call return
    # SMX_ERR_HIP or was a release whose result the library ignores by design
    assert res["sweep_points"] == res["hip_calls"] > 150 and res["skipped"] == 0, res
    assert res["refused"] + res["release_points"] == res["sweep_points"] and res["refused"] > 100, res
    # the clean run went through every kind of call the header makes
    for kind in ("mallocs", "memcpys", "memsets", "frees", "stream_creates"):
        assert res[kind] >= 1, (kind, res)
    assert res["mallocs"] == res["frees"] and res["stream_creates"] == 3, res
    assert res["steps"] >= 30 and res["checks"] > 100000, res


def test_the_handle_header_launches_nothing():
    """smx_handle.h holds no kernel, no launch and no __device__, and makes only memory, stream and event calls."""
    src = open(os.path.join(CSRC, "smx_handle.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("__device__", "__global__", "__host__", "hipLaunchKernelGGL", "<<<", "hipMemcpyAsync", "hipMemsetAsync", "hipGetLastError"):
        assert word not in code, word
    allowed = {"hipSetDevice", "hipDeviceSynchronize", "hipMalloc", "hipFree", "hipMemcpy", "hipMemset", "hipMemcpyHostToDevice",
               "hipGetErrorString", "hipSuccess", "hipError_t", "hipStream_t", "hipEvent_t", "hipDeviceGetStreamPriorityRange",
               "hipStreamCreateWithPriority", "hipStreamNonBlocking", "hipStreamSynchronize", "hipStreamDestroy",
               "hipEventCreateWithFlags", "hipEventDisableTiming", "hipEventDestroy"}
    assert set(re.findall(r"\bhip[A-Z]\w+", code)) <= allowed, set(re.findall(r"\bhip[A-Z]\w+", code)) - allowed
    kernels = open(os.path.join(CSRC, "smx_kernels.hip")).read()
    assert '#include "smx_handle.h"' in kernels
    # ownership is the header's alone: the kernels' file and every other header allocate and free nothing
    others = sorted(f for f in os.listdir(CSRC) if f != "smx_handle.h")
    assert "smx_kernels.hip" in others and "smx_tick.h" in others
    for name in others:
        assert not re.search(r"\bhip(Malloc|Free)\s*\(", re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())), name

"""The device-free half of the C-ABI on the host (smarts_amd/csrc/smx_host.h).

tests/native/host_abi.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over the shim
hip_runtime.h — drives the caller-buffer table (the frame stacks' row sizes against the entry check's extents, the entry
check over heap buffers of exactly the needed size), the frame-stack launch geometry, config_error at the ends of int32,
map_tables_error and the table list on a hand-written map, and the route tables of smx_set_missions."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def test_host_abi_header_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_abi")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_abi.cpp"), "-o", exe]
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
    assert res["configs"] == 4 and res["checks"] > 500, res
    # stackable rows whose sensor is on, over the four configurations of the sweep; int32 extremes that were refused
    assert res["stack_sources_on"] > 80 and res["extremes_refused"] > 20, res


def test_the_header_is_host_only():
    """smx_host.h includes include/smx.h, smx_guard.h and the standard library, and holds no HIP."""
    import re

    src = open(os.path.join(ROOT, "smarts_amd", "csrc", "smx_host.h")).read()
    includes = re.findall(r'#include\s+([<"][^>"]+[>"])', src)
    assert {i for i in includes if i.startswith('"')} == {'"../../include/smx.h"', '"smx_guard.h"'}
    assert not [i for i in includes if "hip" in i]
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("__device__", "__global__", "__host__", "hipMalloc", "hipMemcpy", "hipLaunchKernelGGL", "hipStream_t"):
        assert word not in code, word
    assert '#include "smx_host.h"' in open(os.path.join(ROOT, "smarts_amd", "csrc", "smx_kernels.hip")).read()

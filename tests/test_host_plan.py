"""The tick's launch plan (smarts_amd/csrc/smx_plan.h: tick_plan), host-compiled under AddressSanitizer + UBSan behind one
C entry point (tests/native/host_plan.cpp) and asked, in a child process (tests/native/run_host_plan.py), for every
configuration of the grid

    strategy {auto, small, large, large_one_lane, large_teams} x vehicles on both sides of every threshold x map with /
    without splits x routed or not x wp_paths {8, 9} x waypoints / OGM (three tile sizes) / lidar on or off x timing
    level {0, 2} x step or reset x device blobs present or not x side streams ready or not x IDM social traffic or not.

Checked for every plan: the boundaries as the library had them before the plan existed (AUTO is SMALL up to and
including 16 384 vehicles; one-lane seeds from 114 688 on, or forced; eight-lane team halves on split maps up to 65 536;
the facts half released with the grid kernels up to 32 768; the small form's per-env OGM from 8 192 on with at most 32
vehicles an env and tiles that fit; inline OGM only in the small form up to 16 KiB), the coupling invariants (seed_pending
reaches the seeds kernel <=> the walk / emit kernels <=> exactly one slow chain is scheduled; one-lane seeds never with
routed missions, past 8 rows or without their blobs; nothing on a side stream at timing level 2, in the small form or
without side streams; a reset call plans no control, alive list or fork; k_tail never builds the next list under IDM social
traffic) and the form smx_launch_form reports."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def test_launch_plan_boundaries_and_couplings(tmp_path):
    sys.path.insert(0, ROOT)
    from smarts_amd import _native as nat

    lib = str(tmp_path / "libhost_plan.so")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "smarts_amd", "csrc"), os.path.join(NATIVE, "host_plan.cpp"), "-o", lib]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan):
        pytest.skip("no libasan in this toolchain")
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    sensors = [str(nat.SENSOR_WAYPOINTS), str(nat.SENSOR_OGM), str(nat.SENSOR_LIDAR)]
    proc = subprocess.run([sys.executable, os.path.join(NATIVE, "run_host_plan.py"), lib, *sensors],
                          capture_output=True, text=True, env=env, timeout=900)
    assert proc.returncode == 0 and "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, proc.stderr[-3000:]
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    assert res["checked"] > 100000, res["checked"]
    assert res["failures"] == [], res["failures"][:5]

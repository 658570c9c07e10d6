"""Bubbles over a replayed history, on the host: the rule's header (smarts_amd/csrc/smx_bubbles.h), the validation behind
smx_set_history_bubbles (smx_host.h), the handle's bind / drop / refuse paths (smx_handle.h) and the launch plan's choice of
KINEMATIC_BUBBLES (smx_plan.h).

tests/native/host_history_bubbles.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over
the shim hip_runtime.h and the HIP memory stand-in — drives the first three: the rule in a serial loop over every case of
tests/golden/bubble_cursors.npz (handed over as a text file), the refusals one by one, and the handle with every HIP call
failing in turn.  Nothing is loaded into Python under a sanitizer."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "smarts_amd", "csrc")
KINEMATIC, KINEMATIC_FOLLOW, KINEMATIC_HANDOVER, KINEMATIC_BUBBLES = 6, 7, 8, 9  # smx_plan.h: enum class Control


def _fixture_as_text(path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "bubble_cursors.npz"))
    names = [str(n) for n in g["names"]]
    ticks = 0
    with open(path, "w") as f:
        f.write(f"{len(names)}\n")
        for name in names:
            pos = g[f"{name}/pos"]
            T, A = pos.shape[:2]
            nb = g[f"{name}/bubbles"].shape[0]
            f.write(f"{name} {A} {nb} {T}\n")
            for row in g[f"{name}/bubbles"]:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
            for t in range(T):
                f.write(" ".join(repr(float(v)) for v in pos[t].ravel()) + "\n")
                f.write(" ".join(repr(float(v)) for v in g[f"{name}/heading"][t]) + "\n")
                for key in ("alive", "ego", "state", "mask", "transitions", "cursors"):
                    f.write(" ".join(str(int(v)) for v in g[f"{name}/{key}"][t].ravel()) + "\n")
            ticks += T
    return len(names), ticks


def test_bubble_headers_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_history_bubbles")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", CSRC, "-I", NATIVE,
           os.path.join(NATIVE, "host_history_bubbles.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    fixture = str(tmp_path / "bubble_cursors.txt")
    cases, ticks = _fixture_as_text(fixture)
    # the environment is inherited as it is; the sanitizer runtime is linked into the program itself, so its check of
    # the library order (which a preload of the caller's would trip) has nothing to protect here
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe, fixture], capture_output=True, text=True, env=env, timeout=120)
    assert proc.returncode == 0 and "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, \
        (proc.stdout[-3000:], proc.stderr[-3000:])
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    print(res)
    assert res["cases"] == cases >= 16 and res["ticks"] == ticks > 900 and res["checks"] > 20000, res
    # one sweep point for every HIP call of the clean run, none skipped
    assert res["sweep_points"] == res["hip_calls"] > 60 and res["skipped"] == 0, res
    assert res["refused"] + res["release_points"] == res["sweep_points"] and res["refused"] > 40, res


def test_the_rule_is_one_header_without_hip():
    src = open(os.path.join(CSRC, "smx_bubbles.h")).read()
    assert "hip_runtime" not in src and "SMX_BUBBLES_FN" in src
    for fn in ("bubble_zone", "bubble_admissible", "bubble_transition", "bubble_cursor", "bubble_apply", "bubble_recurrence"):
        assert f"SMX_BUBBLES_FN" in src and f" {fn}(" in src, fn
    kernels = open(os.path.join(CSRC, "smx_kernels.hip")).read()
    assert '#include "smx_bubbles.h"' in kernels and "k_bubbles" in kernels
    # the bubbles are the kernel's own argument: the block every kernel gets does not know them
    tick = open(os.path.join(CSRC, "smx_tick.h")).read()
    assert "BubbleSet" not in tick and "bubble_state" not in tick
    # the drop rule is written once, in the handle's unbind_* functions
    handle = open(os.path.join(CSRC, "smx_handle.h")).read()
    assert handle.count("static void unbind_bubbles(") == 1 and "unbind_bubbles(h);   // (the bubbles' rows" in handle


def test_the_plan_picks_the_bubbles_form_only_when_bubbles_are_bound(tmp_path):
    """With bubbles bound, smx_step_history_handover's Control::KINEMATIC_HANDOVER becomes KINEMATIC_BUBBLES in both launch
    forms, with and without the guard; every other entry keeps its controller, and no other field of the plan moves."""
    lib_path = str(tmp_path / "libhost_plan_history_bubbles.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", CSRC,
           os.path.join(NATIVE, "host_plan_history_bubbles.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_history_bubbles.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    imitation = 8
    seen = set()
    for total, strategy, junctions, auto_reset, guard, bound in itertools.product((64, 32768, 131072), range(5), (0, 1), (0, 1), (0, 1), (0, 1)):
        want = {0: KINEMATIC, 1: KINEMATIC_FOLLOW, 2: KINEMATIC_BUBBLES if bound else KINEMATIC_HANDOVER}
        for entry in (0, 1, 2):
            same = C.c_int(0)
            control = lib.host_plan_history_bubbles((C.c_int * 10)(total // 32, 32, strategy, junctions, entry, 1, auto_reset, guard, imitation, bound),
                                                    C.byref(same))
            assert control == want[entry] and same.value == 1, (total, strategy, junctions, auto_reset, guard, bound, entry, control)
            seen.add(control)
    assert seen == {KINEMATIC, KINEMATIC_FOLLOW, KINEMATIC_HANDOVER, KINEMATIC_BUBBLES}
    for bound in (0, 1):  # a reset call launches no controller; a space that is not kinematic keeps its own
        same = C.c_int(0)
        assert lib.host_plan_history_bubbles((C.c_int * 10)(4, 32, 0, 0, 2, 0, 0, 0, imitation, bound), C.byref(same)) == 0 and same.value == 1
        lane = lib.host_plan_history_bubbles((C.c_int * 10)(4, 32, 0, 0, 0, 1, 0, 0, 0, 0), C.byref(same))
        assert lib.host_plan_history_bubbles((C.c_int * 10)(4, 32, 0, 0, 2, 1, 0, 0, 0, bound), C.byref(same)) == lane and same.value == 1

"""The launch plan and a bound traffic history (smarts_amd/csrc/smx_plan.h, PlanInputs::history_bound), on the host.

With a history bound the reset pass's commit still changes SMX_F_ALIVE of a restarted env's social slots, behind k_tail:
k_tail then never builds the next tick's alive list (smx_set_social_history drops a list that was carried, so the tick
builds its own with k_alive_list).  Nothing else of the plan changes, and without a history the plan is what it was."""
import ctypes as C
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_leaves_the_alive_list_to_the_tick_while_a_history_is_bound(tmp_path):
    lib_path = str(tmp_path / "libhost_plan_history.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "host_plan_history.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_history.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    built = 0
    for total, strategy, junctions, is_step, auto_reset in itertools.product((64, 32768, 131072), range(5), (0, 1), (0, 1), (0, 1)):
        def plan(history, carried=0):
            same = C.c_int(0)
            bits = lib.host_plan_history((C.c_int * 8)(total // 32, 32, strategy, junctions, history, is_step, auto_reset, carried), C.byref(same))
            return bits, same.value

        where = (total, strategy, junctions, is_step, auto_reset)
        (off, same_off), (on, same_on) = plan(0), plan(1)
        assert same_off == 1 and same_on == 1, where  # nothing but tail_builds_list moves
        assert not on & 1, where
        small = bool(off & 8)
        assert bool(off & 1) == (not small), where  # without a history: as before, every large-form pass builds it
        assert on & ~1 == off & ~1, where
        if is_step and not small:
            assert on & 2, where  # no list carried into the tick: k_alive_list heads it
            built += 1
    assert built >= 8

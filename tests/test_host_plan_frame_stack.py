"""The launch plan (smarts_amd/csrc/smx_plan.h) with and without frame stacking, host-compiled: TickPlan.frame_stack is
set only when smx_config.frame_stack is on AND something is bound, and nothing else of the plan moves — with the feature
off (or nothing bound) every value equals what tests/native/host_plan_rgb.cpp reports for the same configuration."""
import ctypes as C
import itertools
import os
import subprocess

from smarts_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_lib(tmp_path, name):
    lib_path = str(tmp_path / f"lib{name}.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", f"{name}.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    fn = getattr(C.CDLL(lib_path), name)
    fn.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    return fn


def test_flag_needs_the_feature_on_and_a_binding_and_nothing_else_moves(tmp_path):
    plan_rgb, plan_fs = _host_lib(tmp_path, "host_plan_rgb"), _host_lib(tmp_path, "host_plan_frame_stack")
    out = (C.c_longlong * 64)()

    def run(fn, values):
        arg = (C.c_int * len(values))(*values)
        return list(out[:fn(arg, out)])

    W, H = 48, 32
    base = nat.SENSOR_WAYPOINTS | nat.SENSOR_NEIGHBORS
    forms = {"small": (1, 0, 0), "large_teams": (4, 1, 1), "large_one_lane": (3, 0, 2)}
    checked = 0
    for (form, (strategy, junctions, want_form)), is_step, auto_reset, (envs, nv), other in itertools.product(
            forms.items(), (0, 1), (0, 1), [(3, 8), (513, 32)], (0, nat.SENSOR_RGB, nat.SENSOR_OGM | nat.SENSOR_EGO_CENTRIC)):
        sensors = base | other
        ogm = bool(other & nat.SENSOR_OGM)
        head = [envs, nv, strategy, junctions, 0, sensors, 4, 32 if ogm else 0, 16 if ogm else 0, 0, is_step, 31, 1, 0, 0, 0,
                auto_reset, W, H]
        where = (form, is_step, auto_reset, envs, nv, other)
        parent = run(plan_rgb, head)
        assert parent[0] == want_form, where
        for k, bound in itertools.product((0, 2, 3, 8), (0, 1)):
            got = run(plan_fs, head + [k, bound])
            assert got[:-1] == parent, (where, k, bound)  # field for field
            assert got[-1] == (1 if (k and bound) else 0), (where, k, bound)
            checked += 1
    assert checked == 3 * 2 * 2 * 2 * 3 * 8

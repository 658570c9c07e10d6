"""The top-down RGB camera sensor (include/smx.h SMX_SENSOR_RGB) without a GPU: the palette, the ABI additions, the
buffer validation (smx_check_rgb_output needs neither a device nor a handle), the launch plan with and without the bit,
and the observation layers over hand-made host rows.  The device side is tests/test_gpu_rgb.py."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from rgb_ref import PALETTE
from smarts_amd import _native as nat
from smarts_amd.engine import SimConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_palette_is_the_references_colours():
    # colors.py:27, 33, 47 (Red, Silver, DarkGrey) through :58-62 (SceneColors.Agent, SocialVehicle, Road), as bytes
    red, silver, dark_grey = (210 / 255, 30 / 255, 30 / 255), (192 / 255, 192 / 255, 192 / 255), (80 / 255, 80 / 255, 80 / 255)
    want = [(0, 0, 0)] + [tuple(round(255 * c) for c in colour) for colour in (dark_grey, silver, red)]
    assert PALETTE.dtype == np.uint8 and PALETTE.tolist() == [list(w) for w in want]
    assert PALETTE.tolist() == [[0, 0, 0], [80, 80, 80], [192, 192, 192], [210, 30, 30]]


@pytest.fixture(scope="module")
def lib():
    from smarts_amd import build

    if not os.path.exists(build.LIB_PATH):
        build.build()
    return nat.load_library()


def test_abi_additions(lib):
    assert lib.smx_struct_size(0) == C.sizeof(nat.SmxConfig)
    assert [n for n, _ in nat.SmxConfig._fields_][-3:] == ["rgb_width", "rgb_height", "rgb_resolution"]
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "SMX_SENSOR_RGB = 1 << 9" in header and nat.SENSOR_RGB == 1 << 9
    assert "int smx_set_rgb_output(smx_handle h, uint8_t* rgb_dev, uint64_t count);" in header
    assert "int smx_check_rgb_output(const smx_config* cfg, uint64_t count, char* err, uint64_t err_len);" in header
    config = header[header.index("typedef struct smx_config"):header.index("} smx_config;")]
    assert config.rstrip().endswith("double rgb_resolution;")  # appended at the end
    assert "smx_set_rgb_output" in nat.EXPORTS and "smx_check_rgb_output" in nat.EXPORTS
    for name in ("smx_set_rgb_output", "smx_check_rgb_output"):
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert SimConfig().sensors_mask() == nat.SENSOR_WAYPOINTS | nat.SENSOR_ACCELEROMETER  # the default is unchanged
    assert SimConfig(rgb=True).sensors_mask() == SimConfig().sensors_mask() | nat.SENSOR_RGB
    assert (SimConfig().rgb_width, SimConfig().rgb_height, SimConfig().rgb_resolution) == (256, 256, 50 / 256)
    # smx_outputs is closed: the image is not one of its pointers
    assert len(nat.OUTPUT_BUFFERS) == 60 and nat.OUTPUT_BUFFERS[-1] == "ec_rw_heading" and "rgb" not in nat.OUTPUT_BUFFERS
    assert lib.smx_struct_size(4) == C.sizeof(nat.SmxOutputs) == 60 * 8 + 60 * 8 + 64


def _config(E=3, N=8, W=48, H=32, res=50 / 32, on=True):
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.dt = E, N, 0.1
    c.sensors = nat.SENSOR_WAYPOINTS | (nat.SENSOR_RGB if on else 0)
    c.rgb_width, c.rgb_height, c.rgb_resolution = W, H, res
    return c


def _check(lib, c, count):
    err = C.create_string_buffer(512)
    rc = lib.smx_check_rgb_output(C.byref(c), count, err, len(err))
    return rc, err.value.decode()


def test_check_rgb_output(lib):
    need = 3 * 8 * 32 * 48 * 3
    assert _check(lib, _config(), need) == (0, "")
    assert _check(lib, _config(), need + 1)[0] == 0
    rc, why = _check(lib, _config(), need - 1)
    assert rc == -1 and "rgb" in why and str(need) in why
    rc, why = _check(lib, _config(W=50, H=5), 10 ** 9)  # 250 pixels: not a multiple of 16
    assert rc == -1 and "rgb" in why and "multiple of 16" in why
    assert _check(lib, _config(W=256, H=257), 10 ** 12)[0] == -1  # past the LDS a workgroup may have
    assert _check(lib, _config(res=0.0), 10 ** 9)[0] == -1
    assert _check(lib, _config(on=False), 0) == (0, "")  # bit off: nothing is asked of the buffer
    assert _check(lib, _config(W=0, H=0, on=False), 0) == (0, "")
    assert lib.smx_check_rgb_output(None, 0, None, 0) == -1


# ---------------------------------------------------------------------------------------------- the launch plan
TAIL_GRIDS, RESET_PASS = 13, 24  # indices into what host_plan_ego / host_plan_rgb report


def _host_lib(tmp_path, name):
    lib_path = str(tmp_path / f"lib{name}.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", f"{name}.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    fn = getattr(C.CDLL(lib_path), name)
    fn.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    return fn


def test_launch_plan_is_the_parents_without_the_bit_and_gains_the_kernel_with_it(tmp_path):
    plan_ego, plan_rgb = _host_lib(tmp_path, "host_plan_ego"), _host_lib(tmp_path, "host_plan_rgb")
    out = (C.c_longlong * 64)()

    def run(fn, values):
        arg = (C.c_int * len(values))(*values)
        return list(out[:fn(arg, out)])

    W, H = 48, 32
    base = nat.SENSOR_WAYPOINTS | nat.SENSOR_NEIGHBORS
    # strategy x map: small (1), large teams (4, a map whose lanes split), large one-lane (3, a map without)
    forms = {"small": (1, 0, 0), "large_teams": (4, 1, 1), "large_one_lane": (3, 0, 2)}
    checked = 0
    for (form, (strategy, junctions, want_form)), is_step, auto_reset, (envs, nv), other in itertools.product(
            forms.items(), (0, 1), (0, 1), [(3, 8), (513, 32)], (0, nat.SENSOR_OGM, nat.SENSOR_LIDAR, nat.SENSOR_EGO_CENTRIC)):
        sensors = base | other
        head = [envs, nv, strategy, junctions, 0, sensors, 4, 32 if other == nat.SENSOR_OGM else 0,
                16 if other == nat.SENSOR_OGM else 0, 0, is_step, 31, 1, 0, 0, 0]
        off = run(plan_rgb, head + [auto_reset, W, H])
        on = run(plan_rgb, head[:5] + [sensors | nat.SENSOR_RGB] + head[6:] + [auto_reset, W, H])
        where = (form, is_step, auto_reset, envs, nv, other)
        assert off[0] == want_form, where
        assert off[-2:] == [0, 0], where  # no flag, no LDS
        if auto_reset:  # host_plan_ego plans with auto_reset on: the same input, the same values
            assert off[:-2] == run(plan_ego, head), where
        assert on[-2:] == [1, W * H], where
        reset_pass = on[RESET_PASS]
        assert reset_pass == (1 if (not is_step or auto_reset) else 0), where
        assert on[TAIL_GRIDS] == reset_pass, where  # the new vehicles' images come from the tail
        assert off[TAIL_GRIDS] == (reset_pass if other == nat.SENSOR_OGM else 0), where
        moved = [k for k in range(len(off) - 2) if on[k] != off[k]]
        assert moved in ([], [TAIL_GRIDS]), (where, moved)  # nothing else moves
        checked += 1
    assert checked == 3 * 2 * 2 * 2 * 4


# ---------------------------------------------------------------------------------------------- the observation layers
def _rows(E, N, H, W, with_rgb=True, with_dagm=True):
    rng = np.random.default_rng(7)
    rows = {
        "ego_pos": rng.normal(size=(E, N, 3)) * 50, "ego_f32": rng.normal(size=(E, N, nat.EGO_F32_COUNT)).astype(np.float32),
        "ego_lane": np.zeros((E, N, 2), np.int16), "events": np.zeros((E, N, nat.EV_COUNT), np.uint8),
        "dist": np.zeros((E, N)), "collidees": np.zeros((E, N), np.int64),
    }
    if with_dagm:
        rows["dagm"] = rng.integers(0, 2, (E, N, H, W)).astype(np.uint8) * 255
    if with_rgb:
        rows["rgb"] = PALETTE[rng.integers(0, 4, (E, N, H, W))]
    return rows


def test_observation_builder_and_format_obs_carry_the_image():
    from smarts_amd.env.agent_interface import RGB, DrivableAreaGridMap
    from smarts_amd.env.format_obs import FormatObs, std_obs
    from smarts_amd.env.observations import ObservationBuilder, TopDownRGB

    E, N, H, W = 2, 3, 32, 48
    rows = _rows(E, N, H, W)
    grid = dict(width=W, height=H, resolution=50 / 32)
    kw = dict(waypoints=False, neighbors=False, accelerometer=True)
    builder = ObservationBuilder(["lane"], ["road"], [f"a{i}" for i in range(N)], rgb=RGB(**grid),
                                 dagm=DrivableAreaGridMap(**grid), **kw)
    for env, slot in ((0, 0), (1, 2)):
        env_rows = {k: v[env] for k, v in rows.items()}
        obs = builder.build(env_rows, slot, step_count=3, elapsed_sim_time=0.4)
        rgb = obs.top_down_rgb
        assert isinstance(rgb, TopDownRGB) and rgb.data.shape == (H, W, 3) and rgb.data.dtype == np.uint8
        assert np.array_equal(rgb.data, rows["rgb"][env, slot])
        assert rgb.metadata == obs.drivable_area_grid_map.metadata  # the DAGM's: one camera
        assert rgb.metadata.camera_pos == tuple(float(x) for x in rows["ego_pos"][env, slot])
        assert rgb.metadata.camera_heading_in_degrees == float(np.degrees(float(rows["ego_f32"][env, slot, 0])))
        assert (rgb.metadata.width, rgb.metadata.height, rgb.metadata.resolution) == (W, H, 50 / 32)
        std = std_obs(obs)
        assert std.rgb.shape == (H, W, 3) and std.rgb.dtype == np.uint8 and np.array_equal(std.rgb, rows["rgb"][env, slot])
        direct = FormatObs.from_rows(rows, env, slot)
        assert direct.rgb.shape == (H, W, 3) and direct.rgb.dtype == np.uint8
        assert np.array_equal(direct.rgb, rows["rgb"][env, slot]) and np.array_equal(direct.dagm[..., 0], rows["dagm"][env, slot])
        low = builder.build(env_rows, slot, step_count=3, elapsed_sim_time=0.4, low_dimensional=True)
        assert low.top_down_rgb is None and low.drivable_area_grid_map is None
    # the sensor off: None on every layer
    off_rows = _rows(E, N, H, W, with_rgb=False, with_dagm=False)
    off = ObservationBuilder(["lane"], ["road"], [f"a{i}" for i in range(N)], **kw)
    obs = off.build({k: v[0] for k, v in off_rows.items()}, 1, step_count=1, elapsed_sim_time=0.2)
    assert obs.top_down_rgb is None and std_obs(obs).rgb is None
    assert FormatObs.from_rows(off_rows, 0, 1).rgb is None


def test_validate_for_device_still_refuses_rgb():
    from smarts_amd.env.agent_interface import AgentInterface, AgentType

    with pytest.raises(NotImplementedError, match="rgb"):
        AgentInterface.from_type(AgentType.Full).validate_for_device()

"""bench.py on the GPU: a plain run prints the headline line and times exactly --steps ticks; --dump-outputs writes
what the last timed tick returned, the same from run to run; --full adds the roofline and the per-kernel pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--config", "c2", "--envs-per-gpu", "16", "--vehicles", "8", "--steps", "7", "--warmup", "3"]


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def test_plain_run_dumps_the_last_timed_tick(tmp_path):
    import torch

    import bench
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns
    from smarts_amd.map_compiler import compile_map
    from smarts_amd.sumo_map import load_net

    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(*SMALL, "--dump-outputs", str(a))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 7 and line["warmup"] == 3 and line["ms_per_step"] > 0
    assert abs(line["value"] - 16 * 7 / (line["ms_per_step"] * 7e-3)) <= 1e-6 * line["value"]
    assert "roofline" not in line and "cpu_baseline" not in line and "repeats" not in line
    _bench(*SMALL, "--dump-outputs", str(b))
    ga, gb = _load(a), _load(b)
    assert set(ga) == set(gb) and all(x.dtype in (np.float32, np.float64) for x in ga.values())
    assert sum(x.nbytes for x in ga.values()) <= 64 << 20
    for name in ga:
        np.testing.assert_array_equal(ga[name], gb[name], err_msg=name)

    # the same workload driven here: the dump is what BatchedSim.step returned on tick warmup + steps - 1
    preset, scenario, cfg_kw = bench.workload_config("c2", 16, 8)
    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", scenario)))
    spawns = make_spawns(cm, 16, 8, episodes=4, seed=42, first_env=0)
    sim = BatchedSim(cm, SimConfig(**cfg_kw), device="cuda:0", spawns=spawns)
    actions = torch.from_numpy(bench.action_stream(16, 8, 42, 0)).cuda()
    sim.reset()
    for i in range(3 + 7):
        out = sim.step(actions[i % bench.ACTION_CYCLE])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ga["env_index"], np.arange(16))
    for name, t in out.items():
        want = bench._dump_array(name, t).cpu().numpy()
        np.testing.assert_array_equal(ga[name], want, err_msg=name)
    sim.close()


def test_full_run_keeps_the_extra_figures():
    line = _bench(*SMALL, "--full", "--repeats", "2", "--phase-steps", "5", "--no-cpu-baseline")
    assert line["repeats"]["n"] == 2 and line["steps"] == 7
    assert line["roofline"]["avg_kernel_ms"] > 0 and line["roofline"]["kernels"]
    assert line["config"]["alive_fraction"] > 0 and line["cpu_baseline"] is None

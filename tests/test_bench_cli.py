"""bench.py's command line without a GPU: the plain / --full split and the --dump-outputs writer."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(E=6, N=3):
    """A BatchedSim.step-shaped dict on the CPU: env axis first, the learner block [2, E, N]."""
    import torch

    g = torch.Generator().manual_seed(0)
    return {
        "ego_pos": torch.randn((E, N, 3), dtype=torch.float64, generator=g),
        "ego_f32": torch.randn((E, N, 25), dtype=torch.float32, generator=g),
        "ego_lane": torch.randint(-300, 300, (E, N, 2), generator=g).to(torch.int16),
        "wp_lane_index": torch.randint(-1, 4, (E, N, 4, 20), generator=g).to(torch.int8),
        "ogm": torch.randint(0, 256, (E, N, 8, 8), generator=g).to(torch.uint8),
        "via_hit": torch.randint(-2**31, 2**31 - 1, (E, N), generator=g).to(torch.int32),
        "collidees": torch.tensor([[-1, 2**63 - 1, 5]] * E, dtype=torch.int64),
        "env_done": torch.randint(0, 2, (E,), generator=g).to(torch.uint8),
        "learner": torch.randn((2, E, N), dtype=torch.float32, generator=g),
    }


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def test_dump_outputs_writes_every_output_as_an_exact_float_array(tmp_path):
    import bench

    out = _outputs()
    bench.dump_outputs(out, str(tmp_path), 6)
    got = _load(tmp_path)
    assert set(got) == set(out) | {"env_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["env_index"], np.arange(6))
    for name, t in out.items():
        if name == "collidees":
            u = t.numpy().view(np.uint64)
            np.testing.assert_array_equal(got[name][..., 0], (u & 0xFFFFFFFF).astype(np.float64))
            np.testing.assert_array_equal(got[name][..., 1], (u >> 32).astype(np.float64))
        else:
            assert got[name].shape == tuple(t.shape)
            np.testing.assert_array_equal(got[name], t.numpy().astype(got[name].dtype))
            np.testing.assert_array_equal(got[name].astype(t.numpy().dtype), t.numpy())  # no rounding


def test_dump_outputs_samples_the_same_envs_within_the_budget(tmp_path, monkeypatch):
    import bench

    E = 200
    out = _outputs(E=E)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 150_000)
    a, b = tmp_path / "a", tmp_path / "b"
    written = bench.dump_outputs(out, str(a), E)
    bench.dump_outputs(out, str(b), E)
    assert written <= 150_000
    ga, gb = _load(a), _load(b)
    envs = ga["env_index"].astype(int)
    assert 0 < len(envs) < E and len(set(envs)) == len(envs) and np.all(np.diff(envs) > 0)
    for name in ga:
        np.testing.assert_array_equal(ga[name], gb[name])
    np.testing.assert_array_equal(ga["ego_pos"], out["ego_pos"].numpy()[envs])
    np.testing.assert_array_equal(ga["learner"], out["learner"].numpy()[:, envs])
    assert sum(x.nbytes for x in ga.values()) == written


@pytest.mark.parametrize("flag", [["--repeats", "2"], ["--phase-steps", "10"]])
def test_full_run_options_need_full(flag):
    """--repeats and --phase-steps shape the --full run only: a plain run times exactly --steps ticks."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", *flag],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--full" in out.stderr

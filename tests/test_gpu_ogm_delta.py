"""OGM delta stores on the device: a call stores only the pieces of a tile that are non-zero now or were after the last
call (KernelArgs::ogm_mask in smarts_amd/csrc/smx_tick.h), and the rows read exactly as if whole tiles had been
stored.  Every kernel form that writes tiles, at the shapes tests/test_gpu_large_form_features.py::test_ogm_kernel_forms
draws them at:

    k_ogm_env<1>     loop 2 x 16 with 128 x 96 (large_teams), minicity 1 x 64 with 64 x 64 (more than 32 vehicles an env)
    k_ogm_env<2>     loop 2 x 16 with 96 x 32 (large_one_lane)
    k_ogm            loop 1 x 8 with 256 x 256 (64 KiB tiles: one per workgroup)
    inside k_sensors loop 4 x 8 with 64 x 64 (small)

Seeds and actions are chosen so that the CPU oracle shows, within 14 ticks, an agent that ends while its env runs on
(half of the fleet slows down: not_moving and rear-end collisions) and every agent ending at max_episode_steps (the env
restarts)."""
import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

FORMS = {
    "env1_teams": ("loop", 2, 16, 184, (128, 96, 50 / 128), "large_teams"),
    "env1_minicity": ("minicity", 1, 64, 181, (64, 64, 50 / 64), "large_teams"),
    "env2": ("loop", 2, 16, 183, (96, 32, 0.5), "large_one_lane"),
    "per_observer": ("loop", 1, 8, 188, (256, 256, 50 / 256), "large_one_lane"),
    "in_sensors": ("loop", 4, 8, 186, (64, 64, 50 / 64), "small"),
}
ENDINGS = dict(done_not_moving=True, not_moving_time=0.5, not_moving_distance=2.5, done_collision=True, auto_reset=True,
               max_episode_steps=14)
TICKS = 30


def _pair(form, nets, compiled_maps, count=2):
    name, E, N, seed, (w, h, res), strategy = FORMS[form]
    sims = []
    for _ in range(count):
        sim, _, _ = parity.make(name, E, N, nets, compiled_maps, seed, launch_strategy=strategy, ogm=True, ogm_width=w,
                                ogm_height=h, ogm_resolution=res, **ENDINGS)
        assert sim.launch_form() == strategy
        sims.append(sim)
    return sims, E, N, seed


def _actions(rng, E, N):
    import torch

    acts = parity.lane_actions(rng, E, N)
    acts[:, ::2] = 1  # slow_down: half of the fleet
    return torch.from_numpy(acts).cuda()


def _same(on, off, where):
    """Every output row, the state rows and the flags of the two sims, byte for byte."""
    import torch

    torch.cuda.synchronize()
    assert set(on.out) == set(off.out)
    for k in on.out:
        a, b = on.out[k].contiguous().view(torch.uint8), off.out[k].contiguous().view(torch.uint8)
        assert torch.equal(a, b), f"{where}: {k} differs in {int((a != b).sum())} bytes"
    assert torch.equal(on.state.contiguous().view(torch.uint8), off.state.contiguous().view(torch.uint8)), f"{where}: state"
    assert torch.equal(on.flags, off.flags), f"{where}: flags"


@pytest.mark.parametrize("form", sorted(FORMS))
def test_delta_on_equals_delta_off(form, nets, compiled_maps):
    """Two sims of one build on the same spawns and actions, one storing whole tiles (set_ogm_delta(False)): equal after
    the reset and after each of 30 ticks — through agents that end while their env runs on (the zeroing path), env
    restarts (k_tail's tiles of new vehicles), rows the caller overwrote and said so, rows rebound to another tensor and
    a partial reset in the middle of the run."""
    import torch

    (on, off), E, N, seed = _pair(form, nets, compiled_maps)
    off.set_ogm_delta(False)
    on.reset(), off.reset()
    _same(on, off, "reset")
    rng = np.random.default_rng(seed)
    ended_alone = restarted = 0
    was_active = on.out["active"].cpu().numpy().astype(bool)
    for t in range(TICKS):
        acts = _actions(rng, E, N)
        on.step(acts), off.step(acts)
        _same(on, off, f"t{t}")
        active, env_done = on.out["active"].cpu().numpy().astype(bool), on.out["env_done"].cpu().numpy().astype(bool)
        if t < TICKS - 1 and t != 20:  # (the next tick zeroes the rows of the agents that went; after t20 comes the reset)
            ended_alone += int((was_active & ~active & ~env_done[:, None]).sum())
        restarted += int(env_done.sum())
        was_active = active
        if t == 5:  # the caller writes into the rows and says so
            for sim in (on, off):
                sim.out["ogm"].fill_(0xAB)
            on.invalidate_outputs()
        if t == 9:  # other rows, full of something else: the pointer alone tells
            for sim in (on, off):
                sim.bind_ogm(torch.full_like(sim.out["ogm"], 0xAB))
        if t == 20:
            mask = torch.zeros(E, dtype=torch.uint8)
            mask[0] = 1
            on.reset(mask), off.reset(mask)
            _same(on, off, "partial reset")
            was_active = on.out["active"].cpu().numpy().astype(bool)
    assert ended_alone > 0, "no agent ended while its env ran on"
    assert restarted > 0, "no env restarted"
    on.close(), off.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_stores_really_are_skipped(form, nets, compiled_maps):
    """The contract: with the delta on, rows the caller fills without smx_invalidate_outputs keep that filling wherever a
    tile was and stays zero — some byte of an alive agent's tile still reads 0x55 after the next tick."""
    (sim,), E, N, seed = _pair(form, nets, compiled_maps, count=1)
    sim.reset()
    rng = np.random.default_rng(seed)
    sim.step(_actions(rng, E, N))
    sim.out["ogm"].fill_(0x55)
    d = parity.host(sim.step(_actions(rng, E, N)))
    alive = d["active"].astype(bool)
    assert alive.any()
    tiles = d["ogm"][alive]
    assert (tiles == 0x55).any() and (tiles == 255).any()
    sim.close()

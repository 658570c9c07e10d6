"""The top-down RGB camera sensor on the device (k_rgb; include/smx.h SMX_SENSOR_RGB): SimConfig(rgb=True), out["rgb"].

Images are held byte for byte to tests/rgb_ref.py — the composition of the two oracle rasters the OGM and the DAGM are
already exact against — in both launch forms, on the reset observation, on ticks, and on the tick an env restarts inside
the launch; to the device's own OGM and DAGM of the same tick; and to the reference's own pin (test_observations.py:
133-233) restated over device rows.  Batches are 3 envs x 8 vehicles, 3 of them social, on a 48 x 32 grid at 50 / 32
metres a pixel: not square, so a swapped row / column or width / height cannot pass.
"""
import ctypes as C

import numpy as np
import pytest

from rgb_ref import PALETTE, bodies, rgb_ref
from smarts_amd import _native as nat

pytestmark = pytest.mark.gpu

E, N, SOCIAL = 3, 8, 3
AGENTS = N - SOCIAL
W, H, RES = 48, 32, 50 / 32
GRID = dict(rgb=True, rgb_width=W, rgb_height=H, rgb_resolution=RES)
FORMS = ("small", "large")


def _sim(cm, seed, strategy, spawns=None, **kw):
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns

    cfg = SimConfig(num_envs=E, num_vehicles=N, num_social=SOCIAL, launch_strategy=strategy, **kw)
    table, where = make_spawns(cm, E, N, episodes=2, seed=seed, return_lanes=True)
    sim = BatchedSim(cm, cfg, spawns=table if spawns is None else spawns(table), social_spawns=where)
    assert (sim.launch_form() == "small") == (strategy == "small")
    return sim


def _host(sim):
    """(state [S_COUNT, E, N], flags [E, N]) on the host, after everything enqueued has run."""
    import torch

    torch.cuda.synchronize()
    return sim.state.cpu().numpy(), sim.flags.cpu().numpy()


def _keep_lane(sim):
    import torch

    return sim.step(torch.zeros((E, N), dtype=torch.int8, device="cuda"))


def _check_images(images, state, flags, observers, lanes, where):
    """images [E, N, H, W, 3] against rgb_ref for every (env, slot) of `observers`, drawn from the poses of `state` and
    the alive / social bits of `flags`.  Returns the classes seen."""
    seen = set()
    for e in range(E):
        agents, socials, by_slot = bodies(state[:, e], flags[e])
        for j in range(N):
            if not observers[e, j]:
                continue
            want = rgb_ref(by_slot[j], agents, socials, lanes, W, H, RES)
            got = images[e, j]
            assert got.shape == (H, W, 3) and got.dtype == np.uint8
            if not np.array_equal(got, want):
                bad = np.argwhere((got != want).any(-1))
                r, c = bad[0]
                raise AssertionError(f"{where} env {e} slot {j}: {len(bad)} pixels differ, first ({r}, {c}) "
                                     f"device={got[r, c].tolist()} reference={want[r, c].tolist()}")
            seen |= {tuple(p) for p in np.unique(want.reshape(-1, 3), axis=0).tolist()}
    return seen


def _observing(flags):
    return ((flags & nat.F_ALIVE) != 0) & ((flags & nat.F_SOCIAL) == 0)


@pytest.mark.parametrize("strategy", FORMS)
@pytest.mark.parametrize("name,seed", [("loop", 211), ("4lane", 212)])
def test_images_equal_the_composed_oracle_rasters(name, seed, strategy, compiled_maps, oracle_maps):
    """Reset observation and 6 ticks of keep_lane: every alive agent's image, array_equal."""
    sim = _sim(compiled_maps(name), seed, strategy, **GRID)
    lanes = oracle_maps(name).lane_bands()
    out = sim.reset()
    assert tuple(out["rgb"].shape) == (E, N, H, W, 3) and str(out["rgb"].dtype) == "torch.uint8"
    state, flags = _host(sim)
    assert _observing(flags).sum() == E * AGENTS and out["active"].cpu().numpy()[:, AGENTS:].sum() == 0
    seen = _check_images(out["rgb"].cpu().numpy(), state, flags, _observing(flags), lanes, f"{name} {strategy} reset")
    assert (out["rgb"].cpu().numpy()[:, AGENTS:] == 0).all()  # social slots observe nothing
    for t in range(6):
        _, before = _host(sim)  # the tick draws the vehicles alive at its start, at the poses it moves them to
        out = _keep_lane(sim)
        state, _ = _host(sim)
        seen |= _check_images(out["rgb"].cpu().numpy(), state, before, _observing(before), lanes, f"{name} {strategy} t{t}")
    assert seen == {tuple(p) for p in PALETTE.tolist()}  # every class was in view somewhere
    sim.close()


@pytest.mark.parametrize("strategy", FORMS)
def test_image_agrees_with_the_ogm_and_the_dagm_of_the_same_tick(strategy, compiled_maps):
    """The three grids on together at one grid: a pose read at another point of the tick would show."""
    kw = dict(ogm=True, ogm_width=W, ogm_height=H, ogm_resolution=RES, dagm=True, dagm_width=W, dagm_height=H,
              dagm_resolution=RES, **GRID)
    sim = _sim(compiled_maps("4lane"), 213, strategy, **kw)
    out = sim.reset()
    reds = silvers = 0
    for t in range(5):
        if t:
            out = _keep_lane(sim)
        live = out["active"].bool() | out["done"].bool()  # an observation in this pass
        assert int(live.sum()) > 0
        rgb, ogm, dagm = out["rgb"][live], out["ogm"][live], out["dagm"][live]
        assert bool((((rgb != 0).any(-1)) == ((ogm == 255) | (dagm == 255))).all()), t
        red = (rgb[..., 0] == 210) & (rgb[..., 1] == 30) & (rgb[..., 2] == 30)
        silver = (rgb == 192).all(-1)
        assert bool(((ogm == 255) == (red | silver)).all()), t
        reds, silvers = reds + int(red.sum()), silvers + int(silver.sum())
    assert reds > 0 and silvers > 0
    sim.close()


@pytest.mark.parametrize("strategy", FORMS)
def test_restart_inside_the_launch_draws_the_next_episodes_first_image(strategy, compiled_maps, oracle_maps):
    sim = _sim(compiled_maps("loop"), 214, strategy, auto_reset=True, max_episode_steps=3, **GRID)
    lanes = oracle_maps("loop").lane_bands()
    sim.reset()
    for t in range(4):  # (the reset observation may count as the episode's first step)
        before, _ = _host(sim)
        out = _keep_lane(sim)
        if out["env_done"].cpu().numpy().any():
            break
    assert t >= 1 and out["env_done"].cpu().numpy().tolist() == [1] * E  # every env finished on this tick and restarted
    state, flags = _host(sim)
    S = nat.S
    spawn = sim.spawns.cpu().numpy()[1].reshape(E, N, 4)  # the second episode's rows
    assert np.array_equal(state[S["X"], :, :AGENTS], spawn[:, :AGENTS, 0])
    assert np.array_equal(state[S["Y"], :, :AGENTS], spawn[:, :AGENTS, 1])
    assert not np.array_equal(state[S["X"]], before[S["X"]])
    pos = out["ego_pos"].cpu().numpy()
    assert np.array_equal(pos[:, :AGENTS, 0], state[S["X"], :, :AGENTS])  # the low-dimensional rows' first observation
    assert np.array_equal(pos[:, :AGENTS, 1], state[S["Y"], :, :AGENTS])
    assert _observing(flags).sum() == E * AGENTS
    _check_images(out["rgb"].cpu().numpy(), state, flags, _observing(flags), lanes, f"restart {strategy}")
    sim.close()


@pytest.mark.parametrize("strategy", FORMS)
def test_rows_without_an_observation_are_not_written(strategy, compiled_maps):
    """Two agents of env 0 start inside each other and are done on the first tick: from the next tick on their images
    keep whatever the buffer held (a fill pattern), like the social slots' from the start; everybody else's image is
    written whole."""
    def collide(table):
        table = table.copy()
        table[:, 1] = table[:, 0]  # env 0: slot 1 on top of slot 0
        return table

    sim = _sim(compiled_maps("loop"), 215, strategy, spawns=collide, **GRID)

    def check(out):
        active, images = out["active"].cpu().numpy().astype(bool), out["rgb"].cpu().numpy()
        assert (images[~active] == 0x5A).all()
        assert active.any() and not (images[active] == 0x5A).any()  # (0x5A is no palette byte)
        return active

    sim.out["rgb"].fill_(0x5A)
    active = check(sim.reset())
    assert active[:, :AGENTS].all() and not active[:, AGENTS:].any()
    out = _keep_lane(sim)  # the collision: both agents get their last observation and are done
    done = out["done"].cpu().numpy().astype(bool)
    assert done[0, 0] and done[0, 1]
    sim.out["rgb"].fill_(0x5A)
    active = check(_keep_lane(sim))
    assert not active[0, 0] and not active[0, 1] and active[1:, :AGENTS].any()
    sim.close()


def test_the_references_own_pin_over_device_rows(compiled_maps):
    """smarts/core/tests/test_observations.py:133-233 at 64 x 64, 50 / 64 m a pixel: after 30 ticks of keep_lane the ego,
    every neighbour (radius 22 m) and the ends of every road-waypoint path (horizon 10 m) project onto pixels of the
    right kind.  The lens is the reference's OrthographicLens with film size (width, height) * resolution, restated:
    normalised coordinates are the rotated offsets over half the film.  Every point lies inside the image (22 m and
    10 m are below the 25 m half view less 2 px): that is asserted, no point is left out."""
    G = 64
    res = 50 / G
    sim = _sim(compiled_maps("loop"), 216, "small", rgb=True, rgb_width=G, rgb_height=G, rgb_resolution=res,
               neighbors=True, nb_radius=22.0, road_waypoints=True, rw_horizon=10)
    out = sim.reset()
    for _ in range(30):
        out = _keep_lane(sim)
    import torch

    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    road = np.array([80, 80, 80])

    def project_2d(center, heading, pos):
        p = np.asarray(pos, dtype=np.float64) - center
        rot = np.array([p[0] * np.cos(-heading) - p[1] * np.sin(-heading), p[0] * np.sin(-heading) + p[1] * np.cos(-heading)])
        nx, ny = rot[0] / (0.5 * res * G), rot[1] / (0.5 * res * G)  # lens.project(): (-1, 1) over the film
        assert -1.0 < nx < 1.0 and -1.0 < ny < 1.0, ("outside the image", pos)
        return int(-ny * G / 2 + G / 2), int(nx * G / 2 + G / 2)

    vehicles = waypoints = 0
    assert o["active"][:, :AGENTS].any()
    for e, j in zip(*np.nonzero(o["active"])):
        image = o["rgb"][e, j]
        center, heading = o["ego_pos"][e, j], float(o["ego_f32"][e, j, nat.EGO["HEADING"]])
        near = [o["nb_pos"][e, j, k] for k in range(min(int(o["nb_count"][e, j]), o["nb_pos"].shape[2]))]
        for pos in [center] + near:
            x, y = project_2d(center, heading, pos)
            assert 2 <= x <= G - 2 and 2 <= y <= G - 2
            assert np.count_nonzero(image[x, y, :])
            assert np.count_nonzero(image[x - 2:x + 2, y - 2:y + 2, :] != road)
            vehicles += 1
        for l in range(o["rw_lane"].shape[2]):
            if o["rw_lane"][e, j, l] < 0:
                continue
            for p in range(min(int(o["rw_path_count"][e, j, l]), o["rw_count"].shape[3])):
                n = int(o["rw_count"][e, j, l, p])
                for w in ((0, n - 1) if n else ()):  # (a path without waypoints has no ends)
                    x, y = project_2d(center, heading, o["rw_pos"][e, j, l, p, w])
                    assert np.count_nonzero(image[x, y, :]), (e, j, l, p, w)
                    waypoints += 1
    assert vehicles > int(o["active"].sum()) and waypoints > 0  # some neighbour was in range
    sim.close()


def test_entry_errors(compiled_maps):
    import torch

    sim = _sim(compiled_maps("loop"), 217, "small", **GRID)
    images = sim.out["rgb"]
    sim.bind_rgb(None)
    with pytest.raises(nat.SmxError, match=r"\(-3\).*smx_set_rgb_output"):  # SMX_ERR_STATE
        sim.reset()
    rc = sim.lib.smx_set_rgb_output(sim.handle, images.data_ptr(), C.c_uint64(images.numel() - 1))
    assert rc == -1 and b"rgb" in sim.lib.smx_last_error(sim.handle)  # SMX_ERR_INVALID at the bind
    with pytest.raises(nat.SmxError, match=r"\(-3\)"):
        sim.reset()  # the short buffer was not taken
    sim.bind_rgb(images)
    out = sim.reset()
    torch.cuda.synchronize()
    assert out["rgb"] is images and bool((images[:, :AGENTS] != 0).any())
    other = torch.zeros_like(images)  # alternate buffers between ticks
    sim.bind_rgb(other)
    out = _keep_lane(sim)
    torch.cuda.synchronize()
    assert out["rgb"] is other and bool((other[:, :AGENTS] != 0).any())
    sim.close()


def test_a_refused_step_leaves_the_learner_blocks_as_they_were(compiled_maps):
    """A step the library refuses (SMX_ERR_STATE: no image buffer bound) flips nothing: ``out["learner"]`` and
    ``next_learner_block`` stay the tensors they were, and the next step that goes ahead writes the block that was
    named before the refusal."""
    import torch

    sim = _sim(compiled_maps("loop"), 217, "small", **GRID)
    images = sim.out["rgb"]
    sim.reset()
    torch.cuda.synchronize()
    current, coming = sim.out["learner"], sim.next_learner_block
    assert current is not coming and current.data_ptr() != coming.data_ptr()
    sim.bind_rgb(None)
    with pytest.raises(nat.SmxError, match=r"\(-3\).*smx_set_rgb_output"):  # SMX_ERR_STATE
        _keep_lane(sim)
    assert sim.out["learner"] is current and sim.next_learner_block is coming
    sim.bind_rgb(images)
    current.fill_(-7.0)
    coming.fill_(-7.0)
    torch.cuda.synchronize()
    out = _keep_lane(sim)
    torch.cuda.synchronize()
    assert out["learner"] is coming and sim.next_learner_block is current
    # the tick wrote the named block ([2, E, N]) and left the other one alone
    assert bool((coming[..., :AGENTS] != -7.0).any()) and bool((current == -7.0).all())
    sim.close()

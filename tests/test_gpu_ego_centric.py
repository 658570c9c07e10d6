"""SMX_SENSOR_EGO_CENTRIC on the device (k_ego_frame, k_actions_to_world): ``out["ego_frame"]`` / ``out["ec_*"]`` against
``ego_centric_rows`` applied to the device's own dense rows of the same tick, and ``actions_to_world`` against
``actions_to_world_rows``.  Bounds: float64 <= 1e-9 absolute (the project's device-vs-host bound: device sin / cos
differ from libm by ulps), float32 headings <= 1e-6 circular (a value on the +-pi seam may land on either side), the
dyn() columns within 2 float32 ulps, lidar misses NaN on both sides."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import parity
from smarts_amd import _native as nat
from smarts_amd.engine import BatchedSim, SimConfig, make_spawns
from smarts_amd.env.ego_centric_rows import actions_to_world_rows, ego_centric_rows
from smarts_amd.lidar import SensorParams

pytestmark = pytest.mark.gpu

SMALL_LIDAR = SensorParams(start_angle=0.0, end_angle=2 * math.pi, laser_angles=(0.0, 0.05), angle_resolution=2 * math.pi / 12,
                           max_distance=20.0)
E_ = nat.EGO
DYN = [E_[k] + i for k in ("LIN_VEL", "LIN_ACC", "LIN_JERK") for i in range(2)]


def _sim(compiled_maps, name, E, N, seed, ego_centric=True, **kw):
    cm = compiled_maps(name)
    base = dict(neighbors=True, nb_radius=50.0, ego_centric=ego_centric)
    base.update(kw)
    cfg = SimConfig(num_envs=E, num_vehicles=N, **base)
    return BatchedSim(cm, cfg, spawns=make_spawns(cm, E, N, episodes=2, seed=seed)), cfg


def _masks(rows):
    m = {}
    if "wp_pos" in rows:
        P, W = rows["wp_heading"].shape[1:]
        c = rows["wp_count"].astype(np.int64)
        m["wp"] = (np.arange(P)[None, :, None] < c[:, :1, None]) & (np.arange(W)[None, None, :] < c[:, 1:, None])
    if "nb_pos" in rows:
        m["nb"] = np.arange(rows["nb_heading"].shape[1])[None, :] < rows["nb_count"].astype(np.int64)[:, None]
    if "rw_pos" in rows:
        L, Q, R = rows["rw_heading"].shape[1:]
        m["rw"] = ((rows["rw_lane"] >= 0)[:, :, None, None] & (np.arange(Q)[None, None, :, None] < rows["rw_path_count"].astype(np.int64)[:, :, None, None])
                   & (np.arange(R)[None, None, None, :] < rows["rw_count"].astype(np.int64)[..., None]))
    return m


def _compare(rows, where):
    """Device rows of one pass against ego_centric_rows of the same pass's world rows (the device's frame).  Returns
    the masks, for the non-vacuity assertions of the caller."""
    valid = rows["ec_flags"] == 1
    assert np.array_equal(rows["ec_flags"], valid.astype(np.uint8)), where
    assert np.array_equal(rows["ego_frame"][valid, :3], rows["ego_pos"][valid]), where
    assert np.array_equal(rows["ego_frame"][valid, 3].astype(np.float32), rows["ego_f32"][valid, E_["HEADING"]]), where
    want = ego_centric_rows(rows)
    m = _masks(rows)
    for key, mask in (("wp", m.get("wp")), ("nb", m.get("nb")), ("rw", m.get("rw")), ("lidar", None)):
        pos = "ec_lidar_point" if key == "lidar" else f"ec_{key}_pos"
        if pos not in rows:
            continue
        if mask is None:  # every ray of the lidar row is written
            mask = np.ones(rows[pos].shape[:-1], dtype=bool)
        keep = valid.reshape((-1,) + (1,) * (mask.ndim - 1)) & mask
        a, b = rows[pos][keep], want[pos][keep]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (where, pos)
        err = np.nanmax(np.abs(a - b)) if a.size and not np.isnan(a).all() else 0.0
        assert err <= 1e-9, (where, pos, err)
        if key != "lidar":
            hd = f"ec_{key}_heading"
            assert rows[hd].dtype == np.float32
            d = np.abs(rows[hd][keep].astype(np.float64) - want[hd][keep].astype(np.float64))
            d = np.minimum(d, 2 * math.pi - d)
            assert (d.max() if d.size else 0.0) <= 1e-6, (where, hd, d.max())
            assert (np.abs(rows[hd][keep]) <= np.float32(math.pi)).all()
    if "ec_lidar_point" in rows:
        miss = (rows["lidar_hit"] == 0) & valid[:, None]
        assert np.isnan(rows["ec_lidar_point"][miss]).all() and np.isfinite(rows["ec_lidar_point"][(rows["lidar_hit"] != 0) & valid[:, None]]).all()
    f, g = rows["ec_ego_f32"][valid], want["ec_ego_f32"][valid]
    same = np.ones(nat.EGO_F32_COUNT, dtype=bool)
    same[[E_["HEADING"], *DYN]] = False
    assert np.array_equal(f[:, same], rows["ego_f32"][valid][:, same], equal_nan=True), where
    assert not f[:, E_["HEADING"]].any()
    assert (np.abs(f[:, DYN] - g[:, DYN]) <= 2 * np.spacing(np.abs(g[:, DYN]))).all(), where
    return valid, m


@pytest.mark.parametrize("strategy", ["small", "large_one_lane", "large_teams"])
def test_loop_in_every_launch_form(strategy, compiled_maps):
    sim, cfg = _sim(compiled_maps, "loop", 4, 8, 3, launch_strategy=strategy)
    assert sim.launch_form() == strategy
    rows = parity.host(sim.reset())
    keep = torch.zeros((4, 8), dtype=torch.int8, device="cuda")
    points = 0
    for t in range(7):
        valid, m = _compare(rows, f"{strategy} t{t}")
        assert valid.all()  # keep_lane on the loop: nobody leaves
        points += int(m["wp"].sum() + m["nb"].sum())
        rows = parity.host(sim.step(keep))
    assert points > 7 * 32 * 20
    sim.close()


def test_junction_paths_road_waypoints_and_lidar(compiled_maps):
    sim, cfg = _sim(compiled_maps, "4lane", 2, 16, 11, road_waypoints=True, rw_horizon=4, rw_lanes=4, rw_paths=2, lidar=SMALL_LIDAR)
    rng = np.random.default_rng(11)
    rows = parity.host(sim.reset())
    fanned = hits = misses = oncoming = rw_points = 0
    for t in range(5):
        valid, m = _compare(rows, f"4lane t{t}")
        fanned += int((rows["wp_count"][valid, 0] > 1).sum())
        hits += int((rows["lidar_hit"][valid] != 0).sum())
        misses += int((rows["lidar_hit"][valid] == 0).sum())
        d = np.abs(rows["nb_heading"].astype(np.float64) - rows["ego_frame"][:, 3:4])
        oncoming += int((m["nb"] & valid[:, None] & (np.minimum(d, 2 * math.pi - d) > 3.0)).sum())
        rw_points += int((m["rw"] & valid[:, None, None, None]).sum())
        rows = parity.host(sim.step(torch.from_numpy(parity.lane_actions(rng, 2, 16)).cuda()))
    assert fanned >= 1 and hits >= 1 and misses >= 1 and oncoming >= 1 and rw_points >= 100, (fanned, hits, misses, oncoming, rw_points)
    sim.close()


def test_first_observation_after_reset_under_auto_reset(compiled_maps):
    sim, cfg = _sim(compiled_maps, "loop", 2, 4, 5, auto_reset=True, max_episode_steps=3)
    keep = torch.zeros((2, 4), dtype=torch.int8, device="cuda")
    _compare(parity.host(sim.reset()), "reset")
    spawn1 = sim.spawns[1, :, :2].cpu().numpy()
    restarts = 0
    for t in range(5):
        out = sim.step(keep)
        rows = parity.host(out)
        valid, _ = _compare(rows, f"auto_reset t{t}")
        for e in np.flatnonzero(out["env_done"].cpu().numpy() != 0):
            mine = slice(e * 4, (e + 1) * 4)
            assert valid[mine].all() and rows["active"][mine].all(), (t, e)
            if restarts < 2:  # the first restart starts episode 1: the frame is its spawn pose
                assert np.abs(rows["ego_frame"][mine, :2] - spawn1[mine]).max() < 3.0, (t, e)
            restarts += 1
    assert restarts >= 2, restarts
    sim.close()


def test_agents_without_an_observation_keep_their_rows(compiled_maps):
    sim, cfg = _sim(compiled_maps, "loop", 2, 4, 5, max_episode_steps=2)
    keep = torch.zeros((2, 4), dtype=torch.int8, device="cuda")
    sim.reset()
    for t in range(6):
        out = sim.step(keep)
        if not bool(out["active"].any()):
            break
    assert not bool(out["active"].any())  # every agent reached max_episode_steps and is gone
    names = [k for k in out if k.startswith("ec_") and k != "ec_flags"] + ["ego_frame"]
    for k in names:
        out[k].fill_(-7)
    rows = parity.host(sim.step(keep))
    assert not rows["ec_flags"].any()
    for k in names:
        assert (rows[k] == -7).all(), k
    sim.close()


def test_phase_timing_changes_no_bit(compiled_maps):
    sims = [_sim(compiled_maps, "loop", 2, 8, 3)[0] for _ in range(2)]
    sims[1].set_timing(2)
    keep = torch.zeros((2, 8), dtype=torch.int8, device="cuda")
    got = []
    for sim in sims:
        sim.reset()
        sim.step(keep)
        got.append(parity.host(sim.step(keep)))
    assert sims[1].read_phase_ms().shape == (2, len(nat.PHASES))
    for k in ["ego_frame"] + [k for k in got[0] if k.startswith("ec_")]:
        assert np.array_equal(got[0][k], got[1][k], equal_nan=True), k
    _compare(got[1], "timing 2")
    for sim in sims:
        sim.close()


def _ego_frame_actions(space, E, N, tick):
    """Drive straight ahead (+y of the ego frame), slightly to the left; agent 1 of every env sends no action."""
    T = E * N
    if space == "TargetPose":
        a = np.tile(np.array([0.3, 1.5 + 0.1 * tick, 0.02, 0.1]), (T, 1))
        a[1::N, 0] = np.nan
        return a, None
    if space == "Trajectory":
        n = 12
        ys = 1.5 * np.arange(1, n + 1)
        full = np.stack([0.02 * ys, ys, np.full(n, 0.01), np.full(n, 10.0)])
        a = np.tile(np.concatenate([full[:, :10], full[:, -1:]], axis=1), (T, 1, 1))
        counts = np.full(T, n, np.int32)
        counts[2::N] = 3  # a short trajectory: columns 3..9 are not converted
    else:
        M = 4
        t = 0.1 * np.arange(M)
        a = np.tile(np.stack([t, 0.1 * t, 10.0 * t, np.full(M, 0.01), np.full(M, 10.0)]), (T, 1, 1))
        counts = np.full(T, M, np.int32)
        counts[2::N] = 3
    counts[1::N] = 0
    return a, counts


@pytest.mark.parametrize("space", ["Trajectory", "TargetPose", "TrajectoryWithTime"])
def test_actions_to_world_and_stepping_in_the_ego_frame(space, compiled_maps):
    E, N = 2, 4
    sim, cfg = _sim(compiled_maps, "loop", E, N, 7, action_space=space)
    twin, _ = _sim(compiled_maps, "loop", E, N, 7, ego_centric=False, action_space=space)
    step = {"Trajectory": "step_trajectory", "TargetPose": "step_target_pose", "TrajectoryWithTime": "step_trajectory_with_time"}[space]
    rows = parity.host(sim.reset())
    twin.reset()
    col = 3 if space == "TrajectoryWithTime" else 2
    for tick in range(3):
        a, counts = _ego_frame_actions(space, E, N, tick)
        shaped = torch.from_numpy(a.reshape((E, N) + a.shape[1:])).cuda()
        cn = torch.from_numpy(counts.reshape(E, N)).cuda() if counts is not None else None
        if tick == 0:
            sim.out["ec_flags"][0, 2] = 0  # the reference's last_obs is None
            rows["ec_flags"][2] = 0
        got = sim.actions_to_world(space, shaped, cn).cpu().numpy().reshape(a.shape)
        want = actions_to_world_rows(space, a, counts, rows)
        head = np.zeros(a.shape, dtype=bool)
        head[:, col] = True
        assert np.nanmax(np.abs(got - want)[~head]) <= 1e-9, (space, tick)
        d = np.abs(got - want)[head]
        assert np.minimum(d, 2 * math.pi - d).max() <= 1e-9, (space, tick)
        assert np.array_equal(got[1::N], a[1::N], equal_nan=True)  # no action: copied bit for bit
        if tick == 0:
            assert np.array_equal(got[2], a[2])  # ec_flags 0: copied bit for bit
            assert (got[0] != a[0]).any()
            sim.out["ec_flags"][0, 2] = 1
            rows["ec_flags"][2] = 1
            want = actions_to_world_rows(space, a, counts, rows)
        if space == "Trajectory":
            assert np.array_equal(got[2::N][:, :, 3:10], a[2::N][:, :, 3:10])  # past the count: not converted
        wt = torch.from_numpy(want.reshape((E, N) + a.shape[1:])).cuda()
        args = (shaped,) if cn is None else (shaped, cn)
        rows = parity.host(getattr(sim, step)(*args, ego_centric=True))
        trows = parity.host(getattr(twin, step)(*((wt,) if cn is None else (wt, cn))))
        _compare(rows, f"{space} t{tick}")
    assert np.abs(rows["ego_pos"] - trows["ego_pos"]).max() <= 1e-9, space
    assert np.abs(rows["ego_pos"][0, :2] - sim.spawns[0, 0, :2].cpu().numpy()).max() > 0.1  # it moved
    sim.close()
    twin.close()


def test_actions_to_world_refusals(compiled_maps):
    plain, _ = _sim(compiled_maps, "loop", 2, 4, 7, ego_centric=False, action_space="TargetPose")
    plain.reset()
    a = torch.zeros((2, 4, 4), dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    call = lambda s, space: s.lib.smx_actions_to_world(s.handle, space, a.data_ptr(), None, 0, b.data_ptr(), C.byref(s._out), s._stream_ptr())  # noqa: E731
    assert call(plain, nat.ACTION_SPACES["TargetPose"]) == -3  # SMX_ERR_STATE: no frame is kept
    with pytest.raises(ValueError):
        plain.actions_to_world("TargetPose", a)
    plain.close()
    lane, _ = _sim(compiled_maps, "loop", 2, 4, 7)
    lane.reset()
    assert call(lane, nat.ACTION_SPACES["Lane"]) == -1  # SMX_ERR_INVALID
    assert call(lane, nat.ACTION_SPACES["TargetPose"]) == -1  # not the handle's action space
    assert call(lane, 99) == -1
    torch.cuda.synchronize()
    lane.close()

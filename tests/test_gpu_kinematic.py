"""The kinematic action spaces (TargetPose, TrajectoryWithTime) on the device, through the C-ABI (BatchedSim is its thin
caller), against the reference's own outputs (tests/golden/kinematic_*.npz; tests/golden/gen_golden_kinematic.py).

Bounds: 1e-9 absolute on float64 state for one teacher-forced tick (the project's per-tick bound), 1e-5
at most over a free run (tightened to 10 x the measured drift: FREE_RUN_BOUND); the float32 ego columns to the float32
rounding of the fixture's float64 value +- 1 ulp — plus, for the "angular velocity" only, 4 x 2^-52 / dt: the column
is a difference of unit-vector components over dt, each component carries up to one float64 ulp of libm error on
either side, and where the heading barely moved the difference is all error (1e-15 against 0 is no float32 ulp).
"""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAPS = ("loop", "4lane", "minicity")
FORMS = ("small", "large")


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _sim(cm, action_space, spawns, E, N, dt, form="auto", **kw):
    from smarts_amd.engine import BatchedSim, SimConfig

    base = dict(done_collision=False, done_off_road=False, done_off_route=False)
    base.update(kw)
    cfg = SimConfig(num_envs=E, num_vehicles=N, dt=dt, action_space=action_space, launch_strategy=form, **base)
    return BatchedSim(cm, cfg, spawns=np.asarray(spawns, dtype=np.float64).reshape(1, E * N, 4))


def _state(sim, *names):
    import torch

    from smarts_amd import _native as nat

    torch.cuda.synchronize()
    return [sim.state[nat.S[n]].cpu().numpy().reshape(-1) for n in names]


def _write_state(sim, **rows):
    import torch

    from smarts_amd import _native as nat

    for name, values in rows.items():
        sim.state[nat.S[name]] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).reshape(sim.E, sim.N).to(sim.device)


def _ulp32(want):
    return np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)


def _check_ego(sim, out, g, t, sel, dt, where):
    """ego_f32 / ego_pos of the observation after tick t (t = 0: the reset observation) against BoxChassis."""
    import torch

    from smarts_amd import _native as nat

    torch.cuda.synchronize()
    ef = out["ego_f32"].cpu().numpy().reshape(-1, nat.EGO_F32_COUNT)
    pos = out["ego_pos"].cpu().numpy().reshape(-1, 3)
    worst = 0.0
    cols = [("HEADING", g["veh"][t, sel, 2], 0.0), ("SPEED", g["box_speed"][t, sel], 0.0),
            ("YAW_RATE", g["box_yaw_rate"][t, sel], 0.0), ("STEERING", g["box_steering"][t, sel], 0.0)]
    for q in range(3):
        cols.append((("LIN_VEL", q), g["box_lin_vel"][t, sel, q], 0.0))
        cols.append((("ANG_VEL", q), g["box_ang_vel"][t, sel, q], 4 * 2.0 ** -52 / dt))
    for col, want, floor in cols:
        k = nat.EGO[col] if isinstance(col, str) else nat.EGO[col[0]] + col[1]
        got = ef[:, k].astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (where, col)  # None -> NaN, at the same places
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok].astype(np.float32).astype(np.float64))
        tol = _ulp32(want[ok]) + floor
        worst = max(worst, float((err / tol).max()) if ok.any() else 0.0)
        assert (err <= tol).all(), (where, col, float(err.max()), got[ok][err.argmax()], want[ok][err.argmax()])
    assert np.abs(pos[:, :2] - g["veh"][t, sel, :2]).max() <= 1e-9, where
    return worst


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag", ["dt100", "dt010"])
def test_target_pose_step_parity_and_ego_read_back(compiled_maps, tag, form):
    """Teacher-forced: every tick starts from the fixture's pose rows, one step, pose / speed / both headings within
    1e-9 and the ego read-back rows against BoxChassis, the reset observation (no yaw rate yet) included."""
    import torch

    g = _load(f"kinematic_target_pose_{tag}.npz")
    dt, tg, raw, veh, speed = float(g["dt"]), g["targets"], g["raw"], g["veh"], g["speed"]
    worst, worst_ego = 0.0, 0.0
    for m, name in enumerate(MAPS):
        sel = np.flatnonzero(g["map"] == m)
        E, N = 3, len(sel) // 3
        sim = _sim(compiled_maps(name), "TargetPose", g["start"][sel], E, N, dt, form)
        assert (sim.launch_form() == "small") == (form == "small")
        out = sim.reset()
        x, y, h, d, u = _state(sim, "X", "Y", "HEADING", "DELTA", "U")
        assert np.array_equal(x, raw[0, sel, 0]) and np.array_equal(h, veh[0, sel, 2]) and np.array_equal(d, raw[0, sel, 2])
        worst_ego = max(worst_ego, _check_ego(sim, out, g, 0, sel, dt, f"{name} reset"))
        for t in range(tg.shape[0]):
            _write_state(sim, X=raw[t, sel, 0], Y=raw[t, sel, 1], HEADING=veh[t, sel, 2], DELTA=raw[t, sel, 2], U=speed[t, sel])
            out = sim.step_target_pose(torch.from_numpy(tg[t, sel].reshape(E, N, 4)))
            x, y, h, d, u = _state(sim, "X", "Y", "HEADING", "DELTA", "U")
            for got, want in ((x, raw[t + 1, sel, 0]), (y, raw[t + 1, sel, 1]), (h, veh[t + 1, sel, 2]), (d, raw[t + 1, sel, 2]),
                              (u, speed[t + 1, sel])):
                err = float(np.abs(got - want).max())
                worst = max(worst, err)
                assert err <= 1e-9, (name, t, err)
            worst_ego = max(worst_ego, _check_ego(sim, out, g, t + 1, sel, dt, f"{name} t{t}"))
        sim.sync()
        sim.close()
    print(f"TargetPose {tag} {form}: worst teacher-forced error {worst:.3g}, worst ego column error {worst_ego:.3g} of its bound")


# The issue's bound is 1e-5 (the project's bound for 30 free ticks), to be tightened to 10 x the measured maximum where
# the drift is nowhere near it.  Measured on an MI355X over the 40 ticks: 0 at dt 0.1, 2.78e-16 at dt 0.01, either form.
FREE_RUN_BOUND = 2.8e-15


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tag", ["dt100", "dt010"])
def test_target_pose_free_run(compiled_maps, tag, form):
    """The fixture's 40 ticks without rewriting state: pose, headings and speed within FREE_RUN_BOUND of the provider's."""
    import torch

    g = _load(f"kinematic_target_pose_{tag}.npz")
    dt, tg, raw, veh, speed = float(g["dt"]), g["targets"], g["raw"], g["veh"], g["speed"]
    worst = 0.0
    for m, name in enumerate(MAPS):
        sel = np.flatnonzero(g["map"] == m)
        E, N = 3, len(sel) // 3
        sim = _sim(compiled_maps(name), "TargetPose", g["start"][sel], E, N, dt, form)
        sim.reset()
        for t in range(tg.shape[0]):
            sim.step_target_pose(torch.from_numpy(tg[t, sel].reshape(E, N, 4)))
            x, y, h, d, u = _state(sim, "X", "Y", "HEADING", "DELTA", "U")
            # (the wrapped heading may sit on the other side of +-pi from the fixture's: compare on the circle)
            dh = np.abs((h - veh[t + 1, sel, 2] + math.pi) % (2 * math.pi) - math.pi)
            for err in (np.abs(x - raw[t + 1, sel, 0]), np.abs(y - raw[t + 1, sel, 1]), dh, np.abs(d - raw[t + 1, sel, 2]),
                        np.abs(u - speed[t + 1, sel])):
                worst = max(worst, float(err.max()))
        sim.sync()
        sim.close()
    print(f"TargetPose {tag} {form}: worst free-run error over {tg.shape[0]} ticks {worst:.3g}")
    assert worst <= FREE_RUN_BOUND, worst


def _twt_batch(g, dt, E, N):
    legal = np.flatnonzero(g["dt"] == dt)[:E * N]
    assert len(legal) == E * N
    return legal, g["trajs"][legal].reshape(E, N, 5, -1), g["counts"][legal].reshape(E, N)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", [0.1, 0.01])
def test_trajectory_with_time_step_parity(compiled_maps, dt, form):
    """One tick per trajectory of the fixture (the provider keeps no state from tick to tick, so a free run is the
    same arithmetic again): pose and speed within 1e-9, and a second tick without actions changes nothing."""
    import torch

    from smarts_amd.engine import make_spawns

    g = _load("kinematic_trajectory_with_time.npz")
    E, N = 5, 32
    cm = compiled_maps("loop")
    sim = _sim(cm, "TrajectoryWithTime", make_spawns(cm, E, N, episodes=1, seed=3), E, N, dt, form)
    legal, trajs, counts = _twt_batch(g, dt, E, N)
    sim.reset()
    h0, = _state(sim, "HEADING")
    sim.step_trajectory_with_time(torch.from_numpy(trajs), torch.from_numpy(counts))
    x, y, h, u, lh, ldt = _state(sim, "X", "Y", "HEADING", "U", "LAT_INT", "SPD_INT")
    worst = max(float(np.abs(got - want).max()) for got, want in
                ((x, g["pose"][legal, 0]), (y, g["pose"][legal, 1]), (h, g["pose"][legal, 2]), (u, g["speed"][legal])))
    print(f"TrajectoryWithTime dt {dt} {form}: worst error {worst:.3g}")
    assert worst <= 1e-9
    assert np.array_equal(lh, h0) and (ldt == dt).all()  # BoxChassis._last_heading / _last_dt
    sim.step_trajectory_with_time(torch.from_numpy(trajs), torch.zeros((E, N), dtype=torch.int32))
    x2, h2, lh2 = _state(sim, "X", "HEADING", "LAT_INT")
    assert np.array_equal(x2, x) and np.array_equal(h2, h) and np.array_equal(lh2, lh)  # no action: no control() call
    sim.sync()
    sim.close()


def test_illegal_trajectories_move_nothing_and_are_reported(compiled_maps):
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import make_spawns

    g = _load("kinematic_trajectory_with_time.npz")
    dt, E, N = 0.1, 2, 16
    bad = np.flatnonzero(g["illegal_dt"] == dt)
    legal = np.flatnonzero(g["dt"] == dt)[:E * N - len(bad)]
    assert len(bad) >= 10 and len(legal) >= 8
    trajs = np.concatenate([g["illegal"][bad], g["trajs"][legal]]).reshape(E, N, 5, -1)
    counts = np.concatenate([g["illegal_counts"][bad], g["counts"][legal]]).astype(np.int32).reshape(E, N)
    cm = compiled_maps("loop")
    sim = _sim(cm, "TrajectoryWithTime", make_spawns(cm, E, N, episodes=1, seed=4), E, N, dt)
    sim.reset()
    sim.sync()
    before = _state(sim, "X", "Y", "HEADING", "U", "LAT_INT", "SPD_INT")
    sim.step_trajectory_with_time(torch.from_numpy(trajs), torch.from_numpy(counts))
    with pytest.raises(nat.SmxError, match=r"\(-1\).*TrajectoryWithTime"):
        sim.sync()
    sim.sync()  # reported once
    after = _state(sim, "X", "Y", "HEADING", "U", "LAT_INT", "SPD_INT")
    nb = len(bad)
    for b, a in zip(before, after):
        assert np.array_equal(b[:nb], a[:nb])
    for got, want in ((after[0], g["pose"][legal, 0]), (after[1], g["pose"][legal, 1]), (after[2], g["pose"][legal, 2]),
                      (after[3], g["speed"][legal])):
        assert np.abs(got[nb:] - want).max() <= 1e-9
    # more points than the buffer holds, or a negative count: refused as well, nothing read
    counts[:] = 0
    counts[0, 0], counts[0, 1] = trajs.shape[3] + 1, -1
    sim.step_trajectory_with_time(torch.from_numpy(trajs), torch.from_numpy(counts))
    with pytest.raises(nat.SmxError):
        sim.sync()
    sim.close()


def test_sensors_see_a_kinematic_agent_as_any_vehicle(compiled_maps):
    """After 7 TargetPose ticks a Continuous batch is reset onto the kinematic batch's poses: the outputs that depend on
    poses alone are the same bytes."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.lidar import Planar100

    g = _load("kinematic_target_pose_dt100.npz")
    for m, name in enumerate(MAPS):
        sel = np.flatnonzero(g["map"] == m)
        E, N = 3, len(sel) // 3
        kw = dict(neighbors=True, nb_radius=60.0, ogm=True, ogm_width=64, ogm_height=64, ogm_resolution=50 / 64, dagm=True,
                  dagm_width=64, dagm_height=64, dagm_resolution=50 / 64, lidar=Planar100)
        a = _sim(compiled_maps(name), "TargetPose", g["start"][sel], E, N, 0.1, **kw)
        a.reset()
        for t in range(7):
            out_a = a.step_target_pose(torch.from_numpy(g["targets"][t, sel].reshape(E, N, 4)))
        x, y, h, u = _state(a, "X", "Y", "HEADING", "U")
        b = _sim(compiled_maps(name), "Continuous", np.stack([x, y, h, u], axis=1), E, N, 0.1, **kw)
        out_b = b.reset()
        torch.cuda.synchronize()
        names = [k for k in out_a if k.startswith("wp_") or k in ("nb_pos", "nb_heading", "nb_slot", "nb_count", "nb_lane_index",
                                                                    "nb_lane_id", "ego_lane", "ogm", "dagm", "lidar_hit", "lidar_point")]
        assert len(names) >= 17
        for k in names:
            assert torch.equal(out_a[k], out_b[k]), (name, k)
        ev_a, ev_b = out_a["events"].cpu().numpy(), out_b["events"].cpu().numpy()
        for col in (nat.EV_OFF_ROAD, nat.EV_ON_SHOULDER, nat.EV_WRONG_WAY):
            assert np.array_equal(ev_a[..., col], ev_b[..., col]), (name, col)
        assert out_a["active"].all() and out_b["active"].all()
        a.close()
        b.close()


def test_collision_thresholds_with_target_poses(compiled_maps):
    """The 0.0499 / 0.0501 m gaps of the contact tests (tests/test_gpu_collisions.py's envelopes of test_collision.py; the
    ring of test_collision.py:206-282 as tests/test_gpu_parity.py lays it out) re-expressed with target poses: four kinematic agents
    are commanded from 10 m away to 0.0501 m (env 0) / 0.0499 m (env 1) clear of a standing one.  The collision test
    runs on the poses after the move: nothing in env 0; in env 1 every pair that touches names each other on that tick."""
    import torch

    from smarts_amd import _native as nat
    from smarts_amd.engine import lane_heading
    from smarts_amd.vias import _position_at_shape_offset

    cm = compiled_maps("4lane")
    E, N = 2, 5
    shape = cm.lane_shape(cm.lane_ids.index("edge-south-SN_0"))
    cx, cy = _position_at_shape_offset(shape, 40.0)
    h = lane_heading(shape, 0)
    f, r = np.array([-np.sin(h), np.cos(h)]), np.array([np.cos(h), np.sin(h)])
    spawns, targets = np.zeros((E * N, 4)), np.full((E, N, 4), np.nan)
    for e, sep in enumerate((0.0501, 0.0499)):
        ring = [(0.0, 0.0), (3.68 + sep, 0.0), (0.0, 1.47 + sep), (-(3.68 + sep), 0.0), (0.0, -(1.47 + sep))]
        for k, (along, across) in enumerate(ring):
            far = 1.0 if k == 0 else (abs(along) + abs(across) + 10.0) / (abs(along) + abs(across))
            spawns[e * N + k] = (*(np.array([cx, cy]) + far * (along * f + across * r)), h, 0.0)
            if k:
                targets[e, k] = (*(np.array([cx, cy]) + along * f + across * r), h, 0.1)  # there in one tick
    sim = _sim(cm, "TargetPose", spawns, E, N, 0.1)
    out = sim.reset()
    torch.cuda.synchronize()
    assert not out["collidees"].cpu().numpy().any()
    out = sim.step_target_pose(torch.from_numpy(targets))
    torch.cuda.synchronize()
    masks = out["collidees"].cpu().numpy().astype(np.uint64)
    hit = out["events"].cpu().numpy()[..., nat.EV_COLLISIONS]
    assert masks[0].tolist() == [0, 0, 0, 0, 0] and not hit[0].any()
    assert masks[1].tolist() == [0b11110, 1, 1, 1, 1] and hit[1].all()
    x, y = _state(sim, "X", "Y")
    assert np.array_equal(x.reshape(E, N)[:, 1:], targets[:, 1:, 0]) and np.array_equal(y.reshape(E, N)[:, 1:], targets[:, 1:, 1])
    # vehicles are not pushed apart: a tick without actions leaves them where they are, still touching
    out = sim.step_target_pose(torch.full((E, N, 4), float("nan"), dtype=torch.float64))
    x2, u2 = _state(sim, "X", "U")
    assert np.array_equal(x2, x) and (u2 == 0).all()
    assert out["collidees"].cpu().numpy().astype(np.uint64)[1].tolist() == [0b11110, 1, 1, 1, 1]
    sim.sync()
    sim.close()


def test_entry_points_accept_and_refuse_by_action_space(compiled_maps):
    """smx_create takes the two spaces; each step entry point refuses a handle of another space, both ways."""
    import ctypes as C

    import torch

    from smarts_amd.engine import make_spawns

    cm = compiled_maps("loop")
    E, N = 1, 4
    sp = make_spawns(cm, E, N, episodes=1, seed=1)
    tp = _sim(cm, "TargetPose", sp, E, N, 0.1)
    tw = _sim(cm, "TrajectoryWithTime", sp, E, N, 0.1)
    co = _sim(cm, "Continuous", sp, E, N, 0.1)
    for s in (tp, tw, co):
        s.reset()
    buf = torch.full((E, N, 5, 8), float("nan"), dtype=torch.float64, device="cuda")  # (NaN x: no action)
    cnt = torch.zeros((E, N), dtype=torch.int32, device="cuda")
    f32 = torch.zeros((E, N, 3), dtype=torch.float32, device="cuda")

    def calls(s):
        args = (C.byref(s._st), C.byref(s._sp), C.byref(s._out), s._stream_ptr())
        return {"TargetPose": s.lib.smx_step_target_pose(s.handle, buf.data_ptr(), *args),
                "TrajectoryWithTime": s.lib.smx_step_trajectory_with_time(s.handle, buf.data_ptr(), cnt.data_ptr(), 8, *args),
                "Continuous": s.lib.smx_step_continuous(s.handle, f32.data_ptr(), *args),
                "Trajectory": s.lib.smx_step_trajectory(s.handle, buf.data_ptr(), cnt.data_ptr(), *args)}

    for s in (tp, tw, co):
        rc = calls(s)
        assert {k for k, v in rc.items() if v == 0} == {s.cfg.action_space}, (s.cfg.action_space, rc)
        assert all(v == -1 for k, v in rc.items() if k != s.cfg.action_space)
        assert b"do not match cfg.action_space" in s.lib.smx_last_error(s.handle)
    for s, hint in ((tp, "step_target_pose"), (tw, "step_trajectory_with_time")):
        with pytest.raises(ValueError, match=hint):
            s.step(f32)
        s.sync()
        s.close()
    co.close()

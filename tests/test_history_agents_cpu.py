"""History agents, host side (smarts_amd/traffic_history.py): first / last frames, the expert action and the windows of
one env per recorded vehicle, on the synthetic histories of tests/golden/traffic_history_*.npz — the tables already pinned
to the reference's provider — and on the scene of tests/history_agents_ref.py's model.  No device."""
import glob
import math
import os

import numpy as np
import pytest

import mpc_imitation_ref as imit
from smarts_amd.traffic_history import TrafficHistoryTable, slots_needed

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("traffic_history_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "traffic_history_*.npz")))


def _table(name, spare=1):
    g = np.load(os.path.join(GOLDEN, f"traffic_history_{name}.npz"))
    veh = [(int(r[0]), int(r[1])) + tuple(None if np.isnan(v) else float(v) for v in r[2:5]) for r in g["vehicle_rows"]]
    traj = [(int(r[0]),) + tuple(float(v) for v in r[1:6]) for r in g["trajectory_rows"]]
    dt = float(g["dt"])
    return TrafficHistoryTable.from_rows(veh, traj, dt, slots_needed(veh, traj, dt) + spare)


def _present(table, vid):
    return [k for k in range(table.num_frames) if vid in table.vehicle[k]]


def test_there_are_cases():
    assert len(CASES) >= 5


@pytest.mark.parametrize("name", CASES)
def test_first_and_last_seen_frames(name):
    table = _table(name)
    first = table.first_seen_frames()
    assert list(first) == table.vehicle_ids() and len(first) >= 2  # every vehicle, ascending
    for vid in table.vehicle_ids():
        held = _present(table, vid)
        assert first[vid] == held[0] and table.last_seen_frame(vid) == held[-1]
        assert table.frames_of(vid).tolist() == held
        assert isinstance(first[vid], int)
    with pytest.raises(KeyError):
        table.last_seen_frame(max(table.vehicle_ids()) + 1)
    with pytest.raises(KeyError):
        table.last_seen_frame(-1)


@pytest.mark.parametrize("name", CASES)
def test_expert_actions_are_the_inverse_of_the_imitation_controller(name):
    """Rule by rule, and through the Imitation step of tests/mpc_imitation_ref.py: from a frame's recorded heading and
    speed the action lands on the next frame's.  Bound 1e-12: the round trip is under twenty float64 operations on values
    below 100 (speeds) and 2 pi (headings), each within 2^-52 relative: 20 x 2^-52 x 100 = 4.4e-13."""
    table = _table(name)
    dt = table.dt
    labelled = gaps = 0
    for vid in table.vehicle_ids():
        held = _present(table, vid)
        acts = table.expert_actions(vid)
        assert acts.shape == (len(held), 2) and acts.dtype == np.float64
        for i, f in enumerate(held):
            s0 = int(np.nonzero(table.vehicle[f] == vid)[0][0])
            x, y, h0, v0 = table.frames[f, s0]
            if f + 1 not in held:
                assert np.isnan(acts[i]).all(), (vid, f)  # "no action": the last frame, or a gap ahead
                gaps += 1
                continue
            s1 = int(np.nonzero(table.vehicle[f + 1] == vid)[0][0])
            h1, v1 = table.frames[f + 1, s1, 2:4]
            assert acts[i, 0] == (v1 - v0) / dt
            assert acts[i, 1] == ((h1 - h0 + math.pi) % (2 * math.pi) - math.pi) / dt
            assert abs(acts[i, 1]) <= math.pi / dt
            out = imit.imitation_step(float(x), float(y), float(h0), float(v0), float(acts[i, 0]), float(acts[i, 1]), dt)
            assert out is not None
            assert abs(out[3] - v1) <= 1e-12, (vid, f, out[3], v1)
            assert abs(imit.min_angles_difference_signed(out[2], h1)) <= 1e-12, (vid, f, out[2], h1)
            labelled += 1
    assert gaps >= len(table.vehicle_ids())  # (every vehicle's last frame at least)
    # period_2dt is recorded every second frame: no frame of it has a successor (the test below)
    assert labelled >= 7 or (name == "period_2dt" and labelled == 0), labelled


def test_data_coarser_than_dt_ends_at_the_first_gap():
    """Data recorded at twice dt flickers: every frame that holds the vehicle is followed by one that lacks it."""
    table = _table("period_2dt")
    for vid in table.vehicle_ids():
        assert np.isnan(table.expert_actions(vid)).all()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("res", [0, 1])
def test_history_agent_windows(name, res):
    table = _table(name)
    ids = table.vehicle_ids()
    first = table.first_seen_frames()
    A = 3
    E = len(ids) + 2
    start, vehicle = table.history_agent_windows(ids, E, A, res)
    assert start.shape == (1, E) and vehicle.shape == (1, E, A) and start.dtype == np.int32 and vehicle.dtype == np.int32
    crowded = 0
    for k, vid in enumerate(ids):
        assert start[0, k] == first[vid] - res
        frame = start[0, k] + res  # the reset observation's frame: the vehicle's first
        assert vehicle[0, k, 0] == vid and vid in table.vehicle[frame]
        others = sorted(int(v) for v in table.vehicle[frame] if v >= 0 and v != vid)
        want = (others + [-1] * A)[:A - 1]
        assert vehicle[0, k, 1:].tolist() == want, (vid, vehicle[0, k], others)
        crowded += len(others) > 0
    assert (vehicle[0, len(ids):] == -1).all() and (start[0, len(ids):] == 0).all()
    assert crowded > 0 or name == "period_2dt"  # (whose two vehicles alternate)
    if res:
        assert (start[0, :len(ids)] < 0).any() or min(first.values()) > 0  # negative starts are fine
    with pytest.raises(ValueError):
        table.history_agent_windows(ids, len(ids) - 1, A)
    with pytest.raises(KeyError):
        table.history_agent_windows([max(ids) + 1], E, A)
    # one agent slot: the vehicle alone
    _, alone = table.history_agent_windows(ids, E, 1)
    assert alone[0, :len(ids), 0].tolist() == ids


def test_the_model_scene_without_a_device():
    """tests/history_agents_ref.py's table on a straight stand-in for a map: the scene the GPU tests run holds what the
    issue asks of it (a follower that runs into a standing vehicle, one that leaves, a reused slot, an agent whose
    vehicle the reset frame lacks, an env that follows nothing, one that also uses `replaced`)."""
    import history_agents_ref as ref
    from smarts_amd import _native as nat

    class Straight:  # the few map fields scene() reads: four straight lanes, two roads, far apart
        n_lanes = 4
        lane_in_junction = [False] * 4
        lane_length = [400.0, 300.0, 200.0, 100.0]
        lane_road = [0, 1, 2, 3]

        def lane_shape(self, i):
            return np.array([[0.0, 300.0 * i], [self.lane_length[i], 300.0 * i]])

    sc = ref.scene(Straight())
    table = sc["table"]
    assert table.num_slots == ref.SLOTS and table.num_frames == ref.FRAMES and sc["far"] > 80.0
    slot = lambda v: int(np.nonzero((table.vehicle == v).any(axis=0))[0][0])  # noqa: E731
    assert slot(ref.LEAVER) == slot(ref.LATE) and table.last_seen_frame(ref.LEAVER) == ref.LEAVER_LAST
    m = ref.Model(table, ref.STARTS, ref.FOLLOW, 0)
    m.reset()
    assert m.status.tolist() == [[0, 0, 2], [0, 0, 2], [2, 2, 2], [0, 0, 2]]
    assert m.done_count.tolist() == [1, 1, 3, 1]
    assert m.social_present(1, ref.REPLACED).tolist() == [False, False, True]  # both twins of env 1 hidden, the leaver not
    assert m.social_present(2, ref.REPLACED).sum() == 3 and m.social_present(3, ref.REPLACED).sum() == 0
    left_at = {}
    for t in range(30):
        left, env_done = m.step()
        for e, a in zip(*np.nonzero(left)):
            left_at[(int(e), int(a))] = t
        assert env_done[2]
    assert left_at == {(0, 1): ref.LEAVER_LAST, (3, 0): ref.LEAVER_LAST}
    assert m.status[0].tolist() == [nat.HA_FOLLOWING, nat.HA_LEFT, nat.HA_ABSENT]
    # the driver closes in on the standing vehicle: centres nearer than a sedan's length within the run
    d = table.frames[:, slot(ref.DRIVER), :2] - table.frames[:, slot(ref.STANDING), :2]
    assert np.hypot(d[:, 0], d[:, 1]).min() < 1.0

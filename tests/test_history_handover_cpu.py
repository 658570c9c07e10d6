"""Handing history agents over to actions, host side: TrafficHistoryTable.zone_entry_frames / handover_ticks on a
hand-made table, tests/history_handover_ref.py's model on a straight stand-in for a map, and HistoryObserver's methods
with and without ``handover`` over a stand-in for the sim.  No device."""
import math
import types

import numpy as np
import pytest

from smarts_amd import _native as nat
from smarts_amd.traffic_history import TrafficHistoryTable

DT = 0.1
# the zone: PositionalZone(pos=(10, 5), size=(4, 2)) = the open rectangle (8, 12) x (4, 6)
POS, SIZE = (10.0, 5.0), (4.0, 2.0)
ON_EDGE, CROSSES, NEVER, RETURNS, CORNER = 1, 2, 3, 4, 5


def _table():
    """Six frames, five slots, one vehicle a slot (slot = id - 1)."""
    frames = np.zeros((6, 5, 4))
    vehicle = np.full((6, 5), -1, dtype=np.int32)
    for k in range(6):
        rows = {
            ON_EDGE: (8.0, 5.0),                                  # exactly on the low x edge, in every frame
            CROSSES: (6.0 + 1.0 * k, 5.0),                        # x = 6, 7, 8 (the edge), 9 (inside: frame 3), 10, 11
            NEVER: (10.0, 20.0 + k),                              # inside in x, far away in y
            RETURNS: ((9.0, 5.5) if k in (1, 4) else (0.0, 0.0)),  # enters at 1, leaves, comes back at 4
            CORNER: (12.0, 6.0) if k < 5 else (11.999, 5.999),    # the high corner itself, then just inside it
        }
        for vid, (x, y) in rows.items():
            frames[k, vid - 1] = (x, y, 0.0, 1.0)
            vehicle[k, vid - 1] = vid
    vehicle[0, RETURNS - 1] = -1  # (absent in frame 0: an empty cell's zeros are not a position)
    return TrafficHistoryTable(frames, vehicle, DT)


def test_zone_entry_frames():
    table = _table()
    entry = table.zone_entry_frames(POS, SIZE)
    assert entry == {CROSSES: 3, RETURNS: 1, CORNER: 5}  # the boundary is outside; the first entry wins; ascending ids
    assert list(entry) == sorted(entry) and all(isinstance(v, int) for v in entry.values())
    assert ON_EDGE not in entry and NEVER not in entry
    # an empty cell is no vehicle at the origin
    assert table.zone_entry_frames((0.0, 0.0), (1.0, 1.0)) == {RETURNS: 2}
    # a zone that holds everything: every vehicle's first frame
    assert table.zone_entry_frames((0.0, 0.0), (1000.0, 1000.0)) == table.first_seen_frames()
    # a zone without an interior holds nobody
    assert table.zone_entry_frames(POS, (0.0, 2.0)) == {}
    # size is (extent along x, extent along y): the transposed zone is another rectangle
    assert table.zone_entry_frames(POS, (2.0, 4.0)) == {CROSSES: 4}


def test_handover_ticks():
    table = _table()
    entry = table.zone_entry_frames(POS, SIZE)
    follow = np.array([[[CROSSES, RETURNS, -1], [NEVER, ON_EDGE, CORNER]],
                       [[CORNER, CROSSES, 77], [RETURNS, -5, CROSSES]]], dtype=np.int32)
    starts = np.array([[0, 2], [4, -3]], dtype=np.int32)
    ticks = table.handover_ticks(follow, starts, entry)
    assert ticks.dtype == np.int32 and ticks.shape == follow.shape
    assert ticks.tolist() == [[[3, 1, -1], [-1, -1, 3]],   # env 1 starts at frame 2: CORNER's frame 5 is tick 3
                              [[1, 0, -1], [4, -1, 6]]]    # a start past the entry clamps to 0; a negative start adds
    # the static form, and shapes that do not belong together
    assert np.array_equal(TrafficHistoryTable.handover_ticks(follow, starts, entry), ticks)
    with pytest.raises(ValueError):
        table.handover_ticks(follow, starts[:, :1], entry)
    assert (table.handover_ticks(follow, starts, {}) == -1).all()


def test_the_handover_scene_without_a_device():
    """tests/history_handover_ref.py's table and actions on a straight stand-in for a map: the cases the issue lists
    are what the model makes of them, and every driven pose of the run is finite and stays near the recording."""
    import history_agents_ref as ref
    import history_handover_ref as hand

    class Straight:  # the few map fields scene() reads: four straight lanes, two roads, far apart
        n_lanes = 4
        lane_in_junction = [False] * 4
        lane_length = [400.0, 300.0, 200.0, 100.0]
        lane_road = [0, 1, 2, 3]

        def lane_shape(self, i):
            return np.array([[0.0, 300.0 * i], [self.lane_length[i], 300.0 * i]])

    table = ref.scene(Straight())["table"]
    assert hand.HANDOVER.shape == ref.FOLLOW.shape and hand.HANDOVER.dtype == np.int32
    assert not np.array_equal(hand.HANDOVER[0], hand.HANDOVER[1])
    m = hand.Model(table, ref.STARTS, ref.FOLLOW, hand.HANDOVER, 0)
    m.reset()
    assert m.status.tolist() == [[0, 0, 2], [0, 0, 2], [2, 2, 2], [0, 0, 2]]
    seen_nan = seen_scalar = False
    driven_ticks = np.zeros((ref.E, ref.AGENTS), dtype=int)
    for t in range(30):
        acts = hand.actions(t)
        will = m.driven_next()
        seen_nan |= bool(np.isnan(acts[..., 0])[:, :ref.AGENTS][will].any())
        seen_scalar |= bool((np.isnan(acts[..., 1]) & ~np.isnan(acts[..., 0]))[:, :ref.AGENTS][will].any())
        left, env_done = m.step(acts)
        driven_ticks += will
        assert np.array_equal(m.status == nat.HA_DRIVEN, will)
        assert not (left & will).any()  # a driven agent never leaves
        assert np.isfinite(m.held[m.alive]).all()
    # case 1: env 0 / agent 0 drives from tick 5 on beside the follower that leaves at its frame
    assert driven_ticks[0, 0] == 25 and m.status[0].tolist() == [nat.HA_DRIVEN, nat.HA_LEFT, nat.HA_ABSENT]
    # case 2: driven from the first tick; case 3: LATE stays absent, whatever its H
    assert driven_ticks[1, 1] == 30 and driven_ticks[1, 2] == 0 and m.status[1, 2] == nat.HA_ABSENT
    # case 4: handed over before its vehicle's last frame, alive and driven at the end; case 5: a follower throughout
    assert driven_ticks[3, 0] == 20 and m.alive[3, 0] and m.status[3, 0] == nat.HA_DRIVEN
    assert driven_ticks[3, 1] == 0 and m.status[3, 1] == nat.HA_FOLLOWING
    # case 6: the slots that follow nothing carry H = 7 and are never driven
    assert (hand.HANDOVER[0][ref.FOLLOW[0] < 0] == 7).all() and driven_ticks[ref.FOLLOW[0] < 0].sum() == 0
    assert seen_nan and seen_scalar
    # the free run the GPU tests check against the map's grids: every driven pose of it, finite
    poses = hand.driven_poses(table, ref.STARTS, hand.HANDOVER, 0, 30)
    assert len(poses) == driven_ticks.sum() and np.isfinite(poses).all()


class _FakeSim:
    """What HistoryObserver's stepping methods touch of a BatchedSim."""

    def __init__(self, E, A, S):
        import torch

        self.device = torch.device("cpu")
        self.calls = []
        self.out = {"expert_action": torch.zeros((E, A + S, 3)), "history_agent_status": torch.zeros((E, A + S), dtype=torch.uint8)}
        self.env_ticks = torch.zeros(E, dtype=torch.int32)
        self.flags = torch.ones((E, A + S), dtype=torch.int32)

    def step_history_agents(self):
        self.calls.append(("follow",))
        return self.out

    def step_history_handover(self, actions):
        self.calls.append(("handover", actions.numpy().copy()))
        return self.out


def _observer(monkeypatch, handover=None):
    import torch

    from smarts_amd.env.history_observer import HistoryObserver

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    ho = object.__new__(HistoryObserver)
    ho.E, ho.A, ho.S, ho.dt = 2, 2, 3, DT
    ho.followed = np.array([[[22, 11], [33, -1]]], dtype=np.int32)
    ho.sim = _FakeSim(ho.E, ho.A, ho.S)
    ho.handover = None if handover is None else ho._handover_table(handover)
    ho._was_reset = True
    ho._collect = types.MethodType(lambda self, out: out, ho)
    return ho


def test_history_observer_without_handover_is_what_it_was(monkeypatch):
    ho = _observer(monkeypatch)
    import inspect

    from smarts_amd.env.history_observer import HistoryObserver

    sig = inspect.signature(HistoryObserver.__init__)
    assert sig.parameters["handover"].default is None and list(sig.parameters)[-1] == "handover"  # appended: positions keep
    assert inspect.signature(HistoryObserver.step).parameters["actions"].default is None
    assert ho.step() is ho.sim.out and ho.sim.calls == [("follow",)]  # the following tick, no action tensor is made
    assert ho.driven() == [[], []]
    with pytest.raises(ValueError, match="handover"):
        ho.step({"Agent-history-vehicle-22": (0.0, 0.0)})
    assert ho.sim.calls == [("follow",)]
    ho.sim.out["history_agent_status"][0, 1] = nat.HA_LEFT
    ho.sim.out["expert_action"][0, 0, :2] = torch_pair = __import__("torch").tensor([0.25, -0.5])
    labels = ho.expert_actions()
    assert [sorted(d) for d in labels] == [["Agent-history-vehicle-22"], ["Agent-history-vehicle-33"]]
    assert labels[0]["Agent-history-vehicle-22"].tolist() == torch_pair.tolist()


def test_history_observer_handover_forms(monkeypatch):
    name = lambda v: f"Agent-history-vehicle-{v}"  # noqa: E731
    assert _observer(monkeypatch, 4).handover.tolist() == [[[4, 4], [4, -1]]]  # an int: every follower; never a slot that follows nothing
    assert _observer(monkeypatch, {22: 0, 33: 9}).handover.tolist() == [[[0, -1], [9, -1]]]
    ready = np.array([[[1, 2], [3, 4]]])
    assert _observer(monkeypatch, ready).handover.tolist() == ready.tolist() and _observer(monkeypatch, ready).handover.dtype == np.int32
    with pytest.raises(ValueError):
        _observer(monkeypatch, np.zeros((1, 2, 3), dtype=np.int32))
    ho = _observer(monkeypatch, {22: 0, 33: 2, 11: 1})
    assert ho.driven() == [[name(22)], []]
    ho.sim.env_ticks[:] = 1
    assert ho.driven() == [[name(22), name(11)], []]
    ho.sim.env_ticks[:] = 2
    ho.sim.flags[0, 0] = 0  # not alive: not driven, whatever its H
    assert ho.driven() == [[name(11)], [name(33)]]
    # actions: a pair, a scalar, a missing id; one mapping for every env or one per env
    ho.step({name(11): (0.5, -0.25), name(33): 3.0, "Agent-history-vehicle-99": (1.0, 1.0)})
    kind, rows = ho.sim.calls[-1]
    assert kind == "handover" and rows.shape == (2, 5, 3) and rows.dtype == np.float32
    assert rows[0, 1].tolist() == [0.5, -0.25, 0.0]
    assert rows[1, 0, 0] == 3.0 and math.isnan(rows[1, 0, 1]) and rows[1, 0, 2] == 0.0  # the scalar form
    rest = np.ones((2, 5), dtype=bool)
    rest[0, 1] = rest[1, 0] = False
    assert np.isnan(rows[rest][:, :2]).all() and (rows[..., 2] == 0).all()  # a missing id, social rows: no action
    ho.step([{name(22): (1.0, 2.0)}, None])
    assert ho.sim.calls[-1][1][0, 0].tolist() == [1.0, 2.0, 0.0] and np.isnan(ho.sim.calls[-1][1][1, :, 0]).all()
    ho.step()
    assert np.isnan(ho.sim.calls[-1][1][..., 0]).all()
    with pytest.raises(ValueError):
        ho.step([{}])
    # a driven agent's label reads NaN
    ho.sim.out["history_agent_status"][0, 1] = nat.HA_DRIVEN
    ho.sim.out["expert_action"][0, 1, :2] = float("nan")
    labels = ho.expert_actions()
    assert np.isnan(labels[0][name(11)]).all() and not np.isnan(labels[0][name(22)]).any()

"""Bubbles over a replayed history, without a device (include/smx.h smx_set_history_bubbles): the rule
in NumPy (tests/history_bubbles_ref.py) against the fixture the reference's own bubble code wrote
(tests/golden/bubble_cursors.npz, tests/golden/gen_golden_bubbles.py), the cases the GPU tests run shown on the model, the
descriptors' refusals and the validation behind smx_set_history_bubbles."""
import ctypes as C
import os
from sys import maxsize

import numpy as np
import pytest

import history_bubbles_ref as bub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "bubble_cursors.npz"))
NAMES = [str(n) for n in GOLDEN["names"]]


def golden_bubbles(name):
    return [bub.B(x=r[0], y=r[1], size_x=r[2], size_y=r[3], margin=r[4], offset=(r[5], r[6]), follow=int(r[7]), hijack_limit=int(r[8]),
                  shadow_limit=int(r[9])) for r in GOLDEN[f"{name}/bubbles"]]


@pytest.mark.parametrize("name", NAMES)
def test_the_rule_equals_the_reference_exactly(name):
    """States, cursor masks, transitions and cursor states after every pass, as integers; the zone tests the fixture's poses
    need are at least CLEARANCE from an edge, so they are the same decisions in any arithmetic."""
    bubbles = golden_bubbles(name)
    pos, heading = GOLDEN[f"{name}/pos"], GOLDEN[f"{name}/heading"]
    alive, ego = GOLDEN[f"{name}/alive"].astype(bool), GOLDEN[f"{name}/ego"].astype(bool)
    A = pos.shape[1]
    state, mask = np.zeros(A, dtype=np.int64), np.zeros(A, dtype=np.int64)
    least = np.inf
    for t in range(len(pos)):
        state, mask, trans, cur, c, _ = bub.bubble_pass(bubbles, pos[t], heading[t], alive[t], ego[t], state, mask)
        least = min(least, c)
        assert np.array_equal(trans, GOLDEN[f"{name}/transitions"][t]), (name, t, trans, GOLDEN[f"{name}/transitions"][t])
        assert np.array_equal(cur, GOLDEN[f"{name}/cursors"][t]), (name, t)
        assert np.array_equal(state, GOLDEN[f"{name}/state"][t]), (name, t, state, GOLDEN[f"{name}/state"][t])
        assert np.array_equal(mask, GOLDEN[f"{name}/mask"][t]), (name, t, mask, GOLDEN[f"{name}/mask"][t])
    assert least >= bub.CLEARANCE, least


def test_the_fixture_covers_the_rule():
    seen_t, seen_s = set(), set()
    for name in NAMES:
        seen_t |= set(GOLDEN[f"{name}/transitions"].ravel().tolist())
        seen_s |= set(GOLDEN[f"{name}/state"].ravel().tolist())
    assert seen_t == {0, 1, 2, 3, 4} and seen_s == {0, 1, 2, 3}
    assert (GOLDEN["jumped_ring/state"] == 0).all() and GOLDEN["jumped_ring/mask"].any()  # inside for ticks, never captured
    assert bub.HIJACKED not in GOLDEN["inside_at_start/state"]
    # a shadowed vehicle that a full bubble does not admit rides through SHADOWED: inside the inner zone, no Entered
    st, cur = GOLDEN["hijack_limit_1/state"], GOLDEN["hijack_limit_1/cursors"]
    assert ((st[:, 0] == bub.HIJACKED) & (st[:, 1] == bub.SHADOWED)).sum() >= 6 and (cur[:, 1, 0] == bub.C_NONE).sum() > 10


@pytest.mark.parametrize("name", ["loop", "4lane"])
def test_the_gpu_cases_show_what_they_are_there_for(name, compiled_maps):
    """Every case of tests/test_gpu_history_bubbles.py on the model alone: the clearance from the edges, and each case's
    own expectations (the through drive, the jumped ring, both outcomes of hijack_limit = 1, ...)."""
    cm = compiled_maps(name)
    sc = bub.scene(cm)
    for case in bub.CASES.values():
        m, hist = bub.run_model(case, sc, 0)
        assert m.clearance >= bub.CLEARANCE, (case.name, m.clearance)
        case.expect(hist, m)
    case = bub.case_wide()
    m, hist = bub.run_model(case, bub.wide_scene(cm), 0, envs=bub.WIDE_E, agents=bub.WIDE_AGENTS)
    assert m.clearance >= bub.CLEARANCE
    case.expect(hist, m)
    # case 7's foil: without the rotation the travelling bubble decides otherwise
    case = bub.CASES["travelling"]
    _, turned = bub.run_model(case, sc, 0)
    _, flat = bub.run_model(case, sc, 0, rotate=False)
    assert sum(int((a["state"] != b["state"]).sum()) for a, b in zip(turned, flat)) >= 1


def test_the_descriptors_refuse_what_the_reference_refuses():
    from smarts_amd.env import Bubble, BubbleLimits, MapZone, PositionalZone

    zone = PositionalZone(pos=(1.0, 2.0), size=(8.0, 4.0))
    with pytest.raises(ValueError, match="margin must be greater than 0"):
        Bubble(zone=zone, margin=0)
    with pytest.raises(ValueError, match="follow offset must be set"):
        Bubble(zone=zone, follow_actor_id="Agent-history-vehicle-1")
    with pytest.raises(ValueError, match="Only boids can have keep_alive"):
        Bubble(zone=zone, keep_alive=True)
    with pytest.raises(ValueError, match="Shadow limit must be >= hijack limit"):
        BubbleLimits(hijack_limit=3, shadow_limit=2)
    with pytest.raises(ValueError, match="Shadow limit must be >= hijack limit"):
        BubbleLimits(hijack_limit=None, shadow_limit=2)
    with pytest.raises(ValueError, match="non-negative"):
        BubbleLimits(hijack_limit=1, shadow_limit=None)
    assert BubbleLimits() == BubbleLimits(maxsize, maxsize)
    with pytest.raises(NotImplementedError, match="PositionalZone"):
        Bubble(zone=MapZone(start=("edge", 0, 5.0), length=20.0)).to_native(lambda name: 0)
    boid = type("BoidAgentActor", (), {})()
    with pytest.raises(NotImplementedError, match="boid"):
        Bubble(zone=zone, actor=boid, keep_alive=True).to_native(lambda name: 0)
    b = Bubble(zone=zone, margin=1.5, limit=BubbleLimits(2, 5), follow_actor_id="x", follow_offset=(0.5, 8.0)).to_native(lambda name: 3)
    assert (b.x, b.y, b.size_x, b.size_y, b.margin, b.offset_x, b.offset_y) == (1.0, 2.0, 8.0, 4.0, 1.5, 0.5, 8.0)
    assert (b.follow_agent, b.hijack_limit, b.shadow_limit) == (3, 2, 5)
    b = Bubble(zone=zone).to_native(lambda name: 0)
    assert (b.follow_agent, b.hijack_limit, b.shadow_limit, b.margin) == (-1, 0, 0, 2.0)  # no limit: none on the device


def _config(nat, E=4, N=8, S=4):
    cfg = nat.SmxConfig()
    cfg.num_envs, cfg.num_vehicles, cfg.num_social, cfg.dt = E, N, S, 0.1
    cfg.action_space = nat.ACTION_SPACES["Imitation"]
    return cfg


def _check(nat, lib, cfg, bubbles, state=32, cursor=32, rows=True, n=None, null_bubbles=False):
    hb = nat.SmxHistoryBubbles()
    host = (nat.SmxBubble * max(len(bubbles), 1))(*bubbles)
    hb.bubbles_host = None if null_bubbles else host
    hb.n_bubbles = len(bubbles) if n is None else n
    keep = np.zeros(8, dtype=np.uint8)  # (host memory stands in for the device rows: the check reads no element)
    hb.state_dev = hb.cursor_dev = keep.ctypes.data if rows else None
    hb.state_count, hb.cursor_count = state, cursor
    err = C.create_string_buffer(512)
    return lib.smx_check_history_bubbles(C.byref(cfg), C.byref(hb), err, len(err)), err.value.decode()


def test_check_history_bubbles():
    from smarts_amd import _native as nat

    lib = nat.load_library()
    assert C.sizeof(nat.SmxBubble) == 72 and C.sizeof(nat.SmxHistoryBubbles) == 48
    assert (nat.HA_SHADOWED, nat.HA_RELEASED, nat.MAX_BUBBLES) == (4, 5, 8)
    assert (nat.BUBBLE_SOCIAL, nat.BUBBLE_SHADOWED, nat.BUBBLE_HIJACKED, nat.BUBBLE_RELEASED) == (0, 1, 2, 3)
    cfg = _config(nat)
    good = bub.B(x=1.0, y=2.0, size_x=8.0, size_y=4.0, margin=2.0, hijack_limit=1, shadow_limit=2)
    ok = lambda **kw: bub.B(**{**good.__dict__, **kw}).native()  # noqa: E731
    assert _check(nat, lib, cfg, [good.native()]) == (0, "")
    assert _check(nat, lib, cfg, [good.native()] * 8) == (0, "")
    assert _check(nat, lib, cfg, [ok(follow=3, offset=(0.0, 8.0)), ok(hijack_limit=0, shadow_limit=0), ok(hijack_limit=0, shadow_limit=2)]) == (0, "")
    refused = [
        (dict(bubbles=[]), "n_bubbles"), (dict(bubbles=[good.native()] * 9), "n_bubbles"), (dict(bubbles=[good.native()], n=-1), "n_bubbles"),
        (dict(bubbles=[good.native()], null_bubbles=True), "bubbles_host"),
        (dict(bubbles=[ok(x=float("nan"))]), "not finite"), (dict(bubbles=[ok(offset=(float("inf"), 0.0))]), "not finite"),
        (dict(bubbles=[ok(size_x=0.0)]), "size"), (dict(bubbles=[ok(size_y=-1.0)]), "size"), (dict(bubbles=[ok(margin=0.0)]), "margin"),
        (dict(bubbles=[good.native(), ok(follow=4)]), "follow_agent"), (dict(bubbles=[ok(hijack_limit=-1)]), "negative"),
        (dict(bubbles=[ok(shadow_limit=-2)]), "negative"), (dict(bubbles=[ok(hijack_limit=3, shadow_limit=2)]), "shadow_limit"),
        (dict(bubbles=[good.native()], rows=False), "NULL"), (dict(bubbles=[good.native()], state=31), "state"),
        (dict(bubbles=[good.native()], cursor=31), "cursor"),
    ]
    for kw, word in refused:
        rc, why = _check(nat, lib, cfg, **kw)
        assert rc == -1 and word in why, (kw, rc, why)
    assert _check(nat, lib, _config(nat, N=4, S=4), [good.native()])[0] == -1  # no agent slot
    assert lib.smx_check_history_bubbles(None, None, None, 0) == -1
    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_set_history_bubbles(smx_handle h, const smx_history_bubbles* hb);" in header
    assert "enum { SMX_HA_SHADOWED = 4, SMX_HA_RELEASED = 5 };" in header and "#define SMX_MAX_BUBBLES 8" in header
    assert "smx_set_history_bubbles" in nat.EXPORTS and "smx_check_history_bubbles" in nat.EXPORTS

"""The dimensions of replayed vehicles on the host (smarts_amd/traffic_history.py): ``TrafficHistoryTable.device_dims``
/ ``resolved_dimensions`` against the reference's rule, whose results for the same ``Vehicle`` rows are the fixture
tests/golden/traffic_history_dims.json (gen_golden_traffic_history_dims.py wrote it with the reference's own
``Dimensions.init_with_defaults`` over ``VEHICLE_CONFIGS``)."""
import json
import os

import numpy as np
import pytest

import traffic_history_dims_ref as ref
from oracle.sim import boxes_within
from smarts_amd.traffic_history import PASSENGER_DIMENSIONS, TrafficHistoryTable, resolve_dimensions

HERE = os.path.dirname(os.path.abspath(__file__))
DT = 0.1


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "traffic_history_dims.json")) as f:
        return json.load(f)


def _table(vehicle_rows, present=None, slots=None):
    """Every vehicle of ``present`` (default: all) in frame 0 of its own slot."""
    ids = [int(r[0]) for r in vehicle_rows] if present is None else list(present)
    traj = [(vid, 0.0, 1.0 * i, 2.0, 0.0, 0.0) for i, vid in enumerate(ids)]
    return TrafficHistoryTable.from_rows(vehicle_rows, traj, DT, slots or len(ids))


def test_the_fixture_covers_the_rule(golden):
    rows = golden["rows"]
    for k in range(3):  # each "no value" spelling in each component
        for missing in (None, 0, -1):
            assert any(r[2 + k] == missing and type(r[2 + k]) is type(missing) for r in rows), (k, missing)
    assert {1, 2, 3, 4} <= {r[1] for r in rows} and any(r[1] not in (1, 2, 3, 4) for r in rows)
    assert golden["passenger"] == list(PASSENGER_DIMENSIONS)


def test_device_dims_is_the_references_rule(golden):
    rows, want = golden["rows"], golden["resolved"]
    table = _table(rows)
    dims = table.device_dims()
    top = max(r[0] for r in rows)
    assert dims.shape == (top + 1, 3) and dims.dtype == np.float64
    for r, w in zip(rows, want):
        assert dims[r[0]].tolist() == w, (r, dims[r[0]], w)  # exactly: values are copied, never computed
        assert list(table.resolved_dimensions(r[0])) == w
        assert list(resolve_dimensions(*r[1:])) == w
    # an id that never occurs in the table holds the passenger default
    never = sorted(set(range(top + 1)) - {r[0] for r in rows})
    assert never and all(dims[v].tolist() == golden["passenger"] for v in never)
    assert np.isfinite(dims).all() and (dims > 0).all()


def test_a_vehicle_with_a_row_but_no_sample_holds_the_passenger_default(golden):
    rows = golden["rows"]
    trailer = next(r for r in rows if r[2:4] == [10.0, 2.5])
    others = [r[0] for r in rows if r[0] < trailer[0]]
    table = _table(rows, present=others)  # the trailer is in the Vehicle rows and never in a frame
    dims = table.device_dims()
    assert dims.shape[0] == max(others) + 1  # n_ids = the largest id that OCCURS + 1
    assert table.resolved_dimensions(trailer[0])[:2] == (10.0, 2.5)  # (asked by id it still resolves)


def test_dimensions_keeps_the_raw_dataset_tuple(golden):
    rows = golden["rows"]
    table = _table(rows)
    for r in rows:
        raw = table.dimensions(r[0])
        assert raw == tuple(None if v is None else float(v) for v in r[2:5]), (r, raw)
    assert any(None in table.dimensions(r[0]) for r in rows)
    assert table.types[rows[0][0]] == rows[0][1]


def test_the_plain_constructor_resolves_to_the_passenger_default():
    frames = np.zeros((2, 2, 4))
    vehicle = np.array([[4, -1], [4, 9]], dtype=np.int32)
    table = TrafficHistoryTable(frames, vehicle, DT)
    dims = table.device_dims()
    assert dims.shape == (10, 3) and (dims == np.asarray(PASSENGER_DIMENSIONS)).all()
    assert table.resolved_dimensions(9) == PASSENGER_DIMENSIONS
    empty = TrafficHistoryTable(frames, np.full((2, 2), -1, dtype=np.int32), DT)
    assert empty.device_dims().tolist() == [list(PASSENGER_DIMENSIONS)]  # n_ids >= 1 always


def test_ids_above_2_pow_20_are_refused():
    ok = _table([(1 << 20, 2, None, None, None)])
    assert ok.device_dims().shape == ((1 << 20) + 1, 3)
    big = _table([((1 << 20) + 1, 3, 5.0, 2.0, None)])
    with pytest.raises(ValueError, match="renumber"):
        big.device_dims()
    assert big.resolved_dimensions((1 << 20) + 1) == (5.0, 2.0, 1.89)  # (the host rule itself has no such limit)


def test_the_gpu_tests_scene_proves_itself(compiled_maps):
    """tests/traffic_history_dims_ref.py ``scene``, before any device run.  Abreast of the standing trailer, both parallel to the lane: the sedan pair is apart, the trailer pair touches
    (oracle.sim.boxes_within); and the table resolves the mixed types and sizes the other tests rely on."""
    for name in ("loop", "4lane"):
        cm = compiled_maps(name)
        sc = ref.scene(cm)
        agent, trailer, sedan = ref.closest_pass(cm, sc)
        assert boxes_within(agent, trailer, ref.LEEWAY) and not boxes_within(agent, sedan, ref.LEEWAY), name
        # by the numbers: centres 1.9 m apart across the heading; half widths 0.735 + 1.25 overlap by 0.085 m, two
        # sedans' 0.735 + 0.735 leave 0.43 m, beyond the 0.05 m leeway
        dx, dy = trailer.x - agent.x, trailer.y - agent.y
        assert abs(np.hypot(dx, dy) - ref.SIDE) < 1e-9 and agent.heading == trailer.heading
        table = sc["table"]
        assert ref.slot_of(table, ref.MOTORCYCLE) == ref.slot_of(table, ref.LATE_TRAILER)  # the reused slot
        assert table.resolved_dimensions(ref.TRAILER) == (10.0, 2.5, 4.0)
        assert table.resolved_dimensions(ref.MOTORCYCLE) == (2.5, 1.0, 1.4)
        assert table.resolved_dimensions(ref.LATE_TRAILER) == (10.0, 2.5, 1.89)
        assert table.resolved_dimensions(ref.PEDESTRIAN) == (0.5, 0.5, 1.6)
        assert table.resolved_dimensions(ref.TRUCK) == (5.0, 1.91, 1.89)

"""The device-free half of the C-ABI, message for message (smarts_amd/csrc/smx_host.h behind the smx_check_* entry points
and smx_create's validation).

tests/golden/host_checks.json holds what the library answered — return code and message — to the sweep of
tests/golden/gen_golden_host_checks.py when the fixture was recorded; the same sweep is replayed here against the built
library and both fields are compared for equality, case by case.  No device is needed."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_golden_host_checks", os.path.join(GOLDEN, "gen_golden_host_checks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_checks_answer_as_recorded():
    from smarts_amd import _native as nat

    gen = _generator()
    assert os.path.getsize(gen.FIXTURE) <= 146 * 1024  # no larger than the largest fixture committed before it
    golden = json.load(open(gen.FIXTURE))
    messages, cases = golden["messages"], golden["cases"]
    got = list(gen.sweep(nat.load_library()))
    assert len(got) == len(cases) and len(cases) > 5000
    wrong = [(label, (rc, msg), (want_rc, messages[want_msg]))
             for (label, rc, msg), (want_rc, want_msg) in zip(got, cases) if (rc, msg) != (want_rc, messages[want_msg])]
    assert not wrong, (len(wrong), wrong[:5])
    # the sweep reaches what it is meant to: accepted and refused cases of every entry point, the asymmetry between the
    # entry check (sized by the shape numbers) and the frame stack (asks whether the sensor is on)
    by_label = {label: (rc, msg) for label, rc, msg in got}
    for part in ("buffers", "stack", "rgb", "guard", "goals", "create"):
        codes = {rc for label, (rc, _) in by_label.items() if label.startswith(part + "/")}
        assert 0 in codes and -1 in codes, (part, codes)
    assert by_label["buffers/everything/vias1/exact"] == (0, "") and by_label["buffers/oversized/vias1/exact"] == (0, "")
    rc, msg = by_label["buffers/oversized/vias0/wp_pos/short"]
    assert rc == -1 and msg.startswith("out.wp_pos: ")
    assert by_label["buffers/oversized/vias0/rw_pos/short"] == (0, "")
    wp_pos = nat.OUTPUT_BUFFERS.index("wp_pos")
    assert by_label[f"stack/everything/k2/src{wp_pos}/layout0/exact"] == (0, "")
    rc, msg = by_label[f"stack/oversized/k2/src{wp_pos}/layout0/exact"]
    assert rc == -1 and "is off in this configuration" in msg

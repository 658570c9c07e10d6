#!/usr/bin/env python3
"""Golden vectors of an agent's own vehicle dimensions and of its start pose, from the reference's OWN
``Vehicle.agent_vehicle_dims`` (smarts/core/vehicle.py:339-357: the mission's ``vehicle_spec`` dimensions over the
defaults of its config type, through ``Dimensions.copy_with_defaults``, or the passenger's without a spec) and
``Pose.from_front_bumper`` (smarts/core/coordinates.py:302-321: the centre of a vehicle whose front bumper stands at a
mission's start, half its own length behind it).

Same import shim as ``gen_golden.py`` (which see): runs only where the reference tree is; the suite consumes the
committed ``tests/golden/agent_dims.json`` (data only).  A mission here is a stand-in with the one attribute the function
reads (``vehicle_spec``: ``None``, or ``veh_config_type`` and ``dimensions``); the ``Dimensions`` are the reference's.

The fixture: ``specs`` — ``null`` (no vehicle_spec) or (length, width, height) with ``null`` where the spec gives none —
and ``resolved``, the (length, width, height) of each, in the same order: every "no value" spelling (None, 0, -1, 0.0,
-1.0) in each component, nothing given, everything given, the trailer's 10 x 2.5 x 4.  ``bumper``: (x, y, heading, length)
and the centre (x, y) ``Pose.from_front_bumper`` gives, at three lengths.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_agent_dims.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden as gg  # noqa: E402


def specs():
    out = [None]  # a mission without a vehicle_spec
    for missing in (None, 0, -1, 0.0, -1.0):
        for k in range(3):
            dims = [6.5, 2.2, 2.9]
            dims[k] = missing
            out.append(dims)
    out.append([None, None, None])
    out.append([2.5, 1.0, 1.4])
    out.append([10.0, 2.5, 4.0])
    out.append([10.0, 2.5, None])
    return out


BUMPERS = [(12.5, -3.25, 0.0, 3.68), (101.0, 57.5, 1.25, 10.0), (-40.75, 8.0, -2.6, 2.5)]


def main():
    gg.install_reference()
    import numpy as np
    from smarts.core.coordinates import Dimensions, Heading, Pose
    from smarts.core.vehicle import VEHICLE_CONFIGS, Vehicle

    resolved = []
    for spec in specs():
        vs = None if spec is None else types.SimpleNamespace(veh_config_type="passenger", dimensions=Dimensions(*spec))
        d = Vehicle.agent_vehicle_dims(types.SimpleNamespace(vehicle_spec=vs))
        resolved.append([float(d.length), float(d.width), float(d.height)])
    centres = []
    for x, y, heading, length in BUMPERS:
        pose = Pose.from_front_bumper(np.array([x, y]), Heading(heading), length)
        centres.append([float(pose.position[0]), float(pose.position[1]), float(pose.heading)])
    data = dict(specs=specs(), resolved=resolved, passenger=[float(v) for v in VEHICLE_CONFIGS["passenger"].dimensions.as_lwh],
                bumper=[list(b) for b in BUMPERS], centre=centres)
    path = os.path.join(gg.OUT, "agent_dims.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print(len(resolved), "specs", len(centres), "poses", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

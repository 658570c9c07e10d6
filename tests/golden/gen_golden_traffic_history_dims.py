#!/usr/bin/env python3
"""Golden vectors of the dimensions a replayed vehicle gets, from the reference's OWN ``Dimensions.init_with_defaults``
(smarts/core/coordinates.py:55-66) over ``VEHICLE_CONFIGS`` (smarts/core/vehicle.py:97-140), keyed by the dataset type as
``TrafficHistory.decode_vehicle_type`` maps it (smarts/core/traffic_history.py:127-146) — what
``TrafficHistoryProvider.step`` hands out per vehicle (traffic_history_provider.py:112-126).

Same import shim as ``gen_golden.py`` (which see): runs only where the reference tree is; the suite consumes the
committed ``tests/golden/traffic_history_dims.json`` (data only).  ``coordinates.py`` and ``vehicle.py``'s table import
without Bullet here, so no triple of the fixture was copied by hand.  ``decode_vehicle_type`` is a method of a class
that opens a dataset file; it is called unbound on a stand-in that has a logger.

The fixture: ``rows`` — (id, type, length, width, height) with ``null`` where the dataset has NULL — and ``resolved``, the
(length, width, height) of each row, in the same order.  Rows: each of None / 0 / -1 in each component over a type with a
non-passenger default; types 1-4 and two unknown ones without any value; full and partial dataset values.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_traffic_history_dims.py
"""
import json
import logging
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden as gg  # noqa: E402


def rows():
    out = []
    vid = 3
    for missing in (None, 0, -1, 0.0, -1.0):  # each "no value" spelling, per component, over the truck's defaults
        for k in range(3):
            dims = [6.5, 2.2, 2.9]
            dims[k] = missing
            out.append((vid, 3, *dims))
            vid += 2
    for vtype in (1, 2, 3, 4, 0, 5, 99):  # nothing given: the type's default (unknown types: the passenger's)
        out.append((vid, vtype, None, None, None))
        vid += 3
    out.append((vid, 1, 2.1, 0.8, 1.2))  # everything given
    out.append((vid + 1, 4, None, 0.6, -1))
    out.append((vid + 2, 3, 10.0, 2.5, None))  # a trailer-sized truck: NGSIM gives length and width, never the height
    out.append((vid + 3, 7, 4.5, 0, 0))
    return out


def main():
    gg.install_reference()
    from smarts.core.coordinates import Dimensions
    from smarts.core.traffic_history import TrafficHistory
    from smarts.core.vehicle import VEHICLE_CONFIGS

    stand_in = types.SimpleNamespace(_log=logging.getLogger("gen_golden_traffic_history_dims"))
    resolved = []
    for vid, vtype, length, width, height in rows():
        config_type = TrafficHistory.decode_vehicle_type(stand_in, vtype)
        d = Dimensions.init_with_defaults(length, width, height, defaults=VEHICLE_CONFIGS[config_type].dimensions)
        resolved.append([float(d.length), float(d.width), float(d.height)])
    data = dict(rows=[list(r) for r in rows()], resolved=resolved,
                passenger=[float(v) for v in VEHICLE_CONFIGS["passenger"].dimensions.as_lwh])
    path = os.path.join(gg.OUT, "traffic_history_dims.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print(len(resolved), "rows", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""The map's knot table without a device (smarts_amd/csrc/smx_roadmap.h: KnotRow, build_knot_row, knot_row_serves).

tests/native/host_knot_table.cpp — a stand-alone program with its own main, built with AddressSanitizer + UBSan over
the shim hip_runtime.h — builds the row of every lanepoint of the three shipped maps at lookaheads 16 and 32 and holds
it to plain walks: the list, the chained D bit for bit from three query points, and the junction-filter rule.  The
compiled tables reach it through a file per map."""
import ctypes as C
import json
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
MAPS = {"loop": "loop", "4lane": "intersections/4lane", "minicity": "minicity"}
# SMX_MAP_TABLES (smx_host.h): the order the program reads the tables in
TABLES = ["lane_road", "lane_index", "lane_width", "lane_speed", "lane_length", "lane_in_junction", "lane_shape_off", "shape_x",
          "shape_y", "shape_rec", "lane_out_off", "lane_out_idx", "lane_in_off", "lane_in_idx", "road_par_off", "road_par_idx",
          "road_lane_off", "road_lanes", "road_is_junction", "road_out_road", "lp_rec", "succ_rec", "lpg_off", "lpg_pts", "sg_off",
          "sg_rec"]


def _write_tables(name, path):
    from smarts_amd.map_compiler import compile_map, map_tables_struct
    from smarts_amd.sumo_map import load_net

    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", MAPS[name])))
    t, keep = map_tables_struct(cm)
    by_address = {a.ctypes.data: a for a in keep}
    with open(path, "wb") as f:
        f.write(bytes(t))
        for field in TABLES:
            arr = by_address[getattr(t, field)]
            f.write(struct.pack("<Q", arr.nbytes))
            f.write(arr.tobytes())
    return cm


def test_knot_rows_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_knot_table")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(NATIVE, "shim"), "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_knot_table.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    files, lanepoints = [], []
    for name in MAPS:
        files.append(str(tmp_path / f"{name}.tables"))
        lanepoints.append(_write_tables(name, files[-1]).n_lanepoints)
    # (the sanitizer runtime is linked into the program itself: the environment is inherited as it is)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, proc.stderr[-3000:]
    res = json.loads(proc.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    assert proc.returncode == 0, res
    assert (res["bad_list"], res["bad_D"], res["bad_rule2"]) == (0, 0, 0), res
    assert res["maps"] == 3 and res["rows"] == 2 * sum(lanepoints)
    assert res["checks"] > res["rows"] + 3 * res["tabled"]
    assert res["rule2_uses"] > 0  # the junction-filter rule is exercised
    # a row is 256 bytes
    for m in res["per_map"]:
        assert m["bytes"] == 256 * m["rows"] and 0 < m["tabled"] <= m["rows"]

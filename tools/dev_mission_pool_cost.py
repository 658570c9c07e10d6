"""Developer: what a mission pool's tick costs, per tick on one MI355X (include/smx.h smx_set_mission_pool).
4lane, 4096 envs x 4 agents, bench.py's sensors (waypoints 4 x 20, neighbours 10 within 50 m), auto_reset on, every agent
at the start of a fixed route through the junction (the four missions of tests/test_gpu_missions.py), keep_lane.  Two
settings of the same shape:
    per_slot   smx_set_missions: slot a flies mission a in every env and episode
    pool       smx_set_mission_pool: a pool of the same four missions and a table of one row that gives slot a of every
               env mission a — the same work, read through the table
Each run is a fresh process: reset, `ticks` ticks timed at level 1 (the median tick).  Runs alternate over the settings.
    python tools/dev_mission_pool_cost.py [runs [ticks]]            (default 3 runs of each, 200 ticks)
    python tools/dev_mission_pool_cost.py --one SETTING [ticks]
Part (b) of profiles/r28_mission_pool_cost.txt is its output."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, N = 4096, 4
SETTINGS = ["per_slot", "pool"]


def one(setting, ticks=200):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from smarts_amd.engine import BatchedSim, SimConfig
    from smarts_amd.map_compiler import compile_map
    from smarts_amd.missions import Mission, Route, plan_mission
    from smarts_amd.sumo_map import load_net

    _, _scenario, kw = bench.workload_config("c2", envs=E, vehicles=N)
    net = load_net(os.path.join(ROOT, "smarts_amd", "scenarios", "intersections", "4lane"))
    cm = compile_map(net)
    routes = [Route(begin=("edge-north-NS", 0, 40), end=("edge-east-WE", 0, 30)),
              Route(begin=("edge-west-WE", 1, 60), end=("edge-east-WE", 1, 12)),
              Route(begin=("edge-south-SN", 0, 55), end=("edge-west-EW", 0, "max")),
              Route(begin=("edge-east-EW", 1, 10), end=("edge-east-EW", 1, 40))]
    missions = [plan_mission(net, Mission(r)) for r in routes]
    spawns = np.zeros((1, E * N, 4))
    for a, m in enumerate(missions):
        spawns[0, a::N] = (*m.spawn_pose(), 8.0)
    sim = BatchedSim(cm, SimConfig(**kw), spawns=spawns, missions=missions if setting == "per_slot" else None)
    if setting == "pool":
        rows = torch.arange(N, dtype=torch.int32, device=sim.device).repeat(1, E, 1).contiguous()
        sim.set_mission_pool(missions, None, rows)
    acts = torch.zeros((E, N), dtype=torch.int8, device=sim.device)
    sim.reset()
    sim.set_timing(1)
    for _ in range(ticks):
        sim.step(acts)
    torch.cuda.synchronize()
    ms = np.asarray(sim.read_step_ms())
    sim.set_timing(0)
    sim.sync()
    res = {"setting": setting, "ms": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
           "ms_p90": round(float(np.percentile(ms, 90)), 4), "episodes": int(sim.env_episode.sum()), "form": sim.launch_form(), "ticks": ticks}
    sim.close()
    print(json.dumps(res))


def main(runs=3, ticks=200):
    rows = []
    for r, setting in enumerate(SETTINGS * runs):
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", setting, str(ticks)], capture_output=True,
                              text=True, timeout=300)
        if proc.returncode != 0:  # nothing more is started after a run that failed
            sys.exit(f"run {r} {setting}: exit {proc.returncode}\n{proc.stderr[-2000:]}")
        row = json.loads(proc.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        rows.append(row)
    med = {s: statistics.median(r["ms"] for r in rows if r["setting"] == s) for s in SETTINGS}
    spread = {s: round(max(r["ms"] for r in rows if r["setting"] == s) - min(r["ms"] for r in rows if r["setting"] == s), 4) for s in SETTINGS}
    print(json.dumps({"median_ms": med, "max_minus_min_ms": spread, "pool_over_per_slot": round(med["pool"] / med["per_slot"], 4)}))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    else:
        main(*(int(a) for a in sys.argv[1:3]))

"""Developer: a replayed history with the per-vehicle dimensions bound against the same history without them, per tick on
one MI355X (include/smx.h smx_set_social_history_dims).  The sim, the recording and the timing are
tools/dev_history_cost.py's: bench.py's configs[3] shape with num_social = 8, every env walking env 0's episode, the
history recorded from a scripted run.  The recorded table has no Vehicle rows, so every vehicle resolves to the passenger
default 3.68 x 1.47 x 1.4: the sedan's footprint — both settings walk the same episode, the driver checks the alive
counts — read through the per-slot triples by every consumer, which is what is timed.  Runs alternate, without the
dimensions first, `runs` of each; every run is a process of its own; the median level-1 tick of a run.
    python tools/dev_history_dims_cost.py [runs [ticks [warmup]]]     (default 3 runs of each, 100 ticks after 20 warm-up ticks)
    python tools/dev_history_dims_cost.py --one history|dims TABLE.npz [ticks [warmup]]
profiles/r17_vehicle_dims_cost.txt was made with it."""
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SOCIAL = 8


def one(setting, path, ticks=100, warm=20):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns
    from smarts_amd.map_compiler import compile_map
    from smarts_amd.sumo_map import load_net
    from smarts_amd.traffic_history import TrafficHistoryTable

    _, scenario, kw = bench.workload_config("c4")
    E, N = kw["num_envs"], kw["num_vehicles"]
    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", scenario)))
    spawns, where = make_spawns(cm, 1, N, episodes=1, seed=42, return_lanes=True)
    spawns, where = np.tile(spawns, (1, E, 1)), np.tile(where, (1, E, 1))
    actions = torch.from_numpy(np.tile(bench.action_stream(1, N, 42, 0), (1, E, 1))).cuda()
    sim = BatchedSim(cm, SimConfig(num_social=SOCIAL, **kw), spawns=spawns, social_spawns=where)
    rec = np.load(path)
    sim.set_traffic_history(TrafficHistoryTable(rec["frames"], rec["vehicle"], kw["dt"]), dims=setting == "dims")
    sim.reset()
    for i in range(warm):
        sim.step(actions[i % bench.ACTION_CYCLE])
    sim.set_timing(1)
    for i in range(warm, warm + ticks):
        sim.step(actions[i % bench.ACTION_CYCLE])
    torch.cuda.synchronize()
    ms = np.asarray(sim.read_step_ms())
    sim.set_timing(0)
    agents = sim.flags[:, :N - SOCIAL]
    res = {"history": setting, "ms": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
           "agents_alive_after": int((agents & 1).sum()), "episodes": int(sim.env_episode.max()),
           "shape": f"{scenario} {E} x {N}, {SOCIAL} social", "form": sim.lib.smx_launch_form(sim.handle), "ticks": ticks, "warmup": warm}
    sim.close()
    print(json.dumps(res))


def main(runs=3, ticks=100, warm=20):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "recorded.npz")
        jobs = [(os.path.join(HERE, "dev_history_cost.py"), "record")] + [(os.path.abspath(__file__), s) for s in ["history", "dims"] * runs]
        for r, (tool, setting) in enumerate(jobs):
            proc = subprocess.run([sys.executable, tool, "--one", setting, path, str(ticks), str(warm)],
                                  capture_output=True, text=True, timeout=300)
            if proc.returncode != 0:  # nothing more is started after a run that failed
                sys.exit(f"run {r} {setting}: exit {proc.returncode}\n{proc.stderr[-2000:]}")
            row = json.loads(proc.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            if setting != "record":
                rows.append(row)
    plain = [r["ms"] for r in rows if r["history"] == "history"]
    dims = [r["ms"] for r in rows if r["history"] == "dims"]
    same = len({(r["agents_alive_after"], r["episodes"]) for r in rows}) == 1
    m_p, m_d = statistics.median(plain), statistics.median(dims)
    print(json.dumps({"history_ms": plain, "dims_ms": dims, "median_history": m_p, "median_dims": m_d,
                      "dims_over_history": round(m_d / m_p, 4), "same_episode": same}))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], sys.argv[3], *(int(a) for a in sys.argv[4:6]))
    else:
        main(*(int(a) for a in sys.argv[1:4]))

"""Developer: a following tick (smx_step_history_agents) against a tick of smx_step_continuous with no action, on the
same bound history and the same follow table, per tick on one MI355X (include/smx.h smx_set_history_agents).  The sim and
the recording are tools/dev_history_cost.py's — bench.py's configs[3] shape with num_social = 8, every env walking env
0's episode, the history recorded from a scripted run — as an Imitation sim: of the 24 agent slots of an env the first
FOLLOWERS follow the recorded vehicles 0 .. FOLLOWERS - 1, the others follow nothing (eight slots hold at most eight
vehicles, and half of them stay social vehicles).  "follow" moves the followers along the recording; "nan" leaves them
where the reset put them while the rest of the tick — the replayed slots, every sensor — runs the same, so the two
settings do not walk the same episode: the alive counts are printed beside the times.  Runs alternate, "nan" first, `runs`
of each; every run is a process of its own; the median level-1 tick of a run.
    python tools/dev_history_agents_cost.py [runs [ticks [warmup]]]     (default 3 runs of each, 60 ticks after 10 warm-up ticks)
    python tools/dev_history_agents_cost.py --one nan|follow TABLE.npz [ticks [warmup]]
profiles/r18_history_agents_cost.txt was made with it."""
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SOCIAL = 8
FOLLOWERS = 4


def one(setting, path, ticks=60, warm=10):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns
    from smarts_amd.map_compiler import compile_map
    from smarts_amd.sumo_map import load_net
    from smarts_amd.traffic_history import TrafficHistoryTable

    _, scenario, kw = bench.workload_config("c4")
    kw = dict(kw, action_space="Imitation")
    E, N = kw["num_envs"], kw["num_vehicles"]
    A = N - SOCIAL
    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", scenario)))
    spawns, where = make_spawns(cm, 1, N, episodes=1, seed=42, return_lanes=True)
    spawns, where = np.tile(spawns, (1, E, 1)), np.tile(where, (1, E, 1))
    sim = BatchedSim(cm, SimConfig(num_social=SOCIAL, **kw), spawns=spawns, social_spawns=where)
    rec = np.load(path)
    sim.set_traffic_history(TrafficHistoryTable(rec["frames"], rec["vehicle"], kw["dt"]))
    follow = np.full((1, E, A), -1, dtype=np.int32)
    follow[0, :, :FOLLOWERS] = np.arange(FOLLOWERS)
    sim.set_history_agents(torch.from_numpy(follow).cuda())
    none = torch.full((E, N, 3), float("nan"), dtype=torch.float32).cuda()
    tick = sim.step_history_agents if setting == "follow" else (lambda: sim.step(none))
    sim.reset()
    for i in range(warm):
        tick()
    sim.set_timing(1)
    for i in range(ticks):
        tick()
    torch.cuda.synchronize()
    ms = np.asarray(sim.read_step_ms())
    sim.set_timing(0)
    res = {"tick": setting, "ms": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
           "agents_alive_after": int((sim.flags[:, :A] & 1).sum()), "social_alive_after": int((sim.flags[:, A:] & 1).sum()),
           "episodes": int(sim.env_episode.max()), "shape": f"{scenario} {E} x {N}, {SOCIAL} social, {FOLLOWERS} followers",
           "form": sim.lib.smx_launch_form(sim.handle), "ticks": ticks, "warmup": warm}
    sim.close()
    print(json.dumps(res))


def main(runs=3, ticks=60, warm=10):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "recorded.npz")
        jobs = [(os.path.join(HERE, "dev_history_cost.py"), "record", ["100", "20"])]
        jobs += [(os.path.abspath(__file__), s, [str(ticks), str(warm)]) for s in ["nan", "follow"] * runs]
        for r, (tool, setting, args) in enumerate(jobs):
            proc = subprocess.run([sys.executable, tool, "--one", setting, path] + args, capture_output=True, text=True, timeout=300)
            if proc.returncode != 0:  # nothing more is started after a run that failed
                sys.exit(f"run {r} {setting}: exit {proc.returncode}\n{proc.stderr[-2000:]}")
            row = json.loads(proc.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            if setting != "record":
                rows.append(row)
    nan = [r["ms"] for r in rows if r["tick"] == "nan"]
    follow = [r["ms"] for r in rows if r["tick"] == "follow"]
    m_n, m_f = statistics.median(nan), statistics.median(follow)
    print(json.dumps({"nan_ms": nan, "follow_ms": follow, "median_nan": m_n, "median_follow": m_f, "follow_over_nan": round(m_f / m_n, 4)}))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], sys.argv[3], *(int(a) for a in sys.argv[4:6]))
    else:
        main(*(int(a) for a in sys.argv[1:4]))

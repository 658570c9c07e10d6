"""Developer: a mixed tick (smx_step_history_handover) against a following tick (smx_step_history_agents) on the same
bound history and follow table, per tick on one MI355X (include/smx.h smx_set_history_handover).  The sim and the
recording are tools/dev_history_agents_cost.py's — bench.py's configs[3] shape with num_social = 8 as an Imitation sim,
every env walking env 0's episode, of the 24 agent slots of an env the first four follow the recorded vehicles 0 .. 3.
Three kinds of tick:
    follow    step_history_agents
    none      step_history_handover with every H = -1: the same episode as "follow", the HANDOVER form of the kernel
    two       step_history_handover with H = 0 for the followers 0 and 1 and zero actions (no acceleration, no turn): they
              keep the speed and heading of their reset frame and drive straight on — off the road where it bends, where
              the default done criteria (done_off_road among them) end them — while the followers 2 and 3 stay on the
              recording; so "two" does not walk the episode of the other two: the alive counts are printed beside the
              times.
Runs alternate, "follow" first, `runs` of each; every run is a process of its own; the median level-1 tick of a run, and
the ratios against the following tick measured in the same job.
    python tools/dev_history_handover_cost.py [runs [ticks [warmup]]]     (default 3 runs of each, 60 ticks after 10 warm-up ticks)
    python tools/dev_history_handover_cost.py --one follow|none|two TABLE.npz [ticks [warmup]]
profiles/r20_history_handover_cost.txt was made with it."""
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
DRIVEN = 2
KINDS = ("follow", "none", "two")


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
    handover = np.full((1, E, A), -1, dtype=np.int32)
    if setting == "two":
        handover[0, :, :DRIVEN] = 0
    sim.set_history_handover(torch.from_numpy(handover).cuda())
    zero = torch.zeros((E, N, 3), dtype=torch.float32).cuda()
    tick = sim.step_history_agents if setting == "follow" else (lambda: sim.step_history_handover(zero))
    sim.reset()
    for i in range(warm):
        tick()
    sim.set_timing(1)
    for i in range(ticks):
        tick()
    torch.cuda.synchronize()
    ms = np.asarray(sim.read_step_ms())
    sim.set_timing(0)
    sim.sync()
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
        jobs += [(os.path.abspath(__file__), s, [str(ticks), str(warm)]) for s in list(KINDS) * runs]
        for r, (tool, setting, args) in enumerate(jobs):
            proc = subprocess.run([sys.executable, tool, "--one", setting, path] + args, capture_output=True, text=True, timeout=300)
            if proc.returncode != 0:  # nothing more is started after a run that failed
                sys.exit(f"run {r} {setting}: exit {proc.returncode}\n{proc.stderr[-2000:]}")
            row = json.loads(proc.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            if setting != "record":
                rows.append(row)
    ms = {k: [r["ms"] for r in rows if r["tick"] == k] for k in KINDS}
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"ms": ms, "median": med, "none_over_follow": round(med["none"] / med["follow"], 4),
                      "two_over_follow": round(med["two"] / med["follow"], 4)}))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], sys.argv[3], *(int(a) for a in sys.argv[4:6]))
    else:
        main(*(int(a) for a in sys.argv[1:4]))

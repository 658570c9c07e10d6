"""Developer: what bubbles cost a mixed tick (smx_step_history_handover; include/smx.h smx_set_history_bubbles), per tick
on one MI355X.  The sim and the method are tools/dev_history_handover_cost.py's — bench.py's configs[3] shape with
num_social = 8 as an Imitation sim, every env walking env 0's episode, of the 24 agent slots of an env the first four
follow the recorded vehicles 0 .. 3.  Three settings of the same tick:
    none      a handover table with every H = -1 and no bubbles: the HANDOVER form of the control kernel
    one       no table, one fixed bubble without limits, 20 m x 20 m around the place vehicle 0 holds 25 frames in:
              k_bubbles, then the BUBBLES form
    eight     no table, eight bubbles with hijack_limit = 2 and shadow_limit = 4: seven fixed ones where the vehicles 0 .. 3
              are 15 .. 75 frames in, and one that travels 8 m ahead of agent slot 0
A hijacked follower is driven by zero actions (no acceleration, no turn) and drives straight on — off the road where it
bends, where the default done criteria end it — so the settings do not walk the same episode: the agents alive after
each run are printed beside the times (the alive count decides a tick's length more than a driven lane does,
profiles/r20_history_handover_cost.txt).
Runs alternate, "none" first, `runs` of each; every run is a process of its own; the median level-1 tick of a run, each
setting against "none", and the spread of the job beside it.
    python tools/dev_history_bubbles_cost.py [runs [ticks [warmup]]]     (default 3 runs of each, 60 ticks after 10 warm-up ticks)
    python tools/dev_history_bubbles_cost.py --one none|one|eight TABLE.npz [ticks [warmup]]
profiles/r23_history_bubbles_cost.txt was made with it."""
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
KINDS = ("none", "one", "eight")


def bubbles_of(setting, rec):
    """The smx_bubble records of a setting, placed on the recording's own poses."""
    from smarts_amd import _native as nat

    frames, vehicle = rec["frames"], rec["vehicle"]

    def where(v, f):  # the pose of recorded vehicle v in frame f (the last frame that has it, if f lacks it)
        for g in range(min(f, len(frames) - 1), -1, -1):
            slot = [k for k in range(vehicle.shape[1]) if vehicle[g, k] == v]
            if slot:
                return float(frames[g, slot[0], 0]), float(frames[g, slot[0], 1])
        raise ValueError(f"vehicle {v} is not in the recording")

    if setting == "one":
        x, y = where(0, 25)
        return [nat.SmxBubble(x, y, 20.0, 20.0, 2.0, 0.0, 0.0, -1, 0, 0)]
    out = []
    for i in range(7):
        x, y = where(i % FOLLOWERS, 15 + 10 * i)
        out.append(nat.SmxBubble(x, y, 12.0 + i, 12.0, 2.0, 0.0, 0.0, -1, 2, 4))
    out.append(nat.SmxBubble(0.0, 0.0, 6.0, 6.0, 2.0, 0.0, 8.0, 0, 2, 4))
    return out


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
    if setting == "none":
        sim.set_history_handover(torch.full((1, E, A), -1, dtype=torch.int32).cuda())
    else:
        sim.set_history_bubbles(bubbles_of(setting, rec))
    zero = torch.zeros((E, N, 3), dtype=torch.float32).cuda()
    tick = lambda: sim.step_history_handover(zero)  # noqa: E731
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
           "hijacked_after": int((sim.out["bubble_state"][:, :A] == 2).sum()) if setting != "none" else 0,
           "released_after": int((sim.out["bubble_state"][:, :A] == 3).sum()) if setting != "none" else 0,
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
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()}
    print(json.dumps({"ms": ms, "median": med, "spread_over_median": spread, "one_over_none": round(med["one"] / med["none"], 4),
                      "eight_over_none": round(med["eight"] / med["none"], 4)}))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], sys.argv[3], *(int(a) for a in sys.argv[4:6]))
    else:
        main(*(int(a) for a in sys.argv[1:4]))

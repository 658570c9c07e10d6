"""Developer: what a mixed fleet's tick costs, per tick on one MI355X (include/smx.h smx_set_agent_spaces / smx_step_mixed).
loop, 4096 envs x 8 agents, bench.py's sensors (waypoints 4 x 20, neighbours 10 within 50 m, OGM 64 x 64 in c4's extra),
no auto_reset.  Four settings of the same shape:
    lane_default      uniform Lane in the form the shape takes by default (large one-lane: k_control_fast + k_control_listed)
    lane_teams        uniform Lane under the teams cut (k_control_paths + k_control_law)
    continuous_teams  uniform Continuous under the teams cut (k_control_law)
    mixed             slots 0, 2, 4, 6 Lane and 1, 3, 5, 7 Continuous — the spaces interleave inside every wavefront — through
                      smx_step_mixed: the teams cut, k_control_paths_mixed<Lane> + k_control_law_mixed<Lane> +
                      k_control_law_mixed<Continuous>
Lane slots take bench.py's action stream; Continuous slots brake to a stop and stand (throttle 0, brake 1, steering 0:
an open-loop throttle leaves the road at the first bend, and the controller's work, law + 24 physics substeps, does not
depend on the values).  No agent ends: done_collision, done_off_road and done_off_route are off in all four settings (a
braking agent rolls straight on and may stop beside its lane), so every setting keeps its whole fleet of E x N agents
and `agents_alive_after` says so.  Each run is a fresh
process: reset, `ticks` ticks timed at level 1 (the median tick), then 50 ticks at level 2 (the median control phase: the
control kernels alone on the caller's stream).  Runs alternate over the settings.
    python tools/dev_agent_spaces_cost.py [runs [ticks]]            (default 2 runs of each, 200 ticks)
    python tools/dev_agent_spaces_cost.py --one SETTING [ticks]
Part (b) of profiles/r27_agent_spaces_cost.txt is its output (2 runs, 200 ticks)."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, N = 4096, 8
SETTINGS = ["lane_default", "lane_teams", "continuous_teams", "mixed"]


def one(setting, ticks=200):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns
    from smarts_amd.map_compiler import compile_map
    from smarts_amd.sumo_map import load_net

    _, scenario, kw = bench.workload_config("c4", envs=E, vehicles=N)
    kw["auto_reset"] = False
    kw["done_collision"] = kw["done_off_road"] = kw["done_off_route"] = False
    kw["action_space"] = "Continuous" if setting == "continuous_teams" else "Lane"
    kw["launch_strategy"] = "auto" if setting in ("lane_default", "mixed") else "large_teams"
    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", scenario)))
    spawns = make_spawns(cm, E, N, episodes=1, seed=42)
    lane = torch.from_numpy(bench.action_stream(E, N, 42, 0)).cuda()
    floats = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float32).repeat(bench.ACTION_CYCLE, E, N, 1).cuda()
    sim = BatchedSim(cm, SimConfig(**kw), spawns=spawns)
    if setting == "mixed":
        sim.set_agent_spaces(["Lane", "Continuous"] * (N // 2))

    def tick(i):
        k = i % bench.ACTION_CYCLE
        if setting == "mixed":
            sim.step_mixed(lane=lane[k], floats=floats[k])
        else:
            sim.step(floats[k] if setting == "continuous_teams" else lane[k])

    sim.reset()
    sim.set_timing(1)
    for i in range(ticks):
        tick(i)
    torch.cuda.synchronize()
    ms = np.asarray(sim.read_step_ms())
    sim.set_timing(2)
    for i in range(ticks, ticks + 50):
        tick(i)
    torch.cuda.synchronize()
    phases = np.asarray(sim.read_phase_ms())
    sim.set_timing(0)
    sim.sync()
    res = {"setting": setting, "ms": round(float(np.median(ms)), 4), "control_ms": round(float(np.median(phases[:, 0])), 4),
           "phased_tick_ms": round(float(np.median(phases.sum(axis=1))), 4), "agents_alive_after": int((sim.flags & 1).sum()),
           "form": sim.launch_form(), "ticks": ticks}
    sim.close()
    print(json.dumps(res))


def main(runs=2, ticks=200):
    rows = []
    for r, setting in enumerate(SETTINGS * runs):
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", setting, str(ticks)], capture_output=True,
                              text=True, timeout=300)
        if proc.returncode != 0:  # nothing more is started after a run that failed
            sys.exit(f"run {r} {setting}: exit {proc.returncode}\n{proc.stderr[-2000:]}")
        row = json.loads(proc.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        rows.append(row)
    med = {s: {k: statistics.median(r[k] for r in rows if r["setting"] == s) for k in ("ms", "control_ms")} for s in SETTINGS}
    out = {"median": med}
    for s in SETTINGS[:3]:
        out[f"mixed_over_{s}"] = {k: round(med["mixed"][k] / med[s][k], 4) for k in ("ms", "control_ms")}
    print(json.dumps(out))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    else:
        main(*(int(a) for a in sys.argv[1:3]))

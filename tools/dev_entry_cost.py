"""Developer: delayed agent entry bound against the same batch without it, per tick on one MI355X (include/smx.h
smx_set_agent_entry).  loop, 4096 envs x 8 agents, bench.py's sensors (waypoints 4 x 20, neighbours 10 within 50 m, OGM
64 x 64 in c4's extra), the launch form bench.py's shape takes (large one-lane), bench.py's action stream.  Bound: agents 6
and 7 of every env — a quarter — enter at ticks drawn over the first 50 (ready tick 1 + (7 e + 13 a) mod 50), checked at
their spawn rows' front bumpers; unbound: every agent from the reset, as today.  Each run is a fresh process: reset, then
`ticks` ticks timed at level 1 (the entries fall inside them); the median tick of a run.  Runs alternate, unbound first.
    python tools/dev_entry_cost.py [runs [ticks]]            (default 3 runs of each, 200 ticks)
    python tools/dev_entry_cost.py --one unbound|bound [ticks]
profiles/r26_delayed_entry_cost.txt was made with it."""
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, N = 4096, 8


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
    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", scenario)))
    spawns = make_spawns(cm, E, N, episodes=1, seed=42)
    actions = torch.from_numpy(bench.action_stream(E, N, 42, 0)).cuda()
    sim = BatchedSim(cm, SimConfig(**kw), spawns=spawns)
    if setting == "bound":
        ready = np.zeros((1, E, N), dtype=np.int32)
        check = np.zeros((1, E, N, 3))
        for e in range(E):
            for a in range(N):
                x, y, h = spawns[0, e * N + a, :3]
                ang = h + 0.5 * math.pi
                check[0, e, a] = (x + math.cos(ang) * 1.84, y + math.sin(ang) * 1.84, 3.68)
            for a in (6, 7):
                ready[0, e, a] = 1 + (7 * e + 13 * a) % 50
        sim.set_agent_entry(ready, check)
    sim.reset()
    sim.set_timing(1)
    for i in range(ticks):
        sim.step(actions[i % bench.ACTION_CYCLE])
    torch.cuda.synchronize()
    ms = np.asarray(sim.read_step_ms())
    sim.set_timing(0)
    res = {"setting": setting, "ms": round(float(np.median(ms)), 4), "ms_first50": round(float(np.median(ms[:50])), 4),
           "agents_alive_after": int((sim.flags & 1).sum()), "form": sim.launch_form(), "ticks": ticks}
    if setting == "bound":
        res["entered"] = int((sim.out["entry_status"] == 2).sum())
    sim.close()
    print(json.dumps(res))


def main(runs=3, ticks=200):
    rows = []
    for r, setting in enumerate(["unbound", "bound"] * runs):
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", setting, str(ticks)], capture_output=True,
                              text=True, timeout=300)
        if proc.returncode != 0:  # nothing more is started after a run that failed
            sys.exit(f"run {r} {setting}: exit {proc.returncode}\n{proc.stderr[-2000:]}")
        row = json.loads(proc.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        rows.append(row)
    plain = [r["ms"] for r in rows if r["setting"] == "unbound"]
    bound = [r["ms"] for r in rows if r["setting"] == "bound"]
    m_p, m_b = statistics.median(plain), statistics.median(bound)
    print(json.dumps({"unbound_ms": plain, "bound_ms": bound, "median_unbound": m_p, "median_bound": m_b,
                      "bound_over_unbound": round(m_b / m_p, 4)}))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    else:
        main(*(int(a) for a in sys.argv[1:3]))

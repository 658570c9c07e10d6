"""Developer: what the state guard (SimConfig(state_guard=True), include/smx.h smx_set_guard) costs per tick on one
MI355X, on bench.py's configs[3] shape (scenarios/loop, 4096 envs x 32 agents, waypoints + neighbours + 64 x 64 OGM,
auto_reset, large launch form).  Every run is a process of its own with one sim — guard off or guard on for the whole
run, reset pass included — over the same spawns, the same action stream and the same ticks, so both settings time the
same stretch of the same episode (the tick gets shorter as agents end; nothing is out of bounds in the run, so the
guard changes no state and the alive counts agree, which the driver checks).  The runs alternate, off first, `runs` of
each, and the figure is the median of each setting's runs.  HIP-event timing of smx_step (smx_set_timing(1)), the
median tick of a run.  The figure is what the tests and the byte cost, not what an ended agent does.  (Two sims in one
process do not measure this: the second one's side streams share hardware queues with the first one's and its forked
tick loses its overlap.)
    python tools/dev_guard_cost.py [runs [ticks [warmup]]]     (default 3 runs of each, 100 ticks after 20 warm-up ticks)
    python tools/dev_guard_cost.py --one off|on [ticks [warmup]]     (one run, what the driver starts)
profiles/r12_guard_cost.txt was made with it."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(setting, ticks=100, warm=20):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from smarts_amd.engine import BatchedSim, SimConfig, make_spawns
    from smarts_amd.map_compiler import compile_map
    from smarts_amd.sumo_map import load_net

    on = setting == "on"
    _, scenario, kw = bench.workload_config("c4")
    E, N = kw["num_envs"], kw["num_vehicles"]
    cm = compile_map(load_net(os.path.join(ROOT, "smarts_amd", "scenarios", scenario)))
    spawns = make_spawns(cm, E, N, episodes=4, seed=42)
    actions = torch.from_numpy(bench.action_stream(E, N, 42, 0)).cuda()
    sim = BatchedSim(cm, SimConfig(state_guard=on, **kw), spawns=spawns)
    out = sim.reset()
    for i in range(warm):
        sim.step(actions[i % bench.ACTION_CYCLE])
    sim.set_timing(1)
    for i in range(warm, warm + ticks):
        sim.step(actions[i % bench.ACTION_CYCLE])
    torch.cuda.synchronize()
    ms = np.asarray(sim.read_step_ms())
    sim.set_timing(0)
    res = {"guard": setting, "ms": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
           "alive_after": int((sim.flags & 1).sum()), "bytes_set": int(out["guard"].sum()) if on else 0,
           "shape": f"{scenario} {E} x {N}", "form": sim.lib.smx_launch_form(sim.handle), "ticks": ticks, "warmup": warm}
    sim.close()
    print(json.dumps(res))


def main(runs=3, ticks=100, warm=20):
    rows = []
    for r in range(runs):
        for setting in ("off", "on"):
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", setting, str(ticks), str(warm)],
                                  capture_output=True, text=True, timeout=300)
            if proc.returncode != 0:  # nothing more is started after a run that failed
                sys.exit(f"run {r} guard {setting}: exit {proc.returncode}\n{proc.stderr[-2000:]}")
            rows.append(json.loads(proc.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[-1]), flush=True)
    off = [r["ms"] for r in rows if r["guard"] == "off"]
    on = [r["ms"] for r in rows if r["guard"] == "on"]
    assert len({r["alive_after"] for r in rows}) == 1 and not any(r["bytes_set"] for r in rows), "the runs differ"
    m_off, m_on = statistics.median(off), statistics.median(on)
    print(json.dumps({"off_ms": off, "on_ms": on, "median_off": m_off, "median_on": m_on,
                      "on_over_off": round(m_on / m_off, 4)}))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], *(int(a) for a in sys.argv[3:5]))
    else:
        main(*(int(a) for a in sys.argv[1:4]))

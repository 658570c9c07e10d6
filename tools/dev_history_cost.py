"""Developer: a replayed social slot against a scripted one, per tick on one MI355X (include/smx.h
smx_set_social_history).  One sim of bench.py's configs[3] shape (scenarios/loop, 4096 envs x 32 vehicles, waypoints +
neighbours + 64 x 64 OGM, auto_reset, large launch form) with num_social = 8.  Every env starts from env 0's spawn rows
(one episode of them), so all envs walk one episode and restart together, in both settings.  A first run records the
scripted social vehicles' poses of env 0 by tick count into a table; then runs alternate, scripted (constant speed
model) first, `runs` of each: the history runs bind that table (every env from frame 0), so both settings see the same
vehicles at the same places — the driver checks that the alive counts agree.  Every run is a process of its own;
HIP-event timing of smx_step (smx_set_timing(1)), the median tick of a run.
    python tools/dev_history_cost.py [runs [ticks [warmup]]]     (default 3 runs of each, 100 ticks after 20 warm-up ticks)
    python tools/dev_history_cost.py --one record|scripted|history TABLE.npz [ticks [warmup]]
profiles/r16_traffic_history_cost.txt was made with it."""
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOCIAL = 8


def one(setting, path, ticks=100, warm=20):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from smarts_amd import _native as nat
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
    S = nat.S
    words = [S[w] for w in ("X", "Y", "HEADING", "U")]
    frames = {}

    def record():
        frames[int(sim.env_ticks[0])] = sim.state[words, 0, N - SOCIAL:].T.cpu().numpy().copy()

    if setting == "history":
        rec = np.load(path)
        sim.set_traffic_history(TrafficHistoryTable(rec["frames"], rec["vehicle"], kw["dt"]))
    sim.reset()
    if setting == "record":
        record()
    for i in range(warm):
        sim.step(actions[i % bench.ACTION_CYCLE])
        if setting == "record":
            record()
    sim.set_timing(1)
    for i in range(warm, warm + ticks):
        sim.step(actions[i % bench.ACTION_CYCLE])
        if setting == "record":
            record()
    torch.cuda.synchronize()
    ms = np.asarray(sim.read_step_ms())
    sim.set_timing(0)
    if setting == "record":
        F = max(frames) + 2  # (one frame beyond the last tick count seen: the commit looks a tick ahead)
        table = np.zeros((F, SOCIAL, 4))
        vehicle = np.full((F, SOCIAL), -1, dtype=np.int32)
        for k, rows in frames.items():
            table[k], vehicle[k] = rows, np.arange(SOCIAL)
        np.savez(path, frames=table, vehicle=vehicle)
    agents = sim.flags[:, :N - SOCIAL]
    res = {"social": setting, "ms": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
           "agents_alive_after": int((agents & 1).sum()), "episodes": int(sim.env_episode.max()),
           "shape": f"{scenario} {E} x {N}, {SOCIAL} social", "form": sim.lib.smx_launch_form(sim.handle), "ticks": ticks, "warmup": warm}
    sim.close()
    print(json.dumps(res))


def main(runs=3, ticks=100, warm=20):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "recorded.npz")
        for r, setting in enumerate(["record"] + ["scripted", "history"] * runs):
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", setting, path, str(ticks), str(warm)],
                                  capture_output=True, text=True, timeout=300)
            if proc.returncode != 0:  # nothing more is started after a run that failed
                sys.exit(f"run {r} {setting}: exit {proc.returncode}\n{proc.stderr[-2000:]}")
            rows.append(json.loads(proc.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[-1]), flush=True)
    scripted = [r["ms"] for r in rows if r["social"] == "scripted"]
    history = [r["ms"] for r in rows if r["social"] == "history"]
    same = len({(r["agents_alive_after"], r["episodes"]) for r in rows}) == 1
    m_s, m_h = statistics.median(scripted), statistics.median(history)
    print(json.dumps({"scripted_ms": scripted, "history_ms": history, "median_scripted": m_s, "median_history": m_h,
                      "history_over_scripted": round(m_h / m_s, 4), "same_episode": same}))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(sys.argv[2], sys.argv[3], *(int(a) for a in sys.argv[4:6]))
    else:
        main(*(int(a) for a in sys.argv[1:4]))

"""The bench's workloads at full size, held to their own shards and to the oracle.

bench.py defines its inputs per global env: env e spawns from PCG64(seed + e) (make_spawns(first_env=...)) and draws its
actions from PCG64(seed + e + 1 000 003) (bench.action_stream).  A rank of `bench.py --gpus N` therefore runs a slice of
the whole batch, and every rank size runs another launch form: C4's whole batch takes the one-lane cut with the
one-lane path-seeds kernel and its slow seeds chain on a side stream (at and above SMX_ONE_LANE_MIN_VEHICLES), its
shards the one-lane cut with team seeds or the small form; C5 and C3 take the teams cut whole and the teams cut or the
small form sharded.  So the whole batch must equal, env for env and bit for bit, the concatenation of its shards, on
every output key, the state and the flags, at every tick — with the whole batch's ticks enqueued back to back as the
bench enqueues them (no host synchronisation between them: the comparisons are enqueued on the device too).  A sample
of the C4 batch's envs, first, last and two in the middle, is held to the oracle teacher-forced as well.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import bench
import parity

pytestmark = pytest.mark.gpu

SEED = 42  # bench.py's spawn and action seed
EPISODES = 4  # spawn rows per vehicle, as bench.py builds them
MAPS = {"loop": "loop", "intersections/4lane": "4lane", "minicity": "minicity"}  # bench scenario -> compiled_maps name
# Through the first restarts: an env restarts once all its vehicles are done, first on tick 1 175 of C4 (4 envs have by
# tick 1 400), on tick 345 of C5 (5 by 460) and on tick 58 of C3 (144 by 100).
TICKS = {"c4": 1400, "c5": 460, "c3": 120}
SLOW_TICKS = (60, 300, 600, 900, 1300)  # C4: where the slow-list lengths are read (each read synchronises the device)
TOL_RESET = dict(tol64=1e-9, tol32=2e-6)  # test_gpu_launch_variants.py's
TOL_TICK = dict(tol64=1e-9, tol32=2e-5)


@pytest.fixture(scope="module")
def bench_inputs(compiled_maps):
    """(cm, cfg_kw, spawns, actions) of bench.py's workload `config` at its full size, as bench.py builds them for one
    rank; built once per module (the spawn tables take seconds)."""
    cache = {}

    def get(config):
        if config not in cache:
            from smarts_amd.engine import make_spawns

            _, scenario, cfg_kw = bench.workload_config(config)
            cm = compiled_maps(MAPS[scenario])
            E, N = cfg_kw["num_envs"], cfg_kw["num_vehicles"]
            cache[config] = (cm, cfg_kw, make_spawns(cm, E, N, episodes=EPISODES, seed=SEED),
                             bench.action_stream(E, N, SEED, 0))
        return cache[config]

    return get


def _batch(cm, cfg_kw, spawns, actions, first, n):
    """The batch of envs [first, first + n) of the whole table, with its slice of the action stream on the device."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig

    kw = dict(cfg_kw)
    kw["num_envs"] = n
    N = kw["num_vehicles"]
    sim = BatchedSim(cm, SimConfig(**kw), spawns=np.ascontiguousarray(spawns[:, first * N:(first + n) * N]))
    return sim, torch.from_numpy(np.ascontiguousarray(actions[:, first:first + n])).cuda()


def _slow_counts(sim):
    """[facts, seeds, control, rows]: the lengths of the last tick's slow lists (developer entry point; synchronises)."""
    fn = sim.lib.smx_debug_slow_counts
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    buf = (C.c_int32 * 4)()
    assert fn(sim.handle, buf) == 0
    return list(buf)


def _env_first(out, sim, key):
    """The array `key` of a batch (an output, "state" or "flags") with the env axis first."""
    if key == "state":
        return sim.state.transpose(0, 1)
    if key == "flags":
        return sim.flags
    if key == "learner":
        return out[key].transpose(0, 1)
    return out[key]


def _env_differs(a, b):
    """Per env (axis 0): whether a and b differ anywhere, as not np.array_equal(a, b, equal_nan=True)."""
    ne = a != b
    if a.is_floating_point():
        ne &= ~(a.isnan() & b.isnan())
    return ne.reshape(a.shape[0], -1).any(1)


class ShardCheck:
    """Enqueues, per tick, key and shard, the number of envs in which the shard differs from its slice of the whole
    batch and the first such env (global index); read once, after the run.  The shards' arrays are concatenated and
    compared with the whole batch's in one pass per key (a few launches per key, whatever the world)."""

    def __init__(self, keys, plans, ticks):
        import torch

        self.keys, self.plans = keys, plans
        E = plans[-1].first_env + plans[-1].num_envs
        self.E = E
        self.owner = torch.from_numpy(np.repeat(np.arange(len(plans)), [p.num_envs for p in plans])).cuda()
        self.env = torch.arange(E, device="cuda")
        self.bad = torch.zeros((len(keys), E), dtype=torch.bool, device="cuda")
        self.rec = torch.zeros((ticks + 1, len(keys), len(plans), 2), dtype=torch.int64, device="cuda")

    def add(self, t, whole, whole_out, shards, shard_outs):
        import torch

        assert sorted(whole_out) == sorted(shard_outs[0]) and len(whole_out) + 2 == len(self.keys)
        for k, key in enumerate(self.keys):
            joined = torch.cat([_env_first(o, s, key) for s, o in zip(shards, shard_outs)])
            self.bad[k] = _env_differs(_env_first(whole_out, whole, key), joined)
        K, R = len(self.keys), len(self.plans)
        owner = self.owner.expand(K, self.E)
        self.rec[t, :, :, 0] = torch.zeros((K, R), dtype=torch.int64, device="cuda").scatter_add_(1, owner, self.bad.long())
        first = torch.where(self.bad, self.env, self.E)
        self.rec[t, :, :, 1] = torch.full((K, R), self.E, dtype=torch.int64, device="cuda").scatter_reduce_(
            1, owner, first, "amin")

    def report(self, world):
        rec = self.rec.cpu().numpy()
        lines = []
        for t, k, r in np.argwhere(rec[..., 0] > 0):
            lines.append(f"world {world} rank {r} {'reset' if t == 0 else f'tick {t - 1}'} {self.keys[k]}: "
                         f"{rec[t, k, r, 0]} envs differ, the first global env {rec[t, k, r, 1]}")
        return lines


# config, envs of the whole batch (its first ones), worlds, form of the whole batch, form of every shard
CASES = [
    ("c4", 4096, 2, "large_one_lane", "large_one_lane"),  # 65 536 vehicles a shard: the one-lane cut with team seeds
    ("c4", 4096, 3, "large_one_lane", "large_one_lane"),  # 43 712 / 43 680
    ("c4", 4096, 4, "large_one_lane", "large_one_lane"),  # 32 768
    ("c4", 4096, 8, "large_one_lane", "small"),           # 16 384
    ("c4", 3584, 7, "large_one_lane", "small"),           # 114 688 vehicles whole, SMX_ONE_LANE_MIN_VEHICLES exactly
    ("c5", 4096, 3, "large_teams", "large_teams"),        # 87 424 / 87 360
    ("c5", 4096, 8, "large_teams", "large_teams"),        # 32 768
    ("c5", 4096, 16, "large_teams", "small"),             # 16 384
    ("c3", 2048, 2, "large_teams", "small"),              # 16 384: k_control, register form
    ("c3", 2048, 3, "large_teams", "small"),              # 10 928 / 10 912: register form
    ("c3", 2048, 4, "large_teams", "small"),              # 8 192: k_control's LDS form
]


@pytest.mark.parametrize("config,E,world,whole_form,shard_form", CASES,
                         ids=[f"{c[0]}-{c[1]}envs-world{c[2]}" for c in CASES])
def test_full_batch_equals_its_shards(config, E, world, whole_form, shard_form, bench_inputs):
    """The bench's whole batch under AUTO against the shards of one world stepped in lockstep, from reset() through
    restarts and a thinned batch: every output key, the state and the flags bit for bit at every tick.  C4's whole
    batch must have run its slow seeds chain (seeds list non-empty), and its 65 536-vehicle shards, the one-lane cut
    with the team seeds kernel, must have left the seeds list empty."""
    import torch

    from smarts_amd.sharding import ShardPlan

    cm, cfg_kw, spawns, actions = bench_inputs(config)
    T = TICKS[config]
    plans = [ShardPlan(E, world, r) for r in range(world)]
    whole, whole_acts = _batch(cm, cfg_kw, spawns, actions, 0, E)
    batches = [_batch(cm, cfg_kw, spawns, actions, p.first_env, p.num_envs) for p in plans]
    shards = [s for s, _ in batches]
    assert whole.launch_form() == whole_form
    assert [s.launch_form() for s in shards] == [shard_form] * world
    one_lane_seeds = config == "c4"  # the whole batch holds >= SMX_ONE_LANE_MIN_VEHICLES vehicles on a loop map
    team_seeds_shard = shard_form == "large_one_lane" and world == 2  # (65 536 vehicles)

    out = whole.reset()
    outs = [s.reset() for s in shards]
    check = ShardCheck(sorted(out) + ["state", "flags"], plans, T)
    check.add(0, whole, out, shards, outs)
    episode0 = whole.env_episode.clone()
    alive = torch.zeros(T, dtype=torch.int64, device="cuda")
    slow = {"whole": [], "shard": []}
    for t in range(T):
        out = whole.step(whole_acts[t % bench.ACTION_CYCLE])
        outs = [s.step(acts[t % bench.ACTION_CYCLE]) for s, (_, acts) in zip(shards, batches)]
        check.add(t + 1, whole, out, shards, outs)
        alive[t] = out["active"].sum()
        if one_lane_seeds and t in SLOW_TICKS:
            slow["whole"].append(_slow_counts(whole))
            if team_seeds_shard:
                slow["shard"].append([_slow_counts(s) for s in shards])
    bad = check.report(world)
    restarted = int((whole.env_episode > episode0).sum().item())
    alive_frac = alive.cpu().numpy() / (E * cfg_kw["num_vehicles"])
    print(f"\n{config} {E} envs world {world}: slow lists [facts, seeds, control, rows] {slow}, "
          f"{restarted} envs restarted, alive fraction min {alive_frac.min():.3f} last {alive_frac[-1]:.3f}")
    assert len(bad) == 0, f"{len(bad)} mismatches, the first:\n" + "\n".join(bad[:12])
    assert restarted > 0
    assert alive_frac.min() < 0.9
    if one_lane_seeds:
        # the one-lane path-seeds kernel sent vehicles to the slow seeds chain
        assert all(c[1] > 0 for c in slow["whole"]), slow["whole"]
    if team_seeds_shard:
        # the one-lane cut with the team seeds kernel: no seeds list on the ticks where the whole batch has one (on loop
        # the facts, control and rows lists stay empty in both)
        for per_tick in slow["shard"]:
            assert all(c[1] == 0 for c in per_tick), slow["shard"]
    whole.close()
    for s in shards:
        s.close()


SAMPLE_TICKS = 12
SAMPLE_SEED = 2024  # draws the two middle envs once


def test_full_batch_sample_against_the_oracle(bench_inputs, nets):
    """C4's whole batch under AUTO (the one-lane cut with the slow seeds chain): env 0, env 4 095 and two middle envs
    against the oracle, teacher-forced, from reset through 12 ticks — float64 to 1e-9, float32 to 2e-6 on reset and
    2e-5 on ticks, integers, counts and flags exact.  An env that ends inside the window is compared through its done
    tick (its finishing rows are the final_* ones) and then dropped.  Some compared vehicle must enter a junction lane
    or change road inside the window: the reasons the one-lane seeds kernel sends a vehicle to the slow chain."""
    import torch

    from smarts_amd.engine import BatchedSim, SimConfig

    cm, cfg_kw, spawns, actions = bench_inputs("c4")
    cfg = SimConfig(**cfg_kw)
    E, N = cfg.num_envs, cfg.num_vehicles
    sim = BatchedSim(cm, cfg, spawns=spawns)
    assert sim.launch_form() == "large_one_lane"
    middle = np.random.default_rng(SAMPLE_SEED).choice(np.arange(1, E - 1), size=2, replace=False)
    envs = [0, *sorted(int(e) for e in middle), E - 1]
    idx = torch.tensor(envs, device="cuda")
    ob = parity.OracleBatch(nets("loop"), cm, dataclasses.replace(cfg, num_envs=len(envs)),
                            spawns[0].reshape(E, N, 4)[envs].reshape(-1, 4))
    acts_dev = torch.from_numpy(actions).cuda()

    def sample(o):
        """The sampled envs' rows, sliced on the device, as parity.host lays them out (env_done kept apart)."""
        return parity.host({k: v.index_select(0, idx) for k, v in o.items() if k not in ("env_done", "learner")}), \
            o["env_done"].index_select(0, idx).cpu().numpy()

    d, _ = sample(sim.reset())
    bad = parity.compare(d, ob.reset_observe(), where="reset ", **TOL_RESET)
    assert bad == [], "\n".join(bad[:8])
    live = list(range(len(envs)))
    lanes = [d["ego_lane"][:, 0].copy()]
    active = [d["active"].astype(bool)]
    compared = [np.ones(len(envs) * N, bool)]
    for t in range(SAMPLE_TICKS):
        a = actions[t % bench.ACTION_CYCLE]
        d, env_done = sample(sim.step(acts_dev[t % bench.ACTION_CYCLE]))
        for i in list(live):
            obs, rew, dones = ob.envs[i].step(list(a[envs[i]]))
            o = parity.pack(ob.cfg, ob.lane_no, N, obs, rew, dones)
            rows = slice(i * N, (i + 1) * N)
            mine = {k: v[rows] for k, v in d.items()}
            where = f"env {envs[i]} t{t} "
            if env_done[i]:
                # the rows are the next episode's first ones; the finishing tick's are the final_* rows
                fin = {k: mine["final_" + k] for k in ("ego_pos", "ego_f32", "ego_lane", "events", "dist")}
                fin.update(reward=mine["reward"], done=mine["done"])
                bad = parity.compare(fin, {k: o[k] for k in fin}, where=where + "(done) ", **TOL_TICK)
                live.remove(i)
            else:
                bad = parity.compare(mine, o, where=where, **TOL_TICK)
            assert bad == [], "\n".join(bad[:8])
        keep = np.zeros(len(envs) * N, bool)
        for i in live:
            keep[i * N:(i + 1) * N] = True
        lanes.append(d["ego_lane"][:, 0].copy())
        active.append(d["active"].astype(bool))
        compared.append(keep)
        parity.sync_oracle_from_device(ob, sim, envs=envs)
    # junction lanes entered and roads changed by vehicles that were compared on both ticks, alive on both
    entered = changed = 0
    for t in range(1, len(lanes)):
        both = compared[t] & active[t - 1] & active[t] & (lanes[t - 1] >= 0) & (lanes[t] >= 0)
        prev, cur = lanes[t - 1][both].astype(np.int64), lanes[t][both].astype(np.int64)
        entered += int((cm.lane_in_junction[cur].astype(bool) & ~cm.lane_in_junction[prev].astype(bool)).sum())
        changed += int((cm.lane_road[cur] != cm.lane_road[prev]).sum())
    print(f"\nsampled envs {envs}: {entered} junction lanes entered, {changed} road changes, "
          f"{len(envs) - len(live)} envs ended")
    assert entered + changed > 0
    sim.close()

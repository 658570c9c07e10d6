"""The mission-pool scenario of the GPU tests (tests/test_gpu_mission_pool.py) and an oracle twin built per env.

``scene(nets, compiled_maps)``: the 4lane junction, E = 3 envs of two agents and one scripted social vehicle, a pool of
four missions — the left turn, the straight route whose goal lies close behind the junction and the single-road route of
tests/test_gpu_missions.py, and a left turn that starts a few metres in front of the junction, with a via list — and a table of rows (R = 2) whose entries include -1: slot 1 is routed in envs 0 and 1 and
endless in env 2.  The spawn row of (episode row, env, agent) is the start of the mission chosen there; an endless entry
starts on a free lane — and so does the one cell in MISPLACED, an agent handed a route it does not stand on: it is off
its route from its first observation.
"""
import numpy as np

import parity
from oracle.sim import OracleEnv

E, AGENTS, SOCIAL, ROWS = 3, 2, 1, 2
N = AGENTS + SOCIAL
SPEED = 13.0
# rows[k][e][a]: a pool index, -1 = endless
TABLE = np.array([[[0, 1], [3, 3], [2, -1]],
                  [[3, -1], [1, 0], [-1, 2]]], dtype=np.int32)
MISPLACED = {(0, 1, 0)}  # (row, env, agent)


def pool_4lane(nets, cm):
    from smarts_amd.missions import Mission, Route, plan_mission
    from smarts_amd.vias import Via, resolve_vias

    net = nets("4lane")
    south = net.getEdge("edge-south-SN").getLane(1).getLength()
    specs = [
        Route(begin=("edge-north-NS", 0, 40), end=("edge-east-WE", 0, 30)),    # left turn through the junction
        Route(begin=("edge-west-WE", 1, 60), end=("edge-east-WE", 1, 12)),     # straight on; the goal lies close behind it
        # a left turn from 6 m in front of the junction, past its vias
        Route(begin=("edge-south-SN", 1, south - 6.0), end=("edge-west-EW", 0, "max")),
        Route(begin=("edge-east-EW", 1, 10), end=("edge-east-EW", 1, 40)),     # single-road route, goal 30 m ahead
    ]
    missions = [plan_mission(net, Mission(r)) for r in specs]
    vias = [[] for _ in missions]
    vias[2] = resolve_vias(cm, [Via("edge-south-SN", 1, south - 3.0, 13), Via("edge-west-EW", 0, 20, 8),
                                Via("edge-north-SN", 1, 8, 13, hit_distance=3.0)])
    return missions, vias


def free_pose(nets, env):
    """Where an agent with an endless entry starts: on the west approach, lane 0, a lane no pool mission starts on."""
    from smarts_amd.missions import EndlessMission, plan_mission

    return plan_mission(nets("4lane"), EndlessMission(begin=("edge-west-WE", 0, 20.0 + 12.0 * env))).spawn_pose()


def spawn_rows(nets, cm, missions, table, seed=7):
    """float64 (R, E * N, 4) agent spawn rows and (R, E * N, 2) social rows: the agents at their missions' starts."""
    from smarts_amd.engine import make_spawns

    R = table.shape[0]
    spawns, where = make_spawns(cm, E, N, episodes=R, seed=seed, return_lanes=True)
    for k in range(R):
        for e in range(E):
            for a in range(AGENTS):
                m = table[k, e, a]
                x, y, h = missions[m].spawn_pose() if m >= 0 and (k, e, a) not in MISPLACED else free_pose(nets, e)
                spawns[k, e * N + a] = (x, y, h, SPEED)
    return spawns, where


def env_missions(missions, vias, table, k, e):
    """Per-slot missions and vias (N entries each) of env e in episode row k: what smx_set_missions / smx_set_vias take."""
    ms = [missions[m] if m >= 0 else None for m in table[k, e]] + [None] * SOCIAL
    vs = [list(vias[m]) if m >= 0 else [] for m in table[k, e]] + [[] for _ in range(SOCIAL)]
    return ms, vs


class PoolOracle(parity.OracleBatch):
    """E oracle envs, each with ITS missions and vias (parity.OracleBatch gives every env one shared list)."""

    def __init__(self, net, cm, cfg, spawns_ep0, social_ep0, missions, vias, table_row):
        from oracle.road_network import ORoadNetwork

        self.cfg = cfg
        self.road_map = ORoadNetwork(net, lanepoint_spacing=cm.lanepoint_spacing)
        self.lane_no = {lid: i for i, lid in enumerate(cm.lane_ids)}
        self.N = cfg.num_vehicles
        ocfg = parity.oracle_config(cfg)
        K = cfg.num_social
        self.envs = []
        for e in range(cfg.num_envs):
            rows = slice(e * self.N, (e + 1) * self.N)
            social = [(cm.lane_ids[int(l)], float(off)) for l, off in social_ep0[rows][self.N - K:]]
            omissions = [dict(route=list(missions[m].route_roads), goal=tuple(missions[m].goal)) if m >= 0 else None
                         for m in table_row[e]]
            ovias = [[dict(lane_id=v.lane_id, position=v.position, hit_distance=v.hit_distance, required_speed=v.required_speed)
                      for v in (vias[m] if m >= 0 else [])] for m in table_row[e]]
            self.envs.append(OracleEnv(self.road_map, spawns_ep0[rows], [ocfg] * (self.N - K), dt=cfg.dt, social=social,
                                       social_speed_factor=cfg.social_speed_factor, vias=ovias, social_model=cfg.social_model,
                                       missions=omissions))

"""``lane_ttc`` over dense rows (smarts_amd/env/lane_ttc_rows.py), the CPU twin of the device's k_lane_ttc: against the
reference's own outputs (tests/golden/std_obs.npz, tests/golden/lane_ttc_cases.npz from gen_golden_lane_ttc.py),
against the host function on ``Observation`` objects over an oracle rollout, and the entry check of the new buffers
(smx_check_buffers, no device).  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import lane_ttc_check as chk
import parity
from conftest import GOLDEN
from smarts_amd import _native as nat
from smarts_amd.engine import SimConfig, make_spawns
from smarts_amd.env.custom_observations import lane_ttc
from smarts_amd.env.format_obs import FormatObs, std_obs
from smarts_amd.env.lane_ttc_rows import lane_ttc_rows
from smarts_amd.env.observations import ObservationBuilder

T = nat.TTC
REF_KEYS = (("distance_from_center", T["DIST_FROM_CENTER"], 1), ("angle_error", T["ANGLE_ERROR"], 1),
            ("ego_ttc", T["TTC"], 3), ("ego_lane_dist", T["DTC"], 3))


def _same_decisions(got, ref):
    """Which lane entries are the defaults (1000 / 1), the end-of-road zeros, or a neighbour's value: exact."""
    for col, defaults in ((T["TTC"], (0.0, 1000.0)), (T["DTC"], (0.0, 1.0))):
        for d in defaults:
            if not np.array_equal(got[..., col:col + 3] == d, ref[..., col:col + 3] == d):
                return False
    return True


def test_rows_match_the_reference_on_the_rollout_fixture():
    """(a) every tick and agent of std_obs.npz: the reference's own lane_ttc outputs on the same rows."""
    g = np.load(os.path.join(GOLDEN, "std_obs.npz"))
    cfg = SimConfig(num_envs=1, num_vehicles=8, neighbors=True, nb_radius=50.0)
    checked = picked = 0
    for t in range(int(g["n_ticks"])):
        rows = {k[len(f"t{t}_in_"):]: g[k] for k in g.files if k.startswith(f"t{t}_in_")}
        values, flags = lane_ttc_rows(rows, cfg)
        for i in range(8):
            if f"t{t}_a{i}_lanettc_ego_ttc" not in g.files:
                assert flags[i] == 0, (t, i)  # no observation: no row
                continue
            ref = np.zeros(nat.TTC_COUNT)
            for key, col, n in REF_KEYS:
                ref[col:col + n] = g[f"t{t}_a{i}_lanettc_{key}"]
            assert flags[i] & nat.TTC_VALID and not flags[i] & nat.TTC_INDEX_ERROR, (t, i, flags[i])
            assert bool(flags[i] & nat.TTC_STD) == (f"t{t}_a{i}_ttc_ttc" in g.files), (t, i)  # _std_ttc is not None
            assert bool(flags[i] & nat.TTC_TRUNCATED)  # 20 of the 33 waypoints are kept
            assert _same_decisions(values[i], ref), (t, i, values[i], ref)
            assert np.abs(values[i] - ref).max() <= chk.TOL64, (t, i, values[i], ref)
            checked += 1
            picked += int(chk.non_default_ttc(ref))
            # FormatObs.from_rows fills StdObs.ttc from the rows: the reference's _std_ttc on the same observation
            d = FormatObs.from_rows({**{k: v[None] for k, v in rows.items()}, "lane_ttc": values[None],
                                     "lane_ttc_flags": flags[None]}, 0, i)
            if f"t{t}_a{i}_ttc_ttc" in g.files:
                for k, v in d.ttc.items():
                    want = g[f"t{t}_a{i}_ttc_{k}"]
                    assert np.asarray(v).dtype == np.float32 and np.abs(np.asarray(v, np.float64) - want).max() <= 1e-6, (t, i, k)
            else:
                assert d.ttc is None
            assert FormatObs.from_rows({k: v[None] for k, v in rows.items()}, 0, i).ttc is None  # unchanged without the key
    assert checked >= 16 and picked >= 3


def test_rows_match_the_reference_on_the_hand_built_cases():
    """(b) lane_ttc_cases.npz: ties, the 2 m gate and one ulp either side, the speed clamp, discarded ttc, a neighbour
    without a lane, min over neighbours, the end lanes, paths sharing a lane index, the reference's IndexError."""
    g = np.load(os.path.join(GOLDEN, "lane_ttc_cases.npz"))
    rows = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    n, P, W = rows["wp_heading"].shape
    cfg = SimConfig(num_envs=1, num_vehicles=n, neighbors=True, wp_paths=P, wp_len=W, nb_max=rows["nb_speed"].shape[1],
                    wp_lookahead=int(g["wp_lookahead"]))
    values, flags = lane_ttc_rows(rows, cfg)
    names = [str(s) for s in g["names"]]
    for want in ("equidistant_on_one_path", "gap_exactly_2_from_zero", "gap_one_ulp_above_2", "gap_one_ulp_below_2",
                 "equal_speeds_clamp", "faster_neighbour_ahead_discarded", "neighbour_without_lane",
                 "two_neighbours_one_path_min", "lane_index_0_right_is_zero", "top_lane_left_is_zero",
                 "junction_paths_share_lane_index", "lane_index_past_the_paths"):
        assert want in names
    assert int(g["raised"].sum()) >= 1
    for i, name in enumerate(names):
        assert flags[i] & nat.TTC_VALID, name
        assert bool(flags[i] & nat.TTC_INDEX_ERROR) == bool(g["raised"][i]), name
        assert bool(flags[i] & nat.TTC_STD) == (rows["nb_count"][i] > 0), name
        assert bool(flags[i] & nat.TTC_TRUNCATED) == (name == "junction_more_paths_than_rows"), name
        if g["raised"][i]:
            assert not values[i, T["TTC"]:].any(), name  # the six lane columns read 0
            continue
        assert _same_decisions(values[i], g["ref"][i]), (name, values[i], g["ref"][i])
        assert np.abs(values[i] - g["ref"][i]).max() <= chk.TOL64, (name, values[i], g["ref"][i])
    # the host function on objects agrees on the same rows, and raises where the reference does
    b = ObservationBuilder([f"lane_{i}" for i in range(8)], [f"road_{i}" for i in range(8)], [f"agent_{i}" for i in range(n)],
                           waypoints=True, neighbors=True, accelerometer=True, dt=0.1)
    for i, name in enumerate(names):
        if g["raised"][i]:
            with pytest.raises(IndexError):
                lane_ttc(b.build(rows, i, 1, 0.1))
        else:
            assert np.abs(_host_row(lane_ttc(b.build(rows, i, 1, 0.1))) - g["ref"][i]).max() <= chk.TOL64, name


def _host_row(val):
    out = np.zeros(nat.TTC_COUNT)
    for key, col, n in REF_KEYS:
        out[col:col + n] = np.asarray(val[key], dtype=np.float64)
    return out


ROLLOUT_SEED = 3  # chosen on the CPU: 259 of the rollout's 768 agent-ticks carry a ttc entry other than 0 / 1000


@pytest.fixture(scope="module")
def rollout(nets, compiled_maps):
    """(c) loop, 2 envs x 32 agents, 12 ticks of parity.lane_actions on the oracle: per tick the dense rows and the
    host function's rows (lane_ttc on Observation objects), NaN where the agent has no observation."""
    cm = compiled_maps("loop")
    E, N = 2, 32
    cfg = SimConfig(num_envs=E, num_vehicles=N, neighbors=True, nb_radius=50.0)
    spawns = make_spawns(cm, E, N, episodes=1, seed=ROLLOUT_SEED)
    ob = parity.OracleBatch(nets("loop"), cm, cfg, spawns[0])
    ob.reset_observe()
    b = ObservationBuilder(cm.lane_ids, [cm.road_ids[r] for r in cm.lane_road], [f"agent_{i}" for i in range(N)],
                           waypoints=True, neighbors=True, accelerometer=True, dt=0.1)
    rng = np.random.default_rng(ROLLOUT_SEED)
    ticks = []
    for t in range(12):
        rows = ob.step(parity.lane_actions(rng, E, N))
        host = np.full((E * N, nat.TTC_COUNT), np.nan)
        std = np.zeros(E * N, dtype=bool)
        for e in range(E):
            env_rows = {k: v[e * N:(e + 1) * N] for k, v in rows.items()}
            for i in range(N):
                if env_rows["wp_count"][i, 0] == 0:
                    continue
                o = b.build(env_rows, i, t + 2, round((t + 2) * 0.1, 6))
                host[e * N + i] = _host_row(lane_ttc(o))
                std[e * N + i] = std_obs(o).ttc is not None
        ticks.append((rows, host, std))
    return cfg, ticks


def test_rows_equal_the_host_function_on_objects(rollout):
    """(c) row for row: flags from the rows' own counts, values within TOL64 (margin-sensitive agent-ticks left out
    and counted: numpy's two-element dot inside np.linalg.norm may or may not fuse), and the rollout is not vacuous."""
    cfg, ticks = rollout
    valid = left_out = picked = 0
    for t, (rows, host, std) in enumerate(ticks):
        has = ~np.isnan(host[:, 0])
        flags = lane_ttc_rows(rows, cfg)[1]
        assert np.array_equal((flags & nat.TTC_VALID) != 0, has), t
        assert np.array_equal((flags & nat.TTC_STD) != 0, std), t  # where FormatObs' _std_ttc is not None
        assert not (flags & nat.TTC_INDEX_ERROR).any(), t  # (the host function ran)
        v, lo, nd = chk.compare(np.nan_to_num(host), flags, rows, cfg, where=f"tick {t}")
        valid, left_out, picked = valid + v, left_out + lo, picked + nd
    assert picked >= 20, picked
    assert left_out <= chk.MAX_LEFT_OUT * valid, (left_out, valid)


def test_restatement_margins_stay_under_the_cap(rollout):
    """The share of agent-ticks lane_ttc_rows itself reports as margin-sensitive on the rollout: under the cap the
    GPU tests allow."""
    cfg, ticks = rollout
    valid = close = 0
    for rows, _, _ in ticks:
        _, flags, margin = lane_ttc_rows(rows, cfg, margins=True)
        ok = (flags & nat.TTC_VALID) != 0
        assert np.isinf(margin[~ok]).all()
        valid, close = valid + int(ok.sum()), close + int((ok & (margin < chk.MARGIN)).sum())
    assert valid >= 600 and close <= chk.MAX_LEFT_OUT * valid, (close, valid)


def test_leading_axes_and_rows_without_an_observation(rollout):
    cfg, ticks = rollout
    rows = ticks[-1][0]
    flat = lane_ttc_rows(rows, cfg)
    shaped = lane_ttc_rows({k: v.reshape((2, 32) + v.shape[1:]) for k, v in rows.items()}, cfg)
    assert shaped[0].shape == (2, 32, nat.TTC_COUNT) and shaped[1].shape == (2, 32)
    assert np.array_equal(shaped[0].reshape(flat[0].shape), flat[0]) and np.array_equal(shaped[1].reshape(-1), flat[1])
    empty = parity.empty_dense(cfg, 5)
    values, flags = lane_ttc_rows(empty, cfg)
    assert not flags.any() and not values.any()


# ---- (d) the entry check of the new buffers (host only, the built library) ----
def _declared(E=3, N=4, sensors=nat.SENSOR_WAYPOINTS | nat.SENSOR_NEIGHBORS | nat.SENSOR_LANE_TTC):
    """An smx_config with SMX_SENSOR_LANE_TTC and structs whose pointers are fake (never dereferenced by
    smx_check_buffers) with exactly the extents the configuration needs."""
    c = nat.SmxConfig()
    c.num_envs, c.num_vehicles, c.dt, c.sensors = E, N, 0.1, sensors
    c.wp_lookahead, c.wp_paths, c.wp_len, c.nb_max, c.nb_radius = 32, 4, 20, 10, 50.0
    n, PW, K = E * N, 4 * 20, 10
    st, sp, out = nat.SmxState(), nat.SmxSpawns(), nat.SmxOutputs()
    state = dict(f64=(nat.S_COUNT * n, nat.DT_F64), flags=(n, nat.DT_I32), steps=(n, nat.DT_I32), env_ticks=(E, nat.DT_I32),
                 env_done_count=(E, nat.DT_I32), env_episode=(E, nat.DT_I32), driven_path=(n * 500, nat.DT_F64),
                 seed_cache=(nat.SEED_COUNT * n, nat.DT_I32), facts_i32=(nat.FACT_I_COUNT * n, nat.DT_I32),
                 facts_f64=(nat.FACT_F_COUNT * n, nat.DT_F64), env_reset_pending=(E, nat.DT_I32))
    for k, name in enumerate(nat.STATE_BUFFERS):
        setattr(st, name, 0x1000 + k)
        st.count[k], st.dtype[k] = state[name]
    sp.episodes, sp.pose, sp.pose_count = 2, 0x2000, 2 * n * 4
    outs = dict(ego_pos=(3 * n, nat.DT_F64), ego_f32=(nat.EGO_F32_COUNT * n, nat.DT_F32), ego_lane=(2 * n, nat.DT_I16),
                events=(9 * n, nat.DT_U8), reward=(n, nat.DT_F64), dist=(n, nat.DT_F64), done=(n, nat.DT_U8),
                active=(n, nat.DT_U8), env_done=(E, nat.DT_U8),
                wp_pos=(n * PW * 3, nat.DT_F64), wp_heading=(n * PW, nat.DT_F32), wp_lane_width=(n * PW, nat.DT_F32),
                wp_speed_limit=(n * PW, nat.DT_F32), wp_lane_index=(n * PW, nat.DT_I8), wp_lane_id=(n * PW, nat.DT_I16),
                wp_count=(n * 5, nat.DT_U8), nb_pos=(n * K * 3, nat.DT_F64), nb_box=(n * K * 3, nat.DT_F32),
                nb_heading=(n * K, nat.DT_F32), nb_speed=(n * K, nat.DT_F32), nb_lane_index=(n * K, nat.DT_I8),
                nb_lane_id=(n * K, nat.DT_I16), nb_slot=(n * K, nat.DT_I8), nb_count=(n, nat.DT_U8),
                lane_ttc=(n * nat.TTC_COUNT, nat.DT_F64), lane_ttc_flags=(n, nat.DT_U8))
    for k, name in enumerate(nat.OUTPUT_FIELDS):
        if name in outs:
            setattr(out, name, 0x3000 + k)
            out.count[k], out.dtype[k] = outs[name]
    return c, st, sp, out


def _check(c, st, sp, out):
    lib = nat.load_library()
    err = C.create_string_buffer(512)
    rc = lib.smx_check_buffers(C.byref(c), 0, C.byref(st), C.byref(sp), C.byref(out), err, 512)
    return rc, err.value.decode()


def test_entry_check_of_the_lane_ttc_buffers():
    c, st, sp, out = _declared()
    assert _check(c, st, sp, out) == (0, "")
    # the outputs are appended: the indices before them keep their values
    assert nat.OUTPUT_FIELDS[-2:] == ["lane_ttc", "lane_ttc_flags"] and nat.OUTPUT_FIELDS.index("final_dist") == 47
    # the bit without waypoints, without neighbours
    for missing in (nat.SENSOR_WAYPOINTS, nat.SENSOR_NEIGHBORS):
        c.sensors &= ~missing
        rc, msg = _check(c, st, sp, out)
        assert rc == -1 and "lane_ttc" in msg and "SMX_SENSOR_WAYPOINTS" in msg, (rc, msg)
        c.sensors |= missing
    k = nat.OUTPUT_FIELDS.index("lane_ttc")
    keep = out.lane_ttc
    out.lane_ttc = None  # NULL
    rc, msg = _check(c, st, sp, out)
    assert rc == -1 and "out.lane_ttc is NULL" in msg, (rc, msg)
    out.lane_ttc = keep
    out.count[k] -= 1  # short
    rc, msg = _check(c, st, sp, out)
    assert rc == -1 and "out.lane_ttc" in msg and "elements declared" in msg, (rc, msg)
    out.count[k] += 1
    out.dtype[k] = nat.DT_F32  # float32 where the ABI writes float64
    rc, msg = _check(c, st, sp, out)
    assert rc == -1 and "out.lane_ttc" in msg and "dtype" in msg, (rc, msg)
    out.dtype[k] = nat.DT_F64
    kf = nat.OUTPUT_FIELDS.index("lane_ttc_flags")
    out.count[kf] -= 1
    rc, msg = _check(c, st, sp, out)
    assert rc == -1 and "out.lane_ttc_flags" in msg, (rc, msg)
    out.count[kf] += 1
    # more waypoints per agent than the kernel stages
    c.wp_paths, c.wp_len = 32, 33
    rc, msg = _check(c, st, sp, out)
    assert rc == -1 and "wp_paths * wp_len" in msg, (rc, msg)
    c.wp_paths, c.wp_len = 4, 20
    assert _check(c, st, sp, out) == (0, "")
    # without the bit the two buffers are not asked for
    c.sensors &= ~nat.SENSOR_LANE_TTC
    out.lane_ttc, out.lane_ttc_flags = None, None
    assert _check(c, st, sp, out) == (0, "")


def test_create_refuses_the_bit_without_its_sensors():
    lib = nat.load_library()
    c, _, _, _ = _declared(sensors=nat.SENSOR_WAYPOINTS | nat.SENSOR_LANE_TTC)
    h = C.c_void_p(0xDEAD)
    rc = lib.smx_create(C.byref(c), 0, C.byref(h))
    assert rc == -1 and not h.value and "lane_ttc" in lib.smx_last_error(None).decode()


def test_sim_config_carries_the_bit():
    assert SimConfig(neighbors=True, lane_ttc=True).sensors_mask() & nat.SENSOR_LANE_TTC
    assert not SimConfig(neighbors=True).sensors_mask() & nat.SENSOR_LANE_TTC

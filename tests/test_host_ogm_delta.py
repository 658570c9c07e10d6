"""OGM delta stores, the host side (no GPU): the piece mask's size and the plan's decision to use it
(smarts_amd/csrc/smx_plan.h: smx_ogm_mask_words, TickPlan::ogm_delta), the two entry points' declarations, and the premise
the change rests on — between two ticks of the headline workload a tile's non-zero pieces barely move — measured on the
CPU oracle."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRIDS = [(64, 64), (96, 32), (128, 96), (256, 256), (10, 10)]


def test_mask_words_and_the_null_mask_decision(tmp_path):
    """A word per 64 pieces of a tile, the last one padded; the plan hands the kernels the mask iff the handle holds one
    and the tile is a whole number of pieces — in a tick and in a reset call, in every form — and nothing else in the plan
    moves with it."""
    lib_path = str(tmp_path / "libhost_plan_ogm_delta.so")
    cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "smarts_amd", "csrc"),
           os.path.join(NATIVE, "host_plan_ogm_delta.cpp"), "-o", lib_path]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lib = C.CDLL(lib_path)
    lib.host_plan_ogm_delta.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]
    piece = lib.host_ogm_piece()
    assert piece in (16, 64)
    for (w, h), (E, N), strategy, is_step, held in itertools.product(GRIDS, ((4, 8), (2, 16), (4096, 32)), range(5), (0, 1), (0, 1)):
        words, same = C.c_ulonglong(0), C.c_int(0)
        delta = lib.host_plan_ogm_delta((C.c_int * 7)(w, h, E, N, strategy, is_step, held), C.byref(words), C.byref(same))
        case = (w, h, E, N, strategy, is_step, held)
        assert words.value == (w * h // piece + 63) // 64, case
        assert delta == int(bool(held) and (w * h) % piece == 0), case
        assert same.value == 1, case
    # the sizes the issue names, spelt out: 64 x 64 is four words at 16 bytes and one at 64; 10 x 10 is no whole piece
    want = {16: {(64, 64): 4, (96, 32): 3, (128, 96): 12, (256, 256): 64}, 64: {(64, 64): 1, (96, 32): 1, (128, 96): 3, (256, 256): 16}}
    for (w, h), n in want[piece].items():
        words, same = C.c_ulonglong(0), C.c_int(0)
        assert lib.host_plan_ogm_delta((C.c_int * 7)(w, h, 2, 16, 0, 1, 1), C.byref(words), C.byref(same)) == 1
        assert words.value == n, (w, h)
    words, same = C.c_ulonglong(0), C.c_int(0)
    assert lib.host_plan_ogm_delta((C.c_int * 7)(10, 10, 2, 16, 0, 1, 1), C.byref(words), C.byref(same)) == 0


def test_entry_points_are_declared_and_bound():
    from smarts_amd import _native as nat
    from smarts_amd.engine import BatchedSim

    header = open(os.path.join(ROOT, "include", "smx.h")).read()
    assert "int smx_invalidate_outputs(smx_handle h);" in header
    assert "int smx_set_ogm_delta(smx_handle h, int on);" in header
    assert "smx_invalidate_outputs" in nat.EXPORTS and "smx_set_ogm_delta" in nat.EXPORTS
    assert callable(BatchedSim.invalidate_outputs) and callable(BatchedSim.set_ogm_delta)


def test_a_tiles_pieces_barely_move_between_ticks(nets, compiled_maps):
    """The premise, on the oracle: loop, 2 envs x 32 vehicles, OGM 64 x 64, the benchmark's own spawns and action
    stream, 12 ticks.  Counted per tile and tick: the pieces that are non-zero now or were a tick ago — what a delta
    store writes — at 16 and at 64 bytes.  (The oracle gave 9.2 % of a tile at 16 bytes when the change was proposed.)"""
    import bench
    import parity
    from smarts_amd.engine import SimConfig, make_spawns

    E, N, T = 2, 32, 12
    _, scenario, kw = bench.workload_config("c4", E, N)
    assert scenario == "loop" and kw["ogm_width"] == 64 and kw["ogm_height"] == 64
    cm = compiled_maps("loop")
    cfg = SimConfig(**kw)
    spawns = make_spawns(cm, E, N, episodes=4, seed=42, first_env=0)
    ob = parity.OracleBatch(nets("loop"), cm, cfg, spawns[0])
    acts = bench.action_stream(E, N, 42, 0)
    tile = 64 * 64
    prev = ob.reset_observe()["ogm"].reshape(E * N, tile)
    stored = {16: 0, 64: 0}
    tiles = 0
    for t in range(T):
        cur = ob.step(acts[t % bench.ACTION_CYCLE])["ogm"].reshape(E * N, tile)
        seen = (cur != 0).any(axis=1)  # the tiles drawn this tick
        for piece in stored:
            nz_now = (cur.reshape(E * N, tile // piece, piece) != 0).any(axis=2)
            nz_old = (prev.reshape(E * N, tile // piece, piece) != 0).any(axis=2)
            stored[piece] += int((nz_now | nz_old)[seen].sum()) * piece
        tiles += int(seen.sum())
        prev = cur
    assert tiles > E * N * T // 2
    share = {piece: stored[piece] / (tiles * tile) for piece in stored}
    print(f"bytes a delta store writes per tile: 16-byte pieces {share[16] * tile:.0f} B ({100 * share[16]:.1f} %), "
          f"64-byte pieces {share[64] * tile:.0f} B ({100 * share[64]:.1f} %) of {tile} B, over {tiles} tiles")
    assert share[16] < 0.25

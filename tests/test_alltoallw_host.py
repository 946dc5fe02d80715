"""MPI_Alltoallw and the batched block pack on the host (no GPU): the exported symbols, the first
check before MPI_Init, and the partition of one launch's workgroups over its blocks
(mv2h_pack_blocks_plan, a pure function)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mvapich2_amd as m
from mvapich2_amd.consts import TYPES
from tests.test_abi import exported

K_DONE_MAX_GRID = 1 << 20


def test_alltoallw_symbols_are_exported():
    syms = exported()
    for name in ("mv2h_pack_blocks", "mv2h_pack_blocks_plan", "PMPI_Alltoallw", "PMPI_Ialltoallw"):
        assert syms.get(name) == "T", name
    for name in ("MPI_Alltoallw", "MPI_Ialltoallw"):
        assert syms.get(name) == "W", name


def test_alltoallw_before_init_is_alltoallv_before_init():
    L = m.lib()
    WORLD, ERRORS_RETURN = 0x44000000, 0x54000001
    L.MPI_Comm_set_errhandler(WORLD, ERRORS_RETURN)
    F = TYPES["MPI_FLOAT"][0]
    buf = (ctypes.c_float * 4)()
    out = (ctypes.c_float * 4)()
    c, d, t = (ctypes.c_int * 1)(4), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(F)
    v = L.MPI_Alltoallv(buf, c, d, F, out, c, d, F, WORLD)
    w = L.MPI_Alltoallw(buf, c, d, t, out, c, d, t, WORLD)
    assert v != 0 and (w & 0x7f) == (v & 0x7f) == 15  # MPI_ERR_OTHER
    req = ctypes.c_int()
    assert L.MPI_Ialltoallw(buf, c, d, t, out, c, d, t, WORLD, ctypes.byref(req)) & 0x7f == 15


def test_both_run_table_kernels_stage_the_same_number_of_runs():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvapich2_amd", "csrc", "pack")
    vals = [re.findall(r"^constexpr int kRunLds = (\d+);", open(os.path.join(csrc, f)).read(), flags=re.M)
            for f in ("pack.hip", "pack_blocks.h")]
    assert vals == [["512"], ["512"]], vals


def check_plan(units, max_grid):
    rc, wg0, nwg, grid, tile = m.pack_blocks_plan(units, max_grid)
    assert rc == 0 and tile > 0
    nonempty = sum(1 for u in units if u)
    cap = min(max(max_grid, nonempty), K_DONE_MAX_GRID)
    assert wg0 == [sum(nwg[:b]) for b in range(len(units))], (units, max_grid, wg0, nwg)  # monotone, back to back
    for u, g in zip(units, nwg):
        assert (g == 0) if u == 0 else (1 <= g <= -(-u // tile)), (units, max_grid, nwg)
    assert sum(nwg) == grid <= cap, (units, max_grid, nwg, grid)
    tiles = [-(-u // tile) for u in units]
    if sum(tiles) <= cap:  # the cap out of reach: exactly the tiles
        assert nwg == tiles, (units, max_grid, nwg)
    return nwg, grid, tile


def test_pack_blocks_plan_hand_made():
    _, _, tile = check_plan([1], 1024)
    assert check_plan([tile], 1024)[0] == [1]
    assert check_plan([tile + 1], 1024)[0] == [2]
    assert check_plan([0, 5, 0, 3 * tile, 0, 0, 1, 2 * tile + 1], 1024)[0] == [0, 1, 0, 3, 0, 0, 1, 3]
    # max_grid = 1 with 3 non-empty blocks: one workgroup each
    nwg, grid, _ = check_plan([10 * tile, 0, 7 * tile, 1], 1)
    assert (nwg, grid) == ([1, 0, 1, 1], 3)
    # one block 1000 x the others under a cap: it takes nearly all, the others keep theirs
    nwg, grid, _ = check_plan([4 * tile] * 3 + [4000 * tile] + [4 * tile] * 4, 256)
    assert grid <= 256 and nwg[3] > 200 and all(g >= 1 for g in nwg)
    # every block empty: nothing to launch
    assert check_plan([0, 0, 0], 64)[1] == 0
    # a cap above the completion counters' range is cut to it
    nwg, grid, _ = check_plan([(K_DONE_MAX_GRID + 5) * tile, 3], 1 << 30)
    assert grid <= K_DONE_MAX_GRID and nwg[1] == 1
    # argument errors
    assert m.pack_blocks_plan([], 8)[0] == 12 and m.pack_blocks_plan([1] * 9, 8)[0] == 12


@pytest.mark.parametrize("seed", range(6))
def test_pack_blocks_plan_random(seed):
    rng = np.random.default_rng(seed)
    for _ in range(200):
        n = int(rng.integers(1, 9))
        units = [int(rng.choice([0, 1, 255, 256, 257, 1000, 70001, 1 << 22])) * int(rng.integers(0, 3)) for _ in range(n)]
        if rng.integers(0, 2) and n > 1:
            units[int(rng.integers(0, n))] = 1000 * max(max(units), 1)
        check_plan(units, int(rng.choice([1, 2, 3, 8, 64, 1024, 1 << 20])))

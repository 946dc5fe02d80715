"""MPI_Gather(v) / MPI_Scatter(v) / MPI_Allgatherv: what can be checked without a GPU -- the
exported symbols, the first check before MPI_Init, and the plan every rank derives for one gather
table from the n block lengths (mv2h_gv_plan, a pure function of the lengths and of the node's
shared limits).  Before MPI_Init there is no one-shot arena (slot size 0), so every non-empty
vector plans the pipelined kernel with the default tiling: up to 256 workgroups of at most 128 KiB
per block and round, 4 KiB at the least."""
import ctypes

import mvapich2_amd as m
from mvapich2_amd.consts import TYPES
from tests.test_abi import exported

MPI_ERR_OTHER = 15
NAMES = ("MPI_Gather", "MPI_Gatherv", "MPI_Scatter", "MPI_Scatterv", "MPI_Allgatherv",
         "MPI_Igather", "MPI_Igatherv", "MPI_Iscatter", "MPI_Iscatterv", "MPI_Iallgatherv")
MV2H = ("mv2h_allgatherv", "mv2h_gather", "mv2h_gatherv", "mv2h_scatter", "mv2h_scatterv", "mv2h_gv_plan")


def test_gather_symbols_are_weak_aliases_of_pmpi():
    syms = exported()
    L = m.lib()
    for n in NAMES:
        assert syms.get(n) == "W" and syms.get("P" + n) == "T", n
        a = ctypes.cast(getattr(L, n), ctypes.c_void_p).value
        b = ctypes.cast(getattr(L, "P" + n), ctypes.c_void_p).value
        assert a == b, n


def test_mv2h_gather_symbols_exist():
    syms = exported()
    for n in MV2H:
        assert syms.get(n) == "T", n


def test_calls_before_init_return_err_other():
    L = m.lib()
    WORLD, ERRORS_RETURN = 0x44000000, 0x54000001
    L.MPI_Comm_set_errhandler(WORLD, ERRORS_RETURN)
    h = TYPES["MPI_FLOAT"][0]
    buf, out = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()
    cnt, dsp = (ctypes.c_int * 2)(4, 4), (ctypes.c_int * 2)(0, 4)
    req = ctypes.c_int(0)
    P = ctypes.c_void_p
    a, b = P(ctypes.addressof(buf)), P(ctypes.addressof(out))
    r = ctypes.byref(req)
    assert L.MPI_Gather(a, 4, h, b, 4, h, 0, WORLD) == MPI_ERR_OTHER
    assert L.MPI_Gather(a, -1, 0x1234, b, 4, h, 99, 0x1) == MPI_ERR_OTHER  # still the first check
    assert L.MPI_Gatherv(a, 4, h, b, cnt, dsp, h, 0, WORLD) == MPI_ERR_OTHER
    assert L.MPI_Scatter(a, 4, h, b, 4, h, 0, WORLD) == MPI_ERR_OTHER
    assert L.MPI_Scatter(a, -1, 0x1234, b, 4, h, 99, 0x1) == MPI_ERR_OTHER
    assert L.MPI_Scatterv(a, cnt, dsp, h, b, 4, h, 0, WORLD) == MPI_ERR_OTHER
    assert L.MPI_Allgatherv(a, 4, h, b, cnt, dsp, h, WORLD) == MPI_ERR_OTHER
    assert L.MPI_Allgatherv(a, -1, 0x1234, b, None, None, h, 0x1) == MPI_ERR_OTHER
    assert L.MPI_Igather(a, 4, h, b, 4, h, 0, WORLD, r) == MPI_ERR_OTHER
    assert L.MPI_Igatherv(a, 4, h, b, cnt, dsp, h, 0, WORLD, r) == MPI_ERR_OTHER
    assert L.MPI_Iscatter(a, 4, h, b, 4, h, 0, WORLD, r) == MPI_ERR_OTHER
    assert L.MPI_Iscatterv(a, cnt, dsp, h, b, 4, h, 0, WORLD, r) == MPI_ERR_OTHER
    assert L.MPI_Iallgatherv(a, 4, h, b, cnt, dsp, h, WORLD, r) == MPI_ERR_OTHER
    sz, so = (ctypes.c_size_t * 2)(16, 16), (ctypes.c_size_t * 2)(0, 16)
    assert L.mv2h_allgatherv(a, 16, b, sz, so, None) == MPI_ERR_OTHER
    assert L.mv2h_gather(a, b, 16, 0, None) == MPI_ERR_OTHER
    assert L.mv2h_gatherv(a, 16, b, sz, so, 0, None) == MPI_ERR_OTHER
    assert L.mv2h_scatter(a, b, 16, 0, None) == MPI_ERR_OTHER
    assert L.mv2h_scatterv(a, sz, so, b, 16, 0, None) == MPI_ERR_OTHER


def test_plan_all_zero_lengths_move_nothing():
    for n in (1, 2, 5, 8):
        assert m.gv_plan([0] * n) == (0, "none", 0, 0, 0), n


def test_plan_follows_the_longest_block_whichever_rank_holds_it():
    long = 70001 * 4  # 280,004 B: 69 workgroups of 4 KiB, one round
    for n in (2, 3, 8):
        plans = set()
        for i in range(n):
            lens = [0] * n
            lens[i] = long
            plans.add(m.gv_plan(lens))
            lens[(i + 1) % n] = 12  # and a block of three floats
            plans.add(m.gv_plan(lens))
        assert plans == {(0, "pipe", (long + 4095) // 4096, 1, long)}, (n, plans)
    assert (long + 4095) // 4096 == 69
    # a block beyond one round of the largest tiling: 256 workgroups x 128 KiB = 32 MiB per round
    big = (64 << 20) + 16
    assert m.gv_plan([0, 16, big]) == (0, "pipe", 256, 3, big)
    assert m.gv_plan([big, 0, 0]) == (0, "pipe", 256, 3, big)


def test_plan_rejects_bad_arguments():
    L = m.lib()
    one = (ctypes.c_size_t * 1)(16)
    assert L.mv2h_gv_plan(0, one, None, None, None, None) != 0
    assert L.mv2h_gv_plan(9, one, None, None, None, None) != 0
    assert L.mv2h_gv_plan(1, None, None, None, None, None) != 0

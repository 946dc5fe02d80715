"""MPI_Alltoall / MPI_Alltoallv: what can be checked without a GPU -- the exported symbols, the
argument checks before MPI_Init, and the plan every rank derives for one MPI_Alltoallv from the
whole matrix of pair lengths (mv2h_alltoallv_plan, a pure function of the matrix and of the
node's shared limits).  Before MPI_Init there is no one-shot arena (slot size 0), so every
non-empty matrix plans the pipelined kernel with the default tiling: up to 256 workgroups of at
most 128 KiB per block and round (coll/kernels.h kPipeMaxGrid, kPipeMaxSub), 4 KiB at the least."""
import ctypes

import mvapich2_amd as m
from mvapich2_amd.consts import TYPES
from tests.test_abi import exported

MPI_ERR_TRUNCATE, MPI_ERR_OTHER = 14, 15
NAMES = ("MPI_Alltoall", "MPI_Alltoallv", "MPI_Ialltoall", "MPI_Ialltoallv", "MPIX_Alltoall_enqueue")


def test_alltoall_symbols_are_weak_aliases_of_pmpi():
    syms = exported()
    L = m.lib()
    for n in NAMES:
        assert syms.get(n) == "W" and syms.get("P" + n) == "T", n
        a = ctypes.cast(getattr(L, n), ctypes.c_void_p).value
        b = ctypes.cast(getattr(L, "P" + n), ctypes.c_void_p).value
        assert a == b, n


def test_mv2h_alltoall_symbols_exist():
    syms = exported()
    for n in ("mv2h_alltoall", "mv2h_alltoall_enqueue", "mv2h_alltoallv", "mv2h_alltoallv_plan"):
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
    a, b = ctypes.addressof(buf), ctypes.addressof(out)
    assert L.MPI_Alltoall(P(a), 4, h, P(b), 4, h, WORLD) == MPI_ERR_OTHER
    assert L.MPI_Alltoall(P(a), -1, 0x1234, P(b), 4, h, 0x1) == MPI_ERR_OTHER  # still the first check
    assert L.MPI_Alltoallv(P(a), cnt, dsp, h, P(b), cnt, dsp, h, WORLD) == MPI_ERR_OTHER
    assert L.MPI_Ialltoall(P(a), 4, h, P(b), 4, h, WORLD, ctypes.byref(req)) == MPI_ERR_OTHER
    assert L.MPI_Ialltoallv(P(a), cnt, dsp, h, P(b), cnt, dsp, h, WORLD, ctypes.byref(req)) == MPI_ERR_OTHER
    assert L.MPIX_Alltoall_enqueue(P(a), 4, h, P(b), 4, h, WORLD, P(1)) == MPI_ERR_OTHER
    sz = (ctypes.c_size_t * 2)(16, 16)
    assert L.mv2h_alltoall(P(a), P(b), 16, None) == MPI_ERR_OTHER
    assert L.mv2h_alltoallv(P(a), sz, sz, P(b), sz, sz, None) == MPI_ERR_OTHER


def test_plan_all_zero_matrix_moves_nothing():
    for n in (1, 2, 5, 8):
        rc, path, grid, rounds, maxlen = m.alltoallv_plan([[0] * n for _ in range(n)])
        assert (rc, path, grid, rounds, maxlen) == (0, "none", 0, 0, 0), n


def test_plan_follows_the_longest_pair_wherever_it_is():
    """one long pair among empties: every rank derives the geometry of that pair, whichever rank
    sends it (the same matrix gives the same plan; the plan does not depend on the pair's place)"""
    n = 3
    long = 70001 * 4
    plans = set()
    for i in range(n):
        for j in range(n):
            mat = [[0] * n for _ in range(n)]
            mat[i][j] = long
            mat[(i + 1) % n][(j + 1) % n] = 4  # and a pair of one element
            plans.add(m.alltoallv_plan(mat, aligned16=[0] * n))
    assert len(plans) == 1
    rc, path, grid, rounds, maxlen = plans.pop()
    assert rc == 0 and path == "pipe" and maxlen == long
    assert grid == (long + 4095) // 4096 and rounds == 1  # 69 workgroups of 4 KiB, one round
    # a pair beyond one round of the largest tiling: 256 workgroups x 128 KiB = 32 MiB per round
    big = (64 << 20) + 16
    mat = [[0] * n for _ in range(n)]
    mat[2][0] = big
    assert m.alltoallv_plan(mat) == (0, "pipe", 256, 3, big)


def test_plan_reports_a_mismatched_pair_as_truncation():
    n = 4
    slen = [[16 * (i + j) for j in range(n)] for i in range(n)]
    rlen = [[slen[j][i] for j in range(n)] for i in range(n)]
    assert m.alltoallv_plan(slen, rlen)[0] == 0
    rlen[3][1] += 4  # rank 3 expects 4 bytes more from rank 1 than rank 1 sends
    assert m.alltoallv_plan(slen, rlen)[0] == MPI_ERR_TRUNCATE
    rlen[3][1] -= 4
    slen[0][0] = 1  # the diagonal counts too
    assert m.alltoallv_plan(slen, rlen)[0] == MPI_ERR_TRUNCATE

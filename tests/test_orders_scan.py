"""MPI_Scan / MPI_Exscan reduction-order programs (runtime/orders.cpp plan_scan /
scan_progs, through mv2h_plan) against tests/ref_scan.py's rank-by-rank
restatement of MPIR_Scan_generic (scan.c:73-213) and MPIR_Exscan
(exscan.c:95-220), without a GPU; and the MPI entry points' boundary (weak
aliases, argument-check order) where that needs no world.

Every rank's result is a tree of its own; the programs are evaluated on the host
(one oracle.reduce_local call, or one call of the Python user function, per step)
and compared bit for bit."""
import ctypes

import numpy as np
import pytest

import mvapich2_amd as m
from mvapich2_amd.consts import OPS, TYPES
from oracle import oracle
from tests import ref_scan
from tests.helpers import assert_bytes_equal, rand_typed
from tests.test_abi import exported
from tests.test_orders import wide

NO_RESULT = 0xFF
ALGO = {"scan": 17, "exscan": 18}
COUNT = 257  # > 12: wide() plants NaN payloads, signed zeros, infinities and denormals


def run_prog(xs, prog, uop):
    """One program over whole operands: step (d, s) is w[d] = uop(in = w[s], inout = w[d])"""
    steps, res = prog
    w = [x.copy() for x in xs]
    for d, s in steps:
        w[d] = uop(w[s], w[d])
    return w[res]


def leaves(prog):
    steps, res = prog
    return sorted({r for st in steps for r in st} | {res})


@pytest.mark.parametrize("coll", ["scan", "exscan"])
@pytest.mark.parametrize("n", range(1, 9))
def test_programs_match_reference_builtin(coll, n):
    rng = np.random.default_rng(4100 + n)
    ref = getattr(ref_scan, coll)
    for t, op in (("MPI_FLOAT", "MPI_SUM"), ("MPI_DOUBLE", "MPI_SUM"), ("MPI_DOUBLE_INT", "MPI_MAXLOC")):
        h = TYPES[t][0]
        # DOUBLE_INT: values floored into [-8, 8) with equal values on many ranks (ties -> min loc)
        xs = [wide(t, COUNT, rng) if t != "MPI_DOUBLE_INT" else rand_typed(t, COUNT, rng).view(np.uint8).ravel().copy()
              for _ in range(n)]
        uop = ref_scan.builtin_uop(COUNT, h, OPS[op])
        want = ref([x.copy() for x in xs], uop)
        for r in range(n):
            algo, inner, unpinned, progs, _ = m.plan(coll, n, r, h, count=COUNT)
            assert (algo, inner, unpinned, len(progs)) == (ALGO[coll], 0, 0, 1)
            if want[r] is None:
                assert progs[0] == ([], NO_RESULT)
                continue
            assert leaves(progs[0]) == list(range(r + 1 if coll == "scan" else r))
            got = run_prog(xs, progs[0], uop)
            assert_bytes_equal(got, want[r], t, COUNT, f"{coll} n={n} rank {r} {op}")


@pytest.mark.parametrize("coll", ["scan", "exscan"])
@pytest.mark.parametrize("n", range(1, 9))
def test_programs_match_reference_user_ops(coll, n):
    """user ops: a commutative one takes the builtin branch, a non-commutative one keeps the lower
    ranks on the left (scan.c:182-190); inout = 2 in + 3 inout on int32 tells every order apart"""
    rng = np.random.default_rng(4200 + n)
    ref = getattr(ref_scan, coll)
    h = TYPES["MPI_INT"][0]
    xs = [rng.integers(-1000, 1000, 64).astype(np.int32).view(np.uint8) for _ in range(n)]
    fn = ref_scan.user_fn_2a3b
    for opkind, commute in ((1, True), (2, False)):
        want = ref([x.copy() for x in xs], fn, commute=commute)
        for r in range(n):
            progs = m.plan(coll, n, r, h, count=64, opkind=opkind)[3]
            if want[r] is None:
                assert progs[0][1] == NO_RESULT
                continue
            assert np.array_equal(run_prog(xs, progs[0], fn), want[r]), (coll, n, r, opkind)
    if n >= 3:  # the two kinds do differ (a rank below its partner reduces the other way round)
        a = [m.plan(coll, n, r, h, count=64, opkind=1)[3] for r in range(n)]
        b = [m.plan(coll, n, r, h, count=64, opkind=2)[3] for r in range(n)]
        assert a != b


def test_noncommutative_plan_keeps_lower_ranks_on_the_left():
    """With a non-commutative op the result must be x_0 . x_1 . ... . x_r with only the grouping
    changed: flattening any rank's tree (inout operand right of in, as uop(in, inout) = in . inout)
    lists the ranks in ascending order."""
    h = TYPES["MPI_INT"][0]

    def flatten(prog):
        steps, res = prog
        seq = {}
        for d, s in steps:
            seq[d] = seq.pop(s, [s]) + seq.get(d, [d])  # in . inout
        return seq.get(res, [res])

    for coll in ("scan", "exscan"):
        for n in range(2, 9):
            for r in range(n):
                prog = m.plan(coll, n, r, h, count=8, opkind=2)[3][0]
                if prog[1] == NO_RESULT:
                    continue
                assert flatten(prog) == list(range(r + 1 if coll == "scan" else r)), (coll, n, r)


@pytest.mark.parametrize("coll", ["scan", "exscan"])
def test_all_ranks_progset_equals_per_rank_plans(coll):
    h = TYPES["MPI_FLOAT"][0]
    for n in range(1, 9):
        for opkind in (0, 1, 2):
            algo, _, _, progs, _ = m.plan(coll + "_all", n, 0, h, count=100, opkind=opkind)
            assert algo == ALGO[coll] and len(progs) == n
            for r in range(n):
                assert progs[r] == m.plan(coll, n, r, h, count=100, opkind=opkind)[3][0], (n, r, opkind)


def test_exscan_rank0_has_no_result_and_rank1_copies():
    h = TYPES["MPI_DOUBLE"][0]
    for n in range(1, 9):
        assert m.plan("exscan", n, 0, h, count=5)[3] == [([], NO_RESULT)]
        if n > 1:
            assert m.plan("exscan", n, 1, h, count=5)[3] == [([], 0)]  # rank 1 takes x_0 as it is
        assert m.plan("scan", n, 0, h, count=5)[3] == [([], 0)]


def test_reference_order_is_not_the_left_to_right_chain():
    """A condition on the inputs: from rank 3 on (n >= 4) the reference's fp32 SUM differs from
    ((x0 + x1) + x2) + ... in at least one element, so a naive prefix order cannot pass the tests
    above; rank 3's tree is uop(in = uop(in = x0, inout = x1), inout = uop(in = x2, inout = x3))."""
    t, op = "MPI_FLOAT", "MPI_SUM"
    h = TYPES[t][0]
    assert m.plan("scan", 4, 3, h, count=1)[3] == [([(3, 2), (1, 0), (3, 1)], 3)]
    for n in range(4, 9):
        rng = np.random.default_rng(4100 + n)  # the operands of test_programs_match_reference_builtin
        xs = [wide(t, COUNT, rng) for _ in range(n)]
        uop = ref_scan.builtin_uop(COUNT, h, OPS[op])
        sc, ex = ref_scan.scan(xs, uop), ref_scan.exscan(xs, uop)
        for r in range(3, n):
            assert not np.array_equal(sc[r], ref_scan.chain(xs, uop, r)), (n, r)
        for r in range(4, n):
            assert not np.array_equal(ex[r], ref_scan.chain(xs, uop, r - 1)), (n, r)


def test_plan_argument_errors():
    L = m.lib()
    h = TYPES["MPI_FLOAT"][0]
    null = ctypes.POINTER(ctypes.c_int)()
    for coll in (4, 5, 6, 7):
        # the code itself is known (an unknown one is MPI_ERR_ARG whatever else is passed), with
        # every output pointer null, so the errors below are about the arguments they name
        assert L.mv2h_plan(coll, 8, 7, 0, 4, None, h, 0, 0, null, null, null, None) == 0
        assert L.mv2h_plan(coll, 4, 0, 0, 4, None, h, 3, 0, null, null, null, None) == 12  # op kind
        assert L.mv2h_plan(coll, 9, 0, 0, 4, None, h, 0, 0, null, null, null, None) == 12  # MPI_ERR_ARG: > 8 ranks
        assert L.mv2h_plan(coll, 4, 4, 0, 4, None, h, 0, 0, null, null, null, None) == 12
        assert L.mv2h_plan(coll, 4, 0, 0, 4, None, 0x1234, 0, 0, null, null, null, None) == 3  # MPI_ERR_TYPE


def test_scan_symbols_are_weak_aliases_of_pmpi():
    syms = exported()
    L = m.lib()
    for n in ("MPI_Scan", "MPI_Exscan", "MPI_Iscan", "MPI_Iexscan"):
        assert syms.get(n) == "W" and syms.get("P" + n) == "T", n
        a = ctypes.cast(getattr(L, n), ctypes.c_void_p).value
        b = ctypes.cast(getattr(L, "P" + n), ctypes.c_void_p).value
        assert a == b, n
    assert "mv2h_scan" in syms and "mv2h_exscan" in syms


def test_argument_checks_before_init():
    """Before MPI_Init every check fails on the first one (MPI_ERR_OTHER), whatever the other
    arguments; the error handler of MPI_COMM_WORLD is set to MPI_ERRORS_RETURN first."""
    L = m.lib()
    WORLD, ERRORS_RETURN = 0x44000000, 0x54000001
    L.MPI_Comm_set_errhandler(WORLD, ERRORS_RETURN)
    h, op = TYPES["MPI_FLOAT"][0], OPS["MPI_SUM"]
    buf = (ctypes.c_float * 4)()
    out = (ctypes.c_float * 4)()
    req = ctypes.c_int(0)
    for f in (L.MPI_Scan, L.MPI_Exscan):
        assert f(buf, out, 4, h, op, WORLD) == 15          # MPI_ERR_OTHER: not initialised
        assert f(buf, out, -1, 0x1234, 0x9999, 0x1) == 15  # still the first check
    for f in (L.MPI_Iscan, L.MPI_Iexscan):
        assert f(buf, out, 4, h, op, WORLD, ctypes.byref(req)) == 15
    # the C-ABI refuses a call without a world, after the op / type checks
    assert L.mv2h_scan(buf, out, 4, 0x1234, op, None) == 3   # MPI_ERR_TYPE
    assert L.mv2h_exscan(buf, out, 4, h, 0x9999, None) == 9  # MPI_ERR_OP
    assert L.mv2h_scan(buf, out, 0, h, op, None) == 0        # count 0 returns at once
    assert L.mv2h_scan(buf, out, 4, h, op, None) == 15       # MPI_ERR_OTHER: before MPI_Init
    L.MPI_Comm_set_errhandler(WORLD, 0x54000000)             # MPI_ERRORS_ARE_FATAL, the default

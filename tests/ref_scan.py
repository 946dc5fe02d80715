"""Rank-by-rank restatements of MPI_Scan and MPI_Exscan as MVAPICH2 2.3.7 runs
them on one node (TEST INFRASTRUCTURE: the expected results of the scan tests).

MPI_Scan: MPIR_Scan_MV2 -> MPIR_Scan (scan.c:225); on one node the intranode step
is the whole call and lands in MPIR_Scan_generic (scan.c:73-213).  MPI_Exscan:
MPIR_Exscan (exscan.c:95-220).  The nonblocking schedules (iscan.c:72-160,
iexscan.c) make the same calls in the same order.

uop(inp, io) returns the new inout, i.e. `inoutvec = invec op inoutvec`; every
call below is one uop(in, inout) of the cited reference code.  builtin_uop makes
one from a predefined op (one oracle.reduce_local call per uop)."""
import numpy as np

from oracle import oracle


def builtin_uop(count, dtype_handle, op_handle):
    def uop(inp, io):
        out = io.copy()
        assert oracle.reduce_local(inp, out, count, dtype_handle, op_handle) == 0
        return out
    return uop


def scan(xs, uop, commute=True):
    """MPIR_Scan_generic (scan.c:120-198): every rank's recvbuf"""
    n = len(xs)
    partial = [x.copy() for x in xs]
    recv = [x.copy() for x in xs]
    mask = 1
    while mask < n:
        prev = [p.copy() for p in partial]
        for r in range(n):
            dst = r ^ mask
            if dst >= n:
                continue
            tmp = prev[dst]
            if r > dst:
                partial[r] = uop(tmp, partial[r])      # :168-171
                recv[r] = uop(tmp, recv[r])            # :172-175
            elif commute:
                partial[r] = uop(tmp, partial[r])      # :177-181
            else:
                partial[r] = uop(partial[r], tmp)      # :182-190: tmp is the inout, then copied
        mask <<= 1
    return recv


def exscan(xs, uop, commute=True):
    """MPIR_Exscan (exscan.c:143-214): every rank's recvbuf; None where it is never written (rank 0)"""
    n = len(xs)
    partial = [x.copy() for x in xs]
    recv = [None] * n
    mask = 1
    while mask < n:
        prev = [p.copy() for p in partial]
        for r in range(n):
            dst = r ^ mask
            if dst >= n:
                continue
            tmp = prev[dst]
            if r > dst:
                partial[r] = uop(tmp, partial[r])                              # :169
                recv[r] = tmp.copy() if recv[r] is None else uop(tmp, recv[r])  # :179-193
            elif commute:
                partial[r] = uop(tmp, partial[r])                              # :196-199
            else:
                partial[r] = uop(partial[r], tmp)                              # :201-209
        mask <<= 1
    return recv


def chain(xs, uop, upto):
    """((x0 . x1) . x2) ... x_upto left to right, x0 the accumulator: the order a scan is NOT run in"""
    acc = xs[0].copy()
    for x in xs[1:upto + 1]:
        acc = uop(x, acc)
    return acc


def user_fn_2a3b(inp, io):
    """inout = 2 in + 3 inout on int32 (wrapping): not commutative, not associative"""
    with np.errstate(over="ignore"):
        return (2 * inp.view(np.int32) + 3 * io.view(np.int32)).astype(np.int32).view(io.dtype)

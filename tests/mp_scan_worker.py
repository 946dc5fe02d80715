"""One rank of the multi-process MPI_Scan / MPI_Exscan GPU tests (launched by
tests/test_gpu_scan_mp.py; several ranks may share one GPU).  Runs every case of
the spec through the MPI API and saves the bytes of its receive buffer, which is
prefilled with 0xA5 so that a buffer the call must not write shows it."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mvapich2_amd as m  # noqa: E402
from mvapich2_amd.consts import OPS, TYPES  # noqa: E402
from tests.helpers import rand_typed  # noqa: E402

WORLD = 0x44000000
IN_PLACE = ctypes.c_void_p(-1 & 0xFFFFFFFFFFFFFFFF)
FILL = 0xA5


def inputs(case, rank, call=0):
    rng = np.random.default_rng(case["seed"] * 1000 + call * 100 + rank)
    return rand_typed(case["type"], case["count"], rng, small=case.get("small", False), ties=case.get("ties", False))


def scan_call(L, case, x, h, op, count, ext):
    """one MPI_Scan / MPI_Exscan (variant: plain, inplace, nonblocking); returns the receive buffer's bytes"""
    excl = case["coll"] == "exscan"
    variant = case.get("variant", "plain")
    sb = m.DeviceBuffer.from_array(x)
    rb = m.DeviceBuffer(count * ext)
    rb.upload(np.full(count * ext, FILL, dtype=np.uint8))
    if variant == "inplace":
        rc = (L.MPI_Exscan if excl else L.MPI_Scan)(IN_PLACE, sb.ptr, count, h, op, WORLD)
        rb = sb
    elif variant == "nonblocking":
        req = ctypes.c_int()
        rc = (L.MPI_Iexscan if excl else L.MPI_Iscan)(sb.ptr, rb.ptr, count, h, op, WORLD, ctypes.byref(req))
        if rc == 0:
            rc = L.MPI_Wait(ctypes.byref(req), None)
    else:
        rc = (L.MPI_Exscan if excl else L.MPI_Scan)(sb.ptr, rb.ptr, count, h, op, WORLD)
    assert rc == 0, (case["id"], rc)
    return rb.download(np.uint8, count=count * ext)


def scan_batch(L, case, rank):
    """Many blocking MPI_Scan / MPI_Exscan calls (case["cases"], each with the fields of a "scan" case)
    on one send and one receive buffer allocated once; the receive buffer is refilled with 0xA5 before
    every call.  Returns every call's receive buffer concatenated: one file per rank."""
    subs = case["cases"]
    cap = max(sub["count"] * TYPES[sub["type"]][3] for sub in subs)
    sb, rb = m.DeviceBuffer(cap), m.DeviceBuffer(cap)
    fill = np.full(cap, FILL, dtype=np.uint8)
    parts = []
    for sub in subs:
        h, ext, count = TYPES[sub["type"]][0], TYPES[sub["type"]][3], sub["count"]
        sb.upload(inputs(sub, rank))
        rb.upload(fill[:count * ext])
        rc = (L.MPI_Exscan if sub["coll"] == "exscan" else L.MPI_Scan)(sb.ptr, rb.ptr, count, h, OPS[sub["op"]], WORLD)
        assert rc == 0, (sub["id"], rc)
        parts.append(rb.download(np.uint8, count=count * ext))
    return np.concatenate(parts)


def main():
    spec = json.load(open(sys.argv[1]))
    out = sys.argv[2]
    rank = int(os.environ["RANK"])
    n = int(os.environ["WORLD_SIZE"])
    L = m.lib()
    m.check(L.MPI_Init(None, None), "MPI_Init")
    L.MPI_Comm_set_errhandler(WORLD, 0x54000001)  # MPI_ERRORS_RETURN
    for case in spec["cases"]:
        k = case["kind"]
        t = case.get("type", "MPI_FLOAT")
        h, ext = TYPES[t][0], TYPES[t][3]
        count = case.get("count", 0)
        if k == "scan":
            res = scan_call(L, case, inputs(case, rank), h, OPS[case["op"]], count, ext)
        elif k == "scan_batch":
            res = scan_batch(L, case, rank)
        elif k == "user_scan":  # inout = 2 in + 3 inout on int32, commutative flag as the case says
            FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_int))

            def uop(inp, io, ln, dt):
                c = ln[0]
                a = np.ctypeslib.as_array((ctypes.c_int * c).from_address(inp))
                b = np.ctypeslib.as_array((ctypes.c_int * c).from_address(io))
                b[:] = a * 2 + b * 3
            cb = FN(uop)
            op = ctypes.c_int()
            L.MPI_Op_create(ctypes.cast(cb, ctypes.c_void_p), case["commute"], ctypes.byref(op))
            x = ((np.arange(count, dtype=np.int32) * 3 + rank * 5) % 11 - 4).astype(np.int32)
            res = scan_call(L, case, x, TYPES["MPI_INT"][0], op.value, count, 4)
            L.MPI_Op_free(ctypes.byref(op))
        elif k == "scan_seq":
            # back-to-back MPI_Scan calls, fresh operands per call, counts alternating between the
            # one-shot and the pipelined kernel; the top rank and rank 0 fall behind before some
            # calls, so the others run ahead as far as the arena reuse protocol lets them
            parts = []
            for i, c in enumerate(case["counts"]):
                call = i + 1
                if (rank == n - 1 and call in case["late_top"]) or (rank == 0 and call in case["late_zero"]):
                    time.sleep(0.03)
                sub = dict(case, count=c, coll="scan")
                parts.append(scan_call(L, sub, inputs(sub, rank, call), h, OPS[case["op"]], c, ext))
            res = np.concatenate(parts)
        elif k == "exscan_ag_seq":
            # a pipelined MPI_Exscan of several rounds, then a pipelined MPI_Allgather, repeated:
            # rank 0 has no Exscan result, gathers nothing and runs ahead into the allgather, whose
            # first act is to write its block into every peer's gather slot
            parts = []
            for i in range(case["repeats"]):
                if rank == n - 1 and i in case["late_top"]:
                    time.sleep(0.03)
                sub = dict(case, count=case["count"], coll="exscan")
                parts.append(scan_call(L, sub, inputs(sub, rank, 2 * i), h, OPS[case["op"]], count, ext))
                agc = case["ag_count"]
                sub = dict(case, count=agc)
                sb = m.DeviceBuffer.from_array(inputs(sub, rank, 2 * i + 1))
                rb = m.DeviceBuffer(n * agc * ext)
                rb.upload(np.full(n * agc * ext, FILL, dtype=np.uint8))
                assert L.MPI_Allgather(sb.ptr, agc, h, rb.ptr, agc, h, WORLD) == 0
                parts.append(rb.download(np.uint8, count=n * agc * ext))
            res = np.concatenate(parts)
        elif k == "scan_multinode":
            # a job over several nodes: both calls are refused with MPI_ERR_OTHER's class
            sb = m.DeviceBuffer.from_array(np.ones(8, dtype=np.float32))
            rb = m.DeviceBuffer(32)
            F, SUM = TYPES["MPI_FLOAT"][0], OPS["MPI_SUM"]
            req = ctypes.c_int()
            rcs = [L.MPI_Scan(sb.ptr, rb.ptr, 8, F, SUM, WORLD), L.MPI_Exscan(sb.ptr, rb.ptr, 8, F, SUM, WORLD),
                   L.MPI_Iscan(sb.ptr, rb.ptr, 8, F, SUM, WORLD, ctypes.byref(req)),
                   L.mv2h_scan(sb.ptr, rb.ptr, 8, F, SUM, None), L.mv2h_exscan(sb.ptr, rb.ptr, 8, F, SUM, None)]
            res = np.array(rcs, dtype=np.int64)
        elif k == "info":
            res = np.array([m.info(key) for key in case["keys"]], dtype=np.int64)
        else:
            raise ValueError(k)
        np.save(os.path.join(out, f"{case['id']}_r{rank}.npy"), res)
    L.MPI_Finalize()
    print(f"rank {rank} done", flush=True)


if __name__ == "__main__":
    main()

"""One rank of the multi-process MPI_Gather(v) / MPI_Scatter(v) / MPI_Allgatherv GPU tests (launched
by tests/test_gpu_gather_mp.py; several ranks may share one GPU).  Runs every case of the spec
through the MPI API and saves, per case, the bytes of its receive buffer with the 64 guard bytes of
0xA5 before and after it (or the return code where the case expects a failure), and by how much the
eight path counters (mv2h_get_info gv_* and a2a_*) rose."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mvapich2_amd as m  # noqa: E402
from mvapich2_amd.consts import OPS, TYPES  # noqa: E402
from tests.mp_alltoall_worker import FILL, IN_PLACE, WORLD, Guarded, P, ints, send_bytes  # noqa: E402

PATH_KEYS = ("gv_oneshot_vec", "gv_oneshot_bytes", "gv_pipe", "gv_pipe_shift",
             "a2a_oneshot_vec", "a2a_oneshot_bytes", "a2a_pipe", "a2a_pipe_shift")
NULL = P(None)


def vext(count):
    """extent in bytes of MPI_Type_vector(count, 1, 3, MPI_FLOAT)"""
    return ((count - 1) * 3 + 1) * 4


def vector_type(L, count):
    t = ctypes.c_int()
    assert L.MPI_Type_vector(count, 1, 3, TYPES["MPI_FLOAT"][0], ctypes.byref(t)) == 0
    assert L.MPI_Type_commit(ctypes.byref(t)) == 0
    return t


def send_buffer(x, variant):
    """(keep-alive object, address) of a send buffer holding x"""
    if variant == "host_send":
        keep = np.concatenate([x, np.zeros(16, np.uint8)])
        return keep, keep.ctypes.data
    if variant == "send_off4":
        keep = m.DeviceBuffer.from_array(np.concatenate([np.zeros(4, np.uint8), x, np.zeros(16, np.uint8)]))
        return keep, keep.ptr + 4
    keep = m.DeviceBuffer.from_array(np.concatenate([x, np.zeros(16, np.uint8)]))
    return keep, keep.ptr


def recv_buffer(nbytes, variant, init=None):
    return Guarded(nbytes, host=variant == "host_recv", shift=4 if variant == "recv_off4" else 0, init=init)


def call(L, name, args, variant):
    """MPI_<name>(*args), or MPI_I<name> + MPI_Wait"""
    if variant != "nonblocking":
        return getattr(L, "MPI_" + name)(*args)
    req = ctypes.c_int()
    rc = getattr(L, "MPI_I" + name.lower())(*args, ctypes.byref(req))
    return rc if rc else L.MPI_Wait(ctypes.byref(req), None)


def span(counts, displs, ext):
    return ext * max([d + c for c, d in zip(counts, displs)] + [1])


def allgatherv_case(L, case, rank, n):
    variant = case.get("variant", "plain")
    h, ext = TYPES[case["type"]][0], TYPES[case["type"]][3]
    m.check(L.mv2h_set_tuning(b"agv_via_a2a", int(bool(case.get("via_a2a")))), "agv_via_a2a")
    if variant == "vector":  # one vector per rank on the receive side, count floats on the send side
        c = case["count"]
        vt = vector_type(L, c)
        x = send_bytes(case["seed"], rank, 4 * c)
        rb = recv_buffer(n * vext(c), variant)
        keep, sp = send_buffer(x, variant)
        rc = L.MPI_Allgatherv(P(sp), c, h, P(rb.ptr), ints([1] * n), ints(list(range(n))), vt.value, WORLD)
        L.MPI_Type_free(ctypes.byref(vt))
    else:
        counts, displs = case["counts"], case["displs"][rank]
        x = send_bytes(case["seed"], rank, ext * counts[rank])
        rlen = span(counts, displs, ext)
        init = None
        if variant == "inplace":
            init = np.full(rlen, FILL, dtype=np.uint8)
            init[ext * displs[rank]:ext * (displs[rank] + counts[rank])] = x
        rb = recv_buffer(rlen, variant, init)
        keep, sp = send_buffer(x, variant)
        args = [P(sp), counts[rank], h, P(rb.ptr), ints(counts), ints(displs), h, WORLD]
        if variant == "inplace":
            args[:3] = [IN_PLACE, 0, 0]
        rc = call(L, "Allgatherv", args, variant)
    m.check(L.mv2h_set_tuning(b"agv_via_a2a", 0), "agv_via_a2a")
    assert rc == case.get("expect_rc", 0), (case["id"], rc)
    return rb.frame()


def gather_case(L, case, rank, n):
    """MPI_Gather (no "counts") or MPI_Gatherv; every rank has a guarded receive buffer, which only
    the root may see written; Gatherv's non-roots pass a null receive buffer"""
    variant, root = case.get("variant", "plain"), case["root"]
    h, ext = TYPES[case.get("type", "MPI_FLOAT")][0], TYPES[case.get("type", "MPI_FLOAT")][3]
    at_root = rank == root
    vt = None
    if "counts" in case:
        counts, displs = case["counts"], case["displs"]
        mine = counts[rank] + case.get("extra", {}).get(str(rank), 0)
        rlen = span(counts, displs, ext)
    else:
        counts = displs = None
        mine = case["count"]
        rlen = n * mine * ext
    rtype = h
    if variant == "vector":
        vt = vector_type(L, mine)
        rtype, rlen = vt.value, n * vext(mine)
    x = send_bytes(case["seed"], rank, ext * mine)
    init = None
    if variant == "inplace" and at_root:
        init = np.full(rlen, FILL, dtype=np.uint8)
        o = ext * (displs[rank] if displs else rank * mine)
        init[o:o + ext * mine] = x
    rb = recv_buffer(rlen, variant if at_root else "plain", init)
    keep, sp = send_buffer(x, variant)
    send = [IN_PLACE, 0, 0] if variant == "inplace" and at_root else [P(sp), mine, h]
    if counts is None:
        rcount = 1 if variant == "vector" else mine
        rc = call(L, "Gather", send + [P(rb.ptr), rcount, rtype, root, WORLD], variant)
    else:
        if variant == "vector":
            counts, displs = [1] * n, list(range(n))
        rp = P(rb.ptr) if at_root else NULL
        rc = call(L, "Gatherv", send + [rp, ints(counts), ints(displs), rtype, root, WORLD], variant)
    if vt is not None:
        L.MPI_Type_free(ctypes.byref(vt))
    assert rc == case.get("expect_rc", 0), (case["id"], rc)
    return rb.frame()


def scatter_case(L, case, rank, n):
    """MPI_Scatter (no "counts") or MPI_Scatterv; non-roots pass a null send buffer"""
    variant, root = case.get("variant", "plain"), case["root"]
    h, ext = TYPES[case.get("type", "MPI_FLOAT")][0], TYPES[case.get("type", "MPI_FLOAT")][3]
    at_root = rank == root
    vt = None
    if "counts" in case:
        counts, displs = case["counts"], case["displs"]
        mine = counts[rank] + case.get("extra", {}).get(str(rank), 0)
        slen = span(counts, displs, ext)
    else:
        counts = displs = None
        mine = case["count"]
        slen = n * mine * ext
    stype = h
    if variant == "vector":
        vt = vector_type(L, mine)
        stype, slen = vt.value, n * vext(mine)
    keep, sp = (None, None)
    if at_root:
        keep, sp = send_buffer(send_bytes(case["seed"], root, slen), variant)
    rb = recv_buffer(max(ext * mine, 1), variant)
    recv = [IN_PLACE, 0, 0] if variant == "inplace" and at_root else [P(rb.ptr), mine, h]
    if counts is None:
        scount = 1 if variant == "vector" else mine
        rc = call(L, "Scatter", [P(sp) if at_root else NULL, scount, stype] + recv + [root, WORLD], variant)
    else:
        if variant == "vector":
            counts, displs = [1] * n, list(range(n))
        rc = call(L, "Scatterv", [P(sp) if at_root else NULL, ints(counts), ints(displs), stype] + recv + [root, WORLD],
                  variant)
    if vt is not None:
        L.MPI_Type_free(ctypes.byref(vt))
    assert rc == case.get("expect_rc", 0), (case["id"], rc)
    return rb.frame()


def sequence_case(L, case, rank, n):
    """calls back to back in one job, cycling through gather (root = i mod n), scatter, allgatherv,
    alltoall and allreduce and through the block sizes; the frames of all of them, in order"""
    F, SUM = TYPES["MPI_FLOAT"][0], OPS["MPI_SUM"]
    frames = []
    for i in range(case["calls"]):
        c, op, seed, root = case["counts"][i % len(case["counts"])], i % 5, case["seed"] + i, i % n
        if op == 0:
            sb = m.DeviceBuffer.from_array(send_bytes(seed, rank, 4 * c))
            rb = Guarded(4 * c * n)
            rc = L.MPI_Gather(P(sb.ptr), c, F, P(rb.ptr) if rank == root else NULL, c, F, root, WORLD)
        elif op == 1:
            sb = m.DeviceBuffer.from_array(send_bytes(seed, root, 4 * c * n)) if rank == root else None
            rb = Guarded(4 * c)
            rc = L.MPI_Scatter(P(sb.ptr) if sb else NULL, c, F, P(rb.ptr), c, F, root, WORLD)
        elif op == 2:
            sb = m.DeviceBuffer.from_array(send_bytes(seed, rank, 4 * c))
            rb = Guarded(4 * c * n)
            rc = L.MPI_Allgatherv(P(sb.ptr), c, F, P(rb.ptr), ints([c] * n), ints([c * j for j in range(n)]), F, WORLD)
        elif op == 3:
            sb = m.DeviceBuffer.from_array(send_bytes(seed, rank, 4 * c * n))
            rb = Guarded(4 * c * n)
            rc = L.MPI_Alltoall(P(sb.ptr), c, F, P(rb.ptr), c, F, WORLD)
        else:
            sb = m.DeviceBuffer.from_array(np.full(c, rank + 1, dtype=np.float32))
            rb = Guarded(4 * c)
            rc = L.MPI_Allreduce(P(sb.ptr), P(rb.ptr), c, F, SUM, WORLD)
        assert rc == 0, (i, op, c, rc)
        frames.append(rb.frame())
    return np.concatenate(frames)


def multinode_case(L, rank, n):
    """a job over several nodes: the five calls and the five C-ABI entries are refused"""
    F = TYPES["MPI_FLOAT"][0]
    sb = m.DeviceBuffer.from_array(np.ones(4 * n, dtype=np.float32))
    rb = m.DeviceBuffer(16 * n)
    c, d = ints([4] * n), ints([4 * j for j in range(n)])
    z = (ctypes.c_size_t * n)(*([16] * n))
    zo = (ctypes.c_size_t * n)(*[16 * j for j in range(n)])
    s, r = P(sb.ptr), P(rb.ptr)
    return np.array([L.MPI_Gather(s, 4, F, r, 4, F, 0, WORLD), L.MPI_Gatherv(s, 4, F, r, c, d, F, 0, WORLD),
                     L.MPI_Scatter(s, 4, F, r, 4, F, 0, WORLD), L.MPI_Scatterv(s, c, d, F, r, 4, F, 0, WORLD),
                     L.MPI_Allgatherv(s, 4, F, r, c, d, F, WORLD),
                     L.mv2h_gather(s, r, 16, 0, None), L.mv2h_gatherv(s, 16, r, z, zo, 0, None),
                     L.mv2h_scatter(s, r, 16, 0, None), L.mv2h_scatterv(s, z, zo, r, 16, 0, None),
                     L.mv2h_allgatherv(s, 16, r, z, zo, None)], dtype=np.int64)


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
        before = [m.info(key) for key in PATH_KEYS]
        if k == "allgatherv":
            res = allgatherv_case(L, case, rank, n)
        elif k in ("gather", "gatherv"):
            res = gather_case(L, case, rank, n)
        elif k in ("scatter", "scatterv"):
            res = scatter_case(L, case, rank, n)
        elif k == "sequence":
            res = sequence_case(L, case, rank, n)
        elif k == "multinode":
            res = multinode_case(L, rank, n)
        elif k == "info":
            res = np.array([m.info(key) for key in case["keys"]], dtype=np.int64)
        else:
            raise ValueError(k)
        np.save(os.path.join(out, f"{case['id']}_r{rank}.npy"), res)
        np.save(os.path.join(out, f"{case['id']}_paths_r{rank}.npy"),
                np.array([m.info(key) - b for key, b in zip(PATH_KEYS, before)], dtype=np.int64))
    m.check(L.MPI_Finalize(), "MPI_Finalize")
    print(f"rank {rank} done", flush=True)


if __name__ == "__main__":
    main()

"""One rank of the multi-process MPI_Alltoall / MPI_Alltoallv GPU tests (launched by
tests/test_gpu_alltoall_mp.py; several ranks may share one GPU).  Runs every case of the spec
through the MPI API and saves, per case, the bytes of its receive buffer with the 64 guard bytes
of 0xA5 before and after it, and by how much the four path counters (mv2h_get_info a2a_*) rose."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mvapich2_amd as m  # noqa: E402
from mvapich2_amd.consts import OPS, TYPES  # noqa: E402

WORLD = 0x44000000
IN_PLACE = ctypes.c_void_p(-1 & 0xFFFFFFFFFFFFFFFF)
FILL, GUARD = 0xA5, 64
PATH_KEYS = ("a2a_oneshot_vec", "a2a_oneshot_bytes", "a2a_pipe", "a2a_pipe_shift")
P = ctypes.c_void_p


def send_bytes(seed, rank, nbytes):
    """rank's send buffer of a case: the test recomputes it"""
    return np.random.default_rng(seed * 1000 + rank).integers(0, 256, nbytes, dtype=np.uint8)


def ints(v):
    return (ctypes.c_int * len(v))(*v)


class Guarded:
    """nbytes of receive buffer between two guards of 0xA5, `shift` bytes off a 16-byte boundary,
    in device memory or (host=True) in a numpy array"""

    def __init__(self, nbytes, host=False, shift=0, init=None):
        self.nbytes, self.shift, self.host = nbytes, shift, host
        frame = np.full(shift + GUARD + nbytes + GUARD, FILL, dtype=np.uint8)
        if init is not None:
            frame[shift + GUARD:shift + GUARD + nbytes] = init
        if host:
            self.arr = frame
            base = frame.ctypes.data
        else:
            self.buf = m.DeviceBuffer.from_array(frame)
            base = self.buf.ptr
        self.ptr = base + shift + GUARD

    def frame(self):
        """guard + data + guard"""
        if self.host:
            return self.arr[self.shift:].copy()
        return self.buf.download(np.uint8, count=GUARD + self.nbytes + GUARD, offset=self.shift)


def alltoall_case(L, hip, case, rank, n):
    h, ext = TYPES[case["type"]][0], TYPES[case["type"]][3]
    count, variant = case["count"], case.get("variant", "plain")
    blk = count * ext
    x = send_bytes(case["seed"], rank, blk * n)
    rb = Guarded(blk * n, host=variant == "host_recv", shift=4 if variant == "recv_off4" else 0,
                 init=x if variant == "inplace" else None)
    if variant == "host_send":
        keep = x.copy()
        sp = keep.ctypes.data
    elif variant == "send_off4":
        keep = m.DeviceBuffer.from_array(np.concatenate([np.zeros(4, np.uint8), x]))
        sp = keep.ptr + 4
    else:
        keep = m.DeviceBuffer.from_array(x)
        sp = keep.ptr
    if variant == "inplace":
        rc = L.MPI_Alltoall(IN_PLACE, 0, 0, P(rb.ptr), count, h, WORLD)
    elif variant == "nonblocking":
        req = ctypes.c_int()
        rc = L.MPI_Ialltoall(P(sp), count, h, P(rb.ptr), count, h, WORLD, ctypes.byref(req))
        if rc == 0:
            rc = L.MPI_Wait(ctypes.byref(req), None)
    elif variant == "enqueue":
        # on the caller's stream, followed by a copy of the result that depends on it
        st = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(st)) == 0
        dep = m.DeviceBuffer(blk * n)
        rc = L.MPIX_Alltoall_enqueue(P(sp), count, h, P(rb.ptr), count, h, WORLD, st)
        assert hip.hipMemcpyAsync(P(dep.ptr), P(rb.ptr), ctypes.c_size_t(blk * n), 3, st) == 0  # device to device
        assert hip.hipStreamSynchronize(st) == 0
        assert L.MPIX_Enqueue_check(WORLD) == 0
        hip.hipStreamDestroy(st)
        frame = rb.frame()
        assert np.array_equal(frame[GUARD:GUARD + blk * n], dep.download(np.uint8)), "the dependent copy differs"
    else:
        rc = L.MPI_Alltoall(P(sp), count, h, P(rb.ptr), count, h, WORLD)
    assert rc == 0, (case["id"], rc)
    return rb.frame()


def derived_case(L, case, rank, n):
    """count floats per block, every second float of the buffer on the `side` that is a vector type
    (MPI_Type_vector(count, 1, 2, MPI_FLOAT) resized to 8 * count bytes so that blocks follow on)"""
    F = TYPES["MPI_FLOAT"][0]
    count, side = case["count"], case["side"]
    vt, t = ctypes.c_int(), ctypes.c_int()
    assert L.MPI_Type_vector(count, 1, 2, F, ctypes.byref(vt)) == 0
    assert L.MPI_Type_create_resized(vt, 0, 8 * count, ctypes.byref(t)) == 0
    assert L.MPI_Type_commit(ctypes.byref(t)) == 0
    sbytes = (8 if side == "send" else 4) * count * n
    rbytes = (8 if side == "recv" else 4) * count * n
    sb = m.DeviceBuffer.from_array(send_bytes(case["seed"], rank, sbytes))
    rb = Guarded(rbytes)
    if side == "send":
        rc = L.MPI_Alltoall(P(sb.ptr), 1, t.value, P(rb.ptr), count, F, WORLD)
    else:
        rc = L.MPI_Alltoall(P(sb.ptr), count, F, P(rb.ptr), 1, t.value, WORLD)
    assert rc == 0, (case["id"], rc)
    L.MPI_Type_free(ctypes.byref(t))
    L.MPI_Type_free(ctypes.byref(vt))
    return rb.frame()


def sequence_case(L, hip, case, rank, n):
    """back-to-back calls on one stream without host synchronisation between them: all-to-alls of
    alternating block sizes with one allreduce and one allgather in between"""
    F, SUM = TYPES["MPI_FLOAT"][0], OPS["MPI_SUM"]
    st = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(st)) == 0
    bufs, keep = [], []
    for i, count in enumerate(case["counts"]):
        sb = m.DeviceBuffer.from_array(send_bytes(case["seed"] + i, rank, 4 * count * n))
        rb = Guarded(4 * count * n)
        assert L.MPIX_Alltoall_enqueue(P(sb.ptr), count, F, P(rb.ptr), count, F, WORLD, st) == 0
        bufs.append(rb)
        keep.append(sb)
        if i == case["allreduce_after"]:
            c = case["ar_count"]
            sb = m.DeviceBuffer.from_array(np.full(c, rank + 1, dtype=np.float32))
            rb = Guarded(4 * c)
            assert L.MPIX_Allreduce_enqueue(P(sb.ptr), P(rb.ptr), c, F, SUM, WORLD, st) == 0
        elif i == case["allgather_after"]:
            c = case["ag_count"]
            sb = m.DeviceBuffer.from_array(send_bytes(case["seed"] + 100, rank, 4 * c))
            rb = Guarded(4 * c * n)
            assert L.MPIX_Allgather_enqueue(P(sb.ptr), c, F, P(rb.ptr), c, F, WORLD, st) == 0
        else:
            continue
        bufs.append(rb)
        keep.append(sb)
    assert hip.hipStreamSynchronize(st) == 0
    assert L.MPIX_Enqueue_check(WORLD) == 0
    hip.hipStreamDestroy(st)
    return np.concatenate([b.frame() for b in bufs])


def alltoallv_case(L, case, rank, n):
    """counts and displacements in floats, per rank, as the case gives them; returns the frame, or
    the return code where the case expects a failure"""
    F = TYPES["MPI_FLOAT"][0]
    sc, sd, rc_, rd = (case[k][rank] for k in ("scounts", "sdispls", "rcounts", "rdispls"))
    variant = case.get("variant", "plain")
    slen = 4 * max([d + c for c, d in zip(sc, sd)] + [1])
    rlen = 4 * max([d + c for c, d in zip(rc_, rd)] + [1])
    x = send_bytes(case["seed"], rank, max(slen, rlen))
    rb = Guarded(rlen, host=variant == "host_recv", init=x[:rlen] if variant == "inplace" else None)
    sb = m.DeviceBuffer.from_array(x[:slen])
    if variant == "inplace":
        rc = L.MPI_Alltoallv(IN_PLACE, None, None, 0, P(rb.ptr), ints(rc_), ints(rd), F, WORLD)
    elif variant == "nonblocking":
        req = ctypes.c_int()
        rc = L.MPI_Ialltoallv(P(sb.ptr), ints(sc), ints(sd), F, P(rb.ptr), ints(rc_), ints(rd), F, WORLD, ctypes.byref(req))
        if rc == 0:
            rc = L.MPI_Wait(ctypes.byref(req), None)
    else:
        rc = L.MPI_Alltoallv(P(sb.ptr), ints(sc), ints(sd), F, P(rb.ptr), ints(rc_), ints(rd), F, WORLD)
    assert rc == case.get("expect_rc", 0), (case["id"], rc)
    return rb.frame()


def main():
    spec = json.load(open(sys.argv[1]))
    out = sys.argv[2]
    rank = int(os.environ["RANK"])
    n = int(os.environ["WORLD_SIZE"])
    L = m.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    m.check(L.MPI_Init(None, None), "MPI_Init")
    L.MPI_Comm_set_errhandler(WORLD, 0x54000001)  # MPI_ERRORS_RETURN
    for case in spec["cases"]:
        k = case["kind"]
        before = [m.info(key) for key in PATH_KEYS]
        if k == "alltoall":
            res = alltoall_case(L, hip, case, rank, n)
        elif k == "derived":
            res = derived_case(L, case, rank, n)
        elif k == "sequence":
            res = sequence_case(L, hip, case, rank, n)
        elif k == "alltoallv":
            res = alltoallv_case(L, case, rank, n)
        elif k == "multinode":
            # a job over several nodes: both calls and both C-ABI entries are refused
            F = TYPES["MPI_FLOAT"][0]
            sb = m.DeviceBuffer.from_array(np.ones(4 * n, dtype=np.float32))
            rb = m.DeviceBuffer(16 * n)
            c, d = ints([4] * n), ints([4 * j for j in range(n)])
            z = (ctypes.c_size_t * n)(*([16] * n))
            zo = (ctypes.c_size_t * n)(*[16 * j for j in range(n)])
            res = np.array([L.MPI_Alltoall(P(sb.ptr), 4, F, P(rb.ptr), 4, F, WORLD),
                            L.MPI_Alltoallv(P(sb.ptr), c, d, F, P(rb.ptr), c, d, F, WORLD),
                            L.mv2h_alltoall(P(sb.ptr), P(rb.ptr), 16, None),
                            L.mv2h_alltoallv(P(sb.ptr), z, zo, P(rb.ptr), z, zo, None)], dtype=np.int64)
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

"""One rank of the multi-process MPI_Alltoallw GPU tests (launched by tests/test_gpu_alltoallw_mp.py;
several ranks may share one GPU), and the model both sides of the test share.

Buffers are float32 arrays.  A block of an Alltoallw side is a dict: "t" names its datatype (below),
"disp" its displacement in floats; block_index() lists the floats it covers in pack order, which is
all the test needs to predict a receive buffer.  An Alltoallv side ("v" cases) has one element type,
three floats either strided by two ("vec") or back to back ("plain"), and counts / displacements in
elements.  Every case runs with the batched pack and, where `twin` is set, again with
mv2h_set_tuning("pack_blocks", 0); per run the worker saves the return code, the receive buffer
between its guards and by how much pack_blocks_calls and a2a_pipe rose."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mvapich2_amd as m  # noqa: E402
from mvapich2_amd.consts import TYPES  # noqa: E402

WORLD = 0x44000000
IN_PLACE = ctypes.c_void_p(-1 & 0xFFFFFFFFFFFFFFFF)
FILL, GUARD = -7777.0, 16  # floats
P = ctypes.c_void_p
F = TYPES["MPI_FLOAT"][0]
COUNTERS = ("pack_blocks_calls", "a2a_pipe")
VEC_ELEM = 3  # floats per element of a "v" case


def send_floats(seed, rank, n):
    """rank's send buffer of a case: float j is unique over (rank, j)"""
    return (seed * 1e6 + rank * 1e5 + np.arange(n)).astype(np.float32)


def indexed_blocks(n):
    """(lens, displs) of the "indexed" type of n floats: blocks of 1, 2, 3, 1, ... floats, one apart"""
    lens, displs, at, k = [], [], 0, 0
    while sum(lens) < n:
        ln = min(1 + k % 3, n - sum(lens))
        lens.append(ln)
        displs.append(at)
        at += ln + 1
        k += 1
    return lens, displs


def block_floats(b):
    """(count, floats of one element in pack order, extent in floats) of a block's datatype"""
    t = b["t"]
    if t == "contig":  # b["n"] MPI_FLOATs
        return b["n"], np.arange(1), 1
    if t == "zero":    # one element of MPI_Type_contiguous(0)
        return 1, np.arange(0), 0
    if t == "vector":  # MPI_Type_vector(n, 1, 2)
        return 1, 2 * np.arange(b["n"]), max(2 * b["n"] - 1, 0)
    if t == "indexed":
        lens, displs = indexed_blocks(b["n"])
        one = np.concatenate([d + np.arange(ln) for ln, d in zip(lens, displs)]) if lens else np.arange(0)
        return 1, one, (displs[-1] + lens[-1]) if lens else 0
    if t == "cols":    # b["count"] columns of a rows x ld matrix: MPI_Type_vector(rows, 1, ld) resized to one float
        return b["count"], b["ld"] * np.arange(b["rows"]), 1
    if t == "sub":     # a rows x cols corner of a matrix with rows of ld floats: MPI_Type_vector(rows, cols, ld)
        return 1, (b["ld"] * np.arange(b["rows"])[:, None] + np.arange(b["cols"])[None, :]).ravel(), 0
    raise ValueError(t)


def block_index(b):
    count, one, ext = block_floats(b)
    if not count or not one.size:
        return np.arange(0)
    return (b["disp"] + ext * np.arange(count)[:, None] + one[None, :]).ravel()


def block_plain(b):
    """the library leaves a side alone when every non-empty block's type is contiguous"""
    count, one, _ = block_floats(b)
    return not count or b["t"] in ("contig", "zero") or (one.size <= 1) or \
        (b["t"] == "sub" and (b["rows"] <= 1 or b["cols"] == b["ld"])) or (b["t"] == "cols" and b["rows"] <= 1)


def side_span(blocks):
    return max([int(block_index(b).max()) + 1 for b in blocks if block_index(b).size] + [1])


def v_index(kind, count, disp):
    """floats of `count` elements at `disp` elements of an Alltoallv side"""
    if kind == "vec":  # MPI_Type_vector(3, 1, 2) resized to 6 floats
        return (6 * (disp + np.arange(count))[:, None] + 2 * np.arange(VEC_ELEM)[None, :]).ravel()
    return VEC_ELEM * disp + np.arange(VEC_ELEM * count)


def ints(v):
    return (ctypes.c_int * max(len(v), 1))(*v)


class Types:
    """the datatypes of one case; freed together"""

    def __init__(self, L):
        self.L, self.made = L, []

    def new(self, fn, *args):
        t = ctypes.c_int()
        assert getattr(self.L, fn)(*args, ctypes.byref(t)) == 0, fn
        self.made.append(t)
        return t.value

    def commit(self, t):
        c = ctypes.c_int(t)
        assert self.L.MPI_Type_commit(ctypes.byref(c)) == 0
        return t

    def of(self, b):
        t = b["t"]
        if t == "contig":
            return F, b["n"]
        if t == "zero":
            return self.commit(self.new("MPI_Type_contiguous", 0, F)), 1
        if t == "vector":
            return self.commit(self.new("MPI_Type_vector", b["n"], 1, 2, F)), 1
        if t == "indexed":
            lens, displs = indexed_blocks(b["n"])
            return self.commit(self.new("MPI_Type_indexed", len(lens), ints(lens), ints(displs), F)), 1
        if t == "cols":
            col = self.new("MPI_Type_vector", b["rows"], 1, b["ld"], F)
            return self.commit(self.new("MPI_Type_create_resized", col, 0, 4)), b["count"]
        if t == "sub":
            return self.commit(self.new("MPI_Type_vector", b["rows"], b["cols"], b["ld"], F)), 1
        raise ValueError(t)

    def vec_elem(self):
        v = self.new("MPI_Type_vector", VEC_ELEM, 1, 2, F)
        return self.commit(self.new("MPI_Type_create_resized", v, 0, 24))

    def plain_elem(self):
        return self.commit(self.new("MPI_Type_contiguous", VEC_ELEM, F))

    def free(self):
        for t in reversed(self.made):
            self.L.MPI_Type_free(ctypes.byref(t))


def framed(data):
    g = np.full(GUARD, FILL, dtype=np.float32)
    return np.concatenate([g, data.astype(np.float32), g])


def run_case(L, case, rank, n):
    """(rc, frame of the receive buffer)"""
    variant, ty = case.get("variant", "plain"), Types(L)
    if case["kind"] == "w":
        sb_, rb_ = case["send"][rank], case["recv"][rank]
        slen, rlen = side_span(sb_), side_span(rb_)
        st = [ty.of(b) for b in sb_]
        rt = [ty.of(b) for b in rb_]
        sargs = (ints([c for _, c in st]), ints([4 * b["disp"] for b in sb_]), ints([t for t, _ in st]))
        rargs = (ints([c for _, c in rt]), ints([4 * b["disp"] for b in rb_]), ints([t for t, _ in rt]))
        call, icall = L.MPI_Alltoallw, L.MPI_Ialltoallw
    else:
        sk, rk = case["sside"], case["rside"]
        sc, sd, rc_, rd = (case[k][rank] for k in ("scounts", "sdispls", "rcounts", "rdispls"))
        slen = max([int(v_index(sk, c, d).max()) + 1 for c, d in zip(sc, sd) if c] + [1])
        rlen = max([int(v_index(rk, c, d).max()) + 1 for c, d in zip(rc_, rd) if c] + [1])
        el = {"vec": ty.vec_elem, "plain": ty.plain_elem}
        sargs, rargs = (ints(sc), ints(sd), el[sk]()), (ints(rc_), ints(rd), el[rk]())
        call, icall = L.MPI_Alltoallv, L.MPI_Ialltoallv
    host = variant == "host"
    x = send_floats(case["seed"], rank, max(slen, rlen))
    r0 = framed(x[:rlen] if variant == "inplace" else np.full(rlen, FILL, dtype=np.float32))
    if host:
        skeep, rkeep = x[:slen].copy(), r0.copy()
        sp, rp = skeep.ctypes.data, rkeep.ctypes.data + 4 * GUARD
    else:
        skeep, rkeep = m.DeviceBuffer.from_array(x[:slen]), m.DeviceBuffer.from_array(r0)
        sp, rp = skeep.ptr, rkeep.ptr + 4 * GUARD
    if variant == "inplace":
        rc = call(IN_PLACE, None, None, None if case["kind"] == "w" else 0, P(rp), *rargs, WORLD)
    elif variant == "nonblocking":
        req = ctypes.c_int()
        rc = icall(P(sp), *sargs, P(rp), *rargs, WORLD, ctypes.byref(req))
        if rc == 0:
            rc = L.MPI_Wait(ctypes.byref(req), None)
    else:
        rc = call(P(sp), *sargs, P(rp), *rargs, WORLD)
    ty.free()
    return rc, (rkeep.copy() if host else rkeep.download(np.float32))


def timing_case(L, case, rank, n):
    """MPI_Alltoallw of the transpose types, `pair` packed bytes per pair: median and minimum of
    `iters` warm blocking calls in microseconds (host clock; a blocking call returns complete) with
    the batched pack and with the per-block route"""
    import time
    side = int(round((case["pair"] // 4) ** 0.5))  # every rank owns side rows; side x side floats per pair
    ld_s, ld_r = side * n, side * n
    ty = Types(L)
    col = ty.commit(ty.new("MPI_Type_create_resized", ty.new("MPI_Type_vector", side, 1, ld_s, F), 0, 4))
    sub = ty.commit(ty.new("MPI_Type_vector", side, side, ld_r, F))
    sb = m.DeviceBuffer.from_array(send_floats(1, rank, side * ld_s))
    rb = m.DeviceBuffer(4 * side * ld_r)
    sargs = (ints([side] * n), ints([4 * side * j for j in range(n)]), ints([col] * n))
    rargs = (ints([1] * n), ints([4 * side * j for j in range(n)]), ints([sub] * n))
    ts = {1: [], 0: []}
    for i in range(case["warmup"] + case["iters"]):
        for batched in (1, 0):  # the two routes alternate, so that both see the same neighbours on the GPU
            assert L.mv2h_set_tuning(b"pack_blocks", batched) == 0
            L.MPI_Barrier(WORLD)
            t0 = time.perf_counter()
            assert L.MPI_Alltoallw(P(sb.ptr), *sargs, P(rb.ptr), *rargs, WORLD) == 0
            ts[batched].append((time.perf_counter() - t0) * 1e6)
    out = []
    for batched in (1, 0):
        t = np.array(ts[batched][case["warmup"]:])
        out += [float(np.median(t)), float(t.min())]
    L.mv2h_set_tuning(b"pack_blocks", 1)
    got = rb.download(np.float32).reshape(side, ld_r)
    for j in range(n):  # the transpose, checked once
        a_j = send_floats(1, j, side * ld_s).reshape(side, ld_s)
        assert np.array_equal(got[:, side * j:side * (j + 1)], a_j[:, side * rank:side * (rank + 1)].T), j
    ty.free()
    return np.array(out)


def main():
    spec = json.load(open(sys.argv[1]))
    out = sys.argv[2]
    rank = int(os.environ["RANK"])
    n = int(os.environ["WORLD_SIZE"])
    L = m.lib()
    m.check(L.MPI_Init(None, None), "MPI_Init")
    L.MPI_Comm_set_errhandler(WORLD, 0x54000001)  # MPI_ERRORS_RETURN
    for case in spec["cases"]:
        save = lambda name, a: np.save(os.path.join(out, f"{case['id']}_{name}_r{rank}.npy"), a)  # noqa: E731
        if case["kind"] == "timing":
            save("us", timing_case(L, case, rank, n))
            continue
        if case["kind"] == "multinode":
            # several nodes: refused before any pack work
            before = m.info("pack_blocks_calls")
            ty = Types(L)
            vt = ty.commit(ty.new("MPI_Type_vector", 4, 1, 2, F))
            sb, rb = m.DeviceBuffer(64 * n), m.DeviceBuffer(64 * n)
            c, d, t = ints([1] * n), ints([32 * j for j in range(n)]), ints([vt] * n)
            req = ctypes.c_int()
            res = [L.MPI_Alltoallw(P(sb.ptr), c, d, t, P(rb.ptr), c, d, t, WORLD),
                   L.MPI_Ialltoallw(P(sb.ptr), c, d, t, P(rb.ptr), c, d, t, WORLD, ctypes.byref(req)),
                   L.MPI_Alltoallv(P(sb.ptr), c, ints(list(range(n))), vt, P(rb.ptr), c, ints(list(range(n))), vt, WORLD)]
            ty.free()
            save("mn", np.array(res + [m.info("pack_blocks_calls") - before], dtype=np.int64))
            continue
        restore = {key: m.info(key) for key in case.get("tuning", {})}
        for key, v in case.get("tuning", {}).items():
            assert L.mv2h_set_tuning(key.encode(), v) == 0, key
        for batched in (1, 0) if case.get("twin") else (1,):
            assert L.mv2h_set_tuning(b"pack_blocks", batched) == 0
            before = [m.info(k) for k in COUNTERS]
            rc, frame = run_case(L, case, rank, n)
            assert rc == case.get("expect_rc", 0), (case["id"], batched, rc)
            save(f"frame{batched}", frame)
            save(f"ctr{batched}", np.array([m.info(k) - b for k, b in zip(COUNTERS, before)], dtype=np.int64))
        L.mv2h_set_tuning(b"pack_blocks", 1)
        for key, v in restore.items():
            assert L.mv2h_set_tuning(key.encode(), v) == 0, key
    m.check(L.MPI_Finalize(), "MPI_Finalize")
    print(f"rank {rank} done", flush=True)


if __name__ == "__main__":
    main()

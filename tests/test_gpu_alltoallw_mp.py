"""MPI_Alltoallw / MPI_Ialltoallw and MPI_Alltoallv with derived types on device buffers, one process
per rank (the launch scheme of tests/test_gpu_alltoall_mp.py with tests/mp_alltoallw_worker.py as
the worker).  Every case names, per rank and per peer, a datatype and a displacement; the expected
receive buffer follows from the floats each type covers in pack order (the worker's block_index),
so nothing of the library is used to predict it.  Each rank count pays one MPI_Init and runs all
its cases inside it.  Cases with a derived type run twice, with the batched pack (one launch per
staged side, counted by pack_blocks_calls) and with mv2h_set_tuning("pack_blocks", 0) (one
MPI_Pack per block): the two receive buffers must be the same bytes.  Receive buffers lie between
two guards, which must come back intact."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from tests.mp_alltoallw_worker import (FILL, block_index, block_plain, framed, send_floats, side_span, v_index)
from tests.test_gpu_collectives_mp import GEOMS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPI_ERR_TRUNCATE, MPI_ERR_OTHER = 14, 15
NOTHING = {"t": "contig", "n": 0, "disp": 0}


def run_workers(n, cases, tmp_path, timeout=200, ppn=None):
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"cases": cases}))
    out = tmp_path / "out"
    out.mkdir()
    ppn = ppn or n
    boot = {}
    if ppn < n:
        import socket
        so = socket.socket()
        so.bind(("127.0.0.1", 0))
        boot = {"MV2AMD_BOOT_ADDR": "127.0.0.1", "MV2AMD_BOOT_PORT": str(so.getsockname()[1]), "MV2AMD_NSHARE": str(n)}
        timeout = max(timeout, 240)
        so.close()
    procs, jobid = [], "w" + uuid.uuid4().hex[:12]
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r % ppn), LOCAL_WORLD_SIZE=str(ppn),
                   MV2AMD_JOBID=jobid)
        env.update({"MV2AMD_TIMEOUT_S": "30", **boot, **GEOMS["small"]})
        env.pop("MV2AMD_DEVICE", None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_alltoallw_worker.py"), str(spec),
                                       str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            logs.append(o.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    bad = [r for r, p in enumerate(procs) if p.returncode != 0]
    assert not bad, "ranks " + ", ".join(f"{r} (rc {procs[r].returncode})" for r in bad) + " failed:\n" + \
        "\n".join(f"--- rank {r}:\n{logs[r][-2000:]}" for r in range(n))
    return (lambda cid, name, r: np.load(out / f"{cid}_{name}_r{r}.npy")), logs


# ---- the cases -------------------------------------------------------------------------------
def split(total, n):
    """block distribution: (first, length) per rank, the last block ragged or empty"""
    b = -(-total // n)
    return [(min(r * b, total), max(0, min(b, total - r * b))) for r in range(n)]


def transpose_case(n, seed, rows=20, cols=30, **kw):
    """rank r owns rows of a rows x cols matrix of floats and ends with rows of its transpose: the
    send type walks columns (a resized vector), the receive type is a corner of the local result"""
    rs, cs = split(rows, n), split(cols, n)
    send = [[{"t": "cols", "rows": rs[r][1], "ld": cols, "count": cs[j][1], "disp": cs[j][0]}
             if rs[r][1] and cs[j][1] else NOTHING for j in range(n)] for r in range(n)]
    recv = [[{"t": "sub", "rows": cs[j][1], "cols": rs[r][1], "ld": rows, "disp": rs[r][0]}
             if rs[r][1] and cs[j][1] else NOTHING for r in range(n)] for j in range(n)]
    return dict({"id": f"transpose{seed}", "kind": "w", "seed": seed, "send": send, "recv": recv, "twin": True}, **kw)


def typed(kind, nfloats, disp):
    if kind == "zero" or nfloats == 0:
        return {"t": "zero", "disp": disp} if kind == "zero" else NOTHING
    return {"t": kind, "n": nfloats, "disp": disp}


def w_case(cid, seed, n, floats, skind, rkind, gap=2, **kw):
    """floats(i, j) from rank i to rank j as skind(i, j) on the send side and rkind(i, j) on the
    receive side; displacements run on with `gap` floats between blocks"""
    def side(me, sending):
        blocks, at = [], 0
        for peer in range(n):
            i, j = (me, peer) if sending else (peer, me)
            k = (skind if sending else rkind)(i, j)
            b = typed(k, 0 if "zero" in (skind(i, j), rkind(i, j)) else floats(i, j), at)
            blocks.append(b)
            at = (side_span([b]) if block_index(b).size else at) + gap
        return blocks
    return dict({"id": cid, "kind": "w", "seed": seed, "send": [side(r, True) for r in range(n)],
                 "recv": [side(r, False) for r in range(n)]}, **kw)


KINDS = ("contig", "vector", "indexed", "zero")


def v_case(cid, seed, n, sside, rside, **kw):
    cnt = [[1 + (i + 2 * j) % 3 for j in range(n)] for i in range(n)]
    cnt[0][n - 1] = 0
    rc = [[cnt[j][i] for j in range(n)] for i in range(n)]
    run = lambda c: [sum(c[:j]) + j for j in range(n)]  # noqa: E731  (one element between blocks)
    return dict({"id": cid, "kind": "v", "seed": seed, "sside": sside, "rside": rside, "scounts": cnt, "rcounts": rc,
                 "sdispls": [run(cnt[i]) for i in range(n)], "rdispls": [run(rc[i]) for i in range(n)], "twin": True}, **kw)


def cases_for(n):
    mixed = dict(floats=lambda i, j: 5 + 3 * i + j, skind=lambda i, j: KINDS[(i + j) % 4],
                 rkind=lambda i, j: KINDS[(2 * i + j + 1) % 4])
    vec = lambda i, j: "vector"  # noqa: E731
    bad = w_case("trunc", 8, n, lambda i, j: 4 + i + j, vec, lambda i, j: "indexed", expect_rc=MPI_ERR_TRUNCATE)
    bad["recv"][2 % n][0]["n"] += 1  # one rank expects a float more than rank 0 sends it
    return [
        transpose_case(n, 1),
        w_case("mixed", 2, n, twin=True, **mixed),
        w_case("by_receiver", 3, n, lambda i, j: 2 * j, vec, lambda i, j: "indexed", twin=True),  # rank 0 receives nothing
        w_case("inplace_derived", 4, n, lambda i, j: 3 + (i + j) % 4, vec, vec, variant="inplace", twin=True),
        w_case("inplace_contig", 5, n, lambda i, j: 3 + (i + j) % 4, lambda i, j: "contig", lambda i, j: "contig",
               gap=3, variant="inplace"),
        w_case("all_contig", 6, n, lambda i, j: 1 + (3 * i + j) % 5, lambda i, j: "contig", lambda i, j: "contig", gap=1),
        v_case("v_send", 7, n, "vec", "plain"), v_case("v_recv", 7, n, "plain", "vec"), v_case("v_both", 7, n, "vec", "vec"),
        v_case("v_nb", 7, n, "vec", "vec", variant="nonblocking"),
        w_case("nonblocking", 9, n, variant="nonblocking", twin=True, **mixed),
        bad,
        w_case("pipelined", 5, n, lambda i, j: 3000 + i + j, vec, vec, twin=True, tuning={"oneshot_max": 4096}),
        w_case("host", 6, n, variant="host", **mixed),
        transpose_case(n, 2, rows=7, cols=5),  # fewer rows than ranks at 8: ranks with nothing to send
    ]


# ---- the model -------------------------------------------------------------------------------
def spans(case, r):
    if case["kind"] == "w":
        return side_span(case["send"][r]), side_span(case["recv"][r])
    ln = lambda k, cs, ds: max([int(v_index(k, c, d).max()) + 1 for c, d in zip(cs, ds) if c] + [1])  # noqa: E731
    return ln(case["sside"], case["scounts"][r], case["sdispls"][r]), ln(case["rside"], case["rcounts"][r], case["rdispls"][r])


def pair_index(case, i, j, inplace):
    """(floats rank i sends rank j, floats rank j receives them into)"""
    if case["kind"] == "w":
        return block_index((case["recv"] if inplace else case["send"])[i][j]), block_index(case["recv"][j][i])
    return (v_index(case["sside"], case["scounts"][i][j], case["sdispls"][i][j]),
            v_index(case["rside"], case["rcounts"][j][i], case["rdispls"][j][i]))


def expected(case, n):
    inplace = case.get("variant") == "inplace"
    xs = [send_floats(case["seed"], r, max(spans(case, r))) for r in range(n)]
    frames = []
    for j in range(n):
        rlen = spans(case, j)[1]
        want = xs[j][:rlen].copy() if inplace else np.full(rlen, FILL, dtype=np.float32)
        if not case.get("expect_rc"):
            for i in range(n):
                src, dst = pair_index(case, i, j, inplace)
                assert src.size == dst.size, (case["id"], i, j)
                want[dst] = xs[i][src]
        frames.append(framed(want))
    return frames


def launches(case, r):
    """batched launches of rank r: one per staged side that has bytes"""
    if case.get("variant") == "host":
        return 0
    if case["kind"] == "v":
        s = int(case["sside"] == "vec" and any(case["scounts"][r]))
        return s + int(case["rside"] == "vec" and any(case["rcounts"][r]))
    staged = lambda blocks: int(any(not block_plain(b) for b in blocks))  # noqa: E731
    if case.get("variant") == "inplace":
        return 2 * staged(case["recv"][r])
    return staged(case["send"][r]) + staged(case["recv"][r])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_alltoallw_multiprocess(n, tmp_path):
    cases = cases_for(n)
    get, _ = run_workers(n, cases, tmp_path)
    # the transpose against its closed form: B_j[c, r0 + i] = A_r[i, c0 + c], A_r[i, c] = 1e6 + r * 1e5 + 30 i + c
    t = cases[0]
    rs, cs = split(20, n), split(30, n)
    for j in range(n):
        got = get(t["id"], "frame1", j)[16:-16]
        for c in range(cs[j][1]):
            for r in range(n):
                for i in range(rs[r][1]):
                    assert got[c * 20 + rs[r][0] + i] == np.float32(1e6 + r * 1e5 + 30 * i + cs[j][0] + c), (j, c, r, i)
    assert n != 3 or (rs[2][1], cs[2][1]) == (6, 10)  # the ragged last block
    derived = 0
    for case in cases:
        want = expected(case, n)
        for r in range(n):
            f1 = get(case["id"], "frame1", r)
            assert np.array_equal(f1.view(np.uint8), want[r].view(np.uint8)), (case["id"], n, r)
            ctr = get(case["id"], "ctr1", r)
            if not case.get("expect_rc"):
                assert ctr[0] == launches(case, r), (case["id"], r, ctr)
            if case.get("twin"):
                f0 = get(case["id"], "frame0", r)
                assert np.array_equal(f0.view(np.uint8), f1.view(np.uint8)), (case["id"], n, r, "pack_blocks = 0 differs")
                assert get(case["id"], "ctr0", r)[0] == 0, (case["id"], r)
            if case["id"] == "pipelined":
                assert ctr[1] == 1 and get(case["id"], "ctr0", r)[1] == 1, (r, ctr)  # the exchange was the pipelined kernel
            elif case["id"] != "trunc":
                assert ctr[1] == 0, (case["id"], r, ctr)
        derived += case.get("twin", False) and any(launches(case, r) for r in range(n))
    assert derived >= 8
    # the counters' three values are all met: both sides derived, one side, none
    assert {launches(c, r) for c in cases for r in range(n)} >= {0, 1, 2}


@pytest.mark.timeout(300)
def test_alltoallw_refused_across_nodes(tmp_path):
    """4 ranks as 2 nodes of 2: MPI_Alltoallw, MPI_Ialltoallw and MPI_Alltoallv with a derived type
    return MPI_ERR_OTHER's class on every rank before any pack work, and MPI_Finalize succeeds"""
    get, logs = run_workers(4, [{"id": "mn", "kind": "multinode"}], tmp_path, ppn=2)
    for r in range(4):
        assert list(get("mn", "mn", r)) == [MPI_ERR_OTHER] * 3 + [0], r
        assert "only jobs on one node are supported" in logs[r]
        assert f"rank {r} done" in logs[r]

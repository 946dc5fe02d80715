"""MPI_Alltoall / MPI_Alltoallv on device buffers, one process per rank (the launch scheme of
tests/test_gpu_scan_mp.py with tests/mp_alltoall_worker.py as the worker).  The expected result
is a plain permutation: block j of rank r's receive buffer is block r of rank j's send buffer.

Every launch runs under the "small" pipeline geometry (3 workgroups x 4 KiB per round), so a
280,004-byte block takes 23 rounds and both slot parities are reused inside one call.  The path
each call took (one-shot by vectors, one-shot byte by byte, pipelined, pipelined with a shifted
gather) is asserted from the a2a_* info keys.  Every receive buffer lies between two 64-byte
guards of 0xA5, which must come back intact."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from mvapich2_amd.consts import TYPES
from tests.mp_alltoall_worker import FILL, GUARD, send_bytes
from tests.test_gpu_collectives_mp import GEOMS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPI_ERR_TRUNCATE, MPI_ERR_OTHER = 14, 15
VEC, BYTES, PIPE, SHIFT = 0, 1, 2, 3  # the worker's path counters


def run_workers(n, cases, tmp_path, timeout=150, ppn=None):
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"cases": cases}))
    out = tmp_path / "out"
    out.mkdir()
    jobid = "a" + uuid.uuid4().hex[:12]
    ppn = ppn or n
    boot = {}
    if ppn < n:
        import socket
        so = socket.socket()
        so.bind(("127.0.0.1", 0))
        boot = {"MV2AMD_BOOT_ADDR": "127.0.0.1", "MV2AMD_BOOT_PORT": str(so.getsockname()[1]), "MV2AMD_NSHARE": str(n)}
        timeout = max(timeout, 240)
        so.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r % ppn), LOCAL_WORLD_SIZE=str(ppn),
                   MV2AMD_JOBID=jobid)
        env.update({"MV2AMD_TIMEOUT_S": "30", **boot, **GEOMS["small"]})
        env.pop("MV2AMD_DEVICE", None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_alltoall_worker.py"), str(spec),
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
    return (lambda cid, r: np.load(out / f"{cid}_r{r}.npy")), logs


def framed(data):
    g = np.full(GUARD, FILL, dtype=np.uint8)
    return np.concatenate([g, data, g])


def check_alltoall(case, n, get, frames=None):
    blk = case["count"] * TYPES[case["type"]][3]
    send = [send_bytes(case["seed"], r, blk * n) for r in range(n)]
    for r in range(n):
        want = framed(np.concatenate([send[j][r * blk:(r + 1) * blk] for j in range(n)]))
        got = frames[r] if frames is not None else get(case["id"], r)
        assert np.array_equal(got, want), f"{case['id']} {case.get('variant', 'plain')} n={n} block {blk} B rank {r}"


def shifts(n, blk):
    """source minus destination misalignment of every block a rank gathers: rank j's block for rank r
    leaves r * blk and lands at j * blk"""
    return {((r * blk) - (j * blk)) & 15 for r in range(n) for j in range(n) if j != r}


# (type, count, path): the issue's table
SIZES = [("MPI_CHAR", 1, BYTES), ("MPI_CHAR", 5, BYTES), ("MPI_FLOAT", 3, BYTES), ("MPI_CHAR", 16, VEC),
         ("MPI_FLOAT", 100, VEC), ("MPI_FLOAT", 16384, VEC), ("MPI_FLOAT", 4099, SHIFT), ("MPI_FLOAT", 70001, SHIFT),
         ("MPI_FLOAT", 70000, PIPE), ("MPI_C_DOUBLE_COMPLEX", 3, VEC)]
VARIANTS = ("inplace", "host_send", "host_recv", "recv_off4", "send_off4", "nonblocking", "enqueue")
VARIANT_COUNTS = (3, 100, 4099, 70001)  # 12 B, 400 B, 16,396 B, 280,004 B


def want_paths(path):
    d = [0, 0, 0, 0]
    d[PIPE if path == SHIFT else path] = 1
    d[SHIFT] = int(path == SHIFT)
    return d


def v_case(cid, seed, C, sd=None, rd=None, **kw):
    """an Alltoallv case from the matrix C[i][j] = floats rank i sends rank j; displacements packed
    in rank order unless given"""
    n = len(C)
    pack = lambda cnt: [sum(cnt[:j]) for j in range(n)]  # noqa: E731
    rc = [[C[j][i] for j in range(n)] for i in range(n)]
    return dict({"id": cid, "kind": "alltoallv", "seed": seed, "scounts": C, "rcounts": rc,
                 "sdispls": sd or [pack(C[i]) for i in range(n)], "rdispls": rd or [pack(rc[i]) for i in range(n)]}, **kw)


def check_alltoallv(case, n, get):
    sc, sd, rc, rd = (case[k] for k in ("scounts", "sdispls", "rcounts", "rdispls"))
    inplace = case.get("variant") == "inplace"
    span = lambda c, d: 4 * max([a + b for a, b in zip(c, d)] + [1])  # noqa: E731
    send = []
    for r in range(n):
        slen, rlen = span(sc[r], sd[r]), span(rc[r], rd[r])
        send.append(send_bytes(case["seed"], r, max(slen, rlen)))
    for r in range(n):
        rlen = span(rc[r], rd[r])
        want = send[r][:rlen].copy() if inplace else np.full(rlen, FILL, dtype=np.uint8)
        if not case.get("expect_rc"):
            for j in range(n):
                want[4 * rd[r][j]:4 * (rd[r][j] + rc[r][j])] = send[j][4 * sd[j][r]:4 * (sd[j][r] + sc[j][r])]
        assert np.array_equal(get(case["id"], r), framed(want)), f"{case['id']} n={n} rank {r}"


def alltoallv_cases(n, seed0):
    rng = np.random.default_rng(seed0)
    rand = rng.choice([0, 0, 1, 3, 4, 8, 100, 1000], size=(n, n)).tolist()
    rand[0][0] = 0                # a zero on the diagonal
    rand[0][n - 1] = 0            # and one off it
    rand[n - 1][n - 1] = 5
    nosend = [[0 if i == 0 else 7 + i + j for j in range(n)] for i in range(n)]
    norecv = [[0 if j == n - 1 else 300 + 4 * i + j for j in range(n)] for i in range(n)]
    uni = [[9 + ((i * j) % 4) for j in range(n)] for i in range(n)]
    rcu = [[uni[j][i] for j in range(n)] for i in range(n)]
    gaps = [[sum(rcu[i][:j]) + 3 * j + 1 for j in range(n)] for i in range(n)]           # 1 float, then 3 between blocks
    desc = [[sum(rcu[i][j + 1:]) + 2 * (n - 1 - j) for j in range(n)] for i in range(n)]  # block 0 last
    one = [[(i + j) % 2 for j in range(n)] for i in range(n)]
    one[1][(2 % n) if n > 2 else 0] = 70001   # known to its sender and its receiver only
    sym = [[16 * (1 + (i + j) % 3) + (i * j) % 2 for j in range(n)] for i in range(n)]  # C == its transpose
    bad = v_case("v_bad", seed0 + 9, uni, expect_rc=MPI_ERR_TRUNCATE)
    bad["rcounts"][(2 % n)][0] += 1   # one rank expects a float more than rank 0 sends it
    return [v_case("v_rand", seed0, rand), v_case("v_nosend", seed0 + 1, nosend), v_case("v_norecv", seed0 + 2, norecv),
            v_case("v_gaps", seed0 + 3, uni, rd=gaps, sd=[[sum(uni[i][:j]) + j for j in range(n)] for i in range(n)]),
            v_case("v_desc", seed0 + 4, uni, rd=desc), v_case("v_one", seed0 + 5, one),
            v_case("v_zero", seed0 + 6, [[0] * n for _ in range(n)]),
            v_case("v_inplace", seed0 + 7, sym, sd=gaps_of(sym), rd=gaps_of(sym), variant="inplace"),
            v_case("v_host", seed0 + 8, uni, rd=gaps, variant="host_recv"),
            v_case("v_nb", seed0 + 10, rand, variant="nonblocking"), bad]


def gaps_of(C):
    n = len(C)
    return [[sum(C[i][:j]) + 2 * j for j in range(n)] for i in range(n)]


@pytest.mark.timeout(400)
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_alltoall_alltoallv_multiprocess(n, tmp_path):
    cases, seed = [], 1
    for t, count, path in SIZES:
        cases.append({"id": f"s{seed}", "kind": "alltoall", "type": t, "count": count, "seed": seed, "path": path})
        seed += 1
    for variant in VARIANTS:
        for count in VARIANT_COUNTS:
            path = next(p for t, c, p in SIZES if t == "MPI_FLOAT" and c == count)
            cases.append({"id": f"v{seed}", "kind": "alltoall", "type": "MPI_FLOAT", "count": count, "seed": seed,
                          "variant": variant, "path": path})
            seed += 1
    derived = []
    if n == 3:
        derived = [{"id": "d_send", "kind": "derived", "side": "send", "count": 1001, "seed": 501},
                   {"id": "d_recv", "kind": "derived", "side": "recv", "count": 1001, "seed": 502}]
    vs = alltoallv_cases(n, 700)
    after = {"id": "after", "kind": "alltoall", "type": "MPI_FLOAT", "count": 4099, "seed": 900, "path": SHIFT}
    info = {"id": "info", "kind": "info", "keys": ["selftest_calls", "oneshot_max"]}
    get, _ = run_workers(n, cases + derived + vs + [after, info], tmp_path, timeout=300)
    if n in (3, 5):  # the shifted sizes really meet several shifts
        for blk in (16396, 280004):
            assert len(shifts(n, blk) - {0}) >= 2, (n, blk)
    for r in range(n):
        calls, oneshot_max = get("info", r)
        assert calls > 0, (r, calls)
        assert 65536 <= oneshot_max < 280000, (r, oneshot_max)  # the table's paths hold for this limit
    for case in cases + [after]:
        check_alltoall(case, n, get)
        blk = case["count"] * TYPES[case["type"]][3]
        path = case["path"]
        # a staged (host or base + 4) buffer is 16-byte aligned, so the shifts are those of the plain call;
        # at 2 ranks 16,396 * 1 = 12 mod 16 still differs from 0
        if path == SHIFT and not (shifts(n, blk) - {0}):
            path = PIPE
        for r in range(n):
            assert list(get(case["id"] + "_paths", r)) == want_paths(path), (case["id"], case.get("variant"), blk, r)
    for case in derived:
        c = case["count"]
        for r in range(n):
            if case["side"] == "send":  # every second float of the send buffer, packed on arrival
                blocks = [send_bytes(case["seed"], j, 8 * c * n).view(np.float32)[2 * c * r:2 * c * (r + 1):2] for j in range(n)]
                want = np.concatenate(blocks).view(np.uint8)
            else:                       # packed floats land on every second float; the others keep the fill
                w = np.full(2 * c * n, np.frombuffer(bytes([FILL] * 4), dtype=np.float32)[0], dtype=np.float32)
                for j in range(n):
                    w[2 * c * j:2 * c * (j + 1):2] = send_bytes(case["seed"], j, 4 * c * n).view(np.float32)[c * r:c * (r + 1)]
                want = w.view(np.uint8)
            assert np.array_equal(get(case["id"], r), framed(want)), (case["id"], r)
    for case in vs:
        check_alltoallv(case, n, get)
        for r in range(n):
            paths = list(get(case["id"] + "_paths", r))
            if case["id"] in ("v_zero", "v_bad"):
                assert paths == [0, 0, 0, 0], (case["id"], r, paths)  # no launch
            elif case["id"] == "v_one":
                assert paths[PIPE] == 1 and paths[VEC] == 0 and paths[BYTES] == 0, (r, paths)  # every rank alike
            else:
                assert sum(paths[:3]) == 1, (case["id"], r, paths)


@pytest.mark.timeout(200)
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_alltoall_back_to_back(n, tmp_path):
    """Eight stream-ordered MPI_Alltoall calls alternating 400-byte (one-shot) and 280,004-byte
    (pipelined, 23 rounds, shifted on every rank at each of these n) blocks with no host
    synchronisation between them, an allreduce after the third and an allgather after the sixth:
    arena halves and slot parities are reused across kernels.  Every byte of every call is checked."""
    counts = [100, 70001] * 4
    case = {"id": "seq", "kind": "sequence", "counts": counts, "seed": 40, "allreduce_after": 2, "ar_count": 70001,
            "allgather_after": 5, "ag_count": 10001}
    get, _ = run_workers(n, [case], tmp_path)
    res = [get("seq", r) for r in range(n)]
    off = 0
    for i, c in enumerate(counts):
        sub = {"id": f"seq call {i}", "type": "MPI_FLOAT", "count": c, "seed": case["seed"] + i}
        size = 4 * c * n + 2 * GUARD
        check_alltoall(sub, n, None, frames=[res[r][off:off + size] for r in range(n)])
        off += size
        if i == case["allreduce_after"]:
            want = framed(np.full(case["ar_count"], n * (n + 1) / 2, dtype=np.float32).view(np.uint8))
        elif i == case["allgather_after"]:
            want = framed(np.concatenate([send_bytes(case["seed"] + 100, j, 4 * case["ag_count"]) for j in range(n)]))
        else:
            continue
        for r in range(n):
            assert np.array_equal(res[r][off:off + len(want)], want), f"call after all-to-all {i}, rank {r}"
        off += len(want)
    assert all(len(res[r]) == off for r in range(n))
    for r in range(n):
        assert list(get("seq_paths", r)) == [4, 0, 4, 4], r


@pytest.mark.timeout(300)
def test_alltoall_refused_across_nodes(tmp_path):
    """4 ranks as 2 nodes of 2: MPI_Alltoall, MPI_Alltoallv and both C-ABI entries return
    MPI_ERR_OTHER's class on every rank, and MPI_Finalize succeeds"""
    get, logs = run_workers(4, [{"id": "mn", "kind": "multinode"}], tmp_path, ppn=2)
    for r in range(4):
        assert list(get("mn", r)) == [MPI_ERR_OTHER] * 4, r
        assert "only jobs on one node are supported" in logs[r]
        assert f"rank {r} done" in logs[r]

"""MPI_Scan / MPI_Exscan on device buffers, one process per rank (the launch scheme
of tests/test_gpu_collectives_mp.py with tests/mp_scan_worker.py as the worker).
Every rank's bytes are compared with tests/ref_scan.py, the rank-by-rank
restatement of MPIR_Scan_generic (scan.c:73-213) and MPIR_Exscan (exscan.c:95-220).

Counts: 1 and 3 (no whole 16-byte vector: the compact one-shot kernel), 100, 4099
(vectors plus a tail, one-shot), 70001 (pipelined for every type of 4 bytes and
more).  Every launch runs under the "small" pipeline geometry (3 workgroups x
4 KiB per round), so a 70001-element segment takes several rounds and both slot
parities are reused inside one call.  A scan's segments always start on 16-byte
boundaries (the runtime cuts them so), so there is no misaligned-segment case; at 3
and 5 ranks the segments differ in length and the last one ends in a tail of
elements.  The kernel choice is asserted from the "oneshot_max" info key."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from mvapich2_amd.consts import OPS, TYPES
from tests import ref_scan
from tests.helpers import assert_bytes_equal, rand_typed
from tests.test_gpu_collectives_mp import GEOMS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
MPI_ERR_OTHER = 15


def inputs(case, rank, call=0):
    rng = np.random.default_rng(case["seed"] * 1000 + call * 100 + rank)
    return rand_typed(case["type"], case["count"], rng, small=case.get("small", False), ties=case.get("ties", False))


def run_scan_workers(n, cases, tmp_path, timeout=100, ppn=None, extra_env=None):
    """n ranks of tests/mp_scan_worker.py, launched as test_gpu_collectives_mp.run_workers launches its
    worker; ppn < n emulates n / ppn nodes (node-major ranks, leaders linked over 127.0.0.1);
    extra_env: settings on top of the "small" geometry"""
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"cases": cases}))
    out = tmp_path / "out"
    out.mkdir()
    jobid = "s" + uuid.uuid4().hex[:12]
    ppn = ppn or n
    boot = {}
    if ppn < n:
        import socket
        so = socket.socket()
        so.bind(("127.0.0.1", 0))
        boot = {"MV2AMD_BOOT_ADDR": "127.0.0.1", "MV2AMD_BOOT_PORT": str(so.getsockname()[1]),
                "MV2AMD_NSHARE": str(n)}
        timeout = max(timeout, 240)
        so.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r % ppn), LOCAL_WORLD_SIZE=str(ppn),
                   MV2AMD_JOBID=jobid)
        env.update({"MV2AMD_TIMEOUT_S": "30", **boot, **GEOMS["small"], **(extra_env or {})})
        env.pop("MV2AMD_DEVICE", None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_scan_worker.py"), str(spec),
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


def check_case(case, n, get, xs=None, uop=None, commute=True, got=None):
    """every rank's receive buffer against ref_scan; a rank without a result (MPI_Exscan's rank 0)
    must hand back its buffer untouched: the 0xA5 fill, or with MPI_IN_PLACE its own operand"""
    t, count = case["type"], case["count"]
    h, ext = TYPES[t][0], TYPES[t][3]
    if xs is None:
        xs = [inputs(case, r).view(np.uint8).ravel().copy() for r in range(n)]
    if uop is None:
        uop = ref_scan.builtin_uop(count, h, OPS[case["op"]])
    want = getattr(ref_scan, case["coll"])([x.copy() for x in xs], uop, commute=commute)
    for r in range(n):
        g = got[r] if got is not None else get(case["id"], r)
        what = f"{case['id']} {case['coll']} {case.get('variant', 'plain')} n={n} count={count} rank {r}"
        if want[r] is None:
            keep = xs[r] if case.get("variant") == "inplace" else np.full(count * ext, FILL, dtype=np.uint8)
            assert np.array_equal(g, keep), what + ": a buffer without a result was written"
        else:
            assert_bytes_equal(g, want[r], t, count, what)


BASIC = [("MPI_SUM", "MPI_FLOAT"), ("MPI_SUM", "MPI_DOUBLE"), ("MPI_SUM", "MPI_INT"), ("MPI_SUM", "MPI_C_FLOAT_COMPLEX"),
         ("MPI_MAX", "MPI_FLOAT"), ("MPI_BXOR", "MPI_UNSIGNED_CHAR"), ("MPI_MAXLOC", "MPI_DOUBLE_INT"),
         ("MPI_MINLOC", "MPI_2INT")]
COUNTS = [1, 3, 100, 4099, 70001]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_scan_exscan_multiprocess(n, tmp_path):
    cases = []
    seed = 1
    for coll in ("scan", "exscan"):
        for op, t in BASIC:
            for count in COUNTS:
                cases.append({"id": f"s{seed}", "kind": "scan", "coll": coll, "type": t, "op": op, "count": count,
                              "seed": seed, "ties": op == "MPI_MAX"})
                seed += 1
        # the complex product: the pipelined kernel evaluates it rank by rank through the programs
        for count in (100, 70001):
            cases.append({"id": f"s{seed}", "kind": "scan", "coll": coll, "type": "MPI_C_FLOAT_COMPLEX",
                          "op": "MPI_PROD", "count": count, "seed": seed})
            seed += 1
        for variant in ("inplace", "nonblocking"):
            for count in (3, 4099, 70001):
                cases.append({"id": f"v{seed}", "kind": "scan", "coll": coll, "variant": variant, "type": "MPI_FLOAT",
                              "op": "MPI_SUM", "count": count, "seed": seed})
                seed += 1
    users = []
    if n in (3, 8):  # host-evaluated user ops: every rank its own program, both branches
        for coll in ("scan", "exscan"):
            for commute in (1, 0):
                users.append({"id": f"u{seed}", "kind": "user_scan", "coll": coll, "type": "MPI_INT", "count": 1000,
                              "commute": commute, "seed": seed})
                seed += 1
    info = {"id": "info", "kind": "info", "keys": ["selftest_calls", "selftest_scan_calls", "oneshot_max"]}
    get, _ = run_scan_workers(n, cases + users + [info], tmp_path, timeout=200)
    for case in cases:
        check_case(case, n, get)
    for case in users:
        xs = [(((np.arange(1000, dtype=np.int32) * 3 + r * 5) % 11 - 4).astype(np.int32)).view(np.uint8) for r in range(n)]
        check_case(case, n, get, xs=xs, uop=ref_scan.user_fn_2a3b, commute=bool(case["commute"]))
    for r in range(n):  # the MPI_Init self-test ran its two scans, counted apart from selftest_calls
        calls, scan_calls, oneshot_max = get("info", r)
        assert calls > 0 and scan_calls == 2, (r, calls, scan_calls)
        # the kernel each count took: up to oneshot_max bytes one-shot, beyond it pipelined
        assert 4099 * 16 <= oneshot_max < 70001 * 4, (r, oneshot_max)


@pytest.mark.timeout(200)
def test_scan_reuse_sequence_4_ranks(tmp_path):
    """Eight back-to-back MPI_Scan calls alternating between the one-shot kernel (4099) and the
    pipelined one (70001, several rounds), fresh operands per call.  The top rank falls 30 ms
    behind before calls 2, 4 and 6, rank 0 before calls 3 and 5: rank 0 depends on nobody's data,
    so only the all-to-all flags keep it from overwriting an arena half (or a pipeline slot) that
    a late rank still reads.  Every word of every call is checked."""
    n = 4
    counts = [4099, 70001] * 4
    case = {"id": "seq", "kind": "scan_seq", "type": "MPI_FLOAT", "op": "MPI_SUM", "counts": counts, "seed": 77,
            "late_top": [2, 4, 6], "late_zero": [3, 5]}
    get, _ = run_scan_workers(n, [case], tmp_path)
    res = [get("seq", r) for r in range(n)]
    off = 0
    for i, c in enumerate(counts):
        sub = dict(case, count=c, coll="scan", id=f"seq call {i + 1}")
        xs = [inputs(sub, r, i + 1).view(np.uint8).ravel().copy() for r in range(n)]
        check_case(sub, n, None, xs=xs, got=[res[r][off:off + c * 4] for r in range(n)])
        off += c * 4
    assert all(len(res[r]) == off for r in range(n))


@pytest.mark.timeout(200)
def test_exscan_then_allgather_4_ranks(tmp_path):
    """A pipelined MPI_Exscan of several rounds followed by a pipelined MPI_Allgather, four times.
    Rank 0 has no Exscan result and gathers nothing, so it reaches the allgather first, and the
    allgather begins by writing its block into the gather slots of every peer -- the slots a late
    peer may still be copying its Exscan result out of.  Rank 0 must therefore keep waiting for
    the gather flags it has no data behind.  The top rank falls 30 ms behind before rounds 1 and
    3.  Every word of both calls is checked."""
    n, repeats, count, agc = 4, 4, 70001, 10001  # 40004-byte blocks: no whole vectors, pipelined
    case = {"id": "xag", "kind": "exscan_ag_seq", "type": "MPI_FLOAT", "op": "MPI_SUM", "count": count,
            "ag_count": agc, "repeats": repeats, "seed": 91, "late_top": [1, 3]}
    info = {"id": "info", "kind": "info", "keys": ["oneshot_max"]}
    get, _ = run_scan_workers(n, [case, info], tmp_path)
    assert all(get("info", r)[0] < count * 4 for r in range(n))
    res = [get("xag", r) for r in range(n)]
    off = 0
    for i in range(repeats):
        sub = dict(case, coll="exscan", id=f"xag exscan {i}")
        xs = [inputs(sub, r, 2 * i).view(np.uint8).ravel().copy() for r in range(n)]
        check_case(sub, n, None, xs=xs, got=[res[r][off:off + count * 4] for r in range(n)])
        off += count * 4
        sub = dict(case, count=agc)
        want = np.concatenate([inputs(sub, r, 2 * i + 1).view(np.uint8).ravel() for r in range(n)])
        for r in range(n):
            assert np.array_equal(res[r][off:off + n * agc * 4], want), f"allgather {i} rank {r}"
        off += n * agc * 4
    assert all(len(res[r]) == off for r in range(n))


@pytest.mark.timeout(300)
def test_scan_refused_across_nodes(tmp_path):
    """4 ranks as 2 nodes of 2: MPI_Scan / MPI_Exscan / MPI_Iscan and the C-ABI calls return
    MPI_ERR_OTHER's class on every rank, the message names the limit, and the job exits cleanly"""
    get, logs = run_scan_workers(4, [{"id": "mn", "kind": "scan_multinode"}], tmp_path, ppn=2)
    for r in range(4):
        assert list(get("mn", r)) == [MPI_ERR_OTHER] * 5, r
        assert "only jobs on one node are supported" in logs[r]
        assert f"rank {r} done" in logs[r]

"""MPI_Gather(v) / MPI_Scatter(v) / MPI_Allgatherv on device buffers, one process per rank (the
launch scheme of tests/test_gpu_alltoall_mp.py with tests/mp_gather_worker.py as the worker).
Expected results are plain placements computed in numpy.

Every launch runs under the "small" pipeline geometry (3 workgroups x 4 KiB per round), so a
280,004-byte block takes 23 rounds and both slot parities are reused inside one call.  The path
each call took is asserted from the gv_* (Allgatherv, Gather) and a2a_* (Gatherv, Scatter,
Scatterv, and Allgatherv under "agv_via_a2a") info keys.  Every receive buffer lies between two
64-byte guards of 0xA5, which must come back intact; gaps between blocks keep their fill; the
receive buffers of Gather's non-roots stay untouched."""
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from mvapich2_amd.consts import TYPES
from tests.mp_alltoall_worker import FILL, GUARD, send_bytes
from tests.mp_gather_worker import vext
from tests.test_gpu_collectives_mp import GEOMS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPI_ERR_TRUNCATE, MPI_ERR_OTHER = 14, 15
VEC, BYTES, PIPE = 0, 1, 2  # offsets into the gv_* / a2a_* counter groups; + 3: the shifted ones
GV, A2A = 0, 4
ONESHOT_MAX = 65536  # asserted below: the node's one-shot limit lies in [65536, 280000)

# (type, count): the issue's table -- 1, 5, 12 B byte-wise; 16, 400, 65,536, 48 B by vectors;
# 16,396 and 280,004 B pipelined and shifted at packed displacements; 280,000 B pipelined, no shift
SIZES = [("MPI_CHAR", 1), ("MPI_CHAR", 5), ("MPI_FLOAT", 3), ("MPI_CHAR", 16), ("MPI_FLOAT", 100),
         ("MPI_FLOAT", 16384), ("MPI_FLOAT", 4099), ("MPI_FLOAT", 70001), ("MPI_FLOAT", 70000),
         ("MPI_C_DOUBLE_COMPLEX", 3)]
VARIANTS = ("inplace", "host_send", "host_recv", "recv_off4", "send_off4", "nonblocking", "vector")
VARIANT_COUNTS = (3, 100, 4099, 70001)  # 12 B, 400 B, 16,396 B, 280,004 B
STAGED_RECV = ("host_recv", "recv_off4")


def run_workers(n, cases, tmp_path, timeout=150, ppn=None):
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"cases": cases}))
    out = tmp_path / "out"
    out.mkdir()
    jobid = "g" + uuid.uuid4().hex[:12]
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
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_gather_worker.py"), str(spec),
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


def plan_path(lens):
    """the path every rank plans from the n block lengths (mv2h_gv_plan with the arena there)"""
    mx = max(lens)
    if mx == 0:
        return None
    if all(v % 16 == 0 for v in lens) and mx <= ONESHOT_MAX:
        return VEC
    return BYTES if mx <= 2048 else PIPE


def want_paths(group, path, shifted):
    d = [0] * 8
    if path is not None:
        d[group + path] = 1
        d[group + 3] = int(path == PIPE and shifted)
    return d


def pack(counts):
    return [sum(counts[:j]) for j in range(len(counts))]


# ---------------------------------------------------------------------------
# Allgatherv
# ---------------------------------------------------------------------------
def agv_case(cid, seed, counts, displs=None, t="MPI_FLOAT", **kw):
    """displs: one list for every rank, or a list per rank; default packed"""
    n = len(counts)
    d = displs or pack(counts)
    if not isinstance(d[0], list):
        d = [d] * n
    return dict({"id": cid, "kind": "allgatherv", "type": t, "counts": counts, "displs": d, "seed": seed}, **kw)


def check_allgatherv(case, n, get):
    variant = case.get("variant", "plain")
    if variant == "vector":
        c = case["count"]
        w = np.full(n * vext(c) // 4, np.frombuffer(bytes([FILL] * 4), dtype=np.float32)[0], dtype=np.float32)
        for j in range(n):
            w[j * vext(c) // 4:(j + 1) * vext(c) // 4:3] = send_bytes(case["seed"], j, 4 * c).view(np.float32)
        for r in range(n):
            assert np.array_equal(get(case["id"], r), framed(w.view(np.uint8))), (case["id"], r)
        return
    ext = TYPES[case["type"]][3]
    counts = case["counts"]
    send = [send_bytes(case["seed"], j, ext * counts[j]) for j in range(n)]
    for r in range(n):
        d = case["displs"][r]
        want = np.full(ext * max([a + b for a, b in zip(counts, d)] + [1]), FILL, dtype=np.uint8)
        for j in range(n):
            want[ext * d[j]:ext * (d[j] + counts[j])] = send[j]
        assert np.array_equal(get(case["id"], r), framed(want)), f"{case['id']} {variant} n={n} rank {r}"


def agv_paths(case, n, r):
    """the counters rank r's call raises"""
    variant = case.get("variant", "plain")
    if variant == "vector":  # the receive side is a packed pooled buffer: blocks back to back
        ext, counts, d = 4, [case["count"]] * n, pack([case["count"]] * n)
    else:
        ext, counts, d = TYPES[case["type"]][3], case["counts"], case["displs"][r]
    path = plan_path([ext * c for c in counts])
    via = bool(case.get("via_a2a"))
    # a block written where it is off a 16-byte boundary (own block: unless in place; the
    # all-to-all table copies the own block outside its count).  A staged receive buffer is
    # gathered at packed aligned offsets.
    skip_own = variant == "inplace" or via
    shifted = variant not in STAGED_RECV and any(
        counts[j] and (ext * d[j]) % 16 for j in range(n) if not (j == r and skip_own))
    return want_paths(A2A if via else GV, path, shifted)


def ragged_vectors(n):
    """the issue's ragged vectors, in floats"""
    small = [0, 3, 4099]
    one_long = [70001 if j == 1 % n else small[j % 3] for j in range(n)]
    zero_first = [0] + [5 + j for j in range(1, n)]
    zero_last = [40 + 4 * j for j in range(n - 1)] + [0]
    return {"one_long": one_long, "zero_first": zero_first, "zero_last": zero_last, "all_zero": [0] * n}


def allgatherv_cases(n, uniform_only=False):
    cases, seed = [], 1
    for t, count in SIZES:
        cases.append(agv_case(f"u{seed}", seed, [count] * n, t=t))
        seed += 1
    if uniform_only:
        return cases
    for name, counts in ragged_vectors(n).items():
        cases.append(agv_case(f"r_{name}", seed, counts))
        seed += 1
    uni = [9 + (j % 4) for j in range(n)]
    gaps = [sum(uni[:j]) + 2 * j + 1 + j % 2 for j in range(n)]           # 1 float, then 2 or 3 between blocks
    desc = [sum(uni[j + 1:]) + (n - 1 - j) for j in range(n)]             # block 0 last, 1 float between
    per_rank = [[sum(uni[:j]) + (j + 1) * (r + 1) for j in range(n)] for r in range(n)]
    big = [4099 + j for j in range(n)]
    cases += [agv_case("d_gaps", seed, uni, gaps), agv_case("d_desc", seed + 1, uni, desc),
              agv_case("d_per_rank", seed + 2, uni, per_rank),
              agv_case("d_vec_gaps", seed + 3, [16] * n, [19 * j + 1 for j in range(n)]),  # vectors, off displacements
              agv_case("d_big_gaps", seed + 4, big, [sum(big[:j]) + 3 * j for j in range(n)])]
    return cases


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_allgatherv(n, tmp_path):
    """uniform counts over the size table, ragged vectors, gapped / descending / per-rank
    displacements; then the same cases through the all-to-all table, byte-identical (8 ranks: the
    uniform table only)"""
    cases = allgatherv_cases(n, uniform_only=n == 8)
    twins = [] if n == 8 else [dict(c, id=c["id"] + "_a2a", via_a2a=True) for c in cases]
    info = {"id": "info", "kind": "info", "keys": ["oneshot_max"]}
    get, _ = run_workers(n, cases + twins + [info], tmp_path, timeout=240)
    for r in range(n):
        assert ONESHOT_MAX <= get("info", r)[0] < 280000, r  # the table's paths hold for this limit
    for case in cases + twins:
        check_allgatherv(case, n, get)
        for r in range(n):
            assert list(get(case["id"] + "_paths", r)) == agv_paths(case, n, r), (case["id"], r)
    for case in twins:
        for r in range(n):
            assert np.array_equal(get(case["id"], r), get(case["id"][:-4], r)), (case["id"], r)


# ---------------------------------------------------------------------------
# Gather / Scatter / Gatherv / Scatterv
# ---------------------------------------------------------------------------
def block_layout(case, n):
    """(ext, counts, displs) of the side that owns n blocks, in elements"""
    ext = TYPES[case.get("type", "MPI_FLOAT")][3]
    if "counts" in case:
        return ext, case["counts"], case["displs"]
    return ext, [case["count"]] * n, pack([case["count"]] * n)


def check_gather(case, n, get):
    ext, counts, d = block_layout(case, n)
    variant, root, bad = case.get("variant", "plain"), case["root"], case.get("expect_rc")
    extra = case.get("extra", {})
    send = [send_bytes(case["seed"], j, ext * (counts[j] + extra.get(str(j), 0))) for j in range(n)]
    if variant == "vector":
        c = counts[0]
        w = np.full(n * vext(c) // 4, np.frombuffer(bytes([FILL] * 4), dtype=np.float32)[0], dtype=np.float32)
        untouched = w.copy().view(np.uint8)
        for j in range(n):
            w[j * vext(c) // 4:(j + 1) * vext(c) // 4:3] = send[j].view(np.float32)
        want = w.view(np.uint8)
    else:
        untouched = np.full(ext * max([a + b for a, b in zip(counts, d)] + [1]), FILL, dtype=np.uint8)
        want = untouched.copy()
        for j in range(n):
            if not bad or (j == root and variant == "inplace"):
                want[ext * d[j]:ext * (d[j] + counts[j])] = send[j][:ext * counts[j]]
    for r in range(n):
        assert np.array_equal(get(case["id"], r), framed(want if r == root else untouched)), \
            f"{case['id']} {variant} n={n} root {root} rank {r}"


def check_scatter(case, n, get):
    ext, counts, d = block_layout(case, n)
    variant, root, bad = case.get("variant", "plain"), case["root"], case.get("expect_rc")
    extra = case.get("extra", {})
    if variant == "vector":
        c = counts[0]
        x = send_bytes(case["seed"], root, n * vext(c)).view(np.float32)
        blocks = [x[j * vext(c) // 4:(j + 1) * vext(c) // 4:3].copy().view(np.uint8) for j in range(n)]
    else:
        x = send_bytes(case["seed"], root, ext * max([a + b for a, b in zip(counts, d)] + [1]))
        blocks = [x[ext * d[j]:ext * (d[j] + counts[j])] for j in range(n)]
    for r in range(n):
        want = np.full(max(ext * (counts[r] + extra.get(str(r), 0)), 1), FILL, dtype=np.uint8)
        if not bad and not (r == root and variant == "inplace"):
            want[:len(blocks[r])] = blocks[r]
        assert np.array_equal(get(case["id"], r), framed(want)), f"{case['id']} {variant} n={n} root {root} rank {r}"


def gather_paths(case, n, r):
    """MPI_Gather: the gather table; only the root writes blocks"""
    ext, counts, d = block_layout(case, n)
    variant, root = case.get("variant", "plain"), case["root"]
    shifted = r == root and variant not in STAGED_RECV and any(
        (ext * d[j]) % 16 for j in range(n) if not (j == r and variant == "inplace"))
    return want_paths(GV, plan_path([ext * c for c in counts]), shifted)


def scatter_paths(case, n, r):
    """MPI_Scatter: the all-to-all table; a receiver's block arrives at (r * bytes) & 15 and lands
    on a 16-byte boundary (its own or the staging buffer's); the root gathers nothing"""
    ext, counts, _ = block_layout(case, n)
    blk = ext * counts[0]
    path = plan_path([blk])
    return want_paths(A2A, path, r != case["root"] and (r * blk) % 16 != 0)


def check_table_paths(case, n, get):
    """Gatherv / Scatterv run on the all-to-all kernels, one launch on every rank alike, or none"""
    for r in range(n):
        p = list(get(case["id"] + "_paths", r))
        assert p[:4] == [0, 0, 0, 0], (case["id"], r, p)
        launches = 0 if case.get("expect_rc") or not any(case["counts"]) else 1
        assert sum(p[4:7]) == launches, (case["id"], r, p)
        assert p[4:7] == list(get(case["id"] + "_paths", 0))[4:7], (case["id"], r, p)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_gather_scatter(n, tmp_path):
    """counts 3, 100, 4099, 70001 at roots 0 and n - 1, and the size table at root 0"""
    cases, seed = [], 100
    for kind in ("gather", "scatter"):
        for count in VARIANT_COUNTS:
            for root in (0, n - 1):
                cases.append({"id": f"{kind[0]}{seed}", "kind": kind, "count": count, "root": root, "seed": seed})
                seed += 1
        for t, count in SIZES:
            cases.append({"id": f"{kind[0]}{seed}", "kind": kind, "type": t, "count": count, "root": 0, "seed": seed})
            seed += 1
    info = {"id": "info", "kind": "info", "keys": ["oneshot_max"]}
    get, _ = run_workers(n, cases + [info], tmp_path, timeout=240)
    for r in range(n):
        assert ONESHOT_MAX <= get("info", r)[0] < 280000, r
    for case in cases:
        (check_gather if case["kind"] == "gather" else check_scatter)(case, n, get)
        model = gather_paths if case["kind"] == "gather" else scatter_paths
        for r in range(n):
            assert list(get(case["id"] + "_paths", r)) == model(case, n, r), (case["id"], case["count"], case["root"], r)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [2, 3, 5])
def test_gatherv_scatterv(n, tmp_path):
    """the ragged vectors at the root (roots 0 and n - 1, packed and gapped displacements); a
    mismatched pair is MPI_ERR_TRUNCATE on every rank with every buffer untouched, and the next
    call still works"""
    cases, seed = [], 300
    for kind in ("gatherv", "scatterv"):
        for name, counts in ragged_vectors(n).items():
            for root, d in ((0, pack(counts)), (n - 1, [sum(counts[:j]) + 3 * j + 1 for j in range(n)])):
                cases.append({"id": f"{kind[0]}{seed}_{name}", "kind": kind, "counts": counts, "displs": d, "root": root,
                              "seed": seed})
                seed += 1
        uni = [9 + (j % 4) for j in range(n)]
        bad_rank = str(1 if n > 1 else 0)  # a non-root sends / expects 4 bytes more than the root holds for it
        cases.append({"id": f"{kind[0]}_bad", "kind": kind, "counts": uni, "displs": pack(uni), "root": 0, "seed": seed,
                      "extra": {bad_rank: 1}, "expect_rc": MPI_ERR_TRUNCATE})
        cases.append({"id": f"{kind[0]}_after", "kind": kind, "counts": uni, "displs": pack(uni), "root": 0, "seed": seed + 1})
        seed += 2
    get, _ = run_workers(n, cases, tmp_path, timeout=240)
    for case in cases:
        (check_gather if case["kind"] == "gatherv" else check_scatter)(case, n, get)
        check_table_paths(case, n, get)


CALLS = ("allgatherv", "gather", "gatherv", "scatter", "scatterv")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("call", CALLS)
def test_variants(call, n, tmp_path):
    """in place (at the root for the rooted calls), host send buffer, host receive buffer, receive
    base + 4 bytes, send base + 4 bytes, nonblocking + MPI_Wait, and a vector datatype on the side
    that owns n blocks, at 12 B, 400 B, 16,396 B and 280,004 B"""
    cases, seed = [], 500
    root = n - 2
    for variant in VARIANTS:
        for count in VARIANT_COUNTS:
            cid = f"{variant}_{count}"
            if call == "allgatherv":
                c = agv_case(cid, seed, [count] * n, variant=variant)
                c["count"] = count
            elif call in ("gather", "scatter"):
                c = {"id": cid, "kind": call, "count": count, "root": root, "seed": seed, "variant": variant}
            else:
                c = {"id": cid, "kind": call, "counts": [count] * n, "displs": pack([count] * n), "root": root,
                     "seed": seed, "variant": variant}
            cases.append(c)
            seed += 1
    get, _ = run_workers(n, cases, tmp_path, timeout=240)
    for case in cases:
        if call == "allgatherv":
            check_allgatherv(case, n, get)
            for r in range(n):
                assert list(get(case["id"] + "_paths", r)) == agv_paths(case, n, r), (case["id"], r)
        elif call in ("gather", "gatherv"):
            check_gather(case, n, get)
        else:
            check_scatter(case, n, get)
        if call == "gather":
            for r in range(n):
                want = gather_paths(case, n, r)
                if case["variant"] == "vector" and r == root:  # packed blocks back to back in a pooled buffer
                    want = want_paths(GV, plan_path([4 * case["count"]]), (4 * case["count"]) % 16 != 0)
                assert list(get(case["id"] + "_paths", r)) == want, (case["id"], r)
        elif call == "scatter":
            for r in range(n):
                assert list(get(case["id"] + "_paths", r)) == scatter_paths(case, n, r), (case["id"], r)
        elif call != "allgatherv":
            check_table_paths(case, n, get)


@pytest.mark.timeout(200)
@pytest.mark.parametrize("n", [3, 5])
def test_back_to_back(n, tmp_path):
    """40 calls in one job cycling through gather (root = i mod n), scatter, allgatherv, alltoall
    and allreduce at 12 B, 400 B and 16,396 B: one-shot arena halves and slot parities are reused
    across different collectives, which is what the all-rank flags exist for.  Every call is checked."""
    counts, calls, seed0 = [3, 100, 4099], 40, 40
    get, _ = run_workers(n, [{"id": "seq", "kind": "sequence", "calls": calls, "counts": counts, "seed": seed0}], tmp_path)
    res = [get("seq", r) for r in range(n)]
    off = 0
    for i in range(calls):
        c, op, seed, root = counts[i % 3], i % 5, seed0 + i, i % n
        blk = 4 * c
        for r in range(n):
            if op == 0:
                want = np.full(blk * n, FILL, dtype=np.uint8)
                if r == root:
                    want = np.concatenate([send_bytes(seed, j, blk) for j in range(n)])
            elif op == 1:
                want = send_bytes(seed, root, blk * n)[r * blk:(r + 1) * blk]
            elif op == 2:
                want = np.concatenate([send_bytes(seed, j, blk) for j in range(n)])
            elif op == 3:
                want = np.concatenate([send_bytes(seed, j, blk * n)[r * blk:(r + 1) * blk] for j in range(n)])
            else:
                want = np.full(c, n * (n + 1) / 2, dtype=np.float32).view(np.uint8)
            size = len(want) + 2 * GUARD
            assert np.array_equal(res[r][off:off + size], framed(want)), \
                f"call {i} (op {op}, {blk} B, root {root}) rank {r}"
        off += 2 * GUARD + (blk if op in (1, 4) else blk * n)
    assert all(len(res[r]) == off for r in range(n))
    for r in range(n):
        p = list(get("seq_paths", r))
        assert sum(p[:3]) == 16 and sum(p[4:7]) == 16, (r, p)  # gather + allgatherv; scatter + alltoall


@pytest.mark.timeout(300)
def test_refused_across_nodes(tmp_path):
    """4 ranks as 2 nodes of 2: the five calls and their C-ABI entries return MPI_ERR_OTHER's class
    on every rank, and MPI_Finalize succeeds"""
    get, logs = run_workers(4, [{"id": "mn", "kind": "multinode"}], tmp_path, ppn=2)
    for r in range(4):
        assert list(get("mn", r)) == [MPI_ERR_OTHER] * 10, r
        assert "only jobs on one node are supported" in logs[r]
        assert f"rank {r} done" in logs[r]

"""Every legal (op, type) pair the device supports -- 291 pairs over 42 types -- through the
cross-GPU allreduce, reduce and reduce-scatter kernels, one process per rank at 3 and 5 ranks,
bit-exact against the oracle's rank-by-rank simulation of the algorithm the reference selects.

The functors themselves are covered pair by pair in test_gpu_reduce_local.py; what differs per pair
around them is covered here: the three bodies of the pipelined reduction (order-free, wide,
eight-column in butterfly / ring / program order), the index arithmetic that scales with the
element size (owners, program blocks, scalar segment heads, element tails) and the sharing of
kernels between kinds (signed integers as unsigned, struct complex SUM as C99).

The case table is tests/all_pairs_cases.py; tests/test_all_pairs_table.py checks on the CPU that
each size selects the algorithm and reaches the kernel named there.  Run D is the default selection
under the "small" pipeline geometry with the one-shot limit at 16 KiB; run K moves the ring wrapper
down to 16 KiB, turns the topology-aware tree off and narrows the compact kernel to 256 B.  Every
rank runs the whole matrix on one pair of device buffers (worker kind "batch").

What the matrix has caught.  MPI_PROD on MPI_COMPLEX and MPI_DOUBLE_COMPLEX (1,552 B and up, both rank
counts): the sign of a NaN, which depends on the operand order of the reference's compiled
multiplies (ops/functors.h).  With the butterfly body of the non-wide pairs replaced by the LINEAR
one, the 40,976 B allreduce fails for fp PROD at 3 ranks and for ten fp / complex SUM and PROD pairs at
5; with the scalar head of a misaligned segment folding in another order, the ring cases fail at 5
ranks.  The head's element index, however, reaches no result today: every segment that starts off
the 16-byte grid belongs to a ring or to a reduce-scatter with one program."""
import json

import numpy as np
import pytest

from mvapich2_amd.consts import OPS, TYPES
from oracle import oracle
from tests import all_pairs_cases as apc
from tests.helpers import as_bytes, assert_bytes_equal
from tests.test_gpu_collectives_mp import inputs, run_workers

pytestmark = pytest.mark.gpu

INFO = {"id": "ti", "kind": "tiling_info"}  # [5]: oneshot_max


def run_matrix(n, cases, env, mpit_calls, tmp_path):
    """the batch, the library's one-shot limit and the MPI_T counters of `mpit_calls` on n ranks;
    returns (per-rank result bytes of each case, per-rank counters)"""
    spec = [{"id": "batch", "kind": "batch", "cases": cases}, INFO, {"id": "mpit", "kind": "mpit_counts", "calls": mpit_calls}]
    res = run_workers(n, spec, tmp_path, timeout=200, extra_env=env)
    got = {c["id"]: [None] * n for c in cases}
    for r in range(n):
        assert res("ti", r)[5] == apc.ONESHOT_MAX, (r, res("ti", r))
        blob, off = res("batch", r), 0
        for c in cases:
            ext = TYPES[c["type"]][3]
            if c["kind"] == "reduce_scatter":
                ln = c["recvcounts"][r] * ext
            elif c["kind"] == "reduce":
                ln = c["count"] * ext if r == c["root"] else 0
            else:
                ln = c["count"] * ext
            got[c["id"]][r] = blob[off:off + ln]
            off += ln
        assert off == len(blob), (r, off, len(blob))
    counters = [json.loads(res("mpit", r).tobytes().decode()) for r in range(n)]
    return got, counters


def sends_of(case, n):
    return [as_bytes(inputs(case, r)).copy() for r in range(n)]


def check(cases, n, got, expected):
    """every case against expected(case, sends) -> {rank: (bytes, count)}; all mismatches are listed"""
    bad = []
    for c in cases:
        want = expected(c, sends_of(c, n))
        for r, (w, count) in want.items():
            try:
                assert_bytes_equal(got[c["id"]][r], w, c["type"], count, "")
            except AssertionError as e:
                bad.append(f"{c['kind']} {c['op']} {c['type']} size {c['size']} count {c['count']} n={n} rank {r} "
                           f"[{c['algo']}, {c['path']}]:{e}")
    assert not bad, f"{len(bad)} results differ from the oracle:\n" + "\n".join(bad[:40])


def counted(counters, want):
    for r, got in enumerate(counters):
        assert {k: got[k] for k in want} == want, (r, {k: v for k, v in got.items() if v})


def mpit_allreduce(sizes, t="MPI_FLOAT"):
    return [{"coll": "allreduce", "type": t, "count": apc.count_for(size, TYPES[t][3])} for size in sizes]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", apc.NS)
def test_allreduce_all_pairs(n, tmp_path):
    """520 B compact kernel and 1,552 B vector body in the topology-aware tree's order, 8,208 B one-shot
    and 40,976 B pipelined (several rounds, a partial last range) in pt2pt_rs's butterfly"""
    cases = apc.allreduce_cases(n, "D")
    got, counters = run_matrix(n, cases, apc.ENV_D, mpit_allreduce([s for s, _, _ in apc.ALLREDUCE_D]), tmp_path)
    counted(counters, {"mv2_coll_allreduce_topo_aware_hierarchical": 2, "mv2_coll_allreduce_shm_rs": 2,
                       "mv2_coll_allreduce_pt2pt_ring_wrapper": 0})

    def expected(c, sends):
        want = oracle.allreduce_ref(sends, c["count"], TYPES[c["type"]][0], OPS[c["op"]])
        return {r: (want[r], c["count"]) for r in range(n)}
    check(cases, n, got, expected)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", apc.NS)
def test_allreduce_all_pairs_ring_and_linear_knobs(n, tmp_path):
    """run K: 200 B compact and 520 B vector body in the two-level LINEAR order; the flat ring on n
    chunks that start off 16-byte boundaries (scalar heads), its n - 1 leftover elements through
    pt2pt_rs on a base that is not 16-byte aligned"""
    cases = apc.allreduce_cases(n, "K")
    calls = mpit_allreduce([s for s, _, _ in apc.ALLREDUCE_K])
    calls.append({"coll": "allreduce", "type": "MPI_FLOAT", "count": apc.ring_count(n, 4)})
    got, counters = run_matrix(n, cases, apc.ENV_K, calls, tmp_path)
    counted(counters, {"mv2_coll_allreduce_shm_intra": 2, "mv2_coll_allreduce_pt2pt_ring_wrapper": 1,
                       "mv2_coll_allreduce_pt2pt_ring": 1, "mv2_coll_allreduce_shm_rs": 1,
                       "mv2_coll_allreduce_topo_aware_hierarchical": 0})
    knobs = oracle.default_knobs(**apc.KNOBS_K)

    def expected(c, sends):
        want = oracle.allreduce_ref(sends, c["count"], TYPES[c["type"]][0], OPS[c["op"]], knobs=knobs)
        return {r: (want[r], c["count"]) for r in range(n)}
    check(cases, n, got, expected)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", apc.NS)
def test_reduce_all_pairs(n, tmp_path):
    """to root n - 1: 520 B shmem, 8,208 B redscat_gather (the padded pair types: knomial), 40,976 B
    knomial through the pipelined reduce"""
    cases = apc.reduce_cases(n)
    calls = [{"coll": "reduce", "type": "MPI_FLOAT", "count": apc.count_for(size, 4), "root": n - 1}
             for size, _, _ in apc.REDUCE_D]
    got, counters = run_matrix(n, cases, apc.ENV_D, calls, tmp_path)
    counted(counters, {"mv2_coll_reduce_shmem": 1, "mv2_coll_reduce_redscat_gather": 1, "mv2_coll_reduce_knomial": 1,
                       "mv2_coll_reduce_binomial": 0})

    def expected(c, sends):
        return {c["root"]: (oracle.reduce_ref(sends, c["count"], TYPES[c["type"]][0], OPS[c["op"]], c["root"]), c["count"])}
    check(cases, n, got, expected)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", apc.NS)
def test_reduce_scatter_all_pairs(n, tmp_path):
    """ragged blocks q + r: 240 B rs_basic and 2,000 B recursive halving one-shot element by element,
    3 KiB recursive halving with blocks inside a vector (pipelined in program order, scalar heads),
    12 KiB of whole-vector blocks (one-shot vector body), 40 KiB pairwise and 96 KiB ring pipelined"""
    cases = apc.reduce_scatter_cases(n)
    calls = []
    for size, _, vec in apc.REDUCE_SCATTER_D:
        counts = apc.rs_counts(n, 4, size, vec)
        calls.append({"coll": "reduce_scatter", "type": "MPI_FLOAT", "count": max(counts), "recvcounts": counts})
    got, counters = run_matrix(n, cases, apc.ENV_D, calls, tmp_path)
    counted(counters, {"mv2_coll_reduce_scatter_basic": 1, "mv2_coll_reduce_scatter_rec_halving": 3,
                       "mv2_coll_reduce_scatter_pairwise": 1, "mv2_coll_reduce_scatter_ring": 1})

    def expected(c, sends):
        counts, ext = c["recvcounts"], TYPES[c["type"]][3]
        full = oracle.reduce_scatter_ref(sends, counts, TYPES[c["type"]][0], OPS[c["op"]])
        offs = apc.segment_offsets(c, n)
        return {r: (full[offs[r]:offs[r] + counts[r] * ext], counts[r]) for r in range(n)}
    check(cases, n, got, expected)

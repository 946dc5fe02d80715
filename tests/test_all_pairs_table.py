"""The case table of the all-pairs GPU matrices (tests/all_pairs_cases.py), checked with the oracle
alone: every size resolves to the algorithm it is meant to exercise at both rank counts and every
extent, lands on the intended side of the compact / one-shot / pipelined limits, ends in a partial
16-byte vector, and the ring and ragged reduce-scatter cases start segments inside a vector."""
import pytest

from mvapich2_amd.consts import DEVICE_UNSUPPORTED, TYPES, legal_pairs
from oracle import oracle
from tests import all_pairs_cases as apc

TABLES = [("allreduce D", lambda n: apc.allreduce_cases(n, "D")), ("allreduce K", lambda n: apc.allreduce_cases(n, "K")),
          ("reduce", apc.reduce_cases), ("reduce_scatter", apc.reduce_scatter_cases),
          ("scan", lambda n: apc.scan_cases(n, "scan")), ("exscan", lambda n: apc.scan_cases(n, "exscan"))]
NSIZES = {"allreduce D": 4, "allreduce K": 3, "reduce": 3, "reduce_scatter": 6, "scan": 3, "exscan": 3}


def test_pairs_are_the_291_legal_device_pairs():
    assert apc.PAIRS == [(op, t) for op, t in legal_pairs() if t not in DEVICE_UNSUPPORTED]
    assert len(apc.PAIRS) == len(set(apc.PAIRS)) == 291
    assert len({t for _, t in apc.PAIRS}) == 42
    assert {TYPES[t][3] for _, t in apc.PAIRS} == {1, 2, 4, 8, 16}


@pytest.mark.parametrize("n", apc.NS)
@pytest.mark.parametrize("name", [name for name, _ in TABLES])
def test_every_size_holds_every_pair_once(name, n):
    cases = dict(TABLES)[name](n)
    assert len({c["id"] for c in cases}) == len(cases) == NSIZES[name] * 291
    assert len({c["seed"] for c in cases}) == len(cases)
    by_size = {}
    for c in cases:
        by_size.setdefault((c["size"], c.get("vec", False)), []).append((c["op"], c["type"]))
        assert c["small"] == (c["op"] == "MPI_PROD")
    assert len(by_size) == NSIZES[name]
    for pairs in by_size.values():
        assert pairs == apc.PAIRS


def kernel_path(nbytes, scalar_max):
    return "compact" if nbytes <= scalar_max else "oneshot" if nbytes <= apc.ONESHOT_MAX else "pipe"


@pytest.mark.parametrize("n", apc.NS)
def test_allreduce_sizes_select_the_intended_algorithm(n):
    for run, knobs, scalar_max in (("D", None, apc.AR_SCALAR_MAX_D),
                                   ("K", oracle.default_knobs(**apc.KNOBS_K), apc.AR_SCALAR_MAX_K)):
        for c in apc.allreduce_cases(n, run):
            got = oracle.ALGOS[oracle.allreduce_select(n, c["count"], TYPES[c["type"]][0], knobs=knobs)]
            assert got == c["algo"], (run, n, c["type"], c["size"], got)
            assert kernel_path(apc.nbytes(c), scalar_max) == c["path"], (run, n, c["type"], c["size"])
    # the listed values of the selection itself
    for t in ("MPI_CHAR", "MPI_SHORT", "MPI_INT", "MPI_DOUBLE", "MPI_C_DOUBLE_COMPLEX", "MPI_DOUBLE_INT"):
        h, size, ext = TYPES[t][0], TYPES[t][2], TYPES[t][3]
        sel = lambda nb, knobs=None: oracle.ALGOS[oracle.allreduce_select(n, nb // ext, h, knobs=knobs)]  # noqa: E731
        assert [sel(nb) for nb in (16, 512, 2048)] == ["topo_tree"] * 3
        assert [sel(nb) for nb in (4096, 16384, 40976, (2 << 20) - 16)] == ["pt2pt_rs"] * 4
        k = oracle.default_knobs(**apc.KNOBS_K)
        assert [sel(nb, k) for nb in (16, 208, 512)] == ["shmem_linear"] * 3
        assert sel(40976, k) == "ring_wrapper"
        # the threshold is on the packed size: MPI_DOUBLE_INT carries 12 KiB at 16,384 B
        assert sel(16384, k) == ("pt2pt_rs" if size != ext else "ring_wrapper")


@pytest.mark.parametrize("n", apc.NS)
def test_reduce_sizes_select_the_intended_algorithm(n):
    padded = set()
    for c in apc.reduce_cases(n):
        got = oracle.ALGOS[oracle.reduce_select(n, c["count"], TYPES[c["type"]][0])[0]]
        assert got == c["algo"], (n, c["type"], c["size"], got)
        assert kernel_path(apc.nbytes(c), apc.AR_SCALAR_MAX_D) == c["path"], (n, c["type"], c["size"])
        assert c["root"] == n - 1
        if c["size"] == 8208 and c["algo"] != "redscat_gather":
            padded.add(c["type"])
    assert padded == {"MPI_SHORT_INT", "MPI_DOUBLE_INT", "MPI_LONG_INT"}  # 6 of 8 and 12 of 16 bytes carry data


@pytest.mark.parametrize("n", apc.NS)
def test_reduce_scatter_totals_select_the_intended_algorithm(n):
    for c in apc.reduce_scatter_cases(n):
        t, counts = c["type"], c["recvcounts"]
        ext = TYPES[t][3]
        got = oracle.ALGOS[oracle.reduce_scatter_select(counts, TYPES[t][0])]
        assert got == c["algo"], (n, t, c["size"], got)
        assert counts == [counts[0] + r for r in range(n)] or c["vec"]
        assert all(x > 0 for x in counts) and sum(counts) == c["count"]
        total = apc.nbytes(c)
        assert 0.75 * c["size"] <= total <= c["size"], (n, t, c["size"], total)
        # the kernel each total reaches (padded pair types always run the pipelined kernel)
        padded = TYPES[t][2] != ext
        want = {240: "oneshot_elem", 2000: "oneshot_elem", 3072: "oneshot_elem" if ext == 16 else "pipe",
                12288: "oneshot_vec", 40960: "pipe", 98304: "pipe"}[c["size"]]
        assert c["path"] == ("pipe" if padded else want), (n, t, c["size"], c["path"])
        assert (total > apc.ONESHOT_MAX) == (c["size"] >= 40960) and (total <= 256) == (c["size"] == 240)
        offs = apc.segment_offsets(c, n)
        if c["vec"]:
            assert all(x * ext % 16 == 0 for x in counts) and all(o % 16 == 0 for o in offs)
            assert len(set(counts)) == n
        elif ext < 16:
            assert counts[0] * ext % 16 != 0 and any(o % 16 for o in offs), (n, t, c["size"])
    # the listed values of the selection itself (ragged MPI_INT counts of at most `total` bytes)
    sel = lambda total, m: oracle.ALGOS[oracle.reduce_scatter_select(  # noqa: E731
        apc.rs_counts(m, 4, total, False), TYPES["MPI_INT"][0])]
    assert sel(256, n) == "rs_basic"
    assert sel(260, 5) == "rs_rec_halving"
    assert [sel(total, n) for total in (8192, 16384)] == ["rs_rec_halving"] * 2
    assert sel(40000, n) == "rs_pairwise"
    assert sel(65540, 3) == "rs_pairwise" and sel(65540, 5) == "rs_ring"
    assert sel(98304, n) == "rs_ring"


@pytest.mark.parametrize("n", apc.NS)
def test_ring_case_starts_its_chunks_inside_a_vector(n):
    for c in apc.allreduce_cases(n, "K"):
        if not c.get("ring"):
            continue
        ext = TYPES[c["type"]][3]
        q, rem = divmod(c["count"], n)
        assert rem == n - 1 and 0.9 * apc.RING_K_TOTAL <= n * q * ext <= apc.RING_K_TOTAL
        if ext < 16:
            assert any(o % 16 for o in apc.segment_offsets(c, n)), (n, c["type"])
            assert n * q * ext % 16 != 0, (n, c["type"])  # the pt2pt_rs remainder starts off the 16-byte grid


@pytest.mark.parametrize("n", apc.NS)
@pytest.mark.parametrize("name", ["allreduce D", "allreduce K", "reduce", "scan", "exscan"])
def test_operands_end_in_a_partial_vector(name, n):
    scalar_max = apc.AR_SCALAR_MAX_K if name == "allreduce K" else apc.AR_SCALAR_MAX_D
    for c in dict(TABLES)[name](n):
        ext = TYPES[c["type"]][3]
        if ext < 16:
            assert apc.nbytes(c) % 16 != 0, (name, n, c["type"], c["size"])
        assert c["size"] - 16 <= apc.nbytes(c) <= c["size"] + 16 or c.get("ring"), (name, n, c["type"], c["size"])
        assert kernel_path(apc.nbytes(c), scalar_max) == c["path"], (name, n, c["type"], c["size"])

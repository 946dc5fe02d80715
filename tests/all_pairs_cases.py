"""The case table of the all-pairs matrices: every legal (op, type) pair the device supports through
the multi-process allreduce / reduce / reduce-scatter kernels (tests/test_gpu_collectives_all_pairs_mp.py)
and through MPI_Scan / MPI_Exscan (tests/test_gpu_scan_all_pairs_mp.py).  tests/test_all_pairs_table.py
checks with the oracle alone that every size below selects the algorithm, and so the kernel path, it
is meant to reach; the GPU tests import the same lists, so the table that runs is the table checked.

Sizes are in bytes B.  An operand has B // ext + 1 elements, one more where that is a whole number
of 16-byte vectors (8-byte types at B = 8 mod 16), so every extent below 16 ends in a partial
vector; 16-byte types have B // 16 elements.  Reduce-scatter cases are ragged (recvcounts q + r) with
q * ext off the 16-byte grid, so blocks start inside a vector."""
from mvapich2_amd.consts import DEVICE_UNSUPPORTED, TYPES, legal_pairs

PAIRS = [(op, t) for op, t in legal_pairs() if t not in DEVICE_UNSUPPORTED]
NS = (3, 5)
ONESHOT_MAX = 16384
# the "small" pipeline geometry (3 workgroups x 4 KiB per round) with the one-shot kernels narrowed
# to 16 KiB: everything above runs the pipelined kernel, a 40 KiB operand in several rounds
ENV_D = {"MV2AMD_PIPE_GRID": "3", "MV2AMD_PIPE_SUB": "4096", "MV2AMD_ONESHOT_MAX": str(ONESHOT_MAX)}
# run K: the ring wrapper from 16 KiB, no topology-aware tree, the compact kernel up to 256 B
ENV_K = dict(ENV_D, MV2_ALLREDUCE_RING_ALGO_THRESHOLD="16K", MV2_USE_TOPO_AWARE_ALLREDUCE="0", MV2AMD_AR_SCALAR_MAX="256")
KNOBS_K = {"ring_thr": 16384, "use_topo_allreduce": 0}
AR_SCALAR_MAX_D, AR_SCALAR_MAX_K = 1024, 256

# (size, algorithm the reference selects, kernel path)
ALLREDUCE_D = [(520, "topo_tree", "compact"), (1552, "topo_tree", "oneshot"), (8208, "pt2pt_rs", "oneshot"),
               (40976, "pt2pt_rs", "pipe")]
# MPI_Reduce selects by the packed size count * size: the padded pair types (MPI_SHORT_INT 6 of 8
# bytes, MPI_DOUBLE_INT / MPI_LONG_INT 12 of 16) carry 6.2 KiB at 8,208 B and stay in knomial
REDUCE_D = [(520, "shmem_linear", "compact"), (8208, "redscat_gather", "oneshot"), (40976, "knomial", "pipe")]
REDUCE_PADDED = {8208: "knomial"}
# (target total, algorithm, every count a multiple of 16 / ext).  The kernel follows from the runtime's
# rule (rs_path below): 240 B and 2,000 B run the one-shot kernel element by element, 3 KiB with
# blocks off the 16-byte grid is past the one-shot element limit and runs the pipelined kernel in
# program order with scalar segment heads, 12 KiB with whole-vector blocks the one-shot vector body
REDUCE_SCATTER_D = [(240, "rs_basic", False), (2000, "rs_rec_halving", False), (3072, "rs_rec_halving", False),
                    (12288, "rs_rec_halving", True), (40960, "rs_pairwise", False), (98304, "rs_ring", False)]
RS_ONESHOT_ELEM_MAX, RS_SCALAR_MAX = 2048, 4096
ALLREDUCE_K = [(200, "shmem_linear", "compact"), (520, "shmem_linear", "oneshot")]
RING_K_TOTAL = 49152  # the ring case of run K: n chunks of about 49152 / n bytes and n - 1 elements more
SCAN = [(520, "compact"), (1552, "oneshot"), (40976, "pipe")]


def count_for(nbytes, ext):
    if ext >= 16:
        return nbytes // ext
    count = nbytes // ext + 1
    return count + 1 if count * ext % 16 == 0 else count


def rs_counts(n, ext, target, vec):
    """ragged recvcounts [q + r] of about `target` bytes in all; vec: every count a whole number of
    16-byte vectors, otherwise q * ext is no multiple of 16 (extents below 16)"""
    tri = n * (n - 1) // 2
    if vec:
        per = 16 // ext
        q = (target // 16 - tri) // n
        return [(q + r) * per for r in range(n)]
    q = (target // ext - tri) // n
    while ext < 16 and q * ext % 16 == 0:
        q -= 1
    return [q + r for r in range(n)]


def ring_count(n, ext):
    """n ring chunks of q elements that start off the 16-byte grid, and n - 1 elements left over for
    pt2pt_rs on a base that is not 16-byte aligned"""
    q = RING_K_TOTAL // n // ext
    while ext < 16 and q * ext % 16 == 0:
        q -= 1
    return n * q + n - 1


def _case(kind, tag, seed, op, t, **kw):
    return dict({"id": f"{tag}{seed}", "kind": kind, "type": t, "op": op, "seed": seed, "small": op == "MPI_PROD"}, **kw)


def allreduce_cases(n, run="D", pairs=PAIRS):
    """run D: the default selection; run K: ENV_K / KNOBS_K, with the ring case last"""
    out, seed = [], 1
    for size, algo, path in (ALLREDUCE_D if run == "D" else ALLREDUCE_K):
        for op, t in pairs:
            out.append(_case("allreduce", "ar", seed, op, t, count=count_for(size, TYPES[t][3]), size=size, algo=algo,
                             path=path))
            seed += 1
    if run == "K":
        for op, t in pairs:
            out.append(_case("allreduce", "ar", seed, op, t, count=ring_count(n, TYPES[t][3]), size=RING_K_TOTAL,
                             algo="ring_wrapper", path="pipe", ring=True))
            seed += 1
    return out


def reduce_cases(n, pairs=PAIRS):
    out, seed = [], 1
    for size, algo, path in REDUCE_D:
        for op, t in pairs:
            if TYPES[t][2] != TYPES[t][3]:
                algo_t = REDUCE_PADDED.get(size, algo)
            else:
                algo_t = algo
            out.append(_case("reduce", "rd", seed, op, t, count=count_for(size, TYPES[t][3]), size=size, algo=algo_t,
                             path=path, root=n - 1))
            seed += 1
    return out


def rs_path(t, counts, algo):
    """the kernel MPI_Reduce_scatter takes (runtime/coll_node.cpp reduce_scatter_entry): one-shot
    unless the algorithm is the ring, the type is padded, the operand is above the one-shot limit,
    or a block starts off the 16-byte grid in an operand above 2 KiB; one-shot operands up to 4 KiB
    and misaligned ones run element by element"""
    size, ext = TYPES[t][2], TYPES[t][3]
    total = sum(counts) * ext
    aligned = all(sum(counts[:j]) * ext % 16 == 0 for j in range(len(counts)))
    if algo == "rs_ring" or size != ext or total > ONESHOT_MAX or (not aligned and total > RS_ONESHOT_ELEM_MAX):
        return "pipe"
    return "oneshot_vec" if aligned and total > RS_SCALAR_MAX else "oneshot_elem"


def reduce_scatter_cases(n, pairs=PAIRS):
    out, seed = [], 1
    for size, algo, vec in REDUCE_SCATTER_D:
        for op, t in pairs:
            counts = rs_counts(n, TYPES[t][3], size, vec)
            out.append(_case("reduce_scatter", "rs", seed, op, t, recvcounts=counts, count=sum(counts), size=size,
                             algo=algo, path=rs_path(t, counts, algo), vec=vec))
            seed += 1
    return out


def scan_cases(n, coll, pairs=PAIRS):
    out, seed = [], 1 if coll == "scan" else 2001
    for size, path in SCAN:
        for op, t in pairs:
            out.append(_case("scan", "sc", seed, op, t, coll=coll, count=count_for(size, TYPES[t][3]), size=size,
                             path=path))
            seed += 1
    return out


def nbytes(case):
    return case["count"] * TYPES[case["type"]][3]


def segment_offsets(case, n):
    """byte offsets of the segments of a ring allreduce (its n chunks) or a reduce-scatter (its blocks)"""
    ext = TYPES[case["type"]][3]
    if case["kind"] == "reduce_scatter":
        offs, off = [], 0
        for c in case["recvcounts"]:
            offs.append(off * ext)
            off += c
        return offs
    return [j * (case["count"] // n) * ext for j in range(n)]

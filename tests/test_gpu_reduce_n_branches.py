"""Launch branches of the n-input reduction that test_gpu_reduce_n.py never takes (coll/kernels_impl.h
LReduceN::run): k_reduce_n_elem (any source or the destination off a 16-byte boundary), k_reduce_n on
several workgroups and several grid-stride iterations in every order, a reduce-scatter block edge
inside a vector of a wrapped iteration, and the pair functor's mixed NaN / signed-zero branches
through the LINEAR and butterfly trees.  Bit-exact against the oracle's simulations."""
import ctypes

import numpy as np
import pytest

import mvapich2_amd as m
from mvapich2_amd.consts import OPS, TYPES
from oracle import oracle
from tests.helpers import assert_bytes_equal, rand_typed
from tests.pair_edges import ALL_BRANCHES, PAIR_FLOAT_TYPES, coverage, edge_operands
from tests.test_gpu_reduce_local_branches import c_align, tuning
from tests.test_gpu_reduce_n import PROG_SEL, SEL, newrank_owner, progset

pytestmark = pytest.mark.gpu

RN_THREADS = 256  # k_reduce_n<Rd, 1>: one vector per thread; k_reduce_n_elem: one element per thread
RN_GRID_CAP = 4096  # mv2h_reduce_n: min(rl_grid, 4096)


class Sources:
    """n sources on the device, each also at a byte offset `a` past a 16-byte boundary, and a
    destination with room for the same offset.  The arrays uploaded are the ones the oracle saw."""

    def __init__(self, srcs, tname, count, a):
        self.ext = TYPES[tname][3]
        self.tname, self.count, self.a, self.n = tname, count, a, len(srcs)
        nbytes = count * self.ext
        self.aligned = [m.DeviceBuffer.from_array(s) for s in srcs]
        self.shifted = []
        for s in srcs:
            b = m.DeviceBuffer(nbytes + 16)
            b.upload(s, a)
            self.shifted.append(b)
        self.dst = m.DeviceBuffer(nbytes + 16)
        assert all(b.ptr % 16 == 0 for b in self.aligned + self.shifted + [self.dst])

    def pointers(self, shift_src=None, shift_dst=False):
        ps = [(self.shifted[j].ptr + self.a) if j == shift_src else self.aligned[j].ptr for j in range(self.n)]
        d = self.dst.ptr + (self.a if shift_dst else 0)
        mis = [p for p in ps + [d] if p % 16]
        assert len(mis) == (shift_src is not None) + bool(shift_dst)  # exactly the pointers asked for
        assert all(p % self.a == 0 for p in ps + [d])
        return (ctypes.c_void_p * self.n)(*ps), d

    def fetch(self, d):
        out = np.empty(self.count * self.ext, dtype=np.uint8)
        m.check(m.lib().mv2h_memcpy_dtoh(out.ctypes.data, d, out.nbytes), "dtoh")
        return out

    def tree(self, op, order, owner, **kw):
        arr, d = self.pointers(**kw)
        rc = m.lib().mv2h_reduce_n(arr, self.n, d, self.count, TYPES[self.tname][0], OPS[op], order, owner, None)
        assert rc == 0, rc
        return self.fetch(d)

    def prog(self, op, ps, **kw):
        arr, d = self.pointers(**kw)
        rc = m.lib().mv2h_reduce_n_prog(arr, self.n, d, self.count, TYPES[self.tname][0], OPS[op], ctypes.byref(ps),
                                        None)
        assert rc == 0, rc
        return self.fetch(d)


def pof2_of(n):
    p = 1
    while p * 2 <= n:
        p *= 2
    return p


def tree_orders(srcs, t, op, count):
    """[(what, order, owner, oracle result)] for LINEAR, the reduce-scatter owners and every fixed owner"""
    n, h, oh = len(srcs), TYPES[t][0], OPS[op]
    out = [("linear", 0, 0, oracle.allreduce([s.copy() for s in srcs], count, h, oh, 1)[0])]
    if count >= pof2_of(n):
        out.append(("rs", 1, -1, oracle.allreduce([s.copy() for s in srcs], count, h, oh, 2)[0]))
    outs = oracle.allreduce([s.copy() for s in srcs], count, h, oh, 3)
    seen = set()
    for r in range(n):
        owner = newrank_owner(r, n)
        if owner not in seen:
            seen.add(owner)
            out.append((f"rd rank {r}", 1, owner, outs[r]))
    return out


def shifts(n, i):
    """first one source off the boundary (a different one from case to case), then only the destination"""
    return [dict(shift_src=i % n), dict(shift_dst=True)]


# ---- 6. k_reduce_n_elem ----
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_element_kernel_tree_orders(n):
    rng = np.random.default_rng(600 + n)
    for i, (op, t) in enumerate(SEL):
        for count in (5, 1023):
            srcs = [rand_typed(t, count, rng, small=op == "MPI_PROD") for _ in range(n)]
            dev = Sources(srcs, t, count, c_align(t))
            for what, order, owner, want in tree_orders(srcs, t, op, count):
                for kw in shifts(n, i):
                    got = dev.tree(op, order, owner, **kw)
                    assert_bytes_equal(got, want, t, count, f"{what} n={n} {op} count={count} {kw}")


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_element_kernel_program_order(n):
    """the planner's programs (mv2h_plan) for MPI_Reduce at both end roots, and for MPI_Allreduce"""
    rng = np.random.default_rng(650 + n)
    for i, (op, t) in enumerate(PROG_SEL):
        h, oh = TYPES[t][0], OPS[op]
        for count in (5, 1023):
            srcs = [rand_typed(t, count, rng, small=op == "MPI_PROD") for _ in range(n)]
            flat = [s.view(np.uint8).ravel().copy() for s in srcs]
            dev = Sources(srcs, t, count, c_align(t))
            cases = []
            for root in sorted({0, n - 1}):
                algo, ps = progset("reduce", n, h, count=count, root=root)
                cases.append((f"reduce root={root} algo={oracle.ALGOS[algo]}", ps,
                              oracle.reduce_ref(flat, count, h, oh, root)))
            if count * TYPES[t][2] <= 2048:
                algo, ps = progset("allreduce", n, h, count=count)
                cases.append((f"allreduce algo={oracle.ALGOS[algo]}", ps, oracle.allreduce_ref(flat, count, h, oh)[0]))
            for what, ps, want in cases:
                for kw in shifts(n, i):
                    got = dev.prog(op, ps, **kw)
                    assert_bytes_equal(got, want, t, count, f"{what} n={n} {op} count={count} {kw}")


# ---- 7. several workgroups, several grid-stride iterations ----
@pytest.mark.parametrize("n", [3, 8])
def test_multi_block_and_wrap(n):
    """rl_grid = 2 and 2 x 256 x 2 + 57 vectors plus a scalar tail: two workgroups, three iterations,
    the last partial, in every order; then the same through the element kernel.  For n = 3 the
    reduce-scatter block (count / 2) is no multiple of the vector width, so a vector of a wrapped
    iteration spans two owners (vreduce_n own0 != ownN)."""
    grid = 2
    nvec = grid * RN_THREADS * 2 + 57
    rng = np.random.default_rng(700 + n)
    spans = 0
    with tuning("rl_grid", grid):
        g = min(m.info("rl_grid"), RN_GRID_CAP)
        assert g == grid
        for op, t in SEL:
            ext = TYPES[t][3]
            vpt = 16 // ext
            count = nvec * vpt + vpt - 1
            assert -(-nvec // (g * RN_THREADS)) >= 3 and nvec > RN_THREADS      # several blocks, >= 3 iterations
            assert -(-count // (g * RN_THREADS)) >= 3                          # the element kernel as well
            srcs = [rand_typed(t, count, rng, small=op == "MPI_PROD") for _ in range(n)]
            dev = Sources(srcs, t, count, c_align(t))
            for what, order, owner, want in tree_orders(srcs, t, op, count):
                if what == "rs":
                    rs_blk = count // pof2_of(n)
                    edge = rs_blk  # first element of the second block
                    if vpt > 1 and rs_blk % vpt and edge // vpt >= g * RN_THREADS:
                        spans += 1  # the vector holding the edge is read in a wrapped iteration
                for kw in (dict(), dict(shift_dst=True)):
                    got = dev.tree(op, order, owner, **kw)
                    assert_bytes_equal(got, want, t, count, f"{what} n={n} {op} count={count} {kw}")
        if n == 3:
            assert spans >= 3, spans
        for op, t in PROG_SEL:
            h, oh = TYPES[t][0], OPS[op]
            ext = TYPES[t][3]
            vpt = 16 // ext
            count = nvec * vpt + vpt - 1
            srcs = [rand_typed(t, count, rng, small=op == "MPI_PROD") for _ in range(n)]
            flat = [s.view(np.uint8).ravel().copy() for s in srcs]
            dev = Sources(srcs, t, count, c_align(t))
            for root in sorted({0, n - 1}):
                algo, ps = progset("reduce", n, h, count=count, root=root)
                want = oracle.reduce_ref(flat, count, h, oh, root)
                for kw in (dict(), dict(shift_src=root)):
                    got = dev.prog(op, ps, **kw)
                    assert_bytes_equal(got, want, t, count, f"reduce root={root} algo={oracle.ALGOS[algo]} n={n} {op} "
                                                            f"count={count} {kw}")


# ---- 5. pair edge values through the trees ----
@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("t", PAIR_FLOAT_TYPES)
def test_pair_edge_values_through_the_trees(t, n):
    """operands whose NaNs, signed zeros and ties sit at different positions in every source, LINEAR
    and butterfly (reduce-scatter owners, every fixed owner), vector and element kernel"""
    rng = np.random.default_rng(900 + n)
    count = 200
    for op in ("MPI_MAXLOC", "MPI_MINLOC"):
        srcs = edge_operands(t, count, rng, n)
        assert coverage(srcs[0], srcs[1]) == ALL_BRANCHES
        dev = Sources(srcs, t, count, c_align(t))
        for what, order, owner, want in tree_orders(srcs, t, op, count):
            for kw in (dict(), dict(shift_src=n - 1)):
                got = dev.tree(op, order, owner, **kw)
                assert_bytes_equal(got, want, t, count, f"{what} n={n} {op} {kw}")

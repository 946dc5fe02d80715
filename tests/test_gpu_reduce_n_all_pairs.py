"""Every legal (op, type) pair the device supports -- 291 pairs -- through the n-input reduction
(mv2h_reduce_n, mv2h_reduce_n_prog: k_reduce_n / k_reduce_n_elem) in every order, bit-exact against
the oracle's simulations, at n = 3 (the n <= 4 columns, one folded pair), 5 (n > 4, one folded pair)
and 8 (a power of two, every column used):
  LINEAR                            oracle algo 1
  BUTTERFLY, reduce-scatter owners  oracle algo 2
  BUTTERFLY, fixed owner            oracle algo 3, owners newrank_owner(0, n) and newrank_owner(n - 1, n)
  program order                     the planner's programs for MPI_Reduce at both end roots and for the
                                    topology-aware MPI_Allreduce, as test_program_evaluator_matches_oracle
Counts: 5 (no whole vector) and 4096 // ext + 1 (vectors, an element tail for every extent below 16,
several workgroups for the 1-byte types); the allreduce programs, which exist up to 2 KiB, at 5
and 1552 // ext + 1.  One order per pair runs again with the destination and every source moved off
the 16-byte grid by the type's C alignment (one element for the plain types; 4 or 8 bytes for the
complex and pair types, so the 16-byte ones leave the grid too), which selects k_reduce_n_elem.
The device buffers are allocated once per test."""
import ctypes

import numpy as np
import pytest

import mvapich2_amd as m
from mvapich2_amd.consts import OPS, TYPES
from oracle import oracle
from tests.all_pairs_cases import PAIRS
from tests.helpers import as_bytes, assert_bytes_equal, rand_typed
from tests.test_gpu_reduce_local_branches import c_align
from tests.test_gpu_reduce_n import newrank_owner, progset

pytestmark = pytest.mark.gpu

BIG = 4096
CAP = BIG + 16 + 16  # the largest operand (4096 // ext + 1 elements) and room for the shift


class Device:
    """n source buffers and a destination, allocated once; load() uploads one set of operands at a
    byte shift from the 16-byte grid"""

    def __init__(self, n):
        self.n = n
        self.srcs = [m.DeviceBuffer(CAP) for _ in range(n)]
        self.dst = m.DeviceBuffer(CAP)
        assert all(b.ptr % 16 == 0 for b in self.srcs + [self.dst])
        self.fill = np.full(CAP, 0xA5, dtype=np.uint8)

    def load(self, srcs, t, count, shift):
        self.t, self.count, self.shift, self.nbytes = t, count, shift, count * TYPES[t][3]
        assert self.nbytes + shift <= CAP
        for b, s in zip(self.srcs, srcs):
            b.upload(s, shift)
        self.arr = (ctypes.c_void_p * self.n)(*[b.ptr + shift for b in self.srcs])

    def _result(self, rc):
        assert rc == 0, rc
        return self.dst.download(np.uint8, count=self.nbytes, offset=self.shift)

    def tree(self, op, order, owner):
        self.dst.upload(self.fill)
        return self._result(m.lib().mv2h_reduce_n(self.arr, self.n, self.dst.ptr + self.shift, self.count,
                                                  TYPES[self.t][0], OPS[op], order, owner, None))

    def prog(self, op, ps):
        self.dst.upload(self.fill)
        return self._result(m.lib().mv2h_reduce_n_prog(self.arr, self.n, self.dst.ptr + self.shift, self.count,
                                                       TYPES[self.t][0], OPS[op], ctypes.byref(ps), None))


def pof2_of(n):
    p = 1
    while p * 2 <= n:
        p *= 2
    return p


def counts_of(t):
    return (5, BIG // TYPES[t][3] + 1)


def operands(t, op, count, n, rng):
    return [rand_typed(t, count, rng, small=op == "MPI_PROD") for _ in range(n)]


def tree_orders(srcs, t, op, count):
    """[(what, order, owner, oracle result)]: LINEAR, the reduce-scatter owners (where every block
    has an element), the fixed owners of ranks 0 and n - 1"""
    n, h, oh = len(srcs), TYPES[t][0], OPS[op]
    out = [("linear", 0, 0, oracle.allreduce([s.copy() for s in srcs], count, h, oh, 1)[0])]
    if count >= pof2_of(n):
        out.append(("rs", 1, -1, oracle.allreduce([s.copy() for s in srcs], count, h, oh, 2)[0]))
    outs = oracle.allreduce([s.copy() for s in srcs], count, h, oh, 3)
    for r in (0, n - 1):
        out.append((f"rd rank {r}", 1, newrank_owner(r, n), outs[r]))
    return out


def report(bad):
    assert not bad, f"{len(bad)} results differ from the oracle:\n" + "\n".join(bad[:40])


def compare(bad, got, want, t, count, what):
    try:
        assert_bytes_equal(got, want, t, count, what)
    except AssertionError as e:
        bad.append(str(e))


@pytest.mark.parametrize("n", [3, 5, 8])
def test_tree_orders_all_pairs(n):
    rng = np.random.default_rng(1100 + n)
    dev, bad = Device(n), []
    assert newrank_owner(0, n) != newrank_owner(n - 1, n)
    for op, t in PAIRS:
        for count in counts_of(t):
            srcs = operands(t, op, count, n, rng)
            dev.load(srcs, t, count, 0)
            for what, order, owner, want in tree_orders(srcs, t, op, count):
                compare(bad, dev.tree(op, order, owner), want, t, count, f"{what} n={n} {op} count={count}")
    report(bad)


@pytest.mark.parametrize("n", [3, 5, 8])
def test_program_order_all_pairs(n):
    rng = np.random.default_rng(1200 + n)
    dev, bad = Device(n), []
    for op, t in PAIRS:
        h, oh, size, ext = TYPES[t][0], OPS[op], TYPES[t][2], TYPES[t][3]
        for count in counts_of(t) + (1552 // ext + 1,):
            srcs = operands(t, op, count, n, rng)
            flat = [as_bytes(s).copy() for s in srcs]
            dev.load(srcs, t, count, 0)
            if count != 1552 // ext + 1:
                for root in (0, n - 1):
                    algo, ps = progset("reduce", n, h, count=count, root=root)
                    want = oracle.reduce_ref(flat, count, h, oh, root)
                    compare(bad, dev.prog(op, ps), want, t, count,
                            f"reduce root={root} algo={oracle.ALGOS[algo]} n={n} {op} count={count}")
            if count * size <= 2048:
                algo, ps = progset("allreduce", n, h, count=count)
                assert oracle.ALGOS[algo] == "topo_tree", (t, count, oracle.ALGOS[algo])
                want = oracle.allreduce_ref(flat, count, h, oh)[0]
                compare(bad, dev.prog(op, ps), want, t, count, f"allreduce topo_tree n={n} {op} count={count}")
    report(bad)


@pytest.mark.parametrize("n", [3, 5, 8])
def test_element_kernel_all_pairs(n):
    """the destination and every source off the 16-byte grid; the order rotates from pair to pair
    through LINEAR, the reduce-scatter owners, both fixed owners and the reduce programs"""
    rng = np.random.default_rng(1300 + n)
    dev, bad = Device(n), []
    for i, (op, t) in enumerate(PAIRS):
        h, oh = TYPES[t][0], OPS[op]
        shift = c_align(t)
        assert 0 < shift < 16 and TYPES[t][3] % shift == 0
        for count in counts_of(t):
            srcs = operands(t, op, count, n, rng)
            dev.load(srcs, t, count, shift)
            assert dev.arr[0] % 16 == shift and (dev.dst.ptr + shift) % 16 == shift
            orders = tree_orders(srcs, t, op, count)
            if i % 5 == 4:
                root = (0, n - 1)[(i // 5) % 2]
                algo, ps = progset("reduce", n, h, count=count, root=root)
                want = oracle.reduce_ref([as_bytes(s).copy() for s in srcs], count, h, oh, root)
                compare(bad, dev.prog(op, ps), want, t, count,
                        f"shifted reduce root={root} algo={oracle.ALGOS[algo]} n={n} {op} count={count}")
            else:
                what, order, owner, want = orders[i % 5 % len(orders)]
                compare(bad, dev.tree(op, order, owner), want, t, count, f"shifted {what} n={n} {op} count={count}")
    report(bad)

"""The hand-written MAXLOC / MINLOC known-answer table (tests/pair_edges.py) against the oracle, and
the edge operand's own guarantees.  The same table is run on the device in
test_gpu_reduce_local_branches.py."""
import numpy as np
import pytest

from mvapich2_amd.consts import OPS, TYPES
from oracle import oracle
from tests.helpers import as_bytes, assert_bytes_equal, rand_typed
from tests.pair_edges import ALL_BRANCHES, KAT, PAIR_FLOAT_TYPES, coverage, edge_operands, kat_arrays


def test_pair_float_types_are_the_four_device_kinds():
    assert PAIR_FLOAT_TYPES == ["MPI_FLOAT_INT", "MPI_DOUBLE_INT", "MPI_2REAL", "MPI_2DOUBLE_PRECISION"]


@pytest.mark.parametrize("op", ["MPI_MAXLOC", "MPI_MINLOC"])
@pytest.mark.parametrize("t", PAIR_FLOAT_TYPES)
def test_oracle_matches_the_hand_written_table(t, op):
    x, y, want = kat_arrays(t, op)
    n = len(KAT[op])
    # the two NaNs differ in their bits, so "whose value survives" is visible in the bytes
    assert as_bytes(x["value"][5:6]).tobytes() != as_bytes(y["value"][0:1]).tobytes()
    assert np.isnan(x["value"][5]) and np.isnan(y["value"][0])
    got = y.copy()
    assert oracle.reduce_local(x, got, n, TYPES[t][0], OPS[op]) == 0
    for i, row in enumerate(KAT[op]):
        assert_bytes_equal(got[i:i + 1], want[i:i + 1], t, 1, f"{op} row {i} ({row[0]})")


def test_table_takes_every_branch():
    for op in KAT:
        x, y, _ = kat_arrays("MPI_DOUBLE_INT", op)
        assert coverage(y, x) == ALL_BRANCHES, op


@pytest.mark.parametrize("t", PAIR_FLOAT_TYPES)
def test_edge_operands_meet_different_values(t):
    """Two edge operands take every NaN, signed-zero and tie branch; two rand_typed operands (what
    the older tests feed) take none of the mixed ones."""
    rng = np.random.default_rng(9)
    a, b = edge_operands(t, 64, rng)
    assert coverage(a, b) == ALL_BRANCHES
    assert as_bytes(a["value"][np.isnan(a["value"])][:1]).tobytes() != as_bytes(b["value"][np.isnan(b["value"])][:1]).tobytes()
    a, b = rand_typed(t, 64, rng), rand_typed(t, 64, rng)
    assert not coverage(a, b) & {"nan_num", "num_nan", "mz_pz", "pz_mz"}


def test_rand_typed_is_unchanged_by_the_new_helper():
    """edge_operand is a new helper: what existing callers of rand_typed get stays the same"""
    a = rand_typed("MPI_DOUBLE_INT", 16, np.random.default_rng(3))
    assert np.isnan(a["value"][0]) and np.isnan(a["value"][3])
    assert np.signbit(a["value"][1]) and a["value"][1] == 0 and not np.signbit(a["value"][2])

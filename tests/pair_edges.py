"""MAXLOC / MINLOC operands whose edge values meet *different* values in the other operand, and a
hand-written known-answer table for the branches of the reference's pair macros.

helpers.rand_typed puts [nan, -0.0, 0.0, nan] at the same positions of every operand, so a
reduction only ever sees NaN against NaN and -0.0 against -0.0.  edge_operand() places its edge
values at positions permuted independently per operand, and coverage() names the branches a pair of
operands really takes, so that a test can assert it covers them.

KAT restates opmaxloc.c:65-87 / opminloc.c:65-87 (a = inoutvec, b = invec) by hand:
    a NaN, b NaN      -> a's value kept (a's bits), loc = min(a.loc, b.loc)
    a NaN, b a number -> b's value and loc
    a a number, b NaN -> a untouched
    neither NaN       -> MAXLOC: a < b takes b; a <= b (equal, -0.0 == +0.0 included) keeps a's
                         value bits with loc = min; otherwise a untouched.  MINLOC: > and >=.
The table is checked against the oracle on the CPU and against the device on the GPU: an error in a
restatement shared by the oracle and the device functor cannot agree with it."""
import numpy as np

from mvapich2_amd.consts import DEVICE_UNSUPPORTED, GROUPS, TYPES
from tests.helpers import np_dtype

PAIR_FLOAT_TYPES = [t for t in GROUPS["PAIR"]
                    if t not in DEVICE_UNSUPPORTED and np.dtype(TYPES[t][1])["value"].kind == "f"]
EDGE_X = 3.0  # the value both operands hold with different locs
EDGE_REGION = 60  # 6 copies of the 10 edge entries


def nan_value(vt, payload, negative=False):
    """a quiet NaN of float type vt whose low mantissa bits are `payload`"""
    vt = np.dtype(vt)
    if vt.itemsize == 4:
        bits = np.array([(0xFFC00000 if negative else 0x7FC00000) | payload], dtype=np.uint32)
    else:
        bits = np.array([(0xFFF8000000000000 if negative else 0x7FF8000000000000) | payload], dtype=np.uint64)
    return bits.view(vt)[0]


def edge_operand(type_name, count, rng, tag):
    """Seeded pair operand: small integral values (ties on purpose) and, in its first
    min(count, EDGE_REGION) elements, the edge values {nan, -0.0, +0.0, x, x with another loc, +inf,
    -inf} (the NaN and the zeros twice as often) in an order drawn for this operand alone.  tag: the
    operand's NaN payload, so the bits of a surviving NaN name the operand they came from."""
    dt = np_dtype(type_name)
    vt, lt = dt["value"], dt["loc"]
    assert vt.kind == "f", type_name
    x = np.zeros(count, dtype=dt)
    x["value"] = np.floor(rng.uniform(-8, 8, count)).astype(vt)
    x["loc"] = rng.integers(0, 8, count).astype(lt)
    nan = nan_value(vt, tag, tag & 1)
    vals = np.array([nan, nan, -0.0, -0.0, 0.0, 0.0, EDGE_X, EDGE_X, np.inf, -np.inf], dtype=vt)
    locs = [None, None, None, None, None, None, 2, 5, None, None]
    region = min(count, EDGE_REGION)
    order = rng.permutation(np.arange(EDGE_REGION) % len(vals))[:region]
    x["value"][:region] = vals[order]
    for i, k in enumerate(order):
        if locs[k] is not None:
            x["loc"][i] = locs[k]
    return x


def edge_operands(type_name, count, rng, n=2):
    """n edge operands; each is drawn again until it and the one before it take every branch of
    ALL_BRANCHES between them (the positions are independent, so one draw may miss a branch)"""
    assert count >= EDGE_REGION
    out = [edge_operand(type_name, count, rng, 1)]
    for j in range(1, n):
        for _ in range(100):
            x = edge_operand(type_name, count, rng, 1 + j)
            if coverage(out[-1], x) == ALL_BRANCHES:
                break
        else:
            raise AssertionError("no covering edge operand in 100 draws")
        out.append(x)
    return out


def coverage(a, b):
    """the branches of the pair macros that (inout a, in b) takes somewhere"""
    av, bv = a["value"], b["value"]
    an, bn = np.isnan(av), np.isnan(bv)
    seen = set()
    if np.any(an & bn):
        seen.add("nan_nan")
    if np.any(an & ~bn):
        seen.add("nan_num")
    if np.any(~an & bn):
        seen.add("num_nan")
    zero = (av == 0) & (bv == 0)
    if np.any(zero & np.signbit(av) & ~np.signbit(bv)):
        seen.add("mz_pz")
    if np.any(zero & ~np.signbit(av) & np.signbit(bv)):
        seen.add("pz_mz")
    if np.any((av == bv) & (av != 0) & (a["loc"] != b["loc"])):
        seen.add("tie_loc")
    return seen


ALL_BRANCHES = {"nan_nan", "nan_num", "num_nan", "mz_pz", "pz_mz", "tie_loc"}

# (what, a = inout (value, loc), b = in (value, loc), whose value bits survive, resulting loc)
# "nanA" / "nanB": NaNs with different payloads and signs
_BOTH = [
    ("nan nan, a.loc larger", ("nanA", 5), ("nanB", 2), "a", 2),
    ("nan nan, a.loc smaller", ("nanA", 2), ("nanB", 5), "a", 2),
    ("nan num", ("nanA", 1), (3.0, 7), "b", 7),
    ("nan -inf", ("nanA", 1), (-np.inf, 7), "b", 7),
    ("nan +inf", ("nanA", 6), (np.inf, 0), "b", 0),
    ("num nan", (3.0, 7), ("nanB", 1), "a", 7),
    ("-inf nan", (-np.inf, 7), ("nanB", 1), "a", 7),
    ("+inf nan", (np.inf, 7), ("nanB", 1), "a", 7),
    ("-0 +0", (-0.0, 4), (0.0, 3), "a", 3),
    ("+0 -0", (0.0, 3), (-0.0, 4), "a", 3),
    ("-0 +0, a.loc smaller", (-0.0, 1), (0.0, 6), "a", 1),
    ("tie, b.loc smaller", (3.0, 6), (3.0, 2), "a", 2),
    ("tie, a.loc smaller", (3.0, 2), (3.0, 6), "a", 2),
    ("inf tie", (np.inf, 6), (np.inf, 1), "a", 1),
    ("-inf tie", (-np.inf, 0), (-np.inf, 1), "a", 0),
]
KAT = {
    "MPI_MAXLOC": _BOTH + [
        ("a < b", (1.0, 0), (3.0, 7), "b", 7),
        ("a > b", (3.0, 7), (1.0, 0), "a", 7),
        ("-inf < +inf", (-np.inf, 0), (np.inf, 4), "b", 4),
        ("+inf > num", (np.inf, 5), (3.0, 1), "a", 5),
        ("-0 < num", (-0.0, 5), (1.0, 6), "b", 6),
    ],
    "MPI_MINLOC": _BOTH + [
        ("a < b", (1.0, 0), (3.0, 7), "a", 0),
        ("a > b", (3.0, 7), (1.0, 0), "b", 0),
        ("-inf < +inf", (-np.inf, 0), (np.inf, 4), "a", 0),
        ("+inf > num", (np.inf, 5), (3.0, 1), "b", 1),
        ("+0 > -num", (0.0, 5), (-1.0, 6), "b", 6),
    ],
}


def kat_arrays(type_name, op):
    """(in, inout, expected) arrays of the table for one pair type; the padding bytes of expected
    are inout's (helpers.data_mask masks them anyway)"""
    dt = np_dtype(type_name)
    vt = dt["value"]
    rows = KAT[op]

    def val(v):
        if v == "nanA":
            return nan_value(vt, 0x11)
        if v == "nanB":
            return nan_value(vt, 0x22, negative=True)
        return vt.type(v)
    n = len(rows)
    x, y = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
    for i, (_, a, b, _, _) in enumerate(rows):
        y["value"][i], y["loc"][i] = val(a[0]), a[1]
        x["value"][i], x["loc"][i] = val(b[0]), b[1]
    want = y.copy()
    for i, (_, _, _, keep, loc) in enumerate(rows):
        want["value"][i] = (y if keep == "a" else x)["value"][i]
        want["loc"][i] = loc
    return x, y, want

"""Launch branches of MPI_Reduce_local that the all-pairs test never takes (coll/kernels_impl.h
LReduceLocal::run): the element-granular kernel on the 16-byte kinds and with one operand aligned
and the other not, the grid-stride loops' second and later iterations, the sizes at which the
launcher switches kernel or a tile fills, one host and one device operand, the mixed NaN /
signed-zero / tie branches of the pair functor, and the completion word's counting at grids of
every regime (device_util.h block_done).  Everything bit-exact against the oracle.

Each test reads the launcher's tunings through m.info, asserts in Python that its shape really is
on the branch it names, and restores every tuning it changes."""
import contextlib

import numpy as np
import pytest

import mvapich2_amd as m
from mvapich2_amd.consts import DEVICE_UNSUPPORTED, OPS, TYPES, legal_pairs
from oracle import oracle
from tests.helpers import assert_bytes_equal, np_dtype, rand_typed
from tests.pair_edges import ALL_BRANCHES, KAT, PAIR_FLOAT_TYPES, coverage, edge_operands, kat_arrays

pytestmark = pytest.mark.gpu
PAIRS = [(op, t) for op, t in legal_pairs() if t not in DEVICE_UNSUPPORTED]

# k_reduce_local's tile: kRLThreads x U vectors of 16 bytes per workgroup and iteration (U = 2,
# LReduceLocal::run); k_reduce_local_elem: kThreads elements.  Not readable through mv2h_get_info.
RL_THREADS, RL_U = 512, 2
RL_TILE = RL_THREADS * RL_U
ELEM_THREADS = 256

# one (op, type) per element width, a padded pair and a complex among them
WIDTHS = [("MPI_BXOR", "MPI_UNSIGNED_CHAR"), ("MPI_MAX", "MPI_SHORT"), ("MPI_SUM", "MPI_FLOAT"),
          ("MPI_MINLOC", "MPI_SHORT_INT"), ("MPI_MIN", "MPI_DOUBLE"), ("MPI_PROD", "MPI_C_DOUBLE_COMPLEX"),
          ("MPI_MAXLOC", "MPI_DOUBLE_INT")]


def c_align(tname):
    """the type's C alignment: its widest member, at most 8"""
    dt = np_dtype(tname)
    if dt.names:
        return min(8, max(dt[f].itemsize for f in dt.names))
    if dt.kind == "c":
        return dt.itemsize // 2
    return min(8, dt.itemsize)


def test_widths_cover_every_element_size():
    assert sorted({TYPES[t][3] for _, t in WIDTHS}) == [1, 2, 4, 8, 16]
    assert [c_align(t) for t in ("MPI_DOUBLE_INT", "MPI_LONG_INT", "MPI_C_DOUBLE_COMPLEX", "MPI_SHORT_INT",
                                 "MPI_2DOUBLE_PRECISION", "MPI_C_FLOAT_COMPLEX", "MPI_CHAR")] == [8, 8, 8, 4, 8, 4, 1]


@contextlib.contextmanager
def tuning(key, value):
    """set one tuning for the block; the value read before it is put back"""
    old = m.info(key)
    m.check(m.lib().mv2h_set_tuning(key.encode(), value), key)
    try:
        assert m.info(key) == value
        yield
    finally:
        m.check(m.lib().mv2h_set_tuning(key.encode(), old), key)
        assert m.info(key) == old


class Operands:
    """two device buffers with room for byte offsets up to `slack`; run() uploads x / y at the given
    byte offsets and returns the device's inout bytes"""

    def __init__(self, nbytes, slack=16):
        self.a, self.b = m.DeviceBuffer(nbytes + slack), m.DeviceBuffer(nbytes + slack)
        assert self.a.ptr % 16 == 0 and self.b.ptr % 16 == 0  # offset 0 is the 16-byte-aligned path
        self.slack = slack

    def run(self, tname, op, x, y, count, off_in=0, off_io=0):
        ext = TYPES[tname][3]
        assert max(off_in, off_io) <= self.slack and x.nbytes == y.nbytes == count * ext
        self.a.upload(x, off_in)
        self.b.upload(y, off_io)
        rc = m.lib().MPI_Reduce_local(self.a.ptr + off_in, self.b.ptr + off_io, count, TYPES[tname][0], OPS[op])
        assert rc == 0, (tname, op, rc)
        return self.b.download(np.uint8, count=count * ext, offset=off_io)


def reference(t, op, count, rng):
    small = op == "MPI_PROD"
    x, y = rand_typed(t, count, rng, small=small), rand_typed(t, count, rng, small=small)
    want = y.copy()
    assert oracle.reduce_local(x, want, count, TYPES[t][0], OPS[op]) == 0
    return x, y, want


# ---- 1. byte-alignment matrix ----
@pytest.mark.parametrize("size", ["tiny", "streaming"])
def test_byte_alignment_matrix(size):
    """Every legal (op, type) with the operands shifted by the type's C alignment, together and apart.
    The 16-byte kinds (double-int, long-int, double complex, 2 x double) are 8-byte aligned in C: a
    shift by one element, as in test_all_pairs_bit_exact, never takes them off the vector kernel."""
    tiny_max = m.info("rl_tiny_max")
    rng = np.random.default_rng(41 + len(size))
    sixteen = set()
    for op, t in PAIRS:
        ext, a = TYPES[t][3], c_align(t)
        count = 5 if size == "tiny" else tiny_max // ext + 1 + 7
        assert (count * ext <= tiny_max) == (size == "tiny"), (t, count, tiny_max)
        x, y, want = reference(t, op, count, rng)
        ops = Operands(count * ext)
        for off_in, off_io in ((0, 0), (a, 0), (0, a), (a, a), (a, 2 * a)):
            pin, pio = ops.a.ptr + off_in, ops.b.ptr + off_io
            assert pin % a == 0 and pio % a == 0
            if (off_in, off_io) != (0, 0):
                assert pin % 16 or pio % 16, (t, off_in, off_io)  # the element-granular branch
                if ext == 16:
                    assert any(p % 8 == 0 and p % 16 for p in (pin, pio)), (t, off_in, off_io)
                    sixteen.add(t)
            got = ops.run(t, op, x, y, count, off_in, off_io)
            assert_bytes_equal(got, want, t, count, f"{op} count={count} off=({off_in},{off_io})")
    assert sixteen >= {"MPI_DOUBLE_INT", "MPI_LONG_INT", "MPI_C_DOUBLE_COMPLEX", "MPI_DOUBLE_COMPLEX",
                       "MPI_2DOUBLE_PRECISION"}


# ---- 2. grid-stride wrap ----
@pytest.mark.parametrize("grid", [1, 2, 3])
def test_grid_stride_wrap(grid):
    """rl_grid below the tile count: k_reduce_local's `base += stride` and k_reduce_local_elem's
    `e += stride` run several iterations (at the default grid they wrap only above 16 GiB).  Seven
    tiles, the last partial with its second unroll slot partly live, and a scalar tail."""
    nvec = 6 * RL_TILE + RL_THREADS + 1
    rng = np.random.default_rng(200 + grid)
    assert m.info("rl_grid") >= 1
    with tuning("rl_grid", grid):
        for op, t in WIDTHS:
            ext, a = TYPES[t][3], c_align(t)
            vpt = 16 // ext
            count = nvec * vpt + vpt - 1
            tiles = -(-nvec // RL_TILE)
            assert tiles == 7 and tiles > m.info("rl_grid")
            assert RL_THREADS < nvec % RL_TILE < RL_TILE            # second slot live for some threads only
            assert count * ext > m.info("rl_tiny_max")
            assert count > 3 * ELEM_THREADS * 2 >= m.info("rl_grid") * ELEM_THREADS * 2  # the element kernel wraps too
            x, y, want = reference(t, op, count, rng)
            ops = Operands(count * ext)
            for off_in, off_io in ((0, 0), (a, a), (0, a)):
                assert bool((ops.a.ptr + off_in) % 16 or (ops.b.ptr + off_io) % 16) == bool(off_in or off_io)
                got = ops.run(t, op, x, y, count, off_in, off_io)
                assert_bytes_equal(got, want, t, count, f"{op} rl_grid={grid} off=({off_in},{off_io})")


# ---- 3. size boundaries ----
def test_tiny_to_streaming_switch():
    """the largest operand of the one-wave kernel, one element less and one element more"""
    tiny_max = m.info("rl_tiny_max")
    rng = np.random.default_rng(31)
    for op, t in WIDTHS:
        ext = TYPES[t][3]
        assert tiny_max % ext == 0 and tiny_max >= 2 * ext, (t, tiny_max)
        at = tiny_max // ext
        for count in (at - 1, at, at + 1):
            assert (count * ext < tiny_max, count * ext == tiny_max, count * ext > tiny_max) == \
                (count == at - 1, count == at, count == at + 1)
            x, y, want = reference(t, op, count, rng)
            ops = Operands(count * ext)
            assert_bytes_equal(ops.run(t, op, x, y, count), want, t, count, f"{op} bytes={count * ext}")


@pytest.mark.parametrize("nvec", [511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049])
def test_tile_edges(nvec):
    """vector counts around one unroll slot (kRLThreads), one tile and two tiles, without and with a
    full scalar tail: the `i < nvec` guard of each slot, and the last workgroup's tail"""
    assert {RL_THREADS, RL_TILE, 2 * RL_TILE} & {nvec - 1, nvec, nvec + 1}
    tiny_max = m.info("rl_tiny_max")
    assert m.info("rl_grid") >= 3  # one tile per workgroup at these sizes
    rng = np.random.default_rng(nvec)
    for op, t in WIDTHS:
        ext = TYPES[t][3]
        vpt = 16 // ext
        for tail in sorted({0, vpt - 1}):
            count = nvec * vpt + tail
            assert count * ext > tiny_max and count // vpt == nvec and count % vpt == tail
            x, y, want = reference(t, op, count, rng)
            ops = Operands(count * ext)
            assert_bytes_equal(ops.run(t, op, x, y, count), want, t, count, f"{op} nvec={nvec} tail={tail}")


# ---- 4. one host and one device operand ----
def host_copy(arr, misalign):
    """a host copy of arr whose address is `misalign` past a 16-byte boundary"""
    raw = np.zeros(arr.nbytes + 32, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + misalign
    view = raw[start:start + arr.nbytes]
    view[:] = arr.view(np.uint8).ravel()
    assert view.ctypes.data % 16 == misalign % 16
    return view


@pytest.mark.parametrize("op,t", [("MPI_SUM", "MPI_FLOAT"), ("MPI_PROD", "MPI_C_FLOAT_COMPLEX"),
                                  ("MPI_MAXLOC", "MPI_DOUBLE_INT")])
def test_mixed_host_and_device_operands(op, t):
    """runtime/coll.cpp mv2h_reduce_local stages each host operand on its own: host in with device
    inout, and device in with host inout (whose result is copied back).  The host pointer has the
    type's natural alignment and is not 16-byte aligned."""
    L = m.lib()
    tiny_max = m.info("rl_tiny_max")
    ext, a = TYPES[t][3], c_align(t)
    assert sorted(TYPES[u][3] for u in ("MPI_FLOAT", "MPI_C_FLOAT_COMPLEX", "MPI_DOUBLE_INT")) == [4, 8, 16]
    rng = np.random.default_rng(ext)
    for count in (7, tiny_max // ext + 1 + 7):
        assert (count * ext > tiny_max) == (count != 7)
        x, y, want = reference(t, op, count, rng)
        # host in, device inout
        hx = host_copy(x, a)
        assert hx.ctypes.data % a == 0 and hx.ctypes.data % 16 != 0
        assert not L.mv2h_is_device_ptr(hx.ctypes.data)
        d = m.DeviceBuffer.from_array(y)
        assert L.MPI_Reduce_local(hx.ctypes.data, d.ptr, count, TYPES[t][0], OPS[op]) == 0
        assert_bytes_equal(d.download(np.uint8, count=count * ext), want, t, count, f"{op} host in, count={count}")
        assert np.array_equal(hx, x.view(np.uint8).ravel())  # the input operand is left alone
        # device in, host inout
        hy = host_copy(y, a)
        assert hy.ctypes.data % a == 0 and hy.ctypes.data % 16 != 0
        d = m.DeviceBuffer.from_array(x)
        assert L.MPI_Reduce_local(d.ptr, hy.ctypes.data, count, TYPES[t][0], OPS[op]) == 0
        assert_bytes_equal(hy, want, t, count, f"{op} host inout, count={count}")
        assert np.array_equal(d.download(np.uint8, count=count * ext), x.view(np.uint8).ravel())


# ---- 5. pair edge values ----
def pair_paths(t):
    """(count, byte offset) of the one-wave, the vector and the element-granular kernel"""
    tiny_max = m.info("rl_tiny_max")
    ext = TYPES[t][3]
    tiny, stream = tiny_max // ext, tiny_max // ext + 1 + 7
    assert tiny * ext <= tiny_max < stream * ext and tiny >= 60
    return [("tiny", tiny, 0), ("vector", stream, 0), ("element", stream, c_align(t))]


@pytest.mark.parametrize("op", ["MPI_MAXLOC", "MPI_MINLOC"])
@pytest.mark.parametrize("t", PAIR_FLOAT_TYPES)
def test_pair_edge_values(t, op):
    """NaN against a number (both ways), -0.0 against +0.0 (both ways) and equal values with
    different locs, through the one-wave, the vector and the element-granular kernel"""
    rng = np.random.default_rng(77)
    for path, count, off in pair_paths(t):
        y, x = edge_operands(t, count, rng)
        assert coverage(y, x) == ALL_BRANCHES, (path, coverage(y, x))
        want = y.copy()
        assert oracle.reduce_local(x, want, count, TYPES[t][0], OPS[op]) == 0
        ops = Operands(count * TYPES[t][3])
        assert bool((ops.a.ptr + off) % 16) == (path == "element")
        got = ops.run(t, op, x, y, count, off, off)
        assert_bytes_equal(got, want, t, count, f"{op} {path}")


@pytest.mark.parametrize("op", ["MPI_MAXLOC", "MPI_MINLOC"])
@pytest.mark.parametrize("t", PAIR_FLOAT_TYPES)
def test_pair_known_answers_on_the_device(t, op):
    """the hand-written table (tests/pair_edges.py KAT; checked against the oracle by
    test_pair_known_answers.py) through the three kernels: as it stands (one wave), and repeated
    past rl_tiny_max at an aligned and at a misaligned address"""
    tiny_max = m.info("rl_tiny_max")
    ext = TYPES[t][3]
    x, y, want = kat_arrays(t, op)
    rows = len(KAT[op])
    assert rows * ext <= tiny_max
    reps = tiny_max // (rows * ext) + 2
    for path, rep, off in (("tiny", 1, 0), ("vector", reps, 0), ("element", reps, c_align(t))):
        count = rows * rep
        assert (count * ext > tiny_max) == (path != "tiny")
        xs, ys, ws = np.tile(x, rep), np.tile(y, rep), np.tile(want, rep)
        ops = Operands(count * ext)
        assert bool((ops.b.ptr + off) % 16) == (path == "element")
        got = ops.run(t, op, xs, ys, count, off, off).view(np.uint8).reshape(count, ext)
        wb = ws.view(np.uint8).reshape(count, ext)
        for i in range(count):
            assert_bytes_equal(got[i], wb[i], t, 1, f"{op} {path} row {i % rows} ({KAT[op][i % rows][0]})")


# ---- 8. completion word ----
SWEEP = list(range(1, 18)) + [63, 64, 65, 71, 127, 128, 129, 511, 512, 513]


def test_completion_word_counts_at_every_grid():
    """block_done's members / subs / groups arithmetic has three regimes of gridDim.x (below 8, 8 to
    63, 64 and more) and remainders in each; a miscount does not hang, the host falls back to the
    stream and counts done_missed.  One tile per workgroup, so count = g x 4096 ints is a grid of g."""
    L = m.lib()
    assert m.info("rl_grid") >= max(SWEEP)
    assert any(g < 8 for g in SWEEP) and any(8 <= g < 64 for g in SWEEP) and any(g >= 64 for g in SWEEP)
    per_tile = RL_TILE * 4
    assert per_tile == 4096
    nmax = max(SWEEP) * per_tile
    rng = np.random.default_rng(8)
    x = rng.integers(-(2**31), 2**31 - 1, nmax, dtype=np.int64).astype(np.int32)
    y = rng.integers(-(2**31), 2**31 - 1, nmax, dtype=np.int64).astype(np.int32)
    want = y.copy()
    assert oracle.reduce_local(x, want, nmax, TYPES["MPI_INT"][0], OPS["MPI_SUM"]) == 0
    a, b = m.DeviceBuffer.from_array(x), m.DeviceBuffer(nmax * 4)
    missed = m.info("done_missed")
    for g in SWEEP:
        count = g * per_tile
        assert -(-(count // 4) // RL_TILE) == g and count * 4 > m.info("rl_tiny_max")
        b.upload(y[:count])
        assert L.MPI_Reduce_local(a.ptr, b.ptr, count, TYPES["MPI_INT"][0], OPS["MPI_SUM"]) == 0
        assert np.array_equal(b.download(np.int32, count=count), want[:count]), g
        assert m.info("done_missed") == missed, g

"""Launch branches of the device pack / unpack that test_gpu_pack.py never takes (pack/pack.hip): a
misaligned packed side, k_pack_lds workgroups that start at an unaligned packed offset, the run-table
kernel past one grid pass (with the LDS and the global-memory table, with an element larger than a
pass, with pointers that lower the unit width), MPI_Pack / MPI_Unpack at a nonzero position, and the
completion word of the pack kernels at grids of every regime.  Byte-exact against the oracle's
segment walk; every test asserts in Python that its shape is on the branch it names."""
import ctypes

import numpy as np
import pytest

import mvapich2_amd as m
from oracle import oracle
from oracle import typemap as tm
from tests.test_gpu_pack import _segments as segments
from tests.typecases import CASES, Built, oracle_type

pytestmark = pytest.mark.gpu

# constants of pack/pack.hip that mv2h_get_info does not export
LDS_SPAN = 32768          # kLdsSpan: k_pack_lds stages (kLdsSpan - 32) / stride rows per workgroup
UNITS_TILE = 512 * 2      # k_pack_units: kPackThreads x kPackU units per workgroup
RUNS_THREADS, RUNS_GRID = 256, 4096  # k_pack_runs: kThreads, launch_pack_runs' grid cap
RUNS_LDS = 512            # kRunLds: larger run tables stay in global memory
CANARY = 0xA5


def takes_lds(blk, stride, unpack):
    """launch_pack_strided's choice of k_pack_lds"""
    return not unpack and blk < 16 and blk <= stride <= 64


def unit_width(*values):
    """the widest of 16 / 8 / 4 / 2 / 1 bytes that divides every value (sizes and addresses)"""
    g = 16
    while g > 1 and any(v % g for v in values):
        g >>= 1
    return g


def strided(nb, blk, stride, off, poff, rng, seen=None):
    """pack and unpack nb rows with the strided side at byte offset off and the packed side at byte
    offset poff of their allocations; everything outside the written bytes must stay as it was"""
    L = m.lib()
    span = (nb - 1) * stride + blk
    src = rng.integers(0, 256, span + 64, dtype=np.uint8)
    d_src = m.DeviceBuffer.from_array(src)
    d_pk = m.DeviceBuffer.from_array(np.full(nb * blk + 64, CANARY, dtype=np.uint8))
    assert d_src.ptr % 16 == 0 and d_pk.ptr % 16 == 0 and off + 15 < 64 and poff < 64
    if seen is not None:
        for unpack in (0, 1):
            if not takes_lds(blk, stride, unpack):
                seen.add(unit_width(blk, stride, d_src.ptr + off, d_pk.ptr + poff))
    assert L.mv2h_pack_strided(d_src.ptr + off, d_pk.ptr + poff, nb, blk, stride, None) == 0
    want = oracle.pack_strided(src[off:].copy(), nb, blk, stride)
    got = d_pk.download(np.uint8)
    assert np.array_equal(got[poff:poff + nb * blk], want), ("pack", nb, blk, stride, off, poff)
    assert np.all(got[:poff] == CANARY) and np.all(got[poff + nb * blk:] == CANARY), ("pack spill", nb, blk, stride, off, poff)
    canvas = rng.integers(0, 256, span + 64, dtype=np.uint8)
    d_can = m.DeviceBuffer.from_array(canvas)
    assert L.mv2h_unpack_strided(d_pk.ptr + poff, d_can.ptr + off, nb, blk, stride, None) == 0
    w2 = canvas.copy()
    tmp = w2[off:].copy()
    oracle.unpack_strided(want, tmp, nb, blk, stride)
    w2[off:] = tmp
    assert np.array_equal(d_can.download(np.uint8), w2), ("unpack", nb, blk, stride, off, poff)


# ---- 9. independent byte offsets of the two sides ----
OFFSET_SHAPES = [(777, 16, 48), (1000, 4, 32), (50, 1000, 1024), (333, 64, 64), (3, 7, 9)]


@pytest.mark.parametrize("nb,blk,stride", OFFSET_SHAPES)
def test_strided_independent_offsets(nb, blk, stride):
    rng = np.random.default_rng(nb * 11 + blk)
    seen = set()
    for off in (0, 1, 2, 4, 8):
        for poff in (0, 1, 2, 4, 8):
            strided(nb, blk, stride, off, poff, rng, seen)
    if blk % 16 == 0 and stride % 16 == 0:
        assert seen == {16, 8, 4, 2, 1}  # the offsets alone take the unit width through every value
    else:
        assert seen and max(seen) == unit_width(blk, stride)


def test_offset_shapes_reach_every_unit_width_and_the_lds_kernel():
    assert any(b % 16 == 0 and s % 16 == 0 for _, b, s in OFFSET_SHAPES)
    assert any(takes_lds(b, s, 0) for _, b, s in OFFSET_SHAPES)
    assert {unit_width(b, s) for _, b, s in OFFSET_SHAPES} >= {16, 8, 4, 1}


# ---- 10. k_pack_lds over several workgroups ----
@pytest.mark.parametrize("blk,stride,rows_per_wg,rem,nb", [(3, 5, 6547, 9, 19652), (7, 64, 511, 9, 1600),
                                                           (15, 15, 2182, 10, 4500), (8, 24, 1364, 0, 3000)])
def test_lds_pack_workgroups_at_unaligned_packed_offsets(blk, stride, rows_per_wg, rem, nb):
    """rows_per_wg x blk is no multiple of 16 in the first three shapes: the second and later
    workgroups start at an unaligned packed offset and write their whole output by bytes; the fourth
    keeps every workgroup on the 16-byte stores.  The last workgroup is partial in all of them."""
    assert takes_lds(blk, stride, 0)
    assert (LDS_SPAN - 32) // stride == rows_per_wg and (rows_per_wg * blk) % 16 == rem
    groups = -(-nb // rows_per_wg)
    assert groups >= 3 and nb % rows_per_wg
    starts = {(w * rows_per_wg * blk) % 16 for w in range(groups)}
    assert (starts == {0}) == (rem == 0)
    rng = np.random.default_rng(blk * 100 + stride)
    missed = m.info("done_missed")
    for off in (0, 3):
        strided(nb, blk, stride, off, 0, rng)
    assert m.info("done_missed") == missed


# ---- 11. the run table past one grid pass ----
def fold_runs(offs, lens, g):
    """launch_pack_runs' folding rule restated: equal-length blocks at a constant distance are one run"""
    runs = []  # [blk, nrep, off, stride]
    for off, ln in zip(offs, lens):
        off, ln = off // g, ln // g
        if runs:
            r = runs[-1]
            last = r[2] + (r[1] - 1) * r[3]
            if r[0] == ln and (r[1] == 1 or off - last == r[3]):
                if r[1] == 1:
                    r[3] = off - last
                r[1] += 1
                continue
        runs.append([ln, 1, off, 0])
    return len(runs)


def run_table(offs, lens, extent, count, rng, src_off=0, dst_off=0):
    """pack then unpack through mv2h_pack_segments with the strided side at src_off and the packed
    side at dst_off; returns (unit width, runs, units per element) as the launcher derives them"""
    L = m.lib()
    nseg = len(offs)
    end = max(o + n for o, n in zip(offs, lens))
    span = (count - 1) * extent + end
    src = rng.integers(0, 256, span + 32, dtype=np.uint8)
    packed_n = count * sum(lens)
    want = np.zeros(packed_n, dtype=np.uint8)
    oracle.pack_segments(src[src_off:].copy(), want, count, extent, offs, lens)
    o64 = (ctypes.c_int64 * nseg)(*offs)
    l64 = (ctypes.c_int64 * nseg)(*lens)
    d_src = m.DeviceBuffer.from_array(src)
    d_pk = m.DeviceBuffer.from_array(np.full(packed_n + 32, CANARY, dtype=np.uint8))
    assert d_src.ptr % 16 == 0 and d_pk.ptr % 16 == 0 and src_off < 32 and dst_off < 32
    g = unit_width(extent, d_src.ptr + src_off, d_pk.ptr + dst_off, *offs, *lens)
    assert L.mv2h_pack_segments(d_src.ptr + src_off, d_pk.ptr + dst_off, count, extent, o64, l64, nseg, 0, None) == 0
    got = d_pk.download(np.uint8)
    assert np.array_equal(got[dst_off:dst_off + packed_n], want), "pack"
    assert np.all(got[:dst_off] == CANARY) and np.all(got[dst_off + packed_n:] == CANARY), "pack spill"
    canvas = rng.integers(0, 256, span + 32, dtype=np.uint8)
    d_can = m.DeviceBuffer.from_array(canvas)
    assert L.mv2h_pack_segments(d_pk.ptr + dst_off, d_can.ptr + src_off, count, extent, o64, l64, nseg, 1, None) == 0
    w2 = canvas.copy()
    tmp = w2[src_off:].copy()
    oracle.pack_segments(want, tmp, count, extent, offs, lens, unpack=True)
    w2[src_off:] = tmp
    assert np.array_equal(d_can.download(np.uint8), w2), "unpack"  # gap bytes included
    return g, fold_runs(offs, lens, g), sum(lens) // g


PASS_UNITS = RUNS_GRID * RUNS_THREADS  # units one grid pass of k_pack_runs moves
WRAP_BYTES = 3 * PASS_UNITS + 12345    # packed bytes of cases (a) and (b): more than three passes at g = 1


def test_run_table_wraps_with_the_lds_table():
    """(a) byte units, 40 segments, more than three grid passes: the (element, unit) pair advances
    by (se, sq) from pass to pass"""
    rng = np.random.default_rng(1101)
    offs, lens, end = segments(rng, 40, 1)
    upe = sum(lens)
    count = -(-WRAP_BYTES // upe)
    g, nrun, units = run_table(offs, lens, end + 1, count, rng)
    assert g == 1 and units == upe and nrun <= RUNS_LDS
    assert count * units > 3 * PASS_UNITS
    assert 0 < PASS_UNITS % units and PASS_UNITS // units > 0  # both se and sq are nonzero


def test_run_table_wraps_with_the_global_table():
    """(b) lengths alternate so that no two blocks fold: more than 512 runs, the table is read from
    global memory, over the same number of passes as (a)"""
    rng = np.random.default_rng(1102)
    offs, lens, pos = [], [], 0
    for k in range(600):
        pos += int(rng.integers(0, 4))
        ln = 1 + k % 2
        offs.append(pos)
        lens.append(ln)
        pos += ln
    upe = sum(lens)
    count = -(-WRAP_BYTES // upe)
    g, nrun, units = run_table(offs, lens, pos + 1, count, rng)
    assert g == 1 and nrun == 600 and nrun > RUNS_LDS
    assert count * units > 3 * PASS_UNITS


def test_run_table_element_larger_than_a_pass():
    """(c) three 500 000-byte segments, two elements, byte units: one element is more than one grid
    pass, so se = 0 and a thread stays inside an element for a pass or crosses into the next.  The
    first two segments fold into one run of two blocks, the third is at another distance."""
    rng = np.random.default_rng(1103)
    lens = [500000] * 3
    offs = [1, 500004, 1000019]
    g, nrun, units = run_table(offs, lens, 1500040, 2, rng)
    assert g == 1 and nrun == 2
    assert units > PASS_UNITS


def test_run_table_pointers_lower_the_unit_width():
    """(d) a table, an extent and lengths of 16-byte multiples; src + 4 and dst + 8 alone lower the
    unit to 4 bytes"""
    rng = np.random.default_rng(1104)
    offs, lens, end = segments(rng, 40, 16)
    assert unit_width(end + 16, *offs, *lens) == 16
    g, nrun, units = run_table(offs, lens, end + 16, 300, rng, src_off=4, dst_off=8)
    assert g == 4 and units == sum(lens) // 4


# ---- 12. MPI_Pack / MPI_Unpack at a nonzero position ----
BY_NAME = {c[0]: c for c in CASES}


@pytest.mark.parametrize("first,second", [("vector_count3", "struct_nested"), ("pair_double_int", "indexed_ragged"),
                                          ("hindexed_bytes", "vector_float_cfg5")])
def test_mpi_pack_unpack_back_to_back_from_position_3(first, second):
    """two different derived types packed one after the other into one device buffer starting at
    position 3, then unpacked in order; the positions returned, the packed bytes, the bytes around
    them and the gaps of the unpacked canvases are all checked"""
    L = m.lib()
    b = Built(L)
    world = 0x44000000
    try:
        rng = np.random.default_rng(len(first) * 31 + len(second))
        items = []
        for name in (first, second):
            _, spec, count = BY_NAME[name]
            h = b.lib_type(spec)
            assert L.MPI_Type_commit(ctypes.byref(ctypes.c_int(h))) == 0
            t = oracle_type(spec)
            assert t.size > 0 and t.true_lb >= 0
            span = (count - 1) * t.extent + t.true_lb + t.true_extent
            src = rng.integers(0, 256, span + 16, dtype=np.uint8)
            items.append((name, h, t, count, src, tm.pack(src, t, count)))
        total = sum(len(it[5]) for it in items)
        start = 3
        d_out = m.DeviceBuffer.from_array(np.full(start + total + 13, CANARY, dtype=np.uint8))
        pos = ctypes.c_int(start)
        at = start
        for name, h, t, count, src, want in items:
            assert pos.value == at and pos.value != 0
            d_src = m.DeviceBuffer.from_array(src)
            assert L.MPI_Pack(d_src.ptr, count, h, d_out.ptr, d_out.nbytes, ctypes.byref(pos), world) == 0
            at += len(want)
            assert pos.value == at, name
        got = d_out.download(np.uint8)
        assert np.all(got[:start] == CANARY) and np.all(got[at:] == CANARY)
        at = start
        for name, h, t, count, src, want in items:
            assert np.array_equal(got[at:at + len(want)], want), name
            at += len(want)
        pos = ctypes.c_int(start)
        at = start
        for name, h, t, count, src, want in items:
            canvas = rng.integers(0, 256, len(src), dtype=np.uint8)
            d_can = m.DeviceBuffer.from_array(canvas)
            assert L.MPI_Unpack(d_out.ptr, start + total, ctypes.byref(pos), d_can.ptr, count, h, world) == 0
            at += len(want)
            assert pos.value == at, name
            assert np.array_equal(d_can.download(np.uint8), tm.unpack(want, canvas, t, count)), ("unpack", name)
    finally:
        b.close()


# ---- 8. completion word of the pack kernels ----
@pytest.mark.parametrize("grid", [5, 37, 131])
def test_pack_completion_word_counts(grid):
    """k_pack_units at a grid below 8, between 8 and 63, and of 64 or more workgroups, the last one
    partial (device_util.h block_done): the bytes are right and no completion word is missed"""
    assert (grid < 8, 8 <= grid < 64, grid >= 64) == (grid == 5, grid == 37, grid == 131)
    blk, stride = 16, 32
    nb = grid * UNITS_TILE - 7
    assert not takes_lds(blk, stride, 0) and unit_width(blk, stride) == 16
    assert -(-(nb * (blk // 16)) // UNITS_TILE) == grid
    missed = m.info("done_missed")
    strided(nb, blk, stride, 0, 0, np.random.default_rng(grid))
    assert m.info("done_missed") == missed

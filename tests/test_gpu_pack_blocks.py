"""The batched block pack / unpack (pack/pack_blocks.hip k_pack_blocks, mv2h_pack_blocks): up to 8
blocks with a layout each in one launch, against a numpy byte model.  A pack must give the model's
packed bytes exactly and leave every other byte of the staging buffer alone; an unpack runs into a
sentinel-filled buffer in which only the bytes of the blocks' type maps may change.  Each test
asserts in Python that its shape is on the branch it names (granule, workgroups per block, run
table in LDS or in global memory)."""
import numpy as np
import pytest

import mvapich2_amd as m

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
RUNS_LDS = 512  # kRunLds
TILE = 256      # kPackBlocksTile: packed units a workgroup moves per stride
E_ARG = 12


def byte_map(blk):
    """the bytes of the strided side, from its base, in pack order"""
    disp, count, extent, _poff, segs = blk
    if not count or not segs:
        return np.zeros(0, dtype=np.int64)
    one = np.concatenate([off + np.arange(ln, dtype=np.int64) for off, ln in segs])
    return (disp + extent * np.arange(count, dtype=np.int64)[:, None] + one[None, :]).ravel()


def folded_runs(segs, g):
    """runs of launch_pack_runs' folding: equal blocks at a constant distance are one run"""
    runs = []
    for off, ln in segs:
        if runs:
            blk, nrep, first, stride = runs[-1]
            last = first + (nrep - 1) * stride
            if blk == ln and (nrep == 1 or off - last == stride):
                runs[-1] = (blk, nrep + 1, first, off - last if nrep == 1 else stride)
                continue
        runs.append((ln, 1, off, 0))
    return len(runs)


def granule(base, packed, blocks):
    vals = [base, packed]
    for disp, count, extent, poff, segs in blocks:
        if count and segs:
            vals += [disp, extent, poff] + [v for s in segs for v in s]
    g = 16
    while g > 1 and any(v % g for v in vals):
        g >>= 1
    return g


def lay_out(shapes, align=16, start=0, gap=48):
    """blocks from (count, extent, segs): displacements (multiples of `align` from `start`, at least
    `gap` bytes between blocks) and 16-byte-aligned packed offsets, both running on"""
    blocks, disp, poff = [], start, 0
    for count, extent, segs in shapes:
        blocks.append((disp, count, extent, poff, segs))
        if count and segs:
            disp += (count - 1) * extent + max(o + ln for o, ln in segs) + gap
            disp += -(disp - start) % align
            poff += count * sum(ln for _, ln in segs)
            poff += -poff % 16
    return blocks, disp + 64, poff + 64


def run(blocks, span, plen, base_off=0, packed_off=0, seed=0, launches=1, global_tab=0):
    """pack and unpack `blocks` once each and check both against the byte model; returns the granule"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, span + base_off, dtype=np.uint8)
    d_src = m.DeviceBuffer.from_array(src)
    d_pk = m.DeviceBuffer.from_array(np.full(plen + packed_off, SENTINEL, dtype=np.uint8))
    assert d_src.ptr % 16 == 0 and d_pk.ptr % 16 == 0
    maps = [byte_map(b) for b in blocks]
    for b, mp in zip(blocks, maps):
        assert mp.size == 0 or (mp.min() >= 0 and mp.max() < span), "the test's own buffer is too small"
        assert b[3] + mp.size <= plen
    calls, glob, missed = m.info("pack_blocks_calls"), m.info("pack_blocks_global_tab"), m.info("done_missed")
    assert m.pack_blocks(d_src.ptr + base_off, d_pk.ptr + packed_off, blocks) == 0
    want = np.full(plen, SENTINEL, dtype=np.uint8)
    for b, mp in zip(blocks, maps):
        want[b[3]:b[3] + mp.size] = src[base_off + mp]
    got = d_pk.download(np.uint8)
    assert np.all(got[:packed_off] == SENTINEL)
    assert np.array_equal(got[packed_off:], want), "pack"
    assert np.array_equal(d_src.download(np.uint8), src), "a pack wrote its source"
    # unpack other packed bytes into a sentinel-filled buffer
    fresh = rng.integers(0, 256, plen, dtype=np.uint8)
    d_pk.upload(fresh, offset=packed_off)
    d_dst = m.DeviceBuffer.from_array(np.full(span + base_off, SENTINEL, dtype=np.uint8))
    assert m.pack_blocks(d_dst.ptr + base_off, d_pk.ptr + packed_off, blocks, unpack=True) == 0
    w2 = np.full(span + base_off, SENTINEL, dtype=np.uint8)
    for b, mp in zip(blocks, maps):
        w2[base_off + mp] = fresh[b[3]:b[3] + mp.size]
    assert np.array_equal(d_dst.download(np.uint8), w2), "unpack"
    assert m.info("pack_blocks_calls") - calls == 2 * launches
    assert m.info("pack_blocks_global_tab") - glob == 2 * global_tab
    assert m.info("done_missed") == missed
    return granule(d_src.ptr + base_off, d_pk.ptr + packed_off, blocks)


VECTOR = (3, 60, [(12 * i, 4) for i in range(5)])                 # 5 floats, every third one
INDEXED = (2, 96, [(0, 8), (24, 4), (40, 12), (72, 4)])           # irregular lengths
PAIR = (7, 8, [(0, 2), (4, 4)])                                   # a short and an int, 2 bytes of padding
CONTIG = (1, 64, [(0, 64)])
SUBARRAY = (2, 192, [((1 + r) * 32 + 8, 16) for r in range(3)])   # rows 1-3, columns 2-5 of 6 x 8 floats
EMPTY = (5, 16, [])
COUNT0 = (0, 60, [(12 * i, 4) for i in range(5)])


def test_one_block_one_run_of_16_bytes():
    blocks, span, plen = lay_out([(1, 16, [(0, 16)])])
    assert run(blocks, span, plen) == 16


def test_eight_layouts_in_one_launch():
    shapes = [VECTOR, INDEXED, PAIR, EMPTY, CONTIG, COUNT0, SUBARRAY, (4, 20, [(0, 4), (8, 6), (14, 2)])]
    blocks, span, plen = lay_out(shapes)
    assert len(blocks) == 8 and byte_map(blocks[3]).size == 0 and byte_map(blocks[5]).size == 0
    assert run(blocks, span, plen, seed=1) == 2  # the pair type's 2-byte field


@pytest.mark.parametrize("want_g,shapes,start", [
    (16, [(3, 64, [(0, 16), (32, 16)]), (2, 48, [(16, 32)])], 0),
    (4, [VECTOR, SUBARRAY], 0),
    (1, [VECTOR, SUBARRAY], 3),  # an odd displacement alone
])
def test_granules(want_g, shapes, start):
    blocks, span, plen = lay_out(shapes, start=start)
    assert all(b[0] % 16 == start and b[3] % 16 == 0 for b in blocks)
    assert run(blocks, span, plen, seed=want_g) == want_g


def test_small_block_next_to_three_tiles():
    big = (2 * TILE + 5, 32, [(0, 16)])  # 517 units of 16 bytes: 3 tiles
    blocks, span, plen = lay_out([(3, 32, [(0, 16)]), big, (1, 16, [(0, 16)])])
    rc, _wg0, nwg, grid, tile = m.pack_blocks_plan([3, 2 * TILE + 5, 1], m.info("max_grid"))
    assert rc == 0 and tile == TILE and nwg == [1, 3, 1] and grid == 5
    assert run(blocks, span, plen, seed=4) == 16


def test_one_workgroup_per_block_strides_several_tiles():
    shapes = [(5 * TILE + 7, 8, [(0, 4)]), (3 * TILE + 1, 12, [(0, 4), (8, 4)]), (2, 60, VECTOR[2])]
    blocks, span, plen = lay_out(shapes)
    units = [byte_map(b).size // 4 for b in blocks]
    before = m.info("max_grid")
    assert m.lib().mv2h_set_tuning(b"max_grid", 1) == 0
    try:
        rc, _wg0, nwg, grid, _tile = m.pack_blocks_plan(units, m.info("max_grid"))
        assert rc == 0 and nwg == [1, 1, 1] and grid == 3 and units[0] > 5 * TILE and units[1] > 6 * TILE
        assert run(blocks, span, plen, seed=5) == 4
    finally:
        assert m.lib().mv2h_set_tuning(b"max_grid", before) == 0


def test_run_table_in_global_memory_next_to_one_in_lds():
    rng = np.random.default_rng(6)
    segs, off = [], 0
    for k in range(600):  # irregular: neither two equal lengths in a row nor a constant distance
        ln = 4 * (1 + k % 3)
        segs.append((off, ln))
        off += ln + 4 * int(rng.integers(1, 4))
    assert folded_runs(segs, 4) == 600 > RUNS_LDS
    assert folded_runs(INDEXED[2], 4) == 4 and folded_runs(VECTOR[2], 4) == 1
    blocks, span, plen = lay_out([INDEXED, (3, off + 8, segs), VECTOR])
    assert run(blocks, span, plen, seed=6, global_tab=1) == 4
    # the same launch without the long block stays in LDS
    blocks, span, plen = lay_out([INDEXED, VECTOR])
    run(blocks, span, plen, seed=7, global_tab=0)


def test_pack_then_unpack_is_the_identity_on_map_bytes():
    shapes = [SUBARRAY, PAIR, (2 * TILE + 9, 24, [(4, 4), (12, 8)]), INDEXED]
    blocks, span, plen = lay_out(shapes)
    src = np.random.default_rng(8).integers(0, 256, span, dtype=np.uint8)
    d_src = m.DeviceBuffer.from_array(src)
    d_pk = m.DeviceBuffer(plen)
    d_dst = m.DeviceBuffer.from_array(np.full(span, SENTINEL, dtype=np.uint8))
    assert m.pack_blocks(d_src.ptr, d_pk.ptr, blocks) == 0
    assert m.pack_blocks(d_dst.ptr, d_pk.ptr, blocks, unpack=True) == 0
    want = np.full(span, SENTINEL, dtype=np.uint8)
    for b in blocks:
        want[byte_map(b)] = src[byte_map(b)]
    assert np.array_equal(d_dst.download(np.uint8), want)


def test_argument_errors_launch_nothing():
    src = np.random.default_rng(9).integers(0, 256, 4096, dtype=np.uint8)
    d_src, d_pk = m.DeviceBuffer.from_array(src), m.DeviceBuffer.from_array(np.full(4096, SENTINEL, dtype=np.uint8))
    calls, missed = m.info("pack_blocks_calls"), m.info("done_missed")
    ok = (0, 1, 16, 0, [(0, 16)])
    assert m.pack_blocks(d_src.ptr, d_pk.ptr, [ok] * 9) == E_ARG                       # more than kMaxRanks blocks
    assert m.pack_blocks(d_src.ptr, d_pk.ptr, [ok, (64, 1, 16, 16, [(0, 0)])]) == E_ARG   # a segment of length 0
    assert m.pack_blocks(d_src.ptr, d_pk.ptr, [ok, (64, 1, 16, 16, [(0, -4)])]) == E_ARG  # of negative length
    assert m.pack_blocks(d_src.ptr, d_pk.ptr, [ok, (64, 1, 16, 16, [(-8, 8)])]) == E_ARG  # a negative offset
    assert m.pack_blocks(d_src.ptr, d_pk.ptr, [ok, (64, 0, 16, 16, [(-8, 8)])]) == E_ARG  # even in an empty block
    # every block empty: success, and nothing launched either
    assert m.pack_blocks(d_src.ptr, d_pk.ptr, []) == 0
    assert m.pack_blocks(d_src.ptr, d_pk.ptr, [(0, 0, 16, 0, [(0, 16)]), (0, 4, 16, 0, [])]) == 0
    assert m.info("pack_blocks_calls") == calls and m.info("done_missed") == missed
    assert np.all(d_pk.download(np.uint8) == SENTINEL)
    # a negative displacement is an argument like any other: the lower bound goes into it
    assert m.pack_blocks(d_src.ptr + 64, d_pk.ptr, [(-64, 2, 32, 0, [(0, 16)])]) == 0
    assert m.info("pack_blocks_calls") == calls + 1
    got = d_pk.download(np.uint8)
    assert np.array_equal(got[:32], np.concatenate([src[0:16], src[32:48]])) and np.all(got[32:] == SENTINEL)

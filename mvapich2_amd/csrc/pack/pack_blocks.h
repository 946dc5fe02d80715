// pack_blocks.h — one launch that packs (or unpacks) up to kMaxRanks blocks, each with a flattened
// layout of its own, into (out of) one packed staging buffer: the descriptors, the partition of the
// grid over the blocks, and the host side of the launch (pack_blocks.hip).  Plain C++: the runtime
// (coll.cpp) includes it too.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../device_util.h"
#include "pack_runs.h"

namespace mv2 {

// One block, in units of the launch's granule.
struct PackBlk {
    int64_t disp;     // element 0, from the strided base (signed)
    uint64_t count;   // elements
    uint64_t ext;     // extent
    uint64_t upe;     // units per packed element
    uint64_t packed;  // first packed unit, from the packed base
    uint32_t run0, nrun;  // the block's slice of the shared run table
    uint32_t wg0, nwg;    // its workgroups [wg0, wg0 + nwg); nwg = 0: an empty block
};
struct PackBlkSet {
    PackBlk b[kMaxRanks];
};

// runs of one block staged in LDS (20 KiB): pack.hip's value for k_pack_runs, restated because that
// file keeps its own (tests/test_alltoallw_host.py holds the two together)
constexpr int kRunLds = 512;
constexpr uint64_t kPackBlocksTile = kThreads;  // packed units one workgroup moves per stride

// The partition: workgroups dealt to the n blocks in proportion to their packed units.  An empty
// block gets none, every other at least one and at most its tiles; the sum is capped by max_grid,
// which is never taken below the number of non-empty blocks nor above kDoneMaxGrid.  With the cap
// out of reach every block gets exactly its tiles.  A pure function.  Returns the grid.
inline int pack_blocks_plan(int n, const uint64_t *units, long max_grid, uint32_t *wg0, uint32_t *nwg) {
    uint64_t want[kMaxRanks], sum_want = 0;
    unsigned __int128 total = 0;
    long nonempty = 0;
    for (int b = 0; b < n; ++b) {
        want[b] = (units[b] + kPackBlocksTile - 1) / kPackBlocksTile;
        sum_want += want[b];
        total += units[b];
        nonempty += units[b] != 0;
    }
    long cap = max_grid < nonempty ? nonempty : max_grid;
    if (cap > kDoneMaxGrid) cap = kDoneMaxGrid;
    const uint64_t spare = (uint64_t)(cap - nonempty);  // what is left once every non-empty block has one
    uint32_t at = 0;
    for (int b = 0; b < n; ++b) {
        uint64_t g = want[b];
        if (sum_want > (uint64_t)cap && g) {
            const uint64_t share = 1 + (uint64_t)((unsigned __int128)spare * units[b] / total);
            if (share < g) g = share;
        }
        wg0[b] = at;
        nwg[b] = (uint32_t)g;
        at += (uint32_t)g;
    }
    return (int)at;
}

// What one launch needs, prepared on the host without touching the GPU.
struct PackBlocksJob {
    PackBlkSet set{};
    std::vector<PackRun> runs;
    int g = 16;          // the granule: bytes per unit
    int grid = 0;        // 0: every block is empty, nothing to launch
    bool global_tab = false;  // some block's run slice does not fit in LDS
};

// Block b: count[b] elements of extent[b] bytes at base + disp[b], one element = the byte segments
// [seg_first[b], seg_first[b + 1]) of offs / lens, packed at packed + packed_off[b].  E_ARG for
// nblk outside [0, kMaxRanks], a non-positive segment length or a negative segment offset.
int pack_blocks_prepare(const void *base, const void *packed, int nblk, const int64_t *disp, const size_t *count,
                        const size_t *extent, const size_t *packed_off, const int *seg_first, const int64_t *offs,
                        const int64_t *lens, long max_grid, PackBlocksJob *job);
int launch_pack_blocks(void *base, void *packed, const PackBlocksJob &job, int unpack, hipStream_t stream, Done done);

}  // namespace mv2

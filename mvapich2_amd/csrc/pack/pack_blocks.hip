// pack_blocks.hip — batched block pack / unpack: the n blocks of one side of an MPI_Alltoallw (or
// of an MPI_Alltoallv with a derived type), each with a datatype of its own, in ONE launch.
//
// The per-block route (one MPI_Pack / MPI_Unpack per block, mpi/mpi_api.cpp nblocks_pack) pays a
// launch and a wait on the completion word per block; here the block descriptors travel by value
// as a kernel argument (at most kMaxRanks, no copy to the device), the blocks' run tables are one
// shared table (pack_runs.h, folded and uploaded as launch_pack_runs does), and every block owns a
// range of workgroups sized by its share of the packed units (pack_blocks.h pack_blocks_plan).
//
// A workgroup belongs to exactly one block: it finds it by a uniform scan of the descriptors'
// wg0 from blockIdx.x, stages the block's run slice in LDS when it fits (else reads it from global
// memory), and walks its share of the block's packed units with pack_runs_units — the incremental
// (element, unit) walk of k_pack_runs, striding by the block's workgroups when those are fewer than
// its tiles.  The packed side is read / written coalesced in g-byte units, g the widest granule
// that divides everything in the launch.
#include <hip/hip_runtime.h>

#include "../coll/kernels.h"
#include "../common.h"
#include "pack_blocks.h"

namespace mv2 {

template <typename G>
__global__ __launch_bounds__(kThreads) void k_pack_blocks(G *__restrict__ strided, G *__restrict__ packed,
                                                          const PackBlkSet set,
                                                          const PackRun *__restrict__ runs, int unpack, Done done) {
    __shared__ PackRun lr[kRunLds];
    // my block: the last non-empty one whose first workgroup is not past me (uniform: scalar selects
    // over constant indices, the descriptors stay in the kernel argument segment)
    PackBlk d = set.b[0];
#pragma unroll
    for (int k = 1; k < kMaxRanks; ++k)
        if (set.b[k].nwg && blockIdx.x >= set.b[k].wg0) d = set.b[k];
    const PackRun *rt = runs + d.run0;
    const int nrun = (int)d.nrun;
    if (nrun <= kRunLds) {
        for (int k = threadIdx.x; k < nrun; k += kThreads) lr[k] = rt[k];
        __syncthreads();
        rt = lr;
    }
    const uint64_t total = d.count * d.upe;
    const uint64_t step = (uint64_t)d.nwg * kThreads;
    const uint64_t u = (uint64_t)(blockIdx.x - d.wg0) * kThreads + threadIdx.x;
    G *s = strided + d.disp, *p = packed + d.packed;
    if (u < total) {
        if (!unpack) pack_runs_units<G>(s, p, d.ext, d.upe, total, step, u, rt, nrun, 0);
        else pack_runs_units<G>(p, s, d.ext, d.upe, total, step, u, rt, nrun, 1);
    }
    block_done(done);  // completion word of a blocking call (every thread of the block arrives)
}

int pack_blocks_prepare(const void *base, const void *packed, int nblk, const int64_t *disp, const size_t *count,
                        const size_t *extent, const size_t *packed_off, const int *seg_first, const int64_t *offs,
                        const int64_t *lens, long max_grid, PackBlocksJob *job) {
    *job = PackBlocksJob{};
    if (nblk < 0 || nblk > kMaxRanks) return E_ARG;
    if (nblk == 0) return 0;
    if (!disp || !count || !extent || !packed_off || !seg_first) return E_ARG;
    if (seg_first[0] < 0) return E_ARG;
    bool live[kMaxRanks];
    bool any = false;
    uint64_t acc = 0;
    for (int b = 0; b < nblk; ++b) {
        const int s0 = seg_first[b], s1 = seg_first[b + 1];
        if (s1 < s0 || (s1 > s0 && (!offs || !lens))) return E_ARG;
        for (int s = s0; s < s1; ++s)
            if (lens[s] <= 0 || offs[s] < 0) return E_ARG;
        live[b] = count[b] != 0 && s1 > s0;
        if (!live[b]) continue;  // an empty block's numbers mean nothing
        any = true;
        acc |= (uint64_t)disp[b] | (uint64_t)extent[b] | (uint64_t)packed_off[b];
        for (int s = s0; s < s1; ++s) acc |= (uint64_t)offs[s] | (uint64_t)lens[s];
    }
    if (!any) return 0;
    acc |= (uint64_t)(uintptr_t)base | (uint64_t)(uintptr_t)packed;
    int g = 16;
    while (g > 1 && (acc % (uint64_t)g)) g >>= 1;
    job->g = g;
    uint64_t units[kMaxRanks] = {};
    for (int b = 0; b < nblk; ++b) {
        PackBlk &d = job->set.b[b];
        if (!live[b]) continue;
        d.run0 = (uint32_t)job->runs.size();
        d.upe = fold_runs(offs + seg_first[b], lens + seg_first[b], seg_first[b + 1] - seg_first[b], g, job->runs);
        d.nrun = (uint32_t)job->runs.size() - d.run0;
        d.disp = disp[b] / g;  // exact: g divides it
        d.count = count[b];
        d.ext = extent[b] / (size_t)g;
        d.packed = packed_off[b] / (size_t)g;
        units[b] = d.count * d.upe;
        job->global_tab = job->global_tab || d.nrun > (uint32_t)kRunLds;
    }
    uint32_t wg0[kMaxRanks], nwg[kMaxRanks];
    job->grid = pack_blocks_plan(nblk, units, max_grid, wg0, nwg);
    for (int b = 0; b < nblk; ++b) {
        job->set.b[b].wg0 = wg0[b];
        job->set.b[b].nwg = nwg[b];
    }
    return 0;
}

int launch_pack_blocks(void *base, void *packed, const PackBlocksJob &job, int unpack, hipStream_t stream, Done done) {
    if (job.grid <= 0) return 0;
    static RunTable tab;
    if (int rc = tab.upload(job.runs, stream)) return rc;
#define MV2_BLOCKS(G)                                                                                         \
    hipLaunchKernelGGL(k_pack_blocks<G>, dim3(job.grid), dim3(kThreads), 0, stream, (G *)base, (G *)packed, \
                       job.set, (const PackRun *)tab.d_tab, unpack, done)
    switch (job.g) {
    case 16: MV2_BLOCKS(v4u); break;
    case 8: MV2_BLOCKS(uint64_t); break;
    case 4: MV2_BLOCKS(uint32_t); break;
    case 2: MV2_BLOCKS(uint16_t); break;
    default: MV2_BLOCKS(uint8_t); break;
    }
#undef MV2_BLOCKS
    return hipGetLastError() == hipSuccess ? 0 : E_INTERN;
}

}  // namespace mv2

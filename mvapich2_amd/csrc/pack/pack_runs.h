// pack_runs.h — the run table of a flattened datatype, shared by pack.hip (k_pack_runs: one
// layout per launch) and pack_blocks.hip (k_pack_blocks: up to kMaxRanks layouts per launch).
//
// One element of a datatype is a list of RUNS in pack order, run k = nrep blocks of blk units at
// off + i*stride units (a vector is one run, an indexed type one run per block); `count` elements
// repeat every `ext` units.  In a packed element, run k starts at unit pp[k] and pp[nrun] = units
// per packed element.  The host part (the struct, the folding, the table's upload) is plain C++;
// the device part is seen by hipcc only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../common.h"

namespace mv2 {

struct PackRun {
    uint64_t pp;     // first packed unit of the run inside a packed element
    uint64_t blk;    // units per block
    uint64_t nrep;   // blocks in the run
    int64_t off;     // unit offset of block 0 inside an element
    int64_t stride;  // units between consecutive blocks
};

// Appends the runs of one element (nseg byte segments, every offset and length a multiple of g)
// to `runs`: equal-length blocks at a constant distance fold into one run.  Returns the units per
// packed element.
inline uint64_t fold_runs(const int64_t *offs, const int64_t *lens, int nseg, int g, std::vector<PackRun> &runs) {
    const size_t first = runs.size();
    uint64_t pp = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t off = offs[s] / g, len = lens[s] / g;
        if (runs.size() > first) {
            PackRun &r = runs.back();
            const int64_t last = r.off + (int64_t)(r.nrep - 1) * r.stride;
            if ((int64_t)r.blk == len && (r.nrep == 1 || off - last == r.stride)) {
                if (r.nrep == 1) r.stride = off - last;
                ++r.nrep;
                pp += (uint64_t)len;
                continue;
            }
        }
        runs.push_back(PackRun{pp, (uint64_t)len, 1, off, 0});
        pp += (uint64_t)len;
    }
    return pp;
}

// device copy of a run table: pinned staging + device buffer, grown on demand
// (every C-ABI call ends stream-synchronised, so the previous table is no longer read)
struct RunTable {
    PackRun *h_tab = nullptr, *d_tab = nullptr;
    size_t cap = 0;
    int upload(const std::vector<PackRun> &runs, hipStream_t stream) {
        const size_t nrun = runs.size();
        if (nrun > cap) {
            (void)hipStreamSynchronize(stream);
            if (h_tab) (void)hipHostFree(h_tab);
            if (d_tab) (void)hipFree(d_tab);
            h_tab = d_tab = nullptr;
            cap = 0;
            const size_t want = std::max<size_t>(64, 2 * nrun);
            if (hipHostMalloc((void **)&h_tab, want * sizeof(PackRun), hipHostMallocDefault) != hipSuccess ||
                hipMalloc((void **)&d_tab, want * sizeof(PackRun)) != hipSuccess)
                return E_NO_MEM;
            cap = want;
        }
        memcpy(h_tab, runs.data(), nrun * sizeof(PackRun));
        if (hipMemcpyAsync(d_tab, h_tab, nrun * sizeof(PackRun), hipMemcpyHostToDevice, stream) != hipSuccess)
            return E_INTERN;
        return 0;
    }
};

#ifdef __HIPCC__
__device__ __forceinline__ uint64_t udiv(uint64_t a, uint64_t b) {
    return ((a | b) >> 32) ? a / b : (uint64_t)((uint32_t)a / (uint32_t)b);
}

template <typename G>
__device__ __forceinline__ void pack_runs_units(const G *__restrict__ src, G *__restrict__ dst, uint64_t ext,
                                                uint64_t upe, uint64_t total, uint64_t step, uint64_t u,
                                                const PackRun *rt, int nrun, int unpack) {
    // (element, unit-in-element) advanced incrementally: no per-unit 64-bit division
    uint64_t e = udiv(u, upe), q = u - e * upe;
    const uint64_t se = udiv(step, upe), sq = step - se * upe;
    for (; u < total; u += step) {
        int lo = 0, hi = nrun;  // largest k with pp[k] <= q
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rt[mid].pp <= q) lo = mid;
            else hi = mid;
        }
        const PackRun r = rt[lo];
        const uint64_t w = q - r.pp;
        const uint64_t i = r.nrep > 1 ? udiv(w, r.blk) : 0;
        const int64_t su = (int64_t)(e * ext) + r.off + (int64_t)i * r.stride + (int64_t)(w - i * r.blk);
        if (!unpack) dst[u] = src[su];
        else dst[su] = src[u];
        q += sq;
        e += se;
        if (q >= upe) {
            q -= upe;
            ++e;
        }
    }
}
#endif  // __HIPCC__

}  // namespace mv2

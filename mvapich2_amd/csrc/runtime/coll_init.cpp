// coll_init.cpp — what MPI_Init runs on this node's world, before any inter-node link exists: the
// probes that choose the pipelined kernels' tiling and the one-shot threshold, and the self-test
// of the cross-GPU publish protocol.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>

#include "coll_internal.h"
#include "log.h"

namespace mv2 {

// The best wall time (us) of this node's fp32 SUM allreduce of `count` elements over `iters` calls
// after a first one that warms up, every rank starting each call together.  *rc: a call failed.
static double probe_allreduce(const void *sb, void *rb, size_t count, int iters, int *rc) {
    const int MPI_FLOAT_H = 0x4c00040a, MPI_SUM_H = 0x58000003;
    double best = 1e30;
    for (int it = 0; it < iters + 1 && !*rc; ++it) {
        host_barrier();
        const auto t0 = std::chrono::steady_clock::now();
        *rc = allreduce_entry(sb, rb, count, MPI_FLOAT_H, MPI_SUM_H, nullptr);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (it) best = std::min(best, us);
    }
    return best;
}

// The one-shot kernel pushes a rank's whole operand to every peer (n-1 times the link bytes of
// the pipelined kernel) but needs one flag exchange instead of two per round: where it stops
// paying is again a property of the links.  Probe 32 KiB .. the arena slot with both kernels
// (max over ranks) and keep the one-shot path up to the largest size it wins, scanning up.
// The path never changes a result: both kernels evaluate the call's plan.
static int oneshot_autotune() {
    World &w = world();
    // probe up to the slot (1 MiB when the node tunes, world.cpp), or to an explicit MV2AMD_ONESHOT_MAX
    const size_t top = getenv("MV2AMD_ONESHOT_MAX") ? std::min(w.oneshot_max, w.slot_bytes) : w.slot_bytes;
    void *sb = nullptr, *rb = nullptr;
    if (top < ((size_t)32 << 10) || hipMalloc(&sb, top) != hipSuccess || hipMalloc(&rb, top) != hipSuccess) {
        if (sb) hipFree(sb);
        return 0;
    }
    hipMemset(sb, 0, top);
    hipDeviceSynchronize();
    const size_t keep = w.oneshot_max;
    size_t sizes[kTuneMax / 2];
    int ns = 0;
    for (size_t b = (size_t)32 << 10; b <= top && ns < kTuneMax / 2; b <<= 1) sizes[ns++] = b;
    int rc = 0;
    for (int i = 0; i < ns && !rc; ++i) {
        for (int path = 0; path < 2 && !rc; ++path) {  // 0: one-shot, 1: pipelined
            w.oneshot_max = path ? 0 : top;  // one-shot up to the probed size, or never
            w.shm->r[w.rank].tune_us[2 * i + path] = probe_allreduce(sb, rb, sizes[i] / 4, 5, &rc);
        }
    }
    hipFree(sb);
    hipFree(rb);
    w.oneshot_max = keep;
    host_barrier();
    if (rc) return rc;
    size_t thr = 0;
    for (int i = 0; i < ns; ++i) {
        double one = 0, pipe = 0;
        for (int j = 0; j < w.size; ++j) {
            one = std::max(one, w.shm->r[j].tune_us[2 * i]);
            pipe = std::max(pipe, w.shm->r[j].tune_us[2 * i + 1]);
        }
        w.os_tune_us[i][0] = one;
        w.os_tune_us[i][1] = pipe;
    }
    for (int i = 0; i < ns && w.os_tune_us[i][0] <= w.os_tune_us[i][1]; ++i) thr = sizes[i];  // wins from the bottom
    host_barrier();
    w.os_tune_n = ns;
    if (thr) w.oneshot_max = thr;  // below 32 KiB the one-shot kernel is kept
    else w.oneshot_max = (size_t)16 << 10;
    MV2_DEBUG("one-shot autotune: one-shot up to %zu bytes", w.oneshot_max);
    return 0;
}

// Init-time choice of the pipelined kernels' tiling (workgroups x bytes per workgroup per
// round) on this node's links.  The link rate of a peer store stream and the cost of a
// round's flag exchange are properties of the machine, not of the message, so MPI_Init times
// the headline operation — a 256 MiB fp32 SUM MPI_Allreduce, which takes the ring-wrapper
// order — under a few tilings on every rank, takes each candidate's maximum over ranks through
// the host control segment, and every rank adopts the same minimum (kernels pair workgroup b
// of every rank, so the grid must agree).  The tiling never changes a result: the reduction
// order is fixed per element by the plan.  Runs with one rank per GPU (xGMI) unless
// MV2AMD_PIPE_AUTOTUNE=0, or on a shared GPU with MV2AMD_PIPE_AUTOTUNE=1; an explicit
// MV2AMD_PIPE_GRID / MV2AMD_PIPE_SUB disables it.
int pipe_autotune() {
    World &w = world();
    const char *ev = getenv("MV2AMD_PIPE_AUTOTUNE");
    const long mode = ev && *ev ? atol(ev) : -1;
    if (mode == 0 || (mode < 0 && w.nshare > 1) || w.size < 2 || getenv("MV2AMD_PIPE_GRID") ||
        getenv("MV2AMD_PIPE_SUB"))
        return 0;
    const char *eb = getenv("MV2AMD_PIPE_AUTOTUNE_BYTES");
    const size_t count = (size_t)(eb && atol(eb) > 0 ? atol(eb) : 256L << 20) / 4;
    void *sb = nullptr, *rb = nullptr;
    if (hipMalloc(&sb, count * 4) != hipSuccess || hipMalloc(&rb, count * 4) != hipSuccess) {
        if (sb) hipFree(sb);
        MV2_DEBUG("pipe autotune skipped: no device memory for the probe buffers");
        return 0;
    }
    hipMemset(sb, 0, count * 4);
    hipDeviceSynchronize();
    // tilings x the flavour of the stores into peers' arenas (non-temporal or plain: how the
    // fabric combines them is a property of the links, measured rather than assumed)
    // (256 x 16 KiB: 8 rounds of a 32 MiB segment at 8 ranks, the deepest pipeline)
    static const int kGrid[] = {256, 256, 256, 256, 128, 128, 64};
    static const size_t kSub[] = {128 << 10, 64 << 10, 32 << 10, 16 << 10, 256 << 10, 128 << 10, 512 << 10};
    constexpr int kTilings = (int)(sizeof(kGrid) / sizeof(kGrid[0]));
    const int g0 = w.pipe_grid, r0 = w.pipe_rnt;
    const size_t s0 = w.pipe_sub;
    int nc = 0;
    int rc = 0;
    // time budget (MV2AMD_PIPE_AUTOTUNE_BUDGET_MS, default 3 s of MPI_Init): rank 0 ends the
    // probe when it is spent and every rank stops at the same candidate (one barrier publishes
    // the decision, a second one keeps rank 0 from rewriting it before every rank has read it)
    const char *em = getenv("MV2AMD_PIPE_AUTOTUNE_BUDGET_MS");
    const double budget_ms = (double)(em && *em ? atol(em) : 3000);
    const auto t_begin = std::chrono::steady_clock::now();
    for (int c = 0; c < 2 * kTilings && nc < kTuneMax; ++c) {
        if (w.rank == 0)
            w.shm->tune_stop.store(
                nc > 0 && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count() >
                              budget_ms ? 1 : 0);
        host_barrier();
        const bool stop = w.shm->tune_stop.load() != 0;
        host_barrier();
        if (stop) break;
        w.pipe_grid = kGrid[c % kTilings];
        w.pipe_sub = kSub[c % kTilings];
        w.pipe_rnt = c < kTilings ? 1 : 0;
        pipe_tiling_for((count * 4 + w.size - 1) / w.size, &w.tune_grid[nc], &w.tune_sub[nc]);
        w.tune_rnt[nc] = w.pipe_rnt;
        bool dup = false;  // the grid cap of a shared GPU can fold candidates together
        for (int k = 0; k < nc; ++k)
            dup |= w.tune_grid[k] == w.tune_grid[nc] && w.tune_sub[k] == w.tune_sub[nc] && w.tune_rnt[k] == w.pipe_rnt;
        if (dup) continue;
        const double best = probe_allreduce(sb, rb, count, 3, &rc);  // the first call warms the tiling up
        if (rc) break;
        w.shm->r[w.rank].tune_us[nc] = best;
        ++nc;
    }
    hipFree(sb);
    hipFree(rb);
    host_barrier();  // every rank's timings are in the control segment
    w.pipe_grid = g0;
    w.pipe_sub = s0;
    w.pipe_rnt = r0;
    if (rc) {
        MV2_ERR("pipe autotune: probe allreduce failed");
        return rc;
    }
    int pick = 0;
    for (int k = 0; k < nc; ++k) {
        double m = 0;
        for (int j = 0; j < w.size; ++j) m = std::max(m, w.shm->r[j].tune_us[k]);
        w.tune_us[k] = m;
        if (m < w.tune_us[pick]) pick = k;
    }
    host_barrier();  // every rank has read every timing
    w.tune_n = nc;
    w.pipe_grid = w.tune_grid[pick];
    w.pipe_sub = w.tune_sub[pick];
    w.pipe_rnt = w.tune_rnt[pick];
    w.pipe_tuned = 1;
    MV2_DEBUG("pipe autotune: grid %d sub %zu %s stores (%.1f us of %d candidates)", w.pipe_grid, w.pipe_sub,
              w.pipe_rnt ? "non-temporal" : "plain", w.tune_us[pick], nc);
    return oneshot_autotune();
}

// ===========================================================================
// MPI_Init self-test of the cross-GPU publish protocol on this node's topology
// ===========================================================================

// The one-shot and pipelined kernels publish arena stores with the light release (stores
// acknowledged, no L2 writeback) and read them with the light acquire, which is right only if a
// peer-mapped uncached arena is not write-back cached by its writer -- a property of the links
// that the one-GPU box cannot show.  A rare ordering failure would not show in one call either, so
// MPI_Init runs every kernel that crosses GPUs, over both slot parities / arena halves, with a
// new operand pattern per call (an element of a stale slot never matches), and checks every
// element of every result on the device:
//   one-shot allreduce (6 sizes x 2 halves), one-shot reduce-scatter (3 x 2), pipelined allreduce
//   (ring order, 4 MiB, x 4; butterfly order x 2; ring + remainder), a multi-round pipelined
//   allreduce (small rounds: both parities inside one call) x 2, pipelined reduce-scatter,
//   allgather and broadcast x 2 each, one-shot allgather and broadcast x 2 each, and, with the
//   graph lane, a captured one-shot and a captured pipelined allreduce replayed 3 times each (its
//   own arenas and device sequence); a one-shot and a pipelined scan (counted apart).
// The per-call mismatch counts are read once at the end; the verdict is agreed through the
// host control segment.  On a mismatch every rank falls back to the full system-scope release
// and runs the whole set again; a second failure fails MPI_Init instead of returning wrong
// sums later.  (Protocol contract: device_util.h:1-13.)
int coll_selftest() {
    World &w = world();
    const int n = w.size, me = w.rank;
    const int MPI_INT_H = 0x4c000405, MPI_SUM_H = 0x58000003;
    // elements per buffer: the largest checked call (1 Mi + 3 elements, a 1 Mi-element allgather
    // result) and the graph lane's second capture, which runs 8192 elements into the buffers
    constexpr size_t kGraphOff = 8192;
    const size_t cap = kGraphOff + ((size_t)1 << 20) + 64;
    constexpr int kMaxCalls = 96;
    uint32_t *sb = nullptr, *rb = nullptr, *bad = nullptr;
    if (hipMalloc((void **)&sb, cap * 4) != hipSuccess || hipMalloc((void **)&rb, cap * 4) != hipSuccess ||
        hipMalloc((void **)&bad, kMaxCalls * 4) != hipSuccess) {
        MV2_ERR("self-test: device allocation failed");
        if (sb) hipFree(sb);
        if (rb) hipFree(rb);
        return E_NO_MEM;
    }
    hipStream_t st = w.stream;
    const char *what[kMaxCalls] = {};
    int verdict = 0, calls = 0, scan_calls = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        hipMemsetAsync(bad, 0, kMaxCalls * 4, st);
        int rc = 0;
        calls = 0;
        auto seed_of = [&](int k) { return (uint32_t)(0x51ed270bu * (uint32_t)(k + 1) + 0x1000193u * (uint32_t)attempt); };
        // one checked call: fill this rank's operand, run the call, check its result on the device
        // every operand and result stays inside its buffer (the graph lane's second
        // capture once ran 8 K elements past the end)
        auto fits = [&](const uint32_t *p, size_t c) {
            const uint32_t *b = (p >= rb && p < rb + cap) ? rb : sb;
            if (p < b || (size_t)(p - b) + c > cap || calls + scan_calls > kMaxCalls) {
                MV2_ERR("self-test: call %d does not fit its buffers (%zu elements at +%td of %zu)", calls, c, p - b, cap);
                if (!rc) rc = E_INTERN;
                return false;
            }
            return true;
        };
        auto fill = [&](uint32_t *p, size_t c, int k, int as_rank) {
            if (!rc && fits(p, c)) rc = launch_selftest_fill(p, c, seed_of(k), as_rank, st);
        };
        auto check = [&](const uint32_t *p, size_t c, int k, int mode, int arg, uint64_t base, const char *name) {
            if (!rc && fits(p, c)) rc = launch_selftest_check(p, c, seed_of(k), n, mode, arg, base, bad + k, st);
            what[k] = name;
        };
        // one-shot allreduce: sizes up to the one-shot limit, each on both arena halves
        const size_t os_max = std::min(w.oneshot_max, w.slot_bytes) / 4;
        const size_t os_sizes[6] = {2, 1027, 4096, 16389, os_max > 3 ? os_max - 3 : 1, os_max};
        for (int i = 0; i < 6 && !rc; ++i)
            for (int h = 0; h < 2 && !rc; ++h) {
                const int k = calls++;
                const size_t c = std::max<size_t>(1, std::min(os_sizes[i], cap));
                fill(sb, c, k, me);
                if (!rc) rc = allreduce_entry(sb, rb, c, MPI_INT_H, MPI_SUM_H, nullptr);
                check(rb, c, k, 0, 0, 0, "one-shot allreduce");
            }
        // one-shot reduce-scatter below the ring threshold: 12-byte blocks (element by element),
        // blocks of 16-byte multiples
        const size_t rs_small[3] = {3, 1024, 2048};
        for (int i = 0; i < 3 && !rc; ++i)
            for (int h = 0; h < 2 && !rc; ++h) {
                const int k = calls++;
                const size_t c = rs_small[i];
                size_t counts[kMaxRanks];
                for (int j = 0; j < n; ++j) counts[j] = c;
                fill(sb, c * n, k, me);
                if (!rc) rc = reduce_scatter_entry(sb, rb, counts, MPI_INT_H, MPI_SUM_H, nullptr);
                check(rb, c, k, 0, 0, (uint64_t)me * c, "one-shot reduce-scatter");
            }
        // pipelined allreduce: ring order (4 MiB) on both slot parities twice, the butterfly
        // (pt2pt_rs, 1 MiB + 5), the ring with a remainder (4 MiB + 3)
        const size_t pa_sizes[7] = {(size_t)1 << 20, (size_t)1 << 20, (size_t)1 << 20, (size_t)1 << 20,
                                    ((size_t)1 << 18) + 5, ((size_t)1 << 18) + 5, ((size_t)1 << 20) + 3};
        for (int i = 0; i < 7 && !rc; ++i) {
            const int k = calls++;
            fill(sb, pa_sizes[i], k, me);
            if (!rc) rc = allreduce_entry(sb, rb, pa_sizes[i], MPI_INT_H, MPI_SUM_H, nullptr);
            check(rb, pa_sizes[i], k, 0, 0, 0, "pipelined allreduce");
        }
        // multi-round pipelined allreduce: small rounds, so one call alternates slot parities
        {
            const int g0 = w.pipe_grid;
            const size_t s0 = w.pipe_sub;
            w.pipe_grid = std::min(g0, 32);
            w.pipe_sub = 4096;
            for (int i = 0; i < 2 && !rc; ++i) {
                const int k = calls++;
                const size_t c = ((size_t)1 << 20) - 7 * (size_t)i;
                fill(sb, c, k, me);
                if (!rc) rc = allreduce_entry(sb, rb, c, MPI_INT_H, MPI_SUM_H, nullptr);
                check(rb, c, k, 0, 0, 0, "multi-round pipelined allreduce");
            }
            w.pipe_grid = g0;
            w.pipe_sub = s0;
        }
        // pipelined reduce-scatter (ring, 4 MiB in all), allgather, broadcast
        for (int i = 0; i < 2 && !rc; ++i) {
            const int k = calls++;
            const size_t c = ((size_t)1 << 20) / (size_t)n;
            size_t counts[kMaxRanks];
            for (int j = 0; j < n; ++j) counts[j] = c;
            fill(sb, c * n, k, me);
            if (!rc) rc = reduce_scatter_entry(sb, rb, counts, MPI_INT_H, MPI_SUM_H, nullptr);
            check(rb, c, k, 0, 0, (uint64_t)me * c, "pipelined reduce-scatter");
        }
        // the pipelined allgather and broadcast below run with the one-shot path off: with a 1 MiB
        // slot their blocks would otherwise fit the one-shot kernel, and the pipelined kernel's
        // cross-GPU publish would go unchecked
        const size_t os_keep = w.oneshot_max;
        w.oneshot_max = 0;
        for (int i = 0; i < 2 && !rc; ++i) {
            const int k = calls++;
            const size_t c = ((size_t)1 << 20) / (size_t)n - 4 * (size_t)i;
            fill(sb, c, k, me);
            if (!rc) rc = allgather_node(sb, rb, c * 4, nullptr);
            check(rb, c * n, k, 2, (int)c, 0, "pipelined allgather");
        }
        w.oneshot_max = os_keep;
        // one-shot allgather and broadcast (k_oneshot_mv): a 12-byte block (byte by byte) and 16-byte
        // blocks, and a broadcast with a tail
        const size_t os_ag[2] = {3, 4096}, os_bc[2] = {3, 16387};
        for (int i = 0; i < 2 && !rc; ++i) {
            const int k = calls++;
            fill(sb, os_ag[i], k, me);
            if (!rc) rc = allgather_node(sb, rb, os_ag[i] * 4, nullptr);
            check(rb, os_ag[i] * n, k, 2, (int)os_ag[i], 0, "one-shot allgather");
        }
        for (int i = 0; i < 2 && !rc; ++i) {
            const int k = calls++;
            const int root = i == 0 ? n - 1 : 0;
            if (me == root) fill(rb, os_bc[i], k, root);
            else if (!rc) rc = hipMemsetAsync(rb, 0x5A, os_bc[i] * 4, st) == hipSuccess ? 0 : E_INTERN;
            if (!rc) rc = bcast_node(rb, os_bc[i] * 4, root, nullptr);
            check(rb, os_bc[i], k, 1, root, 0, "one-shot broadcast");
        }
        w.oneshot_max = 0;
        for (int i = 0; i < 2 && !rc; ++i) {
            const int k = calls++;
            const int root = i == 0 ? 0 : n - 1;
            const size_t c = ((size_t)1 << 18) + 3 * (size_t)i;
            if (me == root) fill(rb, c, k, root);
            else if (!rc) rc = hipMemsetAsync(rb, 0xA5, c * 4, st) == hipSuccess ? 0 : E_INTERN;
            if (!rc) rc = bcast_node(rb, c * 4, root, nullptr);
            check(rb, c, k, 1, root, 0, "pipelined broadcast");
        }
        w.oneshot_max = os_keep;
        // scan: one small (one-shot) and one pipelined MPI_Scan; rank me's element is the sum over
        // ranks 0 .. me.  Counted apart (selftest_scan_calls), their mismatch words taken from the
        // top of `bad`
        {
            const size_t sc_sizes[2] = {1027, ((size_t)1 << 18) + 5};
            scan_calls = 0;
            for (int i = 0; i < 2 && !rc; ++i) {
                const int k = kMaxCalls - 1 - scan_calls++;
                if (i == 1) w.oneshot_max = 0;
                fill(sb, sc_sizes[i], k, me);
                if (!rc) rc = scan_entry(sb, rb, sc_sizes[i], MPI_INT_H, MPI_SUM_H, nullptr, false);
                if (!rc && fits(rb, sc_sizes[i]))
                    rc = launch_selftest_check(rb, sc_sizes[i], seed_of(k), me + 1, 0, 0, 0, bad + k, st);
                what[k] = i ? "pipelined scan" : "one-shot scan";
            }
            w.oneshot_max = os_keep;
        }
        // graph lane: a captured one-shot and a captured pipelined allreduce, replayed
        if (w.graph_lane && !rc) {
            hipStream_t cs = nullptr;
            const size_t gc[2] = {4096, (((size_t)1 << 20) / (16 * (size_t)n)) * 16 * (size_t)n};
            for (int g = 0; g < 2; ++g) fits(sb + (size_t)g * kGraphOff, gc[g]), fits(rb + (size_t)g * kGraphOff, gc[g]);
            hipGraph_t graph[2] = {};
            hipGraphExec_t ex[2] = {};
            if (hipStreamCreate(&cs) != hipSuccess) rc = E_INTERN;
            for (int g = 0; g < 2 && !rc; ++g) {
                if (hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed) != hipSuccess) {
                    rc = E_INTERN;
                    break;
                }
                int crc;
                {
                    EnqueueScope q(true);
                    crc = allreduce_entry(sb + (size_t)g * kGraphOff, rb + (size_t)g * kGraphOff, gc[g], MPI_INT_H, MPI_SUM_H, cs);
                }
                if (hipStreamEndCapture(cs, &graph[g]) != hipSuccess || crc ||
                    hipGraphInstantiate(&ex[g], graph[g], nullptr, nullptr, 0) != hipSuccess)
                    rc = crc ? crc : E_INTERN;
            }
            hipStreamSynchronize(st);  // the blocking calls above are done before the replays
            for (int rep = 0; rep < 3 && !rc; ++rep)
                for (int g = 0; g < 2 && !rc; ++g) {
                    const int k = calls++;
                    if (!fits(sb + (size_t)g * kGraphOff, gc[g]) ||
                        (rc = launch_selftest_fill(sb + (size_t)g * kGraphOff, gc[g], seed_of(k), me, cs)))
                        break;
                    if (hipGraphLaunch(ex[g], cs) != hipSuccess) rc = E_INTERN;
                    if (!rc) rc = launch_selftest_check(rb + (size_t)g * kGraphOff, gc[g], seed_of(k), n, 0, 0, 0, bad + k, cs);
                    what[k] = "graph-lane allreduce";
                }
            if (cs && hipStreamSynchronize(cs) != hipSuccess) rc = rc ? rc : E_INTERN;
            if (!rc && check_err_word()) rc = E_OTHER;
            for (int g = 0; g < 2; ++g) {
                if (ex[g]) hipGraphExecDestroy(ex[g]);
                if (graph[g]) hipGraphDestroy(graph[g]);
            }
            if (cs) hipStreamDestroy(cs);
        }
        uint32_t hb[kMaxCalls] = {};
        if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(hb, bad, sizeof(hb), hipMemcpyDeviceToHost) != hipSuccess)
            rc = rc ? rc : E_INTERN;
        int ok = rc == 0;
        for (int k = 0; k < kMaxCalls && ok; ++k)
            if ((k < calls || k >= kMaxCalls - scan_calls) && hb[k]) {
                MV2_ERR("self-test (%s release): call %d (%s) returned %u wrong elements",
                        w.light_release ? "light" : "full", k, what[k] ? what[k] : "?", hb[k]);
                ok = 0;
            }
        if (rc) MV2_ERR("self-test: a call failed (MPI error class %d)", rc);
        // 1 = every element right, 0 = wrong elements, -1 = a call or launch failed; the retry below
        // is decided from these agreed values, never from this rank's own rc (a rank that stopped
        // while its peers ran the set again would leave them waiting for it)
        w.shm->r[me].selftest_ok = rc ? -1 : ok;
        host_barrier();
        int all_ok = 1, any_err = 0;
        for (int j = 0; j < n; ++j) {
            all_ok &= w.shm->r[j].selftest_ok == 1;
            any_err |= w.shm->r[j].selftest_ok < 0;
        }
        host_barrier();  // every rank has read every verdict
        if (all_ok) {
            verdict = 0;
            MV2_DEBUG("self-test passed: %d calls (light_release=%d)", calls, w.light_release);
            break;
        }
        verdict = E_INTERN;
        if (w.light_release && !any_err) {
            if (me == 0)
                fprintf(stderr, "[mv2amd] warning: device collective self-test failed with the light release; "
                                "using the full system-scope release\n");
            w.light_release = 0;
        } else {
            break;
        }
    }
    w.selftest_calls = calls;
    w.selftest_scan_calls = scan_calls;
    hipFree(sb);
    hipFree(rb);
    hipFree(bad);
    if (verdict) MV2_ERR("device collective self-test failed at MPI_Init (ranks %d): cross-GPU protocol broken", n);
    return verdict;
}

}  // namespace mv2

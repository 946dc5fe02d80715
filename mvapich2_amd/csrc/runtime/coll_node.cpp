// coll_node.cpp — host orchestration of the device collectives over this node's ranks.
//
// Every reducing call first takes the reference's one-node algorithm choice
// (orders.cpp plan_allreduce / plan_reduce / plan_reduce_scatter, restating
// MPIR_Allreduce_index_tuned_intra_MV2 allreduce_osu.c:3015-3420,
// MPIR_Reduce_index_tuned_intra_MV2 reduce_osu.c:2391-2660 and
// MPIR_Reduce_scatter_MV2 red_scat_osu.c:1859-1896) and then runs that
// algorithm's operand order on the device (specialised LINEAR / ring /
// butterfly evaluators, or per-element programs).  The data path is
// MI355X-native: one-shot push through uncached IPC arenas for small messages,
// pipelined direct reduce-scatter + all-gather pushed into peers' arenas over
// xGMI for large ones (coll/pipe.h), tiled by the MPI_Init autotune.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>

#include "../../../include/mv2h.h"
#include "coll_internal.h"
#include "log.h"
#include "pvars.h"

namespace mv2 {

// ---------------------------------------------------------------------------
// reduction order (algorithm choice and programs: orders.cpp)
// ---------------------------------------------------------------------------
TreeParams tree_base(int n) {
    TreeParams tp{};
    int pof2 = 1, lg = 0;
    while (pof2 * 2 <= n) { pof2 *= 2; ++lg; }
    tp.pof2 = pof2;
    tp.lg = lg;
    tp.rem = n - pof2;
    return tp;
}

// pt2pt_rs order on the specialised butterfly evaluator: recursive halving
// with owner bitrev(block), or recursive doubling (count < pof2, or the
// pt2pt_rd algorithm) where each rank keeps its own result and even ranks
// below 2*rem take their odd partner's (allreduce_osu.c:585-600, :1003-1030)
static TreeParams tree_rs(int n, size_t count, int me, bool force_rd) {
    TreeParams tp = tree_base(n);
    tp.linear = 0;
    if (!force_rd && count >= (size_t)tp.pof2) {
        tp.owner_fixed = -1;
        tp.rs_blk = count / tp.pof2;
    } else {
        int r = me;
        if (r < 2 * tp.rem && r % 2 == 0) r = r + 1;
        tp.owner_fixed = (r < 2 * tp.rem) ? r / 2 : r - tp.rem;
    }
    return tp;
}

// A program set whose every program is acc = ((x0 . x1) . x2) ... (the degree-4 tree over one
// group of <= 4 ranks, and any other algorithm that reduces to it) runs on the specialised
// LINEAR evaluator instead of the program kernel: same operands in the same order.
static bool progs_are_linear(const ProgSet &ps, int n) {
    if (ps.nprog < 1) return false;
    for (int k = 0; k < ps.nprog; ++k) {
        const Prog &q = ps.p[k];
        if (q.nsteps != n - 1 || q.res != 0) return false;
        for (int s = 0; s < n - 1; ++s)
            if (q.dst[s] != 0 || q.src[s] != s + 1) return false;
    }
    return true;
}

// The two-level degree-d tree (d < n) as a program: each group leader g reduces g+1 .. g+d-1,
// then rank 0 reduces the leaders d, 2d, ... in order.  Returns d when `ps` is that program.
static int progs_grouped(const ProgSet &ps, int n) {
    if (ps.nprog != 1) return 0;
    const Prog &q = ps.p[0];
    for (int d = 2; d < n; ++d) {
        uint8_t dst[kMaxRanks], src[kMaxRanks];
        int k = 0;
        for (int g = 0; g < n; g += d)
            for (int m = g + 1; m < g + d && m < n; ++m) dst[k] = (uint8_t)g, src[k++] = (uint8_t)m;
        for (int g = d; g < n; g += d) dst[k] = 0, src[k++] = (uint8_t)g;
        if (k != q.nsteps || q.res != 0) continue;
        bool same = true;
        for (int s = 0; s < k && same; ++s) same = q.dst[s] == dst[s] && q.src[s] == src[s];
        if (same) return d;
    }
    return 0;
}

static TreeParams tree_from_plan(const Plan &p, int n, size_t count, int me) {
    if (p.algo != ALG_PT2PT_RS && p.algo != ALG_PT2PT_RD && p.algo != ALG_SHMEM_LINEAR && progs_are_linear(p.ps, n)) {
        TreeParams tp = tree_base(n);
        tp.linear = 1;
        return tp;
    }
    switch (p.algo) {
    case ALG_PT2PT_RS: return tree_rs(n, count, me, false);
    case ALG_PT2PT_RD: return tree_rs(n, count, me, true);
    case ALG_SHMEM_LINEAR:
        if (!p.inner) {
            TreeParams tp = tree_base(n);
            tp.linear = 1;
            return tp;
        }
        [[fallthrough]];  // reduce_shmem from the shmem slot on: the inner reduce's programs
    default: {
        TreeParams tp = tree_base(n);
        tp.linear = 4;
        tp.ps = p.ps;
        return tp;
    }
    }
}

void log_plan(const char *coll, const Plan &p, size_t count) {
    MV2_DEBUG("%s count %zu -> %s%s%s", coll, count, algo_name(p.algo), p.inner ? " / " : "",
              p.inner ? algo_name(p.inner) : "");
}

int grid_cap() {
    World &w = world();
    int g = w.max_grid / (w.nshare > 0 ? w.nshare : 1);
    if (g < 1) g = 1;
    if (g > kMaxBlocks) g = kMaxBlocks;
    return g;
}

// launch config of a collective kernel: identical on every rank (the grid
// must match across ranks: workgroup b of each rank pairs with workgroup b)
LaunchCfg coll_cfg(int grid, hipStream_t st) {
    World &w = world();
    LaunchCfg c{grid, 2, st};
    c.cus = w.cus;
    c.nshare = w.nshare;
    return c;
}

static long env_long_coll(const char *name, long dflt) {
    const char *v = getenv(name);
    return v && *v ? atol(v) : dflt;
}
// constants chosen on one shared GPU (not probed at MPI_Init), read once
long ar_scalar_max() { static const long v = env_long_coll("MV2AMD_AR_SCALAR_MAX", 1024); return v; }
long rs_scalar_max() { static const long v = env_long_coll("MV2AMD_RS_SCALAR_MAX", 4096); return v; }

// ---------------------------------------------------------------------------
// pipelined collectives (coll/pipe.h)
// ---------------------------------------------------------------------------
// Grid and per-block range of a pipelined call.  A pure function of the
// message geometry and of values every rank shares (CU count, ranks per GPU,
// tuning knobs), so block b of every rank handles the same bytes.
PipeGeom pipe_geom(size_t maxlen) {
    World &w = world();
    int cap = std::min(kPipeMaxGrid, xcd_fair_cap(1, w.cus, w.nshare));  // k_pipe: one block per CU
    cap = std::min(cap, std::max(1, w.pipe_grid));
    // the smallest per-workgroup tile: 4 KiB (measured against 8 and 16 KiB: a small message
    // spread over more workgroups leaves each thread fewer dependent memory round trips per
    // phase; 1 MiB at 4 shared ranks 37.1 -> 28.7 us).  MV2AMD_PIPE_MIN_SUB overrides it.
    static const size_t kMinSub = (size_t)std::max(4096L, env_long_coll("MV2AMD_PIPE_MIN_SUB", 4096)) & ~(size_t)4095;
    PipeGeom g{};
    g.grid = (int)std::min<size_t>((size_t)cap, std::max<size_t>(1, (maxlen + kMinSub - 1) / kMinSub));
    size_t tsub = (maxlen + g.grid - 1) / g.grid;
    tsub = (tsub + 4095) & ~(size_t)4095;
    // a round's slot (grid x tsub) must fit the kPipeSlot bytes of an arena slot
    const size_t sub_cap = std::min(kPipeSlot / (size_t)g.grid, std::max<size_t>(4096, w.pipe_sub));
    g.tsub = std::min(tsub, sub_cap & ~(size_t)4095);
    g.tseg = (size_t)g.grid * g.tsub;
    g.nrounds = (int)((maxlen + g.tseg - 1) / g.tseg);
    return g;
}

// the tiling a segment of seg_bytes runs with (MPI_Init's report)
void pipe_tiling_for(size_t seg_bytes, int *grid, size_t *tsub) {
    const PipeGeom g = pipe_geom(seg_bytes);
    *grid = g.grid;
    *tsub = g.tsub;
}

// n contiguous 16-byte-aligned segments of a `bytes` buffer (the last may be short or empty)
static void even_segments(PipeArgs &a, size_t bytes, int n) {
    const size_t seg = (((bytes + n - 1) / n) + 15) & ~(size_t)15;
    for (int j = 0; j < n; ++j) {
        const size_t off = std::min((size_t)j * seg, bytes);
        a.seg_off[j] = a.recv_off[j] = off;
        a.seg_len[j] = std::min(seg, bytes - off);
    }
}

// Fill the runtime part of `a`, reserve rounds/epochs (pipe_reserve) and launch (no sync).
// dt == nullptr: data-movement modes (AG / BC).
static int run_pipe(PipeArgs &a, int oi, const DtypeInfo *dt, hipStream_t st) {
    World &w = world();
    a.n = w.size;
    a.me = w.rank;
    size_t maxlen = 0;
    for (int j = 0; j < a.n; ++j) maxlen = std::max(maxlen, a.seg_len[j]);
    if (maxlen == 0) return 0;  // every rank sees the same geometry
    const PipeGeom g = pipe_geom(maxlen);
    a.rs_peer = w.graph ? w.g_peer_rs : w.peer_rs;
    pipe_reserve(a, g, st);
    MV2_DEBUG("pipe mode %d grid %d tsub %zu rounds %d maxlen %zu", a.mode, g.grid, g.tsub, g.nrounds, maxlen);
    LaunchCfg cfg = coll_cfg(g.grid, st);
    tmark0(st);
    const int rc = dt ? launch_pipe_reduce(oi, dt->kind, a, cfg) : launch_pipe_copy(a, cfg);
    tmark1(st);
    return rc;
}

// The one-shot kernels' per-call part (oneshot_reserve) and the ranks.
static void oneshot_common(OneShotArgs &a, hipStream_t st) {
    a.n = world().size;
    a.me = world().rank;
    oneshot_reserve(a, a.epoch, st);
}

// one 16-B vector per thread of a 256-thread workgroup, up to 64 workgroups (256 KiB): the
// one-shot kernels are latency-bound, and each further vector a thread owns costs it another
// dependent memory round trip (MV2AMD_ONESHOT_VECS_PER_WG / _MAX_WG override)
int oneshot_grid(size_t nvec, int gcap) {
    static const long vpw = std::max(64L, env_long_coll("MV2AMD_ONESHOT_VECS_PER_WG", 256));
    static const int wmax = (int)std::min(1024L, std::max(1L, env_long_coll("MV2AMD_ONESHOT_MAX_WG", 64)));
    const int g = (int)((nvec + vpw - 1) / vpw);
    return std::max(1, std::min(g, std::min(gcap, wmax)));
}

// Launch the one-shot kernel of `a` (after oneshot_common) on the grid of nvec vectors.
// dt == nullptr: the data-movement kernel (allgather / broadcast).
static int oneshot_launch(const OneShotArgs &a, size_t nvec, int oi, const DtypeInfo *dt, hipStream_t st) {
    LaunchCfg cfg = coll_cfg(oneshot_grid(nvec, grid_cap()), st);
    tmark0(st);
    const int rc = dt ? launch_oneshot(oi, dt->kind, a, dt->extent, cfg) : launch_oneshot_mv(a, cfg);
    tmark1(st);
    return rc;
}

// ---------------------------------------------------------------------------
// the collectives
// ---------------------------------------------------------------------------
int require_world() {
    World &w = world();
    if (!w.inited) {
        MV2_ERR("collective called before MPI_Init");
        return E_OTHER;
    }
    if (w.size > kMaxRanks) {
        MV2_ERR("device collectives support up to %d ranks per node (have %d)", kMaxRanks, w.size);
        return E_UNSUPPORTED;
    }
    return 0;
}

// staging: host or misaligned buffers go through device scratch (GPU does the work)
struct Staged {
    const char *send;
    char *recv;
    bool copy_back;
    void *user_recv;
    size_t bytes;
};

// Device staging space of a call.  A captured call (graph lane) cannot use the shared scratch
// buffers — a graph keeps their addresses for every replay while later calls regrow or reuse
// them — so it takes a private piece of a pool that lives until MPI_Finalize.
void *call_scratch(int idx, size_t bytes) {
    World &w = world();
    if (!w.graph) return get_scratch(idx, bytes);
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (!w.g_pool || w.g_pool_used + need > w.g_pool_bytes) {
        MV2_ERR("graph lane: staging pool exhausted (%zu bytes)", w.g_pool_bytes);
        return nullptr;
    }
    void *p = w.g_pool + w.g_pool_used;
    w.g_pool_used += need;
    return p;
}

// An operand the kernels can read: `p` itself when it is device memory with p % 16 == mis, else
// a copy of its `bytes` in scratch block idx at that misalignment (nullptr: no memory).
static const char *device_operand(const void *p, size_t bytes, size_t mis, int idx, hipStream_t st) {
    if (is_device(p) && (uintptr_t)p % 16 == mis) return (const char *)p;
    char *t = (char *)call_scratch(idx, bytes + mis);
    if (!t) return nullptr;
    hipMemcpyAsync(t + mis, p, bytes, hipMemcpyDefault, st);
    return t + mis;
}

static int stage_in(const void *send, void *recv, size_t sbytes, size_t rbytes, bool in_place, hipStream_t st,
                    Staged &s) {
    s.copy_back = false;
    s.user_recv = recv;
    s.bytes = rbytes;
    const bool recv_ok = is_device(recv) && ((uintptr_t)recv % 16 == 0);
    beacon(BC_STAGE);
    if (recv_ok) {
        s.recv = (char *)recv;
    } else {
        s.recv = (char *)call_scratch(1, rbytes);
        if (!s.recv) return E_NO_MEM;
        s.copy_back = true;
        if (in_place) hipMemcpyAsync(s.recv, recv, rbytes, hipMemcpyDefault, st);
    }
    s.send = in_place ? s.recv : device_operand(send, sbytes, 0, 0, st);
    return s.send ? 0 : E_NO_MEM;
}

// the staged result copied back to the caller's buffer; E_INTERN when the copy cannot be
// enqueued (the call must then fail rather than return with the result never delivered)
static int stage_out(const Staged &s, hipStream_t st) {
    if (s.copy_back && enq_copy_last(s.user_recv, s.recv, s.bytes, st) != hipSuccess) return E_INTERN;
    return 0;
}

// One allreduce over `count` elements in the order `tp` (ring = true: the flat
// ring's chunking, segment j = ring chunk j; count is a multiple of n).
static int allreduce_impl(const void *sendbuf, void *recvbuf, size_t count, const DtypeInfo *dt, int oi,
                          hipStream_t st, const TreeParams &tp_in, bool ring = false) {
    World &w = world();
    const size_t bytes = count * (size_t)dt->extent;
    const bool in_place = sendbuf == (const void *)-1 || sendbuf == recvbuf;
    Staged s;
    int rc = stage_in(sendbuf, recvbuf, bytes, bytes, in_place, st, s);
    if (rc) return rc;
    const int n = w.size;
    if (n == 1 || oi == OP_NO_OP) {
        if (!in_place && oi != OP_NO_OP) hipMemcpyAsync(s.recv, s.send, bytes, hipMemcpyDeviceToDevice, st);
        if ((rc = stage_out(s, st))) return rc;
        return finish(st, false);
    }
    if (oi == OP_REPLACE) {
        // result of REPLACE over ranks 0..n-1 in rank order: rank n-1's data; take the two-level
        // linear chain semantics: recv = x_{n-1} everywhere.  Realised as a broadcast from n-1.
        if (!in_place) hipMemcpyAsync(s.recv, s.send, bytes, hipMemcpyDeviceToDevice, st);
        if ((rc = stage_out(s, st))) return rc;
        rc = finish(st, false);
        if (rc) return rc;
        return mv2h_bcast(recvbuf, bytes, n - 1, nullptr);
    }
    TreeParams tp = tp_in;
    if (!ring && bytes <= w.oneshot_max && bytes <= w.slot_bytes) {
        // the degree-d tree (the default small-message order at 6-8 ranks) on its own evaluator
        if (tp.linear == 4) {
            const int d = progs_grouped(tp.ps, n);
            if (d) {
                tp.linear = 5;
                tp.pof2 = d;
            }
        }
        OneShotArgs a{};
        oneshot_common(a, st);
        a.send = s.send;
        a.recv = s.recv;
        a.count = count;
        // small operands element by element in one workgroup, on the compact kernel whose code
        // holds no vector phases (kernels_impl.h LOneShot: 8 B launch -> completion 8.8 -> 7.8 us
        // at 2 shared ranks, profiles/r05az; the general kernel's element-wise body measured no
        // faster than its vector body, r05z)
        a.nvec = bytes <= (size_t)ar_scalar_max() ? 0 : bytes / 16;
        a.tp = tp;
        if ((rc = oneshot_launch(a, a.nvec, oi, dt, st))) return rc;
        if ((rc = stage_out(s, st))) return rc;
        return finish(st, w.timing);
    }
    // pipelined direct reduce-scatter + all-gather, pushed through the arenas
    PipeArgs a{};
    a.mode = PIPE_AR;
    a.send = s.send;
    a.recv = s.recv;
    a.esize = dt->extent;
    if (ring) {
        // segment j = ring chunk j.  Chunks that are not 16-byte multiples keep their
        // misalignment through the arena slots (coll/pipe.h: scalar head, aligned body);
        // only operands whose base is not 16-byte aligned go through padded copies
        tp.linear = 3;
        const size_t cb = (count / n) * (size_t)dt->extent;
        if (cb % 16 == 0 || ((uintptr_t)s.send % 16 == 0 && (uintptr_t)s.recv % 16 == 0)) {
            for (int j = 0; j < n; ++j) {
                a.seg_off[j] = a.recv_off[j] = (size_t)j * cb;
                a.seg_len[j] = cb;
            }
        } else {
            const size_t pcb = (cb + 15) & ~(size_t)15;
            char *ps = (char *)call_scratch(3, pcb * n), *pr = (char *)call_scratch(4, pcb * n);
            if (!ps || !pr) return E_NO_MEM;
            if (hipMemcpy2DAsync(ps, pcb, s.send, cb, cb, n, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return E_INTERN;
            for (int j = 0; j < n; ++j) {
                a.seg_off[j] = a.recv_off[j] = (size_t)j * pcb;
                a.seg_len[j] = cb;
            }
            a.send = ps;
            a.recv = pr;
            a.tp = tp;
            if ((rc = run_pipe(a, oi, dt, st))) return rc;
            if (hipMemcpy2DAsync(s.recv, cb, pr, pcb, cb, n, hipMemcpyDeviceToDevice, st) != hipSuccess)
                return E_INTERN;
            world().pending = 0;
            if ((rc = stage_out(s, st))) return rc;
            return finish(st, w.timing);
        }
    } else {
        even_segments(a, bytes, n);
    }
    a.tp = tp;
    if ((rc = run_pipe(a, oi, dt, st))) return rc;
    if ((rc = stage_out(s, st))) return rc;
    return finish(st, w.timing);
}

// MPIR_Allreduce_index_tuned_intra_MV2's one-node choice (orders.cpp
// plan_allreduce).  The ring wrapper (allreduce_osu.c:3758-3818) runs the
// ring over the first (count/n)*n elements and pt2pt_rs over the remainder;
// with MPI_IN_PLACE the ring body itself falls back to pt2pt_rs (:4095-4100),
// still over the two ranges separately; count < n leaves the ring nothing.
static int allreduce_select(const void *sendbuf, void *recvbuf, size_t count, const DtypeInfo *dt, int oi,
                            hipStream_t st) {
    World &w = world();
    const int n = w.size, me = w.rank;
    const bool reducing = n > 1 && oi != OP_NO_OP && oi != OP_REPLACE;
    const bool in_place = sendbuf == (const void *)-1;
    Plan p;
    if (!reducing) return allreduce_impl(sendbuf, recvbuf, count, dt, oi, st, tree_base(n));
    int rc = plan_allreduce(n, me, count, dt->size, dt->extent, in_place, 0, &p);
    if (rc) return rc;
    log_plan("allreduce", p, count);
    pvar_note(PV_COLL_ALLREDUCE, p, in_place, count, n);
    if (p.algo != ALG_RING) return allreduce_impl(sendbuf, recvbuf, count, dt, oi, st, tree_from_plan(p, n, count, me));
    if (count < (size_t)n) return allreduce_impl(sendbuf, recvbuf, count, dt, oi, st, tree_rs(n, count, me, false));
    const size_t main = (count / n) * n, rest = count - main, off = main * (size_t)dt->extent;
    rc = in_place ? allreduce_impl(sendbuf, recvbuf, main, dt, oi, st, tree_rs(n, main, me, false))
                  : allreduce_impl(sendbuf, recvbuf, main, dt, oi, st, tree_base(n), true);
    if (rc || !rest) return rc;
    return allreduce_impl(in_place ? sendbuf : (const char *)sendbuf + off, (char *)recvbuf + off, rest, dt, oi, st,
                          tree_rs(n, rest, me, false));
}
int allreduce_entry(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream) {
    hp_entry();
    const DtypeInfo *dt = nullptr;
    int rc = check_op_dtype(op, dtype, &dt);
    if (rc || count == 0) return rc;  // allreduce_osu.c:3730
    if ((rc = kind_supported(dt)) || (rc = require_world())) return rc;
    return allreduce_select(sendbuf, recvbuf, count, dt, op_index(op), pick_stream(stream));
}

// MPI_Scan / MPI_Exscan over this node's ranks (orders.cpp plan_scan: MPIR_Scan_generic /
// MPIR_Exscan, one algorithm at every size).  Every rank gets a different tree over the same
// operands.  Small messages: the one-shot scan kernel with this rank's own program, its operand
// pushed only to the ranks above it.  Larger ones: PIPE_SCAN, where the owner of a segment
// computes every rank's value in one pass of the reference's loop and reads from the table of all
// ranks' programs only which ranks have a result (coll/pipe.h).  The crossover is the allreduce's (oneshot_max),
// unmeasured for scans.  MPI_Exscan's rank 0 takes part in every push and flag but has no result:
// its recvbuf is never written, staged or not.
int scan_entry(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream, bool excl) {
    hp_entry();
    const DtypeInfo *dt = nullptr;
    int rc = check_op_dtype(op, dtype, &dt);
    if (rc || count == 0) return rc;
    if ((rc = kind_supported(dt)) || (rc = require_world())) return rc;
    World &w = world();
    const int n = w.size, me = w.rank, oi = op_index(op);
    if (oi >= OP_REPLACE) {
        MV2_ERR("MPI_%s: MPI_REPLACE / MPI_NO_OP are not supported", excl ? "Exscan" : "Scan");
        return E_OP;
    }
    hipStream_t st = pick_stream(stream);
    const size_t bytes = count * (size_t)dt->extent;
    const bool in_place = sendbuf == (const void *)-1 || sendbuf == recvbuf;
    const bool no_result = excl && me == 0;
    if (n == 1) {  // Scan copies, Exscan does nothing
        if (!excl && !in_place && hipMemcpyAsync(recvbuf, sendbuf, bytes, hipMemcpyDefault, st) != hipSuccess)
            return E_INTERN;
        return finish(st, false);
    }
    Staged s;
    if ((rc = stage_in(sendbuf, recvbuf, bytes, bytes, in_place, st, s))) return rc;
    if (no_result) s.copy_back = false;
    TreeParams tp = tree_base(n);
    tp.linear = 4;
    if (bytes <= w.oneshot_max && bytes <= w.slot_bytes) {
        Plan p;
        if ((rc = plan_scan(n, me, count, excl, OPK_BUILTIN, &p))) return rc;
        log_plan(excl ? "exscan" : "scan", p, count);
        tp.ps = p.ps;
        OneShotArgs a{};
        oneshot_common(a, st);
        a.send = s.send;
        a.recv = s.recv;
        a.count = count;
        a.nvec = bytes <= (size_t)ar_scalar_max() ? 0 : bytes / 16;
        a.tp = tp;
        a.scan = no_result ? 2 : 1;
        rc = oneshot_launch(a, a.nvec, oi, dt, st);
    } else {
        if ((rc = scan_progs(n, excl, OPK_BUILTIN, &tp.ps))) return rc;
        MV2_DEBUG("%s count %zu -> pipelined %s", excl ? "exscan" : "scan", count, algo_name(excl ? ALG_EXSCAN_RD : ALG_SCAN_RD));
        PipeArgs a{};
        a.mode = PIPE_SCAN;
        a.send = s.send;
        a.recv = s.recv;
        a.esize = dt->extent;
        even_segments(a, bytes, n);
        a.tp = tp;
        rc = run_pipe(a, oi, dt, st);
    }
    if (rc) return rc;
    if ((rc = stage_out(s, st))) return rc;
    return finish(st, w.timing);
}

// forced: the programs to run instead of the one-node selection's (a node step of
// MPIR_Reduce_two_level_helper_MV2 across nodes, whose function the multi-node table names)
int reduce_entry(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, int root, void *stream,
                 const Plan *forced) {
    hp_entry();
    const DtypeInfo *dt = nullptr;
    int rc = check_op_dtype(op, dtype, &dt);
    if (rc || count == 0) return rc;
    if ((rc = kind_supported(dt)) || (rc = require_world())) return rc;
    World &w = world();
    if (root < 0 || root >= w.size) return E_ROOT;
    hipStream_t st = pick_stream(stream);
    const size_t bytes = count * (size_t)dt->extent;
    const int oi = op_index(op);
    const bool is_root = w.rank == root;
    const bool in_place = sendbuf == (const void *)-1 || (is_root && sendbuf == recvbuf);
    // MPIR_Reduce_index_tuned_intra_MV2's one-node choice (orders.cpp plan_reduce)
    Plan p;
    if (forced) p = *forced;
    else if ((rc = plan_reduce(w.size, w.rank, root, count, dt->size, dt->extent, &p))) return rc;
    log_plan("reduce", p, count);
    pvar_note(PV_COLL_REDUCE, p, in_place, count, w.size);
    const TreeParams tp = tree_from_plan(p, w.size, count, w.rank);
    // small messages, REPLACE / NO_OP, one rank: every rank computes the root's result
    // (one-shot); non-roots discard theirs
    if (w.size == 1 || oi >= OP_REPLACE || (bytes <= w.oneshot_max && bytes <= w.slot_bytes)) {
        if (is_root) return allreduce_impl(sendbuf, recvbuf, count, dt, oi, st, tp);
        void *tmp = call_scratch(2, bytes);
        if (!tmp) return E_NO_MEM;
        return allreduce_impl(in_place ? recvbuf : sendbuf, tmp, count, dt, oi, st, tp);
    }
    // pipelined: scatter -> reduce -> push to the root -> root gathers
    Staged s{};
    if (is_root) {
        if ((rc = stage_in(sendbuf, recvbuf, bytes, bytes, in_place, st, s))) return rc;
    } else {
        s.recv = nullptr;
        s.copy_back = false;
        if (!(s.send = device_operand(in_place ? recvbuf : sendbuf, bytes, 0, 0, st))) return E_NO_MEM;
    }
    PipeArgs a{};
    a.mode = PIPE_RED;
    a.root = root;
    a.send = s.send;
    a.recv = s.recv;
    a.esize = dt->extent;
    a.tp = tp;
    even_segments(a, bytes, w.size);
    if ((rc = run_pipe(a, oi, dt, st))) return rc;
    if (is_root && (rc = stage_out(s, st))) return rc;
    return finish(st, w.timing);
}

int reduce_scatter_entry(const void *sendbuf, void *recvbuf, const size_t *recvcounts, int dtype, int op,
                        void *stream) {
    hp_entry();
    const DtypeInfo *dt = nullptr;
    int rc = check_op_dtype(op, dtype, &dt);
    if (rc) return rc;
    if ((rc = kind_supported(dt))) return rc;
    if ((rc = require_world())) return rc;
    World &w = world();
    const int n = w.size;
    const size_t ext = dt->extent;
    size_t total = 0, off = 0, padded = 0;
    for (int j = 0; j < n; ++j) {
        if (j == w.rank) off = total;
        total += recvcounts[j];
        padded += (recvcounts[j] * ext + 15) & ~(size_t)15;
    }
    if (total == 0) return 0;
    const int oi = op_index(op);
    hipStream_t st = pick_stream(stream);
    const size_t mycnt = recvcounts[w.rank];
    const bool in_place = sendbuf == (const void *)-1;
    const void *send = in_place ? recvbuf : sendbuf;
    if (n == 1 || oi == OP_NO_OP || oi == OP_REPLACE) {
        if (!in_place && oi != OP_NO_OP && mycnt)
            hipMemcpyAsync(recvbuf, (const char *)send + off * ext, mycnt * ext, hipMemcpyDefault, st);
        return finish(st, false);
    }
    // small messages: the one-shot reduce-scatter (each peer pushed only its own block, one flag
    // exchange, this rank's block reduced in program order) when the operand fits an arena slot,
    // every block starts on a 16-byte boundary and the algorithm is not the ring (whose rotated
    // chain only the pipelined kernel evaluates).  Only the counts, the type and the plan enter
    // the choice, so every rank makes it alike.
    Plan p;
    if ((rc = plan_reduce_scatter(n, w.rank, recvcounts, dt->size, dt->extent, &p))) return rc;
    // Blocks off 16-byte boundaries take the same kernel element by element when the whole operand
    // is small (kOneShotScalar; osu_reduce_scatter 8 B at 2 shared ranks: 16.4 us pipelined).
    constexpr size_t kOneShotScalar = 2048;
    bool os = !in_place && p.algo != ALG_RS_RING && (size_t)dt->size == ext && 16 % ext == 0 &&
              total * ext <= std::min(w.oneshot_max, w.slot_bytes);
    bool aligned = true;
    for (size_t j = 0, off0 = 0; j < (size_t)n; off0 += recvcounts[j], ++j) aligned = aligned && (off0 * ext) % 16 == 0;
    if (!aligned && total * ext > kOneShotScalar) os = false;
    // small operands element by element even when aligned: 1.9 / 2.3 us faster at 2 / 4 shared
    // ranks from 32 B to 4 KiB than the vector body (profiles/r05y)
    if (total * ext <= (size_t)rs_scalar_max()) aligned = false;
    if (os) {
        log_plan("reduce_scatter", p, total);
        pvar_note(PV_COLL_REDUCE_SCATTER, p, false, total, n);
        const char *src = (const char *)send;
        if (!is_device(send) || (uintptr_t)send % 16) {
            char *t = (char *)call_scratch(0, total * ext);
            if (!t) return E_NO_MEM;
            beacon(BC_STAGE);
            hipMemcpyAsync(t, send, total * ext, hipMemcpyDefault, st);
            src = t;
        }
        const bool direct = is_device(recvbuf) && (uintptr_t)recvbuf % 16 == 0;
        char *dst = (char *)recvbuf;
        if (!direct && mycnt && !(dst = (char *)call_scratch(1, mycnt * ext))) return E_NO_MEM;
        OneShotArgs o{};
        oneshot_common(o, st);
        o.send = src;
        o.recv = dst;
        o.count = total;
        o.nvec = aligned ? total * ext / 16 : 0;
        o.rs = 1;
        size_t vmax = 0;
        for (size_t j = 0, e = 0; j < (size_t)n; e += recvcounts[j], ++j) {
            o.wlo[j] = e;
            o.wcnt[j] = recvcounts[j];
            vmax = std::max(vmax, (recvcounts[j] * ext + 15) / 16);
        }
        TreeParams tp = tree_base(n);
        tp.linear = 4;
        tp.ps = p.ps;
        o.tp = tp;
        if ((rc = oneshot_launch(o, aligned ? vmax : 0, oi, dt, st))) return rc;
        if (!direct && mycnt && enq_copy_last(recvbuf, dst, mycnt * ext, st) != hipSuccess) return E_INTERN;
        return finish(st, w.timing);
    }
    PipeArgs a{};
    a.mode = PIPE_RS;
    a.esize = (int)ext;
    // operand: the caller's buffer when it is aligned device memory (and not IN_PLACE:
    // the result overwrites the operand's head) — segments off 16-byte boundaries keep
    // their misalignment through the kernel; otherwise a staged copy with every segment
    // padded to 16 bytes
    if (!in_place && is_device(send) && (uintptr_t)send % 16 == 0) {
        a.send = (const char *)send;
        size_t o = 0;
        for (int j = 0; j < n; ++j) {
            a.seg_off[j] = o * ext;
            a.seg_len[j] = recvcounts[j] * ext;
            o += recvcounts[j];
        }
    } else {
        char *t = (char *)call_scratch(0, padded);
        if (!t) return E_NO_MEM;
        beacon(BC_STAGE);
        size_t o = 0, po = 0;
        for (int j = 0; j < n; ++j) {
            const size_t len = recvcounts[j] * ext;
            if (len) hipMemcpyAsync(t + po, (const char *)send + o * ext, len, hipMemcpyDefault, st);
            a.seg_off[j] = po;
            a.seg_len[j] = len;
            o += recvcounts[j];
            po += (len + 15) & ~(size_t)15;
        }
        a.send = t;
    }
    // the result must share my segment's misalignment: the caller's buffer when it does,
    // else a scratch block at that misalignment, copied out after the kernel
    const size_t mis = a.seg_off[w.rank] & 15;
    const bool direct = is_device(recvbuf) && (uintptr_t)recvbuf % 16 == mis;
    char *dst = (char *)recvbuf;
    a.recv_off[w.rank] = 0;
    if (!direct && mycnt) {
        char *t = (char *)call_scratch(1, mycnt * ext + 16);
        if (!t) return E_NO_MEM;
        dst = t + mis;
    }
    a.recv = dst - (direct ? 0 : mis);
    a.recv_off[w.rank] = direct ? 0 : mis;
    // MPIR_Reduce_scatter_MV2's one-node choice (orders.cpp plan_reduce_scatter): ring,
    // recursive halving, pairwise or reduce + scatter, each in its own order
    log_plan("reduce_scatter", p, total);
    pvar_note(PV_COLL_REDUCE_SCATTER, p, false, total, n);
    TreeParams tp = tree_base(n);
    if (p.algo == ALG_RS_RING) {
        tp.linear = 2;  // rotated sources, specialised chain (coll/pipe.h reduce_round)
    } else {
        tp.linear = 4;
        tp.ps = p.ps;
        a.eshift = (int64_t)off - (int64_t)(a.seg_off[w.rank] / ext);
    }
    a.tp = tp;
    if ((rc = run_pipe(a, oi, dt, st))) return rc;
    if (!direct && mycnt && enq_copy_last(recvbuf, dst, mycnt * ext, st) != hipSuccess) return E_INTERN;
    return finish(st, w.timing);
}

int allgather_node(const void *sendbuf, void *recvbuf, size_t bytes, void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    if (bytes == 0) return 0;
    World &w = world();
    hipStream_t st = pick_stream(stream);
    const int n = w.size, me = w.rank;
    const bool in_place = sendbuf == (const void *)-1;
    // direct: rank j's block lands at recvbuf + j*bytes even when that is off a 16-byte
    // boundary (coll/pipe.h keeps each block's misalignment through the slots); the
    // contribution must then share its block's misalignment
    const bool direct = is_device(recvbuf) && (uintptr_t)recvbuf % 16 == 0;
    const size_t pitch = direct ? bytes : (bytes + 15) & ~(size_t)15;
    char *dst = direct ? (char *)recvbuf : (char *)call_scratch(1, pitch * n);
    if (!dst) return E_NO_MEM;
    const char *src = in_place ? (const char *)recvbuf + (size_t)me * bytes : (const char *)sendbuf;
    if (n == 1) {
        if (!in_place) hipMemcpyAsync(recvbuf, src, bytes, hipMemcpyDefault, st);
        return finish(st, false);
    }
    // small blocks: the one-shot kernel (one flag exchange; the choice reads only the size and the
    // node's shared limits, so every rank makes it alike).  Whole 16-byte vectors move as vectors;
    // a block of up to kOneShotBytewise bytes of any other size moves byte by byte (osu_allgather
    // 8 B at 2 shared ranks: 15.6 us through the pipelined kernel)
    const bool vec = bytes % 16 == 0;
    if ((vec || bytes <= kOneShotBytewise) && bytes <= std::min(w.oneshot_max, w.slot_bytes)) {
        // blocks packed at `bytes` in dst (the scratch block holds pitch * n >= bytes * n)
        const char *os = in_place ? dst + (size_t)me * bytes : (const char *)sendbuf;
        if (in_place && !direct) {
            hipMemcpyAsync(dst + (size_t)me * bytes, src, bytes, hipMemcpyDefault, st);
        } else if (!in_place && !(is_device(sendbuf) && (!vec || (uintptr_t)sendbuf % 16 == 0))) {
            char *t = (char *)call_scratch(0, bytes);
            if (!t) return E_NO_MEM;
            hipMemcpyAsync(t, sendbuf, bytes, hipMemcpyDefault, st);
            os = t;
        }
        OneShotArgs a{};
        oneshot_common(a, st);
        a.mv = 1;
        a.send = os;
        a.recv = dst;
        a.count = bytes;
        a.nvec = vec ? bytes / 16 : 0;
        a.pitch = bytes;
        if ((rc = oneshot_launch(a, a.nvec, 0, nullptr, st))) return rc;
        if (!direct && enq_copy_last(recvbuf, dst, bytes * n, st) != hipSuccess) return E_INTERN;
        return finish(st, w.timing);
    }
    const size_t mis = ((size_t)me * pitch) & 15;
    if (!(direct && in_place) && !(src = device_operand(src, bytes, mis, 0, st))) return E_NO_MEM;
    PipeArgs a{};
    a.mode = PIPE_AG;
    a.send = src;
    a.recv = dst;
    a.esize = 1;
    for (int j = 0; j < n; ++j) {
        a.seg_len[j] = bytes;
        a.recv_off[j] = a.seg_off[j] = (size_t)j * pitch;  // seg_off: the block's misalignment
    }
    if ((rc = run_pipe(a, 0, nullptr, st))) return rc;
    if (!direct) {
        w.pending = 0;
        hipMemcpy2DAsync(recvbuf, bytes, dst, pitch, bytes, n, hipMemcpyDefault, st);
    }
    return finish(st, w.timing);
}

int bcast_node(void *buffer, size_t bytes, int root, void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    if (bytes == 0) return 0;
    World &w = world();
    if (root < 0 || root >= w.size) return E_ROOT;
    if (w.size == 1) return 0;
    hipStream_t st = pick_stream(stream);
    char *buf = (char *)buffer;
    const bool direct = is_device(buffer) && (uintptr_t)buffer % 16 == 0;
    if (!direct) {
        buf = (char *)call_scratch(1, bytes);
        if (!buf) return E_NO_MEM;
        if (w.rank == root) hipMemcpyAsync(buf, buffer, bytes, hipMemcpyDefault, st);
    }
    // small messages: the one-shot kernel (the root pushes its buffer into every peer's arena slot,
    // one flag exchange); the choice reads only the size and the node's shared limits
    if (bytes <= std::min(w.oneshot_max, w.slot_bytes)) {
        OneShotArgs a{};
        oneshot_common(a, st);
        a.mv = 2;
        a.root = root;
        a.send = buf;
        a.recv = buf;
        a.count = bytes;
        a.nvec = bytes / 16;
        if ((rc = oneshot_launch(a, a.nvec, 0, nullptr, st))) return rc;
        if (!direct && w.rank != root && enq_copy_last(buffer, buf, bytes, st) != hipSuccess) return E_INTERN;
        return finish(st, w.timing);
    }
    PipeArgs a{};
    a.mode = PIPE_BC;
    a.root = root;
    a.send = buf;
    a.recv = buf;
    a.esize = 1;
    even_segments(a, bytes, w.size);
    if ((rc = run_pipe(a, 0, nullptr, st))) return rc;
    if (!direct && w.rank != root && enq_copy_last(buffer, buf, bytes, st) != hipSuccess) return E_INTERN;
    return finish(st, w.timing);
}

// The node step of a two-level table entry: the entry's intra-node function over the node's ranks
// (MPIR_Allreduce_two_level_MV2 :1727-1745; the leader's result is what the leaders reduce, and the
// node broadcast that ends the call overwrites every other rank's).  MN_INTRA_NODE: the node's own
// one-node selection, which reads the same table entry (16 ppn) or is the shortcut's order.
int node_allreduce_intra(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream,
                                int intra) {
    if (intra == MN_INTRA_NODE) return allreduce_entry(sendbuf, recvbuf, count, dtype, op, stream);
    const DtypeInfo *dt = nullptr;
    int rc = check_op_dtype(op, dtype, &dt);
    if (rc || count == 0) return rc;
    if ((rc = kind_supported(dt)) || (rc = require_world())) return rc;
    World &w = world();
    const int n = w.size, me = w.rank, oi = op_index(op);
    const bool in_place = sendbuf == (const void *)-1;
    if (n == 1 || oi == OP_NO_OP || oi == OP_REPLACE)
        return allreduce_impl(sendbuf, recvbuf, count, dt, oi, pick_stream(stream), tree_base(n));
    Plan p;
    if (intra == MN_INTRA_P2P) {  // MPIR_Reduce_MV2 to local rank 0 (the node's reduce selection)
        rc = plan_reduce(n, me, 0, count, dt->size, dt->extent, &p);
        p.inner = p.algo;
        p.algo = ALG_TWO_LEVEL_P2P;
    } else {
        rc = plan_allreduce(n, me, count, dt->size, dt->extent, in_place,
                            intra == MN_INTRA_RS   ? ALG_PT2PT_RS
                            : intra == MN_INTRA_RD ? ALG_PT2PT_RD
                                                   : ALG_SHMEM_LINEAR,
                            &p);
    }
    if (rc) return rc;
    log_plan("allreduce (node step)", p, count);
    return allreduce_impl(sendbuf, recvbuf, count, dt, oi, pick_stream(stream), tree_from_plan(p, n, count, me));
}

}  // namespace mv2

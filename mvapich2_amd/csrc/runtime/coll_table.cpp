// coll_table.cpp — the one-node collectives that move a table of per-rank blocks and reduce nothing:
// MPI_Alltoall(v), MPI_Gather(v), MPI_Scatter(v), MPI_Allgatherv (kernels: coll/alltoall.hip).  One
// plan, one reservation and launch, and one staging rule serve them all; the launch layer they share
// with the other collectives is coll_node.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../../include/mv2h.h"
#include "../coll/alltoall.h"
#include "coll_internal.h"
#include "log.h"

namespace mv2 {

// ---------------------------------------------------------------------------
// MPI_Alltoall / MPI_Alltoallv (kernels: coll/alltoall.hip).
//
// Both calls end in the same launch: a table of what this rank sends to and receives from every
// rank (offset, length, and the misalignment each incoming block carries), moved by the one-shot
// kernel when every pair is small and by the pipelined kernel otherwise.  The path, the grid and
// the round count read only values every rank shares: for MPI_Alltoall the block size, for
// MPI_Alltoallv the whole matrix of pair lengths, which the ranks publish in the control segment
// and read behind a host barrier (send counts are local knowledge; the longest pair of the job
// decides the geometry).
// ---------------------------------------------------------------------------
static uint64_t g_a2a_paths[4];  // calls by path (a2a_path_calls)
static uint64_t g_a2a_seq;       // MPI_Alltoallv calls issued (the published rows' sequence number)
uint64_t a2a_path_calls(int which) { return which >= 0 && which < 4 ? g_a2a_paths[which] : 0; }

// Path and geometry from the longest pair, whether every pair is a whole number of 16-byte
// vectors on 16-byte offsets, and the node's shared limits.
static A2APlan plan_from(size_t maxlen, bool vec) {
    World &w = world();
    A2APlan p{};
    p.maxlen = maxlen;
    if (!maxlen) return p;
    if ((vec || maxlen <= kOneShotBytewise) && maxlen <= std::min(w.oneshot_max, w.slot_bytes)) {
        p.path = vec ? A2A_ONESHOT_VEC : A2A_ONESHOT_BYTES;
        p.grid = oneshot_grid(vec ? maxlen / 16 : 0, grid_cap());
        p.nrounds = 1;
    } else {
        const PipeGeom g = pipe_geom(maxlen);
        p.path = A2A_PIPE;
        p.grid = g.grid;
        p.nrounds = g.nrounds;
    }
    return p;
}

int alltoallv_plan(int n, const size_t *slen, const size_t *rlen, const unsigned char *al16, A2APlan *out) {
    size_t maxlen = 0;
    bool vec = true, trunc = false;
    for (int i = 0; i < n; ++i) {
        vec = vec && al16[i];
        for (int j = 0; j < n; ++j) {
            trunc = trunc || slen[i * n + j] != rlen[j * n + i];
            maxlen = std::max(maxlen, slen[i * n + j]);
            vec = vec && slen[i * n + j] % 16 == 0;
        }
    }
    if (trunc) return E_TRUNCATE;
    *out = plan_from(maxlen, vec);
    return 0;
}

// The per-call part of a table launch: the pipelined path takes its rounds and epochs, the one-shot
// path its arena half and epoch, as every other collective does (pipe_reserve / oneshot_reserve).
// Returns the grid.
static int table_reserve(TableRt &rt, const A2APlan &p, hipStream_t st) {
    if (p.path == A2A_PIPE) {
        const PipeGeom g = pipe_geom(p.maxlen);
        pipe_reserve(rt, g, st);
        return g.grid;
    }
    oneshot_reserve(rt, rt.epoch0, st);
    rt.nvec = p.path == A2A_ONESHOT_VEC ? p.maxlen / 16 : 0;
    return p.grid;
}

// Launch the planned kernel of either table (send / recv as stage_send / stage_recv leave them) and
// count the call under its path in `paths` (a2a_path_calls / gv_path_calls index them alike).
template <class Args>
static int table_launch(Args &a, const A2APlan &p, bool shifted, uint64_t *paths, const char *what,
                        int (*oneshot)(const Args &, const LaunchCfg &), int (*pipe)(const Args &, const LaunchCfg &),
                        hipStream_t st) {
    a.n = world().size;
    a.me = world().rank;
    const int grid = table_reserve(a.rt, p, st);
    const bool piped = p.path == A2A_PIPE;
    ++paths[piped ? 2 : p.path == A2A_ONESHOT_VEC ? 0 : 1];
    if (piped && shifted) ++paths[3];
    if (piped)
        MV2_DEBUG("%s pipelined grid %d tsub %zu rounds %d maxlen %zu%s", what, grid, a.rt.tsub, a.rt.nrounds, p.maxlen,
                  shifted ? " (shifted gather)" : "");
    tmark0(st);
    const int rc = (piped ? pipe : oneshot)(a, coll_cfg(grid, st));
    tmark1(st);
    return rc;
}

static int a2a_launch(A2AArgs &a, const A2APlan &p, hipStream_t st) {
    bool shifted = false;
    for (int j = 0; j < world().size; ++j)
        shifted = shifted || (j != world().rank && a.rlen[j] && a.smis[j] != (uint32_t)(a.roff[j] & 15));
    return table_launch(a, p, shifted, g_a2a_paths, "alltoall", launch_oneshot_a2a, launch_pipe_a2a, st);
}

// ---------------------------------------------------------------------------
// Staging.  A table kernel takes a buffer as it is when it is device memory and either 16-byte
// aligned or on the byte-wise path (which moves single bytes and takes any address); anything else
// goes through call_scratch: index 0 the send side, 1 the receive side.  A buffer is a list of nb
// blocks (off[j], len[j]), possibly one: only bytes inside blocks are read from a send buffer or
// written to a receive buffer, a gap need not be addressable, and a buffer none of whose blocks has
// a length is never dereferenced.
// ---------------------------------------------------------------------------

// The send side as the kernel reads it, block j at + off[j] (nullptr: no memory).
static const char *stage_send(const void *buf, int nb, const size_t *off, const size_t *len, bool bytewise,
                              hipStream_t st) {
    if (is_device(buf) && (bytewise || (uintptr_t)buf % 16 == 0)) return (const char *)buf;
    size_t span = 16;
    for (int j = 0; j < nb; ++j)
        if (len[j]) span = std::max(span, off[j] + len[j]);
    char *t = (char *)call_scratch(0, span);
    if (!t) return nullptr;
    beacon(BC_STAGE);
    for (int j = 0; j < nb; ++j)
        if (len[j]) hipMemcpyAsync(t + off[j], (const char *)buf + off[j], len[j], hipMemcpyDefault, st);
    return t;
}

// The receive side as the kernel writes it: block j at dst + off[j].
struct RecvStage {
    char *dst = nullptr;
    bool direct = true;
    size_t off[kMaxRanks] = {};
};
enum {
    ST_FILL = 1,   // the blocks are read too (MPI_IN_PLACE): a staged copy starts with their bytes
    ST_PACK = 2,   // a staged copy holds the blocks back to back, each on a 16-byte boundary
    ST_OFF16 = 4,  // taken as it is only if every block's offset is a multiple of 16 as well
};
static int stage_recv(RecvStage &r, void *buf, int nb, const size_t *off, const size_t *len, bool bytewise, int flags,
                      hipStream_t st) {
    bool off16 = true;
    size_t span = 16, packed = 0;
    for (int j = 0; j < nb; ++j) {
        r.off[j] = len[j] ? off[j] : 0;
        if (len[j]) off16 = off16 && off[j] % 16 == 0;
        if (len[j]) span = std::max(span, off[j] + len[j]);
    }
    r.dst = (char *)buf;
    r.direct = is_device(buf) && (bytewise || ((uintptr_t)buf % 16 == 0 && (!(flags & ST_OFF16) || off16)));
    if (r.direct) return 0;
    if (flags & ST_PACK) {
        for (int j = 0; j < nb; packed += (len[j] + 15) & ~(size_t)15, ++j) r.off[j] = packed;
        span = packed;
    }
    if (!(r.dst = (char *)call_scratch(1, span))) return E_NO_MEM;
    if (flags & ST_FILL)
        for (int j = 0; j < nb; ++j)
            if (len[j]) hipMemcpyAsync(r.dst + r.off[j], (char *)buf + off[j], len[j], hipMemcpyDefault, st);
    return 0;
}

// A staged receive side back to the caller's buffer, block by block; one block ends the call.
static int stage_back(const RecvStage &r, void *buf, int nb, const size_t *off, const size_t *len, hipStream_t st) {
    if (r.direct) return 0;
    for (int j = 0; j < nb; ++j)
        if (len[j] && (nb == 1 ? enq_copy_last : enq_copy)((char *)buf + off[j], r.dst + r.off[j], len[j], st) != hipSuccess)
            return E_INTERN;
    return 0;
}

// One rank: the block copied to its place unless it is there (or empty), and the call is over.
static int self_copy(void *dst, const void *src, size_t bytes, bool in_place, hipStream_t st) {
    if (!in_place && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st) != hipSuccess) return E_INTERN;
    return finish(st, false);
}

int alltoall_node(const void *sendbuf, void *recvbuf, size_t bytes, void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    if (bytes == 0) return 0;
    World &w = world();
    hipStream_t st = pick_stream(stream);
    const int n = w.size, me = w.rank;
    const bool in_place = sendbuf == (const void *)-1;
    if (n == 1) return self_copy(recvbuf, sendbuf, bytes, in_place, st);
    const size_t total = bytes * (size_t)n, zero = 0;
    const A2APlan p = plan_from(bytes, bytes % 16 == 0);
    // Blocks lie back to back, so block j starts at j * bytes whatever that is modulo 16: each side
    // is one block.  The receive side wants an aligned base on every path.
    RecvStage r;
    if ((rc = stage_recv(r, recvbuf, 1, &zero, &total, false, in_place ? ST_FILL : 0, st))) return rc;
    char *dst = r.dst;
    const char *src = in_place ? dst : stage_send(sendbuf, 1, &zero, &total, p.path == A2A_ONESHOT_BYTES, st);
    if (!src) return E_NO_MEM;
    A2AArgs a{};
    a.send = src;
    a.recv = dst;
    for (int j = 0; j < n; ++j) {
        a.soff[j] = a.roff[j] = (size_t)j * bytes;
        a.slen[j] = a.rlen[j] = bytes;
        a.smis[j] = (uint32_t)(((size_t)me * bytes) & 15);  // rank j's block for me starts at me * bytes there
    }
    if ((rc = a2a_launch(a, p, st)) || (rc = stage_back(r, recvbuf, 1, &zero, &total, st))) return rc;
    return finish(st, w.timing);
}

// One table of per-pair blocks whose lengths only the two ends of a pair know (MPI_Alltoallv; the
// root's row or column of MPI_Scatterv / MPI_Gatherv), n > 1: exchange the rows, plan from the
// whole matrix, stage, launch, copy back.  in_place: the send blocks are the receive blocks
// (sendbuf is not read).  A buffer none of whose blocks has a length is never dereferenced.
static int a2av_table(const char *name, const void *sendbuf, const size_t *sbytes, const size_t *soffs, void *recvbuf,
                      const size_t *rbytes, const size_t *roffs, bool in_place, hipStream_t st) {
    World &w = world();
    const int n = w.size, me = w.rank;
    int rc;
    // publish my row, meet, read the matrix, meet again (nobody rewrites its row for the next call
    // before every rank has read this one)
    A2ARow &mine = w.shm->a2a[me];
    mine.seq = ++g_a2a_seq;
    bool al16 = true;
    for (int j = 0; j < n; ++j) {
        mine.slen[j] = sbytes[j];
        mine.rlen[j] = rbytes[j];
        mine.smis[j] = (uint8_t)(soffs[j] & 15);
        al16 = al16 && soffs[j] % 16 == 0 && roffs[j] % 16 == 0;
    }
    mine.al16 = al16;
    host_barrier();
    size_t slen[kMaxRanks * kMaxRanks], rlen[kMaxRanks * kMaxRanks];
    unsigned char al[kMaxRanks];
    uint32_t smis[kMaxRanks];
    bool same_call = true;
    for (int i = 0; i < n; ++i) {
        const A2ARow &r = w.shm->a2a[i];
        same_call = same_call && r.seq == mine.seq;
        al[i] = r.al16;
        smis[i] = r.smis[me];
        for (int j = 0; j < n; ++j) {
            slen[i * n + j] = (size_t)r.slen[j];
            rlen[i * n + j] = (size_t)r.rlen[j];
        }
    }
    host_barrier();
    if (!same_call) {
        MV2_ERR("%s: the ranks of the node are not in the same call", name);
        return E_OTHER;
    }
    A2APlan p{};
    if ((rc = alltoallv_plan(n, slen, rlen, al, &p))) {
        MV2_ERR("%s: a pair's send and receive lengths differ", name);
        return rc;
    }
    if (p.path == A2A_NONE) return 0;  // every pair is empty, on every rank
    const bool bytewise = p.path == A2A_ONESHOT_BYTES;
    RecvStage r;
    if ((rc = stage_recv(r, recvbuf, n, roffs, rbytes, bytewise, in_place ? ST_FILL : 0, st))) return rc;
    char *dst = r.dst;
    const char *src = in_place ? dst : stage_send(sendbuf, n, soffs, sbytes, bytewise, st);
    if (!src) return E_NO_MEM;
    A2AArgs a{};
    a.send = src;
    a.recv = dst;
    for (int j = 0; j < n; ++j) {
        a.soff[j] = soffs[j];
        a.slen[j] = sbytes[j];
        a.roff[j] = roffs[j];
        a.rlen[j] = rbytes[j];
        a.smis[j] = smis[j];
    }
    if ((rc = a2a_launch(a, p, st)) || (rc = stage_back(r, recvbuf, n, roffs, rbytes, st))) return rc;
    return finish(st, w.timing);
}

int alltoallv_node(const void *sendbuf, const size_t *sbytes, const size_t *soffs, void *recvbuf, const size_t *rbytes,
                   const size_t *roffs, void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    if (!rbytes || !roffs) return E_ARG;
    World &w = world();
    const bool in_place = sendbuf == (const void *)-1;
    if (in_place) {
        sbytes = rbytes;
        soffs = roffs;
    } else if (!sbytes || !soffs) {
        return E_ARG;
    }
    hipStream_t st = pick_stream(stream);
    if (w.size == 1) {
        if (sbytes[0] != rbytes[0]) return E_TRUNCATE;
        return self_copy((char *)recvbuf + roffs[0], in_place ? nullptr : (const char *)sendbuf + soffs[0], sbytes[0], in_place,
                         st);
    }
    return a2av_table("MPI_Alltoallv", sendbuf, sbytes, soffs, recvbuf, rbytes, roffs, in_place, st);
}

// ---------------------------------------------------------------------------
// MPI_Allgatherv / MPI_Gather(v) / MPI_Scatter(v) (kernels: coll/alltoall.hip).
//
// Allgatherv and Gather: every rank has one block for a set of ranks -- the gather table (GvArgs)
// on k_oneshot_gv / k_pipe_gv, which read a block once and store it to every destination.  The
// plan reads only the n block lengths, which every rank knows (Allgatherv's recvcounts, Gather's
// one count); displacements and addresses are local and never enter it.  recvcounts that differ
// between the ranks of one MPI_Allgatherv are erroneous MPI: the ranks then disagree on the grid
// or the round count and the call ends in the kernels' timeout (MPI_ERR_OTHER).
// Scatter: n different blocks at the root -- an all-to-all table whose only non-empty row is the
// root's, on the all-to-all kernels.  A receiver derives the misalignment its block arrives with
// from the root's 16-byte-aligned base: (me * bytes) & 15.
// Gatherv and Scatterv: only the root knows the lengths, so they are all-to-all tables with one
// non-empty column / row through a2av_table (row exchange, MPI_ERR_TRUNCATE for a mismatched pair
// on every rank before any device work), on the all-to-all kernels and under their counters.
// ---------------------------------------------------------------------------
static uint64_t g_gv_paths[4];  // calls by path (gv_path_calls)
static int g_agv_via_a2a;       // test hook: MPI_Allgatherv through the all-to-all table
uint64_t gv_path_calls(int which) { return which >= 0 && which < 4 ? g_gv_paths[which] : 0; }
void set_agv_via_a2a(int on) { g_agv_via_a2a = on != 0; }

int gv_plan(int n, const size_t *len, A2APlan *out) {
    size_t maxlen = 0;
    bool vec = true;
    for (int j = 0; j < n; ++j) {
        maxlen = std::max(maxlen, len[j]);
        vec = vec && len[j] % 16 == 0;
    }
    *out = plan_from(maxlen, vec);
    return 0;
}

// One gather table, n > 1, planned: my block (slen bytes at sendbuf, any memory) goes to the ranks
// of dmask (own bit: also to my own receive block); I gather rlens[j] bytes from rank j at recvbuf
// + roffs[j] (all zero on a rank that receives nothing; its recvbuf is not dereferenced).  via_a2a:
// the same table on the all-to-all kernels (soff[j] = 0 for every j).
static int gv_run(const void *sendbuf, size_t slen, unsigned dmask, void *recvbuf, const size_t *roffs,
                  const size_t *rlens, const A2APlan &p, bool via_a2a, hipStream_t st) {
    World &w = world();
    const int n = w.size, me = w.rank;
    const bool bytewise = p.path == A2A_ONESHOT_BYTES, vecpath = p.path == A2A_ONESHOT_VEC;
    if (!slen) dmask = 0;
    if (!dmask) slen = 0;
    const bool own = (dmask >> me) & 1u;
    // wr[j]: bytes this call writes into my receive block j
    size_t wr[kMaxRanks] = {}, total = 0;
    for (int j = 0; j < n; ++j) total += wr[j] = j != me ? rlens[j] : (own ? slen : 0);
    // A vector path wants an aligned base (and, one-shot, aligned displacements): a rank whose own
    // are not gathers into scratch at packed aligned offsets and copies out block by block.
    int rc;
    RecvStage r;
    if (total && (rc = stage_recv(r, recvbuf, n, roffs, wr, bytewise, ST_PACK | (vecpath ? ST_OFF16 : 0), st))) return rc;
    char *dst = r.dst;
    const size_t *off = r.off, zero = 0;
    const char *src = slen ? stage_send(sendbuf, 1, &zero, &slen, bytewise, st) : nullptr;
    if (slen && !src) return E_NO_MEM;
    if (via_a2a) {
        A2AArgs a{};
        a.send = src;
        a.recv = dst;
        for (int j = 0; j < n; ++j) {
            a.slen[j] = (dmask >> j) & 1u ? slen : 0;
            a.roff[j] = off[j];
            a.rlen[j] = wr[j];
        }
        if ((rc = a2a_launch(a, p, st))) return rc;
    } else {
        GvArgs a{};
        a.send = src;
        a.slen = slen;
        a.dmask = dmask;
        a.recv = dst;
        bool shifted = false;
        for (int j = 0; j < n; ++j) {
            a.roff[j] = off[j];
            a.rlen[j] = j != me ? wr[j] : 0;
            shifted = shifted || (wr[j] && ((uintptr_t)(dst + off[j]) & 15));
        }
        if ((rc = table_launch(a, p, shifted, g_gv_paths, "gather table", launch_oneshot_gv, launch_pipe_gv, st))) return rc;
    }
    if ((rc = stage_back(r, recvbuf, n, roffs, wr, st))) return rc;
    return finish(st, w.timing);
}

int allgatherv_node(const void *sendbuf, size_t sbytes, void *recvbuf, const size_t *rbytes, const size_t *roffs,
                    void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    if (!rbytes || !roffs) return E_ARG;
    World &w = world();
    const int n = w.size, me = w.rank;
    const bool in_place = sendbuf == (const void *)-1;
    if (!in_place && sbytes != rbytes[me]) return E_TRUNCATE;
    A2APlan p{};
    gv_plan(n, rbytes, &p);
    if (p.path == A2A_NONE) return 0;  // every count is zero, on every rank
    hipStream_t st = pick_stream(stream);
    const size_t mine = rbytes[me];
    const char *src = in_place ? (const char *)recvbuf + roffs[me] : (const char *)sendbuf;
    if (n == 1) return self_copy((char *)recvbuf + roffs[0], src, mine, in_place, st);
    unsigned dmask = ((1u << n) - 1u) & ~(1u << me);
    if (!in_place) dmask |= 1u << me;
    return gv_run(src, mine, dmask, recvbuf, roffs, rbytes, p, g_agv_via_a2a != 0, st);
}

int gather_node(const void *sendbuf, void *recvbuf, size_t bytes, int root, void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    World &w = world();
    const int n = w.size, me = w.rank;
    if (root < 0 || root >= n) return E_ROOT;
    if (bytes == 0) return 0;
    hipStream_t st = pick_stream(stream);
    const bool in_place = me == root && sendbuf == (const void *)-1;
    if (n == 1) return self_copy(recvbuf, sendbuf, bytes, in_place, st);
    size_t len[kMaxRanks], roffs[kMaxRanks] = {}, rlens[kMaxRanks] = {};
    for (int j = 0; j < n; ++j) {
        len[j] = bytes;
        if (me == root) {
            roffs[j] = (size_t)j * bytes;
            rlens[j] = bytes;
        }
    }
    A2APlan p{};
    gv_plan(n, len, &p);
    // the root's own block is copied by the own bit, or is in place: the root pushes nothing
    const unsigned dmask = me == root ? (in_place ? 0u : 1u << me) : 1u << root;
    return gv_run(in_place ? nullptr : sendbuf, bytes, dmask, me == root ? recvbuf : nullptr, roffs, rlens, p, false, st);
}

int gatherv_node(const void *sendbuf, size_t sbytes, void *recvbuf, const size_t *rbytes, const size_t *roffs, int root,
                 void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    World &w = world();
    const int n = w.size, me = w.rank;
    if (root < 0 || root >= n) return E_ROOT;
    if (me == root && (!rbytes || !roffs)) return E_ARG;
    hipStream_t st = pick_stream(stream);
    const bool in_place = me == root && sendbuf == (const void *)-1;
    if (n == 1) {
        if (in_place) return 0;
        if (sbytes != rbytes[0]) return E_TRUNCATE;
        return self_copy((char *)recvbuf + roffs[0], sendbuf, sbytes, false, st);
    }
    size_t sb[kMaxRanks] = {}, so[kMaxRanks] = {}, rb[kMaxRanks] = {}, ro[kMaxRanks] = {};
    if (me == root) {
        for (int j = 0; j < n; ++j) {
            rb[j] = rbytes[j];
            ro[j] = rbytes[j] ? roffs[j] : 0;
        }
        if (in_place) rb[me] = ro[me] = 0;  // already there
        else sb[me] = sbytes;
    } else {
        sb[root] = sbytes;
    }
    return a2av_table("MPI_Gatherv", in_place ? nullptr : sendbuf, sb, so, me == root ? recvbuf : nullptr, rb, ro, false, st);
}

int scatter_node(const void *sendbuf, void *recvbuf, size_t bytes, int root, void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    World &w = world();
    const int n = w.size, me = w.rank;
    if (root < 0 || root >= n) return E_ROOT;
    if (bytes == 0) return 0;
    hipStream_t st = pick_stream(stream);
    const bool in_place = me == root && recvbuf == (void *)-1;
    if (n == 1) return self_copy(recvbuf, sendbuf, bytes, in_place, st);
    const A2APlan p = plan_from(bytes, bytes % 16 == 0);
    const bool bytewise = p.path == A2A_ONESHOT_BYTES;
    A2AArgs a{};
    // my block arrives at recvbuf (the root's own: a local copy, unless it stays in place)
    const size_t total = bytes * (size_t)n, zero = 0;
    RecvStage r;
    if (!in_place && (rc = stage_recv(r, recvbuf, 1, &zero, &bytes, bytewise, 0, st))) return rc;
    a.recv = r.dst;
    if (!in_place) a.rlen[root] = bytes;
    a.smis[root] = (uint32_t)(((size_t)me * bytes) & 15);
    if (me == root) {
        if (!(a.send = stage_send(sendbuf, 1, &zero, &total, bytewise, st))) return E_NO_MEM;
        for (int j = 0; j < n; ++j) {
            a.soff[j] = (size_t)j * bytes;
            a.slen[j] = j == me && in_place ? 0 : bytes;
        }
    }
    if ((rc = a2a_launch(a, p, st)) || (rc = stage_back(r, recvbuf, 1, &zero, &bytes, st))) return rc;
    return finish(st, w.timing);
}

int scatterv_node(const void *sendbuf, const size_t *sbytes, const size_t *soffs, void *recvbuf, size_t rbytes, int root,
                  void *stream) {
    hp_entry();
    int rc;
    if ((rc = require_world())) return rc;
    World &w = world();
    const int n = w.size, me = w.rank;
    if (root < 0 || root >= n) return E_ROOT;
    if (me == root && (!sbytes || !soffs)) return E_ARG;
    hipStream_t st = pick_stream(stream);
    const bool in_place = me == root && recvbuf == (void *)-1;
    if (n == 1) {
        if (in_place) return 0;
        if (sbytes[0] != rbytes) return E_TRUNCATE;
        return self_copy(recvbuf, (const char *)sendbuf + soffs[0], rbytes, false, st);
    }
    size_t sb[kMaxRanks] = {}, so[kMaxRanks] = {}, rb[kMaxRanks] = {}, ro[kMaxRanks] = {};
    if (me == root) {
        for (int j = 0; j < n; ++j) {
            sb[j] = sbytes[j];
            so[j] = sbytes[j] ? soffs[j] : 0;
        }
        if (in_place) sb[me] = so[me] = 0;  // stays where it is
    }
    if (!in_place) rb[root] = rbytes;
    return a2av_table("MPI_Scatterv", me == root ? sendbuf : nullptr, sb, so, in_place ? nullptr : recvbuf, rb, ro, false, st);
}

}  // namespace mv2

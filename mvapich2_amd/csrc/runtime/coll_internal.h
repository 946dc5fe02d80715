// coll_internal.h — what the files of the collective runtime share: call.cpp (a call's stream,
// timing marks, completion and error word), coll_node.cpp (the one-node collectives and the two
// kernel families' per-call reservations), coll_table.cpp (the one-node calls that move a table of
// per-rank blocks: all-to-all, gather, scatter, allgatherv), coll_mn.cpp (across nodes),
// coll_init.cpp (MPI_Init's tuning and self-test), coll.cpp (the mv2h_* C-ABI).
#pragma once
#include "world.h"

namespace mv2 {

// ---- call.cpp ----
hipStream_t pick_stream(void *s);
void stream_tail(hipStream_t st);
uint64_t now_ns();
void hp_entry();  // a new API call
Done arm_done(hipStream_t st);
void withhold_done(int k);  // test hooks (mv2h_set_tuning)
void fake_split(int k);
hipError_t enq_copy(void *dst, const void *src, size_t bytes, hipStream_t st);
hipError_t enq_copy_last(void *dst, const void *src, size_t bytes, hipStream_t st);
hipError_t settle_split(hipStream_t st);
hipError_t wait_done(hipStream_t st, uint64_t want);
void log_epochs(uint64_t lo, uint64_t hi, hipStream_t st);
int check_err_word();
int finish(hipStream_t st, bool timed);
void tmark0(hipStream_t st);
void tmark1(hipStream_t st);
int is_device(const void *p);
int kind_supported(const DtypeInfo *dt);
int check_op_dtype(int op, int dtype, const DtypeInfo **out);

// ---- coll_node.cpp: the collectives over this node's ranks ----
TreeParams tree_base(int n);
void log_plan(const char *coll, const Plan &p, size_t count);
long ar_scalar_max();  // MV2AMD_AR_SCALAR_MAX / MV2AMD_RS_SCALAR_MAX
long rs_scalar_max();
int allreduce_entry(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream);
int node_allreduce_intra(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream, int intra);
int scan_entry(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream, bool excl);
int reduce_entry(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, int root, void *stream,
                 const Plan *forced = nullptr);
int reduce_scatter_entry(const void *sendbuf, void *recvbuf, const size_t *recvcounts, int dtype, int op, void *stream);
int allgather_node(const void *sendbuf, void *recvbuf, size_t bytes, void *stream);
int bcast_node(void *buffer, size_t bytes, int root, void *stream);
// what coll_table.cpp launches with
int grid_cap();
LaunchCfg coll_cfg(int grid, hipStream_t st);
struct PipeGeom {
    int grid;
    size_t tsub, tseg;
    int nrounds;
};
PipeGeom pipe_geom(size_t maxlen);
int oneshot_grid(size_t nvec, int gcap);
int require_world();
void *call_scratch(int idx, size_t bytes);
// blocks of any size up to this move byte by byte through a one-shot kernel (allgather, the tables)
constexpr size_t kOneShotBytewise = 2048;

// The per-call reservation of each kernel family, over any argument struct that names the fields
// alike (PipeArgs, OneShotArgs, coll/alltoall.h TableRt).  Nothing else advances w.round, w.epoch
// and w.os_calls, so every rank advances them alike whatever mix of collectives it runs; on the
// graph lane the kernel reads them from the device and the host advances nothing.
// Pipelined: g.nrounds rounds of slot parities, 2 * g.nrounds flag epochs (the AG region's peers;
// run_pipe adds the RS region's).
template <class A>
void pipe_reserve(A &a, const PipeGeom &g, hipStream_t st) {
    World &w = world();
    a.tsub = g.tsub;
    a.tseg = g.tseg;
    a.nrounds = g.nrounds;
    a.rnt = w.pipe_rnt;
    if (w.graph) {  // graph lane: own arenas and flags
        a.ag_peer = w.g_peer_ag;
        a.sig_peer = w.g_peer_sig;
        a.sig_own = w.g_sig;
        a.dseq = w.dseq;
    } else {
        a.ag_peer = w.peer_ag;
        a.sig_peer = w.peer_sig;
        a.sig_own = w.sig;
        a.round0 = w.round;
        w.round += (uint64_t)g.nrounds;
        a.epoch0 = w.epoch + 1;
        w.epoch += 2 * (uint64_t)g.nrounds;
        log_epochs(a.epoch0, w.epoch, st);
    }
    a.err = w.h_err;
    a.timeout = w.timeout_ticks;
    a.light = w.light_release;
    a.done = arm_done(st);
}
// One-shot: this call's arena half and flag epoch (`epoch`: the struct's member for it), the
// peers, the error word, the completion word.
template <class A>
void oneshot_reserve(A &a, uint64_t &epoch, hipStream_t st) {
    World &w = world();
    const size_t half = (size_t)kMaxRanks * w.slot_bytes;
    if (w.graph) {  // graph lane: the kernel picks the half and the epoch from the device
        for (int j = 0; j < w.size; ++j) a.arena_peer.p[j] = w.g_peer_arena[j];
        a.arena_own = w.g_arena;
        a.sig_peer = w.g_peer_sig;
        a.sig_own = w.g_sig;
        a.dseq = w.dseq;
        a.half = half;
    } else {
        const size_t par = (w.os_calls++ & 1) * half;
        for (int j = 0; j < w.size; ++j) a.arena_peer.p[j] = w.peer_arena[j] + par;
        a.arena_own = w.arena + par;
        a.sig_peer = w.peer_sig;
        a.sig_own = w.sig;
        epoch = ++w.epoch;
        log_epochs(epoch, epoch, st);
    }
    a.slot_bytes = w.slot_bytes;
    a.err = w.h_err;
    a.timeout = w.timeout_ticks;
    a.light = w.light_release;
    a.done = arm_done(st);
}

// ---- coll_table.cpp: the table collectives over this node's ranks (kernels: coll/alltoall.hip) ----
int alltoall_node(const void *sendbuf, void *recvbuf, size_t bytes, void *stream);
int alltoallv_node(const void *sendbuf, const size_t *sbytes, const size_t *soffs, void *recvbuf, const size_t *rbytes,
                   const size_t *roffs, void *stream);
// The plan of one Alltoallv from the whole matrix (slen[i * n + j]: bytes rank i sends rank j;
// rlen[i * n + j]: bytes rank i expects from rank j; al16[i]: every offset of rank i is a multiple
// of 16): a pure function of what every rank sees after the exchange and of the node's shared
// limits.  E_TRUNCATE when a pair's two lengths differ.
enum A2APath { A2A_NONE = 0, A2A_ONESHOT_VEC = 1, A2A_ONESHOT_BYTES = 2, A2A_PIPE = 3 };
struct A2APlan {
    int path, grid, nrounds;
    size_t maxlen;
};
int alltoallv_plan(int n, const size_t *slen, const size_t *rlen, const unsigned char *al16, A2APlan *out);
// all-to-all calls by path (mv2h_get_info a2a_*): 0 one-shot vector, 1 one-shot byte-wise, 2 pipelined,
// 3 those of the pipelined ones whose gather shifted at least one block
uint64_t a2a_path_calls(int which);
// MPI_Allgatherv / MPI_Gather(v) / MPI_Scatter(v) over this node's ranks, in bytes.  (void *)-1 is
// MPI_IN_PLACE: the send buffer of Allgatherv and of Gather(v) at the root, the receive buffer of
// Scatter(v) at the root.  Arguments that matter at the root only are not read elsewhere.
int allgatherv_node(const void *sendbuf, size_t sbytes, void *recvbuf, const size_t *rbytes, const size_t *roffs,
                    void *stream);
int gather_node(const void *sendbuf, void *recvbuf, size_t bytes, int root, void *stream);
int gatherv_node(const void *sendbuf, size_t sbytes, void *recvbuf, const size_t *rbytes, const size_t *roffs, int root,
                 void *stream);
int scatter_node(const void *sendbuf, void *recvbuf, size_t bytes, int root, void *stream);
int scatterv_node(const void *sendbuf, const size_t *sbytes, const size_t *soffs, void *recvbuf, size_t rbytes, int root,
                  void *stream);
// The plan of one gather table (Allgatherv, Gather) from the n block lengths, which every rank
// knows: the all-to-all's paths, never reading a displacement or an address.
int gv_plan(int n, const size_t *len, A2APlan *out);
// gather-table calls by path (mv2h_get_info gv_*), indexed like a2a_path_calls
uint64_t gv_path_calls(int which);
void set_agv_via_a2a(int on);  // test hook (mv2h_set_tuning "agv_via_a2a")

// ---- coll_mn.cpp: the collectives of a job on several nodes ----
int mn_allreduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream);
int mn_reduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, int root, void *stream);
int mn_reduce_scatter(const void *sendbuf, void *recvbuf, const size_t *recvcounts, int dtype, int op, void *stream);
int mn_allgather(const void *sendbuf, void *recvbuf, size_t bytes, void *stream);
int mn_bcast(void *buffer, size_t bytes, int root, void *stream);
int mn_allreduce_route(int ppn, int gsize, long nbytes, size_t count, bool in_place, int nbc, int *intra, int *inter,
                       int *sel_out, int *rem_route);
int mn_reduce_route(int ppn, int gsize, size_t count, int tsize, int nbc);
int mn_reduce_scatter_route(int gsize, long nbytes);

// a stream-ordered call (mv2h_*_enqueue); graph: one being captured into a HIP graph
struct EnqueueScope {
    explicit EnqueueScope(bool graph = false) {
        world().enqueue = true;
        world().graph = graph;
    }
    ~EnqueueScope() {
        world().enqueue = false;
        world().graph = false;
    }
};

}  // namespace mv2

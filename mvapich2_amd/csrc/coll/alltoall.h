// alltoall.h — host-side launch interface of the all-to-all kernels (coll/alltoall.hip).
#pragma once
#include "kernels.h"

namespace mv2 {

// The per-call part of a table launch, the last member of both argument structs below: what the
// runtime reserves for the call (runtime/coll_table.cpp table_reserve) and nothing of the table.
struct TableRt {
    // one-shot kernel: nvec = 16-byte vectors of the longest pair, partitioned over the workgroups
    // (every offset and length is then a multiple of 16); 0 = byte by byte through workgroup 0
    PeerTableW arena_peer;  // peers' one-shot arena (this call's half); my slot at + me * slot_bytes
    const char *arena_own;  // my arena (same half); rank j's slot at + j * slot_bytes
    size_t nvec, slot_bytes, half;
    // pipelined kernel (k_pipe's tiling, slot parities and flags; the AG region only)
    PeerTableW ag_peer;
    size_t tseg, tsub;
    uint64_t round0;
    int nrounds;
    int rnt;  // 1: non-temporal stores into peers' arenas
    SigTable sig_peer;
    uint64_t *sig_own;
    uint64_t epoch0;  // one-shot: the call's epoch; pipelined: round k uses epoch0 + 2k
    int light;
    int *err;
    uint64_t timeout;
    Done done;
    DevSeq *dseq;  // graph lane
};

// One all-to-all over this node's ranks (MPI_Alltoall: every pair the same length; MPI_Alltoallv:
// a length per pair).  Rank me sends slen[j] bytes at send + soff[j] to rank j and receives
// rlen[j] bytes from rank j at recv + roff[j]; slen[j] on rank me equals rlen[me] on rank j.
// send and recv are 16-byte aligned (the runtime stages anything else); the offsets are not.
struct A2AArgs {
    int n, me;
    const char *send;
    char *recv;
    size_t soff[kMaxRanks], slen[kMaxRanks];
    size_t roff[kMaxRanks], rlen[kMaxRanks];
    // smis[j]: rank j's (soff[me] & 15), the misalignment its block arrives with (pipelined kernel)
    uint32_t smis[kMaxRanks];
    TableRt rt;
};

// One gather over this node's ranks (MPI_Allgatherv: every rank receives; MPI_Gather: the root
// alone).  Rank me has one block, slen bytes at send, for the ranks of dmask; the own bit means
// "also copy it to my own recv + roff[me], unless it is already there".  It gathers rlen[j] bytes
// from rank j at recv + roff[j] (rlen[j] on rank me equals rank j's slen where rank j's dmask
// names me; all zero on a rank outside every mask; rlen[me] is not read).  send is 16-byte
// aligned, or any device address on the byte-wise path; the one-shot vector path also wants
// recv + roff[j] 16-byte aligned (the runtime stages anything else).
struct GvArgs {
    int n, me;
    const char *send;
    size_t slen;
    unsigned dmask;
    char *recv;
    size_t roff[kMaxRanks], rlen[kMaxRanks];
    TableRt rt;
};

// the kernarg layout the kernels were measured with, from before the block was one struct
static_assert(sizeof(A2AArgs) == 640 && offsetof(A2AArgs, rt.arena_peer) == 312 && offsetof(A2AArgs, rt.dseq) == 632,
              "A2AArgs layout");
static_assert(sizeof(GvArgs) == 496 && offsetof(GvArgs, rt.arena_peer) == 168 && offsetof(GvArgs, rt.dseq) == 488,
              "GvArgs layout");

int launch_oneshot_a2a(const A2AArgs &a, const LaunchCfg &cfg);
int launch_pipe_a2a(const A2AArgs &a, const LaunchCfg &cfg);
int launch_oneshot_gv(const GvArgs &a, const LaunchCfg &cfg);
int launch_pipe_gv(const GvArgs &a, const LaunchCfg &cfg);

}  // namespace mv2

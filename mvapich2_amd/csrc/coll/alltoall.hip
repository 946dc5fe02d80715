// alltoall.hip — MPI_Alltoall / MPI_Alltoallv over this node's ranks: every rank pushes the block
// it owes rank j into rank j's arena and copies the blocks it is owed out of its own.  Per rank the
// traffic is an allgather's at the same block size, (n-1) blocks out and (n-1) in; nothing is reduced.
//
// Two kernels, shaped like the allgather's: a one-shot kernel for small blocks (one flag exchange,
// the one-shot arena's halves) and a pipelined kernel for everything else (k_pipe's tiling, slot
// parities and flags, coll/pipe.h).
//
// Alignment.  The block a rank sends to rank j leaves send + soff[j] and lands at recv + roff[me]
// on rank j, and the two generally differ modulo 16 (a 12-byte block: offsets 0, 12, 24 ... on one
// side, me * 12 on the other).  Exactly one side realigns, and it is a local one: the arena slot
// keeps the sender's misalignment, so the push into the peer's arena is the equal-alignment copy
// every other collective uses (scalar head, whole 16-byte vectors on 16-byte addresses, scalar
// tail), and the receiver's gather -- its own arena to its own recv -- shifts (blk_copy_shift).
#include "alltoall.h"
#include "pipe.h"

#include "../common.h"

namespace mv2 {

// ---------------------------------------------------------------------------
// What the four kernels share, all of it read from the per-call part of their arguments (TableRt).
// ---------------------------------------------------------------------------

// The call's flag epoch (pipelined: its first), first round and one-shot arena half; on the graph
// lane this replay's, read from the device before any workgroup can advance them.
struct TableCall {
    uint64_t epoch, round0;
    size_t poff;
};
__device__ __forceinline__ TableCall table_call(const TableRt &rt) {
    TableCall c{rt.epoch0, rt.round0, 0};
    if (rt.dseq) {
        const SeqBase q = dseq_read(rt.dseq);
        c = TableCall{q.epoch + 1, q.round, (q.os & 1) * rt.half};
    }
    return c;
}

// The end of a kernel: the graph lane's sequence block advanced, the completion word raised.
__device__ __forceinline__ void table_end(const TableRt &rt, uint64_t epochs, uint64_t rounds, uint64_t os) {
    if (rt.dseq) dseq_advance(rt.dseq, epochs, rounds, os);
    block_done(rt.done);
}

// One-shot, after the wait: slot [j] of my arena to recv + roff[j], as vectors [vb, ve) or, from
// workgroup 0, byte by byte.
template <class Args>
__device__ __forceinline__ void slot_to_recv(const Args &a, int j, int blk, size_t poff, size_t vb, size_t ve) {
    const char *slot = a.rt.arena_own + poff + (size_t)j * a.rt.slot_bytes;
    char *dst = a.recv + a.roff[j];
    const size_t len = a.rlen[j];
    if (a.rt.nvec) {
        const size_t nv = len >> 4, e = ve < nv ? ve : nv;
        for (size_t i = vb + threadIdx.x; i < e; i += kThreads) ((v4u *)dst)[i] = ld_nt((const v4u *)slot + i);
    } else if (blk == 0) {
        for (size_t i = threadIdx.x; i < len; i += kThreads) dst[i] = __builtin_nontemporal_load(slot + i);
    }
}

// Pipelined, round k: the slot parity, the flag epoch and where workgroup b's range starts.
struct PipeRound {
    uint64_t par, E;
    size_t rbase;
};
__device__ __forceinline__ PipeRound pipe_round(const TableRt &rt, const TableCall &c, int k, size_t so) {
    return PipeRound{(c.round0 + (uint64_t)k) & 1, c.epoch + 2 * (uint64_t)k, (size_t)k * rt.tseg + so};
}

// ---------------------------------------------------------------------------
// One-shot kernel.  Rank me pushes block j of its send buffer into slot [me] of rank j's one-shot
// arena (this call's half) and copies its own block locally, raises its flag to every peer, waits
// for every peer's flag, and copies slot [j] to recv + roff[j] for every j != me.  Every rank
// raises and awaits every flag, whatever the pair lengths, so that no rank can reach call i + 2
// while a peer still reads call i's half (the one-shot allreduce's argument).
// nvec > 0: every offset and length is a multiple of 16 and workgroup b moves vectors
// [b * per, (b + 1) * per) of every block; nvec == 0: workgroup 0 moves every block byte by byte.
// MPI_IN_PLACE (send == recv, soff == roff): a workgroup overwrites in its gather only the ranges
// it read in its push, and signal_peers' workgroup barrier stands between the two.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_oneshot_a2a(A2AArgs a) {
    const int blk = blockIdx.x, G = gridDim.x;
    const size_t per = (a.rt.nvec + G - 1) / G;
    const size_t vb = (size_t)blk * per, ve = vb + per;
    const TableCall c = table_call(a.rt);
    const size_t myslot = c.poff + (size_t)a.me * a.rt.slot_bytes;
#pragma unroll
    for (int j = 0; j < kMaxRanks; ++j) {
        if (j >= a.n) continue;
        const char *src = a.send + a.soff[j];
        char *dst = j == a.me ? a.recv + a.roff[j] : a.rt.arena_peer.p[j] + myslot;
        if (src == dst) continue;  // in place: my own block stays where it is
        const size_t len = a.slen[j];
        if (a.rt.nvec) {
            const size_t nv = len >> 4, e = ve < nv ? ve : nv;
            for (size_t i = vb + threadIdx.x; i < e; i += kThreads) ((v4u *)dst)[i] = ((const v4u *)src)[i];
        } else if (blk == 0) {
            for (size_t i = threadIdx.x; i < len; i += kThreads) dst[i] = src[i];
        }
    }
    signal_peers(a.rt.sig_peer, a.n, a.me, blk, c.epoch, a.rt.light != 0);
    if (wait_peers(a.rt.sig_own, a.n, blk, c.epoch, a.rt.err, a.rt.timeout, a.rt.light != 0)) {
#pragma unroll
        for (int j = 0; j < kMaxRanks; ++j)
            if (j < a.n && j != a.me) slot_to_recv(a, j, blk, c.poff, vb, ve);
    }
    table_end(a.rt, 1, 0, 1);
}

// ---------------------------------------------------------------------------
// The shifted copy: source and destination differ modulo 16 (both on this GPU).
// ---------------------------------------------------------------------------

// Bytes [sh + 4i, sh + 4i + 4) for i = 0..3 of the 32-byte stream w[0..7] (little-endian words),
// sh = 4 * Q + r: word i of the result is the 64-bit pair (w[Q+i+1] : w[Q+i]) shifted right by r
// bytes.  Q is a template parameter so that every register index is a compile-time constant.
template <int Q>
__device__ __forceinline__ v4u funnel16(const v4u lo, const v4u hi, unsigned r) {
    const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    v4u o;
    o.x = __builtin_amdgcn_alignbyte(w[Q + 1], w[Q + 0], r);
    o.y = __builtin_amdgcn_alignbyte(w[Q + 2], w[Q + 1], r);
    o.z = __builtin_amdgcn_alignbyte(w[Q + 3], w[Q + 2], r);
    o.w = __builtin_amdgcn_alignbyte(w[Q + 4], w[Q + 3], r);
    return o;
}

// Block-wide copy of len bytes from src to dst, (src - dst) % 16 != 0.  A scalar head brings dst
// to a 16-byte boundary; from there every store is a whole vector on a 16-byte address, built from
// the two 16-byte-aligned source vectors it straddles.  Lane l of a wave loads aligned source vector x
// once and takes vector x + 1 from lane l + 1; only a wave's last lane loads a second one, so
// the source is read 65/64 times, not twice.  Every aligned load holds at least one byte of
// [src, src + len): it stays inside the page, and inside the arena slot, of a byte that is there.
__device__ __forceinline__ void copy_shift_one(const char *src, char *dst, size_t len) {
    const size_t h0 = (16 - ((uintptr_t)dst & 15)) & 15;
    const size_t h = h0 < len ? h0 : len;
    if (threadIdx.x < h) dst[threadIdx.x] = __builtin_nontemporal_load(src + threadIdx.x);
    const char *s = src + h;
    const size_t nv = (len - h) >> 4;
    const unsigned sh = (unsigned)((uintptr_t)s & 15);  // 1..15
    const v4u *sa = (const v4u *)(s - sh);
    v4u *d = (v4u *)(dst + h);
    const unsigned lane = threadIdx.x & 63u, q = sh >> 2, r = sh & 3u;
    for (size_t x = threadIdx.x; x - lane < nv; x += kPipeThreads) {
        // x == nv: vector nv holds the last sh bytes that vector nv - 1 of the destination needs
        v4u lo = v4u{0, 0, 0, 0};
        if (x <= nv) lo = ld_nt(sa + x);
        v4u hi;
        hi.x = __shfl_down(lo.x, 1);
        hi.y = __shfl_down(lo.y, 1);
        hi.z = __shfl_down(lo.z, 1);
        hi.w = __shfl_down(lo.w, 1);
        if (lane == 63u && x < nv) hi = ld_nt(sa + x + 1);
        if (x < nv) {
            v4u o;
            if (q == 0) o = funnel16<0>(lo, hi, r);
            else if (q == 1) o = funnel16<1>(lo, hi, r);
            else if (q == 2) o = funnel16<2>(lo, hi, r);
            else o = funnel16<3>(lo, hi, r);
            d[x] = o;
        }
    }
    const size_t t0 = h + (nv << 4);
    if (t0 + threadIdx.x < len) dst[t0 + threadIdx.x] = __builtin_nontemporal_load(src + t0 + threadIdx.x);
}

// Block-wide: every job of non-zero length, one after the other.  The table lives in LDS because
// the loop over jobs indexes it at run time (private arrays indexed so would go to scratch).
struct ShiftJob {
    const char *src;
    char *dst;
    size_t len;
};
__device__ __forceinline__ void blk_copy_shift(const Jobs &jb) {
    __shared__ ShiftJob t[kMaxRanks];
    __syncthreads();  // previous users of the table are done
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < kMaxRanks; ++j) t[j] = ShiftJob{jb.src[j], jb.dst[j], jb.len[j]};
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < kMaxRanks; ++j) {
        const size_t len = t[j].len;
        if (len) copy_shift_one(t[j].src, t[j].dst, len);
    }
}

// Local copies of any relative alignment: the jobs whose two ends agree modulo 16 through the
// equal-alignment copy, the others through the shifted one.
__device__ __forceinline__ void blk_copy_local(const Jobs &jb) {
    Jobs eq = jb, sh = jb;
    bool any_eq = false, any_sh = false;
#pragma unroll
    for (int j = 0; j < kMaxRanks; ++j) {
        const bool same = (((uintptr_t)jb.src[j] ^ (uintptr_t)jb.dst[j]) & 15) == 0;
        eq.len[j] = same ? jb.len[j] : 0;
        sh.len[j] = same ? 0 : jb.len[j];
        any_eq |= eq.len[j] != 0;
        any_sh |= sh.len[j] != 0;
    }
    if (any_eq) blk_copy_jobs<true>(eq);
    if (any_sh) blk_copy_shift(sh);
}

// ---------------------------------------------------------------------------
// Pipelined kernel: k_pipe's tiling (workgroup b owns [k * tseg + b * tsub, + tsub) of every block
// in round k), its slot parities (round k uses parity (round0 + k) & 1 of the AG region) and its
// flags (round k raises and awaits epoch0 + 2k; the odd epochs stay unused, as in PIPE_AG, so a
// call takes the 2 * nrounds epochs every pipelined call takes).  Round k:
//   push   : my range of block j -> pslot(rank j's AG region, par, me) + b * tsub + (soff[j] & 15)
//            for every j != me; my own block's range straight to recv
//   E(k)   : signal every peer, wait for every peer
//   gather : slot [par][j] + b * tsub + smis[j] -> recv + roff[j] + range, shifted where the two
//            differ modulo 16
// A range is at most tsub bytes at b * tsub + (0..15) and tsub is a multiple of 4 KiB, so the
// ranges of a slot do not overlap and end inside the slot stride's spare 256 bytes.
//
// Slot reuse (coll/pipe.h header).  Rank w writes rank o's parity-p slot [w] in round k + 2 only
// after its wait in round k + 1 saw o's flag E(k+1); o raises E(k+1) after its push of round
// k + 1, which follows, in program order and behind signal_peers' vmcnt(0) and workgroup barrier,
// its gather of round k -- the last read of that slot.  Across calls: w leaves a call only after
// its last wait saw o's E(K-1), raised after o's gather of round K - 2; the next call's first
// round writes the parity of round K - 2 (the other parity is still being read) and its second
// round waits for a flag o raises inside that next call.  Every rank runs the same number of
// rounds (the runtime derives it from the job-wide longest pair) and raises every flag, pairs of
// length 0 included.
//
// MPI_IN_PLACE (send == recv, soff == roff): the kernel reads its round's ranges of every block
// from recv in the push before its gather overwrites the same ranges; workgroup b touches only
// its own ranges, so the workgroup barrier inside signal_peers, between push and gather, is
// required and sufficient.
// ---------------------------------------------------------------------------
__device__ __forceinline__ size_t a2a_range(size_t len, size_t rbase, size_t tsub) {
    return rbase < len ? (len - rbase < tsub ? len - rbase : tsub) : 0;
}

__global__ __launch_bounds__(kPipeThreads) void k_pipe_a2a(A2AArgs a) {
    const TableCall c = table_call(a.rt);
    const int b = blockIdx.x, n = a.n, me = a.me;
    const unsigned all = (1u << n) - 1u;
    const size_t so = (size_t)b * a.rt.tsub;
    for (int k = 0; k < a.rt.nrounds; ++k) {
        const PipeRound r = pipe_round(a.rt, c, k, so);
        {
            Jobs jb{}, own{};
#pragma unroll
            for (int j = 0; j < kMaxRanks; ++j) {
                if (j >= n) continue;
                const char *src = a.send + a.soff[j] + r.rbase;
                const size_t len = a2a_range(a.slen[j], r.rbase, a.rt.tsub);
                if (j != me) {
                    jb.src[j] = src;
                    jb.dst[j] = pslot(a.rt.ag_peer.p[j], r.par, me) + so + (a.soff[j] & 15);
                    jb.len[j] = len;
                } else if (src != a.recv + a.roff[j] + r.rbase) {
                    own.src[j] = src;
                    own.dst[j] = a.recv + a.roff[j] + r.rbase;
                    own.len[j] = len;
                }
            }
            blk_copy_jobs<false>(jb, a.rt.rnt != 0);
            blk_copy_local(own);
        }
        signal_peers(a.rt.sig_peer, n, me, b, r.E, a.rt.light != 0);
        if (!wait_mask(a.rt.sig_own, all, b, r.E, a.rt.err, a.rt.timeout, a.rt.light != 0)) break;
        Jobs g{};
#pragma unroll
        for (int j = 0; j < kMaxRanks; ++j) {
            if (j < n && j != me) {
                g.src[j] = pslot(a.rt.ag_peer.p[me], r.par, j) + so + a.smis[j];
                g.dst[j] = a.recv + a.roff[j] + r.rbase;
                g.len[j] = a2a_range(a.rlen[j], r.rbase, a.rt.tsub);
            }
        }
        blk_copy_local(g);
    }
    table_end(a.rt, 2 * (uint64_t)a.rt.nrounds, (uint64_t)a.rt.nrounds, 0);
}

// ---------------------------------------------------------------------------
// MPI_Allgatherv / MPI_Gather: every rank has one block, and it goes to a set of ranks (dmask:
// all of them, or the root alone).  Through the table above an allgatherv push would be n - 1
// jobs that each read the same source range again; here a vector is loaded once and stored to
// every masked destination (PIPE_AG's blk_copy_multi).  The source is 16-byte aligned (the runtime
// stages anything else), so a block lies in slot [me] of every destination's arena at
// misalignment 0, every store into a peer is a whole aligned vector and no misalignment has to be
// exchanged; the receiver's gather shifts where its own destination is off a 16-byte boundary.
//
// Flags, epochs, arena halves and slot parities are the kernels' above, and the reuse argument
// with them: every rank raises and awaits every flag in every round, whatever its mask and
// lengths, because passing a wait has to prove that every peer has left the previous call --
// which may have been any other collective.
// ---------------------------------------------------------------------------

// One-shot: nvec > 0: every length is a multiple of 16, send, recv and every roff are 16-byte
// aligned, and workgroup b moves vectors [b * per, (b + 1) * per) of every block; nvec == 0:
// workgroup 0 moves every block byte by byte (any address).
__global__ __launch_bounds__(kThreads) void k_oneshot_gv(GvArgs a) {
    const int blk = blockIdx.x, G = gridDim.x;
    const size_t per = (a.rt.nvec + G - 1) / G;
    const size_t vb = (size_t)blk * per, ve = vb + per;
    const TableCall c = table_call(a.rt);
    const size_t myslot = c.poff + (size_t)a.me * a.rt.slot_bytes;
    // the own bit: also to my own recv + roff[me], unless the block is already there
    char *own = a.recv + a.roff[a.me];
    if (!((a.dmask >> a.me) & 1u) || own == a.send) own = nullptr;
    const unsigned peers = a.dmask & ~(1u << a.me);
    if (peers || own) {
        if (a.rt.nvec) {
            const size_t nv = a.slen >> 4, e = ve < nv ? ve : nv;
            for (size_t i = vb + threadIdx.x; i < e; i += kThreads) {
                const v4u v = ((const v4u *)a.send)[i];
#pragma unroll
                for (int j = 0; j < kMaxRanks; ++j)
                    if (j < a.n && ((peers >> j) & 1u)) ((v4u *)(a.rt.arena_peer.p[j] + myslot))[i] = v;
                if (own) ((v4u *)own)[i] = v;
            }
        } else if (blk == 0) {
            for (size_t i = threadIdx.x; i < a.slen; i += kThreads) {
                const char ch = a.send[i];
#pragma unroll
                for (int j = 0; j < kMaxRanks; ++j)
                    if (j < a.n && ((peers >> j) & 1u)) (a.rt.arena_peer.p[j] + myslot)[i] = ch;
                if (own) own[i] = ch;
            }
        }
    }
    signal_peers(a.rt.sig_peer, a.n, a.me, blk, c.epoch, a.rt.light != 0);
    if (wait_peers(a.rt.sig_own, a.n, blk, c.epoch, a.rt.err, a.rt.timeout, a.rt.light != 0)) {
#pragma unroll
        for (int j = 0; j < kMaxRanks; ++j)
            if (j < a.n && j != a.me) slot_to_recv(a, j, blk, c.poff, vb, ve);
    }
    table_end(a.rt, 1, 0, 1);
}

// Pipelined: k_pipe_a2a's tiling, parities and flags.  Round k:
//   push   : my round's range -> pslot(rank j's AG region, par, me) + b * tsub for every masked
//            j != me and, with the own bit, to recv + roff[me], in one blk_copy_multi (the own
//            destination apart, shifted, where it is off a 16-byte boundary)
//   E(k)   : signal every peer, wait for every peer
//   gather : slot [par][j] + b * tsub -> recv + roff[j] + range, shifted where that is off a
//            16-byte boundary
__global__ __launch_bounds__(kPipeThreads) void k_pipe_gv(GvArgs a) {
    const TableCall c = table_call(a.rt);
    const int b = blockIdx.x, n = a.n, me = a.me;
    const unsigned all = (1u << n) - 1u;
    const unsigned peers = a.dmask & ~(1u << me);
    const size_t so = (size_t)b * a.rt.tsub;
    char *own = a.recv + a.roff[me];
    if (!((a.dmask >> me) & 1u) || own == a.send) own = nullptr;
    for (int k = 0; k < a.rt.nrounds; ++k) {
        const PipeRound r = pipe_round(a.rt, c, k, so);
        const size_t len = a2a_range(a.slen, r.rbase, a.rt.tsub);
        if (len && (peers || own)) {
            const bool own_eq = own && ((uintptr_t)own & 15) == 0;
            Dsts d{};
#pragma unroll
            for (int j = 0; j < kMaxRanks; ++j)
                if (j < n && ((peers >> j) & 1u)) d.p[j] = pslot(a.rt.ag_peer.p[j], r.par, me) + so;
            if (own_eq) d.p[kMaxRanks] = own + r.rbase;
            if (peers || own_eq) blk_copy_multi(d, a.send + r.rbase, len, a.rt.rnt != 0);
            if (own && !own_eq) {
                Jobs o{};
                o.src[0] = a.send + r.rbase;
                o.dst[0] = own + r.rbase;
                o.len[0] = len;
                blk_copy_shift(o);
            }
        }
        signal_peers(a.rt.sig_peer, n, me, b, r.E, a.rt.light != 0);
        if (!wait_mask(a.rt.sig_own, all, b, r.E, a.rt.err, a.rt.timeout, a.rt.light != 0)) break;
        Jobs g{};
#pragma unroll
        for (int j = 0; j < kMaxRanks; ++j) {
            if (j < n && j != me) {
                g.src[j] = pslot(a.rt.ag_peer.p[me], r.par, j) + so;
                g.dst[j] = a.recv + a.roff[j] + r.rbase;
                g.len[j] = a2a_range(a.rlen[j], r.rbase, a.rt.tsub);
            }
        }
        blk_copy_local(g);
    }
    table_end(a.rt, 2 * (uint64_t)a.rt.nrounds, (uint64_t)a.rt.nrounds, 0);
}

// Launchers.  A one-shot kernel runs on at most its resident grid: the flags pair workgroup b of
// every rank, so every workgroup of the grid has to be running.
template <class Args>
static int launch_table(void (*k)(Args), const Args &a, int grid, int threads, hipStream_t st) {
    hipLaunchKernelGGL(k, dim3(grid), dim3(threads), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : E_INTERN;
}
int launch_oneshot_a2a(const A2AArgs &a, const LaunchCfg &cfg) {
    static const int cap = resident_grid((const void *)k_oneshot_a2a, cfg);
    return launch_table(k_oneshot_a2a, a, cfg.grid < cap ? cfg.grid : cap, kThreads, cfg.stream);
}
int launch_oneshot_gv(const GvArgs &a, const LaunchCfg &cfg) {
    static const int cap = resident_grid((const void *)k_oneshot_gv, cfg);
    return launch_table(k_oneshot_gv, a, cfg.grid < cap ? cfg.grid : cap, kThreads, cfg.stream);
}
int launch_pipe_a2a(const A2AArgs &a, const LaunchCfg &cfg) {
    return launch_table(k_pipe_a2a, a, cfg.grid, kPipeThreads, cfg.stream);
}
int launch_pipe_gv(const GvArgs &a, const LaunchCfg &cfg) {
    return launch_table(k_pipe_gv, a, cfg.grid, kPipeThreads, cfg.stream);
}

}  // namespace mv2

// coll_mn.cpp — the collectives of a job on several nodes.
//
// Several nodes: MVAPICH2's two-level structure, node step on the device
// kernels of coll_node.cpp (this process's world is its node), inter-node step between the
// node leaders (local rank 0) over internode.cpp's links with host staging; every
// reduction stays a device kernel (mv2h_reduce_local: the reference's uop(tmp, recv)).
//   Allreduce = MPIR_Allreduce_two_level_MV2 (allreduce_osu.c:1687): node reduction
//     (the node's own allreduce: the degree-4 tree up to 2 KiB / shmem LINEAR, the
//     reference's intra step of its topology-aware and skip-small paths, :2272, :118-160),
//     recursive doubling among the leaders (MPIR_Allreduce_pt2pt_rd_MV2 :360-630, the
//     inter step of both paths, :2215-2262), node broadcast.
//   Bcast = node broadcast at the root's node, binomial over the leaders, node broadcast.
//   Reduce = node reduce to the leader, binomial reduce over the leaders to the root's node
//     (MPIR_Reduce_binomial_MV2 reduce_osu.c:425, commutative form), leader -> root.
//   Allgather = node allgather into the node's section, ring over the leaders, node bcast.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../../include/mv2h.h"
#include "coll_internal.h"
#include "internode.h"
#include "log.h"
#include "pvars.h"

namespace mv2 {

// leaders: allgather of one section of `sect` bytes per node in the host buffer h (this node's at
// h + node * sect), as a ring: step k passes node (node - k)'s section to the right
static int leader_ring_sections(char *h, size_t sect) {
    World &w = world();
    const int K = w.nnodes, me = w.node, right = (me + 1) % K, left = (me - 1 + K) % K;
    int rc = 0;
    for (int k = 0; k < K - 1 && !rc; ++k) {
        const int so = (me - k + K) % K, ro = (me - k - 1 + K) % K;
        rc = net_shift(right, h + (size_t)so * sect, sect, left, h + (size_t)ro * sect, sect);
    }
    return rc;
}

// dst = the programs `ps` over n operands of `count` elements, operand r at W + r * S (device)
static int reduce_gathered(const char *W, int n, size_t S, void *dst, size_t count, int dtype, int op,
                           const ProgSet &ps) {
    const void *srcs[kMaxRanks];
    for (int r = 0; r < n; ++r) srcs[r] = W + (size_t)r * S;
    return mv2h_reduce_n_prog(srcs, n, dst, count, dtype, op, (const mv2h_progset *)&ps, nullptr);
}

// C linkage, as before this file was split from coll.cpp: the names of this unnamed namespace stay
// in the library's dynamic symbol table, which the split leaves as it was.
extern "C" {
namespace {
struct MnBufs {
    char *h0 = nullptr, *h1 = nullptr;  // pinned host staging
    size_t hcap = 0;
    char *d0 = nullptr, *d1 = nullptr;  // device: leader partial / received operand
    size_t dcap = 0;
};
MnBufs g_mn;

// host staging h0 / h1 (node leaders: the inter-node messages) and device d0 / d1
int mn_reserve_host(size_t bytes) {
    if (bytes > g_mn.hcap) {
        if (g_mn.h0) hipHostFree(g_mn.h0);
        if (g_mn.h1) hipHostFree(g_mn.h1);
        g_mn.h0 = g_mn.h1 = nullptr;
        g_mn.hcap = 0;
        if (hipHostMalloc((void **)&g_mn.h0, bytes, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void **)&g_mn.h1, bytes, hipHostMallocDefault) != hipSuccess)
            return E_NO_MEM;
        g_mn.hcap = bytes;
    }
    return 0;
}
int mn_reserve_dev(size_t bytes) {
    if (bytes > g_mn.dcap) {
        hipDeviceSynchronize();
        if (g_mn.d0) hipFree(g_mn.d0);
        if (g_mn.d1) hipFree(g_mn.d1);
        g_mn.d0 = g_mn.d1 = nullptr;
        g_mn.dcap = 0;
        if (hipMalloc((void **)&g_mn.d0, bytes) != hipSuccess || hipMalloc((void **)&g_mn.d1, bytes) != hipSuccess)
            return E_NO_MEM;
        g_mn.dcap = bytes;
    }
    return 0;
}
int mn_reserve(size_t bytes) {
    const int rc = mn_reserve_host(bytes);
    return rc ? rc : mn_reserve_dev(bytes);
}

int mn_d2h(void *h, const void *d, size_t b) { return hipMemcpy(h, d, b, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN; }
int mn_h2d(void *d, const void *h, size_t b) { return hipMemcpy(d, h, b, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN; }

// The message schedules of MPIR_Allreduce_pt2pt_rd_MV2 (allreduce_osu.c:455-600) and
// MPIR_Allreduce_pt2pt_rs_MV2 (:740-1054: recursive doubling for count < pof2, :802) run as
// messages over n ranks, this one `rank`.  acc (device, count elements of ext bytes) holds the
// operand and ends with the result; tmp (device, as large) receives.  x.xchg(peer, sb, sbytes, rb,
// rbytes) sends and receives (either side may be empty).  Every uop(tmp, recvbuf) is one device
// Reduce_local; builtin ops only (commutative, so recursive doubling never swaps its operands).
struct Xport {
    // send sbytes of sb to `to` while receiving rbytes into rb from `from` (either side may be empty)
    virtual int shift(int to, const char *sb, size_t sbytes, int from, char *rb, size_t rbytes) = 0;
    int xchg(int peer, const char *sb, size_t sbytes, char *rb, size_t rbytes) {
        return shift(peer, sb, sbytes, peer, rb, rbytes);
    }
};
// redscat: the pre-step of MPIR_Reduce_redscat_gather_MV2 (reduce_osu.c:849-894) instead — the odd
// ranks below 2 * rem hand their operand to rank - 1 — with the allgather standing for its gather
// to the root and the broadcast after it (MPI_Iallreduce's naive schedule moves the blocks only).
int sched_allreduce(Xport &x, int n, int rank, char *acc, char *tmp, size_t count, size_t ext, int dtype, int op,
                    bool rd, bool redscat = false) {
    const int pof2 = floor_pof2(n);
    const int rem = n - pof2;
    const size_t S = count * ext;
    int rc = 0, newrank;
    auto uop = [&](size_t off, size_t cnt) { return mv2h_reduce_local(tmp + off, acc + off, cnt, dtype, op, nullptr); };
    // non-power-of-two pre-step: even ranks below 2 * rem hand their operand to rank + 1 (redscat:
    // the odd ones to rank - 1)
    const int hand = redscat ? 1 : 0, keep = 1 - hand;
    if (rank < 2 * rem) {
        if (rank % 2 == hand) {
            if ((rc = x.xchg(hand ? rank - 1 : rank + 1, acc, S, nullptr, 0))) return rc;
            newrank = -1;
        } else {
            if ((rc = x.xchg(hand ? rank + 1 : rank - 1, nullptr, 0, tmp, S)) || (rc = uop(0, count))) return rc;
            newrank = rank / 2;
        }
    } else {
        newrank = rank - rem;
    }
    auto real = [&](int nr) { return nr < rem ? nr * 2 + keep : nr + rem; };
    if (newrank != -1 && (rd || count < (size_t)pof2)) {
        for (int mask = 1; mask < pof2; mask <<= 1) {
            if ((rc = x.xchg(real(newrank ^ mask), acc, S, tmp, S)) || (rc = uop(0, count))) return rc;
        }
    } else if (newrank != -1) {
        // reduce-scatter by recursive halving over pof2 blocks (the last one takes the remainder),
        // then the recursive-doubling allgather
        std::vector<size_t> cnts((size_t)pof2, count / (size_t)pof2), disps((size_t)pof2, 0);
        cnts[(size_t)pof2 - 1] = count - (count / (size_t)pof2) * (size_t)(pof2 - 1);
        for (int i = 1; i < pof2; ++i) disps[i] = disps[i - 1] + cnts[i - 1];
        auto span = [&](int a, int b) { return a < b ? disps[b - 1] + cnts[b - 1] - disps[a] : (size_t)0; };
        int mask = 1, send_idx = 0, recv_idx = 0, last_idx = pof2;
        while (mask < pof2) {
            const int newdst = newrank ^ mask;
            size_t scnt, rcnt;
            if (newrank < newdst) {
                send_idx = recv_idx + pof2 / (mask * 2);
                scnt = span(send_idx, last_idx);
                rcnt = span(recv_idx, send_idx);
            } else {
                recv_idx = send_idx + pof2 / (mask * 2);
                scnt = span(send_idx, recv_idx);
                rcnt = span(recv_idx, last_idx);
            }
            const size_t so = disps[send_idx] * ext, ro = disps[recv_idx] * ext;
            if ((rc = x.xchg(real(newdst), acc + so, scnt * ext, tmp + ro, rcnt * ext)) || (rc = uop(ro, rcnt)))
                return rc;
            send_idx = recv_idx;
            mask <<= 1;
            if (mask < pof2) last_idx = recv_idx + pof2 / mask;
        }
        for (mask >>= 1; mask > 0; mask >>= 1) {
            const int newdst = newrank ^ mask;
            size_t scnt, rcnt;
            if (newrank < newdst) {
                if (mask != pof2 / 2) last_idx = last_idx + pof2 / (mask * 2);
                recv_idx = send_idx + pof2 / (mask * 2);
                scnt = span(send_idx, recv_idx);
                rcnt = span(recv_idx, last_idx);
            } else {
                recv_idx = send_idx - pof2 / (mask * 2);
                scnt = span(send_idx, last_idx);
                rcnt = span(recv_idx, send_idx);
            }
            if ((rc = x.xchg(real(newdst), acc + disps[send_idx] * ext, scnt * ext, acc + disps[recv_idx] * ext,
                             rcnt * ext)))
                return rc;
            if (newrank > newdst) send_idx = recv_idx;
        }
    }
    // post-step: the ranks that kept their place below 2 * rem return the result to the others
    if (rank < 2 * rem) {
        const int peer = rank % 2 ? rank - 1 : rank + 1;
        rc = rank % 2 == keep ? x.xchg(peer, acc, S, nullptr, 0) : x.xchg(peer, nullptr, 0, acc, S);
    }
    return rc;
}

// MPIR_Reduce_binomial_MV2's commutative schedule (reduce_osu.c:577-663; MPIR_Ireduce_binomial
// reduces the same way): relative rank rel receives from rel | mask and reduces uop(tmp, acc)
// until its bit `mask` is set, then sends its partial to rel & ~mask.  acc ends with the result
// at the root.
int sched_binomial_reduce(Xport &x, int n, int rank, int root, char *acc, char *tmp, size_t count, size_t ext,
                          int dtype, int op) {
    const int rel = (rank - root + n) % n;
    const size_t S = count * ext;
    int rc = 0;
    for (int mask = 1; mask < n; mask <<= 1) {
        if (rel & mask) return x.xchg(((rel & ~mask) + root) % n, acc, S, nullptr, 0);
        if ((rel | mask) < n && ((rc = x.xchg(((rel | mask) + root) % n, nullptr, 0, tmp, S)) ||
                                 (rc = mv2h_reduce_local(tmp, acc, count, dtype, op, nullptr))))
            return rc;
    }
    return 0;
}

// MPIR_Reduce_knomial_MV2 (reduce_osu.c:1639-1837) as messages: the children of
// MPIR_Reduce_knomial_trace (:1568-1633: k - 1 per mask, masks from the largest down) send their
// partials; the receives are posted from the trace's last child to its first (:1735-1741) and
// reduced uop(tmp, acc) in request-index order (the Waitany order restated), then the
// partial goes to the parent.  acc ends with the result at the root (commutative ops only, as in
// the reference's dispatch, :2637-2644).
int sched_knomial_reduce(Xport &x, int n, int rank, int root, int k, char *acc, char *tmp, size_t count, size_t ext,
                         int dtype, int op) {
    const int rel = (rank - root + n) % n;
    const size_t S = count * ext;
    int mask = 1, dst = -1;
    while (mask < n) {
        if (rel % (k * mask)) {
            dst = rel / (k * mask) * (k * mask) + root;
            if (dst >= n) dst -= n;
            break;
        }
        mask *= k;
    }
    mask /= k;
    std::vector<int> src;
    for (int m = mask; m > 0; m /= k)
        for (int j = 1; j < k; ++j)
            if (rel + m * j < n) src.push_back(rank + m * j >= n ? rank + m * j - n : rank + m * j);
    int rc = 0;
    for (size_t i = src.size(); i-- > 0;)
        if ((rc = x.xchg(src[i], nullptr, 0, tmp, S)) || (rc = mv2h_reduce_local(tmp, acc, count, dtype, op, nullptr)))
            return rc;
    return dst >= 0 ? x.xchg(dst, acc, S, nullptr, 0) : 0;
}

// the node leaders as ranks (node index), over their TCP links, staged through g_mn.h0 / h1
struct LeaderLinks : Xport {
    int shift(int to, const char *sb, size_t sbytes, int from, char *rb, size_t rbytes) override {
        int rc = 0;
        if (sbytes && (rc = mn_d2h(g_mn.h0, sb, sbytes))) return rc;
        if (sbytes && rbytes) rc = net_shift(to, g_mn.h0, sbytes, from, g_mn.h1, rbytes);
        else if (sbytes) rc = net_send(to, g_mn.h0, sbytes);
        else if (rbytes) rc = net_recv(from, g_mn.h1, rbytes);
        return rc || !rbytes ? rc : mn_h2d(rb, g_mn.h1, rbytes);
    }
};

// every rank of the job (global rank), over the point-to-point channels in the library's
// collective context: device IPC within a node, the rank mesh between nodes
struct RankChannels : Xport {
    int shift(int to, const char *sb, size_t sbytes, int from, char *rb, size_t rbytes) override {
        unsigned long long sq = 0, rq = 0;
        int rc = 0;
        if (rbytes && (rc = p2p_irecv(rb, rbytes, from, kCollTagBase - 3, &rq))) return rc;
        if (sbytes && (rc = p2p_isend(sb, sbytes, to, kCollTagBase - 3, &sq))) {
            if (rq) p2p_abandon(rq);  // withdrawn, or the context poisoned: never matched into later
            return rc;
        }
        if (sbytes && (rc = mv2h_p2p_wait(sq, nullptr, nullptr, nullptr))) {
            p2p_abandon(sq);
            if (rq) p2p_abandon(rq);
            return rc;
        }
        if (rbytes && (rc = mv2h_p2p_wait(rq, nullptr, nullptr, nullptr))) p2p_abandon(rq);
        return rc;
    }
};

// MPI_Reduce_scatter's message schedules over n ranks (commutative ops, every uop one device
// Reduce_local of the received data `in` into this rank's accumulator `inout`).  in: this rank's
// whole operand (device, total elements, block j at disps[j]); out: its block (cnts[rank]
// elements, device or host); t0 / t1: device scratch of the whole operand.
//
// MPIR_Reduce_scatter_Rec_Halving_MV2 (red_scat_osu.c:428-780): the non-power-of-two pre-step,
// recursive halving over pof2 merged blocks (an odd rank below 2 * rem also works its left
// neighbour's block), the post-step returning the even ranks' blocks.
int sched_rs_halving(Xport &x, int n, int rank, const size_t *cnts, const size_t *disps, const char *in, char *out,
                     char *t0, char *t1, size_t ext, int dtype, int op) {
    const size_t total = disps[n - 1] + cnts[n - 1], S = total * ext;
    char *res = t0, *tmp = t1;  // tmp_results, tmp_recvbuf
    if (hipMemcpy(res, in, S, hipMemcpyDefault) != hipSuccess) return E_INTERN;
    const int pof2 = floor_pof2(n);
    const int rem = n - pof2;
    int rc = 0, newrank;
    if (rank < 2 * rem) {
        if (rank % 2 == 0) {
            if ((rc = x.xchg(rank + 1, res, S, nullptr, 0))) return rc;
            newrank = -1;
        } else {
            if ((rc = x.xchg(rank - 1, nullptr, 0, tmp, S)) ||
                (rc = mv2h_reduce_local(tmp, res, total, dtype, op, nullptr)))
                return rc;
            newrank = rank / 2;
        }
    } else {
        newrank = rank - rem;
    }
    auto real = [&](int nr) { return nr < rem ? nr * 2 + 1 : nr + rem; };
    if (newrank != -1) {
        std::vector<size_t> ncnt((size_t)pof2), ndisp((size_t)pof2, 0);
        for (int i = 0; i < pof2; ++i) {
            const int old = real(i);
            ncnt[i] = cnts[old] + (old < 2 * rem ? cnts[old - 1] : 0);
        }
        for (int i = 1; i < pof2; ++i) ndisp[i] = ndisp[i - 1] + ncnt[i - 1];
        auto span = [&](int a, int b) {
            size_t c = 0;
            for (int i = a; i < b; ++i) c += ncnt[i];
            return c;
        };
        int send_idx = 0, recv_idx = 0, last_idx = pof2;
        for (int mask = pof2 >> 1; mask > 0; mask >>= 1) {
            const int newdst = newrank ^ mask;
            size_t scnt, rcnt;
            if (newrank < newdst) {
                send_idx = recv_idx + mask;
                scnt = span(send_idx, last_idx);
                rcnt = span(recv_idx, send_idx);
            } else {
                recv_idx = send_idx + mask;
                scnt = span(send_idx, recv_idx);
                rcnt = span(recv_idx, last_idx);
            }
            const size_t so = ndisp[send_idx] * ext, ro = ndisp[recv_idx] * ext;
            if ((rc = x.xchg(real(newdst), res + so, scnt * ext, tmp + ro, rcnt * ext))) return rc;
            if (rcnt && (rc = mv2h_reduce_local(tmp + ro, res + ro, rcnt, dtype, op, nullptr))) return rc;
            send_idx = recv_idx;
            last_idx = recv_idx + mask;
        }
        if (cnts[rank] &&
            hipMemcpy(out, res + disps[rank] * ext, cnts[rank] * ext, hipMemcpyDefault) != hipSuccess)
            return E_INTERN;
    }
    if (rank < 2 * rem) {
        if (rank % 2) rc = x.xchg(rank - 1, res + disps[rank - 1] * ext, cnts[rank - 1] * ext, nullptr, 0);
        else if (is_device(out)) rc = x.xchg(rank + 1, nullptr, 0, out, cnts[rank] * ext);
        else if (!(rc = x.xchg(rank + 1, nullptr, 0, tmp, cnts[rank] * ext)) && cnts[rank])
            rc = hipMemcpy(out, tmp, cnts[rank] * ext, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN;
    }
    return rc;
}

// MPIR_Reduce_scatter_Pair_Wise_MV2 (:786-1020): this rank's block starts as its own data; step i
// sends block (rank + i) to that rank and reduces the block received from rank - i into it
int sched_rs_pairwise(Xport &x, int n, int rank, const size_t *cnts, const size_t *disps, const char *in, char *out,
                      char *t0, char *t1, size_t ext, int dtype, int op) {
    const size_t B = cnts[rank] * ext;
    if (B && hipMemcpy(t0, in + disps[rank] * ext, B, hipMemcpyDefault) != hipSuccess) return E_INTERN;
    int rc = 0;
    for (int i = 1; i < n; ++i) {
        const int src = (rank - i + n) % n, dst = (rank + i) % n;
        if ((rc = x.shift(dst, in + disps[dst] * ext, cnts[dst] * ext, src, t1, B))) return rc;
        if (B && (rc = mv2h_reduce_local(t1, t0, cnts[rank], dtype, op, nullptr))) return rc;
    }
    return !B || hipMemcpy(out, t0, B, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN;
}

// MPIR_Reduce_scatter_ring(_2lvl) (:1026-1180, :1190-1300; its 1 MiB chunking does not change an
// element's order): at distance d this rank sends block (rank + d) to the right, having reduced the
// partial received from the left into its own data of that block
int sched_rs_ring(Xport &x, int n, int rank, const size_t *cnts, const size_t *disps, const char *in, char *out,
                  char *t0, char *t1, size_t ext, int dtype, int op) {
    const int right = (rank + 1) % n, left = (rank - 1 + n) % n;
    int rc = 0;
    for (int dist = n - 1; dist >= 0; --dist) {
        const int sr = (rank + dist) % n, rr = (rank + dist - 1 + n) % n;
        const size_t sc = cnts[sr];
        if (sc && hipMemcpy(t0, in + disps[sr] * ext, sc * ext, hipMemcpyDefault) != hipSuccess) return E_INTERN;
        if (dist < n - 1 && sc && (rc = mv2h_reduce_local(t1, t0, sc, dtype, op, nullptr))) return rc;
        if (dist > 0) {
            if ((rc = x.shift(right, t0, sc * ext, left, t1, cnts[rr] * ext))) return rc;
        } else if (sc && hipMemcpy(out, t0, sc * ext, hipMemcpyDefault) != hipSuccess) {
            return E_INTERN;
        }
    }
    return 0;
}

// leaders: recursive doubling on `acc` (device, `count` elements) with the nodes as ranks
int leader_rd(char *acc, size_t count, int dtype, int op, size_t bytes) {
    World &w = world();
    LeaderLinks x;
    return sched_allreduce(x, w.nnodes, w.node, acc, g_mn.d1, count, bytes / count, dtype, op, true);
}

// leaders: binomial broadcast of the host buffer h from node `root` (MPIR_Bcast_binomial order)
int leader_bcast(char *h, size_t bytes, int root) {
    World &w = world();
    const int n = w.nnodes, rel = (w.node - root + n) % n;
    int mask = 1, rc = 0;
    while (mask < n) {
        if (rel & mask) {
            if ((rc = net_recv((w.node - mask + n) % n, h, bytes))) return rc;
            break;
        }
        mask <<= 1;
    }
    for (mask >>= 1; mask > 0; mask >>= 1)
        if (rel + mask < n && (rc = net_send((w.node + mask) % n, h, bytes))) return rc;
    return 0;
}

// leaders: MPIR_Allreduce_pt2pt_rs_MV2 (:633-1054; recursive doubling for count < pof2, :802) with
// the nodes as ranks, MPI_IN_PLACE on `acc`.  Every leader's partial reaches every leader (a ring
// over the leaders) and each evaluates that algorithm's per-element programs for its own node
// index on the device; more than kMaxRanks nodes run the algorithm's message schedule itself.
int leader_prog(char *acc, size_t count, int dtype, int op, size_t bytes, int algo) {
    World &w = world();
    const int K = w.nnodes, me = w.node;
    if (K > mn_prog_max()) {
        LeaderLinks x;
        return sched_allreduce(x, K, me, acc, g_mn.d1, count, bytes / count, dtype, op, algo == ALG_PT2PT_RD);
    }
    const DtypeInfo *dt = dtype_lookup(dtype);
    Plan p;
    int rc = plan_allreduce(K, me, count, dt->size, dt->extent, true, algo, &p);
    if (rc) return rc;
    char *W = (char *)get_scratch(6, (size_t)K * bytes);
    if (!W) return E_NO_MEM;
    if ((rc = mn_reserve_host((size_t)K * bytes)) || (rc = mn_d2h(g_mn.h0 + (size_t)me * bytes, acc, bytes)))
        return rc;
    if ((rc = leader_ring_sections(g_mn.h0, bytes)) || (rc = mn_h2d(W, g_mn.h0, (size_t)K * bytes))) return rc;
    return reduce_gathered(W, K, bytes, acc, count, dtype, op, p.ps);
}
}  // namespace
}  // extern "C"

static int mn_require_device_reduction(int dtype, int op) {
    const DtypeInfo *dt = nullptr;
    const int rc = check_op_dtype(op, dtype, &dt);
    return rc ? rc : kind_supported(dt);
}

// MPIR_Allreduce_index_tuned_intra_MV2's selection (allreduce_osu.c:3015-3373) over the whole job.
// Returns 0 (two-level), 1 (flat ring wrapper), or ALG_PT2PT_RS / ALG_PT2PT_RD (flat over every
// rank).  The small-message shortcuts (:118-160) keep the two-level structure; the skip-large gate
// (:163-171) takes the ring wrapper; then the tuning tables (orders.cpp mn_allreduce_table).
static int mn_select(int ppn, int gsize, long nbytes, int *intra, int *inter) {
    const Knobs &K = knobs();
    *intra = MN_INTRA_NODE;  // the shortcuts' node step is the node's own small-message order
    *inter = ALG_PT2PT_RD;   // and their leaders' step recursive doubling (:2215-2262, :147-153)
    bool tables = false;
    if (K.allred_skip_small) {
        if (nbytes <= K.topo_allred_max && nbytes >= K.topo_allred_min && K.enable_topo && K.use_topo_allreduce) {
            if (ppn >= K.topo_allred_ppn) return 0;  // topology-aware hierarchical
            tables = true;                           // goto use_tables
        }
        if (!tables && K.enable_shmem_allreduce && K.enable_skip_search && nbytes <= K.coll_skip_thr) return 0;
    }
    if (!tables && K.allred_skip_large && K.allred_use_ring == 1 && K.allred_ring_thr <= nbytes &&
        ppn <= K.allred_ring_ppn)
        return 1;
    int in = MN_INTRA_NODE, it = ALG_PT2PT_RD;
    const int t = mn_allreduce_table(ppn, gsize, nbytes, &in, &it);
    if (t == 0) {
        *intra = in;
        *inter = it;
        return 0;
    }
    return t;
}

// How a multi-node call with a builtin op runs (a pure function of the job's shape and the call,
// so every rank takes the same route; mv2h_mn_route exposes it to the CPU tests).  A flat
// algorithm runs as per-element programs up to kMaxRanks ranks (MN_FLAT_PROG), as its message
// schedule over the rank channels up to kMeshMaxRanks (MN_SCHED: the rank mesh exists up to
// there), and above that the two-level structure stands in for it (MN_FALLBACK: Allreduce and
// Iallreduce the two-level allreduce with the default node and leader steps, Ireduce the
// two-level reduce helper, Reduce_scatter the basic algorithm) — correct for every builtin op,
// its fp order not the reference's (unpinned; integer, bitwise, logical and LOC results exact).
enum MnRoute { MN_TWO_LEVEL_R = 0, MN_RING_R = 1, MN_FLAT_PROG = 2, MN_SCHED = 3, MN_FALLBACK = 4, MN_BASIC_R = 5 };
static int mn_flat_route(int gsize) {
    return gsize <= mn_prog_max() ? MN_FLAT_PROG : gsize <= kMeshMaxRanks ? MN_SCHED : MN_FALLBACK;
}
// MPI_Allreduce / MPI_Iallreduce (nbc = the call's mv2h_nbc kind).  *rem_route: the route of the
// ring wrapper's count % gsize remainder (pt2pt_rs over every rank), -1 when there is none.
int mn_allreduce_route(int ppn, int gsize, long nbytes, size_t count, bool in_place, int nbc, int *intra,
                       int *inter, int *sel_out, int *rem_route) {
    *intra = MN_INTRA_NODE;
    *inter = ALG_PT2PT_RD;
    *sel_out = 0;
    *rem_route = -1;
    if (nbc == NBC_IALLREDUCE) return mn_flat_route(gsize);
    const int sel = mn_select(ppn, gsize, nbytes, intra, inter);
    *sel_out = sel;
    if (sel == 1) {
        if (!in_place && count >= (size_t)gsize) {
            if (count % (size_t)gsize) *rem_route = mn_flat_route(gsize);
            return MN_RING_R;
        }
        return mn_flat_route(gsize);
    }
    if (sel == ALG_PT2PT_RS || sel == ALG_PT2PT_RD) return mn_flat_route(gsize);
    return MN_TWO_LEVEL_R;
}
// MPI_Reduce_scatter / MPI_Ireduce_scatter over gsize ranks, nbytes in all
int mn_reduce_scatter_route(int gsize, long nbytes) {
    if (reduce_scatter_algo(gsize, nbytes) == ALG_RS_BASIC) return MN_BASIC_R;
    const int r = mn_flat_route(gsize);
    return r == MN_FALLBACK ? MN_BASIC_R : r;
}
// MPIR_Reduce_index_tuned_intra_MV2 across nodes (reduce_osu.c:2498-2660) for a commutative op
// (opk: builtin or commutative user op; a non-commutative one always takes the flat binomial,
// :2628-2636): two_level = MPIR_Reduce_two_level_helper_MV2 with the node step `intra` to local rank
// 0 and `algo` over the leaders to the root's node; else `algo` flat over every rank.  The
// small-message shortcut (:2508-2514: up to MV2_COLL_SKIP_TABLE_THRESHOLD, shmem + binomial) and the
// tables (orders.cpp mn_reduce_table).  The helper's MPIR_Reduce_shmem_MV2 node step becomes the intra
// knomial wrapper from the shmem slot size on (:2240-2251); the flat knomial needs a commutative op and
// the flat redscat_gather a builtin op with count >= pof2 (:2637-2652), else binomial.  The
// topology-aware reduce (:2498-2506, off by default) is not restated across nodes.
struct MnRedSel {
    bool two_level;
    int intra, algo, k;
};
static MnRedSel mn_reduce_select(int ppn, int gsize, size_t count, int tsize, int textent, int opk) {
    const Knobs &K = knobs();
    const long nbytes = (long)count * tsize;
    MnReduceCell c{};
    MnRedSel r{true, ALG_SHMEM_LINEAR, ALG_BINOMIAL, 4};
    if (opk == OPK_USER_NONCOMM) return MnRedSel{false, 0, ALG_BINOMIAL, 4};
    if (!(K.enable_shmem_reduce && K.enable_skip_search && nbytes <= K.coll_skip_thr)) {
        mn_reduce_table(ppn, gsize, nbytes, &c);
        r = MnRedSel{c.two_level != 0, c.intra, c.inter, c.k};
    } else {
        mn_reduce_table(ppn, gsize, nbytes, &c);  // the knomial factor only
        r.k = c.k;
    }
    if (r.two_level) {
        if (r.intra == ALG_SHMEM_LINEAR && !(K.enable_shmem_reduce && (long)count * textent < K.shmem_coll_max_msg))
            r.intra = ALG_KNOMIAL;
        return r;
    }
    if (r.algo == ALG_REDSCAT_GATHER && !(opk == OPK_BUILTIN && count >= (size_t)floor_pof2(gsize))) r.algo = ALG_BINOMIAL;
    return r;
}
// MPI_Reduce / MPI_Ireduce: MN_TWO_LEVEL_R (the helper), or a flat algorithm's route
int mn_reduce_route(int ppn, int gsize, size_t count, int tsize, int nbc) {
    if (nbc == NBC_IREDUCE) return mn_flat_route(gsize);
    const MnRedSel sel = mn_reduce_select(ppn, gsize, count, tsize, tsize, OPK_BUILTIN);
    return sel.two_level ? MN_TWO_LEVEL_R : mn_flat_route(gsize);
}

static int mn_allreduce_2lvl(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream,
                             int intra = MN_INTRA_NODE, int inter = ALG_PT2PT_RD);
static int mn_flat_allreduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream,
                             int algo, int root = -1, const Plan *forced = nullptr);

// The node's S-byte operands at its leader only (G: L * S bytes, local rank order; unused on the
// other ranks), over the node's device point-to-point channels in the library's collective context
static int gather_node_leader(const void *mine, char *G, size_t S) {
    World &w = world();
    const int L = w.size, base = w.node * w.size;  // point-to-point takes global ranks
    unsigned long long req[kMaxRanks] = {};
    int rc = 0;
    if (w.rank != 0) {
        if ((rc = p2p_isend(mine, S, base, kCollTagBase - 2, &req[0]))) return rc;
        return mv2h_p2p_wait(req[0], nullptr, nullptr, nullptr);
    }
    for (int l = 1; l < L; ++l)
        if ((rc = p2p_irecv(G + (size_t)l * S, S, base + l, kCollTagBase - 2, &req[l]))) return rc;
    if (hipMemcpy(G, mine, S, hipMemcpyDefault) != hipSuccess) return E_INTERN;
    for (int l = 1; l < L; ++l)
        if ((rc = mv2h_p2p_wait(req[l], nullptr, nullptr, nullptr))) return rc;
    return 0;
}

// Flat ring over every rank of the job (MPIR_Allreduce_pt2pt_ring_MV2, allreduce_osu.c:3916-3968):
// chunk c of (count / n) elements ends as x_c (+) x_{c+1} (+) ... (+) x_{c-1} over the global ranks,
// the accumulator always inout (uop(comp_chunk, recv_chunk), :3958).  Here each node gathers its
// ranks' operands, and the node leaders pass partial chunks round the ring of nodes: group g (the
// chunks of node g's ranks) starts at node g with the ranks from the chunk's own onwards, crosses
// every other node whole, and ends at node g with the ranks before it.  Every uop is one device
// Reduce_local.  The wrapper's remainder (count % n elements, pt2pt_rs over every rank, :3800-3818)
// is that flat algorithm (its programs up to kMaxRanks ranks, its message schedule above).
static int mn_ring_allreduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream) {
    World &w = world();
    const DtypeInfo *dt = dtype_lookup(dtype);
    const size_t ext = (size_t)dt->extent, S = count * ext;
    const int L = w.size, K = w.nnodes, n = w.gsize;
    const size_t cc = count / (size_t)n, cb = cc * ext, sect = (size_t)L * cb, main_bytes = (size_t)K * sect;
    const int chain[3] = {PV_AR_RING_WRAPPER, PV_AR_RING, PV_AR_SHM_RS};
    pvar_note_ids(chain, count % (size_t)n ? 3 : 2);
    int rc = 0;
    if (w.rank == 0) {
        char *G = (char *)get_scratch(6, (size_t)L * S);  // the node's operands, local rank order
        if (!G) return E_NO_MEM;
        if ((rc = gather_node_leader(sendbuf, G, S))) return rc;
        if ((rc = mn_reserve(std::max(main_bytes, sect)))) return rc;
        char *A = g_mn.d0;  // partial chunks of the group in hand
        auto X = [&](int l, size_t byte_off) { return (const char *)G + (size_t)l * S + byte_off; };
        const int me = w.node, right = (me + 1) % K, left = (me - 1 + K) % K;
        // round 0: this node's group, from each chunk's own rank to the node's last
        for (int l = 0; l < L; ++l) {
            const size_t off = ((size_t)me * L + l) * cb;
            if (hipMemcpy(A + (size_t)l * cb, X(l, off), cb, hipMemcpyDeviceToDevice) != hipSuccess) return E_INTERN;
            for (int m = l + 1; m < L; ++m)
                if ((rc = mv2h_reduce_local(X(m, off), A + (size_t)l * cb, cc, dtype, op, nullptr))) return rc;
        }
        for (int t = 1; t <= K; ++t) {
            if ((rc = mn_d2h(g_mn.h0, A, sect)) || (rc = net_shift(right, g_mn.h0, sect, left, g_mn.h1, sect)) ||
                (rc = mn_h2d(A, g_mn.h1, sect)))
                return rc;
            const int g = (me - t + K) % K;
            if (t < K) {  // a whole node: its ranks in order, all of the group's chunks at once
                for (int m = 0; m < L; ++m)
                    if ((rc = mv2h_reduce_local(X(m, (size_t)g * sect), A, cc * (size_t)L, dtype, op, nullptr)))
                        return rc;
            } else {  // back home: the ranks before each chunk's own
                for (int l = 0; l < L; ++l)
                    for (int m = 0; m < l; ++m)
                        if ((rc = mv2h_reduce_local(X(m, ((size_t)me * L + l) * cb), A + (size_t)l * cb, cc, dtype,
                                                    op, nullptr)))
                            return rc;
            }
        }
        // allgather of the groups over the leaders (data movement only), then into recvbuf
        if ((rc = mn_d2h(g_mn.h1 + (size_t)me * sect, A, sect)) || (rc = leader_ring_sections(g_mn.h1, sect)) ||
            (rc = mn_h2d(recvbuf, g_mn.h1, main_bytes)))
            return rc;
    } else if ((rc = gather_node_leader(sendbuf, nullptr, S))) {
        return rc;
    }
    if ((rc = bcast_node(recvbuf, main_bytes, 0, stream))) return rc;
    if (count % (size_t)n == 0) return 0;
    // the wrapper's pt2pt_rs over every rank (recursive doubling: rem < n)
    return mn_flat_allreduce((const char *)sendbuf + main_bytes, (char *)recvbuf + main_bytes, count % (size_t)n,
                             dtype, op, stream, ALG_PT2PT_RS);
}

// Every rank's S-byte operand onto every rank, in global rank order (*out: device scratch of
// gsize * S bytes): node allgather into the node's section, a ring of sections over the leaders,
// node broadcast.  The data movement of the flat algorithms restated across nodes.
static int mn_gather_all(const void *mine, size_t S, char **out, void *stream) {
    World &w = world();
    const int n = w.gsize;
    const size_t sect = (size_t)w.size * S, mine_off = (size_t)w.node * sect;
    char *W = (char *)get_scratch(6, (size_t)n * S);
    if (!W) return E_NO_MEM;
    int rc = 0;
    if (w.rank == 0 && (rc = mn_reserve_host((size_t)n * S))) return rc;
    if ((rc = allgather_node(mine, W + mine_off, S, stream))) return rc;
    if (w.rank == 0 && ((rc = mn_d2h(g_mn.h0 + mine_off, W + mine_off, sect)) ||
                        (rc = leader_ring_sections(g_mn.h0, sect)) || (rc = mn_h2d(W, g_mn.h0, (size_t)n * S))))
        return rc;
    if ((rc = bcast_node(W, (size_t)n * S, 0, stream))) return rc;
    *out = W;
    return 0;
}

// Flat pt2pt_rs / pt2pt_rd over more than kMaxRanks ranks (beyond the programs' registers): the
// algorithm's message schedule itself (sched_allreduce) over every rank's point-to-point channels,
// each step's received data reduced into this rank's accumulator (recvbuf, or device scratch when
// recvbuf is host memory) by one device Reduce_local.
static int mn_sched_allreduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, int algo) {
    World &w = world();
    const DtypeInfo *dt = dtype_lookup(dtype);
    const bool in_place = sendbuf == (const void *)-1;
    const size_t ext = (size_t)dt->extent, S = count * ext;
    if (w.gsize > kMeshMaxRanks) return E_UNSUPPORTED;  // no rank mesh: every rank refuses alike
    const int id = algo == ALG_PT2PT_RS ? PV_AR_SHM_RS : PV_AR_SHM_RD;
    pvar_note_ids(&id, 1);
    int rc = mn_reserve_dev(S);
    if (rc) return rc;
    char *acc = is_device(recvbuf) ? (char *)recvbuf : g_mn.d0;
    const void *src = in_place ? recvbuf : sendbuf;
    if (src != acc && hipMemcpy(acc, src, S, hipMemcpyDefault) != hipSuccess) return E_INTERN;
    RankChannels x;
    if ((rc = sched_allreduce(x, w.gsize, w.grank, acc, g_mn.d1, count, ext, dtype, op, algo == ALG_PT2PT_RD)))
        return rc;
    return acc == recvbuf || hipMemcpy(recvbuf, acc, S, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN;
}

// MVAPICH2's nonblocking schedules over more than kMaxRanks ranks, as messages: root >= 0
// MPI_Ireduce = MPIR_Ireduce_binomial to the root (ireduce_osu.c -> ireduce_tuning.c first row);
// root < 0 MPI_Iallreduce = MPIR_Iallreduce_naive (iallreduce.c:109-139): MPIR_Ireduce_intra to
// rank 0 — redscat_gather for builtin ops above MPIR_CVAR_REDUCE_SHORT_MSG_SIZE with count >= pof2
// (ireduce.c:700-731), else binomial — then MPIR_Ibcast, every rank taking rank 0's result.
static int mn_sched_naive(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream,
                          int root) {
    World &w = world();
    const DtypeInfo *dt = dtype_lookup(dtype);
    const bool in_place = sendbuf == (const void *)-1;
    const size_t ext = (size_t)dt->extent, S = count * ext;
    const int n = w.gsize, me = w.grank;
    if (n > kMeshMaxRanks) return E_UNSUPPORTED;  // no rank mesh: every rank refuses alike
    int rc = mn_reserve_dev(S);
    if (rc) return rc;
    // the accumulator: recvbuf where it is significant and device memory, else device scratch
    const bool mine = (root < 0 || me == root) && recvbuf && is_device(recvbuf);
    char *acc = mine ? (char *)recvbuf : g_mn.d0;
    const void *src = in_place ? recvbuf : sendbuf;
    if (src != acc && hipMemcpy(acc, src, S, hipMemcpyDefault) != hipSuccess) return E_INTERN;
    RankChannels x;
    const int pof2 = floor_pof2(n);
    if (root < 0 && (long)(count * (size_t)dt->size) > knobs().reduce_short_msg && count >= (size_t)pof2) {
        rc = sched_allreduce(x, n, me, acc, g_mn.d1, count, ext, dtype, op, false, true);
    } else {
        rc = sched_binomial_reduce(x, n, me, root < 0 ? 0 : root, acc, g_mn.d1, count, ext, dtype, op);
        if (!rc && root < 0) rc = mn_bcast(acc, S, 0, stream);
    }
    if (rc || (root >= 0 && me != root) || acc == recvbuf) return rc;
    return hipMemcpy(recvbuf, acc, S, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN;
}

// Flat pt2pt_rs / pt2pt_rd over every rank (allreduce_osu.c:633-1054, :360-630): every rank's operand reaches every rank
// (node allgather into its global slot, a ring over the leaders, node broadcast), and each rank
// evaluates the algorithm's per-element programs for its own rank — recursive doubling's results
// differ between ranks where the op is not commutative in its bits (MAX/MIN ties of ±0, NaN
// payloads), as the reference's do.  algo 0: the plan of the call's own selection (a nonblocking
// call's: MPIR_Iallreduce_naive = Ireduce to rank 0 + Ibcast, every rank takes rank 0's result).
// root >= 0 (MPI_Ireduce): only the root evaluates, the plan of MPIR_Ireduce_binomial.
static int mn_flat_allreduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream,
                             int algo, int root, const Plan *forced) {
    World &w = world();
    const DtypeInfo *dt = dtype_lookup(dtype);
    const bool in_place = sendbuf == (const void *)-1;
    const size_t S = count * (size_t)dt->extent;
    const int n = w.gsize;
    if (n > mn_prog_max() && root < 0 && (algo == ALG_PT2PT_RS || algo == ALG_PT2PT_RD))
        return mn_flat_route(n) == MN_SCHED ? mn_sched_allreduce(sendbuf, recvbuf, count, dtype, op, algo)
                                            : mn_allreduce_2lvl(sendbuf, recvbuf, count, dtype, op, stream);
    Plan p;
    int rc = forced ? (p = *forced, 0)
             : root >= 0 ? plan_reduce(n, w.grank, root, count, dt->size, dt->extent, &p)
                         : plan_allreduce(n, w.grank, count, dt->size, dt->extent, in_place, algo, &p);
    if (rc) return rc;
    pvar_note(root >= 0 ? PV_COLL_REDUCE : PV_COLL_ALLREDUCE, p, in_place, count, n);
    char *W = nullptr;  // every rank's operand, global rank order
    if ((rc = mn_reserve_dev(S)) || (rc = mn_gather_all(in_place ? recvbuf : sendbuf, S, &W, stream))) return rc;
    if (root >= 0 && w.grank != root) return 0;
    if ((rc = reduce_gathered(W, n, S, g_mn.d1, count, dtype, op, p.ps))) return rc;
    return hipMemcpy(recvbuf, g_mn.d1, S, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN;
}

int mn_allreduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream) {
    int rc = mn_require_device_reduction(dtype, op);
    if (rc || count == 0) return rc;
    const World &w = world();
    const DtypeInfo *dt = dtype_lookup(dtype);
    const bool in_place = sendbuf == (const void *)-1;
    const int gsize = w.gsize;
    int intra = MN_INTRA_NODE, inter = ALG_PT2PT_RD, sel = 0, rem = -1;
    const int route = mn_allreduce_route(w.size, gsize, (long)(count * (size_t)dt->size), count, in_place, nbc_kind(),
                                         &intra, &inter, &sel, &rem);
    // MPI_Iallreduce: MVAPICH2's nonblocking schedule is flat over the whole job
    // (MPIR_Iallreduce_intra_MV2 iallreduce_osu.c:257 -> MPIR_Iallreduce_naive: Ireduce to rank 0,
    // binomial or redscat_gather, then Ibcast), whatever the nodes
    if (nbc_kind() == NBC_IALLREDUCE) {
        if (route == MN_FLAT_PROG) return mn_flat_allreduce(sendbuf, recvbuf, count, dtype, op, stream, 0);
        if (route == MN_SCHED) return mn_sched_naive(sendbuf, recvbuf, count, dtype, op, stream, -1);
        return mn_allreduce_2lvl(sendbuf, recvbuf, count, dtype, op, stream);
    }
    if (route == MN_RING_R) return mn_ring_allreduce(sendbuf, recvbuf, count, dtype, op, stream);
    if (sel == 1) {
        // the wrapper's ring body needs count >= n and a separate sendbuf (:3893-3898); otherwise
        // it runs pt2pt_rs over every rank.  With
        // IN_PLACE the body's own fallback is pt2pt_rs over (count / n) * n elements (:4095-4100),
        // then the wrapper's pt2pt_rs on the remainder (:3800-3818): two calls, as on one node
        const int chain[2] = {PV_AR_RING_WRAPPER, PV_AR_SHM_RS};
        pvar_note_ids(chain, 2);
        const size_t main = in_place ? (count / (size_t)gsize) * (size_t)gsize : 0;
        if (main && main < count) {
            if ((rc = mn_flat_allreduce(sendbuf, recvbuf, main, dtype, op, stream, ALG_PT2PT_RS))) return rc;
            const size_t off = main * (size_t)dt->extent;
            return mn_flat_allreduce(sendbuf, (char *)recvbuf + off, count - main, dtype, op, stream, ALG_PT2PT_RS);
        }
        return mn_flat_allreduce(sendbuf, recvbuf, count, dtype, op, stream, ALG_PT2PT_RS);
    }
    if (sel == ALG_PT2PT_RS || sel == ALG_PT2PT_RD)
        return mn_flat_allreduce(sendbuf, recvbuf, count, dtype, op, stream, sel);
    return mn_allreduce_2lvl(sendbuf, recvbuf, count, dtype, op, stream, intra, inter);
}


static int mn_allreduce_2lvl(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, void *stream,
                             int intra, int inter) {
    World &w = world();
    int rc = 0;
    const DtypeInfo *dt = dtype_lookup(dtype);
    const size_t bytes = count * (size_t)dt->extent;
    // MPI_T: MPIR_Allreduce_two_level_MV2 (allreduce_osu.c:1693) with the leaders' recursive
    // doubling (MPIR_Allreduce_pt2pt_rd_MV2 :366) or pt2pt_rs (:639); the node step's own plan is
    // not counted
    const int chain[2] = {PV_AR_2LVL, inter == ALG_PT2PT_RS ? PV_AR_SHM_RS : PV_AR_SHM_RD};
    pvar_note_ids(chain, w.rank == 0 ? 2 : 1);
    // node step: the leader holds the node's partial
    if ((rc = node_allreduce_intra(sendbuf, recvbuf, count, dtype, op, stream, intra))) return rc;
    if (w.rank == 0) {
        if ((rc = mn_reserve(bytes))) return rc;
        if ((rc = mn_h2d(g_mn.d0, recvbuf, bytes)) ||
            (rc = inter == ALG_PT2PT_RS ? leader_prog(g_mn.d0, count, dtype, op, bytes, ALG_PT2PT_RS)
                                        : leader_rd(g_mn.d0, count, dtype, op, bytes)) ||
            (rc = mn_d2h(recvbuf, g_mn.d0, bytes)))
            return rc;
    }
    return bcast_node(recvbuf, bytes, 0, stream);  // MPIR_Shmem_Bcast_MV2 from the leader
}

int mn_bcast(void *buffer, size_t bytes, int root, void *stream) {
    World &w = world();
    if (root < 0 || root >= w.gsize) return E_ROOT;
    if (bytes == 0) return 0;
    const int rnode = root / w.size, rlocal = root % w.size;
    int rc = 0;
    if (w.node == rnode && rlocal != 0 && (rc = bcast_node(buffer, bytes, rlocal, stream))) return rc;
    if (w.rank == 0) {
        if ((rc = mn_reserve(bytes))) return rc;
        if (w.node == rnode && (rc = mn_d2h(g_mn.h0, buffer, bytes))) return rc;
        if ((rc = leader_bcast(g_mn.h0, bytes, rnode))) return rc;
        if (w.node != rnode && (rc = mn_h2d(buffer, g_mn.h0, bytes))) return rc;
    }
    if (w.node != rnode || rlocal == 0) rc = bcast_node(buffer, bytes, 0, stream);
    return rc;
}

// MPI_Reduce across nodes: the nonblocking schedule (MPI_Ireduce), else MPIR_Reduce_index_tuned_intra_MV2's
// choice (mn_reduce_select): MPIR_Reduce_two_level_helper_MV2 (reduce_osu.c:2030-2330: the node step
// to local rank 0, the leaders' algorithm to the root's node, the leader to the root) or a flat
// algorithm over every rank (programs up to kMaxRanks, its message schedule up to the rank mesh,
// the two-level helper with the shortcut's steps beyond).
static int mn_reduce_flat_sched(const void *src, void *recvbuf, size_t count, const DtypeInfo *dt, int dtype, int op,
                                int root, int algo, int k) {
    World &w = world();
    const size_t ext = (size_t)dt->extent, S = count * ext;
    const int n = w.gsize, me = w.grank;
    int rc = mn_reserve_dev(S);
    if (rc) return rc;
    const bool mine = me == root && recvbuf && is_device(recvbuf);
    char *acc = mine ? (char *)recvbuf : g_mn.d0;
    if (src != acc && hipMemcpy(acc, src, S, hipMemcpyDefault) != hipSuccess) return E_INTERN;
    RankChannels x;
    if (algo == ALG_KNOMIAL) rc = sched_knomial_reduce(x, n, me, root, k, acc, g_mn.d1, count, ext, dtype, op);
    else if (algo == ALG_REDSCAT_GATHER) rc = sched_allreduce(x, n, me, acc, g_mn.d1, count, ext, dtype, op, false, true);
    else rc = sched_binomial_reduce(x, n, me, root, acc, g_mn.d1, count, ext, dtype, op);
    if (rc || me != root || acc == recvbuf) return rc;
    return hipMemcpy(recvbuf, acc, S, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN;
}

// the leaders' step of the two-level helper: every leader's partial in g_mn.d0, the result in the
// root node's leader's g_mn.d0.  Up to kMaxRanks nodes the partials travel to that leader, which
// evaluates the algorithm's programs for the root node; above, the message schedule runs.
static int mn_reduce_leaders(size_t count, const DtypeInfo *dt, int dtype, int op, int rnode, int algo, int k) {
    World &w = world();
    const int K = w.nnodes, me = w.node;
    const size_t ext = (size_t)dt->extent, bytes = count * ext;
    int rc = 0;
    if (K > mn_prog_max()) {
        LeaderLinks x;
        if (algo == ALG_KNOMIAL) return sched_knomial_reduce(x, K, me, rnode, k, g_mn.d0, g_mn.d1, count, ext, dtype, op);
        if (algo == ALG_REDSCAT_GATHER)
            return sched_allreduce(x, K, me, g_mn.d0, g_mn.d1, count, ext, dtype, op, false, true);
        return sched_binomial_reduce(x, K, me, rnode, g_mn.d0, g_mn.d1, count, ext, dtype, op);
    }
    if (me != rnode) return (rc = mn_d2h(g_mn.h0, g_mn.d0, bytes)) ? rc : net_send(rnode, g_mn.h0, bytes);
    Plan pl;
    if ((rc = plan_reduce_forced(K, rnode, count, algo, k, &pl))) return rc;
    char *W = (char *)get_scratch(6, (size_t)K * bytes);
    if (!W) return E_NO_MEM;
    for (int j = 0; j < K; ++j) {
        if (j == me) rc = hipMemcpy(W + (size_t)j * bytes, g_mn.d0, bytes, hipMemcpyDeviceToDevice) == hipSuccess ? 0 : E_INTERN;
        else if (!(rc = net_recv(j, g_mn.h1, bytes))) rc = mn_h2d(W + (size_t)j * bytes, g_mn.h1, bytes);
        if (rc) return rc;
    }
    return reduce_gathered(W, K, bytes, g_mn.d0, count, dtype, op, pl.ps);
}

int mn_reduce(const void *sendbuf, void *recvbuf, size_t count, int dtype, int op, int root, void *stream) {
    World &w = world();
    if (root < 0 || root >= w.gsize) return E_ROOT;
    int rc = mn_require_device_reduction(dtype, op);
    if (rc || count == 0) return rc;
    const DtypeInfo *dt = dtype_lookup(dtype);
    const size_t bytes = count * (size_t)dt->extent;
    const int rnode = root / w.size, rlocal = root % w.size;
    const bool me_root = w.grank == root;
    const void *src = sendbuf == (const void *)-1 ? recvbuf : sendbuf;  // IN_PLACE: at the root only
    // MPI_Ireduce: MVAPICH2's nonblocking schedule (MPIR_Ireduce_binomial, ireduce_osu.c) is flat
    // over the whole job
    if (nbc_kind() == NBC_IREDUCE) {
        const int route = mn_flat_route(w.gsize);
        if (route == MN_FLAT_PROG) return mn_flat_allreduce(sendbuf, recvbuf, count, dtype, op, stream, 0, root);
        if (route == MN_SCHED) return mn_sched_naive(sendbuf, recvbuf, count, dtype, op, stream, root);
    }
    MnRedSel sel = mn_reduce_select(w.size, w.gsize, count, dt->size, dt->extent, OPK_BUILTIN);
    if (nbc_kind() == NBC_IREDUCE || (!sel.two_level && mn_flat_route(w.gsize) == MN_FALLBACK))
        sel = MnRedSel{true, ALG_SHMEM_LINEAR, ALG_BINOMIAL, sel.k};  // beyond the rank mesh (unpinned)
    if (!sel.two_level) {
        const int ids[3] = {sel.algo == ALG_KNOMIAL ? PV_RED_KNOMIAL : sel.algo == ALG_REDSCAT_GATHER ? PV_RED_REDSCAT_GATHER
                                                                                                       : PV_RED_BINOMIAL};
        pvar_note_ids(ids, 1);
        if (mn_flat_route(w.gsize) == MN_FLAT_PROG) {
            Plan p;
            if ((rc = plan_reduce_forced(w.gsize, root, count, sel.algo, sel.k, &p))) return rc;
            return mn_flat_allreduce(sendbuf, recvbuf, count, dtype, op, stream, 0, root, &p);
        }
        return mn_reduce_flat_sched(src, recvbuf, count, dt, dtype, op, root, sel.algo, sel.k);
    }
    // MPIR_Reduce_two_level_helper_MV2 (reduce_osu.c:2039) with the leaders' function
    const int chain[2] = {PV_RED_TWO_LEVEL_HELPER, sel.algo == ALG_KNOMIAL ? PV_RED_KNOMIAL
                                                   : sel.algo == ALG_REDSCAT_GATHER ? PV_RED_REDSCAT_GATHER
                                                                                    : PV_RED_BINOMIAL};
    pvar_note_ids(chain, w.rank == 0 && w.nnodes > 1 ? 2 : 1);
    if ((rc = mn_reserve_dev(bytes)) || (w.rank == 0 && (rc = mn_reserve_host(bytes)))) return rc;
    // node step to local rank 0: the leader's partial lands in g_mn.d0 (a non-root's recvbuf is not
    // significant)
    if (w.size > 1) {
        Plan pn;
        if ((rc = plan_reduce_forced(w.size, 0, count, sel.intra, sel.k, &pn)) ||
            (rc = reduce_entry(src, w.rank == 0 ? g_mn.d0 : nullptr, count, dtype, op, 0, stream, &pn)))
            return rc;
    } else if (hipMemcpy(g_mn.d0, src, bytes, hipMemcpyDefault) != hipSuccess) {
        return E_INTERN;
    }
    if (w.rank == 0 && (rc = mn_reduce_leaders(count, dt, dtype, op, rnode, sel.algo, sel.k))) return rc;
    if (w.node != rnode) return 0;
    if (rlocal == 0) return me_root ? mn_d2h(recvbuf, g_mn.d0, bytes) : 0;
    // the root is not the leader: the node's device point-to-point channel carries the result
    unsigned long long req = 0;
    if (w.rank == 0) {
        if ((rc = p2p_isend(g_mn.d0, bytes, root, kCollTagBase - 1, &req))) return rc;
        return mv2h_p2p_wait(req, nullptr, nullptr, nullptr);
    }
    if (me_root) {
        if ((rc = p2p_irecv(recvbuf, bytes, w.node * w.size, kCollTagBase - 1, &req))) return rc;
        return mv2h_p2p_wait(req, nullptr, nullptr, nullptr);
    }
    return 0;
}

int mn_allgather(const void *sendbuf, void *recvbuf, size_t bytes, void *stream) {
    World &w = world();
    if (bytes == 0) return 0;
    const size_t sect = bytes * (size_t)w.size, total = sect * (size_t)w.nnodes;
    char *mine = (char *)recvbuf + (size_t)w.node * sect;
    const bool in_place = sendbuf == (const void *)-1;
    int rc = allgather_node(in_place ? (const void *)(mine + (size_t)w.rank * bytes) : sendbuf, mine, bytes, stream);
    if (rc) return rc;
    if (w.rank == 0) {
        if ((rc = mn_reserve(total))) return rc;
        if ((rc = mn_d2h(g_mn.h0 + (size_t)w.node * sect, mine, sect)) || (rc = leader_ring_sections(g_mn.h0, sect)) ||
            (rc = mn_h2d(recvbuf, g_mn.h0, total)))
            return rc;
    }
    return bcast_node(recvbuf, total, 0, stream);
}

// Reduce_scatter across nodes: MPIR_Reduce_scatter_MV2 runs its flat algorithms over every rank of
// the job (red_scat_osu.c:1771-1900: ring / basic / recursive halving / pairwise by total size, the
// non-commutative forms for non-commutative ops; MPI_Ireduce_scatter: pairwise).  Every operand
// reaches every rank (mn_gather_all) and each rank evaluates its own block's programs of the
// selected algorithm over the job's ranks (orders.cpp plan_reduce_scatter, the same restatement as
// on one node).  Jobs above kMaxRanks ranks: the algorithm's message schedule itself
// (sched_rs_halving / _pairwise / _ring over the rank channels).  The basic algorithm at any size
// is MPIR_Reduce_MV2 over the whole job (the multi-node reduce) and a scatter.
int mn_reduce_scatter(const void *sendbuf, void *recvbuf, const size_t *recvcounts, int dtype, int op,
                             void *stream) {
    World &w = world();
    int rc = mn_require_device_reduction(dtype, op);
    if (rc) return rc;
    const DtypeInfo *dt = dtype_lookup(dtype);
    size_t total = 0, off = 0;
    for (int j = 0; j < w.gsize; ++j) {
        if (j == w.grank) off = total;
        total += recvcounts[j];
    }
    if (total == 0) return 0;
    const size_t ext = (size_t)dt->extent, S = total * ext;
    const bool in_place = sendbuf == (const void *)-1;
    const void *src = in_place ? recvbuf : sendbuf;
    const int n = w.gsize, me = w.grank, oi = op_index(op);
    const size_t mine = recvcounts[me] * ext;
    if (oi == OP_NO_OP || oi == OP_REPLACE) {  // nothing to reduce: this rank's own block
        return !mine || hipMemcpy(recvbuf, (const char *)src + off * ext, mine, hipMemcpyDefault) == hipSuccess
                   ? 0 : E_INTERN;
    }
    const int algo = reduce_scatter_algo(n, (long)(total * (size_t)dt->size));
    const int route = mn_reduce_scatter_route(n, (long)(total * (size_t)dt->size));
    if (route == MN_BASIC_R) {
        // MPIR_Reduce_Scatter_Basic_MV2 (red_scat_osu.c:300-413): MPIR_Reduce_MV2 to rank 0 over
        // the whole communicator — the multi-node reduce (mn_reduce) — then the blocks scattered
        const int chain[3] = {PV_RS_BASIC, PV_RED_TWO_LEVEL_HELPER, PV_RED_BINOMIAL};
        pvar_note_ids(chain, w.rank == 0 ? 3 : 2);
        char *tmp = (char *)get_scratch(5, S);
        if (!tmp) return E_NO_MEM;
        if ((rc = mn_reduce(src, tmp, total, dtype, op, 0, stream)) || (rc = mn_bcast(tmp, S, 0, stream))) return rc;
        return !mine || hipMemcpy(recvbuf, tmp + off * ext, mine, hipMemcpyDefault) == hipSuccess ? 0 : E_INTERN;
    }
    if (route == MN_SCHED) {
        // beyond the programs' registers: the algorithm's message schedule over the rank channels
        const int id = algo == ALG_RS_RING ? PV_RS_RING : algo == ALG_RS_PAIRWISE ? PV_RS_PAIRWISE : PV_RS_REC_HALVING;
        pvar_note_ids(&id, 1);
        std::vector<size_t> disps((size_t)n, 0);
        for (int j = 1; j < n; ++j) disps[j] = disps[j - 1] + recvcounts[j - 1];
        if ((rc = mn_reserve_dev(S))) return rc;
        const char *in = (const char *)src;
        if (!is_device(src)) {  // a host operand: staged to the device once
            char *stage = (char *)get_scratch(5, S);
            if (!stage || hipMemcpy(stage, src, S, hipMemcpyDefault) != hipSuccess) return stage ? E_INTERN : E_NO_MEM;
            in = stage;
        }
        // (MPI_IN_PLACE needs no copy: every schedule writes this rank's block after its last read)
        RankChannels x;
        auto fn = algo == ALG_RS_RING ? sched_rs_ring : algo == ALG_RS_PAIRWISE ? sched_rs_pairwise : sched_rs_halving;
        return fn(x, n, me, recvcounts, disps.data(), in, (char *)recvbuf, g_mn.d0, g_mn.d1, ext, dtype, op);
    }
    Plan p;
    if ((rc = plan_reduce_scatter(w.gsize, w.grank, recvcounts, dt->size, dt->extent, &p))) return rc;
    log_plan("reduce_scatter (flat over the job)", p, total);
    pvar_note(PV_COLL_REDUCE_SCATTER, p, in_place, total, w.gsize);
    char *W = nullptr;
    if ((rc = mn_reserve_dev(S)) || (rc = mn_gather_all(src, S, &W, stream))) return rc;
    if (!recvcounts[w.grank]) return 0;
    if ((rc = reduce_gathered(W, w.gsize, S, g_mn.d1, total, dtype, op, p.ps))) return rc;
    return hipMemcpy(recvbuf, g_mn.d1 + off * ext, recvcounts[w.grank] * ext, hipMemcpyDefault) == hipSuccess
               ? 0 : E_INTERN;
}

// Host-evaluated reductions across nodes (user ops, x87 types; mpi/user_coll.cpp, a big schedule's
// messages in mpi/host_sched.cpp): the schedule the device path above runs, as programs.
// Allreduce: a non-commutative op fails every shortcut and
// every two-level test and runs recursive doubling over the job (allreduce_osu.c:3359-3368);
// MPI_Iallreduce the flat naive schedule; else mn_select's choice (flat ring wrapper / flat
// pt2pt_rs or _rd / two-level with the entry's intra and inter functions).  Reduce: the flat
// binomial for a non-commutative op (the two-level helper needs a commutative one,
// reduce_osu.c:2628-2636) and for MPI_Ireduce, else the two-level helper (node reduce to local rank
// 0, binomial over the leaders to the root's node).  Flat schedules take the job's ranks as
// program registers up to kMaxRanks; above, `big` names the schedule the host evaluates itself.
int mn_host_schedule(int coll, size_t count, int tsize, int textent, bool in_place, int opk, int root, MnSched *s) {
    const World &w = world();
    const int n = w.gsize, me = w.grank, L = w.size, K = w.nnodes;
    memset(s, 0, sizeof(*s));
    s->kind = MN_FLAT;
    s->coll = coll;
    s->U = 0;
    const bool big = n > mn_prog_max();
    int rc = 0;
    if (coll == MN_COLL_REDUCE) {
        if (opk == OPK_USER_NONCOMM || nbc_kind() == NBC_IREDUCE) {
            if (big) {  // the flat binomial (MPIR_Reduce_binomial_MV2 / MPIR_Ireduce_binomial)
                const int id = PV_RED_BINOMIAL;
                if (nbc_kind() == NBC_NONE) pvar_note_ids(&id, 1);
                s->big = 1;
                s->forced = ALG_BINOMIAL;
                s->root = root;
                return 0;
            }
            rc = plan_reduce(n, me, root, count, tsize, textent, &s->p, opk);
            if (!rc) pvar_note(PV_COLL_REDUCE, s->p, in_place, count, n);
            return rc;
        }
        // MPIR_Reduce_index_tuned_intra_MV2's choice across nodes, as on the device path (mn_reduce)
        const MnRedSel sel = mn_reduce_select(L, n, count, tsize, textent, opk);
        const int fid = sel.algo == ALG_KNOMIAL ? PV_RED_KNOMIAL : sel.algo == ALG_REDSCAT_GATHER ? PV_RED_REDSCAT_GATHER
                                                                                                 : PV_RED_BINOMIAL;
        s->k = sel.k;
        if (!sel.two_level) {
            pvar_note_ids(&fid, 1);
            if (big) {  // the flat algorithm's schedule, evaluated on the host
                s->big = 1;
                s->forced = sel.algo;
                s->root = root;
                return 0;
            }
            s->forced = sel.algo;
            return plan_reduce_forced(n, root, count, sel.algo, sel.k, &s->p);
        }
        s->kind = MN_TWO_LEVEL;
        const int chain[2] = {PV_RED_TWO_LEVEL_HELPER, fid};
        pvar_note_ids(chain, w.rank == 0 ? 2 : 1);
        if ((rc = plan_reduce_forced(L, 0, count, sel.intra, sel.k, &s->node))) return rc;
        if (K > mn_prog_max()) {
            s->big = 1;
            s->forced = sel.algo;
            s->root = root / L;
            return 0;
        }
        return plan_reduce_forced(K, root / L, count, sel.algo, sel.k, &s->lead);
    }
    if (big && nbc_kind() == NBC_IALLREDUCE) {
        // MPIR_Iallreduce_naive: Ireduce to rank 0 — binomial for a user op (redscat_gather needs a
        // builtin one, ireduce.c:700-731) — and Ibcast: every rank takes rank 0's result
        s->big = 1;
        s->forced = ALG_BINOMIAL;
        s->root = 0;
        return 0;
    }
    if (big && opk == OPK_USER_NONCOMM) {  // every shortcut and two-level test fails: recursive doubling
        const int id = PV_AR_SHM_RD;
        pvar_note_ids(&id, 1);
        s->big = 1;
        s->forced = ALG_PT2PT_RD;
        return 0;
    }
    if (opk == OPK_USER_NONCOMM || nbc_kind() == NBC_IALLREDUCE) {
        if ((rc = plan_allreduce(n, me, count, tsize, textent, in_place, 0, &s->p, opk))) return rc;
        pvar_note(PV_COLL_ALLREDUCE, s->p, in_place, count, n);
        return 0;
    }
    int intra = MN_INTRA_NODE, inter = ALG_PT2PT_RD;
    const int sel = mn_select(L, n, (long)count * tsize, &intra, &inter);
    if (big && sel != 0) {
        // flat over more ranks than a program holds: the ring over (count / n) * n elements unless
        // IN_PLACE or count < n, then pt2pt_rs on the rest; IN_PLACE: two pt2pt_rs calls split
        // at (count / n) * n (:4095, :3800); else the tables' pt2pt_rs / pt2pt_rd.  (pt2pt_rs is
        // recursive doubling for a user op or fewer elements than pof2, :802.)
        s->big = 1;
        if (sel == 1 && !in_place && count >= (size_t)n) {
            const int chain[3] = {PV_AR_RING_WRAPPER, PV_AR_RING, PV_AR_SHM_RS};
            pvar_note_ids(chain, count % (size_t)n ? 3 : 2);
            s->forced = ALG_RING;
            s->U = (long)(count / n) * n;
        } else if (sel == 1) {
            const int chain[2] = {PV_AR_RING_WRAPPER, PV_AR_SHM_RS};
            pvar_note_ids(chain, 2);
            s->forced = ALG_PT2PT_RS;
            s->U = in_place ? (long)(count / n) * n : 0;
            if ((size_t)s->U == count) s->U = 0;
        } else {
            const int id = sel == ALG_PT2PT_RS || opk != OPK_BUILTIN ? PV_AR_SHM_RS : PV_AR_SHM_RD;
            pvar_note_ids(&id, 1);
            s->forced = sel;
        }
        return 0;
    }
    if (sel == 1 && n <= mn_prog_max()) {  // the flat ring wrapper over every rank
        const int chain[3] = {PV_AR_RING_WRAPPER, PV_AR_RING, PV_AR_SHM_RS};
        if (!in_place && count >= (size_t)n) {
            pvar_note_ids(chain, count % (size_t)n ? 3 : 2);
            s->forced = ALG_RING;
            s->U = (long)(count / n) * n;
            if ((rc = plan_allreduce(n, me, (size_t)s->U, tsize, textent, false, ALG_RING, &s->p, opk))) return rc;
        } else {
            const int rs_chain[2] = {PV_AR_RING_WRAPPER, PV_AR_SHM_RS};
            pvar_note_ids(rs_chain, 2);
            s->forced = ALG_PT2PT_RS;
            s->U = in_place ? (long)(count / n) * n : 0;  // IN_PLACE: two pt2pt_rs calls (:4095, :3800)
            if (s->U && (rc = plan_allreduce(n, me, (size_t)s->U, tsize, textent, true, ALG_PT2PT_RS, &s->p, opk)))
                return rc;
        }
        if ((size_t)s->U < count)
            rc = plan_allreduce(n, me, count - (size_t)s->U, tsize, textent, in_place, ALG_PT2PT_RS, &s->rem, opk);
        if (!s->U) s->p = s->rem;
        return rc;
    }
    if ((sel == ALG_PT2PT_RS || sel == ALG_PT2PT_RD) && n <= mn_prog_max()) {
        s->forced = sel;
        if ((rc = plan_allreduce(n, me, count, tsize, textent, in_place, sel, &s->p, opk))) return rc;
        pvar_note(PV_COLL_ALLREDUCE, s->p, in_place, count, n);
        return 0;
    }
    s->kind = MN_TWO_LEVEL;
    const int chain[2] = {PV_AR_2LVL, inter == ALG_PT2PT_RS ? PV_AR_SHM_RS : PV_AR_SHM_RD};
    pvar_note_ids(chain, w.rank == 0 ? 2 : 1);
    switch (intra) {
    case MN_INTRA_P2P: rc = plan_reduce(L, 0, 0, count, tsize, textent, &s->node, opk); break;
    case MN_INTRA_SHMEM: rc = plan_allreduce(L, 0, count, tsize, textent, in_place, ALG_SHMEM_LINEAR, &s->node, opk); break;
    case MN_INTRA_RS: rc = plan_allreduce(L, 0, count, tsize, textent, in_place, ALG_PT2PT_RS, &s->node, opk); break;
    case MN_INTRA_RD: rc = plan_allreduce(L, 0, count, tsize, textent, in_place, ALG_PT2PT_RD, &s->node, opk); break;
    default: rc = plan_allreduce(L, 0, count, tsize, textent, in_place, 0, &s->node, opk); break;
    }
    if (rc) return rc;
    if (K > mn_prog_max()) {  // the leaders' pt2pt_rs / _rd: recursive doubling for a user op
        s->big = 1;
        s->forced = ALG_PT2PT_RD;
        return 0;
    }
    return plan_allreduce(K, w.node, count, tsize, textent, true, inter, &s->lead, opk);
}

}  // namespace mv2

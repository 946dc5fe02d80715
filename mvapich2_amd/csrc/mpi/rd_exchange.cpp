// rd_exchange.cpp — recursive doubling for a user op on one node by its messages: every rank keeps
// its accumulator in a host window and reads its partners' (user_coll.cpp has the design and the
// place this path takes in MPI_Allreduce).
#include <stdlib.h>
#include <string.h>

#include "../../../include/mv2h.h"
#include "user_coll_internal.h"

namespace mv2 {

// MPIR_Allreduce_pt2pt_rd_MV2 (allreduce_osu.c:455-600) with its messages, on one node: each
// rank keeps its own accumulator in its host window and exchanges it with the step's partner
// through host shared memory, as the reference's ranks do through their shared-memory channel —
// the pre-step (an odd rank below 2 * rem reduces uop(tmp = x_{r-1}, acc)), log2(pof2) doubling
// steps (uop(tmp, acc) if commutative or the partner is lower, else uop(acc, tmp) copied back),
// the post-step (the even rank takes its partner's result).  The same operand order as the
// rank's own tree over every operand (the programs), with log2(pof2) uop calls instead of n - 1
// and one operand fetched instead of n.  Returns with *taken = false (and nothing done) when some
// rank's window or partner view could not be set up (a small /dev/shm): the caller takes the
// programs' path, on every rank alike.
int run_rd_exchange(const void *src, int count, const Typed &t, const HostOp &op, void *recvbuf, bool *taken) {
    World &w = world();
    const int n = w.size, me = w.rank;
    // MV2AMD_UOP_EXCHANGE: 1 always, 0 never; default from 4 ranks on, where it saves uop calls
    // (log2(pof2) against n - 1) and operand fetches (one against n); at 2 ranks both make one
    // call and the programs' path, whose operands never leave pinned memory, measured faster
    static const long mode = [] {
        const char *e = getenv("MV2AMD_UOP_EXCHANGE");
        return e && *e ? atol(e) : -1L;
    }();
    *taken = false;
    if (mode == 0 || (mode < 0 && n < 4)) return 0;
    const bool comm = op.opk != OPK_USER_NONCOMM;
    const size_t rspan = (size_t)dtype_span(t.dt, count), P = (size_t)count * (size_t)t.tsize;
    const int pof2 = floor_pof2(n), rem = n - pof2;
    const int newrank = me < 2 * rem ? ((me & 1) ? me / 2 : -1) : me - rem;
    auto real = [&](int q) { return q < rem ? 2 * q + 1 : q + rem; };
    // everything this rank needs is allocated before the vote, so that nothing after it can fail
    // short of a copy error (and that one still keeps the barriers: a rank leaving after the vote
    // would stall the others')
    const bool dev_src = mv2h_is_device_ptr(src), dev_dst = mv2h_is_device_ptr(recvbuf);
    // the operand's bytes from its true lower bound on (the layout is copied as it is, gaps
    // included: no pack / unpack on the host, whose block loop over a sparse span is slow)
    MPI_Aint tlb = 0, text = 0;
    PMPI_Type_get_true_extent(t.dt, &tlb, &text);
    const bool direct = tlb >= 0 && (t.contig || layout_on_device());
    const size_t dlen = direct ? rspan - (size_t)tlb : 0;
    HostBuf pk(HS_PACKED), T(HS_OPERANDS);
    pk.resize(P + 1);
    T.resize(rspan + 1);
    char *d = dev_src && !direct ? dev_scratch(DS_MINE, P) : nullptr;
    char *res = dev_scratch(DS_RES_ALL, P);
    char *sp = dev_dst && direct ? dev_scratch(DS_SPAN, rspan) : nullptr;
    char *acc = host_window(rspan + 1);
    bool ok = acc && pk.data() && T.data() && res && (d || !(dev_src && !direct)) && (sp || !(dev_dst && direct));
    host_barrier();  // every window reserved before any peer view is taken
    if (me < 2 * rem) ok = ok && host_peer_window((me & 1) ? me - 1 : me + 1, rspan + 1);
    if (newrank >= 0)
        for (int mask = 1; mask < pof2; mask <<= 1) ok = ok && host_peer_window(real(newrank ^ mask), rspan + 1);
    *taken = host_window_vote(ok);
    if (!*taken) return 0;
    auto peer = [&](int r) { return host_peer_window(r, rspan + 1); };
    auto uop = [&](const char *in, char *io) { call_uop(op.fn, in, io, count, t.dt); };
    // this rank's operand into its window, in the type's layout.  From the vote on, a failing
    // copy or pack leaves rc set but the rank still takes part in every barrier below, so that
    // the other ranks finish the call (with this rank's stale window) instead of stalling
    PhaseClock pc;
    char *tmp = T.data();
    int rc = 0;
    if (direct) {
        if (dev_src) {
            if (dlen && mv2h_memcpy_dtoh(acc + tlb, (const char *)src + tlb, dlen)) rc = MPI_ERR_OTHER;
        } else {
            memcpy(acc + tlb, (const char *)src + tlb, dlen);
        }
    } else if (dev_src) {
        if (!(rc = dtype_pack(src, count, t.dt, d)) && P && mv2h_memcpy_dtoh(pk.data(), d, P)) rc = MPI_ERR_OTHER;
        if (!rc) rc = dtype_unpack(pk.data(), count, t.dt, acc);
    } else if (!(rc = dtype_pack(src, count, t.dt, pk.data()))) {
        rc = dtype_unpack(pk.data(), count, t.dt, acc);
    }
    pc.mark(UP_FETCH);
    // pre-step (:455-505)
    host_barrier();  // every accumulator in place
    if (me < 2 * rem && (me & 1)) memcpy(tmp, peer(me - 1), rspan);
    host_barrier();  // every read done before any accumulator changes
    if (me < 2 * rem && (me & 1)) uop(tmp, acc);
    // doubling steps (:507-584)
    for (int mask = 1; mask < pof2; mask <<= 1) {
        const int dst = newrank >= 0 ? real(newrank ^ mask) : -1;
        host_barrier();
        if (dst >= 0) memcpy(tmp, peer(dst), rspan);
        host_barrier();
        if (dst < 0) continue;
        if (comm || dst < me) {
            uop(tmp, acc);
        } else {
            uop(acc, tmp);
            memcpy(acc, tmp, rspan);
        }
    }
    // post-step (:585-600): the even rank below 2 * rem takes rank + 1's result
    host_barrier();
    if (me < 2 * rem && !(me & 1)) memcpy(tmp, peer(me + 1), rspan);
    const char *res_h = me < 2 * rem && !(me & 1) ? tmp : acc;
    if (!rc && direct && dev_dst) {  // the result's span up, its type map packed on the device
        if (dlen && mv2h_memcpy_htod(sp + tlb, res_h + tlb, dlen)) rc = MPI_ERR_OTHER;
        if (!rc) rc = dtype_pack(sp, count, t.dt, res);
    } else if (!rc && direct) {  // a host receive buffer: its type map from the result's
        dtype_merge_typemap((char *)recvbuf, res_h, t.dt, count);
    } else if (!rc) {
        rc = dtype_pack(res_h, count, t.dt, pk.data());
    }
    host_barrier();  // the post-step's reads are done before any window is reused
    pc.mark(UP_EVAL);  // the exchanges and the uop calls
    if (rc) return rc;
    if (!direct && P && mv2h_memcpy_htod(res, pk.data(), P)) return MPI_ERR_OTHER;
    // operand bytes this rank received (packed measure): pre- or post-step, and one per doubling step
    world().uop_in_bytes = P * (size_t)((me < 2 * rem) + (newrank >= 0 ? __builtin_ctz((unsigned)pof2) : 0));
    world().uop_area_bytes = rspan;
    rc = direct && !dev_dst ? 0 : dtype_unpack(res, count, t.dt, recvbuf);
    pc.mark(UP_DELIVER);
    return rc;
}

}  // namespace mv2

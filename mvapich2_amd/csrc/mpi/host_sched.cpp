// host_sched.cpp — more ranks (or leaders) than a program holds: the reference's message schedules
// restated on the host (user_coll.cpp has the design), one rank's result at a time (sched_eval;
// behind the C ABI for the CPU tests: mv2h_host_sched_eval).
#include <string.h>

#include "../../../include/mv2h.h"
#include "user_coll_internal.h"

namespace mv2 {
namespace {

// W holds `n` operands in the type's layout, rspan bytes apart, cnt elements each; every function
// writes one rank's result (type layout, rspan bytes) to out and leaves W unchanged.
struct BigEval {
    const char *W;
    long rspan;
    int n, cnt;
    const Typed *t;
    MPI_User_function *fn;
    bool comm;
    const Pof2Fold f{n};
    std::vector<std::vector<char>> scratch{};  // one operand-sized buffer per recursion level
    // MPIR_Reduce_redscat_gather_MV2's pre-step (reduce_osu.c:849-894: odd ranks below 2 * rem hand
    // their operand to rank - 1, the even ones keep their place) instead of the allreduce's
    bool redscat = false;
    char *level(int l) {
        if ((int)scratch.size() <= l) scratch.resize((size_t)l + 1);
        if (scratch[l].size() < (size_t)rspan + 1) scratch[l].resize((size_t)rspan + 1);
        return scratch[l].data();
    }
    void uop(const char *in, char *inout) { call_uop(fn, in, inout, cnt, t->dt); }
    const char *x(int r) const { return W + (size_t)r * (size_t)rspan; }
    // one operand's cnt elements (a sub-range's span, not the stride: W may start mid-operand)
    void copy(char *dst, const char *src) const { memcpy(dst, src, (size_t)dtype_span(t->dt, cnt)); }

    int real(int q) const { return f.real(q, redscat); }
    // the non-power-of-two pre-step: newrank nr's starting value (an odd rank below 2 * rem has
    // reduced uop(tmp = x_{r-1}, recvbuf); redscat_gather: an even one uop(tmp = x_{r+1}, recvbuf))
    void base(int nr, char *out) {
        const int r = real(nr);
        copy(out, x(r));
        if (r < 2 * f.rem) uop(x(redscat ? r + 1 : r - 1), out);
    }
    // MPIR_Allreduce_pt2pt_rd_MV2 (allreduce_osu.c:455-600; also pt2pt_rs for a user op, :802): the
    // value newrank nr holds after `lev` doubling steps
    void rd_value(int nr, int lev, char *out) {
        if (lev == 0) return base(nr, out);
        const int mask = 1 << (lev - 1), pr = nr ^ mask;
        char *other = level(lev);
        rd_value(nr, lev - 1, out);
        rd_value(pr, lev - 1, other);
        if (comm || real(pr) < real(nr)) {
            uop(other, out);  // uop(tmp_buf, recvbuf)
        } else {
            uop(out, other);  // uop(recvbuf, tmp_buf), then tmp_buf copied into recvbuf
            copy(out, other);
        }
    }
    // MPIR_Allreduce_pt2pt_rs_MV2's reduce-scatter + allgather (:852-1000; builtin ops, at least
    // pof2 elements): block i of pof2 (count / pof2 elements, the last the remainder) is reduced
    // at the newrank whose bits are i's reversed (each halving step keeps the lower half at the
    // lower newrank), along the same doubling steps as recursive doubling at that newrank, and
    // the allgather gives every rank every block
    void rs(char *out) {
        const long per = cnt / f.pof2;
        for (int i = 0; i < f.pof2; ++i) {
            const long b = (long)i * per, c = i < f.pof2 - 1 ? per : cnt - per * (f.pof2 - 1);
            int owner = 0;
            for (int j = 0; j < f.lev; ++j) owner = (owner << 1) | ((i >> j) & 1);
            BigEval sub{W + (size_t)b * (size_t)t->extent, rspan, n, (int)c, t, fn, comm};
            sub.redscat = redscat;  // the block keeps redscat_gather's pre-step
            std::vector<char> part((size_t)rspan + 1);
            sub.rd_value(owner, f.lev, part.data());
            memcpy(out + (size_t)b * (size_t)t->extent, part.data(), (size_t)dtype_span(t->dt, (int)c));
        }
    }
    // rank me's recursive-doubling result (an even rank below 2 * rem takes rank + 1's in the post-step)
    void rd(int me, char *out) { rd_value(f.newrank(me), f.lev, out); }
    // MPI_Reduce_scatter, this rank's block (W holds its elements of every operand; commutative
    // ops).  MPIR_Reduce_scatter_Rec_Halving_MV2 (red_scat_osu.c:428-780): the pre-step, then
    // halving steps with masks pof2/2, pof2/4, ... 1, each uop(tmp_recvbuf, tmp_results); newrank i
    // ends with new block i, which holds rank i's block (and, below 2 * rem, its even neighbour's)
    void rh_value(int nr, int k, int lev, char *out) {
        if (k == 0) return base(nr, out);
        const int mask = (1 << lev) >> k;
        char *other = level(k);
        rh_value(nr, k - 1, lev, out);
        rh_value(nr ^ mask, k - 1, lev, other);
        uop(other, out);
    }
    void rs_halving(int me, char *out) { rh_value(f.newrank(me), f.lev, f.lev, out); }
    // MPIR_Reduce_scatter_Pair_Wise_MV2 (:786-1020): own data, then uop(x_{me-i}, acc), i = 1 .. n-1
    void rs_pairwise(int me, char *out) {
        copy(out, x(me));
        for (int i = 1; i < n; ++i) uop(x((me - i + n) % n), out);
    }
    // MPIR_Reduce_scatter_ring (:1026-1180): the block starts at rank me + 1; each next rank
    // reduces the partial it receives into its own data, uop(tmp_recvbuf, tmp_sendbuf)
    void rs_ring(int me, char *out) {
        char *acc = level(0), *next = level(1);
        copy(acc, x((me + 1) % n));
        for (int j = 2; j <= n; ++j) {
            copy(next, x((me + j) % n));
            uop(acc, next);
            std::swap(acc, next);
        }
        copy(out, acc);
    }
    // MPIR_Reduce_binomial_MV2 (reduce_osu.c:577-663): relative rank rel's value once the masks
    // below m are done (a non-commutative op reduces towards rank 0, which forwards to the root)
    void bin_value(int rel, int m, int lroot, int l, char *out) {
        if (m == 1) return copy(out, x((rel + lroot) % n));
        const int half = m / 2;
        bin_value(rel, half, lroot, l + 1, out);
        if ((rel | half) >= n) return;
        char *child = level(l);
        bin_value(rel | half, half, lroot, l + 1, child);
        if (comm) {
            uop(child, out);  // uop(tmp_buf, recvbuf)
        } else {
            uop(out, child);  // uop(recvbuf, tmp_buf), then tmp_buf copied into recvbuf
            copy(out, child);
        }
    }
    void binomial(int root, char *out) {
        int m = 1;
        while (m < n) m <<= 1;
        bin_value(0, m, comm ? root : 0, 0, out);
    }
    // MPIR_Reduce_knomial_MV2 (reduce_osu.c:1639-1837) to `root`: relative rank rel's value is its
    // own operand reduced with its children's values (MPIR_Reduce_knomial_trace :1568-1633), the
    // trace's last child first (request-index order), uop(tmp, recvbuf)
    void knom_value(int rel, int root, int k, int l, char *out) {
        copy(out, x((rel + root) % n));
        int mask = 1;
        while (mask < n && !(rel % (k * mask))) mask *= k;
        mask /= k;
        std::vector<int> kids;
        for (int m = mask; m > 0; m /= k)
            for (int j = 1; j < k; ++j)
                if (rel + m * j < n) kids.push_back(rel + m * j);
        char *child = level(l);
        for (size_t i = kids.size(); i-- > 0;) {
            knom_value(kids[i], root, k, l + 1, child);
            uop(child, out);
        }
    }
    void knomial(int root, int k, char *out) { knom_value(0, root, k < 2 ? 2 : k, 0, out); }
    // MPIR_Reduce_redscat_gather_MV2 (reduce_osu.c:718-1100): its reduce-scatter (the recursive
    // halving of pt2pt_rs after its own pre-step), the gather to the root
    void redscat_gather(char *out) { redscat = true, rs(out), redscat = false; }
    // an expression tree (orders.h ExprNode) over the n operands: node e's value into out
    void expr(const std::vector<ExprNode> &nodes, int e, int l, char *out) {
        const ExprNode &nd = nodes[(size_t)e];
        if (nd.leaf >= 0) return copy(out, x(nd.leaf));
        expr(nodes, nd.a, l + 1, out);  // the inout operand
        char *in = level(l);
        expr(nodes, nd.b, l + 1, in);
        uop(in, out);
    }
    // MPIR_Allreduce_pt2pt_ring_MV2's chunk c (allreduce_osu.c:3916-3968): x_c, then uop(x_{c+j},
    // acc) for j = 1 .. n-1
    void ring_chunk(int c, char *out) {
        copy(out, x(c));
        for (int j = 1; j < n; ++j) uop(x((c + j) % n), out);
    }
};

}  // namespace

int sched_eval(const Sched &s, const char *W, long rspan, int n, int cnt, const Typed &t, MPI_User_function *fn,
               bool comm, char *out) {
    BigEval ev{W, rspan, n, cnt, &t, fn, comm};
    switch (s.form) {
        case MV2H_SCHED_RD: ev.rd(s.me, out); break;
        case MV2H_SCHED_PT2PT_RS: ev.rs(out); break;
        case MV2H_SCHED_BINOMIAL: ev.binomial(s.root, out); break;
        case MV2H_SCHED_KNOMIAL: ev.knomial(s.root, s.k, out); break;
        case MV2H_SCHED_REDSCAT_GATHER: ev.redscat_gather(out); break;
        case MV2H_SCHED_RS_HALVING: ev.rs_halving(s.me, out); break;
        case MV2H_SCHED_RS_PAIRWISE: ev.rs_pairwise(s.me, out); break;
        case MV2H_SCHED_RS_RING: ev.rs_ring(s.me, out); break;
        case MV2H_SCHED_RING_CHUNK: ev.ring_chunk(s.me, out); break;
        case MV2H_SCHED_RS_NONCOMM: {  // the expression's tree over the operands, uop(in = b, inout = a) per node
            std::vector<ExprNode> nodes;
            const int e = rs_noncomm_expr(n, s.me, s.k != 0, nodes);
            if (e < 0) return MPI_ERR_INTERN;
            ev.expr(nodes, e, 0, out);
            break;
        }
        default: return MPI_ERR_ARG;
    }
    return 0;
}

int sched_eval_packed(const Sched &s, const char *W, long rspan, int n, int cnt, const Typed &t,
                      MPI_User_function *fn, bool comm, HostBuf &R) {
    std::vector<char> out((size_t)rspan + 1);
    if (const int rc = sched_eval(s, W, rspan, n, cnt, t, fn, comm, out.data())) return rc;
    if (!R.reserve((size_t)cnt * (size_t)t.tsize + 1)) return MPI_ERR_NO_MEM;
    return dtype_pack(out.data(), cnt, t.dt, R.data());
}

}  // namespace mv2

// the hook's user function: inout = 2 in + 3 inout, int32 wrapping (neither commutative nor
// associative, so every operand order shows)
static void hook_fn(void *in, void *inout, int *len, MPI_Datatype *) {
    const int32_t *a = (const int32_t *)in;
    int32_t *b = (int32_t *)inout;
    for (int i = 0; i < *len; ++i) b[i] = (int32_t)((uint32_t)a[i] * 2u + (uint32_t)b[i] * 3u);
}

extern "C" int mv2h_host_sched_eval(int form, int n, int me, int root, int k, int count, int commute,
                                    const int32_t *ops, int32_t *out) {
    using namespace mv2;
    if (n < 1 || count < 1 || me < 0 || me >= n || root < 0 || root >= n || !ops || !out) return MPI_ERR_ARG;
    // MV2H_SCHED_RS_NONCOMM, equal blocks: the mirror-permuted halving at a power of two
    const Sched s{form, me, root, form == MV2H_SCHED_RS_NONCOMM ? (n & (n - 1)) == 0 : k};
    return sched_eval(s, (const char *)ops, (long)count * 4, n, count, typed(MPI_INT), hook_fn, commute != 0,
                      (char *)out);
}

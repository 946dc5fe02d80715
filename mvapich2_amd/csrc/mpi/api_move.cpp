// api_move.cpp — the collectives that move data without reducing it: MPI_Allgather(v),
// MPI_Alltoall(v, w), MPI_Gather(v), MPI_Scatter(v), MPI_Bcast, and the stream-ordered
// Allgather, Alltoall and Bcast (api_internal.h has the front end's shared state and checks).
#include "../runtime/log.h"
#include "../runtime/world.h"
#include "api_internal.h"

using namespace mv2;

// ---------------------------------------------------------------------------
// MPI_Allgather / MPI_Alltoall: n equal blocks.
// ---------------------------------------------------------------------------
// A uniform collective with a non-contiguous type on either side: pack this rank's contribution
// on the device -- its one block (Allgather), or all n (all_blocks, Alltoall: block j is elements
// [j * sendcount, (j + 1) * sendcount), so the n blocks are n * sendcount consecutive elements)
// --, exchange the packed bytes, and unpack all n blocks with one launch (block i of recvbuf
// starts i * recvcount extents in, so the n blocks are n * recvcount consecutive elements of
// recvtype).  The reference stages derived types through Localcopy / segment pack
// (allgather_osu.c:2426, helper_fns.h:62-250).
static int uniform_derived(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                           MPI_Datatype recvtype, MPI_Comm comm, bool all_blocks,
                           int (*exchange)(const void *, void *, size_t, void *)) {
    const bool in_place = sendbuf == MPI_IN_PLACE;
    const long psize = dtype_size(recvtype) * recvcount;
    if (!in_place && dtype_size(sendtype) * sendcount != psize) return MPI_ERR_TRUNCATE;
    if (psize == 0) return MPI_SUCCESS;
    const int n = comm_size_of(comm), k = all_blocks ? n : 1;
    void *out = pool_get((size_t)psize * k), *in = out ? pool_get((size_t)psize * n) : nullptr;
    if (!in) {
        if (out) pool_put(out);
        return MPI_ERR_NO_MEM;
    }
    // in place the contribution is read from recvbuf: all of it, or this rank's block
    const void *src = !in_place    ? sendbuf
                      : all_blocks ? recvbuf
                                   : (const char *)recvbuf + (long)comm_rank_of(comm) * recvcount * dtype_extent(recvtype);
    int pos = 0;
    int rc = PMPI_Pack(src, (in_place ? recvcount : sendcount) * k, in_place ? recvtype : sendtype, out, (int)(psize * k),
                       &pos, comm);
    if (!rc) rc = n > 1 ? exchange(out, in, (size_t)psize, nullptr) : mv2h_memcpy_dtod(in, out, (size_t)psize);
    pos = 0;
    if (!rc) rc = PMPI_Unpack(in, (int)(psize * n), &pos, recvbuf, recvcount * n, recvtype, comm);
    pool_put(out);
    pool_put(in);
    return rc;
}

// allgather.c:952-958, before any other argument check: the send buffer is this rank's block
// of the receive buffer, the block measured in recvtype's size (as the reference measures it)
static bool allgather_alias(const void *sendbuf, int sendcount, MPI_Datatype sendtype, const void *recvbuf,
                            int recvcount, MPI_Datatype recvtype, int rank) {
    return sendbuf != MPI_IN_PLACE && sendtype == recvtype && recvcount != 0 && sendcount != 0 &&
           dtype_valid(recvtype) && sendbuf == (const char *)recvbuf + (long)rank * recvcount * dtype_size(recvtype);
}

// MPI_Allgather, and MPIX_Allgather_enqueue (enq) on `stream`: it tests the stream right after
// the communicator and refuses what the host would have to finish (derived types, host buffers)
template <bool enq>
static int allgather_call(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                          MPI_Datatype recvtype, MPI_Comm comm, void *stream, const char *fn) {
    int me = 0, rc;
    if ((rc = comm_checks(comm, nullptr, &me))) return err_return(comm, rc, fn);
    if (enq && !stream) return err_return(comm, MPI_ERR_ARG, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (allgather_alias(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, me))
        return err_return(comm, MPI_ERR_BUFFER, fn);
    if ((rc = pair_checks(in_place, sendcount, sendtype, recvcount, recvtype))) return err_return(comm, rc, fn);
    // allgather.c:961-987, after the counts and types
    if ((!in_place && null_userbuf(sendbuf, sendcount, sendtype)) || inplace_buf(recvbuf, recvcount) ||
        null_userbuf(recvbuf, recvcount, recvtype))
        return err_return(comm, MPI_ERR_BUFFER, fn);
    if (!dtype_is_contiguous(recvtype) || (!in_place && !dtype_is_contiguous(sendtype))) {
        rc = enq ? MPI_ERR_TYPE
                 : uniform_derived(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm, false, mv2h_allgather);
        return err_return(comm, rc, fn);
    }
    const size_t rbytes = (size_t)dtype_span(recvtype, recvcount);
    if (!in_place && (size_t)dtype_span(sendtype, sendcount) != rbytes) return err_return(comm, MPI_ERR_TRUNCATE, fn);
    if (rbytes == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF)  // blocking: a device copy whatever the pointers are
        rc = enq ? copy_any_enqueue(recvbuf, sendbuf, rbytes, stream) : in_place ? 0 : mv2h_memcpy_dtod(recvbuf, sendbuf, rbytes);
    else
        rc = enq ? mv2h_allgather_enqueue(sendbuf, recvbuf, rbytes, stream) : mv2h_allgather(sendbuf, recvbuf, rbytes, nullptr);
    return err_return(comm, rc, fn);
}

// MPI_Alltoall / MPI_Alltoallv (alltoall.c:650-713, alltoallv.c:520-594 for the checks).
// MPI_IN_PLACE is the send buffer only; with it the send count and type (sendcounts / sdispls)
// are ignored and the blocks are read from recvbuf.
static int alltoall_checks(const void *sendbuf, int sendcount, MPI_Datatype sendtype, const void *recvbuf,
                           int recvcount, MPI_Datatype recvtype, MPI_Comm comm) {
    if (const int rc = comm_checks(comm)) return rc;
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (const int rc = pair_checks(in_place, sendcount, sendtype, recvcount, recvtype)) return rc;
    if (!in_place && null_userbuf(sendbuf, sendcount, sendtype)) return MPI_ERR_BUFFER;
    if (inplace_buf(recvbuf, recvcount) || null_userbuf(recvbuf, recvcount, recvtype)) return MPI_ERR_BUFFER;
    if (!in_place && sendcount != 0 && recvcount != 0 && sendbuf == recvbuf) return MPI_ERR_BUFFER;  // alltoall.c:690-695
    return MPI_SUCCESS;
}

// MPI_Alltoall, and MPIX_Alltoall_enqueue (enq) on `stream`, tested after all of alltoall_checks
template <bool enq>
static int alltoall_call(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                         MPI_Datatype recvtype, MPI_Comm comm, void *stream, const char *fn) {
    int rc = alltoall_checks(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm);
    if (!rc && enq && !stream) rc = MPI_ERR_ARG;
    if (rc) return err_return(comm, rc, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!dtype_is_contiguous(recvtype) || (!in_place && !dtype_is_contiguous(sendtype))) {
        rc = enq ? MPI_ERR_TYPE
                 : uniform_derived(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm, true, mv2h_alltoall);
        return err_return(comm, rc, fn);
    }
    const size_t rbytes = (size_t)dtype_span(recvtype, recvcount);
    if (!in_place && (size_t)dtype_span(sendtype, sendcount) != rbytes) return err_return(comm, MPI_ERR_TRUNCATE, fn);
    if (rbytes == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF)
        rc = in_place ? 0 : enq ? copy_any_enqueue(recvbuf, sendbuf, rbytes, stream) : copy_any(recvbuf, sendbuf, rbytes);
    else
        rc = enq ? mv2h_alltoall_enqueue(sendbuf, recvbuf, rbytes, stream) : mv2h_alltoall(sendbuf, recvbuf, rbytes, nullptr);
    return err_return(comm, rc, fn);
}

// ---------------------------------------------------------------------------
// MPI_Alltoallw, and MPI_Alltoallv with a non-contiguous type (alltoallw.c:425-530 for the checks).
// A side of the call -- n blocks, block j = cnt[j] elements of dt[j] at buf + dsp[j] bytes -- is
// either left alone or staged.  Every type of a non-empty block contiguous: the runtime reads or
// writes the user's buffer at the byte displacements (all-contiguous Alltoallw is Alltoallv with
// byte displacements).  Otherwise the whole side goes through one pooled device buffer in which
// block j is packed at a 16-byte-aligned running offset, cnt[j] x size(dt[j]) bytes long, so the
// exchange sees aligned blocks and never shifts.  A device buffer is staged by ONE launch for all
// n blocks (mv2h_pack_blocks, pack/pack_blocks.hip); a host buffer, or any buffer under
// mv2h_set_tuning("pack_blocks", 0), block by block (dtype_pack / dtype_unpack).  The exchange is
// mv2h_alltoallv on what the two sides show: a pair whose packed lengths differ is
// MPI_ERR_TRUNCATE on every rank before it, and the receive side is then not written.
// ---------------------------------------------------------------------------
struct WSide {
    char *buf = nullptr;
    int n = 0;
    std::vector<int> cnt;
    std::vector<long> dsp;  // bytes
    std::vector<MPI_Datatype> dt;
    bool staged = false;
    void *tmp = nullptr;
    std::vector<size_t> bytes, offs;  // what the runtime sees
    size_t total = 0;                 // of the staging buffer
    char *rt_buf() const { return staged ? (char *)tmp : buf; }
    ~WSide() {
        if (tmp) pool_put(tmp);
    }
};

// one element is its extent's bytes and nothing else (a builtin pair type has padding)
static bool plain_type(MPI_Datatype dt) {
    return dtype_is_contiguous(dt) && dtype_size(dt) == dtype_extent(dt) && dtype_true_lb(dt) == 0;
}

static void wside_set(WSide &s, const void *buf, int n, const int *counts, const int *displs, const MPI_Datatype *types,
                      MPI_Datatype one) {
    s.buf = (char *)buf;
    s.n = n;
    s.cnt.assign(counts, counts + n);
    s.dsp.resize(n), s.dt.resize(n);
    for (int j = 0; j < n; ++j) {
        s.dt[j] = types ? types[j] : one;
        // Alltoallw: bytes; Alltoallv: extents of the side's one type
        s.dsp[j] = !s.cnt[j] ? 0 : (types ? (long)displs[j] : (long)displs[j] * dtype_extent(one));
    }
}

// the runtime's view of the side; a staged side gets its buffer here
static int wside_plan(WSide &s) {
    s.bytes.assign(s.n, 0), s.offs.assign(s.n, 0);
    s.staged = false, s.total = 0;
    for (int j = 0; j < s.n; ++j) s.staged = s.staged || (s.cnt[j] && !plain_type(s.dt[j]));
    for (int j = 0; j < s.n; ++j) {
        if (!s.cnt[j]) continue;
        s.bytes[j] = (size_t)s.cnt[j] * (size_t)dtype_size(s.dt[j]);  // a zero-size type: as count 0
        s.offs[j] = s.staged ? s.total : (size_t)s.dsp[j];
        if (s.staged) s.total += (s.bytes[j] + 15) & ~(size_t)15;
    }
    if (s.staged && s.total && !(s.tmp = pool_get(s.total))) return MPI_ERR_NO_MEM;
    return MPI_SUCCESS;
}

// pack the user's blocks into the staging buffer, or unpack them out of it (gap bytes keep
// their value)
static int wside_move(WSide &s, bool unpack) {
    if (!s.staged || !s.total) return MPI_SUCCESS;
    long batched = 0;
    mv2h_get_info("pack_blocks", &batched);
    if (batched && s.n <= kMaxRanks && is_dev(s.buf)) {
        int64_t disp[kMaxRanks] = {};
        size_t count[kMaxRanks] = {}, extent[kMaxRanks] = {}, poff[kMaxRanks] = {};
        int first[kMaxRanks + 1];
        std::vector<int64_t> offs, lens;
        for (int j = 0; j < s.n; ++j) {
            first[j] = (int)offs.size();
            if (!s.bytes[j]) continue;  // an empty block: no segment
            disp[j] = s.dsp[j];
            poff[j] = s.offs[j];
            if (plain_type(s.dt[j])) {  // one element of the block's bytes
                count[j] = 1;
                extent[j] = s.bytes[j];
                offs.push_back(0), lens.push_back((int64_t)s.bytes[j]);
            } else {
                count[j] = (size_t)s.cnt[j];
                extent[j] = (size_t)dtype_extent(s.dt[j]);
                if (!dtype_flat(s.dt[j], offs, lens)) return MPI_ERR_TYPE;
            }
        }
        first[s.n] = (int)offs.size();
        return mv2h_pack_blocks(s.buf, s.tmp, s.n, disp, count, extent, poff, first, offs.data(), lens.data(), unpack,
                                nullptr);
    }
    int rc = MPI_SUCCESS;
    for (int j = 0; j < s.n && !rc; ++j) {
        if (!s.bytes[j]) continue;
        char *user = s.buf + s.dsp[j], *packed = (char *)s.tmp + s.offs[j];
        rc = unpack ? dtype_unpack(packed, s.cnt[j], s.dt[j], user) : dtype_pack(user, s.cnt[j], s.dt[j], packed);
    }
    return rc;
}

// Several nodes: refused like MPI_Alltoallv, here before any pack work.
static int a2aw_one_node_only(MPI_Comm comm, const char *fn) {
    long nnodes = 1;
    if (comm == MPI_COMM_SELF || mv2h_get_info("nnodes", &nnodes) || nnodes <= 1) return MPI_SUCCESS;
    MV2_ERR("%s: only jobs on one node are supported (this job spans %ld nodes)", fn, nnodes);
    return MPI_ERR_OTHER;
}

// S and R hold the blocks (wside_set); in place S is not read and the blocks leave from R's.
static int a2aw_run(WSide &S, WSide &R, bool in_place, MPI_Comm comm) {
    int rc = wside_plan(R);
    if (rc) return rc;
    if (in_place && !R.staged) {
        if (comm == MPI_COMM_SELF) return MPI_SUCCESS;
        return mv2h_alltoallv(MPI_IN_PLACE, nullptr, nullptr, R.buf, R.bytes.data(), R.offs.data(), nullptr);
    }
    if (in_place) {
        // a non-contiguous receive side: its blocks are packed into a send staging buffer, the
        // exchange fills a second one, and that is unpacked over them
        if (comm == MPI_COMM_SELF) return MPI_SUCCESS;
        S.buf = R.buf, S.n = R.n, S.cnt = R.cnt, S.dsp = R.dsp, S.dt = R.dt;
    }
    if ((rc = wside_plan(S)) || (rc = wside_move(S, false))) return rc;
    if (comm == MPI_COMM_SELF) {
        if (S.bytes[0] != R.bytes[0]) return MPI_ERR_TRUNCATE;
        rc = copy_any(R.rt_buf() + R.offs[0], S.rt_buf() + S.offs[0], R.bytes[0]);
    } else {
        rc = mv2h_alltoallv(S.rt_buf(), S.bytes.data(), S.offs.data(), R.rt_buf(), R.bytes.data(), R.offs.data(), nullptr);
    }
    return rc ? rc : wside_move(R, true);
}

// a displacement matters only where its count is not zero
static bool negative_displ(bool in_place, int n, const int *sendcounts, const int *sdispls, const int *recvcounts,
                           const int *rdispls) {
    for (int j = 0; j < n; ++j)
        if ((recvcounts[j] && rdispls[j] < 0) || (!in_place && sendcounts[j] && sdispls[j] < 0)) return true;
    return false;
}

// ---------------------------------------------------------------------------
// MPI_Gather(v) / MPI_Scatter(v) / MPI_Allgatherv.  Checks after gather.c:823-905, gatherv.c:
// 300-400, scatter.c:740-820, scatterv.c:240-330 and allgatherv.c:1090-1160: communicator, root,
// then per significant side count, type, committed and buffer; MPI_IN_PLACE only where the call
// has it (the send buffer of Allgatherv and of the root's Gather(v), the receive buffer of the
// root's Scatter(v)); the n-block side matters at the root only; a displacement matters only
// where its count is not zero.
//
// The runtime takes bytes and plain pointers, so a non-contiguous type is a local matter of the
// rank that has it: that rank packs its send side into a pooled device buffer (one PMPI_Pack per
// non-empty block on the side that owns n blocks, pos running on) or receives packed and unpacks
// the same way, and the collective itself moves packed bytes (as uniform_derived does).
// ---------------------------------------------------------------------------
// The side of a call that owns n blocks: block j is cnt[j] elements of dt at buf + dsp[j] extents.
// What the runtime sees of it is the user's buffer (contiguous type: bytes[j] at offs[j]) or, for
// a non-contiguous type, a packed copy with the blocks back to back.
struct NBlocks {
    char *buf = nullptr;
    MPI_Datatype dt = 0;
    int n = 0;
    std::vector<int> cnt, dsp;
    bool packed = false;
    void *tmp = nullptr;
    std::vector<size_t> bytes, offs;
    size_t total = 0;  // of the packed copy
    char *rt_buf() const { return packed ? (char *)tmp : buf; }
    ~NBlocks() {
        if (tmp) pool_put(tmp);
    }
};

// displs == nullptr: n blocks of counts[0] elements back to back (Gather / Scatter)
static int nblocks_init(NBlocks &b, const void *buf, int n, const int *counts, const int *displs, MPI_Datatype dt) {
    b.buf = (char *)buf;
    b.dt = dt;
    b.n = n;
    b.cnt.resize(n), b.dsp.resize(n), b.bytes.resize(n), b.offs.resize(n);
    b.packed = !dtype_is_contiguous(dt);
    const size_t ext = b.packed ? 0 : (size_t)dtype_span(dt, 1), size = (size_t)dtype_size(dt);
    for (int j = 0; j < n; ++j) {
        b.cnt[j] = displs ? counts[j] : counts[0];
        b.dsp[j] = displs ? (b.cnt[j] ? displs[j] : 0) : j * counts[0];
        if (b.cnt[j] && b.dsp[j] < 0) return MPI_ERR_ARG;
        b.bytes[j] = (size_t)b.cnt[j] * (b.packed ? size : ext);
        b.offs[j] = b.packed ? b.total : (size_t)b.dsp[j] * ext;
        b.total += b.packed ? b.bytes[j] : 0;
    }
    if (b.packed && b.total && !(b.tmp = pool_get(b.total))) return MPI_ERR_NO_MEM;
    return MPI_SUCCESS;
}

static int nblocks_pack(NBlocks &b, MPI_Comm comm) {
    int pos = 0, rc = MPI_SUCCESS;
    const long ext = dtype_extent(b.dt);
    for (int j = 0; j < b.n && !rc; ++j)
        if (b.cnt[j]) rc = PMPI_Pack(b.buf + (long)b.dsp[j] * ext, b.cnt[j], b.dt, b.tmp, (int)b.total, &pos, comm);
    return rc;
}

static int nblocks_unpack(NBlocks &b, int skip, MPI_Comm comm) {
    int pos = 0, rc = MPI_SUCCESS;
    const long ext = dtype_extent(b.dt);
    for (int j = 0; j < b.n && !rc; ++j) {
        if (!b.cnt[j]) continue;
        if (j == skip) pos += (int)b.bytes[j];
        else rc = PMPI_Unpack(b.tmp, (int)b.total, &pos, b.buf + (long)b.dsp[j] * ext, b.cnt[j], b.dt, comm);
    }
    return rc;
}

// One block of `count` elements of dt as the runtime reads (pack = true) or writes it: the
// user's buffer, or a pooled packed copy for a non-contiguous type.
struct OneBlock {
    void *user = nullptr, *tmp = nullptr;
    int count = 0;
    MPI_Datatype dt = 0;
    size_t bytes = 0;
    void *rt_buf() const { return tmp ? tmp : user; }
    ~OneBlock() {
        if (tmp) pool_put(tmp);
    }
};
static int oneblock_init(OneBlock &o, const void *buf, int count, MPI_Datatype dt, bool pack, MPI_Comm comm) {
    o.user = (void *)buf;
    o.count = count;
    o.dt = dt;
    if (dtype_is_contiguous(dt)) {
        o.bytes = (size_t)dtype_span(dt, count);
        return MPI_SUCCESS;
    }
    o.bytes = (size_t)dtype_size(dt) * (size_t)count;
    if (!o.bytes) return MPI_SUCCESS;
    if (!(o.tmp = pool_get(o.bytes))) return MPI_ERR_NO_MEM;
    int pos = 0;
    return pack ? PMPI_Pack(buf, count, dt, o.tmp, (int)o.bytes, &pos, comm) : MPI_SUCCESS;
}

// Allgatherv / Gather(v): my block goes out, the n-block side `rb` (nullptr where it is not
// significant) comes in.  call(send, sbytes, recv, rbytes, roffs) is the runtime's collective.
template <class Call>
static int gather_like(const void *sendbuf, int sendcount, MPI_Datatype sendtype, NBlocks *rb, int me, MPI_Comm comm,
                       Call call) {
    const bool in_place = sendbuf == MPI_IN_PLACE;
    OneBlock s;
    int rc = MPI_SUCCESS;
    if (in_place && rb->packed)  // my block out of the receive side, packed; in place no longer
        rc = oneblock_init(s, rb->buf + (long)rb->dsp[me] * dtype_extent(rb->dt), rb->cnt[me], rb->dt, true, comm);
    else if (in_place) s.user = MPI_IN_PLACE, s.bytes = rb->bytes[me];
    else rc = oneblock_init(s, sendbuf, sendcount, sendtype, true, comm);
    if (rc) return rc;
    if (comm == MPI_COMM_SELF) {
        if (s.rt_buf() != MPI_IN_PLACE) {
            if (s.bytes != rb->bytes[0]) return MPI_ERR_TRUNCATE;
            rc = copy_any(rb->rt_buf() + rb->offs[0], s.rt_buf(), s.bytes);
        }
    } else {
        rc = call(s.rt_buf(), s.bytes, rb ? rb->rt_buf() : nullptr, rb ? rb->bytes.data() : nullptr,
                  rb ? rb->offs.data() : nullptr);
    }
    if (!rc && rb && rb->packed && rb->total) rc = nblocks_unpack(*rb, in_place ? me : -1, comm);
    return rc;
}

// Scatter(v): the n-block side `sb` (the root's) goes out, my block comes in.
// call(send, sbytes, soffs, recv, rbytes) is the runtime's collective.
template <class Call>
static int scatter_like(NBlocks *sb, void *recvbuf, int recvcount, MPI_Datatype recvtype, MPI_Comm comm, Call call) {
    const bool in_place = recvbuf == MPI_IN_PLACE;
    int rc = MPI_SUCCESS;
    if (sb && sb->packed && sb->total && (rc = nblocks_pack(*sb, comm))) return rc;
    OneBlock r;
    if (in_place) r.user = MPI_IN_PLACE;
    else if ((rc = oneblock_init(r, recvbuf, recvcount, recvtype, false, comm))) return rc;
    if (comm == MPI_COMM_SELF) {
        if (!in_place) {
            if (r.bytes != sb->bytes[0]) return MPI_ERR_TRUNCATE;
            rc = copy_any(r.rt_buf(), sb->rt_buf() + sb->offs[0], r.bytes);
        }
    } else {
        rc = call(sb ? sb->rt_buf() : nullptr, sb ? sb->bytes.data() : nullptr, sb ? sb->offs.data() : nullptr, r.rt_buf(),
                  r.bytes);
    }
    if (!rc && r.tmp) {
        int pos = 0;
        rc = PMPI_Unpack(r.tmp, (int)r.bytes, &pos, recvbuf, recvcount, recvtype, comm);
    }
    return rc;
}

// The preamble of a rooted call: comm_checks, then the root (MPI_ERR_ROOT)
static int rooted_comm_checks(MPI_Comm comm, int root, int *n, int *me) {
    if (const int rc = comm_checks(comm, n, me)) return rc;
    const int csize = comm == MPI_COMM_SELF ? 1 : world().gsize;
    if (root < 0 || root >= csize) return MPI_ERR_ROOT;
    return MPI_SUCCESS;
}

// a side of one block that is significant here: count, type, committed, buffer
static int block_checks(const void *buf, int count, MPI_Datatype dt) {
    if (const int rc = side_checks(count, dt)) return rc;
    return inplace_buf(buf, count) || null_userbuf(buf, count, dt) ? MPI_ERR_BUFFER : MPI_SUCCESS;
}

// the side of n blocks (its arrays are there): n counts non-negative, type, committed, buffer
static int nblock_checks(const void *buf, const int *counts, int n, MPI_Datatype dt) {
    long total = 0;
    for (int j = 0; j < n; ++j) {
        if (counts[j] < 0) return MPI_ERR_COUNT;
        total += counts[j];
    }
    if (const int rc = side_checks(0, dt)) return rc;
    return inplace_buf(buf, total) || null_userbuf(buf, total, dt) ? MPI_ERR_BUFFER : MPI_SUCCESS;
}

// What MPI_Gather and MPI_Gatherv begin with: communicator and root, MPI_IN_PLACE off the root,
// the send side
static int gather_prologue(const void *sendbuf, int sendcount, MPI_Datatype sendtype, int root, MPI_Comm comm, int *n,
                           int *me) {
    if (const int rc = rooted_comm_checks(comm, root, n, me)) return rc;
    if (sendbuf == MPI_IN_PLACE) return *me == root ? MPI_SUCCESS : MPI_ERR_BUFFER;
    return block_checks(sendbuf, sendcount, sendtype);
}

// What MPI_Scatter and MPI_Scatterv begin with: communicator and root, MPI_IN_PLACE off the root
static int scatter_prologue(const void *recvbuf, int root, MPI_Comm comm, int *n, int *me) {
    if (const int rc = rooted_comm_checks(comm, root, n, me)) return rc;
    return recvbuf == MPI_IN_PLACE && *me != root ? MPI_ERR_BUFFER : MPI_SUCCESS;
}

extern "C" {

MPI_API(Allgather, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
        MPI_Datatype recvtype, MPI_Comm comm) {
    CsLock lk;
    return allgather_call<false>(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm, nullptr, "MPI_Allgather");
}

MPIX_API(Allgather_enqueue, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
         MPI_Datatype recvtype, MPI_Comm comm, void *stream) {
    CsLock lk;
    return allgather_call<true>(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm, stream,
                                "MPIX_Allgather_enqueue");
}

MPI_API(Alltoall, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
        MPI_Datatype recvtype, MPI_Comm comm) {
    CsLock lk;
    return alltoall_call<false>(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm, nullptr, "MPI_Alltoall");
}

MPIX_API(Alltoall_enqueue, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
         MPI_Datatype recvtype, MPI_Comm comm, void *stream) {
    CsLock lk;
    return alltoall_call<true>(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm, stream,
                               "MPIX_Alltoall_enqueue");
}

// Counts and displacements are in elements (extents) of their side's type, as in the reference; the
// runtime takes bytes.  A non-contiguous type on either side goes the way of MPI_Alltoallw.
MPI_API(Alltoallv, const void *sendbuf, const int sendcounts[], const int sdispls[], MPI_Datatype sendtype,
        void *recvbuf, const int recvcounts[], const int rdispls[], MPI_Datatype recvtype, MPI_Comm comm) {
    CsLock lk;
    const char *fn = "MPI_Alltoallv";
    int n = 1, rc;
    if ((rc = comm_checks(comm, &n))) return err_return(comm, rc, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!recvcounts || !rdispls || (!in_place && (!sendcounts || !sdispls))) return err_return(comm, MPI_ERR_ARG, fn);
    long stotal = 0, rtotal = 0;
    for (int j = 0; j < n; ++j) {
        if (recvcounts[j] < 0 || (!in_place && sendcounts[j] < 0)) return err_return(comm, MPI_ERR_COUNT, fn);
        rtotal += recvcounts[j];
        if (!in_place) stotal += sendcounts[j];
    }
    if ((rc = pair_checks(in_place, 0, sendtype, 0, recvtype))) return err_return(comm, rc, fn);
    if (!in_place && null_userbuf(sendbuf, stotal, sendtype)) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (inplace_buf(recvbuf, rtotal) || null_userbuf(recvbuf, rtotal, recvtype)) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (!in_place && stotal && rtotal && sendbuf == recvbuf) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (negative_displ(in_place, n, sendcounts, sdispls, recvcounts, rdispls)) return err_return(comm, MPI_ERR_ARG, fn);
    if (!dtype_is_contiguous(recvtype) || (!in_place && !dtype_is_contiguous(sendtype))) {
        if ((rc = a2aw_one_node_only(comm, fn))) return err_return(comm, rc, fn);
        WSide S, R;
        wside_set(R, recvbuf, n, recvcounts, rdispls, nullptr, recvtype);
        if (!in_place) wside_set(S, sendbuf, n, sendcounts, sdispls, nullptr, sendtype);
        return err_return(comm, a2aw_run(S, R, in_place, comm), fn);
    }
    const size_t rext = (size_t)dtype_span(recvtype, 1), sext = in_place ? rext : (size_t)dtype_span(sendtype, 1);
    std::vector<size_t> sb(n), so(n), rb(n), ro(n);
    for (int j = 0; j < n; ++j) {
        rb[j] = (size_t)recvcounts[j] * rext;
        ro[j] = recvcounts[j] ? (size_t)rdispls[j] * rext : 0;
        sb[j] = in_place ? rb[j] : (size_t)sendcounts[j] * sext;
        so[j] = in_place ? ro[j] : (sendcounts[j] ? (size_t)sdispls[j] * sext : 0);
    }
    if (comm == MPI_COMM_SELF) {
        if (sb[0] != rb[0]) return err_return(comm, MPI_ERR_TRUNCATE, fn);
        if (!in_place) rc = copy_any((char *)recvbuf + ro[0], (const char *)sendbuf + so[0], rb[0]);
        return err_return(comm, rc, fn);
    }
    return err_return(comm, mv2h_alltoallv(sendbuf, sb.data(), so.data(), recvbuf, rb.data(), ro.data(), nullptr), fn);
}

// Checks in MPI_Alltoallv's order here: communicator, arrays, then per block count, type and
// committed (a type matters only where its count is not zero, alltoallw.c:483-507), the buffers
// (:509-521), the alias check (:474-475).  MPI_IN_PLACE takes counts, displacements and types from
// the receive side.  Displacements are bytes; one matters only where its count is not zero.
MPI_API(Alltoallw, const void *sendbuf, const int sendcounts[], const int sdispls[], const MPI_Datatype sendtypes[],
        void *recvbuf, const int recvcounts[], const int rdispls[], const MPI_Datatype recvtypes[], MPI_Comm comm) {
    CsLock lk;
    const char *fn = "MPI_Alltoallw";
    int n = 1, rc;
    if ((rc = comm_checks(comm, &n))) return err_return(comm, rc, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!recvcounts || !rdispls || !recvtypes || (!in_place && (!sendcounts || !sdispls || !sendtypes)))
        return err_return(comm, MPI_ERR_ARG, fn);
    int s1 = -1, r1 = -1;  // the first non-empty block of each side
    for (int j = 0; j < n; ++j) {
        if (!in_place) {
            if (sendcounts[j] < 0) return err_return(comm, MPI_ERR_COUNT, fn);
            if (sendcounts[j] > 0 && (!dtype_valid(sendtypes[j]) || !dtype_committed(sendtypes[j])))
                return err_return(comm, MPI_ERR_TYPE, fn);
            if (sendcounts[j] > 0 && s1 < 0) s1 = j;
        }
        if (recvcounts[j] < 0) return err_return(comm, MPI_ERR_COUNT, fn);
        if (recvcounts[j] > 0 && (!dtype_valid(recvtypes[j]) || !dtype_committed(recvtypes[j])))
            return err_return(comm, MPI_ERR_TYPE, fn);
        if (recvcounts[j] > 0 && r1 < 0) r1 = j;
    }
    if (s1 >= 0 && null_userbuf(sendbuf, sendcounts[s1], sendtypes[s1])) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (r1 >= 0 && (inplace_buf(recvbuf, recvcounts[r1]) || null_userbuf(recvbuf, recvcounts[r1], recvtypes[r1])))
        return err_return(comm, MPI_ERR_BUFFER, fn);
    if (!in_place && sendcounts == recvcounts && sendtypes == recvtypes && sendbuf == recvbuf)
        return err_return(comm, MPI_ERR_BUFFER, fn);
    if (negative_displ(in_place, n, sendcounts, sdispls, recvcounts, rdispls)) return err_return(comm, MPI_ERR_ARG, fn);
    if ((rc = a2aw_one_node_only(comm, fn))) return err_return(comm, rc, fn);
    WSide S, R;
    wside_set(R, recvbuf, n, recvcounts, rdispls, recvtypes, MPI_DATATYPE_NULL);
    if (!in_place) wside_set(S, sendbuf, n, sendcounts, sdispls, sendtypes, MPI_DATATYPE_NULL);
    return err_return(comm, a2aw_run(S, R, in_place, comm), fn);
}

MPI_API(Gather, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
        MPI_Datatype recvtype, int root, MPI_Comm comm) {
    CsLock lk;
    const char *fn = "MPI_Gather";
    int n = 1, me = 0, rc;
    if ((rc = gather_prologue(sendbuf, sendcount, sendtype, root, comm, &n, &me))) return err_return(comm, rc, fn);
    const bool at_root = me == root;
    NBlocks rb;
    if (at_root) {
        if ((rc = block_checks(recvbuf, recvcount, recvtype))) return err_return(comm, rc, fn);
        // gather.c:880-886: the send buffer is the root's own block of the receive buffer
        if (sendbuf != MPI_IN_PLACE && sendtype == recvtype && sendcount != 0 && recvcount != 0 &&
            sendbuf == (const char *)recvbuf + (long)me * recvcount * dtype_size(recvtype))
            return err_return(comm, MPI_ERR_BUFFER, fn);
        if ((rc = nblocks_init(rb, recvbuf, n, &recvcount, nullptr, recvtype))) return err_return(comm, rc, fn);
        if (!recvcount) return MPI_SUCCESS;
    } else if (!sendcount || !dtype_size(sendtype)) {
        return MPI_SUCCESS;
    }
    rc = gather_like(sendbuf, sendcount, sendtype, at_root ? &rb : nullptr, me, comm,
                     [&](const void *s, size_t sbytes, void *r, const size_t *rbytes, const size_t *) {
                         const size_t bytes = rbytes ? rbytes[me] : sbytes;
                         if (rbytes && s != MPI_IN_PLACE && sbytes != bytes) return (int)MPI_ERR_TRUNCATE;
                         return mv2h_gather(s, r, bytes, root, nullptr);
                     });
    return err_return(comm, rc, fn);
}

MPI_API(Gatherv, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
        const int displs[], MPI_Datatype recvtype, int root, MPI_Comm comm) {
    CsLock lk;
    const char *fn = "MPI_Gatherv";
    int n = 1, me = 0, rc;
    if ((rc = gather_prologue(sendbuf, sendcount, sendtype, root, comm, &n, &me))) return err_return(comm, rc, fn);
    const bool at_root = me == root;
    NBlocks rb;
    if (at_root) {
        if (!recvcounts || !displs) return err_return(comm, MPI_ERR_ARG, fn);
        if ((rc = nblock_checks(recvbuf, recvcounts, n, recvtype))) return err_return(comm, rc, fn);
        if ((rc = nblocks_init(rb, recvbuf, n, recvcounts, displs, recvtype))) return err_return(comm, rc, fn);
    }
    rc = gather_like(sendbuf, sendcount, sendtype, at_root ? &rb : nullptr, me, comm,
                     [&](const void *s, size_t sbytes, void *r, const size_t *rbytes, const size_t *roffs) {
                         return mv2h_gatherv(s, sbytes, r, rbytes, roffs, root, nullptr);
                     });
    return err_return(comm, rc, fn);
}

MPI_API(Allgatherv, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
        const int displs[], MPI_Datatype recvtype, MPI_Comm comm) {
    CsLock lk;
    const char *fn = "MPI_Allgatherv";
    int n = 1, me = 0, rc;
    if ((rc = comm_checks(comm, &n, &me))) return err_return(comm, rc, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!recvcounts || !displs) return err_return(comm, MPI_ERR_ARG, fn);
    if (!in_place && (rc = block_checks(sendbuf, sendcount, sendtype))) return err_return(comm, rc, fn);
    if ((rc = nblock_checks(recvbuf, recvcounts, n, recvtype))) return err_return(comm, rc, fn);
    // allgatherv.c:1118-1124: the send buffer is this rank's block of the receive buffer
    if (!in_place && sendtype == recvtype && sendcount != 0 && recvcounts[me] != 0 &&
        sendbuf == (const char *)recvbuf + (long)displs[me] * dtype_size(recvtype))
        return err_return(comm, MPI_ERR_BUFFER, fn);
    NBlocks rb;
    if ((rc = nblocks_init(rb, recvbuf, n, recvcounts, displs, recvtype))) return err_return(comm, rc, fn);
    rc = gather_like(sendbuf, sendcount, sendtype, &rb, me, comm,
                     [&](const void *s, size_t sbytes, void *r, const size_t *rbytes, const size_t *roffs) {
                         return mv2h_allgatherv(s, sbytes, r, rbytes, roffs, nullptr);
                     });
    return err_return(comm, rc, fn);
}

MPI_API(Scatter, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
        MPI_Datatype recvtype, int root, MPI_Comm comm) {
    CsLock lk;
    const char *fn = "MPI_Scatter";
    int n = 1, me = 0, rc;
    if ((rc = scatter_prologue(recvbuf, root, comm, &n, &me))) return err_return(comm, rc, fn);
    const bool at_root = me == root, in_place = recvbuf == MPI_IN_PLACE;
    NBlocks sb;
    if (at_root && (rc = block_checks(sendbuf, sendcount, sendtype))) return err_return(comm, rc, fn);
    if (!in_place && (rc = block_checks(recvbuf, recvcount, recvtype))) return err_return(comm, rc, fn);
    if (at_root) {
        // scatter.c:790-796: the receive buffer is the root's own block of the send buffer
        if (!in_place && sendtype == recvtype && sendcount != 0 && recvcount != 0 &&
            recvbuf == (const char *)sendbuf + (long)me * sendcount * dtype_size(sendtype))
            return err_return(comm, MPI_ERR_BUFFER, fn);
        if ((rc = nblocks_init(sb, sendbuf, n, &sendcount, nullptr, sendtype))) return err_return(comm, rc, fn);
        if (!sendcount) return MPI_SUCCESS;
    } else if (!recvcount || !dtype_size(recvtype)) {
        return MPI_SUCCESS;
    }
    rc = scatter_like(at_root ? &sb : nullptr, recvbuf, recvcount, recvtype, comm,
                      [&](const void *s, const size_t *sbytes, const size_t *, void *r, size_t rbytes) {
                          const size_t bytes = sbytes ? sbytes[me] : rbytes;
                          if (sbytes && r != MPI_IN_PLACE && rbytes != bytes) return (int)MPI_ERR_TRUNCATE;
                          return mv2h_scatter(s, r, bytes, root, nullptr);
                      });
    return err_return(comm, rc, fn);
}

MPI_API(Scatterv, const void *sendbuf, const int sendcounts[], const int displs[], MPI_Datatype sendtype, void *recvbuf,
        int recvcount, MPI_Datatype recvtype, int root, MPI_Comm comm) {
    CsLock lk;
    const char *fn = "MPI_Scatterv";
    int n = 1, me = 0, rc;
    if ((rc = scatter_prologue(recvbuf, root, comm, &n, &me))) return err_return(comm, rc, fn);
    const bool at_root = me == root, in_place = recvbuf == MPI_IN_PLACE;
    NBlocks sb;
    if (at_root) {
        if (!sendcounts || !displs) return err_return(comm, MPI_ERR_ARG, fn);
        if ((rc = nblock_checks(sendbuf, sendcounts, n, sendtype))) return err_return(comm, rc, fn);
    }
    if (!in_place && (rc = block_checks(recvbuf, recvcount, recvtype))) return err_return(comm, rc, fn);
    if (at_root && (rc = nblocks_init(sb, sendbuf, n, sendcounts, displs, sendtype))) return err_return(comm, rc, fn);
    rc = scatter_like(at_root ? &sb : nullptr, recvbuf, recvcount, recvtype, comm,
                      [&](const void *s, const size_t *sbytes, const size_t *soffs, void *r, size_t rbytes) {
                          return mv2h_scatterv(s, sbytes, soffs, r, rbytes, root, nullptr);
                      });
    return err_return(comm, rc, fn);
}

MPI_API(Bcast, void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm) {
    CsLock lk;
    const char *fn = "MPI_Bcast";
    int size = 1, rc;
    if ((rc = comm_checks(comm, &size))) return err_return(comm, rc, fn);
    if (count < 0) return err_return(comm, MPI_ERR_COUNT, fn);
    if (!dtype_valid(dt)) return err_return(comm, MPI_ERR_TYPE, fn);
    if (root < 0 || root >= size) return err_return(comm, MPI_ERR_ROOT, fn);
    if (!dtype_committed(dt)) return err_return(comm, MPI_ERR_TYPE, fn);
    if (inplace_buf(buffer, count) || null_userbuf(buffer, count, dt)) return err_return(comm, MPI_ERR_BUFFER, fn);  // bcast.c:1581-1582
    if (count == 0 || size == 1) return MPI_SUCCESS;
    if (dtype_is_contiguous(dt)) return err_return(comm, mv2h_bcast(buffer, (size_t)dtype_span(dt, count), root, nullptr), fn);
    // derived (non-contiguous) type: pack on device at the root, broadcast the
    // packed bytes, unpack on device everywhere else
    int psize = 0;
    PMPI_Pack_size(count, dt, comm, &psize);
    void *packed = pool_get((size_t)psize);
    if (!packed) return err_return(comm, MPI_ERR_NO_MEM, fn);
    int pos = 0;
    if (mv2h_rank() == root) rc = PMPI_Pack(buffer, count, dt, packed, psize, &pos, comm);
    if (!rc) rc = mv2h_bcast(packed, (size_t)psize, root, nullptr);
    pos = 0;
    if (!rc && mv2h_rank() != root) rc = PMPI_Unpack(packed, psize, &pos, buffer, count, dt, comm);
    pool_put(packed);
    return err_return(comm, rc, fn);
}

MPIX_API(Bcast_enqueue, void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm, void *stream) {
    CsLock lk;
    const char *fn = "MPIX_Bcast_enqueue";
    int size = 1;
    if (const int rc = comm_checks(comm, &size)) return err_return(comm, rc, fn);
    if (!stream) return err_return(comm, MPI_ERR_ARG, fn);
    if (const int rc = side_checks(count, dt)) return err_return(comm, rc, fn);
    if (!dtype_is_contiguous(dt)) return err_return(comm, MPI_ERR_TYPE, fn);
    if (root < 0 || root >= size) return err_return(comm, MPI_ERR_ROOT, fn);
    if (inplace_buf(buffer, count) || null_userbuf(buffer, count, dt)) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (count == 0 || size == 1) return MPI_SUCCESS;
    return err_return(comm, mv2h_bcast_enqueue(buffer, (size_t)dtype_span(dt, count), root, stream), fn);
}

MPIX_API(Enqueue_check, MPI_Comm comm) {
    CsLock lk;
    if (comm_index(comm) < 0) return err_return(comm, MPI_ERR_COMM, "MPIX_Enqueue_check");
    return err_return(comm, mv2h_enqueue_check(), "MPIX_Enqueue_check");
}

}  // extern "C"

// api_request.cpp — the request table, the nonblocking collectives, completion calls and
// point-to-point (api_internal.h has the front end's shared state and checks).
// One table for nonblocking collectives (completion-word tickets, mv2h_defer_*)
// and point-to-point requests (mv2h_isend / mv2h_irecv ids).  Handles are
// kReqBase | slot; MPI_REQUEST_NULL is MPICH's 0x2c000000.
#include <sched.h>
#include <stdlib.h>

#include "../runtime/world.h"
#include "api_internal.h"

using namespace mv2;

namespace {
enum ReqKind { RQ_COLL = 1, RQ_P2P = 2, RQ_DONE = 3 };
struct MReq {
    int kind = 0;
    unsigned long long id = 0;
    bool live = false;
    bool is_recv = false;
    int src = MPI_ANY_SOURCE, tag = MPI_ANY_TAG;  // RQ_DONE status
    // derived-type staging: send keeps its packed copy, receive unpacks at completion
    void *tmp = nullptr;
    bool tmp_dev = false;
    int tmp_bytes = 0;
    void *ubuf = nullptr;
    MPI_Datatype dt = MPI_DATATYPE_NULL;
    int err = MPI_SUCCESS;  // a collective's error found by a peek (MPI_Testall), reported at completion
};
}  // namespace
static std::vector<MReq> g_mreqs;
constexpr MPI_Request kReqBase = (MPI_Request)0xac000000;

static MPI_Request req_new(const MReq &r) {
    for (size_t i = 0; i < g_mreqs.size(); ++i)
        if (!g_mreqs[i].live) {
            g_mreqs[i] = r;
            g_mreqs[i].live = true;
            return kReqBase | (MPI_Request)i;
        }
    g_mreqs.push_back(r);
    g_mreqs.back().live = true;
    return kReqBase | (MPI_Request)(g_mreqs.size() - 1);
}

static MReq *req_get(MPI_Request h) {
    if ((h & 0xfc000000) != (kReqBase & 0xfc000000)) return nullptr;
    const size_t i = (size_t)(h & 0x03ffffff);
    return i < g_mreqs.size() && g_mreqs[i].live ? &g_mreqs[i] : nullptr;
}

static void status_set(MPI_Status *st, int src, int tag, size_t bytes, int err) {
    if (!st || st == MPI_STATUS_IGNORE) return;
    st->MPI_SOURCE = src;
    st->MPI_TAG = tag;
    st->MPI_ERROR = err;
    st->count_lo = (int)(bytes & 0xffffffffu);
    st->count_hi_and_cancelled = (int)((bytes >> 32) << 1);
}

// a derived type's packed copy: pooled device memory beside a device buffer, else malloc'd
static int tmp_alloc(MReq &r, const void *buf, int count, MPI_Datatype dt, int *psize) {
    PMPI_Pack_size(count, dt, MPI_COMM_WORLD, psize);
    r.tmp_dev = is_dev(buf);
    r.tmp = r.tmp_dev ? pool_get((size_t)*psize) : malloc((size_t)*psize + 1);
    return r.tmp ? MPI_SUCCESS : MPI_ERR_NO_MEM;
}

static void tmp_free(MReq &r) {
    if (!r.tmp) return;
    if (r.tmp_dev) pool_put(r.tmp);
    else free(r.tmp);
    r.tmp = nullptr;
}

// finish a request whose underlying operation completed (rc = its error class)
static int req_finish(MReq &r, int rc, int src, int tag, size_t bytes, MPI_Status *st) {
    if (r.kind == RQ_P2P && r.is_recv && r.tmp && (rc == MPI_SUCCESS || rc == MPI_ERR_TRUNCATE)) {
        const long tsz = dtype_size(r.dt);
        const int nel = tsz > 0 ? (int)(bytes / (size_t)tsz) : 0;
        int pos = 0;
        const int urc = PMPI_Unpack(r.tmp, (int)bytes, &pos, r.ubuf, nel, r.dt, MPI_COMM_WORLD);
        if (rc == MPI_SUCCESS) rc = urc;
    }
    tmp_free(r);
    if (r.kind == RQ_COLL) status_set(st, MPI_ANY_SOURCE, MPI_ANY_TAG, 0, rc);
    else if (r.kind == RQ_DONE) status_set(st, r.src, r.tag, 0, rc);
    else if (r.is_recv) status_set(st, src, tag, bytes, rc);
    else status_set(st, MPI_ANY_SOURCE, MPI_ANY_TAG, 0, rc);
    r.live = false;
    return rc;
}

static int req_wait(MReq &r, MPI_Status *st) {
    int src = MPI_ANY_SOURCE, tag = MPI_ANY_TAG, rc = MPI_SUCCESS;
    size_t bytes = 0;
    if (r.kind == RQ_COLL) rc = r.err ? r.err : mv2h_wait_ticket(r.id);
    else if (r.kind == RQ_P2P) rc = mv2h_p2p_wait(r.id, &src, &tag, &bytes);
    return req_finish(r, rc, src, tag, bytes, st);
}

static int req_test(MReq &r, int *flag, MPI_Status *st) {
    int src = MPI_ANY_SOURCE, tag = MPI_ANY_TAG, rc = MPI_SUCCESS, done = 1;
    size_t bytes = 0;
    if (r.kind == RQ_COLL) rc = r.err ? r.err : mv2h_test_ticket(r.id, &done);
    else if (r.kind == RQ_P2P) rc = mv2h_p2p_test(r.id, &done, &src, &tag, &bytes);
    *flag = done;
    if (!done && rc == MPI_SUCCESS) return MPI_SUCCESS;
    *flag = 1;
    return req_finish(r, rc, src, tag, bytes, st);
}

// nonblocking collective = the blocking implementation initiated with
// deferred completion (the kernel is enqueued, the ticket waits later)
template <class F>
static int start_coll(MPI_Request *request, const char *fn, F &&call, int nbc = MV2H_NBC_NONE) {
    if (!request) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, fn);
    mv2h_defer_begin();
    mv2h_nbc_begin(nbc);  // the nonblocking selection and reduction order (runtime/orders.h)
    const int rc = call();
    mv2h_nbc_end();
    unsigned long long t = 0;
    mv2h_defer_end(&t);
    if (rc) return rc;  // already passed through the error handler
    MReq r;
    r.kind = RQ_COLL;
    r.id = t;
    *request = req_new(r);
    return MPI_SUCCESS;
}

static int p2p_checks(MPI_Comm comm, int count, MPI_Datatype dt, int tag, bool recv) {
    if (!g_initialized) return MPI_ERR_OTHER;
    if (comm != MPI_COMM_WORLD) return comm_index(comm) < 0 ? MPI_ERR_COMM : MPI_ERR_UNSUPPORTED_OPERATION;
    if (const int rc = side_checks(count, dt)) return rc;
    if (recv ? (tag < 0 && tag != MPI_ANY_TAG) : tag < 0) return MPI_ERR_TAG;
    return MPI_SUCCESS;
}

// a request that is complete when made (MPI_PROC_NULL)
static int req_done(MReq &r, MPI_Request *request) {
    r.kind = RQ_DONE;
    r.src = MPI_PROC_NULL;
    *request = req_new(r);
    return MPI_SUCCESS;
}

static int isend_impl(const void *buf, int count, MPI_Datatype dt, int dest, int tag, MPI_Request *request) {
    MReq r;
    if (dest == MPI_PROC_NULL) return req_done(r, request);
    if (dest < 0 || dest >= world().gsize) return MPI_ERR_RANK;
    r.kind = RQ_P2P;
    const void *src = buf;
    size_t bytes = (size_t)dtype_span(dt, count);
    int rc = MPI_SUCCESS;
    if (!dtype_is_contiguous(dt)) {  // device (or host) pack first, the packed copy travels
        int psize = 0, pos = 0;
        if ((rc = tmp_alloc(r, buf, count, dt, &psize))) return rc;
        rc = PMPI_Pack(buf, count, dt, r.tmp, psize, &pos, MPI_COMM_WORLD);
        src = r.tmp;
        bytes = (size_t)pos;
    }
    if (!rc) rc = mv2h_isend(src, bytes, dest, tag, &r.id);
    if (rc) {
        tmp_free(r);
        return rc;
    }
    *request = req_new(r);
    return MPI_SUCCESS;
}

static int irecv_impl(void *buf, int count, MPI_Datatype dt, int source, int tag, MPI_Request *request) {
    MReq r;
    r.is_recv = true;
    if (source == MPI_PROC_NULL) return req_done(r, request);
    if (source != MPI_ANY_SOURCE && (source < 0 || source >= world().gsize)) return MPI_ERR_RANK;
    r.kind = RQ_P2P;
    void *dst = buf;
    size_t cap = (size_t)dtype_span(dt, count);
    if (!dtype_is_contiguous(dt)) {  // receive packed, unpack at completion
        int psize = 0;
        if (const int rc = tmp_alloc(r, buf, count, dt, &psize)) return rc;
        r.ubuf = buf;
        r.dt = dt;
        dst = r.tmp;
        cap = (size_t)psize;
    }
    const int rc = mv2h_irecv(dst, cap, source, tag, &r.id);
    if (rc) {
        tmp_free(r);
        return rc;
    }
    *request = req_new(r);
    return MPI_SUCCESS;
}

extern "C" {

// ---------------------------------------------------------------- nonblocking collectives
MPI_API(Iallreduce, const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
        MPI_Request *request) {
    CsLock lk;
    return start_coll(
        request, "MPI_Iallreduce", [&] { return PMPI_Allreduce(sendbuf, recvbuf, count, dt, op, comm); },
        MV2H_NBC_IALLREDUCE);
}

// the schedules make MPIR_Scan_generic's / MPIR_Exscan's calls in the same order (iscan.c:72-160,
// iexscan.c): the blocking programs
MPI_API(Iscan, const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
        MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Iscan", [&] { return PMPI_Scan(sendbuf, recvbuf, count, dt, op, comm); });
}

MPI_API(Iexscan, const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
        MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Iexscan", [&] { return PMPI_Exscan(sendbuf, recvbuf, count, dt, op, comm); });
}

MPI_API(Ireduce, const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, int root, MPI_Comm comm,
        MPI_Request *request) {
    CsLock lk;
    return start_coll(
        request, "MPI_Ireduce", [&] { return PMPI_Reduce(sendbuf, recvbuf, count, dt, op, root, comm); },
        MV2H_NBC_IREDUCE);
}

MPI_API(Ireduce_scatter, const void *sendbuf, void *recvbuf, const int recvcounts[], MPI_Datatype dt, MPI_Op op,
        MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(
        request, "MPI_Ireduce_scatter", [&] { return PMPI_Reduce_scatter(sendbuf, recvbuf, recvcounts, dt, op, comm); },
        MV2H_NBC_IREDUCE_SCATTER);
}

MPI_API(Ireduce_scatter_block, const void *sendbuf, void *recvbuf, int recvcount, MPI_Datatype dt, MPI_Op op,
        MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(
        request, "MPI_Ireduce_scatter_block",
        [&] { return PMPI_Reduce_scatter_block(sendbuf, recvbuf, recvcount, dt, op, comm); },
        MV2H_NBC_IREDUCE_SCATTER_BLOCK);
}

MPI_API(Iallgather, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
        MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Iallgather", [&] {
        return PMPI_Allgather(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm);
    });
}

MPI_API(Ialltoall, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
        MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Ialltoall", [&] {
        return PMPI_Alltoall(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm);
    });
}

// The ranks exchange their counts on the host at initiation (two host barriers), so initiation is
// not local: it returns once every rank of the node has initiated the call.  The data moves behind
// the request.
MPI_API(Ialltoallv, const void *sendbuf, const int sendcounts[], const int sdispls[], MPI_Datatype sendtype,
        void *recvbuf, const int recvcounts[], const int rdispls[], MPI_Datatype recvtype, MPI_Comm comm,
        MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Ialltoallv", [&] {
        return PMPI_Alltoallv(sendbuf, sendcounts, sdispls, sendtype, recvbuf, recvcounts, rdispls, recvtype, comm);
    });
}

// As MPI_Ialltoallv: the counts are exchanged on the host at initiation, which is therefore not
// local; packing, exchange and unpacking run behind the request.
MPI_API(Ialltoallw, const void *sendbuf, const int sendcounts[], const int sdispls[], const MPI_Datatype sendtypes[],
        void *recvbuf, const int recvcounts[], const int rdispls[], const MPI_Datatype recvtypes[], MPI_Comm comm,
        MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Ialltoallw", [&] {
        return PMPI_Alltoallw(sendbuf, sendcounts, sdispls, sendtypes, recvbuf, recvcounts, rdispls, recvtypes, comm);
    });
}

// MPI_Igather(v) / MPI_Iscatter(v) / MPI_Iallgatherv: the blocking calls initiated with deferred
// completion.  Igatherv's and Iscatterv's ranks meet on the host inside the initiation (the row
// exchange), so starting them is not local.
MPI_API(Igather, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
        MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Igather", [&] {
        return PMPI_Gather(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, root, comm);
    });
}

MPI_API(Igatherv, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
        const int displs[], MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Igatherv", [&] {
        return PMPI_Gatherv(sendbuf, sendcount, sendtype, recvbuf, recvcounts, displs, recvtype, root, comm);
    });
}

MPI_API(Iallgatherv, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
        const int displs[], MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Iallgatherv", [&] {
        return PMPI_Allgatherv(sendbuf, sendcount, sendtype, recvbuf, recvcounts, displs, recvtype, comm);
    });
}

MPI_API(Iscatter, const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
        MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Iscatter", [&] {
        return PMPI_Scatter(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, root, comm);
    });
}

MPI_API(Iscatterv, const void *sendbuf, const int sendcounts[], const int displs[], MPI_Datatype sendtype, void *recvbuf,
        int recvcount, MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Iscatterv", [&] {
        return PMPI_Scatterv(sendbuf, sendcounts, displs, sendtype, recvbuf, recvcount, recvtype, root, comm);
    });
}

MPI_API(Ibcast, void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Ibcast", [&] { return PMPI_Bcast(buffer, count, dt, root, comm); });
}

MPI_API(Ibarrier, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    return start_coll(request, "MPI_Ibarrier", [&] { return PMPI_Barrier(comm); });
}

// ---------------------------------------------------------------- completion
MPI_API(Wait, MPI_Request *request, MPI_Status *status) {
    CsLock lk;
    if (!request) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Wait");
    if (*request == MPI_REQUEST_NULL) {
        status_set(status, MPI_ANY_SOURCE, MPI_ANY_TAG, 0, MPI_SUCCESS);
        return MPI_SUCCESS;
    }
    MReq *r = req_get(*request);
    if (!r) return err_return(MPI_COMM_WORLD, MPI_ERR_REQUEST, "MPI_Wait");
    const int rc = req_wait(*r, status);
    *request = MPI_REQUEST_NULL;
    return err_return(MPI_COMM_WORLD, rc, "MPI_Wait");
}

MPI_API(Test, MPI_Request *request, int *flag, MPI_Status *status) {
    CsLock lk;
    if (!request || !flag) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Test");
    if (*request == MPI_REQUEST_NULL) {
        *flag = 1;
        status_set(status, MPI_ANY_SOURCE, MPI_ANY_TAG, 0, MPI_SUCCESS);
        return MPI_SUCCESS;
    }
    MReq *r = req_get(*request);
    if (!r) return err_return(MPI_COMM_WORLD, MPI_ERR_REQUEST, "MPI_Test");
    const int rc = req_test(*r, flag, status);
    if (*flag) *request = MPI_REQUEST_NULL;
    return err_return(MPI_COMM_WORLD, rc, "MPI_Test");
}

MPI_API(Waitall, int count, MPI_Request requests[], MPI_Status statuses[]) {
    CsLock lk;
    if (count < 0 || (count && !requests)) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Waitall");
    // progress every request together (a receive may need a send of this rank to move)
    int rc_all = MPI_SUCCESS;
    for (;;) {
        bool pending = false;
        for (int i = 0; i < count; ++i) {
            if (requests[i] == MPI_REQUEST_NULL) continue;
            MReq *r = req_get(requests[i]);
            MPI_Status *st = (!statuses || statuses == MPI_STATUSES_IGNORE) ? MPI_STATUS_IGNORE : &statuses[i];
            if (!r) {
                status_set(st, MPI_ANY_SOURCE, MPI_ANY_TAG, 0, MPI_ERR_REQUEST);
                rc_all = MPI_ERR_IN_STATUS;
                requests[i] = MPI_REQUEST_NULL;
                continue;
            }
            int flag = 0;
            const int rc = req_test(*r, &flag, st);
            if (flag) {
                requests[i] = MPI_REQUEST_NULL;
                if (rc) rc_all = MPI_ERR_IN_STATUS;
            } else {
                pending = true;
            }
        }
        if (!pending) break;
        sched_yield();
    }
    return err_return(MPI_COMM_WORLD, rc_all, "MPI_Waitall");
}

MPI_API(Testall, int count, MPI_Request requests[], int *flag, MPI_Status statuses[]) {
    CsLock lk;
    if (count < 0 || !flag || (count && !requests)) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Testall");
    // MPI-3.1 §3.7.5: flag = true only if all requests have completed, and then all of them
    // are completed (deallocated, statuses set); otherwise no request is modified.  First a
    // peek (progress without completing), then completion of all of them.
    for (int i = 0; i < count; ++i) {
        if (requests[i] == MPI_REQUEST_NULL) continue;
        MReq *r = req_get(requests[i]);
        if (!r) continue;  // reported below
        int d = 1;
        if (r->kind == RQ_COLL) {
            const int rc = mv2h_test_ticket(r->id, &d);  // reads the completion word only
            if (rc) r->err = rc, d = 1;                  // a failed collective has completed
        } else if (r->kind == RQ_P2P && mv2h_p2p_peek(r->id, &d)) {
            d = 1;  // the request's own test reports the error
        }
        if (!d) {
            *flag = 0;
            return MPI_SUCCESS;
        }
    }
    int rc_all = MPI_SUCCESS;
    for (int i = 0; i < count; ++i) {
        if (requests[i] == MPI_REQUEST_NULL) continue;
        MReq *r = req_get(requests[i]);
        MPI_Status *st = (!statuses || statuses == MPI_STATUSES_IGNORE) ? MPI_STATUS_IGNORE : &statuses[i];
        if (!r) {
            status_set(st, MPI_ANY_SOURCE, MPI_ANY_TAG, 0, MPI_ERR_REQUEST);
            requests[i] = MPI_REQUEST_NULL;
            rc_all = MPI_ERR_IN_STATUS;
            continue;
        }
        const int rc = req_wait(*r, st);  // complete: returns at once
        requests[i] = MPI_REQUEST_NULL;
        if (rc) rc_all = MPI_ERR_IN_STATUS;
    }
    *flag = 1;
    return err_return(MPI_COMM_WORLD, rc_all, "MPI_Testall");
}

MPI_API(Request_free, MPI_Request *request) {
    CsLock lk;
    if (!request) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Request_free");
    MReq *r = req_get(*request);
    if (!r) return err_return(MPI_COMM_WORLD, MPI_ERR_REQUEST, "MPI_Request_free");
    // the operation still completes; this library waits for it here
    req_wait(*r, MPI_STATUS_IGNORE);
    *request = MPI_REQUEST_NULL;
    return MPI_SUCCESS;
}

// ---------------------------------------------------------------- point-to-point
MPI_API(Isend, const void *buf, int count, MPI_Datatype dt, int dest, int tag, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    int rc = p2p_checks(comm, count, dt, tag, false);
    if (!rc && !request) rc = MPI_ERR_ARG;
    if (!rc) rc = isend_impl(buf, count, dt, dest, tag, request);
    return err_return(comm, rc, "MPI_Isend");
}

MPI_API(Irecv, void *buf, int count, MPI_Datatype dt, int source, int tag, MPI_Comm comm, MPI_Request *request) {
    CsLock lk;
    int rc = p2p_checks(comm, count, dt, tag, true);
    if (!rc && !request) rc = MPI_ERR_ARG;
    if (!rc) rc = irecv_impl(buf, count, dt, source, tag, request);
    return err_return(comm, rc, "MPI_Irecv");
}

MPI_API(Send, const void *buf, int count, MPI_Datatype dt, int dest, int tag, MPI_Comm comm) {
    CsLock lk;
    MPI_Request rq = MPI_REQUEST_NULL;
    int rc = p2p_checks(comm, count, dt, tag, false);
    if (!rc) rc = isend_impl(buf, count, dt, dest, tag, &rq);
    if (!rc) rc = req_wait(*req_get(rq), MPI_STATUS_IGNORE);
    return err_return(comm, rc, "MPI_Send");
}

MPI_API(Recv, void *buf, int count, MPI_Datatype dt, int source, int tag, MPI_Comm comm, MPI_Status *status) {
    CsLock lk;
    MPI_Request rq = MPI_REQUEST_NULL;
    int rc = p2p_checks(comm, count, dt, tag, true);
    if (!rc) rc = irecv_impl(buf, count, dt, source, tag, &rq);
    if (!rc) rc = req_wait(*req_get(rq), status);
    return err_return(comm, rc, "MPI_Recv");
}

MPI_API(Sendrecv, const void *sendbuf, int sendcount, MPI_Datatype sendtype, int dest, int sendtag, void *recvbuf,
        int recvcount, MPI_Datatype recvtype, int source, int recvtag, MPI_Comm comm, MPI_Status *status) {
    CsLock lk;
    MPI_Request rr = MPI_REQUEST_NULL, sr = MPI_REQUEST_NULL;
    int rc = p2p_checks(comm, recvcount, recvtype, recvtag, true);
    if (!rc) rc = p2p_checks(comm, sendcount, sendtype, sendtag, false);
    if (!rc) rc = irecv_impl(recvbuf, recvcount, recvtype, source, recvtag, &rr);
    if (!rc) rc = isend_impl(sendbuf, sendcount, sendtype, dest, sendtag, &sr);
    if (rc) return err_return(comm, rc, "MPI_Sendrecv");
    MPI_Request both[2] = {rr, sr};
    MPI_Status sts[2];
    rc = PMPI_Waitall(2, both, sts);
    if (status && status != MPI_STATUS_IGNORE) *status = sts[0];
    if (rc == MPI_ERR_IN_STATUS) rc = sts[0].MPI_ERROR ? sts[0].MPI_ERROR : sts[1].MPI_ERROR;
    return err_return(comm, rc, "MPI_Sendrecv");
}

MPI_API(Get_count, const MPI_Status *status, MPI_Datatype dt, int *count) {
    if (!status || !count) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Get_count");
    const long tsz = dtype_size(dt);
    if (tsz < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_TYPE, "MPI_Get_count");
    const unsigned long long bytes = (unsigned long long)(unsigned)status->count_lo |
                                     ((unsigned long long)((unsigned)status->count_hi_and_cancelled >> 1) << 32);
    if (tsz == 0) *count = 0;
    else *count = bytes % (unsigned long long)tsz ? MPI_UNDEFINED : (int)(bytes / (unsigned long long)tsz);
    return MPI_SUCCESS;
}

}  // extern "C"

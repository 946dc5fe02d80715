// mpi_api.cpp — the MPI-3.1 C entry points (include/mpi.h) over the mv2h
// C-ABI.  Argument checking and error-handler behaviour follow the
// reference's MPI layer (e.g. allreduce.c:827-960, reduce_local.c:206-268):
// count == 0 returns immediately, a predefined op on a type outside its
// groups is MPI_ERR_OP, errors go through the communicator's error handler
// (default MPI_ERRORS_ARE_FATAL).  Every MPI_X is a weak alias of PMPI_X
// (allreduce.c:80-84).
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../../include/mpi.h"
#include "../../../include/mv2h.h"
#include "../../../include/mpir_op.h"
#include "../common.h"
#include "../runtime/log.h"
#include "../runtime/orders.h"
#include "../runtime/pvars.h"
#include "../runtime/world.h"
#include "datatype.h"
#include "user_coll.h"

using namespace mv2;

extern "C" int PMPI_Type_get_extent(MPI_Datatype dt, MPI_Aint *lb, MPI_Aint *extent);

namespace {

std::recursive_mutex g_cs;  // global critical section (allreduce.c:838)
MPI_Errhandler g_eh[2] = {MPI_ERRORS_ARE_FATAL, MPI_ERRHANDLER_NULL};  // SELF: unset, WORLD's applies
bool g_initialized = false, g_finalized = false;

struct UserOp {
    MPI_User_function *fn;
    int commute;
    bool live;
};
std::vector<UserOp> g_uops;
constexpr int kUserOpBase = (int)0x98000000;  // direct-kind op handles (MPICH kind bits 10, object 0x18)

const char *err_name(int c) {
    switch (c) {
    case MPI_SUCCESS: return "MPI_SUCCESS: no error";
    case MPI_ERR_BUFFER: return "MPI_ERR_BUFFER: invalid buffer pointer";
    case MPI_ERR_COUNT: return "MPI_ERR_COUNT: invalid count argument";
    case MPI_ERR_TYPE: return "MPI_ERR_TYPE: invalid datatype";
    case MPI_ERR_COMM: return "MPI_ERR_COMM: invalid communicator";
    case MPI_ERR_ROOT: return "MPI_ERR_ROOT: invalid root";
    case MPI_ERR_OP: return "MPI_ERR_OP: invalid reduce operation";
    case MPI_ERR_ARG: return "MPI_ERR_ARG: invalid argument";
    case MPI_ERR_TRUNCATE: return "MPI_ERR_TRUNCATE: message truncated";
    case MPI_ERR_OTHER: return "MPI_ERR_OTHER: other error";
    case MPI_ERR_INTERN: return "MPI_ERR_INTERN: internal error";
    case MPI_ERR_NO_MEM: return "MPI_ERR_NO_MEM: out of memory";
    case MPI_ERR_UNSUPPORTED_OPERATION: return "MPI_ERR_UNSUPPORTED_OPERATION: unsupported operation";
    default: return "unknown error";
    }
}

int comm_index(MPI_Comm c) {
    if (c == MPI_COMM_WORLD) return 0;
    if (c == MPI_COMM_SELF) return 1;
    return -1;
}

// MPIR_Err_return_comm (allreduce.c:956, errutil.c:249-289): fatal handler aborts, return
// handler passes the code; an invalid communicator, or one whose handler was never set
// (MPI_COMM_SELF's until MPI_Comm_set_errhandler), takes MPI_COMM_WORLD's handler
int err_return(MPI_Comm comm, int code, const char *fn) {
    if (code == MPI_SUCCESS) return code;
    const int ci = comm_index(comm);
    const MPI_Errhandler eh = ci >= 0 && g_eh[ci] != MPI_ERRHANDLER_NULL ? g_eh[ci] : g_eh[0];
    if (eh == MPI_ERRORS_ARE_FATAL) {
        fprintf(stderr, "[mv2amd rank %d] Fatal error in %s: %s\n", mv2h_rank(), fn, err_name(code));
        fflush(stderr);
        abort();
    }
    static const int verbose = [] {
        const char *v = getenv("MV2AMD_ERR_VERBOSE");  // tests: name every error a call returns
        return v && *v && *v != '0';
    }();
    if (verbose) {
        fprintf(stderr, "[mv2amd rank %d] %s returned %s\n", mv2h_rank(), fn, err_name(code));
        fflush(stderr);
    }
    return code;
}

UserOp *user_op(MPI_Op op) {
    const unsigned idx = (unsigned)(op - kUserOpBase);
    if ((op & 0xff000000) != (kUserOpBase & 0xff000000) || idx >= g_uops.size() || !g_uops[idx].live) return nullptr;
    return &g_uops[idx];
}

bool op_valid(MPI_Op op) { return is_builtin_op(op) || user_op(op) != nullptr; }

bool is_dev(const void *p) { return p && p != MPI_IN_PLACE && mv2h_is_device_ptr(p); }

// ---- user-op path: user functions are host callbacks (the reference also
// calls them on host copies of device buffers, reduce_local.c:54-164); the
// collectives' host evaluation is user_coll.cpp ----
int copy_to_host(HostBuf &h, const void *p, size_t bytes) {
    h.resize(bytes ? bytes : 1);
    if (!h.data()) return MPI_ERR_NO_MEM;
    if (is_dev(p)) return mv2h_memcpy_dtoh(h.data(), p, bytes);
    memcpy(h.data(), p, bytes);
    return 0;
}
int copy_from_host(void *p, const HostBuf &h, size_t bytes) {
    if (is_dev(p)) return mv2h_memcpy_htod(p, h.data(), bytes);
    memcpy(p, h.data(), bytes);
    return 0;
}

// ---- x87 80-bit long double (MPI_LONG_DOUBLE, MPI_C_LONG_DOUBLE_COMPLEX,
// MPI_LONG_DOUBLE_INT): gfx950 has no 80-bit float, so these builtin ops run
// on the host, as the reference's own loops do (oputil.h:316-349,
// opmaxloc.c:65-87), through the same algorithm plans as user ops.  Only
// these three types take this path; every other builtin type is reduced on
// the GPU and has no host path.
int g_ld_op = -1;  // op index of the current x87 call (set under the global critical section)

template <class T>
inline T x_max(T a, T b) { return (a != a && b != b) ? a : (a != a) ? b : (b != b) ? a : ((b > a) ? b : a); }
template <class T>
inline T x_min(T a, T b) { return (a != a && b != b) ? a : (a != a) ? b : (b != b) ? a : ((a > b) ? b : a); }

struct LdInt {
    long double value;
    int loc;
};

void ld_uop(void *in, void *inout, int *len, MPI_Datatype *dt) {
    const long n = *len;
    const int op = g_ld_op;
    if (*dt == MPI_LONG_DOUBLE) {
        const long double *b = (const long double *)in;
        long double *a = (long double *)inout;
        for (long i = 0; i < n; ++i) {
            switch (op) {
            case OP_SUM: a[i] = a[i] + b[i]; break;
            case OP_PROD: a[i] = a[i] * b[i]; break;
            case OP_MAX: a[i] = x_max(a[i], b[i]); break;
            case OP_MIN: a[i] = x_min(a[i], b[i]); break;
            case OP_LAND: a[i] = (a[i] && b[i]); break;
            case OP_LOR: a[i] = (a[i] || b[i]); break;
            case OP_LXOR: a[i] = ((a[i] && !b[i]) || (!a[i] && b[i])); break;
            case OP_REPLACE: a[i] = b[i]; break;
            default: break;
            }
        }
    } else if (*dt == MPI_C_LONG_DOUBLE_COMPLEX) {
        const __complex__ long double *b = (const __complex__ long double *)in;
        __complex__ long double *a = (__complex__ long double *)inout;
        for (long i = 0; i < n; ++i) {
            if (op == OP_SUM) a[i] = a[i] + b[i];
            else if (op == OP_PROD) a[i] = a[i] * b[i];  // Annex G __mulxc3, like the reference's C99 loop
            else if (op == OP_REPLACE) a[i] = b[i];
        }
    } else if (*dt == MPI_LONG_DOUBLE_INT) {
        const LdInt *b = (const LdInt *)in;
        LdInt *a = (LdInt *)inout;
        for (long i = 0; i < n; ++i) {
            if (op == OP_REPLACE) {
                memcpy(&a[i].value, &b[i].value, 10);
                a[i].loc = b[i].loc;
                continue;
            }
            if (op != OP_MAXLOC && op != OP_MINLOC) continue;
            const long double av = a[i].value, bv = b[i].value;
            if (av != av && bv != bv) {
                a[i].loc = std::min(a[i].loc, b[i].loc);
            } else if (av != av) {
                a[i].value = bv;
                a[i].loc = b[i].loc;
            } else if (bv != bv) {
            } else if (op == OP_MAXLOC ? av < bv : av > bv) {
                a[i].value = bv;
                a[i].loc = b[i].loc;
            } else if (op == OP_MAXLOC ? av <= bv : av >= bv) {
                a[i].loc = std::min(a[i].loc, b[i].loc);
            }
        }
    }
}

bool is_x87(MPI_Datatype dt) {
    return dt == MPI_LONG_DOUBLE || dt == MPI_C_LONG_DOUBLE_COMPLEX || dt == MPI_LONG_DOUBLE_INT;
}

int user_reduce_local(const void *in, void *inout, int count, MPI_Datatype dt, UserOp *u) {
    long span = dtype_span(dt, count);
    if (span < 0) return MPI_ERR_TYPE;
    HostBuf hin(HS_IN), hio(HS_INOUT);
    int rc = copy_to_host(hin, in, span);
    if (!rc) rc = copy_to_host(hio, inout, span);
    if (rc) return MPI_ERR_OTHER;
    int c = count;
    MPI_Datatype d = dt;
    u->fn(hin.data(), hio.data(), &c, &d);
    return copy_from_host(inout, hio, span) ? MPI_ERR_OTHER : MPI_SUCCESS;
}

// one MPI_T-counted call (runtime/pvars.h)
int user_allreduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, UserOp *u, int opk) {
    pvar_begin();
    const int rc = host_allreduce(sendbuf, recvbuf, count, dt, HostOp{u->fn, opk});
    pvar_end(rc == MPI_SUCCESS);
    return rc;
}

// one MPI_T-counted call (runtime/pvars.h)
int user_reduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, UserOp *u, int root, int opk) {
    pvar_begin();
    const int rc = host_reduce(sendbuf, recvbuf, count, dt, HostOp{u->fn, opk}, root);
    pvar_end(rc == MPI_SUCCESS);
    return rc;
}

}  // namespace

extern "C" int PMPI_Type_get_extent(MPI_Datatype dt, MPI_Aint *lb, MPI_Aint *extent);

namespace {

// one MPI_T-counted call (runtime/pvars.h)
int user_reduce_scatter(const void *sendbuf, void *recvbuf, const int *counts, MPI_Datatype dt, UserOp *u, int opk) {
    pvar_begin();
    const int rc = host_reduce_scatter(sendbuf, recvbuf, counts, dt, HostOp{u->fn, opk});
    pvar_end(rc == MPI_SUCCESS);
    return rc;
}

}  // namespace

#define WEAK(name) __attribute__((weak, alias("P" #name)))

extern "C" {

// ---------------------------------------------------------------- environment
int PMPI_Init(int *, char ***) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    if (g_initialized) return err_return(MPI_COMM_WORLD, MPI_ERR_OTHER, "MPI_Init");
    int rc = world_init();
    if (rc) return err_return(MPI_COMM_WORLD, rc, "MPI_Init");
    g_initialized = true;
    return MPI_SUCCESS;
}
int MPI_Init(int *argc, char ***argv) WEAK(MPI_Init);

int PMPI_Init_thread(int *argc, char ***argv, int required, int *provided) {
    int rc = PMPI_Init(argc, argv);
    if (provided) *provided = required > MPI_THREAD_SERIALIZED ? MPI_THREAD_SERIALIZED : required;
    return rc;
}
int MPI_Init_thread(int *argc, char ***argv, int required, int *provided) WEAK(MPI_Init_thread);

int PMPI_Finalize(void) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    world_finalize();
    g_finalized = true;
    return MPI_SUCCESS;
}
int MPI_Finalize(void) WEAK(MPI_Finalize);

int PMPI_Initialized(int *flag) {
    *flag = g_initialized ? 1 : 0;
    return MPI_SUCCESS;
}
int MPI_Initialized(int *flag) WEAK(MPI_Initialized);

int PMPI_Finalized(int *flag) {
    *flag = g_finalized ? 1 : 0;
    return MPI_SUCCESS;
}
int MPI_Finalized(int *flag) WEAK(MPI_Finalized);

int PMPI_Abort(MPI_Comm, int errorcode) {
    fprintf(stderr, "[mv2amd rank %d] MPI_Abort(%d)\n", mv2h_rank(), errorcode);
    fflush(stderr);
    _exit(errorcode ? errorcode : 1);
}
int MPI_Abort(MPI_Comm comm, int errorcode) WEAK(MPI_Abort);

double PMPI_Wtime(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * ts.tv_nsec;
}
double MPI_Wtime(void) WEAK(MPI_Wtime);

double PMPI_Wtick(void) { return 1e-9; }
double MPI_Wtick(void) WEAK(MPI_Wtick);

int PMPI_Get_processor_name(char *name, int *len) {
    gethostname(name, MPI_MAX_PROCESSOR_NAME);
    name[MPI_MAX_PROCESSOR_NAME - 1] = 0;
    *len = (int)strlen(name);
    return MPI_SUCCESS;
}
int MPI_Get_processor_name(char *name, int *len) WEAK(MPI_Get_processor_name);

int PMPI_Error_string(int code, char *s, int *len) {
    snprintf(s, MPI_MAX_ERROR_STRING, "%s", err_name(code));
    *len = (int)strlen(s);
    return MPI_SUCCESS;
}
int MPI_Error_string(int code, char *s, int *len) WEAK(MPI_Error_string);

int PMPI_Error_class(int code, int *cls) {
    *cls = code & 0x7f;
    return MPI_SUCCESS;
}
int MPI_Error_class(int code, int *cls) WEAK(MPI_Error_class);

int PMPI_Comm_set_errhandler(MPI_Comm comm, MPI_Errhandler eh) {
    const int ci = comm_index(comm);
    if (ci < 0) return MPI_ERR_COMM;
    if (eh != MPI_ERRORS_ARE_FATAL && eh != MPI_ERRORS_RETURN) return MPI_ERR_ARG;
    g_eh[ci] = eh;
    return MPI_SUCCESS;
}
int MPI_Comm_set_errhandler(MPI_Comm comm, MPI_Errhandler eh) WEAK(MPI_Comm_set_errhandler);

int PMPI_Errhandler_set(MPI_Comm comm, MPI_Errhandler eh) { return PMPI_Comm_set_errhandler(comm, eh); }
int MPI_Errhandler_set(MPI_Comm comm, MPI_Errhandler eh) WEAK(MPI_Errhandler_set);

int PMPI_Comm_get_errhandler(MPI_Comm comm, MPI_Errhandler *eh) {
    const int ci = comm_index(comm);
    if (ci < 0) return MPI_ERR_COMM;
    *eh = g_eh[ci] == MPI_ERRHANDLER_NULL ? MPI_ERRORS_ARE_FATAL : g_eh[ci];  // comm_get_errhandler.c: unset reads FATAL
    return MPI_SUCCESS;
}
int MPI_Comm_get_errhandler(MPI_Comm comm, MPI_Errhandler *eh) WEAK(MPI_Comm_get_errhandler);

// ---------------------------------------------------------------- communicators
int PMPI_Comm_rank(MPI_Comm comm, int *rank) {
    const int ci = comm_index(comm);
    if (ci < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, "MPI_Comm_rank");
    *rank = ci == 0 ? mv2h_rank() : 0;
    return MPI_SUCCESS;
}
int MPI_Comm_rank(MPI_Comm comm, int *rank) WEAK(MPI_Comm_rank);

int PMPI_Comm_size(MPI_Comm comm, int *size) {
    const int ci = comm_index(comm);
    if (ci < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, "MPI_Comm_size");
    *size = ci == 0 ? mv2h_size() : 1;
    return MPI_SUCCESS;
}
int MPI_Comm_size(MPI_Comm comm, int *size) WEAK(MPI_Comm_size);

int PMPI_Barrier(MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const int ci = comm_index(comm);
    if (ci < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, "MPI_Barrier");
    if (ci == 0 && mv2h_barrier()) return err_return(comm, MPI_ERR_OTHER, "MPI_Barrier");
    return MPI_SUCCESS;
}
int MPI_Barrier(MPI_Comm comm) WEAK(MPI_Barrier);

// ---------------------------------------------------------------- user ops
int PMPI_Op_create(MPI_User_function *fn, int commute, MPI_Op *op) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    if (!fn || !op) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Op_create");
    g_uops.push_back(UserOp{fn, commute ? 1 : 0, true});
    *op = kUserOpBase + (int)(g_uops.size() - 1);
    return MPI_SUCCESS;
}
int MPI_Op_create(MPI_User_function *fn, int commute, MPI_Op *op) WEAK(MPI_Op_create);

int PMPI_Op_free(MPI_Op *op) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    UserOp *u = op ? user_op(*op) : nullptr;
    if (!u) return err_return(MPI_COMM_WORLD, MPI_ERR_OP, "MPI_Op_free");
    u->live = false;
    *op = MPI_OP_NULL;
    return MPI_SUCCESS;
}
int MPI_Op_free(MPI_Op *op) WEAK(MPI_Op_free);

int PMPI_Op_commutative(MPI_Op op, int *commute) {
    if (is_builtin_op(op)) {
        *commute = 1;
        return MPI_SUCCESS;
    }
    UserOp *u = user_op(op);
    if (!u) return err_return(MPI_COMM_WORLD, MPI_ERR_OP, "MPI_Op_commutative");
    *commute = u->commute;
    return MPI_SUCCESS;
}
int MPI_Op_commutative(MPI_Op op, int *commute) WEAK(MPI_Op_commutative);

// ---------------------------------------------------------------- reductions
// A builtin op on `count` elements of a builtin type (device or host buffers;
// x87 types on the host): the MPI error class, no error handler.
static int builtin_reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype dt, MPI_Op op) {
    if (!dtype_is_builtin(dt)) return MPI_ERR_OP;
    if (is_x87(dt)) {
        if (mv2h_op_check(op, dt)) return MPI_ERR_OP;
        UserOp x{ld_uop, 1, true};
        g_ld_op = op_index(op);
        return op_index(op) == OP_NO_OP ? 0 : user_reduce_local(inbuf, inoutbuf, count, dt, &x);
    }
    return mv2h_reduce_local(inbuf, inoutbuf, (size_t)count, dt, op, nullptr);
}

int PMPI_Reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype dt, MPI_Op op) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Reduce_local";
    if (count < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COUNT, fn);
    if (!op_valid(op)) return err_return(MPI_COMM_WORLD, MPI_ERR_OP, fn);
    if (!dtype_valid(dt)) return err_return(MPI_COMM_WORLD, MPI_ERR_TYPE, fn);
    if (!dtype_committed(dt)) return err_return(MPI_COMM_WORLD, MPI_ERR_TYPE, fn);
    if (count == 0) return MPI_SUCCESS;
    // reduce_local.c:233-237: aliased operands (MPIR_ERRTEST_ALIAS_COLL), then MPI_IN_PLACE
    if (inbuf == inoutbuf || inbuf == MPI_IN_PLACE || inoutbuf == MPI_IN_PLACE)
        return err_return(MPI_COMM_WORLD, MPI_ERR_BUFFER, fn);
    if (UserOp *u = user_op(op)) return err_return(MPI_COMM_WORLD, user_reduce_local(inbuf, inoutbuf, count, dt, u), fn);
    return err_return(MPI_COMM_WORLD, builtin_reduce_local(inbuf, inoutbuf, count, dt, op), fn);
}
int MPI_Reduce_local(const void *inbuf, void *inoutbuf, int count, MPI_Datatype dt, MPI_Op op) WEAK(MPI_Reduce_local);

// ---------------------------------------------------------------------------
// The predefined ops as MPI_User_function entry points (include/mpir_op.h):
// MPIR_Op_table (allreduce.c:95-100) indexed by MPIR_OP_HDL_TO_FN
// (mpiimpl.h:4031), and the per-op type checks (MPIR_Op_check_dtype_table).
// Unlike the reference's host loops (opsum.c:26-90 ...) they take device
// buffers: one HBM-streaming kernel, synchronous like any MPI_User_function;
// host buffers are staged as for MPI_Reduce_local.  A type the op does not
// accept leaves inoutvec untouched and sets the error MPIR_Op_errno returns
// (the reference keeps it in the thread-private op_errno, opsum.c:82-86).
// ---------------------------------------------------------------------------
static thread_local int t_op_errno = MPI_SUCCESS;

static void op_entry(MPI_Op op, void *invec, void *inoutvec, int *len, MPI_Datatype *type) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    if (!len || !type || *len < 0) {
        t_op_errno = MPI_ERR_ARG;
        return;
    }
    if (*len == 0) return;
    if (!dtype_valid(*type)) {
        t_op_errno = MPI_ERR_TYPE;
        return;
    }
    if (mv2h_op_check(op, *type)) {
        t_op_errno = MPI_ERR_OP;
        return;
    }
    const int rc = builtin_reduce_local(invec, inoutvec, *len, *type, op);
    if (rc) t_op_errno = rc;
}

#define MV2_OP_FN(NAME, HANDLE)                                                               \
    void NAME(void *invec, void *inoutvec, int *len, MPI_Datatype *type) {                     \
        op_entry(HANDLE, invec, inoutvec, len, type);                                          \
    }                                                                                          \
    int NAME##_check_dtype(MPI_Datatype type) {                                                \
        return !dtype_valid(type) ? MPI_ERR_TYPE : (mv2h_op_check(HANDLE, type) ? MPI_ERR_OP : MPI_SUCCESS); \
    }
MV2_OP_FN(MPIR_MAXF, MPI_MAX)
MV2_OP_FN(MPIR_MINF, MPI_MIN)
MV2_OP_FN(MPIR_SUM, MPI_SUM)
MV2_OP_FN(MPIR_PROD, MPI_PROD)
MV2_OP_FN(MPIR_LAND, MPI_LAND)
MV2_OP_FN(MPIR_BAND, MPI_BAND)
MV2_OP_FN(MPIR_LOR, MPI_LOR)
MV2_OP_FN(MPIR_BOR, MPI_BOR)
MV2_OP_FN(MPIR_LXOR, MPI_LXOR)
MV2_OP_FN(MPIR_BXOR, MPI_BXOR)
MV2_OP_FN(MPIR_MINLOC, MPI_MINLOC)
MV2_OP_FN(MPIR_MAXLOC, MPI_MAXLOC)
MV2_OP_FN(MPIR_REPLACE, MPI_REPLACE)
MV2_OP_FN(MPIR_NO_OP, MPI_NO_OP)
#undef MV2_OP_FN

// order of the predefined op handles' low nibble (mpi.h: MPI_MAX = ...01 .. MPI_NO_OP = ...0e)
MPI_User_function *MPIR_Op_table[] = {MPIR_MAXF, MPIR_MINF, MPIR_SUM,  MPIR_PROD,   MPIR_LAND,   MPIR_BAND,    MPIR_LOR,
                                      MPIR_BOR,  MPIR_LXOR, MPIR_BXOR, MPIR_MINLOC, MPIR_MAXLOC, MPIR_REPLACE, MPIR_NO_OP};
MPIR_Op_check_dtype_fn *MPIR_Op_check_dtype_table[] = {
    MPIR_MAXF_check_dtype, MPIR_MINF_check_dtype,   MPIR_SUM_check_dtype,    MPIR_PROD_check_dtype,
    MPIR_LAND_check_dtype, MPIR_BAND_check_dtype,   MPIR_LOR_check_dtype,    MPIR_BOR_check_dtype,
    MPIR_LXOR_check_dtype, MPIR_BXOR_check_dtype,   MPIR_MINLOC_check_dtype, MPIR_MAXLOC_check_dtype,
    MPIR_REPLACE_check_dtype, MPIR_NO_OP_check_dtype};

int MPIR_Op_errno(void) {
    const int e = t_op_errno;
    t_op_errno = MPI_SUCCESS;
    return e;
}

// The buffer checks of the reference's MPI layer, MPI_ERR_BUFFER each (mpierrs.h):
// MPIR_ERRTEST_USERBUFFER (:313-331) — no buffer for count > 0 elements of a builtin type, or of
// a derived type whose true lb is 0 and size > 0 (a null buffer is MPI_BOTTOM otherwise);
// MPIR_ERRTEST_{SEND,RECV,}BUF_INPLACE (:274-301) — MPI_IN_PLACE where the call has no in-place
// form; MPIR_ERRTEST_ALIAS_COLL (:132-140, MPIR_CVAR_COLL_ALIAS_CHECK's default 1) — the send
// buffer is the receive buffer.
static bool null_userbuf(const void *buf, long count, MPI_Datatype dt) {
    if (count <= 0 || buf) return false;
    return dtype_is_builtin(dt) || (dtype_valid(dt) && dtype_true_lb(dt) == 0 && dtype_size(dt) > 0);
}
static bool inplace_buf(const void *buf, long count) { return count > 0 && buf == MPI_IN_PLACE; }

// allreduce.c:880-888
static int allreduce_buf_checks(const void *sendbuf, const void *recvbuf, int count, MPI_Datatype dt) {
    if (count != 0 && sendbuf != MPI_IN_PLACE && sendbuf == recvbuf) return MPI_ERR_BUFFER;
    if (sendbuf != MPI_IN_PLACE && null_userbuf(sendbuf, count, dt)) return MPI_ERR_BUFFER;
    if (inplace_buf(recvbuf, count) || null_userbuf(recvbuf, count, dt)) return MPI_ERR_BUFFER;
    return MPI_SUCCESS;
}

// reduce.c:1190-1202: the receive buffer matters at the root only; elsewhere MPI_IN_PLACE is
// not a send buffer
static int reduce_buf_checks(const void *sendbuf, const void *recvbuf, int count, MPI_Datatype dt, bool at_root) {
    if (sendbuf != MPI_IN_PLACE && null_userbuf(sendbuf, count, dt)) return MPI_ERR_BUFFER;
    if (!at_root) return inplace_buf(sendbuf, count) ? MPI_ERR_BUFFER : MPI_SUCCESS;
    if (inplace_buf(recvbuf, count) || null_userbuf(recvbuf, count, dt)) return MPI_ERR_BUFFER;
    if (count != 0 && sendbuf != MPI_IN_PLACE && sendbuf == recvbuf) return MPI_ERR_BUFFER;
    return MPI_SUCCESS;
}

// red_scat.c:1182-1189 (and red_scat_block.c:1147-1154, the same with every count equal)
static int reduce_scatter_buf_checks(const void *sendbuf, const void *recvbuf, long mine, long sum, MPI_Datatype dt) {
    if (inplace_buf(recvbuf, mine)) return MPI_ERR_BUFFER;
    if (sendbuf != MPI_IN_PLACE && sum != 0 && sendbuf == recvbuf) return MPI_ERR_BUFFER;
    if (null_userbuf(recvbuf, mine, dt) || null_userbuf(sendbuf, sum, dt)) return MPI_ERR_BUFFER;
    return MPI_SUCCESS;
}

// allgather.c:952-958, before any other argument check: the send buffer is this rank's block
// of the receive buffer, the block measured in recvtype's size (as the reference measures it)
static bool allgather_alias(const void *sendbuf, int sendcount, MPI_Datatype sendtype, const void *recvbuf,
                            int recvcount, MPI_Datatype recvtype, int rank) {
    return sendbuf != MPI_IN_PLACE && sendtype == recvtype && recvcount != 0 && sendcount != 0 &&
           dtype_valid(recvtype) && sendbuf == (const char *)recvbuf + (long)rank * recvcount * dtype_size(recvtype);
}

// allgather.c:961-987, after the counts and types
static int allgather_buf_checks(const void *sendbuf, int sendcount, MPI_Datatype sendtype, const void *recvbuf,
                                int recvcount, MPI_Datatype recvtype) {
    if (sendbuf != MPI_IN_PLACE && null_userbuf(sendbuf, sendcount, sendtype)) return MPI_ERR_BUFFER;
    if (inplace_buf(recvbuf, recvcount) || null_userbuf(recvbuf, recvcount, recvtype)) return MPI_ERR_BUFFER;
    return MPI_SUCCESS;
}

// The checks every reduction shares, in allreduce.c:863-899's order: communicator, count,
// datatype, op handle, a derived type committed, then the call's buffer checks (buf_rc,
// computed by the caller), then the op against the type (MPIR_OP_HDL_TO_DTYPE_FN)
static int coll_checks(MPI_Comm comm, int count, MPI_Datatype dt, MPI_Op op, int buf_rc = MPI_SUCCESS) {
    if (!g_initialized || g_finalized) return MPI_ERR_OTHER;
    if (comm_index(comm) < 0) return MPI_ERR_COMM;
    if (count < 0) return MPI_ERR_COUNT;
    if (!dtype_valid(dt)) return MPI_ERR_TYPE;
    if (!op_valid(op)) return MPI_ERR_OP;
    if (!dtype_committed(dt)) return MPI_ERR_TYPE;
    if (buf_rc) return buf_rc;
    if (is_builtin_op(op) && !dtype_is_builtin(dt)) return MPI_ERR_OP;  // e.g. opsum.c:119-121
    if (is_builtin_op(op) && mv2h_op_check(op, dt)) return MPI_ERR_OP;
    return MPI_SUCCESS;
}

static int comm_rank_of(MPI_Comm comm) { return comm == MPI_COMM_SELF ? 0 : mv2h_rank(); }

int PMPI_Allreduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Allreduce";
    int rc = coll_checks(comm, count, dt, op, allreduce_buf_checks(sendbuf, recvbuf, count, dt));
    if (rc) return err_return(comm, rc, fn);
    if (count == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) {
        if (sendbuf != MPI_IN_PLACE && sendbuf != recvbuf) {
            const long span = dtype_span(dt, count);
            rc = is_dev(recvbuf) || is_dev(sendbuf) ? mv2h_memcpy_dtod(recvbuf, sendbuf, span) : (memcpy(recvbuf, sendbuf, span), 0);
        }
        return err_return(comm, rc, fn);
    }
    if (UserOp *u = user_op(op))
        return err_return(comm, user_allreduce(sendbuf, recvbuf, count, dt, u, u->commute ? OPK_USER_COMM : OPK_USER_NONCOMM), fn);
    if (is_x87(dt) && op_index(op) < OP_REPLACE) {
        UserOp x{ld_uop, 1, true};
        g_ld_op = op_index(op);
        return err_return(comm, user_allreduce(sendbuf, recvbuf, count, dt, &x, OPK_BUILTIN), fn);
    }
    rc = mv2h_allreduce(sendbuf, recvbuf, (size_t)count, dt, op, nullptr);
    return err_return(comm, rc, fn);
}
int MPI_Allreduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm) WEAK(MPI_Allreduce);

// MPI_Scan / MPI_Exscan.  Checks in the reference's order (scan.c:526-555, exscan.c:343-378):
// communicator, count, datatype, op handle, a derived type committed, the send buffer (MPI_IN_PLACE
// is allowed), the receive buffer -- for MPI_Exscan only where rank != 0 --, the op against the
// type, and last the send buffer aliasing the receive buffer.
static int scan_call(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
                     bool excl, const char *fn) {
    const bool recv_matters = !excl || comm_index(comm) < 0 || comm_rank_of(comm) != 0;
    int brc = null_userbuf(sendbuf, count, dt) ? MPI_ERR_BUFFER : MPI_SUCCESS;
    if (!brc && recv_matters && (inplace_buf(recvbuf, count) || null_userbuf(recvbuf, count, dt))) brc = MPI_ERR_BUFFER;
    int rc = coll_checks(comm, count, dt, op, brc);
    if (!rc && sendbuf != MPI_IN_PLACE && count != 0 && sendbuf == recvbuf) rc = MPI_ERR_BUFFER;
    if (rc) return err_return(comm, rc, fn);
    if (count == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) {  // one rank: Scan copies, Exscan leaves recvbuf alone
        if (!excl && sendbuf != MPI_IN_PLACE) {
            const long span = dtype_span(dt, count);
            rc = is_dev(recvbuf) || is_dev(sendbuf) ? mv2h_memcpy_dtod(recvbuf, sendbuf, span) : (memcpy(recvbuf, sendbuf, span), 0);
        }
        return err_return(comm, rc, fn);
    }
    // several nodes: the SMP-aware shape (scan.c:267-406) is not built; refused from the job's
    // shape alone, on every rank, before any device or network work
    if (world().nnodes > 1) {
        MV2_ERR("%s: only jobs on one node are supported (this job spans %d nodes)", fn, world().nnodes);
        return err_return(comm, MPI_ERR_OTHER, fn);
    }
    if (UserOp *u = user_op(op))
        return err_return(comm, host_scan(sendbuf, recvbuf, count, dt, HostOp{u->fn, u->commute ? OPK_USER_COMM : OPK_USER_NONCOMM}, excl), fn);
    if (is_x87(dt) && op_index(op) < OP_REPLACE) {
        g_ld_op = op_index(op);
        return err_return(comm, host_scan(sendbuf, recvbuf, count, dt, HostOp{ld_uop, OPK_BUILTIN}, excl), fn);
    }
    rc = excl ? mv2h_exscan(sendbuf, recvbuf, (size_t)count, dt, op, nullptr)
              : mv2h_scan(sendbuf, recvbuf, (size_t)count, dt, op, nullptr);
    return err_return(comm, rc, fn);
}

int PMPI_Scan(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return scan_call(sendbuf, recvbuf, count, dt, op, comm, false, "MPI_Scan");
}
int MPI_Scan(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm) WEAK(MPI_Scan);

int PMPI_Exscan(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return scan_call(sendbuf, recvbuf, count, dt, op, comm, true, "MPI_Exscan");
}
int MPI_Exscan(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm) WEAK(MPI_Exscan);

int PMPI_Reduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, int root, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Reduce";
    if (!g_initialized || g_finalized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(comm, MPI_ERR_COMM, fn);
    int size = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    if (root < 0 || root >= size) return err_return(comm, MPI_ERR_ROOT, fn);  // reduce.c:1178, before the count
    int rc = coll_checks(comm, count, dt, op, reduce_buf_checks(sendbuf, recvbuf, count, dt, comm_rank_of(comm) == root));
    if (rc) return err_return(comm, rc, fn);
    if (count == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) {
        if (sendbuf != MPI_IN_PLACE && sendbuf != recvbuf) {
            const long span = dtype_span(dt, count);
            rc = is_dev(recvbuf) || is_dev(sendbuf) ? mv2h_memcpy_dtod(recvbuf, sendbuf, span) : (memcpy(recvbuf, sendbuf, span), 0);
        }
        return err_return(comm, rc, fn);
    }
    if (UserOp *u = user_op(op))
        return err_return(comm, user_reduce(sendbuf, recvbuf, count, dt, u, root, u->commute ? OPK_USER_COMM : OPK_USER_NONCOMM), fn);
    if (is_x87(dt) && op_index(op) < OP_REPLACE) {
        UserOp x{ld_uop, 1, true};
        g_ld_op = op_index(op);
        return err_return(comm, user_reduce(sendbuf, recvbuf, count, dt, &x, root, OPK_BUILTIN), fn);
    }
    rc = mv2h_reduce(sendbuf, recvbuf, (size_t)count, dt, op, root, nullptr);
    return err_return(comm, rc, fn);
}
int MPI_Reduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, int root, MPI_Comm comm) WEAK(MPI_Reduce);

int PMPI_Reduce_scatter(const void *sendbuf, void *recvbuf, const int recvcounts[], MPI_Datatype dt, MPI_Op op,
                        MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Reduce_scatter";
    if (!g_initialized || g_finalized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(comm, MPI_ERR_COMM, fn);
    const int n = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    std::vector<size_t> rc_sz(n);
    size_t total = 0;
    for (int j = 0; j < n; ++j) {  // red_scat.c:1168-1171: the counts first
        if (recvcounts[j] < 0) return err_return(comm, MPI_ERR_COUNT, fn);
        rc_sz[j] = (size_t)recvcounts[j];
        total += rc_sz[j];
    }
    int rc = coll_checks(comm, 0, dt, op,
                         reduce_scatter_buf_checks(sendbuf, recvbuf, recvcounts[comm_rank_of(comm)], (long)total, dt));
    if (rc) return err_return(comm, rc, fn);
    if (total == 0) return MPI_SUCCESS;
    if (UserOp *u = user_op(op))
        if (comm != MPI_COMM_SELF)
            return err_return(comm, user_reduce_scatter(sendbuf, recvbuf, recvcounts, dt, u,
                                                        u->commute ? OPK_USER_COMM : OPK_USER_NONCOMM), fn);
    if (is_x87(dt) && comm != MPI_COMM_SELF && op_index(op) < OP_REPLACE) {
        UserOp x{ld_uop, 1, true};
        g_ld_op = op_index(op);
        return err_return(comm, user_reduce_scatter(sendbuf, recvbuf, recvcounts, dt, &x, OPK_BUILTIN), fn);
    }
    if (comm == MPI_COMM_SELF) {
        if (sendbuf != MPI_IN_PLACE)
            rc = mv2h_memcpy_dtod(recvbuf, sendbuf, dtype_span(dt, recvcounts[0]));
        return err_return(comm, rc, fn);
    }
    rc = mv2h_reduce_scatter(sendbuf, recvbuf, rc_sz.data(), dt, op, nullptr);
    return err_return(comm, rc, fn);
}
int MPI_Reduce_scatter(const void *sendbuf, void *recvbuf, const int recvcounts[], MPI_Datatype dt, MPI_Op op,
                       MPI_Comm comm) WEAK(MPI_Reduce_scatter);

int PMPI_Reduce_scatter_block(const void *sendbuf, void *recvbuf, int recvcount, MPI_Datatype dt, MPI_Op op,
                              MPI_Comm comm) {
    // MVAPICH2's MPIR_Reduce_scatter_block_MV2 never sizes the message (nbytes stays 0,
    // red_scat_block_osu.c:320-372), so the default table's first entry runs: MPICH's
    // MPIR_Reduce_scatter_block (red_scat_block.c:305, :515: recursive halving below
    // MPIR_CVAR_REDSCAT_COMMUTATIVE_LONG_MSG_SIZE, pairwise from it) — the same
    // selection as MPI_Ireduce_scatter_block's schedule
    const int n = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    std::vector<int> counts(n, recvcount);
    const bool set = nbc_kind() == NBC_NONE;
    if (set) nbc_set(NBC_IREDUCE_SCATTER_BLOCK);
    const int rc = PMPI_Reduce_scatter(sendbuf, recvbuf, counts.data(), dt, op, comm);
    if (set) nbc_set(NBC_NONE);
    return rc;
}
int MPI_Reduce_scatter_block(const void *sendbuf, void *recvbuf, int recvcount, MPI_Datatype dt, MPI_Op op,
                             MPI_Comm comm) WEAK(MPI_Reduce_scatter_block);

// Allgather with a non-contiguous type on either side: pack this rank's
// contribution on the device, gather the packed bytes, and unpack all n
// blocks with one launch (block i of recvbuf starts i*recvcount extents in,
// so the n blocks are n*recvcount consecutive elements of recvtype).  The
// reference stages derived types through Localcopy / segment pack
// (allgather_osu.c:2426, helper_fns.h:62-250).
static int allgather_derived(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                             MPI_Datatype recvtype, MPI_Comm comm) {
    const long rsize = dtype_size(recvtype), rext = dtype_extent(recvtype);
    const long psize = rsize * recvcount;
    if (sendbuf != MPI_IN_PLACE && dtype_size(sendtype) * sendcount != psize) return MPI_ERR_TRUNCATE;
    if (psize == 0) return MPI_SUCCESS;
    const int n = comm == MPI_COMM_SELF ? 1 : mv2h_size(), me = comm == MPI_COMM_SELF ? 0 : mv2h_rank();
    void *mine = pool_get((size_t)psize), *all = mine ? pool_get((size_t)psize * n) : nullptr;
    if (!all) {
        if (mine) pool_put(mine);
        return MPI_ERR_NO_MEM;
    }
    int pos = 0, rc;
    if (sendbuf == MPI_IN_PLACE)
        rc = PMPI_Pack((const char *)recvbuf + (long)me * recvcount * rext, recvcount, recvtype, mine, (int)psize, &pos,
                       comm);
    else
        rc = PMPI_Pack(sendbuf, sendcount, sendtype, mine, (int)psize, &pos, comm);
    if (!rc) rc = n > 1 ? mv2h_allgather(mine, all, (size_t)psize, nullptr) : mv2h_memcpy_dtod(all, mine, (size_t)psize);
    pos = 0;
    if (!rc) rc = PMPI_Unpack(all, (int)(psize * n), &pos, recvbuf, recvcount * n, recvtype, comm);
    pool_put(mine);
    pool_put(all);
    return rc;
}

int PMPI_Allgather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                   MPI_Datatype recvtype, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Allgather";
    if (!g_initialized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, fn);
    if (allgather_alias(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm_rank_of(comm)))
        return err_return(comm, MPI_ERR_BUFFER, fn);
    if (recvcount < 0 || (sendbuf != MPI_IN_PLACE && sendcount < 0)) return err_return(comm, MPI_ERR_COUNT, fn);
    if (!dtype_valid(recvtype) || (sendbuf != MPI_IN_PLACE && !dtype_valid(sendtype)))
        return err_return(comm, MPI_ERR_TYPE, fn);
    if (!dtype_committed(recvtype) || (sendbuf != MPI_IN_PLACE && !dtype_committed(sendtype)))
        return err_return(comm, MPI_ERR_TYPE, fn);
    if (const int rc = allgather_buf_checks(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype))
        return err_return(comm, rc, fn);
    if (!dtype_is_contiguous(recvtype) || (sendbuf != MPI_IN_PLACE && !dtype_is_contiguous(sendtype)))
        return err_return(comm, allgather_derived(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm), fn);
    const size_t rbytes = (size_t)dtype_span(recvtype, recvcount);
    if (sendbuf != MPI_IN_PLACE && (size_t)dtype_span(sendtype, sendcount) != rbytes)
        return err_return(comm, MPI_ERR_TRUNCATE, fn);
    if (rbytes == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) {
        int rc = sendbuf == MPI_IN_PLACE ? 0 : mv2h_memcpy_dtod(recvbuf, sendbuf, rbytes);
        return err_return(comm, rc, fn);
    }
    return err_return(comm, mv2h_allgather(sendbuf, recvbuf, rbytes, nullptr), fn);
}
int MPI_Allgather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                  MPI_Datatype recvtype, MPI_Comm comm) WEAK(MPI_Allgather);

// ---------------------------------------------------------------------------
// MPI_Alltoall / MPI_Alltoallv (alltoall.c:650-713, alltoallv.c:520-594 for the checks).
// MPI_IN_PLACE is the send buffer only; with it the send count and type (sendcounts / sdispls)
// are ignored and the blocks are read from recvbuf.
// ---------------------------------------------------------------------------
static int alltoall_checks(const void *sendbuf, int sendcount, MPI_Datatype sendtype, const void *recvbuf,
                           int recvcount, MPI_Datatype recvtype, MPI_Comm comm) {
    if (!g_initialized || g_finalized) return MPI_ERR_OTHER;
    if (comm_index(comm) < 0) return MPI_ERR_COMM;
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (recvcount < 0 || (!in_place && sendcount < 0)) return MPI_ERR_COUNT;
    if (!dtype_valid(recvtype) || (!in_place && !dtype_valid(sendtype))) return MPI_ERR_TYPE;
    if (!dtype_committed(recvtype) || (!in_place && !dtype_committed(sendtype))) return MPI_ERR_TYPE;
    if (!in_place && null_userbuf(sendbuf, sendcount, sendtype)) return MPI_ERR_BUFFER;
    if (inplace_buf(recvbuf, recvcount) || null_userbuf(recvbuf, recvcount, recvtype)) return MPI_ERR_BUFFER;
    if (!in_place && sendcount != 0 && recvcount != 0 && sendbuf == recvbuf) return MPI_ERR_BUFFER;  // alltoall.c:690-695
    return MPI_SUCCESS;
}

// Alltoall with a non-contiguous type on either side, the way of allgather_derived: pack the n
// send blocks on the device (block j is elements [j * sendcount, (j + 1) * sendcount), so the n
// blocks are n * sendcount consecutive elements), exchange the packed bytes, unpack n blocks.
static int alltoall_derived(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                            MPI_Datatype recvtype, MPI_Comm comm) {
    const long psize = dtype_size(recvtype) * recvcount;
    if (sendbuf != MPI_IN_PLACE && dtype_size(sendtype) * sendcount != psize) return MPI_ERR_TRUNCATE;
    if (psize == 0) return MPI_SUCCESS;
    const int n = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    void *out = pool_get((size_t)psize * n), *in = out ? pool_get((size_t)psize * n) : nullptr;
    if (!in) {
        if (out) pool_put(out);
        return MPI_ERR_NO_MEM;
    }
    int pos = 0, rc;
    if (sendbuf == MPI_IN_PLACE) rc = PMPI_Pack(recvbuf, recvcount * n, recvtype, out, (int)(psize * n), &pos, comm);
    else rc = PMPI_Pack(sendbuf, sendcount * n, sendtype, out, (int)(psize * n), &pos, comm);
    if (!rc) rc = n > 1 ? mv2h_alltoall(out, in, (size_t)psize, nullptr) : mv2h_memcpy_dtod(in, out, (size_t)psize);
    pos = 0;
    if (!rc) rc = PMPI_Unpack(in, (int)(psize * n), &pos, recvbuf, recvcount * n, recvtype, comm);
    pool_put(out);
    pool_put(in);
    return rc;
}

int PMPI_Alltoall(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                  MPI_Datatype recvtype, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Alltoall";
    if (const int rc = alltoall_checks(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm))
        return err_return(comm_index(comm) < 0 ? MPI_COMM_WORLD : comm, rc, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!dtype_is_contiguous(recvtype) || (!in_place && !dtype_is_contiguous(sendtype)))
        return err_return(comm, alltoall_derived(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm), fn);
    const size_t rbytes = (size_t)dtype_span(recvtype, recvcount);
    if (!in_place && (size_t)dtype_span(sendtype, sendcount) != rbytes) return err_return(comm, MPI_ERR_TRUNCATE, fn);
    if (rbytes == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) {
        int rc = MPI_SUCCESS;
        if (!in_place) rc = is_dev(recvbuf) || is_dev(sendbuf) ? mv2h_memcpy_dtod(recvbuf, sendbuf, rbytes) : (memcpy(recvbuf, sendbuf, rbytes), 0);
        return err_return(comm, rc, fn);
    }
    return err_return(comm, mv2h_alltoall(sendbuf, recvbuf, rbytes, nullptr), fn);
}
int MPI_Alltoall(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                 MPI_Datatype recvtype, MPI_Comm comm) WEAK(MPI_Alltoall);

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
extern "C++" {
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
        void *d = R.rt_buf() + R.offs[0];
        const void *s = S.rt_buf() + S.offs[0];
        if (R.bytes[0]) rc = is_dev(d) || is_dev(s) ? mv2h_memcpy_dtod(d, s, R.bytes[0]) : (memcpy(d, s, R.bytes[0]), 0);
    } else {
        rc = mv2h_alltoallv(S.rt_buf(), S.bytes.data(), S.offs.data(), R.rt_buf(), R.bytes.data(), R.offs.data(), nullptr);
    }
    return rc ? rc : wside_move(R, true);
}
}  // extern "C++"

// Counts and displacements are in elements (extents) of their side's type, as in the reference; the
// runtime takes bytes.  A non-contiguous type on either side goes the way of MPI_Alltoallw above.
int PMPI_Alltoallv(const void *sendbuf, const int sendcounts[], const int sdispls[], MPI_Datatype sendtype,
                   void *recvbuf, const int recvcounts[], const int rdispls[], MPI_Datatype recvtype, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Alltoallv";
    if (!g_initialized || g_finalized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!recvcounts || !rdispls || (!in_place && (!sendcounts || !sdispls))) return err_return(comm, MPI_ERR_ARG, fn);
    const int n = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    long stotal = 0, rtotal = 0;
    for (int j = 0; j < n; ++j) {
        if (recvcounts[j] < 0 || (!in_place && sendcounts[j] < 0)) return err_return(comm, MPI_ERR_COUNT, fn);
        rtotal += recvcounts[j];
        if (!in_place) stotal += sendcounts[j];
    }
    if (!dtype_valid(recvtype) || (!in_place && !dtype_valid(sendtype))) return err_return(comm, MPI_ERR_TYPE, fn);
    if (!dtype_committed(recvtype) || (!in_place && !dtype_committed(sendtype))) return err_return(comm, MPI_ERR_TYPE, fn);
    if (!in_place && null_userbuf(sendbuf, stotal, sendtype)) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (inplace_buf(recvbuf, rtotal) || null_userbuf(recvbuf, rtotal, recvtype)) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (!in_place && stotal && rtotal && sendbuf == recvbuf) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (!dtype_is_contiguous(recvtype) || (!in_place && !dtype_is_contiguous(sendtype))) {
        for (int j = 0; j < n; ++j)
            if ((recvcounts[j] && rdispls[j] < 0) || (!in_place && sendcounts[j] && sdispls[j] < 0))
                return err_return(comm, MPI_ERR_ARG, fn);
        if (const int rc = a2aw_one_node_only(comm, fn)) return err_return(comm, rc, fn);
        WSide S, R;
        wside_set(R, recvbuf, n, recvcounts, rdispls, nullptr, recvtype);
        if (!in_place) wside_set(S, sendbuf, n, sendcounts, sdispls, nullptr, sendtype);
        return err_return(comm, a2aw_run(S, R, in_place, comm), fn);
    }
    const size_t rext = (size_t)dtype_span(recvtype, 1), sext = in_place ? rext : (size_t)dtype_span(sendtype, 1);
    std::vector<size_t> sb(n), so(n), rb(n), ro(n);
    for (int j = 0; j < n; ++j) {
        // a displacement matters only where its count is not zero
        if ((recvcounts[j] && rdispls[j] < 0) || (!in_place && sendcounts[j] && sdispls[j] < 0))
            return err_return(comm, MPI_ERR_ARG, fn);
        rb[j] = (size_t)recvcounts[j] * rext;
        ro[j] = recvcounts[j] ? (size_t)rdispls[j] * rext : 0;
        sb[j] = in_place ? rb[j] : (size_t)sendcounts[j] * sext;
        so[j] = in_place ? ro[j] : (sendcounts[j] ? (size_t)sdispls[j] * sext : 0);
    }
    if (comm == MPI_COMM_SELF) {
        if (sb[0] != rb[0]) return err_return(comm, MPI_ERR_TRUNCATE, fn);
        int rc = MPI_SUCCESS;
        if (!in_place && rb[0]) {
            void *d = (char *)recvbuf + ro[0];
            const void *s = (const char *)sendbuf + so[0];
            rc = is_dev(d) || is_dev(s) ? mv2h_memcpy_dtod(d, s, rb[0]) : (memcpy(d, s, rb[0]), 0);
        }
        return err_return(comm, rc, fn);
    }
    return err_return(comm, mv2h_alltoallv(sendbuf, sb.data(), so.data(), recvbuf, rb.data(), ro.data(), nullptr), fn);
}
int MPI_Alltoallv(const void *sendbuf, const int sendcounts[], const int sdispls[], MPI_Datatype sendtype, void *recvbuf,
                  const int recvcounts[], const int rdispls[], MPI_Datatype recvtype, MPI_Comm comm) WEAK(MPI_Alltoallv);

// Checks in MPI_Alltoallv's order here: communicator, arrays, then per block count, type and
// committed (a type matters only where its count is not zero, alltoallw.c:483-507), the buffers
// (:509-521), the alias check (:474-475).  MPI_IN_PLACE takes counts, displacements and types from
// the receive side.  Displacements are bytes; one matters only where its count is not zero.
int PMPI_Alltoallw(const void *sendbuf, const int sendcounts[], const int sdispls[], const MPI_Datatype sendtypes[],
                   void *recvbuf, const int recvcounts[], const int rdispls[], const MPI_Datatype recvtypes[],
                   MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Alltoallw";
    if (!g_initialized || g_finalized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!recvcounts || !rdispls || !recvtypes || (!in_place && (!sendcounts || !sdispls || !sendtypes)))
        return err_return(comm, MPI_ERR_ARG, fn);
    const int n = comm == MPI_COMM_SELF ? 1 : mv2h_size();
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
    for (int j = 0; j < n; ++j)
        if ((recvcounts[j] && rdispls[j] < 0) || (!in_place && sendcounts[j] && sdispls[j] < 0))
            return err_return(comm, MPI_ERR_ARG, fn);
    if (const int rc = a2aw_one_node_only(comm, fn)) return err_return(comm, rc, fn);
    WSide S, R;
    wside_set(R, recvbuf, n, recvcounts, rdispls, recvtypes, MPI_DATATYPE_NULL);
    if (!in_place) wside_set(S, sendbuf, n, sendcounts, sdispls, sendtypes, MPI_DATATYPE_NULL);
    return err_return(comm, a2aw_run(S, R, in_place, comm), fn);
}
int MPI_Alltoallw(const void *sendbuf, const int sendcounts[], const int sdispls[], const MPI_Datatype sendtypes[],
                  void *recvbuf, const int recvcounts[], const int rdispls[], const MPI_Datatype recvtypes[],
                  MPI_Comm comm) WEAK(MPI_Alltoallw);

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
// the same way, and the collective itself moves packed bytes (as alltoall_derived does).
// ---------------------------------------------------------------------------
extern "C++" {
static int copy_any(void *d, const void *s, size_t bytes) {
    if (!bytes || d == s) return MPI_SUCCESS;
    return is_dev(d) || is_dev(s) ? mv2h_memcpy_dtod(d, s, bytes) : (memcpy(d, s, bytes), 0);
}

static int side_checks(long count, MPI_Datatype dt) {
    if (count < 0) return MPI_ERR_COUNT;
    if (!dtype_valid(dt) || !dtype_committed(dt)) return MPI_ERR_TYPE;
    return MPI_SUCCESS;
}

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

// comm, then root (MPI_ERR_ROOT); *n, *me: the communicator's size and this rank in it
static int rooted_comm_checks(MPI_Comm comm, int root, int *n, int *me) {
    if (!g_initialized || g_finalized) return MPI_ERR_OTHER;
    if (comm_index(comm) < 0) return MPI_ERR_COMM;
    *n = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    *me = comm_rank_of(comm);
    const int csize = comm == MPI_COMM_SELF ? 1 : world().gsize;
    if (root < 0 || root >= csize) return MPI_ERR_ROOT;
    return MPI_SUCCESS;
}

static long sum_counts(const int *c, int n) {
    long s = 0;
    for (int j = 0; j < n; ++j) s += c[j];
    return s;
}

}  // extern "C++"

#define GS_FAIL(rc) return err_return(comm_index(comm) < 0 ? MPI_COMM_WORLD : comm, (rc), fn)

int PMPI_Gather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                MPI_Datatype recvtype, int root, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Gather";
    int n = 1, me = 0, rc;
    if ((rc = rooted_comm_checks(comm, root, &n, &me))) GS_FAIL(rc);
    const bool at_root = me == root, in_place = sendbuf == MPI_IN_PLACE;
    if (in_place && !at_root) GS_FAIL(MPI_ERR_BUFFER);
    if (!in_place) {
        if ((rc = side_checks(sendcount, sendtype))) GS_FAIL(rc);
        if (null_userbuf(sendbuf, sendcount, sendtype)) GS_FAIL(MPI_ERR_BUFFER);
    }
    NBlocks rb;
    if (at_root) {
        if ((rc = side_checks(recvcount, recvtype))) GS_FAIL(rc);
        if (inplace_buf(recvbuf, recvcount) || null_userbuf(recvbuf, recvcount, recvtype)) GS_FAIL(MPI_ERR_BUFFER);
        // gather.c:880-886: the send buffer is the root's own block of the receive buffer
        if (!in_place && sendtype == recvtype && sendcount != 0 && recvcount != 0 &&
            sendbuf == (const char *)recvbuf + (long)me * recvcount * dtype_size(recvtype))
            GS_FAIL(MPI_ERR_BUFFER);
        if ((rc = nblocks_init(rb, recvbuf, n, &recvcount, nullptr, recvtype))) GS_FAIL(rc);
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
int MPI_Gather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
               MPI_Datatype recvtype, int root, MPI_Comm comm) WEAK(MPI_Gather);

int PMPI_Gatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
                 const int displs[], MPI_Datatype recvtype, int root, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Gatherv";
    int n = 1, me = 0, rc;
    if ((rc = rooted_comm_checks(comm, root, &n, &me))) GS_FAIL(rc);
    const bool at_root = me == root, in_place = sendbuf == MPI_IN_PLACE;
    if (in_place && !at_root) GS_FAIL(MPI_ERR_BUFFER);
    if (!in_place) {
        if ((rc = side_checks(sendcount, sendtype))) GS_FAIL(rc);
        if (null_userbuf(sendbuf, sendcount, sendtype)) GS_FAIL(MPI_ERR_BUFFER);
    }
    NBlocks rb;
    if (at_root) {
        if (!recvcounts || !displs) GS_FAIL(MPI_ERR_ARG);
        for (int j = 0; j < n; ++j)
            if (recvcounts[j] < 0) GS_FAIL(MPI_ERR_COUNT);
        if ((rc = side_checks(0, recvtype))) GS_FAIL(rc);
        const long total = sum_counts(recvcounts, n);
        if (inplace_buf(recvbuf, total) || null_userbuf(recvbuf, total, recvtype)) GS_FAIL(MPI_ERR_BUFFER);
        if ((rc = nblocks_init(rb, recvbuf, n, recvcounts, displs, recvtype))) GS_FAIL(rc);
    }
    rc = gather_like(sendbuf, sendcount, sendtype, at_root ? &rb : nullptr, me, comm,
                     [&](const void *s, size_t sbytes, void *r, const size_t *rbytes, const size_t *roffs) {
                         return mv2h_gatherv(s, sbytes, r, rbytes, roffs, root, nullptr);
                     });
    return err_return(comm, rc, fn);
}
int MPI_Gatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
                const int displs[], MPI_Datatype recvtype, int root, MPI_Comm comm) WEAK(MPI_Gatherv);

int PMPI_Allgatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
                    const int displs[], MPI_Datatype recvtype, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Allgatherv";
    int n = 1, me = 0, rc;
    if ((rc = rooted_comm_checks(comm, 0, &n, &me))) GS_FAIL(rc);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!recvcounts || !displs) GS_FAIL(MPI_ERR_ARG);
    if (!in_place) {
        if ((rc = side_checks(sendcount, sendtype))) GS_FAIL(rc);
        if (null_userbuf(sendbuf, sendcount, sendtype)) GS_FAIL(MPI_ERR_BUFFER);
    }
    for (int j = 0; j < n; ++j)
        if (recvcounts[j] < 0) GS_FAIL(MPI_ERR_COUNT);
    if ((rc = side_checks(0, recvtype))) GS_FAIL(rc);
    const long total = sum_counts(recvcounts, n);
    if (inplace_buf(recvbuf, total) || null_userbuf(recvbuf, total, recvtype)) GS_FAIL(MPI_ERR_BUFFER);
    // allgatherv.c:1118-1124: the send buffer is this rank's block of the receive buffer
    if (!in_place && sendtype == recvtype && sendcount != 0 && recvcounts[me] != 0 &&
        sendbuf == (const char *)recvbuf + (long)displs[me] * dtype_size(recvtype))
        GS_FAIL(MPI_ERR_BUFFER);
    NBlocks rb;
    if ((rc = nblocks_init(rb, recvbuf, n, recvcounts, displs, recvtype))) GS_FAIL(rc);
    rc = gather_like(sendbuf, sendcount, sendtype, &rb, me, comm,
                     [&](const void *s, size_t sbytes, void *r, const size_t *rbytes, const size_t *roffs) {
                         return mv2h_allgatherv(s, sbytes, r, rbytes, roffs, nullptr);
                     });
    return err_return(comm, rc, fn);
}
int MPI_Allgatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
                   const int displs[], MPI_Datatype recvtype, MPI_Comm comm) WEAK(MPI_Allgatherv);

int PMPI_Scatter(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                 MPI_Datatype recvtype, int root, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Scatter";
    int n = 1, me = 0, rc;
    if ((rc = rooted_comm_checks(comm, root, &n, &me))) GS_FAIL(rc);
    const bool at_root = me == root, in_place = recvbuf == MPI_IN_PLACE;
    if (in_place && !at_root) GS_FAIL(MPI_ERR_BUFFER);
    NBlocks sb;
    if (at_root) {
        if ((rc = side_checks(sendcount, sendtype))) GS_FAIL(rc);
        if (inplace_buf(sendbuf, sendcount) || null_userbuf(sendbuf, sendcount, sendtype)) GS_FAIL(MPI_ERR_BUFFER);
    }
    if (!in_place) {
        if ((rc = side_checks(recvcount, recvtype))) GS_FAIL(rc);
        if (null_userbuf(recvbuf, recvcount, recvtype)) GS_FAIL(MPI_ERR_BUFFER);
    }
    if (at_root) {
        // scatter.c:790-796: the receive buffer is the root's own block of the send buffer
        if (!in_place && sendtype == recvtype && sendcount != 0 && recvcount != 0 &&
            recvbuf == (const char *)sendbuf + (long)me * sendcount * dtype_size(sendtype))
            GS_FAIL(MPI_ERR_BUFFER);
        if ((rc = nblocks_init(sb, sendbuf, n, &sendcount, nullptr, sendtype))) GS_FAIL(rc);
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
int MPI_Scatter(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                MPI_Datatype recvtype, int root, MPI_Comm comm) WEAK(MPI_Scatter);

int PMPI_Scatterv(const void *sendbuf, const int sendcounts[], const int displs[], MPI_Datatype sendtype, void *recvbuf,
                  int recvcount, MPI_Datatype recvtype, int root, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Scatterv";
    int n = 1, me = 0, rc;
    if ((rc = rooted_comm_checks(comm, root, &n, &me))) GS_FAIL(rc);
    const bool at_root = me == root, in_place = recvbuf == MPI_IN_PLACE;
    if (in_place && !at_root) GS_FAIL(MPI_ERR_BUFFER);
    NBlocks sb;
    if (at_root) {
        if (!sendcounts || !displs) GS_FAIL(MPI_ERR_ARG);
        for (int j = 0; j < n; ++j)
            if (sendcounts[j] < 0) GS_FAIL(MPI_ERR_COUNT);
        if ((rc = side_checks(0, sendtype))) GS_FAIL(rc);
        const long total = sum_counts(sendcounts, n);
        if (inplace_buf(sendbuf, total) || null_userbuf(sendbuf, total, sendtype)) GS_FAIL(MPI_ERR_BUFFER);
    }
    if (!in_place) {
        if ((rc = side_checks(recvcount, recvtype))) GS_FAIL(rc);
        if (null_userbuf(recvbuf, recvcount, recvtype)) GS_FAIL(MPI_ERR_BUFFER);
    }
    if (at_root && (rc = nblocks_init(sb, sendbuf, n, sendcounts, displs, sendtype))) GS_FAIL(rc);
    rc = scatter_like(at_root ? &sb : nullptr, recvbuf, recvcount, recvtype, comm,
                      [&](const void *s, const size_t *sbytes, const size_t *soffs, void *r, size_t rbytes) {
                          return mv2h_scatterv(s, sbytes, soffs, r, rbytes, root, nullptr);
                      });
    return err_return(comm, rc, fn);
}
int MPI_Scatterv(const void *sendbuf, const int sendcounts[], const int displs[], MPI_Datatype sendtype, void *recvbuf,
                 int recvcount, MPI_Datatype recvtype, int root, MPI_Comm comm) WEAK(MPI_Scatterv);
#undef GS_FAIL

int PMPI_Bcast(void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPI_Bcast";
    if (!g_initialized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, fn);
    if (count < 0) return err_return(comm, MPI_ERR_COUNT, fn);
    if (!dtype_valid(dt)) return err_return(comm, MPI_ERR_TYPE, fn);
    const int size = comm == MPI_COMM_SELF ? 1 : mv2h_size();
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
    int pos = 0, rc = MPI_SUCCESS;
    if (mv2h_rank() == root) rc = PMPI_Pack(buffer, count, dt, packed, psize, &pos, comm);
    if (!rc) rc = mv2h_bcast(packed, (size_t)psize, root, nullptr);
    pos = 0;
    if (!rc && mv2h_rank() != root) rc = PMPI_Unpack(packed, psize, &pos, buffer, count, dt, comm);
    pool_put(packed);
    return err_return(comm, rc, fn);
}
int MPI_Bcast(void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm) WEAK(MPI_Bcast);

// ---------------------------------------------------------------------------
// Stream-ordered collectives (extension; mv2h.h *_enqueue): argument checks of the blocking
// calls, then the same algorithms launched on the caller's HIP stream without waiting.
// Calls the host would have to finish after the kernel — user ops, x87 types, derived
// types, host buffers — are refused with MPI_ERR_ARG / MPI_ERR_TYPE instead of blocking.
// ---------------------------------------------------------------------------
static int enqueue_arg_checks(MPI_Datatype dt, MPI_Op op, void *stream) {
    if (!stream) return MPI_ERR_ARG;
    if (user_op(op)) return MPI_ERR_ARG;
    if (is_x87(dt) || !dtype_is_contiguous(dt)) return MPI_ERR_TYPE;
    return MPI_SUCCESS;
}

int PMPIX_Allreduce_enqueue(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
                            void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPIX_Allreduce_enqueue";
    int rc = coll_checks(comm, count, dt, op, allreduce_buf_checks(sendbuf, recvbuf, count, dt));
    if (!rc) rc = enqueue_arg_checks(dt, op, stream);
    if (rc) return err_return(comm, rc, fn);
    if (count == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) {  // a stream-ordered copy
        if (sendbuf == MPI_IN_PLACE || sendbuf == recvbuf) return MPI_SUCCESS;
        if (!is_dev(sendbuf) || !is_dev(recvbuf)) return err_return(comm, MPI_ERR_ARG, fn);
        return err_return(comm, mv2h_copy_enqueue(recvbuf, sendbuf, (size_t)dtype_span(dt, count), stream), fn);
    }
    return err_return(comm, mv2h_allreduce_enqueue(sendbuf, recvbuf, (size_t)count, dt, op, stream), fn);
}
int MPIX_Allreduce_enqueue(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
                           void *stream) WEAK(MPIX_Allreduce_enqueue);

int PMPIX_Reduce_enqueue(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, int root,
                         MPI_Comm comm, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPIX_Reduce_enqueue";
    if (!g_initialized || g_finalized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(comm, MPI_ERR_COMM, fn);
    const int size = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    if (root < 0 || root >= size) return err_return(comm, MPI_ERR_ROOT, fn);
    int rc = coll_checks(comm, count, dt, op, reduce_buf_checks(sendbuf, recvbuf, count, dt, comm_rank_of(comm) == root));
    if (!rc) rc = enqueue_arg_checks(dt, op, stream);
    if (rc) return err_return(comm, rc, fn);
    if (count == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) return PMPIX_Allreduce_enqueue(sendbuf, recvbuf, count, dt, op, comm, stream);
    return err_return(comm, mv2h_reduce_enqueue(sendbuf, recvbuf, (size_t)count, dt, op, root, stream), fn);
}
int MPIX_Reduce_enqueue(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, int root,
                        MPI_Comm comm, void *stream) WEAK(MPIX_Reduce_enqueue);

int PMPIX_Reduce_scatter_enqueue(const void *sendbuf, void *recvbuf, const int recvcounts[], MPI_Datatype dt, MPI_Op op,
                                 MPI_Comm comm, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPIX_Reduce_scatter_enqueue";
    if (!g_initialized || g_finalized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(comm, MPI_ERR_COMM, fn);
    if (!recvcounts) return err_return(comm, MPI_ERR_ARG, fn);
    const int n = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    std::vector<size_t> rc_sz(n);
    size_t total = 0;
    for (int j = 0; j < n; ++j) {
        if (recvcounts[j] < 0) return err_return(comm, MPI_ERR_COUNT, fn);
        rc_sz[j] = (size_t)recvcounts[j];
        total += rc_sz[j];
    }
    int rc = coll_checks(comm, 0, dt, op,
                         reduce_scatter_buf_checks(sendbuf, recvbuf, recvcounts[comm_rank_of(comm)], (long)total, dt));
    if (!rc) rc = enqueue_arg_checks(dt, op, stream);
    if (rc) return err_return(comm, rc, fn);
    if (total == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) return PMPIX_Allreduce_enqueue(sendbuf, recvbuf, recvcounts[0], dt, op, comm, stream);
    return err_return(comm, mv2h_reduce_scatter_enqueue(sendbuf, recvbuf, rc_sz.data(), dt, op, stream), fn);
}
int MPIX_Reduce_scatter_enqueue(const void *sendbuf, void *recvbuf, const int recvcounts[], MPI_Datatype dt, MPI_Op op,
                                MPI_Comm comm, void *stream) WEAK(MPIX_Reduce_scatter_enqueue);

int PMPIX_Allgather_enqueue(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                            MPI_Datatype recvtype, MPI_Comm comm, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPIX_Allgather_enqueue";
    if (!g_initialized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, fn);
    if (!stream) return err_return(comm, MPI_ERR_ARG, fn);
    if (allgather_alias(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm_rank_of(comm)))
        return err_return(comm, MPI_ERR_BUFFER, fn);
    if (recvcount < 0 || (sendbuf != MPI_IN_PLACE && sendcount < 0)) return err_return(comm, MPI_ERR_COUNT, fn);
    if (!dtype_valid(recvtype) || (sendbuf != MPI_IN_PLACE && !dtype_valid(sendtype)))
        return err_return(comm, MPI_ERR_TYPE, fn);
    if (!dtype_committed(recvtype) || (sendbuf != MPI_IN_PLACE && !dtype_committed(sendtype)))
        return err_return(comm, MPI_ERR_TYPE, fn);
    if (const int rc = allgather_buf_checks(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype))
        return err_return(comm, rc, fn);
    if (!dtype_is_contiguous(recvtype) || (sendbuf != MPI_IN_PLACE && !dtype_is_contiguous(sendtype)))
        return err_return(comm, MPI_ERR_TYPE, fn);
    const size_t rbytes = (size_t)dtype_span(recvtype, recvcount);
    if (sendbuf != MPI_IN_PLACE && (size_t)dtype_span(sendtype, sendcount) != rbytes)
        return err_return(comm, MPI_ERR_TRUNCATE, fn);
    if (rbytes == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) {
        if (sendbuf == MPI_IN_PLACE || sendbuf == recvbuf) return MPI_SUCCESS;
        if (!is_dev(sendbuf) || !is_dev(recvbuf)) return err_return(comm, MPI_ERR_ARG, fn);
        return err_return(comm, mv2h_copy_enqueue(recvbuf, sendbuf, rbytes, stream), fn);
    }
    return err_return(comm, mv2h_allgather_enqueue(sendbuf, recvbuf, rbytes, stream), fn);
}
int MPIX_Allgather_enqueue(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                           MPI_Datatype recvtype, MPI_Comm comm, void *stream) WEAK(MPIX_Allgather_enqueue);

int PMPIX_Alltoall_enqueue(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                           MPI_Datatype recvtype, MPI_Comm comm, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPIX_Alltoall_enqueue";
    if (const int rc = alltoall_checks(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm))
        return err_return(comm_index(comm) < 0 ? MPI_COMM_WORLD : comm, rc, fn);
    if (!stream) return err_return(comm, MPI_ERR_ARG, fn);
    const bool in_place = sendbuf == MPI_IN_PLACE;
    if (!dtype_is_contiguous(recvtype) || (!in_place && !dtype_is_contiguous(sendtype)))
        return err_return(comm, MPI_ERR_TYPE, fn);
    const size_t rbytes = (size_t)dtype_span(recvtype, recvcount);
    if (!in_place && (size_t)dtype_span(sendtype, sendcount) != rbytes) return err_return(comm, MPI_ERR_TRUNCATE, fn);
    if (rbytes == 0) return MPI_SUCCESS;
    if (comm == MPI_COMM_SELF) {
        if (in_place) return MPI_SUCCESS;
        if (!is_dev(sendbuf) || !is_dev(recvbuf)) return err_return(comm, MPI_ERR_ARG, fn);
        return err_return(comm, mv2h_copy_enqueue(recvbuf, sendbuf, rbytes, stream), fn);
    }
    return err_return(comm, mv2h_alltoall_enqueue(sendbuf, recvbuf, rbytes, stream), fn);
}
int MPIX_Alltoall_enqueue(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                          MPI_Datatype recvtype, MPI_Comm comm, void *stream) WEAK(MPIX_Alltoall_enqueue);

int PMPIX_Bcast_enqueue(void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm, void *stream) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    const char *fn = "MPIX_Bcast_enqueue";
    if (!g_initialized) return err_return(comm, MPI_ERR_OTHER, fn);
    if (comm_index(comm) < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, fn);
    if (!stream) return err_return(comm, MPI_ERR_ARG, fn);
    if (count < 0) return err_return(comm, MPI_ERR_COUNT, fn);
    if (!dtype_valid(dt) || !dtype_committed(dt)) return err_return(comm, MPI_ERR_TYPE, fn);
    if (!dtype_is_contiguous(dt)) return err_return(comm, MPI_ERR_TYPE, fn);
    const int size = comm == MPI_COMM_SELF ? 1 : mv2h_size();
    if (root < 0 || root >= size) return err_return(comm, MPI_ERR_ROOT, fn);
    if (inplace_buf(buffer, count) || null_userbuf(buffer, count, dt)) return err_return(comm, MPI_ERR_BUFFER, fn);
    if (count == 0 || size == 1) return MPI_SUCCESS;
    return err_return(comm, mv2h_bcast_enqueue(buffer, (size_t)dtype_span(dt, count), root, stream), fn);
}
int MPIX_Bcast_enqueue(void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm, void *stream)
    WEAK(MPIX_Bcast_enqueue);

int PMPIX_Enqueue_check(MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    if (comm_index(comm) < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_COMM, "MPIX_Enqueue_check");
    return err_return(comm, mv2h_enqueue_check(), "MPIX_Enqueue_check");
}
int MPIX_Enqueue_check(MPI_Comm comm) WEAK(MPIX_Enqueue_check);

}  // extern "C"

// ---------------------------------------------------------------- requests
// One table for nonblocking collectives (completion-word tickets, mv2h_defer_*)
// and point-to-point requests (mv2h_isend / mv2h_irecv ids).  Handles are
// kReqBase | slot; MPI_REQUEST_NULL is MPICH's 0x2c000000.
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
std::vector<MReq> g_mreqs;
constexpr MPI_Request kReqBase = (MPI_Request)0xac000000;

MPI_Request req_new(const MReq &r) {
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

MReq *req_get(MPI_Request h) {
    if ((h & 0xfc000000) != (kReqBase & 0xfc000000)) return nullptr;
    const size_t i = (size_t)(h & 0x03ffffff);
    return i < g_mreqs.size() && g_mreqs[i].live ? &g_mreqs[i] : nullptr;
}

void status_set(MPI_Status *st, int src, int tag, size_t bytes, int err) {
    if (!st || st == MPI_STATUS_IGNORE) return;
    st->MPI_SOURCE = src;
    st->MPI_TAG = tag;
    st->MPI_ERROR = err;
    st->count_lo = (int)(bytes & 0xffffffffu);
    st->count_hi_and_cancelled = (int)((bytes >> 32) << 1);
}

void tmp_free(MReq &r) {
    if (!r.tmp) return;
    if (r.tmp_dev) pool_put(r.tmp);
    else free(r.tmp);
    r.tmp = nullptr;
}

// finish a request whose underlying operation completed (rc = its error class)
int req_finish(MReq &r, int rc, int src, int tag, size_t bytes, MPI_Status *st) {
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

int req_wait(MReq &r, MPI_Status *st) {
    int src = MPI_ANY_SOURCE, tag = MPI_ANY_TAG, rc = MPI_SUCCESS;
    size_t bytes = 0;
    if (r.kind == RQ_COLL) rc = r.err ? r.err : mv2h_wait_ticket(r.id);
    else if (r.kind == RQ_P2P) rc = mv2h_p2p_wait(r.id, &src, &tag, &bytes);
    return req_finish(r, rc, src, tag, bytes, st);
}

int req_test(MReq &r, int *flag, MPI_Status *st) {
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
int start_coll(MPI_Request *request, const char *fn, F &&call, int nbc = MV2H_NBC_NONE) {
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

int p2p_checks(MPI_Comm comm, int count, MPI_Datatype dt, int tag, bool recv) {
    if (!g_initialized) return MPI_ERR_OTHER;
    if (comm != MPI_COMM_WORLD) return comm_index(comm) < 0 ? MPI_ERR_COMM : MPI_ERR_UNSUPPORTED_OPERATION;
    if (count < 0) return MPI_ERR_COUNT;
    if (!dtype_valid(dt) || !dtype_committed(dt)) return MPI_ERR_TYPE;
    if (recv ? (tag < 0 && tag != MPI_ANY_TAG) : tag < 0) return MPI_ERR_TAG;
    return MPI_SUCCESS;
}

int isend_impl(const void *buf, int count, MPI_Datatype dt, int dest, int tag, MPI_Request *request) {
    MReq r;
    if (dest == MPI_PROC_NULL) {
        r.kind = RQ_DONE;
        r.src = MPI_PROC_NULL;
        *request = req_new(r);
        return MPI_SUCCESS;
    }
    if (dest < 0 || dest >= world().gsize) return MPI_ERR_RANK;
    r.kind = RQ_P2P;
    const void *src = buf;
    size_t bytes = (size_t)dtype_span(dt, count);
    if (!dtype_is_contiguous(dt)) {  // device (or host) pack first, the packed copy travels
        int psize = 0, pos = 0;
        PMPI_Pack_size(count, dt, MPI_COMM_WORLD, &psize);
        r.tmp_dev = is_dev(buf);
        if (r.tmp_dev) {
            if (!(r.tmp = pool_get((size_t)psize))) return MPI_ERR_NO_MEM;
        } else if (!(r.tmp = malloc((size_t)psize + 1))) {
            return MPI_ERR_NO_MEM;
        }
        const int rc = PMPI_Pack(buf, count, dt, r.tmp, psize, &pos, MPI_COMM_WORLD);
        if (rc) {
            tmp_free(r);
            return rc;
        }
        src = r.tmp;
        bytes = (size_t)pos;
    }
    const int rc = mv2h_isend(src, bytes, dest, tag, &r.id);
    if (rc) {
        tmp_free(r);
        return rc;
    }
    *request = req_new(r);
    return MPI_SUCCESS;
}

int irecv_impl(void *buf, int count, MPI_Datatype dt, int source, int tag, MPI_Request *request) {
    MReq r;
    r.is_recv = true;
    if (source == MPI_PROC_NULL) {
        r.kind = RQ_DONE;
        r.src = MPI_PROC_NULL;
        *request = req_new(r);
        return MPI_SUCCESS;
    }
    if (source != MPI_ANY_SOURCE && (source < 0 || source >= world().gsize)) return MPI_ERR_RANK;
    r.kind = RQ_P2P;
    void *dst = buf;
    size_t cap = (size_t)dtype_span(dt, count);
    if (!dtype_is_contiguous(dt)) {  // receive packed, unpack at completion
        int psize = 0;
        PMPI_Pack_size(count, dt, MPI_COMM_WORLD, &psize);
        r.tmp_dev = is_dev(buf);
        if (r.tmp_dev) {
            if (!(r.tmp = pool_get((size_t)psize))) return MPI_ERR_NO_MEM;
        } else if (!(r.tmp = malloc((size_t)psize + 1))) {
            return MPI_ERR_NO_MEM;
        }
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

}  // namespace

extern "C" {

int PMPI_Iallreduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
                    MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(
        request, "MPI_Iallreduce", [&] { return PMPI_Allreduce(sendbuf, recvbuf, count, dt, op, comm); },
        MV2H_NBC_IALLREDUCE);
}
int MPI_Iallreduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
                   MPI_Request *request) WEAK(MPI_Iallreduce);

// the schedules make MPIR_Scan_generic's / MPIR_Exscan's calls in the same order (iscan.c:72-160,
// iexscan.c): the blocking programs
int PMPI_Iscan(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
               MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Iscan", [&] { return PMPI_Scan(sendbuf, recvbuf, count, dt, op, comm); });
}
int MPI_Iscan(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
              MPI_Request *request) WEAK(MPI_Iscan);

int PMPI_Iexscan(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
                 MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Iexscan", [&] { return PMPI_Exscan(sendbuf, recvbuf, count, dt, op, comm); });
}
int MPI_Iexscan(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, MPI_Comm comm,
                MPI_Request *request) WEAK(MPI_Iexscan);

int PMPI_Ireduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, int root, MPI_Comm comm,
                 MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(
        request, "MPI_Ireduce", [&] { return PMPI_Reduce(sendbuf, recvbuf, count, dt, op, root, comm); },
        MV2H_NBC_IREDUCE);
}
int MPI_Ireduce(const void *sendbuf, void *recvbuf, int count, MPI_Datatype dt, MPI_Op op, int root, MPI_Comm comm,
                MPI_Request *request) WEAK(MPI_Ireduce);

int PMPI_Ireduce_scatter(const void *sendbuf, void *recvbuf, const int recvcounts[], MPI_Datatype dt, MPI_Op op,
                         MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(
        request, "MPI_Ireduce_scatter", [&] { return PMPI_Reduce_scatter(sendbuf, recvbuf, recvcounts, dt, op, comm); },
        MV2H_NBC_IREDUCE_SCATTER);
}
int MPI_Ireduce_scatter(const void *sendbuf, void *recvbuf, const int recvcounts[], MPI_Datatype dt, MPI_Op op,
                        MPI_Comm comm, MPI_Request *request) WEAK(MPI_Ireduce_scatter);

int PMPI_Ireduce_scatter_block(const void *sendbuf, void *recvbuf, int recvcount, MPI_Datatype dt, MPI_Op op,
                               MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(
        request, "MPI_Ireduce_scatter_block",
        [&] { return PMPI_Reduce_scatter_block(sendbuf, recvbuf, recvcount, dt, op, comm); },
        MV2H_NBC_IREDUCE_SCATTER_BLOCK);
}
int MPI_Ireduce_scatter_block(const void *sendbuf, void *recvbuf, int recvcount, MPI_Datatype dt, MPI_Op op,
                              MPI_Comm comm, MPI_Request *request) WEAK(MPI_Ireduce_scatter_block);

int PMPI_Iallgather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                    MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Iallgather", [&] {
        return PMPI_Allgather(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm);
    });
}
int MPI_Iallgather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                   MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request) WEAK(MPI_Iallgather);

int PMPI_Ialltoall(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                   MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Ialltoall", [&] {
        return PMPI_Alltoall(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, comm);
    });
}
int MPI_Ialltoall(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                  MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request) WEAK(MPI_Ialltoall);

// The ranks exchange their counts on the host at initiation (two host barriers), so initiation is
// not local: it returns once every rank of the node has initiated the call.  The data moves behind
// the request.
int PMPI_Ialltoallv(const void *sendbuf, const int sendcounts[], const int sdispls[], MPI_Datatype sendtype,
                    void *recvbuf, const int recvcounts[], const int rdispls[], MPI_Datatype recvtype, MPI_Comm comm,
                    MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Ialltoallv", [&] {
        return PMPI_Alltoallv(sendbuf, sendcounts, sdispls, sendtype, recvbuf, recvcounts, rdispls, recvtype, comm);
    });
}
int MPI_Ialltoallv(const void *sendbuf, const int sendcounts[], const int sdispls[], MPI_Datatype sendtype, void *recvbuf,
                   const int recvcounts[], const int rdispls[], MPI_Datatype recvtype, MPI_Comm comm,
                   MPI_Request *request) WEAK(MPI_Ialltoallv);

// As MPI_Ialltoallv: the counts are exchanged on the host at initiation, which is therefore not
// local; packing, exchange and unpacking run behind the request.
int PMPI_Ialltoallw(const void *sendbuf, const int sendcounts[], const int sdispls[], const MPI_Datatype sendtypes[],
                    void *recvbuf, const int recvcounts[], const int rdispls[], const MPI_Datatype recvtypes[],
                    MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Ialltoallw", [&] {
        return PMPI_Alltoallw(sendbuf, sendcounts, sdispls, sendtypes, recvbuf, recvcounts, rdispls, recvtypes, comm);
    });
}
int MPI_Ialltoallw(const void *sendbuf, const int sendcounts[], const int sdispls[], const MPI_Datatype sendtypes[],
                   void *recvbuf, const int recvcounts[], const int rdispls[], const MPI_Datatype recvtypes[],
                   MPI_Comm comm, MPI_Request *request) WEAK(MPI_Ialltoallw);

// MPI_Igather(v) / MPI_Iscatter(v) / MPI_Iallgatherv: the blocking calls initiated with deferred
// completion.  Igatherv's and Iscatterv's ranks meet on the host inside the initiation (the row
// exchange), so starting them is not local.
int PMPI_Igather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                 MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Igather", [&] {
        return PMPI_Gather(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, root, comm);
    });
}
int MPI_Igather(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) WEAK(MPI_Igather);

int PMPI_Igatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
                  const int displs[], MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Igatherv", [&] {
        return PMPI_Gatherv(sendbuf, sendcount, sendtype, recvbuf, recvcounts, displs, recvtype, root, comm);
    });
}
int MPI_Igatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
                 const int displs[], MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request)
    WEAK(MPI_Igatherv);

int PMPI_Iallgatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
                     const int displs[], MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Iallgatherv", [&] {
        return PMPI_Allgatherv(sendbuf, sendcount, sendtype, recvbuf, recvcounts, displs, recvtype, comm);
    });
}
int MPI_Iallgatherv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, const int recvcounts[],
                    const int displs[], MPI_Datatype recvtype, MPI_Comm comm, MPI_Request *request)
    WEAK(MPI_Iallgatherv);

int PMPI_Iscatter(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                  MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Iscatter", [&] {
        return PMPI_Scatter(sendbuf, sendcount, sendtype, recvbuf, recvcount, recvtype, root, comm);
    });
}
int MPI_Iscatter(const void *sendbuf, int sendcount, MPI_Datatype sendtype, void *recvbuf, int recvcount,
                 MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) WEAK(MPI_Iscatter);

int PMPI_Iscatterv(const void *sendbuf, const int sendcounts[], const int displs[], MPI_Datatype sendtype, void *recvbuf,
                   int recvcount, MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Iscatterv", [&] {
        return PMPI_Scatterv(sendbuf, sendcounts, displs, sendtype, recvbuf, recvcount, recvtype, root, comm);
    });
}
int MPI_Iscatterv(const void *sendbuf, const int sendcounts[], const int displs[], MPI_Datatype sendtype, void *recvbuf,
                  int recvcount, MPI_Datatype recvtype, int root, MPI_Comm comm, MPI_Request *request)
    WEAK(MPI_Iscatterv);

int PMPI_Ibcast(void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Ibcast", [&] { return PMPI_Bcast(buffer, count, dt, root, comm); });
}
int MPI_Ibcast(void *buffer, int count, MPI_Datatype dt, int root, MPI_Comm comm, MPI_Request *request)
    WEAK(MPI_Ibcast);

int PMPI_Ibarrier(MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    return start_coll(request, "MPI_Ibarrier", [&] { return PMPI_Barrier(comm); });
}
int MPI_Ibarrier(MPI_Comm comm, MPI_Request *request) WEAK(MPI_Ibarrier);

int PMPI_Wait(MPI_Request *request, MPI_Status *status) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
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
int MPI_Wait(MPI_Request *request, MPI_Status *status) WEAK(MPI_Wait);

int PMPI_Test(MPI_Request *request, int *flag, MPI_Status *status) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
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
int MPI_Test(MPI_Request *request, int *flag, MPI_Status *status) WEAK(MPI_Test);

int PMPI_Waitall(int count, MPI_Request requests[], MPI_Status statuses[]) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
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
int MPI_Waitall(int count, MPI_Request requests[], MPI_Status statuses[]) WEAK(MPI_Waitall);

int PMPI_Testall(int count, MPI_Request requests[], int *flag, MPI_Status statuses[]) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
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
int MPI_Testall(int count, MPI_Request requests[], int *flag, MPI_Status statuses[]) WEAK(MPI_Testall);

int PMPI_Request_free(MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    if (!request) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Request_free");
    MReq *r = req_get(*request);
    if (!r) return err_return(MPI_COMM_WORLD, MPI_ERR_REQUEST, "MPI_Request_free");
    // the operation still completes; this library waits for it here
    req_wait(*r, MPI_STATUS_IGNORE);
    *request = MPI_REQUEST_NULL;
    return MPI_SUCCESS;
}
int MPI_Request_free(MPI_Request *request) WEAK(MPI_Request_free);

// ---------------------------------------------------------------- point-to-point
int PMPI_Isend(const void *buf, int count, MPI_Datatype dt, int dest, int tag, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    int rc = p2p_checks(comm, count, dt, tag, false);
    if (!rc && !request) rc = MPI_ERR_ARG;
    if (!rc) rc = isend_impl(buf, count, dt, dest, tag, request);
    return err_return(comm, rc, "MPI_Isend");
}
int MPI_Isend(const void *buf, int count, MPI_Datatype dt, int dest, int tag, MPI_Comm comm, MPI_Request *request)
    WEAK(MPI_Isend);

int PMPI_Irecv(void *buf, int count, MPI_Datatype dt, int source, int tag, MPI_Comm comm, MPI_Request *request) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    int rc = p2p_checks(comm, count, dt, tag, true);
    if (!rc && !request) rc = MPI_ERR_ARG;
    if (!rc) rc = irecv_impl(buf, count, dt, source, tag, request);
    return err_return(comm, rc, "MPI_Irecv");
}
int MPI_Irecv(void *buf, int count, MPI_Datatype dt, int source, int tag, MPI_Comm comm, MPI_Request *request)
    WEAK(MPI_Irecv);

int PMPI_Send(const void *buf, int count, MPI_Datatype dt, int dest, int tag, MPI_Comm comm) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    MPI_Request rq = MPI_REQUEST_NULL;
    int rc = p2p_checks(comm, count, dt, tag, false);
    if (!rc) rc = isend_impl(buf, count, dt, dest, tag, &rq);
    if (!rc) rc = req_wait(*req_get(rq), MPI_STATUS_IGNORE);
    return err_return(comm, rc, "MPI_Send");
}
int MPI_Send(const void *buf, int count, MPI_Datatype dt, int dest, int tag, MPI_Comm comm) WEAK(MPI_Send);

int PMPI_Recv(void *buf, int count, MPI_Datatype dt, int source, int tag, MPI_Comm comm, MPI_Status *status) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
    MPI_Request rq = MPI_REQUEST_NULL;
    int rc = p2p_checks(comm, count, dt, tag, true);
    if (!rc) rc = irecv_impl(buf, count, dt, source, tag, &rq);
    if (!rc) rc = req_wait(*req_get(rq), status);
    return err_return(comm, rc, "MPI_Recv");
}
int MPI_Recv(void *buf, int count, MPI_Datatype dt, int source, int tag, MPI_Comm comm, MPI_Status *status)
    WEAK(MPI_Recv);

int PMPI_Sendrecv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, int dest, int sendtag, void *recvbuf,
                  int recvcount, MPI_Datatype recvtype, int source, int recvtag, MPI_Comm comm, MPI_Status *status) {
    std::lock_guard<std::recursive_mutex> lk(g_cs);
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
int MPI_Sendrecv(const void *sendbuf, int sendcount, MPI_Datatype sendtype, int dest, int sendtag, void *recvbuf,
                 int recvcount, MPI_Datatype recvtype, int source, int recvtag, MPI_Comm comm, MPI_Status *status)
    WEAK(MPI_Sendrecv);

int PMPI_Get_count(const MPI_Status *status, MPI_Datatype dt, int *count) {
    if (!status || !count) return err_return(MPI_COMM_WORLD, MPI_ERR_ARG, "MPI_Get_count");
    const long tsz = dtype_size(dt);
    if (tsz < 0) return err_return(MPI_COMM_WORLD, MPI_ERR_TYPE, "MPI_Get_count");
    const unsigned long long bytes = (unsigned long long)(unsigned)status->count_lo |
                                     ((unsigned long long)((unsigned)status->count_hi_and_cancelled >> 1) << 32);
    if (tsz == 0) *count = 0;
    else *count = bytes % (unsigned long long)tsz ? MPI_UNDEFINED : (int)(bytes / (unsigned long long)tsz);
    return MPI_SUCCESS;
}
int MPI_Get_count(const MPI_Status *status, MPI_Datatype dt, int *count) WEAK(MPI_Get_count);

}  // extern "C"

/* scan_suite.c — the checks of the reference's scan tests (MPICH test/mpi/coll scantst.c,
 * exscan.c, exscan2.c, shipped with MVAPICH2 2.3.7) restated as one self-checking C program that
 * links the drop-in libmpi.so like any MPI application.  Operands live in host memory (`host`)
 * or in device memory (`device`: hipMalloc).
 *
 *   usage: mv2run -n N scan_suite {host|device} [case ...]
 *
 * Rank 0 prints one line per case ("<mem> <case> <errors>") and a TOTAL line; the exit status is
 * non-zero when any rank counted an error.  Expected values are closed forms of the rank. */
#include <hip/hip_runtime.h>
#include <mpi.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_dev, g_rank, g_size;

static void *buf_new(size_t bytes) {
    void *p = NULL;
    if (!bytes) bytes = 1;
    if (g_dev) {
        if (hipMalloc(&p, bytes) != hipSuccess) p = NULL;
    } else {
        p = malloc(bytes);
    }
    if (!p) {
        fprintf(stderr, "[%d] no memory for %zu bytes\n", g_rank, bytes);
        MPI_Abort(MPI_COMM_WORLD, 2);
    }
    return p;
}
static void buf_del(void *p) {
    if (g_dev) (void)hipFree(p);
    else free(p);
}
static void buf_set(void *b, const void *host, size_t bytes) {
    if (g_dev) (void)hipMemcpy(b, host, bytes, hipMemcpyHostToDevice);
    else memcpy(b, host, bytes);
}
static void buf_read(void *host, const void *b, size_t bytes) {
    if (g_dev) (void)hipMemcpy(host, b, bytes, hipMemcpyDeviceToHost);
    else memcpy(host, b, bytes);
}

/* one int in, one int out through operand buffers */
static int scan1(int excl, int in, int prefill, MPI_Op op, int *rc) {
    int out = prefill;
    int *s = buf_new(sizeof(int)), *r = buf_new(sizeof(int));
    buf_set(s, &in, sizeof(int));
    buf_set(r, &out, sizeof(int));
    *rc = excl ? MPI_Exscan(s, r, 1, MPI_INT, op, MPI_COMM_WORLD) : MPI_Scan(s, r, 1, MPI_INT, op, MPI_COMM_WORLD);
    buf_read(&out, r, sizeof(int));
    buf_del(s);
    buf_del(r);
    return out;
}

/* user functions of scantst.c: a sum declared commutative; and one declared non-commutative that
 * keeps the operand of the lower ranks and poisons the result when the operands arrive in any
 * order but ascending rank (inout = in op inout, in from the lower ranks) */
#define POISON 100000
static void uf_add(void *in_, void *io_, int *len, MPI_Datatype *dt) {
    (void)dt;
    const int *in = (const int *)in_;
    int *io = (int *)io_;
    for (int i = 0; i < *len; ++i) io[i] += in[i];
}
static void uf_ordered(void *in_, void *io_, int *len, MPI_Datatype *dt) {
    (void)dt;
    const int *in = (const int *)in_;
    int *io = (int *)io_;
    for (int i = 0; i < *len; ++i) io[i] = io[i] <= in[i] ? POISON : in[i];
}

/* scantst.c: MPI_Scan of the ranks, twice with MPI_SUM, twice with the user sum, once with the
 * order-checking non-commutative function */
static int t_scantst(void) {
    int errs = 0, rc;
    const int want = g_rank * (g_rank + 1) / 2;
    MPI_Op add, ordered;
    errs += MPI_Op_create(uf_add, 1, &add) != MPI_SUCCESS;
    errs += MPI_Op_create(uf_ordered, 0, &ordered) != MPI_SUCCESS;
    for (int rep = 0; rep < 2; ++rep) {
        errs += scan1(0, g_rank, -100, MPI_SUM, &rc) != want;
        errs += rc != MPI_SUCCESS;
    }
    for (int rep = 0; rep < 2; ++rep) {
        errs += scan1(0, g_rank, -100, add, &rc) != want;
        errs += rc != MPI_SUCCESS;
    }
    errs += scan1(0, g_rank, -100, ordered, &rc) == POISON;
    errs += rc != MPI_SUCCESS;
    MPI_Op_free(&add);
    MPI_Op_free(&ordered);
    return errs;
}

/* exscan.c: MPI_SUM over MPI_INT of sendbuf[i] = rank + i * size for counts 1, 2, 4 .. 32768;
 * rank r > 0 expects r * i * size + r (r - 1) / 2, rank 0 nothing; then the same with
 * MPI_IN_PLACE, where rank 0's operand must come back unchanged */
static int t_exscan(void) {
    int errs = 0;
    const int r = g_rank, n = g_size;
    for (int count = 1; count < 65000; count *= 2) {
        const size_t bytes = (size_t)count * sizeof(int);
        int *h = malloc(bytes), *g = malloc(bytes);
        int *s = buf_new(bytes), *d = buf_new(bytes);
        for (int i = 0; i < count; ++i) h[i] = r + i * n, g[i] = -1;
        buf_set(s, h, bytes);
        buf_set(d, g, bytes);
        errs += MPI_Exscan(s, d, count, MPI_INT, MPI_SUM, MPI_COMM_WORLD) != MPI_SUCCESS;
        buf_read(g, d, bytes);
        if (r > 0)
            for (int i = 0; i < count; ++i) errs += g[i] != r * i * n + r * (r - 1) / 2;
        buf_set(d, h, bytes);
        errs += MPI_Exscan(MPI_IN_PLACE, d, count, MPI_INT, MPI_SUM, MPI_COMM_WORLD) != MPI_SUCCESS;
        buf_read(g, d, bytes);
        for (int i = 0; i < count; ++i) errs += g[i] != (r == 0 ? h[i] : r * i * n + r * (r - 1) / 2);
        buf_del(s);
        buf_del(d);
        free(h);
        free(g);
    }
    return errs;
}

/* exscan2.c: one int per rank; rank r > 0 expects r (r - 1) / 2, rank 0 keeps its -2 */
static int t_exscan2(void) {
    int rc;
    const int got = scan1(1, g_rank, -2, MPI_SUM, &rc);
    return (rc != MPI_SUCCESS) + (got != (g_rank ? g_rank * (g_rank - 1) / 2 : -2));
}

static const struct {
    const char *name;
    int (*fn)(void);
} kCases[] = {{"scantst", t_scantst}, {"exscan", t_exscan}, {"exscan2", t_exscan2}};

int main(int argc, char **argv) {
    MPI_Init(&argc, &argv);
    MPI_Comm_rank(MPI_COMM_WORLD, &g_rank);
    MPI_Comm_size(MPI_COMM_WORLD, &g_size);
    if (argc < 2 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) {
        if (!g_rank) fprintf(stderr, "usage: scan_suite {host|device} [case ...]\n");
        MPI_Finalize();
        return 2;
    }
    g_dev = !strcmp(argv[1], "device");
    MPI_Comm_set_errhandler(MPI_COMM_WORLD, MPI_ERRORS_RETURN);
    int total = 0;
    for (size_t c = 0; c < sizeof(kCases) / sizeof(kCases[0]); ++c) {
        int wanted = argc <= 2;
        for (int a = 2; a < argc; ++a) wanted |= !strcmp(argv[a], kCases[c].name);
        if (!wanted) continue;
        int mine = kCases[c].fn(), all = 0;
        MPI_Allreduce(&mine, &all, 1, MPI_INT, MPI_SUM, MPI_COMM_WORLD);
        if (!g_rank) printf("%s %s %d\n", argv[1], kCases[c].name, all);
        total += all;
    }
    if (!g_rank) printf("%s TOTAL %d\n", argv[1], total);
    MPI_Finalize();
    return total ? 1 : 0;
}

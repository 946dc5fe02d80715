/* alltoallw_suite.c — the properties the reference's MPI_Alltoallw tests check (MPICH test/mpi/coll
 * alltoallw1.c, alltoallw2.c, alltoallw_zeros.c), written anew as one self-checking C program that
 * links the drop-in libmpi.so like any MPI application.  Buffers live in host memory (`host`) or
 * in device memory (`device`: hipMalloc).
 *
 *   usage: mv2run -n N alltoallw_suite {host|device} [case ...]
 *
 * Rank 0 prints one line per case ("<mem> <case> <errors>") and a TOTAL line; the exit status is
 * non-zero when any rank counted an error. */
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

#define UNTOUCHED (-77)

/* first row / column and their number of rank r's share of `total`, the last share ragged or empty */
static void share(int total, int r, int *first, int *len) {
    const int b = (total + g_size - 1) / g_size;
    *first = r * b < total ? r * b : total;
    *len = total - *first < b ? total - *first : b;
}

/* alltoallw1.c's property: a matrix distributed by blocks of rows is transposed with one
 * MPI_Alltoallw.  Rank r sends rank j the columns j owns of its rows, walking each column (a vector
 * resized to one element, so that the count steps from column to column), and receives from rank
 * r a corner of its rows of the transpose (a vector of whole sub-rows), one type per peer.  The
 * matrix is ROWS x COLS doubles; neither divides by 4 ranks evenly. */
static int t_alltoallw1(void) {
    enum { ROWS = 22, COLS = 37 };
    int errs = 0;
    const int n = g_size, me = g_rank;
    int r0, nr, c0, nc; /* my rows of the matrix, my rows of the transpose */
    share(ROWS, me, &r0, &nr);
    share(COLS, me, &c0, &nc);
    int *sc = calloc(n, sizeof(int)), *sd = calloc(n, sizeof(int)), *rc = calloc(n, sizeof(int)), *rd = calloc(n, sizeof(int));
    MPI_Datatype *st = malloc(n * sizeof(MPI_Datatype)), *rt = malloc(n * sizeof(MPI_Datatype)), col = MPI_DATATYPE_NULL;
    if (nr) {
        MPI_Datatype v;
        MPI_Type_vector(nr, 1, COLS, MPI_DOUBLE, &v);
        MPI_Type_create_resized(v, 0, sizeof(double), &col);
        MPI_Type_commit(&col);
        MPI_Type_free(&v);
    }
    for (int j = 0; j < n; ++j) {
        int f, l;
        share(COLS, j, &f, &l); /* rank j's columns of my rows */
        st[j] = nr && l ? col : MPI_DOUBLE;
        sc[j] = nr ? l : 0;
        sd[j] = sc[j] ? f * (int)sizeof(double) : 0;
        share(ROWS, j, &f, &l); /* rank j's rows are columns [f, f + l) of my rows of the transpose */
        rt[j] = MPI_DOUBLE;
        rc[j] = 0;
        rd[j] = 0;
        if (nc && l) {
            MPI_Type_vector(nc, l, ROWS, MPI_DOUBLE, &rt[j]);
            MPI_Type_commit(&rt[j]);
            rc[j] = 1;
            rd[j] = f * (int)sizeof(double);
        }
    }
    const size_t ns = (size_t)nr * COLS + 1, nd = (size_t)nc * ROWS + 1;
    double *hs = malloc(ns * sizeof(double)), *hr = malloc(nd * sizeof(double));
    for (int i = 0; i < nr; ++i)
        for (int c = 0; c < COLS; ++c) hs[(size_t)i * COLS + c] = (r0 + i) * 1000.0 + c;
    for (size_t i = 0; i < nd; ++i) hr[i] = UNTOUCHED;
    double *s = buf_new(ns * sizeof(double)), *r = buf_new(nd * sizeof(double));
    buf_set(s, hs, ns * sizeof(double));
    buf_set(r, hr, nd * sizeof(double));
    if (MPI_Alltoallw(s, sc, sd, st, r, rc, rd, rt, MPI_COMM_WORLD) != MPI_SUCCESS) ++errs;
    buf_read(hr, r, nd * sizeof(double));
    for (int c = 0; c < nc; ++c)
        for (int i = 0; i < ROWS; ++i)
            if (hr[(size_t)c * ROWS + i] != i * 1000.0 + (c0 + c) && errs++ < 5)
                fprintf(stderr, "[%d] alltoallw1: transpose (%d, %d) is %g\n", me, c0 + c, i, hr[(size_t)c * ROWS + i]);
    if (hr[nd - 1] != UNTOUCHED) ++errs;
    for (int j = 0; j < n; ++j)
        if (rc[j]) MPI_Type_free(&rt[j]);
    if (nr) MPI_Type_free(&col);
    buf_del(s);
    buf_del(r);
    free(hs), free(hr), free(sc), free(sd), free(rc), free(rd), free(st), free(rt);
    return errs;
}

/* the k-th int rank `from` sends rank `to` */
static int val(int from, int to, int k) { return from * 1000003 + to * 1009 + k; }

/* alltoallw2.c's property: everyone sends rank i exactly i ints at byte displacements (so rank 0
 * receives nothing and rank me receives me ints from everyone), with space between the receive
 * blocks that must stay untouched; then the exchange in place, where the pair (i, j) carries
 * (i + j) % 3 + 1 ints either way.  The odd peers' blocks are strided types, so both the staged and
 * the plain side are met. */
static int t_alltoallw2(void) {
    int errs = 0;
    const int n = g_size, me = g_rank;
    int *sc = calloc(n, sizeof(int)), *sd = calloc(n, sizeof(int)), *rc = calloc(n, sizeof(int)), *rd = calloc(n, sizeof(int));
    MPI_Datatype *st = malloc(n * sizeof(MPI_Datatype)), *rt = malloc(n * sizeof(MPI_Datatype));
    for (int pass = 0; pass < 2; ++pass) { /* 0: MPI_INT everywhere; 1: every second int towards odd peers */
        int ns = 0;
        for (int j = 0; j < n; ++j) {
            const int strided = pass && (j & 1) && j > 1;
            st[j] = MPI_INT;
            sc[j] = j;
            sd[j] = ns * (int)sizeof(int);
            if (strided) {
                MPI_Type_vector(j, 1, 2, MPI_INT, &st[j]);
                MPI_Type_commit(&st[j]);
                sc[j] = 1;
            }
            ns += strided ? 2 * j : j;
            rt[j] = MPI_INT;
            rc[j] = me;
            rd[j] = j * (me + 2) * (int)sizeof(int); /* two ints of space behind every block */
        }
        const int nr = n * (me + 2);
        int *hs = calloc(ns + 1, sizeof(int)), *hr = calloc(nr + 1, sizeof(int));
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < j; ++k) hs[sd[j] / (int)sizeof(int) + (st[j] != MPI_INT ? 2 * k : k)] = val(me, j, k);
        for (int i = 0; i < nr; ++i) hr[i] = UNTOUCHED;
        int *s = buf_new((size_t)(ns + 1) * sizeof(int)), *r = buf_new((size_t)(nr + 1) * sizeof(int));
        buf_set(s, hs, (size_t)(ns + 1) * sizeof(int));
        buf_set(r, hr, (size_t)(nr + 1) * sizeof(int));
        if (MPI_Alltoallw(s, sc, sd, st, r, rc, rd, rt, MPI_COMM_WORLD) != MPI_SUCCESS) ++errs;
        buf_read(hr, r, (size_t)(nr + 1) * sizeof(int));
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < me + 2; ++k) {
                const int want = k < me ? val(j, me, k) : UNTOUCHED, got = hr[j * (me + 2) + k];
                if (got != want && errs++ < 5)
                    fprintf(stderr, "[%d] alltoallw2 pass %d: block %d element %d is %d, not %d\n", me, pass, j, k, got, want);
            }
        for (int j = 0; j < n; ++j)
            if (st[j] != MPI_INT) MPI_Type_free(&st[j]);
        buf_del(s);
        buf_del(r);
        free(hs);
        free(hr);
    }
    /* in place; pass 1 receives every second int (a strided type per peer) */
    for (int pass = 0; pass < 2; ++pass) {
        int tot = 0;
        for (int j = 0; j < n; ++j) {
            const int c = (me + j) % 3 + 1;
            rt[j] = MPI_INT;
            rc[j] = c;
            if (pass) {
                MPI_Type_vector(c, 1, 2, MPI_INT, &rt[j]);
                MPI_Type_commit(&rt[j]);
                rc[j] = 1;
            }
            rd[j] = tot * (int)sizeof(int);
            tot += (pass ? 2 * c : c) + 1;
        }
        int *hr = malloc((size_t)(tot + 1) * sizeof(int));
        for (int i = 0; i <= tot; ++i) hr[i] = UNTOUCHED;
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < (me + j) % 3 + 1; ++k) hr[rd[j] / (int)sizeof(int) + (pass ? 2 * k : k)] = val(me, j, k);
        int *r = buf_new((size_t)(tot + 1) * sizeof(int));
        buf_set(r, hr, (size_t)(tot + 1) * sizeof(int));
        if (MPI_Alltoallw(MPI_IN_PLACE, NULL, NULL, NULL, r, rc, rd, rt, MPI_COMM_WORLD) != MPI_SUCCESS) ++errs;
        buf_read(hr, r, (size_t)(tot + 1) * sizeof(int));
        for (int j = 0; j < n; ++j) {
            const int c = (me + j) % 3 + 1, at = rd[j] / (int)sizeof(int);
            for (int k = 0; k < (pass ? 2 * c : c) + 1; ++k) {
                const int data = pass ? (k % 2 == 0 && k / 2 < c) : k < c;
                const int want = data ? val(j, me, pass ? k / 2 : k) : UNTOUCHED;
                if (hr[at + k] != want && errs++ < 5)
                    fprintf(stderr, "[%d] alltoallw2 in place %d: block %d int %d is %d, not %d\n", me, pass, j, k, hr[at + k], want);
            }
        }
        for (int j = 0; j < n; ++j)
            if (pass) MPI_Type_free(&rt[j]);
        buf_del(r);
        free(hr);
    }
    free(sc), free(sd), free(rc), free(rd), free(st), free(rt);
    return errs;
}

/* alltoallw_zeros.c's property: a count of zero of a type that has a size matches a non-zero count
 * of a type of size zero, both ways round, for MPI_Alltoallw and MPI_Alltoallv; in place, the odd
 * and the even ranks pass signatures that differ and still match.  No byte may move. */
static int t_alltoallw_zeros(void) {
    int errs = 0;
    const int n = g_size;
    int *ones = malloc(n * sizeof(int)), *zeros = calloc(n, sizeof(int)), *dz = calloc(n, sizeof(int));
    MPI_Datatype *empties = malloc(n * sizeof(MPI_Datatype)), *intsT = malloc(n * sizeof(MPI_Datatype)), empty;
    MPI_Type_contiguous(0, MPI_INT, &empty);
    MPI_Type_commit(&empty);
    for (int j = 0; j < n; ++j) ones[j] = 1, empties[j] = empty, intsT[j] = MPI_INT;
    int hs = 41, hr = UNTOUCHED;
    int *s = buf_new(sizeof(int)), *r = buf_new(sizeof(int));
    buf_set(s, &hs, sizeof(int));
    buf_set(r, &hr, sizeof(int));
    errs += MPI_Alltoallw(s, ones, dz, empties, r, zeros, dz, intsT, MPI_COMM_WORLD) != MPI_SUCCESS;
    errs += MPI_Alltoallw(s, zeros, dz, intsT, r, ones, dz, empties, MPI_COMM_WORLD) != MPI_SUCCESS;
    if (g_rank % 2) errs += MPI_Alltoallw(MPI_IN_PLACE, NULL, NULL, NULL, r, zeros, dz, intsT, MPI_COMM_WORLD) != MPI_SUCCESS;
    else errs += MPI_Alltoallw(MPI_IN_PLACE, NULL, NULL, NULL, r, ones, dz, empties, MPI_COMM_WORLD) != MPI_SUCCESS;
    errs += MPI_Alltoallv(s, ones, dz, empty, r, zeros, dz, MPI_INT, MPI_COMM_WORLD) != MPI_SUCCESS;
    errs += MPI_Alltoallv(s, zeros, dz, MPI_INT, r, ones, dz, empty, MPI_COMM_WORLD) != MPI_SUCCESS;
    if (g_rank % 2) errs += MPI_Alltoallv(MPI_IN_PLACE, NULL, NULL, MPI_DATATYPE_NULL, r, zeros, dz, MPI_INT, MPI_COMM_WORLD) != MPI_SUCCESS;
    else errs += MPI_Alltoallv(MPI_IN_PLACE, NULL, NULL, MPI_DATATYPE_NULL, r, ones, dz, empty, MPI_COMM_WORLD) != MPI_SUCCESS;
    buf_read(&hs, s, sizeof(int));
    buf_read(&hr, r, sizeof(int));
    if (hs != 41 || hr != UNTOUCHED) ++errs;
    MPI_Type_free(&empty);
    buf_del(s);
    buf_del(r);
    free(ones), free(zeros), free(dz), free(empties), free(intsT);
    return errs;
}

static const struct {
    const char *name;
    int (*fn)(void);
} kCases[] = {
    {"alltoallw1", t_alltoallw1},
    {"alltoallw2", t_alltoallw2},
    {"alltoallw_zeros", t_alltoallw_zeros},
};

int main(int argc, char **argv) {
    if (argc < 2 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) {
        fprintf(stderr, "usage: alltoallw_suite {host|device} [case ...]\n");
        return 2;
    }
    g_dev = !strcmp(argv[1], "device");
    MPI_Init(&argc, &argv);
    MPI_Comm_set_errhandler(MPI_COMM_WORLD, MPI_ERRORS_RETURN);
    MPI_Comm_rank(MPI_COMM_WORLD, &g_rank);
    MPI_Comm_size(MPI_COMM_WORLD, &g_size);
    int total = 0;
    for (size_t i = 0; i < sizeof(kCases) / sizeof(kCases[0]); ++i) {
        int wanted = argc == 2;
        for (int a = 2; a < argc; ++a) wanted |= !strcmp(argv[a], kCases[i].name);
        if (!wanted) continue;
        int errs = kCases[i].fn(), all = 0;
        MPI_Allreduce(&errs, &all, 1, MPI_INT, MPI_SUM, MPI_COMM_WORLD);
        if (g_rank == 0) printf("%s %s %d\n", argv[1], kCases[i].name, all);
        total += all;
    }
    if (g_rank == 0) printf("%s TOTAL %d\n", argv[1], total);
    MPI_Finalize();
    return total ? 1 : 0;
}

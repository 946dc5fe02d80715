/* gather_suite.c — the properties the reference's gather / scatter / allgatherv tests check (MPICH
 * test/mpi/coll gather.c, gather2.c, scatter2.c, scatter3.c, scattern.c, scatterv.c, allgatherv2.c,
 * allgatherv3.c and the gather / scatter members of coll2.c - coll6.c), written anew as one
 * self-checking C program that links the drop-in libmpi.so like any MPI application.  Buffers live
 * in host memory (`host`) or in device memory (`device`: hipMalloc).
 *
 *   usage: mv2run -n N gather_suite {host|device} [case ...]
 *
 * Rank 0 prints one line per case ("<mem> <case> <errors>") and a TOTAL line; the exit status is
 * non-zero when any rank counted an error.  Every check is the test's own closed form. */
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
/* an operand buffer holding the host image h */
static void *buf_of(const void *h, size_t bytes) {
    void *b = buf_new(bytes);
    buf_set(b, h, bytes);
    return b;
}

#define STRIDE 10
#define COMPLAIN(...) \
    do { \
        if (errs++ < 5) fprintf(stderr, __VA_ARGS__); \
    } while (0)

/* gather.c (inplace = 0) and gather2.c (inplace = 1): every rank sends n doubles, every STRIDE-th
 * of its buffer through a vector type, to every root in turn for n = 1, 2, 4 ... 32768; the root
 * receives them contiguously and element i of the result is i.  In place the root's own block is
 * already there and its send arguments mean nothing; elsewhere the receive arguments mean nothing. */
static int gather_vec(int inplace) {
    int errs = 0;
    const int size = g_size, rank = g_rank;
    for (int root = 0; root < size; ++root) {
        for (int n = 1; n < 65000; n *= 2) {
            double *hin = malloc((size_t)n * STRIDE * sizeof(double)), *hout = malloc((size_t)size * n * sizeof(double));
            MPI_Datatype vec;
            MPI_Type_vector(n, 1, STRIDE, MPI_DOUBLE, &vec);
            MPI_Type_commit(&vec);
            for (int i = 0; i < n * STRIDE; ++i) hin[i] = -2;
            for (int i = 0; i < n; ++i) hin[i * STRIDE] = rank * n + i;
            for (int i = 0; i < size * n; ++i) hout[i] = -1;
            if (inplace && rank == root)
                for (int i = 0; i < n; ++i) hout[rank * n + i] = rank * n + i;
            double *in = buf_of(hin, (size_t)n * STRIDE * sizeof(double)), *out = buf_of(hout, (size_t)size * n * sizeof(double));
            int e;
            if (!inplace) e = MPI_Gather(in, 1, vec, out, n, MPI_DOUBLE, root, MPI_COMM_WORLD);
            else if (rank == root) e = MPI_Gather(MPI_IN_PLACE, -1, MPI_DATATYPE_NULL, out, n, MPI_DOUBLE, root, MPI_COMM_WORLD);
            else e = MPI_Gather(in, 1, vec, NULL, -1, MPI_DATATYPE_NULL, root, MPI_COMM_WORLD);
            if (e != MPI_SUCCESS) COMPLAIN("[%d] gather n=%d root %d: rc %d\n", rank, n, root, e);
            buf_read(hout, out, (size_t)size * n * sizeof(double));
            for (int i = 0; i < n * size; ++i) {
                const double want = rank == root ? i : -1;
                if (hout[i] != want) COMPLAIN("[%d] gather n=%d root %d: element %d is %g\n", rank, n, root, i, hout[i]);
            }
            buf_del(in);
            buf_del(out);
            free(hin);
            free(hout);
            MPI_Type_free(&vec);
        }
    }
    /* zero-size gathers */
    int e = MPI_Gather(NULL, 0, MPI_BYTE, NULL, 0, MPI_BYTE, 0, MPI_COMM_WORLD);
    if (e != MPI_SUCCESS) COMPLAIN("[%d] zero-size gather: rc %d\n", rank, e);
    if (inplace) {
        if (rank == 0) e = MPI_Gather(MPI_IN_PLACE, -1, MPI_DATATYPE_NULL, NULL, 0, MPI_BYTE, 0, MPI_COMM_WORLD);
        else e = MPI_Gather(NULL, 0, MPI_BYTE, NULL, 0, MPI_BYTE, 0, MPI_COMM_WORLD);
        if (e != MPI_SUCCESS) COMPLAIN("[%d] zero-size gather in place: rc %d\n", rank, e);
    }
    return errs;
}
static int t_gather(void) { return gather_vec(0); }
static int t_gather2(void) { return gather_vec(1); }

/* scatter2.c (inplace = 1, n = 1000) and scattern.c (inplace = 0, several n): every root in turn
 * scatters one vector of n doubles, STRIDE apart, per rank out of a buffer whose element i is i;
 * blocks follow at the vector's extent, (n - 1) * STRIDE + 1 doubles, so rank r's k-th double is
 * r * ((n - 1) * STRIDE + 1) + k * STRIDE.  In place the root receives nothing. */
static int scatter_vec(int n, int inplace) {
    int errs = 0;
    const int size = g_size, rank = g_rank;
    const size_t nin = (size_t)n * STRIDE * size;
    double *hin = malloc(nin * sizeof(double)), *hout = malloc((size_t)n * sizeof(double));
    MPI_Datatype vec;
    MPI_Aint lb, ext;
    MPI_Type_vector(n, 1, STRIDE, MPI_DOUBLE, &vec);
    MPI_Type_commit(&vec);
    MPI_Type_get_extent(vec, &lb, &ext);
    if (ext != (MPI_Aint)(((size_t)(n - 1) * STRIDE + 1) * sizeof(double))) COMPLAIN("[%d] vector extent %ld\n", rank, (long)ext);
    for (size_t i = 0; i < nin; ++i) hin[i] = (double)i;
    double *in = buf_of(hin, nin * sizeof(double)), *out = buf_new((size_t)n * sizeof(double));
    for (int root = 0; root < size; ++root) {
        for (int i = 0; i < n; ++i) hout[i] = -1;
        buf_set(out, hout, (size_t)n * sizeof(double));
        int e;
        if (inplace && rank == root) e = MPI_Scatter(in, 1, vec, MPI_IN_PLACE, -1, MPI_DATATYPE_NULL, root, MPI_COMM_WORLD);
        else if (inplace) e = MPI_Scatter(NULL, -1, MPI_DATATYPE_NULL, out, n, MPI_DOUBLE, root, MPI_COMM_WORLD);
        else e = MPI_Scatter(in, 1, vec, out, n, MPI_DOUBLE, root, MPI_COMM_WORLD);
        if (e != MPI_SUCCESS) COMPLAIN("[%d] scatter n=%d root %d: rc %d\n", rank, n, root, e);
        buf_read(hout, out, (size_t)n * sizeof(double));
        double want = (double)rank * ((n - 1) * STRIDE + 1);
        for (int i = 0; i < n; ++i, want += STRIDE) {
            const double w = inplace && rank == root ? -1 : want;
            if (hout[i] != w) COMPLAIN("[%d] scatter n=%d root %d: element %d is %g, not %g\n", rank, n, root, i, hout[i], w);
        }
    }
    buf_del(in);
    buf_del(out);
    free(hin);
    free(hout);
    MPI_Type_free(&vec);
    return errs;
}
static int t_scatter2(void) { return scatter_vec(1000, 1); }
static int t_scattern(void) { return scatter_vec(1, 0) + scatter_vec(3, 0) + scatter_vec(1000, 0) + scatter_vec(20011, 0); }

/* scatter3.c: the vector type is on the receiving side, and on the root only -- the root receives
 * its n doubles STRIDE apart (what lies between stays), every other rank contiguously */
static int t_scatter3(void) {
    int errs = 0;
    const int size = g_size, rank = g_rank, n = 1000;
    double *hin = malloc((size_t)n * size * sizeof(double)), *hout = malloc((size_t)n * STRIDE * sizeof(double));
    MPI_Datatype vec;
    MPI_Type_vector(n, 1, STRIDE, MPI_DOUBLE, &vec);
    MPI_Type_commit(&vec);
    for (int i = 0; i < n * size; ++i) hin[i] = i;
    double *in = buf_of(hin, (size_t)n * size * sizeof(double)), *out = buf_new((size_t)n * STRIDE * sizeof(double));
    for (int root = 0; root < size; ++root) {
        for (int i = 0; i < n * STRIDE; ++i) hout[i] = -1;
        buf_set(out, hout, (size_t)n * STRIDE * sizeof(double));
        int e;
        if (rank == root) e = MPI_Scatter(in, n, MPI_DOUBLE, out, 1, vec, root, MPI_COMM_WORLD);
        else e = MPI_Scatter(NULL, -1, MPI_DATATYPE_NULL, out, n, MPI_DOUBLE, root, MPI_COMM_WORLD);
        if (e != MPI_SUCCESS) COMPLAIN("[%d] scatter3 root %d: rc %d\n", rank, root, e);
        buf_read(hout, out, (size_t)n * STRIDE * sizeof(double));
        for (int i = 0; i < n * STRIDE; ++i) {
            double want = -1;
            if (rank == root && i % STRIDE == 0 && i / STRIDE < n) want = n * rank + i / STRIDE;
            if (rank != root && i < n) want = n * rank + i;
            if (hout[i] != want) COMPLAIN("[%d] scatter3 root %d: element %d is %g, not %g\n", rank, root, i, hout[i], want);
        }
    }
    buf_del(in);
    buf_del(out);
    free(hin);
    free(hout);
    MPI_Type_free(&vec);
    return errs;
}

/* scatterv.c: a matrix in column-major order, (nx * nrow) x (ny * ncol) doubles over an nrow x
 * ncol grid of ranks, leaves rank 0 as one nx x ny tile per rank: the send type is a vector of ny
 * runs of nx doubles resized to nx doubles, so the tiles' type maps interleave and a displacement
 * counts tiles' widths.  Tile (row, col) holds 1000 * col + 100 * row + m * nx + k.  Then the
 * same with MPI_IN_PLACE at the root, whose receive buffer keeps its -1. */
static int t_scatterv(void) {
    int errs = 0;
    const int size = g_size, rank = g_rank, nx = 10, ny = 8;
    int nrow = 1;
    for (int d = 1; d * d <= size; ++d)
        if (size % d == 0) nrow = d;
    const int ncol = size / nrow, myrow = rank % nrow, mycol = rank / nrow, coldim = nx * nrow;
    const size_t nsend = (size_t)nx * ny * size;
    double *hs = malloc(nsend * sizeof(double)), *hr = malloc((size_t)nx * ny * sizeof(double));
    int *sc = malloc(size * sizeof(int)), *sd = malloc(size * sizeof(int));
    for (int j = 0; j < ncol; ++j)
        for (int i = 0; i < nrow; ++i) {
            double *p = hs + i * nx + (size_t)j * ny * coldim;
            for (int m = 0; m < ny; ++m, p += coldim)
                for (int k = 0; k < nx; ++k) p[k] = 1000 * j + 100 * i + m * nx + k;
            sc[i + j * nrow] = 1;
            sd[i + j * nrow] = i + j * (nrow * ny);
        }
    MPI_Datatype vec, block;
    MPI_Type_vector(ny, nx, coldim, MPI_DOUBLE, &vec);
    MPI_Type_create_resized(vec, 0, nx * (MPI_Aint)sizeof(double), &block);
    MPI_Type_free(&vec);
    MPI_Type_commit(&block);
    double *s = rank == 0 ? buf_of(hs, nsend * sizeof(double)) : NULL, *r = buf_new((size_t)nx * ny * sizeof(double));
    for (int pass = 0; pass < 2; ++pass) { /* 1: MPI_IN_PLACE at the root */
        for (int i = 0; i < nx * ny; ++i) hr[i] = -1;
        buf_set(r, hr, (size_t)nx * ny * sizeof(double));
        int e;
        if (pass && rank == 0) e = MPI_Scatterv(s, sc, sd, block, MPI_IN_PLACE, -1, MPI_DATATYPE_NULL, 0, MPI_COMM_WORLD);
        else e = MPI_Scatterv(s, sc, sd, block, r, nx * ny, MPI_DOUBLE, 0, MPI_COMM_WORLD);
        if (e != MPI_SUCCESS) COMPLAIN("[%d] scatterv pass %d: rc %d\n", rank, pass, e);
        buf_read(hr, r, (size_t)nx * ny * sizeof(double));
        for (int m = 0; m < ny; ++m)
            for (int k = 0; k < nx; ++k) {
                const double want = pass && rank == 0 ? -1 : 1000 * mycol + 100 * myrow + m * nx + k;
                if (hr[m * nx + k] != want)
                    COMPLAIN("[%d] scatterv pass %d: (%d,%d) is %g, not %g\n", rank, pass, m, k, hr[m * nx + k], want);
            }
    }
    if (s) buf_del(s);
    buf_del(r);
    MPI_Type_free(&block);
    free(hs);
    free(hr);
    free(sc);
    free(sd);
    return errs;
}

/* allgatherv2.c (inplace = 1) and allgatherv3.c (inplace = 0): count doubles per rank for count =
 * 1, 2, 4 ... 8192, block i at i * count; element i of the result is i */
static int allgatherv_uniform(int inplace) {
    int errs = 0;
    const int size = g_size, rank = g_rank;
    int *rc = malloc(size * sizeof(int)), *dp = malloc(size * sizeof(int));
    for (int count = 1; count < 9000; count *= 2) {
        double *hin = malloc((size_t)count * sizeof(double)), *hout = malloc((size_t)size * count * sizeof(double));
        for (int i = 0; i < size * count; ++i) hout[i] = -1;
        for (int i = 0; i < count; ++i) {
            hin[i] = rank * count + i;
            if (inplace) hout[rank * count + i] = rank * count + i;
        }
        for (int i = 0; i < size; ++i) rc[i] = count, dp[i] = i * count;
        double *in = buf_of(hin, (size_t)count * sizeof(double)), *out = buf_of(hout, (size_t)size * count * sizeof(double));
        const int e = inplace ? MPI_Allgatherv(MPI_IN_PLACE, -1, MPI_DATATYPE_NULL, out, rc, dp, MPI_DOUBLE, MPI_COMM_WORLD)
                              : MPI_Allgatherv(in, count, MPI_DOUBLE, out, rc, dp, MPI_DOUBLE, MPI_COMM_WORLD);
        if (e != MPI_SUCCESS) COMPLAIN("[%d] allgatherv count=%d: rc %d\n", rank, count, e);
        buf_read(hout, out, (size_t)size * count * sizeof(double));
        for (int i = 0; i < count * size; ++i)
            if (hout[i] != i) COMPLAIN("[%d] allgatherv count=%d: element %d is %g\n", rank, count, i, hout[i]);
        buf_del(in);
        buf_del(out);
        free(hin);
        free(hout);
    }
    free(rc);
    free(dp);
    return errs;
}
static int t_allgatherv2(void) { return allgatherv_uniform(1); }
static int t_allgatherv3(void) { return allgatherv_uniform(0); }

/* coll2.c - coll6.c: a table of ROWS x COLS ints whose rows are dealt to the ranks in blocks.
 * ROWS is a multiple of every job size the suite runs at, so every rank owns ROWS / size rows. */
#define ROWS 120
#define COLS 10

/* which: 2 MPI_Gather (coll2.c), 3 MPI_Gatherv (coll3.c) to every root in turn, the root in place;
 * 6 MPI_Allgatherv (coll6.c), in place where the block is already its own.  Every rank fills its
 * rows with rank + 10; afterwards row i holds i / block + 10 on every rank that received. */
static int table_gather(int which) {
    int errs = 0;
    const int size = g_size, rank = g_rank, block = ROWS / size, cnt = block * COLS;
    int *ht = malloc(ROWS * COLS * sizeof(int)), *rc = malloc(size * sizeof(int)), *dp = malloc(size * sizeof(int));
    for (int i = 0; i < size; ++i) rc[i] = cnt, dp[i] = i * cnt;
    for (int i = 0; i < ROWS * COLS; ++i) ht[i] = 0;
    for (int i = rank * cnt; i < (rank + 1) * cnt; ++i) ht[i] = rank + 10;
    int *t = buf_of(ht, ROWS * COLS * sizeof(int));
    int e = MPI_SUCCESS;
    if (which == 6) {
        e = MPI_Allgatherv(MPI_IN_PLACE, cnt, MPI_INT, t, rc, dp, MPI_INT, MPI_COMM_WORLD);
    } else {
        for (int root = 0; root < size && e == MPI_SUCCESS; ++root) {
            const void *sb = root == rank ? MPI_IN_PLACE : (const void *)(t + rank * cnt);
            e = which == 2 ? MPI_Gather(sb, cnt, MPI_INT, t, cnt, MPI_INT, root, MPI_COMM_WORLD)
                           : MPI_Gatherv(sb, cnt, MPI_INT, t, rc, dp, MPI_INT, root, MPI_COMM_WORLD);
        }
    }
    if (e != MPI_SUCCESS) COMPLAIN("[%d] coll%d: rc %d\n", rank, which, e);
    buf_read(ht, t, ROWS * COLS * sizeof(int));
    for (int i = 0; i < ROWS; ++i)
        for (int j = 0; j < COLS; ++j)
            if (ht[i * COLS + j] != i / block + 10) COMPLAIN("[%d] coll%d: table[%d][%d] is %d\n", rank, which, i, j, ht[i * COLS + j]);
    buf_del(t);
    free(ht);
    free(rc);
    free(dp);
    return errs;
}
static int t_coll2(void) { return table_gather(2); }
static int t_coll3(void) { return table_gather(3); }
static int t_coll6(void) { return table_gather(6); }

/* which: 4 MPI_Scatter (coll4.c), 5 MPI_Scatterv (coll5.c): rank 0 fills table[i][j] = i + j for
 * the first `size` rows and deals one row to every rank; rank r's row is r, r + 1, ... */
static int table_scatter(int which) {
    int errs = 0;
    const int size = g_size, rank = g_rank;
    int *ht = calloc((size_t)size * COLS, sizeof(int)), hrow[COLS], *sc = malloc(size * sizeof(int)), *dp = malloc(size * sizeof(int));
    for (int i = 0; i < size; ++i) {
        sc[i] = COLS, dp[i] = i * COLS;
        for (int j = 0; j < COLS; ++j) ht[i * COLS + j] = rank == 0 ? i + j : -3;
    }
    for (int j = 0; j < COLS; ++j) hrow[j] = -1;
    int *t = buf_of(ht, (size_t)size * COLS * sizeof(int)), *row = buf_of(hrow, sizeof(hrow));
    const int e = which == 4 ? MPI_Scatter(t, COLS, MPI_INT, row, COLS, MPI_INT, 0, MPI_COMM_WORLD)
                             : MPI_Scatterv(t, sc, dp, MPI_INT, row, COLS, MPI_INT, 0, MPI_COMM_WORLD);
    if (e != MPI_SUCCESS) COMPLAIN("[%d] coll%d: rc %d\n", rank, which, e);
    buf_read(hrow, row, sizeof(hrow));
    for (int j = 0; j < COLS; ++j)
        if (hrow[j] != j + rank) COMPLAIN("[%d] coll%d: row[%d] is %d\n", rank, which, j, hrow[j]);
    buf_del(t);
    buf_del(row);
    free(ht);
    free(sc);
    free(dp);
    return errs;
}
static int t_coll4(void) { return table_scatter(4); }
static int t_coll5(void) { return table_scatter(5); }

static const struct {
    const char *name;
    int (*fn)(void);
} kCases[] = {
    {"gather", t_gather},
    {"gather2", t_gather2},
    {"scatter2", t_scatter2},
    {"scatter3", t_scatter3},
    {"scattern", t_scattern},
    {"scatterv", t_scatterv},
    {"allgatherv2", t_allgatherv2},
    {"allgatherv3", t_allgatherv3},
    {"coll2", t_coll2},
    {"coll3", t_coll3},
    {"coll4", t_coll4},
    {"coll5", t_coll5},
    {"coll6", t_coll6},
};

int main(int argc, char **argv) {
    if (argc < 2 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) {
        fprintf(stderr, "usage: gather_suite {host|device} [case ...]\n");
        return 2;
    }
    g_dev = !strcmp(argv[1], "device");
    MPI_Init(&argc, &argv);
    MPI_Comm_set_errhandler(MPI_COMM_WORLD, MPI_ERRORS_RETURN);
    MPI_Comm_rank(MPI_COMM_WORLD, &g_rank);
    MPI_Comm_size(MPI_COMM_WORLD, &g_size);
    if (ROWS % g_size) {
        if (g_rank == 0) fprintf(stderr, "the job size must divide %d\n", ROWS);
        MPI_Finalize();
        return 2;
    }
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

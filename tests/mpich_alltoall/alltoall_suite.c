/* alltoall_suite.c — the properties the reference's all-to-all tests check (MPICH test/mpi/coll
 * alltoall1.c, alltoallv.c, alltoallv0.c), written anew as one self-checking C program that links
 * the drop-in libmpi.so like any MPI application.  Buffers live in host memory (`host`) or in
 * device memory (`device`: hipMalloc).
 *
 *   usage: mv2run -n N alltoall_suite {host|device} [case ...]
 *
 * Rank 0 prints one line per case ("<mem> <case> <errors>") and a TOTAL line; the exit status is
 * non-zero when any rank counted an error.  Every element names its sender, its receiver and its
 * index, so a block that lands in the wrong place, or comes from the wrong rank, is seen. */
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

/* the k-th int rank `from` sends rank `to` */
static int val(int from, int to, int k) { return from * 1000003 + to * 1009 + k; }
#define UNTOUCHED (-77)

/* one MPI_Alltoallv of ints through operand buffers: hs / hr are the host images of the send and
 * receive buffers (ns / nr ints); hr comes back as the call left it.  sc == NULL: MPI_IN_PLACE. */
static int a2av(const int *hs, int ns, const int *sc, const int *sd, int *hr, int nr, const int *rc, const int *rd) {
    int *s = buf_new((size_t)ns * sizeof(int)), *r = buf_new((size_t)nr * sizeof(int));
    if (ns) buf_set(s, hs, (size_t)ns * sizeof(int));
    buf_set(r, hr, (size_t)nr * sizeof(int));
    const int e = sc ? MPI_Alltoallv(s, sc, sd, MPI_INT, r, rc, rd, MPI_INT, MPI_COMM_WORLD)
                     : MPI_Alltoallv(MPI_IN_PLACE, NULL, NULL, MPI_DATATYPE_NULL, r, rc, rd, MPI_INT, MPI_COMM_WORLD);
    buf_read(hr, r, (size_t)nr * sizeof(int));
    buf_del(s);
    buf_del(r);
    return e;
}

/* alltoall1.c's property: MPI_Alltoall of c ints per pair for c = 1, 2, 4 ... 131072 (512 KiB
 * blocks: past the one-shot kernel's limit), every element checked; then the same in place */
static int t_alltoall1(void) {
    int errs = 0;
    for (int c = 1; c <= 131072; c *= 2) {
        const size_t n = (size_t)c * g_size;
        int *hs = malloc(n * sizeof(int)), *hr = malloc(n * sizeof(int));
        int *s = buf_new(n * sizeof(int)), *r = buf_new(n * sizeof(int));
        for (int pass = 0; pass < 2; ++pass) { /* 0: two buffers, 1: MPI_IN_PLACE */
            for (int j = 0; j < g_size; ++j)
                for (int k = 0; k < c; ++k) hs[(size_t)j * c + k] = val(g_rank, j, k), hr[(size_t)j * c + k] = UNTOUCHED;
            buf_set(s, hs, n * sizeof(int));
            buf_set(r, pass ? hs : hr, n * sizeof(int));
            const int e = pass ? MPI_Alltoall(MPI_IN_PLACE, 0, MPI_DATATYPE_NULL, r, c, MPI_INT, MPI_COMM_WORLD)
                               : MPI_Alltoall(s, c, MPI_INT, r, c, MPI_INT, MPI_COMM_WORLD);
            if (e != MPI_SUCCESS) ++errs;
            buf_read(hr, r, n * sizeof(int));
            for (int j = 0; j < g_size; ++j)
                for (int k = 0; k < c; ++k)
                    if (hr[(size_t)j * c + k] != val(j, g_rank, k) && errs++ < 5)
                        fprintf(stderr, "[%d] alltoall1 c=%d pass %d: block %d element %d is %d\n", g_rank, c, pass, j, k,
                                hr[(size_t)j * c + k]);
        }
        buf_del(s);
        buf_del(r);
        free(hs);
        free(hr);
    }
    return errs;
}

/* alltoallv.c's property: the count of a pair depends on its receiver (rank j is sent j ints by
 * everyone, so rank 0 receives nothing), blocks packed on the send side and spaced on the receive
 * side, the spaces left untouched; then the symmetric matrix (i + j) % 3 in place */
static int t_alltoallv(void) {
    int errs = 0;
    const int n = g_size, me = g_rank;
    int *sc = calloc(n, sizeof(int)), *sd = calloc(n, sizeof(int)), *rc = calloc(n, sizeof(int)), *rd = calloc(n, sizeof(int));
    int ns = 0;
    for (int j = 0; j < n; ++j) {
        sc[j] = j;
        sd[j] = ns;
        ns += j;
        rc[j] = me;
        rd[j] = j * (me + 2); /* two ints of space behind every block */
    }
    const int nr = n * (me + 2);
    int *hs = calloc(ns + 1, sizeof(int)), *hr = calloc(nr + 1, sizeof(int));
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < sc[j]; ++k) hs[sd[j] + k] = val(me, j, k);
    for (int i = 0; i < nr; ++i) hr[i] = UNTOUCHED;
    if (a2av(hs, ns, sc, sd, hr, nr, rc, rd) != MPI_SUCCESS) ++errs;
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < me + 2; ++k) {
            const int want = k < me ? val(j, me, k) : UNTOUCHED;
            if (hr[rd[j] + k] != want && errs++ < 5)
                fprintf(stderr, "[%d] alltoallv: block %d element %d is %d, not %d\n", me, j, k, hr[rd[j] + k], want);
        }
    free(hs);
    free(hr);
    /* in place: the pair (i, j) carries (i + j) % 3 ints either way */
    int tot = 0;
    for (int j = 0; j < n; ++j) {
        rc[j] = (me + j) % 3;
        rd[j] = tot;
        tot += rc[j] + 1; /* one int of space */
    }
    hr = malloc((tot + 1) * sizeof(int));
    for (int i = 0; i < tot; ++i) hr[i] = UNTOUCHED;
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < rc[j]; ++k) hr[rd[j] + k] = val(me, j, k);
    if (a2av(NULL, 0, NULL, NULL, hr, tot, rc, rd) != MPI_SUCCESS) ++errs;
    for (int j = 0; j < n; ++j)
        for (int k = 0; k <= rc[j]; ++k) {
            const int want = k < rc[j] ? val(j, me, k) : UNTOUCHED;
            if (hr[rd[j] + k] != want && errs++ < 5)
                fprintf(stderr, "[%d] alltoallv in place: block %d element %d is %d, not %d\n", me, j, k, hr[rd[j] + k], want);
        }
    free(hr);
    free(sc);
    free(sd);
    free(rc);
    free(rd);
    return errs;
}

/* alltoallv0.c's property: every rank exchanges data with its two ring neighbours only, every
 * other count is 0 (its displacement then points nowhere useful); sizes of both kernels */
static int t_alltoallv0(void) {
    int errs = 0;
    const int n = g_size, me = g_rank, left = (me + n - 1) % n, right = (me + 1) % n;
    const int sizes[3] = {1, 100, 100000};
    int *sc = calloc(n, sizeof(int)), *sd = calloc(n, sizeof(int)), *rc = calloc(n, sizeof(int)), *rd = calloc(n, sizeof(int));
    for (int t = 0; t < 3; ++t) {
        const int c = sizes[t];
        for (int j = 0; j < n; ++j) sc[j] = rc[j] = 0, sd[j] = rd[j] = 1 << 28;
        sc[left] = rc[left] = c;
        sd[left] = rd[left] = 0;
        sc[right] = rc[right] = c; /* n == 2: left == right, one block */
        sd[right] = rd[right] = left == right ? 0 : c;
        int *hs = malloc(2 * (size_t)c * sizeof(int)), *hr = malloc(2 * (size_t)c * sizeof(int));
        for (int k = 0; k < c; ++k) hs[sd[left] + k] = val(me, left, k), hs[sd[right] + k] = val(me, right, k);
        for (int i = 0; i < 2 * c; ++i) hr[i] = UNTOUCHED;
        if (a2av(hs, 2 * c, sc, sd, hr, 2 * c, rc, rd) != MPI_SUCCESS) ++errs;
        for (int k = 0; k < c; ++k) {
            if (hr[rd[left] + k] != val(left, me, k) && errs++ < 5)
                fprintf(stderr, "[%d] alltoallv0 c=%d: from the left, element %d is %d\n", me, c, k, hr[rd[left] + k]);
            if (hr[rd[right] + k] != val(right, me, k) && errs++ < 5)
                fprintf(stderr, "[%d] alltoallv0 c=%d: from the right, element %d is %d\n", me, c, k, hr[rd[right] + k]);
        }
        free(hs);
        free(hr);
    }
    free(sc);
    free(sd);
    free(rc);
    free(rd);
    return errs;
}

static const struct {
    const char *name;
    int (*fn)(void);
} kCases[] = {
    {"alltoall1", t_alltoall1},
    {"alltoallv", t_alltoallv},
    {"alltoallv0", t_alltoallv0},
};

int main(int argc, char **argv) {
    if (argc < 2 || (strcmp(argv[1], "host") && strcmp(argv[1], "device"))) {
        fprintf(stderr, "usage: alltoall_suite {host|device} [case ...]\n");
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
